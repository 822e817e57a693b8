"""CPU checks of the validation scoring (sfh_amd.evaluation, eval.py:142-234): the host-side division of the accumulated
sums, its all-reduce over two gloo ranks, and the argument checks of the new C entries."""
import math
import os

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp


def _batches(seed, n=5):
    """synthetic per-batch values as the device accumulates them: per-batch means of seg / rec / uv / consist, per-frame
    sums of the reprojection errors, the frame count"""
    g = torch.Generator().manual_seed(seed)
    out = []
    for _ in range(n):
        B = int(torch.randint(1, 17, (1,), generator=g))
        out.append({"seg": float(torch.rand(1, generator=g, dtype=torch.float64)) * 2,
                    "rec": float(torch.rand(1, generator=g, dtype=torch.float64)) * 0.1,
                    "uv": float(torch.rand(1, generator=g, dtype=torch.float64)),
                    "consist": float(torch.rand(1, generator=g, dtype=torch.float64)) * 3,
                    "reproj": float(torch.rand(1, generator=g, dtype=torch.float64)) * B,
                    "reproj_px": float(torch.rand(1, generator=g, dtype=torch.float64)) * B * 300,
                    "frames": B})
    return out


def _accumulate(batches, n_val):
    from sfh_amd import evaluation as ev
    acc = torch.zeros(ev.SLOTS, dtype=torch.float64)
    acc[ev.NBATCH] = n_val
    for b in batches:
        acc[ev.SEG] += b["seg"]
        acc[ev.REC] += b["rec"]
        acc[ev.UV] += b["uv"]
        acc[ev.CONSIST] += b["consist"]
        acc[ev.REPROJ] += b["reproj"]
        acc[ev.REPROJ_PX] += b["reproj_px"]
        acc[ev.FRAMES] += b["frames"]
    return acc


def _reference_arithmetic(batches):
    """eval.py:144-225 with the per-batch values given: running sums, then / n_val and / counter"""
    ce = rec = uv = rp = rpx = cons = 0
    counter = 0
    for b in batches:
        counter += b["frames"]
        ce += b["seg"]
        rec += b["rec"]
        uv += b["uv"]
        cons += b["consist"]
        rp += b["reproj"]
        rpx += b["reproj_px"]
    n_val = len(batches)
    return {'val_seg_score': ce / n_val, 'val_rec_score': rec / n_val, 'val_uv_score': uv / n_val,
            'val_reproj_score': rp / counter, 'val_reproj_px': rpx / counter, 'val_consist_score': cons / n_val}


def test_scores_from_accumulator_matches_reference_arithmetic():
    from sfh_amd import evaluation as ev
    batches = _batches(5)
    got = ev.scores_from_accumulator(_accumulate(batches, len(batches)))
    want = _reference_arithmetic(batches)
    assert set(got) == set(want)
    for k in want:
        assert isinstance(got[k], float)
        assert math.isclose(got[k], want[k], rel_tol=1e-14), (k, got[k], want[k])


def test_scores_from_accumulator_rejects_the_error_flag_and_empty_counts():
    from sfh_amd import evaluation as ev
    acc = _accumulate(_batches(6), 5)
    acc[ev.BAD] = 2.0
    with pytest.raises(ValueError, match="mask"):
        ev.scores_from_accumulator(acc)
    with pytest.raises(ValueError, match="no batch"):
        ev.scores_from_accumulator([0.0] * ev.SLOTS)
    with pytest.raises(ValueError):
        ev.scores_from_accumulator([0.0] * (ev.SLOTS - 1))


def test_empty_loader_raises_before_any_device_work():
    from sfh_amd import evaluation as ev

    class Net:
        mask_classes, use_unet, use_resnet, warper, unet_uv, warp_size = 4, True, True, True, False, (640, 360)
    with pytest.raises(ValueError, match="empty"):
        ev.eval_reconstructor(Net(), [], "cuda", (640, 360))
    with pytest.raises(ValueError, match="warp_size"):
        ev.eval_reconstructor(Net(), [{}], "cuda", (320, 180))


def _worker(rank, world, port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from sfh_amd import evaluation as ev, sharding
        batches = _batches(7, n=6)
        mine = batches[rank::world]                # DistributedSampler-style shard: every other batch
        acc = _accumulate(mine, len(mine))
        sharding.allreduce_scores(acc)
        q.put((rank, ev.scores_from_accumulator(acc)))
        dist.barrier()
    finally:
        dist.destroy_process_group()


def test_two_gloo_ranks_give_the_single_process_scores():
    from sfh_amd import evaluation as ev
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 29500 + (os.getpid() % 2000) + 131
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = [q.get(timeout=120) for _ in range(2)]
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    batches = _batches(7, n=6)
    want = ev.scores_from_accumulator(_accumulate(batches, len(batches)))
    for _, got in res:
        for k in want:
            assert math.isclose(got[k], want[k], rel_tol=1e-12), (k, got[k], want[k])


def test_allreduce_scores_without_a_process_group_is_the_identity():
    from sfh_amd import sharding
    v = torch.arange(9, dtype=torch.float64)
    assert sharding.allreduce_scores(v) is v and torch.equal(v, torch.arange(9, dtype=torch.float64))


def test_eval_entries_reject_bad_arguments_without_gpu():
    import ctypes
    from sfh_amd import _lib
    lib = _lib.load()
    assert lib.sfh_eval_workspace_doubles(16, 360, 640) == 5 * 16 * 360 + 7 * 16
    assert lib.sfh_eval_workspace_doubles(0, 360, 640) == -1
    assert lib.sfh_eval_workspace_doubles(4, 0, 640) == -1
    assert lib.sfh_eval_workspace_doubles(70000, 8, 8) == -1
    fake = ctypes.c_void_p(0x1000)     # never dereferenced: every call below fails its argument checks first
    args = dict(logits=fake, mask=fake, warp=fake, weight=None, nc=4, B=2, H=8, W=8, poi=None, gt=None, nz=None, nnz=None,
                npts=0, tw=8.0, th=8.0, ws=fake, flag=fake, acc=fake)

    def call(**kw):
        a = dict(args, **kw)
        return lib.sfh_eval_batch(a["logits"], a["mask"], a["warp"], a["weight"], a["nc"], a["B"], a["H"], a["W"], a["poi"],
                                  a["gt"], a["nz"], a["nnz"], a["npts"], a["tw"], a["th"], a["ws"], a["flag"], a["acc"], None)
    assert call(ws=None) == -1 and b"null" in lib.sfh_last_error()
    assert call(flag=None) == -1
    assert call(acc=None) == -1
    assert call(mask=None) == -1 and b"mask" in lib.sfh_last_error()
    assert call(nc=9) == -1 and b"nc=9" in lib.sfh_last_error()
    assert call(nc=0) == -1
    assert call(B=0) == -1 and b"geometry" in lib.sfh_last_error()
    assert call(H=-1) == -1
    assert call(B=70000) == -1
    assert call(poi=fake) == -1 and b"poi" in lib.sfh_last_error()           # poi without gt / nonzeros / counts
    assert call(poi=fake, gt=fake, nz=fake, nnz=fake, npts=0) == -1
    with pytest.raises(ValueError):
        _lib.check(call(nc=9), "eval_batch")
