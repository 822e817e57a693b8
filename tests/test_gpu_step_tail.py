"""The kernels that open and close a training step (csrc/train_step.hip) one by one against the fp64 CPU references of
tests/step_tail_ref.py (which tests/test_step_tail_host.py holds against torch), through the raw C entry points:

  sfh_train_losses, sfh_reproj_loss, sfh_uv_loss and their _det siblings, sfh_rmsprop_step, sfh_sgd_step, sfh_adam_step,
  sfh_multi_copy, sfh_multi_copy_dscale, sfh_grad_scale

and the two resize backward kernels of csrc/pointwise.hip, sfh_upsample2x_bilinear_nhwc_bwd and sfh_resize_nearest_nchw_bwd.

Conventions of tests/test_gpu_train_kernels.py: every output ends in a guard of 64 sentinel elements that must come back
untouched; an output the kernel overwrites starts as NaN, one it accumulates into (loss3, *loss) starts non-zero and the
reference adds it; every comparison is bit equality or a per-element bound built from the reference's own absolute
quantities (step_tail_ref.py derives each); an element whose bound is zero must be exact.  Each test prints its largest
error / bound (``pytest -s``).  The deterministic siblings must give the element outputs of the plain entries bit for bit
and scalars inside the same bound, with the workspace size their _det_bytes query names.
"""
import math

import numpy as np
import pytest
import torch

import step_tail_cases as cases
import step_tail_ref as R

pytestmark = pytest.mark.gpu

GUARD = 64
SENTINEL = 777.25
NAN = float("nan")
F32 = np.float32


@pytest.fixture(scope="module")
def K():
    """(lib, _ptr, _stream): the raw C entry points"""
    from sfh_amd import _lib
    from sfh_amd.engine import _ptr, _stream
    return _lib.load(), _ptr, _stream


class Guarded:
    """a device buffer of ``shape`` followed by GUARD sentinel elements; ``fill`` is a scalar or a numpy array"""

    def __init__(self, shape, dtype, fill):
        self.n = math.prod(shape)
        self.buf = torch.empty(self.n + GUARD, dtype=dtype, device="cuda")
        self.buf[self.n:] = SENTINEL
        self.guard = self.buf[self.n:].clone()
        self.t = self.buf[:self.n].view(*shape)
        if isinstance(fill, np.ndarray):
            self.t.copy_(torch.from_numpy(np.ascontiguousarray(fill)).to(dtype).reshape(shape))
        else:
            self.t.fill_(fill)

    def result(self):
        """the payload as a numpy array, after checking that the guard is intact"""
        torch.cuda.synchronize()
        assert torch.equal(self.buf[self.n:], self.guard), "the kernel wrote behind its output"
        return self.t.cpu().numpy()


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.itemsize == 4 else np.uint64)


def _same_bits(a, b):
    return np.array_equal(_bits(a), _bits(b))


def _report(name, **ratios):
    print(f"RATIO {name}: " + " ".join(f"{k} {v:.3f}" for k, v in ratios.items()))
    assert all(v <= 1.0 for v in ratios.values()), (name, ratios)


def _workspace(nbytes):
    assert nbytes > 0 and nbytes % 8 == 0
    return torch.full((nbytes // 8,), NAN, dtype=torch.float64, device="cuda")   # a slab element the store pass misses poisons the sum


# ------------------------------------------------------------------------------------------------ sfh_train_losses
def _run_losses(K, c, x, det=False):
    lib, _ptr, _stream = K
    B, H, W = c["shape"] if "shape" in c else x["shape"]
    nc, lam = c["nc"], c["lam"]
    dl = Guarded((B, nc, H, W), torch.float32, NAN)
    dw = Guarded((B, H, W), torch.float32, NAN) if c.get("dwarp", True) and x["warp"] is not None else None
    loss3 = Guarded((3,), torch.float64, x["pre"])
    lg, gt, wt = _dev(x["logits"]), _dev(x["gt"]), _dev(x["weight"])
    wp = _dev(x["warp"]) if x["warp"] is not None else None
    args = [_ptr(lg), _ptr(gt), _ptr(wt), _ptr(wp), nc, B, H, W, lam[0], lam[1], c["rec_mse"], lam[2], c["focal"], _ptr(dl.t),
            _ptr(dw.t) if dw else None, _ptr(loss3.t)]
    if det:
        need = lib.sfh_train_losses_det_bytes(B, H, W)
        ws = _workspace(need)
        rc = lib.sfh_train_losses_det(*args, _ptr(ws), need, _stream())
    else:
        rc = lib.sfh_train_losses(*args, _stream())
    assert rc == 0, lib.sfh_last_error()
    return dict(dlogits=dl.result(), dwarp=dw.result() if dw else None, loss3=loss3.result())


def _check_losses(K, c, x):
    lam = c["lam"]
    r = R.losses_ref(x["logits"], x["gt"], x["weight"], x["warp"], lam[0], lam[1], c["rec_mse"], lam[2], c["focal"], pre=x["pre"])
    got, det = _run_losses(K, c, x), _run_losses(K, c, x, det=True)
    ratios = {"loss3": R.ratio(got["loss3"], r["loss3"], r["b_loss3"]), "det_loss3": R.ratio(det["loss3"], r["loss3"], r["b_loss3"]),
              "dlogits": R.ratio(got["dlogits"], r["dlogits"], r["b_dlogits"])}
    assert _same_bits(det["dlogits"], got["dlogits"])
    if got["dwarp"] is not None:
        ratios["dwarp"] = R.ratio(got["dwarp"], r["dwarp"], r["b_dwarp"])
        assert _same_bits(det["dwarp"], got["dwarp"])
    for k in range(3):                                     # a disabled term leaves its accumulator as it was
        if lam[k] == 0:
            assert got["loss3"][k] == x["pre"][k] and det["loss3"][k] == x["pre"][k]
    _report(f"train_losses {c['id']}", **ratios)
    return got, r


LOSS_CASES = cases.loss_cases()
DECISION_CASES = cases.loss_decision_cases()


@pytest.mark.parametrize("c", LOSS_CASES, ids=[c["id"] for c in LOSS_CASES])
def test_train_losses(K, c):
    """d logits, d warp and the three scalars (onto a loaded loss3) for nc 2 .. 8, CE and focal on each term, SmoothL1 and MSE,
    each lambda zero in turn, without the warp mask and without d warp; logits with a spread of 200, all equal, one at 1e4"""
    _check_losses(K, c, cases.loss_inputs(c))


def test_train_losses_grid_stride(K):
    """525312 pixels: more than 2048 blocks x 256, the grid-stride loop's second trip"""
    c = cases.LOSS_LARGE
    _check_losses(K, c, cases.loss_inputs(c))


@pytest.mark.parametrize("c", DECISION_CASES, ids=[c["id"] for c in DECISION_CASES])
def test_train_losses_decisions(K, c):
    """the consistency target at every class boundary fl32(k / nc), its fp32 neighbours, 1, nextafter(1, 0), a negative value
    and -0: with the consistency term alone d logits is negative on the chosen class and positive on every other, so the
    class is read off the gradient, pixel by pixel.  And SmoothL1 / MSE at d = +-1, their neighbours, 0 and beyond 1."""
    x = cases.loss_inputs(c)
    got, r = _check_losses(K, c, x)
    if c["kind"] == "tc" and not c["focal"]:      # (focal: the +1e-6 on every class can turn a tiny probability's sign)
        neg = got["dlogits"][0, :, 0, :] < 0
        assert (neg.sum(axis=0) == 1).all()
        assert np.array_equal(neg.argmax(axis=0), r["tc"][0, 0])


@pytest.mark.parametrize("nc", [2, 4, 8])
def test_train_losses_exact_cases(K, nc):
    """all logits equal, B * H * W, the lambdas and the weights powers of two: d logits = coef * (1 / nc - onehot) bit for bit
    (segmentation and consistency term in turn); dyadic warp: d warp bit for bit and loss3[1] exact, SmoothL1 and MSE"""
    x = cases.loss_exact_inputs(nc)
    for lam, mse in (((2.0, 0.0, 0.0), 0), ((0.0, 0.0, 4.0), 0), ((0.0, 2.0, 0.0), 0), ((0.0, 0.5, 0.0), 1)):
        c = dict(id=f"exact-nc{nc}", nc=nc, lam=lam, rec_mse=mse, focal=0)
        r = R.losses_ref(x["logits"], x["gt"], x["weight"], x["warp"], lam[0], lam[1], mse, lam[2], 0, pre=x["pre"])
        assert np.array_equal(r["dlogits"].astype(F32).astype(np.float64), r["dlogits"])     # the reference is an fp32 number
        for det in (False, True):
            got = _run_losses(K, c, x, det)
            assert _same_bits(got["dlogits"], r["dlogits"].astype(F32))
            assert _same_bits(got["dwarp"], r["dwarp"].astype(F32))
            assert got["loss3"][1] == float(r["loss3"][1])


# ------------------------------------------------------------------------------------------------ sfh_reproj_loss
def _run_reproj(K, x, pre, det=False):
    lib, _ptr, _stream = K
    B, n = x["nz"].shape
    dp = Guarded((B, n, 2), torch.float32, NAN)
    loss = Guarded((1,), torch.float64, pre)
    a = [_dev(x[k]) for k in ("poi", "gt", "nz", "nn")]
    args = [_ptr(a[0]), _ptr(a[1]), _ptr(a[2]), _ptr(a[3]), B, n, x["lam"], _ptr(dp.t), _ptr(loss.t)]
    if det:
        need = lib.sfh_reproj_loss_det_bytes(B)
        ws = _workspace(need)
        rc = lib.sfh_reproj_loss_det(*args, _ptr(ws), need, _stream())
    else:
        rc = lib.sfh_reproj_loss(*args, _stream())
    assert rc == 0, lib.sfh_last_error()
    return dp.result(), loss.result()[0]


@pytest.mark.parametrize("kind", ["rand", "none"])
@pytest.mark.parametrize("npts", cases.REPROJ_NPTS)
@pytest.mark.parametrize("batch", cases.REPROJ_BATCHES)
def test_reproj_loss(K, batch, npts, kind):
    """lambda * mean_b(sum_n dist nz / num_nonzero) onto a loaded accumulator and d poi, around the 64 frames of a block; a
    point and a whole frame that do not count, no point counting anywhere (loss and gradient exactly zero), and a counted
    point with dist == 0, whose gradient is exactly 0"""
    x = cases.reproj_inputs(batch, npts, kind)
    pre = -2.5
    r = R.reproj_ref(x["poi"], x["gt"], x["nz"], x["nn"], x["lam"], pre=pre)
    dp, loss = _run_reproj(K, x, pre)
    dp_det, loss_det = _run_reproj(K, x, pre, det=True)
    assert _same_bits(dp_det, dp) and (dp[0, 0] == 0).all()
    if kind == "none":
        assert loss == pre and loss_det == pre and not dp.any()
    _report(f"reproj_loss {batch}x{npts} {kind}", loss=R.ratio(loss, r["loss"], r["b_loss"]),
            det_loss=R.ratio(loss_det, r["loss"], r["b_loss"]), dpoi=R.ratio(dp, r["dpoi"], r["b_dpoi"]))


def test_reproj_loss_exact_case(K):
    """Pythagorean coordinate differences, lambda, num_nonzero and batch powers of two: the loss is exact; d poi is exact on
    the two axis-aligned points of every frame (dist a power of two) and inside its bound on the others"""
    x = cases.reproj_exact_inputs()
    r = R.reproj_ref(x["poi"], x["gt"], x["nz"], x["nn"], x["lam"], pre=0.5)
    for det in (False, True):
        dp, loss = _run_reproj(K, x, 0.5, det)
        assert loss == float(r["loss"])
        sl = x["exact_points"]
        assert _same_bits(dp[:, sl], r["dpoi"][:, sl].astype(F32))
        assert R.ratio(dp, r["dpoi"], r["b_dpoi"]) <= 1.0


# ------------------------------------------------------------------------------------------------ sfh_uv_loss
def _run_uv(K, x, shape, nw, mse, pre, det=False):
    lib, _ptr, _stream = K
    B, C, H, W = shape
    duv = Guarded(shape, torch.float32, NAN)
    loss = Guarded((1,), torch.float64, pre)
    a = [_dev(x[k]) for k in ("uv", "gt", "weight")]
    args = [_ptr(a[0]), _ptr(a[1]), _ptr(a[2]), nw, B, C, H, W, x["lam"], mse, _ptr(duv.t), _ptr(loss.t)]
    if det:
        need = lib.sfh_uv_loss_det_bytes(B, C, H, W)
        ws = _workspace(need)
        rc = lib.sfh_uv_loss_det(*args, _ptr(ws), need, _stream())
    else:
        rc = lib.sfh_uv_loss(*args, _stream())
    assert rc == 0, lib.sfh_last_error()
    return duv.result(), loss.result()[0]


def _check_uv(K, shape, nw, mse):
    x = cases.uv_inputs(shape, nw)
    pre = 1.25
    r = R.uv_ref(x["uv"], x["gt"], x["weight"], nw, x["lam"], mse, pre=pre)
    duv, loss = _run_uv(K, x, shape, nw, mse, pre)
    duv_det, loss_det = _run_uv(K, x, shape, nw, mse, pre, det=True)
    assert _same_bits(duv_det, duv)
    _report(f"uv_loss {shape} mse{mse}", loss=R.ratio(loss, r["loss"], r["b_loss"]), det_loss=R.ratio(loss_det, r["loss"], r["b_loss"]),
            duv=R.ratio(duv, r["duv"], r["b_duv"]))


@pytest.mark.parametrize("mse", [0, 1], ids=["SmoothL1", "MSE"])
@pytest.mark.parametrize("shape,nw", cases.UV_CASES, ids=[str(s) for s, _ in cases.UV_CASES])
def test_uv_loss(K, shape, nw, mse):
    """the header's rule (weights along the last axis, nweights in {1, W}), both criteria, differences at +-1 and their
    neighbours; one element; nweights = W = B"""
    _check_uv(K, shape, nw, mse)


def test_uv_loss_grid_stride(K):
    """262654 elements: above 1024 blocks x 256"""
    _check_uv(K, *cases.UV_LARGE, 0)


def test_uv_loss_refusals(K):
    """a weight count that cannot broadcast along the last axis is refused and nothing is written"""
    lib, _ptr, _stream = K
    shape = (3, 2, 5, 4)
    x = cases.uv_inputs(shape, 3)
    duv, loss = Guarded(shape, torch.float32, NAN), Guarded((1,), torch.float64, 1.25)
    a = [_dev(x[k]) for k in ("uv", "gt", "weight")]
    for nw in (3, 5, 0):
        assert lib.sfh_uv_loss(_ptr(a[0]), _ptr(a[1]), _ptr(a[2]), nw, *shape, 2.0, 1, _ptr(duv.t), _ptr(loss.t), _stream()) != 0
    assert np.isnan(duv.result()).all() and loss.result()[0] == 1.25


# ------------------------------------------------------------------------------------------------ optimizers
class OptTable:
    """p, g, sq, buf per tensor (each guarded) and the device tables, chunks as TrainStep._init_optimizer builds them"""

    def __init__(self, x):
        self.sizes = x["sizes"]
        self.t = {k: [Guarded((n,), torch.float32, a) for n, a in zip(self.sizes, x[k])] for k in ("p", "sq", "buf")}
        self.t["g"] = [Guarded((n,), torch.float32, NAN) for n in self.sizes]
        tab = np.array([[self.t[k][i].t.data_ptr() for k in ("p", "g", "sq", "buf")] for i in range(len(self.sizes))], dtype=np.int64)
        self.table = _dev(tab.view(np.uint8).reshape(-1))
        ch, self.nchunks = cases.chunk_table(self.sizes)
        self.chunks = _dev(ch)

    def set_grads(self, gs):
        for dst, g in zip(self.t["g"], gs):
            dst.t.copy_(torch.from_numpy(g))

    def state(self, i):
        return {k: self.t[k][i].result() for k in ("p", "sq", "buf")}


def _opt_call(K, tb, kind, hp, step):
    lib, _ptr, _stream = K
    if kind == "rmsprop":
        return lib.sfh_rmsprop_step(_ptr(tb.table), _ptr(tb.chunks), tb.nchunks, hp["lr"], hp["alpha"], hp["eps"], hp["wd"], hp["mu"],
                                    hp["clip"], hp["gscale"], _stream())
    if kind == "sgd":
        return lib.sfh_sgd_step(_ptr(tb.table), _ptr(tb.chunks), tb.nchunks, hp["lr"], hp["wd"], hp["mu"], hp["clip"], hp["gscale"],
                                _stream())
    return lib.sfh_adam_step(_ptr(tb.table), _ptr(tb.chunks), tb.nchunks, hp["lr"], hp["b1"], hp["b2"], hp["eps"], hp["wd"], hp["clip"],
                             hp["gscale"], step, _stream())


@pytest.mark.parametrize("cid", list(cases.OPT_CASES))
def test_optimizer_steps(K, cid):
    """three steps over tensors of 1, 255, 256, 257, 65536, 65537 and 70001 elements; p, sq and buf of every tensor after every
    step against the fp64 rule started from the kernel's own previous state (step_tail_ref.opt_step gives the bound per
    element and state tensor).  A state tensor the rule does not touch (buf at mu = 0, sq for SGD) starts as a sentinel and
    comes back bit-identical; the gradients are not written.  The edge cases: gradients at +-clip / gscale and one ulp beyond,
    0, -0, +-inf (-> +-clip) and NaN, which must poison p and the touched states as clamp_ does."""
    x = cases.opt_inputs(cid)
    kind, hp = x["kind"], x["hp"]
    tb = OptTable(x)
    prev = [dict(p=x["p"][i], sq=x["sq"][i], buf=x["buf"][i]) for i in range(len(x["sizes"]))]
    worst = {"p": 0.0, "sq": 0.0, "buf": 0.0}
    for it, gs in enumerate(x["grads"]):
        tb.set_grads(gs)
        assert _opt_call(K, tb, kind, hp, it + 1) == 0
        for i, n in enumerate(x["sizes"]):
            got = tb.state(i)
            ref, b = R.opt_step(kind, prev[i], gs[i], hp, step=it + 1)
            for k in worst:
                if (b[k] == 0).all() and np.array_equal(ref[k], R.f64(prev[i][k])):
                    assert _same_bits(got[k], prev[i][k]), (cid, k, n, "an untouched state tensor changed")
                worst[k] = max(worst[k], R.ratio(got[k], ref[k], b[k]))
            assert _same_bits(tb.t["g"][i].result(), gs[i])
            if cid.endswith("edges") and n == 257:
                assert np.isnan(got["p"][9]) and np.isfinite(got["p"][:9]).all() and np.isfinite(got["p"][10:]).all()
            prev[i] = got
    _report(f"optimizer {cid}", **worst)


@pytest.mark.parametrize("cid", list(cases.OPT_EXACT))
def test_optimizer_exact_cases(K, cid):
    """hyperparameters powers of two, dyadic p and g, states chosen so that every square root and quotient is exact: all three
    tensors bit-equal to the fp64 rule after every step"""
    x = cases.opt_exact_inputs(cid)
    tb = OptTable(x)
    prev = [dict(p=x["p"][i], sq=x["sq"][i], buf=x["buf"][i]) for i in range(len(x["sizes"]))]
    for it, gs in enumerate(x["grads"]):
        tb.set_grads(gs)
        assert _opt_call(K, tb, x["kind"], x["hp"], it + 1) == 0
        for i in range(len(x["sizes"])):
            got = tb.state(i)
            ref, _ = R.opt_step(x["kind"], prev[i], gs[i], x["hp"], step=it + 1)
            for k in got:
                assert np.array_equal(ref[k].astype(F32).astype(np.float64), ref[k])
                assert _same_bits(got[k], ref[k].astype(F32)), (cid, k, it)
            prev[i] = got


def test_adam_refuses_step_zero(K):
    """Adam's step counter starts at 1; a refused call writes nothing"""
    x = cases.opt_inputs("adam-defaults", sizes=[257])
    tb = OptTable(x)
    tb.set_grads(x["grads"][0])
    assert _opt_call(K, tb, "adam", x["hp"], 0) != 0
    assert all(_same_bits(tb.state(0)[k], x[k][0]) for k in ("p", "sq", "buf"))


# ------------------------------------------------------------------------------------------------ sfh_multi_copy
def _copy_tables(srcs):
    """device storages, guarded NaN destinations and the two tables for a list of cases.copy_sources() entries"""
    stor, dsts, rows, sizes = [], [], [], []
    for _, storage, off, shape, strides, is_int in srcs:
        s = Guarded((len(storage),), torch.int32 if is_int else torch.float32, storage)   # the guard is slack behind the source
        n = math.prod(shape)
        d = Guarded((n,), torch.int32 if is_int else torch.float32, -1 if is_int else NAN)
        sh = (1,) * (4 - len(shape)) + tuple(shape)
        st = (0,) * (4 - len(strides)) + tuple(strides)
        rows.append([d.t.data_ptr(), s.t.data_ptr() + 4 * off, sh[1] | (sh[2] << 32), sh[3], *st])
        stor.append(s); dsts.append(d); sizes.append(n)
    ch, nchunks = cases.chunk_table(sizes)
    return stor, dsts, _dev(np.array(rows, dtype=np.int64).view(np.uint8).reshape(-1)), _dev(ch), nchunks


def _gather(storage, off, shape, strides):
    return np.lib.stride_tricks.as_strided(storage[off:], shape=shape, strides=[4 * s for s in strides]).reshape(-1).copy()


@pytest.mark.parametrize("dscale", [False, True], ids=["scale", "dscale"])
@pytest.mark.parametrize("scale", [1.0] + cases.COPY_SCALES)
def test_multi_copy(K, scale, dscale):
    """a gather, bit for bit: a contiguous tensor, the permuted (M, N, k, k) weight-gradient view of an [m][tap][n] buffer, a
    view with a storage offset, one element, 65537 words (a second chunk of one) and - at scale 1, where the words are moved
    untouched - an int32 tensor with NaN payloads and -0.  scale != 1: one multiply, correctly rounded, float tensors only.
    The same table through the device scalar of sfh_multi_copy_dscale.  The sources come back untouched."""
    lib, _ptr, _stream = K
    srcs = [s for s in cases.copy_sources() if not s[5] or (scale == 1.0 and not dscale)]
    stor, dsts, table, chunks, nchunks = _copy_tables(srcs)
    if dscale:
        sd = _dev(np.array([scale], dtype=F32))
        assert lib.sfh_multi_copy_dscale(_ptr(table), _ptr(chunks), nchunks, _ptr(sd), _stream()) == 0
    else:
        assert lib.sfh_multi_copy(_ptr(table), _ptr(chunks), nchunks, scale, _stream()) == 0
    for (name, storage, off, shape, strides, is_int), s, d in zip(srcs, stor, dsts):
        want = _gather(storage, off, shape, strides)
        if scale != 1.0 or dscale:
            want = want * F32(scale)
        assert _same_bits(d.result(), want), (name, scale, dscale)
        assert _same_bits(s.result(), storage), name


# ------------------------------------------------------------------------------------------------ sfh_grad_scale
GS_CASES = cases.grad_scale_cases()


@pytest.mark.parametrize("case", GS_CASES, ids=[c[0] for c in GS_CASES])
def test_grad_scale(K, case):
    """S, 1 / S and the overflow word against the header's rule restated on the bit patterns: heads only, theta only, both; the
    largest head at 2^e exactly and one ulp below (the frexpf edge); shift -3, 0, 6; theta raised, at the limit, refused
    (bit 4, S unchanged); NaN and Inf words (bit 2, S = 1); all-zero words (S = 1); the word keeps the bits it held"""
    lib, _ptr, _stream = K
    _, heads, theta, shift, over = case
    words = cases.grad_scale_words(heads, theta)
    S, Sinv, o = R.grad_scale_ref(words, len(heads), theta is not None, shift, over)
    wd = _dev(words.view(np.int32))
    s2 = Guarded((2,), torch.float32, NAN)
    ov = Guarded((1,), torch.int32, over)
    assert lib.sfh_grad_scale(_ptr(wd), len(heads), 1 if theta is not None else 0, shift, _ptr(s2.t), _ptr(ov.t), _stream()) == 0
    got = s2.result()
    assert _same_bits(got, np.array([float(S), float(Sinv)], dtype=F32)) and float(got[0]) * float(got[1]) == 1.0
    assert int(ov.result()[0]) == o
    assert _same_bits(wd.cpu().numpy(), words.view(np.int32))


# ------------------------------------------------------------------------------------------------ resize backward
@pytest.mark.parametrize("shape", cases.UP2_SHAPES, ids=str)
def test_upsample2x_bilinear_bwd(K, shape):
    """dx (B,H,W,C) = the transpose of the 2x bilinear (align_corners) map applied to dy (B,2H,2W,C): one pixel, a single row,
    C = 12 (no multiple of 8).  H = W = 1: all four weights are 1 and an integer-valued dy gives the exact sum."""
    lib, _ptr, _stream = K
    B, C, H, W = shape
    for integer in (False, True):
        dy = cases.up2_dy(shape, integer)
        ref, bound = R.up2_bwd_ref(dy)
        dx = Guarded((B, H, W, C), torch.float32, NAN)
        dyc = _dev(dy)
        assert lib.sfh_upsample2x_bilinear_nhwc_bwd(_ptr(dyc), _ptr(dx.t), B, H, W, C, _stream()) == 0
        got = dx.result()
        if integer and H == 1 and W == 1:
            assert np.array_equal(got.astype(np.float64), ref)
        _report(f"upsample2x_bwd {shape} int{int(integer)}", dx=R.ratio(got, ref, bound))


def test_upsample2x_bilinear_bwd_refuses_channels_off_the_quad(K):
    """the launcher moves four channels per thread: C = 6 is refused and nothing is written"""
    lib, _ptr, _stream = K
    dx = Guarded((1, 2, 2, 6), torch.float32, NAN)
    dy = torch.ones(1, 4, 4, 6, device="cuda")
    assert lib.sfh_upsample2x_bilinear_nhwc_bwd(_ptr(dy), _ptr(dx.t), 1, 2, 2, 6, _stream()) != 0
    assert np.isnan(dx.result()).all()


@pytest.mark.parametrize("shape", cases.NEAREST_SHAPES, ids=str)
def test_resize_nearest_bwd(K, shape):
    """dx (planes,hs,ws) = the sum of dy over the destination pixels that read each source pixel (F.interpolate 'nearest'):
    up, down, odd ratios, the identity (bound zero: a copy), an exact 2x and an exact 1/2; bit for bit on an integer-valued
    dy, where every sum is exact"""
    lib, _ptr, _stream = K
    hs, ws, hd, wd = shape
    P = cases.NEAREST_PLANES
    for integer in (False, True):
        dy = cases.nearest_dy(shape, integer)
        ref, bound = R.nearest_bwd_ref(dy, hs, ws)
        dx = Guarded((P, hs, ws), torch.float32, NAN)
        dyc = _dev(dy)
        assert lib.sfh_resize_nearest_nchw_bwd(_ptr(dyc), _ptr(dx.t), P, hs, ws, hd, wd, _stream()) == 0
        got = dx.result()
        if integer:
            assert np.array_equal(got.astype(np.float64), ref)
        _report(f"resize_nearest_bwd {shape} int{int(integer)}", dx=R.ratio(got, ref, bound))
