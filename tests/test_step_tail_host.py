"""CPU tests of tests/step_tail_ref.py, the references the GPU tests of tests/test_gpu_step_tail.py hold the kernels to:

  * every reference against torch in fp64 (autograd for the gradients, torch.optim behind clip_grad_value_ for the rules)
    within 2^-16 of its own bound - the bound's absolute quantities with 2^-40 in place of u = 2^-24;
  * the distance between the kernel's optimizer rule (gain 1 - fl32(beta), exact) and torch's (fl32(1 - beta_double)), per
    element and per state tensor, against the first-order term of the gain difference carried through the recursion;
  * every kernel's arithmetic restated in numpy float32, operation by operation in the kernel's order (two orders for the
    sums), inside its bound with T = 1 (numpy's float32 exp / log / sqrt), and exact on the exact cases;
  * the decision rules restated, and sfh_grad_scale's reference against a brute-force search.

Run with -s for the RATIO lines (largest error / bound per kernel)."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import step_tail_cases as cases
import step_tail_ref as R
from oracle import train_ref

F32 = np.float32
TIGHT = 2.0 ** -16          # 2^-40 / u: the fp64 comparisons use the same absolute quantities


def _report(name, **ratios):
    print(f"RATIO {name}: " + " ".join(f"{k} {v:.3f}" for k, v in ratios.items()))
    assert all(v <= 1.0 for v in ratios.values()), (name, ratios)


def test_longdouble_is_wider_than_double():
    assert np.finfo(np.longdouble).eps <= 2.0 ** -63


ALL_LOSS = cases.loss_cases() + cases.loss_decision_cases()
LOSS_IDS = [c["id"] for c in ALL_LOSS]


def _loss_ref(c, x, **kw):
    lam = c["lam"]
    return R.losses_ref(x["logits"], x["gt"], x["weight"], x["warp"], lam[0], lam[1], c["rec_mse"], lam[2], c["focal"],
                        pre=x["pre"], **kw)


# ------------------------------------------------------------------------------------------------ references against torch
@pytest.mark.parametrize("c", ALL_LOSS, ids=LOSS_IDS)
def test_losses_ref_vs_torch_fp64(c):
    """F.cross_entropy / oracle.train_ref.focal_loss / F.smooth_l1_loss / F.mse_loss with train_ref.per_sample_weighted in fp64
    and their autograd gradients.  The consistency target is handed to torch as the reference's rule gives it (torch raises
    outside [0, nc)); where warp lies in [0, 1) the rule is torch's own (warp * nc).to(long) in fp32.  focal_loss adds its
    1e-6 as a double, so the reference is called with eps_t = 1e-6 here and eps_q = fl32(1e-8) passed to both."""
    x = cases.loss_inputs(c)
    r = _loss_ref(c, x, eps_t=1e-6)
    lam, nc = c["lam"], c["nc"]
    lg = torch.from_numpy(x["logits"]).double().requires_grad_(True)
    gt, w = torch.from_numpy(x["gt"]), torch.from_numpy(x["weight"]).double()
    ce = lambda f: ((lambda a, t: train_ref.focal_loss(a, t, eps=R.FOCAL_EPS_Q)) if f else
                    (lambda a, t: F.cross_entropy(a, t, reduction="none")))
    total = torch.zeros((), dtype=torch.float64)
    want = [0.0, 0.0, 0.0]
    if lam[0] != 0:
        want[0] = train_ref.per_sample_weighted(ce(c["focal"] & 1)(lg, gt), w) * lam[0]
        total = total + want[0]
    wp = None
    if x["warp"] is not None:
        w32 = torch.from_numpy(x["warp"])
        inside = (w32 >= 0) & (w32 < 1)
        assert torch.equal((w32 * nc).to(torch.long)[inside], torch.from_numpy(r["tc"])[inside])
        wp = w32.double().requires_grad_(True)
        gt_f = (gt.float() / float(nc)).double()
        pw = F.mse_loss if c["rec_mse"] else F.smooth_l1_loss
        if lam[1] != 0:
            want[1] = train_ref.per_sample_weighted(pw(wp, gt_f, reduction="none"), w) * lam[1]
            total = total + want[1]
        if lam[2] != 0:
            want[2] = ce(c["focal"] & 2)(lg, torch.from_numpy(r["tc"])).mean() * lam[2]
            total = total + want[2]
    total.backward()
    got = np.array([float(v.detach()) if torch.is_tensor(v) else v for v in want]) + x["pre"]
    dl_got = lg.grad.numpy() if lg.grad is not None else np.zeros(lg.shape)
    ratios = {"loss3": R.ratio(got, r["loss3"], np.maximum(r["b_loss3"] * TIGHT, 4 * R.E53 * np.abs(x["pre"]))),
              "dlogits": R.ratio(dl_got, r["dlogits"], r["b_dlogits"] * TIGHT)}
    if wp is not None and lam[1] != 0:
        ratios["dwarp"] = R.ratio(wp.grad.numpy(), r["dwarp"], r["b_dwarp"] * TIGHT)
    _report(f"losses_ref/torch {c['id']}", **ratios)


@pytest.mark.parametrize("npts", cases.REPROJ_NPTS)
@pytest.mark.parametrize("batch", cases.REPROJ_BATCHES)
def test_reproj_ref_vs_torch_fp64(batch, npts):
    """train_ref.reprojection_loss and its gradient - except at dist == 0, where torch gives NaN and the rule 0"""
    x = cases.reproj_inputs(batch, npts)
    r = R.reproj_ref(x["poi"], x["gt"], x["nz"], x["nn"], x["lam"])
    poi = torch.from_numpy(x["poi"]).double().requires_grad_(True)
    loss = train_ref.reprojection_loss(poi, torch.from_numpy(x["gt"]).double(), torch.from_numpy(x["nz"]).double(),
                                       torch.from_numpy(x["nn"]).double()) * x["lam"]
    loss.backward()
    g = poi.grad.numpy().copy()
    assert np.isnan(g[0, 0]).all() and (r["dpoi"][0, 0] == 0).all()
    g[0, 0] = 0.0
    _report(f"reproj_ref/torch {batch}x{npts}", loss=R.ratio(float(loss.detach()), r["loss"], r["b_loss"] * TIGHT),
            dpoi=R.ratio(g, r["dpoi"], r["b_dpoi"] * TIGHT))


@pytest.mark.parametrize("mse", [0, 1])
@pytest.mark.parametrize("shape,nw", cases.UV_CASES, ids=[str(s) for s, _ in cases.UV_CASES])
def test_uv_ref_vs_torch_fp64(shape, nw, mse):
    """train_ref.per_sample_weighted on the 4-D map AS WRITTEN: the (B,) weights broadcast along the last axis"""
    x = cases.uv_inputs(shape, nw)
    r = R.uv_ref(x["uv"], x["gt"], x["weight"], nw, x["lam"], mse)
    uv = torch.from_numpy(x["uv"]).double().requires_grad_(True)
    fn = F.mse_loss if mse else F.smooth_l1_loss
    loss = train_ref.per_sample_weighted(fn(uv, torch.from_numpy(x["gt"]).double(), reduction="none"),
                                         torch.from_numpy(x["weight"]).double()) * x["lam"]
    loss.backward()
    _report(f"uv_ref/torch {shape}", loss=R.ratio(float(loss.detach()), r["loss"], r["b_loss"] * TIGHT),
            duv=R.ratio(uv.grad.numpy(), r["duv"], r["b_duv"] * TIGHT))


def _run_rule(kind, hp, state, grads, comp=None, u=R.U, dcomp=None, cast=True):
    """the reference recursion over len(grads) steps with the bounds carried; returns [(state, bounds)] per step"""
    out, err = [], None
    for it, g in enumerate(grads):
        state, err = R.opt_step(kind, state, g, hp, step=it + 1, comp=comp, err_in=err, u=u, dcomp=dcomp, cast=cast)
        out.append((state, err))
    return out


@pytest.mark.parametrize("kind", ["rmsprop", "sgd", "adam"])
def test_opt_rule_vs_torch_optim_fp64(kind):
    """torch.optim.RMSprop / SGD / Adam behind clip_grad_value_ on fp64 tensors over three steps, every state tensor after every
    step.  torch's fp64 run takes every scalar as the Python double it is and 1 - beta in double, so the recursion is run
    with cast=False and the gains 1 - beta_double: this holds the recursion, the scalars' roundings are the next test's."""
    hp = dict(cases.DEFAULTS, lr=1e-2, wd=1e-4)
    r = np.random.RandomState(3)
    n = 300
    p0, grads = r.standard_normal(n), [r.standard_normal(n) * 0.2 for _ in range(3)]
    ref = torch.from_numpy(p0.copy()).requires_grad_(True)
    opt = {"rmsprop": lambda: torch.optim.RMSprop([ref], lr=hp["lr"], alpha=hp["alpha"], eps=hp["eps"], weight_decay=hp["wd"],
                                                  momentum=hp["mu"]),
           "sgd": lambda: torch.optim.SGD([ref], lr=hp["lr"], momentum=hp["mu"], weight_decay=hp["wd"]),
           "adam": lambda: torch.optim.Adam([ref], lr=hp["lr"], betas=(hp["b1"], hp["b2"]), eps=hp["eps"],
                                            weight_decay=hp["wd"])}[kind]()
    comp = {"rmsprop": (1 - hp["alpha"],), "sgd": (), "adam": (1 - hp["b1"], 1 - hp["b2"])}[kind]
    state = dict(p=p0, sq=np.zeros(n), buf=np.zeros(n))
    keys = {"rmsprop": ("square_avg", "momentum_buffer"), "sgd": (None, "momentum_buffer"), "adam": ("exp_avg_sq", "exp_avg")}[kind]
    worst = {}
    for it, (st, b) in enumerate(_run_rule(kind, hp, state, grads, comp=comp, u=2.0 ** -40, cast=False)):
        ref.grad = torch.from_numpy(grads[it].copy())
        torch.nn.utils.clip_grad_value_([ref], hp["clip"])
        opt.step()
        ts = opt.state[ref]
        got = {"p": ref.detach().numpy(), "sq": ts[keys[0]].numpy() if keys[0] else st["sq"], "buf": ts[keys[1]].numpy()}
        for k in got:
            worst[k] = max(worst.get(k, 0.0), R.ratio(got[k], st[k], b[k]))
    _report(f"opt_rule/torch.optim {kind}", **worst)


# ------------------------------------------------------------------------------------------------ the two optimizer rules
def gain_difference_ulps(beta):
    """|fl32(1 - beta_double) - (1 - fl32(beta_double))| in ulps of the gain"""
    t, k = F32(1.0 - beta), 1.0 - float(F32(beta))
    return abs(float(t) - k) / float(np.spacing(t))


def test_gain_differences_of_the_default_hyperparameters():
    """alpha 0.99: 10 ulps (relative 9.3e-7); beta1 0.9: 3 ulps (2.2e-7); beta2 0.999: 111 ulps (1.29e-5) - and the kernel's
    own gain 1 - fl32(beta) is exact in fp32"""
    d = {k: gain_difference_ulps(cases.DEFAULTS[k]) for k in ("alpha", "b1", "b2")}
    print("GAIN ulps:", d)
    assert [round(d[k]) for k in ("alpha", "b1", "b2")] == [10, 3, 111]
    for k in ("alpha", "b1", "b2"):
        b = F32(cases.DEFAULTS[k])
        assert float(F32(1.0) - b) == 1.0 - float(b)
        # include/sfh_amd.h: the relative difference of the gain is at most 2^-24 / (1 - beta)
        assert abs(float(F32(1.0 - cases.DEFAULTS[k])) - (1.0 - float(b))) <= R.U * (1.0 - float(b)) / (1.0 - cases.DEFAULTS[k])


def rule_distance_bound(kind, hp, state, grads):
    """per step (kernel-rule state, torch-rule state, bound on their difference): the first-order term of the gain difference
    carried through the recursion (u = 0: no rounding is counted), times 1.01 for the second order"""
    ck, ct = R.complements(kind, hp), R.complements(kind, hp, torch_like=True)
    dc = tuple(abs(a - b) for a, b in zip(ck, ct))
    a = _run_rule(kind, hp, state, grads, comp=ck, u=0.0, dcomp=dc)
    b = _run_rule(kind, hp, state, grads, comp=ct, u=0.0)
    return [(sa, sb, ba) for (sa, ba), (sb, _) in zip(a, b)]


@pytest.mark.parametrize("kind", ["rmsprop", "sgd", "adam"])
def test_distance_between_the_kernel_rule_and_the_torch_rule(kind):
    hp = dict(cases.DEFAULTS, lr=1e-3, wd=1e-4)
    r = np.random.RandomState(4)
    n = 1000
    state = dict(p=r.standard_normal(n).astype(F32), sq=np.zeros(n), buf=np.zeros(n))
    grads = [(r.standard_normal(n) * 0.2).astype(F32) for _ in range(3)]
    worst = {"p": 0.0, "sq": 0.0, "buf": 0.0}
    for sa, sb, b in rule_distance_bound(kind, hp, state, grads):
        for k in worst:
            worst[k] = max(worst[k], R.ratio(sb[k], sa[k], b[k]))
    if kind == "sgd":
        assert all(v == 0.0 for v in worst.values())       # no gain: the two rules are one
    else:
        assert worst["sq"] > 0.5                           # the bound is the distance, not a multiple of it
    _report(f"rule distance {kind}", **worst)


# ------------------------------------------------------------------------------------------------ fp32 restatements
def losses_f32(x, c, reverse=False):
    """train_losses_kernel in numpy float32, operation by operation; `reverse` sums the classes in the other order"""
    lam, nc = [F32(v) for v in c["lam"]], c["nc"]
    l = x["logits"]
    B, _, H, W = l.shape
    N = H * W
    l = l.reshape(B, nc, N)
    order = list(range(nc))[::-1] if reverse else list(range(nc))
    inv = F32(1.0) / (F32(N) * F32(B))
    mx = l.max(axis=1)
    pr = [None] * nc
    se = None
    for k in range(nc):
        pr[k] = np.exp(l[:, k] - mx)
    for k in order:
        se = pr[k] if se is None else se + pr[k]
    lse = np.log(se) + mx
    rs = F32(1.0) / se
    pr = [q * rs for q in pr]
    gt = x["gt"].reshape(B, N)
    wb = x["weight"].reshape(B, 1)
    wv = x["warp"].reshape(B, N) if x["warp"] is not None else np.zeros((B, N), dtype=F32)
    tc = np.minimum(np.maximum((wv * F32(nc)).astype(np.int32), 0), nc - 1)
    dl = [np.zeros((B, N), dtype=F32) for _ in range(nc)]

    def cls(tgt, focal, coef):
        if not focal:
            lt = np.take_along_axis(l, tgt[:, None, :].astype(np.int64), axis=1)[:, 0]
            for k in range(nc):
                dl[k] = dl[k] + coef * (pr[k] - (tgt == k).astype(F32))
            return lse - lt
        dLdp, dot, loss = [None] * nc, None, None
        for k in range(nc):
            q, t = pr[k] + F32(1e-8), (tgt == k).astype(F32) + F32(1e-6)
            om, lg = F32(1.0) - q, np.log(q)
            term = t * (-om * om * lg)
            dLdp[k] = t * (F32(2.0) * om * lg - om * om / q)
            prod = dLdp[k] * pr[k]
            if reverse:
                loss, dot = (term if loss is None else term + loss), (prod if dot is None else prod + dot)
            else:
                loss, dot = (term if loss is None else loss + term), (prod if dot is None else dot + prod)
        for k in range(nc):
            dl[k] = dl[k] + coef * pr[k] * (dLdp[k] - dot)
        return loss

    s = [np.float64(0), np.float64(0), np.float64(0)]
    red = (lambda a: a.astype(np.float64).reshape(-1)[::-1].sum()) if reverse else (lambda a: a.astype(np.float64).sum())
    if lam[0] != 0:
        s[0] = red(wb * cls(gt, c["focal"] & 1, lam[0] * wb * inv))
    if lam[2] != 0:
        s[2] = red(cls(tc, c["focal"] & 2, np.full((B, 1), lam[2] * inv, dtype=F32)))
    dw = None
    if x["warp"] is not None:
        d = wv - gt.astype(F32) / F32(nc)
        ad = np.abs(d)
        if c["rec_mse"]:
            s[1] = red(wb * d * d)
            dw = lam[1] * wb * inv * F32(2.0) * d
        else:
            s[1] = red(wb * np.where(ad < 1, F32(0.5) * d * d, ad - F32(0.5)))
            dw = lam[1] * wb * inv * np.where(ad < 1, d, np.where(d > 0, F32(1.0), F32(-1.0)))
        dw = dw.reshape(B, H, W)
    loss3 = x["pre"] + np.array([s[k] * np.float64(lam[k]) * np.float64(inv) for k in range(3)])
    return dict(dlogits=np.stack(dl, axis=1).reshape(B, nc, H, W), dwarp=dw, loss3=loss3, tc=tc.reshape(B, H, W))


_LOSS_WORST = {}


@pytest.mark.parametrize("reverse", [False, True], ids=["fwd", "rev"])
@pytest.mark.parametrize("c", ALL_LOSS, ids=LOSS_IDS)
def test_losses_restated_in_fp32_stay_inside_the_bound_with_T_1(c, reverse):
    x = cases.loss_inputs(c)
    r = _loss_ref(c, x, t_ulps=1.0)
    with np.errstate(all="ignore"):
        got = losses_f32(x, c, reverse)
    assert got["dlogits"].dtype == F32
    ratios = {"loss3": R.ratio(got["loss3"], r["loss3"], r["b_loss3"]),
              "dlogits": R.ratio(got["dlogits"], r["dlogits"], r["b_dlogits"])}
    if x["warp"] is not None:
        ratios["dwarp"] = R.ratio(got["dwarp"], r["dwarp"], r["b_dwarp"])
        assert np.array_equal(got["tc"], r["tc"])
    for k, v in ratios.items():
        _LOSS_WORST[k] = max(_LOSS_WORST.get(k, 0.0), v)
    _report(f"losses fp32 restatement {c['id']}", **ratios)
    print("WORST losses restatement so far:", _LOSS_WORST)


@pytest.mark.parametrize("nc", [2, 4, 8])
def test_exact_loss_cases_are_exact_in_the_restatement(nc):
    x = cases.loss_exact_inputs(nc)
    for lam, mse in (((2.0, 0.0, 0.0), 0), ((0.0, 0.0, 4.0), 0), ((0.0, 2.0, 0.0), 0), ((0.0, 0.5, 0.0), 1)):
        c = dict(nc=nc, lam=lam, rec_mse=mse, focal=0)
        r = _loss_ref(c, x)
        got = losses_f32(x, c)
        assert np.array_equal(got["dlogits"].astype(np.float64), r["dlogits"])
        assert np.array_equal(got["dwarp"].astype(np.float64), r["dwarp"])
        assert got["loss3"][1] == float(r["loss3"][1])


def test_consistency_target_rule_and_what_the_boundary_cases_tell_apart():
    """the rule trunc(fl32(warp * nc)) against two near misses: the product left in fp64 (differs at a class boundary's lower
    neighbour, where the fp32 product rounds up to the integer) and rintf in place of truncation; neither differs from the
    rule on warp values drawn at random, which is why the boundary cases exist"""
    unrounded = lambda w, nc: np.clip(np.trunc(w.astype(np.float64) * nc), 0, nc - 1).astype(np.int64)
    rint = lambda w, nc: np.clip(np.rint((w * F32(nc)).astype(F32)), 0, nc - 1).astype(np.int64)
    differs = 0
    for nc in range(2, 9):
        w = cases.boundary_warps(nc)
        tc = R.consistency_target(w, nc)
        assert tc.min() == 0 and tc.max() == nc - 1
        assert tc[list(w).index(F32(1.0))] == nc - 1 and tc[-1] == 0 and tc[-2] == 0     # the clamp, -0 and the negative value
        for k in range(nc):
            assert tc[3 * k + 1] == k and tc[3 * k + 2] == k                              # fl32(k / nc) * nc truncates to k
        differs += int((unrounded(w, nc) != tc).any())
        assert (rint(w, nc) != tc).any()
    assert differs > 0
    rnd = np.random.RandomState(0).random_sample(4096).astype(F32)
    assert all(np.array_equal(unrounded(rnd, nc), R.consistency_target(rnd, nc)) for nc in (2, 4, 8))


def reproj_f32(x, reverse=False):
    poi, gt, nz, nn = x["poi"], x["gt"], x["nz"], x["nn"]
    B, n = nz.shape
    sc = (F32(x["lam"]) / (nn * F32(B)))[:, None]
    dx, dy = gt[..., 0] - poi[..., 0], gt[..., 1] - poi[..., 1]
    dist = np.sqrt(dx * dx + dy * dy)
    t = (dist * nz).astype(np.float64)
    s = (t[:, ::-1] if reverse else t).sum(axis=1)
    with np.errstate(all="ignore"):
        g = np.where(dist > 0, nz * sc / dist, F32(0))
    frames = s * sc[:, 0].astype(np.float64)
    return np.stack([-g * dx, -g * dy], axis=2), (frames[::-1] if reverse else frames).sum()


def test_reproj_restated_in_fp32():
    worst = {"loss": 0.0, "dpoi": 0.0}
    for batch in cases.REPROJ_BATCHES:
        for npts in cases.REPROJ_NPTS:
            for kind in ("rand", "none"):
                x = cases.reproj_inputs(batch, npts, kind)
                r = R.reproj_ref(x["poi"], x["gt"], x["nz"], x["nn"], x["lam"], t_ulps=1.0)
                for rev in (False, True):
                    dp, loss = reproj_f32(x, rev)
                    worst["loss"] = max(worst["loss"], R.ratio(loss, r["loss"], r["b_loss"]))
                    worst["dpoi"] = max(worst["dpoi"], R.ratio(dp, r["dpoi"], r["b_dpoi"]))
    x = cases.reproj_exact_inputs()
    r = R.reproj_ref(x["poi"], x["gt"], x["nz"], x["nn"], x["lam"])
    dp, loss = reproj_f32(x)
    assert loss == float(r["loss"]) and np.array_equal(dp[:, x["exact_points"]].astype(np.float64), r["dpoi"][:, x["exact_points"]])
    _report("reproj fp32 restatement", **worst)


def uv_f32(x, nw, mse, reverse=False):
    uv, gt = x["uv"], x["gt"]
    B, C, H, W = uv.shape
    wb = x["weight"] if (nw == W and nw != 1) else np.full(W, x["weight"][0], dtype=F32)
    inv = F32(1.0) / (F32(B) * F32(C) * F32(H) * F32(W))
    lam = F32(x["lam"])
    d = uv - gt
    ad = np.abs(d)
    if mse:
        t, g = wb * d * d, lam * wb * inv * F32(2.0) * d
    else:
        t = wb * np.where(ad < 1, F32(0.5) * d * d, ad - F32(0.5))
        g = lam * wb * inv * np.where(ad < 1, d, np.where(d > 0, F32(1.0), F32(-1.0)))
    t = t.astype(np.float64).reshape(-1)
    return g, (t[::-1] if reverse else t).sum() * np.float64(lam) * np.float64(inv)


def test_uv_restated_in_fp32():
    worst = {"loss": 0.0, "duv": 0.0}
    for shape, nw in cases.UV_CASES + [cases.UV_LARGE]:
        for mse in (0, 1):
            x = cases.uv_inputs(shape, nw)
            r = R.uv_ref(x["uv"], x["gt"], x["weight"], nw, x["lam"], mse)
            for rev in (False, True):
                g, loss = uv_f32(x, nw, mse, rev)
                worst["loss"] = max(worst["loss"], R.ratio(loss, r["loss"], r["b_loss"]))
                worst["duv"] = max(worst["duv"], R.ratio(g, r["duv"], r["b_duv"]))
    _report("uv fp32 restatement", **worst)


def opt_f32(kind, hp, p, sq, buf, g, step):
    """rmsprop_kernel / sgd_kernel / adam_kernel (and sfh_adam_step's two doubles) in numpy float32"""
    h = {k: F32(v) for k, v in hp.items()}
    g = g * h["gscale"]
    if h["clip"] > 0:
        with np.errstate(invalid="ignore"):
            g = np.where(g < -h["clip"], -h["clip"], np.where(g > h["clip"], h["clip"], g))
    g = g + h["wd"] * p
    sq, buf = sq.copy(), buf.copy()
    if kind == "rmsprop":
        sq = h["alpha"] * sq + (F32(1.0) - h["alpha"]) * g * g
        s = g / (np.sqrt(sq) + h["eps"])
        if h["mu"] > 0:
            s = h["mu"] * buf + s
            buf = s
        return p - h["lr"] * s, sq, buf
    if kind == "sgd":
        if h["mu"] > 0:
            g = h["mu"] * buf + g
            buf = g
        return p - h["lr"] * g, sq, buf
    bias1, bias2 = 1.0 - float(h["b1"]) ** step, 1.0 - float(h["b2"]) ** step
    ss, b2s = F32(float(h["lr"]) / bias1), F32(math.sqrt(bias2))
    buf = buf + (F32(1.0) - h["b1"]) * (g - buf)
    sq = h["b2"] * sq + (F32(1.0) - h["b2"]) * g * g
    return p - ss * (buf / (np.sqrt(sq) / b2s + h["eps"])), sq, buf


@pytest.mark.parametrize("cid", list(cases.OPT_CASES))
def test_optimizers_restated_in_fp32_stay_inside_the_bound(cid):
    """one step at a time from the restatement's own previous state, p, sq and buf after every step; untouched state tensors
    come back bit-identical; the NaN gradient of the edge cases poisons p and the touched states, as clamp_ does"""
    x = cases.opt_inputs(cid, sizes=[1, 257, 65537])
    kind, hp = x["kind"], x["hp"]
    worst = {"p": 0.0, "sq": 0.0, "buf": 0.0}
    for t in range(len(x["sizes"])):
        st = dict(p=x["p"][t], sq=x["sq"][t], buf=x["buf"][t])
        for it, gs in enumerate(x["grads"]):
            ref, b = R.opt_step(kind, st, gs[t], hp, step=it + 1)
            with np.errstate(all="ignore"):
                got = dict(zip(("p", "sq", "buf"), opt_f32(kind, hp, st["p"], st["sq"], st["buf"], gs[t], it + 1)))
            for k in worst:
                assert got[k].dtype == F32
                worst[k] = max(worst[k], R.ratio(got[k], ref[k], b[k]))
            if cid.endswith("edges") and x["sizes"][t] == 257 and it == 0:
                assert np.isnan(got["p"][9]) and np.isfinite(got["p"][:9]).all()
            st = got
    _report(f"optimizer fp32 restatement {cid}", **worst)


@pytest.mark.parametrize("cid", list(cases.OPT_EXACT))
def test_exact_optimizer_cases_are_exact(cid):
    x = cases.opt_exact_inputs(cid)
    for t in range(len(x["sizes"])):
        st = dict(p=x["p"][t], sq=x["sq"][t], buf=x["buf"][t])
        for it, gs in enumerate(x["grads"]):
            ref, _ = R.opt_step(x["kind"], st, gs[t], x["hp"], step=it + 1)
            got = dict(zip(("p", "sq", "buf"), opt_f32(x["kind"], x["hp"], st["p"], st["sq"], st["buf"], gs[t], it + 1)))
            for k in got:
                assert np.array_equal(got[k].astype(np.float64), ref[k]), (cid, k, it)
            st = got


# ------------------------------------------------------------------------------------------------ sfh_grad_scale
@pytest.mark.parametrize("case", cases.grad_scale_cases(), ids=[c[0] for c in cases.grad_scale_cases()])
def test_grad_scale_ref_vs_brute_force(case):
    _, heads, theta, shift, over = case
    words = cases.grad_scale_words(heads, theta)
    a = R.grad_scale_ref(words, len(heads), theta is not None, shift, over)
    assert a == R.grad_scale_brute(words, len(heads), theta is not None, shift, over)
    S = a[0]
    assert S.numerator == 1 or S.denominator == 1          # a power of two
    assert float(F32(float(S))) == float(S) and a[0] * a[1] == 1


def test_grad_scale_cases_reach_every_outcome():
    seen = set()
    for _, heads, theta, shift, over in cases.grad_scale_cases():
        S, _, o = R.grad_scale_ref(cases.grad_scale_words(heads, theta), len(heads), theta is not None, shift, over)
        seen.add((o & ~over, S == 1))
        assert o & over == over                            # the word keeps the bits it held
    assert {(2, True), (4, False), (0, True), (0, False)} <= seen


# ------------------------------------------------------------------------------------------------ resize backward
@pytest.mark.parametrize("shape", cases.UP2_SHAPES, ids=str)
def test_up2_bwd_ref_vs_torch_and_restated(shape):
    """the transpose of nn.Upsample(2x, bilinear, align_corners=True) against fp64 autograd, and the kernel's gather restated in
    float32 (fp32 source coordinate and weights, taps added in scan order and in reverse) inside the bound"""
    B, C, H, W = shape
    dy = cases.up2_dy(shape)
    ref, bound = R.up2_bwd_ref(dy)
    x = torch.zeros(B, C, H, W, dtype=torch.float64, requires_grad=True)
    F.interpolate(x, scale_factor=2, mode="bilinear", align_corners=True).backward(torch.from_numpy(dy).double().permute(0, 3, 1, 2))
    ratios = {"torch": R.ratio(x.grad.permute(0, 2, 3, 1).numpy(), ref, bound * TIGHT + 8 * R.E53 * np.abs(ref))}

    def taps(n):
        sc = F32(n - 1) / F32(2 * n - 1) if n > 1 else F32(0)
        out = []
        for o in range(2 * n):
            src = sc * F32(o)
            i0 = min(int(src), n - 1)
            i1 = i0 + (1 if i0 < n - 1 else 0)
            out.append((i0, i1, src - F32(i0)))
        return out

    ty, tx = taps(H), taps(W)
    for rev in (False, True):
        got = np.zeros((B, H, W, C), dtype=F32)
        oys, oxs = (range(2 * H - 1, -1, -1), range(2 * W - 1, -1, -1)) if rev else (range(2 * H), range(2 * W))
        for y in range(H):
            for x_ in range(W):
                for oy in oys:
                    y0, y1, ly = ty[oy]
                    wy = (F32(1) - ly if y0 == y else F32(0)) + (ly if y1 == y else F32(0))
                    if wy == 0:
                        continue
                    for ox in oxs:
                        x0, x1, lx = tx[ox]
                        wx = (F32(1) - lx if x0 == x_ else F32(0)) + (lx if x1 == x_ else F32(0))
                        if wx != 0:
                            got[:, y, x_] = got[:, y, x_] + wy * wx * dy[:, oy, ox]
        ratios["rev" if rev else "fwd"] = R.ratio(got, ref, bound)
    _report(f"up2_bwd {shape}", **ratios)


@pytest.mark.parametrize("shape", cases.NEAREST_SHAPES, ids=str)
def test_nearest_bwd_ref_vs_torch(shape):
    """the transpose of F.interpolate(mode='nearest') against torch's own fp32 backward (both are fp32 sums of the same
    readers: the bound holds between them) and bit for bit on integer-valued dy, where every sum is exact"""
    hs, ws, hd, wd = shape
    for integer in (False, True):
        dy = cases.nearest_dy(shape, integer)
        ref, bound = R.nearest_bwd_ref(dy, hs, ws)
        x = torch.zeros(1, cases.NEAREST_PLANES, hs, ws, requires_grad=True)
        F.interpolate(x, size=(hd, wd), mode="nearest").backward(torch.from_numpy(dy)[None])
        got = x.grad[0].numpy()
        if integer:
            assert np.array_equal(got.astype(np.float64), ref)
        else:
            _report(f"nearest_bwd {shape}", torch=R.ratio(got, ref, bound))
    if (hs, ws) == (hd, wd):
        assert (bound == 0).all()
