"""DDP_USER_FITTED_WAVE on the GPU: ddp_user_rollout_fit_wave against the long double reference of tests/fitted_reference.py at the
shapes of tests/fitted_wave_cases.py, its bit rules, and kl.iLQGkl(..., fitted=True, wide=True) and cost_model= with wide=True against
oracle.np_kl.iLQGkl on the tables and against the DDP_KL_HOSTLOOP=1 twin.  Tolerance 1e-8 relative per time step (conftest.relerr)
against a reference, 1e-12 between two runs of the same kernels; "the same bits" is array_equal on the bit patterns."""
import ctypes as C

import numpy as np
import pytest

import fitted_reference as fr
import fitted_wave_cases as fw
import kl_wide_cases as kc
from conftest import relerr
from test_gpu_user_problem import PEND_P, car_params, lq_params, pend_params
from test_user_wave_cpu import CHAIN_P, lq_nparam

pytestmark = pytest.mark.gpu
RTOL = fw.RTOL
KERNEL = "ddp_user_rollout_fit_wave"
WIDE = "back_pass_gps_wide"


@pytest.fixture(scope="module")
def ddp():
    import ddp_amd
    import ddp_amd.kl  # noqa: F401
    ddp_amd.default_handle()
    return ddp_amd


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def same(a, b):
    return all(x.shape == y.shape and np.array_equal(bits(x), bits(y)) for x, y in zip(a, b))


_problems = {}


def _problem(ddp, shape):
    if shape not in _problems:
        ex, n, m, kw, _ = fw.SHAPES[shape]
        nparam = 7 if ex.startswith("chain") else lq_nparam(n, m)
        _problems[shape] = ddp.DeviceProblem(ddp.example_source(ex), n, m, nparam=nparam, wave=True, fitted_wave=True, **kw)
    return _problems[shape]


def _run(ddp, prob, c, sl=slice(None), tables=None):
    fx, fu, fc = tables or (c["fx"], c["fu"], c["fc"])
    pol = ddp.GaussianPolicy(c["N"], c["n"], c["m"], c["K"][..., sl], c["k"][..., sl], None, None) if c["closed"] else None
    P = c["P"][:, sl] if c["P"].ndim == 2 else c["P"]
    return ddp.forward_pass(pol, c["x0"][:, sl], c["u"][..., sl], c["x"][..., sl] if c["closed"] else None, c["al"], prob, c["lims"], params=P,
                            model=(fx[..., sl], fu[..., sl], fc[..., sl]))


def _dev_run(ddp, prob, c, active=None, fill=-7.0):
    """the `_dev` entry on uploaded arrays; outputs start as `fill`.  Returns xnew, unew, cnew, csum"""
    h, L = ddp.default_handle(), ddp._lib.lib()
    n, m, N, B, na = c["n"], c["m"], c["N"], c["B"], len(c["al"])
    CL = prob.cost_len(N)
    shapes = [(n, N, B, na), (m, N, B, na), (CL, B, na), (B, na)]
    ins = [h.to_device(np.asfortranarray(a)) for a in (c["P"], c["K"], c["k"], c["x0"], c["u"], c["x"], c["fx"], c["fu"], c["fc"])]
    lim = None if c["lims"] is None else h.to_device(np.asfortranarray(c["lims"]))
    act = None if active is None else h.to_device(np.ascontiguousarray(active, dtype=np.int32))
    outs = [h.to_device(np.full(s, fill, order="F")) for s in shapes]
    dP, dK, dk, dx0, du, dx, dfx, dfu, dfc = ins
    if not c["closed"]:
        dK = dk = dx = None
    try:
        ddp._lib.check(L.ddp_user_rollout_fit_f64_dev(h.raw, prob._ptr(h), N, B, dP, int(c["P"].ndim == 2), dK, dk, dx0, du, dx,
                                                      c["al"].ctypes.data_as(C.c_void_p), na, lim, act, dfx, dfu, dfc, *outs))
        h.sync()
        res = [h.to_host(p, s) for p, s in zip(outs, shapes)]
    finally:
        for p in ins + outs + [q for q in (lim, act) if q is not None]:
            h.free(p)
    return res


# 1. ------------------------------------------------------------------------------------------ the rollout contract against long double
@pytest.mark.parametrize("shape,ci", fw.ROLLOUTS, ids=["%s-B%dxa%d-N%d" % ((s,) + fw.COMBOS[ci][:3]) for s, ci in fw.ROLLOUTS])
def test_rollout_matches_long_double(ddp, shape, ci):
    """xnew, unew, cnew at 1e-8 per time step; csum the in-order sum of cnew; the limits hold; NaN in slot N - 1 of the tables changes no
    bit; with N = 1 all-NaN tables give finite results.  The rows per shape are the covering table of fitted_wave_cases.COMBOS, not the
    full product of (B, nalpha), N, policy and parameter kind (what is left out is listed there).
    Measured worst relerr over the 25 cases on one MI355X: see the README row of DDP_USER_FITTED_WAVE."""
    c, prob = fw.rollout_case(shape, ci), _problem(ddp, shape)
    N, B, na = c["N"], c["B"], len(c["al"])
    xr, ur, cr = fw.rollout_reference(c)
    xg, ug, cg = _run(ddp, prob, c)
    assert ddp.default_handle().last_kernel(1) == KERNEL
    worst = [0.0, 0.0, 0.0]
    for b in range(B):
        for a in range(na):
            e = (relerr(xg[..., b, a], xr[..., b, a]), relerr(ug[..., b, a], ur[..., b, a]), relerr(cg[:, b, a], cr[:, b, a], 0))
            worst = [max(w, v) for w, v in zip(worst, e)]
    print("%s B=%d nalpha=%d N=%d: worst relerr x %.2e u %.2e c %.2e" % (shape, B, na, N, *worst))
    assert max(worst) < RTOL, worst
    if c["lims"] is not None:
        assert np.all(ug >= c["lims"][:, 0, None, None, None]) and np.all(ug <= c["lims"][:, 1, None, None, None])
    # csum against the in-order sum of the kernel's own cnew taken in long double: the kernel adds c_i in that order, but the compiler may
    # fuse the last multiply-add of the user's cost into the addition, so the bits of a float64 sum of the stored c_i are not promised.
    # Every cost here is non-negative: CL additions in float64 err by at most CL 2^-53 of the sum each way, 2^-52 CL is the bound
    xd, ud, cd, sd = _dev_run(ddp, prob, c)
    assert same((xd, ud, cd), (xg, ug, cg))
    acc = np.zeros((B, na), np.longdouble)
    for t in range(cd.shape[0]):
        acc = acc + cd[t].astype(np.longdouble)
    cerr = float(np.max(np.abs(sd - acc) / acc))
    print("csum against the long double sum of cnew: %.2e (bound %.2e)" % (cerr, cd.shape[0] * 2.0 ** -52))
    assert cerr <= cd.shape[0] * 2.0 ** -52
    # NaN in slot N - 1 of all three tables; with N = 1 that is every entry
    nan_t = tuple(a.copy() for a in (c["fx"], c["fu"], c["fc"]))
    for a in nan_t:
        a[..., N - 1, :] = np.nan
    got = _run(ddp, prob, c, tables=nan_t)
    assert same(got, (xg, ug, cg))
    if N == 1:
        assert all(np.all(np.isnan(a)) for a in nan_t) and all(np.all(np.isfinite(a)) for a in got)


# 2. --------------------------------------------------------------------------------------------------------------------- mask and bits
@pytest.mark.parametrize("shape,ci", [("lq_33x2", 3), ("lq_10x9", 0), ("chain_64x32", 0), ("chain_34x17", 3)])
def test_mask_and_bit_rules(ddp, shape, ci):
    """NULL and all-ones `active` give the same bits; under a mask with holes the inactive rows of all four outputs keep the sentinel and
    the active rows their bits; two calls, a slice of the trajectories and the host entry against the `_dev` entry give the same bits"""
    c, prob = fw.rollout_case(shape, ci), _problem(ddp, shape)
    B = c["B"]
    full = _dev_run(ddp, prob, c)
    assert ddp.default_handle().last_kernel(1) == KERNEL
    assert same(_dev_run(ddp, prob, c, active=np.ones(B, np.int32)), full)
    assert same(_dev_run(ddp, prob, c), full)
    host = _run(ddp, prob, c)
    assert same(host, full[:3])
    act = (np.arange(B) % 3 != 1).astype(np.int32)
    sent = np.float64(-7.0)
    part = _dev_run(ddp, prob, c, active=act, fill=sent)
    for got, ref in zip(part, full):
        assert np.array_equal(bits(got[..., act == 1, :]), bits(ref[..., act == 1, :]))
        assert np.all(bits(got[..., act == 0, :]) == bits(np.array([sent]))[0])
    sl = slice(1, min(3, B)) if B > 1 else slice(0, 1)
    assert same(_run(ddp, prob, c, sl), [a[..., sl, :] for a in host])


# 3. ---------------------------------------------------------------------------------------------------- terminal cost and wrapped diff
def test_terminal_cost_and_wrapped_diff(ddp):
    """pendcart_ad 4x1 as a wave problem with WrappedDiff(0): nominal angles whole turns away, so that the difference crosses ±π"""
    n, m, N, B = 4, 1, 33, 4
    rng = np.random.default_rng(5033)
    prob = ddp.DeviceProblem(ddp.example_source("pendcart_ad"), n, m, nparam=25, terminal=True, autodiff=True, diff=ddp.WrappedDiff(0),
                             wave=True, fitted_wave=True)
    fx, fu, fc = fr.designed_tables(rng, n, m, N, B)
    x0, u, x = rng.standard_normal((n, B)), 0.3 * rng.standard_normal((m, N, B)), rng.standard_normal((n, N, B))
    x[0] += 2 * np.pi * rng.integers(-2, 3, (N, B))
    K, k = 0.1 * rng.standard_normal((m, n, N, B)), 0.2 * rng.standard_normal((m, N, B))
    al = np.concatenate([[1.0], 10.0 ** np.linspace(-0.3, -3, 10)])
    P = np.asfortranarray(np.repeat(pend_params()[:, None], B, 1))
    xg, ug, cg = ddp.forward_pass(ddp.GaussianPolicy(N, n, m, K, k, None, None), x0, u, x, al, prob, None, params=P, model=(fx, fu, fc))
    assert ddp.default_handle().last_kernel(1) == KERNEL and cg.shape == (N + 1, B, len(al))
    stage, terminal = fr.pend_cost(PEND_P)
    worst, crossed = 0.0, False
    for b in range(B):
        for a, alpha in enumerate(al):
            xs, us, cs = fr.rollout(x0[:, b], u[..., b], fx[..., b], fu[..., b], fc[..., b], stage, terminal, K=K[..., b], k=k[..., b],
                                    x=x[..., b], alpha=alpha, wrap=1)
            d = xs[0].astype(float) - x[0, :, b]
            crossed = crossed or (np.any(np.abs(d) > np.pi) and np.any(np.abs(d) < np.pi))
            worst = max(worst, relerr(xg[..., b, a], xs.astype(float)), relerr(ug[..., b, a], us.astype(float)),
                        relerr(cg[:, b, a], cs.astype(float), 0))
    print("pendcart_ad 4x1 wrapped, terminal: worst relerr %.2e" % worst)
    assert crossed and worst < RTOL


# 4. -------------------------------------------------------------------------------------------------------------- inside the small box
@pytest.mark.parametrize("name", ["lq_12x3", "car_4x2"])
def test_inside_the_small_box_the_lane_kernel_agrees(ddp, name):
    """the wave kernel on a wave=True, fitted_wave=True problem and ddp_user_rollout_fit on a fitted=True problem, the same inputs"""
    rng = np.random.default_rng(77 + len(name))
    B, N = 5, 21
    if name == "car_4x2":
        n, m, kw, src = 4, 2, dict(nparam=9, terminal=True), ddp.example_source("car")
        P = car_params(rng, B)
        lims = np.array([[-0.5, 0.6], [-0.4, 0.4]])
    else:
        n, m, kw, src = 12, 3, dict(nparam=lq_nparam(12, 3)), ddp.example_source("lq")
        P = np.stack([lq_params(np.zeros((n, n)), np.zeros((n, m)), fr._spd(rng, n), fr._spd(rng, m)) for _ in range(B)], -1)
        lims = np.stack([-0.3 * np.ones(m), 0.25 * np.ones(m)], 1)
    fx, fu, fc = fr.designed_tables(rng, n, m, N, B)
    x0, u, x = rng.standard_normal((n, B)), 0.3 * rng.standard_normal((m, N, B)), rng.standard_normal((n, N, B))
    pol = ddp.GaussianPolicy(N, n, m, 0.1 * rng.standard_normal((m, n, N, B)), 0.2 * rng.standard_normal((m, N, B)), None, None)
    al = np.concatenate([[1.0], 10.0 ** np.linspace(-0.3, -3, 10)])
    h = ddp.default_handle()
    wave = ddp.forward_pass(pol, x0, u, x, al, ddp.DeviceProblem(src, n, m, wave=True, fitted_wave=True, **kw), lims, params=P, model=(fx, fu, fc))
    assert h.last_kernel(1) == KERNEL
    lane = ddp.forward_pass(pol, x0, u, x, al, ddp.DeviceProblem(src, n, m, fitted=True, **kw), lims, params=P, model=(fx, fu, fc))
    assert h.last_kernel(1) == "ddp_user_rollout_fit"
    errs = [relerr(np.moveaxis(g, ax, -1), np.moveaxis(r, ax, -1)) for g, r, ax in zip(wave, lane, (1, 1, 0))]
    print("%s: wave against lane kernel, relerr x %.2e u %.2e c %.2e, bits equal: %s" % (name, *errs, same(wave, lane)))
    assert max(errs) < 1e-12, errs


# 5. ------------------------------------------------------------------------------------------------------- loop against the reference
def _loop_args(ddp, c, **more):
    n, m, T, B = c["n"], c["m"], c["T"], c["B"]
    prev = ddp.GaussianPolicy(T, n, m, np.zeros((m, n, T, B)), c["u"].copy(), c["eye"], c["eye"].copy())
    kw = dict(kl_step=kc.LOOP_KL_STEP, max_iter=kc.LOOP_MAX_ITER, cost=c["cost0"], lims=c["lims"], wide=True)
    kw.update(more)
    return prev, kw


def _lq_wave(ddp, n, m, **kw):
    return ddp.DeviceProblem(ddp.example_source("lq"), n, m, nparam=lq_nparam(n, m), wave=True, **kw)


def _model(ddp, c):
    return ddp.kl.Model(c["tfx"], c["tfu"], c["R1"], c["tfc"])


def _check_loop(got, ref, tag):
    xo, uo, pol, Vx, Vxx, cost, tr = got
    worst = 0.0
    for b, (xr, ur, polr, vx, vxx, cr, info) in enumerate(ref):
        mine = (tr["status"][b], tr["iter"][b], tr["n_backpass"][b])
        print("%s trajectory %d: outcome %s, reference %s" % (tag, b, mine, kc.outcome(info)))
        assert mine == kc.outcome(info), (tag, b)
        for a, r, nm in ((tr["η"][:, b], info["eta"], "η"), (xo[..., b], xr, "x"), (uo[..., b], ur, "u"), (pol.K[..., b], polr["K"], "K"),
                         (pol.Σ[..., b], polr["S"], "Σ"), (Vxx[..., b], vxx, "Vxx"), (cost[:, b], cr, "cost")):
            e = relerr(a, r, 0) if nm in ("η", "cost") else relerr(a, r)
            worst = max(worst, e)
            assert e < RTOL, (tag, b, nm, e)
    print("%s: worst relerr against the reference %.2e" % (tag, worst))


def _close(a, b, tol, tag):
    for k_ in ("status", "iter", "n_backpass"):
        assert np.array_equal(a[6][k_], b[6][k_]), (tag, k_, a[6][k_], b[6][k_])
    assert relerr(a[6]["η"], b[6]["η"], 0) < tol, tag
    for i, nm in ((0, "x"), (1, "u"), (3, "Vx"), (4, "Vxx"), (5, "cost")):
        assert relerr(a[i], b[i]) < tol, (tag, nm, relerr(a[i], b[i]))
    for nm in ("K", "Σ", "Σi"):
        assert relerr(getattr(a[2], nm), getattr(b[2], nm)) < tol, (tag, nm)


@pytest.mark.parametrize("n,m,T,lims", fw.LQ_LOOPS)
def test_loop_matches_the_reference_and_the_host_loop(ddp, monkeypatch, n, m, T, lims):
    c = fw.affine_loop_case(n, m, T, lims)
    prev, kw = _loop_args(ddp, c, fitted=True)
    prob = _lq_wave(ddp, n, m, fitted_wave=True)
    prm = lq_params(c["A"], c["Bm"], c["Q"], c["R"])
    h = ddp.default_handle()
    dev = ddp.kl.iLQGkl(prob, c["x"], prev, _model(ddp, c), params=prm, **kw)
    assert h.last_kernel(1) == KERNEL
    if n > 32 or m > 8:
        assert h.last_kernel(0) == WIDE
    _check_loop(dev, fw.loop_reference(n, m, T, lims), "(%d, %d, %d) limits %s" % (n, m, T, lims))
    monkeypatch.setenv("DDP_KL_HOSTLOOP", "1")
    host = ddp.kl.iLQGkl(prob, c["x"], prev, _model(ddp, c), params=prm, **kw)
    monkeypatch.delenv("DDP_KL_HOSTLOOP")
    _close(dev, host, 1e-12, "host loop")


@pytest.mark.parametrize("lims", [False, True])
def test_loop_at_the_corner_on_the_chain(ddp, monkeypatch, lims):
    """(64, 32, 24): the lq parameter block does not fit there, so the tables of that loop case run under the cost of chain_ad (32 links)
    against oracle.np_kl.iLQGkl with the chain's cost closures, and against the host loop"""
    n, m, T = fw.CHAIN_LOOP
    c = fw.affine_loop_case(n, m, T, lims)
    prev, kw = _loop_args(ddp, c, fitted=True, cost=fw.chain_cost0(c))
    prob = ddp.DeviceProblem(ddp.example_source("chain_ad"), n, m, nparam=7, autodiff=True, wave=True, fitted_wave=True)
    h = ddp.default_handle()
    dev = ddp.kl.iLQGkl(prob, c["x"], prev, _model(ddp, c), params=CHAIN_P, **kw)
    assert h.last_kernel(1) == KERNEL and h.last_kernel(0) == WIDE
    _check_loop(dev, fw.loop_reference(n, m, T, lims, True), "chain_ad (%d, %d, %d) limits %s" % (n, m, T, lims))
    monkeypatch.setenv("DDP_KL_HOSTLOOP", "1")
    host = ddp.kl.iLQGkl(prob, c["x"], prev, _model(ddp, c), params=CHAIN_P, **kw)
    monkeypatch.delenv("DDP_KL_HOSTLOOP")
    _close(dev, host, 1e-12, "host loop")


# 6. ------------------------------------------------------------------------------------------------------- the model is really used
def test_the_model_is_really_used(ddp):
    """the parameters of the problem carry another matrix A: the plan on the tables still matches the reference of the tables, and differs
    from the plan on the problem's own model"""
    n, m, T = 33, 9, 30
    c = fw.affine_loop_case(n, m, T, False)
    prev, kw = _loop_args(ddp, c)
    prob = _lq_wave(ddp, n, m, fitted_wave=True)
    prm = lq_params(fw.other_dynamics(c), c["Bm"], c["Q"], c["R"])
    on = ddp.kl.iLQGkl(prob, c["x"], prev, _model(ddp, c), params=prm, fitted=True, **kw)
    _check_loop(on, fw.loop_reference(n, m, T, False), "tables against other parameters")
    off = ddp.kl.iLQGkl(prob, c["x"], prev, _model(ddp, c), params=prm, fitted=False, **kw)
    assert ddp.default_handle().last_kernel(1) == "ddp_user_rollout_wave"
    assert np.all(np.isfinite(off[1]))
    d = np.max(np.abs(on[1] - off[1])) / np.max(np.abs(off[1]))
    print("u on the tables against u on the problem's own model: %.2e relative" % d)
    assert d > 1e-3


# 7. ------------------------------------------------------------------------------------------------------ cost_model= with wide=True
@pytest.mark.parametrize("fitted", [False, True])
def test_cost_model_with_wide(ddp, fitted):
    """the problem's own derivatives at (x, traj_prev.k) as a cost model give the call without one; doubling cuu moves u"""
    n, m, T = 33, 9, 30
    c = fw.affine_loop_case(n, m, T, True)
    B = c["B"]
    prev, kw = _loop_args(ddp, c, fitted=fitted)
    prob = _lq_wave(ddp, n, m, fitted_wave=True) if fitted else _lq_wave(ddp, n, m)          # (any wave problem takes a cost model)
    if fitted:
        model, prm = _model(ddp, c), lq_params(c["A"], c["Bm"], c["Q"], c["R"])
    else:       # the plan on the problem's own model: x must be its rollout, which is what kl_wide_cases.loop_case holds
        c = kc.loop_case(n, m, T, True)
        prev, kw = _loop_args(ddp, c, fitted=False)
        model, prm = ddp.kl.Model(None, None, c["R1"]), lq_params(c["A"], c["Bm"], c["Q"], c["R"])
    rep = lambda M: np.repeat(np.repeat(M[:, :, None, None], T, 2), B, 3)                       # noqa: E731
    cm = [np.einsum("ij,jtb->itb", c["Q"], c["x"]), np.einsum("ij,jtb->itb", c["R"], c["u"]), rep(c["Q"]), np.zeros((n, m, T, B)), rep(c["R"])]
    plain = ddp.kl.iLQGkl(prob, c["x"], prev, model, params=prm, **kw)
    with_cm = ddp.kl.iLQGkl(prob, c["x"], prev, model, params=prm, cost_model=tuple(cm), **kw)
    assert ddp.default_handle().last_kernel(0) == WIDE
    _close(with_cm, plain, 1e-12, "cost model of the problem's own derivatives")
    cm[4] = 2 * cm[4]
    moved = ddp.kl.iLQGkl(prob, c["x"], prev, model, params=prm, cost_model=tuple(cm), **kw)
    d = np.max(np.abs(moved[1] - plain[1])) / np.max(np.abs(plain[1]))
    print("fitted=%s: u with cuu doubled against u: %.2e relative" % (fitted, d))
    assert np.all(np.isfinite(moved[1])) and d > 1e-3


# 8. --------------------------------------------------------------------------------------------------------------- nothing else moved
def test_nothing_else_moved(ddp):
    """on a problem made with the flag, forward_pass without model=, iLQG and kl.iLQGkl(fitted=False, wide=True) give the bits of a
    problem without it"""
    n, m, T = 33, 9, 30
    c = kc.loop_case(n, m, T, True)
    prev, kw = _loop_args(ddp, c)
    prm = lq_params(c["A"], c["Bm"], c["Q"], c["R"])
    with_flag, without = _lq_wave(ddp, n, m, fitted_wave=True), _lq_wave(ddp, n, m)
    h = ddp.default_handle()
    pol = ddp.GaussianPolicy(T, n, m, 0.05 * np.random.default_rng(3).standard_normal((m, n, T, c["B"])), 0.1 * c["u"], None, None)
    al = np.array([1.0, 0.5, 0.1])
    fa = ddp.forward_pass(pol, c["x"][:, 0], c["u"], c["x"], al, with_flag, c["lims"], params=prm)
    assert h.last_kernel(1) == "ddp_user_rollout_wave"
    assert same(fa, ddp.forward_pass(pol, c["x"][:, 0], c["u"], c["x"], al, without, c["lims"], params=prm))
    sa, sb = (ddp.iLQG(p, c["x"][:, 0], c["u"], params=prm, lims=c["lims"], max_iter=4, timing=False) for p in (with_flag, without))
    assert same(tuple(sa[:2]) + (sa[2].K,) + tuple(sa[3:6]), tuple(sb[:2]) + (sb[2].K,) + tuple(sb[3:6]))
    ka, kb = (ddp.kl.iLQGkl(p, c["x"], prev, ddp.kl.Model(None, None, c["R1"]), params=prm, **kw) for p in (with_flag, without))
    assert h.last_kernel(1) == "ddp_user_rollout_wave"
    outs = lambda r: tuple(r[:2]) + (r[2].K, r[2].Σ) + tuple(r[3:6]) + (r[6]["η"],)                # noqa: E731
    assert same(outs(ka), outs(kb))


# 9. --------------------------------------------------------------------------------------------------------------- the round composes
def test_the_round_composes(ddp):
    """sample on the plant -> fit_dynamics(wide=True) -> rollout on the fit -> iLQGkl(fitted=True, wide=True), chain_plant_ad 34x17"""
    n, m, B, N = 34, 17, 4, 20
    S = 2 * (n + m)
    rng = np.random.default_rng(917)
    prob = ddp.DeviceProblem(ddp.example_source("chain_plant_ad"), n, m, nparam=9, wave=True, plant=True, autodiff=True, sample_wave=True,
                             fitted_wave=True)
    P = np.repeat(np.concatenate([CHAIN_P, [0.8, 0.5]])[:, None], B, axis=1)
    h = ddp.default_handle()
    x0 = 0.4 * rng.standard_normal((n, B))
    u = 0.5 * rng.standard_normal((m, N, B))
    x, _, _ = ddp.forward_pass(None, x0, u, None, 1.0, prob, None, params=P)
    K = -0.5 / np.sqrt(n) * rng.random((m, n, N, B))
    Sig = np.repeat(np.repeat((0.3 ** 2 * np.eye(m))[:, :, None, None], N, 2), B, 3)
    Sigi = np.repeat(np.repeat((np.eye(m) / 0.3 ** 2)[:, :, None, None], N, 2), B, 3)
    pol = ddp.GaussianPolicy(N, n, m, K, np.zeros((m, N, B)), Sig, Sigi)
    xs, us, _, info = ddp.sample_policy(prob, pol, x0, x, u, S, seed=11, plant=True, params=P)
    assert h.last_kernel(1) == "ddp_user_sample_wave" and not np.any(info["status"])
    fx, fu, fc, cov, status = ddp.fit_dynamics(xs, us, ridge=1e-3, wide=True)
    with pytest.raises(ddp.DDPError):                             # the fit records no kernel name: at (34, 17) the narrow entry refuses, so
        ddp.fit_dynamics(xs, us, ridge=1e-3)                      # the call above ran ddp_fit_dynamics_wide
    assert not np.any(status) and all(np.all(np.isfinite(a)) for a in (fx, fu, fc, cov))
    xf, uf, cf = ddp.forward_pass(None, x0, u, None, 1.0, prob, None, params=P, model=(fx, fu, fc))
    assert h.last_kernel(1) == KERNEL and all(np.all(np.isfinite(a)) for a in (xf, uf, cf))
    prev = ddp.GaussianPolicy(N, n, m, K, u.copy(), Sig, Sigi)
    out = ddp.kl.iLQGkl(prob, xf, prev, ddp.kl.Model(fx, fu, np.ascontiguousarray(cov[:, :, 0, 0]), fc), params=P, kl_step=1.0, max_iter=10,
                        cost=cf, fitted=True, wide=True)
    assert h.last_kernel(1) == KERNEL and h.last_kernel(0) == WIDE
    print("the round: status %s, iterations %s" % (out[6]["status"], out[6]["iter"]))
    assert set(out[6]["status"]) <= {1, 2, 3}
    assert all(np.all(np.isfinite(a)) for a in (out[0], out[1], out[2].K, out[2].Σ, out[3], out[4], out[5]))


# 10. ----------------------------------------------------------------------------------------------------------- refusals with a device
def test_a_wave_problem_without_the_flag_is_refused_by_name_and_nothing_is_launched(ddp):
    c = fw.rollout_case("lq_33x2", 2)
    prob = ddp.DeviceProblem(ddp.example_source("lq"), 33, 2, nparam=lq_nparam(33, 2), wave=True)
    h = ddp.default_handle()
    ddp.forward_pass(None, c["x0"], c["u"], None, 1.0, prob, None, params=c["P"])            # (creates the problem; names a kernel)
    before = [h.last_kernel(i) for i in range(3)]
    with pytest.raises(ddp.DDPError, match="made without DDP_USER_FITTED .*DDP_USER_FITTED_WAVE"):
        _dev_run(ddp, prob, c)
    assert [h.last_kernel(i) for i in range(3)] == before
