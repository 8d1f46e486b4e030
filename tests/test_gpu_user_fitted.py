"""DDP_USER_FITTED on the GPU: ddp_user_rollout_fit against the long-double reference of tests/fitted_reference.py and against the table
emulation user_examples/car_table.hip on the existing rollout kernel, and the whole KL loop planning on the fitted model against
oracle.np_kl.iLQGkl with the fitted closures, against its own DDP_KL_HOSTLOOP=1 twin and against car_table.  Tolerance 1e-8 relative per
time step (conftest.relerr); the loops on the same kernels 1e-12.

Measured on one MI355X (worst over the cases of each test): the rollout against long double 2.8e-13 (u of pendcart, the 2π reduction;
every other figure below 2e-14), csum against the long-double sum of cnew 4.0e-16, the loop against np_kl 1.2e-14."""
import ctypes as C
import re

import numpy as np
import pytest

import fitted_reference as fr
from conftest import relerr
from test_gpu_user_problem import PEND_P, lq_params, pend_params

pytestmark = pytest.mark.gpu
RTOL = 1e-8
LQ_NP = lambda n, m: 2 * n * n + n * m + m * m                    # noqa: E731


@pytest.fixture(scope="module")
def ddp():
    import ddp_amd
    import ddp_amd.kl  # noqa: F401
    ddp_amd.default_handle()
    return ddp_amd


def _layout(ddp, problem):
    t = ddp._lib.lib().ddp_user_program_text(problem.source.encode(), problem.n, problem.m, problem.nparam, problem.flags,
                                             int(problem.diff_mask)).decode()
    return int(re.search(r"#define DDP_FLANES (\d+)", t).group(1)), int(re.search(r"#define DDP_FCHUNK (\d+)", t).group(1))


# ------------------------------------------------------------------------------------------------------------------ the rollout cases
def _lq(rng, n, m, B):
    Q = np.stack([fr._spd(rng, n) for _ in range(B)], -1)
    R = np.stack([fr._spd(rng, m) for _ in range(B)], -1)
    P = np.stack([lq_params(np.zeros((n, n)), np.zeros((n, m)), Q[..., b], R[..., b]) for b in range(B)], -1)
    return P, [fr.lq_cost(Q[..., b], R[..., b]) for b in range(B)]


def _case(ddp, name, N):
    """problem, per-trajectory parameters and cost closures, sizes, policy / limits / step sizes of one row of the issue's table"""
    rng = np.random.default_rng({"car": 1, "lq_ad": 2, "lq1": 3, "lq32": 4, "pend": 5}[name] * 1000 + N)
    src = ddp.example_source
    if name == "car":
        n, m, B, wrap, na, lims = 4, 2, 5, 0, 11, np.array([[-0.5, 0.6], [-0.4, 0.4]])
        P = fr.car_params(rng, B)
        prob = ddp.DeviceProblem(src("car"), n, m, nparam=9, terminal=True, fitted=True)
        costs = [fr.car_cost(P[:, b]) for b in range(B)]
    elif name == "lq_ad":
        n, m, B, wrap, na, lims = 5, 3, 3, 0, 1, None
        P, costs = _lq(rng, n, m, B)
        prob = ddp.DeviceProblem(src("lq_ad"), n, m, nparam=LQ_NP(n, m), autodiff=True, fitted=True)
    elif name == "lq1":
        n, m, B, wrap, na, lims = 1, 1, 2, 0, 11, np.array([[-0.2, 0.3]])
        P, costs = _lq(rng, n, m, B)
        prob = ddp.DeviceProblem(src("lq"), n, m, nparam=LQ_NP(n, m), fitted=True)
    elif name == "lq32":
        n, m, B, wrap, na, lims = 32, 8, 3, 0, 11, np.stack([-0.3 * np.ones(8), 0.25 * np.ones(8)], 1)
        P, costs = _lq(rng, n, m, B)
        prob = ddp.DeviceProblem(src("lq"), n, m, nparam=LQ_NP(n, m), const_hessian=True, fitted=True)
    else:
        n, m, B, wrap, na, lims = 4, 1, 4, 1, 11, None
        P = np.repeat(pend_params()[:, None], B, 1)
        prob = ddp.DeviceProblem(src("pendcart"), n, m, nparam=25, terminal=True, diff=ddp.WrappedDiff(0), fitted=True)
        costs = [fr.pend_cost(PEND_P)] * B
    fx, fu, fc = fr.designed_tables(rng, n, m, N, B)
    x0 = rng.standard_normal((n, B))
    u = 0.3 * rng.standard_normal((m, N, B))
    xn = rng.standard_normal((n, N, B))
    if wrap:
        xn[0] += 2 * np.pi * rng.integers(-2, 3, (N, B))        # the wrapped coordinate: nominal angles whole turns away
    K, k = 0.1 * rng.standard_normal((m, n, N, B)), 0.2 * rng.standard_normal((m, N, B))
    al = np.array([1.0]) if na == 1 else np.concatenate([[1.0], 10.0 ** np.linspace(-0.3, -3, 10)])
    return dict(prob=prob, P=np.asfortranarray(P), costs=costs, n=n, m=m, N=N, B=B, wrap=wrap, al=al, lims=lims, fx=fx, fu=fu, fc=fc, x0=x0,
                u=u, x=xn, K=K, k=k)


def _reference(c):
    n, m, N, B, na = c["n"], c["m"], c["N"], c["B"], len(c["al"])
    CL = N + 1 if c["costs"][0][1] is not None else N
    xr, ur, cr = np.zeros((n, N, B, na)), np.zeros((m, N, B, na)), np.zeros((CL, B, na))
    for b in range(B):
        stage, terminal = c["costs"][b]
        for a, alpha in enumerate(c["al"]):
            xs, us, cs = fr.rollout(c["x0"][:, b], c["u"][..., b], c["fx"][..., b], c["fu"][..., b], c["fc"][..., b], stage, terminal,
                                    K=c["K"][..., b], k=c["k"][..., b], x=c["x"][..., b], alpha=alpha, lims=c["lims"], wrap=c["wrap"])
            xr[..., b, a], ur[..., b, a], cr[:, b, a] = xs.astype(float), us.astype(float), cs.astype(float)
    return xr, ur, cr


def _run(ddp, c, sl=slice(None), tables=None):
    fx, fu, fc = tables or (c["fx"], c["fu"], c["fc"])
    pol = ddp.GaussianPolicy(c["N"], c["n"], c["m"], c["K"][..., sl], c["k"][..., sl], None, None)
    return ddp.forward_pass(pol, c["x0"][:, sl], c["u"][..., sl], c["x"][..., sl], c["al"], c["prob"], c["lims"], params=c["P"][:, sl],
                            model=(fx[..., sl], fu[..., sl], fc[..., sl]))


def _dev_run(ddp, c, active=None, fill=-7.0):
    """the `_dev` entry on uploaded arrays; outputs start as `fill`.  Returns xnew, unew, cnew, csum"""
    h, L = ddp.default_handle(), ddp._lib.lib()
    n, m, N, B, na = c["n"], c["m"], c["N"], c["B"], len(c["al"])
    CL = c["prob"].cost_len(N)
    shapes = [(n, N, B, na), (m, N, B, na), (CL, B, na), (B, na)]
    ins = [h.to_device(np.asfortranarray(a)) for a in (c["P"], c["K"], c["k"], c["x0"], c["u"], c["x"], c["fx"], c["fu"], c["fc"])]
    lim = None if c["lims"] is None else h.to_device(np.asfortranarray(c["lims"]))
    act = None if active is None else h.to_device(np.ascontiguousarray(active, dtype=np.int32))
    outs = [h.to_device(np.full(s, fill, order="F")) for s in shapes]
    dP, dK, dk, dx0, du, dx, dfx, dfu, dfc = ins
    try:
        ddp._lib.check(L.ddp_user_rollout_fit_f64_dev(h.raw, c["prob"]._ptr(h), N, B, dP, 1, dK, dk, dx0, du, dx,
                                                      c["al"].ctypes.data_as(C.c_void_p), na, lim, act, dfx, dfu, dfc, *outs))
        h.sync()
        res = [h.to_host(p, s) for p, s in zip(outs, shapes)]
    finally:
        for p in ins + outs + [q for q in (lim, act) if q is not None]:
            h.free(p)
    return res


TABLE = [("car", 40), ("lq_ad", 17), ("lq1", 1), ("lq1", 2), ("lq32", 6), ("pend", 33)]


@pytest.mark.parametrize("name,N", TABLE + [(nm, None) for nm in ("car", "lq_ad", "lq1", "lq32", "pend")],
                         ids=["%s-N%s" % (a, b if b else "chunk") for a, b in TABLE + [(nm, None) for nm in ("car", "lq_ad", "lq1", "lq32", "pend")]])
def test_rollout_matches_long_double(ddp, name, N):
    """every output against the long-double rollout; csum is the in-order sum of cnew; NaN in slot N-1 of the tables changes nothing; a
    slice of the trajectories reproduces its columns, a second call and the `_dev` entry the same bits; `active` with one trajectory off
    leaves its rows alone.  N = None: 2 chunks + 1 of the layout (one past a chunk boundary whatever layout_of picks).
    Measured worst relerr over all cases: x 1.9e-15, u 2.8e-13 (pendcart; 1.7e-14 elsewhere), c 4.8e-15, csum 4.0e-16."""
    if N is None:
        lanes, chunk = _layout(ddp, _case(ddp, name, 2)["prob"])
        N = 2 * chunk + 1
    c = _case(ddp, name, N)
    lanes, chunk = _layout(ddp, c["prob"])
    B, na = c["B"], len(c["al"])
    assert (B * na) % lanes != 0 or B * na < lanes, (B, na, lanes)             # the last work-group is not full
    xr, ur, cr = _reference(c)
    xg, ug, cg = _run(ddp, c)
    assert ddp.default_handle().last_kernel(1) == "ddp_user_rollout_fit"
    worst = [0.0, 0.0, 0.0]
    for b in range(B):
        for a in range(na):
            e = (relerr(xg[..., b, a], xr[..., b, a]), relerr(ug[..., b, a], ur[..., b, a]), relerr(cg[:, b, a], cr[:, b, a], 0))
            worst = [max(w, v) for w, v in zip(worst, e)]
    print("%s N=%d lanes=%d chunk=%d: worst relerr x %.2e u %.2e c %.2e" % (name, N, lanes, chunk, *worst))
    assert max(worst) < RTOL, worst
    # the `_dev` entry: the same bits, and csum the fixed-order sum of cnew
    xd, ud, cd, sd = _dev_run(ddp, c)
    assert np.array_equal(xd, xg) and np.array_equal(ud, ug) and np.array_equal(cd, cg)
    # csum against the in-order sum of the kernel's own cnew, taken in long double.  The kernel adds c_i in that order, but the compiler
    # may fuse the last multiply-add of the user's cost into the addition (csum + (a b + d) as fma(a, b, csum + d)), so the bits of a
    # float64 sum of the stored c_i are not promised.  Every cost here is non-negative: CL additions in float64 err by at most
    # CL 2^-53 of the sum each way, 2^-52 CL is the bound
    acc = np.zeros((B, na), np.longdouble)
    for t in range(cd.shape[0]):
        acc = acc + cd[t].astype(np.longdouble)
    cerr = float(np.max(np.abs(sd - acc) / acc))
    print("csum against the long-double sum of cnew: %.2e (bound %.2e)" % (cerr, cd.shape[0] * 2.0 ** -52))
    assert cerr <= cd.shape[0] * 2.0 ** -52
    # NaN in slot N-1 of all three tables
    nan_t = tuple(a.copy() for a in (c["fx"], c["fu"], c["fc"]))
    for a in nan_t:
        a[..., N - 1, :] = np.nan
    for got, ref in zip(_run(ddp, c, tables=nan_t), (xg, ug, cg)):
        assert np.array_equal(got, ref)
    # a slice of the trajectories, and a second call
    sl = slice(1, min(3, B))
    for got, ref in zip(_run(ddp, c, sl), (xg, ug, cg)):
        assert np.array_equal(got, ref[..., sl, :])
    for got, ref in zip(_run(ddp, c), (xg, ug, cg)):
        assert np.array_equal(got, ref)
    # `active` with trajectory 1 off: its rows keep the fill, the others are the same bits
    act = np.ones(B, dtype=np.int32); act[1] = 0
    for got, ref in zip(_dev_run(ddp, c, active=act), (xd, ud, cd, sd)):
        on = got[..., act == 1, :]
        assert np.array_equal(on, ref[..., act == 1, :]) and np.all(got[..., 1, :] == -7.0)


def test_rollout_matches_the_table_emulation(ddp):
    """the same rollouts through user_examples/car_table.hip (the tables in the parameter block) on the existing ddp_user_rollout: closed
    loop with limits and 11 step sizes, and the open-loop rollout (no policy)"""
    c = _case(ddp, "car", 40)
    tab = ddp.DeviceProblem(ddp.example_source("car_table"), 4, 2, nparam=9 + 28 * c["N"], terminal=True)
    PT = fr.car_table_params(c["P"], c["fx"], c["fu"], c["fc"])
    pol = ddp.GaussianPolicy(c["N"], 4, 2, c["K"], c["k"], None, None)
    ref = ddp.forward_pass(pol, c["x0"], c["u"], c["x"], c["al"], tab, c["lims"], params=PT)
    assert ddp.default_handle().last_kernel(1) == "ddp_user_rollout"
    got = _run(ddp, c)
    for g, r, ax in zip(got, ref, (1, 1, 0)):
        assert relerr(np.moveaxis(g, ax, -1), np.moveaxis(r, ax, -1)) < RTOL
    ref = ddp.forward_pass(None, c["x0"], c["u"], None, 1.0, tab, None, params=PT)
    got = ddp.forward_pass(None, c["x0"], c["u"], None, 1.0, c["prob"], None, params=c["P"], model=(c["fx"], c["fu"], c["fc"]))
    for g, r, ax in zip(got, ref, (1, 1, 0)):
        assert g.shape == r.shape and relerr(np.moveaxis(g, ax, -1), np.moveaxis(r, ax, -1)) < RTOL
    # (n,n,N)-shaped tables with an unbatched call
    one = ddp.forward_pass(None, c["x0"][:, 2], c["u"][..., 2], None, 1.0, c["prob"], None, params=c["P"][:, 2],
                           model=(c["fx"][..., 2], c["fu"][..., 2], c["fc"][..., 2]))
    for g, r in zip(one, got):
        assert np.array_equal(g, r[..., 2])


# ---------------------------------------------------------------------------------------------------------------------- the whole loop
@pytest.fixture(scope="module")
def case():
    return fr.loop_case()


def _car(ddp, case, example="car", **kw):
    return ddp.DeviceProblem(ddp.example_source(example), 4, 2, nparam=9, terminal=True, params=case["P"], **kw)


def _prev(ddp, case):
    return ddp.GaussianPolicy(case["N"], 4, 2, case["Kp"], case["u"], case["Sp"], case["Sip"])


def _model(ddp, case):
    return ddp.kl.Model(case["fx"], case["fu"], case["R1"], case["fc"])


def test_loop_matches_numpy_with_the_fitted_closures(ddp, case):
    """car, N = 40, B = 3, no limits, against oracle.np_kl.iLQGkl on (f = the affine table, derivs = fitted fx, fu + the car's cost
    derivatives): decisions equal, η, x, u, K, Vxx, cost at 1e-8 (measured worst 1.2e-14); the same solve with car_ad (autodiff=True)
    agrees at 1e-8"""
    kw = dict(kl_step=0.5, max_iter=20, cost=case["c"], fitted=True)
    xo, uo, pol, Vx, Vxx, cost, tr = ddp.kl.iLQGkl(_car(ddp, case, fitted=True), case["x"], _prev(ddp, case), _model(ddp, case), **kw)
    assert ddp.default_handle().last_kernel(1) == "ddp_user_rollout_fit"
    worst = 0.0
    for b in range(case["B"]):
        xr, ur, polr, vx, vxx, cr, info = fr.np_loop(case, b)
        assert info["status"] == 1
        assert (tr["status"][b], tr["iter"][b], tr["n_backpass"][b]) == (info["status"], info["iter"], info["n_backpass"]), b
        errs = (relerr(tr["η"][:, b], info["eta"], 0), relerr(xo[..., b], xr), relerr(uo[..., b], ur), relerr(pol.K[..., b], polr["K"]),
                relerr(Vxx[..., b], vxx), relerr(cost[:, b], cr, 0))
        worst = max(worst, *errs)
        assert max(errs) < RTOL, (b, errs)
    print("loop against np_kl: worst relerr %.2e" % worst)
    ad = _car(ddp, case, "car_ad", autodiff=True, fitted=True)
    xa, ua, pola, Vxa, Vxxa, costa, tra = ddp.kl.iLQGkl(ad, case["x"], _prev(ddp, case), _model(ddp, case), **kw)
    assert np.array_equal(tra["iter"], tr["iter"]) and np.array_equal(tra["status"], tr["status"])
    for a, b_ in ((xa, xo), (ua, uo), (pola.K, pol.K), (Vxxa, Vxx), (costa, cost)):
        assert relerr(a, b_) < RTOL


@pytest.mark.parametrize("lims", [None, "on"])
def test_device_loop_equals_host_loop_and_the_table_emulation(ddp, case, monkeypatch, lims):
    """the device-resident loop against DDP_KL_HOSTLOOP=1 (the same kernels, 1e-12), and against the same loop on car_table without
    `fitted` (the tables in the parameter block, the existing kernels, 1e-8)"""
    L = None if lims is None else np.array([[-1.0, 1.0], [-0.8, 0.8]])
    kw = dict(kl_step=0.5, max_iter=20, cost=case["c"], lims=L)
    car = _car(ddp, case, fitted=True)
    dev = ddp.kl.iLQGkl(car, case["x"], _prev(ddp, case), _model(ddp, case), fitted=True, **kw)
    tab = ddp.DeviceProblem(ddp.example_source("car_table"), 4, 2, nparam=9 + 28 * case["N"], terminal=True,
                            params=fr.car_table_params(case["P"], case["fx"], case["fu"], case["fc"]))
    emu = ddp.kl.iLQGkl(tab, case["x"], _prev(ddp, case), ddp.kl.Model(None, None, case["R1"]), **kw)
    monkeypatch.setenv("DDP_KL_HOSTLOOP", "1")
    host = ddp.kl.iLQGkl(car, case["x"], _prev(ddp, case), _model(ddp, case), fitted=True, **kw)
    for other, tol in ((host, 1e-12), (emu, RTOL)):
        for k_ in ("status", "iter", "n_backpass"):
            assert np.array_equal(dev[6][k_], other[6][k_]), k_
        for i in (0, 1, 3, 4, 5):
            assert relerr(dev[i], other[i]) < tol, (i, tol, relerr(dev[i], other[i]))
        assert relerr(dev[2].K, other[2].K) < tol and relerr(dev[2].Σ, other[2].Σ) < tol


def test_the_model_is_really_used(ddp):
    """tables whose fu has the opposite sign of the car's: planning on them gives other controls than planning on the car's own model"""
    case = fr.loop_case(flip_fu=True)
    car = _car(ddp, case, fitted=True)
    kw = dict(kl_step=0.5, max_iter=5, cost=case["c"])
    on = ddp.kl.iLQGkl(car, case["x"], _prev(ddp, case), _model(ddp, case), fitted=True, **kw)
    off = ddp.kl.iLQGkl(car, case["x"], _prev(ddp, case), _model(ddp, case), fitted=False, **kw)
    assert np.all(np.isfinite(on[1])) and np.all(np.isfinite(off[1]))
    assert np.max(np.abs(on[1] - off[1])) > 1e-3 * np.max(np.abs(off[1]))


def test_nothing_else_moved(ddp, case):
    """fitted=False on a problem made with the flag, and forward_pass without model=, are bit for bit what a problem without the flag gives"""
    with_flag, without = _car(ddp, case, fitted=True), _car(ddp, case)
    kw = dict(kl_step=0.5, max_iter=6, cost=case["c"])
    a = ddp.kl.iLQGkl(with_flag, case["x"], _prev(ddp, case), _model(ddp, case), **kw)
    b = ddp.kl.iLQGkl(without, case["x"], _prev(ddp, case), ddp.kl.Model(case["fx"], case["fu"], case["R1"]), **kw)
    for i in (0, 1, 3, 4, 5):
        assert np.array_equal(a[i], b[i]), i
    assert np.array_equal(a[2].K, b[2].K) and np.array_equal(a[2].Σ, b[2].Σ) and np.array_equal(a[6]["η"], b[6]["η"])
    pol = ddp.GaussianPolicy(case["N"], 4, 2, case["Kp"], 0.1 * case["u"], None, None)
    al = np.array([1.0, 0.5, 0.1])
    fa = ddp.forward_pass(pol, case["x0"], case["u"], case["x"], al, with_flag, None)
    fb = ddp.forward_pass(pol, case["x0"], case["u"], case["x"], al, without, None)
    assert ddp.default_handle().last_kernel(1) == "ddp_user_rollout"
    for g, r in zip(fa, fb):
        assert np.array_equal(g, r)
