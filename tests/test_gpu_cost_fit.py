"""DDP_USER_COST_FIT on the GPU: ddp_user_cost_fit (fit_cost) against the long-double reference of tests/cost_fit_reference.py fed with the
per-sample derivatives of the existing kernels (ddp_user_df / ddp_user_df_ad and ddp_user_cost at batch S·B), the bit rules, NaN isolation,
and kl.iLQGkl(..., cost_model=...) against oracle.np_kl.iLQGkl with closures whose derivs returns the tables, against its
DDP_KL_HOSTLOOP=1 twin and against the call without a cost model.  Tolerance 1e-8 relative per time step (conftest.relerr); the loops on
the same kernels 1e-12.

Measured on one MI355X (worst over the cases of each test): fit_cost against long double 2.1e-14 (lq (1, 1) at N = B = S = 9; every
other case below 4e-15), the float64 twin of the reference 2.1e-14, the loop against np_kl 1.9e-14 with the fitted dynamics and 1.2e-14
with the cost model alone."""
import ctypes as C

import numpy as np
import pytest

import cost_fit_reference as cr
import fitted_reference as fr
from conftest import relerr
from test_gpu_user_problem import car_closures

pytestmark = pytest.mark.gpu
RTOL = 1e-8


@pytest.fixture(scope="module")
def ddp():
    import ddp_amd
    import ddp_amd.kl  # noqa: F401
    ddp_amd.default_handle()
    return ddp_amd


_PROBLEMS = {}


def _problem(ddp, name):
    if name not in _PROBLEMS:                                    # one program per example and module
        _PROBLEMS[name] = cr.problem_of(ddp, name)
    return _PROBLEMS[name]


def _per_sample(ddp, prob, P, xs, us):
    """c[N,S,B] and the cost derivatives [.,N,S,B] of every sample, from df and costfun of the problem at batch S·B"""
    n, N, S, B = xs.shape
    m = us.shape[0]
    X, U = np.asfortranarray(xs.reshape(n, N, S * B, order="F")), np.asfortranarray(us.reshape(m, N, S * B, order="F"))
    Pb = np.asfortranarray(np.repeat(P, S, axis=1))              # column s + S b: the parameters of trajectory b
    _, _, _, _, _, cx, cu, cxx, cxu, cuu = ddp.df(prob, X, U, params=Pb)
    if prob.const_hessian:
        cxx, cxu, cuu = (np.repeat(a[:, :, None, :], N, 2) for a in (cxx, cxu, cuu))
    cost = ddp.costfun(prob, X, U, params=Pb)
    c = cost[:N].copy()
    if prob.terminal:
        c[N - 1] += cost[N]
    return tuple(a.reshape(a.shape[:-1] + (S, B), order="F") for a in (c, cx, cu, cxx, cxu, cuu))


def _check(ddp, prob, P, xs, us, x, u, wrap, what):
    out = ddp.fit_cost(prob, xs, us, x, u, params=P)
    assert ddp.default_handle().last_kernel(1) == "ddp_user_cost_fit"
    d = _per_sample(ddp, prob, P, xs, us)
    worst, cond = 0.0, 0.0
    for b in range(xs.shape[3]):
        args = [a[..., b] for a in d] + [xs[..., b], us[..., b], x[..., b], u[..., b], wrap]
        ref, twin = cr.fit_cost(*args), cr.fit_cost(*args, dtype=np.float64)
        for name, got, r, t in zip(cr.NAMES, out, ref, twin):
            ax = 0 if r.ndim == 1 else -1
            cond = max(cond, relerr(t, r.astype(float), ax))
            e = relerr(got[..., b], r.astype(float), ax)
            worst = max(worst, e)
            assert e < RTOL, (what, name, b, e)
    print("%s: fit_cost against long double, worst relerr %.2e (float64 twin %.2e)" % (what, worst, cond))
    assert cond < 1e-10, (what, cond)
    return out


@pytest.mark.parametrize("name,N,B,S", cr.SIZES, ids=cr.IDS)
def test_fit_cost_matches_long_double_on_the_derivatives_of_df(ddp, name, N, B, S):
    c = cr.make_case(ddp, name, N, B, S)
    _check(ddp, _problem(ddp, name), c["P"], c["xs"], c["us"], c["x"], c["u"], c["wrap"], "%s N=%d B=%d S=%d" % (name, c["N"], c["B"], c["S"]))


def test_fit_cost_on_samples_of_the_plant(ddp):
    """car_plant: the samples of sample_policy(plant=True) around a rollout of the model, S = 9, N = 12, B = 4"""
    rng = np.random.default_rng(11)
    N, B, S = 12, 4, 9
    P = np.concatenate([fr.car_params(rng, B), np.array([[1.3], [0.75], [0.05], [-0.03]]) * np.ones((1, B))])
    prob = ddp.DeviceProblem(ddp.example_source("car_plant"), 4, 2, nparam=13, terminal=True, plant=True, sample=True, cost_fit=True, params=P)
    x0 = np.array([1.2, 1.0, 0.6, 0.8])[:, None] + 0.05 * rng.standard_normal((4, B))
    u = np.asfortranarray(0.3 * rng.standard_normal((2, N, B)))
    x, _, _ = ddp.forward_pass(None, x0, u, None, 1.0, prob, None)
    x = np.asfortranarray(x.reshape(4, N, B))
    Sg = np.repeat(np.repeat((0.05 * np.eye(2))[:, :, None, None], N, 2), B, 3)
    pol = ddp.GaussianPolicy(N, 4, 2, 0.1 * rng.standard_normal((2, 4, N, B)), np.zeros((2, N, B)), Sg, Sg)
    xs, us, _, info = ddp.sample_policy(prob, pol, x0, x, u, S, seed=5, plant=True)
    assert not info["status"].any() and np.all(np.isfinite(xs))
    _check(ddp, prob, P, xs, us, x, u, 0, "car_plant")


def test_a_quadratic_cost_gives_df_at_the_nominal(ddp):
    """lq (10, 2): whatever the samples, the fitted model is the expansion at the nominal"""
    for name in ("lq_ad", "lq32"):
        c = cr.make_case(ddp, name, 6, 3, 7)
        prob = _problem(ddp, name)
        cx, cu, cxx, cxu, cuu, c0 = ddp.fit_cost(prob, c["xs"], c["us"], c["x"], c["u"], params=c["P"])
        _, _, _, _, _, dcx, dcu, dcxx, dcxu, dcuu = ddp.df(prob, c["x"], c["u"], params=c["P"])
        if prob.const_hessian:
            dcxx, dcxu, dcuu = (np.repeat(a[:, :, None, :], c["N"], 2) for a in (dcxx, dcxu, dcuu))
        cost = ddp.costfun(prob, c["x"], c["u"], params=c["P"])
        for got, want in ((cx, dcx), (cu, dcu), (cxx, dcxx), (cuu, dcuu)):
            for b in range(c["B"]):
                assert relerr(got[..., b], want[..., b]) < RTOL, name
        assert np.max(np.abs(cxu - dcxu)) == 0.0
        assert relerr(c0, cost[:c["N"]], 0) < RTOL


# -------------------------------------------------------------------------------------------------------------------------- bit rules
@pytest.fixture(scope="module")
def carcase(ddp):
    c = cr.make_case(ddp, "car", 11, 10, 5)                      # two trajectory groups, two chunks of steps, two rounds of samples
    return c, ddp.fit_cost(_problem(ddp, "car"), c["xs"], c["us"], c["x"], c["u"], params=c["P"])


def test_two_calls_a_slice_and_shared_parameters_give_the_same_bits(ddp, carcase):
    c, full = carcase
    prob = _problem(ddp, "car")
    again = ddp.fit_cost(prob, c["xs"], c["us"], c["x"], c["u"], params=c["P"])
    assert all(np.array_equal(a, b) for a, b in zip(full, again))
    f = np.asfortranarray
    part = ddp.fit_cost(prob, f(c["xs"][..., 1:3]), f(c["us"][..., 1:3]), f(c["x"][..., 1:3]), f(c["u"][..., 1:3]), params=f(c["P"][:, 1:3]))
    assert all(np.array_equal(a[..., 1:3], b) for a, b in zip(full, part))
    one = ddp.fit_cost(prob, f(c["xs"][..., 1]), f(c["us"][..., 1]), f(c["x"][..., 1]), f(c["u"][..., 1]), params=f(c["P"][:, 1]))
    assert all(np.array_equal(a[..., 1], b) for a, b in zip(full, one))                # the unbatched call drops the batch axis
    p0 = f(c["P"][:, 0])
    shared = ddp.fit_cost(prob, c["xs"], c["us"], c["x"], c["u"], params=p0)
    tiled = ddp.fit_cost(prob, c["xs"], c["us"], c["x"], c["u"], params=f(np.repeat(p0[:, None], c["B"], 1)))
    assert all(np.array_equal(a, b) for a, b in zip(shared, tiled))


def test_host_entry_matches_the_device_entry(ddp, carcase):
    c, full = carcase
    prob = _problem(ddp, "car")
    h, L = ddp.default_handle(), ddp._lib.lib()
    n, m, N, B, S = c["n"], c["m"], c["N"], c["B"], c["S"]
    ins = [c["P"], c["xs"], c["us"], c["x"], c["u"]]
    shapes = [s + (N, B) for s in ((n,), (m,), (n, n), (n, m), (m, m), ())]
    outs = [np.zeros(s, order="F") for s in shapes]
    din = [h.to_device(np.asfortranarray(a)) for a in ins]
    dout = [h.to_device(np.full(s, -7.0, order="F")) for s in shapes]
    try:
        ddp._lib.check(L.ddp_user_cost_fit_f64_dev(h.raw, prob._ptr(h), N, S, B, din[0], 1, *din[1:], *dout))
        h.sync()
        res = [h.to_host(p, s) for p, s in zip(dout, shapes)]
    finally:
        for p in din + dout:
            h.free(p)
    assert all(np.array_equal(a, b) for a, b in zip(full, res))
    plain = ddp.DeviceProblem(ddp.example_source("car"), 4, 2, nparam=9, terminal=True)
    rc = L.ddp_user_cost_fit_f64(h.raw, plain._ptr(h), N, S, B, *[a.ctypes.data_as(C.c_void_p) for a in ins[:1]], 1,
                                 *[a.ctypes.data_as(C.c_void_p) for a in ins[1:] + outs])
    assert rc == -1 and "made without DDP_USER_COST_FIT" in L.ddp_last_error().decode()


def test_a_nan_sample_stays_in_its_own_step_and_trajectory(ddp, carcase):
    c, full = carcase
    xs = c["xs"].copy(order="F")
    xs[1, 9, 3, 7] = np.nan                                      # step 9, sample 3, trajectory 7
    out = ddp.fit_cost(_problem(ddp, "car"), xs, c["us"], c["x"], c["u"], params=c["P"])
    for name, a, clean in zip(cr.NAMES, out, full):
        bad = ~np.isfinite(a.reshape(-1, c["N"], c["B"])).all(axis=0)
        want = np.zeros((c["N"], c["B"]), bool); want[9, 7] = True
        if name in ("cxu", "cuu"):                               # (the car's cxu = 0 and cuu = wu I do not see x̂: they stay finite)
            assert not bad[~want].any(), name
        else:
            assert np.array_equal(bad, want), name
        keep = np.broadcast_to(~want, a.shape)
        assert np.array_equal(a[keep], clean[keep]), name


# ---------------------------------------------------------------------------------------------------------------------- the whole loop
@pytest.fixture(scope="module")
def loop(ddp):
    case = fr.loop_case()
    rng = np.random.default_rng(17)
    N, B, S = case["N"], case["B"], 8
    xs = np.asfortranarray(case["x"][:, :, None, :] + 0.05 * rng.standard_normal((4, N, S, B)))
    us = np.asfortranarray(case["u"][:, :, None, :] + 0.05 * rng.standard_normal((2, N, S, B)))
    car = ddp.DeviceProblem(ddp.example_source("car"), 4, 2, nparam=9, terminal=True, params=case["P"], fitted=True, cost_fit=True)
    cm = ddp.fit_cost(car, xs, us, case["x"], case["u"])[:5]
    prev = ddp.GaussianPolicy(N, 4, 2, case["Kp"], case["u"], case["Sp"], case["Sip"])
    return case, car, cm, prev


def _oracle(case, b, cm, fx, fu, f, lims=None):
    from oracle import np_kl
    _, costfun, _ = car_closures(case["P"][:, b])
    derivs = lambda x, u: (fx, fu) + tuple(a[..., b] for a in cm)          # noqa: E731
    pb = dict(K=case["Kp"][..., b], k=case["u"][..., b], S=case["Sp"][..., b], Si=case["Sip"][..., b])
    return np_kl.iLQGkl(f, costfun, derivs, case["x"][..., b], pb, dict(fx=fx, R1=case["R1"]), kl_step=0.5, lims=lims, max_iter=20)


def _against_oracle(dev, case, cm, fitted):
    xo, uo, pol, Vx, Vxx, cost, tr = dev
    worst = 0.0
    for b in range(case["B"]):
        if fitted:
            fx, fu, fc = case["fx"][..., b], case["fu"][..., b], case["fc"][..., b]
            f = lambda x, u, i: fx[:, :, i] @ x + fu[:, :, i] @ u + fc[:, i]          # noqa: E731
        else:
            f, _, df = car_closures(case["P"][:, b])
            fx, fu = df(case["x"][..., b], case["u"][..., b])[:2]
        xr, ur, polr, vx, vxx, cr_, info = _oracle(case, b, cm, fx, fu, f)
        assert (tr["status"][b], tr["iter"][b], tr["n_backpass"][b]) == (info["status"], info["iter"], info["n_backpass"]), b
        errs = (relerr(tr["η"][:, b], info["eta"], 0), relerr(xo[..., b], xr), relerr(uo[..., b], ur), relerr(pol.K[..., b], polr["K"]),
                relerr(Vxx[..., b], vxx), relerr(cost[:, b], cr_, 0))
        worst = max(worst, *errs)
        assert max(errs) < RTOL, (b, errs)
    return worst


def test_loop_on_the_fitted_models_matches_numpy(ddp, loop):
    """car, N = 40, B = 3, fitted=True and cost_model=fit_cost(...): decisions equal, η, x, u, K, Vxx, cost at 1e-8"""
    case, car, cm, prev = loop
    dev = ddp.kl.iLQGkl(car, case["x"], prev, ddp.kl.Model(case["fx"], case["fu"], case["R1"], case["fc"]), kl_step=0.5, max_iter=20,
                        cost=case["c"], fitted=True, cost_model=cm)
    assert ddp.default_handle().last_kernel(1) == "ddp_user_rollout_fit"
    print("loop (fitted dynamics and cost) against np_kl: worst relerr %.2e" % _against_oracle(dev, case, cm, True))


def test_loop_on_the_cost_model_alone_matches_numpy(ddp, loop):
    """cost_model= without fitted=True: the oracle with the car's own fx, fu at the nominal and the same cost tables"""
    case, car, cm, prev = loop
    x = np.zeros_like(case["x"])                                 # iLQGkl expects a trajectory consistent with its model: the car's own rollout
    c = np.zeros_like(case["c"])
    for b in range(case["B"]):
        f, costfun, _ = car_closures(case["P"][:, b])
        x[:, 0, b] = case["x0"][:, b]
        for i in range(case["N"] - 1):
            x[:, i + 1, b] = f(x[:, i, b], case["u"][:, i, b], i)
        c[:, b] = costfun(x[..., b], case["u"][..., b])
    own = dict(case, x=x, c=c)
    dev = ddp.kl.iLQGkl(car, x, prev, ddp.kl.Model(None, None, case["R1"]), kl_step=0.5, max_iter=20, cost=c, cost_model=cm)
    assert ddp.default_handle().last_kernel(1) == "ddp_user_rollout"
    print("loop (cost model alone) against np_kl: worst relerr %.2e" % _against_oracle(dev, own, cm, False))


@pytest.mark.parametrize("lims", [None, "on"])
@pytest.mark.parametrize("fitted", [True, False], ids=["fitted", "own-model"])
def test_device_loop_equals_host_loop(ddp, loop, monkeypatch, lims, fitted):
    case, car, cm, prev = loop
    L = None if lims is None else np.array([[-1.0, 1.0], [-0.8, 0.8]])
    model = ddp.kl.Model(case["fx"], case["fu"], case["R1"], case["fc"]) if fitted else ddp.kl.Model(None, None, case["R1"])
    kw = dict(kl_step=0.5, max_iter=20, cost=case["c"], lims=L, fitted=fitted, cost_model=cm)
    dev = ddp.kl.iLQGkl(car, case["x"], prev, model, **kw)
    monkeypatch.setenv("DDP_KL_HOSTLOOP", "1")
    host = ddp.kl.iLQGkl(car, case["x"], prev, model, **kw)
    for k_ in ("status", "iter", "n_backpass"):
        assert np.array_equal(dev[6][k_], host[6][k_]), k_
    for i in (0, 1, 3, 4, 5):
        assert relerr(dev[i], host[i]) < 1e-12, (i, relerr(dev[i], host[i]))
    assert relerr(dev[2].K, host[2].K) < 1e-12 and relerr(dev[2].Σ, host[2].Σ) < 1e-12


@pytest.mark.parametrize("example,kw", [("car", {}), ("lq", dict(const_hessian=True))], ids=["car", "lq-const-hessian"])
def test_the_problems_own_derivatives_as_cost_model_change_nothing(ddp, loop, example, kw):
    """cost_model = df(problem, x, u) at the nominal reproduces the call without it (1e-12), also for a problem with constant Hessians"""
    case, car, _, prev = loop
    N, B = case["N"], case["B"]
    if example == "car":
        prob, x, c, pr = car, case["x"], case["c"], prev
        model = ddp.kl.Model(case["fx"], case["fu"], case["R1"], case["fc"])
        kw = dict(fitted=True)
    else:
        rng = np.random.default_rng(23)
        n, m = 4, 2
        A = np.eye(n) + 0.05 * rng.standard_normal((n, n))
        from test_gpu_user_problem import lq_params
        P = lq_params(A, 0.2 * rng.standard_normal((n, m)), cr._spd(rng, n), cr._spd(rng, m))
        prob = ddp.DeviceProblem(ddp.example_source("lq"), n, m, nparam=cr.LQ_NP(n, m), params=P, **kw)
        u0 = np.asfortranarray(0.3 * rng.standard_normal((m, N, B)))
        x, _, c = ddp.forward_pass(None, rng.standard_normal((n, B)), u0, None, 1.0, prob, None)
        x, c = np.asfortranarray(x.reshape(n, N, B)), c.reshape(-1, B)
        pr = ddp.GaussianPolicy(N, n, m, case["Kp"], u0, case["Sp"], case["Sip"])
        model, kw = ddp.kl.Model(None, None, 1e-3 * np.eye(n)), {}
    _, _, _, _, _, cx, cu, cxx, cxu, cuu = ddp.df(prob, x, pr.k)
    if prob.const_hessian:
        cxx, cxu, cuu = (np.asfortranarray(np.repeat(a[:, :, None, :], N, 2)) for a in (cxx, cxu, cuu))
    a = ddp.kl.iLQGkl(prob, x, pr, model, kl_step=0.5, max_iter=20, cost=c, **kw)
    b = ddp.kl.iLQGkl(prob, x, pr, model, kl_step=0.5, max_iter=20, cost=c, cost_model=(cx, cu, cxx, cxu, cuu), **kw)
    # car: the same kernels on the same numbers, 1e-12.  Constant Hessians: the call without a cost model may take the backward kernel
    # for Hessians without a time axis, the call with one takes a time-varying kernel: the project's 1e-8 between two kernels
    tol = 1e-12 if example == "car" else RTOL
    for k_ in ("status", "iter", "n_backpass"):
        assert np.array_equal(a[6][k_], b[6][k_]), k_
    for i in (0, 1, 3, 4, 5):
        assert relerr(a[i], b[i]) < tol, (i, relerr(a[i], b[i]))
    assert relerr(a[2].K, b[2].K) < tol


def test_the_cost_model_is_really_used(ddp, loop):
    case, car, cm, prev = loop
    model = ddp.kl.Model(case["fx"], case["fu"], case["R1"], case["fc"])
    kw = dict(kl_step=0.5, max_iter=5, cost=case["c"], fitted=True)
    a = ddp.kl.iLQGkl(car, case["x"], prev, model, cost_model=cm, **kw)
    b = ddp.kl.iLQGkl(car, case["x"], prev, model, cost_model=(cm[0], 2.0 * cm[1]) + tuple(cm[2:]), **kw)
    assert np.all(np.isfinite(a[1])) and np.all(np.isfinite(b[1]))
    assert np.max(np.abs(a[1] - b[1])) > 1e-3 * np.max(np.abs(a[1]))
