"""User problems through the KL-constrained loop on the GPU (ddp_user_ilqgkl_*), and back_pass_gps on the mid kernel
(back_pass_mid_kernel<..., GPS>, DDP_GPS_MID).  Tolerance 1e-8 relative per time step (conftest.relerr) against the C oracle, the
committed back_pass_gps fixtures, the registered families' iLQGkl and the NumPy restatement driven by the user's closures."""
import numpy as np
import pytest

from conftest import load_golden, relerr
from test_gpu_user_problem import car_closures, car_params, lq_params, pend_params

pytestmark = pytest.mark.gpu
RTOL = 1e-8
MID = "back_pass_gps_mid"
GPS = ["kl_gps_n4m2", "kl_gps_n4m2_lims", "kl_gps_n4m2_eta_per_step", "kl_gps_n4m1_lims", "kl_gps_n10m2", "kl_gps_n4m2_diverge"]
SHAPES = [(n, m) for n in (1, 3, 6, 10, 13, 16, 17, 24, 32) for m in (1, 2, 3, 4, 5, 8)]


@pytest.fixture(scope="module")
def ddp():
    import ddp_amd
    import ddp_amd.kl  # noqa: F401
    ddp_amd.default_handle()
    return ddp_amd


def _reload(ddp):
    ddp.default_handle().raw                                  # (re-reads the DDP_* switches when they changed)


@pytest.fixture
def gps_mid(ddp, monkeypatch):
    def set_(v):
        if v is None:
            monkeypatch.delenv("DDP_GPS_MID", raising=False)
        else:
            monkeypatch.setenv("DDP_GPS_MID", v)
        _reload(ddp)
    yield set_
    monkeypatch.delenv("DDP_GPS_MID", raising=False)
    _reload(ddp)


def _last(ddp):
    return ddp.default_handle().last_kernel(0)


# ---------------------------------------------------------------------------------------------------------- the kernel alone
@pytest.mark.parametrize("name", GPS)
def test_gps_mid_goldens(ddp, gps_mid, name):
    gps_mid("1")
    kl = ddp.kl
    g = load_golden(name)
    N = g["u"].shape[1]
    prev = ddp.GaussianPolicy(N, g["x"].shape[0], g["u"].shape[0], g["Kp"], g["kp"], g["Sp"], g["Sip"])
    terms = kl.grad_kl(prev)
    L = None if g["lims"].size == 0 else g["lims"]
    d, pol, Vx, Vxx, dV = kl.back_pass_gps(g["cx"], g["cu"], g["cxx"], g["cxu"], g["cuu"], g["fx"], g["fu"], L, g["x"], g["u"], (terms, g["etab"]))
    assert _last(ddp) == MID
    assert d == int(g["diverge"])
    for got, key in ((pol.K, "K"), (pol.k, "k"), (pol.Σ, "Quui"), (pol.Σi, "Quu"), (Vx, "Vx"), (Vxx, "Vxx"), (dV, "dV")):
        assert relerr(got, g[key]) < RTOL, (key, relerr(got, g[key]))
    assert np.array_equal(Vxx, np.transpose(Vxx, (1, 0, 2)))


def _spd(rng, d, s=1.0):
    a = rng.standard_normal((d, d))
    return s * (a @ a.T / d + 0.5 * np.eye(d))


@pytest.mark.parametrize("n,m", SHAPES)
def test_gps_mid_matches_oracle(ddp, gps_mid, n, m):
    """every valid (n, m) pair: with and without active limits, one η per trajectory and per step, shared and per-trajectory dynamics
    and cost, one trajectory whose small η makes Quu indefinite at one step"""
    from oracle import oracle_ctypes as oc
    gps_mid("1")
    kl = ddp.kl
    rng = np.random.default_rng(100 * n + m)
    N, B = 12, 3
    fxb = np.stack([np.stack([np.eye(n) + 0.1 * rng.standard_normal((n, n)) for _ in range(N)], -1) for _ in range(B)], -1)
    fub = 0.3 * rng.standard_normal((n, m, N, B))
    cxxb = np.stack([np.stack([_spd(rng, n) for _ in range(N)], -1) for _ in range(B)], -1)
    cuub = np.stack([np.stack([_spd(rng, m, 0.5) for _ in range(N)], -1) for _ in range(B)], -1)
    cxub = 0.05 * rng.standard_normal((n, m, N, B))
    cx, cu = rng.standard_normal((n, N, B)), rng.standard_normal((m, N, B))
    u, x = 0.3 * rng.standard_normal((m, N, B)), rng.standard_normal((n, N, B))
    Kp, kp = 0.2 * rng.standard_normal((m, n, N, B)), 0.1 * rng.standard_normal((m, N, B))
    Sip = np.stack([np.stack([_spd(rng, m, 2.0) for _ in range(N)], -1) for _ in range(B)], -1)
    Sp = np.stack([np.stack([np.linalg.inv(Sip[:, :, t, b]) for t in range(N)], -1) for b in range(B)], -1)
    prev = ddp.GaussianPolicy(N, n, m, Kp, kp, Sp, Sip)
    terms = kl.grad_kl(prev)
    lims_on = np.stack([-0.3 * np.ones(m), 0.25 * np.ones(m)], 1)
    seen_div = False
    for fx_b, cost_b, lims, eta_tv, bad in ((1, 1, None, False, False), (0, 1, lims_on, False, False), (1, 0, None, True, False),
                                            (0, 0, lims_on, True, False), (1, 1, None, False, True), (1, 1, lims_on, True, True)):
        fx, fu = (fxb, fub) if fx_b else (fxb[..., 0], fub[..., 0])
        cxx, cxu, cuu = (cxxb, cxub, cuub.copy()) if cost_b else (cxxb[..., 0], cxub[..., 0], cuub[..., 0].copy())
        etab = np.stack([1e-8 * np.ones(B), np.array([1.0, 0.5, 2.0]), 1e16 * np.ones(B)])
        if eta_tv:
            etab = np.repeat(etab[:, None, :], N, 1) * (1.0 + 0.1 * np.arange(N))[None, :, None]
        if bad:                                   # Quu indefinite at step 6 of trajectory 1: a small η there lets the cost term dominate
            cuu = cuub.copy()
            cuu[:, :, 6, 1] = -1e3 * np.eye(m)
            cxx, cxu, fx, fu = cxxb, cxub, fxb, fub
        div, pol, Vx, Vxx, dV = kl.back_pass_gps(cx, cu, cxx, cxu, cuu, fx, fu, lims, x, u, (terms, etab))
        assert _last(ddp) == MID
        assert np.array_equal(Vxx, np.transpose(Vxx, (1, 0, 2, 3)))
        for b in range(B):
            sl = (lambda a: a[..., b]) if (cost_b or bad) else (lambda a: a)                                    # noqa: E731
            fl = (lambda a: a[..., b]) if (fx_b or bad) else (lambda a: a)                                      # noqa: E731
            tb = oc.kl_terms(Kp[..., b], kp[..., b], Sip[..., b])
            eb = etab[:, :, b] if eta_tv else etab[:, b]
            d, (K, k, Quui, Quu), vx, vxx, dv = oc.back_pass_gps(cx[..., b], cu[..., b], sl(cxx), sl(cxu), sl(cuu), fl(fx), fl(fu), lims,
                                                                x[..., b], u[..., b], (tb, eb))
            assert div[b] == d, (b, div[b], d)
            seen_div |= d > 0
            for got, ref, nm in ((pol.K[..., b], K, "K"), (pol.k[..., b], k, "k"), (pol.Σ[..., b], Quui, "Quui"),
                                 (pol.Σi[..., b], Quu, "Quu"), (Vx[..., b], vx, "Vx"), (Vxx[..., b], vxx, "Vxx")):
                assert relerr(got, ref) < RTOL, (nm, b, fx_b, cost_b, lims is not None, eta_tv, relerr(got, ref))
            assert relerr(dV[:, b], dv, 0) < RTOL
    assert seen_div


# ------------------------------------------------------------------------------------------------------------- whole loop: LQ
def _lq_setup(rng, n=10, m=2, T=60, B=4, h=0.01):
    import scipy.linalg as sla
    A0 = rng.standard_normal((n, n)); A = sla.expm(h * (A0 - A0.T)); Bm = h * rng.standard_normal((n, m))
    Q, R = h * np.eye(n), 0.1 * h * np.eye(m)
    u = 0.1 * rng.standard_normal((m, T, B)) * np.linspace(0.5, 3.0, B)
    x = np.zeros((n, T, B)); x[:, 0, :] = 1.0 + 0.1 * rng.standard_normal((n, B))
    for t in range(T - 1):
        x[:, t + 1, :] = A @ x[:, t, :] + Bm @ u[:, t, :]
    cost0 = 0.5 * np.einsum("itb,ij,jtb->b", x, Q, x) + 0.5 * np.einsum("itb,ij,jtb->b", u, R, u)
    eye = np.repeat(np.repeat(np.eye(m)[:, :, None, None], T, 2), B, 3)
    return A, Bm, Q, R, u, x, cost0, eye


@pytest.mark.parametrize("mode", ["default", "mid0", "const_hessian"])
def test_user_lq_loop_matches_registered_and_oracle(ddp, gps_mid, mode):
    from oracle import oracle_ctypes as oc
    gps_mid("0" if mode == "mid0" else None)
    kl = ddp.kl
    rng = np.random.default_rng(31)
    n, m, T, B = 10, 2, 60, 4
    A, Bm, Q, R, u, x, cost0, eye = _lq_setup(rng, n, m, T, B)
    prev = ddp.GaussianPolicy(T, n, m, np.zeros((m, n, T, B)), u, eye, eye.copy())
    fx, fu, R1 = np.repeat(A[:, :, None], T, 2), np.repeat(Bm[:, :, None], T, 2), 1e-4 * np.eye(n)
    kw = dict(kl_step=2e-4, max_iter=40, cost=cost0)
    reg = kl.iLQGkl(ddp.LQProblem(A, Bm, Q, R), x, prev, kl.Model(fx, fu, R1), **kw)
    user = ddp.DeviceProblem(ddp.example_source("lq"), n, m, nparam=2 * n * n + n * m + m * m, const_hessian=(mode == "const_hessian"))
    got = kl.iLQGkl(user, x, prev, kl.Model(None, None, R1), params=lq_params(A, Bm, Q, R), **kw)
    assert _last(ddp) == ("back_pass_gps" if mode == "mid0" else MID)
    (xo, uo, pol, Vx, Vxx, cost, tr), (xr, ur, polr, Vxr, Vxxr, costr, trr) = got, reg
    for k_ in ("status", "iter", "n_backpass"):
        assert np.array_equal(tr[k_], trr[k_]), k_
    assert relerr(tr["η"], trr["η"], 0) < RTOL
    for a, b_, nm in ((xo, xr, "x"), (uo, ur, "u"), (pol.K, polr.K, "K"), (pol.Σ, polr.Σ, "S"), (pol.Σi, polr.Σi, "Si"), (Vx, Vxr, "Vx"),
                      (Vxx, Vxxr, "Vxx"), (cost, costr, "cost")):
        assert relerr(a, b_) < RTOL, (nm, relerr(a, b_))
    p = oc.make_problem("lq", n, m, T, A=A, B=Bm, Q=Q, R=R)
    for b in range(B):
        pb = dict(K=np.zeros((m, n, T)), k=u[..., b], S=eye[..., b], Si=eye[..., b])
        xr_, ur_, polr_, vx, vxx, cr, info = oc.ilqgkl(p, x[..., b], float(cost0[b]), pb, dict(fx=fx, R1=R1), kl_step=2e-4, max_iter=40)
        assert (tr["status"][b], tr["iter"][b], tr["n_backpass"][b]) == (info["status"], info["iter"], info["n_backpass"])
        assert relerr(tr["η"][:, b], info["eta"], 0) < RTOL
        assert relerr(xo[..., b], xr_) < RTOL and relerr(uo[..., b], ur_) < RTOL and relerr(pol.K[..., b], polr_["K"]) < RTOL
        assert relerr(Vxx[..., b], vxx) < RTOL and relerr(cost[:, b], cr, 0) < RTOL


# ------------------------------------------------------------------------------------------------------------ whole loop: car
def _car_setup(ddp, rng, B, N=40):
    P = car_params(rng, B)
    x0 = np.array([0.0, 0.0, 0.3, 0.5])[:, None] + 0.05 * rng.standard_normal((4, B))
    u = 0.3 * rng.standard_normal((2, N, B))
    car = ddp.DeviceProblem(ddp.example_source("car"), 4, 2, nparam=9, terminal=True, params=P)
    x, _, c = ddp.forward_pass(None, x0, u, None, 1.0, car, None)
    Sip = np.stack([np.stack([_spd(rng, 2, 2.0) for _ in range(N)], -1) for _ in range(B)], -1)
    Sp = np.stack([np.stack([np.linalg.inv(Sip[:, :, t, b]) for t in range(N)], -1) for b in range(B)], -1)
    Kp = 0.1 * rng.standard_normal((2, 4, N, B))
    prev = ddp.GaussianPolicy(N, 4, 2, Kp, u, Sp, Sip)
    return car, P, x, u, c, prev


@pytest.mark.parametrize("external", [False, True])
def test_user_car_loop_matches_numpy_closures(ddp, gps_mid, external):
    from oracle import np_kl
    gps_mid(None)
    kl = ddp.kl
    rng = np.random.default_rng(41)
    B, N = 3, 40
    car, P, x, u, c, prev = _car_setup(ddp, rng, B, N)
    R1 = 1e-3 * np.eye(4)
    fxm = np.stack([np.stack([np.eye(4) + 0.01 * rng.standard_normal((4, 4)) for _ in range(N)], -1) for _ in range(B)], -1) if external else None
    kw = dict(kl_step=0.5, max_iter=20, cost=c)
    xo, uo, pol, Vx, Vxx, cost, tr = kl.iLQGkl(car, x, prev, kl.Model(fxm, None, R1), **kw)
    assert _last(ddp) == "back_pass_gps_lane"                     # n = 4, m = 2
    for b in range(B):
        f, cf, df = car_closures(P[:, b])
        derivs = lambda xx, uu: df(xx, uu)                                                  # noqa: E731
        mf = fxm[..., b] if external else df(x[..., b], u[..., b])[0]
        pb = dict(K=prev.K[..., b], k=u[..., b], S=prev.Σ[..., b], Si=prev.Σi[..., b])
        xr, ur, polr, vx, vxx, cr, info = np_kl.iLQGkl(f, cf, derivs, x[..., b], pb, dict(fx=mf, R1=R1), kl_step=0.5, max_iter=20)
        assert (tr["status"][b], tr["iter"][b], tr["n_backpass"][b]) == (info["status"], info["iter"], info["n_backpass"]), b
        assert relerr(xo[..., b], xr) < RTOL and relerr(uo[..., b], ur) < RTOL and relerr(pol.K[..., b], polr["K"]) < RTOL
        assert relerr(Vxx[..., b], vxx) < RTOL and relerr(cost[:, b], cr, 0) < RTOL
    ad = ddp.DeviceProblem(ddp.example_source("car_ad"), 4, 2, nparam=9, terminal=True, autodiff=True, params=P)
    xa, ua, pola, Vxa, Vxxa, costa, tra = kl.iLQGkl(ad, x, prev, kl.Model(fxm, None, R1), **kw)
    assert np.array_equal(tra["iter"], tr["iter"])
    for a, b_ in ((xa, xo), (ua, uo), (pola.K, pol.K), (Vxxa, Vxx), (costa, cost)):
        assert relerr(a, b_) < RTOL


def test_user_car_loop_with_limits_matches_or_parts_at_a_tie(ddp, gps_mid):
    """with control limits every trajectory matches the NumPy restatement, or parts from it at a box-QP tie: the loop never moves x, u
    or the derivatives, so up to the parting iteration both solves match and the backward pass of that iteration gets the same operands
    and the same η (to rounding) — the difference can only come from a discontinuity inside the box-QP"""
    from oracle import np_kl
    gps_mid(None)
    kl = ddp.kl
    rng = np.random.default_rng(43)
    B, N = 4, 40
    car, P, x, u, c, prev = _car_setup(ddp, rng, B, N)
    R1, L = 1e-3 * np.eye(4), np.array([[-1.0, 1.0], [-0.6, 0.6]])
    kw = dict(kl_step=0.5, lims=L)
    xo, uo, pol, Vx, Vxx, cost, tr = kl.iLQGkl(car, x, prev, kl.Model(None, None, R1), cost=c, max_iter=20, **kw)

    def numpy_solve(b, it):
        f, cf, df = car_closures(P[:, b])
        pb = dict(K=prev.K[..., b], k=u[..., b], S=prev.Σ[..., b], Si=prev.Σi[..., b])
        return np_kl.iLQGkl(f, cf, df, x[..., b], pb, dict(fx=df(x[..., b], u[..., b])[0], R1=R1), max_iter=it, **kw)

    def agree(got, ref):
        (xg, ug, Kg, cg, trg), (xr, ur, polr, cr, info) = got, ref
        return ((trg["status"], trg["iter"], trg["n_backpass"]) == (info["status"], info["iter"], info["n_backpass"]) and
                relerr(xg, xr) < RTOL and relerr(ug, ur) < RTOL and relerr(Kg, polr["K"]) < RTOL and relerr(cg, cr, 0) < RTOL)
    parted = 0
    for b in range(B):
        xr, ur, polr, vx, vxx, cr, info = numpy_solve(b, 20)
        if agree((xo[..., b], uo[..., b], pol.K[..., b], cost[:, b], {k_: tr[k_][b] for k_ in ("status", "iter", "n_backpass")}),
                 (xr, ur, polr, cr, info)):
            continue
        parted += 1
        sub = ddp.DeviceProblem(ddp.example_source("car"), 4, 2, nparam=9, terminal=True, params=P[:, b])
        pv = ddp.GaussianPolicy(N, 4, 2, prev.K[..., b], u[..., b], prev.Σ[..., b], prev.Σi[..., b])
        for it in range(1, 21):                   # the first iteration count at which the two solves differ
            g = kl.iLQGkl(sub, x[..., b], pv, kl.Model(None, None, R1), cost=c[:, b], max_iter=it, **kw)
            r = numpy_solve(b, it)
            if not agree((g[0], g[1], g[2].K, g[5], g[6]), (r[0], r[1], r[2], r[5], r[6])):
                break
            eta_before = (g[6]["η"], r[6]["eta"])
        assert it > 1, b                                                  # the first iteration's pass agrees
        assert relerr(eta_before[0], eta_before[1], 0) < 1e-12, b         # the parting pass got the same η: a tie, not a wrong kernel
    assert parted < B


@pytest.mark.parametrize("lims", [None, "on"])
def test_device_loop_equals_host_loop(ddp, gps_mid, monkeypatch, lims):
    """the device-resident loop and the DDP_KL_HOSTLOOP=1 loop of the same DeviceProblem (per-trajectory params) on the same kernel"""
    gps_mid("1")
    kl = ddp.kl
    rng = np.random.default_rng(51)
    B, N = 4, 40
    car, P, x, u, c, prev = _car_setup(ddp, rng, B, N)
    L = None if lims is None else np.array([[-1.0, 1.0], [-0.8, 0.8]])
    kw = dict(kl_step=0.5, max_iter=20, cost=c, lims=L)
    dev = kl.iLQGkl(car, x, prev, kl.Model(None, None, 1e-3 * np.eye(4)), **kw)
    monkeypatch.setenv("DDP_KL_HOSTLOOP", "1")
    host = kl.iLQGkl(car, x, prev, kl.Model(None, None, 1e-3 * np.eye(4)), **kw)
    for k_ in ("status", "iter", "n_backpass"):
        assert np.array_equal(dev[6][k_], host[6][k_]), k_
    for i in (0, 1, 3, 4, 5):
        assert relerr(dev[i], host[i]) < 1e-12, i
    assert relerr(dev[2].K, host[2].K) < 1e-12 and relerr(dev[2].Σ, host[2].Σ) < 1e-12


def test_kernel_reporting(ddp, gps_mid):
    gps_mid(None)
    kl = ddp.kl
    rng = np.random.default_rng(61)
    n, m, N, B = 4, 1, 50, 2
    pend = ddp.DeviceProblem(ddp.example_source("pendcart"), 4, 1, nparam=25, params=pend_params(), terminal=True)
    x0 = np.array([0.3, 0.0, 0.0, 0.0])[:, None] + 0.05 * rng.standard_normal((n, B))
    u = 0.2 * rng.standard_normal((m, N, B))
    x, _, c = ddp.forward_pass(None, x0, u, None, 1.0, pend, None)
    eye = np.ones((1, 1, N, B))
    prev = ddp.GaussianPolicy(N, n, m, np.zeros((m, n, N, B)), u, eye, eye.copy())
    kl.iLQGkl(pend, x, prev, kl.Model(None, None, 1e-4 * np.eye(n)), kl_step=0.5, max_iter=3, cost=c)
    assert _last(ddp) == "back_pass_gps_q4"
