"""User problems on the GPU (ddp_user_*, DeviceProblem): the rollout, derivative and cost kernels generated around the bundled example
sources against the built-in families, the C oracle and the NumPy restatement, and whole device-resident iLQG solves of them."""
import numpy as np
import pytest

from conftest import par_map, relerr
from user_lane_cases import car_closures                # noqa: F401  (the car's closures live with the lane cases; imported from here by other tests)

pytestmark = pytest.mark.gpu

PEND_P = dict(g=9.82, l=0.35, h=0.01, d=0.99, goal=np.array([np.pi, 0, 0, 0.0]), Q=np.diag([10.0, 1, 2, 1]), R=1.0)


def pend_params(P=PEND_P):
    return np.concatenate([[P["g"], P["l"], P["h"], P["d"]], P["goal"], P["Q"].ravel(order="F"), [P["R"]]])


def lq_params(A, B, Q, R):
    return np.concatenate([A.ravel(order="F"), B.ravel(order="F"), Q.ravel(order="F"), R.ravel(order="F")])


@pytest.fixture(scope="module")
def ddp():
    import ddp_amd
    return ddp_amd


# one program per example and module: a compile takes a fraction of a second to a few seconds
@pytest.fixture(scope="module")
def pend(ddp):
    return ddp.DeviceProblem(ddp.example_source("pendcart"), 4, 1, nparam=25, params=pend_params(), terminal=True)


@pytest.fixture(scope="module")
def car(ddp):
    return ddp.DeviceProblem(ddp.example_source("car"), 4, 2, nparam=9, terminal=True)


@pytest.fixture(scope="module")
def lq10(ddp):
    return ddp.DeviceProblem(ddp.example_source("lq"), 10, 2, nparam=224)


@pytest.fixture(scope="module")
def lq10c(ddp):
    return ddp.DeviceProblem(ddp.example_source("lq"), 10, 2, nparam=224, const_hessian=True)


# ---------------------------------------------------------------- car: Python closures (the same formulas as user_examples/car.hip)
def car_params(rng, B):
    P = np.empty((9, B))
    P[0] = 0.05                                             # h
    P[1] = 4.0 + rng.uniform(-0.5, 0.5, B); P[2] = 4.0 + rng.uniform(-0.5, 0.5, B)        # goal
    P[3] = 2.0 + rng.uniform(-0.3, 0.3, B); P[4] = 2.0 + rng.uniform(-0.3, 0.3, B)        # obstacle on the way
    P[5] = 0.6 + rng.uniform(0, 0.3, B); P[6] = rng.uniform(5.0, 20.0, B)                 # radius, weight
    P[7] = 0.1; P[8] = rng.uniform(5.0, 20.0, B)                                           # control, terminal weights
    return P


# ------------------------------------------------------------------------------------------------------------------ rollouts
def test_pendulum_rollout_matches_the_builtin_family(ddp, pend):
    """same f and cost as the built-in pendulum (its own sin / cos, pend_math.h): every output of 512 x 11 rollouts with limits"""
    from oracle import np_restatement as npr
    rng = np.random.default_rng(1)
    n, m, N, B = 4, 1, 600, 512
    x0 = np.array([0.3, 0.0, 0.0, 0.0])[:, None] + 0.05 * rng.standard_normal((n, B))
    u = 0.5 * rng.standard_normal((m, N, B))
    K = 0.2 * rng.standard_normal((m, n, N, B)); k = 0.2 * rng.standard_normal((m, N, B))
    x = x0[:, None, :] + 0.05 * rng.standard_normal((n, N, B))
    L = np.array([[-1.0, 1.0]])
    al = ddp.DEFAULT_ALPHA
    pol = ddp.GaussianPolicy(N, n, m, K, k)
    xb, ub, cb = ddp.forward_pass(pol, x0, u, x, al, ddp.PendcartProblem(), L)
    xu, uu, cu = ddp.forward_pass(pol, x0, u, x, al, pend, L)
    assert ddp.default_handle().last_kernel(1) == "ddp_user_rollout"
    assert cu.shape == cb.shape == (N + 1, B, len(al))
    assert relerr(xu, xb, 1) < 1e-12 and relerr(uu, ub, 1) < 1e-12
    assert relerr(cu, cb, 0) < 1e-12
    # the rollout's own running sum (csum, what the driver's line search reads) through the C entries of both families
    import ctypes as C
    from ddp_amd import _lib
    h = ddp.default_handle()
    csb, csu = np.zeros((B, len(al)), order="F"), np.zeros((B, len(al)), order="F")
    dp = ddp._DevProblem(ddp.PendcartProblem(), N, B)
    f64 = [_lib.f64(a) for a in (K, k, x0, u, x, L)]
    _lib.check(_lib.lib().ddp_forward_pass_f64(h.raw, C.byref(dp.struct), *map(_lib.ptr, f64[:5]), _lib.ptr(_lib.f64(al)), len(al),
                                               _lib.ptr(f64[5]), *map(_lib.ptr, (xb.copy(order="F"), ub.copy(order="F"), cb.copy(order="F"))),
                                               _lib.ptr(csb)))
    P = _lib.f64(pend_params())
    _lib.check(_lib.lib().ddp_user_forward_pass_f64(h.raw, pend._ptr(h), N, B, _lib.ptr(P), 0, *map(_lib.ptr, f64[:5]),
                                                    _lib.ptr(_lib.f64(al)), len(al), _lib.ptr(f64[5]),
                                                    *map(_lib.ptr, (xu.copy(order="F"), uu.copy(order="F"), cu.copy(order="F"))), _lib.ptr(csu)))
    assert relerr(csu, csb) < 1e-12 and relerr(csu, cu.sum(0)) < 1e-12
    f, costfun, _ = npr.pendcart_closures()
    for b, ai in ((0, 0), (17, 5), (511, 10)):
        xr, ur, cr = npr.forward_pass((K[..., b], k[..., b]), x0[:, b], u[..., b], x[..., b], al[ai], f, costfun, L)
        assert relerr(xu[:, :, b, ai], xr) < 1e-10 and relerr(uu[:, :, b, ai], ur) < 1e-10 and relerr(cu[:, b, ai], cr, 0) < 1e-10


def test_wrapped_diff_rollout_matches_numpy(ddp):
    from oracle import np_restatement as npr
    prob = ddp.DeviceProblem(ddp.example_source("pendcart"), 4, 1, nparam=25, params=pend_params(), terminal=True,
                             diff=ddp.WrappedDiff(0))
    rng = np.random.default_rng(2)
    n, m, N, B = 4, 1, 120, 6
    x0 = np.array([0.2, 0.0, 0.0, 0.0])[:, None] + 0.05 * rng.standard_normal((n, B))
    u = 0.3 * rng.standard_normal((m, N, B))
    K = 0.2 * rng.standard_normal((m, n, N, B)); k = 0.2 * rng.standard_normal((m, N, B))
    x = x0[:, None, :] + 0.05 * rng.standard_normal((n, N, B))
    x[0] += 2 * np.pi * rng.integers(-2, 3, (N, B))          # nominal angles a few turns away: only the wrapped difference is small
    xu, uu, cu = ddp.forward_pass(ddp.GaussianPolicy(N, n, m, K, k), x0, u, x, 0.5, prob, None)
    f, costfun, _ = npr.pendcart_closures()
    for b in range(B):
        xr, ur, cr = npr.forward_pass((K[..., b], k[..., b]), x0[:, b], u[..., b], x[..., b], 0.5, f, costfun, None, npr.wrapped_diff(1))
        assert relerr(xu[:, :, b], xr) < 1e-10 and relerr(uu[:, :, b], ur) < 1e-10 and relerr(cu[:, b], cr, 0) < 1e-10


# ------------------------------------------------------------------------------------------------------------------------ df
def test_car_derivatives_match_the_python_closures(ddp, car):
    rng = np.random.default_rng(3)
    n, m, N, B = 4, 2, 300, 64
    P = car_params(rng, B)
    x = rng.uniform(0, 4, (n, N, B)); x[2] = rng.uniform(-3, 3, (N, B))
    u = rng.standard_normal((m, N, B))
    fx, fu, fxx, fxu, fuu, cx, cu, cxx, cxu, cuu = ddp.df(car, x, u, params=P)
    assert fxx.size == fxu.size == fuu.size == 0
    for b in range(B):
        want = car_closures(P[:, b])[2](x[..., b], u[..., b])
        for got, ref in zip((fx, fu, cx, cu, cxx, cxu, cuu), want):
            assert relerr(got[..., b], ref) < 1e-8
    c = ddp.costfun(car, x, u, params=P)
    for b in (0, 31, 63):
        assert relerr(c[:, b], car_closures(P[:, b])[1](x[..., b], u[..., b]), 0) < 1e-12


CHAIN = r"""
// 12 coupled pendulums: x = (q[12], v[12]), u[4] drives v[0], v[3], v[6], v[9]; params = [h, k, c, kc, w, r, a]
__device__ void dynamics(const double *x, const double *u, int i, const double *p, double *xn)
{
    const double h = p[0], k = p[1], c = p[2], kc = p[3];
    for (int j = 0; j < 12; ++j) {
        const double ql = j > 0 ? x[j - 1] : 0.0, qr = j < 11 ? x[j + 1] : 0.0;
        double acc = -k * sin(x[j]) - c * x[12 + j] + kc * (ql - 2.0 * x[j] + qr);
        if (j % 3 == 0) acc += u[j / 3];
        xn[j] = x[j] + h * x[12 + j];
        xn[12 + j] = x[12 + j] + h * acc;
    }
}
__device__ double stage_cost(const double *x, const double *u, int i, const double *p)
{
    const double w = p[4], r = p[5], a = p[6];
    double c = 0.0;
    for (int j = 0; j < 12; ++j) c += 0.5 * w * (x[j] * x[j] + 0.1 * x[12 + j] * x[12 + j]) + a * (1.0 - cos(x[j]));
    for (int q = 0; q < 4; ++q) c += 0.5 * r * u[q] * u[q];
    return c;
}
__device__ void derivatives(const double *x, const double *u, int i, int N, const double *p, double *fx, double *fu, double *cx,
                            double *cu, double *cxx, double *cxu, double *cuu)
{
    const double h = p[0], k = p[1], c = p[2], kc = p[3], w = p[4], r = p[5], a = p[6];
    for (int e = 0; e < 24 * 24; ++e) fx[e] = 0.0;
    for (int e = 0; e < 24 * 4; ++e) fu[e] = 0.0;
    for (int e = 0; e < 24 * 24; ++e) cxx[e] = 0.0;
    for (int e = 0; e < 24 * 4; ++e) cxu[e] = 0.0;
    for (int e = 0; e < 16; ++e) cuu[e] = 0.0;
    for (int j = 0; j < 12; ++j) {
        fx[j + 24 * j] = 1.0; fx[j + 24 * (12 + j)] = h;
        fx[12 + j + 24 * j] = h * (-k * cos(x[j]) - 2.0 * kc);
        if (j > 0) fx[12 + j + 24 * (j - 1)] = h * kc;
        if (j < 11) fx[12 + j + 24 * (j + 1)] = h * kc;
        fx[12 + j + 24 * (12 + j)] = 1.0 - h * c;
        if (j % 3 == 0) fu[12 + j + 24 * (j / 3)] = h;
        cx[j] = w * x[j] + a * sin(x[j]); cx[12 + j] = 0.1 * w * x[12 + j];
        cxx[j + 24 * j] = w + a * cos(x[j]); cxx[12 + j + 24 * (12 + j)] = 0.1 * w;
    }
    for (int q = 0; q < 4; ++q) { cu[q] = r * u[q]; cuu[q + 4 * q] = r; }
}
"""
CHAIN_P = np.array([0.02, 9.0, 0.3, 4.0, 1.0, 0.05, 2.0])


def chain_closures(p):
    h, k, c, kc, w, r, a = p

    def acc(x, u):
        q, v = x[:12], x[12:]
        ql = np.concatenate([[0.0], q[:-1]]); qr = np.concatenate([q[1:], [0.0]])
        ac = -k * np.sin(q) - c * v + kc * (ql - 2 * q + qr)
        ac[0::3] += u
        return ac

    def f(x, u, i):
        return np.concatenate([x[:12] + h * x[12:], x[12:] + h * acc(x, u)])

    def costfun(x, u):
        q, v = x[:12], x[12:]
        return (0.5 * w * (q * q + 0.1 * v * v) + a * (1 - np.cos(q))).sum(0) + 0.5 * r * (u * u).sum(0)

    def df(x, u):
        N = x.shape[1]
        fx = np.zeros((24, 24, N)); fu = np.zeros((24, 4, N)); cxx = np.zeros((24, 24, N))
        for t in range(N):
            q = x[:12, t]
            J = np.diag(-k * np.cos(q) - 2 * kc) + kc * (np.eye(12, k=1) + np.eye(12, k=-1))
            fx[:, :, t] = np.block([[np.eye(12), h * np.eye(12)], [h * J, (1 - h * c) * np.eye(12)]])
            fu[12 + np.arange(0, 12, 3), np.arange(4), t] = h
            cxx[:, :, t] = np.diag(np.concatenate([w + a * np.cos(q), 0.1 * w * np.ones(12)]))
        cx = np.concatenate([w * x[:12] + a * np.sin(x[:12]), 0.1 * w * x[12:]])
        cuu = np.repeat((r * np.eye(4))[:, :, None], N, axis=2)
        return fx, fu, cx, r * u, cxx, np.zeros((24, 4, N)), cuu

    return f, costfun, df


def test_large_nonlinear_pass_matches_numpy(ddp):
    """n = 24, m = 4 nonlinear (the rollout with one step per chunk and 32 rollouts per work-group, back_pass_mid): rollout, df,
    backward pass and the rollout of the new policy against NumPy"""
    from oracle import np_restatement as npr
    rng = np.random.default_rng(4)
    n, m, N, B = 24, 4, 200, 4
    prob = ddp.DeviceProblem(CHAIN, n, m, nparam=7, params=CHAIN_P)
    x0 = np.concatenate([0.5 * rng.standard_normal((12, B)), 0.1 * rng.standard_normal((12, B))])
    u = 0.3 * rng.standard_normal((m, N, B))
    lims = np.array([[-1.0, 1.0]] * 4)
    x, u1, c = ddp.forward_pass(None, x0, u, None, 1.0, prob, lims)
    fx, fu, _, _, _, cx, cu, cxx, cxu, cuu = ddp.df(prob, x, u1)
    assert ddp.default_handle().last_kernel(2) == "ddp_user_df"
    div, pol, Vx, Vxx, dV = ddp.back_pass(cx, cu, cxx, cxu, cuu, fx, fu, 1.0, 1, lims, x, u1)
    xn, un, cn = ddp.forward_pass(pol, x0, u1, x, 0.5, prob, lims)
    f, costfun, dfn = chain_closures(CHAIN_P)
    for b in range(B):
        xr, ur, cr = npr.forward_pass(None, x0[:, b], u[..., b], None, 1.0, f, costfun, lims)
        assert relerr(x[..., b], xr) < 1e-10 and relerr(u1[..., b], ur) < 1e-10 and relerr(c[:, b], cr, 0) < 1e-10
        want = dfn(x[..., b], u1[..., b])
        for got, ref in zip((fx, fu, cx, cu, cxx, cxu, cuu), want):
            assert relerr(got[..., b], ref) < 1e-10
        d, (K, k, _), vx, vxx, _ = npr.back_pass(*want[2:], want[0], want[1], 1.0, 1, lims, x[..., b], u1[..., b])
        assert d == div[b] == 0
        assert relerr(pol.K[..., b], K) < 1e-8 and relerr(pol.k[..., b], k) < 1e-8 and relerr(Vxx[..., b], vxx) < 1e-8
        xr, ur, cr = npr.forward_pass((K, k), x0[:, b], u1[..., b], x[..., b], 0.5, f, costfun, lims)
        assert relerr(xn[..., b], xr) < 1e-8 and relerr(un[..., b], ur) < 1e-8 and relerr(cn[:, b], cr, 0) < 1e-8


# ----------------------------------------------------------------------------------------------------------------- whole solves
def test_lq_solves_match_the_c_oracle(ddp, lq10):
    """C2 shape: n = 10, m = 2, N = 1000, 256 trajectories with their own x0, u0 — every output of every solve"""
    from oracle import np_restatement as npr
    from oracle import oracle_ctypes as oc
    rng = np.random.default_rng(5)
    n, m, N, B = 10, 2, 1000, 256
    Pq = npr.make_lq_problem(rng, T=N)
    A, Bm, Q, R = Pq["A"], Pq["B"], Pq["Q"], Pq["R"]
    x0 = 1.0 + 0.1 * rng.standard_normal((n, B)); u0 = 0.1 * rng.standard_normal((m, N, B))
    x, u, pol, Vx, Vxx, cost, tr = ddp.iLQG(lq10, x0, u0, params=lq_params(A, Bm, Q, R), timing=False)
    p = oc.make_problem("lq", n, m, N, A=A, B=Bm, Q=Q, R=R)

    def one(b):
        xr, ur, (K, k, _), vx, vxx, cr, info = oc.ilqg(p, x0[:, b], u0[..., b])
        assert tr["status"][b] == info["status"] and tr["iter"][b] == info["iter"], (b, tr["status"][b], info["status"])
        assert int(tr["stats"][2, b]) == info["accepted_iter"] and int(tr["stats"][3, b]) == info["n_backpass"]
        for got, ref in ((x[..., b], xr), (u[..., b], ur), (pol.K[..., b], K), (Vx[..., b], vx), (Vxx[..., b], vxx)):
            assert relerr(got, ref) < 1e-8, b
        # after a gradient exit k is the last backward pass's feed-forward term: tiny next to u, so its last digits are the rounding
        # of a backward kernel that sums in another order than the oracle (per-trajectory, time-varying cost Hessians)
        assert relerr(pol.k[..., b], k) < 1e-6, b
        assert relerr(cost[:, b], cr, 0) < 1e-8
    par_map(one, range(B))


def test_car_solves_match_numpy(ddp, car):
    """different goals and obstacles per trajectory, the obstacle's indefinite Hessian in the backward pass: the first 8 accepted
    iterations of every solve against the NumPy restatement (an exit by tolerance would hinge on the last digits of g_norm / Δcost).
    Without control limits (with limits: the next test)."""
    from oracle import np_restatement as npr
    rng = np.random.default_rng(6)
    n, m, N, B = 4, 2, 60, 16
    P = car_params(rng, B)
    x0 = np.zeros((n, B)); x0[:2] = rng.uniform(0, 0.5, (2, B)); x0[2] = np.pi / 4 + rng.uniform(-0.2, 0.2, B)
    u0 = 0.1 * rng.standard_normal((m, N, B))
    lims = None
    kw = dict(max_iter=8, tol_grad=0.0, tol_fun=-1.0)
    x, u, pol, Vx, Vxx, cost, tr = ddp.iLQG(car, x0, u0, lims=lims, params=P, timing=False, **kw)
    for b in range(B):
        f, costfun, dfn = car_closures(P[:, b])
        xr, ur, (K, k, _), vx, vxx, cr, info = npr.iLQG(f, costfun, dfn, x0[:, b], u0[..., b], lims=lims, **kw)
        assert tr["status"][b] == info["status"] and tr["iter"][b] == info["iter"], b
        assert int(tr["stats"][3, b]) == info["n_backpass"] and int(tr["stats"][4, b]) == info["n_forward"], b
        for got, ref in ((x[..., b], xr), (u[..., b], ur), (pol.K[..., b], K), (Vx[..., b], vx), (Vxx[..., b], vxx)):
            assert relerr(got, ref) < 1e-8, b
        assert relerr(cost[:, b], cr, 0) < 1e-8


def _np_iteration_row(f, costfun, dfn, x0, x, u, lims, lam, dlam, lam_max=1e10, lam_min=1e-6, lf=1.6):
    """one iteration of the reference (iLQG.jl:225-330: derivatives, backward pass retried with a larger λ on failure, the serial line
    search, accept / reject) from the trajectory (x, u): its trace row (λ, α, sum(cost), g_norm)"""
    from oracle import np_restatement as npr
    from ddp_amd import DEFAULT_ALPHA
    fx, fu, cx, cu, cxx, cxu, cuu = dfn(x, u)
    c0 = float(np.sum(costfun(x, u)))
    while True:
        d, (K, k, _), _, _, dV = npr.back_pass(cx, cu, cxx, cxu, cuu, fx, fu, lam, 1, lims, x, u)
        if d == 0:
            break
        dlam, lam = max(dlam * lf, lf), max(lam * dlam, lam_min)
        if lam > lam_max:
            return None
    g_norm = float(np.mean(np.max(np.abs(k) / (np.abs(u) + 1), axis=0)))
    for a in DEFAULT_ALPHA:
        xn, un, cn = npr.forward_pass((K, k), x0, u, x, a, f, costfun, lims)
        dcost = c0 - float(np.sum(cn))
        expected = -a * (dV[0] + a * dV[1])
        z = dcost / expected if expected > 0 else np.sign(dcost)
        if z > 0:
            dlam = min(dlam / lf, 1 / lf)
            return max(lam * dlam, lam_min), a, float(np.sum(cn)), g_norm
    dlam, lam = max(dlam * lf, lf), max(lam * dlam, lam_min)
    return lam, np.nan, c0, g_norm


def _rows_agree(r1, r2):
    (l1, a1, c1, g1), (l2, a2, c2, g2) = r1, r2
    return (abs(l1 - l2) <= 1e-12 * l2 and ((np.isnan(a1) and np.isnan(a2)) or a1 == a2) and abs(c1 - c2) <= 1e-10 * abs(c2)
            and abs(g1 - g2) <= 1e-8 * g2)


def test_car_solves_with_limits_match_numpy_up_to_box_qp_ties(ddp, car):
    """16 car solves with limits, per-trajectory goals and obstacles, against the NumPy restatement, 8 accepted iterations.  The
    obstacle's indefinite Hessian makes backward passes fail and λ grow.  Every per-iteration trace row (λ, α, cost, g_norm) must
    agree until the two part; a trajectory may part only at a box-QP tie of the reference itself: its warm start k[:, i+1] lies on a
    bound to the last bit or one ulp inside it, and boxQP.jl takes a different branch (exit 6 with every control clamped, or exit 4
    with the previous iteration's free set) — a discontinuity of the reference in the last digits of u.  That is checked here:
    up to the parting iteration the states agree to 1e-11, and the reference's own iteration (backward pass and line search), run on the
    GPU's state, reproduces the GPU's trace row while run on its own state it reproduces its own."""
    from oracle import np_restatement as npr
    rng = np.random.default_rng(6)
    n, m, N, B = 4, 2, 60, 16
    P = car_params(rng, B)
    x0 = np.zeros((n, B)); x0[:2] = rng.uniform(0, 0.5, (2, B)); x0[2] = np.pi / 4 + rng.uniform(-0.2, 0.2, B)
    u0 = 0.1 * rng.standard_normal((m, N, B))
    lims = np.array([[-2.0, 2.0], [-1.5, 1.5]])
    kw = dict(tol_grad=0.0, tol_fun=-1.0)
    x, u, pol, Vx, Vxx, cost, tr = ddp.iLQG(car, x0, u0, lims=lims, params=P, timing=False, max_iter=8, **kw)
    H = tr["history"]
    st = tr["stats"]
    assert (st[3] > st[1] - 1).any()                          # some backward pass failed (Cholesky / box-QP) and λ was raised
    runs = {}

    def gpu_state(acc):
        if acc not in runs:
            runs[acc] = ddp.iLQG(car, x0, u0, lims=lims, params=P, timing=False, max_iter=acc, **kw)
        return runs[acc]

    parted = 0
    for b in range(B):
        f, costfun, dfn = car_closures(P[:, b])
        xr, ur, (K, k, _), vx, vxx, cr, info = npr.iLQG(f, costfun, dfn, x0[:, b], u0[..., b], lims=lims, max_iter=8, **kw)
        t = info["trace"]
        rows = len(t["cost"])
        split = None
        for r_ in range(rows):
            same = (abs(H["cost"][r_, b] - t["cost"][r_]) <= 1e-10 * abs(t["cost"][r_]) and abs(H["λ"][r_, b] - t["lam"][r_]) <= 1e-12 * t["lam"][r_]
                    and abs(H["grad_norm"][r_, b] - t["g_norm"][r_]) <= 1e-8 * max(t["g_norm"][r_], 1e-300)
                    and (np.isnan(H["α"][r_, b]) == np.isnan(t["alpha"][r_])) and (np.isnan(t["alpha"][r_]) or H["α"][r_, b] == t["alpha"][r_]))
            if not same:
                split = r_
                break
        if split is None:
            assert tr["status"][b] == info["status"] and tr["iter"][b] == info["iter"], b
            assert int(st[3, b]) == info["n_backpass"] and int(st[4, b]) == info["n_forward"], b
            for got, ref in ((x[..., b], xr), (u[..., b], ur), (pol.K[..., b], K), (Vx[..., b], vx), (Vxx[..., b], vxx)):
                assert relerr(got, ref) < 1e-8, b
            assert relerr(cost[:, b], cr, 0) < 1e-8
            continue
        parted += 1
        acc = int(np.sum(~np.isnan(H["α"][:split, b])))                 # accepted iterations before the parting one
        assert acc >= 1, b
        xg, ug = gpu_state(acc)[0][..., b], gpu_state(acc)[1][..., b]
        xa, ua, _, _, _, _, _ = npr.iLQG(f, costfun, dfn, x0[:, b], u0[..., b], lims=lims, max_iter=acc, **kw)
        assert relerr(xg, xa) < 1e-11 and relerr(ug, ua) < 1e-11, b
        lam, dlam = H["λ"][split - 1, b], H["dλ"][split - 1, b]
        on_gpu = _np_iteration_row(f, costfun, dfn, x0[:, b], xg, ug, lims, lam, dlam)
        on_np = _np_iteration_row(f, costfun, dfn, x0[:, b], xa, ua, lims, lam, dlam)
        assert on_np is not None and _rows_agree(on_np, (t["lam"][split], t["alpha"][split], t["cost"][split], t["g_norm"][split])), b
        assert on_gpu is not None and _rows_agree(on_gpu, (H["λ"][split, b], H["α"][split, b], H["cost"][split, b], H["grad_norm"][split, b])), b
        assert not _rows_agree(on_gpu, on_np), b                # the reference itself parts on the two (1e-11-close) states
    assert parted <= B // 4, parted


PEND_CONST_HESSIAN = """
__device__ void cost_hessians(const double *p, double *cxx, double *cxu, double *cuu)
{
    for (int e = 0; e < 16; ++e) cxx[e] = p[8 + e];
    for (int e = 0; e < 4; ++e) cxu[e] = 0.0;
    cuu[0] = p[24];
}
"""


@pytest.mark.parametrize("const_hessian", [False, True])
def test_compaction_leaves_user_solves_unchanged(ddp, const_hessian):
    """pendulum swing-ups (their lengths vary widely) with per-trajectory damping and goal, the live trajectories moved to smaller
    working sets (DDP_ILQG_COMPACT=2: whenever a set of >= 2 slots is half empty, so the slot map is composed over several
    compactions): params read through the slot map, the constant Hessians re-evaluated after every compaction — the same solves as
    without compaction"""
    import os
    rng = np.random.default_rng(10)
    n, m, N, B = 4, 1, 200, 96
    prob = ddp.DeviceProblem(ddp.example_source("pendcart") + (PEND_CONST_HESSIAN if const_hessian else ""), 4, 1, nparam=25, terminal=True,
                             const_hessian=const_hessian)
    prm = np.repeat(pend_params()[:, None], B, axis=1)
    prm[3] = rng.uniform(0.5, 1.5, B)                           # damping
    prm[6] = rng.uniform(-0.5, 0.5, B)                          # goal cart position
    x0 = np.array([np.pi - 0.6, 0.0, 0.0, 0.0])[:, None] + 0.3 * rng.standard_normal((n, B))
    u0 = 0.1 * rng.standard_normal((m, N, B))
    out = {}
    for v in ("0", "2"):
        os.environ["DDP_ILQG_COMPACT"] = v
        try:
            out[v] = ddp.iLQG(prob, x0, u0, params=prm, lims=np.array([[-5.0, 5.0]]), max_iter=150, timing=False)
        finally:
            del os.environ["DDP_ILQG_COMPACT"]
    it = out["0"][6]["iter"]
    assert np.median(it) + 8 < it.max(), it                 # trajectories end at different times: the working set shrinks
    for a, b_ in zip(out["0"][:2] + out["0"][3:6], out["2"][:2] + out["2"][3:6]):
        assert relerr(b_, a) < 1e-12
    assert (out["0"][6]["status"] == out["2"][6]["status"]).all() and (out["0"][6]["iter"] == out["2"][6]["iter"]).all()
    assert relerr(out["2"][2].K, out["0"][2].K) < 1e-12


def test_const_hessian_gives_the_same_solves(ddp, lq10, lq10c):
    from oracle import np_restatement as npr
    rng = np.random.default_rng(7)
    n, m, N, B = 10, 2, 300, 64
    Pq = npr.make_lq_problem(rng, T=N)
    prm = np.repeat(lq_params(Pq["A"], Pq["B"], Pq["Q"], Pq["R"])[:, None], B, axis=1)        # per-trajectory params, same values
    x0 = 1.0 + 0.1 * rng.standard_normal((n, B)); u0 = 0.1 * rng.standard_normal((m, N, B))
    r0 = ddp.iLQG(lq10, x0, u0, params=prm, lims=np.array([[-0.3, 0.3]] * 2), timing=False)
    r1 = ddp.iLQG(lq10c, x0, u0, params=prm, lims=np.array([[-0.3, 0.3]] * 2), timing=False)
    assert (r0[6]["status"] == r1[6]["status"]).all() and (r0[6]["iter"] == r1[6]["iter"]).all()
    assert relerr(r1[0], r0[0], 1) < 1e-10 and relerr(r1[1], r0[1], 1) < 1e-10


def test_prerolled_start_and_trace_match_the_oracle(ddp, lq10):
    """pre-rolled x0 without cost0 (costfun on the device) against the oracle's pre-rolled solve and against the registered LQ family
    (its trace keys); the seven trace keys of a cold start against the oracle's trace"""
    from oracle import np_restatement as npr
    from oracle import oracle_ctypes as oc
    rng = np.random.default_rng(8)
    n, m, N, B = 10, 2, 400, 32
    Pq = npr.make_lq_problem(rng, T=N)
    prm = lq_params(Pq["A"], Pq["B"], Pq["Q"], Pq["R"])
    prob = ddp.LQProblem(Pq["A"], Pq["B"], Pq["Q"], Pq["R"])
    p = oc.make_problem("lq", n, m, N, A=Pq["A"], B=Pq["B"], Q=Pq["Q"], R=Pq["R"])
    x0 = 1.0 + 0.1 * rng.standard_normal((n, B)); u0 = 0.1 * rng.standard_normal((m, N, B))
    xpre, upre, _ = ddp.forward_pass(None, x0, u0, None, 1.0, prob, None)
    rb = ddp.iLQG(prob, xpre, upre, timing=False)
    ru = ddp.iLQG(lq10, xpre, upre, params=prm, timing=False)
    assert (rb[6]["status"] == ru[6]["status"]).all() and (rb[6]["iter"] == ru[6]["iter"]).all()
    for key in ("λ", "dλ", "cost", "improvement", "grad_norm"):
        assert relerr(np.nan_to_num(ru[6]["history"][key]), np.nan_to_num(rb[6]["history"][key]), 0) < 1e-8, key
    assert np.array_equal(np.isnan(ru[6]["history"]["α"]), np.isnan(rb[6]["history"]["α"]))
    for b in range(0, B, 4):
        xr, ur, (K, k, _), vx, vxx, cr, info = oc.ilqg_prerolled(p, xpre[..., b], upre[..., b])
        assert (ru[6]["status"][b], ru[6]["iter"][b]) == (info["status"], info["iter"]), b
        for got, ref in ((ru[0][..., b], xr), (ru[1][..., b], ur), (ru[2].K[..., b], K), (ru[3][..., b], vx), (ru[4][..., b], vxx)):
            assert relerr(got, ref) < 1e-8, b
        assert relerr(ru[5][:, b], cr, 0) < 1e-8
    rc = ddp.iLQG(lq10, x0[:, :8], u0[..., :8], params=prm, timing=False)
    for b in range(8):
        _, _, _, _, _, _, info = oc.ilqg_trace7(p, x0[:, b], u0[..., b])
        tl = info["trace_len"]
        assert rc[6]["iter"][b] - 1 == tl, b
        for key in ("λ", "dλ", "improvement", "cost", "reduce_ratio", "grad_norm"):
            assert relerr(np.nan_to_num(rc[6]["history"][key][:tl, b]), np.nan_to_num(info["history"][key]), 0) < 1e-8, (key, b)
        assert np.array_equal(np.isnan(rc[6]["history"]["α"][:tl, b]), np.isnan(info["history"]["α"]))


def test_malformed_arguments_raise_before_any_launch(ddp, car):
    rng = np.random.default_rng(9)
    x0 = np.zeros((4, 8)); u0 = np.zeros((2, 50, 8))
    with pytest.raises(ddp.DDPError, match="params"):
        ddp.iLQG(car, x0, u0, params=np.zeros((9, 7)))
    with pytest.raises(ddp.DDPError, match="params"):
        ddp.forward_pass(None, x0, u0, None, 1.0, car, None, params=np.zeros(8))
    with pytest.raises(ddp.DDPError, match="no params"):
        ddp.df(car, np.zeros((4, 50, 8)), u0)
    with pytest.raises(ddp.DDPError, match="n = 4, m = 2"):
        ddp.forward_pass(None, np.zeros((5, 8)), u0, None, 1.0, car, None, params=car_params(rng, 8))
    with pytest.raises(ddp.DDPError, match="lims"):
        ddp.iLQG(car, x0, u0, params=car_params(rng, 8), lims=np.array([[-1.0, 1.0]]))
