"""User problems with DDP_USER_AUTODIFF on the GPU: ddp_user_df_ad against the hand-written `derivatives` of the bundled examples, its
active mask and per-trajectory parameters, the unchanged rollouts of templated models, every supported function against central
differences, and whole device-resident iLQG solves with derived against hand-written derivatives."""

import numpy as np
import pytest

from conftest import relerr

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ddp():
    import ddp_amd
    return ddp_amd


def pend_params():
    return np.concatenate([[9.82, 0.35, 0.01, 0.99], [np.pi, 0, 0, 0], np.diag([10.0, 1, 2, 1]).ravel(order="F"), [1.0]])


def car_params(rng, B):
    P = np.empty((9, B))
    P[0] = 0.05
    P[1:3] = 4.0 + rng.uniform(-0.5, 0.5, (2, B))
    P[3:5] = 2.0 + rng.uniform(-0.3, 0.3, (2, B))
    P[5] = 0.6 + rng.uniform(0, 0.3, B); P[6] = rng.uniform(5.0, 20.0, B)
    P[7] = 0.1; P[8] = rng.uniform(5.0, 20.0, B)
    return P


def lq_params(rng, n, m):
    A = np.eye(n) + 0.05 * rng.standard_normal((n, n))
    Bm = 0.1 * rng.standard_normal((n, m))
    Q = rng.standard_normal((n, n)); Q = Q @ Q.T / n + 0.1 * np.eye(n)
    R = rng.standard_normal((m, m)); R = R @ R.T / m + 0.1 * np.eye(m)
    return np.concatenate([A.ravel(order="F"), Bm.ravel(order="F"), Q.ravel(order="F"), R.ravel(order="F")]), Q, R


def pair(ddp, name, n, m, nparam, **kw):
    """the hand-written example and its templated twin"""
    return (ddp.DeviceProblem(ddp.example_source(name), n, m, nparam=nparam, **kw),
            ddp.DeviceProblem(ddp.example_source(name + "_ad"), n, m, nparam=nparam, autodiff=True, **kw))


def blockwise_close(got, ref, tol=1e-12):
    """max |got - ref| over each (step, trajectory) block (the two trailing axes) against tol x that block's inf-norm (floored at 1e-3
    of the array's, so that an all-zero block of the reference demands zeros to that accuracy)"""
    lead = tuple(range(ref.ndim - 2))
    err = np.max(np.abs(got - ref), axis=lead) if lead else np.abs(got - ref)
    scale = np.max(np.abs(ref), axis=lead) if lead else np.abs(ref)
    scale = np.maximum(scale, 1e-3 * np.max(np.abs(ref)) + 1e-300)
    return float(np.max(err / scale)) <= tol


def random_xu(rng, n, m, N, B):
    x = rng.uniform(-1.0, 1.0, (n, N, B)); x[:2] += 2.0
    return x, rng.standard_normal((m, N, B))


CASES = [("car", 4, 2, 9, dict(terminal=True)), ("pendcart", 4, 1, 25, dict(terminal=True)), ("lq", 10, 2, 224, {}),
         ("lq", 24, 4, 2 * 576 + 96 + 16, {})]


@pytest.mark.parametrize("name,n,m,nparam,kw", CASES, ids=["car", "pendcart", "lq10x2", "lq24x4"])
def test_autodiff_matches_the_hand_written_derivatives(ddp, name, n, m, nparam, kw):
    rng = np.random.default_rng(11)
    N, B = 64, 256
    hand, ad = pair(ddp, name, n, m, nparam, **kw)
    P = car_params(rng, B) if name == "car" else (pend_params() if name == "pendcart" else lq_params(rng, n, m)[0])
    x, u = random_xu(rng, n, m, N, B)
    want = ddp.df(hand, x, u, params=P)
    got = ddp.df(ad, x, u, params=P)
    assert ddp.default_handle().last_kernel(2) == "ddp_user_df_ad"
    for k in (0, 1, 5, 6, 7, 8, 9):                          # fx fu cx cu cxx cxu cuu
        assert got[k].shape == want[k].shape, k
        assert blockwise_close(got[k], want[k]), (k, float(np.max(np.abs(got[k] - want[k]))))
    cxx, cuu = got[7], got[9]
    assert np.array_equal(cxx, cxx.transpose(1, 0, 2, 3)) and np.array_equal(cuu, cuu.transpose(1, 0, 2, 3))


def test_autodiff_with_const_hessian(ddp):
    rng = np.random.default_rng(12)
    n, m, N, B = 10, 2, 64, 256
    hand, ad = pair(ddp, "lq", n, m, 224, const_hessian=True)
    P, Q, R = lq_params(rng, n, m)
    x, u = random_xu(rng, n, m, N, B)
    want, got = ddp.df(hand, x, u, params=P), ddp.df(ad, x, u, params=P)
    for k in (0, 1, 5, 6):
        assert blockwise_close(got[k], want[k]), k
    for k in (7, 8, 9):                                      # from cost_hessians, [., ., B]
        assert np.array_equal(got[k], want[k]), k
    assert np.array_equal(got[7][..., 0], Q) and np.array_equal(got[9][..., 0], R)


def test_active_mask_and_batched_params(ddp):
    """inactive trajectories' rows stay as they were, exactly as ddp_user_df leaves them; each lane reads its own params column"""
    from ddp_amd import _lib
    rng = np.random.default_rng(13)
    n, m, N, B = 4, 2, 40, 96
    hand, ad = pair(ddp, "car", n, m, 9, terminal=True)
    h = ddp.default_handle()
    P = car_params(rng, B)
    x, u = random_xu(rng, n, m, N, B)
    active = (rng.uniform(size=B) < 0.6).astype(np.int32)
    sizes = (n * n, n * m, n, m, n * n, n * m, m * m)
    dP, dx, du, dact = h.to_device(P), h.to_device(x), h.to_device(u), h.to_device(active)
    res = {}
    for key, prob in (("hand", hand), ("ad", ad)):
        outs = [h.to_device(np.full(s * N * B, 7.25)) for s in sizes]
        _lib.check(_lib.lib().ddp_user_df_f64_dev(h.raw, prob._ptr(h), N, B, dP, 1, dx, du, dact, *outs))
        h.sync()
        res[key] = [h.to_host(o, (s, N, B)) for o, s in zip(outs, sizes)]
        for o in outs:
            h.free(o)
    assert h.last_kernel(2) == "ddp_user_df_ad"
    for g, w in zip(res["ad"], res["hand"]):
        assert np.all(g[:, :, active == 0] == 7.25) and np.all(w[:, :, active == 0] == 7.25)
        assert blockwise_close(g[:, :, active == 1], w[:, :, active == 1])
    for p in (dP, dx, du, dact):
        h.free(p)


@pytest.mark.parametrize("name,n,m,nparam", [("car", 4, 2, 9), ("pendcart", 4, 1, 25)])
def test_templated_rollouts_are_bitwise_unchanged(ddp, name, n, m, nparam):
    rng = np.random.default_rng(14)
    N, B = 120, 64
    hand, ad = pair(ddp, name, n, m, nparam, terminal=True)
    P = car_params(rng, B) if name == "car" else pend_params()
    x0 = np.zeros((n, B)); x0[:2] = rng.uniform(0, 0.5, (2, B)); x0 += 0.05 * rng.standard_normal((n, B))
    u = 0.3 * rng.standard_normal((m, N, B))
    K = 0.2 * rng.standard_normal((m, n, N, B)); k = 0.2 * rng.standard_normal((m, N, B))
    x = x0[:, None, :] + 0.05 * rng.standard_normal((n, N, B))
    lims = np.array([[-1.0, 1.0]] * m)
    pol = ddp.GaussianPolicy(N, n, m, K, k)
    a = ddp.forward_pass(pol, x0, u, x, ddp.DEFAULT_ALPHA, hand, lims, params=P)
    b = ddp.forward_pass(pol, x0, u, x, ddp.DEFAULT_ALPHA, ad, lims, params=P)
    for ga, gb in zip(a, b):
        assert np.array_equal(ga, gb)
    ca, cb = ddp.costfun(hand, x, u, params=P), ddp.costfun(ad, x, u, params=P)
    assert np.array_equal(ca, cb)


EVERY = r"""
// every function of the supported list, n = 6, m = 2, params = [s, w, wt]
template <class T> __device__ void dynamics(const T *x, const T *u, int i, const double *p, T *xn)
{
    xn[0] = sin(x[0]) * cos(x[1]) + tan(0.5 * x[2]) + u[0];
    xn[1] = exp(0.3 * x[3]) * log(1.5 + x[4]) + sqrt(1.0 + x[5] * x[5]) + pow(1.2 + x[0], 2.5);
    xn[2] = pow(1.1 + x[1], 3) + pow(1.3 + x[2], 1.1 + 0.2 * x[3]) + tanh(x[4]) * u[1] + pow(1.7, x[5]);
    xn[3] = sinh(0.4 * x[5]) + cosh(0.3 * x[0]) + atan(x[1] - x[2]) + atan2(x[3] + 2.0, 1.0 + x[4] * x[4]);
    xn[4] = asin(0.5 * sin(x[5])) + acos(0.4 * cos(x[0])) + fabs(x[1] - 3.0) + hypot(x[2], 1.0 + u[0] * u[0]);
    T t = fmin(x[3], 2.0 + x[4]) + fmax(x[5], -3.0) + expm1(0.2 * x[0]) + log1p(x[1] * x[1]);
    t += 0.1 * rint(2.0 * x[3]) + 1e-3 * floor(x[2] + 10.0);
    t -= x[5] / (1.0 + x[4] * x[4]);
    if (x[0] > 100.0) t *= 2;                                // a branch on the value
    xn[5] = p[0] * t;
}

template <class T> __device__ T stage_cost(const T *x, const T *u, int i, const double *p)
{
    T c = 0.0;
    for (int k = 0; k < 6; ++k) c += p[1] * x[k] * x[k];
    c += sin(x[0] * x[1]) + exp(-x[2] * x[2]) + log(2.0 + x[3] * u[0]) + sqrt(2.0 + x[4] * x[4]) + pow(1.5 + x[5], 1.5 + 0.1 * u[1]);
    c += tanh(u[0] * x[1]) + atan2(x[2], 2.0 + x[3]) + hypot(x[4], x[5] + 1.0) + cosh(0.2 * u[1]) * sinh(0.3 * x[0] + 0.1);
    c += acos(0.3 * x[1]) + asin(0.2 * u[0]) + expm1(0.1 * x[5]) * log1p(x[4] * x[4]) + atan(u[1]) + fabs(x[0] + 5.0);
    c += fmin(x[1], 10.0) + fmax(x[2], -10.0) + pow(1.1 + x[3], 2) + cos(x[4] - u[1]) / (2.0 + tan(0.2 * x[5]));
    return c;
}

template <class T> __device__ T terminal_cost(const T *x, const double *p)
{
    T t = 0.0;
    for (int k = 0; k < 6; ++k) t += p[2] * cos(x[k]) * exp(0.1 * x[k]);
    return t + sqrt(1.0 + x[0] * x[1] * x[1]);
}
"""


def test_every_function_against_central_differences(ddp):
    n, m, eps = 6, 2, 1e-5
    prob = ddp.DeviceProblem(EVERY, n, m, nparam=3, params=np.array([0.7, 0.3, 0.4]), terminal=True, autodiff=True)
    rng = np.random.default_rng(15)
    z0 = np.concatenate([rng.uniform(0.2, 0.6, n), rng.uniform(0.1, 0.4, m)])
    Z = np.repeat(z0[:, None], 1 + 2 * (n + m), axis=1)      # column 0: z0; 1 + 2k, 2 + 2k: z0 -/+ eps e_k
    for k in range(n + m):
        Z[k, 1 + 2 * k] -= eps; Z[k, 2 + 2 * k] += eps
    B, N = Z.shape[1], 2
    x = np.repeat(Z[:n, None, :], N, axis=1); u = np.repeat(Z[n:, None, :], N, axis=1)
    # values: f(z) from the rollout (x̂_1 = f(x̂_0, û_0)), the stage cost of step 0 and stage + terminal of step 1 from costfun
    xr, _, _ = ddp.forward_pass(None, x[:, 0, :], u, None, 1.0, prob, None)
    f = xr[:, 1, :]
    c = ddp.costfun(prob, x, u)
    c0, c1 = c[0], c[1] + c[2]
    fx, fu, _, _, _, cx, cu, cxx, cxu, cuu = ddp.df(prob, x, u)
    assert ddp.default_handle().last_kernel(2) == "ddp_user_df_ad"

    def cd(v):                                              # central differences in the n + m directions: [..., n + m]
        return np.stack([(v[..., 2 + 2 * k] - v[..., 1 + 2 * k]) / (2 * eps) for k in range(n + m)], axis=-1)

    def err(got, ref):
        return np.max(np.abs(got - ref)) / np.max(np.abs(ref))

    J = np.concatenate([fx[:, :, 0, 0], fu[:, :, 0, 0]], axis=1)
    assert err(J, cd(f)) < 1e-6, (J, cd(f))
    for s, cs in ((0, c0), (1, c1)):
        g = np.concatenate([cx[:, s, :], cu[:, s, :]])
        assert err(g[:, 0], cd(cs)) < 1e-6, (s, g[:, 0], cd(cs))
        H = np.block([[cxx[:, :, s, 0], cxu[:, :, s, 0]], [cxu[:, :, s, 0].T, cuu[:, :, s, 0]]])
        assert err(H, cd(g)) < 1e-6, (s, H, cd(g))
        assert np.array_equal(H, H.T)


def _solve_pair(ddp, hand, ad, x0, u0, P, **kw):
    return ddp.iLQG(hand, x0, u0, params=P, timing=False, **kw), ddp.iLQG(ad, x0, u0, params=P, timing=False, **kw)


@pytest.mark.parametrize("name", ["lq10x2", "pendcart", "car"])
def test_whole_solves_match_the_hand_written_problem(ddp, name):
    rng = np.random.default_rng(16)
    B = 256
    if name == "lq10x2":
        n, m, N = 10, 2, 200
        hand, ad = pair(ddp, "lq", n, m, 224)
        P = lq_params(rng, n, m)[0]
        x0 = rng.standard_normal((n, B)); u0 = 0.1 * rng.standard_normal((m, N, B))
    elif name == "pendcart":
        n, m, N = 4, 1, 300
        hand, ad = pair(ddp, "pendcart", n, m, 25, terminal=True)
        P = pend_params()
        x0 = 0.1 * rng.standard_normal((n, B)); u0 = 0.1 * rng.standard_normal((m, N, B))
    else:
        n, m, N = 4, 2, 150
        hand, ad = pair(ddp, "car", n, m, 9, terminal=True)
        P = car_params(rng, B)
        x0 = np.zeros((n, B)); x0[:2] = rng.uniform(0, 0.5, (2, B)); x0[2] = np.pi / 4 + rng.uniform(-0.2, 0.2, B)
        u0 = 0.1 * rng.standard_normal((m, N, B))
    (xa, ua, pa, _, _, ca, ta), (xb, ub, pb, _, _, cb, tb) = _solve_pair(ddp, hand, ad, x0, u0, P, max_iter=100)
    assert np.array_equal(ta["status"], tb["status"]) and np.array_equal(ta["iter"], tb["iter"])
    for b in range(B):
        assert relerr(xb[..., b], xa[..., b]) < 1e-8, b
        assert relerr(ub[..., b], ua[..., b]) < 1e-8, b
        assert relerr(cb[:, b], ca[:, b], 0) < 1e-8, b
