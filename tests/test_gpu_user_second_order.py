"""DDP_USER_SECOND_ORDER on the GPU: ddp_user_vhess against analytic second derivatives, ddp_user_back_pass2 against the NumPy
restatement of backward_pass.jl:81-129 (tests/ddp2_reference.py) and, on linear dynamics, against the library's first-order dispatch;
whole solves, the queue, the closed loop and compaction with the flag; and what the flag is for: fewer iterations.
Tolerances: 1e-8 per time step (conftest.relerr) for passes and solves, 1e-12 for AD against analytic derivatives, 1e-10 for the
kernel against the library's own kernels on the same operands."""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import relerr

import ddp2_reference as d2

pytestmark = pytest.mark.gpu

LIMS = d2.BICYCLE_LIMS


@pytest.fixture(scope="module")
def ddp():
    import ddp_amd
    return ddp_amd


@pytest.fixture(scope="module")
def bike(ddp):
    return ddp.DeviceProblem(ddp.example_source("bicycle_ad"), 4, 2, nparam=10, terminal=True, autodiff=True, second_order=True)


@pytest.fixture(scope="module")
def bike1(ddp):
    """the same model without the flag: iLQG"""
    return ddp.DeviceProblem(ddp.example_source("bicycle_ad"), 4, 2, nparam=10, terminal=True, autodiff=True)


@pytest.fixture(scope="module")
def chain(ddp):
    return ddp.DeviceProblem(d2.CHAIN_SOURCE, d2.CHAIN_N, d2.CHAIN_M, nparam=d2.CHAIN_NP, params=d2.CHAIN_P, autodiff=True, second_order=True)


def lq_params(A, B, Q, R):
    return np.concatenate([A.ravel(order="F"), B.ravel(order="F"), Q.ravel(order="F"), R.ravel(order="F")])


def _vh_ref(T, v):
    """Σ_k v[k, i] T[k, a, b, i]"""
    return np.einsum("ki,kabi->abi", v, T)


def _close12(H, ref):
    return np.abs(H - ref).max() <= 1e-12 * max(np.abs(ref).max(), 1.0)


def _rollouts(P, x0, u0, lims):
    """states and controls of the initial rollouts (NumPy), derivative arrays and tensors at them, stacked over the batch"""
    from oracle import np_restatement as npr
    B = P.shape[1]
    xs, us, ds, Ts = [], [], [], []
    for b in range(B):
        f, costfun, df, tens = d2.bicycle(P[:, b])
        x, u, _ = npr.forward_pass(None, x0[:, b], u0[..., b], None, 1.0, f, costfun, lims)
        xs.append(x); us.append(u); ds.append(df(x, u)); Ts.append(tens(x, u))
    stack = lambda arrs: np.stack(arrs, axis=-1)
    return stack(xs), stack(us), [stack([d[j] for d in ds]) for j in range(7)], Ts


# ------------------------------------------------------------------------------------------------------------------ 4. vhess
def test_vhess_of_the_bicycle_matches_the_analytic_tensor(ddp, bike):
    rng = np.random.default_rng(21)
    N, B = 60, 64
    P = np.repeat(d2.sketch_inputs()[0], 4, axis=1)
    P[1] = rng.uniform(0.3, 0.8, B)                              # per-trajectory wheel base: batched params reach the kernel
    x = rng.standard_normal((4, N, B)) + np.array([2, 2, 0, 1.0])[:, None, None]
    u = 0.4 * rng.standard_normal((2, N, B))
    v = rng.standard_normal((4, N, B))
    H = ddp.vhess(bike, x, u, v, params=P)
    assert ddp.default_handle().last_kernel(2) == "ddp_user_vhess"
    assert H.shape == (6, 6, N, B)
    assert np.array_equal(H, H.transpose(1, 0, 2, 3))
    for b in range(B):
        ref = _vh_ref(d2.bicycle(P[:, b])[3](x[..., b], u[..., b]), v[..., b])
        assert _close12(H[..., b], ref), b
    assert np.abs(H[3, 5]).max() > 0 and np.abs(H[5, 5]).max() > 0 and np.abs(H[2, 2]).max() > 0


def test_vhess_of_the_chain_matches_the_analytic_tensor(ddp, chain):
    rng = np.random.default_rng(22)
    N, B = 7, 5
    x = rng.standard_normal((24, N, B)); u = rng.standard_normal((4, N, B)); v = rng.standard_normal((24, N, B))
    H = ddp.vhess(chain, x, u, v)
    tens = d2.chain()[1]
    for b in range(B):
        assert _close12(H[..., b], _vh_ref(tens(x[..., b], u[..., b]), v[..., b])), b
    assert np.array_equal(H, H.transpose(1, 0, 2, 3))


def test_vhess_active_mask_leaves_the_other_trajectories_alone(ddp, bike):
    from ddp_amd import _lib
    rng = np.random.default_rng(23)
    N, B = 9, 6
    P = d2.sketch_inputs()[0][:, :B].copy(order="F")
    x = np.asfortranarray(rng.standard_normal((4, N, B))); u = np.asfortranarray(0.3 * rng.standard_normal((2, N, B)))
    v = np.asfortranarray(rng.standard_normal((4, N, B)))
    act = np.array([1, 0, 1, 1, 0, 1], dtype=np.int32)
    h = ddp.default_handle()
    dP, dx, du, dv, da = (h.to_device(a) for a in (P, x, u, v, act))
    dH = h.to_device(np.full((6, 6, N, B), 7.5, order="F"))
    try:
        _lib.check(_lib.lib().ddp_user_vhess_f64_dev(h.raw, bike._ptr(h), N, B, dP, 1, dx, du, dv, da, dH))
        H = h.to_host(dH, (6, 6, N, B))
    finally:
        for p in (dP, dx, du, dv, da, dH):
            h.free(p)
    for b in range(B):
        if act[b]:
            assert _close12(H[..., b], _vh_ref(d2.bicycle(P[:, b])[3](x[..., b], u[..., b]), v[..., b])), b
        else:
            assert (H[..., b] == 7.5).all(), b


# --------------------------------------------------------------------------------------------------------------- 5. one pass
def _compare_pass(got, refs, B, exact_div=True):
    div, pol, Vx, Vxx, dV = got
    for b in range(B):
        d, (K, k, Quu), vx, vxx, dv = refs[b]
        assert div[b] == d, (b, div[b], d)
        for name, g, r in (("K", pol.K[..., b], K), ("k", pol.k[..., b], k), ("Quu", pol.Σi[..., b], Quu), ("Vx", Vx[..., b], vx),
                           ("Vxx", Vxx[..., b], vxx)):
            e = relerr(g, r)
            assert e < 1e-8, (b, name, e)
        assert relerr(dV[:, b], dv, 0) < 1e-8, (b, dV[:, b], dv)


@pytest.mark.parametrize("regType", [1, 2])
@pytest.mark.parametrize("lims", [None, LIMS], ids=["free", "lims"])
def test_one_pass_matches_the_numpy_restatement(ddp, bike, lims, regType):
    """the 16 problems of ddp2_reference.sketch_inputs at the states of their initial rollouts.  λ = 100: every pass completes and the
    curvature terms move Vxx by a percent and more, so a kernel that dropped one cannot pass; λ = 1 and 10: some passes fail, and
    `diverge` and everything up to it must be the reference's."""
    P, x0, u0 = d2.sketch_inputs()
    B = P.shape[1]
    x, u, (fx, fu, cx, cu, cxx, cxu, cuu), Ts = _rollouts(P, x0, u0, lims)
    from oracle import np_restatement as npr
    for lam in (100.0, 10.0, 1.0):
        got = ddp.back_pass_ddp(bike, cx, cu, cxx, cxu, cuu, fx, fu, lam, regType, lims, x, u, params=P)
        assert ddp.default_handle().last_kernel(0) == "ddp_user_back_pass2"
        refs = [d2.back_pass2(cx[..., b], cu[..., b], cxx[..., b], cxu[..., b], cuu[..., b], fx[..., b], fu[..., b], Ts[b], lam, regType, lims,
                              x[..., b], u[..., b]) for b in range(B)]
        done = sum(r[0] == 0 for r in refs)
        print("lims" if lims is not None else "free", "regType", regType, "λ", lam, "complete in the reference:", done, "of", B)
        if lam == 100.0:
            assert done == B
            for b in range(B):
                first = npr.back_pass(cx[..., b], cu[..., b], cxx[..., b], cxu[..., b], cuu[..., b], fx[..., b], fu[..., b], lam, regType, lims,
                                      x[..., b], u[..., b])
                assert np.abs(refs[b][3] - first[3]).max() > 1e-2 * np.abs(first[3]).max(), b
        else:
            assert 0 < done < B
        _compare_pass(got, refs, B)


BIKE_QUADRATIC = """
template <class T> __device__ void dynamics(const T *x, const T *u, int i, const double *p, T *xnext)
{
    const double h = p[0], L = p[1];
    xnext[0] = x[0] + h * x[3] * cos(x[2]);
    xnext[1] = x[1] + h * x[3] * sin(x[2]);
    xnext[2] = x[2] + h * x[3] * tan(u[1]) / L;
    xnext[3] = x[3] + h * u[0];
}
template <class T> __device__ T stage_cost(const T *x, const T *u, int i, const double *p)
{
    const T ex = x[0] - p[2], ey = x[1] - p[3];
    return 0.5 * p[8] * (u[0] * u[0] + u[1] * u[1]) + 0.5 * p[9] * (ex * ex + ey * ey) + p[7] * x[2] * u[1];
}
__device__ void cost_hessians(const double *p, double *cxx, double *cxu, double *cuu)
{
    for (int e = 0; e < 16; ++e) cxx[e] = 0.0;
    for (int e = 0; e < 8; ++e) cxu[e] = 0.0;
    cxx[0] = cxx[5] = p[9];
    cxu[2 + 4 * 1] = p[7];
    cuu[0] = cuu[3] = p[8]; cuu[1] = cuu[2] = 0.0;
}
"""


@pytest.mark.parametrize("lims", [None, LIMS], ids=["free", "lims"])
def test_one_pass_with_constant_hessians(ddp, lims):
    """DDP_USER_CONST_HESSIAN: the kernel reads cxx / cxu / cuu [., ., B] with time stride 0 and adds the step's curvature to a fresh
    image of them every step.  Bicycle dynamics, a quadratic cost with a cxu entry; derivative arrays from ddp.df."""
    prob = ddp.DeviceProblem(BIKE_QUADRATIC, 4, 2, nparam=10, autodiff=True, const_hessian=True, second_order=True)
    P, x0, u0 = d2.sketch_inputs()
    P[7] = 0.05; P[9] = 0.5
    B = P.shape[1]
    x, u, _, Ts = _rollouts(P, x0, u0, lims)
    fx, fu, _, _, _, cx, cu, cxx, cxu, cuu = ddp.df(prob, x, u, params=P)
    assert cxx.shape == (4, 4, B) and cxu.shape == (4, 2, B)
    for lam in (100.0, 1.0):
        got = ddp.back_pass_ddp(prob, cx, cu, cxx, cxu, cuu, fx, fu, lam, 1, lims, x, u, params=P)
        refs = [d2.back_pass2(cx[..., b], cu[..., b], cxx[..., b], cxu[..., b], cuu[..., b], fx[..., b], fu[..., b], Ts[b], lam, 1, lims,
                              x[..., b], u[..., b]) for b in range(B)]
        _compare_pass(got, refs, B)


@pytest.mark.parametrize("N", [2, 3, 40])
def test_one_pass_of_the_chain(ddp, chain, N):
    """n = 24, m = 4: seven rounds of pairs per step; N = 2 (one step of the recursion) and N = 3 (one hand-over of the operands)"""
    rng = np.random.default_rng(30 + N)
    B = 4
    x = 0.5 * rng.standard_normal((24, N, B)); u = 0.5 * rng.standard_normal((4, N, B))
    fx, fu, _, _, _, cx, cu, cxx, cxu, cuu = ddp.df(chain, x, u)
    tens = d2.chain()[1]
    lims = np.array([[-1.0, 1.0]] * 4)
    for L in (None, lims):
        got = ddp.back_pass_ddp(chain, cx, cu, cxx, cxu, cuu, fx, fu, 5.0, 1, L, x, u)
        refs = [d2.back_pass2(cx[..., b], cu[..., b], cxx[..., b], cxu[..., b], cuu[..., b], fx[..., b], fu[..., b], tens(x[..., b], u[..., b]),
                              5.0, 1, L, x[..., b], u[..., b]) for b in range(B)]
        _compare_pass(got, refs, B)


def test_one_pass_with_an_active_mask_and_per_trajectory_lambda(ddp, bike):
    from ddp_amd import _lib
    P, x0, u0 = d2.sketch_inputs()
    B, N = P.shape[1], u0.shape[1]
    x, u, D, Ts = _rollouts(P, x0, u0, None)
    fx, fu, cx, cu, cxx, cxu, cuu = D
    act = (np.arange(B) % 3 != 1).astype(np.int32)
    lam = np.where(np.arange(B) % 2 == 0, 100.0, 250.0)
    h = ddp.default_handle()
    F = lambda a: np.asfortranarray(a)
    ins = [h.to_device(F(a)) for a in (P, x, u, fx, fu, cx, cu, cxx, cxu, cuu, lam)]
    da = h.to_device(act)
    shapes = [(2, 4, N, B), (2, N, B), (2, 2, N, B), (4, N, B), (4, 4, N, B), (2, B)]
    outs = [h.to_device(np.full(s, -3.25, order="F")) for s in shapes]
    ddiv = h.to_device(np.full(B, 77, dtype=np.int32))
    try:
        _lib.check(_lib.lib().ddp_user_back_pass_f64_dev(h.raw, bike._ptr(h), N, B, ins[0], 1, *ins[1:], 1, None, da, *outs, ddiv))
        K, k, Quu, Vx, Vxx, dV = (h.to_host(p, s) for p, s in zip(outs, shapes))
        div = h.to_host(ddiv, (B,), np.int32)
    finally:
        for p in ins + outs + [da, ddiv]:
            h.free(p)
    for b in range(B):
        if not act[b]:
            assert div[b] == 77 and all((a[..., b] == -3.25).all() for a in (K, k, Quu, Vx, Vxx, dV)), b
            continue
        d, (Kr, kr, Qr), vx, vxx, dv = d2.back_pass2(cx[..., b], cu[..., b], cxx[..., b], cxu[..., b], cuu[..., b], fx[..., b], fu[..., b], Ts[b],
                                                    lam[b], 1, None, x[..., b], u[..., b])
        assert div[b] == d, (b, div[b], d)
        for g, r in ((K[..., b], Kr), (k[..., b], kr), (Quu[..., b], Qr), (Vx[..., b], vx), (Vxx[..., b], vxx)):
            assert relerr(g, r) < 1e-8, b


def test_problem_without_the_flag_is_refused_and_names_the_first_order_entry(ddp, bike1):
    P, x0, u0 = d2.sketch_inputs()
    x, u, (fx, fu, cx, cu, cxx, cxu, cuu), _ = _rollouts(P, x0, u0, None)
    with pytest.raises(ddp.DDPError, match="ddp_back_pass_f64"):
        ddp.back_pass_ddp(bike1, cx, cu, cxx, cxu, cuu, fx, fu, 1.0, 1, None, x, u, params=P)
    with pytest.raises(ddp.DDPError, match="DDP_USER_SECOND_ORDER"):
        ddp.vhess(bike1, x, u, x, params=P)


def test_kl_entry_refuses_the_flag_in_the_library(ddp, bike):
    from ddp_amd import _lib
    h = ddp.default_handle()
    prm = _lib.f64(d2.sketch_inputs()[0][:, 0])                 # refused before anything is read
    args = [None] * 23
    args[7] = 0                                                  # model_fx_batched
    rc = _lib.lib().ddp_user_ilqgkl_f64_dev(h.raw, bike._ptr(h), 5, 1, _lib.ptr(prm), 0, *args)
    assert rc == -1 and "DDP_USER_SECOND_ORDER problem is refused" in _lib.lib().ddp_last_error().decode()


# ------------------------------------------------------------------------------------------------ 6. linear dynamics: H = 0
@pytest.mark.parametrize("case", ["reg1", "reg2", "lims"])
def test_linear_dynamics_give_the_librarys_first_order_pass(ddp, case):
    """lq_ad, n = 10, m = 2, N = 1000, B = 64: the curvature is exactly zero, so the new kernel is the Riccati step itself — against
    the library's own dispatch on the same operands"""
    from oracle import np_restatement as npr
    rng = np.random.default_rng(40)
    n, m, N, B = 10, 2, 1000, 64
    Pq = npr.make_lq_problem(rng, T=N)
    prm = lq_params(Pq["A"], Pq["B"], Pq["Q"], Pq["R"])
    lq2 = ddp.DeviceProblem(ddp.example_source("lq_ad"), n, m, nparam=224, params=prm, autodiff=True, second_order=True)
    x0 = 1.0 + 0.1 * rng.standard_normal((n, B)); u0 = 0.1 * rng.standard_normal((m, N, B))
    x, u, _ = ddp.forward_pass(ddp.GaussianPolicy(), x0, u0, None, 1.0, lq2, None)
    fx, fu, _, _, _, cx, cu, cxx, cxu, cuu = ddp.df(lq2, x, u)
    assert not ddp.vhess(lq2, x, u, rng.standard_normal((n, N, B))).any()
    regType = 2 if case == "reg2" else 1
    lims = np.array([[-0.3, 0.3]] * 2) if case == "lims" else None
    lam = rng.uniform(0.5, 2.0, B)
    d2_, p2, Vx2, Vxx2, dV2 = ddp.back_pass_ddp(lq2, cx, cu, cxx, cxu, cuu, fx, fu, lam, regType, lims, x, u)
    assert ddp.default_handle().last_kernel(0) == "ddp_user_back_pass2"
    d1, p1, Vx1, Vxx1, dV1 = ddp.back_pass(cx, cu, cxx, cxu, cuu, fx, fu, lam, regType, lims, x, u)
    assert ddp.default_handle().last_kernel(0) != "ddp_user_back_pass2"
    assert (d1 == 0).all() and (d2_ == 0).all()
    for name, g, r in (("K", p2.K, p1.K), ("k", p2.k, p1.k), ("Quu", p2.Σi, p1.Σi), ("Vx", Vx2, Vx1), ("Vxx", Vxx2, Vxx1)):
        e = relerr(g, r, -2)
        print(case, name, e)
        assert e < 1e-10, (name, e)
    assert relerr(dV2, dV1, 0) < 1e-10


# ------------------------------------------------------------------------------------------------------------ 7. whole solves
def test_bicycle_solves_match_numpy(ddp, bike):
    """B = 16, N = 60, no limits, 8 accepted iterations with the tolerances off (the protocol of test_car_solves_match_numpy): status,
    counters and every output against np_restatement.iLQG with back_pass2 in place of its backward pass"""
    P, x0, u0 = d2.sketch_inputs()
    B = P.shape[1]
    kw = dict(max_iter=8, tol_grad=0.0, tol_fun=-1.0)
    x, u, pol, Vx, Vxx, cost, tr = ddp.iLQG(bike, x0, u0, lims=None, params=P, timing=False, **kw)
    assert ddp.default_handle().last_kernel(0) == "ddp_user_back_pass2"
    for b in range(B):
        xr, ur, (K, k, _), vx, vxx, cr, info = d2.solve(P[:, b], x0[:, b], u0[..., b], None, True, **kw)
        assert tr["status"][b] == info["status"] and tr["iter"][b] == info["iter"], b
        assert int(tr["stats"][3, b]) == info["n_backpass"] and int(tr["stats"][4, b]) == info["n_forward"], b
        for got, ref in ((x[..., b], xr), (u[..., b], ur), (pol.K[..., b], K), (Vx[..., b], vx), (Vxx[..., b], vxx)):
            assert relerr(got, ref) < 1e-8, b
        assert relerr(cost[:, b], cr, 0) < 1e-8


def _np_iteration_row(f, costfun, dfn, x0, x, u, lims, lam, dlam, lam_max=1e10, lam_min=1e-6, lf=1.6):
    """one iteration of the reference from the trajectory (x, u), as in test_gpu_user_problem.py; np_restatement.back_pass is the
    swapped one while this runs"""
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


def test_bicycle_solves_with_limits_match_numpy_up_to_box_qp_ties(ddp, bike):
    """the parting protocol of test_car_solves_with_limits_match_numpy_up_to_box_qp_ties with its cap: every trace row agrees until the
    two part; a trajectory may part only where the reference itself, run on the GPU's state, reproduces the GPU's row"""
    P, x0, u0 = d2.sketch_inputs()
    B = P.shape[1]
    lims = LIMS
    kw = dict(tol_grad=0.0, tol_fun=-1.0)
    x, u, pol, Vx, Vxx, cost, tr = ddp.iLQG(bike, x0, u0, lims=lims, params=P, timing=False, max_iter=8, **kw)
    H = tr["history"]
    st = tr["stats"]
    runs = {}

    def gpu_state(acc):
        if acc not in runs:
            runs[acc] = ddp.iLQG(bike, x0, u0, lims=lims, params=P, timing=False, max_iter=acc, **kw)
        return runs[acc]

    parted = 0
    for b in range(B):
        f, costfun, dfn, tens = d2.bicycle(P[:, b])
        xr, ur, (K, k, _), vx, vxx, cr, info = d2.solve(P[:, b], x0[:, b], u0[..., b], lims, True, max_iter=8, **kw)
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
        print("trajectory", b, "parts at trace row", split)
        acc = int(np.sum(~np.isnan(H["α"][:split, b])))
        assert acc >= 1, b
        xg, ug = gpu_state(acc)[0][..., b], gpu_state(acc)[1][..., b]
        xa, ua, _, _, _, _, _ = d2.solve(P[:, b], x0[:, b], u0[..., b], lims, True, max_iter=acc, **kw)
        assert relerr(xg, xa) < 1e-11 and relerr(ug, ua) < 1e-11, b
        lam, dlam = H["λ"][split - 1, b], H["dλ"][split - 1, b]
        with d2.swapped_back_pass(tens):
            on_gpu = _np_iteration_row(f, costfun, dfn, x0[:, b], xg, ug, lims, lam, dlam)
            on_np = _np_iteration_row(f, costfun, dfn, x0[:, b], xa, ua, lims, lam, dlam)
        assert on_np is not None and _rows_agree(on_np, (t["lam"][split], t["alpha"][split], t["cost"][split], t["g_norm"][split])), b
        assert on_gpu is not None and _rows_agree(on_gpu, (H["λ"][split, b], H["α"][split, b], H["cost"][split, b], H["grad_norm"][split, b])), b
        assert not _rows_agree(on_gpu, on_np), b
    print("parted:", parted, "of", B)
    assert parted <= B // 4, parted


# ---------------------------------------------------------------------------------------- 8. queue, closed loop, compaction
def _same(a, b):
    return np.array_equal(a, b, equal_nan=True)


def _outputs(r):
    return r[:2] + (r[2].K, r[2].k, r[2].Σi) + r[3:6] + (r[6]["stats"],)


def _bike_batch(P_):
    P4, x4, u4 = d2.sketch_inputs(seed=12, B=P_)
    return P4, x4, u4


def test_queue_equals_standalone_batches_bit_for_bit(ddp, bike):
    """64 bicycle solves through 16 slots: every output of every problem is the stand-alone solve's at batch 16, whichever slot it ran
    on (the new kernel reads a slot's parameters through the slot map)"""
    Pn, S = 64, 16
    P, x0, u0 = _bike_batch(Pn)
    kw = dict(max_iter=40)
    q = ddp.iLQG_queue(bike, x0, u0, slots=S, params=P, **kw)
    assert ddp.default_handle().last_kernel(0) == "ddp_user_back_pass2"
    iters = q[6]["iter"]
    assert iters.max() > iters.min()
    for c in range(0, Pn, S):
        sel = np.arange(c, c + S)
        r = ddp.iLQG(bike, x0[:, sel], u0[:, :, sel], params=P[:, sel], timing=False, **kw)
        for a, b in zip(_outputs(q), _outputs(r)):
            assert _same(a[..., sel], b), c


def test_mpc_equals_the_host_loop(ddp, bike):
    B, steps = 6, 5
    P, x0, u0 = _bike_batch(B)
    kw = dict(max_iter=15)
    xcl, ucl, scl, xp, up, git = ddp.iLQG_mpc(bike, x0, u0, steps, params=P, **kw)
    assert ddp.default_handle().last_kernel(0) == "ddp_user_back_pass2"
    xs, us = x0.copy(), u0.copy()
    assert _same(xcl[:, 0], x0)
    for t in range(steps):
        r = ddp.iLQG(bike, xs, us, params=P, timing=False, **kw)
        assert _same(scl[:, t], r[6]["stats"]), t
        assert _same(xcl[:, t], r[0][:, 0]) and _same(ucl[:, t], r[1][:, 0]) and _same(xcl[:, t + 1], r[0][:, 1]), t
        xs = np.ascontiguousarray(r[0][:, 1])
        us = ddp.mpc_shift(r[1])
    assert _same(xp, r[0]) and _same(up, r[1])


def test_compaction_leaves_second_order_solves_unchanged(ddp, bike):
    """DDP_ILQG_COMPACT=2: the live trajectories move to smaller working sets several times; the new kernel reads params through the
    composed slot map"""
    B = 96
    P, x0, u0 = _bike_batch(B)
    out = {}
    for v in ("0", "2"):
        os.environ["DDP_ILQG_COMPACT"] = v
        try:
            out[v] = ddp.iLQG(bike, x0, u0, params=P, max_iter=60, timing=False)
        finally:
            del os.environ["DDP_ILQG_COMPACT"]
    it = out["0"][6]["iter"]
    assert it.max() > it.min() + 3, it                          # trajectories end at different times: the working set shrinks
    for a, b_ in zip(out["0"][:2] + out["0"][3:6], out["2"][:2] + out["2"][3:6]):
        assert relerr(b_, a) < 1e-12
    assert (out["0"][6]["status"] == out["2"][6]["status"]).all() and (out["0"][6]["iter"] == out["2"][6]["iter"]).all()
    assert relerr(out["2"][2].K, out["0"][2].K) < 1e-12


# ------------------------------------------------------------------------------------------------------------- 9. behaviour
def test_second_order_halves_the_iterations(ddp, bike, bike1):
    """the 16 default-option solves: in the NumPy reference 337 iterations with the curvature terms against 1 189 without; the bound
    (half) leaves a factor 1.75"""
    P, x0, u0 = d2.sketch_inputs()
    r1 = ddp.iLQG(bike1, x0, u0, params=P, timing=False)
    r2 = ddp.iLQG(bike, x0, u0, params=P, timing=False)
    it1, it2 = r1[6]["iter"], r2[6]["iter"]
    print("iterations without the flag", int(it1.sum()), list(it1), "with", int(it2.sum()), list(it2))
    assert np.isfinite(r1[5].sum(0)).all() and np.isfinite(r2[5].sum(0)).all()
    assert 2 * it2.sum() <= it1.sum(), (it2.sum(), it1.sum())
