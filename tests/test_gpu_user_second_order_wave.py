"""DDP_USER_SECOND_ORDER_WAVE on the GPU: ddp_user_vhess at the large shapes against the analytic tensor of user_examples/chain_ddp_ad.hip,
ddp_user_back_pass2_wave against the NumPy restatement of backward_pass.jl:81-129 (tests/ddp2_reference.back_pass2) at the shapes where
the tiling can go wrong — (4, 2) one tile, (18, 9) n over a tile edge and m > 8, (34, 17) three n-tiles and m over a tile edge, (64, 32)
the LDS limit — against the lane kernel of DDP_USER_SECOND_ORDER and, on linear dynamics, the first-order wide kernel; whole solves, the
queue, the closed loop and compaction with the flag; the refusals.
Tolerances: 1e-8 per time step (conftest.relerr) for passes and solves, 1e-12 for AD against analytic derivatives.
The operands of a single pass are random and need not be consistent derivatives (SPD cost Hessians, fx near I); x, u and the parameters
are real: the curvature is evaluated at them."""
import functools
import os

import numpy as np
import pytest

from conftest import relerr

import ddp2_reference as d2
import ddp2_wide_cases as w2

pytestmark = pytest.mark.gpu

KERNEL = "ddp_user_back_pass2_wave"
SHAPES = [(4, 2), (18, 9), (34, 17), (64, 32)]


@pytest.fixture(scope="module")
def ddp():
    import ddp_amd
    return ddp_amd


@functools.lru_cache(maxsize=None)
def _problem(name, n, m, second=True, const_hessian=False, lane=False):
    import ddp_amd
    kw = dict(autodiff=True, const_hessian=const_hessian)
    if lane:
        kw["second_order"] = True
    else:
        kw["wave"] = True
        kw["second_order_wave"] = second
    if name == "bicycle_ad":
        return ddp_amd.DeviceProblem(ddp_amd.example_source(name), 4, 2, nparam=10, terminal=True, **kw)
    if name == "lq_ad":
        return ddp_amd.DeviceProblem(ddp_amd.example_source(name), n, m, nparam=2 * n * n + n * m + m * m, **kw)
    return ddp_amd.DeviceProblem(ddp_amd.example_source("chain_ddp_ad"), n, m, nparam=w2.NPARAM, **kw)


def chain_params(rng, B):
    """per-trajectory parameters: stiffness and torque gain differ, so batched params reach the kernel"""
    P = np.repeat(w2.CHAIN_P[:, None], B, axis=1)
    P[1] *= rng.uniform(0.8, 1.2, B)
    P[7] *= rng.uniform(0.8, 1.2, B)
    return P


def _vh_ref(T, v):
    return np.einsum("ki,kabi->abi", v, T)


def _close12(H, ref):
    return np.abs(H - ref).max() <= 1e-12 * max(np.abs(ref).max(), 1.0)


def _spd(rng, k, shape):
    A = rng.standard_normal((k, k) + shape) / np.sqrt(k)
    return np.einsum("ij...,kj...->ik...", A, A) + 0.5 * np.eye(k).reshape((k, k) + (1,) * len(shape))


def operands(rng, n, m, N, B, const_hessian=False):
    """x, u (real), and random derivative arrays shaped as ddp.df writes them: fx near I, SPD cxx and cuu, a small cxu.  The cost
    gradients are small so that Vx·fuu stays below cuu: the passes complete, and the curvature terms still move Vxx by percents"""
    x = 0.4 * rng.standard_normal((n, N, B)); u = 0.5 * rng.standard_normal((m, N, B))
    fx = np.eye(n)[:, :, None, None] + 0.3 * rng.standard_normal((n, n, N, B)) / np.sqrt(n)
    fu = 0.5 * rng.standard_normal((n, m, N, B)) / np.sqrt(n)
    cx = 0.1 * rng.standard_normal((n, N, B)); cu = 0.3 * rng.standard_normal((m, N, B))
    hs = (B,) if const_hessian else (N, B)
    cxx = _spd(rng, n, hs); cuu = _spd(rng, m, hs); cxu = 0.1 * rng.standard_normal((n, m) + hs)
    return x, u, (fx, fu, cx, cu, cxx, cxu, cuu)


def tensors(name, P, x, u):
    n, _, B = x.shape
    m = u.shape[0]
    if name == "bicycle_ad":
        return [d2.bicycle(P[:, b])[3](x[..., b], u[..., b]) for b in range(B)]
    if name == "lq_ad":
        return [np.zeros((n, n + m, n + m, x.shape[1])) for b in range(B)]
    return [w2.chain_ddp(P[:, b], m)[3](x[..., b], u[..., b]) for b in range(B)]


def reference(D, Ts, lam, regType, lims, x, u, b):
    fx, fu, cx, cu, cxx, cxu, cuu = D
    lam_b = lam[b] if np.ndim(lam) else lam
    return d2.back_pass2(cx[..., b], cu[..., b], cxx[..., b], cxu[..., b], cuu[..., b], fx[..., b], fu[..., b], Ts[b], lam_b, regType, lims,
                         x[..., b], u[..., b])


def _compare_pass(got, refs, B, tol=1e-8):
    div, pol, Vx, Vxx, dV = got
    for b in range(B):
        d, (K, k, Quu), vx, vxx, dv = refs[b]
        assert div[b] == d, (b, div[b], d)
        for name, g, r in (("K", pol.K[..., b], K), ("k", pol.k[..., b], k), ("Quu", pol.Σi[..., b], Quu), ("Vx", Vx[..., b], vx),
                           ("Vxx", Vxx[..., b], vxx)):
            e = relerr(g, r)
            assert e < tol, (b, name, e)
        assert relerr(dV[:, b], dv, 0) < tol, (b, dV[:, b], dv)


def run_pass(ddp, prob, D, lam, regType, lims, x, u, P):
    fx, fu, cx, cu, cxx, cxu, cuu = D
    return ddp.back_pass_ddp(prob, cx, cu, cxx, cxu, cuu, fx, fu, lam, regType, lims, x, u, params=P)


def model_of(n, m):
    return "bicycle_ad" if (n, m) == (4, 2) else "chain_ddp_ad"


def params_of(name, rng, B):
    return np.asfortranarray(d2.sketch_inputs(B=B)[0]) if name == "bicycle_ad" else chain_params(rng, B)


# ---------------------------------------------------------------------------------------------------------------------- vhess
@pytest.mark.parametrize("n,m", [(18, 9), (64, 32)])
def test_vhess_matches_the_analytic_contraction(ddp, n, m):
    rng = np.random.default_rng(100 + n)
    N, B = 5, 3
    prob = _problem("chain_ddp_ad", n, m)
    P = chain_params(rng, B)
    x = rng.standard_normal((n, N, B)); u = rng.standard_normal((m, N, B)); v = rng.standard_normal((n, N, B))
    H = ddp.vhess(prob, x, u, v, params=P)
    assert ddp.default_handle().last_kernel(2) == "ddp_user_vhess"
    assert H.shape == (n + m, n + m, N, B)
    assert np.array_equal(H, H.transpose(1, 0, 2, 3))
    for b in range(B):
        ref = _vh_ref(w2.chain_ddp(P[:, b], m)[3](x[..., b], u[..., b]), v[..., b])
        assert _close12(H[..., b], ref), b
    assert np.abs(H[:n, :n]).max() > 0 and np.abs(H[:n, n:]).max() > 0 and np.abs(H[n:, n:]).max() > 0


def test_vhess_active_mask_leaves_the_other_trajectories_alone(ddp):
    from ddp_amd import _lib
    rng = np.random.default_rng(23)
    n, m, N, B = 18, 9, 4, 5
    prob = _problem("chain_ddp_ad", n, m)
    P = np.asfortranarray(chain_params(rng, B))
    x = np.asfortranarray(rng.standard_normal((n, N, B))); u = np.asfortranarray(rng.standard_normal((m, N, B)))
    v = np.asfortranarray(rng.standard_normal((n, N, B)))
    act = np.array([1, 0, 1, 0, 1], dtype=np.int32)
    h = ddp.default_handle()
    dP, dx, du, dv, da = (h.to_device(a) for a in (P, x, u, v, act))
    dH = h.to_device(np.full((n + m, n + m, N, B), 7.5, order="F"))
    try:
        _lib.check(_lib.lib().ddp_user_vhess_f64_dev(h.raw, prob._ptr(h), N, B, dP, 1, dx, du, dv, da, dH))
        H = h.to_host(dH, (n + m, n + m, N, B))
    finally:
        for p in (dP, dx, du, dv, da, dH):
            h.free(p)
    for b in range(B):
        if act[b]:
            assert _close12(H[..., b], _vh_ref(w2.chain_ddp(P[:, b], m)[3](x[..., b], u[..., b]), v[..., b])), b
        else:
            assert (H[..., b] == 7.5).all(), b


# ------------------------------------------------------------------------------------------------------------------- one pass
@pytest.mark.parametrize("regType", [1, 2])
@pytest.mark.parametrize("n,m", SHAPES)
def test_one_pass_matches_the_numpy_restatement(ddp, n, m, regType):
    """no limits, every pass completes (SPD cuu), and the curvature terms move Vxx: a kernel that dropped one cannot pass"""
    from oracle import np_restatement as npr
    name = model_of(n, m)
    rng = np.random.default_rng(200 + n)
    N, B = (12 if n <= 18 else 6), 3
    P = params_of(name, rng, B)
    x, u, D = operands(rng, n, m, N, B)
    if name == "bicycle_ad":
        x += np.array([2, 2, 0, 1.0])[:, None, None]
    Ts = tensors(name, P, x, u)
    lam = 0.7
    got = run_pass(ddp, _problem(name, n, m), D, lam, regType, None, x, u, P)
    assert ddp.default_handle().last_kernel(0) == KERNEL
    refs = [reference(D, Ts, lam, regType, None, x, u, b) for b in range(B)]
    assert all(r[0] == 0 for r in refs)
    fx, fu, cx, cu, cxx, cxu, cuu = D
    for b in range(B):
        first = npr.back_pass(cx[..., b], cu[..., b], cxx[..., b], cxu[..., b], cuu[..., b], fx[..., b], fu[..., b], lam, regType, None,
                              x[..., b], u[..., b])
        assert np.abs(refs[b][3] - first[3]).max() > 1e-3 * np.abs(first[3]).max(), b
    _compare_pass(got, refs, B)
    Vxx = got[3]
    assert np.array_equal(Vxx, Vxx.transpose(1, 0, 2, 3))


def _clamp_mix(refs, m):
    """steps of the reference at which some coordinates are clamped (their row of K is zero) and some are free, and all steps"""
    mixed = total = 0
    for d, (K, k, Quu), vx, vxx, dv in refs:
        assert d == 0
        for i in range(K.shape[2] - 1):
            c = int((np.abs(K[:, :, i]).max(axis=1) == 0).sum())
            mixed += 0 < c < m
            total += 1
    return mixed, total


@pytest.mark.parametrize("regType", [1, 2])
@pytest.mark.parametrize("n,m", [(18, 9), (34, 17)])
def test_one_pass_with_limits(ddp, n, m, regType):
    """the cross-lane box-QP inside the runtime-compiled step: limits at which some coordinates clamp and some stay free at most
    steps (counted from the reference)"""
    rng = np.random.default_rng(300 + n)
    N, B = 10, 3
    P = chain_params(rng, B)
    x, u, D = operands(rng, n, m, N, B)
    lims = np.stack([-0.55 * np.ones(m), 0.55 * np.ones(m)], axis=1)
    u = np.clip(u, -0.55, 0.55)
    Ts = tensors("chain_ddp_ad", P, x, u)
    lam = 0.7
    refs = [reference(D, Ts, lam, regType, lims, x, u, b) for b in range(B)]
    mixed, total = _clamp_mix(refs, m)
    print("steps with clamped and free coordinates:", mixed, "of", total)
    assert 2 * mixed > total
    got = run_pass(ddp, _problem("chain_ddp_ad", n, m), D, lam, regType, lims, x, u, P)
    assert ddp.default_handle().last_kernel(0) == KERNEL
    _compare_pass(got, refs, B)
    # lims[0, 0] > lims[0, 1]: "no limits", decided on the device
    off = lims.copy(); off[0] = [1.0, -1.0]
    got = run_pass(ddp, _problem("chain_ddp_ad", n, m), D, lam, regType, off, x, u, P)
    _compare_pass(got, [reference(D, Ts, lam, regType, None, x, u, b) for b in range(B)], B)


def test_divergence_index_and_zero_fill(ddp):
    """an indefinite cuu at one step of one trajectory: diverge = that step (1-based), Quu of the step stored, everything at and
    before it zero; the other trajectories complete"""
    n, m, N, B = 18, 9, 9, 3
    rng = np.random.default_rng(400)
    P = chain_params(rng, B)
    x, u, D = operands(rng, n, m, N, B)
    D[6][:, :, 4, 1] = -50.0 * np.eye(m)
    Ts = tensors("chain_ddp_ad", P, x, u)
    for lims in (None, np.stack([-2.0 * np.ones(m), 2.0 * np.ones(m)], axis=1)):
        refs = [reference(D, Ts, 0.5, 1, lims, x, u, b) for b in range(B)]
        assert [r[0] for r in refs] == [0, 5, 0]
        got = run_pass(ddp, _problem("chain_ddp_ad", n, m), D, 0.5, 1, lims, x, u, P)
        _compare_pass(got, refs, B)
        div, pol, Vx, Vxx, dV = got
        assert not pol.K[..., :5, 1].any() and not pol.k[:, :5, 1].any() and not Vx[:, :5, 1].any() and not Vxx[..., :5, 1].any()
        assert not pol.Σi[..., :4, 1].any() and pol.Σi[..., 4, 1].any() and Vxx[..., 5, 1].any()


def test_active_mask_and_per_trajectory_lambda(ddp):
    from ddp_amd import _lib
    n, m, N, B = 18, 9, 7, 5
    rng = np.random.default_rng(500)
    prob = _problem("chain_ddp_ad", n, m)
    P = np.asfortranarray(chain_params(rng, B))
    x, u, D = operands(rng, n, m, N, B)
    fx, fu, cx, cu, cxx, cxu, cuu = D
    Ts = tensors("chain_ddp_ad", P, x, u)
    act = np.array([1, 0, 1, 1, 0], dtype=np.int32)
    lam = np.array([0.5, 1.0, 2.0, 4.0, 8.0])
    h = ddp.default_handle()
    F = np.asfortranarray
    ins = [h.to_device(F(a)) for a in (P, x, u, fx, fu, cx, cu, cxx, cxu, cuu, lam)]
    da = h.to_device(act)
    shapes = [(m, n, N, B), (m, N, B), (m, m, N, B), (n, N, B), (n, n, N, B), (2, B)]
    outs = [h.to_device(np.full(s, -3.25, order="F")) for s in shapes]
    ddiv = h.to_device(np.full(B, 77, dtype=np.int32))
    try:
        _lib.check(_lib.lib().ddp_user_back_pass_f64_dev(h.raw, prob._ptr(h), N, B, ins[0], 1, *ins[1:], 1, None, da, *outs, ddiv))
        K, k, Quu, Vx, Vxx, dV = (h.to_host(p, s) for p, s in zip(outs, shapes))
        div = h.to_host(ddiv, (B,), np.int32)
    finally:
        for p in ins + outs + [da, ddiv]:
            h.free(p)
    for b in range(B):
        if not act[b]:
            assert div[b] == 77 and all((a[..., b] == -3.25).all() for a in (K, k, Quu, Vx, Vxx, dV)), b
            continue
        d, (Kr, kr, Qr), vx, vxx, dv = reference(D, Ts, lam, 1, None, x, u, b)
        assert div[b] == d == 0, (b, div[b], d)
        for g, r in ((K[..., b], Kr), (k[..., b], kr), (Quu[..., b], Qr), (Vx[..., b], vx), (Vxx[..., b], vxx)):
            assert relerr(g, r) < 1e-8, b
        assert relerr(dV[:, b], dv, 0) < 1e-8


def test_second_round_of_work_groups(ddp):
    """B = 260 at (18, 9), N = 4: more work-groups than the device holds at once; every trajectory has its own scratch for H"""
    n, m, N, B = 18, 9, 4, 260
    rng = np.random.default_rng(600)
    P = chain_params(rng, B)
    x, u, D = operands(rng, n, m, N, B)
    got = run_pass(ddp, _problem("chain_ddp_ad", n, m), D, 0.7, 1, None, x, u, P)
    sel = list(range(0, B, 37)) + [B - 1]
    tens = {b: w2.chain_ddp(P[:, b], m)[3](x[..., b], u[..., b]) for b in sel}
    div, pol, Vx, Vxx, dV = got
    assert not div.any()
    for b in sel:
        d, (K, k, Quu), vx, vxx, dv = reference(D, tens, 0.7, 1, None, x, u, b)
        for g, r in ((pol.K[..., b], K), (pol.k[..., b], k), (pol.Σi[..., b], Quu), (Vx[..., b], vx), (Vxx[..., b], vxx)):
            assert relerr(g, r) < 1e-8, b


def lq_params(A, B, Q, R):
    return np.concatenate([A.ravel(order="F"), B.ravel(order="F"), Q.ravel(order="F"), R.ravel(order="F")])


@functools.lru_cache(maxsize=None)
def _lq_case():
    from oracle import np_restatement as npr
    rng = np.random.default_rng(40)
    n, m, N, B = 10, 9, 8, 3
    Pq = npr.make_lq_problem(rng, n=n, m=m, T=N)
    prm = lq_params(Pq["A"], Pq["B"], Pq["Q"], Pq["R"])
    x0 = 1.0 + 0.1 * rng.standard_normal((n, B)); u0 = 0.1 * rng.standard_normal((m, N, B))
    return n, m, N, B, prm, x0, u0


def test_const_hessian_on_a_wave_lq(ddp):
    """DDP_USER_CONST_HESSIAN: cxx / cxu / cuu [., ., B] read with time stride 0.  lq_ad (10, 9): derivative arrays from ddp.df"""
    n, m, N, B, prm, x0, u0 = _lq_case()
    prob = _problem("lq_ad", n, m, const_hessian=True)
    x, u, _ = ddp.forward_pass(ddp.GaussianPolicy(), x0, u0, None, 1.0, prob, None, params=prm)
    fx, fu, _, _, _, cx, cu, cxx, cxu, cuu = ddp.df(prob, x, u, params=prm)
    assert cxx.shape == (n, n, B) and cuu.shape == (m, m, B)
    D = (fx, fu, cx, cu, cxx, cxu, cuu)
    Ts = tensors("lq_ad", None, x, u)
    for lims in (None, np.array([[-0.05, 0.05]] * m)):
        got = run_pass(ddp, prob, D, 0.8, 1, lims, x, u, prm)
        assert ddp.default_handle().last_kernel(0) == KERNEL
        _compare_pass(got, [reference(D, Ts, 0.8, 1, lims, x, u, b) for b in range(B)], B)


# --------------------------------------------------------------------------------------------------------------- cross-checks
@pytest.mark.parametrize("lims", [None, d2.BICYCLE_LIMS], ids=["free", "lims"])
def test_bicycle_agrees_with_the_lane_kernel(ddp, lims):
    """(4, 2): the same operands through ddp_user_back_pass2 (second_order=True) and the new kernel — each within tolerance of NumPy,
    and of each other"""
    rng = np.random.default_rng(700)
    n, m, N, B = 4, 2, 12, 3
    P = params_of("bicycle_ad", rng, B)
    x, u, D = operands(rng, n, m, N, B)
    x += np.array([2, 2, 0, 1.0])[:, None, None]
    u = np.clip(0.5 * u, -0.6, 0.6)
    Ts = tensors("bicycle_ad", P, x, u)
    refs = [reference(D, Ts, 1.5, 1, lims, x, u, b) for b in range(B)]
    lane = run_pass(ddp, _problem("bicycle_ad", n, m, lane=True), D, 1.5, 1, lims, x, u, P)
    assert ddp.default_handle().last_kernel(0) == "ddp_user_back_pass2"
    wave = run_pass(ddp, _problem("bicycle_ad", n, m), D, 1.5, 1, lims, x, u, P)
    assert ddp.default_handle().last_kernel(0) == KERNEL
    _compare_pass(lane, refs, B)
    _compare_pass(wave, refs, B)
    assert (lane[0] == wave[0]).all()
    for g, r in ((wave[1].K, lane[1].K), (wave[1].k, lane[1].k), (wave[1].Σi, lane[1].Σi), (wave[2], lane[2]), (wave[3], lane[3])):
        assert relerr(g, r, -2) < 1e-8


@pytest.mark.parametrize("case", ["reg1", "reg2", "lims"])
def test_linear_dynamics_give_the_first_order_wide_pass(ddp, case):
    """lq_ad (10, 9): H = 0, so the new kernel is the wide kernel's step itself — against ddp.back_pass on the same operands"""
    n, m, N, B, prm, x0, u0 = _lq_case()
    prob = _problem("lq_ad", n, m)
    rng = np.random.default_rng(41)
    x, u, _ = ddp.forward_pass(ddp.GaussianPolicy(), x0, u0, None, 1.0, prob, None, params=prm)
    fx, fu, _, _, _, cx, cu, cxx, cxu, cuu = ddp.df(prob, x, u, params=prm)
    assert not ddp.vhess(prob, x, u, rng.standard_normal((n, N, B)), params=prm).any()
    regType = 2 if case == "reg2" else 1
    lims = np.array([[-0.05, 0.05]] * m) if case == "lims" else None
    lam = rng.uniform(0.5, 2.0, B)
    d2_, p2, Vx2, Vxx2, dV2 = ddp.back_pass_ddp(prob, cx, cu, cxx, cxu, cuu, fx, fu, lam, regType, lims, x, u, params=prm)
    assert ddp.default_handle().last_kernel(0) == KERNEL
    d1, p1, Vx1, Vxx1, dV1 = ddp.back_pass(cx, cu, cxx, cxu, cuu, fx, fu, lam, regType, lims, x, u)
    assert ddp.default_handle().last_kernel(0) == "back_pass_wide_kernel"
    assert (d1 == 0).all() and (d2_ == 0).all()
    for name, g, r in (("K", p2.K, p1.K), ("k", p2.k, p1.k), ("Quu", p2.Σi, p1.Σi), ("Vx", Vx2, Vx1), ("Vxx", Vxx2, Vxx1)):
        e = relerr(g, r, -2)
        print(case, name, e)
        assert e < 1e-8, (name, e)
    assert relerr(dV2, dV1, 0) < 1e-8


# --------------------------------------------------------------------------------------------------------------- whole solves
SOLVE_J, SOLVE_N, SOLVE_B = 9, 20, 4


@functools.lru_cache(maxsize=None)
def solve_case(B=SOLVE_B, seed=800):
    """start states for which the reference with the curvature terms takes fewer iterations than without (checked in
    test_whole_solves_match_numpy_and_take_fewer_iterations from the reference itself)"""
    rng = np.random.default_rng(seed)
    n, m = 2 * SOLVE_J, SOLVE_J
    x0 = np.concatenate([0.8 * rng.standard_normal((SOLVE_J, B)), 0.5 * rng.standard_normal((SOLVE_J, B))])
    u0 = 0.3 * rng.standard_normal((m, SOLVE_N, B))
    return x0, u0


def test_whole_solves_match_numpy_and_take_fewer_iterations(ddp):
    x0, u0 = solve_case()
    n, m, B = 2 * SOLVE_J, SOLVE_J, SOLVE_B
    prob2, prob1 = _problem("chain_ddp_ad", n, m), _problem("chain_ddp_ad", n, m, second=False)
    kw = dict(max_iter=6, tol_grad=0.0, tol_fun=-1.0)
    x, u, pol, Vx, Vxx, cost, tr = ddp.iLQG(prob2, x0, u0, lims=None, params=w2.CHAIN_P, timing=False, **kw)
    assert ddp.default_handle().last_kernel(0) == KERNEL
    H = tr["history"]
    for b in range(B):
        xr, ur, (K, k, _), vx, vxx, cr, info = w2.solve(w2.CHAIN_P, SOLVE_J, x0[:, b], u0[..., b], None, True, **kw)
        assert tr["status"][b] == info["status"] and tr["iter"][b] == info["iter"], b
        assert int(tr["stats"][3, b]) == info["n_backpass"] and int(tr["stats"][4, b]) == info["n_forward"], b
        t = info["trace"]
        for r_ in range(len(t["cost"])):
            assert abs(H["cost"][r_, b] - t["cost"][r_]) <= 1e-10 * abs(t["cost"][r_]), (b, r_)
            assert abs(H["λ"][r_, b] - t["lam"][r_]) <= 1e-12 * t["lam"][r_], (b, r_)
            assert (np.isnan(H["α"][r_, b]) and np.isnan(t["alpha"][r_])) or H["α"][r_, b] == t["alpha"][r_], (b, r_)
        for got, ref in ((x[..., b], xr), (u[..., b], ur), (pol.K[..., b], K), (Vx[..., b], vx), (Vxx[..., b], vxx)):
            assert relerr(got, ref) < 1e-8, b
        assert relerr(cost[:, b], cr, 0) < 1e-8
    # what the flag is for: default options, total iterations with and without; first the reference's own counts
    it_ref2 = sum(w2.solve(w2.CHAIN_P, SOLVE_J, x0[:, b], u0[..., b], None, True)[6]["iter"] for b in range(B))
    it_ref1 = sum(w2.solve(w2.CHAIN_P, SOLVE_J, x0[:, b], u0[..., b], None, False)[6]["iter"] for b in range(B))
    assert it_ref2 < it_ref1, (it_ref2, it_ref1)
    r2 = ddp.iLQG(prob2, x0, u0, params=w2.CHAIN_P, timing=False)
    r1 = ddp.iLQG(prob1, x0, u0, params=w2.CHAIN_P, timing=False)
    assert ddp.default_handle().last_kernel(0) == "back_pass_wide_kernel"
    it2, it1 = int(r2[6]["iter"].sum()), int(r1[6]["iter"].sum())
    print("iterations: reference", it_ref2, "with the curvature,", it_ref1, "without; GPU", it2, it1)
    assert np.isfinite(r1[5].sum(0)).all() and np.isfinite(r2[5].sum(0)).all()
    assert it2 < it1, (it2, it1)


# ------------------------------------------------------------------------------------------- queue, closed loop, compaction
def _same(a, b):
    return np.array_equal(a, b, equal_nan=True)


def _outputs(r):
    return r[:2] + (r[2].K, r[2].k, r[2].Σi) + r[3:6] + (r[6]["stats"],)


def test_queue_equals_standalone_batches_bit_for_bit(ddp):
    """6 problems through 4 slots equal the stand-alone solves at batch 4 (the kernel reads a slot's parameters through the slot map)"""
    n, m, Pn, S = 2 * SOLVE_J, SOLVE_J, 6, 4
    prob = _problem("chain_ddp_ad", n, m)
    x0, u0 = solve_case(B=8, seed=801)
    rng = np.random.default_rng(802)
    P = chain_params(rng, 8)
    kw = dict(max_iter=12)
    q = ddp.iLQG_queue(prob, x0[:, :Pn], u0[:, :, :Pn], slots=S, params=P[:, :Pn], **kw)
    assert ddp.default_handle().last_kernel(0) == KERNEL
    for sel in (np.arange(0, 4), np.arange(4, 8)):
        r = ddp.iLQG(prob, x0[:, sel], u0[:, :, sel], params=P[:, sel], timing=False, **kw)
        keep = sel < Pn
        for a, b in zip(_outputs(q), _outputs(r)):
            assert _same(a[..., sel[keep]], b[..., keep]), sel


def test_mpc_equals_the_host_loop(ddp):
    n, m, B, steps = 2 * SOLVE_J, SOLVE_J, 3, 3
    prob = _problem("chain_ddp_ad", n, m)
    x0, u0 = solve_case(B=B, seed=803)
    P = chain_params(np.random.default_rng(804), B)
    kw = dict(max_iter=8)
    xcl, ucl, scl, xp, up, git = ddp.iLQG_mpc(prob, x0, u0, steps, params=P, **kw)
    assert ddp.default_handle().last_kernel(0) == KERNEL
    xs, us = x0.copy(), u0.copy()
    assert _same(xcl[:, 0], x0)
    for t in range(steps):
        r = ddp.iLQG(prob, xs, us, params=P, timing=False, **kw)
        assert _same(scl[:, t], r[6]["stats"]), t
        assert _same(xcl[:, t], r[0][:, 0]) and _same(ucl[:, t], r[1][:, 0]) and _same(xcl[:, t + 1], r[0][:, 1]), t
        xs = np.ascontiguousarray(r[0][:, 1])
        us = ddp.mpc_shift(r[1])
    assert _same(xp, r[0]) and _same(up, r[1])


def test_compaction_leaves_solves_unchanged(ddp):
    """DDP_ILQG_COMPACT=2: the live trajectories move to smaller working sets; the kernel reads params through the composed slot map
    and H through the working set's own slots"""
    n, m, B = 2 * SOLVE_J, SOLVE_J, 8
    prob = _problem("chain_ddp_ad", n, m)
    x0, u0 = solve_case(B=B, seed=805)
    x0 = x0 * np.linspace(0.2, 2.0, B)                           # easy and hard starts: the reference's solves take 8 to 11 iterations
    P = chain_params(np.random.default_rng(806), B)
    out = {}
    for v in ("0", "2"):
        os.environ["DDP_ILQG_COMPACT"] = v
        try:
            out[v] = ddp.iLQG(prob, x0, u0, params=P, max_iter=40, timing=False)
        finally:
            del os.environ["DDP_ILQG_COMPACT"]
    it = out["0"][6]["iter"]
    assert it.max() > it.min(), it
    for a, b_ in zip(out["0"][:2] + out["0"][3:6], out["2"][:2] + out["2"][3:6]):
        assert relerr(b_, a) < 1e-12
    assert (out["0"][6]["status"] == out["2"][6]["status"]).all() and (out["0"][6]["iter"] == out["2"][6]["iter"]).all()
    assert relerr(out["2"][2].K, out["0"][2].K) < 1e-12


# ------------------------------------------------------------------------------------------------------------------ refusals
def test_kl_refuses_the_problem_and_launches_nothing(ddp):
    from ddp_amd import kl, _lib
    n, m, N = 18, 9, 5
    prob = _problem("chain_ddp_ad", n, m)
    h = ddp.default_handle()
    ddp.vhess(prob, np.zeros((n, N)), np.zeros((m, N)), np.zeros((n, N)), params=w2.CHAIN_P)
    before = [h.last_kernel(j) for j in range(5)]
    prev = ddp.GaussianPolicy(N, n, m, np.zeros((m, n, N)), np.zeros((m, N)), np.zeros((m, m, N)), np.zeros((m, m, N)))
    with pytest.raises(ddp.DDPError, match="second_order_wave=True is refused"):
        kl.iLQGkl(prob, np.zeros((n, N)), prev, None, cost=np.zeros(N), wide=True)
    prm = _lib.f64(w2.CHAIN_P)
    args = [None] * 23
    args[7] = 0                                                  # model_fx_batched
    for wide in (0, 1):
        _lib.lib().ddp_kl_set_wide(h.raw, wide)                  # (returns the previous value)
        try:
            rc = _lib.lib().ddp_user_ilqgkl_f64_dev(h.raw, prob._ptr(h), N, 1, _lib.ptr(prm), 0, *args)
        finally:
            _lib.lib().ddp_kl_set_wide(h.raw, 0)
        assert rc == -1 and "DDP_USER_SECOND_ORDER problem is refused" in _lib.lib().ddp_last_error().decode()
    assert [h.last_kernel(j) for j in range(5)] == before


def test_the_pinned_refusal_stays(ddp):
    with pytest.raises(ddp.DDPError, match="DDP_USER_WAVE"):
        p = ddp.DeviceProblem(ddp.example_source("lq_ad"), 10, 2, nparam=224, autodiff=True, second_order=True, wave=True)
        ddp.vhess(p, np.zeros((10, 3)), np.zeros((2, 3)), np.zeros((10, 3)), params=np.zeros(224))
    wave_only = _problem("chain_ddp_ad", 18, 9, second=False)
    with pytest.raises(ddp.DDPError, match="DDP_USER_SECOND_ORDER"):
        ddp.vhess(wave_only, np.zeros((18, 3)), np.zeros((9, 3)), np.zeros((18, 3)), params=w2.CHAIN_P)
