"""DDP_USER_WAVE on the GPU (DeviceProblem(..., wave=True)): ddp_user_rollout_wave, ddp_user_df_wave and the direct-store ddp_user_df
of large user problems (n <= 64, m <= 32) against NumPy with Python closures, the same arithmetic as the lane kernels on the shapes both
hold, composite passes, whole solves against the C oracle and a NumPy loop, the slot scheduler and the closed loop, and the refusals.
The rollout and derivative entries are called through their device flavour with sentinel-filled outputs (the method of
tests/test_gpu_forward_contract.py): what an inactive trajectory owns keeps its bits."""
import ctypes as C

import numpy as np
import pytest

from conftest import par_map, relerr
from test_user_wave_cpu import (CHAIN_P, PEND_PRM, SOLVE_B, SOLVE_N, SOLVE_SHAPES, chain_closures, lq_nparam, lq_params, pend_euler_df,
                                solve_case)

pytestmark = pytest.mark.gpu
SENT = tuple(np.uint64(0x7FF8DEAD5EED1230 + i) for i in range(8))    # quiet NaNs, a payload per output


@pytest.fixture(scope="module")
def ddp():
    import ddp_amd
    return ddp_amd


# one program per model, shape and module
_made = {}


def problem(ddp, name, n, m, **kw):
    key = (name, n, m, tuple(sorted(kw.items(), key=lambda t: t[0])))
    if key not in _made:
        nparam = {"lq": lq_nparam(n, m), "lq_ad": lq_nparam(n, m), "chain_ad": 7, "pendcart_ad": 25}[name]
        kw = dict(kw)
        wrapped = kw.pop("wrapped", False)
        if wrapped:                                                  # True: coordinate 0; a tuple: those coordinates
            kw["diff"] = ddp.WrappedDiff(*((0,) if wrapped is True else wrapped))
        _made[key] = ddp.DeviceProblem(ddp.example_source(name), n, m, nparam=nparam, autodiff=name.endswith("_ad"), **kw)
    return _made[key]


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


class Dev:
    """device buffers of one test, freed at exit"""

    def __init__(self, h):
        from ddp_amd import _lib
        self.h, self.L, self.bufs = h, _lib.lib(), []

    def alloc(self, nbytes):
        p = self.h.malloc(max(int(nbytes), 8))
        self.bufs.append(p)
        return p.value

    def copy_in(self, dst, a):
        from ddp_amd import _lib
        _lib.check(self.L.ddp_memcpy_h2d(self.h.raw, C.c_void_p(dst), a.ctypes.data_as(C.c_void_p), C.c_size_t(a.nbytes)))

    def put(self, a, dtype=np.float64):
        if a is None:
            return None
        a = np.asfortranarray(a, dtype=dtype)
        p = self.alloc(a.nbytes)
        self.copy_in(p, a)
        return p

    def sentinel(self, shape, which):
        p = self.alloc(8 * int(np.prod(shape)))
        self.copy_in(p, np.full(int(np.prod(shape)), SENT[which], np.uint64))
        return p

    def get(self, p, shape):
        return self.h.to_host(C.c_void_p(p), shape)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        for p in self.bufs:
            self.h.free(p)
        self.bufs = []


def vp(p):
    return C.c_void_p(p)


def dev_rollout(ddp, prob, prm, K, k, x0, u, x, alpha, lims, active):
    """ddp_user_forward_pass_f64_dev on sentinel-filled outputs -> xnew, unew, cnew, csum, kernel name"""
    from ddp_amd import _lib
    h = ddp.default_handle()
    n, B = x0.shape
    m, N = u.shape[:2]
    al = np.ascontiguousarray(alpha, np.float64)
    na, CL = len(al), prob.cost_len(N)
    shapes = ((n, N, B, na), (m, N, B, na), (CL, B, na), (B, na))
    with Dev(h) as d:
        outs = [d.sentinel(s, i) for i, s in enumerate(shapes)]
        ops = [d.put(a) for a in (prm, K, k, x0, u, x)]
        dl, da = d.put(lims), d.put(active, np.int32)
        _lib.check(d.L.ddp_user_forward_pass_f64_dev(h.raw, prob._ptr(h), N, B, vp(ops[0]), int(np.ndim(prm) == 2), *map(vp, ops[1:]),
                                                     al.ctypes.data_as(C.c_void_p), na, vp(dl), vp(da), *map(vp, outs)))
        h.sync()
        return [d.get(p, s) for p, s in zip(outs, shapes)] + [h.last_kernel(1)]


def dev_df(ddp, prob, prm, x, u, active):
    """ddp_user_df_f64_dev on sentinel-filled outputs -> fx, fu, cx, cu, cxx, cxu, cuu, kernel name"""
    from ddp_amd import _lib
    h = ddp.default_handle()
    n, N, B = x.shape
    m = u.shape[0]
    ht = () if prob.const_hessian else (N,)
    shapes = ((n, n, N, B), (n, m, N, B), (n, N, B), (m, N, B), (n, n) + ht + (B,), (n, m) + ht + (B,), (m, m) + ht + (B,))
    with Dev(h) as d:
        outs = [d.sentinel(s, i) for i, s in enumerate(shapes)]
        dp, dx, du, da = d.put(prm), d.put(x), d.put(u), d.put(active, np.int32)
        _lib.check(d.L.ddp_user_df_f64_dev(h.raw, prob._ptr(h), N, B, vp(dp), int(np.ndim(prm) == 2), vp(dx), vp(du), vp(da), *map(vp, outs)))
        h.sync()
        name = h.last_kernel(2)
        return [d.get(p, s) for p, s in zip(outs, shapes)] + [name]


# ------------------------------------------------------------------------------------------------ models: parameters and closures
def lq_model(rng, n, m, B, batched):
    """parameters [nparam] or [nparam, B] of lq.hip / lq_ad.hip and the closures of trajectory b"""
    cols = []
    mats = []
    for _ in range(B if batched else 1):
        A0 = rng.standard_normal((n, n))
        A = np.eye(n) + 0.05 * (A0 - A0.T) / np.sqrt(n)
        Bm = 0.1 * rng.standard_normal((n, m))
        Q0 = rng.standard_normal((n, n)); R0 = rng.standard_normal((m, m))
        Q = 0.01 * (np.eye(n) + Q0 @ Q0.T / n); R = 0.01 * (np.eye(m) + R0 @ R0.T / m)
        Q, R = 0.5 * (Q + Q.T), 0.5 * (R + R.T)
        mats.append((A, Bm, Q, R))
        cols.append(lq_params(A, Bm, Q, R))
    prm = np.stack(cols, axis=1) if batched else cols[0]

    def closures(b):
        from oracle import np_restatement as npr
        return npr.lq_closures(*mats[b if batched else 0])
    return prm, closures


def chain_model(rng, J, B, batched):
    if batched:
        prm = np.repeat(CHAIN_P[:, None], B, axis=1) * (1 + 0.2 * rng.uniform(-1, 1, (7, B)))
    else:
        prm = CHAIN_P.copy()
    return prm, (lambda b: chain_closures(prm[:, b] if batched else prm, J))


def model_of(name, rng, n, m, B, batched):
    return chain_model(rng, m, B, batched) if name == "chain_ad" else lq_model(rng, n, m, B, batched)


def holes(B):
    a = np.ones(B, np.int32)
    a[1::3] = 0
    if B > 40:
        a[30:37] = 0
    if B == 1:
        a[0] = 0
    return a


# ------------------------------------------------------------------------------------------------------------ 1. rollout contract
ROLL_SHAPES = [("lq", 33, 2), ("lq", 10, 9), ("lq_ad", 40, 12), ("chain_ad", 34, 17), ("chain_ad", 64, 32)]


@pytest.mark.parametrize("B,na", [(1, 1), (3, 11), (70, 1)])
@pytest.mark.parametrize("name,n,m", ROLL_SHAPES)
def test_rollout_contract(ddp, name, n, m, B, na):
    """every rollout of N in {1, 2, 37}, with and without a policy and limits, shared and per-trajectory parameters: active rollouts
    against npr.forward_pass with the Python closures (1e-10 per time step, csum included), NULL and all-ones masks the same bits, and
    under a mask with holes the inactive trajectories' rows of all four outputs keep the sentinel bit for bit"""
    from oracle import np_restatement as npr
    prob = problem(ddp, name, n, m, wave=True)
    alpha = 10.0 ** np.linspace(0, -3, na)
    case = 0
    for N in (1, 2, 37):
        for pol in (True, False):
            for lim in (False, True):
                case += 1
                rng = np.random.default_rng(1000 * n + 10 * B + case)
                batched = B > 1 and case % 3 != 0
                prm, closures = model_of(name, rng, n, m, B, batched)
                x0 = 0.5 * rng.standard_normal((n, B))
                u = 0.4 * rng.standard_normal((m, N, B))
                K = k = x = None
                if pol:
                    K = 0.3 * rng.standard_normal((m, n, N, B)) / np.sqrt(n); k = 0.3 * rng.standard_normal((m, N, B))
                    x = x0[:, None, :] + 0.1 * rng.standard_normal((n, N, B))
                lims = np.stack([-0.3 - 0.2 * rng.uniform(size=m), 0.3 + 0.2 * rng.uniform(size=m)], axis=1) if lim else None
                what = (N, pol, lim, batched)
                out = dev_rollout(ddp, prob, prm, K, k, x0, u, x, alpha, lims, None)
                assert out[4] == "ddp_user_rollout_wave", out[4]
                ones = dev_rollout(ddp, prob, prm, K, k, x0, u, x, alpha, lims, np.ones(B, np.int32))
                for a, b_ in zip(out[:4], ones[:4]):
                    assert np.array_equal(bits(a), bits(b_)), (what, "all ones differs from NULL")
                act = holes(B)
                got = dev_rollout(ddp, prob, prm, K, k, x0, u, x, alpha, lims, act)
                on = act != 0
                for i, a in enumerate(got[:4]):
                    assert np.all(bits(a[..., ~on, :]) == SENT[i]), (what, i, "an inactive trajectory was written")
                    assert np.array_equal(bits(a[..., on, :]), bits(out[i][..., on, :])), (what, i, "active rows differ under the mask")
                xn, un, cn, cs = out[:4]
                assert not np.isnan(xn).any() and not np.isnan(un).any() and not np.isnan(cn).any() and not np.isnan(cs).any(), what
                if lim:
                    assert np.all(un >= lims[:, 0, None, None, None]) and np.all(un <= lims[:, 1, None, None, None]), what
                for b in range(B):
                    f, costfun, _ = closures(b)
                    for ai in range(na):
                        p_ = None if not pol else (K[..., b], k[..., b])
                        xr, ur, cr = npr.forward_pass(p_, x0[:, b], u[..., b], None if not pol else x[..., b], alpha[ai], f, costfun, lims)
                        assert relerr(xn[:, :, b, ai], xr) < 1e-10 and relerr(un[:, :, b, ai], ur) < 1e-10, (what, b, ai)
                        assert relerr(cn[:, b, ai], cr, 0) < 1e-10, (what, b, ai)
                        assert abs(cs[b, ai] - cr.sum()) <= 1e-10 * abs(cr.sum()), (what, b, ai)


def test_rollout_with_terminal_cost_and_wrapped_diff(ddp):
    """pendcart_ad (4, 1) under the flag: the terminal cost in cnew[N] and csum, the wrapped difference of coordinate 0, against NumPy"""
    from oracle import np_restatement as npr
    prob = problem(ddp, "pendcart_ad", 4, 1, terminal=True, wave=True, wrapped=True)
    rng = np.random.default_rng(2)
    n, m, N, B = 4, 1, 37, 9
    x0 = np.array([0.2, 0.0, 0.0, 0.0])[:, None] + 0.05 * rng.standard_normal((n, B))
    u = 0.3 * rng.standard_normal((m, N, B))
    K = 0.2 * rng.standard_normal((m, n, N, B)); k = 0.2 * rng.standard_normal((m, N, B))
    x = x0[:, None, :] + 0.05 * rng.standard_normal((n, N, B))
    x[0] += 2 * np.pi * rng.integers(-2, 3, (N, B))
    act = holes(B)
    xn, un, cn, cs, name = dev_rollout(ddp, prob, PEND_PRM, K, k, x0, u, x, [0.5, 1.0], None, act)
    assert name == "ddp_user_rollout_wave" and cn.shape == (N + 1, B, 2)
    f, costfun, _ = npr.pendcart_closures()
    for b in range(B):
        if not act[b]:
            assert np.all(bits(cn[:, b]) == SENT[2]) and np.all(bits(cs[b]) == SENT[3])
            continue
        for ai, al in enumerate((0.5, 1.0)):
            xr, ur, cr = npr.forward_pass((K[..., b], k[..., b]), x0[:, b], u[..., b], x[..., b], al, f, costfun, None, npr.wrapped_diff(1))
            assert relerr(xn[:, :, b, ai], xr) < 1e-10 and relerr(un[:, :, b, ai], ur) < 1e-10 and relerr(cn[:, b, ai], cr, 0) < 1e-10
            assert abs(cs[b, ai] - cr.sum()) <= 1e-10 * abs(cr.sum())


@pytest.mark.parametrize("n,m,coords", [(34, 17, (0, 16)), (64, 32, (5, 31))])
def test_rollout_with_wrapped_diff_beyond_32_states(ddp, n, m, coords):
    """chain_ad with n > 32 and a WrappedDiff on joint angles (31 is the highest coordinate a mask names): the reference states sit whole
    turns away from the rollout, so a plain difference would give other controls; against npr.forward_pass with the same diff as a NumPy closure"""
    from oracle import np_restatement as npr
    prob = problem(ddp, "chain_ad", n, m, wave=True, wrapped=coords)
    assert prob.diff_mask == sum(1 << c for c in coords)
    rng = np.random.default_rng(7 + n)
    N, B = 12, 5
    prm, closures = chain_model(rng, m, B, True)
    x0 = 0.4 * rng.standard_normal((n, B)); u = 0.3 * rng.standard_normal((m, N, B))
    K = 0.3 * rng.standard_normal((m, n, N, B)) / np.sqrt(n); k = 0.3 * rng.standard_normal((m, N, B))
    x = x0[:, None, :] + 0.1 * rng.standard_normal((n, N, B))
    turns = rng.integers(-2, 3, (len(coords), N, B))
    turns[turns == 0] = 1
    x[list(coords)] += 2 * np.pi * turns

    def diff(a, b_):                                                 # (npr.wrapped_diff holds states of up to 32 coordinates)
        d = a - b_
        for c in coords:
            d[c] = np.remainder(d[c] + np.pi, 2 * np.pi) - np.pi
        return d
    xn, un, cn, cs, name = dev_rollout(ddp, prob, prm, K, k, x0, u, x, [1.0, 0.5], None, None)
    assert name == "ddp_user_rollout_wave"
    moved = 0.0
    for b in range(B):
        f, costfun, _ = closures(b)
        for ai, al in enumerate((1.0, 0.5)):
            xr, ur, cr = npr.forward_pass((K[..., b], k[..., b]), x0[:, b], u[..., b], x[..., b], al, f, costfun, None, diff)
            assert relerr(xn[:, :, b, ai], xr) < 1e-10 and relerr(un[:, :, b, ai], ur) < 1e-10 and relerr(cn[:, b, ai], cr, 0) < 1e-10, (b, ai)
            assert abs(cs[b, ai] - cr.sum()) <= 1e-10 * abs(cr.sum())
            plain = npr.forward_pass((K[..., b], k[..., b]), x0[:, b], u[..., b], x[..., b], al, f, costfun, None)[1]
            moved = max(moved, float(np.max(np.abs(plain[:, 0] - ur[:, 0]))))
    assert moved > 1e-2, moved                                       # the wrap decides the controls, from the first step on


# ------------------------------------------------------------------------------------------------------------------ 2. derivatives
def lq_df_reference(prm, n, m, x, u, b, batched):
    p = prm[:, b] if batched else prm
    A = p[:n * n].reshape(n, n, order="F"); Bm = p[n * n:n * n + n * m].reshape(n, m, order="F")
    Q = p[n * n + n * m:2 * n * n + n * m].reshape(n, n, order="F"); R = p[2 * n * n + n * m:].reshape(m, m, order="F")
    N = x.shape[1]
    rep = lambda M: np.repeat(M[:, :, None], N, axis=2)
    return rep(A), rep(Bm), Q @ x[..., b], R @ u[..., b], rep(Q), np.zeros((n, m, N)), rep(R)


@pytest.mark.parametrize("name,n,m,kw,kernel", [
    ("chain_ad", 64, 32, {}, "ddp_user_df_wave"),                  # n + m = 96: two seed rounds
    ("chain_ad", 34, 17, {}, "ddp_user_df_wave"),
    ("lq_ad", 40, 12, {}, "ddp_user_df_wave"),
    ("lq_ad", 40, 12, dict(const_hessian=True), "ddp_user_df_wave"),
    ("lq", 33, 2, {}, "ddp_user_df"),                              # hand-written `derivatives`, stored straight to memory
])
def test_derivatives_match_the_analytic_ones(ddp, name, n, m, kw, kernel):
    prob = problem(ddp, name, n, m, wave=True, **kw)
    rng = np.random.default_rng(3 + n)
    N, B = 5, 5
    batched = True
    prm, closures = model_of(name, rng, n, m, B, batched)
    x = 0.6 * rng.standard_normal((n, N, B)); u = 0.5 * rng.standard_normal((m, N, B))
    act = holes(B)
    out = dev_df(ddp, prob, prm, x, u, act)
    assert out[7] == ("ddp_user_hessians" if kw.get("const_hessian") else kernel), out[7]
    full = dev_df(ddp, prob, prm, x, u, None)
    ch = bool(kw.get("const_hessian"))
    for b in range(B):
        if not act[b]:
            for i in range(7):                                       # (the [., ., B] Hessians of a const-Hessian problem included)
                assert np.all(bits(out[i][..., b]) == SENT[i]), (b, i, "an inactive trajectory was written")
        else:
            for i in range(7):
                assert np.array_equal(bits(out[i][..., b]), bits(full[i][..., b])), (b, i)
        want = closures(b)[2](x[..., b], u[..., b]) if name == "chain_ad" else lq_df_reference(prm, n, m, x, u, b, batched)
        for i, (got, ref) in enumerate(zip(full[:7], want)):
            g = got[..., b]
            if ch and i >= 4:
                ref = ref[..., 0]
            if np.any(ref):
                assert relerr(g, ref) < 1e-10, (b, i, relerr(g, ref))
            else:
                assert not np.any(g), (b, i)
        cxx, cuu = full[4][..., b], full[6][..., b]
        assert np.array_equal(cxx, np.swapaxes(cxx, 0, 1)) and np.array_equal(cuu, np.swapaxes(cuu, 0, 1)), b


def test_terminal_terms_of_the_last_step(ddp):
    """pendcart_ad (4, 1) with DDP_USER_TERMINAL under the flag: at i == N-1 the gradient and Hessian in x of the terminal cost are added"""
    prob = problem(ddp, "pendcart_ad", 4, 1, terminal=True, wave=True, wrapped=True)
    rng = np.random.default_rng(4)
    n, m, N, B = 4, 1, 6, 4
    x = rng.standard_normal((n, N, B)); u = rng.standard_normal((m, N, B))
    out = dev_df(ddp, prob, PEND_PRM, x, u, None)
    assert out[7] == "ddp_user_df_wave"
    for b in range(B):
        want = pend_euler_df(PEND_PRM, x[..., b], u[..., b])
        for i, (got, ref) in enumerate(zip(out[:7], want)):
            if np.any(ref):
                assert relerr(got[..., b], ref) < 1e-10, (b, i, relerr(got[..., b], ref))
            else:
                assert not np.any(got[..., b]), (b, i)
        assert np.max(np.abs(out[4][:, :, N - 1, b] - 2 * out[4][:, :, 0, b])) < 1e-11      # stage Hessian Q, plus the terminal Q
        assert np.array_equal(out[4][..., b], np.swapaxes(out[4][..., b], 0, 1))


# -------------------------------------------------------------------------------------- 3. the same arithmetic on the shared shapes
@pytest.mark.parametrize("name,n,m,kw", [("lq", 10, 2, {}), ("pendcart_ad", 4, 1, dict(terminal=True, wrapped=True)), ("chain_ad", 16, 8, {})])
def test_wave_and_lane_kernels_agree_on_shared_shapes(ddp, name, n, m, kw):
    """rollout and df with wave=True against wave=False at 1e-12 (not bit for bit: the compilers may contract differently)"""
    pw, pl = problem(ddp, name, n, m, wave=True, **kw), problem(ddp, name, n, m, **kw)
    rng = np.random.default_rng(5 + n)
    N, B = 37, 7
    if name == "pendcart_ad":
        prm = PEND_PRM
    else:
        prm = model_of(name, rng, n, m, B, True)[0]
    x0 = 0.4 * rng.standard_normal((n, B)); u = 0.4 * rng.standard_normal((m, N, B))
    K = 0.3 * rng.standard_normal((m, n, N, B)) / np.sqrt(n); k = 0.3 * rng.standard_normal((m, N, B))
    x = x0[:, None, :] + 0.1 * rng.standard_normal((n, N, B))
    lims = np.array([[-0.5, 0.6]] * m)
    al = [1.0, 0.5, 0.1]
    rw = dev_rollout(ddp, pw, prm, K, k, x0, u, x, al, lims, None)
    rl = dev_rollout(ddp, pl, prm, K, k, x0, u, x, al, lims, None)
    assert rw[4] == "ddp_user_rollout_wave" and rl[4] == "ddp_user_rollout"
    for a, b_, ax in zip(rw[:4], rl[:4], (1, 1, 0, 0)):
        assert relerr(a, b_, ax) < 1e-12
    dw = dev_df(ddp, pw, prm, rl[0][..., 0], rl[1][..., 0], None)
    dl = dev_df(ddp, pl, prm, rl[0][..., 0], rl[1][..., 0], None)
    assert dw[7] != dl[7] or name == "lq"
    for i, (a, b_) in enumerate(zip(dw[:7], dl[:7])):
        assert relerr(a, b_, -2) < 1e-12, i


# ---------------------------------------------------------------------------------------------------------- 4. composite passes
@pytest.mark.parametrize("name,n,m,bp", [("chain_ad", 64, 32, "back_pass_wide"), ("lq", 33, 2, None)])
def test_composite_pass_matches_numpy(ddp, name, n, m, bp):
    """rollout, df, back_pass with limits, rollout of the new policy at α = 0.5 — as test_large_nonlinear_pass_matches_numpy"""
    from oracle import np_restatement as npr
    prob = problem(ddp, name, n, m, wave=True)
    rng = np.random.default_rng(6 + n)
    N, B = 40, 3
    prm, closures = model_of(name, rng, n, m, B, False)
    x0 = 0.4 * rng.standard_normal((n, B))
    u = 0.3 * rng.standard_normal((m, N, B))
    lims = np.array([[-1.0, 1.0]] * m)
    h = ddp.default_handle()
    x, u1, c = ddp.forward_pass(None, x0, u, None, 1.0, prob, lims, params=prm)
    assert h.last_kernel(1) == "ddp_user_rollout_wave"
    fx, fu, _, _, _, cx, cu, cxx, cxu, cuu = ddp.df(prob, x, u1, params=prm)
    assert h.last_kernel(2) == ("ddp_user_df_wave" if name == "chain_ad" else "ddp_user_df")
    div, pol, Vx, Vxx, dV = ddp.back_pass(cx, cu, cxx, cxu, cuu, fx, fu, 1.0, 1, lims, x, u1)
    ran = h.last_kernel(0)
    print("backward kernel at (%d, %d): %s" % (n, m, ran))
    if bp is not None:
        assert bp in ran, ran
    else:
        assert any(s in ran for s in ("mf2", "mfma", "big")), ran  # 32 < n <= 64, m <= 8: bp_choose's kernels for that range
    xn, un, cn = ddp.forward_pass(pol, x0, u1, x, 0.5, prob, lims, params=prm)
    f, costfun, dfn = closures(0)

    def one(b):
        xr, ur, cr = npr.forward_pass(None, x0[:, b], u[..., b], None, 1.0, f, costfun, lims)
        assert relerr(x[..., b], xr) < 1e-10 and relerr(u1[..., b], ur) < 1e-10 and relerr(c[:, b], cr, 0) < 1e-10
        want = dfn(x[..., b], u1[..., b])
        if name == "lq":
            want = lq_df_reference(prm, n, m, x, u1, b, False)
        for got, ref in zip((fx, fu, cx, cu, cxx, cxu, cuu), want):
            assert relerr(got[..., b], ref) < 1e-10
        d, (K, k, _), vx, vxx, _ = npr.back_pass(*want[2:], want[0], want[1], 1.0, 1, lims, x[..., b], u1[..., b])
        assert d == div[b] == 0
        assert relerr(pol.K[..., b], K) < 1e-8 and relerr(pol.k[..., b], k) < 1e-8 and relerr(Vxx[..., b], vxx) < 1e-8
        xr, ur, cr = npr.forward_pass((K, k), x0[:, b], u1[..., b], x[..., b], 0.5, f, costfun, lims)
        assert relerr(xn[..., b], xr) < 1e-8 and relerr(un[..., b], ur) < 1e-8 and relerr(cn[:, b], cr, 0) < 1e-8
    par_map(one, range(B))


# ------------------------------------------------------------------------------------------------------------- 5. whole solves
@pytest.mark.parametrize("n,m", SOLVE_SHAPES)
def test_lq_solves_match_the_c_oracle(ddp, n, m):
    """N = 60, 8 trajectories with their own x0 and u0: every output, status and iteration counts of every solve (the seeds are the
    ones tests/test_user_wave_cpu.py checks for iteration counts that a 1e-13 perturbation does not move)"""
    from oracle import oracle_ctypes as oc
    prob = problem(ddp, "lq_ad" if (n, m) == (40, 12) else "lq", n, m, wave=True)
    A, Bm, Q, R, x0, u0 = solve_case(n, m)
    N, B = SOLVE_N, SOLVE_B
    x, u, pol, Vx, Vxx, cost, tr = ddp.iLQG(prob, x0, u0, params=lq_params(A, Bm, Q, R), timing=False)
    h = ddp.default_handle()
    print("kernels at (%d, %d): %s %s %s" % (n, m, h.last_kernel(0), h.last_kernel(1), h.last_kernel(2)))
    assert h.last_kernel(1) == "ddp_user_rollout_wave"
    p = oc.make_problem("lq", n, m, N, A=A, B=Bm, Q=Q, R=R)

    def one(b):
        xr, ur, (K, k, _), vx, vxx, cr, info = oc.ilqg(p, x0[:, b], u0[..., b])
        assert tr["status"][b] == info["status"] and tr["iter"][b] == info["iter"], (b, tr["status"][b], info["status"])
        assert int(tr["stats"][2, b]) == info["accepted_iter"] and int(tr["stats"][3, b]) == info["n_backpass"]
        for got, ref in ((x[..., b], xr), (u[..., b], ur), (pol.K[..., b], K), (Vx[..., b], vx), (Vxx[..., b], vxx)):
            assert relerr(got, ref) < 1e-8, b
        assert relerr(pol.k[..., b], k) < 1e-6, b                 # (as test_lq_solves_match_the_c_oracle of tests/test_gpu_user_problem.py)
        assert relerr(cost[:, b], cr, 0) < 1e-8
    par_map(one, range(B))


def test_chain_solve_matches_a_numpy_loop(ddp):
    """(64, 32), N = 50, B = 4, no limits: the first five trace rows (cost, λ, α) and the trajectories after them against the NumPy
    restatement of the loop with the chain's closures"""
    from oracle import np_restatement as npr
    n, m, N, B = 64, 32, 50, 4
    prob = problem(ddp, "chain_ad", n, m, wave=True)
    rng = np.random.default_rng(8)
    x0 = np.concatenate([0.5 * rng.standard_normal((m, B)), 0.1 * rng.standard_normal((m, B))])
    u0 = 0.2 * rng.standard_normal((m, N, B))
    kw = dict(max_iter=5, tol_grad=0.0, tol_fun=-1.0)
    x, u, pol, Vx, Vxx, cost, tr = ddp.iLQG(prob, x0, u0, params=CHAIN_P, timing=False, **kw)
    h = ddp.default_handle()
    print("kernels at (64, 32): %s %s %s" % (h.last_kernel(0), h.last_kernel(1), h.last_kernel(2)))
    assert "wide" in h.last_kernel(0) and h.last_kernel(1) == "ddp_user_rollout_wave" and h.last_kernel(2) == "ddp_user_df_wave"
    H = tr["history"]
    f, costfun, dfn = chain_closures(CHAIN_P, m)

    def one(b):
        xr, ur, (K, k, _), vx, vxx, cr, info = npr.iLQG(f, costfun, dfn, x0[:, b], u0[..., b], **kw)
        t = info["trace"]
        assert len(t["cost"]) >= 5, len(t["cost"])
        for r_ in range(5):
            assert abs(H["cost"][r_, b] - t["cost"][r_]) <= 1e-8 * abs(t["cost"][r_]), (b, r_)
            assert abs(H["λ"][r_, b] - t["lam"][r_]) <= 1e-8 * t["lam"][r_], (b, r_)
            assert (np.isnan(H["α"][r_, b]) and np.isnan(t["alpha"][r_])) or H["α"][r_, b] == t["alpha"][r_], (b, r_)
        assert tr["status"][b] == info["status"] and tr["iter"][b] == info["iter"], b
        for got, ref in ((x[..., b], xr), (u[..., b], ur), (pol.K[..., b], K), (Vx[..., b], vx), (Vxx[..., b], vxx)):
            assert relerr(got, ref) < 1e-8, b
        assert relerr(cost[:, b], cr, 0) < 1e-8
    par_map(one, range(B))


# ------------------------------------------------------------------------------------------- 6. slot scheduler and closed loop
def test_queue_and_closed_loop_at_10_9(ddp):
    """(10, 9) lq with per-problem parameters.  iLQG_queue: 6 problems through 4 slots, each solve the stand-alone solve at batch size
    4 bit for bit; iLQG_mpc: 3 closed-loop steps equal the host loop over iLQG"""
    n, m, N, P = 10, 9, 30, 6
    prob = problem(ddp, "lq", n, m, wave=True)
    rng = np.random.default_rng(9)
    prm, _ = lq_model(rng, n, m, P, True)
    x0 = 1.0 + 0.2 * rng.standard_normal((n, P)); u0 = 0.1 * rng.standard_normal((m, N, P))
    lims = np.array([[-0.6, 0.6]] * m)
    q = ddp.iLQG_queue(prob, x0, u0, slots=4, lims=lims, params=prm)
    assert ddp.default_handle().last_kernel(1) == "ddp_user_rollout_wave" and ddp.default_handle().last_kernel(2) == "ddp_user_df"
    assert (q[6]["status"] > 0).all(), q[6]["status"]
    outputs = lambda r: r[:2] + (r[2].K, r[2].k) + r[3:6] + (r[6]["stats"],)
    for sel in (np.arange(0, 4), np.arange(2, 6)):                  # column sets of exactly 4 problems covering 0 .. 5
        r = ddp.iLQG(prob, x0[:, sel], u0[:, :, sel], lims=lims, params=prm[:, sel], timing=False)
        for a, b_ in zip(outputs(q), outputs(r)):
            assert np.array_equal(a[..., sel], b_, equal_nan=True), sel[0]
    B, steps = 4, 3
    kw = dict(lims=lims, max_iter=25)
    xcl, ucl, scl, xp, up_, _ = ddp.iLQG_mpc(prob, x0[:, :B], u0[..., :B], steps, params=prm[:, :B], **kw)
    xs, us = x0[:, :B].copy(), u0[..., :B].copy()
    same = lambda a, b_: np.array_equal(a, b_, equal_nan=True)
    for t in range(steps):
        r = ddp.iLQG(prob, xs, us, params=prm[:, :B], timing=False, **kw)
        assert same(scl[:, t], r[6]["stats"]), t
        assert same(xcl[:, t], r[0][:, 0]) and same(ucl[:, t], r[1][:, 0]) and same(xcl[:, t + 1], r[0][:, 1]), t
        xs = np.ascontiguousarray(r[0][:, 1])
        us = ddp.mpc_shift(r[1])
    assert same(xp, r[0]) and same(up_, r[1])
    assert (scl[0] > 0).all()


# ------------------------------------------------------------------------------------------------------------------ 7. refusals
def test_refusals_on_the_device(ddp):
    from ddp_amd import kl
    prob = problem(ddp, "lq", 33, 2, wave=True)
    n, m, N = 33, 2, 10
    rng = np.random.default_rng(10)
    prm, _ = lq_model(rng, n, m, 1, False)
    x0 = 0.1 * rng.standard_normal(n); u0 = 0.1 * rng.standard_normal((m, N))
    x, u, c = ddp.forward_pass(None, x0, u0, None, 1.0, prob, None, params=prm)
    eye = np.repeat(np.eye(m)[:, :, None], N, axis=2)
    prev = ddp.GaussianPolicy(N, n, m, np.zeros((m, n, N)), u.copy(), eye, eye.copy())
    h = ddp.default_handle()
    before = h.last_kernel(0), h.last_kernel(2)
    with pytest.raises(ddp.DDPError, match="back_pass_gps"):
        kl.iLQGkl(prob, x, prev, kl.Model(None, None, np.eye(n)), cost=c, params=prm)
    assert (h.last_kernel(0), h.last_kernel(2)) == before       # nothing was launched
    bad = ddp.DeviceProblem(ddp.example_source("lq_ad"), 10, 2, nparam=224, autodiff=True, second_order=True, wave=True)
    with pytest.raises(ddp.DDPError, match="DDP_USER_WAVE"):
        ddp.forward_pass(None, np.zeros(10), np.zeros((2, 5)), None, 1.0, bad, None, params=np.zeros(224))
