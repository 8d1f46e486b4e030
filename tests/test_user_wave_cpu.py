"""DDP_USER_WAVE (DeviceProblem(..., wave=True)) without a GPU: the programs of large user problems (n <= 64, m <= 32) compile for
gfx950 through hiprtc and contain the wave kernels in place of the lane kernels, the shapes and flag combinations outside the range
are refused before compiling, the compiler's resource records of the new kernels, the constants of the header, the loader and the
Julia binding, and the two things the GPU tests (tests/test_gpu_user_wave.py) lean on: the chain's NumPy closures against central
differences, and whole-solve cases whose iteration counts the C oracle itself keeps under a 1e-13 perturbation of the start."""
import functools
import os
import re

import numpy as np
import pytest

import ddp_amd
from ddp_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TERMINAL, CONST_HESSIAN, AUTODIFF, PLANT, SECOND, WAVE = 1, 2, 4, 8, 16, 32
REMARKS = "-Rpass-analysis=kernel-resource-usage"


def lq_nparam(n, m):
    return 2 * n * n + n * m + m * m


def lq_params(A, B, Q, R):
    return np.concatenate([A.ravel(order="F"), B.ravel(order="F"), Q.ravel(order="F"), R.ravel(order="F")])


# ------------------------------------------------------------------------ the chain of user_examples/chain_ad.hip as NumPy closures
CHAIN_P = np.array([0.02, 9.0, 0.3, 4.0, 1.0, 0.05, 2.0])       # h, k, c, kc, w, r, a


def chain_closures(p, J):
    """f(x, u, i), costfun(x, u) -> [N] and df(x, u) -> fx, fu, cx, cu, cxx, cxu, cuu of the chain with J links (n = 2 J, m = J)"""
    h, k, c, kc, w, r, a = p

    def bend(q):                                                # d_j = q_{j-1} - 2 q_j + q_{j+1}, fixed ends
        return np.concatenate([[0.0], q[:-1]]) - 2 * q + np.concatenate([q[1:], [0.0]])

    def f(x, u, i):
        q, v = x[:J], x[J:]
        d = bend(q)
        acc = -k * np.sin(q) - c * v + kc * (d + 0.5 * d ** 3) + u
        return np.concatenate([q + h * v, v + h * acc])

    def costfun(x, u):
        q, v = x[:J], x[J:]
        return (0.5 * w * (q * q + 0.1 * v * v) + a * (1 - np.cos(q))).sum(0) + 0.5 * r * (u * u).sum(0)

    def df(x, u):
        N = x.shape[1]
        n, m = 2 * J, J
        fx = np.zeros((n, n, N)); fu = np.zeros((n, m, N)); cxx = np.zeros((n, n, N))
        I = np.eye(J)
        for t in range(N):
            q = x[:J, t]
            g = kc * (1 + 1.5 * bend(q) ** 2)                   # kc d/dd (d + d^3 / 2)
            Jq = np.diag(-k * np.cos(q) - 2 * g) + g[:, None] * (np.eye(J, k=1) + np.eye(J, k=-1))
            fx[:, :, t] = np.block([[I, h * I], [h * Jq, (1 - h * c) * I]])
            fu[J:, :, t] = h * I
            cxx[:, :, t] = np.diag(np.concatenate([w + a * np.cos(q), 0.1 * w * np.ones(J)]))
        cx = np.concatenate([w * x[:J] + a * np.sin(x[:J]), 0.1 * w * x[J:]])
        cuu = np.repeat((r * np.eye(m))[:, :, None], N, axis=2)
        return fx, fu, cx, r * u, cxx, np.zeros((n, m, N)), cuu

    return f, costfun, df


def test_chain_closures_match_central_differences():
    """f, cost and every analytic derivative (the cubic spring included) at one point, at the accuracy central differences give: with a
    step of 1e-5 the truncation error is ~1e-10 and the rounding error ~1e-11 relative to O(1) values"""
    J = 5
    n, m = 2 * J, J
    rng = np.random.default_rng(0)
    f, costfun, df = chain_closures(CHAIN_P, J)
    x = np.concatenate([0.8 * rng.standard_normal(J), 0.5 * rng.standard_normal(J)])
    u = 0.5 * rng.standard_normal(m)
    z = np.concatenate([x, u])
    F = lambda z_: f(z_[:n], z_[n:], 0)
    Cf = lambda z_: float(costfun(z_[:n, None], z_[n:, None])[0])
    fx, fu, cx, cu, cxx, cxu, cuu = [a[..., 0] for a in df(x[:, None], u[:, None])]
    e = 1e-5
    E = e * np.eye(n + m)
    Jn = np.stack([(F(z + E[j]) - F(z - E[j])) / (2 * e) for j in range(n + m)], axis=1)
    gn = np.array([(Cf(z + E[j]) - Cf(z - E[j])) / (2 * e) for j in range(n + m)])
    G = lambda z_: np.concatenate([a[..., 0] for a in df(z_[:n, None], z_[n:, None])[2:4]])   # the analytic gradient
    Hn = np.stack([(G(z + E[j]) - G(z - E[j])) / (2 * e) for j in range(n + m)], axis=1)
    tol = 1e-6
    assert np.max(np.abs(Jn - np.hstack([fx, fu]))) < tol
    assert np.max(np.abs(gn - np.concatenate([cx, cu]))) < tol
    H = np.block([[cxx, cxu], [cxu.T, cuu]])
    assert np.max(np.abs(Hn - H)) < tol
    assert np.abs(fx[J:, :J]).max() > 1e-2 and np.abs(np.diff(np.diag(fx[J:, :J]))).max() > 1e-4   # the state-dependent block is there
    # and the closed form of one step
    d1 = x[0] * -2 + x[1]
    acc0 = -CHAIN_P[1] * np.sin(x[0]) - CHAIN_P[2] * x[J] + CHAIN_P[3] * (d1 + 0.5 * d1 ** 3) + u[0]
    assert abs(F(z)[J] - (x[J] + CHAIN_P[0] * acc0)) < 1e-15


# ------------------------------------------------------------- user_examples/pendcart_ad.hip: the reference of its terminal terms
PEND_PRM = np.concatenate([[9.82, 0.35, 0.01, 0.99], [np.pi, 0, 0, 0.0], np.diag([10.0, 1, 2, 1]).ravel(order="F"), [1.0]])


def pend_euler_df(p, x, u):
    """the analytic derivatives of user_examples/pendcart_ad.hip in NumPy: the Jacobian of its explicit Euler step (the registered
    pendulum family and npr.pendcart_closures take the matrix exponential instead), the quadratic cost, and at the last step the gradient
    and Hessian in x of the terminal cost on top (the convention of include/ddp_amd.h)"""
    g, l, h, d = p[:4]
    goal, Q, R = p[4:8], p[8:24].reshape(4, 4, order="F"), p[24]
    N = x.shape[1]
    fx = np.zeros((4, 4, N)); fu = np.zeros((4, 1, N))
    for t in range(N):
        fx[:, :, t] = np.eye(4)
        fx[0, 1, t] = h
        fx[1, 0, t] = h * (-g / l * np.cos(x[0, t]) - u[0, t] / l * np.sin(x[0, t]))
        fx[1, 1, t] = 1.0 - h * d
        fx[2, 3, t] = h
        fu[1, 0, t] = h * np.cos(x[0, t]) / l
        fu[3, 0, t] = h
    w = np.ones(N); w[-1] = 2.0
    cx = (0.5 * (Q + Q.T) @ (x - goal[:, None])) * w
    cxx = 0.5 * (Q + Q.T)[:, :, None] * w
    return fx, fu, cx, R * u, cxx, np.zeros((4, 1, N)), np.full((1, 1, N), R)


def test_pend_euler_df_matches_central_differences():
    """the reference the GPU test of the i == N-1 terms compares with: Jacobian of the explicit Euler step (npr.pendcart_closures' f), and
    gradient and Hessian of the stage cost, at the last step of stage plus terminal cost, against central differences (step 1e-5: ~1e-10
    truncation and ~1e-10 rounding on values up to ~30; the cost is quadratic, so its differences carry rounding only)"""
    from oracle import np_restatement as npr
    f, costfun, _ = npr.pendcart_closures()
    rng = np.random.default_rng(1)
    N = 3
    x = rng.standard_normal((4, N)); u = rng.standard_normal((1, N))
    fx, fu, cx, cu, cxx, cxu, cuu = pend_euler_df(PEND_PRM, x, u)
    e = 1e-5
    E = e * np.eye(5)
    tol = 1e-6
    for t in range(N):
        z = np.concatenate([x[:, t], u[:, t]])
        F = lambda z_: f(z_[:4].copy(), z_[4:].copy(), t)

        def Cf(z_):
            c = costfun(z_[:4, None], z_[4:, None])              # [stage, terminal] at this x
            return c[0] + (c[1] if t == N - 1 else 0.0)

        def G(z_):
            d = pend_euler_df(PEND_PRM, np.repeat(z_[:4, None], N, 1), np.repeat(z_[4:, None], N, 1))
            return np.concatenate([d[2][:, t], d[3][:, t]])
        Jn = np.stack([(F(z + E[j]) - F(z - E[j])) / (2 * e) for j in range(5)], axis=1)
        gn = np.array([(Cf(z + E[j]) - Cf(z - E[j])) / (2 * e) for j in range(5)])
        Hn = np.stack([(G(z + E[j]) - G(z - E[j])) / (2 * e) for j in range(5)], axis=1)
        assert np.max(np.abs(Jn - np.hstack([fx[:, :, t], fu[:, :, t]]))) < tol, t
        assert np.max(np.abs(gn - np.concatenate([cx[:, t], cu[:, t]]))) < tol, t
        H = np.block([[cxx[:, :, t], cxu[:, :, t]], [cxu[:, :, t].T, cuu[:, :, t]]])
        assert np.max(np.abs(Hn - H)) < tol, t
    assert np.array_equal(cxx[:, :, N - 1], 2 * cxx[:, :, 0])    # the terminal Hessian on top of the stage's


# ------------------------------------------------------------------------------------------------- whole-solve cases of the GPU tests
SOLVE_SHAPES = [(33, 2), (10, 9), (40, 12)]
SOLVE_SEEDS = {(33, 2): 11, (10, 9): 12, (40, 12): 13}
SOLVE_N, SOLVE_B = 60, 8


def solve_case(n, m):
    """A, B, Q, R, x0[n, B], u0[m, N, B] of the LQ solves at (n, m): every trajectory its own start"""
    from oracle import np_restatement as npr
    rng = np.random.default_rng(SOLVE_SEEDS[(n, m)])
    P = npr.make_lq_problem(rng, n=n, m=m, T=SOLVE_N)
    x0 = 1.0 + 0.1 * rng.standard_normal((n, SOLVE_B))
    u0 = 0.1 * rng.standard_normal((m, SOLVE_N, SOLVE_B))
    return P["A"], P["B"], P["Q"], P["R"], x0, u0


@pytest.mark.parametrize("n,m", SOLVE_SHAPES)
def test_oracle_iteration_counts_are_stable_under_perturbation(n, m):
    """the seeds of the whole-solve comparison: the oracle's own status and iteration counts do not move when x0 and u0 move by 1e-13
    relative, so a GPU solve that differs in the last digits is compared at the same iteration (no trajectory is left out there)"""
    from oracle import oracle_ctypes as oc
    A, B, Q, R, x0, u0 = solve_case(n, m)
    p = oc.make_problem("lq", n, m, SOLVE_N, A=A, B=B, Q=Q, R=R)
    rng = np.random.default_rng(99)
    for b in range(SOLVE_B):
        base = oc.ilqg(p, x0[:, b], u0[..., b])[6]
        assert base["status"] in (1, 2), (b, base["status"])
        for _ in range(2):
            xp = x0[:, b] * (1 + 1e-13 * rng.choice([-1.0, 1.0], n))
            up = u0[..., b] * (1 + 1e-13 * rng.choice([-1.0, 1.0], (m, SOLVE_N)))
            info = oc.ilqg(p, xp, up)[6]
            for key in ("status", "iter", "accepted_iter", "n_backpass"):
                assert info[key] == base[key], (b, key, info[key], base[key])


# ------------------------------------------------------------------------------------------------------------ compiling
COMPILES = [("lq", 33, 2, WAVE), ("lq", 10, 9, WAVE), ("lq_ad", 40, 12, AUTODIFF | WAVE), ("lq_ad", 40, 12, CONST_HESSIAN | AUTODIFF | WAVE),
            ("chain_ad", 64, 32, AUTODIFF | WAVE), ("chain_ad", 34, 17, AUTODIFF | WAVE), ("chain_ad", 18, 9, AUTODIFF | WAVE),
            ("pendcart_ad", 4, 1, TERMINAL | AUTODIFF | WAVE)]


def nparam_of(name, n, m):
    return {"lq": lq_nparam(n, m), "lq_ad": lq_nparam(n, m), "chain_ad": 7, "pendcart_ad": 25, "pendcart": 25}[name]


@functools.lru_cache(maxsize=None)
def compiled(name, n, m, flags):
    """rc, error, log of one compile with the compiler's resource remarks (once per module run)"""
    L = _lib.lib()
    rc = L.ddp_user_check(ddp_amd.example_source(name).encode(), n, m, nparam_of(name, n, m), flags, REMARKS.encode())
    return rc, L.ddp_last_error().decode(), L.ddp_user_compile_log().decode()


def usage(log):
    """kernel -> {record: value} of the kernel-resource-usage remarks of a hiprtc log"""
    out, cur = {}, None
    for line in log.splitlines():
        mm = re.search(r"remark: Function Name: (\w+)", line)
        if mm:
            cur = out.setdefault(mm.group(1), {})
            continue
        mm = re.search(r"remark:\s+(VGPRs|AGPRs|ScratchSize \[bytes/lane\]|LDS Size \[bytes/block\]|Occupancy \[waves/SIMD\]): (\d+)", line)
        if mm and cur is not None:
            cur[mm.group(1).split(" ")[0]] = int(mm.group(2))
    return out


@pytest.mark.parametrize("name,n,m,flags", COMPILES)
def test_wave_programs_compile_for_gfx950(name, n, m, flags):
    rc, err, log = compiled(name, n, m, flags)
    assert rc == 0, (err, log[-2000:])
    u = usage(log)
    assert "ddp_user_rollout_wave" in u and "ddp_user_rollout" not in u, sorted(u)
    assert "ddp_user_cost" in u
    if flags & AUTODIFF:
        assert "ddp_user_df_wave" in u and "ddp_user_df_ad" not in u and "ddp_user_df" not in u, sorted(u)
    else:
        assert "ddp_user_df" in u and "ddp_user_df_wave" not in u, sorted(u)
    assert ("ddp_user_hessians" in u) == bool(flags & CONST_HESSIAN)
    for k, rec in u.items():
        assert rec.get("LDS", 0) <= 64 * 1024, (k, rec)
    print(" ".join("%s %s" % (k, rec) for k, rec in sorted(u.items())))


@pytest.mark.parametrize("name,n,m,flags", [("lq", 10, 2, 0), ("lq_ad", 10, 2, AUTODIFF), ("pendcart_ad", 4, 1, TERMINAL | AUTODIFF)])
def test_programs_without_the_flag_hold_no_wave_kernel(name, n, m, flags):
    rc, err, log = compiled(name, n, m, flags)
    assert rc == 0, err
    u = usage(log)
    assert "ddp_user_rollout" in u and "ddp_user_rollout_wave" not in u and "ddp_user_df_wave" not in u, sorted(u)
    src = ddp_amd.example_source(name).encode()
    text = _lib.lib().ddp_user_program_text(src, n, m, nparam_of(name, n, m), flags, 0).decode()
    assert "rollout_wave" not in text and "DDP_WG" not in text and "DDP_WAVE" not in text
    wave = _lib.lib().ddp_user_program_text(src, n, m, nparam_of(name, n, m), flags | WAVE, 0).decode()
    assert "ddp_user_rollout_wave" in wave and "void ddp_user_rollout(" not in wave


# the program text of problems without the flag, as it was before the flag existed: (n, m, nparam, flags, diff_wrap) -> (length, sha256)
PIN_SOURCE = b"void dynamics(); void stage_cost(); void derivatives(); void terminal_cost(); void cost_hessians(); void plant();\n"
PLAIN_TEXT_PINS = {
    (10, 2, 3, 0, 0): (13102, "54898c48b244f8324363b5f6d0bc10fbd57117dbee897a5d163a53f751713714"),
    (7, 3, 5, TERMINAL | CONST_HESSIAN | PLANT, 0b101): (13101, "b6f1a258cdd9677a2a36045b571fd3321adf602bb8aabf1eeae5c7308c633ddd"),
    (4, 1, 0, TERMINAL | AUTODIFF, 1): (27670, "e9a6b2c1ee39b38bc63547b658332c9a2d447c7c2ec5f4e067832302df3ae118"),
}


@pytest.mark.parametrize("key", sorted(PLAIN_TEXT_PINS))
def test_program_text_without_the_flag_is_byte_identical(key):
    """the lane kernels' text is cut into pieces so that the wave program can leave some out; without the flag the pieces must join to
    the bytes of the undivided text.  Length and digest were taken from the library before the flag was added, with a fixed source so
    that no example file enters (a deliberate edit of the lane kernels or the AD prelude moves them, and is then re-pinned)."""
    import hashlib
    n, m, nparam, flags, wrap = key
    text = _lib.lib().ddp_user_program_text(PIN_SOURCE, n, m, nparam, flags, wrap)
    assert text is not None, _lib.lib().ddp_last_error().decode()
    assert (len(text), hashlib.sha256(text).hexdigest()) == PLAIN_TEXT_PINS[key]
    wave = _lib.lib().ddp_user_program_text(PIN_SOURCE, n, m, nparam, flags | WAVE, wrap)
    assert wave is not None and wave != text and b"ddp_user_rollout_wave" in wave


@pytest.mark.parametrize("n,m", [(64, 32), (34, 17), (18, 9)])
def test_chain_rollout_wave_does_not_spill(n, m):
    rc, err, log = compiled("chain_ad", n, m, AUTODIFF | WAVE)
    assert rc == 0, err
    rec = usage(log)["ddp_user_rollout_wave"]
    print(n, m, rec)
    assert rec["ScratchSize"] == 0, rec


def test_const_hessians_kernel_keeps_no_private_matrix():
    rc, err, log = compiled("lq_ad", 40, 12, CONST_HESSIAN | AUTODIFF | WAVE)
    assert rc == 0, err
    rec = usage(log)["ddp_user_hessians"]
    print(rec)
    assert rec["ScratchSize"] < 1024, rec                      # (a private hxx[40 * 40] alone would be 12 800 bytes)


# ------------------------------------------------------------------------------------------------------------------ refusals
def _check(src, n, m, nparam, flags):
    L = _lib.lib()
    rc = L.ddp_user_check(src.encode(), n, m, nparam, flags, None)
    return rc, L.ddp_last_error().decode()


@pytest.mark.parametrize("name,n,m,nparam,flags,causes", [
    ("lq", 65, 2, 0, WAVE, ("n = 65",)),
    ("lq", 10, 33, 0, WAVE, ("m = 33",)),
    ("lq_ad", 10, 2, 224, SECOND | AUTODIFF | WAVE, ("DDP_USER_SECOND_ORDER", "DDP_USER_WAVE")),
    ("lq", 33, 2, 0, 0, ("n = 33",)),
    ("lq", 10, 9, 0, 0, ("m = 9",)),
    ("lq", 10, 2, 4097, WAVE, ("nparam = 4097",)),
    ("lq", 10, 2, 224, 64, ("unknown flags",)),
])
def test_refusals_before_compiling(name, n, m, nparam, flags, causes):
    rc, err = _check(ddp_amd.example_source(name), n, m, nparam, flags)
    assert rc == -1, (rc, err)
    for cause in causes:
        assert cause in err, err


def test_chain_example_enforces_its_shape():
    assert "static_assert" in ddp_amd.example_source("chain_ad")
    rc, err = _check(ddp_amd.example_source("chain_ad"), 10, 4, 7, AUTODIFF | WAVE)
    assert rc == -4 and "compilation failed" in err, (rc, err)


# --------------------------------------------------------------------------------------------------- constants and the bindings
def test_header_loader_and_julia_agree():
    hdr = open(os.path.join(ROOT, "include", "ddp_amd.h")).read()
    jl = open(os.path.join(ROOT, "differentialdynamicprogramming.jl_amd", "julia", "DDPAmd.jl")).read()
    assert re.search(r"\bDDP_USER_WAVE = 32\b", hdr) and re.search(r"^#define DDP_MAX_N_USER_WAVE 64\b", hdr, flags=re.M)
    assert _lib.USER_WAVE == 32 and _lib.MAX_N_USER_WAVE == 64
    assert re.search(r"^const MAX_N_USER_WAVE = 64\b", jl, flags=re.M)
    assert re.search(r"wave::Bool=false", jl) and re.search(r"\(wave \? 32 : 0\)", jl)
    p = ddp_amd.DeviceProblem(ddp_amd.example_source("chain_ad"), 64, 32, nparam=7, autodiff=True, wave=True)
    assert p.wave and p.flags == (AUTODIFF | WAVE) and p.diff_mask == 0
    assert ddp_amd.DeviceProblem(ddp_amd.example_source("lq"), 10, 2, nparam=224).flags == 0
    with pytest.raises(ddp_amd.DDPError, match="DDP_USER_WAVE"):
        ddp_amd.DeviceProblem(ddp_amd.example_source("lq_ad"), 10, 2, nparam=224, autodiff=True, second_order=True, wave=True).check()


def test_wrapped_diff_reaches_large_problems():
    """a WrappedDiff (coordinates below 32) is kept at n > 32, the shapes the flag opens; anything else is refused there as at small n"""
    src = ddp_amd.example_source("chain_ad")
    mk = lambda n, m, diff: ddp_amd.DeviceProblem(src, n, m, nparam=7, autodiff=True, wave=True, diff=diff)
    assert mk(40, 20, ddp_amd.WrappedDiff(0)).diff_mask == 1
    assert mk(64, 32, ddp_amd.WrappedDiff(5, 31)).diff_mask == (1 << 5) | (1 << 31)
    assert mk(64, 32, None).diff_mask == 0 and mk(64, 32, np.subtract).diff_mask == 0
    with pytest.raises(TypeError, match="closure"):
        mk(40, 20, lambda a, b: a - b)
    with pytest.raises(ValueError, match="0..31"):
        ddp_amd.WrappedDiff(32)
    with pytest.raises(ValueError, match="state of length 16"):
        mk(16, 8, ddp_amd.WrappedDiff(20))
    text = _lib.lib().ddp_user_program_text(src.encode(), 64, 32, 7, AUTODIFF | WAVE, (1 << 5) | (1 << 31)).decode()
    assert "#define DDP_WRAP 0x80000020u" in text
