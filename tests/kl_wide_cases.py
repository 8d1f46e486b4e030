"""Seeded cases of the wide KL path (kl.* with wide=True: n <= 64, m <= 32), shared by tests/test_kl_wide_cpu.py and
tests/test_gpu_kl_wide.py.  No tests here.  Every reference is the C oracle's (oracle.oracle_ctypes), computed once per case.

Single pass: the recipe of test_gps_mid_matches_oracle (tests/test_gpu_user_kl.py) — N = 12, B = 3, limits (-0.3, 0.25), six
configurations (shared or per-trajectory dynamics and cost, η per trajectory or per step, one trajectory whose cuu[:,:,6] = -1e3 I makes
Quu indefinite there) — at shapes on the tile (16) and lane (32, 64) edges.
Loops: _lq_setup of that file with B = 3, u scaled per trajectory and clipped to the limits."""
import functools

import numpy as np

RTOL = 1e-8
N1, B1 = 12, 3
SHAPES = [(5, 9), (33, 1), (17, 32), (34, 17), (48, 8), (64, 32)]
SMALL = [(4, 1), (10, 2), (32, 8)]                       # the three-way check: wide kernels, default kernels, oracle
# (fx per trajectory, cost per trajectory, limits, η per step, indefinite step)
CONFIGS = [(1, 1, False, False, False), (0, 1, True, False, False), (1, 0, False, True, False), (0, 0, True, True, False),
           (1, 1, False, False, True), (1, 1, True, True, True)]
LIMS1 = (-0.3, 0.25)

LOOP_B, LOOP_KL_STEP, LOOP_MAX_ITER, LOOP_LIM = 3, 2e-4, 40, 0.2
LOOPS = [(12, 12, 40, False), (40, 4, 40, False), (33, 9, 30, False), (64, 32, 24, False),
         (12, 12, 40, True), (33, 9, 30, True), (36, 3, 30, True), (64, 32, 24, True)]
USER_LOOPS = [(33, 9, 30), (12, 12, 40)]
TIE_EPS, TIE_DRAWS = 1e-13, 8


def _spd(rng, d, s=1.0):
    a = rng.standard_normal((d, d))
    return s * (a @ a.T / d + 0.5 * np.eye(d))


@functools.lru_cache(maxsize=None)
def single_pass(n, m, N=N1, B=B1):
    rng = np.random.default_rng(100 * n + m)
    c = dict(n=n, m=m, N=N, B=B)
    c["fx"] = np.stack([np.stack([np.eye(n) + 0.1 * rng.standard_normal((n, n)) for _ in range(N)], -1) for _ in range(B)], -1)
    c["fu"] = 0.3 * rng.standard_normal((n, m, N, B))
    c["cxx"] = np.stack([np.stack([_spd(rng, n) for _ in range(N)], -1) for _ in range(B)], -1)
    c["cuu"] = np.stack([np.stack([_spd(rng, m, 0.5) for _ in range(N)], -1) for _ in range(B)], -1)
    c["cxu"] = 0.05 * rng.standard_normal((n, m, N, B))
    c["cx"], c["cu"] = rng.standard_normal((n, N, B)), rng.standard_normal((m, N, B))
    c["u"], c["x"] = 0.3 * rng.standard_normal((m, N, B)), rng.standard_normal((n, N, B))
    c["Kp"], c["kp"] = 0.2 * rng.standard_normal((m, n, N, B)), 0.1 * rng.standard_normal((m, N, B))
    c["Sip"] = np.stack([np.stack([_spd(rng, m, 2.0) for _ in range(N)], -1) for _ in range(B)], -1)
    c["Sp"] = np.stack([np.stack([np.linalg.inv(c["Sip"][:, :, t, b]) for t in range(N)], -1) for b in range(B)], -1)
    c["lims"] = np.stack([LIMS1[0] * np.ones(m), LIMS1[1] * np.ones(m)], 1)
    return c


def operands(c, cfg):
    """the arrays of one configuration as kl.back_pass_gps takes them (batched), and the η bracket"""
    fx_b, cost_b, lims_on, eta_tv, bad = cfg
    N, B, m = c["N"], c["B"], c["m"]
    fx, fu = (c["fx"], c["fu"]) if fx_b else (c["fx"][..., 0], c["fu"][..., 0])
    cxx, cxu, cuu = (c["cxx"], c["cxu"], c["cuu"].copy()) if cost_b else (c["cxx"][..., 0], c["cxu"][..., 0], c["cuu"][..., 0].copy())
    etab = np.stack([1e-8 * np.ones(B), np.array([1.0, 0.5, 2.0])[:B], 1e16 * np.ones(B)])
    if eta_tv:
        etab = np.repeat(etab[:, None, :], N, 1) * (1.0 + 0.1 * np.arange(N))[None, :, None]
    if bad:                                       # Quu indefinite at step 6 of trajectory 1
        cuu = c["cuu"].copy()
        cuu[:, :, 6, 1] = -1e3 * np.eye(m)
        cxx, cxu, fx, fu = c["cxx"], c["cxu"], c["fx"], c["fu"]
    return dict(fx=fx, fu=fu, cxx=cxx, cxu=cxu, cuu=cuu, etab=etab, lims=c["lims"] if lims_on else None)


def _per_traj(c, cfg, o, b):
    fx_b, cost_b, lims_on, eta_tv, bad = cfg
    sl = (lambda a: a[..., b]) if (cost_b or bad) else (lambda a: a)                                            # noqa: E731
    fl = (lambda a: a[..., b]) if (fx_b or bad) else (lambda a: a)                                              # noqa: E731
    eb = o["etab"][:, :, b] if eta_tv else o["etab"][:, b]
    return sl(o["cxx"]), sl(o["cxu"]), sl(o["cuu"]), fl(o["fx"]), fl(o["fu"]), eb


def _gps_reference(mod, n, m, ci):
    c, cfg = single_pass(n, m), CONFIGS[ci]
    o = operands(c, cfg)
    out = []
    for b in range(c["B"]):
        cxx, cxu, cuu, fx, fu, eb = _per_traj(c, cfg, o, b)
        terms = (mod.kl_terms if hasattr(mod, "kl_terms") else mod.grad_kl)(c["Kp"][..., b], c["kp"][..., b], c["Sip"][..., b])
        d, pol, vx, vxx, dv = mod.back_pass_gps(c["cx"][..., b], c["cu"][..., b], cxx, cxu, cuu, fx, fu, o["lims"], c["x"][..., b],
                                                c["u"][..., b], (terms, eb))
        K, k, Quui, Quu = pol if isinstance(pol, tuple) else (pol["K"], pol["k"], pol["S"], pol["Si"])
        out.append(dict(diverge=int(d), K=K, k=k, Quui=Quui, Quu=Quu, Vx=vx, Vxx=vxx, dV=np.asarray(dv)))
    return out


@functools.lru_cache(maxsize=None)
def gps_reference(n, m, ci):
    """the C oracle's back_pass_gps of configuration ci, one dict per trajectory"""
    from oracle import oracle_ctypes as oc
    return _gps_reference(oc, n, m, ci)


def gps_reference_numpy(n, m, ci):
    from oracle import np_kl
    return _gps_reference(np_kl, n, m, ci)


def clamped_share(n, m, ci):
    """share of the controls k[:, i] of the completed steps that the reference leaves on a bound (k = lims - u there)"""
    c, o = single_pass(n, m), operands(single_pass(n, m), CONFIGS[ci])
    if o["lims"] is None:
        return None
    hit = tot = 0
    for b, r in enumerate(gps_reference(n, m, ci)):
        first = r["diverge"]                       # steps before the failing one are zero-filled
        for i in range(first, c["N"] - 1):
            ki, ui = r["k"][:, i], c["u"][:, i, b]             # the box-QP returns a bound itself: lims - u, bit for bit
            hit += int(np.sum((ki == o["lims"][:, 0] - ui) | (ki == o["lims"][:, 1] - ui)))
            tot += c["m"]
    return hit / max(tot, 1)


# ------------------------------------------------------------------------------------------------------------------------- loops
@functools.lru_cache(maxsize=None)
def loop_case(n, m, T, lims_on):
    import scipy.linalg as sla
    rng = np.random.default_rng(31 + n + m)
    B, h = LOOP_B, 0.01
    A0 = rng.standard_normal((n, n)); A = sla.expm(h * (A0 - A0.T)); Bm = h * rng.standard_normal((n, m))
    Q, R = h * np.eye(n), 0.1 * h * np.eye(m)
    u = 0.1 * rng.standard_normal((m, T, B)) * np.linspace(0.5, 3.0, B)
    L = np.stack([-LOOP_LIM * np.ones(m), LOOP_LIM * np.ones(m)], 1) if lims_on else None
    if lims_on:
        u = np.clip(u, -LOOP_LIM, LOOP_LIM)
    x = np.zeros((n, T, B)); x[:, 0, :] = 1.0 + 0.1 * rng.standard_normal((n, B))
    for t in range(T - 1):
        x[:, t + 1, :] = A @ x[:, t, :] + Bm @ u[:, t, :]
    cost0 = 0.5 * np.einsum("itb,ij,jtb->b", x, Q, x) + 0.5 * np.einsum("itb,ij,jtb->b", u, R, u)
    eye = np.repeat(np.repeat(np.eye(m)[:, :, None, None], T, 2), B, 3)
    return dict(n=n, m=m, T=T, B=B, A=A, Bm=Bm, Q=Q, R=R, u=u, x=x, cost0=cost0, eye=eye, lims=L, R1=1e-4 * np.eye(n),
                fx=np.repeat(A[:, :, None], T, 2), fu=np.repeat(Bm[:, :, None], T, 2))


def _oracle_loop(c, b, x, u):
    from oracle import oracle_ctypes as oc
    n, m, T = c["n"], c["m"], c["T"]
    p = oc.make_problem("lq", n, m, T, A=c["A"], B=c["Bm"], Q=c["Q"], R=c["R"])
    pb = dict(K=np.zeros((m, n, T)), k=u, S=c["eye"][..., b], Si=c["eye"][..., b])
    return oc.ilqgkl(p, x, float(c["cost0"][b]), pb, dict(fx=c["fx"], R1=c["R1"]), kl_step=LOOP_KL_STEP, max_iter=LOOP_MAX_ITER, lims=c["lims"])


@functools.lru_cache(maxsize=None)
def loop_reference(n, m, T, lims_on):
    """the C oracle's iLQGkl of every trajectory: (x, u, policy, Vx, Vxx, cost, info)"""
    c = loop_case(n, m, T, lims_on)
    return [_oracle_loop(c, b, c["x"][..., b], c["u"][..., b]) for b in range(c["B"])]


def outcome(info):
    return (info["status"], info["iter"], info["n_backpass"])


def loop_outcomes_nearby(n, m, T, lims_on, b, seed):
    """the oracle's outcomes of TIE_DRAWS copies of trajectory b whose x, u are off by TIE_EPS relative (reference_outcomes_nearby of
    tests/wide_controls_cases.py): where they differ from the unperturbed outcome the REFERENCE is discontinuous at this input"""
    c = loop_case(n, m, T, lims_on)
    rng = np.random.default_rng(seed)
    xb, ub = c["x"][..., b], c["u"][..., b]
    return [outcome(_oracle_loop(c, b, xb * (1 + TIE_EPS * rng.standard_normal(xb.shape)), ub * (1 + TIE_EPS * rng.standard_normal(ub.shape)))[6])
            for _ in range(TIE_DRAWS)]


def loop_bound_share(n, m, T, b):
    """share of the controls of trajectory b the reference's solve with limits ends on a bound"""
    u = loop_reference(n, m, T, True)[b][1]
    return float(np.mean(np.abs(np.abs(u) - LOOP_LIM) < 1e-15))
