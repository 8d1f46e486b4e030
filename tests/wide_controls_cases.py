"""Seeded cases for the wide-control tests (8 < m <= 32): tests/test_wide_controls_cpu.py checks on the CPU that the C oracle and the NumPy
restatement agree on them (so they do not sit at a tie of the reference), tests/test_gpu_wide_controls.py runs them on the GPU against
the C oracle.  No test in this file."""
import numpy as np

SHAPES = [(6, 9), (12, 12), (10, 24), (24, 16), (32, 32), (33, 9), (48, 12), (63, 17), (64, 32)]
# shared LTI | LTV | LTV with a time-varying cost | per-trajectory everything  (F / C: time-varying dynamics / cost, f / c: per trajectory)
LAYOUTS = ("", "F", "FC", "FCfc")


def _mats(rng, n, m, count):
    """count sets of (fx, fu, cxx, cxu, cuu): fx = 0.95 I + 0.05/sqrt(n) randn, fu = 0.3/sqrt(n) randn, cxx = I + 0.2 AA'/n,
    cuu = 0.1 (I + 0.2 AA'/m), cxu = 0.02 randn"""
    fx = 0.95 * np.eye(n)[:, :, None] + 0.05 / np.sqrt(n) * rng.standard_normal((n, n, count))
    fu = 0.3 / np.sqrt(n) * rng.standard_normal((n, m, count))
    a = rng.standard_normal((n, n, count))
    cxx = np.eye(n)[:, :, None] + 0.2 * np.einsum("ikc,jkc->ijc", a, a) / n
    a = rng.standard_normal((m, m, count))
    cuu = 0.1 * (np.eye(m)[:, :, None] + 0.2 * np.einsum("ikc,jkc->ijc", a, a) / m)
    cxu = 0.02 * rng.standard_normal((n, m, count))
    return fx, fu, cxx, cxu, cuu


def bp_case(seed, n, m, N, B, layout="", lim=None, lims_off=False):
    """one backward-pass call: operands in the layout, cx = randn, cu = 0.3 randn, u = clip(0.2 randn, lims), λ = 10^U(-3, 0.5) per
    trajectory.  lim: None, or the bound (limits are -lim, +lim); lims_off: lims[1,1] > lims[1,2] ("no limits" upstream)"""
    rng = np.random.default_rng(seed)
    nf = (N if "F" in layout else 1) * (B if "f" in layout else 1)
    nc = (N if "C" in layout else 1) * (B if "c" in layout else 1)
    fx, fu, _, _, _ = _mats(rng, n, m, nf)
    _, _, cxx, cxu, cuu = _mats(rng, n, m, nc)
    tf = ((N,) if "F" in layout else ()) + ((B,) if "f" in layout else ())
    tc = ((N,) if "C" in layout else ()) + ((B,) if "c" in layout else ())
    rs = lambda a, t: np.asfortranarray(a.reshape(a.shape[:2] + t, order="F"))
    c = dict(n=n, m=m, N=N, B=B, layout=layout, fx=rs(fx, tf), fu=rs(fu, tf), cxx=rs(cxx, tc), cxu=rs(cxu, tc), cuu=rs(cuu, tc),
             cx=rng.standard_normal((n, N, B)), cu=0.3 * rng.standard_normal((m, N, B)), u=0.2 * rng.standard_normal((m, N, B)),
             lam=10.0 ** rng.uniform(-3, 0.5, B), lims=None)
    if lims_off:
        c["lims"] = np.stack([0.5 * np.ones(m), -0.5 * np.ones(m)], 1)
    elif lim is not None:
        c["lims"] = np.stack([-lim * np.ones(m), lim * np.ones(m)], 1)
        c["u"] = np.clip(c["u"], -lim, lim)
    return c


def bp_operands(c, b):
    """trajectory b's operands as the single-trajectory references take them"""
    lay = c["layout"]
    f = lambda a: a[..., b] if "f" in lay else a
    g = lambda a: a[..., b] if "c" in lay else a
    return (c["cx"][..., b], c["cu"][..., b], g(c["cxx"]), g(c["cxu"]), g(c["cuu"]), f(c["fx"]), f(c["fu"]), float(c["lam"][b]))


def clamped_share(k, u, lims):
    """share of the entries of a reference's k that put u + k on a bound (k = lims - u exactly: what the box-QP's clamp returns)"""
    lo, hi = lims[:, 0, None] - u, lims[:, 1, None] - u
    return float(np.mean((k == lo) | (k == hi)))


# whole solves: make_lq_problem(rng, n, m, T, h = 0.05), u0 scaled by 3, max_iter = 50
SOLVES = [(12, 12, 80, None), (12, 12, 80, 0.6), (24, 16, 60, 0.6), (32, 32, 50, 0.6), (48, 12, 50, 0.6), (36, 12, 50, None)]


def solve_case(n, m, T, lim, seed=0):
    from oracle import np_restatement as npr
    rng = np.random.default_rng(1000 * n + m + seed)
    P = npr.make_lq_problem(rng, n=n, m=m, T=T, h=0.05)
    P["u0"] = 3.0 * P["u0"]
    P["lims"] = None if lim is None else np.stack([-lim * np.ones(m), lim * np.ones(m)], 1)
    return P


def solve_batch(P, B=64):
    """the solve of the table (trajectory 0) and B - 1 perturbed copies: x0 + 0.1 randn, u0 scaled by 1 + 0.3 randn plus 0.05 randn"""
    n, m, T = P["n"], P["m"], P["N"]
    rng = np.random.default_rng(n + m)
    x0 = np.concatenate([P["x0"][:, None], P["x0"][:, None] + 0.1 * rng.standard_normal((n, B - 1))], 1)
    u0 = np.concatenate([P["u0"][:, :, None], P["u0"][:, :, None] * (1 + 0.3 * rng.standard_normal((1, 1, B - 1))) + 0.05 * rng.standard_normal((m, T, B - 1))], 2)
    return x0, u0


TIE_EPS, TIE_DRAWS = 1e-13, 8


def reference_outcomes_nearby(p, x0b, u0b, lims, seed):
    """The C oracle's own solves of TIE_DRAWS copies of one problem whose x0, u0 are off by TIE_EPS relative (500 ulp: far below the
    tests' 1e-8, above the rounding a reordered sum leaves).  Made without looking at any GPU result: if their (status, iterations,
    back passes) differ from the unperturbed oracle's, the REFERENCE is discontinuous at this input (a box-QP warm start
    on a bound in one state and an ulp inside it in the other), and no implementation that reorders a sum can be asked for one side."""
    from oracle import oracle_ctypes as oc
    rng = np.random.default_rng(seed)
    return [oc.ilqg(p, x0b * (1 + TIE_EPS * rng.standard_normal(x0b.shape)), u0b * (1 + TIE_EPS * rng.standard_normal(u0b.shape)), lims=lims, max_iter=50)
            for _ in range(TIE_DRAWS)]


def outcome(info):
    return (info["status"], info["iter"], info["n_backpass"])
