"""Reference for expected_cost and kl_step_adjust (tests/test_expect_cpu.py, tests/test_gpu_expect.py), independent of csrc/expect.hip:
the recursion of include/ddp_amd.h in np.longdouble, written from the formulas with the full H and Σz, the scales the GPU errors are
measured against, the growth of the state covariance, the designed cases the GPU tests share (each computed once), and the plain
float64 statement of the step rule with its designed triples."""
import functools

import numpy as np

LD = np.longdouble
TOL = 1e-8                 # BASELINE.json, the project's parity tolerance
GROWTH_CAP = 1e3           # every designed case: p N GROWTH_CAP 2^-53 < TOL for p <= 40, N <= 33 (1.5e-10)
SEC_FLOOR = 1e-3           # no step's scale of ec is below this fraction of the largest one of its case


def recursion(K, Sg, x0, x, u, model, cost, Sigma0):
    """K[m,n,N,B], Sg[m,m,N,B] or None, x0[n,B] or None, x[n,N,B], u[m,N,B], model = (fx, fu, fc, cov) and cost = (cx, cu, cxx, cxu, cuu, c0)
    with or without the batch axis (cov may be None), Sigma0[n,n,B] or None -> dict: ec[N,B], mu[p,N,B], sigma[p,p,N,B] (long double),
    the terms of ec t[5,N,B], sec[N,B] the sum of their absolute values, smu[N,B] = |μx_i| + |u_i + δu_i|, ssig[N,B] = |Σz_i|_F,
    sx[n,n,N,B] the state covariances and growth[B]"""
    m, n, N, B = K.shape
    p = n + m
    out = dict(ec=np.zeros((N, B), LD), mu=np.zeros((p, N, B), LD), sigma=np.zeros((p, p, N, B), LD), t=np.zeros((5, N, B), LD),
               sec=np.zeros((N, B)), smu=np.zeros((N, B)), ssig=np.zeros((N, B)), sx=np.zeros((n, n, N, B), LD), growth=np.zeros(B))
    fro = lambda A: float(np.sqrt((np.asarray(A, LD) ** 2).sum()))                       # noqa: E731
    for b in range(B):
        at = lambda a, i: np.asarray(a[..., i, b] if _has_b(a, N, B) else a[..., i], LD)      # noqa: E731
        fx, fu, fc, cov = model
        cx, cu, cxx, cxu, cuu, c0 = cost
        mux = np.asarray(x[:, 0, b] if x0 is None else x0[:, b], LD)
        Sx = np.zeros((n, n), LD) if Sigma0 is None else np.asarray(Sigma0[:, :, b], LD)
        inj = fro(Sx)
        worst = 0.0
        for i in range(N):
            Ki = np.asarray(K[:, :, i, b], LD)
            Si = np.zeros((m, m), LD) if Sg is None else np.asarray(Sg[:, :, i, b], LD)
            dx = mux - np.asarray(x[:, i, b], LD)
            du = Ki @ dx
            dz = np.concatenate([dx, du])
            T = Sx @ Ki.T
            Suu = Ki @ T + Si
            Sz = np.block([[Sx, T], [T.T, (Suu + Suu.T) / 2]])                           # (symmetric to the bit, as the kernel's is)
            H = np.block([[at(cxx, i), at(cxu, i)], [at(cxu, i).T, at(cuu, i)]])
            t = np.array([at(c0, i), at(cx, i) @ dx, at(cu, i) @ du, dz @ H @ dz / 2, np.trace(H @ Sz) / 2], LD)
            un = np.asarray(u[:, i, b], LD) + du
            out["ec"][i, b] = t.sum()
            out["t"][:, i, b] = t
            out["sec"][i, b] = float(np.abs(t).sum())
            out["mu"][:, i, b] = np.concatenate([mux, un])
            out["sigma"][:, :, i, b] = Sz
            out["sx"][:, :, i, b] = Sx
            out["smu"][i, b] = fro(mux) + fro(un)
            out["ssig"][i, b] = fro(Sz)
            worst = max(worst, fro(Sx))
            if i < N - 1:
                G = np.concatenate([at(fx, i), at(fu, i)], axis=1)
                mux = at(fx, i) @ mux + at(fu, i) @ un + at(fc, i)
                ci = np.zeros((n, n), LD) if cov is None else at(cov, i)
                Sx = G @ Sz @ G.T + ci
                Sx = (Sx + Sx.T) / 2
                inj += fro(ci) + fro(at(fu, i) @ Si @ at(fu, i).T)
        out["growth"][b] = worst / inj if inj > 0 else (0.0 if worst == 0 else np.inf)
    return out


def _has_b(a, N, B):
    """whether a table [..., N] or [..., N, B] carries the batch axis (N and B differ in every designed case that shares a table)"""
    return a.shape[-1] == B and a.ndim >= 2 and a.shape[-2] == N


# ------------------------------------------------------------------------------------------------------------------- designed inputs
def _spd(rng, k, scale):
    A = rng.standard_normal((k, k))
    return scale * (A @ A.T / k + 0.5 * np.eye(k))


def _sym(rng, k):
    A = rng.standard_normal((k, k)) / np.sqrt(k)
    return (A + A.T) / 2


def designed(n, m, N, B, seed, model_shared=False, cost_shared=False, no_sigma=False, no_cov=False, no_sigma0=False, given_x0=False):
    """seeded inputs of one case, Fortran-ordered float64: every closed loop fx_i + fu_i K_i has spectral radius at most 0.9 (fx_i, fu_i
    are scaled to it), cov, Σ and Sigma0 are symmetric positive definite, cxx and cuu symmetric and indefinite"""
    rng = np.random.default_rng(seed)
    F = np.asfortranarray
    mB, cB = (1 if model_shared else B), (1 if cost_shared else B)
    K = 0.5 * rng.standard_normal((m, n, N, B)) / np.sqrt(n)
    fx, fu = rng.standard_normal((n, n, N, mB)) / np.sqrt(n), rng.standard_normal((n, m, N, mB)) / np.sqrt(m)
    for i in range(N):
        for b in range(mB):
            # a shared model serves every trajectory's K: scale to the largest radius among them
            rho = max(np.abs(np.linalg.eigvals(fx[:, :, i, b] + fu[:, :, i, b] @ K[:, :, i, bb])).max() for bb in (range(B) if model_shared else (b,)))
            s = min(1.0, 0.9 / rho)
            fx[:, :, i, b] *= s; fu[:, :, i, b] *= s
    fc = rng.standard_normal((n, N, mB))
    cov = np.stack([np.stack([_spd(rng, n, 0.1) for _ in range(N)], -1) for _ in range(mB)], -1)
    Sg = np.stack([np.stack([_spd(rng, m, 0.2) for _ in range(N)], -1) for _ in range(B)], -1)
    S0 = np.stack([_spd(rng, n, 0.3) for _ in range(B)], -1)
    # the nominal follows the mean of the closed loop at a distance of about 0.5 a coordinate: δx keeps its size along the horizon
    x, u = rng.standard_normal((n, N, B)), rng.standard_normal((m, N, B))
    x0 = x[:, 0, :] + 0.5 * rng.standard_normal((n, B))
    for b in range(B):
        mb_ = 0 if model_shared else b
        mux = x0[:, b] if given_x0 else x[:, 0, b]
        for i in range(N - 1):
            mux = fx[:, :, i, mb_] @ mux + fu[:, :, i, mb_] @ (u[:, i, b] + K[:, :, i, b] @ (mux - x[:, i, b])) + fc[:, i, mb_]
            x[:, i + 1, b] = mux + 0.5 * rng.standard_normal(n)
    cx, cu, c0 = rng.standard_normal((n, N, cB)), rng.standard_normal((m, N, cB)), 2.0 + rng.standard_normal((N, cB))
    cxx = np.stack([np.stack([_sym(rng, n) for _ in range(N)], -1) for _ in range(cB)], -1)
    cuu = np.stack([np.stack([_sym(rng, m) for _ in range(N)], -1) for _ in range(cB)], -1)
    cxu = rng.standard_normal((n, m, N, cB)) / np.sqrt(n)
    sq = lambda a, shared: F(a[..., 0]) if shared else F(a)                               # noqa: E731
    model = tuple(sq(a, model_shared) for a in (fx, fu, fc)) + (None if no_cov else sq(cov, model_shared),)
    cost = tuple(sq(a, cost_shared) for a in (cx, cu, cxx, cxu, cuu, c0))
    return dict(n=n, m=m, N=N, B=B, K=F(K), Sg=None if no_sigma else F(Sg), x0=F(x0) if given_x0 else None, x=F(x), u=F(u), model=model,
                cost=cost, Sigma0=None if no_sigma0 else F(S0))


# name -> (n, m, N, keywords of designed); B = 3.  (n, m): (1,1), (4,2), (13,4) where p = 17 crosses a tile, (16,1), (17,8), (32,8) where
# p = 40; N in 1, 2, 7 and one N = 33 at (4,2); a shared model with a batched cost model and the reverse at (13,4); Σ = None, cov = None,
# Sigma0 = None and a given x0.
CASES = {
    "1x1": (1, 1, 7, dict(given_x0=True)),
    "1x1-N1": (1, 1, 1, dict()),
    "4x2": (4, 2, 7, dict()),
    "4x2-N2": (4, 2, 2, dict(given_x0=True, no_sigma0=True)),
    "4x2-N33": (4, 2, 33, dict()),
    "4x2-deterministic": (4, 2, 7, dict(no_sigma=True, no_cov=True, no_sigma0=True, given_x0=True)),
    "13x4": (13, 4, 7, dict(no_sigma=True)),
    "13x4-shared-model": (13, 4, 7, dict(model_shared=True, given_x0=True)),
    "13x4-shared-cost": (13, 4, 2, dict(cost_shared=True, no_cov=True)),
    "16x1": (16, 1, 7, dict(no_sigma0=True)),
    "17x8": (17, 8, 2, dict(given_x0=True)),
    "17x8-N1": (17, 8, 1, dict()),
    "32x8": (32, 8, 7, dict(given_x0=True)),
    "32x8-N2": (32, 8, 2, dict(no_cov=True)),
}
B_CASES = 3


@functools.lru_cache(maxsize=None)
def case(name):
    """the inputs of a designed case and `ref`, recursion(...) on them"""
    n, m, N, kw = CASES[name]
    c = designed(n, m, N, B_CASES, sum(map(ord, name)) + 1000 * n + m, **kw)
    c["ref"] = recursion(c["K"], c["Sg"], c["x0"], c["x"], c["u"], c["model"], c["cost"], c["Sigma0"])
    return c


def errors(got, ref):
    """the worst relative errors of a result (ec, mu, sigma) over steps and trajectories: |Δec| / sec, |Δmu| / smu, |Δsigma|_F / ssig"""
    ec, mu, sigma = got
    e_ec = np.abs(ec - ref["ec"].astype(np.float64)) / ref["sec"]
    e_mu = np.sqrt(((mu - ref["mu"].astype(np.float64)) ** 2).sum(axis=0)) / ref["smu"]
    d = np.sqrt(((sigma - ref["sigma"].astype(np.float64)) ** 2).sum(axis=(0, 1)))
    e_sig = np.where(ref["ssig"] > 0, d / np.where(ref["ssig"] > 0, ref["ssig"], 1.0), d)
    return float(e_ec.max()), float(e_mu.max()), float(e_sig.max())


# ------------------------------------------------------------------------------------------------------------------- the step rule
def step_rule(ec_prev, ec_pred, ec_act, kl_step, step_min=1e-2, step_max=1e2):
    """kl_step_adjust in plain float64: ec[N,B], sums in ascending i -> (kl_step_new[B], mult[B])"""
    N, B = ec_prev.shape
    ks = np.broadcast_to(np.asarray(kl_step, np.float64), (B,))
    new, mult = np.zeros(B), np.zeros(B)
    for b in range(B):
        J = [0.0, 0.0, 0.0]
        for i in range(N):
            for q, a in enumerate((ec_prev, ec_pred, ec_act)):
                J[q] = J[q] + float(a[i, b])
        mu = 0.1
        if all(np.isfinite(v) for v in J):
            pred, act = J[0] - J[1], J[0] - J[2]
            mu = min(max(pred / (2.0 * max(1e-4, pred - act)), 0.1), 5.0)
        mult[b] = mu
        new[b] = min(max(float(ks[b]) * mu, step_min), step_max)
    return new, mult


STEP_CANCEL = 1e-2         # the designed triples: |pred - act| >= STEP_CANCEL sum|ec| (and |pred| too where mult is not clipped)
# (J_prev, pred, act, kl_step, what the column exercises)
STEP_COLUMNS = [
    (4.0, 2.0, 1.0, 1.0, "interior"),
    (4.0, 3.0, 2.8, 1.0, "mult clipped at 5"),
    (4.0, 0.3, -3.0, 1.0, "mult clipped at 0.1"),
    (4.0, 2.0, 3.0, 1.0, "floor 1e-4, then clipped at 5"),
    (4.0, -1.0, -2.0, 1.0, "negative pred: clipped at 0.1"),
    (4.0, 2.0, 1.0, 1.0, "nan"),
    (4.0, 2.0, 1.0, 1.0, "inf"),
    (4.0, 2.0, 0.5, 400.0, "interior, step_max"),
    (4.0, 2.0, 1.0, 1e-3, "interior, step_min"),
    (4.0, 2.0, 1.0, 1.0, "overflow"),
]
STEP_MULT_EXACT = (1, 2, 3, 4, 5, 6, 9)     # columns whose mult is fixed by a clip or the non-finite branch: compared exactly
STEP_NEW_EXACT = STEP_MULT_EXACT + (7, 8)   # columns whose kl_step_new is (those, and the two clipped at step_max / step_min)


@functools.lru_cache(maxsize=None)
def step_triples(N=7):
    """(ec_prev, ec_pred, ec_act)[N,B], kl_step[B] of STEP_COLUMNS: positive entries with the column sums of the table"""
    rng = np.random.default_rng(77)
    B = len(STEP_COLUMNS)
    ecs = [np.zeros((N, B), order="F") for _ in range(3)]
    ks = np.zeros(B)
    for b, (Jp, pred, act, k, what) in enumerate(STEP_COLUMNS):
        for a, J in zip(ecs, (Jp, Jp - pred, Jp - act)):
            w = rng.uniform(0.5, 1.5, N)
            a[:, b] = J * w / w.sum()
        ks[b] = k
        if what == "nan":
            ecs[1][3, b] = np.nan
        if what == "inf":
            ecs[2][N - 1, b] = np.inf
        if what == "overflow":
            ecs[0][:2, b] = 1e308
    return ecs[0], ecs[1], ecs[2], ks
