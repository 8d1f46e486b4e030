"""Reference for fit_dynamics (tests/test_fit_cpu.py, tests/test_gpu_fit.py), independent of csrc/fit.hip: the linear-Gaussian dynamics
fit of include/ddp_amd.h in np.longdouble — centred sums, the Cholesky factorisation (lower triangle read) and the substitutions — with
the same status rule, the condition number of every A, the scales the GPU tolerances refer to, and the designed cases the GPU tests share
(each computed once)."""
import functools

import numpy as np

LD = np.longdouble
KAPPA_CAP = 2e3            # every step of a designed case that is expected to succeed: d (S + d) kappa 2^-53 < 1e-8 for d <= 40, S <= 130
TOL = 1e-8                 # BASELINE.json, the project's parity tolerance


def chol_status(A):
    """(L, status) of the lower Cholesky factorisation in long double: status 0, or c + 1 for the first pivot c that is not a positive
    finite double (the test of factor_lower in csrc/sample.hip); L is None then"""
    d = A.shape[0]
    L = np.zeros((d, d), dtype=LD)
    for c in range(d):
        piv = A[c, c] - L[c, :c] @ L[c, :c]
        if not (piv > 0 and np.isfinite(np.float64(piv))):
            return None, c + 1
        L[c, c] = np.sqrt(piv)
        for q in range(c + 1, d):
            L[q, c] = (A[q, c] - L[q, :c] @ L[c, :c]) / L[c, c]
    return L, 0


def solve_chol(L, Bm):
    """A^-1 Bm from A = L L' by forward and backward substitution in long double"""
    d = L.shape[0]
    Y = np.zeros(Bm.shape, dtype=LD)
    for r in range(d):
        Y[r] = (Bm[r] - L[r, :r] @ Y[:r]) / L[r, r]
    X = np.zeros(Bm.shape, dtype=LD)
    for r in range(d - 1, -1, -1):
        X[r] = (Y[r] - L[r + 1:, r] @ X[r + 1:]) / L[r, r]
    return X


def fit_step(W, n, m, ridge=0.0, prior=None):
    """one step: W[p, S] = [x_i; u_i; x_i+1] over the samples.  prior = (Phi[p,p], mu0[p], m0, n0) or None.  Returns a dict: F[n,d], fc[n],
    cov[n,n] (NaN when status != 0), status (d + 1: no pivot failed, but a result is not finite), kappa (of A, in double, from its
    lower triangle; inf when the step failed) and the scales of the tolerances: sF = |F|_F, sfc = |mu_y| + |F| |mu_z|, scov = |C_yy|_F"""
    d, S = n + m, W.shape[1]
    W = np.asarray(W, dtype=LD)
    mu = W.sum(axis=1) / LD(S)
    Wc = W - mu[:, None]
    E = Wc @ Wc.T
    if prior is None:
        C = E / LD(S - 1)
    else:
        Phi, mu0, m0, n0 = prior
        Phi, dm = np.asarray(Phi, dtype=LD), mu - np.asarray(mu0, dtype=LD)
        Phi = np.tril(Phi) + np.tril(Phi, -1).T                                    # the lower triangle is read
        C = (E + Phi + LD(S) * LD(m0) / (LD(S) + LD(m0)) * np.outer(dm, dm)) / (LD(S) + LD(n0))
    A = C[:d, :d] + LD(ridge) * np.eye(d, dtype=LD)
    A = np.tril(A) + np.tril(A, -1).T
    Czy, Cyy = C[:d, d:], C[d:, d:]
    L, status = chol_status(A)
    nan = np.full
    out = dict(status=status, kappa=np.inf, F=nan((n, d), np.nan), fc=nan(n, np.nan), cov=nan((n, n), np.nan), sF=np.nan, sfc=np.nan, scov=np.nan)
    if status:
        return out
    F = solve_chol(L, Czy).T
    M = Cyy - F @ Czy
    A64 = A.astype(np.float64)
    if not (np.all(np.isfinite(F.astype(np.float64))) and np.all(np.isfinite(M.astype(np.float64))) and np.all(np.isfinite(mu.astype(np.float64)))):
        out["status"] = d + 1                                     # every pivot of A is fine, the results are not finite (a NaN in y)
        return out
    out.update(F=F, fc=mu[d:] - F @ mu[:d], cov=(M + M.T) / 2, kappa=float(np.linalg.cond(A64)) if np.all(np.isfinite(A64)) else np.inf,
               sF=float(np.sqrt((F * F).sum())), scov=float(np.sqrt((Cyy * Cyy).sum())),
               sfc=float(np.sqrt(mu[d:] @ mu[d:]) + np.sqrt((F * F).sum()) * np.sqrt(mu[:d] @ mu[:d])))
    return out


def fit(xs, us, ridge=0.0, prior=None):
    """xs[n,N,S,B], us[m,N,S,B] -> dict of fx[n,n,N,B], fu[n,m,N,B], fc[n,N,B], cov[n,n,N,B] (float64 of the long double results),
    status[N,B], kappa[N,B], sF, sfc, scov [N,B].  prior = (Phi, mu0, m0, n0), Phi[p,p] / mu0[p] or Phi[p,p,N,B] / mu0[p,N,B].  Slot N - 1:
    zeros, status 0."""
    n, N, S, B = xs.shape
    m = us.shape[0]
    r = dict(fx=np.zeros((n, n, N, B)), fu=np.zeros((n, m, N, B)), fc=np.zeros((n, N, B)), cov=np.zeros((n, n, N, B)),
             status=np.zeros((N, B), dtype=np.int32), kappa=np.zeros((N, B)), sF=np.zeros((N, B)), sfc=np.zeros((N, B)), scov=np.zeros((N, B)))
    for b in range(B):
        for i in range(N - 1):
            pr = prior
            if prior is not None and np.ndim(prior[0]) == 4:
                pr = (prior[0][:, :, i, b], prior[1][:, i, b], prior[2], prior[3])
            W = np.concatenate([xs[:, i, :, b], us[:, i, :, b], xs[:, i + 1, :, b]], axis=0)
            o = fit_step(W, n, m, ridge, pr)
            r["fx"][:, :, i, b], r["fu"][:, :, i, b] = o["F"][:, :n].astype(np.float64), o["F"][:, n:].astype(np.float64)
            r["fc"][:, i, b], r["cov"][:, :, i, b] = o["fc"].astype(np.float64), o["cov"].astype(np.float64)
            for k in ("status", "kappa", "sF", "sfc", "scov"):
                r[k][i, b] = o[k]
    return r


def errors(got, ref):
    """the three relative errors of the GPU tests per step and trajectory, [N,B] each (NaN where the reference failed; 0 in slot N - 1,
    whose arrays are compared exactly elsewhere): |dF|_F / |F|_F with F = [fx fu], |dfc| / (|mu_y| + |F| |mu_z|), |dcov|_F / |C_yy|_F"""
    fx, fu, fc, cov = got[:4]
    dF = np.sqrt(((fx - ref["fx"]) ** 2).sum(axis=(0, 1)) + ((fu - ref["fu"]) ** 2).sum(axis=(0, 1)))
    dc = np.sqrt(((fc - ref["fc"]) ** 2).sum(axis=0))
    dcov = np.sqrt(((cov - ref["cov"]) ** 2).sum(axis=(0, 1)))
    with np.errstate(invalid="ignore", divide="ignore"):
        e = [np.where(ref["sF"] > 0, dF / ref["sF"], dF), np.where(ref["sfc"] > 0, dc / ref["sfc"], dc), np.where(ref["scov"] > 0, dcov / ref["scov"], dcov)]
    return e


# ------------------------------------------------------------------------------------------------------------------- designed inputs
def smax_for(d, S):
    """the largest scale factor (at most 30) of a designed case without prior and ridge.  The population condition number of C_zz with
    independent columns scaled by factors in [1, smax] is smax^2; the extreme eigenvalues of a sample covariance of d independent unit
    columns over S samples lie near (1 +- sqrt(d / (S - 1)))^2 (Marchenko-Pastur edges), so the sample condition number is about
    smax^2 ((1 + q) / (1 - q))^2 with q = sqrt(d / (S - 1)).  Half of KAPPA_CAP is left for the fluctuation around those edges."""
    q = np.sqrt(d / (S - 1.0))
    assert q < 1, "S > d + 1 is needed without a prior"
    return float(min(30.0, np.sqrt(0.5 * KAPPA_CAP) * (1 - q) / (1 + q)))


def designed(n, m, N, S, B, seed, noise=0.1, smax=None):
    """xs[n,N,S,B], us[m,N,S,B] and the truth F[n,d,N,B], c[n,N,B]: the columns of z = [x; u] are independent normals scaled by factors
    in [1, smax] (log-uniform; both ends occur when d >= 2) around drawn offsets; y = F z + c + noise * N(0, I) with
    F = diag(s_y) P diag(1 / s_z), P with orthonormal rows, so that the next state has independent columns of scales s_y again."""
    rng = np.random.default_rng(seed)
    d = n + m
    smax = smax_for(d, S) if smax is None else smax

    def scales(k):
        s = np.exp(rng.uniform(0, np.log(smax), k))
        if k >= 2:
            s[rng.integers(k)] = smax
        return s

    xs, us = np.zeros((n, N, S, B)), np.zeros((m, N, S, B))
    F, c = np.zeros((n, d, N, B)), np.zeros((n, N, B))
    for b in range(B):
        sx = scales(n)
        off = 3 * rng.standard_normal(n)
        xs[:, 0, :, b] = off[:, None] + sx[:, None] * rng.standard_normal((n, S))
        for i in range(N):
            su = scales(m)
            uo = 3 * rng.standard_normal(m)
            us[:, i, :, b] = uo[:, None] + su[:, None] * rng.standard_normal((m, S))
            if i == N - 1:
                break
            sy = scales(n)
            P = np.linalg.qr(rng.standard_normal((d, n)))[0].T
            F[:, :, i, b] = sy[:, None] * P / np.concatenate([sx, su])[None, :]
            c[:, i, b] = 3 * rng.standard_normal(n)
            z = np.concatenate([xs[:, i, :, b] - off[:, None], us[:, i, :, b] - uo[:, None]], axis=0)
            off = F[:, :, i, b] @ np.concatenate([off, uo]) + c[:, i, b]
            xs[:, i + 1, :, b] = off[:, None] + F[:, :, i, b] @ z + noise * rng.standard_normal((n, S))
            sx = sy
    return xs, us, F, c


def designed_prior(n, m, N, B, seed, per_step):
    """a normal-inverse-Wishart prior for the designed cases: Phi = n0 (G G' / p + I) scaled like the data, mu0 drawn; shared, or one per
    (step, trajectory)"""
    rng = np.random.default_rng(seed)
    p = 2 * n + m
    shape = (N, B) if per_step else ()
    n0, m0 = 4.0, 2.0
    G = rng.standard_normal(shape + (p, p))
    Phi = n0 * 4.0 * (G @ np.swapaxes(G, -1, -2) / p + np.eye(p))
    mu0 = 3 * rng.standard_normal(shape + (p,))
    if per_step:
        Phi, mu0 = np.moveaxis(Phi, (0, 1), (2, 3)), np.moveaxis(mu0, (0, 1), (1, 2))
    return np.asfortranarray(Phi), np.asfortranarray(mu0), m0, n0


# name -> (n, m, N, S, B, prior: None / "shared" / "per_step").  Every value of each axis of the issue appears: (n, m) in (1,1), (4,2), (5,3),
# (12,4) (d one tile), (13,4) (d crosses a tile), (32,8); S in 2 (with a prior), 63, 64, 65, 130; N in 1, 2, 7; B in 1, 3.
CASES = {
    "1x1": (1, 1, 7, 64, 3, None),
    "4x2": (4, 2, 7, 63, 3, None),
    "4x2-N1": (4, 2, 1, 64, 3, None),
    "5x3": (5, 3, 7, 65, 1, None),
    "5x3-prior-S2": (5, 3, 7, 2, 3, "shared"),
    "12x4": (12, 4, 2, 130, 3, None),
    "13x4": (13, 4, 7, 64, 1, None),
    "13x4-prior": (13, 4, 2, 65, 3, "per_step"),
    "4x2-prior-per-step-S2": (4, 2, 7, 2, 3, "per_step"),
    "32x8": (32, 8, 2, 130, 3, None),
    "32x8-prior-N7": (32, 8, 7, 63, 1, "shared"),
}


@functools.lru_cache(maxsize=None)
def case(name):
    """dict(n, m, N, S, B, xs, us, F, c, ridge, prior, ref) of a designed case; ref is fit(...) on it"""
    n, m, N, S, B, pk = CASES[name]
    seed = sum(map(ord, name)) + 1000 * n + m
    # with a prior the data may be fewer than d + 1 samples: A is carried by Phi, and the data keep scales up to 3
    xs, us, F, c = designed(n, m, N, S, B, seed, smax=(3.0 if pk else None))
    prior = None if pk is None else designed_prior(n, m, N, B, seed + 1, pk == "per_step")
    return dict(n=n, m=m, N=N, S=S, B=B, xs=xs, us=us, F=F, c=c, ridge=0.0, prior=prior, ref=fit(xs, us, 0.0, prior))


FAIL_STEP = 3


@functools.lru_cache(maxsize=None)
def identical_columns_case():
    """(4, 2), N = 7, S = 65, B = 2: in trajectory 1 the first two columns of z at step 3 (states 0 and 1) are the same exact pattern —
    32 samples of +2, 32 of -2, one 0.  Every operation on them is exact in double and in long double: the mean is 0, C_00 = C_10 = C_11 =
    256 / 64 = 4, L_00 = 2, L_10 = 2 and the second pivot is exactly 4 - 4 = 0, so step 3 fails at pivot 1 (status 2) whatever the
    rounding.  Steps 2 (whose y holds the pattern) and 4 (whose z does not) are ordinary."""
    n, m, N, S, B = 4, 2, 7, 65, 2
    xs, us, F, c = designed(n, m, N, S, B, 4265)
    pat = np.concatenate([np.full(32, 2.0), np.full(32, -2.0), [0.0]])
    pat = pat[np.random.default_rng(1).permutation(S)]
    xs[0, FAIL_STEP, :, 1] = pat
    xs[1, FAIL_STEP, :, 1] = pat
    return dict(n=n, m=m, N=N, S=S, B=B, xs=xs, us=us, ref=fit(xs, us))


@functools.lru_cache(maxsize=None)
def nan_case(which):
    """(4, 2), N = 7, S = 64, B = 2 with one NaN: which = "state": xs[2, 3, 17, 1]; "control": us[1, 3, 17, 1]"""
    n, m, N, S, B = 4, 2, 7, 64, 2
    xs, us, F, c = designed(n, m, N, S, B, 4264)
    (xs if which == "state" else us)[2 if which == "state" else 1, 3, 17, 1] = np.nan
    return dict(n=n, m=m, N=N, S=S, B=B, xs=xs, us=us, ref=fit(xs, us))


# ------------------------------------------------------------------------------------------------------------- through the sampler
SAMPLER_RIDGE = 1e-3


@functools.lru_cache(maxsize=None)
def sampler_case():
    """the lq_ad case of sample_reference.py (n = 5, m = 3, N = 37, S = 70, B = 3): its reference samples, the long double fit of them
    with SAMPLER_RIDGE and with ridge 0, and the example's A, B per trajectory"""
    import sample_reference as sr
    c = sr.case("lq_ad")
    xs, us, _ = sr.reference("lq_ad")
    n, m, B = c["n"], c["m"], c["B"]
    AB = np.stack([np.concatenate([c["params"][:n * n, b].reshape(n, n, order="F"), c["params"][n * n:n * n + n * m, b].reshape(n, m, order="F")], axis=1)
                   for b in range(B)], axis=-1)
    return dict(case=c, xs=xs, us=us, AB=AB, ref=fit(xs, us, SAMPLER_RIDGE), ref0=fit(xs, us, 0.0))
