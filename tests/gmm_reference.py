"""Reference for fit_gmm and gmm_prior (tests/test_gmm_cpu.py, tests/test_gpu_gmm.py): the definitions of include/ddp_amd.h restated in
NumPy, in `np.longdouble` by default (dtype=np.float64 runs the same code in double, which is how the condition on the designed inputs
is measured), independent of csrc/gmm.hip.  The Philox assignment comes from tests/sample_reference.py.  The cases the GPU tests share
are computed once each."""
import functools

import numpy as np

import sample_reference as sr

LD = np.longdouble
TOL = 1e-8                      # device against long double, relative
COND_TOL = 1e-10                # float64 against long double on the designed inputs
KAPPA_CAP = 2e3                 # every Sigma_k at every iteration
PI_MIN = 0.02                   # every pi_k at every iteration


def points(xs, us, dtype=LD):
    """W[p, N-1, S, B]: w = [x_i; u_i; x_{i+1}]"""
    xs, us = np.asarray(xs, dtype=dtype), np.asarray(us, dtype=dtype)
    return np.concatenate([xs[:, :-1], us[:, :-1], xs[:, 1:]], axis=0)


def mixture_points(W, pool):
    """the points of every mixture as [p, P], point j = s + S (i + (N - 1) b)"""
    p, N1, S, B = W.shape
    if pool:
        return [W.transpose(0, 3, 1, 2).reshape(p, B * N1 * S)]
    return [W[..., b].reshape(p, N1 * S) for b in range(B)]


def hard_assignment(seed, K, N, S, B, traj0=0):
    """cluster[N-1, S, B] of the start: the first word of Philox4x32-10, counter (i, s, traj0 + b, 0x80000000), mod K"""
    seed = int(seed)
    i, s, b = np.meshgrid(np.arange(N - 1), np.arange(S), traj0 + np.arange(B), indexing="ij")
    r0 = sr.philox4x32_10(i, s, b, np.full(i.shape, 0x80000000), seed & 0xFFFFFFFF, seed >> 32)[0]
    return (r0 % np.uint64(K)).astype(np.int64)


def _posfin(v):
    return bool(v > 0) and bool(np.isfinite(v))


def chol(A):
    """lower Cholesky factor in A's dtype (the lower triangle is read); None if a pivot is not a positive finite number"""
    p = A.shape[0]
    L = np.zeros_like(A)
    for c in range(p):
        d = A[c, c] - L[c, :c] @ L[c, :c]
        if not _posfin(d):
            return None
        L[c, c] = np.sqrt(d)
        if c + 1 < p:
            L[c + 1:, c] = (A[c + 1:, c] - L[c + 1:, :c] @ L[c, :c]) / L[c, c]
    return L


def forward_solve(L, D):
    """L^-1 D, columns of D at once"""
    Y = np.zeros_like(D)
    for c in range(L.shape[0]):
        Y[c] = (D[c] - L[c, :c] @ Y[:c]) / L[c, c]
    return Y


def check(weights, mu, Sigma):
    """(status, factors): 0, or k + 1 for the smallest k whose weight (N_k, or pi_k of a start that is given) is not a positive finite
    number, whose mu_k is not finite or whose Sigma_k has a pivot that is not a positive finite number"""
    Ls = []
    for k in range(len(weights)):
        L = chol(Sigma[:, :, k]) if _posfin(weights[k]) and np.all(np.isfinite(mu[:, k])) else None
        if L is None:
            return k + 1, None
        Ls.append(L)
    return 0, Ls


def mstep(Wg, R, reg):
    """R[P, K] -> N_k, pi, mu, Sigma (centred on the new mu_k)"""
    dt = Wg.dtype
    p, P = Wg.shape
    K = R.shape[1]
    Nk = R.sum(axis=0)
    mu, Sigma = np.zeros((p, K), dtype=dt), np.zeros((p, p, K), dtype=dt)
    with np.errstate(all="ignore"):
        for k in range(K):
            mu[:, k] = (Wg @ R[:, k]) / Nk[k]
            D = Wg - mu[:, k, None]
            C = (D * R[:, k]) @ D.T / Nk[k]
            Sigma[:, :, k] = (C + C.T) / 2 + reg * np.eye(p, dtype=dt)
        return Nk, Nk / dt.type(P), mu, Sigma


def estep(Wg, pi, mu, Ls):
    dt = Wg.dtype
    p, P = Wg.shape
    K = len(Ls)
    log2pi = np.log(2 * dt.type("3.14159265358979323846264338327950288") if dt == LD else dt.type(2 * np.pi))
    lo = np.zeros((P, K), dtype=dt)
    for k in range(K):
        Y = forward_solve(Ls[k], Wg - mu[:, k, None])
        lo[:, k] = np.log(pi[k]) - dt.type(p) / 2 * log2pi - np.sum(np.log(np.diag(Ls[k]))) - (Y * Y).sum(axis=0) / 2
    mx = lo.max(axis=1)
    lse = mx + np.log(np.exp(lo - mx[:, None]).sum(axis=1))
    return np.exp(lo - lse[:, None]), lse.sum()


def kappa(S):
    w = np.linalg.eigvalsh(np.asarray(S, dtype=np.float64))
    return float(w[-1] / w[0]) if w[0] > 0 else np.inf


def fit(xs, us, K, iters=20, reg=1e-6, seed=0, init=None, pool=True, traj0=0, dtype=LD):
    """dict(pi[K,G], mu[p,K,G], Sigma[p,p,K,G], ll[iters,G], status[G]) in `dtype`, and what the condition tests ask of the inputs:
    kappa_max (the largest kappa(Sigma_k) over the mixtures formed, the start included) and pi_min (the smallest pi_k)"""
    dt = np.dtype(dtype)
    W = points(xs, us, dt)
    p, N1, S, B = W.shape
    N = N1 + 1
    G = 1 if pool else B
    pi, mu, Sigma = np.zeros((K, G), dtype=dt), np.zeros((p, K, G), dtype=dt), np.zeros((p, p, K, G), dtype=dt)
    ll, status = np.zeros((iters, G), dtype=dt), np.zeros(G, dtype=np.int32)
    kmax, pmin = 0.0, 1.0
    reg = dt.type(reg)
    asg = None if init is not None else hard_assignment(seed, K, N, S, B, traj0)
    for g, Wg in enumerate(mixture_points(W, pool)):
        P = Wg.shape[1]
        if init is not None:
            pg, mg, Sg = (np.asarray(a, dtype=dt)[..., g] for a in init)           # pi[K,G], mu[p,K,G], Sigma[p,p,K,G]
            Sg = np.stack([np.tril(Sg[:, :, k]) + np.tril(Sg[:, :, k], -1).T for k in range(K)], axis=-1)
            st, Ls = check(pg, mg, Sg)
        else:
            a = asg.transpose(2, 0, 1).reshape(-1) if pool else asg[..., g].reshape(-1)
            R = (a[:, None] == np.arange(K)[None, :]).astype(dt)
            Nk, pg, mg, Sg = mstep(Wg, R, reg)
            st, Ls = check(Nk, mg, Sg)
        dead = -2
        for t in range(-1, iters):
            if t >= 0:
                R, ll[t, g] = estep(Wg, pg, mg, Ls)
                Nk, pg, mg, Sg = mstep(Wg, R, reg)
                st, Ls = check(Nk, mg, Sg)
            if st:
                status[g], dead = st, t
                break
            kmax = max(kmax, max(kappa(Sg[:, :, k]) for k in range(K)))
            pmin = min(pmin, float(pg.min()))
        if status[g]:
            pg, mg, Sg = pg * np.nan, mg * np.nan, Sg * np.nan
            ll[dead + 1:, g] = np.nan
        pi[:, g], mu[..., g], Sigma[..., g] = pg, mg, Sg
    return dict(pi=pi, mu=mu, Sigma=Sigma, ll=ll, status=status, pool=bool(pool), kappa_max=kmax, pi_min=pmin)


def prior(gmm, xs, us, m0=1.0, n0=1.0, dtype=LD):
    """(Phi[p,p,N,B], mu0[p,N,B], status[N,B]) in `dtype`; status 2: the mixture is not usable, else 1: a point of the step is not finite"""
    dt = np.dtype(dtype)
    W = points(xs, us, dt)
    p, N1, S, B = W.shape
    N = N1 + 1
    K = gmm["pi"].shape[0]
    Phi, mu0, status = np.zeros((p, p, N, B), dtype=dt), np.zeros((p, N, B), dtype=dt), np.zeros((N, B), dtype=np.int32)
    facs = {}
    for b in range(B):
        g = 0 if gmm["pool"] else b
        if g not in facs:
            pg, mg = np.asarray(gmm["pi"][:, g], dtype=dt), np.asarray(gmm["mu"][..., g], dtype=dt)
            Sg = np.asarray(gmm["Sigma"][..., g], dtype=dt)
            Sg = np.stack([np.tril(Sg[:, :, k]) + np.tril(Sg[:, :, k], -1).T for k in range(K)], axis=-1)
            facs[g] = (pg, mg, Sg) + check(pg, mg, Sg)
        pg, mg, Sg, st, Ls = facs[g]
        for i in range(N1):
            Wi = W[:, i, :, b]
            if st:
                status[i, b] = 2
            elif not np.all(np.isfinite(Wi)):
                status[i, b] = 1
            if status[i, b]:
                Phi[:, :, i, b], mu0[:, i, b] = np.nan, np.nan
                continue
            R, _ = estep(Wi, pg, mg, Ls)
            om = R.sum(axis=0) / dt.type(S)
            m_ = mg @ om
            D = mg - m_[:, None]
            Phi[:, :, i, b] = dt.type(n0) * (np.einsum("k,ijk->ij", om, Sg) + (D * om) @ D.T)
            mu0[:, i, b] = m_
    return Phi, mu0, status


# ----------------------------------------------------------------------------------------------------------------- designed inputs
def designed(n, m, N, S, B, K, seed, sep=4.0):
    """xs[n,N,S,B], us[m,N,S,B] whose transition tuples fall into K well-conditioned clusters, and the true label of every point
    [N-1,S,B]: step i of sample s of trajectory b belongs to cluster (i + s + b) mod K; x_{i+1} = x_i of the next step is shared between
    two tuples, so the state of step i carries the centre of ITS cluster in its x-part and the next state in the y-part — a point is
    [c_x(k_i) + e; c_u(k_i) + e; c_x(k_{i+1}) + e'] and the clusters differ in all three parts.  Scales in [0.6, 1.4] per coordinate."""
    rng = np.random.default_rng(seed)
    cx = sep * rng.standard_normal((n, K)) / np.sqrt(n) + sep * rng.permutation(K)[None, :] * (np.arange(n)[:, None] == 0)
    cu = sep * rng.standard_normal((m, K)) / np.sqrt(m)
    sx, su = 0.6 + 0.8 * rng.random(n), 0.6 + 0.8 * rng.random(m)
    i, s, b = np.meshgrid(np.arange(N), np.arange(S), np.arange(B), indexing="ij")
    lab = (i + s + b) % K
    xs = cx[:, lab] + sx[:, None, None, None] * rng.standard_normal((n, N, S, B))
    us = cu[:, lab] + su[:, None, None, None] * rng.standard_normal((m, N, S, B))
    return np.asfortranarray(xs), np.asfortranarray(us), lab[:-1]


def true_init(xs, us, lab, K, reg=0.0):
    """(pi, mu, Sigma) in float64 of one M-step from the true labels, pooled"""
    W = points(xs, us)
    Wg = mixture_points(W, True)[0]
    R = (lab.transpose(2, 0, 1).reshape(-1)[:, None] == np.arange(K)[None, :]).astype(LD)
    _, pi, mu, Sigma = mstep(Wg, R, LD(reg))
    return pi.astype(np.float64), mu.astype(np.float64), Sigma.astype(np.float64)


# name -> (n, m, N, S, B, K, iters, pool, start): start "philox" or "init"
CASES = {
    "p3_k1":        (1, 1, 4, 7, 3, 1, 10, 1, "philox"),          # P = 63
    "p3_k32_init":  (1, 1, 9, 50, 4, 32, 1, 1, "init"),           # P = 1600, every cluster 50 points
    "p3_k32_hard":  (1, 1, 9, 50, 4, 32, 0, 1, "philox"),         # the assignment alone
    "p10_k2":       (4, 2, 6, 13, 1, 2, 10, 1, "philox"),         # P = 65
    "p10_k5":       (4, 2, 5, 101, 3, 5, 10, 0, "philox"),        # one mixture per trajectory, P = 404: two chunks a work-group
    "p10_k5_init":  (4, 2, 5, 37, 3, 5, 1, 0, "init"),
    "p17_k2":       (6, 5, 3, 49, 2, 2, 10, 1, "philox"),         # one past a tile; P = 196: one past four E-step chunks, 3 * 64 + 4
    "p17_hard":     (6, 5, 3, 49, 2, 2, 0, 0, "philox"),
    "p33_k1":       (13, 7, 2, 97, 1, 1, 1, 1, "philox"),         # P = 97 = 2 * 48 + 1
    "p33_k2":       (13, 7, 4, 43, 1, 2, 1, 1, "philox"),         # P = 129 = 2 * 64 + 1
    "p33_k5_init":  (13, 7, 4, 70, 2, 5, 10, 1, "init"),
    "p72_k2":       (32, 8, 3, 80, 2, 2, 10, 1, "philox"),        # reg = 0
    "p72_k1_b":     (32, 8, 3, 80, 2, 1, 1, 0, "philox"),         # P = 160 per trajectory
}
REG = {"p72_k2": 0.0}
# separation of the cluster centres and the offset of the data's seed, where EM from the Philox start would leave the condition cap with
# the defaults (4.0, 0): found with this reference alone (tests/test_gmm_cpu.py asserts the cap for every case)
DESIGN = {"p10_k2": (4.0, 2), "p10_k5": (2.0, 2)}
SEED = 20141208


@functools.lru_cache(maxsize=None)
def case(name):
    n, m, N, S, B, K, iters, pool, start = CASES[name]
    sep, off = DESIGN.get(name, (4.0, 0))
    xs, us, lab = designed(n, m, N, S, B, K, sum(map(ord, name)) + off, sep)
    init = None
    if start == "init":
        pi, mu, Sigma = true_init(xs, us, lab, K)
        rng = np.random.default_rng(5)
        mu = mu + 0.3 * rng.standard_normal(mu.shape)            # not the fixed point: the iteration has something to do
        G = 1 if pool else B
        init = tuple(np.asfortranarray(np.repeat(a[..., None], G, axis=-1)) for a in (pi, mu, Sigma + 0.5 * np.eye(2 * n + m)[:, :, None]))
    reg = REG.get(name, 1e-6)
    kw = dict(K=K, iters=iters, reg=reg, seed=SEED, init=init, pool=bool(pool))
    ref = fit(xs, us, **kw)
    Phi, mu0, pst = prior(ref, xs, us, 1.0, 1.5)
    return dict(name=name, n=n, m=m, N=N, S=S, B=B, xs=xs, us=us, lab=lab, kw=kw, ref=ref, Phi=Phi, mu0=mu0, pstatus=pst, m0=1.0, n0=1.5)


@functools.lru_cache(maxsize=None)
def case64(name):
    """the same case through the same code in float64"""
    c = case(name)
    ref = fit(c["xs"], c["us"], dtype=np.float64, **c["kw"])
    Phi, mu0, pst = prior(ref, c["xs"], c["us"], c["m0"], c["n0"], dtype=np.float64)
    return dict(ref=ref, Phi=Phi, mu0=mu0, pstatus=pst)


def rel(a, b):
    """|a - b| / |b| in the Frobenius norm"""
    a, b = np.asarray(a, dtype=LD), np.asarray(b, dtype=LD)
    return float(np.linalg.norm((a - b).reshape(-1).astype(np.float64)) / np.linalg.norm(b.reshape(-1).astype(np.float64)))


def errors(got, want):
    """worst relative errors of a mixture against the reference: per Sigma_k and mu_k slot, pi absolute, ll relative"""
    K, G = want["pi"].shape
    e = dict(Sigma=0.0, mu=0.0, pi=float(np.max(np.abs(np.asarray(got["pi"], dtype=LD) - want["pi"]))), ll=0.0)
    for g in range(G):
        for k in range(K):
            e["Sigma"] = max(e["Sigma"], rel(got["Sigma"][:, :, k, g], want["Sigma"][:, :, k, g]))
            e["mu"] = max(e["mu"], rel(got["mu"][:, k, g], want["mu"][:, k, g]))
    if want["ll"].size:
        e["ll"] = float(np.max(np.abs((np.asarray(got["ll"], dtype=LD) - want["ll"]) / want["ll"])))
    return e


def prior_errors(Phi, mu0, c):
    N, B = c["N"], c["B"]
    e = dict(Phi=0.0, mu0=0.0)
    for b in range(B):
        for i in range(N - 1):
            e["Phi"] = max(e["Phi"], rel(Phi[:, :, i, b], c["Phi"][:, :, i, b]))
            e["mu0"] = max(e["mu0"], rel(mu0[:, i, b], c["mu0"][:, i, b]))
    return e


# ------------------------------------------------------------------------------------------------------------------- status cases
def empty_cluster_case():
    """pool = 0, B = 2, K = 2: trajectory 1 starts from an init whose second cluster sits far away with a tiny pi: every r_j1 underflows to
    0, N_1 = 0 -> status 2; trajectory 0 starts from the true clusters"""
    n, m, N, S, B, K = 2, 1, 4, 20, 2, 2
    xs, us, lab = designed(n, m, N, S, B, K, 911)
    pi, mu, Sigma = true_init(xs, us, lab, K)
    init = [np.asfortranarray(np.repeat(a[..., None], B, axis=-1)) for a in (pi, mu, Sigma)]
    init[0][:, 1] = (1.0 - 1e-300, 1e-300)
    init[1][:, 1, 1] += 1e3
    kw = dict(K=K, iters=3, reg=1e-6, seed=SEED, init=tuple(init), pool=False)
    return dict(n=n, m=m, N=N, S=S, B=B, xs=xs, us=us, kw=kw, ref=fit(xs, us, **kw))


def nan_point_case():
    """a NaN in state 1 of step 2 of sample 3 of trajectory 1: in the tuples of steps 1 and 2 of that trajectory"""
    c = dict(case("p10_k5_init"))
    xs = c["xs"].copy()
    xs[1, 2, 3, 1] = np.nan
    Phi, mu0, pst = prior(c["ref"], xs, c["us"], c["m0"], c["n0"])
    c.update(xs=xs, Phi=Phi, mu0=mu0, pstatus=pst)
    return c
