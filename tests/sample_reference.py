"""Reference for DDP_USER_SAMPLE (tests/test_user_sample_cpu.py, tests/test_gpu_user_sample.py), independent of csrc/philox.h and of
the kernels:

  * Philox4x32-10 and Box-Muller in NumPy, written from Salmon, Moraes, Dror, Shaw, "Parallel random numbers: as easy as 1, 2, 3"
    (SC'11) and the counter layout of include/ddp_amd.h: counter (i, sample0 + s, traj0 + b, q), key (seed_lo, seed_hi);
  * the closed-loop rollout with noise of the bundled examples car / car_plant / pendcart / lq in long double, the models restated in
    NumPy (as tests/constraints_cases.py does for its model);
  * the cases the GPU tests share, each computed once.
"""
import functools

import numpy as np

LD = np.longdouble
M0, M1, W0, W1, MASK = (np.uint64(v) for v in (0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85, 0xFFFFFFFF))
S32 = np.uint64(32)


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """ten rounds on arrays of 32-bit words held in uint64; returns the four output words"""
    c0, c1, c2, c3 = (np.asarray(c, dtype=np.uint64) & MASK for c in (c0, c1, c2, c3))
    k0, k1 = np.uint64(k0) & MASK, np.uint64(k1) & MASK
    for _ in range(10):
        p0, p1 = M0 * c0, M1 * c2                                # 32 x 32 -> 64 bits: no overflow
        c0, c1, c2, c3 = (p1 >> S32) ^ c1 ^ k0, p1 & MASK, (p0 >> S32) ^ c3 ^ k1, p0 & MASK
        k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
    return c0, c1, c2, c3


def normals(seed, m, N, S, B, sample0=0, traj0=0):
    """xi[m, N, S, B] of the sampler's stream"""
    seed = int(seed)
    mp = (m + 1) // 2
    q, i, s, b = np.meshgrid(np.arange(mp), np.arange(N), sample0 + np.arange(S), traj0 + np.arange(B), indexing="ij")
    r0, r1, r2, r3 = philox4x32_10(i, s, b, q, seed & 0xFFFFFFFF, seed >> 32)
    k1 = (r0 >> np.uint64(5)) * np.uint64(1 << 26) + (r1 >> np.uint64(6))
    k2 = (r2 >> np.uint64(5)) * np.uint64(1 << 26) + (r3 >> np.uint64(6))
    u1 = (k1 + np.uint64(1)).astype(np.float64) * 2.0 ** -53     # (0, 1]
    u2 = k2.astype(np.float64) * 2.0 ** -53                      # [0, 1)
    rho, ang = np.sqrt(-2.0 * np.log(u1)), 2.0 * np.pi * u2
    xi = np.empty((2 * mp, N, S, B))
    xi[0::2], xi[1::2] = rho * np.cos(ang), rho * np.sin(ang)
    return xi[:m]


# ---------------------------------------------------------------------------------------------------------------- the models, restated
def car_f(x, u, i, p):
    h = p[0]
    return np.stack([x[0] + h * x[3] * np.cos(x[2]), x[1] + h * x[3] * np.sin(x[2]), x[2] + h * u[1], x[3] + h * u[0]])


def car_cost(x, u, i, p):
    dx, dy, r2 = x[0] - p[3], x[1] - p[4], p[5] * p[5]
    return LD(0.5) * p[7] * (u[0] * u[0] + u[1] * u[1]) + p[6] * np.exp(-(dx * dx + dy * dy) / r2)


def car_terminal(x, p):
    ex, ey = x[0] - p[1], x[1] - p[2]
    return LD(0.5) * p[8] * (ex * ex + ey * ey + x[3] * x[3])


def car_plant(x, u, t, p):
    xn = car_f(x, np.stack([p[9] * u[0], p[10] * u[1]]), t, p)
    xn[0] += p[0] * p[11]
    xn[1] += p[0] * p[12]
    return xn


def pend_f(x, u, i, p):
    g, l, h, d = p[0], p[1], p[2], p[3]
    return np.stack([x[0] + h * x[1], x[1] + h * (-(g / l) * np.sin(x[0]) + u[0] / l * np.cos(x[0]) - d * x[1]), x[2] + h * x[3],
                     x[3] + h * u[0]])


def _pend_state(x, p):
    e = x - p[4:8, None]
    Q = p[8:24].reshape(4, 4, order="F")
    return np.einsum("rs,rk,ks->s", e, Q, e)


def pend_cost(x, u, i, p):
    return LD(0.5) * (_pend_state(x, p) + p[24] * u[0] * u[0])


def pend_terminal(x, p):
    return LD(0.5) * _pend_state(x, p)


def _lq_parts(p, n, m):
    o = np.cumsum([0, n * n, n * m, n * n, m * m])
    return [p[o[k]:o[k + 1]].reshape(shp, order="F") for k, shp in enumerate(((n, n), (n, m), (n, n), (m, m)))]


def lq_model(n, m):
    def f(x, u, i, p):
        A, Bm, _, _ = _lq_parts(p, n, m)
        return A @ x + Bm @ u

    def cost(x, u, i, p):
        _, _, Q, R = _lq_parts(p, n, m)
        return LD(0.5) * np.einsum("rs,rk,ks->s", x, Q, x) + LD(0.5) * np.einsum("rs,rk,ks->s", u, R, u)
    return f, cost


MODELS = {"car": (car_f, car_cost, car_terminal, None), "car_plant": (car_f, car_cost, car_terminal, car_plant),
          "pendcart": (pend_f, pend_cost, pend_terminal, None)}


def chol_lower(A):
    """lower Cholesky in long double (the lower triangle is read); None if a pivot is not positive"""
    A = np.asarray(A, dtype=LD)
    m = A.shape[0]
    L = np.zeros((m, m), dtype=LD)
    for c in range(m):
        d = A[c, c] - L[c, :c] @ L[c, :c]
        if not d > 0:
            return None
        L[c, c] = np.sqrt(d)
        for q in range(c + 1, m):
            L[q, c] = (A[q, c] - L[q, :c] @ L[c, :c]) / L[c, c]
    return L


def rollout(model, p, K, Sigma, x0, u, x, xi, lims=None, wrap=(), plant=False):
    """one trajectory, all samples at once, in long double: K[m,n,N], Sigma[m,m,N] or None, x0[n], u[m,N], x[n,N], xi[m,N,S] (or S, an
    int, without noise) -> xs[n,N,S], us[m,N,S], cs[CL,S].  model = (f, cost, terminal or None, plant or None)"""
    f, cost, terminal, pl = model
    p, K, x0, u, x = (np.asarray(a, dtype=LD) for a in (p, K, x0, u, x))
    m, n, N = K.shape
    S = xi if isinstance(xi, int) else xi.shape[2]
    twopi = 2 * LD("3.14159265358979323846264338327950288")
    xs, us = np.zeros((n, N, S), dtype=LD), np.zeros((m, N, S), dtype=LD)
    cs = np.zeros((N + (terminal is not None), S), dtype=LD)
    xh = np.repeat(x0[:, None], S, axis=1)
    for i in range(N):
        d = xh - x[:, i, None]
        for c in wrap:
            d[c] = d[c] - twopi * np.rint(d[c] / twopi)
        uu = np.repeat(u[:, i, None], S, axis=1)
        if Sigma is not None:
            uu = uu + chol_lower(Sigma[:, :, i]) @ np.asarray(xi[:, i, :], dtype=LD)
        uu = uu + K[:, :, i] @ d
        if lims is not None:
            uu = np.clip(uu, np.asarray(lims, dtype=LD)[:, 0, None], np.asarray(lims, dtype=LD)[:, 1, None])
        xs[:, i], us[:, i], cs[i] = xh, uu, cost(xh, uu, i, p)
        if i < N - 1:
            xh = (pl if plant else f)(xh, uu, i, p)
    if terminal is not None:
        cs[N] = terminal(xh, p)
    return xs, us, cs


# ---------------------------------------------------------------------------------------------------------------------- shared cases
CAR_P = np.array([0.05, 2.0, 1.0, 1.0, 0.4, 0.5, 2.0, 0.1, 5.0])
CAR_PLANT_TAIL = np.array([0.8, 1.2, 0.3, -0.2])
LIMS = np.array([[-0.6, 0.6], [-0.9, 0.9]])


def spd(rng, m, N, B, scale):
    """Sigma[m,m,N,B], symmetric positive definite, of size ~scale^2"""
    G = rng.standard_normal((m, m, N, B))
    return scale ** 2 * (np.einsum("ikjb,lkjb->iljb", G, G) / m + 0.5 * np.eye(m)[:, :, None, None])


@functools.lru_cache(maxsize=None)
def case(name):
    """inputs of one GPU case: dict(example, n, m, nparam, flags (DeviceProblem keywords), wrap, params[np,B], K, Sigma, x0, u, x, lims, N, S, B, seed)"""
    rng = np.random.default_rng(sum(map(ord, name)))
    B, S = 3, 70
    if name in ("car", "car_lims", "car_plant"):
        n, m, N = 4, 2, 37
        P = np.repeat(CAR_P[:, None], B, axis=1)
        P[0] *= 1 + 0.1 * np.arange(B); P[3] += 0.2 * np.arange(B)          # per-trajectory step and obstacle
        ex = "car"
        kw = dict(terminal=True)
        if name == "car_plant":
            P = np.vstack([P, np.repeat(CAR_PLANT_TAIL[:, None], B, axis=1) * (1 + 0.05 * np.arange(B))])
            ex, kw = "car_plant", dict(terminal=True, plant=True)
        x0 = np.array([[0.0, 0.0, 0.3, 1.0]]).T + 0.1 * rng.standard_normal((n, B))
        u = 0.3 * rng.standard_normal((m, N, B))
        K = -0.4 * rng.random((m, n, N, B))
        scale, wrap, lims = 0.2, (), (LIMS if name == "car_lims" else None)
    elif name == "pendcart":
        n, m, N = 4, 1, 37
        Q = np.diag([10.0, 1.0, 2.0, 1.0])
        base = np.concatenate([[9.82, 0.35, 0.01, 0.99], [np.pi, 0, 0, 0], Q.flatten(order="F"), [1.0]])
        P = np.repeat(base[:, None], B, axis=1)
        P[1] *= 1 + 0.1 * np.arange(B)
        ex, kw = "pendcart", dict(terminal=True)
        x0 = np.array([[np.pi - 0.4, 0.0, 0.0, 0.0]]).T + 0.05 * rng.standard_normal((n, B))
        u = 0.5 * rng.standard_normal((m, N, B))
        K = -1.0 * rng.random((m, n, N, B))
        scale, wrap, lims = 0.5, (0,), None
    else:
        n, m, N = {"lq_ad": (5, 3, 37), "lq_big": (32, 8, 5)}[name]
        A = np.stack([0.7 * np.eye(n) + 0.2 / np.sqrt(n) * rng.standard_normal((n, n)) for _ in range(B)], axis=-1)
        Bm = rng.standard_normal((n, m, B)) / np.sqrt(n)
        Q, R = np.eye(n) + 0.1 * np.ones((n, n)), np.eye(m) + 0.05 * np.ones((m, m))
        P = np.stack([np.concatenate([A[..., b].flatten(order="F"), Bm[..., b].flatten(order="F"), Q.flatten(order="F"), R.flatten(order="F")])
                      for b in range(B)], axis=-1)
        ex, kw = ("lq_ad", dict(autodiff=True)) if name == "lq_ad" else ("lq", {})
        x0 = rng.standard_normal((n, B))
        u = 0.3 * rng.standard_normal((m, N, B))
        K = -0.3 / np.sqrt(n) * rng.random((m, n, N, B))
        scale, wrap, lims = 0.3, (), None
    Sigma = spd(rng, m, N, B, scale)
    # the nominal states: the model's rollout of u without feedback, in double (any x serves as the point K acts around)
    x = np.zeros((n, N, B))
    for b in range(B):
        mdl = MODELS[ex] if ex in MODELS else lq_model(n, m) + (None, None)
        x[..., b] = rollout(mdl, P[:, b], np.zeros((m, n, N)), None, x0[:, b], u[..., b], np.zeros((n, N)), 1)[0][..., 0]
    x = x + 0.05 * rng.standard_normal(x.shape)                  # (the policy acts around a nominal the samples do not start on)
    return dict(name=name, example=ex, n=n, m=m, N=N, S=S, B=B, nparam=P.shape[0], kw=kw, wrap=wrap, params=P, K=K, Sigma=Sigma, x0=x0, u=u,
                x=x, lims=lims, seed=sum(map(ord, name)) * 7919 + (1 << 40))


def model_of(c):
    return MODELS[c["example"]] if c["example"] in MODELS else lq_model(c["n"], c["m"]) + (None, None)


@functools.lru_cache(maxsize=None)
def noise_of(name):
    c = case(name)
    return normals(c["seed"], c["m"], c["N"], c["S"], c["B"])


@functools.lru_cache(maxsize=None)
def reference(name, plant=False):
    """(xs[n,N,S,B], us, cs) in float64 of the long double rollout with the reference stream as noise"""
    c = case(name)
    xi = noise_of(name)
    out = [rollout(model_of(c), c["params"][:, b], c["K"][..., b], c["Sigma"][..., b], c["x0"][:, b], c["u"][..., b], c["x"][..., b], xi[..., b],
                   c["lims"], c["wrap"], plant) for b in range(c["B"])]
    return tuple(np.stack([o[k] for o in out], axis=-1).astype(np.float64) for k in range(3))


# ---- the LQ covariance case of the moments test: n = 3, m = 2, N = 6, B = 2, S = 4096, no limits
def lq_cov_case():
    rng = np.random.default_rng(606)
    n, m, N, B, S = 3, 2, 6, 2, 4096
    A = np.stack([0.9 * np.eye(n) + 0.2 * rng.standard_normal((n, n)) for _ in range(B)], axis=-1)
    Bm = rng.standard_normal((n, m, B))
    Q, R = np.eye(n), np.eye(m)
    P = np.stack([np.concatenate([A[..., b].flatten(order="F"), Bm[..., b].flatten(order="F"), Q.flatten(), R.flatten()]) for b in range(B)], axis=-1)
    K = -0.3 * rng.random((m, n, N, B))
    Sigma = spd(rng, m, N, B, 0.5)
    # x0 dyadic: every partial sum of S copies is exact, so the sample covariance of step 0 is exactly the 0 of the recursion
    x0 = np.array([[1.0, -0.5, 0.25], [0.5, 2.0, -1.0]]).T
    u = 0.3 * rng.standard_normal((m, N, B))
    x = rng.standard_normal((n, N, B))
    cov = np.zeros((n, n, N, B), dtype=LD)
    for b in range(B):
        for i in range(N - 1):
            M = (A[..., b] + Bm[..., b] @ K[:, :, i, b]).astype(LD)
            cov[:, :, i + 1, b] = M @ cov[:, :, i, b] @ M.T + Bm[..., b].astype(LD) @ Sigma[:, :, i, b].astype(LD) @ Bm[..., b].T.astype(LD)
    return dict(n=n, m=m, N=N, B=B, S=S, nparam=P.shape[0], params=P, K=K, Sigma=Sigma, x0=x0, u=u, x=x, cov=cov.astype(np.float64))


def lq_cov_within(cov_hat, c, k=6.0):
    """every entry of cov_hat[n,n,N,B] within k standard errors sqrt((s_ii s_jj + s_ij^2) / (S - 1)) of the exact recursion"""
    s = c["cov"]
    d = np.einsum("iitb->itb", s)
    se = np.sqrt((d[:, None] * d[None, :] + s * s) / (c["S"] - 1))
    return np.abs(cov_hat - s) <= k * se, np.abs(cov_hat - s), se


def lq_cov_reference_samples(c, seed):
    """the sample covariance the reference sampler gives for `seed` (float64 arithmetic, all samples at once)"""
    n, m, N, B, S = c["n"], c["m"], c["N"], c["B"], c["S"]
    xi = normals(seed, m, N, S, B)
    cov = np.zeros((n, n, N, B))
    f, cost = lq_model(n, m)
    for b in range(B):
        xs = rollout((f, cost, None, None), c["params"][:, b], c["K"][..., b], c["Sigma"][..., b], c["x0"][:, b], c["u"][..., b], c["x"][..., b],
                     xi[..., b])[0].astype(np.float64)
        for i in range(N):
            cov[:, :, i, b] = np.cov(xs[:, i, :]) if S > 1 else np.nan
    return cov


LQ_COV_SEED = 2024          # chosen on the CPU (tests/test_user_sample_cpu.py checks it): the reference sampler is inside the bound on every entry
