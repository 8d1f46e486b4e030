"""Cases and long double models for DDP_USER_SAMPLE_WAVE (tests/test_user_sample_wave_cpu.py, tests/test_gpu_user_sample_wave.py), built
on tests/sample_reference.py (normals, chol_lower, rollout, lq_model, the pendcart model): no GPU, no library.

  * the chain of user_examples/chain_ad.hip and the plant of user_examples/chain_plant_ad.hip restated in long double
    (tests/test_user_wave_cpu.py holds the float64 closures they are compared against);
  * the seven cases of the GPU tests and their long double reference rollouts, each computed once.

SPW below is the number of samples per work-group of ddp_user_sample_wave, 64 / WG with WG the power of two >= m, 8 at least.
"""
import functools

import numpy as np

import sample_reference as sr

LD = np.longdouble
CHAIN_P = np.array([0.02, 9.0, 0.3, 4.0, 1.0, 0.05, 2.0])       # h, k, c, kc, w, r, a (as tests/test_user_wave_cpu.py)
CHAIN_PLANT_TAIL = np.array([0.8, 0.5])                         # gp, cp


def chain_model(J):
    """(f, cost, None, plant) of the chain with J links, x[n, S] and u[m, S] in long double; the plant reads p[7], p[8]"""
    def bend(q):                                                 # d_j = q_{j-1} - 2 q_j + q_{j+1}, fixed ends
        d = -2 * q
        d[1:] += q[:-1]
        d[:-1] += q[1:]
        return d

    def step(x, u, p, damp, gain):
        q, v = x[:J], x[J:]
        d = bend(q)
        acc = -p[1] * np.sin(q) - damp * v + p[3] * (d + LD(0.5) * d * d * d) + gain * u
        return np.concatenate([q + p[0] * v, v + p[0] * acc])

    def f(x, u, i, p):
        return step(x, u, p, p[2], LD(1))

    def plant(x, u, i, p):
        gain = p[7] / (1 + LD(0.05) * np.arange(J, dtype=LD))
        return step(x, u, p, p[8], gain[:, None] if x.ndim == 2 else gain)

    def cost(x, u, i, p):
        q, v = x[:J], x[J:]
        return (LD(0.5) * p[4] * (q * q + LD(0.1) * v * v) + p[6] * (1 - np.cos(q))).sum(0) + LD(0.5) * p[5] * (u * u).sum(0)
    return f, cost, None, plant


def wg_of(m):
    return 8 if m <= 8 else (16 if m <= 16 else 32)


# name: (example, n, m, N, S, B, DeviceProblem keywords, wrap, lims half-width or None)
TABLE = {
    "chain_plant_64x32": ("chain_plant_ad", 64, 32, 5, 5, 3, dict(autodiff=True, plant=True), (), None),    # the edge of the box
    "chain_34x17": ("chain_ad", 34, 17, 6, 3, 3, dict(autodiff=True), (), None),            # n no multiple of WG, m odd, S = SPW + 1
    "lq_ad_40x12": ("lq_ad", 40, 12, 7, 4, 3, dict(autodiff=True), (), 0.35),               # four samples per wave (S = SPW), lims
    "lq_33x2": ("lq", 33, 2, 8, 7, 1, {}, (), None),                                        # narrow factor, no AUTODIFF, B = 1, S = SPW - 1
    "lq_10x9": ("lq", 10, 9, 1, 65, 3, {}, (), None),                                       # m just past 8, N = 1, S = 65
    "pendcart_4x1": ("pendcart_ad", 4, 1, 9, 5, 3, dict(terminal=True, autodiff=True), (0,), None),     # terminal, the wrapped angle
    "chain_16x8": ("chain_ad", 16, 8, 5, 1, 3, dict(autodiff=True), (), None),              # inside the lane box, S = 1
}
NAMES = tuple(TABLE)


def model_of(c):
    ex = c["example"]
    if ex.startswith("chain"):
        return chain_model(c["m"])
    if ex.startswith("pendcart"):
        return sr.MODELS["pendcart"]
    return sr.lq_model(c["n"], c["m"]) + (None, None)


@functools.lru_cache(maxsize=None)
def case(name):
    """inputs of one case, as sample_reference.case: dict(example, n, m, N, S, B, nparam, kw, wrap, params[np,B], K, Sigma, x0, u, x, lims, seed)"""
    ex, n, m, N, S, B, kw, wrap, lim = TABLE[name]
    rng = np.random.default_rng(sum(map(ord, name)))
    if ex.startswith("chain"):
        P = np.repeat(CHAIN_P[:, None], B, axis=1)
        P[1] *= 1 + 0.1 * np.arange(B); P[2] += 0.05 * np.arange(B)          # per-trajectory stiffness and damping
        if ex == "chain_plant_ad":
            P = np.vstack([P, np.repeat(CHAIN_PLANT_TAIL[:, None], B, axis=1) * (1 + 0.05 * np.arange(B))])
        x0 = 0.4 * rng.standard_normal((n, B))
        u = 0.5 * rng.standard_normal((m, N, B))
        K = -0.5 / np.sqrt(n) * rng.random((m, n, N, B))
        scale = 0.3
    elif ex.startswith("pendcart"):
        Q = np.diag([10.0, 1.0, 2.0, 1.0])
        base = np.concatenate([[9.82, 0.35, 0.01, 0.99], [np.pi, 0, 0, 0], Q.flatten(order="F"), [1.0]])
        P = np.repeat(base[:, None], B, axis=1)
        P[1] *= 1 + 0.1 * np.arange(B)
        x0 = np.array([[np.pi, 0.0, 0.0, 0.0]]).T + 0.02 * rng.standard_normal((n, B))
        x0[0] += 0.05 * (np.arange(B) - 1)                          # the trajectories start below, at and above π
        u = 0.5 * rng.standard_normal((m, N, B))
        K = -1.0 * rng.random((m, n, N, B))
        scale = 0.5
    else:
        A = np.stack([0.7 * np.eye(n) + 0.2 / np.sqrt(n) * rng.standard_normal((n, n)) for _ in range(B)], axis=-1)
        Bm = rng.standard_normal((n, m, B)) / np.sqrt(n)
        Q, R = np.eye(n) + 0.1 * np.ones((n, n)), np.eye(m) + 0.05 * np.ones((m, m))
        P = np.stack([np.concatenate([A[..., b].flatten(order="F"), Bm[..., b].flatten(order="F"), Q.flatten(order="F"), R.flatten(order="F")])
                      for b in range(B)], axis=-1)
        x0 = rng.standard_normal((n, B))
        u = 0.3 * rng.standard_normal((m, N, B))
        K = -0.3 / np.sqrt(n) * rng.random((m, n, N, B))
        scale = 0.3
    Sigma = sr.spd(rng, m, N, B, scale)
    c = dict(name=name, example=ex, n=n, m=m, N=N, S=S, B=B, nparam=P.shape[0], kw=kw, wrap=wrap, params=P, K=K, Sigma=Sigma, x0=x0, u=u,
             lims=None if lim is None else np.repeat(np.array([[-lim, lim]]), m, axis=0), seed=sum(map(ord, name)) * 7919 + (1 << 40),
             wg=wg_of(m), spw=64 // wg_of(m))
    # the nominal states: the model's rollout of u without feedback, in double, moved a little (the policy acts around a nominal the
    # samples do not start on)
    x = np.zeros((n, N, B))
    for b in range(B):
        x[..., b] = sr.rollout(model_of(c), P[:, b], np.zeros((m, n, N)), None, x0[:, b], u[..., b], np.zeros((n, N)), 1)[0][..., 0]
    x = x + 0.05 * rng.standard_normal(x.shape)
    if wrap:
        # the nominal angle a turn ahead of the samples at steps 1, 4, 7 and a turn behind at steps 2, 5, 8 (|x̂ − x| > π on both sides,
        # diff brings it back); the samples themselves sit on both sides of π
        x[0, 1::3] += 2 * np.pi
        x[0, 2::3] -= 2 * np.pi
    c["x"] = x
    return c


@functools.lru_cache(maxsize=None)
def noise_of(name, S=None):
    c = case(name)
    return sr.normals(c["seed"], c["m"], c["N"], c["S"] if S is None else S, c["B"])


@functools.lru_cache(maxsize=None)
def reference_ld(name, plant=False, S=None, noise=True):
    """(xs[n,N,S,B], us, cs) of the long double rollout with the reference stream as noise (noise=False: Σ empty), in long double"""
    c = case(name)
    xi = noise_of(name, S)
    S = xi.shape[2]
    out = [sr.rollout(model_of(c), c["params"][:, b], c["K"][..., b], c["Sigma"][..., b] if noise else None, c["x0"][:, b], c["u"][..., b],
                      c["x"][..., b], xi[..., b] if noise else S, c["lims"], c["wrap"], plant) for b in range(c["B"])]
    return tuple(np.stack([o[k] for o in out], axis=-1) for k in range(3))


def reference(name, plant=False, S=None, noise=True):
    """the same in float64"""
    return tuple(a.astype(np.float64) for a in reference_ld(name, plant, S, noise))
