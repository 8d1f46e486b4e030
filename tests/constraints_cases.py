"""NumPy side of the DDP_USER_CONSTRAINTS tests (tests/test_user_constraints_cpu.py, tests/test_gpu_user_constraints.py): the closures of
user_examples/car_keepout_ad.hip, the analytic gradient and Hessian of the Powell-Hestenes-Rockafellar term

    ψ = Σ_j (max(0, λ_j + μ g_j)² − λ_j²) / (2μ),     ∇ψ = Σ_j ψ'_j ∇g_j,     ∇²ψ = Σ_j μ·1[λ_j + μ g_j > 0] ∇g_j∇g_jᵀ + ψ'_j ∇²g_j,

with ψ'_j = max(0, λ_j + μ g_j), an augmented-Lagrangian loop around oracle.np_restatement.iLQG (imported, nothing under oracle/ changes),
and the designed inputs: every straight path from the start to the goal crosses the keep-out disc and the speed cap binds on the way.
No control limits in the parity cases: box-QP ties are known to part GPU and NumPy solves."""
import functools

import numpy as np

from oracle import np_restatement as npr

N_STATE, N_CTRL, NPARAM, NC = 4, 2, 10, 2
AL_DEFAULTS = dict(mu0=1.0, mu_factor=10.0, mu_max=1e8, ctol=1e-5, max_outer=20)


def designed(seed, B, N):
    """params[10, B] = [h, gx, gy, ox, oy, r, wo, wu, wt, vmax], x0[4, B], u0[2, N, B].  The soft obstacle cost is off (wo = 0): the disc
    is a constraint.  The disc sits on the segment from the start to the goal, a little to one side, so the unconstrained optimum cuts
    through it; the goal needs a mean speed above the cap."""
    rng = np.random.default_rng(seed)
    h = 0.1
    T = h * N
    p = np.zeros((NPARAM, B))
    p[0] = h
    p[1] = 1.2 * T + 0.1 * rng.standard_normal(B)                 # goal: a mean speed of about 1.2
    p[2] = 0.05 * rng.standard_normal(B)
    p[3] = 0.5 * p[1] + 0.05 * rng.standard_normal(B)             # the disc: half way, off the axis by a fraction of its radius
    p[4] = rng.choice([-1.0, 1.0], B) * rng.uniform(0.05, 0.15, B)
    p[5] = rng.uniform(0.3, 0.4, B)
    p[6] = 0.0
    p[7] = 0.1
    p[8] = 10.0
    p[9] = rng.uniform(1.3, 1.4, B)                               # the cap: above the mean speed, below what the free optimum reaches
    x0 = np.zeros((N_STATE, B))
    x0[3] = 1.0 + 0.05 * rng.standard_normal(B)
    u0 = 0.01 * rng.standard_normal((N_CTRL, N, B))
    return p, x0, u0


def dynamics(p, x, u):
    h = p[0]
    return np.array([x[0] + h * x[3] * np.cos(x[2]), x[1] + h * x[3] * np.sin(x[2]), x[2] + h * u[1], x[3] + h * u[0]])


def constraints(p, x, u):
    """g[2, ...] at x[4, ...], u[2, ...]"""
    dx, dy = x[0] - p[3], x[1] - p[4]
    return np.array([p[5] * p[5] - (dx * dx + dy * dy), x[3] + p[0] * u[0] - p[9]])


def constraint_derivs(p, x, u):
    """∇g[2, 6] and ∇²g[2, 6, 6] at one (x, u), z = [x; u]"""
    dx, dy = x[0] - p[3], x[1] - p[4]
    G = np.zeros((NC, 6), dtype=np.result_type(x, u, p))
    G[0, 0], G[0, 1] = -2 * dx, -2 * dy
    G[1, 3], G[1, 4] = 1.0, p[0]
    H = np.zeros((NC, 6, 6), dtype=G.dtype)
    H[0, 0, 0] = H[0, 1, 1] = -2.0
    return G, H


def raw_stage(p, x, u):
    """the user's stage cost with gradient[6] and Hessian[6, 6] at one (x, u)"""
    dx, dy = x[0] - p[3], x[1] - p[4]
    r2 = p[5] * p[5]
    E = p[6] * np.exp(-(dx * dx + dy * dy) / r2)
    c = 0.5 * p[7] * (u[0] * u[0] + u[1] * u[1]) + E
    dt = np.result_type(x, u, p)
    g = np.zeros(6, dtype=dt)
    H = np.zeros((6, 6), dtype=dt)
    g[0], g[1] = -2 * dx / r2 * E, -2 * dy / r2 * E
    g[4], g[5] = p[7] * u[0], p[7] * u[1]
    H[0, 0] = E * (4 * dx * dx / (r2 * r2) - 2 / r2)
    H[1, 1] = E * (4 * dy * dy / (r2 * r2) - 2 / r2)
    H[0, 1] = H[1, 0] = E * 4 * dx * dy / (r2 * r2)
    H[4, 4] = H[5, 5] = p[7]
    return c, g, H


def psi(p, x, u, lam, mu):
    """ψ with gradient[6] and Hessian[6, 6] at one (x, u) under λ[2], μ (μ <= 0: zeros); works in whatever precision its inputs have"""
    dt = np.result_type(x, u, p, lam)
    if mu <= 0:
        return dt.type(0), np.zeros(6, dtype=dt), np.zeros((6, 6), dtype=dt)
    g = constraints(p, x, u)
    G, H2 = constraint_derivs(p, x, u)
    t = lam + mu * g
    on = t > 0
    dpsi = np.where(on, t, 0)
    val = np.sum(dpsi * dpsi - lam * lam) / (2 * mu)
    grad = dpsi @ G
    hess = np.einsum("j,ja,jb->ab", np.where(on, mu, 0).astype(dt), G, G) + np.einsum("j,jab->ab", dpsi, H2)
    return val, grad, hess


def terminal(p, x):
    ex, ey = x[0] - p[1], x[1] - p[2]
    c = 0.5 * p[8] * (ex * ex + ey * ey + x[3] * x[3])
    g = np.array([p[8] * ex, p[8] * ey, 0.0, p[8] * x[3]])
    H = np.diag([p[8], p[8], 0.0, p[8]])
    return c, g, H


def cost_trajectory(p, x, u, lam=None, mu=0.0):
    """cost[N + 1] of one trajectory x[4, N], u[2, N]: augmented stage costs, then the terminal cost on x[:, N-1]"""
    N = u.shape[1]
    c = np.empty(N + 1)
    for i in range(N):
        c[i] = raw_stage(p, x[:, i], u[:, i])[0] + (psi(p, x[:, i], u[:, i], lam[:, i], mu)[0] if lam is not None else 0.0)
    c[N] = terminal(p, x[:, N - 1])[0]
    return c


def derivs_trajectory(p, x, u, lam=None, mu=0.0):
    """fx, fu, cx, cu, cxx, cxu, cuu of one trajectory, as ddp_user_df writes them (terminal terms added at i = N - 1)"""
    n, m, N = N_STATE, N_CTRL, u.shape[1]
    h = p[0]
    fx = np.zeros((n, n, N)); fu = np.zeros((n, m, N))
    cx = np.zeros((n, N)); cu = np.zeros((m, N)); cxx = np.zeros((n, n, N)); cxu = np.zeros((n, m, N)); cuu = np.zeros((m, m, N))
    for i in range(N):
        th, v = x[2, i], x[3, i]
        fx[:, :, i] = np.eye(n)
        fx[0, 2, i], fx[0, 3, i] = -h * v * np.sin(th), h * np.cos(th)
        fx[1, 2, i], fx[1, 3, i] = h * v * np.cos(th), h * np.sin(th)
        fu[2, 1, i] = h
        fu[3, 0, i] = h
        _, g, H = raw_stage(p, x[:, i], u[:, i])
        if lam is not None:
            _, g2, H2 = psi(p, x[:, i], u[:, i], lam[:, i], mu)
            g, H = g + g2, H + H2
        if i == N - 1:
            _, gt, Ht = terminal(p, x[:, i])
            g[:n] += gt
            H[:n, :n] += Ht
        cx[:, i], cu[:, i] = g[:n], g[n:]
        cxx[:, :, i], cxu[:, :, i], cuu[:, :, i] = H[:n, :n], H[:n, n:], H[n:, n:]
    return fx, fu, cx, cu, cxx, cxu, cuu


def closures(p, lam, mu):
    """f, costfun, df of oracle.np_restatement.iLQG for one trajectory under (λ[2, N], μ)"""
    def f(x, u, i):
        return dynamics(p, x, u)

    def costfun(x, u):
        return cost_trajectory(p, x, u, lam, mu)

    def df(x, u):
        return derivs_trajectory(p, x, u, lam, mu)

    return f, costfun, df


def update(lam, mu, g, mu_factor, mu_max):
    """λ⁺ = max(0, λ + μ g), μ⁺ = min(mu_factor μ, mu_max): NumPy rounds every product and sum, as the update kernel does"""
    return np.maximum(0.0, lam + mu * g), min(mu_factor * mu, mu_max)


def al_loop(p, x0, u0, *, mu0=1.0, mu_factor=10.0, mu_max=1e8, ctol=1e-5, max_outer=20, **ilqg_kw):
    """The loop of ddp_user_ilqg_al for one trajectory, around oracle.np_restatement.iLQG.  Returns (status, rounds): one record per round
    with x, u, the (λ, μ) the round was solved under, g, cviol and the inner iteration count.  A later round starts from x[:, 0] and the
    last u: the initial rollout at α = 1 reproduces the last x."""
    N = u0.shape[1]
    lam, mu = np.zeros((NC, N)), mu0
    xs, us = x0, u0
    rounds = []
    for r in range(max_outer):
        out = npr.iLQG(*closures(p, lam, mu), xs, us.copy(), **ilqg_kw)
        if out is None:
            return -1, rounds
        x, u, _, _, _, cost, info = out
        g = constraints(p, x, u)
        cviol = max(0.0, float(g.max()))
        rounds.append(dict(x=x, u=u, lam=lam.copy(), mu=mu, g=g, cviol=cviol, iter=info["iter"], cost=cost, inner_status=info["status"]))
        if cviol <= ctol:
            return 1, rounds
        if r + 1 == max_outer:
            return 2, rounds
        lam, mu = update(lam, mu, g, mu_factor, mu_max)
        xs, us = x[:, 0].copy(), u
    return 2, rounds


@functools.lru_cache(maxsize=None)
def reference(seed, B, N):
    """the designed inputs, the unconstrained NumPy solves and the NumPy loops on them, computed once per process and left unchanged"""
    p, x0, u0 = designed(seed, B, N)
    plain = [npr.iLQG(*closures(p[:, b], None, 0.0), x0[:, b], u0[:, :, b].copy()) for b in range(B)]
    loops = [al_loop(p[:, b], x0[:, b], u0[:, :, b], **AL_DEFAULTS) for b in range(B)]
    return p, x0, u0, plain, loops


def rollout(p, x0, u):
    """x[4, N] of one trajectory under u[2, N]"""
    x = np.empty((N_STATE, u.shape[1]))
    x[:, 0] = x0
    for i in range(u.shape[1] - 1):
        x[:, i + 1] = dynamics(p, x[:, i], u[:, i])
    return x
