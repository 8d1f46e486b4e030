"""Reference of DDP_USER_FITTED (ddp_user_rollout_fit, iLQGkl(..., fitted=True)) in NumPy: the rollout formula in long double with the
cost as closures, designed tables, the costs of the bundled examples, the closures of the fitted car for oracle.np_kl.iLQGkl and the
inputs of the whole-loop tests (built without a GPU, so that the CPU suite can assert that the reference converges on them).

    û_i   = clamp(u_i + α k_i + K_i diff(x̂_i, x_i))
    c_i   = stage(x̂_i, û_i, i)
    x̂_i+1 = fc_i + Σ_j fx_i[:,j] x̂_i[j] + Σ_q fu_i[:,q] û_i[q]      for i < N-1        (slot N-1 of the tables is never read)
"""
import numpy as np

from test_gpu_user_problem import car_closures, car_params

LD = np.longdouble
TWO_PI = 2 * np.arccos(LD(-1))


def rollout(x0, u, fx, fu, fc, stage, terminal=None, K=None, k=None, x=None, alpha=1.0, lims=None, wrap=0, dtype=LD):
    """one trajectory: x0[n], u[m,N], tables fx[n,n,N], fu[n,m,N], fc[n,N]; policy K[m,n,N], k[m,N] around x[n,N] or none; lims[m,2];
    wrap: bit mask of the coordinates whose difference is taken modulo 2π (the policy term only).  Every operation in `dtype`.
    Returns xnew[n,N], unew[m,N], cost[N (+1 with terminal)]."""
    T = dtype
    n, N = fc.shape
    m = u.shape[0]
    fx, fu, fc, u = fx.astype(T), fu.astype(T), fc.astype(T), u.astype(T)
    two_pi = T(TWO_PI)
    xh = np.asarray(x0, T).copy()
    xs, us, cs = np.zeros((n, N), T), np.zeros((m, N), T), []
    for i in range(N):
        uu = u[:, i].copy()
        if K is not None:
            d = xh - x[:, i].astype(T)
            for l in range(n):
                if (wrap >> l) & 1:
                    d[l] = d[l] - two_pi * np.rint(d[l] / two_pi)
            uu = uu + T(alpha) * k[:, i].astype(T) + K[:, :, i].astype(T) @ d
        if lims is not None:
            uu = np.minimum(np.maximum(uu, lims[:, 0].astype(T)), lims[:, 1].astype(T))
        xs[:, i], us[:, i] = xh, uu
        cs.append(T(stage(xh, uu, i)))
        if i < N - 1:
            xn = fc[:, i].copy()
            for j in range(n):
                xn = xn + fx[:, j, i] * xh[j]
            for q in range(m):
                xn = xn + fu[:, q, i] * uu[q]
            xh = xn
    if terminal is not None:
        cs.append(T(terminal(xh)))
    return xs, us, np.array(cs, T)


def designed_tables(rng, n, m, N, B, x=None, u=None):
    """fx = I + 0.02 randn, fu = 0.05 randn (spectral radius near 1: N = 40 does not blow up); fc random and small, or, with a nominal
    x[n,N,B], u[m,N,B], the offsets that make it consistent: x[:,i+1] = fx_i x_i + fu_i u_i + fc_i"""
    fx = np.eye(n)[:, :, None, None] + 0.02 * rng.standard_normal((n, n, N, B))
    fu = 0.05 * rng.standard_normal((n, m, N, B))
    fc = 0.01 * rng.standard_normal((n, N, B))
    if x is not None:
        for i in range(N - 1):
            fc[:, i] = x[:, i + 1] - np.einsum("ijb,jb->ib", fx[:, :, i], x[:, i]) - np.einsum("iqb,qb->ib", fu[:, :, i], u[:, i])
    return np.asfortranarray(fx), np.asfortranarray(fu), np.asfortranarray(fc)


# ---- the costs of the bundled examples (user_examples/*.hip), generic in the scalar type of x, u
def car_cost(p):
    h, gx, gy, ox, oy, r, wo, wu, wt = p

    def stage(x, u, i):
        dx, dy = x[0] - ox, x[1] - oy
        return 0.5 * wu * (u[0] * u[0] + u[1] * u[1]) + wo * np.exp(-(dx * dx + dy * dy) / (r * r))

    def terminal(x):
        return 0.5 * wt * ((x[0] - gx) ** 2 + (x[1] - gy) ** 2 + x[3] ** 2)
    return stage, terminal


def lq_cost(Q, R):
    def stage(x, u, i):
        return 0.5 * (x @ (Q.astype(x.dtype) @ x)) + 0.5 * (u @ (R.astype(u.dtype) @ u))
    return stage, None


def pend_cost(P):
    goal, Q, R = P["goal"], P["Q"], P["R"]

    def state(x):
        e = x - goal.astype(x.dtype)
        return e @ (Q.astype(x.dtype) @ e)

    def stage(x, u, i):
        return 0.5 * (state(x) + R * u[0] * u[0])

    def terminal(x):
        return 0.5 * state(x)
    return stage, terminal


# ---- the fitted car: closures (f, costfun, derivs) for oracle.np_kl.iLQGkl
def car_fitted_closures(p, fx, fu, fc):
    """f(x, u, i) is the affine table, derivs returns the fitted fx, fu with the car's cost derivatives (car_closures)"""
    _, costfun, df = car_closures(p)

    def f(x, u, i):
        return fx[:, :, i] @ x + fu[:, :, i] @ u + fc[:, i]

    def derivs(x, u):
        _, _, cx, cu, cxx, cxu, cuu = df(x, u)
        return fx, fu, cx, cu, cxx, cxu, cuu
    return f, costfun, derivs


def car_table_params(P, fx, fu, fc):
    """the parameter block of user_examples/car_table.hip: [9 cost parameters | per step fx (16) | fu (8) | fc (4)], one column per trajectory"""
    N, B = fc.shape[1], fc.shape[2]
    T = np.concatenate([fx.reshape(16, N, B, order="F"), fu.reshape(8, N, B, order="F"), fc], axis=0)       # [28, N, B]
    return np.asfortranarray(np.concatenate([P, T.reshape(28 * N, B, order="F")], axis=0))


def _spd(rng, d, s=1.0):
    a = rng.standard_normal((d, d))
    return s * (a @ a.T / d + 0.5 * np.eye(d))


def loop_case(seed=71, B=3, N=40, gains=(1.3, 0.75), drift=(0.05, -0.03), noise=1e-3, flip_fu=False):
    """The inputs of the whole-loop tests: B cars (car_params), a random control sequence, and tables that are the linearisation of the
    gain-mismatched car (car_plant.hip: the controls act with gains ga, gw and the position drifts) along its own rollout, + `noise` on
    fx, fu, with fc making that rollout consistent; x is the float64 rollout of u on the tables.  flip_fu: fu with the opposite sign
    (a model that contradicts the car's own)."""
    rng = np.random.default_rng(seed)
    P = car_params(rng, B)
    x0 = np.array([0.0, 0.0, 0.3, 0.5])[:, None] + 0.05 * rng.standard_normal((4, B))
    u = 0.3 * rng.standard_normal((2, N, B))
    fx, fu, fc = np.zeros((4, 4, N, B)), np.zeros((4, 2, N, B)), np.zeros((4, N, B))
    G = np.diag(gains)
    for b in range(B):
        f, _, df = car_closures(P[:, b])
        h = P[0, b]
        xp = np.zeros((4, N)); xp[:, 0] = x0[:, b]
        for i in range(N - 1):
            xp[:, i + 1] = f(xp[:, i], G @ u[:, i, b], i) + h * np.array([drift[0], drift[1], 0.0, 0.0])
        jx, ju = df(xp, G @ u[..., b])[:2]
        fx[..., b] = jx + noise * rng.standard_normal((4, 4, N))
        fu[..., b] = np.einsum("iqt,qr->irt", ju, G) + noise * rng.standard_normal((4, 2, N))
        if flip_fu:
            fu[..., b] = -fu[..., b]
        for i in range(N - 1):
            fc[:, i, b] = xp[:, i + 1] - fx[:, :, i, b] @ xp[:, i] - fu[:, :, i, b] @ u[:, i, b]
        fx[:, :, N - 1, b] = 0.0; fu[:, :, N - 1, b] = 0.0          # slot N-1 has no transition (fit_dynamics writes zeros there)
    x = np.zeros((4, N, B)); c = np.zeros((N + 1, B))
    for b in range(B):
        stage, terminal = car_cost(P[:, b])
        xs, _, cs = rollout(x0[:, b], u[..., b], fx[..., b], fu[..., b], fc[..., b], stage, terminal, dtype=np.float64)
        x[..., b], c[:, b] = xs, cs
    Sip = np.stack([np.stack([_spd(rng, 2, 2.0) for _ in range(N)], -1) for _ in range(B)], -1)
    Sp = np.stack([np.stack([np.linalg.inv(Sip[:, :, t, b]) for t in range(N)], -1) for b in range(B)], -1)
    Kp = 0.1 * rng.standard_normal((2, 4, N, B))
    return dict(P=P, x0=x0, u=u, x=x, c=c, fx=np.asfortranarray(fx), fu=np.asfortranarray(fu), fc=np.asfortranarray(fc), Kp=Kp, Sp=Sp,
                Sip=Sip, R1=1e-3 * np.eye(4), B=B, N=N)


def np_loop(case, b, lims=None, kl_step=0.5, max_iter=20):
    """oracle.np_kl.iLQGkl on trajectory b of a loop_case with the fitted closures"""
    from oracle import np_kl
    f, cf, derivs = car_fitted_closures(case["P"][:, b], case["fx"][..., b], case["fu"][..., b], case["fc"][..., b])
    pb = dict(K=case["Kp"][..., b], k=case["u"][..., b], S=case["Sp"][..., b], Si=case["Sip"][..., b])
    return np_kl.iLQGkl(f, cf, derivs, case["x"][..., b], pb, dict(fx=case["fx"][..., b], R1=case["R1"]), kl_step=kl_step, lims=lims,
                        max_iter=max_iter)
