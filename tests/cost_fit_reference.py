"""Reference of DDP_USER_COST_FIT (ddp_user_cost_fit, fit_cost) in NumPy: the six formulas in long double, their float64 twin in the
kernel's summation order (the same code, another scalar type), and the designed cases of the CPU and GPU tests.

For one trajectory, from the cost c_s and its derivatives (cx_s, cu_s, cxx_s, cxu_s, cuu_s) at every sample (x̂_s, û_s) of step i, with
δx_s = diff(x̂_s, x_i) (modulo 2π on the wrapped coordinates) and δu_s = û_s - u_i:

    cxx_i = mean_s cxx_s        cxu_i = mean_s cxu_s        cuu_i = mean_s cuu_s
    cx_i  = mean_s (cx_s - cxx_s δx_s - cxu_s δu_s)
    cu_i  = mean_s (cu_s - cxu_sᵀ δx_s - cuu_s δu_s)
    c0_i  = mean_s (c_s - cx_s·δx_s - cu_s·δu_s + ½ [δx_s; δu_s]ᵀ H_s [δx_s; δu_s])

Every sum over the samples runs s = 0..S-1 and is divided by S at the end; inside a sample the sums run j = 0..n-1, then q = 0..m-1.
"""
import re

import numpy as np

LD = np.longdouble
TWO_PI = 2 * np.arccos(LD(-1))
LQ_NP = lambda n, m: 2 * n * n + n * m + m * m                    # noqa: E731


def fit_cost(c, cx, cu, cxx, cxu, cuu, xs, us, x, u, wrap=0, dtype=LD):
    """One trajectory.  Per sample: c[N,S], cx[n,N,S], cu[m,N,S], cxx[n,n,N,S], cxu[n,m,N,S], cuu[m,m,N,S]; the samples xs[n,N,S],
    us[m,N,S]; the nominal x[n,N], u[m,N]; wrap: bit mask of the coordinates whose difference is taken modulo 2π.  Every operation in
    `dtype`, in the order of the kernel.  Returns cx[n,N], cu[m,N], cxx[n,n,N], cxu[n,m,N], cuu[m,m,N], c0[N]."""
    T = dtype
    c, cx, cu, cxx, cxu, cuu, xs, us, x, u = (np.asarray(a).astype(T) for a in (c, cx, cu, cxx, cxu, cuu, xs, us, x, u))
    n, N, S = xs.shape
    m = us.shape[0]
    two_pi = T(TWO_PI)
    ox, ou, oxx, oxu, ouu, o0 = (np.zeros(s, T) for s in ((n, N), (m, N), (n, n, N), (n, m, N), (m, m, N), (N,)))
    for s in range(S):
        dx = xs[:, :, s] - x
        for l in range(n):
            if (wrap >> l) & 1:
                dx[l] = dx[l] - two_pi * np.rint(dx[l] / two_pi)
        du = us[:, :, s] - u
        lin, quad = np.zeros(N, T), np.zeros(N, T)
        for r in range(n):
            h = np.zeros(N, T)
            for j in range(n):
                h = h + cxx[r, j, :, s] * dx[j]
            for q in range(m):
                h = h + cxu[r, q, :, s] * du[q]
            ox[r] = ox[r] + (cx[r, :, s] - h)
            lin = lin + cx[r, :, s] * dx[r]
            quad = quad + dx[r] * h
        for r in range(m):
            h = np.zeros(N, T)
            for j in range(n):
                h = h + cxu[j, r, :, s] * dx[j]
            for q in range(m):
                h = h + cuu[r, q, :, s] * du[q]
            ou[r] = ou[r] + (cu[r, :, s] - h)
            lin = lin + cu[r, :, s] * du[r]
            quad = quad + du[r] * h
        oxx, oxu, ouu = oxx + cxx[..., s], oxu + cxu[..., s], ouu + cuu[..., s]
        o0 = o0 + ((c[:, s] - lin) + T(0.5) * quad)
    return tuple(a / T(S) for a in (ox, ou, oxx, oxu, ouu, o0))


NAMES = ("cx", "cu", "cxx", "cxu", "cuu", "c0")


def layout(ddp, problem):
    """(lanes, steps per work-group, sample indices per round) that the library picks for ddp_user_cost_fit of `problem`"""
    t = ddp._lib.lib().ddp_user_program_text(problem.source.encode(), problem.n, problem.m, problem.nparam, problem.flags,
                                             int(problem.diff_mask)).decode()
    return tuple(int(re.search(r"#define %s (\d+)" % k, t).group(1)) for k in ("DDP_CLANES", "DDP_CCHUNK", "DDP_CSB"))


# ------------------------------------------------------------------------------------------------------------------ the designed cases
# name -> (example source, n, m, nparam, DeviceProblem keywords, wrap mask, N, B, S); N, B, S = None: one step, one trajectory group and one
# sample past the chunk sizes of the layout (`past`)
EXAMPLES = {"lq1": ("lq", 1, 1, LQ_NP(1, 1), {}, 0), "car": ("car", 4, 2, 9, dict(terminal=True), 0),
            "car_ad": ("car_ad", 4, 2, 9, dict(terminal=True, autodiff=True), 0), "lq_ad": ("lq_ad", 5, 3, LQ_NP(5, 3), dict(autodiff=True), 0),
            "lq32": ("lq", 32, 8, LQ_NP(32, 8), dict(const_hessian=True), 0), "pend": ("pendcart", 4, 1, 25, dict(terminal=True), 1)}
SIZES = [("lq1", 2, 2, 2), ("car", 7, 3, 3), ("car", 7, 3, 64), ("car", 7, 3, 65), ("car_ad", 7, 3, 3), ("lq_ad", 17, 2, 5), ("lq32", 3, 2, 5),
         ("pend", 9, 2, 6)] + [(k, None, None, None) for k in EXAMPLES]
IDS = ["%s-N%s-B%s-S%s" % s if s[1] else "%s-past" % s[0] for s in SIZES]


def problem_of(ddp, name, **kw):
    ex, n, m, nparam, pkw, wrap = EXAMPLES[name]
    return ddp.DeviceProblem(ddp.example_source(ex), n, m, nparam=nparam, cost_fit=True, diff=ddp.WrappedDiff(0) if wrap else None,
                             **pkw, **kw)


def _spd(rng, d):
    a = rng.standard_normal((d, d))
    return a @ a.T / d + 0.5 * np.eye(d)


def make_case(ddp, name, N=None, B=None, S=None):
    """the inputs of one designed case: parameters P[nparam,B], the nominal x[n,N,B], u[m,N,B] and the samples xs[n,N,S,B], us[m,N,S,B]
    (the nominal perturbed with a fixed seed; pendcart: the angle of every sample moved by -2π, 0 or 2π, so that the samples sit on both
    sides of the wrap)"""
    ex, n, m, nparam, pkw, wrap = EXAMPLES[name]
    if N is None:
        lanes, chunk, csb = layout(ddp, problem_of(ddp, name))
        N, B, S = chunk + 1, lanes // chunk + 1, csb + 1
    rng = np.random.default_rng(1000 * N + 10 * S + B + sum(map(ord, name)))
    if ex.startswith("car"):
        from test_gpu_user_problem import car_params
        P = car_params(rng, B)
        x = np.stack([rng.uniform(1.0, 3.0, (N, B)), rng.uniform(1.0, 3.0, (N, B)), rng.uniform(-1, 1, (N, B)), rng.uniform(0, 1, (N, B))])
        u, sx, su = 0.3 * rng.standard_normal((m, N, B)), 0.1, 0.1
    elif ex.startswith("lq"):
        from test_gpu_user_problem import lq_params
        P = np.stack([lq_params(rng.standard_normal((n, n)), rng.standard_normal((n, m)), _spd(rng, n), _spd(rng, m)) for _ in range(B)], -1)
        x, u, sx, su = rng.standard_normal((n, N, B)), rng.standard_normal((m, N, B)), 0.3, 0.3
    else:
        from test_gpu_user_problem import pend_params
        P = np.repeat(pend_params()[:, None], B, 1)
        x = np.stack([np.pi + rng.uniform(-0.3, 0.3, (N, B)), rng.standard_normal((N, B)), rng.standard_normal((N, B)), rng.standard_normal((N, B))])
        u, sx, su = rng.standard_normal((m, N, B)), 0.2, 0.2
    xs = x[:, :, None, :] + sx * rng.standard_normal((n, N, S, B))
    us = u[:, :, None, :] + su * rng.standard_normal((m, N, S, B))
    if wrap:
        xs[0] += 2 * np.pi * (np.arange(S) % 3 - 1)[None, :, None]
    f = np.asfortranarray
    return dict(name=name, n=n, m=m, N=N, B=B, S=S, wrap=wrap, P=f(P), x=f(x), u=f(u), xs=f(xs), us=f(us), terminal=bool(pkw.get("terminal")))


def host_derivatives(case, b):
    """c[N,S], cx[n,N,S], cu[m,N,S], cxx[n,n,N,S], cxu[n,m,N,S], cuu[m,m,N,S] of trajectory b at its samples, from the formulas of the
    bundled examples in float64 NumPy (user_examples/car.hip, lq.hip, pendcart.hip; at the last step with the terminal cost)"""
    n, m, N, S, name = case["n"], case["m"], case["N"], case["S"], case["name"]
    p = case["P"][:, b]
    c, cx, cu = np.zeros((N, S)), np.zeros((n, N, S)), np.zeros((m, N, S))
    cxx, cxu, cuu = np.zeros((n, n, N, S)), np.zeros((n, m, N, S)), np.zeros((m, m, N, S))
    for s in range(S):
        X, U = case["xs"][:, :, s, b], case["us"][:, :, s, b]
        if name.startswith("car"):
            from test_gpu_user_problem import car_closures
            _, costfun, df = car_closures(p)
            cc = costfun(X, U)
            c[:, s] = cc[:N]; c[N - 1, s] += cc[N]
            _, _, cx[..., s], cu[..., s], cxx[..., s], cxu[..., s], cuu[..., s] = df(X, U)
        elif name.startswith("lq"):
            Q, R = p[n * n + n * m:2 * n * n + n * m].reshape(n, n, order="F"), p[2 * n * n + n * m:].reshape(m, m, order="F")
            c[:, s] = 0.5 * np.einsum("it,ij,jt->t", X, Q, X) + 0.5 * np.einsum("it,ij,jt->t", U, R, U)
            cx[..., s], cu[..., s] = Q @ X, R @ U
            cxx[..., s], cuu[..., s] = Q[:, :, None], R[:, :, None]
        else:
            goal, Q, R = p[4:8], p[8:24].reshape(4, 4, order="F"), p[24]
            w = np.ones(N); w[N - 1] = 2.0                         # the last step also carries the terminal cost
            E = X - goal[:, None]
            c[:, s] = 0.5 * (w * np.einsum("it,ij,jt->t", E, Q, E) + R * U[0] ** 2)
            cx[..., s], cu[..., s] = w * (Q @ E), R * U
            cxx[..., s], cuu[..., s] = Q[:, :, None] * w, R
    return c, cx, cu, cxx, cxu, cuu
