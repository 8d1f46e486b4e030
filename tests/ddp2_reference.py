"""NumPy reference of the second-order backward pass (DDP_USER_SECOND_ORDER) for the tests: `back_pass2` restates
backward_pass.jl:81-129 over the box-QP and Cholesky of oracle/np_restatement.py with `vectens(v, t) = Σ_k v[k] t[k]` (undefined
upstream, fixed in include/ddp_amd.h), the closures of user_examples/bicycle_ad.hip and of a 24-state chain with their analytic
second derivatives T[k, a, b, i] = ∂²f_k/∂z_a∂z_b (z = [x; u]), and whole solves: np_restatement.iLQG with its module-level
`back_pass` swapped for the duration of a call."""
import contextlib

import numpy as np
import scipy.linalg as sla

from oracle import np_restatement as npr


def back_pass2(cx, cu, cxx, cxu, cuu, fx, fu, T, lam, regType, lims, x, u):
    """backward_pass.jl:81-129.  cxx / cxu / cuu 3-D (time-varying) or 2-D (DDP_USER_CONST_HESSIAN).  Written as
    np_restatement.back_pass with the three tensor terms added where the reference adds them: with T = 0 it returns that function's
    arrays bit for bit."""
    m, N = u.shape
    n = fx.shape[0]
    c_tv = cxx.ndim == 3
    k = np.zeros((m, N)); K = np.zeros((m, n, N)); Vx = np.zeros((n, N)); Vxx = np.zeros((n, n, N)); Quu = np.zeros((m, m, N))
    dV = np.zeros(2)
    Vx[:, N - 1] = cx[:, N - 1]
    Vxx[:, :, N - 1] = cxx[:, :, N - 1] if c_tv else cxx
    Quu[:, :, N - 1] = cuu[:, :, N - 1] if c_tv else cuu
    no_lims = (lims is None) or (np.size(lims) == 0) or (lims[0, 0] > lims[0, 1])
    In, Im = np.eye(n), np.eye(m)
    for i in range(N - 2, -1, -1):
        fxi, fui = fx[:, :, i], fu[:, :, i]
        cxxi = cxx[:, :, i] if c_tv else cxx
        cxui = cxu[:, :, i] if c_tv else cxu
        cuui = cuu[:, :, i] if c_tv else cuu
        V = Vxx[:, :, i + 1]
        H = np.tensordot(Vx[:, i + 1], T[:, :, :, i], axes=(0, 0))
        Hxx, Hux, Huu = H[:n, :n], H[n:, :n], H[n:, n:]
        Qu = cu[:, i] + fui.T @ Vx[:, i + 1]
        Qx = cx[:, i] + fxi.T @ Vx[:, i + 1]
        Qux = cxui.T + (fui.T @ V) @ fxi + Hux
        Quu[:, :, i] = cuui + (fui.T @ V) @ fui + Huu
        Qxx = cxxi + (fxi.T @ V) @ fxi + Hxx
        Vreg = V + (lam * In if regType == 2 else 0)
        Qux_reg = cxui.T + (fui.T @ Vreg) @ fxi + Hux
        QuuF = cuui + (fui.T @ Vreg) @ fui + (lam * Im if regType == 1 else 0) + Huu
        if no_lims:
            try:
                R = npr._chol_upper(QuuF)
            except npr.PosDef:
                return i + 1, (K, k, Quu), Vx, Vxx, dV
            k_i = -sla.cho_solve((R, False), Qu)
            K_i = -sla.cho_solve((R, False), Qux_reg)
        else:
            lower = lims[:, 0] - u[:, i]; upper = lims[:, 1] - u[:, i]
            ws = min(i + 1, N - 2)
            try:
                k_i, result, R, free = npr.boxQP(QuuF, Qu, lower, upper, k[:, ws].copy())
            except npr.PosDef:
                result = 0
            if result < 1:
                return i + 1, (K, k, Quu), Vx, Vxx, dV
            K_i = np.zeros((m, n))
            if free.any():
                y = sla.solve_triangular(R, Qux_reg[free, :], trans='T', lower=False)
                K_i[free, :] = -sla.solve_triangular(R, y, lower=False)
        Quuk = Quu[:, :, i] @ k_i
        kQuuk = k_i @ Quuk
        KQuuk = K_i.T @ Quuk
        KQuuK = (K_i.T @ Quu[:, :, i]) @ K_i
        dV = dV + np.array([k_i @ Qu, 0.5 * kQuuk])
        Vx[:, i] = Qx + KQuuk + K_i.T @ Qu + Qux.T @ k_i
        M = Qxx + KQuuK + K_i.T @ Qux + Qux.T @ K_i
        Vxx[:, :, i] = (M + M.T) / 2
        k[:, i] = k_i; K[:, :, i] = K_i
    return 0, (K, k, Quu), Vx, Vxx, dV


# ---------------------------------------------------------------- kinematic bicycle (user_examples/bicycle_ad.hip)
# x = (px, py, θ, v), u = (a, δ); p = [h, L, gx, gy, ox, oy, r, wo, wu, wt]
def bicycle(p):
    h, L, gx, gy, ox, oy, r, wo, wu, wt = p

    def f(x, u, i):
        return np.array([x[0] + h * x[3] * np.cos(x[2]), x[1] + h * x[3] * np.sin(x[2]), x[2] + h * x[3] * np.tan(u[1]) / L, x[3] + h * u[0]])

    def costfun(x, u):
        dx, dy = x[0] - ox, x[1] - oy
        c = 0.5 * wu * (u[0] ** 2 + u[1] ** 2) + wo * np.exp(-(dx * dx + dy * dy) / r ** 2)
        e = x[:, -1]
        return np.concatenate([c, [0.5 * wt * ((e[0] - gx) ** 2 + (e[1] - gy) ** 2 + e[3] ** 2)]])

    def df(x, u):
        n, N = x.shape
        fx = np.zeros((4, 4, N)); fu = np.zeros((4, 2, N))
        for j in range(4):
            fx[j, j] = 1.0
        c, s = np.cos(x[2]), np.sin(x[2]); t = np.tan(u[1]); se = 1 / np.cos(u[1]) ** 2
        fx[0, 2] = -h * x[3] * s; fx[0, 3] = h * c; fx[1, 2] = h * x[3] * c; fx[1, 3] = h * s
        fx[2, 3] = h * t / L
        fu[3, 0] = h; fu[2, 1] = h * x[3] * se / L
        dx, dy = x[0] - ox, x[1] - oy
        phi = wo * np.exp(-(dx * dx + dy * dy) / r ** 2); k = -2.0 / r ** 2
        cx = np.zeros((4, N)); cxx = np.zeros((4, 4, N))
        cx[0] = phi * k * dx; cx[1] = phi * k * dy
        cxx[0, 0] = phi * (k + k * k * dx * dx); cxx[1, 1] = phi * (k + k * k * dy * dy); cxx[0, 1] = cxx[1, 0] = phi * k * k * dx * dy
        cx[0, -1] += wt * (x[0, -1] - gx); cx[1, -1] += wt * (x[1, -1] - gy); cx[3, -1] += wt * x[3, -1]
        cxx[0, 0, -1] += wt; cxx[1, 1, -1] += wt; cxx[3, 3, -1] += wt
        cuu = np.zeros((2, 2, N)); cuu[0, 0] = cuu[1, 1] = wu
        return fx, fu, cx, wu * u, cxx, np.zeros((4, 2, N)), cuu

    def tens(x, u):
        N = x.shape[1]
        T = np.zeros((4, 6, 6, N))
        c, s = np.cos(x[2]), np.sin(x[2]); t = np.tan(u[1]); se = 1 / np.cos(u[1]) ** 2
        T[0, 2, 2] = -h * x[3] * c; T[0, 2, 3] = T[0, 3, 2] = -h * s
        T[1, 2, 2] = -h * x[3] * s; T[1, 2, 3] = T[1, 3, 2] = h * c
        T[2, 3, 5] = T[2, 5, 3] = h * se / L
        T[2, 5, 5] = 2 * h * x[3] * se * t / L
        return T

    return f, costfun, df, tens


def car_tens(p, x, u):
    """second derivatives of user_examples/car_ad.hip's dynamics (p[0] = h): the bicycle's without the steering terms"""
    h = p[0]
    T = np.zeros((4, 6, 6, x.shape[1]))
    c, s = np.cos(x[2]), np.sin(x[2])
    T[0, 2, 2] = -h * x[3] * c; T[0, 2, 3] = T[0, 3, 2] = -h * s
    T[1, 2, 2] = -h * x[3] * s; T[1, 2, 3] = T[1, 3, 2] = h * c
    return T


def sketch_inputs(seed=11, B=16, N=60):
    """the 16 bicycle problems of the issue's measurements: params[10, B], x0[4, B], u0[2, N, B] (per problem: 8 uniform draws for
    the parameters, 3 for the start state, then the controls)"""
    rng = np.random.default_rng(seed)
    P = np.zeros((10, B)); x0 = np.zeros((4, B)); u0 = np.zeros((2, N, B))
    for b in range(B):
        P[:, b] = [0.05, 0.5, 4 + rng.uniform(-.5, .5), 4 + rng.uniform(-.5, .5), 2 + rng.uniform(-.3, .3), 2 + rng.uniform(-.3, .3),
                   0.6 + rng.uniform(0, .3), rng.uniform(5, 20), 0.1, rng.uniform(5, 20)]
        x0[:, b] = [rng.uniform(0, .5), rng.uniform(0, .5), np.pi / 4 + rng.uniform(-.2, .2), 0.5]
        u0[:, :, b] = 0.1 * rng.standard_normal((2, N))
    return P, x0, u0


BICYCLE_LIMS = np.array([[-2.0, 2.0], [-0.6, 0.6]])


# ---------------------------------------------------------------- chain: 12 masses on nonlinear springs, n = 24, m = 4
# x = (q_0..q_11, w_0..w_11), u_c pushes mass 3c through tanh(u_c) cos(q_3c); p = [h, k, g, wq, wu]
CHAIN_N, CHAIN_M, CHAIN_NP = 24, 4, 5
CHAIN_SOURCE = """
template <class T> __device__ void dynamics(const T *x, const T *u, int i, const double *p, T *xnext)
{
    const double h = p[0], k = p[1], g = p[2];
#pragma unroll
    for (int j = 0; j < 12; ++j) {
        xnext[j] = x[j] + h * x[12 + j];
        T acc;
        if (j > 0) acc = -k * sin(x[j] - x[j - 1]);
        else acc = -k * sin(x[j]);
        if (j < 11) acc += k * sin(x[j + 1] - x[j]);
        if (j % 3 == 0) acc += g * tanh(u[j / 3]) * cos(x[j]);
        xnext[12 + j] = x[12 + j] + h * acc;
    }
}

template <class T> __device__ T stage_cost(const T *x, const T *u, int i, const double *p)
{
    T cq(0.0), cu(0.0);
#pragma unroll
    for (int j = 0; j < 24; ++j) cq += x[j] * x[j];
#pragma unroll
    for (int c = 0; c < 4; ++c) cu += u[c] * u[c];
    return 0.5 * p[3] * cq + 0.5 * p[4] * cu;
}
"""
CHAIN_P = np.array([0.05, 3.0, 2.0, 1.0, 0.1])


def chain(p=CHAIN_P):
    h, k, g, wq, wu = p

    def f(x, u, i):
        q, w = x[:12], x[12:]
        acc = -k * np.sin(q - np.concatenate([[0.0], q[:-1]]))
        acc[:-1] += k * np.sin(q[1:] - q[:-1])
        acc[0::3] += g * np.tanh(u) * np.cos(q[0::3])
        return np.concatenate([q + h * w, w + h * acc])

    def tens(x, u):
        N = x.shape[1]
        T = np.zeros((24, 28, 28, N))
        for j in range(12):
            r = 12 + j
            s = np.sin(x[j] - x[j - 1]) if j > 0 else np.sin(x[j])            # -k sin(q_j - q_{j-1})
            T[r, j, j] += h * k * s
            if j > 0:
                T[r, j - 1, j - 1] += h * k * s
                T[r, j, j - 1] -= h * k * s; T[r, j - 1, j] -= h * k * s
            if j < 11:                                                      # +k sin(q_{j+1} - q_j)
                s = np.sin(x[j + 1] - x[j])
                T[r, j, j] -= h * k * s; T[r, j + 1, j + 1] -= h * k * s
                T[r, j, j + 1] += h * k * s; T[r, j + 1, j] += h * k * s
            if j % 3 == 0:                                                  # g tanh(u_c) cos(q_j)
                c = 24 + j // 3
                th = np.tanh(u[j // 3]); d1 = 1 - th * th
                T[r, j, j] -= h * g * th * np.cos(x[j])
                T[r, j, c] -= h * g * d1 * np.sin(x[j]); T[r, c, j] -= h * g * d1 * np.sin(x[j])
                T[r, c, c] += h * g * (-2 * th * d1) * np.cos(x[j])
        return T

    return f, tens


def fd_tensor(f, x, u, e=1e-4):
    """T[k, a, b] at one point by second-order central differences of f"""
    z = np.concatenate([x, u]); n = len(x); nz = len(z)
    F = lambda zz: f(zz[:n], zz[n:], 0)
    T = np.zeros((n, nz, nz))
    for a in range(nz):
        for b in range(a, nz):
            da = np.zeros(nz); da[a] = e
            db = np.zeros(nz); db[b] = e
            T[:, a, b] = T[:, b, a] = (F(z + da + db) - F(z + da - db) - F(z - da + db) + F(z - da - db)) / (4 * e * e)
    return T


# ---------------------------------------------------------------- whole solves
@contextlib.contextmanager
def swapped_back_pass(tens):
    """np_restatement.back_pass replaced by back_pass2 with T = tens(x, u) (None: zero tensors) while the block runs"""
    def bp(cx, cu, cxx, cxu, cuu, fx, fu, lam, regType, lims, x, u):
        n, m = x.shape[0], u.shape[0]
        T = tens(x, u) if tens is not None else np.zeros((n, n + m, n + m, x.shape[1]))
        return back_pass2(cx, cu, cxx, cxu, cuu, fx, fu, T, lam, regType, lims, x, u)
    old = npr.back_pass
    npr.back_pass = bp
    try:
        yield
    finally:
        npr.back_pass = old


def solve(p, x0, u0, lims, second, **kw):
    """np_restatement.iLQG on the bicycle with parameters p; second: with the curvature terms"""
    f, costfun, df, tens = bicycle(p)
    with swapped_back_pass(tens if second else None):
        return npr.iLQG(f, costfun, df, x0, u0, lims=lims, **kw)
