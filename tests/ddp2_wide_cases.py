"""NumPy side of the DDP_USER_SECOND_ORDER_WAVE tests: the closures of user_examples/chain_ddp_ad.hip (f, costfun, df) and the analytic
tensor of its dynamics, T[k, a, b, i] = ∂²f_k/∂z_a∂z_b with z = [x; u], for any number of links m (n = 2 m).  The backward pass they
are checked against is tests/ddp2_reference.back_pass2; fd_tensor and swapped_back_pass come from there too."""
import numpy as np

from oracle import np_restatement as npr
from ddp2_reference import back_pass2, fd_tensor, swapped_back_pass  # noqa: F401  (re-exported for the tests)

# h, k, c, kc, w, r, a, g
CHAIN_P = np.array([0.02, 9.0, 0.3, 4.0, 1.0, 0.05, 2.0, 3.0])
NPARAM = 8


def chain_ddp(p, J):
    """f(x, u, i), costfun(x, u) -> [N], df(x, u) -> fx, fu, cx, cu, cxx, cxu, cuu and tens(x, u) -> T[n, n+m, n+m, N] of the chain with
    J links whose torque enters as g tanh(u_j) cos(q_j)"""
    h, k, c, kc, w, r, a, g = p
    n, m = 2 * J, J

    def bend(q):                                                # d_j = q_{j-1} - 2 q_j + q_{j+1}, fixed ends
        z = np.zeros_like(q[:1])
        return np.concatenate([z, q[:-1]]) - 2 * q + np.concatenate([q[1:], z])

    def f(x, u, i):
        q, v = x[:J], x[J:]
        d = bend(q)
        acc = -k * np.sin(q) - c * v + kc * (d + 0.5 * d ** 3) + g * np.tanh(u) * np.cos(q)
        return np.concatenate([q + h * v, v + h * acc])

    def costfun(x, u):
        q, v = x[:J], x[J:]
        return (0.5 * w * (q * q + 0.1 * v * v) + a * (1 - np.cos(q))).sum(0) + 0.5 * r * (u * u).sum(0)

    def df(x, u):
        N = x.shape[1]
        fx = np.zeros((n, n, N)); fu = np.zeros((n, m, N)); cxx = np.zeros((n, n, N))
        I = np.eye(J)
        for t in range(N):
            q = x[:J, t]
            th = np.tanh(u[:, t])
            s = kc * (1 + 1.5 * bend(q) ** 2)                   # kc d/dd (d + d^3 / 2)
            Jq = np.diag(-k * np.cos(q) - 2 * s - g * th * np.sin(q)) + s[:, None] * (np.eye(J, k=1) + np.eye(J, k=-1))
            fx[:, :, t] = np.block([[I, h * I], [h * Jq, (1 - h * c) * I]])
            fu[J:, :, t] = h * np.diag(g * (1 - th * th) * np.cos(q))
            cxx[:, :, t] = np.diag(np.concatenate([w + a * np.cos(q), 0.1 * w * np.ones(J)]))
        cx = np.concatenate([w * x[:J] + a * np.sin(x[:J]), 0.1 * w * x[J:]])
        cuu = np.repeat((r * np.eye(m))[:, :, None], N, axis=2)
        return fx, fu, cx, r * u, cxx, np.zeros((n, m, N)), cuu

    def tens(x, u):
        N = x.shape[1]
        T = np.zeros((n, n + m, n + m, N))
        q = x[:J]
        d = bend(q)
        th = np.tanh(u); d1 = 1 - th * th
        for j in range(J):
            row = J + j
            T[row, j, j] += h * k * np.sin(q[j])                                  # -k sin q_j
            nb = [(a_, w_) for a_, w_ in ((j - 1, 1.0), (j, -2.0), (j + 1, 1.0)) if 0 <= a_ < J]
            for a_, wa in nb:                                                    # kc (d + d^3 / 2): 3 kc d ∂d/∂q_a ∂d/∂q_b
                for b_, wb in nb:
                    T[row, a_, b_] += h * kc * 3.0 * d[j] * wa * wb
            cu_ = n + j                                                          # g tanh(u_j) cos(q_j)
            T[row, j, j] -= h * g * th[j] * np.cos(q[j])
            T[row, j, cu_] -= h * g * d1[j] * np.sin(q[j])
            T[row, cu_, j] -= h * g * d1[j] * np.sin(q[j])
            T[row, cu_, cu_] += h * g * (-2 * th[j] * d1[j]) * np.cos(q[j])
        return T

    return f, costfun, df, tens


def solve(p, J, x0, u0, lims, second, **kw):
    """np_restatement.iLQG on the chain with J links; second: with the curvature terms in the backward pass"""
    f, costfun, df, tens = chain_ddp(p, J)
    with swapped_back_pass(tens if second else None):
        return npr.iLQG(f, costfun, df, x0, u0, lims=lims, **kw)
