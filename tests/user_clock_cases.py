"""Shared by tests/test_user_clock_cpu.py and tests/test_gpu_user_clock.py: the parameters of the car_track examples, their model in
NumPy, and the UNCLOCKED TWIN the GPU tests compare a clocked problem with — the example's own text with t replaced by i, run through
the entry points that existed before the flag, with the sampled paths in its parameter column shifted by the clock on the host."""
import numpy as np

L_TRACK = 64


def nparam_of(name):
    return 7 + (6 if name == "car_track_plant" else 4) * L_TRACK


def twin_source(src, N):
    """car_track.hip without the clock: the old signatures, the paths read at min(i, L-1) — and at N-1 in terminal_cost, which has no i"""
    s = src.replace("int i, int t, ", "int i, ")
    s = s.replace("const double *x, int t, const double *p)", "const double *x, const double *p)")
    a = s.index("double terminal_cost(")
    b = s.index("\n}\n", a)
    s = s[:a] + s[a:b].replace("track_k(t, p)", "track_k(%d, p)" % (N - 1)) + s[b:]
    return s.replace("track_k(t, p)", "track_k(i, p)")


def shifted(P, t0):
    """params[nparam, B] with every sampled path of column b moved forward by t0[b] steps (clamped at its last sample): what a clocked
    problem with the clocks t0 reads at t0[b] + i, the twin reads at i"""
    Q = np.array(P, order="F", copy=True)
    L = int(P[6, 0])
    t0 = np.broadcast_to(np.asarray(t0), (P.shape[1],))
    for b, c in enumerate(t0):
        idx = np.minimum(np.arange(L) + int(c), L - 1)
        for off in range(7, P.shape[0], 2 * L):
            Q[off:off + 2 * L, b] = P[off:off + 2 * L, b].reshape(2, L, order="F")[:, idx].ravel(order="F")
    return Q


def track_params(rng, B, L=L_TRACK, plant=False):
    """params[nparam, B] of the car_track examples: a reference that moves along a curve, an obstacle that crosses it"""
    s = np.arange(L)
    P = np.zeros((7 + (6 if plant else 4) * L, B))
    for b in range(B):
        h, r, wo, wu, wp, wt = 0.1, 0.6 + 0.1 * rng.random(), 2.0 + rng.random(), 0.05, 1.0 + rng.random(), 5.0
        ref = np.stack([0.12 * s + 0.3 * rng.standard_normal(), 0.8 * np.sin(0.11 * s + rng.random())])
        obs = np.stack([4.0 - 0.05 * s + 0.2 * rng.standard_normal(), 0.9 * np.cos(0.07 * s + rng.random())])
        P[:7, b] = (h, r, wo, wu, wp, wt, L)
        P[7:7 + 2 * L, b] = ref.ravel(order="F")
        P[7 + 2 * L:7 + 4 * L, b] = obs.ravel(order="F")
    return P


def track_cost(p, x, u, i, t, N):
    L = int(p[6])
    k = 7 + 2 * min(t, L - 1)
    ex, ey, dx, dy = x[0] - p[k], x[1] - p[k + 1], x[0] - p[k + 2 * L], x[1] - p[k + 2 * L + 1]
    c = 0.5 * p[3] * (u @ u) + 0.5 * p[4] * (ex * ex + ey * ey) + p[2] * np.exp(-(dx * dx + dy * dy) / p[1] ** 2)
    if i == N - 1:
        c += 0.5 * p[5] * (ex * ex + ey * ey + x[3] ** 2)
    return c


def track_f(p, x, u):
    h = p[0]
    return np.array([x[0] + h * x[3] * np.cos(x[2]), x[1] + h * x[3] * np.sin(x[2]), x[2] + h * u[1], x[3] + h * u[0]])


