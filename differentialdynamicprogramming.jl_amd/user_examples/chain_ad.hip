// chain_ad.hip — a chain of m actuated pendulums coupled by hardening springs, with DDP_USER_AUTODIFF: any m, n = 2 m (up to the
// largest shape of DDP_USER_WAVE, n = 64, m = 32), nparam = 7 at every size: params = [h, k, c, kc, w, r, a].
// State x = [q; v] (angles, then rates).  With d_j = q_{j-1} - 2 q_j + q_{j+1} and both ends of the chain fixed (q_{-1} = q_m = 0):
//   acc_j = -k sin q_j - c v_j + kc (d_j + d_j^3 / 2) + u_j,     q+ = q + h v,   v+ = v + h acc
// Stage cost: Σ_j 0.5 w (q_j^2 + 0.1 v_j^2) + a (1 - cos q_j) + 0.5 r u_j^2: neither the dynamics nor the cost is quadratic, the
// Jacobians are banded.  Flags: DDP_USER_AUTODIFF (| DDP_USER_WAVE above n = 32 or m = 8).
static_assert(DDP_N == 2 * DDP_M, "chain_ad: n = 2 m (x = [q; v])");

template <class T> __device__ void dynamics(const T *x, const T *u, int i, const double *p, T *xnext)
{
    constexpr int J = DDP_M;
    const double h = p[0], k = p[1], c = p[2], kc = p[3];
    for (int j = 0; j < J; ++j) {
        T d = -2.0 * x[j];
        if (j > 0) d += x[j - 1];
        if (j < J - 1) d += x[j + 1];
        const T acc = -k * sin(x[j]) - c * x[J + j] + kc * (d + 0.5 * d * d * d) + u[j];
        xnext[j] = x[j] + h * x[J + j];
        xnext[J + j] = x[J + j] + h * acc;
    }
}

template <class T> __device__ T stage_cost(const T *x, const T *u, int i, const double *p)
{
    constexpr int J = DDP_M;
    const double w = p[4], r = p[5], a = p[6];
    T s = 0.0;
    for (int j = 0; j < J; ++j)
        s += 0.5 * w * (x[j] * x[j] + 0.1 * x[J + j] * x[J + j]) + a * (1.0 - cos(x[j])) + 0.5 * r * u[j] * u[j];
    return s;
}
