// chain_ddp_ad.hip — chain_ad.hip with the torque entering through the pendulum: `+ g tanh(u_j) cos(q_j)` in place of `+ u_j`, so that the
// dynamics have curvature in x (fxx), in u (fuu) and mixed (fxu): the model of DDP_USER_SECOND_ORDER_WAVE (full DDP at large shapes).  Any
// m, n = 2 m (up to n = 64, m = 32), nparam = 8 at every size: params = [h, k, c, kc, w, r, a, g].
// State x = [q; v] (angles, then rates).  With d_j = q_{j-1} - 2 q_j + q_{j+1} and both ends of the chain fixed (q_{-1} = q_m = 0):
//   acc_j = -k sin q_j - c v_j + kc (d_j + d_j^3 / 2) + g tanh(u_j) cos(q_j),     q+ = q + h v,   v+ = v + h acc
// Stage cost: Σ_j 0.5 w (q_j^2 + 0.1 v_j^2) + a (1 - cos q_j) + 0.5 r u_j^2.
// Flags: DDP_USER_AUTODIFF (| DDP_USER_WAVE | DDP_USER_SECOND_ORDER_WAVE above n = 32 or m = 8, DDP_USER_SECOND_ORDER below).
static_assert(DDP_N == 2 * DDP_M, "chain_ddp_ad: n = 2 m (x = [q; v])");

template <class T> __device__ void dynamics(const T *x, const T *u, int i, const double *p, T *xnext)
{
    constexpr int J = DDP_M;
    const double h = p[0], k = p[1], c = p[2], kc = p[3], g = p[7];
    for (int j = 0; j < J; ++j) {
        T d = -2.0 * x[j];
        if (j > 0) d += x[j - 1];
        if (j < J - 1) d += x[j + 1];
        const T acc = -k * sin(x[j]) - c * x[J + j] + kc * (d + 0.5 * d * d * d) + g * tanh(u[j]) * cos(x[j]);
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
