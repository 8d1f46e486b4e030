// chain_plant_ad.hip — the chain of chain_ad.hip with a plant for the closed loop (flags DDP_USER_AUTODIFF | DDP_USER_PLANT, | DDP_USER_WAVE
// above n = 32 or m = 8): any m, n = 2 m, nparam = 9 at every size: params = [h, k, c, kc, w, r, a, gp, cp].  The solver plans with the
// model below (the seven parameters of chain_ad); the true system differs from it in two ways, both the plant's alone:
//   an actuator gain per joint    g_j = gp / (1 + 0.05 j)    (the torque that arrives is g_j u_j, weaker down the chain)
//   another damping               cp in place of c
//   plant   acc_j = -k sin q_j - cp v_j + kc (d_j + d_j^3 / 2) + g_j u_j,     q+ = q + h v,   v+ = v + h acc
// with d_j = q_{j-1} - 2 q_j + q_{j+1} and both ends fixed, as in the model.  With gp = 1 (at j = 0) and cp = c the plant is the model.
static_assert(DDP_N == 2 * DDP_M, "chain_plant_ad: n = 2 m (x = [q; v])");

// the step of the chain with damping `damp` and the torque gain `gain / (1 + 0.05 j)` on joint j
template <class T> __device__ void chain_step(const T *x, const T *u, const double *p, double damp, double gain, T *xnext)
{
    constexpr int J = DDP_M;
    const double h = p[0], k = p[1], kc = p[3];
    for (int j = 0; j < J; ++j) {
        T d = -2.0 * x[j];
        if (j > 0) d += x[j - 1];
        if (j < J - 1) d += x[j + 1];
        const T acc = -k * sin(x[j]) - damp * x[J + j] + kc * (d + 0.5 * d * d * d) + (gain / (1.0 + 0.05 * j)) * u[j];
        xnext[j] = x[j] + h * x[J + j];
        xnext[J + j] = x[J + j] + h * acc;
    }
}

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

__device__ void plant(const double *x, const double *u, int t, const double *p, double *xnext)
{
    chain_step(x, u, p, p[8], p[7], xnext);
}
