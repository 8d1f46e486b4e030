// car_track.hip with DDP_USER_AUTODIFF: the same car on a clock (n = 4, m = 2, nparam = 7 + 4 L, flags DDP_USER_CLOCK |
// DDP_USER_TERMINAL | DDP_USER_AUTODIFF) with the model as templates over the scalar type T of x and u; i, t and p stay plain.
// params (per trajectory) = [h, r, wo, wu, wp, wt, L, ref(2, L)..., obs(2, L)...], as in car_track.hip.
__device__ int track_k(int t, const double *p)
{
    const int L = (int)p[6];
    return 7 + 2 * (t < L - 1 ? t : L - 1);
}

template <class T> __device__ void dynamics(const T *x, const T *u, int i, int t, const double *p, T *xnext)
{
    const double h = p[0];
    xnext[0] = x[0] + h * x[3] * cos(x[2]);
    xnext[1] = x[1] + h * x[3] * sin(x[2]);
    xnext[2] = x[2] + h * u[1];
    xnext[3] = x[3] + h * u[0];
}

template <class T> __device__ T stage_cost(const T *x, const T *u, int i, int t, const double *p)
{
    const int k = track_k(t, p), L = (int)p[6];
    const T ex = x[0] - p[k], ey = x[1] - p[k + 1], dx = x[0] - p[k + 2 * L], dy = x[1] - p[k + 2 * L + 1];
    const double r2 = p[1] * p[1];
    return 0.5 * p[3] * (u[0] * u[0] + u[1] * u[1]) + 0.5 * p[4] * (ex * ex + ey * ey) + p[2] * exp(-(dx * dx + dy * dy) / r2);
}

template <class T> __device__ T terminal_cost(const T *x, int t, const double *p)
{
    const int k = track_k(t, p);
    const T ex = x[0] - p[k], ey = x[1] - p[k + 1];
    return 0.5 * p[5] * (ex * ex + ey * ey + x[3] * x[3]);
}
