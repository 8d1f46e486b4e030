// car_ad.hip with DDP_USER_CONSTRAINTS: the same kinematic car (n = 4, m = 2, nparam = 10, nc = 2, flags DDP_USER_TERMINAL |
// DDP_USER_AUTODIFF | DDP_USER_CONSTRAINTS).  The obstacle is a keep-out disc, stated as a constraint instead of a tuned soft cost, and
// the speed is capped.
// params (per trajectory) = [h, gx, gy, ox, oy, r, wo, wu, wt, vmax]: as in car.hip (wo = 0 switches the soft obstacle cost off), then the cap.
template <class T> __device__ void dynamics(const T *x, const T *u, int i, const double *p, T *xnext)
{
    const double h = p[0];
    xnext[0] = x[0] + h * x[3] * cos(x[2]);
    xnext[1] = x[1] + h * x[3] * sin(x[2]);
    xnext[2] = x[2] + h * u[1];
    xnext[3] = x[3] + h * u[0];
}

template <class T> __device__ T stage_cost(const T *x, const T *u, int i, const double *p)
{
    const T dx = x[0] - p[3], dy = x[1] - p[4];
    const double r2 = p[5] * p[5];
    return 0.5 * p[7] * (u[0] * u[0] + u[1] * u[1]) + p[6] * exp(-(dx * dx + dy * dy) / r2);
}

template <class T> __device__ T terminal_cost(const T *x, const double *p)
{
    const T ex = x[0] - p[1], ey = x[1] - p[2];
    return 0.5 * p[8] * (ex * ex + ey * ey + x[3] * x[3]);
}

// g[0]: outside the disc; g[1]: the speed of the next step under its cap (state and control together)
template <class T> __device__ void constraints(const T *x, const T *u, int i, const double *p, T *g)
{
    const T dx = x[0] - p[3], dy = x[1] - p[4];
    g[0] = p[5] * p[5] - (dx * dx + dy * dy);
    g[1] = x[3] + p[0] * u[0] - p[9];
}
