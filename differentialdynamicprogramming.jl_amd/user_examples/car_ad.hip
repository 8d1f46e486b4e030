// car.hip with DDP_USER_AUTODIFF: the same kinematic car (n = 4, m = 2, nparam = 9, flags DDP_USER_TERMINAL | DDP_USER_AUTODIFF) with
// the model as templates over the scalar type T of x and u; the library derives fx, fu, cx, cu, cxx, cxu, cuu.
// params (per trajectory) = [h, gx, gy, ox, oy, r, wo, wu, wt], as in car.hip.
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
