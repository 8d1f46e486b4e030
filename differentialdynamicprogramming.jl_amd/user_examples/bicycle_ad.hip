// Kinematic bicycle for DDP_USER_AUTODIFF (and DDP_USER_SECOND_ORDER): n = 4 (px, py, θ, v), m = 2 (a, δ), nparam = 10, flags
// DDP_USER_TERMINAL | DDP_USER_AUTODIFF.  The heading follows the steering angle, θ⁺ = θ + h v tan(δ) / L, so unlike car_ad.hip the
// dynamics have mixed and control second derivatives (fxu, fuu ≠ 0).  The cost is the car's: control effort, a Gaussian bump around an
// obstacle, a terminal pull to the goal.  params (per trajectory) = [h, L, gx, gy, ox, oy, r, wo, wu, wt].
template <class T> __device__ void dynamics(const T *x, const T *u, int i, const double *p, T *xnext)
{
    const double h = p[0], L = p[1];
    xnext[0] = x[0] + h * x[3] * cos(x[2]);
    xnext[1] = x[1] + h * x[3] * sin(x[2]);
    xnext[2] = x[2] + h * x[3] * tan(u[1]) / L;
    xnext[3] = x[3] + h * u[0];
}

template <class T> __device__ T stage_cost(const T *x, const T *u, int i, const double *p)
{
    const T dx = x[0] - p[4], dy = x[1] - p[5];
    const double r2 = p[6] * p[6];
    return 0.5 * p[8] * (u[0] * u[0] + u[1] * u[1]) + p[7] * exp(-(dx * dx + dy * dy) / r2);
}

template <class T> __device__ T terminal_cost(const T *x, const double *p)
{
    const T ex = x[0] - p[2], ey = x[1] - p[3];
    return 0.5 * p[9] * (ex * ex + ey * ey + x[3] * x[3]);
}
