// The kinematic car of car.hip on a clock (n = 4, m = 2, flags DDP_USER_CLOCK | DDP_USER_TERMINAL): it follows a sampled reference path
// past an obstacle that moves along a sampled path of its own.  The model sees the absolute step t = c + i behind i, so one set of
// samples serves every solve of a closed loop and every problem of a queue, whenever they start.
// params (per trajectory) = [h, r, wo, wu, wp, wt, L, ref(2, L)..., obs(2, L)...] (nparam = 7 + 4 L): Euler step h, obstacle radius r and
// weight wo, control weight wu, tracking weight wp, terminal weight wt, the number of samples L, the reference and obstacle positions
// at the steps 0 .. L-1 (column-major: x then y of every step); both paths are read at min(t, L - 1).
//   stage cost   .5 wu |u|^2 + .5 wp |pos - ref(t)|^2 + wo exp(-|pos - obs(t)|^2 / r^2)
//   terminal     .5 wt (|pos - ref(t)|^2 + v^2),  t = c + N - 1
__device__ int track_k(int t, const double *p)
{
    const int L = (int)p[6];
    return 7 + 2 * (t < L - 1 ? t : L - 1);
}

__device__ void dynamics(const double *x, const double *u, int i, int t, const double *p, double *xnext)
{
    const double h = p[0];
    xnext[0] = x[0] + h * x[3] * cos(x[2]);
    xnext[1] = x[1] + h * x[3] * sin(x[2]);
    xnext[2] = x[2] + h * u[1];
    xnext[3] = x[3] + h * u[0];
}

__device__ double stage_cost(const double *x, const double *u, int i, int t, const double *p)
{
    const int k = track_k(t, p), L = (int)p[6];
    const double ex = x[0] - p[k], ey = x[1] - p[k + 1], dx = x[0] - p[k + 2 * L], dy = x[1] - p[k + 2 * L + 1], r2 = p[1] * p[1];
    return 0.5 * p[3] * (u[0] * u[0] + u[1] * u[1]) + 0.5 * p[4] * (ex * ex + ey * ey) + p[2] * exp(-(dx * dx + dy * dy) / r2);
}

__device__ double terminal_cost(const double *x, int t, const double *p)
{
    const int k = track_k(t, p);
    const double ex = x[0] - p[k], ey = x[1] - p[k + 1];
    return 0.5 * p[5] * (ex * ex + ey * ey + x[3] * x[3]);
}

__device__ void derivatives(const double *x, const double *u, int i, int t, int N, const double *p, double *fx, double *fu, double *cx,
                            double *cu, double *cxx, double *cxu, double *cuu)
{
    const double h = p[0], c = cos(x[2]), s = sin(x[2]);
    for (int e = 0; e < 16; ++e) fx[e] = (e % 5 == 0) ? 1.0 : 0.0;
    fx[0 + 4 * 2] = -h * x[3] * s;
    fx[0 + 4 * 3] = h * c;
    fx[1 + 4 * 2] = h * x[3] * c;
    fx[1 + 4 * 3] = h * s;
    for (int e = 0; e < 8; ++e) fu[e] = 0.0;
    fu[3 + 4 * 0] = h;
    fu[2 + 4 * 1] = h;
    // tracking: .5 wp |pos - ref|^2;  obstacle: phi = wo exp(-(dx^2 + dy^2) / r^2)
    const int k = track_k(t, p), L = (int)p[6];
    const double ex = x[0] - p[k], ey = x[1] - p[k + 1], dx = x[0] - p[k + 2 * L], dy = x[1] - p[k + 2 * L + 1], r2 = p[1] * p[1];
    const double phi = p[2] * exp(-(dx * dx + dy * dy) / r2), q = -2.0 / r2, wp = p[4];
    for (int e = 0; e < 16; ++e) cxx[e] = 0.0;
    cx[0] = wp * ex + phi * q * dx; cx[1] = wp * ey + phi * q * dy; cx[2] = 0.0; cx[3] = 0.0;
    cxx[0] = wp + phi * (q + q * q * dx * dx);
    cxx[5] = wp + phi * (q + q * q * dy * dy);
    cxx[1] = cxx[4] = phi * q * q * dx * dy;
    if (i == N - 1) {                                          // the terminal cost acts on x[:,N-1], at the same t
        const double wt = p[5];
        cx[0] += wt * ex; cx[1] += wt * ey; cx[3] += wt * x[3];
        cxx[0] += wt; cxx[5] += wt; cxx[15] += wt;
    }
    cu[0] = p[3] * u[0]; cu[1] = p[3] * u[1];
    for (int e = 0; e < 8; ++e) cxu[e] = 0.0;
    cuu[0] = p[3]; cuu[1] = 0.0; cuu[2] = 0.0; cuu[3] = p[3];
}
