// The kinematic car of car.hip with a plant for the closed loop (flags DDP_USER_TERMINAL | DDP_USER_PLANT): the solver plans with the
// model below while the system it controls has another actuator gain and drifts.
// params (per trajectory) = [h, gx, gy, ox, oy, r, wo, wu, wt,  ga, gw, vx, vy] (nparam = 13): the model's nine of car.hip, then the
// plant's: gains ga, gw on the acceleration and the turn rate, and a constant drift velocity (vx, vy) of the position.
//   plant   x_{t+1} = f(x_t, (ga u_0, gw u_1)) + h (vx, vy, 0, 0)
__device__ void dynamics(const double *x, const double *u, int i, const double *p, double *xnext)
{
    const double h = p[0];
    xnext[0] = x[0] + h * x[3] * cos(x[2]);
    xnext[1] = x[1] + h * x[3] * sin(x[2]);
    xnext[2] = x[2] + h * u[1];
    xnext[3] = x[3] + h * u[0];
}

__device__ double stage_cost(const double *x, const double *u, int i, const double *p)
{
    const double dx = x[0] - p[3], dy = x[1] - p[4], r2 = p[5] * p[5];
    return 0.5 * p[7] * (u[0] * u[0] + u[1] * u[1]) + p[6] * exp(-(dx * dx + dy * dy) / r2);
}

__device__ double terminal_cost(const double *x, const double *p)
{
    const double ex = x[0] - p[1], ey = x[1] - p[2];
    return 0.5 * p[8] * (ex * ex + ey * ey + x[3] * x[3]);
}

__device__ void derivatives(const double *x, const double *u, int i, int N, const double *p, double *fx, double *fu, double *cx,
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
    // obstacle: phi = wo exp(-(dx^2 + dy^2) / r^2)
    const double dx = x[0] - p[3], dy = x[1] - p[4], r2 = p[5] * p[5];
    const double phi = p[6] * exp(-(dx * dx + dy * dy) / r2), k = -2.0 / r2;
    for (int e = 0; e < 16; ++e) cxx[e] = 0.0;
    cx[0] = phi * k * dx; cx[1] = phi * k * dy; cx[2] = 0.0; cx[3] = 0.0;
    cxx[0] = phi * (k + k * k * dx * dx);
    cxx[5] = phi * (k + k * k * dy * dy);
    cxx[1] = cxx[4] = phi * k * k * dx * dy;
    if (i == N - 1) {                                          // the terminal cost acts on x[:,N-1]
        const double wt = p[8];
        cx[0] += wt * (x[0] - p[1]); cx[1] += wt * (x[1] - p[2]); cx[3] += wt * x[3];
        cxx[0] += wt; cxx[5] += wt; cxx[15] += wt;
    }
    cu[0] = p[7] * u[0]; cu[1] = p[7] * u[1];
    for (int e = 0; e < 8; ++e) cxu[e] = 0.0;
    cuu[0] = p[7]; cuu[1] = 0.0; cuu[2] = 0.0; cuu[3] = p[7];
}

__device__ void plant(const double *x, const double *u, int t, const double *p, double *xnext)
{
    const double h = p[0], ua[2] = {p[9] * u[0], p[10] * u[1]};
    dynamics(x, ua, t, p, xnext);
    xnext[0] += h * p[11];
    xnext[1] += h * p[12];
}
