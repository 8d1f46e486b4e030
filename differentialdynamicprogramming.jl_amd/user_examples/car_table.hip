// The car's cost on a tabulated time-varying affine model: what a user could do before DDP_USER_FITTED to plan on fitted dynamics.
// x = (px, py, θ, v), u = (acceleration, turn rate), n = 4, m = 2, flag DDP_USER_TERMINAL.
// params (per trajectory) = [h, gx, gy, ox, oy, r, wo, wu, wt | T_0 | T_1 | ... | T_{N-1}] (nparam = 9 + 28 N), the cost parameters of
// car.hip (h is not used) and per step i the 28 doubles T_i = [fx_i (16, column-major) | fu_i (8, column-major) | fc_i (4)]:
//   dynamics     x+ = fc_i + fx_i x + fu_i u        (per component: fc, then the columns of fx, then those of fu)
//   stage cost   .5 wu |u|^2 + wo exp(-|p - o|^2 / r^2),   terminal .5 wt (|p - g|^2 + v^2)
// The tables live in the parameter block, so the horizon is bounded by DDP_USER_MAX_NPARAM (N <= 145 here; N <= 3 at n = 32, m = 8),
// and every lane reads its own block with 8-byte accesses.  ddp_user_rollout_fit takes the tables as arrays instead.
#define CAR_TABLE(p, i) ((p) + 9 + 28 * (i))

__device__ void dynamics(const double *x, const double *u, int i, const double *p, double *xnext)
{
    const double *T = CAR_TABLE(p, i);
    for (int l = 0; l < 4; ++l) xnext[l] = T[24 + l];
    for (int j = 0; j < 4; ++j)
        for (int l = 0; l < 4; ++l) xnext[l] += T[l + 4 * j] * x[j];
    for (int q = 0; q < 2; ++q)
        for (int l = 0; l < 4; ++l) xnext[l] += T[16 + l + 4 * q] * u[q];
}

__device__ double stage_cost(const double *x, const double *u, int i, const double *p)
{
    const double ax = x[0] - p[3], ay = x[1] - p[4];
    return 0.5 * p[7] * (u[0] * u[0] + u[1] * u[1]) + p[6] * exp(-(ax * ax + ay * ay) / (p[5] * p[5]));
}

__device__ double terminal_cost(const double *x, const double *p)
{
    const double ex = x[0] - p[1], ey = x[1] - p[2];
    return 0.5 * p[8] * (ex * ex + ey * ey + x[3] * x[3]);
}

__device__ void derivatives(const double *x, const double *u, int i, int N, const double *p, double *fx, double *fu, double *cx,
                            double *cu, double *cxx, double *cxu, double *cuu)
{
    const double *T = CAR_TABLE(p, i);
    for (int e = 0; e < 16; ++e) fx[e] = T[e];
    for (int e = 0; e < 8; ++e) fu[e] = T[16 + e];
    // the obstacle term w(x) = wo exp(s |p - o|^2), s = -1 / r^2: ∇w = 2 s w a, ∇²w = 2 s w (I + 2 s a a'), a = p - o
    const double ax = x[0] - p[3], ay = x[1] - p[4], s = -1.0 / (p[5] * p[5]);
    const double w = p[6] * exp(s * (ax * ax + ay * ay)), g = 2.0 * s * w;
    for (int e = 0; e < 16; ++e) cxx[e] = 0.0;
    for (int e = 0; e < 8; ++e) cxu[e] = 0.0;
    cx[0] = g * ax; cx[1] = g * ay; cx[2] = 0.0; cx[3] = 0.0;
    cxx[0 + 4 * 0] = g * (1.0 + 2.0 * s * ax * ax);
    cxx[1 + 4 * 1] = g * (1.0 + 2.0 * s * ay * ay);
    cxx[0 + 4 * 1] = cxx[1 + 4 * 0] = g * 2.0 * s * ax * ay;
    if (i == N - 1) {                                          // the terminal cost acts on the last state
        cx[0] += p[8] * (x[0] - p[1]); cx[1] += p[8] * (x[1] - p[2]); cx[3] += p[8] * x[3];
        cxx[0 + 4 * 0] += p[8]; cxx[1 + 4 * 1] += p[8]; cxx[3 + 4 * 3] += p[8];
    }
    cu[0] = p[7] * u[0]; cu[1] = p[7] * u[1];
    cuu[0] = p[7]; cuu[1] = 0.0; cuu[2] = 0.0; cuu[3] = p[7];
}
