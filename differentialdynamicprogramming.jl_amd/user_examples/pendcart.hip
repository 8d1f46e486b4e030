// The reference's pendulum on a cart (src/system_pendcart.jl:83-106) as a user problem: n = 4, m = 1, flag DDP_USER_TERMINAL.
// params = [g, l, h, d, goal[4], Q[4,4], R] (nparam = 25).  f is the explicit Euler step, the cost .5((x-goal)'Q(x-goal) + R u^2)
// per step and .5 (x_N-goal)'Q(x_N-goal) at the end; df is the Euler Jacobian (the built-in family takes the matrix exponential).
__device__ void dynamics(const double *x, const double *u, int i, const double *p, double *xnext)
{
    const double g = p[0], l = p[1], h = p[2], d = p[3];
    const double gl = g / l;
    xnext[0] = x[0] + h * x[1];
    xnext[1] = x[1] + h * (-gl * sin(x[0]) + u[0] / l * cos(x[0]) - d * x[1]);
    xnext[2] = x[2] + h * x[3];
    xnext[3] = x[3] + h * u[0];
}

__device__ double pend_state_cost(const double *x, const double *p)
{
    const double *goal = p + 4, *Q = p + 8;
    double c = 0.0;
    for (int r = 0; r < 4; ++r) {
        double s = 0.0;
        for (int k = 0; k < 4; ++k) s += Q[r + 4 * k] * (x[k] - goal[k]);
        c += (x[r] - goal[r]) * s;
    }
    return c;
}

__device__ double stage_cost(const double *x, const double *u, int i, const double *p)
{
    return 0.5 * (pend_state_cost(x, p) + p[24] * u[0] * u[0]);
}

__device__ double terminal_cost(const double *x, const double *p) { return 0.5 * pend_state_cost(x, p); }

__device__ void derivatives(const double *x, const double *u, int i, int N, const double *p, double *fx, double *fu, double *cx,
                            double *cu, double *cxx, double *cxu, double *cuu)
{
    const double g = p[0], l = p[1], h = p[2], d = p[3], *goal = p + 4, *Q = p + 8, R = p[24];
    const double s0 = sin(x[0]), c0 = cos(x[0]);
    for (int e = 0; e < 16; ++e) fx[e] = (e % 5 == 0) ? 1.0 : 0.0;
    fx[0 + 4 * 1] = h;                                          // d x0' / d x1
    fx[1 + 4 * 0] = h * (-g / l * c0 - u[0] / l * s0);
    fx[1 + 4 * 1] = 1.0 - h * d;
    fx[2 + 4 * 3] = h;
    fu[0] = 0.0; fu[1] = h * c0 / l; fu[2] = 0.0; fu[3] = h;
    const double w = (i == N - 1) ? 2.0 : 1.0;                  // the last step also carries the terminal cost on x[:,N-1]
    for (int r = 0; r < 4; ++r) {
        double s = 0.0;
        for (int k = 0; k < 4; ++k) s += Q[r + 4 * k] * (x[k] - goal[k]);
        cx[r] = w * s;
        for (int k = 0; k < 4; ++k) cxx[r + 4 * k] = w * Q[r + 4 * k];
        cxu[r] = 0.0;
    }
    cu[0] = R * u[0];
    cuu[0] = R;
}
