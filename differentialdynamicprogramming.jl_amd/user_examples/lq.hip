// The reference's linear-quadratic demo (src/demo_linear.jl:30-50) as a user problem, any n, m.
// params = [A[n,n], B[n,m], Q[n,n], R[m,m]] column-major (nparam = 2 n^2 + n m + m^2), shared or one column per trajectory.
// Flags: none, or DDP_USER_CONST_HESSIAN (cost_hessians below).
__device__ void dynamics(const double *x, const double *u, int i, const double *p, double *xnext)
{
    const double *A = p, *B = p + DDP_N * DDP_N;
    for (int r = 0; r < DDP_N; ++r) {
        double s = 0.0, t = 0.0;
        for (int c = 0; c < DDP_N; ++c) s += A[r + DDP_N * c] * x[c];
        for (int c = 0; c < DDP_M; ++c) t += B[r + DDP_N * c] * u[c];
        xnext[r] = s + t;
    }
}

__device__ double stage_cost(const double *x, const double *u, int i, const double *p)
{
    const double *Q = p + DDP_N * DDP_N + DDP_N * DDP_M, *R = Q + DDP_N * DDP_N;
    double qx = 0.0, ru = 0.0;
    for (int r = 0; r < DDP_N; ++r) {
        double s = 0.0;
        for (int c = 0; c < DDP_N; ++c) s += Q[r + DDP_N * c] * x[c];
        qx += x[r] * s;
    }
    for (int r = 0; r < DDP_M; ++r) {
        double s = 0.0;
        for (int c = 0; c < DDP_M; ++c) s += R[r + DDP_M * c] * u[c];
        ru += u[r] * s;
    }
    return 0.5 * qx + 0.5 * ru;
}

__device__ void cost_hessians(const double *p, double *cxx, double *cxu, double *cuu)
{
    const double *Q = p + DDP_N * DDP_N + DDP_N * DDP_M, *R = Q + DDP_N * DDP_N;
    for (int e = 0; e < DDP_N * DDP_N; ++e) cxx[e] = Q[e];
    for (int e = 0; e < DDP_N * DDP_M; ++e) cxu[e] = 0.0;
    for (int e = 0; e < DDP_M * DDP_M; ++e) cuu[e] = R[e];
}

__device__ void derivatives(const double *x, const double *u, int i, int N, const double *p, double *fx, double *fu, double *cx,
                            double *cu, double *cxx, double *cxu, double *cuu)
{
    const double *A = p, *B = p + DDP_N * DDP_N, *Q = B + DDP_N * DDP_M, *R = Q + DDP_N * DDP_N;
    for (int e = 0; e < DDP_N * DDP_N; ++e) fx[e] = A[e];
    for (int e = 0; e < DDP_N * DDP_M; ++e) fu[e] = B[e];
    for (int r = 0; r < DDP_N; ++r) {
        double s = 0.0;
        for (int c = 0; c < DDP_N; ++c) s += Q[r + DDP_N * c] * x[c];
        cx[r] = s;
    }
    for (int r = 0; r < DDP_M; ++r) {
        double s = 0.0;
        for (int c = 0; c < DDP_M; ++c) s += R[r + DDP_M * c] * u[c];
        cu[r] = s;
    }
    cost_hessians(p, cxx, cxu, cuu);
}
