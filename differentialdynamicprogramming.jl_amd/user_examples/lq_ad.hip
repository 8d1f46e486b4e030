// lq.hip with DDP_USER_AUTODIFF: the reference's linear-quadratic demo (src/demo_linear.jl:30-50), any n, m, with the model as
// templates over the scalar type T of x and u.  params = [A[n,n], B[n,m], Q[n,n], R[m,m]] column-major (nparam = 2 n^2 + n m + m^2).
// Flags: DDP_USER_AUTODIFF, or DDP_USER_AUTODIFF | DDP_USER_CONST_HESSIAN (cost_hessians below; AD then derives fx, fu, cx, cu only).
template <class T> __device__ void dynamics(const T *x, const T *u, int i, const double *p, T *xnext)
{
    const double *A = p, *B = p + DDP_N * DDP_N;
    for (int r = 0; r < DDP_N; ++r) {
        T s = 0.0, t = 0.0;
        for (int c = 0; c < DDP_N; ++c) s += A[r + DDP_N * c] * x[c];
        for (int c = 0; c < DDP_M; ++c) t += B[r + DDP_N * c] * u[c];
        xnext[r] = s + t;
    }
}

template <class T> __device__ T stage_cost(const T *x, const T *u, int i, const double *p)
{
    const double *Q = p + DDP_N * DDP_N + DDP_N * DDP_M, *R = Q + DDP_N * DDP_N;
    T qx = 0.0, ru = 0.0;
    for (int r = 0; r < DDP_N; ++r) {
        T s = 0.0;
        for (int c = 0; c < DDP_N; ++c) s += Q[r + DDP_N * c] * x[c];
        qx += x[r] * s;
    }
    for (int r = 0; r < DDP_M; ++r) {
        T s = 0.0;
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
