// pendcart.hip with DDP_USER_AUTODIFF: the same pendulum on a cart (n = 4, m = 1, nparam = 25, flags DDP_USER_TERMINAL |
// DDP_USER_AUTODIFF) with the model as templates over the scalar type T of x and u.  The terminal cost's gradient and Hessian at the
// last step (the hand-written w = 2) are added by the library.  params = [g, l, h, d, goal[4], Q[4,4], R], as in pendcart.hip.
template <class T> __device__ void dynamics(const T *x, const T *u, int i, const double *p, T *xnext)
{
    const double g = p[0], l = p[1], h = p[2], d = p[3];
    const double gl = g / l;
    xnext[0] = x[0] + h * x[1];
    xnext[1] = x[1] + h * (-gl * sin(x[0]) + u[0] / l * cos(x[0]) - d * x[1]);
    xnext[2] = x[2] + h * x[3];
    xnext[3] = x[3] + h * u[0];
}

template <class T> __device__ T pend_state_cost(const T *x, const double *p)
{
    const double *goal = p + 4, *Q = p + 8;
    T c = 0.0;
    for (int r = 0; r < 4; ++r) {
        T s = 0.0;
        for (int k = 0; k < 4; ++k) s += Q[r + 4 * k] * (x[k] - goal[k]);
        c += (x[r] - goal[r]) * s;
    }
    return c;
}

template <class T> __device__ T stage_cost(const T *x, const T *u, int i, const double *p)
{
    return 0.5 * (pend_state_cost(x, p) + p[24] * u[0] * u[0]);
}

template <class T> __device__ T terminal_cost(const T *x, const double *p) { return 0.5 * pend_state_cost(x, p); }
