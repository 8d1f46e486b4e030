// user_autodiff.h — forward-mode automatic differentiation of a user problem (DDP_USER_AUTODIFF), as program text for hiprtc.
//
// With the flag, the user writes dynamics / stage_cost / terminal_cost as templates over the scalar type of x and u (include/ddp_amd.h)
// and no `derivatives`.  program_text() (user_problem.hip) then compiles
//   DDP_* macros, kUserAutodiff, the user's source, kUserAutodiffDerivs, DDP_USER_ABI, kUserKernels
// and kUserKernels' ddp_user_df_ad calls ddp_ad_derivatives where ddp_user_df calls the user's `derivatives`.
//
//   kUserAutodiff        ddp_dual<V, P>: a value of type V and P partials of type V.  First derivatives: ddp_dual<double, P>;
//                        second derivatives: the dual over a dual ddp_dual<ddp_dual<double, P>, P>.  Every operator and function is
//                        written once, as a chain rule on V, and nests by itself.
//   kUserAutodiffDerivs  ddp_ad_derivatives: fx, fu by DDP_ADJ seeds per call of `dynamics`; cx, cu, cxx, cxu, cuu by the
//                        second-order type over the block upper triangle of z = [x; u] (DDP_ADH seeds per block), mirrored.
//   kUserAutodiffVhess   ddp_ad_vhess: one entry of the Hessian of v·f(z) (DDP_USER_SECOND_ORDER), the pair (a, b) a run-time value.
//
// Neither text uses a device builtin or include: with DDP_AD_FN defined as `inline` (and __device__ as nothing for the user's
// source), both compile as host C++, which is how tests/test_user_autodiff_cpu.py checks the arithmetic without a GPU.  Every loop
// over partials has a compile-time trip count and is unrolled; the chunk and block loops are template recursions, so every seed is a
// constant and every partial array is indexed at compile time only (a runtime-indexed array would live in scratch).
#pragma once

static const char *kUserAutodiff = R"DDPA(
#ifndef DDP_AD_FN
#define DDP_AD_FN __device__ __forceinline__
#endif
// a copy of the parameter pointer the compiler cannot see through: each call of the model reloads its parameters (from the cache)
// instead of keeping every parameter it read in an earlier call live in VGPRs (lq 10x2: A and Q are 200 doubles)
#ifndef DDP_AD_FRESH
#define DDP_AD_FRESH(q) asm volatile("" : "+v"(q))
#endif

template <class V, int P> struct ddp_dual {
    V v;
    V d[P];
    ddp_dual() = default;
    DDP_AD_FN ddp_dual(double c) : v(c)
    {
#pragma unroll
        for (int j = 0; j < P; ++j) d[j] = V(0.0);
    }
    DDP_AD_FN ddp_dual(int c) : ddp_dual((double)c) {}
    DDP_AD_FN ddp_dual &operator+=(const ddp_dual &b)
    {
        v += b.v;
#pragma unroll
        for (int j = 0; j < P; ++j) d[j] += b.d[j];
        return *this;
    }
    DDP_AD_FN ddp_dual &operator-=(const ddp_dual &b)
    {
        v -= b.v;
#pragma unroll
        for (int j = 0; j < P; ++j) d[j] -= b.d[j];
        return *this;
    }
    DDP_AD_FN ddp_dual &operator*=(const ddp_dual &b) { return *this = *this * b; }
    DDP_AD_FN ddp_dual &operator/=(const ddp_dual &b) { return *this = *this / b; }
    DDP_AD_FN ddp_dual &operator+=(double b) { v += b; return *this; }
    DDP_AD_FN ddp_dual &operator-=(double b) { v -= b; return *this; }
    DDP_AD_FN ddp_dual &operator*=(double b) { return *this = *this * b; }
    DDP_AD_FN ddp_dual &operator/=(double b) { return *this = *this / b; }
};

DDP_AD_FN double ddp_value(double a) { return a; }
template <class V, int P> DDP_AD_FN double ddp_value(const ddp_dual<V, P> &a) { return ddp_value(a.v); }

// f(a) with f(a.v) = fv, f'(a.v) = dv
template <class V, int P> DDP_AD_FN ddp_dual<V, P> ddp_chain(const ddp_dual<V, P> &a, const V &fv, const V &dv)
{
    ddp_dual<V, P> r;
    r.v = fv;
#pragma unroll
    for (int j = 0; j < P; ++j) r.d[j] = dv * a.d[j];
    return r;
}

// ---- arithmetic: dual op dual, dual op double, double op dual (an int converts to double)
template <class V, int P> DDP_AD_FN ddp_dual<V, P> operator+(const ddp_dual<V, P> &a) { return a; }
template <class V, int P> DDP_AD_FN ddp_dual<V, P> operator-(const ddp_dual<V, P> &a)
{
    ddp_dual<V, P> r;
    r.v = -a.v;
#pragma unroll
    for (int j = 0; j < P; ++j) r.d[j] = -a.d[j];
    return r;
}
template <class V, int P> DDP_AD_FN ddp_dual<V, P> operator+(const ddp_dual<V, P> &a, const ddp_dual<V, P> &b) { ddp_dual<V, P> r = a; return r += b; }
template <class V, int P> DDP_AD_FN ddp_dual<V, P> operator-(const ddp_dual<V, P> &a, const ddp_dual<V, P> &b) { ddp_dual<V, P> r = a; return r -= b; }
template <class V, int P> DDP_AD_FN ddp_dual<V, P> operator+(const ddp_dual<V, P> &a, double b) { ddp_dual<V, P> r = a; r.v += b; return r; }
template <class V, int P> DDP_AD_FN ddp_dual<V, P> operator+(double a, const ddp_dual<V, P> &b) { ddp_dual<V, P> r = b; r.v = a + b.v; return r; }
template <class V, int P> DDP_AD_FN ddp_dual<V, P> operator-(const ddp_dual<V, P> &a, double b) { ddp_dual<V, P> r = a; r.v -= b; return r; }
template <class V, int P> DDP_AD_FN ddp_dual<V, P> operator-(double a, const ddp_dual<V, P> &b) { ddp_dual<V, P> r = -b; r.v = a - b.v; return r; }
template <class V, int P> DDP_AD_FN ddp_dual<V, P> operator*(const ddp_dual<V, P> &a, const ddp_dual<V, P> &b)
{
    ddp_dual<V, P> r;
    r.v = a.v * b.v;
#pragma unroll
    for (int j = 0; j < P; ++j) r.d[j] = a.d[j] * b.v + a.v * b.d[j];
    return r;
}
template <class V, int P> DDP_AD_FN ddp_dual<V, P> operator*(const ddp_dual<V, P> &a, double b)
{
    ddp_dual<V, P> r;
    r.v = a.v * b;
#pragma unroll
    for (int j = 0; j < P; ++j) r.d[j] = a.d[j] * b;
    return r;
}
template <class V, int P> DDP_AD_FN ddp_dual<V, P> operator*(double a, const ddp_dual<V, P> &b) { return b * a; }
template <class V, int P> DDP_AD_FN ddp_dual<V, P> operator/(const ddp_dual<V, P> &a, const ddp_dual<V, P> &b)
{
    ddp_dual<V, P> r;
    r.v = a.v / b.v;
    const V ib = 1.0 / b.v;
#pragma unroll
    for (int j = 0; j < P; ++j) r.d[j] = (a.d[j] - r.v * b.d[j]) * ib;
    return r;
}
template <class V, int P> DDP_AD_FN ddp_dual<V, P> operator/(const ddp_dual<V, P> &a, double b)
{
    ddp_dual<V, P> r;
    r.v = a.v / b;
    const double ib = 1.0 / b;
#pragma unroll
    for (int j = 0; j < P; ++j) r.d[j] = a.d[j] * ib;
    return r;
}
template <class V, int P> DDP_AD_FN ddp_dual<V, P> operator/(double a, const ddp_dual<V, P> &b)
{
    const V r = a / b.v;
    return ddp_chain(b, r, -r / b.v);
}

// ---- comparisons on the value
#define DDP_AD_CMP(OP)                                                                                                                \
    template <class V, int P> DDP_AD_FN bool operator OP(const ddp_dual<V, P> &a, const ddp_dual<V, P> &b) { return ddp_value(a) OP ddp_value(b); } \
    template <class V, int P> DDP_AD_FN bool operator OP(const ddp_dual<V, P> &a, double b) { return ddp_value(a) OP b; }                       \
    template <class V, int P> DDP_AD_FN bool operator OP(double a, const ddp_dual<V, P> &b) { return a OP ddp_value(b); }
DDP_AD_CMP(<)
DDP_AD_CMP(<=)
DDP_AD_CMP(>)
DDP_AD_CMP(>=)
DDP_AD_CMP(==)
DDP_AD_CMP(!=)
#undef DDP_AD_CMP

// ---- functions (found by ADL; on V they call themselves, so they nest).  Anything not listed here does not compile for a dual.
template <class V, int P> DDP_AD_FN ddp_dual<V, P> sin(const ddp_dual<V, P> &a) { return ddp_chain(a, V(sin(a.v)), V(cos(a.v))); }
template <class V, int P> DDP_AD_FN ddp_dual<V, P> cos(const ddp_dual<V, P> &a) { return ddp_chain(a, V(cos(a.v)), V(-sin(a.v))); }
template <class V, int P> DDP_AD_FN ddp_dual<V, P> tan(const ddp_dual<V, P> &a)
{
    const V t = tan(a.v);
    return ddp_chain(a, t, V(1.0 + t * t));
}
template <class V, int P> DDP_AD_FN ddp_dual<V, P> exp(const ddp_dual<V, P> &a)
{
    const V e = exp(a.v);
    return ddp_chain(a, e, e);
}
template <class V, int P> DDP_AD_FN ddp_dual<V, P> expm1(const ddp_dual<V, P> &a) { return ddp_chain(a, V(expm1(a.v)), V(exp(a.v))); }
template <class V, int P> DDP_AD_FN ddp_dual<V, P> log(const ddp_dual<V, P> &a) { return ddp_chain(a, V(log(a.v)), V(1.0 / a.v)); }
template <class V, int P> DDP_AD_FN ddp_dual<V, P> log1p(const ddp_dual<V, P> &a) { return ddp_chain(a, V(log1p(a.v)), V(1.0 / (1.0 + a.v))); }
template <class V, int P> DDP_AD_FN ddp_dual<V, P> sqrt(const ddp_dual<V, P> &a)
{
    const V s = sqrt(a.v);
    return ddp_chain(a, s, V(0.5 / s));
}
template <class V, int P> DDP_AD_FN ddp_dual<V, P> tanh(const ddp_dual<V, P> &a)
{
    const V t = tanh(a.v);
    return ddp_chain(a, t, V(1.0 - t * t));
}
template <class V, int P> DDP_AD_FN ddp_dual<V, P> sinh(const ddp_dual<V, P> &a) { return ddp_chain(a, V(sinh(a.v)), V(cosh(a.v))); }
template <class V, int P> DDP_AD_FN ddp_dual<V, P> cosh(const ddp_dual<V, P> &a) { return ddp_chain(a, V(cosh(a.v)), V(sinh(a.v))); }
template <class V, int P> DDP_AD_FN ddp_dual<V, P> atan(const ddp_dual<V, P> &a) { return ddp_chain(a, V(atan(a.v)), V(1.0 / (1.0 + a.v * a.v))); }
template <class V, int P> DDP_AD_FN ddp_dual<V, P> asin(const ddp_dual<V, P> &a) { return ddp_chain(a, V(asin(a.v)), V(1.0 / sqrt(1.0 - a.v * a.v))); }
template <class V, int P> DDP_AD_FN ddp_dual<V, P> acos(const ddp_dual<V, P> &a) { return ddp_chain(a, V(acos(a.v)), V(-1.0 / sqrt(1.0 - a.v * a.v))); }
template <class V, int P> DDP_AD_FN ddp_dual<V, P> fabs(const ddp_dual<V, P> &a) { return ddp_value(a) < 0.0 ? -a : a; }
template <class V, int P> DDP_AD_FN ddp_dual<V, P> rint(const ddp_dual<V, P> &a) { return ddp_dual<V, P>(ddp_value(rint(a.v))); }
template <class V, int P> DDP_AD_FN ddp_dual<V, P> floor(const ddp_dual<V, P> &a) { return ddp_dual<V, P>(ddp_value(floor(a.v))); }
// a^b: b = 0 has the derivative 0 everywhere (a^(b-1) is infinite at a = 0)
template <class V, int P> DDP_AD_FN ddp_dual<V, P> pow(const ddp_dual<V, P> &a, double b)
{
    if (b == 0.0) return ddp_dual<V, P>(1.0);
    return ddp_chain(a, V(pow(a.v, b)), V(b * pow(a.v, b - 1.0)));
}
template <class V, int P> DDP_AD_FN ddp_dual<V, P> pow(const ddp_dual<V, P> &a, int b) { return pow(a, (double)b); }
template <class V, int P> DDP_AD_FN ddp_dual<V, P> pow(double a, const ddp_dual<V, P> &b)
{
    const V r = pow(a, b.v);
    return ddp_chain(b, r, V(r * log(a)));
}
template <class V, int P> DDP_AD_FN ddp_dual<V, P> pow(const ddp_dual<V, P> &a, const ddp_dual<V, P> &b)
{
    ddp_dual<V, P> r;
    r.v = pow(a.v, b.v);
    const V da = b.v * pow(a.v, b.v - 1.0), db = ddp_value(a.v) > 0.0 ? V(r.v * log(a.v)) : V(0.0);
#pragma unroll
    for (int j = 0; j < P; ++j) r.d[j] = da * a.d[j] + db * b.d[j];
    return r;
}
template <class V, int P> DDP_AD_FN ddp_dual<V, P> atan2(const ddp_dual<V, P> &y, const ddp_dual<V, P> &x)
{
    ddp_dual<V, P> r;
    r.v = atan2(y.v, x.v);
    const V is = 1.0 / (x.v * x.v + y.v * y.v), dy = x.v * is, dx = -y.v * is;
#pragma unroll
    for (int j = 0; j < P; ++j) r.d[j] = dy * y.d[j] + dx * x.d[j];
    return r;
}
template <class V, int P> DDP_AD_FN ddp_dual<V, P> hypot(const ddp_dual<V, P> &a, const ddp_dual<V, P> &b)
{
    ddp_dual<V, P> r;
    r.v = hypot(a.v, b.v);
    const V ir = 1.0 / r.v, da = a.v * ir, db = b.v * ir;
#pragma unroll
    for (int j = 0; j < P; ++j) r.d[j] = da * a.d[j] + db * b.d[j];
    return r;
}
template <class V, int P> DDP_AD_FN ddp_dual<V, P> fmin(const ddp_dual<V, P> &a, const ddp_dual<V, P> &b) { return b < a ? b : a; }
template <class V, int P> DDP_AD_FN ddp_dual<V, P> fmax(const ddp_dual<V, P> &a, const ddp_dual<V, P> &b) { return a < b ? b : a; }
#define DDP_AD_MIXED(F)                                                                                                               \
    template <class V, int P> DDP_AD_FN ddp_dual<V, P> F(const ddp_dual<V, P> &a, double b) { return F(a, ddp_dual<V, P>(b)); }     \
    template <class V, int P> DDP_AD_FN ddp_dual<V, P> F(double a, const ddp_dual<V, P> &b) { return F(ddp_dual<V, P>(a), b); }
DDP_AD_MIXED(atan2)
DDP_AD_MIXED(hypot)
DDP_AD_MIXED(fmin)
DDP_AD_MIXED(fmax)
#undef DDP_AD_MIXED
)DDPA";

static const char *kUserAutodiffDerivs = R"DDPA(
// the user's `derivatives`, derived from the templated dynamics / stage_cost / terminal_cost (same arguments, same outputs)
struct ddp_ad_out { double *fx, *fu, *cx, *cu, *cxx, *cxu, *cuu; };

// z = [x; u] as duals seeded in directions z0 .. z0 + P - 1 (partials past n + m stay zero)
template <int Z0, class D> DDP_AD_FN void ddp_ad_seed1(const double *x, const double *u, D *xd, D *ud)
{
    constexpr int n = DDP_N, m = DDP_M;
#pragma unroll
    for (int k = 0; k < n + m; ++k) {
        D &z = k < n ? xd[k] : ud[k - n];
        z = D(k < n ? x[k] : u[k - n]);
        if (k >= Z0 && k < Z0 + DDP_ADJ) z.d[k - Z0] = 1.0;
    }
}

// the first derivatives in directions C·DDP_ADJ .. : fx / fu columns; under DDP_CONST_HESSIAN also cx / cu
template <int C> DDP_AD_FN void ddp_ad_jacobian(const double *x, const double *u, int i, int N, const double *p, const ddp_ad_out &o)
{
    constexpr int n = DDP_N, m = DDP_M, Z0 = C * DDP_ADJ;
    if constexpr (Z0 < n + m) {
        typedef ddp_dual<double, DDP_ADJ> D;
        D xd[n], ud[m], xn[n];
        ddp_ad_seed1<Z0>(x, u, xd, ud);
        DDP_AD_FRESH(p);
        dynamics(xd, ud, i, p, xn);
#if DDP_CONST_HESSIAN
        D c = stage_cost(xd, ud, i, p);
#if DDP_TERMINAL
        if (Z0 < n && i == N - 1) c += terminal_cost(xd, p);
#endif
#endif
#pragma unroll
        for (int j = 0; j < DDP_ADJ; ++j) {
            const int z = Z0 + j;
            if (z >= n + m) break;
#pragma unroll
            for (int r = 0; r < n; ++r) {
                if (z < n) o.fx[r + n * z] = xn[r].d[j];
                else o.fu[r + n * (z - n)] = xn[r].d[j];
            }
#if DDP_CONST_HESSIAN
            if (z < n) o.cx[z] = c.d[j];
            else o.cu[z - n] = c.d[j];
#endif
        }
        ddp_ad_jacobian<C + 1>(x, u, i, N, p, o);
    }
}

#if !DDP_CONST_HESSIAN
// the Hessian block of the directions (BI, BJ), BI <= BJ: a dual over a dual, the inner seeded in block BI, the outer in block BJ.
// Only a <= b is stored, into both (a, b) and (b, a): the blocks are exactly symmetric.  The diagonal blocks also give cx / cu.
template <int BI, int BJ> DDP_AD_FN void ddp_ad_hessian_block(const double *x, const double *u, int i, int N, const double *p,
                                                               const ddp_ad_out &o)
{
    constexpr int n = DDP_N, m = DDP_M, H = DDP_ADH, A0 = BI * H, B0 = BJ * H;
    typedef ddp_dual<double, H> D1;
    typedef ddp_dual<D1, H> D2;
    D2 xd[n], ud[m];
#pragma unroll
    for (int k = 0; k < n + m; ++k) {
        D2 &z = k < n ? xd[k] : ud[k - n];
        z = D2(k < n ? x[k] : u[k - n]);
        if (k >= A0 && k < A0 + H) z.v.d[k - A0] = 1.0;
        if (k >= B0 && k < B0 + H) z.d[k - B0].v = 1.0;
    }
    DDP_AD_FRESH(p);
    D2 c = stage_cost(xd, ud, i, p);
#if DDP_TERMINAL
    if (B0 < n && i == N - 1) c += terminal_cost(xd, p);      // the terminal cost acts on x[:,N-1] (the header's convention)
#endif
#pragma unroll
    for (int ja = 0; ja < H; ++ja) {
        const int a = A0 + ja;
        if (a >= n + m) break;
        if (BI == BJ) {
            if (a < n) o.cx[a] = c.v.d[ja];
            else o.cu[a - n] = c.v.d[ja];
        }
#pragma unroll
        for (int jb = 0; jb < H; ++jb) {
            const int b = B0 + jb;
            if (b >= n + m) break;
            if (b < a) continue;
            const double v = c.d[jb].d[ja];
            if (b < n) { o.cxx[a + n * b] = v; o.cxx[b + n * a] = v; }
            else if (a < n) o.cxu[a + n * (b - n)] = v;
            else { o.cuu[(a - n) + m * (b - n)] = v; o.cuu[(b - n) + m * (a - n)] = v; }
        }
    }
}

template <int BI, int BJ> DDP_AD_FN void ddp_ad_hessian(const double *x, const double *u, int i, int N, const double *p, const ddp_ad_out &o)
{
    constexpr int NB = (DDP_N + DDP_M + DDP_ADH - 1) / DDP_ADH;
    if constexpr (BI < NB) {
        if constexpr (BJ < NB) {
            ddp_ad_hessian_block<BI, BJ>(x, u, i, N, p, o);
            ddp_ad_hessian<BI, BJ + 1>(x, u, i, N, p, o);
        } else {
            ddp_ad_hessian<BI + 1, BI + 1>(x, u, i, N, p, o);
        }
    }
}
#endif

DDP_AD_FN void ddp_ad_derivatives(const double *x, const double *u, int i, int N, const double *p, double *fx, double *fu, double *cx,
                                  double *cu, double *cxx, double *cxu, double *cuu)
{
    const ddp_ad_out o = {fx, fu, cx, cu, cxx, cxu, cuu};
    ddp_ad_jacobian<0>(x, u, i, N, p, o);
#if !DDP_CONST_HESSIAN
    ddp_ad_hessian<0, 0>(x, u, i, N, p, o);
#endif
}
)DDPA";

// DDP_USER_SECOND_ORDER only (a program without the flag does not contain it)
static const char *kUserAutodiffVhess = R"DDPA(
// Σ_k v[k] · ∂²f_k/∂z_a∂z_b at (x, u, i), z = [x; u]: the (a, b) entry of the Hessian of the scalar v·f(z), from ONE call of `dynamics`
// on a dual over a dual with one partial each, the inner number seeded in direction min(a, b), the outer in max(a, b) (so the value
// does not depend on the order of a and b).  a and b are run-time values: the seeds come from compares in the unrolled loop over z, no
// array is indexed by them, and every lane of a wave may ask for its own pair while all of them run the same code
// (ddp_user_back_pass2, ddp_user_vhess), which the template recursion over blocks above cannot offer.
DDP_AD_FN double ddp_ad_vhess(const double *x, const double *u, int i, const double *p, const double *v, int a, int b)
{
    constexpr int n = DDP_N, m = DDP_M;
    typedef ddp_dual<ddp_dual<double, 1>, 1> D2;
    const int lo = a < b ? a : b, hi = a < b ? b : a;
    D2 xd[n], ud[m], xn[n];
#pragma unroll
    for (int k = 0; k < n + m; ++k) {
        D2 &z = k < n ? xd[k] : ud[k - n];
        z = D2(k < n ? x[k] : u[k - n]);
        z.v.d[0] = k == lo ? 1.0 : 0.0;
        z.d[0].v = k == hi ? 1.0 : 0.0;
    }
    DDP_AD_FRESH(p);
    dynamics(xd, ud, i, p, xn);
    double s = 0.0;
#pragma unroll
    for (int r = 0; r < n; ++r) s += v[r] * xn[r].d[0].d[0];
    return s;
}
)DDPA";
