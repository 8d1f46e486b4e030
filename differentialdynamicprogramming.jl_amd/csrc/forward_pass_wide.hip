// forward_pass_wide.hip — closed-loop rollout of the LQ family for WIDE CONTROLS: 8 < m <= 32 with any n <= 64
// (src/forward_pass.jl:9-33, f / costfun of src/demo_linear.jl:42-49).  The scheme of forward_big_kernel (forward_pass_big.hip)
// extended in the control axis: one wavefront per (trajectory, α) rollout, lane j holds x̂_j; per step x̂ and diff(x̂, x) go through
// the LDS once, lanes q < m form the controls (row q of K_i streamed from global memory, coalesced across the lanes for every
// column), then lane j forms row j of A x̂ + B u.  Sums run with eight requests in flight.  diff_wrap (n <= 32) wraps the named
// coordinates of diff(x̂, x) as the run-time-sized kernel of forward_pass.hip does.  The per-step cost is evaluated afterwards by a
// kernel with its lanes over time, and its sum per rollout by the same kernel.
#include "ddp_internal.h"

namespace {

struct FWArgs {
    int n, m, N, B, nalpha;
    int dyn_tv, dyn_batched, has_policy, has_lims;
    unsigned wrap;
    const double *A, *Bm, *Q, *R, *K, *k, *x0, *u, *x, *lims;
    const int32_t *active;
    double alpha[16];
    double *xnew, *unew, *cnew, *csum;
};

__device__ __forceinline__ double clampw(double x, double lo, double hi) { return x > hi ? hi : (x < lo ? lo : x); }

// d - 2π·rint(d / 2π) with 2π in two parts (forward_pass.hip, wrap_pi)
__device__ __forceinline__ double wrap_pi_w(double d)
{
    const double q = rint(d * 0x1.45f306dc9c883p-3);
    return fma(-q, 0x1.1a62633145c07p-52, fma(-q, 0x1.921fb54442d18p+2, d));
}

// Σ_l w[l·stride]·v[l], l < len, eight requests in flight per round trip; the partial sums meet pairwise
__device__ __forceinline__ double dot8w(const double *w, size_t stride, const double *v, int len)
{
    double acc[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    int l = 0;
    for (; l + 8 <= len; l += 8) {
        double wv[8];
#pragma unroll
        for (int q = 0; q < 8; ++q) wv[q] = w[stride * (l + q)];
#pragma unroll
        for (int q = 0; q < 8; ++q) acc[q] += wv[q] * v[l + q];
    }
    for (; l < len; ++l) acc[l & 7] += w[stride * l] * v[l];
    return ((acc[0] + acc[1]) + (acc[2] + acc[3])) + ((acc[4] + acc[5]) + (acc[6] + acc[7]));
}

__global__ __launch_bounds__(DDP_WAVE) void forward_wide_kernel(FWArgs a)
{
    const int n = a.n, m = a.m, N = a.N, B = a.B;
    const long rho = blockIdx.x;
    const int b = (int)(rho % B), ai = (int)(rho / B);
    if (a.active && a.active[b] == 0) return;
    const int j = threadIdx.x;
    const bool inx = j < n, inu = j < m;
    const int jx = inx ? j : 0, ju = inu ? j : 0;
    const double alpha = a.alpha[ai];
    __shared__ double xs[DDP_WAVE], dxs[DDP_WAVE], us[DDP_MAX_M_WIDE];
    const size_t nn = (size_t)n * n, nm = (size_t)n * m;
    const double *ug = a.u + (size_t)m * N * b;
    const double *xg = a.has_policy ? a.x + (size_t)n * N * b : nullptr;
    const double *Kg = a.has_policy ? a.K + nm * N * b : nullptr;
    const double *kg = a.has_policy ? a.k + (size_t)m * N * b : nullptr;
    double *xo = a.xnew + (size_t)n * N * ((size_t)b + (size_t)B * ai);
    double *uo = a.unew + (size_t)m * N * ((size_t)b + (size_t)B * ai);
    const double *Ab = a.A + (a.dyn_batched ? nn * (a.dyn_tv ? N : 1) * b : 0);
    const double *Bb = a.Bm + (a.dyn_batched ? nm * (a.dyn_tv ? N : 1) * b : 0);
    const double lo = (a.has_lims && inu) ? a.lims[ju] : 0.0, hi = (a.has_lims && inu) ? a.lims[ju + m] : 0.0;
    const bool wrapj = inx && j < 32 && ((a.wrap >> j) & 1u);

    double xh = inx ? a.x0[(size_t)n * b + jx] : 0.0;
    for (int i = 0; i < N; ++i) {
        xs[j] = xh;
        double dx = a.has_policy ? xh - (inx ? xg[(size_t)n * i + jx] : 0.0) : 0.0;
        if (wrapj) dx = wrap_pi_w(dx);                              // diff_fun with wrapped coordinates
        dxs[j] = dx;
        wave_sync();
        const double *Ai = Ab + (a.dyn_tv ? nn * i : 0), *Bi = Bb + (a.dyn_tv ? nm * i : 0);
        double ax = 0.0;
        if (i < N - 1) ax = dot8w(Ai + jx, (size_t)n, xs, n);       // (A x̂)_j does not wait for the controls
        if (inu) {                                                  // controls (forward_pass.jl:17-24)
            double v = ug[(size_t)m * i + ju];
            if (a.has_policy) {
                v += kg[(size_t)m * i + ju] * alpha;                // unew .+= k*α
                v += dot8w(Kg + nm * i + ju, (size_t)m, dxs, n);    // unew .+= K*dx
            }
            if (a.has_lims) v = clampw(v, lo, hi);
            if (v != v) v = 0.0;                                    // u[isnan.(u)] .= 0 inside f
            us[ju] = v;
            uo[(size_t)m * i + ju] = v;
        }
        if (inx) xo[(size_t)n * i + jx] = xh;
        wave_sync();
        if (i < N - 1) {                                            // x+ = A x + B u (src/demo_linear.jl:42-46)
            const double t = dot8w(Bi + jx, (size_t)n, us, m);
            xh = inx ? ax + t : 0.0;
        }
        wave_sync();
    }
}

// cost per step and its sum per rollout: one wave per rollout, lanes over time (demo_linear.jl:49 split per step); Q, R in the LDS
__global__ __launch_bounds__(DDP_WAVE) void cost_wide_kernel(FWArgs a)
{
    const int n = a.n, m = a.m, N = a.N, B = a.B;
    const long rho = blockIdx.x;
    const int b = (int)(rho % B);
    if (a.active && a.active[b] == 0) return;
    const int lane = threadIdx.x;
    const double *x = a.xnew + (size_t)n * N * rho, *u = a.unew + (size_t)m * N * rho;
    double *c = a.cnew + (size_t)N * rho;
    extern __shared__ double qr[];
    for (int e = lane; e < n * n; e += DDP_WAVE) qr[e] = a.Q[e];
    for (int e = lane; e < m * m; e += DDP_WAVE) qr[n * n + e] = a.R[e];
    wave_sync();
    const double *Q = qr, *R = qr + n * n;
    double acc = 0.0;
    for (int t = lane; t < N; t += DDP_WAVE) {
        const double *xt = x + (size_t)n * t, *ut = u + (size_t)m * t;
        double qx = 0.0, ru = 0.0;
        for (int i = 0; i < n; ++i) {
            double s = 0.0;
            for (int jj = 0; jj < n; ++jj) s += Q[i + n * jj] * xt[jj];
            qx += xt[i] * s;
        }
        for (int i = 0; i < m; ++i) {
            double s = 0.0;
            for (int jj = 0; jj < m; ++jj) s += R[i + m * jj] * ut[jj];
            ru += ut[i] * s;
        }
        const double ct = 0.5 * qx + 0.5 * ru;
        c[t] = ct;
        acc += ct;
    }
    for (int off = 32; off >= 1; off >>= 1) acc += __shfl_xor(acc, off, 64);
    if (lane == 0) a.csum[rho] = acc;
}

}   // namespace

// LQ family, n <= 64, m <= DDP_MAX_M_WIDE
int ddp_launch_forward_wide(ddp_handle h, const FPCall &c)
{
    const ddp_problem *p = c.p;
    DDP_CHECK(p->kind == DDP_PROBLEM_LQ && p->n >= 1 && p->n <= 64 && p->m >= 1 && p->m <= DDP_MAX_M_WIDE,
              "forward_pass: n=%d m=%d outside the wide-control rollout (LQ family, n <= 64, m <= %d)", p->n, p->m, DDP_MAX_M_WIDE);
    FWArgs a;
    fp_fill(a, c);
    a.n = p->n; a.m = p->m;
    a.dyn_tv = p->dyn_tv; a.dyn_batched = p->dyn_batched; a.has_policy = c.K != nullptr; a.has_lims = c.lims != nullptr;
    a.wrap = p->diff_wrap;
    a.lims = c.lims;
    const dim3 grid((unsigned)((long)p->B * c.nalpha)), block(DDP_WAVE);
    hipLaunchKernelGGL(forward_wide_kernel, grid, block, 0, h->stream, a);
    const size_t shmem = ((size_t)p->n * p->n + (size_t)p->m * p->m) * sizeof(double);      // <= 40 KB
    hipLaunchKernelGGL(cost_wide_kernel, grid, block, shmem, h->stream, a);
    DDP_HIP(hipGetLastError());
    return 0;
}
