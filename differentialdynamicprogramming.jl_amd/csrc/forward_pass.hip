// forward_pass.hip — batched closed-loop rollout / line-search candidates for gfx950.
//
// Replaces  forward_pass(traj_new,x0,u,x,α,f,costfun,lims,diff)  (src/forward_pass.jl:9-33) for the
// registered problem families (the Julia closures f / costfun cannot run on the device):
//   LQ        f: src/demo_linear.jl:42-46,  costfun: src/demo_linear.jl:49
//   pendcart  f: src/system_pendcart.jl:83-89, costfun: src/system_pendcart.jl:97-106
// All nalpha step sizes of the serial backtracking search (src/iLQG.jl:267-281) are rolled out
// concurrently; the caller picks the FIRST α (list order) that passes the acceptance test, which is
// what the serial loop returns.
//
// Mapping: a group of G lanes (G = 4/16/32/64 >= n) owns one (trajectory, α) rollout, 64/G rollouts
// per wavefront.  Lane j of a group holds x̂_j; per time step the state is exchanged through LDS once
// (one wave-level hand-off), every lane forms the m controls redundantly (so no second exchange is
// needed), then lane j forms row j of the dynamics.  The step-(i+1) operands K,k,x,u are fetched while
// step i computes.  The time loop is a strict dependency chain: throughput comes from the
// (trajectory, α) batch, not from the horizon.
#include <vector>
#include "ddp_internal.h"

namespace {

struct FPArgs {
    int n, m, N, B, nalpha;
    int dyn_tv, dyn_batched, has_policy, has_lims;
    unsigned wrap;                                  // ddp_problem::diff_wrap
    const double *A, *Bm, *Q, *R, *K, *k, *x0, *u, *x, *lims;
    const int32_t *active;
    double alpha[16];
    double g, l, h, d, goal[4];
    double *xnew, *unew, *cnew, *csum;
};

// diff_fun for an angle coordinate (ddp_amd.h, ddp_problem::diff_wrap): d - 2π·rint(d / 2π) with 2π in two parts, so that the result is
// within an ulp of rem2pi(d, RoundNearest) for every difference a rollout can produce
__device__ __forceinline__ double wrap_pi(double d)
{
    const double q = rint(d * 0x1.45f306dc9c883p-3);                       // 1 / 2π
    return fma(-q, 0x1.1a62633145c07p-52, fma(-q, 0x1.921fb54442d18p+2, d));   // 2π = 0x1.921fb54442d18p+2 + 0x1.1a62633145c07p-52
}

__device__ __forceinline__ double clampd(double x, double lo, double hi) { return x > hi ? hi : (x < lo ? lo : x); }

template <int G>
__device__ __forceinline__ double group_sum(double v)
{
#pragma unroll
    for (int off = G / 2; off >= 1; off >>= 1) v += __shfl_xor(v, off, G);
    return v;
}

template <int KIND, int NS, int MS, int G>
__global__ __launch_bounds__(DDP_WAVE) void forward_pass_kernel(FPArgs a)
{
    constexpr int NMAX = NS ? NS : G;
    constexpr int MM = MS ? MS : DDP_MAX_M;
    constexpr bool PF = NS != 0;          // register prefetch of K_i, x_i only for compiled sizes
    constexpr int KP = PF ? MM * NMAX : 1, XP = PF ? NMAX : 1;
    constexpr int GPW = DDP_WAVE / G;                         // rollouts per wavefront
    const int n = NS ? NS : a.n, m = MS ? MS : a.m, N = a.N, B = a.B;
    const int lane = threadIdx.x, grp = lane / G, jl = lane % G;
    const long total = (long)B * a.nalpha;
    long rho = (long)blockIdx.x * GPW + grp;
    const bool valid = rho < total;
    if (!valid) rho = total - 1;                              // keep the wave converged; stores are masked
    const int b = (int)(rho % B), ai = (int)(rho / B);
    const bool act = valid && !(a.active && a.active[b] == 0);
    const double alpha = a.alpha[ai];
    const int CL = (KIND == DDP_PROBLEM_PENDCART) ? N + 1 : N;

    __shared__ double xs[GPW][G];

    const size_t nn = (size_t)n * n, nm = (size_t)n * m;
    const double *ug = a.u + (size_t)m * N * b;
    const double *xg = a.has_policy ? a.x + (size_t)n * N * b : nullptr;
    const double *Kg = a.has_policy ? a.K + nm * N * b : nullptr;
    const double *kg = a.has_policy ? a.k + (size_t)m * N * b : nullptr;
    double *xo = a.xnew + (size_t)n * N * ((size_t)b + (size_t)B * ai);
    double *uo = a.unew + (size_t)m * N * ((size_t)b + (size_t)B * ai);
    double *co = a.cnew + (size_t)CL * ((size_t)b + (size_t)B * ai);

    // loop-invariant rows (LTI): row jl of A, B, Q
    double Arow[NMAX], Brow[MM], Qrow[NMAX], Rm[MM * MM], lo[MM], hi[MM];
    const double *Ab = nullptr, *Bb = nullptr;
    if (KIND == DDP_PROBLEM_LQ) {
        Ab = a.A + (a.dyn_batched ? nn * (a.dyn_tv ? N : 1) * b : 0);
        Bb = a.Bm + (a.dyn_batched ? nm * (a.dyn_tv ? N : 1) * b : 0);
    }
#pragma unroll
    for (int l = 0; l < NMAX; ++l) {
        const bool in = (jl < n && l < n);
        Arow[l] = (KIND == DDP_PROBLEM_LQ && !a.dyn_tv && in) ? Ab[jl + n * l] : 0.0;
        Qrow[l] = in ? a.Q[jl + n * l] : 0.0;
    }
#pragma unroll
    for (int q = 0; q < MM; ++q) {
        Brow[q] = (KIND == DDP_PROBLEM_LQ && !a.dyn_tv && jl < n && q < m) ? Bb[jl + n * q] : 0.0;
        lo[q] = (a.has_lims && q < m) ? a.lims[q] : 0.0;
        hi[q] = (a.has_lims && q < m) ? a.lims[q + m] : 0.0;
#pragma unroll
        for (int q2 = 0; q2 < MM; ++q2) Rm[q + MM * q2] = (q < m && q2 < m) ? a.R[q + m * q2] : 0.0;
    }

    double xh = (jl < n) ? a.x0[(size_t)n * b + jl] : 0.0;
    double csum = 0.0;

    // operands of step i, fetched one step ahead
    double uc[MM], kc[MM], Kc[KP], xc[XP];
    auto fetch = [&](int i) {
#pragma unroll
        for (int q = 0; q < MM; ++q) {
            uc[q] = (q < m) ? ug[(size_t)m * i + q] : 0.0;
            kc[q] = (a.has_policy && q < m) ? kg[(size_t)m * i + q] : 0.0;
        }
        if (PF && a.has_policy) {
#pragma unroll
            for (int l = 0; l < NMAX; ++l) {
                xc[l] = (l < n) ? xg[(size_t)n * i + l] : 0.0;
#pragma unroll
                for (int q = 0; q < MM; ++q) Kc[q + MM * l] = (q < m && l < n) ? Kg[nm * i + q + m * l] : 0.0;
            }
        }
        if (KIND == DDP_PROBLEM_LQ && a.dyn_tv) {
#pragma unroll
            for (int l = 0; l < NMAX; ++l) Arow[l] = (jl < n && l < n) ? Ab[nn * i + jl + n * l] : 0.0;
#pragma unroll
            for (int q = 0; q < MM; ++q) Brow[q] = (jl < n && q < m) ? Bb[nm * i + jl + n * q] : 0.0;
        }
    };

    double un[MM], kn[MM], Kn[KP], xn_[XP], An[NMAX], Bn[MM];
    fetch(0);
    for (int i = 0; i < N; ++i) {
        // stash step i's operands, start fetching step i+1 (lands during the dependent chain below)
#pragma unroll
        for (int q = 0; q < MM; ++q) { un[q] = uc[q]; kn[q] = kc[q]; Bn[q] = Brow[q]; }
#pragma unroll
        for (int l = 0; l < NMAX; ++l) {
            An[l] = Arow[l];
            if (PF) {
                xn_[l] = xc[l];
#pragma unroll
                for (int q = 0; q < MM; ++q) Kn[q + MM * l] = Kc[q + MM * l];
            }
        }
        if (i + 1 < N) fetch(i + 1);

        xs[grp][jl] = xh;
        wave_sync();
        double xv[NMAX];
#pragma unroll
        for (int l = 0; l < NMAX; ++l) xv[l] = (l < n) ? xs[grp][l] : 0.0;

        // ---- controls (forward_pass.jl:17-24), every lane of the group redundantly
        double uu[MM];
#pragma unroll
        for (int q = 0; q < MM; ++q) {
            double v = un[q];
            if (a.has_policy) {
                v += kn[q] * alpha;                                  // unew .+= k*α
                double s = 0.0;
                if (a.wrap == 0) {                                   // diff_fun = `-` (wave-uniform: the default pays nothing for the hook)
#pragma unroll
                    for (int l = 0; l < NMAX; ++l) {
                        if (PF) s += Kn[q + MM * l] * (xv[l] - xn_[l]);
                        else if (l < n && q < m) s += Kg[nm * i + q + m * l] * (xv[l] - xg[(size_t)n * i + l]);
                    }
                } else {
#pragma unroll
                    for (int l = 0; l < NMAX; ++l) {
                        if (!(PF || (l < n && q < m))) continue;
                        double dxl = PF ? xv[l] - xn_[l] : xv[l] - xg[(size_t)n * i + l];
                        if ((a.wrap >> l) & 1u) dxl = wrap_pi(dxl);
                        s += (PF ? Kn[q + MM * l] : Kg[nm * i + q + m * l]) * dxl;
                    }
                }
                v += s;                                              // unew .+= K*dx
            }
            if (a.has_lims) v = clampd(v, lo[q], hi[q]);
            if (v != v) v = 0.0;                                     // u[isnan.(u)] .= 0 inside f
            uu[q] = (q < m) ? v : 0.0;
        }
        // ---- dynamics row jl and this lane's share of the cost
        double xnext = 0.0, cpart = 0.0;
        if (KIND == DDP_PROBLEM_LQ) {
            double s = 0.0, t = 0.0, qx = 0.0;
#pragma unroll
            for (int l = 0; l < NMAX; ++l) { s += An[l] * xv[l]; qx += Qrow[l] * xv[l]; }
#pragma unroll
            for (int q = 0; q < MM; ++q) t += Bn[q] * uu[q];
            xnext = s + t;                                           // A*x + B*u
            cpart = 0.5 * xh * qx;                                   // .5 x.*(Q*x), row jl
            if (jl == 0) {
                double ru = 0.0;
#pragma unroll
                for (int q = 0; q < MM; ++q) {
                    double r = 0.0;
#pragma unroll
                    for (int q2 = 0; q2 < MM; ++q2) r += Rm[q + MM * q2] * uu[q2];
                    ru += uu[q] * r;
                }
                cpart += 0.5 * ru;
            }
        } else {
            const double gl = a.g / a.l, h = a.h;
            if (jl == 0) xnext = xv[0] + h * xv[1];
            else if (jl == 1) xnext = xv[1] + h * (-gl * sin(xv[0]) + uu[0] / a.l * cos(xv[0]) - a.d * xv[1]);
            else if (jl == 2) xnext = xv[2] + h * xv[3];
            else xnext = xv[3] + h * uu[0];
            double qd = 0.0;
#pragma unroll
            for (int l = 0; l < NMAX; ++l) qd += Qrow[l] * (xv[l] - a.goal[l < 4 ? l : 0]);
            cpart = 0.5 * (xh - a.goal[jl < 4 ? jl : 0]) * qd;
            if (jl == 0) cpart += 0.5 * uu[0] * Rm[0] * uu[0];
        }
        const double ci = group_sum<G>(cpart);
        if (act) {
            if (jl < n) xo[(size_t)n * i + jl] = xh;
            if (jl < m) {
                double v = uu[0];
#pragma unroll
                for (int q = 1; q < MM; ++q) v = (jl == q) ? uu[q] : v;
                uo[(size_t)m * i + jl] = v;
            }
            if (jl == 0) co[i] = ci;
        }
        csum += ci;
        if (KIND == DDP_PROBLEM_PENDCART && i == N - 1) {            // c[end] re-counts x[:,N] with u = 0
            const double cend = group_sum<G>(cpart - ((jl == 0) ? 0.5 * uu[0] * Rm[0] * uu[0] : 0.0));
            if (act && jl == 0) co[N] = cend;
            csum += cend;
        }
        if (i < N - 1) xh = xnext;                                   // f is also called at i == N, result discarded
    }
    if (act && jl == 0) a.csum[(size_t)b + (size_t)B * ai] = csum;
}

template <int KIND, int NS, int MS, int G>
int launch_fp(ddp_handle h, const FPArgs &a)
{
    const long total = (long)a.B * a.nalpha;
    const int gpw = DDP_WAVE / G;
    const dim3 grid((unsigned)((total + gpw - 1) / gpw)), block(DDP_WAVE);
    hipLaunchKernelGGL((forward_pass_kernel<KIND, NS, MS, G>), grid, block, 0, h->stream, a);
    DDP_HIP(hipGetLastError());
    return 0;
}

}   // namespace

int ddp_cost_len(const ddp_problem *p) { return p->kind == DDP_PROBLEM_PENDCART ? p->N + 1 : p->N; }

int ddp_check_cost_diag_host(const ddp_problem *p)
{
    if (!p->cost_diag || !p->Q || !p->R) return 0;
    const int n = p->n, m = p->m;
    int ok = 1;
    for (int j = 0; j < n; ++j) for (int i = 0; i < n; ++i) if (i != j && p->Q[i + (size_t)n * j] != 0.0) ok = 0;
    for (int j = 0; j < m; ++j) for (int i = 0; i < m; ++i) if (i != j && p->R[i + (size_t)m * j] != 0.0) ok = 0;
    DDP_CHECK(ok, "ddp_problem.cost_diag = 1 but Q or R has a non-zero off-diagonal entry (the fused rollout cost would drop it); set cost_diag = 0");
    return 0;
}

int ddp_check_cost_diag(ddp_handle h, const ddp_problem *p)
{
    if (h->diag_skip > 0) return 0;
    for (const auto &e : h->diag_cache)
        if (e.Q == p->Q && e.R == p->R && e.n == p->n && e.m == p->m && e.Q) {
            DDP_CHECK(e.ok, "forward_pass: ddp_problem.cost_diag = 1 but Q or R has a non-zero off-diagonal entry (the fused rollout cost would drop it); set cost_diag = 0");
            return 0;
        }
    const int n = p->n, m = p->m;
    std::vector<double> q((size_t)n * n), r((size_t)m * m);
    DDP_HIP(hipMemcpyAsync(q.data(), p->Q, q.size() * 8, hipMemcpyDeviceToHost, h->stream));
    DDP_HIP(hipMemcpyAsync(r.data(), p->R, r.size() * 8, hipMemcpyDeviceToHost, h->stream));
    DDP_HIP(hipStreamSynchronize(h->stream));
    int ok = 1;
    for (int j = 0; j < n; ++j) for (int i = 0; i < n; ++i) if (i != j && q[i + (size_t)n * j] != 0.0) ok = 0;
    for (int j = 0; j < m; ++j) for (int i = 0; i < m; ++i) if (i != j && r[i + (size_t)m * j] != 0.0) ok = 0;
    // only a PASS is remembered (a refused pair is looked at again on the next call: the caller may have repaired Q in place); the
    // entry dies with ddp_free of the allocation it points into and with ddp_reload_env
    if (ok) { auto &e = h->diag_cache[h->diag_next++ % 8]; e.Q = p->Q; e.R = p->R; e.n = n; e.m = m; e.ok = 1; }
    DDP_CHECK(ok, "forward_pass: ddp_problem.cost_diag = 1 but Q or R has a non-zero off-diagonal entry (the fused rollout cost would drop it); set cost_diag = 0");
    return 0;
}

// ---- kernel choice
// Several implementations of the same rollout exist, one per enumerator of FPKernel; the name is what ddp_last_kernel(h, 1) reports:
//   wide       8 < m <= 32 with any n <= 64 (forward_pass_wide.hip, LQ family): one wave per rollout, no other kernel holds the shape;
//   big64      the exact (64, 8) shape (forward_pass_big.hip): up to 4 step sizes of a trajectory per wave, operands fetched once;
//   mid        LQ, n <= 32, m <= 8 that no 16-lane row holds (forward_pass_big.hip): one wave per rollout, the operands of a step
//              requested a step ahead;
//   big        LQ, 32 < n <= 64 (forward_pass_big.hip): one wave per rollout with run-time sizes, then cost_mid_kernel at the larger
//              paddings or the run-time-sized cost kernel;
//   pipe4,     LQ (10, 2) with a policy, no limits and diagonal costs up to 1 024 rollouts (forward_pass_pipe.hip): a producer/consumer
//   pipe,      pipeline of one work-group per 4 rollouts; pipe4 for shared time-invariant dynamics, pipe for per-trajectory ones,
//   pipe_tv    pipe_tv for time-varying ones (A_i, B_i through the same LDS image);
//   pend_lane, pendcart (forward_pass_dpp.hip): one lane per rollout from 12 288 rollouts on, below that the pendulum's own 16-lane-row
//   pend_row   kernel, element-wise or (from 3 584 rollouts) in 16-step chunks through LDS; both wrap x̂ - x for diff_wrap;
//   dpp        16 lanes per rollout, 4 rollouts per wave, compiled for LQ (10, 2) and pendcart (4, 1) (forward_pass_dpp.hip);
//   row        the same row kernel compiled for PADDED sizes (forward_pass_row.hip): every other LQ shape a 16-lane row holds;
//   group      a group of 4 / 8 / 16 / 32 lanes per rollout with run-time sizes (this file): DDP_FORWARD=group, wrapped differences
//              outside the pendulum's kernels, pendcart without them.
static const char *const fp_kernel_name[] = {"", "forward_wide_kernel", "forward_big_kernel", "forward_mid_kernel", "forward_big_kernel",
                                             "forward_pipe4_kernel", "forward_pipe_kernel", "forward_pipe_kernel", "forward_dpp_kernel",
                                             "forward_dpp_kernel", "forward_dpp_kernel", "forward_row_kernel", "forward_pass_kernel"};
static const char *const fp_kernel_label[] = {"none", "wide", "big64", "mid", "big", "pipe4", "pipe", "pipe_tv", "pend_lane", "pend_row",
                                              "dpp", "row", "group"};

enum { FP_AL_POLICY = 1, FP_AL_DYN = 2, FP_AL_ROW = 4 };      // 16-byte aligned: K, k, u, x | A, Bm | u, k, K

// What the choice depends on besides the problem and nalpha.  Host facts only: the choice itself reads no device memory and no handle.
struct FPChoiceIn {
    unsigned al16;                                        // FP_AL_* bits
    bool sink;                                            // the handle has its sink buffer
    bool has_policy, has_lims;
    // the handle's DDP_FORWARD, DDP_FORWARD_PIPE, _FUSE, _PEND, _LANE, DDP_FORWARD64, DDP_FORWARD_MID, _FAST, DDP_PEND_CHUNK (nullptr: unset)
    const char *forward, *pipe, *fuse, *pend, *lane, *forward64, *mid, *fast, *pend_chunk;
};

// The switches (A/B timing, tests of every code path) are looked at by their first letter.  DDP_FORWARD=group forces the group-of-lanes
// kernel for everything but wide controls and n > 32; DDP_FORWARD=b puts the large-state kernels first for LQ problems without wrapped
// differences.
static FPChoice fp_choose(const ddp_problem &p, int nalpha, const FPChoiceIn &q)
{
    auto is = [](const char *s, char c) { return s && s[0] == c; };
    const int n = p.n, m = p.m;
    const long total = (long)p.B * nalpha;
    const bool lq = p.kind == DDP_PROBLEM_LQ, pendcart = p.kind == DDP_PROBLEM_PENDCART;
    FPChoice c = {FP_NONE, false, false, false, false, false, 1};
    auto pick = [&c](FPKernel k) { c.k = k; return c; };
    // one wave per rollout (forward_pass_big.hip), LQ with n <= 64, m <= 8
    auto large = [&]() {
        // DDP_FORWARD64=0: run-time-sized kernels also at n = 64, m = 8.  Up to 4 step sizes of a trajectory per wave (operands fetched
        // once); a single α, and a call without a policy, keep the one-rollout instantiation
        if (n == 64 && m == 8 && !is(q.forward64, '0')) {
            c.na = !q.has_policy ? 1 : (nalpha >= 3 ? 4 : (nalpha == 2 ? 2 : 1));
            return pick(FP_BIG64);
        }
        // DDP_FORWARD_MID=0: forward_big_kernel and the run-time-sized cost kernel below n = 64 too
        if (n <= DDP_MAX_N_GENERIC && !is(q.mid, '0')) return pick(FP_MID);
        c.cost_mid = n > DDP_MAX_N_GENERIC && !is(q.mid, '0');      // the cost kernel of the mid-size rollouts at the larger paddings
        return pick(FP_BIG);
    };
    if (m > DDP_MAX_M) return (lq && n >= 1 && n <= 64 && m <= DDP_MAX_M_WIDE) ? pick(FP_WIDE) : c;
    if (n > DDP_MAX_N_GENERIC) return (lq && n <= 64) ? large() : c;       // above the run-time-sized kernels: LQ only
    if (p.diff_wrap == 0 && is(q.forward, 'b') && lq) return large();
    if (is(q.forward, 'g')) return pick(FP_GROUP);
    const bool fuse = p.cost_diag != 0 && !is(q.fuse, '0');                 // Q, R declared diagonal: cost inside the rollout kernel
    // the pendulum's own kernels (DDP_FORWARD_PEND=0: the generic row kernel): their stores carry no exec-mask branch
    const bool pend_own = pendcart && q.sink && !is(q.pend, '0');
    // wrapped differences exist in the pendulum's own kernels (row and lane) and in the group-of-lanes kernel
    if (p.diff_wrap != 0 && !pend_own) return pick(FP_GROUP);
    if (pendcart || (lq && n == 10 && m == 2)) {
        c.fuse = fuse;
        if (pendcart) {
            c.wrap = p.diff_wrap != 0 && q.has_policy;                      // (only a policy has a difference to wrap)
            // DDP_FORWARD_LANE=1 / 0 forces the lane-per-rollout kernel on / off; by default from ~3 rollouts per lane of a row kernel wave
            if (q.lane ? q.lane[0] == '1' : total >= 12288) return pick(FP_PEND_LANE);
            // 16-step chunks through LDS from 3 584 rollouts on: below that the element-wise streams keep up with the 208 ns step (0.133
            // ms at 2 048 rollouts of N = 600 against 0.142 chunked: ~15 ticks of chunk bookkeeping per step), above it they are the
            // bound (4 096: 0.189 -> 0.147 ms).  DDP_PEND_CHUNK=0 / 1: never / always.
            if (pend_own) { c.chunked = q.pend_chunk ? q.pend_chunk[0] != '0' : total >= 3584; return pick(FP_PEND_ROW); }
        }
        // The pipeline of (10, 2): a policy, no limits, diagonal costs (DDP_FORWARD_FUSE=0 keeps it out), 16-byte pieces of K_i, x_i, k_i, ū_i — and
        // of A_i, B_i when they vary in time — for the DMA.  One work-group (4 rollouts) per CU: with two the chain waves share their SIMDs
        // and the pass is no faster than the row kernel (2 048 rollouts: 0.215 against 0.201 ms).  DDP_FORWARD_PIPE=0: never, 1 | 2:
        // whatever the number of rollouts (2: the two-row kernel for shared time-invariant dynamics too).
        if (lq && q.has_policy && !q.has_lims && fuse && q.sink && !is(q.pipe, '0') && (is(q.pipe, '1') || is(q.pipe, '2') || total <= 1024) &&
            (q.al16 & FP_AL_POLICY) && !(p.dyn_tv && !(q.al16 & FP_AL_DYN)))
            return pick(p.dyn_tv ? FP_PIPE_TV : (!p.dyn_batched && !is(q.pipe, '2')) ? FP_PIPE4 : FP_PIPE);
        // the 16-lane-row kernel.  DDP_FORWARD_FAST=0: the variant with the run-time dyn_tv test and masked stores; (10, 2) loads ū_i, k_i,
        // K_i[:, j] in 16-byte pieces
        c.fast = q.has_policy && !p.dyn_tv && q.sink && (m != 2 || (q.al16 & FP_AL_ROW)) && !is(q.fast, '0');
        return pick(FP_DPP);
    }
    if (lq) {
        // every other LQ shape a 16-lane row holds: the row kernel compiled for padded sizes.  What no row holds (n > 14 or m > 4, and
        // n > 12 with m > 2: (13,3) (13,4) (14,3) (14,4) used to drop to the group-of-lanes kernel) goes to one wave per rollout
        // (n = 24, m = 4, N = 300, B = 1 024 LTV: 0.56 ms on forward_mid_kernel against 3.1 on forward_big_kernel and 6.0 on the group
        // kernel)
        const bool row_holds = m <= 4 && n <= 14 && !(n > 12 && m > 2);
        if (!row_holds) return large();
        if (n >= 1 && m >= 1) return pick(FP_ROW);
    }
    return pick(FP_GROUP);
}

static FPChoiceIn fp_choice_in(ddp_handle h, const FPCall &c)
{
    auto al16 = [](uintptr_t p) { return (p & 15) == 0; };
    const uintptr_t ukK = (uintptr_t)c.u | (uintptr_t)c.k | (uintptr_t)c.K;
    return {(al16(ukK | (uintptr_t)c.x) ? FP_AL_POLICY : 0u) | (al16((uintptr_t)c.p->A | (uintptr_t)c.p->Bm) ? FP_AL_DYN : 0u) | (al16(ukK) ? FP_AL_ROW : 0u),
            h->sink != nullptr, c.K != nullptr, c.lims != nullptr, ddp_env(h, ENV_FORWARD), ddp_env(h, ENV_FORWARD_PIPE), ddp_env(h, ENV_FORWARD_FUSE),
            ddp_env(h, ENV_FORWARD_PEND), ddp_env(h, ENV_FORWARD_LANE), ddp_env(h, ENV_FORWARD64), ddp_env(h, ENV_FORWARD_MID),
            ddp_env(h, ENV_FORWARD_FAST), ddp_env(h, ENV_PEND_CHUNK)};
}

// the group-of-lanes kernel of this file: the instantiations compiled for a shape, run-time sizes otherwise
static int launch_group(ddp_handle h, const FPCall &c)
{
    const ddp_problem *p = c.p;
    FPArgs a;
    fp_fill(a, c);
    a.n = p->n; a.m = p->m; a.wrap = p->diff_wrap; a.lims = c.lims;
    a.dyn_tv = p->dyn_tv; a.dyn_batched = p->dyn_batched; a.has_policy = c.K != nullptr; a.has_lims = c.lims != nullptr;
    a.g = p->g; a.l = p->l; a.h = p->h; a.d = p->d;
    for (int i = 0; i < 4; ++i) a.goal[i] = p->goal[i];
    if (p->kind == DDP_PROBLEM_PENDCART) return launch_fp<DDP_PROBLEM_PENDCART, 4, 1, 4>(h, a);
    if (p->n == 10 && p->m == 2) return launch_fp<DDP_PROBLEM_LQ, 10, 2, 16>(h, a);
    if (p->n == 4 && p->m == 1) return launch_fp<DDP_PROBLEM_LQ, 4, 1, 4>(h, a);
    if (p->n == 6 && p->m == 3) return launch_fp<DDP_PROBLEM_LQ, 6, 3, 8>(h, a);
    if (p->n <= 16) return launch_fp<DDP_PROBLEM_LQ, 0, 0, 16>(h, a);
    return launch_fp<DDP_PROBLEM_LQ, 0, 0, 32>(h, a);
}

int ddp_forward_pass_f64_dev(ddp_handle h, const ddp_problem *p, const double *K, const double *k,
                             const double *x0, const double *u, const double *x, const double *alpha,
                             int nalpha, const double *lims, const int32_t *active, double *xnew,
                             double *unew, double *cnew, double *csum)
{
    DDP_DEVICE(h);
    DDP_CHECK(h && p, "forward_pass: null handle/problem");
    DDP_CHECK(nalpha >= 1 && nalpha <= 16, "forward_pass: nalpha=%d out of [1,16]", nalpha);
    DDP_CHECK((K == nullptr) == (k == nullptr), "forward_pass: K and k must both be given or both NULL");
    DDP_CHECK(!K || x, "forward_pass: a non-empty policy needs the nominal trajectory x");
    DDP_CHECK(p->m <= DDP_MAX_M_WIDE && p->n <= 64, "forward_pass: n=%d m=%d unsupported (n<=64, m<=%d)", p->n, p->m, DDP_MAX_M_WIDE);
    DDP_CHECK(p->kind == DDP_PROBLEM_LQ || p->kind == DDP_PROBLEM_PENDCART, "forward_pass: unknown problem kind %d", p->kind);
    // the pendulum's kernels are compiled for its shape: refused here, whichever kernel the call would get
    DDP_CHECK(p->kind != DDP_PROBLEM_PENDCART || (p->n == 4 && p->m == 1), "forward_pass: pendcart needs n=4, m=1 (got n=%d, m=%d)", p->n, p->m);
    // the trailing field of ddp_problem (library 0.2.0): a caller built against the older layout, or one that does not zero the struct,
    // hands over garbage here — anything but 0 / 1 is refused instead of silently selecting the diagonal-cost rollout
    DDP_CHECK(p->cost_diag == 0 || p->cost_diag == 1, "forward_pass: ddp_problem.cost_diag = %d (0 or 1; zero-initialise the struct)", p->cost_diag);
    if (p->cost_diag) { const int rd = ddp_check_cost_diag(h, p); if (rd) return rd; }
    // diff_fun with wrapped coordinates: the pendulum's row / lane kernels and the run-time-sized group kernel implement it
    DDP_CHECK(p->diff_wrap == 0 || (p->n <= DDP_MAX_N_GENERIC && (p->n >= 32 || (p->diff_wrap >> p->n) == 0)),
              "forward_pass: ddp_problem.diff_wrap = 0x%x needs n <= %d and no bits at or above n = %d (zero-initialise the struct)", p->diff_wrap, DDP_MAX_N_GENERIC, p->n);
    const FPCall c = {p, K, k, x0, u, x, alpha, lims, nalpha, active, xnew, unew, cnew, csum};
    const FPChoice ch = fp_choose(*p, nalpha, fp_choice_in(h, c));
    h->last_kernel[1] = fp_kernel_name[ch.k];
    switch (ch.k) {
    case FP_WIDE: return ddp_launch_forward_wide(h, c);
    case FP_BIG64: case FP_MID: case FP_BIG: return ddp_launch_forward_big(h, c, ch);
    case FP_PIPE4: case FP_PIPE: case FP_PIPE_TV: return ddp_launch_forward_pipe(h, c, ch);
    case FP_PEND_LANE: case FP_PEND_ROW: case FP_DPP: return ddp_launch_forward_dpp(h, c, ch);
    case FP_ROW: return ddp_launch_forward_row(h, c);
    case FP_GROUP: return launch_group(h, c);
    default: break;
    }
    DDP_CHECK(false, "forward_pass: n=%d m=%d has no kernel", p->n, p->m);
}

// Unlisted debug hook (not in ddp_amd.h): the name ddp_last_kernel(h, 1) reports after a forward pass with these facts — the same
// choice the dispatcher makes, callable without a GPU (tests/test_fp_choice.py).  Of *p the sizes and flags are read, no pointer.
// al16: bit 0 K, k, u, x; bit 1 A, Bm; bit 2 u, k, K 16-byte aligned.  sw: the nine switches as strings (NULL: unset) in the order
// DDP_FORWARD, DDP_FORWARD_PIPE, DDP_FORWARD_FUSE, DDP_FORWARD_PEND, DDP_FORWARD_LANE, DDP_FORWARD64, DDP_FORWARD_MID, DDP_FORWARD_FAST,
// DDP_PEND_CHUNK.  label (may be NULL): the enumerator and its variant facts, e.g. "pend_row+fuse+chunked", "big64+na4", "big+cost_mid".
extern "C" const char *ddp_fp_choice(const ddp_problem *p, int nalpha, unsigned al16, int sink, int has_policy, int has_lims,
                                     const char *const *sw, char *label, int label_len)
{
    const FPChoiceIn q = {al16, sink != 0, has_policy != 0, has_lims != 0, sw[0], sw[1], sw[2], sw[3], sw[4], sw[5], sw[6], sw[7], sw[8]};
    const FPChoice ch = fp_choose(*p, nalpha, q);
    if (label && label_len > 0)
        snprintf(label, (size_t)label_len, "%s%s%s%s%s%s%s", fp_kernel_label[ch.k], ch.fuse ? "+fuse" : "", ch.chunked ? "+chunked" : "", ch.fast ? "+fast" : "",
                 ch.wrap ? "+wrap" : "", ch.cost_mid ? "+cost_mid" : "", ch.k != FP_BIG64 ? "" : ch.na == 4 ? "+na4" : ch.na == 2 ? "+na2" : "+na1");
    return fp_kernel_name[ch.k];
}
