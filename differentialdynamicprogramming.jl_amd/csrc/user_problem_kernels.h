// user_problem_kernels.h — the kernel templates of a user problem (user_problem.hip), as program text for hiprtc.
//
// The program hiprtc compiles is: the size / flag macros (DDP_N, DDP_M, DDP_NP, DDP_TERMINAL, DDP_CONST_HESSIAN, DDP_WRAP, DDP_CHUNK,
// DDP_RLANES, DDP_DFLANES, DDP_AUTODIFF, DDP_ADJ, DDP_ADH, DDP_PLANT), the user's source (with DDP_AUTODIFF between the texts of user_autodiff.h),
// DDP_USER_ABI (the argument structs, shared with the host through the macro below) and kUserKernels.  Every size is a compile-time constant there: the state of a rollout stays in VGPRs and every loop over n, m unrolls.
//
//   ddp_user_rollout   one lane per (trajectory, α) rollout, DDP_RLANES rollouts per 64-lane work-group.  The operand streams (u, x, k, K)
//                      of DDP_CHUNK steps are staged through LDS as one contiguous run per rollout and stream (a rollout's chunk of K is
//                      m·n·DDP_CHUNK doubles back to back in memory), the results (x̂, û, cost) go back the same way into the slots of
//                      the operands they replace: a lane that walks its own time steps would issue one 8-byte access per lane and step,
//                      the pattern that tops out at ~1.8 TB/s (profiles/r06_narrow_streams.txt).  The stage cost is fused (csum).
//   ddp_user_df        one lane per (time step, trajectory), DDP_DFLANES per work-group; `derivatives` writes straight into the lane's
//                      LDS slot, and each output array leaves as the contiguous run of the work-group's (step, trajectory) pairs.
//   ddp_user_df_ad     DDP_AUTODIFF (in place of ddp_user_df): the same, with forward-mode AD of the templated model (user_autodiff.h)
//                      writing the slot.
//   ddp_user_cost      costfun on given trajectories: one wave per trajectory, lanes over time.
//   ddp_user_hessians  DDP_CONST_HESSIAN: cost_hessians once per trajectory (per armed slot in the slot scheduler: `active`).
//   ddp_user_plant     DDP_PLANT: one lane per slot of the closed loop; the user's plant advances the trajectories whose solve has just
//                      ended (xcl[:, t+1], and the next solve's initial state).
#pragma once

// argument structs of the kernels: compiled into the host library and, as text (DDP_USER_ABI_TEXT), into every user program.
// Only int / pointer / double members, so that both compilers lay them out alike.
#define DDP_USER_ABI                                                                                                                  \
    struct UserRollArgs {                                                                                                            \
        int N, B, nalpha, has_policy, has_lims, params_batched;                                                                       \
        const double *params, *K, *k, *x0, *u, *x, *lims;                                                                            \
        const int *active, *map;                                                                                                     \
        double *xnew, *unew, *cnew, *csum;                                                                                           \
        double alpha[16];                                                                                                            \
    };                                                                                                                               \
    struct UserDfArgs {                                                                                                              \
        int N, B, params_batched, pad_;                                                                                              \
        const double *params, *x, *u;                                                                                                \
        const int *active, *map;                                                                                                     \
        double *fx, *fu, *cx, *cu, *cxx, *cxu, *cuu;                                                                                 \
    };                                                                                                                               \
    struct UserCostArgs {                                                                                                            \
        int N, B, params_batched, pad_;                                                                                              \
        const double *params, *x, *u;                                                                                                \
        const int *active, *map;                                                                                                     \
        double *cost, *csum;                                                                                                         \
    };                                                                                                                               \
    struct UserHessArgs {                                                                                                            \
        int B, params_batched;                                                                                                       \
        const double *params;                                                                                                        \
        const int *map, *active;                                                                                                     \
        double *cxx, *cxu, *cuu;                                                                                                     \
    };                                                                                                                               \
    struct UserPlantArgs {                                                                                                           \
        int S, steps, params_batched, pad_;                                                                                          \
        const double *params, *ucl;                                                                                                  \
        const int *adv, *advp, *map;                                                                                                 \
        double *xcl, *x0s;                                                                                                           \
    };
#define DDP_USER_STR_(...) #__VA_ARGS__
#define DDP_USER_STR(x) DDP_USER_STR_(x)
#define DDP_USER_ABI_TEXT DDP_USER_STR(DDP_USER_ABI)

static const char *kUserKernels = R"DDPK(
#define DDP_PS (2 * DDP_M + DDP_M * DDP_N + DDP_N)            // doubles per rollout step in LDS: u, x, k, K
#define DDP_RS ((DDP_CHUNK * DDP_PS) | 1)                     // per-rollout stride (odd: 8-byte accesses of a wave spread over the banks)
#define DDP_DT (DDP_N * DDP_N + DDP_N * DDP_M + DDP_N + DDP_M + (DDP_CONST_HESSIAN ? 0 : DDP_N * DDP_N + DDP_N * DDP_M + DDP_M * DDP_M))
#define DDP_DS (DDP_DT | 1)

__device__ __forceinline__ void ddp_wave_sync()              // one wave per work-group: a wave barrier with LDS fences
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

__device__ __forceinline__ double ddp_wrap_pi(double d)     // rem2pi(d, RoundNearest), as ddp_problem::diff_wrap
{
    const double q = rint(d * 0x1.45f306dc9c883p-3);
    return fma(-q, 0x1.1a62633145c07p-52, fma(-q, 0x1.921fb54442d18p+2, d));
}

// the parameters of slot b; NULL for an empty (-1) or resting (-2) slot of the scheduler's map, whose lanes never run the model
__device__ __forceinline__ const double *ddp_params(const double *P, int batched, const int *map, int b)
{
    if (!P) return nullptr;
    if (!batched) return P;
    const int j = map ? map[b] : b;
    return j >= 0 ? P + (size_t)DDP_NP * (size_t)j : nullptr;
}

// chunk [i0, i0 + cs) of one operand stream (W doubles per step) of every rollout of the work-group into its LDS slots
template <int W, int OFF>
__device__ __forceinline__ void ddp_roll_load(double *lds, const int *rb, const double *src, int N, int i0, int cs, int lane)
{
    constexpr int RUN = W * DDP_CHUNK;
    for (int g = lane; g < DDP_RLANES * RUN; g += 64) {
        const int t = g / RUN, r = g - t * RUN, s = r / W, e = r - s * W;
        const int bt = rb[t];
        if (bt >= 0 && s < cs) lds[t * DDP_RS + s * DDP_PS + OFF + e] = src[(size_t)W * N * bt + (size_t)W * i0 + r];
    }
}

// the same chunk of one result stream (W doubles per step, `per` doubles per rollout in memory) from LDS to the rollouts' rows
template <int W, int OFF>
__device__ __forceinline__ void ddp_roll_store(const double *lds, const int *rb, double *dst, size_t per, long rho0, int i0, int cs, int lane)
{
    constexpr int RUN = W * DDP_CHUNK;
    for (int g = lane; g < DDP_RLANES * RUN; g += 64) {
        const int t = g / RUN, r = g - t * RUN, s = r / W, e = r - s * W;
        if (rb[t] >= 0 && s < cs) dst[per * (size_t)(rho0 + t) + (size_t)W * i0 + r] = lds[t * DDP_RS + s * DDP_PS + OFF + e];
    }
}

extern "C" __global__ __launch_bounds__(64) void ddp_user_rollout(UserRollArgs a)
{
    constexpr int n = DDP_N, m = DDP_M, OU = 0, OX = DDP_M, OK = DDP_M + DDP_N, OKK = 2 * DDP_M + DDP_N;
    __shared__ double lds[DDP_RLANES * DDP_RS];
    __shared__ int rb[DDP_RLANES];                            // trajectory of each rollout of the work-group, -1: nothing to do
    const int lane = threadIdx.x, N = a.N, B = a.B, CL = DDP_TERMINAL ? N + 1 : N;
    const long total = (long)B * a.nalpha, rho0 = (long)blockIdx.x * DDP_RLANES, rho = rho0 + lane;
    const bool mine = lane < DDP_RLANES && rho < total;
    const int b = mine ? (int)(rho % B) : 0, ai = mine ? (int)(rho / B) : 0;
    const bool act = mine && !(a.active && a.active[b] == 0);
    if (lane < DDP_RLANES) rb[lane] = act ? b : -1;
    const double alpha = a.alpha[ai];
    const double *p = ddp_params(a.params, a.params_batched, a.map, b);
    double xh[n], lo[m], hi[m];
#pragma unroll
    for (int l = 0; l < n; ++l) xh[l] = act ? a.x0[(size_t)n * b + l] : 0.0;
#pragma unroll
    for (int q = 0; q < m; ++q) { lo[q] = a.has_lims ? a.lims[q] : 0.0; hi[q] = a.has_lims ? a.lims[q + m] : 0.0; }
    double csum = 0.0;
    ddp_wave_sync();
    for (int i0 = 0; i0 < N; i0 += DDP_CHUNK) {
        const int cs = N - i0 < DDP_CHUNK ? N - i0 : DDP_CHUNK;
        ddp_roll_load<m, OU>(lds, rb, a.u, N, i0, cs, lane);
        if (a.has_policy) {
            ddp_roll_load<n, OX>(lds, rb, a.x, N, i0, cs, lane);
            ddp_roll_load<m, OK>(lds, rb, a.k, N, i0, cs, lane);
            ddp_roll_load<m * n, OKK>(lds, rb, a.K, N, i0, cs, lane);
        }
        ddp_wave_sync();
        if (act) {
            for (int s = 0; s < cs; ++s) {
                const int i = i0 + s;
                double *L = lds + lane * DDP_RS + s * DDP_PS;
                double uu[m];
#pragma unroll
                for (int q = 0; q < m; ++q) uu[q] = L[OU + q];
                if (a.has_policy) {                            // forward_pass.jl:17-20: unew += k α;  unew += K diff(x̂, x)
                    double dx[n];
#pragma unroll
                    for (int l = 0; l < n; ++l) {
                        double d = xh[l] - L[OX + l];
                        if ((DDP_WRAP >> l) & 1u) d = ddp_wrap_pi(d);
                        dx[l] = d;
                    }
#pragma unroll
                    for (int q = 0; q < m; ++q) {
                        double v = uu[q] + L[OK + q] * alpha, s2 = 0.0;
#pragma unroll
                        for (int l = 0; l < n; ++l) s2 += L[OKK + q + m * l] * dx[l];
                        uu[q] = v + s2;
                    }
                }
                if (a.has_lims) {                              // :22-24
#pragma unroll
                    for (int q = 0; q < m; ++q) uu[q] = uu[q] > hi[q] ? hi[q] : (uu[q] < lo[q] ? lo[q] : uu[q]);
                }
                const double c = stage_cost(xh, uu, i, p);
                csum += c;
#pragma unroll
                for (int q = 0; q < m; ++q) L[OU + q] = uu[q];
#pragma unroll
                for (int l = 0; l < n; ++l) L[OX + l] = xh[l];
                L[OK] = c;
                if (i < N - 1) {                               // :25-28 (the successor of the last step is not stored)
                    double xn[n];
                    dynamics(xh, uu, i, p, xn);
#pragma unroll
                    for (int l = 0; l < n; ++l) xh[l] = xn[l];
                }
            }
        }
        ddp_wave_sync();
        ddp_roll_store<n, OX>(lds, rb, a.xnew, (size_t)n * N, rho0, i0, cs, lane);
        ddp_roll_store<m, OU>(lds, rb, a.unew, (size_t)m * N, rho0, i0, cs, lane);
        ddp_roll_store<1, OK>(lds, rb, a.cnew, (size_t)CL, rho0, i0, cs, lane);
        ddp_wave_sync();
    }
#if DDP_TERMINAL
    if (act) {
        const double c = terminal_cost(xh, p);
        a.cnew[(size_t)CL * rho + N] = c;
        csum += c;
    }
#endif
    if (act) a.csum[rho] = csum;
}

template <int S, int OFF>
__device__ __forceinline__ void ddp_df_store(const double *lds, const int *rb, double *dst, long r0, int lane)
{
    if (!dst) return;
    for (int g = lane; g < DDP_DFLANES * S; g += 64) {
        const int t = g / S, e = g - t * S;
        if (rb[t] >= 0) dst[(size_t)S * (size_t)(r0 + t) + e] = lds[t * DDP_DS + OFF + e];
    }
}

// ddp_user_df_ad (DDP_AUTODIFF): the same kernel, with the lane's slot written by ddp_ad_derivatives (user_autodiff.h), the derivatives of
// the user's templated model, instead of the user's `derivatives`
#if DDP_AUTODIFF
#define DDP_DF_KERNEL ddp_user_df_ad
#define DDP_DERIVATIVES ddp_ad_derivatives
#else
#define DDP_DF_KERNEL ddp_user_df
#define DDP_DERIVATIVES derivatives
#endif
extern "C" __global__ __launch_bounds__(64) void DDP_DF_KERNEL(UserDfArgs a)
{
    constexpr int n = DDP_N, m = DDP_M;
    constexpr int OFX = 0, OFU = OFX + n * n, OCX = OFU + n * m, OCU = OCX + n, OXX = OCU + m, OXU = OXX + n * n, OUU = OXU + n * m;
    __shared__ double lds[DDP_DFLANES * DDP_DS];
    __shared__ int rb[DDP_DFLANES];
    const int lane = threadIdx.x, N = a.N;
    const long R = (long)N * a.B, r0 = (long)blockIdx.x * DDP_DFLANES, r = r0 + lane;
    if (lane < DDP_DFLANES) {
        int b = -1, i = 0;
        if (r < R) {
            b = (int)(r / N); i = (int)(r - (long)b * N);
            if (a.active && a.active[b] == 0) b = -1;
        }
        rb[lane] = b;
        if (b >= 0) {
            double x[n], u[m];
#pragma unroll
            for (int l = 0; l < n; ++l) x[l] = a.x[(size_t)n * r + l];
#pragma unroll
            for (int q = 0; q < m; ++q) u[q] = a.u[(size_t)m * r + q];
            const double *p = ddp_params(a.params, a.params_batched, a.map, b);
            double *L = lds + lane * DDP_DS;
#if DDP_CONST_HESSIAN
            // the Hessians `derivatives` writes are not used (cost_hessians supplies them): lane-private arrays that are never read,
            // so the compiler drops the stores
            double nxx[n * n], nxu[n * m], nuu[m * m];
            DDP_DERIVATIVES(x, u, i, N, p, L + OFX, L + OFU, L + OCX, L + OCU, nxx, nxu, nuu);
#else
            DDP_DERIVATIVES(x, u, i, N, p, L + OFX, L + OFU, L + OCX, L + OCU, L + OXX, L + OXU, L + OUU);
#endif
        }
    }
    ddp_wave_sync();
    ddp_df_store<n * n, OFX>(lds, rb, a.fx, r0, lane);
    ddp_df_store<n * m, OFU>(lds, rb, a.fu, r0, lane);
    ddp_df_store<n, OCX>(lds, rb, a.cx, r0, lane);
    ddp_df_store<m, OCU>(lds, rb, a.cu, r0, lane);
#if !DDP_CONST_HESSIAN
    ddp_df_store<n * n, OXX>(lds, rb, a.cxx, r0, lane);
    ddp_df_store<n * m, OXU>(lds, rb, a.cxu, r0, lane);
    ddp_df_store<m * m, OUU>(lds, rb, a.cuu, r0, lane);
#endif
}

extern "C" __global__ __launch_bounds__(64) void ddp_user_cost(UserCostArgs a)
{
    constexpr int n = DDP_N, m = DDP_M;
    const int b = blockIdx.x, lane = threadIdx.x, N = a.N, CL = DDP_TERMINAL ? N + 1 : N;
    if (a.active && a.active[b] == 0) return;
    const double *p = ddp_params(a.params, a.params_batched, a.map, b);
    double acc = 0.0;
    for (int t = lane; t < CL; t += 64) {
        const int tx = t < N ? t : N - 1;
        double x[n], u[m];
#pragma unroll
        for (int l = 0; l < n; ++l) x[l] = a.x[(size_t)n * ((size_t)N * b + tx) + l];
#pragma unroll
        for (int q = 0; q < m; ++q) u[q] = a.u[(size_t)m * ((size_t)N * b + tx) + q];
        double c;
#if DDP_TERMINAL
        c = t < N ? stage_cost(x, u, t, p) : terminal_cost(x, p);
#else
        c = stage_cost(x, u, t, p);
#endif
        a.cost[(size_t)CL * b + t] = c;
        acc += c;
    }
    for (int off = 32; off >= 1; off >>= 1) acc += __shfl_xor(acc, off, 64);
    if (lane == 0 && a.csum) a.csum[b] = acc;
}

#if DDP_CONST_HESSIAN
extern "C" __global__ __launch_bounds__(64) void ddp_user_hessians(UserHessArgs a)
{
    constexpr int n = DDP_N, m = DDP_M;
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b >= a.B || (a.active && a.active[b] == 0)) return;
    double hxx[n * n], hxu[n * m], huu[m * m];
    cost_hessians(ddp_params(a.params, a.params_batched, a.map, b), hxx, hxu, huu);
    for (int e = 0; e < n * n; ++e) a.cxx[(size_t)n * n * b + e] = hxx[e];
    for (int e = 0; e < n * m; ++e) a.cxu[(size_t)n * m * b + e] = hxu[e];
    for (int e = 0; e < m * m; ++e) a.cuu[(size_t)m * m * b + e] = huu[e];
}
#endif

#if DDP_PLANT
// xcl[n, steps+1, P], ucl[m, steps, P]; adv[b] = t + 1 when solve t of trajectory advp[b] has just ended on slot b (0: nothing to do)
extern "C" __global__ __launch_bounds__(64) void ddp_user_plant(UserPlantArgs a)
{
    constexpr int n = DDP_N, m = DDP_M;
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b >= a.S) return;
    const int t1 = a.adv[b];
    if (t1 <= 0) return;
    const int t = t1 - 1, j = a.advp[b];
    double *xc = a.xcl + (size_t)n * ((size_t)(a.steps + 1) * j + t);
    const double *uc = a.ucl + (size_t)m * ((size_t)a.steps * j + t);
    double x[n], u[m], xn[n];
#pragma unroll
    for (int l = 0; l < n; ++l) x[l] = xc[l];
#pragma unroll
    for (int q = 0; q < m; ++q) u[q] = uc[q];
    plant(x, u, t, ddp_params(a.params, a.params_batched, a.advp, b), xn);
#pragma unroll
    for (int l = 0; l < n; ++l) xc[n + l] = xn[l];
    if (a.map[b] == j) {                                       // the slot goes on with this trajectory: its next initial state
#pragma unroll
        for (int l = 0; l < n; ++l) a.x0s[(size_t)n * b + l] = xn[l];
    }
}
#endif
)DDPK";
