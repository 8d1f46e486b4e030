// user_problem_kernels.h — the kernel templates of a user problem (user_problem.hip), as program text for hiprtc.
//
// The program hiprtc compiles is: the size / flag macros (DDP_N, DDP_M, DDP_NP, DDP_TERMINAL, DDP_CONST_HESSIAN, DDP_WRAP, DDP_CHUNK,
// DDP_RLANES, DDP_DFLANES, DDP_AUTODIFF, DDP_ADJ, DDP_ADH, DDP_PLANT), the user's source (with DDP_AUTODIFF between the texts of user_autodiff.h),
// DDP_USER_ABI (the argument structs, shared with the host through the macro below) and kUserKernels (five pieces, below).  Every size is a compile-time constant there: the state of a rollout stays in VGPRs and every loop over n, m unrolls.
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
// DDP_USER_WAVE (n <= 64, m <= 32): ddp_user_rollout_wave, ddp_user_df_wave and the direct-store ddp_user_df / ddp_user_hessians of
// user_problem_wave_kernels.h take the place of the rollout, derivative and Hessian kernels here; ddp_user_cost and ddp_user_plant stay.
// DDP_USER_SECOND_ORDER / DDP_USER_SECOND_ORDER_WAVE append a backward pass with the curvature of the dynamics (ddp_user_back_pass2, one
// wave per trajectory, n <= 32, m <= 8; ddp_user_back_pass2_wave, the wide kernel's step, n <= 64, m <= 32) and ddp_user_vhess: below.
#pragma once

// argument structs of the kernels: compiled into the host library and, as text (DDP_USER_ABI_TEXT), into every user program.
// Only int / pointer / double members, so that both compilers lay them out alike.
// DDP_USER_CLOCK: the structs of the kernels that call the user's functions end in the clock pointer (clk[b] of the slot or trajectory b
// the kernel works on; ddp_user_plant: t0[j] of trajectory j; NULL: every clock is 0).  The host always fills the long form; a program
// without the flag is compiled with the text it always had (DDP_USER_ABI_TEXT, the structs without the member) and its kernels read
// the leading bytes of the argument, which are laid out alike.
#define DDP_USER_ABI_(CLK)                                                                                                               \
    struct UserRollArgs {                                                                                                            \
        int N, B, nalpha, has_policy, has_lims, params_batched;                                                                       \
        const double *params, *K, *k, *x0, *u, *x, *lims;                                                                            \
        const int *active, *map;                                                                                                     \
        double *xnew, *unew, *cnew, *csum;                                                                                           \
        double alpha[16];                                                                                                            \
        CLK                                                                                                                          \
    };                                                                                                                               \
    struct UserDfArgs {                                                                                                              \
        int N, B, params_batched, pad_;                                                                                              \
        const double *params, *x, *u;                                                                                                \
        const int *active, *map;                                                                                                     \
        double *fx, *fu, *cx, *cu, *cxx, *cxu, *cuu;                                                                                 \
        CLK                                                                                                                          \
    };                                                                                                                               \
    struct UserCostArgs {                                                                                                            \
        int N, B, params_batched, pad_;                                                                                              \
        const double *params, *x, *u;                                                                                                \
        const int *active, *map;                                                                                                     \
        double *cost, *csum;                                                                                                         \
        CLK                                                                                                                          \
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
        CLK                                                                                                                          \
    };
#define DDP_USER_STR_(...) #__VA_ARGS__
#define DDP_USER_STR(x) DDP_USER_STR_(x)
#define DDP_USER_ABI DDP_USER_ABI_(const int *clk;)
#define DDP_USER_ABI_TEXT DDP_USER_STR(DDP_USER_ABI_())
#define DDP_USER_ABI_CLOCK_TEXT DDP_USER_STR(DDP_USER_ABI)

// kUserKernels in five pieces: a problem without DDP_USER_WAVE compiles Head + Lane + Cost + Hessians + Plant (the same bytes as ever), one
// with the flag Head + kUserWaveKernels (user_problem_wave_kernels.h) + Cost + Plant
static const char *kUserKernelsHead = R"DDPK(
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

)DDPK";

static const char *kUserKernelsLane = R"DDPK(// chunk [i0, i0 + cs) of one operand stream (W doubles per step) of every rollout of the work-group into its LDS slots
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

)DDPK";

static const char *kUserKernelsCost = R"DDPK(extern "C" __global__ __launch_bounds__(64) void ddp_user_cost(UserCostArgs a)
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

)DDPK";

static const char *kUserKernelsHessians = R"DDPK(#if DDP_CONST_HESSIAN
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

)DDPK";

static const char *kUserKernelsPlant = R"DDPK(#if DDP_PLANT
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

// ---- DDP_USER_SECOND_ORDER: appended to the program of a problem with the flag only (a problem without it compiles the text above,
// unchanged).  The program then is: the macros (+ DDP_SECOND_ORDER 1), user_autodiff.h's texts around the user's source, DDP_USER_ABI,
// kUserKernels, ddp_rsqrt + the text of boxqp_dev.h (kBoxqpDevText, written by build.py from the header the precompiled backward
// kernels include: one definition of the Cholesky and the box-QP for both compilers), DDP_USER_ABI2, kUserKernels2.
//
//   ddp_user_back_pass2  the backward pass of backward_pass.jl:81-160 (the reference's second-order variant): Qxx += Vx⁺·fxx,
//                        Qux += Vx⁺·fxu, Quu += Vx⁺·fuu, and the same Hux, Huu in Qux_reg and QuuF.  One wave per trajectory, the step
//                        as in back_pass.hip (P1-P4, operands and intermediates in LDS, fx/fu and the cost Hessians one step ahead in
//                        registers, cx|cu|x|u in chunks of DDP_TC steps) with every size a compile-time constant.  The curvature
//                        H_i = ∇²_z (Vx_{i+1}·f(z)) needs no tensor: the (n+m)(n+m+1)/2 pairs a <= b are dealt over the 64 lanes, each
//                        lane calls ddp_ad_vhess for its pair and adds the value into the LDS image of the step's cost Hessians at
//                        (a, b) and (b, a) before the Q-expansion reads it.  The phase reads Vx_{i+1}, x_i, u_i and the parameters
//                        only, so it runs after the step's prefetch loads are issued, in their shadow.
//   ddp_user_vhess       H[n+m, n+m, N, B] = Σ_k v[k, i, b] ∂²f_k/∂z∂z at (x, u): one lane per (pair, step, trajectory).
#define DDP_USER_ABI2                                                                                                                 \
    struct UserBp2Args {                                                                                                             \
        int N, B, regType, has_lims, params_batched, pad_;                                                                           \
        const double *params, *x, *u, *cx, *cu, *cxx, *cxu, *cuu, *fx, *fu, *lambda, *lims;                                          \
        const int *active, *map;                                                                                                     \
        double *K, *k, *Quu, *Vx, *Vxx, *dV;                                                                                         \
        int *diverge;                                                                                                                \
    };                                                                                                                               \
    struct UserVhessArgs {                                                                                                           \
        int N, B, params_batched, pad_;                                                                                              \
        const double *params, *x, *u, *v;                                                                                            \
        const int *active, *map;                                                                                                     \
        double *H;                                                                                                                   \
    };
#define DDP_USER_ABI2_TEXT DDP_USER_STR(DDP_USER_ABI2)

// 1/sqrt(x) of ddp_internal.h (which hiprtc cannot include), for the text of boxqp_dev.h
static const char *kUserRsqrt = R"DDPK(
__device__ __forceinline__ double ddp_rsqrt(double x)
{
    double y = __builtin_amdgcn_rsq(x);
    double e = fma(-(x * y), y, 1.0);
    y = fma(0.5 * y, e, y);
    e = fma(-(x * y), y, 1.0);
    y = fma(0.5 * y, e, y);
    return y;
}
)DDPK";

// kUserKernels2 in three pieces: a DDP_USER_SECOND_ORDER problem compiles Head + Bp2 + Vhess (the same bytes as ever), one with
// DDP_USER_SECOND_ORDER_WAVE Head + Vhess (the static_assert of ddp_user_back_pass2 on 64 KB fails at its shapes) + kUserKernels2Wave
static const char *kUserKernels2Head = R"DDPK(
#if DDP_SECOND_ORDER
#define DDP_NZ (DDP_N + DDP_M)
#define DDP_NPAIR (DDP_NZ * (DDP_NZ + 1) / 2)
#define DDP_TC 8                                              // time steps per cx | cu | x | u chunk

// Hand-off between the lanes of the one wave of a work-group through LDS.  Wavefront scope: LDS operations of a wave execute in issue
// order, the compiler must not move them across the hand-off, and nothing here may wait for the step's outstanding global loads and
// stores (a wider scope may: the prefetch of the next step would then land on the critical path)
__device__ __forceinline__ void ddp_bp2_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__host__ __device__ constexpr int ddp_cdiv(int a, int b) { return (a + b - 1) / b; }

// element e of the upper triangle stored by columns: e = j (j + 1) / 2 + i, i <= j
__device__ __forceinline__ void ddp_tri(int e, int &i, int &j)
{
    int c = (int)((sqrtf(8.0f * (float)e + 1.0f) - 1.0f) * 0.5f);
    while (c * (c + 1) / 2 > e) --c;
    while ((c + 1) * (c + 2) / 2 <= e) ++c;
    j = c;
    i = e - c * (c + 1) / 2;
}

)DDPK";

static const char *kUserKernels2Bp2 = R"DDPK(extern "C" __global__ __launch_bounds__(64) void ddp_user_back_pass2(UserBp2Args a)
{
    constexpr int n = DDP_N, m = DDP_M, p = DDP_NZ, TC = DDP_TC, HS = DDP_CONST_HESSIAN ? 0 : 1;
    constexpr int nn = n * n, nm = n * m, mm = m * m, ntri = n * (n + 1) / 2;
    constexpr int R1 = ddp_cdiv(n * p, 64), RT = ddp_cdiv(ntri, 64), RU = ddp_cdiv(m * p, 64), RN = ddp_cdiv(nn, 64), RX = ddp_cdiv(nm, 64);
    constexpr int CLEN = 2 * p, RC = ddp_cdiv(TC * CLEN, 64), RP = ddp_cdiv(DDP_NPAIR, 64);
    // LDS carve-up (doubles)
    constexpr int oF = 0, oV = oF + n * p, ov = oV + nn, oW = ov + n, oQ = oW + n * p, oxx = oQ + p, oxu = oxx + nn, ouu = oxu + nm,
                  oQux = ouu + mm, oQuxr = oQux + nm, oQuu = oQuxr + nm, oQuuF = oQuu + mm, oK = oQuuF + mm, ok = oK + nm, oT = ok + m,
                  oQuuk = oT + nm, oC = (oQuuk + m + 1) & ~1, TOTAL = oC + 2 * TC * CLEN;
    static_assert(TOTAL * 8 <= 64 * 1024, "ddp_user_back_pass2: the step does not fit 64 KB of LDS");
    __shared__ double lds[TOTAL];
    double *Fs = lds + oF, *Vs = lds + oV, *vs = lds + ov, *Ws = lds + oW, *Qs = lds + oQ, *cxxs = lds + oxx, *cxus = lds + oxu,
           *cuus = lds + ouu, *Quxs = lds + oQux, *Quxrs = lds + oQuxr, *Quus = lds + oQuu, *QuuFs = lds + oQuuF, *Ks = lds + oK,
           *ks = lds + ok, *Ts = lds + oT, *Quuks = lds + oQuuk, *cbuf = lds + oC;

    const int b = blockIdx.x, lane = threadIdx.x, N = a.N;
    if (b >= a.B || (a.active && a.active[b] == 0)) return;
    const double *pp = ddp_params(a.params, a.params_batched, a.map, b);
    const double *cx = a.cx + (size_t)n * N * b, *cu = a.cu + (size_t)m * N * b, *xg = a.x + (size_t)n * N * b, *ug = a.u + (size_t)m * N * b;
    const double *fx = a.fx + (size_t)nn * N * b, *fu = a.fu + (size_t)nm * N * b;
    const double *cxx = a.cxx + (size_t)nn * (HS ? N : 1) * b, *cxu = a.cxu + (size_t)nm * (HS ? N : 1) * b,
                 *cuu = a.cuu + (size_t)mm * (HS ? N : 1) * b;
    double *Kg = a.K + (size_t)nm * N * b, *kg = a.k + (size_t)m * N * b, *Quug = a.Quu + (size_t)mm * N * b,
           *Vxg = a.Vx + (size_t)n * N * b, *Vxxg = a.Vxx + (size_t)nn * N * b;
    const double lam = a.lambda[b];
    const int regType = a.regType;
    bool nolims = true;
    double limlo[m], limhi[m];
#pragma unroll
    for (int q = 0; q < m; ++q) { limlo[q] = 0.0; limhi[q] = 0.0; }
    if (a.has_lims) {
        nolims = a.lims[0] > a.lims[m];                          // backward_pass.jl:31
#pragma unroll
        for (int q = 0; q < m; ++q) { limlo[q] = a.lims[q]; limhi[q] = a.lims[q + m]; }
    }
    const QPOptsDev qpo = {100, 1e-8, 1e-8, 0.6, 1e-22, 0.1};    // boxQP.jl:30-35

    // ---- per-lane element assignments (loop invariant)
    int t_i[RT], t_j[RT];                                        // P2 / P4: (i <= j) of the Qxx / Vxx upper-triangle element
#pragma unroll
    for (int r = 0; r < RT; ++r) ddp_tri(lane + 64 * r, t_i[r], t_j[r]);
    int h_a[RP], h_b[RP];                                        // curvature phase: the lane's pairs a <= b of z = [x; u]
#pragma unroll
    for (int r = 0; r < RP; ++r) ddp_tri(lane + 64 * r, h_a[r], h_b[r]);

    // chunk c holds the time steps [c TC, c TC + TC) of cx | cu | x | u, time-major per stream
    auto chunk_elem = [&](int c, int e) -> double {              // e in [0, TC * CLEN)
        const int t0 = c * TC;
        if (e < TC * n) return t0 + e / n < N ? cx[(size_t)t0 * n + e] : 0.0;
        e -= TC * n;
        if (e < TC * m) return t0 + e / m < N ? cu[(size_t)t0 * m + e] : 0.0;
        e -= TC * m;
        if (e < TC * n) return t0 + e / n < N ? xg[(size_t)t0 * n + e] : 0.0;
        e -= TC * n;
        return t0 + e / m < N ? ug[(size_t)t0 * m + e] : 0.0;
    };

    // ---- the last step has no dynamics (backward_pass.jl:93-95): Vx = cx, Vxx = cxx, Quu = cuu
    for (int e = lane; e < nn; e += 64) {
        const double v = cxx[(size_t)nn * (N - 1) * HS + e];
        Vs[e] = v;
        Vxxg[(size_t)nn * (N - 1) + e] = v;
    }
    for (int e = lane; e < n; e += 64) {
        const double v = cx[(size_t)n * (N - 1) + e];
        vs[e] = v;
        Vxg[(size_t)n * (N - 1) + e] = v;
    }
    for (int e = lane; e < mm; e += 64) Quug[(size_t)mm * (N - 1) + e] = cuu[(size_t)mm * (N - 1) * HS + e];
    for (int e = lane; e < nm; e += 64) Kg[(size_t)nm * (N - 1) + e] = 0.0;
    for (int e = lane; e < m; e += 64) { kg[(size_t)m * (N - 1) + e] = 0.0; ks[e] = 0.0; }
    double dV0 = 0.0, dV1 = 0.0;
    if (N < 2) {
        if (lane == 0) { a.dV[2 * b] = 0.0; a.dV[2 * b + 1] = 0.0; a.diverge[b] = 0; }
        return;
    }
    // the first step's operands straight to LDS, the next chunk into registers
    double pfc[RC];
    {
        const int c0 = (N - 2) / TC;
        for (int e = lane; e < TC * CLEN; e += 64) cbuf[(c0 & 1) * TC * CLEN + e] = chunk_elem(c0, e);
#pragma unroll
        for (int r = 0; r < RC; ++r) {
            const int e = lane + 64 * r;
            pfc[r] = (c0 > 0 && e < TC * CLEN) ? chunk_elem(c0 - 1, e) : 0.0;
        }
    }
    double pfF[R1], pfxx[RN], pfxu[RX], pfuu = 0.0;
    {
        const int i0 = N - 2;
        for (int e = lane; e < nn; e += 64) { Fs[e] = fx[(size_t)nn * i0 + e]; cxxs[e] = cxx[(size_t)nn * i0 * HS + e]; }
        for (int e = lane; e < nm; e += 64) { Fs[nn + e] = fu[(size_t)nm * i0 + e]; cxus[e] = cxu[(size_t)nm * i0 * HS + e]; }
        for (int e = lane; e < mm; e += 64) cuus[e] = cuu[(size_t)mm * i0 * HS + e];
    }
    ddp_bp2_sync();

    int diverge = 0;
    for (int i = N - 2; i >= 0; --i) {
        const int cc = i / TC;
        const double *cb = cbuf + (cc & 1) * TC * CLEN;
        const double *cxi = cb + (i - cc * TC) * n;
        const double *cui = cb + TC * n + (i - cc * TC) * m;
        const double *xi = cb + TC * p + (i - cc * TC) * n;
        const double *ui = cb + TC * (p + n) + (i - cc * TC) * m;

        // ---- issue the next step's operands (they land while this step computes)
        if (i > 0) {
#pragma unroll
            for (int r = 0; r < R1; ++r) {
                const int e = lane + 64 * r;
                if (e < n * p) pfF[r] = (e < nn) ? fx[(size_t)nn * (i - 1) + e] : fu[(size_t)nm * (i - 1) + (e - nn)];
            }
#pragma unroll
            for (int r = 0; r < RN; ++r) {
                const int e = lane + 64 * r;
                if (e < nn) pfxx[r] = cxx[(size_t)nn * (i - 1) * HS + e];
            }
#pragma unroll
            for (int r = 0; r < RX; ++r) {
                const int e = lane + 64 * r;
                if (e < nm) pfxu[r] = cxu[(size_t)nm * (i - 1) * HS + e];
            }
            if (lane < mm) pfuu = cuu[(size_t)mm * (i - 1) * HS + lane];
        }

        // ================= P0: H = ∇²_z (Vx_{i+1}·f)(x_i, u_i) into the cost Hessians of the step (:106-123) =================
        // every pair belongs to one lane and is written to (a, b) and (b, a): cxx + Hxx and cuu + Huu stay exactly symmetric
#ifndef DDP_BP2_NO_CURVATURE                                      // (a source that defines it: the pass without P0, for bench/user_second_order.py)
#pragma unroll
        for (int r = 0; r < RP; ++r) {
            if (lane + 64 * r < DDP_NPAIR) {
                const int pa = h_a[r], pb = h_b[r];
                const double hv = ddp_ad_vhess(xi, ui, i, pp, vs, pa, pb);
                if (pb < n) {
                    cxxs[pa + n * pb] += hv;
                    if (pa != pb) cxxs[pb + n * pa] += hv;
                } else if (pa < n) {
                    cxus[pa + n * (pb - n)] += hv;
                } else {
                    cuus[(pa - n) + m * (pb - n)] += hv;
                    if (pa != pb) cuus[(pb - n) + m * (pa - n)] += hv;
                }
            }
        }
#endif

        // ================= P1: W = Vxx·F,  Qs = [cx; cu] + F'Vx =================
#pragma unroll
        for (int r = 0; r < R1; ++r) {
            const int e = lane + 64 * r;
            if (e < n * p) {
                const double *vc = Vs + (e % n) * n, *fc = Fs + (e / n) * n;
                double s = 0.0;
#pragma unroll
                for (int l = 0; l < n; ++l) s += vc[l] * fc[l];
                Ws[e] = s;
            }
        }
        for (int j = 63 - lane; j < p; j += 64) {                // high lanes: idle in the last W round
            const double *fc = Fs + j * n;
            double s = 0.0;
#pragma unroll
            for (int l = 0; l < n; ++l) s += fc[l] * vs[l];
            Qs[j] = (j < n ? cxi[j] : cui[j - n]) + s;
        }
        ddp_bp2_sync();

        // ================= P2: Qxx (registers), Qux, Quu and the regularised variants =================
        double qxx[RT];
#pragma unroll
        for (int r = 0; r < RT; ++r) {
            const int e = lane + 64 * r;
            qxx[r] = 0.0;
            if (e < ntri) {
                const double *fc = Fs + t_i[r] * n, *wc = Ws + t_j[r] * n;
                double s = 0.0;
#pragma unroll
                for (int l = 0; l < n; ++l) s += fc[l] * wc[l];
                qxx[r] = cxxs[t_i[r] + n * t_j[r]] + s;
            }
        }
#pragma unroll
        for (int r = 0; r < RU; ++r) {
            const int e = (63 - lane) + 64 * r;
            if (e < m * p) {
                const int q = e % m, j = e / m;
                const double *fc = Fs + (n + q) * n, *wc = Ws + j * n, *fj = Fs + j * n;
                double s = 0.0, sr = 0.0;
#pragma unroll
                for (int l = 0; l < n; ++l) { s += fc[l] * wc[l]; sr += fc[l] * fj[l]; }
                if (j < n) {                                     // Qux, Qux_reg
                    const double c = cxus[j + n * q];
                    Quxs[q + m * j] = c + s;
                    Quxrs[q + m * j] = c + (regType == 2 ? s + lam * sr : s);
                } else {                                         // Quu, QuuF
                    const int bb = j - n;
                    const double c = cuus[q + m * bb];
                    Quus[q + m * bb] = c + s;
                    QuuFs[q + m * bb] = c + (regType == 2 ? s + lam * sr : s) + ((regType == 1 && q == bb) ? lam : 0.0);
                }
            }
        }
        ddp_bp2_sync();

        // ================= P3: gains (backward_pass.jl:30-62), every lane the same solve =================
        double H[mm], R[mm], kk[m], ri[m];
        unsigned clamped = 0u;
#pragma unroll
        for (int e = 0; e < mm; ++e) H[e] = QuuFs[e];
        int fail;
        if (nolims) {
            fail = chol_masked_ri<m>(m, H, 0u, R, ri);
#pragma unroll
            for (int q = 0; q < m; ++q) kk[q] = Qs[n + q];
            chol_solve_ri<m>(m, R, ri, kk);
#pragma unroll
            for (int q = 0; q < m; ++q) kk[q] = -kk[q];
        } else {
            double g[m], lo[m], up[m], x0[m];
#pragma unroll
            for (int q = 0; q < m; ++q) {
                const double uq = ui[q];
                g[q] = Qs[n + q];
                lo[q] = limlo[q] - uq;
                up[q] = limhi[q] - uq;
                x0[q] = ks[q];                                   // k[:, min(i+1, N-1)]
            }
            int iters;
            const int result = boxqp_dev_ri<m>(m, H, g, lo, up, x0, qpo, kk, R, ri, clamped, iters);
            fail = (result < 1);
        }
        if (fail) {                                              // wave-uniform: diverge = i (1-based)
            diverge = i + 1;
            for (int e = lane; e < mm; e += 64) Quug[(size_t)mm * i + e] = Quus[e];   // the reference has stored Quu[:,:,i] already
            for (size_t e = lane; e < (size_t)nm * (i + 1); e += 64) Kg[e] = 0.0;
            for (size_t e = lane; e < (size_t)m * (i + 1); e += 64) kg[e] = 0.0;
            for (size_t e = lane; e < (size_t)n * (i + 1); e += 64) Vxg[e] = 0.0;
            for (size_t e = lane; e < (size_t)nn * (i + 1); e += 64) Vxxg[e] = 0.0;
            for (size_t e = lane; e < (size_t)mm * i; e += 64) Quug[e] = 0.0;
            break;
        }
        if (lane < n) {                                          // column `lane` of K_i
            double col[m];
#pragma unroll
            for (int q = 0; q < m; ++q) col[q] = ((clamped >> q) & 1u) ? 0.0 : Quxrs[q + m * lane];
            chol_solve<m>(m, R, col);
#pragma unroll
            for (int q = 0; q < m; ++q) col[q] = ((clamped >> q) & 1u) ? 0.0 : -col[q];
#pragma unroll
            for (int q = 0; q < m; ++q) {
                double t = Quxs[q + m * lane];                   // T = Quu·K + Qux
#pragma unroll
                for (int q2 = 0; q2 < m; ++q2) t += Quus[q + m * q2] * col[q2];
                Ks[q + m * lane] = col[q];
                Ts[q + m * lane] = t;
            }
        } else if (lane == n) {                                  // k_i, Quu·k, dV
            double kQu = 0.0, kQuuk = 0.0;
#pragma unroll
            for (int q = 0; q < m; ++q) {
                double t = 0.0;
#pragma unroll
                for (int q2 = 0; q2 < m; ++q2) t += Quus[q + m * q2] * kk[q2];
                Quuks[q] = t;
                ks[q] = kk[q];
                kQu += kk[q] * Qs[n + q];
                kQuuk += kk[q] * t;
            }
            dV0 += kQu;
            dV1 += 0.5 * kQuuk;
        }
        ddp_bp2_sync();

        // ================= P4: value update, stores, operand hand-over =================
#pragma unroll
        for (int r = 0; r < RT; ++r) {
            const int e = lane + 64 * r;
            if (e < ntri) {
                const int ii = t_i[r], jj = t_j[r];
                double mij = qxx[r], mji = qxx[r];
#pragma unroll
                for (int q = 0; q < m; ++q) {
                    const double Ki = Ks[q + m * ii], Kj = Ks[q + m * jj];
                    mij += Ki * Ts[q + m * jj] + Quxs[q + m * ii] * Kj;
                    mji += Kj * Ts[q + m * ii] + Quxs[q + m * jj] * Ki;
                }
                const double v = (mij + mji) / 2;
                Vs[ii + n * jj] = v;
                Vs[jj + n * ii] = v;
                Vxxg[(size_t)nn * i + ii + n * jj] = v;
                Vxxg[(size_t)nn * i + jj + n * ii] = v;
            }
        }
        for (int j = 63 - lane; j < n; j += 64) {                // Vx_i
            double s1 = 0.0, s2 = 0.0, s3 = 0.0;
#pragma unroll
            for (int q = 0; q < m; ++q) {
                s1 += Ks[q + m * j] * Quuks[q];
                s2 += Ks[q + m * j] * Qs[n + q];
                s3 += Quxs[q + m * j] * ks[q];
            }
            const double v = ((Qs[j] + s1) + s2) + s3;
            vs[j] = v;
            Vxg[(size_t)n * i + j] = v;
        }
        for (int e = lane; e < nm; e += 64) Kg[(size_t)nm * i + e] = Ks[e];
        if (lane < m) kg[(size_t)m * i + lane] = ks[lane];
        if (lane < mm) Quug[(size_t)mm * i + lane] = Quus[lane];
        // the prefetched operands of step i-1 into LDS (their last readers were P1 / P2)
        if (i > 0) {
#pragma unroll
            for (int r = 0; r < R1; ++r) {
                const int e = lane + 64 * r;
                if (e < n * p) Fs[e] = pfF[r];
            }
#pragma unroll
            for (int r = 0; r < RN; ++r) {
                const int e = lane + 64 * r;
                if (e < nn) cxxs[e] = pfxx[r];
            }
#pragma unroll
            for (int r = 0; r < RX; ++r) {
                const int e = lane + 64 * r;
                if (e < nm) cxus[e] = pfxu[r];
            }
            if (lane < mm) cuus[lane] = pfuu;
        }
        if (i > 0 && i == cc * TC) {                             // leaving chunk cc: publish cc-1, fetch cc-2
            double *nb = cbuf + ((cc - 1) & 1) * TC * CLEN;
#pragma unroll
            for (int r = 0; r < RC; ++r) {
                const int e = lane + 64 * r;
                if (e < TC * CLEN) nb[e] = pfc[r];
            }
            if (cc >= 2) {
#pragma unroll
                for (int r = 0; r < RC; ++r) {
                    const int e = lane + 64 * r;
                    if (e < TC * CLEN) pfc[r] = chunk_elem(cc - 2, e);
                }
            }
        }
        ddp_bp2_sync();
    }
    if (lane == n) { a.dV[2 * b] = dV0; a.dV[2 * b + 1] = dV1; }
    if (lane == 0) a.diverge[b] = diverge;
}

)DDPK";

static const char *kUserKernels2Vhess = R"DDPK(extern "C" __global__ __launch_bounds__(64) void ddp_user_vhess(UserVhessArgs a)
{
    constexpr int n = DDP_N, m = DDP_M, nz = DDP_NZ;
    const long total = (long)DDP_NPAIR * a.N * a.B, g = (long)blockIdx.x * 64 + threadIdx.x;
    if (g >= total) return;
    const int e = (int)(g % DDP_NPAIR);
    const long r = g / DDP_NPAIR;                                // (step, trajectory)
    const int b = (int)(r / a.N), i = (int)(r - (long)b * a.N);
    if (a.active && a.active[b] == 0) return;
    int pa, pb;
    ddp_tri(e, pa, pb);
    double x[n], u[m], v[n];
#pragma unroll
    for (int l = 0; l < n; ++l) { x[l] = a.x[(size_t)n * r + l]; v[l] = a.v[(size_t)n * r + l]; }
#pragma unroll
    for (int q = 0; q < m; ++q) u[q] = a.u[(size_t)m * r + q];
    const double hv = ddp_ad_vhess(x, u, i, ddp_params(a.params, a.params_batched, a.map, b), v, pa, pb);
    double *H = a.H + (size_t)nz * nz * r;
    H[pa + nz * pb] = hv;
    H[pb + nz * pa] = hv;
}
#endif
)DDPK";

// ---- DDP_USER_SECOND_ORDER_WAVE: full DDP at the shapes of DDP_USER_WAVE.  The program is that of a wave problem, then DDP_SECOND_ORDER 1,
// kUserAutodiffVhess, ddp_rsqrt + the text of boxqp_dev.h, kUserWidePrelude, the texts of wide_tile.h and back_pass_wide_kernel.h
// (written by build.py: one definition of the wide kernel's step, its Cholesky and its box-QP for both compilers), DDP_USER_ABI2 and
// DDP_USER_ABI3, kUserKernels2Head + Vhess, kUserKernels2Wave.
//
//   ddp_user_back_pass2_wave  back_pass_wide_body of back_pass_wide_kernel.h with n, m as constants: one work-group of four waves per
//                             trajectory, P1-P4 on v_mfma_f64_16x16x4, the step in a static LDS array (at most 160 KB, a static_assert).
//                             P0 in front of P1: the (n+m)(n+m+1)/2 pairs a <= b are dealt over the 256 threads, each thread calls
//                             ddp_ad_vhess for its pairs (every thread runs the model the same number of times, with a clamped pair
//                             where it has none: no thread leaves the phase early) and stores the value at (a, b) and (b, a) of the
//                             trajectory's [n+m, n+m] scratch in global memory (the step's LDS is full at (64, 32)); the barrier that
//                             ends P1 orders the stores before the reads of P2, which adds the entries to the cost Hessians where the
//                             accumulators start.  x_i, u_i are read from the caller's arrays, Vx_{i+1} from the LDS.
#define DDP_USER_ABI3                                                                                                                 \
    struct UserBp2WaveArgs {                                                                                                         \
        BPWArgs w;                                                                                                                   \
        const double *params, *x;                                                                                                    \
        double *H;                                                                                                                   \
        const int *map;                                                                                                              \
        int params_batched, pad_;                                                                                                    \
    };
#define DDP_USER_ABI3_TEXT DDP_USER_STR(DDP_USER_ABI3)

// what back_pass_wide_kernel.h and wide_tile.h take from ddp_internal.h and ddp_amd.h (which hiprtc cannot include)
#define DDP_USER_WIDE_PRELUDE_TEXT                                                                                                    \
    "\ntypedef int int32_t;\n#define DDP_MAX_M_WIDE " DDP_USER_STR(DDP_MAX_M_WIDE) "\n"                                               \
    "__device__ __forceinline__ void wave_sync()\n{\n"                                                                               \
    "    __builtin_amdgcn_fence(__ATOMIC_RELEASE, \"wavefront\");\n    __builtin_amdgcn_wave_barrier();\n"                           \
    "    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, \"wavefront\");\n}\n"
static const char *kUserWidePrelude = DDP_USER_WIDE_PRELUDE_TEXT;

static const char *kUserKernels2Wave = R"DDPK(
struct ddp_bp2_wave_curv {
#ifdef DDP_BP2_NO_CURVATURE                                   // (a source that defines it: the pass without P0, for bench/user_second_order_wave.py)
    static constexpr bool on = false;
#else
    static constexpr bool on = true;
#endif
    double *H;                                                   // [n+m, n+m] of this trajectory
    const double *x, *u, *pp;                                    // x[n, N], u[m, N] of this trajectory, its parameters
    __device__ __forceinline__ void p0(int i, const double *vs, int t) const
    {
        constexpr int n = DDP_N, m = DDP_M, p = DDP_NZ;
#pragma unroll 1
        for (int e0 = 0; e0 < DDP_NPAIR; e0 += 256) {            // one call site: (a, b) and (b, a) are one number
            const int e = e0 + t;
            const bool mine = e < DDP_NPAIR;
            int pa, pb;
            ddp_tri(mine ? e : 0, pa, pb);
            const double hv = ddp_ad_vhess(x + (size_t)n * i, u + (size_t)m * i, i, pp, vs, pa, pb);
            if (mine) {
                H[pa + p * pb] = hv;
                H[pb + p * pa] = hv;
            }
        }
    }
    __device__ __forceinline__ double h(int a, int b) const { return H[a + DDP_NZ * b]; }
};

extern "C" __global__ __launch_bounds__(256) void ddp_user_back_pass2_wave(UserBp2WaveArgs a)
{
    constexpr int n = DDP_N, m = DDP_M;
    constexpr WLds L(n, m);
    static_assert(L.total * 8 <= 160 * 1024, "ddp_user_back_pass2_wave: the step does not fit 160 KB of LDS");
    __shared__ double lds[L.total];
    const int b = blockIdx.x;
    ddp_bp2_wave_curv c;
    c.H = a.H + (size_t)DDP_NZ * DDP_NZ * b;
    c.x = a.x + (size_t)n * a.w.N * b;
    c.u = a.w.u + (size_t)m * a.w.N * b;
    c.pp = ddp_params(a.params, a.params_batched, a.map, b);
    back_pass_wide_body<false, n, m>(a.w, lds, c);
}
)DDPK";

// ---- DDP_USER_CLOCK: absolute time for the user's functions.  Every trajectory (every slot of the scheduler) has a clock c, an int, and
// dynamics, stage_cost, derivatives and terminal_cost take the absolute step t = c + i behind i (include/ddp_amd.h).  The texts above and
// those of user_autodiff.h are compiled byte for byte by every problem without the flag (the tests pin them), so their call sites carry
// no macro: the program of a clocked problem is made from the SAME texts by with_clock() (user_problem.hip), which
//   - puts DDP_T(i) behind the third argument of every call of dynamics, stage_cost, derivatives / DDP_DERIVATIVES and of the
//     ddp_ad_* chain (`int ddp_t` where the third argument is the declaration `int i`), and DDP_T(N - 1) behind the first of terminal_cost;
//   - wraps the third argument of plant in DDP_PLANT_T;
//   - reads the clock once per kernel, behind the line that takes the slot's parameters: const int ddp_c = ddp_clock(a.clk, b).
// A call that it misses does not compile (the user's functions take one argument more), so no kernel can run on the horizon index
// alone by accident.  There is one definition of every kernel.
static const char *kUserClockAd = "\n#define DDP_T(i) ddp_t\n";      // inside ddp_ad_*: the chain works on ONE step and carries its t
static const char *kUserClockKernels = R"DDPK(
#undef DDP_T
#define DDP_T(i) (ddp_c + (i))                                // in a kernel: ddp_c is the clock of the slot or trajectory b it works on
#define DDP_PLANT_T(t) (ddp_clock(a.clk, j) + (t))            // ddp_user_plant: t0 of trajectory j + the closed-loop step
__device__ __forceinline__ int ddp_clock(const int *clk, int b) { return clk ? clk[b] : 0; }
)DDPK";
