// user_fitted_kernels.h — DDP_USER_FITTED: the rollout of a user problem on a fitted time-varying affine model, appended to the program
// of a problem with the flag only (a problem without it compiles the text it always did, not a byte more).  The program then ends in:
// DDP_FLANES, DDP_FCHUNK (user_problem.hip, layout_of), DDP_USER_ABI_FIT and kUserKernelsFit.  The tail goes last, behind the tail of
// DDP_USER_SAMPLE.
//
//   ddp_user_rollout_fit   the contract of ddp_user_rollout (operands, active, map, nalpha, lims, has_policy, fused csum, DDP_WRAP in the
//                          policy term, the terminal cost) with one difference, the successor state:
//                              û_i = clamp(u_i + α k_i + K_i diff(x̂_i, x_i)),   c_i = stage_cost(x̂_i, û_i, i, p)   (the user's cost)
//                              x̂_{i+1} = fc_i + Σ_j fx_i[:, j] x̂_i[j] + Σ_q fu_i[:, q] û_i[q]                      for i < N - 1
//                          on the tables fit_dynamics returns: fx[n,n,N,B], fu[n,m,N,B], fc[n,N,B], column-major, indexed by trajectory
//                          (through `map` where one is given).  The affine map acts on raw coordinates.  Slot N - 1 of the tables is
//                          neither loaded nor read.
//                          One lane per (trajectory, α) rollout, DDP_FLANES rollouts per 64-lane work-group, the state in VGPRs.  The
//                          tables of DDP_FCHUNK steps are staged through LDS as ddp_roll_load stages K: a trajectory's chunk of fx is
//                          n·n·DDP_FCHUNK doubles back to back in memory and the lanes of the wave read it as one contiguous run (a lane
//                          that walked its own steps would issue one 8-byte access per lane and step, the pattern that tops out at
//                          ~1.8 TB/s, profiles/r06_narrow_streams.txt).  The rollouts of a work-group are rho0 + t with trajectory
//                          (rho0 + t) % B, so with B < DDP_FLANES the lanes t, t + B, t + 2B, ... are the α candidates of ONE trajectory:
//                          they share table slot t % B — the tables are read from memory once and from LDS at one address (a broadcast).
//                          Per component l the sum runs fc, then j = 0..n-1, then q = 0..m-1: fixed by (l, j, q) alone, whatever B,
//                          nalpha or the launch geometry are.
#pragma once

// only int / pointer / double members (as DDP_USER_ABI): UserRollArgs without the clock, then the three tables
#define DDP_USER_ABI_FIT                                                                                                              \
    struct UserRollFitArgs {                                                                                                         \
        int N, B, nalpha, has_policy, has_lims, params_batched;                                                                       \
        const double *params, *K, *k, *x0, *u, *x, *lims;                                                                            \
        const int *active, *map;                                                                                                     \
        double *xnew, *unew, *cnew, *csum;                                                                                           \
        double alpha[16];                                                                                                            \
        const double *fx, *fu, *fc;                                                                                                  \
    };
#define DDP_USER_ABI_FIT_TEXT DDP_USER_STR(DDP_USER_ABI_FIT)

static const char *kUserKernelsFit = R"DDPK(
#define DDP_FTS (DDP_N * DDP_N + DDP_N * DDP_M + DDP_N)       // doubles per step of the tables in LDS: fx, fu, fc
#define DDP_FTR ((DDP_FCHUNK * DDP_FTS) | 1)                  // per-slot stride of the tables (odd: the lanes' reads spread over the banks)
#define DDP_FRS ((DDP_FCHUNK * DDP_PS) | 1)                   // per-rollout stride of u, x, k, K (DDP_PS doubles per step)

// chunk [i0, i0 + cs) of one stream (W doubles per step) of the first `nslot` slots into LDS; idx[t]: the trajectory of slot t, -1: none
template <int W, int OFF, int PSTEP, int STRIDE>
__device__ __forceinline__ void ddp_fit_load(double *lds, const int *idx, int nslot, const double *src, int N, int i0, int cs, int lane)
{
    constexpr int RUN = W * DDP_FCHUNK, U = 8;
    // U loads are issued before the first of them is waited for: a loop of load -> LDS store would pay one round trip to memory per
    // 64 elements (the loop-header s_waitcnt vmcnt(0) of DESIGN §9.1)
    for (int g0 = lane; g0 < nslot * RUN; g0 += 64 * U) {
        double v[U];
        int at[U];
#pragma unroll
        for (int c = 0; c < U; ++c) {
            const int g = g0 + 64 * c;
            at[c] = -1;
            v[c] = 0.0;
            if (g < nslot * RUN) {
                const int t = g / RUN, r = g - t * RUN, s = r / W, e = r - s * W;
                const int bt = idx[t];
                if (bt >= 0 && s < cs) {
                    at[c] = t * STRIDE + s * PSTEP + OFF + e;
                    v[c] = src[(size_t)W * N * bt + (size_t)W * i0 + r];
                }
            }
        }
#pragma unroll
        for (int c = 0; c < U; ++c)
            if (at[c] >= 0) lds[at[c]] = v[c];
    }
}

// the same chunk of one result stream (W doubles per step, `per` doubles per rollout in memory) from LDS to the rollouts' rows
template <int W, int OFF>
__device__ __forceinline__ void ddp_fit_store(const double *lds, const int *rb, double *dst, size_t per, long rho0, int i0, int cs, int lane)
{
    constexpr int RUN = W * DDP_FCHUNK;
    for (int g = lane; g < DDP_FLANES * RUN; g += 64) {
        const int t = g / RUN, r = g - t * RUN, s = r / W, e = r - s * W;
        if (rb[t] >= 0 && s < cs) dst[per * (size_t)(rho0 + t) + (size_t)W * i0 + r] = lds[t * DDP_FRS + s * DDP_PS + OFF + e];
    }
}

extern "C" __global__ __launch_bounds__(64) void ddp_user_rollout_fit(UserRollFitArgs a)
{
    constexpr int n = DDP_N, m = DDP_M, OU = 0, OX = DDP_M, OK = DDP_M + DDP_N, OKK = 2 * DDP_M + DDP_N;
    constexpr int TFX = 0, TFU = DDP_N * DDP_N, TFC = DDP_N * DDP_N + DDP_N * DDP_M;
    static_assert(DDP_FLANES >= 1 && DDP_FLANES <= 64 && DDP_FCHUNK >= 1, "ddp_user_rollout_fit: layout");
    static_assert(DDP_FLANES * (DDP_FRS + DDP_FTR + 1) * 8 <= 64 * 1024, "ddp_user_rollout_fit: the chunk does not fit 64 KB of LDS");
    __shared__ double lds[DDP_FLANES * DDP_FRS];
    __shared__ double tab[DDP_FLANES * DDP_FTR];
    __shared__ int rb[DDP_FLANES];                            // trajectory of each rollout of the work-group, -1: nothing to do
    __shared__ int tb[DDP_FLANES];                            // trajectory whose tables sit in each table slot, -1: none
    const int lane = threadIdx.x, N = a.N, B = a.B, CL = DDP_TERMINAL ? N + 1 : N;
    const long total = (long)B * a.nalpha, rho0 = (long)blockIdx.x * DDP_FLANES, rho = rho0 + lane;
    const bool mine = lane < DDP_FLANES && rho < total;
    const int b = mine ? (int)(rho % B) : 0, ai = mine ? (int)(rho / B) : 0;
    const int tj = mine ? (a.map ? a.map[b] : b) : -1;          // the trajectory the tables are indexed by
    const bool act = mine && tj >= 0 && !(a.active && a.active[b] == 0);
    // the rollouts t, t + B, ... of the work-group are the α candidates of one trajectory: one table slot for all of them.  Lane t < nts
    // is the first of its slot (the smallest rho), so it is active whenever one of them is
    const int nts = B < DDP_FLANES ? B : DDP_FLANES, ts = lane % nts;
    if (lane < DDP_FLANES) rb[lane] = act ? b : -1;
    if (lane < nts) tb[lane] = act ? tj : -1;
    const double alpha = a.alpha[ai];
    const double *p = ddp_params(a.params, a.params_batched, a.map, b);
    double xh[n], lo[m], hi[m];
#pragma unroll
    for (int l = 0; l < n; ++l) xh[l] = act ? a.x0[(size_t)n * b + l] : 0.0;
#pragma unroll
    for (int q = 0; q < m; ++q) { lo[q] = a.has_lims ? a.lims[q] : 0.0; hi[q] = a.has_lims ? a.lims[q + m] : 0.0; }
    double csum = 0.0;
    ddp_wave_sync();
    for (int i0 = 0; i0 < N; i0 += DDP_FCHUNK) {
        const int cs = N - i0 < DDP_FCHUNK ? N - i0 : DDP_FCHUNK;
        const int ct = N - 1 - i0 < cs ? N - 1 - i0 : cs;      // steps of the chunk that have a successor: slot N - 1 of the tables stays in memory
        ddp_fit_load<m, OU, DDP_PS, DDP_FRS>(lds, rb, DDP_FLANES, a.u, N, i0, cs, lane);
        if (a.has_policy) {
            ddp_fit_load<n, OX, DDP_PS, DDP_FRS>(lds, rb, DDP_FLANES, a.x, N, i0, cs, lane);
            ddp_fit_load<m, OK, DDP_PS, DDP_FRS>(lds, rb, DDP_FLANES, a.k, N, i0, cs, lane);
            ddp_fit_load<m * n, OKK, DDP_PS, DDP_FRS>(lds, rb, DDP_FLANES, a.K, N, i0, cs, lane);
        }
        ddp_fit_load<n * n, TFX, DDP_FTS, DDP_FTR>(tab, tb, nts, a.fx, N, i0, ct, lane);
        ddp_fit_load<n * m, TFU, DDP_FTS, DDP_FTR>(tab, tb, nts, a.fu, N, i0, ct, lane);
        ddp_fit_load<n, TFC, DDP_FTS, DDP_FTR>(tab, tb, nts, a.fc, N, i0, ct, lane);
        ddp_wave_sync();
        if (act) {
            for (int s = 0; s < cs; ++s) {
                const int i = i0 + s;
                double *L = lds + lane * DDP_FRS + s * DDP_PS;
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
                // x̂_i, û_i go to their result slots first and the user's cost reads them there: a cost that walks x in a loop the
                // compiler does not unroll (lq at n = 32) indexes LDS, not a register array that would have to live in scratch
#pragma unroll
                for (int q = 0; q < m; ++q) L[OU + q] = uu[q];
#pragma unroll
                for (int l = 0; l < n; ++l) L[OX + l] = xh[l];
                const double c = stage_cost(L + OX, L + OU, i, p);
                csum += c;
                L[OK] = c;
                if (i < N - 1) {                               // the fitted model in place of `dynamics`, on raw coordinates
                    const double *T = tab + ts * DDP_FTR + s * DDP_FTS;
                    double xn[n];
#pragma unroll
                    for (int l = 0; l < n; ++l) xn[l] = T[TFC + l];
#pragma unroll
                    for (int j = 0; j < n; ++j) {              // column by column: per component the order is fc, j = 0..n-1, q = 0..m-1
#pragma unroll
                        for (int l = 0; l < n; ++l) xn[l] += T[TFX + l + n * j] * xh[j];
                    }
#pragma unroll
                    for (int q = 0; q < m; ++q) {
#pragma unroll
                        for (int l = 0; l < n; ++l) xn[l] += T[TFU + l + n * q] * uu[q];
                    }
#pragma unroll
                    for (int l = 0; l < n; ++l) xh[l] = xn[l];
                }
            }
        }
        ddp_wave_sync();
        ddp_fit_store<n, OX>(lds, rb, a.xnew, (size_t)n * N, rho0, i0, cs, lane);
        ddp_fit_store<m, OU>(lds, rb, a.unew, (size_t)m * N, rho0, i0, cs, lane);
        ddp_fit_store<1, OK>(lds, rb, a.cnew, (size_t)CL, rho0, i0, cs, lane);
        ddp_wave_sync();
    }
#if DDP_TERMINAL
    if (act) {
        double *L = lds + lane * DDP_FRS;                      // (the lane's own slot: its results have left)
#pragma unroll
        for (int l = 0; l < n; ++l) L[l] = xh[l];
        const double c = terminal_cost(L, p);
        a.cnew[(size_t)CL * rho + N] = c;
        csum += c;
    }
#endif
    if (act) a.csum[rho] = csum;
}
)DDPK";
