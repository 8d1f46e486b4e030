// user_fitted_wave_kernels.h — DDP_USER_FITTED_WAVE: the rollout of a large user problem (n <= 64, m <= 32) on a fitted time-varying affine
// model, appended last to the program of a problem with the flag only (a problem without it compiles the text it always did, not a byte
// more).  The program then ends in: DDP_USER_ABI_FIT (user_fitted_kernels.h: UserRollFitArgs, unchanged) and kUserKernelsFitWave, behind
// the tail of DDP_USER_SAMPLE_WAVE.
//
//   ddp_user_rollout_fit_wave  the contract of ddp_user_rollout_fit (user_fitted_kernels.h: operands, active, map, nalpha, lims,
//                              has_policy, fused csum, DDP_WRAP in the policy term, the terminal cost, slot N - 1 of the tables neither
//                              loaded nor read) in the layout of ddp_user_rollout_wave: a group of DDP_WG lanes (8, 16 or 32: the power
//                              of two >= m) per (trajectory, α) rollout, 64 / DDP_WG rollouts per one-wave work-group.  x̂, diff(x̂, x)
//                              and û of a rollout live in LDS (2n + m doubles at an odd stride); no lane holds an array of n or n·n
//                              doubles of the library's own.  Step i:
//                                  lanes l = q, q + WG, ...   x̂_l leaves, dx_l = diff(x̂, x_i)_l
//                                  lane q < m                 û_q = clamp(u_q + α k_q + Σ_l K_i[q,l] dx_l), streaming row q of K_i
//                                  lanes l = q, q + WG, ...   x̂⁺_l = fc_i[l], then + fx_i[l,j] x̂_j (j = 0..n-1), then + fu_i[l,c] û_c
//                                                             (c = 0..m-1): the order of ddp_user_rollout_fit, fixed by (l, j, c)
//                                                             alone; the ceil(n / WG) sums of a lane run side by side in registers
//                                  lane 0                     c_i = stage_cost(x̂, û, i, p)
//                              The tables are column-major, so the lanes of a group read consecutive doubles of every column, and the
//                              loads of a column do not wait for the state: the unrolled loop keeps several columns in flight.  The
//                              rollouts of a work-group are rho0 + g with trajectory (rho0 + g) % B: with B < 64 / DDP_WG the groups of
//                              a work-group are α candidates of the same trajectories and read the same addresses in the same
//                              instruction.  The successor state goes to LDS behind the cost: no copy of x̂⁺ in LDS, three barriers a step.
#pragma once

static const char *kUserKernelsFitWave = R"DDPF(
#define DDP_FWS ((2 * DDP_N + DDP_M) | 1)                      // doubles per rollout in LDS: x̂, dx, û (odd stride)

extern "C" __global__ __launch_bounds__(64) void ddp_user_rollout_fit_wave(UserRollFitArgs a)
{
    constexpr int n = DDP_N, m = DDP_M, G = DDP_WG, RPW = 64 / G, R = (n + G - 1) / G;
    static_assert(G >= m && G <= 64 && (G & (G - 1)) == 0, "ddp_user_rollout_fit_wave: DDP_WG is a power of two >= m");
    static_assert(RPW * DDP_FWS * 8 <= 64 * 1024, "ddp_user_rollout_fit_wave: the rollouts of a work-group do not fit 64 KB of LDS");
    __shared__ double lds[RPW * DDP_FWS];
    const int lane = threadIdx.x, g = lane / G, q = lane - g * G, N = a.N, B = a.B, CL = DDP_TERMINAL ? N + 1 : N;
    const long total = (long)B * a.nalpha, rho = (long)blockIdx.x * RPW + g;
    const bool mine = rho < total;
    const int b = mine ? (int)(rho % B) : 0, ai = mine ? (int)(rho / B) : 0;
    const int tj = mine ? (a.map ? a.map[b] : b) : -1;           // the trajectory the tables are indexed by
    const bool act = mine && tj >= 0 && !(a.active && a.active[b] == 0);
    const bool lead = act && q == 0, ctl = act && q < m;
    const double alpha = a.alpha[ai];
    const double *p = ddp_params(a.params, a.params_batched, a.map, b);
    double *xh = lds + g * DDP_FWS, *dx = xh + n, *uu = dx + n;
    const double lo = (a.has_lims && q < m) ? a.lims[q] : 0.0, hi = (a.has_lims && q < m) ? a.lims[q + m] : 0.0;
    const double *ub = a.u + (size_t)m * N * b, *xb = a.x + (size_t)n * N * b, *kb = a.k + (size_t)m * N * b,
                 *Kb = a.K + (size_t)m * n * N * b;
    const size_t tt = act ? (size_t)tj : 0;
    const double *fxb = a.fx + (size_t)n * n * N * tt, *fub = a.fu + (size_t)n * m * N * tt, *fcb = a.fc + (size_t)n * N * tt;
    double *xo = a.xnew + (size_t)n * N * rho, *uo = a.unew + (size_t)m * N * rho, *co = a.cnew + (size_t)CL * rho;
    if (act)
        for (int l = q; l < n; l += G) xh[l] = a.x0[(size_t)n * b + l];
    int row[R];                                                  // the rows of [fc | fx | fu] of this lane, clamped to the last one
#pragma unroll
    for (int r = 0; r < R; ++r) row[r] = q + G * r < n ? q + G * r : n - 1;
    double csum = 0.0;
    ddp_wave_sync();
    for (int i = 0; i < N; ++i) {
        if (act) {
            for (int l = q; l < n; l += G) {
                const double xv = xh[l];
                xo[(size_t)n * i + l] = xv;
                if (a.has_policy) {                            // forward_pass.jl:17-20: unew += k α;  unew += K diff(x̂, x)
                    double d = xv - xb[(size_t)n * i + l];
                    if (l < 32 && ((DDP_WRAP >> l) & 1u)) d = ddp_wrap_pi(d);
                    dx[l] = d;
                }
            }
        }
        ddp_wave_sync();
        if (ctl) {
            double v = ub[(size_t)m * i + q];
            if (a.has_policy) {
                const double *Kr = Kb + (size_t)m * n * i + q;   // row q of K_i
                double s2 = 0.0;
                v += kb[(size_t)m * i + q] * alpha;
#pragma unroll 8
                for (int l = 0; l < n; ++l) s2 += Kr[m * l] * dx[l];
                v += s2;
            }
            if (a.has_lims) v = v > hi ? hi : (v < lo ? lo : v);   // :22-24
            uu[q] = v;
            uo[(size_t)m * i + q] = v;
        }
        ddp_wave_sync();
        // the fitted model in place of `dynamics`, on raw coordinates: rows q, q + G, ... of [fc | fx | fu] of step i (slot N - 1 stays in
        // memory); per row the sum runs fc, j = 0..n-1, c = 0..m-1.  A lane whose row q + G r lies past n takes row n - 1 once more and drops the sum: every lane issues every load and the
        // column loops hold no branch
        double xn[R];
        const bool succ = act && i < N - 1;
        if (succ) {
            const double *Fx = fxb + (size_t)n * n * i, *Fu = fub + (size_t)n * m * i, *Fc = fcb + (size_t)n * i;
#pragma unroll
            for (int r = 0; r < R; ++r) xn[r] = Fc[row[r]];
#pragma unroll 8
            for (int j = 0; j < n; ++j) {
                const double xj = xh[j];
#pragma unroll
                for (int r = 0; r < R; ++r) xn[r] += Fx[n * j + row[r]] * xj;
            }
#pragma unroll 8
            for (int c = 0; c < m; ++c) {
                const double uc = uu[c];
#pragma unroll
                for (int r = 0; r < R; ++r) xn[r] += Fu[n * c + row[r]] * uc;
            }
        }
        if (lead) {
            const double c = stage_cost(xh, uu, i, p);
            csum += c;
            co[i] = c;
        }
        ddp_wave_sync();
        // (no barrier behind this: the next step's first phase reads the rows this lane wrote, everything else waits for its barriers)
        if (succ) {
#pragma unroll
            for (int r = 0; r < R; ++r)
                if (q + G * r < n) xh[q + G * r] = xn[r];
        }
    }
    ddp_wave_sync();
    if (lead) {
#if DDP_TERMINAL
        const double c = terminal_cost(xh, p);
        co[N] = c;
        csum += c;
#endif
        a.csum[rho] = csum;
    }
}
)DDPF";
