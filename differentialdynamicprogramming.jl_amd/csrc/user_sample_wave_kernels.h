// user_sample_wave_kernels.h — DDP_USER_SAMPLE_WAVE: sampled closed-loop rollouts of a Gaussian policy at the shapes of DDP_USER_WAVE
// (n <= 64, m <= 32), appended last to the program of a problem with the flag only (a problem without it compiles the text it always
// did, not a byte more).  The program then ends in: the text of philox.h (kPhiloxText), DDP_USER_ABI_SAMPLE and kUserKernelsSampleWave.
//
//   ddp_user_sample_wave  the semantics of ddp_user_sample (user_sample_kernels.h), word for word, in the layout of ddp_user_rollout_wave:
//                         a group of DDP_WG lanes (8, 16 or 32: the power of two >= m) per sample, 64 / DDP_WG samples per one-wave
//                         work-group, and every group of a work-group works on the SAME trajectory b.  x̂, diff(x̂, x), the successor
//                         state, û and ξ of a sample live in LDS (3n + 2m doubles at an odd stride); no lane holds an array of n, m,
//                         m·n or m·m doubles of the library's own.  Step i:
//                             lanes l = q, q + WG, ...   x̂_l leaves, dx_l = diff(x̂, x_i)_l
//                             lane q2 < (m + 1) / 2      ξ_{2 q2}, ξ_{2 q2 + 1} = ddp_normal_pair(seed, i, sample0 + s, traj0 + b, q2) (the
//                                                        odd normal past m is dropped) — or lane q < m takes ξ_q from noise[m,N,S,B]
//                             lane q < m                 û_q = u_q, then + Σ_c L[q,c] ξ_c (c = 0..m-1 ascending from 0.0), then
//                                                        + Σ_l K[q,l] dx_l (l = 0..n-1 ascending from 0.0), then the clamp to lims:
//                                                        the order of ddp_user_sample
//                             lane 0                     c_i = stage_cost(x̂, û, i, p);  x̂⁺ = dynamics(...) or plant(...) for i < N-1
//                         K_i and L_i are never staged: lane q streams row q of K_i and of L_i from memory (both column-major, so the
//                         lanes of a group read m consecutive doubles per column), and the groups of a work-group read the same
//                         addresses in the same instruction — one trip to the cache per work-group, not per sample.  x̂, û and c leave
//                         as contiguous runs written by the group.  A trajectory whose status is not 0 runs no rollout: its rows of every
//                         output are NaN.  Nothing depends on S, B or the launch geometry.
#pragma once

static const char *kUserKernelsSampleWave = R"DDPS(
#define DDP_SWS ((3 * DDP_N + 2 * DDP_M) | 1)                 // doubles per sample in LDS: x̂, dx, x̂⁺, û, ξ (odd stride)

extern "C" __global__ __launch_bounds__(64) void ddp_user_sample_wave(UserSampleArgs a)
{
    constexpr int n = DDP_N, m = DDP_M, G = DDP_WG, SPW = 64 / G;
    static_assert(G >= m && G <= 64 && (G & (G - 1)) == 0, "ddp_user_sample_wave: DDP_WG is a power of two >= m");
    static_assert(SPW * DDP_SWS * 8 <= 64 * 1024, "ddp_user_sample_wave: the samples of a work-group do not fit 64 KB of LDS");
    __shared__ double lds[SPW * DDP_SWS];
    const int lane = threadIdx.x, g = lane / G, q = lane - g * G, N = a.N, S = a.S, CL = DDP_TERMINAL ? N + 1 : N;
    const int groups = (S + SPW - 1) / SPW;
    const int b = (int)(blockIdx.x / (unsigned)groups), s = (int)(blockIdx.x - (unsigned)b * (unsigned)groups) * SPW + g;
    if (b >= a.B) return;
    const bool mine = s < S;
    const size_t rho = (size_t)S * b + (mine ? s : 0);            // the sample's row of xs, us, cs, csum
    const bool bad = a.status[b] != 0;                            // (the same for every lane of the work-group)
    const bool act = mine && !bad, lead = act && q == 0, ctl = act && q < m;
    const bool has_noise = a.L != nullptr;
    const double *p = ddp_params(a.params, a.params_batched, nullptr, b);
    const unsigned seed_lo = (unsigned)a.seed_lo, seed_hi = (unsigned)a.seed_hi;
    const int sg = a.sample0 + s, bg = a.traj0 + b;               // the sample and trajectory the generator counts
    double *xh = lds + g * DDP_SWS, *dx = xh + n, *xn = dx + n, *uu = xn + n, *xi = uu + m;
    const double lo = (a.has_lims && q < m) ? a.lims[q] : 0.0, hi = (a.has_lims && q < m) ? a.lims[q + m] : 0.0;
    const double *ub = a.u + (size_t)m * N * b, *xb = a.x + (size_t)n * N * b, *Kb = a.K + (size_t)m * n * N * b,
                 *Lb = has_noise ? a.L + (size_t)m * m * N * b : nullptr, *zb = a.noise ? a.noise + (size_t)m * N * rho : nullptr;
    double *xo = a.xs ? a.xs + (size_t)n * N * rho : nullptr, *uo = a.us ? a.us + (size_t)m * N * rho : nullptr,
           *co = a.cs + (size_t)CL * rho;
    if (mine && bad) {                                            // no rollout: NaN rows, written by the group as contiguous runs
        const double nan = __builtin_nan("");
        if (xo) for (size_t e = q; e < (size_t)n * N; e += G) xo[e] = nan;
        if (uo) for (size_t e = q; e < (size_t)m * N; e += G) uo[e] = nan;
        for (int e = q; e < CL; e += G) co[e] = nan;
        if (q == 0) a.csum[rho] = nan;
    }
    if (bad) return;                                              // (wave-uniform)
    if (act)
        for (int l = q; l < n; l += G) xh[l] = a.x0[(size_t)n * b + l];
    double csum = 0.0;
    ddp_wave_sync();
    for (int i = 0; i < N; ++i) {
        if (act) {
            for (int l = q; l < n; l += G) {                      // forward_pass.jl:19: diff(x̂, x)
                const double xv = xh[l];
                if (xo) xo[(size_t)n * i + l] = xv;
                double d = xv - xb[(size_t)n * i + l];
                if (l < 32 && ((DDP_WRAP >> l) & 1u)) d = ddp_wrap_pi(d);
                dx[l] = d;
            }
            if (has_noise) {
                if (zb) {
                    if (q < m) xi[q] = zb[(size_t)m * i + q];
                } else if (q < (m + 1) / 2) {                     // the pairs of the step, one per lane
                    double z0, z1;
                    ddp_normal_pair(seed_lo, seed_hi, i, sg, bg, q, z0, z1);
                    xi[2 * q] = z0;
                    if (2 * q + 1 < m) xi[2 * q + 1] = z1;
                }
            }
        }
        ddp_wave_sync();
        if (ctl) {
            double v = ub[(size_t)m * i + q];
            if (has_noise) {                                      // u_i + L_i ξ_i, columns in order
                const double *Lr = Lb + (size_t)m * m * i + q;    // row q of L_i
                double s1 = 0.0;
#pragma unroll 8
                for (int c = 0; c < m; ++c) s1 += Lr[m * c] * xi[c];
                v += s1;
            }
            {
                const double *Kr = Kb + (size_t)m * n * i + q;    // row q of K_i
                double s2 = 0.0;
#pragma unroll 8
                for (int l = 0; l < n; ++l) s2 += Kr[m * l] * dx[l];
                v += s2;
            }
            if (a.has_lims) v = v > hi ? hi : (v < lo ? lo : v);   // :22-24
            uu[q] = v;
            if (uo) uo[(size_t)m * i + q] = v;
        }
        ddp_wave_sync();
        if (lead) {
            const double c = stage_cost(xh, uu, i, p);
            csum += c;
            co[i] = c;
            if (i < N - 1) {                                       // :25-28 (the successor of the last step is not stored)
#if DDP_PLANT
                if (a.use_plant) plant(xh, uu, i, p, xn);
                else dynamics(xh, uu, i, p, xn);
#else
                dynamics(xh, uu, i, p, xn);
#endif
            }
        }
        ddp_wave_sync();
        if (act && i < N - 1)
            for (int l = q; l < n; l += G) xh[l] = xn[l];
        ddp_wave_sync();
    }
    if (lead) {
#if DDP_TERMINAL
        const double c = terminal_cost(xh, p);
        co[N] = c;
        csum += c;
#endif
        a.csum[rho] = csum;
    }
}
)DDPS";
