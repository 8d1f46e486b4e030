// user_sample_kernels.h — DDP_USER_SAMPLE: sampled closed-loop rollouts of a Gaussian policy, appended to the program of a problem with
// the flag only (a problem without it compiles the text it always did, not a byte more).  The program then ends in: DDP_SLANES,
// DDP_SCHUNK (user_problem.hip, layout_of), the text of philox.h (kPhiloxText, written by build.py: one definition of the generator for
// both compilers), DDP_USER_ABI_SAMPLE and kUserKernelsSample.
//
//   ddp_user_sample   one lane per sample, DDP_SLANES samples per 64-lane work-group, and every lane of a work-group works on the SAME
//                     trajectory b: the operands of DDP_SCHUNK steps — u_i, x_i, K_i and the noise factor L_i (lower Cholesky of Σ_i,
//                     ddp_policy_factor) — are brought into LDS once per work-group and read by all lanes at the same address
//                     (broadcast reads: K_i is read from memory once per 64 samples, not once per sample).  The state stays in VGPRs.
//                     Step i, forward_pass.jl:17-28 with the noise of iLQGkl's docstring:
//                         û = u_i + L_i ξ_i + K_i diff(x̂, x_i), clamp to lims, c_i = stage_cost(x̂, û, i, p),
//                         x̂ <- dynamics(x̂, û, i, p) for i < N-1 — or plant(x̂, û, i, p) when the call asks for the plant.
//                     ξ_i comes from ddp_normal_pair (philox.h) inside the kernel — there is no noise array in memory — or, when the
//                     caller gives one, from noise[m,N,S,B], staged through the lane's û slot.  Σ_c L_i[:,c] ξ_i[c] runs over the columns
//                     c = 0..m-1 in that order.  x̂, û and c of a chunk leave through LDS as one contiguous run per sample and stream,
//                     as ddp_roll_store does (one 8-byte element per lane and step tops out at ~1.8 TB/s,
//                     profiles/r06_narrow_streams.txt).  A trajectory whose status is not 0 (Σ_i not positive definite) runs no
//                     rollout: its rows of every output are NaN.
#pragma once

// only int / pointer / double members (as DDP_USER_ABI); the two seed words travel as int
#define DDP_USER_ABI_SAMPLE                                                                                                           \
    struct UserSampleArgs {                                                                                                          \
        int N, B, S, has_lims, params_batched, use_plant, sample0, traj0, seed_lo, seed_hi;                                          \
        const double *params, *K, *L, *x0, *u, *x, *lims, *noise;                                                                    \
        const int *status;                                                                                                           \
        double *xs, *us, *cs, *csum;                                                                                                 \
    };
#define DDP_USER_ABI_SAMPLE_TEXT DDP_USER_STR(DDP_USER_ABI_SAMPLE)

static const char *kUserKernelsSample = R"DDPK(
#define DDP_SOPS (DDP_M + DDP_N + DDP_M * DDP_N + DDP_M * DDP_M)   // doubles per step of the shared operands in LDS: u, x, K, L
#define DDP_SOS (DDP_N + DDP_M + 1)                           // doubles per step and sample of the results in LDS: x̂, û, c
#define DDP_SSS ((DDP_SCHUNK * DDP_SOS) | 1)                  // per-sample stride (odd: 8-byte accesses of a wave spread over the banks)

// chunk [i0, i0 + cs) of one operand stream of trajectory b (W doubles per step) into the work-group's shared slots
template <int W, int OFF>
__device__ __forceinline__ void ddp_sample_load(double *ops, const double *src, int N, int b, int i0, int cs, int lane)
{
    const double *s0 = src + (size_t)W * ((size_t)N * b + i0);
    for (int g = lane; g < W * cs; g += 64) {
        const int s = g / W, e = g - s * W;
        ops[s * DDP_SOPS + OFF + e] = s0[g];
    }
}

// the same chunk of the caller's noise (m doubles per step, one run per sample) into the û slots of the samples
__device__ __forceinline__ void ddp_sample_load_noise(double *out, const double *noise, int N, size_t rho0, int nvalid, int i0, int cs, int lane)
{
    constexpr int W = DDP_M, RUN = W * DDP_SCHUNK;
    for (int g = lane; g < DDP_SLANES * RUN; g += 64) {
        const int t = g / RUN, r = g - t * RUN, s = r / W, e = r - s * W;
        if (t < nvalid && s < cs) out[t * DDP_SSS + s * DDP_SOS + DDP_N + e] = noise[(size_t)W * N * (rho0 + t) + (size_t)W * i0 + r];
    }
}

// chunk [i0, i0 + cs) of one result stream (W doubles per step, `per` doubles per sample in memory) from LDS to the samples' rows
template <int W, int OFF>
__device__ __forceinline__ void ddp_sample_store(const double *out, double *dst, size_t per, size_t rho0, int nvalid, int i0, int cs, int lane)
{
    if (!dst) return;
    constexpr int RUN = W * DDP_SCHUNK;
    for (int g = lane; g < DDP_SLANES * RUN; g += 64) {
        const int t = g / RUN, r = g - t * RUN, s = r / W, e = r - s * W;
        if (t < nvalid && s < cs) dst[per * (rho0 + t) + (size_t)W * i0 + r] = out[t * DDP_SSS + s * DDP_SOS + OFF + e];
    }
}

extern "C" __global__ __launch_bounds__(64) void ddp_user_sample(UserSampleArgs a)
{
    constexpr int n = DDP_N, m = DDP_M, OU = 0, OX = DDP_M, OK = DDP_M + DDP_N, OL = DDP_M + DDP_N + DDP_M * DDP_N;
    constexpr int RX = 0, RU = DDP_N, RC = DDP_N + DDP_M;
    static_assert((DDP_SLANES * DDP_SSS + DDP_SCHUNK * DDP_SOPS) * 8 <= 64 * 1024, "ddp_user_sample: the chunk does not fit 64 KB of LDS");
    static_assert(DDP_SLANES >= 1 && DDP_SLANES <= 64 && DDP_SCHUNK >= 1, "ddp_user_sample: layout");
    __shared__ double out[DDP_SLANES * DDP_SSS];
    __shared__ double ops[DDP_SCHUNK * DDP_SOPS];
    const int lane = threadIdx.x, N = a.N, S = a.S, CL = DDP_TERMINAL ? N + 1 : N;
    const int groups = (S + DDP_SLANES - 1) / DDP_SLANES;
    const int b = (int)(blockIdx.x / (unsigned)groups), s0 = (int)(blockIdx.x - (unsigned)b * (unsigned)groups) * DDP_SLANES;
    if (b >= a.B) return;
    const int nvalid = S - s0 < DDP_SLANES ? S - s0 : DDP_SLANES;
    const bool mine = lane < nvalid;
    const size_t rho0 = (size_t)S * b + s0, rho = rho0 + lane;    // the sample's row of xs, us, cs, csum
    const bool bad = a.status[b] != 0;                            // (the same for every lane of the work-group)
    const bool act = mine && !bad;
    const bool has_noise = a.L != nullptr;
    const double *p = ddp_params(a.params, a.params_batched, nullptr, b);
    const unsigned seed_lo = (unsigned)a.seed_lo, seed_hi = (unsigned)a.seed_hi;
    const int sg = a.sample0 + s0 + lane, bg = a.traj0 + b;       // the sample and trajectory the generator counts
    const double nan = __builtin_nan("");
    double xh[n], lo[m], hi[m];
#pragma unroll
    for (int l = 0; l < n; ++l) xh[l] = act ? a.x0[(size_t)n * b + l] : 0.0;
#pragma unroll
    for (int q = 0; q < m; ++q) { lo[q] = a.has_lims ? a.lims[q] : 0.0; hi[q] = a.has_lims ? a.lims[q + m] : 0.0; }
    double csum = 0.0;
    for (int i0 = 0; i0 < N; i0 += DDP_SCHUNK) {
        const int cs = N - i0 < DDP_SCHUNK ? N - i0 : DDP_SCHUNK;
        if (!bad) {
            ddp_sample_load<m, OU>(ops, a.u, N, b, i0, cs, lane);
            ddp_sample_load<n, OX>(ops, a.x, N, b, i0, cs, lane);
            ddp_sample_load<m * n, OK>(ops, a.K, N, b, i0, cs, lane);
            if (has_noise) {
                ddp_sample_load<m * m, OL>(ops, a.L, N, b, i0, cs, lane);
                if (a.noise) ddp_sample_load_noise(out, a.noise, N, rho0, nvalid, i0, cs, lane);
            }
        }
        ddp_wave_sync();
        if (mine && bad) {
            for (int s = 0; s < cs; ++s)
                for (int e = 0; e < DDP_SOS; ++e) out[lane * DDP_SSS + s * DDP_SOS + e] = nan;
        }
        if (act) {
            for (int s = 0; s < cs; ++s) {
                const int i = i0 + s;
                const double *O = ops + s * DDP_SOPS;
                double *R = out + lane * DDP_SSS + s * DDP_SOS;
                double uu[m];
#pragma unroll
                for (int q = 0; q < m; ++q) uu[q] = O[OU + q];
                if (has_noise) {                               // u_i + L_i ξ_i, columns in order
                    double xi[m];
                    if (a.noise) {
#pragma unroll
                        for (int q = 0; q < m; ++q) xi[q] = R[RU + q];
                    } else {
#pragma unroll
                        for (int q2 = 0; q2 < (m + 1) / 2; ++q2) {
                            double z0, z1;
                            ddp_normal_pair(seed_lo, seed_hi, i, sg, bg, q2, z0, z1);
                            xi[2 * q2] = z0;
                            if (2 * q2 + 1 < m) xi[2 * q2 + 1] = z1;
                        }
                    }
#pragma unroll
                    for (int q = 0; q < m; ++q) {
                        double s1 = 0.0;
#pragma unroll
                        for (int c = 0; c < m; ++c) s1 += O[OL + q + m * c] * xi[c];
                        uu[q] += s1;
                    }
                }
                {                                              // forward_pass.jl:19: unew += K diff(x̂, x)
                    double dx[n];
#pragma unroll
                    for (int l = 0; l < n; ++l) {
                        double d = xh[l] - O[OX + l];
                        if ((DDP_WRAP >> l) & 1u) d = ddp_wrap_pi(d);
                        dx[l] = d;
                    }
#pragma unroll
                    for (int q = 0; q < m; ++q) {
                        double s2 = 0.0;
#pragma unroll
                        for (int l = 0; l < n; ++l) s2 += O[OK + q + m * l] * dx[l];
                        uu[q] += s2;
                    }
                }
                if (a.has_lims) {                              // :22-24
#pragma unroll
                    for (int q = 0; q < m; ++q) uu[q] = uu[q] > hi[q] ? hi[q] : (uu[q] < lo[q] ? lo[q] : uu[q]);
                }
                const double c = stage_cost(xh, uu, i, p);
                csum += c;
#pragma unroll
                for (int l = 0; l < n; ++l) R[RX + l] = xh[l];
#pragma unroll
                for (int q = 0; q < m; ++q) R[RU + q] = uu[q];
                R[RC] = c;
                if (i < N - 1) {                               // :25-28 (the successor of the last step is not stored)
                    double xn[n];
#if DDP_PLANT
                    if (a.use_plant) plant(xh, uu, i, p, xn);
                    else dynamics(xh, uu, i, p, xn);
#else
                    dynamics(xh, uu, i, p, xn);
#endif
#pragma unroll
                    for (int l = 0; l < n; ++l) xh[l] = xn[l];
                }
            }
        }
        ddp_wave_sync();
        ddp_sample_store<n, RX>(out, a.xs, (size_t)n * N, rho0, nvalid, i0, cs, lane);
        ddp_sample_store<m, RU>(out, a.us, (size_t)m * N, rho0, nvalid, i0, cs, lane);
        ddp_sample_store<1, RC>(out, a.cs, (size_t)CL, rho0, nvalid, i0, cs, lane);
        ddp_wave_sync();
    }
#if DDP_TERMINAL
    if (mine) {
        const double c = bad ? nan : terminal_cost(xh, p);
        a.cs[(size_t)CL * rho + N] = c;
        csum += c;
    }
#endif
    if (mine) a.csum[rho] = bad ? nan : csum;
}
)DDPK";
