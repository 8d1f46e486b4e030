// user_cost_fit_kernels.h — DDP_USER_COST_FIT: the quadratic cost model of a guided-policy-search round, fitted to the sampled rollouts the
// dynamics model is fitted to, appended to the program of a problem with the flag only (a problem without it compiles the text it always
// did, not a byte more).  The program then ends in: DDP_CLANES, DDP_CCHUNK, DDP_CSB (user_problem.hip, layout_of), DDP_USER_ABI_COST_FIT
// and kUserKernelsCostFit.  The tail goes last, behind the tail of DDP_USER_FITTED.
//
//   ddp_user_cost_fit   for every step i and trajectory b, over the samples s = 0..S-1 in that order, with δx = diff(x̂_s, x_i) (DDP_WRAP, the
//                       rollout's policy term), δu = û_s - u_i and (c, cx, cu, cxx, cxu, cuu) the user's cost and its derivatives at
//                       (x̂_s, û_s, i) — `derivatives`, forward-mode AD of the cost alone with DDP_AUTODIFF, `cost_hessians` with
//                       DDP_CONST_HESSIAN; at i = N-1 whatever `derivatives` adds there, and c = stage_cost + terminal_cost:
//                           hx[a] = Σ_j cxx[a,j] δx[j] + Σ_q cxu[a,q] δu[q]        hu[r] = Σ_j cxu[j,r] δx[j] + Σ_q cuu[r,q] δu[q]
//                           cxx_i += cxx,  cxu_i += cxu,  cuu_i += cuu,  cx_i[a] += cx[a] - hx[a],  cu_i[r] += cu[r] - hu[r]
//                           c0_i += (c - (Σ_j cx[j] δx[j] + Σ_q cu[q] δu[q])) + ½ (Σ_j δx[j] hx[j] + Σ_q δu[q] hu[q])
//                       (every Σ starts at 0 and runs j = 0..n-1, then q = 0..m-1), and every sum is divided by S when it is stored.
//                       One lane per (step, trajectory): a work-group takes DDP_CCHUNK consecutive steps of DDP_CLANES / DDP_CCHUNK
//                       trajectories.  A lane owns two LDS slots of n + m + n² + nm + m² doubles: `derivatives` writes one (as ddp_user_df's
//                       lane does), the other holds the running sums; no per-sample array exists in memory.  The samples of DDP_CSB
//                       sample indices are staged through LDS per round: for fixed (s, b) the DDP_CCHUNK steps of the work-group are one
//                       contiguous run of n·DDP_CCHUNK doubles of xs, and the lanes of the wave read it as such (a lane that fetched its
//                       own step of every sample would issue one 8-byte access per lane, n·N doubles apart).  The six outputs leave the
//                       same way, one contiguous run per trajectory and array.  The fx, fu `derivatives` writes go to lane-private
//                       arrays that are never read (the compiler drops the stores).  Nothing depends on S, B or the launch geometry:
//                       a lane sees its own (i, b) only, so a non-finite sample stays in its own outputs and a call on a slice of the
//                       trajectories gives that slice of the full call bit for bit.
#pragma once

// only int / pointer / double members (as DDP_USER_ABI)
#define DDP_USER_ABI_COST_FIT                                                                                                         \
    struct UserCostFitArgs {                                                                                                         \
        int N, S, B, params_batched;                                                                                                 \
        const double *params, *xs, *us, *x, *u;                                                                                      \
        double *cx, *cu, *cxx, *cxu, *cuu, *c0;                                                                                      \
    };
#define DDP_USER_ABI_COST_FIT_TEXT DDP_USER_STR(DDP_USER_ABI_COST_FIT)

static const char *kUserKernelsCostFit = R"DDPK(
#define DDP_CTRAJ (DDP_CLANES / DDP_CCHUNK)                   // trajectories per work-group
#define DDP_CDC (DDP_N + DDP_M + DDP_N * DDP_N + DDP_N * DDP_M + DDP_M * DDP_M)   // cx, cu, cxx, cxu, cuu
// per-lane stride (odd: the lanes' 8-byte accesses spread over the banks): derivatives, sums, c0, the nominal, DDP_CSB samples
#define DDP_CLS ((2 * DDP_CDC + 1 + (DDP_CSB + 1) * (DDP_N + DDP_M)) | 1)

// W doubles per step of the work-group's steps [i0, i0 + cs), for NSL sample slots per trajectory, into the lanes' slots at OFF (+ NZ per
// sample slot).  In memory the run of (trajectory b, sample index sidx) starts at W (i0 + N (sidx + smul b)) — the samples: sidx = s0 + sl,
// smul = S; the nominal: NSL = 1, sidx = 0, smul = 1.  tb[t]: the trajectory of slot t, -1: none
template <int W, int OFF, int NSL>
__device__ __forceinline__ void ddp_cf_load(double *lds, const int *tb, const double *src, int N, int smul, int s0, int sb, int i0, int cs, int lane)
{
    constexpr int RUN = W * DDP_CCHUNK, TOT = DDP_CTRAJ * NSL * RUN, U = 8, NZ = DDP_N + DDP_M;
    // U loads are issued before the first of them is waited for (ddp_fit_load)
    for (int g0 = lane; g0 < TOT; g0 += 64 * U) {
        double v[U];
        int at[U];
#pragma unroll
        for (int c = 0; c < U; ++c) {
            const int g = g0 + 64 * c;
            at[c] = -1;
            v[c] = 0.0;
            if (g < TOT) {
                const int t = g / (NSL * RUN), rem = g - t * (NSL * RUN), sl = rem / RUN, r = rem - sl * RUN, st = r / W, e = r - st * W;
                const int bt = tb[t];
                if (bt >= 0 && sl < sb && st < cs) {
                    at[c] = (t * DDP_CCHUNK + st) * DDP_CLS + OFF + sl * NZ + e;
                    v[c] = src[(size_t)W * ((size_t)i0 + (size_t)N * ((size_t)(s0 + sl) + (size_t)smul * bt)) + r];
                }
            }
        }
#pragma unroll
        for (int c = 0; c < U; ++c)
            if (at[c] >= 0) lds[at[c]] = v[c];
    }
}

// the sums of one output array (W doubles per step) of the work-group's steps, divided by S, to the rows of its trajectories
template <int W, int OFF>
__device__ __forceinline__ void ddp_cf_store(const double *lds, const int *tb, double *dst, int N, double S, int i0, int cs, int lane)
{
    constexpr int RUN = W * DDP_CCHUNK;
    for (int g = lane; g < DDP_CTRAJ * RUN; g += 64) {
        const int t = g / RUN, r = g - t * RUN, st = r / W, e = r - st * W;
        const int bt = tb[t];
        if (bt >= 0 && st < cs) dst[(size_t)W * ((size_t)i0 + (size_t)N * bt) + r] = lds[(t * DDP_CCHUNK + st) * DDP_CLS + OFF + e] / S;
    }
}

#if DDP_AUTODIFF && DDP_CONST_HESSIAN
// cx, cu alone by forward-mode AD of the cost (ddp_ad_jacobian also runs `dynamics`): directions C·DDP_ADJ ..
template <int C> DDP_AD_FN void ddp_cf_ad_gradient(const double *x, const double *u, int i, int N, const double *p, double *cx, double *cu)
{
    constexpr int n = DDP_N, m = DDP_M, Z0 = C * DDP_ADJ;
    if constexpr (Z0 < n + m) {
        typedef ddp_dual<double, DDP_ADJ> D;
        D xd[n], ud[m];
        ddp_ad_seed1<Z0>(x, u, xd, ud);
        DDP_AD_FRESH(p);
        D c = stage_cost(xd, ud, i, p);
#if DDP_TERMINAL
        if (Z0 < n && i == N - 1) c += terminal_cost(xd, p);
#endif
#pragma unroll
        for (int j = 0; j < DDP_ADJ; ++j) {
            const int z = Z0 + j;
            if (z >= n + m) break;
            if (z < n) cx[z] = c.d[j];
            else cu[z - n] = c.d[j];
        }
        ddp_cf_ad_gradient<C + 1>(x, u, i, N, p, cx, cu);
    }
}
#endif

extern "C" __global__ __launch_bounds__(64) void ddp_user_cost_fit(UserCostFitArgs a)
{
    constexpr int n = DDP_N, m = DDP_M, NZ = DDP_N + DDP_M;
    constexpr int OCX = 0, OCU = OCX + n, OXX = OCU + m, OXU = OXX + n * n, OUU = OXU + n * m, DC = DDP_CDC;
    constexpr int OD = 0, OA = DC, OC0 = 2 * DC, ON = OC0 + 1, OS = ON + NZ;
    static_assert(DDP_CCHUNK >= 1 && DDP_CSB >= 1 && DDP_CLANES >= DDP_CCHUNK && DDP_CLANES <= 64 && DDP_CLANES % DDP_CCHUNK == 0,
                  "ddp_user_cost_fit: layout");
    static_assert((DDP_CLANES * DDP_CLS + DDP_CTRAJ) * 8 <= 64 * 1024, "ddp_user_cost_fit: the lanes' slots do not fit 64 KB of LDS");
    __shared__ double lds[DDP_CLANES * DDP_CLS];
    __shared__ int tb[DDP_CTRAJ];                             // trajectory of each trajectory slot of the work-group, -1: none
    const int lane = threadIdx.x, N = a.N, S = a.S, B = a.B;
    const int nchunk = (N + DDP_CCHUNK - 1) / DDP_CCHUNK, ic = (int)(blockIdx.x % (unsigned)nchunk), ig = (int)(blockIdx.x / (unsigned)nchunk);
    const int i0 = ic * DDP_CCHUNK, cs = N - i0 < DDP_CCHUNK ? N - i0 : DDP_CCHUNK;
    const int ts = lane % DDP_CCHUNK, tt = lane / DDP_CCHUNK, i = i0 + ts;
    const long bl = (long)ig * DDP_CTRAJ + tt;
    const bool act = lane < DDP_CLANES && bl < B && ts < cs;
    const int b = act ? (int)bl : 0;
    if (lane < DDP_CTRAJ) tb[lane] = (long)ig * DDP_CTRAJ + lane < B ? ig * DDP_CTRAJ + lane : -1;
    double *L = lds + (act ? lane : 0) * DDP_CLS;              // (a lane without a pair touches no slot)
    const double *p = act ? ddp_params(a.params, a.params_batched, nullptr, b) : nullptr;
    ddp_wave_sync();
    ddp_cf_load<n, ON, 1>(lds, tb, a.x, N, 1, 0, 1, i0, cs, lane);
    ddp_cf_load<m, ON + n, 1>(lds, tb, a.u, N, 1, 0, 1, i0, cs, lane);
    if (act) {
        for (int e = 0; e < DC; ++e) L[OA + e] = 0.0;
#if DDP_CONST_HESSIAN
        cost_hessians(p, L + OD + OXX, L + OD + OXU, L + OD + OUU);     // the Hessians of every sample
#endif
    }
    double c0 = 0.0;
    for (int s0 = 0; s0 < S; s0 += DDP_CSB) {
        const int sb = S - s0 < DDP_CSB ? S - s0 : DDP_CSB;
        ddp_cf_load<n, OS, DDP_CSB>(lds, tb, a.xs, N, S, s0, sb, i0, cs, lane);
        ddp_cf_load<m, OS + n, DDP_CSB>(lds, tb, a.us, N, S, s0, sb, i0, cs, lane);
        ddp_wave_sync();
        if (act) {
            for (int sl = 0; sl < sb; ++sl) {
                double *Z = L + OS + sl * NZ;                  // x̂_s, û_s; below: δx, δu
                double *D = L + OD;
                // the user's functions read the sample in LDS: a cost that walks x in a loop the compiler does not unroll (lq at n = 32)
                // indexes LDS, not a register array that would have to live in scratch
#if DDP_AUTODIFF
#if DDP_CONST_HESSIAN
                ddp_cf_ad_gradient<0>(Z, Z + n, i, N, p, D + OCX, D + OCU);
#else
                const ddp_ad_out o = {nullptr, nullptr, D + OCX, D + OCU, D + OXX, D + OXU, D + OUU};
                ddp_ad_hessian<0, 0>(Z, Z + n, i, N, p, o);      // the cost alone: `dynamics` is not run
#endif
#else
                // fx, fu (with DDP_CONST_HESSIAN the Hessians too) of `derivatives` are not used: lane-private arrays that are never read
                double nfx[n * n], nfu[n * m];
#if DDP_CONST_HESSIAN
                double nxx[n * n], nxu[n * m], nuu[m * m];
                derivatives(Z, Z + n, i, N, p, nfx, nfu, D + OCX, D + OCU, nxx, nxu, nuu);
#else
                derivatives(Z, Z + n, i, N, p, nfx, nfu, D + OCX, D + OCU, D + OXX, D + OXU, D + OUU);
#endif
#endif
                double c = stage_cost(Z, Z + n, i, p);
#if DDP_TERMINAL
                if (i == N - 1) c += terminal_cost(Z, p);
#endif
                for (int l = 0; l < n; ++l) {
                    double d = Z[l] - L[ON + l];
                    if ((DDP_WRAP >> l) & 1u) d = ddp_wrap_pi(d);
                    Z[l] = d;
                }
                for (int q = 0; q < m; ++q) Z[n + q] -= L[ON + n + q];
                double lin = 0.0, quad = 0.0;
                for (int r = 0; r < n; ++r) {                  // row r of [cxx cxu] on [δx; δu]
                    double h = 0.0;
                    for (int j = 0; j < n; ++j) h += D[OXX + r + n * j] * Z[j];
                    for (int q = 0; q < m; ++q) h += D[OXU + r + n * q] * Z[n + q];
                    L[OA + OCX + r] += D[OCX + r] - h;
                    lin += D[OCX + r] * Z[r];
                    quad += Z[r] * h;
                }
                for (int r = 0; r < m; ++r) {                  // row r of [cxuᵀ cuu]
                    double h = 0.0;
                    for (int j = 0; j < n; ++j) h += D[OXU + j + n * r] * Z[j];
                    for (int q = 0; q < m; ++q) h += D[OUU + r + m * q] * Z[n + q];
                    L[OA + OCU + r] += D[OCU + r] - h;
                    lin += D[OCU + r] * Z[n + r];
                    quad += Z[n + r] * h;
                }
                for (int e = OXX; e < DC; ++e) L[OA + e] += D[e];
                c0 += (c - lin) + 0.5 * quad;
            }
        }
        ddp_wave_sync();
    }
    if (act) L[OC0] = c0;
    ddp_wave_sync();
    const double Sd = (double)S;
    ddp_cf_store<n, OA + OCX>(lds, tb, a.cx, N, Sd, i0, cs, lane);
    ddp_cf_store<m, OA + OCU>(lds, tb, a.cu, N, Sd, i0, cs, lane);
    ddp_cf_store<n * n, OA + OXX>(lds, tb, a.cxx, N, Sd, i0, cs, lane);
    ddp_cf_store<n * m, OA + OXU>(lds, tb, a.cxu, N, Sd, i0, cs, lane);
    ddp_cf_store<m * m, OA + OUU>(lds, tb, a.cuu, N, Sd, i0, cs, lane);
    ddp_cf_store<1, OC0>(lds, tb, a.c0, N, Sd, i0, cs, lane);
}
)DDPK";
