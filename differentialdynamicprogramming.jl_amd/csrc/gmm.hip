// gmm.hip — ddp_gmm_fit, ddp_gmm_prior: a Gaussian mixture over the transition tuples w = [x_i; u_i; x_i+1] of sampled rollouts (EM), and
// from it the normal-inverse-Wishart prior of every (step, trajectory) that ddp_fit_dynamics takes with prior_layout = 1 (Levine &
// Abbeel 2014; include/ddp_amd.h has the formulas).
//
// In xs[n,N,S,B] the point of (i, s, b) is two contiguous runs: [x_i; x_i+1], 2n doubles of xs, and u_i, m doubles of us.  Point j of a
// mixture is (s, i, b) with s fastest, so that the S points of one step lie together (ddp_gmm_prior takes them as they are).
//   gmm_estep   three waves, a chunk of 48 points in LDS as W[c][48] (the two k of one LDS access of the tile product are 48 = 16 mod 32
//               doubles apart).  Per cluster the Mahalanobis terms are V_k (W - mu_k) on v_mfma_f64_16x16x4 with V_k = L_k^-1 read from
//               global memory (lower blocks only), 16 points as the columns of a tile, one tile a wave; the mean is subtracted as the
//               operand is read.  Then lse and r per point, r to the workspace r[K][P], and the sums N_k, sum_j r_jk w_j of the chunk
//               (thread on (k, c), k fastest, j ascending).  A work-group takes a contiguous range of chunks and leaves one partial sum.
//               hard = 1: r is the 0/1 assignment of the Philox start instead.
//   gmm_means   one work-group per cluster: the partial sums in work-group order -> N_k, mu_k; and ll.
//   gmm_gram    four waves, chunks of 64 points in LDS as rows of ldc doubles (ldc = 16 mod 32, the layout of fit.hip); the upper 16-blocks
//               of sum_j r_jk (w_j - mu_k)(w_j - mu_k)' with the points as the contraction index, centred on the new mu_k as the operands
//               are read, at most GM_ACC accumulators a wave: (cluster, tile) items dealt over the waves, 16 / tiles clusters a work-group.
//   gmm_prep    one work-group per cluster: the partial Gram matrices in work-group order, 1 / N_k, reg -> Sigma_k, pi_k; then (also for a
//               mixture that is given: mode 1) the Cholesky factor in LDS, log det, V_k = L_k^-1 by columns, and the cluster's fail flag.
//   gmm_status  status and, after the last iteration, the NaNs of a mixture that failed.
//   gmm_prior   three waves per (step, trajectory): the E-step of its S points, omega, then mu0 and Phi in contiguous runs.
// Every sum has a fixed order: the split of the points over work-groups comes from (n, m, K, N, S, B) alone (gmm_plan), with pool = 0
// not from B.
#include <float.h>
#include <math.h>
#include <algorithm>
#include "ddp_internal.h"
#include "wide_tile.h"
#include "philox.h"
#include "staging.h"

namespace {

constexpr int GMM_PMAX = 2 * DDP_MAX_N_GENERIC + DDP_MAX_M, GMM_KMAX = 32;
constexpr int GE_CH = 48, GE_THREADS = 192, GE_LDR = GE_CH + 1, GE_SUMS = 13;   // K (p + 1) <= 32 * 73 <= 13 * 192
constexpr int GM_CH = 64, GM_ACC = 4, GM_KG = 4 * GM_ACC;
static_assert(GMM_KMAX * (GMM_PMAX + 1) <= GE_SUMS * GE_THREADS, "sums of gmm_estep");
static_assert((GMM_PMAX * GE_CH + GMM_KMAX * GE_LDR + GE_CH + GMM_PMAX + GMM_KMAX) * 8 + GE_CH * 20 + 16 <= 65536, "static LDS of gmm_estep");
static_assert(GMM_PMAX * GMM_PMAX * 8 + 64 <= 65536, "static LDS of gmm_prep");

struct GmmArgs {
    int n, m, N, S, B, K, pool, G, traj0;
    long P;                                                      // points of one mixture
    int nce, cpe, nwe, ncm, cpm, nwm;                            // chunks, chunks per work-group, work-groups per mixture: E-step, Gram
    int nb, ntiles, KG, ldc;
    unsigned seed_lo, seed_hi;
    int hard, t, iters, mode, last;
    double reg, n0;
    const double *xs, *us;
    double *pi, *mu, *Sigma, *ll;
    int32_t *status;
    double *V, *cst, *nk, *r, *part1, *llp, *part2;             // the workspace
    int32_t *fail, *badfrom;
    double *Phi, *mu0;                                           // ddp_gmm_prior
    int32_t *pstatus;
};

// the split of the points: from (n, m, K, N, S, B) alone, with pool = 0 not from B
void gmm_plan(GmmArgs &a)
{
    const int p = 2 * a.n + a.m;
    a.G = a.pool ? 1 : a.B;
    a.P = (long)(a.N - 1) * a.S * (a.pool ? a.B : 1);
    a.nb = cdivw(p, 16);
    a.ntiles = a.nb * (a.nb + 1) / 2;
    a.KG = imax(1, GM_KG / a.ntiles);
    a.ldc = p <= 16 ? 16 : (p <= 48 ? 48 : 80);
    a.nce = (int)((a.P + GE_CH - 1) / GE_CH);
    a.ncm = (int)((a.P + GM_CH - 1) / GM_CH);
    const int cape = a.pool ? 1024 : 8;
    long capm = a.pool ? 512 : 4;
    if (a.pool) capm = std::min(capm, std::max(1L, (64L << 20) / ((long)a.K * p * p * 8)));
    a.cpe = cdivw(a.nce, cape); a.nwe = cdivw(a.nce, a.cpe);
    a.cpm = cdivw(a.ncm, (int)capm); a.nwm = cdivw(a.ncm, a.cpm);
}

// point j of mixture g: its step, sample and trajectory
__device__ __forceinline__ void gmm_point(const GmmArgs &a, int g, long j, int &i, int &s, int &b)
{
    const long per = (long)(a.N - 1) * a.S;
    b = a.pool ? (int)(j / per) : g;
    const int rem = (int)(j - (a.pool ? (long)b * per : 0));
    i = rem / a.S; s = rem - i * a.S;
}

struct EShared {
    double W[GMM_PMAX * GE_CH];                                  // W[c][j]
    double r[GMM_KMAX * GE_LDR];                                 // lo, then r: r[k][j]
    double lse[GE_CH];
    double mu0[GMM_PMAX], om[GMM_KMAX];                          // gmm_prior
    unsigned long long xo[GE_CH], uo[GE_CH];
    int asg[GE_CH];
    int bad, mixbad;
};

// the cn points whose offsets stand in sh.xo, sh.uo -> sh.W (columns cn .. 47: zeros); sh.bad is raised by a point that is not finite
__device__ __forceinline__ void gmm_stage(EShared &sh, const double *xs, const double *us, int n, int m, int cn, int tid)
{
    const int p = 2 * n + m;
    bool bad = false;
    for (int e = tid; e < GE_CH * p; e += GE_THREADS) {
        const int j = e / p, c = e - j * p;
        double v = 0.0;
        if (j < cn) {
            v = c < n ? xs[sh.xo[j] + c] : (c < n + m ? us[sh.uo[j] + (c - n)] : xs[sh.xo[j] + (c - m)]);
            bad |= !(fabs(v) <= DBL_MAX);
        }
        sh.W[c * GE_CH + j] = v;
    }
    if (bad) atomicOr(&sh.bad, 1);
}

// the E-step of the staged chunk against the K clusters at V, mu, cst: sh.r = r_jk, sh.lse = lse_j (columns cn .. 47: zeros)
__device__ __forceinline__ void gmm_echunk(EShared &sh, const double *V, const double *mu, const double *cst, int p, int K, int cn, int tid)
{
    const int lane = tid & 63, wave = tid >> 6, l15 = lane & 15, l4 = lane >> 4, col = 16 * wave + l15, nb = cdivw(p, 16);
    for (int k = 0; k < K; ++k) {
        const double *Vk = V + (size_t)p * p * k, *muk = mu + (size_t)p * k;
        double sq = 0.0;
        for (int rb = 0; rb < nb; ++rb) {
            const int row = 16 * rb + l15, kend = min(16 * rb + 16, p);
            const bool rv = row < p;
            const double *vrow = Vk + (rv ? row : 0);
            d4 acc = d4{0.0, 0.0, 0.0, 0.0};
#pragma unroll 4
            for (int k0 = 0; k0 < kend; k0 += 4) {
                const int kk = k0 + l4;
                const bool kv = kk < kend;
                const int kc = kv ? kk : 0;
                const double av = vrow[(size_t)p * kc], bv = sh.W[kc * GE_CH + col] - muk[kc];
                acc = mf((rv && kv) ? av : 0.0, kv ? bv : 0.0, acc);
            }
            sq += acc.x * acc.x + acc.y * acc.y + acc.z * acc.z + acc.w * acc.w;
        }
        sq += __shfl_xor(sq, 16);
        sq += __shfl_xor(sq, 32);
        if (l4 == 0) sh.r[k * GE_LDR + col] = cst[k] - 0.5 * sq;
    }
    __syncthreads();
    if (tid < GE_CH) {
        double lse = 0.0;
        if (tid < cn) {
            double mx = sh.r[tid];
            for (int k = 1; k < K; ++k) mx = fmax(mx, sh.r[k * GE_LDR + tid]);
            double se = 0.0;
            for (int k = 0; k < K; ++k) se += exp(sh.r[k * GE_LDR + tid] - mx);
            lse = mx + log(se);
        }
        for (int k = 0; k < K; ++k) sh.r[k * GE_LDR + tid] = tid < cn ? exp(sh.r[k * GE_LDR + tid] - lse) : 0.0;
        sh.lse[tid] = lse;
    }
    __syncthreads();
}

__global__ __launch_bounds__(GE_THREADS) void gmm_estep(GmmArgs a)
{
    __shared__ EShared sh;
    const int tid = threadIdx.x, n = a.n, m = a.m, p = 2 * n + m, K = a.K;
    const int g = blockIdx.x / a.nwe, wg = blockIdx.x - g * a.nwe;
    const size_t gK = (size_t)g * K;
    const int nitems = K * (p + 1);
    double acc[GE_SUMS], llacc = 0.0;
#pragma unroll
    for (int q = 0; q < GE_SUMS; ++q) acc[q] = 0.0;
    if (tid == 0) sh.bad = 0;
    for (int ch = wg * a.cpe; ch < min((wg + 1) * a.cpe, a.nce); ++ch) {
        const long j0 = (long)ch * GE_CH;
        const int cn = (int)min((long)GE_CH, a.P - j0);
        if (tid < cn) {
            int i, s, b;
            gmm_point(a, g, j0 + tid, i, s, b);
            const size_t e = (size_t)i + (size_t)a.N * ((size_t)s + (size_t)a.S * b);
            sh.xo[tid] = (size_t)n * e; sh.uo[tid] = (size_t)m * e;
            if (a.hard) {
                unsigned w[4];
                ddp_philox4x32_10((unsigned)i, (unsigned)s, (unsigned)(a.traj0 + b), 0x80000000u, a.seed_lo, a.seed_hi, w);
                sh.asg[tid] = (int)(w[0] % (unsigned)K);
            }
        }
        __syncthreads();
        gmm_stage(sh, a.xs, a.us, n, m, cn, tid);
        __syncthreads();
        if (a.hard) {
            for (int e = tid; e < K * GE_CH; e += GE_THREADS) {
                const int k = e / GE_CH, j = e - k * GE_CH;
                sh.r[k * GE_LDR + j] = (j < cn && sh.asg[j] == k) ? 1.0 : 0.0;
            }
            __syncthreads();
        } else {
            gmm_echunk(sh, a.V + (size_t)p * p * gK, a.mu + (size_t)p * gK, a.cst + gK, p, K, cn, tid);
            if (tid == 0)
                for (int j = 0; j < cn; ++j) llacc += sh.lse[j];
        }
        for (int e = tid; e < K * GE_CH; e += GE_THREADS) {
            const int k = e / GE_CH, j = e - k * GE_CH;
            if (j < cn) a.r[(gK + k) * (size_t)a.P + j0 + j] = sh.r[k * GE_LDR + j];
        }
#pragma unroll
        for (int q = 0; q < GE_SUMS; ++q) {
            const int it = tid + GE_THREADS * q;
            if (it < nitems) {
                const int c = it / K, k = it - c * K;
                const double *rk = sh.r + k * GE_LDR, *wc = sh.W + (c < p ? c : 0) * GE_CH;
                double s = acc[q];
                if (c < p) for (int j = 0; j < cn; ++j) s += rk[j] * wc[j];
                else for (int j = 0; j < cn; ++j) s += rk[j];
                acc[q] = s;
            }
        }
        __syncthreads();
    }
    double *part = a.part1 + ((size_t)g * a.nwe + wg) * K * (p + 1);
#pragma unroll
    for (int q = 0; q < GE_SUMS; ++q) {
        const int it = tid + GE_THREADS * q;
        if (it < nitems) { const int c = it / K, k = it - c * K; part[k * (p + 1) + c] = acc[q]; }
    }
    if (tid == 0) a.llp[(size_t)g * a.nwe + wg] = llacc;
}

__global__ __launch_bounds__(128) void gmm_means(GmmArgs a)
{
    __shared__ double nk;
    const int tid = threadIdx.x, p = 2 * a.n + a.m, K = a.K, g = blockIdx.x / K, k = blockIdx.x - g * K;
    double s = 0.0;
    if (tid <= p)
#pragma unroll 8
        for (int wg = 0; wg < a.nwe; ++wg) s += a.part1[(((size_t)g * a.nwe + wg) * K + k) * (p + 1) + tid];
    if (tid == p) { nk = s; a.nk[(size_t)g * K + k] = s; }
    __syncthreads();
    if (tid < p) a.mu[((size_t)g * K + k) * p + tid] = s / nk;
    if (k == 0 && tid == 127 && a.t >= 0) {
        double l = 0.0;
        for (int wg = 0; wg < a.nwe; ++wg) l += a.llp[(size_t)g * a.nwe + wg];
        a.ll[a.t + (size_t)a.iters * g] = l;
    }
}

// tile q of the upper 16-blocks of a p x p matrix, nb blocks a side
__device__ __forceinline__ void gmm_tile(int q, int nb, int p, int &r0, int &r1, int &c0, int &c1)
{
    int bi = 0;
    while (q >= nb - bi) { q -= nb - bi; ++bi; }
    const int bj = bi + q;
    r0 = 16 * bi; r1 = min(r0 + 16, p); c0 = 16 * bj; c1 = min(c0 + 16, p);
}

template <int LDC>
__global__ __launch_bounds__(256) void gmm_gram(GmmArgs a)
{
    __shared__ double Wp[GM_CH * LDC];
    __shared__ double rl[GM_KG * GM_CH];
    __shared__ unsigned long long xo[GM_CH], uo[GM_CH];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l15 = lane & 15, l4 = lane >> 4;
    const int n = a.n, m = a.m, p = 2 * n + m, K = a.K;
    const int g = blockIdx.x / a.nwm, wg = blockIdx.x - g * a.nwm, k0 = blockIdx.y * a.KG, kn = min(a.KG, K - k0);
    const size_t gK = (size_t)g * K;
    const int nitems = kn * a.ntiles;
    d4 acc[GM_ACC];
    int oi[GM_ACC], oj[GM_ACC], kl[GM_ACC];
    double mi[GM_ACC], mj[GM_ACC];
#pragma unroll
    for (int ai = 0; ai < GM_ACC; ++ai) {
        acc[ai] = d4{0.0, 0.0, 0.0, 0.0};
        oi[ai] = oj[ai] = -1; kl[ai] = 0; mi[ai] = mj[ai] = 0.0;
        const int item = wave + 4 * ai;
        if (item < nitems) {
            kl[ai] = item / a.ntiles;
            int r0, r1, c0, c1;
            gmm_tile(item - kl[ai] * a.ntiles, a.nb, p, r0, r1, c0, c1);
            const double *muk = a.mu + (gK + k0 + kl[ai]) * p;
            if (r0 + l15 < r1) { oi[ai] = r0 + l15; mi[ai] = muk[oi[ai]]; }
            if (c0 + l15 < c1) { oj[ai] = c0 + l15; mj[ai] = muk[oj[ai]]; }
        }
    }
    for (int ch = wg * a.cpm; ch < min((wg + 1) * a.cpm, a.ncm); ++ch) {
        const long j0 = (long)ch * GM_CH;
        const int cn = (int)min((long)GM_CH, a.P - j0);
        if (tid < cn) {
            int i, s, b;
            gmm_point(a, g, j0 + tid, i, s, b);
            const size_t e = (size_t)i + (size_t)a.N * ((size_t)s + (size_t)a.S * b);
            xo[tid] = (size_t)n * e; uo[tid] = (size_t)m * e;
        }
        __syncthreads();
        for (int e = tid; e < cn * p; e += 256) {
            const int j = e / p, c = e - j * p;
            Wp[j * LDC + c] = c < n ? a.xs[xo[j] + c] : (c < n + m ? a.us[uo[j] + (c - n)] : a.xs[xo[j] + (c - m)]);
        }
        for (int e = tid; e < kn * GM_CH; e += 256) {
            const int k = e / GM_CH, j = e - k * GM_CH;
            rl[e] = j < cn ? a.r[(gK + k0 + k) * (size_t)a.P + j0 + j] : 0.0;
        }
        __syncthreads();
#pragma unroll
        for (int ai = 0; ai < GM_ACC; ++ai) {
            if (wave + 4 * ai >= nitems) continue;
            const bool iv = oi[ai] >= 0, jv = oj[ai] >= 0;
            const int ci = iv ? oi[ai] : 0, cj = jv ? oj[ai] : 0;
            const double *rk = rl + kl[ai] * GM_CH;
            d4 c = acc[ai];
            for (int q0 = 0; q0 < cn; q0 += 4) {
                const int q = q0 + l4;
                const bool qv = q < cn;
                const int qc = qv ? q : 0;
                const double *row = Wp + qc * LDC;
                const double av = rk[qc] * (row[ci] - mi[ai]), bv = row[cj] - mj[ai];
                c = mf((iv && qv) ? av : 0.0, (jv && qv) ? bv : 0.0, c);
            }
            acc[ai] = c;
        }
        __syncthreads();
    }
#pragma unroll
    for (int ai = 0; ai < GM_ACC; ++ai) {
        const int item = wave + 4 * ai;
        if (item >= nitems) continue;
        int r0, r1, c0, c1;
        gmm_tile(item - kl[ai] * a.ntiles, a.nb, p, r0, r1, c0, c1);
        double *part = a.part2 + (((size_t)g * a.nwm + wg) * K + k0 + kl[ai]) * p * p;
        const int j = c0 + l15;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int i = r0 + l4 + 4 * r;
            if (i < r1 && j < c1) part[i + p * j] = comp(acc[ai], r);
        }
    }
}

// mode 0: Sigma_k, pi_k of the M-step from the partial Gram matrices; mode 1: a mixture that is given.  Then L_k, log det, V_k, fail.
__global__ __launch_bounds__(256) void gmm_prep(GmmArgs a)
{
    __shared__ double A[GMM_PMAX * GMM_PMAX];
    __shared__ int badv;
    const int tid = threadIdx.x, p = 2 * a.n + a.m, K = a.K, g = blockIdx.x / K, k = blockIdx.x - g * K;
    const size_t gk = (size_t)g * K + k;
    double *Sg = a.Sigma + gk * p * p;
    double wk;                                                   // N_k, or pi_k of a mixture that is given
    if (tid == 0) badv = 0;
    __syncthreads();
    if (a.mode == 0) {
        wk = a.nk[gk];
        for (int e = tid; e < p * p; e += 256) {
            const int j = e / p, i = e - j * p;
            if (i > j) continue;
            double s = 0.0;
#pragma unroll 8
            for (int wg = 0; wg < a.nwm; ++wg) s += a.part2[(((size_t)g * a.nwm + wg) * K + k) * p * p + e];
            s /= wk;
            if (i == j) s += a.reg;
            A[i + p * j] = s; A[j + p * i] = s;
        }
        if (tid == 0) a.pi[gk] = wk / (double)a.P;
    } else {
        wk = a.pi[gk];
        bool bad = false;
        for (int e = tid; e < p * p; e += 256) {
            const int j = e / p, i = e - j * p;
            if (i < j) continue;
            const double s = Sg[e];
            A[i + p * j] = s; A[j + p * i] = s;
        }
        if (tid < p) bad |= !(fabs(a.mu[gk * p + tid]) <= DBL_MAX);
        if (bad) atomicOr(&badv, 1);
    }
    __syncthreads();
    if (a.mode == 0)
        for (int e = tid; e < p * p; e += 256) Sg[e] = A[e];
    int fail = (wk > 0.0 && wk <= DBL_MAX) ? 0 : 1;
    if (badv) fail = 1;
    for (int c = 0; c < p; ++c) {
        const double piv = A[c + p * c];
        if (!(piv > 0.0 && piv <= DBL_MAX)) fail = 1;
        const double rr = sqrt(piv);
        __syncthreads();
        if (tid == c) A[c + p * c] = rr;
        if (tid > c && tid < p) A[tid + p * c] /= rr;
        __syncthreads();
        const int w = p - c - 1;
        for (int e = tid; e < w * w; e += 256) {
            const int jj = e / w, ii = e - jj * w;
            if (ii >= jj) A[(c + 1 + ii) + p * (c + 1 + jj)] -= A[(c + 1 + ii) + p * c] * A[(c + 1 + jj) + p * c];
        }
        __syncthreads();
    }
    // column j of V = L^-1, thread j: v_j in a register, v_l (l > j) in row j of the upper triangle
    if (tid < p) {
        const int j = tid;
        const double vj = 1.0 / A[j + p * j];
        for (int i = j + 1; i < p; ++i) {
            double s = -A[i + p * j] * vj;
            for (int l = j + 1; l < i; ++l) s -= A[i + p * l] * A[j + p * l];
            A[j + p * i] = s / A[i + p * i];
        }
    }
    __syncthreads();
    double *Vk = a.V + gk * p * p;
    for (int e = tid; e < p * p; e += 256) {
        const int j = e / p, i = e - j * p;
        Vk[e] = i > j ? A[j + p * i] : (i == j ? 1.0 / A[e] : 0.0);
    }
    if (tid == 0) {
        double ld = 0.0;
        for (int c = 0; c < p; ++c) ld += log(A[c + p * c]);
        const double pik = a.mode == 0 ? wk / (double)a.P : wk;
        a.cst[gk] = log(pik) - 0.5 * (double)p * 1.8378770664093453 - ld;
        a.fail[gk] = fail;
    }
}

// status[g] after the M-step of iteration t (-1: the start); last: the NaNs of a mixture that failed
__global__ __launch_bounds__(256) void gmm_status(GmmArgs a)
{
    const int tid = threadIdx.x, p = 2 * a.n + a.m, K = a.K, g = blockIdx.x;
    int st = a.status[g], bf = a.badfrom[g], first = 0;
    for (int k = K - 1; k >= 0; --k)
        if (a.fail[(size_t)g * K + k]) first = k + 1;
    __syncthreads();
    if (st == 0 && first) {
        st = first; bf = a.t;
        if (tid == 0) { a.status[g] = st; a.badfrom[g] = bf; }
    }
    if (!a.last || st == 0) return;
    const double nan = __builtin_nan("");
    for (size_t e = tid; e < (size_t)K * p * p; e += 256) a.Sigma[(size_t)g * K * p * p + e] = nan;
    for (int e = tid; e < K * p; e += 256) a.mu[(size_t)g * K * p + e] = nan;
    if (tid < K) a.pi[(size_t)g * K + tid] = nan;
    for (int t = bf + 1 + tid; t < a.iters; t += 256) a.ll[t + (size_t)a.iters * g] = nan;
}

__global__ __launch_bounds__(GE_THREADS) void gmm_prior(GmmArgs a)
{
    __shared__ EShared sh;
    const int tid = threadIdx.x, n = a.n, m = a.m, p = 2 * n + m, K = a.K, N = a.N, S = a.S;
    const int b = blockIdx.x / N, i = blockIdx.x - b * N, g = a.pool ? 0 : b;
    const size_t gK = (size_t)g * K, sidx = (size_t)i + (size_t)N * b;
    double *Phi = a.Phi + sidx * p * p, *mu0 = a.mu0 + sidx * p;
    if (i == N - 1) {                                            // slot N - 1 has no transition
        for (int e = tid; e < p * p; e += GE_THREADS) Phi[e] = 0.0;
        if (tid < p) mu0[tid] = 0.0;
        if (tid == 0) a.pstatus[sidx] = 0;
        return;
    }
    if (tid == 0) {
        int mb = 0;
        for (int k = 0; k < K; ++k) mb |= a.fail[gK + k];
        sh.bad = 0; sh.mixbad = mb;
    }
    double om = 0.0;
    for (int s0 = 0; s0 < S; s0 += GE_CH) {
        const int cn = min(GE_CH, S - s0);
        if (tid < cn) {
            const size_t e = (size_t)i + (size_t)N * ((size_t)(s0 + tid) + (size_t)S * b);
            sh.xo[tid] = (size_t)n * e; sh.uo[tid] = (size_t)m * e;
        }
        __syncthreads();
        gmm_stage(sh, a.xs, a.us, n, m, cn, tid);
        __syncthreads();
        gmm_echunk(sh, a.V + (size_t)p * p * gK, a.mu + (size_t)p * gK, a.cst + gK, p, K, cn, tid);
        if (tid < K)
            for (int j = 0; j < cn; ++j) om += sh.r[tid * GE_LDR + j];
        __syncthreads();
    }
    if (tid < K) sh.om[tid] = om / (double)S;
    __syncthreads();
    const int st = sh.mixbad ? 2 : (sh.bad ? 1 : 0);
    const double nan = __builtin_nan("");
    const double *mu = a.mu + (size_t)p * gK, *Sg = a.Sigma + (size_t)p * p * gK;
    if (tid < p) {
        double s = 0.0;
        for (int k = 0; k < K; ++k) s += sh.om[k] * mu[k * p + tid];
        sh.mu0[tid] = s;
        mu0[tid] = st ? nan : s;
    }
    __syncthreads();
    for (int e = tid; e < p * p; e += GE_THREADS) {
        const int c = e / p, r = e - c * p, hi = max(r, c), lo = min(r, c);
        double s = 0.0;
        for (int k = 0; k < K; ++k)
            s += sh.om[k] * (Sg[(size_t)p * p * k + hi + p * lo] + (mu[k * p + hi] - sh.mu0[hi]) * (mu[k * p + lo] - sh.mu0[lo]));
        Phi[e] = st ? nan : a.n0 * s;
    }
    if (tid == 0) a.pstatus[sidx] = st;
}

bool finite_nonneg(double v) { return v >= 0.0 && v <= DBL_MAX; }

// what the entries refuse, before the device is touched
int gmm_validate(const char *who, int n, int m, int N, int S, int B, int K, int pool, const void *xs, const void *us)
{
    DDP_CHECK(n >= 1 && n <= DDP_MAX_N_GENERIC, "%s: n = %d out of [1, %d]", who, n, DDP_MAX_N_GENERIC);
    DDP_CHECK(m >= 1 && m <= DDP_MAX_M, "%s: m = %d out of [1, %d]", who, m, DDP_MAX_M);
    DDP_CHECK(K >= 1 && K <= GMM_KMAX, "%s: K = %d out of [1, %d]", who, K, GMM_KMAX);
    DDP_CHECK(N >= 2, "%s: N = %d, at least 2 steps are needed", who, N);
    DDP_CHECK(S >= 1, "%s: S = %d (>= 1)", who, S);
    DDP_CHECK(B >= 1, "%s: B = %d (>= 1)", who, B);
    DDP_CHECK(pool == 0 || pool == 1, "%s: pool = %d (0: one mixture per trajectory, 1: one over all)", who, pool);
    DDP_CHECK((double)N * S * B <= 2147483647.0, "%s: N = %d, S = %d, B = %d is too large", who, N, S, B);
    DDP_CHECK(xs && us, "%s: null argument", who);
    return 0;
}

int gmm_fit_validate(int n, int m, int N, int S, int B, int K, int iters, int pool, const void *xs, const void *us, double reg, const void *pi0,
                     const void *mu0, const void *Sigma0, const void *pi, const void *mu, const void *Sigma, const void *ll, const void *status)
{
    { const int rc = gmm_validate("fit_gmm", n, m, N, S, B, K, pool, xs, us); if (rc) return rc; }
    const long P = (long)(N - 1) * S * (pool ? B : 1);
    DDP_CHECK(P >= 2, "fit_gmm: P = %ld points a mixture, at least 2 are needed", P);
    DDP_CHECK(P <= 0x7fffffffL - GM_CH, "fit_gmm: P = %ld points a mixture is too large", P);
    DDP_CHECK(iters >= 0, "fit_gmm: iters = %d (>= 0)", iters);
    DDP_CHECK(finite_nonneg(reg), "fit_gmm: reg = %g should be a finite number >= 0", reg);
    DDP_CHECK((pi0 != nullptr) == (mu0 != nullptr) && (pi0 != nullptr) == (Sigma0 != nullptr), "fit_gmm: init needs pi, mu and Sigma together");
    DDP_CHECK(pi && mu && Sigma && status && (ll || iters == 0), "fit_gmm: null argument");
    return 0;
}

int gmm_prior_validate(int n, int m, int N, int S, int B, int K, int pool, const void *xs, const void *us, const void *pi, const void *mu,
                       const void *Sigma, double m0, double n0, const void *Phi, const void *mu0, const void *status)
{
    { const int rc = gmm_validate("gmm_prior", n, m, N, S, B, K, pool, xs, us); if (rc) return rc; }
    DDP_CHECK(finite_nonneg(m0) && finite_nonneg(n0), "gmm_prior: m0 = %g, n0 = %g should be finite numbers >= 0", m0, n0);
    DDP_CHECK(pi && mu && Sigma && Phi && mu0 && status, "gmm_prior: null argument");
    return 0;
}

template <class T> T *carve(char *&at, size_t count)
{
    T *q = (T *)at;
    at += Staging::al(count * sizeof(T));
    return q;
}

void gmm_launch_gram(ddp_handle h, const GmmArgs &a)
{
    const dim3 grid((unsigned)((long)a.nwm * a.G), (unsigned)cdivw(a.K, a.KG));
    if (a.ldc == 16) hipLaunchKernelGGL(gmm_gram<16>, grid, dim3(256), 0, h->stream, a);
    else if (a.ldc == 48) hipLaunchKernelGGL(gmm_gram<48>, grid, dim3(256), 0, h->stream, a);
    else hipLaunchKernelGGL(gmm_gram<80>, grid, dim3(256), 0, h->stream, a);
}

}   // namespace

extern "C" {

int ddp_gmm_fit_f64_dev(ddp_handle h, int n, int m, int N, int S, int B, int K, int iters, int pool, int traj0, const double *xs,
                        const double *us, double reg, int seed_lo, int seed_hi, const double *pi0, const double *mu0, const double *Sigma0,
                        double *pi, double *mu, double *Sigma, double *ll, int32_t *status)
{
    { const int rc = gmm_fit_validate(n, m, N, S, B, K, iters, pool, xs, us, reg, pi0, mu0, Sigma0, pi, mu, Sigma, ll, status); if (rc) return rc; }
    DDP_DEVICE(h);
    GmmArgs a{};
    a.n = n; a.m = m; a.N = N; a.S = S; a.B = B; a.K = K; a.pool = pool; a.traj0 = traj0; a.iters = iters; a.reg = reg;
    a.seed_lo = (unsigned)seed_lo; a.seed_hi = (unsigned)seed_hi;
    a.xs = xs; a.us = us; a.pi = pi; a.mu = mu; a.Sigma = Sigma; a.ll = ll; a.status = status;
    gmm_plan(a);
    const size_t p = 2 * (size_t)n + m, GK = (size_t)a.G * K;
    const size_t sizes[9] = {GK * p * p, GK, GK, GK * (size_t)a.P, (size_t)a.G * a.nwe * K * (p + 1), (size_t)a.G * a.nwe,
                             (size_t)a.G * a.nwm * K * p * p, GK, (size_t)a.G};
    size_t need = 0;
    for (int q = 0; q < 9; ++q) need += Staging::al(sizes[q] * 8);
    DDP_CHECK(need <= ((size_t)8 << 30), "fit_gmm: a workspace of %zu bytes (K = %d, B = %d, pool = %d) is too large", need, K, B, pool);
    DDP_CHECK((long)a.nwe * a.G <= 0x7fffffffL && (long)a.nwm * a.G <= 0x7fffffffL && (long)K * a.G <= 0x7fffffffL,
              "fit_gmm: K = %d, B = %d is too large for one launch", K, B);
    void *base;
    { const int rc = ddp_scratch(h, need, &base); if (rc) return rc; }
    char *at = (char *)base;
    a.V = carve<double>(at, sizes[0]); a.cst = carve<double>(at, sizes[1]); a.nk = carve<double>(at, sizes[2]); a.r = carve<double>(at, sizes[3]);
    a.part1 = carve<double>(at, sizes[4]); a.llp = carve<double>(at, sizes[5]); a.part2 = carve<double>(at, sizes[6]);
    a.fail = carve<int32_t>(at, 2 * sizes[7]); a.badfrom = carve<int32_t>(at, 2 * sizes[8]);
    DDP_HIP(hipMemsetAsync(status, 0, sizeof(int32_t) * a.G, h->stream));
    DDP_HIP(hipMemsetAsync(a.badfrom, 0, sizeof(int32_t) * a.G, h->stream));
    const dim3 ge((unsigned)((long)a.nwe * a.G)), gk((unsigned)(K * a.G));
    auto mstep = [&]() {
        hipLaunchKernelGGL(gmm_means, gk, dim3(128), 0, h->stream, a);
        gmm_launch_gram(h, a);
        a.mode = 0;
        hipLaunchKernelGGL(gmm_prep, gk, dim3(256), 0, h->stream, a);
        hipLaunchKernelGGL(gmm_status, dim3(a.G), dim3(256), 0, h->stream, a);
    };
    a.t = -1; a.last = iters == 0;
    if (pi0) {
        if (pi0 != pi) DDP_HIP(hipMemcpyAsync(pi, pi0, GK * 8, hipMemcpyDeviceToDevice, h->stream));
        if (mu0 != mu) DDP_HIP(hipMemcpyAsync(mu, mu0, GK * p * 8, hipMemcpyDeviceToDevice, h->stream));
        if (Sigma0 != Sigma) DDP_HIP(hipMemcpyAsync(Sigma, Sigma0, GK * p * p * 8, hipMemcpyDeviceToDevice, h->stream));
        a.mode = 1;
        hipLaunchKernelGGL(gmm_prep, gk, dim3(256), 0, h->stream, a);
        hipLaunchKernelGGL(gmm_status, dim3(a.G), dim3(256), 0, h->stream, a);
    } else {
        a.hard = 1;
        hipLaunchKernelGGL(gmm_estep, ge, dim3(GE_THREADS), 0, h->stream, a);
        mstep();
    }
    a.hard = 0;
    for (int t = 0; t < iters; ++t) {
        a.t = t; a.last = t == iters - 1;
        hipLaunchKernelGGL(gmm_estep, ge, dim3(GE_THREADS), 0, h->stream, a);
        mstep();
    }
    DDP_HIP(hipGetLastError());
    return 0;
}

int ddp_gmm_fit_f64(ddp_handle h, int n, int m, int N, int S, int B, int K, int iters, int pool, int traj0, const double *xs,
                    const double *us, double reg, int seed_lo, int seed_hi, const double *pi0, const double *mu0, const double *Sigma0,
                    double *pi, double *mu, double *Sigma, double *ll, int32_t *status)
{
    { const int rc = gmm_fit_validate(n, m, N, S, B, K, iters, pool, xs, us, reg, pi0, mu0, Sigma0, pi, mu, Sigma, ll, status); if (rc) return rc; }
    DDP_DEVICE(h);
    const size_t nb = (size_t)N * S * B, p = 2 * (size_t)n + m, GK = (size_t)(pool ? 1 : B) * K;
    const double *dxs, *dus, *dpi0, *dmu0, *dSigma0;
    double *dpi, *dmu, *dSigma, *dll;
    int32_t *dstatus;
    Staging St(h, Staging::OWNED, "fit_gmm");
    St.in(&dxs, xs, (size_t)n * nb); St.in(&dus, us, (size_t)m * nb);
    St.in(&dpi0, pi0, GK); St.in(&dmu0, mu0, GK * p); St.in(&dSigma0, Sigma0, GK * p * p);
    St.out(&dpi, pi, GK); St.out(&dmu, mu, GK * p); St.out(&dSigma, Sigma, GK * p * p);
    St.out(&dll, iters ? ll : nullptr, (size_t)iters * (pool ? 1 : B)); St.out(&dstatus, status, pool ? 1 : B);
    int rc = St.commit();
    if (rc) return rc;
    return St.finish(ddp_gmm_fit_f64_dev(h, n, m, N, S, B, K, iters, pool, traj0, dxs, dus, reg, seed_lo, seed_hi, dpi0, dmu0, dSigma0, dpi, dmu,
                                         dSigma, dll, dstatus));
}

int ddp_gmm_prior_f64_dev(ddp_handle h, int n, int m, int N, int S, int B, int K, int pool, const double *xs, const double *us,
                          const double *pi, const double *mu, const double *Sigma, double m0, double n0, double *Phi, double *mu0,
                          int32_t *status)
{
    { const int rc = gmm_prior_validate(n, m, N, S, B, K, pool, xs, us, pi, mu, Sigma, m0, n0, Phi, mu0, status); if (rc) return rc; }
    DDP_DEVICE(h);
    GmmArgs a{};
    a.n = n; a.m = m; a.N = N; a.S = S; a.B = B; a.K = K; a.pool = pool; a.n0 = n0;
    a.xs = xs; a.us = us; a.pi = const_cast<double *>(pi); a.mu = const_cast<double *>(mu); a.Sigma = const_cast<double *>(Sigma);
    a.Phi = Phi; a.mu0 = mu0; a.pstatus = status;
    gmm_plan(a);
    const size_t p = 2 * (size_t)n + m, GK = (size_t)a.G * K;
    DDP_CHECK((long)N * B <= 0x7fffffffL && (long)K * a.G <= 0x7fffffffL, "gmm_prior: N = %d, B = %d is too large for one launch", N, B);
    const size_t need = Staging::al(GK * p * p * 8) + Staging::al(GK * 8) + Staging::al(GK * 8);
    void *base;
    { const int rc = ddp_scratch(h, need, &base); if (rc) return rc; }
    char *at = (char *)base;
    a.V = carve<double>(at, GK * p * p); a.cst = carve<double>(at, GK); a.fail = carve<int32_t>(at, 2 * GK);
    a.mode = 1;
    hipLaunchKernelGGL(gmm_prep, dim3((unsigned)(K * a.G)), dim3(256), 0, h->stream, a);
    hipLaunchKernelGGL(gmm_prior, dim3((unsigned)((long)N * B)), dim3(GE_THREADS), 0, h->stream, a);
    DDP_HIP(hipGetLastError());
    return 0;
}

int ddp_gmm_prior_f64(ddp_handle h, int n, int m, int N, int S, int B, int K, int pool, const double *xs, const double *us, const double *pi,
                      const double *mu, const double *Sigma, double m0, double n0, double *Phi, double *mu0, int32_t *status)
{
    { const int rc = gmm_prior_validate(n, m, N, S, B, K, pool, xs, us, pi, mu, Sigma, m0, n0, Phi, mu0, status); if (rc) return rc; }
    DDP_DEVICE(h);
    const size_t nb = (size_t)N * B, p = 2 * (size_t)n + m, GK = (size_t)(pool ? 1 : B) * K;
    const double *dxs, *dus, *dpi, *dmu, *dSigma;
    double *dPhi, *dmu0;
    int32_t *dstatus;
    Staging St(h, Staging::OWNED, "gmm_prior");
    St.in(&dxs, xs, (size_t)n * S * nb); St.in(&dus, us, (size_t)m * S * nb);
    St.in(&dpi, pi, GK); St.in(&dmu, mu, GK * p); St.in(&dSigma, Sigma, GK * p * p);
    St.out(&dPhi, Phi, p * p * nb); St.out(&dmu0, mu0, p * nb); St.out(&dstatus, status, nb);
    int rc = St.commit();
    if (rc) return rc;
    return St.finish(ddp_gmm_prior_f64_dev(h, n, m, N, S, B, K, pool, dxs, dus, dpi, dmu, dSigma, m0, n0, dPhi, dmu0, dstatus));
}

}   // extern "C"
