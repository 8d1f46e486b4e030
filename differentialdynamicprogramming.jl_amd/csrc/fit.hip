// fit.hip — ddp_fit_dynamics: time-varying linear-Gaussian dynamics fitted to sampled rollouts, the step between ddp_user_sample and
// iLQGkl's Model(fx, fu) in the guided-policy-search round (include/ddp_amd.h has the formula).
//
// One work-group of four waves per run of T consecutive steps of one trajectory; T comes from (n, m) alone (fit_plan), so the summation
// order does not depend on B.  In xs[n,N,S,B] the states of a run are S pieces of (T + 1) n contiguous doubles: a chunk of `sc` samples
// is brought into LDS as rows [x_i0 .. x_i0+T | u_i0 .. u_i0+T-1] of `ld` doubles (ld = 16 mod 32: the 2 x 16 lanes of one LDS access
// of the tile product fall on 32 different banks), and every state serves as x of its step and y of the step before.
//   pass 1   column sums over the samples, one thread per column of the row, s ascending -> mu
//   pass 2   the centred Gram matrices on v_mfma_f64_16x16x4 with the samples as the contraction index: (step, tile) items dealt over the
//            waves, at most FIT_ACC accumulators a wave; the mean is subtracted as the operands are read (no sum w w' - S mu mu').
//            Tiles: the upper 16-blocks of C_zz, all of C_zy, the upper blocks of C_yy (15 at (32, 8)); one tile when p <= 16.
//   then     the tiles go to LDS as A = C_zz + ridge I (both triangles), C_zy, C_yy with the prior and the divisor applied, and the
//            rest runs out of LDS in four phases whose items are dealt over the waves: (A) the Cholesky factor of a step, lane r on row
//            r, the multipliers passed between lanes in registers; (B) eight right-hand sides of a step at a time, lane r holding entry
//            r of each in registers through both substitutions; (C) fc and eight rows of C_yy - F C_zy, lane j on column j; (D) the
//            test that the results of a step are finite, and the stores, all threads.
// Two instantiations by LDS size: p <= 16 (one tile a step) takes the small pool, so that more work-groups share a compute unit.
#include <float.h>
#include "ddp_internal.h"
#include "wide_tile.h"
#include "staging.h"

namespace {

constexpr int FIT_ACC = 4;                                       // tile accumulators per wave: T * tiles <= 4 FIT_ACC
constexpr int FIT_TMAX = 4 * FIT_ACC;
constexpr int FIT_ROW = 112;                                     // doubles of a staged row, (T + 1) n + T m, at most
// The pool holds the staged chunk during the two passes and the per-step matrices of the run afterwards (the Gram matrices wait in
// registers in between): one step at (32, 8) is 5280 doubles.  p <= 16: a smaller pool, and at most FIT_CAREA_S doubles of matrices.
constexpr int FIT_POOL = 5280, FIT_POOL_S = 2560, FIT_CAREA_S = 1024;
static_assert((FIT_POOL + 2 * FIT_ROW) * sizeof(double) + 8 * FIT_TMAX <= 65536, "static LDS of ddp_fit_dynamics");

struct FitArgs {
    int n, m, N, S, T, ld, sc, ntiles, nz, ny, runs, prior, small;                 // prior: 0 none, 1 one for all, 2 per (step, trajectory)
    double ridge, m0, n0;
    const double *xs, *us, *Phi, *mu0;
    double *fx, *fu, *fc, *cov;
    int32_t *status;
};

__host__ __device__ constexpr int fit_stepsz(int n, int m) { return (n + m) * (n + m) + 2 * ((n + m) | 1) * n + (n | 1) * n; }

// T, ld, sc, the tile counts and the pool of (n, m)
void fit_plan(FitArgs &a)
{
    const int n = a.n, m = a.m, d = n + m, p = d + n;
    a.nz = cdivw(d, 16); a.ny = cdivw(n, 16);
    a.small = p <= 16;
    a.ntiles = a.small ? 1 : a.nz * (a.nz + 1) / 2 + a.nz * a.ny + a.ny * (a.ny + 1) / 2;
    const int carea = a.small ? FIT_CAREA_S : FIT_POOL, pool = a.small ? FIT_POOL_S : FIT_POOL;
    int T = FIT_TMAX / a.ntiles;
    while (T > 1 && ((T + 1) * n + T * m > FIT_ROW || T * fit_stepsz(n, m) > carea)) --T;
    a.T = T;
    a.ld = ((T + 1) * n + T * m + 15) / 32 * 32 + 16;
    a.sc = (pool / a.ld) & ~3;
    a.runs = a.N > 1 ? cdivw(a.N - 1, T) : 1;
}

// tile q of a step: rows [r0, r1) x columns [c0, c1) of the p x p matrix
__device__ __forceinline__ void fit_tile(const FitArgs &a, int q, int &r0, int &r1, int &c0, int &c1)
{
    const int d = a.n + a.m, p = d + a.n;
    if (a.ntiles == 1) { r0 = 0; r1 = p; c0 = 0; c1 = p; return; }
    const int nzz = a.nz * (a.nz + 1) / 2, nzy = a.nz * a.ny;
    int bi = 0, bj;
    if (q < nzz) {
        while (q >= a.nz - bi) { q -= a.nz - bi; ++bi; }
        bj = bi + q;
        r0 = 16 * bi; r1 = min(r0 + 16, d); c0 = 16 * bj; c1 = min(c0 + 16, d);
    } else if (q < nzz + nzy) {
        q -= nzz; bi = q / a.ny; bj = q - bi * a.ny;
        r0 = 16 * bi; r1 = min(r0 + 16, d); c0 = d + 16 * bj; c1 = min(c0 + 16, p);
    } else {
        q -= nzz + nzy;
        while (q >= a.ny - bi) { q -= a.ny - bi; ++bi; }
        bj = bi + q;
        r0 = d + 16 * bi; r1 = min(r0 + 16, p); c0 = d + 16 * bj; c1 = min(c0 + 16, p);
    }
}

// where entry i of w = [x_t; u_t; x_t+1] lies in a staged row
__device__ __forceinline__ int fit_off(int i, int t, int n, int m, int T)
{
    return i < n ? t * n + i : (i < n + m ? (T + 1) * n + t * m + (i - n) : (t + 1) * n + (i - n - m));
}

// v of lane k (wave-uniform) in every lane
__device__ __forceinline__ double lane_bcast(double v, int k)
{
    return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), k), __builtin_amdgcn_readlane(__double2loint(v), k));
}

// (A) A = L L' in place, one wave, lane r on row r: L in the lower triangle, L' in the upper one, 1 / L_cc on the diagonal (all the
// substitutions need of it).  The pivot test of factor_lower (sample.hip); returns 0, or c + 1 for the first pivot that is not a
// positive finite number.
__device__ __forceinline__ int fit_chol(double *A, int d, int lane)
{
    int fail = 0;
    for (int c = 0; c < d; ++c) {
        const double piv = A[c + d * c];
        if (!(piv > 0.0 && piv <= DBL_MAX) && fail == 0) fail = c + 1;
        const double rr = sqrt(piv);
        const bool below = lane > c && lane < d;
        const double lrc = below ? A[lane + d * c] / rr : 0.0;
        if (below) { A[lane + d * c] = lrc; A[c + d * lane] = lrc; }
        if (lane == c) A[c + d * c] = 1.0 / rr;
#pragma unroll 4
        for (int j = c + 1; j < d; ++j) {
            const double ljc = lane_bcast(lrc, j);
            if (lane >= j && lane < d) A[lane + d * j] -= lrc * ljc;
        }
        wave_sync();
    }
    return fail;
}

// (B) columns j0 .. j0 + 7 of G = A^-1 C_zy, one wave: lane r holds entry r of each right-hand side through L y = b and L' g = y
__device__ __forceinline__ void fit_solve8(const double *A, const double *Z, double *G, int d, int lz, int n, int j0, int lane)
{
    double b[8];
    const int r = lane < d ? lane : 0;
#pragma unroll
    for (int q = 0; q < 8; ++q) b[q] = (lane < d && j0 + q < n) ? Z[r + lz * (j0 + q)] : 0.0;
    for (int k = 0; k < d; ++k) {
        const double rk = A[k + d * k], lrk = A[r + d * k];
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            const double y = lane_bcast(b[q], k) * rk;
            b[q] = lane == k ? y : (lane > k ? b[q] - lrk * y : b[q]);
        }
    }
    for (int k = d - 1; k >= 0; --k) {
        const double rk = A[k + d * k], urk = A[r + d * k];                          // r < k: the upper triangle, L[k, r]
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            const double x = lane_bcast(b[q], k) * rk;
            b[q] = lane == k ? x : (lane < k ? b[q] - urk * x : b[q]);
        }
    }
#pragma unroll
    for (int q = 0; q < 8; ++q)
        if (lane < d && j0 + q < n) G[r + lz * (j0 + q)] = b[q];
}

template <int POOL>
__global__ __launch_bounds__(256) void ddp_fit_dynamics(FitArgs a)
{
    __shared__ double pool[POOL];
    __shared__ double mu[FIT_ROW];
    __shared__ double fcv[FIT_ROW];                              // fc of the steps of the run: T n < FIT_ROW
    __shared__ int failv[FIT_TMAX], badv[FIT_TMAX];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l15 = lane & 15, l4 = lane >> 4;
    const int n = a.n, m = a.m, d = n + m, p = d + n, N = a.N, S = a.S, T = a.T, ld = a.ld;
    const int b = blockIdx.x / a.runs, run = blockIdx.x - b * a.runs, i0 = run * T;
    const int tc = min(T, N - 1 - i0);                           // the steps of this run; 0 when N = 1
    const int XL = (T + 1) * n, xlen = tc > 0 ? (tc + 1) * n : 0, ulen = tc * m, rowlen = XL + T * m;
    const int lz = d | 1, ly = n | 1, stepsz = fit_stepsz(n, m);
    double *stage = pool;
    const double *xb = a.xs + (size_t)n * ((size_t)N * S * b + i0), *ub = a.us + (size_t)m * ((size_t)N * S * b + i0);
    const size_t xss = (size_t)n * N, uss = (size_t)m * N;

    auto load = [&](int s0, int sn) {                            // samples s0 .. s0 + sn - 1 in contiguous runs
#pragma unroll 4
        for (int g = tid; g < sn * xlen; g += 256) {
            const int s = g / xlen, e = g - s * xlen;
            stage[s * ld + e] = xb[xss * (s0 + s) + e];
        }
#pragma unroll 4
        for (int g = tid; g < sn * ulen; g += 256) {
            const int s = g / ulen, e = g - s * ulen;
            stage[s * ld + XL + e] = ub[uss * (s0 + s) + e];
        }
    };

    // the mean as first + mean(w_s - first): a column that is the same in every sample (the sampler's x0) has exactly that mean
    double sum = 0.0, first = 0.0;
    if (tid < FIT_TMAX) badv[tid] = 0;
    for (int s0 = 0; s0 < S && tc > 0; s0 += a.sc) {
        const int sn = min(a.sc, S - s0);
        load(s0, sn);
        __syncthreads();
        if (tid < rowlen) {
            if (s0 == 0) first = stage[tid];
            for (int s = 0; s < sn; ++s) sum += stage[s * ld + tid] - first;
        }
        __syncthreads();
    }
    if (tid < rowlen) mu[tid] = first + sum / (double)S;
    __syncthreads();

    // the lane's two operand columns of every item of its wave: offset in a staged row (-1: outside the tile) and mean
    d4 acc[FIT_ACC];
    int oi[FIT_ACC], oj[FIT_ACC];
    double mi[FIT_ACC], mj[FIT_ACC];
    const int nitems = tc * a.ntiles;
#pragma unroll
    for (int ai = 0; ai < FIT_ACC; ++ai) {
        acc[ai] = d4{0.0, 0.0, 0.0, 0.0};
        oi[ai] = oj[ai] = -1; mi[ai] = mj[ai] = 0.0;
        const int item = wave + 4 * ai;
        if (item < nitems) {
            const int t = item / a.ntiles;
            int r0, r1, c0, c1;
            fit_tile(a, item - t * a.ntiles, r0, r1, c0, c1);
            if (r0 + l15 < r1) { oi[ai] = fit_off(r0 + l15, t, n, m, T); mi[ai] = mu[oi[ai]]; }
            if (c0 + l15 < c1) { oj[ai] = fit_off(c0 + l15, t, n, m, T); mj[ai] = mu[oj[ai]]; }
        }
    }
    for (int s0 = 0; s0 < S && tc > 0; s0 += a.sc) {
        const int sn = min(a.sc, S - s0);
        load(s0, sn);
        __syncthreads();
#pragma unroll
        for (int ai = 0; ai < FIT_ACC; ++ai) {
            if (wave + 4 * ai >= nitems) continue;
            const bool iv = oi[ai] >= 0, jv = oj[ai] >= 0;
            const int ci = iv ? oi[ai] : 0, cj = jv ? oj[ai] : 0;
            d4 c = acc[ai];
            for (int k0 = 0; k0 < sn; k0 += 4) {
                const int k = k0 + l4;
                const bool kv = k < sn;
                const double *row = stage + (kv ? k : 0) * ld;
                const double av = row[ci] - mi[ai], bv = row[cj] - mj[ai];
                c = mf((iv && kv) ? av : 0.0, (jv && kv) ? bv : 0.0, c);
            }
            acc[ai] = c;
        }
        __syncthreads();
    }

    // the tiles -> A, C_zy, C_yy of their steps, with the prior, the divisor and the ridge
    const double den = a.prior ? (double)S + a.n0 : (double)(S - 1), kap = a.prior ? (double)S * a.m0 / ((double)S + a.m0) : 0.0;
#pragma unroll
    for (int ai = 0; ai < FIT_ACC; ++ai) {
        const int item = wave + 4 * ai;
        if (item >= nitems) continue;
        const int t = item / a.ntiles;
        int r0, r1, c0, c1;
        fit_tile(a, item - t * a.ntiles, r0, r1, c0, c1);
        double *A = pool + t * stepsz, *Z = A + d * d, *Y = Z + 2 * lz * n;
        const size_t sidx = (size_t)(i0 + t) + (size_t)N * b;
        const double *Phi = a.prior == 2 ? a.Phi + (size_t)p * p * sidx : a.Phi, *mu0 = a.prior == 2 ? a.mu0 + (size_t)p * sidx : a.mu0;
        const int j = c0 + l15;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int i = r0 + l4 + 4 * r;
            if (!(i < r1 && j < c1 && i <= j)) continue;
            double v = comp(acc[ai], r);
            if (a.prior) v += Phi[j + p * i] + kap * (mu[fit_off(i, t, n, m, T)] - mu0[i]) * (mu[fit_off(j, t, n, m, T)] - mu0[j]);
            v /= den;
            if (j < d) {
                if (i == j) v += a.ridge;
                A[j + d * i] = v; A[i + d * j] = v;
            } else if (i < d) {
                Z[i + lz * (j - d)] = v;
            } else {
                Y[(i - d) + ly * (j - d)] = v; Y[(j - d) + ly * (i - d)] = v;
            }
        }
    }
    __syncthreads();

    for (int t = wave; t < tc; t += 4) {                         // (A)
        const int fail = fit_chol(pool + t * stepsz, d, lane);
        if (lane == 0) failv[t] = fail;
    }
    __syncthreads();
    const int ng = cdivw(n, 8);
    for (int item = wave; item < tc * ng; item += 4) {           // (B)
        const int t = item / ng, g = item - t * ng;
        const double *A = pool + t * stepsz, *Z = A + d * d;
        fit_solve8(A, Z, pool + t * stepsz + d * d + lz * n, d, lz, n, 8 * g, lane);
    }
    __syncthreads();
    const double nan = __builtin_nan("");
    for (int item = wave; item < tc * ng; item += 4) {           // (C): column j = lane of M = C_yy - F C_zy, rows 8 g .. 8 g + 7, and fc
        const int t = item / ng, g = item - t * ng;
        const double *Z = pool + t * stepsz + d * d, *G = Z + lz * n;
        double *Y = pool + t * stepsz + d * d + 2 * lz * n;
        if (lane >= n) continue;
        const double *z = Z + lz * lane;
        for (int i = 8 * g; i < min(8 * g + 8, n); ++i) {
            const double *gi = G + lz * i;
            double s = 0.0;
            for (int c = 0; c < d; ++c) s += gi[c] * z[c];
            Y[i + ly * lane] -= s;
        }
        if (g == 0) {
            const double *gj = G + lz * lane, *mx = mu + t * n, *mu_u = mu + XL + t * m;
            double s = 0.0;
            for (int c = 0; c < n; ++c) s += gj[c] * mx[c];
            for (int c = 0; c < m; ++c) s += gj[n + c] * mu_u[c];
            fcv[t * n + lane] = mu[(t + 1) * n + lane] - s;
        }
    }
    __syncthreads();
    // a step whose factorisation went through but whose results are not finite (a NaN or Inf among C_zy, C_yy or mu_y) fails too: d + 1
    for (int t = 0; t < tc; ++t) {
        if (failv[t]) continue;
        const double *G = pool + t * stepsz + d * d + lz * n, *Y = G + lz * n;
        bool bad = false;
        for (int e = tid; e < d * n; e += 256) { const int j = e / d; bad |= !(fabs(G[e - j * d + lz * j]) <= DBL_MAX); }
        for (int e = tid; e < n * n; e += 256) { const int j = e / n; bad |= !(fabs(Y[e - j * n + ly * j]) <= DBL_MAX); }
        if (tid < n) bad |= !(fabs(fcv[t * n + tid]) <= DBL_MAX);
        if (bad) atomicOr(&badv[t], 1);
    }
    __syncthreads();
    for (int t = 0; t < tc; ++t) {                               // (D)
        const double *G = pool + t * stepsz + d * d + lz * n, *Y = G + lz * n;
        const size_t sidx = (size_t)(i0 + t) + (size_t)N * b;
        const int fail = failv[t] ? failv[t] : (badv[t] ? d + 1 : 0);
        double *fx = a.fx + (size_t)n * n * sidx, *fu = a.fu + (size_t)n * m * sidx, *cov = a.cov + (size_t)n * n * sidx;
        for (int e = tid; e < n * n; e += 256) {
            const int c = e / n, r = e - c * n;
            fx[e] = fail ? nan : G[c + lz * r];
            cov[e] = fail ? nan : 0.5 * (Y[r + ly * c] + Y[c + ly * r]);
        }
        for (int e = tid; e < n * m; e += 256) {
            const int c = e / n, r = e - c * n;
            fu[e] = fail ? nan : G[n + c + lz * r];
        }
        if (tid < n) a.fc[(size_t)n * sidx + tid] = fail ? nan : fcv[t * n + tid];
        if (tid == 0) a.status[sidx] = fail;
    }
    if (run == a.runs - 1) {                                     // slot N - 1 has no transition
        const size_t sidx = (size_t)(N - 1) + (size_t)N * b;
        for (int e = tid; e < n * n; e += 256) { a.fx[(size_t)n * n * sidx + e] = 0.0; a.cov[(size_t)n * n * sidx + e] = 0.0; }
        for (int e = tid; e < n * m; e += 256) a.fu[(size_t)n * m * sidx + e] = 0.0;
        if (tid < n) a.fc[(size_t)n * sidx + tid] = 0.0;
        if (tid == 0) a.status[sidx] = 0;
    }
}

// what both entries refuse, before the device is touched
int fit_validate(int n, int m, int N, int S, int B, const void *xs, const void *us, double ridge, const void *Phi, const void *mu0, double m0,
                 double n0, int prior_layout, const void *fx, const void *fu, const void *fc, const void *cov, const void *status)
{
    DDP_CHECK(n >= 1 && n <= DDP_MAX_N_GENERIC, "fit_dynamics: n = %d out of [1, %d]", n, DDP_MAX_N_GENERIC);
    DDP_CHECK(m >= 1 && m <= DDP_MAX_M, "fit_dynamics: m = %d out of [1, %d]", m, DDP_MAX_M);
    DDP_CHECK(S >= 2, "fit_dynamics: S = %d, at least 2 samples are needed", S);
    DDP_CHECK(N >= 1 && B >= 1, "fit_dynamics: N = %d, B = %d (both >= 1)", N, B);
    DDP_CHECK(ridge >= 0.0 && ridge <= DBL_MAX, "fit_dynamics: ridge = %g should be a finite number >= 0", ridge);
    DDP_CHECK(xs && us && fx && fu && fc && cov && status, "fit_dynamics: null argument");
    if (Phi) {
        DDP_CHECK(mu0, "fit_dynamics: a prior needs mu0 with Phi");
        DDP_CHECK(prior_layout == 0 || prior_layout == 1, "fit_dynamics: prior_layout = %d (0: one prior, 1: one per step and trajectory)", prior_layout);
        DDP_CHECK(m0 >= 0.0 && m0 <= DBL_MAX && n0 >= 0.0 && n0 <= DBL_MAX, "fit_dynamics: m0 = %g, n0 = %g should be finite numbers >= 0", m0, n0);
    }
    return 0;
}

}   // namespace

extern "C" {

int ddp_fit_dynamics_f64_dev(ddp_handle h, int n, int m, int N, int S, int B, const double *xs, const double *us, double ridge,
                             const double *Phi, const double *mu0, double m0, double n0, int prior_layout, double *fx, double *fu,
                             double *fc, double *cov, int32_t *status)
{
    { const int rc = fit_validate(n, m, N, S, B, xs, us, ridge, Phi, mu0, m0, n0, prior_layout, fx, fu, fc, cov, status); if (rc) return rc; }
    DDP_DEVICE(h);
    FitArgs a{};
    a.n = n; a.m = m; a.N = N; a.S = S; a.prior = Phi ? 1 + prior_layout : 0;
    a.ridge = ridge; a.m0 = m0; a.n0 = n0;
    a.xs = xs; a.us = us; a.Phi = Phi; a.mu0 = mu0; a.fx = fx; a.fu = fu; a.fc = fc; a.cov = cov; a.status = status;
    fit_plan(a);
    DDP_CHECK(a.T >= 1 && a.T * a.ntiles <= FIT_TMAX && (a.T + 1) * n + a.T * m <= FIT_ROW && a.sc >= 4
              && a.T * fit_stepsz(n, m) <= (a.small ? FIT_POOL_S : FIT_POOL) && a.sc * a.ld <= (a.small ? FIT_POOL_S : FIT_POOL), "fit_dynamics: no plan for n = %d, m = %d", n, m);
    DDP_CHECK((long)a.runs * B <= 0x7fffffffL, "fit_dynamics: N = %d, B = %d is too large for one launch", N, B);
    const dim3 grid((unsigned)((long)a.runs * B));
    if (a.small) hipLaunchKernelGGL(ddp_fit_dynamics<FIT_POOL_S>, grid, dim3(256), 0, h->stream, a);
    else hipLaunchKernelGGL(ddp_fit_dynamics<FIT_POOL>, grid, dim3(256), 0, h->stream, a);
    DDP_HIP(hipGetLastError());
    return 0;
}

int ddp_fit_dynamics_f64(ddp_handle h, int n, int m, int N, int S, int B, const double *xs, const double *us, double ridge,
                         const double *Phi, const double *mu0, double m0, double n0, int prior_layout, double *fx, double *fu,
                         double *fc, double *cov, int32_t *status)
{
    { const int rc = fit_validate(n, m, N, S, B, xs, us, ridge, Phi, mu0, m0, n0, prior_layout, fx, fu, fc, cov, status); if (rc) return rc; }
    DDP_DEVICE(h);
    const size_t nb = (size_t)N * B, p = 2 * (size_t)n + m, np = Phi && prior_layout == 1 ? nb : 1;
    const double *dxs, *dus, *dPhi, *dmu0;
    double *dfx, *dfu, *dfc, *dcov;
    int32_t *dstatus;
    Staging St(h, Staging::OWNED, "fit_dynamics");
    St.in(&dxs, xs, (size_t)n * S * nb); St.in(&dus, us, (size_t)m * S * nb);
    St.in(&dPhi, Phi, p * p * np); St.in(&dmu0, Phi ? mu0 : nullptr, p * np);
    St.out(&dfx, fx, (size_t)n * n * nb); St.out(&dfu, fu, (size_t)n * m * nb); St.out(&dfc, fc, (size_t)n * nb);
    St.out(&dcov, cov, (size_t)n * n * nb); St.out(&dstatus, status, nb);
    int rc = St.commit();
    if (rc) return rc;
    return St.finish(ddp_fit_dynamics_f64_dev(h, n, m, N, S, B, dxs, dus, ridge, dPhi, dmu0, m0, n0, prior_layout, dfx, dfu, dfc, dcov, dstatus));
}

}   // extern "C"
