// fit_wide.hip — ddp_fit_dynamics_wide: the fit of fit.hip for n <= 64, m <= 32 (include/ddp_amd.h has the formula).  A shape inside the
// box of fit.hip is handed to its entry; everything else runs the kernel below.
//
// One work-group of four waves per (step, trajectory).  Everything after the Gram matrix lives in LDS as 16 x 16 blocks of FW_BS = 272
// doubles, entry (i, j) of a block at i + 17 j: the lower blocks of A = C_zz + ridge I, the blocks of C_zy' (rows y, columns z) and the
// upper blocks of C_yy, one block per Gram tile (55 at (64, 32): 117 KiB of dynamic LDS, sized from (n, m) at launch).  Blocks that
// reach past d or n are padded: A with the identity, the others with zeros, so that no product below looks at a bound.
//   pass 1   column sums straight from memory, one thread per column, s ascending -> mu = first + mean(w_s - first)
//   pass 2   the samples are staged in LDS with the mean taken off, rows [x_i | u_i | x_i+1 | 0] of ld = 16 (mod 32) doubles, and every
//            wave runs its tiles (at most FW_ACC accumulators) on v_mfma_f64_16x16x4 over the samples; the chunk length comes from
//            (n, m) alone, and the staged chunk shares the pool with the blocks (the tiles wait in registers in between).
//   factor   blocked left-looking Cholesky over 16 columns: (U) the blocks of column kb take their updates from the columns before
//            on the matrix cores, (D) one wave factors the diagonal block in registers, lane r on row r, tests the fully updated
//            pivots and leaves W = L_kk^-1 in its place, (P) the blocks below become A_ik W' on the matrix cores.
//   solves   wave cb owns columns 16 cb .. of the right-hand sides through both substitutions, a block row at a time: products with
//            the blocks of L, then with W (forward) or W' (backward).  Between the two, cov = C_yy - Y1' Y1 with Y1 = L^-1 C_zy:
//            the same matrix as C_yy - F C_zy, symmetric by construction, and G = A^-1 C_zy overwrites Y1 in place.
//   stores   fc, the test that the results are finite, and the outputs, all threads.
#include <float.h>
#include "ddp_internal.h"
#include "wide_tile.h"
#include "staging.h"

namespace {

constexpr int FW_LB = 17, FW_BS = 16 * FW_LB;                    // leading dimension and doubles of a block
constexpr int FW_ACC = 14;                                       // tile accumulators per wave: 55 tiles at (64, 32) over four waves
constexpr int FW_MAX_N = DDP_MAX_N_USER_WAVE, FW_MAX_M = DDP_MAX_M_WIDE;
constexpr int FW_PMAX = 2 * FW_MAX_N + FW_MAX_M, FW_LDMAX = (FW_PMAX + 16) / 32 * 32 + 16;
constexpr int FW_MAX_TILES = 4 * FW_ACC;
constexpr int FW_DEPTH = 8;                                      // loads of a thread in flight while the samples are fetched
constexpr int FW_MAX_LDS = 55 * FW_BS * (int)sizeof(double);     // dynamic LDS at (64, 32)
// Timing of the phases: a build with -DDDP_FIT_WIDE_STOP=k ends the kernel after the Gram matrices (1), the factor (2) or
// the solves (3); 0, the default and the only value the library is built with, runs all of it.
#ifndef DDP_FIT_WIDE_STOP
#define DDP_FIT_WIDE_STOP 0
#endif
constexpr int FW_STOP = DDP_FIT_WIDE_STOP;
static_assert(FW_MAX_N == 64 && FW_MAX_M == 32, "the tile counts of ddp_fit_dynamics_wide are those of n <= 64, m <= 32");
static_assert(FW_MAX_LDS + (FW_LDMAX + FW_MAX_N) * sizeof(double) + 64 <= 160 * 1024, "LDS of ddp_fit_dynamics_wide");

struct FitWideArgs {
    int n, m, N, S, ld, sc, nzb, nyb, ntiles, prior;             // prior: 0 none, 1 one for all, 2 per (step, trajectory)
    double ridge, m0, n0;
    const double *xs, *us, *Phi, *mu0;
    double *fx, *fu, *fc, *cov;
    int32_t *status;
};

// ld, sc and the block counts of (n, m)
void fit_wide_plan(FitWideArgs &a)
{
    const int d = a.n + a.m, p = d + a.n;
    a.nzb = cdivw(d, 16); a.nyb = cdivw(a.n, 16);
    a.ntiles = a.nzb * (a.nzb + 1) / 2 + a.nzb * a.nyb + a.nyb * (a.nyb + 1) / 2;
    a.ld = (p + 16) / 32 * 32 + 16;                              // > p: column p of a staged row is the zero every lane outside a tile reads
    a.sc = (a.ntiles * FW_BS / a.ld) & ~3;
}

// tile q = block q of the pool: its rows are w[xb .. xl), its columns w[yb .. yl); kind 0 A (lower), 1 C_zy', 2 C_yy (upper)
__device__ __forceinline__ void fw_tile(int nzb, int nyb, int d, int p, int q, int &xb, int &xl, int &yb, int &yl, int &kind)
{
    const int nzz = nzb * (nzb + 1) / 2, nzy = nzb * nyb;
    int bi = 0;
    if (q < nzz) {
        while (q > bi) { q -= bi + 1; ++bi; }
        kind = 0; xb = 16 * bi; xl = d; yb = 16 * q; yl = d;
    } else if (q < nzz + nzy) {
        q -= nzz;
        const int cb = q / nzb, kb = q - cb * nzb;
        kind = 1; xb = d + 16 * cb; xl = p; yb = 16 * kb; yl = d;
    } else {
        q -= nzz + nzy;
        while (q > bi) { q -= bi + 1; ++bi; }
        kind = 2; xb = d + 16 * q; xl = p; yb = d + 16 * bi; yl = p;
    }
}

__device__ __forceinline__ double fw_bcast(double v, int k)
{
    return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), k), __builtin_amdgcn_readlane(__double2loint(v), k));
}

// acc[i][j] += sum_{k < 16} X[k xk + i xi] Y[k yk + j yj] on whole blocks; component r of lane l is row (l >> 4) + 4 r, column l & 15
__device__ __forceinline__ d4 fw_prod(const double *X, int xk, int xi, const double *Y, int yk, int yj, d4 acc, int l15, int l4)
{
#pragma unroll
    for (int k0 = 0; k0 < 16; k0 += 4) acc = mf(X[(k0 + l4) * xk + l15 * xi], Y[(k0 + l4) * yk + l15 * yj], acc);
    return acc;
}

// block[row + 17 col] -= acc (tr = false), block[col + 17 row] -= acc (tr = true)
template <bool TR>
__device__ __forceinline__ void fw_sub(double *blk, const d4 &acc, int l15, int l4)
{
#pragma unroll
    for (int r = 0; r < 4; ++r) blk[TR ? l15 + FW_LB * (l4 + 4 * r) : (l4 + 4 * r) + FW_LB * l15] -= comp(acc, r);
}
template <bool TR>
__device__ __forceinline__ void fw_put(double *blk, const d4 &acc, int l15, int l4)
{
#pragma unroll
    for (int r = 0; r < 4; ++r) blk[TR ? l15 + FW_LB * (l4 + 4 * r) : (l4 + 4 * r) + FW_LB * l15] = comp(acc, r);
}

// (D) the diagonal block D = L L' in registers, one wave, lane r (and its copies r + 16, ..) on row r; the pivot test of fit_chol on
// the fully updated diagonal; W = L^-1 (lower, zeros above) is left in D.  Returns 0 or c0 + c + 1 for the first bad pivot c.
__device__ __forceinline__ int fw_diag(double *D, int c0, int lane)
{
    const int r = lane & 15;
    double a[16], x[16];
#pragma unroll
    for (int c = 0; c < 16; ++c) a[c] = D[r + FW_LB * c];
    int fail = 0;
#pragma unroll
    for (int c = 0; c < 16; ++c) {
        const double piv = fw_bcast(a[c], c);
        if (!(piv > 0.0 && piv <= DBL_MAX) && fail == 0) fail = c0 + c + 1;
        const double ri = 1.0 / sqrt(piv);
        const double l = r > c ? a[c] * ri : 0.0;
        a[c] = r == c ? ri : l;                                  // 1 / L_cc on the diagonal
#pragma unroll
        for (int j = c + 1; j < 16; ++j) a[j] -= l * fw_bcast(l, j);
    }
    // column j = r of W: x_i = (delta_ij - sum_{k < i} L_ik x_k) / L_ii; L_ik is a[k] of lane i
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        double s = i == r ? 1.0 : 0.0;
#pragma unroll
        for (int k = 0; k < i; ++k) s -= fw_bcast(a[k], i) * x[k];
        x[i] = s * fw_bcast(a[i], i);
    }
    if (lane < 16) {
#pragma unroll
        for (int i = 0; i < 16; ++i) D[i + FW_LB * r] = i >= r ? x[i] : 0.0;
    }
    return fail;
}

__global__ __launch_bounds__(256) void ddp_fit_dynamics_wide(FitWideArgs a)
{
    extern __shared__ double pool[];
    __shared__ double mu[FW_LDMAX];
    __shared__ double fcv[FW_MAX_N];
    __shared__ int failv, badv;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l15 = lane & 15, l4 = lane >> 4;
    const int n = a.n, m = a.m, d = n + m, p = d + n, N = a.N, S = a.S, ld = a.ld, nzb = a.nzb, nyb = a.nyb;
    const int b = blockIdx.x / N, step = blockIdx.x - b * N;
    const size_t sidx = (size_t)step + (size_t)N * b;
    double *fx = a.fx + (size_t)n * n * sidx, *fu = a.fu + (size_t)n * m * sidx, *cov = a.cov + (size_t)n * n * sidx;
    if (step == N - 1) {                                         // slot N - 1 has no transition
        for (int e = tid; e < n * n; e += 256) { fx[e] = 0.0; cov[e] = 0.0; }
        for (int e = tid; e < n * m; e += 256) fu[e] = 0.0;
        if (tid < n) a.fc[(size_t)n * sidx + tid] = 0.0;
        if (tid == 0) a.status[sidx] = 0;
        return;
    }
    double *stage = pool;
    const double *xb = a.xs + (size_t)n * ((size_t)N * S * b + step), *ub = a.us + (size_t)m * ((size_t)N * S * b + step);
    const size_t xss = (size_t)n * N, uss = (size_t)m * N;

    // samples s0 .. s0 + sn - 1, the mean taken off, as rows [x_i | u_i | x_i+1]: contiguous runs of xs and us, whole rows dealt over the
    // threads, FW_DEPTH loads of a thread in flight before the first of them is waited for
    const int rx = 256 / (2 * n), srx = tid / (2 * n), ex = tid - srx * 2 * n, wx = ex < n ? ex : ex + m;
    const int ru = 256 / m, sru = tid / m, eu = tid - sru * m;
    auto load = [&](int s0, int sn) {
        if (srx < rx) {
            const double mw = mu[wx];
            for (int s = srx; s < sn; s += FW_DEPTH * rx) {
                double v[FW_DEPTH];
#pragma unroll
                for (int q = 0; q < FW_DEPTH; ++q) v[q] = s + q * rx < sn ? xb[xss * (s0 + s + q * rx) + ex] : 0.0;
#pragma unroll
                for (int q = 0; q < FW_DEPTH; ++q)
                    if (s + q * rx < sn) stage[(s + q * rx) * ld + wx] = v[q] - mw;
            }
        }
        if (sru < ru) {
            const double mw = mu[n + eu];
            for (int s = sru; s < sn; s += FW_DEPTH * ru) {
                double v[FW_DEPTH];
#pragma unroll
                for (int q = 0; q < FW_DEPTH; ++q) v[q] = s + q * ru < sn ? ub[uss * (s0 + s + q * ru) + eu] : 0.0;
#pragma unroll
                for (int q = 0; q < FW_DEPTH; ++q)
                    if (s + q * ru < sn) stage[(s + q * ru) * ld + n + eu] = v[q] - mw;
            }
        }
    };

    // pass 1 straight from memory (entry w of consecutive threads is consecutive there): column sums, s ascending
    if (tid == 0) { failv = 0; badv = 0; }
    if (tid < p) {
        const double *src = tid < n ? xb + tid : (tid < d ? ub + (tid - n) : xb + n + (tid - d));
        const size_t st = (tid >= n && tid < d) ? uss : xss;
        const double first = src[0];
        double sum = 0.0;
        for (int s = 0; s < S; s += FW_DEPTH) {
            double v[FW_DEPTH];
#pragma unroll
            for (int q = 0; q < FW_DEPTH; ++q) v[q] = s + q < S ? src[st * (s + q)] : 0.0;
#pragma unroll
            for (int q = 0; q < FW_DEPTH; ++q)
                if (s + q < S) sum += v[q] - first;
        }
        mu[tid] = first + sum / (double)S;
    }
    __syncthreads();

    // the lane's two operand columns of every tile of its wave; a lane outside the tile reads the zero in column p
    d4 acc[FW_ACC];
    int ox[FW_ACC], oy[FW_ACC];
    const int cnt = (a.ntiles - wave + 3) >> 2;
#pragma unroll
    for (int ai = 0; ai < FW_ACC; ++ai) {
        acc[ai] = d4{0.0, 0.0, 0.0, 0.0};
        ox[ai] = oy[ai] = p;
        if (ai < cnt) {
            int x0, xl, y0, yl, kind;
            fw_tile(nzb, nyb, d, p, wave + 4 * ai, x0, xl, y0, yl, kind);
            if (x0 + l15 < xl) ox[ai] = x0 + l15;
            if (y0 + l15 < yl) oy[ai] = y0 + l15;
        }
    }
    for (int s0 = 0; s0 < S; s0 += a.sc) {
        const int sn = min(a.sc, S - s0), sn4 = (sn + 3) & ~3;   // sc is a multiple of 4: rows sn .. sn4 - 1 exist
        load(s0, sn);
        for (int g = tid; g < (sn4 - sn) * p; g += 256) { const int s = g / p; stage[(sn + s) * ld + g - s * p] = 0.0; }
        if (tid < sn4) stage[tid * ld + p] = 0.0;
        __syncthreads();
        for (int k0 = 0; k0 < sn4; k0 += 4) {
            const double *row = stage + (k0 + l4) * ld;
#pragma unroll
            for (int ai = 0; ai < FW_ACC; ++ai)
                if (ai < cnt) acc[ai] = mf(row[ox[ai]], row[oy[ai]], acc[ai]);
        }
        __syncthreads();
    }

    // the tiles -> their blocks, with the prior, the divisor, the ridge and the padding
    const double den = a.prior ? (double)S + a.n0 : (double)(S - 1), kap = a.prior ? (double)S * a.m0 / ((double)S + a.m0) : 0.0;
    const double *Phi = a.prior == 2 ? a.Phi + (size_t)p * p * sidx : a.Phi, *mu0 = a.prior == 2 ? a.mu0 + (size_t)p * sidx : a.mu0;
#pragma unroll
    for (int ai = 0; ai < FW_ACC; ++ai) {
        if (ai >= cnt) continue;
        int x0, xl, y0, yl, kind;
        fw_tile(nzb, nyb, d, p, wave + 4 * ai, x0, xl, y0, yl, kind);
        double *blk = pool + (wave + 4 * ai) * FW_BS;
        const int gj = y0 + l15;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int gi = x0 + l4 + 4 * r;
            double v;
            if (gi < xl && gj < yl) {
                const int lo = min(gi, gj), hi = max(gi, gj);
                v = comp(acc[ai], r);
                if (a.prior) v += Phi[hi + p * lo] + kap * (mu[lo] - mu0[lo]) * (mu[hi] - mu0[hi]);
                v /= den;
                if (kind == 0 && gi == gj) v += a.ridge;
            } else {
                v = (kind == 0 && gi == gj) ? 1.0 : 0.0;
            }
            blk[(l4 + 4 * r) + FW_LB * l15] = v;
        }
    }
    __syncthreads();

    // a stopped build writes one entry of the pool per thread, so that what ran before is kept
    auto stop = [&]() { if (tid < n) a.fc[(size_t)n * sidx + tid] = pool[(tid * 37) % (a.ntiles * FW_BS)]; };
    if (FW_STOP == 1) { stop(); return; }
    double *Ab = pool, *Zt = pool + nzb * (nzb + 1) / 2 * FW_BS, *Yb = Zt + nzb * nyb * FW_BS;
    auto Ablk = [&](int ib, int jb) { return Ab + (ib * (ib + 1) / 2 + jb) * FW_BS; };
    const d4 zero = d4{0.0, 0.0, 0.0, 0.0};

    for (int kb = 0; kb < nzb; ++kb) {                           // the factor
        if (kb > 0) {
            for (int ib = kb + wave; ib < nzb; ib += 4) {        // (U)
                d4 c = zero;
                for (int jb = 0; jb < kb; ++jb) c = fw_prod(Ablk(ib, jb), FW_LB, 1, Ablk(kb, jb), FW_LB, 1, c, l15, l4);
                fw_sub<false>(Ablk(ib, kb), c, l15, l4);
            }
            __syncthreads();
        }
        if (wave == 0) {                                         // (D)
            const int fail = fw_diag(Ablk(kb, kb), 16 * kb, lane);
            if (lane == 0 && fail && failv == 0) failv = fail;
        }
        __syncthreads();
        for (int ib = kb + 1 + wave; ib < nzb; ib += 4) {        // (P)
            const d4 c = fw_prod(Ablk(ib, kb), FW_LB, 1, Ablk(kb, kb), FW_LB, 1, zero, l15, l4);
            wave_sync();
            fw_put<false>(Ablk(ib, kb), c, l15, l4);
        }
        __syncthreads();
    }

    if (FW_STOP == 2) { stop(); return; }
    for (int cb = wave; cb < nyb; cb += 4) {                     // Y1 = L^-1 C_zy, columns 16 cb ..: block (z, y) of it is Zc[z]'
        double *Zc = Zt + cb * nzb * FW_BS;
        for (int kb = 0; kb < nzb; ++kb) {
            if (kb > 0) {
                d4 c = zero;
                for (int jb = 0; jb < kb; ++jb) c = fw_prod(Ablk(kb, jb), FW_LB, 1, Zc + jb * FW_BS, FW_LB, 1, c, l15, l4);
                fw_sub<true>(Zc + kb * FW_BS, c, l15, l4);
                wave_sync();
            }
            const d4 y = fw_prod(Ablk(kb, kb), FW_LB, 1, Zc + kb * FW_BS, FW_LB, 1, zero, l15, l4);
            wave_sync();
            fw_put<true>(Zc + kb * FW_BS, y, l15, l4);
            wave_sync();
        }
    }
    __syncthreads();
    for (int q = wave; q < nyb * (nyb + 1) / 2; q += 4) {        // cov = C_yy - Y1' Y1, the upper blocks
        int bj = 0, bi = q;
        while (bi > bj) { bi -= bj + 1; ++bj; }
        d4 c = zero;
        for (int kb = 0; kb < nzb; ++kb) c = fw_prod(Zt + (bi * nzb + kb) * FW_BS, FW_LB, 1, Zt + (bj * nzb + kb) * FW_BS, FW_LB, 1, c, l15, l4);
        fw_sub<false>(Yb + q * FW_BS, c, l15, l4);
    }
    __syncthreads();
    for (int cb = wave; cb < nyb; cb += 4) {                     // G = L'^-1 Y1 in place
        double *Zc = Zt + cb * nzb * FW_BS;
        for (int kb = nzb - 1; kb >= 0; --kb) {
            if (kb < nzb - 1) {
                d4 c = zero;
                for (int jb = kb + 1; jb < nzb; ++jb) c = fw_prod(Ablk(jb, kb), 1, FW_LB, Zc + jb * FW_BS, FW_LB, 1, c, l15, l4);
                fw_sub<true>(Zc + kb * FW_BS, c, l15, l4);
                wave_sync();
            }
            const d4 g = fw_prod(Ablk(kb, kb), 1, FW_LB, Zc + kb * FW_BS, FW_LB, 1, zero, l15, l4);
            wave_sync();
            fw_put<true>(Zc + kb * FW_BS, g, l15, l4);
            wave_sync();
        }
    }
    __syncthreads();

    if (FW_STOP == 3) { stop(); return; }

    // G[c, j] (c < d of z, j < n of y) and the upper triangle of cov
    auto G = [&](int c, int j) { return Zt[((j >> 4) * nzb + (c >> 4)) * FW_BS + (j & 15) + FW_LB * (c & 15)]; };
    auto Y = [&](int i, int j) {
        const int lo = min(i, j), hi = max(i, j), bi = lo >> 4, bj = hi >> 4;
        return Yb[(bj * (bj + 1) / 2 + bi) * FW_BS + (lo & 15) + FW_LB * (hi & 15)];
    };
    if (tid < n) {
        double s = 0.0;
        for (int c = 0; c < d; ++c) s += G(c, tid) * mu[c];
        fcv[tid] = mu[d + tid] - s;
    }
    __syncthreads();
    // a step whose factorisation went through but whose results are not finite (a NaN or Inf among C_zy, C_yy or mu_y) fails too: d + 1
    if (!failv) {
        bool bad = false;
        for (int e = tid; e < d * n; e += 256) { const int c = e / n; bad |= !(fabs(G(c, e - c * n)) <= DBL_MAX); }
        for (int e = tid; e < n * n; e += 256) { const int c = e / n; bad |= !(fabs(Y(e - c * n, c)) <= DBL_MAX); }
        if (tid < n) bad |= !(fabs(fcv[tid]) <= DBL_MAX);
        if (bad) atomicOr(&badv, 1);
    }
    __syncthreads();
    const int fail = failv ? failv : (badv ? d + 1 : 0);
    const double nan = __builtin_nan("");
    for (int e = tid; e < n * n; e += 256) {
        const int c = e / n, r = e - c * n;
        fx[e] = fail ? nan : G(c, r);
        cov[e] = fail ? nan : Y(r, c);
    }
    for (int e = tid; e < n * m; e += 256) {
        const int c = e / n, r = e - c * n;
        fu[e] = fail ? nan : G(n + c, r);
    }
    if (tid < n) a.fc[(size_t)n * sidx + tid] = fail ? nan : fcv[tid];
    if (tid == 0) a.status[sidx] = fail;
}

// what both entries refuse, before the device is touched
int fit_wide_validate(int n, int m, int N, int S, int B, const void *xs, const void *us, double ridge, const void *Phi, const void *mu0, double m0,
                      double n0, int prior_layout, const void *fx, const void *fu, const void *fc, const void *cov, const void *status)
{
    DDP_CHECK(n >= 1 && n <= FW_MAX_N, "fit_dynamics (wide): n = %d out of [1, %d]", n, FW_MAX_N);
    DDP_CHECK(m >= 1 && m <= FW_MAX_M, "fit_dynamics (wide): m = %d out of [1, %d]", m, FW_MAX_M);
    DDP_CHECK(S >= 2, "fit_dynamics (wide): S = %d, at least 2 samples are needed", S);
    DDP_CHECK(N >= 1 && B >= 1, "fit_dynamics (wide): N = %d, B = %d (both >= 1)", N, B);
    DDP_CHECK(ridge >= 0.0 && ridge <= DBL_MAX, "fit_dynamics (wide): ridge = %g should be a finite number >= 0", ridge);
    DDP_CHECK(xs && us && fx && fu && fc && cov && status, "fit_dynamics (wide): null argument");
    if (Phi) {
        DDP_CHECK(mu0, "fit_dynamics (wide): a prior needs mu0 with Phi");
        DDP_CHECK(prior_layout == 0 || prior_layout == 1, "fit_dynamics (wide): prior_layout = %d (0: one prior, 1: one per step and trajectory)", prior_layout);
        DDP_CHECK(m0 >= 0.0 && m0 <= DBL_MAX && n0 >= 0.0 && n0 <= DBL_MAX, "fit_dynamics (wide): m0 = %g, n0 = %g should be finite numbers >= 0", m0, n0);
    }
    return 0;
}

bool fit_wide_in_box(int n, int m) { return n <= DDP_MAX_N_GENERIC && m <= DDP_MAX_M; }

}   // namespace

extern "C" {

int ddp_fit_dynamics_wide_f64_dev(ddp_handle h, int n, int m, int N, int S, int B, const double *xs, const double *us, double ridge,
                                  const double *Phi, const double *mu0, double m0, double n0, int prior_layout, double *fx, double *fu,
                                  double *fc, double *cov, int32_t *status)
{
    { const int rc = fit_wide_validate(n, m, N, S, B, xs, us, ridge, Phi, mu0, m0, n0, prior_layout, fx, fu, fc, cov, status); if (rc) return rc; }
    if (fit_wide_in_box(n, m))                                   // smaller shapes keep their kernel, and its bits
        return ddp_fit_dynamics_f64_dev(h, n, m, N, S, B, xs, us, ridge, Phi, mu0, m0, n0, prior_layout, fx, fu, fc, cov, status);
    DDP_DEVICE(h);
    FitWideArgs a{};
    a.n = n; a.m = m; a.N = N; a.S = S; a.prior = Phi ? 1 + prior_layout : 0;
    a.ridge = ridge; a.m0 = m0; a.n0 = n0;
    a.xs = xs; a.us = us; a.Phi = Phi; a.mu0 = mu0; a.fx = fx; a.fu = fu; a.fc = fc; a.cov = cov; a.status = status;
    fit_wide_plan(a);
    const int bytes = a.ntiles * FW_BS * (int)sizeof(double);
    DDP_CHECK(a.ntiles <= FW_MAX_TILES && bytes <= FW_MAX_LDS && a.ld > 2 * n + m && a.ld <= FW_LDMAX && a.sc >= 4 && a.sc * a.ld * (int)sizeof(double) <= bytes,
              "fit_dynamics (wide): no plan for n = %d, m = %d", n, m);
    DDP_CHECK((long)N * B <= 0x7fffffffL, "fit_dynamics (wide): N = %d, B = %d is too large for one launch", N, B);
    if (int rc = ddp_raise_lds(h, (const void *)ddp_fit_dynamics_wide, FW_MAX_LDS)) return rc;
    hipLaunchKernelGGL(ddp_fit_dynamics_wide, dim3((unsigned)((long)N * B)), dim3(256), bytes, h->stream, a);
    DDP_HIP(hipGetLastError());
    return 0;
}

int ddp_fit_dynamics_wide_f64(ddp_handle h, int n, int m, int N, int S, int B, const double *xs, const double *us, double ridge,
                              const double *Phi, const double *mu0, double m0, double n0, int prior_layout, double *fx, double *fu,
                              double *fc, double *cov, int32_t *status)
{
    { const int rc = fit_wide_validate(n, m, N, S, B, xs, us, ridge, Phi, mu0, m0, n0, prior_layout, fx, fu, fc, cov, status); if (rc) return rc; }
    if (fit_wide_in_box(n, m))
        return ddp_fit_dynamics_f64(h, n, m, N, S, B, xs, us, ridge, Phi, mu0, m0, n0, prior_layout, fx, fu, fc, cov, status);
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
    return St.finish(ddp_fit_dynamics_wide_f64_dev(h, n, m, N, S, B, dxs, dus, ridge, dPhi, dmu0, m0, n0, prior_layout, dfx, dfu, dfc, dcov, dstatus));
}

}   // extern "C"
