// wide_tile.h — the 16 x 16 tile product on v_mfma_f64_16x16x4 with LDS operands and the Gauss-Jordan inverse across the lanes of a
// wave, shared by the four-wave kernels of back_pass_wide.hip and kl_wide.hip.
#pragma once
#include "ddp_internal.h"

namespace {

typedef double d4 __attribute__((ext_vector_type(4)));

__host__ __device__ constexpr int cdivw(int a, int b) { return (a + b - 1) / b; }
// leading dimension for r rows: the smallest ld >= r with ld = 2 (mod 4)
__host__ __device__ constexpr int ld4(int r) { return ((r + 1) & ~3) + 2; }
__host__ __device__ constexpr int imax(int a, int b) { return a > b ? a : b; }
__host__ __device__ constexpr int even(int a) { return (a + 1) & ~1; }

__device__ __forceinline__ d4 mf(double x, double y, d4 c) { return __builtin_amdgcn_mfma_f64_16x16x4f64(x, y, c, 0, 0, 0); }

// acc[i][j] += sum_{k < kn} X(k, i) Y(k, j) on one 16 x 16 tile, i = r0 + (lane & 15) < nr, j = c0 + (lane & 15) < nc; X(k, i) is
// X[k xk + i xi], Y(k, j) is Y[k yk + j yj].  Rows, columns and k outside the ranges contribute exact zeros (their addresses are
// clamped to entries that exist).  Result: component r of lane l is row (l >> 4) + 4 r, column l & 15 of the tile.
__device__ __forceinline__ d4 xty(const double *X, int xk, int xi, int r0, int nr, const double *Y, int yk, int yj, int c0, int nc, int kn,
                                  d4 acc, int l15, int l4)
{
    const int i = r0 + l15, j = c0 + l15;
    const bool iv = i < nr, jv = j < nc;
    const double *xp = X + (iv ? i : 0) * xi, *yp = Y + (jv ? j : 0) * yj;
    for (int k0 = 0; k0 < kn; k0 += 4) {
        const int k = k0 + l4;
        const bool kv = k < kn;
        const int kc = kv ? k : 0;
        const double av = xp[kc * xk], bv = yp[kc * yk];
        acc = mf((iv && kv) ? av : 0.0, (jv && kv) ? bv : 0.0, acc);
    }
    return acc;
}

__device__ __forceinline__ double comp(const d4 &v, int r) { return r == 0 ? v.x : (r == 1 ? v.y : (r == 2 ? v.z : v.w)); }

// doubles of the [A | X | pivot column] image of inv_wave for an m x m matrix with leading dimension ldm
__host__ __device__ constexpr int inv_wave_len(int ldm, int m) { return ldm * (2 * m + 1); }

// X = inv(A) by Gauss-Jordan elimination with partial pivoting (the algorithm of inv_small in back_pass.hip, `inv(Quu[:,:,i])` of
// backward_pass.jl:283,346), one wave, m <= 32.  img holds [A | X | f]: A in columns 0..m-1 (filled by the caller), X in columns
// m..2m-1 (set here), f the pivot column of the current step.  Lane j owns column j of [A | X]: the row swap, the scaling of the pivot
// row and the elimination touch only the lane's own column, and the multipliers come from f.  On return columns m..2m-1 hold inv(A).
__device__ __forceinline__ void inv_wave(double *img, int ldm, int m, int lane)
{
    double *mine = img + ldm * (lane < 2 * m ? lane : 0), *f = img + ldm * 2 * m;
    const bool on = lane < 2 * m;
    if (lane >= m && on)
        for (int r = 0; r < m; ++r) mine[r] = (r == lane - m) ? 1.0 : 0.0;
    wave_sync();
    for (int c = 0; c < m; ++c) {
        if (lane == c)
            for (int r = 0; r < m; ++r) f[r] = mine[r];
        wave_sync();
        int pr = c;
        double best = fabs(f[c]);
        for (int r = c + 1; r < m; ++r) {
            const double v = fabs(f[r]);
            if (v > best) { best = v; pr = r; }
        }
        const double piv = 1.0 / f[pr];
        if (on) {
            const double t = mine[pr];                                  // rows c and pr change places, the pivot row is scaled
            mine[pr] = mine[c];
            const double pc = t * piv;
            mine[c] = pc;
            for (int r = 0; r < m; ++r) {
                if (r == c) continue;
                const double fr = r == pr ? f[c] : f[r];                // the multiplier of row r after the swap
                mine[r] -= fr * pc;
            }
        }
        wave_sync();
    }
}

}   // namespace
