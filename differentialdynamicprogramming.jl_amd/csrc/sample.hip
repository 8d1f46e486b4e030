// sample.hip — the library kernels around ddp_user_sample (user_sample_kernels.h): the noise factor of a Gaussian policy, the sample
// moments of its rollouts, and the normals of philox.h as an array.
//
//   ddp_policy_factor    lower Cholesky L_i L_i' = Σ_i of Sigma[m,m,N,B], one lane per (step, trajectory), the lower triangle read, the
//                        upper triangle of L written as zeros.  status[b] = 0, or i + 1 for the smallest step i whose pivot is not a
//                        positive finite number (an atomic min over the steps, then ddp_policy_status turns "none" into 0).
//                        The reference's docstring says chol(Σ)*randn(m): Julia's chol is the UPPER factor U, and U ξ has covariance
//                        U U', which is not Σ for m > 1.  The lower factor is used here on purpose (L ξ has covariance Σ).
//   ddp_policy_factor_wide  the same contract for 8 < m <= 32 (DDP_USER_SAMPLE_WAVE): a half-wave per matrix, a row per lane, out of LDS;
//                        the m <= 8 kernel is untouched.
//   ddp_sample_moments   xs[n,N,S,B] -> xmean[n,N,B] and the unbiased xcov[n,n,N,B] over the samples: one wave per (step, trajectory),
//                        two passes (the mean, then the centred products).  Lane l sums s = l, l + 64, ..., then a fixed butterfly:
//                        two runs give the same bits.  S = 1: the covariance is 0/0 = NaN.
//   ddp_normal_fill      xi[m,N,S,B]: exactly the normals ddp_user_sample draws for (seed, sample0, traj0).
#include <float.h>
#include <limits.h>
#include "ddp_internal.h"
#include "philox.h"
#include "staging.h"

namespace {

template <int M>
__device__ __forceinline__ int factor_lower(const double *S, double *L)
{
    double l[M * M];
    int fail = 0;
#pragma unroll
    for (int e = 0; e < M * M; ++e) l[e] = 0.0;
#pragma unroll
    for (int c = 0; c < M; ++c) {
        double d = S[c + M * c];
#pragma unroll
        for (int k = 0; k < c; ++k) d -= l[c + M * k] * l[c + M * k];
        if (!(d > 0.0 && d <= DBL_MAX) && fail == 0) fail = c + 1;
        const double r = sqrt(d);
        l[c + M * c] = r;
#pragma unroll
        for (int q = c + 1; q < M; ++q) {
            double s = S[q + M * c];
#pragma unroll
            for (int k = 0; k < c; ++k) s -= l[q + M * k] * l[c + M * k];
            l[q + M * c] = s / r;
        }
    }
#pragma unroll
    for (int e = 0; e < M * M; ++e) L[e] = l[e];
    return fail;
}

template <int M>
__global__ __launch_bounds__(64) void ddp_policy_factor(int N, int B, const double *Sigma, double *L, int32_t *status)
{
    const long r = (long)blockIdx.x * 64 + threadIdx.x;
    if (r >= (long)N * B) return;
    const int b = (int)(r / N), i = (int)(r - (long)b * N);
    if (factor_lower<M>(Sigma + (size_t)M * M * r, L + (size_t)M * M * r)) atomicMin(status + b, i + 1);
}

// 8 < m <= 32: two matrices per wave, a half-wave each, lane q of the half owning row q of the factor; the matrix lives in LDS, column-major
// at stride m (the lanes of a half read consecutive addresses, the pivot row is a broadcast), and is factored in place.  The order is
// factor_lower's, left-looking: column c = 0..m-1; d = S[c,c] - Σ_k l[c,k]² and s = S[q,c] - Σ_k l[q,k] l[c,k] with k = 0..c-1 ascending;
// l[c,c] = sqrt(d), l[q,c] = s / l[c,c].  Every lane forms d itself from the broadcast row (the same bits in every lane).  Entries above
// the diagonal come into LDS with the rest but enter no sum, and leave as zeros.
__global__ __launch_bounds__(64) void ddp_policy_factor_wide(int m, int N, int B, const double *Sigma, double *L, int32_t *status)
{
    __shared__ double lds[2][DDP_MAX_M_WIDE * DDP_MAX_M_WIDE];
    const int half = threadIdx.x >> 5, q = threadIdx.x & 31, mm = m * m;
    const long r = (long)blockIdx.x * 2 + half;
    const bool act = r < (long)N * B;
    double *l = lds[half];
    if (act)
        for (int e = q; e < mm; e += 32) l[e] = Sigma[(size_t)mm * r + e];
    __syncthreads();
    int fail = 0;
    for (int c = 0; c < m; ++c) {
        double lqc = 0.0;
        if (act) {
            double d = l[c + m * c];
            for (int k = 0; k < c; ++k) d -= l[c + m * k] * l[c + m * k];
            if (!(d > 0.0 && d <= DBL_MAX) && fail == 0) fail = c + 1;
            const double rt = sqrt(d);
            if (q == c) lqc = rt;
            else if (q > c && q < m) {
                double s = l[q + m * c];
                for (int k = 0; k < c; ++k) s -= l[q + m * k] * l[c + m * k];
                lqc = s / rt;
            }
        }
        __syncthreads();                                         // (every read of column c's old values and of the diagonal is done)
        if (act && q < m) l[q + m * c] = lqc;
        __syncthreads();
    }
    if (act) {
        for (int e = q; e < mm; e += 32) L[(size_t)mm * r + e] = l[e];
        if (fail && q == 0) atomicMin(status + (int)(r / N), (int)(r % N) + 1);
    }
}

__global__ void ddp_policy_status(int B, int32_t *status, int first)
{
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    status[b] = first ? INT_MAX : (status[b] == INT_MAX ? 0 : status[b]);
}

__device__ __forceinline__ double wave_sum(double v)            // a fixed butterfly: every lane ends with the same bits
{
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

__global__ __launch_bounds__(64) void ddp_sample_moments(int n, int N, int S, int B, const double *xs, double *xmean, double *xcov)
{
    __shared__ double mean[DDP_MAX_N_USER_WAVE];
    const long r = blockIdx.x;                                  // (step, trajectory)
    const int lane = threadIdx.x, b = (int)(r / N), i = (int)(r - (long)b * N);
    const double *x = xs + (size_t)n * ((size_t)N * S * b + i);  // sample s: x + n N s
    const size_t ss = (size_t)n * N;
    for (int l = 0; l < n; ++l) {
        double acc = 0.0;
        for (int s = lane; s < S; s += 64) acc += x[ss * s + l];
        const double mu = wave_sum(acc) / (double)S;
        if (lane == 0) { mean[l] = mu; if (xmean) xmean[(size_t)n * r + l] = mu; }
    }
    __syncthreads();
    if (!xcov) return;
    for (int c = 0; c < n; ++c)
        for (int q = 0; q <= c; ++q) {
            const double mq = mean[q], mc = mean[c];
            double acc = 0.0;
            for (int s = lane; s < S; s += 64) acc += (x[ss * s + q] - mq) * (x[ss * s + c] - mc);
            const double v = wave_sum(acc) / (double)(S - 1);
            if (lane == 0) { xcov[(size_t)n * n * r + q + n * c] = v; xcov[(size_t)n * n * r + c + n * q] = v; }
        }
}

__global__ __launch_bounds__(256) void ddp_normal_fill(int seed_lo, int seed_hi, int m, int N, int S, int B, int sample0, int traj0, double *xi)
{
    const int mp = (m + 1) / 2;
    const size_t total = (size_t)mp * N * S * B, g = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (g >= total) return;
    const int q = (int)(g % mp);
    const size_t r = g / mp;                                     // i + N (s + S b)
    const int i = (int)(r % N);
    const size_t sb = r / N;
    const int s = (int)(sb % S), b = (int)(sb / S);
    double z0, z1;
    ddp_normal_pair((unsigned)seed_lo, (unsigned)seed_hi, i, sample0 + s, traj0 + b, q, z0, z1);
    xi[(size_t)m * r + 2 * q] = z0;
    if (2 * q + 1 < m) xi[(size_t)m * r + 2 * q + 1] = z1;
}

}   // namespace

int ddp_policy_factor_dev(ddp_handle h, int m, int N, int B, const double *Sigma, double *L, int32_t *status)
{
    DDP_CHECK(m >= 1 && m <= DDP_MAX_M_WIDE, "policy_factor: m = %d out of [1, %d]", m, DDP_MAX_M_WIDE);
    DDP_CHECK(((long)N * B + 63) / 64 <= 0x7fffffffL, "policy_factor: N = %d, B = %d is too large for one launch", N, B);
    const unsigned gb = (unsigned)((B + 255) / 256), gr = (unsigned)(((long)N * B + 63) / 64);
    hipLaunchKernelGGL(ddp_policy_status, dim3(gb), dim3(256), 0, h->stream, B, status, 1);
    switch (m) {
#define DDP_FACTOR_CASE(M) case M: hipLaunchKernelGGL(ddp_policy_factor<M>, dim3(gr), dim3(64), 0, h->stream, N, B, Sigma, L, status); break;
        DDP_FACTOR_CASE(1) DDP_FACTOR_CASE(2) DDP_FACTOR_CASE(3) DDP_FACTOR_CASE(4) DDP_FACTOR_CASE(5) DDP_FACTOR_CASE(6) DDP_FACTOR_CASE(7)
        DDP_FACTOR_CASE(8)
#undef DDP_FACTOR_CASE
    default:                                                     // 8 < m <= 32
        hipLaunchKernelGGL(ddp_policy_factor_wide, dim3((unsigned)(((long)N * B + 1) / 2)), dim3(64), 0, h->stream, m, N, B, Sigma, L, status);
    }
    hipLaunchKernelGGL(ddp_policy_status, dim3(gb), dim3(256), 0, h->stream, B, status, 0);
    DDP_HIP(hipGetLastError());
    return 0;
}

int ddp_sample_moments_dev(ddp_handle h, int n, int N, int S, int B, const double *xs, double *xmean, double *xcov)
{
    DDP_CHECK(n >= 1 && n <= DDP_MAX_N_USER_WAVE, "sample_moments: n = %d out of [1, %d]", n, DDP_MAX_N_USER_WAVE);
    DDP_CHECK((long)N * B <= 0x7fffffffL, "sample_moments: N = %d, B = %d is too large for one launch", N, B);
    hipLaunchKernelGGL(ddp_sample_moments, dim3((unsigned)((long)N * B)), dim3(64), 0, h->stream, n, N, S, B, xs, xmean, xcov);
    DDP_HIP(hipGetLastError());
    return 0;
}

extern "C" {

int ddp_normal_f64_dev(ddp_handle h, int seed_lo, int seed_hi, int m, int N, int S, int B, int sample0, int traj0, double *xi)
{
    DDP_DEVICE(h);
    DDP_CHECK(m >= 1 && N >= 1 && S >= 1 && B >= 1, "normal: m = %d, N = %d, S = %d, B = %d (all >= 1)", m, N, S, B);
    DDP_CHECK(sample0 >= 0 && traj0 >= 0, "normal: sample0 = %d, traj0 = %d (both >= 0)", sample0, traj0);
    DDP_CHECK(xi, "normal: null argument");
    const size_t total = (size_t)((m + 1) / 2) * N * S * B;
    DDP_CHECK((total + 255) / 256 <= 0x7fffffffu, "normal: m = %d, N = %d, S = %d, B = %d is too large for one launch", m, N, S, B);
    hipLaunchKernelGGL(ddp_normal_fill, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, h->stream, seed_lo, seed_hi, m, N, S, B, sample0,
                       traj0, xi);
    DDP_HIP(hipGetLastError());
    return 0;
}

int ddp_normal_f64(ddp_handle h, int seed_lo, int seed_hi, int m, int N, int S, int B, int sample0, int traj0, double *xi)
{
    DDP_DEVICE(h);
    DDP_CHECK(m >= 1 && N >= 1 && S >= 1 && B >= 1, "normal: m = %d, N = %d, S = %d, B = %d (all >= 1)", m, N, S, B);
    DDP_CHECK(xi, "normal: null argument");
    double *dxi;
    Staging St(h, Staging::OWNED, "normal");
    St.out(&dxi, xi, (size_t)m * N * S * B);
    int rc = St.commit();
    if (rc) return rc;
    return St.finish(ddp_normal_f64_dev(h, seed_lo, seed_hi, m, N, S, B, sample0, traj0, dxi));
}

}   // extern "C"
