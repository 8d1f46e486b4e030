// kl_wide.hip — the KL-constrained path for the shapes beyond n <= 32, m <= 8 (ddp_kl_set_wide; any n <= 64, m <= DDP_MAX_M_WIDE):
//   ∇kl                src/klutils.jl:8-23       one work-group per (time step, trajectory), the three products through the LDS
//   forward_covariance src/forward_pass.jl:37-56 one work-group of four waves per trajectory, every product on v_mfma_f64_16x16x4 tiles
//   kl_div_wiki        src/klutils.jl:70-103     one wave per (time step, trajectory), then a fixed-order mean over time
// The kernels of kl.hip keep per-thread arrays sized by the largest n and m (Sik[8], A[64], mu[32], nv[16]); at m = 32 those would be
// kilobytes of scratch per lane.  Here every vector and matrix of a step lives in the LDS and a lane owns one row, column or entry.
// Not tuned: none of this is on the benchmarked path.  back_pass_gps for these shapes is the GPS instantiation of back_pass_wide.hip.
#include "ddp_internal.h"
#include "wide_tile.h"

namespace {

constexpr int KW_MAX_N = 64, KW_MAX_M = DDP_MAX_M_WIDE;
constexpr int KW_T = 256, KW_WAVES = KW_T / DDP_WAVE;

// ------------------------------------------------------------------------------------------------ ∇kl
__global__ __launch_bounds__(KW_T) void kl_terms_wide_kernel(int n, int m, const double *__restrict__ K, const double *__restrict__ k,
                                                             const double *__restrict__ Si, double *__restrict__ cx,
                                                             double *__restrict__ cu, double *__restrict__ cxx,
                                                             double *__restrict__ cxu, double *__restrict__ cuu)
{
    const size_t t = blockIdx.x;                                       // flat (time, trajectory) index
    const int tid = threadIdx.x;
    const size_t nm = (size_t)n * m, mm = (size_t)m * m, nn = (size_t)n * n;
    extern __shared__ double lds[];
    double *S = lds, *Kt = S + m * m, *SK = Kt + m * n, *kv = SK + m * n, *Sk = kv + m;
    for (int e = tid; e < m * m; e += KW_T) { const double v = Si[mm * t + e]; S[e] = v; cuu[mm * t + e] = v; }       // cuu = Σi     (:19)
    for (int e = tid; e < m * n; e += KW_T) Kt[e] = K[nm * t + e];
    if (tid < m) kv[tid] = k[(size_t)m * t + tid];
    __syncthreads();
    for (int e = tid; e < m * n; e += KW_T) {                          // cxu = -Σi K  (:20), m x n
        const int a = e % m, j = e / m;
        double s = 0.0;
        for (int b = 0; b < m; ++b) s += S[a + m * b] * Kt[b + m * j];
        SK[e] = s;
        cxu[nm * t + e] = -s;
    }
    if (tid < m) {                                                     // cu = -Σi k   (:17)
        double s = 0.0;
        for (int b = 0; b < m; ++b) s += S[tid + m * b] * kv[b];
        Sk[tid] = s;
        cu[(size_t)m * t + tid] = -s;
    }
    __syncthreads();
    if (tid < n) {                                                     // cx = K'Σi k  (:16)
        double s = 0.0;
        for (int a = 0; a < m; ++a) s += Kt[a + m * tid] * Sk[a];
        cx[(size_t)n * t + tid] = s;
    }
    for (int e = tid; e < n * n; e += KW_T) {                          // cxx = K'(Σi K)  (:18)
        const int r = e % n, j = e / n;
        double s = 0.0;
        for (int a = 0; a < m; ++a) s += Kt[a + m * r] * SK[a + m * j];
        cxx[nn * t + e] = s;
    }
}

size_t kl_terms_wide_lds(int n, int m) { return ((size_t)m * m + 2 * (size_t)m * n + 2 * (size_t)m) * sizeof(double); }

// ------------------------------------------------------------------------------------------------ forward_covariance
// The LDS holds Σ, fx Σ, fx_i (ldn x n each), K_i and K Σ (ldm x n each), column-major with the leading dimensions of
// back_pass_wide.hip (2 mod 4): 136 KB at (64, 32).  Per step: A) fx Σ, K Σ (:50), Σ K' (:51); B) Σ⁺ = (fx Σ) fx' + R1 (:49, the
// reference's association) into accumulators, K Σ K' + Σ_policy (:52); C) Σ⁺ takes the place of Σ.  The last step has no policy block
// (the loop of :44-53 ends before it): zeros there, as the kernels of kl.hip write.
constexpr int FW_LDS_BYTES = 160 * 1024;
size_t fcov_wide_lds(int n, int m) { return ((size_t)3 * ld4(n) * n + 2 * (size_t)ld4(m) * n) * sizeof(double); }

__global__ __launch_bounds__(KW_T) void fcov_wide_kernel(int n, int m, int N, const double *__restrict__ fx, int fx_batched,
                                                         const double *__restrict__ R1, const double *__restrict__ K,
                                                         const double *__restrict__ Sigma, double *__restrict__ out)
{
    const int b = blockIdx.x, t = threadIdx.x, lane = t & (DDP_WAVE - 1), w = t / DDP_WAVE, l15 = lane & 15, l4 = lane >> 4;
    const int p = n + m, ldn = ld4(n), ldm = ld4(m), NT = cdivw(n, 16), MT = cdivw(m, 16);
    constexpr int QS = cdivw(cdivw(KW_MAX_N, 16) * cdivw(KW_MAX_N, 16), KW_WAVES);      // Σ⁺ tiles per wave
    const size_t nn = (size_t)n * n, nm = (size_t)n * m, mm = (size_t)m * m, pp = (size_t)p * p;
    extern __shared__ double lds[];
    double *S = lds, *T1 = S + ldn * n, *F = T1 + ldn * n, *Kl = F + ldn * n, *KS = Kl + ldm * n;
    const double *fxb = fx + (fx_batched ? nn * N * b : 0), *Kb = K + nm * N * b, *Sgb = Sigma + mm * N * b;
    double *ob = out + pp * N * b;
    const d4 zero = d4{0.0, 0.0, 0.0, 0.0};
    for (int e = t; e < n * n; e += KW_T) S[(e % n) + ldn * (e / n)] = R1[e];                 // Σ0 = R1  (:43)
    __syncthreads();
    for (int i = 0; i < N; ++i) {
        double *oi = ob + pp * i;
        for (int e = t; e < n * n; e += KW_T) oi[(e % n) + p * (e / n)] = S[(e % n) + ldn * (e / n)];     // sigmanew[ix,ix,i]
        if (i == N - 1) {
            for (int e = t; e < m * n; e += KW_T) { const int a = e % m, c = e / m; oi[(n + a) + p * c] = 0.0; oi[c + p * (n + a)] = 0.0; }
            for (int e = t; e < m * m; e += KW_T) oi[(n + e % m) + p * (n + e / m)] = 0.0;
            break;
        }
        for (int e = t; e < n * n; e += KW_T) F[(e % n) + ldn * (e / n)] = fxb[nn * i + e];
        for (int e = t; e < m * n; e += KW_T) Kl[(e % m) + ldm * (e / m)] = Kb[nm * i + e];
        __syncthreads();
        // ---- A: fx Σ -> T1;  K Σ -> KS and sigmanew[iu,ix,i];  Σ K' -> sigmanew[ix,iu,i]
        for (int tt = w; tt < NT * NT + 2 * MT * NT; tt += KW_WAVES) {
            if (tt < NT * NT) {
                const int r0 = 16 * (tt / NT), c0 = 16 * (tt % NT);
                const d4 acc = xty(F, ldn, 1, r0, n, S, 1, ldn, c0, n, n, zero, l15, l4);
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int row = r0 + l4 + 4 * r, col = c0 + l15;
                    if (row < n && col < n) T1[row + ldn * col] = comp(acc, r);
                }
            } else if (tt < NT * NT + MT * NT) {
                const int u = tt - NT * NT, r0 = 16 * (u / NT), c0 = 16 * (u % NT);
                const d4 acc = xty(Kl, ldm, 1, r0, m, S, 1, ldn, c0, n, n, zero, l15, l4);
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int row = r0 + l4 + 4 * r, col = c0 + l15;
                    if (row < m && col < n) { KS[row + ldm * col] = comp(acc, r); oi[(n + row) + p * col] = comp(acc, r); }
                }
            } else {
                const int u = tt - NT * NT - MT * NT, r0 = 16 * (u / MT), c0 = 16 * (u % MT);
                const d4 acc = xty(S, ldn, 1, r0, n, Kl, ldm, 1, c0, m, n, zero, l15, l4);
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int row = r0 + l4 + 4 * r, col = c0 + l15;
                    if (row < n && col < m) oi[row + p * (n + col)] = comp(acc, r);
                }
            }
        }
        __syncthreads();
        // ---- B: Σ⁺ = (fx Σ) fx' + R1 (accumulators);  K Σ K' + Σ_policy -> sigmanew[iu,iu,i]
        d4 nacc[QS];
#pragma unroll
        for (int s = 0; s < QS; ++s) {
            const int tt = w + KW_WAVES * s;
            nacc[s] = zero;
            if (tt < NT * NT) {
                const int r0 = 16 * (tt / NT), c0 = 16 * (tt % NT), col = c0 + l15;
                d4 sd = zero;
                if (col < n) {
                    if (r0 + l4 < n) sd.x = R1[(r0 + l4) + n * col];
                    if (r0 + l4 + 4 < n) sd.y = R1[(r0 + l4 + 4) + n * col];
                    if (r0 + l4 + 8 < n) sd.z = R1[(r0 + l4 + 8) + n * col];
                    if (r0 + l4 + 12 < n) sd.w = R1[(r0 + l4 + 12) + n * col];
                }
                nacc[s] = xty(T1, ldn, 1, r0, n, F, ldn, 1, c0, n, n, sd, l15, l4);
            }
        }
        for (int tt = w; tt < MT * MT; tt += KW_WAVES) {
            const int r0 = 16 * (tt / MT), c0 = 16 * (tt % MT), col = c0 + l15;
            const double *sg = Sgb + mm * i;
            d4 sd = zero;
            if (col < m) {
                if (r0 + l4 < m) sd.x = sg[(r0 + l4) + m * col];
                if (r0 + l4 + 4 < m) sd.y = sg[(r0 + l4 + 4) + m * col];
                if (r0 + l4 + 8 < m) sd.z = sg[(r0 + l4 + 8) + m * col];
                if (r0 + l4 + 12 < m) sd.w = sg[(r0 + l4 + 12) + m * col];
            }
            const d4 acc = xty(KS, ldm, 1, r0, m, Kl, ldm, 1, c0, m, n, sd, l15, l4);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = r0 + l4 + 4 * r;
                if (row < m && col < m) oi[(n + row) + p * (n + col)] = comp(acc, r);
            }
        }
        __syncthreads();                                               // Σ, F, K, K Σ are dead
        // ---- C
#pragma unroll
        for (int s = 0; s < QS; ++s) {
            const int tt = w + KW_WAVES * s;
            if (tt < NT * NT) {
                const int r0 = 16 * (tt / NT), c0 = 16 * (tt % NT), col = c0 + l15;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int row = r0 + l4 + 4 * r;
                    if (row < n && col < n) S[row + ldn * col] = comp(nacc[s], r);
                }
            }
        }
        __syncthreads();
    }
}

// ------------------------------------------------------------------------------------------------ kl_div_wiki
// every lane gets sum_{i < cnt} v_i, added in index order
__device__ __forceinline__ double kw_sum(double v, double *sb, int lane, int cnt)
{
    sb[lane] = v;
    wave_sync();
    double s = 0.0;
    for (int i = 0; i < cnt; ++i) s += sb[i];
    wave_sync();
    return s;
}

// log|det A| and the sign of det A (LU with partial pivoting, like logdet of a Matrix; the sign rule of logabsdet_small in kl.hip),
// one wave: lane j owns column j of the m x m image A (leading dimension m, destroyed).  All lanes return the same values.
__device__ double logabsdet_wave(double *A, int m, int lane, int &sgn)
{
    double *mine = A + m * (lane < m ? lane : 0);
    double s = 0.0;
    sgn = 1;
    for (int c = 0; c < m; ++c) {
        const double *f = A + m * c;
        int pr = c;
        double best = fabs(f[c]);
        for (int r = c + 1; r < m; ++r) {
            const double v = fabs(f[r]);
            if (v > best) { best = v; pr = r; }
        }
        if (best == 0.0) { sgn = 0; return -INFINITY; }
        wave_sync();
        if (pr != c) {
            sgn = -sgn;
            if (lane < m) { const double tsw = mine[c]; mine[c] = mine[pr]; mine[pr] = tsw; }
        }
        wave_sync();
        const double d = f[c];
        if (d < 0.0) sgn = -sgn;
        s += log(fabs(d));
        wave_sync();
        if (lane == c)
            for (int r = c + 1; r < m; ++r) mine[r] = mine[r] / d;      // the multipliers
        wave_sync();
        if (lane > c && lane < m) {
            const double pc = mine[c];
            for (int r = c + 1; r < m; ++r) mine[r] -= f[r] * pc;
        }
        wave_sync();
    }
    return s;
}

size_t kl_div_wide_lds(int n, int m) { return (2 * (size_t)m * n + 2 * (size_t)m * m + 3 * (size_t)m + n + DDP_WAVE) * sizeof(double); }

// one time step of kl_div_wiki (klutils.jl:84-101); a negative determinant (logdet throws a DomainError, :95-99) marks the trajectory's
// klmean with +Inf — every wave that does so stores the same value, and kl_mean_wide_kernel leaves it
__global__ __launch_bounds__(DDP_WAVE) void kl_div_wide_kernel(int n, int m, int N, const double *__restrict__ xnew,
                                                               const double *__restrict__ xold, const double *__restrict__ sig,
                                                               const double *__restrict__ Kn, const double *__restrict__ kn,
                                                               const double *__restrict__ Sn, const double *__restrict__ Kp,
                                                               const double *__restrict__ kp, const double *__restrict__ Sp,
                                                               const double *__restrict__ Sip, double *__restrict__ kldiv,
                                                               double *__restrict__ klmean)
{
    const size_t tb = blockIdx.x;
    const int lane = threadIdx.x, p = n + m;
    const size_t nm = (size_t)n * m, mm = (size_t)m * m, pp = (size_t)p * p;
    extern __shared__ double lds[];
    double *Kd = lds, *SK = Kd + m * n, *Si = SK + m * n, *A = Si + m * m, *kd = A + m * m, *Kmu = kd + m, *SKmu = Kmu + m, *mu = SKmu + m,
           *sb = mu + n;
    const double *Snt = Sn + mm * tb, *Spt = Sp + mm * tb, *St = sig + pp * tb;
    const int la = lane < m ? lane : 0, lc = lane < n ? lane : 0;
    for (int e = lane; e < m * n; e += DDP_WAVE) Kd[e] = Kp[nm * tb + e] - Kn[nm * tb + e];
    for (int e = lane; e < m * m; e += DDP_WAVE) { Si[e] = Sip[mm * tb + e]; A[e] = Spt[e]; }
    if (lane < m) kd[lane] = kp[(size_t)m * tb + lane] - kn[(size_t)m * tb + lane];
    if (lane < n) mu[lane] = xnew[(size_t)n * tb + lane] - xold[(size_t)n * tb + lane];
    wave_sync();
    double ta = 0.0, qa = 0.0;
    if (lane < m)
        for (int c = 0; c < m; ++c) {
            ta += Si[la + m * c] * Snt[c + m * la];                     // tr(Σip Σn)
            qa += kd[la] * Si[la + m * c] * kd[c];                      // k_diff'Σip k_diff
        }
    const double tr1 = kw_sum(ta, sb, lane, m), q1 = kw_sum(qa, sb, lane, m);
    int sp, sn;
    const double ldp = logabsdet_wave(A, m, lane, sp);
    wave_sync();
    for (int e = lane; e < m * m; e += DDP_WAVE) A[e] = Snt[e];
    wave_sync();
    const double ldn = logabsdet_wave(A, m, lane, sn);
    double v = 0.5 * (tr1 + q1 - m + ldp - ldn);                        // :92
    if (lane < m) {
        double s = 0.0;
        for (int j = 0; j < n; ++j) s += Kd[la + m * j] * mu[j];
        Kmu[la] = s;
    }
    wave_sync();
    double q2a = 0.0, q3a = 0.0;
    if (lane < m) {                                                     // Σip K_diff μ
        double s = 0.0;
        for (int c = 0; c < m; ++c) s += Si[la + m * c] * Kmu[c];
        q2a = Kmu[la] * s;
        q3a = kd[la] * s;
    }
    const double q2 = kw_sum(q2a, sb, lane, m), q3 = kw_sum(q3a, sb, lane, m);
    for (int e = lane; e < m * n; e += DDP_WAVE) {                      // Σip K_diff
        const int a = e % m, c = e / m;
        double s = 0.0;
        for (int a2 = 0; a2 < m; ++a2) s += Si[a + m * a2] * Kd[a2 + m * c];
        SK[e] = s;
    }
    wave_sync();
    double tc = 0.0;
    if (lane < n)                                                       // tr(K_diff'Σip K_diff Σt), Σt = sigmanew[1:n,1:n,t]
        for (int r = 0; r < n; ++r) {
            double s = 0.0;
            for (int a = 0; a < m; ++a) s += Kd[a + m * r] * SK[a + m * lc];
            tc += s * St[lc + p * r];
        }
    const double tr2 = kw_sum(tc, sb, lane, n);
    v += 0.5 * (q2 + tr2) + q3;                                         // :93-94
    if (lane == 0) {
        kldiv[tb] = v <= 0.0 ? 0.0 : v;                                 // :101 max(0, v): a NaN stays a NaN
        if (sp < 0 || sn < 0) klmean[tb / (size_t)N] = INFINITY;
    }
}

// klmean[b] = mean_t kldiv[t, b], added in time order by one thread (the second, fixed-order reduction: no atomics, the same bits
// in every run); +Inf where kl_div_wide_kernel left it
__global__ __launch_bounds__(DDP_WAVE) void kl_mean_wide_kernel(int N, int B, const double *__restrict__ kldiv, double *__restrict__ klmean)
{
    const int b = blockIdx.x * DDP_WAVE + threadIdx.x;
    if (b >= B) return;
    double s = 0.0;
    for (int t = 0; t < N; ++t) s += kldiv[(size_t)N * b + t];
    if (!(klmean[b] == INFINITY)) klmean[b] = s / N;
}

bool kw_shape(int n, int m) { return n >= 1 && n <= KW_MAX_N && m >= 1 && m <= KW_MAX_M; }

}   // namespace

int ddp_launch_kl_terms_wide(ddp_handle h, int n, int m, int N, int B, const double *K, const double *k, const double *Sigmai,
                             double *cx, double *cu, double *cxx, double *cxu, double *cuu)
{
    DDP_CHECK(kw_shape(n, m), "kl_terms: n=%d m=%d outside the wide KL kernels (n <= %d, m <= %d)", n, m, KW_MAX_N, KW_MAX_M);
    hipLaunchKernelGGL(kl_terms_wide_kernel, dim3((unsigned)((size_t)N * B)), dim3(KW_T), kl_terms_wide_lds(n, m), h->stream, n, m, K, k, Sigmai,
                       cx, cu, cxx, cxu, cuu);
    DDP_HIP(hipGetLastError());
    return 0;
}

int ddp_launch_fcov_wide(ddp_handle h, int n, int m, int N, int B, const double *fx, int fx_batched, const double *R1, const double *K,
                         const double *Sigma, double *sigmanew)
{
    DDP_CHECK(kw_shape(n, m), "forward_covariance: n=%d m=%d outside the wide KL kernels (n <= %d, m <= %d)", n, m, KW_MAX_N, KW_MAX_M);
    const size_t bytes = fcov_wide_lds(n, m);
    DDP_CHECK(bytes <= (size_t)FW_LDS_BYTES, "forward_covariance: n=%d m=%d needs %zu bytes of LDS (limit %d)", n, m, bytes, FW_LDS_BYTES);
    if (int rc = ddp_raise_lds(h, (const void *)fcov_wide_kernel, FW_LDS_BYTES)) return rc;      // per handle (its device), not per process
    hipLaunchKernelGGL(fcov_wide_kernel, dim3(B), dim3(KW_T), bytes, h->stream, n, m, N, fx, fx_batched, R1, K, Sigma, sigmanew);
    DDP_HIP(hipGetLastError());
    return 0;
}

int ddp_launch_kl_div_wide(ddp_handle h, int n, int m, int N, int B, const double *xnew, const double *xold, const double *sigmanew,
                           const double *Kn, const double *kn, const double *Sn, const double *Kp, const double *kp, const double *Sp,
                           const double *Sip, double *kldiv, double *klmean)
{
    DDP_CHECK(kw_shape(n, m), "kl_div: n=%d m=%d outside the wide KL kernels (n <= %d, m <= %d)", n, m, KW_MAX_N, KW_MAX_M);
    DDP_HIP(hipMemsetAsync(klmean, 0, sizeof(double) * (size_t)B, h->stream));
    hipLaunchKernelGGL(kl_div_wide_kernel, dim3((unsigned)((size_t)N * B)), dim3(DDP_WAVE), kl_div_wide_lds(n, m), h->stream, n, m, N, xnew, xold,
                       sigmanew, Kn, kn, Sn, Kp, kp, Sp, Sip, kldiv, klmean);
    DDP_HIP(hipGetLastError());
    hipLaunchKernelGGL(kl_mean_wide_kernel, dim3((unsigned)((B + DDP_WAVE - 1) / DDP_WAVE)), dim3(DDP_WAVE), 0, h->stream, N, B,
                       (const double *)kldiv, klmean);
    DDP_HIP(hipGetLastError());
    return 0;
}
