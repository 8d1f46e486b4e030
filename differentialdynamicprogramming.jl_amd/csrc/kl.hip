// kl.hip — the KL-constrained path around back_pass_gps (BASELINE config 5):
//   ∇kl                src/klutils.jl:8-23       one lane per (time step, trajectory)
//   forward_covariance src/forward_pass.jl:37-56 one wave per trajectory, the discrete Lyapunov chain Σ⁺ = fx Σ fx' + R1
//   kl_div_wiki        src/klutils.jl:70-103     one wave per trajectory, lanes over time, mean over time in the wave
// plus the C-ABI entry points of the four KL calls (the back_pass_gps kernels: the GPS variants of back_pass.hip and back_pass_mid.hip,
// the n = 4 ones of back_pass_q4.hip and back_pass_gps_lane.hip; gps_choose below chooses) and the iLQGkl driver for registered and
// user problems.
// None of this is on the benchmarked path; the kernels are written for clarity and coalescing, not tuned.
#include <float.h>
#include <stdlib.h>
#include <vector>
#include <type_traits>
#include "ddp_internal.h"
#include "ilqg_model.h"
#include "kl_workspace.h"
#include "staging.h"

namespace {

constexpr int NMAXK = DDP_MAX_N_GENERIC, MMAXK = DDP_MAX_M;
constexpr int KL_WIDE_MAX_N = 64;        // with ddp_kl_set_wide: n <= 64, m <= DDP_MAX_M_WIDE (kl_wide.hip, back_pass_wide.hip)

// ------------------------------------------------------------------------------------------------ ∇kl
__global__ void kl_terms_kernel(int n, int m, long NB, const double *__restrict__ K, const double *__restrict__ k,
                                const double *__restrict__ Si, double *__restrict__ cx, double *__restrict__ cu,
                                double *__restrict__ cxx, double *__restrict__ cxu, double *__restrict__ cuu)
{
    const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;       // flat (time, trajectory) index
    if (t >= NB) return;
    const size_t nm = (size_t)n * m, mm = (size_t)m * m, nn = (size_t)n * n;
    const double *Kt = K + nm * t, *kt = k + (size_t)m * t, *S = Si + mm * t;
    double Sik[MMAXK];
    for (int a = 0; a < m; ++a) {
        double s = 0.0;
        for (int b = 0; b < m; ++b) s += S[a + m * b] * kt[b];
        Sik[a] = s;
        cu[(size_t)m * t + a] = -s;                                    // cu = -Σi k   (:17)
    }
    for (size_t e = 0; e < mm; ++e) cuu[mm * t + e] = S[e];           // cuu = Σi     (:19)
    for (int j = 0; j < n; ++j) {
        double SiKj[MMAXK];
        for (int a = 0; a < m; ++a) {
            double s = 0.0;
            for (int b = 0; b < m; ++b) s += S[a + m * b] * Kt[b + m * j];
            SiKj[a] = s;
            cxu[nm * t + a + m * j] = -s;                              // cxu = -Σi K  (:20), m x n
        }
        double sx = 0.0;
        for (int a = 0; a < m; ++a) sx += Kt[a + m * j] * Sik[a];
        cx[(size_t)n * t + j] = sx;                                    // cx = K'Σi k  (:16)
        for (int r = 0; r < n; ++r) {                                  // cxx[:, j] = K'(Σi K[:, j])  (:18)
            double s = 0.0;
            for (int a = 0; a < m; ++a) s += Kt[a + m * r] * SiKj[a];
            cxx[nn * t + r + n * j] = s;
        }
    }
}

// ------------------------------------------------------------------------------------------------ forward_covariance
__global__ __launch_bounds__(DDP_WAVE) void fcov_kernel(int n, int m, int N, const double *__restrict__ fx, int fx_batched,
                                                        const double *__restrict__ R1, const double *__restrict__ K,
                                                        const double *__restrict__ Sigma, double *__restrict__ out)
{
    const int b = blockIdx.x, lane = threadIdx.x, p = n + m;
    const size_t nn = (size_t)n * n, nm = (size_t)n * m, mm = (size_t)m * m, pp = (size_t)p * p;
    extern __shared__ double lds[];
    double *S = lds, *T1 = S + nn, *F = T1 + nn, *Kl = F + nn, *KS = Kl + nm;      // Σxx, F·Σ, fx_i, K_i, K·Σ
    const double *fxb = fx + (fx_batched ? nn * N * b : 0), *Kb = K + nm * N * b, *Sgb = Sigma + mm * N * b;
    double *ob = out + pp * N * b;
    for (int e = lane; e < n * n; e += DDP_WAVE) S[e] = R1[e];                    // Σ0 = R1  (:43)
    for (size_t e = lane; e < pp * N; e += DDP_WAVE) ob[e] = 0.0;
    wave_sync();
    for (int i = 0; i < N; ++i) {
        double *oi = ob + pp * i;
        for (int e = lane; e < n * n; e += DDP_WAVE) oi[(e % n) + p * (e / n)] = S[e];        // sigmanew[ix,ix,i]
        if (i == N - 1) break;
        for (int e = lane; e < n * n; e += DDP_WAVE) F[e] = fxb[nn * i + e];
        for (int e = lane; e < n * m; e += DDP_WAVE) Kl[e] = Kb[nm * i + e];
        wave_sync();
        for (int e = lane; e < n * n; e += DDP_WAVE) {                                        // T1 = fx·Σ
            const int r = e % n, c = e / n;
            double s = 0.0;
            for (int l = 0; l < n; ++l) s += F[r + n * l] * S[l + n * c];
            T1[e] = s;
        }
        for (int e = lane; e < n * m; e += DDP_WAVE) {                                        // K·Σ  (:50) and Σ·K' (:51)
            const int a = e % m, c = e / m;
            double s = 0.0, s2 = 0.0;
            for (int l = 0; l < n; ++l) { s += Kl[a + m * l] * S[l + n * c]; s2 += S[c + n * l] * Kl[a + m * l]; }
            KS[e] = s;
            oi[(n + a) + p * c] = s;
            oi[c + p * (n + a)] = s2;
        }
        wave_sync();
        for (int e = lane; e < m * m; e += DDP_WAVE) {                                        // K Σ K' + Σ_policy  (:52)
            const int a = e % m, bb = e / m;
            double s = 0.0;
            for (int l = 0; l < n; ++l) s += KS[a + m * l] * Kl[bb + m * l];
            oi[(n + a) + p * (n + bb)] = s + Sgb[mm * i + e];
        }
        double nv[(NMAXK * NMAXK + DDP_WAVE - 1) / DDP_WAVE];
#pragma unroll
        for (int q = 0; q < (NMAXK * NMAXK + DDP_WAVE - 1) / DDP_WAVE; ++q) {                 // Σ⁺ = T1·fx' + R1  (:49)
            const int e = lane + DDP_WAVE * q;
            nv[q] = 0.0;
            if (e < n * n) {
                const int r = e % n, c = e / n;
                double s = 0.0;
                for (int l = 0; l < n; ++l) s += T1[r + n * l] * F[c + n * l];
                nv[q] = s + R1[e];
            }
        }
        wave_sync();
#pragma unroll
        for (int q = 0; q < (NMAXK * NMAXK + DDP_WAVE - 1) / DDP_WAVE; ++q) {
            const int e = lane + DDP_WAVE * q;
            if (e < n * n) S[e] = nv[q];
        }
        wave_sync();
    }
}


// ------------------------------------------------------------------------------------------------ forward_covariance, n = 4
// The C5 shape on the fp64 matrix cores, as the backward pass of back_pass_q4.hip: ONE TRAJECTORY PER BLOCK of v_mfma_f64_4x4x4_4b, four
// per wave, every 4x4 matrix one element per lane ([r][c] in lane 16 r + 4 blk + c), mm(X, Y, C) = X'Y + C per block.  The chain
// Σ -> Σ⁺ = (fx Σ) fx' + R1 (forward_pass.jl:49, the reference's association) is three dependent products per step — T = X1'Σ with
// X1 = fx' (the load picks the lanes), T' = T'·I, Σ⁺ = (T')'X1 + R1 — against ~2 500 cycles per step of the run-time-sized kernel above
// (one wave per trajectory, operands through the LDS, three hand-offs).  Off the chain: KΣ = Kt'Σ, ΣK' = (Σ')'Kt, (KΣ)K' + Σ_policy
// with the transposes again by products with (shifted) identities; Kt holds K' in its columns 0..m-1 AND m..2m-1, so the last product
// lands in lanes [m+a][m+b], which no other result uses: three stores per step (Σ | KΣ and KΣK' | ΣK').
__device__ const double fcov_zeros[2] = {0.0, 0.0};

template <int M>
__global__ __launch_bounds__(DDP_WAVE) void fcov_q4_kernel(int N, int B, const double *__restrict__ fx, int fx_batched,
                                                           const double *__restrict__ R1, const double *__restrict__ K,
                                                           const double *__restrict__ Sigma, double *__restrict__ out, double *__restrict__ sink)
{
    constexpr int n = 4, p = n + M, pp = p * p, D = 6;
    const int lane = threadIdx.x, r = lane >> 4, blk = (lane >> 2) & 3, c = lane & 3;
    long tb = (long)blockIdx.x * 4 + blk;
    const bool valid = tb < B;
    if (!valid) tb = B - 1;                                     // idle blocks repeat the last trajectory (their stores go to the sink)
    const size_t b = (size_t)tb;
    auto mm = [](double a_, double b_, double c_) { return __builtin_amdgcn_mfma_f64_4x4x4f64(a_, b_, c_, 0, 0, 0); };
    // ---- per-lane operand streams (pointer to this lane's entry of step 0, bytes per step); lanes without an entry read a zero
    const char *pX = (const char *)(fx + (fx_batched ? (size_t)n * n * N * b : 0) + (c + n * r));      // X1[r][c] = fx[c, r]
    const bool hasK = c < 2 * M;                                                                        // Kt[r][c] = K[c mod M, r]
    const char *pK = hasK ? (const char *)(K + (size_t)M * n * N * b + (c % M) + M * r) : (const char *)fcov_zeros;
    const unsigned sK = hasK ? M * n * 8u : 0u;
    const bool hasS = r >= M && r < 2 * M && c >= M && c < 2 * M;                                       // Σ_policy[a, b] in lane [M+a][M+b]
    const char *pS = hasS ? (const char *)(Sigma + (size_t)M * M * N * b + (r - M) + M * (c - M)) : (const char *)fcov_zeros;
    const unsigned sS = hasS ? M * M * 8u : 0u;
    // ---- per-lane result streams: sigmanew[ix,ix] = Σ | [iu,ix] = KΣ and [iu,iu] | [ix,iu] = ΣK'
    double *ob = out + (size_t)pp * N * b;
    const bool st2 = r < M || hasS, st3 = c < M;
    char *q1 = valid ? (char *)(ob + r + p * c) : (char *)(sink + lane);
    char *q2 = (valid && st2) ? (char *)(ob + (r < M ? (n + r) + p * c : (n + r - M) + p * (n + c - M))) : (char *)(sink + lane);
    char *q3 = (valid && st3) ? (char *)(ob + r + p * (n + c)) : (char *)(sink + lane);
    const unsigned s1 = valid ? pp * 8u : 0u, s2 = (valid && st2) ? pp * 8u : 0u, s3 = (valid && st3) ? pp * 8u : 0u;
    const bool isU1 = r < M;
    const double I = r == c ? 1.0 : 0.0, Ish = c == r + M ? 1.0 : 0.0;
    const double R1L = R1[r + n * c];
    double S = R1L;                                                                                    // Σ0 = R1 (forward_pass.jl:43)
    struct Ops { double X1, Kt, Sp; };
    auto fetch = [&](int i, Ops &o) {
        o.X1 = *(const double *)(pX + (size_t)(n * n * 8u) * (unsigned)i);
        o.Kt = *(const double *)(pK + (size_t)sK * (unsigned)i);
        o.Sp = *(const double *)(pS + (size_t)sS * (unsigned)i);
    };
    auto step = [&](int i, const Ops &o) __attribute__((always_inline)) {
        *(double *)(q1 + (size_t)s1 * (unsigned)i) = S;                                                // sigmanew[ix,ix,i] (:45)
        const double T = mm(o.X1, S, 0.0);                                                             // fx Σ
        const double U1 = mm(o.Kt, S, 0.0);                                                            // K Σ          (:50)
        const double St = mm(S, I, 0.0);                                                               // Σ'
        const double Tt = mm(T, I, 0.0);                                                               // (fx Σ)'
        const double U1s = mm(U1, Ish, 0.0);                                                           // (K Σ)' shifted by M columns
        const double U2 = mm(St, o.Kt, 0.0);                                                           // Σ K'         (:51)
        const double Sn = mm(Tt, o.X1, R1L);                                                           // (fx Σ) fx' + R1 (:49)
        const double U3 = mm(U1s, o.Kt, o.Sp);                                                         // K Σ K' + Σ_policy (:52)
        *(double *)(q2 + (size_t)s2 * (unsigned)i) = isU1 ? U1 : U3;
        *(double *)(q3 + (size_t)s3 * (unsigned)i) = U2;
        S = Sn;
    };
    Ops ring[D];
#pragma unroll
    for (int d = 0; d < D; ++d) fetch(d < N ? d : N - 1, ring[d]);
    int i0 = 0;
    for (; i0 + 2 * D <= N - 1; i0 += D) {
#pragma unroll
        for (int d = 0; d < D; ++d) {
            step(i0 + d, ring[d]);
            fetch(i0 + d + D, ring[d]);
        }
    }
    for (; i0 < N - 1; i0 += D) {
#pragma unroll
        for (int d = 0; d < D; ++d) {
            const int i = i0 + d;
            if (i < N - 1) {
                step(i, ring[d]);
                fetch(i + D < N ? i + D : N - 1, ring[d]);
            }
        }
    }
    // the last step has no policy block (the loop of forward_pass.jl:44-53 ends before it): Σ, zeros elsewhere
    *(double *)(q1 + (size_t)s1 * (unsigned)(N - 1)) = S;
    *(double *)(q2 + (size_t)s2 * (unsigned)(N - 1)) = 0.0;
    *(double *)(q3 + (size_t)s3 * (unsigned)(N - 1)) = 0.0;
}

// ---- the same chain with CHUNKS OF EIGHT TIME STEPS THROUGH THE LDS (m = 1, N a multiple of 8; the scheme of back_pass_q4l_kernel): the kernel
// above issues three 8-byte loads and three 8-byte stores per step — ~60 issue cycles each for the lone wave this batch gives a SIMD, 0.40 ms
// for 0.9 GB.  Here six direct-to-LDS loads fetch fx (four pieces), K, Σ_policy of 8 steps x 4 trajectories a chunk ahead, the 25 entries of
// sigmanew[:,:,i] are assembled as one record per step in the LDS and leave as 16-byte pieces that are contiguous across the lanes (seven
// stores per chunk); per step the wave issues 3 LDS reads + 3 LDS writes (lanes without an entry read zeros / write to a dump area).
constexpr int FQL_CH = 8, FQL_IK = 512, FQL_IS = 640, FQL_IN = 768;          // in: fx [4 pieces][4 traj][32] | K [4][32] | Σ_policy [4][32] (8 used)
constexpr int FQL_REC = 25, FQL_OT = FQL_CH * FQL_REC, FQL_DUMP = 4 * FQL_OT, FQL_OUT = FQL_DUMP + 64 + FQL_REC * (FQL_CH - 1) + 1;
typedef __attribute__((address_space(3))) void fq_lds_void;
typedef const __attribute__((address_space(1))) void fq_glb_void;
typedef double fq_d2 __attribute__((ext_vector_type(2)));

__global__ __launch_bounds__(DDP_WAVE) void fcov_q4l_kernel(int N, int B, const double *__restrict__ fx, int fx_batched,
                                                            const double *__restrict__ R1, const double *__restrict__ K,
                                                            const double *__restrict__ Sigma, double *__restrict__ out, double *__restrict__ sink)
{
    constexpr int n = 4, M = 1, CH = FQL_CH;
    __shared__ __attribute__((aligned(16))) double lin[2][FQL_IN];
    __shared__ __attribute__((aligned(16))) double lout[FQL_OUT];
    __shared__ __attribute__((aligned(16))) double lzero[32];
    const int lane = threadIdx.x, r = lane >> 4, blk = (lane >> 2) & 3, c = lane & 3;
    const int NC = N / CH;
    if (lane < 32) lzero[lane] = 0.0;
    auto mm = [](double a_, double b_, double c_) { return __builtin_amdgcn_mfma_f64_4x4x4f64(a_, b_, c_, 0, 0, 0); };
    // ---- global side: lane = (trajectory tl, 16-byte piece q) of the lane-linear image
    const int tl = lane >> 4, q = lane & 15;
    long tbd = (long)blockIdx.x * 4 + tl;
    const bool validd = tbd < B;
    if (!validd) tbd = B - 1;
    const size_t bd = (size_t)tbd;
    const double *gfx = fx + (fx_batched ? (size_t)n * n * N * bd : 0) + 2 * q, *gK = K + (size_t)n * N * bd + 2 * q;
    const double *gS = Sigma + (size_t)N * bd + 2 * (q & 3);
    auto dma = [&](int ch, double *in) {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            __builtin_amdgcn_global_load_lds((fq_glb_void *)(gfx + (size_t)ch * (16 * CH) + 32 * j), (fq_lds_void *)(in + 128 * j), 16, 0, 0);
        __builtin_amdgcn_global_load_lds((fq_glb_void *)(gK + (size_t)ch * (4 * CH)), (fq_lds_void *)(in + FQL_IK), 16, 0, 0);
        if (q < 4) __builtin_amdgcn_global_load_lds((fq_glb_void *)(gS + (size_t)ch * CH), (fq_lds_void *)(in + FQL_IS), 16, 0, 0);
    };
    // results: 4 trajectories x 8 steps x 25 doubles = 400 16-byte pieces per chunk, piece idx = 64 pass + lane (the last pass repeats piece 399)
    constexpr int NPS = (4 * FQL_OT / 2 + DDP_WAVE - 1) / DDP_WAVE;
    int dl[NPS];
    double *dg[NPS];
    size_t dstep[NPS];
#pragma unroll
    for (int ps = 0; ps < NPS; ++ps) {
        const int idx0 = ps * DDP_WAVE + lane, idx = idx0 < 4 * FQL_OT / 2 ? idx0 : 4 * FQL_OT / 2 - 1;
        const int t = idx / (FQL_OT / 2), pc = idx % (FQL_OT / 2);
        const long tb = (long)blockIdx.x * 4 + t;
        const bool on = tb < B;
        dl[ps] = t * FQL_OT + 2 * pc;
        dg[ps] = on ? out + (size_t)FQL_REC * N * (size_t)tb + 2 * pc : sink + 2 * lane;
        dstep[ps] = on ? (size_t)FQL_OT : 0;
    }
    auto drain = [&](int ch) {
        fq_d2 v[NPS];
#pragma unroll
        for (int ps = 0; ps < NPS; ++ps) v[ps] = *(const fq_d2 *)(lout + dl[ps]);
#pragma unroll
        for (int ps = 0; ps < NPS; ++ps) *(fq_d2 *)(dg[ps] + dstep[ps] * (size_t)ch) = v[ps];
    };
    // ---- compute side: per-lane LDS offsets (doubles); lanes without an operand read zeros, lanes without a result write to the dump area
    const int ox = 32 * blk + c + n * r;                                                             // X1[r][c] = fx[c, r]
    const bool hasK = c < 2 * M, hasS = r == M && c == M;
    const double *kb = hasK ? nullptr : lzero, *sb = hasS ? nullptr : lzero;                         // (selected per buffer below)
    const int okk = FQL_IK + 32 * blk + r, oss = FQL_IS + 32 * blk;
    double *w1 = lout + blk * FQL_OT + r + 5 * c;                                                    // sigmanew[ix,ix] = Σ
    double *w2 = (r == 0) ? lout + blk * FQL_OT + 4 + 5 * c : hasS ? lout + blk * FQL_OT + 24 : lout + FQL_DUMP + lane;      // [iu,ix] = KΣ | [iu,iu]
    double *w3 = (c == 0) ? lout + blk * FQL_OT + 20 + r : lout + FQL_DUMP + lane;                   // [ix,iu] = ΣK'
    const bool isU1 = r < M;
    const double I = r == c ? 1.0 : 0.0, Ish = c == r + M ? 1.0 : 0.0;
    const double R1L = R1[r + n * c];
    double S = R1L;                                                                                  // Σ0 = R1 (forward_pass.jl:43)
    struct Ops { double X1, Kt, Sp; };
    auto readin = [&](const double *in, int sidx, Ops &o) __attribute__((always_inline)) {
        o.X1 = in[ox + 128 * (sidx >> 1) + 16 * (sidx & 1)];
        o.Kt = (kb ? kb : in + okk)[4 * sidx];
        o.Sp = (sb ? sb : in + oss)[sidx];
    };
    double *cur = lin[0], *nxt = lin[1];
    dma(0, cur);
    if (NC > 1) dma(1, nxt);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    Ops in;
    readin(cur, 0, in);
    for (int ch = 0; ch < NC; ++ch) {
#pragma unroll
        for (int sidx = 0; sidx < CH; ++sidx) {
            Ops nx;
            if (sidx < CH - 1) readin(cur, sidx + 1, nx);
            else {
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");       // the next chunk was requested a whole chunk ago
                readin(nxt, 0, nx);
            }
            w1[FQL_REC * sidx] = S;                                                                    // sigmanew[ix,ix,i] (:45)
            if (sidx == CH - 1 && ch == NC - 1) {
                // the last step has no policy block (the loop of forward_pass.jl:44-53 ends before it): Σ, zeros elsewhere
                w2[FQL_REC * sidx] = 0.0;
                w3[FQL_REC * sidx] = 0.0;
            } else {
                const double T = mm(in.X1, S, 0.0);                                                    // fx Σ
                const double U1 = mm(in.Kt, S, 0.0);                                                   // K Σ          (:50)
                const double St = mm(S, I, 0.0);                                                       // Σ'
                const double Tt = mm(T, I, 0.0);                                                       // (fx Σ)'
                const double U1s = mm(U1, Ish, 0.0);                                                   // (K Σ)' shifted by M columns
                const double U2 = mm(St, in.Kt, 0.0);                                                  // Σ K'         (:51)
                const double Sn = mm(Tt, in.X1, R1L);                                                  // (fx Σ) fx' + R1 (:49)
                const double U3 = mm(U1s, in.Kt, in.Sp);                                               // K Σ K' + Σ_policy (:52)
                w2[FQL_REC * sidx] = isU1 ? U1 : U3;
                w3[FQL_REC * sidx] = U2;
                S = Sn;
            }
            in = nx;
        }
        drain(ch);
        if (ch + 2 < NC) dma(ch + 2, cur);
        double *t = cur; cur = nxt; nxt = t;
    }
}

// ------------------------------------------------------------------------------------------------ kl_div_wiki
// log|det A| and the sign of det A for the leading m x m block (LU with partial pivoting, like logdet of a Matrix)
__device__ __forceinline__ double logabsdet_small(int m, const double *Ain, int &sgn)
{
    double A[MMAXK * MMAXK];
    for (int e = 0; e < m * m; ++e) A[e] = Ain[e];
    double s = 0.0;
    sgn = 1;
    for (int c = 0; c < m; ++c) {
        int pr = c; double best = fabs(A[c + m * c]);
        for (int r = c + 1; r < m; ++r) if (fabs(A[r + m * c]) > best) { best = fabs(A[r + m * c]); pr = r; }
        if (best == 0.0) { sgn = 0; return -INFINITY; }
        if (pr != c) {
            sgn = -sgn;
            for (int j = 0; j < m; ++j) { const double t = A[c + m * j]; A[c + m * j] = A[pr + m * j]; A[pr + m * j] = t; }
        }
        const double d = A[c + m * c];
        if (d < 0.0) sgn = -sgn;
        s += log(fabs(d));
        for (int r = c + 1; r < m; ++r) {
            const double f = A[r + m * c] / d;
            for (int j = c + 1; j < m; ++j) A[r + m * j] -= f * A[c + m * j];
        }
    }
    return s;
}

// one time step of kl_div_wiki (klutils.jl:84-101) from the step's own slices of the ten arrays (global memory or an LDS image)
template <int NC = 0, int MC = 0>
__device__ __forceinline__ double kl_div_step(int n_, int m_, const double *xn, const double *xo, const double *St, const double *Knt,
                                              const double *knt, const double *Snt, const double *Kpt, const double *kpt,
                                              const double *Spt, const double *Si, int &threw)
{
    const int n = NC ? NC : n_, m = MC ? MC : m_;                        // compile-time sizes unroll every loop below
    const int p = n + m;
    double kd[MMAXK], mu[NMAXK], SKmu[MMAXK], Kmu[MMAXK];
    for (int a = 0; a < m; ++a) kd[a] = kpt[a] - knt[a];
    for (int j = 0; j < n; ++j) mu[j] = xn[j] - xo[j];
    double tr1 = 0.0, q1 = 0.0;
    for (int a = 0; a < m; ++a)
        for (int c = 0; c < m; ++c) {
            tr1 += Si[a + m * c] * Snt[c + m * a];                       // tr(Σip Σn)
            q1 += kd[a] * Si[a + m * c] * kd[c];                         // k_diff'Σip k_diff
        }
    int sp, sn;
    const double ldp = logabsdet_small(m, Spt, sp), ldn = logabsdet_small(m, Snt, sn);
    if (sp < 0 || sn < 0) threw = 1;                                     // logdet throws a DomainError (:95-99)
    double v = 0.5 * (tr1 + q1 - m + ldp - ldn);                         // :92
    for (int a = 0; a < m; ++a) {
        double s = 0.0;
        for (int j = 0; j < n; ++j) s += (Kpt[a + m * j] - Knt[a + m * j]) * mu[j];
        Kmu[a] = s;
    }
    double q2 = 0.0, q3 = 0.0, tr2 = 0.0;
    for (int a = 0; a < m; ++a) {                                        // Σip K_diff μ
        double s = 0.0;
        for (int c = 0; c < m; ++c) s += Si[a + m * c] * Kmu[c];
        SKmu[a] = s;
        q2 += Kmu[a] * s;
        q3 += kd[a] * s;
    }
    for (int c = 0; c < n; ++c) {                                        // tr(K_diff'Σip K_diff Σt), Σt = sigmanew[1:n,1:n,t]
        double SK[MMAXK];
        for (int a = 0; a < m; ++a) {
            double s = 0.0;
            for (int a2 = 0; a2 < m; ++a2) s += Si[a + m * a2] * (Kpt[a2 + m * c] - Knt[a2 + m * c]);
            SK[a] = s;
        }
        for (int r = 0; r < n; ++r) {
            double s = 0.0;
            for (int a = 0; a < m; ++a) s += (Kpt[a + m * r] - Knt[a + m * r]) * SK[a];
            tr2 += s * St[c + p * r];
        }
    }
    v += 0.5 * (q2 + tr2) + q3;                                          // :93-94
    return v <= 0.0 ? 0.0 : v;                                           // :101 max(0, v): a NaN stays a NaN, -0.0 becomes 0.0
}

__global__ __launch_bounds__(DDP_WAVE) void kl_div_kernel(int n, int m, int N, const double *__restrict__ xnew,
                                                          const double *__restrict__ xold, const double *__restrict__ sig,
                                                          const double *__restrict__ Kn, const double *__restrict__ kn,
                                                          const double *__restrict__ Sn, const double *__restrict__ Kp,
                                                          const double *__restrict__ kp, const double *__restrict__ Sp,
                                                          const double *__restrict__ Sip, double *__restrict__ kldiv,
                                                          double *__restrict__ klmean)
{
    const int b = blockIdx.x, lane = threadIdx.x, p = n + m;
    const size_t nm = (size_t)n * m, mm = (size_t)m * m, pp = (size_t)p * p;
    double acc = 0.0;
    int threw = 0;
    for (int t = lane; t < N; t += DDP_WAVE) {
        const size_t tb = (size_t)N * b + t;
        const double v = kl_div_step(n, m, xnew + (size_t)n * tb, xold + (size_t)n * tb, sig + pp * tb, Kn + nm * tb, kn + (size_t)m * tb,
                                     Sn + mm * tb, Kp + nm * tb, kp + (size_t)m * tb, Sp + mm * tb, Sip + mm * tb, threw);
        kldiv[tb] = v;
        acc += v;
    }
    for (int off = 32; off >= 1; off >>= 1) { acc += __shfl_xor(acc, off, 64); threw |= __shfl_xor(threw, off, 64); }
    if (lane == 0) klmean[b] = threw ? INFINITY : acc / N;
}

// The same with the operands of 64 time steps brought in by COALESCED loads into an LDS image first (small n, m: the C5 shape keeps 46
// doubles per step).  With lanes over time every lane's own slice is contiguous but the lanes' slices are 8 .. 200 bytes apart: the
// 25 loads of a step's sigmanew each touch 64 different lines, and the kernel above moved 7.0 GB for 0.93 GB of operands
// (profiles/r03_c5_pmc.txt).  Per-step strides in the image are odd numbers of doubles (no bank conflicts).
struct KlSrc { const double *g; int len; };
template <int I, int E, class F>
__device__ __forceinline__ void kl_static_for(F &&f)
{
    if constexpr (I < E) { f(std::integral_constant<int, I>{}); kl_static_for<I + 1, E>(f); }
}
template <int NC, int MC>
__global__ __launch_bounds__(DDP_WAVE) void kl_div_lds_kernel(int n, int m, int N, KlSrc s0, KlSrc s1, KlSrc s2, KlSrc s3, KlSrc s4, KlSrc s5,
                                                              KlSrc s6, KlSrc s7, KlSrc s8, KlSrc s9, double *__restrict__ kldiv,
                                                              double *__restrict__ klmean)
{
    extern __shared__ double klds[];
    const int b = blockIdx.x, lane = threadIdx.x;
    const KlSrc src[10] = {s0, s1, s2, s3, s4, s5, s6, s7, s8, s9};
    int off[10], stride[10], q0[10], r0[10];
    {
        int o = 0;
#pragma unroll
        for (int a = 0; a < 10; ++a) {
            stride[a] = src[a].len | 1;
            off[a] = o;
            o += stride[a] * DDP_WAVE;
            q0[a] = lane / src[a].len; r0[a] = lane % src[a].len;        // (step, entry) of this lane's first element of a chunk
        }
    }
    double acc = 0.0;
    int threw = 0;
    for (int t0 = 0; t0 < N; t0 += DDP_WAVE) {
        const int cnt = N - t0 < DDP_WAVE ? N - t0 : DDP_WAVE;
        if constexpr (NC != 0) {
            // compile-time sizes: ALL loads of the chunk are issued before the first LDS write (46 per lane at n = 4, m = 1) — one memory
            // latency per chunk.  The run-time-sized loop below waits for every load before its LDS write: 46 latencies per chunk, 0.62 ms
            // of the 0.62 ms this kernel took on the C5 shape.
            constexpr int P_ = NC + MC;
            constexpr int LEN[10] = {NC, NC, P_ * P_, NC * MC, MC, MC * MC, NC * MC, MC, MC * MC, MC * MC};
            constexpr int TOT = LEN[0] + LEN[1] + LEN[2] + LEN[3] + LEN[4] + LEN[5] + LEN[6] + LEN[7] + LEN[8] + LEN[9];
            double v[TOT];
            int vi = 0;
            kl_static_for<0, 10>([&](auto ac) {
                constexpr int a = decltype(ac)::value, len = LEN[a];
                const double *gp = src[a].g + (size_t)len * ((size_t)N * b + t0);
                const int total = cnt * len;
#pragma unroll
                for (int k = 0; k < len; ++k) {
                    const int g = k * DDP_WAVE + lane;
                    v[vi + k] = gp[g < total ? g : total - 1];
                }
                vi += len;
            });
            vi = 0;
            kl_static_for<0, 10>([&](auto ac) {
                constexpr int a = decltype(ac)::value, len = LEN[a];
                const int total = cnt * len;
#pragma unroll
                for (int k = 0; k < len; ++k) {
                    const int g = k * DDP_WAVE + lane;
                    if (g < total) klds[off[a] + (g / len) * (len | 1) + g % len] = v[vi + k];
                }
                vi += len;
            });
        } else {
#pragma unroll
        for (int a = 0; a < 10; ++a) {
            const int len = src[a].len, total = cnt * len, dq = DDP_WAVE / len, dr = DDP_WAVE % len;
            const double *gp = src[a].g + (size_t)len * ((size_t)N * b + t0);
            int t = q0[a], e = r0[a];
            for (int g = lane; g < total; g += DDP_WAVE) {
                klds[off[a] + t * stride[a] + e] = gp[g];
                t += dq; e += dr;
                if (e >= len) { e -= len; ++t; }
            }
        }
        }
        wave_sync();
        if (lane < cnt) {
            const double *L[10];
#pragma unroll
            for (int a = 0; a < 10; ++a) L[a] = klds + off[a] + lane * stride[a];
            const double v = kl_div_step<NC, MC>(n, m, L[0], L[1], L[2], L[3], L[4], L[5], L[6], L[7], L[8], L[9], threw);
            kldiv[(size_t)N * b + t0 + lane] = v;
            acc += v;
        }
        wave_sync();
    }
    for (int o2 = 32; o2 >= 1; o2 >>= 1) { acc += __shfl_xor(acc, o2, 64); threw |= __shfl_xor(threw, o2, 64); }
    if (lane == 0) klmean[b] = threw ? INFINITY : acc / N;
}

// ---- the dual variable of the KL constraint, one thread per trajectory (calc_η klutils.jl:112-133, the bracket/exit logic of
// iLQGkl.jl:91-178).  op 0: start of an iteration, 1: after a back pass, 2: after the divergence of the new trajectory is known.
// steps (ddp_kl_set_steps, else NULL): one kl_step per trajectory in place of the scalar.
__global__ void kl_dual_kernel(int op, int B, int it, double kl_step_all, ddp_kl_dual s, const int32_t *__restrict__ diverge,
                               const double *__restrict__ klmean, int32_t *__restrict__ count, const double *__restrict__ steps)
{
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    int one = 0;
    if (b < B) {
        double *e = s.etab + 3 * (long)b;
        if (op == 0) {                                                        // iLQGkl.jl:91-95
            const int lv = s.live[b];
            s.pend[b] = lv;
            if (lv) { s.iters[b] = it; s.eta[b] = e[1]; }
            one = lv;
        } else if (op == 1) {                                                 // :100-122
            if (s.pend[b]) {
                s.nback[b] += 1;
                if (diverge[b] > 0) {                                         // :103-105  η += del; del *= 2; back pass again
                    e[1] += s.del[b];
                    s.del[b] *= 2.0;
                    s.eta[b] = e[1];
                    one = 1;
                } else s.pend[b] = 0;
            }
        } else if (s.live[b]) {                                               // :141 calc_η, :169-177
            bool sat = true;
            double dv = 0.0;
            const double kl_step = steps ? steps[b] : kl_step_all;
            if (kl_step > 0) {                                                // klutils.jl:113
                dv = klmean[b];
                const double viol = dv - kl_step;                             // :116
                sat = fabs(viol) < 0.1 * kl_step;                             // :118
                if (!sat) {
                    if (viol < 0) {                                           // :121-124  η was too big
                        e[2] = e[1];
                        const double g = sqrt(e[0] * e[2]), o = 0.1 * e[2];
                        e[1] = (o > g) ? o : g;
                    } else {                                                  // :126-129  η was too small (also a NaN divergence)
                        e[0] = e[1];
                        const double g = sqrt(e[0] * e[2]), o = 10.0 * e[0];
                        e[1] = (o < g) ? o : g;
                    }
                }
            }
            s.divergence[b] = dv;
            s.satisfied[b] = sat;
            if (sat) { s.status[b] = 1; s.live[b] = 0; }                      // iLQGkl.jl:169
            else if (e[1] > 0.999 * e[2]) { s.status[b] = 2; s.live[b] = 0; } // :174  (the back pass of this η never happens)
            one = s.live[b];
        }
    }
    const unsigned long long bal = __ballot(one);
    if ((threadIdx.x & 63) == 0 && bal) atomicAdd(count, (int)__popcll(bal));
}


// ---- helpers of the iLQGkl driver (ddp_ilqgkl_f64_dev below)
// dst[e, t, b] = src[e (, b)]: gives a time-invariant operand the time axis back_pass_gps wants (demo_linear.jl:91-101 hands out 3-D arrays)
__global__ __launch_bounds__(256) void kl_repeat_kernel(int len, int N, long total, int src_batched, const double *__restrict__ src,
                                                        double *__restrict__ dst)
{
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e >= total) return;
    const long per = (long)len * N;
    dst[e] = src ? src[(e % len) + (src_batched ? (e / per) * len : 0)] : 0.0;
}
// x0c[:, b] = x0[:, 1, b]  (the start of every rollout, iLQGkl.jl:132)
__global__ __launch_bounds__(256) void kl_first_col_kernel(int n, int N, int B, const double *__restrict__ x0, double *__restrict__ x0c)
{
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e < n * B) x0c[e] = x0[(size_t)n * N * (e / n) + (e % n)];
}
__global__ __launch_bounds__(256) void kl_dual_init_kernel(int B, double e0, double e1, double e2, double del0, int own_etab, ddp_kl_dual s)
{
    const int b = blockIdx.x * 256 + threadIdx.x;
    if (b >= B) return;
    if (own_etab) { s.etab[3 * (long)b] = e0; s.etab[3 * (long)b + 1] = e1; s.etab[3 * (long)b + 2] = e2; }
    s.eta[b] = s.etab[3 * (long)b + 1];
    s.del[b] = del0; s.divergence[b] = 0.0;
    s.satisfied[b] = 0; s.status[b] = 0; s.live[b] = 1; s.pend[b] = 0; s.iters[b] = 0; s.nback[b] = 0;
}
// one wave per trajectory: g_norm = mean_t max_a |k[a,t]| / (|u[a,t]| + 1)  (iLQGkl.jl:125) and the summary row of the trajectory
__global__ __launch_bounds__(DDP_WAVE) void kl_summary_kernel(int m, int N, ddp_kl_dual s, const double *__restrict__ k,
                                                              const double *__restrict__ u, const double *__restrict__ csum_new,
                                                              const double *__restrict__ cost0, const double *__restrict__ dV,
                                                              double *__restrict__ stats)
{
    const int b = blockIdx.x, lane = threadIdx.x;
    double acc = 0.0;
    for (int t = lane; t < N; t += DDP_WAVE) {
        double mx = 0.0;
        for (int a = 0; a < m; ++a) {
            const size_t e = (size_t)m * ((size_t)N * b + t) + a;
            const double r = fabs(k[e]) / (fabs(u[e]) + 1.0);
            mx = r > mx ? r : mx;
        }
        acc += mx;
    }
    for (int off = 32; off >= 1; off >>= 1) acc += __shfl_xor(acc, off, 64);
    if (lane == 0) {
        double *r = stats + (size_t)DDP_ILQGKL_NSTATS * b;
        const int st = s.status[b];
        r[0] = st ? st : 3;                                                   // still live when the loop ran out: max_iter (iLQGkl.jl:234)
        r[1] = s.iters[b]; r[2] = s.nback[b]; r[3] = s.satisfied[b];
        r[4] = s.etab[3 * (long)b]; r[5] = s.etab[3 * (long)b + 1]; r[6] = s.etab[3 * (long)b + 2];
        r[7] = s.divergence[b];
        r[8] = csum_new[b];
        r[9] = cost0 ? cost0[b] - csum_new[b] : NAN;                          // Δcost (:135)
        r[10] = -(dV[2 * (long)b] + dV[2 * (long)b + 1]);                     // expected_reduction (:136)
        r[11] = acc / N;
    }
}

size_t fcov_lds(int n, int m) { return ((size_t)3 * n * n + 2 * (size_t)n * m) * sizeof(double); }

// ---- kernel choice of the four KL entry points, host facts only.  Each entry point fills a KlChoiceIn, asks its *_choose function and
// launches what that returns; the unlisted hooks ddp_gps_choice .. ddp_kl_div_choice are wrappers over the same functions.
// back_pass_gps.  q4: n = 4, m = 1, one η per trajectory (back_pass_q4.hip); lane: n = 4, m <= 2 (back_pass_gps_lane.hip); mid: any
// n <= 32, m <= 8 on the matrix cores behind a combine prepass (back_pass_mid.hip); generic: the 64-lane run-time-sized kernel
// (back_pass.hip), also every call whose `kl` argument is incomplete (the generic launcher words that refusal).  The user-problem KL
// driver takes q4, lane, mid, generic; the stand-alone call and the registered families' driver q4, lane, generic.  DDP_GPS_MID=1 puts
// mid first in every call, =0 keeps it out of all of them (A/B timing, tests).  wide: the GPS instantiation of back_pass_wide.hip, see
// kl_shape.
enum GpsKernel { GPS_Q4, GPS_LANE, GPS_MID, GPS_GENERIC, GPS_WIDE, GPS_NONE };
const char *const gps_kernel_name[] = {"back_pass_gps_q4", "back_pass_gps_lane", "back_pass_gps_mid", "back_pass_gps", "back_pass_gps_wide", "none"};
enum GpsCaller { GPS_STANDALONE = 0, GPS_REGISTERED = 1, GPS_USER = 2 };

// What a choice depends on besides the sizes.  caller, eta_tv, complete: back_pass_gps (complete: every pointer of `kl` is there, and
// lims and u with has_lims); al16: forward_covariance, its fx, K, Sigma and sigmanew are 16-byte aligned; sink: the handle has its sink
// buffer; wide_on: ddp_kl_set_wide; the switches as strings (NULL: unset)
struct KlChoiceIn {
    int caller = GPS_STANDALONE, eta_tv = 0;
    bool complete = true, al16 = false, sink = false;
    int wide_on = 0;
    const char *gps_mid = nullptr, *gps_q4 = nullptr, *gps_lane = nullptr, *gps_wide = nullptr, *fcov_q4 = nullptr, *fcov_q4l = nullptr,
               *kl_lds = nullptr;
};
KlChoiceIn kl_choice_in(ddp_handle h, const BPCall *c = nullptr)
{
    KlChoiceIn q;
    q.sink = h->sink != nullptr; q.wide_on = h->kl_wide;
    q.gps_mid = ddp_env(h, ENV_GPS_MID); q.gps_q4 = ddp_env(h, ENV_GPS_Q4); q.gps_lane = ddp_env(h, ENV_GPS_LANE);
    q.gps_wide = ddp_env(h, ENV_GPS_WIDE); q.fcov_q4 = ddp_env(h, ENV_FCOV_Q4); q.fcov_q4l = ddp_env(h, ENV_FCOV_Q4L);
    q.kl_lds = ddp_env(h, ENV_KL_LDS);
    if (c) {
        const ddp_kl_cost_terms *kl = c->kl;
        q.eta_tv = kl ? kl->eta_tv : 0;
        q.complete = kl && kl->cx && kl->cu && kl->cxx && kl->cxu && kl->cuu && kl->eta && (!c->d.has_lims || (c->lims && c->u));
    }
    return q;
}

// The KL shape box: 0 the kernels of n <= 32, m <= 8; 1 the wide kernels of n <= 64, m <= DDP_MAX_M_WIDE (the switch is on and the shape
// is beyond the box, or DDP_GPS_WIDE=1 inside it); -1 no kernel.
int kl_shape(int n, int m, const KlChoiceIn &q)
{
    const bool small = n >= 1 && n <= NMAXK && m >= 1 && m <= MMAXK, wide_ok = n >= 1 && n <= KL_WIDE_MAX_N && m >= 1 && m <= DDP_MAX_M_WIDE;
    if (small) return (q.gps_wide && q.gps_wide[0] == '1') ? 1 : 0;
    return (q.wide_on && wide_ok) ? 1 : -1;
}
// The one shape check: every KL entry point and the iLQGkl driver call it before anything else depends on the sizes
// (`kernel`: what the entry has no kernel for — "back_pass_gps" for that entry and the loop around it, as the wrappers word it, "KL" else)
int kl_check_shape(ddp_handle h, const char *who, const char *kernel, int n, int m, int N, int B)
{
    DDP_CHECK(kl_shape(n, m, kl_choice_in(h)) >= 0, "%s: n=%d m=%d has no %s kernel (n <= %d, m <= %d; after ddp_kl_set_wide(h, 1): "
              "n <= %d, m <= %d)", who, n, m, kernel, NMAXK, MMAXK, KL_WIDE_MAX_N, DDP_MAX_M_WIDE);
    DDP_CHECK(N >= 1 && B >= 1, "%s: bad sizes N=%d B=%d (both >= 1)", who, N, B);
    return 0;
}

GpsKernel gps_choose(const ddp_bp_desc &d, const KlChoiceIn &q)
{
    const int sh = kl_shape(d.n, d.m, q);
    if (sh < 0) return GPS_NONE;
    if (!q.complete) return GPS_GENERIC;
    if (sh) return GPS_WIDE;
    const char mid = q.gps_mid ? q.gps_mid[0] : 0;
    if (mid == '1') return GPS_MID;
    const bool fast = q.caller != GPS_STANDALONE || !(q.gps_lane && q.gps_lane[0] == '0');    // stand-alone DDP_GPS_LANE=0: the generic kernel
    const bool tv = d.N >= 2 && d.fx_tv && d.cost_tv;
    if (fast && tv && d.n == 4 && d.m == 1 && !q.eta_tv && !(q.gps_q4 && q.gps_q4[0] == '0')) return GPS_Q4;
    if (fast && tv && d.n == 4 && (d.m == 1 || d.m == 2)) return GPS_LANE;
    if (q.caller == GPS_USER && mid != '0') return GPS_MID;
    return GPS_GENERIC;
}

// ∇kl: the small kernel or the wide one
enum KlTermsKernel { KLTERMS_SMALL, KLTERMS_WIDE, KLTERMS_NONE };
KlTermsKernel kl_terms_choose(int n, int m, const KlChoiceIn &q)
{
    const int sh = kl_shape(n, m, q);
    return sh < 0 ? KLTERMS_NONE : sh ? KLTERMS_WIDE : KLTERMS_SMALL;
}

// forward_covariance (the names are what ddp_last_kernel(h, 5) reports).  q4<M>: n = 4, m = M <= 2 on the matrix cores, four
// trajectories per wave (needs the handle's sink buffer; DDP_FCOV_Q4=0: not); q4l: its m = 1 variant with chunks of eight steps through
// the LDS — N a multiple of 8 and >= 16, fx, K, Sigma and sigmanew 16-byte aligned, B <= 6144 (DDP_FCOV_Q4L=0: not); generic: the
// run-time-sized kernel, every n <= 32, m <= 8; wide: kl_shape.
enum FcovKernel { FCOV_GENERIC, FCOV_Q4_1, FCOV_Q4_2, FCOV_Q4L, FCOV_WIDE, FCOV_NONE };
const char *const fcov_kernel_name[] = {"fcov_kernel", "fcov_q4_kernel<1>", "fcov_q4_kernel<2>", "fcov_q4l_kernel", "fcov_wide_kernel", "none"};

FcovKernel fcov_choose(int n, int m, int N, int B, const KlChoiceIn &q)
{
    const int sh = kl_shape(n, m, q);
    if (sh < 0 || N < 1 || B < 1) return FCOV_NONE;
    if (sh) return FCOV_WIDE;
    if (n == 4 && (m == 1 || m == 2) && q.sink && !(q.fcov_q4 && q.fcov_q4[0] == '0')) {
        if (m == 1 && N % FQL_CH == 0 && N >= 2 * FQL_CH && q.al16 && B <= 6144 && !(q.fcov_q4l && q.fcov_q4l[0] == '0')) return FCOV_Q4L;
        return m == 1 ? FCOV_Q4_1 : FCOV_Q4_2;
    }
    return FCOV_GENERIC;
}

// kl_div_wiki (ddp_last_kernel(h, 6)).  lds: the operands of 64 steps through an LDS image when that fits 48 KB (DDP_KL_LDS=0: not) —
// <4,1> and <4,2> with compile-time sizes, <0,0> the run-time-sized staging loop; direct: every n <= 32, m <= 8 from global memory;
// wide: kl_shape.
enum KlDivKernel { KLDIV_DIRECT, KLDIV_LDS41, KLDIV_LDS42, KLDIV_LDS00, KLDIV_WIDE, KLDIV_NONE };
const char *const kl_div_kernel_name[] = {"kl_div_kernel", "kl_div_lds_kernel<4,1>", "kl_div_lds_kernel<4,2>", "kl_div_lds_kernel<0,0>",
                                          "kl_div_wide_kernel", "none"};

// bytes of the LDS image of 64 steps: the ten operands of a step, each at an odd stride
size_t kl_div_image(int n, int m)
{
    const int lens[10] = {n, n, (n + m) * (n + m), n * m, m, m * m, n * m, m, m * m, m * m};
    size_t image = 0;
    for (int l : lens) image += (size_t)(l | 1) * DDP_WAVE * sizeof(double);
    return image;
}

KlDivKernel kl_div_choose(int n, int m, int N, int B, const KlChoiceIn &q)
{
    const int sh = kl_shape(n, m, q);
    if (sh < 0 || N < 1 || B < 1) return KLDIV_NONE;
    if (sh) return KLDIV_WIDE;
    if (kl_div_image(n, m) <= 48 * 1024 && !(q.kl_lds && q.kl_lds[0] == '0'))
        return (n == 4 && m == 1) ? KLDIV_LDS41 : (n == 4 && m == 2) ? KLDIV_LDS42 : KLDIV_LDS00;
    return KLDIV_DIRECT;
}

// Launches the kernel gps_choose returned for the call.  A launcher returns 1 to decline, and the next of q4 -> lane -> generic takes the
// call.  What they test is what gps_choose has tested already — q4: n = 4, m = 1, N >= 2, time-varying fx and cost, one η per
// trajectory, DDP_GPS_Q4; lane: n = 4, m <= 2, N >= 2, time-varying fx and cost; mid: the box, a `kl` and a Quui — so behind gps_choose
// only mid can decline, on a BPCall without Quui (no entry point builds one).  ddp_last_kernel(h, 0) names the kernel that ran.
int gps_launch(ddp_handle h, const BPCall &c, GpsKernel k)
{
    int rc = 1;
    if (k == GPS_WIDE) {
        rc = ddp_launch_back_pass_gps_wide(h, c);           // 0 or < 0: it never declines (nothing else takes a wide shape)
    } else if (k == GPS_MID) {
        rc = ddp_launch_back_pass_gps_mid(h, c);
    } else if (k == GPS_Q4) {
        rc = ddp_launch_back_pass_gps_q4(h, c);
        if (rc > 0) k = GPS_LANE;
    }
    if (k == GPS_LANE) rc = ddp_launch_back_pass_gps_lane(h, c);
    if (rc > 0) { k = GPS_GENERIC; rc = ddp_launch_back_pass_gps(h, c); }
    if (!rc || k != GPS_WIDE) h->last_kernel[0] = gps_kernel_name[k];      // (a wide launch that failed ran nothing; the others as ever)
    return rc;
}

}   // namespace

extern "C" {

int ddp_kl_terms_f64_dev(ddp_handle h, int n, int m, int N, int B, const double *K, const double *k, const double *Sigmai,
                         double *cx, double *cu, double *cxx, double *cxu, double *cuu)
{
    DDP_DEVICE(h);
    DDP_CHECK(K && k && Sigmai && cx && cu && cxx && cxu && cuu, "kl_terms: null argument");
    if (int rc = kl_check_shape(h, "kl_terms", "KL", n, m, N, B)) return rc;
    if (kl_terms_choose(n, m, kl_choice_in(h)) == KLTERMS_WIDE) return ddp_launch_kl_terms_wide(h, n, m, N, B, K, k, Sigmai, cx, cu, cxx, cxu, cuu);
    const long NB = (long)N * B;
    hipLaunchKernelGGL(kl_terms_kernel, dim3((unsigned)((NB + 255) / 256)), dim3(256), 0, h->stream, n, m, NB, K, k, Sigmai, cx, cu, cxx, cxu, cuu);
    DDP_HIP(hipGetLastError());
    return 0;
}

int ddp_back_pass_gps_f64_dev(ddp_handle h, const ddp_bp_desc *d,
                              const double *cx, const double *cu, const double *cxx, const double *cxu, const double *cuu,
                              const double *fx, const double *fu, const ddp_kl_cost_terms *kl,
                              const double *lims, const double *u, const int32_t *active,
                              double *K, double *k, double *Quu, double *Quui, double *Vx, double *Vxx, double *dV,
                              int32_t *diverge)
{
    DDP_DEVICE(h);
    DDP_CHECK(d && cx && cu && cxx && cxu && cuu && fx && fu && kl && K && k && Quu && Quui && Vx && Vxx && dV && diverge,
              "back_pass_gps: null argument");
    if (int rc = kl_check_shape(h, "back_pass_gps", "back_pass_gps", d->n, d->m, d->N, d->B)) return rc;
    DDP_HIP(hipMemsetAsync(Quui, 0, sizeof(double) * (size_t)d->m * d->m * d->N * d->B, h->stream));
    const BPCall c = {*d, cx, cu, cxx, cxu, cuu, fx, fu, nullptr, lims, u, active, K, k, Quu, Vx, Vxx, dV, diverge, kl, Quui};
    return gps_launch(h, c, gps_choose(c.d, kl_choice_in(h, &c)));
}

// Unlisted debug hooks (not in ddp_amd.h): the kernel names ddp_last_kernel(h, 0) / (h, 5) / (h, 6) report after a back_pass_gps /
// forward_covariance / kl_div_wiki with these facts (the fields of KlChoiceIn; the switches as strings, NULL: unset) — gps_choose,
// fcov_choose and kl_div_choose, the functions the entry points call, callable without a GPU.  "none": the call is refused.
// ddp_gps_choice3 takes every fact of back_pass_gps; ddp_gps_choice2 is a complete call, ddp_gps_choice one with the wide switch off too.
const char *ddp_gps_choice3(const ddp_bp_desc *d, int eta_tv, int caller, int complete, const char *gps_mid, const char *gps_q4,
                            const char *gps_lane, int wide_on, const char *gps_wide)
{
    KlChoiceIn q;
    q.caller = caller; q.eta_tv = eta_tv; q.complete = complete != 0; q.wide_on = wide_on;
    q.gps_mid = gps_mid; q.gps_q4 = gps_q4; q.gps_lane = gps_lane; q.gps_wide = gps_wide;
    return gps_kernel_name[gps_choose(*d, q)];
}
const char *ddp_gps_choice2(const ddp_bp_desc *d, int eta_tv, int caller, const char *gps_mid, const char *gps_q4, const char *gps_lane,
                            int wide_on, const char *gps_wide)
{
    return ddp_gps_choice3(d, eta_tv, caller, 1, gps_mid, gps_q4, gps_lane, wide_on, gps_wide);
}
const char *ddp_gps_choice(const ddp_bp_desc *d, int eta_tv, int caller, const char *gps_mid, const char *gps_q4, const char *gps_lane)
{
    return ddp_gps_choice3(d, eta_tv, caller, 1, gps_mid, gps_q4, gps_lane, 0, nullptr);
}
const char *ddp_fcov_choice(int n, int m, int N, int B, int al16, int sink, int wide_on, const char *gps_wide, const char *fcov_q4,
                            const char *fcov_q4l)
{
    KlChoiceIn q;
    q.al16 = al16 != 0; q.sink = sink != 0; q.wide_on = wide_on; q.gps_wide = gps_wide; q.fcov_q4 = fcov_q4; q.fcov_q4l = fcov_q4l;
    return fcov_kernel_name[fcov_choose(n, m, N, B, q)];
}
const char *ddp_kl_div_choice(int n, int m, int N, int B, int wide_on, const char *gps_wide, const char *kl_lds)
{
    KlChoiceIn q;
    q.wide_on = wide_on; q.gps_wide = gps_wide; q.kl_lds = kl_lds;
    return kl_div_kernel_name[kl_div_choose(n, m, N, B, q)];
}

int ddp_kl_set_wide(ddp_handle h, int on)
{
    if (!h) { ddp_set_error("null handle"); return -1; }
    const int was = h->kl_wide;
    h->kl_wide = on ? 1 : 0;
    return was;
}

int ddp_forward_covariance_f64_dev(ddp_handle h, int n, int m, int N, int B, const double *fx, int fx_batched,
                                   const double *R1, const double *K, const double *Sigma, double *sigmanew)
{
    DDP_DEVICE(h);
    DDP_CHECK(fx && R1 && K && Sigma && sigmanew, "forward_covariance: null argument");
    int rc = kl_check_shape(h, "forward_covariance", "KL", n, m, N, B);
    if (rc) return rc;
    KlChoiceIn q = kl_choice_in(h);
    q.al16 = ((((uintptr_t)fx | (uintptr_t)K | (uintptr_t)Sigma | (uintptr_t)sigmanew) & 15) == 0);
    // DDP_FCOV_Q4=0: the run-time-sized kernel for every shape; DDP_FCOV_Q4L=0: the step-by-step q4 kernel (cross-checks in the tests)
    const FcovKernel kern = fcov_choose(n, m, N, B, q);
    const dim3 grid4((unsigned)((B + 3) / 4)), block(DDP_WAVE);
    if (kern == FCOV_WIDE)
        rc = ddp_launch_fcov_wide(h, n, m, N, B, fx, fx_batched, R1, K, Sigma, sigmanew);
    else if (kern == FCOV_Q4L)
        hipLaunchKernelGGL(fcov_q4l_kernel, grid4, block, 0, h->stream, N, B, fx, fx_batched, R1, K, Sigma, sigmanew, (double *)h->sink);
    else if (kern == FCOV_Q4_1)
        hipLaunchKernelGGL(fcov_q4_kernel<1>, grid4, block, 0, h->stream, N, B, fx, fx_batched, R1, K, Sigma, sigmanew, (double *)h->sink);
    else if (kern == FCOV_Q4_2)
        hipLaunchKernelGGL(fcov_q4_kernel<2>, grid4, block, 0, h->stream, N, B, fx, fx_batched, R1, K, Sigma, sigmanew, (double *)h->sink);
    else
        hipLaunchKernelGGL(fcov_kernel, dim3(B), block, fcov_lds(n, m), h->stream, n, m, N, fx, fx_batched, R1, K, Sigma, sigmanew);
    if (rc) return rc;
    DDP_HIP(hipGetLastError());
    h->last_kernel[5] = fcov_kernel_name[kern];
    return 0;
}

int ddp_kl_div_f64_dev(ddp_handle h, int n, int m, int N, int B, const double *xnew, const double *xold,
                       const double *sigmanew, const double *Kn, const double *kn, const double *Sn,
                       const double *Kp, const double *kp, const double *Sp, const double *Sip,
                       double *kldiv, double *klmean)
{
    DDP_DEVICE(h);
    DDP_CHECK(xnew && xold && sigmanew && Kn && kn && Sn && Kp && kp && Sp && Sip && kldiv && klmean, "kl_div: null argument");
    int rc = kl_check_shape(h, "kl_div", "KL", n, m, N, B);
    if (rc) return rc;
    const KlDivKernel kern = kl_div_choose(n, m, N, B, kl_choice_in(h));
    // operands through an LDS image of 64 steps when that fits (DDP_KL_LDS=0: the direct kernel, cross-check in the tests)
    if (kern == KLDIV_WIDE) {
        rc = ddp_launch_kl_div_wide(h, n, m, N, B, xnew, xold, sigmanew, Kn, kn, Sn, Kp, kp, Sp, Sip, kldiv, klmean);
    } else if (kern != KLDIV_DIRECT) {
        const int lens[10] = {n, n, (n + m) * (n + m), n * m, m, m * m, n * m, m, m * m, m * m};
        const size_t image = kl_div_image(n, m);
        const double *ptr[10] = {xnew, xold, sigmanew, Kn, kn, Sn, Kp, kp, Sp, Sip};
        KlSrc a[10];
        for (int i = 0; i < 10; ++i) a[i] = KlSrc{ptr[i], lens[i]};
#define DDP_KLL(NC_, MC_) hipLaunchKernelGGL((kl_div_lds_kernel<NC_, MC_>), dim3(B), dim3(DDP_WAVE), image, h->stream, n, m, N, a[0], a[1], a[2], \
                                             a[3], a[4], a[5], a[6], a[7], a[8], a[9], kldiv, klmean)
        if (kern == KLDIV_LDS41) DDP_KLL(4, 1);
        else if (kern == KLDIV_LDS42) DDP_KLL(4, 2);
        else DDP_KLL(0, 0);
#undef DDP_KLL
    } else {
        hipLaunchKernelGGL(kl_div_kernel, dim3(B), dim3(DDP_WAVE), 0, h->stream, n, m, N, xnew, xold, sigmanew, Kn, kn, Sn, Kp, kp, Sp, Sip,
                           kldiv, klmean);
    }
    if (rc) return rc;
    DDP_HIP(hipGetLastError());
    h->last_kernel[6] = kl_div_kernel_name[kern];
    return 0;
}

// one dual step on the stream: clears `count`, then kl_dual_kernel counts into it (the stand-alone entries and the driver)
static int kl_dual_enqueue(ddp_handle h, int op, int B, int it, double kl_step, const ddp_kl_dual &s, const int32_t *diverge,
                           const double *klmean, int32_t *count)
{
    DDP_HIP(hipMemsetAsync(count, 0, sizeof(int32_t), h->stream));
    hipLaunchKernelGGL(kl_dual_kernel, dim3((unsigned)((B + 255) / 256)), dim3(256), 0, h->stream, op, B, it, kl_step, s, diverge, klmean, count,
                       (const double *)h->kl_steps);
    DDP_HIP(hipGetLastError());
    return 0;
}
// reads a count of kl_dual_kernel back (the one synchronisation of a dual step)
static int kl_dual_poll(ddp_handle h, const int32_t *count, int *out)
{
    DDP_HIP(hipMemcpyAsync(h->h_pinned, count, sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
    DDP_HIP(hipStreamSynchronize(h->stream));
    *out = h->h_pinned[0];
    return 0;
}
static int kl_dual_launch(ddp_handle h, int op, int B, int it, double kl_step, const ddp_kl_dual *s, const int32_t *diverge,
                          const double *klmean, int *count)
{
    DDP_DEVICE(h);
    DDP_CHECK(s && count && B >= 1, "kl_dual: null argument");
    DDP_CHECK(s->etab && s->eta && s->del && s->divergence && s->satisfied && s->status && s->live && s->pend && s->iters && s->nback,
              "kl_dual: null state array");
    DDP_CHECK(!h->kl_steps || h->kl_steps_B == B, "kl_dual: B = %d, the table of ddp_kl_set_steps holds %d steps", B, h->kl_steps_B);
    void *cnt = nullptr;
    int rc = ddp_scratch(h, 256, &cnt);
    if (rc || (rc = kl_dual_enqueue(h, op, B, it, kl_step, *s, diverge, klmean, (int32_t *)cnt))) return rc;
    return kl_dual_poll(h, (const int32_t *)cnt, count);
}

int ddp_kl_dual_begin_f64_dev(ddp_handle h, int B, int it, const ddp_kl_dual *s, int *n_live)
{
    return kl_dual_launch(h, 0, B, it, 0.0, s, nullptr, nullptr, n_live);
}

int ddp_kl_dual_retry_f64_dev(ddp_handle h, int B, const ddp_kl_dual *s, const int32_t *diverge, int *n_pending)
{
    DDP_CHECK(diverge, "kl_dual_retry: null argument");
    return kl_dual_launch(h, 1, B, 0, 0.0, s, diverge, nullptr, n_pending);
}

int ddp_kl_dual_update_f64_dev(ddp_handle h, int B, double kl_step, const ddp_kl_dual *s, const double *klmean, int *n_live)
{
    DDP_CHECK(klmean, "kl_dual_update: null argument");
    return kl_dual_launch(h, 2, B, 0, kl_step, s, nullptr, klmean, n_live);
}

// ---- one kl_step per trajectory: the handle keeps its own device copy, kl_dual_kernel reads it in place of the scalar of the call
static int kl_steps_finite(int B, const double *steps)
{
    for (int b = 0; b < B; ++b)
        DDP_CHECK(fabs(steps[b]) <= DBL_MAX, "kl_set_steps: steps[%d] = %g is not finite", b, steps[b]);
    return 0;
}
static int kl_steps_store(ddp_handle h, int B, const double *steps, hipMemcpyKind kind)
{
    DDP_HIP(hipStreamSynchronize(h->stream));
    if (h->kl_steps) { DDP_HIP(hipFree(h->kl_steps)); h->kl_steps = nullptr; h->kl_steps_B = 0; }
    if (!steps) return 0;
    DDP_HIP(hipMalloc((void **)&h->kl_steps, (size_t)B * sizeof(double)));
    h->kl_steps_B = B;
    DDP_HIP(hipMemcpy(h->kl_steps, steps, (size_t)B * sizeof(double), kind));
    return 0;
}
int ddp_kl_set_steps_f64(ddp_handle h, int B, const double *steps)
{
    if (steps) {
        DDP_CHECK(B >= 1, "kl_set_steps: B = %d (>= 1)", B);
        const int rc = kl_steps_finite(B, steps);
        if (rc) return rc;
    }
    DDP_DEVICE(h);
    return kl_steps_store(h, B, steps, hipMemcpyHostToDevice);
}
int ddp_kl_set_steps_f64_dev(ddp_handle h, int B, const double *steps)
{
    DDP_CHECK(!steps || B >= 1, "kl_set_steps: B = %d (>= 1)", B);
    DDP_DEVICE(h);
    if (steps) {                                           // (a setter, not a hot path: the test needs the values on the host)
        std::vector<double> host((size_t)B);
        DDP_HIP(hipStreamSynchronize(h->stream));
        DDP_HIP(hipMemcpy(host.data(), steps, (size_t)B * sizeof(double), hipMemcpyDeviceToHost));
        const int rc = kl_steps_finite(B, host.data());
        if (rc) return rc;
    }
    return kl_steps_store(h, B, steps, hipMemcpyDeviceToDevice);
}

// ---- the step rule of the round, one thread per trajectory: J = sum_i ec[i, b] in ascending i of the three expected costs,
// mult = clip(pred / (2 max(1e-4, pred - act)), 0.1, 5) (a non-finite J: 0.1), kl_step_new = clip(kl_step mult, step_min, step_max)
__global__ __launch_bounds__(256) void kl_step_adjust_kernel(int N, int B, const double *__restrict__ ec_prev, const double *__restrict__ ec_pred,
                                                             const double *__restrict__ ec_act, const double *__restrict__ kl_step,
                                                             double step_min, double step_max, double *__restrict__ kl_step_new,
                                                             double *__restrict__ mult)
{
    const int b = blockIdx.x * 256 + threadIdx.x;
    if (b >= B) return;
    double Jp = 0.0, Jd = 0.0, Ja = 0.0;
    for (int i = 0; i < N; ++i) { const size_t e = (size_t)N * b + i; Jp += ec_prev[e]; Jd += ec_pred[e]; Ja += ec_act[e]; }
    double mu = 0.1;
    if (fabs(Jp) <= DBL_MAX && fabs(Jd) <= DBL_MAX && fabs(Ja) <= DBL_MAX) {
        const double pred = Jp - Jd, act = Jp - Ja;
        mu = pred / (2.0 * fmax(1e-4, pred - act));
        mu = mu < 0.1 ? 0.1 : (mu > 5.0 ? 5.0 : mu);
    }
    const double s = kl_step[b] * mu;
    mult[b] = mu;
    kl_step_new[b] = s < step_min ? step_min : (s > step_max ? step_max : s);
}
static int kl_step_adjust_validate(int N, int B, const void *ec_prev, const void *ec_pred, const void *ec_act, const void *kl_step,
                                   double step_min, double step_max, const void *kl_step_new, const void *mult)
{
    DDP_CHECK(N >= 1 && B >= 1, "kl_step_adjust: N = %d, B = %d (both >= 1)", N, B);
    DDP_CHECK(step_min > 0.0 && step_min <= step_max && step_max <= DBL_MAX, "kl_step_adjust: step_min = %g, step_max = %g should be finite with 0 < step_min <= step_max", step_min, step_max);
    DDP_CHECK(ec_prev && ec_pred && ec_act && kl_step && kl_step_new && mult, "kl_step_adjust: null argument");
    return 0;
}
int ddp_kl_step_adjust_f64_dev(ddp_handle h, int N, int B, const double *ec_prev, const double *ec_pred, const double *ec_act,
                               const double *kl_step, double step_min, double step_max, double *kl_step_new, double *mult)
{
    { const int rc = kl_step_adjust_validate(N, B, ec_prev, ec_pred, ec_act, kl_step, step_min, step_max, kl_step_new, mult); if (rc) return rc; }
    DDP_DEVICE(h);
    hipLaunchKernelGGL(kl_step_adjust_kernel, dim3((unsigned)((B + 255) / 256)), dim3(256), 0, h->stream, N, B, ec_prev, ec_pred, ec_act, kl_step,
                       step_min, step_max, kl_step_new, mult);
    DDP_HIP(hipGetLastError());
    return 0;
}
int ddp_kl_step_adjust_f64(ddp_handle h, int N, int B, const double *ec_prev, const double *ec_pred, const double *ec_act,
                           const double *kl_step, double step_min, double step_max, double *kl_step_new, double *mult)
{
    { const int rc = kl_step_adjust_validate(N, B, ec_prev, ec_pred, ec_act, kl_step, step_min, step_max, kl_step_new, mult); if (rc) return rc; }
    DDP_DEVICE(h);
    const size_t nb = (size_t)N * B;
    const double *d0, *d1, *d2, *ds;
    double *o0, *o1;
    Staging S(h, Staging::SCRATCH, "kl_step_adjust");
    S.in(&d0, ec_prev, nb); S.in(&d1, ec_pred, nb); S.in(&d2, ec_act, nb); S.in(&ds, kl_step, (size_t)B);
    S.out(&o0, kl_step_new, (size_t)B); S.out(&o1, mult, (size_t)B);
    const int rc = S.commit();
    if (rc) return rc;
    return S.finish(ddp_kl_step_adjust_f64_dev(h, N, B, d0, d1, d2, ds, step_min, step_max, o0, o1));
}


// ---- iLQGkl (single KL constraint, src/iLQGkl.jl:25-178,234-252) as ONE call on device-resident arrays.
// The batch advances in lock step; every pass recomputes ALL trajectories with their current η: one that has already left keeps its η
// (kl_dual_kernel), so it is recomputed to the same result and the arrays are right for everyone at the end.  Two stream
// synchronisations per iteration (the counts of still-diverging and of live trajectories), nothing else crosses PCIe.
void ddp_ilqgkl_default_opts(ddp_ilqgkl_opts *o)
{   // iLQGkl.jl:25-44
    o->kl_step = 1.0; o->max_iter = 50; o->etabracket[0] = 1e-8; o->etabracket[1] = 1.0; o->etabracket[2] = 1e16; o->del0 = 1e-4;
}

// The body of ddp_ilqgkl_f64_dev and ddp_user_ilqgkl*_f64_dev: the registered problem `p`, or the family `f` (a user problem) with its
// derivatives [.,.,N,B] (constant Hessians [.,.,B]), its costfun and its rollout — the three calls go through Model (ilqg_model.h); the
// operand layouts (kl_workspace.h) are back_pass_gps's own.  c.model_fx == NULL (family only): the model is the problem itself,
// forward_covariance takes the fx of STEP 1.
static int ilqgkl_impl(ddp_handle h, const ddp_problem *p, const ddp_family *f, const KlCall &c)
{
    const bool fit = c.fit_fx || c.fit_fu || c.fit_fc, cm = c.cm_cx || c.cm_cu || c.cm_cxx || c.cm_cxu || c.cm_cuu;
    DDP_CHECK(!fit || (f && c.fit_fx && c.fit_fu && c.fit_fc), "ilqgkl: a fitted model is fx, fu and fc, with a user problem");
    DDP_CHECK(!cm || (f && c.cm_cx && c.cm_cu && c.cm_cxx && c.cm_cxu && c.cm_cuu),
              "ilqgkl: a cost model is cx, cu, cxx, cxu and cuu, with a user problem");
    DDP_CHECK((p || f) && c.x0 && c.Kp && c.kp && c.Sp && c.Sip && (c.model_fx || f) && c.R1 && c.x && c.u && c.K && c.Sigma && c.Sigmai && c.Vx &&
              c.Vxx && c.cost && c.dV && c.stats, "ilqgkl: null argument");
    ddp_ilqgkl_opts od;
    const ddp_ilqgkl_opts *oo = c.opts;
    if (!oo) { ddp_ilqgkl_default_opts(&od); oo = &od; }
    DDP_CHECK(oo->max_iter >= 1, "ilqgkl: max_iter=%d (the reference returns undefined arrays without an iteration)", oo->max_iter);
    DDP_CHECK(c.x0 != c.x && c.kp != c.u, "ilqgkl: x0 / traj_prev.k must not alias the outputs x / u");
    const Model M(p, f);
    int rc = kl_check_shape(h, "ilqgkl", "back_pass_gps", M.n, M.m, M.N, M.B);
    if (rc) return rc;
    const size_t n = M.n, m = M.m, N = M.N, B = M.B, NB = N * B;
    DDP_CHECK(!h->kl_steps || (size_t)h->kl_steps_B == B, "ilqgkl: B = %zu, the table of ddp_kl_set_steps holds %d steps", B, h->kl_steps_B);
    const bool pend = M.pw.kind == DDP_PROBLEM_PENDCART;
    // dynamics as back_pass_gps wants them: [n,n,N] or [n,n,N,B]
    const bool fx_b = f || pend || p->dyn_batched, fx_rep = !f && !pend && !p->dyn_tv, fx_own = f || pend || fx_rep;
    // cost Hessians: [.,.,N] of the registered problem, [.,.,N,B] of a family; constant Hessians of a family [.,.,B], repeated along time
    // (hrep) for every kernel but mid and wide, which read every operand layout
    const bool cst = f && f->const_hessian && !cm;         // (a cost model is time-varying and per trajectory, whatever the problem's own is)
    ddp_kl_cost_terms t = {};
    BPCall gps = {};
    ddp_bp_desc &d = gps.d;
    d.n = M.n; d.m = M.m; d.N = M.N; d.B = M.B; d.fx_tv = 1; d.fx_batched = fx_b; d.cost_tv = 1; d.cost_batched = f != nullptr;
    d.regType = 1; d.has_lims = c.lims != nullptr;
    // the kernel of every back pass below, chosen once, for time-varying operands (the loop's call is complete: one η per trajectory,
    // lims with kp)
    KlChoiceIn q = kl_choice_in(h);
    q.caller = f ? GPS_USER : GPS_REGISTERED;
    const GpsKernel kern = gps_choose(d, q);
    const bool hrep = cst && kern != GPS_MID && kern != GPS_WIDE;
    if (cst && !hrep) d.cost_tv = 0;

    KlWork W;
    const KlWorkIn wi = {n, m, N, B, f != nullptr, fx_own, fx_b, cst, hrep};
    void *base;
    if ((rc = ddp_scratch(h, W.carve(Carver(), wi), &base))) return rc;
    W.carve(Carver(base), wi);
    const KlDeriv &dv = W.dv;
    ddp_kl_dual &s = W.dual.s;
    if (c.etab) s.etab = c.etab;
    t.cx = W.kt.cx; t.cu = W.kt.cu; t.cxx = W.kt.cxx; t.cxu = W.kt.cxu; t.cuu = W.kt.cuu; t.eta = s.eta; t.eta_tv = 0;

    hipStream_t st = h->stream;
    const unsigned gB = (unsigned)((B + 255) / 256);
    auto grid = [](size_t tot) { return dim3((unsigned)((tot + 255) / 256)); };
    hipLaunchKernelGGL(kl_dual_init_kernel, dim3(gB), dim3(256), 0, st, (int)B, oo->etabracket[0], oo->etabracket[1], oo->etabracket[2],
                       oo->del0, c.etab ? 0 : 1, s);
    DDP_HIP(hipMemsetAsync(W.kzero, 0, m * NB * 8, st));
    hipLaunchKernelGGL(kl_first_col_kernel, grid(n * B), dim3(256), 0, st, (int)n, (int)N, (int)B, c.x0, W.x0c);
    // STEP 1 (:86): derivs(x, u) with u = copy(traj_prev.k) (:45); a family evaluates every trajectory (no slot map: the loop recomputes all)
    if ((rc = M.df(h, (int)B, nullptr, c.x0, c.kp, nullptr, dv.fxw, dv.fuw, dv.cx, dv.cu, dv.cxx, dv.cxu, dv.cuu))) return rc;
    if (!cm && (rc = M.hessians(h, (int)B, nullptr, nullptr, hrep ? dv.hxx : dv.cxx, hrep ? dv.hxu : dv.cxu, hrep ? dv.huu : dv.cuu))) return rc;      // const_hessian only
    auto repeat = [&](size_t len, size_t cols, int batched, const double *src, double *dst) {      // dst[len, N, cols / N] = src[len (, b)]
        hipLaunchKernelGGL(kl_repeat_kernel, grid(len * cols), dim3(256), 0, st, (int)len, (int)N, (long)(len * cols), batched, src, dst);
    };
    if (hrep) { repeat(n * n, NB, 1, dv.hxx, dv.cxx); repeat(n * m, NB, 1, dv.hxu, dv.cxu); repeat(m * m, NB, 1, dv.huu, dv.cuu); }
    const size_t fxc = N * (fx_b ? B : 1);
    if (fx_rep) { repeat(n * n, fxc, fx_b, p->A, dv.fxw); repeat(n * m, fxc, fx_b, p->Bm, dv.fuw); }      // (a registered LTI problem)
    // a fitted model: the plan is made on its fx, fu (the fxw, fuw STEP 1 wrote stay in scratch) and every rollout below runs on its tables
    const double *fx = fit ? c.fit_fx : (fx_own ? dv.fxw : p->A), *fu = fit ? c.fit_fu : (fx_own ? dv.fuw : p->Bm);
    FitScope fit_scope(fit ? f : nullptr, c.fit_fx, c.fit_fu, c.fit_fc);
    if (!f) { repeat(n * n, N, 0, p->Q, dv.cxx); repeat(n * m, N, 0, nullptr, dv.cxu); repeat(m * m, N, 0, p->R, dv.cuu); }
    if ((rc = ddp_kl_terms_f64_dev(h, M.n, M.m, M.N, M.B, c.Kp, W.kzero, c.Sip, W.kt.cx, W.kt.cu, W.kt.cxx, W.kt.cxu, W.kt.cuu))) return rc;   // :90
    const double *cost0 = c.cost0;
    if (!cost0) {                                          // the reference insists on `cost` (:69); a C caller may leave it to costfun(x0, u)
        if ((rc = M.costfun(h, (int)B, nullptr, c.x0, c.kp, nullptr, c.cost, W.c0buf))) return rc;
        cost0 = W.c0buf;
    }
    // the problem's own linearisation: df(model, x, u) at (x0, kp) (forward_pass.jl:37-56); a fitted model: its fx
    const double *model_fx = c.model_fx ? c.model_fx : fx;
    const int model_fx_batched = c.model_fx ? c.model_fx_batched : 1;
    // a cost model: the backward passes take the caller's arrays (the cost derivatives STEP 1 wrote stay in scratch); cost0, the rollouts'
    // user cost and the loop are as without one
    gps.cx = cm ? c.cm_cx : dv.cx; gps.cu = cm ? c.cm_cu : dv.cu; gps.cxx = cm ? c.cm_cxx : dv.cxx; gps.cxu = cm ? c.cm_cxu : dv.cxu;
    gps.cuu = cm ? c.cm_cuu : dv.cuu; gps.fx = fx; gps.fu = fu; gps.lims = c.lims; gps.u = c.kp; gps.kl = &t;
    gps.K = c.K; gps.k = W.k; gps.Quu = c.Sigmai; gps.Vx = c.Vx; gps.Vxx = c.Vxx; gps.dV = c.dV; gps.diverge = W.dual.div; gps.Quui = c.Sigma;
    auto dual = [&](int op, int it, int *count) -> int {
        const int rcd = kl_dual_enqueue(h, op, (int)B, it, oo->kl_step, s, W.dual.div, W.dual.klm, W.counter);
        return rcd || !count ? rcd : kl_dual_poll(h, W.counter, count);
    };
    const double one = 1.0;
    int it = 0, live = (int)B;
    for (it = 1; it <= oo->max_iter && live > 0; ++it) {                                                  // :91
        if ((rc = dual(0, it, nullptr))) return rc;
        for (int guard = 0;; ++guard) {                    // back passes until the KL-regularised Quu is positive definite everywhere (:95-122)
            DDP_HIP(hipMemsetAsync(c.Sigma, 0, m * m * NB * 8, st));
            if ((rc = gps_launch(h, gps, kern))) return rc;
            int pending = 0;
            if ((rc = dual(1, it, &pending))) return rc;                                                   // :103-105
            if (!pending) break;
            DDP_CHECK(guard < 200, "ilqgkl: back_pass_gps keeps diverging (the reference would loop forever)");
        }
        rc = M.rollout(h, (int)B, nullptr, c.K, W.k, W.x0c, c.kp, c.x0, &one, 1, c.lims, nullptr, c.x, c.u, c.cost, W.cs);                  // :132
        if (rc) return rc;
        if ((rc = ddp_forward_covariance_f64_dev(h, M.n, M.m, M.N, M.B, model_fx, model_fx_batched, c.R1, c.K, c.Sigma, W.sig))) return rc;      // :133
        if ((rc = ddp_kl_div_f64_dev(h, M.n, M.m, M.N, M.B, c.x, c.x0, W.sig, c.K, W.k, c.Sigma, c.Kp, W.kzero, c.Sp, c.Sip, W.kld, W.dual.klm)))
            return rc;
        if ((rc = dual(2, it, &live))) return rc;                                                          // :141, :169-177
    }
    hipLaunchKernelGGL(kl_summary_kernel, dim3((unsigned)B), dim3(DDP_WAVE), 0, st, (int)m, (int)N, s, (const double *)W.k, c.kp,
                       (const double *)W.cs, cost0, (const double *)c.dV, c.stats);
    DDP_HIP(hipGetLastError());
    DDP_HIP(hipStreamSynchronize(st));
    if (c.iters) *c.iters = it - 1;
    return 0;
}

int ddp_ilqgkl_f64_dev(ddp_handle h, const ddp_problem *p, const ddp_ilqgkl_opts *oo, const double *x0, const double *cost0,
                       const double *Kp, const double *kp, const double *Sp, const double *Sip,
                       const double *model_fx, int model_fx_batched, const double *R1, const double *lims, double *etab,
                       double *x, double *u, double *K, double *Sigma, double *Sigmai, double *Vx, double *Vxx, double *cost,
                       double *dV, double *stats, int *iters_out)
{
    DDP_DEVICE(h);
    DDP_CHECK(p && model_fx, "ilqgkl: null argument");
    KlCall c;
    c.opts = oo; c.x0 = x0; c.cost0 = cost0; c.Kp = Kp; c.kp = kp; c.Sp = Sp; c.Sip = Sip; c.model_fx = model_fx;
    c.model_fx_batched = model_fx_batched; c.R1 = R1; c.lims = lims; c.etab = etab;
    c.x = x; c.u = u; c.K = K; c.Sigma = Sigma; c.Sigmai = Sigmai; c.Vx = Vx; c.Vxx = Vxx; c.cost = cost; c.dV = dV; c.stats = stats;
    c.iters = iters_out;
    return ilqgkl_impl(h, p, nullptr, c);
}

}   // extern "C"

int ddp_ilqgkl_family_dev(ddp_handle h, const ddp_family *f, const KlCall &c)
{
    DDP_DEVICE(h);
    DDP_CHECK(f, "ilqgkl: null problem");
    DDP_CHECK(!f->second_order, "ilqgkl: a DDP_USER_SECOND_ORDER problem is refused (back_pass_gps has no second-order variant); make the "
                                "problem without the flag for the KL loop");
    return ilqgkl_impl(h, nullptr, f, c);
}

extern "C" {


// host-pointer flavour of the driver: OWNED staging (the driver carves the handle's scratch itself), one upload, one download
int ddp_ilqgkl_f64(ddp_handle h, const ddp_problem *p, const ddp_ilqgkl_opts *o, const double *x0, const double *cost0,
                   const double *Kp, const double *kp, const double *Sp, const double *Sip,
                   const double *model_fx, int model_fx_batched, const double *R1, const double *lims, double *etab,
                   double *x, double *u, double *K, double *Sigma, double *Sigmai, double *Vx, double *Vxx, double *cost,
                   double *dV, double *stats, int *iters_out)
{
    DDP_DEVICE(h);
    DDP_CHECK(p && x0 && Kp && kp && Sp && Sip && model_fx && R1, "ilqgkl: null argument");
    const size_t n = p->n, m = p->m, N = p->N, B = p->B, CL = ddp_cost_len(p), NB = N * B;
    ddp_problem pd;
    const double *dx0, *dc0, *dKp, *dkp, *dSp, *dSip, *dmf, *dR1, *dl;
    double *det, *dx, *du, *dK, *dS, *dSi, *dVx, *dVxx, *dcost, *ddV, *dst;
    Staging S(h, Staging::OWNED, "ilqgkl");
    int rc = stage_problem(S, p, &pd);
    if (rc) return rc;
    DiagVerified diag_verified_(h);
    S.in(&dx0, x0, n * NB); S.in(&dc0, cost0, B); S.in(&dKp, Kp, m * n * NB); S.in(&dkp, kp, m * NB); S.in(&dSp, Sp, m * m * NB);
    S.in(&dSip, Sip, m * m * NB); S.in(&dmf, model_fx, n * n * N * (model_fx_batched ? B : 1)); S.in(&dR1, R1, n * n); S.in(&dl, lims, 2 * m);
    S.inout(&det, etab, 3 * B);
    // the driver writes every result: device storage also for those the caller leaves out
    S.out_or_temp(&dx, x, n * NB); S.out_or_temp(&du, u, m * NB); S.out_or_temp(&dK, K, m * n * NB); S.out_or_temp(&dS, Sigma, m * m * NB);
    S.out_or_temp(&dSi, Sigmai, m * m * NB); S.out_or_temp(&dVx, Vx, n * NB); S.out_or_temp(&dVxx, Vxx, n * n * NB);
    S.out_or_temp(&dcost, cost, CL * B); S.out_or_temp(&ddV, dV, 2 * B); S.out_or_temp(&dst, stats, DDP_ILQGKL_NSTATS * B);
    if ((rc = S.commit())) return rc;
    return S.finish(ddp_ilqgkl_f64_dev(h, &pd, o, dx0, dc0, dKp, dkp, dSp, dSip, dmf, model_fx_batched, dR1, dl, det, dx, du, dK, dS, dSi, dVx, dVxx,
                                       dcost, ddV, dst, iters_out));
}

// ---- host-pointer flavours (stage through the handle's scratch; PCIe-inclusive, for drop-in use with host arrays)
int ddp_kl_terms_f64(ddp_handle h, int n, int m, int N, int B, const double *K, const double *k, const double *Sigmai,
                     double *cx, double *cu, double *cxx, double *cxu, double *cuu)
{
    DDP_CHECK(h, "kl_terms: null handle");
    const size_t nb = (size_t)N * B, sn = n, sm = m;
    const double *dK, *dk, *dS;
    double *o0, *o1, *o2, *o3, *o4;
    Staging S(h, Staging::SCRATCH, "kl_terms");
    S.in(&dK, K, sm * sn * nb); S.in(&dk, k, sm * nb); S.in(&dS, Sigmai, sm * sm * nb);
    S.out(&o0, cx, sn * nb); S.out(&o1, cu, sm * nb); S.out(&o2, cxx, sn * sn * nb); S.out(&o3, cxu, sm * sn * nb); S.out(&o4, cuu, sm * sm * nb);
    const int rc = S.commit();
    if (rc) return rc;
    return S.finish(ddp_kl_terms_f64_dev(h, n, m, N, B, dK, dk, dS, o0, o1, o2, o3, o4));
}

int ddp_back_pass_gps_f64(ddp_handle h, const ddp_bp_desc *d,
                          const double *cx, const double *cu, const double *cxx, const double *cxu, const double *cuu,
                          const double *fx, const double *fu, const ddp_kl_cost_terms *kl,
                          const double *lims, const double *u,
                          double *K, double *k, double *Quu, double *Quui, double *Vx, double *Vxx, double *dV,
                          int32_t *diverge)
{
    DDP_CHECK(h && d && kl, "back_pass_gps: null handle/descriptor/kl terms");
    const size_t n = d->n, m = d->m, N = d->N, B = d->B, nb = N * B;
    const size_t fxc = N * (d->fx_batched ? B : 1), cc = N * (d->cost_batched ? B : 1);
    const double *dcx, *dcu, *dcxx, *dcxu, *dcuu, *dfx, *dfu, *dl = nullptr, *du = nullptr;
    ddp_kl_cost_terms kd;
    double *dK, *dk, *dQuu, *dQuui, *dVx, *dVxx, *ddV;
    int32_t *ddiv;
    Staging S(h, Staging::SCRATCH, "back_pass_gps");
    S.in(&dcx, cx, n * nb); S.in(&dcu, cu, m * nb); S.in(&dcxx, cxx, n * n * cc); S.in(&dcxu, cxu, n * m * cc); S.in(&dcuu, cuu, m * m * cc);
    S.in(&dfx, fx, n * n * fxc); S.in(&dfu, fu, n * m * fxc);
    if (d->has_lims) { S.in(&dl, lims, 2 * m); S.in(&du, u, m * nb); }
    S.in(&kd.cx, kl->cx, n * nb); S.in(&kd.cu, kl->cu, m * nb); S.in(&kd.cxx, kl->cxx, n * n * nb); S.in(&kd.cxu, kl->cxu, m * n * nb);
    S.in(&kd.cuu, kl->cuu, m * m * nb); S.in(&kd.eta, kl->eta, kl->eta_tv ? nb : B); kd.eta_tv = kl->eta_tv;
    S.out(&dK, K, m * n * nb); S.out(&dk, k, m * nb); S.out(&dQuu, Quu, m * m * nb); S.out(&dQuui, Quui, m * m * nb); S.out(&dVx, Vx, n * nb);
    S.out(&dVxx, Vxx, n * n * nb); S.out(&ddV, dV, 2 * B); S.out(&ddiv, diverge, B);
    const int rc = S.commit();
    if (rc) return rc;
    return S.finish(ddp_back_pass_gps_f64_dev(h, d, dcx, dcu, dcxx, dcxu, dcuu, dfx, dfu, &kd, dl, du, nullptr, dK, dk, dQuu, dQuui, dVx, dVxx, ddV, ddiv));
}

int ddp_forward_covariance_f64(ddp_handle h, int n, int m, int N, int B, const double *fx, int fx_batched,
                               const double *R1, const double *K, const double *Sigma, double *sigmanew)
{
    DDP_CHECK(h, "forward_covariance: null handle");
    const size_t nb = (size_t)N * B, p = (size_t)n + m;
    const double *dfx, *dR, *dK, *dS;
    double *o;
    Staging S(h, Staging::SCRATCH, "forward_covariance");
    S.in(&dfx, fx, (size_t)n * n * N * (fx_batched ? B : 1)); S.in(&dR, R1, (size_t)n * n); S.in(&dK, K, (size_t)m * n * nb); S.in(&dS, Sigma, (size_t)m * m * nb);
    S.out(&o, sigmanew, p * p * nb);
    const int rc = S.commit();
    if (rc) return rc;
    return S.finish(ddp_forward_covariance_f64_dev(h, n, m, N, B, dfx, fx_batched, dR, dK, dS, o));
}

int ddp_kl_div_f64(ddp_handle h, int n, int m, int N, int B, const double *xnew, const double *xold,
                   const double *sigmanew, const double *Kn, const double *kn, const double *Sn,
                   const double *Kp, const double *kp, const double *Sp, const double *Sip,
                   double *kldiv, double *klmean)
{
    DDP_CHECK(h, "kl_div: null handle");
    const size_t nb = (size_t)N * B, p = (size_t)n + m;
    const size_t sK = (size_t)m * n * nb, sk = (size_t)m * nb, sS = (size_t)m * m * nb;
    const double *a0, *a1, *a2, *a3, *a4, *a5, *a6, *a7, *a8, *a9;
    double *o0, *o1;
    Staging S(h, Staging::SCRATCH, "kl_div");
    S.in(&a0, xnew, n * nb); S.in(&a1, xold, n * nb); S.in(&a2, sigmanew, p * p * nb); S.in(&a3, Kn, sK); S.in(&a4, kn, sk); S.in(&a5, Sn, sS);
    S.in(&a6, Kp, sK); S.in(&a7, kp, sk); S.in(&a8, Sp, sS); S.in(&a9, Sip, sS);
    S.out_or_temp(&o0, kldiv, nb); S.out(&o1, klmean, (size_t)B);       // klmean is summed from kldiv: the kernel writes kldiv either way
    const int rc = S.commit();
    if (rc) return rc;
    return S.finish(ddp_kl_div_f64_dev(h, n, m, N, B, a0, a1, a2, a3, a4, a5, a6, a7, a8, a9, o0, o1));
}

}   // extern "C"
