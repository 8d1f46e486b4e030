// expect.hip — ddp_expected_cost: the moments and the expected cost of a linear-Gaussian policy under a fitted linear-Gaussian model
// and a fitted quadratic cost, the step that closes the guided-policy-search round (include/ddp_amd.h has the recursion).
//
// The time chain of a trajectory is serial: one work-group of four waves per trajectory, the batch is the parallelism.  With p = n + m,
// G = [fx fu] and Z = Σz, a step runs in four phases between work-group barriers; every matrix lives in LDS with the index of the
// lane (l & 15 of a tile product) contiguous and a leading dimension ld = 16 mod 32 (the comment at the top of fit.hip), and every
// product is xty of wide_tile.h on v_mfma_f64_16x16x4:
//   (A)  T = Sx K' (the xu and ux blocks of Z; Sx is the xx block, where the step before left it), waves 0 and 1;
//        δx = μx - x, δu = K δx, u + δu and the row of `mu`, wave 2
//   (B)  K T + Σ, the uu block of Z, upper triangle mirrored, wave 0
//   (C)  M = Z G' (p x n, kept transposed), at most 3 x 2 tiles dealt over the waves; the row of `sigma`; the sums of ec, every thread
//        on the entries of H it holds in registers, then a shuffle tree and one partial sum a wave; μx of the next step, wave 3
//   (D)  ec and its test, every thread from the four partial sums in a fixed order; Sx' = G M + cov, the upper tiles (at most 3),
//        mirrored into the xx block of Z
// The operands of the steps ahead are on their way while step i computes.  Behind (D) every thread puts its contiguous share of [fx fu],
// K and the short vectors of step i + 1 from registers into LDS and then asks for its shares of step i + 2, and for H and cov of step
// i + 1, which stay in registers (they never go to LDS): all requests of a step leave from this one place, behind the last use of the
// registers they fill, because the wait in front of the first use of any of them is a wait for all of them — it comes in (C) of the
// next step, three barriers later.  Nothing depends on B or on the other trajectories: two calls give the same bits, and a slice of the
// trajectories gives the bits of that slice.
#include <float.h>
#include <math.h>
#include "ddp_internal.h"
#include "wide_tile.h"
#include "staging.h"

namespace {

constexpr int EX_NMAX = DDP_MAX_N_GENERIC, EX_MMAX = DDP_MAX_M, EX_PMAX = EX_NMAX + EX_MMAX;
__host__ __device__ constexpr int ex_ld(int r) { return (r + 15) / 32 * 32 + 16; }                  // ld >= r, ld = 16 mod 32
constexpr int EX_LD = ex_ld(EX_PMAX);                                                                // 48
constexpr int EX_GQ = cdivw(EX_NMAX * EX_PMAX, 256), EX_HQ = cdivw(EX_NMAX * EX_NMAX, 256);          // a thread's share of G: 5, of cxx: 4
constexpr int EX_SMALL = EX_MMAX * EX_MMAX + 3 * EX_NMAX + 2 * EX_MMAX + 1;                          // Σ, fc, cx, x, cu, u, c0
static_assert(EX_SMALL <= 256 && EX_MMAX * EX_NMAX <= 256, "one entry of K and one of the short vectors a thread");
static_assert((3 * EX_LD * EX_PMAX + EX_MMAX * EX_NMAX + EX_SMALL + 2 * EX_NMAX + EX_PMAX + EX_MMAX + 4) * sizeof(double) <= 65536,
              "static LDS of ddp_expected_cost");

struct ExArgs {
    int n, m, N, model_b, cost_b;
    const double *K, *Sigma, *x0, *x, *u, *fx, *fu, *fc, *cov, *cx, *cu, *cxx, *cxu, *cuu, *c0, *Sigma0;
    double *ec, *mu, *sigma;
    int32_t *status;
};

__global__ __launch_bounds__(256) void ddp_expected_cost(ExArgs a)
{
    __shared__ double Z[EX_LD * EX_PMAX];                        // Σz of the step, Z[r + ldz c]; its xx block is Sx
    __shared__ double Mt[EX_LD * EX_PMAX];                       // (Σz G')' : Mt[j + ldn k] = M[k][j]
    __shared__ double G[EX_LD * EX_PMAX];                        // [fx fu] : G[j + ldn k]
    __shared__ double Ks[EX_MMAX * EX_NMAX];                     // K[j + m k]
    __shared__ double sm[EX_SMALL];                              // Σ | fc | cx | cu | x | u | c0 of the step
    __shared__ double mux[2][EX_NMAX];
    __shared__ double dz[EX_PMAX];                               // [δx; δu]
    __shared__ double un[EX_MMAX];                               // u + δu
    __shared__ double red[4];                                    // ec - c0, one partial sum a wave
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l15 = lane & 15, l4 = lane >> 4;
    const int n = a.n, m = a.m, p = n + m, N = a.N, ldz = ex_ld(p), ldn = ex_ld(n);
    const int b = blockIdx.x;
    const size_t pb = (size_t)N * b, mb = a.model_b ? pb : 0, cb = a.cost_b ? pb : 0;
    const int oS = 0, oFc = m * m, oCx = oFc + n, oCu = oCx + n, oX = oCu + m, oU = oX + n, oC0 = oU + m, nsm = oC0 + 1;
    const int ntn = cdivw(n, 16), ntp = cdivw(p, 16);
    // the tile of Sx' this wave owns in (D): (0,0), (0,1), (1,1)
    const int dbi = wave == 2 ? 1 : 0, dbj = wave == 0 ? 0 : 1;
    const bool dtile = wave < ntn * (ntn + 1) / 2;

    double rG[EX_GQ], rK = 0.0, rS = 0.0, rHxx[EX_HQ], rHxu = 0.0, rHuu = 0.0, rCov[4];
    auto loadG = [&](int i) {                                    // [fx_i fu_i] is n p contiguous doubles in two runs
        const double *fx = a.fx + (size_t)n * n * (mb + i), *fu = a.fu + (size_t)n * m * (mb + i);
#pragma unroll
        for (int q = 0; q < EX_GQ; ++q) {
            const int e = tid + 256 * q;
            rG[q] = e < n * n ? fx[e] : (e < n * p ? fu[e - n * n] : 0.0);
        }
    };
    auto storeG = [&]() {
#pragma unroll
        for (int q = 0; q < EX_GQ; ++q) {
            const int e = tid + 256 * q, c = e / n;
            if (e < n * p) G[e - c * n + ldn * c] = rG[q];
        }
    };
    auto loadSmall = [&](int i) {
        const size_t s = pb + i;
        rK = tid < m * n ? a.K[(size_t)m * n * s + tid] : 0.0;
        double v = 0.0;
        if (tid < oFc) v = a.Sigma ? a.Sigma[(size_t)m * m * s + tid] : 0.0;
        else if (tid < oCx) v = i < N - 1 ? a.fc[(size_t)n * (mb + i) + (tid - oFc)] : 0.0;      // slot N - 1 of the dynamics is not read
        else if (tid < oCu) v = a.cx[(size_t)n * (cb + i) + (tid - oCx)];
        else if (tid < oX) v = a.cu[(size_t)m * (cb + i) + (tid - oCu)];
        else if (tid < oU) v = a.x[(size_t)n * s + (tid - oX)];
        else if (tid < oC0) v = a.u[(size_t)m * s + (tid - oU)];
        else if (tid < nsm) v = a.c0[cb + i];
        rS = v;
    };
    auto storeSmall = [&]() {
        if (tid < m * n) Ks[tid] = rK;
        if (tid < nsm) sm[tid] = rS;
    };
    auto loadH = [&](int i) {
        const double *cxx = a.cxx + (size_t)n * n * (cb + i);
#pragma unroll
        for (int q = 0; q < EX_HQ; ++q) { const int e = tid + 256 * q; rHxx[q] = e < n * n ? cxx[e] : 0.0; }
        rHxu = tid < n * m ? a.cxu[(size_t)n * m * (cb + i) + tid] : 0.0;
        rHuu = tid < m * m ? a.cuu[(size_t)m * m * (cb + i) + tid] : 0.0;
    };
    auto loadCov = [&](int i) {                                  // the entries of cov_i the lane adds to its tile of Sx' (upper triangle)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int ii = 16 * dbi + l4 + 4 * r, jj = 16 * dbj + l15;
            rCov[r] = (a.cov && dtile && ii <= jj && jj < n) ? a.cov[(size_t)n * n * (mb + i) + ii + n * jj] : 0.0;
        }
    };

    // step 0: Sx_0 = Sigma0 (its upper triangle, mirrored) or 0, μx_0 = x0 or x[:, 0]
    for (int e = tid; e < n * n; e += 256) {
        const int c = e / n, r = e - c * n;
        Z[r + ldz * c] = a.Sigma0 ? a.Sigma0[(size_t)n * n * b + (r < c ? r + n * c : c + n * r)] : 0.0;
    }
    if (tid < n) mux[0][tid] = a.x0 ? a.x0[(size_t)n * b + tid] : a.x[(size_t)n * pb + tid];
    loadSmall(0);
    storeSmall();
    if (N > 1) { loadG(0); storeG(); }
    // one place a step where loads are asked for, behind the last use of what they replace: a wait for one of them waits for all
    loadH(0);
    if (N > 1) { loadCov(0); loadSmall(1); }
    if (N > 2) loadG(1);
    __syncthreads();

    int cur = 0, fail = 0;
    for (int i = 0; i < N; ++i) {
        const bool last = i == N - 1;

        // (A)
        if (wave < ntn) {
            const d4 t = xty(Z, ldz, 1, 16 * wave, n, Ks, m, 1, 0, m, n, d4{0.0, 0.0, 0.0, 0.0}, l15, l4);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int ii = 16 * wave + l4 + 4 * r;
                if (ii < n && l15 < m) { const double v = comp(t, r); Z[(n + l15) + ldz * ii] = v; Z[ii + ldz * (n + l15)] = v; }
            }
        } else if (wave == 2) {
            double mxv = 0.0;
            if (lane < n) { mxv = mux[cur][lane]; dz[lane] = mxv - sm[oX + lane]; }
            wave_sync();
            if (lane < m) {
                double s = 0.0;
#pragma unroll 8
                for (int k = 0; k < n; ++k) s += Ks[lane + m * k] * dz[k];
                dz[n + lane] = s;
                un[lane] = sm[oU + lane] + s;
            }
            wave_sync();
            if (a.mu) {
                double *mu = a.mu + (size_t)p * (pb + i);
                if (lane < n) mu[lane] = mxv;
                else if (lane < p) mu[lane] = un[lane - n];
            }
        }
        __syncthreads();

        // (B)
        if (wave == 0) {
            const d4 t = xty(Ks, m, 1, 0, m, Z + n, ldz, 1, 0, m, n, d4{0.0, 0.0, 0.0, 0.0}, l15, l4);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int ii = l4 + 4 * r;
                if (ii <= l15 && l15 < m) {
                    const double v = comp(t, r) + sm[oS + ii + m * l15];
                    Z[(n + ii) + ldz * (n + l15)] = v; Z[(n + l15) + ldz * (n + ii)] = v;
                }
            }
        }
        __syncthreads();

        // (C)
        if (!last)
            for (int item = wave; item < ntp * ntn; item += 4) {
                const int bi = item / ntn, bj = item - bi * ntn;
                const d4 t = xty(Z, ldz, 1, 16 * bi, p, G, ldn, 1, 16 * bj, n, p, d4{0.0, 0.0, 0.0, 0.0}, l15, l4);
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int ii = 16 * bi + l4 + 4 * r, jj = 16 * bj + l15;
                    if (ii < p && jj < n) Mt[jj + ldn * ii] = comp(t, r);
                }
            }
        if (a.sigma) {
            double *sg = a.sigma + (size_t)p * p * (pb + i);
            for (int e = tid; e < p * p; e += 256) { const int c = e / p; sg[e] = Z[e - c * p + ldz * c]; }
        }
        const double c0v = sm[oC0];
        {
            // cx'δx | cu'δu | δz' H δz | tr(H Σz), over the entries of H of this thread; the xu block of H counts twice
            double t2 = tid < n ? sm[oCx + tid] * dz[tid] : 0.0, t3 = (tid >= n && tid < p) ? sm[oCu + tid - n] * dz[tid] : 0.0, t4 = 0.0, t5 = 0.0;
#pragma unroll
            for (int q = 0; q < EX_HQ; ++q) {
                const int e = tid + 256 * q, c = e / n, r = e - c * n;
                if (e < n * n) { t4 += rHxx[q] * (dz[r] * dz[c]); t5 += rHxx[q] * Z[r + ldz * c]; }
            }
            if (tid < n * m) { const int c = tid / n, r = tid - c * n; t4 += 2.0 * rHxu * (dz[r] * dz[n + c]); t5 += 2.0 * rHxu * Z[r + ldz * (n + c)]; }
            if (tid < m * m) { const int c = tid / m, r = tid - c * m; t4 += rHuu * (dz[n + r] * dz[n + c]); t5 += rHuu * Z[(n + r) + ldz * (n + c)]; }
            // one value a thread through the shuffle tree (each stage is a round trip through the LDS crossbar): the thread's share of
            // ec - c0, whose rounding is still measured by the sum of the absolute values of the terms
            double t = (t2 + t3) + 0.5 * (t4 + t5);
            for (int o = 32; o >= 1; o >>= 1) t += __shfl_xor(t, o, 64);
            if (lane == 0) red[wave] = t;
        }
        if (wave == 3 && !last && lane < n) {                    // μx of the next step
            double s = 0.0;
#pragma unroll 8
            for (int k = 0; k < n; ++k) s += G[lane + ldn * k] * mux[cur][k];
            for (int c = 0; c < m; ++c) s += G[lane + ldn * (n + c)] * un[c];
            mux[cur ^ 1][lane] = s + sm[oFc + lane];
        }
        __syncthreads();

        // (D)
        const double ec = c0v + ((red[0] + red[1]) + (red[2] + red[3]));
        if (!(fabs(ec) <= DBL_MAX)) { fail = i + 1; break; }     // (the same value in every thread)
        if (tid == 0) a.ec[pb + i] = ec;
        if (!last) {
            if (dtile) {
                const d4 t = xty(G, ldn, 1, 16 * dbi, n, Mt, ldn, 1, 16 * dbj, n, p, d4{0.0, 0.0, 0.0, 0.0}, l15, l4);
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int ii = 16 * dbi + l4 + 4 * r, jj = 16 * dbj + l15;
                    if (ii <= jj && jj < n) { const double v = comp(t, r) + rCov[r]; Z[ii + ldz * jj] = v; Z[jj + ldz * ii] = v; }
                }
            }
        }
        cur ^= 1;
        __syncthreads();
        // the operands of step i + 1 -> LDS (every reader of step i is behind the barrier), then the requests for what follows them
        if (!last) {
            storeSmall();
            if (i + 1 < N - 1) storeG();
            loadH(i + 1);
            if (i + 1 < N - 1) loadCov(i + 1);
            if (i + 2 < N) loadSmall(i + 2);
            if (i + 2 < N - 1) loadG(i + 2);
            __syncthreads();
        }
    }

    // from the first step whose ec is not finite on, the outputs of the trajectory are NaN (the threads that wrote a row rewrite it)
    if (fail) {
        const double nan = __builtin_nan("");
        for (int i = fail - 1; i < N; ++i) {
            if (tid == 0) a.ec[pb + i] = nan;
            if (a.mu && wave == 2 && lane < p) a.mu[(size_t)p * (pb + i) + lane] = nan;
            if (a.sigma)
                for (int e = tid; e < p * p; e += 256) a.sigma[(size_t)p * p * (pb + i) + e] = nan;
        }
    }
    if (tid == 0) a.status[b] = fail;
}

// what both entries refuse, before the handle is looked at
int ex_validate(int n, int m, int N, int B, const void *K, const void *x, const void *u, const void *fx, const void *fu, const void *fc,
                int model_batched, const void *cx, const void *cu, const void *cxx, const void *cxu, const void *cuu, const void *c0,
                int cost_batched, const void *ec, const void *status)
{
    DDP_CHECK(n >= 1 && n <= EX_NMAX, "expected_cost: n = %d out of [1, %d]", n, EX_NMAX);
    DDP_CHECK(m >= 1 && m <= EX_MMAX, "expected_cost: m = %d out of [1, %d]", m, EX_MMAX);
    DDP_CHECK(N >= 1 && B >= 1, "expected_cost: N = %d, B = %d (both >= 1)", N, B);
    DDP_CHECK(model_batched == 0 || model_batched == 1, "expected_cost: model_batched = %d (0: one model for the batch, 1: one per trajectory)", model_batched);
    DDP_CHECK(cost_batched == 0 || cost_batched == 1, "expected_cost: cost_batched = %d (0: one cost model for the batch, 1: one per trajectory)", cost_batched);
    DDP_CHECK(K && x && u && fx && fu && fc && cx && cu && cxx && cxu && cuu && c0 && ec && status, "expected_cost: null argument");
    return 0;
}

}   // namespace

extern "C" {

int ddp_expected_cost_f64_dev(ddp_handle h, int n, int m, int N, int B, const double *K, const double *Sigma, const double *x0,
                              const double *x, const double *u, const double *fx, const double *fu, const double *fc, const double *cov,
                              int model_batched, const double *cx, const double *cu, const double *cxx, const double *cxu,
                              const double *cuu, const double *c0, int cost_batched, const double *Sigma0, double *ec, int32_t *status,
                              double *mu, double *sigma)
{
    { const int rc = ex_validate(n, m, N, B, K, x, u, fx, fu, fc, model_batched, cx, cu, cxx, cxu, cuu, c0, cost_batched, ec, status); if (rc) return rc; }
    DDP_DEVICE(h);
    ExArgs a{};
    a.n = n; a.m = m; a.N = N; a.model_b = model_batched; a.cost_b = cost_batched;
    a.K = K; a.Sigma = Sigma; a.x0 = x0; a.x = x; a.u = u; a.fx = fx; a.fu = fu; a.fc = fc; a.cov = cov;
    a.cx = cx; a.cu = cu; a.cxx = cxx; a.cxu = cxu; a.cuu = cuu; a.c0 = c0; a.Sigma0 = Sigma0;
    a.ec = ec; a.mu = mu; a.sigma = sigma; a.status = status;
    hipLaunchKernelGGL(ddp_expected_cost, dim3((unsigned)B), dim3(256), 0, h->stream, a);
    DDP_HIP(hipGetLastError());
    return 0;
}

int ddp_expected_cost_f64(ddp_handle h, int n, int m, int N, int B, const double *K, const double *Sigma, const double *x0,
                          const double *x, const double *u, const double *fx, const double *fu, const double *fc, const double *cov,
                          int model_batched, const double *cx, const double *cu, const double *cxx, const double *cxu,
                          const double *cuu, const double *c0, int cost_batched, const double *Sigma0, double *ec, int32_t *status,
                          double *mu, double *sigma)
{
    { const int rc = ex_validate(n, m, N, B, K, x, u, fx, fu, fc, model_batched, cx, cu, cxx, cxu, cuu, c0, cost_batched, ec, status); if (rc) return rc; }
    const size_t nb = (size_t)N * B, sn = n, sm = m, p = sn + sm, mc = (size_t)N * (model_batched ? B : 1), cc = (size_t)N * (cost_batched ? B : 1);
    if (Sigma0)
        for (size_t e = 0; e < sn * sn * B; ++e)
            DDP_CHECK(fabs(Sigma0[e]) <= DBL_MAX, "expected_cost: Sigma0 is not finite (entry %zu of trajectory %zu)", e % (sn * sn), e / (sn * sn));
    DDP_DEVICE(h);
    const double *dK, *dSg, *dx0, *dx, *du, *dfx, *dfu, *dfc, *dcov, *dcx, *dcu, *dcxx, *dcxu, *dcuu, *dc0, *dS0;
    double *dec, *dmu, *dsig;
    int32_t *dst;
    Staging St(h, Staging::SCRATCH, "expected_cost");
    St.in(&dK, K, sm * sn * nb); St.in(&dSg, Sigma, sm * sm * nb); St.in(&dx0, x0, sn * B); St.in(&dx, x, sn * nb); St.in(&du, u, sm * nb);
    St.in(&dfx, fx, sn * sn * mc); St.in(&dfu, fu, sn * sm * mc); St.in(&dfc, fc, sn * mc); St.in(&dcov, cov, sn * sn * mc);
    St.in(&dcx, cx, sn * cc); St.in(&dcu, cu, sm * cc); St.in(&dcxx, cxx, sn * sn * cc); St.in(&dcxu, cxu, sn * sm * cc);
    St.in(&dcuu, cuu, sm * sm * cc); St.in(&dc0, c0, cc); St.in(&dS0, Sigma0, sn * sn * B);
    St.out(&dec, ec, nb); St.out(&dst, status, (size_t)B); St.out(&dmu, mu, p * nb); St.out(&dsig, sigma, p * p * nb);
    const int rc = St.commit();
    if (rc) return rc;
    return St.finish(ddp_expected_cost_f64_dev(h, n, m, N, B, dK, dSg, dx0, dx, du, dfx, dfu, dfc, dcov, model_batched, dcx, dcu, dcxx, dcxu,
                                               dcuu, dc0, cost_batched, dS0, dec, dst, dmu, dsig));
}

}   // extern "C"
