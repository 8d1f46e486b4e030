// back_pass_wide_kernel.h — the step of the wide-control backward pass (back_pass_wide.hip has the mapping and the phases P1-P4): the LDS
// plan, the cross-lane Cholesky and box-QP of P3 and the kernel body, for both compilers.  back_pass_wide.hip includes it; build.py hands
// its text (and that of wide_tile.h) to user_problem.hip, whose ddp_user_back_pass2_wave is the same body compiled by hiprtc with n, m as
// constants and a curvature phase P0 in front of P1.  What it needs besides wide_tile.h and boxqp_dev.h (QPOptsDev, ddp_clamp): wave_sync,
// int32_t and DDP_MAX_M_WIDE, which a hiprtc program gets from a small prelude (kUserWidePrelude, user_problem_kernels.h).
#pragma once
#include "ddp_internal.h"
#include "boxqp_dev.h"      // QPOptsDev, ddp_clamp
#include "wide_tile.h"      // xty, inv_wave

namespace {

constexpr int WT = 256;                 // threads per work-group (four waves)
constexpr int WIDE_WAVE = 64;            // lanes of a wave (DDP_WAVE of ddp_internal.h; a user program has a macro of that name)
constexpr int NWAVE = WT / WIDE_WAVE;
constexpr int WIDE_MAX_N = 64, WIDE_MAX_M = DDP_MAX_M_WIDE;
constexpr int WIDE_LDS_BYTES = 160 * 1024;

struct BPWArgs {
    int n, m, N, B, regType, has_lims;
    long fx_t, fx_b, fu_t, fu_b, cxx_t, cxx_b, cxu_t, cxu_b, cuu_t, cuu_b;      // element strides per time step / per trajectory (0: shared)
    const double *cx, *cu, *cxx, *cxu, *cuu, *fx, *fu, *lambda, *lims, *u;
    const int32_t *active;
    double *K, *k, *Quu, *Vx, *Vxx, *dV;
    int32_t *diverge;
    // back_pass_gps only: the KL terms [., N, B], η [B] or [N, B], and inv(Quu)
    const double *cxkl, *cukl, *cxxkl, *cxukl, *cuukl, *eta;
    int eta_tv;
    double *Quui;
};

// LDS map (doubles).  Two regions change hands inside a step:
//   V : Vxx_{i+1} (ldn x n) for P1;  then H = QuuF (ldm x m) | Kx = Qux_reg -> K in place (ldm x n) for P2-P4;  then M, Vxx_i (P4)
//   G : Gt (ldn x (n+m)) for P1-P2;  then R = the Cholesky factor (ldm x m) | T (ldm x n) for P3-P4
// back_pass_gps adds the [Quu | inv(Quu) | pivot column] image of inv_wave: behind R | T in the G region where that has the room (at
// (64, 32) it has, and nothing else would fit under the 160 KB), else a region of its own.
struct WLds {
    int ldn = 0, ldm = 0, F = 0, V = 0, G = 0, Qux = 0, Quu = 0, Qs = 0, vs = 0, ks = 0, Quuk = 0, xb = 0, sb = 0, flags = 0, inv = 0, total = 0;
    __host__ __device__ constexpr WLds(int n, int m, bool gps = false)
    {
        const int p = n + m;
        ldn = ld4(n); ldm = ld4(m);
        int o = 0;
        F = o; o += ldn * p;
        V = o; o += imax(ldn * n, ldm * p);
        G = o; o += imax(ldn * p, ldm * p);
        Qux = o; o += ldm * n;
        Quu = o; o += ldm * m;
        Qs = o; o += even(p);
        vs = o; o += even(n);
        ks = o; o += even(m);
        Quuk = o; o += even(m);
        xb = o; o += even(m);           // box-QP: the vector a matrix-vector product reads
        sb = o; o += even(m);           // box-QP: the terms of a sum
        flags = o; o += 2;              // two ints: failure, free mask
        inv = 0;
        if (gps) {
            if (ldm * p + inv_wave_len(ldm, m) <= imax(ldn * p, ldm * p)) inv = G + ldm * p;
            else { inv = o; o += even(inv_wave_len(ldm, m)); }
        }
        total = o;
    }
};

// ---- wave-level pieces of P3 (wave 0; `lane` is the coordinate)
// every lane gets sum_{i < m} v_i, added in index order (the order of the reference's loops)
__device__ __forceinline__ double wsum(double v, double *sb, int lane, int m)
{
    if (lane < m) sb[lane] = v;
    wave_sync();
    double s = 0.0;
    for (int i = 0; i < m; ++i) s += sb[i];
    wave_sync();
    return s;
}

// Upper Cholesky of H[free, free] (upper triangle read, LAPACK potrf 'U'), lane i computes column i; the factor goes to the same
// positions of R (entries of clamped rows / columns are not touched and never read).  0, or j + 1 at the first non-positive pivot.
__device__ int chol_wave(const double *H, double *R, int ldm, int m, unsigned freem, int lane)
{
    const int li = lane < m ? lane : 0;
    for (int j = 0; j < m; ++j) {
        if (!((freem >> j) & 1u)) continue;
        double s = 0.0;
        if (lane < m && lane >= j) {
            s = H[j + ldm * li];
            for (int k = 0; k < j; ++k)
                if ((freem >> k) & 1u) s -= R[k + ldm * j] * R[k + ldm * li];
        }
        const double ajj = __shfl(s, j);
        if (!(ajj > 0.0)) return j + 1;
        const double dj = sqrt(ajj);
        if (lane == j) R[j + ldm * j] = dj;
        else if (lane > j && lane < m && ((freem >> lane) & 1u)) R[j + ldm * lane] = s / dj;
        wave_sync();
    }
    return 0;
}

// (x'g + 0.5x'H*x) of boxQP.jl:63,141,146: x'g, then (0.5x')*H, then *x
__device__ __forceinline__ double qp_value(const double *H, int ldm, int m, double g, double x, double *xb, double *sb, int lane)
{
    const int li = lane < m ? lane : 0;
    if (lane < m) xb[lane] = x;
    const double xg = wsum(lane < m ? x * g : 0.0, sb, lane, m);        // (its hand-off publishes xb too)
    double t = 0.0;
    for (int i = 0; i < m; ++i) t += (0.5 * xb[i]) * H[i + ldm * li];
    const double q = wsum(lane < m ? t * x : 0.0, sb, lane, m);
    return xg + q;
}

// g + H v for the lane's row
__device__ __forceinline__ double qp_grad(const double *H, int ldm, int m, double g, double v, double *xb, int lane)
{
    const int li = lane < m ? lane : 0;
    wave_sync();
    if (lane < m) xb[lane] = v;
    wave_sync();
    double s = 0.0;
    for (int j = 0; j < m; ++j) s += H[li + ldm * j] * xb[j];
    return g + s;
}

// boxQP(H, g, lower, upper, x0) of boxQP.jl:46-169, statement by statement: one coordinate per lane, wave-uniform control
// flow (every test is made on a value all lanes hold).  Returns `result`; x is the lane's coordinate of the solution, freem the free
// set, R the factor of H[free, free] (valid whenever freem != 0).
__device__ int boxqp_wave(const double *H, double *R, int ldm, int m, double g, double lo, double up, double x0, double *xb, double *sb,
                          int lane, double &xout, unsigned &freeout)
{
    const QPOptsDev o = {100, 1e-8, 1e-8, 0.6, 1e-22, 0.1};             // boxQP.jl:30-35
    const bool in = lane < m;
    const int li = in ? lane : 0;
    const unsigned full = m >= 32 ? 0xffffffffu : ((1u << m) - 1u);
    unsigned clampedm = 0u, freem = full;
    int result = 0, iter = 1;
    double x = in ? ddp_clamp(x0, lo, up) : 0.0;                        // :58
    double value = qp_value(H, ldm, m, g, x, xb, sb, lane), oldvalue = 0.0;   // :63
    while (iter <= o.maxIter) {                                         // :71
        if (result != 0) break;                                         // :73-75
        if (iter > 1 && (oldvalue - value) < o.minRelImprove * fabs(oldvalue)) { result = 4; break; }   // :78-81
        oldvalue = value;
        const double grad = qp_grad(H, ldm, m, g, x, xb, lane);         // :85
        const bool cl = in && (((x == lo) && (grad > 0)) || ((x == up) && (grad < 0)));   // :88-95
        const unsigned newm = (unsigned)__ballot(cl);
        const bool changed = newm != clampedm;
        clampedm = newm;
        freem = full & ~newm;
        if (freem == 0u) { result = 6; break; }                         // :98-101
        if (iter == 1 || changed) {                                     // :104-117
            wave_sync();
            if (chol_wave(H, R, ldm, m, freem, lane) != 0) { result = 0; xout = x; freeout = freem; return 0; }
        }
        const bool isfree = in && !cl;
        const double gn = sqrt(wsum(isfree ? grad * grad : 0.0, sb, lane, m));   // :120-124
        if (gn < o.minGrad) { result = 5; break; }
        const double gc = qp_grad(H, ldm, m, g, cl ? x : 0.0, xb, lane);      // :127  g + H*(x.*clamped)
        double b = isfree ? gc : 0.0;                                   // :128-129  (R'R) \ gc[free]
        for (int k = 0; k < m; ++k) {                                   // R'y = b: y_i = (b_i - sum_{k<i} R[k,i] y_k) / R[i,i]
            if (!((freem >> k) & 1u)) continue;
            if (lane == k) b = b / R[k + ldm * k];
            const double bk = __shfl(b, k);
            if (isfree && lane > k) b -= R[k + ldm * li] * bk;
        }
        for (int k = m - 1; k >= 0; --k) {                              // R x = y
            if (!((freem >> k) & 1u)) continue;
            if (lane == k) b = b / R[k + ldm * k];
            const double bk = __shfl(b, k);
            if (isfree && lane < k) b -= R[li + ldm * k] * bk;
        }
        const double search = isfree ? -b - x : 0.0;
        const double sdotg = wsum(in ? search * grad : 0.0, sb, lane, m);    // :132-135
        if (sdotg >= 0) break;                                          // result stays 0 (the reference's own exit)
        double step = 1.0;                                              // :138-151
        double xc = in ? ddp_clamp(x + step * search, lo, up) : 0.0;
        double vc = qp_value(H, ldm, m, g, xc, xb, sb, lane);
        while ((vc - oldvalue) / (step * sdotg) < o.Armijo) {
            step = step * o.stepDec;
            xc = in ? ddp_clamp(x + step * search, lo, up) : 0.0;
            vc = qp_value(H, ldm, m, g, xc, xb, sb, lane);
            if (step < o.minStep) { result = 2; break; }
        }
        x = xc;                                                         // :161-163
        value = vc;
        iter += 1;
    }
    if (iter == o.maxIter) result = 1;                                  // :167-169
    xout = x;
    freeout = freem;
    return result;
}

// b <- -(R'R) \ b over the free coordinates (potrs), zero at the clamped ones; b is a column in the LDS, one thread per column
__device__ __forceinline__ void solve_col(double *b, const double *R, int ldm, int m, unsigned freem)
{
    for (int i = 0; i < m; ++i) {
        if (!((freem >> i) & 1u)) continue;
        double s = b[i];
        for (int k = 0; k < i; ++k)
            if ((freem >> k) & 1u) s -= R[k + ldm * i] * b[k];
        b[i] = s / R[i + ldm * i];
    }
    for (int i = m - 1; i >= 0; --i) {
        if (!((freem >> i) & 1u)) continue;
        double s = b[i];
        for (int k = i + 1; k < m; ++k)
            if ((freem >> k) & 1u) s -= R[i + ldm * k] * b[k];
        b[i] = s / R[i + ldm * i];
    }
    for (int i = 0; i < m; ++i) b[i] = ((freem >> i) & 1u) ? -b[i] : 0.0;
}

// the curvature hooks of a kernel without a curvature phase (the precompiled kernels): nothing is compiled in
struct WNoCurv {
    static constexpr bool on = false;
    __device__ __forceinline__ void p0(int, const double *, int) const {}
    __device__ __forceinline__ double h(int, int) const { return 0.0; }
};

// The kernel body.  GPS: back_pass_gps (backward_pass.jl:259-350) on the same phases — every Q• is Q•/η + c•kl, no λ; Quu is symmetrised
// and is the matrix that is factorised; wave 1 inverts it in P3 (Gauss-Jordan across its lanes) while wave 0 solves for the gains.
// CN, CM > 0: n and m are these constants (a program compiled for one shape), 0: a.n, a.m at run time, sized for WIDE_MAX_N, WIDE_MAX_M.
// Curv::on: the second-order pass (backward_pass.jl:81-160).  curv.p0(i, Vx_{i+1}, t) runs on all WT threads in front of P1 and leaves
// H_i = ∇²_z (Vx_{i+1}·f)(x_i, u_i), z = [x; u], where curv.h(a, b) reads entry (a, b) after the barrier that ends P1; P2 starts the
// accumulators of Qxx, Qux | Qux_reg and Quu | QuuF from the cost Hessians plus these entries (:106-123).
// Every thread of the work-group reaches every barrier: the early returns and the divergence exit are taken by all of them.
template <bool GPS, int CN, int CM, class Curv>
__device__ __forceinline__ void back_pass_wide_body(const BPWArgs &a, double *lds, const Curv &curv)
{
    const int b = blockIdx.x, t = threadIdx.x;
    if (a.active && a.active[b] == 0) return;
    const int lane = t & (WIDE_WAVE - 1), w = t / WIDE_WAVE, l15 = lane & 15, l4 = lane >> 4;
    const int n = CN > 0 ? CN : a.n, m = CM > 0 ? CM : a.m, N = a.N, p = n + m;
    constexpr int SN = CN > 0 ? CN : WIDE_MAX_N, SM = CM > 0 ? CM : WIDE_MAX_M;        // what the per-thread arrays are sized for
    const int NT = cdivw(n, 16), MT = cdivw(m, 16), PT = cdivw(p, 16);
    constexpr int QS = cdivw(cdivw(SN, 16) * cdivw(SN, 16), NWAVE);                                       // Qxx tiles per wave
    constexpr int US = cdivw(cdivw(SM, 16) * (cdivw(SN, 16) + cdivw(SM, 16)), NWAVE);             // u-row tiles per wave
    constexpr int TS = cdivw(cdivw(SM, 16) * cdivw(SN, 16), NWAVE);                                       // T tiles per wave
    constexpr int RV = cdivw(SN * SN, WT);                                                                // Vxx entries per thread

    const WLds L(n, m, GPS);
    const int ldn = L.ldn, ldm = L.ldm;
    double *Fs = lds + L.F, *Vs = lds + L.V, *Gt = lds + L.G, *Quxs = lds + L.Qux, *Quus = lds + L.Quu, *Qs = lds + L.Qs, *vs = lds + L.vs,
           *ks = lds + L.ks, *Quuks = lds + L.Quuk, *xb = lds + L.xb, *sb = lds + L.sb;
    int *flags = (int *)(lds + L.flags);
    double *Hs = Vs, *Kx = Vs + ldm * m;        // QuuF; Qux_reg, then K in place
    double *Rs = Gt, *Ts = Gt + ldm * m;        // the Cholesky factor; T = Quu K + Qux
    const double *Fu = Fs + ldn * n;            // the fu columns of [fx fu]

    const size_t nn = (size_t)n * n, nm = (size_t)n * m, mm = (size_t)m * m;
    const double *cx = a.cx + (size_t)n * N * b, *cu = a.cu + (size_t)m * N * b;
    const double *ug = a.has_lims ? a.u + (size_t)m * N * b : nullptr;
    const double *fx = a.fx + a.fx_b * b, *fu = a.fu + a.fu_b * b;
    const double *cxx = a.cxx + a.cxx_b * b, *cxu = a.cxu + a.cxu_b * b, *cuu = a.cuu + a.cuu_b * b;
    double *Kg = a.K + nm * N * b, *kg = a.k + (size_t)m * N * b, *Quug = a.Quu + mm * N * b, *Vxg = a.Vx + (size_t)n * N * b,
           *Vxxg = a.Vxx + nn * N * b;
    const double lam = GPS ? 0.0 : a.lambda[b];
    const int regType = GPS ? 0 : a.regType;
    const double *cxkl = GPS ? a.cxkl + (size_t)n * N * b : nullptr, *cukl = GPS ? a.cukl + (size_t)m * N * b : nullptr,
                 *cxxkl = GPS ? a.cxxkl + nn * N * b : nullptr, *cxukl = GPS ? a.cxukl + nm * N * b : nullptr,
                 *cuukl = GPS ? a.cuukl + mm * N * b : nullptr, *etag = GPS ? a.eta + (a.eta_tv ? (size_t)N * b : b) : nullptr;
    double *Quuig = GPS ? a.Quui + mm * N * b : nullptr;
    double *img = lds + L.inv;                  // GPS: [Quu | inv(Quu) | pivot column]
    const bool nolims = !a.has_lims || a.lims[0] > a.lims[m];           // backward_pass.jl:31, read on the device
    const unsigned full = m >= 32 ? 0xffffffffu : ((1u << m) - 1u);
    double limlo = 0.0, limhi = 0.0;
    if (!nolims && lane < m) { limlo = a.lims[lane]; limhi = a.lims[lane + m]; }

    auto load_F = [&](int i, int first, int stride) {                   // [fx fu] of step i -> Fs
        const double *fxi = fx + a.fx_t * i, *fui = fu + a.fu_t * i;
        for (int e = first; e < n * p; e += stride) {
            const int l = e % n, c = e / n;
            Fs[l + ldn * c] = c < n ? fxi[e] : fui[e - n * n];
        }
    };

    // ---- terminal step (backward_pass.jl:234-236 / :197-199)
    {
        const double *cxxN = cxx + a.cxx_t * (N - 1), *cuuN = cuu + a.cuu_t * (N - 1);
        for (int e = t; e < n * n; e += WT) {
            const double v = cxxN[e];
            Vs[(e % n) + ldn * (e / n)] = v;
            Vxxg[nn * (N - 1) + e] = v;
        }
        for (int e = t; e < n; e += WT) {
            const double v = cx[(size_t)n * (N - 1) + e];
            vs[e] = v;
            Vxg[(size_t)n * (N - 1) + e] = v;
        }
        for (int e = t; e < m * m; e += WT) {
            double v = cuuN[e];
            if (GPS) { v = v / etag[a.eta_tv ? N - 1 : 0] + cuukl[mm * (N - 1) + e]; img[(e % m) + ldm * (e / m)] = v; }   // :282
            Quug[mm * (N - 1) + e] = v;
        }
        if (GPS) {                                                      // Quui[:,:,N] = inv(Quu[:,:,N])  (:283)
            __syncthreads();
            if (w == 0) inv_wave(img, ldm, m, lane);
            __syncthreads();
            for (int e = t; e < m * m; e += WT) Quuig[mm * (N - 1) + e] = img[(e % m) + ldm * (m + e / m)];
        }
        for (int e = t; e < m * n; e += WT) Kg[nm * (N - 1) + e] = 0.0;
        for (int e = t; e < m; e += WT) { kg[(size_t)m * (N - 1) + e] = 0.0; ks[e] = 0.0; }
    }
    double dV0 = 0.0, dV1 = 0.0;
    if (N < 2) {
        if (t == 0) { a.dV[2 * b] = 0.0; a.dV[2 * b + 1] = 0.0; a.diverge[b] = 0; }
        return;
    }
    load_F(N - 2, t, WT);
    __syncthreads();

    int diverge = 0;
    for (int i = N - 2; i >= 0; --i) {
        // ================= P0 (Curv::on): H_i from Vx_{i+1} (vs: written before the barrier that ended the last step) ===
        if constexpr (Curv::on) curv.p0(i, vs, t);
        // ================= P1: Gt = ([fx fu]'Vxx)', Qs = [cx; cu] + [fx fu]'Vx =====================
        for (int tt = w; tt < PT * NT; tt += NWAVE) {
            const int r0 = 16 * (tt / NT), c0 = 16 * (tt % NT);
            const d4 acc = xty(Fs, 1, ldn, r0, p, Vs, 1, ldn, c0, n, n, d4{0.0, 0.0, 0.0, 0.0}, l15, l4);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = r0 + l4 + 4 * r, col = c0 + l15;
                if (row < p && col < n) Gt[col + ldn * row] = comp(acc, r);
            }
        }
        if (t < p) {
            const double *fc = Fs + ldn * t;
            double s = 0.0;
            for (int l = 0; l < n; ++l) s += fc[l] * vs[l];
            double qv = (t < n ? cx[(size_t)n * i + t] : cu[(size_t)m * i + (t - n)]) + s;     // :240-241
            if (GPS) qv = qv / etag[a.eta_tv ? i : 0] + (t < n ? cxkl[(size_t)n * i + t] : cukl[(size_t)m * i + (t - n)]);   // :295,298
            Qs[t] = qv;
        }
        __syncthreads();

        // ================= P2: Qxx (accumulators), Qux, Quu and the regularised variants ===========
        d4 qacc[QS];
        {
            const double *cxxi = cxx + a.cxx_t * i;
#pragma unroll
            for (int s = 0; s < QS; ++s) {
                const int tt = w + NWAVE * s;
                qacc[s] = d4{0.0, 0.0, 0.0, 0.0};
                if (tt < NT * NT) {
                    const int r0 = 16 * (tt / NT), c0 = 16 * (tt % NT), col = c0 + l15;
                    d4 sd;
                    sd.x = (r0 + l4 < n && col < n) ? cxxi[(r0 + l4) + n * col] : 0.0;
                    sd.y = (r0 + l4 + 4 < n && col < n) ? cxxi[(r0 + l4 + 4) + n * col] : 0.0;
                    sd.z = (r0 + l4 + 8 < n && col < n) ? cxxi[(r0 + l4 + 8) + n * col] : 0.0;
                    sd.w = (r0 + l4 + 12 < n && col < n) ? cxxi[(r0 + l4 + 12) + n * col] : 0.0;
                    if constexpr (Curv::on) {                           // + Hxx (:106), symmetric entry by entry
                        if (r0 + l4 < n && col < n) sd.x += curv.h(r0 + l4, col);
                        if (r0 + l4 + 4 < n && col < n) sd.y += curv.h(r0 + l4 + 4, col);
                        if (r0 + l4 + 8 < n && col < n) sd.z += curv.h(r0 + l4 + 8, col);
                        if (r0 + l4 + 12 < n && col < n) sd.w += curv.h(r0 + l4 + 12, col);
                    }
                    qacc[s] = xty(Gt, 1, ldn, r0, n, Fs, 1, ldn, c0, n, n, sd, l15, l4);       // :244
                    if (GPS) {                                          // :299; only the symmetric part of cxxkl survives :341
                        const double et = etag[a.eta_tv ? i : 0];
                        const double *kx = cxxkl + nn * i;
                        d4 kd = d4{0.0, 0.0, 0.0, 0.0};
                        if (col < n) {
                            if (r0 + l4 < n) kd.x = 0.5 * (kx[(r0 + l4) + n * col] + kx[col + n * (r0 + l4)]);
                            if (r0 + l4 + 4 < n) kd.y = 0.5 * (kx[(r0 + l4 + 4) + n * col] + kx[col + n * (r0 + l4 + 4)]);
                            if (r0 + l4 + 8 < n) kd.z = 0.5 * (kx[(r0 + l4 + 8) + n * col] + kx[col + n * (r0 + l4 + 8)]);
                            if (r0 + l4 + 12 < n) kd.w = 0.5 * (kx[(r0 + l4 + 12) + n * col] + kx[col + n * (r0 + l4 + 12)]);
                        }
                        qacc[s] = qacc[s] / et + kd;
                    }
                }
            }
            const double *cxui = cxu + a.cxu_t * i, *cuui = cuu + a.cuu_t * i;
            const double *Gu = Gt + ldn * n;                            // rows n .. n+m-1 of G: fu'Vxx
#pragma unroll
            for (int s = 0; s < US; ++s) {
                const int tt = w + NWAVE * s;
                if (tt < MT * (NT + MT)) {
                    const int r0 = 16 * (tt / (NT + MT)), tc = tt % (NT + MT), col15 = l15;
                    const bool xcols = tc < NT;
                    const int c0 = 16 * (xcols ? tc : tc - NT), nc = xcols ? n : m, col = c0 + col15;
                    const double *Y = xcols ? Fs : Fu;
                    d4 sd;
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int row = r0 + l4 + 4 * r;
                        double v = 0.0;
                        if (row < m && col < nc) v = xcols ? cxui[col + n * row] : cuui[row + m * col];
                        if constexpr (Curv::on) {                       // + Hux, Huu (:107-108): they reach the regularised variants too
                            if (row < m && col < nc) v += curv.h(n + row, xcols ? col : n + col);
                        }
                        if (r == 0) sd.x = v; else if (r == 1) sd.y = v; else if (r == 2) sd.z = v; else sd.w = v;
                    }
                    const d4 acc = xty(Gu, 1, ldn, r0, m, Y, 1, ldn, c0, nc, n, sd, l15, l4);  // :242-243
                    d4 reg = acc;
                    if (GPS) {                                          // Q• <- Q•/η + c•kl, no λ  (:296-297)
                        const double et = etag[a.eta_tv ? i : 0];
                        const double *kp = xcols ? cxukl + nm * i : cuukl + mm * i;     // both m rows: cxukl[q + m j], cuukl[q + m b]
                        d4 kd = d4{0.0, 0.0, 0.0, 0.0};
                        if (col < nc) {
                            if (r0 + l4 < m) kd.x = kp[(r0 + l4) + m * col];
                            if (r0 + l4 + 4 < m) kd.y = kp[(r0 + l4 + 4) + m * col];
                            if (r0 + l4 + 8 < m) kd.z = kp[(r0 + l4 + 8) + m * col];
                            if (r0 + l4 + 12 < m) kd.w = kp[(r0 + l4 + 12) + m * col];
                        }
                        reg = acc / et + kd;
                    } else if (regType == 2) {                                 // Vxx_reg = Vxx + λI (:245): + λ fu'[fx fu]
                        const d4 sr = xty(Fu, 1, ldn, r0, m, Y, 1, ldn, c0, nc, n, d4{0.0, 0.0, 0.0, 0.0}, l15, l4);
                        reg = acc + lam * sr;
                    }
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int row = r0 + l4 + 4 * r;
                        if (row < m && col < nc) {
                            if (xcols) {                                // Qux, Qux_reg (:242,246)
                                Quxs[row + ldm * col] = comp(GPS ? reg : acc, r);
                                Kx[row + ldm * col] = comp(reg, r);
                            } else {                                    // Quu, QuuF (:243,247)
                                Quus[row + ldm * col] = comp(GPS ? reg : acc, r);
                                Hs[row + ldm * col] = comp(reg, r) + ((regType == 1 && row == col) ? lam : 0.0);
                            }
                        }
                    }
                }
            }
        }
        __syncthreads();
        if (GPS) {                                                      // Quu = .5(Quu + Quu')  (:301); it is also the matrix factorised
            constexpr int RQ = cdivw(SM * SM, WT);
            double sv[RQ];
#pragma unroll
            for (int r = 0; r < RQ; ++r) {
                const int e = t + WT * r, ii = e % m, jj = e / m;
                sv[r] = e < m * m ? 0.5 * (Quus[ii + ldm * jj] + Quus[jj + ldm * ii]) : 0.0;
            }
            __syncthreads();
#pragma unroll
            for (int r = 0; r < RQ; ++r) {
                const int e = t + WT * r, ii = e % m, jj = e / m;
                if (e < m * m) { Quus[ii + ldm * jj] = sv[r]; Hs[ii + ldm * jj] = sv[r]; img[ii + ldm * jj] = sv[r]; }
            }
            __syncthreads();
        }

        // ================= P3: gains (backward_pass.jl:30-62) =======================================
        if (w == 0) {
            int fail;
            unsigned freem = full;
            if (nolims) {
                fail = chol_wave(Hs, Rs, ldm, m, full, lane);           // cholesky(Hermitian(QuuF)), :35
            } else {
                const double uq = lane < m ? ug[(size_t)m * i + lane] : 0.0;
                double xq;
                const int result = boxqp_wave(Hs, Rs, ldm, m, lane < m ? Qs[n + lane] : 0.0, limlo - uq, limhi - uq,   // :45-49
                                              lane < m ? ks[lane] : 0.0, xb, sb, lane, xq, freem);
                fail = result < 1;                                      // :53
                wave_sync();
                if (lane < m) ks[lane] = xq;
            }
            if (lane == 0) { flags[0] = fail; flags[1] = (int)freem; }
        } else if (GPS && w == 1) {
            inv_wave(img, ldm, m, lane);                                // Quui[:,:,i] = inv(Quu[:,:,i])  (:346), off the chain
        } else if (a.fx_t != 0 && i > 0) {
            if (GPS) load_F(i - 1, t - 2 * WIDE_WAVE, WT - 2 * WIDE_WAVE);
            else load_F(i - 1, t - WIDE_WAVE, WT - WIDE_WAVE);            // (Fs: last read in P2)
        }
        __syncthreads();
        if (flags[0]) {                                                 // uniform: diverge = i (:37-38, :54-55)
            diverge = i + 1;
            // Quu[:,:,i] was already assigned by the reference before the failure
            for (int e = t; e < m * m; e += WT) Quug[mm * i + e] = Quus[(e % m) + ldm * (e / m)];
            for (size_t e = t; e < nm * (i + 1); e += WT) Kg[e] = 0.0;
            for (size_t e = t; e < (size_t)m * (i + 1); e += WT) kg[e] = 0.0;
            for (size_t e = t; e < (size_t)n * (i + 1); e += WT) Vxg[e] = 0.0;
            for (size_t e = t; e < nn * (i + 1); e += WT) Vxxg[e] = 0.0;
            for (size_t e = t; e < mm * i; e += WT) Quug[e] = 0.0;
            break;
        }
        {
            const unsigned freem = (unsigned)flags[1];
            if (t < n) solve_col(Kx + ldm * t, Rs, ldm, m, freem);      // K_i column t (:42 / :59)
            else if (t == n && nolims) {                                // k_i = -(R \ Qu) (:41)
                for (int q = 0; q < m; ++q) ks[q] = Qs[n + q];
                solve_col(ks, Rs, ldm, m, full);
            }
        }
        __syncthreads();

        // ================= P4: T, stores of K, k, Quu; value update (:64-76) ========================
#pragma unroll
        for (int s = 0; s < TS; ++s) {
            const int tt = w + NWAVE * s;
            if (tt < MT * NT) {
                const int r0 = 16 * (tt / NT), c0 = 16 * (tt % NT), col = c0 + l15;
                d4 sd;
                sd.x = (r0 + l4 < m && col < n) ? Quxs[(r0 + l4) + ldm * col] : 0.0;
                sd.y = (r0 + l4 + 4 < m && col < n) ? Quxs[(r0 + l4 + 4) + ldm * col] : 0.0;
                sd.z = (r0 + l4 + 8 < m && col < n) ? Quxs[(r0 + l4 + 8) + ldm * col] : 0.0;
                sd.w = (r0 + l4 + 12 < m && col < n) ? Quxs[(r0 + l4 + 12) + ldm * col] : 0.0;
                const d4 acc = xty(Quus, ldm, 1, r0, m, Kx, 1, ldm, c0, n, m, sd, l15, l4);      // T = Quu K + Qux
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int row = r0 + l4 + 4 * r;
                    if (row < m && col < n) Ts[row + ldm * col] = comp(acc, r);
                }
            }
        }
        if (t < m) {                                                    // Quu k (:66-68)
            double s = 0.0;
            for (int q = 0; q < m; ++q) s += Quus[t + ldm * q] * ks[q];
            Quuks[t] = s;
            kg[(size_t)m * i + t] = ks[t];                              // :75
        }
        for (int e = t; e < m * n; e += WT) Kg[nm * i + e] = Kx[(e % m) + ldm * (e / m)];       // :76
        for (int e = t; e < m * m; e += WT) Quug[mm * i + e] = Quus[(e % m) + ldm * (e / m)];
        if (GPS)
            for (int e = t; e < m * m; e += WT) Quuig[mm * i + e] = img[(e % m) + ldm * (m + e / m)];
        __syncthreads();

#pragma unroll
        for (int s = 0; s < QS; ++s) {                                  // M = Qxx + K'T + Qux'K (:67,70)
            const int tt = w + NWAVE * s;
            if (tt < NT * NT) {
                const int r0 = 16 * (tt / NT), c0 = 16 * (tt % NT);
                qacc[s] = xty(Kx, 1, ldm, r0, n, Ts, 1, ldm, c0, n, m, qacc[s], l15, l4);
                qacc[s] = xty(Quxs, 1, ldm, r0, n, Kx, 1, ldm, c0, n, m, qacc[s], l15, l4);
            }
        }
        if (t < n) {                                                    // Vx_i (:69)
            double s1 = 0.0, s2 = 0.0, s3 = 0.0;
            for (int q = 0; q < m; ++q) {
                const double Kq = Kx[q + ldm * t];
                s1 += Kq * Quuks[q];
                s2 += Kq * Qs[n + q];
                s3 += Quxs[q + ldm * t] * ks[q];
            }
            const double v = ((Qs[t] + s1) + s2) + s3;
            vs[t] = v;                                                  // (vs: read in P1 only)
            Vxg[(size_t)n * i + t] = v;
        } else if (t == WT - 1) {                                       // dV (:68)
            double kQu = 0.0, kQuuk = 0.0;
            for (int q = 0; q < m; ++q) { kQuuk += ks[q] * Quuks[q]; kQu += ks[q] * Qs[n + q]; }
            dV0 += kQu;
            dV1 += 0.5 * kQuuk;
        }
        __syncthreads();                                                // K and QuuF are dead: the V region takes M
#pragma unroll
        for (int s = 0; s < QS; ++s) {
            const int tt = w + NWAVE * s;
            if (tt < NT * NT) {
                const int r0 = 16 * (tt / NT), c0 = 16 * (tt % NT), col = c0 + l15;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int row = r0 + l4 + 4 * r;
                    if (row < n && col < n) Vs[row + ldn * col] = comp(qacc[s], r);
                }
            }
        }
        __syncthreads();
        double vr[RV];
#pragma unroll
        for (int r = 0; r < RV; ++r) {                                  // Vxx_i = ½(M + M') (:71-72)
            const int e = t + WT * r;
            vr[r] = 0.0;
            if (e < n * n) {
                const int ii = e % n, jj = e / n;
                vr[r] = (Vs[ii + ldn * jj] + Vs[jj + ldn * ii]) / 2;
            }
        }
        __syncthreads();
#pragma unroll
        for (int r = 0; r < RV; ++r) {
            const int e = t + WT * r;
            if (e < n * n) {
                Vs[(e % n) + ldn * (e / n)] = vr[r];
                Vxxg[nn * i + e] = vr[r];
            }
        }
        __syncthreads();
    }
    if (t == WT - 1) { a.dV[2 * b] = dV0; a.dV[2 * b + 1] = dV1; }
    if (t == 0) a.diverge[b] = diverge;
}

#ifndef __HIPCC_RTC__
// the arguments of one call (the element strides from the descriptor); the GPS members are left null
inline void bpw_fill(BPWArgs &a, const BPCall &c)
{
    const ddp_bp_desc *d = &c.d;
    const long n = d->n, m = d->m, N = d->N;
    a.n = d->n; a.m = d->m; a.N = d->N; a.B = d->B; a.regType = d->regType; a.has_lims = d->has_lims;
    a.fx_t = d->fx_tv ? n * n : 0; a.fx_b = d->fx_batched ? n * n * (d->fx_tv ? N : 1) : 0;
    a.fu_t = d->fx_tv ? n * m : 0; a.fu_b = d->fx_batched ? n * m * (d->fx_tv ? N : 1) : 0;
    a.cxx_t = d->cost_tv ? n * n : 0; a.cxx_b = d->cost_batched ? n * n * (d->cost_tv ? N : 1) : 0;
    a.cxu_t = d->cost_tv ? n * m : 0; a.cxu_b = d->cost_batched ? n * m * (d->cost_tv ? N : 1) : 0;
    a.cuu_t = d->cost_tv ? m * m : 0; a.cuu_b = d->cost_batched ? m * m * (d->cost_tv ? N : 1) : 0;
    a.cx = c.cx; a.cu = c.cu; a.cxx = c.cxx; a.cxu = c.cxu; a.cuu = c.cuu; a.fx = c.fx; a.fu = c.fu; a.lambda = c.lambda;
    a.lims = c.lims; a.u = c.u; a.active = c.active;
    a.K = c.K; a.k = c.k; a.Quu = c.Quu; a.Vx = c.Vx; a.Vxx = c.Vxx; a.dV = c.dV; a.diverge = c.diverge;
    a.cxkl = a.cukl = a.cxxkl = a.cxukl = a.cuukl = a.eta = nullptr; a.eta_tv = 0; a.Quui = nullptr;
}
#endif

}   // namespace
