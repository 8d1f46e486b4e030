// user_problem_wave_kernels.h — DDP_USER_WAVE: the kernel templates of a large user problem (n <= 64, m <= 32), as program text for hiprtc.
//
// A problem with the flag compiles, in place of the rollout and derivative kernels of user_problem_kernels.h (kUserKernelsLane) and of
// its ddp_user_hessians: the macros (+ DDP_WAVE 1, DDP_WG), the user's source, DDP_USER_ABI, kUserKernelsHead, kUserWaveKernels,
// kUserKernelsCost, kUserKernelsPlant.  The argument structs are the same.  A problem without the flag does not contain this text.
// The lane-per-rollout kernels keep x̂[n], dx[n], û[m] in registers, a chunk of K in LDS (2m + mn + n doubles per step and rollout) and
// an LDS slot of every derivative per lane: at (64, 32) that is 17 KB per rollout step and 107 KB per (step, trajectory).  Here no lane
// holds an array of n or m·n doubles of the library's own (what the user's functions keep is theirs):
//
//   ddp_user_rollout_wave  a group of DDP_WG lanes (8, 16 or 32: the power of two >= m) per (trajectory, α) rollout, 64 / DDP_WG rollouts
//                          per one-wave work-group.  x̂, diff(x̂, x), û and the successor state live in LDS (3n + m doubles per rollout).
//                          K is never staged: lane q of the group streams row q of K_i from memory (K_i is m x n column-major, so the
//                          group's lanes read m consecutive doubles per column) against dx in LDS.  One lane of the group calls the
//                          user's stage_cost and dynamics on the LDS vectors; x̂ and û leave as contiguous runs written by the group.
//                          Semantics and the order of every sum are those of ddp_user_rollout (forward_pass.jl:9-33).
//   ddp_user_df_wave       DDP_USER_AUTODIFF: one wave per (step, trajectory), one seed direction of z = [x; u] per lane
//                          (ddp_dual<double, 1>, the seed a run-time compare as in ddp_ad_vhess: `dynamics` is instantiated once),
//                          ceil((n + m) / 64) rounds.  The Jacobian columns of a round go through LDS and leave as contiguous runs of
//                          fx and fu; cx, cu come from the same pass of stage_cost (+ terminal_cost at i == N-1).  Without
//                          DDP_USER_CONST_HESSIAN the (n + m)(n + m + 1) / 2 pairs a <= b are dealt over the lanes, each pair one call of
//                          stage_cost on a dual over a dual with one partial each, written to (a, b) and (b, a) of the LDS image (cxx and
//                          cuu exactly symmetric); the image leaves in two pieces (cxx; cxu and cuu).  With DDP_USER_CONST_HESSIAN only
//                          the first-order rounds run: the fast path for quadratic costs.
//   ddp_user_df            hand-written `derivatives` under the flag: one lane per (step, trajectory), 64 per work-group, the user's
//                          function writing straight into the output arrays in memory (8-byte stores at a stride of the array's slice:
//                          slower than ddp_user_df_wave at large shapes — prefer DDP_USER_AUTODIFF there).  Hessians that are discarded
//                          (DDP_USER_CONST_HESSIAN, or NULL outputs) go to one LDS dump area of the work-group, never to a private array.
//   ddp_user_hessians      DDP_USER_CONST_HESSIAN: cost_hessians writes straight into cxx, cxu, cuu in memory.
#pragma once

static const char *kUserWaveKernels = R"DDPW(
#define DDP_WRS ((3 * DDP_N + DDP_M) | 1)                      // doubles per rollout in LDS: x̂, dx, x̂⁺, û (odd stride)

extern "C" __global__ __launch_bounds__(64) void ddp_user_rollout_wave(UserRollArgs a)
{
    constexpr int n = DDP_N, m = DDP_M, G = DDP_WG, RPW = 64 / G;
    static_assert(G >= m && G <= 64 && (G & (G - 1)) == 0, "ddp_user_rollout_wave: DDP_WG is a power of two >= m");
    __shared__ double lds[RPW * DDP_WRS];
    const int lane = threadIdx.x, g = lane / G, q = lane - g * G, N = a.N, B = a.B, CL = DDP_TERMINAL ? N + 1 : N;
    const long total = (long)B * a.nalpha, rho = (long)blockIdx.x * RPW + g;
    const bool mine = rho < total;
    const int b = mine ? (int)(rho % B) : 0, ai = mine ? (int)(rho / B) : 0;
    const bool act = mine && !(a.active && a.active[b] == 0);
    const bool lead = act && q == 0, ctl = act && q < m;
    const double alpha = a.alpha[ai];
    const double *p = ddp_params(a.params, a.params_batched, a.map, b);
    double *xh = lds + g * DDP_WRS, *dx = xh + n, *xn = dx + n, *uu = xn + n;
    const double lo = (a.has_lims && q < m) ? a.lims[q] : 0.0, hi = (a.has_lims && q < m) ? a.lims[q + m] : 0.0;
    const double *ub = a.u + (size_t)m * N * b, *xb = a.x + (size_t)n * N * b, *kb = a.k + (size_t)m * N * b,
                 *Kb = a.K + (size_t)m * n * N * b;
    double *xo = a.xnew + (size_t)n * N * rho, *uo = a.unew + (size_t)m * N * rho, *co = a.cnew + (size_t)CL * rho;
    if (act)
        for (int l = q; l < n; l += G) xh[l] = a.x0[(size_t)n * b + l];
    double csum = 0.0;
    ddp_wave_sync();
    for (int i = 0; i < N; ++i) {
        if (act) {
            for (int l = q; l < n; l += G) {
                const double xv = xh[l];
                xo[(size_t)n * i + l] = xv;
                if (a.has_policy) {                            // forward_pass.jl:17-20: unew += k α;  unew += K diff(x̂, x)
                    double d = xv - xb[(size_t)n * i + l];
                    if (l < 32 && ((DDP_WRAP >> l) & 1u)) d = ddp_wrap_pi(d);
                    dx[l] = d;
                }
            }
        }
        ddp_wave_sync();
        if (ctl) {
            double v = ub[(size_t)m * i + q];
            if (a.has_policy) {
                const double *Kr = Kb + (size_t)m * n * i + q;   // row q of K_i
                double s2 = 0.0;
                v += kb[(size_t)m * i + q] * alpha;
#pragma unroll 8
                for (int l = 0; l < n; ++l) s2 += Kr[m * l] * dx[l];
                v += s2;
            }
            if (a.has_lims) v = v > hi ? hi : (v < lo ? lo : v);   // :22-24
            uu[q] = v;
            uo[(size_t)m * i + q] = v;
        }
        ddp_wave_sync();
        if (lead) {
            const double c = stage_cost(xh, uu, i, p);
            csum += c;
            co[i] = c;
            if (i < N - 1) dynamics(xh, uu, i, p, xn);         // :25-28 (the successor of the last step is not stored)
        }
        ddp_wave_sync();
        if (act && i < N - 1)
            for (int l = q; l < n; l += G) xh[l] = xn[l];
        ddp_wave_sync();
    }
    if (lead) {
#if DDP_TERMINAL
        const double c = terminal_cost(xh, p);
        co[N] = c;
        csum += c;
#endif
        a.csum[rho] = csum;
    }
}

#if DDP_AUTODIFF
// pair e of the upper triangle stored by columns: e = hi (hi + 1) / 2 + lo, lo <= hi
__device__ __forceinline__ void ddp_wave_tri(int e, int &lo, int &hi)
{
    int c = (int)((sqrtf(8.0f * (float)e + 1.0f) - 1.0f) * 0.5f);
    while (c * (c + 1) / 2 > e) --c;
    while ((c + 1) * (c + 2) / 2 <= e) ++c;
    hi = c;
    lo = e - c * (c + 1) / 2;
}

// elements [0, len) of an LDS image to memory, by the whole wave
__device__ __forceinline__ void ddp_wave_store(const double *img, double *dst, int len, int lane)
{
    for (int e = lane; e < len; e += 64) dst[e] = img[e];
}

extern "C" __global__ __launch_bounds__(64) void ddp_user_df_wave(UserDfArgs a)
{
    constexpr int n = DDP_N, m = DDP_M, nz = n + m, nn = n * n, nm = n * m, mm = m * m;
    constexpr int JC = nz < 64 ? nz : 64;                      // Jacobian columns per round
    constexpr int NPX = n * (n + 1) / 2, NP = nz * (nz + 1) / 2;   // pairs with hi < n (cxx) come first
    constexpr int I1 = n * JC, I2 = DDP_CONST_HESSIAN ? 0 : (nn > nm + mm ? nn : nm + mm), IMG = I1 > I2 ? I1 : I2;
    static_assert((IMG + nz) * 8 <= 64 * 1024, "ddp_user_df_wave: the image does not fit 64 KB of LDS");
    __shared__ double img[IMG];
    __shared__ double zs[nz];                                   // z = [x; u] of the step
    const int lane = threadIdx.x, N = a.N;
    const long r = blockIdx.x;                                  // (step, trajectory)
    const int b = (int)(r / N), i = (int)(r - (long)b * N);
    if (b >= a.B || (a.active && a.active[b] == 0)) return;     // wave-uniform
    const double *p = ddp_params(a.params, a.params_batched, a.map, b);
    for (int k = lane; k < nz; k += 64) zs[k] = k < n ? a.x[(size_t)n * r + k] : a.u[(size_t)m * r + (k - n)];
    ddp_wave_sync();
    double *fx = a.fx + (size_t)nn * r, *fu = a.fu + (size_t)nm * r;

    // ---- first order: lane z0 + lane carries the seed of its direction; a lane past nz seeds nothing and stores nothing
    for (int z0 = 0; z0 < nz; z0 += 64) {
        typedef ddp_dual<double, 1> D;
        const int z = z0 + lane;
        {
            D xd[n], ud[m], xnx[n];
#pragma unroll
            for (int k = 0; k < nz; ++k) {
                D &t = k < n ? xd[k] : ud[k - n];
                t.v = zs[k];
                t.d[0] = k == z ? 1.0 : 0.0;
            }
            DDP_AD_FRESH(p);
            dynamics(xd, ud, i, p, xnx);
            if (z < nz) {
#pragma unroll
                for (int rr = 0; rr < n; ++rr) img[rr + n * lane] = xnx[rr].d[0];
            }
        }
        {
            D xd[n], ud[m];
#pragma unroll
            for (int k = 0; k < nz; ++k) {
                D &t = k < n ? xd[k] : ud[k - n];
                t.v = zs[k];
                t.d[0] = k == z ? 1.0 : 0.0;
            }
            DDP_AD_FRESH(p);
            D c = stage_cost(xd, ud, i, p);
#if DDP_TERMINAL
            if (i == N - 1) c += terminal_cost(xd, p);         // the terminal cost acts on x[:,N-1] (the header's convention)
#endif
            if (z < n) a.cx[(size_t)n * r + z] = c.d[0];
            else if (z < nz) a.cu[(size_t)m * r + (z - n)] = c.d[0];
        }
        ddp_wave_sync();
        // columns [z0, z0 + nc) of [fx fu]: column-major, so both parts are contiguous runs
        const int nc = nz - z0 < 64 ? nz - z0 : 64;
        for (int e = lane; e < n * nc; e += 64) {
            const int ge = n * z0 + e;                          // element of [fx fu]
            if (ge < nn) fx[ge] = img[e];
            else fu[ge - nn] = img[e];
        }
        ddp_wave_sync();
    }

#if !DDP_CONST_HESSIAN
    // ---- second order: piece 0 = the pairs of cxx, piece 1 = the pairs of cxu and cuu
    typedef ddp_dual<ddp_dual<double, 1>, 1> D2;
    for (int piece = 0; piece < 2; ++piece) {
        if (piece == 0 ? !a.cxx : (!a.cxu && !a.cuu)) continue;  // wave-uniform: Hessians that are not asked for are not computed
        const int e0 = piece == 0 ? 0 : NPX, e1 = piece == 0 ? NPX : NP;
        for (int e = e0 + lane; e < e1; e += 64) {
            int pa, pb;
            ddp_wave_tri(e, pa, pb);
            D2 xd[n], ud[m];
#pragma unroll
            for (int k = 0; k < nz; ++k) {
                D2 &t = k < n ? xd[k] : ud[k - n];
                t.v.v = zs[k];
                t.v.d[0] = k == pa ? 1.0 : 0.0;
                t.d[0].v = k == pb ? 1.0 : 0.0;
                t.d[0].d[0] = 0.0;
            }
            DDP_AD_FRESH(p);
            D2 c = stage_cost(xd, ud, i, p);
#if DDP_TERMINAL
            if (piece == 0 && i == N - 1) c += terminal_cost(xd, p);
#endif
            const double hv = c.d[0].d[0];
            if (pb < n) {
                img[pa + n * pb] = hv;
                img[pb + n * pa] = hv;
            } else if (pa < n) {
                img[pa + n * (pb - n)] = hv;
            } else {
                img[nm + (pa - n) + m * (pb - n)] = hv;
                img[nm + (pb - n) + m * (pa - n)] = hv;
            }
        }
        ddp_wave_sync();
        if (piece == 0) {
            ddp_wave_store(img, a.cxx + (size_t)nn * r, nn, lane);
        } else {
            if (a.cxu) ddp_wave_store(img, a.cxu + (size_t)nm * r, nm, lane);
            if (a.cuu) ddp_wave_store(img + nm, a.cuu + (size_t)mm * r, mm, lane);
        }
        ddp_wave_sync();
    }
#endif
}
#else
extern "C" __global__ __launch_bounds__(64) void ddp_user_df(UserDfArgs a)
{
    constexpr int n = DDP_N, m = DDP_M, nn = n * n, nm = n * m, mm = m * m;
    constexpr int DUMP = nn > nm ? (nn > mm ? nn : mm) : (nm > mm ? nm : mm);
    __shared__ double dump[DUMP];                               // discarded Hessians of every lane: written, never read
    const int N = a.N;
    const long R = (long)N * a.B, r = (long)blockIdx.x * 64 + threadIdx.x;
    if (r >= R) return;
    const int b = (int)(r / N), i = (int)(r - (long)b * N);
    if (a.active && a.active[b] == 0) return;
    double x[n], u[m];
#pragma unroll
    for (int l = 0; l < n; ++l) x[l] = a.x[(size_t)n * r + l];
#pragma unroll
    for (int q = 0; q < m; ++q) u[q] = a.u[(size_t)m * r + q];
    const double *p = ddp_params(a.params, a.params_batched, a.map, b);
    double *oxx = (DDP_CONST_HESSIAN || !a.cxx) ? dump : a.cxx + (size_t)nn * r;
    double *oxu = (DDP_CONST_HESSIAN || !a.cxu) ? dump : a.cxu + (size_t)nm * r;
    double *ouu = (DDP_CONST_HESSIAN || !a.cuu) ? dump : a.cuu + (size_t)mm * r;
    derivatives(x, u, i, N, p, a.fx + (size_t)nn * r, a.fu + (size_t)nm * r, a.cx + (size_t)n * r, a.cu + (size_t)m * r, oxx, oxu, ouu);
}
#endif

#if DDP_CONST_HESSIAN
extern "C" __global__ __launch_bounds__(64) void ddp_user_hessians(UserHessArgs a)
{
    constexpr int n = DDP_N, m = DDP_M;
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b >= a.B || (a.active && a.active[b] == 0)) return;
    cost_hessians(ddp_params(a.params, a.params_batched, a.map, b), a.cxx + (size_t)n * n * b, a.cxu + (size_t)n * m * b,
                  a.cuu + (size_t)m * m * b);
}
#endif
)DDPW";
