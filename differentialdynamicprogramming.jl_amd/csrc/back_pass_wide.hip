// back_pass_wide.hip — backward pass for WIDE CONTROLS: any 1 <= n <= 64 with 1 <= m <= 32 at run time (src/backward_pass.jl:162-252 +
// @end_backward_pass :28-79).  The dispatcher sends 8 < m <= 32 here (back_pass.hip, BP_WIDE); DDP_BACKPASS=c forces it for m <= 8.
//
// Mapping: ONE work-group of four waves per trajectory.  The time loop is a dependency chain (Vxx_{i+1} -> Vxx_i), so a step is a
// sequence of phases separated by work-group barriers; inside a phase the 16 x 16 tiles of a product are dealt to the four waves.
// Every matrix of a step lives in the LDS, column-major with a leading dimension = 2 (mod 4) doubles, so that the 16 x 4 operand
// fragment of v_mfma_f64_16x16x4 (lane l: row l & 15, k = l >> 4) falls on 32 distinct bank pairs per half wave.  Per step i:
//   P1  G = [fx fu]'Vxx_{i+1}  (stored transposed: Gt[l, r] = G[r, l])                 MFMA, (n+m) x n, k = n        (:165/:203/:240)
//       Qs = [cx; cu] + [fx fu]'Vx_{i+1}                                              one thread per entry
//   P2  Qxx = cxx + G_x fx  -> accumulators, they stay in registers until P4             MFMA, n x n, k = n
//       Qux = cxu' + G_u fx, Quu = cuu + G_u fu (+ regularised variants)              MFMA, m x (n+m), k = n
//       regType 2 adds λ fu'[fx fu] (a third product); regType 1 adds λ I to QuuF
//   P3  wave 0: Cholesky of QuuF across lanes, one column per lane (no limits, or lims[1,1] > lims[1,2] — decided on the device), or
//       the projected-Newton box-QP of boxQP.jl:46-169 with one coordinate per lane and wave-uniform control flow; the other waves
//       fetch the next step's fx, fu meanwhile.  Then the n + 1 right-hand sides [Qux_reg | Qu] one per thread (clamped rows: zero).
//   P4  T = Quu K + Qux (MFMA, m x n, k = m); Vxx_i = ½(M + M'), M = Qxx + K'T + Qux'K (MFMA, n x n, k = 2m, on the accumulators of
//       P2); Vx_i, dV; stores of K, k, Quu, Vx, Vxx.
// The LDS regions are reused across the phases (WLds below): at (64, 32) a private buffer for every matrix would need about 250 KB;
// the plan below needs 160 KB.  The cost Hessians are never staged: a tile's accumulator starts from its cxx / cxu / cuu entries,
// read from the user's arrays.  Operands and results are the caller's arrays, nothing is padded or copied, nothing lives on the handle.
// The step itself — the LDS plan, the wave-level pieces of P3 and the kernel body — is in back_pass_wide_kernel.h, which the runtime-compiled
// ddp_user_back_pass2_wave of user_problem.hip shares (DDP_USER_SECOND_ORDER_WAVE); this file has the two precompiled kernels and their launch.
#include <stdlib.h>
#include "back_pass_wide_kernel.h"

namespace {

static_assert(WIDE_WAVE == DDP_WAVE, "the wide kernel's wave size");

template <bool GPS>
__global__ __launch_bounds__(WT) void back_pass_wide_kernel(BPWArgs a)
{
    extern __shared__ double lds[];
    back_pass_wide_body<GPS, 0, 0>(a, lds, WNoCurv());
}

}   // namespace

static int launch_wide(ddp_handle h, const BPCall &c, bool gps)
{
    const ddp_bp_desc *d = &c.d;
    const char *who = gps ? "back_pass_gps" : "back_pass";
    DDP_CHECK(d->n >= 1 && d->n <= WIDE_MAX_N && d->m >= 1 && d->m <= WIDE_MAX_M, "%s: n=%d m=%d outside the wide-control kernel (n <= %d, m <= %d)",
              who, d->n, d->m, WIDE_MAX_N, WIDE_MAX_M);
    BPWArgs a;
    bpw_fill(a, c);
    if (gps) {
        const ddp_kl_cost_terms *kl = c.kl;
        DDP_CHECK(kl && kl->cx && kl->cu && kl->cxx && kl->cxu && kl->cuu && kl->eta && c.Quui, "back_pass_gps: null KL terms / Quui");
        DDP_CHECK(!d->has_lims || (c.lims && c.u), "back_pass_gps: has_lims without lims / u");
        a.cxkl = kl->cx; a.cukl = kl->cu; a.cxxkl = kl->cxx; a.cxukl = kl->cxu; a.cuukl = kl->cuu; a.eta = kl->eta; a.eta_tv = kl->eta_tv;
        a.Quui = c.Quui;
        a.regType = 0;
    }
    const WLds L(d->n, d->m, gps);
    const size_t bytes = (size_t)L.total * sizeof(double);
    DDP_CHECK(bytes <= (size_t)WIDE_LDS_BYTES, "%s: n=%d m=%d needs %zu bytes of LDS (limit %d)", who, d->n, d->m, bytes, WIDE_LDS_BYTES);
    const void *kern = gps ? (const void *)back_pass_wide_kernel<true> : (const void *)back_pass_wide_kernel<false>;
    if (int rc = ddp_raise_lds(h, kern, WIDE_LDS_BYTES)) return rc;    // per handle, not per process
    if (gps) hipLaunchKernelGGL(back_pass_wide_kernel<true>, dim3(d->B), dim3(WT), bytes, h->stream, a);
    else hipLaunchKernelGGL(back_pass_wide_kernel<false>, dim3(d->B), dim3(WT), bytes, h->stream, a);
    DDP_HIP(hipGetLastError());
    return 0;
}

// any n <= 64, m <= 32 (the dispatcher has checked the shape)
int ddp_launch_back_pass_wide(ddp_handle h, const BPCall &c) { return launch_wide(h, c, false); }
// back_pass_gps on the same kernel (the GPS instantiation)
int ddp_launch_back_pass_gps_wide(ddp_handle h, const BPCall &c) { return launch_wide(h, c, true); }
