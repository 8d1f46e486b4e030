// back_pass_mf2.hip — launcher of the large-state matrix-core backward pass, 32 < n <= 64, m <= 8 at run time (kernel: back_pass_mf2_kernel.h)
#include "back_pass_mf2_kernel.h"

// 32 < n <= 64, 1 <= m <= 8.  lims[1,1] > lims[1,2] means "no limits" upstream (backward_pass.jl:31: the Cholesky branch, not a box-QP
// with infinite bounds, whose projected-Newton iterations and extra exits would differ by rounding): `lims_active` is that test, made
// once by the caller
int ddp_launch_back_pass_mf2(ddp_handle h, const BPCall &c, bool lims_active)
{
    const ddp_bp_desc *d = &c.d;
    const int nt = (d->n + 15) / 16;                 // 3 or 4 tiles of 16 states
    BPM2Args a;
    a.n = d->n; a.m = d->m; a.N = d->N; a.B = d->B;
    a.fx_tv = d->fx_tv; a.fx_batched = d->fx_batched; a.cost_tv = d->cost_tv; a.cost_batched = d->cost_batched;
    a.regType = d->regType; a.has_lims = d->has_lims;
    a.cx = c.cx; a.cu = c.cu; a.cxx = c.cxx; a.cxu = c.cxu; a.cuu = c.cuu; a.fx = c.fx; a.fu = c.fu; a.lambda = c.lambda; a.lims = c.lims;
    a.u = c.u; a.active = c.active;
    a.K = c.K; a.k = c.k; a.Quu = c.Quu; a.Vx = c.Vx; a.Vxx = c.Vxx; a.dV = c.dV; a.diverge = c.diverge;
    a.sink = (double *)h->sink;
    DDP_CHECK(a.sink, "back_pass: the handle has no sink buffer");
    if (lims_active) return ddp_bpm2_launch_lims(h, a, nt);
    a.has_lims = 0; a.lims = nullptr;
    return nt == 4 ? mf2::launch<4, false>(h, a) : mf2::launch<3, false>(h, a);
}
