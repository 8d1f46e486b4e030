// back_pass_mfma.hip — launcher of the n = 64, m = 8 matrix-core backward pass (kernel: back_pass_mfma_kernel.h)
#include "back_pass_mfma_kernel.h"

// n = 64, m = 8; `lims_active` as for back_pass_mf2
int ddp_launch_back_pass_mfma(ddp_handle h, const BPCall &c, bool lims_active)
{
    const ddp_bp_desc *d = &c.d;
    BPMArgs a;
    a.N = d->N; a.B = d->B;
    a.fx_tv = d->fx_tv; a.fx_batched = d->fx_batched; a.cost_tv = d->cost_tv; a.cost_batched = d->cost_batched;
    a.regType = d->regType; a.has_lims = d->has_lims;
    a.cx = c.cx; a.cu = c.cu; a.cxx = c.cxx; a.cxu = c.cxu; a.cuu = c.cuu; a.fx = c.fx; a.fu = c.fu; a.lambda = c.lambda; a.lims = c.lims;
    a.u = c.u; a.active = c.active;
    a.K = c.K; a.k = c.k; a.Quu = c.Quu; a.Vx = c.Vx; a.Vxx = c.Vxx; a.dV = c.dV; a.diverge = c.diverge;
    if (lims_active) return ddp_bpm_launch_lims(h, a);
    a.has_lims = 0; a.lims = nullptr;
    return ddp_bpm_launch<false>(h, a);
}
