// back_pass_mfma.hip — launcher of the n = 64, m = 8 matrix-core backward pass (kernel: back_pass_mfma_kernel.h)
#include "back_pass_mfma_kernel.h"

// n = 64, m = 8; `lims_active` as for back_pass_mf2
int ddp_launch_back_pass_mfma(ddp_handle h, const BPCall &c, bool lims_active)
{
    BPKArgs a = bp_kargs(h, c);
    if (lims_active) return ddp_bpm_launch_lims(h, a);
    a.has_lims = 0; a.lims = nullptr;
    return ddp_bpm_launch<false>(h, a);
}
