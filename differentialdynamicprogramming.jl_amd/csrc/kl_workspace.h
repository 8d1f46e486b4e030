// kl_workspace.h — the workspace of the iLQGkl driver (kl.hip) in the handle's scratch, written once as a function of a Carver.
// Plain host code: tests/kl_workspace_check.cpp runs the layout without a device.
#pragma once
#include "carver.h"
#include "../../include/ddp_amd.h"

// What the layout depends on.  family: a ddp_family (derivatives per trajectory), else a registered problem; fx_own: the dynamics
// back_pass_gps reads are the driver's own copy (df writes them, or an LTI problem's are repeated along time), [n,n,N,B] with fx_batched;
// const_hessian (family only): one set of cost Hessians per trajectory, read as such by the mid and wide kernels or, with hrep,
// repeated along time for the others
struct KlWorkIn { size_t n, m, N, B; bool family, fx_own, fx_batched, const_hessian, hrep; };

// the derivatives of STEP 1 in the layouts of back_pass_gps: cost gradients [.,N,B]; Hessians [.,.,N] of a registered problem,
// [.,.,N,B] of a family, [.,.,B] with const_hessian and no hrep; hxx, hxu, huu [.,.,B]: what hrep repeats
struct KlDeriv {
    double *cx, *cu, *cxx, *cxu, *cuu, *fxw, *fuw, *hxx, *hxu, *huu;
    void carve(Carver &c, const KlWorkIn &w)
    {
        const size_t n = w.n, m = w.m, NB = w.N * w.B, hc = w.family ? (w.const_hessian && !w.hrep ? w.B : NB) : w.N, fxc = w.N * (w.fx_batched ? w.B : 1);
        cx = c.take<double>(n * NB); cu = c.take<double>(m * NB);
        cxx = c.take<double>(n * n * hc); cxu = c.take<double>(n * m * hc); cuu = c.take<double>(m * m * hc);
        fxw = c.take_if<double>(w.fx_own, n * n * fxc); fuw = c.take_if<double>(w.fx_own, n * m * fxc);
        hxx = c.take_if<double>(w.hrep, n * n * w.B); hxu = c.take_if<double>(w.hrep, n * m * w.B); huu = c.take_if<double>(w.hrep, m * m * w.B);
    }
};

// ∇kl of the previous policy (ddp_kl_terms writes them, back_pass_gps reads them through ddp_kl_cost_terms)
struct KlTerms {
    double *cx, *cu, *cxx, *cxu, *cuu;
    void carve(Carver &c, const KlWorkIn &w)
    {
        const size_t n = w.n, m = w.m, NB = w.N * w.B;
        cx = c.take<double>(n * NB); cu = c.take<double>(m * NB); cxx = c.take<double>(n * n * NB); cxu = c.take<double>(m * n * NB);
        cuu = c.take<double>(m * m * NB);
    }
};

// the dual state of every trajectory and what the dual steps read and write besides: etab [3,B] of the driver's own (the caller may bring
// one), klmean [B], diverge [B] of the back pass
struct KlDual {
    ddp_kl_dual s;
    double *etab_own, *klm;
    int32_t *div;
    void carve(Carver &c, const KlWorkIn &w)
    {
        const size_t B = w.B;
        etab_own = c.take<double>(3 * B);
        s.etab = etab_own; s.eta = c.take<double>(B); s.del = c.take<double>(B); s.divergence = c.take<double>(B);
        s.satisfied = c.take<int32_t>(B); s.status = c.take<int32_t>(B); s.live = c.take<int32_t>(B); s.pend = c.take<int32_t>(B);
        s.iters = c.take<int32_t>(B); s.nback = c.take<int32_t>(B);
        div = c.take<int32_t>(B); klm = c.take<double>(B);
    }
};

struct KlWork {
    int32_t *counter;
    KlDeriv dv;
    KlTerms kt;
    KlDual dual;
    // k: the new policy's feed-forward; kzero: zeros (traj_prev.k *= 0); sig: sigmanew [n+m,n+m,N,B]; kld [N,B]; cs: the rollout's cost
    // sums; x0c: x0[:,1,:]; c0buf: sum(cost0) when the caller leaves cost0 out
    double *k, *kzero, *sig, *kld, *cs, *x0c, *c0buf;
    // returns the end of the block: its size when run from address 0
    size_t carve(Carver c, const KlWorkIn &w)
    {
        const size_t n = w.n, m = w.m, B = w.B, NB = w.N * B;
        counter = c.take<int32_t>(64);       // first: the stand-alone ddp_kl_dual_* entry points keep theirs at the scratch base
        dv.carve(c, w); kt.carve(c, w); dual.carve(c, w);
        k = c.take<double>(m * NB); kzero = c.take<double>(m * NB); sig = c.take<double>((n + m) * (n + m) * NB); kld = c.take<double>(NB);
        cs = c.take<double>(B); x0c = c.take<double>(n * B); c0buf = c.take<double>(B);
        return (size_t)c.p;
    }
};
