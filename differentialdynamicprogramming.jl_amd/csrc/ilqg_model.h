// ilqg_model.h — the problem as the iLQG drivers (ilqg.hip) and the iLQGkl driver (kl.hip) see it, and the derivative workspace they
// hand to it.  A driver runs a registered ddp_problem kind or a ddp_family (a user problem); Model is the only place that asks which.
#pragma once
#include "carver.h"
#include "ddp_internal.h"

struct Model;
// workspace of STEPS 1-2 for `slots` trajectories: what df writes (fxw, fuw: dynamics of the problem's own; hxx, hxu, huu: the cost
// Hessians of a ddp_family, [.,.,N,slots] or with const_hessian [.,.,slots]), the zero cxu[n,m] of the registered kinds (cleared by the
// driver), and what the backward pass returns besides the gains: dV[2,slots], diverge[slots]
struct Deriv {
    double *cx, *cu, *fxw, *fuw, *hxx, *hxu, *huu, *cxu, *dV;
    int32_t *div;
    inline void carve(Carver &c, const Model &M, size_t slots);
};

struct Model {
    const ddp_family *fam;              // NULL: the registered kind of pw
    ddp_problem pw;                     // the registered problem; for a family a shell that carries the sizes only (kind = -1)
    int n, m, N, B, CL;                 // B: the trajectories (problems) of the call
    bool own_fx, const_hessian, second_order, has_plant, clocked;

    Model(const ddp_problem *p, const ddp_family *f) : fam(f), pw()
    {
        if (f) { pw.kind = -1; pw.n = f->n; pw.m = f->m; pw.N = f->N; pw.B = f->B; }
        else pw = *p;
        n = pw.n; m = pw.m; N = pw.N; B = pw.B; CL = f ? f->CL : ddp_cost_len(&pw);
        own_fx = f || pw.kind == DDP_PROBLEM_PENDCART;        // time-varying per-trajectory fx, fu written by df
        const_hessian = f && f->const_hessian; second_order = f && f->second_order; has_plant = f && f->has_plant; clocked = f && f->t0;
    }
    // the problem as the kernels of a registered kind see it: B = slots of the working set
    ddp_problem sized(int slots) const { ddp_problem q = pw; q.B = slots; return q; }

    // The calls of ddp_family (slot count, slot -> trajectory map, active mask, outputs); a registered kind has no use for the map.
    // const_hessian: df leaves the Hessians alone, hessians() writes them once per trajectory (and does nothing otherwise).
    int df(ddp_handle h, int slots, const int32_t *map, const double *x, const double *u, const int32_t *active, double *fx, double *fu,
           double *cx, double *cu, double *cxx, double *cxu, double *cuu) const
    {
        const ddp_problem q = sized(slots);
        const bool ch = const_hessian;
        return fam ? fam->df(h, slots, map, x, u, active, fx, fu, cx, cu, ch ? nullptr : cxx, ch ? nullptr : cxu, ch ? nullptr : cuu)
                   : ddp_df_f64_dev(h, &q, x, u, active, cx, cu, fx, fu);
    }
    int hessians(ddp_handle h, int slots, const int32_t *map, const int32_t *active, double *cxx, double *cxu, double *cuu) const
    {
        return const_hessian ? fam->hessians(h, slots, map, active, cxx, cxu, cuu) : 0;
    }
    int rollout(ddp_handle h, int slots, const int32_t *map, const double *K, const double *k, const double *x0, const double *u,
                const double *x, const double *alpha, int nalpha, const double *lims, const int32_t *active, double *xnew, double *unew,
                double *cnew, double *csum) const
    {
        const ddp_problem q = sized(slots);
        return fam ? fam->rollout(h, slots, map, K, k, x0, u, x, alpha, nalpha, lims, active, xnew, unew, cnew, csum)
                   : ddp_forward_pass_f64_dev(h, &q, K, k, x0, u, x, alpha, nalpha, lims, active, xnew, unew, cnew, csum);
    }
    int costfun(ddp_handle h, int slots, const int32_t *map, const double *x, const double *u, const int32_t *active, double *cost, double *csum) const
    {
        const ddp_problem q = sized(slots);
        return fam ? fam->costfun(h, slots, map, x, u, active, cost, csum) : ddp_costfun_f64_dev(h, &q, x, u, active, cost, csum);
    }
    // closed loop with has_plant: ddp_family::plant
    int plant(ddp_handle h, int slots, int steps, const int32_t *adv, const int32_t *advp, const int32_t *map, const double *ucl, double *xcl,
              double *x0s) const { return fam->plant(h, slots, steps, adv, advp, map, ucl, xcl, x0s); }
    // STEP 2: the family's own pass when second_order (it takes the nominal states and the slot map as well), else the dispatcher
    int back_pass(ddp_handle h, BPCall &c, const double *x, const int32_t *map) const
    {
        if (!second_order) return ddp_launch_back_pass(h, c);
        c.x = x; c.map = map;
        return fam->back_pass(h, c);
    }
    // the sizes and operand flags of the descriptor and the seven operands of a backward pass over the derivatives in `w`: the
    // dynamics df wrote or the problem's A, Bm; the family's Hessians (one set per trajectory with const_hessian) or the problem's Q, 0, R
    void operands(BPCall &c, const Deriv &w, int slots) const
    {
        c.d.n = n; c.d.m = m; c.d.N = N; c.d.B = slots;
        c.d.fx_tv = own_fx ? 1 : pw.dyn_tv; c.d.fx_batched = own_fx ? 1 : pw.dyn_batched;
        c.d.cost_tv = (fam && !const_hessian) ? 1 : 0; c.d.cost_batched = fam ? 1 : 0;
        c.cx = w.cx; c.cu = w.cu; c.fx = own_fx ? w.fxw : pw.A; c.fu = own_fx ? w.fuw : pw.Bm;
        c.cxx = fam ? w.hxx : pw.Q; c.cxu = fam ? w.hxu : w.cxu; c.cuu = fam ? w.huu : pw.R;
    }
};

inline void Deriv::carve(Carver &c, const Model &M, size_t slots)
{
    const size_t n = M.n, m = M.m, N = M.N, hT = M.const_hessian ? 1 : N;
    const bool fam = M.fam != nullptr;
    cx = c.take<double>(n * N * slots); cu = c.take<double>(m * N * slots);
    fxw = c.take_if<double>(M.own_fx, n * n * N * slots); fuw = c.take_if<double>(M.own_fx, n * m * N * slots);
    hxx = c.take_if<double>(fam, n * n * hT * slots); hxu = c.take_if<double>(fam, n * m * hT * slots); huu = c.take_if<double>(fam, m * m * hT * slots);
    cxu = c.take<double>(n * m); dV = c.take<double>(2 * slots); div = c.take<int32_t>(slots);
}
