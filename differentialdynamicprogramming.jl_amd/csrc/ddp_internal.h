// ddp_internal.h — shared between the translation units of libddp_amd.so (not installed).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <string>
#include <utility>
#include <vector>
#include "../../include/ddp_amd.h"

#define DDP_WAVE 64
#define DDP_MAX_N_GENERIC 32      // run-time-sized kernels: n <= 32, m <= DDP_MAX_M
#define DDP_SH_MIN_N 16           // the shared-operand backward pass needs two chunks of steps (back_pass_sh.hip)

// The DDP_* switches of the dispatchers (kernel choice for A/B timing and for the tests that force every code path) are read from the
// environment ONCE per handle (ddp_create) and again on ddp_reload_env(): no launch calls getenv, and a setenv() in another thread
// cannot race with a launch.  ddp_env() returns the cached value or nullptr.
enum ddp_env_id { ENV_BACKPASS, ENV_SH_MIN_B, ENV_MX2, ENV_DPPW, ENV_MX_LDS, ENV_Q4_SINGLE, ENV_Q4_LDS, ENV_GPS_Q4, ENV_GPS_Q4L, ENV_DF_DENSE, ENV_FORWARD, ENV_FORWARD64, ENV_FORWARD_FAST, ENV_FORWARD_FUSE, ENV_FORWARD_LANE, ENV_FORWARD_PEND, ENV_FORWARD_PIPE, ENV_ILQG_COMPACT, ENV_ILQG_LSGROUPS, ENV_TEST_COMPACT_ALLOC_FAIL, ENV_GPS_LANE, ENV_FCOV_Q4, ENV_FCOV_Q4L, ENV_KL_LDS, ENV_TEST_SH_ABORT, ENV_MXG_COAL, ENV_FORWARD_MID, ENV_PEND_CHUNK, ENV_GPS_MID, ENV_GPS_WIDE, ENV_SH_REUSE, ENV_COUNT };

struct ddp_handle_s {
    int          device;
    hipStream_t  stream;
    bool         owns_stream;
    // scratch owned by the handle (host-pointer entry points, iLQG driver)
    void        *scratch;
    size_t       scratch_bytes;
    int32_t     *h_pinned;        // small pinned buffer for polling
    void        *pad;             // operands / results of a backward pass padded to even sizes (back_pass.hip), grown on demand
    size_t       pad_bytes;
    void        *sh;              // back_pass_sh.hip: control block, work items, record streams of the shared-LTI backward pass
    size_t       sh_bytes;
    int          sh_timeouts;     // timed-out tiles counted by control blocks that have been freed (ddp_sh_timeouts)
    hipStream_t  sh_last_stream;  // the stream of the last shared-LTI launch (the record streams it kept are reused in stream order only)
    bool         sh_launched;
    int          ncu;             // compute units of the device (0: not asked yet)
    struct { const void *Q, *R; int n, m, ok; } diag_cache[8];      // verdicts of ddp_check_cost_diag (forward_pass.hip)
    int          diag_next;
    int          diag_skip;       // > 0: a host-pointer flavour has verified Q, R on the host and staged them itself (addresses recycle)
    hipStream_t  sched_aux;       // ilqg.hip, slot scheduler: side stream of the initial rollouts + its two events (created on first use)
    hipEvent_t   sched_ev[2];
    char         envv[ENV_COUNT][24];
    bool         envset[ENV_COUNT];
    const char  *last_kernel[7];  // what the last backward / forward / user-derivative / user-cost / user-plant / forward_covariance / kl_div_wiki dispatch launched (ddp_last_kernel)
    void        *sink;            // 4 KB of device memory that masked-out lanes may write (stores without an exec-mask branch) + a flag word (df.hip)
    std::vector<std::pair<const void *, int>> lds_raised;   // kernels whose dynamic-LDS limit has been raised on this device, to how many bytes
    double      *timing;          // ddp_ilqg_set_timing: host buffer [3, timing_cap] or NULL
    int          timing_cap;
    hipEvent_t   tev[4];          // created on first use
    bool         tev_ok;
    int          kl_wide;         // ddp_kl_set_wide: the KL functions take n <= 64, m <= DDP_MAX_M_WIDE
    void        *user_cache;      // user_problem.hip: the modules of the user problems compiled for this handle (unloaded by ddp_destroy)
    double      *kl_steps = nullptr;   // ddp_kl_set_steps: one kl_step per trajectory, the handle's own device copy (NULL: the scalar of the call)
    int          kl_steps_B = 0;
};

void ddp_set_error(const char *fmt, ...);
static inline const char *ddp_env(ddp_handle h, int id) { return h->envset[id] ? h->envv[id] : nullptr; }

#define DDP_HIP(call)                                                                         \
    do {                                                                                      \
        hipError_t e_ = (call);                                                               \
        if (e_ != hipSuccess) {                                                               \
            ddp_set_error("%s failed: %s (%s:%d)", #call, hipGetErrorString(e_), __FILE__,    \
                          __LINE__);                                                          \
            return -2;                                                                        \
        }                                                                                     \
    } while (0)

#define DDP_CHECK(cond, ...)                                                                  \
    do {                                                                                      \
        if (!(cond)) {                                                                        \
            ddp_set_error(__VA_ARGS__);                                                       \
            return -1;                                                                        \
        }                                                                                     \
    } while (0)

// every public entry point makes the handle's device current first: a process may hold handles on several devices, and scratch
// allocations / kernel launches go to the CURRENT device of the calling thread.  A handle is single-threaded (ddp_amd.h).
#define DDP_DEVICE(h)                                                                         \
    do {                                                                                      \
        if (!(h)) { ddp_set_error("null handle"); return -1; }                                \
        DDP_HIP(hipSetDevice((h)->device));                                                   \
    } while (0)

// grows the handle's scratch to at least `bytes` (contents not preserved)
int ddp_scratch(ddp_handle h, size_t bytes, void **out);
// the same for the handle's pad buffer (the padded or combined operands of a backward pass); the caller has made the device current
int ddp_pad(ddp_handle h, size_t bytes, void **out);

// ddp_problem::cost_diag = 1 declares Q and R diagonal (the fused rollout cost reads only the diagonals): verified on the first call
// with a (Q, R) pointer pair — one small device-to-host copy — and cached per handle; 0 ok, < 0 refused
int ddp_check_cost_diag(ddp_handle h, const ddp_problem *p);
// the same test on HOST copies of Q, R (the host-pointer flavours, before they stage the problem); while a DiagVerified lives the
// device-side test is skipped for this handle (the staging addresses are recycled from call to call: a pointer-keyed verdict would go stale)
int ddp_check_cost_diag_host(const ddp_problem *p);
struct DiagVerified { ddp_handle h; explicit DiagVerified(ddp_handle h_) : h(h_) { ++h->diag_skip; } ~DiagVerified() { --h->diag_skip; } };

// user_problem.hip: unloads the handle's user-problem modules (ddp_destroy)
void ddp_user_release(ddp_handle h);

// A problem family the iLQG driver (ilqg.hip) runs besides the registered ddp_problem kinds: the user's compiled problems
// (user_problem.hip).  `map` (may be NULL) is the slot -> trajectory map of a compacted working set; the family reads what it keeps
// per trajectory (its parameters) through it.  Derivatives are time-varying and per trajectory (fx[n,n,N,B] ...); the cost Hessians
// too, or, with const_hessian, one set per trajectory written by hessians() (cxx[n,n,B] ...) for the slots `active` names (NULL: all).
// The slot scheduler's map also holds -1 (empty slot) and -2 (resting slot): the family never reads parameters through those.
// has_plant: the closed loop of ddp_ilqg_sched_family_dev advances its trajectories with plant() instead of x_1 of the plan.
// second_order (DDP_USER_SECOND_ORDER): STEP 2 of the iLQG drivers calls back_pass() — the family's own backward pass, with the
// curvature of its dynamics — instead of the dispatcher of back_pass.hip; the call carries x and the slot map besides the operands.
// t0 (DDP_USER_CLOCK, else NULL): the clock of every trajectory (problem) of the call, t0[B] on the device.  clk is the array the
// family's kernels read, indexed by the slot they work on: t0 itself in a stand-alone call; a driver whose slots are not the caller's
// trajectories (the slot scheduler, a compacted working set) points it at its own per-slot array for the time of the call (ClockScope).
struct BPCall;
struct ddp_family {
    int n, m, N, B, CL;
    bool const_hessian, has_plant, second_order = false;
    const int32_t *t0 = nullptr;
    mutable const int32_t *clk = nullptr;
    // DDP_USER_FITTED (else NULL): fx[n,n,N,B], fu[n,m,N,B], fc[n,N,B] of a fitted time-varying affine model on the device.  While they
    // are set, rollout() runs x̂[i+1] = fx_i x̂_i + fu_i û_i + fc_i in place of the family's dynamics (ddp_user_rollout_fit); an entry sets
    // them for the time of its call (FitScope)
    mutable const double *fit_fx = nullptr, *fit_fu = nullptr, *fit_fc = nullptr;
    virtual ~ddp_family() {}
    virtual int back_pass(ddp_handle h, const BPCall &c) const { ddp_set_error("back_pass: the family has no backward pass of its own"); return -1; }
    virtual int df(ddp_handle h, int B, const int32_t *map, const double *x, const double *u, const int32_t *active, double *fx,
                   double *fu, double *cx, double *cu, double *cxx, double *cxu, double *cuu) const = 0;
    virtual int hessians(ddp_handle h, int B, const int32_t *map, const int32_t *active, double *cxx, double *cxu, double *cuu) const = 0;
    virtual int rollout(ddp_handle h, int B, const int32_t *map, const double *K, const double *k, const double *x0, const double *u,
                        const double *x, const double *alpha, int nalpha, const double *lims, const int32_t *active, double *xnew,
                        double *unew, double *cnew, double *csum) const = 0;
    virtual int costfun(ddp_handle h, int B, const int32_t *map, const double *x, const double *u, const int32_t *active, double *cost,
                        double *csum) const = 0;
    // closed loop, S slots: for every slot with adv[b] = t + 1 > 0 (its solve t of trajectory advp[b] has just ended)
    // xcl[:, t+1, advp[b]] = plant(xcl[:, t, .], ucl[:, t, .], t, params of advp[b]), and x0s[:, b] the same when the slot was re-armed
    // for that trajectory (map[b] == advp[b]).  xcl[n, steps+1, P], ucl[m, steps, P].
    virtual int plant(ddp_handle h, int S, int steps, const int32_t *adv, const int32_t *advp, const int32_t *map, const double *ucl,
                      double *xcl, double *x0s) const = 0;
};
// puts the family's clk back when the driver returns (every way out)
struct ClockScope {
    const ddp_family *f;
    const int32_t *was;
    explicit ClockScope(const ddp_family *f_) : f(f_), was(f_ ? f_->clk : nullptr) {}
    ~ClockScope() { if (f) f->clk = was; }
};
// sets the family's fitted tables for the time of a call and puts back what was there (every way out)
struct FitScope {
    const ddp_family *f;
    const double *was[3];
    FitScope(const ddp_family *f_, const double *fx, const double *fu, const double *fc) : f(f_), was{nullptr, nullptr, nullptr}   // f_ == NULL: nothing to set
    {
        if (!f) return;
        was[0] = f->fit_fx; was[1] = f->fit_fu; was[2] = f->fit_fc;
        f->fit_fx = fx; f->fit_fu = fu; f->fit_fc = fc;
    }
    ~FitScope() { if (f) { f->fit_fx = was[0]; f->fit_fu = was[1]; f->fit_fc = was[2]; } }
};
// the device-resident iLQG of ilqg.hip for such a family (arguments as ddp_ilqg_ex_f64_dev)
int ddp_ilqg_family_dev(ddp_handle h, const ddp_family *f, const ddp_ilqg_opts *o, const double *x0, int x0_prerolled, const double *u0,
                        const double *cost0, const double *lims, double *x, double *u, double *K, double *k, double *Quu, double *Vx,
                        double *Vxx, double *cost, double *stats, int trace_cap, double *trace7, int *global_iters);
// the slot scheduler of ilqg.hip for such a family: the queue (steps == 0; arguments as ddp_ilqg_queue_f64_dev, f->B = P problems) or
// the closed loop (steps >= 1; as ddp_ilqg_mpc_f64_dev, f->B = trajectories)
int ddp_ilqg_sched_family_dev(ddp_handle h, const ddp_family *f, const ddp_ilqg_opts *o, int slots, int steps, int zero_tail, const double *x0,
                              const double *u0, const double *lims, double *x, double *u, double *K, double *k, double *Quu, double *Vx,
                              double *Vxx, double *cost, double *stats, double *xcl, double *ucl, double *stats_cl, int *global_iters);

// One iLQGkl call as the C ABI passes it (ddp_ilqgkl_f64_dev, ddp_user_ilqgkl*_f64_dev): every entry fills one, the driver of kl.hip
// takes it.  Optional members are NULL when the entry has none.
struct KlCall {
    const ddp_ilqgkl_opts *opts = nullptr;                                     // NULL: ddp_ilqgkl_default_opts
    const double *x0 = nullptr, *cost0 = nullptr;                              // cost0 == NULL: costfun(x0, kp)
    const double *Kp = nullptr, *kp = nullptr, *Sp = nullptr, *Sip = nullptr;   // the previous policy
    const double *model_fx = nullptr;                                          // the model of forward_covariance; NULL (family only): the fx of STEP 1,
    int model_fx_batched = 0;                                                  // or fit_fx
    const double *R1 = nullptr, *lims = nullptr;
    double *etab = nullptr;                                                    // NULL: the driver's own, from opts->etabracket
    // a fitted model [.,.,N,B] (all three or none, family only): the loop plans on it — back_pass_gps takes fit_fx, fit_fu, the rollouts
    // run on the family with the tables set (FitScope)
    const double *fit_fx = nullptr, *fit_fu = nullptr, *fit_fc = nullptr;
    // a cost model cx[n,N,B], cu[m,N,B], cxx[n,n,N,B], cxu[n,m,N,B], cuu[m,m,N,B] (all five or none, family only): the backward passes
    // take these arrays in place of the cost derivatives STEP 1 wrote; nothing else of the loop changes
    const double *cm_cx = nullptr, *cm_cu = nullptr, *cm_cxx = nullptr, *cm_cxu = nullptr, *cm_cuu = nullptr;
    double *x = nullptr, *u = nullptr, *K = nullptr, *Sigma = nullptr, *Sigmai = nullptr, *Vx = nullptr, *Vxx = nullptr, *cost = nullptr,
           *dV = nullptr, *stats = nullptr;
    int *iters = nullptr;                                                      // may stay NULL
};
// the device-resident iLQGkl of kl.hip for such a family (arguments as ddp_ilqgkl_f64_dev)
int ddp_ilqgkl_family_dev(ddp_handle h, const ddp_family *f, const KlCall &c);

// sample.hip: the lower Cholesky factors L[m,m,N,B] of Sigma[m,m,N,B] and status[B] (0, or i + 1 of the first step that is not positive
// definite), and the moments xmean[n,N,B] / xcov[n,n,N,B] (either may be NULL) of xs[n,N,S,B] over its samples; the device is current
int ddp_policy_factor_dev(ddp_handle h, int m, int N, int B, const double *Sigma, double *L, int32_t *status);
int ddp_sample_moments_dev(ddp_handle h, int n, int N, int S, int B, const double *xs, double *xmean, double *xcov);

// raises the dynamic-LDS limit of `kernel` to at least `bytes`, once per handle (capi.hip; the attribute belongs to the device the handle
// runs on: a process-wide flag would leave a second handle on another device at the 64 KB default)
int ddp_raise_lds(ddp_handle h, const void *kernel, int bytes);

// One backward-pass call: the descriptor, operands and results as the C ABI passes them (ddp_back_pass_f64_dev), and for back_pass_gps
// its KL terms and Quui.  Every backward-pass launcher takes one; back_pass.hip chooses which one runs.
struct BPCall {
    ddp_bp_desc d;
    const double *cx, *cu, *cxx, *cxu, *cuu, *fx, *fu, *lambda, *lims, *u;
    const int32_t *active;
    double *K, *k, *Quu, *Vx, *Vxx, *dV;
    int32_t *diverge;
    const ddp_kl_cost_terms *kl = nullptr;      // back_pass_gps only
    double *Quui = nullptr;                     // back_pass_gps only
    const double *x = nullptr;                  // ddp_family::back_pass only: the nominal states x[n,N,B]
    const int32_t *map = nullptr;               // ddp_family::back_pass only: slot -> trajectory map of the working set (may be NULL)
};

// The kernel argument of the dpp, dppw, row, big, mfma and gps_lane families (the general, mx, mxg, mid, mf2, q4, wide and shared-operand
// kernels keep structs of their own): the descriptor, the element strides it implies, the call's pointers in BPCall's order, the KL terms
// of back_pass_gps and the handle's sink.  bp_kargs fills it; a launcher changes only what is particular to its kernel.  (The field
// order keeps every field the row kernels read at the offset it had in their own struct: their compiler records are the ones they had.)
struct BPKArgs {
    int n, m, N, B, regType, has_lims;
    long fx_t, fx_b, fu_t, fu_b, cxx_t, cxx_b, cxu_t, cxu_b, cuu_t, cuu_b;      // element strides per time step / per trajectory (0: shared)
    const double *cx, *cu, *cxx, *cxu, *cuu, *fx, *fu, *lambda, *lims, *u;
    const int32_t *active;
    double *K, *k, *Quu, *Vx, *Vxx, *dV;
    int32_t *diverge;
    double *sink;               // the handle's 4 KB that lanes without an output may write (stores without an exec-mask branch); may be NULL
    // back_pass_gps (backward_pass.jl:259-350): ∇kl [n,N,B] [m,N,B] [n,n,N,B] [m,n,N,B] [m,m,N,B], η [B] or [N,B] (eta_tv), Quui = inv(Quu)
    const double *kcx, *kcu, *kcxx, *kcxu, *kcuu;
    int eta_tv, fx_tv;
    const double *eta;
    double *Quui;
    int fx_batched, cost_tv, cost_batched;
};
inline BPKArgs bp_kargs(ddp_handle h, const BPCall &c)
{
    BPKArgs a = {};
    const ddp_bp_desc &d = c.d;
    a.n = d.n; a.m = d.m; a.N = d.N; a.B = d.B; a.regType = d.regType; a.has_lims = d.has_lims;
    a.fx_tv = d.fx_tv; a.fx_batched = d.fx_batched; a.cost_tv = d.cost_tv; a.cost_batched = d.cost_batched;
    const long N = d.N, nn = (long)d.n * d.n, nm = (long)d.n * d.m, mm = (long)d.m * d.m;
    auto set = [N](long &t, long &b, long len, int tv, int batched) { t = tv ? len : 0; b = batched ? len * (tv ? N : 1) : 0; };
    set(a.fx_t, a.fx_b, nn, d.fx_tv, d.fx_batched);
    set(a.fu_t, a.fu_b, nm, d.fx_tv, d.fx_batched);
    set(a.cxx_t, a.cxx_b, nn, d.cost_tv, d.cost_batched);
    set(a.cxu_t, a.cxu_b, nm, d.cost_tv, d.cost_batched);
    set(a.cuu_t, a.cuu_b, mm, d.cost_tv, d.cost_batched);
    a.cx = c.cx; a.cu = c.cu; a.cxx = c.cxx; a.cxu = c.cxu; a.cuu = c.cuu; a.fx = c.fx; a.fu = c.fu; a.lambda = c.lambda; a.lims = c.lims;
    a.u = c.u; a.active = c.active;
    a.K = c.K; a.k = c.k; a.Quu = c.Quu; a.Vx = c.Vx; a.Vxx = c.Vxx; a.dV = c.dV; a.diverge = c.diverge;
    if (c.kl) { a.kcx = c.kl->cx; a.kcu = c.kl->cu; a.kcxx = c.kl->cxx; a.kcxu = c.kl->cxu; a.kcuu = c.kl->cuu; a.eta = c.kl->eta; a.eta_tv = c.kl->eta_tv; }
    a.Quui = c.Quui;
    a.sink = (double *)h->sink;
    return a;
}

// the dispatcher (back_pass.hip) and back_pass_gps (run-time sizes n <= 32, m <= 8)
int ddp_launch_back_pass(ddp_handle h, const BPCall &c);
int ddp_launch_back_pass_gps(ddp_handle h, const BPCall &c);
// Family launchers.  Each launches the kernel of its family for a call back_pass.hip has chosen it for (the shape and alignment tests
// live there); 0 launched, < 0 error.
// back_pass_gps for n = 4, m <= 2 and time-varying operands, one lane per trajectory (back_pass_gps_lane.hip); 1 = not applicable
int ddp_launch_back_pass_gps_lane(ddp_handle h, const BPCall &c);
// back_pass_gps for n = 4, m = 1 with one η per trajectory on the matrix cores (back_pass_q4.hip); 1 = not applicable
int ddp_launch_back_pass_gps_q4(ddp_handle h, const BPCall &c);
// n=10, m=2, no limits: one wave per trajectory, all matrices of a step in one 16x16 fp64 MFMA tile (back_pass_mx.hip)
int ddp_launch_back_pass_mx(ddp_handle h, const BPCall &c);
// any n <= 10, m <= 2 without limits inside the same tile (run-time sizes, results straight to global memory)
int ddp_launch_back_pass_mxr(ddp_handle h, const BPCall &c);
// the same tile arithmetic with a chain wave + a write-back wave per trajectory (back_pass_mx2.hip)
int ddp_launch_back_pass_mx2(ddp_handle h, const BPCall &c);
// the tile kernel for any n <= 12, m <= 4 (m <= 3 above n = 8), with or without limits (back_pass_mxg.hip)
int ddp_launch_back_pass_mxg(ddp_handle h, const BPCall &c);
// the 16-lane-row kernel compiled for padded sizes — any n <= 14, m <= 4 with n + m <= 15 (back_pass_row.hip)
int ddp_launch_back_pass_row(ddp_handle h, const BPCall &c);
// one wave per trajectory, the products on the fp64 matrix cores with LDS operands — any n <= 32, m <= 8 (back_pass_mid.hip)
int ddp_launch_back_pass_mid(ddp_handle h, const BPCall &c);
// back_pass_gps on the same kernel (GPS instantiations, KL terms combined by a prepass) — any n <= 32, m <= 8; 1 = not applicable
int ddp_launch_back_pass_gps_mid(ddp_handle h, const BPCall &c);
// back_pass_gps on the wide-control kernel (the GPS instantiation of back_pass_wide.hip) — any n <= 64, m <= DDP_MAX_M_WIDE
int ddp_launch_back_pass_gps_wide(ddp_handle h, const BPCall &c);
// the KL kernels of the same shapes (kl_wide.hip): ∇kl, forward_covariance, kl_div_wiki; the entry points of kl.hip choose them
int ddp_launch_kl_terms_wide(ddp_handle h, int n, int m, int N, int B, const double *K, const double *k, const double *Sigmai,
                             double *cx, double *cu, double *cxx, double *cxu, double *cuu);
int ddp_launch_fcov_wide(ddp_handle h, int n, int m, int N, int B, const double *fx, int fx_batched, const double *R1, const double *K,
                         const double *Sigma, double *sigmanew);
int ddp_launch_kl_div_wide(ddp_handle h, int n, int m, int N, int B, const double *xnew, const double *xold, const double *sigmanew,
                           const double *Kn, const double *kn, const double *Sn, const double *Kp, const double *kp, const double *Sp,
                           const double *Sip, double *kldiv, double *klmean);
// shared time-invariant operands (n=10, m=2, no limits): the matrix recursion once per distinct λ, an affine chain per trajectory
// (back_pass_sh.hip); the trajectories it left out are flagged in *fb_active
extern "C" int ddp_sh_max_tiles(int B, int ncu);      // capacity of its work-item list: the most consumer tiles any grouping of B trajectories can make
int ddp_launch_back_pass_sh(ddp_handle h, const BPCall &c, const int32_t **fb_active);
// 16-lane DPP-row backward pass, 4 trajectories per wave, (10, 2) and (4, 1) (back_pass_dpp.hip)
int ddp_launch_back_pass_dpp(ddp_handle h, const BPCall &c);
// the (10, 2) row kernel with a write-back wave per chain wave (back_pass_dppw.hip)
int ddp_launch_back_pass_dppw(ddp_handle h, const BPCall &c);
// n = 4, m = 1 on v_mfma_f64_4x4x4_4b, one trajectory per MFMA block (back_pass_q4.hip)
int ddp_launch_back_pass_q4(ddp_handle h, const BPCall &c);
// large states (even n <= 64, even m <= 8): 256-thread work-group per trajectory (back_pass_big.hip)
int ddp_launch_back_pass_big(ddp_handle h, const BPCall &c);
// 32 < n <= 64, m <= 8 at run time: every product on the fp64 matrix cores (back_pass_mf2.hip), and the round-5 kernel of the exact
// n = 64, m = 8 shape (back_pass_mfma.hip).  `lims_active`: has_lims with real limits (lims[1,1] <= lims[1,2]), read by the caller
int ddp_launch_back_pass_mf2(ddp_handle h, const BPCall &c, bool lims_active);
int ddp_launch_back_pass_mfma(ddp_handle h, const BPCall &c, bool lims_active);
// wide controls, any n <= 64 with m <= DDP_MAX_M_WIDE at run time: one work-group of four waves per trajectory (back_pass_wide.hip)
int ddp_launch_back_pass_wide(ddp_handle h, const BPCall &c);
// One forward-pass call as the C ABI passes it (ddp_forward_pass_f64_dev).  Every rollout launcher takes one; forward_pass.hip chooses
// which one runs (fp_choose) and hands the launchers of several kernels the FPChoice it made.
struct FPCall {
    const ddp_problem *p;
    const double *K, *k, *x0, *u, *x, *alpha, *lims;
    int nalpha;
    const int32_t *active;
    double *xnew, *unew, *cnew, *csum;
};
// one enumerator per rollout kernel that differs (forward_pass.hip: the family overview and the names ddp_last_kernel(h, 1) reports)
enum FPKernel { FP_NONE, FP_WIDE, FP_BIG64, FP_MID, FP_BIG, FP_PIPE4, FP_PIPE, FP_PIPE_TV, FP_PEND_LANE, FP_PEND_ROW, FP_DPP, FP_ROW, FP_GROUP };
// fuse: pipe, pendulum and dpp kernels, the cost inside the rollout kernel (cost_diag without DDP_FORWARD_FUSE=0); chunked: FP_PEND_ROW, whole
// 16-step chunks through LDS; fast: FP_DPP, the instantiation without the run-time dyn_tv test and with unmasked stores; wrap: pendulum
// kernels, the instantiation that wraps x̂ - x (diff_wrap with a policy); cost_mid: FP_BIG, cost_mid_kernel behind forward_big_kernel
// (cost_rt_kernel otherwise); na: FP_BIG64, step sizes of a trajectory per wave (1, 2 or 4)
struct FPChoice { FPKernel k; bool fuse, chunked, fast, wrap, cost_mid; int na; };
// what the argument struct of every rollout kernel takes from the call
template <class Args>
static inline void fp_fill(Args &a, const FPCall &c)
{
    a.N = c.p->N; a.B = c.p->B; a.nalpha = c.nalpha;
    a.A = c.p->A; a.Bm = c.p->Bm; a.Q = c.p->Q; a.R = c.p->R; a.K = c.K; a.k = c.k; a.x0 = c.x0; a.u = c.u; a.x = c.x; a.active = c.active;
    for (int i = 0; i < 16; ++i) a.alpha[i] = i < c.nalpha ? c.alpha[i] : 0.0;
    a.xnew = c.xnew; a.unew = c.unew; a.cnew = c.cnew; a.csum = c.csum;
}
// Rollout launchers.  Each launches the kernel fp_choose has chosen it for (the shape, switch, batch-size and alignment tests live there);
// 0 launched, < 0 error.
// the 16-lane-row rollout compiled for padded sizes (forward_pass_row.hip): LQ, n <= 14, m <= 4 minus n > 12 with m > 2
int ddp_launch_forward_row(ddp_handle h, const FPCall &c);
// FP_DPP, FP_PEND_ROW, FP_PEND_LANE: 16-lane rows for LQ (10, 2) and pendcart, the pendulum's own row and lane kernels (forward_pass_dpp.hip)
int ddp_launch_forward_dpp(ddp_handle h, const FPCall &c, const FPChoice &ch);
// one wave per rollout for wide controls (LQ family, n <= 64, 8 < m <= DDP_MAX_M_WIDE; forward_pass_wide.hip)
int ddp_launch_forward_wide(ddp_handle h, const FPCall &c);
// FP_PIPE4, FP_PIPE, FP_PIPE_TV: the LQ (10, 2) rollout as a producer/consumer pipeline, one work-group per 4 rollouts (forward_pass_pipe.hip)
int ddp_launch_forward_pipe(ddp_handle h, const FPCall &c, const FPChoice &ch);
// FP_BIG64, FP_MID, FP_BIG: one wave per rollout for large states (LQ family, n <= 64, m <= DDP_MAX_M; forward_pass_big.hip)
int ddp_launch_forward_big(ddp_handle h, const FPCall &c, const FPChoice &ch);

struct QPOptsDev;
int ddp_launch_boxqp_big(ddp_handle h, int m, int count, const double *H, const double *g, const double *lower, const double *upper,
                         const double *x0, const QPOptsDev &o, double *x, int32_t *result, double *Hfree, uint8_t *free_out);   // boxqp_big.hip

// 1/sqrt(x): hardware estimate (v_rsq_f64) + two Newton steps -> ~1 ulp.  The caller checks x > 0.
__device__ __forceinline__ double ddp_rsqrt(double x)
{
    double y = __builtin_amdgcn_rsq(x);
    double e = fma(-(x * y), y, 1.0);
    y = fma(0.5 * y, e, y);
    e = fma(-(x * y), y, 1.0);
    y = fma(0.5 * y, e, y);
    return y;
}

// Upper Cholesky of H (column-major M x M, upper triangle read) with RECIPROCAL pivots: fills the strictly upper
// entries of R and ri[j] = 1/R[j][j].  Division-free (v_rsq_f64 + Newton), which matters where every lane repeats
// the factorisation.  Returns 0, or j+1 for the first non-positive pivot (LAPACK potrf semantics).
template <int M>
__device__ __forceinline__ int ddp_chol_rinv(const double (&H)[M * M], double (&R)[M * M], double (&ri)[M])
{
    int fail = 0;
#pragma unroll
    for (int c = 0; c < M; ++c) {
        double ajj = H[c + M * c];
#pragma unroll
        for (int k2 = 0; k2 < c; ++k2) ajj -= R[k2 + M * c] * R[k2 + M * c];
        if (!(ajj > 0.0) && fail == 0) fail = c + 1;
        ri[c] = ddp_rsqrt(ajj);
#pragma unroll
        for (int c2 = c + 1; c2 < M; ++c2) {
            double s = H[c + M * c2];
#pragma unroll
            for (int k2 = 0; k2 < c; ++k2) s -= R[k2 + M * c] * R[k2 + M * c2];
            R[c + M * c2] = s * ri[c];
        }
    }
    return fail;
}
// b <- -(R'R)\b with the factor of ddp_chol_rinv
template <int M>
__device__ __forceinline__ void ddp_rsolve_neg(const double (&R)[M * M], const double (&ri)[M], double (&b)[M])
{
#pragma unroll
    for (int c = 0; c < M; ++c) {
        double s = b[c];
#pragma unroll
        for (int k2 = 0; k2 < c; ++k2) s -= R[k2 + M * c] * b[k2];
        b[c] = s * ri[c];
    }
#pragma unroll
    for (int c = M - 1; c >= 0; --c) {
        double s = b[c];
#pragma unroll
        for (int k2 = c + 1; k2 < M; ++k2) s -= R[c + M * k2] * b[k2];
        b[c] = s * ri[c];
    }
#pragma unroll
    for (int c = 0; c < M; ++c) b[c] = -b[c];
}

// Hand-off between the lanes of ONE wavefront through LDS.  The kernels that use it run one wave per
// work-group, so no s_barrier is needed: LDS operations of a wave execute in issue order, the only
// requirements are (a) the compiler must not move LDS accesses across the hand-off and (b) nothing may
// wait on outstanding GLOBAL stores/loads here (__syncthreads() would emit s_waitcnt vmcnt(0) and stall
// every hand-off on the HBM round trip of the step's output stores).
__device__ __forceinline__ void wave_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
