// user_problem.hip — user-defined problems: the user's f / costfun / df as HIP device source, compiled at run time for gfx950.
//
// The reference's iLQG(f, costfun, df, x0, u0; ...) takes the user's own closures.  Here the user writes four device functions
// (include/ddp_amd.h lists the contract); the library wraps them in its kernel templates (user_problem_kernels.h), compiles the
// program with hiprtc once per (source, n, m, nparam, flags, diff_wrap) and handle (user_program.hip), and loads it on the handle's
// device.  The device-resident iLQG of ilqg.hip runs such a problem through its ddp_family interface (behind Model, ilqg_model.h), so
// the whole loop — statuses, trace keys, timing, pre-rolled starts, compaction, the slot scheduler — is the one the registered kinds run.
#include <string.h>
#include <map>
#include <string>
#include <vector>
#include "ddp_internal.h"
#include "staging.h"
#include "user_program.h"
#include "user_constraints.h"
#include "user_problem_kernels.h"
#include "user_sample_kernels.h"
#include "user_fitted_kernels.h"
#include "user_cost_fit_kernels.h"
#include "back_pass_wide_kernel.h"   // BPWArgs, WLds, bpw_fill: the wide kernel's step, shared with ddp_user_back_pass2_wave

DDP_USER_ABI
DDP_USER_ABI2
DDP_USER_ABI3
DDP_USER_ABI_C
DDP_USER_ABI_SAMPLE
DDP_USER_ABI_FIT
DDP_USER_ABI_COST_FIT

using user_program::Layout;

namespace {

// device storage a problem keeps between calls and grows on demand: no allocation per call once the largest batch has been seen
struct DevBuf {
    void *ptr = nullptr;
    size_t cap = 0;
    DevBuf() = default;
    DevBuf(const DevBuf &) = delete;
    ~DevBuf() { if (ptr) (void)hipFree(ptr); }
    template <class T> T *as() const { return (T *)ptr; }
    // at least `bytes`; the contents do not survive growth.  A failed allocation leaves the buffer empty
    int reserve(hipStream_t stream, size_t bytes)
    {
        if (bytes <= cap) return 0;
        const int rc = release(stream);
        if (rc) return rc;
        DDP_HIP(hipMalloc(&ptr, bytes));
        cap = bytes;
        return 0;
    }
    // kernels in flight on `stream` may still read the block: they finish before it is freed
    int release(hipStream_t stream)
    {
        if (!ptr) return 0;
        DDP_HIP(hipStreamSynchronize(stream));
        void *p = ptr;
        ptr = nullptr; cap = 0;
        DDP_HIP(hipFree(p));
        return 0;
    }
};

struct Module {
    hipModule_t mod = nullptr;
    hipFunction_t roll = nullptr, df = nullptr, cost = nullptr, hess = nullptr, plant = nullptr, bp2 = nullptr, vhess = nullptr;
    hipFunction_t bp2w = nullptr;                                // ddp_user_back_pass2_wave (DDP_USER_SECOND_ORDER_WAVE)
    hipFunction_t sample = nullptr;                              // ddp_user_sample (DDP_USER_SAMPLE) or ddp_user_sample_wave (DDP_USER_SAMPLE_WAVE)
    const char *sample_name = nullptr;
    int sample_per = 0;                                          // samples per work-group of `sample`
    hipFunction_t rollfit = nullptr;                             // ddp_user_rollout_fit (DDP_USER_FITTED) or ddp_user_rollout_fit_wave (DDP_USER_FITTED_WAVE)
    const char *rollfit_name = nullptr;
    hipFunction_t costfit = nullptr;                             // ddp_user_cost_fit (DDP_USER_COST_FIT)
    hipFunction_t con = nullptr, alup = nullptr;                 // ddp_user_constraints, ddp_user_al_update (DDP_USER_CONSTRAINTS)
    const char *df_name = nullptr;                               // ddp_user_df, ddp_user_df_ad (DDP_USER_AUTODIFF) or ddp_user_df_wave (+ DDP_USER_WAVE)
    const char *roll_name = nullptr;                             // ddp_user_rollout, or ddp_user_rollout_wave (DDP_USER_WAVE)
    Layout L{};
};
struct Cache { std::map<std::string, Module> mods; };

// DDP_USER_CONSTRAINTS: the parameter block of trajectory b, [user params | μ_b | the bits of the pointer to λ[:, :, b]] (user_constraints.h).
// mu == NULL: μ = 0 and a null pointer, which the model never dereferences.  lam_stride = nc · N doubles per trajectory.
__global__ void al_block_kernel(int B, int np, int batched, const double *params, const double *mu, const double *lam, size_t lam_stride,
                                double *blk)
{
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    double *o = blk + (size_t)(np + 2) * b;
    for (int e = 0; e < np; ++e) o[e] = params[batched ? (size_t)np * b + e : (size_t)e];
    const bool on = mu && lam;
    o[np] = on ? mu[b] : 0.0;
    const double *q = on ? lam + lam_stride * b : nullptr;
    double bits;
    memcpy(&bits, &q, sizeof bits);                              // a plain 8-byte move: the bits of the pointer are preserved
    o[np + 1] = bits;
}

__global__ void al_fill_kernel(int B, double v, double *mu, int32_t *live)
{
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    if (mu) mu[b] = v;
    live[b] = 1;
}

// the rows of the trajectories that are still live, from the arrays a later round was solved into, to the caller's arrays: one
// work-group per (trajectory, array); a frozen trajectory keeps the outputs of the round it froze in
struct AlMerge { const double *src[9]; double *dst[9]; size_t per[9]; };
__global__ void al_merge_kernel(AlMerge a, const int32_t *live)
{
    const int b = blockIdx.x, k = blockIdx.y;
    if (live[b] == 0) return;
    const size_t per = a.per[k];
    const double *s = a.src[k] + per * b;
    double *d = a.dst[k] + per * b;
    for (size_t e = threadIdx.x; e < per; e += blockDim.x) d[e] = s[e];
}

}   // namespace

struct UserProblem final : ddp_family {
    ddp_handle h;
    int nparam, flags;
    unsigned wrap;
    const Module *mod;
    // per call (ddp_user_ilqg_*): the parameters
    const double *params = nullptr;
    int params_batched = 0;
    // DDP_USER_SECOND_ORDER_WAVE: H_i of the step in flight, [n+m, n+m] per trajectory (ddp_user_back_pass2_wave); grown on demand
    mutable DevBuf curv;
    // DDP_USER_CLOCK: the clocks ddp_user_set_t0 gave (none: all 0, one: every trajectory's), and their device copy for the batch of
    // the last call (t0 of ddp_family points at it)
    std::vector<int32_t> t0_host;
    DevBuf t0_dev;
    int t0_count = 0;                                            // entries of t0_dev that are valid (0: to be written)
    // DDP_USER_CONSTRAINTS: nc, the multipliers ddp_user_set_multipliers gave (device copies the problem owns; none: μ = 0), the ones an
    // augmented-Lagrangian loop works on for the time of its call (al_lam, al_mu: the caller's arrays), and the parameter block of the
    // last call.  The block is written again by every bind(), from pointers that are valid then: none outlives its array.
    int nc = 0;
    DevBuf lam_dev, mu_dev;
    int lam_N = 0, lam_B = 0;
    const double *al_lam = nullptr, *al_mu = nullptr;
    DevBuf blk;
    // ddp_user_ilqg_al_*: the arrays later rounds are solved into, the live flags and the counter
    DevBuf al_ws;
    // ddp_user_sample_*: the noise factors L[m,m,N,B] of the last call
    DevBuf chol;

    int df(ddp_handle hh, int Bc, const int32_t *map, const double *x, const double *u, const int32_t *active, double *fx, double *fu,
           double *cx, double *cu, double *cxx, double *cxu, double *cuu) const override
    {
        UserDfArgs a;
        a.N = N; a.B = Bc; a.params_batched = params_batched; a.pad_ = 0;
        a.params = params; a.x = x; a.u = u; a.active = active; a.map = map;
        a.fx = fx; a.fu = fu; a.cx = cx; a.cu = cu; a.cxx = cxx; a.cxu = cxu; a.cuu = cuu; a.clk = clk;
        void *args[] = {&a};
        const long R = (long)N * Bc;
        DDP_HIP(hipModuleLaunchKernel(mod->df, (unsigned)((R + mod->L.dflanes - 1) / mod->L.dflanes), 1, 1, 64, 1, 1, 0, hh->stream, args, nullptr));
        hh->last_kernel[2] = mod->df_name;
        return 0;
    }
    int hessians(ddp_handle hh, int Bc, const int32_t *map, const int32_t *active, double *cxx, double *cxu, double *cuu) const override
    {
        DDP_CHECK(mod->hess, "user problem: compiled without DDP_USER_CONST_HESSIAN");
        UserHessArgs a;
        a.B = Bc; a.params_batched = params_batched; a.params = params; a.map = map; a.active = active; a.cxx = cxx; a.cxu = cxu; a.cuu = cuu;
        void *args[] = {&a};
        DDP_HIP(hipModuleLaunchKernel(mod->hess, (unsigned)((Bc + 63) / 64), 1, 1, 64, 1, 1, 0, hh->stream, args, nullptr));
        hh->last_kernel[2] = "ddp_user_hessians";
        return 0;
    }
    int rollout(ddp_handle hh, int Bc, const int32_t *map, const double *K, const double *k, const double *x0, const double *u, const double *x,
                const double *alpha, int nalpha, const double *lims, const int32_t *active, double *xnew, double *unew, double *cnew,
                double *csum) const override
    {
        DDP_CHECK(nalpha >= 1 && nalpha <= 16, "forward_pass: nalpha=%d out of [1,16]", nalpha);
        DDP_CHECK((K == nullptr) == (k == nullptr), "forward_pass: K and k must both be given or both NULL");
        DDP_CHECK(!K || x, "forward_pass: a non-empty policy needs the nominal trajectory x");
        if (fit_fx) {                                            // the fitted model of the call in place of `dynamics` (FitScope)
            DDP_CHECK(mod->rollfit, "forward_pass: the problem was made without DDP_USER_FITTED (a DDP_USER_WAVE problem: without DDP_USER_FITTED_WAVE)");
            UserRollFitArgs a;
            a.N = N; a.B = Bc; a.nalpha = nalpha; a.has_policy = K != nullptr; a.has_lims = lims != nullptr; a.params_batched = params_batched;
            a.params = params; a.K = K; a.k = k; a.x0 = x0; a.u = u; a.x = x; a.lims = lims; a.active = active; a.map = map;
            a.xnew = xnew; a.unew = unew; a.cnew = cnew; a.csum = csum; a.fx = fit_fx; a.fu = fit_fu; a.fc = fit_fc;
            for (int i = 0; i < 16; ++i) a.alpha[i] = i < nalpha ? alpha[i] : 0.0;
            void *args[] = {&a};
            const long total = (long)Bc * nalpha;
            DDP_HIP(hipModuleLaunchKernel(mod->rollfit, (unsigned)((total + mod->L.flanes - 1) / mod->L.flanes), 1, 1, 64, 1, 1, 0, hh->stream,
                                          args, nullptr));
            hh->last_kernel[1] = mod->rollfit_name;
            return 0;
        }
        UserRollArgs a;
        a.N = N; a.B = Bc; a.nalpha = nalpha; a.has_policy = K != nullptr; a.has_lims = lims != nullptr; a.params_batched = params_batched;
        a.params = params; a.K = K; a.k = k; a.x0 = x0; a.u = u; a.x = x; a.lims = lims; a.active = active; a.map = map;
        a.xnew = xnew; a.unew = unew; a.cnew = cnew; a.csum = csum; a.clk = clk;
        for (int i = 0; i < 16; ++i) a.alpha[i] = i < nalpha ? alpha[i] : 0.0;
        void *args[] = {&a};
        const long total = (long)Bc * nalpha;
        DDP_HIP(hipModuleLaunchKernel(mod->roll, (unsigned)((total + mod->L.rlanes - 1) / mod->L.rlanes), 1, 1, 64, 1, 1, 0, hh->stream, args,
                                      nullptr));
        hh->last_kernel[1] = mod->roll_name;
        return 0;
    }
    int costfun(ddp_handle hh, int Bc, const int32_t *map, const double *x, const double *u, const int32_t *active, double *cost,
                double *csum) const override
    {
        UserCostArgs a;
        a.N = N; a.B = Bc; a.params_batched = params_batched; a.pad_ = 0;
        a.params = params; a.x = x; a.u = u; a.active = active; a.map = map; a.cost = cost; a.csum = csum; a.clk = clk;
        void *args[] = {&a};
        DDP_HIP(hipModuleLaunchKernel(mod->cost, (unsigned)Bc, 1, 1, 64, 1, 1, 0, hh->stream, args, nullptr));
        hh->last_kernel[3] = "ddp_user_cost";
        return 0;
    }
    int plant(ddp_handle hh, int S, int steps, const int32_t *adv, const int32_t *advp, const int32_t *map, const double *ucl, double *xcl,
              double *x0s) const override
    {
        DDP_CHECK(mod->plant, "user problem: compiled without DDP_USER_PLANT");
        UserPlantArgs a;
        a.S = S; a.steps = steps; a.params_batched = params_batched; a.pad_ = 0;
        a.params = params; a.ucl = ucl; a.adv = adv; a.advp = advp; a.map = map; a.xcl = xcl; a.x0s = x0s;
        a.clk = t0;                                              // (per trajectory: the slot's clock has moved on to the next solve)
        void *args[] = {&a};
        DDP_HIP(hipModuleLaunchKernel(mod->plant, (unsigned)((S + 63) / 64), 1, 1, 64, 1, 1, 0, hh->stream, args, nullptr));
        hh->last_kernel[4] = "ddp_user_plant";
        return 0;
    }
    // DDP_USER_SECOND_ORDER: the backward pass with the curvature of the dynamics (ddp_user_back_pass2); c.x and c.map are read
    int back_pass(ddp_handle hh, const BPCall &c) const override
    {
        DDP_CHECK(mod->bp2 || mod->bp2w, "user problem: compiled without DDP_USER_SECOND_ORDER");
        const ddp_bp_desc &d = c.d;
        DDP_CHECK(d.n == n && d.m == m && d.N == N && d.B >= 1, "back_pass: sizes n=%d m=%d N=%d B=%d do not match the problem", d.n, d.m, d.N, d.B);
        DDP_CHECK(d.regType == 1 || d.regType == 2, "back_pass: regType must be 1 or 2 (got %d)", d.regType);
        DDP_CHECK(d.fx_tv && d.fx_batched && d.cost_batched && (d.cost_tv != 0) == !const_hessian,
                  "back_pass: a second-order pass takes the derivative arrays as ddp_user_df writes them");
        DDP_CHECK(c.x && c.u, "back_pass: a second-order pass needs x and u");
        DDP_CHECK(!d.has_lims || c.lims, "back_pass: has_lims needs lims");
        if (mod->bp2w) {                                         // DDP_USER_SECOND_ORDER_WAVE: the wide kernel's step, one work-group per trajectory
            const int rc = curv.reserve(hh->stream, (size_t)(n + m) * (n + m) * sizeof(double) * (size_t)d.B);
            if (rc) return rc;
            UserBp2WaveArgs w;
            bpw_fill(w.w, c);
            w.params = params; w.x = c.x; w.H = curv.as<double>(); w.map = c.map; w.params_batched = params_batched; w.pad_ = 0;
            void *wargs[] = {&w};
            DDP_HIP(hipModuleLaunchKernel(mod->bp2w, (unsigned)d.B, 1, 1, WT, 1, 1, 0, hh->stream, wargs, nullptr));
            hh->last_kernel[0] = "ddp_user_back_pass2_wave";
            return 0;
        }
        UserBp2Args a;
        a.N = N; a.B = d.B; a.regType = d.regType; a.has_lims = d.has_lims; a.params_batched = params_batched; a.pad_ = 0;
        a.params = params; a.x = c.x; a.u = c.u; a.cx = c.cx; a.cu = c.cu; a.cxx = c.cxx; a.cxu = c.cxu; a.cuu = c.cuu; a.fx = c.fx; a.fu = c.fu;
        a.lambda = c.lambda; a.lims = c.lims; a.active = c.active; a.map = c.map;
        a.K = c.K; a.k = c.k; a.Quu = c.Quu; a.Vx = c.Vx; a.Vxx = c.Vxx; a.dV = c.dV; a.diverge = c.diverge;
        void *args[] = {&a};
        DDP_HIP(hipModuleLaunchKernel(mod->bp2, (unsigned)d.B, 1, 1, 64, 1, 1, 0, hh->stream, args, nullptr));
        hh->last_kernel[0] = "ddp_user_back_pass2";
        return 0;
    }
};

void ddp_user_release(ddp_handle h)
{
    if (!h || !h->user_cache) return;
    Cache *c = (Cache *)h->user_cache;
    for (auto &kv : c->mods)
        if (kv.second.mod) hipModuleUnload(kv.second.mod);
    delete c;
    h->user_cache = nullptr;
}

namespace {

UserProblem *as_problem(ddp_handle h, void *up)
{
    UserProblem *P = (UserProblem *)up;
    if (!P) { ddp_set_error("user problem: null problem"); return nullptr; }
    if (P->h != h) { ddp_set_error("user problem: used with a handle other than the one it was created on"); return nullptr; }
    return P;
}

// where the `params` of a call live: a host-pointer flavour binds the caller's array (ON_HOST), its `_dev` twin the device copy
enum ParamsOn { ON_HOST, ON_DEVICE };

// sizes and parameters of one call
int bind(UserProblem *P, int N, int B, const double *params, int params_batched, ParamsOn on)
{
    DDP_CHECK(N >= 1 && B >= 1, "user problem: N = %d, B = %d (both >= 1)", N, B);
    DDP_CHECK(params_batched == 0 || params_batched == 1, "user problem: params_batched = %d (0 or 1)", params_batched);
    DDP_CHECK(P->nparam == 0 || params, "user problem: nparam = %d but params is NULL", P->nparam);
    P->N = N; P->B = B; P->CL = (P->flags & DDP_USER_TERMINAL) ? N + 1 : N;
    P->params = P->nparam ? params : nullptr; P->params_batched = params_batched;
    P->has_plant = false;
    P->t0 = P->clk = nullptr;
    if (P->flags & DDP_USER_CONSTRAINTS) {
        // the multipliers of ddp_user_set_multipliers belong to one (N, B); an augmented-Lagrangian loop brings its own for its call
        const bool loop = P->al_lam != nullptr;
        DDP_CHECK(loop || !P->lam_dev.ptr || (P->lam_N == N && P->lam_B == B),
                  "user problem: ddp_user_set_multipliers gave lambda[%d, N = %d, B = %d], the call has N = %d, B = %d", P->nc, P->lam_N,
                  P->lam_B, N, B);
        if (on != ON_DEVICE) return 0;                           // (a host-pointer flavour: its `_dev` twin binds the device copy)
        const int rc = P->blk.reserve(P->h->stream, (size_t)(P->nparam + 2) * B * sizeof(double));
        if (rc) return rc;
        const double *lam = loop ? P->al_lam : P->lam_dev.as<double>(), *mu = loop ? P->al_mu : P->mu_dev.as<double>();
        hipLaunchKernelGGL(al_block_kernel, dim3((unsigned)((B + 255) / 256)), dim3(256), 0, P->h->stream, B, P->nparam, params_batched,
                           P->params, mu, lam, (size_t)P->nc * N, P->blk.as<double>());
        DDP_HIP(hipGetLastError());
        P->params = P->blk.as<double>(); P->params_batched = 1;
    }
    if (!(P->flags & DDP_USER_CLOCK)) return 0;
    // DDP_USER_CLOCK: one clock per trajectory (problem) of this call on the device, written when the batch or the clocks have changed
    const int count = (int)P->t0_host.size();
    DDP_CHECK(count <= 1 || count == B, "user problem: ddp_user_set_t0 gave %d clocks, the call has %d trajectories (1 or %d are taken)",
              count, B, B);
    if (P->t0_count != B) {
        P->t0_count = 0;
        if (P->t0_dev.ptr) DDP_HIP(hipStreamSynchronize(P->h->stream));      // (the rewrite without growth: kernels in flight may still read the clocks)
        const int rc = P->t0_dev.reserve(P->h->stream, (size_t)B * sizeof(int32_t));
        if (rc) return rc;
        std::vector<int32_t> t(B, count == 1 ? P->t0_host[0] : 0);
        if (count == B) t = P->t0_host;
        DDP_HIP(hipMemcpy(P->t0_dev.ptr, t.data(), (size_t)B * sizeof(int32_t), hipMemcpyHostToDevice));
        P->t0_count = B;
    }
    P->t0 = P->clk = P->t0_dev.as<int32_t>();
    return 0;
}

// what every ddp_user_* entry does first: the handle's device made current, the problem checked against the handle, the sizes and
// parameters of the call bound.  A host-pointer flavour binds twice, here (it needs CL to size its staging) and in its `_dev` twin (the three
// ddp_user_ilqgkl*: in their staging body, ilqgkl_host), with the device copy of the parameters; the second bind finds t0_count == B and leaves the clocks on the device alone.
// DDP_USER_CONSTRAINTS: ON_DEVICE says that params is a device pointer (the `_dev` entries that take such a problem: the parameter block
// is assembled from it); `deferred` names an entry that refuses such a problem.
int enter(ddp_handle h, void *up, int N, int B, const double *params, int params_batched, UserProblem **P, ParamsOn on = ON_HOST,
          const char *deferred = nullptr)
{
    DDP_DEVICE(h);
    *P = as_problem(h, up);
    if (!*P) return -1;
    DDP_CHECK(!deferred || !((*P)->flags & DDP_USER_CONSTRAINTS), "%s: a DDP_USER_CONSTRAINTS problem is refused (deferred: constraints run "
                                                                  "through ddp_user_ilqg_* and ddp_user_ilqg_al_* only)", deferred);
    return bind(*P, N, B, params, params_batched, on);
}

// A host-pointer flavour stages its arguments IN PLACE: S.in(&x, x, count) registers the caller's array and, once S.commit() has run, the
// argument itself is the device copy, so the `_dev` twin is called with the names of the signature.
// The parameters: nparam numbers, per trajectory if `batched`
void stage_params(Staging &S, const UserProblem *P, const double **params, int batched, int B)
{
    S.in(params, *params, (size_t)P->nparam * (batched ? B : 1));
}

// the nine arrays a solve returns, as outputs of S, for B trajectories of the bound horizon
void stage_solution(Staging &S, const UserProblem *P, int B, double **x, double **u, double **K, double **k, double **Quu, double **Vx,
                    double **Vxx, double **cost, double **stats)
{
    const size_t n = P->n, m = P->m, T = (size_t)P->N * B;
    S.out(x, *x, n * T); S.out(u, *u, m * T); S.out(K, *K, m * n * T); S.out(k, *k, m * T); S.out(Quu, *Quu, m * m * T);
    S.out(Vx, *Vx, n * T); S.out(Vxx, *Vxx, n * n * T); S.out(cost, *cost, (size_t)P->CL * B); S.out(stats, *stats, (size_t)DDP_ILQG_NSTATS * B);
}

}   // namespace

extern "C" {

static int user_create(ddp_handle h, const char *source, int n, int m, int nparam, int nc, int flags, int diff_wrap, void **out)
{
    DDP_DEVICE(h);
    DDP_CHECK(out, "user problem: null output");
    *out = nullptr;
    const unsigned wrap = (unsigned)diff_wrap;
    int rc = user_program::validate(source, n, m, nparam, flags, wrap, nc);
    if (rc) return rc;
    char key_head[96];
    if (nc > 0) snprintf(key_head, sizeof key_head, "%d,%d,%d,%d,%x,c%d\n", n, m, nparam, flags, wrap, nc);
    else snprintf(key_head, sizeof key_head, "%d,%d,%d,%d,%x\n", n, m, nparam, flags, wrap);
    const std::string key = std::string(key_head) + source;
    if (!h->user_cache) h->user_cache = new Cache();
    Cache *c = (Cache *)h->user_cache;
    auto it = c->mods.find(key);
    if (it == c->mods.end()) {
        std::vector<char> code;
        rc = user_program::compile(source, n, m, nparam, flags, wrap, nullptr, &code, nc);
        if (rc) return rc;
        Module M;
        M.L = user_program::layout_of(n, m, flags);
        const bool wave = (flags & DDP_USER_WAVE) != 0;
        M.df_name = (flags & DDP_USER_AUTODIFF) ? (wave ? "ddp_user_df_wave" : "ddp_user_df_ad") : "ddp_user_df";
        M.roll_name = wave ? "ddp_user_rollout_wave" : "ddp_user_rollout";
        M.sample_name = (flags & DDP_USER_SAMPLE_WAVE) ? "ddp_user_sample_wave" : "ddp_user_sample";
        M.sample_per = (flags & DDP_USER_SAMPLE_WAVE) ? 64 / M.L.wg : M.L.slanes;
        M.rollfit_name = (flags & DDP_USER_FITTED_WAVE) ? "ddp_user_rollout_fit_wave" : "ddp_user_rollout_fit";
        DDP_HIP(hipModuleLoadData(&M.mod, code.data()));
        // the kernels of the program: mask 0 = every program has it, else the flags (any of them) whose programs do
        const struct { int mask; const char *name; hipFunction_t Module::*fn; } kernels[] = {
            {0, M.roll_name, &Module::roll}, {0, M.df_name, &Module::df}, {0, "ddp_user_cost", &Module::cost},
            {DDP_USER_CONST_HESSIAN, "ddp_user_hessians", &Module::hess}, {DDP_USER_PLANT, "ddp_user_plant", &Module::plant},
            {DDP_USER_SECOND_ORDER, "ddp_user_back_pass2", &Module::bp2},
            {DDP_USER_SECOND_ORDER_WAVE, "ddp_user_back_pass2_wave", &Module::bp2w},
            {DDP_USER_SECOND_ORDER | DDP_USER_SECOND_ORDER_WAVE, "ddp_user_vhess", &Module::vhess},
            {DDP_USER_CONSTRAINTS, "ddp_user_constraints", &Module::con}, {DDP_USER_CONSTRAINTS, "ddp_user_al_update", &Module::alup},
            {DDP_USER_SAMPLE | DDP_USER_SAMPLE_WAVE, M.sample_name, &Module::sample},
            {DDP_USER_FITTED | DDP_USER_FITTED_WAVE, M.rollfit_name, &Module::rollfit},
            {DDP_USER_COST_FIT, "ddp_user_cost_fit", &Module::costfit}};
        bool ok = true;
        for (const auto &k : kernels)
            if (ok && (k.mask == 0 || (flags & k.mask))) ok = hipModuleGetFunction(&(M.*k.fn), M.mod, k.name) == hipSuccess;
        if (!ok) {
            hipModuleUnload(M.mod);
            ddp_set_error("user problem: a kernel of the compiled program is missing");
            return -4;
        }
        it = c->mods.emplace(key, M).first;
    }
    UserProblem *P = new UserProblem();
    P->h = h; P->n = n; P->m = m; P->N = 0; P->B = 0; P->CL = 0; P->const_hessian = (flags & DDP_USER_CONST_HESSIAN) != 0;
    P->has_plant = false;                                        // set by the closed-loop entry points only
    P->second_order = (flags & (DDP_USER_SECOND_ORDER | DDP_USER_SECOND_ORDER_WAVE)) != 0;
    P->nparam = nparam; P->flags = flags; P->wrap = wrap; P->mod = &it->second;
    P->nc = nc > 0 ? nc : 0;
    *out = P;
    return 0;
}

int ddp_user_create(ddp_handle h, const char *source, int n, int m, int nparam, int flags, int diff_wrap, void **out)
{
    return user_create(h, source, n, m, nparam, -1, flags, diff_wrap, out);
}

int ddp_user_create_c(ddp_handle h, const char *source, int n, int m, int nparam, int nc, int flags, int diff_wrap, void **out)
{
    DDP_CHECK(nc >= 0, "user problem: nc = %d (>= 0)", nc);
    return user_create(h, source, n, m, nparam, nc, flags, diff_wrap, out);
}

int ddp_user_destroy(void *up)
{
    delete (UserProblem *)up;
    return 0;
}

int ddp_user_set_t0(void *up, const int32_t *t0, int count)
{
    UserProblem *P = (UserProblem *)up;
    DDP_CHECK(P, "user problem: null problem");
    DDP_CHECK(P->flags & DDP_USER_CLOCK, "set_t0: the problem was made without DDP_USER_CLOCK");
    DDP_CHECK(count >= 0 && (count == 0 || t0), "set_t0: count = %d, t0 = %s", count, t0 ? "given" : "NULL");
    P->t0_host.assign(t0, t0 + count);
    P->t0_count = 0;                                             // the device copy is written by the next call, for its batch
    return 0;
}

int ddp_user_df_f64_dev(ddp_handle h, void *up, int N, int B, const double *params, int params_batched, const double *x, const double *u,
                        const int32_t *active, double *fx, double *fu, double *cx, double *cu, double *cxx, double *cxu, double *cuu)
{
    UserProblem *P;
    int rc = enter(h, up, N, B, params, params_batched, &P, ON_DEVICE);
    if (rc) return rc;
    DDP_CHECK(x && u && fx && fu && cx && cu, "df: null argument");
    rc = P->df(h, B, nullptr, x, u, active, fx, fu, cx, cu, P->const_hessian ? nullptr : cxx, P->const_hessian ? nullptr : cxu,
               P->const_hessian ? nullptr : cuu);
    if (rc) return rc;
    if (P->const_hessian && cxx && cxu && cuu) return P->hessians(h, B, nullptr, active, cxx, cxu, cuu);
    return 0;
}

int ddp_user_df_f64(ddp_handle h, void *up, int N, int B, const double *params, int params_batched, const double *x, const double *u,
                    double *fx, double *fu, double *cx, double *cu, double *cxx, double *cxu, double *cuu)
{
    UserProblem *P;
    int rc = enter(h, up, N, B, params, params_batched, &P);
    if (rc) return rc;
    DDP_CHECK(x && u && fx && fu && cx && cu, "df: null argument");
    const size_t n = P->n, m = P->m, T = (size_t)N * B, HT = P->const_hessian ? (size_t)B : T;
    Staging S(h, Staging::OWNED, "user problem");
    stage_params(S, P, &params, params_batched, B); S.in(&x, x, n * T); S.in(&u, u, m * T);
    S.out(&fx, fx, n * n * T); S.out(&fu, fu, n * m * T); S.out(&cx, cx, n * T); S.out(&cu, cu, m * T); S.out(&cxx, cxx, n * n * HT);
    S.out(&cxu, cxu, n * m * HT); S.out(&cuu, cuu, m * m * HT);
    if ((rc = S.commit())) return rc;
    return S.finish(ddp_user_df_f64_dev(h, up, N, B, params, params_batched, x, u, nullptr, fx, fu, cx, cu, cxx, cxu, cuu));
}

int ddp_user_vhess_f64_dev(ddp_handle h, void *up, int N, int B, const double *params, int params_batched, const double *x, const double *u,
                           const double *v, const int32_t *active, double *H)
{
    UserProblem *P;
    int rc = enter(h, up, N, B, params, params_batched, &P);
    if (rc) return rc;
    DDP_CHECK(P->mod->vhess, "vhess: the problem was made without DDP_USER_SECOND_ORDER");
    DDP_CHECK(x && u && v && H, "vhess: null argument");
    UserVhessArgs a;
    a.N = N; a.B = B; a.params_batched = P->params_batched; a.pad_ = 0;
    a.params = P->params; a.x = x; a.u = u; a.v = v; a.active = active; a.map = nullptr; a.H = H;
    void *args[] = {&a};
    const int nz = P->n + P->m;
    const long total = (long)(nz * (nz + 1) / 2) * N * B;
    DDP_CHECK(total <= 64L * 0x7fffffffL, "vhess: N = %d, B = %d is too large for one launch", N, B);
    DDP_HIP(hipModuleLaunchKernel(P->mod->vhess, (unsigned)((total + 63) / 64), 1, 1, 64, 1, 1, 0, h->stream, args, nullptr));
    h->last_kernel[2] = "ddp_user_vhess";
    return 0;
}

int ddp_user_vhess_f64(ddp_handle h, void *up, int N, int B, const double *params, int params_batched, const double *x, const double *u,
                       const double *v, double *H)
{
    UserProblem *P;
    int rc = enter(h, up, N, B, params, params_batched, &P);
    if (rc) return rc;
    DDP_CHECK(x && u && v && H, "vhess: null argument");
    const size_t n = P->n, m = P->m, T = (size_t)N * B;
    Staging S(h, Staging::OWNED, "user problem");
    stage_params(S, P, &params, params_batched, B); S.in(&x, x, n * T); S.in(&u, u, m * T); S.in(&v, v, n * T);
    S.out(&H, H, (n + m) * (n + m) * T);
    if ((rc = S.commit())) return rc;
    return S.finish(ddp_user_vhess_f64_dev(h, up, N, B, params, params_batched, x, u, v, nullptr, H));
}

int ddp_user_back_pass_f64_dev(ddp_handle h, void *up, int N, int B, const double *params, int params_batched, const double *x,
                               const double *u, const double *fx, const double *fu, const double *cx, const double *cu, const double *cxx,
                               const double *cxu, const double *cuu, const double *lambda, int regType, const double *lims,
                               const int32_t *active, double *K, double *k, double *Quu, double *Vx, double *Vxx, double *dV,
                               int32_t *diverge)
{
    UserProblem *P;
    int rc = enter(h, up, N, B, params, params_batched, &P);
    if (rc) return rc;
    DDP_CHECK(P->second_order, "back_pass: the problem was made without DDP_USER_SECOND_ORDER; a first-order pass is ddp_back_pass_f64 "
                               "on the arrays of ddp_user_df");
    DDP_CHECK(x && u && fx && fu && cx && cu && cxx && cxu && cuu && lambda && K && k && Quu && Vx && Vxx && dV && diverge,
              "back_pass: null argument");
    BPCall c = {};
    c.d.n = P->n; c.d.m = P->m; c.d.N = N; c.d.B = B; c.d.fx_tv = 1; c.d.fx_batched = 1; c.d.cost_tv = P->const_hessian ? 0 : 1;
    c.d.cost_batched = 1; c.d.regType = regType; c.d.has_lims = lims != nullptr;
    c.cx = cx; c.cu = cu; c.cxx = cxx; c.cxu = cxu; c.cuu = cuu; c.fx = fx; c.fu = fu; c.lambda = lambda; c.lims = lims; c.u = u; c.x = x;
    c.active = active; c.K = K; c.k = k; c.Quu = Quu; c.Vx = Vx; c.Vxx = Vxx; c.dV = dV; c.diverge = diverge;
    return P->back_pass(h, c);
}

int ddp_user_back_pass_f64(ddp_handle h, void *up, int N, int B, const double *params, int params_batched, const double *x, const double *u,
                           const double *fx, const double *fu, const double *cx, const double *cu, const double *cxx, const double *cxu,
                           const double *cuu, const double *lambda, int regType, const double *lims, double *K, double *k, double *Quu,
                           double *Vx, double *Vxx, double *dV, int32_t *diverge)
{
    UserProblem *P;
    int rc = enter(h, up, N, B, params, params_batched, &P);
    if (rc) return rc;
    DDP_CHECK(x && u && fx && fu && cx && cu && cxx && cxu && cuu && lambda && K && k && Quu && Vx && Vxx && dV && diverge,
              "back_pass: null argument");
    const size_t n = P->n, m = P->m, T = (size_t)N * B, HT = P->const_hessian ? (size_t)B : T;
    Staging S(h, Staging::OWNED, "user problem");
    stage_params(S, P, &params, params_batched, B); S.in(&x, x, n * T); S.in(&u, u, m * T); S.in(&fx, fx, n * n * T);
    S.in(&fu, fu, n * m * T); S.in(&cx, cx, n * T); S.in(&cu, cu, m * T); S.in(&cxx, cxx, n * n * HT); S.in(&cxu, cxu, n * m * HT);
    S.in(&cuu, cuu, m * m * HT); S.in(&lambda, lambda, (size_t)B); S.in(&lims, lims, 2 * m);
    S.out(&K, K, m * n * T); S.out(&k, k, m * T); S.out(&Quu, Quu, m * m * T); S.out(&Vx, Vx, n * T); S.out(&Vxx, Vxx, n * n * T);
    S.out(&dV, dV, (size_t)2 * B); S.out(&diverge, diverge, (size_t)B);
    if ((rc = S.commit())) return rc;
    return S.finish(ddp_user_back_pass_f64_dev(h, up, N, B, params, params_batched, x, u, fx, fu, cx, cu, cxx, cxu, cuu, lambda, regType, lims,
                                               nullptr, K, k, Quu, Vx, Vxx, dV, diverge));
}

int ddp_user_set_multipliers(void *up, const double *lambda, const double *mu, int N, int B)
{
    UserProblem *P = (UserProblem *)up;
    DDP_CHECK(P, "user problem: null problem");
    DDP_CHECK(P->flags & DDP_USER_CONSTRAINTS, "set_multipliers: the problem was made without DDP_USER_CONSTRAINTS");
    DDP_HIP(hipSetDevice(P->h->device));
    int rc = P->lam_dev.release(P->h->stream);                   // (kernels in flight may still read them)
    if (!rc) rc = P->mu_dev.release(P->h->stream);
    if (rc) return rc;
    P->lam_N = P->lam_B = 0;
    if (!lambda && !mu) return 0;
    DDP_CHECK(lambda && mu, "set_multipliers: lambda and mu must both be given or both NULL");
    DDP_CHECK(N >= 1 && B >= 1, "set_multipliers: N = %d, B = %d (both >= 1)", N, B);
    const size_t ln = (size_t)P->nc * N * B;
    if ((rc = P->lam_dev.reserve(P->h->stream, ln * sizeof(double)))) return rc;
    if ((rc = P->mu_dev.reserve(P->h->stream, (size_t)B * sizeof(double)))) return rc;
    DDP_HIP(hipMemcpy(P->lam_dev.ptr, lambda, ln * sizeof(double), hipMemcpyHostToDevice));
    DDP_HIP(hipMemcpy(P->mu_dev.ptr, mu, (size_t)B * sizeof(double), hipMemcpyHostToDevice));
    P->lam_N = N; P->lam_B = B;
    return 0;
}

int ddp_user_constraints_f64_dev(ddp_handle h, void *up, int N, int B, const double *params, int params_batched, const double *x,
                                 const double *u, double *g)
{
    UserProblem *P;
    int rc = enter(h, up, N, B, params, params_batched, &P, ON_DEVICE);
    if (rc) return rc;
    DDP_CHECK(P->mod->con, "constraints: the problem was made without DDP_USER_CONSTRAINTS");
    DDP_CHECK(x && u && g, "constraints: null argument");
    UserConArgs a;
    a.N = N; a.B = B; a.params = P->params; a.x = x; a.u = u; a.g = g;
    void *args[] = {&a};
    const long R = (long)N * B;
    DDP_HIP(hipModuleLaunchKernel(P->mod->con, (unsigned)((R + 63) / 64), 1, 1, 64, 1, 1, 0, h->stream, args, nullptr));
    return 0;
}

int ddp_user_constraints_f64(ddp_handle h, void *up, int N, int B, const double *params, int params_batched, const double *x,
                             const double *u, double *g)
{
    UserProblem *P;
    int rc = enter(h, up, N, B, params, params_batched, &P);
    if (rc) return rc;
    DDP_CHECK(P->mod->con, "constraints: the problem was made without DDP_USER_CONSTRAINTS");
    DDP_CHECK(x && u && g, "constraints: null argument");
    const size_t n = P->n, m = P->m, T = (size_t)N * B;
    Staging S(h, Staging::OWNED, "user problem");
    stage_params(S, P, &params, params_batched, B); S.in(&x, x, n * T); S.in(&u, u, m * T);
    S.out(&g, g, (size_t)P->nc * T);
    if ((rc = S.commit())) return rc;
    return S.finish(ddp_user_constraints_f64_dev(h, up, N, B, params, params_batched, x, u, g));
}

void ddp_al_default_opts(ddp_al_opts *o)
{
    if (!o) return;
    o->mu0 = 1.0; o->mu_factor = 10.0; o->mu_max = 1e8; o->ctol = 1e-5; o->max_outer = 20;
}

int ddp_user_ilqg_al_f64_dev(ddp_handle h, void *up, int N, int B, const double *params, int params_batched, const ddp_ilqg_opts *o,
                             const ddp_al_opts *ao, const double *x0, int x0_prerolled, const double *u0, const double *lims,
                             const double *lambda0, const double *mu_init, double *x, double *u, double *K, double *k, double *Quu,
                             double *Vx, double *Vxx, double *cost, double *stats, double *lambda, double *mu, double *g, double *al_stats,
                             int *global_iters)
{
    UserProblem *P;
    int rc = enter(h, up, N, B, params, params_batched, &P);      // (sizes only: every round binds with its multipliers, below)
    if (rc) return rc;
    DDP_CHECK(P->mod->alup, "ilqg_al: the problem was made without DDP_USER_CONSTRAINTS");
    DDP_CHECK(x0 && u0 && x && u && K && k && Quu && Vx && Vxx && cost && stats && lambda && mu && g && al_stats, "ilqg_al: null argument");
    ddp_al_opts ad;
    if (!ao) { ddp_al_default_opts(&ad); ao = &ad; }
    DDP_CHECK(ao->mu0 > 0.0 && ao->mu_factor >= 1.0 && ao->mu_max >= ao->mu0 && ao->ctol >= 0.0 && ao->max_outer >= 1,
              "ilqg_al: mu0 = %g (> 0), mu_factor = %g (>= 1), mu_max = %g (>= mu0), ctol = %g (>= 0), max_outer = %d (>= 1)", ao->mu0,
              ao->mu_factor, ao->mu_max, ao->ctol, ao->max_outer);
    const size_t n = P->n, m = P->m, T = (size_t)N * B, CL = P->CL, nc = P->nc;
    // later rounds are solved into arrays of the loop's own and the rows of the live trajectories merged into the caller's
    const size_t per[9] = {n * N, m * N, m * n * N, m * N, m * m * N, n * N, n * n * N, CL, (size_t)DDP_ILQG_NSTATS};
    size_t off[10] = {0};
    for (int e = 0; e < 9; ++e) off[e + 1] = off[e] + Staging::al(per[e] * B * sizeof(double));
    const size_t o_live = off[9], o_cnt = o_live + Staging::al((size_t)B * sizeof(int32_t)), bytes = o_cnt + 256;
    DDP_CHECK(h->h_pinned, "ilqg_al: pinned poll buffer missing");
    hipStream_t st = h->stream;
    if ((rc = P->al_ws.reserve(st, bytes))) return rc;
    char *ws = P->al_ws.as<char>();
    struct Scope {                                               // every way out: the loop's multipliers leave the problem
        UserProblem *P;
        ~Scope() { P->al_lam = P->al_mu = nullptr; }
    } scope{P};
    double *sc[9];
    for (int e = 0; e < 9; ++e) sc[e] = (double *)(ws + off[e]);
    int32_t *live = (int32_t *)(ws + o_live);
    int *counter = (int *)(ws + o_cnt);
    double *user[9] = {x, u, K, k, Quu, Vx, Vxx, cost, stats};

    if (lambda0) DDP_HIP(hipMemcpyAsync(lambda, lambda0, nc * T * sizeof(double), hipMemcpyDeviceToDevice, st));
    else DDP_HIP(hipMemsetAsync(lambda, 0, nc * T * sizeof(double), st));
    if (mu_init) DDP_HIP(hipMemcpyAsync(mu, mu_init, (size_t)B * sizeof(double), hipMemcpyDeviceToDevice, st));
    hipLaunchKernelGGL(al_fill_kernel, dim3((unsigned)((B + 255) / 256)), dim3(256), 0, st, B, ao->mu0, mu_init ? (double *)nullptr : mu, live);
    DDP_HIP(hipGetLastError());
    DDP_HIP(hipMemsetAsync(al_stats, 0, (size_t)6 * B * sizeof(double), st));

    int total = 0;
    for (int r = 0; r < ao->max_outer; ++r) {
        P->al_lam = lambda; P->al_mu = mu;
        rc = bind(P, N, B, params, params_batched, ON_DEVICE);        // the block of this round: μ and the pointers to λ as they stand now
        if (rc) return rc;
        double **out = r == 0 ? user : sc;
        int git = 0;
        // round 0: the caller's start; later rounds: pre-rolled from the last solution, its cost evaluated again under the new multipliers
        rc = ddp_ilqg_family_dev(h, P, o, r == 0 ? x0 : x, r == 0 ? x0_prerolled : 1, r == 0 ? u0 : u, nullptr, lims, out[0], out[1], out[2],
                                 out[3], out[4], out[5], out[6], out[7], out[8], 0, nullptr, &git);
        if (rc) return rc;
        total += git;
        if (r > 0) {
            AlMerge mg;
            for (int e = 0; e < 9; ++e) { mg.src[e] = sc[e]; mg.dst[e] = user[e]; mg.per[e] = per[e]; }
            hipLaunchKernelGGL(al_merge_kernel, dim3((unsigned)B, 9), dim3(256), 0, st, mg, (const int32_t *)live);
            DDP_HIP(hipGetLastError());
        }
        DDP_HIP(hipMemsetAsync(counter, 0, sizeof(int), st));
        UserAlArgs a;
        a.N = N; a.B = B; a.round = r; a.max_outer = ao->max_outer; a.mu_factor = ao->mu_factor; a.mu_max = ao->mu_max; a.ctol = ao->ctol;
        a.params = P->params; a.x = x; a.u = u; a.stats = stats; a.lambda = lambda; a.mu = mu; a.g = g; a.al_stats = al_stats;
        a.live = live; a.counter = counter;
        void *args[] = {&a};
        DDP_HIP(hipModuleLaunchKernel(P->mod->alup, (unsigned)B, 1, 1, 64, 1, 1, 0, st, args, nullptr));
        DDP_HIP(hipMemcpyAsync(h->h_pinned, counter, sizeof(int), hipMemcpyDeviceToHost, st));
        DDP_HIP(hipStreamSynchronize(st));
        if (h->h_pinned[0] == 0) break;                          // the one number the host reads per round: trajectories still live
    }
    if (global_iters) *global_iters = total;
    return 0;
}

int ddp_user_ilqg_al_f64(ddp_handle h, void *up, int N, int B, const double *params, int params_batched, const ddp_ilqg_opts *o,
                         const ddp_al_opts *ao, const double *x0, int x0_prerolled, const double *u0, const double *lims,
                         const double *lambda0, const double *mu_init, double *x, double *u, double *K, double *k, double *Quu,
                         double *Vx, double *Vxx, double *cost, double *stats, double *lambda, double *mu, double *g, double *al_stats,
                         int *global_iters)
{
    UserProblem *P;
    int rc = enter(h, up, N, B, params, params_batched, &P);
    if (rc) return rc;
    DDP_CHECK(P->mod->alup, "ilqg_al: the problem was made without DDP_USER_CONSTRAINTS");
    DDP_CHECK(x0 && u0 && x && u && K && k && Quu && Vx && Vxx && cost && stats && lambda && mu && g && al_stats, "ilqg_al: null argument");
    const size_t n = P->n, m = P->m, T = (size_t)N * B, nc = P->nc;
    Staging S(h, Staging::OWNED, "user problem");
    stage_params(S, P, &params, params_batched, B); S.in(&x0, x0, n * (x0_prerolled ? T : (size_t)B)); S.in(&u0, u0, m * T);
    S.in(&lims, lims, 2 * m); S.in(&lambda0, lambda0, nc * T); S.in(&mu_init, mu_init, (size_t)B);
    stage_solution(S, P, B, &x, &u, &K, &k, &Quu, &Vx, &Vxx, &cost, &stats);
    S.out(&lambda, lambda, nc * T); S.out(&mu, mu, (size_t)B); S.out(&g, g, nc * T); S.out(&al_stats, al_stats, (size_t)6 * B);
    if ((rc = S.commit())) return rc;
    return S.finish(ddp_user_ilqg_al_f64_dev(h, up, N, B, params, params_batched, o, ao, x0, x0_prerolled, u0, lims, lambda0, mu_init, x, u, K,
                                             k, Quu, Vx, Vxx, cost, stats, lambda, mu, g, al_stats, global_iters));
}

int ddp_user_costfun_f64_dev(ddp_handle h, void *up, int N, int B, const double *params, int params_batched, const double *x,
                             const double *u, const int32_t *active, double *cost, double *csum)
{
    UserProblem *P;
    int rc = enter(h, up, N, B, params, params_batched, &P, ON_DEVICE);
    if (rc) return rc;
    DDP_CHECK(x && u && cost, "costfun: null argument");
    return P->costfun(h, B, nullptr, x, u, active, cost, csum);
}

int ddp_user_costfun_f64(ddp_handle h, void *up, int N, int B, const double *params, int params_batched, const double *x,
                         const double *u, double *cost, double *csum)
{
    UserProblem *P;
    int rc = enter(h, up, N, B, params, params_batched, &P);
    if (rc) return rc;
    DDP_CHECK(x && u && cost, "costfun: null argument");
    const size_t n = P->n, m = P->m, T = (size_t)N * B;
    Staging S(h, Staging::OWNED, "user problem");
    stage_params(S, P, &params, params_batched, B); S.in(&x, x, n * T); S.in(&u, u, m * T);
    S.out(&cost, cost, (size_t)P->CL * B); S.out(&csum, csum, (size_t)B);
    if ((rc = S.commit())) return rc;
    return S.finish(ddp_user_costfun_f64_dev(h, up, N, B, params, params_batched, x, u, nullptr, cost, csum));
}

int ddp_user_ilqg_f64_dev(ddp_handle h, void *up, int N, int B, const double *params, int params_batched, const ddp_ilqg_opts *o,
                          const double *x0, int x0_prerolled, const double *u0, const double *cost0, const double *lims,
                          double *x, double *u, double *K, double *k, double *Quu, double *Vx, double *Vxx,
                          double *cost, double *stats, int trace_cap, double *trace7, int *global_iters)
{
    UserProblem *P;
    int rc = enter(h, up, N, B, params, params_batched, &P, ON_DEVICE);
    if (rc) return rc;
    return ddp_ilqg_family_dev(h, P, o, x0, x0_prerolled, u0, cost0, lims, x, u, K, k, Quu, Vx, Vxx, cost, stats, trace_cap, trace7,
                               global_iters);
}

int ddp_user_ilqg_f64(ddp_handle h, void *up, int N, int B, const double *params, int params_batched, const ddp_ilqg_opts *o,
                      const double *x0, int x0_prerolled, const double *u0, const double *cost0, const double *lims,
                      double *x, double *u, double *K, double *k, double *Quu, double *Vx, double *Vxx,
                      double *cost, double *stats, int trace_cap, double *trace7, int *global_iters)
{
    UserProblem *P;
    int rc = enter(h, up, N, B, params, params_batched, &P);
    if (rc) return rc;
    DDP_CHECK(x0 && u0 && x && u && K && k && Quu && Vx && Vxx && cost && stats, "ilqg: null argument");
    const size_t n = P->n, m = P->m, T = (size_t)N * B, CL = P->CL;
    Staging S(h, Staging::OWNED, "user problem");
    stage_params(S, P, &params, params_batched, B); S.in(&x0, x0, n * (x0_prerolled ? T : (size_t)B)); S.in(&u0, u0, m * T);
    S.in(&cost0, x0_prerolled ? cost0 : nullptr, CL * B); S.in(&lims, lims, 2 * m);
    stage_solution(S, P, B, &x, &u, &K, &k, &Quu, &Vx, &Vxx, &cost, &stats);
    S.out(&trace7, trace_cap > 0 ? trace7 : nullptr, (size_t)7 * trace_cap * B);
    if ((rc = S.commit())) return rc;
    return S.finish(ddp_user_ilqg_f64_dev(h, up, N, B, params, params_batched, o, x0, x0_prerolled, u0, cost0, lims, x, u, K, k, Quu, Vx, Vxx,
                                          cost, stats, trace_cap, trace7, global_iters));
}

int ddp_user_ilqg_queue_f64_dev(ddp_handle h, void *up, int N, int P, const double *params, int params_batched, const ddp_ilqg_opts *o,
                                int slots, const double *x0, const double *u0, const double *lims, double *x, double *u, double *K, double *k,
                                double *Quu, double *Vx, double *Vxx, double *cost, double *stats, int *global_iters)
{
    UserProblem *U;
    int rc = enter(h, up, N, P, params, params_batched, &U, ON_HOST, "ilqg_queue");
    if (rc) return rc;
    DDP_CHECK(x0 && u0 && x && u && K && k && Quu && Vx && Vxx && cost && stats, "ilqg_queue: null argument");
    return ddp_ilqg_sched_family_dev(h, U, o, slots, 0, 0, x0, u0, lims, x, u, K, k, Quu, Vx, Vxx, cost, stats, nullptr, nullptr, nullptr,
                                     global_iters);
}

int ddp_user_ilqg_queue_f64(ddp_handle h, void *up, int N, int P, const double *params, int params_batched, const ddp_ilqg_opts *o,
                            int slots, const double *x0, const double *u0, const double *lims, double *x, double *u, double *K, double *k,
                            double *Quu, double *Vx, double *Vxx, double *cost, double *stats, int *global_iters)
{
    UserProblem *U;
    int rc = enter(h, up, N, P, params, params_batched, &U, ON_HOST, "ilqg_queue");
    if (rc) return rc;
    DDP_CHECK(x0 && u0 && x && u && K && k && Quu && Vx && Vxx && cost && stats, "ilqg_queue: null argument");
    const size_t n = U->n, m = U->m, T = (size_t)N * P;
    Staging S(h, Staging::OWNED, "user problem");
    stage_params(S, U, &params, params_batched, P); S.in(&x0, x0, n * P); S.in(&u0, u0, m * T); S.in(&lims, lims, 2 * m);
    stage_solution(S, U, P, &x, &u, &K, &k, &Quu, &Vx, &Vxx, &cost, &stats);
    if ((rc = S.commit())) return rc;
    return S.finish(ddp_user_ilqg_queue_f64_dev(h, up, N, P, params, params_batched, o, slots, x0, u0, lims, x, u, K, k, Quu, Vx, Vxx, cost,
                                                stats, global_iters));
}

int ddp_user_ilqg_mpc_f64_dev(ddp_handle h, void *up, int N, int B, const double *params, int params_batched, const ddp_ilqg_opts *o,
                              int steps, int zero_tail, const double *x0, const double *u0, const double *lims, double *xcl, double *ucl,
                              double *stats_cl, double *x, double *u, int *global_iters)
{
    UserProblem *U;
    int rc = enter(h, up, N, B, params, params_batched, &U, ON_HOST, "ilqg_mpc");
    if (rc) return rc;
    DDP_CHECK(steps >= 1, "ilqg_mpc: steps=%d", steps);
    DDP_CHECK(x0 && u0 && xcl && ucl && stats_cl && x && u, "ilqg_mpc: null argument");
    U->has_plant = (U->flags & DDP_USER_PLANT) != 0;           // the plant acts in the closed loop only
    rc = ddp_ilqg_sched_family_dev(h, U, o, 0, steps, zero_tail, x0, u0, lims, x, u, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                                   nullptr, xcl, ucl, stats_cl, global_iters);
    U->has_plant = false;
    return rc;
}

int ddp_user_ilqg_mpc_f64(ddp_handle h, void *up, int N, int B, const double *params, int params_batched, const ddp_ilqg_opts *o,
                          int steps, int zero_tail, const double *x0, const double *u0, const double *lims, double *xcl, double *ucl,
                          double *stats_cl, double *x, double *u, int *global_iters)
{
    UserProblem *U;
    int rc = enter(h, up, N, B, params, params_batched, &U, ON_HOST, "ilqg_mpc");
    if (rc) return rc;
    DDP_CHECK(steps >= 1, "ilqg_mpc: steps=%d", steps);
    DDP_CHECK(x0 && u0 && xcl && ucl && stats_cl && x && u, "ilqg_mpc: null argument");
    const size_t n = U->n, m = U->m, T = (size_t)N * B;
    Staging S(h, Staging::OWNED, "user problem");
    stage_params(S, U, &params, params_batched, B); S.in(&x0, x0, n * B); S.in(&u0, u0, m * T); S.in(&lims, lims, 2 * m);
    S.out(&xcl, xcl, n * (size_t)(steps + 1) * B); S.out(&ucl, ucl, m * (size_t)steps * B);
    S.out(&stats_cl, stats_cl, (size_t)DDP_ILQG_NSTATS * steps * B); S.out(&x, x, n * T); S.out(&u, u, m * T);
    if ((rc = S.commit())) return rc;
    return S.finish(ddp_user_ilqg_mpc_f64_dev(h, up, N, B, params, params_batched, o, steps, zero_tail, x0, u0, lims, xcl, ucl, stats_cl, x, u,
                                              global_iters));
}

// what both flavours of ddp_user_sample refuse, before anything is staged or launched
static int sample_check(const UserProblem *P, int S, const double *K, const double *x0, const double *u, const double *x, int sample0,
                        int traj0, int use_plant, const double *xs, const double *cs, const double *csum, const double *xmean,
                        const double *xcov, const int32_t *status)
{
    DDP_CHECK(P->mod->sample, "sample: the problem was made without DDP_USER_SAMPLE (a DDP_USER_WAVE problem: without DDP_USER_SAMPLE_WAVE)");
    DDP_CHECK(use_plant == 0 || use_plant == 1, "sample: use_plant = %d (0 or 1)", use_plant);
    DDP_CHECK(!use_plant || (P->flags & DDP_USER_PLANT), "sample: use_plant = 1 but the problem was made without DDP_USER_PLANT");
    DDP_CHECK(S >= 1, "sample: S = %d (>= 1)", S);
    DDP_CHECK(sample0 >= 0 && traj0 >= 0, "sample: sample0 = %d, traj0 = %d (both >= 0)", sample0, traj0);
    DDP_CHECK(K && x0 && u && x && cs && csum && status, "sample: null argument");
    DDP_CHECK(xs || (!xmean && !xcov), "sample: xmean / xcov need xs (the moments are computed from the stored samples)");
    return 0;
}

int ddp_user_sample_f64_dev(ddp_handle h, void *up, int N, int B, int S, const double *params, int params_batched, const double *K,
                            const double *Sigma, const double *x0, const double *u, const double *x, const double *lims, const double *noise,
                            int seed_lo, int seed_hi, int sample0, int traj0, int use_plant, double *xs, double *us, double *cs, double *csum,
                            double *xmean, double *xcov, int32_t *status)
{
    UserProblem *P;
    int rc = enter(h, up, N, B, params, params_batched, &P, ON_DEVICE);
    if (rc) return rc;
    if ((rc = sample_check(P, S, K, x0, u, x, sample0, traj0, use_plant, xs, cs, csum, xmean, xcov, status))) return rc;
    const int m = P->m;
    const long groups = ((long)S + P->mod->sample_per - 1) / P->mod->sample_per;
    DDP_CHECK(groups * B <= 0x7fffffffL, "sample: S = %d, B = %d is too large for one launch", S, B);
    if (Sigma) {
        if ((rc = P->chol.reserve(h->stream, (size_t)m * m * N * B * sizeof(double)))) return rc;
        if ((rc = ddp_policy_factor_dev(h, m, N, B, Sigma, P->chol.as<double>(), status))) return rc;
    } else {
        DDP_HIP(hipMemsetAsync(status, 0, (size_t)B * sizeof(int32_t), h->stream));
    }
    UserSampleArgs a;
    a.N = N; a.B = B; a.S = S; a.has_lims = lims != nullptr; a.params_batched = P->params_batched; a.use_plant = use_plant;
    a.sample0 = sample0; a.traj0 = traj0; a.seed_lo = seed_lo; a.seed_hi = seed_hi;
    a.params = P->params; a.K = K; a.L = Sigma ? P->chol.as<double>() : nullptr; a.x0 = x0; a.u = u; a.x = x; a.lims = lims;
    a.noise = Sigma ? noise : nullptr; a.status = status; a.xs = xs; a.us = us; a.cs = cs; a.csum = csum;
    void *args[] = {&a};
    DDP_HIP(hipModuleLaunchKernel(P->mod->sample, (unsigned)(groups * B), 1, 1, 64, 1, 1, 0, h->stream, args, nullptr));
    h->last_kernel[1] = P->mod->sample_name;
    if (xmean || xcov) return ddp_sample_moments_dev(h, P->n, N, S, B, xs, xmean, xcov);
    return 0;
}

int ddp_user_sample_f64(ddp_handle h, void *up, int N, int B, int S, const double *params, int params_batched, const double *K,
                        const double *Sigma, const double *x0, const double *u, const double *x, const double *lims, const double *noise,
                        int seed_lo, int seed_hi, int sample0, int traj0, int use_plant, double *xs, double *us, double *cs, double *csum,
                        double *xmean, double *xcov, int32_t *status)
{
    UserProblem *P;
    int rc = enter(h, up, N, B, params, params_batched, &P);
    if (rc) return rc;
    if ((rc = sample_check(P, S, K, x0, u, x, sample0, traj0, use_plant, xs, cs, csum, xmean, xcov, status))) return rc;
    const size_t n = P->n, m = P->m, T = (size_t)N * B, R = (size_t)S * B;
    Staging St(h, Staging::OWNED, "user problem");
    stage_params(St, P, &params, params_batched, B); St.in(&K, K, m * n * T);
    St.in(&noise, Sigma ? noise : nullptr, m * N * R); St.in(&Sigma, Sigma, m * m * T);      // (noise first: it asks for Sigma)
    St.in(&x0, x0, n * B); St.in(&u, u, m * T); St.in(&x, x, n * T); St.in(&lims, lims, 2 * m);
    St.out(&xs, xs, n * N * R); St.out(&us, us, m * N * R); St.out(&cs, cs, (size_t)P->CL * R); St.out(&csum, csum, R);
    St.out(&xmean, xmean, n * T); St.out(&xcov, xcov, n * n * T); St.out(&status, status, (size_t)B);
    if ((rc = St.commit())) return rc;
    return St.finish(ddp_user_sample_f64_dev(h, up, N, B, S, params, params_batched, K, Sigma, x0, u, x, lims, noise, seed_lo, seed_hi, sample0,
                                             traj0, use_plant, xs, us, cs, csum, xmean, xcov, status));
}

// ---- DDP_USER_COST_FIT: the quadratic cost model fitted to sampled rollouts (ddp_user_cost_fit)
// what both flavours of ddp_user_cost_fit refuse, before anything is staged or launched
static int cost_fit_check(const UserProblem *P, int S, const double *xs, const double *us, const double *x, const double *u, const double *cx,
                          const double *cu, const double *cxx, const double *cxu, const double *cuu, const double *c0)
{
    DDP_CHECK(P->mod->costfit, "cost_fit: the problem was made without DDP_USER_COST_FIT");
    DDP_CHECK(S >= 1, "cost_fit: S = %d (>= 1)", S);
    DDP_CHECK(xs && us && x && u && cx && cu && cxx && cxu && cuu && c0, "cost_fit: null argument");
    return 0;
}

int ddp_user_cost_fit_f64_dev(ddp_handle h, void *up, int N, int S, int B, const double *params, int params_batched, const double *xs,
                              const double *us, const double *x, const double *u, double *cx, double *cu, double *cxx, double *cxu,
                              double *cuu, double *c0)
{
    UserProblem *P;
    int rc = enter(h, up, N, B, params, params_batched, &P, ON_DEVICE);
    if (rc) return rc;
    if ((rc = cost_fit_check(P, S, xs, us, x, u, cx, cu, cxx, cxu, cuu, c0))) return rc;
    const Layout &L = P->mod->L;
    const long chunks = ((long)N + L.cchunk - 1) / L.cchunk, ctraj = L.clanes / L.cchunk, groups = ((long)B + ctraj - 1) / ctraj;
    DDP_CHECK(chunks * groups <= 0x7fffffffL, "cost_fit: N = %d, B = %d is too large for one launch", N, B);
    UserCostFitArgs a;
    a.N = N; a.S = S; a.B = B; a.params_batched = P->params_batched;
    a.params = P->params; a.xs = xs; a.us = us; a.x = x; a.u = u;
    a.cx = cx; a.cu = cu; a.cxx = cxx; a.cxu = cxu; a.cuu = cuu; a.c0 = c0;
    void *args[] = {&a};
    DDP_HIP(hipModuleLaunchKernel(P->mod->costfit, (unsigned)(chunks * groups), 1, 1, 64, 1, 1, 0, h->stream, args, nullptr));
    h->last_kernel[1] = "ddp_user_cost_fit";
    return 0;
}

int ddp_user_cost_fit_f64(ddp_handle h, void *up, int N, int S, int B, const double *params, int params_batched, const double *xs,
                          const double *us, const double *x, const double *u, double *cx, double *cu, double *cxx, double *cxu,
                          double *cuu, double *c0)
{
    UserProblem *P;
    int rc = enter(h, up, N, B, params, params_batched, &P);
    if (rc) return rc;
    if ((rc = cost_fit_check(P, S, xs, us, x, u, cx, cu, cxx, cxu, cuu, c0))) return rc;
    const size_t n = P->n, m = P->m, T = (size_t)N * B, R = (size_t)S * T;
    Staging St(h, Staging::OWNED, "user problem");
    stage_params(St, P, &params, params_batched, B); St.in(&xs, xs, n * R); St.in(&us, us, m * R); St.in(&x, x, n * T); St.in(&u, u, m * T);
    St.out(&cx, cx, n * T); St.out(&cu, cu, m * T); St.out(&cxx, cxx, n * n * T); St.out(&cxu, cxu, n * m * T);
    St.out(&cuu, cuu, m * m * T); St.out(&c0, c0, T);
    if ((rc = St.commit())) return rc;
    return St.finish(ddp_user_cost_fit_f64_dev(h, up, N, S, B, params, params_batched, xs, us, x, u, cx, cu, cxx, cxu, cuu, c0));
}

// ---- the rollout, on the problem's own `dynamics` (ddp_user_forward_pass) or on the tables fx, fu, fc of ddp_fit_dynamics
// (ddp_user_rollout_fit, DDP_USER_FITTED; ddp_user_rollout_fit_wave, DDP_USER_FITTED_WAVE): the tables ride on the family for the time
// of the call (FitScope), rollout() then launches the fitted rollout of the program
int ddp_user_forward_pass_f64_dev(ddp_handle h, void *up, int N, int B, const double *params, int params_batched,
                                  const double *K, const double *k, const double *x0, const double *u, const double *x,
                                  const double *alpha, int nalpha, const double *lims, const int32_t *active,
                                  double *xnew, double *unew, double *cnew, double *csum)
{
    UserProblem *P;
    int rc = enter(h, up, N, B, params, params_batched, &P, ON_DEVICE);
    if (rc) return rc;
    DDP_CHECK(x0 && u && alpha && xnew && unew && cnew && csum, "forward_pass: null argument");
    return P->rollout(h, B, nullptr, K, k, x0, u, x, alpha, nalpha, lims, active, xnew, unew, cnew, csum);
}

int ddp_user_rollout_fit_f64_dev(ddp_handle h, void *up, int N, int B, const double *params, int params_batched,
                                 const double *K, const double *k, const double *x0, const double *u, const double *x,
                                 const double *alpha, int nalpha, const double *lims, const int32_t *active,
                                 const double *fx, const double *fu, const double *fc,
                                 double *xnew, double *unew, double *cnew, double *csum)
{
    UserProblem *P;
    int rc = enter(h, up, N, B, params, params_batched, &P, ON_DEVICE);
    if (rc) return rc;
    DDP_CHECK(P->mod->rollfit, "rollout_fit: the problem was made without DDP_USER_FITTED (a DDP_USER_WAVE problem: without DDP_USER_FITTED_WAVE)");
    DDP_CHECK(x0 && u && alpha && fx && fu && fc && xnew && unew && cnew && csum, "rollout_fit: null argument");
    FitScope fit(P, fx, fu, fc);
    return P->rollout(h, B, nullptr, K, k, x0, u, x, alpha, nalpha, lims, active, xnew, unew, cnew, csum);
}

// the host flavour of both, behind the checks of each: the staging, then the `_dev` twin (fx, fu, fc == NULL: ddp_user_forward_pass_f64_dev)
static int rollout_host(ddp_handle h, void *up, const UserProblem *P, int N, int B, const double *params, int params_batched, const double *K,
                        const double *k, const double *x0, const double *u, const double *x, const double *alpha, int nalpha,
                        const double *lims, const double *fx, const double *fu, const double *fc, double *xnew, double *unew, double *cnew,
                        double *csum)
{
    DDP_CHECK(nalpha >= 1 && nalpha <= 16, "forward_pass: nalpha=%d out of [1,16]", nalpha);
    const size_t n = P->n, m = P->m, T = (size_t)N * B, na = nalpha;
    const bool fit = fx != nullptr;
    Staging S(h, Staging::OWNED, "user problem");
    stage_params(S, P, &params, params_batched, B); S.in(&K, K, m * n * T); S.in(&k, k, m * T); S.in(&x0, x0, n * B); S.in(&u, u, m * T);
    S.in(&x, x, n * T); S.in(&lims, lims, 2 * m); S.in(&fx, fx, n * n * T); S.in(&fu, fu, n * m * T); S.in(&fc, fc, n * T);
    S.out(&xnew, xnew, n * T * na); S.out(&unew, unew, m * T * na); S.out(&cnew, cnew, (size_t)P->CL * B * na); S.out(&csum, csum, (size_t)B * na);
    const int rc = S.commit();
    if (rc) return rc;
    if (!fit) return S.finish(ddp_user_forward_pass_f64_dev(h, up, N, B, params, params_batched, K, k, x0, u, x, alpha, nalpha, lims, nullptr,
                                                            xnew, unew, cnew, csum));
    return S.finish(ddp_user_rollout_fit_f64_dev(h, up, N, B, params, params_batched, K, k, x0, u, x, alpha, nalpha, lims, nullptr, fx, fu, fc,
                                                 xnew, unew, cnew, csum));
}

int ddp_user_forward_pass_f64(ddp_handle h, void *up, int N, int B, const double *params, int params_batched,
                              const double *K, const double *k, const double *x0, const double *u, const double *x,
                              const double *alpha, int nalpha, const double *lims,
                              double *xnew, double *unew, double *cnew, double *csum)
{
    UserProblem *P;
    int rc = enter(h, up, N, B, params, params_batched, &P);
    if (rc) return rc;
    DDP_CHECK(x0 && u && alpha && xnew && unew && cnew && csum, "forward_pass: null argument");
    return rollout_host(h, up, P, N, B, params, params_batched, K, k, x0, u, x, alpha, nalpha, lims, nullptr, nullptr, nullptr, xnew, unew,
                        cnew, csum);
}

int ddp_user_rollout_fit_f64(ddp_handle h, void *up, int N, int B, const double *params, int params_batched,
                             const double *K, const double *k, const double *x0, const double *u, const double *x,
                             const double *alpha, int nalpha, const double *lims,
                             const double *fx, const double *fu, const double *fc,
                             double *xnew, double *unew, double *cnew, double *csum)
{
    UserProblem *P;
    int rc = enter(h, up, N, B, params, params_batched, &P);
    if (rc) return rc;
    DDP_CHECK(P->mod->rollfit, "rollout_fit: the problem was made without DDP_USER_FITTED (a DDP_USER_WAVE problem: without DDP_USER_FITTED_WAVE)");
    DDP_CHECK(x0 && u && alpha && fx && fu && fc && xnew && unew && cnew && csum, "rollout_fit: null argument");
    return rollout_host(h, up, P, N, B, params, params_batched, K, k, x0, u, x, alpha, nalpha, lims, fx, fu, fc, xnew, unew, cnew, csum);
}

// ---- the KL loop: ddp_user_ilqgkl on the problem's own model, _fit on the tables fx, fu, fc of ddp_fit_dynamics (DDP_USER_FITTED), _cost
// on a cost model cx .. cuu as well (and on the tables or not).  Every entry fills one KlCall (absent tables, an absent cost model stay
// NULL) for the one loop, ddp_ilqgkl_family_dev; the host flavours share one staging body; what differs between the entries is what
// each refuses.
int ddp_user_ilqgkl_f64_dev(ddp_handle h, void *up, int N, int B, const double *params, int params_batched, const ddp_ilqgkl_opts *o,
                            const double *x0, const double *cost0, const double *Kp, const double *kp, const double *Sp, const double *Sip,
                            const double *model_fx, int model_fx_batched, const double *R1, const double *lims, double *etab,
                            double *x, double *u, double *K, double *Sigma, double *Sigmai, double *Vx, double *Vxx,
                            double *cost, double *dV, double *stats, int *iters)
{
    UserProblem *U;
    int rc = enter(h, up, N, B, params, params_batched, &U, ON_HOST, "ilqgkl");
    if (rc) return rc;
    KlCall c;
    c.opts = o; c.x0 = x0; c.cost0 = cost0; c.Kp = Kp; c.kp = kp; c.Sp = Sp; c.Sip = Sip; c.model_fx = model_fx;
    c.model_fx_batched = model_fx_batched; c.R1 = R1; c.lims = lims; c.etab = etab;
    c.x = x; c.u = u; c.K = K; c.Sigma = Sigma; c.Sigmai = Sigmai; c.Vx = Vx; c.Vxx = Vxx; c.cost = cost; c.dV = dV; c.stats = stats;
    c.iters = iters;
    return ddp_ilqgkl_family_dev(h, U, c);
}

int ddp_user_ilqgkl_fit_f64_dev(ddp_handle h, void *up, int N, int B, const double *params, int params_batched, const ddp_ilqgkl_opts *o,
                                const double *x0, const double *cost0, const double *Kp, const double *kp, const double *Sp,
                                const double *Sip, const double *model_fx, int model_fx_batched, const double *R1, const double *lims,
                                double *etab, const double *fx, const double *fu, const double *fc,
                                double *x, double *u, double *K, double *Sigma, double *Sigmai, double *Vx, double *Vxx,
                                double *cost, double *dV, double *stats, int *iters)
{
    UserProblem *U;
    int rc = enter(h, up, N, B, params, params_batched, &U, ON_HOST, "ilqgkl");
    if (rc) return rc;
    DDP_CHECK(U->mod->rollfit, "ilqgkl_fit: the problem was made without DDP_USER_FITTED (a DDP_USER_WAVE problem: without DDP_USER_FITTED_WAVE)");
    DDP_CHECK(fx && fu && fc, "ilqgkl_fit: null argument");
    KlCall c;
    c.opts = o; c.x0 = x0; c.cost0 = cost0; c.Kp = Kp; c.kp = kp; c.Sp = Sp; c.Sip = Sip; c.model_fx = model_fx;
    c.model_fx_batched = model_fx_batched; c.R1 = R1; c.lims = lims; c.etab = etab;
    c.fit_fx = fx; c.fit_fu = fu; c.fit_fc = fc;
    c.x = x; c.u = u; c.K = K; c.Sigma = Sigma; c.Sigmai = Sigmai; c.Vx = Vx; c.Vxx = Vxx; c.cost = cost; c.dV = dV; c.stats = stats;
    c.iters = iters;
    return ddp_ilqgkl_family_dev(h, U, c);
}

// what both flavours of ddp_user_ilqgkl_cost refuse
static int ilqgkl_cost_check(const UserProblem *U, const KlCall &c)
{
    DDP_CHECK((c.fit_fx && c.fit_fu && c.fit_fc) || (!c.fit_fx && !c.fit_fu && !c.fit_fc),
              "ilqgkl_cost: fx, fu and fc are given all three (the plan is made on the tables) or all three NULL (on the problem's own model)");
    DDP_CHECK(!c.fit_fx || U->mod->rollfit, "ilqgkl_cost: the problem was made without DDP_USER_FITTED (a DDP_USER_WAVE problem: without DDP_USER_FITTED_WAVE; the tables "
                                            "fx, fu, fc need it)");
    DDP_CHECK(c.cm_cx && c.cm_cu && c.cm_cxx && c.cm_cxu && c.cm_cuu, "ilqgkl_cost: a cost model is cx, cu, cxx, cxu and cuu (null argument)");
    return 0;
}

int ddp_user_ilqgkl_cost_f64_dev(ddp_handle h, void *up, int N, int B, const double *params, int params_batched, const ddp_ilqgkl_opts *o,
                                 const double *x0, const double *cost0, const double *Kp, const double *kp, const double *Sp,
                                 const double *Sip, const double *model_fx, int model_fx_batched, const double *R1, const double *lims,
                                 double *etab, const double *fx, const double *fu, const double *fc,
                                 double *x, double *u, double *K, double *Sigma, double *Sigmai, double *Vx, double *Vxx,
                                 double *cost, double *dV, double *stats, int *iters,
                                 const double *cx, const double *cu, const double *cxx, const double *cxu, const double *cuu)
{
    UserProblem *U;
    int rc = enter(h, up, N, B, params, params_batched, &U, ON_HOST, "ilqgkl");
    if (rc) return rc;
    KlCall c;
    c.opts = o; c.x0 = x0; c.cost0 = cost0; c.Kp = Kp; c.kp = kp; c.Sp = Sp; c.Sip = Sip; c.model_fx = model_fx;
    c.model_fx_batched = model_fx_batched; c.R1 = R1; c.lims = lims; c.etab = etab;
    c.fit_fx = fx; c.fit_fu = fu; c.fit_fc = fc;
    c.cm_cx = cx; c.cm_cu = cu; c.cm_cxx = cxx; c.cm_cxu = cxu; c.cm_cuu = cuu;
    c.x = x; c.u = u; c.K = K; c.Sigma = Sigma; c.Sigmai = Sigmai; c.Vx = Vx; c.Vxx = Vxx; c.cost = cost; c.dV = dV; c.stats = stats;
    c.iters = iters;
    if ((rc = ilqgkl_cost_check(U, c))) return rc;
    return ddp_ilqgkl_family_dev(h, U, c);
}

// the host flavour of the three, behind the checks of each (`who` words the null-argument refusal): the staging, the device copy of the
// parameters bound as a `_dev` entry binds it, then the loop on the staged call
static int ilqgkl_host(ddp_handle h, UserProblem *U, const char *who, int N, int B, const double *params, int params_batched, KlCall c)
{
    DDP_CHECK(c.x0 && c.Kp && c.kp && c.Sp && c.Sip && c.R1 && c.x && c.u && c.K && c.Sigma && c.Sigmai && c.Vx && c.Vxx && c.cost && c.dV && c.stats,
              "%s: null argument", who);
    const size_t n = U->n, m = U->m, T = (size_t)N * B, CL = U->CL;
    Staging S(h, Staging::OWNED, "user problem");
    stage_params(S, U, &params, params_batched, B); S.in(&c.x0, c.x0, n * T); S.in(&c.cost0, c.cost0, (size_t)B); S.in(&c.Kp, c.Kp, m * n * T);
    S.in(&c.kp, c.kp, m * T); S.in(&c.Sp, c.Sp, m * m * T); S.in(&c.Sip, c.Sip, m * m * T);
    S.in(&c.model_fx, c.model_fx, n * n * (size_t)N * (c.model_fx_batched ? B : 1)); S.in(&c.R1, c.R1, n * n); S.in(&c.lims, c.lims, 2 * m);
    S.in(&c.fit_fx, c.fit_fx, n * n * T); S.in(&c.fit_fu, c.fit_fu, n * m * T); S.in(&c.fit_fc, c.fit_fc, n * T);
    S.in(&c.cm_cx, c.cm_cx, n * T); S.in(&c.cm_cu, c.cm_cu, m * T); S.in(&c.cm_cxx, c.cm_cxx, n * n * T); S.in(&c.cm_cxu, c.cm_cxu, n * m * T);
    S.in(&c.cm_cuu, c.cm_cuu, m * m * T);
    S.inout(&c.etab, c.etab, (size_t)3 * B); S.out(&c.x, c.x, n * T); S.out(&c.u, c.u, m * T); S.out(&c.K, c.K, m * n * T);
    S.out(&c.Sigma, c.Sigma, m * m * T); S.out(&c.Sigmai, c.Sigmai, m * m * T); S.out(&c.Vx, c.Vx, n * T); S.out(&c.Vxx, c.Vxx, n * n * T);
    S.out(&c.cost, c.cost, CL * B); S.out(&c.dV, c.dV, (size_t)2 * B); S.out(&c.stats, c.stats, (size_t)DDP_ILQGKL_NSTATS * B);
    int rc = S.commit();
    if (rc) return rc;
    if (!(rc = bind(U, N, B, params, params_batched, ON_HOST))) rc = ddp_ilqgkl_family_dev(h, U, c);
    return S.finish(rc);
}

int ddp_user_ilqgkl_f64(ddp_handle h, void *up, int N, int B, const double *params, int params_batched, const ddp_ilqgkl_opts *o,
                        const double *x0, const double *cost0, const double *Kp, const double *kp, const double *Sp, const double *Sip,
                        const double *model_fx, int model_fx_batched, const double *R1, const double *lims, double *etab,
                        double *x, double *u, double *K, double *Sigma, double *Sigmai, double *Vx, double *Vxx,
                        double *cost, double *dV, double *stats, int *iters)
{
    UserProblem *U;
    int rc = enter(h, up, N, B, params, params_batched, &U, ON_HOST, "ilqgkl");
    if (rc) return rc;
    KlCall c;
    c.opts = o; c.x0 = x0; c.cost0 = cost0; c.Kp = Kp; c.kp = kp; c.Sp = Sp; c.Sip = Sip; c.model_fx = model_fx;
    c.model_fx_batched = model_fx_batched; c.R1 = R1; c.lims = lims; c.etab = etab;
    c.x = x; c.u = u; c.K = K; c.Sigma = Sigma; c.Sigmai = Sigmai; c.Vx = Vx; c.Vxx = Vxx; c.cost = cost; c.dV = dV; c.stats = stats;
    c.iters = iters;
    return ilqgkl_host(h, U, "ilqgkl", N, B, params, params_batched, c);
}

int ddp_user_ilqgkl_fit_f64(ddp_handle h, void *up, int N, int B, const double *params, int params_batched, const ddp_ilqgkl_opts *o,
                            const double *x0, const double *cost0, const double *Kp, const double *kp, const double *Sp,
                            const double *Sip, const double *model_fx, int model_fx_batched, const double *R1, const double *lims,
                            double *etab, const double *fx, const double *fu, const double *fc,
                            double *x, double *u, double *K, double *Sigma, double *Sigmai, double *Vx, double *Vxx,
                            double *cost, double *dV, double *stats, int *iters)
{
    UserProblem *U;
    int rc = enter(h, up, N, B, params, params_batched, &U, ON_HOST, "ilqgkl");
    if (rc) return rc;
    DDP_CHECK(U->mod->rollfit, "ilqgkl_fit: the problem was made without DDP_USER_FITTED (a DDP_USER_WAVE problem: without DDP_USER_FITTED_WAVE)");
    DDP_CHECK(fx && fu && fc, "ilqgkl_fit: null argument");
    KlCall c;
    c.opts = o; c.x0 = x0; c.cost0 = cost0; c.Kp = Kp; c.kp = kp; c.Sp = Sp; c.Sip = Sip; c.model_fx = model_fx;
    c.model_fx_batched = model_fx_batched; c.R1 = R1; c.lims = lims; c.etab = etab;
    c.fit_fx = fx; c.fit_fu = fu; c.fit_fc = fc;
    c.x = x; c.u = u; c.K = K; c.Sigma = Sigma; c.Sigmai = Sigmai; c.Vx = Vx; c.Vxx = Vxx; c.cost = cost; c.dV = dV; c.stats = stats;
    c.iters = iters;
    return ilqgkl_host(h, U, "ilqgkl_fit", N, B, params, params_batched, c);
}

int ddp_user_ilqgkl_cost_f64(ddp_handle h, void *up, int N, int B, const double *params, int params_batched, const ddp_ilqgkl_opts *o,
                             const double *x0, const double *cost0, const double *Kp, const double *kp, const double *Sp,
                             const double *Sip, const double *model_fx, int model_fx_batched, const double *R1, const double *lims,
                             double *etab, const double *fx, const double *fu, const double *fc,
                             double *x, double *u, double *K, double *Sigma, double *Sigmai, double *Vx, double *Vxx,
                             double *cost, double *dV, double *stats, int *iters,
                             const double *cx, const double *cu, const double *cxx, const double *cxu, const double *cuu)
{
    UserProblem *U;
    int rc = enter(h, up, N, B, params, params_batched, &U, ON_HOST, "ilqgkl");
    if (rc) return rc;
    KlCall c;
    c.opts = o; c.x0 = x0; c.cost0 = cost0; c.Kp = Kp; c.kp = kp; c.Sp = Sp; c.Sip = Sip; c.model_fx = model_fx;
    c.model_fx_batched = model_fx_batched; c.R1 = R1; c.lims = lims; c.etab = etab;
    c.fit_fx = fx; c.fit_fu = fu; c.fit_fc = fc;
    c.cm_cx = cx; c.cm_cu = cu; c.cm_cxx = cxx; c.cm_cxu = cxu; c.cm_cuu = cuu;
    c.x = x; c.u = u; c.K = K; c.Sigma = Sigma; c.Sigmai = Sigmai; c.Vx = Vx; c.Vxx = Vxx; c.cost = cost; c.dV = dV; c.stats = stats;
    c.iters = iters;
    if ((rc = ilqgkl_cost_check(U, c))) return rc;
    return ilqgkl_host(h, U, "ilqgkl_cost", N, B, params, params_batched, c);
}

}   // extern "C"
