/*
 * ddp_amd.h — C ABI of libddp_amd.so: the MI355X (gfx950) implementation of the iLQG hot path of
 * baggepinnen/DifferentialDynamicProgramming.jl v0.5.0 (back_pass / boxQP / forward_pass and the
 * iLQG iteration around them), batched over B independent trajectories.
 *
 * The reference has no FFI for this path (it is plain Julia); each entry point below replaces the
 * Julia function cited next to it and is what a Julia `@ccall` wrapper (INTEGRATION.md,
 * differentialdynamicprogramming.jl_amd/julia/DDPAmd.jl) or any other host binds.
 *
 * Conventions
 *  - every array is fp64, Julia column-major, batch index slowest:  K[m,n,N,B]  is  B  copies of the
 *    reference's  K[m,n,N]  back to back, so B == 1 accepts the reference's arrays unchanged;
 *  - `_dev` entry points take DEVICE pointers (caller-owned, never freed here) and are asynchronous
 *    on the handle's HIP stream; the plain entry points take HOST pointers, copy H2D, run, copy D2H
 *    and synchronise;
 *  - return value: 0 = ok, < 0 = argument or HIP error (text via ddp_last_error()).  Numerical failure
 *    is NOT an error: it is reported per trajectory in `diverge` (backward_pass.jl:37-38,53-56) and
 *    `result` (boxQP.jl:172-179) exactly like the reference;
 *  - one handle = one HIP stream + scratch; a handle is not thread-safe, distinct handles are.
 *  - there is NO CPU fallback: without a gfx950 device ddp_create() fails.
 */
#ifndef DDP_AMD_H
#define DDP_AMD_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

typedef struct ddp_handle_s *ddp_handle;

/* ---- library / handle --------------------------------------------------------------------- */
const char *ddp_last_error(void);
const char *ddp_version(void);
int  ddp_device_count(void);
int  ddp_create(int device, ddp_handle *out);
/* adopt a caller-owned hipStream_t (e.g. the host framework's current stream) instead of creating one;
 * the stream is not destroyed by ddp_destroy() */
int  ddp_create_with_stream(int device, void *hip_stream, ddp_handle *out);
int  ddp_destroy(ddp_handle h);
int  ddp_sync(ddp_handle h);
/* The DDP_* environment switches (kernel choice for A/B timing and for the tests that force every code path; none is needed in
 * production) are read ONCE, in ddp_create(); no launch calls getenv().  ddp_reload_env() reads them again for this handle.          */
int  ddp_reload_env(ddp_handle h);
/* name of the kernel the last back_pass (which = 0) / forward_pass (which = 1) dispatch of this handle launched ("" before the first
 * one): a debug query — the tests assert through it that the timed path is the one they checked.  which = 2 / 3: the last derivative /
 * cost kernel of a user problem (ddp_user_df*, ddp_user_costfun*; the hessians of DDP_USER_CONST_HESSIAN count as derivatives);
 * which = 4: the plant kernel of a user problem's closed loop (ddp_user_plant).  ddp_user_sample_* counts as a forward_pass
 * (which = 1: ddp_user_sample).  which = 5 / 6: the kernel of the last
 * ddp_forward_covariance_* / ddp_kl_div_* call, the iLQGkl drivers' included (fcov_kernel, fcov_q4_kernel<1|2>, fcov_q4l_kernel,
 * fcov_wide_kernel / kl_div_kernel, kl_div_lds_kernel<4,1|4,2|0,0>, kl_div_wide_kernel).                                           */
const char *ddp_last_kernel(ddp_handle h, int which);
/* The shared-operand backward pass (one fx, fu, cxx, cxu, cuu for the batch) hands work between work-groups of one launch; every such
 * wait is time-bounded (4 s).  A tile whose wait ran out gives its trajectories to the per-trajectory kernels launched behind it — the
 * results stay correct — and is counted: this returns the number of such tiles since ddp_create (synchronises the stream; 0 in a
 * healthy run, < 0 on error).  A debug query like ddp_last_kernel.                                                                  */
int  ddp_sh_timeouts(ddp_handle h);
/* What the tiles counted by ddp_sh_timeouts were waiting for: up to 8 records of 8 ints — {work-group, group, chunk (of 8 time steps)
 * waited for, progress word last seen (chunks published | 1 << 30: group finished), milliseconds waited, XCD, groups of that launch,
 * launch number} — of the first tiles that gave up since the control block was allocated, followed by the 16 progress words as they
 * stand now.  out: cap >= 80 ints.  Returns the number of records (0 in a healthy run), < 0 on error; synchronises the stream.  (Own
 * protocol of the shared-operand kernel: no counterpart in the reference.)                                                              */
int  ddp_sh_timeout_info(ddp_handle h, int *out, int cap);
/* The shared-operand backward pass keeps the matrix recursion of each λ it has computed (a record stream in the handle's scratch) and
 * reuses it in later calls with bit-identical fx, fu, cxx, cxu, cuu, N, regType and λ (compared on the device in every call;
 * DDP_SH_REUSE=0 switches the reuse off).  out[0]: λ groups served from a kept stream, out[1]: groups whose recursion was computed,
 * since the scratch was (re)allocated.  out: 2 ints.  Synchronises the stream; 0, < 0 on error.  A debug query like ddp_sh_timeouts.  */
int  ddp_sh_reuse_stats(ddp_handle h, int *out);
/* The plan ddp_df_* follows for the matrix exponential of a pendcart element whose ZoH block matrix has 1-norm nA (Higham's scaling and
 * squaring): *degree = 3 / 5 / 7 / 9 for nA <= 0.015 / 0.25 / 0.95 / 2.1 and 13 beyond, *squarings = max(0, ceil(log2(nA / 5.4))) of the
 * degree-13 result.  A norm that is not finite (an infinite control; NaN) has no plan: *degree = 0, no exponential is formed and that
 * element's fx and fu are NaN (cx and cu are written as usual).  Needs no handle and no GPU; returns 0.  A debug query like
 * ddp_last_kernel: the function the kernels call.                                                                                    */
int  ddp_df_expm_plan(double nA, int *degree, int *squarings);
void *ddp_stream(ddp_handle h);                 /* the hipStream_t of the handle */
/* device memory helpers for hosts without their own allocator (the Julia wrapper, tests) */
int  ddp_malloc(ddp_handle h, size_t bytes, void **dptr);
int  ddp_free(ddp_handle h, void *dptr);
int  ddp_memcpy_h2d(ddp_handle h, void *dst, const void *src, size_t bytes);   /* synchronous */
int  ddp_memcpy_d2h(ddp_handle h, void *dst, const void *src, size_t bytes);   /* synchronous */
int  ddp_memset(ddp_handle h, void *dst, int value, size_t bytes);             /* async on stream */
/* Page-locked host memory for the RESULT arrays of the host-pointer entry points.  The link moves 56 GB/s into pinned or already-touched
 * pages; what a host-pointer call used to pay for is the first touch of freshly allocated pageable result arrays (1.2 GB per C2 pass:
 * 8-13 k passes/s against a link bound of ~46 k).  Blocks freed with ddp_host_free are kept in a process-wide cache (same size -> same
 * block on the next call: no pinning, no page faults), bounded by DDP_PINNED_CACHE_MB (default 2048, clamped to [0, 65536]); ddp_host_trim
 * empties the cache.  Blocks that are in use (the arrays the hosts returned) are page-locked for as long as the caller keeps them.
 * Any host pointer still works everywhere — this is an allocator the hosts (ctypes mirror, DDPAmd.jl) use for what they return.       */
int  ddp_host_alloc(size_t bytes, void **hptr);
int  ddp_host_free(void *hptr);
int  ddp_host_trim(void);
/* HIP events on the handle's stream (bench.py's per-kernel timing) */
int  ddp_event_create(ddp_handle h, void **ev);
int  ddp_event_destroy(ddp_handle h, void *ev);
int  ddp_event_record(ddp_handle h, void *ev);
int  ddp_event_elapsed_ms(ddp_handle h, void *start, void *stop, float *ms);   /* syncs on `stop` */

/* ---- back_pass — replaces back_pass(cx,cu,cxx,cxu,cuu,fx,fu,λ,regType,lims,x,u) ---------------
 * reference: src/backward_pass.jl:217-252 (LTI), :162-177 (LTV, time-invariant cost),
 *            :179-215 (LTV, time-varying cost), shared tail @end_backward_pass :28-79,
 *            called from src/iLQG.jl:237.                                                        */
typedef struct {
    int n, m, N, B;        /* state dim, control dim, time steps (= size(u,2)), batch              */
    int fx_tv;             /* 0: fx[n,n], fu[n,m]           1: fx[n,n,N], fu[n,m,N]                */
    int fx_batched;        /* 0: one fx/fu shared by the batch   1: one per trajectory (batch slowest) */
    int cost_tv;           /* 0: cxx[n,n], cxu[n,m], cuu[m,m]    1: [..,N]                          */
    int cost_batched;      /* as fx_batched for cxx/cxu/cuu                                         */
    int regType;           /* 1 or 2 (backward_pass.jl:245-247)                                     */
    int has_lims;          /* 0: `lims == []`   1: lims[m,2] given (the lims[1,1] > lims[1,2] test of
                              backward_pass.jl:31 is applied on the device as well)                 */
} ddp_bp_desc;

/* inputs : cx[n,N,B] cu[m,N,B]  cxx/cxu/cuu/fx/fu per the flags  lambda[B]  lims[m,2] (shared) u[m,N,B]
 *          `active` (may be NULL): int32[B]; trajectories with active[b]==0 are skipped entirely
 * outputs: K[m,n,N,B] k[m,N,B] Quu[m,m,N,B] Vx[n,N,B] Vxx[n,n,N,B] dV[2,B] diverge int32[B]
 *          (diverge: 0 ok, else the 1-based failing time index; outputs earlier in time than the
 *          failing step are zero like the reference's zero-initialised arrays)
 * shapes : any 1 <= n <= 64 with 1 <= m <= DDP_MAX_M_WIDE (32).  Kernel families by size, for m <= DDP_MAX_M (8): n = 10/m = 2,
 *          n = 4/m = 1, any n <= 12/m <= 4, n <= 14/m <= 4, n <= 32/m <= 8, 32 < n <= 64 with m <= 8 at run time on the matrix-core kernel
 *          back_pass_mf2 (padded to 16-row tiles and 8 controls inside the LDS only, no scratch on the handle).  Wide controls,
 *          8 < m <= 32 with any n <= 64: back_pass_wide_kernel, one work-group of four waves per trajectory, run-time sizes, every
 *          operand layout, limits by a box-QP across the lanes of a wave; operands are read from the caller's arrays (no padded
 *          copies, no scratch on the handle).  n > 64 or m > 32: return code < 0.
 *          back_pass_gps and the KL functions: n <= 32, m <= DDP_MAX_M; after ddp_kl_set_wide(h, 1) any n <= 64 with
 *          m <= DDP_MAX_M_WIDE (the KL section below).  User problems (ddp_user_*) without DDP_USER_WAVE and the lane-per-problem
 *          boxQP stop at m = DDP_MAX_M; full DDP of a user problem beyond n = 32, m = 8 is DDP_USER_SECOND_ORDER_WAVE.                                                                                    */
int ddp_back_pass_f64_dev(ddp_handle h, const ddp_bp_desc *d,
                          const double *cx, const double *cu, const double *cxx, const double *cxu,
                          const double *cuu, const double *fx, const double *fu,
                          const double *lambda, const double *lims, const double *u,
                          const int32_t *active,
                          double *K, double *k, double *Quu, double *Vx, double *Vxx, double *dV,
                          int32_t *diverge);
int ddp_back_pass_f64(ddp_handle h, const ddp_bp_desc *d,
                      const double *cx, const double *cu, const double *cxx, const double *cxu,
                      const double *cuu, const double *fx, const double *fu,
                      const double *lambda, const double *lims, const double *u,
                      double *K, double *k, double *Quu, double *Vx, double *Vxx, double *dV,
                      int32_t *diverge);

/* ---- boxQP — replaces boxQP(H,g,lower,upper,x0) ------------------------------------------------
 * reference: src/boxQP.jl:29-188, called from src/backward_pass.jl:49.
 * `count` independent problems of dimension m <= DDP_QP_MAX_M (m <= DDP_MAX_M, the sizes the backward pass uses: one
 * lane per problem; larger m — upstream's demoQP runs m = 500, boxQP.jl:190-199 — one work-group per problem):
 * H[m,m,count] g/lower/upper/x0[m,count] -> x[m,count] result int32[count]
 * Hfree[m,m,count] (leading nfree x nfree block = upper Cholesky factor of H[free,free], zero elsewhere)
 * free uint8[m,count].                                                                             */
#define DDP_MAX_M 8
#define DDP_MAX_M_WIDE 32   /* back_pass, forward_pass, df, costfun and the iLQG drivers of DDP_PROBLEM_LQ: 8 < m <= 32 on the wide-control kernels */
#define DDP_QP_MAX_M 1024
typedef struct {
    int    maxIter;        /* 100   */
    double minGrad;        /* 1e-8  */
    double minRelImprove;  /* 1e-8  */
    double stepDec;        /* 0.6   */
    double minStep;        /* 1e-22 */
    double Armijo;         /* 0.1   */
} ddp_qp_opts;
int ddp_boxqp_f64_dev(ddp_handle h, int m, int count, const double *H, const double *g,
                      const double *lower, const double *upper, const double *x0,
                      const ddp_qp_opts *opts /* NULL = defaults */,
                      double *x, int32_t *result, double *Hfree, uint8_t *free_out);
int ddp_boxqp_f64(ddp_handle h, int m, int count, const double *H, const double *g,
                  const double *lower, const double *upper, const double *x0,
                  const ddp_qp_opts *opts,
                  double *x, int32_t *result, double *Hfree, uint8_t *free_out);

/* ---- forward_pass — replaces forward_pass(traj_new,x0,u,x,α,f,costfun,lims,diff) ----------------
 * reference: src/forward_pass.jl:9-33, called from src/iLQG.jl:185,268.
 * The user closures f / costfun cannot run on the GPU; registered problem families stand in:
 *   DDP_PROBLEM_LQ        x+ = A x + B u,  cost_i = .5 x_i'Q x_i + .5 u_i'R u_i
 *                         (src/demo_linear.jl:42-49; cost returned per time step, the sum is the
 *                          reference's scalar)
 *   DDP_PROBLEM_PENDCART  explicit-Euler pendulum on a cart (src/system_pendcart.jl:83-89) with
 *                         cost vector of length N+1 (src/system_pendcart.jl:97-106)               */
enum { DDP_PROBLEM_LQ = 0, DDP_PROBLEM_PENDCART = 1 };
typedef struct {
    int kind;
    int n, m, N, B;
    /* LQ */
    const double *A;       /* [n,n] | [n,n,N] | [n,n,B] | [n,n,N,B] per dyn_tv / dyn_batched        */
    const double *Bm;      /* [n,m] ...                                                              */
    int dyn_tv, dyn_batched;
    const double *Q;       /* [n,n] (shared)                                                         */
    const double *R;       /* [m,m] (shared)                                                         */
    /* pendcart (n = 4, m = 1; Q [4,4], R [1,1] above) */
    double g, l, h, d;
    double goal[4];
    /* 1: the caller declares Q and R DIAGONAL (true for the reference's demos: Q = h·I, R = 0.1h·I, Q = diag(10,1,2,1)); the rollout
     * kernels of the n = 10 / m = 2 and pendcart shapes then evaluate the cost themselves from the values they hold instead of a
     * second kernel re-reading xnew, unew (only the diagonals are read).  0: general Q, R.  The declaration IS verified: the host-pointer
     * entry points test the host copies; the _dev entry points look at Q, R once per (Q, R) address pair and handle (one small
     * device-to-host copy; a PASS is cached — a caller that rewrites Q or R in place must keep the flag honest; ddp_free of
     * the allocation holding Q or R, ddp_reload_env and a new handle forget it; a refusal is never cached).  A full Q or R with cost_diag = 1 is refused (< 0).  Any value but 0 / 1 is refused,
     * so a struct that was not zero-initialised — or a caller built against the 0.1.0 layout, which ended at goal[] — fails loudly.   */
    int cost_diag;
    /* diff_fun (src/forward_pass.jl:19, iLQG.jl:160: `K*diff_fun(x̂, x)`; default `-`).  A closure cannot cross the C ABI; what stands in
     * is subtraction with the coordinates named in this bit mask (bit j = state j, n <= 32) wrapped to [-π, π]:
     *     d = x̂_j - x_j;  d - 2π·rint(d / 2π)        (Julia: rem2pi(x̂[j] - x[j], RoundNearest))
     * — the usual reason the hook exists (angles).  0 = the reference's default.  Bits at or above n are refused (a struct that was not
     * zero-initialised fails loudly); with a non-zero mask the rollout runs in the run-time-sized kernel (n <= 32).                 */
    uint32_t diff_wrap;
} ddp_problem;

/* cost vector length per trajectory: LQ -> N, pendcart -> N+1 */
int ddp_cost_len(const ddp_problem *p);

/* All `nalpha` step sizes are rolled out concurrently (one work-group slice per (trajectory, α)).
 * shapes : DDP_PROBLEM_LQ: any n <= 64 with m <= DDP_MAX_M_WIDE (32); 8 < m <= 32 runs in forward_wide_kernel (one wave per
 *          (trajectory, α), every dyn_tv / dyn_batched layout, limits, diff_wrap for n <= 32 as below).  DDP_PROBLEM_PENDCART:
 *          n = 4, m = 1.  Anything else: return code < 0.
 * inputs : K[m,n,N,B], k[m,N,B] (both NULL = empty policy, forward_pass.jl:17), x0[n,B], u[m,N,B],
 *          x[n,N,B] (may be NULL with an empty policy), alpha[nalpha] (HOST pointer, <= 16 values),
 *          lims[m,2] or NULL, active int32[B] or NULL
 * outputs: xnew[n,N,B,nalpha], unew[m,N,B,nalpha], cnew[CL,B,nalpha], csum[B,nalpha] (= sum(cnew))  */
int ddp_forward_pass_f64_dev(ddp_handle h, const ddp_problem *p,
                             const double *K, const double *k, const double *x0, const double *u,
                             const double *x, const double *alpha, int nalpha, const double *lims,
                             const int32_t *active,
                             double *xnew, double *unew, double *cnew, double *csum);
int ddp_forward_pass_f64(ddp_handle h, const ddp_problem *p,
                         const double *K, const double *k, const double *x0, const double *u,
                         const double *x, const double *alpha, int nalpha, const double *lims,
                         double *xnew, double *unew, double *cnew, double *csum);

/* ---- df of the registered families (the `df` closure; STEP 1 of src/iLQG.jl:225-229) -------------
 * LQ: cx = Q x, cu = R u (src/demo_linear.jl:35-41).  pendcart: also fx[4,4,N,B], fu[4,1,N,B] by
 * exp of the 5x5 block matrix (src/system_pendcart.jl:137-154).  fx/fu may be NULL for LQ.         */
int ddp_df_f64_dev(ddp_handle h, const ddp_problem *p, const double *x, const double *u,
                   const int32_t *active, double *cx, double *cu, double *fx, double *fu);
int ddp_df_f64(ddp_handle h, const ddp_problem *p, const double *x, const double *u,
               double *cx, double *cu, double *fx, double *fu);

/* ---- iLQG — replaces iLQG(f,costfun,df,x0,u0; lims, ...) for registered families ----------------
 * reference: src/iLQG.jl:143-341.  Every trajectory of the batch runs its own iLQG (own λ, dλ,
 * line search, termination) with state resident on the device; the host only launches kernels
 * and polls one counter per iteration.                                                            */
typedef struct {
    double lambda, dlambda, lambda_factor, lambda_max, lambda_min;   /* 1, 1, 1.6, 1e10, 1e-6 */
    double tol_fun, tol_grad;                                        /* 1e-7, 1e-4            */
    int    max_iter;                                                 /* 500                   */
    int    regType;                                                  /* 1                     */
    double reduce_ratio_min;                                         /* 0                     */
    int    n_alpha;                                                  /* 11                    */
    double alpha[16];                                                /* 10^linspace(0,-3,11)  */
} ddp_ilqg_opts;
void ddp_ilqg_default_opts(ddp_ilqg_opts *o);

enum {
    DDP_EXIT_RUNNING       = 0,
    DDP_EXIT_GRAD          = 1,   /* SUCCESS: gradient norm < tol_grad   (iLQG.jl:258-261) */
    DDP_EXIT_COST          = 2,   /* SUCCESS: cost change < tol_fun      (iLQG.jl:306-309) */
    DDP_EXIT_LAMBDA        = 3,   /* EXIT: lambda > lambda_max           (iLQG.jl:319-322) */
    DDP_EXIT_MAXITER       = 4,   /* while condition exhausted           (iLQG.jl:222)     */
    DDP_EXIT_CAP           = 5,   /* NOT a state of the reference: the driver's own bound on batch-level iterations
                                     (4 max_iter + 1000) ran out while this trajectory was still running         */
    DDP_EXIT_INIT_DIVERGED = -1   /* initial control sequence diverged   (iLQG.jl:205-210) */
};

/* per-trajectory summary, one row per trajectory: stats[8,B] =
 *   [status, iter, accepted_iter, n_backpass, n_forward, lambda, g_norm, sum(cost)]               */
#define DDP_ILQG_NSTATS 8
/* host-pointer flavour. inputs x0[n,B], u0[m,N,B], lims[m,2] or NULL.
 * outputs x[n,N,B] u[m,N,B] K[m,n,N,B] k[m,N,B] (quirk: after an accepted step L.k is the control
 * sequence, iLQG.jl:303) Quu[m,m,N,B] Vx[n,N,B] Vxx[n,n,N,B] cost[CL,B] stats[8,B];
 * trace_cost (may be NULL) [trace_cap,B]: sum(cost) after every iteration (trace(:cost,...)).
 * `global_iters` (may be NULL) receives the number of batch-level iterations executed.
 * x0 / u0 must not alias x / u (the outputs are cleared before the initial rollout).                */
int ddp_ilqg_f64(ddp_handle h, const ddp_problem *p, const ddp_ilqg_opts *o,
                 const double *x0, const double *u0, const double *lims,
                 double *x, double *u, double *K, double *k, double *Quu, double *Vx, double *Vxx,
                 double *cost, double *stats, int trace_cap, double *trace_cost, int *global_iters);
int ddp_ilqg_f64_dev(ddp_handle h, const ddp_problem *p, const ddp_ilqg_opts *o,
                     const double *x0, const double *u0, const double *lims,
                     double *x, double *u, double *K, double *k, double *Quu, double *Vx, double *Vxx,
                     double *cost, double *stats, int trace_cap, double *trace_cost, int *global_iters);

/* Warm start from a PRE-ROLLED trajectory (src/iLQG.jl:193-197: `size(x0,2) == N` ⇒ `x = x0`, no initial rollout, no
 * divergence test; `cost` as given or `costfun(x,u)`) — the entry an MPC loop calls with its shifted previous solution.
 * x0[n,N,B]; cost0[CL,B] or NULL.  Line-search rollouts start from x0[:,1] like the reference (iLQG.jl:268).          */
int ddp_ilqg_warm_f64(ddp_handle h, const ddp_problem *p, const ddp_ilqg_opts *o,
                      const double *x0, const double *u0, const double *cost0, const double *lims,
                      double *x, double *u, double *K, double *k, double *Quu, double *Vx, double *Vxx,
                      double *cost, double *stats, int trace_cap, double *trace_cost, int *global_iters);
int ddp_ilqg_warm_f64_dev(ddp_handle h, const ddp_problem *p, const ddp_ilqg_opts *o,
                          const double *x0, const double *u0, const double *cost0, const double *lims,
                          double *x, double *u, double *K, double *k, double *Quu, double *Vx, double *Vxx,
                          double *cost, double *stats, int trace_cap, double *trace_cost, int *global_iters);
/* ---- slot scheduler: more problems than resident trajectories, and closed-loop MPC on the device -------------------------------
 * The batch of ddp_ilqg_* advances in lock step: a trajectory that has ended keeps its place until the slowest one ends (pendcart:
 * median 50 iterations, slowest 233).  Here `slots` trajectories are resident and the P = p->B problems go through them: a slot
 * whose solve has ended is flushed to its problem's rows of the outputs and armed with the next problem ON THE DEVICE, in the global
 * iteration in which it ended; the host only polls the number of busy slots.  Every solve performs the launches of its stand-alone
 * solve at batch size `slots` (initial rollout of src/iLQG.jl:181-192 included), so its results are those of ddp_ilqg_f64 with
 * p->B = slots.  inputs x0[n,P] u0[m,N,P]; outputs as ddp_ilqg_f64 with P columns; slots <= 0: min(P, 4096).  Per-trajectory
 * dynamics (dyn_batched) are refused.                                                                                             */
int ddp_ilqg_queue_f64(ddp_handle h, const ddp_problem *p, const ddp_ilqg_opts *o, int slots,
                       const double *x0, const double *u0, const double *lims,
                       double *x, double *u, double *K, double *k, double *Quu, double *Vx, double *Vxx,
                       double *cost, double *stats, int *global_iters);
int ddp_ilqg_queue_f64_dev(ddp_handle h, const ddp_problem *p, const ddp_ilqg_opts *o, int slots,
                           const double *x0, const double *u0, const double *lims,
                           double *x, double *u, double *K, double *k, double *Quu, double *Vx, double *Vxx,
                           double *cost, double *stats, int *global_iters);
/* Closed loop (the receding-horizon use of the warm-start hook, src/iLQG.jl:193-197): every trajectory is solved `steps` times; after
 * solve t its first control is applied (the model is the plant: the next initial state is x_1 of the solution), the control
 * sequence is shifted by one step (tail: last column repeated, or zeros) and solved again — shift and re-solve happen on the
 * device by the same mechanism that re-arms a slot of the queue.  outputs: xcl[n,steps+1,B] (the closed-loop states, xcl[:,0,b] =
 * x0[:,b]), ucl[m,steps,B] (the applied controls), stats_cl[8,steps,B] (the summary row of every solve), x[n,N,B] / u[m,N,B] (the
 * last plan).  A solve whose initial rollout diverges ends the loop of its trajectory (later columns stay zero).                  */
int ddp_ilqg_mpc_f64(ddp_handle h, const ddp_problem *p, const ddp_ilqg_opts *o, int steps, int zero_tail,
                     const double *x0, const double *u0, const double *lims,
                     double *xcl, double *ucl, double *stats_cl, double *x, double *u, int *global_iters);
int ddp_ilqg_mpc_f64_dev(ddp_handle h, const ddp_problem *p, const ddp_ilqg_opts *o, int steps, int zero_tail,
                         const double *x0, const double *u0, const double *lims,
                         double *xcl, double *ucl, double *stats_cl, double *x, double *u, int *global_iters);
/* Per-phase GPU time of the following ddp_ilqg_* calls on this handle — the time_derivs / time_backward / time_forward
 * trace keys of the reference (src/iLQG.jl:227,241,281; print_timing :343-366): host_buf[3, cap] (row-major: row r at
 * host_buf + cap*r), seconds per GLOBAL iteration (the batch advances in lock step; the call's *global_iters says how many
 * columns were written), measured with HIP events on the handle's stream.  NULL switches it off. */
int ddp_ilqg_set_timing(ddp_handle h, double *host_buf, int cap);
/* The general entry: optional pre-rolled x0 (x0_prerolled != 0: x0[n,N,B] and cost0[CL,B] or NULL) and ALL per-iteration
 * trace keys of the reference (src/iLQG.jl:257,325-330) per trajectory: trace7[7, trace_cap, B] (may be NULL), rows
 * λ, dλ, α (NaN when no step was accepted), improvement (Δcost), cost (sum), reduce_ratio, grad_norm; entry `iter-1` of
 * trajectory b is written when its iteration `iter` completes (exits by tolerance leave before the trace like upstream). */
int ddp_ilqg_ex_f64(ddp_handle h, const ddp_problem *p, const ddp_ilqg_opts *o,
                    const double *x0, int x0_prerolled, const double *u0, const double *cost0, const double *lims,
                    double *x, double *u, double *K, double *k, double *Quu, double *Vx, double *Vxx,
                    double *cost, double *stats, int trace_cap, double *trace7, int *global_iters);
int ddp_ilqg_ex_f64_dev(ddp_handle h, const ddp_problem *p, const ddp_ilqg_opts *o,
                        const double *x0, int x0_prerolled, const double *u0, const double *cost0, const double *lims,
                        double *x, double *u, double *K, double *k, double *Quu, double *Vx, double *Vxx,
                        double *cost, double *stats, int trace_cap, double *trace7, int *global_iters);
/* batch-level statistics of one pass in one launch: out4 = [sum(csum[B]), sum(dV[1,:]), sum(dV[2,:]), #(diverge != 0)];
 * any input may be NULL.  This is the vector a multi-GPU job all-reduces (one small collective per pass).               */
int ddp_batch_stats_f64_dev(ddp_handle h, int B, const double *csum, const double *dV, const int32_t *diverge, double *out4);
/* ---- multi-GPU: the one collective of the path -------------------------------------------------------
 * New (the reference is single-process).  One process per GPU, trajectories sharded over the ranks, no data-path exchange; a job
 * shares one small statistics vector per pass / solve.  RCCL is loaded at first use (no link-time dependency).
 *   rank 0: ddp_comm_unique_id(id); ship the 128 bytes to the other ranks by any means (file, MPI, torch.distributed broadcast)
 *   every rank: ddp_comm_create(h, nranks, rank, id, &comm)                       (= ncclCommInitRank, collective)
 *   ddp_allreduce_stats_f64_dev(h, comm, buf, nsum, nmax): device vector buf[nsum + nmax] (<= DDP_COMM_MAX_STATS) becomes, on every
 *   rank, the SUM over ranks of its first nsum entries and the MAX over ranks of the remaining nmax — ONE RCCL call (all-gather of
 *   the tiny vectors + a local reduction), asynchronous on the handle's stream.                                         */
#define DDP_COMM_ID_BYTES 128
#define DDP_COMM_MAX_STATS 64
typedef struct ddp_comm_s *ddp_comm;
/* RCCL as the library sees it: *version = NCCL_VERSION_CODE of the librccl in use (the hand-declared ABI needs >= 2.18: return < 0 below
 * that or when no librccl can be loaded), *preloaded = 1 when the process already held a librccl (e.g. PyTorch's torch/lib/librccl.so) and
 * that instance is used — a second copy is never loaded beside it.                                                            */
int ddp_comm_rccl_info(int *version, int *preloaded);
int ddp_comm_unique_id(char id[DDP_COMM_ID_BYTES]);
int ddp_comm_create(ddp_handle h, int nranks, int rank, const char id[DDP_COMM_ID_BYTES], ddp_comm *out);
int ddp_comm_destroy(ddp_comm c);
int ddp_allreduce_stats_f64_dev(ddp_handle h, ddp_comm c, double *buf, int nsum, int nmax);
/* Receding-horizon warm start between two MPC solves (new, the reference has no MPC loop — its hook is
 * the pre-rolled `x0[n,N]` + `cost` of src/iLQG.jl:193-197, see ddp_ilqg_warm_f64): a time-major array a[d, N, B] moves
 * `shift` steps towards the present, dst[:, i, b] = src[:, i+shift, b]; the vacated tail repeats the last column
 * (zero_tail = 0: controls, nominal states) or is zero (zero_tail = 1: gains).  Out of place, device pointers.        */
int ddp_mpc_shift_f64_dev(ddp_handle h, int d, int N, int B, int shift, int zero_tail, const double *src, double *dst);
/* the `costfun` closure of the registered families on given trajectories: cost[CL,B], csum[B] (may be NULL)          */
int ddp_costfun_f64_dev(ddp_handle h, const ddp_problem *p, const double *x, const double *u, const int32_t *active,
                        double *cost, double *csum);

/* ---- KL-constrained path (BASELINE config 5) ------------------------------------------------------
 * reference: back_pass_gps src/backward_pass.jl:259-350 (called from src/iLQGkl.jl:100,191), ∇kl and kl_div_wiki
 * src/klutils.jl:8-23,70-103, forward_covariance src/forward_pass.jl:37-56, calc_η src/klutils.jl:112-133 (ddp_kl_dual_*).
 * `df(model,·)` / `covariance(model,·)` belong to the un-vendored dependency LinearTimeVaryingModelsBase: the model is
 * passed as the arrays it would return (fx, R1).
 * shapes : 1 <= n <= 32, 1 <= m <= DDP_MAX_M (8) for every call of this section.  ddp_kl_set_wide(h, 1) opens 1 <= n <= 64,
 *          1 <= m <= DDP_MAX_M_WIDE (32) for ddp_kl_terms_*, ddp_back_pass_gps_*, ddp_forward_covariance_*, ddp_kl_div_*,
 *          ddp_ilqgkl_* (DDP_PROBLEM_LQ) and ddp_user_ilqgkl_* (problems made with DDP_USER_WAVE; DDP_USER_SECOND_ORDER and
 *          DDP_USER_SECOND_ORDER_WAVE stay refused).  Shapes beyond n <= 32, m <= 8 then run on kernels of their own: back_pass_gps on the GPS instantiation of
 *          back_pass_wide_kernel (ddp_last_kernel(h, 0) reports "back_pass_gps_wide"; Quui by Gauss-Jordan elimination across the
 *          lanes of a wave), ∇kl, forward_covariance (v_mfma_f64_16x16x4 tiles, up to 136 KB of LDS) and kl_div_wiki (both
 *          log-determinants by LU across lanes, klmean by a fixed-order sum: two runs agree bit for bit) on those of kl_wide.hip.
 *          Shapes with n <= 32 and m <= 8 keep the kernels they had.  n > 64 or m > 32: return code < 0 before any launch, and so
 *          for n > 32 or m > 8 while the switch is off.  DDP_GPS_WIDE=1 in the environment (read at ddp_create / ddp_reload_env)
 *          sends every shape to the wide kernels (A/B timing, tests).                                                  */
typedef struct {
    const double *cx, *cu;       /* cxkl[n,N,B], cukl[m,N,B]                                                     */
    const double *cxx, *cxu;     /* cxxkl[n,n,N,B], cxukl[m,n,N,B]  (m x n, the layout ∇kl returns, klutils.jl:20) */
    const double *cuu;           /* cuukl[m,m,N,B]                                                               */
    const double *eta;           /* eta_tv == 0: η[B] (ηbracket[2] per trajectory); 1: η[N,B] (ηbracket[2,i])     */
    int eta_tv;
} ddp_kl_cost_terms;

/* The switch of the handle for the large shapes (default 0: every call of this section does what it always did).  Returns the
 * previous value (0 or 1), < 0 for a null handle.                                                                   */
int ddp_kl_set_wide(ddp_handle h, int on);

/* ∇kl(traj_prev): K[m,n,N,B], k[m,N,B], Sigmai[m,m,N,B] -> the five arrays of ddp_kl_cost_terms (outputs)      */
int ddp_kl_terms_f64_dev(ddp_handle h, int n, int m, int N, int B, const double *K, const double *k, const double *Sigmai,
                         double *cx, double *cu, double *cxx, double *cxu, double *cuu);
int ddp_kl_terms_f64(ddp_handle h, int n, int m, int N, int B, const double *K, const double *k, const double *Sigmai,
                     double *cx, double *cu, double *cxx, double *cxu, double *cuu);

/* back_pass_gps: d->fx_tv and d->cost_tv must be 1 (3-D arrays, as the reference's method signature), regType unused.
 * Outputs as ddp_back_pass plus Quui[m,m,N,B] = inv(Quu_i) (the Σ field of the returned GaussianPolicy); Quu is the
 * KL-augmented, symmetrised matrix (the Σi field).  n <= 32, m <= 8; with ddp_kl_set_wide n <= 64, m <= 32, where the
 * layout flags of d are all honoured (fx_tv, cost_tv may be 0).                                                   */
int ddp_back_pass_gps_f64_dev(ddp_handle h, const ddp_bp_desc *d,
                              const double *cx, const double *cu, const double *cxx, const double *cxu, const double *cuu,
                              const double *fx, const double *fu, const ddp_kl_cost_terms *kl,
                              const double *lims, const double *u, const int32_t *active,
                              double *K, double *k, double *Quu, double *Quui, double *Vx, double *Vxx, double *dV,
                              int32_t *diverge);
int ddp_back_pass_gps_f64(ddp_handle h, const ddp_bp_desc *d,
                          const double *cx, const double *cu, const double *cxx, const double *cxu, const double *cuu,
                          const double *fx, const double *fu, const ddp_kl_cost_terms *kl,
                          const double *lims, const double *u,
                          double *K, double *k, double *Quu, double *Quui, double *Vx, double *Vxx, double *dV,
                          int32_t *diverge);

/* forward_covariance: fx[n,n,N] (fx_batched: [n,n,N,B]) and R1[n,n] (shared) of the model, K[m,n,N,B], Sigma[m,m,N,B]
 * -> sigmanew[(n+m),(n+m),N,B]; entries the reference leaves undef (u-blocks of the last step) are zero.           */
int ddp_forward_covariance_f64_dev(ddp_handle h, int n, int m, int N, int B, const double *fx, int fx_batched,
                                   const double *R1, const double *K, const double *Sigma, double *sigmanew);
int ddp_forward_covariance_f64(ddp_handle h, int n, int m, int N, int B, const double *fx, int fx_batched,
                               const double *R1, const double *K, const double *Sigma, double *sigmanew);

/* kl_div_wiki: per-step divergence kldiv[N,B] (clipped at 0) and its mean over time klmean[B]; a trajectory whose
 * logdet would throw (non-positive determinant of Σ) gets klmean = +Inf like the reference's `return Inf`.          */
int ddp_kl_div_f64_dev(ddp_handle h, int n, int m, int N, int B, const double *xnew, const double *xold,
                       const double *sigmanew, const double *Kn, const double *kn, const double *Sn,
                       const double *Kp, const double *kp, const double *Sp, const double *Sip,
                       double *kldiv, double *klmean);
int ddp_kl_div_f64(ddp_handle h, int n, int m, int N, int B, const double *xnew, const double *xold,
                   const double *sigmanew, const double *Kn, const double *kn, const double *Sn,
                   const double *Kp, const double *kp, const double *Sp, const double *Sip,
                   double *kldiv, double *klmean);

/* The dual variable η of the KL constraint, per trajectory, on the device: calc_η (src/klutils.jl:112-133, scalar kl_step) and the
 * bracket / retry / exit logic of the iLQGkl loop (src/iLQGkl.jl:91-122,141,169-177).  All arrays are device pointers owned by
 * the caller; `eta` is what ddp_kl_cost_terms.eta points at.  A host loop is
 *     begin(it) -> n_live;  do { back_pass_gps;  retry(diverge) -> n_pending } while (n_pending);
 *     forward_pass; forward_covariance; kl_div;  update(klmean) -> n_live
 * and only those counts cross PCIe.  A trajectory that has left (status 1/2) keeps its `eta`, so recomputing it with the
 * others reproduces its results.                                                                                      */
typedef struct {
    double  *etab;        /* [3,B]  ηbracket of every trajectory (in/out)                                              */
    double  *eta;         /* [B]    η of the next / last back pass                                                     */
    double  *del;         /* [B]    del (iLQGkl.jl:54,103-105), initialised to del0                                    */
    double  *divergence;  /* [B]    mean KL divergence at the last update                                              */
    int32_t *satisfied;   /* [B]                                                                                       */
    int32_t *status;      /* [B]    0 running, 1 constraint satisfied (:169), 2 η > 0.999 ηmax (:174)                  */
    int32_t *live;        /* [B]    1 while the trajectory iterates (initialise to 1)                                  */
    int32_t *pend;        /* [B]    scratch: still needs a back pass in this iteration                                 */
    int32_t *iters;       /* [B]    last iteration the trajectory took part in                                         */
    int32_t *nback;       /* [B]    back passes spent                                                                  */
} ddp_kl_dual;
int ddp_kl_dual_begin_f64_dev(ddp_handle h, int B, int it, const ddp_kl_dual *s, int *n_live);
int ddp_kl_dual_retry_f64_dev(ddp_handle h, int B, const ddp_kl_dual *s, const int32_t *diverge, int *n_pending);
int ddp_kl_dual_update_f64_dev(ddp_handle h, int B, double kl_step, const ddp_kl_dual *s, const double *klmean, int *n_live);

/* One kl_step per trajectory for every iLQGkl loop of the handle (registered and user problems, fitted tables, a cost model) and for
 * ddp_kl_dual_update_f64_dev: steps[B], finite (a non-finite entry is refused by name); the handle keeps its own device copy, and
 * while it is set the update of the dual variable reads steps[b] in place of the scalar kl_step of the call — also in calc_η's
 * `kl_step > 0` test.  steps == NULL clears the table (B is not read).  A loop whose B differs from the table's is refused by name
 * before any launch.  This is one step per TRAJECTORY; the reference's per-time-step meaning of a vector kl_step belongs to
 * constrain_per_step, which is not offloaded.  No struct changes its layout.                                                   */
int ddp_kl_set_steps_f64(ddp_handle h, int B, const double *steps);
int ddp_kl_set_steps_f64_dev(ddp_handle h, int B, const double *steps);

/* The step rule of a guided-policy-search round, per trajectory, from three results of ddp_expected_cost_* (below): ec_prev[N,B] the
 * old policy on the old models, ec_pred[N,B] the new policy on the old models, ec_act[N,B] the new policy on the new models.  With
 * J = sum_i ec[i,b] in ascending i:  pred = J_prev - J_pred,  act = J_prev - J_act,
 *   mult[b] = clip(pred / (2 max(1e-4, pred - act)), 0.1, 5)   (0.1 when one of the three J is not finite),
 *   kl_step_new[b] = clip(kl_step[b] mult[b], step_min, step_max),   kl_step[B], 0 < step_min <= step_max finite.
 * One thread per trajectory (kl.hip): a device-resident round reads nothing back here; kl_step_new goes to ddp_kl_set_steps_*_dev. */
int ddp_kl_step_adjust_f64_dev(ddp_handle h, int N, int B, const double *ec_prev, const double *ec_pred, const double *ec_act,
                               const double *kl_step, double step_min, double step_max, double *kl_step_new, double *mult);
int ddp_kl_step_adjust_f64(ddp_handle h, int N, int B, const double *ec_prev, const double *ec_pred, const double *ec_act,
                           const double *kl_step, double step_min, double step_max, double *kl_step_new, double *mult);

/* ---- iLQGkl — replaces iLQGkl(dynamics,costfun,derivs,x0,traj_prev,model; kl_step,lims,max_iter,cost,ηbracket,del0) ------------
 * reference: src/iLQGkl.jl:25-178,234-252 (single KL constraint; the per-time-step branch :180-232 cannot run upstream), called from
 * src/demo_linear.jl:124.  The whole loop — derivs, ∇kl, back_pass_gps until the KL-regularised Quu is positive definite (η += del;
 * del *= 2), forward_pass(α = 1), forward_covariance, kl_div_wiki, calc_η, the exit tests — runs on device-resident arrays with one η
 * bracket per trajectory; the registered problem `p` stands in for the three closures, the model is the arrays `df(model,·)` /
 * `covariance(model,·)` would return.
 * inputs : x0[n,N,B] pre-rolled trajectory (:66-73), cost0[B] = sum(cost) of it (NULL: costfun(x0,u); the reference insists on `cost`),
 *          traj_prev = Kp[m,n,N,B], kp[m,N,B] (the previous controls u, :45), Sp / Sip[m,m,N,B]; model_fx[n,n,N] or [n,n,N,B], R1[n,n];
 *          lims[m,2] or NULL; etab[3,B] in/out (NULL: o->etabracket for every trajectory)
 * outputs: x[n,N,B] u[m,N,B] (traj_new.k = copy(u), :239) K[m,n,N,B] Sigma = inv(Quu) and Sigmai = Quu [m,m,N,B] Vx Vxx cost[CL,B] dV[2,B]
 *          stats[DDP_ILQGKL_NSTATS,B] = [status (1 SUCCESS :169, 2 η > ηmax :174, 3 max_iter :234), iter, n_backpass, satisfied,
 *          ηmin, η, ηmax, divergence, sum(cost), Δcost (:135), expected_reduction (:136), grad_norm (:125)]; *iters = batch-level iterations */
typedef struct {
    double kl_step;        /* 1                */
    int    max_iter;       /* 50               */
    double etabracket[3];  /* 1e-8, 1, 1e16    */
    double del0;           /* 1e-4             */
} ddp_ilqgkl_opts;
void ddp_ilqgkl_default_opts(ddp_ilqgkl_opts *o);
#define DDP_ILQGKL_NSTATS 12
int ddp_ilqgkl_f64_dev(ddp_handle h, const ddp_problem *p, const ddp_ilqgkl_opts *o, const double *x0, const double *cost0,
                       const double *Kp, const double *kp, const double *Sp, const double *Sip,
                       const double *model_fx, int model_fx_batched, const double *R1, const double *lims, double *etab,
                       double *x, double *u, double *K, double *Sigma, double *Sigmai, double *Vx, double *Vxx, double *cost,
                       double *dV, double *stats, int *iters);
int ddp_ilqgkl_f64(ddp_handle h, const ddp_problem *p, const ddp_ilqgkl_opts *o, const double *x0, const double *cost0,
                   const double *Kp, const double *kp, const double *Sp, const double *Sip,
                   const double *model_fx, int model_fx_batched, const double *R1, const double *lims, double *etab,
                   double *x, double *u, double *K, double *Sigma, double *Sigmai, double *Vx, double *Vxx, double *cost,
                   double *dV, double *stats, int *iters);

/* ---- user-defined problems: the user's f / costfun / df as HIP device source, compiled at run time for gfx950 ---------------------
 * The reference's entry point is iLQG(f, costfun, df, x0, u0; ...) with the user's own closures.  Here the user writes four plain
 * device functions; the library puts its kernel templates around them and compiles the program with hiprtc (loaded with dlopen at
 * first use: no link-time dependency; without it these entry points return < 0).  Before the user's source the library #defines
 * DDP_N, DDP_M, DDP_NP (state / control / parameter counts, compile-time constants), DDP_TERMINAL and DDP_CONST_HESSIAN (0 / 1).
 * The source must not #include <hip/hip_runtime.h> (hiprtc provides it).  All arrays are column-major, i is the 0-based time step:
 *
 *   __device__ void   dynamics(const double *x, const double *u, int i, const double *p, double *xnext);     f(x, u, i+1)
 *   __device__ double stage_cost(const double *x, const double *u, int i, const double *p);                 costfun column i < N
 *   __device__ double terminal_cost(const double *x, const double *p);       DDP_USER_TERMINAL only: cost[N] on x[:,N-1], CL = N+1
 *   __device__ void   derivatives(const double *x, const double *u, int i, int N, const double *p,         df column i
 *                                 double *fx, double *fu, double *cx, double *cu, double *cxx, double *cxu, double *cuu);
 *            fx[n,n] fu[n,m] cx[n] cu[m] cxx[n,n] cxu[n,m] cuu[m,m]; every entry must be written (the buffers are not cleared).
 *            With DDP_USER_CONST_HESSIAN the cxx / cxu / cuu written here are discarded.
 *   __device__ void   cost_hessians(const double *p, double *cxx, double *cxu, double *cuu);               DDP_USER_CONST_HESSIAN only:
 *            evaluated once per trajectory per solve; the backward pass then reads cxx[n,n,B] cxu[n,m,B] cuu[m,m,B].
 *
 * `p` points at the trajectory's parameters: params[nparam] shared by the batch (params_batched = 0) or its column of
 * params[nparam,B] (params_batched = 1); NULL when nparam = 0.  Semantics of the rollout: src/forward_pass.jl:9-33 (u + α k +
 * K diff(x̂, x), clamp to lims[m,2], x̂_{i+1} = f(x̂_i, û_i, i) for i < N-1 — the reference's last call of f is discarded, so it is not
 * made); diff_wrap is the bit mask of ddp_problem::diff_wrap.  Limits: n <= DDP_MAX_N_USER, m <= DDP_MAX_M (with DDP_USER_WAVE:
 * n <= DDP_MAX_N_USER_WAVE, m <= DDP_MAX_M_WIDE), nparam <= DDP_USER_MAX_NPARAM;
 * anything else is refused before compiling.  A problem is compiled once per (source, n, m, nparam, flags) and handle: the handle keeps
 * the module until ddp_destroy.  Kernel names (rocprofv3, ddp_last_kernel): ddp_user_rollout, ddp_user_df, ddp_user_cost,
 * ddp_user_hessians.
 *
 * The terminal cost at the last step: `derivatives` at i == N-1 adds the gradient and Hessian in x of terminal_cost(x[:,N-1]) to cx
 * and cxx (the backward pass has no separate terminal term; user_examples/pendcart.hip's w = 2 and car.hip follow this).
 *
 * DDP_USER_AUTODIFF: df by forward-mode automatic differentiation on the device.  The model functions are templates over the scalar
 * type T of x and u, and `derivatives` is neither required nor called (a definition is ignored):
 *
 *   template <class T> __device__ void dynamics(const T *x, const T *u, int i, const double *p, T *xnext);
 *   template <class T> __device__ T    stage_cost(const T *x, const T *u, int i, const double *p);
 *   template <class T> __device__ T    terminal_cost(const T *x, const double *p);                       with DDP_USER_TERMINAL
 *
 * p, i and N stay plain; every intermediate that depends on x or u must be a T.  T = double in the rollout and cost kernels (the
 * same code as a non-template model) and a dual number in ddp_user_df_ad, which writes what `derivatives` would: fx = ∂f/∂x,
 * fu = ∂f/∂u at (x_i, u_i, i); cx, cu, cxx, cxu, cuu of stage_cost, plus, with DDP_USER_TERMINAL at i == N-1, the gradient and
 * Hessian of terminal_cost in x.  cxx and cuu are exactly symmetric (one triangle is evaluated and mirrored).  With
 * DDP_USER_AUTODIFF | DDP_USER_CONST_HESSIAN only fx, fu, cx, cu are derived (first-order passes) and cost_hessians stays.  A T
 * supports + - * / (with T, double or int on either side), unary -, += -= *= /=, comparisons on the value, and
 *   sin cos tan exp log sqrt pow (T^double, T^int, T^T, double^T) tanh sinh cosh atan atan2 asin acos fabs fmin fmax hypot
 *   expm1 log1p, and rint floor (derivative 0);
 * any other function of a T fails to compile, with its name in ddp_user_compile_log().  Kernel name: ddp_user_df_ad, in place of
 * ddp_user_df.
 *
 * DDP_USER_PLANT: the true system of the closed loop (ddp_user_ilqg_mpc_*; every other entry point ignores the flag), for a solver that
 * plans with the model while the system it controls differs (mass, actuator gain, drift, a known disturbance sequence):
 *
 *   __device__ void   plant(const double *x, const double *u, int t, const double *p, double *xnext);
 *
 * t is the 0-based closed-loop step and p the trajectory's parameter column, the one the model sees: plant-only parameters go into the
 * same params (after the model's, for instance; a disturbance sequence indexed by t included).  plant is a plain double function, also
 * with DDP_USER_AUTODIFF (it may call dynamics<double>).  After every solve t of a trajectory that did not diverge at its start (the
 * last one included) xcl[:,t+1] = plant(xcl[:,t], ucl[:,t], t, p) replaces x_1 of the plan, and is the next solve's initial state.  A
 * plant that leaves the state non-finite or beyond the bound of the initial rollout ends the trajectory's loop through the initial-
 * divergence exit of the next solve.  Kernel name: ddp_user_plant (one lane per slot; ddp_last_kernel(h, 4)).
 *
 * DDP_USER_SECOND_ORDER: full DDP, the second-order backward pass of the reference (backward_pass.jl:81-160) in every iLQG-type solve
 * of the problem (ddp_user_ilqg_*, ddp_user_ilqg_queue_*, ddp_user_ilqg_mpc_*).  It needs DDP_USER_AUTODIFF (the templates; refused
 * otherwise) and nothing else from the user.  With T_i[k,a,b] = ∂²f_k/∂z_a∂z_b at (x_i, u_i, i), z = [x; u], and
 * H_i = Σ_k Vx_{i+1}[k] T_i[k] split as Hxx, Hux, Huu:  Qxx += Hxx, Qux += Hux, Quu[:,:,i] += Huu, and the same Hux, Huu go into
 * Qux_reg and QuuF (:106-123); everything after that is the shared tail (:28-79) — the first-order pass with the cost Hessians of step
 * i replaced by cxx + Hxx, cxu + Hux', cuu + Huu; the stored Quu includes Huu; the last step has no dynamics (Vx = cx, Vxx = cxx).
 * The λ schedule, line search and exits of the driver are untouched: an indefinite QuuF is a `diverge` like any other.  No tensor is
 * formed: H_i is the Hessian of the scalar Vx_{i+1}·f(z), one call of `dynamics` per pair a <= b on a dual over a dual, inside the
 * recursion (kernel ddp_user_back_pass2, one wave per trajectory; ddp_last_kernel(h, 0)).  ddp_user_ilqgkl_* refuses such a problem
 * (back_pass_gps has no second-order variant).  A problem without the flag compiles and runs exactly as before.  Shapes: n <= 32,
 * m <= 8 (the kernel holds the step in 64 KB of LDS); larger problems take DDP_USER_SECOND_ORDER_WAVE.
 *
 * DDP_USER_SECOND_ORDER_WAVE: the same full DDP at the shapes of DDP_USER_WAVE, 1 <= n <= 64 and 1 <= m <= 32.  It needs DDP_USER_WAVE
 * and DDP_USER_AUTODIFF (each refused by name when missing) and excludes DDP_USER_SECOND_ORDER; it combines with DDP_USER_TERMINAL,
 * DDP_USER_CONST_HESSIAN, DDP_USER_PLANT and diff_wrap as DDP_USER_WAVE does.  Semantics are those of DDP_USER_SECOND_ORDER to the
 * letter (Hxx, Hux, Huu, the regularised variants, the tail, `diverge`, `active`, per-trajectory λ, lims[0] > lims[m] = no limits read on
 * the device).  Kernel ddp_user_back_pass2_wave (ddp_last_kernel(h, 0)): the step of back_pass_wide — one work-group of four waves per
 * trajectory, products on the fp64 matrix cores, Cholesky and box-QP across the lanes of a wave — compiled with n, m as constants, with
 * the curvature phase in front of it: the (n+m)(n+m+1)/2 pairs dealt over the 256 threads, H_i handed to the products through an
 * [n+m, n+m] scratch per trajectory that the problem owns (allocated at the first pass, freed by ddp_user_destroy).  ddp_user_vhess_*
 * and ddp_user_back_pass_* take such a problem as they take a DDP_USER_SECOND_ORDER one (ddp_user_vhess unchanged); ddp_user_ilqgkl_*
 * refuses it the same way, with ddp_kl_set_wide on or off.  user_examples/chain_ddp_ad.hip is a model with curvature in x and u at
 * every m (n = 2 m, 8 parameters).  Bit 64 of the flags is not assigned and stays refused as unknown.
 *
 * DDP_USER_WAVE: large problems, 1 <= n <= DDP_MAX_N_USER_WAVE (64) and 1 <= m <= DDP_MAX_M_WIDE (32), the shapes the backward-pass
 * kernels hold.  The user's functions and the argument lists do not change; the library compiles other kernels around them, in which no
 * lane holds a vector of n or a matrix of m x n doubles of the library's own:
 *   ddp_user_rollout_wave   a group of 8, 16 or 32 lanes (the power of two >= m) per (trajectory, alpha) rollout; the state, diff(x^, x),
 *                           the control and the successor state live in LDS, lane q of the group streams row q of K_i from memory, one
 *                           lane of the group calls stage_cost and dynamics (their x, u and xnext then point into LDS).  Semantics and
 *                           the order of every sum are those of ddp_user_rollout (ddp_last_kernel(h, 1)).
 *   ddp_user_df_wave        with DDP_USER_AUTODIFF: one wave per (step, trajectory), one seed direction of z = [x; u] per lane and round
 *                           (ceil((n + m) / 64) rounds; `dynamics` is instantiated once); cx, cu from the same pass of stage_cost; the
 *                           Hessians from one call of stage_cost per pair a <= b on a dual over a dual, dealt over the lanes, each
 *                           value stored to (a, b) and (b, a): cxx and cuu are exactly symmetric.  DDP_USER_CONST_HESSIAN skips the
 *                           pairs: the fast path for quadratic costs (ddp_last_kernel(h, 2)).
 *   ddp_user_df             hand-written `derivatives` under the flag: one lane per (step, trajectory), writing straight into the
 *                           output arrays in memory (discarded Hessians go to a dump area in LDS).  At large shapes this is slower
 *                           than ddp_user_df_wave: prefer DDP_USER_AUTODIFF there.
 *   ddp_user_hessians       cost_hessians writes straight into cxx, cxu, cuu in memory.
 * The flag is legal at every shape (n <= 32, m <= 8 included: the same arithmetic on the other kernels) and with DDP_USER_TERMINAL,
 * DDP_USER_CONST_HESSIAN, DDP_USER_AUTODIFF and DDP_USER_PLANT.  DDP_USER_SECOND_ORDER | DDP_USER_WAVE is refused (ddp_user_back_pass2
 * is sized for n <= 32, m <= 8; full DDP at these shapes is DDP_USER_SECOND_ORDER_WAVE, above), and ddp_user_ilqgkl_* refuses a problem with n > 32 or m > 8 before any launch unless the handle's
 * ddp_kl_set_wide switch is on (back_pass_gps has no kernel there otherwise).  diff_wrap names coordinates below 32 only.  The backward pass of a solve is the one ddp_back_pass_f64 chooses for
 * the shape (32 < n <= 64, m <= 8: the MFMA kernels; m > 8: back_pass_wide).  user_examples/chain_ad.hip is a model with 7 parameters
 * at every size.  A problem without the flag compiles the text it always did and refuses n > 32, m > 8.
 *
 * DDP_USER_CLOCK: absolute time for a time-varying model (a reference that moves, a moving obstacle, a gain or disturbance schedule
 * sampled in params), also where the solve is one of many in a closed loop or a queue.  Every trajectory has a clock c, an int32, and
 * the user's functions take the absolute step t = c + i as one more int behind i:
 *
 *   __device__ void   dynamics(const double *x, const double *u, int i, int t, const double *p, double *xnext);
 *   __device__ double stage_cost(const double *x, const double *u, int i, int t, const double *p);
 *   __device__ double terminal_cost(const double *x, int t, const double *p);                              t = c + N - 1
 *   __device__ void   derivatives(const double *x, const double *u, int i, int t, int N, const double *p, double *fx, ...);
 *
 * and the templates of DDP_USER_AUTODIFF the same way.  i and N keep their meaning (i == N-1 is still the terminal step);
 * cost_hessians(p, ...) is unchanged (constant per solve by its contract); plant keeps its signature, and its t is absolute under the
 * flag: t0 + s at closed-loop step s.  The clocks come from ddp_user_set_t0 (below): none (the state after ddp_user_create: every clock
 * is 0), one value for every trajectory, or one per trajectory (per problem of the queue); a call whose batch or problem count is
 * neither 1 nor that count is refused before any launch.  Clock of trajectory or problem b:
 *   ddp_user_forward_pass_*, ddp_user_df_*, ddp_user_costfun_*, ddp_user_ilqg_*, ddp_user_ilqgkl_*     c = t0[b]
 *   ddp_user_ilqg_queue_*    the slot that takes problem p runs with c = t0[p]
 *   ddp_user_ilqg_mpc_*      the solve at closed-loop step s of trajectory b runs with c = t0[b] + s, the plant call after it gets
 *                            t = t0[b] + s; the clock advances on the device, where the slot is armed again (no host work per step)
 * Legal with DDP_USER_TERMINAL, DDP_USER_CONST_HESSIAN, DDP_USER_AUTODIFF, DDP_USER_PLANT, DDP_USER_WAVE and diff_wrap.  Together with
 * DDP_USER_SECOND_ORDER or DDP_USER_SECOND_ORDER_WAVE it is refused by name: their backward kernels evaluate the model inside the
 * recursion and would have to carry the clock as well — deferred, not impossible.  The kernels are the ones of a problem without the
 * flag (same names, same text, with t handed on at every call of the user's functions); such a problem compiles and runs exactly as
 * before.  user_examples/car_track.hip, car_track_ad.hip and car_track_plant.hip follow a sampled reference past a moving obstacle.
 * Bits 64 and 256 of the flags are not assigned and stay refused as unknown.
 *
 * DDP_USER_CONSTRAINTS: inequality constraints on the state, or on state and control together (a keep-out disc, a speed cap, a
 * corridor), handled by an augmented Lagrangian around the iLQG solve.  The source also defines
 *
 *   template <class T> __device__ void constraints(const T *x, const T *u, int i, const double *p, T *g);   g[nc], feasible: g[j] <= 0
 *
 * evaluated at every stage i = 0..N-1 on (x_i, u_i), which covers every state of the horizon; nc <= DDP_USER_MAX_NC reaches the
 * library through ddp_user_check_c / ddp_user_create_c (the entries without `_c` refuse the flag by name).  Every kernel of such a
 * problem evaluates, in place of stage_cost, the user's stage cost plus the Powell-Hestenes-Rockafellar term
 *   psi = sum_j (max(0, lambda_ij + mu g_j)^2 - lambda_ij^2) / (2 mu)   for mu > 0,   0 for mu <= 0
 * with multipliers lambda[nc,N,B] and a penalty mu[B] per trajectory: those of ddp_user_set_multipliers (none set: mu = 0, the raw
 * cost) in ddp_user_df_*, ddp_user_forward_pass_*, ddp_user_costfun_* and ddp_user_ilqg_*, and the loop's own in ddp_user_ilqg_al_*.
 * The user's indices into p are unchanged (the library appends two slots of its own behind the nparam parameters).  The flag needs
 * DDP_USER_AUTODIFF (the augmented cost is differentiated by AD) and combines with DDP_USER_TERMINAL, DDP_USER_WAVE, DDP_USER_PLANT and
 * diff_wrap; with DDP_USER_CONST_HESSIAN, DDP_USER_CLOCK, DDP_USER_SECOND_ORDER or DDP_USER_SECOND_ORDER_WAVE it is refused by name, and
 * ddp_user_ilqg_queue_*, ddp_user_ilqg_mpc_* and ddp_user_ilqgkl_* refuse such a problem by name before any launch.  Equality
 * constraints are not offered.  user_examples/car_keepout_ad.hip keeps the car out of a disc and caps its speed.
 *
 * DDP_USER_SAMPLE: sampled closed-loop rollouts of a time-varying linear-Gaussian policy (ddp_user_sample_*, below; every other entry
 * point ignores the flag) — the sampling step of the guided-policy-search loop, and, without noise, "run this policy on the plant".
 * S samples of every trajectory b run
 *   u^ = u_i + L_i xi_i + K_i diff(x^, x_i), clamped to lims;  c_i = stage_cost(x^, u^, i, p);  x^ <- dynamics(x^, u^, i, p), i < N-1
 * (src/forward_pass.jl:17-28 with the noise of iLQGkl's docstring; with use_plant = 1 the user's plant(x^, u^, i, p, .) of
 * DDP_USER_PLANT takes the place of dynamics), L_i the LOWER Cholesky factor of Sigma_i and xi_i standard normal.  The reference's
 * chol(Sigma)*randn(m) uses the upper factor U, whose samples have covariance U U', not Sigma, for m > 1: the lower factor is a
 * deliberate deviation (L xi has covariance Sigma).  xi is generated inside the kernel and never stored: Philox4x32-10 (Salmon et al.,
 * SC'11; multipliers 0xD2511F53, 0xCD9E8D57, key increments 0x9E3779B9, 0xBB67AE85), one call per (step, sample, trajectory, pair) with
 *   counter = (i, sample0 + s, traj0 + b, q),  key = (seed_lo, seed_hi)
 * and from its words r0..r3: k1 = (r0 >> 5) 2^26 + (r1 >> 6), k2 = (r2 >> 5) 2^26 + (r3 >> 6), u1 = (k1 + 1) 2^-53 in (0, 1],
 * u2 = k2 2^-53 in [0, 1), xi[2q] = sqrt(-2 log u1) cos(2 pi u2), xi[2q+1] = sqrt(-2 log u1) sin(2 pi u2) (dropped when 2q+1 == m).
 * Nothing depends on the launch geometry, S, B or the device: a call that passes its own sample0 / traj0 reproduces its slice of the
 * full call bit for bit.  Kernel ddp_user_sample (ddp_last_kernel(h, 1)): one lane per sample, all lanes of a work-group on one
 * trajectory, u_i, x_i, K_i, L_i through LDS once per work-group (broadcast reads), the state in registers, results out through LDS in
 * contiguous runs; n <= 32, m <= 8.  Legal with DDP_USER_TERMINAL, DDP_USER_CONST_HESSIAN, DDP_USER_AUTODIFF, DDP_USER_PLANT,
 * DDP_USER_SECOND_ORDER and diff_wrap.  Together with DDP_USER_WAVE (and so DDP_USER_SECOND_ORDER_WAVE), DDP_USER_CLOCK or
 * DDP_USER_CONSTRAINTS it is refused by name — deferred, not impossible.  A problem without the flag compiles the text it always did.
 *
 * DDP_USER_FITTED: the rollout, and the whole KL-constrained loop, on a fitted time-varying affine model in place of `dynamics` and
 * `derivatives` (ddp_user_rollout_fit_*, ddp_user_ilqgkl_fit_*, below; every other entry point ignores the flag): the tables
 * fx[n,n,N,B], fu[n,m,N,B], fc[n,N,B] that ddp_fit_dynamics_* returns, column-major, one set per trajectory,
 *   u^_i = clamp(u_i + alpha k_i + K_i diff(x^_i, x_i));  c_i = stage_cost(x^_i, u^_i, i, p);
 *   x^_{i+1} = fc_i + sum_j fx_i[:,j] x^_i[j] + sum_q fu_i[:,q] u^_i[q],  i < N-1
 * with the user's own cost (and terminal cost).  The affine map acts on raw coordinates: diff_wrap applies in the policy term only.
 * Slot N-1 of the tables is never read.  Per component the sum runs fc, j = 0..n-1, q = 0..m-1: nothing depends on B, nalpha or the
 * launch geometry, and a call on a slice of the trajectories reproduces that slice of the full call bit for bit.  Kernel
 * ddp_user_rollout_fit (ddp_last_kernel(h, 1)): one lane per rollout, the state in registers, the tables staged through LDS in
 * contiguous runs per trajectory and chunk of steps, shared by the alpha candidates of a trajectory that sit in one work-group;
 * n <= 32, m <= 8.  Legal with DDP_USER_TERMINAL, DDP_USER_CONST_HESSIAN, DDP_USER_AUTODIFF, DDP_USER_PLANT, DDP_USER_SAMPLE,
 * DDP_USER_SECOND_ORDER and diff_wrap.  Together with DDP_USER_WAVE (and so DDP_USER_SECOND_ORDER_WAVE), DDP_USER_CLOCK or
 * DDP_USER_CONSTRAINTS it is refused by name — deferred, not impossible.  A problem without the flag compiles the text it always did;
 * the tail of the flag goes last in the program.
 *
 * DDP_USER_COST_FIT: the quadratic cost model of a guided-policy-search round (Levine & Abbeel 2014), fitted to the samples the
 * dynamics model is fitted to (ddp_user_cost_fit_*, below; every other entry point ignores the flag).  For every step i and trajectory b,
 * over the samples s = 0..S-1 of xs[n,N,S,B], us[m,N,S,B] around the nominal x[n,N,B], u[m,N,B], with dx = diff(x^_s, x_i) (diff_wrap,
 * as in the rollout's policy term), du = u^_s - u_i and (c, cx, cu, cxx, cxu, cuu) the user's cost and its derivatives at
 * (x^_s, u^_s, i) — `derivatives`, forward-mode AD of the cost alone with DDP_USER_AUTODIFF, `cost_hessians` with
 * DDP_USER_CONST_HESSIAN, at i = N-1 whatever `derivatives` adds there and c = stage_cost + terminal_cost (DDP_USER_TERMINAL):
 *   cxx_i = mean_s cxx,  cxu_i = mean_s cxu,  cuu_i = mean_s cuu,
 *   cx_i = mean_s (cx - cxx dx - cxu du),  cu_i = mean_s (cu - cxu' dx - cuu du),
 *   c0_i = mean_s (c - cx.dx - cu.du + 1/2 [dx; du]' H [dx; du]),
 * every expansion moved to the nominal before it is averaged.  Every sum runs s = 0..S-1 in that order and is divided by S at the end;
 * inside a sample the sums run j = 0..n-1, then q = 0..m-1: nothing depends on S, B or the launch geometry, two calls give the same
 * bits and a call on a slice of the trajectories reproduces that slice of the full call bit for bit.  A non-finite sample makes the
 * outputs of its own (i, b) non-finite and touches nothing else.  Kernel ddp_user_cost_fit (ddp_last_kernel(h, 1)): one lane per
 * (step, trajectory), the derivatives of a sample and the running sums in the lane's LDS slots, the samples staged through LDS in
 * contiguous runs over the steps of a work-group; no per-sample array exists in memory; n <= 32, m <= 8.  Legal with
 * DDP_USER_TERMINAL, DDP_USER_CONST_HESSIAN, DDP_USER_AUTODIFF, DDP_USER_PLANT, DDP_USER_SAMPLE, DDP_USER_FITTED,
 * DDP_USER_SECOND_ORDER and diff_wrap.  Together with DDP_USER_WAVE (and so DDP_USER_SECOND_ORDER_WAVE), DDP_USER_CLOCK or
 * DDP_USER_CONSTRAINTS it is refused by name — deferred, not impossible.  A problem without the flag compiles the text it always did;
 * the tail of the flag goes last in the program, behind that of DDP_USER_FITTED.
 *
 * DDP_USER_SAMPLE_WAVE: the sampled rollouts of DDP_USER_SAMPLE at the shapes of DDP_USER_WAVE, n <= 64, m <= 32 (ddp_user_sample_*,
 * below; every other entry point ignores the flag).  A flag of its own, which needs DDP_USER_WAVE: DDP_USER_SAMPLE | DDP_USER_WAVE stays
 * refused, as DDP_USER_SECOND_ORDER | DDP_USER_WAVE is next to DDP_USER_SECOND_ORDER_WAVE.  The step, the noise, the generator and its
 * counter, the status and the NaN rows are those of DDP_USER_SAMPLE, word for word; nothing depends on the launch geometry, S or B.
 * Kernel ddp_user_sample_wave (ddp_last_kernel(h, 1)): a group of lanes per sample (8, 16 or 32: the power of two >= m), 64 / group
 * samples per one-wave work-group, every group of a work-group on one trajectory; x^, diff(x^, x_i), u^ and xi_i in LDS; lane q of
 * the group draws the Philox pair q of the step and forms row q of u^ = u_i, + sum_c L_i[q,c] xi_c (c ascending), + sum_l K_i[q,l] dx_l
 * (l ascending), clamp — the order of ddp_user_sample — streaming row q of K_i and L_i from memory; one lane of the group calls the
 * user's stage_cost and dynamics (or plant) on the LDS vectors; results leave in contiguous runs written by the group.  The noise
 * factor of 8 < m <= 32 is ddp_policy_factor_wide (one wave per Sigma_i, a row per lane, left-looking).  Legal with DDP_USER_TERMINAL,
 * DDP_USER_CONST_HESSIAN, DDP_USER_AUTODIFF, DDP_USER_PLANT, DDP_USER_SECOND_ORDER_WAVE and diff_wrap.  Without DDP_USER_WAVE, or
 * together with DDP_USER_CLOCK or DDP_USER_CONSTRAINTS, it is refused by name — the last two deferred, not impossible.  A problem
 * without the flag compiles the text it always did; the tail of the flag goes last in the program.  user_examples/chain_plant_ad.hip is
 * chain_ad.hip with a plant (an actuator gain per joint, another damping; 9 parameters), for use_plant = 1 at these sizes.
 *
 * DDP_USER_FITTED_WAVE: the rollout on a fitted model, and the KL-constrained loop on it, of DDP_USER_FITTED at the shapes of
 * DDP_USER_WAVE, n <= 64, m <= 32 (ddp_user_rollout_fit_*, ddp_user_ilqgkl_fit_*, ddp_user_ilqgkl_cost_*, below; every other entry point
 * ignores the flag).  A flag of its own, which needs DDP_USER_WAVE: DDP_USER_FITTED | DDP_USER_WAVE stays refused.  The step, the
 * tables and their layout, map, active, nalpha, has_policy, lims, the fused csum, slot N-1 that is never read and the order of the sum
 * (per component fc, j = 0..n-1, q = 0..m-1) are those of DDP_USER_FITTED, word for word; nothing depends on B, nalpha or the launch
 * geometry.  Kernel ddp_user_rollout_fit_wave (ddp_last_kernel(h, 1)): a group of lanes per rollout (8, 16 or 32: the power of two
 * >= m), 64 / group rollouts per one-wave work-group; x^, diff(x^, x_i) and u^ in LDS; lane q of the group forms row q of
 * u_i + alpha k_i + K_i dx streaming row q of K_i, then rows q, q + group, ... of [fc | fx | fu] against x^ and u^ (the tables are
 * column-major: the lanes of a group read consecutive doubles of every column); one lane of the group calls the user's cost.  Legal
 * with DDP_USER_TERMINAL, DDP_USER_CONST_HESSIAN, DDP_USER_AUTODIFF, DDP_USER_PLANT, DDP_USER_SAMPLE_WAVE, DDP_USER_SECOND_ORDER_WAVE
 * and diff_wrap.  Without DDP_USER_WAVE, or together with DDP_USER_CLOCK or DDP_USER_CONSTRAINTS, it is refused by name — the last two
 * deferred, not impossible.  A problem without the flag compiles the text it always did; the tail of the flag goes last in the
 * program, behind that of DDP_USER_SAMPLE_WAVE. */
#define DDP_MAX_N_USER 32
#define DDP_USER_MAX_NPARAM 4096
#define DDP_MAX_N_USER_WAVE 64   /* with DDP_USER_WAVE: n <= 64, m <= DDP_MAX_M_WIDE */
enum { DDP_USER_TERMINAL = 1, DDP_USER_CONST_HESSIAN = 2, DDP_USER_AUTODIFF = 4, DDP_USER_PLANT = 8, DDP_USER_SECOND_ORDER = 16,
       DDP_USER_WAVE = 32, DDP_USER_SECOND_ORDER_WAVE = 128, DDP_USER_CLOCK = 512,
       DDP_USER_CONSTRAINTS = 1024, DDP_USER_SAMPLE = 2048, DDP_USER_FITTED = 4096,
       DDP_USER_COST_FIT = 8192, DDP_USER_SAMPLE_WAVE = 16384,
       DDP_USER_FITTED_WAVE = 65536 };                            /* 64: not assigned, refused as unknown (256 and 32768 too) */
#define DDP_USER_MAX_NC 16       /* with DDP_USER_CONSTRAINTS: 1 <= nc <= 16 */
/* compile-only check for gfx950 (no handle, no GPU): 0 = compiled, < 0 = refused or the compiler failed (ddp_user_compile_log()).
 * extra_options: more hiprtc options separated by spaces, or NULL (e.g. "-Rpass-analysis=kernel-resource-usage")               */
int ddp_user_check(const char *source, int n, int m, int nparam, int flags, const char *extra_options);
/* the log of the last compile in this process ("" before the first one) */
const char *ddp_user_compile_log(void);
/* compile (or take from the handle's cache) and load on the handle's device: *out is the problem, used with this handle only */
int ddp_user_create(ddp_handle h, const char *source, int n, int m, int nparam, int flags, int diff_wrap, void **out);
int ddp_user_destroy(void *up);
/* The same two entries with the number of constraints nc (DDP_USER_CONSTRAINTS: 1 <= nc <= DDP_USER_MAX_NC; a problem without the
 * flag: nc = 0, and they do what the entries above do).                                                                        */
int ddp_user_check_c(const char *source, int n, int m, int nparam, int nc, int flags, const char *extra_options);
int ddp_user_create_c(ddp_handle h, const char *source, int n, int m, int nparam, int nc, int flags, int diff_wrap, void **out);
/* DDP_USER_CONSTRAINTS problems only: the multipliers lambda[nc,N,B] and penalties mu[B] of the following ddp_user_df_*,
 * ddp_user_forward_pass_*, ddp_user_costfun_* and ddp_user_ilqg_* calls.  Host pointers, copied; the problem owns the device copies.
 * Both NULL clears them (mu = 0: the raw cost).  A call whose N or B differs from the ones given here is refused before any launch. */
int ddp_user_set_multipliers(void *up, const double *lambda, const double *mu, int N, int B);
/* constraints: x[n,N,B] u[m,N,B] -> g[nc,N,B] (kernel ddp_user_constraints, one lane per step and trajectory)                      */
int ddp_user_constraints_f64_dev(ddp_handle h, void *up, int N, int B, const double *params, int params_batched, const double *x,
                                 const double *u, double *g);
int ddp_user_constraints_f64(ddp_handle h, void *up, int N, int B, const double *params, int params_batched, const double *x,
                             const double *u, double *g);
/* DDP_USER_CLOCK problems only (others are refused by name): the clocks of the following calls.  t0 is a host pointer and is copied;
 * count = 0: every clock is 0; 1: one value for every trajectory; B (P for the queue): one per trajectory or problem.  The problem
 * owns the device copy (ddp_user_destroy frees it).                                                                             */
int ddp_user_set_t0(void *up, const int32_t *t0, int count);
/* df: x[n,N,B] u[m,N,B] -> fx[n,n,N,B] fu[n,m,N,B] cx[n,N,B] cu[m,N,B], cxx[n,n,N,B] cxu[n,m,N,B] cuu[m,m,N,B] (CONST_HESSIAN: [.,.,B]);
 * fx .. cu may not be NULL, the Hessians may (not computed then).  `active` as in ddp_back_pass_f64_dev.                        */
int ddp_user_df_f64_dev(ddp_handle h, void *up, int N, int B, const double *params, int params_batched, const double *x, const double *u,
                        const int32_t *active, double *fx, double *fu, double *cx, double *cu, double *cxx, double *cxu, double *cuu);
int ddp_user_df_f64(ddp_handle h, void *up, int N, int B, const double *params, int params_batched, const double *x, const double *u,
                    double *fx, double *fu, double *cx, double *cu, double *cxx, double *cxu, double *cuu);
/* DDP_USER_SECOND_ORDER and DDP_USER_SECOND_ORDER_WAVE problems only.  vhess: x[n,N,B] u[m,N,B] v[n,N,B] -> H[n+m,n+m,N,B] = Σ_k v[k,i,b] ∂²f_k/∂z∂z at (x_i, u_i, i),
 * exactly symmetric (kernel ddp_user_vhess, one lane per pair, step and trajectory): the `vectens` terms for a caller of the array API. */
int ddp_user_vhess_f64_dev(ddp_handle h, void *up, int N, int B, const double *params, int params_batched, const double *x, const double *u,
                           const double *v, const int32_t *active, double *H);
int ddp_user_vhess_f64(ddp_handle h, void *up, int N, int B, const double *params, int params_batched, const double *x, const double *u,
                       const double *v, double *H);
/* One second-order backward pass: x, u and the seven derivative arrays as ddp_user_df writes them (Hessians [.,.,B] with
 * DDP_USER_CONST_HESSIAN), lambda[B], regType 1 | 2, lims[m,2] or NULL, `active` -> K, k, Quu, Vx, Vxx, dV[2,B], diverge[B] shaped as
 * ddp_back_pass_f64_dev.  A problem without the flag is refused: its backward pass is ddp_back_pass_f64 on the same arrays.      */
int ddp_user_back_pass_f64_dev(ddp_handle h, void *up, int N, int B, const double *params, int params_batched, const double *x,
                               const double *u, const double *fx, const double *fu, const double *cx, const double *cu, const double *cxx,
                               const double *cxu, const double *cuu, const double *lambda, int regType, const double *lims,
                               const int32_t *active, double *K, double *k, double *Quu, double *Vx, double *Vxx, double *dV,
                               int32_t *diverge);
int ddp_user_back_pass_f64(ddp_handle h, void *up, int N, int B, const double *params, int params_batched, const double *x, const double *u,
                           const double *fx, const double *fu, const double *cx, const double *cu, const double *cxx, const double *cxu,
                           const double *cuu, const double *lambda, int regType, const double *lims, double *K, double *k, double *Quu,
                           double *Vx, double *Vxx, double *dV, int32_t *diverge);
/* forward_pass: arguments and outputs as ddp_forward_pass_f64_dev; cnew[CL,B,nalpha]                                           */
int ddp_user_forward_pass_f64_dev(ddp_handle h, void *up, int N, int B, const double *params, int params_batched,
                                  const double *K, const double *k, const double *x0, const double *u, const double *x,
                                  const double *alpha, int nalpha, const double *lims, const int32_t *active,
                                  double *xnew, double *unew, double *cnew, double *csum);
int ddp_user_forward_pass_f64(ddp_handle h, void *up, int N, int B, const double *params, int params_batched,
                              const double *K, const double *k, const double *x0, const double *u, const double *x,
                              const double *alpha, int nalpha, const double *lims,
                              double *xnew, double *unew, double *cnew, double *csum);
/* costfun(x, u): cost[CL,B], csum[B] (may be NULL)                                                                              */
int ddp_user_costfun_f64_dev(ddp_handle h, void *up, int N, int B, const double *params, int params_batched, const double *x,
                             const double *u, const int32_t *active, double *cost, double *csum);
int ddp_user_costfun_f64(ddp_handle h, void *up, int N, int B, const double *params, int params_batched, const double *x,
                         const double *u, double *cost, double *csum);
/* iLQG with the user's closures: arguments and outputs as ddp_ilqg_ex_f64(_dev) (pre-rolled x0 + cost0, trace7, stats[8,B]);
 * ddp_ilqg_set_timing applies.  The live trajectories are compacted like those of the registered families; the kernels then read
 * params[:, b] through the working set's slot map.                                                                             */
int ddp_user_ilqg_f64_dev(ddp_handle h, void *up, int N, int B, const double *params, int params_batched, const ddp_ilqg_opts *o,
                          const double *x0, int x0_prerolled, const double *u0, const double *cost0, const double *lims,
                          double *x, double *u, double *K, double *k, double *Quu, double *Vx, double *Vxx,
                          double *cost, double *stats, int trace_cap, double *trace7, int *global_iters);
int ddp_user_ilqg_f64(ddp_handle h, void *up, int N, int B, const double *params, int params_batched, const ddp_ilqg_opts *o,
                      const double *x0, int x0_prerolled, const double *u0, const double *cost0, const double *lims,
                      double *x, double *u, double *K, double *k, double *Quu, double *Vx, double *Vxx,
                      double *cost, double *stats, int trace_cap, double *trace7, int *global_iters);
/* The slot scheduler with the user's closures: P solves through `slots` resident trajectories, arguments and outputs as
 * ddp_ilqg_queue_f64(_dev) (x0[n,P], u0[m,N,P]; every solve is the one ddp_user_ilqg_f64 performs at batch size `slots`).  params:
 * [nparam] shared or [nparam,P] one column per problem (params_batched = 1), read through the slot -> problem map.  With
 * DDP_USER_CONST_HESSIAN the Hessians of a slot are evaluated when it takes a problem (ddp_user_hessians on the armed slots).        */
int ddp_user_ilqg_queue_f64_dev(ddp_handle h, void *up, int N, int P, const double *params, int params_batched, const ddp_ilqg_opts *o,
                                int slots, const double *x0, const double *u0, const double *lims,
                                double *x, double *u, double *K, double *k, double *Quu, double *Vx, double *Vxx,
                                double *cost, double *stats, int *global_iters);
int ddp_user_ilqg_queue_f64(ddp_handle h, void *up, int N, int P, const double *params, int params_batched, const ddp_ilqg_opts *o,
                            int slots, const double *x0, const double *u0, const double *lims,
                            double *x, double *u, double *K, double *k, double *Quu, double *Vx, double *Vxx,
                            double *cost, double *stats, int *global_iters);
/* The closed loop with the user's closures: arguments and outputs as ddp_ilqg_mpc_f64(_dev); params [nparam] or [nparam,B] per
 * trajectory.  Without DDP_USER_PLANT the model is the plant (x_1 of the plan is the next state); with it, the user's plant.        */
int ddp_user_ilqg_mpc_f64_dev(ddp_handle h, void *up, int N, int B, const double *params, int params_batched, const ddp_ilqg_opts *o,
                              int steps, int zero_tail, const double *x0, const double *u0, const double *lims,
                              double *xcl, double *ucl, double *stats_cl, double *x, double *u, int *global_iters);
int ddp_user_ilqg_mpc_f64(ddp_handle h, void *up, int N, int B, const double *params, int params_batched, const ddp_ilqg_opts *o,
                          int steps, int zero_tail, const double *x0, const double *u0, const double *lims,
                          double *xcl, double *ucl, double *stats_cl, double *x, double *u, int *global_iters);
/* iLQGkl with the user's closures: arguments, outputs, stats[DDP_ILQGKL_NSTATS,B] and exit codes as ddp_ilqgkl_f64(_dev), with the
 * user problem in place of dynamics / costfun / derivs and params [nparam] shared or [nparam,B] per trajectory (params_batched = 1);
 * cost[CL,B] uses the problem's CL (N+1 with DDP_USER_TERMINAL).  STEP 1 evaluates `derivatives` (or its forward-mode AD) once at
 * (x0, kp) for every trajectory; DDP_USER_CONST_HESSIAN and the compiled diff_wrap apply, DDP_USER_PLANT is ignored.  model_fx == NULL:
 * the model is the problem itself — forward_covariance takes the fx of STEP 1 [n,n,N,B], which is df(model, x, u) of the reference's
 * forward_covariance (the loop never moves x0, kp); R1 is still required.  The backward pass is back_pass_gps on q4 (n = 4, m = 1),
 * lane (n = 4, m = 2) or the mid kernel (every other n <= 32, m <= 8); ddp_last_kernel(h, 0) names it.                            */
int ddp_user_ilqgkl_f64_dev(ddp_handle h, void *up, int N, int B, const double *params, int params_batched, const ddp_ilqgkl_opts *o,
                            const double *x0, const double *cost0, const double *Kp, const double *kp, const double *Sp, const double *Sip,
                            const double *model_fx, int model_fx_batched, const double *R1, const double *lims, double *etab,
                            double *x, double *u, double *K, double *Sigma, double *Sigmai, double *Vx, double *Vxx,
                            double *cost, double *dV, double *stats, int *iters);
int ddp_user_ilqgkl_f64(ddp_handle h, void *up, int N, int B, const double *params, int params_batched, const ddp_ilqgkl_opts *o,
                        const double *x0, const double *cost0, const double *Kp, const double *kp, const double *Sp, const double *Sip,
                        const double *model_fx, int model_fx_batched, const double *R1, const double *lims, double *etab,
                        double *x, double *u, double *K, double *Sigma, double *Sigmai, double *Vx, double *Vxx,
                        double *cost, double *dV, double *stats, int *iters);

/* The augmented-Lagrangian loop of a DDP_USER_CONSTRAINTS problem, per trajectory, round r = 0, 1, ...:
 *   1. the solve of ddp_user_ilqg_f64 under (lambda, mu): round 0 from x0[n,B] (x0_prerolled: x0[n,N,B]) and u0, later rounds pre-rolled
 *      from the last (x, u) with the cost evaluated again under the new multipliers;
 *   2. g = constraints(x, u), cviol = max_ij max(0, g_ij) (kernel ddp_user_al_update, reductions in a fixed order);
 *   3. inner status DDP_EXIT_INIT_DIVERGED in round 0: AL status -1; cviol <= ctol: 1; r + 1 == max_outer: 2; each of them freezes the
 *      trajectory with the multipliers its solution was computed under.  Otherwise lambda <- max(0, lambda + mu g),
 *      mu <- min(mu_factor mu, mu_max), evaluated without contraction.
 * A frozen trajectory's outputs are, bit for bit, those of the round it froze in.  The host reads one counter per round; lambda, mu, x
 * and u stay on the device between rounds.  lambda0[nc,N,B] (NULL: zeros) and mu_init[B] (NULL: mu0 everywhere) are the initial
 * multipliers.  Outputs: those of ddp_user_ilqg_f64 (cost is the augmented one, stats[8,B] those of the last round each trajectory
 * ran; no trace), lambda[nc,N,B], mu[B], g[nc,N,B] at the returned (x, u), and
 *   al_stats[6,B] = [status, rounds, total inner iterations, mu of the last solve, cviol, sum of the raw cost]
 * global_iters (may be NULL): batch-level iterations of all rounds.                                                              */
typedef struct {
    double mu0, mu_factor, mu_max, ctol;
    int max_outer;
} ddp_al_opts;
#define DDP_AL_NSTATS 6
void ddp_al_default_opts(ddp_al_opts *o);      /* mu0 1, mu_factor 10, mu_max 1e8, ctol 1e-5, max_outer 20 */
int ddp_user_ilqg_al_f64_dev(ddp_handle h, void *up, int N, int B, const double *params, int params_batched, const ddp_ilqg_opts *o,
                             const ddp_al_opts *ao, const double *x0, int x0_prerolled, const double *u0, const double *lims,
                             const double *lambda0, const double *mu_init, double *x, double *u, double *K, double *k, double *Quu,
                             double *Vx, double *Vxx, double *cost, double *stats, double *lambda, double *mu, double *g, double *al_stats,
                             int *global_iters);
int ddp_user_ilqg_al_f64(ddp_handle h, void *up, int N, int B, const double *params, int params_batched, const ddp_ilqg_opts *o,
                         const ddp_al_opts *ao, const double *x0, int x0_prerolled, const double *u0, const double *lims,
                         const double *lambda0, const double *mu_init, double *x, double *u, double *K, double *k, double *Quu,
                         double *Vx, double *Vxx, double *cost, double *stats, double *lambda, double *mu, double *g, double *al_stats,
                         int *global_iters);

/* xi[m,N,S,B]: the standard normals ddp_user_sample_* draws for (seed_lo, seed_hi, sample0, traj0) — see DDP_USER_SAMPLE above.  The
 * two seed words are the low and high 32 bits of a 64-bit seed, passed as int (their bits are what counts).  Kernel ddp_normal_fill. */
int ddp_normal_f64_dev(ddp_handle h, int seed_lo, int seed_hi, int m, int N, int S, int B, int sample0, int traj0, double *xi);
int ddp_normal_f64(ddp_handle h, int seed_lo, int seed_hi, int m, int N, int S, int B, int sample0, int traj0, double *xi);
/* DDP_USER_SAMPLE and DDP_USER_SAMPLE_WAVE problems only (others are refused by name).  K[m,n,N,B], Sigma[m,m,N,B] (lower triangle read), x0[n,B], u[m,N,B],
 * x[n,N,B], lims[m,2] or NULL -> xs[n,N,S,B], us[m,N,S,B], cs[CL,S,B], csum[S,B], status[B], and the moments over the samples
 * xmean[n,N,B], xcov[n,n,N,B] (unbiased; S = 1: NaN).  Sigma == NULL: no noise, the deterministic policy rollout (S is usually 1).
 * noise[m,N,S,B] != NULL overrides the seed (ignored without Sigma).  xs, us, xmean, xcov may be NULL; moments without xs are
 * refused by name.  status[b] is 0, or i + 1 for the smallest step whose Sigma_i is not positive definite (a pivot of its Cholesky
 * factorisation that is not a positive finite number): such a trajectory runs no rollout and its rows of every non-NULL output are
 * NaN.  use_plant = 1 on a problem without DDP_USER_PLANT is refused by name.  The noise factors (kernel ddp_policy_factor, for m > 8
 * ddp_policy_factor_wide) live in a buffer the problem owns; the moments are ddp_sample_moments, one wave per step and trajectory, a fixed summation order.        */
int ddp_user_sample_f64_dev(ddp_handle h, void *up, int N, int B, int S, const double *params, int params_batched, const double *K,
                            const double *Sigma, const double *x0, const double *u, const double *x, const double *lims, const double *noise,
                            int seed_lo, int seed_hi, int sample0, int traj0, int use_plant, double *xs, double *us, double *cs, double *csum,
                            double *xmean, double *xcov, int32_t *status);
int ddp_user_sample_f64(ddp_handle h, void *up, int N, int B, int S, const double *params, int params_batched, const double *K,
                        const double *Sigma, const double *x0, const double *u, const double *x, const double *lims, const double *noise,
                        int seed_lo, int seed_hi, int sample0, int traj0, int use_plant, double *xs, double *us, double *cs, double *csum,
                        double *xmean, double *xcov, int32_t *status);

/* The linear-Gaussian dynamics fit of the guided-policy-search round (sample -> fit -> iLQGkl): xs[n,N,S,B], us[m,N,S,B] (the arrays
 * ddp_user_sample_* writes) -> fx[n,n,N,B], fu[n,m,N,B], fc[n,N,B], cov[n,n,N,B], status[N,B], per step i < N - 1 and trajectory b
 * independently.  With w_s = [xs_i; us_i; xs_{i+1}] of sample s (p = 2n + m entries; z the first d = n + m, y the last n):
 *   mu = mean_s w_s,   E = sum_s (w_s - mu)(w_s - mu)'  (the samples are centred before the products),
 *   C = E / (S - 1) without a prior (Phi == NULL: mu0, m0, n0, prior_layout are not read), else the normal-inverse-Wishart posterior
 *   C = (E + Phi + (S m0 / (S + m0)) (mu - mu0)(mu - mu0)') / (S + n0),
 *   A = C_zz + ridge I (ridge >= 0, absolute), A = L L' (the lower triangle is read),
 *   [fx fu] = (A^-1 C_zy)',   fc = mu_y - [fx fu] mu_z,   cov = C_yy - [fx fu] C_zy, symmetrised as (M + M') / 2.
 * prior_layout = 0: one Phi[p,p], mu0[p] for every step and trajectory; 1: Phi[p,p,N,B], mu0[p,N,B] (slot N - 1 is not read).
 * status[i,b] is 0, or c + 1 for the first pivot c of the factorisation that is not a positive finite number: that step's fx, fu, fc,
 * cov are NaN and no other step is touched (every rollout of the sampler starts at the same x0, so C_xx of step 0 is exactly zero:
 * with ridge = 0 and no prior that step reports pivot 1; the mean is formed as w_0 + mean_s (w_s - w_0), which gives a column that
 * is the same in every sample exactly).  A step whose pivots are all fine but whose results are not finite (a NaN in xs_{i+1} of one
 * sample, which is no part of A) fails too, with status d + 1 = n + m + 1.  Slot N - 1 has no transition: zeros, status 0.  1 <= n <= 32, 1 <= m <= 8,
 * S >= 2; anything else is refused by name before any launch.  The summation order is fixed: two calls give the same bits, and a call
 * on a slice of the trajectories gives the bits of that slice of the full call.  kl's Model takes fx, fu as they are.  Kernel
 * ddp_fit_dynamics (fit.hip): one work-group per run of steps of one trajectory, the Gram matrix on v_mfma_f64_16x16x4.          */
int ddp_fit_dynamics_f64_dev(ddp_handle h, int n, int m, int N, int S, int B, const double *xs, const double *us, double ridge,
                             const double *Phi, const double *mu0, double m0, double n0, int prior_layout, double *fx, double *fu,
                             double *fc, double *cov, int32_t *status);
int ddp_fit_dynamics_f64(ddp_handle h, int n, int m, int N, int S, int B, const double *xs, const double *us, double ridge,
                         const double *Phi, const double *mu0, double m0, double n0, int prior_layout, double *fx, double *fu,
                         double *fc, double *cov, int32_t *status);

/* The same fit for large problems, 1 <= n <= 64 (DDP_MAX_N_USER_WAVE), 1 <= m <= 32 (DDP_MAX_M_WIDE): the arguments, layouts, formula,
 * outputs and status of ddp_fit_dynamics_f64(_dev) above; anything outside that box is refused by name before the handle is looked
 * at.  A shape inside the small box (n <= 32 and m <= 8) is handed to ddp_fit_dynamics_f64(_dev) and gives its bits; every other
 * shape runs kernel ddp_fit_dynamics_wide (fit_wide.hip): one work-group per step and trajectory, the Gram matrix, the blocked
 * Cholesky factorisation (16 columns a block) and both substitutions on v_mfma_f64_16x16x4, the matrices as 16 x 16 blocks in
 * dynamic LDS sized from (n, m) (117 KiB at (64, 32)).  cov is formed as C_yy - Y1' Y1 with Y1 = L^-1 C_zy, the same matrix as
 * C_yy - [fx fu] C_zy and symmetric to the bit.  The chunking of the samples and the order of every sum come from (n, m) alone:
 * two calls give the same bits, a call on a slice of the trajectories gives the bits of that slice, and the two flavours agree.  */
int ddp_fit_dynamics_wide_f64_dev(ddp_handle h, int n, int m, int N, int S, int B, const double *xs, const double *us, double ridge,
                                  const double *Phi, const double *mu0, double m0, double n0, int prior_layout, double *fx, double *fu,
                                  double *fc, double *cov, int32_t *status);
int ddp_fit_dynamics_wide_f64(ddp_handle h, int n, int m, int N, int S, int B, const double *xs, const double *us, double ridge,
                              const double *Phi, const double *mu0, double m0, double n0, int prior_layout, double *fx, double *fu,
                              double *fc, double *cov, int32_t *status);

/* DDP_USER_FITTED and DDP_USER_FITTED_WAVE problems only (a problem made without either flag is refused by name).  The rollout of
 * ddp_user_forward_pass_f64(_dev), arguments and outputs alike, on the fitted model fx[n,n,N,B], fu[n,m,N,B], fc[n,N,B] (see
 * DDP_USER_FITTED above; kernel ddp_user_rollout_fit, with DDP_USER_FITTED_WAVE ddp_user_rollout_fit_wave).                           */
int ddp_user_rollout_fit_f64_dev(ddp_handle h, void *up, int N, int B, const double *params, int params_batched,
                                 const double *K, const double *k, const double *x0, const double *u, const double *x,
                                 const double *alpha, int nalpha, const double *lims, const int32_t *active,
                                 const double *fx, const double *fu, const double *fc,
                                 double *xnew, double *unew, double *cnew, double *csum);
int ddp_user_rollout_fit_f64(ddp_handle h, void *up, int N, int B, const double *params, int params_batched,
                             const double *K, const double *k, const double *x0, const double *u, const double *x,
                             const double *alpha, int nalpha, const double *lims,
                             const double *fx, const double *fu, const double *fc,
                             double *xnew, double *unew, double *cnew, double *csum);
/* iLQGkl planning on the fitted model: arguments and outputs as ddp_user_ilqgkl_f64(_dev), then the tables.  The backward pass takes the
 * fitted fx, fu, every rollout of the loop runs ddp_user_rollout_fit, and model_fx == NULL means the fitted fx.  STEP 1 still evaluates
 * the problem's derivatives once at (x0, kp) for the derivatives of the cost; the fx, fu it writes are not used.  The tables must be
 * finite at every step (a step ddp_fit_dynamics_* rejected is NaN: the caller checks its status).  x0 is expected to be the rollout of kp
 * on the tables (ddp_user_rollout_fit_* without a policy), as iLQGkl expects a trajectory consistent with its model.                */
int ddp_user_ilqgkl_fit_f64_dev(ddp_handle h, void *up, int N, int B, const double *params, int params_batched, const ddp_ilqgkl_opts *o,
                                const double *x0, const double *cost0, const double *Kp, const double *kp, const double *Sp,
                                const double *Sip, const double *model_fx, int model_fx_batched, const double *R1, const double *lims,
                                double *etab, const double *fx, const double *fu, const double *fc,
                                double *x, double *u, double *K, double *Sigma, double *Sigmai, double *Vx, double *Vxx,
                                double *cost, double *dV, double *stats, int *iters);
int ddp_user_ilqgkl_fit_f64(ddp_handle h, void *up, int N, int B, const double *params, int params_batched, const ddp_ilqgkl_opts *o,
                            const double *x0, const double *cost0, const double *Kp, const double *kp, const double *Sp,
                            const double *Sip, const double *model_fx, int model_fx_batched, const double *R1, const double *lims,
                            double *etab, const double *fx, const double *fu, const double *fc,
                            double *x, double *u, double *K, double *Sigma, double *Sigmai, double *Vx, double *Vxx,
                            double *cost, double *dV, double *stats, int *iters);

/* DDP_USER_COST_FIT problems only (a problem made without the flag is refused by name).  The cost model of DDP_USER_COST_FIT above:
 * xs[n,N,S,B], us[m,N,S,B] (what ddp_user_sample_* returns), the nominal x[n,N,B], u[m,N,B]; outputs in the layouts of
 * ddp_user_df_f64(_dev), always time-varying and per trajectory (also with DDP_USER_CONST_HESSIAN): cx[n,N,B], cu[m,N,B],
 * cxx[n,n,N,B], cxu[n,m,N,B], cuu[m,m,N,B], and c0[N,B], the model's value at the nominal (sum(c0[:,b]) is comparable with a rollout's
 * csum).  S >= 1.  The host flavour stages its arrays like every host-pointer entry; both give the same bits.                          */
int ddp_user_cost_fit_f64_dev(ddp_handle h, void *up, int N, int S, int B, const double *params, int params_batched, const double *xs,
                              const double *us, const double *x, const double *u, double *cx, double *cu, double *cxx, double *cxu,
                              double *cuu, double *c0);
int ddp_user_cost_fit_f64(ddp_handle h, void *up, int N, int S, int B, const double *params, int params_batched, const double *xs,
                          const double *us, const double *x, const double *u, double *cx, double *cu, double *cxx, double *cxu,
                          double *cuu, double *c0);
/* iLQGkl with a cost model: arguments and outputs as ddp_user_ilqgkl_fit_f64(_dev), then cx[n,N,B], cu[m,N,B], cxx[n,n,N,B],
 * cxu[n,m,N,B], cuu[m,m,N,B] (all five, time-varying and batched), which every backward pass of the loop takes in place of the cost
 * derivatives STEP 1 evaluates at (x0, kp).  fx, fu, fc: all three given — the loop plans on the tables as ddp_user_ilqgkl_fit_* does
 * (a DDP_USER_FITTED or DDP_USER_FITTED_WAVE problem) — or all three NULL — on the problem's own model, as ddp_user_ilqgkl_* does.  Everything else is as
 * without a cost model: cost0, the user's cost of the rollouts (the cost the loop compares and reports) and the loop itself.  The
 * tables need not come from ddp_user_cost_fit_* and the problem needs no DDP_USER_COST_FIT; non-finite tables are the caller's to check. */
int ddp_user_ilqgkl_cost_f64_dev(ddp_handle h, void *up, int N, int B, const double *params, int params_batched, const ddp_ilqgkl_opts *o,
                                 const double *x0, const double *cost0, const double *Kp, const double *kp, const double *Sp,
                                 const double *Sip, const double *model_fx, int model_fx_batched, const double *R1, const double *lims,
                                 double *etab, const double *fx, const double *fu, const double *fc,
                                 double *x, double *u, double *K, double *Sigma, double *Sigmai, double *Vx, double *Vxx,
                                 double *cost, double *dV, double *stats, int *iters,
                                 const double *cx, const double *cu, const double *cxx, const double *cxu, const double *cuu);
int ddp_user_ilqgkl_cost_f64(ddp_handle h, void *up, int N, int B, const double *params, int params_batched, const ddp_ilqgkl_opts *o,
                             const double *x0, const double *cost0, const double *Kp, const double *kp, const double *Sp,
                             const double *Sip, const double *model_fx, int model_fx_batched, const double *R1, const double *lims,
                             double *etab, const double *fx, const double *fu, const double *fc,
                             double *x, double *u, double *K, double *Sigma, double *Sigmai, double *Vx, double *Vxx,
                             double *cost, double *dV, double *stats, int *iters,
                             const double *cx, const double *cu, const double *cxx, const double *cxu, const double *cuu);

/* The dynamics prior of the guided-policy-search round (Levine & Abbeel 2014): a Gaussian mixture over the transition tuples of all
 * steps and samples, and from it the normal-inverse-Wishart prior (Phi, mu0) of every step that ddp_fit_dynamics_* takes with
 * prior_layout = 1.  From xs[n,N,S,B], us[m,N,S,B] the point of (step i < N - 1, sample s, trajectory b) is w = [xs_i; us_i; xs_{i+1}],
 * p = 2n + m entries (the w of ddp_fit_dynamics).  pool = 1: one mixture over all trajectories, G = 1, P = (N - 1) S B points;
 * pool = 0: one per trajectory, G = B, P = (N - 1) S points each.
 *
 * ddp_gmm_fit: K clusters, `iters` EM iterations, reg >= 0 absolute.
 *   M-step from r[j,k]:  N_k = sum_j r_jk,  pi_k = N_k / P,  mu_k = sum_j r_jk w_j / N_k,
 *                        Sigma_k = sum_j r_jk (w_j - mu_k)(w_j - mu_k)' / N_k + reg I   (the products are centred on the new mu_k);
 *   E-step:  Sigma_k = L_k L_k',  lo_jk = log pi_k - (p/2) log 2 pi - sum_c log L_k,cc - |L_k^-1 (w_j - mu_k)|^2 / 2,
 *            lse_j = logsumexp_k lo_jk,  r_jk = exp(lo_jk - lse_j),  ll = sum_j lse_j.
 *   Start: pi0[K,G], mu0[p,K,G], Sigma0[p,p,K,G] when they are given (all three, or all NULL; the lower triangle of Sigma0 is read) —
 *   the warm start of the next round; else an M-step from a hard assignment: the cluster of point (i, s, b) is the first output word of
 *   Philox4x32-10 mod K with counter (i, s, traj0 + b, 0x80000000) and key (seed_lo, seed_hi) (the fourth word keeps the draw off the
 *   sampler's noise stream, whose fourth word is a pair index < 4): independent of the launch geometry and of B.  Then `iters` times
 *   (E-step, M-step); ll[t,g] is the log-likelihood the E-step of iteration t sees; iters = 0 returns the start (ll may be NULL).
 *   Outputs pi[K,G], mu[p,K,G], Sigma[p,p,K,G] (both triangles, exactly symmetric), ll[iters,G], status[G].  Every mixture that is
 *   formed, the start included, is tested: status[g] is 0, or k + 1 for the smallest k whose N_k (pi_k of a start that is given) is
 *   not a positive finite number, whose mu_k of a given start is not finite, or for which a pivot of Sigma_k's factorisation is not a
 *   positive finite number (the pivot test of ddp_user_sample's factorisation).  The first iteration where this happens sets the
 *   status; that mixture's pi, mu, Sigma and the ll of the iterations after it are NaN, and no other mixture is touched.
 *
 * ddp_gmm_prior: per step i < N - 1 and trajectory b, with mixture g = pool ? 0 : b: r_sk of the step's S points by the E-step above,
 *   omega_k = (1/S) sum_s r_sk,  mu0 = sum_k omega_k mu_k,  Phi = n0 sum_k omega_k (Sigma_k + (mu_k - mu0)(mu_k - mu0)'), exactly
 *   symmetric (the lower triangle of Sigma is read) -> Phi[p,p,N,B], mu0[p,N,B], status[N,B]; slot N - 1: zeros, status 0.  status 2:
 *   the mixture is not usable (the test above on the mixture as given); else 1: a point of the step is not finite.  In both cases that
 *   step's Phi, mu0 are NaN and no other step is touched.  m0 is only validated: it goes to ddp_fit_dynamics_* with n0.
 *
 * 1 <= n <= 32, 1 <= m <= 8, 1 <= K <= 32, N >= 2, S >= 1, P >= 2, iters >= 0, reg, m0, n0 finite and >= 0, pool 0 or 1; anything else
 * is refused by name before any launch.  Every sum has a fixed order: two calls give the same bits; with pool = 0 a call on a slice of
 * the trajectories (with its traj0) gives the bits of that slice of the full call, for ddp_gmm_prior in both modes; with pool = 1 the
 * split of the points over work-groups and the order of the final reduction depend on (n, m, K, N, S, B) alone.  The responsibilities
 * (K P doubles), L_k^-1 and the per-work-group partial sums live in the handle's scratch.  Kernels: gmm.hip, the Mahalanobis terms and
 * the weighted Gram matrices on v_mfma_f64_16x16x4.                                                                                 */
int ddp_gmm_fit_f64_dev(ddp_handle h, int n, int m, int N, int S, int B, int K, int iters, int pool, int traj0, const double *xs,
                        const double *us, double reg, int seed_lo, int seed_hi, const double *pi0, const double *mu0, const double *Sigma0,
                        double *pi, double *mu, double *Sigma, double *ll, int32_t *status);
int ddp_gmm_fit_f64(ddp_handle h, int n, int m, int N, int S, int B, int K, int iters, int pool, int traj0, const double *xs,
                    const double *us, double reg, int seed_lo, int seed_hi, const double *pi0, const double *mu0, const double *Sigma0,
                    double *pi, double *mu, double *Sigma, double *ll, int32_t *status);
int ddp_gmm_prior_f64_dev(ddp_handle h, int n, int m, int N, int S, int B, int K, int pool, const double *xs, const double *us,
                          const double *pi, const double *mu, const double *Sigma, double m0, double n0, double *Phi, double *mu0,
                          int32_t *status);
int ddp_gmm_prior_f64(ddp_handle h, int n, int m, int N, int S, int B, int K, int pool, const double *xs, const double *us,
                      const double *pi, const double *mu, const double *Sigma, double m0, double n0, double *Phi, double *mu0,
                      int32_t *status);

/* The moments and the expected cost of a linear-Gaussian policy under a fitted linear-Gaussian model and a fitted quadratic cost, the
 * step that closes the guided-policy-search round (sample -> fit -> iLQGkl -> expected cost -> ddp_kl_step_adjust_*).  The policy is
 * the one ddp_user_sample_* runs, u^_i = u_i + K_i (x^_i - x_i) + L_i xi with L_i L_i' = Sigma_i; the dynamics
 * x^_{i+1} = fx_i x^_i + fu_i u^_i + fc_i + w_i, w_i ~ N(0, cov_i), are the first four results of ddp_fit_dynamics_*; the cost of step i
 * is the quadratic model (cx, cu, cxx, cxu, cuu, c0) of ddp_user_cost_fit_* around (x_i, u_i).  With p = n + m, G_i = [fx_i fu_i],
 * H_i = [cxx_i cxu_i; cxu_i' cuu_i]:
 *   mux_0 = x0 (NULL: x[:,0]),  Sx_0 = Sigma0 (NULL: 0)
 *   dx_i = mux_i - x_i,   du_i = K_i dx_i,   dz_i = [dx_i; du_i]            (plain subtraction; lims play no part)
 *   Sz_i = [Sx_i, Sx_i K_i'; K_i Sx_i, K_i Sx_i K_i' + Sigma_i]
 *   ec_i = c0_i + cx_i.dx_i + cu_i.du_i + dz_i' H_i dz_i / 2 + tr(H_i Sz_i) / 2                       i = 0 .. N - 1
 *   mux_{i+1} = fx_i mux_i + fu_i (u_i + du_i) + fc_i,   Sx_{i+1} = G_i Sz_i G_i' + cov_i             i = 0 .. N - 2
 * inputs : K[m,n,N,B], Sigma[m,m,N,B] (NULL: a deterministic policy), x0[n,B] or NULL, x[n,N,B], u[m,N,B];
 *          fx[n,n,N(,B)], fu[n,m,N(,B)], fc[n,N(,B)], cov[n,n,N(,B)] (NULL: zeros) with the batch axis iff model_batched = 1 (slot N - 1
 *          is not read by the kernel); cx[n,N(,B)], cu[m,N(,B)], cxx[n,n,N(,B)], cxu[n,m,N(,B)], cuu[m,m,N(,B)], c0[N(,B)] with the batch
 *          axis iff cost_batched = 1; Sigma0[n,n,B] or NULL.
 * outputs: ec[N,B], status[B], and (each may be NULL) mu[p,N,B] = [mux_i; u_i + du_i], sigma[p,p,N,B] = Sz_i in the layout of
 *          ddp_forward_covariance_*'s sigmanew, filled at every step including N - 1.
 * cxx, cuu, cov, Sigma and Sigma0 are taken as symmetric (their upper triangles are what Sigma, Sigma0 and cov contribute); the
 * result on input that is not symmetric is undefined.  Sx and Sz are computed on their upper blocks and mirrored: sigma is symmetric to
 * the bit.  status[b] is 0, or i + 1 for the first step whose ec is not finite; from that step on the trajectory's ec, mu and sigma
 * are NaN — also when the value that was not finite (a c0_i, say) does not enter the chain of moments — and no other trajectory is
 * touched.  1 <= n <= 32, 1 <= m <= 8, N >= 1, B >= 1; anything else — a null required pointer, a *_batched flag other than 0 or 1,
 * for the host flavour a Sigma0 that is not finite (the _dev flavour cannot see it: it ends in status 1) — is refused by name before any
 * launch and before the handle is looked at.  Every sum has a fixed order that does not depend on B: two calls give the same bits, a
 * call on a slice of the trajectories gives the bits of that slice, and the host flavour (which stages its arrays like every
 * host-pointer entry) gives the bits of the _dev one.  Kernel ddp_expected_cost (expect.hip): one work-group of four waves per
 * trajectory, the matrix products on v_mfma_f64_16x16x4, the operands of step i + 1 fetched while step i computes.                 */
int ddp_expected_cost_f64_dev(ddp_handle h, int n, int m, int N, int B, const double *K, const double *Sigma, const double *x0,
                              const double *x, const double *u, const double *fx, const double *fu, const double *fc, const double *cov,
                              int model_batched, const double *cx, const double *cu, const double *cxx, const double *cxu,
                              const double *cuu, const double *c0, int cost_batched, const double *Sigma0, double *ec, int32_t *status,
                              double *mu, double *sigma);
int ddp_expected_cost_f64(ddp_handle h, int n, int m, int N, int B, const double *K, const double *Sigma, const double *x0,
                          const double *x, const double *u, const double *fx, const double *fu, const double *fc, const double *cov,
                          int model_batched, const double *cx, const double *cu, const double *cxx, const double *cxu,
                          const double *cuu, const double *c0, int cost_batched, const double *Sigma0, double *ec, int32_t *status,
                          double *mu, double *sigma);

#ifdef __cplusplus
}
#endif
#endif
