// user_problem.hip — user-defined problems: the user's f / costfun / df as HIP device source, compiled at run time for gfx950.
//
// The reference's iLQG(f, costfun, df, x0, u0; ...) takes the user's own closures.  Here the user writes four device functions
// (include/ddp_amd.h lists the contract); the library wraps them in its kernel templates (user_problem_kernels.h), compiles the
// program with hiprtc once per (source, n, m, nparam, flags, diff_wrap) and handle, and loads it on the handle's device.  The
// device-resident iLQG of ilqg.hip runs such a problem through its ddp_family interface (behind Model, ilqg_model.h), so the whole
// loop — statuses, trace keys, timing, pre-rolled starts, compaction, the slot scheduler — is the one the registered kinds run.
// hiprtc is loaded at first use (dlopen), like RCCL in comm.hip: the library has no link-time dependency on it.
#include <dlfcn.h>
#include <string.h>
#include <map>
#include <mutex>
#include <string>
#include <vector>
#include "ddp_internal.h"
#include "staging.h"
#include "user_autodiff.h"
#include "user_constraints.h"
#include "user_problem_kernels.h"
#include "user_problem_wave_kernels.h"
#include "user_sample_kernels.h"
#include "user_fitted_kernels.h"
#include "user_cost_fit_kernels.h"
#include "boxqp_dev_text.h"      // kBoxqpDevText: the text of boxqp_dev.h (written by build.py)
#include "back_pass_wide_kernel.h"   // BPWArgs, WLds, bpw_fill: the wide kernel's step, shared with ddp_user_back_pass2_wave
#include "philox_text.h"         // kPhiloxText: the text of philox.h (written by build.py)
#include "wide_kernel_text.h"    // kWideTileText, kWideKernelText: the texts of wide_tile.h and back_pass_wide_kernel.h (written by build.py)

DDP_USER_ABI
DDP_USER_ABI2
DDP_USER_ABI3
DDP_USER_ABI_C
DDP_USER_ABI_SAMPLE
DDP_USER_ABI_FIT
DDP_USER_ABI_COST_FIT

namespace {

typedef void *rtc_program;
struct Hiprtc {
    void *lib = nullptr;
    int (*CreateProgram)(rtc_program *, const char *, const char *, int, const char *const *, const char *const *) = nullptr;
    int (*CompileProgram)(rtc_program, int, const char *const *) = nullptr;
    int (*GetProgramLogSize)(rtc_program, size_t *) = nullptr;
    int (*GetProgramLog)(rtc_program, char *) = nullptr;
    int (*GetCodeSize)(rtc_program, size_t *) = nullptr;
    int (*GetCode)(rtc_program, char *) = nullptr;
    int (*DestroyProgram)(rtc_program *) = nullptr;
    const char *(*GetErrorString)(int) = nullptr;
};

Hiprtc *hiprtc()
{
    static Hiprtc r;
    static std::once_flag once;
    std::call_once(once, [] {
        const char *names[] = {"libhiprtc.so", "libhiprtc.so.7", "libhiprtc.so.6", "/opt/rocm/lib/libhiprtc.so"};
        for (const char *name : names) {
            r.lib = dlopen(name, RTLD_NOW | RTLD_LOCAL);
            if (r.lib) break;
        }
        if (!r.lib) return;
        r.CreateProgram = (decltype(r.CreateProgram))dlsym(r.lib, "hiprtcCreateProgram");
        r.CompileProgram = (decltype(r.CompileProgram))dlsym(r.lib, "hiprtcCompileProgram");
        r.GetProgramLogSize = (decltype(r.GetProgramLogSize))dlsym(r.lib, "hiprtcGetProgramLogSize");
        r.GetProgramLog = (decltype(r.GetProgramLog))dlsym(r.lib, "hiprtcGetProgramLog");
        r.GetCodeSize = (decltype(r.GetCodeSize))dlsym(r.lib, "hiprtcGetCodeSize");
        r.GetCode = (decltype(r.GetCode))dlsym(r.lib, "hiprtcGetCode");
        r.DestroyProgram = (decltype(r.DestroyProgram))dlsym(r.lib, "hiprtcDestroyProgram");
        r.GetErrorString = (decltype(r.GetErrorString))dlsym(r.lib, "hiprtcGetErrorString");
    });
    return (r.lib && r.CreateProgram && r.CompileProgram && r.GetProgramLogSize && r.GetProgramLog && r.GetCodeSize && r.GetCode &&
            r.DestroyProgram) ? &r : nullptr;
}

std::mutex g_log_mu;
std::string g_log;                                          // log of the last compile (ddp_user_compile_log)

// LDS budgets of the generated kernels (per 64-lane work-group): the rollout keeps several waves per CU (its time loop is a
// dependency chain, latency is hidden by more rollouts in flight), the derivative kernel is a stream of stores
constexpr int ROLL_LDS = 32 * 1024, DF_LDS = 64 * 1024, MAX_LDS = 64 * 1024, FIT_LDS = 48 * 1024, COST_FIT_LDS = 48 * 1024;

struct Layout { int chunk, rlanes, dflanes, adj, adh, wg, schunk, slanes, fchunk, flanes, clanes, cchunk, csb; };

// bytes of LDS of ddp_user_rollout_fit with `lanes` rollouts per work-group and `chunk` steps per chunk: u, x, k, K and the tables fx, fu,
// fc per rollout at odd strides, and the two slot arrays
size_t fit_lds(int n, int m, int lanes, int chunk)
{
    const int ps = 2 * m + m * n + n, ts = n * n + n * m + n;
    return (size_t)lanes * (((chunk * ps) | 1) + ((chunk * ts) | 1) + 1) * 8;
}

// bytes of LDS of ddp_user_cost_fit with `lanes` (step, trajectory) pairs per work-group and `csb` sample indices per round: per lane the
// derivatives and the sums (cx, cu, cxx, cxu, cuu each), c0, the nominal and csb samples at an odd stride, and the slot array
size_t cost_fit_lds(int n, int m, int lanes, int csb)
{
    const int dc = n + m + n * n + n * m + m * m;
    return (size_t)lanes * (((2 * dc + 1 + (csb + 1) * (n + m)) | 1) + 1) * 8;
}

// chunk length and rollouts per work-group of ddp_user_rollout, (step, trajectory) pairs per work-group of ddp_user_df; 0 lanes = no fit.
// DDP_USER_WAVE: rlanes and dflanes are the same two counts of the wave kernels (the launch geometry reads nothing else), wg the group.
// DDP_USER_AUTODIFF: seeds per call of `dynamics` (adj) and per Hessian block (adh) of ddp_user_df_ad, chosen by the kernel's VGPR and
// scratch counts (-Rpass-analysis=kernel-resource-usage)
Layout layout_of(int n, int m, int flags)
{
    Layout L;
    // nz <= 6 (car, pendcart): one call of `dynamics`, two Hessian blocks (3 block pairs).  lq 10x2 spills with 3-wide blocks or
    // 6-wide Jacobian chunks next to its 2-wide blocks; beyond nz = 12 the kernel spills anyway and 8-wide blocks halve the compile time
    const int nz = n + m;
    L.adj = nz <= 8 ? nz : 4;
    L.adh = nz <= 6 ? (nz + 1) / 2 : (nz <= 12 ? 2 : 8);
    const int ps = 2 * m + m * n + n;                            // DDP_PS
    L.rlanes = 64;
    L.chunk = (ROLL_LDS / 8 / 64 - 1) / ps;
    if (L.chunk > 16) L.chunk = 16;
    if (L.chunk < 1) {                                           // large n·m: one step per chunk, fewer rollouts per work-group
        L.chunk = 1;
        while (L.rlanes > 1 && (size_t)L.rlanes * (ps | 1) * 8 > (size_t)MAX_LDS) L.rlanes /= 2;
    }
    const int dt = n * n + n * m + n + m + ((flags & DDP_USER_CONST_HESSIAN) ? 0 : n * n + n * m + m * m);
    L.dflanes = 64;
    while (L.dflanes > 1 && (size_t)L.dflanes * (dt | 1) * 8 > (size_t)DF_LDS) L.dflanes /= 2;
    // ddp_user_sample (DDP_USER_SAMPLE): 64 samples of one trajectory per work-group; per step the shared operands u, x, K, L once and
    // x̂, û, c per sample.  The chunk that fits the rollout's budget, one step at least (n = 32, m = 8: 24 KB a step)
    L.slanes = 64;
    L.schunk = (ROLL_LDS / 8 - L.slanes) / (L.slanes * (n + m + 1) + m + n + m * n + m * m);
    if (L.schunk > 16) L.schunk = 16;
    if (L.schunk < 1) L.schunk = 1;
    // ddp_user_rollout_fit (DDP_USER_FITTED): the time loop is a chain of chunks, each a round trip to memory, so the chunk counts more
    // than the lanes: 64 rollouts per work-group where four steps of operands and tables fit FIT_LDS, else 32, else 16 with the chunk that
    // fits; a shape whose single step does not fit at 16 (n = 32, m = 8: 12.9 KB a rollout) takes one step and the rollouts that fit 64 KB
    L.flanes = 64;
    auto fit_chunk = [&](int lanes) { int c = 0; while (c < 8 && fit_lds(n, m, lanes, c + 1) <= (size_t)FIT_LDS) ++c; return c; };
    L.fchunk = fit_chunk(L.flanes);
    while (L.fchunk < 4 && L.flanes > 16) { L.flanes /= 2; L.fchunk = fit_chunk(L.flanes); }
    if (L.fchunk < 1) {
        L.fchunk = 1;
        while (L.flanes > 1 && fit_lds(n, m, L.flanes, 1) > (size_t)MAX_LDS) --L.flanes;
    }
    // ddp_user_cost_fit (DDP_USER_COST_FIT): one lane per (step, trajectory) with two slots of the cost derivatives in LDS, so the lanes
    // are what fits 64 KB (car 4x2: 64, lq 10x2: 16, lq 32x8: 2, as ddp_user_df); up to 8 consecutive steps of a trajectory per work-group
    // (the contiguous run of a sample), and the sample indices per round that keep the work-group within COST_FIT_LDS, one at least
    L.clanes = 64;
    while (L.clanes > 1 && cost_fit_lds(n, m, L.clanes, 1) > (size_t)MAX_LDS) L.clanes /= 2;
    L.cchunk = L.clanes < 8 ? L.clanes : 8;
    L.csb = 1;
    while (L.csb < 8 && cost_fit_lds(n, m, L.clanes, L.csb + 1) <= (size_t)COST_FIT_LDS) ++L.csb;
    L.wg = 0;
    if (flags & DDP_USER_WAVE) {
        // ddp_user_rollout_wave: a group of wg lanes (the power of two >= m, 8 at least) per rollout, 64 / wg rollouts per work-group;
        // ddp_user_df_wave: one (step, trajectory) per work-group; the hand-written ddp_user_df under the flag: 64 of them
        L.wg = m <= 8 ? 8 : (m <= 16 ? 16 : 32);
        L.chunk = 1;
        L.rlanes = 64 / L.wg;
        L.dflanes = (flags & DDP_USER_AUTODIFF) ? 1 : 64;
    }
    return L;
}

// `name` appears in `src` as a whole identifier (outside // and /* */ comments)
bool has_identifier(const std::string &src, const char *name)
{
    const size_t ln = strlen(name);
    auto ident = [](char c) { return c == '_' || (c >= '0' && c <= '9') || (c >= 'a' && c <= 'z') || (c >= 'A' && c <= 'Z'); };
    for (size_t i = 0; i < src.size();) {
        if (src.compare(i, 2, "//") == 0) { i = src.find('\n', i); if (i == std::string::npos) return false; continue; }
        if (src.compare(i, 2, "/*") == 0) { i = src.find("*/", i + 2); if (i == std::string::npos) return false; i += 2; continue; }
        if (src.compare(i, ln, name) == 0 && (i == 0 || !ident(src[i - 1])) && (i + ln >= src.size() || !ident(src[i + ln]))) return true;
        ++i;
    }
    return false;
}

// DDP_USER_CLOCK: the kernel text `text` with the absolute step handed to the user's functions (user_problem_kernels.h, at its end)
std::string with_clock(const char *text)
{
    struct Rule { const char *name; int arg; char kind; };      // kind: 'i' insert behind argument `arg`, 'w' wrap it, 'n' insert N - 1
    static const Rule rules[] = {{"dynamics", 3, 'i'}, {"stage_cost", 3, 'i'}, {"derivatives", 3, 'i'}, {"DDP_DERIVATIVES", 3, 'i'},
                                 {"ddp_ad_derivatives", 3, 'i'}, {"ddp_ad_jacobian", 3, 'i'}, {"ddp_ad_hessian", 3, 'i'},
                                 {"ddp_ad_hessian_block", 3, 'i'}, {"terminal_cost", 1, 'n'}, {"plant", 3, 'w'}};
    auto ident = [](char c) { return c == '_' || (c >= '0' && c <= '9') || (c >= 'a' && c <= 'z') || (c >= 'A' && c <= 'Z'); };
    const std::string src(text);
    std::string out;
    size_t i = 0;
    while (i < src.size()) {
        if (src.compare(i, 2, "//") == 0) {                      // comments pass through
            size_t e = src.find('\n', i);
            if (e == std::string::npos) e = src.size();
            out.append(src, i, e - i); i = e; continue;
        }
        if (src.compare(i, 2, "/*") == 0) {
            size_t e = src.find("*/", i + 2);
            e = e == std::string::npos ? src.size() : e + 2;
            out.append(src, i, e - i); i = e; continue;
        }
        if (!ident(src[i]) || (i > 0 && ident(src[i - 1]))) { out.push_back(src[i++]); continue; }
        size_t e = i;
        while (e < src.size() && ident(src[e])) ++e;
        const std::string word = src.substr(i, e - i);
        const Rule *r = nullptr;
        for (const Rule &c : rules)
            if (word == c.name) r = &c;
        size_t open = e;
        if (r && open < src.size() && src[open] == '<') {         // explicit template arguments: name<...>(
            const size_t gt = src.find('>', open);
            open = gt == std::string::npos ? src.size() : gt + 1;
        }
        if (!r || open >= src.size() || src[open] != '(') { out.append(word); i = e; continue; }
        // the arguments up to the one the rule names: [a0, a1) is argument r->arg (1-based), at parenthesis depth 0
        size_t a0 = open + 1, a1 = a0;
        int depth = 0, arg = 1;
        for (size_t k = open + 1; k < src.size(); ++k) {
            const char c = src[k];
            if (c == '(' || c == '[') ++depth;
            else if ((c == ')' || c == ']') && depth > 0) --depth;
            else if (c == ',' || c == ')') {
                if (arg == r->arg) { a1 = k; break; }
                if (c == ')') break;
                ++arg; a0 = k + 1;
            }
        }
        if (a1 <= a0) { out.append(word); i = e; continue; }      // fewer arguments than the rule needs: not a call of the model
        while (a0 < a1 && src[a0] == ' ') ++a0;
        const std::string a = src.substr(a0, a1 - a0);
        out.append(src, i, a0 - i);
        if (r->kind == 'w') out += "DDP_PLANT_T(" + a + ")";
        else if (r->kind == 'n') out += a + ", DDP_T(N - 1)";
        else if (a.compare(0, 4, "int ") == 0) out += a + ", int ddp_t";
        else out += a + ", DDP_T(" + a + ")";
        i = a1;
    }
    // the clock of the kernel's slot, read once: behind every line that takes the slot's parameters
    std::string res;
    for (size_t b = 0; b < out.size();) {
        size_t e = out.find('\n', b);
        e = e == std::string::npos ? out.size() : e + 1;
        res.append(out, b, e - b);
        const size_t at = out.find("= ddp_params(", b);
        if (at != std::string::npos && at < e) res += "    const int ddp_c = ddp_clock(a.clk, b);\n";
        b = e;
    }
    return res;
}

// nc < 0: an entry from before DDP_USER_CONSTRAINTS (ddp_user_check, ddp_user_create), which has no way to say how many there are
int validate(const char *source, int n, int m, int nparam, int flags, unsigned wrap, int nc = -1)
{
    DDP_CHECK(source, "user problem: null source");
    DDP_CHECK(nc >= 0 || !(flags & DDP_USER_CONSTRAINTS),
              "user problem: DDP_USER_CONSTRAINTS needs the number of constraints: ddp_user_check_c / ddp_user_create_c take it");
    const bool wave = (flags & DDP_USER_WAVE) != 0;
    if (wave) {
        DDP_CHECK(n >= 1 && n <= DDP_MAX_N_USER_WAVE, "user problem: n = %d out of [1, %d] (DDP_MAX_N_USER_WAVE)", n, DDP_MAX_N_USER_WAVE);
        DDP_CHECK(m >= 1 && m <= DDP_MAX_M_WIDE, "user problem: m = %d out of [1, %d] (DDP_MAX_M_WIDE)", m, DDP_MAX_M_WIDE);
    } else {
        DDP_CHECK(n >= 1 && n <= DDP_MAX_N_USER, "user problem: n = %d out of [1, %d] (DDP_MAX_N_USER; DDP_USER_WAVE takes n <= %d)", n,
                  DDP_MAX_N_USER, DDP_MAX_N_USER_WAVE);
        DDP_CHECK(m >= 1 && m <= DDP_MAX_M, "user problem: m = %d out of [1, %d] (DDP_MAX_M; DDP_USER_WAVE takes m <= %d)", m, DDP_MAX_M,
                  DDP_MAX_M_WIDE);
    }
    DDP_CHECK(nparam >= 0 && nparam <= DDP_USER_MAX_NPARAM, "user problem: nparam = %d out of [0, %d] (DDP_USER_MAX_NPARAM)", nparam,
              DDP_USER_MAX_NPARAM);
    DDP_CHECK((flags & ~(DDP_USER_TERMINAL | DDP_USER_CONST_HESSIAN | DDP_USER_AUTODIFF | DDP_USER_PLANT | DDP_USER_SECOND_ORDER |
                         DDP_USER_WAVE | DDP_USER_SECOND_ORDER_WAVE | DDP_USER_CLOCK | DDP_USER_CONSTRAINTS | DDP_USER_SAMPLE | DDP_USER_FITTED |
                         DDP_USER_COST_FIT)) == 0,
              "user problem: unknown flags 0x%x", flags);
    if (flags & DDP_USER_SAMPLE) {
        // deferred, not impossible: ddp_user_sample is a lane-per-sample kernel with the state in registers (n <= 32, m <= 8) and hands
        // the user's functions neither a clock nor multipliers
        DDP_CHECK(!(flags & DDP_USER_SECOND_ORDER_WAVE), "user problem: DDP_USER_SAMPLE | DDP_USER_SECOND_ORDER_WAVE is refused (deferred: "
                                                         "ddp_user_sample is sized for n <= %d, m <= %d)", DDP_MAX_N_USER, DDP_MAX_M);
        DDP_CHECK(!wave, "user problem: DDP_USER_SAMPLE | DDP_USER_WAVE is refused (deferred: ddp_user_sample is sized for n <= %d, m <= %d)",
                  DDP_MAX_N_USER, DDP_MAX_M);
        DDP_CHECK(!(flags & DDP_USER_CLOCK), "user problem: DDP_USER_SAMPLE | DDP_USER_CLOCK is refused (deferred: ddp_user_sample takes no clock)");
        DDP_CHECK(!(flags & DDP_USER_CONSTRAINTS), "user problem: DDP_USER_SAMPLE | DDP_USER_CONSTRAINTS is refused (deferred: ddp_user_sample "
                                                   "takes no multipliers)");
    }
    if (flags & DDP_USER_FITTED) {
        // deferred, not impossible: ddp_user_rollout_fit is a lane-per-rollout kernel with the state in registers (n <= 32, m <= 8) and hands
        // the user's cost neither a clock nor multipliers
        DDP_CHECK(!(flags & DDP_USER_SECOND_ORDER_WAVE), "user problem: DDP_USER_FITTED | DDP_USER_SECOND_ORDER_WAVE is refused (deferred: "
                                                         "ddp_user_rollout_fit is sized for n <= %d, m <= %d)", DDP_MAX_N_USER, DDP_MAX_M);
        DDP_CHECK(!wave, "user problem: DDP_USER_FITTED | DDP_USER_WAVE is refused (deferred: ddp_user_rollout_fit is sized for n <= %d, m <= %d)",
                  DDP_MAX_N_USER, DDP_MAX_M);
        DDP_CHECK(!(flags & DDP_USER_CLOCK), "user problem: DDP_USER_FITTED | DDP_USER_CLOCK is refused (deferred: ddp_user_rollout_fit takes no "
                                             "clock)");
        DDP_CHECK(!(flags & DDP_USER_CONSTRAINTS), "user problem: DDP_USER_FITTED | DDP_USER_CONSTRAINTS is refused (deferred: "
                                                   "ddp_user_rollout_fit takes no multipliers)");
    }
    if (flags & DDP_USER_COST_FIT) {
        // deferred, not impossible: ddp_user_cost_fit is a lane-per-(step, trajectory) kernel with the cost derivatives of a lane in LDS
        // (n <= 32, m <= 8) and hands the user's functions neither a clock nor multipliers
        DDP_CHECK(!(flags & DDP_USER_SECOND_ORDER_WAVE), "user problem: DDP_USER_COST_FIT | DDP_USER_SECOND_ORDER_WAVE is refused (deferred: "
                                                         "ddp_user_cost_fit is sized for n <= %d, m <= %d)", DDP_MAX_N_USER, DDP_MAX_M);
        DDP_CHECK(!wave, "user problem: DDP_USER_COST_FIT | DDP_USER_WAVE is refused (deferred: ddp_user_cost_fit is sized for n <= %d, m <= %d)",
                  DDP_MAX_N_USER, DDP_MAX_M);
        DDP_CHECK(!(flags & DDP_USER_CLOCK), "user problem: DDP_USER_COST_FIT | DDP_USER_CLOCK is refused (deferred: ddp_user_cost_fit takes no "
                                             "clock)");
        DDP_CHECK(!(flags & DDP_USER_CONSTRAINTS), "user problem: DDP_USER_COST_FIT | DDP_USER_CONSTRAINTS is refused (deferred: "
                                                   "ddp_user_cost_fit takes no multipliers)");
    }
    if (flags & DDP_USER_CONSTRAINTS) {
        // deferred, not impossible: the augmented cost is differentiated by AD, its Hessian is not constant, and the clocked and
        // second-order kernels would have to carry the multipliers as well
        DDP_CHECK(flags & DDP_USER_AUTODIFF, "user problem: DDP_USER_CONSTRAINTS needs DDP_USER_AUTODIFF (the augmented cost is differentiated by "
                                             "forward-mode AD of the templated model)");
        DDP_CHECK(!(flags & DDP_USER_CONST_HESSIAN), "user problem: DDP_USER_CONSTRAINTS | DDP_USER_CONST_HESSIAN is refused (the Hessian of the "
                                                     "penalty changes with the active set)");
        DDP_CHECK(!(flags & DDP_USER_CLOCK), "user problem: DDP_USER_CONSTRAINTS | DDP_USER_CLOCK is refused (deferred: constraints take no clock)");
        DDP_CHECK(!(flags & DDP_USER_SECOND_ORDER), "user problem: DDP_USER_CONSTRAINTS | DDP_USER_SECOND_ORDER is refused (deferred)");
        DDP_CHECK(!(flags & DDP_USER_SECOND_ORDER_WAVE), "user problem: DDP_USER_CONSTRAINTS | DDP_USER_SECOND_ORDER_WAVE is refused (deferred)");
        DDP_CHECK(nc >= 1 && nc <= DDP_USER_MAX_NC, "user problem: nc = %d out of [1, %d] (DDP_USER_MAX_NC)", nc, DDP_USER_MAX_NC);
        DDP_CHECK(nparam + 2 <= DDP_USER_MAX_NPARAM, "user problem: nparam = %d leaves no room for the two multiplier slots (DDP_USER_MAX_NPARAM "
                                                     "= %d)", nparam, DDP_USER_MAX_NPARAM);
    } else {
        DDP_CHECK(nc <= 0, "user problem: nc = %d but DDP_USER_CONSTRAINTS is not set (flag and nc must agree)", nc);
    }
    // deferred, not impossible: ddp_user_back_pass2 and ddp_user_back_pass2_wave evaluate the model inside the recursion (ddp_ad_vhess)
    DDP_CHECK(!((flags & DDP_USER_CLOCK) && (flags & DDP_USER_SECOND_ORDER)),
              "user problem: DDP_USER_CLOCK | DDP_USER_SECOND_ORDER is refused (ddp_user_back_pass2 runs the model on the horizon index)");
    DDP_CHECK(!((flags & DDP_USER_CLOCK) && (flags & DDP_USER_SECOND_ORDER_WAVE)),
              "user problem: DDP_USER_CLOCK | DDP_USER_SECOND_ORDER_WAVE is refused (ddp_user_back_pass2_wave runs the model on the horizon "
              "index)");
    if (flags & DDP_USER_SECOND_ORDER_WAVE) {
        DDP_CHECK(wave, "user problem: DDP_USER_SECOND_ORDER_WAVE needs DDP_USER_WAVE (ddp_user_back_pass2_wave is the wide kernel's step)");
        DDP_CHECK(flags & DDP_USER_AUTODIFF, "user problem: DDP_USER_SECOND_ORDER_WAVE needs DDP_USER_AUTODIFF (the curvature of the dynamics is "
                                             "derived from the templated model)");
        DDP_CHECK(!(flags & DDP_USER_SECOND_ORDER), "user problem: DDP_USER_SECOND_ORDER_WAVE excludes DDP_USER_SECOND_ORDER (one backward pass "
                                                    "per problem: ddp_user_back_pass2_wave or ddp_user_back_pass2)");
    }
    DDP_CHECK(!(wave && (flags & DDP_USER_SECOND_ORDER)),
              "user problem: DDP_USER_SECOND_ORDER | DDP_USER_WAVE is refused (ddp_user_back_pass2 is sized for n <= %d, m <= %d)",
              DDP_MAX_N_USER, DDP_MAX_M);
    DDP_CHECK(!(flags & DDP_USER_SECOND_ORDER) || (flags & DDP_USER_AUTODIFF),
              "user problem: DDP_USER_SECOND_ORDER needs DDP_USER_AUTODIFF (the curvature of the dynamics is derived from the templated model)");
    DDP_CHECK(n >= 32 || (wrap >> n) == 0, "user problem: diff_wrap = 0x%x names coordinates at or above n = %d", wrap, n);
    const std::string src(source);
    const char *need[] = {"dynamics", "stage_cost", "derivatives"};
    const int nneed = (flags & DDP_USER_AUTODIFF) ? 2 : 3;      // DDP_USER_AUTODIFF derives `derivatives`
    for (int k = 0; k < nneed; ++k)
        DDP_CHECK(has_identifier(src, need[k]), "user problem: the source defines no `%s` (the contract of ddp_amd.h)", need[k]);
    if (flags & DDP_USER_TERMINAL)
        DDP_CHECK(has_identifier(src, "terminal_cost"), "user problem: DDP_USER_TERMINAL is set but the source defines no `terminal_cost`");
    if (flags & DDP_USER_CONST_HESSIAN)
        DDP_CHECK(has_identifier(src, "cost_hessians"), "user problem: DDP_USER_CONST_HESSIAN is set but the source defines no `cost_hessians`");
    if (flags & DDP_USER_PLANT)
        DDP_CHECK(has_identifier(src, "plant"), "user problem: DDP_USER_PLANT is set but the source defines no `plant`");
    if (flags & DDP_USER_CONSTRAINTS)
        DDP_CHECK(has_identifier(src, "constraints"), "user problem: DDP_USER_CONSTRAINTS is set but the source defines no `constraints`");
    if (wave) return 0;                                          // (the wave kernels check their LDS with a static_assert: it fits at every shape)
    const Layout L = layout_of(n, m, flags);
    const int ps = 2 * m + m * n + n;
    DDP_CHECK((size_t)L.rlanes * ((L.chunk * ps) | 1) * 8 <= (size_t)MAX_LDS, "user problem: n = %d, m = %d does not fit the rollout's LDS", n, m);
    if (flags & DDP_USER_FITTED)
        DDP_CHECK(fit_lds(n, m, L.flanes, L.fchunk) <= (size_t)MAX_LDS, "user problem: n = %d, m = %d does not fit the LDS of ddp_user_rollout_fit", n, m);
    if (flags & DDP_USER_COST_FIT)
        DDP_CHECK(cost_fit_lds(n, m, L.clanes, L.csb) <= (size_t)MAX_LDS, "user problem: n = %d, m = %d does not fit the LDS of ddp_user_cost_fit", n, m);
    return 0;
}

std::string program_text(const char *source, int n, int m, int nparam, int flags, unsigned wrap, int nc = 0)
{
    const Layout L = layout_of(n, m, flags);
    char head[512];
    snprintf(head, sizeof head,
             "#define DDP_N %d\n#define DDP_M %d\n#define DDP_NP %d\n#define DDP_TERMINAL %d\n#define DDP_CONST_HESSIAN %d\n"
             "#define DDP_WRAP 0x%xu\n#define DDP_CHUNK %d\n#define DDP_RLANES %d\n#define DDP_DFLANES %d\n"
             "#define DDP_AUTODIFF %d\n#define DDP_ADJ %d\n#define DDP_ADH %d\n#define DDP_PLANT %d\n",
             n, m, (flags & DDP_USER_CONSTRAINTS) ? nparam + 2 : nparam,     // (the two multiplier slots of user_constraints.h)
             (flags & DDP_USER_TERMINAL) ? 1 : 0, (flags & DDP_USER_CONST_HESSIAN) ? 1 : 0, wrap, L.chunk, L.rlanes, L.dflanes,
             (flags & DDP_USER_AUTODIFF) ? 1 : 0, L.adj, L.adh, (flags & DDP_USER_PLANT) ? 1 : 0);
    std::string s(head);
    const bool ad = (flags & DDP_USER_AUTODIFF) != 0, wave = (flags & DDP_USER_WAVE) != 0, clock = (flags & DDP_USER_CLOCK) != 0;
    // DDP_USER_CLOCK: the same texts with the absolute step in every call of the user's functions (a problem without the flag: the texts)
    auto lib = [clock](const char *text) { return clock ? with_clock(text) : std::string(text); };
    if (clock) s += "#define DDP_CLOCK 1\n";
    if (wave) {                                                  // a problem without the flag: not a byte of its text changes
        snprintf(head, sizeof head, "#define DDP_WAVE 1\n#define DDP_WG %d\n", L.wg);
        s += head;
    }
    if (ad) {
        s += "#line 1 \"ddp_user_autodiff\"\n";
        s += kUserAutodiff;
    }
    const bool con = (flags & DDP_USER_CONSTRAINTS) != 0;        // a problem without the flag: not a byte of its text changes
    if (con) {
        snprintf(head, sizeof head, "#define DDP_NC %d\n", nc);
        s += head;
        s += kUserConstraintsBefore;
    }
    s += "#line 1 \"user_source\"\n";
    s += source;
    if (con) {
        s += "\n#line 1 \"ddp_user_constraints\"\n";
        s += kUserConstraintsAfter;
    }
    if (ad) {
        if (clock) s += kUserClockAd;
        s += "\n#line 1 \"ddp_user_autodiff_derivs\"\n";
        s += lib(kUserAutodiffDerivs);
    }
    s += "\n#line 1 \"ddp_user_kernels\"\n";
    s += clock ? DDP_USER_ABI_CLOCK_TEXT : DDP_USER_ABI_TEXT;
    s += "\n";
    if (clock) s += kUserClockKernels;
    s += kUserKernelsHead;
    if (wave) {
        s += "\n#line 1 \"ddp_user_wave_kernels\"\n";
        s += lib(kUserWaveKernels);
        s += "\n#line 1 \"ddp_user_kernels_shared\"\n";
        s += lib(kUserKernelsCost);
    } else {
        s += lib(kUserKernelsLane);
        s += lib(kUserKernelsCost);
        s += kUserKernelsHessians;
    }
    s += lib(kUserKernelsPlant);
    if (con) {
        s += "\n#line 1 \"ddp_user_constraints_kernels\"\n";
        s += DDP_USER_ABI_C_TEXT;
        s += "\n";
        s += kUserConstraintsKernels;
    }
    if (flags & DDP_USER_SECOND_ORDER) {                         // a problem without the flag: the text above, nothing more
        s += "\n#define DDP_SECOND_ORDER 1\n#line 1 \"ddp_user_autodiff_vhess\"\n";
        s += kUserAutodiffVhess;
        s += "\n#line 1 \"ddp_boxqp_dev\"\n";
        s += kUserRsqrt;
        s += kBoxqpDevText;
        s += "\n#line 1 \"ddp_user_kernels2\"\n";
        s += DDP_USER_ABI2_TEXT;
        s += "\n";
        s += kUserKernels2Head;
        s += kUserKernels2Bp2;
        s += kUserKernels2Vhess;
    }
    if (flags & DDP_USER_SECOND_ORDER_WAVE) {                    // the wave program above, then the wide kernel's step and its curvature phase
        s += "\n#define DDP_SECOND_ORDER 1\n#line 1 \"ddp_user_autodiff_vhess\"\n";
        s += kUserAutodiffVhess;
        s += "\n#line 1 \"ddp_boxqp_dev\"\n";
        s += kUserRsqrt;
        s += kBoxqpDevText;
        s += "\n#line 1 \"ddp_wide_tile\"\n";
        s += kUserWidePrelude;
        s += kWideTileText;
        s += "\n#line 1 \"ddp_back_pass_wide_kernel\"\n";
        s += kWideKernelText;
        s += "\n#line 1 \"ddp_user_kernels2\"\n";
        s += DDP_USER_ABI2_TEXT;
        s += "\n";
        s += DDP_USER_ABI3_TEXT;
        s += "\n";
        s += kUserKernels2Head;
        s += kUserKernels2Vhess;
        s += "\n#line 1 \"ddp_user_kernels2_wave\"\n";
        s += kUserKernels2Wave;
    }
    if (flags & DDP_USER_SAMPLE) {                               // a problem without the flag: the text above, nothing more
        snprintf(head, sizeof head, "\n#define DDP_SLANES %d\n#define DDP_SCHUNK %d\n#line 1 \"ddp_philox\"\n", L.slanes, L.schunk);
        s += head;
        s += kPhiloxText;
        s += "\n#line 1 \"ddp_user_kernels_sample\"\n";
        s += DDP_USER_ABI_SAMPLE_TEXT;
        s += "\n";
        s += kUserKernelsSample;
    }
    if (flags & DDP_USER_FITTED) {                               // a problem without the flag: the text above, nothing more; this tail goes last
        snprintf(head, sizeof head, "\n#define DDP_FLANES %d\n#define DDP_FCHUNK %d\n#line 1 \"ddp_user_kernels_fit\"\n", L.flanes, L.fchunk);
        s += head;
        s += DDP_USER_ABI_FIT_TEXT;
        s += "\n";
        s += kUserKernelsFit;
    }
    if (flags & DDP_USER_COST_FIT) {                             // a problem without the flag: the text above, nothing more; behind the fitted tail
        snprintf(head, sizeof head, "\n#define DDP_CLANES %d\n#define DDP_CCHUNK %d\n#define DDP_CSB %d\n#line 1 \"ddp_user_kernels_cost_fit\"\n",
                 L.clanes, L.cchunk, L.csb);
        s += head;
        s += DDP_USER_ABI_COST_FIT_TEXT;
        s += "\n";
        s += kUserKernelsCostFit;
    }
    return s;
}

// hiprtc: program text -> gfx950 code object; the log goes to g_log
int compile(const char *source, int n, int m, int nparam, int flags, unsigned wrap, const char *extra, std::vector<char> *code, int nc = -1)
{
    int rc = validate(source, n, m, nparam, flags, wrap, nc);
    if (rc) return rc;
    Hiprtc *R = hiprtc();
    DDP_CHECK(R, "user problem: hiprtc (libhiprtc.so) could not be loaded");
    const std::string text = program_text(source, n, m, nparam, flags, wrap, nc);
    std::vector<std::string> opts = {"--offload-arch=gfx950", "-O3", "-std=c++17"};
    if (extra) {
        const std::string e(extra);
        size_t i = 0;
        while (i < e.size()) {
            while (i < e.size() && e[i] == ' ') ++i;
            size_t j = i;
            while (j < e.size() && e[j] != ' ') ++j;
            if (j > i) opts.push_back(e.substr(i, j - i));
            i = j;
        }
    }
    std::vector<const char *> argv;
    for (auto &o : opts) argv.push_back(o.c_str());
    rtc_program prog = nullptr;
    int e = R->CreateProgram(&prog, text.c_str(), "ddp_user_problem.hip", 0, nullptr, nullptr);
    DDP_CHECK(e == 0, "user problem: hiprtcCreateProgram failed (%d)", e);
    e = R->CompileProgram(prog, (int)argv.size(), argv.data());
    size_t ls = 0;
    std::string log;
    if (R->GetProgramLogSize(prog, &ls) == 0 && ls > 1) {
        log.resize(ls);
        if (R->GetProgramLog(prog, &log[0]) != 0) log.clear();
        while (!log.empty() && log.back() == '\0') log.pop_back();
    }
    {
        std::lock_guard<std::mutex> g(g_log_mu);
        g_log = log;
    }
    if (e != 0) {
        R->DestroyProgram(&prog);
        // the first error line of the log names the cause (user_source:LINE:COL: error: ...)
        std::string first = log;
        const size_t at = log.find("error");
        if (at != std::string::npos) {
            const size_t b = log.rfind('\n', at), en = log.find('\n', at);
            first = log.substr(b == std::string::npos ? 0 : b + 1, en == std::string::npos ? std::string::npos : en - (b == std::string::npos ? 0 : b + 1));
        }
        ddp_set_error("user problem: compilation failed (%s): %s", R->GetErrorString ? R->GetErrorString(e) : "hiprtc error", first.c_str());
        return -4;
    }
    size_t cs = 0;
    if (R->GetCodeSize(prog, &cs) != 0 || cs == 0) { R->DestroyProgram(&prog); ddp_set_error("user problem: hiprtc returned no code"); return -4; }
    code->resize(cs);
    e = R->GetCode(prog, code->data());
    R->DestroyProgram(&prog);
    DDP_CHECK(e == 0, "user problem: hiprtcGetCode failed (%d)", e);
    return 0;
}

struct Module {
    hipModule_t mod = nullptr;
    hipFunction_t roll = nullptr, df = nullptr, cost = nullptr, hess = nullptr, plant = nullptr, bp2 = nullptr, vhess = nullptr;
    hipFunction_t bp2w = nullptr;                                // ddp_user_back_pass2_wave (DDP_USER_SECOND_ORDER_WAVE)
    hipFunction_t sample = nullptr;                              // ddp_user_sample (DDP_USER_SAMPLE)
    hipFunction_t rollfit = nullptr;                             // ddp_user_rollout_fit (DDP_USER_FITTED)
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
    mutable double *curv = nullptr;
    mutable size_t curv_bytes = 0;
    // DDP_USER_CLOCK: the clocks ddp_user_set_t0 gave (none: all 0, one: every trajectory's), and their device copy for the batch of
    // the last call (t0 of ddp_family points at it)
    std::vector<int32_t> t0_host;
    int32_t *t0_dev = nullptr;
    int t0_count = 0;                                            // entries of t0_dev that are valid (0: to be written)
    // DDP_USER_CONSTRAINTS: nc, the multipliers ddp_user_set_multipliers gave (device copies the problem owns; none: μ = 0), the ones an
    // augmented-Lagrangian loop works on for the time of its call (al_lam, al_mu: the caller's arrays), and the parameter block of the
    // last call.  The block is written again by every bind(), from pointers that are valid then: none outlives its array.
    int nc = 0;
    double *lam_dev = nullptr, *mu_dev = nullptr;
    int lam_N = 0, lam_B = 0;
    const double *al_lam = nullptr, *al_mu = nullptr;
    double *blk = nullptr;
    size_t blk_bytes = 0;
    // ddp_user_ilqg_al_*: the arrays later rounds are solved into, the live flags and the counter; grown on demand, kept between calls
    char *al_ws = nullptr;
    size_t al_ws_bytes = 0;
    // ddp_user_sample_*: the noise factors L[m,m,N,B] of the last call; grown on demand, kept between calls
    double *chol = nullptr;
    size_t chol_bytes = 0;
    ~UserProblem() override
    {
        if (curv) hipFree(curv);
        if (t0_dev) hipFree(t0_dev);
        if (lam_dev) hipFree(lam_dev);
        if (mu_dev) hipFree(mu_dev);
        if (blk) hipFree(blk);
        if (al_ws) hipFree(al_ws);
        if (chol) hipFree(chol);
    }

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
            DDP_CHECK(mod->rollfit, "forward_pass: the problem was made without DDP_USER_FITTED");
            UserRollFitArgs a;
            a.N = N; a.B = Bc; a.nalpha = nalpha; a.has_policy = K != nullptr; a.has_lims = lims != nullptr; a.params_batched = params_batched;
            a.params = params; a.K = K; a.k = k; a.x0 = x0; a.u = u; a.x = x; a.lims = lims; a.active = active; a.map = map;
            a.xnew = xnew; a.unew = unew; a.cnew = cnew; a.csum = csum; a.fx = fit_fx; a.fu = fit_fu; a.fc = fit_fc;
            for (int i = 0; i < 16; ++i) a.alpha[i] = i < nalpha ? alpha[i] : 0.0;
            void *args[] = {&a};
            const long total = (long)Bc * nalpha;
            DDP_HIP(hipModuleLaunchKernel(mod->rollfit, (unsigned)((total + mod->L.flanes - 1) / mod->L.flanes), 1, 1, 64, 1, 1, 0, hh->stream,
                                          args, nullptr));
            hh->last_kernel[1] = "ddp_user_rollout_fit";
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
            const size_t need = (size_t)(n + m) * (n + m) * sizeof(double) * (size_t)d.B;
            if (need > curv_bytes) {
                if (curv) { DDP_HIP(hipStreamSynchronize(hh->stream)); DDP_HIP(hipFree(curv)); curv = nullptr; curv_bytes = 0; }
                DDP_HIP(hipMalloc((void **)&curv, need));
                curv_bytes = need;
            }
            UserBp2WaveArgs w;
            bpw_fill(w.w, c);
            w.params = params; w.x = c.x; w.H = curv; w.map = c.map; w.params_batched = params_batched; w.pad_ = 0;
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

// sizes and parameters of one call
int bind(UserProblem *P, int N, int B, const double *params, int params_batched, bool params_on_device = false)
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
        DDP_CHECK(loop || !P->lam_dev || (P->lam_N == N && P->lam_B == B),
                  "user problem: ddp_user_set_multipliers gave lambda[%d, N = %d, B = %d], the call has N = %d, B = %d", P->nc, P->lam_N,
                  P->lam_B, N, B);
        if (!params_on_device) return 0;                         // (a host-pointer flavour: its `_dev` twin binds the device copy)
        const size_t need = (size_t)(P->nparam + 2) * B * sizeof(double);
        if (need > P->blk_bytes) {
            if (P->blk) { DDP_HIP(hipStreamSynchronize(P->h->stream)); DDP_HIP(hipFree(P->blk)); P->blk = nullptr; P->blk_bytes = 0; }
            DDP_HIP(hipMalloc((void **)&P->blk, need));
            P->blk_bytes = need;
        }
        const double *lam = loop ? P->al_lam : P->lam_dev, *mu = loop ? P->al_mu : P->mu_dev;
        hipLaunchKernelGGL(al_block_kernel, dim3((unsigned)((B + 255) / 256)), dim3(256), 0, P->h->stream, B, P->nparam, params_batched,
                           P->params, mu, lam, (size_t)P->nc * N, P->blk);
        DDP_HIP(hipGetLastError());
        P->params = P->blk; P->params_batched = 1;
    }
    if (!(P->flags & DDP_USER_CLOCK)) return 0;
    // DDP_USER_CLOCK: one clock per trajectory (problem) of this call on the device, written when the batch or the clocks have changed
    const int count = (int)P->t0_host.size();
    DDP_CHECK(count <= 1 || count == B, "user problem: ddp_user_set_t0 gave %d clocks, the call has %d trajectories (1 or %d are taken)",
              count, B, B);
    if (P->t0_count != B) {
        if (P->t0_dev) { DDP_HIP(hipStreamSynchronize(P->h->stream)); DDP_HIP(hipFree(P->t0_dev)); P->t0_dev = nullptr; }
        P->t0_count = 0;
        DDP_HIP(hipMalloc((void **)&P->t0_dev, (size_t)B * sizeof(int32_t)));
        std::vector<int32_t> t(B, count == 1 ? P->t0_host[0] : 0);
        if (count == B) t = P->t0_host;
        DDP_HIP(hipMemcpy(P->t0_dev, t.data(), (size_t)B * sizeof(int32_t), hipMemcpyHostToDevice));
        P->t0_count = B;
    }
    P->t0 = P->clk = P->t0_dev;
    return 0;
}

// what every ddp_user_* entry does first: the handle's device made current, the problem checked against the handle, the sizes and
// parameters of the call bound.  A host-pointer flavour binds twice, here (it needs CL to size its staging) and in its `_dev` twin, with
// the device copy of the parameters; the second bind finds t0_count == B and leaves the clocks on the device alone.
// DDP_USER_CONSTRAINTS: `dev` says that params is a device pointer (the `_dev` entries that take such a problem: the parameter block is
// assembled from it); `deferred` names an entry that refuses such a problem.
int enter(ddp_handle h, void *up, int N, int B, const double *params, int params_batched, UserProblem **P, bool dev = false,
          const char *deferred = nullptr)
{
    DDP_DEVICE(h);
    *P = as_problem(h, up);
    if (!*P) return -1;
    DDP_CHECK(!deferred || !((*P)->flags & DDP_USER_CONSTRAINTS), "%s: a DDP_USER_CONSTRAINTS problem is refused (deferred: constraints run "
                                                                  "through ddp_user_ilqg_* and ddp_user_ilqg_al_* only)", deferred);
    return bind(*P, N, B, params, params_batched, dev);
}

}   // namespace

extern "C" {

int ddp_user_check(const char *source, int n, int m, int nparam, int flags, const char *extra_options)
{
    std::vector<char> code;
    return compile(source, n, m, nparam, flags, 0u, extra_options, &code);
}

int ddp_user_check_c(const char *source, int n, int m, int nparam, int nc, int flags, const char *extra_options)
{
    DDP_CHECK(nc >= 0, "user problem: nc = %d (>= 0)", nc);
    std::vector<char> code;
    return compile(source, n, m, nparam, flags, 0u, extra_options, &code, nc);
}

const char *ddp_user_compile_log(void)
{
    static thread_local std::string copy;
    std::lock_guard<std::mutex> g(g_log_mu);
    copy = g_log;
    return copy.c_str();
}

static int user_create(ddp_handle h, const char *source, int n, int m, int nparam, int nc, int flags, int diff_wrap, void **out)
{
    DDP_DEVICE(h);
    DDP_CHECK(out, "user problem: null output");
    *out = nullptr;
    const unsigned wrap = (unsigned)diff_wrap;
    int rc = validate(source, n, m, nparam, flags, wrap, nc);
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
        rc = compile(source, n, m, nparam, flags, wrap, nullptr, &code, nc);
        if (rc) return rc;
        Module M;
        M.L = layout_of(n, m, flags);
        const bool wave = (flags & DDP_USER_WAVE) != 0;
        M.df_name = (flags & DDP_USER_AUTODIFF) ? (wave ? "ddp_user_df_wave" : "ddp_user_df_ad") : "ddp_user_df";
        M.roll_name = wave ? "ddp_user_rollout_wave" : "ddp_user_rollout";
        DDP_HIP(hipModuleLoadData(&M.mod, code.data()));
        const bool ok = hipModuleGetFunction(&M.roll, M.mod, M.roll_name) == hipSuccess &&
                        hipModuleGetFunction(&M.df, M.mod, M.df_name) == hipSuccess &&
                        hipModuleGetFunction(&M.cost, M.mod, "ddp_user_cost") == hipSuccess &&
                        (!(flags & DDP_USER_CONST_HESSIAN) || hipModuleGetFunction(&M.hess, M.mod, "ddp_user_hessians") == hipSuccess) &&
                        (!(flags & DDP_USER_PLANT) || hipModuleGetFunction(&M.plant, M.mod, "ddp_user_plant") == hipSuccess) &&
                        (!(flags & DDP_USER_SECOND_ORDER) || (hipModuleGetFunction(&M.bp2, M.mod, "ddp_user_back_pass2") == hipSuccess &&
                                                              hipModuleGetFunction(&M.vhess, M.mod, "ddp_user_vhess") == hipSuccess)) &&
                        (!(flags & DDP_USER_SECOND_ORDER_WAVE) ||
                         (hipModuleGetFunction(&M.bp2w, M.mod, "ddp_user_back_pass2_wave") == hipSuccess &&
                          hipModuleGetFunction(&M.vhess, M.mod, "ddp_user_vhess") == hipSuccess)) &&
                        (!(flags & DDP_USER_CONSTRAINTS) || (hipModuleGetFunction(&M.con, M.mod, "ddp_user_constraints") == hipSuccess &&
                                                             hipModuleGetFunction(&M.alup, M.mod, "ddp_user_al_update") == hipSuccess)) &&
                        (!(flags & DDP_USER_SAMPLE) || hipModuleGetFunction(&M.sample, M.mod, "ddp_user_sample") == hipSuccess) &&
                        (!(flags & DDP_USER_FITTED) || hipModuleGetFunction(&M.rollfit, M.mod, "ddp_user_rollout_fit") == hipSuccess) &&
                        (!(flags & DDP_USER_COST_FIT) || hipModuleGetFunction(&M.costfit, M.mod, "ddp_user_cost_fit") == hipSuccess);
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
    int rc = enter(h, up, N, B, params, params_batched, &P, true);
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
    const double *dp, *dx, *du;
    double *dfx, *dfu, *dcx, *dcu, *dxx, *dxu, *duu;
    Staging S(h, Staging::OWNED, "user problem");
    S.in(&dp, params, (size_t)P->nparam * (params_batched ? B : 1)); S.in(&dx, x, n * T); S.in(&du, u, m * T);
    S.out(&dfx, fx, n * n * T); S.out(&dfu, fu, n * m * T); S.out(&dcx, cx, n * T); S.out(&dcu, cu, m * T); S.out(&dxx, cxx, n * n * HT);
    S.out(&dxu, cxu, n * m * HT); S.out(&duu, cuu, m * m * HT);
    if ((rc = S.commit())) return rc;
    return S.finish(ddp_user_df_f64_dev(h, up, N, B, dp, params_batched, dx, du, nullptr, dfx, dfu, dcx, dcu, dxx, dxu, duu));
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
    a.N = N; a.B = B; a.params_batched = params_batched; a.pad_ = 0;
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
    const double *dp, *dx, *du, *dv;
    double *dH;
    Staging S(h, Staging::OWNED, "user problem");
    S.in(&dp, params, (size_t)P->nparam * (params_batched ? B : 1)); S.in(&dx, x, n * T); S.in(&du, u, m * T); S.in(&dv, v, n * T);
    S.out(&dH, H, (n + m) * (n + m) * T);
    if ((rc = S.commit())) return rc;
    return S.finish(ddp_user_vhess_f64_dev(h, up, N, B, dp, params_batched, dx, du, dv, nullptr, dH));
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
    const double *dp, *dx, *du, *dfx, *dfu, *dcx, *dcu, *dxx, *dxu, *duu, *dlam, *dl;
    double *dK, *dk, *dQ, *dVx, *dVxx, *ddV;
    int32_t *ddiv;
    Staging S(h, Staging::OWNED, "user problem");
    S.in(&dp, params, (size_t)P->nparam * (params_batched ? B : 1)); S.in(&dx, x, n * T); S.in(&du, u, m * T); S.in(&dfx, fx, n * n * T);
    S.in(&dfu, fu, n * m * T); S.in(&dcx, cx, n * T); S.in(&dcu, cu, m * T); S.in(&dxx, cxx, n * n * HT); S.in(&dxu, cxu, n * m * HT);
    S.in(&duu, cuu, m * m * HT); S.in(&dlam, lambda, (size_t)B); S.in(&dl, lims, 2 * m);
    S.out(&dK, K, m * n * T); S.out(&dk, k, m * T); S.out(&dQ, Quu, m * m * T); S.out(&dVx, Vx, n * T); S.out(&dVxx, Vxx, n * n * T);
    S.out(&ddV, dV, (size_t)2 * B); S.out(&ddiv, diverge, (size_t)B);
    if ((rc = S.commit())) return rc;
    return S.finish(ddp_user_back_pass_f64_dev(h, up, N, B, dp, params_batched, dx, du, dfx, dfu, dcx, dcu, dxx, dxu, duu, dlam, regType, dl,
                                               nullptr, dK, dk, dQ, dVx, dVxx, ddV, ddiv));
}

// Unlisted debug hook (not in ddp_amd.h): the program text hiprtc compiles for these arguments (tests: a problem without
// DDP_USER_SECOND_ORDER compiles the text it compiled before the flag existed).  NULL if the arguments are refused.
const char *ddp_user_program_text(const char *source, int n, int m, int nparam, int flags, int diff_wrap)
{
    static thread_local std::string text;
    if (validate(source, n, m, nparam, flags, (unsigned)diff_wrap)) return nullptr;
    text = program_text(source, n, m, nparam, flags, (unsigned)diff_wrap);
    return text.c_str();
}

// the same hook with the number of constraints (the program of a DDP_USER_CONSTRAINTS problem)
const char *ddp_user_program_text_c(const char *source, int n, int m, int nparam, int nc, int flags, int diff_wrap)
{
    static thread_local std::string text;
    if (nc < 0 || validate(source, n, m, nparam, flags, (unsigned)diff_wrap, nc)) return nullptr;
    text = program_text(source, n, m, nparam, flags, (unsigned)diff_wrap, nc);
    return text.c_str();
}

int ddp_user_set_multipliers(void *up, const double *lambda, const double *mu, int N, int B)
{
    UserProblem *P = (UserProblem *)up;
    DDP_CHECK(P, "user problem: null problem");
    DDP_CHECK(P->flags & DDP_USER_CONSTRAINTS, "set_multipliers: the problem was made without DDP_USER_CONSTRAINTS");
    DDP_HIP(hipSetDevice(P->h->device));
    if (P->lam_dev || P->mu_dev) {                               // (kernels in flight may still read them)
        DDP_HIP(hipStreamSynchronize(P->h->stream));
        if (P->lam_dev) DDP_HIP(hipFree(P->lam_dev));
        if (P->mu_dev) DDP_HIP(hipFree(P->mu_dev));
        P->lam_dev = P->mu_dev = nullptr; P->lam_N = P->lam_B = 0;
    }
    if (!lambda && !mu) return 0;
    DDP_CHECK(lambda && mu, "set_multipliers: lambda and mu must both be given or both NULL");
    DDP_CHECK(N >= 1 && B >= 1, "set_multipliers: N = %d, B = %d (both >= 1)", N, B);
    const size_t ln = (size_t)P->nc * N * B;
    DDP_HIP(hipMalloc((void **)&P->lam_dev, ln * sizeof(double)));
    DDP_HIP(hipMalloc((void **)&P->mu_dev, (size_t)B * sizeof(double)));
    DDP_HIP(hipMemcpy(P->lam_dev, lambda, ln * sizeof(double), hipMemcpyHostToDevice));
    DDP_HIP(hipMemcpy(P->mu_dev, mu, (size_t)B * sizeof(double), hipMemcpyHostToDevice));
    P->lam_N = N; P->lam_B = B;
    return 0;
}

int ddp_user_constraints_f64_dev(ddp_handle h, void *up, int N, int B, const double *params, int params_batched, const double *x,
                                 const double *u, double *g)
{
    UserProblem *P;
    int rc = enter(h, up, N, B, params, params_batched, &P, true);
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
    const double *dp, *dx, *du;
    double *dg;
    Staging S(h, Staging::OWNED, "user problem");
    S.in(&dp, params, (size_t)P->nparam * (params_batched ? B : 1)); S.in(&dx, x, n * T); S.in(&du, u, m * T);
    S.out(&dg, g, (size_t)P->nc * T);
    if ((rc = S.commit())) return rc;
    return S.finish(ddp_user_constraints_f64_dev(h, up, N, B, dp, params_batched, dx, du, dg));
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
    if (bytes > P->al_ws_bytes) {                                // (as curv and blk: no allocation per call once the batch has been seen)
        if (P->al_ws) { DDP_HIP(hipStreamSynchronize(st)); DDP_HIP(hipFree(P->al_ws)); P->al_ws = nullptr; P->al_ws_bytes = 0; }
        DDP_HIP(hipMalloc((void **)&P->al_ws, bytes));
        P->al_ws_bytes = bytes;
    }
    char *ws = P->al_ws;
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
        rc = bind(P, N, B, params, params_batched, true);        // the block of this round: μ and the pointers to λ as they stand now
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
    const size_t n = P->n, m = P->m, T = (size_t)N * B, CL = P->CL, nc = P->nc;
    const double *dp, *dx0, *du0, *dl, *dl0, *dm0;
    double *dx, *du, *dK, *dk, *dQ, *dVx, *dVxx, *dc, *ds, *dlam, *dmu, *dg, *das;
    Staging S(h, Staging::OWNED, "user problem");
    S.in(&dp, params, (size_t)P->nparam * (params_batched ? B : 1)); S.in(&dx0, x0, n * (x0_prerolled ? T : (size_t)B)); S.in(&du0, u0, m * T);
    S.in(&dl, lims, 2 * m); S.in(&dl0, lambda0, nc * T); S.in(&dm0, mu_init, (size_t)B);
    S.out(&dx, x, n * T); S.out(&du, u, m * T); S.out(&dK, K, m * n * T); S.out(&dk, k, m * T); S.out(&dQ, Quu, m * m * T); S.out(&dVx, Vx, n * T);
    S.out(&dVxx, Vxx, n * n * T); S.out(&dc, cost, CL * B); S.out(&ds, stats, (size_t)DDP_ILQG_NSTATS * B);
    S.out(&dlam, lambda, nc * T); S.out(&dmu, mu, (size_t)B); S.out(&dg, g, nc * T); S.out(&das, al_stats, (size_t)6 * B);
    if ((rc = S.commit())) return rc;
    return S.finish(ddp_user_ilqg_al_f64_dev(h, up, N, B, dp, params_batched, o, ao, dx0, x0_prerolled, du0, dl, dl0, dm0, dx, du, dK, dk, dQ,
                                             dVx, dVxx, dc, ds, dlam, dmu, dg, das, global_iters));
}

int ddp_user_forward_pass_f64_dev(ddp_handle h, void *up, int N, int B, const double *params, int params_batched,
                                  const double *K, const double *k, const double *x0, const double *u, const double *x,
                                  const double *alpha, int nalpha, const double *lims, const int32_t *active,
                                  double *xnew, double *unew, double *cnew, double *csum)
{
    UserProblem *P;
    int rc = enter(h, up, N, B, params, params_batched, &P, true);
    if (rc) return rc;
    DDP_CHECK(x0 && u && alpha && xnew && unew && cnew && csum, "forward_pass: null argument");
    return P->rollout(h, B, nullptr, K, k, x0, u, x, alpha, nalpha, lims, active, xnew, unew, cnew, csum);
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
    DDP_CHECK(nalpha >= 1 && nalpha <= 16, "forward_pass: nalpha=%d out of [1,16]", nalpha);
    const size_t n = P->n, m = P->m, T = (size_t)N * B, na = nalpha;
    const double *dp, *dK, *dk, *dx0, *du, *dx, *dl;
    double *dxn, *dun, *dcn, *dcs;
    Staging S(h, Staging::OWNED, "user problem");
    S.in(&dp, params, (size_t)P->nparam * (params_batched ? B : 1)); S.in(&dK, K, m * n * T); S.in(&dk, k, m * T); S.in(&dx0, x0, n * B);
    S.in(&du, u, m * T); S.in(&dx, x, n * T); S.in(&dl, lims, 2 * m);
    S.out(&dxn, xnew, n * T * na); S.out(&dun, unew, m * T * na); S.out(&dcn, cnew, (size_t)P->CL * B * na); S.out(&dcs, csum, (size_t)B * na);
    if ((rc = S.commit())) return rc;
    return S.finish(ddp_user_forward_pass_f64_dev(h, up, N, B, dp, params_batched, dK, dk, dx0, du, dx, alpha, nalpha, dl, nullptr, dxn, dun,
                                                  dcn, dcs));
}

int ddp_user_costfun_f64_dev(ddp_handle h, void *up, int N, int B, const double *params, int params_batched, const double *x,
                             const double *u, const int32_t *active, double *cost, double *csum)
{
    UserProblem *P;
    int rc = enter(h, up, N, B, params, params_batched, &P, true);
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
    const double *dp, *dx, *du;
    double *dc, *ds;
    Staging S(h, Staging::OWNED, "user problem");
    S.in(&dp, params, (size_t)P->nparam * (params_batched ? B : 1)); S.in(&dx, x, n * T); S.in(&du, u, m * T);
    S.out(&dc, cost, (size_t)P->CL * B); S.out(&ds, csum, (size_t)B);
    if ((rc = S.commit())) return rc;
    return S.finish(ddp_user_costfun_f64_dev(h, up, N, B, dp, params_batched, dx, du, nullptr, dc, ds));
}

int ddp_user_ilqg_f64_dev(ddp_handle h, void *up, int N, int B, const double *params, int params_batched, const ddp_ilqg_opts *o,
                          const double *x0, int x0_prerolled, const double *u0, const double *cost0, const double *lims,
                          double *x, double *u, double *K, double *k, double *Quu, double *Vx, double *Vxx,
                          double *cost, double *stats, int trace_cap, double *trace7, int *global_iters)
{
    UserProblem *P;
    int rc = enter(h, up, N, B, params, params_batched, &P, true);
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
    const double *dp, *dx0, *du0, *dc0 = nullptr, *dl;
    double *dx, *du, *dK, *dk, *dQ, *dVx, *dVxx, *dc, *ds, *dt7 = nullptr;
    Staging S(h, Staging::OWNED, "user problem");
    S.in(&dp, params, (size_t)P->nparam * (params_batched ? B : 1)); S.in(&dx0, x0, n * (x0_prerolled ? T : (size_t)B)); S.in(&du0, u0, m * T);
    if (x0_prerolled) S.in(&dc0, cost0, CL * B);
    S.in(&dl, lims, 2 * m);
    S.out(&dx, x, n * T); S.out(&du, u, m * T); S.out(&dK, K, m * n * T); S.out(&dk, k, m * T); S.out(&dQ, Quu, m * m * T); S.out(&dVx, Vx, n * T);
    S.out(&dVxx, Vxx, n * n * T); S.out(&dc, cost, CL * B); S.out(&ds, stats, (size_t)DDP_ILQG_NSTATS * B);
    if (trace7 && trace_cap > 0) S.out(&dt7, trace7, (size_t)7 * trace_cap * B);
    if ((rc = S.commit())) return rc;
    return S.finish(ddp_user_ilqg_f64_dev(h, up, N, B, dp, params_batched, o, dx0, x0_prerolled, du0, dc0, dl, dx, du, dK, dk, dQ, dVx, dVxx,
                                          dc, ds, trace_cap, dt7, global_iters));
}

int ddp_user_ilqg_queue_f64_dev(ddp_handle h, void *up, int N, int P, const double *params, int params_batched, const ddp_ilqg_opts *o,
                                int slots, const double *x0, const double *u0, const double *lims, double *x, double *u, double *K, double *k,
                                double *Quu, double *Vx, double *Vxx, double *cost, double *stats, int *global_iters)
{
    UserProblem *U;
    int rc = enter(h, up, N, P, params, params_batched, &U, false, "ilqg_queue");
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
    int rc = enter(h, up, N, P, params, params_batched, &U, false, "ilqg_queue");
    if (rc) return rc;
    DDP_CHECK(x0 && u0 && x && u && K && k && Quu && Vx && Vxx && cost && stats, "ilqg_queue: null argument");
    const size_t n = U->n, m = U->m, T = (size_t)N * P, CL = U->CL;
    const double *dp, *dx0, *du0, *dl;
    double *dx, *du, *dK, *dk, *dQ, *dVx, *dVxx, *dc, *ds;
    Staging S(h, Staging::OWNED, "user problem");
    S.in(&dp, params, (size_t)U->nparam * (params_batched ? P : 1)); S.in(&dx0, x0, n * P); S.in(&du0, u0, m * T); S.in(&dl, lims, 2 * m);
    S.out(&dx, x, n * T); S.out(&du, u, m * T); S.out(&dK, K, m * n * T); S.out(&dk, k, m * T); S.out(&dQ, Quu, m * m * T); S.out(&dVx, Vx, n * T);
    S.out(&dVxx, Vxx, n * n * T); S.out(&dc, cost, CL * P); S.out(&ds, stats, (size_t)DDP_ILQG_NSTATS * P);
    if ((rc = S.commit())) return rc;
    return S.finish(ddp_user_ilqg_queue_f64_dev(h, up, N, P, dp, params_batched, o, slots, dx0, du0, dl, dx, du, dK, dk, dQ, dVx, dVxx, dc, ds,
                                                global_iters));
}

int ddp_user_ilqg_mpc_f64_dev(ddp_handle h, void *up, int N, int B, const double *params, int params_batched, const ddp_ilqg_opts *o,
                              int steps, int zero_tail, const double *x0, const double *u0, const double *lims, double *xcl, double *ucl,
                              double *stats_cl, double *x, double *u, int *global_iters)
{
    UserProblem *U;
    int rc = enter(h, up, N, B, params, params_batched, &U, false, "ilqg_mpc");
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
    int rc = enter(h, up, N, B, params, params_batched, &U, false, "ilqg_mpc");
    if (rc) return rc;
    DDP_CHECK(steps >= 1, "ilqg_mpc: steps=%d", steps);
    DDP_CHECK(x0 && u0 && xcl && ucl && stats_cl && x && u, "ilqg_mpc: null argument");
    const size_t n = U->n, m = U->m, T = (size_t)N * B;
    const double *dp, *dx0, *du0, *dl;
    double *dxcl, *ducl, *dscl, *dx, *du;
    Staging S(h, Staging::OWNED, "user problem");
    S.in(&dp, params, (size_t)U->nparam * (params_batched ? B : 1)); S.in(&dx0, x0, n * B); S.in(&du0, u0, m * T); S.in(&dl, lims, 2 * m);
    S.out(&dxcl, xcl, n * (size_t)(steps + 1) * B); S.out(&ducl, ucl, m * (size_t)steps * B);
    S.out(&dscl, stats_cl, (size_t)DDP_ILQG_NSTATS * steps * B); S.out(&dx, x, n * T); S.out(&du, u, m * T);
    if ((rc = S.commit())) return rc;
    return S.finish(ddp_user_ilqg_mpc_f64_dev(h, up, N, B, dp, params_batched, o, steps, zero_tail, dx0, du0, dl, dxcl, ducl, dscl, dx, du,
                                              global_iters));
}

int ddp_user_ilqgkl_f64_dev(ddp_handle h, void *up, int N, int B, const double *params, int params_batched, const ddp_ilqgkl_opts *o,
                            const double *x0, const double *cost0, const double *Kp, const double *kp, const double *Sp, const double *Sip,
                            const double *model_fx, int model_fx_batched, const double *R1, const double *lims, double *etab,
                            double *x, double *u, double *K, double *Sigma, double *Sigmai, double *Vx, double *Vxx,
                            double *cost, double *dV, double *stats, int *iters)
{
    UserProblem *U;
    int rc = enter(h, up, N, B, params, params_batched, &U, false, "ilqgkl");
    if (rc) return rc;
    return ddp_ilqgkl_family_dev(h, U, o, x0, cost0, Kp, kp, Sp, Sip, model_fx, model_fx_batched, R1, lims, etab, x, u, K, Sigma, Sigmai, Vx,
                                 Vxx, cost, dV, stats, iters);
}

int ddp_user_ilqgkl_f64(ddp_handle h, void *up, int N, int B, const double *params, int params_batched, const ddp_ilqgkl_opts *o,
                        const double *x0, const double *cost0, const double *Kp, const double *kp, const double *Sp, const double *Sip,
                        const double *model_fx, int model_fx_batched, const double *R1, const double *lims, double *etab,
                        double *x, double *u, double *K, double *Sigma, double *Sigmai, double *Vx, double *Vxx,
                        double *cost, double *dV, double *stats, int *iters)
{
    UserProblem *U;
    int rc = enter(h, up, N, B, params, params_batched, &U, false, "ilqgkl");
    if (rc) return rc;
    DDP_CHECK(x0 && Kp && kp && Sp && Sip && R1 && x && u && K && Sigma && Sigmai && Vx && Vxx && cost && dV && stats, "ilqgkl: null argument");
    const size_t n = U->n, m = U->m, T = (size_t)N * B, CL = U->CL;
    const double *dp, *dx0, *dc0, *dKp, *dkp, *dSp, *dSip, *dmf, *dR1, *dl;
    double *det, *dx, *du, *dK, *dS, *dSi, *dVx, *dVxx, *dc, *ddV, *ds;
    Staging S(h, Staging::OWNED, "user problem");
    S.in(&dp, params, (size_t)U->nparam * (params_batched ? B : 1)); S.in(&dx0, x0, n * T); S.in(&dc0, cost0, (size_t)B); S.in(&dKp, Kp, m * n * T);
    S.in(&dkp, kp, m * T); S.in(&dSp, Sp, m * m * T); S.in(&dSip, Sip, m * m * T);
    S.in(&dmf, model_fx, n * n * (size_t)N * (model_fx_batched ? B : 1)); S.in(&dR1, R1, n * n); S.in(&dl, lims, 2 * m);
    S.inout(&det, etab, (size_t)3 * B); S.out(&dx, x, n * T); S.out(&du, u, m * T); S.out(&dK, K, m * n * T); S.out(&dS, Sigma, m * m * T);
    S.out(&dSi, Sigmai, m * m * T); S.out(&dVx, Vx, n * T); S.out(&dVxx, Vxx, n * n * T); S.out(&dc, cost, CL * B); S.out(&ddV, dV, (size_t)2 * B);
    S.out(&ds, stats, (size_t)DDP_ILQGKL_NSTATS * B);
    if ((rc = S.commit())) return rc;
    return S.finish(ddp_user_ilqgkl_f64_dev(h, up, N, B, dp, params_batched, o, dx0, dc0, dKp, dkp, dSp, dSip, dmf, model_fx_batched, dR1, dl,
                                            det, dx, du, dK, dS, dSi, dVx, dVxx, dc, ddV, ds, iters));
}

// what both flavours of ddp_user_sample refuse, before anything is staged or launched
static int sample_check(const UserProblem *P, int S, const double *K, const double *x0, const double *u, const double *x, int sample0,
                        int traj0, int use_plant, const double *xs, const double *cs, const double *csum, const double *xmean,
                        const double *xcov, const int32_t *status)
{
    DDP_CHECK(P->mod->sample, "sample: the problem was made without DDP_USER_SAMPLE");
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
    int rc = enter(h, up, N, B, params, params_batched, &P, true);
    if (rc) return rc;
    if ((rc = sample_check(P, S, K, x0, u, x, sample0, traj0, use_plant, xs, cs, csum, xmean, xcov, status))) return rc;
    const int m = P->m;
    const long groups = ((long)S + P->mod->L.slanes - 1) / P->mod->L.slanes;
    DDP_CHECK(groups * B <= 0x7fffffffL, "sample: S = %d, B = %d is too large for one launch", S, B);
    if (Sigma) {
        const size_t need = (size_t)m * m * N * B * sizeof(double);
        if (need > P->chol_bytes) {
            if (P->chol) { DDP_HIP(hipStreamSynchronize(h->stream)); DDP_HIP(hipFree(P->chol)); P->chol = nullptr; P->chol_bytes = 0; }
            DDP_HIP(hipMalloc((void **)&P->chol, need));
            P->chol_bytes = need;
        }
        if ((rc = ddp_policy_factor_dev(h, m, N, B, Sigma, P->chol, status))) return rc;
    } else {
        DDP_HIP(hipMemsetAsync(status, 0, (size_t)B * sizeof(int32_t), h->stream));
    }
    UserSampleArgs a;
    a.N = N; a.B = B; a.S = S; a.has_lims = lims != nullptr; a.params_batched = params_batched; a.use_plant = use_plant;
    a.sample0 = sample0; a.traj0 = traj0; a.seed_lo = seed_lo; a.seed_hi = seed_hi;
    a.params = P->params; a.K = K; a.L = Sigma ? P->chol : nullptr; a.x0 = x0; a.u = u; a.x = x; a.lims = lims;
    a.noise = Sigma ? noise : nullptr; a.status = status; a.xs = xs; a.us = us; a.cs = cs; a.csum = csum;
    void *args[] = {&a};
    DDP_HIP(hipModuleLaunchKernel(P->mod->sample, (unsigned)(groups * B), 1, 1, 64, 1, 1, 0, h->stream, args, nullptr));
    h->last_kernel[1] = "ddp_user_sample";
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
    const double *dp, *dK, *dSg, *dx0, *du, *dx, *dl, *dno;
    double *dxs, *dus, *dcs, *dcsum, *dmean, *dcov;
    int32_t *dst;
    Staging St(h, Staging::OWNED, "user problem");
    St.in(&dp, params, (size_t)P->nparam * (params_batched ? B : 1)); St.in(&dK, K, m * n * T); St.in(&dSg, Sigma, m * m * T);
    St.in(&dx0, x0, n * B); St.in(&du, u, m * T); St.in(&dx, x, n * T); St.in(&dl, lims, 2 * m);
    St.in(&dno, Sigma ? noise : nullptr, m * N * R);
    St.out(&dxs, xs, n * N * R); St.out(&dus, us, m * N * R); St.out(&dcs, cs, (size_t)P->CL * R); St.out(&dcsum, csum, R);
    St.out(&dmean, xmean, n * T); St.out(&dcov, xcov, n * n * T); St.out(&dst, status, (size_t)B);
    if ((rc = St.commit())) return rc;
    return St.finish(ddp_user_sample_f64_dev(h, up, N, B, S, dp, params_batched, dK, dSg, dx0, du, dx, dl, dno, seed_lo, seed_hi, sample0,
                                             traj0, use_plant, dxs, dus, dcs, dcsum, dmean, dcov, dst));
}

// ---- DDP_USER_FITTED: the rollout and the KL loop on the tables of ddp_fit_dynamics.  The tables ride on the family for the time of the
// call (FitScope): rollout() then launches ddp_user_rollout_fit.
int ddp_user_rollout_fit_f64_dev(ddp_handle h, void *up, int N, int B, const double *params, int params_batched,
                                 const double *K, const double *k, const double *x0, const double *u, const double *x,
                                 const double *alpha, int nalpha, const double *lims, const int32_t *active,
                                 const double *fx, const double *fu, const double *fc,
                                 double *xnew, double *unew, double *cnew, double *csum)
{
    UserProblem *P;
    int rc = enter(h, up, N, B, params, params_batched, &P, true);
    if (rc) return rc;
    DDP_CHECK(P->mod->rollfit, "rollout_fit: the problem was made without DDP_USER_FITTED");
    DDP_CHECK(x0 && u && alpha && fx && fu && fc && xnew && unew && cnew && csum, "rollout_fit: null argument");
    FitScope fit(P, fx, fu, fc);
    return P->rollout(h, B, nullptr, K, k, x0, u, x, alpha, nalpha, lims, active, xnew, unew, cnew, csum);
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
    DDP_CHECK(P->mod->rollfit, "rollout_fit: the problem was made without DDP_USER_FITTED");
    DDP_CHECK(x0 && u && alpha && fx && fu && fc && xnew && unew && cnew && csum, "rollout_fit: null argument");
    DDP_CHECK(nalpha >= 1 && nalpha <= 16, "forward_pass: nalpha=%d out of [1,16]", nalpha);
    const size_t n = P->n, m = P->m, T = (size_t)N * B, na = nalpha;
    const double *dp, *dK, *dk, *dx0, *du, *dx, *dl, *dfx, *dfu, *dfc;
    double *dxn, *dun, *dcn, *dcs;
    Staging S(h, Staging::OWNED, "user problem");
    S.in(&dp, params, (size_t)P->nparam * (params_batched ? B : 1)); S.in(&dK, K, m * n * T); S.in(&dk, k, m * T); S.in(&dx0, x0, n * B);
    S.in(&du, u, m * T); S.in(&dx, x, n * T); S.in(&dl, lims, 2 * m);
    S.in(&dfx, fx, n * n * T); S.in(&dfu, fu, n * m * T); S.in(&dfc, fc, n * T);
    S.out(&dxn, xnew, n * T * na); S.out(&dun, unew, m * T * na); S.out(&dcn, cnew, (size_t)P->CL * B * na); S.out(&dcs, csum, (size_t)B * na);
    if ((rc = S.commit())) return rc;
    return S.finish(ddp_user_rollout_fit_f64_dev(h, up, N, B, dp, params_batched, dK, dk, dx0, du, dx, alpha, nalpha, dl, nullptr, dfx, dfu,
                                                 dfc, dxn, dun, dcn, dcs));
}

int ddp_user_ilqgkl_fit_f64_dev(ddp_handle h, void *up, int N, int B, const double *params, int params_batched, const ddp_ilqgkl_opts *o,
                                const double *x0, const double *cost0, const double *Kp, const double *kp, const double *Sp,
                                const double *Sip, const double *model_fx, int model_fx_batched, const double *R1, const double *lims,
                                double *etab, const double *fx, const double *fu, const double *fc,
                                double *x, double *u, double *K, double *Sigma, double *Sigmai, double *Vx, double *Vxx,
                                double *cost, double *dV, double *stats, int *iters)
{
    UserProblem *U;
    int rc = enter(h, up, N, B, params, params_batched, &U, false, "ilqgkl");
    if (rc) return rc;
    DDP_CHECK(U->mod->rollfit, "ilqgkl_fit: the problem was made without DDP_USER_FITTED");
    DDP_CHECK(fx && fu && fc, "ilqgkl_fit: null argument");
    return ddp_ilqgkl_family_dev(h, U, o, x0, cost0, Kp, kp, Sp, Sip, model_fx, model_fx_batched, R1, lims, etab, x, u, K, Sigma, Sigmai, Vx,
                                 Vxx, cost, dV, stats, iters, fx, fu, fc);
}

int ddp_user_ilqgkl_fit_f64(ddp_handle h, void *up, int N, int B, const double *params, int params_batched, const ddp_ilqgkl_opts *o,
                            const double *x0, const double *cost0, const double *Kp, const double *kp, const double *Sp,
                            const double *Sip, const double *model_fx, int model_fx_batched, const double *R1, const double *lims,
                            double *etab, const double *fx, const double *fu, const double *fc,
                            double *x, double *u, double *K, double *Sigma, double *Sigmai, double *Vx, double *Vxx,
                            double *cost, double *dV, double *stats, int *iters)
{
    UserProblem *U;
    int rc = enter(h, up, N, B, params, params_batched, &U, false, "ilqgkl");
    if (rc) return rc;
    DDP_CHECK(U->mod->rollfit, "ilqgkl_fit: the problem was made without DDP_USER_FITTED");
    DDP_CHECK(x0 && Kp && kp && Sp && Sip && R1 && fx && fu && fc && x && u && K && Sigma && Sigmai && Vx && Vxx && cost && dV && stats,
              "ilqgkl_fit: null argument");
    const size_t n = U->n, m = U->m, T = (size_t)N * B, CL = U->CL;
    const double *dp, *dx0, *dc0, *dKp, *dkp, *dSp, *dSip, *dmf, *dR1, *dl, *dfx, *dfu, *dfc;
    double *det, *dx, *du, *dK, *dS, *dSi, *dVx, *dVxx, *dc, *ddV, *ds;
    Staging S(h, Staging::OWNED, "user problem");
    S.in(&dp, params, (size_t)U->nparam * (params_batched ? B : 1)); S.in(&dx0, x0, n * T); S.in(&dc0, cost0, (size_t)B); S.in(&dKp, Kp, m * n * T);
    S.in(&dkp, kp, m * T); S.in(&dSp, Sp, m * m * T); S.in(&dSip, Sip, m * m * T);
    S.in(&dmf, model_fx, n * n * (size_t)N * (model_fx_batched ? B : 1)); S.in(&dR1, R1, n * n); S.in(&dl, lims, 2 * m);
    S.in(&dfx, fx, n * n * T); S.in(&dfu, fu, n * m * T); S.in(&dfc, fc, n * T);
    S.inout(&det, etab, (size_t)3 * B); S.out(&dx, x, n * T); S.out(&du, u, m * T); S.out(&dK, K, m * n * T); S.out(&dS, Sigma, m * m * T);
    S.out(&dSi, Sigmai, m * m * T); S.out(&dVx, Vx, n * T); S.out(&dVxx, Vxx, n * n * T); S.out(&dc, cost, CL * B); S.out(&ddV, dV, (size_t)2 * B);
    S.out(&ds, stats, (size_t)DDP_ILQGKL_NSTATS * B);
    if ((rc = S.commit())) return rc;
    return S.finish(ddp_user_ilqgkl_fit_f64_dev(h, up, N, B, dp, params_batched, o, dx0, dc0, dKp, dkp, dSp, dSip, dmf, model_fx_batched, dR1, dl,
                                                det, dfx, dfu, dfc, dx, du, dK, dS, dSi, dVx, dVxx, dc, ddV, ds, iters));
}

// ---- DDP_USER_COST_FIT: the quadratic cost model fitted to sampled rollouts (ddp_user_cost_fit), and the KL loop on a cost model
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
    int rc = enter(h, up, N, B, params, params_batched, &P, true);
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
    const double *dp, *dxs, *dus, *dx, *du;
    double *dcx, *dcu, *dcxx, *dcxu, *dcuu, *dc0;
    Staging St(h, Staging::OWNED, "user problem");
    St.in(&dp, params, (size_t)P->nparam * (params_batched ? B : 1)); St.in(&dxs, xs, n * R); St.in(&dus, us, m * R);
    St.in(&dx, x, n * T); St.in(&du, u, m * T);
    St.out(&dcx, cx, n * T); St.out(&dcu, cu, m * T); St.out(&dcxx, cxx, n * n * T); St.out(&dcxu, cxu, n * m * T);
    St.out(&dcuu, cuu, m * m * T); St.out(&dc0, c0, T);
    if ((rc = St.commit())) return rc;
    return St.finish(ddp_user_cost_fit_f64_dev(h, up, N, S, B, dp, params_batched, dxs, dus, dx, du, dcx, dcu, dcxx, dcxu, dcuu, dc0));
}

// what both flavours of ddp_user_ilqgkl_cost refuse
static int ilqgkl_cost_check(const UserProblem *U, const double *fx, const double *fu, const double *fc, const double *cx, const double *cu,
                             const double *cxx, const double *cxu, const double *cuu)
{
    DDP_CHECK((fx && fu && fc) || (!fx && !fu && !fc), "ilqgkl_cost: fx, fu and fc are given all three (the plan is made on the tables) or all "
                                                       "three NULL (on the problem's own model)");
    DDP_CHECK(!fx || U->mod->rollfit, "ilqgkl_cost: the problem was made without DDP_USER_FITTED (the tables fx, fu, fc need it)");
    DDP_CHECK(cx && cu && cxx && cxu && cuu, "ilqgkl_cost: a cost model is cx, cu, cxx, cxu and cuu (null argument)");
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
    int rc = enter(h, up, N, B, params, params_batched, &U, false, "ilqgkl");
    if (rc) return rc;
    if ((rc = ilqgkl_cost_check(U, fx, fu, fc, cx, cu, cxx, cxu, cuu))) return rc;
    return ddp_ilqgkl_family_dev(h, U, o, x0, cost0, Kp, kp, Sp, Sip, model_fx, model_fx_batched, R1, lims, etab, x, u, K, Sigma, Sigmai, Vx,
                                 Vxx, cost, dV, stats, iters, fx, fu, fc, cx, cu, cxx, cxu, cuu);
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
    int rc = enter(h, up, N, B, params, params_batched, &U, false, "ilqgkl");
    if (rc) return rc;
    if ((rc = ilqgkl_cost_check(U, fx, fu, fc, cx, cu, cxx, cxu, cuu))) return rc;
    DDP_CHECK(x0 && Kp && kp && Sp && Sip && R1 && x && u && K && Sigma && Sigmai && Vx && Vxx && cost && dV && stats, "ilqgkl_cost: null argument");
    const size_t n = U->n, m = U->m, T = (size_t)N * B, CL = U->CL;
    const double *dp, *dx0, *dc0, *dKp, *dkp, *dSp, *dSip, *dmf, *dR1, *dl, *dfx, *dfu, *dfc, *dmx, *dmu, *dmxx, *dmxu, *dmuu;
    double *det, *dx, *du, *dK, *dS, *dSi, *dVx, *dVxx, *dc, *ddV, *ds;
    Staging S(h, Staging::OWNED, "user problem");
    S.in(&dp, params, (size_t)U->nparam * (params_batched ? B : 1)); S.in(&dx0, x0, n * T); S.in(&dc0, cost0, (size_t)B); S.in(&dKp, Kp, m * n * T);
    S.in(&dkp, kp, m * T); S.in(&dSp, Sp, m * m * T); S.in(&dSip, Sip, m * m * T);
    S.in(&dmf, model_fx, n * n * (size_t)N * (model_fx_batched ? B : 1)); S.in(&dR1, R1, n * n); S.in(&dl, lims, 2 * m);
    S.in(&dfx, fx, n * n * T); S.in(&dfu, fu, n * m * T); S.in(&dfc, fc, n * T);
    S.in(&dmx, cx, n * T); S.in(&dmu, cu, m * T); S.in(&dmxx, cxx, n * n * T); S.in(&dmxu, cxu, n * m * T); S.in(&dmuu, cuu, m * m * T);
    S.inout(&det, etab, (size_t)3 * B); S.out(&dx, x, n * T); S.out(&du, u, m * T); S.out(&dK, K, m * n * T); S.out(&dS, Sigma, m * m * T);
    S.out(&dSi, Sigmai, m * m * T); S.out(&dVx, Vx, n * T); S.out(&dVxx, Vxx, n * n * T); S.out(&dc, cost, CL * B); S.out(&ddV, dV, (size_t)2 * B);
    S.out(&ds, stats, (size_t)DDP_ILQGKL_NSTATS * B);
    if ((rc = S.commit())) return rc;
    return S.finish(ddp_user_ilqgkl_cost_f64_dev(h, up, N, B, dp, params_batched, o, dx0, dc0, dKp, dkp, dSp, dSip, dmf, model_fx_batched, dR1, dl,
                                                 det, dfx, dfu, dfc, dx, du, dK, dS, dSi, dVx, dVxx, dc, ddV, ds, iters, dmx, dmu, dmxx, dmxu,
                                                 dmuu));
}

}   // extern "C"
