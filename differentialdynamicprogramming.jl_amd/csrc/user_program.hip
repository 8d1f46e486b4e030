// user_program.hip — user-defined problems, from the user's source to a code object: the flags that go together (validate), the launch
// layout of a shape (layout_of), the program text handed to hiprtc (program_text, with_clock) and the compile itself, for gfx950.
//
// user_problem.hip loads what compile() returns and launches it; nothing here touches the device.  hiprtc is loaded at first use
// (dlopen), like RCCL in comm.hip: the library has no link-time dependency on it.
#include <dlfcn.h>
#include <string.h>
#include <mutex>
#include <string>
#include <vector>
#include "ddp_internal.h"
#include "user_program.h"
#include "user_autodiff.h"
#include "user_constraints.h"
#include "user_problem_kernels.h"
#include "user_problem_wave_kernels.h"
#include "user_sample_kernels.h"
#include "user_sample_wave_kernels.h"
#include "user_fitted_kernels.h"
#include "user_fitted_wave_kernels.h"
#include "user_cost_fit_kernels.h"
#include "boxqp_dev_text.h"      // kBoxqpDevText: the text of boxqp_dev.h (written by build.py)
#include "philox_text.h"         // kPhiloxText: the text of philox.h (written by build.py)
#include "wide_kernel_text.h"    // kWideTileText, kWideKernelText: the texts of wide_tile.h and back_pass_wide_kernel.h (written by build.py)

namespace user_program {

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

static Hiprtc *hiprtc()
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

static std::mutex g_log_mu;
static std::string g_log;                                   // log of the last compile (ddp_user_compile_log)

// LDS budgets of the generated kernels (per 64-lane work-group): the rollout keeps several waves per CU (its time loop is a
// dependency chain, latency is hidden by more rollouts in flight), the derivative kernel is a stream of stores
constexpr int ROLL_LDS = 32 * 1024, DF_LDS = 64 * 1024, MAX_LDS = 64 * 1024, FIT_LDS = 48 * 1024, COST_FIT_LDS = 48 * 1024;

// bytes of LDS of ddp_user_rollout_fit with `lanes` rollouts per work-group and `chunk` steps per chunk: u, x, k, K and the tables fx, fu,
// fc per rollout at odd strides, and the two slot arrays
static size_t fit_lds(int n, int m, int lanes, int chunk)
{
    const int ps = 2 * m + m * n + n, ts = n * n + n * m + n;
    return (size_t)lanes * (((chunk * ps) | 1) + ((chunk * ts) | 1) + 1) * 8;
}

// bytes of LDS of ddp_user_cost_fit with `lanes` (step, trajectory) pairs per work-group and `csb` sample indices per round: per lane the
// derivatives and the sums (cx, cu, cxx, cxu, cuu each), c0, the nominal and csb samples at an odd stride, and the slot array
static size_t cost_fit_lds(int n, int m, int lanes, int csb)
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
        // ddp_user_rollout_fit_wave (DDP_USER_FITTED_WAVE): the groups of ddp_user_rollout_wave, a step at a time, nothing staged
        if (flags & DDP_USER_FITTED_WAVE) { L.flanes = L.rlanes; L.fchunk = 1; }
    }
    return L;
}

// `name` appears in `src` as a whole identifier (outside // and /* */ comments)
static bool has_identifier(const std::string &src, const char *name)
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
static std::string with_clock(const char *text)
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

int validate(const char *source, int n, int m, int nparam, int flags, unsigned wrap, int nc)
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
                         DDP_USER_COST_FIT | DDP_USER_SAMPLE_WAVE | DDP_USER_FITTED_WAVE)) == 0,
              "user problem: unknown flags 0x%x", flags);
    // deferred, not impossible: the sampled kernels keep a lane's state in registers or its cost derivatives in LDS (n <= 32, m <= 8) and hand
    // the user's functions neither a clock nor multipliers
    static const struct { int flag; const char *name, *kernel; } sampled[] = {{DDP_USER_SAMPLE, "DDP_USER_SAMPLE", "ddp_user_sample"},
                                                                              {DDP_USER_FITTED, "DDP_USER_FITTED", "ddp_user_rollout_fit"},
                                                                              {DDP_USER_COST_FIT, "DDP_USER_COST_FIT", "ddp_user_cost_fit"}};
    for (const auto &s : sampled) {
        if (!(flags & s.flag)) continue;
        DDP_CHECK(!(flags & DDP_USER_SECOND_ORDER_WAVE), "user problem: %s | DDP_USER_SECOND_ORDER_WAVE is refused (deferred: %s is sized for "
                                                         "n <= %d, m <= %d)", s.name, s.kernel, DDP_MAX_N_USER, DDP_MAX_M);
        DDP_CHECK(!wave, "user problem: %s | DDP_USER_WAVE is refused (deferred: %s is sized for n <= %d, m <= %d)", s.name, s.kernel,
                  DDP_MAX_N_USER, DDP_MAX_M);
        DDP_CHECK(!(flags & DDP_USER_CLOCK), "user problem: %s | DDP_USER_CLOCK is refused (deferred: %s takes no clock)", s.name, s.kernel);
        DDP_CHECK(!(flags & DDP_USER_CONSTRAINTS), "user problem: %s | DDP_USER_CONSTRAINTS is refused (deferred: %s takes no multipliers)",
                  s.name, s.kernel);
    }
    if (flags & DDP_USER_SAMPLE_WAVE) {
        // the sampler at the wave sizes is a flag of its own (DDP_USER_SAMPLE | DDP_USER_WAVE stays refused, as it always was); deferred, not
        // impossible: ddp_user_sample_wave hands the user's functions neither a clock nor multipliers, as ddp_user_sample
        DDP_CHECK(wave, "user problem: DDP_USER_SAMPLE_WAVE needs DDP_USER_WAVE (ddp_user_sample_wave runs in the layout of "
                        "ddp_user_rollout_wave; without DDP_USER_WAVE the sampler is DDP_USER_SAMPLE)");
        DDP_CHECK(!(flags & DDP_USER_CLOCK), "user problem: DDP_USER_SAMPLE_WAVE | DDP_USER_CLOCK is refused (deferred: ddp_user_sample_wave "
                                             "takes no clock)");
        DDP_CHECK(!(flags & DDP_USER_CONSTRAINTS), "user problem: DDP_USER_SAMPLE_WAVE | DDP_USER_CONSTRAINTS is refused (deferred: "
                                                   "ddp_user_sample_wave takes no multipliers)");
    }
    if (flags & DDP_USER_FITTED_WAVE) {
        // the fitted rollout at the wave sizes is a flag of its own (DDP_USER_FITTED | DDP_USER_WAVE stays refused, as it always was);
        // deferred, not impossible: ddp_user_rollout_fit_wave hands the user's cost neither a clock nor multipliers, as ddp_user_rollout_fit
        DDP_CHECK(wave, "user problem: DDP_USER_FITTED_WAVE needs DDP_USER_WAVE (ddp_user_rollout_fit_wave runs in the layout of "
                        "ddp_user_rollout_wave; without DDP_USER_WAVE the fitted rollout is DDP_USER_FITTED)");
        DDP_CHECK(!(flags & DDP_USER_CLOCK), "user problem: DDP_USER_FITTED_WAVE | DDP_USER_CLOCK is refused (deferred: "
                                             "ddp_user_rollout_fit_wave takes no clock)");
        DDP_CHECK(!(flags & DDP_USER_CONSTRAINTS), "user problem: DDP_USER_FITTED_WAVE | DDP_USER_CONSTRAINTS is refused (deferred: "
                                                   "ddp_user_rollout_fit_wave takes no multipliers)");
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

// one section of the program: its #defines (may be empty), a #line that names it in the compiler's messages, its argument structs, its text
static void section(std::string &s, const char *defines, const char *name, const char *abi, const char *text)
{
    s.append("\n").append(defines).append("#line 1 \"").append(name).append("\"\n").append(abi).append("\n").append(text);
}

// what both second-order programs put in front of their kernels: ddp_ad_vhess, and the Cholesky and box-QP of boxqp_dev.h
static void second_order_prelude(std::string &s)
{
    s.append("\n#define DDP_SECOND_ORDER 1\n#line 1 \"ddp_user_autodiff_vhess\"\n").append(kUserAutodiffVhess);
    s.append("\n#line 1 \"ddp_boxqp_dev\"\n").append(kUserRsqrt).append(kBoxqpDevText);
}

static std::string program_text(const char *source, int n, int m, int nparam, int flags, unsigned wrap, int nc = 0)
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
    if (con) section(s, "", "ddp_user_constraints_kernels", DDP_USER_ABI_C_TEXT, kUserConstraintsKernels);
    // every tail below: a problem without its flag keeps the text above, nothing more; the tails come in this order
    if (flags & DDP_USER_SECOND_ORDER) {
        second_order_prelude(s);
        section(s, "", "ddp_user_kernels2", DDP_USER_ABI2_TEXT, kUserKernels2Head);
        s += kUserKernels2Bp2;
        s += kUserKernels2Vhess;
    }
    if (flags & DDP_USER_SECOND_ORDER_WAVE) {                    // the wave program above, then the wide kernel's step and its curvature phase
        second_order_prelude(s);
        s += "\n#line 1 \"ddp_wide_tile\"\n";
        s += kUserWidePrelude;
        s += kWideTileText;
        s += "\n#line 1 \"ddp_back_pass_wide_kernel\"\n";
        s += kWideKernelText;
        section(s, "", "ddp_user_kernels2", DDP_USER_ABI2_TEXT, DDP_USER_ABI3_TEXT);     // (two blocks of argument structs)
        s += "\n";
        s += kUserKernels2Head;
        s += kUserKernels2Vhess;
        s += "\n#line 1 \"ddp_user_kernels2_wave\"\n";
        s += kUserKernels2Wave;
    }
    if (flags & DDP_USER_SAMPLE) {
        snprintf(head, sizeof head, "#define DDP_SLANES %d\n#define DDP_SCHUNK %d\n#line 1 \"ddp_philox\"\n", L.slanes, L.schunk);
        s += "\n";
        s += head;
        s += kPhiloxText;
        section(s, "", "ddp_user_kernels_sample", DDP_USER_ABI_SAMPLE_TEXT, kUserKernelsSample);
    }
    if (flags & DDP_USER_FITTED) {
        snprintf(head, sizeof head, "#define DDP_FLANES %d\n#define DDP_FCHUNK %d\n", L.flanes, L.fchunk);
        section(s, head, "ddp_user_kernels_fit", DDP_USER_ABI_FIT_TEXT, kUserKernelsFit);
    }
    if (flags & DDP_USER_COST_FIT) {
        snprintf(head, sizeof head, "#define DDP_CLANES %d\n#define DDP_CCHUNK %d\n#define DDP_CSB %d\n", L.clanes, L.cchunk, L.csb);
        section(s, head, "ddp_user_kernels_cost_fit", DDP_USER_ABI_COST_FIT_TEXT, kUserKernelsCostFit);
    }
    if (flags & DDP_USER_SAMPLE_WAVE) {                          // (never next to DDP_USER_SAMPLE: one copy of philox.h and of the struct)
        s += "\n#line 1 \"ddp_philox\"\n";
        s += kPhiloxText;
        section(s, "", "ddp_user_kernels_sample_wave", DDP_USER_ABI_SAMPLE_TEXT, kUserKernelsSampleWave);
    }
    if (flags & DDP_USER_FITTED_WAVE)                            // (never next to DDP_USER_FITTED: one copy of the struct)
        section(s, "", "ddp_user_kernels_fit_wave", DDP_USER_ABI_FIT_TEXT, kUserKernelsFitWave);
    return s;
}

// hiprtc: program text -> gfx950 code object; the log goes to g_log
int compile(const char *source, int n, int m, int nparam, int flags, unsigned wrap, const char *extra, std::vector<char> *code, int nc)
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

}   // namespace user_program

using namespace user_program;

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

}   // extern "C"
