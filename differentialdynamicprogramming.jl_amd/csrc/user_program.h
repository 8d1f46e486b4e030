// user_program.h — what user_problem.hip takes from user_program.hip: the road from (source, n, m, nparam, nc, flags, diff_wrap) to a
// gfx950 code object, and the launch layout that was compiled into it.
#pragma once
#include <vector>

namespace user_program {

// chunk length and rollouts per work-group of ddp_user_rollout, (step, trajectory) pairs per work-group of ddp_user_df, and the same counts
// of the sampled kernels (s: ddp_user_sample, f: ddp_user_rollout_fit, c: ddp_user_cost_fit); every member is a #define of the program
struct Layout { int chunk, rlanes, dflanes, adj, adh, wg, schunk, slanes, fchunk, flanes, clanes, cchunk, csb; };
Layout layout_of(int n, int m, int flags);

// nc < 0: an entry from before DDP_USER_CONSTRAINTS (ddp_user_check, ddp_user_create), which has no way to say how many there are
int validate(const char *source, int n, int m, int nparam, int flags, unsigned wrap, int nc = -1);

// validate, then hiprtc: program text -> gfx950 code object; the log goes to ddp_user_compile_log
int compile(const char *source, int n, int m, int nparam, int flags, unsigned wrap, const char *extra, std::vector<char> *code, int nc = -1);

}   // namespace user_program
