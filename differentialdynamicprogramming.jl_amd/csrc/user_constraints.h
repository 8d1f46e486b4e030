// user_constraints.h — state and path constraints of a user problem (DDP_USER_CONSTRAINTS), as program text for hiprtc.
//
// With the flag the user's source also defines
//   template <class T> __device__ void constraints(const T *x, const T *u, int i, const double *p, T *g);      g[DDP_NC], feasible: g[j] <= 0
// and program_text() (user_problem.hip) places two texts around it:
//   kUserConstraintsBefore   renames the user's stage_cost to ddp_user_stage_cost
//   kUserConstraintsAfter    takes the name back and defines the library's stage_cost: the user's cost plus the
//                            Powell-Hestenes-Rockafellar term  ψ = Σ_j (max(0, λ_ij + μ g_j)² − λ_ij²) / (2μ)  for μ > 0, 0 for μ <= 0
// Every kernel of the program (rollout, cost, the AD derivatives, lane or wave) calls stage_cost by name with deduced types, so each of
// them evaluates the augmented cost and not a byte of their text changes; terminal_cost and dynamics are untouched.
//
// λ and μ reach the model through p.  Such a problem is compiled with the stride DDP_NP = nparam + 2, and before every launch the library
// assembles one block per trajectory on the device (bind() of user_problem.hip, always batched):
//   [ the user's nparam parameters | μ_b | the bits of the pointer to λ[:, :, b] ]
// The user's own indices into p are unchanged.  The wrapper reads μ = p[DDP_NP - 2]; only with μ > 0 it moves the 8 bytes of the last
// slot into a pointer (a plain move: the bits are preserved) and reads λ_ij = lam[j + DDP_NC i].
//
// kUserConstraintsAfter uses no device builtin or include: with __device__ defined as nothing it compiles as host C++ next to
// kUserAutodiff, which is how tests/test_user_constraints_cpu.py checks ψ, its gradient and its Hessian without a GPU.
//
//   ddp_user_constraints   g[nc, N, B] on given (x, u): one lane per (step, trajectory); the lane's g goes through LDS and the array
//                          leaves as the contiguous run of the work-group's pairs, like the arrays of ddp_user_df.
//   ddp_user_al_update     one round of the multiplier update, one wave per trajectory that is still live: g on the solution,
//                          cviol = max_ij max(0, g_ij) and Σ raw cost reduced in a fixed order (each lane its steps in ascending
//                          order, then a butterfly over the lanes), then the decision of ddp_user_ilqg_al (ddp_amd.h) and, for a
//                          trajectory that goes on, λ ← max(0, λ + μ g), μ ← min(mu_factor μ, mu_max), both without contraction,
//                          so that a host that applies the same formula to the returned g gets the same bits.
#pragma once

#define DDP_USER_ABI_C                                                                                                                \
    struct UserConArgs {                                                                                                             \
        int N, B;                                                                                                                    \
        const double *params, *x, *u;                                                                                                \
        double *g;                                                                                                                   \
    };                                                                                                                               \
    struct UserAlArgs {                                                                                                              \
        int N, B, round, max_outer;                                                                                                  \
        double mu_factor, mu_max, ctol;                                                                                              \
        const double *params, *x, *u, *stats;                                                                                        \
        double *lambda, *mu, *g, *al_stats;                                                                                          \
        int *live, *counter;                                                                                                         \
    };
#define DDP_USER_ABI_C_TEXT DDP_USER_STR(DDP_USER_ABI_C)

static const char *kUserConstraintsBefore = "#define stage_cost ddp_user_stage_cost\n";

static const char *kUserConstraintsAfter = R"DDPC(
#undef stage_cost
// the augmented stage cost: what every kernel of the program calls stage_cost
template <class T> __device__ T stage_cost(const T *x, const T *u, int i, const double *p)
{
    T c = ddp_user_stage_cost(x, u, i, p);
    const double mu = p[DDP_NP - 2];
    if (mu > 0.0) {
        const double *lam;
        __builtin_memcpy(&lam, p + (DDP_NP - 1), sizeof lam);
        lam += DDP_NC * i;
        T g[DDP_NC];
        constraints(x, u, i, p, g);
        const double h = 0.5 / mu;
#pragma unroll
        for (int j = 0; j < DDP_NC; ++j) {
            const double l = lam[j];
            const T t = l + mu * g[j];
            if (t > 0.0) c += (t * t - l * l) * h;
            else c -= l * l * h;
        }
    }
    return c;
}
)DDPC";

static const char *kUserConstraintsKernels = R"DDPC(
#define DDP_CS (DDP_NC | 1)
extern "C" __global__ __launch_bounds__(64) void ddp_user_constraints(UserConArgs a)
{
    constexpr int n = DDP_N, m = DDP_M, nc = DDP_NC;
    __shared__ double lds[64 * DDP_CS];
    const int lane = threadIdx.x, N = a.N;
    const long R = (long)N * a.B, r0 = (long)blockIdx.x * 64, r = r0 + lane;
    if (r < R) {
        const int b = (int)(r / N), i = (int)(r - (long)b * N);
        double x[n], u[m], g[nc];
#pragma unroll
        for (int l = 0; l < n; ++l) x[l] = a.x[(size_t)n * r + l];
#pragma unroll
        for (int q = 0; q < m; ++q) u[q] = a.u[(size_t)m * r + q];
        constraints(x, u, i, a.params + (size_t)DDP_NP * b, g);
#pragma unroll
        for (int j = 0; j < nc; ++j) lds[lane * DDP_CS + j] = g[j];
    }
    ddp_wave_sync();
    for (int e = lane; e < 64 * nc; e += 64) {
        const int t = e / nc, j = e - t * nc;
        if (r0 + t < R) a.g[(size_t)nc * (size_t)r0 + e] = lds[t * DDP_CS + j];
    }
}

extern "C" __global__ __launch_bounds__(64) void ddp_user_al_update(UserAlArgs a)
{
#pragma clang fp contract(off)
    constexpr int n = DDP_N, m = DDP_M, nc = DDP_NC;
    const int b = blockIdx.x, lane = threadIdx.x, N = a.N;
    if (b >= a.B || a.live[b] == 0) return;
    const double *p = a.params + (size_t)DDP_NP * b;
    double *gb = a.g + (size_t)nc * N * b, *lb = a.lambda + (size_t)nc * N * b;
    double viol = 0.0, raw = 0.0;
    for (int i = lane; i < N; i += 64) {
        double x[n], u[m], g[nc];
#pragma unroll
        for (int l = 0; l < n; ++l) x[l] = a.x[(size_t)n * ((size_t)N * b + i) + l];
#pragma unroll
        for (int q = 0; q < m; ++q) u[q] = a.u[(size_t)m * ((size_t)N * b + i) + q];
        constraints(x, u, i, p, g);
#pragma unroll
        for (int j = 0; j < nc; ++j) {
            gb[nc * i + j] = g[j];
            viol = g[j] > viol ? g[j] : viol;
        }
        raw += ddp_user_stage_cost(x, u, i, p);
#if DDP_TERMINAL
        if (i == N - 1) raw += terminal_cost(x, p);
#endif
    }
    for (int off = 32; off >= 1; off >>= 1) {
        const double v2 = __shfl_xor(viol, off, 64), r2 = __shfl_xor(raw, off, 64);
        viol = v2 > viol ? v2 : viol;
        raw += r2;
    }
    const double mu = a.mu[b];
    const int inner = (int)a.stats[8 * b];
    int status = 0;
    if (a.round == 0 && inner == -1) status = -1;
    else if (viol <= a.ctol) status = 1;
    else if (a.round + 1 >= a.max_outer) status = 2;
    if (status == 0) {
        // every lane rereads the g it wrote itself
        for (int i = lane; i < N; i += 64) {
#pragma unroll
            for (int j = 0; j < nc; ++j) {
                const double t = lb[nc * i + j] + mu * gb[nc * i + j];
                lb[nc * i + j] = t > 0.0 ? t : 0.0;
            }
        }
    }
    if (lane == 0) {
        double *s = a.al_stats + 6 * b;
        s[0] = (double)status;
        s[1] = (double)(a.round + 1);
        s[2] += a.stats[8 * b + 1];
        s[3] = mu;
        s[4] = viol;
        s[5] = raw;
        if (status == 0) {
            const double mn = a.mu_factor * mu;
            a.mu[b] = mn < a.mu_max ? mn : a.mu_max;
            atomicAdd(a.counter, 1);
        } else {
            a.live[b] = 0;
        }
    }
}
)DDPC";
