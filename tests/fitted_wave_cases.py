"""Seeded cases of DDP_USER_FITTED_WAVE (ddp_user_rollout_fit_wave, kl.iLQGkl(..., fitted=True, wide=True)), shared by
tests/test_user_fitted_wave_cpu.py and tests/test_gpu_user_fitted_wave.py.  No tests here.

Rollouts: the long double reference is fitted_reference.rollout with the cost closures of the bundled examples.
Loops: kl_wide_cases.loop_case with time-varying tables drawn around its (A, Bm); the reference per trajectory is oracle.np_kl.iLQGkl with
f = the affine table and derivs = the tables plus the derivatives of the quadratic cost."""
import functools

import numpy as np

import fitted_reference as fr
import kl_wide_cases as kc
from test_user_wave_cpu import CHAIN_P, chain_closures, lq_nparam, lq_params

LD = np.longdouble
RTOL = 1e-8

# ------------------------------------------------------------------------------------------------------------------------ rollouts
# name -> (example, n, m, DeviceProblem keywords, group of lanes DDP_WG): the group sizes 8 / 16 / 32, a group wider than n (10x9), a
# ragged last round of rows (33 = 4 * 8 + 1, 34 = 32 + 2, 40 = 2 * 16 + 8) and the corner
SHAPES = {"lq_33x2": ("lq", 33, 2, {}, 8), "lq_10x9": ("lq", 10, 9, {}, 16), "lq_ad_40x12": ("lq_ad", 40, 12, dict(autodiff=True), 16),
          "chain_34x17": ("chain_ad", 34, 17, dict(autodiff=True), 32), "chain_64x32": ("chain_ad", 64, 32, dict(autodiff=True), 32)}
# (B, nalpha, N, policy and limits, per-trajectory parameters): every (B, nalpha) of {(1, 1), (3, 11), (70, 1)}, every N of {1, 2, 37},
# with and without a policy and limits, shared and per-trajectory parameters; (70, 1) at N = 37 with a policy fills several work-groups
# (9 at a group of 8, 35 at a group of 32) whose last one is not full.  A covering table, not the full product (3 x 3 x 2 x 2 = 36 rows
# a shape, 180 references in long double): every value of each factor, every (B, nalpha) with N = 37 and with a short N, N = 1 with a
# policy at B = 1 and at (3, 11), several work-groups with and without a policy.  Not run: (1, 1) at N = 2 and 37, (70, 1) at N = 1,
# and the pairings of policy and parameter kind that the rows do not list
COMBOS = [(3, 11, 37, True, True), (70, 1, 2, False, False), (1, 1, 1, True, False), (70, 1, 37, True, True), (3, 11, 2, False, True),
          (70, 1, 37, False, False), (3, 11, 1, True, True)]
ROLLOUTS = [(s, ci) for s in SHAPES for ci in range(len(COMBOS))]


def chain_cost(p, J):
    """(stage, None) of the chain with J links on the parameters p, in the scalar type of x, u"""
    def stage(x, u, i):
        return chain_closures(p.astype(x.dtype), J)[1](x, u)
    return stage, None


@functools.lru_cache(maxsize=None)
def rollout_case(shape, ci):
    ex, n, m, kw, wg = SHAPES[shape]
    B, na, N, closed, per_traj = COMBOS[ci]
    rng = np.random.default_rng(4000 + 10 * sorted(SHAPES).index(shape) + ci)
    nb = B if per_traj else 1
    if ex.startswith("chain"):
        P = np.repeat(CHAIN_P[:, None], nb, axis=1)
        P[4] *= 1 + 0.1 * np.arange(nb); P[5] *= 1 + 0.2 * np.arange(nb)         # per-trajectory weights of the cost
        costs = [chain_cost(P[:, b], m) for b in range(nb)]
        nparam = 7
    else:
        Q = [fr._spd(rng, n) for _ in range(nb)]
        R = [fr._spd(rng, m) for _ in range(nb)]
        P = np.stack([lq_params(np.zeros((n, n)), np.zeros((n, m)), Q[b], R[b]) for b in range(nb)], -1)
        costs = [fr.lq_cost(Q[b], R[b]) for b in range(nb)]
        nparam = lq_nparam(n, m)
    fx = np.asfortranarray(np.eye(n)[:, :, None, None] + 0.1 / np.sqrt(n) * rng.standard_normal((n, n, N, B)))
    fu = np.asfortranarray(0.05 * rng.standard_normal((n, m, N, B)))
    fc = np.asfortranarray(0.01 * rng.standard_normal((n, N, B)))
    x0 = 0.5 * rng.standard_normal((n, B))
    u = 0.3 * rng.standard_normal((m, N, B))
    x = 0.5 * rng.standard_normal((n, N, B))
    K, k = 0.3 / np.sqrt(n) * rng.standard_normal((m, n, N, B)), 0.2 * rng.standard_normal((m, N, B))
    al = np.array([1.0]) if na == 1 else np.concatenate([[1.0], 10.0 ** np.linspace(-0.3, -3, na - 1)])
    lims = np.stack([-0.3 * np.ones(m), 0.25 * np.ones(m)], 1) if closed else None
    return dict(shape=shape, example=ex, n=n, m=m, kw=kw, wg=wg, nparam=nparam, B=B, N=N, al=al, closed=closed, per_traj=per_traj,
                P=np.asfortranarray(P if per_traj else P[:, 0]), costs=costs if per_traj else costs * B, fx=fx, fu=fu, fc=fc, x0=x0, u=u,
                x=x, K=K, k=k, lims=lims, wrap=0)


def rollout_reference(c):
    """(xnew[n,N,B,na], unew[m,N,B,na], cnew[CL,B,na]) of the long double rollout, rounded to float64"""
    n, m, N, B, na = c["n"], c["m"], c["N"], c["B"], len(c["al"])
    CL = N + 1 if c["costs"][0][1] is not None else N
    xr, ur, cr = np.zeros((n, N, B, na)), np.zeros((m, N, B, na)), np.zeros((CL, B, na))
    pol = dict(K=None) if not c["closed"] else None
    for b in range(B):
        stage, terminal = c["costs"][b]
        for a, alpha in enumerate(c["al"]):
            kw = pol or dict(K=c["K"][..., b], k=c["k"][..., b], x=c["x"][..., b], alpha=alpha)
            xs, us, cs = fr.rollout(c["x0"][:, b], c["u"][..., b], c["fx"][..., b], c["fu"][..., b], c["fc"][..., b], stage, terminal,
                                    lims=c["lims"], wrap=c["wrap"], **kw)
            xr[..., b, a], ur[..., b, a], cr[:, b, a] = xs.astype(float), us.astype(float), cs.astype(float)
    return xr, ur, cr


# --------------------------------------------------------------------------------------------------------------------------- loops
# (n, m, T, limits).  LQ_LOOPS run on the wave `lq` problem; at (64, 32) its parameter block, 11 264 doubles, does not fit
# DDP_USER_MAX_NPARAM, and (40, 4, 40) of kl_wide_cases.LOOPS stands in — without limits, as there: with limits the reference's count of
# backward passes at (40, 4, 40) moves under perturbations of TIE_EPS (a tie, measured on the CPU), which the GPU test must not meet.
# The reference of (64, 32, 24) is held to the same conditions in the CPU suite, and so is CHAIN_LOOP: the tables of (64, 32, 24) under the
# cost of chain_ad (32 links, 7 parameters), which is how the corner runs on the GPU against a reference
LQ_LOOPS = [(33, 9, 30, False), (33, 9, 30, True), (12, 12, 40, False), (12, 12, 40, True), (40, 4, 40, False)]
CPU_LOOPS = LQ_LOOPS + [(64, 32, 24, False), (64, 32, 24, True)]
CHAIN_LOOP = (64, 32, 24)


@functools.lru_cache(maxsize=None)
def affine_loop_case(n, m, T, lims_on):
    """kl_wide_cases.loop_case with tables fx, fu, fc [.,.,T,B] around its (A, Bm); x is the float64 rollout of u on the tables"""
    c = dict(kc.loop_case(n, m, T, lims_on))
    B, h = c["B"], 0.01
    rng = np.random.default_rng(977 + n + m)
    fx = c["A"][:, :, None, None] + 1e-3 * h * rng.standard_normal((n, n, T, B))
    fu = c["Bm"][:, :, None, None] + 1e-3 * h * rng.standard_normal((n, m, T, B))
    fc = 0.05 * h * rng.standard_normal((n, T, B))
    fx[:, :, T - 1] = 0.0; fu[:, :, T - 1] = 0.0; fc[:, T - 1] = 0.0
    u = c["u"]
    x = np.zeros((n, T, B)); x[:, 0] = c["x"][:, 0]
    for t in range(T - 1):
        x[:, t + 1] = np.einsum("ijb,jb->ib", fx[:, :, t], x[:, t]) + np.einsum("iqb,qb->ib", fu[:, :, t], u[:, t]) + fc[:, t]
    cost0 = 0.5 * np.einsum("itb,ij,jtb->b", x, c["Q"], x) + 0.5 * np.einsum("itb,ij,jtb->b", u, c["R"], u)
    c.update(x=x, cost0=cost0, tfx=np.asfortranarray(fx), tfu=np.asfortranarray(fu), tfc=np.asfortranarray(fc))
    return c


def other_dynamics(c):
    """another drawn matrix A for the parameters of the problem (item 6: the loop must plan on the tables, not on this)"""
    import scipy.linalg as sla
    A0 = np.random.default_rng(5).standard_normal((c["n"], c["n"]))
    return sla.expm(0.05 * (A0 - A0.T))


def lq_table_closures(c, b):
    """(f, costfun, derivs) of trajectory b for oracle.np_kl.iLQGkl: f the affine table, derivs the tables and Q x, R u, Q, 0, R"""
    fx, fu, fc, Q, R = c["tfx"][..., b], c["tfu"][..., b], c["tfc"][..., b], c["Q"], c["R"]
    n, m, T = c["n"], c["m"], c["T"]

    def f(x, u, i):
        return fx[:, :, i] @ x + fu[:, :, i] @ u + fc[:, i]

    def costfun(x, u):
        return 0.5 * np.einsum("it,ij,jt->t", x, Q, x) + 0.5 * np.einsum("it,ij,jt->t", u, R, u)

    def derivs(x, u):
        return (fx, fu, Q @ x, R @ u, np.repeat(Q[:, :, None], T, 2), np.zeros((n, m, T)), np.repeat(R[:, :, None], T, 2))
    return f, costfun, derivs


def chain_table_closures(c, b):
    """the same with the cost of chain_ad (CHAIN_P, m links, n = 2 m): f the affine table, derivs the tables and the chain's cost derivatives"""
    fx, fu = c["tfx"][..., b], c["tfu"][..., b]
    _, costfun, df = chain_closures(CHAIN_P, c["m"])

    def derivs(x, u):
        return (fx, fu) + tuple(df(x, u)[2:])
    return lq_table_closures(c, b)[0], costfun, derivs


def chain_cost0(c):
    """the chain's cost of the nominal (x, u) of an affine loop case, per trajectory"""
    costfun = chain_closures(CHAIN_P, c["m"])[1]
    return np.array([costfun(c["x"][..., b], c["u"][..., b]).sum() for b in range(c["B"])])


def _np_loop(c, b, x, u, chain=False):
    from oracle import np_kl
    f, cf, derivs = (chain_table_closures if chain else lq_table_closures)(c, b)
    n, m, T = c["n"], c["m"], c["T"]
    pb = dict(K=np.zeros((m, n, T)), k=u, S=c["eye"][..., b], Si=c["eye"][..., b])
    return np_kl.iLQGkl(f, cf, derivs, x, pb, dict(fx=c["tfx"][..., b], R1=c["R1"]), kl_step=kc.LOOP_KL_STEP, lims=c["lims"],
                        max_iter=kc.LOOP_MAX_ITER)


@functools.lru_cache(maxsize=None)
def loop_reference(n, m, T, lims_on, chain=False):
    """oracle.np_kl.iLQGkl of every trajectory on the tables: (x, u, policy, Vx, Vxx, cost, info); chain: under the cost of chain_ad"""
    c = affine_loop_case(n, m, T, lims_on)
    return [_np_loop(c, b, c["x"][..., b], c["u"][..., b], chain) for b in range(c["B"])]


def loop_outcomes_nearby(n, m, T, lims_on, b, seed, chain=False):
    """the reference's outcomes of TIE_DRAWS copies of trajectory b whose x, u are off by TIE_EPS relative"""
    c = affine_loop_case(n, m, T, lims_on)
    rng = np.random.default_rng(seed)
    xb, ub = c["x"][..., b], c["u"][..., b]
    return [kc.outcome(_np_loop(c, b, xb * (1 + kc.TIE_EPS * rng.standard_normal(xb.shape)),
                                ub * (1 + kc.TIE_EPS * rng.standard_normal(ub.shape)), chain)[6]) for _ in range(kc.TIE_DRAWS)]


def loop_bound_share(n, m, T, b, chain=False):
    """share of the controls of trajectory b the reference's solve with limits ends on a bound"""
    u = loop_reference(n, m, T, True, chain)[b][1]
    return float(np.mean(np.abs(np.abs(u) - kc.LOOP_LIM) < 1e-15))
