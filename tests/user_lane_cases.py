"""Cases, references and device-call helpers of the contract tests of the default (lane) user-problem kernels: ddp_user_rollout,
ddp_user_df / ddp_user_df_ad, ddp_user_cost and ddp_user_hessians (tests/test_user_lane_cpu.py, tests/test_gpu_user_lane.py).

The launch geometry of these kernels is chosen per shape by layout_of (csrc/user_program.hip): DDP_CHUNK time steps per LDS chunk and
DDP_RLANES rollouts per work-group of the rollout, DDP_DFLANES (step, trajectory) pairs per work-group of the derivatives.  SHAPES
holds one shape per regime, EXPECT what layout_of gives them today (the CPU test pins it), and every size below is read from the
layout the library reports, so that the cases stay on the edges (a partial last chunk, a work-group over an α boundary or over two
trajectories) when the layout moves.

References, all independent of the library:
  * rollout()     the closed-loop rollout of forward_pass.jl:17-28 in long double (u + k α, + K diff, clamp, stage cost, successor; the
                  terminal cost on x[:, N-1]) on the long-double models of tests/sample_reference.py;
  * lq_df()       the derivatives of user_examples/lq.hip in closed form in long double; car_closures (moved here from
                  tests/test_gpu_user_problem.py) and test_user_wave_cpu.pend_euler_df are the NumPy derivatives of the car and the
                  pendulum that the suite already compares with;
  * costs()       stage and terminal cost of the same models in long double.
"""
import ctypes as C
import functools
import math
import re

import numpy as np

from sample_reference import MODELS, lq_model

LD = np.longdouble
SENT = tuple(np.uint64(0x7FF8DEAD5EED1230 + i) for i in range(8))    # quiet NaNs, a payload per output


# ---------------------------------------------------------------- car: Python closures (the same formulas as user_examples/car.hip)
def car_closures(p):
    h, gx, gy, ox, oy, r, wo, wu, wt = p

    def f(x, u, i):
        return np.array([x[0] + h * x[3] * np.cos(x[2]), x[1] + h * x[3] * np.sin(x[2]), x[2] + h * u[1], x[3] + h * u[0]])

    def costfun(x, u):
        dx, dy = x[0] - ox, x[1] - oy
        c = 0.5 * wu * (u[0] ** 2 + u[1] ** 2) + wo * np.exp(-(dx * dx + dy * dy) / r ** 2)
        e = x[:, -1]
        return np.concatenate([c, [0.5 * wt * ((e[0] - gx) ** 2 + (e[1] - gy) ** 2 + e[3] ** 2)]])

    def df(x, u):
        n, N = x.shape
        fx = np.zeros((4, 4, N)); fu = np.zeros((4, 2, N))
        for j in range(4):
            fx[j, j] = 1.0
        c, s = np.cos(x[2]), np.sin(x[2])
        fx[0, 2] = -h * x[3] * s; fx[0, 3] = h * c; fx[1, 2] = h * x[3] * c; fx[1, 3] = h * s
        fu[3, 0] = h; fu[2, 1] = h
        dx, dy = x[0] - ox, x[1] - oy
        phi = wo * np.exp(-(dx * dx + dy * dy) / r ** 2); k = -2.0 / r ** 2
        cx = np.zeros((4, N)); cxx = np.zeros((4, 4, N))
        cx[0] = phi * k * dx; cx[1] = phi * k * dy
        cxx[0, 0] = phi * (k + k * k * dx * dx); cxx[1, 1] = phi * (k + k * k * dy * dy); cxx[0, 1] = cxx[1, 0] = phi * k * k * dx * dy
        cx[0, -1] += wt * (x[0, -1] - gx); cx[1, -1] += wt * (x[1, -1] - gy); cx[3, -1] += wt * x[3, -1]
        cxx[0, 0, -1] += wt; cxx[1, 1, -1] += wt; cxx[3, 3, -1] += wt
        cu = wu * u
        cuu = np.zeros((2, 2, N)); cuu[0, 0] = cuu[1, 1] = wu
        return fx, fu, cx, cu, cxx, np.zeros((4, 2, N)), cuu

    return f, costfun, df


# ------------------------------------------------------------------------------------------------------------ shapes and layouts
LQ_NP = lambda n, m: 2 * n * n + n * m + m * m                    # noqa: E731
AD, TERM, CH = dict(autodiff=True), dict(terminal=True), dict(const_hessian=True)
# key -> (example, n, m, nparam, DeviceProblem keywords, wrapped coordinates)
SHAPES = {
    "lq1": ("lq", 1, 1, LQ_NP(1, 1), {}, ()),
    "pend": ("pendcart", 4, 1, 25, TERM, (0,)),
    "car": ("car", 4, 2, 9, TERM, ()),
    "car_ad": ("car_ad", 4, 2, 9, dict(terminal=True, autodiff=True), ()),
    "lq10": ("lq", 10, 2, LQ_NP(10, 2), {}, ()),
    "lq10c": ("lq", 10, 2, LQ_NP(10, 2), CH, ()),
    "lq10_ad": ("lq_ad", 10, 2, LQ_NP(10, 2), AD, ()),
    "lq16": ("lq", 16, 3, LQ_NP(16, 3), {}, ()),
    "lq24": ("lq", 24, 4, LQ_NP(24, 4), {}, ()),
    "lq32c": ("lq", 32, 8, LQ_NP(32, 8), CH, ()),
    "lq32": ("lq", 32, 8, LQ_NP(32, 8), {}, ()),
}
# (DDP_CHUNK, DDP_RLANES, DDP_DFLANES) of layout_of today: the regimes the shapes were chosen for.  ps = 2 m + m n + n doubles per step and
# rollout: chunk = min(16, 63 / ps) while 64 rollouts fit 32 KB, then one step and the rollouts (a power of two) that fit 64 KB.
EXPECT = {"lq1": (15, 64, 64), "pend": (6, 64, 64), "car": (3, 64, 64), "car_ad": (3, 64, 64), "lq10": (1, 64, 16), "lq10c": (1, 64, 32),
          "lq10_ad": (1, 64, 16), "lq16": (1, 64, 8), "lq24": (1, 32, 4), "lq32c": (1, 16, 4), "lq32": (1, 16, 2)}
ROLL_SHAPES = list(SHAPES)
DF_SHAPES = list(SHAPES)
COST_SHAPES = ["car", "lq10"]                                      # one with the terminal slot, one without
BNA = [(1, 1), (3, 11), (70, 1), (23, 3), (2, 16)]                 # (B, nα) of the rollout cases
COST_N, COST_B = (1, 63, 64, 65, 130), 3


def ps_of(key):
    n, m = SHAPES[key][1:3]
    return 2 * m + m * n + n


def make_problem(ddp, key):
    ex, n, m, nparam, kw, wrap = SHAPES[key]
    return ddp.DeviceProblem(ddp.example_source(ex), n, m, nparam=nparam, diff=ddp.WrappedDiff(*wrap) if wrap else None, **kw)


@functools.lru_cache(maxsize=None)
def layout(key):
    """(DDP_CHUNK, DDP_RLANES, DDP_DFLANES) that the library picks for the shape, from the program text (no GPU)"""
    import ddp_amd
    p = make_problem(ddp_amd, key)
    t = ddp_amd._lib.lib().ddp_user_program_text(p.source.encode(), p.n, p.m, p.nparam, p.flags, int(p.diff_mask)).decode()
    return tuple(int(re.search(r"#define %s (\d+)" % k, t).group(1)) for k in ("DDP_CHUNK", "DDP_RLANES", "DDP_DFLANES"))


def roll_N(key):
    chunk = layout(key)[0]
    return sorted({1, 2, 2 * chunk + 1, 37} | ({chunk} if chunk > 1 else set()))


def df_NB(key):
    """(N, B) of the derivative cases: N in {1, 37} x B in {1, 3}, and N B one past a multiple of the lanes of a work-group"""
    dfl = layout(key)[2]
    return sorted({(1, 1), (1, 3), (37, 1), (37, 3), (1, dfl + 1)})


def holes(B):
    a = np.ones(B, np.int32)
    a[1::3] = 0
    if B > 40:
        a[30:37] = 0
    if B == 1:
        a[0] = 0
    return a


def roll_groups(B, na, rlanes, act):
    """per work-group of ddp_user_rollout (rollout rho = ai B + b, rlanes of them per group): (α's in it, inactive and active in it, full)"""
    out = []
    for r0 in range(0, B * na, rlanes):
        rho = np.arange(r0, min(r0 + rlanes, B * na))
        a = act[rho % B] != 0
        out.append((len(set(rho // B)), bool(a.any() and (~a).any()), len(rho) == rlanes))
    return out


def df_groups(N, B, dflanes, act):
    """per work-group of ddp_user_df (row r = b N + i, dflanes of them per group): (trajectories in it, inactive and active in it, full)"""
    out = []
    for r0 in range(0, N * B, dflanes):
        r = np.arange(r0, min(r0 + dflanes, N * B))
        a = act[r // N] != 0
        out.append((len(set(r // N)), bool(a.any() and (~a).any()), len(r) == dflanes))
    return out


# ------------------------------------------------------------------------------------------------------------------------ the models
def model_of(key):
    """(f, stage, terminal or None) in the scalar type of their arguments: x[n,S], u[m,S], p[nparam]"""
    ex, n, m = SHAPES[key][:3]
    if ex.startswith("lq"):
        return lq_model(n, m) + (None,)
    return MODELS["car" if ex.startswith("car") else "pendcart"][:3]


def params_of(key, rng, B, batched):
    """[nparam] or [nparam, B]"""
    from test_gpu_user_problem import car_params, lq_params, pend_params
    ex, n, m = SHAPES[key][:3]
    cols = []
    for b in range(B if batched else 1):
        if ex.startswith("lq"):
            A0 = rng.standard_normal((n, n))
            A = np.eye(n) + 0.05 * (A0 - A0.T) / np.sqrt(n)
            Bm = 0.1 * rng.standard_normal((n, m))
            Q0 = rng.standard_normal((n, n)); R0 = rng.standard_normal((m, m))
            Q = 0.01 * (np.eye(n) + Q0 @ Q0.T / n); R = 0.01 * (np.eye(m) + R0 @ R0.T / m)
            cols.append(lq_params(A, Bm, 0.5 * (Q + Q.T), 0.5 * (R + R.T)))
        elif ex.startswith("car"):
            cols.append(car_params(rng, 1)[:, 0])
        else:
            p = pend_params()
            p[1] *= 1 + 0.1 * (b % 7); p[3] *= 1 - 0.05 * (b % 5)   # length and damping
            cols.append(p)
    return np.stack(cols, axis=1) if batched else cols[0]


def rollout(model, p, x0, u, K=None, k=None, x=None, alpha=(1.0,), lims=None, wrap=(), dtype=LD):
    """one trajectory, every α at once, every operation in `dtype`: x0[n], u[m,N]; policy K[m,n,N], k[m,N] around x[n,N] or none;
    lims[m,2].  Returns xnew[n,N,na], unew[m,N,na], cnew[CL,na]"""
    f, stage, terminal = model
    T = dtype
    p, x0, u, al = (np.asarray(a, dtype=T) for a in (p, x0, u, alpha))
    if K is not None:
        K, k, x = (np.asarray(a, dtype=T) for a in (K, k, x))
    (m, N), n, S = u.shape, x0.shape[0], al.shape[0]
    two_pi = T(2) * np.arccos(T(-1))
    xs, us, cs = np.zeros((n, N, S), T), np.zeros((m, N, S), T), np.zeros((N + (terminal is not None), S), T)
    xh = np.repeat(x0[:, None], S, axis=1)
    for i in range(N):
        uu = np.repeat(u[:, i, None], S, axis=1)
        if K is not None:
            uu = uu + k[:, i, None] * al[None, :]
            d = xh - x[:, i, None]
            for c in wrap:
                d[c] = d[c] - two_pi * np.rint(d[c] / two_pi)
            uu = uu + K[:, :, i] @ d
        if lims is not None:
            L = np.asarray(lims, dtype=T)
            uu = np.minimum(np.maximum(uu, L[:, 0, None]), L[:, 1, None])
        xs[:, i], us[:, i], cs[i] = xh, uu, stage(xh, uu, i, p)
        if i < N - 1:
            xh = np.asarray(f(xh, uu, i, p), dtype=T)
    if terminal is not None:
        cs[N] = terminal(xh, p)
    return xs, us, cs


def costs(model, p, x, u, dtype=LD):
    """cost[CL] of one trajectory x[n,N], u[m,N]: the stage costs and, with a terminal cost, that of x[:, N-1]"""
    f, stage, terminal = model
    p, x, u = (np.asarray(a, dtype=dtype) for a in (p, x, u))
    N = x.shape[1]
    c = [stage(x[:, i:i + 1], u[:, i:i + 1], i, p)[0] for i in range(N)]
    if terminal is not None:
        c.append(terminal(x[:, N - 1:N], p)[0])
    return np.array(c, dtype=dtype)


def lq_df(p, n, m, x, u, dtype=LD):
    """fx, fu, cx, cu, cxx, cxu, cuu of user_examples/lq.hip on x[n,N], u[m,N]: A, B, Q x, R u, Q, 0, R (no symmetrisation: the example's own)"""
    p, x, u = (np.asarray(a, dtype=dtype) for a in (p, x, u))
    o = np.cumsum([0, n * n, n * m, n * n, m * m])
    A, Bm, Q, R = (p[o[j]:o[j + 1]].reshape(s, order="F") for j, s in enumerate(((n, n), (n, m), (n, n), (m, m))))
    N = x.shape[1]
    rep = lambda M: np.repeat(M[:, :, None], N, axis=2)            # noqa: E731
    return rep(A), rep(Bm), Q @ x, R @ u, rep(Q), np.zeros((n, m, N), dtype), rep(R)


# ------------------------------------------------------------------------------------------------------------------ rollout cases
def roll_cases(key):
    """[(N, B, nα, policy, limits, per-trajectory parameters)]: N x (B, nα), the options cycled over them (every (B, nα) meets every
    (policy, limits) pair: its five N fall on case numbers that differ by 5 = 1 mod 4).  A case with fewer than two controls takes no
    limits: it could not hold a clamped and a free one."""
    m = SHAPES[key][2]
    out = []
    for iN, N in enumerate(roll_N(key)):
        for iB, (B, na) in enumerate(BNA):
            c = iN * len(BNA) + iB
            pol, lim = c % 2 == 0, (c // 2) % 2 == 1
            if m * N * B * (na if pol else 1) < 2:
                lim = False
            out.append((N, B, na, pol, lim, B > 1 and c % 3 != 0))
    return out


def _roll_inputs(key, N, B, na, pol, lim, batched, seed):
    ex, n, m, _, _, wrap = SHAPES[key]
    rng = np.random.default_rng(seed)
    prm = params_of(key, rng, B, batched)
    x0 = 0.5 * rng.standard_normal((n, B))
    u = 0.4 * rng.standard_normal((m, N, B))
    K = k = x = None
    if pol:
        K = 0.3 * rng.standard_normal((m, n, N, B)) / np.sqrt(n); k = 0.3 * rng.standard_normal((m, N, B))
        x = x0[:, None, :] + 0.1 * rng.standard_normal((n, N, B))
        for c in wrap:                                               # the nominal angles whole turns away, never none
            turns = rng.integers(-2, 3, (N, B))
            turns[turns == 0] = 1
            x[c] += 2 * np.pi * turns
    lims = np.stack([-0.3 - 0.2 * rng.uniform(size=m), 0.3 + 0.2 * rng.uniform(size=m)], axis=1) if lim else None
    return dict(key=key, n=n, m=m, N=N, B=B, na=na, pol=pol, lim=lim, batched=batched, wrap=wrap, prm=prm, x0=x0, u=u, K=K, k=k, x=x, lims=lims,
                alpha=10.0 ** np.linspace(0, -3, na), seed=seed)


def roll_reference(c, dtype=LD):
    """xnew[n,N,B,na], unew[m,N,B,na], cnew[CL,B,na] of a case in `dtype`"""
    mdl = model_of(c["key"])
    out = []
    for b in range(c["B"]):
        pol = (None, None, None) if not c["pol"] else (c["K"][..., b], c["k"][..., b], c["x"][..., b])
        out.append(rollout(mdl, c["prm"][:, b] if c["batched"] else c["prm"], c["x0"][:, b], c["u"][..., b], *pol, c["alpha"], c["lims"],
                           c["wrap"], dtype))
    return tuple(np.stack([o[j] for o in out], axis=-2) for j in range(3))


def clamp_census(c, un):
    """(controls on a bound, controls strictly inside) of unew[m,N,B,na]"""
    lo, hi = c["lims"][:, 0, None, None, None], c["lims"][:, 1, None, None, None]
    on = (un == lo) | (un == hi)
    return int(on.sum()), int(((un > lo) & (un < hi)).sum())


@functools.lru_cache(maxsize=None)
def roll_case(key, N, B, na, pol, lim, batched):
    """the inputs of one case and its long-double reference (`ref`).  A case with limits takes the first seed of its sequence whose
    reference holds a control on a bound and one inside (the CPU test asserts it for all of them)."""
    base = 7919 * ROLL_SHAPES.index(key) + 1009 * N + 31 * B + na
    for attempt in range(200):
        c = _roll_inputs(key, N, B, na, pol, lim, batched, base + 100003 * attempt)
        c["ref"] = roll_reference(c)
        if not lim or min(clamp_census(c, c["ref"][1])) > 0:
            return c
    raise AssertionError("no seed gives %s N=%d B=%d na=%d a clamped and a free control" % (key, N, B, na))


# --------------------------------------------------------------------------------------------------- derivative and cost cases
def _points(key, rng, N, B):
    """x[n,N,B], u[m,N,B] to differentiate at"""
    ex, n, m = SHAPES[key][:3]
    if ex.startswith("car"):                                         # as test_car_derivatives_match_the_python_closures
        x = rng.uniform(0, 4, (n, N, B)); x[2] = rng.uniform(-3, 3, (N, B))
        return x, rng.standard_normal((m, N, B))
    return 0.6 * rng.standard_normal((n, N, B)), 0.5 * rng.standard_normal((m, N, B))


@functools.lru_cache(maxsize=None)
def df_case(key, N, B):
    """inputs (per-trajectory parameters when B > 1, except the pendulum: pend_euler_df takes one set) and `ref`, the seven arrays
    [.., N, B] in float64 of the reference named in the module's text"""
    ex, n, m = SHAPES[key][:3]
    rng = np.random.default_rng(31 * DF_SHAPES.index(key) + 7 * N + B)
    batched = B > 1 and ex != "pendcart"
    prm = params_of(key, rng, B, batched)
    x, u = _points(key, rng, N, B)
    per = []
    for b in range(B):
        p = prm[:, b] if batched else prm
        if ex.startswith("lq"):
            per.append(lq_df(p, n, m, x[..., b], u[..., b]))
        elif ex.startswith("car"):
            per.append(car_closures(p)[2](x[..., b], u[..., b]))
        else:
            from test_user_wave_cpu import pend_euler_df
            per.append(pend_euler_df(p, x[..., b], u[..., b]))
    ref = tuple(np.stack([np.asarray(r[j]) for r in per], axis=-1).astype(np.float64) for j in range(7))
    return dict(key=key, n=n, m=m, N=N, B=B, batched=batched, prm=prm, x=x, u=u, ref=ref)


def df_tolerance(key):
    """lq and the pendulum: 1e-10 (tests/test_gpu_user_wave.py); the car against car_closures: 1e-8 (tests/test_gpu_user_problem.py)"""
    return 1e-8 if SHAPES[key][0].startswith("car") else 1e-10


def cost_reference(c, dtype=LD):
    mdl = model_of(c["key"])
    return np.stack([costs(mdl, c["prm"][:, b], c["x"][..., b], c["u"][..., b], dtype) for b in range(c["B"])], axis=-1)


@functools.lru_cache(maxsize=None)
def cost_case(key, N):
    """x[n,N,B], u[m,N,B], per-trajectory parameters and `ref`, cost[CL,B] in long double"""
    ex, n, m = SHAPES[key][:3]
    rng = np.random.default_rng(977 * COST_SHAPES.index(key) + N)
    prm = params_of(key, rng, COST_B, True)
    x, u = _points(key, rng, N, COST_B)
    c = dict(key=key, n=n, m=m, N=N, B=COST_B, prm=prm, x=x, u=u)
    c["ref"] = cost_reference(c)
    return c


def cost_csum_bound(CL):
    """|csum - Σ c| <= this · Σ|c| for ddp_user_cost: a lane adds its ceil(CL / 64) costs in order, then six butterfly steps over the 64
    lanes; every addition errs by at most 2^-53 of its partial sum, which is at most Σ|c|"""
    return (6 + math.ceil(CL / 64)) * 2.0 ** -53


# ------------------------------------------------------------------------------------------------------------- device-call helpers
def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


class Dev:
    """device buffers of one call, freed at exit"""

    def __init__(self, h):
        from ddp_amd import _lib
        self.h, self.L, self.bufs = h, _lib.lib(), []

    def alloc(self, nbytes):
        p = self.h.malloc(max(int(nbytes), 8))
        self.bufs.append(p)
        return p.value

    def copy_in(self, dst, a):
        from ddp_amd import _lib
        _lib.check(self.L.ddp_memcpy_h2d(self.h.raw, C.c_void_p(dst), a.ctypes.data_as(C.c_void_p), C.c_size_t(a.nbytes)))

    def put(self, a, dtype=np.float64):
        if a is None:
            return None
        a = np.asfortranarray(a, dtype=dtype)
        p = self.alloc(a.nbytes)
        self.copy_in(p, a)
        return p

    def sentinel(self, shape, which):
        p = self.alloc(8 * int(np.prod(shape)))
        self.copy_in(p, np.full(int(np.prod(shape)), SENT[which], np.uint64))
        return p

    def get(self, p, shape):
        return self.h.to_host(C.c_void_p(p), shape)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        for p in self.bufs:
            self.h.free(p)
        self.bufs = []


def vp(p):
    return C.c_void_p(p)


def dev_rollout(ddp, prob, prm, K, k, x0, u, x, alpha, lims, active):
    """ddp_user_forward_pass_f64_dev on sentinel-filled outputs -> xnew[n,N,B,na], unew[m,N,B,na], cnew[CL,B,na], csum[B,na], kernel name"""
    from ddp_amd import _lib
    h = ddp.default_handle()
    n, B = x0.shape
    m, N = u.shape[:2]
    al = np.ascontiguousarray(alpha, np.float64)
    na, CL = len(al), prob.cost_len(N)
    shapes = ((n, N, B, na), (m, N, B, na), (CL, B, na), (B, na))
    with Dev(h) as d:
        outs = [d.sentinel(s, i) for i, s in enumerate(shapes)]
        ops = [d.put(a) for a in (prm, K, k, x0, u, x)]
        dl, da = d.put(lims), d.put(active, np.int32)
        _lib.check(d.L.ddp_user_forward_pass_f64_dev(h.raw, prob._ptr(h), N, B, vp(ops[0]), int(np.ndim(prm) == 2), *map(vp, ops[1:]),
                                                     al.ctypes.data_as(C.c_void_p), na, vp(dl), vp(da), *map(vp, outs)))
        h.sync()
        return [d.get(p, s) for p, s in zip(outs, shapes)] + [h.last_kernel(1)]


def df_shapes(prob, N, B):
    n, m = prob.n, prob.m
    ht = () if prob.const_hessian else (N,)
    return ((n, n, N, B), (n, m, N, B), (n, N, B), (m, N, B), (n, n) + ht + (B,), (n, m) + ht + (B,), (m, m) + ht + (B,))


def dev_df(ddp, prob, prm, x, u, active, hessians=True):
    """ddp_user_df_f64_dev on sentinel-filled outputs -> fx, fu, cx, cu, cxx, cxu, cuu, kernel name.  hessians=False: NULL in place of
    the three Hessian outputs (their buffers are read back all the same: nothing may have found them)"""
    from ddp_amd import _lib
    h = ddp.default_handle()
    n, N, B = x.shape
    shapes = df_shapes(prob, N, B)
    with Dev(h) as d:
        outs = [d.sentinel(s, i) for i, s in enumerate(shapes)]
        dp, dx, du, da = d.put(prm), d.put(x), d.put(u), d.put(active, np.int32)
        given = outs if hessians else outs[:4] + [None] * 3
        _lib.check(d.L.ddp_user_df_f64_dev(h.raw, prob._ptr(h), N, B, vp(dp), int(np.ndim(prm) == 2), vp(dx), vp(du), vp(da), *map(vp, given)))
        h.sync()
        name = h.last_kernel(2)
        return [d.get(p, s) for p, s in zip(outs, shapes)] + [name]


def dev_cost(ddp, prob, prm, x, u, active, csum=True):
    """ddp_user_costfun_f64_dev on sentinel-filled outputs -> cost[CL,B], csum[B], kernel name.  csum=False: NULL in its place"""
    from ddp_amd import _lib
    h = ddp.default_handle()
    n, N, B = x.shape
    shapes = ((prob.cost_len(N), B), (B,))
    with Dev(h) as d:
        outs = [d.sentinel(s, i) for i, s in enumerate(shapes)]
        dp, dx, du, da = d.put(prm), d.put(x), d.put(u), d.put(active, np.int32)
        _lib.check(d.L.ddp_user_costfun_f64_dev(h.raw, prob._ptr(h), N, B, vp(dp), int(np.ndim(prm) == 2), vp(dx), vp(du), vp(da), vp(outs[0]),
                                                vp(outs[1] if csum else None)))
        h.sync()
        return [d.get(p, s) for p, s in zip(outs, shapes)] + [h.last_kernel(3)]
