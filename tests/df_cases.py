"""Designed inputs of the derivative step (csrc/df.hip), shared by tests/test_df_reference_cpu.py and tests/test_gpu_df_reference.py.
No tests here.

A pendcart call is one parameter set and E elements (angle, control); each element records the 1-norm the kernel will compute for its
ZoH block matrix — `kernel_norm`, the double expression of df.hip (df_pendcart_kernel: m10 ... nA) restated with numpy, fmax and all —
and the Padé degree and number of squarings it was designed for (`plan`, the thresholds restated here; the library's own answer,
ddp_df_expm_plan, is compared with it in the CPU test).  The restated norm can differ from the device's in the last place (sin, cos and
a contracted multiply-add); no element sits closer than 4e-4, relative, to a threshold, so its plan does not depend on that.

Column 0 of the block matrix is |g/l cos θ + u/l sin θ| h; `solve_u` picks the control that gives it a target value, with either sign
of the entry: negative (the linearised pendulum oscillates) or positive (it grows)."""
import functools

import numpy as np

from df_reference import BANDS, band_of

DEFAULT = dict(g=9.82, l=0.35, h=0.01, d=0.99, goal=np.array([np.pi, 0.0, 0.0, 0.0]), Q=np.diag([10.0, 1.0, 2.0, 1.0]), R=np.array([[1.0]]))
QFULL = np.array([[10.0, 0.3, -0.2, 0.1], [0.5, 1.0, 0.05, -0.4], [-0.7, 0.2, 2.0, 0.6], [0.15, -0.25, 0.35, 1.0]])      # not symmetric: df reads all of Q
THRESHOLDS = (0.015, 0.25, 0.95, 2.1, 5.4, 10.8)
PAIR_REL = 5e-4                                  # threshold pairs sit at thr (1 -+ PAIR_REL): within 1e-3 on either side


def params(**kw):
    p = dict(DEFAULT)
    p.update(kw)
    return p


SMALL = params(h=0.005, l=5.0)                   # h (1 + d) = 0.00995, (|cos θ| / l + 1) h <= 0.006: column 0 can set a norm down to 0.01
TINY = params(h=0.001, l=5.0, d=0.5)             # floor 0.0015


def kernel_norm(par, x0, u):
    """the norm of df_pendcart_kernel, in double, operation by operation"""
    g, l, h, d = (np.float64(par[k]) for k in ("g", "l", "h", "d"))
    x0 = np.asarray(x0, dtype=np.float64)
    uu = np.asarray(u, dtype=np.float64).copy()
    uu[uu != uu] = 0.0
    with np.errstate(invalid="ignore"):
        sn, cs = np.sin(x0), np.cos(x0)
        m01 = 1.0 * h; m10 = (-g / l * cs - uu / l * sn) * h; m11 = (-d) * h; m23 = 1.0 * h; m14 = (cs / l) * h; m34 = 1.0 * h
        return np.fmax(np.fmax(0.0 + np.abs(m10), np.abs(m01) + np.abs(m11)), np.fmax(np.abs(m23), np.abs(m14) + np.abs(m34)))


def plan(norm):
    """(degree, squarings) of a norm: the thresholds of Higham's scaling and squaring as df.hip states them; (0, 0): not finite"""
    if not np.isfinite(norm):
        return 0, 0
    for thr, deg in ((0.015, 3), (0.25, 5), (0.95, 7), (2.1, 9)):
        if norm <= thr:
            return deg, 0
    return 13, max(0, int(np.ceil(np.log2(norm / 5.4))))


def solve_u(par, theta, target, grow):
    """u with |g/l cos θ + u/l sin θ| h = target; grow: the (1, 0) entry positive"""
    g, l, h = par["g"], par["l"], par["h"]
    v = -target / h if grow else target / h                       # v = g/l cos θ + u/l sin θ; the entry is -v h
    return (v - g / l * np.cos(theta)) * l / np.sin(theta)


class PendCall:
    """E elements under one parameter set; laid out as [*, N, B] with the element index t + N b (the kernel's flat index)"""

    def __init__(self, name, par, theta, u, rest=None, B=1):
        self.name, self.par = name, par
        theta = np.asarray(theta, dtype=np.float64); u = np.asarray(u, dtype=np.float64)
        E = theta.size
        assert E % B == 0 and u.size == E
        self.E, self.B, self.N = E, B, E // B
        rng = np.random.default_rng(E + 17 * len(name))
        rest = rng.standard_normal((3, E)) if rest is None else np.asarray(rest, dtype=np.float64)
        self.xe = np.vstack([theta[None], rest])                  # [4, E]
        self.ue = u.copy()                                        # [E]
        self.norm = kernel_norm(par, theta, u)
        self.plan = [plan(v) for v in self.norm]
        self.band = [band_of(v) if np.isfinite(v) else -1 for v in self.norm]

    @property
    def x(self):
        return np.asfortranarray(self.xe.reshape(4, self.N, self.B, order="F"))

    @property
    def u(self):
        return np.asfortranarray(self.ue.reshape(1, self.N, self.B, order="F"))

    def matrices(self):
        """the 5 x 5 block matrices in double, entry by entry as the kernel forms them: [E, 5, 5]"""
        par = self.par
        g, l, h, d = (np.float64(par[k]) for k in ("g", "l", "h", "d"))
        uu = self.ue.copy(); uu[uu != uu] = 0.0
        sn, cs = np.sin(self.xe[0]), np.cos(self.xe[0])
        M = np.zeros((self.E, 5, 5))
        M[:, 0, 1] = 1.0 * h; M[:, 1, 0] = (-g / l * cs - uu / l * sn) * h; M[:, 1, 1] = (-d) * h
        M[:, 2, 3] = 1.0 * h; M[:, 1, 4] = (cs / l) * h; M[:, 3, 4] = 1.0 * h
        return M


def _ladder_targets(lo, hi, count):
    """count norms inside (lo, hi], log-spaced, clear of both ends"""
    return np.exp(np.linspace(np.log(lo) + 0.06 * np.log(hi / lo), np.log(hi) - 0.06 * np.log(hi / lo), count))


def _angles(count, seed):
    """angles with |sin θ| >= 0.3 (the control stays moderate) and cos θ of both signs"""
    rng = np.random.default_rng(seed)
    th = rng.uniform(0.32, np.pi - 0.32, count) * rng.choice([-1.0, 1.0], count)
    return th


@functools.lru_cache(maxsize=None)
def ladder():
    """>= 8 elements in every band; the sign of the (1, 0) entry alternates.  Band 0 (Padé 3) needs the small-step parameter sets."""
    calls = []
    lo = 0.0
    for i, hi in enumerate(BANDS):
        if i == 0:
            for par, nm, a, b in ((TINY, "tiny", 0.002, 0.0099), (SMALL, "small", 0.0101, 0.015)):
                t = _ladder_targets(a, b, 8); th = _angles(8, 100 + len(calls))
                u = np.array([solve_u(par, th[k], t[k], k % 2 == 1) for k in range(8)])
                calls.append(PendCall("ladder0_" + nm, par, th, u, B=2))
        else:
            if i == 1:                                           # default parameters: the other columns reach 0.0386
                t = _ladder_targets(lo, 0.04, 8); th = _angles(8, 100 + len(calls))
                u = np.array([solve_u(SMALL, th[k], t[k], k % 2 == 1) for k in range(8)])
                calls.append(PendCall("ladder1_small", SMALL, th, u, B=2))
            a = 0.04 if i == 1 else lo
            t = _ladder_targets(a, hi, 10); th = _angles(10, 100 + len(calls))
            u = np.array([solve_u(DEFAULT, th[k], t[k], k % 2 == 1) for k in range(10)])
            calls.append(PendCall("ladder%d" % i, DEFAULT, th, u, B=2))
        lo = hi
    return tuple(calls)


@functools.lru_cache(maxsize=None)
def threshold_pairs():
    """both sides of every threshold, column 0 setting the norm — and 0.015 once more with column 1, h (1 + d), setting it"""
    calls = []
    for j, thr in enumerate(THRESHOLDS):
        par = SMALL if thr == 0.015 else DEFAULT
        th = np.array([0.9, 0.9, -2.1, -2.1])
        t = thr * np.array([1 - PAIR_REL, 1 + PAIR_REL, 1 - PAIR_REL, 1 + PAIR_REL])
        u = np.array([solve_u(par, th[k], t[k], k >= 2) for k in range(4)])
        calls.append(PendCall("pair_%g" % thr, par, th, u, B=2))
    for side, f in (("below", 1 - PAIR_REL), ("above", 1 + PAIR_REL)):
        par = params(l=5.0, h=0.015 * f / 1.99)                    # column 1: h (1 + d); column 0 with |u| <= 0.2 at θ = 1.2, -1.9: below 0.006
        calls.append(PendCall("pair_col1_" + side, par, np.array([1.2, -1.9]), np.array([0.2, -0.1]), B=1))
    return tuple(calls)


@functools.lru_cache(maxsize=None)
def edges():
    """parameter edges: sin θ = 0 (u drops out of the matrix), cos θ = 0, d = 0 and g = 0, a growing exponential, θ of many turns,
    a goal with no zero entry, a full non-symmetric Q, a NaN control"""
    par = params(Q=QFULL, goal=np.array([3.0, -0.7, 1.3, 0.2]), R=np.array([[0.37]]))
    th = np.array([0.0, 0.0, np.pi / 2, -np.pi / 2, 1.0, 2.5, 1e6 + 0.3, -12345.678, 0.7, 4.0])
    u = np.array([1e6, -3.0, 2.0, -250.0, -500.0, -4000.0, 1.5, 60.0, np.nan, 0.0])
    a = PendCall("edges_default", par, th, u, B=2)
    par0 = params(Q=QFULL, d=0.0, g=0.0)
    th0 = np.array([0.0, 0.4, -2.0, np.pi / 2, 3.0, 1.1])
    u0 = np.array([5.0, 0.0, 35.0, -120.0, np.nan, -900.0])
    b = PendCall("edges_d0_g0", par0, th0, u0, B=3)
    return a, b


def all_finite_calls():
    return ladder() + threshold_pairs() + edges()


_REFS = {}


def references(call):
    """long double df of a call, the C oracle's, and the oracle's distance to long double per element — computed once per call.
    Arrays are laid out like the call's x and u ([*, N, B]); d_orc is [E] in the kernel's flat order."""
    if id(call) not in _REFS:
        from oracle import oracle_ctypes as oc
        import df_reference as dr
        fx, fu, cx, cu, cxs, cus = dr.pend_df_ld(call.par, call.x, call.u)
        par = call.par
        p = oc.make_problem("pendcart", 4, 1, call.E, Q=par["Q"], R=par["R"], pend=par)
        ofx, ofu, ocx, ocu = oc.df(p, call.xe, call.ue[None])               # the E elements as one trajectory
        sh = (call.N, call.B)
        ofx, ofu = ofx.reshape((4, 4) + sh, order="F"), ofu.reshape((4, 1) + sh, order="F")
        with np.errstate(invalid="ignore"):
            d_orc = dr.block_distance(ofx, ofu, fx, fu).ravel(order="F")
        _REFS[id(call)] = dict(call=call, fx=fx, fu=fu, cx=cx, cu=cu, cxs=cxs, cus=cus, ofx=ofx, ofu=ofu, d_orc=d_orc)
    return _REFS[id(call)]


def oracle_band_distance(extra=()):
    """d_orc(band): the oracle's worst distance to long double over every designed finite element of the band (and over `extra`,
    pairs (band, distance) of elements a test adds)"""
    worst = [0.0] * len(BANDS)
    for call in all_finite_calls():
        r = references(call)
        for e in range(call.E):
            worst[call.band[e]] = max(worst[call.band[e]], float(r["d_orc"][e]))
    for band, d in extra:
        worst[band] = max(worst[band], float(d))
    return worst


@functools.lru_cache(maxsize=None)
def nonfinite():
    """u = +-Inf (sin θ != 0: the norm is +Inf, the plan is degree 0), θ = NaN and θ = Inf (the sine is NaN; fmax drops it from the norm,
    the element takes the Padé of the remaining columns and comes out NaN by arithmetic), each between ordinary elements — one of them
    with a norm beyond 2.1.  Returns the call, the indices of the non-finite elements, and the same call with those replaced."""
    th = np.array([0.5, 1.0, -0.8, 2.0, 1.3, np.nan, -2.9, np.inf, 0.2, 1.0])
    u = np.array([1.0, np.inf, -2.0, -np.inf, 700.0, 0.5, 0.0, 1.0, -3.0, 2.0])
    bad = np.array([1, 3, 5, 7])
    par = params(Q=QFULL)
    with np.errstate(invalid="ignore"):
        call = PendCall("nonfinite", par, th, u, B=2)
    th2, u2 = th.copy(), u.copy()
    th2[bad] = 0.3; u2[bad] = 0.1
    plain = PendCall("nonfinite", par, th2, u2, rest=call.xe[1:], B=2)
    return call, bad, plain


# ---- LQ: (name, n, m, N, B, NaN control?, active mask?) — tiled kernel: n <= 64 and m <= 16, 256 / n columns per tile
LQ_SHAPES = (
    ("1x1", 1, 1, 7, 3, True, True),
    ("3x1_85_per_tile", 3, 1, 50, 4, True, True),              # 200 columns: 2 full tiles and 30 columns, one idle thread
    ("33x2_7_per_tile", 33, 2, 5, 5, True, True),              # 25 columns: 3 tiles and 4 columns, 25 idle threads
    ("64x16", 64, 16, 3, 3, True, True),                       # 9 columns: 2 tiles and 1 column
    ("5x16", 5, 16, 21, 3, True, True),                        # 63 columns: 1 tile and 12 columns
    ("10x17_column_kernel", 10, 17, 30, 10, True, True),       # m > 16: one thread per column, 300 columns = 2 blocks
    ("10x32_column_kernel", 10, 32, 30, 10, True, True),
    ("64x1_tile_loop_wraps", 64, 1, 129, 256, True, True),     # 33 024 columns = 8 256 tiles of 4: more than the 8 192 blocks
)


@functools.lru_cache(maxsize=None)
def lq_case(name):
    _, n, m, N, B, nan, mask = next(s for s in LQ_SHAPES if s[0] == name)
    rng = np.random.default_rng(1000 * n + m)
    c = dict(n=n, m=m, N=N, B=B, Q=rng.standard_normal((n, n)), R=rng.standard_normal((m, m)),
             x=np.asfortranarray(rng.standard_normal((n, N, B))), u=np.asfortranarray(rng.standard_normal((m, N, B))))
    if nan:
        c["u"][m - 1, N // 2, B - 1] = np.nan
        c["u"][0, 0, 0] = np.nan
    c["active"] = None
    if mask:
        a = np.ones(B, dtype=np.int32); a[1::3] = 0
        c["active"] = a
    return c
