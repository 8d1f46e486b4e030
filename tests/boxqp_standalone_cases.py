"""Designed box-QPs for the stand-alone solvers behind ddp_boxqp_f64[_dev] (boxqp_kernel<1..8> of csrc/capi.hip, one lane per problem;
boxqp_big_kernel of csrc/boxqp_big.hip, one work-group per problem, 8 < m <= DDP_QP_MAX_M), with the long-double reference of
tests/boxqp_designed_cases.py on every one of them.  No test in this file, no GPU, no oracle.

small_qps(m)      m = 1..8: the QPs the designed table already holds for the in-kernel solvers (every step of every call of the first
                  group of that m; m = 6, which no group runs, through ("general", 6, 6)), as one list; a batch is a slice of it
big_batches(m)    m in M_BIG: name -> list of problems.  "main<k>": the clamp patterns, free-set shapes and sizes, warm starts, box shapes
                  and the many-iteration problem under the default options; "pivot": matrices that lose a pivot of the first
                  factorisation (result 0); one batch per option set of OPTION_SETS (the options are per call).
                  The issue asks for one batch per m and for at most 6 problems in a launch from m = 511 up (8 m^2 bytes of host memory
                  per problem and array).  The listed items are more than 6, so the list of an m is cut into launches of at most
                  BATCH_MAX(m) problems: main0, main1, ...
stack             the operands of a list of problems as the batch arrays boxQP takes
compare           what tests/test_gpu_boxqp_standalone.py asserts of the outputs of a launch (result, free set, x to RTOL and bit-equal on
                  the bounds, the factor and the zeros around it); here, so that it can be shown without a GPU to reject a faulty solver

A problem is a dict: H, g, lo, up, x0 (float64), opts (None or the options that differ from the defaults), tag, pivot (True: result 0
by design, x is clamp(x0) bit for bit and Hfree is not compared), and the reference's x (long double), result, free, iters, trace."""
import functools

import numpy as np

from boxqp_designed_cases import GROUPS, LD, OPTS, _clamp, _design, _spd, call_names, chol_lower, ref_boxqp, reference

M_SMALL = tuple(range(1, 9))
M_BIG = (9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 513, 743, 744, 768, 1023, 1024)
SMALL_COUNTS = (1, 63, 64, 65, None)                       # None: the whole list; 63 and 65 leave a partly filled last wave
NFREE_TARGETS = (16, 17, 255, 256, 257)                    # m >= 257: both sides of the 16-wide unrolling and of the 256 column slots
OPTION_SETS = {"maxIter1": dict(maxIter=1), "maxIter2": dict(maxIter=2), "maxIter3": dict(maxIter=3),
               "minStep": dict(Armijo=0.9999, stepDec=0.5, minStep=0.3), "minGrad": dict(minGrad=1e3), "minRelImprove": dict(minRelImprove=0.5),
               # not in the issue's list: a full Newton step inside the box has the ratio 1/2 < 0.6 and the step 0.6 has 0.7, so every
               # iteration goes 60 % of the way, the clamped set stays and the kept factor is solved with again (factor_reused_solve);
               # under the default options a set that repeats is the converged one, and the kept factor is only returned
               "reuse": dict(Armijo=0.6)}
OPTION_EXIT = {"maxIter1": 1, "maxIter2": 1, "maxIter3": 1, "minStep": 2, "minGrad": 5, "minRelImprove": 4, "reuse": None}
SPEC, SPEC_HARD = (0.05, 5.0), (0.03, 10.0)                # spectra of H: cond <= 100, and <= 334 for the many-iteration problems
# (m, tag) -> draw, where the first draw misses a condition of tests/test_boxqp_standalone_cpu.py (none does so far); for "iter" the draw
# at which the search for a problem with four iterations, two set changes and a kept factor begins
DRAW = {}
RTOL = 1e-8


def BATCH_MAX(m):
    return 12 if m <= 257 else 6


# ------------------------------------------------------------------------------------------------------------------- small m
def small_group(m):
    """(family, n) of the back_pass calls whose QPs the stand-alone kernel of this m replays"""
    for family, n, mm in GROUPS:
        if mm == m:
            return family, n
    return "general", 6                                    # m = 6: no group of the in-kernel table runs it; the generic family takes it


@functools.lru_cache(maxsize=None)
def small_qps(m):
    family, n = small_group(m)
    out = []
    for name in call_names(m):
        ref = reference(family, n, m, name)
        for b, steps in enumerate(ref["qps"]):
            for i in sorted(steps):
                out.append(dict(steps[i], tag="%s/%d/%d" % (name, b, i), opts=None, pivot=False))
    return out


def small_batches(m):
    """name -> list of problems: slices of the one list"""
    qps = small_qps(m)
    return {"all" if c is None else "first%d" % c: qps[:c] for c in SMALL_COUNTS}


# ------------------------------------------------------------------------------------------------------------------- large m
def _rng(m, tag, extra=0):
    return np.random.default_rng([2718, m, sum(ord(ch) * (i + 1) for i, ch in enumerate(tag)), DRAW.get((m, tag), 0) + extra])


def _box(rng, m):
    return -rng.uniform(0.2, 0.5, m), rng.uniform(0.2, 0.5, m)


def _free_pat(rng, m, free):
    pat = rng.integers(1, 3, m)
    pat[np.asarray(free, int)] = 0
    return pat


def _near(rng, pat, xs, lo, up, wrong=3):
    """a start next to the designed minimiser: x* with `wrong` of its clamped coordinates moved into the box and `wrong` of its free ones
    put on a bound, so that the first factorisation is about the size of the last one (from inside the box the first free set is
    everything, and a long-double factorisation of m = 1024 takes seconds)"""
    x0 = xs.copy()
    cl = np.flatnonzero((pat > 0) & (lo < up))
    fr = np.flatnonzero(pat == 0)
    for i in rng.permutation(cl)[:wrong]:
        x0[i] = xs[i] + (0.1 if pat[i] == 1 else -0.1)
    for i in rng.permutation(fr)[:wrong]:
        x0[i] = lo[i] if np.isfinite(lo[i]) else up[i]
    return x0


@functools.lru_cache(maxsize=None)
def _shared_H(m):
    return _spd(_rng(m, "H"), m, *SPEC)


def _problem(m, tag, pat, start="zero", box=None, rng=None):
    """a QP whose minimiser has the clamp pattern pat.  start: "zero" (inside every box that has an interior), "near" (_near), "outside"
    (beyond the bound the minimiser sits on, where it has one), "free_off" (x* with its free coordinates moved: the clamped set is right
    from the first iteration and the second one finds nothing to do), or a function of (rng, pat, x*, lo, up).  From m = 511 up the
    problems of an m share one H (an orthogonal factor of that size is the larger part of building a problem); g, box and start differ"""
    rng = rng or _rng(m, tag)
    H = _shared_H(m) if m >= 511 else _spd(rng, m, *SPEC)
    lo, up = _box(rng, m)
    if box is not None:
        box(lo, up)
    g, xs = _design(rng, H, lo, up, np.asarray(pat))
    pat = np.where(xs == lo, 1, np.where(xs == up, 2, 0))
    if start == "zero":
        x0 = np.zeros(m)
    elif start == "near":
        x0 = _near(rng, pat, xs, lo, up)
    elif start == "outside":
        x0 = xs + np.where(pat == 1, -1.0, np.where(pat == 2, 1.0, 0.0))
    elif start == "free_off":
        w = np.where(np.isfinite(up - lo), up - lo, 1.0)                     # free coordinates sit 20 .. 80 % into their box
        x0 = np.where(pat == 0, xs + 0.1 * w * rng.uniform(-1, 1, m), xs)
    else:
        x0 = start(rng, pat, xs, lo, up)
    return dict(H=H, g=g, lo=lo, up=up, x0=np.asarray(x0, float), opts=None, tag=tag, pivot=False, pat=pat, xs=xs)


def _hard(m, tag, rng=None):
    """a wide spectrum and a Newton point well outside the box in many coordinates: the clamped set moves for several iterations"""
    rng = rng or _rng(m, tag)
    H = _spd(rng, m, *SPEC_HARD)
    lo, up = _box(rng, m)
    xn = 0.5 * (lo + up) + rng.standard_normal(m) * (up - lo) * rng.choice([0.3, 1.0, 3.0], m)
    return dict(H=H, g=-(H @ xn), lo=lo, up=up, x0=np.zeros(m), opts=None, tag=tag, pivot=False)


def _iter_problem(m):
    """the first _hard draw with >= 4 iterations, >= 2 changes of the clamped set after the first iteration and an iteration whose
    set is the previous one's (the factor is kept); searched in float64 from DRAW's entry on"""
    for t in range(200):
        p = _hard(m, "iter", rng=_rng(m, "iter", t))
        x, res, free, it, tr = ref_boxqp(p["H"], p["g"], p["lo"], p["up"], p["x0"], dtype=np.float64)
        if res >= 4 and 4 <= it <= 30 and tr["changes"] >= 2 and "factor_reused" in tr["events"] and tr["margin"] >= 1e-4:
            p["draw"] = DRAW.get((m, "iter"), 0) + t
            return p
    raise AssertionError("no many-iteration problem for m = %d" % m)


def _pivot_problem(m, tag, nfree, j):
    """an SPD matrix whose pivot j of the factorisation of the first iteration's free block is turned into its negative (j = None: a
    NaN on a free diagonal entry).  The start is the designed minimiser, so the first free set is the designed one"""
    rng = _rng(m, tag)
    free = np.sort(rng.permutation(m)[:nfree])
    p = _problem(m, tag, _free_pat(rng, m, free), rng=rng)
    p["x0"] = p["xs"].copy()
    H = p["H"] = p["H"].copy()
    if j is None:
        H[free[nfree // 2], free[nfree // 2]] = np.nan
    else:
        L = chol_lower(H[np.ix_(free, free)])
        H[free[j], free[j]] -= 2.0 * L[j, j] ** 2           # pivot j: d -> d - 2 d; the pivots before it keep their bits
    p.update(pivot=True, first_free=free, lost=j)
    return p


def _main_problems(m):
    big = m >= 511
    start = "near" if big else "zero"
    some = lambda rng, k: np.sort(rng.permutation(m)[:k])
    P = [_problem(m, "none", np.zeros(m, int)),
         _problem(m, "all_first_iteration", np.ones(m, int) + (np.arange(m) % 2), start="outside"),
         _problem(m, "all_later", np.ones(m, int) + (np.arange(m) % 3 == 0), start="near" if big else "zero"),
         _problem(m, "all_but_last", _free_pat(_rng(m, "p3"), m, [m - 1]), start=start),
         _problem(m, "all_but_first", _free_pat(_rng(m, "p4"), m, [0]), start=start),
         _problem(m, "only_last", np.r_[np.zeros(m - 1, int), 1 + m % 2])]
    if m > 64:
        P.append(_problem(m, "free_0_63", _free_pat(_rng(m, "p5"), m, np.arange(64)), start=start))
        k = (m - 1) // 64 - 1                               # the last segment that has another one behind it
        r = _rng(m, "p6")
        fr = np.r_[np.flatnonzero(r.uniform(size=64 * k + 63) < 0.5), 64 * k + 63]
        P.append(_problem(m, "ends_at_lane_63", _free_pat(r, m, fr), start=start))
    if m >= 129:
        r = _rng(m, "p7")
        gap = (m + 63) // 64 // 2                           # an inner segment: all of it clamped, free coordinates on both sides
        fr = [i for i in range(m) if i // 64 != gap and (r.uniform() < 0.4 or i in (0, m - 1))]
        P.append(_problem(m, "clamped_segment", _free_pat(r, m, fr), start=start))
    if m >= 257:
        for nf in NFREE_TARGETS:
            r = _rng(m, "nfree%d" % nf)
            P.append(_problem(m, "nfree%d" % nf, _free_pat(r, m, some(r, nf)), start=start))
    nf = max(1, min(m // 3, 200))

    def below(rng, pat, xs, lo, up):
        x0 = _near(rng, pat, xs, lo, up) if big else np.zeros(m)
        x0[[0, m // 2]] = lo[[0, m // 2]] - 0.3
        return x0

    def above(rng, pat, xs, lo, up):
        x0 = _near(rng, pat, xs, lo, up) if big else np.zeros(m)
        x0[[m - 1, m // 3]] = up[[m - 1, m // 3]] + 0.3
        return x0

    def inward(rng, pat, xs, lo, up):                       # a free coordinate of the minimiser started on its bound: the gradient points in
        x0 = xs.copy() if big else np.where(pat == 0, 0.5 * (xs + 0.5 * (lo + up)), xs)
        fr = np.flatnonzero(pat == 0)
        x0[fr[0]], x0[fr[-1]] = lo[fr[0]], up[fr[-1]]
        return x0

    for tag, st in (("warm_below", below), ("warm_above", above), ("warm_on_bound_inward", inward)):
        r = _rng(m, tag)
        P.append(_problem(m, tag, _free_pat(r, m, some(r, nf)), start=st))
    P.append(_iter_problem(m))

    def shapes(lo, up):
        up[m // 2] = lo[m // 2]; up[m - 2] = lo[m - 2]      # lower == upper
        lo[0] = -np.inf; up[m - 1] = np.inf                 # one infinite bound per side
    r = _rng(m, "box_shapes")
    P.append(_problem(m, "box_shapes", _free_pat(r, m, some(r, nf)), start=start, box=shapes))
    return P


def _pivot_problems(m):
    nf = max(4, min(m // 2, 100))
    P = [_pivot_problem(m, "pivot_first", nf, 0), _pivot_problem(m, "pivot_last", nf, nf - 1), _pivot_problem(m, "pivot_nan", nf, None)]
    if m >= 513:
        P.append(_pivot_problem(m, "pivot_beyond_256", 300, 280))
    return P


@functools.lru_cache(maxsize=None)
def _option_base(m):
    """the QPs every option set of an m runs: all clamped at once, the right set from the start (done in iteration 2), one clamped
    coordinate started inside the box (done in iteration 3), and up to m = 257 a pattern found from inside the box, the
    unconstrained and a many-iteration one"""
    big = m >= 511

    def one_wrong(rng, pat, xs, lo, up):
        x0 = np.where(pat == 0, xs + 0.1 * (up - lo) * rng.uniform(-1, 1, m), xs)
        i = np.flatnonzero(pat > 0)[m // 4]
        x0[i] = xs[i] + (0.1 if pat[i] == 1 else -0.1)
        return x0

    nf = max(1, min(m // 3, 200))
    r = _rng(m, "options")
    P = [_problem(m, "all", 1 + (np.arange(m) % 2), start="outside", rng=r),
         _problem(m, "free_off", _free_pat(r, m, np.sort(r.permutation(m)[:nf])), start="free_off", rng=r),
         _problem(m, "one_wrong", _free_pat(r, m, np.sort(r.permutation(m)[:nf])), start=one_wrong, rng=r)]
    if not big:
        P += [_problem(m, "pattern", _free_pat(r, m, np.sort(r.permutation(m)[:nf])), rng=r),
              _problem(m, "none", np.zeros(m, int), rng=r), _hard(m, "hard", rng=r)]
    return P


def _option_problems(m, name):
    return [dict(p, opts=OPTION_SETS[name], tag=name + "/" + p["tag"]) for p in _option_base(m)]


def solve(p, dtype=LD):
    """the reference's answer to a problem, under the problem's own options"""
    o = OPTS if p["opts"] is None else dict(OPTS, **p["opts"])
    x, result, free, iters, trace = ref_boxqp(p["H"], p["g"], p["lo"], p["up"], p["x0"], dtype=dtype, opts=o)
    return dict(x=x, result=result, free=free, iters=iters, trace=trace)


@functools.lru_cache(maxsize=None)
def big_batches(m):
    """name -> list of solved problems"""
    main = _main_problems(m)
    out = {"main%d" % k: main[i:i + BATCH_MAX(m)] for k, i in enumerate(range(0, len(main), BATCH_MAX(m)))}
    out["pivot"] = _pivot_problems(m)
    for name in OPTION_SETS:
        out[name] = _option_problems(m, name)
    for ps in out.values():
        for p in ps:
            p.update(solve(p))
    return out


def batch_opts(problems):
    o = problems[0]["opts"]
    assert all(p["opts"] == o for p in problems)
    return o or {}


# --------------------------------------------------------------------------------------------------------- launches and checks
def stack(problems):
    """H [m,m,count], g, lo, up, x0 [m,count] in column-major order"""
    F = np.asfortranarray
    return (F(np.stack([p["H"] for p in problems], 2)),) + tuple(F(np.stack([p[k] for p in problems], 1)) for k in ("g", "lo", "up", "x0"))


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def compare(problems, x, res, Hf, free, where=()):
    """the outputs of one launch against the reference, every problem; returns the worst distances (x, Hfree).
    result and free: equal.  x: within RTOL of max(1, max|x|), and bit-equal to the bound wherever the reference sits on one.
    Hfree[:nf, :nf]: the transpose of the reference's lower factor for the returned free set within RTOL of its largest entry (exit 4
    returns the previous iteration's set and factor); exactly zero everywhere else, the strict lower triangle of the block included; a
    returned set with no free coordinate leaves nothing but zeros.  A pivot problem: x is clamp(x0) bit for bit, Hfree is not compared."""
    wx, wh = 0.0, 0.0
    for c, p in enumerate(problems):
        w = tuple(where) + (p["tag"], c)
        assert int(res[c]) == p["result"], (w, "result", int(res[c]), p["result"])
        got_free = np.asarray(free[:, c], bool)
        assert np.array_equal(got_free, p["free"]), (w, "free", np.flatnonzero(got_free != p["free"])[:8].tolist())
        if p["pivot"]:
            assert p["result"] == 0
            assert np.array_equal(_bits(x[:, c]), _bits(_clamp(p["x0"], p["lo"], p["up"]))), (w, "x is not clamp(x0) bit for bit")
            continue
        xr = np.asarray(p["x"], LD)
        d = float(np.max(np.abs(np.asarray(x[:, c], LD) - xr)) / max(LD(1), np.max(np.abs(xr))))
        wx = max(wx, d)
        assert d < RTOL, (w, "x", d)
        xf = np.asarray(xr, float)
        on = (xf == p["lo"]) | (xf == p["up"])
        bound = np.where(xf == p["lo"], p["lo"], p["up"])
        assert np.array_equal(_bits(x[on, c]), _bits(bound[on])), (w, "x is not bit-equal to its bound")
        nf = int(p["free"].sum())
        rest = np.array(Hf[:, :, c], dtype=np.float64, copy=True)
        if nf:
            L = p["trace"]["L"]
            assert L.shape == (nf, nf), (w, L.shape, nf)
            want = np.asarray(L.T, LD)
            d = float(np.max(np.abs(np.asarray(rest[:nf, :nf], LD) - want)) / np.max(np.abs(want)))
            wh = max(wh, d)
            assert d < RTOL, (w, "Hfree", d)
            rest[:nf, :nf] = np.tril(rest[:nf, :nf], -1)
        assert np.array_equal(_bits(rest) << np.uint64(1), np.zeros(rest.shape, np.uint64)), \
            (w, "Hfree is not zero outside the factor", np.argwhere(rest != 0)[:4].tolist() or "NaN")
    return wx, wh
