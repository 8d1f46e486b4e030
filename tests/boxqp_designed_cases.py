"""Designed box-QPs for the in-kernel solvers, and a long-double reference to check them with.  No test in this file, no GPU, no oracle.

A control-limited backward step solves boxQP(QuuF, Qu, lims - u, k+) (src/backward_pass.jl:44-61, src/boxQP.jl:46-169).  With fu = 0
the step's QP is chosen by its operands alone: Qu_i = cu_i, QuuF_i = cuu_i + λI (regType 1) or cuu_i (regType 2), the box is lims - u_i
and the warm start is the solution of step i + 1.  One back_pass call with a time-varying cost therefore runs (N - 1) B QPs that this
file designs, in setter -> probe pairs of steps (i + 1, i): the setter's solution is the warm start the probe needs.

ref_boxqp        np.longdouble projected Newton, statement by statement, with a trace of the events it reached and its decision margin
ref_back_pass    the long-double recursion of backward_pass.jl:179-215 with :28-79 around it
kkt              scaled KKT residual and strict-complementarity margin of a point: what certifies the reference itself
brute_force      the minimiser by enumeration of the 3^m active sets (m <= 4): a second opinion that is no projected Newton
GROUPS, calls    the table: one group per (family, n, m), each a list of calls; the QPs depend on (m, call) only, so every family
                 that runs an m meets the same QPs (and the reference's solves are shared through a memo on the QP's bytes)
"""
import functools
import itertools

import numpy as np

LD = np.longdouble
OPTS = dict(maxIter=100, minGrad=1e-8, minRelImprove=1e-8, stepDec=0.6, minStep=1e-22, Armijo=0.1)      # boxQP.jl:30-35
GUARD = 0.59                                   # csrc/boxqp_dev.h, csrc/back_pass_q4.hip: the closed-form back-off's re-entry test


# ------------------------------------------------------------------------------------------------ long-double linear algebra
def chol_lower(A):
    """L with L L' = A (numpy.linalg refuses float128); ValueError where A is not positive definite"""
    n = A.shape[0]
    L = np.zeros_like(A)
    for j in range(n):
        d = A[j, j] - L[j, :j] @ L[j, :j]
        if not d > 0:
            raise ValueError("not positive definite")
        L[j, j] = np.sqrt(d)
        if j + 1 < n:
            L[j + 1:, j] = (A[j + 1:, j] - L[j + 1:, :j] @ L[j, :j]) / L[j, j]
    return L


def chol_solve(L, b):
    """(L L')^-1 b for b [n] or [n, k]"""
    n = L.shape[0]
    y = np.array(b, dtype=L.dtype, copy=True)
    for i in range(n):
        y[i] = (y[i] - L[i, :i] @ y[:i]) / L[i, i]
    for i in range(n - 1, -1, -1):
        y[i] = (y[i] - L[i + 1:, i] @ y[i + 1:]) / L[i, i]
    return y


def _clamp(x, lo, up):
    return np.where(x > up, up, np.where(x < lo, lo, x))          # Julia's clamp


# ---------------------------------------------------------------------------------------------------------------- the box-QP
class _Margin:
    def __init__(self):
        self.v, self.where = np.inf, None

    def __call__(self, dist, what):
        dist = float(dist)
        if dist < self.v:
            self.v, self.where = dist, what


def ref_boxqp(H, g, lo, up, x0, dtype=LD, opts=OPTS):
    """boxQP.jl:46-169 in `dtype`.  Returns x, result, free, iters (the value of `iter` at the exit) and the trace:
    events   set of strings: exit<r>, exit<r>_iter<1|2|3+>, exit6_later, iters3 / iters4 / iters6 (the value of `iter` at the exit), q12,
             armijo_pinned_closed / armijo_pinned_slow / armijo_inside (a line search that fails at step 1), warm_below / warm_above
             (x0 outside the box, clamped at :58), warm_on_bound_inward (x0 on a bound, the gradient pointing into the box),
             factor_reused (an iteration after the first whose clamped set is the previous one's: :104 keeps the factor),
             factor_reused_solve (such an iteration that goes on to the search direction: :127-129 solve with the kept factor)
    margin   the smallest relative distance between a tested quantity and its threshold over every comparison of the run
    guard    for every line search that failed at step 1 with all moving coordinates pinned: |max_j r_j - 0.59| / 0.59, r_j = the step
             at which coordinate j re-enters the box over s* = (old - v(pinned)) / (Armijo |s'g|); the kernels' closed-form back-off
             takes the step iff every r_j <= 0.59
    changes  the number of iterations after the first that found another clamped set and factorised again
    L        lower Cholesky factor of H[free, free] for the RETURNED free set (Q12: on exit 4 both are the previous iteration's)
    A matrix that is not positive definite gives result 0 (backward_pass.jl:48-52 swallows the exception)."""
    H, g, lo, up, x0 = (np.asarray(a, dtype) for a in (H, g, lo, up, x0))
    n = len(g)
    ev, margin, guard = set(), _Margin(), []
    clamped = np.zeros(n, bool); free = np.ones(n, bool)
    oldvalue = dtype(0); result = 0; L = np.zeros((0, 0), dtype); changes = 0
    x = _clamp(x0, lo, up)                                                                  # :58
    if (x0 < lo).any():
        ev.add("warm_below")
    if (x0 > up).any():
        ev.add("warm_above")
    value = x @ g + dtype(0.5) * (x @ (H @ x))                                              # :63
    it = 1
    while it <= opts["maxIter"]:                                                            # :71
        if result != 0:
            break
        if it > 1:                                                                          # :78-81
            imp, thr = oldvalue - value, dtype(opts["minRelImprove"]) * abs(oldvalue)
            margin(abs(imp - thr) / max(thr, dtype(1e-300)), ("improve", it))
            if imp < thr:
                result = 4
                break
        oldvalue = value
        grad = g + H @ x                                                                    # :85
        old_clamped = clamped
        clamped = ((x == lo) & (grad > 0)) | ((x == up) & (grad < 0))                       # :88-95
        on = (x == lo) | (x == up)
        if on.any():
            margin(np.min(np.abs(grad[on]) / np.maximum(np.abs(g[on]), dtype(1e-3))), ("sign", it))
        if it == 1 and (on & ~clamped & (x0 == x) & (lo < up)).any():
            ev.add("warm_on_bound_inward")
        free = ~clamped
        if clamped.all():                                                                   # :98-101
            result = 6
            break
        reused = not (it == 1 or (old_clamped != clamped).any())
        if not reused:                                                                      # :104-117
            changes += it > 1
            try:
                L = chol_lower(H[np.ix_(free, free)])
            except ValueError:
                return x, 0, free, it, dict(events=ev, margin=margin.v, where=margin.where, guard=guard, L=L, changes=changes)
        else:
            ev.add("factor_reused")
        gnorm = np.sqrt(np.sum(grad[free] ** 2))                                            # :120-124
        margin(abs(gnorm - dtype(opts["minGrad"])) / dtype(opts["minGrad"]), ("gnorm", it))
        if gnorm < opts["minGrad"]:
            result = 5
            break
        if reused:
            ev.add("factor_reused_solve")
        grad_clamped = g + H @ (x * clamped)                                                # :127-129
        search = np.zeros(n, dtype)
        search[free] = -chol_solve(L, grad_clamped[free]) - x[free]
        sdotg = np.sum(search * grad)                                                       # :132-135
        margin(abs(sdotg) / max(np.sqrt(np.sum(search ** 2) * np.sum(grad[free] ** 2)), dtype(1e-300)), ("sdotg", it))
        if sdotg >= 0:
            break
        step, nstep = dtype(1), 0                                                           # :138-151
        xc = _clamp(x + step * search, lo, up)
        vc = xc @ g + dtype(0.5) * (xc @ (H @ xc))
        ratio = (vc - oldvalue) / (step * sdotg)
        margin(abs(ratio - dtype(opts["Armijo"])) / dtype(opts["Armijo"]), ("armijo", it, 0))
        if ratio < opts["Armijo"]:
            moving = search != 0
            pinned = moving & (xc == np.where(search > 0, up, lo))
            if (pinned == moving).all():
                sstar = (oldvalue - vc) / (-dtype(opts["Armijo"]) * sdotg)
                r = (np.abs(xc - x)[moving] / np.abs(search[moving])) / sstar if sstar > 0 else np.full(int(moving.sum()), np.inf)
                guard.append(float(abs(np.max(r) - GUARD) / GUARD))          # closed form iff every r_j <= 0.59: the largest decides
                ev.add("armijo_pinned_closed" if (r <= GUARD).all() else "armijo_pinned_slow")
            else:
                ev.add("armijo_inside")
        while ratio < opts["Armijo"]:
            step = step * dtype(opts["stepDec"])
            nstep += 1
            xc = _clamp(x + step * search, lo, up)
            vc = xc @ g + dtype(0.5) * (xc @ (H @ xc))
            if step < opts["minStep"]:
                result = 2
                break
            ratio = (vc - oldvalue) / (step * sdotg)
            margin(abs(ratio - dtype(opts["Armijo"])) / dtype(opts["Armijo"]), ("armijo", it, nstep))
        x, value = xc, vc                                                                   # :161-163
        it += 1
    if it == opts["maxIter"]:                                                               # :167-169
        result = 1
    ev.add("exit%d" % result)
    ev.add("exit%d_iter%s" % (result, it if it <= 2 else "3+"))
    if result == 6 and it >= 2:
        ev.add("exit6_later")
    if it >= 3:
        ev.add("iters3")
    if it >= 4:
        ev.add("iters4")
    if it >= 6:
        ev.add("iters6")
    if result == 4 and (free & ((x == lo) | (x == up)) & (lo < up)).any():
        ev.add("q12")                                # the last step put a coordinate on its bound; the returned set still has it free
    return x, result, free, it, dict(events=ev, margin=margin.v, where=margin.where, guard=guard, L=L, changes=changes)


_MEMO = {}


def _boxqp_memo(H, g, lo, up, x0):
    """ref_boxqp in long double, remembered by the bytes of its operands (with fu = 0 the QPs of a call do not depend on n)"""
    key = b"".join(np.ascontiguousarray(a, LD).tobytes() for a in (H, g, lo, up, x0))
    if key not in _MEMO:
        _MEMO[key] = ref_boxqp(H, g, lo, up, x0)
    return _MEMO[key]


def kkt(H, g, lo, up, x):
    """(residual, margin) of x for min 0.5 x'Hx + x'g on [lo, up], in long double.
    residual: the largest of the bound violations and of the gradient entries that the KKT conditions want zero (all of a coordinate
    strictly inside, the inward part of one on a bound), over max|g|.
    margin (strict complementarity): the smallest of |grad_i| / max|g| over the coordinates on a bound and of the distance to the nearer
    bound over max(1, |x_i|) for the others; a coordinate with lower == upper has no say in either."""
    H, g, lo, up, x = (np.asarray(a, LD) for a in (H, g, lo, up, x))
    grad = g + H @ x
    sc = max(np.max(np.abs(g)), LD(1e-300))
    fixed = lo == up
    at_lo, at_up = (x == lo) & ~fixed, (x == up) & ~fixed
    inside = ~at_lo & ~at_up & ~fixed
    res = max(np.max(np.maximum(lo - x, 0)), np.max(np.maximum(x - up, 0)))
    res = max(res, np.max(np.where(inside, np.abs(grad), 0)), np.max(np.where(at_lo, np.maximum(-grad, 0), 0)),
              np.max(np.where(at_up, np.maximum(grad, 0), 0)))
    mg = [LD(np.inf)]
    if (at_lo | at_up).any():
        mg.append(np.min(np.abs(grad[at_lo | at_up])) / sc)
    if inside.any():
        mg.append(np.min(np.minimum(x - lo, up - x)[inside] / np.maximum(1, np.abs(x[inside]))))
    return float(res / sc), float(min(mg))


def brute_force(H, g, lo, up):
    """the minimiser over the box by enumeration: for each of the 3^m assignments (free / at lower / at upper) solve the free block,
    keep the feasible candidates and return the one of least value (long double).  m <= 4."""
    H, g, lo, up = (np.asarray(a, LD) for a in (H, g, lo, up))
    m = len(g)
    best, bx = None, None
    for pat in itertools.product((0, 1, 2), repeat=m):
        pat = np.array(pat)
        if (np.isinf(lo) & (pat == 1)).any() or (np.isinf(up) & (pat == 2)).any():
            continue
        x = np.where(pat == 1, lo, np.where(pat == 2, up, LD(0)))
        fr = pat == 0
        if fr.any():
            rhs = g[fr] + H[np.ix_(fr, ~fr)] @ x[~fr]
            x[fr] = -chol_solve(chol_lower(H[np.ix_(fr, fr)]), rhs)
        if (x < lo).any() or (x > up).any():
            continue
        v = x @ g + LD(0.5) * (x @ (H @ x))
        if best is None or v < best:
            best, bx = v, x
    return bx


# ----------------------------------------------------------------------------------------------------------- the backward pass
def ref_back_pass(case, regType=None):
    """backward_pass.jl:179-215 (time-varying cost and dynamics) with :28-79, every trajectory, in long double.  Returns a dict of
    float64 arrays K [m,n,N,B], k, Quu, Vx, Vxx, dV [2,B], diverge [B], and qps[b][i] = dict(H, g, lo, up, x0 (float64 images of the
    step's QP), x, result, free, iters, trace)."""
    c = case
    regType = c["regType"] if regType is None else regType
    n, m, N, B = c["n"], c["m"], c["N"], c["B"]
    out = dict(K=np.zeros((m, n, N, B)), k=np.zeros((m, N, B)), Quu=np.zeros((m, m, N, B)), Vx=np.zeros((n, N, B)),
               Vxx=np.zeros((n, n, N, B)), dV=np.zeros((2, B)), diverge=np.zeros(B, np.int32), qps=[dict() for _ in range(B)])
    ld = lambda a: np.asarray(a, LD)
    fx, fu, cxx, cxu, cuu = ld(c["fx"]), ld(c["fu"]), ld(c["cxx"]), ld(c["cxu"]), ld(c["cuu"])
    In, Im = np.eye(n, dtype=LD), np.eye(m, dtype=LD)
    for b in range(B):
        lam = LD(c["lam"][b])
        cx, cu = ld(c["cx"][..., b]), ld(c["cu"][..., b])
        k, K = np.zeros((m, N), LD), np.zeros((m, n, N), LD)
        Vx, Vxx, Quu = np.zeros((n, N), LD), np.zeros((n, n, N), LD), np.zeros((m, m, N), LD)
        dV = np.zeros(2, LD)
        Vx[:, N - 1], Vxx[:, :, N - 1], Quu[:, :, N - 1] = cx[:, N - 1], cxx[:, :, N - 1], cuu[:, :, N - 1]
        for i in range(N - 2, -1, -1):
            fxi, fui, V, v = fx[:, :, i], fu[:, :, i], Vxx[:, :, i + 1], Vx[:, i + 1]
            Qu = cu[:, i] + fui.T @ v
            Qx = cx[:, i] + fxi.T @ v
            Vr = V + (lam * In if regType == 2 else 0)
            Qux_reg = cxu[:, :, i].T + fui.T @ Vr @ fxi
            QuuF = cuu[:, :, i] + fui.T @ Vr @ fui + (lam * Im if regType == 1 else 0)
            Qux = cxu[:, :, i].T + fui.T @ V @ fxi
            Quu[:, :, i] = cuu[:, :, i] + fui.T @ V @ fui
            Qxx = cxx[:, :, i] + fxi.T @ V @ fxi
            lo = ld(c["lims"][:, 0] - c["u"][:, i, b])                   # the bounds in float64, as the kernels form them (:45-46)
            up = ld(c["lims"][:, 1] - c["u"][:, i, b])
            x0 = k[:, min(i + 1, N - 2)]
            ki, result, free, iters, tr = _boxqp_memo(QuuF, Qu, lo, up, x0)
            out["qps"][b][i] = dict(H=np.asarray(QuuF, float), g=np.asarray(Qu, float), lo=np.asarray(lo, float), up=np.asarray(up, float),
                                    x0=np.asarray(x0, float), x=ki, result=result, free=free, iters=iters, trace=tr)
            if result < 1:
                out["diverge"][b] = i + 1
                break
            Ki = np.zeros((m, n), LD)
            if free.any():
                Ki[free] = -chol_solve(tr["L"], Qux_reg[free])
            Quuk = Quu[:, :, i] @ ki                                     # :64-76
            dV += np.array([ki @ Qu, LD(0.5) * (ki @ Quuk)])
            Vx[:, i] = Qx + Ki.T @ Quuk + Ki.T @ Qu + Qux.T @ ki
            W = Qxx + Ki.T @ Quu[:, :, i] @ Ki + Ki.T @ Qux + Qux.T @ Ki
            Vxx[:, :, i] = (W + W.T) / 2
            k[:, i], K[:, :, i] = ki, Ki
        for name, a in (("K", K), ("k", k), ("Quu", Quu), ("Vx", Vx), ("Vxx", Vxx), ("dV", dV)):
            out[name][..., b] = np.asarray(a, float)
    return out


# ------------------------------------------------------------------------------------------------------------------ the table
# family -> (how the GPU test reaches it, the kernel it asserts); the shapes are the issue's
FAMILIES = {
    "q4": ("host", None, "back_pass_q4"), "dpp": ("host", "dpp", "back_pass_dpp_kernel"), "row": ("host", "row", "back_pass_row_kernel"),
    "mxg": ("host", None, "back_pass_mxg_kernel"), "mid": ("host", None, "back_pass_mid_kernel"),
    "mf2": ("host", None, "back_pass_mf2_kernel"), "mf2new": ("host", "new", "back_pass_mf2_kernel"),
    "mfma": ("host", None, "back_pass_mfma_kernel"), "general": ("host", "general", "back_pass_kernel"),
    "big": ("host", "big", "back_pass_big_kernel"), "wide": ("dev", None, "back_pass_wide_kernel"),
}
GROUPS = [("q4", 4, 1), ("dpp", 4, 1), ("dpp", 10, 2), ("row", 5, 1), ("row", 5, 2), ("row", 6, 3), ("row", 7, 4), ("row", 14, 1),
          ("mxg", 3, 1), ("mxg", 6, 2), ("mxg", 6, 3), ("mxg", 8, 4), ("mid", 16, 2), ("mid", 16, 3), ("mid", 15, 5), ("mid", 20, 7),
          ("mid", 32, 8), ("mf2", 33, 1), ("mf2", 33, 5), ("mf2", 40, 8), ("mf2new", 64, 8), ("mfma", 64, 8), ("general", 6, 3),
          ("general", 20, 4), ("big", 20, 4), ("wide", 4, 9), ("wide", 12, 16), ("wide", 5, 17), ("wide", 10, 31), ("wide", 8, 32)]
# the ordinary calls: (regType, λ); then the short horizons, a lims row with lower == upper, an infinite bound per side
ORDINARY = [(1, 1e-3), (1, 1.0), (2, 1e-3), (2, 1.0)]
KINDS = ["rep6", "rep5", "rep4", "q12", "pin_closed", "pin_slow", "arm_inside", "warm_out", "on_bound", "pat", "pat", "pat",
         "hard", "hard", "hard", "hard"]


def call_names(m):
    names = ["ord%d" % i for i in range(len(ORDINARY))] + ["N2", "N3", "inf"]
    return names + (["deg"] if m >= 2 else ["inf2"])         # m = 1: coordinate 0's lims row is the reference's "no limits" switch


def _spd(rng, m, e_lo, e_hi):
    q, _ = np.linalg.qr(rng.standard_normal((m, m)))
    e = 10.0 ** rng.uniform(np.log10(e_lo), np.log10(e_hi), m)
    A = (q * e) @ q.T
    return (A + A.T) / 2


def _hard(rng, m):
    """matrices on which the projected Newton needs many iterations: a wide spectrum, or strongly correlated coordinates
    (ρ ss' + (1 - ρ) I, scaled); redrawn until cond <= 3e3, so that cond(cuu + λI) stays below 1e4"""
    while True:
        if m == 1 or rng.uniform() < 0.4:
            A = _spd(rng, m, 0.003, 10.0)
        else:
            rho, d, sg = rng.uniform(0.9, 0.99), 10.0 ** rng.uniform(-0.4, 0.4, m), rng.choice([-1.0, 1.0], m)
            A = (rho * np.outer(sg, sg) + (1 - rho) * np.eye(m)) * np.outer(d, d)
        if np.linalg.cond(A) <= 3e3:
            return A


def _design(rng, H, lo, up, pat):
    """g such that the minimiser has the clamp pattern pat (0 free, 1 at lower, 2 at upper; an infinite bound turns free): free
    coordinates 20 .. 80 % into the box, multipliers 0.2 .. 1 times the scale of H x on the clamped ones.  Returns g, x*."""
    m = len(lo)
    pat = np.where(((pat == 1) & np.isinf(lo)) | ((pat == 2) & np.isinf(up)), 0, pat)
    pat = np.where((lo == up) & (pat == 0), rng.integers(1, 3, m), pat)      # lower == upper: a zero multiplier there is a tie of the sign test
    w = np.where(np.isfinite(up - lo), up - lo, 1.0)
    th = rng.uniform(0.2, 0.8, m)
    inner = np.where(np.isinf(lo), up - th * w, lo + th * w)
    x = np.where(pat == 1, lo, np.where(pat == 2, up, inner))
    mu = rng.uniform(0.2, 1.0, m) * (0.3 * np.mean(np.diag(H)) + np.max(np.abs(H @ x)))
    g = -(H @ x) + np.where(pat == 1, mu, np.where(pat == 2, -mu, 0.0))
    return g, x


def _patterns(m, count, rng):
    """clamp patterns to cycle through: all 3^m for m <= 2; else every coordinate in each state, 0, 1, m - 1 and m clamped, and the
    last coordinate (the one next to a kernel's padding) in each state with the others mixed"""
    if m <= 2:
        base = [np.array(p) for p in itertools.product((0, 1, 2), repeat=m)]
    else:
        base = [np.zeros(m, int), np.ones(m, int), np.full(m, 2)]
        for j in (m - 1, 0, m // 2):
            for s in (1, 2):
                p = np.zeros(m, int); p[j] = s; base.append(p)                    # one clamped
                p = rng.integers(1, 3, m); p[j] = 0; base.append(p)              # m - 1 clamped
        for s in (0, 1, 2):
            p = rng.integers(0, 3, m); p[m - 1] = s; base.append(p)
    return [base[i % len(base)] for i in range(count)]


@functools.lru_cache(maxsize=None)
def qp_data(m, name):
    """the QP side of a call: dict(regType, lam, N, B', cuu [m,m,N], cu [m,N,6], u [m,N,6], lims [m,2]) for B = 6 trajectories (a
    case with B = 3 takes the first three)"""
    ci = call_names(m).index(name)
    rng = np.random.default_rng(SEEDS.get((m, name), 7000 + 101 * m + ci))
    regType, lam = ORDINARY[ci] if name.startswith("ord") else ORDINARY[(m + ci) % 4]
    N = {"N2": 2, "N3": 3, "inf": 9, "inf2": 9, "deg": 9}.get(name, 33)
    B = 6
    lims = np.stack([-rng.uniform(0.2, 0.5, m), rng.uniform(0.2, 0.5, m)], 1)
    if name == "deg":
        lims[m - 1, 1] = lims[m - 1, 0]
    if name == "inf":
        lims[0, 0] = -np.inf
        if m >= 2:
            lims[m - 1, 1] = np.inf
    if name == "inf2":
        lims[0, 1] = np.inf
    reg = lam if regType == 1 else 0.0
    cuu = np.zeros((m, m, N)); cu = np.zeros((m, N, B)); u = rng.uniform(-0.3, 0.3, (m, N, B))
    w = lims[:, 1] - lims[:, 0]
    box = lambda i, b: (lims[:, 0] - u[:, i, b], lims[:, 1] - u[:, i, b])
    kinds = list(KINDS) if name.startswith("ord") else ["pat"] * 16
    rot = int(rng.integers(0, 16))
    kinds = kinds[rot:] + kinds[:rot]
    pats = _patterns(m, 2 * N * B, rng)
    pi = 0
    # the last step (i = N - 1) has no QP; step N - 2 warm-starts from zeros; then pairs (setter i + 1, probe i)
    steps = list(range(N - 2, -1, -1))
    cuu[:, :, N - 1] = _spd(rng, m, 0.05, 5.0)
    pairs = [(steps[j], steps[j + 1] if j + 1 < len(steps) else None) for j in range(0, len(steps), 2)]
    if N == 33:                                   # 32 steps: one single step first, then 15 pairs and a last single step
        pairs = [(steps[0], None)] + [(steps[j], steps[j + 1]) for j in range(1, 31, 2)] + [(steps[31], None)]
    for pj, (s, p) in enumerate(pairs):
        kind = kinds[pj % 16] if p is not None else "pat"
        hard = kind == "hard"
        cuu[:, :, s] = _hard(rng, m) if hard else _spd(rng, m, 0.05, 5.0)
        if p is not None:
            cuu[:, :, p] = cuu[:, :, s] if kind in ("rep6", "rep5", "rep4", "q12") else (_hard(rng, m) if hard else _spd(rng, m, 0.05, 5.0))
        jq = m - 1 if pj % 2 else int(rng.integers(0, m))         # q12: the coordinate whose box the probe widens, decoupled in H
        if kind == "q12":
            cuu[jq, :, s] = cuu[:, jq, s] = 0.0
            cuu[jq, jq, s] = rng.uniform(0.5, 2.0)
            cuu[:, :, p] = cuu[:, :, s]
        Hs = cuu[:, :, s] + reg * np.eye(m)
        Hp = None if p is None else cuu[:, :, p] + reg * np.eye(m)
        for b in range(B):
            if p is not None:
                u[:, p, b] = u[:, s, b]                                    # same box unless the kind moves it
            lo, up = box(s, b)
            fin = np.where(np.isfinite(lo), lo, up - 1.0), np.where(np.isfinite(up), up, lo + 1.0)
            pat = pats[pi]; pi += 1
            if kind == "pat" or p is None:
                cu[:, s, b], _ = _design(rng, Hs, lo, up, pat)
                if p is not None:
                    cu[:, p, b], _ = _design(rng, Hp, lo, up, pats[pi]); pi += 1
            elif kind == "rep6":
                cu[:, s, b], _ = _design(rng, Hs, lo, up, rng.integers(1, 3, m))
                cu[:, p, b] = cu[:, s, b]
            elif kind in ("rep5", "rep4"):
                if b == 0:
                    pat = np.zeros(m, int)
                elif pat.all():
                    pat = pat.copy(); pat[int(rng.integers(0, m))] = 0
                cu[:, s, b], _ = _design(rng, Hs, lo, up, pat)
                cu[:, p, b] = cu[:, s, b]
                if kind == "rep4":            # ~1e-6 of the largest entry, on every coordinate: |grad_free| stays far above minGrad
                    cu[:, p, b] += 1e-6 * rng.choice([-1.0, 1.0], m) * rng.uniform(0.5, 1.5, m) * max(np.max(np.abs(cu[:, s, b])), 0.1)
            elif kind == "q12":
                pat = pat.copy(); pat[jq] = 1 + b % 2
                g, xs = _design(rng, Hs, lo, up, pat)
                cu[:, s, b] = cu[:, p, b] = g
                val = abs(xs @ g + 0.5 * xs @ Hs @ xs)
                gap = 3e-9 * val / abs((g + Hs @ xs)[jq])
                u[jq, p, b] = u[jq, s, b] + (gap if pat[jq] == 1 else -gap)
            elif kind in ("pin_closed", "pin_slow", "arm_inside"):
                side = rng.integers(0, 2, m)                                             # the corner the probe's Newton point lies beyond
                d = rng.uniform(0.1, 0.3, m) * w
                xs = np.where(side == 1, up - d, lo + d)
                cu[:, s, b] = -(Hs @ xs)                                                 # setter: all free, solution xs
                t = rng.uniform(0.01, 0.02, m)
                sv = np.where(side == 1, 1.0, -1.0) * d / t
                if m >= 2 and kind != "pin_closed":
                    jb = int(rng.integers(0, m))
                    sv[jb] = np.sign(sv[jb]) * d[jb] / 0.5 if kind == "pin_slow" else -np.sign(sv[jb]) * 0.3 * d[jb]
                cu[:, p, b] = -(Hp @ (xs + sv))
            elif kind == "warm_out":
                g, xs = _design(rng, Hs, lo, up, pat)
                cu[:, s, b] = g
                j0 = int(rng.integers(0, m)); j1 = (j0 + 1 + int(rng.integers(0, max(m - 1, 1)))) % m
                if m == 1 and b % 2:
                    j0, j1 = -1, 0
                if j0 >= 0:
                    u[j0, p, b] = lims[j0, 0] - xs[j0] - 0.3 * w[j0]                    # the probe's lower bound above the warm start
                if j1 != j0 and m > 1 or j0 < 0:
                    u[j1, p, b] = lims[j1, 1] - xs[j1] + 0.3 * w[j1]                    # ... upper bound below it
                cu[:, p, b], _ = _design(rng, Hp, *box(p, b), pats[pi]); pi += 1
            elif kind == "on_bound":
                pat = pat.copy()
                if not pat.any():
                    pat[int(rng.integers(0, m))] = 1 + b % 2
                cu[:, s, b], _ = _design(rng, Hs, lo, up, pat)
                cu[:, p, b], _ = _design(rng, Hp, lo, up, np.where(pat > 0, 0, pats[pi])); pi += 1
            elif kind == "hard":
                for st, Hh in ((s, Hs), (p, Hp)):
                    xn = 0.5 * (fin[0] + fin[1]) + rng.standard_normal(m) * w * rng.choice([0.3, 1.0, 3.0], m)
                    cu[:, st, b] = -(Hh @ xn)
    return dict(regType=regType, lam=lam, N=N, cuu=cuu, cu=cu, u=u, lims=lims)


# (m, call) -> seed, where the default draw misses a condition of the table (tests/test_boxqp_designed_cpu.py asserts them all)
SEEDS = {(4, 'ord0'): 91004, (4, 'deg'): 91004, (5, 'ord0'): 91005, (5, 'ord2'): 91005, (7, 'ord0'): 92007, (8, 'ord3'): 93008,
         (9, 'ord2'): 91009, (9, 'ord3'): 91009, (9, 'deg'): 91009, (16, 'ord0'): 98016, (16, 'ord1'): 91016, (16, 'ord2'): 94016,
         (16, 'ord3'): 94016, (16, 'inf'): 91016, (16, 'deg'): 91016, (17, 'ord0'): 92017, (17, 'ord2'): 92017, (31, 'ord0'): 93031,
         (31, 'ord2'): 110031, (31, 'ord3'): 110031, (31, 'deg'): 91031, (32, 'ord0'): 93032, (32, 'ord2'): 93032, (32, 'ord3'): 93032}


@functools.lru_cache(maxsize=None)
def case(family, n, m, name):
    """one back_pass call of the group: operands in layout "FC" (time-varying dynamics and cost, shared by the trajectories), fu = 0,
    fx a well-conditioned near-rotation per step, cx / cu / u per trajectory; keys as tests/wide_controls_cases.bp_case"""
    import scipy.linalg as sla
    q = qp_data(m, name)
    N = q["N"]
    B = 3 if n * m >= 1024 else 6
    rng = np.random.default_rng(1000 * n + 10 * m + call_names(m).index(name))
    fx = np.empty((n, n, N)); cxx = np.empty((n, n, N))
    for i in range(N):
        a = rng.standard_normal((n, n))
        fx[:, :, i] = sla.expm(0.1 * (a - a.T)) * rng.uniform(0.95, 1.02)
        a = rng.standard_normal((n, n))
        cxx[:, :, i] = 0.2 * (a @ a.T / n + 0.5 * np.eye(n))
    F = np.asfortranarray
    return dict(family=family, name=name, n=n, m=m, N=N, B=B, layout="FC", regType=q["regType"], fx=F(fx), fu=F(np.zeros((n, m, N))),
                cxx=F(cxx), cxu=F(0.05 * rng.standard_normal((n, m, N))), cuu=F(q["cuu"]), cx=F(0.3 * rng.standard_normal((n, N, B))),
                cu=F(q["cu"][..., :B]), u=F(q["u"][..., :B]), x=np.zeros((n, N, B), order="F"), lam=np.full(B, q["lam"]), lims=F(q["lims"]))


@functools.lru_cache(maxsize=None)
def reference(family, n, m, name):
    return ref_back_pass(case(family, n, m, name))


def required_events(m):
    """what the traces of a group must show (the issue's coverage list); m = 1 cannot fail Armijo with a coordinate moving inside the
    box (a one-dimensional Newton step that stays inside has ratio 1/2), nor re-enter the box early: one moving coordinate re-enters at
    r = 0.1 / (1 - t / 2) < 0.106"""
    ev = {"exit4", "exit5", "exit6", "exit6_iter1", "exit6_later", "exit5_iter1", "exit4_iter2", "q12", "armijo_pinned_closed",
          "warm_below", "warm_above", "warm_on_bound_inward"}
    if m >= 2:
        ev |= {"armijo_pinned_slow", "armijo_inside", "iters3", "iters4"}
    if m >= 4:
        ev |= {"iters6"}
    return ev
