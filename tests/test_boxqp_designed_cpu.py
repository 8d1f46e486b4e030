"""The designed box-QP table of tests/boxqp_designed_cases.py, checked without a GPU: every QP of every call meets the table's conditions
(decisive comparisons, a certified minimiser, strict complementarity), every group reaches the branches the in-kernel solvers have, and
the long-double reference agrees with the C oracle (same path, 1e-9 / 1e-8) and, up to m = 4, with a brute-force enumeration of the
active sets.  tests/test_gpu_boxqp_in_kernel.py then holds every backward-pass kernel family to the same reference."""
import numpy as np
import pytest

from boxqp_designed_cases import GROUPS, ORDINARY, brute_force, call_names, case, kkt, reference, required_events
from conftest import relerr

MARGIN, KKT, STRICT, MAX_ITERS, GUARD_DIST = 1e-6, 1e-12, 1e-6, 50, 0.05
M_VALUES = sorted({m for _, _, m in GROUPS})


def _qps(family, n, m):
    """(call, b, i, qp) over every QP of the group"""
    for name in call_names(m):
        ref = reference(family, n, m, name)
        for b, steps in enumerate(ref["qps"]):
            for i, q in steps.items():
                yield name, b, i, q


def _state(q):
    """per coordinate: 0 strictly inside, 1 at lower, 2 at upper (a coordinate with lower == upper counts as lower)"""
    x = np.asarray(q["x"], float)
    return np.where(x == q["lo"], 1, np.where(x == q["up"], 2, 0))


@pytest.mark.parametrize("m", M_VALUES)
def test_every_qp_meets_the_conditions_and_every_branch_is_reached(m):
    """the QPs of a call depend on (m, call) alone (fu = 0), so one group per m stands for all that share it: test_reference_matches_the_
    oracle_back_pass asserts for every group that its QPs are these"""
    family, n, _ = next(g for g in GROUPS if g[2] == m)
    events, patterns, counts, last, states = set(), set(), set(), set(), [set() for _ in range(m)]
    worst = dict(margin=np.inf, kkt=0.0, strict=np.inf, iters=0, guard=np.inf)
    total = 0
    for name, b, i, q in _qps(family, n, m):
        tr, where = q["trace"], (m, name, b, i)
        total += 1
        res, strict = kkt(q["H"], q["g"], q["lo"], q["up"], q["x"])
        assert tr["margin"] >= MARGIN, (where, tr["margin"], tr["where"])
        assert res <= KKT, (where, res)
        assert strict >= STRICT, (where, strict)
        assert q["result"] >= 1 and q["iters"] <= MAX_ITERS, (where, q["result"], q["iters"])
        assert all(gd >= GUARD_DIST for gd in tr["guard"]), (where, tr["guard"])
        assert np.linalg.cond(q["H"]) <= 1e4, (where, np.linalg.cond(q["H"]))                 # cond(cuu_i + λI)
        worst = dict(margin=min(worst["margin"], tr["margin"]), kkt=max(worst["kkt"], res), strict=min(worst["strict"], strict),
                     iters=max(worst["iters"], q["iters"]), guard=min([worst["guard"]] + tr["guard"]))
        events |= tr["events"]
        st = _state(q)
        patterns.add(tuple(st)); counts.add(int((st > 0).sum())); last.add(int(st[-1]))
        for j in range(m):
            states[j].add(int(st[j]))
    print("m = %d: %d QPs, least margin %.2g, largest KKT residual %.2g, least strict complementarity %.2g, most iterations %d, "
          "least distance from the 0.59 test %.2g" % (m, total, worst["margin"], worst["kkt"], worst["strict"], worst["iters"], worst["guard"]))
    assert not required_events(m) - events, sorted(required_events(m) - events)
    if m <= 2:
        assert len(patterns) == 3 ** m, sorted(patterns)
    assert all(s == {0, 1, 2} for s in states), states
    assert {0, 1, m - 1, m} <= counts, counts
    assert last == {0, 1, 2}
    # the calls themselves: both regTypes with both λ, the short horizons, an infinite bound per side, a lims row with lower == upper
    names = call_names(m)
    assert {(case(family, n, m, nm)["regType"], float(case(family, n, m, nm)["lam"][0])) for nm in names[:4]} == set(ORDINARY)
    assert case(family, n, m, "N2")["N"] == 2 and case(family, n, m, "N3")["N"] == 3
    inf = [case(family, n, m, nm)["lims"] for nm in names if nm.startswith("inf")]
    assert any(np.isneginf(L[:, 0]).any() for L in inf) and any(np.isposinf(L[:, 1]).any() for L in inf)
    if m >= 2:
        L = case(family, n, m, "deg")["lims"]
        assert L[0, 0] < L[0, 1] and (L[1:, 0] == L[1:, 1]).any()


@pytest.mark.parametrize("m", M_VALUES)
def test_reference_boxqp_matches_the_oracle_and_brute_force(m):
    """ref_boxqp against the C oracle's boxqp on the float64 image of every QP: same result code, iteration count and free set, x
    within 1e-9 scaled (the bound of tests/test_gpu_boxqp2.py); up to m = 4 also against the enumeration of the 3^m active sets"""
    from oracle import oracle_ctypes as oc
    family, n, _ = next(g for g in GROUPS if g[2] == m)
    worst, worst_bf = 0.0, 0.0
    for name, b, i, q in _qps(family, n, m):
        xr, rr, Hfr, fr, it = oc.boxqp(q["H"], q["g"], q["lo"], q["up"], q["x0"])
        where = (m, name, b, i)
        assert (rr, it) == (q["result"], q["iters"]) and np.array_equal(fr, q["free"]), (where, rr, it, q["result"], q["iters"])
        x = np.asarray(q["x"], float)
        sc = max(1.0, float(np.max(np.abs(xr))))
        worst = max(worst, float(np.max(np.abs(x - xr))) / sc)
        assert np.max(np.abs(x - xr)) < 1e-9 * sc, (where, x, xr)
        if m <= 4:
            xb = np.asarray(brute_force(q["H"], q["g"], q["lo"], q["up"]), float)
            worst_bf = max(worst_bf, float(np.max(np.abs(x - xb))) / sc)
            assert np.max(np.abs(x - xb)) < 1e-9 * sc, (where, x, xb)
    print("m = %d: oracle to long double %.3g, brute force to long double %.3g" % (m, worst, worst_bf))


@pytest.mark.parametrize("family,n,m", GROUPS)
def test_reference_matches_the_oracle_back_pass(family, n, m):
    """ref_back_pass against the C oracle's back_pass, every trajectory of every call: relerr < 1e-8 as in the other parity tests.
    The printed distances are the float64 noise floor the GPU's figures compare with."""
    from oracle import oracle_ctypes as oc
    f0, n0, _ = next(g for g in GROUPS if g[2] == m)
    worst = {}
    for name in call_names(m):
        c, ref = case(family, n, m, name), reference(family, n, m, name)
        first = reference(f0, n0, m, name)
        for b in range(c["B"]):
            for i, q in ref["qps"][b].items():                       # the group's QPs are the ones the per-m tests checked
                assert all(np.array_equal(q[key], first["qps"][b][i][key]) for key in ("H", "g", "lo", "up", "x0")), (name, b, i)
            d, (K, k, Quu), vx, vxx, dv = oc.back_pass(c["cx"][..., b], c["cu"][..., b], c["cxx"], c["cxu"], c["cuu"], c["fx"], c["fu"],
                                                      float(c["lam"][b]), c["regType"], c["lims"], None, c["u"][..., b])
            assert d == ref["diverge"][b] == 0, (name, b, d)
            for key, got in (("K", K), ("k", k), ("Quu", Quu), ("Vx", vx), ("Vxx", vxx), ("dV", dv)):
                e = relerr(got, ref[key][..., b])
                worst[key] = max(worst.get(key, 0.0), e)
                assert e < 1e-8, (name, b, key, e)
    print("%s (%d, %d) oracle to long double:" % (family, n, m), " ".join("%s %.3g" % kv for kv in sorted(worst.items())))
