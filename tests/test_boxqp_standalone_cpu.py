"""The table of tests/boxqp_standalone_cases.py certifies itself without a GPU: every problem that is expected to solve under the default
options has decisive comparisons, a certified minimiser and strict complementarity (the conditions of tests/test_boxqp_designed_cpu.py),
every item the issue lists is shown on the reference (patterns, free-set shapes and sizes, warm starts, box shapes, the factor reuse, the
option-driven exits, the lost pivots), and the long-double reference, the same statements in float64 and the C oracle take one path on
every problem — so tests/test_gpu_boxqp_standalone.py has nothing to excuse."""
import numpy as np
import pytest

from boxqp_designed_cases import kkt, ref_boxqp, required_events, OPTS
from boxqp_standalone_cases import (BATCH_MAX, M_BIG, M_SMALL, NFREE_TARGETS, OPTION_EXIT, OPTION_SETS, SMALL_COUNTS, _bits, _clamp, big_batches,
                                    small_batches, small_qps)

MARGIN, KKT, STRICT, MAX_ITERS = 1e-6, 1e-12, 1e-6, 50


def _conditions(m, p, worst):
    """margin, KKT residual, strict complementarity, cond(H) and the iteration count of a problem solved under the default options"""
    tr, w = p["trace"], (m, p["tag"])
    res, strict = kkt(p["H"], p["g"], p["lo"], p["up"], p["x"])
    cond = float(np.linalg.cond(p["H"]))
    assert p["result"] >= 4, (w, p["result"])
    assert tr["margin"] >= MARGIN, (w, tr["margin"], tr["where"])
    assert res <= KKT, (w, res)
    assert strict >= STRICT, (w, strict)
    assert cond <= (1e3 if m >= 255 else 1e4), (w, cond)
    assert p["iters"] <= MAX_ITERS, (w, p["iters"])
    worst.update(margin=min(worst.get("margin", np.inf), tr["margin"]), kkt=max(worst.get("kkt", 0.0), res),
                 strict=min(worst.get("strict", np.inf), strict), cond=max(worst.get("cond", 0.0), cond), iters=max(worst.get("iters", 0), p["iters"]))


def _same_path(m, p, worst):
    """float64 ref_boxqp and the C oracle against the long-double reference: result, iteration count, free set; x within 1e-9 scaled"""
    from oracle import oracle_ctypes as oc
    o = dict(OPTS, **(p["opts"] or {}))
    w = (m, p["tag"])
    x64, r64, f64, it64, _ = ref_boxqp(p["H"], p["g"], p["lo"], p["up"], p["x0"], dtype=np.float64, opts=o)
    xo, ro, Hfo, fo, ito = oc.boxqp(p["H"], p["g"], p["lo"], p["up"], p["x0"], opts=o if p["opts"] else None)
    assert (r64, it64) == (p["result"], p["iters"]) and np.array_equal(f64, p["free"]), (w, "float64", r64, it64, p["result"], p["iters"])
    assert (ro, ito) == (p["result"], p["iters"]) and np.array_equal(fo, p["free"]), (w, "oracle", ro, ito, p["result"], p["iters"])
    x = np.asarray(p["x"], float)
    sc = max(1.0, float(np.max(np.abs(x))))
    for name, got in (("float64", x64), ("oracle", xo)):
        d = float(np.max(np.abs(np.asarray(got, float) - x))) / sc
        worst[name] = max(worst.get(name, 0.0), d)
        assert d < 1e-9, (w, name, d)


# ------------------------------------------------------------------------------------------------------------------- small m
@pytest.mark.parametrize("m", M_SMALL)
def test_small_m_list(m):
    """the replayed QPs of an m: the conditions, the events the in-kernel table requires (m = 6 included, which only this list runs),
    one path in long double, float64 and the oracle, and batch sizes on both sides of a full wave"""
    qps = small_qps(m)
    worst, path, events = {}, {}, set()
    for p in qps:
        _conditions(m, p, worst)
        _same_path(m, p, path)
        events |= p["trace"]["events"]
    print("m = %d: %d QPs, least margin %.2g, largest KKT residual %.2g, least strict complementarity %.2g, largest cond %.3g, most "
          "iterations %d; float64 to long double %.3g, oracle %.3g" % (m, len(qps), worst["margin"], worst["kkt"], worst["strict"],
                                                                         worst["cond"], worst["iters"], path["float64"], path["oracle"]))
    assert not required_events(m) - events, sorted(required_events(m) - events)
    sizes = sorted(len(b) for b in small_batches(m).values())
    assert sizes[:4] == [1, 63, 64, 65] and sizes[4] == len(qps) > 65 and len(qps) % 64 != 0, sizes
    assert len(SMALL_COUNTS) == 5


# ------------------------------------------------------------------------------------------------------------------- large m
def _by_tag(batches):
    return {p["tag"]: p for ps in batches.values() for p in ps}


@pytest.mark.parametrize("m", M_BIG)
def test_large_m_table(m):
    B = big_batches(m)
    T = _by_tag(B)
    worst, codes = {}, set()
    for name, ps in B.items():
        assert 1 <= len(ps) <= BATCH_MAX(m), (m, name, len(ps))
        for p in ps:
            assert np.array_equal(p["H"], p["H"].T) or p["tag"] == "pivot_nan", (m, p["tag"], "H is not symmetric")
            codes.add(p["result"])
            if name.startswith("main"):
                _conditions(m, p, worst)
            elif name != "pivot":                                   # option-driven exits stop early by design: margin and exit code
                assert p["trace"]["margin"] >= MARGIN, (m, p["tag"], p["trace"]["margin"], p["trace"]["where"])
                worst["margin"] = min(worst["margin"], p["trace"]["margin"]) if "margin" in worst else p["trace"]["margin"]
    print("m = %d: %d problems in %d launches, least margin %.2g, largest KKT residual %.2g, least strict complementarity %.2g, largest "
          "cond %.3g, most iterations %d" % (m, len(T), len(B), worst["margin"], worst["kkt"], worst["strict"], worst["cond"], worst["iters"]))
    free = lambda tag: np.flatnonzero(T[tag]["free"])
    ev = lambda tag: T[tag]["trace"]["events"]
    # clamp patterns
    assert len(free("none")) == m and T["none"]["result"] in (4, 5)
    assert T["all_first_iteration"]["result"] == 6 and T["all_first_iteration"]["iters"] == 1 and {"warm_below", "warm_above"} <= ev("all_first_iteration")
    assert T["all_later"]["result"] == 6 and "exit6_later" in ev("all_later")
    assert free("all_but_last").tolist() == [m - 1] and free("all_but_first").tolist() == [0]
    assert free("only_last").tolist() == list(range(m - 1))
    # free-set shapes: a full segment and nothing else, a free set that ends at a segment's last lane, an empty segment between two others
    if m > 64:
        assert free("free_0_63").tolist() == list(range(64))
        last = free("ends_at_lane_63")[-1]
        assert last % 64 == 63 and last < m - 1 and len(free("ends_at_lane_63")) > 1
    if m >= 129:
        seg = set((free("clamped_segment") // 64).tolist())
        assert any(s not in seg and min(seg) < s < max(seg) for s in range((m + 63) // 64)), sorted(seg)
    # free-set sizes
    if m >= 257:
        for nf in NFREE_TARGETS:
            assert len(free("nfree%d" % nf)) == nf, (m, nf, len(free("nfree%d" % nf)))
    # warm starts, iterations and reuse, box shapes
    for tag in ("warm_below", "warm_above", "warm_on_bound_inward"):
        assert tag in ev(tag) and 0 < len(free(tag)) < m, (m, tag, sorted(ev(tag)))
    it = T["iter"]
    assert it["iters"] >= 4 and it["trace"]["changes"] >= 2 and "factor_reused" in ev("iter"), (m, it["iters"], it["trace"]["changes"])
    bs = T["box_shapes"]
    assert (bs["lo"] == bs["up"]).any() and np.isneginf(bs["lo"]).any() and np.isposinf(bs["up"]).any()
    # option-driven exits: each set reaches its code; the iteration cap also through the reference's `iter == maxIter` quirk (a solve that
    # ends in its last allowed iteration reports 1, one that runs out of iterations reports 0)
    for name, code in OPTION_EXIT.items():
        got = [p["result"] for p in B[name]]
        assert all(p["opts"] == OPTION_SETS[name] for p in B[name])
        assert code is None or code in got, (m, name, got)
    assert any(p["result"] == 0 for k in (1, 2, 3) for p in B["maxIter%d" % k])
    assert any("factor_reused_solve" in p["trace"]["events"] for p in B["reuse"]), m
    # lost pivots: result 0, the first iteration's free set, x = clamp(x0) untouched
    lost = set()
    for p in B["pivot"]:
        assert p["result"] == 0 and p["iters"] == 1 and np.array_equal(np.flatnonzero(p["free"]), p["first_free"]), (m, p["tag"])
        assert np.array_equal(_bits(np.asarray(p["x"], float)), _bits(_clamp(p["x0"], p["lo"], p["up"]))), (m, p["tag"])
        lost.add("nan" if p["lost"] is None else "first" if p["lost"] == 0 else "last" if p["lost"] == len(p["first_free"]) - 1 else p["lost"])
    assert {"nan", "first", "last"} <= lost and (m < 513 or any(isinstance(j, int) and j > 256 for j in lost)), (m, lost)
    assert codes == {0, 1, 2, 4, 5, 6}, (m, sorted(codes))


@pytest.mark.parametrize("m", M_BIG)
def test_large_m_three_paths_agree(m):
    worst = {}
    n = 0
    for ps in big_batches(m).values():
        for p in ps:
            _same_path(m, p, worst)
            n += 1
    print("m = %d: %d problems, float64 to long double %.3g, oracle to long double %.3g" % (m, n, worst["float64"], worst["oracle"]))
