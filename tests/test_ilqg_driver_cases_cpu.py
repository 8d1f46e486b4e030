"""The designed solves of tests/ilqg_driver_cases.py prove themselves on the CPU oracle alone: every branch a case claims to reach
is reached (status, iter, rollouts per iteration, NaN in α, z == -1 rows, λ rows at λmin ...), the cases together reach the whole
tag list, and every decision a solve takes is at least MARGIN away from its threshold — 1000 times the 1e-7 allowed between the
device and the oracle on trace values (tests/test_gpu_edge_cases.py, test_ilqg_trace_history_matches_oracle) — so that the
device test (tests/test_gpu_ilqg_driver.py) may compare the decisions themselves exactly."""
import numpy as np
import pytest

import ilqg_driver_cases as dc

MARGIN = 1e-4


@pytest.mark.parametrize("name", dc.ORACLE_CASES)
def test_case_reaches_its_branches_with_a_margin(name):
    case = dc.BY_NAME[name]
    res = dc.oracle_results(name)
    seen = dc.observed_tags(case, res)
    assert case["tags"] <= seen, (name, sorted(case["tags"] - seen))
    m, exact = dc.margins(case, res)
    for key, vals in m.items():
        print("%-28s %-14s smallest margin %.3e over %d decisions" % (name, key, min(vals) if vals else np.inf, len(vals)))
        assert all(v >= MARGIN for v in vals), (name, key, min(vals))
    # a decision that is a division of two rounding residues has no margin whatever its value: where z = Δcost / expected decided,
    # both are far above the rounding of the cost sums they come from (1e-16 relative)
    for r in res:
        if r["info"]["status"] == 2:
            _, dcost, expected, z = dc.exit_decision(case, r)
            scale = max(abs(r["cost0"]), 1e-300)
            assert expected <= 0 or (abs(expected) > 1e-11 * scale and abs(dcost) > 1e-11 * scale), (name, dcost, expected)


def test_designed_expectations_of_single_cases():
    """what the issue's table states about single cases, from the oracle"""
    def infos(name):
        return [r["info"] for r in dc.oracle_results(name)], [r["history"] for r in dc.oracle_results(name)]
    for name in ("grad_exit", "zero_start_lambda_small"):
        for i in infos(name)[0]:
            assert (i["status"], i["iter"], i["trace_len"], i["n_forward"]) == (1, 1, 0, 0)
    inf, hist = infos("zero_start")
    for i, h in zip(inf, hist):
        assert i["status"] == 3 and np.isnan(h["α"]).all() and not h["reduce_ratio"].any() and not h["improvement"].any()
        assert list(h["λ"][:3]) == [1.0, 1.0 * 1.6, 1.0 * 1.6 * (1.6 * 1.6)]          # λ·dλ with the OLD dλ, dλ·f (:313)
    for i in infos("cost_exit_first")[0] + infos("cost_exit_first_pendcart")[0]:
        assert (i["status"], i["iter"]) == (2, 1)
    assert all((i["status"], i["iter"], i["n_backpass"]) == (4, 1, 0) for i in infos("maxiter_0")[0])
    assert all((i["status"], i["iter"]) == (4, 2) for i in infos("maxiter_1")[0])
    for i in infos("newton_overshoot")[0]:
        searches = i["trace_len"] + (i["status"] == 2)                              # (a gradient exit comes before the search)
        assert i["n_forward"] == 3 * searches and i["status"] in (1, 2)            # two overshoots rejected, α = 1 accepted, every time
    for r in dc.oracle_results("newton_overshoot_rr_neg"):
        assert (r["info"]["status"], r["info"]["iter"], r["info"]["n_forward"]) == (2, 1, 1) and r["cost"].sum() > r["cost0"]
    for i, h in zip(*infos("only_overshoot")):
        assert h["reduce_ratio"][0] == -1.0 and np.isnan(h["α"][0]) and i["accepted_iter"] > 5 and i["iter"] > 2 * i["accepted_iter"]
    for i, h in zip(*infos("rr_above_one")):
        assert i["status"] == 3 and i["accepted_iter"] == 1 and np.all(np.abs(h["reduce_ratio"] - 1) < 0.01)
    for i, h in zip(*infos("rr_half")):
        assert np.all(h["α"] == 1.9) and i["n_forward"] == 2 * 6
    for i, h in zip(*infos("huge_alpha_first")):
        assert np.all(h["α"] == 1.0) and i["n_forward"] == 2 * 3
    assert all(i["status"] == -1 for i in infos("huge_alpha_only")[0])
    for name in ("lambda_schedule", "lambda_schedule_pendcart"):
        for h in infos(name)[1]:
            assert list(h["dλ"][:3]) == [1.0 / 3.0, 1.0 / 3.0 / 3.0, 1.0 / 3.0 / 3.0 / 3.0]
            assert list(h["λ"][:3]) == [7.0 * (1.0 / 3.0), 7.0 * (1.0 / 3.0) * (1.0 / 3.0 / 3.0), 1e-2]
    for i in infos("bp_diverge_then_recover")[0]:
        assert i["n_backpass"] >= i["iter"] + 2
    for i in infos("bp_diverge_lambda_exit")[0]:
        assert (i["status"], i["iter"], i["n_forward"]) == (3, 1, 0)


def test_group_boundary_cases_accept_where_designed():
    """every list of the group_boundaries family accepts at its designed index (or nowhere) in every iteration and trajectory"""
    for name in dc.GROUP_CASES:
        case = dc.BY_NAME[name]
        want = -1 if name.endswith("none") else int(name.rsplit("at", 1)[1])
        na = len(dc.alphas(case))
        for r in dc.oracle_results(name):
            idx = dc.accepted_index(case, r["history"]["α"])
            assert len(idx) >= 1 and np.all(idx == want), (name, idx)
            per_iter = na if want < 0 else want + 1
            searches = r["info"]["trace_len"] + (r["info"]["status"] in (2, 3))     # (a gradient exit comes before the search)
            assert r["info"]["n_forward"] == per_iter * searches, name
    for na, need in ((2, {0, 1, -1}), (3, {0, 1, 2, -1}), (4, {0, 1, 2, 3, -1}), (16, {0, 1, 2, 3, 15, -1})):
        got = set()
        for name in dc.GROUP_CASES:
            if len(dc.alphas(dc.BY_NAME[name])) == na:
                for r in dc.oracle_results(name):
                    got |= set(dc.accepted_index(dc.BY_NAME[name], r["history"]["α"]))
        assert got == need, (na, got)


def test_the_cases_cover_the_whole_tag_list_and_none_is_left_out():
    """the tag list itself is asserted: a dropped case (or tag) fails here.  No case is skipped or expected to fail."""
    assert len(dc.TAGS) == len(set(dc.TAGS)) == 38
    union = set()
    for c in dc.CASES:
        assert c["tags"] and c["tags"] <= set(dc.TAGS), c["name"]
        union |= c["tags"]
    assert union == set(dc.TAGS), sorted(set(dc.TAGS) - union)
    # ... and from the oracle alone (the cap case has no oracle: its expectation is the header's contract)
    seen = {"exit_cap"}
    for name in dc.ORACLE_CASES:
        seen |= dc.observed_tags(dc.BY_NAME[name], dc.oracle_results(name)) & dc.BY_NAME[name]["tags"]
    assert seen == set(dc.TAGS)
    assert [c["name"] for c in dc.CASES if not c["oracle"]] == ["cap"]
    assert len(dc.ORACLE_CASES) == len(dc.CASES) - 1 == 23 + 18
    for names in (dc.SCHEDULING_EXTRA, dc.OTHER_DRIVER_CASES, dc.USER_PROBLEM_CASES):
        assert set(names) <= set(dc.ORACLE_CASES)


def test_scheduling_cases_end_at_different_iterations():
    """the driver compacts its working set once half of the slots have stopped: the cases of the scheduling test on the device (but
    the lists that never accept, whose solves all end together) have at least half of the batch ending before the last solve"""
    for name in dc.SCHEDULING_EXTRA + [n for n in dc.GROUP_CASES if not n.endswith("none")]:
        its = sorted(r["info"]["iter"] for r in dc.oracle_results(name))
        assert its[len(its) // 2 - 1] < its[-1], (name, its)
