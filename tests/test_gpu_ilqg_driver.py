"""The per-trajectory state machine of the iLQG driver (csrc/ilqg.hip: post_bp_kernel, accept_kernel, ls_more_kernel,
init_finish_kernel, the host loop and its hard cap) on the designed solves of tests/ilqg_driver_cases.py, against the CPU oracle's
restatement of src/iLQG.jl:205-331.  tests/test_ilqg_driver_cases_cpu.py shows from the oracle alone that the cases reach every
branch and that every decision they take is at least 1e-4 away from its threshold; so the decisions themselves (status, counters,
λ, dλ, the accepted step size of every iteration) are compared exactly here, the values they were taken on at 1e-7."""
import numpy as np
import pytest

from conftest import relerr

import ilqg_driver_cases as dc

pytestmark = pytest.mark.gpu
TRACE_KEYS = ("λ", "dλ", "α", "improvement", "cost", "reduce_ratio", "grad_norm")


@pytest.fixture(scope="module")
def ddp():
    import ddp_amd
    ddp_amd.default_handle()
    return ddp_amd


def _solve(ddp, case, sel=None, **extra):
    x0, u0 = dc.starts(case)
    if sel is not None:
        x0, u0 = x0[:, sel], u0[:, :, sel]
    return ddp.iLQG(dc.gpu_problem(ddp, case), x0, u0, **dc.gpu_kwargs(case), **extra)


def _arrays(r):
    """every array a solve returns: x, u, K, k, Quu, Vx, Vxx, cost"""
    return (r[0], r[1], r[2].K, r[2].k, r[2].Σi, r[3], r[4], r[5])


def _same(a, b):
    return np.array_equal(a, b, equal_nan=True)


@pytest.mark.parametrize("name", dc.ORACLE_CASES)
def test_case_matches_the_oracle(ddp, name):
    case = dc.BY_NAME[name]
    ref = dc.oracle_results(name)
    x, u, pol, Vx, Vxx, cost, tr = _solve(ddp, case)
    st, hist = tr["stats"], tr["history"]
    for b, r in enumerate(ref):
        info, h, tl = r["info"], r["history"], r["info"]["trace_len"]
        got = tuple(int(v) for v in st[:5, b])
        want = (info["status"], info["iter"], info["accepted_iter"], info["n_backpass"], info["n_forward"])
        print(name, b, "status, iter, accepted_iter, n_backpass, n_forward:", got, "oracle", want, "λ", st[5, b], info["lam"])
        assert got == want, (name, b)
        assert st[5, b] == info["lam"], (name, b)
        # ---- trace rows: the decisions exactly (λ, dλ: products of the same doubles in the same order; α: the step size or NaN) ...
        assert tl == info["iter"] - 1
        for key in ("λ", "dλ", "α"):
            assert _same(hist[key][:tl, b], h[key]), (name, b, key, hist[key][:tl, b], h[key])
        # ... the values at 1e-7, the ones that are exact by construction (z from sign(): -1, 0; Δcost = 0) with ==
        for key in ("improvement", "cost", "reduce_ratio", "grad_norm"):
            g_, r_ = hist[key][:tl, b], h[key]
            exact = np.isnan(r_) | (r_ == 0.0) | (r_ == -1.0)
            assert _same(g_[exact], r_[exact]), (name, b, key, g_, r_)
            scale = max(1e-300, np.max(np.abs(r_[~exact]))) if (~exact).any() else 1.0
            assert np.all(np.abs(g_[~exact] - r_[~exact]) <= 1e-7 * scale + 1e-12), (name, b, key, g_, r_)
        for key in TRACE_KEYS:                                      # no row behind the last iteration
            assert not np.nan_to_num(hist[key][tl:, b], nan=1.0).any(), (name, b, key)
        # ---- arrays
        mine = dict(x=x[..., b], u=u[..., b], K=pol.K[..., b], k=pol.k[..., b], Vx=Vx[..., b], Vxx=Vxx[..., b])
        if info["status"] == -1:                                   # iLQG.jl:205-210: nothing to return
            assert not any(np.any(v) for v in mine.values()) and not cost[:, b].any()
            continue
        keys = ("x", "u", "K", "k", "Vx", "Vxx")
        if info["status"] == 3 and info["n_forward"] == dc.forwards_in_rows(case, dc.accepted_index(case, h["α"])):
            keys = ("x", "u")                                       # the last back pass diverged: gains and value function are partial
        for key in keys:
            e = relerr(mine[key], r[key])
            assert e < 1e-7, (name, b, key, e)
        assert abs(cost[:, b].sum() - r["cost"].sum()) <= 1e-8 * abs(r["cost"].sum()), (name, b)
        assert abs(st[7, b] - r["cost"].sum()) <= 1e-8 * abs(r["cost"].sum()), (name, b)


def test_unbatched_initial_divergence_returns_none(ddp):
    """huge_alpha_only through the unbatched API (iLQG.jl:205-210 returns nothing)"""
    case = dc.BY_NAME["huge_alpha_only"]
    x0, u0 = dc.starts(case)
    assert ddp.iLQG(dc.gpu_problem(ddp, case), x0[:, 0], u0[..., 0], **dc.gpu_kwargs(case)) is None


def test_cap_ends_a_solve_the_reference_would_never_end(ddp):
    """λfactor = 1 and a back pass that never succeeds: λ never grows, iLQG.jl:244-251 loops for ever.  The driver's own bound
    (include/ddp_amd.h, DDP_EXIT_CAP): exactly 4 max_iter + 1000 batch iterations, one back pass each, nothing else moves."""
    case = dc.BY_NAME["cap"]
    x0, u0 = dc.starts(case)
    cap = 4 * dc.opt(case, "max_iter") + 1000
    for timing in (True, False):                                    # the host polls every iteration | every fourth
        x, u, pol, Vx, Vxx, cost, tr = _solve(ddp, case, timing=timing)
        st = tr["stats"]
        assert tr["global_iters"] == cap
        for b in range(x0.shape[1]):
            assert tuple(int(v) for v in st[:5, b]) == (5, 1, 1, cap, 0), (b, st[:, b])       # status, iter, accepted_iter, n_backpass, n_forward
            assert st[5, b] == dc.opt(case, "lam")                  # λ · dλ = 1 · 1; dλ = max(dλ · 1, 1) = 1
            for key in TRACE_KEYS:                                  # no iteration ever completed: no trace row
                assert not np.nan_to_num(tr["history"][key][:, b], nan=1.0).any()
        assert np.array_equal(x[:, 0, :], x0) and np.isfinite(x).all()      # the initial rollout is what is left


@pytest.mark.parametrize("name", dc.GROUP_CASES + dc.SCHEDULING_EXTRA)
def test_scheduling_changes_nothing_where_candidates_are_rejected(ddp, monkeypatch, name):
    """The grouped line search ([0,1) [1,3) [3,nα), masks from ls_more_kernel) and the compaction of the working set are scheduling
    only: with acceptance placed at every group boundary (and nowhere), all four runs are bit-identical — summary rows 0-4, every
    array, every trace key."""
    case = dc.BY_NAME[name]
    runs = {}
    for groups in ("0", "1"):
        for compact in ("0", "4"):
            monkeypatch.setenv("DDP_ILQG_LSGROUPS", groups); monkeypatch.setenv("DDP_ILQG_COMPACT", compact)
            runs[groups, compact] = _solve(ddp, case)
    ref = runs["0", "0"]
    if name in dc.SCHEDULING_EXTRA or not name.endswith("none"):
        its = np.sort(ref[6]["stats"][1])
        assert its[len(its) // 2 - 1] < its[-1], its                # half of the batch ends before the rest: a compacted set forms
    for key, r in runs.items():
        assert r[6]["global_iters"] == ref[6]["global_iters"], key
        assert np.array_equal(r[6]["stats"][:5], ref[6]["stats"][:5]), (key, r[6]["stats"][:5], ref[6]["stats"][:5])
        for a, b_ in zip(_arrays(r), _arrays(ref)):
            assert _same(a, b_), key
        for k_ in TRACE_KEYS:
            assert _same(r[6]["history"][k_], ref[6]["history"][k_]), (key, k_)
    # and the plain run is the oracle's: status, iter, accepted_iter, n_backpass, n_forward
    for b, r in enumerate(dc.oracle_results(name)):
        i = r["info"]
        assert tuple(int(v) for v in ref[6]["stats"][:5, b]) == (i["status"], i["iter"], i["accepted_iter"], i["n_backpass"], i["n_forward"])


@pytest.mark.parametrize("name", dc.OTHER_DRIVER_CASES)
def test_queue_fills_its_options_like_the_standalone_driver(ddp, name):
    """iLQG_queue with fewer slots than problems: the scheduler fills an option struct of its own; every problem comes out with the
    bits of the stand-alone solve at the batch size of the slots"""
    case = dc.BY_NAME[name]
    x0, u0 = dc.starts(case)
    S = 2
    q = ddp.iLQG_queue(dc.gpu_problem(ddp, case), x0, u0, slots=S, **dc.gpu_kwargs(case))
    for c in range(0, x0.shape[1], S):
        sel = list(range(c, c + S))
        r = _solve(ddp, case, sel=sel, timing=False)
        assert _same(q[6]["stats"][:, sel], r[6]["stats"]), (name, sel, q[6]["stats"][:, sel], r[6]["stats"])
        for a, b_ in zip(_arrays(q), _arrays(r)):
            assert _same(a[..., sel], b_), (name, sel)
    for b, r in enumerate(dc.oracle_results(name)):
        i = r["info"]
        assert tuple(int(v) for v in q[6]["stats"][:5, b]) == (i["status"], i["iter"], i["accepted_iter"], i["n_backpass"], i["n_forward"])
        assert q[6]["stats"][5, b] == i["lam"]


@pytest.mark.parametrize("name", dc.OTHER_DRIVER_CASES)
def test_mpc_of_one_step_is_the_standalone_solve(ddp, name):
    """iLQG_mpc with one closed-loop step: summary, plan and the applied control of the stand-alone solve, bit for bit"""
    case = dc.BY_NAME[name]
    x0, u0 = dc.starts(case)
    xcl, ucl, scl, xp, up, git = ddp.iLQG_mpc(dc.gpu_problem(ddp, case), x0, u0, 1, **dc.gpu_kwargs(case))
    r = _solve(ddp, case, timing=False)
    assert _same(scl[:, 0, :], r[6]["stats"]), (name, scl[:, 0, :], r[6]["stats"])
    assert _same(xp, r[0]) and _same(up, r[1])
    assert _same(xcl[:, 0, :], r[0][:, 0, :]) and _same(xcl[:, 1, :], r[0][:, 1, :]) and _same(ucl[:, 0, :], r[1][:, 0, :])
    assert np.array_equal(xcl[:, 0, :], x0)


@pytest.fixture(scope="module")
def lq_user(ddp):
    return ddp.DeviceProblem(ddp.example_source("lq"), 10, 2, nparam=224)


@pytest.mark.parametrize("name", dc.USER_PROBLEM_CASES)
def test_user_problem_driver_takes_the_same_decisions(ddp, lq_user, name):
    """the bundled `lq` example as a DeviceProblem with the matrices of the built-in family: the same state machine through
    ddp_ilqg_family_dev — counters, λ, dλ and the step size of every iteration exactly, arrays and trace values at the 1e-8 that
    tests/test_gpu_user_problem.py uses for this pairing"""
    case = dc.BY_NAME[name]
    M = dc.lq_matrices(case["R"])
    prm = np.concatenate([M[k].ravel(order="F") for k in ("A", "B", "Q", "R")])
    x0, u0 = dc.starts(case)
    rb = _solve(ddp, case, timing=False)
    ru = ddp.iLQG(lq_user, x0, u0, params=prm, timing=False, **dc.gpu_kwargs(case))
    assert np.array_equal(ru[6]["stats"][:6], rb[6]["stats"][:6]), (ru[6]["stats"][:6], rb[6]["stats"][:6])
    for key in ("λ", "dλ", "α"):
        assert _same(ru[6]["history"][key], rb[6]["history"][key]), key
    hu, hb = ru[6]["history"], rb[6]["history"]
    for key in ("improvement", "cost", "grad_norm"):
        assert relerr(np.nan_to_num(hu[key]), np.nan_to_num(hb[key]), 0) < 1e-8, key
    # z = Δcost / expected, Δcost the difference of two sums of N costs that the two families add up in their own order: each sum
    # is good to N eps times itself, so next to the 1e-8 of the other keys z may move by 2 N eps (c_before + c_after) / expected
    N = u0.shape[1]
    for b in range(x0.shape[1]):
        tl = int(rb[6]["stats"][1, b]) - 1
        zu, zb, imp, c = hu["reduce_ratio"][:tl, b], hb["reduce_ratio"][:tl, b], hb["improvement"][:tl, b], hb["cost"][:tl, b]
        ok = np.isfinite(zb) & (zb != 0) & (imp != 0)
        assert _same(zu[~ok], zb[~ok])
        expected = np.abs(imp[ok] / zb[ok])
        bound = 1e-8 * np.abs(zb[ok]) + 2 * N * np.finfo(float).eps * (2 * np.abs(c[ok]) + np.abs(imp[ok])) / expected
        assert np.all(np.abs(zu[ok] - zb[ok]) <= bound), (name, b, zu, zb, bound)
    for a, b_ in zip(_arrays(ru), _arrays(rb)):
        assert relerr(a, b_, -2) < 1e-8                            # [..., N, B]: the time axis is the one before the trajectory's
