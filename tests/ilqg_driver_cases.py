"""Designed solves for the per-trajectory state machine of the iLQG driver (csrc/ilqg.hip: post_bp_kernel, accept_kernel,
ls_more_kernel, init_finish_kernel and the host loop), which follows src/iLQG.jl:205-331 statement by statement.

Plain data plus builders; nothing here touches the GPU.  One case is ONE iLQG call (options are per call) on a small batch of
perturbed starts: a problem family, x0, u0, lims, the option set and the TAGS the case is designed to hit.  A tag names a branch
of the state machine; `observed_tags` derives the tags from the CPU oracle's result of the case, and
tests/test_ilqg_driver_cases_cpu.py asserts that every claimed tag is observed and that the union over the cases is the whole
list TAGS.  tests/test_gpu_ilqg_driver.py runs the same cases on the device.

Shapes: LQ n=10, m=2, N=40 (np_restatement.make_lq_problem(default_rng(4), T=40)); pendcart n=4, m=1, N=60, lims [-5,5],
regType 2 — the smallest at which the project's real kernels are picked."""
import functools

import numpy as np

# every branch the set of cases has to reach (the CPU test asserts that the union of the cases' tags equals this tuple)
TAGS = (
    "exit_grad",                    # status 1 (post_bp_kernel: g_norm < tol_grad && λ < 1e-5)
    "exit_grad_first_iter",         # ... at iter 1, no trace row
    "grad_small_lambda_large",      # g_norm < tol_grad in a trace row: the exit was blocked by λ >= 1e-5, the solve went on
    "exit_cost",                    # status 2 (accept_kernel: Δcost < tol_fun)
    "exit_cost_first_iter",         # ... at iter 1
    "exit_lambda_backpass",         # status 3 out of post_bp_kernel (the last iteration rolled nothing out)
    "exit_lambda_search",           # status 3 out of the "no step" branch of accept_kernel (after a failed line search)
    "exit_maxiter",                 # status 4
    "maxiter_zero",                 # max_iter = 0: status 4 before the first iteration (iter 1, no back pass)
    "maxiter_one",                  # max_iter = 1: status 4 with iter 2
    "exit_init_diverged",           # status -1 (init_finish_kernel)
    "exit_cap",                     # status 5: the driver's own bound (not a state of the reference; no oracle for it)
    "alpha_nan_rows",               # NaN in the α column: iterations without a step
    "z_zero_rows",                  # expected == 0 and Δcost == 0: z = sign(0) = 0, not > 0
    "z_minus_one_rows",             # expected <= 0 and Δcost < 0: z = -1 exactly, the whole search fails
    "overshoot_rejected_then_accepted",   # step sizes > 2 in front of the accepted one are rejected with z = -1 (no limits)
    "cost_raise_accepted",          # reduce_ratio_min < 0: a candidate that raises the cost is accepted
    "rr_mid_accepted",              # accepted with 0.2 < z < 0.8 (neither sign() nor the Newton value 1)
    "search_failed_z_near_one",     # reduce_ratio_min = 1.5: z ≈ 1 is rejected for every step size
    "second_alpha_every_time",      # every accepted step is the second of the list
    "nonfinite_candidate_rejected", # the first candidate's cost is not finite
    "lambda_at_min_rows",           # λ clamped at λmin
    "dlambda_inverse_factor",       # dλ = min(dλ/f, 1/f) picks 1/f
    "dlambda_quotient",             # ... picks dλ/f
    "single_alpha",                 # nα = 1: no grouped search by construction
    "accept_idx_0", "accept_idx_1", "accept_idx_2", "accept_idx_3", "accept_idx_last", "accept_none",
    "n_alpha_2", "n_alpha_3", "n_alpha_4", "n_alpha_16",
    "backpass_retry_then_search",   # the back pass diverges, λ grows, it succeeds and a normal search follows (`continue`, :244-251)
    "lims", "pendcart",             # the rollout / cost / box-QP kernels of these are different ones
)

LQ_SHAPE = dict(n=10, m=2, N=40)
PEND_SHAPE = dict(n=4, m=1, N=60)
LQ_LIMS = np.array([[-0.5, 0.5], [-0.3, 0.4]])
PEND_LIMS = np.array([[-5.0, 5.0]])
X0_SCALE = (1.0, 0.5, 2.0, 1.0)          # per-trajectory scale of the LQ start: the solves of a batch end at different iterations

# oracle keyword -> keyword of ddp.iLQG
GREEK = dict(alpha="α", lam="λ", dlam="dλ", lam_factor="λfactor", lam_max="λmax", lam_min="λmin")


def _case(name, tags, family="lq", R="default", lims=False, start="perturbed", group=False, oracle=True, **opts):
    return dict(name=name, tags=frozenset(tags), family=family, R=R, lims=lims, start=start, group=group, oracle=oracle, opts=opts)


def _over(j):
    """j distinct step sizes > 2 (the Newton step overshoots: expected < 0 and Δcost < 0)"""
    return [4.0 - 0.1 * i for i in range(j)]


def _gb_list(na, idx):
    """nα step sizes whose first acceptable one sits at `idx` (None: all overshoot)"""
    if idx is None:
        return _over(na)
    return _over(idx) + [1.0] + [0.5 ** (t + 1) for t in range(na - idx - 1)]


NEWTON = dict(lam=1e-6, lam_min=1e-8)     # λ ≈ 0: the LQ step is the Newton step, expected > 0 exactly for α < 2


def _cases():
    c = [
        _case("grad_exit", {"exit_grad", "exit_grad_first_iter"}, tol_grad=1e3, **NEWTON),
        _case("grad_small_but_lambda_large", {"grad_small_lambda_large", "exit_maxiter", "accept_idx_0"}, tol_grad=1e3, lam=1.0, max_iter=3),
        _case("zero_start", {"z_zero_rows", "alpha_nan_rows", "exit_lambda_search", "accept_none"}, start="zero", lam=1.0, lam_max=1e4),
        _case("zero_start_lambda_small", {"exit_grad", "exit_grad_first_iter"}, start="zero", lam=1e-6),
        _case("cost_exit_first", {"exit_cost", "exit_cost_first_iter"}, tol_fun=1e9),
        _case("maxiter_0", {"exit_maxiter", "maxiter_zero"}, tol_fun=-1.0, tol_grad=0.0, max_iter=0),
        _case("maxiter_1", {"exit_maxiter", "maxiter_one"}, tol_fun=-1.0, tol_grad=0.0, max_iter=1),
        _case("newton_overshoot", {"overshoot_rejected_then_accepted", "accept_idx_2", "exit_cost", "n_alpha_4"},
              alpha=[4.0, 2.5, 1.0, 0.3], **NEWTON),
        _case("newton_overshoot_rr_neg", {"cost_raise_accepted", "exit_cost", "exit_cost_first_iter"},
              alpha=[4.0, 2.5, 1.0, 0.3], reduce_ratio_min=-2.0, **NEWTON),
        _case("only_overshoot", {"z_minus_one_rows", "alpha_nan_rows", "rr_mid_accepted", "accept_none", "accept_idx_last", "n_alpha_2"},
              alpha=[4.0, 2.5], lam_max=1e2, **NEWTON),
        _case("rr_above_one", {"search_failed_z_near_one", "alpha_nan_rows", "exit_lambda_search", "accept_none"},
              reduce_ratio_min=1.5, lam_max=1e3),
        _case("rr_half", {"second_alpha_every_time", "accept_idx_1", "exit_maxiter", "lambda_at_min_rows", "n_alpha_4"},
              alpha=[3.0, 1.9, 1.2, 0.5], reduce_ratio_min=0.5, max_iter=6, **NEWTON),
        _case("huge_alpha_first", {"nonfinite_candidate_rejected", "accept_idx_1", "exit_maxiter", "n_alpha_3"},
              alpha=[1e160, 1.0, 0.1], max_iter=3),
        _case("huge_alpha_only", {"exit_init_diverged", "n_alpha_2"}, alpha=[1e160, 1e200]),
        _case("lambda_schedule", {"lambda_at_min_rows", "dlambda_inverse_factor", "dlambda_quotient", "exit_maxiter"},
              lam=7.0, dlam=5.0, lam_factor=3.0, lam_min=1e-2, tol_fun=-1.0, tol_grad=0.0, max_iter=6),
        _case("single_alpha", {"single_alpha", "exit_cost", "accept_idx_0"}, alpha=[0.5]),
        _case("bp_diverge_then_recover", {"backpass_retry_then_search", "exit_maxiter"}, R="indef", lam=1e-2, max_iter=3),
        _case("bp_diverge_lambda_exit", {"exit_lambda_backpass"}, R="negdef", lam_max=1e2),
        # limits and the pendulum: other rollout, cost and backward kernels under the same state machine
        _case("newton_overshoot_lims", {"lims", "accept_idx_0", "accept_idx_1", "accept_idx_2", "rr_mid_accepted", "exit_grad"},
              lims=True, alpha=[4.0, 2.5, 1.0, 0.3], **NEWTON),
        _case("rr_half_lims", {"lims", "accept_idx_0", "accept_idx_1", "exit_maxiter", "lambda_at_min_rows"},
              lims=True, alpha=[3.0, 1.9, 1.2, 0.5], reduce_ratio_min=0.5, max_iter=6, **NEWTON),
        _case("lambda_schedule_pendcart", {"pendcart", "lims", "lambda_at_min_rows", "dlambda_inverse_factor", "dlambda_quotient", "exit_maxiter"},
              family="pendcart", lims=True, regType=2, lam=7.0, dlam=5.0, lam_factor=3.0, lam_min=1e-2, tol_fun=-1.0, tol_grad=0.0, max_iter=6),
        _case("rr_above_one_pendcart", {"pendcart", "lims", "alpha_nan_rows", "exit_lambda_search"},
              family="pendcart", lims=True, regType=2, reduce_ratio_min=1.5, lam_max=1e3),
        _case("cost_exit_first_pendcart", {"pendcart", "lims", "exit_cost", "exit_cost_first_iter"},
              family="pendcart", lims=True, regType=2, tol_fun=1e9),
        # λ never grows (λfactor = 1) and the back pass never succeeds: the reference would loop for ever; the driver stops after
        # 4 max_iter + 1000 batch iterations (include/ddp_amd.h, DDP_EXIT_CAP).  No oracle for this one.
        _case("cap", {"exit_cap"}, R="negdef", oracle=False, lam_factor=1.0, max_iter=1),
    ]
    # the grouped line search rolls the step sizes out as [0,1) [1,3) [3,nα): acceptance at every group boundary, for every nα
    for na in (2, 3, 4, 16):
        for idx in sorted({0, 1, 2, 3, na - 1} & set(range(na))) + [None]:
            tags = {"n_alpha_%d" % na}
            if idx is None:
                tags |= {"accept_none", "z_minus_one_rows", "alpha_nan_rows", "exit_lambda_search"}
                extra = dict(lam_max=1e-4)           # λ = 1e-6, 1.6e-6, 4.1e-6, 1.7e-5, 1.1e-4: four rows without a step, then status 3
            else:
                tags |= {"accept_idx_%d" % idx} if idx < 4 else set()
                tags |= {"accept_idx_last"} if idx == na - 1 else set()
                tags |= {"overshoot_rejected_then_accepted"} if idx > 0 else set()
                extra = {}
            c.append(_case("group_boundaries_n%d_%s" % (na, "none" if idx is None else "at%d" % idx), tags, group=True,
                           alpha=_gb_list(na, idx), **NEWTON, **extra))
    return c


CASES = _cases()
BY_NAME = {c["name"]: c for c in CASES}
assert len(BY_NAME) == len(CASES)
ORACLE_CASES = [c["name"] for c in CASES if c["oracle"]]
GROUP_CASES = [c["name"] for c in CASES if c["group"]]
# three more that reject candidates, with solves of unequal length (the compacted working set really forms)
SCHEDULING_EXTRA = ["only_overshoot", "newton_overshoot_lims", "rr_above_one_pendcart"]
OTHER_DRIVER_CASES = ["lambda_schedule", "newton_overshoot", "rr_half", "zero_start", "huge_alpha_first", "maxiter_0"]
USER_PROBLEM_CASES = ["lambda_schedule", "newton_overshoot", "zero_start"]


# ------------------------------------------------------------------------------------------------------------------ builders
@functools.lru_cache(maxsize=None)
def lq_matrices(R="default"):
    from oracle import np_restatement as npr
    P = npr.make_lq_problem(np.random.default_rng(4), T=LQ_SHAPE["N"])
    Rm = {"default": P["R"], "negdef": -1e3 * np.eye(2), "indef": np.diag([1e-3, -0.3])}[R]
    return dict(A=P["A"], B=P["B"], Q=P["Q"], R=Rm, u0=P["u0"])


PEND = dict(g=9.82, l=0.35, h=0.01, d=0.99, goal=np.array([np.pi, 0.0, 0.0, 0.0]), Q=np.diag([10.0, 1.0, 2.0, 1.0]), R=1.0)


def starts(case):
    """x0[n,B], u0[m,N,B] of a case (B = 4)"""
    B = len(X0_SCALE)
    if case["family"] == "pendcart":
        rng = np.random.default_rng(20)
        x0 = np.array([np.pi - 0.6, 0.0, 0.0, 0.0])[:, None] + 0.05 * rng.standard_normal((4, B))
        return x0, 0.3 * rng.standard_normal((1, PEND_SHAPE["N"], B))
    if case["start"] == "zero":
        return np.zeros((10, B)), np.zeros((2, LQ_SHAPE["N"], B))
    rng = np.random.default_rng(11)
    x0 = (np.ones((10, B)) + 0.1 * rng.standard_normal((10, B))) * np.array(X0_SCALE)
    u0 = lq_matrices()["u0"][:, :, None] + 0.02 * rng.standard_normal((2, LQ_SHAPE["N"], B))
    return x0, u0


def lims(case):
    if not case["lims"]:
        return None
    return PEND_LIMS if case["family"] == "pendcart" else LQ_LIMS


def alphas(case):
    return np.asarray(case["opts"].get("alpha", 10.0 ** np.linspace(0, -3, 11)), dtype=float)


def opt(case, key):
    """an option of the case, or the reference's default (iLQG.jl:143-163)"""
    default = dict(lam=1.0, dlam=1.0, lam_factor=1.6, lam_max=1e10, lam_min=1e-6, tol_fun=1e-7, tol_grad=1e-4, max_iter=500, regType=1,
                   reduce_ratio_min=0.0)
    return case["opts"].get(key, default[key])


def oracle_problem(case):
    from oracle import oracle_ctypes as oc
    if case["family"] == "pendcart":
        return oc.make_problem("pendcart", 4, 1, PEND_SHAPE["N"], Q=PEND["Q"], R=np.array([[PEND["R"]]]),
                               pend=dict(g=PEND["g"], l=PEND["l"], h=PEND["h"], d=PEND["d"], goal=PEND["goal"]))
    M = lq_matrices(case["R"])
    return oc.make_problem("lq", 10, 2, LQ_SHAPE["N"], A=M["A"], B=M["B"], Q=M["Q"], R=M["R"])


def gpu_problem(ddp, case):
    if case["family"] == "pendcart":
        return ddp.PendcartProblem()
    M = lq_matrices(case["R"])
    return ddp.LQProblem(M["A"], M["B"], M["Q"], M["R"])


def gpu_kwargs(case):
    kw = {GREEK.get(k, k): v for k, v in case["opts"].items()}
    if case["lims"]:
        kw["lims"] = lims(case)
    return kw


def initial_cost(case, p, x0, u0):
    """sum of the cost of the initial rollout (iLQG.jl:181-192: the first α whose open-loop rollout of α·u0 stays bounded)"""
    from oracle import oracle_ctypes as oc
    for a in alphas(case):
        with np.errstate(all="ignore"):
            x, _, c = oc.forward_pass(p, None, x0, a * u0, None, 1.0, lims(case))
        if np.all(np.abs(x) < 1e8):
            return float(c.sum())
    return float("nan")


@functools.lru_cache(maxsize=None)
def oracle_results(name):
    """the oracle's solve of every trajectory of a case: a list of dicts (arrays, summary, the seven trace keys, initial cost).
    Computed once and shared; the callers do not change it."""
    from oracle import oracle_ctypes as oc
    case = BY_NAME[name]
    assert case["oracle"]
    p = oracle_problem(case)
    x0, u0 = starts(case)
    out = []
    for b in range(x0.shape[1]):
        x, u, (K, k, Quu), Vx, Vxx, cost, info = oc.ilqg_trace7(p, x0[:, b], u0[..., b], lims(case), **dict(case["opts"]))
        out.append(dict(x=x, u=u, K=K, k=k, Quu=Quu, Vx=Vx, Vxx=Vxx, cost=cost, info=info, history=info["history"],
                        cost0=initial_cost(case, p, x0[:, b], u0[..., b])))
    return out


# ------------------------------------------------------------------------------------------------- reading a result
def accepted_index(case, alpha_row):
    """index into the case's step sizes of every trace row (-1: no step)"""
    al = alphas(case)
    idx = np.full(len(alpha_row), -1)
    for i, a in enumerate(alpha_row):
        if not np.isnan(a):
            (hit,) = np.nonzero(al == a)
            assert len(hit) == 1, (case["name"], a)
            idx[i] = hit[0]
    return idx


def forwards_in_rows(case, idx):
    """rollouts the serial search of the reference does in the iterations that left a trace row"""
    return int(np.sum(np.where(idx >= 0, idx + 1, len(alphas(case)))))


def exit_decision(case, r):
    """the last iteration of a solve that ended with status 2 leaves no trace row: its step size, Δcost and z rebuilt from the summary
    (n_forward, dV of the last back pass, the costs).  Returns (index, Δcost, expected, z)."""
    info, h = r["info"], r["history"]
    assert info["status"] == 2
    idx = info["n_forward"] - forwards_in_rows(case, accepted_index(case, h["α"])) - 1
    a = alphas(case)[idx]
    prev = h["cost"][-1] if len(h["cost"]) else r["cost0"]
    dcost = prev - float(np.sum(r["cost"]))
    expected = -a * (info["dV"][0] + a * info["dV"][1])
    z = dcost / expected if expected > 0 else float(np.sign(dcost))
    return idx, dcost, expected, z


def observed_tags(case, results):
    """the tags the oracle's result of a case shows"""
    t = set()
    al = alphas(case)
    na = len(al)
    f, lmin, rrmin = opt(case, "lam_factor"), opt(case, "lam_min"), opt(case, "reduce_ratio_min")
    if na in (2, 3, 4, 16):
        t.add("n_alpha_%d" % na)
    if case["lims"]:
        t.add("lims")
    if case["family"] == "pendcart":
        t.add("pendcart")
    for r in results:
        info, h = r["info"], r["history"]
        st, it, tl = info["status"], info["iter"], info["trace_len"]
        idx = accepted_index(case, h["α"])
        fr = forwards_in_rows(case, idx)
        z, imp = h["reduce_ratio"], h["improvement"]
        acc, none = idx >= 0, idx < 0
        if st == 1:
            t.add("exit_grad")
            if it == 1 and tl == 0:
                t.add("exit_grad_first_iter")
        if tl and np.any(h["grad_norm"] < opt(case, "tol_grad")):
            t.add("grad_small_lambda_large")
        if st == 2:
            t.add("exit_cost")
            if it == 1:
                t.add("exit_cost_first_iter")
            ei, dcost, expected, ze = exit_decision(case, r)
            if rrmin < 0 and dcost < 0:
                t.add("cost_raise_accepted")
        if st == 3:
            t.add("exit_lambda_backpass" if info["n_forward"] == fr else "exit_lambda_search")
            assert info["n_forward"] in (fr, fr + na)
        if st == 4:
            t.add("exit_maxiter")
            if opt(case, "max_iter") == 0 and it == 1 and info["n_backpass"] == 0:
                t.add("maxiter_zero")
            if opt(case, "max_iter") == 1 and it == 2:
                t.add("maxiter_one")
        if st == -1:
            t.add("exit_init_diverged")
        if none.any():
            t.update({"alpha_nan_rows", "accept_none"})
            if np.any(none & (z == 0) & (imp == 0)):
                t.add("z_zero_rows")
            if np.any(none & (z == -1)):
                t.add("z_minus_one_rows")
            if rrmin == 1.5 and np.any(none & (z > 0.9) & (z < 1.5)):
                t.add("search_failed_z_near_one")
        if not case["lims"] and np.any([i > 0 and np.all(al[:i] > 2) for i in idx]):
            t.add("overshoot_rejected_then_accepted")
        if np.any(acc & (z > 0.2) & (z < 0.8)):
            t.add("rr_mid_accepted")
        if acc.sum() >= 3 and np.all(idx == 1):
            t.add("second_alpha_every_time")
        if al[0] >= 1e100 and np.any(idx == 1):
            t.add("nonfinite_candidate_rejected")
        if np.any(h["λ"] == lmin):
            t.add("lambda_at_min_rows")
        prev = np.concatenate([[opt(case, "dlam")], h["dλ"][:-1]])
        if np.any(acc & (h["dλ"] == 1.0 / f) & (prev / f > 1.0 / f)):
            t.add("dlambda_inverse_factor")
        if np.any(acc & (h["dλ"] == prev / f) & (prev / f < 1.0 / f)):
            t.add("dlambda_quotient")
        if na == 1 and acc.any():
            t.add("single_alpha")
        for i in set(idx[acc]):
            if i < 4:
                t.add("accept_idx_%d" % i)
            if i == na - 1 and na >= 2:
                t.add("accept_idx_last")
        if info["n_backpass"] > it and info["n_forward"] > 0 and st != 3:
            t.add("backpass_retry_then_search")
    return t


def _away(v, thr):
    """distance of a decided quantity from its threshold: relative to the threshold, absolute where the threshold is 0"""
    return abs(v - thr) / (abs(thr) if thr != 0 else 1.0)


def margins(case, results):
    """Every decision the solves of a case took, as {quantity: [distance from its threshold, ...]}, and the count of rows whose value
    is exact by construction (z from sign(): -1, 0, 1; Δcost = 0; NaN) and therefore exempt.
      reduce_ratio against reduce_ratio_min   every trace row (the last candidate tried) and the exit of a status-2 solve
      improvement  against tol_fun            the rows with a step and the exit of a status-2 solve
      grad_norm    against tol_grad           every row, and the exit of a status-1 solve
      λ            against λmax and 1e-5      the initial value, every row, the value after the solve"""
    m = {"reduce_ratio": [], "improvement": [], "grad_norm": [], "λ_vs_λmax": [], "λ_vs_1e-5": []}
    exact = 0
    rrmin, tol_fun, tol_grad, lmax = (opt(case, k) for k in ("reduce_ratio_min", "tol_fun", "tol_grad", "lam_max"))
    for r in results:
        info, h = r["info"], r["history"]
        idx = accepted_index(case, h["α"])
        zs, imps = list(h["reduce_ratio"]), [v for v, i in zip(h["improvement"], idx) if i >= 0]
        gs = list(h["grad_norm"])
        if info["status"] == 2:
            _, dcost, expected, z = exit_decision(case, r)
            zs.append(z); imps.append(dcost)
        if info["status"] == 1:
            gs.append(info["g_norm"])
        for z in zs:
            if np.isnan(z) or z in (-1.0, 0.0, 1.0):
                exact += 1
            else:
                m["reduce_ratio"].append(_away(z, rrmin))
        for v in imps:
            if v == 0.0 or np.isnan(v):
                exact += 1
            else:
                m["improvement"].append(_away(v, tol_fun))
        for v in gs:
            m["grad_norm"].append(_away(v, tol_grad))
        if info["status"] != -1:
            for v in [opt(case, "lam")] + list(h["λ"]) + [info["lam"]]:
                m["λ_vs_λmax"].append(_away(v, lmax))
                m["λ_vs_1e-5"].append(_away(v, 1e-5))
    return m, exact
