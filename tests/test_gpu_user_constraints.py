"""DDP_USER_CONSTRAINTS on the GPU (DeviceProblem(..., constraints=nc), user_examples/car_keepout_ad.hip): ddp_user_constraints and the
augmented df / costfun against NumPy closed forms, one round of the solve against the NumPy inner solve, the multiplier update against its
formula, composition and determinism of ddp_user_ilqg_al bit for bit, the whole loop against the NumPy loop of tests/constraints_cases.py,
the same on the wave kernels and with control limits, and the refusals.

Shapes: (n, m, nc) = (4, 2, 2) with N = 30, B = 5 and N = 70, B = 3 (more than one wave of steps: the loop of ddp_user_al_update and its
partial tail)."""
import numpy as np
import pytest

import constraints_cases as cc
from conftest import relerr

pytestmark = pytest.mark.gpu

SEED = 1
SHAPES = [(30, 5), (70, 3)]
OUT_KEYS = ("x", "u", "K", "k", "Quu", "Vx", "Vxx", "cost", "λ", "μ", "g")


@pytest.fixture(scope="module")
def ddp():
    import ddp_amd
    return ddp_amd


def _problem(ddp, **kw):
    return ddp.DeviceProblem(ddp.example_source("car_keepout_ad"), 4, 2, nparam=cc.NPARAM, terminal=True, autodiff=True, **kw)


@pytest.fixture(scope="module")
def prob(ddp):
    return _problem(ddp, constraints=cc.NC)


@pytest.fixture(scope="module")
def prob_wave(ddp):
    return _problem(ddp, constraints=cc.NC, wave=True)


@pytest.fixture(scope="module")
def prob_plain(ddp):
    """the same source compiled without the flag (its `constraints` template is never instantiated)"""
    return _problem(ddp)


def _fast_through_the_disc(N, B):
    """trajectories that drive through the disc above the cap for a while: both constraints change sign along the horizon"""
    p, x0, u0 = cc.designed(SEED + N, B, N)
    x0 = x0.copy()
    x0[3] = 1.5
    u = 30.0 * u0
    u[0] -= 0.4 * (np.arange(N)[:, None] > N // 2)               # brakes in the second half: under the cap again
    x = np.stack([cc.rollout(p[:, b], x0[:, b], u[:, :, b]) for b in range(B)], axis=-1)
    rng = np.random.default_rng(5)
    lam = rng.uniform(0.0, 0.5, (cc.NC, N, B)) * (rng.uniform(size=(cc.NC, N, B)) < 0.5)     # zero and positive, mixed
    mu = np.array([0.5, 2.0, 10.0, 1.0, 4.0])[:B]
    return p, x0, u, x, lam, mu


def _all(out):
    x, u, pol, Vx, Vxx, cost, info = out
    return dict(x=x, u=u, K=pol.K, k=pol.k, Quu=pol.Σi, Vx=Vx, Vxx=Vxx, cost=cost, λ=info["λ"], μ=info["μ"], g=info["g"])


def _same_bits(a, b, rows=None, what=""):
    for key in OUT_KEYS:
        va, vb = a[key], b[key]
        if rows is not None:
            va, vb = va[..., rows], vb[..., rows]
        assert np.array_equal(va, vb), (what, key)


@pytest.mark.parametrize("N,B", SHAPES)
@pytest.mark.parametrize("wave", [False, True])
def test_constraints_df_costfun_against_numpy(ddp, prob, prob_wave, prob_plain, N, B, wave):
    P = prob_wave if wave else prob
    p, x0, u, x, lam, mu = _fast_through_the_disc(N, B)
    g_ref = cc.constraints(p[:, None, :], x, u)
    t = lam + mu * g_ref
    for j in range(cc.NC):                                       # the data is what it claims: each constraint on both sides, λ mixed
        assert (t[j] > 0).any() and (t[j] < 0).any() and (g_ref[j] > 0).any() and (g_ref[j] < 0).any()
    assert (lam == 0).any() and (lam > 0).any()
    g = ddp.constraints(P, x, u, params=p)
    # g is a handful of roundings on operands of its own size (contraction may merge some): 1e-13 of the largest leaves a decade or two
    assert np.max(np.abs(g - g_ref)) <= 1e-13 * max(1.0, np.max(np.abs(g_ref)))
    d = ddp.df(P, x, u, params=p, multipliers=(lam, mu))
    c = ddp.costfun(P, x, u, params=p, multipliers=(lam, mu))
    fx, fu, cx, cu, cxx, cxu, cuu = d[0], d[1], d[5], d[6], d[7], d[8], d[9]
    assert np.array_equal(cxx, cxx.transpose(1, 0, 2, 3)) and np.array_equal(cuu, cuu.transpose(1, 0, 2, 3))
    saw_cross = False
    for b in range(B):
        ref = cc.derivs_trajectory(p[:, b], x[..., b], u[..., b], lam[..., b], mu[b])
        for name, got, want in zip(("fx", "fu", "cx", "cu", "cxx", "cxu", "cuu"), (fx, fu, cx, cu, cxx, cxu, cuu), ref):
            e = relerr(got[..., b], want)
            print("df", N, b, name, e)
            assert e <= 1e-8, (name, b, e)
        saw_cross |= bool(np.any(ref[5] != 0))                   # the cap mixes state and control: the penalty reaches cxu
        e = relerr(c[:, b], cc.cost_trajectory(p[:, b], x[..., b], u[..., b], lam[..., b], mu[b]))
        print("costfun", N, b, e)
        assert e <= 1e-8, (b, e)
    assert saw_cross
    # without multipliers: the raw cost, bit for bit what the same model gives without the flag
    if not wave:
        d0, dp_ = ddp.df(P, x, u, params=p), ddp.df(prob_plain, x, u, params=p)
        for k in (0, 1, 5, 6, 7, 8, 9):
            assert np.array_equal(d0[k], dp_[k]), k
        assert np.array_equal(ddp.costfun(P, x, u, params=p), ddp.costfun(prob_plain, x, u, params=p))
        f0 = ddp.forward_pass(None, x0, u, None, 1.0, P, None, params=p)
        f1 = ddp.forward_pass(None, x0, u, None, 1.0, prob_plain, None, params=p)
        assert all(np.array_equal(a, b_) for a, b_ in zip(f0, f1))
        # and the rollout's fused cost under multipliers is the cost kernel's
        fm = ddp.forward_pass(None, x0, u, None, 1.0, P, None, params=p, multipliers=(lam, mu))
        assert relerr(fm[2], ddp.costfun(P, fm[0], fm[1], params=p, multipliers=(lam, mu))) <= 1e-12


def test_one_round_against_the_numpy_inner_solve_and_the_update_formula(ddp, prob):
    N, B = SHAPES[0]
    p, x0, u0, plain, loops = cc.reference(SEED, B, N)
    lam0, mu0 = np.zeros((cc.NC, N, B)), np.ones(B)
    x, u, pol, Vx, Vxx, cost, tr = ddp.iLQG(prob, x0, u0, params=p, multipliers=(lam0, mu0))
    for b in range(B):
        r0 = loops[b][1][0]
        ex, eu = relerr(x[..., b], r0["x"]), relerr(u[..., b], r0["u"])
        print("round 0", b, ex, eu, int(tr["iter"][b]), r0["iter"])
        assert ex <= 1e-8 and eu <= 1e-8 and int(tr["iter"][b]) == r0["iter"], (b, ex, eu)
        assert relerr(cost[:, b], r0["cost"]) <= 1e-8
    # the unconstrained solve (no multipliers) is the plain NumPy one, and it violates
    xp, up = ddp.iLQG(prob, x0, u0, params=p)[:2]
    for b in range(B):
        assert relerr(xp[..., b], plain[b][0]) <= 1e-8 and relerr(up[..., b], plain[b][1]) <= 1e-8
    # max_outer = 1: the same solve, frozen with the multipliers it was computed under (status 2: none is feasible after one round)
    a1 = ddp.iLQG_al(prob, x0, u0, params=p, max_outer=1)
    o1, i1 = _all(a1), a1[6]
    assert np.array_equal(o1["x"], x) and np.array_equal(o1["u"], u) and np.array_equal(o1["cost"], cost)
    assert np.all(i1["status"] == 2) and np.all(i1["rounds"] == 1) and np.array_equal(i1["inner_iters"], tr["iter"])
    assert np.array_equal(o1["λ"], lam0) and np.array_equal(o1["μ"], mu0) and np.array_equal(i1["mu_last"], mu0)
    g1 = cc.constraints(p[:, None, :], o1["x"], o1["u"])
    assert np.max(np.abs(o1["g"] - g1)) <= 1e-12 * max(1.0, np.max(np.abs(g1)))
    assert np.array_equal(o1["g"], ddp.constraints(prob, o1["x"], o1["u"], params=p))
    assert np.max(np.abs(i1["cviol"] - np.maximum(0.0, g1.max(axis=(0, 1))))) <= 1e-12
    assert np.array_equal(i1["cviol"], np.maximum(0.0, o1["g"].max(axis=(0, 1))))         # the maximum itself is exact
    raw = np.array([cc.cost_trajectory(p[:, b], o1["x"][..., b], o1["u"][..., b]).sum() for b in range(B)])
    assert np.max(np.abs(i1["raw_cost"] - raw)) <= 1e-12 * np.max(np.abs(raw))
    # max_outer = 2: round 1 ran under λ⁺ = max(0, λ + μ g), μ⁺ = mu_factor μ of round 0, and froze with them
    a2 = ddp.iLQG_al(prob, x0, u0, params=p, max_outer=2)
    o2, i2 = _all(a2), a2[6]
    lam_f, mu_f = np.maximum(0.0, lam0 + mu0 * g1), np.minimum(10.0 * mu0, 1e8)
    assert np.max(np.abs(o2["λ"] - lam_f)) <= 1e-12 * max(1.0, np.max(np.abs(lam_f))) and np.max(np.abs(o2["μ"] - mu_f)) <= 1e-12 * 10.0
    assert np.array_equal(o2["λ"], np.maximum(0.0, lam0 + mu0 * o1["g"]))                 # on the device's own g: the same bits
    assert np.all(i2["rounds"] == 2) and np.array_equal(i2["mu_last"], mu_f)
    g2 = cc.constraints(p[:, None, :], o2["x"], o2["u"])
    assert np.max(np.abs(i2["cviol"] - np.maximum(0.0, g2.max(axis=(0, 1))))) <= 1e-12


def _chain(ddp, P, p, x0, u0, rounds, lims=None):
    """`rounds` calls of one round each, seeded with the previous x, u and the update formula in NumPy on the returned g"""
    outs = []
    x, u, mult = x0, u0, None
    for r in range(rounds):
        a = ddp.iLQG_al(P, x, u, params=p, max_outer=1, multipliers=mult, lims=lims)
        o = _all(a)
        outs.append((o, a[6]))
        x, u, mult = o["x"], o["u"], (np.maximum(0.0, o["λ"] + o["μ"] * o["g"]), np.minimum(10.0 * o["μ"], 1e8))
    return outs


def _composition(ddp, P, p, x0, u0, k, lims=None):
    full = ddp.iLQG_al(P, x0, u0, params=p, max_outer=k, lims=lims)
    of, info = _all(full), full[6]
    again = ddp.iLQG_al(P, x0, u0, params=p, max_outer=k, lims=lims)
    _same_bits(of, _all(again), what="two identical calls")
    assert np.array_equal(info["al_stats"], again[6]["al_stats"]) and np.array_equal(info["stats"], again[6]["stats"])
    chain = _chain(ddp, P, p, x0, u0, k, lims)
    for b in range(x0.shape[1]):                                 # every trajectory: the chained call of the round it froze in
        r = int(info["rounds"][b])
        _same_bits(of, chain[r - 1][0], rows=b, what="k rounds against %d chained calls, trajectory %d" % (r, b))
        assert info["cviol"][b] == chain[r - 1][1]["cviol"][b] and np.array_equal(info["stats"][:, b], chain[r - 1][1]["stats"][:, b])
        assert info["inner_iters"][b] == sum(int(c[1]["inner_iters"][b]) for c in chain[:r])
    return of, info


@pytest.mark.parametrize("N,B", SHAPES)
def test_composition_determinism_and_frozen_trajectories(ddp, prob, N, B):
    p, x0, u0 = cc.designed(SEED, B, N)
    _composition(ddp, prob, p, x0, u0, 3)
    full = ddp.iLQG_al(prob, x0, u0, params=p)
    of, info = _all(full), full[6]
    assert np.all(info["status"] == 1) and np.all(info["cviol"] <= 1e-5), (info["status"], info["cviol"])
    assert info["rounds"].min() >= 2
    if (N, B) == SHAPES[0]:                                      # the designed inputs freeze in different rounds: a mixed batch below
        assert len(set(info["rounds"])) >= 2, info["rounds"]
    for r in sorted(set(int(v) for v in info["rounds"])):        # frozen in round r - 1: the outputs of a max_outer = r call
        short = ddp.iLQG_al(prob, x0, u0, params=p, max_outer=r)
        rows = np.flatnonzero(info["rounds"] == r)
        _same_bits(of, _all(short), rows=rows, what="frozen after %d rounds" % r)
        assert np.array_equal(info["al_stats"][:, rows], short[6]["al_stats"][:, rows])


def test_the_whole_loop_against_the_numpy_loop(ddp, prob):
    N, B = SHAPES[0]
    p, x0, u0, plain, loops = cc.reference(SEED, B, N)
    full = ddp.iLQG_al(prob, x0, u0, params=p)
    info = full[6]
    assert np.all(info["status"] == 1) and np.all(info["cviol"] <= 1e-5), (info["status"], info["cviol"])
    R = max(len(lp[1]) for lp in loops)
    together = np.ones(B, dtype=bool)                            # inner iteration counts have coincided so far
    parted_after_round_1 = 0
    for r in range(R):
        a = ddp.iLQG_al(prob, x0, u0, params=p, max_outer=r + 1)
        o, i = _all(a), a[6]
        for b in range(B):
            ref = loops[b][1]
            if r >= len(ref) or not together[b] or int(i["rounds"][b]) != r + 1:
                continue
            ex, eu = relerr(o["x"][..., b], ref[r]["x"]), relerr(o["u"][..., b], ref[r]["u"])
            el = float(np.max(np.abs(o["λ"][..., b] - ref[r]["lam"]))) / max(1.0, float(np.max(np.abs(ref[r]["lam"]))))
            same = int(i["stats"][1, b]) == ref[r]["iter"]
            print("round", r, "trajectory", b, "x", ex, "u", eu, "λ", el, "iters", int(i["stats"][1, b]), ref[r]["iter"])
            assert el <= 1e-8 and o["μ"][b] == ref[r]["mu"], (r, b, el)          # the multipliers this round ran under
            if same:
                assert ex <= 1e-8 and eu <= 1e-8, (r, b, ex, eu)
            else:
                assert r > 0, "round 1 must coincide for every trajectory (trajectory %d)" % b
                together[b] = False
                parted_after_round_1 += 1
    assert parted_after_round_1 <= B // 4, parted_after_round_1
    for b in range(B):
        if together[b]:
            assert int(info["rounds"][b]) == len(loops[b][1])


def test_wave_kernels_one_round_and_composition(ddp, prob, prob_wave):
    N, B = 30, 3
    p, x0, u0, plain, loops = cc.reference(SEED, 5, N)
    p, x0, u0 = p[:, :B], x0[:, :B], u0[..., :B]
    h = ddp.default_handle()
    x, u, pol, Vx, Vxx, cost, tr = ddp.iLQG(prob_wave, x0, u0, params=p, multipliers=(np.zeros((cc.NC, N, B)), np.ones(B)))
    assert h.last_kernel(1) == "ddp_user_rollout_wave" and h.last_kernel(2) == "ddp_user_df_wave"
    for b in range(B):
        r0 = loops[b][1][0]
        assert relerr(x[..., b], r0["x"]) <= 1e-8 and relerr(u[..., b], r0["u"]) <= 1e-8 and int(tr["iter"][b]) == r0["iter"], b
    _composition(ddp, prob_wave, p, x0, u0, 2)
    info = ddp.iLQG_al(prob_wave, x0, u0, params=p)[6]
    assert np.all(info["status"] == 1) and np.all(info["cviol"] <= 1e-5)


def test_control_limits_composition_and_feasibility(ddp, prob):
    N, B = SHAPES[0]
    p, x0, u0 = cc.designed(SEED, B, N)
    lims = np.array([[-1.0, 1.0], [-1.5, 1.5]])
    free = ddp.iLQG_al(prob, x0, u0, params=p)
    assert np.abs(free[1][0]).max() > 1.0 or np.abs(free[1][1]).max() > 1.5         # the limits bind on these inputs
    of, info = _composition(ddp, prob, p, x0, u0, 3, lims=lims)
    full = ddp.iLQG_al(prob, x0, u0, params=p, lims=lims)
    assert np.all(full[6]["status"] == 1) and np.all(full[6]["cviol"] <= 1e-5), (full[6]["status"], full[6]["cviol"])
    assert np.all(full[1][0] >= -1.0) and np.all(full[1][0] <= 1.0) and np.all(full[1][1] >= -1.5) and np.all(full[1][1] <= 1.5)


def test_refusals_before_any_launch_leave_the_problem_usable(ddp, prob):
    from ddp_amd import _lib, kl
    N, B = SHAPES[0]
    p, x0, u, x, lam, mu = _fast_through_the_disc(N, B)
    h = ddp.default_handle()
    before = ddp.costfun(prob, x, u, params=p)
    up = prob._ptr(h)
    L = _lib.lib()
    for n_set, b_set in ((N + 1, B), (N, B - 1)):
        lam_s = np.zeros((cc.NC, n_set, b_set), order="F")
        _lib.check(L.ddp_user_set_multipliers(up, _lib.ptr(lam_s), _lib.ptr(np.ones(b_set)), n_set, b_set))
        try:
            for call in (lambda: ddp.costfun(prob, x, u, params=p), lambda: ddp.df(prob, x, u, params=p),
                         lambda: ddp.forward_pass(None, x0, u, None, 1.0, prob, None, params=p), lambda: ddp.iLQG(prob, x0, u, params=p)):
                with pytest.raises(ddp.DDPError, match="ddp_user_set_multipliers gave"):
                    call()
        finally:
            _lib.check(L.ddp_user_set_multipliers(up, None, None, 0, 0))
    with pytest.raises(ddp.DDPError, match="λ should be"):
        ddp.costfun(prob, x, u, params=p, multipliers=(lam[:, :-1], mu))
    with pytest.raises(ddp.DDPError, match="μ should be"):
        ddp.iLQG_al(prob, x0, u, params=p, multipliers=(lam, mu[:-1]))
    with pytest.raises(ddp.DDPError, match="DDP_USER_CONSTRAINTS"):
        ddp.iLQG_queue(prob, x0, u, params=p)
    with pytest.raises(ddp.DDPError, match="DDP_USER_CONSTRAINTS"):
        ddp.iLQG_mpc(prob, x0, u, 2, params=p)
    pf = np.asfortranarray(p)
    rc = L.ddp_user_ilqgkl_f64(h.raw, up, N, B, _lib.ptr(pf), 1, *([None] * 23))
    assert rc != 0 and "ilqgkl" in L.ddp_last_error().decode() and "DDP_USER_CONSTRAINTS" in L.ddp_last_error().decode()
    with pytest.raises(ddp.DDPError, match="constraints=nc"):
        ddp.iLQG_al(_problem(ddp), x0, u, params=p)
    # afterwards: μ = 0, as if nothing had been set
    assert np.array_equal(ddp.costfun(prob, x, u, params=p), before)


def test_unbatched_call_and_a_start_that_diverges(ddp, prob):
    N, B = SHAPES[0]
    p, x0, u0 = cc.designed(SEED, B, N)
    full = ddp.iLQG_al(prob, x0, u0, params=p)
    one = ddp.iLQG_al(prob, x0[:, 1], u0[..., 1], params=p[:, 1])
    assert one[0].shape == (4, N) and one[6]["λ"].shape == (cc.NC, N) and np.ndim(one[6]["μ"]) == 0
    o, f = _all(one), _all(full)
    for key in OUT_KEYS:                                         # a trajectory's results do not depend on the batch around it
        assert np.array_equal(o[key], f[key][..., 1]), key
    assert np.array_equal(one[6]["al_stats"][:, 0], full[6]["al_stats"][:, 1])
    # an initial control sequence that diverges at every step size: AL status -1 after one round, the others untouched
    ub = u0.copy()
    ub[..., 2] = 1e12
    bad = ddp.iLQG_al(prob, x0, ub, params=p)
    assert bad[6]["status"][2] == -1 and bad[6]["rounds"][2] == 1 and bad[6]["stats"][0, 2] == -1
    assert np.array_equal(bad[6]["λ"][..., 2], np.zeros((cc.NC, N))) and bad[6]["μ"][2] == 1.0
    rows = [0, 1, 3, 4]
    _same_bits(_all(bad), f, rows=rows, what="next to a diverged start")
    assert np.array_equal(bad[6]["al_stats"][:, rows], full[6]["al_stats"][:, rows])
