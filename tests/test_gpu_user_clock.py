"""DDP_USER_CLOCK on the GPU: a DeviceProblem made with clock=True sees the absolute step t = c + i in every kernel that calls the
user's functions, at the array level, in iLQG, in the slot scheduler (one clock per problem), in the closed loop on the device (the
clock advances where the slot is armed again; the plant gets the absolute t) and in iLQGkl.

The independent reference throughout is the UNCLOCKED TWIN (tests/user_clock_cases.py): the text of user_examples/car_track.hip with t
replaced by i, compiled without the flag and run through the entry points that existed before it, with the sampled paths of its
parameter column shifted by the clock on the host.  It shares no code path with the feature.  Only an integer index differs between
the two programs, so equal bits are expected; the asserts use the suite's parity tolerance (conftest.relerr, 1e-8 per time step).
Where the reference is the clocked problem itself through another entry point (queue against stand-alone batches, device loop against
the host loop) the comparison is bit for bit, as in tests/test_gpu_user_sched.py.  Shapes: n = 4, m = 2, N = 12, L = 64."""
import functools

import numpy as np
import pytest

from conftest import relerr
from user_clock_cases import L_TRACK, nparam_of, shifted, track_f, track_params, twin_source

pytestmark = pytest.mark.gpu

RTOL = 1e-8
n, m, N = 4, 2, 12
T0 = np.array([0, 1, 7, 30, 51])
LIMS = np.array([[-2.0, 2.0], [-1.5, 1.5]])
ALPHAS = np.array([1.0, 0.5, 0.1])
VARIANTS = {"hand": ("car_track", {}), "ad": ("car_track_ad", dict(autodiff=True)), "ad_wave": ("car_track_ad", dict(autodiff=True, wave=True)),
            "hand_wave": ("car_track", dict(wave=True))}


def _same(a, b):
    return np.array_equal(a, b, equal_nan=True)


@pytest.fixture(scope="module")
def ddp():
    import ddp_amd
    return ddp_amd


@functools.lru_cache(maxsize=None)
def _clocked(variant):
    import ddp_amd
    name, kw = VARIANTS[variant]
    return ddp_amd.DeviceProblem(ddp_amd.example_source(name), n, m, nparam=nparam_of(name), terminal=True, clock=True, **kw)


@functools.lru_cache(maxsize=None)
def _twin(horizon=N):
    import ddp_amd
    return ddp_amd.DeviceProblem(twin_source(ddp_amd.example_source("car_track"), horizon), n, m, nparam=nparam_of("car_track"), terminal=True)


@functools.lru_cache(maxsize=None)
def _case(B, seed=11, horizon=N):
    """parameters, start states near the start of the reference path, controls, and a policy around a nominal rollout (of the twin)"""
    import ddp_amd
    rng = np.random.default_rng(seed)
    P = track_params(rng, B)
    x0 = np.stack([P[7] + 0.2 * rng.standard_normal(B), P[8] + 0.2 * rng.standard_normal(B), 0.3 + 0.1 * rng.standard_normal(B),
                   0.8 + 0.1 * rng.standard_normal(B)])
    u0 = 0.2 * rng.standard_normal((m, horizon, B))
    x, _, _ = ddp_amd.forward_pass(None, x0, u0, None, 1.0, _twin(horizon), None, params=P)
    pol = ddp_amd.GaussianPolicy(horizon, n, m, 0.1 * rng.standard_normal((m, n, horizon, B)), 0.1 * rng.standard_normal((m, horizon, B)),
                                 np.zeros((m, m, horizon, B)), np.zeros((m, m, horizon, B)))
    for a in (P, x0, u0, x):
        a.setflags(write=False)
    return P, x0, u0, x, pol


@functools.lru_cache(maxsize=None)
def _twin_arrays(t0):
    """forward_pass, df and costfun of the twin with its paths shifted by the clocks t0 (a tuple of 5): computed once, shared"""
    import ddp_amd
    P, x0, u0, x, pol = _case(5)
    Ps = shifted(P, np.array(t0))
    fp = ddp_amd.forward_pass(pol, x0, u0, x, ALPHAS, _twin(), LIMS, params=Ps)
    d = ddp_amd.df(_twin(), x, u0, params=Ps)
    c = ddp_amd.costfun(_twin(), x, u0, params=Ps)
    return fp, d, c


def _close(got, ref, what):
    for k, (a, b) in enumerate(zip(got, ref)):
        if np.size(b):
            e = relerr(a, b)
            assert e < RTOL, (what, k, e)


# --------------------------------------------------------------------------------------------------------------- 1. array level
@pytest.mark.parametrize("variant", sorted(VARIANTS))
def test_array_level_calls_see_the_clock(ddp, variant):
    """forward_pass (three step sizes), df and costfun with one clock per trajectory, with a scalar clock and with none, against the
    twin; 51 + 11 stays below the last sample, so the clocks [60, 64, 70, 90, 200] check the clamp at L - 1 besides"""
    prob = _clocked(variant)
    P, x0, u0, x, pol = _case(5)
    h = ddp.default_handle()
    for t0 in (T0, 7, None, np.array([60, 64, 70, 90, 200])):
        ref = _twin_arrays(tuple(np.broadcast_to(0 if t0 is None else t0, (5,)).tolist()))
        fp = ddp.forward_pass(pol, x0, u0, x, ALPHAS, prob, LIMS, params=P, t0=t0)
        assert h.last_kernel(1) == ("ddp_user_rollout_wave" if "wave" in variant else "ddp_user_rollout")
        d = ddp.df(prob, x, u0, params=P, t0=t0)
        assert h.last_kernel(2) == {"hand": "ddp_user_df", "hand_wave": "ddp_user_df", "ad": "ddp_user_df_ad", "ad_wave": "ddp_user_df_wave"}[variant]
        c = ddp.costfun(prob, x, u0, params=P, t0=t0)
        _close(fp, ref[0], "forward_pass"); _close(d, ref[1], "df"); _close((c,), (ref[2],), "costfun")
        if t0 is None:                                           # no clock given: every clock is 0
            z = (ddp.forward_pass(pol, x0, u0, x, ALPHAS, prob, LIMS, params=P, t0=0), ddp.df(prob, x, u0, params=P, t0=0),
                 ddp.costfun(prob, x, u0, params=P, t0=0))
            assert all(_same(a, b) for a, b in zip(fp + tuple(d) + (c,), z[0] + tuple(z[1]) + (z[2],)))
    # the clock matters: other clocks, other numbers
    assert relerr(_twin_arrays(tuple(T0.tolist()))[2], _twin_arrays((0,) * 5)[2]) > 1e-3
    if variant == "ad":                                          # AD derivatives against the hand-written ones at the same clocks
        _close(ddp.df(prob, x, u0, params=P, t0=T0), ddp.df(_clocked("hand"), x, u0, params=P, t0=T0), "ad vs hand")


# ----------------------------------------------------------------------------------------------------------------------- 2. iLQG
def _outputs(r):
    return r[:2] + (r[2].K, r[2].k) + r[3:6] + (r[6]["stats"],)


def test_ilqg_with_one_clock_per_trajectory(ddp):
    P, x0, u0, _, _ = _case(5)
    kw = dict(max_iter=30, lims=LIMS, timing=False)
    r = ddp.iLQG(_clocked("hand"), x0, u0, params=P, t0=T0, **kw)
    t = ddp.iLQG(_twin(), x0, u0, params=shifted(P, T0), **kw)
    assert (r[6]["status"] > 0).all() and (r[6]["iter"] > 2).all(), r[6]["stats"][:2]
    _close(_outputs(r), _outputs(t), "iLQG")
    z = ddp.iLQG(_clocked("hand"), x0, u0, params=P, **kw)       # no t0: clock 0, another problem
    assert relerr(z[0], r[0]) > 1e-3
    _close(_outputs(z), _outputs(ddp.iLQG(_twin(), x0, u0, params=P, **kw)), "iLQG at clock 0")


def test_compaction_moves_the_clock_with_its_trajectory(ddp, monkeypatch):
    """DDP_ILQG_COMPACT=2: the live trajectories of a stand-alone solve move to smaller working sets, where slot b is no longer
    trajectory b; the clocks are gathered with them.  12 cars whose clocks differ: the solves of the run without compaction"""
    B = 12
    t0 = 4 * np.arange(B)
    P, x0, u0, _, _ = _case(B, seed=15)
    out = {}
    for v in ("0", "2"):
        monkeypatch.setenv("DDP_ILQG_COMPACT", v)
        out[v] = ddp.iLQG(_clocked("hand"), x0, u0, params=P, t0=t0, max_iter=60, lims=LIMS, timing=False)
    monkeypatch.delenv("DDP_ILQG_COMPACT")
    it = out["0"][6]["iter"]
    print("iterations", it)
    assert np.sort(it)[B // 2 - 1] + 4 <= it.max(), it           # half of the batch ends a poll interval before the last one: it compacts
    for a, b in zip(_outputs(out["2"]), _outputs(out["0"])):
        assert relerr(a, b) < 1e-12
    _close(_outputs(out["2"]), _outputs(ddp.iLQG(_twin(), x0, u0, params=shifted(P, t0), max_iter=60, lims=LIMS, timing=False)), "compacted")


# ---------------------------------------------------------------------------------------------------------------------- 3. queue
def test_queue_gives_every_problem_its_clock(ddp):
    """7 problems through 3 slots: a slot that takes its second or third problem must run with THAT problem's clock.  Bit for bit the
    stand-alone solves of the clocked problem at batch size 3, and the twin's queue at tolerance"""
    P_, S = 7, 3
    t0 = np.array([0, 3, 3, 11, 20, 1, 40])
    P, x0, u0, _, _ = _case(P_, seed=12)
    kw = dict(max_iter=30, lims=LIMS)
    q = ddp.iLQG_queue(_clocked("hand"), x0, u0, slots=S, params=P, t0=t0, **kw)
    assert (q[6]["status"] > 0).all(), q[6]["status"]
    for c in range(0, P_, S):
        sel = np.arange(c, c + S) if c + S <= P_ else np.arange(P_ - S, P_)
        r = ddp.iLQG(_clocked("hand"), x0[:, sel], u0[:, :, sel], params=P[:, sel], t0=t0[sel], timing=False, **kw)
        for a, b in zip(_outputs(q), _outputs(r)):
            assert _same(a[..., sel], b), sel[0]
    t = ddp.iLQG_queue(_twin(), x0, u0, slots=S, params=shifted(P, t0), **kw)
    _close(_outputs(q), _outputs(t), "queue")


# ------------------------------------------------------------------------------------------------------------------------ 4. MPC
def test_mpc_without_a_plant_advances_the_clock_on_the_device(ddp):
    """4 cars, 6 closed-loop steps, N = 10: the solve at step s runs with the clock t0 + s.  Bit for bit the host loop of iLQG calls on the
    clocked problem with t0 + s; at tolerance the twin's host loop, whose parameters are shifted again at every step"""
    B, steps, H = 4, 6, 10
    t0 = np.array([0, 5, 5, 17])
    P, x0, u0, _, _ = _case(B, seed=13, horizon=H)
    kw = dict(max_iter=25, lims=LIMS)
    car = _clocked("hand")
    xcl, ucl, scl, xp, up, git = ddp.iLQG_mpc(car, x0, u0, steps, params=P, t0=t0, **kw)
    assert (scl[0] > 0).all(), scl[0]
    xs, us, xt, ut = x0.copy(), u0.copy(), x0.copy(), u0.copy()
    assert _same(xcl[:, 0], x0)
    for s in range(steps):
        r = ddp.iLQG(car, xs, us, params=P, t0=t0 + s, timing=False, **kw)
        assert _same(scl[:, s], r[6]["stats"]), s
        assert _same(xcl[:, s], r[0][:, 0]) and _same(ucl[:, s], r[1][:, 0]) and _same(xcl[:, s + 1], r[0][:, 1]), s
        xs, us = np.ascontiguousarray(r[0][:, 1]), ddp.mpc_shift(r[1])
        w = ddp.iLQG(_twin(H), xt, ut, params=shifted(P, t0 + s), timing=False, **kw)
        _close((xcl[:, s], ucl[:, s], xcl[:, s + 1], scl[:, s]), (w[0][:, 0], w[1][:, 0], w[0][:, 1], w[6]["stats"]), "twin step %d" % s)
        xt, ut = np.ascontiguousarray(w[0][:, 1]), ddp.mpc_shift(w[1])
    assert _same(xp, r[0]) and _same(up, r[1])
    _close((xp, up), (w[0], w[1]), "last plan")
    frozen = ddp.iLQG_mpc(_twin(H), x0, u0, steps, params=shifted(P, t0), **kw)      # a clock that stands still: another loop
    assert relerr(frozen[0], xcl) > 1e-3


def test_mpc_with_a_plant_gets_the_absolute_step(ddp):
    """car_track_plant.hip, the sizes of the test above, a disturbance that is non-zero at the absolute steps 6 and 7 only: every
    closed-loop state is the plant's step in NumPy at t0 + s, and the push shows at the steps 6 - t0 and 7 - t0 of the trajectories
    whose window holds them (t0 = 5), nowhere in the others (t0 = 0: steps 0..5; t0 = 17)"""
    B, steps, H, L = 4, 6, 10, L_TRACK
    t0 = np.array([0, 5, 5, 17])
    P4, x0, u0, _, _ = _case(B, seed=13, horizon=H)
    P = np.zeros((nparam_of("car_track_plant"), B))
    P[:7 + 4 * L] = P4
    d = np.zeros((2, L)); d[:, 6] = (1.5, -1.0); d[:, 7] = (-0.5, 2.0)
    P[7 + 4 * L:] = d.ravel(order="F")[:, None]
    car = ddp.DeviceProblem(ddp.example_source("car_track_plant"), n, m, nparam=P.shape[0], terminal=True, plant=True, clock=True)
    xcl, ucl, scl, xp, up, git = ddp.iLQG_mpc(car, x0, u0, steps, params=P, t0=t0, max_iter=25, lims=LIMS)
    assert ddp.default_handle().last_kernel(4) == "ddp_user_plant"
    assert (scl[0] > 0).all(), scl[0]
    for s in range(steps):
        for b in range(B):
            model = track_f(P[:, b], xcl[:, s, b], ucl[:, s, b])
            t = min(int(t0[b]) + s, L - 1)
            ref = model + P[0, b] * np.array([d[0, t], d[1, t], 0.0, 0.0])
            assert relerr(xcl[:, s + 1, b], ref) < 1e-12, (s, b)
            pushed = np.abs(xcl[:2, s + 1, b] - model[:2]).max() > 1e-3
            assert pushed == (int(t0[b]) + s in (6, 7)), (s, b)


# --------------------------------------------------------------------------------------------------------------------- 6. iLQGkl
def test_ilqgkl_evaluates_the_model_at_absolute_time(ddp):
    from ddp_amd import kl
    B = 2
    t0 = np.array([0, 9])
    rng = np.random.default_rng(14)
    P, x0, u0, _, _ = _case(B, seed=14)
    u = np.array(u0)
    x, _, c = ddp.forward_pass(None, x0, u, None, 1.0, _clocked("hand"), None, params=P, t0=t0)
    Sip = np.stack([np.stack([(lambda a: a @ a.T + 2.0 * np.eye(m))(rng.standard_normal((m, m))) for _ in range(N)], -1) for _ in range(B)], -1)
    Sp = np.stack([np.stack([np.linalg.inv(Sip[:, :, t, b]) for t in range(N)], -1) for b in range(B)], -1)
    prev = ddp.GaussianPolicy(N, n, m, 0.1 * rng.standard_normal((m, n, N, B)), u, Sp, Sip)
    kw = dict(kl_step=0.5, max_iter=20, cost=c)
    model = kl.Model(None, None, 1e-3 * np.eye(n))
    r = kl.iLQGkl(_clocked("hand"), x, prev, model, params=P, t0=t0, **kw)
    w = kl.iLQGkl(_twin(), x, prev, model, params=shifted(P, t0), **kw)
    assert np.array_equal(r[6]["iter"], w[6]["iter"]) and np.array_equal(r[6]["status"], w[6]["status"])
    for a, b in ((r[0], w[0]), (r[1], w[1]), (r[2].K, w[2].K), (r[4], w[4]), (r[5], w[5])):
        assert relerr(a, b) < RTOL
    z = kl.iLQGkl(_clocked("hand"), x, prev, model, params=P, **kw)                  # no clocks: another problem for trajectory 1
    assert relerr(z[1][..., 1], r[1][..., 1]) > 1e-6


# ------------------------------------------------------------------------------------------------------------------ 7. refusals
def test_refusals_launch_nothing_and_leave_the_clock_at_zero(ddp):
    P, x0, u0, x, pol = _case(5)
    h = ddp.default_handle()
    car = _clocked("hand")
    ref0 = ddp.forward_pass(pol, x0, u0, x, ALPHAS, car, LIMS, params=P, t0=0)
    before = [h.last_kernel(k) for k in range(5)]
    with pytest.raises(ddp.DDPError, match=r"clock=True \(DDP_USER_CLOCK\)"):
        ddp.iLQG(_twin(), x0, u0, params=P, t0=T0)
    with pytest.raises(ddp.DDPError, match=r"3 clocks.* 5 trajectories"):
        ddp.iLQG(car, x0, u0, params=P, t0=T0[:3])
    with pytest.raises(ddp.DDPError, match=r"3 clocks.* 5 trajectories"):
        ddp.forward_pass(pol, x0, u0, x, ALPHAS, car, LIMS, params=P, t0=T0[:3])
    with pytest.raises(ddp.DDPError, match=r"DDP_USER_CLOCK \| DDP_USER_SECOND_ORDER is refused"):
        bad = ddp.DeviceProblem(ddp.example_source("car_track_ad"), n, m, nparam=nparam_of("car_track_ad"), terminal=True, autodiff=True,
                                clock=True, second_order=True)
        ddp.iLQG(bad, x0, u0, params=P, t0=T0)
    assert [h.last_kernel(k) for k in range(5)] == before
    # after a call that raised, a call without t0 runs at clock 0
    again = ddp.forward_pass(pol, x0, u0, x, ALPHAS, car, LIMS, params=P)
    assert all(_same(a, b) for a, b in zip(again, ref0))
    _close(again, _twin_arrays((0,) * 5)[0], "clock 0 after a refusal")
