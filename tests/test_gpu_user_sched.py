"""User problems in the slot scheduler (ddp_user_ilqg_queue_f64) and in the closed loop on the device (ddp_user_ilqg_mpc_f64), with and
without a plant (DDP_USER_PLANT).  Reference: the stand-alone device-resident iLQG of the same DeviceProblem (ddp_user_ilqg_f64) — a
slot performs the launches of a stand-alone solve at batch size `slots`, so every solve must come out with its bits — the C oracle,
and a NumPy restatement of the plant."""
import numpy as np
import pytest

from conftest import relerr

pytestmark = pytest.mark.gpu

PEND_P = dict(g=9.82, l=0.35, h=0.01, d=0.99, goal=np.array([np.pi, 0, 0, 0.0]), Q=np.diag([10.0, 1, 2, 1]), R=1.0)
PEND = dict(lims=np.array([[-5.0, 5.0]]), regType=2, α=10.0 ** np.linspace(0.2, -3, 6), λmax=1e15, tol_fun=1e-8, tol_grad=1e-8, max_iter=60)


def pend_params(P=PEND_P):
    return np.concatenate([[P["g"], P["l"], P["h"], P["d"]], P["goal"], P["Q"].ravel(order="F"), [P["R"]]])


def lq_params(A, B, Q, R):
    return np.concatenate([A.ravel(order="F"), B.ravel(order="F"), Q.ravel(order="F"), R.ravel(order="F")])


def _same(a, b):
    return np.array_equal(a, b, equal_nan=True)


@pytest.fixture(scope="module")
def ddp():
    import ddp_amd
    return ddp_amd


@pytest.fixture(scope="module")
def pend(ddp):
    return ddp.DeviceProblem(ddp.example_source("pendcart"), 4, 1, nparam=25, params=pend_params(), terminal=True)


def _pend_batch(rng, P, T=80):
    x0 = np.tile(np.array([np.pi - 0.6, 0.0, 0.0, 0.0])[:, None], (1, P))
    x0[0] += rng.uniform(-0.4, 0.4, P); x0[1] += rng.uniform(-0.3, 0.3, P)
    u0 = 0.05 * rng.standard_normal((1, T, P))
    prm = np.repeat(pend_params()[:, None], P, axis=1)
    prm[3] = rng.uniform(0.5, 1.5, P)                           # damping
    prm[4] = np.pi + rng.uniform(-0.1, 0.1, P)                  # goal angle
    return x0, u0, prm


def _outputs(r):
    return r[:2] + (r[2].K, r[2].k, r[2].Σi) + r[3:6] + (r[6]["stats"],)


def _batches(P, S):
    """column sets of exactly S problems covering 0..P-1 (the last one overlaps its predecessor when S does not divide P): every
    stand-alone reference runs at the queue's batch size"""
    return [np.arange(c, c + S) if c + S <= P else np.arange(P - S, P) for c in range(0, P, S)]


def test_queue_user_pendulum_equals_standalone_batches_bit_for_bit(ddp, pend):
    """40 user-pendulum solves with their own start states, damping and goal through 16 slots (16 does not divide 40): every output of
    every problem is the one of `iLQG` with the DeviceProblem on a batch of 16 over the same columns, whichever slot it ran on.  (A
    stand-alone batch of 16 never compacts: compaction starts at thousands of slots for n = 4.)"""
    rng = np.random.default_rng(3)
    P, S = 40, 16
    x0, u0, prm = _pend_batch(rng, P)
    q = ddp.iLQG_queue(pend, x0, u0, slots=S, params=prm, **PEND)
    assert ddp.default_handle().last_kernel(1) == "ddp_user_rollout" and ddp.default_handle().last_kernel(2) == "ddp_user_df"
    iters = q[6]["iter"]
    assert (q[6]["status"] > 0).all(), q[6]["status"]
    assert iters.max() > iters.min() + 5                       # unequal solve lengths: slots change problems at different times
    for sel in _batches(P, S):
        r = ddp.iLQG(pend, x0[:, sel], u0[:, :, sel], params=prm[:, sel], timing=False, **PEND)
        for a, b in zip(_outputs(q), _outputs(r)):
            assert _same(a[..., sel], b), sel[0]
    assert q[6]["global_iters"] < 3 * iters.max()            # fewer batch iterations than three lock-step batches of the slowest


def test_queue_const_hessian_per_problem_matches_standalone_and_the_oracle(ddp):
    """LQ example with DDP_USER_CONST_HESSIAN, Q and R scaled differently per problem: a slot that took a new problem must back-propagate
    with ITS Hessians (evaluated when the slot was armed), not with those of the slot's previous problem.  24 problems through 8 slots:
    bits of the stand-alone solves at batch size 8, and the C oracle's iLQG for every solve"""
    from oracle import np_restatement as npr
    from oracle import oracle_ctypes as oc
    rng = np.random.default_rng(8)
    n, m, T, P, S = 10, 2, 60, 24, 8
    Pm = npr.make_lq_problem(rng, T=T)
    qs, rs = rng.uniform(0.3, 3.0, P), rng.uniform(0.2, 5.0, P)
    prm = np.stack([lq_params(Pm["A"], Pm["B"], qs[b] * Pm["Q"], rs[b] * Pm["R"]) for b in range(P)], axis=1)
    lq = ddp.DeviceProblem(ddp.example_source("lq"), n, m, nparam=prm.shape[0], const_hessian=True)
    x0 = np.ones((n, P)) + 0.1 * rng.standard_normal((n, P))
    u0 = 0.1 * rng.standard_normal((m, T, P)) * (1 + np.arange(P) % 5)[None, None, :]
    q = ddp.iLQG_queue(lq, x0, u0, slots=S, params=prm)
    for sel in _batches(P, S):
        r = ddp.iLQG(lq, x0[:, sel], u0[:, :, sel], params=prm[:, sel], timing=False)
        for a, b in zip(_outputs(q), _outputs(r)):
            assert _same(a[..., sel], b), sel[0]
    x, u, pol, Vx, Vxx, cost, tr = q
    for b in range(P):
        p = oc.make_problem("lq", n, m, T, A=Pm["A"], B=Pm["B"], Q=qs[b] * Pm["Q"], R=rs[b] * Pm["R"])
        xr, ur, (Kr, kr, _), vxr, vxxr, cr, info = oc.ilqg(p, x0[:, b], u0[..., b])
        st = tr["stats"][:, b]
        assert (int(st[0]), int(st[1]), int(st[3])) == (info["status"], info["iter"], info["n_backpass"]), b
        for got, ref in ((x[..., b], xr), (u[..., b], ur), (pol.K[..., b], Kr), (Vx[..., b], vxr), (Vxx[..., b], vxxr)):
            assert relerr(got, ref) < 1e-8, b
        assert relerr(cost[:, b], cr, 0) < 1e-8, b


def test_queue_user_problems_with_initially_diverging_problems(ddp):
    """problems whose initial rollout leaves the bound for every step size end with status -1 and zero outputs and hand their slot on;
    problems that need a smaller α for the initial rollout take it; the others are the stand-alone solves"""
    import scipy.linalg as sla
    rng = np.random.default_rng(2)
    n, m, T, P, S = 10, 2, 40, 12, 4
    A0 = rng.standard_normal((n, n)); A = 1.3 * sla.expm(0.3 * (A0 - A0.T)); Bm = 0.5 * rng.standard_normal((n, m))
    prm = lq_params(A, Bm, 0.01 * np.eye(n), 0.001 * np.eye(m))
    lq = ddp.DeviceProblem(ddp.example_source("lq"), n, m, nparam=prm.size, params=prm)
    x0 = 0.01 * rng.standard_normal((n, P))
    u0 = 0.01 * rng.standard_normal((m, T, P))
    x0[:, [1, 6, 7]] *= 1e11                                        # |x_1| > 1e8: diverges whatever α (iLQG.jl:187)
    u0[:, :, [2, 9]] *= 1e6                                         # bounded only from a later step size on
    q = ddp.iLQG_queue(lq, x0, u0, slots=S, max_iter=5)
    st = q[6]["stats"]
    assert list(np.where(st[0] == -1)[0]) == [1, 6, 7]
    for b in (1, 6, 7):
        for a in _outputs(q)[:8]:
            assert not a[..., b].any(), b
    for sel in _batches(P, S):
        r = ddp.iLQG(lq, x0[:, sel], u0[:, :, sel], max_iter=5, timing=False)
        for a, b in zip(_outputs(q), _outputs(r)):
            assert _same(a[..., sel], b), sel[0]


def test_mpc_user_pendulum_without_plant_equals_the_host_loop(ddp, pend):
    """5 receding-horizon steps of 6 user pendulums (own damping and goal) on the device against the loop driven from the host (iLQG,
    apply u_0, x_1 as the next start, mpc_shift): closed-loop states, applied controls, every summary row and the last plan, bit for bit"""
    rng = np.random.default_rng(5)
    B, T, steps = 6, 60, 5
    x0, u0, prm = _pend_batch(rng, B, T)
    kw = dict(PEND, max_iter=25)
    xcl, ucl, scl, xp, up, git = ddp.iLQG_mpc(pend, x0, u0, steps, params=prm, **kw)
    xs, us = x0.copy(), u0.copy()
    assert _same(xcl[:, 0], x0)
    for t in range(steps):
        r = ddp.iLQG(pend, xs, us, params=prm, timing=False, **kw)
        assert _same(scl[:, t], r[6]["stats"]), t
        assert _same(xcl[:, t], r[0][:, 0]) and _same(ucl[:, t], r[1][:, 0]) and _same(xcl[:, t + 1], r[0][:, 1]), t
        xs = np.ascontiguousarray(r[0][:, 1])
        us = ddp.mpc_shift(r[1])
    assert _same(xp, r[0]) and _same(up, r[1])
    assert (scl[0] > 0).all() and (scl[1] > 1).all() and np.abs(xcl[:, -1] - xcl[:, 0]).max() > 1e-3


def car_plant_params(rng, B):
    P = np.empty((13, B))
    P[0] = 0.05                                             # h
    P[1] = 4.0 + rng.uniform(-0.5, 0.5, B); P[2] = 4.0 + rng.uniform(-0.5, 0.5, B)        # goal
    P[3] = 2.0 + rng.uniform(-0.3, 0.3, B); P[4] = 2.0 + rng.uniform(-0.3, 0.3, B)        # obstacle on the way
    P[5] = 0.6 + rng.uniform(0, 0.3, B); P[6] = rng.uniform(5.0, 20.0, B)                 # radius, weight
    P[7] = 0.1; P[8] = rng.uniform(5.0, 20.0, B)                                           # control, terminal weights
    P[9] = rng.uniform(0.6, 0.9, B); P[10] = rng.uniform(1.1, 1.4, B)                      # the plant's actuator gains
    P[11] = rng.uniform(-0.5, 0.5, B); P[12] = rng.uniform(-0.5, 0.5, B)                   # and its drift
    return P


def np_car_plant(x, u, t, p):
    """user_examples/car_plant.hip's plant in NumPy"""
    h, ua = p[0], (p[9] * u[0], p[10] * u[1])
    return np.array([x[0] + h * x[3] * np.cos(x[2]) + h * p[11], x[1] + h * x[3] * np.sin(x[2]) + h * p[12], x[2] + h * ua[1],
                     x[3] + h * ua[0]])


def test_mpc_with_a_plant(ddp):
    """8 cars, each with its own actuator-gain mismatch and drift, 5 closed-loop steps: every closed-loop state is the plant's step from
    the previous one under the applied control; every solve t is the stand-alone iLQG from the device's xcl[:,t] and the shifted
    previous plan, bit for bit; and the loop differs from the model-as-plant loop, so the plant acts"""
    rng = np.random.default_rng(6)
    n, m, N, B, steps = 4, 2, 40, 8, 5
    prm = car_plant_params(rng, B)
    x0 = np.zeros((n, B)); x0[:2] = rng.uniform(0, 0.5, (2, B)); x0[2] = np.pi / 4 + rng.uniform(-0.2, 0.2, B)
    u0 = 0.1 * rng.standard_normal((m, N, B))
    kw = dict(max_iter=30, lims=np.array([[-2.0, 2.0], [-1.5, 1.5]]))
    src = ddp.example_source("car_plant")
    car = ddp.DeviceProblem(src, n, m, nparam=13, terminal=True, plant=True)
    xcl, ucl, scl, xp, up, git = ddp.iLQG_mpc(car, x0, u0, steps, params=prm, **kw)
    assert ddp.default_handle().last_kernel(4) == "ddp_user_plant"
    assert (scl[0] > 0).all(), scl[0]
    assert _same(xcl[:, 0], x0)
    for t in range(steps):
        for b in range(B):
            ref = np_car_plant(xcl[:, t, b], ucl[:, t, b], t, prm[:, b])
            assert relerr(xcl[:, t + 1, b], ref) < 1e-12, (t, b)
    us = u0.copy()
    for t in range(steps):
        r = ddp.iLQG(car, np.ascontiguousarray(xcl[:, t]), us, params=prm, timing=False, **kw)
        assert _same(scl[:, t], r[6]["stats"]), t
        assert _same(xcl[:, t], r[0][:, 0]) and _same(ucl[:, t], r[1][:, 0]), t
        us = ddp.mpc_shift(r[1])
    assert _same(xp, r[0]) and _same(up, r[1])
    model = ddp.DeviceProblem(src, n, m, nparam=13, terminal=True)
    xm = ddp.iLQG_mpc(model, x0, u0, steps, params=prm, **kw)[0]
    assert _same(xm[:, 0], xcl[:, 0])
    assert np.abs(xm[:, 1:] - xcl[:, 1:]).max() > 1e-3
