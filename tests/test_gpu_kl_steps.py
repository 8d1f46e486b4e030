"""One kl_step per trajectory in kl.iLQGkl (ddp_kl_set_steps) on the GPU, on the smallest KL fixture shape (an LQProblem, n = 4, m = 2,
T = 20, B = 3; tests/kl_steps_cases.py): equal steps give the bits of the scalar call, distinct steps make every trajectory run as it
does in the scalar call with its own step, the DDP_KL_HOSTLOOP=1 loop (a fresh child process) agrees with the device loop, the table
is cleared on every way out of a call, a table of another B is refused by name, and the user loops (a DeviceProblem on fitted tables
with a cost model) read the table as well."""
import os
import subprocess
import sys

import numpy as np
import pytest

import kl_steps_cases as kc
from conftest import ROOT, relerr
from test_gpu_user_problem import lq_params

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ddp():
    import ddp_amd
    import ddp_amd.kl  # noqa: F401
    ddp_amd.default_handle()
    return ddp_amd


@pytest.fixture(scope="module")
def case():
    return kc.lq_case()


@pytest.fixture(scope="module")
def scalar(ddp, case):
    """the same-B scalar calls at every step of kc.STEPS, each computed once"""
    return {s: kc.flat(kc.run(ddp, case, s)) for s in kc.STEPS}


@pytest.fixture(scope="module")
def mixed(ddp, case):
    return kc.flat(kc.run(ddp, case, np.array(kc.STEPS)))


def test_equal_steps_give_the_bits_of_the_scalar_call(ddp, case, scalar):
    s = kc.STEPS[0]
    vec = kc.flat(kc.run(ddp, case, [s, s, s]))
    assert set(vec) == set(scalar[s]) and {"x", "u", "K", "S", "trace_status", "trace_η", "trace_divergence"} <= set(vec)
    for k in vec:
        assert np.array_equal(vec[k], scalar[s][k]), k


def test_distinct_steps_run_every_trajectory_with_its_own(ddp, case, scalar, mixed):
    B = case["B"]
    for s in kc.STEPS:                                           # first: the scalar calls end with status 1
        assert list(scalar[s]["trace_status"]) == [1] * B, (s, scalar[s]["trace_status"])
    assert len(set(kc.STEPS)) == B
    assert list(mixed["trace_status"]) == [1] * B
    bits = True
    for b, s in enumerate(kc.STEPS):
        dv = mixed["trace_divergence"][b]
        print("trajectory %d: kl_step %g, divergence %.6g, iterations %d" % (b, s, dv, mixed["trace_iter"][b]))
        assert abs(dv - s) < 0.1 * s
        ref = scalar[s]
        assert mixed["trace_status"][b] == ref["trace_status"][b] and mixed["trace_iter"][b] == ref["trace_iter"][b]
        assert mixed["trace_n_backpass"][b] == ref["trace_n_backpass"][b]
        for k in ("x", "u", "K"):
            assert relerr(mixed[k][..., b], ref[k][..., b]) < 1e-12, (b, k)
            bits = bits and np.array_equal(mixed[k][..., b], ref[k][..., b])
    print("x, u, K of every trajectory are %s to the scalar calls" % ("bit-equal" if bits else "NOT bit-equal (within 1e-12)"))
    # the steps really differ in their effect
    assert len({float(mixed["trace_η"][1, b]) for b in range(B)}) == B


def test_host_loop_in_a_child_process_agrees(ddp, case, mixed, tmp_path):
    out = str(tmp_path / "hostloop.npz")
    env = dict(os.environ, DDP_KL_HOSTLOOP="1")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "kl_steps_cases.py"), out], env=env, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    with np.load(out) as z:
        host = {k: z[k] for k in z.files}
    for k in ("trace_status", "trace_iter", "trace_n_backpass"):
        assert np.array_equal(mixed[k], host[k]), k
    for k in ("x", "u", "K", "S", "Si", "Vx", "Vxx", "cost", "trace_η"):
        assert relerr(mixed[k], host[k]) < 1e-12, (k, relerr(mixed[k], host[k]))
    for b, s in enumerate(kc.STEPS):
        assert abs(host["trace_divergence"][b] - s) < 0.1 * s


def test_the_table_is_cleared_when_a_vector_call_returns_or_raises(ddp, case, scalar):
    s = kc.STEPS[0]
    kc.run(ddp, case, np.array(kc.STEPS)[::-1].copy())
    after = kc.flat(kc.run(ddp, case, s))
    for k in after:
        assert np.array_equal(after[k], scalar[s][k]), ("after a vector call", k)
    with pytest.raises(ddp.DDPError, match="max_iter"):
        kc.run(ddp, case, np.array(kc.STEPS)[::-1].copy(), max_iter=0)           # refused by the library, with the table set
    after = kc.flat(kc.run(ddp, case, s))
    for k in after:
        assert np.array_equal(after[k], scalar[s][k]), ("after a vector call that raised", k)


def test_a_table_of_another_batch_size_is_refused_by_name(ddp, case, scalar, mixed):
    h, L = ddp.default_handle(), ddp._lib.lib()
    steps = np.full(case["B"] + 1, 1e-4)
    ddp._lib.check(L.ddp_kl_set_steps_f64(h.raw, steps.size, ddp._lib.ptr(steps)))
    try:
        with pytest.raises(ddp.DDPError, match=r"B = 3, the table of ddp_kl_set_steps holds 4 steps"):
            kc.run(ddp, case, kc.STEPS[0])
    finally:
        ddp._lib.check(L.ddp_kl_set_steps_f64(h.raw, 0, None))
    # the _dev flavour takes a device array and refuses a value that is not finite by name
    bad = h.to_device(np.array([1e-4, np.inf, 1e-4]))
    try:
        assert L.ddp_kl_set_steps_f64_dev(h.raw, 3, bad) == -1
        assert "steps[1]" in L.ddp_last_error().decode() and "not finite" in L.ddp_last_error().decode()
        good = h.to_device(np.array(kc.STEPS))
        try:
            ddp._lib.check(L.ddp_kl_set_steps_f64_dev(h.raw, 3, good))
            vec = kc.flat(kc.run(ddp, case, 123.0))                  # the table, not the scalar of the call, is what the loop reads
        finally:
            ddp._lib.check(L.ddp_kl_set_steps_f64_dev(h.raw, 0, None))
            h.free(good)
    finally:
        h.free(bad)
    assert list(vec["trace_status"]) == [1] * case["B"]
    for k in ("x", "u", "K", "trace_divergence"):
        assert np.array_equal(vec[k], mixed[k]), k                   # the bits of the call with the keyword
    after = kc.flat(kc.run(ddp, case, kc.STEPS[0]))
    assert np.array_equal(after["x"], scalar[kc.STEPS[0]]["x"])


def test_user_loop_on_fitted_tables_with_a_cost_model_reads_the_table(ddp):
    """the lq example as a DeviceProblem made with fitted=True, planning on tables with cost_model=: B = 2, two steps"""
    rng = np.random.default_rng(41)
    n, m, N, B, h = 4, 2, 12, 2, 0.05
    A = np.eye(n) + h * rng.standard_normal((n, n)); Bm = h * rng.standard_normal((n, m))
    Q, R = h * np.eye(n), 0.1 * h * np.eye(m)
    prob = ddp.DeviceProblem(ddp.example_source("lq"), n, m, nparam=2 * n * n + n * m + m * m, params=lq_params(A, Bm, Q, R), fitted=True)
    F = np.asfortranarray
    fx, fu = F(np.repeat(np.repeat(A[:, :, None, None], N, 2), B, 3)), F(np.repeat(np.repeat(Bm[:, :, None, None], N, 2), B, 3))
    fc = F(0.01 * rng.standard_normal((n, N, B)))
    u0 = F(0.2 * rng.standard_normal((m, N, B)) * np.array([1.0, 2.0]))
    x, _, c = ddp.forward_pass(None, 1.0 + 0.1 * rng.standard_normal((n, B)), u0, None, 1.0, prob, None, model=(fx, fu, fc))
    x, c = F(x.reshape(n, N, B)), c.reshape(-1, B)
    cm = ddp.df(prob, x, u0)[5:10]
    eye = np.repeat(np.repeat(np.eye(m)[:, :, None, None], N, 2), B, 3)
    model = ddp.kl.Model(fx, fu, 1e-4 * np.eye(n), fc)

    def run(kl_step):
        prev = ddp.GaussianPolicy(N, n, m, np.zeros((m, n, N, B)), u0.copy(), eye, eye.copy())
        return kc.flat(ddp.kl.iLQGkl(prob, x, prev, model, kl_step=kl_step, max_iter=40, cost=c, fitted=True, cost_model=cm))

    steps = (1e-3, 3e-3)
    ref = {s: run(s) for s in steps}
    vec = run(np.array(steps))
    assert ddp.default_handle().last_kernel(1) == "ddp_user_rollout_fit"
    for b, s in enumerate(steps):
        print("trajectory %d: kl_step %g, status %d, divergence %.6g, iterations %d" % (b, s, vec["trace_status"][b], vec["trace_divergence"][b], vec["trace_iter"][b]))
        for k in ("trace_status", "trace_iter", "trace_n_backpass"):
            assert vec[k][b] == ref[s][k][b], (b, k)
        for k in ("x", "u", "K"):
            assert relerr(vec[k][..., b], ref[s][k][..., b]) < 1e-12, (b, k)
        if vec["trace_status"][b] == 1:
            assert abs(vec["trace_divergence"][b] - s) < 0.1 * s
    assert list(vec["trace_status"]) == [1, 1]
    assert not np.array_equal(ref[steps[0]]["x"][..., 1], ref[steps[1]]["x"][..., 1])      # the step matters for this trajectory
