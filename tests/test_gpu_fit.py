"""fit_dynamics on the GPU against the long double reference of tests/fit_reference.py.  Tolerance: 1e-8 (BASELINE.json), for [fx fu]
relative to |[fx fu]_i|_F per step, for fc relative to |mu_y| + |F| |mu_z|, for cov relative to |C_yy|_F; every designed input has
kappa(A) <= 2e3 at the steps that are expected to succeed (tests/test_fit_cpu.py), which keeps the first-order bound
d (S + d) kappa 2^-53 under that tolerance.  Every device result is computed once and shared; nothing is written into a shared array."""
import functools

import numpy as np
import pytest

import ddp_amd
from ddp_amd import _lib

import fit_reference as fr
import sample_reference as sr

pytestmark = pytest.mark.gpu
TOL = fr.TOL


def same(a, b):
    return all(np.array_equal(x, y, equal_nan=True) for x, y in zip(a, b))


@functools.lru_cache(maxsize=None)
def device(name):
    c = fr.case(name)
    return ddp_amd.fit_dynamics(c["xs"], c["us"], ridge=c["ridge"], prior=c["prior"])


def check(got, ref, N, what):
    """status equal everywhere; the three errors under TOL at the steps where the reference succeeded; NaN where it failed; slot N - 1 zeros"""
    fx, fu, fc, cov, status = got
    assert np.array_equal(status, ref["status"]), (what, status.T, ref["status"].T)
    e = fr.errors(got, ref)
    ok = ref["status"] == 0
    ok[N - 1] = False
    if ok.any():
        worst = [float(np.max(v[ok])) for v in e]
        print("%s: [fx fu] %.2e  fc %.2e  cov %.2e   (kappa max %.1f)" % ((what,) + tuple(worst) + (ref["kappa"][ok].max(),)))
        assert max(worst) <= TOL, (what, worst)
    bad = ref["status"] != 0
    for a in (fx, fu, cov):
        assert np.all(np.isnan(a[:, :, bad]))
    assert np.all(np.isnan(fc[:, bad]))
    for a in (fx[:, :, N - 1], fu[:, :, N - 1], fc[:, N - 1], cov[:, :, N - 1], status[N - 1]):
        assert not np.any(a)


# ------------------------------------------------------------------------------------------------------------ 1. against the reference
@pytest.mark.parametrize("name", sorted(fr.CASES))
def test_designed_cases_match_the_long_double_reference(name):
    c = fr.case(name)
    got = device(name)
    n, m, N, B = c["n"], c["m"], c["N"], c["B"]
    assert [a.shape for a in got] == [(n, n, N, B), (n, m, N, B), (n, N, B), (n, n, N, B), (N, B)] and got[4].dtype == np.int32
    check(got, c["ref"], N, name)
    assert np.array_equal(got[3], np.swapaxes(got[3], 0, 1))                         # cov is symmetric to the bit


def test_unbatched_arrays_drop_the_batch_axis():
    c = fr.case("4x2")
    one = ddp_amd.fit_dynamics(c["xs"][..., 1], c["us"][..., 1])
    assert [a.shape for a in one] == [(4, 4, 7), (4, 2, 7), (4, 7), (4, 4, 7), (7,)]
    assert same(one, [a[..., 1] for a in device("4x2")])


def test_ridge_is_added_to_the_diagonal():
    c = fr.case("5x3")
    got = ddp_amd.fit_dynamics(c["xs"], c["us"], ridge=2.5)
    check(got, fr.fit(c["xs"], c["us"], 2.5), c["N"], "5x3 ridge 2.5")
    assert not same(got[:1], device("5x3")[:1])


# ------------------------------------------------------------------------------------------------------------------------- 2. status
def test_identical_columns_fail_their_step_only():
    c = fr.identical_columns_case()
    got = ddp_amd.fit_dynamics(c["xs"], c["us"])
    assert got[4][fr.FAIL_STEP, 1] == c["ref"]["status"][fr.FAIL_STEP, 1] == 2 and np.count_nonzero(got[4]) == 1
    check(got, c["ref"], c["N"], "identical columns")


@pytest.mark.parametrize("which", ["state", "control"])
def test_a_nan_fails_only_the_steps_that_read_it(which):
    c = fr.nan_case(which)
    r = c["ref"]
    got = ddp_amd.fit_dynamics(c["xs"], c["us"])
    reads = np.zeros((c["N"], c["B"]), dtype=bool)
    reads[3, 1] = True                                           # the step whose z holds it: pivot 2 (state 2) or n + 1 (control 1) fails
    reads[2, 1] = which == "state"                               # the step whose y holds it: no pivot fails, the results are not finite: d + 1
    assert np.array_equal(got[4], r["status"]) and np.array_equal(got[4] != 0, reads)
    assert got[4][3, 1] == (3 if which == "state" else 6) and got[4][2, 1] == (7 if which == "state" else 0)
    for a in got[:4]:
        finite = np.isfinite(a).all(axis=tuple(range(a.ndim - 2)))
        assert np.array_equal(~finite, reads), (which, finite.T)
    check(got, r, c["N"], "NaN in a " + which)


# --------------------------------------------------------------------------------------------------------------------------- 3. bits
@pytest.mark.parametrize("name", ["4x2", "13x4-prior", "32x8"])
def test_two_calls_and_trajectory_slices_give_the_same_bits(name):
    c = fr.case(name)
    full = device(name)
    again = ddp_amd.fit_dynamics(c["xs"], c["us"], ridge=c["ridge"], prior=c["prior"])
    assert same(again, full)
    for b in range(c["B"]):
        pr = c["prior"]
        if pr is not None and pr[0].ndim == 4:
            pr = (pr[0][..., b:b + 1], pr[1][..., b:b + 1], pr[2], pr[3])
        one = ddp_amd.fit_dynamics(c["xs"][..., b:b + 1], c["us"][..., b:b + 1], ridge=c["ridge"], prior=pr)
        assert same(one, [a[..., b:b + 1] for a in full]), (name, b)


@pytest.mark.parametrize("name", ["5x3-prior-S2", "13x4-prior", "12x4"])
def test_device_pointer_entry_gives_the_bits_of_the_host_pointer_entry(name):
    c = fr.case(name)
    n, m, N, S, B = c["n"], c["m"], c["N"], c["S"], c["B"]
    h = ddp_amd.default_handle()
    pr = c["prior"]
    bufs = [h.to_device(c["xs"]), h.to_device(c["us"])] + ([h.to_device(pr[0]), h.to_device(pr[1])] if pr else [None, None])
    shapes = [(n, n, N, B), (n, m, N, B), (n, N, B), (n, n, N, B)]
    outs = [h.malloc(8 * int(np.prod(s))) for s in shapes] + [h.malloc(4 * N * B)]
    try:
        _lib.check(_lib.lib().ddp_fit_dynamics_f64_dev(h.raw, n, m, N, S, B, bufs[0], bufs[1], c["ridge"], bufs[2], bufs[3], pr[2] if pr else 0.0,
                                                       pr[3] if pr else 0.0, int(pr is not None and pr[0].ndim == 4), *outs))
        h.sync()
        got = [h.to_host(p, s) for p, s in zip(outs, shapes)] + [h.to_host(outs[4], (N, B), dtype=np.int32)]
    finally:
        for p in bufs + outs:
            if p is not None:
                h.free(p)
    assert same(got, device(name))


# ------------------------------------------------------------------------------------------------------------ 4. through the sampler
@functools.lru_cache(maxsize=None)
def sampled():
    """sample_policy on lq_ad with the seed of tests/sample_reference.py"""
    c = sr.case("lq_ad")
    prob = ddp_amd.DeviceProblem(ddp_amd.example_source(c["example"]), c["n"], c["m"], nparam=c["nparam"], sample=True, **c["kw"])
    pol = ddp_amd.GaussianPolicy(c["N"], c["n"], c["m"], c["K"], np.zeros((c["m"], c["N"], c["B"])), c["Sigma"], np.zeros((0, 0, 0)))
    xs, us, _, info = ddp_amd.sample_policy(prob, pol, c["x0"], c["x"], c["u"], c["S"], seed=c["seed"], params=c["params"])
    assert not np.any(info["status"])
    return xs, us


def test_sampler_rollouts_with_the_ridge_match_the_reference_on_its_own_samples():
    s = fr.sampler_case()
    xs, us = sampled()
    got = ddp_amd.fit_dynamics(xs, us, ridge=fr.SAMPLER_RIDGE)
    check(got, s["ref"], s["case"]["N"], "lq_ad through the sampler, ridge %g" % fr.SAMPLER_RIDGE)


def test_sampler_rollouts_without_ridge_report_step_0_and_recover_the_model():
    s = fr.sampler_case()
    c, r0 = s["case"], s["ref0"]
    n, m, N, S, B = c["n"], c["m"], c["N"], c["S"], c["B"]
    xs, us = sampled()
    fx, fu, fc, cov, status = ddp_amd.fit_dynamics(xs, us)
    assert np.all(status[0] == 1) and np.all(np.isnan(fx[:, :, 0])) and np.all(np.isnan(fc[:, 0]))      # C_xx of step 0 is exactly zero
    assert np.all(status[N - 4:] == 0)
    for b in range(B):
        for i in range(N - 4, N - 1):
            bound = max(TOL, (n + m) * (S + n + m) * r0["kappa"][i, b] * 2.0 ** -53)
            F = np.concatenate([fx[:, :, i, b], fu[:, :, i, b]], axis=1)
            err = np.linalg.norm(F - s["AB"][..., b]) / np.linalg.norm(s["AB"][..., b])
            mu_z = np.concatenate([xs[:, i, :, b].mean(axis=1), us[:, i, :, b].mean(axis=1)])
            efc = np.linalg.norm(fc[:, i, b]) / (np.linalg.norm(xs[:, i + 1, :, b].mean(axis=1)) + np.linalg.norm(F) * np.linalg.norm(mu_z))
            print("step %d trajectory %d: [fx fu] - [A B] %.2e, fc %.2e, kappa %.3g" % (i, b, err, efc, r0["kappa"][i, b]))
            assert err <= bound and efc <= bound
