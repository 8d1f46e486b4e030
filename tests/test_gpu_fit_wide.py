"""fit_dynamics(..., wide=True) on the GPU against the long double reference of tests/fit_reference.py on the cases of
tests/fit_wide_cases.py.  Tolerance: 1e-8 (fit_reference.TOL, the project's parity tolerance) on the three relative errors of
fit_reference.errors; every designed input has kappa(A) <= 500 at the steps that are expected to succeed (tests/test_fit_wide_cpu.py),
which keeps the first-order bound d (S + d) kappa 2^-53 under that tolerance.  Every device result and every reference is computed once
and shared; nothing is written into a shared array."""
import functools

import numpy as np
import pytest

import ddp_amd
from ddp_amd import _lib, kl

import fit_reference as fr
import fit_wide_cases as fw
import sample_wave_cases as wc

pytestmark = pytest.mark.gpu
TOL = fr.TOL


def same(a, b):
    return all(np.array_equal(x, y, equal_nan=True) for x, y in zip(a, b))


@functools.lru_cache(maxsize=None)
def device(name):
    c = fw.case(name)
    return ddp_amd.fit_dynamics(c["xs"], c["us"], ridge=c["ridge"], prior=c["prior"], wide=True)


def check(got, ref, N, what):
    """status equal everywhere; the three errors under TOL at the steps where the reference succeeded; NaN where it failed; slot N - 1
    zeros; cov symmetric to the bit"""
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
        assert np.all(np.isnan(a[:, :, bad])) and np.all(np.isfinite(a[:, :, ~bad]))
    assert np.all(np.isnan(fc[:, bad])) and np.all(np.isfinite(fc[:, ~bad]))
    for a in (fx[:, :, N - 1], fu[:, :, N - 1], fc[:, N - 1], cov[:, :, N - 1], status[N - 1]):
        assert not np.any(a)
    assert np.array_equal(cov, np.swapaxes(cov, 0, 1), equal_nan=True)


# ------------------------------------------------------------------------------------------------------------ 1. against the reference
@pytest.mark.parametrize("name", sorted(fw.CASES))
def test_designed_cases_match_the_long_double_reference(name):
    c = fw.case(name)
    got = device(name)
    n, m, N, B = c["n"], c["m"], c["N"], c["B"]
    assert [a.shape for a in got] == [(n, n, N, B), (n, m, N, B), (n, N, B), (n, n, N, B), (N, B)] and got[4].dtype == np.int32
    assert all(a.dtype == np.float64 for a in got[:4])
    check(got, c["ref"], N, name)


def test_unbatched_arrays_drop_the_batch_axis():
    c = fw.case("33x8")
    one = ddp_amd.fit_dynamics(c["xs"][..., 1], c["us"][..., 1], wide=True)
    assert [a.shape for a in one] == [(33, 33, 3), (33, 8, 3), (33, 3), (33, 33, 3), (3,)]
    assert same(one, [a[..., 1] for a in device("33x8")])


def test_ridge_is_added_to_the_diagonal():
    c = fw.case("64x32")
    got = ddp_amd.fit_dynamics(c["xs"], c["us"], ridge=2.5, wide=True)
    check(got, fw.ridge_reference("64x32", 2.5), c["N"], "64x32 ridge 2.5")
    assert not same(got[:1], device("64x32")[:1])


# ------------------------------------------------------------------------------------------------------------------------- 2. status
@pytest.mark.parametrize("name", sorted(fw.STATUS_CASES))
def test_status_cases(name):
    c = fw.STATUS_CASES[name]()
    got = ddp_amd.fit_dynamics(c["xs"], c["us"], wide=True)
    assert np.array_equal(got[4], c["expect"]), (name, got[4].T)
    reads = c["expect"] != 0
    for a in got[:4]:
        finite = np.isfinite(a).all(axis=tuple(range(a.ndim - 2)))
        assert np.array_equal(~finite, reads), (name, finite.T)
    check(got, c["ref"], c["N"], name)


# --------------------------------------------------------------------------------------------------------------------------- 3. bits
BITS = ["40x25", "64x32-prior-S2", "33x8"]


@pytest.mark.parametrize("name", BITS)
def test_two_calls_and_trajectory_slices_give_the_same_bits(name):
    c = fw.case(name)
    full = device(name)
    again = ddp_amd.fit_dynamics(c["xs"], c["us"], ridge=c["ridge"], prior=c["prior"], wide=True)
    assert same(again, full)
    for b in range(c["B"]):
        pr = c["prior"]
        if pr is not None and pr[0].ndim == 4:
            pr = (pr[0][..., b:b + 1], pr[1][..., b:b + 1], pr[2], pr[3])
        one = ddp_amd.fit_dynamics(c["xs"][..., b:b + 1], c["us"][..., b:b + 1], ridge=c["ridge"], prior=pr, wide=True)
        assert same(one, [a[..., b:b + 1] for a in full]), (name, b)


@pytest.mark.parametrize("name", BITS)
def test_device_pointer_entry_gives_the_bits_of_the_host_pointer_entry(name):
    c = fw.case(name)
    n, m, N, S, B = c["n"], c["m"], c["N"], c["S"], c["B"]
    h = ddp_amd.default_handle()
    pr = c["prior"]
    bufs = [h.to_device(c["xs"]), h.to_device(c["us"])] + ([h.to_device(pr[0]), h.to_device(pr[1])] if pr else [None, None])
    shapes = [(n, n, N, B), (n, m, N, B), (n, N, B), (n, n, N, B)]
    outs = [h.malloc(8 * int(np.prod(s))) for s in shapes] + [h.malloc(4 * N * B)]
    try:
        _lib.check(_lib.lib().ddp_fit_dynamics_wide_f64_dev(h.raw, n, m, N, S, B, bufs[0], bufs[1], c["ridge"], bufs[2], bufs[3], pr[2] if pr else 0.0,
                                                            pr[3] if pr else 0.0, int(pr is not None and pr[0].ndim == 4), *outs))
        h.sync()
        got = [h.to_host(p, s) for p, s in zip(outs, shapes)] + [h.to_host(outs[4], (N, B), dtype=np.int32)]
    finally:
        for p in bufs + outs:
            if p is not None:
                h.free(p)
    assert same(got, device(name))


@pytest.mark.parametrize("name", ["4x2", "32x8"])
def test_a_shape_inside_the_small_box_keeps_its_kernel_and_its_bits(name):
    c = fr.case(name)
    narrow = ddp_amd.fit_dynamics(c["xs"], c["us"], ridge=c["ridge"], prior=c["prior"])
    wide = ddp_amd.fit_dynamics(c["xs"], c["us"], ridge=c["ridge"], prior=c["prior"], wide=True)
    assert same(wide, narrow)


# ------------------------------------------------------------------------------------------------------------ 4. through the sampler
def test_samples_of_the_wave_sampler_at_the_corner():
    """chain_plant_ad at (64, 32) through sample_policy(plant=True) of a wave=True, sample_wave=True problem, N = 5, B = 2, S = 8 < d.
    ridge = lambda_max / 200 with lambda_max the largest eigenvalue of the sample covariances of z over all steps and trajectories (float64
    NumPy, from the downloaded samples): kappa(A) <= 201 at every step by construction.  The device fit of those samples against the
    reference on the same samples, and the model it gives to forward_covariance(..., wide=True)."""
    c = wc.case("chain_plant_64x32")
    n, m, N, B, S = c["n"], c["m"], c["N"], 2, 8
    prob = ddp_amd.DeviceProblem(ddp_amd.example_source(c["example"]), n, m, nparam=c["nparam"], wave=True, sample_wave=True, **c["kw"])
    pol = ddp_amd.GaussianPolicy(N, n, m, c["K"][..., :B], np.zeros((m, N, B)), c["Sigma"][..., :B], np.zeros((0, 0, 0)))
    xs, us, _, info = ddp_amd.sample_policy(prob, pol, c["x0"][..., :B], c["x"][..., :B], c["u"][..., :B], S, seed=c["seed"], plant=True,
                                            params=c["params"][..., :B])
    assert not np.any(info["status"]) and xs.shape == (n, N, S, B) and us.shape == (m, N, S, B)
    lam = max(np.linalg.eigvalsh(np.cov(np.concatenate([xs[:, i, :, b], us[:, i, :, b]], axis=0)))[-1] for i in range(N - 1) for b in range(B))
    ridge = lam / 200
    got = ddp_amd.fit_dynamics(xs, us, ridge=ridge, wide=True)
    ref = fr.fit(xs, us, ridge)
    assert ref["kappa"][:N - 1].max() <= 201.5
    check(got, ref, N, "chain_plant_ad (64, 32) through the wave sampler, ridge %.3g" % ridge)
    fx, fu, fc, cov, status = got
    sig = kl.forward_covariance(kl.Model(fx, fu, cov[:, :, 0, 0]), c["x"][..., :B], c["u"][..., :B], pol, wide=True)
    assert sig.shape == (n + m, n + m, N, B) and np.all(np.isfinite(sig))
