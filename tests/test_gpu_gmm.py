"""fit_gmm and gmm_prior on the GPU against the long double reference of tests/gmm_reference.py.  Tolerance 1e-8: relative in the Frobenius
norm per Sigma_k and Phi slot and in the norm per mu_k and mu0 slot, absolute for pi, relative for ll.  Every designed input keeps
kappa(Sigma_k) <= 2e3 and pi_k >= 0.02 at every iteration, and the reference in float64 within 1e-10 of itself in long double
(tests/test_gmm_cpu.py).  Every device result is computed once and shared; nothing is written into a shared array.

Worst errors measured on an MI355X over the designed cases: see DESIGN.md, "GMM dynamics prior"."""
import functools

import numpy as np
import pytest

import ddp_amd
from ddp_amd import _lib

import fit_reference as fr
import gmm_reference as gr
import sample_reference as sr

pytestmark = pytest.mark.gpu
TOL = gr.TOL
FIELDS = ("pi", "mu", "Sigma", "ll", "status")


def bits(g):
    return [getattr(g, k) for k in FIELDS]


def same(a, b):
    return all(np.array_equal(x, y, equal_nan=True) for x, y in zip(a, b))


def as_gmm(ref):
    """the reference mixture rounded to double, as an input of gmm_prior"""
    return ddp_amd.GMM(*(np.asfortranarray(ref[k].astype(np.float64)) for k in FIELDS[:4]), ref["status"], ref["pool"])


@functools.lru_cache(maxsize=None)
def device(name):
    c = gr.case(name)
    return ddp_amd.fit_gmm(c["xs"], c["us"], **c["kw"])


@functools.lru_cache(maxsize=None)
def device_prior(name):
    c = gr.case(name)
    return ddp_amd.gmm_prior(as_gmm(c["ref"]), c["xs"], c["us"], m0=c["m0"], n0=c["n0"])


# ------------------------------------------------------------------------------------------------------------ 1. against the reference
@pytest.mark.parametrize("name", sorted(gr.CASES))
def test_designed_cases_match_the_long_double_reference(name):
    c, got = gr.case(name), device(name)
    r = c["ref"]
    p, (K, G), iters = 2 * c["n"] + c["m"], r["pi"].shape, c["kw"]["iters"]
    assert [a.shape for a in bits(got)] == [(K, G), (p, K, G), (p, p, K, G), (iters, G), (G,)] and got.status.dtype == np.int32
    assert not np.any(got.status) and got.pool == r["pool"]
    e = gr.errors(dict(pi=got.pi, mu=got.mu, Sigma=got.Sigma, ll=got.ll), r)
    print("%s: Sigma %.2e  mu %.2e  pi %.2e  ll %.2e   (kappa max %.1f, pi min %.3f)" % (name, e["Sigma"], e["mu"], e["pi"], e["ll"], r["kappa_max"], r["pi_min"]))
    assert max(e.values()) <= TOL, e
    assert np.array_equal(got.Sigma, np.swapaxes(got.Sigma, 0, 1))                   # symmetric to the bit


@pytest.mark.parametrize("name", sorted(gr.CASES))
def test_prior_matches_the_long_double_reference(name):
    c = gr.case(name)
    Phi, mu0, m0, n0 = device_prior(name)
    p, N, B = 2 * c["n"] + c["m"], c["N"], c["B"]
    assert Phi.shape == (p, p, N, B) and mu0.shape == (p, N, B) and (m0, n0) == (c["m0"], c["n0"])
    e = gr.prior_errors(Phi, mu0, c)
    print("%s: Phi %.2e  mu0 %.2e" % (name, e["Phi"], e["mu0"]))
    assert max(e.values()) <= TOL, e
    assert np.array_equal(Phi, np.swapaxes(Phi, 0, 1)) and not np.any(Phi[:, :, N - 1]) and not np.any(mu0[:, N - 1])


def test_the_philox_assignment_alone():
    """iters = 0 without init is one M-step from the hard assignment: a wrong counter layout moves points between clusters, which pi shows
    in multiples of 1 / P"""
    for name in ("p3_k32_hard", "p17_hard"):
        c, got = gr.case(name), device(name)
        assert c["kw"]["iters"] == 0 and c["kw"]["init"] is None and got.ll.shape[0] == 0
        P = (c["N"] - 1) * c["S"] * (c["B"] if c["kw"]["pool"] else 1)
        assert np.array_equal(np.rint(got.pi * P), np.rint(c["ref"]["pi"].astype(np.float64) * P))
        assert np.max(np.abs(got.pi * P - np.rint(got.pi * P))) <= 1e-9


def test_zero_iterations_from_an_init_return_the_init():
    c = gr.case("p10_k5_init")
    got = ddp_amd.fit_gmm(c["xs"], c["us"], **{**c["kw"], "iters": 0})
    assert same([got.pi, got.mu, got.Sigma], c["kw"]["init"]) and not np.any(got.status) and got.ll.shape == (0, c["B"])
    again = ddp_amd.fit_gmm(c["xs"], c["us"], **{**c["kw"], "init": got})              # a GMM is an init
    assert same(bits(again), bits(device("p10_k5_init")))


def test_unbatched_arrays_are_one_trajectory():
    c = gr.case("p10_k2")
    assert c["B"] == 1
    one = ddp_amd.fit_gmm(c["xs"][..., 0], c["us"][..., 0], **c["kw"])
    assert same(bits(one), bits(device("p10_k2")))
    Phi, mu0, _, _ = ddp_amd.gmm_prior(as_gmm(c["ref"]), c["xs"][..., 0], c["us"][..., 0], m0=c["m0"], n0=c["n0"])
    assert Phi.shape == (10, 10, c["N"]) and same([Phi, mu0], [a[..., 0] for a in device_prior("p10_k2")[:2]])


# --------------------------------------------------------------------------------------------------------------------------- 2. bits
@pytest.mark.parametrize("name", ["p3_k32_init", "p17_k2", "p72_k2"])
def test_two_calls_give_the_same_bits(name):
    c = gr.case(name)
    assert same(bits(ddp_amd.fit_gmm(c["xs"], c["us"], **c["kw"])), bits(device(name)))
    assert same(ddp_amd.gmm_prior(as_gmm(c["ref"]), c["xs"], c["us"], m0=c["m0"], n0=c["n0"])[:2], device_prior(name)[:2])


@pytest.mark.parametrize("name", ["p10_k5", "p10_k5_init", "p17_hard", "p72_k1_b"])
def test_one_mixture_per_trajectory_is_sliceable(name):
    c, full = gr.case(name), device(name)
    assert not c["kw"]["pool"]
    for b in range(c["B"]):
        kw = dict(c["kw"])
        if kw["init"] is not None:
            kw["init"] = tuple(np.asfortranarray(a[..., b:b + 1]) for a in kw["init"])
        one = ddp_amd.fit_gmm(c["xs"][..., b:b + 1], c["us"][..., b:b + 1], traj0=b, **kw)
        assert same(bits(one), [a[..., b:b + 1] for a in bits(full)]), (name, b)


@pytest.mark.parametrize("name", ["p10_k5", "p17_k2", "p33_k5_init"])
def test_prior_is_sliceable_in_both_modes(name):
    c, full = gr.case(name), device_prior(name)
    g = as_gmm(c["ref"])
    for b in range(c["B"]):
        gb = g if g.pool else ddp_amd.GMM(*(np.asfortranarray(a[..., b:b + 1]) for a in bits(g)[:4]), g.status[b:b + 1], False)
        one = ddp_amd.gmm_prior(gb, c["xs"][..., b:b + 1], c["us"][..., b:b + 1], m0=c["m0"], n0=c["n0"])
        assert same(one[:2], [a[..., b:b + 1] for a in full[:2]]), (name, b)


@pytest.mark.parametrize("name", ["p10_k5_init", "p17_k2"])
def test_device_pointer_entries_give_the_bits_of_the_host_pointer_entries(name):
    c = gr.case(name)
    n, m, N, S, B, kw = c["n"], c["m"], c["N"], c["S"], c["B"], c["kw"]
    p, K, G, iters = 2 * n + m, kw["K"], 1 if kw["pool"] else B, kw["iters"]
    h = ddp_amd.default_handle()
    g = as_gmm(c["ref"])
    ins = [h.to_device(c["xs"]), h.to_device(c["us"])] + [h.to_device(a) if kw["init"] else None for a in (kw["init"] or (None,) * 3)]
    mix = [h.to_device(a) for a in (g.pi, g.mu, g.Sigma)]
    shapes = [(K, G), (p, K, G), (p, p, K, G), (iters, G)]
    outs = [h.malloc(8 * int(np.prod(s))) for s in shapes] + [h.malloc(4 * G)]
    pshapes = [(p, p, N, B), (p, N, B)]
    pouts = [h.malloc(8 * int(np.prod(s))) for s in pshapes] + [h.malloc(4 * N * B)]
    try:
        _lib.check(_lib.lib().ddp_gmm_fit_f64_dev(h.raw, n, m, N, S, B, K, iters, int(kw["pool"]), 0, ins[0], ins[1], kw["reg"], gr.SEED & 0xffffffff,
                                                  gr.SEED >> 32, ins[2], ins[3], ins[4], *outs))
        h.sync()
        got = [h.to_host(q, s) for q, s in zip(outs, shapes)] + [h.to_host(outs[4], (G,), dtype=np.int32)]
        _lib.check(_lib.lib().ddp_gmm_prior_f64_dev(h.raw, n, m, N, S, B, K, int(kw["pool"]), ins[0], ins[1], *mix, c["m0"], c["n0"], *pouts))
        h.sync()
        pgot = [h.to_host(q, s) for q, s in zip(pouts, pshapes)] + [h.to_host(pouts[2], (N, B), dtype=np.int32)]
    finally:
        for q in ins + mix + outs + pouts:
            if q is not None:
                h.free(q)
    assert same(got, bits(device(name)))
    assert same(pgot[:2], device_prior(name)[:2]) and not np.any(pgot[2])


# ------------------------------------------------------------------------------------------------------------------------- 3. status
def test_an_emptied_cluster_fails_its_mixture_only():
    c = gr.empty_cluster_case()
    r = c["ref"]
    got = ddp_amd.fit_gmm(c["xs"], c["us"], **c["kw"])
    assert list(got.status) == list(r["status"]) == [0, 2]
    for a in (got.pi[:, 1], got.mu[..., 1], got.Sigma[..., 1], got.ll[1:, 1]):
        assert np.all(np.isnan(a))
    assert abs(got.ll[0, 1] - float(r["ll"][0, 1])) <= TOL * abs(float(r["ll"][0, 1]))
    solo = ddp_amd.fit_gmm(c["xs"][..., :1], c["us"][..., :1], **{**c["kw"], "init": tuple(np.asfortranarray(a[..., :1]) for a in c["kw"]["init"])})
    assert same(bits(solo), [a[..., :1] for a in bits(got)])
    e = gr.errors(dict(pi=solo.pi, mu=solo.mu, Sigma=solo.Sigma, ll=solo.ll), {k: r[k][..., :1] for k in FIELDS[:4]})
    assert max(e.values()) <= TOL, e
    # the failed mixture as an input of gmm_prior: status 2 on its trajectory, nothing else
    Phi, mu0, _, _ = ddp_amd.gmm_prior(got, c["xs"], c["us"])
    st = _prior_status(got, c["xs"], c["us"])
    assert np.all(st[:-1, 1] == 2) and not np.any(st[:, 0]) and st[-1, 1] == 0
    assert np.all(np.isnan(Phi[:, :, :-1, 1])) and np.all(np.isnan(mu0[:, :-1, 1])) and np.all(np.isfinite(Phi[..., 0])) and not np.any(Phi[:, :, -1])


def _prior_status(g, xs, us, m0=1.0, n0=1.0):
    """status[N,B] of gmm_prior, which the Python function does not return: the host-pointer entry"""
    n, N, S, B = xs.shape
    m = us.shape[0]
    p, K = 2 * n + m, g.pi.shape[0]
    Phi, mu0, st = np.zeros((p, p, N, B), order="F"), np.zeros((p, N, B), order="F"), np.full((N, B), -1, dtype=np.int32, order="F")
    _lib.check(_lib.lib().ddp_gmm_prior_f64(ddp_amd.default_handle().raw, n, m, N, S, B, K, int(g.pool), _lib.ptr(_lib.f64(xs)), _lib.ptr(_lib.f64(us)),
                                            _lib.ptr(_lib.f64(g.pi)), _lib.ptr(_lib.f64(g.mu)), _lib.ptr(_lib.f64(g.Sigma)), m0, n0, _lib.ptr(Phi),
                                            _lib.ptr(mu0), st.ctypes.data_as(_lib.vp)))
    return st


def test_a_nan_fails_only_the_two_steps_that_contain_it():
    c = gr.nan_point_case()
    g = as_gmm(c["ref"])
    Phi, mu0, _, _ = ddp_amd.gmm_prior(g, c["xs"], c["us"], m0=c["m0"], n0=c["n0"])
    st = _prior_status(g, c["xs"], c["us"], c["m0"], c["n0"])
    assert np.array_equal(st, c["pstatus"]) and st[1, 1] == 1 and st[2, 1] == 1 and np.count_nonzero(st) == 2
    bad = st != 0
    assert np.all(np.isnan(Phi[:, :, bad])) and np.all(np.isnan(mu0[:, bad]))
    clean = device_prior("p10_k5_init")
    assert np.array_equal(Phi[:, :, ~bad], clean[0][:, :, ~bad]) and np.array_equal(mu0[:, ~bad], clean[1][:, ~bad])


# ------------------------------------------------------------------------------------------------------------ 4. through the sampler
# With S = 6 < n + m + 1 the centred Gram matrix of a step has rank 5 < n + m: in exact arithmetic pivot 6 of every step is zero.  In double
# it is rounding noise of either sign, and a step whose pivots 6, 7 and 8 all round to tiny positive numbers passes the pivot test with
# meaningless tables: measured on an MI355X, 1 to 7 of the 108 steps with each of the sampler seeds 1 .. 10 and 12, and 1 with the seed of
# tests/sample_reference.py.  Seed 11 is the first of 1, 2, 3, ... for which fit_dynamics alone rejects every step, which is the premise
# this test states; the sampler and the fit are deterministic, so it holds on every run.
E2E_SEED = 11


def test_round_with_fewer_samples_than_regressors():
    """lq_ad (n = 5, m = 3) through sample_policy with S = 6 < n + m + 1: fit_dynamics alone rejects every step; with the GMM prior every
    step is fitted, and the tables agree with the long double pipeline (GMM, prior, fit) on the same samples"""
    c = sr.case("lq_ad")
    n, m, N, B, S, K = c["n"], c["m"], c["N"], c["B"], 6, 3
    prob = ddp_amd.DeviceProblem(ddp_amd.example_source(c["example"]), n, m, nparam=c["nparam"], sample=True, **c["kw"])
    pol = ddp_amd.GaussianPolicy(N, n, m, c["K"], np.zeros((m, N, B)), c["Sigma"], np.zeros((0, 0, 0)))
    xs, us, _, info = ddp_amd.sample_policy(prob, pol, c["x0"], c["x"], c["u"], S, seed=E2E_SEED, params=c["params"])
    assert not np.any(info["status"])
    alone = ddp_amd.fit_dynamics(xs, us)
    print("fit_dynamics alone: %d of %d steps pass the pivot test %s" % (np.count_nonzero(alone[4][:N - 1] == 0), (N - 1) * B,
                                                                         np.argwhere(alone[4][:N - 1] == 0).tolist()))
    assert np.all(alone[4][:N - 1] != 0)
    kw = dict(K=K, iters=10, reg=1e-6, seed=77)
    g = ddp_amd.fit_gmm(xs, us, **kw)
    assert not np.any(g.status)
    got = ddp_amd.fit_dynamics(xs, us, prior=ddp_amd.gmm_prior(g, xs, us, m0=1.0, n0=1.0))
    assert not np.any(got[4])
    rg = gr.fit(xs, us, **kw)
    Phi, mu0, pst = gr.prior(rg, xs, us, 1.0, 1.0)
    ref = fr.fit(xs, us, 0.0, (Phi, mu0, 1.0, 1.0))
    assert not np.any(rg["status"]) and not np.any(pst) and not np.any(ref["status"])
    ok = np.ones((N, B), dtype=bool)
    ok[N - 1] = False
    worst = [float(np.max(v[ok])) for v in fr.errors(got, ref)]
    print("lq_ad, S = 6, K = 3: [fx fu] %.2e  fc %.2e  cov %.2e   (GMM kappa max %.1f, pi min %.3f; fit kappa max %.1f)"
          % (tuple(worst) + (rg["kappa_max"], rg["pi_min"], ref["kappa"][ok].max())))
    assert max(worst) <= TOL, worst
