"""fit_gmm and gmm_prior without a GPU: the four exports and the bindings, what is refused by name before the device is touched, the
build's resource record of the kernels, the long double reference of tests/gmm_reference.py against known answers, and the condition on
the inputs of the GPU cases (float64 against long double, kappa of every Sigma_k, every pi_k)."""
import json
import os
import re

import numpy as np
import pytest

import ddp_amd
from ddp_amd import _lib

import gmm_reference as gr
from conftest import ROOT

LD = np.longdouble
FIT = ("ddp_gmm_fit_f64_dev", "ddp_gmm_fit_f64")
PRIOR = ("ddp_gmm_prior_f64_dev", "ddp_gmm_prior_f64")


def test_new_names_are_present():
    hdr = open(os.path.join(ROOT, "include", "ddp_amd.h")).read()
    jl = open(os.path.join(ROOT, "differentialdynamicprogramming.jl_amd", "julia", "DDPAmd.jl"), encoding="utf-8").read()
    L = _lib.lib()
    for name, nargs in zip(FIT + PRIOR, (23, 23, 18, 18)):
        assert name in _lib.EXPORTS and hasattr(L, name) and re.search(r"\b%s\s*\(" % name, hdr), name
        assert len(getattr(L, name).argtypes) == nargs
    for name in ("fit_gmm", "gmm_prior", "GMM"):
        assert name in ddp_amd.__all__ and callable(getattr(ddp_amd, name))
    assert re.search(r"^function fit_gmm\(", jl, flags=re.M) and "@ccall libddp.ddp_gmm_fit_f64(" in jl
    assert re.search(r"^function gmm_prior\(", jl, flags=re.M) and "@ccall libddp.ddp_gmm_prior_f64(" in jl
    assert len(L.ddp_fit_dynamics_f64.argtypes) == 19            # what this feature builds on keeps its signature
    assert "fit_dynamics(xs, us, prior=" in ddp_amd.gmm_prior.__doc__


def _fit(entry, n=4, m=2, N=5, S=8, B=2, K=3, iters=2, pool=1, reg=1e-6, init=False, null=False):
    """the entry with a NULL handle: what is refused by name is refused before the handle is looked at"""
    p, G = 2 * n + m, 1 if pool else max(B, 1)
    Kc = min(max(K, 1), 32)
    xs, us = np.zeros((n, N, S, max(B, 1)), order="F"), np.zeros((m, N, S, max(B, 1)), order="F")
    out = [np.zeros(s, order="F") for s in ((Kc, G), (p, Kc, G), (p, p, Kc, G), (max(iters, 1), G))]
    ini = [_lib.ptr(o.copy(order="F")) if init else None for o in out[:3]]
    st = np.zeros(G, dtype=np.int32)
    L = _lib.lib()
    rc = getattr(L, entry)(None, n, m, N, S, B, K, iters, pool, 0, None if null else _lib.ptr(xs), _lib.ptr(us), reg, 1, 2, *ini,
                           *[_lib.ptr(o) for o in out], st.ctypes.data_as(_lib.vp))
    return rc, L.ddp_last_error().decode()


def _prior(entry, n=4, m=2, N=5, S=8, B=2, K=3, pool=1, m0=1.0, n0=1.0, null=False):
    p, G = 2 * n + m, 1 if pool else max(B, 1)
    Kc = min(max(K, 1), 32)
    xs, us = np.zeros((n, N, S, max(B, 1)), order="F"), np.zeros((m, N, S, max(B, 1)), order="F")
    mix = [np.zeros(s, order="F") for s in ((Kc, G), (p, Kc, G), (p, p, Kc, G))]
    out = [np.zeros(s, order="F") for s in ((p, p, max(N, 1), max(B, 1)), (p, max(N, 1), max(B, 1)))]
    st = np.zeros((max(N, 1), max(B, 1)), dtype=np.int32, order="F")
    L = _lib.lib()
    rc = getattr(L, entry)(None, n, m, N, S, B, K, pool, _lib.ptr(xs), _lib.ptr(us), *[_lib.ptr(o) for o in mix], m0, n0,
                           None if null else _lib.ptr(out[0]), _lib.ptr(out[1]), st.ctypes.data_as(_lib.vp))
    return rc, L.ddp_last_error().decode()


COMMON = [(dict(n=33), "n = 33"), (dict(n=0), "n = 0"), (dict(m=9), "m = 9"), (dict(m=0), "m = 0"), (dict(K=33), "K = 33"), (dict(K=0), "K = 0"),
          (dict(N=1), "N = 1"), (dict(S=0), "S = 0"), (dict(B=0), "B = 0"), (dict(pool=2), "pool = 2"), (dict(null=True), "null argument")]


@pytest.mark.parametrize("entry", FIT)
@pytest.mark.parametrize("kw,word", COMMON + [(dict(iters=-1), "iters = -1"), (dict(reg=-1e-3), "reg = -0.001"), (dict(reg=float("nan")), "reg"),
                                              (dict(reg=float("inf")), "reg"), (dict(N=2, S=1, B=1), "P = 1"), (dict(N=2, S=1, B=5, pool=0), "P = 1")],
                         ids=lambda v: v if isinstance(v, str) else None)
def test_fit_refused_by_name_before_any_launch(entry, kw, word):
    rc, err = _fit(entry, **kw)
    assert rc == -1, (rc, err)
    assert err.startswith("fit_gmm:") and word in err, err


@pytest.mark.parametrize("entry", PRIOR)
@pytest.mark.parametrize("kw,word", COMMON + [(dict(m0=-1.0), "m0 = -1"), (dict(n0=-2.0), "n0 = -2"), (dict(n0=float("nan")), "n0"),
                                              (dict(m0=float("inf")), "m0")], ids=lambda v: v if isinstance(v, str) else None)
def test_prior_refused_by_name_before_any_launch(entry, kw, word):
    rc, err = _prior(entry, **kw)
    assert rc == -1, (rc, err)
    assert err.startswith("gmm_prior:") and word in err, err


def test_legal_arguments_reach_the_handle():
    for entry in FIT:
        for kw in (dict(), dict(n=32, m=8, K=32), dict(n=1, m=1, K=1, N=2, S=2, B=1), dict(iters=0), dict(pool=0), dict(init=True), dict(reg=0.0),
                   dict(N=2, S=1, B=2)):
            rc, err = _fit(entry, **kw)
            assert rc == -1 and err == "null handle", (entry, kw, rc, err)
    for entry in PRIOR:
        for kw in (dict(), dict(n=32, m=8, K=32), dict(n=1, m=1, K=1, N=2, S=1, B=1), dict(pool=0), dict(m0=0.0, n0=0.0)):
            rc, err = _prior(entry, **kw)
            assert rc == -1 and err == "null handle", (entry, kw, rc, err)


def test_fit_refuses_half_an_init():
    L = _lib.lib()
    z = np.zeros(2000)
    st = np.zeros(1, dtype=np.int32)
    rc = L.ddp_gmm_fit_f64(None, 4, 2, 5, 8, 2, 3, 2, 1, 0, _lib.ptr(z), _lib.ptr(z), 0.0, 0, 0, _lib.ptr(z), None, _lib.ptr(z), _lib.ptr(z),
                           _lib.ptr(z), _lib.ptr(z), _lib.ptr(z), st.ctypes.data_as(_lib.vp))
    assert rc == -1 and "init needs pi, mu and Sigma together" in L.ddp_last_error().decode()


def test_python_refuses_wrong_shapes_without_a_device():
    xs, us = np.zeros((4, 5, 8)), np.zeros((2, 5, 8))
    for f in (lambda a, b: ddp_amd.fit_gmm(a, b, 2), lambda a, b: ddp_amd.gmm_prior(g1, a, b)):
        g1 = ddp_amd.GMM(np.ones((2, 1)) / 2, np.zeros((10, 2, 1)), np.zeros((10, 10, 2, 1)), np.zeros((0, 1)), np.zeros(1, dtype=np.int32), True)
        with pytest.raises(ddp_amd.DDPError, match="xs, us should be"):
            f(np.zeros((4, 5)), np.zeros((2, 5)))
        with pytest.raises(ddp_amd.DDPError, match="xs, us should be"):
            f(xs, us[..., None])
        with pytest.raises(ddp_amd.DDPError, match="does not match"):
            f(xs, np.zeros((2, 5, 9)))
    for init in ((np.ones(2), np.zeros((9, 2)), np.zeros((10, 10, 2))), (np.ones(3), np.zeros((10, 3)), np.zeros((10, 10, 3))),
                 (np.ones((2, 2)), np.zeros((10, 2, 2)), np.zeros((10, 10, 2, 2)))):
        with pytest.raises(ddp_amd.DDPError, match=r"p = 2n \+ m = 10, K = 2, G = 1"):
            ddp_amd.fit_gmm(xs, us, 2, init=init)
    with pytest.raises(ddp_amd.DDPError, match="G = 3"):           # one mixture per trajectory wants one init per trajectory
        ddp_amd.fit_gmm(np.zeros((4, 5, 8, 3)), np.zeros((2, 5, 8, 3)), 2, pool=False, init=(np.ones(2), np.zeros((10, 2)), np.zeros((10, 10, 2))))
    with pytest.raises(ddp_amd.DDPError, match="a GMM"):
        ddp_amd.gmm_prior((1, 2, 3), xs, us)
    bad = ddp_amd.GMM(np.ones((2, 1)) / 2, np.zeros((9, 2, 1)), np.zeros((10, 10, 2, 1)), np.zeros((0, 1)), np.zeros(1, dtype=np.int32), True)
    with pytest.raises(ddp_amd.DDPError, match=r"p = 2n \+ m = 10"):
        ddp_amd.gmm_prior(bad, xs, us)
    with pytest.raises(ddp_amd.DDPError, match="seed"):
        ddp_amd.fit_gmm(xs, us, 2, seed=-1)
    for kw, word in ((dict(K=0), "K = 0"), (dict(K=33), "K = 33"), (dict(K=2, iters=-1), "iters = -1")):
        with pytest.raises(ddp_amd.DDPError, match=word):
            ddp_amd.fit_gmm(xs, us, kw.pop("K"), **kw)


def test_kernels_use_no_scratch():
    f = os.path.join(ROOT, "differentialdynamicprogramming.jl_amd", "build", "gmm.o.usage.json")
    assert os.path.exists(f), "no build/gmm.o.usage.json: build first"
    usage = json.load(open(f))
    for want in ("gmm_estep", "gmm_means", "gmm_gram", "gmm_prep", "gmm_status", "gmm_prior"):
        assert any(want in k for k in usage), want
    assert not any("ddp_fit_dynamics" in k for k in usage)
    for k, u in usage.items():
        assert int(u["ScratchSize"]) == 0 and int(u["VGPRs Spill"]) == 0 and u["Dynamic Stack"] == "False", (k, u)
        assert int(u["LDS Size"]) <= 65536, (k, u)


# ------------------------------------------------------------------------------------------------------------------- the reference
def _gauss_ll(W, mu, Sigma):
    """sum_j log N(w_j; mu, Sigma) by the textbook formula (slogdet, solve) in float64"""
    p, P = W.shape
    D = W - mu[:, None]
    return -0.5 * (P * (p * np.log(2 * np.pi) + np.linalg.slogdet(Sigma)[1]) + np.sum(D * np.linalg.solve(Sigma, D)))


@pytest.mark.parametrize("iters", [0, 1, 4])
@pytest.mark.parametrize("pool", [True, False])
def test_reference_with_one_cluster_is_the_moments(iters, pool):
    n, m, N, S, B, reg = 3, 2, 5, 9, 2, 1e-3
    xs, us, _ = gr.designed(n, m, N, S, B, 3, 41)
    r = gr.fit(xs, us, K=1, iters=iters, reg=reg, seed=7, pool=pool)
    for g, Wg in enumerate(gr.mixture_points(gr.points(xs, us, np.float64), pool)):
        mu, C = Wg.mean(axis=1), np.cov(Wg, bias=True) + reg * np.eye(2 * n + m)
        assert r["status"][g] == 0 and r["pi"][0, g] == 1
        assert np.allclose(r["mu"][:, 0, g].astype(float), mu, rtol=0, atol=1e-13 * np.linalg.norm(mu))
        assert np.allclose(r["Sigma"][:, :, 0, g].astype(float), C, rtol=0, atol=1e-13 * np.linalg.norm(C))
        for t in range(iters):
            assert abs(float(r["ll"][t, g]) - _gauss_ll(Wg, mu, C)) <= 1e-12 * abs(_gauss_ll(Wg, mu, C))
    Phi, mu0, st = gr.prior(r, xs, us, 1.0, 2.5)
    assert np.all(st == 0) and np.all(Phi[:, :, N - 1] == 0) and np.all(mu0[:, N - 1] == 0)
    for b in range(B):
        g = 0 if pool else b
        for i in range(N - 1):                                    # K = 1: omega = 1 whatever the points
            assert gr.rel(mu0[:, i, b], r["mu"][:, 0, g]) <= 1e-18 and gr.rel(Phi[:, :, i, b], 2.5 * r["Sigma"][:, :, 0, g]) <= 1e-18


def test_reference_likelihood_does_not_decrease_without_reg():
    xs, us, _ = gr.designed(3, 2, 6, 30, 2, 3, 42, sep=2.0)
    r = gr.fit(xs, us, K=3, iters=15, reg=0.0, seed=11)
    ll = r["ll"][:, 0]
    assert r["status"][0] == 0 and np.all(np.diff(ll) >= -1e-15 * np.abs(ll[:-1])), ll
    assert ll[-1] > ll[0]


def test_reference_m_step_from_true_labels_is_the_cluster_moments():
    n, m, N, S, B, K = 2, 2, 5, 12, 3, 3
    xs, us, lab = gr.designed(n, m, N, S, B, K, 43, sep=8.0)
    pi, mu, Sigma = gr.true_init(xs, us, lab, K)
    Wg = gr.mixture_points(gr.points(xs, us, np.float64), True)[0]
    flat = lab.transpose(2, 0, 1).reshape(-1)
    for k in range(K):
        Wk = Wg[:, flat == k]
        assert abs(pi[k] - Wk.shape[1] / Wg.shape[1]) <= 1e-15
        assert np.allclose(mu[:, k], Wk.mean(axis=1), rtol=0, atol=1e-13 * np.linalg.norm(mu[:, k]))
        assert np.allclose(Sigma[:, :, k], np.cov(Wk, bias=True), rtol=0, atol=1e-13 * np.linalg.norm(Sigma[:, :, k]))
    # clusters this far apart: one E-step from the true moments gives the true labels back, so EM stays where it is
    init = tuple(np.asfortranarray(a[..., None]) for a in (pi, mu, Sigma))
    r = gr.fit(xs, us, K=K, iters=1, reg=0.0, init=init)
    assert gr.errors(r, dict(pi=pi[:, None], mu=mu[..., None], Sigma=Sigma[..., None], ll=np.zeros((0, 1))))["Sigma"] <= 1e-9


def test_reference_assignment_is_a_slice_of_itself_and_off_the_noise_stream():
    a = gr.hard_assignment(99, 5, 7, 6, 4)
    assert a.shape == (6, 6, 4) and a.min() == 0 and a.max() == 4
    assert np.array_equal(gr.hard_assignment(99, 5, 7, 6, 1, traj0=2)[..., 0], a[..., 2])
    assert np.array_equal(gr.hard_assignment(99, 5, 4, 6, 4), a[:3])              # N does not enter
    import sample_reference as sr
    w = sr.philox4x32_10(np.arange(3), np.arange(3), np.arange(3), np.full(3, 0x80000000), 99, 0)[0]
    assert np.array_equal(w % np.uint64(5), [a[0, 0, 0], a[1, 1, 1], a[2, 2, 2]])
    assert not np.array_equal(sr.philox4x32_10(np.arange(3), np.arange(3), np.arange(3), np.zeros(3), 99, 0)[0], w)


def test_reference_status_rules():
    c = gr.empty_cluster_case()
    r = c["ref"]
    assert list(r["status"]) == [0, 2]
    assert np.all(np.isnan(r["pi"][:, 1])) and np.all(np.isnan(r["mu"][..., 1])) and np.all(np.isnan(r["Sigma"][..., 1]))
    assert np.isfinite(r["ll"][0, 1]) and np.all(np.isnan(r["ll"][1:, 1]))        # the E-step of iteration 0 ran; its M-step emptied cluster 1
    assert np.all(np.isfinite(r["ll"][:, 0])) and np.all(np.isfinite(r["Sigma"][..., 0]))
    Phi, mu0, st = gr.prior(r, c["xs"], c["us"])
    assert np.all(st[:-1, 1] == 2) and np.all(st[:, 0] == 0) and np.all(np.isnan(Phi[:, :, :-1, 1])) and np.all(np.isfinite(Phi[..., 0]))
    d = gr.nan_point_case()
    st = d["pstatus"]
    assert st[1, 1] == 1 and st[2, 1] == 1 and np.count_nonzero(st) == 2
    bad = ~np.isfinite(d["Phi"]).all(axis=(0, 1))
    assert set(zip(*np.nonzero(bad))) == {(1, 1), (2, 1)}


# ------------------------------------------------------------------------------------------- the condition on the GPU tests' inputs
@pytest.mark.parametrize("name", sorted(gr.CASES))
def test_designed_cases_are_well_conditioned(name):
    c, d = gr.case(name), gr.case64(name)
    r = c["ref"]
    assert np.all(r["status"] == 0) and np.all(c["pstatus"] == 0)
    e = {**gr.errors(d["ref"], r), **gr.prior_errors(d["Phi"], d["mu0"], c)}
    print("%s: float64 against long double %s, kappa max %.1f, pi min %.3f" % (name, {k: "%.1e" % v for k, v in e.items()}, r["kappa_max"], r["pi_min"]))
    for k, v in e.items():
        assert v <= gr.COND_TOL, (k, v)
    assert r["kappa_max"] <= gr.KAPPA_CAP
    assert r["pi_min"] >= gr.PI_MIN
    assert np.finfo(LD).eps < 2.0 ** -60, "np.longdouble is no wider than double here"


def test_status_cases_are_well_conditioned_where_they_succeed():
    c = gr.empty_cluster_case()
    solo = gr.fit(c["xs"][..., :1], c["us"][..., :1], **{**c["kw"], "init": tuple(a[..., :1] for a in c["kw"]["init"])})
    assert solo["status"][0] == 0 and solo["kappa_max"] <= gr.KAPPA_CAP and solo["pi_min"] >= gr.PI_MIN
    assert np.array_equal(solo["Sigma"][..., 0], c["ref"]["Sigma"][..., 0])
