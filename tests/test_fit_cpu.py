"""fit_dynamics without a GPU: the two exports and the bindings, what is refused by name before the device is touched, the build's
resource record of the kernel, the long double reference of tests/fit_reference.py against known answers, and the condition on the
inputs of the GPU cases (kappa of every step that is expected to succeed)."""
import json
import os
import re

import numpy as np
import pytest

import ddp_amd
from ddp_amd import _lib

import fit_reference as fr
from conftest import ROOT

NEW = ("ddp_fit_dynamics_f64_dev", "ddp_fit_dynamics_f64")


def test_new_names_are_present():
    hdr = open(os.path.join(ROOT, "include", "ddp_amd.h")).read()
    jl = open(os.path.join(ROOT, "differentialdynamicprogramming.jl_amd", "julia", "DDPAmd.jl"), encoding="utf-8").read()
    L = _lib.lib()
    for name in NEW:
        assert name in _lib.EXPORTS and hasattr(L, name) and re.search(r"\b%s\s*\(" % name, hdr), name
        assert len(getattr(L, name).argtypes) == 19
    assert "fit_dynamics" in ddp_amd.__all__ and callable(ddp_amd.fit_dynamics)
    assert re.search(r"^function fit_dynamics\(", jl, flags=re.M) and "@ccall libddp.ddp_fit_dynamics_f64(" in jl
    assert "kl.Model(fx, fu, R1)" in ddp_amd.fit_dynamics.__doc__


def _call(entry, n=4, m=2, N=5, S=8, B=2, ridge=0.0, prior=False, layout=0, m0=1.0, n0=1.0, null=False):
    """the entry with a NULL handle: what is refused by name is refused before the handle is looked at"""
    p = 2 * n + m
    xs, us = np.zeros((n, N, S, B), order="F"), np.zeros((m, N, S, B), order="F")
    Phi, mu0 = (np.eye(p), np.zeros(p)) if prior else (None, None)
    out = [np.zeros(s, order="F") for s in ((n, n, N, B), (n, m, N, B), (n, N, B), (n, n, N, B))]
    st = np.zeros((N, B), dtype=np.int32, order="F")
    L = _lib.lib()
    rc = getattr(L, entry)(None, n, m, N, S, B, None if null else _lib.ptr(xs), _lib.ptr(us), ridge, _lib.ptr(Phi), _lib.ptr(mu0), m0, n0, layout,
                           *[_lib.ptr(o) for o in out], st.ctypes.data_as(_lib.vp))
    return rc, L.ddp_last_error().decode()


@pytest.mark.parametrize("entry", NEW)
@pytest.mark.parametrize("kw,words", [(dict(n=33), ("n = 33",)), (dict(n=0), ("n = 0",)), (dict(m=9), ("m = 9",)), (dict(m=0), ("m = 0",)),
                                      (dict(S=1), ("S = 1",)), (dict(N=0), ("N = 0",)), (dict(B=0), ("B = 0",)),
                                      (dict(ridge=-1e-3), ("ridge = -0.001",)), (dict(ridge=float("nan")), ("ridge",)),
                                      (dict(prior=True, layout=2), ("prior_layout = 2",)), (dict(prior=True, n0=-1.0), ("n0 = -1",)),
                                      (dict(null=True), ("null argument",))],
                         ids=["n33", "n0", "m9", "m0", "S1", "N0", "B0", "ridge<0", "ridge-nan", "layout", "n0<0", "null"])
def test_refused_by_name_before_any_launch(entry, kw, words):
    rc, err = _call(entry, **kw)
    assert rc == -1, (rc, err)
    assert "fit_dynamics" in err
    for w in words:
        assert w in err, err


@pytest.mark.parametrize("entry", NEW)
def test_legal_arguments_reach_the_handle(entry):
    for kw in (dict(), dict(n=32, m=8), dict(n=1, m=1, S=2), dict(prior=True, layout=1), dict(ridge=0.5)):
        rc, err = _call(entry, **kw)
        assert rc == -1 and err == "null handle", (kw, rc, err)


def test_python_refuses_wrong_shapes_without_a_device():
    xs, us = np.zeros((4, 5, 8)), np.zeros((2, 5, 8))
    with pytest.raises(ddp_amd.DDPError, match="xs, us should be"):
        ddp_amd.fit_dynamics(np.zeros((4, 5)), np.zeros((2, 5)))
    with pytest.raises(ddp_amd.DDPError, match="xs, us should be"):
        ddp_amd.fit_dynamics(xs, us[..., None])
    with pytest.raises(ddp_amd.DDPError, match="does not match"):
        ddp_amd.fit_dynamics(xs, np.zeros((2, 5, 9)))
    with pytest.raises(ddp_amd.DDPError, match="does not match"):
        ddp_amd.fit_dynamics(xs[..., None], np.zeros((2, 6, 8, 1)))
    for Phi, mu0 in ((np.eye(9), np.zeros(10)), (np.eye(10), np.zeros(9)), (np.zeros((10, 10, 5)), np.zeros(10)),
                     (np.zeros((10, 10, 4)), np.zeros((10, 4))), (np.zeros((10, 10, 5, 1)), np.zeros((10, 5, 1)))):
        with pytest.raises(ddp_amd.DDPError, match=r"p = 2n \+ m = 10"):
            ddp_amd.fit_dynamics(xs, us, prior=(Phi, mu0, 1.0, 1.0))


def test_kernel_uses_no_scratch():
    f = os.path.join(ROOT, "differentialdynamicprogramming.jl_amd", "build", "fit.o.usage.json")
    assert os.path.exists(f), "no build/fit.o.usage.json: build first"
    hit = [v for k, v in json.load(open(f)).items() if "ddp_fit_dynamics" in k]
    assert len(hit) == 2, hit                                    # the pool of p <= 16 and the full one
    for u in hit:
        assert int(u["ScratchSize"]) == 0 and int(u["VGPRs Spill"]) == 0 and u["Dynamic Stack"] == "False", u
        assert int(u["LDS Size"]) <= 65536, u
    assert min(int(u["LDS Size"]) for u in hit) <= 32768


# ------------------------------------------------------------------------------------------------------------------- the reference
EPS_LD = float(np.finfo(np.longdouble).eps)


@pytest.mark.parametrize("n,m,S", [(1, 1, 4), (4, 2, 9), (13, 4, 40)])
def test_reference_recovers_noise_free_dynamics(n, m, S):
    """y = F z + c exactly, ridge 0, S > d: F, c and cov = 0 to long double rounding (the inputs are rounded to double: their own
    rounding, 2^-53 relative, is amplified by kappa like any perturbation of the data)"""
    xs, us, F, c = fr.designed(n, m, 3, S, 2, 77, noise=0.0, smax=4.0)
    r = fr.fit(xs, us)
    assert np.all(r["status"] == 0)
    for b in range(2):
        for i in range(2):
            tol = 40 * (n + m) * r["kappa"][i, b] * 2.0 ** -53
            got = np.concatenate([r["fx"][:, :, i, b], r["fu"][:, :, i, b]], axis=1)
            assert np.linalg.norm(got - F[:, :, i, b]) <= tol * np.linalg.norm(F[:, :, i, b]), (i, b)
            assert np.linalg.norm(r["fc"][:, i, b] - c[:, i, b]) <= tol * r["sfc"][i, b], (i, b)
            assert np.linalg.norm(r["cov"][:, :, i, b]) <= tol * r["scov"][i, b], (i, b)
    assert EPS_LD < 2.0 ** -60, "np.longdouble is no wider than double here"


@pytest.mark.parametrize("n,m,S", [(1, 1, 64), (5, 3, 65), (13, 4, 64)])
def test_reference_matches_lstsq_with_an_intercept(n, m, S):
    xs, us, _, _ = fr.designed(n, m, 3, S, 1, 78)
    r = fr.fit(xs, us)
    for i in range(2):
        Z = np.concatenate([xs[:, i, :, 0], us[:, i, :, 0], np.ones((1, S))], axis=0).T
        Y = xs[:, i + 1, :, 0].T
        sol, res, _, _ = np.linalg.lstsq(Z, Y, rcond=None)
        tol = 100 * (n + m) * r["kappa"][i, 0] * 2.0 ** -53
        assert np.linalg.norm(np.concatenate([r["fx"][:, :, i, 0], r["fu"][:, :, i, 0]], axis=1) - sol[:-1].T) <= tol * r["sF"][i, 0]
        assert np.linalg.norm(r["fc"][:, i, 0] - sol[-1]) <= tol * r["sfc"][i, 0]
        E = Y - Z @ sol
        assert np.linalg.norm(r["cov"][:, :, i, 0] - E.T @ E / (S - 1)) <= tol * r["scov"][i, 0]


def test_reference_with_a_prior_and_two_samples_is_the_closed_form():
    """S = 2 < d: the centred sum is (w_1 - w_2)(w_1 - w_2)' / 2 and mu = (w_1 + w_2) / 2, so C is known in closed form; F = C_yz C_zz^-1 by
    np.linalg.solve"""
    n, m, S = 4, 2, 2
    xs, us, _, _ = fr.designed(n, m, 2, S, 1, 79, smax=3.0)
    Phi, mu0, m0, n0 = fr.designed_prior(n, m, 2, 1, 80, False)
    r = fr.fit(xs, us, 0.0, (Phi, mu0, m0, n0))
    assert r["status"][0, 0] == 0 and np.all(np.isfinite(r["fx"])) and np.all(np.isfinite(r["cov"]))
    W = np.concatenate([xs[:, 0, :, 0], us[:, 0, :, 0], xs[:, 1, :, 0]], axis=0)
    dw, mu = W[:, 0] - W[:, 1], (W[:, 0] + W[:, 1]) / 2
    Cm = (np.outer(dw, dw) / 2 + Phi + (S * m0 / (S + m0)) * np.outer(mu - mu0, mu - mu0)) / (S + n0)
    d = n + m
    F = np.linalg.solve(Cm[:d, :d], Cm[:d, d:]).T
    assert np.allclose(np.concatenate([r["fx"][:, :, 0, 0], r["fu"][:, :, 0, 0]], axis=1), F, rtol=0, atol=1e-12 * np.linalg.norm(F))
    assert np.allclose(r["fc"][:, 0, 0], mu[d:] - F @ mu[:d], rtol=0, atol=1e-12 * r["sfc"][0, 0])
    assert np.allclose(r["cov"][:, :, 0, 0], Cm[d:, d:] - F @ Cm[:d, d:], rtol=0, atol=1e-12 * r["scov"][0, 0])


def test_reference_status_rule():
    c = fr.identical_columns_case()
    st = c["ref"]["status"]
    assert st[fr.FAIL_STEP, 1] == 2 and np.count_nonzero(st) == 1
    assert np.all(np.isnan(c["ref"]["fx"][:, :, fr.FAIL_STEP, 1])) and np.all(np.isnan(c["ref"]["cov"][:, :, fr.FAIL_STEP, 1]))
    s = fr.nan_case("state")["ref"]
    assert s["status"][3, 1] == 3                                # state 2 of step 3 is pivot 2 of its own step ...
    assert s["status"][2, 1] == 4 + 2 + 1                        # ... and a y of step 2: no pivot of A fails, the results are not finite: d + 1
    assert np.count_nonzero(s["status"]) == 2 and np.all(np.isnan(s["fx"][:, :, 2, 1])) and np.all(np.isnan(s["cov"][:, :, 2, 1]))
    u = fr.nan_case("control")["ref"]
    assert u["status"][3, 1] == 4 + 1 + 1 and np.count_nonzero(u["status"]) == 1
    for r in (s, u):
        bad = ~np.isfinite(r["fx"]).all(axis=(0, 1))
        assert set(zip(*np.nonzero(bad))) <= {(2, 1), (3, 1)}


# ------------------------------------------------------------------------------------------- the condition on the GPU tests' inputs
@pytest.mark.parametrize("name", sorted(fr.CASES))
def test_designed_cases_are_inside_the_condition_cap(name):
    c = fr.case(name)
    r = c["ref"]
    N = c["N"]
    assert np.all(r["status"] == 0)
    if N > 1:
        print("%s: kappa max %.1f" % (name, r["kappa"][:N - 1].max()))
        assert r["kappa"][:N - 1].max() <= fr.KAPPA_CAP
    d, S = c["n"] + c["m"], c["S"]
    assert d <= 40 and S <= 130 and d * (S + d) * fr.KAPPA_CAP * 2.0 ** -53 < fr.TOL


def test_status_cases_are_inside_the_cap_where_they_succeed():
    for c in (fr.identical_columns_case(), fr.nan_case("state"), fr.nan_case("control")):
        r = c["ref"]
        ok = (r["status"] == 0) & np.isfinite(r["kappa"])
        ok[c["N"] - 1] = False
        print("kappa max %.1f" % r["kappa"][ok].max())
        assert r["kappa"][ok].max() <= fr.KAPPA_CAP


def test_sampler_case_is_inside_the_cap_with_its_ridge():
    s = fr.sampler_case()
    N = s["case"]["N"]
    r, r0 = s["ref"], s["ref0"]
    print("ridge %g: kappa max %.1f" % (fr.SAMPLER_RIDGE, r["kappa"][:N - 1].max()))
    assert np.all(r["status"] == 0) and r["kappa"][:N - 1].max() <= fr.KAPPA_CAP
    assert np.all(r0["status"][0] == 1)                                     # every rollout starts at x0: C_xx of step 0 is exactly zero
    # the model is linear and the dynamics carry no noise: without the ridge the last steps recover [A B], within the first-order bound
    n, m, S = s["case"]["n"], s["case"]["m"], s["case"]["S"]
    for b in range(s["case"]["B"]):
        for i in range(N - 4, N - 1):
            assert r0["status"][i, b] == 0
            got = np.concatenate([r0["fx"][:, :, i, b], r0["fu"][:, :, i, b]], axis=1)
            bound = (n + m) * (S + n + m) * r0["kappa"][i, b] * 2.0 ** -53
            print("step %d trajectory %d: kappa %.3g" % (i, b, r0["kappa"][i, b]))
            assert np.linalg.norm(got - s["AB"][..., b]) <= bound * np.linalg.norm(s["AB"][..., b])
