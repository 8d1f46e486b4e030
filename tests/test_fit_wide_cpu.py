"""fit_dynamics(..., wide=True) without a GPU: the two exports and the bindings, the named export tuples of _lib after the append, what
is refused by name before the handle is looked at, the build's resource record of the kernel, and the condition on the inputs of the
GPU cases (tests/fit_wide_cases.py) with the statuses the reference gives to the three status cases."""
import inspect
import json
import os
import re

import numpy as np
import pytest

import ddp_amd
from ddp_amd import _lib

import fit_reference as fr
import fit_wide_cases as fw
from conftest import ROOT

NEW = ("ddp_fit_dynamics_wide_f64_dev", "ddp_fit_dynamics_wide_f64")


def test_new_names_are_present():
    hdr = open(os.path.join(ROOT, "include", "ddp_amd.h")).read()
    jl = open(os.path.join(ROOT, "differentialdynamicprogramming.jl_amd", "julia", "DDPAmd.jl"), encoding="utf-8").read()
    L = _lib.lib()
    for name in NEW:
        assert name in _lib.EXPORTS and hasattr(L, name) and re.search(r"\b%s\s*\(" % name, hdr), name
        assert len(getattr(L, name).argtypes) == 19
        assert getattr(L, name).argtypes == L.ddp_fit_dynamics_f64.argtypes
    assert _lib.FIT_WIDE_EXPORTS == NEW
    sig = inspect.signature(ddp_amd.fit_dynamics).parameters["wide"]
    assert sig.kind is inspect.Parameter.KEYWORD_ONLY and sig.default is False
    assert "n <= 64" in ddp_amd.fit_dynamics.__doc__ and "n <= 32" in ddp_amd.fit_dynamics.__doc__
    assert "@ccall libddp.ddp_fit_dynamics_wide_f64(" in jl and "@ccall libddp.ddp_fit_dynamics_f64(" in jl
    assert re.search(r"^function fit_dynamics\(xs, us;[^\n]*wide::Bool=false", jl, flags=re.M)


def test_named_export_tuples_hold_what_they_held():
    assert _lib.EXPECT_EXPORTS == ("ddp_expected_cost_f64_dev", "ddp_expected_cost_f64", "ddp_kl_step_adjust_f64_dev", "ddp_kl_step_adjust_f64",
                                   "ddp_kl_set_steps_f64_dev", "ddp_kl_set_steps_f64")
    assert _lib.COST_FIT_EXPORTS == ("ddp_user_cost_fit_f64_dev", "ddp_user_cost_fit_f64", "ddp_user_ilqgkl_cost_f64_dev", "ddp_user_ilqgkl_cost_f64")
    assert _lib.GMM_EXPORTS == ("ddp_gmm_fit_f64_dev", "ddp_gmm_fit_f64", "ddp_gmm_prior_f64_dev", "ddp_gmm_prior_f64")
    assert _lib.FITTED_EXPORTS == ("ddp_user_rollout_fit_f64_dev", "ddp_user_rollout_fit_f64", "ddp_user_ilqgkl_fit_f64_dev", "ddp_user_ilqgkl_fit_f64")
    assert _lib.FIT_EXPORTS == ("ddp_fit_dynamics_f64_dev", "ddp_fit_dynamics_f64")
    assert _lib.SAMPLE_EXPORTS == ("ddp_normal_f64_dev", "ddp_normal_f64", "ddp_user_sample_f64_dev", "ddp_user_sample_f64")
    assert _lib.CONSTRAINTS_EXPORTS == ("ddp_user_check_c", "ddp_user_create_c", "ddp_user_set_multipliers", "ddp_user_constraints_f64_dev",
                                        "ddp_user_constraints_f64", "ddp_al_default_opts", "ddp_user_ilqg_al_f64_dev", "ddp_user_ilqg_al_f64")
    assert _lib.FIT_WIDE_EXPORTS == ("ddp_fit_dynamics_wide_f64_dev", "ddp_fit_dynamics_wide_f64")
    assert len(set(_lib.EXPORTS)) == len(_lib.EXPORTS)


def _call(entry, n=40, m=12, N=5, S=8, B=2, ridge=0.0, prior=False, layout=0, m0=1.0, n0=1.0, null=False):
    """the entry with a NULL handle: what is refused by name is refused before the handle is looked at"""
    p = 2 * max(n, 0) + max(m, 0)
    sh = lambda *s: tuple(max(k, 0) for k in s)
    xs, us = np.zeros(sh(n, N, S, B), order="F"), np.zeros(sh(m, N, S, B), order="F")
    Phi, mu0 = (np.eye(p), np.zeros(p)) if prior else (None, None)
    out = [np.zeros(s, order="F") for s in (sh(n, n, N, B), sh(n, m, N, B), sh(n, N, B), sh(n, n, N, B))]
    st = np.zeros(max(N * B, 1), dtype=np.int32)
    keep = np.zeros(1)                                           # an empty array (n, N or B = 0) still passes a non-null pointer
    ptr = lambda a: _lib.ptr(a if a.size else keep)
    L = _lib.lib()
    rc = getattr(L, entry)(None, n, m, N, S, B, None if null else ptr(xs), ptr(us), ridge, _lib.ptr(Phi), _lib.ptr(mu0), m0, n0, layout,
                           *[ptr(o) for o in out], st.ctypes.data_as(_lib.vp))
    return rc, L.ddp_last_error().decode()


@pytest.mark.parametrize("entry", NEW)
@pytest.mark.parametrize("kw,words", [(dict(n=65), ("n = 65",)), (dict(n=0), ("n = 0",)), (dict(m=33), ("m = 33",)), (dict(m=0), ("m = 0",)),
                                      (dict(S=1), ("S = 1",)), (dict(N=0), ("N = 0",)), (dict(B=0), ("B = 0",)),
                                      (dict(ridge=-1e-3), ("ridge = -0.001",)), (dict(ridge=float("nan")), ("ridge",)),
                                      (dict(prior=True, layout=2), ("prior_layout = 2",)), (dict(prior=True, n0=-1.0), ("n0 = -1",)),
                                      (dict(null=True), ("null argument",))],
                         ids=["n65", "n0", "m33", "m0", "S1", "N0", "B0", "ridge<0", "ridge-nan", "layout", "n0<0", "null"])
def test_refused_by_name_before_the_handle_is_looked_at(entry, kw, words):
    rc, err = _call(entry, **kw)
    assert rc == -1, (rc, err)
    assert "fit_dynamics" in err and err != "null handle"
    for w in words:
        assert w in err, err


@pytest.mark.parametrize("entry", NEW)
@pytest.mark.parametrize("prior", [False, True])
def test_legal_arguments_reach_the_handle(entry, prior):
    for n, m in ((33, 8), (32, 9), (1, 32), (64, 32), (4, 2)):
        for layout in ((0, 1) if prior else (0,)):
            rc, err = _call(entry, n=n, m=m, prior=prior, layout=layout)
            assert rc == -1 and err == "null handle", (n, m, prior, layout, rc, err)


def test_narrow_entries_keep_their_box():
    for entry in ("ddp_fit_dynamics_f64_dev", "ddp_fit_dynamics_f64"):
        for kw, word in ((dict(n=33, m=8), "n = 33"), (dict(n=32, m=9), "m = 9")):
            rc, err = _call(entry, **kw)
            assert rc == -1 and "fit_dynamics" in err and word in err, (entry, kw, err)


def test_kernel_uses_no_scratch():
    f = os.path.join(ROOT, "differentialdynamicprogramming.jl_amd", "build", "fit_wide.o.usage.json")
    assert os.path.exists(f), "no build/fit_wide.o.usage.json: build first"
    use = json.load(open(f))
    assert any("ddp_fit_dynamics_wide" in k for k in use), list(use)
    for k, u in use.items():
        assert int(u["ScratchSize"]) == 0 and int(u["VGPRs Spill"]) == 0 and u["Dynamic Stack"] == "False", (k, u)
        assert int(u["LDS Size"]) <= 4096, (k, u)               # the static part; the blocks are dynamic LDS sized from (n, m)


# ------------------------------------------------------------------------------------------- the condition on the GPU tests' inputs
@pytest.mark.parametrize("name", sorted(fw.CASES))
def test_designed_cases_are_inside_the_condition_cap(name):
    c = fw.case(name)
    r = c["ref"]
    N = c["N"]
    assert np.all(r["status"] == 0)
    if N > 1:
        print("%s: kappa max %.1f" % (name, r["kappa"][:N - 1].max()))
        assert r["kappa"][:N - 1].max() <= fw.KAPPA_CAP_WIDE
    d, S = c["n"] + c["m"], c["S"]
    assert d <= 96 and S <= 230 and d * (S + d) * fw.KAPPA_CAP_WIDE * 2.0 ** -53 < fr.TOL
    assert not (c["n"] <= 32 and c["m"] <= 8), "a wide case should run the wide kernel"


@pytest.mark.parametrize("name", sorted(fw.STATUS_CASES))
def test_status_cases_in_the_reference(name):
    c = fw.STATUS_CASES[name]()
    r = c["ref"]
    assert np.array_equal(r["status"], c["expect"]), (name, r["status"].T)
    bad = c["expect"] != 0
    for a in (r["fx"], r["fu"], r["cov"]):
        assert np.all(np.isnan(a[:, :, bad])) and np.all(np.isfinite(a[:, :, ~bad]))
    ok = ~bad
    ok[c["N"] - 1] = False
    print("%s: kappa max %.1f" % (name, r["kappa"][ok].max()))
    assert r["kappa"][ok].max() <= fw.KAPPA_CAP_WIDE
    d, S = c["n"] + c["m"], c["S"]
    assert d * (S + d) * fw.KAPPA_CAP_WIDE * 2.0 ** -53 < fr.TOL
