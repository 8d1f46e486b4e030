"""expected_cost, kl_step_adjust and the table of kl_steps without a GPU: the exports and the bindings, what is refused by name before
the handle is looked at, the build's resource record of the kernel, the long double reference of tests/expect_reference.py against known
answers, and the condition on the inputs of the GPU cases (the growth of the state covariance, the scales of ec, the cancellation cap of
the step-rule triples)."""
import json
import os
import re

import numpy as np
import pytest

import ddp_amd
from ddp_amd import _lib, kl

import expect_reference as er
from conftest import ROOT

NEW = {"ddp_expected_cost_f64_dev": 27, "ddp_expected_cost_f64": 27, "ddp_kl_step_adjust_f64_dev": 11, "ddp_kl_step_adjust_f64": 11,
       "ddp_kl_set_steps_f64_dev": 3, "ddp_kl_set_steps_f64": 3}


def test_new_names_are_present():
    hdr = open(os.path.join(ROOT, "include", "ddp_amd.h")).read()
    jl = open(os.path.join(ROOT, "differentialdynamicprogramming.jl_amd", "julia", "DDPAmd.jl"), encoding="utf-8").read()
    L = _lib.lib()
    for name, arity in NEW.items():
        assert name in _lib.EXPORTS and hasattr(L, name) and re.search(r"\b%s\s*\(" % name, hdr), name
        assert len(getattr(L, name).argtypes) == arity, name
    assert "expected_cost" in ddp_amd.__all__ and callable(ddp_amd.expected_cost)
    assert "kl_step_adjust" in kl.__all__ and callable(kl.kl_step_adjust)
    assert re.search(r"^function expected_cost\(", jl, flags=re.M) and re.search(r"^function kl_step_adjust\(", jl, flags=re.M)
    for name in ("ddp_expected_cost_f64", "ddp_kl_step_adjust_f64", "ddp_kl_set_steps_f64"):
        assert "@ccall libddp.%s(" % name in jl, name
    assert "one step per trajectory" in kl.iLQGkl.__doc__.lower()
    assert "status" in ddp_amd.expected_cost.__doc__


def test_the_older_export_groups_keep_their_names():
    """the groups of _lib are slices of EXPORTS counted from its end: six new names behind them must not shift one"""
    assert _lib.COST_FIT_EXPORTS[0] == "ddp_user_cost_fit_f64_dev" and _lib.GMM_EXPORTS[0] == "ddp_gmm_fit_f64_dev"
    assert _lib.FITTED_EXPORTS[0] == "ddp_user_rollout_fit_f64_dev" and _lib.FIT_EXPORTS == ("ddp_fit_dynamics_f64_dev", "ddp_fit_dynamics_f64")
    assert _lib.SAMPLE_EXPORTS[0] == "ddp_normal_f64_dev" and _lib.CONSTRAINTS_EXPORTS[0] == "ddp_user_check_c"
    assert len(_lib.CONSTRAINTS_EXPORTS) == 8 and set(_lib.EXPECT_EXPORTS) == set(NEW)


def _expect(entry, n=4, m=2, N=5, B=2, mb=1, cb=1, null=None, sigma0=None):
    """the entry with a NULL handle: what is refused by name is refused before the handle is looked at"""
    z = lambda *s: np.zeros(s, order="F")                                                # noqa: E731
    a = dict(K=z(m, n, N, B), Sg=z(m, m, N, B), x0=z(n, B), x=z(n, N, B), u=z(m, N, B), fx=z(n, n, N, B), fu=z(n, m, N, B), fc=z(n, N, B),
             cov=z(n, n, N, B), cx=z(n, N, B), cu=z(m, N, B), cxx=z(n, n, N, B), cxu=z(n, m, N, B), cuu=z(m, m, N, B), c0=z(N, B),
             S0=z(n, n, B) if sigma0 is None else sigma0, ec=z(N, B), mu=z(n + m, N, B), sigma=z(n + m, n + m, N, B))
    st = np.zeros(max(B, 1), dtype=np.int32)
    if null:
        a[null] = None
    P = _lib.ptr
    L = _lib.lib()
    rc = getattr(L, entry)(None, n, m, N, B, P(a["K"]), P(a["Sg"]), P(a["x0"]), P(a["x"]), P(a["u"]), P(a["fx"]), P(a["fu"]), P(a["fc"]), P(a["cov"]),
                           mb, P(a["cx"]), P(a["cu"]), P(a["cxx"]), P(a["cxu"]), P(a["cuu"]), P(a["c0"]), cb, P(a["S0"]), P(a["ec"]),
                           st.ctypes.data_as(_lib.vp), P(a["mu"]), P(a["sigma"]))
    return rc, L.ddp_last_error().decode()


@pytest.mark.parametrize("entry", ["ddp_expected_cost_f64_dev", "ddp_expected_cost_f64"])
@pytest.mark.parametrize("kw,words", [(dict(n=0), ("n = 0",)), (dict(n=33), ("n = 33",)), (dict(m=0), ("m = 0",)), (dict(m=9), ("m = 9",)),
                                      (dict(N=0), ("N = 0",)), (dict(B=0), ("B = 0",)), (dict(mb=2), ("model_batched = 2",)),
                                      (dict(cb=-1), ("cost_batched = -1",)), (dict(null="K"), ("null argument",)),
                                      (dict(null="fc"), ("null argument",)), (dict(null="c0"), ("null argument",)),
                                      (dict(null="ec"), ("null argument",))],
                         ids=["n0", "n33", "m0", "m9", "N0", "B0", "model-flag", "cost-flag", "null-K", "null-fc", "null-c0", "null-ec"])
def test_expected_cost_refuses_by_name_before_any_launch(entry, kw, words):
    rc, err = _expect(entry, **kw)
    assert rc == -1, (rc, err)
    assert "expected_cost" in err
    for w in words:
        assert w in err, err


def test_expected_cost_host_flavour_refuses_a_non_finite_sigma0():
    for bad in (np.nan, np.inf):
        S0 = np.zeros((4, 4, 2), order="F")
        S0[1, 2, 1] = bad
        rc, err = _expect("ddp_expected_cost_f64", sigma0=S0)
        assert rc == -1 and "expected_cost" in err and "Sigma0 is not finite" in err and "trajectory 1" in err, err


@pytest.mark.parametrize("entry", ["ddp_expected_cost_f64_dev", "ddp_expected_cost_f64"])
def test_expected_cost_legal_arguments_reach_the_handle(entry):
    for kw in (dict(), dict(n=32, m=8), dict(n=1, m=1, N=1, B=1), dict(mb=0), dict(cb=0), dict(null="Sg"), dict(null="cov"), dict(null="x0"),
               dict(null="S0"), dict(null="mu"), dict(null="sigma")):
        rc, err = _expect(entry, **kw)
        assert rc == -1 and err == "null handle", (kw, rc, err)


def _adjust(entry, N=5, B=3, step_min=1e-2, step_max=1e2, null=None):
    a = dict(p=np.zeros((N, B), order="F"), d=np.zeros((N, B), order="F"), a=np.zeros((N, B), order="F"), k=np.ones(max(B, 1)), new=np.zeros(max(B, 1)),
             mult=np.zeros(max(B, 1)))
    if null:
        a[null] = None
    L = _lib.lib()
    rc = getattr(L, entry)(None, N, B, *[_lib.ptr(a[k]) for k in ("p", "d", "a", "k")], step_min, step_max, _lib.ptr(a["new"]), _lib.ptr(a["mult"]))
    return rc, L.ddp_last_error().decode()


@pytest.mark.parametrize("entry", ["ddp_kl_step_adjust_f64_dev", "ddp_kl_step_adjust_f64"])
def test_kl_step_adjust_refuses_by_name_and_reaches_the_handle(entry):
    for kw, word in ((dict(N=0), "N = 0"), (dict(B=0), "B = 0"), (dict(step_min=0.0), "step_min = 0"), (dict(step_min=2.0, step_max=1.0), "step_max = 1"),
                     (dict(step_max=float("inf")), "step_max = inf"), (dict(step_min=float("nan")), "step_min = nan"), (dict(null="k"), "null argument"),
                     (dict(null="mult"), "null argument")):
        rc, err = _adjust(entry, **kw)
        assert rc == -1 and "kl_step_adjust" in err and word in err, (kw, err)
    rc, err = _adjust(entry)
    assert rc == -1 and err == "null handle", err


def test_kl_set_steps_refuses_by_name_and_reaches_the_handle():
    L = _lib.lib()
    for bad, word in ((np.nan, "nan"), (np.inf, "inf"), (-np.inf, "-inf")):
        s = np.array([1.0, 0.5, bad, 2.0])
        assert L.ddp_kl_set_steps_f64(None, 4, _lib.ptr(s)) == -1
        err = L.ddp_last_error().decode()
        assert "kl_set_steps" in err and "steps[2]" in err and word in err and "not finite" in err, err
    s = np.ones(3)
    assert L.ddp_kl_set_steps_f64(None, 0, _lib.ptr(s)) == -1 and "B = 0" in L.ddp_last_error().decode()
    assert L.ddp_kl_set_steps_f64_dev(None, 0, _lib.ptr(s)) == -1 and "B = 0" in L.ddp_last_error().decode()
    for entry in ("ddp_kl_set_steps_f64", "ddp_kl_set_steps_f64_dev"):
        assert getattr(L, entry)(None, 3, _lib.ptr(s)) == -1 and L.ddp_last_error().decode() == "null handle"
        assert getattr(L, entry)(None, 0, None) == -1 and L.ddp_last_error().decode() == "null handle"      # NULL clears: B is not read


def test_python_refuses_wrong_shapes_without_a_device():
    c = er.case("4x2")
    pol = ddp_amd.GaussianPolicy(c["N"], 4, 2, c["K"], np.zeros((2, c["N"], 3)), c["Sg"], c["Sg"])
    E, ec = ddp_amd.DDPError, ddp_amd.expected_cost
    with pytest.raises(E, match="x, u should be"):
        ec(pol, None, c["x"][:, 0, 0], c["u"], c["model"], c["cost"])
    with pytest.raises(E, match="does not match"):
        ec(pol, None, c["x"], c["u"][:, :-1], c["model"], c["cost"])
    with pytest.raises(E, match="out of the box"):
        ec(pol, None, np.zeros((33, 7, 3)), c["u"], c["model"], c["cost"])
    with pytest.raises(E, match="out of the box"):
        ec(pol, None, c["x"], np.zeros((9, 7, 3)), c["model"], c["cost"])
    with pytest.raises(E, match="traj.K should be"):
        ec(ddp_amd.GaussianPolicy(7, 4, 2, c["K"][..., 0], None, None, None), None, c["x"], c["u"], c["model"], c["cost"])
    with pytest.raises(E, match="x0 should be"):
        ec(pol, np.zeros(5), c["x"], c["u"], c["model"], c["cost"])
    with pytest.raises(E, match="four arrays"):
        ec(pol, None, c["x"], c["u"], c["model"][:3], c["cost"])
    with pytest.raises(E, match="six arrays"):
        ec(pol, None, c["x"], c["u"], c["model"], c["cost"][:5])
    with pytest.raises(E, match="fu should be"):
        ec(pol, None, c["x"], c["u"], (c["model"][0], c["model"][1][:, :1], c["model"][2], None), c["cost"])
    with pytest.raises(E, match="c0 should be"):
        ec(pol, None, c["x"], c["u"], c["model"], c["cost"][:5] + (np.zeros(6),))
    with pytest.raises(E, match="fc is None"):
        ec(pol, None, c["x"], c["u"], c["model"][:2] + (None, None), c["cost"])
    with pytest.raises(E, match="Sigma0 should be"):
        ec(pol, None, c["x"], c["u"], c["model"], c["cost"], Sigma0=np.zeros((4, 5)))
    with pytest.raises(E, match="Sigma0 is not finite"):
        ec(pol, None, c["x"], c["u"], c["model"], c["cost"], Sigma0=np.full((4, 4), np.nan))
    with pytest.raises(E, match="three"):
        kl.kl_step_adjust(np.zeros((5, 3)), np.zeros((5, 2)), np.zeros((5, 3)), 1.0)
    with pytest.raises(E, match="scalar or B = 3"):
        kl.kl_step_adjust(np.zeros((5, 3)), np.zeros((5, 3)), np.zeros((5, 3)), np.ones(2))
    with pytest.raises(E, match="step_min"):
        kl.kl_step_adjust(np.zeros((5, 3)), np.zeros((5, 3)), np.zeros((5, 3)), 1.0, step_min=0.0)


def test_python_refuses_a_malformed_kl_step_vector_without_a_device():
    n, m, N, B = 4, 2, 6, 3
    prob = ddp_amd.LQProblem(np.eye(n), np.ones((n, m)), np.eye(n), np.eye(m))
    eye = np.repeat(np.repeat(np.eye(m)[:, :, None, None], N, 2), B, 3)
    pol = ddp_amd.GaussianPolicy(N, n, m, np.zeros((m, n, N, B)), np.zeros((m, N, B)), eye, eye.copy())
    model = kl.Model(np.zeros((n, n, N)), np.zeros((n, m, N)), np.eye(n))
    with pytest.raises(ddp_amd.DDPError, match="one step per trajectory"):
        kl.iLQGkl(prob, np.zeros((n, N, B)), pol, model, kl_step=np.ones(B + 1), cost=np.zeros(B))
    with pytest.raises(ddp_amd.DDPError, match=r"kl_step\[1\].*not finite"):
        kl.iLQGkl(prob, np.zeros((n, N, B)), pol, model, kl_step=np.array([1.0, np.nan, 1.0]), cost=np.zeros(B))
    pol1 = ddp_amd.GaussianPolicy(N, n, m, np.zeros((m, n, N)), np.zeros((m, N)), eye[..., 0], eye[..., 0].copy())
    with pytest.raises(ddp_amd.DDPError, match="one step per trajectory"):
        kl.iLQGkl(prob, np.zeros((n, N)), pol1, model, kl_step=np.ones(1), cost=0.0)
    with pytest.raises(NotImplementedError):
        kl.iLQGkl(prob, np.zeros((n, N, B)), pol, model, kl_step=np.ones(B), cost=np.zeros(B), constrain_per_step=True)


def test_kernel_uses_no_scratch():
    f = os.path.join(ROOT, "differentialdynamicprogramming.jl_amd", "build", "expect.o.usage.json")
    assert os.path.exists(f), "no build/expect.o.usage.json: build first"
    hit = [v for k, v in json.load(open(f)).items() if "ddp_expected_cost" in k]
    assert len(hit) >= 1, hit
    for u in hit:
        assert int(u["ScratchSize"]) == 0 and int(u["VGPRs Spill"]) == 0 and u["Dynamic Stack"] == "False", u
        assert int(u["LDS Size"]) <= 65536, u


# ------------------------------------------------------------------------------------------------------------------- the reference
EPS_LD = float(np.finfo(np.longdouble).eps)


def test_long_double_is_wider_than_double():
    assert EPS_LD < 2.0 ** -60, "np.longdouble is no wider than double here"


def test_reference_without_covariances_is_the_cost_along_a_deterministic_rollout():
    c = er.case("4x2-deterministic")
    r = c["ref"]
    n, m, N, B = c["n"], c["m"], c["N"], c["B"]
    fx, fu, fc, _ = c["model"]
    cx, cu, cxx, cxu, cuu, c0 = c["cost"]
    assert np.all(r["sigma"] == 0) and np.all(r["t"][4] == 0)
    for b in range(B):
        xh = c["x0"][:, b].copy()
        for i in range(N):
            dx = xh - c["x"][:, i, b]
            du = c["K"][:, :, i, b] @ dx
            uh = c["u"][:, i, b] + du
            q = c0[i, b] + cx[:, i, b] @ dx + cu[:, i, b] @ du + 0.5 * dx @ cxx[:, :, i, b] @ dx + dx @ cxu[:, :, i, b] @ du + 0.5 * du @ cuu[:, :, i, b] @ du
            assert abs(q - float(r["ec"][i, b])) <= 1e-13 * r["sec"][i, b], (i, b)
            assert np.allclose(np.concatenate([xh, uh]), r["mu"][:, i, b].astype(float), rtol=0, atol=1e-13 * r["smu"][i, b])
            xh = fx[:, :, i, b] @ xh + fu[:, :, i, b] @ uh + fc[:, i, b]


def test_reference_with_zero_gains_is_the_partial_sum_of_the_noise():
    """K = 0, time-invariant fx and cov, Σ = 0, Sigma0 = 0: Sx_i = sum_{j < i} fx^j cov fx^j'"""
    rng = np.random.default_rng(5)
    n, m, N, B = 5, 2, 6, 1
    A = 0.8 * np.linalg.qr(rng.standard_normal((n, n)))[0]
    C = er._spd(rng, n, 0.1)
    rep = lambda a: np.repeat(a[..., None], N, -1)[..., None]                            # noqa: E731
    c = er.designed(n, m, N, B, 6, no_sigma=True, no_sigma0=True)
    model = (rep(A), c["model"][1], c["model"][2], rep(C))
    r = er.recursion(np.zeros((m, n, N, B)), None, None, c["x"], c["u"], model, c["cost"], None)
    S, P = np.zeros((n, n)), np.eye(n)
    for i in range(N):
        assert np.allclose(r["sx"][:, :, i, 0].astype(float), S, rtol=0, atol=1e-14)
        assert np.allclose(r["sigma"][n:, :, i, 0].astype(float), 0) and np.allclose(r["sigma"][:n, :n, i, 0].astype(float), S, rtol=0, atol=1e-14)
        S = S + P @ C @ P.T
        P = A @ P


def test_reference_scalar_case_is_its_closed_form():
    """n = m = 1, K = 0, constant a, b, c, q (cov), s (Σ), cost 0.5 h x^2 + 0.5 r u^2 around x = u = 0: Sx_i = q (1 - a^2i) / (1 - a^2) +
    b^2 s (same sum) + a^2i S0, μx_i follows the affine map, ec_i = 0.5 h (μx_i^2 + Sx_i) + 0.5 r s"""
    a_, b_, c_, q, s, S0, h, r_ = 0.7, 0.3, 0.2, 0.05, 0.4, 0.25, 1.5, -0.6
    N = 8
    one = lambda v: np.full((1, 1, N, 1), v)                                             # noqa: E731
    vec = lambda v: np.full((1, N, 1), v)                                                # noqa: E731
    r = er.recursion(one(0.0), one(s), np.full((1, 1), 2.0), vec(0.0), vec(0.0), (one(a_), one(b_), vec(c_), one(q)),
                     (vec(0.0), vec(0.0), one(h), one(0.0), one(r_), np.zeros((N, 1))), np.full((1, 1, 1), S0))
    mu, S = 2.0, S0
    for i in range(N):
        assert abs(float(r["mu"][0, i, 0]) - mu) < 1e-14 and abs(float(r["sx"][0, 0, i, 0]) - S) < 1e-14
        geo = (1 - a_ ** (2 * i)) / (1 - a_ ** 2)
        assert abs(S - ((q + b_ * b_ * s) * geo + a_ ** (2 * i) * S0)) < 1e-14
        assert abs(float(r["ec"][i, 0]) - (0.5 * h * (mu * mu + S) + 0.5 * r_ * s)) < 1e-14
        mu, S = a_ * mu + c_, a_ * a_ * S + b_ * b_ * s + q


def test_reference_trace_term_is_the_explicit_double_loop():
    c = er.case("13x4-shared-model")
    r, (cx, cu, cxx, cxu, cuu, c0) = c["ref"], c["cost"]
    n, m = c["n"], c["m"]
    for b in range(c["B"]):
        for i in (0, 3, c["N"] - 1):
            H = np.block([[cxx[:, :, i, b], cxu[:, :, i, b]], [cxu[:, :, i, b].T, cuu[:, :, i, b]]])
            Sz = r["sigma"][:, :, i, b].astype(float)
            tr = 0.0
            for p in range(n + m):
                for q in range(n + m):
                    tr += H[p, q] * Sz[q, p]
            assert abs(0.5 * tr - float(r["t"][4, i, b])) <= 1e-13 * r["sec"][i, b]
            assert np.array_equal(Sz, Sz.T)


# ------------------------------------------------------------------------------------------- the condition on the GPU tests' inputs
@pytest.mark.parametrize("name", sorted(er.CASES))
def test_designed_cases_are_inside_the_growth_cap(name):
    c = er.case(name)
    r = c["ref"]
    n, m, N = c["n"], c["m"], c["N"]
    assert np.all(np.isfinite(r["ec"].astype(float)))
    print("%s: growth max %.2f, sec min / max %.3g" % (name, r["growth"].max(), r["sec"].min() / r["sec"].max()))
    assert r["growth"].max() <= er.GROWTH_CAP
    assert r["sec"].min() >= er.SEC_FLOOR * r["sec"].max()
    assert n + m <= 40 and N <= 33 and (n + m) * N * er.GROWTH_CAP * 2.0 ** -53 < er.TOL
    fx, fu = c["model"][0], c["model"][1]
    for b in range(c["B"]):
        for i in range(N):
            A = (fx[:, :, i, b] if fx.ndim == 4 else fx[:, :, i]) + (fu[:, :, i, b] if fu.ndim == 4 else fu[:, :, i]) @ c["K"][:, :, i, b]
            assert np.abs(np.linalg.eigvals(A)).max() <= 0.9 * (1 + 1e-12)
    for a in ((c["model"][3],) if c["model"][3] is not None else ()) + ((c["Sg"],) if c["Sg"] is not None else ()):
        a2 = a.reshape(a.shape[0], a.shape[1], -1)
        for k in range(a2.shape[2]):
            assert np.array_equal(a2[:, :, k], a2[:, :, k].T) and np.linalg.eigvalsh(a2[:, :, k]).min() > 0


def test_case_list_covers_the_axes():
    shapes = {v[:2] for v in er.CASES.values()}
    assert shapes == {(1, 1), (4, 2), (13, 4), (16, 1), (17, 8), (32, 8)}
    assert {v[2] for v in er.CASES.values()} == {1, 2, 7, 33} and er.CASES["4x2-N33"][:3] == (4, 2, 33)
    flags = set().union(*[set(k for k, on in v[3].items() if on) for v in er.CASES.values()])
    assert flags == {"model_shared", "cost_shared", "no_sigma", "no_cov", "no_sigma0", "given_x0"}


def test_step_rule_triples_are_inside_their_cancellation_cap():
    p, d, a, ks = er.step_triples()
    new, mult = er.step_rule(p, d, a, ks)
    seen = set()
    for b, (_, _, _, _, what) in enumerate(er.STEP_COLUMNS):
        with np.errstate(over="ignore", invalid="ignore"):
            J = [float(np.sum(v[:, b])) for v in (p, d, a)]
        if not all(np.isfinite(J)):
            assert mult[b] == 0.1 and new[b] == 0.1 * ks[b]
            seen.add("nonfinite")
            continue
        tot = sum(float(np.abs(v[:, b]).sum()) for v in (p, d, a))
        pred, act = J[0] - J[1], J[0] - J[2]
        assert abs(pred - act) >= er.STEP_CANCEL * tot, what
        raw = pred / (2 * max(1e-4, pred - act))
        if b not in er.STEP_MULT_EXACT:
            assert abs(pred) >= er.STEP_CANCEL * tot and 0.1 * 1.01 < raw < 5.0 / 1.01, what
            seen.add("interior")
        else:
            assert raw < 0.1 / 1.01 or raw > 5.0 * 1.01, what     # a clipped mult stays clipped under the rounding of the sums
            seen.add("low" if mult[b] == 0.1 else "high")
        if b in er.STEP_NEW_EXACT and b not in er.STEP_MULT_EXACT:
            assert ks[b] * raw < 1e-2 / 1.01 or ks[b] * raw > 1e2 * 1.01, what
        if pred - act < 1e-4:
            seen.add("floor")
        if new[b] == 1e-2:
            seen.add("step_min")
        if new[b] == 1e2:
            seen.add("step_max")
    assert seen >= {"nonfinite", "interior", "low", "high", "floor", "step_min", "step_max"}, seen
