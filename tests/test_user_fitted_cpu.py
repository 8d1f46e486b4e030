"""DDP_USER_FITTED without a GPU: the flag, the four new exports, the program text (append-only, the fitted tail last; a problem without the
flag compiles what it compiled before), the compile report of ddp_user_rollout_fit, the refused combinations, what Python refuses before
it needs a device, and the reference of tests/fitted_reference.py (it converges on the inputs of the GPU loop tests; long double against
float64)."""
import os
import re

import numpy as np
import pytest

import ddp_amd
from ddp_amd import _lib, kl

import fitted_reference as fr
from conftest import ROOT, relerr

FITTED, SAMPLE, TERMINAL, CONST_H, AUTODIFF, PLANT, SECOND, WAVE, SECOND_WAVE, CLOCK, CONSTRAINTS = 4096, 2048, 1, 2, 4, 8, 16, 32, 128, 512, 1024
NEW = ("ddp_user_rollout_fit_f64_dev", "ddp_user_rollout_fit_f64", "ddp_user_ilqgkl_fit_f64_dev", "ddp_user_ilqgkl_fit_f64")
LQ_NP = lambda n, m: 2 * n * n + n * m + m * m                    # noqa: E731
HDR = os.path.join(ROOT, "include", "ddp_amd.h")
JL = os.path.join(ROOT, "differentialdynamicprogramming.jl_amd", "julia", "DDPAmd.jl")

COMPILES = [("car", 4, 2, 9, dict(terminal=True)), ("car_ad", 4, 2, 9, dict(terminal=True, autodiff=True)),
            ("car_plant", 4, 2, 13, dict(terminal=True, plant=True, sample=True)),
            ("pendcart", 4, 1, 25, dict(terminal=True, diff=ddp_amd.WrappedDiff(0))),
            ("lq", 32, 8, LQ_NP(32, 8), dict(const_hessian=True)), ("lq_ad", 5, 3, LQ_NP(5, 3), dict(autodiff=True))]


def test_flag_value_everywhere():
    hdr, jl = open(HDR).read(), open(JL, encoding="utf-8").read()
    assert _lib.USER_FITTED == 4096
    assert re.search(r"\bDDP_USER_FITTED = 4096\b", hdr)
    assert re.search(r"^const USER_FITTED = 4096\b", jl, flags=re.M)
    assert re.search(r"fitted::Bool=false", jl) and re.search(r"\(fitted \? USER_FITTED : 0\)", jl)
    assert ddp_amd.DeviceProblem("", 1, 1, fitted=True).flags == 4096 and ddp_amd.DeviceProblem("", 1, 1).flags == 0
    assert ddp_amd.DeviceProblem("", 1, 1, fitted=True, sample=True, terminal=True).flags == 4096 | 2048 | 1


def test_new_names_are_declared_exported_bound_and_called():
    hdr, jl = open(HDR).read(), open(JL, encoding="utf-8").read()
    L = _lib.lib()
    for name in NEW:
        assert name in _lib.EXPORTS and hasattr(L, name) and re.search(r"\b%s\s*\(" % name, hdr), name
        assert getattr(L, name).argtypes is not None, name
        assert "@ccall libddp.%s(" % name in jl, name
    import inspect
    assert "fitted" in inspect.signature(kl.iLQGkl).parameters and "model" in inspect.signature(ddp_amd.forward_pass).parameters
    assert kl.Model(1, 2, 3).fc is None and kl.Model(1, 2, 3, 4).fc == 4


@pytest.mark.parametrize("ex,n,m,nparam,kw", COMPILES, ids=["%s-%dx%d" % c[:3] for c in COMPILES])
def test_flag_compiles(ex, n, m, nparam, kw):
    ddp_amd.DeviceProblem(ddp_amd.example_source(ex), n, m, nparam=nparam, fitted=True, **kw).check()


def test_car_table_compiles():
    ddp_amd.DeviceProblem(ddp_amd.example_source("car_table"), 4, 2, nparam=9 + 28 * 40, terminal=True).check()


def _usage(log, kernel):
    """the figures of one kernel from the kernel-resource-usage remarks of a hiprtc log"""
    out, cur = {}, None
    for line in log.splitlines():
        mm = re.search(r"remark: Function Name: (\w+)", line)
        if mm:
            cur = mm.group(1)
        mm = re.search(r"remark:\s+([A-Za-z][\w \[\]/]*): (\d+)", line)
        if mm and cur == kernel and "Function Name" not in mm.group(1):
            out[mm.group(1).strip()] = int(mm.group(2))
    return out


@pytest.mark.parametrize("ex,n,m,nparam,kw", [("car", 4, 2, 9, dict(terminal=True)), ("lq", 10, 2, LQ_NP(10, 2), {}),
                                              ("lq", 32, 8, LQ_NP(32, 8), dict(const_hessian=True))], ids=["4x2", "10x2", "32x8"])
def test_rollout_fit_has_no_scratch_and_no_spill(ex, n, m, nparam, kw):
    log = ddp_amd.DeviceProblem(ddp_amd.example_source(ex), n, m, nparam=nparam, fitted=True, **kw).check("-Rpass-analysis=kernel-resource-usage")
    u = _usage(log, "ddp_user_rollout_fit")
    print(u)
    assert u["ScratchSize [bytes/lane]"] == 0 and u["VGPRs Spill"] == 0, u
    assert u["LDS Size [bytes/block]"] <= 64 * 1024, u


def _text(src, n, m, nparam, flags, wrap=0):
    t = _lib.lib().ddp_user_program_text(src.encode(), n, m, nparam, flags, wrap)
    return None if t is None else t.decode()


TEXTS = [("car", 4, 2, 9, TERMINAL, 0), ("car_ad", 4, 2, 9, TERMINAL | AUTODIFF | SECOND, 0), ("car_plant", 4, 2, 13, TERMINAL | PLANT, 0),
         ("pendcart", 4, 1, 25, TERMINAL, 1), ("lq", 32, 8, LQ_NP(32, 8), CONST_H, 0), ("lq_ad", 5, 3, LQ_NP(5, 3), AUTODIFF, 0)]


@pytest.mark.parametrize("sample", [0, SAMPLE], ids=["plain", "sample"])
@pytest.mark.parametrize("ex,n,m,nparam,flags,wrap", TEXTS, ids=[t[0] for t in TEXTS])
def test_program_text_is_appended_only(ex, n, m, nparam, flags, wrap, sample):
    src = ddp_amd.example_source(ex)
    base, with_flag = _text(src, n, m, nparam, flags | sample, wrap), _text(src, n, m, nparam, flags | sample | FITTED, wrap)
    assert base and with_flag and with_flag.startswith(base) and len(with_flag) > len(base)
    tail = with_flag[len(base):]
    assert "ddp_user_rollout_fit" in tail and "UserRollFitArgs" in tail and "ddp_user_sample" not in tail
    lanes, chunk = int(re.search(r"#define DDP_FLANES (\d+)\b", tail).group(1)), int(re.search(r"#define DDP_FCHUNK (\d+)\b", tail).group(1))
    ps, ts = 2 * m + m * n + n, n * n + n * m + n
    assert 1 <= lanes <= 64 and chunk >= 1 and lanes * (((chunk * ps) | 1) + ((chunk * ts) | 1) + 1) * 8 <= 64 * 1024
    assert "ddp_user_rollout_fit" not in base and "DDP_FLANES" not in base


def test_no_program_without_the_flag_mentions_the_fitted_rollout():
    texts = [_text(ddp_amd.example_source("car"), 4, 2, 9, TERMINAL), _text(ddp_amd.example_source("car"), 4, 2, 9, TERMINAL | SAMPLE),
             _text(ddp_amd.example_source("lq_ad"), 5, 3, LQ_NP(5, 3), AUTODIFF | SECOND),
             _text(ddp_amd.example_source("chain_ad"), 16, 8, 7, AUTODIFF | WAVE),
             _text(ddp_amd.example_source("chain_ddp_ad"), 24, 12, 8, AUTODIFF | WAVE | SECOND_WAVE),
             _text(ddp_amd.example_source("car_track"), 4, 2, 7 + 4 * 8, TERMINAL | CLOCK),
             _lib.lib().ddp_user_program_text_c(ddp_amd.example_source("car_keepout_ad").encode(), 4, 2, 10, 2, TERMINAL | AUTODIFF | CONSTRAINTS, 0)]
    texts = [t.decode() if isinstance(t, bytes) else t for t in texts]
    assert all(texts), "arguments that are legal without the flag were refused: %s" % _lib.lib().ddp_last_error().decode()
    for t in texts:
        assert "ddp_user_rollout_fit" not in t and "DDP_FLANES" not in t and "DDP_FCHUNK" not in t and "UserRollFitArgs" not in t


@pytest.mark.parametrize("ex,n,m,nparam,nc,flags,words", [
    ("chain_ad", 16, 8, 7, 0, FITTED | AUTODIFF | WAVE, ("DDP_USER_FITTED | DDP_USER_WAVE", "deferred", "n <= 32", "m <= 8")),
    ("chain_ddp_ad", 16, 8, 8, 0, FITTED | AUTODIFF | WAVE | SECOND_WAVE, ("DDP_USER_FITTED | DDP_USER_SECOND_ORDER_WAVE", "deferred", "n <= 32")),
    ("car_track", 4, 2, 39, 0, FITTED | TERMINAL | CLOCK, ("DDP_USER_FITTED | DDP_USER_CLOCK", "deferred", "no clock")),
    ("car_keepout_ad", 4, 2, 10, 2, FITTED | TERMINAL | AUTODIFF | CONSTRAINTS, ("DDP_USER_FITTED | DDP_USER_CONSTRAINTS", "deferred", "no multipliers")),
    ("car", 4, 2, 9, 0, FITTED | 64, ("unknown flags",)), ("car", 4, 2, 9, 0, FITTED | 256, ("unknown flags",)),
    ("lq", 33, 8, LQ_NP(33, 8), 0, FITTED, ("n = 33",)), ("lq", 8, 9, LQ_NP(8, 9), 0, FITTED, ("m = 9",))])
def test_refused_by_name_before_compiling(ex, n, m, nparam, nc, flags, words):
    L = _lib.lib()
    src = ddp_amd.example_source(ex).encode()
    rc = L.ddp_user_check_c(src, n, m, nparam, nc, flags, None) if nc else L.ddp_user_check(src, n, m, nparam, flags, None)
    err = L.ddp_last_error().decode()
    assert rc == -1, (rc, err)                                   # -1: refused by validate(); the compiler (-4) was never asked
    for w in words:
        assert w in err, err


@pytest.fixture(scope="module")
def case():
    return fr.loop_case()


def _call(case, problem, model, **kw):
    B, N = case["B"], case["N"]
    prev = ddp_amd.GaussianPolicy(N, 4, 2, case["Kp"], case["u"], case["Sp"], case["Sip"])
    return kl.iLQGkl(problem, case["x"], prev, model, kl_step=0.5, max_iter=20, cost=case["c"], **kw)


def test_python_refuses_what_it_can_without_a_device(case):
    src = ddp_amd.example_source("car")
    plain = ddp_amd.DeviceProblem(src, 4, 2, nparam=9, terminal=True, params=case["P"])
    fit = ddp_amd.DeviceProblem(src, 4, 2, nparam=9, terminal=True, params=case["P"], fitted=True)
    fx, fu, fc, R1 = case["fx"], case["fu"], case["fc"], case["R1"]
    with pytest.raises(ddp_amd.DDPError, match=r"made with fitted=True"):
        _call(case, plain, kl.Model(fx, fu, R1, fc), fitted=True)
    with pytest.raises(ddp_amd.DDPError, match=r"model\.fc"):
        _call(case, fit, kl.Model(fx, fu, R1), fitted=True)
    with pytest.raises(ddp_amd.DDPError, match=r"model\.fx, model\.fu"):
        _call(case, fit, kl.Model(fx, None, R1, fc), fitted=True)
    with pytest.raises(ddp_amd.DDPError, match=r"fx, fu, fc should be"):
        _call(case, fit, kl.Model(fx, fu[:, :1], R1, fc), fitted=True)
    with pytest.raises(ddp_amd.DDPError, match=r"fx, fu, fc should be"):
        _call(case, fit, kl.Model(fx, fu, R1, fc[:, :-1]), fitted=True)
    with pytest.raises(ddp_amd.DDPError, match=r"one set of tables per trajectory"):
        _call(case, fit, kl.Model(fx[..., 0], fu[..., 0], R1, fc[..., 0]), fitted=True)
    bad = fu.copy(); bad[1, 0, 17, 2] = np.nan; bad[0, 0, 30, 2] = np.nan
    with pytest.raises(ddp_amd.DDPError, match=r"model\.fu is not finite at step 17 of trajectory 2"):
        _call(case, fit, kl.Model(fx, bad, R1, fc), fitted=True)
    with pytest.raises(ddp_amd.DDPError, match=r"wide=True"):
        _call(case, fit, kl.Model(fx, fu, R1, fc), fitted=True, wide=True)
    so = ddp_amd.DeviceProblem(ddp_amd.example_source("car_ad"), 4, 2, nparam=9, terminal=True, autodiff=True, second_order=True, fitted=True,
                               params=case["P"])
    with pytest.raises(ddp_amd.DDPError, match=r"second_order=True is refused"):
        _call(case, so, kl.Model(fx, fu, R1, fc), fitted=True)
    with pytest.raises(ddp_amd.DDPError, match=r"made with fitted=True"):
        ddp_amd.forward_pass(None, case["x0"], case["u"], None, 1.0, plain, None, model=(fx, fu, fc))
    with pytest.raises(ddp_amd.DDPError, match=r"fx, fu, fc should be"):
        ddp_amd.forward_pass(None, case["x0"], case["u"], None, 1.0, fit, None, model=(fx, fu, fc[:, :, :2]))
    with pytest.raises(ddp_amd.DDPError, match=r"made with fitted=True"):
        ddp_amd.forward_pass(None, np.ones(2), np.zeros((1, 3)), None, 1.0, ddp_amd.LQProblem(np.eye(2), np.ones((2, 1)), np.eye(2), np.eye(1)),
                             None, model=(fx, fu, fc))


@pytest.mark.parametrize("lims", [None, "on"])
def test_the_reference_converges_on_the_inputs_of_the_gpu_loop_test(case, lims):
    """the condition that keeps the GPU loop test from hiding a failure behind max_iter: status 1 within max_iter = 20 on every trajectory"""
    L = None if lims is None else np.array([[-1.0, 1.0], [-0.8, 0.8]])
    for b in range(case["B"]):
        info = fr.np_loop(case, b, L)[6]
        print(b, info["status"], info["iter"], info["n_backpass"])
        assert info["status"] == 1 and info["iter"] < 20, (b, info["status"], info["iter"])


def test_the_nominal_of_the_loop_case_is_consistent_with_its_tables(case):
    x, u, fx, fu, fc = case["x"], case["u"], case["fx"], case["fu"], case["fc"]
    for i in range(case["N"] - 1):
        nxt = np.einsum("ijb,jb->ib", fx[:, :, i], x[:, i]) + np.einsum("iqb,qb->ib", fu[:, :, i], u[:, i]) + fc[:, i]
        assert np.max(np.abs(nxt - x[:, i + 1])) < 1e-12


def test_long_double_rollout_against_float64():
    rng = np.random.default_rng(5)
    n, m, N = 5, 3, 40
    fx, fu, fc = (a[..., 0] for a in fr.designed_tables(rng, n, m, N, 1))
    Q, R = fr._spd(rng, n), fr._spd(rng, m)
    stage, _ = fr.lq_cost(Q, R)
    x0, u, xn = rng.standard_normal(n), 0.3 * rng.standard_normal((m, N)), rng.standard_normal((n, N))
    K, k = 0.1 * rng.standard_normal((m, n, N)), 0.1 * rng.standard_normal((m, N))
    L = np.stack([-0.4 * np.ones(m), 0.5 * np.ones(m)], 1)
    kw = dict(K=K, k=k, x=xn, alpha=0.5, lims=L, wrap=0b10)
    a = fr.rollout(x0, u, fx, fu, fc, stage, None, **kw)
    b = fr.rollout(x0, u, fx, fu, fc, stage, None, dtype=np.float64, **kw)
    assert a[0].dtype == np.longdouble and b[0].dtype == np.float64
    for p, q in zip(a, b):
        assert relerr(q, p.astype(float), -1 if p.ndim == 2 else 0) < 1e-12
    fx2 = fx.copy(); fx2[:, :, N - 1] = np.nan                  # slot N-1 is never read
    c = fr.rollout(x0, u, fx2, fu, fc, stage, None, **kw)
    assert all(np.array_equal(p, q) for p, q in zip(a, c))
