"""DDP_USER_SAMPLE_WAVE without a GPU: the flag (value, program text appended last and only under the flag, refusals by name before any
compile), the cross-compile of ddp_user_sample_wave at the shapes of tests/sample_wave_cases.py with its resources, and the conditions on
the long double references that the GPU tests (tests/test_gpu_user_sample_wave.py) rely on."""
import os
import re

import numpy as np
import pytest

import ddp_amd
from ddp_amd import _lib

import sample_wave_cases as wc
from conftest import ROOT
from test_user_wave_cpu import CHAIN_P, chain_closures

SAMPLE_WAVE, SAMPLE, TERMINAL, CONST_H, AUTODIFF, PLANT, WAVE, SECOND_WAVE, CLOCK, CONSTRAINTS = 16384, 2048, 1, 2, 4, 8, 32, 128, 512, 1024
LQ_NP = lambda n, m: 2 * n * n + n * m + m * m                    # noqa: E731

# (example, n, m, nparam, flags without DDP_USER_SAMPLE_WAVE, diff_wrap)
PROGRAMS = [("chain_plant_ad", 64, 32, 9, AUTODIFF | PLANT | WAVE, 0), ("chain_ad", 34, 17, 7, AUTODIFF | WAVE, 0),
            ("lq", 33, 2, LQ_NP(33, 2), WAVE, 0), ("lq", 10, 9, LQ_NP(10, 9), WAVE | CONST_H, 0),
            ("pendcart_ad", 4, 1, 25, TERMINAL | AUTODIFF | WAVE, 1),
            ("chain_ddp_ad", 24, 12, 8, AUTODIFF | WAVE | SECOND_WAVE, 0)]


def _text(src, n, m, nparam, flags, wrap=0):
    t = _lib.lib().ddp_user_program_text(src.encode(), n, m, nparam, flags, wrap)
    return None if t is None else t.decode()


# ------------------------------------------------------------------------------------------------------------------------ the flag
def test_flag_value_everywhere():
    hdr = open(os.path.join(ROOT, "include", "ddp_amd.h")).read()
    jl = open(os.path.join(ROOT, "differentialdynamicprogramming.jl_amd", "julia", "DDPAmd.jl"), encoding="utf-8").read()
    assert _lib.USER_SAMPLE_WAVE == 16384
    assert re.search(r"\bDDP_USER_SAMPLE_WAVE = 16384\b", hdr)
    assert re.search(r"^const USER_SAMPLE_WAVE = 16384\b", jl, flags=re.M) and "sample_wave::Bool=false" in jl
    assert ddp_amd.DeviceProblem("", 1, 1, wave=True, sample_wave=True).flags == 16384 | 32
    assert ddp_amd.DeviceProblem("", 1, 1, wave=True).flags == 32
    assert len(_lib.EXPORTS) == len(set(_lib.EXPORTS)) and _lib.SAMPLE_EXPORTS[-1] == "ddp_user_sample_f64"     # (no new entry point)


def test_python_refuses_the_flag_without_wave_in_the_words_of_the_library():
    with pytest.raises(ddp_amd.DDPError, match="DDP_USER_SAMPLE_WAVE needs DDP_USER_WAVE"):
        ddp_amd.DeviceProblem("", 1, 1, sample_wave=True)
    rc = _lib.lib().ddp_user_check(ddp_amd.example_source("chain_ad").encode(), 16, 8, 7, AUTODIFF | SAMPLE_WAVE, None)
    assert rc == -1 and "DDP_USER_SAMPLE_WAVE needs DDP_USER_WAVE" in _lib.lib().ddp_last_error().decode()


@pytest.mark.parametrize("ex,n,m,nparam,flags,wrap", PROGRAMS, ids=["%s-%dx%d" % p[:3] for p in PROGRAMS])
def test_program_text_is_appended_last_and_only_under_the_flag(ex, n, m, nparam, flags, wrap):
    src = ddp_amd.example_source(ex)
    base, with_flag = _text(src, n, m, nparam, flags, wrap), _text(src, n, m, nparam, flags | SAMPLE_WAVE, wrap)
    assert base and with_flag and with_flag.startswith(base) and len(with_flag) > len(base)
    tail = with_flag[len(base):]
    assert "ddp_user_sample_wave" in tail and "UserSampleArgs" in tail and "philox" in tail
    assert "ddp_user_sample_wave" not in base and "philox" not in base.lower()


def test_no_program_without_the_flag_mentions_the_kernel():
    car = ddp_amd.example_source("car")
    texts = [_text(car, 4, 2, 9, TERMINAL), _text(car, 4, 2, 9, TERMINAL | SAMPLE),
             _text(ddp_amd.example_source("lq"), 32, 8, LQ_NP(32, 8), SAMPLE | 4096 | 8192),
             _text(ddp_amd.example_source("chain_ad"), 16, 8, 7, AUTODIFF | WAVE),
             _text(ddp_amd.example_source("car_track"), 4, 2, 7 + 4 * 8, TERMINAL | CLOCK)]
    assert all(texts), _lib.lib().ddp_last_error().decode()
    for t in texts:
        assert "ddp_user_sample_wave" not in t and "DDP_SWS" not in t


@pytest.mark.parametrize("ex,n,m,nparam,nc,flags,words", [
    ("chain_ad", 16, 8, 7, 0, SAMPLE_WAVE | AUTODIFF, ("DDP_USER_SAMPLE_WAVE needs DDP_USER_WAVE",)),
    ("car_track", 4, 2, 39, 0, SAMPLE_WAVE | WAVE | TERMINAL | CLOCK, ("DDP_USER_SAMPLE_WAVE | DDP_USER_CLOCK", "deferred")),
    ("car_keepout_ad", 4, 2, 10, 2, SAMPLE_WAVE | WAVE | TERMINAL | AUTODIFF | CONSTRAINTS, ("DDP_USER_SAMPLE_WAVE | DDP_USER_CONSTRAINTS", "deferred")),
    ("chain_ad", 16, 8, 7, 0, SAMPLE_WAVE | SAMPLE | WAVE | AUTODIFF, ("DDP_USER_SAMPLE | DDP_USER_WAVE", "deferred")),
    ("lq", 65, 8, LQ_NP(65, 8), 0, SAMPLE_WAVE | WAVE, ("n = 65",)), ("lq", 8, 33, LQ_NP(8, 33), 0, SAMPLE_WAVE | WAVE, ("m = 33",)),
    ("chain_ad", 16, 8, 7, 0, SAMPLE_WAVE | WAVE | AUTODIFF | 32768, ("unknown flags",)),
    ("chain_ad", 16, 8, 7, 0, SAMPLE_WAVE | WAVE | AUTODIFF | 64, ("unknown flags",)),
    ("chain_ad", 16, 8, 7, 0, SAMPLE_WAVE | WAVE | AUTODIFF | 256, ("unknown flags",))],
    ids=["no-wave", "clock", "constraints", "sample", "n65", "m33", "bit32768", "bit64", "bit256"])
def test_refused_by_name_before_compiling(ex, n, m, nparam, nc, flags, words):
    L = _lib.lib()
    src = ddp_amd.example_source(ex).encode()
    rc = L.ddp_user_check_c(src, n, m, nparam, nc, flags, None) if nc else L.ddp_user_check(src, n, m, nparam, flags, None)
    err = L.ddp_last_error().decode()
    assert rc == -1, (rc, err)                                   # -1: refused by validate(); the compiler (-4) was never asked
    for w in words:
        assert w in err, err


def test_the_plant_example_is_the_chain_with_a_plant():
    chain, plant = ddp_amd.example_source("chain_ad"), ddp_amd.example_source("chain_plant_ad")
    body = chain[chain.index("template <class T> __device__ void dynamics"):]
    assert body in plant and "__device__ void plant(" in plant and "__device__ void plant(" not in chain
    assert "chain_plant_ad" in ddp_amd.example_source.__doc__


# ------------------------------------------------------------------------------------------------------------------- compile only
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


@pytest.mark.parametrize("name", ["chain_plant_64x32", "chain_34x17", "lq_33x2", "lq_10x9", "pendcart_4x1"])
def test_flag_compiles_without_more_scratch_than_the_wave_rollout_and_within_its_lds(name):
    c = wc.case(name)
    n, m = c["n"], c["m"]
    diff = ddp_amd.WrappedDiff(*c["wrap"]) if c["wrap"] else None
    log = ddp_amd.DeviceProblem(ddp_amd.example_source(c["example"]), n, m, nparam=c["nparam"], wave=True, sample_wave=True, diff=diff,
                                **c["kw"]).check("-Rpass-analysis=kernel-resource-usage")
    u, r = _usage(log, "ddp_user_sample_wave"), _usage(log, "ddp_user_rollout_wave")
    print(name, u)
    assert u and r, log[:2000]
    assert u["ScratchSize [bytes/lane]"] <= r["ScratchSize [bytes/lane]"] and u["VGPRs Spill"] == 0, (u, r)
    # the launch asks for no dynamic LDS: the kernel's own array is all there is, SPW samples of x̂, dx, x̂⁺, û, ξ at an odd stride
    want = c["spw"] * ((3 * n + 2 * m) | 1) * 8
    assert want <= u["LDS Size [bytes/block]"] <= want + 64 and u["LDS Size [bytes/block]"] <= 64 * 1024, (u, want)


# ----------------------------------------------------------------------------------------------- what the GPU tests take for granted
def test_the_table_covers_the_sizes():
    cs = [wc.case(k) for k in wc.NAMES]
    assert [(c["n"], c["m"], c["wg"]) for c in cs] == [(64, 32, 32), (34, 17, 32), (40, 12, 16), (33, 2, 8), (10, 9, 16), (4, 1, 8), (16, 8, 8)]
    assert {c["S"] for c in cs} >= {1, 5, 65} and {c["N"] for c in cs} >= {1} and {c["B"] for c in cs} == {1, 3}
    assert {c["S"] - c["spw"] for c in cs} >= {-1, 0, 1}
    assert all(1 <= c["N"] <= 9 for c in cs)
    for c in cs:                                                  # Σ positive definite with off-diagonal terms
        Sg = np.moveaxis(c["Sigma"], (0, 1), (-2, -1))
        assert np.all(np.linalg.eigvalsh(Sg) > 0) and (c["m"] == 1 or np.min(np.abs(Sg[..., 1, 0])) > 0)


@pytest.mark.parametrize("name", wc.NAMES)
def test_reference_rollouts_are_finite(name):
    c = wc.case(name)
    for plant in ((False, True) if c["kw"].get("plant") else (False,)):
        xs, us, cs = wc.reference(name, plant)
        assert xs.shape == (c["n"], c["N"], c["S"], c["B"]) and cs.shape[0] == c["N"] + bool(c["kw"].get("terminal"))
        assert all(np.all(np.isfinite(a)) for a in (xs, us, cs))
        assert np.max(np.abs(xs)) < 50                            # (K of moderate gain: the closed loop stays bounded)
    if c["kw"].get("plant"):
        assert np.max(np.abs(wc.reference(name, True)[0][:, -1] - wc.reference(name, False)[0][:, -1])) > 1e-3     # another system


def test_the_limits_act_on_some_controls_not_on_all():
    c = wc.case("lq_ad_40x12")
    ru = wc.reference("lq_ad_40x12")[1]
    hit = (ru == c["lims"][:, 0, None, None, None]) | (ru == c["lims"][:, 1, None, None, None])
    assert 0.02 < hit.mean() < 0.9, hit.mean()


def test_the_wrap_case_crosses_the_wrap():
    c = wc.case("pendcart_4x1")
    rx = wc.reference("pendcart_4x1")[0]
    d = rx[0] - c["x"][0][:, None, :]                            # [N, S, B]
    assert np.any(d > np.pi) and np.any(d < -np.pi) and np.any(np.abs(d) < 1)
    assert np.any(rx[0] > np.pi) and np.any(rx[0] < np.pi)       # samples on both sides of π


def test_long_double_chain_matches_the_float64_closures():
    rng = np.random.default_rng(5)
    for J in (8, 17, 32):
        f, cost, _, plant = wc.chain_model(J)
        f64, cost64, _ = chain_closures(CHAIN_P, J)
        x, u = rng.standard_normal((2 * J, 4)), rng.standard_normal((J, 4))
        p = np.concatenate([CHAIN_P, [1.0, CHAIN_P[2]]]).astype(wc.LD)
        xn = f(x.astype(wc.LD), u.astype(wc.LD), 0, p)
        ref = np.stack([f64(x[:, s], u[:, s], 0) for s in range(4)], axis=1)
        assert np.max(np.abs(xn - ref)) <= 1e-12 * max(1.0, np.max(np.abs(ref)))
        assert np.max(np.abs(cost(x.astype(wc.LD), u.astype(wc.LD), 0, p) - cost64(x, u))) <= 1e-12 * np.max(np.abs(cost64(x, u)))
        # the plant with gain 1 at every joint and the model's damping is the model but for the per-joint gain
        g = 1 / (1 + 0.05 * np.arange(J))
        assert np.max(np.abs(plant(x.astype(wc.LD), u.astype(wc.LD), 0, p) - f(x.astype(wc.LD), (g[:, None] * u).astype(wc.LD), 0, p))) < 1e-15
