"""DDP_USER_SAMPLE without a GPU: the flag, the program text (a problem without the flag compiles what it compiled before), the refused
combinations, the four new exports, and the reference generator of tests/sample_reference.py (known answers, moments, the seed the GPU
covariance test uses)."""
import os
import re

import numpy as np
import pytest

import ddp_amd
from ddp_amd import _lib

import sample_reference as sr
from conftest import ROOT

SAMPLE, TERMINAL, CONST_H, AUTODIFF, PLANT, SECOND, WAVE, SECOND_WAVE, CLOCK, CONSTRAINTS = 2048, 1, 2, 4, 8, 16, 32, 128, 512, 1024
NEW = ("ddp_normal_f64_dev", "ddp_normal_f64", "ddp_user_sample_f64_dev", "ddp_user_sample_f64")
LQ_NP = lambda n, m: 2 * n * n + n * m + m * m                    # noqa: E731

# (example, n, m, nparam, DeviceProblem keywords)
COMPILES = [("car", 4, 2, 9, dict(terminal=True)), ("car_ad", 4, 2, 9, dict(terminal=True, autodiff=True)),
            ("car_ad", 4, 2, 9, dict(terminal=True, autodiff=True, second_order=True)),
            ("car_plant", 4, 2, 13, dict(terminal=True, plant=True)), ("pendcart", 4, 1, 25, dict(terminal=True, diff=ddp_amd.WrappedDiff(0))),
            ("lq", 32, 8, LQ_NP(32, 8), dict(const_hessian=True)), ("lq_ad", 5, 3, LQ_NP(5, 3), dict(autodiff=True))]


def test_flag_value_everywhere():
    hdr = open(os.path.join(ROOT, "include", "ddp_amd.h")).read()
    jl = open(os.path.join(ROOT, "differentialdynamicprogramming.jl_amd", "julia", "DDPAmd.jl"), encoding="utf-8").read()
    assert _lib.USER_SAMPLE == 2048
    assert re.search(r"\bDDP_USER_SAMPLE = 2048\b", hdr)
    assert re.search(r"^const USER_SAMPLE = 2048\b", jl, flags=re.M)
    assert ddp_amd.DeviceProblem("", 1, 1, sample=True).flags == 2048 and ddp_amd.DeviceProblem("", 1, 1).flags == 0


def test_new_names_are_present():
    hdr = open(os.path.join(ROOT, "include", "ddp_amd.h")).read()
    jl = open(os.path.join(ROOT, "differentialdynamicprogramming.jl_amd", "julia", "DDPAmd.jl"), encoding="utf-8").read()
    L = _lib.lib()
    for name in NEW:
        assert name in _lib.EXPORTS and hasattr(L, name) and re.search(r"\b%s\s*\(" % name, hdr), name
    for name in ("ddp_normal_f64", "ddp_user_sample_f64"):
        assert "@ccall libddp.%s(" % name in jl, name
    assert "sample_policy" in ddp_amd.__all__ and "normal" in ddp_amd.__all__
    assert re.search(r"^function sample_policy\(", jl, flags=re.M) and re.search(r"^function normal\(", jl, flags=re.M)


@pytest.mark.parametrize("ex,n,m,nparam,kw", COMPILES, ids=["%s-%dx%d%s" % (c[0], c[1], c[2], "-ddp" if c[4].get("second_order") else "") for c in COMPILES])
def test_flag_compiles(ex, n, m, nparam, kw):
    ddp_amd.DeviceProblem(ddp_amd.example_source(ex), n, m, nparam=nparam, sample=True, **kw).check()


def _text(src, n, m, nparam, flags, wrap=0):
    t = _lib.lib().ddp_user_program_text(src.encode(), n, m, nparam, flags, wrap)
    return None if t is None else t.decode()


@pytest.mark.parametrize("ex,n,m,nparam,flags,wrap", [("car", 4, 2, 9, TERMINAL, 0), ("car_ad", 4, 2, 9, TERMINAL | AUTODIFF | SECOND, 0),
                                                     ("car_plant", 4, 2, 13, TERMINAL | PLANT, 0), ("pendcart", 4, 1, 25, TERMINAL, 1),
                                                     ("lq", 32, 8, LQ_NP(32, 8), CONST_H, 0), ("lq_ad", 5, 3, LQ_NP(5, 3), AUTODIFF, 0)])
def test_program_text_is_appended_only(ex, n, m, nparam, flags, wrap):
    src = ddp_amd.example_source(ex)
    base, with_flag = _text(src, n, m, nparam, flags, wrap), _text(src, n, m, nparam, flags | SAMPLE, wrap)
    assert base and with_flag and with_flag.startswith(base) and len(with_flag) > len(base)
    tail = with_flag[len(base):]
    assert "ddp_user_sample" in tail and "philox" in tail and "UserSampleArgs" in tail
    assert re.search(r"#define DDP_SLANES 64\b", tail) and re.search(r"#define DDP_SCHUNK \d+\b", tail)


def test_no_program_without_the_flag_mentions_the_sampler():
    lq = ddp_amd.example_source("lq_ad")
    chain = ddp_amd.example_source("chain_ad")
    keep = ddp_amd.example_source("car_keepout_ad")
    track = ddp_amd.example_source("car_track")
    texts = [_text(ddp_amd.example_source("car"), 4, 2, 9, TERMINAL), _text(lq, 5, 3, LQ_NP(5, 3), AUTODIFF | SECOND),
             _text(chain, 16, 8, 7, AUTODIFF | WAVE), _text(ddp_amd.example_source("chain_ddp_ad"), 24, 12, 8, AUTODIFF | WAVE | SECOND_WAVE),
             _text(track, 4, 2, 7 + 4 * 8, TERMINAL | CLOCK),
             _lib.lib().ddp_user_program_text_c(keep.encode(), 4, 2, 10, 2, TERMINAL | AUTODIFF | CONSTRAINTS, 0)]
    texts = [t.decode() if isinstance(t, bytes) else t for t in texts]
    assert all(texts), "arguments that are legal without the flag were refused: %s" % _lib.lib().ddp_last_error().decode()
    for t in texts:
        assert "ddp_user_sample" not in t and "philox" not in t.lower() and "DDP_SLANES" not in t


@pytest.mark.parametrize("ex,n,m,nparam,nc,flags,words", [
    ("chain_ad", 16, 8, 7, 0, SAMPLE | AUTODIFF | WAVE, ("DDP_USER_SAMPLE | DDP_USER_WAVE", "deferred")),
    ("chain_ddp_ad", 16, 8, 8, 0, SAMPLE | AUTODIFF | WAVE | SECOND_WAVE, ("DDP_USER_SAMPLE | DDP_USER_SECOND_ORDER_WAVE", "deferred")),
    ("car_track", 4, 2, 39, 0, SAMPLE | TERMINAL | CLOCK, ("DDP_USER_SAMPLE | DDP_USER_CLOCK", "deferred")),
    ("car_keepout_ad", 4, 2, 10, 2, SAMPLE | TERMINAL | AUTODIFF | CONSTRAINTS, ("DDP_USER_SAMPLE | DDP_USER_CONSTRAINTS", "deferred")),
    ("car", 4, 2, 9, 0, SAMPLE | 64, ("unknown flags",)), ("car", 4, 2, 9, 0, SAMPLE | 256, ("unknown flags",)),
    ("lq", 33, 8, LQ_NP(33, 8), 0, SAMPLE, ("n = 33",)), ("lq", 8, 9, LQ_NP(8, 9), 0, SAMPLE, ("m = 9",))])
def test_refused_by_name_before_compiling(ex, n, m, nparam, nc, flags, words):
    L = _lib.lib()
    src = ddp_amd.example_source(ex).encode()
    rc = L.ddp_user_check_c(src, n, m, nparam, nc, flags, None) if nc else L.ddp_user_check(src, n, m, nparam, flags, None)
    err = L.ddp_last_error().decode()
    assert rc == -1, (rc, err)                                   # -1: refused by validate(); the compiler (-4) was never asked
    for w in words:
        assert w in err, err


def test_python_refuses_what_it_can_without_a_device():
    with pytest.raises(ddp_amd.DDPError, match=r"2\^64"):
        ddp_amd.normal(1 << 64, 2, 3, 4)
    with pytest.raises(ddp_amd.DDPError, match=r"2\^64"):
        ddp_amd.normal(-1, 2, 3, 4)
    with pytest.raises(TypeError, match="DeviceProblem"):
        ddp_amd.sample_policy(ddp_amd.PendcartProblem(), ddp_amd.GaussianPolicy(), np.zeros(4), np.zeros((4, 3)), np.zeros((1, 3)), 2)


# ---------------------------------------------------------------------------------------------------------------- the reference generator
def test_philox_known_answers():
    """Random123's known-answer vectors of philox4x32-10 (its kat_vectors file): counter and key all zero, all ones, and the digits of
    pi.  No copy of that file was at hand when this was written: the three vectors are quoted from memory, so the assertion rests on
    that recollection plus the agreement of two independent implementations (this one, written from the paper, and csrc/philox.h, which
    the GPU tests compare with it)."""
    def words(c, k):
        return ["%08x" % int(v) for v in sr.philox4x32_10(*c, *k)]
    assert words((0, 0, 0, 0), (0, 0)) == ["6627e8d5", "e169c58d", "bc57ac4c", "9b00dbd8"]
    f = 0xFFFFFFFF
    assert words((f, f, f, f), (f, f)) == ["408f276d", "41c83b0e", "a20bc7c6", "6d5451fd"]
    assert words((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0)) == ["d16cfe09", "94fdcceb", "5001e420", "24126ea1"]


def test_normals_slices_and_odd_m():
    full = sr.normals(99, 3, 5, 9, 4)
    assert full.shape == (3, 5, 9, 4) and np.all(np.isfinite(full)) and np.max(np.abs(full)) <= 8.6
    assert np.array_equal(sr.normals(99, 3, 5, 4, 2, sample0=3, traj0=1), full[:, :, 3:7, 1:3])
    assert np.array_equal(sr.normals(99, 2, 5, 9, 4), full[:2])                      # the odd pair drops its second normal, nothing shifts
    assert not np.array_equal(sr.normals(99 + (1 << 32), 3, 5, 9, 4), full)          # the high seed word is part of the key


def test_normals_moments_and_lag_correlations():
    """2^18 normals of seed 12345: mean, variance, skewness, kurtosis and the lag-1 correlation along each of the four axes within 5
    standard errors of their sampling distributions (1/sqrt(n), sqrt(2/n), sqrt(6/n), sqrt(24/n), 1/sqrt(n))"""
    z = sr.normals(12345, 4, 16, 64, 64)
    n = z.size
    assert n == 1 << 18
    mu, var = z.mean(), z.var()
    zs = (z - mu) / np.sqrt(var)
    figures = {"mean": (abs(mu), 1 / np.sqrt(n)), "var": (abs(var - 1), np.sqrt(2 / n)), "skew": (abs(np.mean(zs ** 3)), np.sqrt(6 / n)),
               "kurt": (abs(np.mean(zs ** 4) - 3), np.sqrt(24 / n))}
    for ax in range(4):
        a, b = np.moveaxis(zs, ax, 0)[:-1], np.moveaxis(zs, ax, 0)[1:]
        figures["lag1 axis %d" % ax] = (abs(np.mean(a * b)), 1 / np.sqrt(a.size))
    for k, (v, se) in figures.items():
        print("%-12s %.3e  (%.2f standard errors)" % (k, v, v / se))
    for k, (v, se) in figures.items():
        assert v <= 5 * se, (k, v, se)


def test_the_seed_of_the_covariance_test_is_inside_the_bound_on_the_reference():
    c = sr.lq_cov_case()
    ok, err, se = sr.lq_cov_within(sr.lq_cov_reference_samples(c, sr.LQ_COV_SEED), c)
    assert ok.all(), (err / np.maximum(se, 1e-300)).max()
    assert np.all(c["cov"][:, :, 0] == 0) and np.all(se[:, :, 1:].reshape(9, -1).min(axis=0) > 0)


def test_reference_rollout_plant_differs_from_model():
    a, b = sr.reference("car_plant", False)[0], sr.reference("car_plant", True)[0]
    assert np.array_equal(a[:, 0], b[:, 0]) and np.max(np.abs(a[:, -1] - b[:, -1])) > 1e-2
