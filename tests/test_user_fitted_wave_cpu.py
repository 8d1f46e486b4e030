"""DDP_USER_FITTED_WAVE without a GPU: the flag (value, program text appended last and only under the flag, refusals by name before any
compile), the cross-compile of ddp_user_rollout_fit_wave with its resources, the Python refusals that need no device, and the conditions on
the references of the whole-loop cases that the GPU tests (tests/test_gpu_user_fitted_wave.py) rely on."""
import os
import re

import numpy as np
import pytest

import ddp_amd
from ddp_amd import _lib, kl

import fitted_wave_cases as fw
import kl_wide_cases as kc
from conftest import ROOT
from test_user_sample_wave_cpu import LQ_NP, PROGRAMS, _text, _usage

FITTED_WAVE, SAMPLE_WAVE, FITTED, TERMINAL, AUTODIFF, WAVE, CLOCK, CONSTRAINTS = 65536, 16384, 4096, 1, 4, 32, 512, 1024
KERNEL = "ddp_user_rollout_fit_wave"


# ------------------------------------------------------------------------------------------------------------------------ the flag
def test_flag_value_everywhere():
    hdr = open(os.path.join(ROOT, "include", "ddp_amd.h")).read()
    jl = open(os.path.join(ROOT, "differentialdynamicprogramming.jl_amd", "julia", "DDPAmd.jl"), encoding="utf-8").read()
    assert _lib.USER_FITTED_WAVE == 65536
    assert re.search(r"\bDDP_USER_FITTED_WAVE = 65536\b", hdr)
    assert re.search(r"^const USER_FITTED_WAVE = 65536\b", jl, flags=re.M) and "fitted_wave::Bool=false" in jl
    assert ddp_amd.DeviceProblem("", 1, 1, wave=True, fitted_wave=True).flags == 65536 | 32
    assert ddp_amd.DeviceProblem("", 1, 1, wave=True).flags == 32
    # no new entry point: the literal count of the parent commit, and the fitted entries are the ones that were there
    assert len(_lib.EXPORTS) == len(set(_lib.EXPORTS)) == N_EXPORTS
    assert not [e for e in _lib.EXPORTS if "fit_wave" in e or "fitted_wave" in e]


N_EXPORTS = 127


def test_python_refuses_the_flag_without_wave_in_the_words_of_the_library():
    with pytest.raises(ddp_amd.DDPError, match="DDP_USER_FITTED_WAVE needs DDP_USER_WAVE"):
        ddp_amd.DeviceProblem("", 1, 1, fitted_wave=True)
    rc = _lib.lib().ddp_user_check(ddp_amd.example_source("chain_ad").encode(), 16, 8, 7, AUTODIFF | FITTED_WAVE, None)
    assert rc == -1 and "DDP_USER_FITTED_WAVE needs DDP_USER_WAVE" in _lib.lib().ddp_last_error().decode()


@pytest.mark.parametrize("ex,n,m,nparam,nc,flags,words", [
    ("chain_ad", 16, 8, 7, 0, FITTED_WAVE | AUTODIFF, ("DDP_USER_FITTED_WAVE needs DDP_USER_WAVE",)),
    ("car_track", 4, 2, 39, 0, FITTED_WAVE | WAVE | TERMINAL | CLOCK, ("DDP_USER_FITTED_WAVE | DDP_USER_CLOCK", "deferred", "takes no clock")),
    ("car_keepout_ad", 4, 2, 10, 2, FITTED_WAVE | WAVE | TERMINAL | AUTODIFF | CONSTRAINTS,
     ("DDP_USER_FITTED_WAVE | DDP_USER_CONSTRAINTS", "deferred", "takes no multipliers")),
    ("chain_ad", 16, 8, 7, 0, FITTED_WAVE | FITTED | WAVE | AUTODIFF,
     ("DDP_USER_FITTED | DDP_USER_WAVE is refused (deferred: ddp_user_rollout_fit is sized for n <= 32, m <= 8)",)),
    ("chain_ad", 16, 8, 7, 0, FITTED_WAVE | WAVE | AUTODIFF | 32768, ("unknown flags",)),
    ("chain_ad", 16, 8, 7, 0, FITTED_WAVE | WAVE | AUTODIFF | 64, ("unknown flags",)),
    ("chain_ad", 16, 8, 7, 0, FITTED_WAVE | WAVE | AUTODIFF | 256, ("unknown flags",)),
    ("lq", 65, 8, LQ_NP(65, 8), 0, FITTED_WAVE | WAVE, ("n = 65",)), ("lq", 8, 33, LQ_NP(8, 33), 0, FITTED_WAVE | WAVE, ("m = 33",))],
    ids=["no-wave", "clock", "constraints", "fitted", "bit32768", "bit64", "bit256", "n65", "m33"])
def test_refused_by_name_before_compiling(ex, n, m, nparam, nc, flags, words):
    L = _lib.lib()
    src = ddp_amd.example_source(ex).encode()
    rc = L.ddp_user_check_c(src, n, m, nparam, nc, flags, None) if nc else L.ddp_user_check(src, n, m, nparam, flags, None)
    err = L.ddp_last_error().decode()
    assert rc == -1, (rc, err)                                   # -1: refused by validate(); the compiler (-4) was never asked
    for w in words:
        assert w in err, err


def test_the_pinned_refusal_of_fitted_with_wave_keeps_its_words():
    """the message of DDP_USER_FITTED | DDP_USER_WAVE with the new flag next to it is the message without it"""
    L = _lib.lib()
    src = ddp_amd.example_source("chain_ad").encode()
    msgs = []
    for extra in (0, FITTED_WAVE):
        assert L.ddp_user_check(src, 16, 8, 7, FITTED | WAVE | AUTODIFF | extra, None) == -1
        msgs.append(L.ddp_last_error().decode())
    assert msgs[0] == msgs[1] and "DDP_USER_FITTED | DDP_USER_WAVE" in msgs[0]


# -------------------------------------------------------------------------------------------------------------------- program text
@pytest.mark.parametrize("ex,n,m,nparam,flags,wrap", PROGRAMS, ids=["%s-%dx%d" % p[:3] for p in PROGRAMS])
def test_program_text_is_appended_last_and_only_under_the_flag(ex, n, m, nparam, flags, wrap):
    src = ddp_amd.example_source(ex)
    base, with_flag = _text(src, n, m, nparam, flags, wrap), _text(src, n, m, nparam, flags | FITTED_WAVE, wrap)
    assert base and with_flag and with_flag.startswith(base) and len(with_flag) > len(base)
    tail = with_flag[len(base):]
    assert KERNEL in tail and "UserRollFitArgs" in tail
    assert KERNEL not in base and "UserRollFitArgs" not in base
    # next to DDP_USER_SAMPLE_WAVE: behind that tail, which is what it is without the new flag
    sw, both = _text(src, n, m, nparam, flags | SAMPLE_WAVE, wrap), _text(src, n, m, nparam, flags | SAMPLE_WAVE | FITTED_WAVE, wrap)
    assert both.startswith(sw) and both[len(sw):] == tail and "ddp_user_sample_wave" in sw[len(base):]


def test_no_program_without_the_flag_mentions_the_kernel():
    car = ddp_amd.example_source("car")
    texts = [_text(car, 4, 2, 9, TERMINAL), _text(car, 4, 2, 9, TERMINAL | FITTED),
             _text(ddp_amd.example_source("lq"), 32, 8, LQ_NP(32, 8), 2048 | FITTED | 8192),
             _text(ddp_amd.example_source("chain_ad"), 16, 8, 7, AUTODIFF | WAVE),
             _text(ddp_amd.example_source("chain_ad"), 16, 8, 7, AUTODIFF | WAVE | SAMPLE_WAVE),
             _text(ddp_amd.example_source("car_track"), 4, 2, 7 + 4 * 8, TERMINAL | CLOCK)]
    assert all(texts), _lib.lib().ddp_last_error().decode()
    for t in texts:
        assert KERNEL not in t and "DDP_FWS" not in t


# ------------------------------------------------------------------------------------------------------------------- compile only
COMPILES = {"chain_plant_64x32": ("chain_plant_ad", 64, 32, 9, dict(autodiff=True, plant=True), None, 32),
            "chain_34x17": ("chain_ad", 34, 17, 7, dict(autodiff=True), None, 32),
            "lq_33x2": ("lq", 33, 2, LQ_NP(33, 2), {}, None, 8), "lq_10x9": ("lq", 10, 9, LQ_NP(10, 9), {}, None, 16),
            "pendcart_4x1": ("pendcart_ad", 4, 1, 25, dict(autodiff=True, terminal=True), (0,), 8)}


@pytest.mark.parametrize("name", list(COMPILES))
def test_flag_compiles_without_more_scratch_than_the_wave_rollout_and_within_its_lds(name):
    ex, n, m, nparam, kw, wrap, wg = COMPILES[name]
    diff = ddp_amd.WrappedDiff(*wrap) if wrap else None
    log = ddp_amd.DeviceProblem(ddp_amd.example_source(ex), n, m, nparam=nparam, wave=True, fitted_wave=True, diff=diff,
                                **kw).check("-Rpass-analysis=kernel-resource-usage")
    u, r = _usage(log, KERNEL), _usage(log, "ddp_user_rollout_wave")
    print(name, u)
    assert u and r, log[:2000]
    assert u["ScratchSize [bytes/lane]"] <= r["ScratchSize [bytes/lane]"] and u["VGPRs Spill"] == 0, (u, r)
    # the launch asks for no dynamic LDS: the kernel's own array is all there is, 64 / wg rollouts of x̂, dx, û at an odd stride
    want = (64 // wg) * ((2 * n + m) | 1) * 8
    assert want <= u["LDS Size [bytes/block]"] <= want + 64 and u["LDS Size [bytes/block]"] <= 64 * 1024, (u, want)


# ---------------------------------------------------------------------------------------------------- Python refusals, no device
def _loop_call(problem, c, **kw):
    n, m, T, B = c["n"], c["m"], c["T"], c["B"]
    prev = ddp_amd.GaussianPolicy(T, n, m, np.zeros((m, n, T, B)), c["u"].copy(), c["eye"], c["eye"].copy())
    return kl.iLQGkl(problem, c["x"], prev, kl.Model(c["tfx"], c["tfu"], c["R1"], c["tfc"]), kl_step=kc.LOOP_KL_STEP, max_iter=3,
                     cost=c["cost0"], **kw)


def test_python_refusals_need_no_device():
    c = fw.affine_loop_case(12, 12, 40, False)
    lq = ddp_amd.example_source("lq")
    cm = tuple(np.zeros(s + (c["T"], c["B"])) for s in ((12,), (12,), (12, 12), (12, 12), (12, 12)))
    narrow = ddp_amd.DeviceProblem(lq, 12, 12, nparam=LQ_NP(12, 12), fitted=True)         # (never compiled: m = 12 is refused later)
    wave = ddp_amd.DeviceProblem(lq, 12, 12, nparam=LQ_NP(12, 12), wave=True)
    plain = ddp_amd.DeviceProblem(lq, 12, 12, nparam=LQ_NP(12, 12))
    for p in (narrow, wave):
        with pytest.raises(ddp_amd.DDPError, match=r"fitted=True together with wide=True"):
            _loop_call(p, c, fitted=True, wide=True)
    with pytest.raises(ddp_amd.DDPError, match=r"^iLQGkl: cost_model= together with wide=True"):
        _loop_call(plain, c, cost_model=cm, wide=True)
    with pytest.raises(ddp_amd.DDPError, match=r"^iLQGkl: cost_model= together with wide=True"):
        _loop_call(ddp_amd.LQProblem(c["A"], c["Bm"], c["Q"], c["R"]), c, cost_model=cm, wide=True)
    with pytest.raises(ddp_amd.DDPError, match=r"fitted_wave=True \(DDP_USER_FITTED_WAVE\)"):
        ddp_amd.forward_pass(None, c["x"][:, 0], c["u"], None, 1.0, wave, None, model=(c["tfx"], c["tfu"], c["tfc"]))
    for name in ("DeviceProblem", "forward_pass"):
        assert "fitted_wave" in getattr(ddp_amd, name).__doc__
    assert "fitted_wave" in kl.iLQGkl.__doc__


# ----------------------------------------------------------------------------------------------- what the GPU tests take for granted
def test_the_rollout_table_covers_the_sizes():
    cs = [fw.rollout_case(s, ci) for s, ci in fw.ROLLOUTS]
    assert {(c["n"], c["m"], c["wg"]) for c in cs} == {(33, 2, 8), (10, 9, 16), (40, 12, 16), (34, 17, 32), (64, 32, 32)}
    for s in fw.SHAPES:
        mine = [c for c in cs if c["shape"] == s]
        assert {(c["B"], len(c["al"])) for c in mine} == {(1, 1), (3, 11), (70, 1)} and {c["N"] for c in mine} == {1, 2, 37}
        assert {c["closed"] for c in mine} == {True, False} and {c["per_traj"] for c in mine} == {True, False}
        assert any(c["B"] * len(c["al"]) > 2 * (64 // c["wg"]) and (c["B"] * len(c["al"])) % (64 // c["wg"]) for c in mine)   # a ragged last work-group


def test_the_rollout_limits_act_on_some_controls_not_on_all():
    c = fw.rollout_case("lq_ad_40x12", 0)
    ur = fw.rollout_reference(c)[1]
    hit = (ur == c["lims"][:, 0, None, None, None]) | (ur == c["lims"][:, 1, None, None, None])
    assert 0.02 < hit.mean() < 0.9, hit.mean()


@pytest.mark.parametrize("n,m,T,lims,chain", [c + (False,) for c in fw.CPU_LOOPS] + [fw.CHAIN_LOOP + (False, True), fw.CHAIN_LOOP + (True, True)])
def test_the_loop_references_converge_and_are_stable(n, m, T, lims, chain):
    """conditions, not measurements: the reference ends with status 1 before max_iter on every trajectory, its outcome does not move
    under perturbations of TIE_EPS, and with limits trajectories 1 and 2 end with 5 % to 50 % of their controls on a bound.  chain: the
    tables of (64, 32, 24) under the cost of chain_ad, the reference of the GPU loop test at the corner"""
    ref = fw.loop_reference(n, m, T, lims, chain)
    for b, r in enumerate(ref):
        info = r[6]
        print((n, m, T, lims), b, kc.outcome(info))
        assert info["status"] == 1 and info["iter"] < kc.LOOP_MAX_ITER, (b, kc.outcome(info))
        assert all(np.all(np.isfinite(a)) for a in (r[0], r[1], r[4], r[5]))
        near = fw.loop_outcomes_nearby(n, m, T, lims, b, 1000 * n + 10 * m + b, chain)
        assert all(o == kc.outcome(info) for o in near), (b, kc.outcome(info), near)
    if lims:
        shares = [fw.loop_bound_share(n, m, T, b, chain) for b in range(len(ref))]
        print((n, m, T), "bound shares", shares)
        assert all(0.05 <= s <= 0.5 for s in shares[1:]), shares


def test_the_model_case_has_another_matrix():
    """item 6 of the GPU tests: the parameters of the problem carry a matrix A that is not the one of the tables"""
    c = fw.affine_loop_case(33, 9, 30, False)
    A2 = fw.other_dynamics(c)
    assert np.max(np.abs(A2 - c["A"])) > 1e-3 and np.max(np.abs(np.linalg.eigvals(A2))) < 1 + 1e-9
