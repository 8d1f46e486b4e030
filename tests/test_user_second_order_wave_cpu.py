"""DDP_USER_SECOND_ORDER_WAVE (flag 128, DeviceProblem(second_order_wave=True)) without a GPU: the flag rules of ddp_user_check, the
program text of problems without the flag (unchanged), the new program compiled for gfx950 through hiprtc with its resource records,
the analytic tensor of user_examples/chain_ddp_ad.hip (tests/ddp2_wide_cases.py) against second differences, the reference pass with
zero tensors against the first-order restatement at (18, 9), and the constant and keyword in the header, the loader and the Julia
binding."""
import functools
import hashlib
import os
import re

import numpy as np
import pytest

import ddp_amd
from ddp_amd import _lib

import ddp2_wide_cases as w2
from test_user_wave_cpu import PIN_SOURCE, PLAIN_TEXT_PINS, lq_nparam, usage

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "differentialdynamicprogramming.jl_amd")
TERMINAL, CONST_HESSIAN, AUTODIFF, PLANT, SECOND, WAVE, SECOND_WAVE = 1, 2, 4, 8, 16, 32, 128
REMARKS = "-Rpass-analysis=kernel-resource-usage"
LDS_LIMIT = 160 * 1024


def _check(src, n, m, nparam, flags, extra=None):
    L = _lib.lib()
    rc = L.ddp_user_check(src.encode(), n, m, nparam, flags, extra.encode() if extra else None)
    return rc, L.ddp_last_error().decode(), L.ddp_user_compile_log().decode()


# ------------------------------------------------------------------------------------------------------------------ flag rules
@pytest.mark.parametrize("flags,causes", [
    (SECOND_WAVE, ("DDP_USER_SECOND_ORDER_WAVE needs DDP_USER_WAVE",)),
    (SECOND_WAVE | AUTODIFF, ("DDP_USER_SECOND_ORDER_WAVE needs DDP_USER_WAVE",)),
    (SECOND_WAVE | WAVE, ("DDP_USER_SECOND_ORDER_WAVE needs DDP_USER_AUTODIFF",)),
    (SECOND_WAVE | SECOND | AUTODIFF, ("DDP_USER_SECOND_ORDER_WAVE needs DDP_USER_WAVE",)),
    (SECOND_WAVE | SECOND | WAVE | AUTODIFF, ("DDP_USER_SECOND_ORDER_WAVE excludes DDP_USER_SECOND_ORDER",)),
    (SECOND | WAVE | AUTODIFF, ("DDP_USER_SECOND_ORDER | DDP_USER_WAVE is refused (ddp_user_back_pass2 is sized for n <= 32, m <= 8)",)),
    (64, ("unknown flags 0x40",)),
    (64 | SECOND_WAVE | WAVE | AUTODIFF, ("unknown flags",)),
    (256 | WAVE | AUTODIFF, ("unknown flags",)),
])
def test_flag_rules(flags, causes):
    """refused before compiling, with a message that names the missing or the excluded flag; 16 | 32 keeps its message with or
    without the new bit, 64 stays unknown"""
    rc, err, _ = _check(ddp_amd.example_source("lq_ad"), 10, 2, lq_nparam(10, 2), flags)
    assert rc == -1, (rc, err)
    for cause in causes:
        assert cause in err, err


def test_python_keyword_sets_the_flags_and_the_kl_entry_refuses_them():
    from ddp_amd import kl
    p = ddp_amd.DeviceProblem(ddp_amd.example_source("chain_ddp_ad"), 18, 9, nparam=w2.NPARAM, autodiff=True, second_order_wave=True)
    assert p.wave and p.second_order_wave and not p.second_order
    assert p.flags == AUTODIFF | WAVE | SECOND_WAVE
    q = ddp_amd.DeviceProblem(ddp_amd.example_source("chain_ddp_ad"), 18, 9, nparam=w2.NPARAM, autodiff=True, wave=True)
    assert q.flags == AUTODIFF | WAVE and not q.second_order_wave
    with pytest.raises(ddp_amd.DDPError, match="needs DDP_USER_AUTODIFF"):
        ddp_amd.DeviceProblem(ddp_amd.example_source("lq"), 10, 9, nparam=lq_nparam(10, 9), second_order_wave=True).check()
    with pytest.raises(ddp_amd.DDPError, match="DDP_USER_WAVE"):
        ddp_amd.DeviceProblem(ddp_amd.example_source("lq_ad"), 10, 2, nparam=224, autodiff=True, second_order=True, wave=True).check()
    N = 5
    prev = ddp_amd.GaussianPolicy(N, 18, 9, np.zeros((9, 18, N)), np.zeros((9, N)), np.zeros((9, 9, N)), np.zeros((9, 9, N)))
    for wide in (False, True):
        with pytest.raises(ddp_amd.DDPError, match="second_order_wave=True is refused"):
            kl.iLQGkl(p, np.zeros((18, N)), prev, None, cost=np.zeros(N), **({"wide": True} if wide else {}))
    ksrc = open(os.path.join(PKG, "csrc", "kl.hip")).read()
    assert re.search(r"DDP_CHECK\(!f->second_order, \"ilqgkl: a DDP_USER_SECOND_ORDER problem is refused", ksrc)   # the C entry: both flags set it
    usrc = open(os.path.join(PKG, "csrc", "user_problem.hip")).read()
    assert "P->second_order = (flags & (DDP_USER_SECOND_ORDER | DDP_USER_SECOND_ORDER_WAVE)) != 0;" in usrc


def test_header_loader_and_julia_agree():
    hdr = open(os.path.join(ROOT, "include", "ddp_amd.h")).read()
    jl = open(os.path.join(PKG, "julia", "DDPAmd.jl")).read()
    assert re.search(r"\bDDP_USER_SECOND_ORDER_WAVE = 128\b", hdr)
    assert not re.search(r"DDP_USER_\w+\s*=\s*64\b", hdr) and "64: not assigned" in hdr
    assert _lib.USER_SECOND_ORDER_WAVE == 128
    assert re.search(r"^const USER_SECOND_ORDER_WAVE = 128\b", jl, flags=re.M)
    assert re.search(r"second_order_wave::Bool=false", jl) and re.search(r"\(second_order_wave \? USER_SECOND_ORDER_WAVE : 0\)", jl)
    assert re.search(r"wave = wave \|\| second_order_wave", jl)
    for word in ("ddp_user_back_pass2_wave", "chain_ddp_ad", "excludes DDP_USER_SECOND_ORDER"):
        assert word in hdr, word
    import inspect
    assert "second_order_wave" in inspect.signature(ddp_amd.DeviceProblem.__init__).parameters


# ---------------------------------------------------------------------------------------------------------------- program text
NEW_WORDS = ("ddp_user_back_pass2_wave", "back_pass_wide_body", "WLds", "UserBp2WaveArgs", "boxqp_wave", "v_mfma", "mfma_f64_16x16x4f64")
# sha256 of kUserKernels2 (csrc/user_problem_kernels.h) before it was cut into Head + Bp2 + Vhess
KERNELS2_LEN, KERNELS2_SHA = 18264, "b04f7b333578765a3b6244c46f59e99d74b8ff206c488774736fa219da79e5d9"


def _text(src, n, m, nparam, flags, wrap=0):
    t = _lib.lib().ddp_user_program_text(src, n, m, nparam, flags, wrap)
    assert t is not None, _lib.lib().ddp_last_error().decode()
    return t.decode()


@pytest.mark.parametrize("key", sorted(PLAIN_TEXT_PINS))
def test_lane_program_text_is_unchanged(key):
    """a lane problem: the bytes pinned before DDP_USER_WAVE existed (tests/test_user_wave_cpu.py) still hold, and none of the new text"""
    n, m, nparam, flags, wrap = key
    text = _lib.lib().ddp_user_program_text(PIN_SOURCE, n, m, nparam, flags, wrap)
    assert (len(text), hashlib.sha256(text).hexdigest()) == PLAIN_TEXT_PINS[key]
    for word in NEW_WORDS:
        assert word.encode() not in text, word


def test_wave_program_text_is_unchanged_and_the_flag_only_appends():
    """a wave problem: the flagged program STARTS with its text (the method of tests/test_user_second_order_cpu.py), which holds none
    of the new words; everything new comes behind it"""
    src = ddp_amd.example_source("chain_ddp_ad").encode()
    for n, m in ((18, 9), (64, 32)):
        plain = _text(src, n, m, w2.NPARAM, AUTODIFF | WAVE)
        full = _text(src, n, m, w2.NPARAM, AUTODIFF | WAVE | SECOND_WAVE)
        assert full.startswith(plain) and len(full) > len(plain)
        for word in NEW_WORDS + ("DDP_SECOND_ORDER", "ddp_user_vhess", "ddp_ad_vhess"):
            assert word not in plain, word
        for word in ("ddp_user_back_pass2_wave", "back_pass_wide_body", "WLds", "UserBp2WaveArgs", "ddp_user_vhess", "ddp_ad_vhess"):
            assert word in full[len(plain):], word
        assert "void ddp_user_back_pass2(" not in full          # its static_assert on 64 KB fails at these shapes


def test_second_order_program_text_is_unchanged():
    """a DDP_USER_SECOND_ORDER problem: the three pieces of kUserKernels2 join to the bytes of the undivided text (length and digest taken
    before the cut), the program ends with them, and holds none of the new text"""
    hdr = open(os.path.join(PKG, "csrc", "user_problem_kernels.h")).read()
    pieces = [re.search(r'static const char \*kUserKernels2%s = R"DDPK\((.*?)\)DDPK";' % k, hdr, re.S).group(1) for k in ("Head", "Bp2", "Vhess")]
    joined = "".join(pieces)
    assert (len(joined), hashlib.sha256(joined.encode()).hexdigest()) == (KERNELS2_LEN, KERNELS2_SHA)
    src = ddp_amd.example_source("bicycle_ad").encode()
    plain = _text(src, 4, 2, 10, TERMINAL | AUTODIFF)
    full = _text(src, 4, 2, 10, TERMINAL | AUTODIFF | SECOND)
    assert full.startswith(plain) and full.endswith(joined)
    for word in NEW_WORDS:
        assert word not in full, word


def test_the_wide_step_of_the_program_is_the_librarys():
    """one definition for both compilers: the program holds csrc/wide_tile.h and csrc/back_pass_wide_kernel.h line for line (without their
    #include and #pragma once lines), and back_pass_wide.hip includes the header rather than a copy of the step"""
    full = _text(ddp_amd.example_source("chain_ddp_ad").encode(), 18, 9, w2.NPARAM, AUTODIFF | WAVE | SECOND_WAVE)
    for name in ("wide_tile.h", "back_pass_wide_kernel.h"):
        hdr = open(os.path.join(PKG, "csrc", name)).read()
        body = "".join(l for l in hdr.splitlines(True) if not l.startswith("#include") and not l.startswith("#pragma once"))
        assert body in full, name
    hip = open(os.path.join(PKG, "csrc", "back_pass_wide.hip")).read()
    assert '#include "back_pass_wide_kernel.h"' in hip
    for word in ("chol_wave(const", "boxqp_wave(const", "struct WLds"):
        assert word not in hip, word
        assert full.count(word) == 1, word


# -------------------------------------------------------------------------------------------------------------------- compiling
COMPILES = [("bicycle_ad", 4, 2, TERMINAL), ("chain_ddp_ad", 18, 9, 0), ("chain_ddp_ad", 34, 17, 0), ("chain_ddp_ad", 64, 32, 0),
            ("lq_ad", 10, 9, CONST_HESSIAN)]


def nparam_of(name, n, m):
    return {"bicycle_ad": 10, "chain_ddp_ad": w2.NPARAM, "lq_ad": lq_nparam(n, m)}[name]


@functools.lru_cache(maxsize=None)
def compiled(name, n, m, flags):
    return _check(ddp_amd.example_source(name), n, m, nparam_of(name, n, m), flags, REMARKS)


@pytest.mark.parametrize("name,n,m,flags", COMPILES)
def test_second_order_wave_programs_compile_for_gfx950(name, n, m, flags):
    """limits are a run-time argument of the kernel (has_lims, and lims[0] > lims[m] read on the device): one instantiation per shape
    serves both.  The step's LDS is a static array: the compiler's record is the whole of it and stays within gfx950's 160 KB.
    Registers and scratch are printed (pytest -s) as DESIGN.md §3.5 records them; scratch is expected (the dual numbers of
    ddp_ad_vhess: n + m + n numbers of four components per lane) and is not asserted."""
    rc, err, log = compiled(name, n, m, flags | AUTODIFF | WAVE | SECOND_WAVE)
    assert rc == 0, (err, log[-4000:])
    u = usage(log)
    assert "ddp_user_back_pass2_wave" in u and "ddp_user_vhess" in u and "ddp_user_back_pass2" not in u, sorted(u)
    assert "ddp_user_rollout_wave" in u and "ddp_user_df_wave" in u
    for kernel in ("ddp_user_back_pass2_wave", "ddp_user_vhess"):
        print(name, n, m, kernel, u[kernel])
    rec = u["ddp_user_back_pass2_wave"]
    assert 0 < rec["LDS"] <= LDS_LIMIT, rec
    for k, r in u.items():
        if k != "ddp_user_back_pass2_wave":
            assert r.get("LDS", 0) <= 64 * 1024, (k, r)


def test_the_pass_without_curvature_compiles():
    """DDP_BP2_NO_CURVATURE in the source (bench/user_second_order_wave.py): the same program without P0"""
    src = "#define DDP_BP2_NO_CURVATURE 1\n" + ddp_amd.example_source("chain_ddp_ad")
    rc, err, log = _check(src, 18, 9, w2.NPARAM, AUTODIFF | WAVE | SECOND_WAVE, REMARKS)
    assert rc == 0, (err, log[-4000:])
    with_p0 = usage(compiled("chain_ddp_ad", 18, 9, AUTODIFF | WAVE | SECOND_WAVE)[2])["ddp_user_back_pass2_wave"]
    without = usage(log)["ddp_user_back_pass2_wave"]
    print(with_p0, without)
    assert without["LDS"] == with_p0["LDS"]


def test_chain_ddp_example_enforces_its_shape():
    assert "static_assert" in ddp_amd.example_source("chain_ddp_ad")
    rc, err, _ = _check(ddp_amd.example_source("chain_ddp_ad"), 10, 4, w2.NPARAM, AUTODIFF | WAVE | SECOND_WAVE)
    assert rc == -4 and "compilation failed" in err, (rc, err)


# ------------------------------------------------------------------------------------------------------------- the NumPy reference
@pytest.mark.parametrize("J", [3, 9])
def test_chain_ddp_tensor_agrees_with_second_differences(J):
    """second differences of f itself (e = 1e-4), the comparison and the bound of tests/test_user_second_order_cpu.py for its chain:
    rounding 4 eps |f| / (4 e²) ~ 1e-8 |f|, truncation e² f'''' ~ 1e-8: bound 1e-5"""
    f, costfun, df, tens = w2.chain_ddp(w2.CHAIN_P, J)
    rng = np.random.default_rng(J)
    x, u = rng.standard_normal(2 * J), rng.standard_normal(J)
    T = tens(x[:, None], u[:, None])[..., 0]
    assert np.abs(w2.fd_tensor(f, x, u) - T).max() < 1e-5
    assert np.array_equal(T, T.transpose(0, 2, 1))
    n = 2 * J
    assert np.abs(T[:, :n, :n]).max() > 0 and np.abs(T[:, :n, n:]).max() > 0 and np.abs(T[:, n:, n:]).max() > 0     # fxx, fxu, fuu


def test_chain_ddp_closures_match_central_differences():
    """f against df (e = 1e-5: truncation ~1e-10, rounding ~1e-11 for O(1) values; bound 1e-6 as for chain_ad)"""
    J = 5
    n, m = 2 * J, J
    f, costfun, df, tens = w2.chain_ddp(w2.CHAIN_P, J)
    rng = np.random.default_rng(0)
    x = np.concatenate([0.8 * rng.standard_normal(J), 0.5 * rng.standard_normal(J)])
    u = 0.5 * rng.standard_normal(m)
    z = np.concatenate([x, u])
    F = lambda z_: f(z_[:n], z_[n:], 0)
    Cf = lambda z_: float(costfun(z_[:n, None], z_[n:, None])[0])
    fx, fu, cx, cu, cxx, cxu, cuu = [a[..., 0] for a in df(x[:, None], u[:, None])]
    e = 1e-5
    E = e * np.eye(n + m)
    Jn = np.stack([(F(z + E[j]) - F(z - E[j])) / (2 * e) for j in range(n + m)], axis=1)
    gn = np.array([(Cf(z + E[j]) - Cf(z - E[j])) / (2 * e) for j in range(n + m)])
    assert np.max(np.abs(Jn - np.hstack([fx, fu]))) < 1e-6
    assert np.max(np.abs(gn - np.concatenate([cx, cu]))) < 1e-6


def test_reference_with_zero_tensors_is_the_first_order_restatement_at_18_9():
    from oracle import np_restatement as npr
    J, N = 9, 8
    n, m = 2 * J, J
    f, costfun, df, tens = w2.chain_ddp(w2.CHAIN_P, J)
    rng = np.random.default_rng(3)
    x0 = 0.5 * rng.standard_normal(n)
    u0 = 0.3 * rng.standard_normal((m, N))
    lims = np.stack([-0.25 * np.ones(m), 0.25 * np.ones(m)], axis=1)
    for L in (None, lims):
        x, u, _ = npr.forward_pass(None, x0, u0, None, 1.0, f, costfun, L)
        d = df(x, u)
        for lam, reg in ((1.0, 1), (10.0, 2)):
            ref = npr.back_pass(*d[2:], d[0], d[1], lam, reg, L, x, u)
            z = w2.back_pass2(*d[2:], d[0], d[1], 0 * tens(x, u), lam, reg, L, x, u)
            assert ref[0] == z[0] == 0
            for a, c in ((ref[1][0], z[1][0]), (ref[1][1], z[1][1]), (ref[1][2], z[1][2]), (ref[2], z[2]), (ref[3], z[3]), (ref[4], z[4])):
                assert np.array_equal(a, c)
            s = w2.back_pass2(*d[2:], d[0], d[1], tens(x, u), lam, reg, L, x, u)
            assert s[0] == 0 and np.abs(s[3] - ref[3]).max() > 1e-6 * np.abs(ref[3]).max()     # the curvature terms are not zero
