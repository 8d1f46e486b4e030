"""DDP_USER_SECOND_ORDER (flag 16, DeviceProblem(second_order=True)) without a GPU: the NumPy reference of the second-order backward
pass reduces to the first-order restatement, its analytic tensors are right, ddp_ad_vhess (csrc/user_autodiff.h) compiled as host C++
gives them, the flagged programs compile for gfx950, and the contract is enforced."""
import os
import re

import numpy as np
import pytest

import ddp_amd
from ddp_amd import _lib

import ddp2_reference as d2
from test_user_autodiff_cpu import _run_host

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "differentialdynamicprogramming.jl_amd")
TERMINAL, CONST_HESSIAN, AUTODIFF, PLANT, SECOND = 1, 2, 4, 8, 16


def _vhess_text():
    src = open(os.path.join(PKG, "csrc", "user_autodiff.h")).read()
    return re.search(r'static const char \*kUserAutodiffVhess = R"DDPA\((.*?)\)DDPA";', src, re.S).group(1)


def _lq_np(n, m):
    return 2 * n * n + n * m + m * m


# ------------------------------------------------------------------------------------------------ the reference itself
@pytest.mark.parametrize("lims", [None, d2.BICYCLE_LIMS])
def test_reference_with_zero_tensors_is_the_first_order_restatement_bit_for_bit(lims):
    from oracle import np_restatement as npr
    P, x0, u0 = d2.sketch_inputs()
    for b in range(4):
        f, costfun, df, tens = d2.bicycle(P[:, b])
        x, u, _ = npr.forward_pass(None, x0[:, b], u0[..., b], None, 1.0, f, costfun, lims)
        d = df(x, u)
        for lam in (1.0, 100.0):
            ref = npr.back_pass(*d[2:], d[0], d[1], lam, 1, lims, x, u)
            z = d2.back_pass2(*d[2:], d[0], d[1], 0 * tens(x, u), lam, 1, lims, x, u)
            assert ref[0] == z[0]
            for a, c in ((ref[1][0], z[1][0]), (ref[1][1], z[1][1]), (ref[1][2], z[1][2]), (ref[2], z[2]), (ref[3], z[3]), (ref[4], z[4])):
                assert np.array_equal(a, c)
            s = d2.back_pass2(*d[2:], d[0], d[1], tens(x, u), lam, 1, lims, x, u)
            if lam == 100.0:                                     # the curvature terms matter: a pass without them is percents away
                assert s[0] == 0 and ref[0] == 0
                assert np.abs(s[3] - ref[3]).max() > 1e-2 * np.abs(ref[3]).max()


def test_analytic_tensors_agree_with_finite_differences():
    """bicycle: central differences (e = 1e-6) of the analytic Jacobian — truncation e² f'''' ~ 1e-12, rounding eps |J| / e ~ 1e-10 with
    |J| <= 1: bound 1e-8.  chain: second differences of f itself (e = 1e-4): rounding 4 eps |f| / (4 e²) ~ 1e-8 |f|, truncation
    e² f'''' ~ 1e-8: bound 1e-5 (|f| up to ~10)."""
    from oracle import np_restatement as npr
    P, x0, u0 = d2.sketch_inputs()
    f, costfun, df, tens = d2.bicycle(P[:, 0])
    x, u, _ = npr.forward_pass(None, x0[:, 0], u0[..., 0], None, 1.0, f, costfun, None)
    e = 1e-6
    for i in (7, 30):
        zz = np.concatenate([x[:, i], u[:, i]])

        def jac(zv):
            dd = df(zv[:4, None].repeat(2, 1), zv[4:, None].repeat(2, 1))
            return np.concatenate([dd[0][:, :, 0], dd[1][:, :, 0]], axis=1)
        Tf = np.zeros((4, 6, 6))
        for a in range(6):
            dz = np.zeros(6); dz[a] = e
            Tf[:, :, a] = (jac(zz + dz) - jac(zz - dz)) / (2 * e)
        T = tens(x, u)[..., i]
        assert np.abs(Tf - T).max() < 1e-8
        assert np.abs(T[:, 3, 5]).max() > 0 and np.abs(T[:, 5, 5]).max() > 0      # fxu and fuu are not zero
    fc, tc = d2.chain()
    rng = np.random.default_rng(0)
    xc, uc = rng.standard_normal(24), rng.standard_normal(4)
    T = tc(xc[:, None], uc[:, None])[..., 0]
    assert np.abs(d2.fd_tensor(fc, xc, uc) - T).max() < 1e-5
    assert np.array_equal(T, T.transpose(0, 2, 1))


# ------------------------------------------------------------------------------------------------ ddp_ad_vhess as host C++
def _host_vhess(tmp_path, src, n, m, cases):
    """H[n+m, n+m] for every case (x, u, p, v): all (a, b), a and b in both orders"""
    nz = n + m
    main = ["int main() {"]
    for x, u, p, v in cases:
        arr = lambda a: ",".join(repr(float(t)) for t in a)
        main.append("{ double x[%d] = {%s}, u[%d] = {%s}, p[%d] = {%s}, v[%d] = {%s};" % (n, arr(x), m, arr(u), len(p), arr(p), n, arr(v)))
        main.append("  for (int b = 0; b < %d; ++b) for (int a = 0; a < %d; ++a) printf(\"%%.17g\\n\", ddp_ad_vhess(x, u, 3, p, v, a, b)); }" % (nz, nz))
    main.append("return 0; }")
    macros = {"DDP_N": n, "DDP_M": m, "DDP_TERMINAL": 0, "DDP_CONST_HESSIAN": 0, "DDP_ADJ": 2, "DDP_ADH": 2}
    out = _run_host(tmp_path, macros, src + "\n" + _vhess_text() + "\n", "\n".join(main))
    return out.reshape(len(cases), nz, nz).transpose(0, 2, 1)     # [case, a, b]


def _check_vhess(H, T, v):
    ref = np.tensordot(v, T, axes=(0, 0))
    assert np.array_equal(H, H.T)                                # H(a, b) == H(b, a) exactly
    assert np.abs(H - ref).max() <= 1e-12 * max(np.abs(ref).max(), 1.0), np.abs(H - ref).max()


def test_host_vhess_of_bicycle_and_car_matches_the_analytic_tensors(tmp_path):
    rng = np.random.default_rng(4)
    Pb, _, _ = d2.sketch_inputs()
    cases = [(rng.standard_normal(4) + [2, 2, 0, 1], 0.4 * rng.standard_normal(2), Pb[:, t], rng.standard_normal(4)) for t in range(4)]
    (tmp_path / "b").mkdir(); (tmp_path / "c").mkdir()
    H = _host_vhess(tmp_path / "b", ddp_amd.example_source("bicycle_ad"), 4, 2, cases)
    for c, (x, u, p, v) in enumerate(cases):
        _check_vhess(H[c], d2.bicycle(p)[3](x[:, None], u[:, None])[..., 0], v)
        assert np.abs(H[c][3, 5]) > 0 and np.abs(H[c][5, 5]) > 0
    pc = [0.05, 4.1, 3.9, 2.1, 1.8, 0.7, 12.0, 0.1, 9.0]
    cases = [(x, u, pc, v) for x, u, _, v in cases]
    H = _host_vhess(tmp_path / "c", ddp_amd.example_source("car_ad"), 4, 2, cases)
    for c, (x, u, p, v) in enumerate(cases):
        _check_vhess(H[c], d2.car_tens(p, x[:, None], u[:, None])[..., 0], v)


def test_host_vhess_of_the_chain_matches_the_analytic_tensor(tmp_path):
    rng = np.random.default_rng(5)
    cases = [(rng.standard_normal(24), rng.standard_normal(4), d2.CHAIN_P, rng.standard_normal(24)) for _ in range(2)]
    H = _host_vhess(tmp_path, d2.CHAIN_SOURCE, 24, 4, cases)
    tens = d2.chain()[1]
    for c, (x, u, p, v) in enumerate(cases):
        _check_vhess(H[c], tens(x[:, None], u[:, None])[..., 0], v)


# ------------------------------------------------------------------------------------------------ compile and contract
def _check(src, n, m, nparam, flags, extra=None):
    L = _lib.lib()
    rc = L.ddp_user_check(src.encode(), n, m, nparam, flags, extra.encode() if extra else None)
    return rc, L.ddp_last_error().decode(), L.ddp_user_compile_log().decode()


def _usage(log, kernel):
    out, cur = {}, None
    for line in log.splitlines():
        mm = re.search(r"remark: Function Name: (\w+)", line)
        if mm:
            cur = mm.group(1)
        mm = re.search(r"remark:\s+([A-Za-z ]+?)(?: \[[^\]]*\])?: (\S+) \[-Rpass-analysis", line)
        if mm and cur == kernel:
            out[mm.group(1).strip()] = mm.group(2)
    return out


SHAPES = [("bicycle_ad", 4, 2, 10, TERMINAL), ("car_ad", 4, 2, 9, TERMINAL), ("pendcart_ad", 4, 1, 25, TERMINAL), ("lq_ad", 10, 2, 224, 0),
          ("chain", 24, 4, d2.CHAIN_NP, 0)]


@pytest.mark.parametrize("name,n,m,nparam,flags", SHAPES)
def test_second_order_programs_compile_for_gfx950(name, n, m, nparam, flags):
    """both new kernels are in the program; their registers, LDS and scratch are printed (pytest -s) as DESIGN.md §3.5 records them.
    The shapes up to 10 x 2 keep ddp_user_back_pass2 out of scratch; 24 x 4 spills (the dual numbers of ddp_ad_vhess: 52 numbers of
    four components), which is recorded, not asserted."""
    src = d2.CHAIN_SOURCE if name == "chain" else ddp_amd.example_source(name)
    rc, err, log = _check(src, n, m, nparam, flags | AUTODIFF | SECOND, "-Rpass-analysis=kernel-resource-usage")
    assert rc == 0, (err, log[:4000])
    for kernel in ("ddp_user_back_pass2", "ddp_user_vhess"):
        u = _usage(log, kernel)
        assert u, kernel
        print(name, kernel, {k: u.get(k) for k in ("VGPRs", "AGPRs", "ScratchSize", "LDS Size", "Occupancy")})
        assert int(u["LDS Size"]) <= 64 * 1024
    if n <= 10:
        assert int(_usage(log, "ddp_user_back_pass2")["ScratchSize"]) == 0


def test_flag_without_autodiff_is_refused():
    rc, err, _ = _check(ddp_amd.example_source("car"), 4, 2, 9, TERMINAL | SECOND)
    assert rc == -1 and "DDP_USER_SECOND_ORDER needs DDP_USER_AUTODIFF" in err, err
    with pytest.raises(ddp_amd.DDPError, match="needs DDP_USER_AUTODIFF"):
        ddp_amd.DeviceProblem(ddp_amd.example_source("car"), 4, 2, nparam=9, terminal=True, second_order=True).check()


def test_kl_entry_refuses_the_flag():
    from ddp_amd import kl
    p = ddp_amd.DeviceProblem(ddp_amd.example_source("bicycle_ad"), 4, 2, nparam=10, terminal=True, autodiff=True, second_order=True)
    assert p.flags == TERMINAL | AUTODIFF | SECOND
    N = 5
    prev = ddp_amd.GaussianPolicy(N, 4, 2, np.zeros((2, 4, N)), np.zeros((2, N)), np.zeros((2, 2, N)), np.zeros((2, 2, N)))
    with pytest.raises(ddp_amd.DDPError, match="second_order=True is refused"):
        kl.iLQGkl(p, np.zeros((4, N)), prev, None, cost=np.zeros(N + 1))
    src = open(os.path.join(ROOT, "differentialdynamicprogramming.jl_amd", "csrc", "kl.hip")).read()
    assert re.search(r"DDP_CHECK\(!f->second_order, \"ilqgkl: a DDP_USER_SECOND_ORDER problem is refused", src)


def test_a_problem_without_the_flag_compiles_the_text_it_compiled_before():
    """the flag only APPENDS to the program (the size macros, the user's source and the first-order kernels come first, unchanged):
    without it none of the new text is there"""
    L = _lib.lib()
    for name, n, m, nparam, flags in SHAPES[:4]:
        src = ddp_amd.example_source(name).encode()
        plain = L.ddp_user_program_text(src, n, m, nparam, flags | AUTODIFF, 0).decode()
        full = L.ddp_user_program_text(src, n, m, nparam, flags | AUTODIFF | SECOND, 0).decode()
        assert full.startswith(plain) and len(full) > len(plain)
        for word in ("DDP_SECOND_ORDER", "ddp_user_back_pass2", "ddp_user_vhess", "UserBp2Args", "chol_masked", "boxqp_dev_ri", "ddp_ad_vhess"):
            assert word not in plain and word in full[len(plain):], word
    hand = L.ddp_user_program_text(ddp_amd.example_source("car").encode(), 4, 2, 9, TERMINAL, 0).decode()
    assert "DDP_SECOND_ORDER" not in hand and "ddp_ad_vhess" not in hand


def test_the_box_qp_of_the_program_is_the_librarys():
    """one definition for both compilers: the program's box-QP and Cholesky are csrc/boxqp_dev.h line for line"""
    L = _lib.lib()
    full = L.ddp_user_program_text(ddp_amd.example_source("bicycle_ad").encode(), 4, 2, 10, TERMINAL | AUTODIFF | SECOND, 0).decode()
    hdr = open(os.path.join(ROOT, "differentialdynamicprogramming.jl_amd", "csrc", "boxqp_dev.h")).read()
    body = "".join(l for l in hdr.splitlines(True) if not l.startswith("#include") and not l.startswith("#pragma once"))
    assert body in full


def test_header_documents_the_flag_and_the_entry_points():
    txt = open(os.path.join(ROOT, "include", "ddp_amd.h")).read()
    assert re.search(r"DDP_USER_SECOND_ORDER\s*=\s*16", txt)
    for word in ("ddp_user_vhess_f64_dev", "ddp_user_back_pass_f64_dev", "ddp_user_back_pass2", "needs DDP_USER_AUTODIFF"):
        assert word in txt, word
