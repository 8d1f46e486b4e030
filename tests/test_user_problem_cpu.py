"""User problems (ddp_user_*, DeviceProblem) without a GPU: the bundled examples compile for gfx950 through hiprtc, the contract
violations are refused before compiling with a message that names the cause, the generated kernels of the n = 4 / n = 10 examples do
not spill, and every new entry point is exported and bound from Julia."""
import os
import re

import pytest

import ddp_amd
from ddp_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LQ = ddp_amd.example_source("lq")
PEND = ddp_amd.example_source("pendcart")
CAR = ddp_amd.example_source("car")
NEW = ["ddp_user_check", "ddp_user_compile_log", "ddp_user_create", "ddp_user_destroy", "ddp_user_df_f64_dev", "ddp_user_df_f64",
       "ddp_user_forward_pass_f64_dev", "ddp_user_forward_pass_f64", "ddp_user_costfun_f64_dev", "ddp_user_costfun_f64",
       "ddp_user_ilqg_f64_dev", "ddp_user_ilqg_f64"]


def _check(src, n, m, nparam=0, flags=0, extra=None):
    L = _lib.lib()
    rc = L.ddp_user_check(src.encode(), n, m, nparam, flags, extra.encode() if extra else None)
    return rc, L.ddp_last_error().decode(), L.ddp_user_compile_log().decode()


@pytest.mark.parametrize("name,n,m,nparam,flags", [("lq", 10, 2, 224, 0), ("lq", 10, 2, 224, 2), ("pendcart", 4, 1, 25, 1),
                                                   ("car", 4, 2, 9, 1), ("lq", 24, 4, 2 * 576 + 96 + 16, 0)])
def test_examples_compile_for_gfx950(name, n, m, nparam, flags):
    rc, err, log = _check(ddp_amd.example_source(name), n, m, nparam, flags)
    assert rc == 0, (err, log)


def test_syntax_error_reports_the_compiler_line():
    bad = PEND.replace("xnext[2] = x[2] + h * x[3];", "xnext[2] = x[2] + h * x[3]")
    rc, err, log = _check(bad, 4, 1, 25, 1)
    assert rc < 0
    assert re.search(r"user_source:\d+:\d+: error", log), log
    assert "compilation failed" in err


@pytest.mark.parametrize("src,n,m,nparam,flags,cause", [
    (CAR.replace("derivatives", "derivs"), 4, 2, 9, 1, "derivatives"),
    (LQ, 10, 2, 224, 1, "terminal_cost"),
    (LQ.replace("cost_hessians", "hessians_of_cost"), 10, 2, 224, 2, "cost_hessians"),
    (LQ, 33, 2, 0, 0, "n = 33"),
    (LQ, 10, 9, 0, 0, "m = 9"),
    (LQ, 10, 2, 4097, 0, "nparam = 4097"),
])
def test_contract_violations_are_refused_before_compiling(src, n, m, nparam, flags, cause):
    rc, err, _ = _check(src, n, m, nparam, flags)
    assert rc == -1, err                                     # -1: refused by the argument checks (a failed compile is -4)
    assert cause in err, err


def test_device_problem_check_raises_with_the_log():
    with pytest.raises(ddp_amd.DDPError, match="user_source"):
        ddp_amd.DeviceProblem("__device__ void dynamics(", 4, 1).check()


def _usage(log):
    """kernel -> ScratchSize from the kernel-resource-usage remarks of a hiprtc log"""
    out, cur = {}, None
    for line in log.splitlines():
        mm = re.search(r"remark: Function Name: (\w+)", line)
        if mm:
            cur = mm.group(1)
        mm = re.search(r"remark:\s+ScratchSize \[bytes/lane\]: (\d+)", line)
        if mm and cur:
            out[cur] = int(mm.group(1))
    return out


@pytest.mark.parametrize("name,n,m,nparam,flags", [("pendcart", 4, 1, 25, 1), ("car", 4, 2, 9, 1), ("lq", 10, 2, 224, 0),
                                                   ("lq", 10, 2, 224, 2)])
def test_rollout_and_derivative_kernels_do_not_spill(name, n, m, nparam, flags):
    rc, err, log = _check(ddp_amd.example_source(name), n, m, nparam, flags, "-Rpass-analysis=kernel-resource-usage")
    assert rc == 0, err
    u = _usage(log)
    for k in ("ddp_user_rollout", "ddp_user_df"):
        assert k in u, (k, sorted(u))
        assert u[k] == 0, (k, u)


def test_new_symbols_are_exported_and_listed():
    import ctypes
    L = ctypes.CDLL(_lib.LIB_PATH)
    txt = open(os.path.join(ROOT, "include", "ddp_amd.h")).read()
    for s in NEW:
        assert re.search(r"\b%s\s*\(" % s, txt), s
        assert hasattr(L, s), s
        assert s in _lib.EXPORTS, s


def test_julia_binding_calls_the_new_entry_points():
    src = open(os.path.join(ROOT, "differentialdynamicprogramming.jl_amd", "julia", "DDPAmd.jl")).read()
    called = set(re.findall(r"@ccall\s+libddp\.(\w+)\(", src))
    missing = [s for s in NEW if s not in called and s != "ddp_user_compile_log"]
    assert not missing, missing
    assert "struct DeviceProblem" in src or "mutable struct DeviceProblem" in src


def test_params_shape_is_checked_before_any_launch():
    p = ddp_amd.DeviceProblem(CAR, 4, 2, nparam=9, terminal=True)
    with pytest.raises(ddp_amd.DDPError, match="params"):
        p._params(8, __import__("numpy").zeros((9, 7)))
    with pytest.raises(ddp_amd.DDPError, match="no params"):
        p._params(8)
