"""The slot scheduler and the closed loop for user problems (ddp_user_ilqg_queue_*, ddp_user_ilqg_mpc_*, DDP_USER_PLANT) without a GPU:
the plant example compiles for gfx950, the flag without a `plant` is refused before compiling, the plant kernel and the masked Hessian
kernel do not spill, the new entry points are declared, exported and bound from Julia, and iLQG_queue / iLQG_mpc check the extents
of a DeviceProblem's arrays before anything reaches the device."""
import os
import re

import numpy as np
import pytest

import ddp_amd
from ddp_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CAR = ddp_amd.example_source("car")
CAR_PLANT = ddp_amd.example_source("car_plant")
TERMINAL, CONST_HESSIAN, AUTODIFF, PLANT = 1, 2, 4, 8
NEW = ["ddp_user_ilqg_queue_f64_dev", "ddp_user_ilqg_queue_f64", "ddp_user_ilqg_mpc_f64_dev", "ddp_user_ilqg_mpc_f64"]

# the templated car of car_ad.hip with a plain-double plant that calls the model: the plant of an autodiff problem
CAR_AD_PLANT = ddp_amd.example_source("car_ad") + """
__device__ void plant(const double *x, const double *u, int t, const double *p, double *xnext)
{
    const double ua[2] = {1.1 * u[0], u[1]};
    dynamics<double>(x, ua, t, p, xnext);
}
"""

# the pendulum with constant cost Hessians (the per-step cxx of pendcart.hip without the terminal weight)
PEND_CONST_HESSIAN = """
__device__ void cost_hessians(const double *p, double *cxx, double *cxu, double *cuu)
{
    for (int e = 0; e < 16; ++e) cxx[e] = p[8 + e];
    for (int e = 0; e < 4; ++e) cxu[e] = 0.0;
    cuu[0] = p[24];
}
"""


def _check(src, n, m, nparam=0, flags=0, extra=None):
    L = _lib.lib()
    rc = L.ddp_user_check(src.encode(), n, m, nparam, flags, extra.encode() if extra else None)
    return rc, L.ddp_last_error().decode(), L.ddp_user_compile_log().decode()


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


@pytest.mark.parametrize("src,flags", [(CAR_PLANT, TERMINAL | PLANT), (CAR_PLANT, TERMINAL), (CAR_AD_PLANT, TERMINAL | AUTODIFF | PLANT)])
def test_plant_example_compiles_for_gfx950(src, flags):
    rc, err, log = _check(src, 4, 2, 13, flags)
    assert rc == 0, (err, log)


def test_plant_flag_without_a_plant_is_refused_before_compiling():
    rc, err, _ = _check(CAR, 4, 2, 9, TERMINAL | PLANT)
    assert rc == -1, err                                     # -1: refused by the argument checks (a failed compile is -4)
    assert "plant" in err, err
    # the word in a comment is no definition
    rc, err, _ = _check(CAR + "\n// no plant here\n", 4, 2, 9, TERMINAL | PLANT)
    assert rc == -1 and "plant" in err, err


@pytest.mark.parametrize("src,n,m,nparam,flags,kernels", [
    (CAR_PLANT, 4, 2, 13, TERMINAL | PLANT, ("ddp_user_plant", "ddp_user_rollout", "ddp_user_df")),
    (CAR_AD_PLANT, 4, 2, 13, TERMINAL | AUTODIFF | PLANT, ("ddp_user_plant",)),
    (ddp_amd.example_source("pendcart") + PEND_CONST_HESSIAN, 4, 1, 25, TERMINAL | CONST_HESSIAN, ("ddp_user_hessians",)),
    (ddp_amd.example_source("lq"), 4, 1, 2 * 16 + 4 + 1, CONST_HESSIAN, ("ddp_user_hessians",)),
])
def test_plant_and_masked_hessian_kernels_do_not_spill(src, n, m, nparam, flags, kernels):
    rc, err, log = _check(src, n, m, nparam, flags, "-Rpass-analysis=kernel-resource-usage")
    assert rc == 0, err
    u = _usage(log)
    for k in kernels:
        assert k in u, (k, sorted(u))
        assert u[k] == 0, (k, u)
    if not flags & PLANT:
        assert "ddp_user_plant" not in u, sorted(u)


def test_new_symbols_are_declared_exported_and_bound_from_julia():
    import ctypes
    L = ctypes.CDLL(_lib.LIB_PATH)
    txt = open(os.path.join(ROOT, "include", "ddp_amd.h")).read()
    jl = open(os.path.join(ROOT, "differentialdynamicprogramming.jl_amd", "julia", "DDPAmd.jl")).read()
    called = set(re.findall(r"@ccall\s+libddp\.(\w+)\(", jl))
    for s in NEW:
        assert re.search(r"\b%s\s*\(" % s, txt), s
        assert hasattr(L, s), s
        assert s in _lib.EXPORTS, s
        assert s in called, s
    assert re.search(r"DDP_USER_PLANT\s*=\s*8", txt)
    assert re.search(r"function iLQG_queue\(problem::DeviceProblem", jl) and re.search(r"function iLQG_mpc\(problem::DeviceProblem", jl)
    assert "plant::Bool=false" in jl


def test_device_problem_plant_flag():
    assert ddp_amd.DeviceProblem(CAR_PLANT, 4, 2, nparam=13, terminal=True, plant=True).flags == TERMINAL | PLANT
    assert ddp_amd.DeviceProblem(CAR_PLANT, 4, 2, nparam=13, terminal=True).flags == TERMINAL
    p = ddp_amd.DeviceProblem(CAR_PLANT, 4, 2, nparam=13, terminal=True, plant=True)
    assert "ddp_user_plant" in "".join(_usage(p.check("-Rpass-analysis=kernel-resource-usage")))


class _NoDevice:
    """a handle that fails the test as soon as anything would use it: the call did not stop before the device"""
    def __getattr__(self, name):
        raise AssertionError("reached the device (handle.%s)" % name)


@pytest.mark.parametrize("entry", ["queue", "mpc"])
def test_queue_and_mpc_reject_wrong_extents_before_any_launch(entry):
    p = ddp_amd.DeviceProblem(CAR_PLANT, 4, 2, nparam=13, terminal=True, plant=True)
    B, N = 6, 20
    x0, u0 = np.zeros((4, B)), np.zeros((2, N, B))
    call = ((lambda *a, **k: ddp_amd.iLQG_queue(*a, slots=4, **k)) if entry == "queue"
            else (lambda *a, **k: ddp_amd.iLQG_mpc(a[0], a[1], a[2], 3, **k)))
    h = _NoDevice()
    with pytest.raises(ddp_amd.DDPError, match="params"):
        call(p, x0, u0, params=np.zeros((13, B + 1)), handle=h)
    with pytest.raises(ddp_amd.DDPError, match="params"):
        call(p, x0, u0, params=np.zeros((12,)), handle=h)
    with pytest.raises(ddp_amd.DDPError, match="no params"):
        call(p, x0, u0, handle=h)
    with pytest.raises(ddp_amd.DDPError, match="n = 4, m = 2"):
        call(p, np.zeros((3, B)), u0, params=np.zeros(13), handle=h)
    with pytest.raises(ddp_amd.DDPError, match="n = 4, m = 2"):
        call(p, x0, np.zeros((1, N, B)), params=np.zeros(13), handle=h)
    with pytest.raises(ddp_amd.DDPError, match="different B"):
        call(p, np.zeros((4, B - 1)), u0, params=np.zeros(13), handle=h)
    with pytest.raises(ddp_amd.DDPError, match="lims"):
        call(p, x0, u0, params=np.zeros(13), lims=np.zeros((3, 2)), handle=h)
