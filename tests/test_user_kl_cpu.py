"""User problems through the KL-constrained loop (ddp_user_ilqgkl_*) without a GPU: the entry points are declared, exported, listed and
bound from Julia; the build's resource records hold the GPS instantiations of back_pass_mid_kernel with no more scratch than their iLQG
twins; ddp_gps_choice names the back_pass_gps kernel each kind of call gets; kl.iLQGkl checks a DeviceProblem's extents before any launch;
the driver's workspace layout holds together (tests/kl_workspace_check.cpp, a host program of its own)."""
import ctypes as C
import glob
import json
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import ddp_amd
from ddp_amd import _lib, kl

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["ddp_user_ilqgkl_f64_dev", "ddp_user_ilqgkl_f64"]
Q4, LANE, MID, GEN = "back_pass_gps_q4", "back_pass_gps_lane", "back_pass_gps_mid", "back_pass_gps"
STANDALONE, REGISTERED, USER = 0, 1, 2


def test_new_symbols_are_declared_exported_and_bound_from_julia():
    L = C.CDLL(_lib.LIB_PATH)
    txt = open(os.path.join(ROOT, "include", "ddp_amd.h")).read()
    jl = open(os.path.join(ROOT, "differentialdynamicprogramming.jl_amd", "julia", "DDPAmd.jl")).read()
    called = set(re.findall(r"@ccall\s+libddp\.(\w+)\(", jl))
    for s in NEW:
        assert re.search(r"\b%s\s*\(" % s, txt), s
        assert hasattr(L, s), s
        assert s in _lib.EXPORTS, s
        assert s in called, s
    assert re.search(r"function iLQGkl\(problem::DeviceProblem", jl)
    assert hasattr(L, "ddp_gps_choice") and "ddp_gps_choice" not in txt          # an unlisted debug hook, like ddp_bp_choice


def _usage():
    recs = {}
    for f in glob.glob(os.path.join(ROOT, "differentialdynamicprogramming.jl_amd", "build", "back_pass_mid.o.usage.json")):
        recs.update(json.load(open(f)))
    return recs


def test_gps_mid_instantiations_spill_no_more_than_their_ilqg_twins():
    """back_pass_mid_kernel<NTR, PT, MMX, LIMS, CTV, GPSK>: every GPS instantiation (CTV = true) next to the iLQG one with the same
    template arguments.  Mangled names end in GPSK: ...ELi0EEEv iLQG, ...ELi1EEEv prepass-fed (NTR = 2), ...ELi2EEEv fused (NTR = 1)."""
    recs = _usage()
    assert recs, "no build/back_pass_mid.o.usage.json: build first"
    mid = {k: v for k, v in recs.items() if "back_pass_mid_kernel" in k}
    tail = "EEEvNS_9BPMidArgsE"
    gps = {k: v for k, v in mid.items() if k.endswith("ELi1" + tail) or k.endswith("ELi2" + tail)}
    assert len(gps) == 12, sorted(mid)                                  # (NTR, PT, MMX) x 6, with and without limits
    for k, v in gps.items():
        assert "ELb1ELi" in k, k                                        # CTV: operands requested per step
        fused = k.endswith("ELi2" + tail)
        assert fused == ("kernelILi1E" in k), k                         # fused for NTR = 1, prepass-fed for NTR = 2
        twin = k[: -len("ELi1" + tail)] + "ELi0" + tail
        assert twin in mid, (k, sorted(mid))
        assert int(v["ScratchSize"]) <= int(mid[twin]["ScratchSize"]), (k, v, mid[twin])


def _choice(n, m, N=100, caller=USER, eta_tv=0, mid=None, q4=None, lane=None):
    f = C.CDLL(_lib.LIB_PATH).ddp_gps_choice
    f.restype = C.c_char_p
    f.argtypes = [C.POINTER(_lib.BPDesc), C.c_int, C.c_int, C.c_char_p, C.c_char_p, C.c_char_p]
    d = _lib.BPDesc(n, m, N, 16, 1, 1, 1, 1, 1, 0)
    enc = lambda s: None if s is None else s.encode()                                   # noqa: E731
    return f(C.byref(d), eta_tv, caller, enc(mid), enc(q4), enc(lane)).decode()


@pytest.mark.parametrize("n,m,want", [(4, 1, Q4), (4, 2, LANE), (10, 2, MID), (4, 3, MID), (17, 5, MID), (32, 8, MID), (1, 1, MID)])
def test_user_driver_choice(n, m, want):
    assert _choice(n, m) == want


def test_other_calls_keep_q4_lane_generic_by_default():
    for caller in (STANDALONE, REGISTERED):
        assert _choice(10, 2, caller=caller) == GEN
        assert _choice(4, 1, caller=caller) == Q4
        assert _choice(4, 2, caller=caller) == LANE
        assert _choice(4, 1, caller=caller, eta_tv=1) == LANE                           # q4 takes one η per trajectory only
    assert _choice(4, 1, caller=STANDALONE, lane="0") == GEN                            # DDP_GPS_LANE=0: the run-time-sized kernel
    assert _choice(4, 1, caller=REGISTERED, q4="0") == LANE


@pytest.mark.parametrize("caller", [STANDALONE, REGISTERED, USER])
def test_gps_mid_switch(caller):
    shapes = [(n, m) for n in (1, 3, 4, 6, 10, 13, 16, 17, 24, 32) for m in (1, 2, 3, 4, 5, 8)]
    for n, m in shapes:
        assert _choice(n, m, caller=caller, mid="1") == MID, (n, m)
        assert _choice(n, m, caller=caller, mid="1", eta_tv=1) == MID, (n, m)
        assert _choice(n, m, caller=caller, mid="0") != MID, (n, m)
    assert _choice(10, 2, caller=USER, mid="0") == GEN


class _NoDevice:
    """a handle that fails the test as soon as anything would use it: the call did not stop before the device"""
    def __getattr__(self, name):
        raise AssertionError("reached the device (handle.%s)" % name)


def test_ilqgkl_rejects_wrong_extents_before_any_launch():
    p = ddp_amd.DeviceProblem(ddp_amd.example_source("car"), 4, 2, nparam=9, terminal=True)
    n, m, N, B = 4, 2, 20, 6
    x0 = np.zeros((n, N, B))
    prev = ddp_amd.GaussianPolicy(N, n, m, np.zeros((m, n, N, B)), np.zeros((m, N, B)), np.zeros((m, m, N, B)), np.zeros((m, m, N, B)))
    R1 = np.eye(n)
    ok = dict(cost=np.zeros((N + 1, B)), params=np.zeros(9), handle=_NoDevice())

    def call(**kw):
        a = dict(ok); a.update(kw)
        return kl.iLQGkl(a.pop("problem", p), a.pop("x0", x0), a.pop("prev", prev), a.pop("model", kl.Model(None, None, R1)), **a)
    with pytest.raises(ddp_amd.DDPError, match="params"):
        call(params=np.zeros((9, B + 1)))
    with pytest.raises(ddp_amd.DDPError, match="params"):
        call(params=np.zeros(8))
    with pytest.raises(ddp_amd.DDPError, match="no params"):
        call(params=None)
    with pytest.raises(ddp_amd.DDPError, match="n = 4, m = 2"):
        call(x0=np.zeros((3, N, B)))
    with pytest.raises(ddp_amd.DDPError, match="model.fx"):
        call(model=kl.Model(np.zeros((n, n, N - 1)), None, R1))
    with pytest.raises(ddp_amd.DDPError, match="R1"):
        call(model=kl.Model(None, None, np.eye(3)))
    with pytest.raises(ddp_amd.DDPError, match="cost"):
        call(cost=np.zeros((N, B)))                                     # CL = N + 1 with the terminal cost
    with pytest.raises(ddp_amd.DDPError, match="traj_prev"):
        call(prev=ddp_amd.GaussianPolicy(N, n, m, np.zeros((m, n, N - 1, B)), np.zeros((m, N, B)), np.zeros((m, m, N, B)),
                                         np.zeros((m, m, N, B))))
    with pytest.raises(ddp_amd.DDPError, match="lims"):
        call(lims=np.zeros((3, 2)))


# ------------------------------------------------------------------------------------------------------------- the workspace layout
def _cxx():
    for c in ("c++", "g++", "clang++", "/opt/rocm/llvm/bin/clang++"):
        p = shutil.which(c) or (c if os.path.isabs(c) and os.path.exists(c) else None)
        if p:
            return p
    raise RuntimeError("no host C++ compiler")


def test_driver_workspace_layout(tmp_path):
    """csrc/kl_workspace.h, compiled for the host with the address and undefined-behaviour sanitizers and run as a program of its own:
    pieces disjoint, 256-byte aligned, the counter block first, no gap, and the size the hand-written sum gave — (4, 1), (10, 2), (32, 8),
    (40, 20), (64, 32), with and without a family, constant Hessians, their repetition and the driver's own dynamics"""
    exe = tmp_path / "kl_workspace_check"
    cxx = _cxx()
    # g++ links the sanitizers' runtimes as shared libraries unless told otherwise, and a shared runtime insists on being the first library
    # of the process; linked statically (clang's default) the program runs in whatever environment the suite has
    static = [] if "clang" in subprocess.run([cxx, "--version"], capture_output=True, text=True).stdout else ["-static-libasan", "-static-libubsan"]
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] + static + [
        "-I", os.path.join(ROOT, "differentialdynamicprogramming.jl_amd", "csrc"), "-o", str(exe),
        os.path.join(ROOT, "tests", "kl_workspace_check.cpp")]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[:4000]
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    lines = r.stdout.splitlines()
    assert lines[-1] == "ok: 70 cases", lines[-3:]
    for n, m in ((4, 1), (10, 2), (32, 8), (40, 20), (64, 32)):
        for tag in ("family=0", "family=1", "const_hessian=1 hrep=0", "const_hessian=1 hrep=1", "fx_own=0", "fx_own=1"):
            assert any(l.startswith("n=%d m=%d " % (n, m)) and tag in l for l in lines), (n, m, tag)
