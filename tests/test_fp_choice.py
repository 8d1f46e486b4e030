"""Which rollout kernel a forward-pass call gets (csrc/forward_pass.hip, fp_choose), asked of the library's unlisted debug hook
ddp_fp_choice — the function the dispatcher calls, no GPU needed.  Every row of the table the device test runs
(tests/forward_contract_cases.py; tests/test_gpu_forward_contract.py reads ddp_last_kernel(h, 1) after each), then both sides of every
threshold at its real size, calls without the handle's sink buffer, wrapped differences and each switch in each direction.  The label
the hook writes names what ddp_last_kernel cannot tell apart: the enumerator and its variants (pend_row+fuse+chunked, big64+na4)."""
import ctypes as C
import os

import pytest

from conftest import ROOT
from forward_contract_cases import BIG, DPP, GRP, MID, PIPE, PIPE4, ROW, TABLE, _id

LIB = os.path.join(ROOT, "differentialdynamicprogramming.jl_amd", "libddp_amd.so")
WIDE = "forward_wide_kernel"
POLICY, DYN, ROWAL = 1, 2, 4                 # 16-byte aligned: K, k, u, x | A, Bm | u, k, K
ALL = POLICY | DYN | ROWAL
SWITCHES = ("DDP_FORWARD", "DDP_FORWARD_PIPE", "DDP_FORWARD_FUSE", "DDP_FORWARD_PEND", "DDP_FORWARD_LANE", "DDP_FORWARD64",
            "DDP_FORWARD_MID", "DDP_FORWARD_FAST", "DDP_PEND_CHUNK")


@pytest.fixture(scope="module")
def choice():
    if not os.path.exists(LIB):
        pytest.skip("libddp_amd.so not built")
    try:
        L = C.CDLL(LIB)
    except OSError as e:                      # no HIP runtime on this host
        pytest.skip(str(e))
    f = L.ddp_fp_choice
    f.restype = C.c_char_p
    f.argtypes = [C.c_void_p, C.c_int, C.c_uint, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_char_p), C.c_char_p, C.c_int]
    return f


def ask(choice, kind, n, m, B=7, na=3, dyn="", pol=True, lims=False, diag=False, al=ALL, sink=1, wrap=0, **env):
    """(reported name, label) for one call; kind: "lq" | "pend"; env: switches by their name without DDP_"""
    from ddp_amd import _lib
    P = _lib.Problem()
    P.kind, P.n, P.m, P.N, P.B = int(kind == "pend"), n, m, 16, B
    P.dyn_tv, P.dyn_batched, P.cost_diag, P.diff_wrap = int("F" in dyn), int("f" in dyn), int(diag), wrap
    assert not set("DDP_" + k for k in env) - set(SWITCHES), env
    sw = (C.c_char_p * len(SWITCHES))(*[env[s[4:]].encode() if s[4:] in env else None for s in SWITCHES])
    label = C.create_string_buffer(64)
    name = choice(C.byref(P), na, al, sink, int(pol), int(lims), sw, label, len(label)).decode()
    assert choice(C.byref(P), na, al, sink, int(pol), int(lims), sw, None, 0).decode() == name      # (the label is optional)
    return name, label.value.decode()


def al_of(mis):
    """the alignment bits of a table row: `mis` names the operands 8 bytes into their allocation"""
    return ((0 if set(mis) & set("Kkux") else POLICY) | (0 if set(mis) & set("AB") else DYN) | (0 if set(mis) & set("ukK") else ROWAL))


@pytest.mark.parametrize("r", TABLE, ids=_id)
def test_table_row(choice, r):
    name, label = ask(choice, r["fam"], r["n"], r["m"], r["B"], r["na"], r["dyn"], r["pol"], r["lims"], not r["full"], al_of(r["mis"]),
                      **{k[4:]: v for k, v in r["env"].items()})
    assert name == r["want"], (name, label, r)


def test_pipeline_up_to_1024_rollouts(choice):
    lq = dict(diag=True)
    assert ask(choice, "lq", 10, 2, 1024, 1, **lq) == (PIPE4, "pipe4+fuse")
    assert ask(choice, "lq", 10, 2, 1025, 1, **lq) == (DPP, "dpp+fuse+fast")
    assert ask(choice, "lq", 10, 2, 256, 4, **lq) == (PIPE4, "pipe4+fuse")              # B x nalpha
    assert ask(choice, "lq", 10, 2, 205, 5, **lq) == (DPP, "dpp+fuse+fast")             # 1 025
    assert ask(choice, "lq", 10, 2, 256, 4, dyn="F", **lq) == (PIPE, "pipe_tv+fuse")
    assert ask(choice, "lq", 10, 2, 256, 4, dyn="f", **lq) == (PIPE, "pipe+fuse")
    assert ask(choice, "lq", 10, 2, 257, 4, dyn="F", **lq) == (DPP, "dpp+fuse")         # (FAST needs time-invariant dynamics)


def test_pendcart_chunks_from_3584_and_lanes_from_12288_rollouts(choice):
    assert ask(choice, "pend", 4, 1, 3583, 1, diag=True) == (DPP, "pend_row+fuse")
    assert ask(choice, "pend", 4, 1, 3584, 1, diag=True) == (DPP, "pend_row+fuse+chunked")
    assert ask(choice, "pend", 4, 1, 512, 7, diag=True) == (DPP, "pend_row+fuse+chunked")       # 3 584 = B x nalpha
    assert ask(choice, "pend", 4, 1, 12287, 1) == (DPP, "pend_row+chunked")
    assert ask(choice, "pend", 4, 1, 12288, 1) == (DPP, "pend_lane")
    assert ask(choice, "pend", 4, 1, 768, 16, diag=True) == (DPP, "pend_lane+fuse")             # 12 288 = B x nalpha


@pytest.mark.parametrize("n, m, want", [(12, 2, ROW), (12, 3, ROW), (13, 2, ROW), (13, 3, MID), (14, 2, ROW), (14, 3, MID), (14, 4, MID),
                                        (15, 1, MID), (10, 4, ROW), (11, 4, ROW), (4, 5, MID), (12, 4, ROW), (13, 1, ROW), (14, 1, ROW)])
def test_what_a_padded_row_holds(choice, n, m, want):
    assert ask(choice, "lq", n, m) == (want, "row" if want == ROW else "mid")


def test_large_states(choice):
    assert ask(choice, "lq", 32, 8) == (MID, "mid")
    assert ask(choice, "lq", 33, 8) == (BIG, "big+cost_mid")
    assert ask(choice, "lq", 64, 7) == (BIG, "big+cost_mid")
    assert ask(choice, "lq", 63, 8) == (BIG, "big+cost_mid")
    for na, per_wave in ((1, 1), (2, 2), (3, 4), (5, 4)):
        assert ask(choice, "lq", 64, 8, 5, na) == (BIG, "big64+na%d" % per_wave)
        assert ask(choice, "lq", 64, 8, 5, na, pol=False) == (BIG, "big64+na1")            # without a policy: one rollout per wave
        assert ask(choice, "lq", 64, 7, 5, na) == (BIG, "big+cost_mid")
        assert ask(choice, "lq", 63, 8, 5, na) == (BIG, "big+cost_mid")


def test_wide_controls_and_shapes_without_a_kernel(choice):
    assert ask(choice, "lq", 10, 8) == (MID, "mid")
    assert ask(choice, "lq", 10, 9) == (WIDE, "wide")
    assert ask(choice, "lq", 64, 32) == (WIDE, "wide")
    assert ask(choice, "lq", 10, 9, FORWARD="group") == (WIDE, "wide")
    assert ask(choice, "lq", 10, 33) == ("", "none")
    assert ask(choice, "lq", 65, 2) == ("", "none")
    assert ask(choice, "lq", 65, 9) == ("", "none")
    assert ask(choice, "pend", 40, 1) == ("", "none")                                      # above n = 32: the LQ family only
    assert ask(choice, "pend", 4, 9) == ("", "none")


def test_without_the_sink_buffer(choice):
    """a handle whose sink buffer could not be allocated: no pipeline, no pendulum row kernel, no FAST variant"""
    assert ask(choice, "lq", 10, 2, diag=True) == (PIPE4, "pipe4+fuse")
    assert ask(choice, "lq", 10, 2, diag=True, sink=0) == (DPP, "dpp+fuse")
    assert ask(choice, "pend", 4, 1, diag=True) == (DPP, "pend_row+fuse")
    assert ask(choice, "pend", 4, 1, diag=True, sink=0) == (DPP, "dpp+fuse")
    assert ask(choice, "pend", 4, 1, 12288, 1, sink=0) == (DPP, "pend_lane")                # (the lane kernel masks its stores)
    assert ask(choice, "pend", 4, 1, wrap=1, sink=0) == (GRP, "group")
    assert ask(choice, "pend", 4, 1, 12288, 1, wrap=1, sink=0) == (GRP, "group")
    assert ask(choice, "lq", 6, 3, sink=0) == (ROW, "row")


def test_wrapped_differences(choice):
    assert ask(choice, "lq", 10, 2, diag=True, wrap=2) == (GRP, "group")
    assert ask(choice, "lq", 6, 3, wrap=1) == (GRP, "group")
    assert ask(choice, "lq", 20, 3, wrap=1) == (GRP, "group")
    assert ask(choice, "pend", 4, 1, diag=True, wrap=1) == (DPP, "pend_row+fuse+wrap")
    assert ask(choice, "pend", 4, 1, wrap=5, lims=True) == (DPP, "pend_row+wrap")
    assert ask(choice, "pend", 4, 1, wrap=1, pol=False) == (DPP, "pend_row")                # (only a policy has a difference to wrap)
    assert ask(choice, "pend", 4, 1, 12288, 1, wrap=1) == (DPP, "pend_lane+wrap")
    assert ask(choice, "pend", 4, 1, wrap=1, FORWARD_LANE="1") == (DPP, "pend_lane+wrap")
    assert ask(choice, "pend", 4, 1, wrap=1, FORWARD_PEND="0") == (GRP, "group")
    assert ask(choice, "pend", 4, 1, 12288, 1, wrap=1, FORWARD_PEND="0") == (GRP, "group")
    assert ask(choice, "pend", 4, 1, wrap=1, FORWARD="group") == (GRP, "group")
    # DDP_FORWARD=b is ignored with wrapped differences
    assert ask(choice, "lq", 20, 3, wrap=1, FORWARD="b") == (GRP, "group")
    assert ask(choice, "pend", 4, 1, wrap=1, FORWARD="b") == (DPP, "pend_row+wrap")


def test_every_switch_in_each_direction(choice):
    lq, pd = dict(diag=True), dict(diag=True)
    # DDP_FORWARD: group, b (LQ only: any other kind keeps the normal order), anything else is no switch
    assert ask(choice, "lq", 10, 2, FORWARD="group", **lq) == (GRP, "group")
    assert ask(choice, "lq", 40, 2, FORWARD="group") == (BIG, "big+cost_mid")
    assert ask(choice, "lq", 10, 2, FORWARD="b", **lq) == (MID, "mid")
    assert ask(choice, "lq", 10, 2, FORWARD="b", FORWARD_MID="0", **lq) == (BIG, "big")
    assert ask(choice, "pend", 4, 1, FORWARD="b", **pd) == (DPP, "pend_row+fuse")
    assert ask(choice, "lq", 10, 2, FORWARD="x", **lq) == (PIPE4, "pipe4+fuse")
    # DDP_FORWARD_PIPE: 0 never; 1 | 2 lift the 1 024 cap but not the alignment tests; 2 the two-row kernel
    assert ask(choice, "lq", 10, 2, FORWARD_PIPE="0", **lq) == (DPP, "dpp+fuse+fast")
    assert ask(choice, "lq", 10, 2, 2048, 1, FORWARD_PIPE="1", **lq) == (PIPE4, "pipe4+fuse")
    assert ask(choice, "lq", 10, 2, 2048, 1, FORWARD_PIPE="2", **lq) == (PIPE, "pipe+fuse")
    assert ask(choice, "lq", 10, 2, 2048, 1, dyn="F", FORWARD_PIPE="2", **lq) == (PIPE, "pipe_tv+fuse")
    assert ask(choice, "lq", 10, 2, 2048, 1, FORWARD_PIPE="1", al=DYN | ROWAL, **lq) == (DPP, "dpp+fuse+fast")
    assert ask(choice, "lq", 10, 2, dyn="F", FORWARD_PIPE="1", al=POLICY | ROWAL, **lq) == (DPP, "dpp+fuse")
    assert ask(choice, "lq", 10, 2, FORWARD_PIPE="1", al=POLICY | ROWAL, **lq) == (PIPE4, "pipe4+fuse")    # misaligned A, Bm matter with dyn_tv only
    assert ask(choice, "lq", 10, 2, FORWARD_PIPE="1", lims=True, **lq) == (DPP, "dpp+fuse+fast")
    # DDP_FORWARD_FUSE=0: the separate cost kernels, and no pipeline
    assert ask(choice, "lq", 10, 2, FORWARD_FUSE="0", **lq) == (DPP, "dpp+fast")
    assert ask(choice, "lq", 10, 2, FORWARD_FUSE="0", FORWARD_PIPE="1", **lq) == (DPP, "dpp+fast")
    assert ask(choice, "lq", 10, 2, FORWARD_FUSE="1", **lq) == (PIPE4, "pipe4+fuse")
    assert ask(choice, "pend", 4, 1, FORWARD_FUSE="0", **pd) == (DPP, "pend_row")
    assert ask(choice, "pend", 4, 1, 12288, 1, FORWARD_FUSE="0", **pd) == (DPP, "pend_lane")
    assert ask(choice, "lq", 10, 2, FORWARD_FUSE="1") == (DPP, "dpp+fast")                   # (the switch does not make a full cost diagonal)
    # DDP_FORWARD_PEND=0: the generic row kernel for the pendulum
    assert ask(choice, "pend", 4, 1, FORWARD_PEND="0", **pd) == (DPP, "dpp+fuse+fast")
    assert ask(choice, "pend", 4, 1, FORWARD_PEND="1", **pd) == (DPP, "pend_row+fuse")
    assert ask(choice, "pend", 4, 1, 12288, 1, FORWARD_PEND="0", **pd) == (DPP, "pend_lane+fuse")
    # DDP_FORWARD_LANE
    assert ask(choice, "pend", 4, 1, FORWARD_LANE="1", **pd) == (DPP, "pend_lane+fuse")
    assert ask(choice, "pend", 4, 1, 12288, 1, FORWARD_LANE="0", **pd) == (DPP, "pend_row+fuse+chunked")
    assert ask(choice, "lq", 10, 2, FORWARD_LANE="1", **lq) == (PIPE4, "pipe4+fuse")
    # DDP_FORWARD64, DDP_FORWARD_MID
    assert ask(choice, "lq", 64, 8, FORWARD64="0") == (BIG, "big+cost_mid")
    assert ask(choice, "lq", 64, 8, FORWARD64="1") == (BIG, "big64+na4")
    assert ask(choice, "lq", 64, 8, FORWARD64="0", FORWARD_MID="0") == (BIG, "big")
    assert ask(choice, "lq", 64, 8, FORWARD_MID="0") == (BIG, "big64+na4")
    assert ask(choice, "lq", 20, 3, FORWARD_MID="0") == (BIG, "big")
    assert ask(choice, "lq", 20, 3, FORWARD_MID="1") == (MID, "mid")
    assert ask(choice, "lq", 40, 3, FORWARD_MID="0") == (BIG, "big")
    # DDP_FORWARD_FAST=0; the FAST variant of (10, 2) loads u, k, K in 16-byte pieces, the pendulum's has no such loads
    assert ask(choice, "lq", 10, 2, lims=True, **lq) == (DPP, "dpp+fuse+fast")
    assert ask(choice, "lq", 10, 2, lims=True, FORWARD_FAST="0", **lq) == (DPP, "dpp+fuse")
    assert ask(choice, "lq", 10, 2, lims=True, FORWARD_FAST="1", al=POLICY | DYN, **lq) == (DPP, "dpp+fuse")
    assert ask(choice, "lq", 10, 2, lims=True, pol=False, **lq) == (DPP, "dpp+fuse")
    assert ask(choice, "pend", 4, 1, FORWARD_PEND="0", al=DYN, **pd) == (DPP, "dpp+fuse+fast")
    # DDP_PEND_CHUNK
    assert ask(choice, "pend", 4, 1, PEND_CHUNK="1", **pd) == (DPP, "pend_row+fuse+chunked")
    assert ask(choice, "pend", 4, 1, 3584, 1, PEND_CHUNK="0", **pd) == (DPP, "pend_row+fuse")
