"""Wide controls (8 < m <= 32) without a GPU: which kernel the dispatcher names for them (csrc/back_pass.hip, bp_choose, through the
unlisted debug hook ddp_bp_choice), that no m <= 8 call changes its kernel, the constants of the public header and of the Julia host,
and that the C oracle and the NumPy restatement agree on the cases the GPU tests use (tests/wide_controls_cases.py) — which shows that
those inputs do not sit at a tie of the reference's box-QP."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT, relerr
from test_bp_choice import ALL, TABLE, _desc, row
from test_bp_choice import choice  # noqa: F401  (the fixture: ddp_bp_choice of the built library)
from wide_controls_cases import LAYOUTS, SOLVES, bp_case, bp_operands, clamped_share, outcome, reference_outcomes_nearby, solve_batch, solve_case

WIDE = "back_pass_wide_kernel"


def _ask(choice, n, m, B, ops="", lims=None, backpass=None, al=ALL, sink=1):
    from ddp_amd import _lib
    d = _desc(row(n, m, B, None, ops, lims), _lib.BPDesc)
    return choice(C.byref(d), al, sink, int(lims == "on"), backpass.encode() if backpass else None, None, None, None).decode()


@pytest.mark.parametrize("m", [9, 16, 32])
@pytest.mark.parametrize("n", [1, 10, 32, 33, 64])
def test_wide_shapes_get_the_wide_kernel(choice, n, m):
    """(a) every operand layout, with and without limits, aligned or not, with or without a sink, batch sizes on both sides of every
    threshold of the other families"""
    for ops in ("", "F", "FC", "FCfc", "f", "Cc"):
        for lims in (None, "on", "off"):
            for B in (1, 8, 1024, 1025, 5120, 6144):
                assert _ask(choice, n, m, B, ops, lims) == WIDE, (n, m, B, ops, lims)
    assert _ask(choice, n, m, 64, al=0, sink=0) == WIDE
    for letter in ("x", "g", "big", "mid", "row", "new", "old", "s", "wtile"):       # no other family holds m > 8
        assert _ask(choice, n, m, 64, backpass=letter) == WIDE, letter


def test_no_kernel_beyond_the_bounds(choice):
    """(b)"""
    for n, m in ((10, 33), (64, 33), (65, 9), (65, 32), (65, 1)):
        assert _ask(choice, n, m, 8) == "", (n, m)
        assert _ask(choice, n, m, 8, backpass="controls") == "", (n, m)


@pytest.mark.parametrize("n,m", [(10, 2), (32, 8), (64, 8), (12, 3), (4, 1)])
def test_forced_onto_the_wide_kernel(choice, n, m):
    """(c) DDP_BACKPASS=c... at m <= 8"""
    for bp in ("c", "controls"):
        for lims in (None, "on"):
            for B in (8, 1024, 6144):
                assert _ask(choice, n, m, B, "FCfc", lims, backpass=bp) == WIDE
                assert _ask(choice, n, m, B, "", lims, backpass=bp) == WIDE


@pytest.mark.parametrize("r", [r for r in TABLE if r["env"].get("DDP_BACKPASS") is None][::3] + [r for r in TABLE if r["env"].get("DDP_BACKPASS")],
                         ids=lambda r: "n%d_m%d_B%d_%s" % (r["n"], r["m"], r["B"], r["want"]))
def test_narrow_shapes_keep_their_kernel(choice, r):
    """(d) a sample of the parent's table (every third unforced row, every forced one): the answer it pins"""
    from ddp_amd import _lib
    assert r["m"] <= 8
    sw = [r["env"].get(k) for k in ("DDP_BACKPASS", "DDP_SH_MIN_B", "DDP_MX2", "DDP_DPPW")]
    got = choice(C.byref(_desc(r, _lib.BPDesc)), r["al"], 1, int(r["lims"] == "on"), *[s.encode() if s else None for s in sw]).decode()
    assert got == r["want"] and got != WIDE


def test_constants_of_the_header_and_the_julia_host():
    """(e)"""
    hdr = open(os.path.join(ROOT, "include", "ddp_amd.h")).read()
    assert re.search(r"^#define DDP_MAX_M 8\b", hdr, flags=re.M) and re.search(r"^#define DDP_MAX_M_WIDE 32\b", hdr, flags=re.M)
    jl = open(os.path.join(ROOT, "differentialdynamicprogramming.jl_amd", "julia", "DDPAmd.jl")).read()
    assert re.search(r"^const MAX_M = 8\b", jl, flags=re.M) and re.search(r"^const MAX_M_WIDE = 32\b", jl, flags=re.M)
    assert re.search(r"1 <= m <= MAX_M_WIDE", jl)


BP_CPU = [(6, 9), (12, 12), (10, 24), (24, 16), (32, 32), (48, 12), (64, 32)]


@pytest.mark.parametrize("n,m", BP_CPU)
def test_oracle_and_numpy_agree_on_the_backward_cases(n, m):
    """(f) the C oracle against the NumPy restatement on the generator of the GPU tests, every trajectory at 1e-11: no limits and limits
    ±0.5 / ±0.25, LTI and time-varying operands, regType 1 and 2; no trajectory diverges; with limits at least a fifth of k is clamped (mean over the cases of a shape)"""
    from oracle import np_restatement as npr
    from oracle import oracle_ctypes as oc
    N, B = 40, 2
    worst, shares = 0.0, []
    for li, lim in enumerate((None, 0.5, 0.25)):
        for lay in ("", "FCfc"):
            for regType in (1, 2):
                c = bp_case(7 + 100 * n + m + li, n, m, N, B, lay, lim)
                for b in range(B):
                    cx, cu, cxx, cxu, cuu, fx, fu, lam = bp_operands(c, b)
                    u = c["u"][..., b]
                    d1, (K1, k1, Q1), vx1, vxx1, dv1 = oc.back_pass(cx, cu, cxx, cxu, cuu, fx, fu, lam, regType, c["lims"], None, u)
                    d2, (K2, k2, Q2), vx2, vxx2, dv2 = npr.back_pass(cx, cu, cxx, cxu, cuu, fx, fu, lam, regType, c["lims"], None, u)
                    assert d1 == d2 == 0
                    for a_, b_ in ((K1, K2), (k1, k2), (Q1, Q2), (vx1, vx2), (vxx1, vxx2)):
                        worst = max(worst, relerr(a_, b_))
                    if lim is not None:
                        shares.append(clamped_share(k1[:, :-1], u[:, :-1], c["lims"]))
    print("worst oracle-vs-NumPy distance %.3g; clamped share of k %.0f %% .. %.0f %%, mean %.0f %%" % (worst, 100 * min(shares), 100 * max(shares),
                                                                                                    100 * np.mean(shares)))
    assert worst < 1e-11 and np.mean(shares) >= 0.2


@pytest.mark.parametrize("n,m,T,lim", SOLVES[:2])
def test_oracle_and_numpy_agree_on_whole_solves(n, m, T, lim):
    """(f) the C oracle's ilqg against the NumPy restatement's on the solves the GPU test runs (the two (12, 12) ones here: the larger
    ones take the NumPy loop minutes): same status, iteration and back-pass counts, x, u, Vxx at 1e-11"""
    from oracle import np_restatement as npr
    from oracle import oracle_ctypes as oc
    P = solve_case(n, m, T, lim)
    p = oc.make_problem("lq", n, m, T, A=P["A"], B=P["B"], Q=P["Q"], R=P["R"])
    xr, ur, (Kr, kr, Quur), vxr, vxxr, cr, info = oc.ilqg(p, P["x0"], P["u0"], lims=P["lims"], max_iter=50)
    f, costfun, df = npr.lq_closures(P["A"], P["B"], P["Q"], P["R"])
    x2, u2, pol2, vx2, vxx2, c2, info2 = npr.iLQG(f, costfun, df, P["x0"], P["u0"].copy(), lims=P["lims"], max_iter=50)
    assert (info["status"], info["iter"], info["n_backpass"]) == (info2["status"], info2["iter"], info2["n_backpass"])
    assert info["status"] in (1, 2)
    assert relerr(xr, x2) < 1e-11 and relerr(ur, u2) < 1e-11 and relerr(vxxr, vxx2) < 1e-11


def test_the_reference_contradicts_itself_at_one_perturbed_copy():
    """what tests/test_gpu_wide_controls.py::test_whole_solves allows for, shown on the oracle alone: copy 28 of the (12, 12, 80, ±0.6)
    batch ends by gradient after 9 iterations, and by tolerance after 8 on inputs 1e-13 (relative) away — the table's own solve
    (copy 0) and a neighbour give one answer on every nearby input"""
    from oracle import oracle_ctypes as oc
    n, m, T, lim = SOLVES[1]
    P = solve_case(n, m, T, lim)
    x0, u0 = solve_batch(P)
    p = oc.make_problem("lq", n, m, T, A=P["A"], B=P["B"], Q=P["Q"], R=P["R"])
    sides = {}
    for b in (0, 27, 28):
        own = outcome(oc.ilqg(p, x0[:, b], u0[..., b], lims=P["lims"], max_iter=50)[6])
        sides[b] = {own} | {outcome(r[6]) for r in reference_outcomes_nearby(p, x0[:, b], u0[..., b], P["lims"], 1000 * b + n)}
    print(sides)
    assert len(sides[0]) == 1 and len(sides[27]) == 1
    assert sides[28] == {(1, 9, 9), (2, 8, 8)}
