"""The cases of tests/test_gpu_user_lane.py without a GPU (tests/user_lane_cases.py): the layout layout_of gives every case shape, so
that a change of it says which regime lost its shape; that the cases put work-groups over α boundaries, over two trajectories, over an
inactive next to an active trajectory and leave the last one partial at every layout in use; that the references are well conditioned
(float64 against long double) and hold what the GPU assertions rely on (a clamped and a free control, a wrap beyond π, finite values);
and that lq at (16, 3), the one shape no other test compiles, compiles for gfx950."""
import numpy as np
import pytest

import ddp_amd
import user_lane_cases as lc
from conftest import relerr


def test_layouts_of_the_case_shapes():
    """(DDP_CHUNK, DDP_RLANES, DDP_DFLANES) of every shape are the ones the cases were chosen for"""
    got = {k: lc.layout(k) for k in lc.SHAPES}
    print(got)
    assert got == lc.EXPECT, {k: (got[k], lc.EXPECT[k]) for k in got if got[k] != lc.EXPECT[k]}


def test_layouts_cover_the_regimes():
    """independent of EXPECT: whatever layout_of picks, the shapes together still reach every regime"""
    L = {k: lc.layout(k) for k in lc.SHAPES}
    chunks = {v[0] for v in L.values()}
    assert 1 in chunks and any(c > 1 for c in chunks), chunks
    assert {v[1] for v in L.values()} >= {64, 32, 16}, L
    assert {v[2] for v in L.values()} >= {64, 16, 4, 2}, L
    # one step per chunk both by division (ps <= 63) and forced (ps > 63) with all 64 rollouts
    assert any(L[k][:2] == (1, 64) and lc.ps_of(k) <= 63 for k in L) and any(L[k][:2] == (1, 64) and lc.ps_of(k) > 63 for k in L), L
    # (24, 4), ps = 128, is the first size past the budget of 64 rollouts: 64 (ps | 1) 8 > 64 KB from ps = 128 on
    narrow = [k for k in L if L[k][1] < 64]
    assert min(narrow, key=lc.ps_of) == "lq24" and lc.ps_of("lq24") == 128 and 64 * (127 | 1) * 8 <= 65536 < 64 * (128 | 1) * 8
    assert all(L[k][1] == 64 for k in L if lc.ps_of(k) < 128), L


@pytest.mark.parametrize("key", lc.ROLL_SHAPES)
def test_rollout_cases_mix_work_groups(key):
    chunk, rlanes, _ = lc.layout(key)
    Ns = lc.roll_N(key)
    assert 1 in Ns and 2 * chunk + 1 in Ns, (Ns, chunk)            # one chunk and less; a last chunk of one step behind two full ones
    assert chunk == 1 or (chunk in Ns and any(N < chunk for N in Ns) and any(N % chunk for N in Ns if N > chunk)), (Ns, chunk)
    groups = {(B, na): lc.roll_groups(B, na, rlanes, lc.holes(B)) for B, na in lc.BNA}
    assert any(g[0] > 1 for g in groups[(3, 11)]), "no work-group of (3, 11) holds two α's"
    assert any(g[0] > 1 for g in groups[(23, 3)]) and not groups[(23, 3)][-1][2], "(23, 3): no α boundary inside a work-group, or a full last one"
    assert any(g[1] for gs in groups.values() for g in gs), "no work-group holds an inactive and an active trajectory"
    assert any(g[1] and g[0] > 1 for gs in groups.values() for g in gs)
    assert any(B * na < rlanes for B, na in lc.BNA)               # fewer rollouts than slots
    cs = lc.roll_cases(key)
    for B, na in lc.BNA:                                             # every (B, nα) meets every option
        mine = [c for c in cs if c[1:3] == (B, na)]
        assert {c[3] for c in mine} == {True, False}, (B, na)
        if B > 1:
            assert {c[4] for c in mine} == {True, False} and {c[5] for c in mine} == {True, False}, (B, na)
    assert {c[3:] for c in cs} >= {(p, l, b) for p in (True, False) for l in (True, False) for b in (True, False)}


@pytest.mark.parametrize("key", lc.DF_SHAPES)
def test_derivative_cases_mix_work_groups(key):
    dfl = lc.layout(key)[2]
    groups = {(N, B): lc.df_groups(N, B, dfl, lc.holes(B)) for N, B in lc.df_NB(key)}
    assert any(g[0] > 1 for g in groups[(37, 3)]), "no work-group over two trajectories"
    assert any(g[1] for g in groups[(37, 3)]), "no work-group holds an inactive and an active trajectory"
    assert any(not gs[-1][2] for gs in groups.values())
    assert any(N * B % dfl == 1 % dfl and N * B > dfl for N, B in groups), "no case one past a multiple of the lanes"
    assert any(N * B < dfl for N, B in groups) or dfl <= 2


def test_cost_cases_sit_on_the_lane_count():
    """with the terminal slot CL = N + 1 lands on 64, one past it and beyond two rounds of the 64 lanes; without it N does"""
    assert {N + 1 for N in lc.COST_N} >= {64, 65} and {N for N in lc.COST_N} >= {64, 65} and max(lc.COST_N) > 128 and 1 in lc.COST_N
    term = [bool(lc.SHAPES[k][4].get("terminal")) for k in lc.COST_SHAPES]
    assert sorted(term) == [False, True]
    a = lc.holes(lc.COST_B)
    assert a.any() and not a.all()


@pytest.mark.parametrize("key", lc.ROLL_SHAPES)
def test_rollout_references_are_well_conditioned_and_hold_their_content(key):
    """float64 against long double <= 1e-12 per time step (two decades under the 1e-10 of the GPU test); finite; every case with limits
    has a control on a bound and one inside; the wrapped case differs from its nominal by more than π somewhere"""
    worst, wrapped = 0.0, 0
    for spec in lc.roll_cases(key):
        c = lc.roll_case(key, *spec)
        ref = c["ref"]
        dbl = lc.roll_reference(c, np.float64)
        assert all(np.isfinite(a.astype(np.float64)).all() for a in ref), spec
        for b in range(c["B"]):
            for ai in range(c["na"]):
                e = max(relerr(dbl[0][:, :, b, ai], ref[0][:, :, b, ai]), relerr(dbl[1][:, :, b, ai], ref[1][:, :, b, ai]),
                        relerr(dbl[2][:, b, ai], ref[2][:, b, ai], 0))
                worst = max(worst, e)
                assert e <= 1e-12, (spec, b, ai, e)
        if c["lim"]:
            on, free = lc.clamp_census(c, ref[1].astype(np.float64))
            assert on > 0 and free > 0, (spec, on, free)
        if c["wrap"] and c["pol"]:
            d = np.abs(ref[0][0].astype(np.float64)[..., 0] - c["x"][0])
            assert d.max() > np.pi, spec
            wrapped += 1
    assert wrapped > 0 or not lc.SHAPES[key][5]
    print("%s: float64 against long double, worst %.2e over %d cases" % (key, worst, len(lc.roll_cases(key))))


@pytest.mark.parametrize("key", lc.COST_SHAPES)
def test_cost_references_are_well_conditioned(key):
    for N in lc.COST_N:
        c = lc.cost_case(key, N)
        assert c["ref"].shape == (N + bool(lc.SHAPES[key][4].get("terminal")), lc.COST_B)
        assert np.isfinite(c["ref"].astype(np.float64)).all()
        assert relerr(lc.cost_reference(c, np.float64), c["ref"], 0) <= 1e-12, N


@pytest.mark.parametrize("key", lc.DF_SHAPES)
def test_derivative_references_are_finite(key):
    for N, B in lc.df_NB(key):
        c = lc.df_case(key, N, B)
        n, m = c["n"], c["m"]
        assert [r.shape for r in c["ref"]] == [s + (N, B) for s in ((n, n), (n, m), (n,), (m,), (n, n), (n, m), (m, m))]
        assert all(np.isfinite(r).all() for r in c["ref"])
        if lc.SHAPES[key][0].startswith("lq"):                       # the closed form in float64 against long double
            p = c["prm"][:, B - 1] if c["batched"] else c["prm"]
            for a, r in zip(lc.lq_df(p, c["n"], c["m"], c["x"][..., B - 1], c["u"][..., B - 1], np.float64), c["ref"]):
                assert relerr(a, r[..., B - 1]) <= 1e-12


def test_lq_16_3_compiles_for_gfx950():
    ex, n, m, nparam, kw, _ = lc.SHAPES["lq16"]
    L = ddp_amd._lib.lib()
    rc = L.ddp_user_check(ddp_amd.example_source(ex).encode(), n, m, nparam, 0, None)
    assert rc == 0, (L.ddp_last_error().decode(), L.ddp_user_compile_log().decode())
