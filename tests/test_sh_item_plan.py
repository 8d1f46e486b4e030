"""The item and unit plan of the shared-LTI backward pass (csrc/back_pass_sh.hip: sh_item_plan, the function sh_group_kernel calls,
compiled for the host behind the unlisted debug hook ddp_sh_item_plan; no GPU needed).  A launch gives the λ groups that miss classic
tiles and splits those that hit into affine tiles (Vx, k, dV: the chain in time) and broadcast units (group, chunk of 8 steps, block of
trajectories: Vxx | K | Quu, stored by writer waves).  Swept over the compute-unit counts, batches, group counts and group shapes of
test_sh_tiles_cpu.py, N in {16, 17, 24, 1000} and the hit masks none / all / one group / alternating:
  with no hit, T and W are what that file's restatement of the parent's rule gives;
  the item count never exceeds ddp_sh_max_tiles(B, ncu), the hit-path work-groups never the compute units;
  every trajectory of every group lies in exactly one tile (classic for a miss, affine for a hit when the launch is split);
  the units cover every (chunk, trajectory) of every hit group exactly once and touch no group that missed;
  every unit belongs to exactly one writer wave (the waves number 0 .. NW - 1 without gaps, unit u goes to wave u % NW)."""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import ROOT
from test_sh_tiles_cpu import GMAX, TMAX, device_tiles

LIB = os.path.join(ROOT, "differentialdynamicprogramming.jl_amd", "libddp_amd.so")
CH, NWAVES, WTB = 8, 15, 16
IP = C.POINTER(C.c_int)


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB):
        pytest.skip("libddp_amd.so not built")
    try:
        L = C.CDLL(LIB)
    except OSError as e:                      # no HIP runtime on this host
        pytest.skip(str(e))
    L.ddp_sh_max_tiles.restype = C.c_int
    L.ddp_sh_max_tiles.argtypes = [C.c_int, C.c_int]
    L.ddp_sh_item_plan.restype = C.c_int
    L.ddp_sh_item_plan.argtypes = [C.c_int, IP, C.c_uint, C.c_int, C.c_int, C.c_int, IP, IP, C.c_int, IP, C.c_int, IP, C.c_int]
    return L


def scalars(L, counts, hit, ncu, wmax, N):
    cnt = np.asarray(counts, np.int32)
    sc = np.zeros(10, np.int32)
    assert L.ddp_sh_item_plan(len(cnt), cnt.ctypes.data_as(IP), hit, ncu, wmax, N, sc.ctypes.data_as(IP), None, 0, None, 0, None, 0) >= 0
    return tuple(int(v) for v in sc)


class Plan:
    def __init__(self, L, counts, hit, ncu, wmax, N):
        cnt = np.asarray(counts, np.int32)
        sc = np.zeros(10, np.int32)
        W = L.ddp_sh_item_plan(len(cnt), cnt.ctypes.data_as(IP), hit, ncu, wmax, N, sc.ctypes.data_as(IP), None, 0, None, 0, None, 0)
        assert W >= 0
        self.T, self.Wc, self.warm, self.TA, self.NA, self.NWO, self.W, self.WA, self.NW, self.U = (int(v) for v in sc)
        assert W == self.W
        self.items, self.units, self.writers = np.zeros((W, 4), np.int32), np.zeros((self.U, 4), np.int32), np.zeros((W, NWAVES), np.int32)
        L.ddp_sh_item_plan(len(cnt), cnt.ctypes.data_as(IP), hit, ncu, wmax, N, sc.ctypes.data_as(IP), self.items.ctypes.data_as(IP), W,
                           self.units.ctypes.data_as(IP), self.U, self.writers.ctypes.data_as(IP), W)


def check(L, counts, hit, ncu, B, N, first=None):
    """first: the plan of the same launch at another horizon, checked already — only the units may differ"""
    G = len(counts)
    wmax = L.ddp_sh_max_tiles(B, ncu)
    p = Plan(L, counts, hit, ncu, wmax, N)
    ctx = (ncu, B, N, G, hex(hit), counts[:4], vars(p) if p.W < 40 else (p.T, p.Wc, p.warm, p.TA, p.NA, p.NWO, p.W, p.WA, p.NW, p.U))
    nchk = (N - 1) // CH + 1
    if hit == 0:
        assert not p.warm and (p.T, p.W) == device_tiles(counts, ncu, wmax), ctx
    assert p.W <= wmax and p.W == p.Wc + p.NA + p.NWO, ctx
    if not p.warm:
        assert p.NA == p.NWO == p.U == p.NW == 0, ctx
    else:
        assert hit != 0 and 4 <= p.TA <= TMAX and p.TA % 4 == 0 and p.NA >= 1, ctx
        # the work-groups of the hit path fit the compute units that the producers and the classic tiles leave (one when they leave none)
        misses = G - bin(hit).count("1")
        assert p.NWO <= max(ncu - misses - p.Wc - p.NA, 0), ctx
    if first is not None:
        assert np.array_equal(p.items, first.items) and np.array_equal(p.writers, first.writers), ctx
        assert (p.T, p.Wc, p.warm, p.TA, p.NA, p.NWO, p.W, p.WA, p.NW) == (first.T, first.Wc, first.warm, first.TA, first.NA, first.NWO, first.W, first.WA, first.NW), ctx
    # every trajectory of every group in exactly one tile of the right kind
    kind, g, t0, n_ = (p.items[:, e] for e in range(4))
    assert np.all(kind[:p.Wc] == 0) and np.all(kind[p.Wc:p.Wc + p.NA] == 1) and np.all(kind[p.Wc + p.NA:] == 2), ctx
    for gg in range(G if first is None else 0):
        want = 1 if (p.warm and (hit >> gg) & 1) else 0
        sel = (g == gg) & (kind < 2)
        assert np.all(kind[sel] == want), ctx
        size = p.TA if want else p.T
        assert np.all((n_[sel] >= 1) & (n_[sel] <= size)), ctx
        cover = np.bincount(t0[sel], minlength=counts[gg] + 1) - np.bincount(t0[sel] + n_[sel], minlength=counts[gg] + 1)
        assert len(cover) == counts[gg] + 1 and np.all(np.cumsum(cover)[:-1] == 1), ctx
    assert np.all(g[kind < 2] >= 0) and np.all(g[kind < 2] < G), ctx
    if not p.warm:
        return p
    # units: (chunk, trajectory) of every hit group exactly once, nothing of a group that missed
    ug, uq, ut, un = (p.units[:, e] for e in range(4))
    assert p.U == sum(nchk * ((counts[gg] + WTB - 1) // WTB) for gg in range(G) if (hit >> gg) & 1), ctx
    assert np.all((uq >= 0) & (uq < nchk) & (un >= 1) & (un <= WTB) & (ut >= 0)), ctx
    for gg in range(G):
        sel = ug == gg
        if not (hit >> gg) & 1:
            assert not sel.any(), ctx
            continue
        assert np.all(ut[sel] + un[sel] <= counts[gg]), ctx
        # (every unit is a whole block of the group's partition into blocks of WTB trajectories, the last one ragged: the units cover every
        # (chunk, trajectory) exactly once if and only if their (chunk, block) pairs are all the pairs, each once)
        nb = (counts[gg] + WTB - 1) // WTB
        assert np.all(ut[sel] % WTB == 0) and np.all(un[sel] == np.minimum(WTB, counts[gg] - ut[sel])), ctx
        key = uq[sel].astype(np.int64) * nb + ut[sel] // WTB
        assert len(key) == nchk * nb and np.array_equal(np.sort(key), np.arange(nchk * nb)), ctx
    # writer waves: 0 .. NW - 1, each once, only in hit-path work-groups; an affine tile keeps its DMA wave and TA / 4 affine waves
    if first is not None:
        return p
    wr = p.writers
    assert np.all(wr[:p.Wc] == -1), ctx
    ids = np.sort(wr[wr >= 0])
    assert p.NW == p.NA * p.WA + p.NWO * NWAVES and np.array_equal(ids, np.arange(p.NW)) and p.NW >= 1, ctx
    # (an affine tile's spare waves write only when there is no writer-only work-group)
    assert p.WA == (0 if p.NWO > 0 else NWAVES - 1 - p.TA // 4) and np.all(wr[p.Wc:p.Wc + p.NA, :NWAVES - p.WA] == -1), ctx
    return p


def masks(G):
    return sorted({0, (1 << G) - 1, 1, 1 << (G - 1), 0x5555 & ((1 << G) - 1), 0xAAAA & ((1 << G) - 1)})


@pytest.mark.parametrize("ncu", [256, 304, 64, 20])
def test_the_plan_over_the_tile_sweep(lib, ncu):
    rng = np.random.default_rng(ncu)
    nwarm = 0
    for G in (1, 2, 3, 8, 15, 16):
        slots = max(ncu - G, 8)
        edges = {k * TMAX * slots + d for k in (1, 2, 3, 4, 5) for d in (-33, -1, 0, 1, 31, 32, 33, 100)}
        for B in sorted(edges | {G * 2, 1024, 2048, 8000, 8160, 32768, 100000}):
            if B < 2 * G:
                continue
            shapes = [np.full(G, B // G)]
            shapes.append(np.r_[np.full(G - 1, 2), B - 2 * (G - 1)])
            shapes.append(np.maximum(2, rng.multinomial(B - 2 * G, rng.dirichlet(np.ones(G))) + 2))
            shapes.append(np.maximum(2, (np.full(G, B // G) * rng.uniform(0.3, 1.0, G)).astype(int)))
            for c in shapes:
                c = [int(v) for v in c if v >= 2]
                if sum(c) > B or not c:
                    continue
                for hit in masks(len(c)):
                    first = check(lib, c, hit, ncu, B, 16)
                    nwarm += first.warm
                    for N in (17, 24, 1000):
                        if first.warm:
                            check(lib, c, hit, ncu, B, N, first)
                        else:                   # no unit: the horizon must not move the plan (checked in full at N = 16)
                            assert scalars(lib, c, hit, ncu, lib.ddp_sh_max_tiles(B, ncu), N) == scalars(lib, c, hit, ncu, lib.ddp_sh_max_tiles(B, ncu), 16)
    assert nwarm > 100          # the sweep does reach the split


def test_the_benchmark_launch(lib):
    """B = 1 024 trajectories of one λ on 256 compute units, N = 1 000: cold 205 tiles of 5 (the parent's), warm 128 affine tiles of 8
    and 128 writer-only work-groups, 125 chunks x 64 blocks of 16 trajectories"""
    cold = check(lib, [1024], 0, 256, 1024, 1000)
    assert (cold.T, cold.W) == (5, 205)
    warm = check(lib, [1024], 1, 256, 1024, 1000)
    assert (warm.warm, warm.Wc, warm.TA, warm.NA, warm.NWO, warm.U) == (1, 0, 8, 128, 128, 125 * 64)
    assert (warm.WA, warm.NW) == (0, 128 * 15)


@pytest.mark.parametrize("B", [1025, 2048, 32768])
def test_a_batch_beyond_the_measured_gain_is_not_split(lib, B):
    p = check(lib, [B], 1, 256, B, 1000)
    assert not p.warm and (p.T, p.W) == device_tiles([B], 256, lib.ddp_sh_max_tiles(B, 256))


def test_a_small_hit_beside_a_machine_filling_miss(lib):
    """the classic tiles of the group that misses leave no compute unit: affine tiles of 32 whose 6 spare waves write the units"""
    p = check(lib, [1260, 70], 2, 256, 1330, 17)
    assert (p.warm, p.T, p.Wc, p.TA, p.NA, p.NWO, p.WA, p.NW) == (1, 5, 252, 32, 3, 0, 6, 18)
    # ten more trajectories in the group that misses: 254 classic tiles and 3 affine ones are more than the list holds, nothing is split
    p = check(lib, [1270, 70], 2, 256, 1340, 17)
    assert not p.warm and p.W <= lib.ddp_sh_max_tiles(1340, 256)
