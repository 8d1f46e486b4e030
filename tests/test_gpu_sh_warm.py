"""The split of the λ groups that hit a kept record stream (csrc/back_pass_sh.hip, sh_item_plan): affine tiles for Vx, k, dV, diverge
and broadcast units — (group, chunk of 8 steps, block of 16 trajectories) — whose writer waves store Vxx | K | Quu from the stream in
global memory.  Every call runs on two handles, reuse on and off, and the WHOLE output buffers are compared bit for bit; they are
refilled with 7.0 in front of every call, so an element the writers of a warm call skip shows as a difference.  Every call is also
compared with the C oracle (worst relative error below 1e-10, test_gpu_sh_reuse.Call.oracle).
Shapes: N in {16, 17, 23, 41} — empty, one-step, ragged top chunk, several chunks; B in {2, 5, 33, 70} — one pair, one affine wave
plus one trajectory, more than TMAX = 32 trajectories, blocks of 16 that do not divide the group; and the batches at which the plan takes
another path on 256 compute units: 520 and 1 024 (affine tiles of 8: two affine waves), 1 028 (more than SH_WARM_MAX = 1 024 hit
trajectories: classic tiles), and a group of 70 that hits beside one of 1 260 that misses (its classic tiles leave no compute unit free:
affine tiles of 32 whose spare waves write the units, no writer-only work-group)."""
import ctypes as C
import types

import numpy as np
import pytest

from test_gpu_shared_lti import _check_all, _lti, _lti_failing
from test_gpu_sh_reuse import NAMES, Call, Pair, handles, same  # noqa: F401  (handles: the fixture)

pytestmark = pytest.mark.gpu
n, m = 10, 2


def refill(pair):
    """7.0 into every output buffer of both handles (7 into diverge)"""
    for c in (pair.on, pair.off):
        for k, s in c.shapes.items():
            v = np.full(s, 7.0)
            c._lib.check(c._lib.lib().ddp_memcpy_h2d(c.h._h, c.o[k], v.ctypes.data_as(C.c_void_p), C.c_size_t(v.nbytes)))
        v = np.full(c.B, 7, np.int32)
        c._lib.check(c._lib.lib().ddp_memcpy_h2d(c.h._h, c.o["diverge"], v.ctypes.data_as(C.c_void_p), C.c_size_t(v.nbytes)))


def run(pair, **kw):
    refill(pair)
    return pair.run(**kw)


@pytest.mark.parametrize("regType", [1, 2])
@pytest.mark.parametrize("B", [2, 5, 33, 70])
@pytest.mark.parametrize("N", [16, 17, 23, 41])
def test_cold_then_warm(handles, N, B, regType):
    rng = np.random.default_rng(100 * N + 2 * B + regType)
    p = Pair(handles, *_lti(rng, N, B)[:7], 0.37, regType)
    a, d1 = run(p)
    b, d2 = run(p)
    p.free()
    assert d1 == (0, 1) and d2 == (1, 0), (d1, d2)
    assert same(a, b)
    assert handles[0].sh_timeouts() == 0 and handles[1].sh_reuse_stats()[0] == 0


@pytest.mark.parametrize("N,B,regType", [(17, 520, 1), (17, 520, 2), (16, 1024, 1), (16, 1028, 1)])
def test_cold_then_warm_at_the_batches_where_the_plan_changes(handles, N, B, regType):
    rng = np.random.default_rng(B + regType)
    p = Pair(handles, *_lti(rng, N, B)[:7], 1.5, regType)
    a, d1 = run(p, grows=True)
    b, d2 = run(p)
    p.free()
    assert d1 == (0, 1) and d2 == (1, 0), (d1, d2)
    assert same(a, b)
    assert handles[0].sh_timeouts() == 0


class Masked:
    """a Pair whose calls carry an activity mask: both handles, whole buffers bit for bit, the active trajectories against the oracle,
    the others untouched"""

    def __init__(self, handles, args, lam, act, regType=1):
        self.p = Pair(handles, *args, lam, regType)
        self.act = np.asarray(act, np.int32)
        self.dact = {c: c.h.to_device(self.act) for c in (self.p.on, self.p.off)}

    def _run(self, c):
        _lib, h, d, o = c._lib, c.h, c.d, c.o
        desc = _lib.BPDesc(n, m, c.N, c.B, 0, 0, 0, 0, c.regType, 0)
        _lib.check(_lib.lib().ddp_back_pass_f64_dev(h._h, C.byref(desc), d["cx"], d["cu"], d["cxx"], d["cxu"], d["cuu"], d["fx"], d["fu"],
                                                    d["lam"], None, None, self.dact[c], o["K"], o["k"], o["Quu"], o["Vx"], o["Vxx"], o["dV"], o["diverge"]))
        h.sync()
        assert h.last_kernel(0) == "sh_back_kernel"
        out = {k: h.to_host(o[k], s) for k, s in c.shapes.items()}
        out["diverge"] = h.to_host(o["diverge"], (c.B,), np.int32)
        return out

    def run(self):
        refill(self.p)
        h = self.p.h
        s0 = h.sh_reuse_stats()
        a = self._run(self.p.on)
        s1 = h.sh_reuse_stats()
        b = self._run(self.p.off)
        for k in NAMES:
            assert np.array_equal(a[k], b[k]), k
        on, off = self.act != 0, self.act == 0
        for k in NAMES:
            assert np.all(a[k][..., off] == 7), k
        hh, c = self.p.on.host, self.p.on
        pol = types.SimpleNamespace(K=a["K"][..., on], k=a["k"][..., on], Σi=a["Quu"][..., on])
        worst = _check_all((a["diverge"][on], pol, a["Vx"][..., on], a["Vxx"][..., on], a["dV"][..., on]), hh["cx"][..., on], hh["cu"][..., on],
                           hh["cxx"], hh["cxu"], hh["cuu"], hh["fx"], hh["fu"], c.lam[on], c.regType, np.zeros((m, c.N, int(on.sum()))))
        print("worst relative error against the oracle: %.3e" % worst)
        assert worst < 1e-10, worst
        return a, (s1[0] - s0[0], s1[1] - s0[1])

    def free(self):
        for c, p_ in self.dact.items():
            c.h.free(p_)
        self.p.free()


@pytest.mark.parametrize("regType", [1, 2])
def test_a_group_that_hits_beside_one_that_misses_singletons_and_holes(handles, regType):
    """call 1: one λ for the batch.  Call 2: that λ on 19 trajectories (a hit: affine tiles and units), a new λ on 17 (its chain and
    classic tiles in the same launch), 6 trajectories with a λ of their own (the per-trajectory kernels), holes in the activity mask in
    every part"""
    rng = np.random.default_rng(40 + regType)
    N, B = 23, 42
    act = np.ones(B, np.int32)
    act[[0, 7, 18, 20, 35, 37, 41]] = 0
    mk = Masked(handles, _lti(rng, N, B)[:7], 0.8, act, regType)
    _, d1 = mk.run()
    lam = np.r_[np.full(19, 0.8), np.full(17, 2.5), 10.0 + np.arange(6)]
    mk.p.both(lambda c: c.set_lam(lam))
    a, d2 = mk.run()
    b, d3 = mk.run()
    mk.free()
    assert d1 == (0, 1) and d2 == (1, 1) and d3 == (2, 0), (d1, d2, d3)
    assert same(a, b)
    assert handles[0].sh_timeouts() == 0


def test_a_small_group_hits_beside_a_machine_filling_one_that_misses(handles):
    rng = np.random.default_rng(60)
    N, B = 17, 1330
    p = Pair(handles, *_lti(rng, N, B)[:7], 0.8)
    _, d1 = run(p, grows=True)
    p.both(lambda c: c.set_lam(np.r_[np.full(70, 0.8), np.full(B - 70, 2.5)]))
    a, d2 = run(p)
    b, d3 = run(p)
    p.free()
    assert d1 == (0, 1) and d2 == (1, 1) and d3 == (2, 0), (d1, d2, d3)
    assert same(a, b)
    assert handles[0].sh_timeouts() == 0


def test_seventeen_groups_evict_and_recompute_a_slot(handles):
    """λ = 1..16, then 2..17 (15 hits; 17 takes the slot of 1), the same again (16 hits: the survivors), then 1..16 (1 is computed again)"""
    rng = np.random.default_rng(51)
    p = Pair(handles, *_lti(rng, 17, 32)[:7], np.repeat(np.arange(1.0, 17.0), 2))
    _, d1 = run(p)
    p.both(lambda c: c.set_lam(np.repeat(np.arange(2.0, 18.0), 2)))
    a, d2 = run(p)
    b, d3 = run(p)
    p.both(lambda c: c.set_lam(np.repeat(np.arange(1.0, 17.0), 2)))
    _, d4 = run(p)
    _, d5 = run(p)
    p.free()
    assert d1 == (0, 16) and d2 == (15, 1) and d3 == (16, 0) and d4 == (15, 1) and d5 == (16, 0), (d1, d2, d3, d4, d5)
    assert same(a, b)
    assert handles[0].sh_timeouts() == 0


def test_an_operand_poked_after_a_warm_call_empties_every_slot(handles):
    rng = np.random.default_rng(52)
    p = Pair(handles, *_lti(rng, 23, 33)[:7], np.where(np.arange(33) % 3 == 0, 0.5, 1.0))
    _, d1 = run(p)
    _, d2 = run(p)
    old = p.on.host["fx"].reshape(-1, order="F")[37]
    p.both(lambda c: c.poke("fx", 37, np.nextafter(old, np.inf)))
    _, d3 = run(p)                                         # (bit for bit against the handle that never reuses, and the oracle of the new operands)
    _, d4 = run(p)
    p.free()
    assert d1 == (0, 2) and d2 == (2, 0) and d3 == (0, 2) and d4 == (2, 0), (d1, d2, d3, d4)


def test_a_diverging_group_is_never_served_from_a_slot(handles):
    rng = np.random.default_rng(12)
    N, B = 41, 33
    lam = np.array([0.02, 0.04, 0.06, 50.0])[np.arange(B) % 4]
    p = Pair(handles, *_lti_failing(rng, N, B)[:7], lam)
    a, d1 = run(p)
    b, d2 = run(p)
    c_, d3 = run(p)
    p.free()
    nbad = len({l for l, d in zip(lam, a["diverge"]) if d > 0})
    assert nbad >= 1 and a["diverge"][3] == 0, a["diverge"][:4]
    assert d1 == (0, 4) and d2 == (4 - nbad, nbad) and d3 == d2, (d1, d2, d3, nbad)
    assert same(a, b) and same(a, c_)
