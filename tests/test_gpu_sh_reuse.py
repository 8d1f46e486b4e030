"""The record streams the shared-LTI backward pass keeps across calls (csrc/back_pass_sh.hip, "Reuse across calls"): a λ group whose
stream an earlier call of the handle left behind is served from it, and every rule that keeps such a stream from being read for other
operands, another horizon, another regType, another λ, after a divergence, a reallocation, a time-out or a change of stream.
Every call runs on two handles — one created under DDP_SH_REUSE=0 — and the results are compared bit for bit; every trajectory is also
compared with the C oracle (worst relative error below 1e-10).  Shapes: B in 6..40, N in {16, 21, 37}: two chunks of 8 steps with an empty
top chunk, a ragged top chunk, several chunks."""
import ctypes as C
import os
import types

import numpy as np
import pytest

from test_gpu_shared_lti import _check_all, _lti, _lti_failing

pytestmark = pytest.mark.gpu
n, m = 10, 2
OPS = ("cxx", "cxu", "cuu", "fx", "fu")                 # the shared operands in the order of a call's arguments
NAMES = ("K", "k", "Quu", "Vx", "Vxx", "dV", "diverge")


@pytest.fixture
def handles():
    """(reuse on, reuse off): two handles that keep the switches they were created under (their calls go through `_h`, not through
    `raw`, which would read the environment again)"""
    from ddp_amd import _lib
    keys = ("DDP_SH_MIN_B", "DDP_SH_REUSE", "DDP_TEST_SH_ABORT", "DDP_BACKPASS")
    old = {k: os.environ.get(k) for k in keys}
    try:
        for k in keys:
            os.environ.pop(k, None)
        os.environ["DDP_SH_MIN_B"] = "1"
        on = _lib.Handle(0)
        os.environ["DDP_SH_REUSE"] = "0"
        off = _lib.Handle(0)
    finally:
        for k, v in old.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v
    yield on, off
    on.close(); off.close()


class Call:
    """one batch on the device of one handle: operands, λ and results stay where they are between calls (the `_dev` entry point)"""

    def __init__(self, h, cx, cu, cxx, cxu, cuu, A, Bm, lam, regType=1):
        from ddp_amd import _lib
        self._lib, self.h = _lib, h
        self.N, self.B, self.regType = cx.shape[1], cx.shape[2], regType
        self.host = dict(cx=cx, cu=cu, cxx=np.array(cxx, order="F"), cxu=np.array(cxu, order="F"), cuu=np.array(cuu, order="F"),
                         fx=np.array(A, order="F"), fu=np.array(Bm, order="F"))
        self.lam = np.broadcast_to(np.asarray(lam, float), (self.B,)).copy()
        self.d = {k: h.to_device(v) for k, v in self.host.items()}
        self.d["lam"] = h.to_device(self.lam)
        N, B = self.N, self.B
        self.shapes = {"K": (m, n, N, B), "k": (m, N, B), "Quu": (m, m, N, B), "Vx": (n, N, B), "Vxx": (n, n, N, B), "dV": (2, B)}
        self.o = {k: h.to_device(np.full(s, 7.0)) for k, s in self.shapes.items()}
        self.o["diverge"] = h.to_device(np.full(B, 7, np.int32))

    def run(self):
        _lib, h, d, o = self._lib, self.h, self.d, self.o
        desc = _lib.BPDesc(n, m, self.N, self.B, 0, 0, 0, 0, self.regType, 0)
        _lib.check(_lib.lib().ddp_back_pass_f64_dev(h._h, C.byref(desc), d["cx"], d["cu"], d["cxx"], d["cxu"], d["cuu"], d["fx"], d["fu"],
                                                    d["lam"], None, None, None, o["K"], o["k"], o["Quu"], o["Vx"], o["Vxx"], o["dV"], o["diverge"]))
        h.sync()
        assert h.last_kernel(0) == "sh_back_kernel"
        out = {k: h.to_host(o[k], s) for k, s in self.shapes.items()}
        out["diverge"] = h.to_host(o["diverge"], (self.B,), np.int32)
        return out

    def poke(self, name, flat, value):
        """one double of a shared operand, in place on the device"""
        self.host[name].reshape(-1, order="F")[flat] = value
        v = np.array([value])
        self._lib.check(self._lib.lib().ddp_memcpy_h2d(self.h._h, C.c_void_p(self.d[name].value + 8 * flat), v.ctypes.data_as(C.c_void_p), C.c_size_t(8)))

    def set_lam(self, lam):
        self.lam = np.broadcast_to(np.asarray(lam, float), (self.B,)).copy()
        self._lib.check(self._lib.lib().ddp_memcpy_h2d(self.h._h, self.d["lam"], self.lam.ctypes.data_as(C.c_void_p), C.c_size_t(8 * self.B)))

    def free(self):
        for p_ in list(self.d.values()) + list(self.o.values()):
            self.h.free(p_)

    def oracle(self, out):
        """every trajectory against the C oracle: _check_all's own assertions (1e-8) and the worst error below 1e-10"""
        hh = self.host
        pol = types.SimpleNamespace(K=out["K"], k=out["k"], Σi=out["Quu"])
        worst = _check_all((out["diverge"], pol, out["Vx"], out["Vxx"], out["dV"]), hh["cx"], hh["cu"], hh["cxx"], hh["cxu"], hh["cuu"], hh["fx"], hh["fu"],
                           self.lam, self.regType, np.zeros((m, self.N, self.B)))
        print("worst relative error against the oracle: %.3e" % worst)
        assert worst < 1e-10, worst


class Pair:
    """the same batch on both handles"""

    def __init__(self, handles, *args, **kw):
        self.on, self.off = Call(handles[0], *args, **kw), Call(handles[1], *args, **kw)
        self.h = handles[0]

    def both(self, f):
        f(self.on); f(self.off)

    def run(self, grows=False):
        """runs the call on both handles; the results must agree bit for bit and with the oracle.  Returns the results and the
        (hits, misses) this call added on the reusing handle (grows: the call reallocates the scratch, and the counters start again
        with it)"""
        s0 = (0, 0) if grows else self.h.sh_reuse_stats()
        a = self.on.run()
        s1 = self.h.sh_reuse_stats()
        b = self.off.run()
        for k in NAMES:
            assert np.array_equal(a[k], b[k]), k
        self.on.oracle(a)
        return a, (s1[0] - s0[0], s1[1] - s0[1])

    def free(self):
        self.both(Call.free)


def same(a, b):
    return all(np.array_equal(a[k], b[k]) for k in NAMES)


@pytest.mark.parametrize("regType", [1, 2])
@pytest.mark.parametrize("N,B", [(16, 6), (21, 9), (37, 40)])
def test_the_same_call_twice_is_served_from_the_kept_stream(handles, N, B, regType):
    rng = np.random.default_rng(1000 + 10 * N + regType)
    p = Pair(handles, *_lti(rng, N, B)[:7], 0.37, regType)
    a, d1 = p.run()
    b, d2 = p.run()
    p.free()
    assert d1 == (0, 1) and d2 == (1, 0), (d1, d2)
    assert same(a, b)
    assert handles[1].sh_reuse_stats()[0] == 0           # DDP_SH_REUSE=0 never reuses
    assert handles[0].sh_timeouts() == 0


@pytest.mark.parametrize("end", ["first", "last"])
@pytest.mark.parametrize("name", ["fx", "fu", "cxx", "cxu", "cuu"])
def test_an_operand_changed_in_place_by_one_bit_is_noticed(handles, name, end):
    """same device pointers, the first or the last double of one shared operand moved to the next representable number between two
    calls: a miss, and the result of the new operands"""
    rng = np.random.default_rng(7 + OPS.index(name))
    p = Pair(handles, *_lti(rng, 21, 8)[:7], 1.0)
    _, d1 = p.run()
    _, d1b = p.run()
    flat = 0 if end == "first" else p.on.host[name].size - 1
    old = p.on.host[name].reshape(-1, order="F")[flat]
    new = np.nextafter(old, np.inf)
    assert new != old
    p.both(lambda c: c.poke(name, flat, new))
    _, d2 = p.run()                                       # (compared with the handle that never reuses and with the oracle of the new operands)
    _, d3 = p.run()
    p.free()
    assert d1 == (0, 1) and d1b == (1, 0) and d2 == (0, 1) and d3 == (1, 0), (d1, d1b, d2, d3)


def test_a_lambda_comes_back(handles):
    rng = np.random.default_rng(21)
    p = Pair(handles, *_lti(rng, 37, 7)[:7], 1.0)
    a, d1 = p.run()
    p.both(lambda c: c.set_lam(2.0))
    b, d2 = p.run()
    p.both(lambda c: c.set_lam(1.0))
    c_, d3 = p.run()
    p.free()
    assert d1 == (0, 1) and d2 == (0, 1) and d3 == (1, 0), (d1, d2, d3)
    assert same(a, c_) and not np.array_equal(a["K"], b["K"])


def test_one_group_hits_beside_one_that_misses(handles):
    rng = np.random.default_rng(22)
    la, lb, lc = 0.5, 1.0, 3.0
    p = Pair(handles, *_lti(rng, 21, 8)[:7], np.repeat([la, lb], 4))
    a, d1 = p.run()
    p.both(lambda c: c.set_lam(np.repeat([lb, lc], 4)))
    b, d2 = p.run()
    p.free()
    assert d1 == (0, 2) and d2 == (1, 1), (d1, d2)
    # λb moved from the second half of the batch to the first; λc is neither of the streams of the first call
    assert np.array_equal(b["K"][..., 0], a["K"][..., 4]) and not np.array_equal(b["K"][..., 4], a["K"][..., 0])
    assert not np.array_equal(b["K"][..., 4], a["K"][..., 4])


def test_sixteen_groups_evict_sixteen_others(handles):
    rng = np.random.default_rng(23)
    first, other = np.repeat(np.arange(1.0, 17.0), 2), np.repeat(np.arange(17.0, 33.0), 2)
    p = Pair(handles, *_lti(rng, 16, 32)[:7], first)
    _, d1 = p.run()
    p.both(lambda c: c.set_lam(other))
    _, d2 = p.run()
    p.both(lambda c: c.set_lam(first))
    a, d3 = p.run()
    b, d4 = p.run()
    p.free()
    assert d1 == (0, 16) and d2 == (0, 16) and d3 == (0, 16) and d4 == (16, 0), (d1, d2, d3, d4)
    assert same(a, b)


def test_another_horizon_never_reads_a_kept_stream(handles):
    """N 21 -> 37 -> 21 (-> 37) with the same shared operands and λ: the streams are laid out by absolute step, every call is a miss"""
    rng = np.random.default_rng(24)
    cx, cu, cxx, cxu, cuu, A, Bm, _ = _lti(rng, 37, 8)
    ps = {N: Pair(handles, cx[:, :N], cu[:, :N], cxx, cxu, cuu, A, Bm, 1.0) for N in (21, 37)}
    ds = [ps[N].run(grows=(i == 1))[1] for i, N in enumerate((21, 37, 21, 37))]        # (more chunks: the second call reallocates)
    for p in ps.values():
        p.free()
    assert ds == [(0, 1)] * 4, ds


def test_another_regtype_never_reads_a_kept_stream(handles):
    rng = np.random.default_rng(25)
    args = _lti(rng, 21, 8)[:7]
    ps = {r: Pair(handles, *args, 1.0, r) for r in (1, 2)}
    ds = [ps[r].run()[1] for r in (1, 2, 1)]
    for p in ps.values():
        p.free()
    assert ds == [(0, 1)] * 3, ds


def test_a_diverged_group_is_never_kept(handles):
    """the operands and λ values of test_divergence_follows_the_group: the groups that lose positive definiteness are computed again in
    the repeat (same diverge, same zeros), the healthy group beside them is reused"""
    rng = np.random.default_rng(12)
    N, B = 37, 40
    lam = np.array([0.02, 0.04, 0.06, 50.0])[np.arange(B) % 4]
    p = Pair(handles, *_lti_failing(rng, N, B)[:7], lam)
    a, d1 = p.run()
    b, d2 = p.run()
    p.free()
    nbad = len({l for l, d in zip(lam, a["diverge"]) if d > 0})
    assert nbad >= 1 and a["diverge"][3] == 0, a["diverge"][:4]
    assert d1 == (0, 4) and d2 == (4 - nbad, nbad), (d1, d2, nbad)
    assert same(a, b)
    for b_ in range(B):
        d = a["diverge"][b_]
        if d > 0:
            assert not a["K"][:, :, :d, b_].any() and not a["Vxx"][:, :, :d, b_].any() and not a["Vx"][:, :d, b_].any() and not a["k"][:, :d, b_].any()


def test_a_reallocated_scratch_starts_empty(handles):
    """B = 8, 40, 8 with the same operands and λ: every call correct.  (The scratch is laid out in 256-byte pieces and its list of
    trajectories holds 64 of them in one, so B = 40 does not reallocate it — the second call is a hit.)  B = 72 does: the counters start
    again with the new block, the call is a miss, and B = 8 behind it is served from the stream that call left."""
    rng = np.random.default_rng(26)
    cx, cu, cxx, cxu, cuu, A, Bm, _ = _lti(rng, 21, 72)
    ps = {B: Pair(handles, cx[..., :B], cu[..., :B], cxx, cxu, cuu, A, Bm, 1.0) for B in (8, 40, 72)}
    st = []
    for B in (8, 40, 8, 72, 8):
        ps[B].run()
        st.append(handles[0].sh_reuse_stats())
    for p in ps.values():
        p.free()
    assert st == [(0, 1), (1, 1), (2, 1), (0, 1), (1, 1)], st


def test_a_timed_out_call_on_a_warm_handle(handles, monkeypatch):
    """DDP_TEST_SH_ABORT on a handle whose stream is warm: what test_a_timed_out_tile_hands_its_trajectories_to_the_per_trajectory_kernels
    expects of such a call, and the next normal call is correct"""
    from ddp_amd import _lib
    from conftest import relerr
    h = handles[0]
    rng = np.random.default_rng(77)
    N, B = 37, 40
    lam = np.where(np.arange(B) % 3 == 0, 0.5, 1.0)
    p = Pair(handles, *_lti(rng, N, B)[:7], lam)
    good, d1 = p.run()
    _, d1b = p.run()
    assert d1 == (0, 2) and d1b == (2, 0)
    t0 = h.sh_timeouts()
    monkeypatch.setenv("DDP_SH_MIN_B", "1")
    monkeypatch.setenv("DDP_TEST_SH_ABORT", "1")
    _lib.check(_lib.lib().ddp_reload_env(h._h))
    s0 = h.sh_reuse_stats()
    out = p.on.run()
    assert h.sh_reuse_stats()[0] == s0[0]                  # nothing is reused under the switch
    assert h.sh_timeouts() > t0
    info = h.sh_timeout_info()
    assert info["records"] and any(r["chunk"] == 1 and 0 <= r["group"] < 2 and r["groups"] == 2 and r["waited_ms"] < 4000 for r in info["records"]), info
    monkeypatch.delenv("DDP_TEST_SH_ABORT")
    _lib.check(_lib.lib().ddp_reload_env(h._h))
    hh = p.on.host
    pol = types.SimpleNamespace(K=out["K"], k=out["k"], Σi=out["Quu"])
    _check_all((out["diverge"], pol, out["Vx"], out["Vxx"], out["dV"]), hh["cx"], hh["cu"], hh["cxx"], hh["cxu"], hh["cuu"], hh["fx"], hh["fu"], lam, 1,
               np.zeros((m, N, B)))
    for k in ("K", "Vx", "Vxx", "dV"):
        assert relerr(out[k], good[k]) < 1e-10
    t1 = h.sh_timeouts()
    again, d3 = p.run()
    p.free()
    assert same(again, good) and h.sh_timeouts() == t1
    assert d3 == (0, 2), d3                                # the aborted call left nothing behind that counts as complete


def test_a_call_on_another_stream_starts_from_empty_slots(handles):
    """the handle is put on another HIP stream (as the slot scheduler does for its side stream) after a warm call: the kept streams
    were ordered against the old stream only, so the call counts misses; staying on the new stream reuses again"""
    from ddp_amd import _lib
    L = _lib.lib()
    h, other = handles
    rng = np.random.default_rng(27)
    p = Pair(handles, *_lti(rng, 21, 8)[:7], 1.0)
    a, d1 = p.run()
    _, d2 = p.run()
    prev = C.c_void_p()
    side = _lib.Handle(0)                                  # (its stream is the other stream)
    L.ddp_sh_test_swap_stream.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p)]
    try:
        _lib.check(L.ddp_sh_test_swap_stream(h._h, C.c_void_p(L.ddp_stream(side._h)), C.byref(prev)))
        b, d3 = p.run()
        _, d4 = p.run()
    finally:
        _lib.check(L.ddp_sh_test_swap_stream(h._h, prev, None))
    c_, d5 = p.run()
    p.free()
    side.close()
    assert d1 == (0, 1) and d2 == (1, 0) and d3 == (0, 1) and d4 == (1, 0) and d5 == (0, 1), (d1, d2, d3, d4, d5)
    assert same(a, b) and same(a, c_)
