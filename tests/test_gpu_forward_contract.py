"""What ddp_forward_pass_f64_dev promises the device-resident iLQG driver, for every rollout kernel of the registered families
(csrc/forward_pass*.hip), asserted through the device entry itself: the `active` mask (an inactive trajectory's rows of all four
outputs keep their bits), `csum` (= sum(cnew), what the line search accepts a step on), which kernel a call gets (ddp_last_kernel(h, 1),
one TABLE of calls in the style of tests/test_bp_choice.py, every threshold pinned on both sides) and the rollouts themselves at
32 < n < 64.  Every rollout of every case is compared with a longdouble restatement of src/forward_pass.jl:9-33
(tests/test_forward_reference_cpu.py, which checks it against the C oracle without a GPU); the pendulum with the C oracle."""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import par_map
from forward_contract_cases import BIG, DPP, GRP, MID, PIPE, PIPE4, ROW, TABLE, _id, lq102, pend, row
from test_forward_reference_cpu import LD, RTOL, clamped_share, lq_reference, make_lq_case, need_longdouble, rollout_dist

pytestmark = pytest.mark.gpu
CSUM_TOL = 1e-12                              # csum against the longdouble sum of the kernel's own cnew (tests/test_gpu_full_size.py)
# what xnew, unew, cnew, csum hold before a call: quiet NaNs with a payload of their own each (the hardware hands a NaN operand's payload
# on, so a csum summed from an untouched cnew would otherwise still look untouched)
SENT = tuple(np.uint64(0x7FF8DEAD5EED1230 + i) for i in range(4))
MASKS = ("none", "first", "last", "alt", "mid")       # beside all active / NULL, which every case runs first
A16 = np.array([1.0, 0.5, 0.0, 0.25, 0.5, 1.0, 0.1, 0.03, 0.0, 0.7, 0.25, 0.01, 0.003, 1.0, 0.001, 0.5])   # 0, 1 and repeated values


# ------------------------------------------------------------------------------------------------------------ cases and references
def make_case(r, N, seed, alpha=None, nan=None):
    al = 10.0 ** np.linspace(0, -3, r["na"]) if alpha is None else np.asarray(alpha, float)
    if r["fam"] == "lq":
        return make_lq_case(seed, r["n"], r["m"], N, r["B"], al, r["dyn"], r["pol"], r["lims"], r["full"], nan)
    from oracle import np_restatement as npr
    rng = np.random.default_rng(seed)
    P, B = npr.PENDCART, r["B"]
    Q = P["Q"] + (0.3 * np.ones((4, 4)) if r["full"] else 0)
    x0 = np.array([np.pi - 0.5, 0.0, 0.0, 0.0])[:, None] + 0.1 * rng.standard_normal((4, B))
    c = dict(kind="pend", n=4, m=1, N=N, B=B, dyn="", Q=Q, R=P["R"], full=r["full"], alpha=al, x0=x0, u=1.5 * rng.standard_normal((1, N, B)),
             K=None, k=None, x=None, lims=np.array([[-2.0, 2.0]]) if r["lims"] else None)
    if r["pol"]:
        x = np.cumsum(0.05 * rng.standard_normal((4, N, B)), axis=1) + x0[:, None, :]
        x[:, 0] = x0
        c.update(K=0.3 * rng.standard_normal((1, 4, N, B)), k=0.2 * rng.standard_normal((1, N, B)), x=x)
    if nan is not None:
        c["u"][0, N // 2, nan] = np.nan
        if r["pol"]:
            c["k"][0, min(N - 1, 1), nan] = np.nan
    return c


def reference(c):
    """xnew, unew, cnew, csum of every rollout: the longdouble restatement (LQ) or the C oracle with the longdouble sum of ITS cnew"""
    if c["kind"] == "lq":
        return lq_reference(c)
    from oracle import np_restatement as npr
    from oracle import oracle_ctypes as oc
    N, B, na = c["N"], c["B"], len(c["alpha"])
    po = oc.make_problem("pendcart", 4, 1, N, Q=c["Q"], R=c["R"], pend=npr.PENDCART)
    xs, us, cn = np.empty((4, N, B, na)), np.empty((1, N, B, na)), np.empty((N + 1, B, na))

    def one(b):
        pol = None if c["K"] is None else (c["K"][..., b], c["k"][..., b])
        for ai in range(na):
            xs[:, :, b, ai], us[:, :, b, ai], cn[:, b, ai] = oc.forward_pass(po, pol, c["x0"][:, b], c["u"][..., b],
                                                                            None if pol is None else c["x"][..., b], float(c["alpha"][ai]), c["lims"])
    par_map(one, range(B), workers=min(16, len(os.sched_getaffinity(0))))
    return xs.astype(LD), us.astype(LD), cn.astype(LD), cn.astype(LD).sum(axis=0)


def mask_of(pattern, B):
    a = np.ones(B, np.int32)
    if pattern == "none":
        a[:] = 0
    elif pattern == "first":
        a[1:] = 0
    elif pattern == "last":
        a[:-1] = 0
    elif pattern == "alt":
        a[1::2] = 0
    elif pattern == "mid":                    # one inactive trajectory inside a wave's group of four rollouts
        a[min(B - 1, 4 * ((B // 2) // 4) + 1)] = 0
    else:
        assert pattern == "all"
    return a


# ------------------------------------------------------------------------------------------------------- the driver (device entry)
class OnDevice:
    """a case's operands on the device (the listed ones 8 bytes into their allocation), its four outputs allocated once; run(active)
    fills the outputs with the sentinel, calls ddp_forward_pass_f64_dev and returns [xnew, unew, cnew, csum, ddp_last_kernel(h, 1)]"""

    def __init__(self, h, c, mis=()):
        from ddp_amd import _lib
        self.h, self.c, self.L, self.bufs = h, c, _lib.lib(), []
        n, m, N, B, na = c["n"], c["m"], c["N"], c["B"], len(c["alpha"])
        self.CL = N + 1 if c["kind"] == "pend" else N
        try:
            dev = {k: self.put(c[k], k in mis) for k in ("K", "k", "u", "x", "x0", "Q", "R", "lims")}
            P = _lib.Problem()
            P.kind, P.n, P.m, P.N, P.B = int(c["kind"] == "pend"), n, m, N, B
            P.Q, P.R, P.cost_diag = dev["Q"], dev["R"], int(not c["full"])
            if c["kind"] == "lq":
                P.A, P.Bm = self.put(c["A"], "A" in mis), self.put(c["Bm"], "B" in mis)
                P.dyn_tv, P.dyn_batched = int("F" in c["dyn"]), int("f" in c["dyn"])
            else:
                from oracle import np_restatement as npr
                P.g, P.l, P.h, P.d = (npr.PENDCART[k] for k in "glhd")
                for i in range(4):
                    P.goal[i] = float(npr.PENDCART["goal"][i])
            self.P, self.dev = P, dev
            self.shapes = ((n, N, B, na), (m, N, B, na), (self.CL, B, na), (B, na))
            self.outs = [self.alloc(8 * int(np.prod(s))) for s in self.shapes]
            self.act = self.alloc(4 * B)
            self.fill = [np.full(int(np.prod(s)), v, np.uint64) for s, v in zip(self.shapes, SENT)]
            self.alpha = np.ascontiguousarray(c["alpha"], np.float64)
        except Exception:
            self.close()
            raise

    def alloc(self, nbytes):
        p = self.h.malloc(nbytes + 16)
        self.bufs.append(p)
        return p.value

    def copy_in(self, dst, a):
        from ddp_amd import _lib
        _lib.check(self.L.ddp_memcpy_h2d(self.h.raw, C.c_void_p(dst), a.ctypes.data_as(C.c_void_p), C.c_size_t(a.nbytes)))

    def put(self, a, off=False):
        if a is None:
            return None
        a = np.asfortranarray(a, dtype=np.float64)
        p = self.alloc(a.nbytes) + (8 if off else 0)
        assert p % 16 == (8 if off else 0)
        self.copy_in(p, a)
        return p

    def run(self, active):
        from ddp_amd import _lib
        for p, f in zip(self.outs, self.fill):
            self.copy_in(p, f)
        if active is not None:
            self.copy_in(self.act, np.ascontiguousarray(active, np.int32))
        d = self.dev
        ptrs = [d["K"], d["k"], d["x0"], d["u"], d["x"], self.alpha.ctypes.data]
        tail = [d["lims"], None if active is None else self.act] + self.outs
        _lib.check(self.L.ddp_forward_pass_f64_dev(self.h.raw, C.byref(self.P), *[C.c_void_p(a) for a in ptrs], C.c_int(len(self.alpha)),
                                                   *[C.c_void_p(a) for a in tail]))
        self.h.sync()
        out = [self.h.to_host(C.c_void_p(p), s) for p, s in zip(self.outs, self.shapes)]
        return out + [self.h.last_kernel(1)]

    def close(self):
        for p in self.bufs:
            self.h.free(p)
        self.bufs = []

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def untouched(a, which):
    return bool(np.all(bits(a) == SENT[which]))


def check_outputs(c, ref, out, active, worst, what):
    """the contract of one call: active rollouts against the reference, csum both ways, x̂_0 = x0 and the sentinel of the rest bit for bit"""
    xn, un, cn, cs = out[:4]
    on = np.ones(c["B"], bool) if active is None else np.asarray(active) != 0
    for i, (name, a) in enumerate((("xnew", xn), ("unew", un), ("cnew", cn), ("csum", cs))):
        assert untouched(a[..., ~on, :], i), (what, name, "of an inactive trajectory was written")
    if not on.any():
        return
    for name, got, want in (("xnew", xn, ref[0]), ("unew", un, ref[1]), ("cnew", cn, ref[2])):
        d = rollout_dist(got[..., on, :], want[..., on, :])
        worst[name] = max(worst.get(name, 0.0), float(np.max(d)))
        assert np.all(d < RTOL), (what, name, float(np.nanmax(d)), np.argwhere(~(d < RTOL))[:4].tolist())
    d = (np.abs(cs[on].astype(LD) - ref[3][on]) / np.abs(ref[3][on])).astype(float)
    worst["csum"] = max(worst.get("csum", 0.0), float(np.max(d)))
    assert np.all(d < RTOL), (what, "csum", float(np.nanmax(d)), np.argwhere(~(d < RTOL))[:4].tolist())
    own = cn[:, on].astype(LD).sum(axis=0)
    d = (np.abs(cs[on].astype(LD) - own) / np.abs(own)).astype(float)
    worst["csum_own"] = max(worst.get("csum_own", 0.0), float(np.max(d)))
    assert np.all(d < CSUM_TOL), (what, "csum against the sum of cnew", float(np.nanmax(d)), np.argwhere(~(d < CSUM_TOL))[:4].tolist())
    assert np.array_equal(bits(xn[:, 0][:, on]), bits(np.repeat(c["x0"][:, on, None], xn.shape[-1], 2))), (what, "xnew[:, 0] is not x0")


@pytest.fixture
def handle(monkeypatch):
    need_longdouble()
    from ddp_amd import _lib
    for k in [k for k in os.environ if k.startswith("DDP_") and not k.startswith("DDP_AMD_")]:      # (kernel switches, not the loader's)
        monkeypatch.delenv(k)
    return _lib.default_handle()              # (Handle.raw re-reads the DDP_* switches whenever they changed: ddp_reload_env)


# ------------------------------------------------------------------------------------------------------------------- the table
@pytest.mark.parametrize("r", TABLE, ids=_id)
def test_forward_contract(handle, monkeypatch, r):
    """one row of the table at each of its horizons: NULL and all-ones masks give the same bits, then every mask pattern"""
    for k, v in r["env"].items():
        monkeypatch.setenv(k, v)
    worst = {}
    for N in r["Ns"]:
        c = make_case(r, N, 7919 * TABLE.index(r) + N)
        ref = reference(c)
        if r["lims"] and ref[1].size >= 200:                       # (a handful of controls, N = 1 .. 3, says nothing about the share)
            share = clamped_share(c, ref[1])
            assert 0.1 < share < 0.9, (N, share)
        with OnDevice(handle, c, r["mis"]) as dev:
            out = dev.run(None)
            assert out[4] == r["want"], (N, out[4], r["want"])
            check_outputs(c, ref, out, None, worst, (N, "NULL"))
            ones = dev.run(mask_of("all", r["B"]))
            assert ones[4] == r["want"]
            for a, b in zip(out[:4], ones[:4]):
                assert np.array_equal(bits(a), bits(b)), (N, "all ones differs from NULL")
            for pattern in MASKS:
                act = mask_of(pattern, r["B"])
                got = dev.run(act)
                assert got[4] == r["want"], (N, pattern, got[4])
                check_outputs(c, ref, got, act, worst, (N, pattern))
    print("worst distances:", " ".join("%s %.3g" % kv for kv in sorted(worst.items())))


# ------------------------------------------------------------------------------------- NaN controls under a mask; sixteen step sizes
ONE_PER_KERNEL = [lq102(PIPE4, Ns=(13,)), lq102(PIPE, dyn="F", Ns=(13,)), lq102(DPP, lims=True, Ns=(13,)), row("lq", 6, 3, ROW, lims=True, Ns=(13,)),
                  row("lq", 20, 6, MID, dyn="F", lims=True, Ns=(13,)), row("lq", 47, 3, BIG, lims=True, Ns=(13,)),
                  row("lq", 64, 8, BIG, dyn="F", Ns=(13,)), row("lq", 9, 2, GRP, lims=True, Ns=(13,), FORWARD="group"),
                  pend(7, 3, lims=True, Ns=(13,)), pend(70, 3, Ns=(13,), FORWARD_LANE="1")]


@pytest.mark.parametrize("r", ONE_PER_KERNEL, ids=_id)
def test_nan_controls_of_an_active_rollout_beside_an_inactive_one(handle, monkeypatch, r):
    """a NaN in u and one in k of trajectory 2 (zeroed inside f, forward_pass.jl:21; the pipeline rolls such a rollout out again in
    pipe_redo, which then writes csum instead of the output stage) while trajectory 3 of the same group of four is inactive"""
    for k, v in r["env"].items():
        monkeypatch.setenv(k, v)
    worst = {}
    N = r["Ns"][0]
    c = make_case(r, N, 31337 + ONE_PER_KERNEL.index(r), nan=2)
    ref = reference(c)
    assert not np.any(ref[1][0, N // 2, 2]) and np.isfinite(ref[3].astype(float)).all()
    with OnDevice(handle, c) as dev:
        for inactive in ((3,), (1, 3), ()):
            act = np.ones(r["B"], np.int32)
            act[list(inactive)] = 0
            got = dev.run(act)
            assert got[4] == r["want"], got[4]
            check_outputs(c, ref, got, act, worst, ("nan", inactive))
            assert not got[1][0, N // 2, 2].any()
    print("worst distances:", " ".join("%s %.3g" % kv for kv in sorted(worst.items())))


@pytest.mark.parametrize("r", ONE_PER_KERNEL, ids=_id)
def test_sixteen_step_sizes_with_zero_one_and_repeats(handle, monkeypatch, r):
    """slots with equal α hold the same bits; without limits, with x[:, 0] = x0, α = 0 leaves the first control at ū_0 exactly"""
    for k, v in r["env"].items():
        monkeypatch.setenv(k, v)
    worst = {}
    N = r["Ns"][0]
    r = dict(r, na=16)
    c = make_case(r, N, 4242 + N + r["n"], alpha=A16)
    ref = reference(c)
    with OnDevice(handle, c) as dev:
        act = mask_of("mid", r["B"])
        got = dev.run(act)
        assert got[4] == r["want"], got[4]
        check_outputs(c, ref, got, act, worst, "a16")
    on = act != 0
    for v in np.unique(A16):
        slots = np.flatnonzero(A16 == v)
        for s in slots[1:]:
            for name, a in zip(("xnew", "unew", "cnew", "csum"), got[:4]):
                assert np.array_equal(bits(a[..., on, slots[0]]), bits(a[..., on, s])), (name, "slots", int(slots[0]), int(s), "alpha", v)
    if not r["lims"]:
        for s in np.flatnonzero(A16 == 0.0):
            assert np.array_equal(got[1][:, 0, on, s], c["u"][:, 0, on]), ("alpha = 0: first control", int(s))
    print("worst distances:", " ".join("%s %.3g" % kv for kv in sorted(worst.items())))
