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
from test_forward_reference_cpu import LD, RTOL, clamped_share, lq_reference, make_lq_case, need_longdouble, rollout_dist

pytestmark = pytest.mark.gpu
CSUM_TOL = 1e-12                              # csum against the longdouble sum of the kernel's own cnew (tests/test_gpu_full_size.py)
# what xnew, unew, cnew, csum hold before a call: quiet NaNs with a payload of their own each (the hardware hands a NaN operand's payload
# on, so a csum summed from an untouched cnew would otherwise still look untouched)
SENT = tuple(np.uint64(0x7FF8DEAD5EED1230 + i) for i in range(4))
PIPE4, PIPE, DPP, ROW = "forward_pipe4_kernel", "forward_pipe_kernel", "forward_dpp_kernel", "forward_row_kernel"
MID, BIG, GRP = "forward_mid_kernel", "forward_big_kernel", "forward_pass_kernel"
MASKS = ("none", "first", "last", "alt", "mid")       # beside all active / NULL, which every case runs first
A16 = np.array([1.0, 0.5, 0.0, 0.25, 0.5, 1.0, 0.1, 0.03, 0.0, 0.7, 0.25, 0.01, 0.003, 1.0, 0.001, 0.5])   # 0, 1 and repeated values


def row(fam, n, m, want, B=7, na=3, dyn="", pol=True, lims=False, full=True, mis=(), Ns=(5,), **env):
    """fam: "lq" | "pend"; dyn: "" shared LTI, "F" shared LTV, "f" / "Ff" per trajectory; full: full Q and R with cost_diag = 0, else
    diagonal ones with cost_diag = 1; mis: the operands placed 8 bytes into their allocation (of K k u x A B); Ns: the horizons the
    call is made at; env: DDP_* switches by their name without the prefix"""
    return dict(fam=fam, n=n, m=m, want=want, B=B, na=na, dyn=dyn, pol=pol, lims=lims, full=full, mis=tuple(mis), Ns=tuple(Ns),
                env={("DDP_" + k): v for k, v in env.items()})


def lq102(want, **kw):                        # the (10, 2) call the pipeline takes unless a row says otherwise
    kw.setdefault("full", False)
    return row("lq", 10, 2, want, **kw)


def pend(B, na, **kw):
    kw.setdefault("Ns", (15, 16, 17))
    kw.setdefault("full", False)
    return row("pend", 4, 1, kw.pop("want", DPP), B=B, na=na, **kw)


S63, S15, SP = (63, 64, 65), (15, 16, 17), (7, 8, 9, 11, 12, 13)
TABLE = [
    # (10, 2), policy, no limits, diagonal cost, aligned operands: the pipeline up to 1 024 rollouts (forward_pass_pipe.hip, total > 1024)
    lq102(PIPE4, Ns=(1, 2, 3) + SP), lq102(PIPE4, B=64, na=16, Ns=(12, 13)), lq102(DPP, B=205, na=5, Ns=(12, 13)),
    lq102(PIPE4, B=1024, na=1, Ns=(9,)), lq102(DPP, B=1025, na=1, Ns=(9,)),
    lq102(PIPE, dyn="F", Ns=(1, 2, 3) + SP), lq102(PIPE, dyn="Ff", Ns=SP), lq102(PIPE, dyn="f", Ns=SP),
    lq102(PIPE, dyn="F", B=64, na=16, Ns=(8, 9)), lq102(DPP, dyn="F", B=205, na=5, Ns=(8, 9)), lq102(DPP, dyn="Ff", B=205, na=5, Ns=(8,)),
    # ... and each single reason for which it declines
    lq102(DPP, pol=False, Ns=(1, 2, 3, 16)), lq102(DPP, lims=True, Ns=(1, 2, 3, 16)), lq102(DPP, full=True, Ns=S63), lq102(DPP, FORWARD_PIPE="0"),
    lq102(DPP, FORWARD_FUSE="0", Ns=S63), lq102(DPP, mis="K"), lq102(DPP, mis="k"), lq102(DPP, mis="u"), lq102(DPP, mis="x"),
    lq102(DPP, dyn="F", mis="A"), lq102(DPP, dyn="F", mis="B"), lq102(DPP, dyn="Ff", lims=True, full=True, Ns=(2, 17)),
    lq102(PIPE4, mis="AB", Ns=(9,)),            # (time-invariant dynamics are not fetched in 16-byte pieces: no reason to decline)
    lq102(PIPE4, B=128, na=16, Ns=(12,), FORWARD_PIPE="1"), lq102(PIPE, Ns=SP, FORWARD_PIPE="2"), lq102(PIPE, B=128, na=16, dyn="F", Ns=(8,), FORWARD_PIPE="1"),
    # the variants of the 16-lane-row kernel (launch_dpp: FAST, al16)
    lq102(DPP, FORWARD_FAST="0", FORWARD_PIPE="0"), lq102(DPP, lims=True, FORWARD_FAST="0"), lq102(DPP, mis="uk", lims=True), lq102(DPP, mis="Kkux", Ns=(3, 16)),
    lq102(DPP, dyn="f", pol=False, lims=True, full=True),
    # LQ shapes a padded 16-lane row holds (forward_pass_row.hip, ddp_launch_forward_row)
    row("lq", 1, 1, ROW, Ns=(1, 2, 3) + S63), row("lq", 4, 1, ROW, dyn="F", Ns=S63), row("lq", 6, 3, ROW, lims=True, Ns=S63),
    row("lq", 12, 4, ROW, dyn="Ff", lims=True, Ns=S63), row("lq", 13, 2, ROW, pol=False, Ns=S63), row("lq", 14, 1, ROW, dyn="f", Ns=S63),
    row("lq", 14, 2, ROW, dyn="F", lims=True, Ns=S63), row("lq", 8, 2, ROW, pol=False, lims=True, Ns=(1, 64)), row("lq", 9, 2, ROW, mis="Kkux", Ns=(3, 33)),
    # what no row holds, up to n = 32: one wave per rollout (forward_pass_big.hip, forward_mid_kernel)
    row("lq", 13, 3, MID, Ns=(1, 2, 3) + S63), row("lq", 14, 4, MID, lims=True, Ns=S63), row("lq", 15, 1, MID, dyn="F", Ns=S63),
    row("lq", 16, 8, MID, dyn="Ff", lims=True, Ns=S63), row("lq", 17, 1, MID, pol=False, Ns=S63), row("lq", 24, 4, MID, dyn="f", Ns=S63),
    row("lq", 25, 8, MID, lims=True, Ns=S63), row("lq", 32, 8, MID, dyn="F", Ns=S63), row("lq", 3, 5, MID, lims=True, Ns=S63),
    row("lq", 24, 4, MID, mis="KkuxAB", dyn="F", Ns=(4, 33)),
    *[row("lq", n, m, BIG, Ns=(1, 2, 3, 64) if n == 13 else (64, 65), FORWARD_MID="0", **kw) for n, m, kw in (
        (13, 3, {}), (14, 4, dict(lims=True)), (15, 1, dict(dyn="F")), (16, 8, dict(dyn="Ff", lims=True)), (17, 1, dict(pol=False)),
        (24, 4, dict(dyn="f")), (25, 8, dict(lims=True)), (32, 8, dict(dyn="F")), (3, 5, dict(lims=True)))],
    # 32 < n <= 64: forward_big_kernel with cost_mid_kernel<48> / <64>; full Q and R reach the last rows and columns of the padding
    row("lq", 33, 1, BIG, Ns=(1, 2, 3) + S63), row("lq", 40, 5, BIG, dyn="F", lims=True, Ns=S63), row("lq", 47, 8, BIG, dyn="Ff", Ns=S63),
    row("lq", 48, 6, BIG, lims=True, Ns=S63), row("lq", 49, 1, BIG, dyn="f", Ns=S63), row("lq", 63, 8, BIG, dyn="F", lims=True, Ns=S63),
    row("lq", 64, 1, BIG, pol=False, lims=True, Ns=S63), row("lq", 64, 7, BIG, dyn="Ff", lims=True, Ns=S63),
    row("lq", 48, 8, BIG, pol=False, Ns=(1, 64)), row("lq", 64, 8, BIG, dyn="F", lims=True, Ns=(1, 2, 3) + S63, FORWARD64="0"),
    row("lq", 48, 6, BIG, lims=True, Ns=(64, 65), FORWARD_MID="0"), row("lq", 40, 5, BIG, mis="KkuxAB", dyn="F", Ns=(4, 33)),
    # (64, 8): forward_big64_kernel (1, 2 or 4 step sizes of a trajectory per wave) reports the family's name
    *[row("lq", 64, 8, BIG, B=5, na=na, pol=pol, lims=(na % 2 == 1), dyn=("F" if na in (2, 5) else ""), Ns=((1, 2, 3) if na == 3 else ()) + S15)
      for na in (1, 2, 3, 5, 16) for pol in (True, False)],
    # DDP_FORWARD=group: the run-time-sized group-of-lanes kernel, the five instantiations of launch_fp
    row("lq", 10, 2, GRP, Ns=(1, 2, 3, 16), FORWARD="group"), row("lq", 4, 1, GRP, dyn="F", lims=True, FORWARD="group"),
    row("lq", 6, 3, GRP, dyn="Ff", FORWARD="group"), row("lq", 9, 2, GRP, pol=False, lims=True, FORWARD="group"),
    row("lq", 16, 3, GRP, dyn="f", lims=True, FORWARD="group"), row("lq", 17, 3, GRP, dyn="F", FORWARD="group"),
    row("lq", 32, 8, GRP, lims=True, Ns=(9,), FORWARD="group"), row("lq", 10, 2, GRP, full=False, mis="Kkux", FORWARD="group"),
    # DDP_FORWARD=b: the large-state launcher first
    row("lq", 10, 2, MID, Ns=(3, 64), FORWARD="b"), row("lq", 20, 3, MID, lims=True, dyn="F", Ns=(64,), FORWARD="b"),
    # pendcart (forward_pass_dpp.hip): element-wise / chunked streams at 3 584 rollouts, the lane kernel from 12 288
    pend(7, 3, Ns=(1, 2, 3) + S15), pend(7, 3, pol=False, lims=True, Ns=(1, 2, 3) + S15), pend(5, 2, lims=True, full=True),
    pend(3583, 1, Ns=(16, 17)), pend(512, 7, Ns=(16, 17)), pend(3583, 1, pol=False, lims=True, Ns=(17,)), pend(224, 16, lims=True, Ns=(15, 24)),
    pend(1117, 11, Ns=(17,)), pend(768, 16, Ns=(16, 17)), pend(1117, 11, lims=True, pol=False, Ns=(24,)), pend(768, 16, lims=True, Ns=(15,)),
    pend(12288, 1, pol=False, Ns=(3,)),
    pend(7, 3, lims=True, FORWARD_LANE="1"), pend(70, 3, pol=False, Ns=(1, 2, 3, 17), FORWARD_LANE="1"), pend(768, 16, Ns=(17,), FORWARD_LANE="0"),
    pend(7, 3, lims=True, PEND_CHUNK="1"), pend(512, 7, Ns=(17,), PEND_CHUNK="0"), pend(7, 3, lims=True, FORWARD_PEND="0"),
    pend(7, 3, pol=False, FORWARD_PEND="0", FORWARD_FUSE="0"), pend(7, 3, lims=True, FORWARD_FUSE="0"), pend(70, 3, FORWARD_FUSE="0", FORWARD_LANE="1"),
    pend(7, 3, lims=True, want=GRP, Ns=(1, 2, 3, 16), FORWARD="group"), pend(7, 3, pol=False, want=GRP, FORWARD="group"),
]


def _id(r):
    return "%s_n%d_m%d_B%dx%d_%s_%s%s%s%s_%s" % (r["fam"], r["n"], r["m"], r["B"], r["na"], r["dyn"] or "lti", "pol" if r["pol"] else "open",
                                                "_lims" if r["lims"] else "", "_full" if r["full"] else "_diag",
                                                ("_mis" + "".join(r["mis"])) if r["mis"] else "",
                                                "_".join("%s=%s" % (k[4:], v) for k, v in sorted(r["env"].items())) or "default")


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
