"""Wide controls on the GPU: 8 < m <= 32 with any n <= 64 (csrc/back_pass_wide.hip, csrc/forward_pass_wide.hip and the device-resident
drivers on top of them) against the C oracle, 1e-8 relative per time step (conftest.relerr), every trajectory of every call.  The cases
come from tests/wide_controls_cases.py; tests/test_wide_controls_cpu.py shows without a GPU that the oracle and the NumPy restatement
agree on them at 1e-11."""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import par_map, relerr
from test_forward_reference_cpu import LD, lq_oracle_problem, make_lq_case, oracle_rollout
from test_gpu_forward_contract import MASKS, OnDevice, bits, check_outputs, mask_of
from test_gpu_forward_contract import handle  # noqa: F401  (fixture: the default handle with every DDP_* switch cleared)
from wide_controls_cases import LAYOUTS, SHAPES, SOLVES, bp_case, bp_operands, clamped_share, outcome, reference_outcomes_nearby, solve_batch, solve_case

pytestmark = pytest.mark.gpu
RTOL = 1e-8
WIDE, FWIDE = "back_pass_wide_kernel", "forward_wide_kernel"
OUT_SENT = tuple(np.uint64(0x7FF8BEEF5EED4560 + i) for i in range(7))      # K k Quu Vx Vxx dV diverge before a call: NaNs with own payloads


@pytest.fixture(scope="module")
def ddp():
    import ddp_amd
    ddp_amd.default_handle()
    return ddp_amd


# ------------------------------------------------------------------------------------------------ the backward pass, device entry
class BPOnDevice:
    """a backward-pass case on the device; run(regType, active) pre-fills the seven outputs with sentinels, calls
    ddp_back_pass_f64_dev and returns dict(K, k, Quu, Vx, Vxx, dV, diverge (int32), raw (the uint64 images), kernel)"""
    NAMES = ("K", "k", "Quu", "Vx", "Vxx", "dV", "diverge")

    def __init__(self, h, c):
        from ddp_amd import _lib
        self.h, self.c, self.L, self.bufs = h, c, _lib.lib(), []
        n, m, N, B = c["n"], c["m"], c["N"], c["B"]
        self.shapes = ((m, n, N, B), (m, N, B), (m, m, N, B), (n, N, B), (n, n, N, B), (2, B), ((B + 1) // 2,))     # diverge: int32[B] in 8-byte words
        try:
            self.dev = {k: self.put(c[k]) for k in ("cx", "cu", "cxx", "cxu", "cuu", "fx", "fu", "lam", "lims", "u")}
            self.outs = [self.alloc(8 * int(np.prod(s))) for s in self.shapes]
            self.act = self.alloc(4 * B)
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

    def put(self, a):
        if a is None:
            return None
        a = np.asfortranarray(a, dtype=np.float64)
        p = self.alloc(a.nbytes)
        self.copy_in(p, a)
        return p

    def run(self, regType=1, active=None):
        from ddp_amd import _lib
        c, d = self.c, self.dev
        lay = c["layout"]
        for p, s, v in zip(self.outs, self.shapes, OUT_SENT):
            self.copy_in(p, np.full(int(np.prod(s)), v, np.uint64))
        if active is not None:
            self.copy_in(self.act, np.ascontiguousarray(active, np.int32))
        desc = _lib.BPDesc(c["n"], c["m"], c["N"], c["B"], int("F" in lay), int("f" in lay), int("C" in lay), int("c" in lay), int(regType),
                           int(c["lims"] is not None))
        args = [d[k] for k in ("cx", "cu", "cxx", "cxu", "cuu", "fx", "fu", "lam")] + [d["lims"], d["u"] if c["lims"] is not None else None,
                                                                                       None if active is None else self.act] + self.outs
        _lib.check(self.L.ddp_back_pass_f64_dev(self.h.raw, C.byref(desc), *[C.c_void_p(a) for a in args]))
        self.h.sync()
        out = {}
        raw = {}
        for name, p, s in zip(self.NAMES, self.outs, self.shapes):
            a = self.h.to_host(C.c_void_p(p), s)
            raw[name] = bits(a)
            out[name] = a
        out["diverge"] = np.ascontiguousarray(out["diverge"]).view(np.int32)[: c["B"]].copy()
        out["raw"] = raw
        out["kernel"] = self.h.last_kernel(0)
        return out

    def close(self):
        for p in self.bufs:
            self.h.free(p)
        self.bufs = []

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def oracle_bp(c, regType, trajectories=None):
    """the C oracle's back_pass of every (listed) trajectory: {b: (diverge, K, k, Quu, Vx, Vxx, dV)}"""
    from oracle import oracle_ctypes as oc

    def one(b):
        cx, cu, cxx, cxu, cuu, fx, fu, lam = bp_operands(c, b)
        d, (K, k, Quu), vx, vxx, dv = oc.back_pass(cx, cu, cxx, cxu, cuu, fx, fu, lam, regType, c["lims"], None, c["u"][..., b])
        return b, (d, K, k, Quu, vx, vxx, dv)
    bs = list(range(c["B"])) if trajectories is None else list(trajectories)
    return dict(par_map(one, bs, workers=min(16, len(os.sched_getaffinity(0)))))


def traj_dist(out, ref, b):
    d, K, k, Quu, vx, vxx, dv = ref
    return {name: relerr(got[..., b], want) for name, got, want in (("K", out["K"], K), ("k", out["k"], k), ("Quu", out["Quu"], Quu),
                                                                    ("Vx", out["Vx"], vx), ("Vxx", out["Vxx"], vxx), ("dV", out["dV"], dv))}


def oracle_step_on_gpu_state(c, out, b, i, regType):
    """The reference's own step i on the GPU's Vx_{i+1}, Vxx_{i+1} and warm start ("Control limits and the reference's
    box-QP ties"): Q-terms as backward_pass.jl:240-247, then the oracle's boxQP and the gains of :58-61.  Returns (K_i, k_i)."""
    from oracle import oracle_ctypes as oc
    cx, cu, cxx, cxu, cuu, fx, fu, lam = bp_operands(c, b)
    n, m, N = c["n"], c["m"], c["N"]
    at = lambda a, nd: a[..., i] if a.ndim == nd + 1 else a
    fxi, fui, cxui, cuui = at(fx, 2), at(fu, 2), at(cxu, 2), at(cuu, 2)
    V, v = out["Vxx"][:, :, i + 1, b], out["Vx"][:, i + 1, b]
    Vr = V + (lam * np.eye(n) if regType == 2 else 0)
    Qu = cu[:, i] + fui.T @ v
    Quxr = cxui.T + (fui.T @ Vr) @ fxi
    QuuF = cuui + (fui.T @ Vr) @ fui + (lam * np.eye(m) if regType == 1 else 0)
    u = c["u"][:, i, b]
    x0 = out["k"][:, min(i + 1, N - 2), b] if i + 1 <= N - 2 else np.zeros(m)
    ki, res, Hfree, free, _ = oc.boxqp(QuuF, Qu, c["lims"][:, 0] - u, c["lims"][:, 1] - u, x0)
    Ki = np.zeros((m, n))
    if res >= 1 and free.any():
        import scipy.linalg as sla
        Ki[free] = -sla.cho_solve((Hfree, False), Quxr[free])
    return Ki, ki, res


def check_bp(c, out, ref, regType, what, worst, on=None):
    """every active trajectory against the oracle; a trajectory that parts from it under limits must be a box-QP tie of the reference
    (at most 1 % of the batch): up to the parting step both agree, and the reference's own step on the GPU's state gives the GPU's"""
    parted = []
    for b in range(c["B"]):
        if on is not None and not on[b]:
            continue
        assert out["diverge"][b] == ref[b][0] == 0, (what, b, out["diverge"][b], ref[b][0])
        dist = traj_dist(out, ref[b], b)
        for name, v in dist.items():
            worst[name] = max(worst.get(name, 0.0), v) if v < RTOL else worst.get(name, 0.0)
        if all(v < RTOL for v in dist.values()):
            continue
        assert c["lims"] is not None and c["lims"][0, 0] <= c["lims"][0, 1], (what, b, dist)
        N = c["N"]
        e = np.array([relerr(out["K"][:, :, i, b], ref[b][1][:, :, i]) + relerr(out["k"][:, i, b], ref[b][2][:, i]) for i in range(N)])
        i = int(np.max(np.flatnonzero(e > RTOL)))                 # the first step (backward in time) at which the gains part
        assert relerr(out["Vxx"][:, :, i + 1:, b], ref[b][5][:, :, i + 1:]) < RTOL and relerr(out["Vx"][:, i + 1:, b], ref[b][4][:, i + 1:]) < RTOL
        Ki, ki, res = oracle_step_on_gpu_state(c, out, b, i, regType)
        assert res >= 1 and relerr(out["K"][:, :, i, b], Ki) < RTOL and relerr(out["k"][:, i, b], ki) < RTOL, (what, b, i, "not a tie of the reference")
        parted.append(b)
    assert len(parted) <= 0.01 * c["B"], (what, "trajectories parted at a box-QP tie", parted)
    return parted


# 1. ------------------------------------------------------------------------------------------- no limits / inverted limits
# horizons: the kernel has no chunk length (cx, cu, u are read per step); 1, 2 and 3 are its edge cases, the others ordinary
@pytest.mark.parametrize("n,m", SHAPES)
def test_back_pass_without_limits(handle, n, m):
    worst = {}
    big = n * m >= 1024
    for li, layout in enumerate(LAYOUTS):
        for regType, off in ((1, False), (2, False), (1, True)):
            for N, B in (((3, 2), (17, 3)) if big else ((1, 2), (2, 3), (3, 1), (9, 5), (33, 2))):
                c = bp_case(31 * n + m + 7 * li + N, n, m, N, B, layout, None, lims_off=off)
                with BPOnDevice(handle, c) as dev:
                    out = dev.run(regType)
                assert out["kernel"] == WIDE
                assert np.array_equal(out["Vxx"], np.transpose(out["Vxx"], (1, 0, 2, 3)))
                if N >= 2:
                    check_bp(c, out, oracle_bp(c, regType), regType, (layout, regType, off, N, B), worst)
                else:                                              # N = 1: the terminal step alone (backward_pass.jl:234-236)
                    for b in range(B):
                        cxb, cub, cxxb, cxub, cuub = bp_operands(c, b)[:5]
                        assert np.array_equal(out["Vxx"][:, :, 0, b], cxxb.reshape(n, n, -1)[:, :, -1]) and np.array_equal(out["Vx"][:, 0, b], cxb[:, 0])
                        assert np.array_equal(out["Quu"][:, :, 0, b], cuub.reshape(m, m, -1)[:, :, -1])
                    assert not out["diverge"].any() and not out["dV"].any() and not out["K"].any() and not out["k"].any()
    print("worst distances:", " ".join("%s %.3g" % kv for kv in sorted(worst.items())))


def test_back_pass_more_than_one_round_of_work_groups(handle):
    """B = 600 work-groups on 256 compute units at (12, 12), and 300 at (64, 32) where one work-group fills a unit's LDS"""
    worst = {}
    for n, m, N, B, layout in ((12, 12, 12, 600, "FCfc"), (64, 32, 6, 300, "F")):
        c = bp_case(5 + n, n, m, N, B, layout)
        with BPOnDevice(handle, c) as dev:
            out = dev.run(1)
        assert out["kernel"] == WIDE
        check_bp(c, out, oracle_bp(c, 1), 1, (n, m, B), worst)
    print("worst distances:", " ".join("%s %.3g" % kv for kv in sorted(worst.items())))


# 2. ------------------------------------------------------------------------------------------------------------- with limits
@pytest.mark.parametrize("n,m", SHAPES)
def test_back_pass_with_limits(handle, n, m):
    worst, shares, parted = {}, [], 0
    big = n * m >= 1024
    for li, (layout, lim, regType) in enumerate((("", 0.5, 1), ("F", 0.25, 2), ("FC", 0.25, 1), ("FCfc", 0.5, 2), ("FCfc", 0.25, 1))):
        N, B = (40, 3) if big else (40, 6)
        c = bp_case(977 * n + m + li, n, m, N, B, layout, lim)
        ref = oracle_bp(c, regType)
        share = float(np.mean([clamped_share(ref[b][2][:, :-1], c["u"][:, :-1, b], c["lims"]) for b in range(B)]))
        shares.append(share)
        assert share >= 0.2, (layout, lim, share)
        with BPOnDevice(handle, c) as dev:
            out = dev.run(regType)
        assert out["kernel"] == WIDE
        gone = check_bp(c, out, ref, regType, (layout, lim, regType), worst)
        parted += len(gone)
        for b in set(range(B)) - set(gone):                        # rows of K of the reference's clamped coordinates are exactly zero
            zero_rows = ~ref[b][1].any(axis=1)                     # [m, N]
            assert not np.moveaxis(out["K"][..., b], 1, 2)[zero_rows].any(), (layout, b)
    print("clamped share %.0f %% .. %.0f %%; parted %d; worst distances:" % (100 * min(shares), 100 * max(shares), parted),
          " ".join("%s %.3g" % kv for kv in sorted(worst.items())))


# 3. -------------------------------------------------------------------------------------------------------------- divergence
@pytest.mark.parametrize("n,m,lim", [(12, 12, None), (24, 16, 0.5), (64, 32, None), (10, 24, 0.25)])
def test_back_pass_divergence(handle, n, m, lim):
    """an indefinite cuu at one step of trajectories 1 and 3: diverge is the oracle's index, everything earlier in time is zero, the
    neighbours are what they are without the defect.  With limits the failure is the box-QP's result < 1."""
    N, B, step = 10, 5, 4
    c = bp_case(404 + n, n, m, N, B, "FCfc", lim)
    clean = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in c.items()}
    for b in (1, 3):
        c["cuu"][:, :, step, b] = -np.eye(m)
    ref = oracle_bp(c, 1)
    with BPOnDevice(handle, c) as dev:
        out = dev.run(1)
    with BPOnDevice(handle, clean) as dev:
        good = dev.run(1)
    assert out["kernel"] == WIDE
    assert [int(ref[b][0]) for b in range(B)] == [0, step + 1, 0, step + 1, 0]
    assert out["diverge"].tolist() == [0, step + 1, 0, step + 1, 0]
    for b in (1, 3):
        for name in ("K", "k", "Vx", "Vxx"):
            assert not out[name][..., : step + 1, b].any(), (name, b)
        assert not out["Quu"][..., :step, b].any()
        d = traj_dist(out, ref[b], b)
        assert all(v < RTOL for v in d.values()), (b, d)
    for b in (0, 2, 4):
        for name in ("K", "k", "Quu", "Vx", "Vxx", "dV"):
            assert np.array_equal(out["raw"][name].reshape(out[name].shape)[..., b], good["raw"][name].reshape(good[name].shape)[..., b]), (name, b)
        d = traj_dist(out, ref[b], b)
        assert all(v < RTOL for v in d.values()), (b, d)


# 4. ------------------------------------------------------------------------------------------------------------- active mask
@pytest.mark.parametrize("n,m,lim", [(12, 12, 0.5), (33, 9, None), (64, 32, 0.25)])
def test_back_pass_active_mask(handle, n, m, lim):
    """inactive trajectories keep the sentinel bits of all seven outputs; active ones are the bits of the unmasked call"""
    N, B = 8, 7
    c = bp_case(55 + n, n, m, N, B, "FCfc", lim)
    with BPOnDevice(handle, c) as dev:
        full = dev.run(1)
        ones = dev.run(1, mask_of("all", B))
        for name in BPOnDevice.NAMES:
            assert np.array_equal(full["raw"][name], ones["raw"][name]), name
        for pattern in MASKS:
            act = mask_of(pattern, B)
            got = dev.run(1, act)
            assert got["kernel"] == WIDE
            for i, name in enumerate(BPOnDevice.NAMES[:6]):
                a, f = got["raw"][name].reshape(got[name].shape), full["raw"][name].reshape(full[name].shape)
                assert np.all(a[..., act == 0] == OUT_SENT[i]), (pattern, name, "of an inactive trajectory was written")
                assert np.array_equal(a[..., act != 0], f[..., act != 0]), (pattern, name)
            dv = got["raw"]["diverge"].view(np.int32)[:B]
            sent = np.full(1, OUT_SENT[6], np.uint64).view(np.int32)[np.arange(B) % 2]      # the two halves of the sentinel word
            assert np.array_equal(dv[act == 0], sent[act == 0]) and not dv[act != 0].any(), pattern


# 5. -------------------------------------------------------------------------------------- the same arithmetic as the families
@pytest.mark.parametrize("n,m,lim", [(10, 2, None), (12, 3, 0.5), (32, 8, None), (64, 8, None)])
def test_forced_wide_kernel_on_narrow_shapes(handle, monkeypatch, n, m, lim):
    """DDP_BACKPASS=c on shapes the other families hold: the wide kernel agrees with the oracle as the default kernel does"""
    worst = {}
    N, B = 20, 4
    for layout, regType in (("", 1), ("FCfc", 2)):
        c = bp_case(88 + n + m, n, m, N, B, layout, lim)
        ref = oracle_bp(c, regType)
        with BPOnDevice(handle, c) as dev:
            default = dev.run(regType)
            monkeypatch.setenv("DDP_BACKPASS", "c")
            forced = dev.run(regType)
            monkeypatch.delenv("DDP_BACKPASS")
        assert default["kernel"] != WIDE and forced["kernel"] == WIDE, (default["kernel"], forced["kernel"])
        check_bp(c, default, ref, regType, ("default", layout), {})
        check_bp(c, forced, ref, regType, ("forced", layout), worst)
    print("worst distances:", " ".join("%s %.3g" % kv for kv in sorted(worst.items())))


# 6. ------------------------------------------------------------------------------------------------------------------ rollout
def oracle_reference(c):
    """xnew, unew, cnew of every rollout by oracle_ctypes.forward_pass, and the longdouble sum of its cnew"""
    N, B, na = c["N"], c["B"], len(c["alpha"])
    xs, us, cn = np.empty((c["n"], N, B, na)), np.empty((c["m"], N, B, na)), np.empty((N, B, na))

    def one(b):
        po = lq_oracle_problem(c, b)
        for ai in range(na):
            xs[:, :, b, ai], us[:, :, b, ai], cn[:, b, ai] = oracle_rollout(po, c, b, ai)
    par_map(one, range(B), workers=min(16, len(os.sched_getaffinity(0))))
    return xs.astype(LD), us.astype(LD), cn.astype(LD), cn.astype(LD).sum(axis=0)


ROLLOUTS = [(12, 12, "", True, True), (12, 12, "F", False, True), (24, 16, "Ff", True, True), (24, 16, "f", True, False),
            (32, 32, "F", True, True), (32, 32, "", False, False), (48, 12, "Ff", True, True), (48, 12, "", True, False),
            (64, 32, "F", True, True), (64, 32, "f", False, True), (64, 32, "Ff", True, False), (6, 9, "", True, True)]


@pytest.mark.parametrize("n,m,dyn,pol,lims", ROLLOUTS, ids=lambda v: str(v))
def test_rollout(handle, n, m, dyn, pol, lims):
    """11 step sizes, every mask pattern, against oracle_ctypes.forward_pass per time step; csum against the sum of cnew at 1e-12
    (tests/test_gpu_forward_contract.py, check_outputs)"""
    worst = {}
    al = 10.0 ** np.linspace(0, -3, 11)
    for N in (1, 2, 23):
        B = 5
        c = make_lq_case(4000 + 64 * n + m + N, n, m, N, B, al, dyn, pol, lims, True)
        ref = oracle_reference(c)
        with OnDevice(handle, c) as dev:
            out = dev.run(None)
            assert out[4] == FWIDE, out[4]
            check_outputs(c, ref, out, None, worst, (N, "NULL"))
            ones = dev.run(mask_of("all", B))
            for a, b in zip(out[:4], ones[:4]):
                assert np.array_equal(bits(a), bits(b))
            for pattern in MASKS:
                act = mask_of(pattern, B)
                got = dev.run(act)
                assert got[4] == FWIDE
                check_outputs(c, ref, got, act, worst, (N, pattern))
    print("worst distances:", " ".join("%s %.3g" % kv for kv in sorted(worst.items())))


def test_rollout_sixteen_step_sizes(handle):
    from test_gpu_forward_contract import A16
    worst = {}
    c = make_lq_case(99, 24, 16, 13, 7, A16, "F", True, True, True)
    with OnDevice(handle, c) as dev:
        act = mask_of("mid", 7)
        got = dev.run(act)
        assert got[4] == FWIDE
        check_outputs(c, oracle_reference(c), got, act, worst, "a16")


@pytest.mark.parametrize("n,m,dyn,pol,lims", [r for r in ROLLOUTS if r[0] >= 12], ids=lambda v: str(v))
def test_rollout_at_eight_controls_keeps_its_kernel(handle, n, m, dyn, pol, lims):
    """the calls of test_rollout with m = 8: the kernel names of tests/test_gpu_forward_contract.py's table"""
    c = make_lq_case(7 + n, n, 8, 9, 5, 10.0 ** np.linspace(0, -3, 11), dyn, pol, lims, True)
    with OnDevice(handle, c) as dev:
        out = dev.run(None)
    assert out[4] == ("forward_mid_kernel" if n <= 32 else "forward_big_kernel"), out[4]


def test_rollout_with_wrapped_coordinates(ddp):
    """diff_wrap at n <= 32 with wide controls against the oracle; refused above n = 32 as for every other shape"""
    from oracle import oracle_ctypes as oc
    rng = np.random.default_rng(3)
    n, m, N, B = 12, 12, 15, 3
    c = make_lq_case(31, n, m, N, B, np.array([1.0, 0.3]), "", True, True, True)
    c["x"][0] += 2 * np.pi * rng.integers(-2, 3, (N, B))
    c["x"][5] += 2 * np.pi * rng.integers(-2, 3, (N, B))
    diff = ddp.WrappedDiff(0, 5)
    prob = ddp.LQProblem(c["A"], c["Bm"], c["Q"], c["R"])
    xn, un, cn = ddp.forward_pass(ddp.GaussianPolicy(N, n, m, c["K"], c["k"]), c["x0"], c["u"], c["x"], c["alpha"], prob, c["lims"], diff)
    from ddp_amd import _lib
    assert _lib.default_handle().last_kernel(1) == FWIDE
    for b in range(B):
        po = oc.make_problem("lq", n, m, N, A=c["A"], B=c["Bm"], Q=c["Q"], R=c["R"], diff_wrap=diff.mask)
        for j, a in enumerate(c["alpha"]):
            xr, ur, cr = oc.forward_pass(po, (c["K"][..., b], c["k"][..., b]), c["x0"][:, b], c["u"][..., b], c["x"][..., b], float(a), c["lims"])
            assert relerr(xn[..., b, j], xr) < RTOL and relerr(un[..., b, j], ur) < RTOL and relerr(cn[..., b, j], cr) < RTOL
    c = make_lq_case(32, 40, 12, 5, 2, np.array([1.0]), "", True, False, True)
    with pytest.raises(ddp.DDPError):
        ddp.forward_pass(ddp.GaussianPolicy(5, 40, 12, c["K"], c["k"]), c["x0"], c["u"], c["x"], c["alpha"],
                         ddp.LQProblem(c["A"], c["Bm"], c["Q"], c["R"]), None, ddp.WrappedDiff(0))


# 7. ------------------------------------------------------------------------------------------------------------- whole solves
def _check_solve(res, b, ref, what):
    x, u, pol, Vx, Vxx, cost, tr = res
    xr, ur, (Kr, kr, Quur), vxr, vxxr, cr, info = ref
    st = tr["stats"][:, b]
    assert (int(st[0]), int(st[1]), int(st[3])) == outcome(info), (what, b, st[:5], info)
    rows = info["iter"] - 1
    for key, okey in (("cost", "cost"), ("λ", "lam"), ("α", "alpha")):
        got, want = tr["history"][key][:rows, b], info["trace"][okey][:rows]
        assert np.allclose(got, want, rtol=RTOL, atol=0, equal_nan=True), (what, b, key)
    for name, got, want in (("x", x[..., b], xr), ("u", u[..., b], ur), ("Vxx", Vxx[..., b], vxxr), ("Vx", Vx[..., b], vxr), ("K", pol.K[..., b], Kr)):
        assert relerr(got, want) < RTOL, (what, b, name, relerr(got, want))
    assert abs(cost[:, b].sum() - cr.sum()) < 1e-9 * abs(cr.sum()), (what, b)


@pytest.mark.parametrize("n,m,T,lim", SOLVES)
def test_whole_solves(ddp, n, m, T, lim):
    """the solve of the table and a batch of 64 perturbed copies (x0, u0 per trajectory) against the C oracle's ilqg: status, iteration
    and back-pass counts, the trace rows, x, u, Vx, Vxx, K, cost.

    The solve of the table (trajectory 0) must agree outright.  A perturbed copy whose counts differ from the oracle's is accepted
    only where the reference contradicts ITSELF: the oracle, on inputs 1e-13 (relative) away, must give other counts than on the
    inputs themselves (reference_outcomes_nearby), and the GPU's solve must then agree in every respect, at RTOL, with one of those
    solves of the oracle.  Where the oracle's nearby solves all agree with its own, the GPU has to as well.  First seen at
    (12, 12, 80, ±0.6), trajectory 28: the oracle ends by gradient after 9 iterations on the inputs and by tolerance after 8 on 36 of
    39 inputs 1e-13 away; the GPU ends by tolerance after 8."""
    from oracle import oracle_ctypes as oc
    from ddp_amd import _lib
    P = solve_case(n, m, T, lim)
    B = 64
    x0, u0 = solve_batch(P, B)
    prob = ddp.LQProblem(P["A"], P["B"], P["Q"], P["R"])
    res = ddp.iLQG(prob, x0, u0, lims=P["lims"], max_iter=50, timing=False)
    assert _lib.default_handle().last_kernel(0) == WIDE and _lib.default_handle().last_kernel(1) == FWIDE
    p = oc.make_problem("lq", n, m, T, A=P["A"], B=P["B"], Q=P["Q"], R=P["R"])
    refs = par_map(lambda b: oc.ilqg(p, x0[:, b], u0[..., b], lims=P["lims"], max_iter=50), range(B), workers=min(16, len(os.sched_getaffinity(0))))
    assert refs[0][6]["status"] in (1, 2)
    ties = []
    for b in range(B):
        st = res[6]["stats"][:, b]
        got = (int(st[0]), int(st[1]), int(st[3]))
        if got == outcome(refs[b][6]) or b == 0:
            _check_solve(res, b, refs[b], (n, m, T, lim))
            continue
        near = reference_outcomes_nearby(p, x0[:, b], u0[..., b], P["lims"], 1000 * b + n)
        sides = sorted({outcome(r[6]) for r in near} | {outcome(refs[b][6])})
        assert len(sides) > 1, ((n, m, T, lim), b, "the reference is stable here", sides, "GPU", got)
        match = [r for r in near if outcome(r[6]) == got]
        assert match, ((n, m, T, lim), b, "the GPU's counts are on no side of the reference's tie", sides, "GPU", got)
        _check_solve(res, b, match[0], (n, m, T, lim, "tie"))
        ties.append((b, got, sides))
    print("trajectories at a tie of the reference:", ties)
    if lim is not None:
        on = np.mean((res[1] == -lim) | (res[1] == lim))
        assert 0.05 < on < 0.6, on


def _same(a, b):
    return np.array_equal(a, b, equal_nan=True)


def test_queue_equals_standalone_batches_bit_for_bit(ddp):
    """64 problems at (12, 12) with limits through 16 slots: the bits of iLQG on the batches of 16"""
    n, m, T, lim = SOLVES[1]
    P = solve_case(n, m, T, lim)
    rng = np.random.default_rng(21)
    Pn, S = 64, 16
    x0 = P["x0"][:, None] + 0.1 * rng.standard_normal((n, Pn))
    u0 = P["u0"][:, :, None] * (1 + np.arange(Pn) % 5)[None, None, :] / 3 + 0.05 * rng.standard_normal((m, T, Pn))
    prob = ddp.LQProblem(P["A"], P["B"], P["Q"], P["R"])
    kw = dict(lims=P["lims"], max_iter=50)
    q = ddp.iLQG_queue(prob, x0, u0, slots=S, **kw)
    assert (q[6]["status"] > 0).all()
    for c0 in range(0, Pn, S):
        sel = np.arange(c0, c0 + S)
        r = ddp.iLQG(prob, x0[:, sel], u0[:, :, sel], timing=False, **kw)
        for a, b in ((q[0], r[0]), (q[1], r[1]), (q[2].K, r[2].K), (q[2].k, r[2].k), (q[2].Σi, r[2].Σi), (q[3], r[3]), (q[4], r[4]), (q[5], r[5])):
            assert _same(a[..., sel], b), c0
        assert _same(q[6]["stats"][:, sel], r[6]["stats"])


def test_mpc_closed_loop_on_device(ddp):
    """5 receding-horizon steps at (12, 12) with limits against the host loop built from iLQG + mpc_shift, bit for bit"""
    n, m, T, lim = SOLVES[1]
    P = solve_case(n, m, 40, lim)
    rng = np.random.default_rng(22)
    B, steps = 6, 5
    x0 = P["x0"][:, None] + 0.1 * rng.standard_normal((n, B))
    u0 = P["u0"][:, :, None] + 0.05 * rng.standard_normal((m, 40, B))
    prob = ddp.LQProblem(P["A"], P["B"], P["Q"], P["R"])
    kw = dict(lims=P["lims"], max_iter=20)
    xcl, ucl, scl, xp, up, git = ddp.iLQG_mpc(prob, x0, u0, steps, **kw)
    xs, us = x0.copy(), u0.copy()
    assert _same(xcl[:, 0], x0)
    for t in range(steps):
        r = ddp.iLQG(prob, xs, us, timing=False, **kw)
        assert _same(scl[:, t], r[6]["stats"]), t
        assert _same(xcl[:, t], r[0][:, 0]) and _same(ucl[:, t], r[1][:, 0]) and _same(xcl[:, t + 1], r[0][:, 1]), t
        xs = np.ascontiguousarray(r[0][:, 1])
        us = ddp.mpc_shift(r[1])
    assert _same(xp, r[0]) and _same(up, r[1])
    assert (scl[0] > 0).all() and np.abs(xcl[:, -1] - xcl[:, 0]).max() > 1e-3


def test_df_of_wide_controls(ddp):
    """cx = Q x, cu = R u at m = 12 (tiled kernel) and m = 32 (plain kernel) against NumPy"""
    rng = np.random.default_rng(9)
    for n, m in ((12, 12), (64, 32)):
        c = make_lq_case(n, n, m, 9, 4, np.ones(1), "", False, False, True)
        x = rng.standard_normal((n, 9, 4))
        out = ddp.df(ddp.LQProblem(c["A"], c["Bm"], c["Q"], c["R"]), x, c["u"])
        assert relerr(out[5], np.einsum("ij,jtb->itb", c["Q"], x)) < 1e-12 and relerr(out[6], np.einsum("ij,jtb->itb", c["R"], c["u"])) < 1e-12


# 8. ---------------------------------------------------------------------------------------------------------------- refusals
def test_refusals(ddp):
    c = bp_case(1, 10, 33, 5, 2)
    with pytest.raises(ddp.DDPError, match="32"):
        ddp.back_pass(c["cx"], c["cu"], c["cxx"], c["cxu"], c["cuu"], c["fx"], c["fu"], c["lam"], 1, None, None, c["u"])
    f = make_lq_case(2, 10, 33, 5, 2, np.ones(1), "", False, False, True)
    with pytest.raises(ddp.DDPError, match="32"):
        ddp.forward_pass(None, f["x0"], f["u"], None, 1.0, ddp.LQProblem(f["A"], f["Bm"], f["Q"], f["R"]), None)
    with pytest.raises(ddp.DDPError, match="32"):
        ddp.iLQG(ddp.LQProblem(f["A"], f["Bm"], f["Q"], f["R"]), f["x0"], f["u"], max_iter=2)
    with pytest.raises(ddp.DDPError):                               # user problems stop at DDP_MAX_M = 8
        ddp.DeviceProblem(ddp.example_source("lq"), 10, 9).check()
    # back_pass_gps stops at m = 8
    from ddp_amd import kl
    g = bp_case(3, 10, 9, 5, 2, "FCfc")
    terms = (np.zeros((10, 5, 2)), np.zeros((9, 5, 2)), np.zeros((10, 10, 5, 2)), np.zeros((9, 10, 5, 2)), np.tile(np.eye(9)[:, :, None, None], (1, 1, 5, 2)))
    with pytest.raises(ddp.DDPError):
        kl.back_pass_gps(g["cx"], g["cu"], g["cxx"], g["cxu"], g["cuu"], g["fx"], g["fu"], None, None, g["u"], (terms, np.array([1e-8, 1.0, 1e16])))
