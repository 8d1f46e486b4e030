"""The derivative kernels of csrc/df.hip on the device against long double (tests/df_reference.py), on the designed inputs of
tests/df_cases.py.  Every call goes through ddp_df_f64_dev on buffers of its own: outputs pre-filled with a NaN-payload sentinel, eight
guard words before and after each, fx and fu placed at a 16-byte boundary or 8 bytes past one.

Bound of the pendcart exponential.  d(element) = max|got - ref| / max|ref| over the element's 4 x 5 block [fx fu].  The kernels and the
C oracle do the same operations in the same order and differ by FMA contraction and the device's sin / cos, so the kernel is held to the
oracle's own distance from long double: d_gpu(element) <= K * max(d_orc(band), F), d_orc(band) computed at run time as the oracle's worst
distance over the designed elements of the band, F = 4 * 2^-52 a floor for bands where d_orc is itself around an ulp, K the margin:
the worst d_gpu / max(d_orc, F) measured per band on the MI355X, doubled and rounded up (table below).  cx, cu and the LQ
products are held to the product's own bound, (n + 1) 2^-53 |Q||x| row by row (one rounding for x - goal, n for the sum).

Measured on the MI355X over every designed finite element (test 1 prints the table):
  band            d_orc     d_gpu     d_gpu / d_orc   d_gpu / max(d_orc, F)   K = that, doubled and rounded up
  (0, 0.015]      2.21e-16  2.21e-16  1.00            0.25                    1
  (0.015, 0.25]   2.42e-16  2.42e-16  1.00            0.27                    1
  (0.25, 0.95]    3.07e-16  3.99e-16  1.30            0.45                    1
  (0.95, 2.1]     5.88e-16  5.88e-16  1.00            0.66                    2
  (2.1, 5.4]      4.86e-16  3.61e-16  0.74            0.41                    1
  (5.4, 10.8]     4.95e-16  3.75e-16  0.76            0.42                    1
  (10.8, 43]      6.43e-15  3.84e-15  0.60            0.60                    2
  (43, 700]       6.67e-13  7.19e-13  1.08            1.08                    3
  (700, 3e4]      1.08e-09  2.25e-10  0.21            0.21                    1
Up to 10.8 everything sits within three ulps and under the floor; beyond, d_orc grows with the squarings (2^squarings, times the norm
in the conditioning of exp) and the kernel grows with it: no band needs a margin that contraction does not explain."""
import ctypes as C
import os

import numpy as np
import pytest

import df_cases as dc
import df_reference as dr

pytestmark = pytest.mark.gpu

SENT = np.uint64(0x7FF8DEAD0000BEEF)             # a quiet NaN no arithmetic produces
GUARD = 8                                        # words before and after every output
U = 2.0 ** -53
F_FLOOR = 4 * 2.0 ** -52
K_BAND = {0.015: 1, 0.25: 1, 0.95: 1, 2.1: 2, 5.4: 1, 10.8: 1, 43.0: 2, 700.0: 3, 3e4: 1}


@pytest.fixture
def ddp(monkeypatch):
    dr.need_longdouble()
    import ddp_amd
    for k in [k for k in os.environ if k.startswith("DDP_") and not k.startswith("DDP_AMD_")]:
        monkeypatch.delenv(k)
    ddp_amd.default_handle().raw
    yield ddp_amd


class Out:
    """an output of `count` doubles on the device, `off` bytes (0 or 8) past a 16-byte boundary, sentinels and guards around it"""

    def __init__(self, h, count, off=0):
        from ddp_amd import _lib
        self.h, self.count, self.off = h, int(count), off
        self.total = 2 * GUARD + 2 + self.count
        host = np.full(self.total, SENT, dtype=np.uint64)
        self.base = h.malloc(self.total * 8)
        _lib.check(_lib.lib().ddp_memcpy_h2d(h.raw, self.base, host.ctypes.data_as(C.c_void_p), C.c_size_t(host.nbytes)))
        assert self.base.value % 16 == 0
        self.ptr = C.c_void_p(self.base.value + 8 * GUARD + off)

    def fetch(self, shape):
        """the payload as float64 (Fortran order) after checking that nothing around it was written"""
        whole = self.h.to_host(self.base, (self.total,), dtype=np.uint64)
        self.h.free(self.base)
        lo = GUARD + self.off // 8
        assert (whole[:lo] == SENT).all() and (whole[lo + self.count:] == SENT).all(), "guard words written"
        return whole[lo:lo + self.count].view(np.float64).reshape(shape, order="F").copy(order="F")


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(bits(np.asfortranarray(a)).ravel(), bits(np.asfortranarray(b)).ravel())


def untouched(a):
    return (bits(np.asfortranarray(a)) == SENT)


def run_df(ddp, kind, n, m, N, B, Q, R, x, u, par=None, active=None, off=(0, 0), handle=None):
    """one ddp_df_f64_dev call; returns dict(cx, cu[, fx, fu]) as host arrays"""
    from ddp_amd import _lib
    h = handle or ddp.default_handle()
    L = _lib.lib()
    ins = [h.to_device(np.asfortranarray(a, dtype=np.float64)) for a in (Q, R, x, u)]
    dact = h.to_device(np.ascontiguousarray(active, dtype=np.int32)) if active is not None else None
    p = _lib.Problem()
    p.kind, p.n, p.m, p.N, p.B = kind, n, m, N, B
    p.Q, p.R = ins[0].value, ins[1].value
    if kind == 1:
        p.g, p.l, p.h, p.d = par["g"], par["l"], par["h"], par["d"]
        for i in range(4):
            p.goal[i] = float(par["goal"][i])
    cx, cu = Out(h, n * N * B), Out(h, m * N * B)
    fx = Out(h, n * n * N * B, off[0]) if kind == 1 else None
    fu = Out(h, n * m * N * B, off[1]) if kind == 1 else None
    _lib.check(L.ddp_df_f64_dev(h.raw, C.byref(p), ins[2], ins[3], dact, cx.ptr, cu.ptr, fx.ptr if fx else None, fu.ptr if fu else None))
    h.sync()
    out = dict(cx=cx.fetch((n, N, B)), cu=cu.fetch((m, N, B)))
    if kind == 1:
        out["fx"] = fx.fetch((n, n, N, B)); out["fu"] = fu.fetch((n, m, N, B))
    for d in ins + ([dact] if dact is not None else []):
        h.free(d)
    return out


def run_pend(ddp, call, **kw):
    par = call.par
    return run_df(ddp, 1, 4, 1, call.N, call.B, par["Q"], par["R"], call.x, call.u, par=par, **kw)


def check_costs(call, got, ref):
    assert dr.row_distance(got["cx"], ref["cx"], ref["cxs"]).max() <= 5 * U, call.name
    assert dr.row_distance(got["cu"], ref["cu"], ref["cus"]).max() <= U, call.name


def test_ladder_pairs_and_edges_against_long_double(ddp, monkeypatch):
    """1. every designed finite element, default path (MODE 1 + MODE 2) and DDP_DF_DENSE=1 (MODE 0): the same bits, and each element
    inside the bound of its band; cx and cu against long double.  Would have caught: a wrong Padé coefficient or degree choice in either
    routine (each degree has its own elements on both sides of its threshold), a term dropped from the zero-last-row routine, an error
    in one small element that a per-array norm hides behind a large one."""
    calls = dc.all_finite_calls()
    monkeypatch.delenv("DDP_DF_DENSE", raising=False)
    fast = [run_pend(ddp, c) for c in calls]
    monkeypatch.setenv("DDP_DF_DENSE", "1")
    dense = [run_pend(ddp, c) for c in calls]
    monkeypatch.delenv("DDP_DF_DENSE")
    ddp.default_handle().raw
    d_orc = dc.oracle_band_distance()
    worst_gpu, worst_ratio, worst_raw = [0.0] * len(dr.BANDS), [0.0] * len(dr.BANDS), [0.0] * len(dr.BANDS)
    fails = []
    for call, a, b in zip(calls, fast, dense):
        for k in ("cx", "cu", "fx", "fu"):
            assert same_bits(a[k], b[k]), (call.name, k)
            assert not untouched(a[k]).any(), (call.name, k)
        ref = dc.references(call)
        check_costs(call, a, ref)
        d = dr.block_distance(a["fx"], a["fu"], ref["fx"], ref["fu"]).ravel(order="F")
        for e in range(call.E):
            bd = call.band[e]
            base = max(d_orc[bd], F_FLOOR)
            worst_gpu[bd] = max(worst_gpu[bd], d[e]); worst_ratio[bd] = max(worst_ratio[bd], d[e] / base)
            worst_raw[bd] = max(worst_raw[bd], d[e] / ref["d_orc"][e] if ref["d_orc"][e] > 0 else 0.0)
            if not d[e] <= K_BAND[dr.BANDS[bd]] * base:
                fails.append((call.name, e, bd, d[e], base))
    lo = 0.0
    for bd, hi in enumerate(dr.BANDS):
        print("band (%g, %g]: d_orc = %.2e  d_gpu = %.2e  d_gpu / max(d_orc, F) = %.2f  worst per-element d_gpu / d_orc = %.2f  K = %d"
              % (lo, hi, d_orc[bd], worst_gpu[bd], worst_ratio[bd], worst_raw[bd], K_BAND[hi]))
        lo = hi
    assert not fails, fails


def test_mode2_grid_stride_wraps(ddp):
    """2. N B = 65 920 > 1024 x 64: the second pass of MODE 2's loop.  Large-norm elements at flat indices 0, 65 535, 65 536, 65 537 and
    the last equal the same (x, u) computed in a ten-element call, bit for bit; a sample of ordinary elements against long double.
    Would have caught: a stride or bound error in the fixed-grid loop (elements past 65 536 left to MODE 1's flag and never written)."""
    N, B = 1030, 64
    E = N * B
    rng = np.random.default_rng(5)
    xe = np.vstack([rng.uniform(-4, 4, (1, E)), rng.standard_normal((3, E))])
    ue = rng.uniform(-3, 3, E)
    big = np.array([0, 65535, 65536, 65537, E - 1])
    xe[0, big] = [1.0, -2.0, 0.7, 2.4, -1.2]
    ue[big] = [400.0, -2500.0, 300.0, 1e4, -700.0]
    assert (dc.kernel_norm(dc.DEFAULT, xe[0, big], ue[big]) > 2.2).all()
    whole = dc.PendCall("wrap", dc.DEFAULT, xe[0], ue, rest=xe[1:], B=B)
    others = np.setdiff1d(np.arange(E), big)
    assert (whole.norm[others] <= 2.0).all() and all(whole.plan[i][0] == 13 for i in big)  # nothing else asks for MODE 2
    got = run_pend(ddp, whole)
    for k in ("cx", "cu", "fx", "fu"):
        assert not untouched(got[k]).any(), k
    ten_idx = np.concatenate([big, [1, 2, 3, 70000 % E, 12345]])
    ten = dc.PendCall("wrap_ten", dc.DEFAULT, xe[0, ten_idx], ue[ten_idx], rest=xe[1:, ten_idx], B=1)
    small = run_pend(ddp, ten)
    flat = lambda a: a.reshape(a.shape[:-2] + (E,), order="F")                         # noqa: E731
    for k in ("cx", "cu", "fx", "fu"):
        assert same_bits(flat(got[k])[..., ten_idx], small[k][..., 0]), k
    idx = np.concatenate([big, rng.choice(E, 59, replace=False)])
    sample = dc.PendCall("wrap_sample", dc.DEFAULT, xe[0, idx], ue[idx], rest=xe[1:, idx], B=1)
    ref = dc.references(sample)
    d_orc = dc.oracle_band_distance(extra=zip(sample.band, ref["d_orc"]))
    d = dr.block_distance(flat(got["fx"])[..., idx, None], flat(got["fu"])[..., idx, None], ref["fx"], ref["fu"]).ravel(order="F")
    for e in range(sample.E):
        bd = sample.band[e]
        assert d[e] <= K_BAND[dr.BANDS[bd]] * max(d_orc[bd], F_FLOOR), (e, idx[e], bd, d[e], d_orc[bd])
    check_costs(sample, dict(cx=flat(got["cx"])[..., idx, None], cu=flat(got["cu"])[..., idx, None]), ref)


def test_store_paths_by_alignment(ddp):
    """3. fx and fu at a 16-byte boundary and 8 bytes past one, all four combinations: the 16-byte stores run only for the first; the
    same bits, guards intact (checked in every fetch).  Would have caught: a wrong offset in the paired stores of the fu tail (entries
    16..19 of the 4 x 5 result) or the launcher taking the vector path for a pointer it may not."""
    call = dc.edges()[0]
    base = run_pend(ddp, call, off=(0, 0))
    for off in ((0, 8), (8, 0), (8, 8)):
        got = run_pend(ddp, call, off=off)
        for k in ("cx", "cu", "fx", "fu"):
            assert same_bits(got[k], base[k]), (off, k)
    ref = dc.references(call)
    check_costs(call, base, ref)


def test_active_mask(ddp):
    """4. an inactive trajectory keeps its sentinels in cx, cu, fx and fu — also the one that holds a large-norm element, which MODE 2
    (run here: an active trajectory raises the flag) must not write; active trajectories equal the unmasked call.  Would have caught:
    MODE 2 ignoring the mask."""
    call = dc.edges()[1]
    assert call.B == 3 and call.plan[3][0] == 13 and call.plan[5][0] == 13             # trajectory 1 (elements 2, 3) and 2 (4, 5)
    full = run_pend(ddp, call)
    active = np.array([1, 0, 1], dtype=np.int32)
    got = run_pend(ddp, call, active=active)
    for k in ("cx", "cu", "fx", "fu"):
        assert untouched(got[k][..., 1]).all(), k
        assert same_bits(got[k][..., [0, 2]], full[k][..., [0, 2]]), k
    none = run_pend(ddp, call, active=np.zeros(3, dtype=np.int32))
    for k in ("cx", "cu", "fx", "fu"):
        assert untouched(none[k]).all(), k


def test_flag_word_is_reset_between_calls(ddp):
    """5. one handle: a call with large norms (the flag goes up), then a call without — equal, bit for bit, to that call made first on a
    fresh handle.  Would have caught: a stale flag letting MODE 2 rewrite elements of the second call."""
    from ddp_amd import _lib
    loud, quiet = dc.edges()[0], dc.ladder()[3]
    assert any(p[0] == 13 for p in loud.plan) and all(p[0] <= 9 for p in quiet.plan)
    h1, h2 = _lib.Handle(0), _lib.Handle(0)
    try:
        run_pend(ddp, loud, handle=h1)
        second = run_pend(ddp, quiet, handle=h1)
        first = run_pend(ddp, quiet, handle=h2)
    finally:
        h1.close(); h2.close()
    for k in ("cx", "cu", "fx", "fu"):
        assert same_bits(second[k], first[k]), k


@pytest.mark.parametrize("name", [s[0] for s in dc.LQ_SHAPES])
def test_lq_shapes_against_long_double(ddp, name):
    """6. cx = Q x, cu = R u on both LQ kernels: idle threads of a tile, a last tile that is not full, the tile loop wrapping past its
    8 192 blocks, m > 16 on the one-thread-per-column kernel; a NaN control reads as zero; inactive columns keep their sentinels and
    active ones equal the unmasked call.  Would have caught: a tile index or column bound error at any of these shapes."""
    c = dc.lq_case(name)
    n, m, N, B = c["n"], c["m"], c["N"], c["B"]
    full = run_df(ddp, 0, n, m, N, B, c["Q"], c["R"], c["x"], c["u"])
    cx, cu, cxs, cus = dr.lq_df_ld(c["Q"], c["R"], c["x"], c["u"])
    assert not untouched(full["cx"]).any() and not untouched(full["cu"]).any()
    dx, du = dr.row_distance(full["cx"], cx, cxs).max(), dr.row_distance(full["cu"], cu, cus).max()
    print("%s: cx %.2f u, cu %.2f u" % (name, dx / U, du / U))
    assert dx <= (n + 1) * U and du <= (m + 1) * U
    got = run_df(ddp, 0, n, m, N, B, c["Q"], c["R"], c["x"], c["u"], active=c["active"])
    on = c["active"] != 0
    assert on.any() and not on.all()
    for k in ("cx", "cu"):
        assert untouched(got[k][..., ~on]).all(), k
        assert same_bits(got[k][..., on], full[k][..., on]), k


def test_nonfinite_inputs(ddp, monkeypatch):
    """7. u = +-Inf (no plan: degree 0), θ = NaN and θ = Inf between ordinary elements, on the default path and on the dense one: fx and
    fu of those elements are NaN throughout, cx and cu are the reference's, and every other element has the bits of the call without
    them.  Before expm_plan the infinite controls sent a lane into ceil(log2(+Inf)) squarings."""
    call, bad, plain = dc.nonfinite()
    with np.errstate(invalid="ignore", over="ignore"):
        _, _, cx, cu, cxs, cus = dr.pend_df_ld(call.par, call.x, call.u)
    good = np.setdiff1d(np.arange(call.E), bad)
    flat = lambda a: a.reshape(a.shape[:-2] + (call.E,), order="F")                    # noqa: E731
    for dense in (False, True):
        if dense:
            monkeypatch.setenv("DDP_DF_DENSE", "1")
        else:
            monkeypatch.delenv("DDP_DF_DENSE", raising=False)
        want = run_pend(ddp, plain)
        got = run_pend(ddp, call)
        assert np.isnan(flat(got["fx"])[..., bad]).all() and np.isnan(flat(got["fu"])[..., bad]).all(), dense
        assert not untouched(got["fx"]).any() and not untouched(got["fu"]).any()
        for k in ("cx", "cu", "fx", "fu"):
            assert same_bits(flat(got[k])[..., good], flat(want[k])[..., good]), (dense, k)
        gcx, gcu = flat(got["cx"]), flat(got["cu"])
        rcx, rcu = flat(cx).astype(np.float64), flat(cu).astype(np.float64)
        fin = np.isfinite(rcx)
        assert np.array_equal(gcx[~fin], rcx[~fin], equal_nan=True) and np.array_equal(gcu, rcu, equal_nan=True)
        assert np.isnan(gcx[:, bad[2]]).all() and np.isinf(gcx[:, bad[3]]).all() and fin[:, bad[:2]].all()  # NaN where x is, Inf where x is
        assert np.array_equal(gcu[:, bad[:2]], np.array([[np.inf, -np.inf]]) * call.par["R"][0, 0])
        with np.errstate(invalid="ignore"):                                            # (Inf - Inf in the columns left out by `fin`)
            assert (dr.row_distance(gcx, flat(cx), flat(cxs))[fin] <= 5 * U).all()
    monkeypatch.delenv("DDP_DF_DENSE")
    ddp.default_handle().raw
