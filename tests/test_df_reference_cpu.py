"""CPU side of the df tests (csrc/df.hip; the GPU side is tests/test_gpu_df_reference.py):
  * the plan of the matrix exponential — Padé degree and squarings from the 1-norm — asked of the library's debug hook
    ddp_df_expm_plan, the function the kernels call, over a table: every threshold and its neighbours, 5.4 * 2^k, the largest doubles,
    +Inf and NaN (degree 0: no exponential; the cast of ceil(log2(+Inf)) to int that stood there is undefined);
  * that every designed element of tests/df_cases.py lands on the degree and the number of squarings it was designed for;
  * the long double reference (tests/df_reference.py) against mpmath at 50 digits on every designed element: at least 100 times closer
    than the C oracle in every band, which is what entitles it to judge the oracle and the kernels;
  * the C oracle on the non-finite inputs."""
import ctypes as C
import math

import numpy as np
import pytest

import df_cases as dc
import df_reference as dr


@pytest.fixture(scope="module")
def hook():
    from ddp_amd import _lib
    L = _lib.lib()

    def ask(nA):
        deg, sq = C.c_int(-7), C.c_int(-7)
        assert L.ddp_df_expm_plan(C.c_double(nA), C.byref(deg), C.byref(sq)) == 0
        return deg.value, sq.value
    return ask


def test_plan_hook_over_the_table(hook):
    up = lambda v: np.nextafter(v, np.inf)          # noqa: E731
    dn = lambda v: np.nextafter(v, -np.inf)         # noqa: E731
    # a threshold belongs to the lower degree (nA <= thr), the next double to the higher one
    for thr, lo, hi in ((0.015, 3, 5), (0.25, 5, 7), (0.95, 7, 9), (2.1, 9, 13)):
        assert hook(dn(thr)) == (lo, 0) and hook(thr) == (lo, 0) and hook(up(thr)) == (hi, 0), thr
    # squarings: 5.4 * 2^k is scaled to exactly 5.4 by k squarings (x / 5.4 is exactly 2^k); the first double above 5.4 needs one
    assert hook(dn(5.4)) == (13, 0) and hook(5.4) == (13, 0) and hook(up(5.4)) == (13, 1)
    assert hook(dn(10.8)) == (13, 1) and hook(10.8) == (13, 1)
    for k in (0, 1, 2, 10):
        v = 5.4 * 2.0 ** k
        assert hook(v) == (13, k), k
        # the neighbour above: k + 1 squarings unless log2 rounds to k in double (k = 10: 10 + 3e-16 is 10) — then the scaled norm
        # is 5.4 (1 + 2^-52), which is the same plan for all purposes
        want = int(math.ceil(math.log2(up(v) / 5.4)))
        assert want in (k, k + 1) and hook(up(v)) == (13, want), k
    assert hook(up(5.4)) == (13, 1) and hook(up(10.8)) == (13, 2) and hook(up(21.6)) == (13, 3)
    assert hook(1e300) == (13, int(math.ceil(math.log2(1e300 / 5.4)))) == (13, 995)
    dmax = np.finfo(np.float64).max
    assert hook(dmax) == (13, 1022)
    assert hook(0.0) == (3, 0) and hook(np.finfo(np.float64).tiny) == (3, 0)
    # no plan for a norm that is not finite — and the hook is back at once: nothing loops on the count
    assert hook(np.inf) == (0, 0) and hook(np.nan) == (0, 0)
    for v in list(np.logspace(-6, 308, 400)) + [dmax, np.inf, np.nan]:
        deg, sq = hook(v)
        assert 0 <= sq <= 1024 and (deg, sq) == dc.plan(v), v


def test_plan_hook_takes_null_outputs():
    from ddp_amd import _lib
    assert _lib.lib().ddp_df_expm_plan(C.c_double(1.0), None, None) == 0


def test_every_designed_element_lands_where_it_was_designed(hook):
    """the design itself: >= 8 ladder elements per band with both signs of the (1, 0) entry, threshold pairs within 1e-3 on either side
    with different plans, column 1 setting the norm in the pair that says so — and the library's plan for each recorded norm"""
    per_band = [0] * len(dr.BANDS)
    signs = [set() for _ in dr.BANDS]
    for call in dc.ladder():
        M = call.matrices()
        for e in range(call.E):
            per_band[call.band[e]] += 1
            signs[call.band[e]].add(M[e, 1, 0] > 0)
            assert call.norm[e] == abs(M[e, 1, 0]), (call.name, e)                   # column 0 sets the norm
    assert min(per_band) >= 8 and all(s == {True, False} for s in signs), (per_band, signs)
    want_plans = {0.015: ((3, 0), (5, 0)), 0.25: ((5, 0), (7, 0)), 0.95: ((7, 0), (9, 0)), 2.1: ((9, 0), (13, 0)), 5.4: ((13, 0), (13, 1)),
                  10.8: ((13, 1), (13, 2))}
    for call in dc.threshold_pairs():
        if call.name.startswith("pair_col1"):
            h, d = call.par["h"], call.par["d"]
            assert (call.norm == abs(1.0 * h) + abs(-d * h)).all() and (np.abs(call.matrices()[:, 1, 0]) < 0.5 * call.norm).all()
            assert abs(call.norm[0] / 0.015 - 1) < 1e-3 and call.plan[0] == call.plan[1] == ((3, 0) if "below" in call.name else (5, 0))
            continue
        thr = float(call.name.split("_")[1])
        for e in range(4):
            rel = call.norm[e] / thr - 1
            assert 4e-4 < abs(rel) < 1e-3 and (rel > 0) == (e % 2 == 1), (call.name, e, rel)
            assert call.plan[e] == want_plans[thr][e % 2], (call.name, e)
        assert (call.matrices()[:2, 1, 0] < 0).all() and (call.matrices()[2:, 1, 0] > 0).all()
    a, b = dc.edges()
    Ma = a.matrices()
    assert Ma[0, 1, 0] == Ma[1, 1, 0] and a.ue[0] != a.ue[1]                         # sin θ = 0: u drops out
    assert abs(Ma[2, 1, 4]) < 1e-17 and abs(Ma[3, 1, 4]) < 1e-17                     # cos θ = 0 (to the rounding of π / 2)
    assert (Ma[4:6, 1, 0] > 0).all() and np.isnan(a.ue[8]) and np.isnan(b.ue[4])
    assert b.matrices()[0, 1, 0] == 0 and (b.matrices()[:, 1, 1] == 0).all()         # g = 0 and sin θ = 0; d = 0
    seen = set()
    for call in dc.all_finite_calls():
        for e in range(call.E):
            assert np.isfinite(call.norm[e]) and hook(call.norm[e]) == call.plan[e], (call.name, e)
            seen.add(call.plan[e][0])
            for thr in dc.THRESHOLDS:                                                  # clear of every threshold: the plan does not hang on the last place
                assert abs(call.norm[e] / thr - 1) > 4e-4, (call.name, e, thr)
    assert seen == {3, 5, 7, 9, 13}
    call, bad, plain = dc.nonfinite()
    assert [call.plan[e] for e in bad] == [(0, 0), (0, 0), (5, 0), (5, 0)] and call.plan[4][0] == 13
    for e in range(call.E):
        assert hook(call.norm[e]) == call.plan[e]
        if e not in bad:
            assert call.plan[e] == plain.plan[e] and call.plan[e][0] > 0


def _mp_block_distance(mp, E_mp, got):
    """max|got - E| / max|E| over rows 0..3 of the 5 x 5 exponential; got: long double or double [5, 5]"""
    num, den = mp.mpf(0), mp.mpf(0)
    for r in range(4):
        for c in range(5):
            g = got[r, c]
            hi = float(g)
            gm = mp.mpf(hi) + mp.mpf(float(g - dr.LD(hi)))                             # exact: 64 bits in two doubles
            num = max(num, abs(gm - E_mp[r, c])); den = max(den, abs(E_mp[r, c]))
    return float(num / den)


def test_long_double_reference_against_mpmath():
    """d_ld and d_orc: distance of the long double exponential and of the C oracle's to mpmath.expm at 50 digits, of the SAME double
    matrix, worst per band over every designed element.  Printed; asserted: d_ld <= d_orc / 100 in every band."""
    dr.need_longdouble()
    mp = pytest.importorskip("mpmath")
    from oracle import oracle_ctypes as oc
    d_ld, d_orc = [0.0] * len(dr.BANDS), [0.0] * len(dr.BANDS)
    with mp.workdps(50):
        for call in dc.all_finite_calls():
            M = call.matrices()
            E_ld = dr.expm_ld(M)
            for e in range(call.E):
                E_mp = mp.expm(mp.matrix(M[e].tolist()), method="taylor")
                b = call.band[e]
                d_ld[b] = max(d_ld[b], _mp_block_distance(mp, E_mp, E_ld[e]))
                d_orc[b] = max(d_orc[b], _mp_block_distance(mp, E_mp, oc.expm(M[e]).astype(dr.LD)))
    lo = 0.0
    for b, hi in enumerate(dr.BANDS):
        print("band (%g, %g]: d_orc = %.2e, d_ld = %.2e, ratio %.0f" % (lo, hi, d_orc[b], d_ld[b], d_orc[b] / d_ld[b]))
        lo = hi
    for b in range(len(dr.BANDS)):
        assert d_ld[b] * 100 <= d_orc[b], (b, d_ld[b], d_orc[b])


def test_oracle_df_against_long_double_per_band():
    """d_orc(band) of the whole df (matrix entries formed in double by the oracle, in long double by the reference) — the figure the
    GPU test scales its bound with; printed, and sanity-bounded by the growth the squarings explain: 2^squarings ulps"""
    dr.need_longdouble()
    worst = dc.oracle_band_distance()
    lo = 0.0
    for b, hi in enumerate(dr.BANDS):
        print("band (%g, %g]: d_orc(df) = %.2e" % (lo, hi, worst[b]))
        sq = dc.plan(hi)[1]
        assert 0 < worst[b] < 64 * 2.0 ** sq * 2.0 ** -52 * max(1.0, hi), (b, worst[b])
        lo = hi
    for call in dc.all_finite_calls():                                                # cx, cu of the oracle: a matrix-vector product's error
        r = dc.references(call)
        from oracle import oracle_ctypes as oc
        p = oc.make_problem("pendcart", 4, 1, call.E, Q=call.par["Q"], R=call.par["R"], pend=call.par)
        _, _, ocx, ocu = oc.df(p, call.xe, call.ue[None])
        sh = (call.N, call.B)
        assert dr.row_distance(ocx.reshape((4,) + sh, order="F"), r["cx"], r["cxs"]).max() <= 5 * 2.0 ** -53, call.name
        assert dr.row_distance(ocu.reshape((1,) + sh, order="F"), r["cu"], r["cus"]).max() <= 2.0 ** -53, call.name


def test_oracle_has_no_plan_for_a_norm_that_is_not_finite():
    """ddp_oracle_expm: +Inf in the matrix gives NaN by rule (degree 0), not by what a cast of +Inf to int happens to give"""
    from oracle import oracle_ctypes as oc
    M = np.zeros((5, 5)); M[0, 1] = 0.01; M[1, 0] = np.inf
    assert np.isnan(oc.expm(M)).all()
    M[1, 0] = -np.inf
    assert np.isnan(oc.expm(M)).all()
    call, bad, plain = dc.nonfinite()
    par = call.par
    p = oc.make_problem("pendcart", 4, 1, call.E, Q=par["Q"], R=par["R"], pend=par)
    fx, fu, cx, cu = oc.df(p, call.xe, call.ue[None])
    fx2, fu2, cx2, cu2 = oc.df(p, plain.xe, plain.ue[None])
    good = np.setdiff1d(np.arange(call.E), bad)
    assert np.isnan(fx[..., bad]).all() and np.isnan(fu[..., bad]).all()
    assert np.array_equal(fx[..., good], fx2[..., good]) and np.array_equal(fu[..., good], fu2[..., good])
    assert np.array_equal(cx[..., good], cx2[..., good]) and np.array_equal(cu[..., good], cu2[..., good])


def test_lq_reference_shapes_and_nan_control():
    dr.need_longdouble()
    for name, n, m, N, B, nan, mask in dc.LQ_SHAPES[:-1]:
        c = dc.lq_case(name)
        cx, cu, cxs, cus = dr.lq_df_ld(c["Q"], c["R"], c["x"], c["u"])
        assert cx.shape == (n, N, B) and cu.shape == (m, N, B) and cx.dtype == dr.LD
        u0 = np.where(np.isnan(c["u"]), 0.0, c["u"])
        assert np.isnan(c["u"]).sum() == (2 if (m, N, B) != (1, 1, 1) else 1) and np.isfinite(cu.astype(float)).all()
        ref = np.einsum("ij,jtb->itb", c["R"], u0)
        assert dr.row_distance(ref, cu, cus).max() <= (m + 1) * 2.0 ** -53
        assert dr.row_distance(np.einsum("ij,jtb->itb", c["Q"], c["x"]), cx, cxs).max() <= (n + 1) * 2.0 ** -53
