"""The yardstick of the n <= 32, m <= 8 KL kernels, checked where no GPU is needed:
  * the long double restatement (tests/kl_reference.py) against the C oracle and the NumPy restatement on every case of
    tests/kl_narrow_cases.py, with the worst oracle-to-long-double distance per operation printed (DESIGN.md §KL quotes the table:
    it is the measured base of the tolerance tests/test_gpu_kl_narrow.py asserts);
  * the Inf / NaN / 0 pattern of every designed input on all three;
  * the kernel choice of forward_covariance and kl_div_wiki (csrc/kl.hip, fcov_choose and kl_div_choose), asked of the library's
    unlisted debug hooks ddp_fcov_choice / ddp_kl_div_choice — the functions the entry points call — for every row of the tables,
    for every row under each switch, and over the whole 32 x 8 box against the image formula restated here;
  * that the designed inputs are what they claim to be, in long double."""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import ROOT, relerr
import kl_narrow_cases as nc
import kl_reference as ref

LIB = os.path.join(ROOT, "differentialdynamicprogramming.jl_amd", "libddp_amd.so")
RTOL = nc.RTOL


def _cases(rows):
    return sorted({(r["n"], r["m"], r["N"], r["B"]) for r in rows})


_worst = {}


def _note(op, d, key):
    if d > _worst.get(op, (-1.0, None))[0]:
        _worst[op] = (d, key)
    print("d_orc %-11s %-22s %.3e   (worst so far %.3e at %s)" % (op, key, d, _worst[op][0], _worst[op][1]))


# ------------------------------------------------------------------------------------------------- reference against the oracles
@pytest.mark.parametrize("n,m,N,B", _cases(nc.TERMS))
def test_grad_kl_reference_matches_both_oracles(n, m, N, B):
    ref.need_longdouble()
    c, want = nc.case(n, m, N, B), nc.ref_terms(n, m, N, B)
    assert all(w.dtype == ref.LD for w in want)
    for b in range(B):
        for which in ("c", "np"):
            for a, w, nm in zip(nc.oracle_terms(which, c, b), want, ("cx", "cu", "cxx", "cxu", "cuu")):
                assert relerr(a, w[..., b]) < RTOL, (which, nm, b)
    _note("∇kl", nc.oracle_dist("terms", n, m, N, B), (n, m, N, B))


@pytest.mark.parametrize("n,m,N,B", _cases(nc.FCOV))
def test_forward_covariance_reference_matches_both_oracles(n, m, N, B):
    ref.need_longdouble()
    c = nc.case(n, m, N, B)
    for shared in (False, True):
        want = nc.ref_fcov(n, m, N, B, shared)
        assert want.dtype == ref.LD and want.shape == (n + m, n + m, N, B)
        assert not want[n:, :, N - 1].any() and not want[:, n:, N - 1].any()          # the last step has no policy block
        for b in list(range(min(B, 8))) + ([B - 1] if B > 8 else []):
            for which in ("c", "np"):
                assert relerr(nc.oracle_fcov(which, c, b, shared), want[..., b]) < RTOL, (which, shared, b)
        _note("fcov", nc.oracle_dist("fcov_shared" if shared else "fcov", n, m, N, B), (n, m, N, B, "shared" if shared else "own"))


@pytest.mark.parametrize("n,m,N,B", _cases(nc.KLDIV))
def test_kl_div_reference_matches_both_oracles(n, m, N, B):
    ref.need_longdouble()
    c = nc.case(n, m, N, B)
    kld, mean = nc.ref_kl_div(n, m, N, B)
    assert kld.dtype == ref.LD and np.all(np.isfinite(kld.astype(float))) and np.all(kld >= 0)
    assert kld.astype(float).max() > 0                                                 # (not a case the clamp empties)
    for b in range(B):
        for which in ("c", "np"):
            got, gm = nc.oracle_kl_div(which, c, b)
            assert relerr(got, kld[:, b], 0) < RTOL, (which, b)
            assert abs(gm - float(mean[b])) <= RTOL * float(mean[b]), (which, b)
    _note("kl_div_wiki", nc.oracle_dist("kl_div", n, m, N, B), (n, m, N, B))


def test_lu_logdet_against_slogdet():
    ref.need_longdouble()
    rng = np.random.default_rng(11)
    for m in (1, 2, 3, 5, 8):
        A = rng.standard_normal((m, m, 40))
        ld, sg = ref.lu_logdet(A)
        s, l = np.linalg.slogdet(np.moveaxis(A, 2, 0))
        assert np.array_equal(sg, s.astype(int)) and np.max(np.abs(ld.astype(float) - l)) < 1e-12
    ld, sg = ref.lu_logdet(np.zeros((3, 3, 1)))
    assert ld[0] == -np.inf and sg[0] == 0
    Z = np.array([[1.0, 2.0], [2.0, 4.0]])[:, :, None]                                  # singular without a zero entry: an exact zero pivot
    assert ref.lu_logdet(Z)[0][0] == -np.inf


# ------------------------------------------------------------------------------------------------- designed inputs
def _three(c):
    """(kldiv[T,B], mean[B]) of the long double reference, the C oracle and np_kl; a call that threw leaves NaN-free finite kldiv of its
    own: the oracles return the scalar Inf then, so their kldiv row is taken from the reference (only the mean is theirs)"""
    kld, mean, threw = ref.kl_div_wiki(*[c[k_] for k_ in nc.KL_ARGS])
    out = {"long double": (kld.astype(float), mean.astype(float))}
    for which, tag in (("c", "C oracle"), ("np", "np_kl")):
        rows, means = [], []
        for b in range(c["B"]):
            r, mu = nc.oracle_kl_div(which, c, b)
            assert (r is None) == bool(threw[b]), (tag, b)
            rows.append(kld[:, b].astype(float) if r is None else r); means.append(mu)
        out[tag] = (np.stack(rows, 1), np.array(means))
    return out


@pytest.mark.parametrize("n,m,kind", nc.designed_ids())
def test_designed_input_outcomes_on_reference_and_oracles(n, m, kind):
    ref.need_longdouble()
    c = nc.designed(n, m, kind)
    res = _three(c)
    base = nc.ref_kl_div(n, m, nc.DN, nc.DB)[0].astype(float)
    ld_kld, ld_mean = res["long double"]
    for tag, (kld, mean) in res.items():
        nc.check_designed(n, m, kind, kld, mean)
        # the same Inf / NaN / 0 pattern on all three ("inverse": which steps round to 0 is rounding's choice; its bound is the check)
        assert np.array_equal(np.isnan(kld), np.isnan(ld_kld)) and np.array_equal(np.isposinf(kld), np.isposinf(ld_kld)), tag
        assert np.array_equal(np.isnan(mean), np.isnan(ld_mean)) and np.array_equal(np.isposinf(mean), np.isposinf(ld_mean)), tag
        if kind == "inverse":
            continue
        assert np.array_equal(kld == 0, ld_kld == 0), tag
        fin = np.isfinite(ld_kld)
        assert np.max(np.abs(kld[fin] - ld_kld[fin])) <= RTOL * max(ld_kld[fin].max(), 1e-300), tag
        if kind != "identical":                              # outside the designed step: the undesigned case's values
            other = np.ones(kld.shape, bool); other[nc.DT, nc.DTRAJ] = False
            assert np.max(np.abs(kld[other] - base[other])) <= RTOL * base.max(), tag


@pytest.mark.parametrize("n,m", nc.DESIGNED_SHAPES)
def test_designed_inputs_are_what_they_claim(n, m):
    ref.need_longdouble()
    t, b = nc.DT, nc.DTRAJ
    # condition numbers of every policy covariance of every case of the tables: below 1e2 (long double singular values are not
    # available: float64 cond of a matrix this well conditioned is good to 1e-14)
    c = nc.case(n, m, nc.DN, nc.DB)
    for key in ("Sn", "Sp", "Sip"):
        assert max(np.linalg.cond(c[key][:, :, i, j]) for i in range(nc.DN) for j in range(nc.DB)) < 1e2
    # row exchange: zero leading entry, positive determinant, one exchange and one negative pivot, no tie in any pivot column
    S = nc.designed(n, m, "row_exchange")["Sn"][:, :, t, b]
    assert S[0, 0] == 0.0
    trace = []
    ld, sg = ref.lu_logdet(S[:, :, None], trace)
    assert sg[0] == 1 and np.isfinite(float(ld[0]))
    assert trace[0][1][0] != 0 and all(tr[1][0] == col for col, tr in enumerate(trace) if col > 0)       # exactly one exchange, in column 0
    for mag, _ in trace:
        v = np.sort(mag[:, 0])
        assert np.all(np.diff(v) > 0.05 * v[-1]), "pivot-column magnitudes must be distinct"
    assert abs(float(np.exp(ld[0])) - np.linalg.det(S)) < 1e-12 and np.linalg.det(S) > 0
    # negative determinant, singular Σn and Σp
    assert ref.lu_logdet(nc.designed(n, m, "negative_det")["Sn"][:, :, t, b][:, :, None])[1][0] == -1
    for kind, key in (("singular_new", "Sn"), ("singular_prev", "Sp")):
        ld, sg = ref.lu_logdet(nc.designed(n, m, kind)[key][:, :, t, b][:, :, None])
        assert ld[0] == -np.inf and sg[0] == 0
    # every other determinant of the designed cases is positive
    for kind in nc.DESIGNED:
        d = nc.designed(n, m, kind)
        for key in ("Sn", "Sp"):
            sg = ref.lu_logdet(d[key].reshape(m, m, -1))[1].reshape(nc.DN, nc.DB)
            keep = np.ones((nc.DN, nc.DB), bool)
            if (kind, key) in (("negative_det", "Sn"), ("singular_new", "Sn"), ("singular_prev", "Sp")):
                keep[t, b] = False
            assert np.all(sg[keep] == 1), (kind, key)
    x = nc.designed(n, m, "nan")["xnew"]
    assert np.isnan(x[0, t, b]) and np.isnan(x).sum() == 1


def test_all_table_covariances_are_well_conditioned():
    worst = 0.0
    for (n, m, N, B) in _cases(nc.KLDIV + nc.FCOV + nc.TERMS):
        if B > 64:
            continue
        c = nc.case(n, m, N, B)
        for key in ("Sn", "Sp", "Sip"):
            worst = max(worst, float(np.linalg.cond(np.moveaxis(c[key], (0, 1), (-2, -1))).max()))
    print("worst condition number of a policy covariance: %.1f" % worst)
    assert worst < 1e2


# ------------------------------------------------------------------------------------------------- whole loops: the reference is continuous
@pytest.mark.parametrize("n,m,T,seed", nc.LOOPS)
def test_loop_reference_is_not_discontinuous_at_the_inputs(n, m, T, seed):
    assert nc.image_fits(n, m) and (n, m) not in ((4, 1), (4, 2))                       # a shape kl_div_lds_kernel<0,0> serves
    refs = nc.loop_reference(n, m, T, seed)
    for b in range(nc.LOOP_B):
        want = nc.outcome(refs[b][6])
        near = nc.loop_outcomes_nearby(n, m, T, seed, b, 1000 + b)
        print("(%d, %d, %d) trajectory %d: outcome %s, nearby %s" % (n, m, T, b, want, sorted(set(near))))
        assert all(o == want for o in near), (b, want, near)
    assert any(r[6]["iter"] > 1 for r in refs)                                          # (the loop does iterate)


# ------------------------------------------------------------------------------------------------- kernel choice
@pytest.fixture(scope="module")
def choice():
    if not os.path.exists(LIB):
        pytest.skip("libddp_amd.so not built")
    try:
        L = C.CDLL(LIB)
    except OSError as e:                      # no HIP runtime on this host
        pytest.skip(str(e))
    s = C.c_char_p
    L.ddp_fcov_choice.restype = s
    L.ddp_fcov_choice.argtypes = [C.c_int] * 7 + [s, s, s]
    L.ddp_kl_div_choice.restype = s
    L.ddp_kl_div_choice.argtypes = [C.c_int] * 5 + [s, s]
    return L


def _e(v):
    return None if v is None else v.encode()


def fcov(L, n, m, N, B=3, al16=1, sink=1, wide=0, gps_wide=None, q4=None, q4l=None):
    return L.ddp_fcov_choice(n, m, N, B, al16, sink, wide, _e(gps_wide), _e(q4), _e(q4l)).decode()


def kldiv(L, n, m, N, B=3, wide=0, gps_wide=None, lds=None):
    return L.ddp_kl_div_choice(n, m, N, B, wide, _e(gps_wide), _e(lds)).decode()


def _inline_fcov(n, m, N, B, al16, sink, q4, q4l):
    """the conditions ddp_forward_covariance_f64_dev held inline before fcov_choose (n <= 32, m <= 8, switch off)"""
    if n == 4 and m in (1, 2) and sink and not (q4 and q4[0] == "0"):
        if m == 1 and N % 8 == 0 and N >= 16 and al16 and B <= 6144 and not (q4l and q4l[0] == "0"):
            return nc.Q4L
        return nc.Q4_1 if m == 1 else nc.Q4_2
    return nc.GENERIC


def _inline_kl_div(n, m, lds):
    """the conditions ddp_kl_div_f64_dev held inline before kl_div_choose"""
    if nc.image_fits(n, m) and not (lds and lds[0] == "0"):
        return nc.LDS41 if (n, m) == (4, 1) else nc.LDS42 if (n, m) == (4, 2) else nc.LDS00
    return nc.DIRECT


@pytest.mark.parametrize("r", nc.KLDIV, ids=nc.kid)
def test_kl_div_table_row(choice, r):
    n, m, N, B = r["n"], r["m"], r["N"], r["B"]
    assert kldiv(choice, n, m, N, B, lds=r["env"]) == r["want"] == _inline_kl_div(n, m, r["env"])
    assert kldiv(choice, n, m, N, B, lds="0") == nc.DIRECT                              # the switch, for every row
    assert kldiv(choice, n, m, N, B, lds="1") == _inline_kl_div(n, m, None)
    assert kldiv(choice, n, m, N, B, gps_wide="1") == "kl_div_wide_kernel"
    assert kldiv(choice, n, m, N, B, wide=1, lds=r["env"]) == r["want"]                 # the handle's switch leaves the small box alone


@pytest.mark.parametrize("r", nc.FCOV, ids=nc.kid)
def test_fcov_table_row(choice, r):
    n, m, N, B = r["n"], r["m"], r["N"], r["B"]
    al, (q4, q4l) = int(not r["mis"]), r["env"]
    assert fcov(choice, n, m, N, B, al, q4=q4, q4l=q4l) == r["want"] == _inline_fcov(n, m, N, B, al, 1, q4, q4l)
    assert fcov(choice, n, m, N, B, al, q4="0", q4l=q4l) == nc.GENERIC                  # each switch, for every row
    assert fcov(choice, n, m, N, B, al, q4=q4, q4l="0") == (nc.Q4_1 if r["want"] == nc.Q4L else r["want"])
    assert fcov(choice, n, m, N, B, al, q4="0", q4l="0") == nc.GENERIC
    assert fcov(choice, n, m, N, B, al, sink=0, q4=q4, q4l=q4l) == nc.GENERIC           # no sink buffer: no four-per-wave kernel
    assert fcov(choice, n, m, N, B, al, gps_wide="1", q4=q4, q4l=q4l) == "fcov_wide_kernel"
    assert fcov(choice, n, m, N, B, al, wide=1, q4=q4, q4l=q4l) == r["want"]


def test_every_kernel_is_in_the_tables():
    assert {r["want"] for r in nc.KLDIV} == {nc.DIRECT, nc.LDS41, nc.LDS42, nc.LDS00}
    assert {r["want"] for r in nc.FCOV} == {nc.GENERIC, nc.Q4_1, nc.Q4_2, nc.Q4L}
    assert {r["N"] for r in nc.KLDIV if r["want"] == nc.LDS00} >= {1, 64, 65, 130}


def test_lds_is_chosen_exactly_when_the_image_fits(choice):
    fits = 0
    for n in range(1, 33):
        for m in range(1, 9):
            lens = [n, n, (n + m) * (n + m), n * m, m, m * m, n * m, m, m * m, m * m]       # the ten operands of a step
            image = sum((l | 1) * 64 * 8 for l in lens)                                     # odd strides, 64 steps, doubles
            got = kldiv(choice, n, m, 65)
            assert got.startswith("kl_div_lds_kernel") == (image <= 48 * 1024), (n, m, image, got)
            assert got == _inline_kl_div(n, m, None) and kldiv(choice, n, m, 65, lds="0") == nc.DIRECT
            fits += image <= 48 * 1024
    # n <= 6 with m = 1 (6), n <= 4 with m = 2 (4), n <= 3 with m = 3 (3): what the issue's list of shapes says
    assert fits == 13
    assert all(kldiv(choice, n, 1, 2) == (nc.LDS41 if n == 4 else nc.LDS00) for n in range(1, 7)) and kldiv(choice, 7, 1, 2) == nc.DIRECT


def test_fcov_thresholds_and_the_whole_box(choice):
    for n in range(1, 33):
        for m in range(1, 9):
            for N in (1, 8, 16, 17, 24):
                for al in (0, 1):
                    assert fcov(choice, n, m, N, 3, al) == _inline_fcov(n, m, N, 3, al, 1, None, None), (n, m, N, al)
    assert fcov(choice, 4, 1, 16, 6144) == nc.Q4L and fcov(choice, 4, 1, 16, 6145) == nc.Q4_1
    assert fcov(choice, 4, 1, 8) == nc.Q4_1 and fcov(choice, 4, 1, 16) == nc.Q4L and fcov(choice, 4, 1, 20) == nc.Q4_1
    assert fcov(choice, 4, 2, 16) == nc.Q4_2 and fcov(choice, 4, 3, 16) == nc.GENERIC and fcov(choice, 5, 1, 16) == nc.GENERIC
    assert fcov(choice, 4, 1, 16, q4l="1") == nc.Q4L and fcov(choice, 4, 1, 16, q4="1") == nc.Q4L


def test_shapes_without_a_kernel_and_the_wide_switch(choice):
    for f in (lambda *a, **k: fcov(choice, *a, **k), lambda *a, **k: kldiv(choice, *a, **k)):
        wide = "fcov_wide_kernel" if f(4, 1, 16, gps_wide="1").startswith("fcov") else "kl_div_wide_kernel"
        assert f(33, 1, 5) == "none" and f(4, 9, 5) == "none" and f(0, 1, 5) == "none" and f(4, 0, 5) == "none"
        assert f(33, 1, 5, wide=1) == wide and f(64, 32, 5, wide=1) == wide and f(65, 1, 5, wide=1) == "none" and f(4, 33, 5, wide=1) == "none"
        assert f(4, 1, 0) == "none" and f(4, 1, 5, 0) == "none" and f(33, 1, 0, wide=1) == "none"
        assert f(4, 1, 16, gps_wide="0") != wide and f(33, 1, 5, gps_wide="1") == "none"
