"""The wide KL path on the GPU (kl.*(wide=True), ddp_kl_set_wide: n <= 64, m <= 32): back_pass_gps on the GPS instantiation of
back_pass_wide_kernel, ∇kl / forward_covariance / kl_div_wiki on the kernels of kl_wide.hip, the iLQGkl loop of LQ and user problems.
Tolerance 1e-8 relative per time step (conftest.relerr) against the C oracle; cases and references from tests/kl_wide_cases.py."""
import ctypes as C

import numpy as np
import pytest

from conftest import relerr
import kl_wide_cases as kc

pytestmark = pytest.mark.gpu
RTOL = kc.RTOL
WIDE = "back_pass_gps_wide"


@pytest.fixture(scope="module")
def ddp():
    import ddp_amd
    import ddp_amd.kl  # noqa: F401
    ddp_amd.default_handle()
    return ddp_amd


@pytest.fixture
def gps_wide(ddp, monkeypatch):
    def set_(v):
        if v is None:
            monkeypatch.delenv("DDP_GPS_WIDE", raising=False)
        else:
            monkeypatch.setenv("DDP_GPS_WIDE", v)
        ddp.default_handle().raw                              # (re-reads the DDP_* switches when they changed)
    yield set_
    monkeypatch.delenv("DDP_GPS_WIDE", raising=False)
    ddp.default_handle().raw


def _last(ddp):
    return ddp.default_handle().last_kernel(0)


def _prev(ddp, c):
    return ddp.GaussianPolicy(c["N"], c["n"], c["m"], c["Kp"], c["kp"], c["Sp"], c["Sip"])


def _gps(ddp, c, o, terms, **kw):
    return ddp.kl.back_pass_gps(c["cx"], c["cu"], o["cxx"], o["cxu"], o["cuu"], o["fx"], o["fu"], o["lims"], c["x"], c["u"], (terms, o["etab"]), **kw)


def _check_gps(got, ref, b, tag):
    div, pol, Vx, Vxx, dV = got
    assert div[b] == ref["diverge"], (tag, b, div[b], ref["diverge"])
    for a, key in ((pol.K, "K"), (pol.k, "k"), (pol.Σ, "Quui"), (pol.Σi, "Quu"), (Vx, "Vx"), (Vxx, "Vxx")):
        e = relerr(a[..., b], ref[key])
        print("%s trajectory %d %s: %.2e" % (tag, b, key, e))
        assert e < RTOL, (tag, b, key, e)
    assert relerr(dV[:, b], ref["dV"], 0) < RTOL, (tag, b)


# 1. --------------------------------------------------------------------------------------------- back_pass_gps against the oracle
@pytest.mark.parametrize("n,m", kc.SHAPES)
def test_back_pass_gps_wide_matches_oracle(ddp, gps_wide, n, m):
    gps_wide(None)
    c = kc.single_pass(n, m)
    terms = ddp.kl.grad_kl(_prev(ddp, c), wide=True)
    seen_div = False
    for ci, cfg in enumerate(kc.CONFIGS):
        got = _gps(ddp, c, kc.operands(c, cfg), terms, wide=True)
        assert _last(ddp) == WIDE
        assert np.array_equal(got[3], np.transpose(got[3], (1, 0, 2, 3)))                # Vxx exactly symmetric
        for b, ref in enumerate(kc.gps_reference(n, m, ci)):
            _check_gps(got, ref, b, "(%d, %d) configuration %d" % (n, m, ci))
            seen_div |= ref["diverge"] > 0
            if ref["diverge"] > 0:                           # Quui of the steps not reached: the zeros the entry point writes
                assert not got[1].Σ[:, :, : ref["diverge"], b].any()
    assert seen_div


# 2. --------------------------------------------------------------------------------------------- three ways at small shapes
@pytest.mark.parametrize("n,m", kc.SMALL)
def test_wide_kernels_at_small_shapes_match_default_kernels_and_oracle(ddp, gps_wide, n, m):
    c = kc.single_pass(n, m)
    prev = _prev(ddp, c)
    gps_wide(None)
    terms0 = ddp.kl.grad_kl(prev)
    base = [_gps(ddp, c, kc.operands(c, cfg), terms0) for cfg in kc.CONFIGS]
    assert _last(ddp) != WIDE
    gps_wide("1")
    terms1 = ddp.kl.grad_kl(prev)
    for a, b_ in zip(terms1, terms0):
        assert relerr(a, b_) < 1e-10
    for ci, cfg in enumerate(kc.CONFIGS):
        got = _gps(ddp, c, kc.operands(c, cfg), terms1)
        assert _last(ddp) == WIDE
        assert np.array_equal(got[0], base[ci][0])
        for a, b_, nm in ((got[1].K, base[ci][1].K, "K"), (got[1].k, base[ci][1].k, "k"), (got[1].Σ, base[ci][1].Σ, "Quui"),
                          (got[1].Σi, base[ci][1].Σi, "Quu"), (got[2], base[ci][2], "Vx"), (got[3], base[ci][3], "Vxx"), (got[4], base[ci][4], "dV")):
            assert relerr(a, b_) < 1e-10, (ci, nm, relerr(a, b_))
        for b, ref in enumerate(kc.gps_reference(n, m, ci)):
            _check_gps(got, ref, b, "(%d, %d) configuration %d" % (n, m, ci))


# 3. --------------------------------------------------------------------------------------------- the three KL kernels
def _kl_inputs(c):
    """a new policy (the oracle's back pass of configuration 0), a per-trajectory model and a moved trajectory"""
    n, m, N, B = c["n"], c["m"], c["N"], c["B"]
    ref = kc.gps_reference(n, m, 0)
    st = lambda key: np.stack([r[key] for r in ref], -1)                                 # noqa: E731
    xnew = c["x"] + 0.1 * np.cos(np.arange(c["x"].size).reshape(c["x"].shape))
    return st("K"), st("k"), st("Quui"), st("Quu"), 0.01 * np.eye(n), xnew


def _kl_three(ddp, c, **kw):
    kl = ddp.kl
    K, k, S, Si, R1, xnew = _kl_inputs(c)
    prev = _prev(ddp, c)
    new = ddp.GaussianPolicy(c["N"], c["n"], c["m"], K, k, S, Si)
    terms = kl.grad_kl(prev, **kw)
    sig = kl.forward_covariance(kl.Model(c["fx"], None, R1), c["x"], c["u"], new, **kw)
    sig1 = kl.forward_covariance(kl.Model(c["fx"][..., 1], None, R1), c["x"], c["u"], new, **kw)       # one model for the batch
    kld, mean = kl._kl_div(xnew, c["x"], sig, new, prev, None, **kw)
    return terms, sig, sig1, kld, mean


def _check_kl_three(ddp, c, out):
    from oracle import oracle_ctypes as oc
    terms, sig, sig1, kld, mean = out
    K, k, S, Si, R1, xnew = _kl_inputs(c)
    n, N = c["n"], c["N"]
    for b in range(c["B"]):
        for a, r, nm in zip(terms, oc.kl_terms(c["Kp"][..., b], c["kp"][..., b], c["Sip"][..., b]), ("cx", "cu", "cxx", "cxu", "cuu")):
            assert relerr(a[..., b], r) < RTOL, (nm, b, relerr(a[..., b], r))
        assert relerr(sig[..., b], oc.forward_covariance(c["fx"][..., b], R1, K[..., b], S[..., b])) < RTOL, b
        assert relerr(sig1[..., b], oc.forward_covariance(c["fx"][..., 1], R1, K[..., b], S[..., b])) < RTOL, b
        assert not sig[n:, :, N - 1, b].any() and not sig[:, n:, N - 1, b].any()          # last step: no policy block
        kr = oc.kl_div_wiki(xnew[..., b], c["x"][..., b], sig[..., b], dict(K=K[..., b], k=k[..., b], S=S[..., b]),
                            dict(K=c["Kp"][..., b], k=c["kp"][..., b], S=c["Sp"][..., b], Si=c["Sip"][..., b]))
        assert np.all(np.isfinite(kr)) and relerr(kld[:, b], kr) < RTOL, (b, relerr(kld[:, b], kr))
        assert abs(mean[b] - kr.mean()) <= RTOL * abs(kr.mean())


@pytest.mark.parametrize("n,m", kc.SHAPES + kc.SMALL)
def test_kl_kernels_match_oracle_and_repeat_bit_for_bit(ddp, gps_wide, n, m):
    small = (n, m) in kc.SMALL
    gps_wide("1" if small else None)                          # small shapes reach the wide kernels through DDP_GPS_WIDE=1
    kw = {} if small else dict(wide=True)
    c = kc.single_pass(n, m)
    out = _kl_three(ddp, c, **kw)
    _check_kl_three(ddp, c, out)
    again = _kl_three(ddp, c, **kw)
    for a, b_ in zip(out[0] + out[1:], again[0] + again[1:]):
        assert np.array_equal(a, b_)                          # no atomics, fixed-order sums: the same bits
    if small:                                                 # and the default kernels of these shapes
        gps_wide(None)
        base = _kl_three(ddp, c)
        for a, b_ in zip(out[0] + out[1:], base[0] + base[1:]):
            assert relerr(a, b_) < 1e-10


@pytest.mark.parametrize("n,m", [(5, 9), (34, 17), (64, 32)])
def test_kl_div_identical_policies_and_negative_determinant(ddp, gps_wide, n, m):
    from oracle import oracle_ctypes as oc
    gps_wide(None)
    kl = ddp.kl
    c = kc.single_pass(n, m)
    N, B = c["N"], c["B"]
    sig = kl.forward_covariance(kl.Model(c["fx"], None, 0.01 * np.eye(n)), c["x"], c["u"], _prev(ddp, c), wide=True)
    # identical policies: with Σ = Σi = I every term is exact (tr(I I) = m, both logdets 0): the divergence is 0, not about 0
    eye = np.tile(np.eye(m)[:, :, None, None], (1, 1, N, B))
    same = ddp.GaussianPolicy(N, n, m, c["Kp"], c["kp"], eye, eye.copy())
    kld, mean = kl._kl_div(c["x"], c["x"], sig, same, same, None, wide=True)
    assert not kld.any() and not mean.any()
    # Σ = inv(Σi) to rounding: tr(Σi Σ) - m is m · eps · cond(Σi) at most (cond < 1e2 here), nothing else is left
    prev = _prev(ddp, c)
    kld, mean = kl._kl_div(c["x"], c["x"], sig, prev, prev, None, wide=True)
    assert np.all(kld >= 0) and np.all(kld <= 32 * 2.3e-16 * 1e2)
    # a covariance of the new policy with negative determinant at one step of trajectory 1: logdet throws (klutils.jl:95-99)
    Sn = c["Sp"].copy()
    Sn[:, :, 3, 1] = np.diag([-1.0] + [1.0] * (m - 1))
    new = ddp.GaussianPolicy(N, n, m, c["Kp"], c["kp"], Sn, c["Sip"])
    kld, mean = kl._kl_div(c["x"], c["x"], sig, new, prev, None, wide=True)
    assert np.isinf(mean[1]) and mean[1] > 0 and np.all(np.isfinite(mean[[0, 2]])) and np.all(np.isfinite(kld))
    one = lambda p, b: ddp.GaussianPolicy(N, n, m, p.K[..., b], p.k[..., b], p.Σ[..., b], p.Σi[..., b])       # noqa: E731
    assert kl.kl_div_wiki(c["x"][..., 1], c["x"][..., 1], sig[..., 1], one(new, 1), one(prev, 1), wide=True) == np.inf
    assert oc.kl_div_wiki(c["x"][..., 1], c["x"][..., 1], sig[..., 1], dict(K=new.K[..., 1], k=new.k[..., 1], S=Sn[..., 1]),
                          dict(K=prev.K[..., 1], k=prev.k[..., 1], S=prev.Σ[..., 1], Si=prev.Σi[..., 1])) == np.inf
    # a NaN in xnew at one step of trajectory 1: max(0, v) hands it on (klutils.jl:98) — that step and that mean are NaN, nothing else moves
    xn = c["x"] + 0.1 * np.cos(np.arange(c["x"].size).reshape(c["x"].shape))
    moved = ddp.GaussianPolicy(N, n, m, 1.5 * c["Kp"], c["kp"] + 0.1, c["Sp"], c["Sip"])
    kld0, mean0 = kl._kl_div(xn, c["x"], sig, moved, prev, None, wide=True)
    assert np.all(np.isfinite(kld0)) and np.all(kld0[3] > 0)
    xn[0, 3, 1] = np.nan
    kld, mean = kl._kl_div(xn, c["x"], sig, moved, prev, None, wide=True)
    hit = np.zeros((N, B), bool); hit[3, 1] = True
    assert np.array_equal(np.isnan(kld), hit) and np.array_equal(kld[~hit], kld0[~hit])
    assert np.isnan(mean[1]) and np.array_equal(mean[[0, 2]], mean0[[0, 2]])
    got = oc.kl_div_wiki(xn[..., 1], c["x"][..., 1], sig[..., 1], dict(K=moved.K[..., 1], k=moved.k[..., 1], S=moved.Σ[..., 1]),
                         dict(K=prev.K[..., 1], k=prev.k[..., 1], S=prev.Σ[..., 1], Si=prev.Σi[..., 1]))
    assert np.array_equal(np.isnan(got), hit[:, 1])


# 4. --------------------------------------------------------------------------------------------- active mask (device entry)
SENT = [0x7FF8000000000A00 + i for i in range(8)]            # one quiet-NaN bit pattern per output


@pytest.mark.parametrize("n,m,lims", [(34, 17, True), (64, 32, False)])
def test_back_pass_gps_dev_active_mask(ddp, gps_wide, n, m, lims):
    """inactive trajectories keep the sentinel bits of K, k, Quu, Vx, Vxx, dV and diverge (their Quui holds the zeros the entry point
    writes for every trajectory before the launch); active ones are the bits of the unmasked call"""
    from ddp_amd import _lib
    gps_wide(None)
    h, L = ddp.default_handle(), _lib.lib()
    c = kc.single_pass(n, m)
    o = kc.operands(c, kc.CONFIGS[3 if lims else 0])
    N, B = c["N"], c["B"]
    terms = ddp.kl.grad_kl(_prev(ddp, c), wide=True)
    eta = np.asfortranarray(o["etab"][1])
    bufs = []

    def alloc(nbytes):
        p = h.malloc(nbytes + 16)
        bufs.append(p)
        return p.value

    def put(a, dtype=np.float64):
        a = np.asfortranarray(a, dtype=dtype)
        p = alloc(a.nbytes)
        _lib.check(L.ddp_memcpy_h2d(h.raw, C.c_void_p(p), a.ctypes.data_as(C.c_void_p), C.c_size_t(a.nbytes)))
        return p
    shapes = ((m, n, N, B), (m, N, B), (m, m, N, B), (m, m, N, B), (n, N, B), (n, n, N, B), (2, B), ((B + 1) // 2,))
    names = ("K", "k", "Quu", "Quui", "Vx", "Vxx", "dV", "diverge")
    try:
        ins = [put(a) for a in (c["cx"], c["cu"], o["cxx"], o["cxu"], o["cuu"], o["fx"], o["fu"])]
        kt = [put(a) for a in terms] + [put(eta)]
        t = _lib.KLCostTerms(*kt, int(eta.ndim == 2))
        dl, du = (put(o["lims"]), put(c["u"])) if lims else (None, None)
        desc = _lib.BPDesc(n, m, N, B, 1, int(o["fx"].ndim == 4), 1, int(o["cxx"].ndim == 4), 1, int(lims))
        h.set_kl_wide(True)

        def run(active):
            outs = [put(np.full(int(np.prod(s)), v, np.uint64), np.uint64) for s, v in zip(shapes, SENT)]
            act = None if active is None else put(np.ascontiguousarray(active, np.int32), np.int32)
            _lib.check(L.ddp_back_pass_gps_f64_dev(h.raw, C.byref(desc), *[C.c_void_p(a) for a in ins], C.byref(t), C.c_void_p(dl), C.c_void_p(du),
                                                   C.c_void_p(act), *[C.c_void_p(a) for a in outs]))
            h.sync()
            assert h.last_kernel(0) == WIDE
            return {nm: np.ascontiguousarray(h.to_host(C.c_void_p(p), s)).view(np.uint64) for nm, p, s in zip(names, outs, shapes)}
        full = run(None)
        active = np.array([1, 0, 1], np.int32)
        part = run(active)
        for i, nm in enumerate(names[:7]):
            for b in range(B):
                if active[b]:
                    assert np.array_equal(part[nm][..., b], full[nm][..., b]), (nm, b)
                elif nm == "Quui":
                    assert not part[nm][..., b].any(), b
                else:
                    assert np.all(part[nm][..., b] == SENT[i]), (nm, b, "of an inactive trajectory was written")
        dv = lambda r: r["diverge"].view(np.int32)[:B]                                   # noqa: E731
        sent = np.full(1, SENT[7], np.uint64).view(np.int32)[np.arange(B) % 2]           # the two halves of the sentinel word
        assert np.array_equal(dv(part)[active == 1], dv(full)[active == 1]) and np.array_equal(dv(part)[active == 0], sent[active == 0])
    finally:
        h.set_kl_wide(False)
        for p in bufs:
            h.free(p)


# 5. --------------------------------------------------------------------------------------------- whole loops, LQProblem
def _loop_args(ddp, c):
    n, m, T, B = c["n"], c["m"], c["T"], c["B"]
    prev = ddp.GaussianPolicy(T, n, m, np.zeros((m, n, T, B)), c["u"].copy(), c["eye"], c["eye"].copy())
    return prev, dict(kl_step=kc.LOOP_KL_STEP, max_iter=kc.LOOP_MAX_ITER, cost=c["cost0"], lims=c["lims"], wide=True)


_registered = {}


def _registered_loop(ddp, case):
    if case not in _registered:
        c = kc.loop_case(*case)
        prev, kw = _loop_args(ddp, c)
        _registered[case] = ddp.kl.iLQGkl(ddp.LQProblem(c["A"], c["Bm"], c["Q"], c["R"]), c["x"], prev, ddp.kl.Model(c["fx"], c["fu"], c["R1"]), **kw)
    return _registered[case]


@pytest.mark.parametrize("n,m,T,lims", kc.LOOPS)
def test_lq_loop_matches_oracle(ddp, gps_wide, n, m, T, lims):
    gps_wide(None)
    c = kc.loop_case(n, m, T, lims)
    xo, uo, pol, Vx, Vxx, cost, tr = _registered_loop(ddp, (n, m, T, lims))
    assert _last(ddp) == WIDE
    assert np.array_equal(pol.k, uo)                                  # traj_new.k = copy(u)  (iLQGkl.jl:239)
    for b, (xr, ur, polr, vx, vxx, cr, info) in enumerate(kc.loop_reference(n, m, T, lims)):
        got = (tr["status"][b], tr["iter"][b], tr["n_backpass"][b])
        print("(%d, %d, %d) limits %s trajectory %d: outcome %s, oracle %s" % (n, m, T, lims, b, got, kc.outcome(info)))
        assert got == kc.outcome(info), b
        for a, r, nm in ((tr["η"][:, b], info["eta"], "η"), (xo[..., b], xr, "x"), (uo[..., b], ur, "u"), (pol.K[..., b], polr["K"], "K"),
                         (pol.Σ[..., b], polr["S"], "Σ"), (Vxx[..., b], vxx, "Vxx")):
            e = relerr(a, r, 0) if nm == "η" else relerr(a, r)
            print("    %s %.2e" % (nm, e))
            assert e < RTOL, (b, nm, e)
        assert relerr(cost[:, b], cr, 0) < RTOL, b


# 6. --------------------------------------------------------------------------------------------- user problems
@pytest.mark.parametrize("lims", [False, True])
@pytest.mark.parametrize("n,m,T", kc.USER_LOOPS)
def test_user_wave_loop_matches_registered_and_host_loop(ddp, gps_wide, monkeypatch, n, m, T, lims):
    from test_gpu_user_problem import lq_params
    gps_wide(None)
    kl = ddp.kl
    c = kc.loop_case(n, m, T, lims)
    prev, kw = _loop_args(ddp, c)
    reg = _registered_loop(ddp, (n, m, T, lims))
    user = ddp.DeviceProblem(ddp.example_source("lq"), n, m, nparam=2 * n * n + n * m + m * m, wave=True)
    prm = lq_params(c["A"], c["Bm"], c["Q"], c["R"])
    dev = kl.iLQGkl(user, c["x"], prev, kl.Model(None, None, c["R1"]), params=prm, **kw)
    assert _last(ddp) == WIDE
    monkeypatch.setenv("DDP_KL_HOSTLOOP", "1")
    host = kl.iLQGkl(user, c["x"], prev, kl.Model(None, None, c["R1"]), params=prm, **kw)
    monkeypatch.delenv("DDP_KL_HOSTLOOP")
    for other, tol, tag in ((reg, RTOL, "registered"), (host, 1e-12, "host loop")):
        for k_ in ("status", "iter", "n_backpass"):
            assert np.array_equal(dev[6][k_], other[6][k_]), (tag, k_, dev[6][k_], other[6][k_])
        assert relerr(dev[6]["η"], other[6]["η"], 0) < tol, tag
        for i, nm in ((0, "x"), (1, "u"), (3, "Vx"), (4, "Vxx"), (5, "cost")):
            assert relerr(dev[i], other[i]) < tol, (tag, nm, relerr(dev[i], other[i]))
        for nm in ("K", "Σ", "Σi"):
            assert relerr(getattr(dev[2], nm), getattr(other[2], nm)) < tol, (tag, nm)


# 7. --------------------------------------------------------------------------------------------- switch handling
def test_switch_is_off_again_after_a_wide_call(ddp, gps_wide):
    gps_wide(None)
    kl = ddp.kl
    h = ddp.default_handle()
    c = kc.single_pass(5, 9)
    prev = _prev(ddp, c)
    terms = kl.grad_kl(prev, wide=True)
    _gps(ddp, c, kc.operands(c, kc.CONFIGS[0]), terms, wide=True)
    assert _last(ddp) == WIDE and h.set_kl_wide(False) is False              # the keyword put the switch back
    before = h.last_kernel(0), h.last_kernel(1), h.last_kernel(2)
    with pytest.raises(ddp.DDPError, match="back_pass_gps"):
        _gps(ddp, c, kc.operands(c, kc.CONFIGS[0]), terms)
    with pytest.raises(ddp.DDPError):
        kl.grad_kl(prev)
    lc = kc.loop_case(33, 9, 30, False)
    lprev, kw = _loop_args(ddp, lc)
    kw.pop("wide")
    with pytest.raises(ddp.DDPError, match="back_pass_gps"):
        kl.iLQGkl(ddp.LQProblem(lc["A"], lc["Bm"], lc["Q"], lc["R"]), lc["x"], lprev, kl.Model(lc["fx"], lc["fu"], lc["R1"]), **kw)
    assert (h.last_kernel(0), h.last_kernel(1), h.last_kernel(2)) == before  # nothing was launched
    # the library's own refusal (the switch of the handle is what counts there): the C entry, past the Python check
    from ddp_amd import _lib
    n, m, N, B = c["n"], c["m"], c["N"], c["B"]
    out = [np.zeros(s, order="F") for s in ((n, N, B), (m, N, B), (n, n, N, B), (m, n, N, B), (m, m, N, B))]
    rc = _lib.lib().ddp_kl_terms_f64(h.raw, n, m, N, B, *map(_lib.ptr, [_lib.f64(c["Kp"]), _lib.f64(c["kp"]), _lib.f64(c["Sip"])] + out))
    assert rc < 0 and b"ddp_kl_set_wide" in _lib.lib().ddp_last_error()


# 8. --------------------------------------------------------------------------------------------- the hook is the dispatcher
Q4, LANE, MID, GEN = "back_pass_gps_q4", "back_pass_gps_lane", "back_pass_gps_mid", "back_pass_gps"
STANDALONE, USER = 0, 2
TWO_WAYS = 1e-10                                             # two kernels of one shape (tests/test_gpu_kl.py)
# (n, m, N, η per step, switches, wide=, expected kernel): the smallest shape that reaches each branch of gps_choose, B = 2
BRANCHES = [(4, 1, 1, False, {}, False, GEN),                # below N >= 2 of q4 and lane
            (4, 1, 2, False, {}, False, Q4), (4, 1, 2, True, {}, False, LANE), (4, 2, 2, False, {}, False, LANE),
            (10, 2, 3, False, {}, False, GEN),
            (33, 2, 3, False, {}, True, WIDE), (10, 9, 3, False, {}, True, WIDE), (10, 2, 3, False, {"DDP_GPS_WIDE": "1"}, False, WIDE)]


@pytest.fixture
def switches(ddp, monkeypatch):
    names = ("DDP_GPS_WIDE", "DDP_GPS_MID", "DDP_GPS_LANE", "DDP_GPS_Q4")

    def set_(env):
        for k in names:
            if k in env:
                monkeypatch.setenv(k, env[k])
            else:
                monkeypatch.delenv(k, raising=False)
        ddp.default_handle().raw                              # (re-reads the DDP_* switches when they changed)
    set_({})
    yield set_
    set_({})


def _hook(n, m, N, B, caller, eta_tv, env, wide_on, complete=1):
    """ddp_gps_choice3 for a call with time-varying per-trajectory operands and no limits, the switches as the environment has them"""
    from ddp_amd import _lib
    f = C.CDLL(_lib.LIB_PATH).ddp_gps_choice3
    f.restype = C.c_char_p
    f.argtypes = [C.POINTER(_lib.BPDesc), C.c_int, C.c_int, C.c_int, C.c_char_p, C.c_char_p, C.c_char_p, C.c_int, C.c_char_p]
    e = lambda k: env[k].encode() if k in env else None                                  # noqa: E731
    return f(C.byref(_lib.BPDesc(n, m, N, B, 1, 1, 1, 1, 1, 0)), int(eta_tv), caller, complete, e("DDP_GPS_MID"), e("DDP_GPS_Q4"),
             e("DDP_GPS_LANE"), int(wide_on), e("DDP_GPS_WIDE")).decode()


def _flat(got):
    div, pol, Vx, Vxx, dV = got
    return dict(K=pol.K, k=pol.k, Quui=pol.Σ, Quu=pol.Σi, Vx=Vx, Vxx=Vxx, dV=dV), div


@pytest.mark.parametrize("n,m,N,eta_tv,env,wide,want", BRANCHES)
def test_hook_names_the_kernel_the_entry_point_runs(ddp, switches, n, m, N, eta_tv, env, wide, want):
    """ddp_back_pass_gps_f64 with B = 2: ddp_last_kernel(h, 0) is what ddp_gps_choice3 answers for the same facts, and the results are
    the long double reference's to 1e-8 (kl_reference.back_pass_gps; the project's bar for back_pass_gps).  Bit for bit with the
    run-time-sized kernel holds where that kernel is the one that ran, whichever way it is reached: q4, lane and wide do the same
    arithmetic in another order and cannot share its bits, so a small-box kernel that is not the run-time-sized one is held to 1e-10 of
    it, the bar tests/test_gpu_kl.py sets for two kernels of one shape.  (The reference is long double, not the C oracle of
    kl_wide_cases.gps_reference: that one is fixed to N = 12, B = 3 and is itself double arithmetic.)"""
    import kl_reference as ref
    ref.need_longdouble()
    B = 2
    c = kc.single_pass(n, m, N, B)
    cfg = (1, 1, False, eta_tv, False)
    o = kc.operands(c, cfg)
    kw = dict(wide=True) if wide else {}
    switches(env)
    terms = ddp.kl.grad_kl(_prev(ddp, c), **kw)
    got, div = _flat(_gps(ddp, c, o, terms, **kw))
    ran = _last(ddp)
    hook = _hook(n, m, N, B, STANDALONE, eta_tv, env, wide)
    print("(%d, %d) N = %d: ran %s, hook %s" % (n, m, N, ran, hook))
    assert ran == hook == want
    assert not div.any()
    for b in range(B):
        tl = ref.grad_kl(c["Kp"][..., b], c["kp"][..., b], c["Sip"][..., b])
        eb = o["etab"][1, :, b] if eta_tv else o["etab"][1, b]
        want_b = ref.back_pass_gps(c["cx"][..., b], c["cu"][..., b], o["cxx"][..., b], o["cxu"][..., b], o["cuu"][..., b], o["fx"][..., b],
                                   o["fu"][..., b], tl, eb)
        for key, a in got.items():
            e = relerr(a[..., b], want_b[key].astype(float), 0) if key == "dV" else relerr(a[..., b], want_b[key].astype(float))
            print("    trajectory %d %-4s %.2e" % (b, key, e))
            assert e < RTOL, (b, key, e)
    if n <= 32 and m <= 8:                                   # the run-time-sized kernel of the same call: DDP_GPS_LANE=0, no other switch
        switches({"DDP_GPS_LANE": "0"})
        gen, gdiv = _flat(_gps(ddp, c, o, ddp.kl.grad_kl(_prev(ddp, c))))
        assert _last(ddp) == GEN == _hook(n, m, N, B, STANDALONE, eta_tv, {"DDP_GPS_LANE": "0"}, False)
        assert np.array_equal(div, gdiv)
        for key, a in got.items():
            if want == GEN:
                assert np.array_equal(a, gen[key]), key
            else:
                assert relerr(a, gen[key]) < TWO_WAYS, (key, relerr(a, gen[key]))


def test_hook_names_the_kernel_of_the_user_loop_with_constant_hessians(ddp, switches):
    """ddp_user_ilqgkl on lq_ad with const_hessian, (10, 2), N = 3, B = 2: the mid kernel reads the [.,.,B] Hessians as they are; with
    DDP_GPS_MID=0 the run-time-sized kernel gets them repeated along time.  Both are what the hook names for the driver's call, and
    both loops are the registered problem's (1e-8, the bar of tests/test_gpu_user_kl.py), which never sees a constant Hessian"""
    from test_gpu_user_kl import _lq_setup
    from test_gpu_user_problem import lq_params
    kl = ddp.kl
    n, m, T, B = 10, 2, 3, 2
    A, Bm, Q, R, u, x, cost0, eye = _lq_setup(np.random.default_rng(8), n, m, T, B)
    prev = ddp.GaussianPolicy(T, n, m, np.zeros((m, n, T, B)), u, eye, eye.copy())
    fx, fu, R1 = np.repeat(A[:, :, None], T, 2), np.repeat(Bm[:, :, None], T, 2), 1e-4 * np.eye(n)
    kw = dict(kl_step=2e-4, max_iter=6, cost=cost0)
    switches({})
    reg = kl.iLQGkl(ddp.LQProblem(A, Bm, Q, R), x, prev, kl.Model(fx, fu, R1), **kw)
    user = ddp.DeviceProblem(ddp.example_source("lq_ad"), n, m, nparam=2 * n * n + n * m + m * m, autodiff=True, const_hessian=True)
    for env, want in (({}, MID), ({"DDP_GPS_MID": "0"}, GEN)):
        switches(env)
        got = kl.iLQGkl(user, x, prev, kl.Model(None, None, R1), params=lq_params(A, Bm, Q, R), **kw)
        ran, hook = _last(ddp), _hook(n, m, T, B, USER, False, env, False)
        print("DDP_GPS_MID %s: ran %s, hook %s" % (env.get("DDP_GPS_MID"), ran, hook))
        assert ran == hook == want
        for k_ in ("status", "iter", "n_backpass"):
            assert np.array_equal(got[6][k_], reg[6][k_]), (want, k_, got[6][k_], reg[6][k_])
        assert relerr(got[6]["η"], reg[6]["η"], 0) < RTOL, want
        for i, nm in ((0, "x"), (1, "u"), (3, "Vx"), (4, "Vxx"), (5, "cost")):
            assert relerr(got[i], reg[i]) < RTOL, (want, nm, relerr(got[i], reg[i]))
        for nm in ("K", "Σ", "Σi"):
            assert relerr(getattr(got[2], nm), getattr(reg[2], nm)) < RTOL, (want, nm)
