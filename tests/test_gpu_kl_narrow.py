"""The n <= 32, m <= 8 KL kernels of csrc/kl.hip over their whole box, against the long double reference (tests/kl_reference.py):
kl_terms_kernel; fcov_kernel, fcov_q4_kernel<1>, <2>, fcov_q4l_kernel; kl_div_kernel, kl_div_lds_kernel<4,1>, <4,2>, <0,0>.
Cases, expected kernels and references come from tests/kl_narrow_cases.py; every case asserts through ddp_last_kernel(h, 5) / (h, 6)
that the kernel it checks is the one that ran.

Tolerance, with d_gpu = relerr(kernel, long double) and d_orc = relerr(C oracle, long double) on the same case (conftest.relerr):
d_gpu < RTOL = 1e-8, the project's bar, and d_gpu <= max(8 d_orc, L 2^-52) with L the longest dot product: n + m for ∇kl and
kl_div_wiki, N (2n + m) for the covariance chain.  Kernel and oracle evaluate the same associations and differ in summation order and
FMA contraction, which moves a dot product's error within its L eps bound, not by orders of magnitude: three bits leave room for that,
a kernel that loses digits the oracle keeps does not fit.  klmean, the mean over time of kldiv, is held to the same bound.
Two runs of a kernel agree bit for bit; two kernels of one shape agree to 1e-11 (fcov_q4l and fcov_q4 bit for bit)."""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import relerr
import kl_narrow_cases as nc
from kl_reference import need_longdouble

pytestmark = pytest.mark.gpu
RTOL = nc.RTOL
TWO_WAYS = 1e-11
SWITCHES = ("DDP_KL_LDS", "DDP_FCOV_Q4", "DDP_FCOV_Q4L")


@pytest.fixture
def ddp(monkeypatch):
    need_longdouble()
    import ddp_amd
    import ddp_amd.kl  # noqa: F401
    for k in [k for k in os.environ if k.startswith("DDP_") and not k.startswith("DDP_AMD_")]:      # (kernel switches, not the loader's)
        monkeypatch.delenv(k)
    ddp_amd.default_handle().raw                              # (re-reads the DDP_* switches when they changed)
    yield ddp_amd
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    ddp_amd.default_handle().raw


def _switch(ddp, monkeypatch, **kw):
    """DDP_<name> = value (None: unset); Handle.raw re-reads the switches at the next call"""
    for k, v in kw.items():
        if v is None:
            monkeypatch.delenv("DDP_" + k, raising=False)
        else:
            monkeypatch.setenv("DDP_" + k, v)
    ddp.default_handle().raw


def _judge(kernel, what, d_gpu, d_orc, lim):
    print("RATIO %-24s %-28s d_gpu %.3e  d_orc %.3e  d_gpu/d_orc %s  bound %.3e" %
          (kernel, what, d_gpu, d_orc, "%.2f" % (d_gpu / d_orc) if d_orc > 0 else "-", lim))
    assert d_gpu < RTOL, (kernel, what, d_gpu)
    assert d_gpu <= lim, (kernel, what, "d_gpu %.3e above max(8 d_orc, L eps) = %.3e (d_orc %.3e)" % (d_gpu, lim, d_orc))


def _prev(ddp, c):
    return ddp.GaussianPolicy(c["N"], c["n"], c["m"], c["Kp"], c["kp"], c["Sp"], c["Sip"])


def _new(ddp, c):
    return ddp.GaussianPolicy(c["N"], c["n"], c["m"], c["Kn"], c["kn"], c["Sn"], c["Sn"])         # (Σi of the new policy is never read)


# 1. ------------------------------------------------------------------------------------------------------------------- ∇kl
@pytest.mark.parametrize("r", nc.TERMS, ids=nc.kid)
def test_kl_terms_matches_long_double(ddp, r):
    n, m, N, B = r["n"], r["m"], r["N"], r["B"]
    c, want = nc.case(n, m, N, B), nc.ref_terms(n, m, N, B)
    got = ddp.kl.grad_kl(_prev(ddp, c))
    d_gpu = max(relerr(a[..., b], w[..., b]) for a, w in zip(got, want) for b in range(B))
    d_orc = nc.oracle_dist("terms", n, m, N, B)
    _judge("kl_terms_kernel", nc.kid(r), d_gpu, d_orc, nc.bound("terms", n, m, N, d_orc))
    assert np.array_equal(got[4], c["Sip"])                                              # cuu = Σi, a copy
    for a, b_ in zip(got, ddp.kl.grad_kl(_prev(ddp, c))):
        assert np.array_equal(a, b_)


# 2. ------------------------------------------------------------------------------------------------------------------- forward_covariance
def _fcov(ddp, c, shared):
    kl = ddp.kl
    sig = kl.forward_covariance(kl.Model(c["fx"][..., 0] if shared else c["fx"], None, c["R1"]), None, None, _new(ddp, c))
    return sig, ddp.default_handle().last_kernel(5)


def _fcov_misaligned(ddp, c, shared):
    """ddp_forward_covariance_f64_dev with K 8 bytes into its device buffer (every other operand at the start of its own)"""
    from ddp_amd import _lib
    h, L = ddp.default_handle(), _lib.lib()
    n, m, N, B = c["n"], c["m"], c["N"], c["B"]
    bufs = []

    def put(a, off=0):
        a = np.asfortranarray(a, dtype=np.float64)
        p = h.malloc(a.nbytes + 16)
        bufs.append(p)
        _lib.check(L.ddp_memcpy_h2d(h.raw, C.c_void_p(p.value + off), a.ctypes.data_as(C.c_void_p), C.c_size_t(a.nbytes)))
        return p.value + off
    try:
        fx = put(c["fx"][..., 0] if shared else c["fx"])
        R1, K, Sg = put(c["R1"]), put(c["Kn"], 8), put(c["Sn"])
        assert K % 16 == 8 and fx % 16 == 0 and Sg % 16 == 0
        shape = (n + m, n + m, N, B)
        out = put(np.full(shape, np.nan))
        _lib.check(L.ddp_forward_covariance_f64_dev(h.raw, n, m, N, B, C.c_void_p(fx), int(not shared), C.c_void_p(R1), C.c_void_p(K),
                                                    C.c_void_p(Sg), C.c_void_p(out)))
        h.sync()
        return h.to_host(C.c_void_p(out), shape), h.last_kernel(5)
    finally:
        for p in bufs:
            h.free(p)


def _fcov_dist(sig, want, B):
    return max(relerr(sig[..., b], want[..., b]) for b in range(B))


@pytest.mark.parametrize("r", nc.FCOV, ids=nc.kid)
def test_forward_covariance_matches_long_double(ddp, monkeypatch, r):
    n, m, N, B = r["n"], r["m"], r["N"], r["B"]
    c = nc.case(n, m, N, B)
    run = _fcov_misaligned if r["mis"] else _fcov
    for shared in (False, True):                              # the model per trajectory, and one model for the batch
        tag = nc.kid(r) + ("-shared" if shared else "-own")
        _switch(ddp, monkeypatch, FCOV_Q4=r["env"][0], FCOV_Q4L=r["env"][1])
        sig, kern = run(ddp, c, shared)
        assert kern == r["want"], (kern, r)
        want = nc.ref_fcov(n, m, N, B, shared)
        d_orc = nc.oracle_dist("fcov_shared" if shared else "fcov", n, m, N, B)
        lim = nc.bound("fcov", n, m, N, d_orc)
        _judge(kern, tag, _fcov_dist(sig, want, B), d_orc, lim)
        # the last step has no policy block: its rows and columns beyond n are exactly 0
        assert not sig[n:, :, N - 1, :].any() and not sig[:, n:, N - 1, :].any()
        again, kern2 = run(ddp, c, shared)
        assert kern2 == kern and np.array_equal(sig, again)                              # fixed-order sums: the same bits
        if kern == nc.Q4L:                                   # the step-by-step kernel does the same products in the same order
            _switch(ddp, monkeypatch, FCOV_Q4L="0")
            step, k3 = run(ddp, c, shared)
            assert k3 == nc.Q4_1 and np.array_equal(step, sig)
            _judge(k3, tag, _fcov_dist(step, want, B), d_orc, lim)
        if kern in (nc.Q4L, nc.Q4_1, nc.Q4_2):               # one shape, two ways: the run-time-sized kernel
            _switch(ddp, monkeypatch, FCOV_Q4="0", FCOV_Q4L=None)
            gen, k4 = run(ddp, c, shared)
            assert k4 == nc.GENERIC
            _judge(k4, tag, _fcov_dist(gen, want, B), d_orc, lim)
            assert relerr(sig, gen) < TWO_WAYS, relerr(sig, gen)
            assert not gen[n:, :, N - 1, :].any() and not gen[:, n:, N - 1, :].any()


# 3. ------------------------------------------------------------------------------------------------------------------- kl_div_wiki
def _kl_div(ddp, c):
    kld, mean = ddp.kl._kl_div(c["xnew"], c["xold"], c["sig"], _new(ddp, c), _prev(ddp, c), None)
    return kld, mean, ddp.default_handle().last_kernel(6)


def _kl_dist(kld, mean, want, wmean, B):
    d = max(relerr(kld[:, b], want[:, b], 0) for b in range(B))
    dm = max(abs(mean[b] - float(wmean[b])) / max(float(wmean[b]), 1e-300) for b in range(B))
    return d, dm


@pytest.mark.parametrize("r", nc.KLDIV, ids=nc.kid)
def test_kl_div_matches_long_double(ddp, monkeypatch, r):
    n, m, N, B = r["n"], r["m"], r["N"], r["B"]
    c = nc.case(n, m, N, B)
    want, wmean = nc.ref_kl_div(n, m, N, B)
    d_orc = nc.oracle_dist("kl_div", n, m, N, B)
    lim = nc.bound("kl_div", n, m, N, d_orc)
    _switch(ddp, monkeypatch, KL_LDS=r["env"])
    kld, mean, kern = _kl_div(ddp, c)
    assert kern == r["want"], (kern, r)
    d, dm = _kl_dist(kld, mean, want, wmean, B)
    _judge(kern, nc.kid(r), d, d_orc, lim)
    _judge(kern, nc.kid(r) + " mean", dm, d_orc, lim)
    kld2, mean2, _ = _kl_div(ddp, c)
    assert np.array_equal(kld, kld2) and np.array_equal(mean, mean2)
    if kern != nc.DIRECT:                                     # one shape, two ways: the direct kernel
        _switch(ddp, monkeypatch, KL_LDS="0")
        kd, md, k2 = _kl_div(ddp, c)
        assert k2 == nc.DIRECT
        d, dm = _kl_dist(kd, md, want, wmean, B)
        _judge(k2, nc.kid(r), d, d_orc, lim)
        _judge(k2, nc.kid(r) + " mean", dm, d_orc, lim)
        assert relerr(kld, kd, 0) < TWO_WAYS and np.max(np.abs(mean - md) / np.maximum(md, 1e-300)) < TWO_WAYS


# 4. ------------------------------------------------------------------------------------------------------------------- designed inputs
FAMILY = {(4, 1): nc.LDS41, (4, 2): nc.LDS42, (3, 3): nc.LDS00, (5, 2): nc.DIRECT}


@pytest.mark.parametrize("n,m,kind", nc.designed_ids())
def test_designed_inputs_give_the_exact_outcomes(ddp, monkeypatch, n, m, kind):
    import kl_reference as ref
    c = nc.designed(n, m, kind)
    wk, wm, _ = ref.kl_div_wiki(*[c[k_] for k_ in nc.KL_ARGS])
    wk, wm = wk.astype(float), wm.astype(float)
    for lds in (None, "0"):                                   # the shape's own kernel, and the direct one
        _switch(ddp, monkeypatch, KL_LDS=lds)
        kld, mean, kern = _kl_div(ddp, c)
        assert kern == (nc.DIRECT if lds == "0" else FAMILY[(n, m)])
        nc.check_designed(n, m, kind, kld, mean)
        assert np.array_equal(np.isnan(kld), np.isnan(wk)) and np.array_equal(np.isposinf(kld), np.isposinf(wk)), kern
        assert np.array_equal(np.isnan(mean), np.isnan(wm)) and np.array_equal(np.isposinf(mean), np.isposinf(wm)), kern
        if kind == "inverse":
            continue
        assert np.array_equal(kld == 0, wk == 0), kern
        fin = np.isfinite(wk)
        assert np.max(np.abs(kld[fin] - wk[fin])) <= RTOL * max(wk[fin].max(), 1e-300), kern
        fm = np.isfinite(wm)
        assert np.all(np.abs(mean[fm] - wm[fm]) <= RTOL * np.abs(wm[fm])), kern


# 5. ------------------------------------------------------------------------------------------------------------------- whole loops
@pytest.mark.parametrize("n,m,T,seed", nc.LOOPS)
def test_lq_loop_on_the_run_time_sized_lds_kernel_matches_oracle(ddp, n, m, T, seed):
    c = nc.loop_case(n, m, T, seed)
    B = c["B"]
    prev = ddp.GaussianPolicy(T, n, m, np.zeros((m, n, T, B)), c["u"].copy(), c["eye"], c["eye"].copy())
    xo, uo, pol, Vx, Vxx, cost, tr = ddp.kl.iLQGkl(ddp.LQProblem(c["A"], c["Bm"], c["Q"], c["R"]), c["x"], prev,
                                                   ddp.kl.Model(c["fx"], c["fu"], c["R1"]), kl_step=nc.LOOP_KL_STEP,
                                                   max_iter=nc.LOOP_MAX_ITER, cost=c["cost0"])
    h = ddp.default_handle()
    assert h.last_kernel(6) == nc.LDS00 and h.last_kernel(5) == nc.GENERIC and h.last_kernel(7) == ""      # (slots 0..6)
    assert np.array_equal(pol.k, uo)                                  # traj_new.k = copy(u)  (iLQGkl.jl:239)
    for b, (xr, ur, polr, vx, vxx, cr, info) in enumerate(nc.loop_reference(n, m, T, seed)):
        got = (tr["status"][b], tr["iter"][b], tr["n_backpass"][b])
        print("(%d, %d, %d) trajectory %d: outcome %s, oracle %s" % (n, m, T, b, got, nc.outcome(info)))
        assert got == nc.outcome(info), b
        for a, r_, nm in ((tr["η"][:, b], info["eta"], "η"), (xo[..., b], xr, "x"), (uo[..., b], ur, "u"), (pol.K[..., b], polr["K"], "K"),
                          (pol.Σ[..., b], polr["S"], "Σ"), (Vxx[..., b], vxx, "Vxx")):
            e = relerr(a, r_, 0) if nm == "η" else relerr(a, r_)
            print("    %s %.2e" % (nm, e))
            assert e < RTOL, (b, nm, e)
        assert relerr(cost[:, b], cr, 0) < RTOL, b
