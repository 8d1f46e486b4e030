"""The reference the forward-rollout contract tests (tests/test_gpu_forward_contract.py) compare every kernel with: a plain NumPy
restatement of src/forward_pass.jl:9-33 for the LQ family in np.longdouble (64-bit mantissa), written from oracle/ddp_oracle.c and
oracle/np_restatement.py and vectorised over the batch and the step sizes, so that EVERY rollout of a case is compared:

    u_t = ū_t + α k_t + K_t (x̂_t − x_t)   (empty policy: u_t = ū_t);  clamp to lims when given;  then NaN entries of u_t -> 0
    x̂_{t+1} = A_t x̂_t + B_t u_t;   c_t = ½ x̂_t' Q x̂_t + ½ u_t' R u_t   (N entries: x̂_N is computed and dropped);   csum = Σ_t c_t

This module needs no GPU: it holds the reference, the seeded case generator and the rollout distance, and checks all three against the C
oracle (one rollout at a time) at the project's RTOL before any kernel is judged by them."""
import numpy as np
import pytest

from conftest import STEP_FLOOR, relerr

LD = np.longdouble
RTOL = 1e-8


def need_longdouble():
    if np.finfo(LD).eps >= 2e-16:
        pytest.skip("np.longdouble is no wider than float64 on this host (eps = %g)" % np.finfo(LD).eps)


def _dyn_mul(M, t, tv, v):
    """M_t v for M[r,c] | [r,c,N] | [r,c,B] | [r,c,N,B] and v[c,B,na]"""
    Mt = M[:, :, t] if tv else M
    return np.einsum("ij,jba->iba", Mt, v) if Mt.ndim == 2 else np.einsum("ijb,jba->iba", Mt, v)


def lq_reference(c):
    """every rollout of an LQ case in longdouble: xnew[n,N,B,na], unew[m,N,B,na], cnew[N,B,na], csum[B,na]"""
    A, Bm, Q, R, x0, u = (np.asarray(c[k], LD) for k in ("A", "Bm", "Q", "R", "x0", "u"))
    al = np.atleast_1d(np.asarray(c["alpha"], LD))
    (n, B), (m, N), na = x0.shape, u.shape[:2], len(al)
    tv = "F" in c["dyn"]
    pol = c["K"] is not None
    if pol:
        K, k, x = (np.asarray(c[k_], LD) for k_ in ("K", "k", "x"))
    lims = None if c["lims"] is None else np.asarray(c["lims"], LD)
    xs, us = np.empty((n, N, B, na), LD), np.empty((m, N, B, na), LD)
    xh = np.repeat(x0[:, :, None], na, axis=2)
    with np.errstate(invalid="ignore"):
        for t in range(N):
            xs[:, t] = xh
            ut = np.repeat(u[:, t, :, None], na, axis=2)
            if pol:
                ut = ut + k[:, t, :, None] * al[None, None, :]
                ut = ut + np.einsum("ijb,jba->iba", K[:, :, t, :], xh - x[:, t, :, None])
            if lims is not None:                                      # Base.clamp: a NaN passes through
                lo, hi = lims[:, 0, None, None], lims[:, 1, None, None]
                ut = np.where(ut > hi, hi, np.where(ut < lo, lo, ut))
            ut = np.where(np.isnan(ut), LD(0), ut)                    # inside f, in place: unew holds the zero
            us[:, t] = ut
            if t < N - 1:
                xh = _dyn_mul(A, t, tv, xh) + _dyn_mul(Bm, t, tv, ut)
    cn = 0.5 * np.sum(xs * np.einsum("ij,jtba->itba", Q, xs), axis=0) + 0.5 * np.sum(us * np.einsum("ij,jtba->itba", R, us), axis=0)
    return xs, us, cn, cn.sum(axis=0)


def clamped_share(c, unew):
    """share of the reference's own controls that sit on a bound"""
    lims = np.asarray(c["lims"], LD)
    return float(np.mean((unew == lims[:, 0, None, None, None]) | (unew == lims[:, 1, None, None, None])))


def rollout_dist(got, ref):
    """conftest.relerr of every rollout at once: got, ref [d,T,B,na] or [T,B,na] (T the time axis) -> float64 [B,na].  A NaN in `got`
    gives a NaN distance, which no `< tol` passes."""
    got, ref = np.asarray(got, LD), np.asarray(ref, LD)
    if ref.ndim == 3:
        got, ref = got[None], ref[None]
    with np.errstate(invalid="ignore"):
        e_t, s_t = np.abs(got - ref).max(axis=0), np.abs(ref).max(axis=0)
        g = np.maximum(s_t.max(axis=0), LD(1e-300))
        return np.maximum(e_t.max(axis=0) / g, (e_t / np.maximum(s_t, STEP_FLOOR * g)).max(axis=0)).astype(np.float64)


def make_lq_case(seed, n, m, N, B, alpha, dyn="", policy=True, lims=False, full=True, nan=None):
    """dyn: "" shared LTI, "F" shared LTV, "f" per-trajectory LTI, "Ff" per-trajectory LTV; lims: bounds inside the spread of the controls
    (they clamp on roughly a third of the steps); full: full symmetric Q, R (else diagonal); nan: b — a NaN in u and in k of trajectory b.
    0.99·expm(skew) dynamics and gains of 0.2·randn/sqrt(n) keep the closed loop bounded over any horizon used here."""
    import scipy.linalg as sla
    rng = np.random.default_rng(seed)
    A0 = rng.standard_normal((n, n))
    A = sla.expm(0.1 * (A0 - A0.T)) * 0.99
    Bm = 0.2 * rng.standard_normal((n, m))
    shape = ((N,) if "F" in dyn else ()) + ((B,) if "f" in dyn else ())
    if shape:
        A = np.ascontiguousarray(A.reshape(n, n, *([1] * len(shape))) * (1 + 0.02 * rng.standard_normal((1, 1) + shape)))
        Bm = np.ascontiguousarray(Bm.reshape(n, m, *([1] * len(shape))) * (1 + 0.05 * rng.standard_normal((1, 1) + shape)))
    q, r = rng.standard_normal((n, n)), rng.standard_normal((m, m))
    Q, R = 0.1 * (q @ q.T / n + 0.3 * np.eye(n)), 0.05 * (r @ r.T / m + 0.3 * np.eye(m))
    if not full:
        Q, R = np.diag(np.diag(Q)), np.diag(np.diag(R))
    c = dict(kind="lq", n=n, m=m, N=N, B=B, dyn=dyn, A=A, Bm=Bm, Q=Q, R=R, full=full, alpha=np.atleast_1d(np.asarray(alpha, float)),
             x0=rng.standard_normal((n, B)), u=0.3 * rng.standard_normal((m, N, B)), K=None, k=None, x=None, lims=None)
    if policy:
        # the nominal states: the open-loop rollout of u (rounded to fp64) off by a little, so that K (x̂ − x) is at work from step 1 on
        x = lq_reference(dict(c, alpha=np.ones(1)))[0][..., 0].astype(np.float64)
        x[:, 1:] += 0.05 * rng.standard_normal((n, N - 1, B))
        c.update(K=0.2 * rng.standard_normal((m, n, N, B)) / np.sqrt(n), k=0.1 * rng.standard_normal((m, N, B)), x=x)
    if lims:
        s = 1 + 0.1 * np.arange(m)
        c["lims"] = np.stack([-0.25 * s, 0.3 * s], 1)
    if nan is not None:
        c["u"][0, N // 2, nan] = np.nan
        if policy:
            c["k"][m - 1, min(N - 1, 1), nan] = np.nan
    return c


def oracle_rollout(po, c, b, ai):
    from oracle import oracle_ctypes as oc
    pol = None if c["K"] is None else (c["K"][..., b], c["k"][..., b])
    return oc.forward_pass(po, pol, c["x0"][:, b], c["u"][..., b], None if pol is None else c["x"][..., b], float(c["alpha"][ai]), c["lims"])


def lq_oracle_problem(c, b):
    from oracle import oracle_ctypes as oc
    A, Bm = (c[k][..., b] if "f" in c["dyn"] else c[k] for k in ("A", "Bm"))
    return oc.make_problem("lq", c["n"], c["m"], c["N"], A=A, B=Bm, Q=c["Q"], R=c["R"])


ALPHAS = np.array([1.0, 0.3, 0.0, 0.01])
CASES = [  # n, m, N, B, dyn, policy, lims, full, nan
    (10, 2, 13, 5, "", True, False, False, None), (10, 2, 9, 5, "F", True, False, False, None), (10, 2, 12, 3, "Ff", True, True, True, None),
    (10, 2, 8, 5, "f", False, True, False, None), (1, 1, 3, 5, "", True, True, True, None), (6, 3, 65, 3, "F", True, True, True, None),
    (14, 2, 17, 3, "Ff", True, False, True, 1), (13, 3, 24, 3, "", False, False, True, 0), (25, 8, 16, 3, "F", True, True, True, 2),
    (33, 1, 7, 2, "Ff", True, True, True, None), (48, 6, 11, 2, "", True, True, True, 1), (64, 8, 15, 2, "F", True, False, True, None),
    (64, 7, 1, 3, "", True, True, True, None), (3, 5, 2, 3, "f", True, True, True, None),
]


@pytest.mark.parametrize("case", CASES, ids=lambda t: "n%d_m%d_N%d_%s_%s%s%s" % (t[0], t[1], t[2], t[4] or "lti", "pol" if t[5] else "open",
                                                                                "_lims" if t[6] else "", "_nan" if t[8] is not None else ""))
def test_longdouble_reference_agrees_with_the_c_oracle(case):
    """the reference rounded to fp64 against oc.forward_pass, every rollout, conftest.relerr per time step; with limits, between a tenth
    and nine tenths of the reference's controls sit on a bound; the vectorised distance equals conftest.relerr rollout by rollout"""
    need_longdouble()
    n, m, N, B, dyn, policy, lims, full, nan = case
    c = make_lq_case(1000 * n + 10 * m + N, n, m, N, B, ALPHAS, dyn, policy, lims, full, nan)
    xs, us, cn, cs = lq_reference(c)
    assert xs.dtype == LD and cs.shape == (B, len(ALPHAS)) and cn.shape == (N, B, len(ALPHAS))
    assert np.array_equal(xs[:, 0].astype(float), np.repeat(c["x0"][:, :, None], len(ALPHAS), 2)) and np.isfinite(xs.astype(float)).all()
    if nan is not None:                                               # the NaN control reads zero, for every step size
        assert not us[0, N // 2, nan].any() and (not policy or not us[m - 1, min(N - 1, 1), nan].any())
    worst = 0.0
    xo, uo, co = np.empty(xs.shape), np.empty(us.shape), np.empty(cn.shape)
    for b in range(B):
        po = lq_oracle_problem(c, b)
        for ai in range(len(ALPHAS)):
            xo[:, :, b, ai], uo[:, :, b, ai], co[:, b, ai] = oracle_rollout(po, c, b, ai)
            for got, ref in ((xs[:, :, b, ai], xo[:, :, b, ai]), (us[:, :, b, ai], uo[:, :, b, ai]), (cn[:, b, ai], co[:, b, ai])):
                worst = max(worst, relerr(got.astype(float), ref))
    for got, ref in ((xs, xo), (us, uo), (cn, co)):
        d = rollout_dist(got.astype(float), ref)
        for b in range(B):
            for ai in range(len(ALPHAS)):
                one = relerr((got[:, :, b, ai] if got.ndim == 4 else got[:, b, ai]).astype(float), ref[:, :, b, ai] if ref.ndim == 4 else ref[:, b, ai])
                assert abs(d[b, ai] - one) <= 1e-3 * one + 1e-300, (b, ai, d[b, ai], one)
    csd = float(np.max(np.abs(cs.astype(float) - co.sum(axis=0)) / np.abs(co.sum(axis=0))))
    print("worst longdouble-vs-oracle distance %.3g (csum %.3g)" % (worst, csd))
    assert worst < RTOL and csd < RTOL
    if lims:
        share = clamped_share(c, us)
        print("clamped share %.1f %%" % (100 * share))
        assert 0.1 < share < 0.9
    if policy and not lims and nan is None:                           # α = 0 with x[:, 0] = x0: the first control is ū_0 exactly
        assert np.array_equal(us[:, 0, :, 2].astype(float), c["u"][:, 0, :])


def test_rollout_dist_sees_a_nan_and_a_wrong_small_step():
    need_longdouble()
    ref = np.ones((2, 5, 3, 2)); ref[:, 3] = 1e-3
    got = ref.copy(); got[0, 3, 1, 1] = 1.1e-3
    d = rollout_dist(got, ref)
    assert d[1, 1] == pytest.approx(0.1) and not d[0].any() and d[1, 0] == 0
    got[1, 0, 2, 0] = np.nan
    assert np.isnan(rollout_dist(got, ref)[2, 0]) and not (rollout_dist(got, ref) < RTOL).all()
