"""Seeded cases of the n <= 32, m <= 8 KL kernels of csrc/kl.hip (∇kl, forward_covariance, kl_div_wiki), shared by
tests/test_kl_reference_cpu.py and tests/test_gpu_kl_narrow.py.  No tests here.

One table per operation; the first column of a row is the kernel the library's choice function is expected to name for it
(ddp_kl_div_choice, ddp_fcov_choice), so that every kernel and both sides of every limit appear.  Conventions, after the recipe of
kl_wide_cases.single_pass: dynamics 0.9 I + 0.05 randn drawn per step and per trajectory (Σ does not grow over N = 130), policy
covariances SPD with condition number below 1e2, K at scale 0.2 (previous) and 0.3 (new), B = 3 unless the row says otherwise.
References: tests/kl_reference.py (long double), oracle/ddp_oracle_kl.c, oracle/np_kl.py — computed once per case and cached."""
import functools

import numpy as np

RTOL = 1e-8
B0 = 3
EPS = 2.0 ** -52

DIRECT, LDS41, LDS42, LDS00 = "kl_div_kernel", "kl_div_lds_kernel<4,1>", "kl_div_lds_kernel<4,2>", "kl_div_lds_kernel<0,0>"
GENERIC, Q4_1, Q4_2, Q4L = "fcov_kernel", "fcov_q4_kernel<1>", "fcov_q4_kernel<2>", "fcov_q4l_kernel"


def _rows(want, shapes, Ns, Bs=(B0,), **kw):
    return [dict(want=want, n=n, m=m, N=N, B=B, **kw) for (n, m) in shapes for N in Ns for B in Bs]


# ---- kl_div_wiki: env is the switch setting of the row (DDP_KL_LDS)
KLDIV = (_rows(LDS41, [(4, 1)], (1, 63, 64, 65, 130), env=None) + _rows(LDS42, [(4, 2)], (1, 63, 64, 65, 130), env=None)
         + _rows(LDS00, [(1, 1), (6, 1), (3, 2), (2, 3), (3, 3)], (1, 2, 63, 64, 65, 130), env=None)
         + _rows(DIRECT, [(7, 1), (5, 2), (4, 3), (1, 4)], (2, 65), env=None)                     # one step past the image limit
         + _rows(DIRECT, [(32, 1), (1, 8), (17, 5), (32, 8)], (1, 65), env=None)                  # box corners
         + _rows(DIRECT, [(4, 1), (3, 3)], (65,), env="0"))                                       # direct by DDP_KL_LDS=0

# ---- forward_covariance: env = (DDP_FCOV_Q4, DDP_FCOV_Q4L); mis: K sits 8 bytes into its device buffer
FCOV = (_rows(GENERIC, [(1, 1), (7, 1), (8, 2), (9, 3), (17, 5), (32, 1), (1, 8), (32, 8)], (1, 2, 13), env=(None, None), mis=False)
        + _rows(Q4_1, [(4, 1)], (1, 2, 8, 15, 70), (1, 2, 5), env=(None, None), mis=False)
        + _rows(Q4_2, [(4, 2)], (1, 2, 8, 15, 70), (1, 2, 5), env=(None, None), mis=False)
        + _rows(Q4L, [(4, 1)], (16, 24, 72), (1, 5), env=(None, None), mis=False)
        + _rows(Q4_1, [(4, 1)], (16,), (6145,), env=(None, None), mis=False)                      # q4 by fall-back: B > 6144
        + _rows(Q4_1, [(4, 1)], (16,), env=(None, None), mis=True)                                # q4 by fall-back: one operand misaligned
        + _rows(GENERIC, [(4, 2)], (15,), env=("0", None), mis=False))                            # generic by DDP_FCOV_Q4=0

SHAPES = sorted({(r["n"], r["m"]) for r in KLDIV + FCOV})
TERMS = [dict(n=n, m=m, N=N, B=B0) for (n, m) in SHAPES for N in (2, 65)]                         # N·B = 6 and 195: a ragged block of 256


def kid(r):
    tag = "n%dm%d-N%d-B%d" % (r["n"], r["m"], r["N"], r["B"])
    env = r.get("env")
    if env == "0" or (isinstance(env, tuple) and env[0] == "0"):
        tag += "-off"
    return tag + ("-mis" if r.get("mis") else "")


def image_fits(n, m):
    """the LDS image of kl_div_lds_kernel: 64 steps of the ten operands, each at an odd stride of doubles, in 48 KB"""
    lens = (n, n, (n + m) ** 2, n * m, m, m * m, n * m, m, m * m, m * m)              # xnew xold sigmanew Kn kn Σn Kp kp Σp Σip
    return sum((l | 1) * 64 * 8 for l in lens) <= 48 * 1024


def _spd(rng, d, s=1.0):
    a = rng.standard_normal((d, d))
    return s * (a @ a.T / d + 0.5 * np.eye(d))


def _spd_stack(rng, d, N, B, s=1.0):
    return np.stack([np.stack([_spd(rng, d, s) for _ in range(N)], -1) for _ in range(B)], -1)


def _inv_stack(S):
    return np.moveaxis(np.linalg.inv(np.moveaxis(S, (0, 1), (-2, -1))), (-2, -1), (0, 1))


@functools.lru_cache(maxsize=None)
def case(n, m, N, B):
    """the operands of all three operations at one size: a previous policy (Kp, kp, Σp, Σip), a new one (Kn, kn, Σn), a model
    (fx per step and trajectory, R1), two trajectories and the covariance chain of the new policy (float64 of the long double one)"""
    import kl_reference as ref
    rng = np.random.default_rng(100000 * n + 1000 * m + 7 * N + B)
    c = dict(n=n, m=m, N=N, B=B)
    if B > 64:                                            # the big batch: one vectorised draw
        c["fx"] = 0.9 * np.eye(n)[:, :, None, None] + 0.05 * rng.standard_normal((n, n, N, B))
        a = rng.standard_normal((m, m, N, B))
        c["Sn"] = 0.5 * (np.einsum("ijtb,kjtb->iktb", a, a) / m + 0.5 * np.eye(m)[:, :, None, None])
        a = rng.standard_normal((m, m, N, B))
        c["Sip"] = 2.0 * (np.einsum("ijtb,kjtb->iktb", a, a) / m + 0.5 * np.eye(m)[:, :, None, None])
    else:
        c["fx"] = np.stack([np.stack([0.9 * np.eye(n) + 0.05 * rng.standard_normal((n, n)) for _ in range(N)], -1) for _ in range(B)], -1)
        c["Sn"] = _spd_stack(rng, m, N, B, 0.5)
        c["Sip"] = _spd_stack(rng, m, N, B, 2.0)
    c["Sp"] = _inv_stack(c["Sip"])
    c["R1"] = 0.01 * np.eye(n)
    c["Kp"], c["kp"] = 0.2 * rng.standard_normal((m, n, N, B)), 0.1 * rng.standard_normal((m, N, B))
    c["Kn"], c["kn"] = 0.3 * rng.standard_normal((m, n, N, B)), 0.1 * rng.standard_normal((m, N, B))
    c["xold"] = rng.standard_normal((n, N, B))
    c["xnew"] = c["xold"] + 0.1 * rng.standard_normal((n, N, B))
    for k_ in list(c):
        if isinstance(c[k_], np.ndarray):
            c[k_] = np.asfortranarray(c[k_])
            c[k_].setflags(write=False)
    c["sig"] = np.asfortranarray(ref.forward_covariance(c["fx"], c["R1"], c["Kn"], c["Sn"]).astype(np.float64))
    c["sig"].setflags(write=False)
    return c


KL_ARGS = ("xnew", "xold", "sig", "Kn", "kn", "Sn", "Kp", "kp", "Sp", "Sip")


def _frozen(*arrs):
    for a in arrs:
        a.setflags(write=False)
    return arrs


# ---- long double references, once per case (frozen)
@functools.lru_cache(maxsize=None)
def ref_terms(n, m, N, B):
    import kl_reference as ref
    c = case(n, m, N, B)
    return _frozen(*ref.grad_kl(c["Kp"], c["kp"], c["Sip"]))


@functools.lru_cache(maxsize=None)
def ref_fcov(n, m, N, B, shared):
    """shared: the model of trajectory 0 for the whole batch"""
    import kl_reference as ref
    c = case(n, m, N, B)
    return _frozen(ref.forward_covariance(c["fx"][..., 0] if shared else c["fx"], c["R1"], c["Kn"], c["Sn"]))[0]


@functools.lru_cache(maxsize=None)
def ref_kl_div(n, m, N, B):
    import kl_reference as ref
    c = case(n, m, N, B)
    kld, mean, threw = ref.kl_div_wiki(*[c[k_] for k_ in KL_ARGS])
    assert not threw.any()
    return _frozen(kld, mean)


# ---- the C oracle and the NumPy restatement, one trajectory at a time, stacked along the batch
def _oracle_mod(which):
    if which == "c":
        from oracle import oracle_ctypes as mod
    else:
        from oracle import np_kl as mod
    return mod


def oracle_terms(which, c, b):
    mod = _oracle_mod(which)
    return (mod.kl_terms if which == "c" else mod.grad_kl)(c["Kp"][..., b], c["kp"][..., b], c["Sip"][..., b])


def oracle_fcov(which, c, b, shared=False):
    return _oracle_mod(which).forward_covariance(c["fx"][..., 0 if shared else b], c["R1"], c["Kn"][..., b], c["Sn"][..., b])


def oracle_kl_div(which, c, b):
    """(kldiv[T], mean) of trajectory b; a logdet that threw: (None, +Inf)"""
    new = dict(K=c["Kn"][..., b], k=c["kn"][..., b], S=c["Sn"][..., b])
    prev = dict(K=c["Kp"][..., b], k=c["kp"][..., b], S=c["Sp"][..., b], Si=c["Sip"][..., b])
    r = _oracle_mod(which).kl_div_wiki(c["xnew"][..., b], c["xold"][..., b], c["sig"][..., b], new, prev)
    return (None, np.inf) if np.isscalar(r) or np.ndim(r) == 0 else (r, r.mean())


@functools.lru_cache(maxsize=None)
def oracle_dist(op, n, m, N, B):
    """d_orc: conftest.relerr of the C oracle against the long double reference, the worst trajectory of the case (of the first 64 of
    a big batch: the oracle is one trajectory per call).  op: "terms" | "fcov" | "fcov_shared" | "kl_div" """
    from conftest import relerr
    c = case(n, m, N, B)
    worst = 0.0
    for b in range(min(B, 64)):
        if op == "terms":
            worst = max([worst] + [relerr(a, r[..., b].astype(float)) for a, r in zip(oracle_terms("c", c, b), ref_terms(n, m, N, B))])
        elif op == "kl_div":
            worst = max(worst, relerr(oracle_kl_div("c", c, b)[0], ref_kl_div(n, m, N, B)[0][:, b].astype(float), 0))
        else:
            sh = op == "fcov_shared"
            worst = max(worst, relerr(oracle_fcov("c", c, b, sh), ref_fcov(n, m, N, B, sh)[..., b].astype(float)))
    return worst


def bound(op, n, m, N, d_orc):
    """what a kernel's distance to the long double reference may be besides RTOL: eight times the oracle's on the same case, or the
    rounding of the longest dot product — n + m terms in ∇kl and kl_div_wiki, N (2n + m) along the covariance chain"""
    L = N * (2 * n + m) if op.startswith("fcov") else n + m
    return max(8.0 * d_orc, L * EPS)


# ------------------------------------------------------------------------------------------------------------- designed inputs
DESIGNED_SHAPES = [(4, 2), (3, 3), (5, 2)]                    # lds<4,2>, lds<0,0>, direct: one shape per kernel family with m >= 2
DESIGNED = ("identical", "inverse", "row_exchange", "negative_det", "singular_new", "singular_prev", "nan")
DESIGNED_11 = ("negative_det", "nan")                        # also at (4, 1): 1 x 1 covariances
DN, DB, DT, DTRAJ = 5, 3, 2, 1                                # N, B, and the designed step (DT) of trajectory DTRAJ
# Σn of the row-exchange step: a zero leading entry, determinant 6/256 and 23.55/4096 — column 0 holds |0| < |b|: one exchange; the next
# pivot is negative: the second sign flip; the magnitudes of every pivot column differ (checked in long double by the CPU test)
ROWX = {2: np.array([[0.0, -2.0], [3.0, 1.0]]) / 16, 3: np.array([[0.0, -2.0, 0.5], [3.0, 1.0, 0.25], [1.5, 0.7, 4.0]]) / 16}


def designed_ids():
    return [(n, m, kind) for (n, m) in DESIGNED_SHAPES for kind in DESIGNED] + [(4, 1, kind) for kind in DESIGNED_11]


@functools.lru_cache(maxsize=None)
def designed(n, m, kind):
    """the ten kl_div_wiki operands (a dict like case()) with one designed step, and what the step, its trajectory's mean and the
    rest must be"""
    base = case(n, m, DN, DB)
    c = {k_: (v.copy() if isinstance(v, np.ndarray) else v) for k_, v in base.items()}
    eye = np.asfortranarray(np.tile(np.eye(m)[:, :, None, None], (1, 1, DN, DB)))
    if kind == "identical":                                   # Σ = Σi = I, one policy on both sides: tr(I I) = m, both logdets 0 — exactly 0
        c.update(Kn=c["Kp"].copy(), kn=c["kp"].copy(), Sn=eye.copy(), Sp=eye.copy(), Sip=eye.copy())
    elif kind == "inverse":                                   # one policy on both sides, Σi = inv(Σ) to rounding: only tr(Σi Σ) - m is left
        c.update(Kn=c["Kp"].copy(), kn=c["kp"].copy(), Sn=c["Sp"].copy())
    elif kind == "row_exchange":
        c["Sn"][:, :, DT, DTRAJ] = ROWX[m]
    elif kind == "negative_det":
        c["Sn"][:, :, DT, DTRAJ] = np.diag([-1.0] + [1.0] * (m - 1))
    elif kind == "singular_new":
        c["Sn"][0, :, DT, DTRAJ] = 0.0
    elif kind == "singular_prev":
        c["Sp"][0, :, DT, DTRAJ] = 0.0
    elif kind == "nan":
        c["xnew"][0, DT, DTRAJ] = np.nan
    else:
        raise KeyError(kind)
    for v in c.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return c


def check_designed(n, m, kind, kld, mean, ref=None):
    """the exact outcome of a designed input on (kldiv[T,B], mean[B]); ref: (kldiv, mean) of the undesigned case — what every
    other step and trajectory must still be (to `tol`), or None"""
    kld, mean = np.asarray(kld, dtype=float), np.asarray(mean, dtype=float)
    assert kld.shape == (DN, DB) and mean.shape == (DB,)
    other = np.ones((DN, DB), bool); other[DT, DTRAJ] = False
    others = [b for b in range(DB) if b != DTRAJ]
    if kind == "identical":
        assert not kld.any() and not mean.any() and not np.signbit(kld).any()
    elif kind == "inverse":
        cmax = max(float(np.linalg.cond(designed(n, m, kind)["Sip"][:, :, t, b])) for t in range(DN) for b in range(DB))
        assert np.all(kld >= 0) and np.all(kld <= m * EPS * cmax), (kld.max(), m * EPS * cmax)
    elif kind == "row_exchange":
        assert np.all(np.isfinite(kld)) and np.all(np.isfinite(mean)) and kld[DT, DTRAJ] > 0
    elif kind == "negative_det":
        assert np.all(np.isfinite(kld)), "kldiv itself is finite"
        assert np.isposinf(mean[DTRAJ]) and np.all(np.isfinite(mean[others]))
    elif kind == "singular_new":
        assert np.isposinf(kld[DT, DTRAJ]) and np.all(np.isfinite(kld[other]))
        assert np.isposinf(mean[DTRAJ]) and np.all(np.isfinite(mean[others]))
    elif kind == "singular_prev":
        assert kld[DT, DTRAJ] == 0 and not np.signbit(kld[DT, DTRAJ]) and np.all(np.isfinite(kld)) and np.all(np.isfinite(mean))
    elif kind == "nan":
        assert np.isnan(kld[DT, DTRAJ]) and np.all(np.isfinite(kld[other]))
        assert np.isnan(mean[DTRAJ]) and np.all(np.isfinite(mean[others]))


# ------------------------------------------------------------------------------------------------------------- whole loops
# registered LQ problems on shapes kl_div_lds_kernel<0,0> serves, built as kl_wide_cases.loop_case; the seed is one at which the
# oracle's outcome does not change under TIE_EPS perturbations (test_kl_reference_cpu.py checks that)
LOOPS = [(6, 1, 70, 37), (3, 3, 66, 37)]                     # (n, m, T, seed)
LOOP_B, LOOP_KL_STEP, LOOP_MAX_ITER = 3, 2e-4, 40
TIE_EPS, TIE_DRAWS = 1e-13, 8


@functools.lru_cache(maxsize=None)
def loop_case(n, m, T, seed):
    import scipy.linalg as sla
    rng = np.random.default_rng(seed)
    B, h = LOOP_B, 0.01
    A0 = rng.standard_normal((n, n)); A = sla.expm(h * (A0 - A0.T)); Bm = h * rng.standard_normal((n, m))
    Q, R = h * np.eye(n), 0.1 * h * np.eye(m)
    u = 0.1 * rng.standard_normal((m, T, B)) * np.linspace(0.5, 3.0, B)
    x = np.zeros((n, T, B)); x[:, 0, :] = 1.0 + 0.1 * rng.standard_normal((n, B))
    for t in range(T - 1):
        x[:, t + 1, :] = A @ x[:, t, :] + Bm @ u[:, t, :]
    cost0 = 0.5 * np.einsum("itb,ij,jtb->b", x, Q, x) + 0.5 * np.einsum("itb,ij,jtb->b", u, R, u)
    eye = np.repeat(np.repeat(np.eye(m)[:, :, None, None], T, 2), B, 3)
    return dict(n=n, m=m, T=T, B=B, A=A, Bm=Bm, Q=Q, R=R, u=u, x=x, cost0=cost0, eye=eye, lims=None, R1=1e-4 * np.eye(n),
                fx=np.repeat(A[:, :, None], T, 2), fu=np.repeat(Bm[:, :, None], T, 2))


def _oracle_loop(c, b, x, u):
    from oracle import oracle_ctypes as oc
    n, m, T = c["n"], c["m"], c["T"]
    p = oc.make_problem("lq", n, m, T, A=c["A"], B=c["Bm"], Q=c["Q"], R=c["R"])
    pb = dict(K=np.zeros((m, n, T)), k=u, S=c["eye"][..., b], Si=c["eye"][..., b])
    return oc.ilqgkl(p, x, float(c["cost0"][b]), pb, dict(fx=c["fx"], R1=c["R1"]), kl_step=LOOP_KL_STEP, max_iter=LOOP_MAX_ITER, lims=None)


@functools.lru_cache(maxsize=None)
def loop_reference(n, m, T, seed):
    """the C oracle's iLQGkl of every trajectory: (x, u, policy, Vx, Vxx, cost, info)"""
    c = loop_case(n, m, T, seed)
    return [_oracle_loop(c, b, c["x"][..., b], c["u"][..., b]) for b in range(c["B"])]


def outcome(info):
    return (info["status"], info["iter"], info["n_backpass"])


def loop_outcomes_nearby(n, m, T, seed, b, draw_seed):
    """the oracle's outcomes of TIE_DRAWS copies of trajectory b whose x, u are off by TIE_EPS relative (kl_wide_cases): where they
    differ from the unperturbed outcome the REFERENCE is discontinuous at this input"""
    c = loop_case(n, m, T, seed)
    rng = np.random.default_rng(draw_seed)
    xb, ub = c["x"][..., b], c["u"][..., b]
    return [outcome(_oracle_loop(c, b, xb * (1 + TIE_EPS * rng.standard_normal(xb.shape)), ub * (1 + TIE_EPS * rng.standard_normal(ub.shape)))[6])
            for _ in range(TIE_DRAWS)]
