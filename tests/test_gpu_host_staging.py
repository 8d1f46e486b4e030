"""Every host-pointer flavour of the C ABI (`*_f64`) against its `_dev` twin on buffers uploaded with ddp_memcpy_h2d: the same kernels on
the same inputs, so every output is equal BIT FOR BIT (compared as uint64 / raw integers, no tolerance).  What differs between the two
calls is the staging alone: which buffers get device storage, how large each is, what is uploaded and what comes back — a swapped
size, a missing upload or a null pointer that should have been storage shows up as a different bit (n != m and N != B, so no two
buffers of a call have the same size by accident)."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

n, m, N, B = 3, 2, 4, 3
NSTATS, KLSTATS = 8, 12


# ---------------------------------------------------------------------------------------------------------------- argument kinds
class In:
    def __init__(self, a):
        self.a = None if a is None else np.asfortranarray(a)


class Out:
    """host=False: the host flavour gets NULL (it stages a temporary or hands the null on), the `_dev` twin a buffer; not compared"""
    def __init__(self, shape, dtype=np.float64, host=True):
        self.shape, self.dtype, self.host = tuple(int(s) for s in np.atleast_1d(shape)), dtype, host


class InOut(In):
    pass


class Raw:
    """passed as it is to both calls (sizes, flags, option structs, host arrays such as alpha)"""
    def __init__(self, v):
        self.v = v


class DevOnly(Raw):
    """an argument only the `_dev` twin has (`active`)"""


class HostInt:
    """an int the library writes through a host pointer in both flavours (global_iters)"""


class Prob:
    def __init__(self, kind=0, B_=B, cost_diag=1, Q=None, R=None, A=None, Bm=None):
        self.kind, self.B, self.cost_diag = kind, B_, cost_diag
        self.Q, self.R, self.A, self.Bm = (None if a is None else np.asfortranarray(a) for a in (Q, R, A, Bm))


class KLTerms:
    def __init__(self, cx, cu, cxx, cxu, cuu, eta):
        self.arrs = [np.asfortranarray(a) for a in (cx, cu, cxx, cxu, cuu, eta)]


@pytest.fixture(scope="module")
def lib():
    from ddp_amd import _lib
    return _lib


@pytest.fixture()
def h(lib):
    hd = lib.Handle()                                          # a handle of its own: its scratch starts empty in every test
    yield hd
    hd.close()


def bits(a):
    a = np.ascontiguousarray(np.asarray(a).ravel(order="F"))
    return a.view(np.uint64) if a.dtype == np.float64 else a


def pair(lib, h, name, args):
    """calls `name` on host arrays and `name`_dev on uploaded copies; asserts equal bits for every output the host flavour returns;
    returns the host flavour's outputs in argument order (None for those it was not asked for)"""
    L = lib.lib()
    keep, frees = [], []

    def up(a):
        if a is None:
            return None
        p = h.to_device(a)
        frees.append(p)
        return p

    def problem(P, dev):
        S = lib.Problem()
        S.kind, S.n, S.m, S.N, S.B = P.kind, (4 if P.kind else n), (1 if P.kind else m), N, P.B
        mk = up if dev else lib.ptr
        S.Q, S.R = mk(P.Q), mk(P.R)
        if P.kind == 0:
            S.A, S.Bm = mk(P.A), mk(P.Bm)
        else:
            S.g, S.l, S.h, S.d = 9.82, 0.35, 0.01, 0.99
            S.goal[0] = np.pi
        S.cost_diag = P.cost_diag
        keep.append(S)
        return C.byref(S)

    def klterms(K, dev):
        S = lib.KLCostTerms()
        mk = up if dev else lib.ptr
        S.cx, S.cu, S.cxx, S.cxu, S.cuu, S.eta = (mk(a) for a in K.arrs)
        S.eta_tv = 0
        keep.append(S)
        return C.byref(S)

    # ---- host flavour
    hargs, houts, hints = [], [], []
    for a in args:
        if isinstance(a, DevOnly):
            continue
        if isinstance(a, InOut):
            buf = None if a.a is None else a.a.copy(order="F")
            houts.append(buf); hargs.append(lib.ptr(buf))
        elif isinstance(a, In):
            hargs.append(lib.ptr(a.a))
        elif isinstance(a, Out):
            buf = np.zeros(a.shape, dtype=a.dtype, order="F") if a.host else None
            houts.append(buf); hargs.append(lib.ptr(buf))
        elif isinstance(a, HostInt):
            v = C.c_int(-1); hints.append(v); hargs.append(C.byref(v))
        elif isinstance(a, Prob):
            hargs.append(problem(a, False))
        elif isinstance(a, KLTerms):
            hargs.append(klterms(a, False))
        else:
            hargs.append(a.v)
    lib.check(getattr(L, name)(h.raw, *hargs))
    # ---- the `_dev` twin
    dargs, douts, dints = [], [], []
    for a in args:
        if isinstance(a, InOut):
            p = up(a.a); douts.append((p, a.a)); dargs.append(p)
        elif isinstance(a, In):
            dargs.append(up(a.a))
        elif isinstance(a, Out):
            p = h.malloc(int(np.prod(a.shape)) * np.dtype(a.dtype).itemsize); frees.append(p)
            douts.append((p, np.empty(a.shape, dtype=a.dtype))); dargs.append(p)
        elif isinstance(a, HostInt):
            v = C.c_int(-1); dints.append(v); dargs.append(C.byref(v))
        elif isinstance(a, Prob):
            dargs.append(problem(a, True))
        elif isinstance(a, KLTerms):
            dargs.append(klterms(a, True))
        else:
            dargs.append(a.v)
    lib.check(getattr(L, name + "_dev")(h.raw, *dargs))
    h.sync()
    try:
        assert len(houts) == len(douts)
        for i, (hb, (p, like)) in enumerate(zip(houts, douts)):
            if hb is None:
                continue
            db = h.to_host(p, like.shape, like.dtype)
            assert hb.shape == db.shape
            assert np.array_equal(bits(hb), bits(db)), "%s: output %d differs from %s_dev at %d of %d words" % (
                name, i, name, int(np.sum(bits(hb) != bits(db))), bits(hb).size)
        assert [v.value for v in hints] == [v.value for v in dints], name
    finally:
        for p in frees:
            h.free(p)
    return houts


# ------------------------------------------------------------------------------------------------------------------------ data
def lq_data(seed=0, B_=B):
    r = np.random.default_rng(seed)
    A = 0.9 * np.eye(n) + 0.05 * r.standard_normal((n, n))
    Bm = 0.3 * r.standard_normal((n, m))
    d = dict(A=A, Bm=Bm, Q=np.diag([1.0, 2.0, 0.5]), R=np.diag([0.1, 0.2]))
    d["x0"] = 1.0 + 0.1 * r.standard_normal((n, B_))
    d["u"] = 0.1 * r.standard_normal((m, N, B_))
    d["x"] = 1.0 + 0.1 * r.standard_normal((n, N, B_))
    d["K"] = 0.1 * r.standard_normal((m, n, N, B_))
    d["k"] = 0.1 * r.standard_normal((m, N, B_))
    d["lims"] = np.array([[-0.5, 0.5], [-0.4, 0.6]])
    return d


def lq_prob(d, B_=B, cost_diag=1, Q=None):
    return Prob(0, B_, cost_diag, d["Q"] if Q is None else Q, d["R"], d["A"], d["Bm"])


def spd(r, k, *lead):
    a = r.standard_normal((k, k) + lead)
    s = np.einsum("ij...,kj...->ik...", a, a)
    return s + (k * np.eye(k)).reshape((k, k) + (1,) * len(lead))


def ilqg_opts(lib, max_iter=4):
    o = lib.ILQGOpts()
    lib.lib().ddp_ilqg_default_opts(C.byref(o))
    o.max_iter = max_iter
    return o


def ilqg_outs(B_=B, CL=N):
    return [Out((n, N, B_)), Out((m, N, B_)), Out((m, n, N, B_)), Out((m, N, B_)), Out((m, m, N, B_)), Out((n, N, B_)), Out((n, n, N, B_)),
            Out((CL, B_)), Out((NSTATS, B_))]


# ------------------------------------------------------------------------------------------------- capi.hip: array-level entries
def back_pass_case(lib, has_lims, B_=B, seed=1):
    r = np.random.default_rng(seed)
    d = lib.BPDesc(n, m, N, B_, 1, 1, 1, 0, 1, int(has_lims))     # fx[n,n,N,B], fu[n,m,N,B]; cxx[n,n,N] ... shared by the batch
    lims = np.array([[-0.05, 0.05], [-0.04, 0.06]])
    return [Raw(C.byref(d)), In(r.standard_normal((n, N, B_))), In(r.standard_normal((m, N, B_))), In(spd(r, n, N)),
            In(0.1 * r.standard_normal((n, m, N))), In(spd(r, m, N)), In(0.9 * np.eye(n)[:, :, None, None] + 0.05 * r.standard_normal((n, n, N, B_))),
            In(0.3 * r.standard_normal((n, m, N, B_))), In(np.linspace(1.0, 2.0, B_)), In(lims if has_lims else None),
            In(0.1 * r.standard_normal((m, N, B_)) if has_lims else None), DevOnly(None),
            Out((m, n, N, B_)), Out((m, N, B_)), Out((m, m, N, B_)), Out((n, N, B_)), Out((n, n, N, B_)), Out((2, B_)), Out((B_,), np.int32)], d


@pytest.mark.parametrize("has_lims", [False, True])
def test_back_pass(lib, h, has_lims):
    args, keep = back_pass_case(lib, has_lims)
    out = pair(lib, h, "ddp_back_pass_f64", args)
    assert not out[-1].any() and np.abs(out[0]).max() > 0          # no trajectory diverged: every output was computed


def test_scratch_shrinks_then_regrows(lib, h):
    """one handle: a small call (the scratch is allocated), a large one (it regrows), the small one again (it is reused as it is)"""
    small = pair(lib, h, "ddp_back_pass_f64", back_pass_case(lib, True)[0])
    pair(lib, h, "ddp_back_pass_f64", back_pass_case(lib, True, B_=67, seed=2)[0])
    again = pair(lib, h, "ddp_back_pass_f64", back_pass_case(lib, True)[0])
    for a, b in zip(small, again):
        assert np.array_equal(bits(a), bits(b))
    d = lq_data()
    pair(lib, h, "ddp_df_f64", [lq_prob(d), In(d["x"]), In(d["u"]), DevOnly(None), Out((n, N, B)), Out((m, N, B)), Raw(None), Raw(None)])


def forward_args(d, null=None, cost_diag=1, Q=None, na=2):
    alpha = np.array([1.0, 0.5])
    shapes = dict(xnew=(n, N, B, na), unew=(m, N, B, na), cnew=(N, B, na), csum=(B, na))
    return [lq_prob(d, cost_diag=cost_diag, Q=Q), In(d["K"]), In(d["k"]), In(d["x0"]), In(d["u"]), In(d["x"]), Raw(lib_ptr(alpha)), Raw(na), In(d["lims"]),
            DevOnly(None)] + [Out(s, host=k_ != null) for k_, s in shapes.items()], alpha


def lib_ptr(a):
    return a.ctypes.data_as(C.c_void_p)


@pytest.mark.parametrize("null", [None, "xnew", "unew", "cnew"])
def test_forward_pass(lib, h, null):
    args, keep = forward_args(lq_data(), null)
    out = pair(lib, h, "ddp_forward_pass_f64", args)
    assert np.abs(out[3]).min() > 0


def test_forward_pass_full_Q(lib, h):
    """cost_diag = 0: a full Q, no diagonal declaration to verify"""
    d = lq_data()
    Q = d["Q"] + 0.1 * np.ones((n, n))
    args, keep = forward_args(d, cost_diag=0, Q=Q)
    pair(lib, h, "ddp_forward_pass_f64", args)


def test_boxqp(lib, h):
    r = np.random.default_rng(3)
    cnt = 5
    args = [Raw(m), Raw(cnt), In(spd(r, m, cnt)), In(r.standard_normal((m, cnt))), In(-0.1 * np.ones((m, cnt))), In(0.2 * np.ones((m, cnt))),
            In(np.zeros((m, cnt))), Raw(None), Out((m, cnt)), Out((cnt,), np.int32), Out((m, m, cnt)), Out((m, cnt), np.uint8)]
    out = pair(lib, h, "ddp_boxqp_f64", args)
    assert np.abs(out[0]).max() > 0


def test_df_lq_and_pendcart(lib, h):
    d = lq_data()
    pair(lib, h, "ddp_df_f64", [lq_prob(d), In(d["x"]), In(d["u"]), DevOnly(None), Out((n, N, B)), Out((m, N, B)), Raw(None), Raw(None)])
    r = np.random.default_rng(4)
    P = Prob(1, B, 1, np.diag([10.0, 1, 2, 1]), np.array([[1.0]]))
    x, u = 0.3 * r.standard_normal((4, N, B)), 0.3 * r.standard_normal((1, N, B))
    pair(lib, h, "ddp_df_f64", [P, In(x), In(u), DevOnly(None), Out((4, N, B)), Out((1, N, B)), Out((4, 4, N, B)), Out((4, 1, N, B))])
    # fx, fu left out: the pendulum's kernel still writes them, into storage of the staging's own
    pair(lib, h, "ddp_df_f64", [P, In(x), In(u), DevOnly(None), Out((4, N, B)), Out((1, N, B)), Out((4, 4, N, B), host=False),
                                Out((4, 1, N, B), host=False)])


# ------------------------------------------------------------------------------------------------------------- kl.hip: KL entries
def kl_inputs(seed=5):
    r = np.random.default_rng(seed)
    S = spd(r, m, N, B) / m
    return dict(K=0.1 * r.standard_normal((m, n, N, B)), k=0.1 * r.standard_normal((m, N, B)), S=S,
                Si=np.linalg.inv(S.transpose(2, 3, 0, 1)).transpose(2, 3, 0, 1))


def kl_terms(lib, h, q):
    return pair(lib, h, "ddp_kl_terms_f64", [Raw(n), Raw(m), Raw(N), Raw(B), In(q["K"]), In(q["k"]), In(q["Si"]),
                                             Out((n, N, B)), Out((m, N, B)), Out((n, n, N, B)), Out((m, n, N, B)), Out((m, m, N, B))])


def test_kl_terms_and_back_pass_gps(lib, h):
    q = kl_inputs()
    t = kl_terms(lib, h, q)
    assert all(np.abs(a).max() > 0 for a in t)
    r = np.random.default_rng(6)
    for has_lims in (0, 1):
        d = lib.BPDesc(n, m, N, B, 1, 1, 1, 0, 1, has_lims)
        args = [Raw(C.byref(d)), In(r.standard_normal((n, N, B))), In(r.standard_normal((m, N, B))), In(spd(r, n, N)),
                In(0.1 * r.standard_normal((n, m, N))), In(spd(r, m, N)), In(0.9 * np.eye(n)[:, :, None, None] + 0.05 * r.standard_normal((n, n, N, B))),
                In(0.3 * r.standard_normal((n, m, N, B))), KLTerms(*t, np.linspace(0.5, 1.5, B)),
                In(np.array([[-0.05, 0.05], [-0.04, 0.06]]) if has_lims else None), In(0.1 * r.standard_normal((m, N, B)) if has_lims else None),
                DevOnly(None), Out((m, n, N, B)), Out((m, N, B)), Out((m, m, N, B)), Out((m, m, N, B)), Out((n, N, B)), Out((n, n, N, B)),
                Out((2, B)), Out((B,), np.int32)]
        out = pair(lib, h, "ddp_back_pass_gps_f64", args)
        assert not out[-1].any()


@pytest.mark.parametrize("kldiv", [True, False])
def test_forward_covariance_and_kl_div(lib, h, kldiv):
    q, q2 = kl_inputs(), kl_inputs(7)
    r = np.random.default_rng(8)
    fx = 0.9 * np.eye(n)[:, :, None] + 0.05 * r.standard_normal((n, n, N))
    sig, = pair(lib, h, "ddp_forward_covariance_f64", [Raw(n), Raw(m), Raw(N), Raw(B), In(fx), Raw(0), In(0.1 * spd(r, n)), In(q["K"]), In(q["S"]),
                                                       Out((n + m, n + m, N, B))])
    assert np.abs(sig).max() > 0
    d = lq_data()
    out = pair(lib, h, "ddp_kl_div_f64", [Raw(n), Raw(m), Raw(N), Raw(B), In(d["x"]), In(d["x"] + 0.01), In(sig), In(q2["K"]), In(q2["k"]), In(q2["S"]),
                                          In(q["K"]), In(q["k"]), In(q["S"]), In(q["Si"]), Out((N, B), host=kldiv), Out((B,))])
    assert out[1].shape == (B,)


# --------------------------------------------------------------------------------------------------------- ilqg.hip: the drivers
def test_ilqg_flavours(lib, h):
    d = lq_data()
    o = ilqg_opts(lib)
    cap = 6
    head = [lq_prob(d), Raw(C.byref(o))]
    # ddp_ilqg_f64 with trace_cost; with limits
    pair(lib, h, "ddp_ilqg_f64", head + [In(d["x0"]), In(d["u"]), In(d["lims"])] + ilqg_outs() + [Raw(cap), Out((cap, B)), HostInt()])
    # ddp_ilqg_ex_f64: with trace7, without it, and pre-rolled with cost0
    out = pair(lib, h, "ddp_ilqg_ex_f64", head + [In(d["x0"]), Raw(0), In(d["u"]), In(None), In(None)] + ilqg_outs() + [Raw(cap), Out((7, cap, B)), HostInt()])
    assert (out[8][1] >= 1).all() and np.abs(out[9]).max() > 0       # every trajectory iterated, and the trace was written
    plain = pair(lib, h, "ddp_ilqg_ex_f64", head + [In(d["x0"]), Raw(0), In(d["u"]), In(None), In(None)] + ilqg_outs() + [Raw(0), Raw(None), HostInt()])
    for a, b in zip(out[:9], plain):
        assert np.array_equal(bits(a), bits(b))
    x, u, cost = plain[0], plain[1], plain[7]
    pair(lib, h, "ddp_ilqg_ex_f64", head + [In(x), Raw(1), In(u), In(cost), In(None)] + ilqg_outs() + [Raw(cap), Out((7, cap, B)), HostInt()])
    pair(lib, h, "ddp_ilqg_ex_f64", head + [In(x), Raw(1), In(u), In(None), In(d["lims"])] + ilqg_outs() + [Raw(0), Raw(None), HostInt()])
    # ddp_ilqg_warm_f64
    pair(lib, h, "ddp_ilqg_warm_f64", head + [In(x), In(u), In(cost), In(None)] + ilqg_outs() + [Raw(cap), Out((cap, B)), HostInt()])


def test_ilqg_queue_and_mpc(lib, h):
    P_ = 5                                                     # problems of the queue: more than its two slots
    d = lq_data(9, P_)
    o = ilqg_opts(lib)
    out = pair(lib, h, "ddp_ilqg_queue_f64", [lq_prob(d, P_), Raw(C.byref(o)), Raw(2), In(d["x0"]), In(d["u"]), In(d["lims"])] + ilqg_outs(P_) + [HostInt()])
    assert (out[8][1] >= 1).all()
    d = lq_data()
    steps = 2
    # the closed loop: K ... stats are no arguments of this entry, the driver gets them as NULL
    out = pair(lib, h, "ddp_ilqg_mpc_f64", [lq_prob(d), Raw(C.byref(o)), Raw(steps), Raw(0), In(d["x0"]), In(d["u"]), In(None),
                                            Out((n, steps + 1, B)), Out((m, steps, B)), Out((NSTATS, steps, B)), Out((n, N, B)), Out((m, N, B)), HostInt()])
    assert np.array_equal(out[0][:, 0], d["x0"]) and np.abs(out[1]).max() > 0


def ilqgkl_args(lib, d, q, o, etab, cost0, user=False):
    r = np.random.default_rng(10)
    fx = np.repeat(d["A"][:, :, None], N, 2)
    args = [Raw(C.byref(o)), In(d["x"]), In(cost0), In(q["K"]), In(d["u"]), In(q["S"]), In(q["Si"]), In(fx), Raw(0), In(0.1 * spd(r, n)), In(None),
            InOut(etab), Out((n, N, B)), Out((m, N, B)), Out((m, n, N, B)), Out((m, m, N, B)), Out((m, m, N, B)), Out((n, N, B)), Out((n, n, N, B)),
            Out((N, B)), Out((2, B)), Out((KLSTATS, B)), HostInt()]
    return args


@pytest.mark.parametrize("etab", [True, False])
def test_ilqgkl(lib, h, etab):
    d, q = lq_data(), kl_inputs()
    o = lib.ILQGKLOpts()
    lib.lib().ddp_ilqgkl_default_opts(C.byref(o))
    o.max_iter = 3
    eb = np.repeat(np.array([1e-8, 1.0, 1e16])[:, None], B, 1) * np.array([1.0, 2.0, 3.0])[None, :] if etab else None
    out = pair(lib, h, "ddp_ilqgkl_f64", [lq_prob(d)] + ilqgkl_args(lib, d, q, o, eb, np.array([3.0, 4.0, 5.0]) if etab else None))
    assert (out[-1][1] >= 1).all()
    if etab:
        assert out[0].shape == (3, B) and np.isfinite(out[0]).all()    # the brackets came back (and equal those of _dev, above)


# -------------------------------------------------------------------------------------------------------------- user_problem.hip
def user_params(d):
    return np.concatenate([d[k_].ravel(order="F") for k_ in ("A", "Bm", "Q", "R")])


@pytest.fixture(scope="module")
def user(lib):
    """the linear-quadratic example as a user problem with n = 3, m = 2: (plain, second-order) on a handle of the module's own"""
    import ddp_amd
    hd = lib.Handle()
    src = ddp_amd.example_source("lq_ad")
    L = lib.lib()
    if L.ddp_user_check(src.encode(), n, m, 28, 4, None) != 0 and b"hiprtc" in L.ddp_last_error() and b"load" in L.ddp_last_error():
        pytest.skip("no hiprtc on this machine: %s" % L.ddp_last_error().decode())
    p1 = ddp_amd.DeviceProblem(src, n, m, nparam=28, autodiff=True)
    p2 = ddp_amd.DeviceProblem(src, n, m, nparam=28, autodiff=True, second_order=True)
    yield hd, p1._ptr(hd), p2._ptr(hd)
    hd.close()


def test_user_array_entries(lib, user):
    h, up, up2 = user
    d = lq_data()
    r = np.random.default_rng(11)
    # per-trajectory parameters: [28, B]
    prm = np.repeat(user_params(d)[:, None], B, 1) * (1.0 + 0.01 * np.arange(B))[None, :]
    head = lambda p, P_=prm, pb=1: [Raw(p), Raw(N), Raw(B), In(P_), Raw(pb)]
    df = pair(lib, h, "ddp_user_df_f64", head(up) + [In(d["x"]), In(d["u"]), DevOnly(None), Out((n, n, N, B)), Out((n, m, N, B)), Out((n, N, B)),
                                                    Out((m, N, B)), Out((n, n, N, B)), Out((n, m, N, B)), Out((m, m, N, B))])
    # the Hessians left out: not computed, no storage
    pair(lib, h, "ddp_user_df_f64", head(up) + [In(d["x"]), In(d["u"]), DevOnly(None), Out((n, n, N, B)), Out((n, m, N, B)), Out((n, N, B)),
                                               Out((m, N, B)), Raw(None), Raw(None), Raw(None)])
    alpha = np.array([1.0, 0.5])
    pair(lib, h, "ddp_user_forward_pass_f64", head(up) + [In(d["K"]), In(d["k"]), In(d["x0"]), In(d["u"]), In(d["x"]), Raw(lib_ptr(alpha)), Raw(2),
                                                         In(d["lims"]), DevOnly(None), Out((n, N, B, 2)), Out((m, N, B, 2)), Out((N, B, 2)), Out((B, 2))])
    pair(lib, h, "ddp_user_costfun_f64", head(up, user_params(d), 0) + [In(d["x"]), In(d["u"]), DevOnly(None), Out((N, B)), Out((B,))])
    pair(lib, h, "ddp_user_costfun_f64", head(up, user_params(d), 0) + [In(d["x"]), In(d["u"]), DevOnly(None), Out((N, B)), Raw(None)])
    pair(lib, h, "ddp_user_vhess_f64", head(up2) + [In(d["x"]), In(d["u"]), In(r.standard_normal((n, N, B))), DevOnly(None), Out((n + m, n + m, N, B))])
    for lims in (None, d["lims"]):
        out = pair(lib, h, "ddp_user_back_pass_f64", head(up2) + [In(d["x"]), In(d["u"])] + [In(a) for a in df] + [In(np.linspace(1.0, 2.0, B)), Raw(1),
                   In(lims), DevOnly(None), Out((m, n, N, B)), Out((m, N, B)), Out((m, m, N, B)), Out((n, N, B)), Out((n, n, N, B)), Out((2, B)),
                   Out((B,), np.int32)])
        assert not out[-1].any()


def test_user_drivers(lib, user):
    h, up, up2 = user
    d = lq_data()
    prm = user_params(d)
    o = ilqg_opts(lib)
    cap = 6
    head = lambda B_=B: [Raw(up), Raw(N), Raw(B_), In(prm), Raw(0), Raw(C.byref(o))]
    out = pair(lib, h, "ddp_user_ilqg_f64", head() + [In(d["x0"]), Raw(0), In(d["u"]), In(None), In(d["lims"])] + ilqg_outs() +
               [Raw(cap), Out((7, cap, B)), HostInt()])
    assert (out[8][1] >= 1).all()
    pair(lib, h, "ddp_user_ilqg_f64", head() + [In(out[0]), Raw(1), In(out[1]), In(out[7]), In(None)] + ilqg_outs() + [Raw(0), Raw(None), HostInt()])
    # the second-order problem reaches the driver through the same staging
    pair(lib, h, "ddp_user_ilqg_f64", [Raw(up2)] + head()[1:] + [In(d["x0"]), Raw(0), In(d["u"]), In(None), In(None)] + ilqg_outs() +
         [Raw(0), Raw(None), HostInt()])
    P_ = 5
    dq = lq_data(9, P_)
    pair(lib, h, "ddp_user_ilqg_queue_f64", head(P_) + [Raw(2), In(dq["x0"]), In(dq["u"]), In(None)] + ilqg_outs(P_) + [HostInt()])
    steps = 2
    pair(lib, h, "ddp_user_ilqg_mpc_f64", head() + [Raw(steps), Raw(1), In(d["x0"]), In(d["u"]), In(d["lims"]), Out((n, steps + 1, B)), Out((m, steps, B)),
                                                    Out((NSTATS, steps, B)), Out((n, N, B)), Out((m, N, B)), HostInt()])
    q = kl_inputs()
    ok = lib.ILQGKLOpts()
    lib.lib().ddp_ilqgkl_default_opts(C.byref(ok))
    ok.max_iter = 3
    for etab in (np.repeat(np.array([1e-8, 1.0, 1e16])[:, None], B, 1), None):
        pair(lib, h, "ddp_user_ilqgkl_f64", [Raw(up), Raw(N), Raw(B), In(prm), Raw(0)] + ilqgkl_args(lib, d, q, ok, etab, None))


@pytest.fixture(scope="module")
def user_fit(lib):
    """the same example made with DDP_USER_FITTED | DDP_USER_COST_FIT, on a handle of the module's own"""
    import ddp_amd
    hd = lib.Handle()
    p = ddp_amd.DeviceProblem(ddp_amd.example_source("lq_ad"), n, m, nparam=28, autodiff=True, fitted=True, cost_fit=True)
    yield hd, p._ptr(hd)
    hd.close()


def test_user_fitted_and_cost_model_entries(lib, user_fit):
    """ddp_user_rollout_fit, ddp_user_ilqgkl_fit and ddp_user_ilqgkl_cost (with the tables and with the three tables NULL): the tables are
    the model's own A, Bm with a small offset fc, the cost model the Hessians Q, R of the example and gradients at the nominal"""
    h, up = user_fit
    d, q = lq_data(), kl_inputs()
    prm = user_params(d)
    r = np.random.default_rng(12)
    rep = lambda a: np.ascontiguousarray(np.broadcast_to(a.reshape(a.shape + (1, 1)), a.shape + (N, B)))
    tabs = [rep(d["A"]) * (1.0 + 0.01 * r.standard_normal((n, n, N, B))), rep(d["Bm"]), 0.01 * r.standard_normal((n, N, B))]
    model = [np.einsum("ij,jtb->itb", d["Q"], d["x"]), np.einsum("ij,jtb->itb", d["R"], d["u"]), rep(d["Q"]), 0.01 * r.standard_normal((n, m, N, B)),
             rep(d["R"])]
    alpha = np.array([1.0, 0.5])
    pair(lib, h, "ddp_user_rollout_fit_f64", [Raw(up), Raw(N), Raw(B), In(prm), Raw(0), In(d["K"]), In(d["k"]), In(d["x0"]), In(d["u"]), In(d["x"]),
                                              Raw(lib_ptr(alpha)), Raw(2), In(d["lims"]), DevOnly(None)] + [In(a) for a in tabs] +
         [Out((n, N, B, 2)), Out((m, N, B, 2)), Out((N, B, 2)), Out((B, 2))])
    ok = lib.ILQGKLOpts()
    lib.lib().ddp_ilqgkl_default_opts(C.byref(ok))
    ok.max_iter = 3
    base = ilqgkl_args(lib, d, q, ok, np.repeat(np.array([1e-8, 1.0, 1e16])[:, None], B, 1), None)
    cut = next(i for i, a in enumerate(base) if isinstance(a, InOut)) + 1      # the tables go behind etab, the cost model behind iters
    head = [Raw(up), Raw(N), Raw(B), In(prm), Raw(0)]
    fit = pair(lib, h, "ddp_user_ilqgkl_fit_f64", head + base[:cut] + [In(a) for a in tabs] + base[cut:])
    assert (fit[-1][1] >= 1).all()
    for tables in (tabs, [None] * 3):
        out = pair(lib, h, "ddp_user_ilqgkl_cost_f64", head + base[:cut] + [In(a) for a in tables] + base[cut:] + [In(a) for a in model])
        assert (out[-1][1] >= 1).all()
