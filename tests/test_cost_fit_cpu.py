"""DDP_USER_COST_FIT without a GPU: the reference of tests/cost_fit_reference.py (quadratic exactness in long double, one sample on the
nominal, the wrapped difference), the conditioning of every designed case of the GPU tests (float64 twin against long double), the flag,
the four new exports and their prototypes, the program text (append-only, behind the fitted tail), the refused combinations, the compile
report of ddp_user_cost_fit and what Python refuses before it needs a device."""
import inspect
import os
import re

import numpy as np
import pytest

import ddp_amd
from ddp_amd import _lib, kl

import cost_fit_reference as cr
from conftest import ROOT, relerr

COST_FIT, FITTED, SAMPLE, TERMINAL, CONST_H, AUTODIFF, PLANT, SECOND, WAVE, SECOND_WAVE, CLOCK, CONSTRAINTS = (8192, 4096, 2048, 1, 2, 4, 8, 16, 32, 128,
                                                                                                               512, 1024)
NEW = ("ddp_user_cost_fit_f64_dev", "ddp_user_cost_fit_f64", "ddp_user_ilqgkl_cost_f64_dev", "ddp_user_ilqgkl_cost_f64")
LQ_NP = cr.LQ_NP
LD = np.longdouble
HDR = os.path.join(ROOT, "include", "ddp_amd.h")
JL = os.path.join(ROOT, "differentialdynamicprogramming.jl_amd", "julia", "DDPAmd.jl")


# ------------------------------------------------------------------------------------------------------------------------ the reference
def _lq_samples(rng, n, m, N, S):
    Q, R, M = cr._spd(rng, n).astype(LD), cr._spd(rng, m).astype(LD), rng.standard_normal((n, m)).astype(LD)     # with a cross term x'Mu
    x, u = rng.standard_normal((n, N)).astype(LD), rng.standard_normal((m, N)).astype(LD)
    xs, us = x[:, :, None] + rng.standard_normal((n, N, S)), u[:, :, None] + rng.standard_normal((m, N, S))

    def expansion(X, U):                                         # the closed form at the columns of X[n,T], U[m,T], in long double
        c = (np.einsum("it,ij,jt->t", X, Q, X) + np.einsum("it,ij,jt->t", U, R, U)) / 2 + np.einsum("it,ij,jt->t", X, M, U)
        return c, Q @ X + M @ U, R @ U + M.T @ X
    return Q, R, M, x, u, xs, us, expansion


def test_a_quadratic_cost_is_reproduced_at_the_nominal():
    rng = np.random.default_rng(3)
    n, m, N, S = 5, 3, 4, 7
    Q, R, M, x, u, xs, us, expansion = _lq_samples(rng, n, m, N, S)
    per = [expansion(xs[:, :, s], us[:, :, s]) for s in range(S)]
    c, cx, cu = (np.stack([p[k] for p in per], -1) for k in range(3))
    rep = lambda A: np.repeat(np.repeat(A[:, :, None, None], N, 2), S, 3)          # noqa: E731
    out = cr.fit_cost(c, cx, cu, rep(Q), rep(M), rep(R), xs, us, x, u)
    assert all(a.dtype == LD for a in out)
    c0, cx0, cu0 = expansion(x, u)
    for got, want in zip(out, (cx0, cu0, rep(Q)[..., 0], rep(M)[..., 0], rep(R)[..., 0], c0)):
        err = float(np.max(np.abs(got - want)) / np.max(np.abs(want)))
        assert err < 1e-15, err


def test_one_sample_on_the_nominal_gives_its_derivatives():
    rng = np.random.default_rng(4)
    n, m, N = 3, 2, 5
    x, u = rng.standard_normal((n, N)), rng.standard_normal((m, N))
    d = [rng.standard_normal(s + (N, 1)) for s in ((), (n,), (m,), (n, n), (n, m), (m, m))]
    out = cr.fit_cost(*d, x[:, :, None], u[:, :, None], x, u, dtype=np.float64)
    for got, want in zip(out, (d[1], d[2], d[3], d[4], d[5], d[0])):
        assert np.array_equal(got, want[..., 0])


def test_the_wrapped_coordinate_uses_the_wrapped_difference():
    rng = np.random.default_rng(5)
    n, m, N, S = 2, 1, 3, 4
    Q, R, M, x, u, xs, us, expansion = _lq_samples(rng, n, m, N, S)
    d = [rng.standard_normal(s + (N, S)) for s in ((), (n,), (m,), (n, n), (n, m), (m, m))]
    moved = xs.copy()
    moved[0] += cr.TWO_PI * np.array([-1, 0, 1, 2])[None, :]                     # coordinate 0: the same points modulo 2π
    plain = cr.fit_cost(*d, xs, us, x, u, wrap=0)
    for got, want in zip(cr.fit_cost(*d, moved, us, x, u, wrap=1), plain):
        assert float(np.max(np.abs(got - want))) < 1e-16 * 50
    other = cr.fit_cost(*d, moved, us, x, u, wrap=0)                             # without the mask the raw difference is taken
    assert float(np.max(np.abs(other[0] - plain[0]))) > 1.0
    moved1 = xs.copy(); moved1[1] += cr.TWO_PI                                   # coordinate 1 is not wrapped by mask 1
    assert float(np.max(np.abs(cr.fit_cost(*d, moved1, us, x, u, wrap=1)[0] - plain[0]))) > 1.0


@pytest.mark.parametrize("name,N,B,S", cr.SIZES, ids=cr.IDS)
def test_designed_cases_are_well_conditioned(name, N, B, S):
    """the condition on the inputs of the GPU tests: the float64 twin (the kernel's order) within 1e-10 of long double, every trajectory"""
    case = cr.make_case(ddp_amd, name, N, B, S)
    if N is None:
        lanes, chunk, csb = cr.layout(ddp_amd, cr.problem_of(ddp_amd, name))
        assert (case["N"], case["S"]) == (chunk + 1, csb + 1) and case["B"] == lanes // chunk + 1
    worst = 0.0
    for b in range(case["B"]):
        d = cr.host_derivatives(case, b)
        args = (case["xs"][..., b], case["us"][..., b], case["x"][..., b], case["u"][..., b], case["wrap"])
        for a, r in zip(cr.fit_cost(*d, *args, dtype=np.float64), cr.fit_cost(*d, *args)):
            worst = max(worst, relerr(a, r.astype(float), 0 if r.ndim == 1 else -1))
    print(name, case["N"], case["B"], case["S"], "twin against long double: %.2e" % worst)
    assert worst < 1e-10, worst


# --------------------------------------------------------------------------------------------------------- flag, exports, prototypes
def test_flag_value_everywhere():
    hdr, jl = open(HDR).read(), open(JL, encoding="utf-8").read()
    assert _lib.USER_COST_FIT == 8192
    assert re.search(r"\bDDP_USER_COST_FIT = 8192\b", hdr)
    assert re.search(r"^const USER_COST_FIT = 8192\b", jl, flags=re.M)
    assert re.search(r"cost_fit::Bool=false", jl) and re.search(r"\(cost_fit \? USER_COST_FIT : 0\)", jl)
    assert ddp_amd.DeviceProblem("", 1, 1, cost_fit=True).flags == 8192 and ddp_amd.DeviceProblem("", 1, 1).flags == 0
    assert ddp_amd.DeviceProblem("", 1, 1, cost_fit=True, fitted=True, sample=True, terminal=True).flags == 8192 | 4096 | 2048 | 1


def _c_arity(hdr, name):
    mm = re.search(r"\bint %s\s*\(([^;]*?)\);" % name, hdr, flags=re.S)
    assert mm, name
    return len([a for a in mm.group(1).split(",") if a.strip()])


def _jl_arity(jl, name):
    """arguments of every `@ccall libddp.<name>(...)::Cint` of the Julia binding"""
    out = []
    for mm in re.finditer(r"@ccall libddp\.%s\(" % name, jl):
        depth, i = 1, mm.end()
        while depth:
            depth += {"(": 1, ")": -1}.get(jl[i], 0)
            i += 1
        body = jl[mm.end():i - 1]
        flat, d = "", 0
        for ch in body:                                          # commas of nested calls such as _ptr_or_null(P) and (ndims(f) == 4) do not count
            d += {"(": 1, ")": -1}.get(ch, 0)
            flat += ch if d == 0 or ch not in "," else " "
        out.append(len([a for a in flat.split(",") if a.strip()]))
    return out


def test_new_names_are_declared_exported_bound_and_called():
    hdr, jl = open(HDR).read(), open(JL, encoding="utf-8").read()
    L = _lib.lib()
    for name in NEW:
        assert name in _lib.EXPORTS and hasattr(L, name) and re.search(r"\b%s\s*\(" % name, hdr), name
        nc = _c_arity(hdr, name)
        assert len(getattr(L, name).argtypes) == nc, (name, nc, len(getattr(L, name).argtypes))
        calls = _jl_arity(jl, name)
        assert calls and all(k == nc for k in calls), (name, nc, calls)
    assert _c_arity(hdr, NEW[0]) == 17 and _c_arity(hdr, NEW[2]) == _c_arity(hdr, "ddp_user_ilqgkl_fit_f64_dev") + 5
    assert "cost_model" in inspect.signature(kl.iLQGkl).parameters and "fit_cost" in ddp_amd.__all__
    assert re.search(r"^function fit_cost\(problem::DeviceProblem, xs, us, x, u;", jl, flags=re.M) and "cost_model=nothing" in jl


# ------------------------------------------------------------------------------------------------------------------- the program text
def _text(src, n, m, nparam, flags, wrap=0):
    t = _lib.lib().ddp_user_program_text(src.encode(), n, m, nparam, flags, wrap)
    return None if t is None else t.decode()


TEXTS = [("car", 4, 2, 9, TERMINAL, 0), ("car_ad", 4, 2, 9, TERMINAL | AUTODIFF | SECOND, 0), ("car_plant", 4, 2, 13, TERMINAL | PLANT, 0),
         ("pendcart", 4, 1, 25, TERMINAL, 1), ("lq", 32, 8, LQ_NP(32, 8), CONST_H, 0), ("lq_ad", 5, 3, LQ_NP(5, 3), AUTODIFF, 0)]


@pytest.mark.parametrize("other", [0, SAMPLE | FITTED], ids=["plain", "sample-fitted"])
@pytest.mark.parametrize("ex,n,m,nparam,flags,wrap", TEXTS, ids=[t[0] for t in TEXTS])
def test_program_text_is_appended_only(ex, n, m, nparam, flags, wrap, other):
    src = ddp_amd.example_source(ex)
    base, with_flag = _text(src, n, m, nparam, flags | other, wrap), _text(src, n, m, nparam, flags | other | COST_FIT, wrap)
    assert base and with_flag and with_flag.startswith(base) and len(with_flag) > len(base)
    tail = with_flag[len(base):]
    assert "ddp_user_cost_fit" in tail and "UserCostFitArgs" in tail and "ddp_user_rollout_fit" not in tail and "ddp_user_sample" not in tail
    if other:
        assert "ddp_user_rollout_fit" in base and base.rstrip().endswith("}")                              # behind the fitted tail
    lanes, chunk, csb = (int(re.search(r"#define %s (\d+)\b" % k, tail).group(1)) for k in ("DDP_CLANES", "DDP_CCHUNK", "DDP_CSB"))
    dc = n + m + n * n + n * m + m * m
    assert 1 <= chunk <= lanes <= 64 and lanes % chunk == 0 and csb >= 1
    assert lanes * (((2 * dc + 1 + (csb + 1) * (n + m)) | 1) + 1) * 8 <= 64 * 1024
    assert "ddp_user_cost_fit" not in base and "DDP_CLANES" not in base


@pytest.mark.parametrize("n,m", [(1, 1), (4, 2), (10, 2), (17, 5), (32, 1), (32, 8), (1, 8), (31, 7)])
def test_layout_fits_lds_over_the_box(n, m):
    t = _text(ddp_amd.example_source("lq"), n, m, LQ_NP(n, m), COST_FIT)
    lanes, chunk, csb = (int(re.search(r"#define %s (\d+)\b" % k, t).group(1)) for k in ("DDP_CLANES", "DDP_CCHUNK", "DDP_CSB"))
    dc = n + m + n * n + n * m + m * m
    assert lanes >= 1 and lanes * (((2 * dc + 1 + (csb + 1) * (n + m)) | 1) + 1) * 8 <= 64 * 1024, (lanes, chunk, csb)


def test_no_program_without_the_flag_mentions_the_kernel():
    texts = [_text(ddp_amd.example_source("car"), 4, 2, 9, TERMINAL), _text(ddp_amd.example_source("car"), 4, 2, 9, TERMINAL | SAMPLE | FITTED),
             _text(ddp_amd.example_source("lq_ad"), 5, 3, LQ_NP(5, 3), AUTODIFF | SECOND),
             _text(ddp_amd.example_source("chain_ad"), 16, 8, 7, AUTODIFF | WAVE),
             _text(ddp_amd.example_source("chain_ddp_ad"), 24, 12, 8, AUTODIFF | WAVE | SECOND_WAVE),
             _text(ddp_amd.example_source("car_track"), 4, 2, 7 + 4 * 8, TERMINAL | CLOCK),
             _lib.lib().ddp_user_program_text_c(ddp_amd.example_source("car_keepout_ad").encode(), 4, 2, 10, 2, TERMINAL | AUTODIFF | CONSTRAINTS, 0)]
    texts = [t.decode() if isinstance(t, bytes) else t for t in texts]
    assert all(texts), "arguments that are legal without the flag were refused: %s" % _lib.lib().ddp_last_error().decode()
    for t in texts:
        assert "ddp_user_cost_fit" not in t and "DDP_CLANES" not in t and "DDP_CSB" not in t and "UserCostFitArgs" not in t and "ddp_cf_" not in t


# --------------------------------------------------------------------------------------------------------------------------- refusals
@pytest.mark.parametrize("ex,n,m,nparam,nc,flags,words", [
    ("chain_ad", 16, 8, 7, 0, COST_FIT | AUTODIFF | WAVE, ("DDP_USER_COST_FIT | DDP_USER_WAVE", "deferred", "n <= 32", "m <= 8")),
    ("chain_ddp_ad", 16, 8, 8, 0, COST_FIT | AUTODIFF | WAVE | SECOND_WAVE, ("DDP_USER_COST_FIT | DDP_USER_SECOND_ORDER_WAVE", "deferred", "n <= 32")),
    ("car_track", 4, 2, 39, 0, COST_FIT | TERMINAL | CLOCK, ("DDP_USER_COST_FIT | DDP_USER_CLOCK", "deferred", "no clock")),
    ("car_keepout_ad", 4, 2, 10, 2, COST_FIT | TERMINAL | AUTODIFF | CONSTRAINTS, ("DDP_USER_COST_FIT | DDP_USER_CONSTRAINTS", "deferred", "no multipliers")),
    ("car", 4, 2, 9, 0, COST_FIT | 64, ("unknown flags",)), ("car", 4, 2, 9, 0, COST_FIT | 256, ("unknown flags",)),
    ("lq", 33, 8, LQ_NP(33, 8), 0, COST_FIT, ("n = 33",)), ("lq", 8, 9, LQ_NP(8, 9), 0, COST_FIT, ("m = 9",))])
def test_refused_by_name_before_compiling(ex, n, m, nparam, nc, flags, words):
    L = _lib.lib()
    src = ddp_amd.example_source(ex).encode()
    rc = L.ddp_user_check_c(src, n, m, nparam, nc, flags, None) if nc else L.ddp_user_check(src, n, m, nparam, flags, None)
    err = L.ddp_last_error().decode()
    assert rc == -1, (rc, err)                                   # -1: refused by validate(); the compiler (-4) was never asked
    for w in words:
        assert w in err, err


LEGAL = [("car_plant", 4, 2, 13, dict(terminal=True, plant=True, sample=True, fitted=True)),
         ("car_ad", 4, 2, 9, dict(terminal=True, autodiff=True, second_order=True)),
         ("lq_ad", 5, 3, LQ_NP(5, 3), dict(autodiff=True, const_hessian=True)),
         ("pendcart", 4, 1, 25, dict(terminal=True, diff=ddp_amd.WrappedDiff(0)))]


@pytest.mark.parametrize("ex,n,m,nparam,kw", LEGAL, ids=[c[0] for c in LEGAL])
def test_legal_combinations_compile(ex, n, m, nparam, kw):
    ddp_amd.DeviceProblem(ddp_amd.example_source(ex), n, m, nparam=nparam, cost_fit=True, **kw).check()


# -------------------------------------------------------------------------------------------------------------------------- resources
def _usage(log, kernel):
    """the figures of one kernel from the kernel-resource-usage remarks of a hiprtc log"""
    out, cur = {}, None
    for line in log.splitlines():
        mm = re.search(r"remark: Function Name: (\w+)", line)
        if mm:
            cur = mm.group(1)
        mm = re.search(r"remark:\s+([A-Za-z][\w \[\]/]*): (\d+)", line)
        if mm and cur == kernel and "Function Name" not in mm.group(1):
            out[mm.group(1).strip()] = int(mm.group(2))
    return out


@pytest.mark.parametrize("ex,n,m,nparam,kw", [("car", 4, 2, 9, dict(terminal=True)), ("lq", 10, 2, LQ_NP(10, 2), {}),
                                              ("lq", 32, 8, LQ_NP(32, 8), dict(const_hessian=True)),
                                              ("car_ad", 4, 2, 9, dict(terminal=True, autodiff=True))], ids=["4x2", "10x2", "32x8", "4x2-ad"])
def test_cost_fit_fits_lds_without_spills_and_with_no_more_scratch_than_df(ex, n, m, nparam, kw):
    log = ddp_amd.DeviceProblem(ddp_amd.example_source(ex), n, m, nparam=nparam, cost_fit=True, **kw).check("-Rpass-analysis=kernel-resource-usage")
    u, d = _usage(log, "ddp_user_cost_fit"), _usage(log, "ddp_user_df_ad" if kw.get("autodiff") else "ddp_user_df")
    print(u)
    assert u and d, log[:2000]
    assert u["LDS Size [bytes/block]"] <= 64 * 1024 and u["VGPRs Spill"] == 0, u
    assert u["ScratchSize [bytes/lane]"] <= d["ScratchSize [bytes/lane]"], (u, d)


# ------------------------------------------------------------------------------------------------------------------- Python refusals
def test_python_refuses_what_it_can_without_a_device():
    import fitted_reference as fr
    case = fr.loop_case()
    src = ddp_amd.example_source("car")
    plain = ddp_amd.DeviceProblem(src, 4, 2, nparam=9, terminal=True, params=case["P"])
    cf = ddp_amd.DeviceProblem(src, 4, 2, nparam=9, terminal=True, params=case["P"], cost_fit=True)
    N, B, S = case["N"], case["B"], 4
    xs, us = np.zeros((4, N, S, B)), np.zeros((2, N, S, B))
    with pytest.raises(TypeError, match=r"fit_cost: a DeviceProblem is needed"):
        ddp_amd.fit_cost(ddp_amd.LQProblem(np.eye(2), np.ones((2, 1)), np.eye(2), np.eye(1)), xs, us, case["x"], case["u"])
    with pytest.raises(ddp_amd.DDPError, match=r"made with cost_fit=True"):
        ddp_amd.fit_cost(plain, xs, us, case["x"], case["u"])
    with pytest.raises(ddp_amd.DDPError, match=r"xs, us should be"):
        ddp_amd.fit_cost(cf, xs[..., 0, 0], us, case["x"], case["u"])
    with pytest.raises(ddp_amd.DDPError, match=r"does not match xs"):
        ddp_amd.fit_cost(cf, xs, us[:, :, :3], case["x"], case["u"])
    with pytest.raises(ddp_amd.DDPError, match=r"x, u should be"):
        ddp_amd.fit_cost(cf, xs, us, case["x"][:, :-1], case["u"])
    with pytest.raises(ddp_amd.DDPError, match=r"x, u should be"):
        ddp_amd.fit_cost(cf, xs, us, case["x"][..., 0], case["u"][..., 0])
    with pytest.raises(ddp_amd.DDPError, match=r"compiled for n = 4, m = 2"):
        ddp_amd.fit_cost(cf, np.zeros((3, N, S, B)), us, np.zeros((3, N, B)), case["u"])
    # kl.iLQGkl(..., cost_model=)
    prev = ddp_amd.GaussianPolicy(N, 4, 2, case["Kp"], case["u"], case["Sp"], case["Sip"])
    model = kl.Model(None, None, case["R1"])
    tabs = [np.zeros(s + (N, B)) for s in ((4,), (2,), (4, 4), (4, 2), (2, 2))]
    call = lambda p, cm, **kw: kl.iLQGkl(p, case["x"], prev, model, kl_step=0.5, max_iter=3, cost=case["c"], cost_model=cm, **kw)   # noqa: E731
    with pytest.raises(ddp_amd.DDPError, match=r"cost_model= together with wide=True"):
        call(plain, tabs, wide=True)
    with pytest.raises(ddp_amd.DDPError, match=r"cost_model= needs a DeviceProblem"):
        kl.iLQGkl(ddp_amd.LQProblem(np.eye(4), np.ones((4, 2)), np.eye(4), np.eye(2)), case["x"], prev, kl.Model(case["fx"], case["fu"], case["R1"]),
                  cost=case["c"], cost_model=tabs)
    with pytest.raises(ddp_amd.DDPError, match=r"five arrays"):
        call(plain, tabs[:4])
    with pytest.raises(ddp_amd.DDPError, match=r"cx, cu, cxx, cxu, cuu should be"):
        call(plain, tabs[:3] + [np.zeros((2, 4, N, B))] + tabs[4:])
    with pytest.raises(ddp_amd.DDPError, match=r"one cost model per trajectory"):
        call(plain, [t[..., 0] for t in tabs])
    bad = [t.copy() for t in tabs]
    bad[2][1, 0, 17, 2] = np.nan; bad[2][0, 0, 30, 2] = np.inf
    with pytest.raises(ddp_amd.DDPError, match=r"cxx is not finite at step 17 of trajectory 2"):
        call(plain, bad)
    with pytest.raises(ddp_amd.DDPError, match=r"made with fitted=True"):
        call(plain, tabs, fitted=True)
