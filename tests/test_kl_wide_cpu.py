"""The wide KL path (ddp_kl_set_wide, kl.*(wide=True): n <= 64, m <= 32) without a GPU: the switch is declared, exported and bound;
ddp_gps_choice2 names the back_pass_gps kernel of every shape (ddp_gps_choice3: and of an incomplete call); out-of-range shapes are refused before anything touches the handle; the
keyword restores the switch; the cases of tests/kl_wide_cases.py are sound (two independent references agree, no loop case sits on a
tie of the reference, the limits bind); the GPS instantiation of back_pass_wide_kernel carries no more scratch than its twin."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest

import ddp_amd
from ddp_amd import _lib, kl

import kl_wide_cases as kc
from test_user_kl_cpu import _NoDevice

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WIDE = "back_pass_gps_wide"
STANDALONE, REGISTERED, USER = 0, 1, 2


def test_switch_is_declared_exported_and_bound():
    L = C.CDLL(_lib.LIB_PATH)
    hdr = open(os.path.join(ROOT, "include", "ddp_amd.h")).read()
    jl = open(os.path.join(ROOT, "differentialdynamicprogramming.jl_amd", "julia", "DDPAmd.jl")).read()
    assert re.search(r"\bint\s+ddp_kl_set_wide\s*\(\s*ddp_handle h,\s*int on\s*\)\s*;", hdr)
    assert hasattr(L, "ddp_kl_set_wide") and "ddp_kl_set_wide" in _lib.EXPORTS
    assert "ddp_kl_set_wide" in set(re.findall(r"@ccall\s+libddp\.(\w+)\(", jl))
    assert hasattr(L, "ddp_gps_choice2") and "ddp_gps_choice2" not in hdr                # an unlisted debug hook, like ddp_gps_choice
    assert hasattr(_lib.Handle, "set_kl_wide")
    import inspect
    for fn in (kl.grad_kl, kl.back_pass_gps, kl.forward_covariance, kl.kl_div_wiki, kl.calc_η, kl.iLQGkl, kl.demo_linear_kl):
        p = inspect.signature(fn).parameters["wide"]
        assert p.default is False and p.kind is inspect.Parameter.KEYWORD_ONLY, fn.__name__
    for head in ("∇kl(traj_prev", "back_pass_gps(cx", "forward_covariance(fx", "kl_div_wiki(xnew", "iLQGkl(problem::RegisteredProblem",
                 "iLQGkl(problem::DeviceProblem"):                  # (calc_η and the demo stay the reference's own Julia code)
        i = jl.index("function " + head)
        assert jl[i:jl.index(")\n    ", i) + 1].endswith("wide::Bool=false)"), head           # the signature, up to its closing parenthesis


# ------------------------------------------------------------------------------------------------------------- the choice table
def _desc(n, m):
    return _lib.BPDesc(n, m, 100, 16, 1, 1, 1, 1, 1, 0)


def _choice(n, m, caller, eta_tv=0):
    f = C.CDLL(_lib.LIB_PATH).ddp_gps_choice
    f.restype = C.c_char_p
    f.argtypes = [C.POINTER(_lib.BPDesc), C.c_int, C.c_int, C.c_char_p, C.c_char_p, C.c_char_p]
    return f(C.byref(_desc(n, m)), eta_tv, caller, None, None, None).decode()


def _choice2(n, m, caller, wide_on, gps_wide=None, eta_tv=0):
    f = C.CDLL(_lib.LIB_PATH).ddp_gps_choice2
    f.restype = C.c_char_p
    f.argtypes = [C.POINTER(_lib.BPDesc), C.c_int, C.c_int, C.c_char_p, C.c_char_p, C.c_char_p, C.c_int, C.c_char_p]
    return f(C.byref(_desc(n, m)), eta_tv, caller, None, None, None, wide_on, None if gps_wide is None else gps_wide.encode()).decode()


def _choice3(n, m, caller, complete, wide_on, gps_wide=None, eta_tv=0, N=100, mid=None):
    f = C.CDLL(_lib.LIB_PATH).ddp_gps_choice3
    f.restype = C.c_char_p
    f.argtypes = [C.POINTER(_lib.BPDesc), C.c_int, C.c_int, C.c_int, C.c_char_p, C.c_char_p, C.c_char_p, C.c_int, C.c_char_p]
    enc = lambda s: None if s is None else s.encode()                                   # noqa: E731
    return f(C.byref(_lib.BPDesc(n, m, N, 16, 1, 1, 1, 1, 1, 0)), eta_tv, caller, complete, enc(mid), None, None, wide_on, enc(gps_wide)).decode()


BEYOND = [(33, 1), (33, 8), (1, 9), (32, 9), (64, 32), (40, 20), (65, 1), (1, 33), (64, 33), (65, 32), (0, 1), (1, 0)]


@pytest.mark.parametrize("caller", [STANDALONE, REGISTERED, USER])
def test_choice_table(caller):
    for n in range(1, 33):
        for m in range(1, 9):
            for eta_tv in (0, 1):
                want = _choice(n, m, caller, eta_tv)
                assert _choice2(n, m, caller, 0, eta_tv=eta_tv) == want, (n, m)           # switch off: today's answers
                assert _choice2(n, m, caller, 1, eta_tv=eta_tv) == want, (n, m)           # switch on: small shapes keep their kernels
                assert _choice2(n, m, caller, 0, "1", eta_tv) == WIDE, (n, m)             # DDP_GPS_WIDE=1: the wide kernel everywhere
                assert _choice2(n, m, caller, 0, "0", eta_tv) == want, (n, m)
    for n, m in BEYOND:
        inside = 1 <= n <= 64 and 1 <= m <= 32
        assert _choice2(n, m, caller, 0) == "none", (n, m)
        assert _choice2(n, m, caller, 0, "1") == "none", (n, m)                           # the environment does not open the large shapes
        assert _choice2(n, m, caller, 1) == (WIDE if inside else "none"), (n, m)
        assert _choice2(n, m, caller, 1, "1") == (WIDE if inside else "none"), (n, m)
    for n in range(1, 65):                                                                # wide exactly when n > 32 or m > 8
        for m in range(1, 33):
            assert (_choice2(n, m, caller, 1) == WIDE) == (n > 32 or m > 8), (n, m)


@pytest.mark.parametrize("caller", [STANDALONE, REGISTERED, USER])
def test_choice_with_an_incomplete_kl_argument(caller):
    """ddp_gps_choice3 carries the fact the dispatcher has always looked at first: a `kl` with a pointer missing (or limits without lims
    and u) goes to the generic kernel, whose launcher words the refusal — inside the box whatever the shape, the step sizes and the
    switches say, and for the wide shapes too; a complete call answers as ddp_gps_choice2 does"""
    for n in range(1, 33):
        for m in range(1, 9):
            for eta_tv in (0, 1):
                for wide_on in (0, 1):
                    for N in (1, 100):
                        assert _choice3(n, m, caller, 0, wide_on, eta_tv=eta_tv, N=N) == "back_pass_gps", (n, m)
                assert _choice3(n, m, caller, 0, 0, "1", eta_tv) == "back_pass_gps", (n, m)           # DDP_GPS_WIDE=1
                assert _choice3(n, m, caller, 0, 0, eta_tv=eta_tv, mid="1") == "back_pass_gps", (n, m)   # DDP_GPS_MID=1
                assert _choice3(n, m, caller, 1, 0, eta_tv=eta_tv) == _choice2(n, m, caller, 0, eta_tv=eta_tv), (n, m)
                assert _choice3(n, m, caller, 1, 0, "1", eta_tv) == WIDE, (n, m)
    for n, m in BEYOND:
        inside = 1 <= n <= 64 and 1 <= m <= 32
        assert _choice3(n, m, caller, 0, 0) == "none", (n, m)                                        # refused by the shape check first
        assert _choice3(n, m, caller, 0, 1) == ("back_pass_gps" if inside else "none"), (n, m)
        assert _choice3(n, m, caller, 1, 1) == (WIDE if inside else "none"), (n, m)


# ------------------------------------------------------------------------------------------------ refusals before any launch
def _policy(n, m, N, B=None):
    tb = () if B is None else (B,)
    return ddp_amd.GaussianPolicy(N, n, m, np.zeros((m, n, N) + tb), np.zeros((m, N) + tb), np.zeros((m, m, N) + tb), np.zeros((m, m, N) + tb))


def _calls(n, m, wide, handle):
    """every function with the keyword at shape (n, m): nothing but the extents is valid, nothing may reach the handle"""
    N = 4
    z = np.zeros
    pol = _policy(n, m, N)
    terms = (z((n, N)), z((m, N)), z((n, n, N)), z((m, n, N)), z((m, m, N)))
    kw = dict(handle=handle, wide=wide)
    return {
        "grad_kl": lambda: kl.grad_kl(pol, **kw),
        "back_pass_gps": lambda: kl.back_pass_gps(z((n, N)), z((m, N)), z((n, n, N)), z((n, m, N)), z((m, m, N)), z((n, n, N)), z((n, m, N)), None,
                                                  z((n, N)), z((m, N)), (terms, np.array([1e-8, 1.0, 1e16])), **kw),
        "forward_covariance": lambda: kl.forward_covariance(kl.Model(z((n, n, N)), None, np.eye(n)), None, None, pol, **kw),
        "kl_div_wiki": lambda: kl.kl_div_wiki(z((n, N)), z((n, N)), z((n + m, n + m, N)), pol, pol, **kw),
        "calc_η": lambda: kl.calc_η(z((n, N)), z((n, N)), z((n + m, n + m, N)), np.array([1e-8, 1.0, 1e16]), pol, pol, 1.0, **kw),
        "iLQGkl": lambda: kl.iLQGkl(ddp_amd.LQProblem(np.eye(n), z((n, m)), np.eye(n), np.eye(m)), z((n, N)), pol,
                                    kl.Model(z((n, n, N)), None, np.eye(n)), cost=1.0, **kw),
        "demo_linear_kl": lambda: kl.demo_linear_kl(n=n, m=m, T=N, **kw),
    }


@pytest.mark.parametrize("n,m,wide", [(10, 9, False), (33, 2, False), (65, 2, True), (10, 33, True)])
def test_refusals_before_any_launch(n, m, wide):
    for name, call in _calls(n, m, wide, _NoDevice()).items():
        with pytest.raises(ddp_amd.DDPError, match=r"n=%d m=%d has no back_pass_gps kernel .*n <= 64, m <= 32" % (n, m)):
            call()


def test_second_order_problem_stays_refused():
    p = ddp_amd.DeviceProblem(ddp_amd.example_source("lq_ad"), 10, 2, nparam=224, autodiff=True, second_order=True)
    with pytest.raises(ddp_amd.DDPError, match="second_order"):
        kl.iLQGkl(p, np.zeros((10, 5)), _policy(10, 2, 5), kl.Model(None, None, np.eye(10)), cost=1.0, wide=True, handle=_NoDevice())


def test_user_problem_extents_are_checked_before_any_launch_at_large_shapes():
    p = ddp_amd.DeviceProblem(ddp_amd.example_source("lq"), 40, 12, nparam=2 * 40 * 40 + 40 * 12 + 12 * 12, wave=True)
    n, m, N = 40, 12, 6
    ok = dict(cost=np.zeros(N), params=np.zeros(p.nparam), handle=_NoDevice(), wide=True)
    with pytest.raises(ddp_amd.DDPError, match="R1"):
        kl.iLQGkl(p, np.zeros((n, N)), _policy(n, m, N), kl.Model(None, None, np.eye(n - 1)), **ok)
    with pytest.raises(ddp_amd.DDPError, match="n = 40, m = 12"):
        kl.iLQGkl(p, np.zeros((n + 1, N)), _policy(n + 1, m, N), kl.Model(None, None, np.eye(n + 1)), **ok)


# ------------------------------------------------------------------------------------------------------------- switch restore
class _FakeHandle:
    """records the switch; `raw` either works (a stub library takes the call) or raises, as a failing launch would"""
    def __init__(self, start, fail):
        self.state, self.fail, self.seen = start, fail, []

    def set_kl_wide(self, on):
        was, self.state = self.state, bool(on)
        return was

    @property
    def raw(self):
        self.seen.append(self.state)
        if self.fail:
            raise RuntimeError("launch failed")
        return None


class _StubLib:
    def __getattr__(self, name):
        return lambda *a: 0


@pytest.mark.parametrize("start", [False, True])
def test_keyword_restores_the_switch(monkeypatch, start):
    pol = _policy(40, 12, 3)
    h = _FakeHandle(start, fail=True)
    with pytest.raises(RuntimeError, match="launch failed"):
        kl.grad_kl(pol, handle=h, wide=True)
    assert h.seen == [True] and h.state is start                     # on during the call, back after the exception
    monkeypatch.setattr(_lib, "lib", lambda: _StubLib())
    h = _FakeHandle(start, fail=False)
    kl.grad_kl(pol, handle=h, wide=True)
    assert h.seen == [True] and h.state is start                     # and after a call that returns
    h = _FakeHandle(start, fail=False)
    kl.grad_kl(_policy(10, 2, 3), handle=h)
    assert h.seen == [start] and h.state is start                    # without the keyword the switch is left alone


# ------------------------------------------------------------------------------------------------------------- the cases
@pytest.mark.parametrize("n,m", kc.SHAPES + kc.SMALL)
def test_references_agree_on_single_pass_cases(n, m):
    """the C oracle and the NumPy restatement, written independently, agree to 1e-10 on every configuration"""
    from conftest import relerr
    seen_div = False
    for ci in range(len(kc.CONFIGS)):
        for b, (a, r) in enumerate(zip(kc.gps_reference(n, m, ci), kc.gps_reference_numpy(n, m, ci))):
            assert a["diverge"] == r["diverge"], (ci, b)
            seen_div |= a["diverge"] > 0
            for key in ("K", "k", "Quu", "Quui", "Vx", "Vxx"):
                assert relerr(a[key], r[key]) < 1e-10, (ci, b, key, relerr(a[key], r[key]))
            assert relerr(a["dV"], r["dV"], 0) < 1e-10, (ci, b)
    assert seen_div


@pytest.mark.parametrize("n,m", kc.SHAPES)
def test_limits_bind_in_single_pass_cases(n, m):
    for ci, cfg in enumerate(kc.CONFIGS):
        if cfg[2]:
            share = kc.clamped_share(n, m, ci)
            print("clamped share (%d, %d) configuration %d: %.3f" % (n, m, ci, share))
            assert share > 0.05, (ci, share)


@pytest.mark.parametrize("n,m,T,lims", kc.LOOPS)
def test_loop_cases_are_not_at_a_tie_of_the_reference(n, m, T, lims):
    ref = kc.loop_reference(n, m, T, lims)
    for b in range(kc.LOOP_B):
        want = kc.outcome(ref[b][6])
        near = kc.loop_outcomes_nearby(n, m, T, lims, b, 1000 * n + m + b)
        assert all(o == want for o in near), (b, want, near)
        if lims and b > 0:
            print("share on a bound (%d, %d, %d) trajectory %d: %.3f" % (n, m, T, b, kc.loop_bound_share(n, m, T, b)))


# ------------------------------------------------------------------------------------------------------------- resource records
def test_gps_instantiation_of_the_wide_kernel_spills_no_more_than_its_twin():
    f = os.path.join(ROOT, "differentialdynamicprogramming.jl_amd", "build", "back_pass_wide.o.usage.json")
    assert os.path.exists(f), "no build/back_pass_wide.o.usage.json: build first"
    recs = json.load(open(f))
    gps = [v for k, v in recs.items() if "back_pass_wide_kernelILb1E" in k]
    twin = [v for k, v in recs.items() if "back_pass_wide_kernelILb0E" in k]
    assert len(gps) == 1 and len(twin) == 1, sorted(recs)
    assert int(gps[0]["ScratchSize"]) <= int(twin[0]["ScratchSize"]), (gps[0], twin[0])


def test_wide_kl_kernels_hold_no_scratch():
    """no per-thread array sized by n or m: the three kernels of kl_wide.hip (and the mean) need no scratch memory at all"""
    f = os.path.join(ROOT, "differentialdynamicprogramming.jl_amd", "build", "kl_wide.o.usage.json")
    assert os.path.exists(f), "no build/kl_wide.o.usage.json: build first"
    recs = json.load(open(f))
    for name in ("kl_terms_wide_kernel", "fcov_wide_kernel", "kl_div_wide_kernel", "kl_mean_wide_kernel"):
        hit = [v for k, v in recs.items() if name in k]
        assert len(hit) == 1, (name, sorted(recs))
        assert int(hit[0]["ScratchSize"]) == 0, (name, hit[0])
