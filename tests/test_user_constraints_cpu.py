"""DDP_USER_CONSTRAINTS (DeviceProblem(..., constraints=nc)) without a GPU: every refusal by its message, the keep-out example compiles for
gfx950 as a lane and as a wave problem with no scratch in the two new kernels, a problem without the flag compiles the text it always
did, the wrapper text of csrc/user_constraints.h built for the host gives ψ, its gradient and its Hessian through the nested duals as the
longdouble closed forms do, and the NumPy augmented-Lagrangian loop that the GPU tests compare with behaves on the designed inputs."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import ddp_amd
from ddp_amd import _lib
import constraints_cases as cc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "differentialdynamicprogramming.jl_amd")
TERMINAL, CONST_HESSIAN, AUTODIFF, PLANT, SECOND, WAVE, SECOND_WAVE, CLOCK, CONSTRAINTS = 1, 2, 4, 8, 16, 32, 128, 512, 1024
BASE = TERMINAL | AUTODIFF | CONSTRAINTS
SRC = ddp_amd.example_source("car_keepout_ad")


def _check_c(src, nc, flags, nparam=cc.NPARAM, extra=None):
    L = _lib.lib()
    rc = L.ddp_user_check_c(src.encode(), 4, 2, nparam, nc, flags, extra.encode() if extra else None)
    return rc, L.ddp_last_error().decode(), L.ddp_user_compile_log().decode()


@pytest.mark.parametrize("src,nc,flags,words", [
    (SRC, 2, TERMINAL | CONSTRAINTS, ("DDP_USER_CONSTRAINTS", "needs DDP_USER_AUTODIFF")),
    (SRC, 2, BASE | CONST_HESSIAN, ("DDP_USER_CONSTRAINTS", "DDP_USER_CONST_HESSIAN")),
    (SRC, 2, BASE | CLOCK, ("DDP_USER_CONSTRAINTS", "DDP_USER_CLOCK")),
    (SRC, 2, BASE | SECOND, ("DDP_USER_CONSTRAINTS", "DDP_USER_SECOND_ORDER is refused")),
    (SRC, 2, BASE | WAVE | SECOND_WAVE, ("DDP_USER_CONSTRAINTS", "DDP_USER_SECOND_ORDER_WAVE")),
    (SRC.replace("constraints", "path_limits"), 2, BASE, ("defines no `constraints`",)),
    (SRC, 0, BASE, ("nc = 0 out of [1, 16]", "DDP_USER_MAX_NC")),
    (SRC, 17, BASE, ("nc = 17 out of [1, 16]",)),
    (SRC, 2, TERMINAL | AUTODIFF, ("nc = 2 but DDP_USER_CONSTRAINTS is not set",)),
    (SRC, 2, BASE | 64, ("unknown flags",)),
    (SRC, 2, BASE | 256, ("unknown flags",)),
])
def test_refusals_name_their_cause(src, nc, flags, words):
    rc, err, _ = _check_c(src, nc, flags)
    assert rc == -1, (rc, err)                                   # refused before compiling
    for w in words:
        assert w in err, err


def test_the_old_entries_refuse_the_flag_and_point_at_the_new_ones():
    L = _lib.lib()
    rc = L.ddp_user_check(SRC.encode(), 4, 2, cc.NPARAM, BASE, None)
    err = L.ddp_last_error().decode()
    assert rc == -1 and "DDP_USER_CONSTRAINTS" in err and "ddp_user_check_c" in err and "ddp_user_create_c" in err, err
    for flags in (64, 256):                                      # the bits next to it stay unknown, in the old entry too
        rc = L.ddp_user_check(ddp_amd.example_source("car_ad").encode(), 4, 2, 9, flags | TERMINAL | AUTODIFF, None)
        assert rc == -1 and "unknown flags" in L.ddp_last_error().decode()
    # the new entry takes a problem without the flag and nc = 0 as the old one does
    rc, err, _ = _check_c(ddp_amd.example_source("car_ad"), 0, TERMINAL | AUTODIFF, nparam=9)
    assert rc == 0, err


def _usage(log):
    out, cur = {}, None
    for line in log.splitlines():
        mm = re.search(r"remark: Function Name: (\w+)", line)
        if mm:
            cur = mm.group(1)
        mm = re.search(r"remark:\s+ScratchSize \[bytes/lane\]: (\d+)", line)
        if mm and cur:
            out[cur] = int(mm.group(1))
    return out


@pytest.mark.parametrize("flags,kernels", [(BASE, ("ddp_user_rollout", "ddp_user_df_ad")), (BASE | WAVE, ("ddp_user_rollout_wave", "ddp_user_df_wave")),
                                           (BASE | PLANT, ())])
def test_keepout_example_compiles_for_gfx950_without_scratch(flags, kernels):
    src = SRC
    if flags & PLANT:
        src += ("\n__device__ void plant(const double *x, const double *u, int t, const double *p, double *xnext)\n"
                "{\n    dynamics<double>(x, u, t, p, xnext);\n}\n")
    rc, err, log = _check_c(src, cc.NC, flags, extra="-Rpass-analysis=kernel-resource-usage")
    assert rc == 0, (err, log[-3000:])
    u = _usage(log)
    for k in kernels + ("ddp_user_cost", "ddp_user_constraints", "ddp_user_al_update"):
        assert k in u, sorted(u)
    assert u["ddp_user_constraints"] == 0 and u["ddp_user_al_update"] == 0, u


def _text(name, nparam, nc, flags):
    L = _lib.lib()
    t = (L.ddp_user_program_text_c(ddp_amd.example_source(name).encode(), 4, 2, nparam, nc, flags, 0) if nc else
         L.ddp_user_program_text(ddp_amd.example_source(name).encode(), 4, 2, nparam, flags, 0))
    assert t is not None, L.ddp_last_error().decode()
    return t.decode()


def test_the_program_without_the_flag_holds_nothing_of_the_constraints():
    for flags in (TERMINAL | AUTODIFF, TERMINAL | AUTODIFF | WAVE):
        plain = _text("car_ad", 9, 0, flags)
        for word in ("DDP_NC", "ddp_user_stage_cost", "constraints", "ddp_user_constraints", "ddp_user_al_update", "UserAlArgs", "UserConArgs", "DDP_CS"):
            assert not re.search(r"\b%s\b" % word, plain), word
        assert plain == _lib.lib().ddp_user_program_text_c(ddp_amd.example_source("car_ad").encode(), 4, 2, 9, 0, flags, 0).decode()
        full = _text("car_keepout_ad", cc.NPARAM, cc.NC, flags | CONSTRAINTS)
        assert full.count(SRC) == 1
        assert "#define DDP_NP 12\n" in full and "#define DDP_NC 2\n" in full            # the stride: nparam + 2
        a, b, c = full.index("#define stage_cost ddp_user_stage_cost\n"), full.index(SRC), full.index("#undef stage_cost\n")
        assert a < b < c < full.index('#line 1 "ddp_user_autodiff_derivs"') < full.index("void ddp_user_constraints(")
        # the kernels of the library are the ones of the plain program, byte for byte: the wrap is around the user's source only
        tail = lambda t: t[t.index('#line 1 "ddp_user_autodiff_derivs"'):]
        assert tail(full).startswith(tail(plain))


def test_header_loader_and_python_agree():
    hdr = open(os.path.join(ROOT, "include", "ddp_amd.h")).read()
    assert re.search(r"\bDDP_USER_CONSTRAINTS = 1024\b", hdr) and re.search(r"^#define DDP_USER_MAX_NC 16\b", hdr, flags=re.M)
    assert "64: not assigned" in hdr and not re.search(r"DDP_USER_\w+\s*=\s*(64|256)\b", hdr)
    assert _lib.USER_CONSTRAINTS == 1024 and _lib.USER_MAX_NC == 16
    jl = open(os.path.join(PKG, "julia", "DDPAmd.jl")).read()
    assert re.search(r"^const USER_CONSTRAINTS = 1024\b", jl, flags=re.M)
    o = _lib.ALOpts()
    _lib.lib().ddp_al_default_opts(ctypes.byref(o))
    assert (o.mu0, o.mu_factor, o.mu_max, o.ctol, o.max_outer) == (1.0, 10.0, 1e8, 1e-5, 20)
    p = ddp_amd.DeviceProblem(SRC, 4, 2, nparam=cc.NPARAM, terminal=True, autodiff=True, constraints=2)
    assert p.flags == BASE and p.nc == 2
    p.check()
    with pytest.raises(ddp_amd.DDPError, match="DDP_USER_CLOCK"):
        ddp_amd.DeviceProblem(SRC, 4, 2, nparam=cc.NPARAM, terminal=True, autodiff=True, constraints=2, clock=True).check()
    with pytest.raises(ddp_amd.DDPError, match="multipliers"):
        ddp_amd.DeviceProblem(ddp_amd.example_source("car_ad"), 4, 2, nparam=9, terminal=True, autodiff=True)._multiplier_arrays(
            (np.zeros((2, 5)), 1.0), 5, 1, False)
    with pytest.raises(ddp_amd.DDPError, match="λ should be"):
        p._multiplier_arrays((np.zeros((3, 5, 2)), 1.0), 5, 2, True)
    with pytest.raises(ddp_amd.DDPError, match="μ should be"):
        p._multiplier_arrays((np.zeros((2, 5, 2)), np.ones(3)), 5, 2, True)


# ---------------------------------------------------------------------------------------------- the wrapper text as host C++
def _raw(path, tag):
    src = open(os.path.join(PKG, "csrc", path)).read()
    return dict(re.findall(r'static const char \*(\w+) = R"%s\((.*?)\)%s";' % (tag, tag), src, re.S))


def _cxx():
    for c in ("c++", "g++", "clang++", "/opt/rocm/llvm/bin/clang++"):
        p = shutil.which(c) or (c if os.path.isabs(c) and os.path.exists(c) else None)
        if p:
            return p
    raise RuntimeError("no host C++ compiler")


# (x, u, λ, μ): t = λ + μ g on both sides of 0 for each constraint, λ = 0 on both sides, and μ = 0 (the pointer slot is null there)
P_HOST = np.array([0.1, 3.6, 0.05, 1.8, 0.1, 0.35, 0.7, 0.1, 10.0, 1.3])
HOST_CASES = [
    ([1.7, 0.2, 0.3, 1.5], [0.8, -0.4], [0.3, 0.2], 2.0),        # inside the disc, over the cap: both active
    ([0.4, -0.6, -0.2, 0.9], [-0.5, 0.3], [0.1, 0.05], 2.0),     # far outside, slow: both t < 0, ψ = −Σλ²/2μ, no derivative
    ([1.9, 0.15, 0.1, 1.0], [0.2, 0.1], [0.0, 0.0], 5.0),        # λ = 0: g0 > 0 active, g1 < 0 not
    ([0.2, 0.9, 0.0, 0.5], [0.1, 0.2], [0.0, 0.0], 5.0),         # λ = 0, both feasible: ψ = 0
    ([1.7, 0.2, 0.3, 1.5], [0.8, -0.4], [0.3, 0.2], 0.0),        # μ = 0: the raw cost
    ([2.4, 0.4, 0.5, 1.45], [1.0, 0.0], [0.05, 0.4], 3.0),       # outside the disc with a small λ0 (t0 < 0), over the cap (t1 > 0)
]


def test_wrapper_text_on_the_host_matches_the_longdouble_closed_forms(tmp_path):
    ad = _raw("user_autodiff.h", "DDPA")
    con = _raw("user_constraints.h", "DDPC")
    before = re.search(r'kUserConstraintsBefore = "(.*?)\\n";', open(os.path.join(PKG, "csrc", "user_constraints.h")).read()).group(1)
    N, i = 5, 2
    head = "#include <cmath>\n#include <cstdio>\n#include <cstring>\n#define DDP_AD_FN inline\n#define DDP_AD_FRESH(q) ((void)0)\n#define __device__\n"
    macros = dict(DDP_N=4, DDP_M=2, DDP_NP=cc.NPARAM + 2, DDP_NC=cc.NC, DDP_TERMINAL=1, DDP_CONST_HESSIAN=0, DDP_ADJ=6, DDP_ADH=3)
    head += "".join("#define %s %s\n" % kv for kv in macros.items())
    rows = ["{%s}" % ", ".join("%.17g" % v for v in list(x) + list(u) + list(lam) + [mu]) for x, u, lam, mu in HOST_CASES]
    main = """
int main()
{
    const double cases[%d][9] = {%s};
    const double pu[10] = {%s};
    for (auto &c : cases) {
        double p[12], lam[2 * %d] = {0}, fx[16], fu[8], cx[4], cu[2], cxx[16], cxu[8], cuu[4];
        for (int e = 0; e < 10; ++e) p[e] = pu[e];
        lam[2 * %d] = c[6]; lam[2 * %d + 1] = c[7];
        p[10] = c[8];
        const double *lp = c[8] > 0.0 ? lam : nullptr;
        std::memcpy(&p[11], &lp, sizeof lp);
        const double v = stage_cost<double>(c, c + 4, %d, p);
        ddp_ad_derivatives(c, c + 4, %d, %d, p, fx, fu, cx, cu, cxx, cxu, cuu);
        std::printf("%%.17g\\n", v);
        for (double d : cx) std::printf("%%.17g\\n", d);
        for (double d : cu) std::printf("%%.17g\\n", d);
        for (double d : cxx) std::printf("%%.17g\\n", d);
        for (double d : cxu) std::printf("%%.17g\\n", d);
        for (double d : cuu) std::printf("%%.17g\\n", d);
    }
    return 0;
}
""" % (len(HOST_CASES), ", ".join(rows), ", ".join("%.17g" % v for v in P_HOST), N, i, i, i, i, N)
    src = head + ad["kUserAutodiff"] + "\n" + before + "\n" + SRC + "\n" + con["kUserConstraintsAfter"] + "\n" + ad["kUserAutodiffDerivs"] + main
    cpp, exe = tmp_path / "t.cpp", tmp_path / "t"
    cpp.write_text(src)
    r = subprocess.run([_cxx(), "-std=c++17", "-O1", "-o", str(exe), str(cpp)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[:4000]
    out = np.array([float(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]).reshape(len(HOST_CASES), 35)
    ld = np.longdouble
    p = P_HOST.astype(ld)
    active = []
    for row, (x, u, lam, mu) in zip(out, HOST_CASES):
        x, u, lam = np.array(x, dtype=ld), np.array(u, dtype=ld), np.array(lam, dtype=ld)
        c0, g0, H0 = cc.raw_stage(p, x, u)
        c1, g1, H1 = cc.psi(p, x, u, lam, ld(mu))
        g, H = g0 + g1, H0 + H1
        want = np.concatenate([[c0 + c1], g[:4], g[4:], H[:4, :4].ravel(order="F"), H[:4, 4:].ravel(order="F"), H[4:, 4:].ravel(order="F")])
        for sl in (slice(0, 1), slice(1, 7), slice(7, 35)):      # ψ, its gradient, its Hessian: 1e-13 relative, each on its own scale
            scale = float(np.max(np.abs(want[sl])))
            assert float(np.max(np.abs(row[sl] - want[sl]))) <= 1e-13 * max(scale, 1.0), (x, mu, row[sl], want[sl])
        cxx, cuu = row[7:23].reshape(4, 4), row[31:35].reshape(2, 2)
        assert np.array_equal(cxx, cxx.T) and np.array_equal(cuu, cuu.T)
        active.append(tuple((lam + ld(mu) * cc.constraints(p, x, u)) > 0) if mu > 0 else None)
    # the designed cases are what their comments say
    assert active == [(True, True), (False, False), (True, False), (False, False), None, (False, True)], active
    # the penalty acts: case 0 and case 4 differ in μ only, and the cap's term reaches cxu, cuu and cu (g1 mixes state and control)
    assert out[0, 0] != out[4, 0] and np.any(out[0, 23:31] != out[4, 23:31]) and out[0, 31] != out[4, 31] and out[0, 5] != out[4, 5]


# ---------------------------------------------------------------------------------------------- the NumPy loop on the designed inputs
SEED, B_REF, N_REF = 1, 5, 30


@pytest.fixture(scope="module")
def reference():
    return cc.reference(SEED, B_REF, N_REF)


def test_numpy_loop_on_the_designed_inputs(reference):
    p, x0, u0, plain, loops = reference
    ctol, max_outer = cc.AL_DEFAULTS["ctol"], cc.AL_DEFAULTS["max_outer"]
    for b in range(B_REF):
        g = cc.constraints(p[:, b], plain[b][0], plain[b][1])
        assert g[0].max() > 10 * ctol and g[1].max() > 10 * ctol, (b, g.max(axis=1))      # the disc is crossed and the cap binds
        status, rounds = loops[b]
        assert status == 1 and len(rounds) <= max_outer and rounds[-1]["cviol"] <= ctol, (b, status, len(rounds))
    # how far the iteration counts of the reference itself move under a perturbation of u0 at rounding level: the cap that the GPU
    # comparison inherits
    changed = 0
    for b in range(B_REF):
        _, again = cc.al_loop(p[:, b], x0[:, b], u0[:, :, b] + 1e-13, **cc.AL_DEFAULTS)
        a, c = [r["iter"] for r in loops[b][1]], [r["iter"] for r in again]
        changed += a[:-1] != c[:len(a) - 1] or len(a) != len(c)
    assert changed <= B_REF // 4, changed
