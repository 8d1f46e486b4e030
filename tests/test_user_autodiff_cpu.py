"""User problems with DDP_USER_AUTODIFF (flag 4, DeviceProblem(autodiff=True)) without a GPU: the templated examples compile for gfx950,
ddp_user_df_ad does not spill on the bundled shapes, the contract is enforced, and the dual-number texts of csrc/user_autodiff.h, compiled
as host C++, give the analytic derivatives of every supported function and car.hip's hand-written derivatives."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import ddp_amd
from ddp_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "differentialdynamicprogramming.jl_amd")
AUTODIFF, TERMINAL, CONST_HESSIAN = 4, 1, 2


def _check(src, n, m, nparam=0, flags=0, extra=None):
    L = _lib.lib()
    rc = L.ddp_user_check(src.encode(), n, m, nparam, flags, extra.encode() if extra else None)
    return rc, L.ddp_last_error().decode(), L.ddp_user_compile_log().decode()


def _lq_np(n, m):
    return 2 * n * n + n * m + m * m


@pytest.mark.parametrize("name,n,m,nparam,flags", [
    ("car_ad", 4, 2, 9, AUTODIFF | TERMINAL),
    ("pendcart_ad", 4, 1, 25, AUTODIFF | TERMINAL),
    ("lq_ad", 10, 2, 224, AUTODIFF),
    ("lq_ad", 10, 2, 224, AUTODIFF | CONST_HESSIAN),
    ("lq_ad", 24, 4, _lq_np(24, 4), AUTODIFF),
    ("lq_ad", 32, 8, _lq_np(32, 8), AUTODIFF),
])
def test_autodiff_examples_compile_for_gfx950(name, n, m, nparam, flags):
    rc, err, log = _check(ddp_amd.example_source(name), n, m, nparam, flags)
    assert rc == 0, (err, log[:4000])


def _usage(log):
    """kernel -> ScratchSize from the kernel-resource-usage remarks of a hiprtc log (as test_user_problem_cpu._usage)"""
    out, cur = {}, None
    for line in log.splitlines():
        mm = re.search(r"remark: Function Name: (\w+)", line)
        if mm:
            cur = mm.group(1)
        mm = re.search(r"remark:\s+ScratchSize \[bytes/lane\]: (\d+)", line)
        if mm and cur:
            out[cur] = int(mm.group(1))
    return out


@pytest.mark.parametrize("name,n,m,nparam,flags", [("car_ad", 4, 2, 9, AUTODIFF | TERMINAL), ("pendcart_ad", 4, 1, 25, AUTODIFF | TERMINAL),
                                                   ("lq_ad", 10, 2, 224, AUTODIFF), ("lq_ad", 10, 2, 224, AUTODIFF | CONST_HESSIAN)])
def test_autodiff_derivative_kernel_does_not_spill(name, n, m, nparam, flags):
    rc, err, log = _check(ddp_amd.example_source(name), n, m, nparam, flags, "-Rpass-analysis=kernel-resource-usage")
    assert rc == 0, err
    u = _usage(log)
    assert "ddp_user_df_ad" in u and "ddp_user_df" not in u, sorted(u)
    assert u["ddp_user_df_ad"] == 0, u
    assert u["ddp_user_rollout"] == 0, u


def test_templated_source_without_the_flag_needs_derivatives():
    rc, err, _ = _check(ddp_amd.example_source("car_ad"), 4, 2, 9, TERMINAL)
    assert rc == -1 and "derivatives" in err, err


def test_unsupported_function_fails_with_its_name():
    bad = ddp_amd.example_source("car_ad").replace("exp(-(dx * dx + dy * dy) / r2)", "erf(-(dx * dx + dy * dy) / r2)")
    rc, err, log = _check(bad, 4, 2, 9, AUTODIFF | TERMINAL)
    assert rc == -4, err
    assert re.search(r"user_source:\d+:\d+: error", log) and "erf" in log, log[:4000]


def test_device_problem_autodiff_keyword_sets_the_flag():
    p = ddp_amd.DeviceProblem(ddp_amd.example_source("car_ad"), 4, 2, nparam=9, terminal=True, autodiff=True)
    assert p.flags & AUTODIFF and p.flags & TERMINAL
    assert not ddp_amd.DeviceProblem(ddp_amd.example_source("car"), 4, 2, nparam=9).flags & AUTODIFF
    p.check()                                                # compiles with the flags it carries (raises otherwise)


def test_header_documents_the_flag():
    txt = open(os.path.join(ROOT, "include", "ddp_amd.h")).read()
    assert re.search(r"DDP_USER_AUTODIFF\s*=\s*4", txt)
    for f in ("atan2", "hypot", "expm1", "log1p", "floor", "ddp_user_df_ad"):
        assert f in txt, f


# ---------------------------------------------------------------------------------------------- host C++ build of the AD texts
def _texts():
    src = open(os.path.join(PKG, "csrc", "user_autodiff.h")).read()
    t = dict(re.findall(r'static const char \*(\w+) = R"DDPA\((.*?)\)DDPA";', src, re.S))
    return t["kUserAutodiff"], t["kUserAutodiffDerivs"]


def _cxx():
    for c in ("c++", "g++", "clang++", "/opt/rocm/llvm/bin/clang++"):
        p = shutil.which(c) or (c if os.path.isabs(c) and os.path.exists(c) else None)
        if p:
            return p
    raise RuntimeError("no host C++ compiler")


def _run_host(tmp_path, macros, body, main):
    pre, derivs = _texts()
    head = "#include <cmath>\n#include <cstdio>\n#define DDP_AD_FN inline\n#define DDP_AD_FRESH(q) ((void)0)\n#define __device__\n"
    head += "".join("#define %s %s\n" % kv for kv in macros.items())
    src = head + pre + "\n" + body.replace("@DERIVS@", derivs) + "\n" + main
    cpp, exe = tmp_path / "t.cpp", tmp_path / "t"
    cpp.write_text(src)
    r = subprocess.run([_cxx(), "-std=c++17", "-O1", "-o", str(exe), str(cpp)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[:4000]
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout
    return np.array([float(v) for v in out.split()])


UNARY = {   # f, f', f'' at x (numpy)
    "sin": (np.sin, np.cos, lambda x: -np.sin(x)),
    "cos": (np.cos, lambda x: -np.sin(x), lambda x: -np.cos(x)),
    "tan": (np.tan, lambda x: 1 + np.tan(x) ** 2, lambda x: 2 * np.tan(x) * (1 + np.tan(x) ** 2)),
    "exp": (np.exp, np.exp, np.exp),
    "log": (np.log, lambda x: 1 / x, lambda x: -1 / x ** 2),
    "sqrt": (np.sqrt, lambda x: 0.5 / np.sqrt(x), lambda x: -0.25 * x ** -1.5),
    "tanh": (np.tanh, lambda x: 1 - np.tanh(x) ** 2, lambda x: -2 * np.tanh(x) * (1 - np.tanh(x) ** 2)),
    "sinh": (np.sinh, np.cosh, np.sinh),
    "cosh": (np.cosh, np.sinh, np.cosh),
    "atan": (np.arctan, lambda x: 1 / (1 + x * x), lambda x: -2 * x / (1 + x * x) ** 2),
    "asin": (np.arcsin, lambda x: (1 - x * x) ** -0.5, lambda x: x * (1 - x * x) ** -1.5),
    "acos": (np.arccos, lambda x: -(1 - x * x) ** -0.5, lambda x: -x * (1 - x * x) ** -1.5),
    "fabs": (np.abs, np.sign, lambda x: 0 * x),
    "expm1": (np.expm1, np.exp, np.exp),
    "log1p": (np.log1p, lambda x: 1 / (1 + x), lambda x: -1 / (1 + x) ** 2),
    "rint": (np.rint, lambda x: 0 * x, lambda x: 0 * x),
    "floor": (np.floor, lambda x: 0 * x, lambda x: 0 * x),
    "pow_d": (lambda x: x ** 2.5, lambda x: 2.5 * x ** 1.5, lambda x: 3.75 * x ** 0.5),
    "pow_i": (lambda x: x ** 3, lambda x: 3 * x ** 2, lambda x: 6 * x),
    "pow_c": (lambda x: 1.7 ** x, lambda x: 1.7 ** x * np.log(1.7), lambda x: 1.7 ** x * np.log(1.7) ** 2),
    "arith": (lambda x: (2 * x - x / 3 + 1) * x / (x + 3) - 1 / x + 4 - (-x),
              lambda x: (10 / 3 * x + 1) / (x + 3) - (5 / 3 * x * x + x) / (x + 3) ** 2 + 1 / x ** 2 + 1,
              lambda x: 10 / 3 / (x + 3) - 2 * (10 / 3 * x + 1) / (x + 3) ** 2 + 2 * (5 / 3 * x * x + x) / (x + 3) ** 3 - 2 / x ** 3),
}
CALL = {"pow_d": "pow(z, 2.5)", "pow_i": "pow(z, 3)", "pow_c": "pow(1.7, z)",
        "arith": "[&] { T t = 2 * z; t -= z / 3; t += 1; t *= z; t /= z + 3; return t - 1 / z + 4 - (-z); }()"}


def _hess2(f, x, y):
    """value, gradient and Hessian of f(x, y) (numpy) by analytic formulas for the binary functions"""
    r2 = x * x + y * y
    if f == "pow":
        v = x ** y
        return v, [y * x ** (y - 1), v * np.log(x)], [[y * (y - 1) * x ** (y - 2), x ** (y - 1) * (1 + y * np.log(x))],
                                                     [x ** (y - 1) * (1 + y * np.log(x)), v * np.log(x) ** 2]]
    if f == "atan2":                                          # atan2(x, y): x is the ordinate
        return np.arctan2(x, y), [y / r2, -x / r2], [[-2 * x * y / r2 ** 2, (x * x - y * y) / r2 ** 2],
                                                     [(x * x - y * y) / r2 ** 2, 2 * x * y / r2 ** 2]]
    if f == "hypot":
        h = np.sqrt(r2)
        return h, [x / h, y / h], [[y * y / h ** 3, -x * y / h ** 3], [-x * y / h ** 3, x * x / h ** 3]]
    if f == "fmin":
        return min(x, y), [float(x <= y), float(y < x)], [[0, 0], [0, 0]]
    if f == "fmax":
        return max(x, y), [float(x >= y), float(y > x)], [[0, 0], [0, 0]]
    if f == "mul_div":                                        # x * y / (x - y)
        d = x - y
        return x * y / d, [-y * y / d ** 2, x * x / d ** 2], [[2 * y * y / d ** 3, -2 * x * y / d ** 3], [-2 * x * y / d ** 3, 2 * x * x / d ** 3]]


def test_dual_numbers_give_the_analytic_derivatives(tmp_path):
    pts = {"asin": 0.3, "acos": -0.4, "fabs": -0.7, "rint": 1.3, "floor": 2.6, "log1p": 0.8, "pow_i": -1.2}
    names = list(UNARY)
    main = ["int main() {", "typedef ddp_dual<ddp_dual<double, 1>, 1> T;", "typedef ddp_dual<ddp_dual<double, 2>, 2> T2;"]
    for f in names:
        x = pts.get(f, 0.9)
        main.append("{ T z(%r); z.v.d[0] = 1; z.d[0].v = 1; T r = %s;" % (x, CALL.get(f, "%s(z)" % f)))
        main.append("  printf(\"%.17g %.17g %.17g %.17g\\n\", r.v.v, r.v.d[0], r.d[0].v, r.d[0].d[0]); }")
    binary = [("pow", "pow(a, b)"), ("atan2", "atan2(a, b)"), ("hypot", "hypot(a, b)"), ("fmin", "fmin(a, b)"), ("fmax", "fmax(a, b)"),
              ("mul_div", "a * b / (a - b)")]
    for _, call in binary:
        main.append("{ T2 a(1.3), b(0.7); a.v.d[0] = 1; a.d[0].v = 1; b.v.d[1] = 1; b.d[1].v = 1; T2 r = %s;" % call)
        main.append("  printf(\"%.17g %.17g %.17g %.17g %.17g %.17g %.17g\\n\", r.v.v, r.v.d[0], r.v.d[1], r.d[0].d[0], r.d[0].d[1], "
                    "r.d[1].d[0], r.d[1].d[1]); }")
    # mixed operands: dual op double / int and the comparisons
    main.append("{ ddp_dual<double, 1> z(2.0); z.d[0] = 1; ddp_dual<double, 1> w = fmin(z, 3) + atan2(1.0, z) + hypot(z, 1.5) + pow(z, z);")
    main.append("  printf(\"%.17g %.17g %d\\n\", w.v, w.d[0], (int)(z < 3) + 2 * (int)(3.0 > z) + 4 * (int)(z == 2) + 8 * (int)(z != z)); }")
    main.append("return 0; }")
    out = _run_host(tmp_path, {}, "", "\n".join(main))
    k = 0
    for f in names:
        x = pts.get(f, 0.9)
        v, d1, d1b, d2 = out[k:k + 4]
        k += 4
        F, dF, ddF = UNARY[f]
        ref = [F(x), dF(x), dF(x), ddF(x)]
        assert np.allclose([v, d1, d1b, d2], ref, rtol=1e-13, atol=1e-13), (f, [v, d1, d1b, d2], ref)
    for f, _ in binary:
        got = out[k:k + 7]
        k += 7
        v, g, H = _hess2(f, 1.3, 0.7)
        ref = [v, g[0], g[1], H[0][0], H[0][1], H[1][0], H[1][1]]
        assert np.allclose(got, ref, rtol=1e-13, atol=1e-13), (f, got, ref)
    w, dw, cmp = out[k:k + 3]
    z = 2.0
    assert np.isclose(w, z + np.arctan2(1, z) + np.hypot(z, 1.5) + z ** z, rtol=1e-14)
    assert np.isclose(dw, 1 - 1 / (1 + z * z) + z / np.hypot(z, 1.5) + z ** z * (np.log(z) + 1), rtol=1e-14)
    assert cmp == 1 + 2 + 4


def test_host_ad_of_car_matches_the_hand_written_derivatives(tmp_path):
    car, car_ad = ddp_amd.example_source("car"), ddp_amd.example_source("car_ad")
    rng = np.random.default_rng(3)
    cases = []
    for t in range(6):
        x = rng.standard_normal(4) + [2, 2, 0, 1]
        u = rng.standard_normal(2)
        p = [0.05, 4.1, 3.9, 2.1, 1.8, 0.7, 12.0, 0.1, 9.0]
        cases.append((x, u, p, 9 if t % 2 else 3))           # N = 10: step 9 carries the terminal cost
    body = car_ad + "\n@DERIVS@\nnamespace hand {\n" + car + "\n}\n"
    main = ["int main() {"]
    for x, u, p, i in cases:
        main.append("{ double x[4] = {%s}, u[2] = {%s}, p[9] = {%s}, a[58], h[58];" % tuple(",".join(repr(float(v)) for v in a) for a in (x, u, p)))
        main.append("  ddp_ad_derivatives(x, u, %d, 10, p, a, a + 16, a + 24, a + 28, a + 30, a + 46, a + 54);" % i)
        main.append("  hand::derivatives(x, u, %d, 10, p, h, h + 16, h + 24, h + 28, h + 30, h + 46, h + 54);" % i)
        main.append("  for (int e = 0; e < 58; ++e) printf(\"%.17g %.17g\\n\", a[e], h[e]); }")
    main.append("return 0; }")
    out = _run_host(tmp_path, {"DDP_N": 4, "DDP_M": 2, "DDP_TERMINAL": 1, "DDP_CONST_HESSIAN": 0, "DDP_ADJ": 6, "DDP_ADH": 3}, body,
                    "\n".join(main)).reshape(len(cases), 58, 2)
    for c in range(len(cases)):
        ad, hand = out[c, :, 0], out[c, :, 1]
        for lo, hi in ((0, 16), (16, 24), (24, 28), (28, 30), (30, 46), (46, 54), (54, 58)):
            scale = max(np.max(np.abs(hand[lo:hi])), 1.0)
            assert np.max(np.abs(ad[lo:hi] - hand[lo:hi])) <= 1e-13 * scale, (c, lo, ad[lo:hi], hand[lo:hi])
        cxx = ad[30:46].reshape(4, 4)
        assert np.array_equal(cxx, cxx.T)
