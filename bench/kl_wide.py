"""The wide KL path (ddp_kl_set_wide: n <= 64, m <= 32).  First, without touching a device, every new kernel is compiled for gfx950
and the compiler's resource record (registers, scratch, LDS, occupancy) is written: the GPS instantiation of back_pass_wide_kernel next
to its twin, and the kernels of kl_wide.hip.  Then, on one GPU, HIP events around `--reps` launches of ∇kl, back_pass_gps,
forward_covariance and kl_div_wiki on device arrays and the wall time of a whole kl.iLQGkl (host arrays in and out) at (64, 32),
(48, 12) and (12, 12); and at (32, 8) the same legs with DDP_GPS_WIDE=1 next to the default kernels (back_pass_gps: DDP_GPS_MID=1, the
mid kernel) in the same run, so that a later change can decide the dispatch of that shape from a number.  --compile-only stops after the
first part and writes "not measured" for every timed leg.  No time here is a pass criterion.

    python bench/kl_wide.py [--compile-only] [--reps 10] [--B 256] [--N 50] [--out profiles/kl_wide.txt]
"""
import argparse
import ctypes as C
import os
import re
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
CSRC = os.path.join(ROOT, "differentialdynamicprogramming.jl_amd", "csrc")
UNITS = ["back_pass_wide.hip", "kl_wide.hip"]
SHAPES = [(64, 32), (48, 12), (12, 12)]
LEGS = ("∇kl", "back_pass_gps", "forward_covariance", "kl_div_wiki")


def compile_part(say):
    flags = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-fno-gpu-rdc", "-Rpass-analysis=kernel-resource-usage", "-mllvm",
             "-amdgpu-mfma-vgpr-form=1"]
    say("# the compiler's records per kernel (hipcc %s), no device" % " ".join(flags))
    with tempfile.TemporaryDirectory() as tmp:
        for unit in UNITS:
            t0 = time.perf_counter()
            r = subprocess.run(["hipcc"] + flags + ["-c", os.path.join(CSRC, unit), "-o", os.path.join(tmp, unit + ".o")], capture_output=True, text=True)
            if r.returncode != 0:
                raise RuntimeError("hipcc failed for %s:\n%s" % (unit, r.stderr[-2000:]))
            say("%s: compiled in %.1f s" % (unit, time.perf_counter() - t0))
            cur = None
            for line in r.stderr.splitlines():
                mm = re.search(r"remark: Function Name: (\S+)", line)
                if mm:
                    if cur:
                        say("%s:   %s" % (unit, cur))
                    name = re.sub(r"^_ZN12_GLOBAL__N_1\d+", "", mm.group(1))
                    name = re.sub(r"ILb([01])E.*", lambda g: "<GPS>" if g.group(1) == "1" else "<iLQG>", name)
                    cur = re.sub(r"(kernel)E.*", r"\1", name)
                    continue
                mm = re.search(r"remark:\s+(VGPRs|AGPRs|SGPRs|ScratchSize \[bytes/lane\]|LDS Size \[bytes/block\]|Occupancy \[waves/SIMD\]): (\d+)", line)
                if mm and cur is not None:
                    cur += " %s=%s" % (mm.group(1).split(" ")[0], mm.group(2))
            if cur:
                say("%s:   %s" % (unit, cur))
    say("# dynamic LDS at launch (bytes): back_pass_gps_wide (64, 32) 163600; forward_covariance (64, 32) 136192; "
        "kl_div_wiki (64, 32) 50944; ∇kl (64, 32) 41472")


def setup(rng, n, m, N, B):
    import scipy.linalg as sla
    h_ = 0.01
    A0 = rng.standard_normal((n, n)); A = sla.expm(h_ * (A0 - A0.T)); Bm = h_ * rng.standard_normal((n, m))
    Q, R = h_ * np.eye(n), 0.1 * h_ * np.eye(m)
    u = 0.1 * rng.standard_normal((m, N, B))
    x = np.zeros((n, N, B)); x[:, 0, :] = 1.0 + 0.1 * rng.standard_normal((n, B))
    for t in range(N - 1):
        x[:, t + 1, :] = A @ x[:, t, :] + Bm @ u[:, t, :]
    cost0 = 0.5 * np.einsum("itb,ij,jtb->b", x, Q, x) + 0.5 * np.einsum("itb,ij,jtb->b", u, R, u)
    eye = np.ascontiguousarray(np.broadcast_to(np.eye(m)[:, :, None, None], (m, m, N, B)))
    return dict(A=A, Bm=Bm, Q=Q, R=R, u=u, x=x, cost0=cost0, eye=eye, fx=np.repeat(A[:, :, None], N, 2), fu=np.repeat(Bm[:, :, None], N, 2),
                R1=1e-4 * np.eye(n))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--compile-only", action="store_true")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--B", type=int, default=256)
    ap.add_argument("--N", type=int, default=50)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    B, N = a.B, a.N
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    def finish():
        if a.out:
            with open(a.out, "w") as f:
                f.write("\n".join(lines) + "\n")

    say("# the wide KL path, bench/kl_wide.py")
    compile_part(say)
    say("#")
    if a.compile_only:
        say("# kernel and loop times at B = %d, N = %d: not measured (--compile-only)" % (B, N))
        for n, m in SHAPES:
            say("(%d, %d) wide: %s; iLQGkl loop not measured" % (n, m, "; ".join("%s not measured" % leg for leg in LEGS)))
        for tag in ("DDP_GPS_WIDE=1", "default kernels (back_pass_gps: DDP_GPS_MID=1)"):
            say("(32, 8) %s: %s; iLQGkl loop not measured" % (tag, "; ".join("%s not measured" % leg for leg in LEGS)))
        return finish()

    import ddp_amd as ddp
    from ddp_amd import _lib, kl
    h = ddp.default_handle()
    L = _lib.lib()
    rng = np.random.default_rng(0)
    ev0, ev1 = C.c_void_p(), C.c_void_p()
    _lib.check(L.ddp_event_create(h.raw, C.byref(ev0))); _lib.check(L.ddp_event_create(h.raw, C.byref(ev1)))

    def timed(fn):
        fn(); h.sync()
        L.ddp_event_record(h.raw, ev0)
        for _ in range(a.reps):
            fn()
        L.ddp_event_record(h.raw, ev1)
        ms = C.c_float()
        L.ddp_event_elapsed_ms(h.raw, ev0, ev1, C.byref(ms))
        return ms.value / a.reps

    def legs(n, m, tag, wide):
        c = setup(rng, n, m, N, B)
        NB = N * B
        dK = h.to_device(0.05 * rng.standard_normal((m, n, N, B)) / np.sqrt(n)); dk = h.to_device(np.zeros((m, N, B)))
        dS = h.to_device(c["eye"]); dx = h.to_device(c["x"]); du = h.to_device(c["u"])
        dfx = h.to_device(np.ascontiguousarray(c["fx"])); dfu = h.to_device(np.ascontiguousarray(c["fu"]))
        dcxx = h.to_device(np.repeat(c["Q"][:, :, None], N, 2)); dcxu = h.to_device(np.zeros((n, m, N))); dcuu = h.to_device(np.repeat(c["R"][:, :, None], N, 2))
        dcx = h.to_device(np.einsum("ij,jtb->itb", c["Q"], c["x"])); dcu = h.to_device(np.einsum("ij,jtb->itb", c["R"], c["u"]))
        dR1 = h.to_device(c["R1"]); deta = h.to_device(np.ones(B))
        kt = [h.malloc(8 * s * NB) for s in (n, m, n * n, m * n, m * m)]
        outs = [h.malloc(8 * s) for s in (m * n * NB, m * NB, m * m * NB, m * m * NB, n * NB, n * n * NB, 2 * B)]
        ddiv = h.malloc(4 * B + 16); dsig = h.malloc(8 * (n + m) * (n + m) * NB); dkld = h.malloc(8 * NB); dklm = h.malloc(8 * B)
        t = _lib.KLCostTerms(*[p.value for p in kt], deta.value, 0)
        d = _lib.BPDesc(n, m, N, B, 1, 0, 1, 0, 1, 0)
        res = []
        was = h.set_kl_wide(wide)
        try:
            res.append(timed(lambda: _lib.check(L.ddp_kl_terms_f64_dev(h.raw, n, m, N, B, dK, dk, dS, *kt))))
            res.append(timed(lambda: _lib.check(L.ddp_back_pass_gps_f64_dev(h.raw, C.byref(d), dcx, dcu, dcxx, dcxu, dcuu, dfx, dfu, C.byref(t), None, None,
                                                                            None, *outs, ddiv))))
            kern = h.last_kernel(0)
            res.append(timed(lambda: _lib.check(L.ddp_forward_covariance_f64_dev(h.raw, n, m, N, B, dfx, 0, dR1, outs[0], outs[3], dsig))))
            res.append(timed(lambda: _lib.check(L.ddp_kl_div_f64_dev(h.raw, n, m, N, B, dx, dx, dsig, outs[0], outs[1], outs[3], dK, dk, dS, dS, dkld, dklm))))
        finally:
            h.set_kl_wide(was)
        for p in [dK, dk, dS, dx, du, dfx, dfu, dcxx, dcxu, dcuu, dcx, dcu, dR1, deta, ddiv, dsig, dkld, dklm] + kt + outs:
            h.free(p)
        prev = ddp.GaussianPolicy(N, n, m, np.zeros((m, n, N, B)), c["u"].copy(), c["eye"], c["eye"].copy())
        prob, mdl = ddp.LQProblem(c["A"], c["Bm"], c["Q"], c["R"]), kl.Model(c["fx"], c["fu"], c["R1"])
        kw = dict(kl_step=2e-4, max_iter=10, cost=c["cost0"], wide=wide)
        kl.iLQGkl(prob, c["x"][..., :4], ddp.GaussianPolicy(N, n, m, prev.K[..., :4], prev.k[..., :4], prev.Σ[..., :4], prev.Σi[..., :4]), mdl,
                  **dict(kw, cost=c["cost0"][:4], max_iter=2))
        t0 = time.perf_counter()
        out = kl.iLQGkl(prob, c["x"], prev, mdl, **kw)
        wall = time.perf_counter() - t0
        say("(%d, %d) %s: %s; iLQGkl loop %.3f s wall (host arrays in and out, at most 10 iterations, %d back passes at most per trajectory), %s"
            % (n, m, tag, "; ".join("%s %.3f ms" % (leg, ms) for leg, ms in zip(LEGS, res)), wall, int(out[6]["n_backpass"].max()), kern))

    say("# kernel times at B = %d, N = %d on one GPU: HIP events around %d launches on device arrays; loops: host wall time" % (B, N, a.reps))
    for n, m in SHAPES:
        legs(n, m, "wide", True)
    os.environ["DDP_GPS_WIDE"] = "1"
    legs(32, 8, "DDP_GPS_WIDE=1", False)
    del os.environ["DDP_GPS_WIDE"]
    os.environ["DDP_GPS_MID"] = "1"
    legs(32, 8, "default kernels (back_pass_gps: DDP_GPS_MID=1)", False)
    del os.environ["DDP_GPS_MID"]
    for ev in (ev0, ev1):
        _lib.check(L.ddp_event_destroy(h.raw, ev))
    finish()


if __name__ == "__main__":
    main()
