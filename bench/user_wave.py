"""DDP_USER_WAVE: the wave kernels of large user problems at B = 1024, N = 200.  Per leg one line: the rollout (policy, one step size),
df and a whole solve (5 iterations) of chain_ad (64, 32) and lq_ad (40, 12) with the flag, the same legs of chain_ad (16, 8) with and
without it (the shape both kernel sets hold), and the registered LQ family's rollout (forward_wide_kernel) at (40, 12) as the yardstick
of the rollout.  Before that, without touching a device, the hiprtc compile time (ddp_user_check, with the compiler's resource remarks)
of every program of PROGRAMS and the VGPR / scratch / LDS records of its kernels; --compile-only stops there and writes "not measured"
for the timed legs, so the first part can be produced on a machine without a GPU.

    python bench/user_wave.py [--compile-only] [--reps 10] [--B 1024] [--N 200] [--out profiles/user_wave.txt]
"""
import argparse
import ctypes as C
import os
import re
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
CHAIN_P = np.array([0.02, 9.0, 0.3, 4.0, 1.0, 0.05, 2.0])


def lq_mats(rng, n, m):
    A0 = rng.standard_normal((n, n))
    A = np.eye(n) + 0.05 * (A0 - A0.T) / np.sqrt(n)
    Bm = 0.1 * rng.standard_normal((n, m))
    return A, Bm, 0.01 * np.eye(n), 0.001 * np.eye(m)


def records(log):
    out, cur = [], None
    for line in log.splitlines():
        mm = re.search(r"remark: Function Name: (\w+)", line)
        if mm:
            cur = {"kernel": mm.group(1)}
            out.append(cur)
            continue
        mm = re.search(r"remark:\s+(VGPRs|AGPRs|ScratchSize \[bytes/lane\]|LDS Size \[bytes/block\]|Occupancy \[waves/SIMD\]): (\d+)", line)
        if mm and cur is not None:
            cur[mm.group(1).split(" ")[0]] = int(mm.group(2))
    return out


# model, n, m, keywords of DeviceProblem, tag: the programs whose compile time and records are written
PROGRAMS = [("chain_ad", 64, 32, dict(wave=True), "wave"), ("chain_ad", 34, 17, dict(wave=True), "wave"), ("chain_ad", 18, 9, dict(wave=True), "wave"),
            ("lq_ad", 40, 12, dict(wave=True), "wave"), ("lq_ad", 40, 12, dict(wave=True, const_hessian=True), "CONST_HESSIAN wave"),
            ("lq", 33, 2, dict(wave=True), "wave"), ("lq", 10, 9, dict(wave=True), "wave"),
            ("pendcart_ad", 4, 1, dict(wave=True, terminal=True), "TERMINAL wave"),
            ("chain_ad", 16, 8, dict(wave=True), "wave"), ("chain_ad", 16, 8, dict(), "lane")]
LEGS = [("chain_ad", 64, 32, True), ("lq_ad", 40, 12, True), ("chain_ad", 16, 8, True), ("chain_ad", 16, 8, False)]


def nparam_of(name, n, m):
    return {"chain_ad": 7, "pendcart_ad": 25}.get(name, 2 * n * n + n * m + m * m)


def compile_part(ddp, say):
    """compile time and resource records of every program: ddp_user_check, no device"""
    say("# hiprtc compile times (host) and the compiler's records per kernel (-Rpass-analysis=kernel-resource-usage), from ddp_user_check")
    for name, n, m, kw, tag in PROGRAMS:
        tag = "%s (%d, %d) %s" % (name, n, m, tag)
        prob = ddp.DeviceProblem(ddp.example_source(name), n, m, nparam=nparam_of(name, n, m), autodiff=name.endswith("_ad"), **kw)
        t0 = time.perf_counter()
        log = prob.check("-Rpass-analysis=kernel-resource-usage")
        say("%s: hiprtc compile %.2f s" % (tag, time.perf_counter() - t0))
        for r in records(log):
            say("%s:   %s" % (tag, " ".join("%s=%s" % kv for kv in r.items())))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--compile-only", action="store_true")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--B", type=int, default=1024)
    ap.add_argument("--N", type=int, default=200)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import ddp_amd as ddp
    from ddp_amd import _lib
    B, N = a.B, a.N
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    def finish():
        if a.out:
            with open(a.out, "w") as f:
                f.write("\n".join(lines) + "\n")

    say("# DDP_USER_WAVE, bench/user_wave.py")
    compile_part(ddp, say)
    say("#")
    if a.compile_only:
        say("# kernel and solve times at B = %d, N = %d: not measured (--compile-only)" % (B, N))
        for name, n, m, wave in LEGS:
            say("%s (%d, %d) %s: rollout not measured; df not measured; iLQG 5 iterations not measured" % (name, n, m, "wave" if wave else "lane"))
        say("LQ family (40, 12): rollout forward_wide_kernel not measured")
        return finish()
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

    say("# kernel and solve times at B = %d, N = %d on one GPU: HIP events around %d launches; solves: host wall time" % (B, N, a.reps))
    for name, n, m, wave in LEGS:
        tag = "%s (%d, %d) %s" % (name, n, m, "wave" if wave else "lane")
        if name == "chain_ad":
            prm, npar = CHAIN_P, 7
        else:
            A, Bm, Q, R = lq_mats(rng, n, m)
            prm = np.concatenate([M.ravel(order="F") for M in (A, Bm, Q, R)])
            npar = prm.size
        prob = ddp.DeviceProblem(ddp.example_source(name), n, m, nparam=npar, autodiff=True, wave=wave)
        up = prob._ptr(h)
        x0 = 0.3 * rng.standard_normal((n, B)); u = 0.2 * rng.standard_normal((m, N, B))
        x, u1, _ = ddp.forward_pass(None, x0, u, None, 1.0, prob, None, params=prm)
        dP, dx0, du, dx = (h.to_device(v) for v in (prm, x0, u1, x))
        dK = h.to_device(0.05 * rng.standard_normal((m, n, N, B)) / np.sqrt(n)); dk = h.to_device(0.05 * rng.standard_normal((m, N, B)))
        outs = [h.malloc(8 * s) for s in (n * N * B, m * N * B, N * B, B)]
        al = np.array([0.5])
        t = timed(lambda: _lib.check(L.ddp_user_forward_pass_f64_dev(h.raw, up, N, B, dP, 0, dK, dk, dx0, du, dx, al.ctypes.data_as(C.c_void_p), 1,
                                                                     None, None, *outs)))
        byt = 8.0 * N * B * (m * n + 2 * m + 2 * n + n + m + 1)
        say("%s: rollout %s %.3f ms (%.1f GB/s of operands and results)" % (tag, h.last_kernel(1), t, byt / t * 1e-6))
        for p in outs + [dK, dk]:
            h.free(p)
        douts = [h.malloc(8 * s * N * B) for s in (n * n, n * m, n, m, n * n, n * m, m * m)]
        t = timed(lambda: _lib.check(L.ddp_user_df_f64_dev(h.raw, up, N, B, dP, 0, dx, du, None, *douts)))
        byt = 8.0 * N * B * (2 * n * n + 2 * n * m + m * m + 2 * (n + m))
        say("%s: df %s %.3f ms (%.1f GB/s)" % (tag, h.last_kernel(2), t, byt / t * 1e-6))
        for p in douts + [dP, dx0, du, dx]:
            h.free(p)
        ddp.iLQG(prob, x0[:, :8], u[..., :8], params=prm, max_iter=2, timing=False)
        t0 = time.perf_counter()
        r = ddp.iLQG(prob, x0, u, params=prm, max_iter=5, tol_grad=0.0, tol_fun=-1.0, timing=False)
        say("%s: iLQG 5 iterations %.3f s wall (host arrays in and out), backward kernel %s, %d batch iterations"
            % (tag, time.perf_counter() - t0, h.last_kernel(0), r[6]["global_iters"]))
        del prob

    # the yardstick: the registered LQ family at (40, 12)
    n, m = 40, 12
    A, Bm, Q, R = lq_mats(rng, n, m)
    x0 = 0.3 * rng.standard_normal((n, B)); u = 0.2 * rng.standard_normal((m, N, B))
    x, u1, _ = ddp.forward_pass(None, x0, u, None, 1.0, ddp.LQProblem(A, Bm, Q, R), None)
    dx0, du, dx = (h.to_device(v) for v in (x0, u1, x))
    dK = h.to_device(0.05 * rng.standard_normal((m, n, N, B)) / np.sqrt(n)); dk = h.to_device(0.05 * rng.standard_normal((m, N, B)))
    dA, dB, dQ, dR = (h.to_device(v) for v in (A, Bm, Q, R))
    P = _lib.Problem()
    P.kind, P.n, P.m, P.N, P.B = 0, n, m, N, B
    P.A, P.Bm, P.Q, P.R, P.cost_diag = dA.value, dB.value, dQ.value, dR.value, 1
    outs = [h.malloc(8 * s) for s in (n * N * B, m * N * B, N * B, B)]
    al = np.array([0.5])
    t = timed(lambda: _lib.check(L.ddp_forward_pass_f64_dev(h.raw, C.byref(P), dK, dk, dx0, du, dx, al.ctypes.data_as(C.c_void_p), 1, None, None,
                                                            *outs)))
    say("LQ family (40, 12): rollout %s %.3f ms" % (h.last_kernel(1), t))
    for p in outs + [dx0, du, dx, dK, dk, dA, dB, dQ, dR]:
        h.free(p)
    for ev in (ev0, ev1):
        _lib.check(L.ddp_event_destroy(h.raw, ev))
    finish()


if __name__ == "__main__":
    main()
