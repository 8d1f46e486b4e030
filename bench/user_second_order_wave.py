"""DDP_USER_SECOND_ORDER_WAVE, timed with HIP events on the handle's stream (device-resident operands, the events around the backward
call alone; median of --reps):
  (a) one backward pass of ddp_user_back_pass2_wave on user_examples/chain_ddp_ad.hip at (18, 9), (34, 17) and (64, 32), B = 1 024,
      N = 200, against the same program compiled without its curvature phase P0 (the source defines DDP_BP2_NO_CURVATURE) and against
      the precompiled first-order wide pass (ddp_back_pass_f64_dev -> back_pass_wide) on the same operands, alternated inside one call;
  (b) whole solves (default options) with and without the flag: iterations and wall time of ddp_amd.iLQG.
One line per measurement (profiles/user_second_order_wave.txt).

    python bench/user_second_order_wave.py [--reps 5] [--only 18,34,64,solves] [--B 1024] [--N 200] [--solve-B 256] [--solve-N 100]
"""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

SHAPES = {"18": (18, 9), "34": (34, 17), "64": (64, 32)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--only", default="18,34,64,solves")
    ap.add_argument("--B", type=int, default=1024)
    ap.add_argument("--N", type=int, default=200)
    ap.add_argument("--solve-B", type=int, default=256)
    ap.add_argument("--solve-N", type=int, default=100)
    ap.add_argument("--solve-shapes", default="18,34,64")
    a = ap.parse_args()
    legs = set(a.only.split(","))
    import ddp_amd as ddp
    from ddp_amd import _lib
    import ddp2_wide_cases as w2
    L = _lib.lib()
    h = ddp.default_handle()
    ev0, ev1 = C.c_void_p(), C.c_void_p()
    _lib.check(L.ddp_event_create(h.raw, C.byref(ev0))); _lib.check(L.ddp_event_create(h.raw, C.byref(ev1)))
    src = ddp.example_source("chain_ddp_ad")
    prm = w2.CHAIN_P

    def timed(fn):
        h.sync()
        L.ddp_event_record(h.raw, ev0)
        fn()
        L.ddp_event_record(h.raw, ev1)
        h.sync()
        ms = C.c_float()
        _lib.check(L.ddp_event_elapsed_ms(h.raw, ev0, ev1, C.byref(ms)))
        return ms.value

    rng = np.random.default_rng(7)

    def one_pass(n, m, N, B):
        kw = dict(nparam=w2.NPARAM, autodiff=True, second_order_wave=True)
        full = ddp.DeviceProblem(src, n, m, **kw)
        bare = ddp.DeviceProblem("#define DDP_BP2_NO_CURVATURE 1\n" + src, n, m, **kw)
        x0 = 0.3 * rng.standard_normal((n, B)); u0 = 0.3 * rng.standard_normal((m, N, B))
        x, u, _ = ddp.forward_pass(None, x0, u0, None, 1.0, full, None, params=prm)
        bufs = []

        def up(arr):
            p_ = h.to_device(_lib.f64(arr)); bufs.append(p_); return p_

        def out(*shape):
            p_ = h.malloc(int(np.prod(shape)) * 8); bufs.append(p_); return p_
        dprm, dx, du, dlam = up(prm), up(x), up(u), up(np.ones(B))
        fx, fu, cx, cu, cxx, cxu, cuu = out(n, n, N, B), out(n, m, N, B), out(n, N, B), out(m, N, B), out(n, n, N, B), out(n, m, N, B), out(m, m, N, B)
        _lib.check(L.ddp_user_df_f64_dev(h.raw, full._ptr(h), N, B, dprm, 0, dx, du, None, fx, fu, cx, cu, cxx, cxu, cuu))
        res = [out(m, n, N, B), out(m, N, B), out(m, m, N, B), out(n, N, B), out(n, n, N, B), out(2, B)]
        div = h.malloc(4 * B); bufs.append(div)
        d = _lib.BPDesc(n, m, N, B, 1, 1, 1, 1, 1, 0)

        def second(prob):
            return lambda: _lib.check(L.ddp_user_back_pass_f64_dev(h.raw, prob._ptr(h), N, B, dprm, 0, dx, du, fx, fu, cx, cu, cxx, cxu, cuu,
                                                                  dlam, 1, None, None, *res, div))
        first = lambda: _lib.check(L.ddp_back_pass_f64_dev(h.raw, C.byref(d), cx, cu, cxx, cxu, cuu, fx, fu, dlam, None, None, None, *res, div))  # noqa: E731
        t = {"second": [], "bare": [], "first": []}
        try:
            second(full)(); k2 = h.last_kernel(0)
            second(bare)(); first()                                # warm
            k1 = h.last_kernel(0)
            ndiv = int(np.count_nonzero(h.to_host(div, (B,), np.int32)))
            for _ in range(a.reps):
                t["second"].append(timed(second(full))); t["bare"].append(timed(second(bare))); t["first"].append(timed(first))
        finally:
            for p_ in bufs:
                h.free(p_)
        med = {k_: float(np.median(v_)) for k_, v_ in t.items()}
        print("back pass chain_ddp_ad n=%d m=%d N=%d B=%d: %s %.3f ms, without P0 %.3f ms (P0 share %.0f %%), first-order (%s) %.3f ms: "
              "with P0 %.2fx, without P0 %.2fx of it (first-order passes that diverged: %d)"
              % (n, m, N, B, k2, med["second"], med["bare"], 100.0 * (med["second"] - med["bare"]) / med["second"], k1, med["first"],
                 med["second"] / med["first"], med["bare"] / med["first"], ndiv), flush=True)

    for key, (n, m) in SHAPES.items():
        if key in legs:
            one_pass(n, m, a.N, a.B)
    if "solves" in legs:
        B, N = a.solve_B, a.solve_N
        for key in a.solve_shapes.split(","):
            n, m = SHAPES[key]
            x0 = np.concatenate([0.8 * rng.standard_normal((m, B)), 0.5 * rng.standard_normal((m, B))])
            u0 = 0.3 * rng.standard_normal((m, N, B))
            for second in (False, True):
                prob = ddp.DeviceProblem(src, n, m, nparam=w2.NPARAM, autodiff=True, wave=True, second_order_wave=second)
                ddp.iLQG(prob, x0[:, :4], u0[:, :, :4], params=prm, max_iter=2, timing=False)      # compile, warm
                t0 = time.perf_counter()
                r = ddp.iLQG(prob, x0, u0, params=prm, timing=False)
                dt = time.perf_counter() - t0
                it, st = r[6]["iter"], r[6]["status"]
                print("%d chain_ddp_ad solves n=%d m=%d N=%d second_order_wave=%s: %.1f ms wall, iterations total %d, mean %.1f, max %d, "
                      "global iterations %d, final cost mean %.4f, statuses %s"
                      % (B, n, m, N, second, 1e3 * dt, int(it.sum()), it.mean(), int(it.max()), int(r[6]["global_iters"]),
                         float(r[5].sum(0).mean()), dict(zip(*np.unique(st, return_counts=True)))), flush=True)


if __name__ == "__main__":
    main()
