"""DDP_USER_SECOND_ORDER, timed with HIP events on the handle's stream (device-resident operands, the events around the backward call
alone):
  (a) one backward pass of ddp_user_back_pass2 against the default first-order dispatch (ddp_back_pass_f64_dev) on the same operands,
      and against the same kernel compiled without its curvature phase (the source defines DDP_BP2_NO_CURVATURE), alternated inside
      one call: bicycle (B = 4 096, N = 150), lq 10x2 (B = 1 024, N = 1 000; H = 0, pure overhead), chain 24x4 (B = 1 024, N = 300);
  (b) 4 096 bicycle solves (N = 60, default options) with and without the flag: iterations and wall time of ddp_amd.iLQG.
One line per measurement (profiles/user_second_order.txt).

    python bench/user_second_order.py [--reps 5] [--only bike,lq,chain,solves]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--only", default="bike,lq,chain,solves")
    a = ap.parse_args()
    legs = set(a.only.split(","))
    import ddp_amd as ddp
    from ddp_amd import _lib
    import ddp2_reference as d2
    L = _lib.lib()
    h = ddp.default_handle()
    ev0, ev1 = C.c_void_p(), C.c_void_p()
    _lib.check(L.ddp_event_create(h.raw, C.byref(ev0))); _lib.check(L.ddp_event_create(h.raw, C.byref(ev1)))

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

    def one_pass(name, src, n, m, N, B, flags, prm, x0, u0):
        kw = dict(nparam=prm.shape[0], terminal=bool(flags & 1), autodiff=True, second_order=True)
        full = ddp.DeviceProblem(src, n, m, **kw)
        bare = ddp.DeviceProblem("#define DDP_BP2_NO_CURVATURE 1\n" + src, n, m, **kw)
        x, u, _ = ddp.forward_pass(None, x0, u0, None, 1.0, full, None, params=prm)
        bufs = []

        def up(arr):
            p_ = h.to_device(_lib.f64(arr)); bufs.append(p_); return p_

        def out(*shape):
            p_ = h.malloc(int(np.prod(shape)) * 8); bufs.append(p_); return p_
        pb = int(prm.ndim == 2)
        dprm, dx, du, dlam = up(prm), up(x), up(u), up(np.ones(B))
        fx, fu, cx, cu, cxx, cxu, cuu = out(n, n, N, B), out(n, m, N, B), out(n, N, B), out(m, N, B), out(n, n, N, B), out(n, m, N, B), out(m, m, N, B)
        _lib.check(L.ddp_user_df_f64_dev(h.raw, full._ptr(h), N, B, dprm, pb, dx, du, None, fx, fu, cx, cu, cxx, cxu, cuu))
        res = [out(m, n, N, B), out(m, N, B), out(m, m, N, B), out(n, N, B), out(n, n, N, B), out(2, B)]
        div = h.malloc(4 * B); bufs.append(div)
        d = _lib.BPDesc(n, m, N, B, 1, 1, 1, 1, 1, 0)

        def second(prob):
            return lambda: _lib.check(L.ddp_user_back_pass_f64_dev(h.raw, prob._ptr(h), N, B, dprm, pb, dx, du, fx, fu, cx, cu, cxx, cxu, cuu,
                                                                  dlam, 1, None, None, *res, div))
        first = lambda: _lib.check(L.ddp_back_pass_f64_dev(h.raw, C.byref(d), cx, cu, cxx, cxu, cuu, fx, fu, dlam, None, None, None, *res, div))  # noqa: E731
        t = {"second": [], "bare": [], "first": []}
        try:
            second(full)(); second(bare)(); first()                # warm
            k1 = h.last_kernel(0)
            for _ in range(a.reps):
                t["second"].append(timed(second(full))); t["bare"].append(timed(second(bare))); t["first"].append(timed(first))
        finally:
            for p_ in bufs:
                h.free(p_)
        med = {k_: float(np.median(v_)) for k_, v_ in t.items()}
        print("back pass %s n=%d m=%d N=%d B=%d: ddp_user_back_pass2 %.3f ms, without its curvature phase %.3f ms (AD share %.0f %%), "
              "first-order dispatch (%s) %.3f ms: %.2fx" % (name, n, m, N, B, med["second"], med["bare"],
                                                           100.0 * (med["second"] - med["bare"]) / med["second"], k1, med["first"],
                                                           med["second"] / med["first"]), flush=True)

    if "bike" in legs:
        B, N = 4096, 150
        P = np.repeat(d2.sketch_inputs(B=64)[0], B // 64, axis=1)
        x0 = np.array([0.2, 0.2, np.pi / 4, 0.5])[:, None] + 0.05 * rng.standard_normal((4, B))
        one_pass("bicycle", ddp.example_source("bicycle_ad"), 4, 2, N, B, 1, P, x0, 0.1 * rng.standard_normal((2, N, B)))
    if "lq" in legs:
        from oracle import np_restatement as npr
        n, m, N, B = 10, 2, 1000, 1024
        Pq = npr.make_lq_problem(rng, T=N)
        prm = np.concatenate([Pq[k_].ravel(order="F") for k_ in ("A", "B", "Q", "R")])
        one_pass("lq", ddp.example_source("lq_ad"), n, m, N, B, 0, prm, 1.0 + 0.1 * rng.standard_normal((n, B)), 0.1 * rng.standard_normal((m, N, B)))
    if "chain" in legs:
        n, m, N, B = 24, 4, 300, 1024
        one_pass("chain", d2.CHAIN_SOURCE, n, m, N, B, 0, d2.CHAIN_P, 0.3 * rng.standard_normal((n, B)), 0.3 * rng.standard_normal((m, N, B)))
    if "solves" in legs:
        B, N = 4096, 60
        P, x0, u0 = d2.sketch_inputs(seed=11, B=B, N=N)
        src = ddp.example_source("bicycle_ad")
        for second in (False, True):
            prob = ddp.DeviceProblem(src, 4, 2, nparam=10, terminal=True, autodiff=True, second_order=second)
            ddp.iLQG(prob, x0[:, :64], u0[:, :, :64], params=P[:, :64], max_iter=2, timing=False)      # compile, warm
            t0 = time.perf_counter()
            r = ddp.iLQG(prob, x0, u0, params=P, timing=False)
            dt = time.perf_counter() - t0
            it, st = r[6]["iter"], r[6]["status"]
            print("4096 bicycle solves N=%d second_order=%s: %.1f ms wall, iterations total %d, mean %.1f, max %d, global iterations %d, "
                  "final cost mean %.4f, statuses %s" % (N, second, 1e3 * dt, int(it.sum()), it.mean(), int(it.max()), int(r[6]["global_iters"]),
                                                         float(r[5].sum(0).mean()), dict(zip(*np.unique(st, return_counts=True)))), flush=True)


if __name__ == "__main__":
    main()
