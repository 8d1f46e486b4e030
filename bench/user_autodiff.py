"""DDP_USER_AUTODIFF: ddp_user_df_ad against the hand-written ddp_user_df on the bundled examples, and wall time of a batch of car solves
with derived against hand-written derivatives.  One end-to-end run prints one line per measurement (append to profiles/user_autodiff.txt);
kernel-only times come from a separate run under `rocprofv3 --kernel-trace --stats -- python bench/user_autodiff.py --quick`.

    python bench/user_autodiff.py [--reps 20] [--quick]
"""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from user_problem import car_params, pend_params  # noqa: E402  (bench/user_problem.py: the same problems)


def lq_params(rng, n, m):
    A = np.eye(n) + 0.05 * rng.standard_normal((n, n))
    Bm = 0.1 * rng.standard_normal((n, m))
    Q = rng.standard_normal((n, n)); Q = Q @ Q.T / n + 0.1 * np.eye(n)
    R = rng.standard_normal((m, m)); R = R @ R.T / m + 0.1 * np.eye(m)
    return np.concatenate([A.ravel(order="F"), Bm.ravel(order="F"), Q.ravel(order="F"), R.ravel(order="F")])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--quick", action="store_true", help="one repetition of each step (for a profiler run)")
    a = ap.parse_args()
    reps = 1 if a.quick else a.reps
    import ddp_amd as ddp
    from ddp_amd import _lib
    h = ddp.default_handle()
    L = _lib.lib()
    rng = np.random.default_rng(0)
    ev0, ev1 = C.c_void_p(), C.c_void_p()
    L.ddp_event_create(h.raw, C.byref(ev0)); L.ddp_event_create(h.raw, C.byref(ev1))

    def timed(fn):
        fn(); h.sync()
        L.ddp_event_record(h.raw, ev0)
        for _ in range(reps):
            fn()
        L.ddp_event_record(h.raw, ev1)
        ms = C.c_float()
        L.ddp_event_elapsed_ms(h.raw, ev0, ev1, C.byref(ms))
        return ms.value / reps

    targets = {"car": 1.5, "pendcart": 1.5, "lq": 2.5}
    for name, n, m, npar, B, N, kw in (("car", 4, 2, 9, 4096, 600, dict(terminal=True)), ("pendcart", 4, 1, 25, 4096, 600, dict(terminal=True)),
                                       ("lq", 10, 2, 224, 1024, 1000, {})):
        P = car_params(rng, B) if name == "car" else (pend_params() if name == "pendcart" else lq_params(rng, n, m))
        batched = int(P.ndim == 2)
        dP = h.to_device(P); dx = h.to_device(rng.uniform(0, 4, (n, N, B))); du = h.to_device(rng.standard_normal((m, N, B)))
        outs = [h.malloc(s * N * B * 8) for s in (n * n, n * m, n, m, n * n, n * m, m * m)]
        t = {}
        for ad in (False, True):
            src = ddp.example_source(name + ("_ad" if ad else ""))
            prob = ddp.DeviceProblem(src, n, m, nparam=npar, autodiff=ad, **kw)
            up = prob._ptr(h)
            t[ad] = timed(lambda: _lib.check(L.ddp_user_df_f64_dev(h.raw, up, N, B, dP, batched, dx, du, None, *outs)))
            assert h.last_kernel(2) == ("ddp_user_df_ad" if ad else "ddp_user_df")
        byt = 8.0 * N * B * (n + m + 2 * n * n + 2 * n * m + n + m + m * m)
        r = t[True] / t[False]
        print("df %s (%d, %d) B=%d N=%d: ddp_user_df %.3f ms (%.2f of 8 TB/s), ddp_user_df_ad %.3f ms (%.2f of 8 TB/s): ratio %.2f, "
              "target <= %.1f %s" % (name, n, m, B, N, t[False], byt / t[False] * 1e-9 / 8.0, t[True], byt / t[True] * 1e-9 / 8.0, r,
                                     targets[name], "met" if r <= targets[name] else "MISSED"))
        for p in outs + [dP, dx, du]:
            h.free(p)

    # whole car solves, with limits: derived against hand-written derivatives
    n, m, B, N = 4, 2, 4096, 150
    P = car_params(rng, B)
    x0 = np.zeros((n, B)); x0[:2] = rng.uniform(0, 0.5, (2, B)); x0[2] = np.pi / 4
    u0 = 0.1 * rng.standard_normal((m, N, B))
    lims = np.array([[-2.0, 2.0], [-1.5, 1.5]])
    wall = {}
    for ad in (False, True):
        car = ddp.DeviceProblem(ddp.example_source("car_ad" if ad else "car"), n, m, nparam=9, terminal=True, autodiff=ad)
        ddp.iLQG(car, x0[:, :64], u0[..., :64], lims=lims, params=P[:, :64], max_iter=5, timing=False)
        t0 = time.perf_counter()
        r = ddp.iLQG(car, x0, u0, lims=lims, params=P, max_iter=1 if a.quick else 100, timing=False)
        wall[ad] = time.perf_counter() - t0
        st = r[6]["status"]
        print("iLQG car B=%d N=%d %s: %.3f s wall, %d batch iterations, statuses %s"
              % (B, N, "autodiff    " if ad else "hand-written", wall[ad], r[6]["global_iters"],
                 {int(s): int((st == s).sum()) for s in np.unique(st)}))
    print("iLQG car autodiff / hand-written wall: %.2f, target <= 1.25 %s" % (wall[True] / wall[False], "met" if wall[True] <= 1.25 * wall[False] else "MISSED"))


if __name__ == "__main__":
    main()
