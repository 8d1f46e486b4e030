"""User problems (DeviceProblem): compile time, the user pendulum rollout against the built-in one, the car's derivative kernel against
HBM, and wall time of a batch of car solves.  One end-to-end run prints one line per measurement (append to profiles/user_problem.txt);
kernel times come from a separate run under `rocprofv3 --kernel-trace --stats -- python bench/user_problem.py --quick`.

    python bench/user_problem.py [--B 4096] [--N 600] [--reps 20] [--quick]
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def pend_params():
    """[g, l, h, d, goal[4], Q[4,4], R] of user_examples/pendcart.hip: the built-in family's defaults"""
    return np.concatenate([[9.82, 0.35, 0.01, 0.99], [np.pi, 0, 0, 0], np.diag([10.0, 1, 2, 1]).ravel(order="F"), [1.0]])


def car_params(rng, B):
    """[h, gx, gy, ox, oy, r, wo, wu, wt] of user_examples/car.hip, one column per trajectory"""
    P = np.empty((9, B))
    P[0] = 0.05
    P[1:3] = 4.0 + rng.uniform(-0.5, 0.5, (2, B))
    P[3:5] = 2.0 + rng.uniform(-0.3, 0.3, (2, B))
    P[5] = 0.6 + rng.uniform(0, 0.3, B); P[6] = rng.uniform(5.0, 20.0, B)
    P[7] = 0.1; P[8] = rng.uniform(5.0, 20.0, B)
    return P


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=4096)
    ap.add_argument("--N", type=int, default=600)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--quick", action="store_true", help="one repetition of each step (for a profiler run)")
    a = ap.parse_args()
    reps = 1 if a.quick else a.reps
    import ddp_amd as ddp
    from ddp_amd import _lib
    h = ddp.default_handle()
    B, N = a.B, a.N
    rng = np.random.default_rng(0)

    # compile time: a fresh handle compiles (the cache is per handle)
    for name, n, m, npar, kw in (("pendcart", 4, 1, 25, dict(terminal=True)), ("car", 4, 2, 9, dict(terminal=True))):
        hh = ddp.Handle(0)
        p = ddp.DeviceProblem(ddp.example_source(name), n, m, nparam=npar, **kw)
        t = time.perf_counter(); p._ptr(hh); dt = time.perf_counter() - t
        print("compile+load %-9s %.3f s" % (name, dt))
        del p
        hh.close()

    # rollouts: user pendulum vs built-in, B x 11 step sizes, device pointers, HIP events
    pend = ddp.DeviceProblem(ddp.example_source("pendcart"), 4, 1, nparam=25, params=pend_params(), terminal=True)
    n, m = 4, 1
    al = np.ascontiguousarray(ddp.DEFAULT_ALPHA); na = len(al)
    x0 = np.array([0.3, 0, 0, 0.0])[:, None] + 0.05 * rng.standard_normal((n, B))
    dev = {k: h.to_device(v) for k, v in dict(x0=x0, u=0.3 * rng.standard_normal((m, N, B)), K=0.2 * rng.standard_normal((m, n, N, B)),
                                              k=0.2 * rng.standard_normal((m, N, B)), x=x0[:, None, :] + 0.05 * rng.standard_normal((n, N, B)),
                                              lims=np.array([[-1.0, 1.0]]), params=pend_params()).items()}
    xn = h.malloc(n * N * B * na * 8); un = h.malloc(m * N * B * na * 8); cn = h.malloc((N + 1) * B * na * 8); cs = h.malloc(B * na * 8)
    dp = ddp._DevProblem(ddp.PendcartProblem(), N, B)
    Pd = dp.struct
    Pd.Q, Pd.R = h.to_device(dp.Q), h.to_device(dp.R)
    L = _lib.lib()
    up = pend._ptr(h)
    import ctypes as C
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

    t_b = timed(lambda: _lib.check(L.ddp_forward_pass_f64_dev(h.raw, C.byref(Pd), dev["K"], dev["k"], dev["x0"], dev["u"], dev["x"],
                                                            _lib.ptr(al), na, dev["lims"], None, xn, un, cn, cs)))
    t_u = timed(lambda: _lib.check(L.ddp_user_forward_pass_f64_dev(h.raw, up, N, B, dev["params"], 0, dev["K"], dev["k"], dev["x0"],
                                                                 dev["u"], dev["x"], _lib.ptr(al), na, dev["lims"], None, xn, un, cn, cs)))
    print("rollout pendulum B=%d N=%d nalpha=%d: built-in %.3f ms (%s), user %.3f ms (ddp_user_rollout): ratio %.2f"
          % (B, N, na, t_b, "forward kernel of the family", t_u, t_u / t_b))

    # derivative kernel of the car: algorithmic bytes (x, u in; fx fu cx cu cxx cxu cuu out) over kernel time
    car = ddp.DeviceProblem(ddp.example_source("car"), 4, 2, nparam=9, terminal=True)
    n, m = 4, 2
    P = car_params(rng, B)
    dP = h.to_device(P); dx = h.to_device(rng.uniform(0, 4, (n, N, B))); du = h.to_device(rng.standard_normal((m, N, B)))
    outs = [h.malloc(s * N * B * 8) for s in (16, 8, 4, 2, 16, 8, 4)]
    upc = car._ptr(h)
    t_d = timed(lambda: _lib.check(L.ddp_user_df_f64_dev(h.raw, upc, N, B, dP, 1, dx, du, None, *outs)))
    byt = 8.0 * N * B * (n + m + 16 + 8 + 4 + 2 + 16 + 8 + 4)
    print("df car B=%d N=%d: %.3f ms, %.2f TB/s algorithmic (%.2f of 8 TB/s HBM)" % (B, N, t_d, byt / t_d * 1e-9, byt / t_d * 1e-9 / 8.0))

    # whole solves of the car
    x0c = np.zeros((n, B)); x0c[:2] = rng.uniform(0, 0.5, (2, B)); x0c[2] = np.pi / 4
    u0 = 0.1 * rng.standard_normal((m, N // 4, B))
    lims = np.array([[-2.0, 2.0], [-1.5, 1.5]])
    ddp.iLQG(car, x0c[:, :64], u0[..., :64], lims=lims, params=P[:, :64], max_iter=5, timing=False)
    t = time.perf_counter()
    r = ddp.iLQG(car, x0c, u0, lims=lims, params=P, max_iter=100, timing=False)
    wall = time.perf_counter() - t
    st = r[6]["status"]
    print("iLQG car B=%d N=%d: %.3f s wall, %d batch iterations, statuses %s"
          % (B, N // 4, wall, r[6]["global_iters"], {int(s): int((st == s).sum()) for s in np.unique(st)}))


if __name__ == "__main__":
    main()
