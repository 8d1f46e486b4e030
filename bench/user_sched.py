"""User problems (DeviceProblem) in the slot scheduler and the closed loop on the device, timed with HIP events on the handle's stream:
  (a) 32 768 user-pendulum solves (user_examples/pendcart.hip, N = 600, per-problem start states, control limits, regType 2) through
      4 096 slots (ddp_user_ilqg_queue_f64_dev) against eight lock-step batches of 4 096 (ddp_user_ilqg_f64_dev);
  (b) a 4 096-trajectory car closed loop (user_examples/car_plant.hip, 20 steps) with the model as the plant and with the plant
      (ddp_user_ilqg_mpc_f64_dev), as ms per closed-loop step.
Operands live on the device; one line per measurement (append to profiles/user_sched.txt).  Kernel times: a separate run under
`rocprofv3 --kernel-trace --stats -- python bench/user_sched.py --P 8192`.

    python bench/user_sched.py [--P 32768] [--slots 4096] [--B 4096] [--steps 20] [--N 600] [--Nmpc 100]
"""
import argparse
import ctypes as C
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def pend_params():
    """[g, l, h, d, goal[4], Q[4,4], R] of user_examples/pendcart.hip: the built-in family's defaults"""
    return np.concatenate([[9.82, 0.35, 0.01, 0.99], [np.pi, 0, 0, 0], np.diag([10.0, 1, 2, 1]).ravel(order="F"), [1.0]])


def car_plant_params(rng, B):
    """[h, gx, gy, ox, oy, r, wo, wu, wt, ga, gw, vx, vy] of user_examples/car_plant.hip, one column per trajectory"""
    P = np.empty((13, B))
    P[0] = 0.05
    P[1:3] = 4.0 + rng.uniform(-0.5, 0.5, (2, B))
    P[3:5] = 2.0 + rng.uniform(-0.3, 0.3, (2, B))
    P[5] = 0.6 + rng.uniform(0, 0.3, B); P[6] = rng.uniform(5.0, 20.0, B)
    P[7] = 0.1; P[8] = rng.uniform(5.0, 20.0, B)
    P[9] = rng.uniform(0.6, 0.9, B); P[10] = rng.uniform(1.1, 1.4, B)
    P[11:13] = rng.uniform(-0.5, 0.5, (2, B))
    return P


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--P", type=int, default=32768)
    ap.add_argument("--slots", type=int, default=4096)
    ap.add_argument("--B", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--N", type=int, default=600)
    ap.add_argument("--Nmpc", type=int, default=100)
    a = ap.parse_args()
    import ddp_amd as ddp
    from ddp_amd import _lib
    L = _lib.lib()
    h = ddp.default_handle()
    ev0, ev1 = C.c_void_p(), C.c_void_p()
    _lib.check(L.ddp_event_create(h.raw, C.byref(ev0))); _lib.check(L.ddp_event_create(h.raw, C.byref(ev1)))

    def timed(fn):
        """ms of fn() between two events on the handle's stream (the entry points synchronise themselves)"""
        h.sync()
        L.ddp_event_record(h.raw, ev0)
        fn()
        L.ddp_event_record(h.raw, ev1)
        h.sync()
        ms = C.c_float()
        _lib.check(L.ddp_event_elapsed_ms(h.raw, ev0, ev1, C.byref(ms)))
        return ms.value

    # ---- (a) queue against lock-step batches
    P, S, N, n, m = a.P, a.slots, a.N, 4, 1
    rng = np.random.default_rng(1234)
    x0 = np.tile(np.array([np.pi - 0.6, 0.0, 0.0, 0.0])[:, None], (1, P)); x0[0] += rng.uniform(-0.1, 0.1, P)
    pend = ddp.DeviceProblem(ddp.example_source("pendcart"), n, m, nparam=25, terminal=True)
    up = pend._ptr(h)
    o = ddp._ilqg_opts(10.0 ** np.linspace(0.2, -3, 6), 1e-8, 1e-8, 1000, 1.0, 1.0, 1.6, 1e15, 1e-6, 2, 0.0)
    dprm, dl = h.to_device(pend_params()), h.to_device(np.array([[-5.0, 5.0]]))
    dx0, du0 = h.to_device(x0), h.to_device(np.zeros((m, N, P)))

    def outs(B):
        return [h.malloc(8 * s * B) for s in (n * N, m * N, m * n * N, m * N, m * m * N, n * N, n * n * N, N + 1, 8)]

    git = C.c_int(0)
    o_q = outs(P)
    run_q = lambda: _lib.check(L.ddp_user_ilqg_queue_f64_dev(h.raw, up, N, P, dprm, 0, C.byref(o), S, dx0, du0, dl, *o_q, C.byref(git)))
    run_q()                                                     # warm-up (compile, scratch)
    tq = timed(run_q)
    st_q = h.to_host(o_q[8], (8, P))
    print("user queue pendulum: %d problems through %d slots N=%d: %.1f ms, %d global iterations, iterations per solve median %d max %d, "
          "status %s" % (P, S, N, tq, git.value, np.median(st_q[1]), st_q[1].max(),
                         dict(zip(*[v.tolist() for v in np.unique(st_q[0].astype(int), return_counts=True)]))))
    for p_ in o_q:
        h.free(p_)
    o_b = outs(S)
    st_b = np.zeros((8, P)); gits = []

    def run_b():
        gits.clear()
        for c in range(0, P, S):
            _lib.check(L.ddp_user_ilqg_f64_dev(h.raw, up, N, S, dprm, 0, C.byref(o), C.c_void_p(dx0.value + 8 * n * c), 0,
                                               C.c_void_p(du0.value + 8 * m * N * c), None, dl, *o_b[:8], o_b[8], 0, None, C.byref(git)))
            gits.append(git.value)
            st_b[:, c:c + S] = h.to_host(o_b[8], (8, S))
    tb = timed(run_b)
    print("user lock step pendulum: %d batches of %d: %.1f ms, global iterations %s" % (P // S, S, tb, gits))
    print("user queue vs lock step: same summaries %s; speed-up %.2fx; %.0f solves/s queued" % (np.array_equal(st_q, st_b), tb / tq,
                                                                                                  P / tq * 1e3))
    for p_ in o_b:
        h.free(p_)

    # ---- (b) car closed loop, model as plant vs plant
    B, T, steps, n, m = a.B, a.Nmpc, a.steps, 4, 2
    rng = np.random.default_rng(7)
    prm = car_plant_params(rng, B)
    x0 = np.zeros((n, B)); x0[:2] = rng.uniform(0, 0.5, (2, B)); x0[2] = np.pi / 4 + rng.uniform(-0.2, 0.2, B)
    u0 = 0.1 * rng.standard_normal((m, T, B))
    oc = ddp._ilqg_opts(ddp.DEFAULT_ALPHA, 1e-7, 1e-4, 100, 1.0, 1.0, 1.6, 1e10, 1e-6, 1, 0.0)
    dprm, dx0, du0 = h.to_device(prm), h.to_device(x0), h.to_device(u0)
    dl = h.to_device(np.array([[-2.0, 2.0], [-1.5, 1.5]]))
    xcl, ucl, scl = h.malloc(8 * n * (steps + 1) * B), h.malloc(8 * m * steps * B), h.malloc(8 * 8 * steps * B)
    xp, upl = h.malloc(8 * n * T * B), h.malloc(8 * m * T * B)
    src = ddp.example_source("car_plant")
    res = {}
    for name, plant in (("model as plant", False), ("plant", True)):
        car = ddp.DeviceProblem(src, n, m, nparam=13, terminal=True, plant=plant)
        upc = car._ptr(h)
        run = lambda: _lib.check(L.ddp_user_ilqg_mpc_f64_dev(h.raw, upc, T, B, dprm, 1, C.byref(oc), steps, 0, dx0, du0, dl, xcl, ucl, scl,
                                                             xp, upl, C.byref(git)))
        run()
        t = timed(run)
        st = h.to_host(scl, (8, steps, B))
        res[name] = h.to_host(xcl, (n, steps + 1, B))
        print("user car mpc (%s): B=%d N=%d steps=%d: %.1f ms, %.2f ms per closed-loop step, %d global iterations, iterations per solve "
              "median %d max %d, statuses %s" % (name, B, T, steps, t, t / steps, git.value, np.median(st[1]), st[1].max(),
                                                 dict(zip(*[v.tolist() for v in np.unique(st[0].astype(int), return_counts=True)]))))
    print("user car mpc: final state plant vs model-as-plant, max |diff| %.3g" % np.abs(res["plant"][:, -1] - res["model as plant"][:, -1]).max())


if __name__ == "__main__":
    main()
