"""User problems (DeviceProblem) through the KL-constrained loop, timed with HIP events on the handle's stream:
  (a) back_pass_gps alone at B = 1 024 with per-trajectory, time-varying operands for (n, m, N) = (10, 2, 1000), (24, 4, 300), (32, 8, 300):
      the mid kernel (DDP_GPS_MID=1: prepass + back_pass_mid_kernel<GPS> + Quui post-kernel) against the 64-lane generic kernel
      (DDP_GPS_MID=0), alternated inside one call, and the iLQG mid kernel (ddp_back_pass_f64_dev, DDP_BACKPASS=m) on the same operands
      as context; algorithmic bytes (every operand read once, every result written once) and the fraction of 8 TB/s they make;
  (b) whole solves on device-resident arrays, the events around ddp_user_ilqgkl_f64_dev / ddp_ilqgkl_f64_dev alone: user lq 10x2
      (B = 1 024, N = 1 000) against the registered LQ iLQGkl on the same problem, the user car (B = 4 096, N = 150), the user pendulum at
      config 5's B = 4 096, N = 600; ms per KL iteration = the call's time / its iterations (STEP 1 and the summary included).
Every shape is warmed before it is timed.  One line per measurement (append to profiles/user_kl.txt).  Kernel shares: a separate run
under `rocprofv3 --kernel-trace --stats -- python bench/user_kl.py --only lq,pend --solve-reps 1 --max-iter 3`.

    python bench/user_kl.py [--reps 5] [--solve-reps 3] [--max-iter 10] [--only gps,lq,car,pend]
"""
import argparse
import ctypes as C
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
HBM = 8.0e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--solve-reps", type=int, default=3)
    ap.add_argument("--max-iter", type=int, default=10)
    ap.add_argument("--only", default="gps,lq,car,pend", help="comma-separated legs: gps, lq, car, pend")
    a = ap.parse_args()
    legs = set(a.only.split(","))
    import ddp_amd as ddp
    from ddp_amd import _lib
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

    def env(k, v):
        if v is None:
            os.environ.pop(k, None)
        else:
            os.environ[k] = v
        h.raw                                               # (re-reads the switches)

    rng = np.random.default_rng(7)
    B = 1024
    if "gps" in legs:
        # ---- (a) the backward pass alone
        for n, m, N in ((10, 2, 1000), (24, 4, 300), (32, 8, 300)):
            NB = N * B
            def dev(*shape, s=1.0):
                return h.to_device(s * rng.standard_normal(shape))
            fx = h.to_device(np.eye(n)[:, :, None, None] + 0.05 * rng.standard_normal((n, n, N, B)))
            fu, cx, cu, u = dev(n, m, N, B, s=0.3), dev(n, N, B), dev(m, N, B), dev(m, N, B, s=0.1)
            cxx = h.to_device(np.broadcast_to(np.eye(n)[:, :, None, None], (n, n, N, B)) * (1.0 + 0.1 * rng.random((1, 1, N, B))))
            cxu = dev(n, m, N, B, s=0.01)
            cuu = h.to_device(np.broadcast_to(np.eye(m)[:, :, None, None], (m, m, N, B)) * 1.0)
            kcx, kcu, kcxu = dev(n, N, B, s=0.01), dev(m, N, B, s=0.01), dev(m, n, N, B, s=0.01)
            kcxx = h.to_device(np.broadcast_to(0.01 * np.eye(n)[:, :, None, None], (n, n, N, B)) * 1.0)
            kcuu = h.to_device(np.broadcast_to(np.eye(m)[:, :, None, None], (m, m, N, B)) * 1.0)
            eta = h.to_device(np.ones(B))
            lam = h.to_device(np.ones(B))
            outs = [h.malloc(8 * s * NB) for s in (m * n, m, m * m, m * m, n, n * n)] + [h.malloc(16 * B), h.malloc(4 * B)]
            K, k, Quu, Quui, Vx, Vxx, dV, div = outs
            d = _lib.BPDesc(n, m, N, B, 1, 1, 1, 1, 1, 0)
            t = _lib.KLCostTerms(kcx, kcu, kcxx, kcxu, kcuu, eta, 0)
            gps = lambda: _lib.check(L.ddp_back_pass_gps_f64_dev(h.raw, C.byref(d), cx, cu, cxx, cxu, cuu, fx, fu, C.byref(t), None, None,  # noqa: E731
                                                                 None, K, k, Quu, Quui, Vx, Vxx, dV, div))
            ilqg = lambda: _lib.check(L.ddp_back_pass_f64_dev(h.raw, C.byref(d), cx, cu, cxx, cxu, cuu, fx, fu, lam, None, None, None,  # noqa: E731
                                                              K, k, Quu, Vx, Vxx, dV, div))
            res = {"mid": [], "generic": [], "ilqg_mid": []}
            for v in ("1", "0"):                                # warm both
                env("DDP_GPS_MID", v); gps()
            env("DDP_GPS_MID", None); env("DDP_BACKPASS", "m"); ilqg()
            assert h.last_kernel(0) == "back_pass_mid_kernel", h.last_kernel(0)
            env("DDP_BACKPASS", None)
            for _ in range(a.reps):
                env("DDP_GPS_MID", "1"); res["mid"].append(timed(gps)); assert h.last_kernel(0) == "back_pass_gps_mid"
                env("DDP_GPS_MID", "0"); res["generic"].append(timed(gps)); assert h.last_kernel(0) == "back_pass_gps"
                env("DDP_GPS_MID", None); env("DDP_BACKPASS", "m"); res["ilqg_mid"].append(timed(ilqg)); env("DDP_BACKPASS", None)
            per = (n * n + n * m + n + m + n * n + n * m + m * m) + (n + m + n * n + m * n + m * m) + (m * n + m + 2 * m * m + n + n * n)
            byts = 8.0 * per * NB
            med = {k_: float(np.median(v_)) for k_, v_ in res.items()}
            print("gps back pass n=%d m=%d N=%d B=%d per-trajectory TV operands: mid-GPS %.3f ms, generic %.3f ms (%.2fx), iLQG mid %.3f ms "
                  "(mid-GPS / iLQG mid %.2fx); algorithmic %.2f GB -> mid-GPS %.3f of HBM, generic %.3f"
                  % (n, m, N, B, med["mid"], med["generic"], med["generic"] / med["mid"], med["ilqg_mid"], med["mid"] / med["ilqg_mid"],
                     byts / 1e9, byts / (med["mid"] * 1e-3) / HBM, byts / (med["generic"] * 1e-3) / HBM), flush=True)
            for p_ in [fx, fu, cx, cu, u, cxx, cxu, cuu, kcx, kcu, kcxu, kcxx, kcuu, eta, lam] + outs:
                h.free(p_)
    # ---- (b) whole solves on device-resident arrays: the events bracket ddp_user_ilqgkl_f64_dev / ddp_ilqgkl_f64_dev alone (inputs uploaded
    # and outputs allocated before; ms per KL iteration = the call's time / its batch-level iterations)
    import scipy.linalg as sla

    def dev_solve(n, m, N, Bq, x, u, c0, R1, kl_step, max_iter, user=None, params=None, P=None, lims=None, mfx=None):
        bufs = []

        def up(arr):
            p_ = h.to_device(_lib.f64(arr)); bufs.append(p_); return p_

        def out(*shape):
            p_ = h.malloc(int(np.prod(shape)) * 8); bufs.append(p_); return p_
        eye = np.broadcast_to(np.eye(m)[:, :, None, None], (m, m, N, Bq))
        dx, dc0, dKp, du, dS = up(x), up(c0), up(np.zeros((m, n, N, Bq))), up(u), up(eye)
        dmf, dR1, dl = (up(mfx) if mfx is not None else None), up(R1), (up(lims) if lims is not None else None)
        dprm = up(params) if params is not None else None
        o = _lib.ILQGKLOpts()
        L.ddp_ilqgkl_default_opts(C.byref(o))
        o.kl_step, o.max_iter = float(kl_step), int(max_iter)
        res = [out(n, N, Bq), out(m, N, Bq), out(m, n, N, Bq), out(m, m, N, Bq), out(m, m, N, Bq), out(n, N, Bq), out(n, n, N, Bq),
               out(N + 1, Bq), out(2, Bq), out(12, Bq)]
        its = C.c_int(0)
        if P is not None:
            P, (A_, B_, Q_, R_) = P
            P.A, P.Bm, P.Q, P.R = up(A_), up(B_), up(Q_), up(R_)

        def call():
            if user is not None:
                _lib.check(L.ddp_user_ilqgkl_f64_dev(h.raw, user._ptr(h), N, Bq, dprm, int(params is not None and np.ndim(params) == 2),
                                                     C.byref(o), dx, dc0, dKp, du, dS, dS, dmf, int(mfx is not None and mfx.ndim == 4), dR1, dl,
                                                     None, *res, C.byref(its)))
            else:
                _lib.check(L.ddp_ilqgkl_f64_dev(h.raw, C.byref(P), C.byref(o), dx, dc0, dKp, du, dS, dS, dmf, int(mfx.ndim == 4), dR1, dl,
                                                None, *res, C.byref(its)))
        try:
            call()                                                                      # warm (compiles / loads the user module)
            ms = [timed(call) for _ in range(a.solve_reps)]
            kern = h.last_kernel(0)
        finally:
            for p_ in bufs:
                h.free(p_)
        return float(np.median(ms)), its.value, kern

    def lq_problem(A, Bm, Q, R, N, Bq):
        P = _lib.Problem()
        P.kind, P.n, P.m, P.N, P.B, P.cost_diag = 0, A.shape[0], Bm.shape[1], N, Bq, 1
        return P, (A, Bm, Q, R)

    if "lq" in legs:
        n, m, N, Bq, hh = 10, 2, 1000, 1024, 0.01
        A0 = rng.standard_normal((n, n)); A = sla.expm(hh * (A0 - A0.T)); Bm = hh * rng.standard_normal((n, m))
        Q, R = hh * np.eye(n), 0.1 * hh * np.eye(m)
        u = 0.1 * rng.standard_normal((m, N, Bq))
        x = np.zeros((n, N, Bq)); x[:, 0, :] = 1.0 + 0.1 * rng.standard_normal((n, Bq))
        for t_ in range(N - 1):
            x[:, t_ + 1, :] = A @ x[:, t_, :] + Bm @ u[:, t_, :]
        c0 = 0.5 * np.einsum("itb,ij,jtb->b", x, Q, x) + 0.5 * np.einsum("itb,ij,jtb->b", u, R, u)
        fx = np.repeat(A[:, :, None], N, 2); R1 = 1e-4 * np.eye(n)
        lq = ddp.DeviceProblem(ddp.example_source("lq"), n, m, nparam=2 * n * n + n * m + m * m)
        prm = np.concatenate([A.ravel(order="F"), Bm.ravel(order="F"), Q.ravel(order="F"), R.ravel(order="F")])
        t_reg, i_reg, k_reg = dev_solve(n, m, N, Bq, x, u, c0, R1, 2e-4, a.max_iter, P=lq_problem(A, Bm, Q, R, N, Bq), mfx=fx)
        t_usr, i_usr, k_usr = dev_solve(n, m, N, Bq, x, u, c0, R1, 2e-4, a.max_iter, user=lq, params=prm)
        print("iLQGkl device entry, lq 10x2 B=%d N=%d (max_iter %d): user %.1f ms (%s, %d iterations, %.2f ms per KL iteration), registered "
              "%.1f ms (%s, %d iterations, %.2f ms per KL iteration)" % (Bq, N, a.max_iter, t_usr, k_usr, i_usr, t_usr / i_usr, t_reg, k_reg,
                                                                        i_reg, t_reg / i_reg), flush=True)
    if "car" in legs:
        n, m, N, Bq = 4, 2, 150, 4096
        P = np.empty((9, Bq)); P[0] = 0.05; P[1:3] = 4.0 + rng.uniform(-0.5, 0.5, (2, Bq)); P[3:5] = 2.0 + rng.uniform(-0.3, 0.3, (2, Bq))
        P[5] = 0.6 + rng.uniform(0, 0.3, Bq); P[6] = rng.uniform(5.0, 20.0, Bq); P[7] = 0.1; P[8] = rng.uniform(5.0, 20.0, Bq)
        car = ddp.DeviceProblem(ddp.example_source("car"), n, m, nparam=9, terminal=True, params=P)
        u = 0.3 * rng.standard_normal((m, N, Bq))
        x, _, c = ddp.forward_pass(None, np.array([0.0, 0.0, 0.3, 0.5])[:, None] + 0.05 * rng.standard_normal((n, Bq)), u, None, 1.0, car, None)
        t_car, i_car, k_car = dev_solve(n, m, N, Bq, x, u, c.sum(axis=0), 1e-3 * np.eye(n), 0.5, a.max_iter, user=car, params=P)
        print("iLQGkl device entry, user car B=%d N=%d (max_iter %d): %.1f ms (%s, %d iterations, %.2f ms per KL iteration)"
              % (Bq, N, a.max_iter, t_car, k_car, i_car, t_car / i_car), flush=True)
    if "pend" in legs:
        n, m, N, Bq = 4, 1, 600, 4096
        prm = np.concatenate([[9.82, 0.35, 0.01, 0.99], [np.pi, 0, 0, 0], np.diag([10.0, 1, 2, 1]).ravel(order="F"), [1.0]])
        pend = ddp.DeviceProblem(ddp.example_source("pendcart"), n, m, nparam=25, terminal=True, params=prm)
        u = 0.2 * rng.standard_normal((m, N, Bq))
        x, _, c = ddp.forward_pass(None, np.array([0.3, 0.0, 0.0, 0.0])[:, None] + 0.05 * rng.standard_normal((n, Bq)), u, None, 1.0, pend, None)
        t_p, i_p, k_p = dev_solve(n, m, N, Bq, x, u, c.sum(axis=0), 1e-4 * np.eye(n), 0.5, a.max_iter, user=pend, params=prm,
                                  lims=np.array([[-5.0, 5.0]]))
        print("iLQGkl device entry, user pendulum B=%d N=%d (max_iter %d): %.1f ms (%s, %d iterations, %.2f ms per KL iteration)"
              % (Bq, N, a.max_iter, t_p, k_p, i_p, t_p / i_p), flush=True)

if __name__ == "__main__":
    main()
