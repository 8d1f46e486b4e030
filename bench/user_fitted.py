"""DDP_USER_FITTED: the rollout and the whole KL loop on fitted time-varying affine dynamics, against what a user could do before the
flag — the same tables written into the parameter block of user_examples/car_table.hip and run on the existing kernels.
  (1) ddp_user_rollout_fit_f64_dev against ddp_user_forward_pass_f64_dev of car_table: B car_plant policies, N = 50, tables from one
      sample_policy(plant=True) + fit_dynamics, closed loop with limits, one step size;
  (2) ddp_user_ilqgkl_fit_f64_dev against ddp_user_ilqgkl_f64_dev of car_table on the same inputs (whole solves);
  (3) (n, m) = (32, 8), N = 50, B2 trajectories, lq cost, designed tables: no emulation exists (nparam is capped at 4096), the kernel
      time and its share of the 8 TB/s roofline by algorithmic bytes;
  (4) information, not a test: the noise-free cost on the gain-mismatched plant over three guided-policy-search rounds with
      fitted=True and with fitted=False.
Every pair alternates inside one process, five windows each, every figure given per window.  One line per measurement (append to
profiles/user_fitted.txt).

    python bench/user_fitted.py [--B 1024] [--N 50] [--B2 128] [--repeats 5] [--inner 200] [--inner-kl 3] [--gps-B 64]
"""
import argparse
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from user_clock import Bench, car_plant_params       # noqa: E402
from user_sample import spread                       # noqa: E402

RIDGE = 1e-3
LIMS = np.array([[-2.0, 2.0], [-1.5, 1.5]])


def table_params(P9, fx, fu, fc):
    """the parameter block of car_table.hip: [9 cost parameters | per step fx (16) | fu (8) | fc (4)], one column per trajectory"""
    N, B = fc.shape[1], fc.shape[2]
    T = np.concatenate([fx.reshape(16, N, B, order="F"), fu.reshape(8, N, B, order="F"), fc], axis=0)
    return np.asfortranarray(np.concatenate([P9, T.reshape(28 * N, B, order="F")], axis=0))


def setup(ddp, B, N, seed=11, S=64):
    """B car_plant policies and the tables fitted to their noisy closed loop on the plant"""
    n, m = 4, 2
    rng = np.random.default_rng(seed)
    prm = car_plant_params(rng, B)
    x0 = np.zeros((n, B)); x0[:2] = rng.uniform(0, 0.5, (2, B)); x0[2] = np.pi / 4 + rng.uniform(-0.2, 0.2, B); x0[3] = 1.0
    u = 0.1 * rng.standard_normal((m, N, B))
    K = -0.4 * rng.random((m, n, N, B))
    G = rng.standard_normal((m, m, N, B))
    Sigma = 0.04 * (np.einsum("ikjb,lkjb->iljb", G, G) / m + 0.5 * np.eye(m)[:, :, None, None])
    Sigmai = np.stack([np.stack([np.linalg.inv(Sigma[:, :, t, b]) for t in range(N)], -1) for b in range(B)], -1)
    car = ddp.DeviceProblem(ddp.example_source("car_plant"), n, m, nparam=13, terminal=True, plant=True, sample=True, fitted=True)
    x = ddp.forward_pass(ddp.GaussianPolicy(), x0, u, None, 1.0, car, LIMS, params=prm)[0]
    traj = ddp.GaussianPolicy(N, n, m, K, u, Sigma, Sigmai)
    xs, us, _, _ = ddp.sample_policy(car, traj, x0, x, u, S, seed=20240611, lims=LIMS, plant=True, params=prm)
    fx, fu, fc, _, st = ddp.fit_dynamics(xs, us, ridge=RIDGE)
    assert not np.any(st), "fit_dynamics rejected %d steps" % np.count_nonzero(st)
    return car, prm, x0, u, traj, (fx, fu, fc)


def windows(b, a, f1, f2, inner):
    t1, t2 = [], []
    f1(); f2(); b.h.sync()
    for _ in range(a.repeats):
        t1.append(b.timed(lambda: [f1() for _ in range(inner)]) / inner)
        t2.append(b.timed(lambda: [f2() for _ in range(inner)]) / inner)
    return t1, t2


def verdict(t1, t2):
    m1, m2 = float(np.median(t1)), float(np.median(t2))
    s1, s2 = (max(t1) - min(t1)) / m1, (max(t2) - min(t2)) / m2
    return "fitted over emulation %.2fx the time (medians); the two spreads %.1f%% + %.1f%%: %s" % (
        m1 / m2, 100 * s1, 100 * s2, "not slower beyond the spreads" if m1 <= m2 * (1 + s1 + s2) else "SLOWER beyond the spreads")


def pair_car(b, a):
    ddp, _lib, L, h = b.ddp, b._lib, b.L, b.h
    B, N, n, m = a.B, a.N, 4, 2
    car, prm, x0, u, traj, (fx, fu, fc) = setup(ddp, B, N)
    tab = ddp.DeviceProblem(ddp.example_source("car_table"), n, m, nparam=9 + 28 * N, terminal=True)
    PT = table_params(prm[:9], fx, fu, fc)
    # the nominal consistent with the tables, and its cost
    x, _, c = ddp.forward_pass(None, x0, u, None, 1.0, car, LIMS, params=prm, model=(fx, fu, fc))
    c0 = c.sum(axis=0)
    T = N * B
    one = np.array([1.0])
    dev = {k: h.to_device(np.asfortranarray(v)) for k, v in dict(prm=prm, PT=PT, K=traj.K, k0=np.zeros((m, N, B)), x0=x0, u=u, x=x, fx=fx, fu=fu,
                                                                 fc=fc, lims=LIMS, Sp=traj.Σ, Sip=traj.Σi, c0=c0, R1=1e-3 * np.eye(n)).items()}
    out = [[h.malloc(8 * n * T), h.malloc(8 * m * T), h.malloc(8 * (N + 1) * B), h.malloc(8 * B)] for _ in range(2)]
    upf, upt = car._ptr(h), tab._ptr(h)
    al = one.ctypes.data_as(C.c_void_p)

    def roll_fit():
        _lib.check(L.ddp_user_rollout_fit_f64_dev(h.raw, upf, N, B, dev["prm"], 1, dev["K"], dev["k0"], dev["x0"], dev["u"], dev["x"], al, 1,
                                                  dev["lims"], None, dev["fx"], dev["fu"], dev["fc"], *out[0]))

    def roll_tab():
        _lib.check(L.ddp_user_forward_pass_f64_dev(h.raw, upt, N, B, dev["PT"], 1, dev["K"], dev["k0"], dev["x0"], dev["u"], dev["x"], al, 1,
                                                   dev["lims"], None, *out[1]))

    roll_fit(); roll_tab(); h.sync()
    xa, xb = h.to_host(out[0][0], (n, N, B)), h.to_host(out[1][0], (n, N, B))
    what = "car_plant B=%d N=%d, tables of sample_policy(plant) + fit_dynamics" % (B, N)
    print("%s: rollout on the tables, ddp_user_rollout_fit vs car_table on ddp_user_rollout: states differ by %.3g (relative, max)"
          % (what, float(np.abs(xa - xb).max() / np.abs(xb).max())), flush=True)
    t1, t2 = windows(b, a, roll_fit, roll_tab, a.inner)
    print("%s (1a) ddp_user_rollout_fit per call (%d calls per window): %s" % (what, a.inner, spread(t1)), flush=True)
    print("%s (1b) car_table on ddp_user_rollout per call: %s" % (what, spread(t2)), flush=True)
    print("%s (1) %s" % (what, verdict(t1, t2)), flush=True)

    # ---- whole solves
    o = _lib.ILQGKLOpts()
    L.ddp_ilqgkl_default_opts(C.byref(o))
    o.kl_step, o.max_iter = 0.5, 20
    res = [[h.malloc(8 * s) for s in (n * T, m * T, m * n * T, m * m * T, m * m * T, n * T, n * n * T, (N + 1) * B, 2 * B, 12 * B)] for _ in range(2)]
    its = [C.c_int(0), C.c_int(0)]

    def kl_fit():
        _lib.check(L.ddp_user_ilqgkl_fit_f64_dev(h.raw, upf, N, B, dev["prm"], 1, C.byref(o), dev["x"], dev["c0"], dev["K"], dev["u"], dev["Sp"],
                                                 dev["Sip"], None, 1, dev["R1"], dev["lims"], None, dev["fx"], dev["fu"], dev["fc"], *res[0],
                                                 C.byref(its[0])))

    def kl_tab():
        _lib.check(L.ddp_user_ilqgkl_f64_dev(h.raw, upt, N, B, dev["PT"], 1, C.byref(o), dev["x"], dev["c0"], dev["K"], dev["u"], dev["Sp"],
                                             dev["Sip"], None, 1, dev["R1"], dev["lims"], None, *res[1], C.byref(its[1])))

    kl_fit(); kl_tab(); h.sync()
    ua, ub = h.to_host(res[0][1], (m, N, B)), h.to_host(res[1][1], (m, N, B))
    sa = h.to_host(res[0][9], (12, B))
    print("%s: iLQGkl(fitted) vs iLQGkl on car_table: %d and %d batch iterations, statuses %s, controls differ by %.3g (relative, max)"
          % (what, its[0].value, its[1].value, dict(zip(*[v.tolist() for v in np.unique(sa[0].astype(int), return_counts=True)])),
             float(np.abs(ua - ub).max() / np.abs(ub).max())), flush=True)
    t1, t2 = windows(b, a, kl_fit, kl_tab, a.inner_kl)
    print("%s (2a) ddp_user_ilqgkl_fit per solve (%d solves per window): %s" % (what, a.inner_kl, spread(t1)), flush=True)
    print("%s (2b) ddp_user_ilqgkl on car_table per solve: %s" % (what, spread(t2)), flush=True)
    print("%s (2) %s" % (what, verdict(t1, t2)), flush=True)


def big(b, a):
    ddp, _lib, L, h = b.ddp, b._lib, b.L, b.h
    n, m, N, B = 32, 8, a.N, a.B2
    rng = np.random.default_rng(12)
    fx = np.eye(n)[:, :, None, None] + 0.02 * rng.standard_normal((n, n, N, B))
    fu = 0.05 * rng.standard_normal((n, m, N, B)); fc = 0.01 * rng.standard_normal((n, N, B))
    prm = np.concatenate([np.zeros(n * n + n * m), np.eye(n).ravel(), np.eye(m).ravel()])
    lq = ddp.DeviceProblem(ddp.example_source("lq"), n, m, nparam=2 * n * n + n * m + m * m, const_hessian=True, fitted=True)
    x0, u, x = rng.standard_normal((n, B)), 0.3 * rng.standard_normal((m, N, B)), rng.standard_normal((n, N, B))
    K, k = 0.05 * rng.standard_normal((m, n, N, B)), 0.1 * rng.standard_normal((m, N, B))
    T = N * B
    d = [h.to_device(np.asfortranarray(v)) for v in (prm, K, k, x0, u, x, fx, fu, fc)]
    out = [h.malloc(8 * n * T), h.malloc(8 * m * T), h.malloc(8 * N * B), h.malloc(8 * B)]
    one = np.array([1.0])
    up = lq._ptr(h)

    def roll():
        _lib.check(L.ddp_user_rollout_fit_f64_dev(h.raw, up, N, B, d[0], 0, d[1], d[2], d[3], d[4], d[5], one.ctypes.data_as(C.c_void_p), 1, None,
                                                  None, d[6], d[7], d[8], *out))

    roll(); h.sync()
    ts = [b.timed(lambda: [roll() for _ in range(a.inner)]) / a.inner for _ in range(a.repeats)]
    gb = 8.0 * T * ((n * n + n * m + n) * (N - 1) / N + 2 * m + m * n + n + n + m + 1) / 1e9     # tables (N-1 steps), u x k K in, x u c out
    med = float(np.median(ts)) * 1e-3
    print("lq n=32 m=8 N=%d B=%d, designed tables: ddp_user_rollout_fit per call (%d calls per window): %s; %.4f GB algorithmic -> %.0f GB/s, "
          "%.2f%% of the 8 TB/s roofline (no emulation exists: nparam would be %d > 4096)"
          % (N, B, a.inner, spread(ts), gb, gb / med, 100 * gb / med / 8000.0, 2 * n * n + n * m + m * m + (n * n + n * m + n) * N), flush=True)


def gps(b, a):
    """three guided-policy-search rounds on the gain-mismatched plant: the noise-free plant cost of the policy after each round"""
    ddp = b.ddp
    kl = ddp.kl
    B, N, n, m = a.gps_B, a.N, 4, 2
    for fitted in (True, False):
        car, prm, x0, u, traj, _ = setup(ddp, B, N, seed=21, S=2)
        x = ddp.forward_pass(ddp.GaussianPolicy(), x0, u, None, 1.0, car, LIMS, params=prm)[0]
        quiet = lambda t: ddp.GaussianPolicy(N, n, m, t.K, t.k, None, None)                    # noqa: E731
        costs = [float(ddp.sample_policy(car, quiet(traj), x0, x, u, 1, lims=LIMS, plant=True, params=prm)[3]["csum"].mean())]
        for it in range(3):
            xs, us, cs, _ = ddp.sample_policy(car, traj, x0, x, u, 64, seed=100 + it, lims=LIMS, plant=True, params=prm)
            fx, fu, fc, _, st = ddp.fit_dynamics(xs, us, ridge=RIDGE)
            assert not np.any(st)
            if fitted:
                xm, _, c = ddp.forward_pass(None, x0, u, None, 1.0, car, LIMS, params=prm, model=(fx, fu, fc))
                out = kl.iLQGkl(car, xm, traj, kl.Model(fx, fu, 1e-3 * np.eye(n), fc), cost=c, kl_step=0.5, lims=LIMS, params=prm, fitted=True,
                                max_iter=20)
            else:
                xm, _, c = ddp.forward_pass(None, x0, u, None, 1.0, car, LIMS, params=prm)
                out = kl.iLQGkl(car, xm, traj, kl.Model(fx, fu, 1e-3 * np.eye(n)), cost=c, kl_step=0.5, lims=LIMS, params=prm, max_iter=20)
            x, u, traj = out[0], out[1], out[2]
            costs.append(float(ddp.sample_policy(car, quiet(traj), x0, x, u, 1, lims=LIMS, plant=True, params=prm)[3]["csum"].mean()))
        print("(4) information: car_plant B=%d N=%d, noise-free cost on the plant (mean over the trajectories) before and after each of three "
              "GPS rounds, fitted=%s: %s" % (B, N, fitted, " ".join("%.4f" % c for c in costs)), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=1024)
    ap.add_argument("--N", type=int, default=50)
    ap.add_argument("--B2", type=int, default=128)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--inner", type=int, default=200)
    ap.add_argument("--inner-kl", type=int, default=3, dest="inner_kl")
    ap.add_argument("--gps-B", type=int, default=64, dest="gps_B")
    a = ap.parse_args()
    if a.repeats < 3:
        raise SystemExit("--repeats: three runs at least (the spread is part of the result)")
    b = Bench()
    import ddp_amd.kl  # noqa: F401
    pair_car(b, a)
    big(b, a)
    gps(b, a)


if __name__ == "__main__":
    main()
