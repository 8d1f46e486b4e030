"""fit_cost: the quadratic cost model of a guided-policy-search round fitted to the S noisy closed-loop rollouts of each of B policies,
the step next to fit_dynamics.  Two shapes: user_examples/car_plant.hip on its plant (N = 50), and lq (32, 8) with constant Hessians
around the rollouts of a drawn stable linear system.  On the same samples, alternating inside one process, every figure per window:
  (1) ddp_user_cost_fit_f64_dev on arrays that are on the device (HIP events, `--inner` calls per window, and one call under a host
      clock with its synchronisation, the clock of (2));
  (2) the emulation a user has without the entry: ddp_user_df_f64_dev and ddp_user_costfun_f64_dev at batch S·B, then the shift to the
      nominal and the mean over the samples in torch on the device (einsum on the arrays the kernels wrote, no copy; a host clock around
      the two launches, the synchronisation, the torch operations and torch's synchronisation).  Without torch: the two launches alone;
  (3) fit_cost host to host, and (car shape) df + costfun host to host with the reduction in NumPy.
Then, information only: three guided-policy-search rounds on the gain-mismatched plant with and without cost_model=.
One line per measurement (append to profiles/user_cost_fit.txt).

    python bench/user_cost_fit.py [--B 1024] [--S 64] [--N 50] [--B2 128] [--S2 128] [--repeats 5] [--inner 20] [--gps-B 64]
"""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from user_clock import Bench, car_plant_params       # noqa: E402
from user_fit import get_torch                       # noqa: E402
from user_fitted import LIMS, RIDGE, setup           # noqa: E402
from user_sample import spread                       # noqa: E402


def reduce_numpy(c, cx, cu, cxx, cxu, cuu, xs, us, x, u):
    """the six formulas on per-sample arrays [., N, S, B] in float64 NumPy"""
    dx, du = xs - x[:, :, None], us - u[:, :, None]
    hx = np.einsum("rjisb,jisb->risb", cxx, dx, optimize=True) + np.einsum("rqisb,qisb->risb", cxu, du, optimize=True)
    hu = np.einsum("jqisb,jisb->qisb", cxu, dx, optimize=True) + np.einsum("qpisb,pisb->qisb", cuu, du, optimize=True)
    c0 = c - (cx * dx).sum(0) - (cu * du).sum(0) + 0.5 * ((dx * hx).sum(0) + (du * hu).sum(0))
    return (cx - hx).mean(2), (cu - hu).mean(2), cxx.mean(3), cxu.mean(3), cuu.mean(3), c0.mean(1)


def reduce_torch(torch, t, N, S, B, n, m, const_h, terminal):
    """the same on the device tensors of the emulation (row-major views of the column-major arrays: the axes are reversed)"""
    dx, du = t["xs"] - t["x"][:, None], t["us"] - t["u"][:, None]                    # [B, S, N, n], [B, S, N, m]
    cxx, cxu, cuu = t["cxx"], t["cxu"], t["cuu"]                                      # [B, S, (N,) col, row]
    if const_h:
        cxx, cxu, cuu = (a[:, :, None] for a in (cxx, cxu, cuu))
    hx = torch.einsum("bsijr,bsij->bsir", cxx.expand(B, S, N, n, n), dx) + torch.einsum("bsiqr,bsiq->bsir", cxu.expand(B, S, N, m, n), du)
    hu = torch.einsum("bsiqr,bsir->bsiq", cxu.expand(B, S, N, m, n), dx) + torch.einsum("bsipq,bsip->bsiq", cuu.expand(B, S, N, m, m), du)
    c = t["cost"][:, :, :N]
    if terminal:
        c = c.clone()
        c[:, :, N - 1] += t["cost"][:, :, N]
    c0 = c - (t["cx"] * dx).sum(-1) - (t["cu"] * du).sum(-1) + 0.5 * ((dx * hx).sum(-1) + (du * hu).sum(-1))
    return ((t["cx"] - hx).mean(1), (t["cu"] - hu).mean(1), cxx.expand(B, S, N, n, n).mean(1), cxu.expand(B, S, N, m, n).mean(1),
            cuu.expand(B, S, N, m, m).mean(1), c0.mean(1))


def measure(b, a, what, prob, prm, xs, us, x, u, torch, host_emulation):
    ddp, _lib, L, h = b.ddp, b._lib, b.L, b.h
    n, N, S, B = xs.shape
    m = us.shape[0]
    T, R, CL = N * B, S * B, prob.cost_len(N)
    const_h, up = prob.const_hessian, prob._ptr(h)
    hN = 1 if const_h else N
    vp = lambda p: C.c_void_p(p)                                                      # noqa: E731
    prm_sb = np.asfortranarray(np.repeat(prm, S, axis=1))                             # column s + S b: the parameters of trajectory b
    dprm, dprm_sb, dx, du = (h.to_device(np.asfortranarray(v)) for v in (prm, prm_sb, x, u))
    shapes = [(n, N, B), (m, N, B), (n, n, N, B), (n, m, N, B), (m, m, N, B), (N, B)]
    outs = [h.malloc(8 * int(np.prod(s))) for s in shapes]
    sizes = dict(fx=n * n * N * R, fu=n * m * N * R, cx=n * N * R, cu=m * N * R, cxx=n * n * hN * R, cxu=n * m * hN * R, cuu=m * m * hN * R,
                 cost=CL * R, csum=R)
    if torch is not None:                                  # the emulation's arrays are torch's, so that its reduction reads them in place
        t = {k: torch.empty(v, dtype=torch.float64, device="cuda") for k, v in sizes.items()}
        t["xs"], t["us"] = torch.from_numpy(xs.T.copy()).cuda(), torch.from_numpy(us.T.copy()).cuda()       # [B, S, N, n]: the memory of xs[n,N,S,B]
        t["x"], t["u"] = torch.from_numpy(x.T.copy()).cuda(), torch.from_numpy(u.T.copy()).cuda()
        torch.cuda.synchronize()
        ptr = {k: vp(v.data_ptr()) for k, v in t.items()}
        dxs, dus = ptr["xs"], ptr["us"]
        hsh = (R,) + (() if const_h else (N,))
        for k, s in (("cx", (R, N, n)), ("cu", (R, N, m)), ("cxx", hsh + (n, n)), ("cxu", hsh + (m, n)), ("cuu", hsh + (m, m)), ("cost", (R, CL))):
            t[k] = t[k].view((B, S) + s[1:])
    else:
        ptr = {k: h.malloc(8 * v) for k, v in sizes.items()}
        dxs, dus = h.to_device(xs), h.to_device(us)

    def fused():
        _lib.check(L.ddp_user_cost_fit_f64_dev(h.raw, up, N, S, B, dprm, 1, dxs, dus, dx, du, *outs))

    def launches():
        _lib.check(L.ddp_user_df_f64_dev(h.raw, up, N, R, dprm_sb, 1, dxs, dus, None, ptr["fx"], ptr["fu"], ptr["cx"], ptr["cu"], ptr["cxx"],
                                         ptr["cxu"], ptr["cuu"]))
        _lib.check(L.ddp_user_costfun_f64_dev(h.raw, up, N, R, dprm_sb, 1, dxs, dus, None, ptr["cost"], ptr["csum"]))

    def emulation():
        launches()
        h.sync()
        if torch is None:
            return None
        r = reduce_torch(torch, t, N, S, B, n, m, const_h, prob.terminal)
        torch.cuda.synchronize()
        return r

    def host():
        return ddp.fit_cost(prob, xs, us, x, u, params=prm)

    # ---- the paths agree on the same samples
    fused(); h.sync()
    dev = [h.to_host(p, s) for p, s in zip(outs, shapes)]
    hh = host()
    bits = all(np.array_equal(p, q) for p, q in zip(dev, hh))
    rel = lambda p, q: float(np.abs(p - q).max() / max(np.abs(q).max(), 1e-300))      # noqa: E731
    line = "%s: (1) and (3) %s" % (what, "agree bit for bit" if bits else "DIFFER")
    r = emulation()
    if r is not None:
        line += "; (1) vs the torch emulation, relative, max: " + ", ".join(
            "%s %.2g" % (k, rel(p, q.cpu().numpy().T)) for k, p, q in zip(("cx", "cu", "cxx", "cxu", "cuu", "c0"), dev, r))
    print(line, flush=True)

    # ---- five windows each, alternating
    t1, t1h, t2, t3 = [], [], [], []
    for _ in range(a.repeats):
        t1.append(b.timed(lambda: [fused() for _ in range(a.inner)]) / a.inner)
        h.sync(); tt = time.perf_counter(); fused(); h.sync(); t1h.append(1e3 * (time.perf_counter() - tt))
        tt = time.perf_counter(); emulation(); t2.append(1e3 * (time.perf_counter() - tt))
        tt = time.perf_counter(); host(); t3.append(1e3 * (time.perf_counter() - tt))
    gb_in = 8.0 * (n + m) * N * R / 1e9
    gb_emu = 8.0 * (sum(sizes.values()) + (n + m) * N * R) / 1e9
    print("%s (1) ddp_user_cost_fit, device alone per call (%d calls per window): %s; %.3f GB of samples -> %.0f GB/s"
          % (what, a.inner, spread(t1), gb_in, gb_in / (float(np.median(t1)) * 1e-3)), flush=True)
    print("%s (1) ddp_user_cost_fit, one call and its synchronisation under the host clock: %s" % (what, spread(t1h)), flush=True)
    print("%s (2) emulation, ddp_user_df + ddp_user_cost at batch S·B = %d%s (%.2f GB written and read back): %s"
          % (what, R, ", shift and mean in torch on the device" if torch is not None else " ALONE (torch not available: no reduction)", gb_emu,
             spread(t2)), flush=True)
    m1, m2 = float(np.median(t1h)), float(np.median(t2))
    s1, s2 = (max(t1h) - min(t1h)) / m1, (max(t2) - min(t2)) / m2
    print("%s: (2) over (1) %.2fx the time (medians, both under the host clock); the two spreads %.1f%% + %.1f%%: the fused kernel is %s"
          % (what, m2 / m1, 100 * s1, 100 * s2, "faster beyond the spreads" if m1 * (1 + s1 + s2) < m2 else "NOT faster beyond the spreads"),
          flush=True)
    print("%s (3) fit_cost host to host: %s" % (what, spread(t3)), flush=True)
    if host_emulation:
        t4 = []
        for _ in range(3):
            tt = time.perf_counter()
            X, U = np.asfortranarray(xs.reshape(n, N, R, order="F")), np.asfortranarray(us.reshape(m, N, R, order="F"))
            d = ddp.df(prob, X, U, params=prm_sb)[5:]
            cost = ddp.costfun(prob, X, U, params=prm_sb)
            c = cost[:N].copy()
            if prob.terminal:
                c[N - 1] += cost[N]
            rn = reduce_numpy(*(v.reshape(v.shape[:-1] + (S, B), order="F") for v in (c,) + tuple(d)), xs, us, x, u)
            t4.append(1e3 * (time.perf_counter() - tt))
        print("%s (3) emulation host to host (df, costfun, NumPy einsum): %s; against (1) %.2g (cx, relative, max)"
              % (what, spread(t4), rel(rn[0], dev[0])), flush=True)
    for p in outs + [dprm, dprm_sb, dx, du]:
        h.free(p)
    if torch is None:
        for p in list(ptr.values()) + [dxs, dus]:
            h.free(p)
    else:
        del t, r
        torch.cuda.empty_cache()


def gps(b, a):
    """three guided-policy-search rounds on the gain-mismatched plant, planning on the fitted dynamics: the noise-free plant cost of the
    policy after each round, with the cost linearised at the nominal and with the cost model fitted to the samples"""
    ddp = b.ddp
    kl = ddp.kl
    B, N, n, m = a.gps_B, a.N, 4, 2
    for use_model in (True, False):
        _, prm, x0, u, traj, _ = setup(ddp, B, N, seed=21, S=2)
        car = ddp.DeviceProblem(ddp.example_source("car_plant"), n, m, nparam=13, terminal=True, plant=True, sample=True, fitted=True, cost_fit=True)
        x = ddp.forward_pass(ddp.GaussianPolicy(), x0, u, None, 1.0, car, LIMS, params=prm)[0]
        quiet = lambda t: ddp.GaussianPolicy(N, n, m, t.K, t.k, None, None)                    # noqa: E731
        costs = [float(ddp.sample_policy(car, quiet(traj), x0, x, u, 1, lims=LIMS, plant=True, params=prm)[3]["csum"].mean())]
        for it in range(3):
            xs, us, cs, _ = ddp.sample_policy(car, traj, x0, x, u, 64, seed=100 + it, lims=LIMS, plant=True, params=prm)
            fx, fu, fc, _, st = ddp.fit_dynamics(xs, us, ridge=RIDGE)
            assert not np.any(st)
            xm, _, c = ddp.forward_pass(None, x0, u, None, 1.0, car, LIMS, params=prm, model=(fx, fu, fc))
            cm = ddp.fit_cost(car, xs, us, np.asfortranarray(xm.reshape(n, N, B)), u, params=prm)[:5] if use_model else None
            out = kl.iLQGkl(car, xm, traj, kl.Model(fx, fu, 1e-3 * np.eye(n), fc), cost=c, kl_step=0.5, lims=LIMS, params=prm, fitted=True,
                            max_iter=20, cost_model=cm)
            x, u, traj = out[0], out[1], out[2]
            costs.append(float(ddp.sample_policy(car, quiet(traj), x0, x, u, 1, lims=LIMS, plant=True, params=prm)[3]["csum"].mean()))
        print("information: car_plant B=%d N=%d, noise-free cost on the plant (mean over the trajectories) before and after each of three GPS "
              "rounds, fitted=True, cost_model=%s: %s" % (B, N, "fit_cost(...)" if use_model else "None", " ".join("%.4f" % c for c in costs)),
              flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=1024)
    ap.add_argument("--S", type=int, default=64)
    ap.add_argument("--N", type=int, default=50)
    ap.add_argument("--B2", type=int, default=128)
    ap.add_argument("--S2", type=int, default=128)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--gps-B", type=int, default=64, dest="gps_B")
    a = ap.parse_args()
    if a.repeats < 3:
        raise SystemExit("--repeats: three runs at least (the spread is part of the result)")
    torch = get_torch()
    if torch is not None:
        torch.zeros(1, device="cuda")                       # torch's runtime first (the library then shares it)
    b = Bench()
    ddp, h = b.ddp, b.h
    import ddp_amd.kl  # noqa: F401

    # ---- car_plant: the sampler's bench shape, on the plant
    B, S, N, n, m = a.B, a.S, a.N, 4, 2
    rng = np.random.default_rng(11)
    prm = car_plant_params(rng, B)
    x0 = np.zeros((n, B)); x0[:2] = rng.uniform(0, 0.5, (2, B)); x0[2] = np.pi / 4 + rng.uniform(-0.2, 0.2, B); x0[3] = 1.0
    u = np.asfortranarray(0.1 * rng.standard_normal((m, N, B)))
    K = -0.4 * rng.random((m, n, N, B))
    G = rng.standard_normal((m, m, N, B))
    Sigma = 0.04 * (np.einsum("ikjb,lkjb->iljb", G, G) / m + 0.5 * np.eye(m)[:, :, None, None])
    car = ddp.DeviceProblem(ddp.example_source("car_plant"), n, m, nparam=13, terminal=True, plant=True, sample=True, cost_fit=True)
    x = np.asfortranarray(ddp.forward_pass(ddp.GaussianPolicy(), x0, u, None, 1.0, car, LIMS, params=prm)[0].reshape(n, N, B))
    xs, us, _, info = ddp.sample_policy(car, ddp.GaussianPolicy(N, n, m, K, u, Sigma, Sigma), x0, x, u, S, seed=20240611, lims=LIMS, plant=True,
                                        params=prm)
    assert not np.any(info["status"])
    measure(b, a, "car_plant on its plant B=%d S=%d N=%d" % (B, S, N), car, prm, xs, us, x, u, torch, True)

    # ---- lq (32, 8), constant Hessians: samples around the rollouts of a drawn stable linear system
    B, S, n, m = a.B2, a.S2, 32, 8
    rng = np.random.default_rng(12)
    xs, us = np.zeros((n, N, S, B), order="F"), np.zeros((m, N, S, B), order="F")
    Am = 0.8 * np.eye(n) + 0.2 / np.sqrt(n) * rng.standard_normal((B, n, n))
    Bm = rng.standard_normal((B, n, m)) / np.sqrt(n)
    xh = rng.standard_normal((B, n, 1)) + 0.3 * rng.standard_normal((B, n, S))
    for i in range(N):
        uh = 0.5 * rng.standard_normal((B, m, S))
        xs[:, i], us[:, i] = np.moveaxis(xh, 0, -1), np.moveaxis(uh, 0, -1)
        xh = Am @ xh + Bm @ uh + 0.05 * rng.standard_normal((B, n, S))
    x, u = np.asfortranarray(xs.mean(axis=2)), np.asfortranarray(us.mean(axis=2))
    spd = lambda d: (lambda q: q @ q.T / d + 0.5 * np.eye(d))(rng.standard_normal((d, d)))       # noqa: E731
    prm = np.asfortranarray(np.stack([np.concatenate([Am[j].ravel(order="F"), Bm[j].ravel(order="F"), spd(n).ravel(order="F"),
                                                      spd(m).ravel(order="F")]) for j in range(B)], -1))
    lq = ddp.DeviceProblem(ddp.example_source("lq"), n, m, nparam=2 * n * n + n * m + m * m, const_hessian=True, cost_fit=True)
    measure(b, a, "lq n=32 m=8 const_hessian B=%d S=%d N=%d" % (B, S, N), lq, prm, xs, us, x, u, torch, False)
    gps(b, a)


if __name__ == "__main__":
    main()
