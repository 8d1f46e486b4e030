"""fit_dynamics: time-varying linear-Gaussian dynamics fitted to the S noisy closed-loop rollouts of each of B policies of
user_examples/car_plant.hip on its plant (N = 50), the step between sample_policy and iLQGkl.  Four paths on the same samples:
  (1) ddp_fit_dynamics_f64_dev on the arrays ddp_user_sample_f64_dev left on the device (HIP events, `--inner` calls per window);
  (2) fit_dynamics host to host (a host clock around the Python call, which ends in a stream synchronisation);
  (3) the same formula in NumPy on the downloaded arrays (einsum + np.linalg.solve): what a user does without the entry;
  (4) the same formula in torch on the GPU (einsum, torch.linalg.cholesky, cholesky_solve) on tensors that are on the device already,
      if torch imports and sees the device: the device comparator of (1).
The paths alternate inside one process; every figure is given per window.  Then one more shape, (n, m) = (32, 8), S = 128, on the
rollouts of a drawn stable linear system (the many-tile case).  One line per measurement (append to profiles/user_fit.txt).

    python bench/user_fit.py [--B 1024] [--S 64] [--N 50] [--B2 128] [--S2 128] [--repeats 5] [--inner 50]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from user_clock import Bench, car_plant_params       # noqa: E402
from user_sample import spread                       # noqa: E402

RIDGE = 1e-3                                         # the ridge of the sampler case of tests/fit_reference.py


def fit_numpy(xs, us, ridge):
    """the formula of include/ddp_amd.h in float64 NumPy, all steps and trajectories at once"""
    n, N, S, B = xs.shape
    d = n + us.shape[0]
    W = np.concatenate([xs[:, :-1], us[:, :-1], xs[:, 1:]], axis=0)                  # [p, N-1, S, B]
    mu = W.mean(axis=2)
    Wc = W - mu[:, :, None, :]
    Cm = np.einsum("pisb,qisb->ibpq", Wc, Wc, optimize=True) / (S - 1)
    A = Cm[..., :d, :d] + ridge * np.eye(d)
    F = np.swapaxes(np.linalg.solve(A, Cm[..., :d, d:]), -1, -2)                     # [N-1, B, n, d]
    mut = np.moveaxis(mu, 0, -1)                                                     # [N-1, B, p]
    fc = mut[..., d:] - np.einsum("ibnd,ibd->ibn", F, mut[..., :d])
    M = Cm[..., d:, d:] - F @ Cm[..., :d, d:]
    return F, fc, (M + np.swapaxes(M, -1, -2)) / 2


def fit_torch(torch, xt, ut, ridge):
    """the same on device tensors xt[B,S,N,n], ut[B,S,N,m] (the memory of xs[n,N,S,B], us[m,N,S,B])"""
    S, n = xt.shape[1], xt.shape[3]
    d = n + ut.shape[3]
    W = torch.cat([xt[:, :, :-1], ut[:, :, :-1], xt[:, :, 1:]], dim=-1)               # [B, S, N-1, p]
    mu = W.mean(dim=1)
    Wc = W - mu[:, None]
    Cm = torch.einsum("bsip,bsiq->bipq", Wc, Wc) / (S - 1)
    A = Cm[..., :d, :d] + ridge * torch.eye(d, dtype=W.dtype, device=W.device)
    F = torch.cholesky_solve(Cm[..., :d, d:], torch.linalg.cholesky(A)).transpose(-1, -2)      # [B, N-1, n, d]
    fc = mu[..., d:] - torch.einsum("bind,bid->bin", F, mu[..., :d])
    M = Cm[..., d:, d:] - F @ Cm[..., :d, d:]
    return F, fc, (M + M.transpose(-1, -2)) / 2


def get_torch():
    try:
        import torch
        return torch if torch.cuda.is_available() else None
    except Exception:
        return None


def measure(b, a, what, n, m, N, S, B, dxs, dus, xs, us, torch):
    ddp, _lib, L, h = b.ddp, b._lib, b.L, b.h
    T = N * B
    outs = [h.malloc(8 * n * n * T), h.malloc(8 * n * m * T), h.malloc(8 * n * T), h.malloc(8 * n * n * T), h.malloc(4 * T)]

    def dev():
        for _ in range(a.inner):
            _lib.check(L.ddp_fit_dynamics_f64_dev(h.raw, n, m, N, S, B, dxs, dus, RIDGE, None, None, 0.0, 0.0, 0, *outs))

    def host():
        return ddp.fit_dynamics(xs, us, ridge=RIDGE)

    if torch is not None:
        xt, ut = torch.from_numpy(xs.T).cuda(), torch.from_numpy(us.T).cuda()

        def tor():
            r = fit_torch(torch, xt, ut, RIDGE)
            torch.cuda.synchronize()
            return r

    # ---- the paths agree on the same samples
    dev(); h.sync()
    fxd = h.to_host(outs[0], (n, n, N, B)); fud = h.to_host(outs[1], (n, m, N, B)); covd = h.to_host(outs[3], (n, n, N, B))
    sth = h.to_host(outs[4], (N, B), dtype=np.int32)
    fx, fu, fc, cov, st = host()
    bits = all(np.array_equal(p, q, equal_nan=True) for p, q in ((fxd, fx), (fud, fu), (covd, cov), (sth, st)))
    Fn, fcn, covn = fit_numpy(xs, us, RIDGE)
    Fk = np.moveaxis(np.concatenate([fx, fu], axis=1)[:, :, :-1], (0, 1), (2, 3))   # [N-1, B, n, d]
    rel = lambda p, q: float(np.abs(p - q).max() / np.abs(q).max())                  # noqa: E731
    line = "%s: failed steps %d of %d; (1) and (2) %s; [fx fu] of (2) vs NumPy %.3g, cov %.3g (relative, max)" % (
        what, int(np.count_nonzero(st)), (N - 1) * B, "agree bit for bit" if bits else "DIFFER", rel(Fk, Fn),
        rel(np.moveaxis(cov[:, :, :-1], (0, 1), (2, 3)), covn))
    if torch is not None:
        Ft, fct, covt = (v.cpu().numpy() for v in tor())
        line += "; vs torch %.3g, cov %.3g" % (rel(np.moveaxis(Fk, 0, 1), Ft), rel(np.moveaxis(cov[:, :, :-1], (0, 1, 2, 3), (2, 3, 1, 0)), covt))
    print(line, flush=True)

    # ---- five windows each, alternating
    t1, t2, t3, t4 = [], [], [], []
    for _ in range(a.repeats):
        t1.append(b.timed(dev) / a.inner)
        t = time.perf_counter(); host(); t2.append(1e3 * (time.perf_counter() - t))
        t = time.perf_counter(); fit_numpy(xs, us, RIDGE); t3.append(1e3 * (time.perf_counter() - t))
        if torch is not None:
            torch.cuda.synchronize()
            t = time.perf_counter(); tor(); t4.append(1e3 * (time.perf_counter() - t))
    gb = 8.0 * (n + m) * N * S * B / 1e9
    print("%s (1) device alone per call (%d calls per window), ddp_fit_dynamics: %s; %.3f GB of samples -> %.0f GB/s"
          % (what, a.inner, spread(t1), gb, gb / (float(np.median(t1)) * 1e-3)), flush=True)
    print("%s (2) host to host, fit_dynamics: %s" % (what, spread(t2)), flush=True)
    print("%s (3) NumPy on the downloaded arrays (einsum + solve): %s" % (what, spread(t3)), flush=True)
    if torch is not None:
        print("%s (4) torch on the device (cat, einsum, cholesky, cholesky_solve; tensors resident, one synchronisation): %s" % (what, spread(t4)), flush=True)
        print("%s: (4) over (1) %.2fx the time; (3) over (2) %.2fx the time (medians)"
              % (what, float(np.median(t4)) / float(np.median(t1)), float(np.median(t3)) / float(np.median(t2))), flush=True)
    else:
        print("%s (4) torch: not available in this process; (3) over (2) %.2fx the time (medians)"
              % (what, float(np.median(t3)) / float(np.median(t2))), flush=True)
    for p in outs:
        h.free(p)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=1024)
    ap.add_argument("--S", type=int, default=64)
    ap.add_argument("--N", type=int, default=50)
    ap.add_argument("--B2", type=int, default=128)
    ap.add_argument("--S2", type=int, default=128)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--inner", type=int, default=50)
    a = ap.parse_args()
    if a.repeats < 3:
        raise SystemExit("--repeats: three runs at least (the spread is part of the result)")
    torch = get_torch()
    b = Bench()
    ddp, _lib, L, h = b.ddp, b._lib, b.L, b.h

    # ---- car_plant: the sampler's bench shape, on the plant
    B, S, N, n, m = a.B, a.S, a.N, 4, 2
    rng = np.random.default_rng(11)
    prm = car_plant_params(rng, B)
    x0 = np.zeros((n, B)); x0[:2] = rng.uniform(0, 0.5, (2, B)); x0[2] = np.pi / 4 + rng.uniform(-0.2, 0.2, B); x0[3] = 1.0
    u = 0.1 * rng.standard_normal((m, N, B))
    K = -0.4 * rng.random((m, n, N, B))
    G = rng.standard_normal((m, m, N, B))
    Sigma = 0.04 * (np.einsum("ikjb,lkjb->iljb", G, G) / m + 0.5 * np.eye(m)[:, :, None, None])
    lims = np.array([[-2.0, 2.0], [-1.5, 1.5]])
    car = ddp.DeviceProblem(ddp.example_source("car_plant"), n, m, nparam=13, terminal=True, plant=True, sample=True)
    x = ddp.forward_pass(ddp.GaussianPolicy(), x0, u, None, 1.0, car, lims, params=prm)[0]
    R = S * B
    dprm, dK, dSg, dx0, du, dx, dl = (h.to_device(v) for v in (prm, K, Sigma, x0, u, x, lims.flatten(order="F")))
    dxs, dus, ocs, ocsum, ost = h.malloc(8 * n * N * R), h.malloc(8 * m * N * R), h.malloc(8 * (N + 1) * R), h.malloc(8 * R), h.malloc(4 * B)
    lo, hi = ddp._seed_words(20240611)
    _lib.check(L.ddp_user_sample_f64_dev(h.raw, car._ptr(h), N, B, S, dprm, 1, dK, dSg, dx0, du, dx, dl, None, lo, hi, 0, 0, 1, dxs, dus, ocs,
                                         ocsum, None, None, ost))
    h.sync()
    xs, us = h.to_host(dxs, (n, N, S, B)), h.to_host(dus, (m, N, S, B))
    measure(b, a, "car_plant on its plant B=%d S=%d N=%d ridge=%g" % (B, S, N, RIDGE), n, m, N, S, B, dxs, dus, xs, us, torch)
    for p in (dxs, dus, ocs, ocsum, ost):
        h.free(p)

    # ---- (32, 8): the closed loop of a drawn stable linear system under control noise, B2 trajectories
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
    dxs, dus = h.to_device(xs), h.to_device(us)
    measure(b, a, "linear system n=32 m=8 B=%d S=%d N=%d ridge=%g" % (B, S, N, RIDGE), n, m, N, S, B, dxs, dus, xs, us, torch)


if __name__ == "__main__":
    main()
