"""fit_dynamics(..., wide=True): the dynamics fit at the two shapes of bench/user_sample_wave.py, (n, m) = (64, 32) at B = 64 and
(34, 17) at B = 128, N = 50, with S = 2 d samples (a fit without prior), on the closed-loop rollouts of a drawn stable linear system
under control noise (as the (32, 8) line of bench/user_fit.py).  Four paths on the same samples:
  (1) ddp_fit_dynamics_wide_f64_dev on arrays that are on the device (HIP events, `--inner` calls per window);
  (2) fit_dynamics(..., wide=True) host to host (a host clock around the Python call, which ends in a stream synchronisation);
  (3) the same formula in NumPy on the downloaded arrays (einsum + np.linalg.solve): what a user does without the entry;
  (4) the same formula in torch on the GPU (fit_torch of bench/user_fit.py) on tensors that are on the device already, if torch imports
      and sees the device: there is no earlier device path at these shapes, so this is the comparator of (1).
The paths alternate inside one process; every figure is given per window.  One line per measurement (append to
profiles/user_fit_wide.txt).

    python bench/user_fit_wide.py [--B 64] [--B2 128] [--N 50] [--repeats 5] [--inner 10]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from user_clock import Bench                         # noqa: E402
from user_sample import spread                       # noqa: E402
from user_fit import RIDGE, fit_numpy, fit_torch, get_torch      # noqa: E402


def rollouts(n, m, N, S, B, seed):
    """xs[n,N,S,B], us[m,N,S,B]: the closed loop of a drawn stable linear system per trajectory under control and process noise"""
    rng = np.random.default_rng(seed)
    xs, us = np.zeros((n, N, S, B), order="F"), np.zeros((m, N, S, B), order="F")
    Am = 0.8 * np.eye(n) + 0.2 / np.sqrt(n) * rng.standard_normal((B, n, n))
    Bm = rng.standard_normal((B, n, m)) / np.sqrt(n)
    xh = rng.standard_normal((B, n, 1)) + 0.3 * rng.standard_normal((B, n, S))
    for i in range(N):
        uh = 0.5 * rng.standard_normal((B, m, S))
        xs[:, i], us[:, i] = np.moveaxis(xh, 0, -1), np.moveaxis(uh, 0, -1)
        xh = Am @ xh + Bm @ uh + 0.05 * rng.standard_normal((B, n, S))
    return xs, us


def measure(b, a, what, n, m, N, S, B, xs, us, torch):
    ddp, _lib, L, h = b.ddp, b._lib, b.L, b.h
    T = N * B
    dxs, dus = h.to_device(xs), h.to_device(us)
    outs = [h.malloc(8 * n * n * T), h.malloc(8 * n * m * T), h.malloc(8 * n * T), h.malloc(8 * n * n * T), h.malloc(4 * T)]

    def dev():
        for _ in range(a.inner):
            _lib.check(L.ddp_fit_dynamics_wide_f64_dev(h.raw, n, m, N, S, B, dxs, dus, RIDGE, None, None, 0.0, 0.0, 0, *outs))

    def host():
        return ddp.fit_dynamics(xs, us, ridge=RIDGE, wide=True)

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
    med = float(np.median(t1))
    print("%s (1) device alone per call (%d calls per window), ddp_fit_dynamics_wide: %s; %.3f GB of samples; %.2f us per step and trajectory"
          % (what, a.inner, spread(t1), gb, 1e3 * med / ((N - 1) * B)), flush=True)
    print("%s (2) host to host, fit_dynamics(wide=True): %s" % (what, spread(t2)), flush=True)
    print("%s (3) NumPy on the downloaded arrays (einsum + solve): %s" % (what, spread(t3)), flush=True)
    if torch is not None:
        print("%s (4) torch on the device (cat, einsum, cholesky, cholesky_solve; tensors resident, one synchronisation): %s" % (what, spread(t4)), flush=True)
        print("%s: (4) over (1) %.2fx the time; (3) over (2) %.2fx the time (medians)"
              % (what, float(np.median(t4)) / med, float(np.median(t3)) / float(np.median(t2))), flush=True)
    else:
        print("%s (4) torch: not available in this process; (3) over (2) %.2fx the time (medians)"
              % (what, float(np.median(t3)) / float(np.median(t2))), flush=True)
    for p in outs + [dxs, dus]:
        h.free(p)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=64)
    ap.add_argument("--B2", type=int, default=128)
    ap.add_argument("--N", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--inner", type=int, default=10)
    a = ap.parse_args()
    if a.repeats < 3:
        raise SystemExit("--repeats: three runs at least (the spread is part of the result)")
    torch = get_torch()
    b = Bench()
    for n, m, B, seed in ((64, 32, a.B, 21), (34, 17, a.B2, 22)):
        S = 2 * (n + m)
        xs, us = rollouts(n, m, a.N, S, B, seed)
        measure(b, a, "linear system n=%d m=%d B=%d S=%d N=%d ridge=%g" % (n, m, B, S, a.N, RIDGE), n, m, a.N, S, B, xs, us, torch)


if __name__ == "__main__":
    main()
