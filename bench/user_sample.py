"""DDP_USER_SAMPLE: S noisy closed-loop rollouts of each of B linear-Gaussian policies of user_examples/car_plant.hip (N = 50), on the
model's dynamics so that both paths compute the same thing.
  (A) sample_policy(seed=...): ddp_policy_factor + ddp_user_sample, the noise generated inside the kernel;
  (B) the emulation that was the only way before the flag: NumPy noise, u + L ξ on the host, forward_pass at batch S·B with K, x, x0
      and the parameters tiled S times.  (B) runs code this flag does not touch, so on one build its time is that of the commit before.
Each path twice: host to host (a host clock around the Python call, which ends in a stream synchronisation; for (B) the noise, the
Cholesky factors, u + L ξ and the tiling are part of the call) and the device alone (the `_dev` entry on arrays uploaded beforehand, HIP
events on the handle's stream, `--inner` calls per timed window).  The runs of (A) and (B) alternate; every figure is given per run.
One line per measurement (append to profiles/user_sample.txt).

    python bench/user_sample.py [--B 1024] [--S 64] [--N 50] [--repeats 5] [--inner 200]
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


def spread(ts):
    med = float(np.median(ts))
    return "ms %s, median %.3f, spread %.1f%%" % (" ".join("%.3f" % t for t in ts), med, 100 * (max(ts) - min(ts)) / med)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=1024)
    ap.add_argument("--S", type=int, default=64)
    ap.add_argument("--N", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--inner", type=int, default=200)
    a = ap.parse_args()
    if a.repeats < 3:
        raise SystemExit("--repeats: three runs at least (the spread is part of the result)")
    b = Bench()
    ddp, _lib, L, h = b.ddp, b._lib, b.L, b.h
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
    x = ddp.forward_pass(ddp.GaussianPolicy(), x0, u, None, 1.0, car, lims, params=prm)[0]         # the nominal the policy acts around
    pol = ddp.GaussianPolicy(N, n, m, K, np.zeros((m, N, B)), Sigma, np.zeros((0, 0, 0)))
    seed = 20240611

    def tiled(arr):
        return np.repeat(arr[..., None, :], S, axis=-2).reshape(arr.shape[:-1] + (S * B,), order="F")

    def emulate(xi):
        """(B) on the host: u + L ξ and the tiled operands at batch S·B"""
        Lf = np.linalg.cholesky(np.moveaxis(Sigma, (0, 1), (-2, -1)))                              # [N, B, m, m]
        up = u[:, :, None, :] + np.einsum("nbij,jnsb->insb", Lf, xi)
        return (ddp.GaussianPolicy(N, n, m, tiled(K), np.zeros((m, N, S * B)), np.zeros((0, 0, 0)), np.zeros((0, 0, 0))), tiled(x0),
                up.reshape((m, N, S * B), order="F"), tiled(x), tiled(prm))

    def path_a():
        return ddp.sample_policy(car, pol, x0, x, u, S, seed=seed, lims=lims, params=prm)

    def path_b():
        xi = np.random.default_rng(seed).standard_normal((m, N, S, B))
        polt, x0t, upt, xt, prmt = emulate(xi)
        return ddp.forward_pass(polt, x0t, upt, xt, 1.0, car, lims, params=prmt)

    # ---- the two paths compute the same thing: (B) on the noise (A) draws
    xa = path_a()[0]
    kernel = h.last_kernel(1)
    polt, x0t, upt, xt, prmt = emulate(ddp.normal(seed, m, N, S, B))
    xb = ddp.forward_pass(polt, x0t, upt, xt, 1.0, car, lims, params=prmt)[0]
    err = float(np.abs(xa.reshape(xb.shape, order="F") - xb).max() / np.abs(xb).max())
    print("B=%d S=%d N=%d car_plant (model dynamics): sample_policy vs the emulation on the same noise: states differ by %.3g "
          "(relative, max); kernel %s" % (B, S, N, err, kernel), flush=True)

    # ---- host to host, alternating
    path_b()
    ta, tb = [], []
    for _ in range(a.repeats):
        t = time.perf_counter(); path_a(); ta.append(1e3 * (time.perf_counter() - t))
        t = time.perf_counter(); path_b(); tb.append(1e3 * (time.perf_counter() - t))
    print("host to host, (A) sample_policy(seed): %s" % spread(ta), flush=True)
    print("host to host, (B) NumPy noise + tiling + forward_pass at batch S*B: %s" % spread(tb), flush=True)

    # ---- the device alone
    T, R = N * B, S * B
    dprm, dK, dSg, dx0, du, dx, dl = (h.to_device(v) for v in (prm, K, Sigma, x0, u, x, lims.flatten(order="F")))
    oxs, ous, ocs, ocsum, ost = h.malloc(8 * n * N * R), h.malloc(8 * m * N * R), h.malloc(8 * (N + 1) * R), h.malloc(8 * R), h.malloc(4 * B)
    upa = car._ptr(h)
    lo, hi = ddp._seed_words(seed)
    one = np.ones(1)

    def dev_a():
        for _ in range(a.inner):
            _lib.check(L.ddp_user_sample_f64_dev(h.raw, upa, N, B, S, dprm, 1, dK, dSg, dx0, du, dx, dl, None, lo, hi, 0, 0, 0, oxs, ous, ocs,
                                                 ocsum, None, None, ost))
    dKt, dkt, dx0t, dupt, dxt, dprmt = (h.to_device(v) for v in (polt.K, polt.k, x0t, upt, xt, prmt))

    def dev_b():
        for _ in range(a.inner):
            _lib.check(L.ddp_user_forward_pass_f64_dev(h.raw, upa, N, R, dprmt, 1, dKt, dkt, dx0t, dupt, dxt, one.ctypes.data_as(C.c_void_p), 1,
                                                       dl, None, oxs, ous, ocs, ocsum))
    dev_a(); dev_b()
    da, db = [], []
    for _ in range(a.repeats):
        da.append(b.timed(dev_a) / a.inner)
        db.append(b.timed(dev_b) / a.inner)
    gb_a = 8.0 * (n + m + 1) * N * R / 1e9
    gb_b = gb_a + 8.0 * (m * n + 2 * m + n) * N * R / 1e9
    print("device alone per call (%d calls per window), (A) ddp_policy_factor + ddp_user_sample: %s; %.3f GB of results -> %.0f GB/s"
          % (a.inner, spread(da), gb_a, gb_a / (float(np.median(da)) * 1e-3)), flush=True)
    print("device alone per call (%d calls per window), (B) ddp_user_rollout at batch S*B on uploaded, tiled operands: %s; %.3f GB of operands "
          "and results -> %.0f GB/s" % (a.inner, spread(db), gb_b, gb_b / (float(np.median(db)) * 1e-3)), flush=True)
    print("(A) over (B): host to host %.2fx the speed, device alone %.2fx the speed (medians; (B) ran on this same build)"
          % (float(np.median(tb)) / float(np.median(ta)), float(np.median(db)) / float(np.median(da))), flush=True)


if __name__ == "__main__":
    main()
