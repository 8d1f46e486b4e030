"""DDP_USER_SAMPLE_WAVE: S noisy closed-loop rollouts of each of B linear-Gaussian policies of user_examples/chain_plant_ad.hip (N = 50)
at the shapes of DDP_USER_WAVE, (n, m) = (64, 32) and (34, 17), on the model's dynamics so that both paths compute the same thing.
  (A) sample_policy(seed=...): ddp_policy_factor_wide + ddp_user_sample_wave, the noise generated inside the kernel;
  (B) the emulation that was the only way before the flag: NumPy noise, u + L ξ on the host, forward_pass of the wave problem
      (ddp_user_rollout_wave) at batch S·B with K, x, x0 and the parameters tiled S times.  (B) runs code this flag does not touch.
Each path twice: host to host (a host clock around the Python call, which ends in a stream synchronisation; for (B) the noise, the
Cholesky factors, u + L ξ and the tiling are part of the call) and the device alone (the `_dev` entry on arrays uploaded beforehand, HIP
events on the handle's stream, `--inner` calls per timed window).  The windows of (A) and (B) alternate in one process; every figure is
given per window, with the median and the spread.  One line per measurement (append to profiles/user_sample_wave.txt).

    python bench/user_sample_wave.py [--shapes 64x32x64,34x17x128] [--S 64] [--N 50] [--repeats 5] [--inner 10]
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

from user_clock import Bench       # noqa: E402
from user_sample import spread     # noqa: E402

CHAIN_P = np.array([0.02, 9.0, 0.3, 4.0, 1.0, 0.05, 2.0, 0.8, 0.5])       # h, k, c, kc, w, r, a, gp, cp


def shape(b, a, n, m, B):
    ddp, _lib, L, h = b.ddp, b._lib, b.L, b.h
    S, N = a.S, a.N
    rng = np.random.default_rng(11)
    prm = np.repeat(CHAIN_P[:, None], B, axis=1)
    prm[1] *= 1 + 0.2 * rng.random(B)
    x0 = 0.4 * rng.standard_normal((n, B))
    u = 0.5 * rng.standard_normal((m, N, B))
    K = -0.5 / np.sqrt(n) * rng.random((m, n, N, B))
    G = rng.standard_normal((m, m, N, B))
    Sigma = 0.09 * (np.einsum("ikjb,lkjb->iljb", G, G) / m + 0.5 * np.eye(m)[:, :, None, None])
    lims = np.repeat(np.array([[-2.0, 2.0]]), m, axis=0)
    chain = ddp.DeviceProblem(ddp.example_source("chain_plant_ad"), n, m, nparam=9, autodiff=True, plant=True, wave=True, sample_wave=True)
    x = ddp.forward_pass(ddp.GaussianPolicy(), x0, u, None, 1.0, chain, lims, params=prm)[0]       # the nominal the policy acts around
    pol = ddp.GaussianPolicy(N, n, m, K, np.zeros((m, N, B)), Sigma, np.zeros((0, 0, 0)))
    seed = 20240611
    tag = "n=%d m=%d B=%d S=%d N=%d chain_plant_ad (model dynamics)" % (n, m, B, S, N)

    def tiled(arr):
        return np.repeat(arr[..., None, :], S, axis=-2).reshape(arr.shape[:-1] + (S * B,), order="F")

    def emulate(xi):
        """(B) on the host: u + L ξ and the tiled operands at batch S·B"""
        Lf = np.linalg.cholesky(np.moveaxis(Sigma, (0, 1), (-2, -1)))                              # [N, B, m, m]
        up = u[:, :, None, :] + np.einsum("nbij,jnsb->insb", Lf, xi)
        return (ddp.GaussianPolicy(N, n, m, tiled(K), np.zeros((m, N, S * B)), np.zeros((0, 0, 0)), np.zeros((0, 0, 0))), tiled(x0),
                up.reshape((m, N, S * B), order="F"), tiled(x), tiled(prm))

    def path_a():
        return ddp.sample_policy(chain, pol, x0, x, u, S, seed=seed, lims=lims, params=prm)

    def path_b():
        xi = np.random.default_rng(seed).standard_normal((m, N, S, B))
        polt, x0t, upt, xt, prmt = emulate(xi)
        return ddp.forward_pass(polt, x0t, upt, xt, 1.0, chain, lims, params=prmt)

    # ---- the two paths compute the same thing: (B) on the noise (A) draws
    xa = path_a()[0]
    kernel = h.last_kernel(1)
    polt, x0t, upt, xt, prmt = emulate(ddp.normal(seed, m, N, S, B))
    xb = ddp.forward_pass(polt, x0t, upt, xt, 1.0, chain, lims, params=prmt)[0]
    err = float(np.abs(xa.reshape(xb.shape, order="F") - xb).max() / np.abs(xb).max())
    print("%s: sample_policy vs the emulation on the same noise: states differ by %.3g (relative, max); kernels %s, %s"
          % (tag, err, kernel, h.last_kernel(1)), flush=True)

    # ---- host to host, alternating
    ta, tb = [], []
    for _ in range(a.repeats):
        t = time.perf_counter(); path_a(); ta.append(1e3 * (time.perf_counter() - t))
        t = time.perf_counter(); path_b(); tb.append(1e3 * (time.perf_counter() - t))
    print("%s: host to host, (A) sample_policy(seed): %s" % (tag, spread(ta)), flush=True)
    print("%s: host to host, (B) NumPy noise + tiling + forward_pass at batch S*B: %s" % (tag, spread(tb)), flush=True)

    # ---- the device alone
    R = S * B
    dprm, dK, dSg, dx0, du, dx, dl = (h.to_device(v) for v in (prm, K, Sigma, x0, u, x, lims.flatten(order="F")))
    oxs, ous, ocs, ocsum, ost = h.malloc(8 * n * N * R), h.malloc(8 * m * N * R), h.malloc(8 * N * R), h.malloc(8 * R), h.malloc(4 * B)
    upa = chain._ptr(h)
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
    print("%s: device alone per call (%d calls per window), (A) ddp_policy_factor_wide + ddp_user_sample_wave: %s; %.3f GB of results -> %.0f GB/s"
          % (tag, a.inner, spread(da), gb_a, gb_a / (float(np.median(da)) * 1e-3)), flush=True)
    print("%s: device alone per call (%d calls per window), (B) ddp_user_rollout_wave at batch S*B on uploaded, tiled operands: %s; %.3f GB of "
          "operands and results -> %.0f GB/s" % (tag, a.inner, spread(db), gb_b, gb_b / (float(np.median(db)) * 1e-3)), flush=True)
    print("%s: (A) over (B): host to host %.2fx the speed, device alone %.2fx the speed (medians; (B) ran on this same build)"
          % (tag, float(np.median(tb)) / float(np.median(ta)), float(np.median(db)) / float(np.median(da))), flush=True)
    for p in (dprm, dK, dSg, dx0, du, dx, dl, oxs, ous, ocs, ocsum, ost, dKt, dkt, dx0t, dupt, dxt, dprmt):
        h.free(p)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="64x32x64,34x17x128", help="n x m x B, comma separated")
    ap.add_argument("--S", type=int, default=64)
    ap.add_argument("--N", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--inner", type=int, default=10)
    a = ap.parse_args()
    if a.repeats < 3:
        raise SystemExit("--repeats: three runs at least (the spread is part of the result)")
    b = Bench()
    for s in a.shapes.split(","):
        n, m, B = (int(v) for v in s.split("x"))
        shape(b, a, n, m, B)


if __name__ == "__main__":
    main()
