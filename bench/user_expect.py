"""expected_cost: moments and expected cost of B linear-Gaussian policies under fitted linear-Gaussian dynamics and a fitted quadratic cost
(N = 50), the step that closes the guided-policy-search round.  Four paths on the same drawn tables:
  (1) ddp_expected_cost_f64_dev on device arrays (HIP events, `--inner` calls per window), ec only — what kl_step_adjust needs;
  (2) expected_cost host to host (a host clock around the Python call, which ends in a stream synchronisation);
  (3) the same recursion in NumPy on host arrays: a loop over i of batched products, what a user does without the entry;
  (4) the same recursion in torch on the same device, tensors resident: the loop over i of batched products (torch.matmul), one
      synchronisation at the end — the device comparator of (1), in the same process and the same windows.
(3) and (4) get their operands in the layout they like ([B, N, rows, cols], G = [fx fu] and H assembled beforehand, outside the clock).
The paths alternate; every figure is given per window.  Shapes: the car_plant shape of bench/user_fit.py (n, m) = (4, 2), B = 1 024, and
(n, m) = (32, 8), B = 128.  One line per measurement (append to profiles/user_expect.txt).

    python bench/user_expect.py [--B 1024] [--N 50] [--B2 128] [--repeats 5] [--inner 50]
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
from user_fit import get_torch                       # noqa: E402
from user_sample import spread                       # noqa: E402

HBM_PEAK = 8.0e12                                    # bytes/s, the MI355X specification


def draw(n, m, N, B, seed):
    """tables in the library's layout: a contracting closed loop, positive definite covariances, indefinite cost Hessians"""
    rng = np.random.default_rng(seed)
    F = np.asfortranarray
    spd = lambda k, s, *lead: (lambda A: s * (A @ np.swapaxes(A, -1, -2) / k + 0.5 * np.eye(k)))(rng.standard_normal(lead + (k, k)))    # noqa: E731
    mats = lambda a: F(np.moveaxis(a, (0, 1), (3, 2)))                                   # noqa: E731  [B,N,r,c] -> [r,c,N,B]
    vecs = lambda a: F(np.moveaxis(a, (0, 1), (2, 1)))                                   # noqa: E731  [B,N,r] -> [r,N,B]
    sym = lambda a: (a + np.swapaxes(a, -1, -2)) / 2                                     # noqa: E731
    t = dict(K=mats(0.3 * rng.standard_normal((B, N, m, n)) / np.sqrt(n)), Sg=mats(spd(m, 0.2, B, N)),
             fx=mats(0.7 * rng.standard_normal((B, N, n, n)) / np.sqrt(n)), fu=mats(0.5 * rng.standard_normal((B, N, n, m)) / np.sqrt(m)),
             fc=vecs(0.3 * rng.standard_normal((B, N, n))), cov=mats(spd(n, 0.1, B, N)), x=vecs(rng.standard_normal((B, N, n))),
             u=vecs(rng.standard_normal((B, N, m))), cx=vecs(rng.standard_normal((B, N, n))), cu=vecs(rng.standard_normal((B, N, m))),
             cxx=mats(sym(rng.standard_normal((B, N, n, n)) / np.sqrt(n))), cxu=mats(rng.standard_normal((B, N, n, m)) / np.sqrt(n)),
             cuu=mats(sym(rng.standard_normal((B, N, m, m)) / np.sqrt(m))), c0=F(2.0 + rng.standard_normal((N, B))),
             S0=F(np.moveaxis(spd(n, 0.3, B), 0, 2)))
    return t


def as_rows(t, conv):
    """the operands of the emulations: [B, N, rows, cols] / [B, N, rows], G = [fx fu] and H = [cxx cxu; cxu' cuu] assembled"""
    mat = lambda a: np.ascontiguousarray(a.transpose(3, 2, 0, 1))                        # noqa: E731
    vec = lambda a: np.ascontiguousarray(a.transpose(2, 1, 0))                           # noqa: E731
    cxu = mat(t["cxu"])
    H = np.concatenate([np.concatenate([mat(t["cxx"]), cxu], -1), np.concatenate([np.swapaxes(cxu, -1, -2), mat(t["cuu"])], -1)], -2)
    r = dict(K=mat(t["K"]), Sg=mat(t["Sg"]), G=np.concatenate([mat(t["fx"]), mat(t["fu"])], -1), fc=vec(t["fc"]), cov=mat(t["cov"]), x=vec(t["x"]),
             u=vec(t["u"]), cx=vec(t["cx"]), cu=vec(t["cu"]), H=np.ascontiguousarray(H), c0=np.ascontiguousarray(t["c0"].T),
             S0=np.ascontiguousarray(t["S0"].transpose(2, 0, 1)))
    return {k: conv(v) for k, v in r.items()}


def recursion(r, N, cat, stack, tr):
    """the recursion of include/ddp_amd.h as a loop over i of batched products -> ec[N, B]"""
    mux, Sx = r["x"][:, 0], r["S0"]
    ecs = []
    for i in range(N):
        K = r["K"][:, i]
        dx = mux - r["x"][:, i]
        du = (K @ dx[..., None])[..., 0]
        SK = Sx @ tr(K)
        Sz = cat([cat([Sx, SK], -1), cat([tr(SK), K @ SK + r["Sg"][:, i]], -1)], -2)
        dz = cat([dx, du], -1)
        H = r["H"][:, i]
        ecs.append(r["c0"][:, i] + (r["cx"][:, i] * dx).sum(-1) + (r["cu"][:, i] * du).sum(-1) + 0.5 * (dz * (H @ dz[..., None])[..., 0]).sum(-1)
                   + 0.5 * (H * Sz).sum((-1, -2)))
        if i < N - 1:
            G = r["G"][:, i]
            mux = (G @ cat([mux, r["u"][:, i] + du], -1)[..., None])[..., 0] + r["fc"][:, i]
            Sx = G @ Sz @ tr(G) + r["cov"][:, i]
    return stack(ecs, 0)


def measure(b, a, what, n, m, N, B, torch):
    ddp, _lib, L, h = b.ddp, b._lib, b.L, b.h
    t = draw(n, m, N, B, 17 + n)
    order = ("K", "Sg", None, "x", "u", "fx", "fu", "fc", "cov", "cx", "cu", "cxx", "cxu", "cuu", "c0", "S0")
    dev_in = {k: h.to_device(t[k]) for k in order if k}
    dec, dst = h.malloc(8 * N * B), h.malloc(4 * B)
    ptr = lambda k: None if k is None else dev_in[k]                                     # noqa: E731

    def dev():
        for _ in range(a.inner):
            _lib.check(L.ddp_expected_cost_f64_dev(h.raw, n, m, N, B, *[ptr(k) for k in order[:9]], 1, *[ptr(k) for k in order[9:15]], 1, ptr("S0"),
                                                   dec, dst, None, None))

    pol = ddp.GaussianPolicy(N, n, m, t["K"], np.zeros((m, N, B)), t["Sg"], None)

    def host():
        return ddp.expected_cost(pol, None, t["x"], t["u"], (t["fx"], t["fu"], t["fc"], t["cov"]), tuple(t[k] for k in ("cx", "cu", "cxx", "cxu", "cuu", "c0")),
                                 Sigma0=t["S0"])

    rn = as_rows(t, lambda v: v)

    def num():
        return recursion(rn, N, np.concatenate, np.stack, lambda v: np.swapaxes(v, -1, -2))

    if torch is not None:
        rt = as_rows(t, lambda v: torch.from_numpy(v).cuda())

        def tor():
            r = recursion(rt, N, torch.cat, torch.stack, lambda v: v.transpose(-1, -2))
            torch.cuda.synchronize()
            return r

    # ---- the paths agree on the same tables
    dev(); h.sync()
    ecd, std = h.to_host(dec, (N, B)), h.to_host(dst, (B,), dtype=np.int32)
    ech, sth = host()
    ecn = num()
    rel = lambda p, q: float(np.abs(p - q).max() / np.abs(q).max())                      # noqa: E731
    line = "%s: failed trajectories %d of %d; (1) and (2) %s; ec of (2) vs NumPy %.3g (relative, max)" % (
        what, int(np.count_nonzero(sth)), B, "agree bit for bit" if np.array_equal(ecd, ech) and np.array_equal(std, sth) else "DIFFER", rel(ech, ecn))
    if torch is not None:
        line += "; vs torch %.3g" % rel(ech, tor().cpu().numpy())
    print(line, flush=True)

    # ---- five windows each, alternating
    t1, t2, t3, t4 = [], [], [], []
    for _ in range(a.repeats):
        t1.append(b.timed(dev) / a.inner)
        c = time.perf_counter(); host(); t2.append(1e3 * (time.perf_counter() - c))
        c = time.perf_counter(); num(); t3.append(1e3 * (time.perf_counter() - c))
        if torch is not None:
            torch.cuda.synchronize()
            c = time.perf_counter(); tor(); t4.append(1e3 * (time.perf_counter() - c))
    p = n + m
    per_step = 8.0 * (m * n + m * m + p + n * p + n + n * n + p + n * n + n * m + m * m + 1)
    gb = (per_step * N * B + 8.0 * (n * n * B + N * B)) / 1e9
    rate = gb * 1e9 / (float(np.median(t1)) * 1e-3)
    print("%s (1) device alone per call (%d calls per window), ddp_expected_cost: %s; %.1f KB of operands a trajectory-step, %.3f GB a call -> "
          "%.0f GB/s, %.1f%% of the 8 TB/s of HBM; %.2f us a step of the chain"
          % (what, a.inner, spread(t1), per_step / 1e3, gb, rate / 1e9, 100 * rate / HBM_PEAK, 1e3 * float(np.median(t1)) / N), flush=True)
    print("%s (2) host to host, expected_cost: %s" % (what, spread(t2)), flush=True)
    print("%s (3) NumPy on host arrays (a loop over i of batched products): %s" % (what, spread(t3)), flush=True)
    if torch is not None:
        print("%s (4) torch on the device (the same loop, tensors resident, one synchronisation): %s" % (what, spread(t4)), flush=True)
        print("%s: (4) over (1) %.2fx the time; (3) over (2) %.2fx the time (medians)"
              % (what, float(np.median(t4)) / float(np.median(t1)), float(np.median(t3)) / float(np.median(t2))), flush=True)
    else:
        print("%s (4) torch: not available in this process; (3) over (2) %.2fx the time (medians)"
              % (what, float(np.median(t3)) / float(np.median(t2))), flush=True)
    for q in list(dev_in.values()) + [dec, dst]:
        h.free(q)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=1024)
    ap.add_argument("--N", type=int, default=50)
    ap.add_argument("--B2", type=int, default=128)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--inner", type=int, default=50)
    a = ap.parse_args()
    if a.repeats < 3:
        raise SystemExit("--repeats: three runs at least (the spread is part of the result)")
    torch = get_torch()
    b = Bench()
    measure(b, a, "car_plant shape n=4 m=2 B=%d N=%d" % (a.B, a.N), 4, 2, a.N, a.B, torch)
    measure(b, a, "n=32 m=8 B=%d N=%d" % (a.B2, a.N), 32, 8, a.N, a.B2, torch)


if __name__ == "__main__":
    main()
