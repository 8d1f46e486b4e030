"""fit_gmm / gmm_prior: the GMM dynamics prior of the guided-policy-search round, on the rollouts the sampler left on the device.
Workloads: (a) B policies of user_examples/car_plant.hip on its plant, S samples each, N = 50, K = 8, 10 EM iterations, pooled;
(b) (n, m) = (32, 8), S = 128, B = 128, K = 4 on the closed loop of a drawn stable linear system.  Paths on the same samples:
  (1) ddp_gmm_fit_f64_dev and ddp_gmm_prior_f64_dev on device arrays (HIP events);
  (2) fit_gmm and gmm_prior host to host (a host clock around the Python calls, which end in a stream synchronisation);
  (3) the same formulas in NumPy on the downloaded arrays, `--np-iters` EM iterations (it is slow: the figure is scaled to `iters`);
  (4) the same formulas in torch on the device, tensors resident (linalg.cholesky, solve_triangular for L^-1, bmm, logsumexp), if torch sees it.
(3) and (4) start from the mixture (1) starts from (its Philox start, taken with iters = 0), so all paths run the same iteration.  The
paths alternate inside one process; every figure is given per window.  Then the counts: P K p^2 fused multiply-adds of the E-step and the
bytes an iteration moves.  `--leg device` runs path (1) alone, a few calls: the leg to put under a kernel trace, which gives the time
of gmm_estep itself.  Last, one accuracy figure without a threshold: a two-regime linear plant with S < n + m, the error of [fx fu]
against the truth with the GMM prior and with a ridge alone.  One line per measurement (append to profiles/user_gmm.txt).

    python bench/user_gmm.py [--B 1024] [--S 64] [--N 50] [--K 8] [--iters 10] [--B2 128] [--S2 128] [--K2 4] [--repeats 5] [--leg all]
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
from user_fit import get_torch                       # noqa: E402
from user_sample import spread                       # noqa: E402

REG = 1e-6
LOG2PI = float(np.log(2 * np.pi))


def tuples(xs, us):
    """W[P, p], point j = s + S (i + (N - 1) b)"""
    W = np.concatenate([xs[:, :-1], us[:, :-1], xs[:, 1:]], axis=0)                  # [p, N-1, S, B]
    return np.ascontiguousarray(W.transpose(3, 1, 2, 0).reshape(-1, W.shape[0]))


def em_numpy(W, pi, mu, Sg, iters, reg):
    """pi[K], mu[K,p], Sg[K,p,p] -> after `iters` (E, M); and ll of every E-step"""
    P, p = W.shape
    ll = []
    for _ in range(iters):
        L = np.linalg.cholesky(Sg)
        lo = np.empty((len(pi), P))
        for k in range(len(pi)):
            Y = np.linalg.solve(L[k], (W - mu[k]).T)                                 # (NumPy has no triangular solve)
            lo[k] = np.log(pi[k]) - 0.5 * p * LOG2PI - np.log(np.diag(L[k])).sum() - 0.5 * (Y * Y).sum(axis=0)
        mx = lo.max(axis=0)
        lse = mx + np.log(np.exp(lo - mx).sum(axis=0))
        R = np.exp(lo - lse)
        ll.append(lse.sum())
        Nk = R.sum(axis=1)
        mu = (R @ W) / Nk[:, None]
        for k in range(len(pi)):
            D = W - mu[k]
            Sg[k] = (D * R[k, :, None]).T @ D / Nk[k] + reg * np.eye(p)
        pi = Nk / P
    return pi, mu, Sg, ll


def e_torch(torch, W, pi, mu, Sg):
    p = W.shape[1]
    L = torch.linalg.cholesky(Sg)
    V = torch.linalg.solve_triangular(L, torch.eye(p, dtype=W.dtype, device=W.device).expand_as(L), upper=False)     # L^-1: the product route
    Y = torch.bmm(V, (W[None] - mu[:, None]).transpose(1, 2))                        # [K, p, P] (a triangular solve with P right-hand sides is far slower)
    lo = torch.log(pi)[:, None] - 0.5 * p * LOG2PI - torch.log(torch.diagonal(L, dim1=1, dim2=2)).sum(1)[:, None] - 0.5 * (Y * Y).sum(1)
    lse = torch.logsumexp(lo, 0)
    return torch.exp(lo - lse), lse.sum()


def em_torch(torch, W, pi, mu, Sg, iters, reg):
    P, p = W.shape
    eye = torch.eye(p, dtype=W.dtype, device=W.device)
    ll = []
    for _ in range(iters):
        R, l = e_torch(torch, W, pi, mu, Sg)
        ll.append(l)
        Nk = R.sum(1)
        mu = (R @ W) / Nk[:, None]
        D = W[None] - mu[:, None]                                                    # [K, P, p]
        Sg = torch.bmm((D * R[:, :, None]).transpose(1, 2), D) / Nk[:, None, None] + reg * eye
        pi = Nk / P
    return pi, mu, Sg, ll


def prior_torch(torch, W, pi, mu, Sg, S, n0):
    """Phi[T, p, p], mu0[T, p] of the T = (N - 1) B steps (their S points lie together in W)"""
    R, _ = e_torch(torch, W, pi, mu, Sg)
    om = R.reshape(R.shape[0], -1, S).mean(2).T                                      # [T, K]
    m0 = om @ mu
    D = mu[None] - m0[:, None]                                                       # [T, K, p]
    return n0 * (torch.einsum("tk,kij->tij", om, Sg) + torch.einsum("tk,tki,tkj->tij", om, D, D)), m0


def measure(b, a, what, n, m, N, S, B, K, dxs, dus, xs, us, torch):
    ddp, _lib, L, h = b.ddp, b._lib, b.L, b.h
    p, iters, P, T = 2 * n + m, a.iters, (N - 1) * S * B, N * B
    lo, hi = ddp._seed_words(a.seed)
    mix = [h.malloc(8 * K), h.malloc(8 * p * K), h.malloc(8 * p * p * K), h.malloc(8 * max(iters, 1)), h.malloc(4)]
    pri = [h.malloc(8 * p * p * T), h.malloc(8 * p * T), h.malloc(4 * T)]

    def dev_fit(it=iters):
        _lib.check(L.ddp_gmm_fit_f64_dev(h.raw, n, m, N, S, B, K, it, 1, 0, dxs, dus, REG, lo, hi, None, None, None, *mix))

    def dev_prior():
        _lib.check(L.ddp_gmm_prior_f64_dev(h.raw, n, m, N, S, B, K, 1, dxs, dus, mix[0], mix[1], mix[2], 1.0, 1.0, *pri))

    def download():
        h.sync()
        return h.to_host(mix[0], (K,)), h.to_host(mix[1], (p, K)), h.to_host(mix[2], (p, p, K)), h.to_host(mix[3], (max(iters, 1),))

    dev_fit(0)
    pi0, mu0, Sg0, _ = download()                                                    # the start of every path
    dev_fit(); dev_prior()
    pid, mud, Sgd, lld = download()
    st = int(h.to_host(mix[4], (1,), dtype=np.int32)[0])
    print("%s: P = %d points, p = %d, K = %d, %d iterations: status %d, pi in [%.3f, %.3f], ll per point %.6f -> %.6f"
          % (what, P, p, K, iters, st, pid.min(), pid.max(), lld[0] / P, lld[-1] / P), flush=True)
    if a.leg == "device":
        for _ in range(3):
            dev_fit(); dev_prior()
        h.sync()
        return
    rel = lambda x, y: float(np.abs(x - y).max() / np.abs(y).max())                  # noqa: E731
    g = ddp.fit_gmm(xs, us, K, iters=iters, reg=REG, seed=a.seed)
    Phi, m0h, _, _ = ddp.gmm_prior(g, xs, us)
    Phid = h.to_host(pri[0], (p, p, N, B))
    bits = all(np.array_equal(x, y) for x, y in ((g.pi[:, 0], pid), (g.Sigma[..., 0], Sgd), (g.ll[:, 0], lld), (Phi, Phid)))
    line = "%s: (1) and (2) %s" % (what, "agree bit for bit" if bits else "DIFFER")
    W = tuples(xs, us)
    if torch is not None:
        Wt = torch.from_numpy(W).cuda()
        start = [torch.from_numpy(np.ascontiguousarray(v)).cuda() for v in (pi0, mu0.T, Sg0.transpose(2, 0, 1))]

        def tor_fit():
            r = em_torch(torch, Wt, *start, iters, REG)
            torch.cuda.synchronize()
            return r

        pit, mut, Sgt, llt = tor_fit()

        def tor_prior():
            r = prior_torch(torch, Wt, pit, mut, Sgt, S, 1.0)
            torch.cuda.synchronize()
            return r

        Phit = tor_prior()[0].cpu().numpy().reshape(B, N - 1, p, p)
        line += "; (1) vs torch: Sigma %.3g, ll %.3g, Phi %.3g (relative, max)" % (
            rel(Sgd.transpose(2, 0, 1), Sgt.cpu().numpy()), abs(lld[-1] - float(llt[-1])) / abs(lld[-1]), rel(Phid[:, :, :-1].transpose(3, 2, 0, 1), Phit))
    pin, mun, Sgn, lln = em_numpy(W, pi0, mu0.T.copy(), Sg0.transpose(2, 0, 1).copy(), a.np_iters, REG)
    line += "; (1) vs NumPy after %d iterations: ll %.3g" % (a.np_iters, abs(lld[a.np_iters - 1] - lln[-1]) / abs(lln[-1]))
    print(line, flush=True)

    t1, t1p, t2, t2p, t3, t4, t4p = [], [], [], [], [], [], []
    for _ in range(a.repeats):
        t1.append(b.timed(dev_fit)); t1p.append(b.timed(dev_prior))
        t = time.perf_counter(); g = ddp.fit_gmm(xs, us, K, iters=iters, reg=REG, seed=a.seed); t2.append(1e3 * (time.perf_counter() - t))
        t = time.perf_counter(); ddp.gmm_prior(g, xs, us); t2p.append(1e3 * (time.perf_counter() - t))
        t = time.perf_counter(); em_numpy(W, pi0, mu0.T.copy(), Sg0.transpose(2, 0, 1).copy(), a.np_iters, REG)
        t3.append(1e3 * (time.perf_counter() - t) * iters / a.np_iters)
        if torch is not None:
            torch.cuda.synchronize()
            t = time.perf_counter(); tor_fit(); t4.append(1e3 * (time.perf_counter() - t))
            t = time.perf_counter(); tor_prior(); t4p.append(1e3 * (time.perf_counter() - t))
    t0 = [b.timed(lambda: dev_fit(0)) for _ in range(a.repeats)]
    per = (float(np.median(t1)) - float(np.median(t0))) / iters
    fma = float(P) * K * p * p
    kg = max(1, 16 // ((p + 15) // 16 * ((p + 15) // 16 + 1) // 2))
    by = 8.0 * P * (p + K) + 8.0 * P * (p * -(-K // kg) + K)                          # E: the points in, r out; Gram: the points per cluster group, r in
    print("%s (1) ddp_gmm_fit_f64_dev, start and %d iterations: %s" % (what, iters, spread(t1)), flush=True)
    print("%s (1) the start alone (iters = 0): %s -> %.3f ms an iteration (E-step, means, Gram, factorisation, status)" % (what, spread(t0), per), flush=True)
    print("%s (1) an iteration: E-step %.3g fused multiply-adds (P K p^2; as much again in the Gram matrices, half of it by symmetry), "
          "%.3f GB of points and responsibilities -> at least %.0f GFLOP/s over the whole iteration, %.0f GB/s"
          % (what, fma, by / 1e9, 2 * fma / (per * 1e-3) / 1e9, by / (per * 1e-3) / 1e9), flush=True)
    print("%s (1) ddp_gmm_prior_f64_dev: %s; %.3f GB of Phi written -> %.0f GB/s" % (what, spread(t1p), 8.0 * p * p * T / 1e9,
                                                                                 8.0 * p * p * T / 1e9 / (float(np.median(t1p)) * 1e-3)), flush=True)
    print("%s (2) host to host: fit_gmm %s; gmm_prior %s" % (what, spread(t2), spread(t2p)), flush=True)
    print("%s (3) NumPy on the downloaded arrays, %d iterations scaled to %d: %s" % (what, a.np_iters, iters, spread(t3)), flush=True)
    if torch is not None:
        print("%s (4) torch on the device, tensors resident: EM %s; prior %s" % (what, spread(t4), spread(t4p)), flush=True)
        print("%s: (4) over (1): EM %.2fx the time, prior %.2fx; (3) over (2): EM %.2fx (medians)"
              % (what, float(np.median(t4)) / float(np.median(t1)), float(np.median(t4p)) / float(np.median(t1p)),
                 float(np.median(t3)) / float(np.median(t2))), flush=True)
    else:
        print("%s (4) torch: not available in this process; (3) over (2): EM %.2fx the time (medians)" % (what, float(np.median(t3)) / float(np.median(t2))), flush=True)
    for q in mix + pri:
        h.free(q)


def two_regimes(ddp):
    """x+ = A_r x + B_r u + noise, regime r = (x[0] > 0), n = 4, m = 2, S = 5 < n + m: the error of [fx fu] against [A_r B_r] on the steps
    whose samples share a regime, with the GMM prior (K = 4, pooled) and with a ridge alone"""
    rng = np.random.default_rng(31)
    n, m, N, S, B = 4, 2, 30, 5, 256
    A = np.stack([0.9 * np.eye(n) + 0.3 * rng.standard_normal((n, n)) / np.sqrt(n) for _ in range(2)])
    Bm = rng.standard_normal((2, n, m)) / np.sqrt(n)
    xs, us = np.zeros((n, N, S, B), order="F"), np.zeros((m, N, S, B), order="F")
    xh = (2.0 * rng.standard_normal((n, 1, B)) + 0.2 * rng.standard_normal((n, S, B)))
    for i in range(N):
        uh = 0.5 * rng.standard_normal((m, S, B))
        xs[:, i], us[:, i] = xh, uh
        r = (xh[0] > 0).astype(int)
        xh = np.einsum("sbij,jsb->isb", A[r], xh) + np.einsum("sbij,jsb->isb", Bm[r], uh) + 0.02 * rng.standard_normal((n, S, B))
    reg = (xs[0, :-1] > 0)                                                           # [N-1, S, B]
    one = reg.all(axis=1) | (~reg).all(axis=1)
    truth = np.concatenate([A, Bm], axis=2)[reg[:, 0].astype(int)]                   # [N-1, B, n, d]

    def err(fx, fu):
        F = np.moveaxis(np.concatenate([fx, fu], axis=1)[:, :, :-1], (0, 1), (2, 3))
        e = np.linalg.norm(F - truth, axis=(2, 3)) / np.linalg.norm(truth, axis=(2, 3))
        return np.median(e[one]), np.percentile(e[one], 90)

    g = ddp.fit_gmm(xs, us, 4, iters=20, reg=REG, seed=5)
    fp = ddp.fit_dynamics(xs, us, prior=ddp.gmm_prior(g, xs, us))
    line = "two-regime linear plant n=4 m=2 S=5 N=30 B=256, %d of %d steps in one regime, |[fx fu] - truth| / |truth| (median, 90th percentile): " \
           "GMM prior (K = 4, status %d, failed steps %d) %.3f, %.3f" % ((int(one.sum()), one.size, int(g.status[0]), int(np.count_nonzero(fp[4]))) + err(fp[0], fp[1]))
    for ridge in (1e-3, 1e-1):
        fr_ = ddp.fit_dynamics(xs, us, ridge=ridge)
        line += "; ridge %g alone (failed steps %d) %.3f, %.3f" % ((ridge, int(np.count_nonzero(fr_[4]))) + err(np.nan_to_num(fr_[0]), np.nan_to_num(fr_[1])))
    print(line, flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=1024)
    ap.add_argument("--S", type=int, default=64)
    ap.add_argument("--N", type=int, default=50)
    ap.add_argument("--K", type=int, default=8)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--B2", type=int, default=128)
    ap.add_argument("--S2", type=int, default=128)
    ap.add_argument("--K2", type=int, default=4)
    ap.add_argument("--np-iters", type=int, default=1)
    ap.add_argument("--seed", type=int, default=20141208)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--leg", choices=["all", "device"], default="all")
    a = ap.parse_args()
    if a.repeats < 3:
        raise SystemExit("--repeats: three runs at least (the spread is part of the result)")
    torch = get_torch() if a.leg == "all" else None
    b = Bench()
    ddp, _lib, L, h = b.ddp, b._lib, b.L, b.h

    # ---- (a) car_plant: the sampler's bench shape, on the plant
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
    measure(b, a, "car_plant on its plant B=%d S=%d N=%d" % (B, S, N), n, m, N, S, B, a.K, dxs, dus, xs, us, torch)
    for q in (dxs, dus, ocs, ocsum, ost):
        h.free(q)

    # ---- (b) (32, 8): the closed loop of a drawn stable linear system under control noise, B2 trajectories
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
    measure(b, a, "linear system n=32 m=8 B=%d S=%d N=%d" % (B, S, N), n, m, N, S, B, a.K2, dxs, dus, xs, us, torch)
    if a.leg == "all":
        two_regimes(ddp)


if __name__ == "__main__":
    main()
