"""Wide controls (8 < m <= 32): back_pass_wide_kernel and forward_wide_kernel timed with HIP events on the handle's stream, medians of
`--reps` launches after `--warmup`.  Operands are generated on the device (torch) and stay there; every leg prints one line
(append to profiles/wide_controls.txt):
  ab      DDP_BACKPASS=c against the default kernel on the shapes they share — (32, 8) N = 300 and (64, 8) N = 256, B = 1 024,
          per-trajectory LTV dynamics — alternating the two in one process;
  shapes  (12,12) N = 500 B = 2 048; (24,16), (36,12) N = 300 B = 1 024; (64,32) N = 256 B = 1 024, per-trajectory LTV dynamics and a
          shared cost, with and without limits: backward pass, rollout (1 and 11 step sizes), and the fraction of the 8 TB/s HBM
          roofline from the algorithmic bytes (what a step must read and write once);
  cpu     one backward + one forward pass of the C oracle on one host core at (24,16), N = 300 (ddp_oracle_pass_batch_lq, as
          bench.py --full's CPU leg) against the same two passes on the GPU at B = 1 .. 1 024: the batch size from which the GPU wins;
  solves  1 024 LQ solves at (12,12), T = 500, limits ±0.6: wall time and global iterations of ddp_amd.iLQG;
  usage   registers / LDS / scratch of the new kernels from the build's kernel-resource-usage records.

    python bench/wide_controls.py [--legs ab,shapes,cpu,solves,usage] [--reps 7] [--warmup 2]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_PEAK = 8e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--legs", default="usage,ab,shapes,cpu,solves")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--scale", type=float, default=1.0, help="scales every batch size (rehearsals)")
    a = ap.parse_args()
    legs = a.legs.split(",")
    if "usage" in legs:
        for unit in ("back_pass_wide", "forward_pass_wide"):
            p = os.path.join(ROOT, "differentialdynamicprogramming.jl_amd", "build", unit + ".o.usage.json")
            for name, u in json.load(open(p)).items():
                print("usage %s: VGPRs %s AGPRs %s SGPRs %s (spilled %s) scratch %s B/lane static LDS %s B occupancy %s" % (
                    name, u.get("VGPRs"), u.get("AGPRs"), u.get("TotalSGPRs"), u.get("SGPRs Spill"), u.get("ScratchSize"), u.get("LDS Size"), u.get("Occupancy")))
        legs.remove("usage")
    if not legs:
        return
    import torch
    assert torch.cuda.is_available(), "bench/wide_controls.py needs a GPU"
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    import ddp_amd
    from ddp_amd import _lib
    h = ddp_amd.Handle(0, stream=torch.cuda.current_stream(dev).cuda_stream)
    L = _lib.lib()
    gen = torch.Generator(device=dev).manual_seed(7)
    f64 = dict(dtype=torch.float64, device=dev)
    randn = lambda *s: torch.randn(*s, generator=gen, **f64)
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    sc = lambda B: max(1, int(round(B * a.scale)))

    def median_ms(fn):
        for _ in range(a.warmup):
            fn()
        ts = []
        for _ in range(a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); fn(); e1.record(); torch.cuda.synchronize()
            ts.append(e0.elapsed_time(e1))
        return float(np.median(ts)), float(min(ts)), float(max(ts))

    class BP:
        """a backward-pass call on the device, operands in torch's column-major-by-construction flat layout [.., N, B] -> (B, N, ..)"""
        def __init__(self, n, m, N, B, dyn_batched_tv=True, lim=None):
            self.n, self.m, self.N, self.B, self.lim = n, m, N, B, lim
            cnt = (B, N) if dyn_batched_tv else ()
            eye = lambda d: torch.eye(d, **f64)
            self.fx = (0.95 * eye(n) + 0.05 / np.sqrt(n) * randn(*cnt, n, n)).contiguous()       # (B, N, col, row): symmetric in law, any layout does
            self.fu = (0.3 / np.sqrt(n) * randn(*cnt, m, n)).contiguous()
            A1, A2 = randn(n, n), randn(m, m)
            self.cxx = (eye(n) + 0.2 * A1 @ A1.T / n).contiguous()
            self.cuu = (0.1 * (eye(m) + 0.2 * A2 @ A2.T / m)).contiguous()
            self.cxu = (0.02 * randn(m, n)).contiguous()
            self.cx, self.cu, self.u = randn(B, N, n), 0.3 * randn(B, N, m), 0.2 * randn(B, N, m)
            self.lam = torch.ones(B, **f64)
            self.lims = None
            if lim is not None:
                self.u.clamp_(-lim, lim)
                self.lims = torch.tensor([-lim] * m + [lim] * m, **f64)
            self.K, self.k, self.Quu = torch.empty(B * N * n * m, **f64), torch.empty(B * N * m, **f64), torch.empty(B * N * m * m, **f64)
            self.Vx, self.Vxx, self.dV = torch.empty(B * N * n, **f64), torch.empty(B * N * n * n, **f64), torch.empty(2 * B, **f64)
            self.div = torch.zeros(B, dtype=torch.int32, device=dev)
            self.desc = _lib.BPDesc(n, m, N, B, int(dyn_batched_tv), int(dyn_batched_tv), 0, 0, 1, int(lim is not None))

        def run(self):
            _lib.check(L.ddp_back_pass_f64_dev(h.raw, C.byref(self.desc), p(self.cx), p(self.cu), p(self.cxx), p(self.cxu), p(self.cuu), p(self.fx),
                                               p(self.fu), p(self.lam), p(self.lims), p(self.u if self.lims is not None else None), None, p(self.K),
                                               p(self.k), p(self.Quu), p(self.Vx), p(self.Vxx), p(self.dV), p(self.div)))

        def bytes(self):
            n, m = self.n, self.m
            rd = (n + m + (m if self.lim is not None else 0) + (n * n + n * m if self.desc.fx_tv else 0)) * 8
            wr = (m * n + m + n + n * n + m * m) * 8
            return (rd + wr) * (self.N - 1) * self.B

    def env(**kw):
        for k_, v in kw.items():
            if v is None:
                os.environ.pop(k_, None)
            else:
                os.environ[k_] = v

    if "ab" in legs:
        for n, m, N, B in ((32, 8, 300, sc(1024)), (64, 8, 256, sc(1024))):
            bp = BP(n, m, N, B)
            res = {}
            for rnd in range(2):                                   # alternate: default, forced, default, forced
                for name, val in (("default", None), ("wide", "c")):
                    env(DDP_BACKPASS=val)
                    med = median_ms(bp.run)
                    torch.cuda.synchronize()
                    res.setdefault(name, []).append((med, h.last_kernel(0), int(bp.div.abs().max())))
            env(DDP_BACKPASS=None)
            d, w = res["default"], res["wide"]
            print("ab n=%d m=%d N=%d B=%d per-trajectory LTV: %s %.3f / %.3f ms (two rounds, median of %d; min %.3f max %.3f), %s %.3f / %.3f ms "
                  "(min %.3f max %.3f): ratio %.2f; diverged %d %d" % (n, m, N, B, d[0][1], d[0][0][0], d[1][0][0], a.reps, min(d[0][0][1], d[1][0][1]),
                                                                   max(d[0][0][2], d[1][0][2]), w[0][1], w[0][0][0], w[1][0][0], min(w[0][0][1], w[1][0][1]),
                                                                   max(w[0][0][2], w[1][0][2]), (w[0][0][0] + w[1][0][0]) / (d[0][0][0] + d[1][0][0]), d[0][2], w[0][2]))
            del bp
            torch.cuda.empty_cache()

    def rollout_call(n, m, N, B, bp, na, lim):
        """forward pass on the backward pass's own K, k around x = 0, u: returns the call"""
        P = _lib.Problem()
        P.kind, P.n, P.m, P.N, P.B = 0, n, m, N, B
        Q, R = torch.eye(n, **f64) * 0.05, torch.eye(m, **f64) * 0.005
        P.A, P.Bm, P.Q, P.R = bp.fx.data_ptr(), bp.fu.data_ptr(), Q.data_ptr(), R.data_ptr()
        P.dyn_tv, P.dyn_batched, P.cost_diag = int(bp.desc.fx_tv), int(bp.desc.fx_batched), 0
        x0, x = 0.1 * randn(B, n), torch.zeros(B * N * n, **f64)
        al = np.ascontiguousarray(10.0 ** np.linspace(0, -3, 11)[:na])
        xn, un = torch.empty(n * N * B * na, **f64), torch.empty(m * N * B * na, **f64)
        cn, cs = torch.empty(N * B * na, **f64), torch.empty(B * na, **f64)
        keep = (Q, R, x0, x, al, xn, un, cn, cs, P)

        def run():
            _lib.check(L.ddp_forward_pass_f64_dev(h.raw, C.byref(P), p(bp.K), p(bp.k), p(x0), p(bp.u), p(x), C.c_void_p(al.ctypes.data), na,
                                                  p(bp.lims), None, p(xn), p(un), p(cn), p(cs)))
        run.keep = keep
        return run

    if "shapes" in legs:
        for n, m, N, B in ((12, 12, 500, sc(2048)), (24, 16, 300, sc(1024)), (36, 12, 300, sc(1024)), (64, 32, 256, sc(1024))):
            for lim in (None, 0.5):
                bp = BP(n, m, N, B, lim=lim)
                med, lo, hi = median_ms(bp.run)
                torch.cuda.synchronize()
                kern, dv = h.last_kernel(0), int((bp.div != 0).sum())
                frac = bp.bytes() / (med * 1e-3) / HBM_PEAK
                clamped = float(((bp.k.view(B, N, m) + bp.u == lim) | (bp.k.view(B, N, m) + bp.u == -lim)).double().mean()) if lim else 0.0
                r1 = rollout_call(n, m, N, B, bp, 1, lim)
                f1 = median_ms(r1)
                r11 = rollout_call(n, m, N, B, bp, 11, lim)
                f11 = median_ms(r11)
                torch.cuda.synchronize()
                print("shapes n=%d m=%d N=%d B=%d per-trajectory LTV limits=%s: %s %.3f ms (min %.3f max %.3f, median of %d), %.1f MB algorithmic, "
                      "%.4f of 8 TB/s; diverged %d, clamped share of k %.2f; %s 1 step size %.3f ms, 11 step sizes %.3f ms" % (
                          n, m, N, B, lim, kern, med, lo, hi, a.reps, bp.bytes() / 1e6, frac, dv, clamped, h.last_kernel(1), f1[0], f11[0]))
                del bp, r1, r11
                torch.cuda.empty_cache()

    if "cpu" in legs:
        from oracle import oracle_ctypes as oc
        n, m, N = 24, 16, 300
        rng = np.random.default_rng(3)
        A = 0.95 * np.eye(n) + 0.05 / np.sqrt(n) * rng.standard_normal((n, n)); Bm = 0.3 / np.sqrt(n) * rng.standard_normal((n, m))
        Q, R = 0.05 * np.eye(n), 0.005 * np.eye(m)
        S = 16
        prob = oc.make_problem("lq", n, m, N, A=A, B=Bm, Q=Q, R=R)
        F = lambda *s: np.asfortranarray(rng.standard_normal(s))
        xs, us, cxs, cus, x0s = 0.1 * F(n, N, S), 0.1 * F(m, N, S), F(n, N, S), 0.3 * F(m, N, S), 0.1 * F(n, S)
        z = lambda *s: np.zeros(s, order="F")
        outs = [z(m, n, N, S), z(m, N, S), z(m, m, N, S), z(n, N, S), z(n, n, N, S), z(2, S), z(n, N, S), z(m, N, S), z(N, S)]
        P_ = oc._p
        lib = oc.lib()
        best = 1e9
        for _ in range(3):
            t0 = time.perf_counter()
            lib.ddp_oracle_pass_batch_lq(C.byref(prob), S, P_(cxs), P_(cus), P_(oc._f(Q)), P_(z(n, m)), P_(oc._f(R)), C.c_double(1.0), 1, P_(x0s), P_(us),
                                         P_(xs), C.c_double(1.0), *[P_(o) for o in outs])
            best = min(best, (time.perf_counter() - t0) / S)
        line, win = [], None
        for B in (1, 2, 4, 8, 16, 32, 64, 128, 256, 1024):
            bp = BP(n, m, N, B, dyn_batched_tv=False)
            bp.fx, bp.fu = torch.from_numpy(np.ascontiguousarray(A.T)).to(dev), torch.from_numpy(np.ascontiguousarray(Bm.T)).to(dev)
            roll = rollout_call(n, m, N, B, bp, 1, None)
            med = median_ms(lambda: (bp.run(), roll()))[0]
            line.append("B=%d %.3f ms (CPU %.3f)" % (B, med, best * 1e3 * B))
            if win is None and med < best * 1e3 * B:
                win = B
        print("cpu n=%d m=%d N=%d: one core of the C oracle %.3f ms per backward + forward pass; GPU backward + rollout, shared LTI: %s; the GPU wins "
              "from B = %s" % (n, m, N, best * 1e3, ", ".join(line), win))

    if "solves" in legs:
        from oracle import np_restatement as npr
        n, m, T, B = 12, 12, 500, sc(1024)
        rng = np.random.default_rng(5)
        Pm = npr.make_lq_problem(rng, n=n, m=m, T=T, h=0.05)
        x0 = Pm["x0"][:, None] + 0.1 * rng.standard_normal((n, B))
        u0 = 3.0 * 0.1 * rng.standard_normal((m, T, B))
        lims = np.stack([-0.6 * np.ones(m), 0.6 * np.ones(m)], 1)
        prob = ddp_amd.LQProblem(Pm["A"], Pm["B"], Pm["Q"], Pm["R"])
        best = None
        for _ in range(2):
            t0 = time.perf_counter()
            r = ddp_amd.iLQG(prob, x0, u0, lims=lims, timing=False, handle=h)
            dt = time.perf_counter() - t0
            best = dt if best is None else min(best, dt)
        st = r[6]["status"]
        print("solves %d LQ solves n=%d m=%d T=%d limits ±0.6: %.3f s wall (host arrays in and out, best of 2), %d global iterations, iterations per "
              "solve median %d max %d, status counts %s, %.2f of the final controls on a bound, kernels %s / %s" % (
                  B, n, m, T, best, r[6]["global_iters"], int(np.median(r[6]["iter"])), int(r[6]["iter"].max()),
                  dict(zip(*np.unique(st, return_counts=True))), float(np.mean(np.abs(r[1]) == 0.6)), h.last_kernel(0), h.last_kernel(1)))


if __name__ == "__main__":
    main()
