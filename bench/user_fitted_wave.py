"""DDP_USER_FITTED_WAVE: the rollout and the whole KL loop of user_examples/chain_plant_ad.hip on fitted time-varying affine tables at the
shapes of DDP_USER_WAVE, (n, m) = (64, 32) with B = 64 and (34, 17) with B = 128, N = 50.  No emulation exists (the tables of one
trajectory at (64, 32) hold 310 000 doubles, a parameter block 4 096), so the yardsticks are:
  (a) ddp_user_rollout_fit_wave with a policy and limits, one step size (the `_dev` entry on uploaded arrays);
  (b) ddp_user_rollout_wave on the problem's own dynamics at the same shape and batch: the rollout the loop runs without the flag, code
      this flag does not touch.  The chain's dynamics are sparse (a few operations per coordinate), so (a) does more arithmetic,
      2 n (n + m) flops per step, and moves the tables on top;
  (c) the same recursion in torch on the device, if torch imports and sees it: a loop over the steps of batched products (bmm) on
      resident tensors, with the clamp and the quadratic part of the cost;
  (d) the algorithmic bytes of (a) and their share of the 8 TB/s roofline;
  (e) whole solves: ddp_user_ilqgkl_fit_f64_dev (fitted=True, wide=True) against ddp_user_ilqgkl_f64_dev (wide=True) on the problem's
      own model, the same inputs.
The tables are the linearisation of the chain's model along its nominal plus a small perturbation, fc making the nominal consistent: a
bounded closed loop, so that every path works on ordinary numbers.  (a), (b) and (c) alternate inside one process, five windows each,
every figure given per window.  One line per measurement (append to profiles/user_fitted_wave.txt).

    python bench/user_fitted_wave.py [--shapes 64x32x64,34x17x128] [--N 50] [--repeats 5] [--inner 20] [--inner-kl 2]
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
from user_fit import get_torch     # noqa: E402
from user_sample import spread     # noqa: E402

CHAIN_P = np.array([0.02, 9.0, 0.3, 4.0, 1.0, 0.05, 2.0, 0.8, 0.5])       # h, k, c, kc, w, r, a, gp, cp


def shape(b, a, n, m, B, torch):
    ddp, _lib, L, h = b.ddp, b._lib, b.L, b.h
    N, T = a.N, a.N * B
    rng = np.random.default_rng(13)
    prm = np.repeat(CHAIN_P[:, None], B, axis=1)
    prm[1] *= 1 + 0.2 * rng.random(B)
    x0 = 0.4 * rng.standard_normal((n, B))
    u = 0.5 * rng.standard_normal((m, N, B))
    K = -0.5 / np.sqrt(n) * rng.random((m, n, N, B))
    lims = np.repeat(np.array([[-2.0, 2.0]]), m, axis=0)
    chain = ddp.DeviceProblem(ddp.example_source("chain_plant_ad"), n, m, nparam=9, autodiff=True, plant=True, wave=True, sample_wave=True,
                              fitted_wave=True)
    tag = "n=%d m=%d B=%d N=%d chain_plant_ad" % (n, m, B, N)
    # the tables: the model's Jacobians along its own rollout + 1e-3 noise, fc making that rollout consistent
    x = ddp.forward_pass(ddp.GaussianPolicy(), x0, u, None, 1.0, chain, lims, params=prm)[0]
    fx, fu = (np.array(v, order="F") for v in ddp.df(chain, x, u, params=prm)[:2])
    fx += 1e-3 * rng.standard_normal(fx.shape); fu += 1e-3 * rng.standard_normal(fu.shape)
    fc = np.zeros((n, N, B), order="F")
    fc[:, :-1] = x[:, 1:] - np.einsum("ijtb,jtb->itb", fx, x)[:, :-1] - np.einsum("iqtb,qtb->itb", fu, u)[:, :-1]
    fx[:, :, -1] = 0.0; fu[:, :, -1] = 0.0
    xm, _, cm = ddp.forward_pass(None, x0, u, None, 1.0, chain, lims, params=prm, model=(fx, fu, fc))
    k0 = 0.05 * rng.standard_normal((m, N, B))
    one = np.array([1.0])
    al = one.ctypes.data_as(C.c_void_p)
    dev = {k_: h.to_device(np.asfortranarray(v)) for k_, v in dict(prm=prm, K=K, k0=k0, x0=x0, u=u, x=xm, xo=x, fx=fx, fu=fu, fc=fc,
                                                                   lims=lims).items()}
    out = [[h.malloc(8 * n * T), h.malloc(8 * m * T), h.malloc(8 * N * B), h.malloc(8 * B)] for _ in range(2)]
    up = chain._ptr(h)

    def roll_fit():
        for _ in range(a.inner):
            _lib.check(L.ddp_user_rollout_fit_f64_dev(h.raw, up, N, B, dev["prm"], 1, dev["K"], dev["k0"], dev["x0"], dev["u"], dev["x"], al, 1,
                                                      dev["lims"], None, dev["fx"], dev["fu"], dev["fc"], *out[0]))

    def roll_own():
        for _ in range(a.inner):
            _lib.check(L.ddp_user_forward_pass_f64_dev(h.raw, up, N, B, dev["prm"], 1, dev["K"], dev["k0"], dev["x0"], dev["u"], dev["xo"], al, 1,
                                                       dev["lims"], None, *out[1]))

    roll_fit(); ka = h.last_kernel(1); roll_own(); kb = h.last_kernel(1); h.sync()
    xa, ua = h.to_host(out[0][0], (n, N, B)), h.to_host(out[0][1], (m, N, B))
    line = "%s: kernels %s, %s; states of (a) finite: %s, max |x| %.3g" % (tag, ka, kb, bool(np.all(np.isfinite(xa))), float(np.abs(xa).max()))

    tor = None
    if torch is not None:
        tK, tk, tu, tx, tfx, tfu, tfc = (torch.from_numpy(np.ascontiguousarray(np.moveaxis(v, -1, 0))).cuda() for v in (K, k0, u, xm, fx, fu, fc))
        tx0 = torch.from_numpy(np.ascontiguousarray(x0.T)).cuda()
        w, r = float(CHAIN_P[4]), float(CHAIN_P[5])

        def tor():
            """[B, ...] tensors: û = clamp(u + k + K (x̂ - x)), the quadratic part of the chain's cost, x̂⁺ = fx x̂ + fu û + fc"""
            xh = tx0
            xs, us, cs = [], [], []
            for i in range(N):
                uu = torch.clamp(tu[:, :, i] + tk[:, :, i] + torch.bmm(tK[:, :, :, i], (xh - tx[:, :, i]).unsqueeze(2)).squeeze(2), -2.0, 2.0)
                xs.append(xh); us.append(uu)
                cs.append(0.5 * w * ((xh[:, :m] ** 2).sum(1) + 0.1 * (xh[:, m:] ** 2).sum(1)) + 0.5 * r * (uu ** 2).sum(1))
                if i < N - 1:
                    xh = tfc[:, :, i] + torch.bmm(tfx[:, :, :, i], xh.unsqueeze(2)).squeeze(2) + torch.bmm(tfu[:, :, :, i], uu.unsqueeze(2)).squeeze(2)
            r_ = torch.stack(xs, 2), torch.stack(us, 2), torch.stack(cs, 1)
            torch.cuda.synchronize()
            return r_
        xt, ut, _ = tor()
        rel = lambda p, q: float(np.abs(p - q).max() / np.abs(q).max())                        # noqa: E731
        line += "; (a) vs torch: x %.3g, u %.3g (relative, max)" % (rel(xa, np.moveaxis(xt.cpu().numpy(), 0, -1)), rel(ua, np.moveaxis(ut.cpu().numpy(), 0, -1)))
    print(line, flush=True)

    ta, tb, tc = [], [], []
    for _ in range(a.repeats):
        ta.append(b.timed(roll_fit) / a.inner)
        tb.append(b.timed(roll_own) / a.inner)
        if tor is not None:
            torch.cuda.synchronize()
            t = time.perf_counter(); tor(); tc.append(1e3 * (time.perf_counter() - t))
    ma, mb = float(np.median(ta)), float(np.median(tb))
    # (d) tables of N - 1 steps, K, k, u, x in, x, u, c out
    gb = 8.0 * B * ((n * n + n * m + n) * (N - 1) + N * (m * n + 2 * m + n + n + m + 1)) / 1e9
    print("%s (a) ddp_user_rollout_fit_wave per call, policy and limits (%d calls per window): %s" % (tag, a.inner, spread(ta)), flush=True)
    print("%s (b) ddp_user_rollout_wave on the problem's own (sparse) dynamics per call: %s" % (tag, spread(tb)), flush=True)
    if tc:
        print("%s (c) torch on the device (a loop over the steps of bmm; tensors resident, one synchronisation): %s" % (tag, spread(tc)), flush=True)
    else:
        print("%s (c) torch: not available in this process" % tag, flush=True)
    print("%s (d) %.4f GB algorithmic -> %.0f GB/s, %.2f%% of the 8 TB/s roofline; %.1f us per step of the chain"
          % (tag, gb, gb / (ma * 1e-3), 100 * gb / (ma * 1e-3) / 8000.0, 1e3 * ma / N), flush=True)
    print("%s: (a) over (b) %.2fx the time%s (medians; (b) ran on this same build)"
          % (tag, ma / mb, "; (c) over (a) %.2fx the time" % (float(np.median(tc)) / ma) if tc else ""), flush=True)

    if not a.inner_kl:
        for p in list(dev.values()) + out[0] + out[1]:
            h.free(p)
        return
    # ---- (e) whole solves
    o = _lib.ILQGKLOpts()
    L.ddp_ilqgkl_default_opts(C.byref(o))
    o.kl_step, o.max_iter = 1.0, 10
    Sp = np.repeat(np.repeat((0.09 * np.eye(m))[:, :, None, None], N, 2), B, 3)
    Sip = np.repeat(np.repeat((np.eye(m) / 0.09)[:, :, None, None], N, 2), B, 3)
    co = ddp.forward_pass(None, x0, u, None, 1.0, chain, lims, params=prm)[2]
    dk = {k_: h.to_device(np.asfortranarray(v)) for k_, v in dict(Sp=Sp, Sip=Sip, c0=cm.sum(axis=0), c1=co.sum(axis=0), R1=1e-3 * np.eye(n)).items()}
    res = [[h.malloc(8 * s) for s in (n * T, m * T, m * n * T, m * m * T, m * m * T, n * T, n * n * T, N * B, 2 * B, 12 * B)] for _ in range(2)]
    its = [C.c_int(0), C.c_int(0)]
    was = h.set_kl_wide(True)

    def kl_fit():
        for _ in range(a.inner_kl):
            _lib.check(L.ddp_user_ilqgkl_fit_f64_dev(h.raw, up, N, B, dev["prm"], 1, C.byref(o), dev["x"], dk["c0"], dev["K"], dev["u"], dk["Sp"],
                                                     dk["Sip"], None, 1, dk["R1"], dev["lims"], None, dev["fx"], dev["fu"], dev["fc"], *res[0],
                                                     C.byref(its[0])))

    def kl_own():
        for _ in range(a.inner_kl):
            _lib.check(L.ddp_user_ilqgkl_f64_dev(h.raw, up, N, B, dev["prm"], 1, C.byref(o), dev["xo"], dk["c1"], dev["K"], dev["u"], dk["Sp"],
                                                 dk["Sip"], None, 1, dk["R1"], dev["lims"], None, *res[1], C.byref(its[1])))
    try:
        kl_fit(); kf = (h.last_kernel(0), h.last_kernel(1)); kl_own(); ko = (h.last_kernel(0), h.last_kernel(1)); h.sync()
        st = [h.to_host(r_[9], (12, B))[0].astype(int) for r_ in res]
        print("%s (e) iLQGkl(fitted, wide) and iLQGkl(wide): kernels %s and %s, %d and %d batch iterations, statuses %s and %s"
              % (tag, kf, ko, its[0].value, its[1].value, *[dict(zip(*[v.tolist() for v in np.unique(s_, return_counts=True)])) for s_ in st]),
              flush=True)
        t1, t2 = [], []
        for _ in range(a.repeats):
            t1.append(b.timed(kl_fit) / a.inner_kl)
            t2.append(b.timed(kl_own) / a.inner_kl)
    finally:
        h.set_kl_wide(was)
    print("%s (e1) ddp_user_ilqgkl_fit per solve on the tables (%d solves per window): %s" % (tag, a.inner_kl, spread(t1)), flush=True)
    print("%s (e2) ddp_user_ilqgkl per solve on the problem's own model: %s" % (tag, spread(t2)), flush=True)
    print("%s (e) per batch iteration %.2f ms on the tables, %.2f ms on the own model; (e1) over (e2) %.2fx the time (medians)"
          % (tag, float(np.median(t1)) / max(its[0].value, 1), float(np.median(t2)) / max(its[1].value, 1),
             float(np.median(t1)) / float(np.median(t2))), flush=True)
    for p in list(dev.values()) + list(dk.values()) + out[0] + out[1] + res[0] + res[1]:
        h.free(p)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="64x32x64,34x17x128", help="n x m x B, comma separated")
    ap.add_argument("--N", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--inner-kl", type=int, default=2, dest="inner_kl", help="0: no whole solves")
    a = ap.parse_args()
    if a.repeats < 3:
        raise SystemExit("--repeats: three runs at least (the spread is part of the result)")
    torch = get_torch()
    b = Bench()
    import ddp_amd.kl  # noqa: F401
    for s in a.shapes.split(","):
        n, m, B = (int(v) for v in s.split("x"))
        shape(b, a, n, m, B, torch)


if __name__ == "__main__":
    main()
