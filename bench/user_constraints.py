"""DDP_USER_CONSTRAINTS: B keep-out cars (user_examples/car_keepout_ad.hip, N steps), with and without control limits, timed with HIP
events on the handle's stream, in one process on one box:
  (a) the device loop: ONE call of ddp_user_ilqg_al_f64_dev (operands and results stay on the device);
  (b) the host loop a user can write from the pieces: iLQG(..., multipliers=) per round, constraints(), the update in NumPy, the same
      rounds and the same freezing rule — its results are compared with (a)'s;
  (c) the plain car_ad solve (the soft obstacle cost in place of the constraints) next to one round of the constrained solve: the cost
      of the constraint terms per inner iteration, and the shares of the derivative, backward and forward phases of that round.
One line per measurement (append to profiles/user_constraints.txt).

    python bench/user_constraints.py [--B 4096] [--N 150] [--repeats 3]
"""
import argparse
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def keepout_inputs(rng, B, N):
    """[h, gx, gy, ox, oy, r, wo, wu, wt, vmax]: the disc half way to the goal and a little to one side, the goal further than the cap allows
    at the mean speed (tests/constraints_cases.py draws the same family)"""
    h = 0.1
    p = np.zeros((10, B))
    p[0] = h
    p[1] = 1.2 * h * N + 0.1 * rng.standard_normal(B)
    p[2] = 0.05 * rng.standard_normal(B)
    p[3] = 0.5 * p[1] + 0.05 * rng.standard_normal(B)
    p[4] = rng.choice([-1.0, 1.0], B) * rng.uniform(0.05, 0.15, B)
    p[5] = rng.uniform(0.3, 0.4, B)
    p[7], p[8] = 0.1, 10.0
    p[9] = rng.uniform(1.3, 1.4, B)
    x0 = np.zeros((4, B)); x0[3] = 1.0 + 0.05 * rng.standard_normal(B)
    return p, x0, 0.01 * rng.standard_normal((2, N, B))


class Events:
    def __init__(self, h, L, check):
        self.h, self.L, self.check = h, L, check
        self.ev0, self.ev1 = C.c_void_p(), C.c_void_p()
        check(L.ddp_event_create(h.raw, C.byref(self.ev0))); check(L.ddp_event_create(h.raw, C.byref(self.ev1)))

    def timed(self, fn):
        h, L = self.h, self.L
        h.sync()
        L.ddp_event_record(h.raw, self.ev0)
        fn()
        L.ddp_event_record(h.raw, self.ev1)
        h.sync()
        ms = C.c_float()
        self.check(L.ddp_event_elapsed_ms(h.raw, self.ev0, self.ev1, C.byref(ms)))
        return ms.value


def counts(v):
    return dict(zip(*[a.tolist() for a in np.unique(np.asarray(v).astype(int), return_counts=True)]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=4096)
    ap.add_argument("--N", type=int, default=150)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--max-outer", type=int, default=20)
    a = ap.parse_args()
    import warnings
    warnings.simplefilter("ignore")                           # (trace_cap = 1: the history rows are not kept, and iLQG says so)
    import ddp_amd as ddp
    from ddp_amd import _lib
    L, h = _lib.lib(), ddp.default_handle()
    ev = Events(h, L, _lib.check)
    B, N, n, m, nc = a.B, a.N, 4, 2, 2
    p, x0, u0 = keepout_inputs(np.random.default_rng(11), B, N)
    prob = ddp.DeviceProblem(ddp.example_source("car_keepout_ad"), n, m, nparam=10, terminal=True, autodiff=True, constraints=nc)
    up = prob._ptr(h)
    oc = ddp._ilqg_opts(ddp.DEFAULT_ALPHA, 1e-7, 1e-4, 500, 1.0, 1.0, 1.6, 1e10, 1e-6, 1, 0.0)
    ao = _lib.ALOpts(1.0, 10.0, 1e8, 1e-5, a.max_outer)
    dp, dx0, du0 = h.to_device(p), h.to_device(x0), h.to_device(u0)
    sizes = (n * N, m * N, m * n * N, m * N, m * m * N, n * N, n * n * N, N + 1, 8, nc * N, 1, nc * N, 6)
    outs = [h.malloc(8 * s * B) for s in sizes]
    git = C.c_int(0)
    for tag, lims in (("no limits", None), ("lims [-1, 1] x [-1.5, 1.5]", np.array([[-1.0, 1.0], [-1.5, 1.5]]))):
        dl = h.to_device(lims) if lims is not None else None

        def run_dev():
            _lib.check(L.ddp_user_ilqg_al_f64_dev(h.raw, up, N, B, dp, 1, C.byref(oc), C.byref(ao), dx0, 0, du0, dl, None, None, *outs,
                                                  C.byref(git)))
        run_dev()                                               # warm-up (compile, scratch)
        td = [ev.timed(run_dev) for _ in range(a.repeats)]
        xd, ud = h.to_host(outs[0], (n, N, B)), h.to_host(outs[1], (m, N, B))
        als = h.to_host(outs[12], (6, B))
        rounds = int(als[1].max())
        print("device loop (%s): B=%d N=%d: ms %s; %d rounds at most (median %d), %d batch iterations in all, AL statuses %s, cviol max %.3g"
              % (tag, B, N, " ".join("%.1f" % t for t in td), rounds, np.median(als[1]), git.value, counts(als[0]), als[4].max()), flush=True)

        res = {}

        def run_host():
            lam, mu = np.zeros((nc, N, B)), np.ones(B)
            live = np.ones(B, dtype=bool)
            x = u = None
            its = 0
            for r in range(rounds):
                o = ddp.iLQG(prob, x0 if r == 0 else x, u0 if r == 0 else u, params=p, multipliers=(lam, mu), lims=lims, timing=False,
                             trace_cap=1)
                its += o[6]["global_iters"]
                if r == 0:
                    x, u = o[0].copy(), o[1].copy()
                else:
                    x[..., live], u[..., live] = o[0][..., live], o[1][..., live]
                g = ddp.constraints(prob, x, u, params=p)
                viol = np.maximum(0.0, g.max(axis=(0, 1)))
                go = live & (viol > 1e-5) & (r + 1 < rounds)
                lam[..., go] = np.maximum(0.0, lam[..., go] + mu[go] * g[..., go])
                mu[go] = np.minimum(10.0 * mu[go], 1e8)
                live = go
                if not live.any():
                    break
            res.update(x=x, u=u, its=its)
        run_host()
        th = [ev.timed(run_host) for _ in range(a.repeats)]
        err = max(float(np.abs(res["x"] - xd).max() / np.abs(xd).max()), float(np.abs(res["u"] - ud).max() / max(np.abs(ud).max(), 1e-300)))
        print("host loop of iLQG(multipliers=) calls + NumPy update (%s): ms %s; %d batch iterations in all; x, u differ from the device "
              "loop's by %.3g (relative, max); device loop %.2fx the speed of the host loop"
              % (tag, " ".join("%.1f" % t for t in th), res["its"], err, float(np.median(th)) / float(np.median(td))), flush=True)
        if dl is not None:
            h.free(dl)

    # ---- (c) the plain car_ad solve next to round 0 of the constrained one
    car = ddp.DeviceProblem(ddp.example_source("car_ad"), n, m, nparam=9, terminal=True, autodiff=True)
    ps = p[:9].copy(); ps[6] = 10.0                            # the soft obstacle cost in place of the disc
    lam, mu = np.zeros((nc, N, B)), np.ones(B)
    for label, fn in (("plain car_ad (soft obstacle cost)", lambda **k: ddp.iLQG(car, x0, u0, params=ps, **k)),
                      ("car_keepout_ad round 0 (mu = 1)", lambda **k: ddp.iLQG(prob, x0, u0, params=p, multipliers=(lam, mu), **k))):
        fn(timing=False, trace_cap=1)
        box = {}
        ts = [ev.timed(lambda: box.update(o=fn(timing=False, trace_cap=1))) for _ in range(a.repeats)]
        gi = box["o"][6]["global_iters"]
        tr = fn(timing=True, trace_cap=1)[6]
        ph = [float(np.nansum(tr[k])) for k in ("time_derivs", "time_backward", "time_forward")]
        print("%s: ms %s; %d batch iterations, %.3f ms per batch iteration; phases of a timed run: derivatives %.1f%%, backward %.1f%%, "
              "forward %.1f%% of %.1f ms on the device" % (label, " ".join("%.1f" % t for t in ts), gi, float(np.median(ts)) / gi,
                                                          *(100 * v / sum(ph) for v in ph), 1e3 * sum(ph)), flush=True)


if __name__ == "__main__":
    main()
