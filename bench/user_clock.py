"""DDP_USER_CLOCK: a closed loop that follows a moving reference, timed with HIP events on the handle's stream.
  (a) the clocked device loop: B cars of user_examples/car_track.hip (N = 50) for `steps` closed-loop steps in ONE call of
      ddp_user_ilqg_mpc_f64_dev, the clock of every trajectory advanced on the device;
  (b) the host loop that does the same job without the flag (the only way before it): the unclocked twin of the model (t replaced by
      i), one ddp_user_ilqg_f64_dev call per closed-loop step, the sampled paths in the parameters shifted by one step, x_1 taken as the
      next start and the plan shifted between the calls (operands stay on the device; the shifted parameters are uploaded per step);
  (c) --ab OTHER_LIB: what the clock costs a problem WITHOUT the flag — the closed loop of user_examples/car_plant.hip (model as
      plant, as bench/user_sched.py) in fresh child processes that alternate between this build of the library and OTHER_LIB
      (a build of the commit before the flag), --rounds times each; the spread of either build's own repeats is printed next to
      the difference of the medians.
One line per measurement (append to profiles/user_clock.txt).

    python bench/user_clock.py [--B 1024] [--N 50] [--steps 100] [--repeats 3] [--ab OTHER_LIB --rounds 4]
"""
import argparse
import ctypes as C
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def track_params(rng, B, L):
    """[h, r, wo, wu, wp, wt, L, ref(2, L), obs(2, L)] of user_examples/car_track.hip, one column per trajectory"""
    s = np.arange(L)
    P = np.zeros((7 + 4 * L, B))
    P[0], P[1], P[2], P[3], P[4], P[5], P[6] = 0.1, 0.6 + 0.1 * rng.random(B), 2.0 + rng.random(B), 0.05, 1.0 + rng.random(B), 5.0, L
    ph = rng.random((2, B))
    ref = np.stack([0.12 * s[:, None] + 0.3 * rng.standard_normal(B), 0.8 * np.sin(0.11 * s[:, None] + ph[0])])        # [2, L, B]
    obs = np.stack([4.0 - 0.05 * s[:, None] + 0.2 * rng.standard_normal(B), 0.9 * np.cos(0.07 * s[:, None] + ph[1])])
    P[7:7 + 2 * L] = ref.reshape(2 * L, B, order="F")
    P[7 + 2 * L:] = obs.reshape(2 * L, B, order="F")
    return P


def twin_source(src, N):
    """car_track.hip without the clock: the old signatures, the paths read at min(i, L-1) (terminal_cost: at N-1)"""
    s = src.replace("int i, int t, ", "int i, ").replace("const double *x, int t, const double *p)", "const double *x, const double *p)")
    a = s.index("double terminal_cost(")
    b = s.index("\n}\n", a)
    s = s[:a] + s[a:b].replace("track_k(t, p)", "track_k(%d, p)" % (N - 1)) + s[b:]
    return s.replace("track_k(t, p)", "track_k(i, p)")


def shifted(P, c, L):
    idx = np.minimum(np.arange(L) + c, L - 1)
    Q = P.copy()
    for off in (7, 7 + 2 * L):
        Q[off:off + 2 * L] = P[off:off + 2 * L].reshape(2, L, -1, order="F")[:, idx].reshape(2 * L, -1, order="F")
    return Q


def car_plant_params(rng, B):
    """[h, gx, gy, ox, oy, r, wo, wu, wt, ga, gw, vx, vy] of user_examples/car_plant.hip (bench/user_sched.py)"""
    P = np.empty((13, B))
    P[0] = 0.05
    P[1:3] = 4.0 + rng.uniform(-0.5, 0.5, (2, B))
    P[3:5] = 2.0 + rng.uniform(-0.3, 0.3, (2, B))
    P[5] = 0.6 + rng.uniform(0, 0.3, B); P[6] = rng.uniform(5.0, 20.0, B)
    P[7] = 0.1; P[8] = rng.uniform(5.0, 20.0, B)
    P[9] = rng.uniform(0.6, 0.9, B); P[10] = rng.uniform(1.1, 1.4, B)
    P[11:13] = rng.uniform(-0.5, 0.5, (2, B))
    return P


class Bench:
    def __init__(self):
        import ddp_amd as ddp
        from ddp_amd import _lib
        self.ddp, self._lib, self.L, self.h = ddp, _lib, _lib.lib(), ddp.default_handle()
        self.ev0, self.ev1 = C.c_void_p(), C.c_void_p()
        _lib.check(self.L.ddp_event_create(self.h.raw, C.byref(self.ev0))); _lib.check(self.L.ddp_event_create(self.h.raw, C.byref(self.ev1)))

    def timed(self, fn):
        """ms of fn() between two events on the handle's stream (the entry points synchronise themselves)"""
        h, L = self.h, self.L
        h.sync()
        L.ddp_event_record(h.raw, self.ev0)
        fn()
        L.ddp_event_record(h.raw, self.ev1)
        h.sync()
        ms = C.c_float()
        self._lib.check(L.ddp_event_elapsed_ms(h.raw, self.ev0, self.ev1, C.byref(ms)))
        return ms.value


def statuses(st):
    return dict(zip(*[v.tolist() for v in np.unique(st.astype(int), return_counts=True)]))


def unclocked(a):
    """(c), one process: the closed loop of an unclocked problem, `repeats` timed calls after a warm-up"""
    b = Bench()
    ddp, _lib, L, h = b.ddp, b._lib, b.L, b.h
    B, T, steps, n, m = a.B, a.N, a.steps, 4, 2
    rng = np.random.default_rng(7)
    prm = car_plant_params(rng, B)
    x0 = np.zeros((n, B)); x0[:2] = rng.uniform(0, 0.5, (2, B)); x0[2] = np.pi / 4 + rng.uniform(-0.2, 0.2, B)
    u0 = 0.1 * rng.standard_normal((m, T, B))
    oc = ddp._ilqg_opts(ddp.DEFAULT_ALPHA, 1e-7, 1e-4, 100, 1.0, 1.0, 1.6, 1e10, 1e-6, 1, 0.0)
    dprm, dx0, du0 = h.to_device(prm), h.to_device(x0), h.to_device(u0)
    dl = h.to_device(np.array([[-2.0, 2.0], [-1.5, 1.5]]))
    xcl, ucl, scl = h.malloc(8 * n * (steps + 1) * B), h.malloc(8 * m * steps * B), h.malloc(8 * 8 * steps * B)
    xp, upl = h.malloc(8 * n * T * B), h.malloc(8 * m * T * B)
    car = ddp.DeviceProblem(ddp.example_source("car_plant"), n, m, nparam=13, terminal=True)
    upc = car._ptr(h)
    git = C.c_int(0)
    run = lambda: _lib.check(L.ddp_user_ilqg_mpc_f64_dev(h.raw, upc, T, B, dprm, 1, C.byref(oc), steps, 0, dx0, du0, dl, xcl, ucl, scl, xp,
                                                         upl, C.byref(git)))
    run()
    ts = [b.timed(run) for _ in range(a.repeats)]
    st = h.to_host(scl, (8, steps, B))
    digest = float(np.abs(h.to_host(xcl, (n, steps + 1, B))).sum())
    print("unclocked car mpc (%s): B=%d N=%d steps=%d: ms %s, %d global iterations, statuses %s, sum|xcl| %.17g"
          % (a.label, B, T, steps, " ".join("%.1f" % t for t in ts), git.value, statuses(st[0]), digest), flush=True)


def ab(a):
    """(c): child processes alternating between this build and --ab OTHER_LIB"""
    import re
    this = os.path.join(ROOT, "differentialdynamicprogramming.jl_amd", "libddp_amd.so")
    res = {"this": [], "other": []}
    digests = {}
    for r in range(a.rounds):
        for label, lib in (("this", this), ("other", a.ab)):
            env = dict(os.environ, DDP_AMD_LIB=lib)
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--mode", "unclocked", "--label", label, "--B", str(a.B), "--N",
                                  str(a.N), "--steps", str(a.steps), "--repeats", str(a.repeats)], env=env, capture_output=True, text=True,
                                 timeout=600)
            if out.returncode != 0:
                print(out.stdout + out.stderr[-2000:])
                raise SystemExit("child failed (%s, exit status %d): nothing more is started" % (label, out.returncode))
            line = out.stdout.strip().splitlines()[-1]
            print(line, flush=True)
            res[label] += [float(v) for v in re.search(r": ms ([\d. ]+),", line).group(1).split()]
            digests.setdefault(label, set()).add(re.search(r"sum\|xcl\| (\S+)", line).group(1))
    med = {k: float(np.median(v)) for k, v in res.items()}
    spread = {k: (min(v), max(v)) for k, v in res.items()}
    print("unclocked A/B: this build median %.1f ms (min %.1f max %.1f, %d runs); build before the flag median %.1f ms (min %.1f max %.1f); "
          "difference of medians %+.2f%%; run-to-run spread this %.2f%% other %.2f%%; same closed loop %s"
          % (med["this"], *spread["this"], len(res["this"]), med["other"], *spread["other"], 100 * (med["this"] / med["other"] - 1),
             100 * (spread["this"][1] - spread["this"][0]) / med["this"], 100 * (spread["other"][1] - spread["other"][0]) / med["other"],
             digests["this"] == digests["other"] and len(digests["this"]) == 1))


def clocked(a):
    """(a) and (b)"""
    b = Bench()
    ddp, _lib, L, h = b.ddp, b._lib, b.L, b.h
    B, N, steps, n, m = a.B, a.N, a.steps, 4, 2
    Ls = N + steps                                              # samples: every step any solve of the loop reads
    rng = np.random.default_rng(21)
    prm = track_params(rng, B, Ls)
    x0 = np.stack([prm[7] + 0.2 * rng.standard_normal(B), prm[8] + 0.2 * rng.standard_normal(B), 0.3 + 0.1 * rng.standard_normal(B),
                   0.8 + 0.1 * rng.standard_normal(B)])
    u0 = 0.1 * rng.standard_normal((m, N, B))
    t0 = np.zeros(B, dtype=np.int32)
    oc = ddp._ilqg_opts(ddp.DEFAULT_ALPHA, 1e-7, 1e-4, 100, 1.0, 1.0, 1.6, 1e10, 1e-6, 1, 0.0)
    dprm, dx0, du0 = h.to_device(prm), h.to_device(x0), h.to_device(u0)
    dl = h.to_device(np.array([[-2.0, 2.0], [-1.5, 1.5]]))
    xcl, ucl, scl = h.malloc(8 * n * (steps + 1) * B), h.malloc(8 * m * steps * B), h.malloc(8 * 8 * steps * B)
    xp, upl = h.malloc(8 * n * N * B), h.malloc(8 * m * N * B)
    src = ddp.example_source("car_track")
    car = ddp.DeviceProblem(src, n, m, nparam=prm.shape[0], terminal=True, clock=True)
    upc = car._ptr(h)
    git = C.c_int(0)

    def run_dev():
        _lib.check(L.ddp_user_set_t0(upc, t0.ctypes.data_as(C.c_void_p), B))
        _lib.check(L.ddp_user_ilqg_mpc_f64_dev(h.raw, upc, N, B, dprm, 1, C.byref(oc), steps, 0, dx0, du0, dl, xcl, ucl, scl, xp, upl,
                                               C.byref(git)))
    run_dev()                                                   # warm-up (compile, scratch)
    td = [b.timed(run_dev) for _ in range(a.repeats)]
    st = h.to_host(scl, (8, steps, B))
    xcl_dev = h.to_host(xcl, (n, steps + 1, B))
    print("clocked car mpc on the device: B=%d N=%d steps=%d: ms %s, %.2f ms per closed-loop step, %d global iterations, iterations per "
          "solve median %d max %d, statuses %s" % (B, N, steps, " ".join("%.1f" % t for t in td), float(np.median(td)) / steps, git.value,
                                                   np.median(st[1]), st[1].max(), statuses(st[0])), flush=True)

    # ---- (b) the host loop on the unclocked twin
    twin = ddp.DeviceProblem(twin_source(src, N), n, m, nparam=prm.shape[0], terminal=True)
    upt = twin._ptr(h)
    outs = [h.malloc(8 * s * B) for s in (n * N, m * N, m * n * N, m * N, m * m * N, n * N, n * n * N, N + 1, 8)]
    dxs, dus, dps = h.malloc(8 * n * B), h.malloc(8 * m * N * B), h.malloc(8 * prm.size)
    xcl_host = np.zeros((n, steps + 1, B))
    its = []

    def run_host():
        its.clear()
        _lib.check(L.ddp_memcpy_h2d(h.raw, dxs, np.asfortranarray(x0).ctypes.data_as(C.c_void_p), C.c_size_t(8 * n * B)))
        _lib.check(L.ddp_memcpy_h2d(h.raw, dus, np.asfortranarray(u0).ctypes.data_as(C.c_void_p), C.c_size_t(8 * m * N * B)))
        xcl_host[:, 0] = x0
        for s in range(steps):
            ps = np.asfortranarray(shifted(prm, s, Ls))
            _lib.check(L.ddp_memcpy_h2d(h.raw, dps, ps.ctypes.data_as(C.c_void_p), C.c_size_t(ps.nbytes)))
            _lib.check(L.ddp_user_ilqg_f64_dev(h.raw, upt, N, B, dps, 1, C.byref(oc), dxs, 0, dus, None, dl, *outs[:8], outs[8], 0, None,
                                               C.byref(git)))
            its.append(git.value)
            xs = h.to_host(outs[0], (n, N, B))[:, 1]              # x_1 of the plan: the next start (the model is the plant)
            xcl_host[:, s + 1] = xs
            _lib.check(L.ddp_memcpy_h2d(h.raw, dxs, np.asfortranarray(xs).ctypes.data_as(C.c_void_p), C.c_size_t(8 * n * B)))
            _lib.check(L.ddp_mpc_shift_f64_dev(h.raw, m, N, B, 1, 0, outs[1], dus))
    run_host()
    th = [b.timed(run_host) for _ in range(a.repeats)]
    err = float(np.abs(xcl_host - xcl_dev).max() / np.abs(xcl_dev).max())
    print("host loop of iLQG calls on the unclocked twin with shifted params: B=%d N=%d steps=%d: ms %s, %.2f ms per closed-loop step, "
          "%d global iterations in all" % (B, N, steps, " ".join("%.1f" % t for t in th), float(np.median(th)) / steps, sum(its)), flush=True)
    print("clocked device loop vs host loop: closed-loop states differ by %.3g (relative, max); device loop %.2fx the speed of the host loop"
          % (err, float(np.median(th)) / float(np.median(td))), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=1024)
    ap.add_argument("--N", type=int, default=50)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--mode", choices=("clocked", "unclocked"), default="clocked")
    ap.add_argument("--label", default="this")
    ap.add_argument("--ab", default=None, help="another build of libddp_amd.so (the commit before the flag) for the unclocked A/B")
    ap.add_argument("--rounds", type=int, default=4)
    a = ap.parse_args()
    if a.mode == "unclocked":
        return unclocked(a)
    clocked(a)
    if a.ab:
        ab(a)


if __name__ == "__main__":
    main()
