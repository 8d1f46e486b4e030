"""A/B of the record-stream reuse of the shared-LTI backward pass (csrc/back_pass_sh.hip) on the benchmark's own step, in ONE process:
two handles on the benchmark's stream, one created under DDP_SH_REUSE=0 and one with the default, each with the benchmark's workload
(bench.PassBench: config 2, B = 1024); timed regions of bench.py's step alternate between them.  Per region: ms per step, backward ms
(HIP events, as bench.py takes them), hits and misses.  Then the COLD figure: before every call one shared operand is changed in place
(a double of cxu flips between 0 and 1e-300), so that each call computes its stream — what a single iLQG solve, whose λ changes every
iteration, sees — again alternating between the handles.

    python profiles/ab_sh_reuse.py [--rounds 5] [--steps 200] [--batch 1024]"""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--cold-steps", type=int, default=100)
    args = ap.parse_args()
    import torch
    import bench
    from ddp_amd import _lib

    class Fixed(_lib.Handle):
        """a handle that keeps the switches it was created under (Handle.raw reads the environment again when it has changed)"""
        @property
        def raw(self):
            return self._h

    L = _lib.lib()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    stream = torch.cuda.current_stream(dev).cuda_stream
    os.environ["DDP_SH_REUSE"] = "0"
    h_off = Fixed(0, stream=stream)
    del os.environ["DDP_SH_REUSE"]
    h_on = Fixed(0, stream=stream)
    n, m, N, B = bench.N_STATE, bench.N_CTRL, 1000, args.batch
    legs = [("reuse=0", h_off, bench.PassBench(torch, dev, h_off, L, 0, n, m, N, B)), ("reuse=1", h_on, bench.PassBench(torch, dev, h_on, L, 0, n, m, N, B))]
    fence = torch.cuda.synchronize
    for _, _, pb in legs:                                   # preheat, as bench.py does
        pb.timed(1, 100, fence)
    print("warm: the benchmark's step, the same operands and λ in every call (n=%d m=%d N=%d B=%d, %d steps per region)" % (n, m, N, B, args.steps))
    for r in range(args.rounds):
        for tag, h, pb in legs:
            s0 = h.sh_reuse_stats()
            el, bp, fp = pb.timed(args.steps, args.warmup, fence)
            s1 = h.sh_reuse_stats()
            print("round %d %-8s %.4f ms/step  backward %.4f ms  forward %.4f ms  hits %d misses %d  kernel %s" %
                  (r, tag, 1e3 * el / args.steps, bp, fp, s1[0] - s0[0], s1[1] - s0[1], h.last_kernel(0)), flush=True)

    def cold_region(pb, h, steps):
        """the step with a changed operand in front of every call: cxu[0] alternates between 0 and 1e-300 (an 8-byte copy on the stream;
        the results do not move — 1e-300 vanishes against every term it meets — but the content comparison sees another operand)"""
        vals = [torch.tensor([1e-300], dtype=torch.float64, device=dev), torch.zeros(1, dtype=torch.float64, device=dev)]
        ev = [C.c_void_p() for _ in range(3)]
        for e in ev:
            _lib.check(L.ddp_event_create(h.raw, C.byref(e)))
        for i in range(10):
            pb.dcxu[:1].copy_(vals[i % 2]); pb.step()
        fence()
        t0 = time.perf_counter()
        for i in range(steps):
            pb.dcxu[:1].copy_(vals[i % 2])
            pb.step(ev if i == steps // 2 else None)
        fence()
        el = time.perf_counter() - t0
        ms = C.c_float(0)
        _lib.check(L.ddp_event_elapsed_ms(h.raw, ev[0], ev[1], C.byref(ms)))
        for e in ev:
            L.ddp_event_destroy(h.raw, e)
        pb.dcxu.zero_()
        return 1e3 * el / steps, ms.value

    print("cold: one shared operand changed in place before every call (%d steps per region)" % args.cold_steps)
    for r in range(args.rounds):
        for tag, h, pb in legs:
            s0 = h.sh_reuse_stats()
            per, bp = cold_region(pb, h, args.cold_steps)
            s1 = h.sh_reuse_stats()
            print("round %d %-8s %.4f ms/step  backward %.4f ms  hits %d misses %d" % (r, tag, per, bp, s1[0] - s0[0], s1[1] - s0[1]), flush=True)
    print("sh_timeouts: reuse=0 %d, reuse=1 %d" % (h_off.sh_timeouts(), h_on.sh_timeouts()))


if __name__ == "__main__":
    main()
