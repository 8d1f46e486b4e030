"""The two kernels behind ddp_boxqp_f64[_dev] — boxqp_kernel<1..8> (csrc/capi.hip, one lane per problem) and boxqp_big_kernel
(csrc/boxqp_big.hip, one work-group per problem, 8 < m <= DDP_QP_MAX_M = 1024) — on the designed problems of
tests/boxqp_standalone_cases.py against the long-double reference, which tests/test_boxqp_standalone_cpu.py certifies without a GPU.
The table's margins make every decision of the solver decisive and float64 takes the reference's path on every problem, so no problem
is skipped or excused.  m >= 744 needs more than 64 KB of dynamic LDS (88 m + 80 bytes): those launches take the raised limit.

ddp_last_kernel has no slot for boxQP (0 .. 6 are the backward, forward, derivative, cost, plant, covariance and KL kernels), so no
kernel name is asserted; which kernel runs is fixed by m alone (m <= DDP_MAX_M = 8: boxqp_kernel<m>)."""
import ctypes as C

import numpy as np
import pytest

from boxqp_standalone_cases import M_BIG, M_SMALL, batch_opts, big_batches, compare, small_batches, small_qps, stack
from test_gpu_forward_contract import SENT, handle  # noqa: F401  (fixture: the default handle with every DDP_* switch cleared)

pytestmark = pytest.mark.gpu
GUARD = 512                                    # bytes of sentinel behind every output buffer


def _launch(problems):
    """one call of the host-pointer entry on the problems as a batch: x [m,c], result [c], Hfree [m,m,c], free [m,c]"""
    import ddp_amd
    return ddp_amd.boxQP(*stack(problems), **batch_opts(problems))


def _bytes(out):
    x, res, Hf, free = out
    per_problem = (np.asarray(x).T, np.asarray(res), np.asarray(Hf).transpose(2, 0, 1), np.asarray(free).T)
    return [np.ascontiguousarray(a).reshape(len(a), -1).view(np.uint8) for a in per_problem]


def _same_bits(a, b, order=None):
    """the four outputs of two calls, problem by problem (order: problem c of `a` is problem order[c] of `b`)"""
    for u, v in zip(_bytes(a), _bytes(b)):
        if not np.array_equal(u, v if order is None else v[order]):
            return False
    return True


@pytest.mark.parametrize("m", M_SMALL)
def test_small_m_on_the_replayed_qps(handle, m):
    """boxqp_kernel<m>: batches of 1, 63, 64, 65 problems and the whole list (a partly filled last wave among them)"""
    wx, wh, n = 0.0, 0.0, 0
    for name, ps in small_batches(m).items():
        dx, dh = compare(ps, *_launch(ps), where=(m, name))
        wx, wh, n = max(wx, dx), max(wh, dh), n + len(ps)
    print("m = %d boxqp_kernel<%d>: %d problems in 5 launches, worst distances: x %.3g Hfree %.3g" % (m, m, n, wx, wh))


@pytest.mark.parametrize("m", M_BIG)
def test_large_m_on_the_designed_batches(handle, m):
    """boxqp_big_kernel: every launch of the table — default options, the lost pivots, each option set"""
    wx, wh, n = 0.0, 0.0, 0
    B = big_batches(m)
    for name, ps in B.items():
        dx, dh = compare(ps, *_launch(ps), where=(m, name))
        wx, wh, n = max(wx, dx), max(wh, dh), n + len(ps)
    print("m = %d boxqp_big_kernel: %d problems in %d launches, worst distances: x %.3g Hfree %.3g" % (m, n, len(B), wx, wh))


def _independence_batch(m):
    if m <= 8:
        return small_qps(m)[:130]                                   # three waves, the last one partly filled
    B = big_batches(m)
    return B["main0"] + (B["pivot"] if m <= 257 else [])            # at most 6 problems at the largest m


@pytest.mark.parametrize("m", [8, 65, 257, 1024])
def test_a_problem_does_not_depend_on_its_batch(handle, m):
    """the sums of both kernels have a fixed order and a lane or work-group sees its own problem only: the batch in another order, each
    problem alone and the same call again give the same bits"""
    ps = _independence_batch(m)
    first = _launch(ps)
    compare(ps, *first, where=(m, "batch"))
    assert _same_bits(_launch(ps), first), (m, "the same call twice")
    order = np.random.default_rng(m).permutation(len(ps))
    assert _same_bits(_launch([ps[i] for i in order]), first, order), (m, "permuted batch")
    for c in (range(len(ps)) if m > 8 else (0, 63, 64, 129)):
        assert _same_bits(_launch([ps[c]]), first, [c]), (m, "problem %d alone" % c)


class _Outputs:
    """the four outputs of ddp_boxqp_f64_dev in device buffers filled with a NaN sentinel each, a guard run of the sentinel behind"""

    def __init__(self, h, m, count):
        self.h, self.m, self.count = h, m, count
        self.nbytes = [8 * m * count, 4 * count, 8 * m * m * count, m * count]                      # x, result, Hfree, free
        self.total = [(nb + 7) // 8 * 8 + GUARD for nb in self.nbytes]
        self.bufs = []

    def __enter__(self):
        from ddp_amd import _lib
        for i, tot in enumerate(self.total):
            p = self.h.malloc(tot)
            self.bufs.append(p)
            fill = np.full(tot // 8, SENT[i], np.uint64)
            _lib.check(_lib.lib().ddp_memcpy_h2d(self.h.raw, p, fill.ctypes.data_as(C.c_void_p), C.c_size_t(fill.nbytes)))
        return self

    def __exit__(self, *exc):
        for p in self.bufs:
            self.h.free(p)

    def read(self):
        """(x, result, Hfree, free) as boxQP returns them, and per buffer whether everything behind its last element kept its bits"""
        m, c = self.m, self.count
        raw = [self.h.to_host(p, (tot,), np.uint8) for p, tot in zip(self.bufs, self.total)]
        kept = [bool(np.all(r[nb:] == np.full(tot // 8, SENT[i], np.uint64).view(np.uint8)[nb:]))
                for i, (r, nb, tot) in enumerate(zip(raw, self.nbytes, self.total))]
        x = raw[0][:self.nbytes[0]].view(np.float64).reshape((m, c), order="F")
        res = raw[1][:self.nbytes[1]].view(np.int32)
        Hf = raw[2][:self.nbytes[2]].view(np.float64).reshape((m, m, c), order="F")
        free = raw[3][:self.nbytes[3]].reshape((m, c), order="F")
        return (x, res, Hf, free), kept


@pytest.mark.parametrize("m,count", [(5, 65), (8, 1), (17, 5), (257, 3), (1024, 2)])
def test_device_entry_writes_every_output_and_nothing_else(handle, m, count):
    """ddp_boxqp_f64_dev on device buffers pre-filled with NaN sentinels: every element of x, result, Hfree and free is written (Hfree's
    zeros by the kernel), the sentinels behind each buffer keep their bits (the t >= count tail of a partly filled wave, the last
    work-group), and the values are the host entry's bit for bit"""
    from ddp_amd import _lib
    ps = small_qps(m)[:count] if m <= 8 else big_batches(m)["main0"][:count]
    host = _launch(ps)
    ins = [handle.to_device(a) for a in stack(ps)]
    try:
        with _Outputs(handle, m, count) as out:
            _lib.check(_lib.lib().ddp_boxqp_f64_dev(handle.raw, C.c_int(m), C.c_int(count), *ins, None, *out.bufs))
            handle.sync()
            dev, kept = out.read()
    finally:
        for p in ins:
            handle.free(p)
    assert all(kept), (m, count, "written behind the end of", [n for n, k in zip(("x", "result", "Hfree", "free"), kept) if not k])
    assert np.isfinite(dev[0]).all() and np.isfinite(dev[2]).all() and set(np.unique(dev[3]).tolist()) <= {0, 1}, (m, count, "an element was left unwritten")
    assert set(np.unique(dev[1]).tolist()) <= {4, 5, 6}, np.unique(dev[1])
    compare(ps, dev[0], dev[1], dev[2], dev[3].astype(bool), where=(m, "device entry"))
    assert _same_bits((dev[0], dev[1], dev[2], dev[3].astype(bool)), host), (m, count, "device entry and host entry differ")
