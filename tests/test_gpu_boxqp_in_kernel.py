"""Every in-kernel box-QP of the backward pass on the designed QPs of tests/boxqp_designed_cases.py, against the long-double reference
(which tests/test_boxqp_designed_cpu.py certifies by KKT conditions, brute force and the C oracle without a GPU).

Each group is a (kernel family, n, m); each of its calls is one back_pass with fu = 0 and a time-varying cost, so that step i solves
the QP the table chose: boxqp1_two_iterations / boxqp_dev1 (q4), boxqp_dev1 / boxqp_dev2 (dpp, row, mxg), the generic loop (row, mxg,
mid, general, big), bqr::boxqp_rows (mid with m > 4, mf2, mfma) and boxqp_wave (wide).  The table's margins make every decision of the
solver decisive, so there is no allowance for trajectories that part from the reference: the number allowed is zero."""
import os

import numpy as np
import pytest

from boxqp_designed_cases import FAMILIES, GROUPS, call_names, case, reference
from conftest import relerr
from test_gpu_forward_contract import handle  # noqa: F401  (fixture: the default handle with every DDP_* switch cleared)

pytestmark = pytest.mark.gpu
RTOL = 1e-8
NAMES = ("K", "k", "Quu", "Vx", "Vxx", "dV")


def _host(c, force):
    """ddp.back_pass of the case with DDP_BACKPASS forced as _run of tests/test_gpu_row_shapes.py does (the `handle` fixture has cleared
    every kernel switch); the environment is restored afterwards"""
    import ddp_amd
    from ddp_amd import _lib
    if force:
        os.environ["DDP_BACKPASS"] = force
    try:
        div, pol, Vx, Vxx, dV = ddp_amd.back_pass(c["cx"], c["cu"], c["cxx"], c["cxu"], c["cuu"], c["fx"], c["fu"], c["lam"], c["regType"],
                                                  c["lims"], c["x"], c["u"])
        name = _lib.default_handle().last_kernel(0)
    finally:
        os.environ.pop("DDP_BACKPASS", None)
        _lib.default_handle().raw
    return dict(K=pol.K, k=pol.k, Quu=pol.Σi, Vx=Vx, Vxx=Vxx, dV=dV, diverge=np.asarray(div), kernel=name)


def _dev(h, c):
    from test_gpu_wide_controls import BPOnDevice
    with BPOnDevice(h, c) as dev:
        return dev.run(c["regType"])


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


@pytest.mark.parametrize("family,n,m", GROUPS)
def test_in_kernel_boxqp_on_designed_qps(handle, family, n, m):
    how, force, kernel = FAMILIES[family]
    worst, q12_rows, clamped_entries, qps = {}, 0, 0, 0
    for name in call_names(m):
        c, ref = case(family, n, m, name), reference(family, n, m, name)
        out = _host(c, force) if how == "host" else _dev(handle, c)
        what = (family, n, m, name)
        assert out["kernel"] == kernel, (what, out["kernel"])
        assert not out["diverge"].any() and not ref["diverge"].any(), (what, out["diverge"])
        assert np.array_equal(out["Vxx"], np.transpose(out["Vxx"], (1, 0, 2, 3))), what
        dist = {key: max(relerr(out[key][..., b], ref[key][..., b]) for b in range(c["B"])) for key in NAMES}
        for key, v in dist.items():
            worst[key] = max(worst.get(key, 0.0), v)
        print("%s (%d, %d) %s:" % what, " ".join("%s %.3g" % kv for kv in sorted(dist.items())))
        for b in range(c["B"]):
            for key in NAMES:                                           # every trajectory: none may part from the reference
                e = relerr(out[key][..., b], ref[key][..., b])
                assert e < RTOL, (what, b, key, e)
            for i, q in ref["qps"][b].items():
                qps += 1
                x = np.asarray(q["x"], float)
                on = (x == q["lo"]) | (x == q["up"])                    # the reference's k_i sits on the float64 bound lims - u
                bound = np.where(x == q["lo"], c["lims"][:, 0] - c["u"][:, i, b], c["lims"][:, 1] - c["u"][:, i, b])
                assert np.array_equal(_bits(out["k"][on, i, b]), _bits(bound[on])), (what, b, i, "k is not bit-equal to lims - u")
                clamped_entries += int(on.sum())
                rows = out["K"][:, :, i, b]
                assert not rows[~q["free"]].any(), (what, b, i, "K row of a clamped coordinate is not zero")
                left_free = on & q["free"] & (q["lo"] < q["up"])       # Q12: on its bound, free in the returned set
                if q["result"] == 4 and left_free.any():
                    assert rows[left_free].any(axis=1).all(), (what, b, i, "K row zero where exit 4 returns the previous free set")
                    q12_rows += int(left_free.sum())
    assert q12_rows > 0 and clamped_entries > 0
    print("%s (%d, %d) %s: %d QPs, %d entries of k bit-equal to a bound, %d Q12 rows; worst distances:" % (family, n, m, kernel, qps, clamped_entries, q12_rows),
          " ".join("%s %.3g" % kv for kv in sorted(worst.items())))
