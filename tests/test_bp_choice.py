"""Which backward-pass kernel a call gets (csrc/back_pass.hip, bp_choose).  One table of calls pins every threshold edge, each family's
shapes, misaligned operands and each DDP_BACKPASS letter.  The CPU test asks the library's choice through its unlisted debug hook
(ddp_bp_choice, no GPU needed); the GPU test makes each call through ddp_back_pass_f64_dev and reads ddp_last_kernel(h, 0).
The operand strides bp_kargs (csrc/ddp_internal.h) computes for the kernels that take a BPKArgs are checked the same way, through
ddp_bp_strides; the families that keep an argument struct of their own compute theirs in their launchers."""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import ROOT

LIB = os.path.join(ROOT, "differentialdynamicprogramming.jl_amd", "libddp_amd.so")
IN, COST, OUT = 1, 2, 4                     # 16-byte aligned: cx, cu | cxx, cuu | K, k, Quu, Vx, Vxx
ALL = IN | COST | OUT
PER_TRAJ = {"SH_MIN_B": "1000000"}      # (10, 2) with shared operands below the shared-operand kernel's batch
N_STEPS = 16

MX, MX2, MXR, MXG = "back_pass_mx_kernel", "back_pass_mx2_kernel", "back_pass_mx_kernel<RT>", "back_pass_mxg_kernel"
DPP, DPPW, ROW, MID, Q4 = "back_pass_dpp_kernel", "back_pass_dppw_kernel", "back_pass_row_kernel", "back_pass_mid_kernel", "back_pass_q4"
GEN, SH, MF2, MFMA, BIG = "back_pass_kernel", "sh_back_kernel", "back_pass_mf2_kernel", "back_pass_mfma_kernel", "back_pass_big_kernel"


def row(n, m, B, want, ops="", lims=None, al=ALL, **env):
    """ops: F time-varying dynamics, C time-varying cost, f / c per-trajectory dynamics / cost; lims: None, "on" or "off" (has_lims with
    lims[1,1] > lims[1,2], "no limits" upstream); env: DDP_* switches by their name without the prefix"""
    return dict(n=n, m=m, B=B, want=want, ops=ops, lims=lims, al=al, env={("DDP_" + k): v for k, v in env.items()})


TABLE = [
    # (10, 2), shared LTI operands: the shared-operand kernel from B = 1 024, the tile kernels below
    row(10, 2, 512, MX2), row(10, 2, 1023, MX2), row(10, 2, 1024, SH), row(10, 2, 1025, SH), row(10, 2, 6144, SH),
    row(10, 2, 64, SH, SH_MIN_B="1"), row(10, 2, 8, SH, SH_MIN_B="1"),
    # (10, 2) per trajectory: mx2 up to 1 024, mx below 5 120, dpp, dppw from 6 144 (shared LTI only)
    *[row(10, 2, B, want, **PER_TRAJ) for B, want in ((511, MX2), (512, MX2), (513, MX2), (1023, MX2), (1024, MX2), (1025, MX),
                                                       (2048, MX), (2049, MX), (3072, MX), (3073, MX), (4096, MX), (4097, MX),
                                                       (5119, MX), (5120, DPP), (6143, DPP), (6144, DPPW))],
    row(10, 2, 512, MX, MX2="0", **PER_TRAJ), row(10, 2, 2048, MX2, MX2="1", **PER_TRAJ),
    row(10, 2, 5120, DPPW, DPPW="1", **PER_TRAJ), row(10, 2, 512, MX2, DPPW="1", **PER_TRAJ), row(10, 2, 6144, DPP, DPPW="0", **PER_TRAJ),
    row(10, 2, 512, MX2, "FCfc"), row(10, 2, 1025, MX, "FCfc"), row(10, 2, 5120, DPP, "FCfc"), row(10, 2, 6144, DPP, "FCfc"),
    row(10, 2, 6144, DPP, "f"),
    # (10, 2) with limits: the wide tile kernel up to 2 048, then dpp
    row(10, 2, 512, MXG, "FCfc", "on"), row(10, 2, 2048, MXG, "FCfc", "on"), row(10, 2, 2049, DPP, "FCfc", "on"), row(10, 2, 64, MXG, "", "off"),
    # (4, 1)
    row(4, 1, 64, Q4), row(4, 1, 64, Q4, "FC", "on"), row(4, 1, 6144, Q4), row(4, 1, 64, GEN, BACKPASS="g"), row(4, 1, 64, DPP, BACKPASS="dpp"),
    # n <= 10, m <= 2 without limits: tile with run-time sizes, then the wide tile, then the row kernel
    row(6, 2, 1024, MXR), row(6, 2, 1025, MXR), row(6, 2, 3072, MXR), row(6, 2, 3073, MXG), row(6, 2, 4096, MXG), row(6, 2, 4097, ROW),
    row(3, 2, 1024, MXR), row(3, 2, 1025, MXG), row(3, 2, 3072, MXG), row(3, 2, 3073, ROW), row(1, 1, 8, MXR, "FC"),
    # n <= 12, m <= 4 with and without limits
    row(8, 4, 3072, MXG), row(8, 4, 4096, MXG), row(8, 4, 4097, ROW), row(6, 3, 64, MXG, "Cc"),
    row(8, 4, 2048, MXG, "F", "on"), row(8, 4, 2049, ROW, "F", "on"), row(12, 3, 2048, MXG, "C", "on"), row(12, 3, 2049, ROW, "C", "on"),
    row(6, 2, 1023, MXG, "", "on"), row(6, 2, 1024, MXG, "", "on"), row(6, 2, 1025, ROW, "", "on"),
    row(3, 1, 511, MXG, "", "on"), row(3, 1, 512, MXG, "", "on"), row(3, 1, 513, ROW, "", "on"), row(4, 2, 2048, MXG, "", "off"),
    # padded row shapes
    row(13, 1, 64, ROW), row(14, 1, 64, ROW, "FC", "on"), row(11, 3, 4096, ROW, "", "on"), row(5, 3, 5000, ROW), row(12, 4, 64, MID),
    # 14 < n <= 32
    row(20, 3, 64, MID), row(32, 8, 8, MID, "FCfc", "on"), row(16, 5, 64, MID), row(20, 3, 64, GEN, BACKPASS="general"),
    row(20, 4, 8, BIG, BACKPASS="big"), row(21, 3, 8, GEN, BACKPASS="big"), row(6, 3, 8, GEN, BACKPASS="g"),
    # 32 < n <= 64; (64, 8) with every combination of a time-varying cost and limits
    row(40, 5, 8, MF2), row(33, 1, 8, MF2, "FC", "on"), row(63, 8, 8, MF2, "C", "off"),
    row(64, 8, 8, MF2), row(64, 8, 8, MF2, "", "off"), row(64, 8, 8, MFMA, "", "on"),
    # (the last one went to back_pass_mf2_kernel before the choice moved to one place: a time-varying cost at this shape belongs on the
    # round-5 kernel whether or not limits are set)
    row(64, 8, 8, MFMA, "C"), row(64, 8, 8, MFMA, "C", "on"), row(64, 8, 8, MFMA, "C", "off"),
    row(64, 8, 8, MF2, "C", "on", BACKPASS="new"), row(64, 8, 8, MFMA, BACKPASS="old"), row(40, 5, 8, MF2, BACKPASS="old"),
    row(64, 8, 8, BIG, BACKPASS="b"), row(40, 4, 8, BIG, "C", "on", BACKPASS="g"), row(41, 3, 8, BIG, BACKPASS="g"),
    # misaligned operands
    row(10, 2, 2048, MX, al=IN | OUT), row(10, 2, 512, MX, al=COST | OUT), row(10, 2, 2048, MX, al=IN | COST),
    row(10, 2, 6144, DPP, al=IN | COST, **PER_TRAJ), row(10, 2, 6144, DPPW, al=IN | OUT, **PER_TRAJ),
    # every DDP_BACKPASS letter on the (10, 2) shape
    *[row(10, 2, 64, want, BACKPASS=f) for f, want in (("x", MX2), ("q", DPP), ("dpp", DPP), ("general", GEN), ("big", GEN), ("s", DPP),
                                                        ("row", ROW), ("tile", MXR), ("wtile", MXG), ("mid", MID), ("old", DPP), ("new", DPP))],
    row(10, 2, 64, SH, BACKPASS="s", SH_MIN_B="1"), row(10, 2, 512, MX, BACKPASS="x", al=COST | OUT),
]


def _id(r):
    return "n%d_m%d_B%d_%s_%s_al%d_%s" % (r["n"], r["m"], r["B"], r["ops"] or "lti", r["lims"], r["al"],
                                          "_".join("%s=%s" % (k[4:], v) for k, v in sorted(r["env"].items())) or "default")


def _desc(r, BPDesc):
    o = r["ops"]
    return BPDesc(r["n"], r["m"], N_STEPS, r["B"], int("F" in o), int("f" in o), int("C" in o), int("c" in o), 1, int(r["lims"] is not None))


@pytest.fixture(scope="module")
def choice():
    if not os.path.exists(LIB):
        pytest.skip("libddp_amd.so not built")
    try:
        L = C.CDLL(LIB)
    except OSError as e:                      # no HIP runtime on this host
        pytest.skip(str(e))
    f = L.ddp_bp_choice
    f.restype = C.c_char_p
    f.argtypes = [C.c_void_p, C.c_uint, C.c_int, C.c_int, C.c_char_p, C.c_char_p, C.c_char_p, C.c_char_p]
    return f


@pytest.mark.parametrize("r", TABLE, ids=_id)
def test_kernel_choice(choice, r):
    from ddp_amd import _lib
    d = _desc(r, _lib.BPDesc)
    sw = [r["env"].get(k) for k in ("DDP_BACKPASS", "DDP_SH_MIN_B", "DDP_MX2", "DDP_DPPW")]
    got = choice(C.byref(d), r["al"], 1, int(r["lims"] == "on"), *[s.encode() if s else None for s in sw]).decode()
    assert got == r["want"], (got, r)


def test_kernel_choice_without_a_sink(choice):
    """a handle whose sink buffer could not be allocated: no shared-operand, dppw or row kernel"""
    from ddp_amd import _lib
    def ask(n, m, B, sink, sh_min_b=None):
        return choice(C.byref(_desc(row(n, m, B, None), _lib.BPDesc)), ALL, sink, 0, None, sh_min_b, None, None).decode()
    assert ask(10, 2, 2048, 0) == MX
    assert ask(10, 2, 6144, 0, b"1000000") == DPP
    assert ask(13, 1, 64, 0) == MID
    assert ask(65, 1, 8, 1) == ""                 # no kernel: the dispatcher reports the error


def _strides(L, n, m, N, fx_tv, fx_batched, cost_tv, cost_batched):
    """the ten element strides the kernels get (bp_kargs through its unlisted debug hook ddp_bp_strides), as
    {"fx": (per step, per trajectory), ...}"""
    from ddp_amd import _lib
    out = (C.c_longlong * 10)(*([-1] * 10))
    L.ddp_bp_strides.restype = None
    L.ddp_bp_strides.argtypes = [C.c_void_p, C.c_void_p]
    L.ddp_bp_strides(C.byref(_lib.BPDesc(n, m, N, 4, fx_tv, fx_batched, cost_tv, cost_batched, 1, 0)), out)
    return {k: (out[2 * i], out[2 * i + 1]) for i, k in enumerate(("fx", "fu", "cxx", "cxu", "cuu"))}


def _strides_expected(n, m, N, fx_tv, fx_batched, cost_tv, cost_batched):
    """an array [len] / [len, N] / [len, B] / [len, N, B] (column-major, batch slowest): a step is len elements further when the array
    has the time axis, a trajectory len * (N when it has the time axis) further when it has the batch axis; 0 where the axis is missing"""
    want = {}
    for k, ln, tv, batched in (("fx", n * n, fx_tv, fx_batched), ("fu", n * m, fx_tv, fx_batched), ("cxx", n * n, cost_tv, cost_batched),
                               ("cxu", n * m, cost_tv, cost_batched), ("cuu", m * m, cost_tv, cost_batched)):
        shape = [ln] + ([N] if tv else []) + ([4] if batched else [])
        el = np.cumprod([1] + shape[:-1])                   # column-major element strides of the axes
        want[k] = (int(el[1]) if tv else 0, int(el[-1]) if batched else 0)
    return want


FLAGS16 = [tuple((i >> s) & 1 for s in (3, 2, 1, 0)) for i in range(16)]


@pytest.mark.parametrize("n,m,N", [(3, 1, 2), (64, 8, 300)])
def test_kernel_argument_strides(choice, n, m, N):
    """every combination of fx_tv, fx_batched, cost_tv, cost_batched against the strides of the arrays' own shapes"""
    L = C.CDLL(LIB)
    for flags in FLAGS16:
        assert _strides(L, n, m, N, *flags) == _strides_expected(n, m, N, *flags), flags


def test_kernel_argument_strides_stay_exact_in_64_bits(choice):
    """n = 64, N = 400 000: a trajectory of fx is 64 * 64 * 400 000 = 1 638 400 000 elements, 13 107 200 000 bytes, past 2^32; the
    expected values are Python integers (exact)"""
    n, m, N = 64, 8, 400000
    got = _strides(C.CDLL(LIB), n, m, N, 1, 1, 1, 1)
    assert got == {"fx": (n * n, n * n * N), "fu": (n * m, n * m * N), "cxx": (n * n, n * n * N), "cxu": (n * m, n * m * N),
                   "cuu": (m * m, m * m * N)}
    assert got["fx"][1] == 1638400000 and got["fx"][1] * 8 > 2 ** 32
    assert got == _strides_expected(n, m, N, 1, 1, 1, 1)


def run_row(h, r):
    """one backward pass of the row's call on the device (operands at 8-byte offsets where the row says misaligned); returns
    ddp_last_kernel(h, 0)"""
    from ddp_amd import _lib
    n, m, N, B, o = r["n"], r["m"], N_STEPS, r["B"], r["ops"]
    rng = np.random.default_rng(n * 1000 + m * 100 + B)
    nf = (N if "F" in o else 1) * (B if "f" in o else 1)
    nc = (N if "C" in o else 1) * (B if "c" in o else 1)
    ins = {"cx": (0.1 * rng.standard_normal(n * N * B), IN), "cu": (0.1 * rng.standard_normal(m * N * B), IN),
           "cxx": (np.tile(np.eye(n).ravel("F"), nc), COST), "cxu": (np.zeros(n * m * nc), 0), "cuu": (np.tile(np.eye(m).ravel("F"), nc), COST),
           "fx": (np.tile(0.9 * np.eye(n).ravel("F"), nf), 0), "fu": (0.1 * rng.standard_normal(n * m * nf), 0),
           "lambda": (np.ones(B), 0), "u": (np.zeros(m * N * B), 0)}
    if r["lims"] is not None:
        lo, hi = (-1.0, 1.0) if r["lims"] == "on" else (1.0, -1.0)
        ins["lims"] = (np.concatenate([np.full(m, lo), np.full(m, hi)]), 0)
    outs = {"K": (m * n * N * B, OUT), "k": (m * N * B, OUT), "Quu": (m * m * N * B, OUT), "Vx": (n * N * B, OUT), "Vxx": (n * n * N * B, OUT),
            "dV": (2 * B, 0)}
    bufs, ptr = [], {}
    try:
        for name, (a, grp) in ins.items():
            p = h.malloc(a.nbytes + 16)
            bufs.append(p)
            ptr[name] = p.value + (8 if grp and not (r["al"] & grp) else 0)
            a = np.ascontiguousarray(a, dtype=np.float64)
            _lib.check(_lib.lib().ddp_memcpy_h2d(h.raw, C.c_void_p(ptr[name]), a.ctypes.data_as(C.c_void_p), C.c_size_t(a.nbytes)))
        for name, (cnt, grp) in list(outs.items()) + [("diverge", (B // 2 + 1, 0))]:
            p = h.malloc(8 * cnt + 16)
            bufs.append(p)
            ptr[name] = p.value + (8 if grp and not (r["al"] & grp) else 0)
        d = _desc(r, _lib.BPDesc)
        args = [ptr[k] for k in ("cx", "cu", "cxx", "cxu", "cuu", "fx", "fu", "lambda")] + [ptr.get("lims"), ptr["u"] if r["lims"] else None,
                                                                                           None] + [ptr[k] for k in ("K", "k", "Quu", "Vx", "Vxx", "dV", "diverge")]
        _lib.check(_lib.lib().ddp_back_pass_f64_dev(h.raw, C.byref(d), *[C.c_void_p(a) for a in args]))
        h.sync()
        return h.last_kernel(0)
    finally:
        for p in bufs:
            h.free(p)


@pytest.mark.gpu
def test_kernel_census(monkeypatch):
    """every row of the table through the device dispatcher: the kernel it reports is the one the choice names"""
    from ddp_amd import _lib
    h = _lib.default_handle()
    for k in [k for k in os.environ if k.startswith("DDP_")]:
        monkeypatch.delenv(k)
    bad = []
    for r in TABLE:
        for k, v in r["env"].items():
            monkeypatch.setenv(k, v)
        try:
            got = run_row(h, r)
        finally:
            for k in r["env"]:
                monkeypatch.delenv(k)
        if got != r["want"]:
            bad.append((_id(r), got, r["want"]))
    assert not bad, bad
