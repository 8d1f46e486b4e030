"""DDP_USER_CLOCK (DeviceProblem(..., clock=True)) without a GPU: the three car_track examples compile for gfx950 with the flag in every
legal combination, the combinations with the second-order flags are refused by name, a source with the wrong signatures fails to
compile with the function's name in the log, the constants of the header, the loader and the Julia binding agree, a problem without
the flag compiles the text it always did, and the unclocked twin that the GPU tests (tests/test_gpu_user_clock.py) compare with is
what it should be: the example's text with t replaced by i, compiled without the flag."""
import os
import re

import numpy as np
import pytest

import ddp_amd
from ddp_amd import _lib
from user_clock_cases import L_TRACK, nparam_of, track_cost, track_params, twin_source

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "differentialdynamicprogramming.jl_amd")
TERMINAL, CONST_HESSIAN, AUTODIFF, PLANT, SECOND, WAVE, SECOND_WAVE, CLOCK = 1, 2, 4, 8, 16, 32, 128, 512


def _check(name, flags, nparam=None):
    L = _lib.lib()
    src = ddp_amd.example_source(name).encode()
    rc = L.ddp_user_check(src, 4, 2, nparam_of(name) if nparam is None else nparam, flags, None)
    return rc, L.ddp_last_error().decode(), L.ddp_user_compile_log().decode()


@pytest.mark.parametrize("name,flags", [("car_track", CLOCK | TERMINAL), ("car_track_ad", CLOCK | TERMINAL | AUTODIFF),
                                        ("car_track_ad", CLOCK | TERMINAL | AUTODIFF | WAVE), ("car_track_plant", CLOCK | TERMINAL | PLANT),
                                        ("car_track", CLOCK | TERMINAL | WAVE)])
def test_clock_examples_compile_for_gfx950(name, flags):
    rc, err, log = _check(name, flags)
    assert rc == 0, (err, log[-3000:])


@pytest.mark.parametrize("flags,other", [(CLOCK | AUTODIFF | SECOND, "DDP_USER_SECOND_ORDER"),
                                         (CLOCK | WAVE | AUTODIFF | SECOND_WAVE, "DDP_USER_SECOND_ORDER_WAVE")])
def test_second_order_with_the_clock_is_refused_by_name(flags, other):
    rc, err, _ = _check("car_track_ad", flags | TERMINAL)
    assert rc != 0
    assert "DDP_USER_CLOCK" in err and re.search(other + r"\b", err), err
    with pytest.raises(ddp_amd.DDPError, match="DDP_USER_CLOCK"):
        ddp_amd.DeviceProblem(ddp_amd.example_source("car_track_ad"), 4, 2, nparam=nparam_of("car_track_ad"), terminal=True, autodiff=True,
                              clock=True, second_order=bool(flags & SECOND), second_order_wave=bool(flags & SECOND_WAVE)).check()


def test_the_old_signatures_do_not_compile_with_the_clock_nor_the_new_ones_without():
    rc, err, log = _check("car", CLOCK | TERMINAL, nparam=9)
    assert rc != 0 and "compilation failed" in err, err
    assert re.search(r"error: no matching function for call to 'dynamics'", log), log[-2000:]
    rc, err, log = _check("car_track", TERMINAL)
    assert rc != 0 and "compilation failed" in err, err
    assert re.search(r"error: no matching function for call to 'dynamics'", log), log[-2000:]


def test_header_loader_and_julia_agree():
    hdr = open(os.path.join(ROOT, "include", "ddp_amd.h")).read()
    jl = open(os.path.join(PKG, "julia", "DDPAmd.jl")).read()
    assert re.search(r"\bDDP_USER_CLOCK = 512\b", hdr)
    assert not re.search(r"DDP_USER_\w+\s*=\s*(64|256)\b", hdr)
    assert re.search(r"int ddp_user_set_t0\(void \*up, const int32_t \*t0, int count\);", hdr)
    assert "deferred, not impossible" in hdr
    assert _lib.USER_CLOCK == 512 and hasattr(_lib.lib(), "ddp_user_set_t0")
    assert re.search(r"^const USER_CLOCK = 512\b", jl, flags=re.M)
    assert re.search(r"clock::Bool=false", jl) and re.search(r"\(clock \? USER_CLOCK : 0\)", jl)
    assert re.search(r"@ccall libddp\.ddp_user_set_t0\(up::Ptr\{Cvoid\}, t::Ptr\{Int32\}, n::Cint\)::Cint", jl)
    for fn in ("forward_pass", "df", "costfun", "iLQG", "iLQG_queue", "iLQG_mpc", "iLQGkl"):
        sig = re.search(r"\nfunction %s\([^\n]*problem::DeviceProblem.*?\)\n" % fn, jl, flags=re.S).group(0)
        assert "t0=nothing" in sig, fn
    import inspect
    from ddp_amd import kl
    assert "clock" in inspect.signature(ddp_amd.DeviceProblem.__init__).parameters
    for fn in (ddp_amd.forward_pass, ddp_amd.df, ddp_amd.costfun, ddp_amd.iLQG, ddp_amd.iLQG_queue, ddp_amd.iLQG_mpc, kl.iLQGkl):
        assert "t0" in inspect.signature(fn).parameters, fn
    p = ddp_amd.DeviceProblem(ddp_amd.example_source("car_track"), 4, 2, nparam=nparam_of("car_track"), terminal=True, clock=True)
    assert p.flags == CLOCK | TERMINAL and p.clock
    for flags in (64, 256, 64 | CLOCK, 256 | CLOCK):            # the bits next to the flag stay unknown
        rc, err, _ = _check("car_track", flags | TERMINAL)
        assert rc != 0 and "unknown flags" in err, err


def _text(name, flags):
    t = _lib.lib().ddp_user_program_text(ddp_amd.example_source(name).encode(), 4, 2, nparam_of(name) if "track" in name else 9, flags, 0)
    assert t is not None, _lib.lib().ddp_last_error().decode()
    return t.decode()


def test_the_program_without_the_flag_holds_nothing_of_the_clock():
    """the byte pins of tests/test_user_wave_cpu.py hold the lane programs; here: no word of the clock in any program without the flag,
    the clocked program hands t to every call of the user's functions, and reads the clock once per kernel"""
    for name, flags in (("car", TERMINAL), ("car_ad", TERMINAL | AUTODIFF), ("car_ad", TERMINAL | AUTODIFF | WAVE), ("car_plant", TERMINAL | PLANT)):
        plain = _text(name, flags)
        for word in ("DDP_CLOCK", "DDP_T", "ddp_c", "ddp_t", "ddp_clock", "clk", "DDP_PLANT_T"):
            assert not re.search(r"\b%s\b" % word, plain), (name, word)
    for name, flags in (("car_track", TERMINAL), ("car_track_ad", TERMINAL | AUTODIFF), ("car_track_ad", TERMINAL | AUTODIFF | WAVE),
                        ("car_track_plant", TERMINAL | PLANT)):
        full = _text(name, flags | CLOCK)
        lib = full[full.index('#line 1 "ddp_user_kernels"'):]     # the library's kernels (the user's source comes before)
        assert full.startswith("#define DDP_N 4\n") and "#define DDP_CLOCK 1\n" in full
        assert "const int *clk; };" in lib
        # every call of the model in the library's text carries t
        assert not re.search(r"\b(stage_cost|dynamics)\([^()]*, (i|t), p[,)]", lib), name
        assert not re.search(r"\bterminal_cost\(\w+, p\)", lib), name
        assert re.search(r"stage_cost\(\w+, \w+, \w+, DDP_T\(\w+\), p\)", lib) and "DDP_T(N - 1), p)" in lib
        kernels = len(re.findall(r"= ddp_params\(", lib))
        assert kernels >= 3 and len(re.findall(r"const int ddp_c = ddp_clock\(a\.clk, b\);", lib)) == kernels
        if flags & PLANT:
            assert "plant(x, u, DDP_PLANT_T(t), ddp_params(" in lib
        if flags & AUTODIFF:
            ad = full[full.index('#line 1 "ddp_user_autodiff_derivs"'):full.index('#line 1 "ddp_user_kernels"')]
            assert "int i, int ddp_t, int N" in ad and "(x, u, i, DDP_T(i), N, p, o)" in ad and "terminal_cost(xd, DDP_T(N - 1), p)" in ad


def test_track_model_text_matches_the_numpy_restatement():
    """the example's source says what the NumPy restatement above says: the index clamp, the offsets and the cost terms (the restatement
    is what tests/test_gpu_user_clock.py recomputes the plant with)"""
    src = ddp_amd.example_source("car_track")
    assert "return 7 + 2 * (t < L - 1 ? t : L - 1);" in src
    assert "0.5 * p[3] * (u[0] * u[0] + u[1] * u[1]) + 0.5 * p[4] * (ex * ex + ey * ey) + p[2] * exp(-(dx * dx + dy * dy) / r2)" in src
    assert "dx = x[0] - p[k + 2 * L], dy = x[1] - p[k + 2 * L + 1]" in src
    assert "return 0.5 * p[5] * (ex * ex + ey * ey + x[3] * x[3]);" in src
    plant = ddp_amd.example_source("car_track_plant")
    assert plant[plant.index("__device__ int track_k"):].startswith(src[src.index("__device__ int track_k"):])
    assert "const int k = track_k(t, p) + 4 * (int)p[6];" in plant and "xnext[0] += p[0] * p[k];" in plant
    # the central differences of the restatement are finite and the cost sees the clock: another t, another value
    rng = np.random.default_rng(3)
    p = track_params(rng, 1)[:, 0]
    x, u = rng.standard_normal(4), rng.standard_normal(2)
    assert track_cost(p, x, u, 0, 3, 12) != track_cost(p, x, u, 0, 4, 12)
    assert track_cost(p, x, u, 0, 63, 12) == track_cost(p, x, u, 0, 90, 12)      # the clamp


def test_the_unclocked_twin_compiles_without_the_flag_and_holds_no_t():
    for N in (10, 12):
        tw = twin_source(ddp_amd.example_source("car_track"), N)
        assert "int t, const double *p, double *xnext" not in tw and "int i, int t" not in tw
        assert tw.count("track_k(i, p)") == 2 and tw.count("track_k(%d, p)" % (N - 1)) == 1 and "track_k(t, p)" not in tw
        L = _lib.lib()
        assert L.ddp_user_check(tw.encode(), 4, 2, nparam_of("car_track"), TERMINAL, None) == 0, L.ddp_user_compile_log().decode()[-2000:]
        assert L.ddp_user_check(tw.encode(), 4, 2, nparam_of("car_track"), TERMINAL | CLOCK, None) != 0
