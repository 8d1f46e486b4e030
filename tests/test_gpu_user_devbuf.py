"""The device storage a user problem keeps between calls (DevBuf of csrc/user_problem.hip: grown on demand, never shrunk): ONE problem object
called with B = 3, then 7, then 3 returns, bit for bit, what a freshly created problem returns for the same call.  The second call grows
every buffer (and frees the block the first one used), the third runs in a block larger than it needs.  One case per buffer:

    t0_dev            a clock=True problem through ddp_user_forward_pass_f64 with one clock per trajectory
    blk, lam, mu      car_keepout_ad through ddp_user_ilqg_f64 with multipliers set (the parameter block of bind())
    al_ws             car_keepout_ad through ddp_user_ilqg_al_f64 with max_outer = 2 (the arrays of the second round)
    chol              a sample=True problem through ddp_user_sample_f64 with a Σ (the noise factors)
    curv              bicycle_ad, second_order_wave=True, through ddp_user_back_pass_f64 (the curvature block of the step in flight)

The kernels are deterministic and the inputs of a call depend on (case, B) alone, so equal bits are expected and asserted."""
import numpy as np
import pytest

import constraints_cases as cc
import ddp2_reference as d2
from user_clock_cases import nparam_of, track_params

pytestmark = pytest.mark.gpu

BATCHES = (3, 7, 3)
N = 5


@pytest.fixture(scope="module")
def ddp():
    import ddp_amd
    return ddp_amd


def _spd(rng, k, shape):
    A = rng.standard_normal((k, k) + shape) / np.sqrt(k)
    return np.einsum("ij...,kj...->ik...", A, A) + 0.5 * np.eye(k).reshape((k, k) + (1,) * len(shape))


def _flat(out):
    """every array of a (nested) result, in order"""
    if isinstance(out, dict):
        return [a for k in sorted(out) for a in _flat(out[k])]
    if isinstance(out, (tuple, list)):
        return [a for o in out for a in _flat(o)]
    if hasattr(out, "K") and hasattr(out, "Σi"):                 # a GaussianPolicy
        return [np.asarray(out.K), np.asarray(out.k), np.asarray(out.Σ), np.asarray(out.Σi)]
    return [np.asarray(out)]


def _clock(ddp):
    make = lambda: ddp.DeviceProblem(ddp.example_source("car_track"), 4, 2, nparam=nparam_of("car_track"), terminal=True, clock=True)

    def call(prob, B):
        rng = np.random.default_rng(20 + B)
        P = track_params(rng, B)
        x0 = np.stack([P[7], P[8], np.full(B, 0.3), np.full(B, 0.8)]) + 0.1 * rng.standard_normal((4, B))
        u0 = 0.2 * rng.standard_normal((2, N, B))
        return ddp.forward_pass(None, x0, u0, None, 1.0, prob, None, params=P, t0=3 * np.arange(B) + 1)
    return make, call


def _keepout(ddp):
    return lambda: ddp.DeviceProblem(ddp.example_source("car_keepout_ad"), 4, 2, nparam=cc.NPARAM, terminal=True, autodiff=True,
                                     constraints=cc.NC)


def _multipliers(ddp):
    def call(prob, B):
        p, x0, u0 = cc.designed(30 + B, B, N)
        rng = np.random.default_rng(31 + B)
        lam = rng.uniform(0.0, 0.5, (cc.NC, N, B)) * (rng.uniform(size=(cc.NC, N, B)) < 0.5)
        out = ddp.iLQG(prob, x0, u0, params=p, multipliers=(lam, np.linspace(0.5, 4.0, B)), max_iter=3, timing=False)
        return out[:6] + (out[6]["stats"],)                      # (the rest of the trace holds wall-clock times)
    return _keepout(ddp), call


def _al(ddp):
    def call(prob, B):
        p, x0, u0 = cc.designed(40 + B, B, N)
        return ddp.iLQG_al(prob, x0, u0, params=p, max_outer=2, max_iter=3)
    return _keepout(ddp), call


def _sample(ddp):
    n, m = 3, 2
    make = lambda: ddp.DeviceProblem(ddp.example_source("lq_ad"), n, m, nparam=2 * n * n + n * m + m * m, autodiff=True, sample=True)

    def call(prob, B):
        rng = np.random.default_rng(50 + B)
        A = 0.9 * np.eye(n) + 0.05 * rng.standard_normal((n, n))
        prm = np.concatenate([a.ravel(order="F") for a in (A, 0.3 * rng.standard_normal((n, m)), np.diag([1.0, 2.0, 0.5]), np.diag([0.1, 0.2]))])
        P = np.repeat(prm[:, None], B, 1) * (1.0 + 0.01 * np.arange(B))[None, :]
        x0 = 1.0 + 0.1 * rng.standard_normal((n, B))
        x, u = 1.0 + 0.1 * rng.standard_normal((n, N, B)), 0.1 * rng.standard_normal((m, N, B))
        pol = ddp.GaussianPolicy(N, n, m, 0.1 * rng.standard_normal((m, n, N, B)), np.zeros((m, N, B)), 0.05 * _spd(rng, m, (N, B)),
                                 np.zeros((m, m, N, B)))
        return ddp.sample_policy(prob, pol, x0, x, u, 5, seed=7, params=P, moments=True)
    return make, call


def _curvature(ddp):
    n, m = 4, 2
    make = lambda: ddp.DeviceProblem(ddp.example_source("bicycle_ad"), n, m, nparam=10, terminal=True, autodiff=True, wave=True,
                                     second_order_wave=True)

    def call(prob, B):
        rng = np.random.default_rng(60 + B)
        P = np.asfortranarray(d2.sketch_inputs(B=B)[0])
        x, u = 0.4 * rng.standard_normal((n, N, B)), 0.5 * rng.standard_normal((m, N, B))
        fx = np.eye(n)[:, :, None, None] + 0.15 * rng.standard_normal((n, n, N, B))
        fu = 0.25 * rng.standard_normal((n, m, N, B))
        cx, cu = 0.1 * rng.standard_normal((n, N, B)), 0.3 * rng.standard_normal((m, N, B))
        cxx, cuu, cxu = _spd(rng, n, (N, B)), _spd(rng, m, (N, B)), 0.1 * rng.standard_normal((n, m, N, B))
        return ddp.back_pass_ddp(prob, cx, cu, cxx, cxu, cuu, fx, fu, np.linspace(1.0, 2.0, B), 1, None, x, u, params=P)
    return make, call


CASES = {"t0_dev": _clock, "blk_lam_mu": _multipliers, "al_ws": _al, "chol": _sample, "curv": _curvature}


@pytest.mark.parametrize("case", sorted(CASES))
def test_a_problem_called_with_growing_and_shrinking_batches_returns_what_a_fresh_one_does(ddp, case):
    make, call = CASES[case](ddp)
    kept = make()
    for i, B in enumerate(BATCHES):
        got, want = _flat(call(kept, B)), _flat(call(make(), B))
        assert len(got) == len(want) and len(got) >= 3
        for j, (a, b) in enumerate(zip(got, want)):
            assert a.shape == b.shape and a.dtype == b.dtype, (case, i, B, j)
            assert a.tobytes() == b.tobytes(), "%s: call %d (B = %d): output %d differs from a fresh problem's" % (case, i, B, j)
        assert any(np.isfinite(a).all() and np.any(a) for a in got if a.dtype == np.float64), (case, i, B)
