"""expected_cost and kl_step_adjust on the GPU: every designed case of tests/expect_reference.py against the long double recursion
(ec relative to the sum of the absolute values of its five terms, mu relative to |μx| + |u + δu|, sigma relative to |Σz|_F, per step;
TOL = 1e-8, the project's parity tolerance), the bit-for-bit guarantees (two calls, a slice of the trajectories, host against `_dev`,
unbatched arrays), the status rule, two cross-checks against the existing product path (forward_pass on fitted tables,
kl.forward_covariance) and the step rule against its float64 NumPy statement.  Every device result is computed once and shared.

Rule tested for a value that is not finite: the first step whose ec is not finite sets status = i + 1, and from that step on the
trajectory's ec, mu and sigma are NaN — also when the value (a c0_i) does not enter the chain of moments.

Measured on one MI355X, worst over the designed cases: ec 1.4e-15 (13x4), mu 4.5e-16 (4x2-N33), sigma 4.3e-16 (32x8); against
forward_pass on the tables 4.4e-16, against kl.forward_covariance 2.6e-16; kl_step_adjust equal to its NumPy statement on every
column."""
import functools

import numpy as np
import pytest

import expect_reference as er
from conftest import relerr
from test_gpu_user_problem import lq_params

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ddp():
    import ddp_amd
    import ddp_amd.kl  # noqa: F401
    ddp_amd.default_handle()
    return ddp_amd


def _policy(ddp, c, sl=slice(None)):
    K = c["K"][..., sl]
    return ddp.GaussianPolicy(c["N"], c["n"], c["m"], K, np.zeros((c["m"],) + K.shape[2:]), None if c["Sg"] is None else c["Sg"][..., sl], None)


def _cut(tabs, sl, N, B):
    """the trajectories `sl` of a model whose tables carry the batch axis; a shared model as it is"""
    return tuple(None if a is None else (a[..., sl] if er._has_b(a, N, B) else a) for a in tabs)


def _call(ddp, c, sl=slice(None), **kw):
    N, B = c["N"], c["B"]
    return ddp.expected_cost(_policy(ddp, c, sl), None if c["x0"] is None else c["x0"][..., sl], c["x"][..., sl], c["u"][..., sl],
                             _cut(c["model"], sl, N, B), _cut(c["cost"], sl, N, B), Sigma0=None if c["Sigma0"] is None else c["Sigma0"][..., sl],
                             moments=True, **kw)


@functools.lru_cache(maxsize=None)
def _result(name):
    import ddp_amd
    return _call(ddp_amd, er.case(name))


def _dev_call(ddp, c):
    """ddp_expected_cost_f64_dev on uploaded arrays; the outputs start as -7"""
    h, L = ddp.default_handle(), ddp._lib.lib()
    n, m, N, B = c["n"], c["m"], c["N"], c["B"]
    p = n + m
    fx, fu, fc, cov = c["model"]
    ins = [c["K"], c["Sg"], c["x0"], c["x"], c["u"], fx, fu, fc, cov] + list(c["cost"]) + [c["Sigma0"]]
    dev = [None if a is None else h.to_device(np.asfortranarray(a)) for a in ins]
    shapes = [((N, B), np.float64), ((B,), np.int32), ((p, N, B), np.float64), ((p, p, N, B), np.float64)]
    outs = [h.to_device(np.full(s, -7, dtype=t, order="F")) for s, t in shapes]
    try:
        ddp._lib.check(L.ddp_expected_cost_f64_dev(h.raw, n, m, N, B, *dev[:9], int(er._has_b(fx, N, B)), *dev[9:15], int(er._has_b(c["cost"][0], N, B)),
                                                   dev[15], *outs))
        h.sync()
        return tuple(h.to_host(q, s, t) for q, (s, t) in zip(outs, shapes))
    finally:
        for q in [d for d in dev if d is not None] + outs:
            h.free(q)


WORST = {}


@pytest.mark.parametrize("name", sorted(er.CASES))
def test_matches_long_double(ddp, name):
    c = er.case(name)
    n, m, N, B = c["n"], c["m"], c["N"], c["B"]
    ec, status, mu, sigma = _result(name)
    assert ec.shape == (N, B) and mu.shape == (n + m, N, B) and sigma.shape == (n + m, n + m, N, B) and status.shape == (B,)
    assert ec.dtype == mu.dtype == sigma.dtype == np.float64 and status.dtype == np.int32
    assert np.all(status == 0)
    assert np.array_equal(sigma, np.swapaxes(sigma, 0, 1)), "sigma is not symmetric to the bit"
    e = er.errors((ec, mu, sigma), c["ref"])
    WORST[name] = e
    print("%s: ec %.2e  mu %.2e  sigma %.2e   (worst so far: ec %.2e mu %.2e sigma %.2e)"
          % ((name,) + e + tuple(max(w[k] for w in WORST.values()) for k in range(3))))
    assert max(e) < er.TOL, e


def test_unbatched_arrays_drop_the_batch_axis_and_give_the_bits_of_their_slice(ddp):
    for name in ("4x2", "13x4-shared-model", "4x2-deterministic"):
        c = er.case(name)
        full = _result(name)
        b = 1
        out = _call(ddp, c, b)
        assert isinstance(out[1], int) and out[1] == 0
        assert out[0].shape == (c["N"],) and out[2].shape == (c["n"] + c["m"], c["N"]) and out[3].shape == (c["n"] + c["m"],) * 2 + (c["N"],)
        for got, ref in zip((out[0], out[2], out[3]), (full[0], full[2], full[3])):
            assert np.array_equal(got, ref[..., b]), name
        ec_only = ddp.expected_cost(_policy(ddp, c, b), None if c["x0"] is None else c["x0"][..., b], c["x"][..., b], c["u"][..., b],
                                    _cut(c["model"], b, c["N"], c["B"]), _cut(c["cost"], b, c["N"], c["B"]),
                                    Sigma0=None if c["Sigma0"] is None else c["Sigma0"][..., b])
        assert len(ec_only) == 2 and np.array_equal(ec_only[0], full[0][:, b])


@pytest.mark.parametrize("name", ["4x2", "13x4-shared-model", "13x4-shared-cost", "32x8"])
def test_same_bits_twice_on_a_slice_and_through_the_dev_entry(ddp, name):
    c = er.case(name)
    first = _result(name)
    again = _call(ddp, c)
    dev = _dev_call(ddp, c)
    part = _call(ddp, c, slice(1, 3))
    for k in range(4):
        assert np.array_equal(first[k], again[k]), (name, "second call", k)
        assert np.array_equal(first[k], dev[k]), (name, "_dev", k)
        assert np.array_equal(first[k][..., 1:3], part[k]), (name, "slice", k)


def test_nan_in_the_dynamics_sets_the_status_and_poisons_what_follows(ddp):
    c = dict(er.case("4x2"))
    clean = _result("4x2")
    fc = c["model"][2].copy(order="F")
    fc[:, 3, 1] = np.nan
    c["model"] = c["model"][:2] + (fc,) + c["model"][3:]
    ec, status, mu, sigma = _call(ddp, c)
    assert list(status) == [0, 5, 0]                             # step 4 is the first whose ec reads fc_3
    for got, ref in zip((ec, mu, sigma), (clean[0], clean[2], clean[3])):
        assert np.all(np.isnan(got[..., 4:, 1]))
        assert np.array_equal(got[..., :4, 1], ref[..., :4, 1])
        assert np.array_equal(got[..., [0, 2]], ref[..., [0, 2]])


def test_nan_in_c0_sets_the_status_and_poisons_what_follows(ddp):
    """c0 does not enter the chain of moments: the documented rule is that the outputs are NaN from the failing step on all the same"""
    c = dict(er.case("4x2"))
    clean = _result("4x2")
    c0 = c["cost"][5].copy(order="F")
    c0[2, 1] = np.nan
    c["cost"] = c["cost"][:5] + (c0,)
    ec, status, mu, sigma = _call(ddp, c)
    assert list(status) == [0, 3, 0]
    for got, ref in zip((ec, mu, sigma), (clean[0], clean[2], clean[3])):
        assert np.all(np.isnan(got[..., 2:, 1]))
        assert np.array_equal(got[..., :2, 1], ref[..., :2, 1])
        assert np.array_equal(got[..., [0, 2]], ref[..., [0, 2]])
    # the last step has no transition: a failure there is reported the same way
    c0 = c["cost"][5].copy(order="F")
    c0[2, 1] = 1.0
    c0[c["N"] - 1, 0] = np.inf
    c["cost"] = c["cost"][:5] + (c0,)
    ec, status, _, _ = _call(ddp, c)
    assert list(status) == [c["N"], 0, 0] and np.isnan(ec[-1, 0]) and np.all(np.isfinite(ec[:-1, 0]))


# ------------------------------------------------------------------------------------------------- against the existing product path
@functools.lru_cache(maxsize=None)
def _lq_case():
    import ddp_amd as ddp
    n, m, N, B = 4, 2, 7, 3
    c = er.designed(n, m, N, B, 901, no_sigma=True, no_cov=True, no_sigma0=True, given_x0=True)
    rng = np.random.default_rng(902)
    spd = lambda k: er._spd(rng, k, 1.0)                                                 # noqa: E731
    P = np.asfortranarray(np.stack([lq_params(np.zeros((n, n)), np.zeros((n, m)), spd(n), spd(m)) for _ in range(B)], -1))
    prob = ddp.DeviceProblem(ddp.example_source("lq"), n, m, nparam=2 * n * n + n * m + m * m, fitted=True)
    return c, prob, P


def test_deterministic_case_is_the_cost_of_the_rollout_on_the_tables(ddp):
    """the lq example on fitted tables: its cost is quadratic, so the model made of its derivatives at the nominal is exact, and ec is
    the cost per step of forward_pass(..., model=(fx, fu, fc)) under the same policy"""
    c, prob, P = _lq_case()
    n, m, N, B = c["n"], c["m"], c["N"], c["B"]
    fx, fu, fc, _ = c["model"]
    d = ddp.df(prob, c["x"], c["u"], params=P)
    cx, cu, cxx, cxu, cuu = d[5:10]
    c0 = ddp.costfun(prob, c["x"], c["u"], params=P)
    assert c0.shape == (N, B) and cxx.shape == (n, n, N, B)
    pol = ddp.GaussianPolicy(N, n, m, c["K"], np.zeros((m, N, B)), None, None)
    xn, un, cn = ddp.forward_pass(pol, c["x0"], c["u"], c["x"], 1.0, prob, None, params=P, model=(fx, fu, fc))
    ec, status, mu, sigma = ddp.expected_cost(pol, c["x0"], c["x"], c["u"], (fx, fu, fc, None), (cx, cu, cxx, cxu, cuu, c0), moments=True)
    assert np.all(status == 0) and np.all(sigma == 0)
    e = max(relerr(ec, cn.reshape(N, B), 0), relerr(mu[:n], xn.reshape(n, N, B), 1), relerr(mu[n:], un.reshape(m, N, B), 1))
    print("expected_cost against forward_pass on the tables: %.2e" % e)
    assert e < er.TOL


def test_open_loop_covariance_is_forward_covariance(ddp):
    """K = 0, Σ = None, cov_i = R1 and Sigma0 = R1: the chain is the reference's fx Σ fx' + R1"""
    c, _, _ = _lq_case()
    n, m, N, B = c["n"], c["m"], c["N"], c["B"]
    fx, fu, fc, _ = c["model"]
    R1 = er._spd(np.random.default_rng(903), n, 0.2)
    rep = np.asfortranarray(np.repeat(np.repeat(R1[:, :, None, None], N, 2), B, 3))
    zero = ddp.GaussianPolicy(N, n, m, np.zeros((m, n, N, B)), np.zeros((m, N, B)), None, None)
    _, status, _, sigma = ddp.expected_cost(zero, None, c["x"], c["u"], (fx, fu, fc, rep), c["cost"], Sigma0=R1, moments=True)
    zs = np.zeros((m, m, N, B))
    ref = ddp.kl.forward_covariance(ddp.kl.Model(fx, fu, R1), c["x"], c["u"], ddp.GaussianPolicy(N, n, m, np.zeros((m, n, N, B)), np.zeros((m, N, B)), zs, zs))
    assert np.all(status == 0)
    e = relerr(sigma[:n, :n], ref[:n, :n], 2)
    print("xx blocks against kl.forward_covariance: %.2e" % e)
    assert e < er.TOL


# ----------------------------------------------------------------------------------------------------------------------- the step rule
def test_kl_step_adjust_matches_its_numpy_statement(ddp):
    p, d, a, ks = er.step_triples()
    N, B = p.shape
    with np.errstate(over="ignore", invalid="ignore"):
        new_ref, mult_ref = er.step_rule(p, d, a, ks)
    new, mult = ddp.kl.kl_step_adjust(p, d, a, ks)
    assert new.shape == (B,) and mult.shape == (B,)
    bound = 3 * N * 2.0 ** -53 / er.STEP_CANCEL
    for b in range(B):
        print("column %d (%s): mult %.17g (%.17g)  kl_step_new %.17g (%.17g)" % (b, er.STEP_COLUMNS[b][4], mult[b], mult_ref[b], new[b], new_ref[b]))
        if b in er.STEP_MULT_EXACT:
            assert mult[b] == mult_ref[b], b
        else:
            assert abs(mult[b] - mult_ref[b]) <= bound * abs(mult_ref[b]), b
        if b in er.STEP_NEW_EXACT:
            assert new[b] == new_ref[b], b
        else:
            assert abs(new[b] - new_ref[b]) <= bound * abs(new_ref[b]), b
    # a scalar kl_step serves every trajectory; other bounds
    new1, mult1 = ddp.kl.kl_step_adjust(p, d, a, 1.0, step_min=0.2, step_max=3.0)
    r1 = er.step_rule(p, d, a, 1.0, 0.2, 3.0)
    assert np.allclose(new1, r1[0], rtol=bound, atol=0) and np.array_equal(mult1, mult)
    assert new1.min() == 0.2 and new1.max() == 3.0
    # one column, unbatched
    n0, m0 = ddp.kl.kl_step_adjust(p[:, 0], d[:, 0], a[:, 0], ks[0])
    assert n0.shape == (1,) and n0[0] == new[0] and m0[0] == mult[0]
