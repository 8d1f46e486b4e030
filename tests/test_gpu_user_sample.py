"""DDP_USER_SAMPLE on the GPU: ddp_normal_fill against the NumPy generator, ddp_user_sample against the long double rollout of
tests/sample_reference.py (1e-8 relative per time step, conftest.relerr) and against ddp_user_rollout, the generated stream against the
explicit one bit for bit, independence of the launch geometry, the moments, the plant, the status path of an indefinite Σ, and that
nothing else moved.  Every device result is computed once and shared (the caches below); nothing is written into a shared array."""
import functools

import numpy as np
import pytest

import ddp_amd
import sample_reference as sr
from conftest import relerr

pytestmark = pytest.mark.gpu
RTOL = 1e-8
LD = np.longdouble


@functools.lru_cache(maxsize=None)
def problem(name, sample=True):
    c = sr.case(name)
    diff = ddp_amd.WrappedDiff(*c["wrap"]) if c["wrap"] else None
    return ddp_amd.DeviceProblem(ddp_amd.example_source(c["example"]), c["n"], c["m"], nparam=c["nparam"], sample=sample, diff=diff, **c["kw"])


def policy(c, Sigma="case", b=None):
    sl = (Ellipsis,) if b is None else (Ellipsis, slice(b, b + 1))
    K = c["K"][sl]
    Sg = c["Sigma"] if isinstance(Sigma, str) else Sigma
    Sg = np.zeros((0, 0, 0)) if Sg is None else Sg[sl]
    return ddp_amd.GaussianPolicy(c["N"], c["n"], c["m"], K, np.zeros((c["m"], c["N"]) + K.shape[3:]), Sg, np.zeros((0, 0, 0)))


def run(name, *, S=None, Sigma="case", plant=False, b=None, **kw):
    c = sr.case(name)
    sl = (Ellipsis,) if b is None else (Ellipsis, slice(b, b + 1))
    return ddp_amd.sample_policy(problem(name), policy(c, Sigma, b), c["x0"][sl], c["x"][sl], c["u"][sl], c["S"] if S is None else S, lims=c["lims"],
                                 plant=plant, params=c["params"][sl], **kw)


@functools.lru_cache(maxsize=None)
def explicit(name, plant=False):
    """the call with the reference stream as explicit noise, moments included"""
    return run(name, noise=sr.noise_of(name), plant=plant, moments=True)


@functools.lru_cache(maxsize=None)
def generated(name, S=None):
    return run(name, S=S, seed=sr.case(name)["seed"], moments=True)


def same(a, b):
    return np.array_equal(a, b, equal_nan=True)


# ------------------------------------------------------------------------------------------------------------------------ 1. normals
def test_normals_match_the_numpy_generator():
    seed = (0x9ABCDEF0 << 32) | 0x87654321                       # both words have their top bit set: they travel as negative C ints
    got = ddp_amd.normal(seed, 3, 5, 70, 3)
    ref = sr.normals(seed, 3, 5, 70, 3)
    assert got.shape == ref.shape == (3, 5, 70, 3)
    err = float(np.max(np.abs(got - ref)))
    print("normal vs NumPy: max abs err %.3e, max |xi| %.3f" % (err, np.max(np.abs(ref))))
    assert err <= 1e-13 and np.max(np.abs(ref)) <= 8.6
    assert same(ddp_amd.normal(seed, 3, 5, 20, 2, sample0=37, traj0=1), got[:, :, 37:57, 1:3])
    assert same(ddp_amd.normal(seed, 3, 5, 70, sample0=0, traj0=2), got[..., 2])          # unbatched: the batch axis is dropped
    assert same(ddp_amd.normal(seed, 2, 5, 70, 3), got[:2])                              # the odd pair drops its second normal
    assert not same(ddp_amd.normal(seed ^ (1 << 63), 3, 5, 70, 3), got)


# ------------------------------------------------------------------------------------- 2. explicit noise against the long double rollout
@pytest.mark.parametrize("name", ["car", "car_lims", "pendcart", "lq_ad", "lq_big"])
def test_explicit_noise_matches_the_long_double_reference(name):
    c = sr.case(name)
    xs, us, cs, info = explicit(name)
    rx, ru, rc = sr.reference(name)
    assert xs.shape == (c["n"], c["N"], c["S"], c["B"]) and us.shape == (c["m"], c["N"], c["S"], c["B"]) and cs.shape == rc.shape
    errs = relerr(xs, rx, 1), relerr(us, ru, 1), relerr(cs, rc, 0), relerr(info["csum"], rc.sum(axis=0), 0)
    print("%s: xs %.2e us %.2e cs %.2e csum %.2e" % ((name,) + errs))
    assert max(errs) < RTOL, errs
    assert np.all(info["status"] == 0)
    if c["lims"] is not None:                                    # the limits act on some controls, not on all
        hit = (ru == c["lims"][:, 0, None, None, None]) | (ru == c["lims"][:, 1, None, None, None])
        assert 0.02 < hit.mean() < 0.9, hit.mean()
        assert np.all(us >= c["lims"][:, 0, None, None, None]) and np.all(us <= c["lims"][:, 1, None, None, None])


def test_last_kernel_names_the_sampler():
    explicit("car")
    run("car", S=2, seed=1)
    assert ddp_amd.default_handle().last_kernel(1) == "ddp_user_sample"


# --------------------------------------------------------------------------------------------------- 3. against the kernel that exists
@pytest.mark.parametrize("name", ["car_lims", "pendcart", "lq_ad"])
def test_matches_forward_pass_on_the_emulated_batch(name):
    """the same call as forward_pass(traj(K, k = 0), x0, u + L ξ, x, α = 1) at batch S·B (sample s of trajectory b is column s + S b)"""
    c = sr.case(name)
    n, m, N, S, B = (c[k] for k in "nmNSB")
    xi = sr.noise_of(name)
    up = np.empty((m, N, S, B))
    for b in range(B):
        for i in range(N):
            up[:, i, :, b] = c["u"][:, i, b, None] + np.linalg.cholesky(c["Sigma"][:, :, i, b]) @ xi[:, i, :, b]
    rep = lambda a: np.repeat(a[..., None, :], S, axis=-2).reshape(a.shape[:-1] + (S * B,), order="F")      # noqa: E731
    pol = ddp_amd.GaussianPolicy(N, n, m, rep(c["K"]), np.zeros((m, N, S * B)), np.zeros((0, 0, 0)), np.zeros((0, 0, 0)))
    xf, uf, cf = ddp_amd.forward_pass(pol, rep(c["x0"]), up.reshape((m, N, S * B), order="F"), rep(c["x"]), 1.0, problem(name, False), c["lims"],
                                      params=rep(c["params"]))
    xs, us, cs, _ = explicit(name)
    errs = (relerr(xs.reshape(xf.shape, order="F"), xf, 1), relerr(us.reshape(uf.shape, order="F"), uf, 1),
            relerr(cs.reshape(cf.shape, order="F"), cf, 0))
    print("%s vs forward_pass: xs %.2e us %.2e cs %.2e" % ((name,) + errs))
    assert max(errs) < RTOL, errs


# -------------------------------------------------------------------------------------------------------------- 4. generated = explicit
@pytest.mark.parametrize("name", ["car_lims", "pendcart", "lq_ad"])
def test_generated_noise_equals_explicit_noise_bit_for_bit(name):
    c = sr.case(name)
    a = generated(name)
    b = run(name, noise=ddp_amd.normal(c["seed"], c["m"], c["N"], c["S"], c["B"]))
    assert same(a[0], b[0]) and same(a[1], b[1]) and same(a[2], b[2]) and same(a[3]["csum"], b[3]["csum"])
    # and the device stream is the reference stream to rounding: the generated call meets the reference at the same bar
    rx, ru, rc = sr.reference(name)
    assert max(relerr(a[0], rx, 1), relerr(a[1], ru, 1), relerr(a[2], rc, 0)) < RTOL


# ---------------------------------------------------------------------------------------------------------------------- 5. geometry
def test_samples_split_over_calls():
    seed = sr.case("car")["seed"]
    whole = generated("car", 130)
    first, second = run("car", S=64, seed=seed), run("car", S=66, seed=seed, sample0=64)
    for k in range(3):
        assert same(whole[k], np.concatenate([first[k], second[k]], axis=-2)), k
    assert same(whole[3]["csum"], np.concatenate([first[3]["csum"], second[3]["csum"]], axis=0))


def test_trajectories_split_over_calls():
    seed = sr.case("car")["seed"]
    whole = generated("car")
    for b in range(3):
        part = run("car", seed=seed, b=b, traj0=b, moments=True)
        for k in range(3):
            assert same(whole[k][..., b:b + 1], part[k]), (b, k)
        assert same(whole[3]["mean"][..., b:b + 1], part[3]["mean"]) and same(whole[3]["cov"][..., b:b + 1], part[3]["cov"])


def test_two_identical_calls_give_identical_bits():
    a, b = generated("car"), run("car", seed=sr.case("car")["seed"], moments=True)
    assert all(same(a[k], b[k]) for k in range(3))
    assert all(same(a[3][k], b[3][k]) for k in ("csum", "status", "mean", "cov"))
    assert np.all(np.isfinite(a[3]["cov"]))


def test_unbatched_inputs_drop_the_batch_axis():
    c = sr.case("car")
    pol = ddp_amd.GaussianPolicy(c["N"], c["n"], c["m"], c["K"][..., 1], np.zeros((c["m"], c["N"])), c["Sigma"][..., 1], np.zeros((0, 0, 0)))
    xs, us, cs, info = ddp_amd.sample_policy(problem("car"), pol, c["x0"][:, 1], c["x"][..., 1], c["u"][..., 1], 70, seed=c["seed"],
                                             params=c["params"][:, 1], traj0=1, moments=True)
    whole = generated("car")
    assert xs.shape == (4, 37, 70) and info["status"] == 0 and info["cov"].shape == (4, 4, 37)
    assert same(xs, whole[0][..., 1]) and same(us, whole[1][..., 1]) and same(cs, whole[2][..., 1]) and same(info["csum"], whole[3]["csum"][:, 1])


# ----------------------------------------------------------------------------------------------------------------------- 6. moments
def test_moments_of_the_returned_samples():
    """mean and cov against long double moments of the xs the call returned.  The device sums S terms in double (64 partial sums, then
    a tree): |error| <= S 2^-52 Σ|terms| covers any order of summation, and is the bound of the mean, e.  A covariance entry is a sum of
    products of factors centred with the DEVICE's mean, each off from the exactly centred d by at most e: the sum of products moves by
    at most Σ(|d_i| + e_i)(|d_j| + e_j) - Σ|d_i||d_j|, and the summation adds S 2^-52 Σ(|d_i| + e_i)(|d_j| + e_j).  (Without the first
    term the bound of step 0, where every sample is x0 and every d is 0, would be 0, which no mean rounded to double can meet.)"""
    xs, _, _, info = explicit("car")
    S = xs.shape[2]
    x = xs.astype(LD)
    mu = x.sum(axis=2) / S
    e_mu = S * 2.0 ** -52 * np.abs(x).sum(axis=2) / S
    d = x - mu[:, :, None, :]
    cov = np.einsum("insb,jnsb->ijnb", d, d) / (S - 1)
    a = np.abs(d) + e_mu[:, :, None, :]
    moved, exact = np.einsum("insb,jnsb->ijnb", a, a), np.einsum("insb,jnsb->ijnb", np.abs(d), np.abs(d))
    e_cov = ((moved - exact) + S * 2.0 ** -52 * moved) / (S - 1)
    err_mu, err_cov = np.abs(info["mean"] - mu), np.abs(info["cov"] - cov)
    print("moments: mean err / bound %.3f, cov err / bound %.3f" % (float((err_mu / e_mu).max()), float((err_cov / e_cov).max())))
    assert np.all(err_mu <= e_mu) and np.all(err_cov <= e_cov)
    assert same(info["cov"], np.swapaxes(info["cov"], 0, 1))


def test_sample_covariance_follows_the_exact_recursion():
    """lq, n = 3, m = 2, N = 6, B = 2, S = 4096, no limits: every entry of cov within 6 standard errors of
    Σ⁺ = (A + B K) Σ (A + B K)' + B Σ_u B'.  The seed was chosen on the CPU with the reference sampler (tests/test_user_sample_cpu.py)."""
    c = sr.lq_cov_case()
    prob = ddp_amd.DeviceProblem(ddp_amd.example_source("lq"), c["n"], c["m"], nparam=c["nparam"], sample=True)
    pol = ddp_amd.GaussianPolicy(c["N"], c["n"], c["m"], c["K"], np.zeros((c["m"], c["N"], c["B"])), c["Sigma"], np.zeros((0, 0, 0)))
    xs, _, _, info = ddp_amd.sample_policy(prob, pol, c["x0"], c["x"], c["u"], c["S"], seed=sr.LQ_COV_SEED, params=c["params"], moments=True)
    ok, err, se = sr.lq_cov_within(info["cov"], c)
    print("cov vs recursion: worst %.2f standard errors" % float(np.max(err[:, :, 1:] / se[:, :, 1:])))
    assert ok.all(), np.argwhere(~ok)
    assert np.all(info["cov"][:, :, 0] == 0)                     # (x0 is dyadic: the sums of step 0 are exact)


# ------------------------------------------------------------------------------------------------------------------------- 7. plant
def test_plant_rollouts():
    xs, us, cs, info = explicit("car_plant", True)
    rx, ru, rc = sr.reference("car_plant", True)
    errs = relerr(xs, rx, 1), relerr(us, ru, 1), relerr(cs, rc, 0)
    print("car_plant, plant: xs %.2e us %.2e cs %.2e" % errs)
    assert max(errs) < RTOL, errs
    xm = explicit("car_plant", False)[0]
    assert relerr(xm, sr.reference("car_plant", False)[0], 1) < RTOL
    assert np.max(np.abs(xm[:, -1] - xs[:, -1])) > 1e-2          # the plant is another system


def test_noise_free_closed_loop_on_the_plant():
    c = sr.case("car_plant")
    xs, us, cs, info = run("car_plant", S=1, Sigma=None, plant=True)
    for b in range(c["B"]):
        r = sr.rollout(sr.model_of(c), c["params"][:, b], c["K"][..., b], None, c["x0"][:, b], c["u"][..., b], c["x"][..., b], 1, plant=True)
        assert max(relerr(xs[..., b], r[0].astype(float), 1), relerr(us[..., b], r[1].astype(float), 1), relerr(cs[..., b], r[2].astype(float), 0)) < RTOL
    zero = run("car_plant", S=1, Sigma=np.zeros_like(c["Sigma"]), plant=True, seed=5)       # Σ all zero: the same path
    assert all(same(a, b) for a, b in zip((xs, us, cs), zero[:3]))


def test_plant_without_the_flag_is_refused_by_name():
    with pytest.raises(ddp_amd.DDPError, match="DDP_USER_PLANT"):
        run("car", plant=True, seed=1)
    with pytest.raises(ddp_amd.DDPError, match="DDP_USER_SAMPLE"):
        c = sr.case("car")
        ddp_amd.sample_policy(problem("car", False), policy(c), c["x0"], c["x"], c["u"], 4, params=c["params"])


# ------------------------------------------------------------------------------------------------------------------ 8. indefinite Σ
def test_indefinite_sigma_is_a_status():
    c = sr.case("car")
    Sg = c["Sigma"].copy()
    Sg[:, :, 3, 1] = -np.eye(c["m"])
    Sg[:, :, 9, 1] = -np.eye(c["m"])                             # the smallest failing step is reported
    xs, us, cs, info = run("car", Sigma=Sg, seed=c["seed"], moments=True)
    good = generated("car")
    assert info["status"].tolist() == [0, 4, 0]
    for a in (xs, us, cs, info["csum"], info["mean"], info["cov"]):
        assert np.all(np.isnan(a[..., 1]))
    for b in (0, 2):
        assert all(same(a[..., b], g[..., b]) for a, g in zip((xs, us, cs), good[:3]))
        assert same(info["mean"][..., b], good[3]["mean"][..., b]) and same(info["cov"][..., b], good[3]["cov"][..., b])


# ------------------------------------------------------------------------------------------------------------ 9. nothing else moved
def test_ilqg_ignores_the_flag():
    rng = np.random.default_rng(9)
    N, B = 30, 3
    P = np.repeat(sr.CAR_P[:, None], B, axis=1)
    x0 = np.array([[0.0, 0.0, 0.3, 1.0]]).T + 0.1 * rng.standard_normal((4, B))
    u0 = 0.1 * rng.standard_normal((2, N, B))
    out = []
    for flag in (False, True):
        prob = ddp_amd.DeviceProblem(ddp_amd.example_source("car_ad"), 4, 2, nparam=9, terminal=True, autodiff=True, sample=flag)
        x, u, traj, Vx, Vxx, cost, trace = ddp_amd.iLQG(prob, x0, u0, params=P, max_iter=30, timing=False)
        out.append((x, u, traj.K, traj.k, Vx, Vxx, cost, trace["status"], trace["iter"]))
    assert all(same(a, b) for a, b in zip(*out))
    assert np.all(out[0][7] != -1) and np.all(out[0][8] >= 2)    # (the solves ran)
