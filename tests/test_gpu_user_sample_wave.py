"""DDP_USER_SAMPLE_WAVE on the GPU: ddp_user_sample_wave against the long double rollouts of tests/sample_wave_cases.py (1e-8 relative
per time step, conftest.relerr) on every case of its table, against ddp_user_sample inside the lane box and against ddp_user_rollout_wave
on the emulated batch, the bit rules (generated = explicit noise, splits over sample0 / traj0, two calls), the plant at (64, 32), the wide
noise factor and its status path, the moments at n = 64, and that nothing else moved.  Every compiled problem and every shared device
result is made once (the caches below); nothing is written into a shared array."""
import functools

import numpy as np
import pytest

import ddp_amd
import sample_wave_cases as wc
from conftest import relerr

pytestmark = pytest.mark.gpu
RTOL = 1e-8
LD = np.longdouble
GEO = "chain_34x17"                                              # the case of the bit rules: wide factor, m odd, two samples per work-group


@functools.lru_cache(maxsize=None)
def problem(name, mode="wave"):
    """mode: "wave" (wave=True, sample_wave=True), "plain" (wave=True alone) or "lane" (sample=True, no wave)"""
    c = wc.case(name)
    diff = ddp_amd.WrappedDiff(*c["wrap"]) if c["wrap"] else None
    flags = dict(wave=True, sample_wave=True) if mode == "wave" else (dict(wave=True) if mode == "plain" else dict(sample=True))
    return ddp_amd.DeviceProblem(ddp_amd.example_source(c["example"]), c["n"], c["m"], nparam=c["nparam"], diff=diff, **flags, **c["kw"])


def policy(c, Sigma="case", b=None):
    sl = (Ellipsis,) if b is None else (Ellipsis, slice(b, b + 1))
    K = c["K"][sl]
    Sg = c["Sigma"] if isinstance(Sigma, str) else Sigma
    Sg = np.zeros((0, 0, 0)) if Sg is None else Sg[sl]
    return ddp_amd.GaussianPolicy(c["N"], c["n"], c["m"], K, np.zeros((c["m"], c["N"]) + K.shape[3:]), Sg, np.zeros((0, 0, 0)))


def run(name, *, S=None, Sigma="case", plant=False, b=None, mode="wave", **kw):
    c = wc.case(name)
    sl = (Ellipsis,) if b is None else (Ellipsis, slice(b, b + 1))
    return ddp_amd.sample_policy(problem(name, mode), policy(c, Sigma, b), c["x0"][sl], c["x"][sl], c["u"][sl], c["S"] if S is None else S,
                                 lims=c["lims"], plant=plant, params=c["params"][sl], **kw)


@functools.lru_cache(maxsize=None)
def explicit(name, plant=False, S=None, mode="wave"):
    """the call with the reference stream as explicit noise"""
    return run(name, S=S, noise=wc.noise_of(name, S), plant=plant, mode=mode)


@functools.lru_cache(maxsize=None)
def generated(name, S=None):
    return run(name, S=S, seed=wc.case(name)["seed"], moments=True)


def same(a, b):
    return np.array_equal(a, b, equal_nan=True)


def errors(out, ref):
    return relerr(out[0], ref[0], 1), relerr(out[1], ref[1], 1), relerr(out[2], ref[2], 0), relerr(out[3]["csum"], ref[2].sum(axis=0), 0)


# ------------------------------------------------------------------------------------- 1. explicit noise against the long double rollout
@pytest.mark.parametrize("name", wc.NAMES)
def test_explicit_noise_matches_the_long_double_reference(name):
    c = wc.case(name)
    out = explicit(name)
    ref = wc.reference(name)
    assert out[0].shape == (c["n"], c["N"], c["S"], c["B"]) and out[1].shape == (c["m"], c["N"], c["S"], c["B"]) and out[2].shape == ref[2].shape
    errs = errors(out, ref)
    print("%s: xs %.2e us %.2e cs %.2e csum %.2e" % ((name,) + errs))
    assert max(errs) < RTOL, errs
    assert np.all(out[3]["status"] == 0)
    if c["lims"] is not None:
        assert np.all(out[1] >= c["lims"][:, 0, None, None, None]) and np.all(out[1] <= c["lims"][:, 1, None, None, None])


# ------------------------------------------------------------------------------------------------------- 2. against the lane sampler
def test_agrees_with_the_lane_sampler_inside_its_box():
    """chain_ad (16, 8), S = 5: ddp_user_sample_wave and ddp_user_sample on the same inputs and noise, each against the long double
    reference at the bar; their largest difference is printed (two kernels compiled in different contexts: bit equality is not claimed)"""
    ref = wc.reference("chain_16x8", S=5)
    wave, lane = explicit("chain_16x8", S=5), explicit("chain_16x8", S=5, mode="lane")
    ew, el = errors(wave, ref), errors(lane, ref)
    print("wave vs long double %.2e, lane vs long double %.2e, wave vs lane: xs %.2e us %.2e cs %.2e" %
          (max(ew), max(el), np.max(np.abs(wave[0] - lane[0])), np.max(np.abs(wave[1] - lane[1])), np.max(np.abs(wave[2] - lane[2]))))
    assert max(ew) < RTOL and max(el) < RTOL, (ew, el)


# ------------------------------------------------------------------------------------------------------- 3. against the wave rollout
@pytest.mark.parametrize("name", ["chain_34x17", "lq_ad_40x12"])
def test_matches_forward_pass_on_the_emulated_batch(name):
    """the same call as forward_pass(traj(K, k = 0), x0, u + L ξ, x, α = 1) of the wave problem at batch S·B (sample s of trajectory b is
    column s + S b)"""
    c = wc.case(name)
    n, m, N, S, B = (c[k] for k in "nmNSB")
    xi = wc.noise_of(name)
    up = np.empty((m, N, S, B))
    for b in range(B):
        for i in range(N):
            up[:, i, :, b] = c["u"][:, i, b, None] + np.linalg.cholesky(c["Sigma"][:, :, i, b]) @ xi[:, i, :, b]
    rep = lambda a: np.repeat(a[..., None, :], S, axis=-2).reshape(a.shape[:-1] + (S * B,), order="F")      # noqa: E731
    pol = ddp_amd.GaussianPolicy(N, n, m, rep(c["K"]), np.zeros((m, N, S * B)), np.zeros((0, 0, 0)), np.zeros((0, 0, 0)))
    xf, uf, cf = ddp_amd.forward_pass(pol, rep(c["x0"]), up.reshape((m, N, S * B), order="F"), rep(c["x"]), 1.0, problem(name), c["lims"],
                                      params=rep(c["params"]))
    assert ddp_amd.default_handle().last_kernel(1) == "ddp_user_rollout_wave"
    xs, us, cs, _ = explicit(name)
    errs = (relerr(xs.reshape(xf.shape, order="F"), xf, 1), relerr(us.reshape(uf.shape, order="F"), uf, 1),
            relerr(cs.reshape(cf.shape, order="F"), cf, 0))
    print("%s vs forward_pass: xs %.2e us %.2e cs %.2e" % ((name,) + errs))
    assert max(errs) < RTOL, errs


# ------------------------------------------------------------------------------------------------------------------- 4. the bit rules
@pytest.mark.parametrize("name", [GEO, "lq_ad_40x12", "pendcart_4x1"])
def test_generated_noise_equals_explicit_noise_bit_for_bit(name):
    c = wc.case(name)
    a = generated(name)
    b = run(name, noise=ddp_amd.normal(c["seed"], c["m"], c["N"], c["S"], c["B"]))
    assert same(a[0], b[0]) and same(a[1], b[1]) and same(a[2], b[2]) and same(a[3]["csum"], b[3]["csum"])
    assert max(errors(a, wc.reference(name))) < RTOL             # (the device stream is the reference stream to rounding)


def test_samples_split_over_calls():
    seed = wc.case(GEO)["seed"]
    whole = generated(GEO, 130)
    first, second = run(GEO, S=64, seed=seed), run(GEO, S=66, seed=seed, sample0=64)
    for k in range(3):
        assert same(whole[k], np.concatenate([first[k], second[k]], axis=-2)), k
    assert same(whole[3]["csum"], np.concatenate([first[3]["csum"], second[3]["csum"]], axis=0))
    assert np.all(np.isfinite(whole[0]))


def test_trajectories_split_over_calls():
    seed = wc.case(GEO)["seed"]
    whole = generated(GEO)
    for b in range(3):
        part = run(GEO, seed=seed, b=b, traj0=b, moments=True)
        for k in range(3):
            assert same(whole[k][..., b:b + 1], part[k]), (b, k)
        assert same(whole[3]["mean"][..., b:b + 1], part[3]["mean"]) and same(whole[3]["cov"][..., b:b + 1], part[3]["cov"])


def test_two_identical_calls_give_identical_bits():
    a, b = generated(GEO), run(GEO, seed=wc.case(GEO)["seed"], moments=True)
    assert all(same(a[k], b[k]) for k in range(3))
    assert all(same(a[3][k], b[3][k]) for k in ("csum", "status", "mean", "cov"))
    assert np.all(np.isfinite(a[3]["cov"]))


def test_unbatched_inputs_drop_the_batch_axis():
    c = wc.case(GEO)
    n, m, N, S = c["n"], c["m"], c["N"], c["S"]
    pol = ddp_amd.GaussianPolicy(N, n, m, c["K"][..., 1], np.zeros((m, N)), c["Sigma"][..., 1], np.zeros((0, 0, 0)))
    xs, us, cs, info = ddp_amd.sample_policy(problem(GEO), pol, c["x0"][:, 1], c["x"][..., 1], c["u"][..., 1], S, seed=c["seed"],
                                             params=c["params"][:, 1], traj0=1, moments=True)
    whole = generated(GEO)
    assert xs.shape == (n, N, S) and info["status"] == 0 and info["cov"].shape == (n, n, N)
    assert same(xs, whole[0][..., 1]) and same(us, whole[1][..., 1]) and same(cs, whole[2][..., 1]) and same(info["csum"], whole[3]["csum"][:, 1])


# ------------------------------------------------------------------------------------------------------ 5. kernel name and refusals
def test_last_kernel_names_the_sampler():
    run("pendcart_4x1", S=2, seed=1)
    assert ddp_amd.default_handle().last_kernel(1) == "ddp_user_sample_wave"


def test_refusals_by_name():
    c = wc.case("pendcart_4x1")
    with pytest.raises(ddp_amd.DDPError, match="DDP_USER_SAMPLE_WAVE"):
        ddp_amd.sample_policy(problem("pendcart_4x1", "plain"), policy(c), c["x0"], c["x"], c["u"], 4, params=c["params"])
    with pytest.raises(ddp_amd.DDPError, match="DDP_USER_PLANT"):
        run("pendcart_4x1", plant=True, seed=1)


# ------------------------------------------------------------------------------------------------------------------------- 6. plant
def test_plant_rollouts_at_the_edge_of_the_box():
    name = "chain_plant_64x32"
    out, ref = explicit(name, True), wc.reference(name, True)
    errs = errors(out, ref)
    print("%s, plant: xs %.2e us %.2e cs %.2e csum %.2e" % ((name,) + errs))
    assert max(errs) < RTOL, errs
    assert np.max(np.abs(explicit(name)[0][:, -1] - out[0][:, -1])) > 1e-3          # the plant is another system


def test_noise_free_closed_loop_on_the_plant():
    name = "chain_plant_64x32"
    c = wc.case(name)
    out = run(name, S=1, Sigma=None, plant=True)
    errs = errors(out, wc.reference(name, True, 1, False))
    print("%s, plant, no noise: xs %.2e us %.2e cs %.2e csum %.2e" % ((name,) + errs))
    assert max(errs) < RTOL, errs
    zero = run(name, S=1, Sigma=np.zeros_like(c["Sigma"]), plant=True, seed=5)      # Σ all zero: the same path
    assert all(same(a, b) for a, b in zip(out[:3], zero[:3]))


# ------------------------------------------------------------------------------------------------------------ 7. factor and status
@pytest.mark.parametrize("name", [GEO, "lq_33x2"])
def test_indefinite_sigma_is_a_status(name):
    """m = 17 (ddp_policy_factor_wide) and m = 2 (ddp_policy_factor): Σ indefinite at steps 3 and 5 of trajectory 1 of 3"""
    c = wc.case(name)
    pick = lambda a: a if c["B"] == 3 else np.repeat(a, 3, axis=-1)      # noqa: E731  (lq_33x2 has B = 1: three copies of its trajectory)
    m, N = c["m"], c["N"]
    Sg = pick(c["Sigma"]).copy()
    G = np.random.default_rng(3).standard_normal((m, m))
    Sg[:, :, 3, 1] = G @ G.T - 3.0 * np.eye(m)                   # symmetric, eigenvalues on both sides of 0
    Sg[:, :, 5, 1] = -np.eye(m)                                  # the smallest failing step is reported
    assert np.min(np.linalg.eigvalsh(Sg[:, :, 3, 1])) < 0 < np.max(np.linalg.eigvalsh(Sg[:, :, 3, 1]))
    pol = lambda S_: ddp_amd.GaussianPolicy(N, c["n"], m, pick(c["K"]), np.zeros((m, N, 3)), S_, np.zeros((0, 0, 0)))    # noqa: E731
    call = lambda S_: ddp_amd.sample_policy(problem(name), pol(S_), pick(c["x0"]), pick(c["x"]), pick(c["u"]), 5, seed=c["seed"],      # noqa: E731
                                            lims=c["lims"], params=pick(c["params"]), moments=True)
    xs, us, cs, info = call(Sg)
    good = call(pick(c["Sigma"]))
    assert info["status"].tolist() == [0, 4, 0] and good[3]["status"].tolist() == [0, 0, 0]
    for a in (xs, us, cs, info["csum"], info["mean"], info["cov"]):
        assert np.all(np.isnan(a[..., 1]))
    for b in (0, 2):
        assert all(same(a[..., b], g[..., b]) for a, g in zip((xs, us, cs), good[:3])) and np.all(np.isfinite(xs[..., b]))
        assert same(info["mean"][..., b], good[3]["mean"][..., b]) and same(info["cov"][..., b], good[3]["cov"][..., b])


# ----------------------------------------------------------------------------------------------------------------------- 8. moments
def test_moments_of_the_returned_samples_at_n_64():
    """mean and cov (n = 64, S = 70, N = 3) against long double moments of the xs the call returned, with the bound of
    tests/test_gpu_user_sample.py: the device sums S terms in double, |error| <= S 2^-52 Σ|terms| in any order; a covariance entry is a
    sum of products of factors centred with the device's mean, each off by at most that bound e: it moves by at most
    Σ(|d_i| + e_i)(|d_j| + e_j) - Σ|d_i||d_j|, and its own summation adds S 2^-52 Σ(|d_i| + e_i)(|d_j| + e_j)."""
    name = "chain_plant_64x32"
    c = wc.case(name)
    S, N = 70, 3
    pol = ddp_amd.GaussianPolicy(N, c["n"], c["m"], c["K"][:, :, :N], np.zeros((c["m"], N, c["B"])), c["Sigma"][:, :, :N], np.zeros((0, 0, 0)))
    xs, _, _, info = ddp_amd.sample_policy(problem(name), pol, c["x0"], c["x"][:, :N], c["u"][:, :N], S, seed=c["seed"], params=c["params"],
                                           moments=True)
    assert xs.shape == (64, N, S, 3) and np.all(info["status"] == 0)
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
    assert np.max(np.abs(info["cov"][:, :, 1:])) > 0


# ------------------------------------------------------------------------------------------------------------ 9. nothing else moved
def test_ilqg_ignores_the_flag():
    c = wc.case("pendcart_4x1")
    rng = np.random.default_rng(9)
    N = 30
    x0 = np.array([[np.pi - 0.4, 0.0, 0.0, 0.0]]).T + 0.05 * rng.standard_normal((4, 3))
    u0 = 0.1 * rng.standard_normal((1, N, 3))
    out = []
    for mode in ("plain", "wave"):
        x, u, traj, Vx, Vxx, cost, trace = ddp_amd.iLQG(problem("pendcart_4x1", mode), x0, u0, params=c["params"], max_iter=30, timing=False)
        out.append((x, u, traj.K, traj.k, Vx, Vxx, cost, trace["status"], trace["iter"]))
    assert all(same(a, b) for a, b in zip(*out))
    assert np.all(out[0][7] != -1) and np.all(out[0][8] >= 2)    # (the solves ran)


def test_the_other_entry_points_ignore_the_flag():
    """forward_pass, df and costfun of the (34, 17) problem with and without the flag: the same bits"""
    c = wc.case(GEO)
    pol = ddp_amd.GaussianPolicy(c["N"], c["n"], c["m"], c["K"], np.zeros((c["m"], c["N"], c["B"])), np.zeros((0, 0, 0)), np.zeros((0, 0, 0)))
    out = []
    for mode in ("plain", "wave"):
        p = problem(GEO, mode)
        out.append(tuple(ddp_amd.forward_pass(pol, c["x0"], c["u"], c["x"], 1.0, p, None, params=c["params"])) +
                   tuple(np.asarray(a) for a in ddp_amd.df(p, c["x"], c["u"], params=c["params"])) +
                   (ddp_amd.costfun(p, c["x"], c["u"], params=c["params"]),))
    assert len(out[0]) == len(out[1]) == 14 and all(same(a, b) for a, b in zip(*out)) and all(np.all(np.isfinite(a)) for a in out[0])
