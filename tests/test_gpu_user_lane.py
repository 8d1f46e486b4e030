"""The default (lane) user-problem kernels on the GPU over every launch layout layout_of picks: ddp_user_rollout, ddp_user_df /
ddp_user_df_ad, ddp_user_hessians and ddp_user_cost against the long-double references of tests/user_lane_cases.py, at sizes read from
the layout (a last chunk shorter than DDP_CHUNK, work-groups over an α boundary, over two trajectories, over an inactive next to an
active one, fewer rollouts than slots).  The `_dev` entries are called on sentinel-filled outputs (the method of
tests/test_gpu_forward_contract.py): what an inactive trajectory owns keeps its bits, and a rollout's result depends neither on the α's
nor on the trajectories it shares its work-group with.  tests/test_user_lane_cpu.py guards the cases themselves.

Measured on one MI355X, worst over all cases (relerr per time step): x 4.7e-13 (lq (1, 1), a scalar state at a zero crossing; 3.2e-15
elsewhere), u 7.4e-13 (pendcart, the 2π reduction), c 6.8e-15, csum 5.4e-16; derivatives 6.7e-16 (lq), 3.7e-15 (car); ddp_user_cost
8.6e-16, its csum 2.3e-16."""
import numpy as np
import pytest

import user_lane_cases as lc
from conftest import relerr
from user_lane_cases import SENT, bits

pytestmark = pytest.mark.gpu
RTOL = 1e-10                                                         # per time step, as test_rollout_contract of tests/test_gpu_user_wave.py
LD = np.longdouble


@pytest.fixture(scope="module")
def ddp():
    import ddp_amd
    return ddp_amd


@pytest.fixture(scope="module")
def problems(ddp):
    """one compiled program per shape and module"""
    made = {}

    def get(key):
        if key not in made:
            made[key] = lc.make_problem(ddp, key)
        return made[key]
    return get


def same_bits(a, b):
    return np.array_equal(bits(a), bits(b))


def slice_picks(B):
    """the trajectories whose B = 1 call is compared: all of a small batch, of 70 the ones around the slot counts 16, 32 and 64"""
    return range(B) if B <= 23 else (0, 1, 15, 16, 31, 32, 33, 63, 64, 69)


# ------------------------------------------------------------------------------------------------------------------------ rollout
@pytest.mark.parametrize("B,na", lc.BNA)
@pytest.mark.parametrize("key", lc.ROLL_SHAPES)
def test_rollout_contract(ddp, problems, key, B, na):
    """every N of the shape at this (B, nα): the kernel's name; xnew, unew, cnew against long double at 1e-10 per time step; csum against
    the long-double sum of the device's cnew within CL 2^-52 Σ|c| (not bit for bit: the compiler may fuse the cost's last multiply-add
    into the running sum, tests/test_gpu_user_fitted.py); NULL and all-ones masks the same bits; under the mask with holes the inactive
    rows of all four outputs keep the sentinel and the active ones their bits; unew inside the limits exactly; column ai the one-α call,
    trajectory b the B = 1 call, bit for bit; the terminal slot of cnew only for terminal problems"""
    prob = problems(key)
    mdl = lc.model_of(key)
    worst = [0.0] * 4
    for spec in lc.roll_cases(key):
        if spec[1:3] != (B, na):
            continue
        c = lc.roll_case(key, *spec)
        N, prm, K, k, x0, u, x, alpha, lims = (c[s] for s in ("N", "prm", "K", "k", "x0", "u", "x", "alpha", "lims"))
        out = lc.dev_rollout(ddp, prob, prm, K, k, x0, u, x, alpha, lims, None)
        assert out[4] == "ddp_user_rollout", out[4]
        xn, un, cn, cs = out[:4]
        CL = N + 1 if lc.SHAPES[key][4].get("terminal") else N
        assert cn.shape == (CL, B, na), (spec, cn.shape)
        assert not any(np.isnan(a).any() for a in out[:4]), (spec, "an active rollout left a sentinel")
        # ---- the masks
        ones = lc.dev_rollout(ddp, prob, prm, K, k, x0, u, x, alpha, lims, np.ones(B, np.int32))
        for i in range(4):
            assert same_bits(out[i], ones[i]), (spec, i, "all ones differs from NULL")
        act = lc.holes(B)
        on = act != 0
        got = lc.dev_rollout(ddp, prob, prm, K, k, x0, u, x, alpha, lims, act)
        for i in range(4):
            assert np.all(bits(got[i][..., ~on, :]) == SENT[i]), (spec, i, "an inactive trajectory was written")
            assert same_bits(got[i][..., on, :], out[i][..., on, :]), (spec, i, "active rows differ under the mask")
        # ---- the reference
        xr, ur, cr = c["ref"]
        for b in range(B):
            for ai in range(na):
                e = (relerr(xn[:, :, b, ai], xr[:, :, b, ai]), relerr(un[:, :, b, ai], ur[:, :, b, ai]), relerr(cn[:, b, ai], cr[:, b, ai], 0))
                worst[:3] = [max(w, v) for w, v in zip(worst, e)]
                assert max(e) < RTOL, (spec, b, ai, e)
        acc, mag = np.zeros((B, na), LD), np.zeros((B, na), LD)
        for t in range(CL):
            acc, mag = acc + cn[t].astype(LD), mag + np.abs(cn[t]).astype(LD)
        cerr = float(np.max(np.abs(cs - acc) / mag))
        worst[3] = max(worst[3], cerr)
        assert cerr <= CL * 2.0 ** -52, (spec, cerr)
        if CL > N:                                                   # row N: the terminal cost of xnew[:, N-1]
            for b in range(B):
                tc = mdl[2](xn[:, N - 1, b, :].astype(LD), np.asarray(prm[:, b] if c["batched"] else prm, LD))
                assert np.max(np.abs(cn[N, b] - tc) / np.abs(tc)) < RTOL, (spec, b)
        if lims is not None:
            lo, hi = lims[:, 0, None, None, None], lims[:, 1, None, None, None]
            assert np.all(un >= lo) and np.all(un <= hi), spec
            assert ((un == lo) | (un == hi)).any() and ((un > lo) & (un < hi)).any(), spec
        # ---- a rollout's result does not depend on its slot: one α at a time, one trajectory at a time
        if na > 1:
            for ai in range(na):
                one = lc.dev_rollout(ddp, prob, prm, K, k, x0, u, x, alpha[ai:ai + 1], lims, None)
                for i in range(4):
                    assert same_bits(one[i][..., 0], out[i][..., ai]), (spec, ai, i, "column ai differs from the one-α call")
        if B > 1:
            for b in slice_picks(B):
                s = slice(b, b + 1)
                pol = (None, None) if K is None else (K[..., s], k[..., s])
                one = lc.dev_rollout(ddp, prob, prm[:, s] if c["batched"] else prm, *pol, x0[:, s], u[..., s], None if x is None else x[..., s],
                                     alpha, lims, None)
                for i in range(4):
                    assert same_bits(one[i][..., 0, :], out[i][..., b, :]), (spec, b, i, "trajectory b differs from the B = 1 call")
    print("%s %s B=%d na=%d: worst relerr x %.2e u %.2e c %.2e, csum %.2e" % (key, lc.layout(key), B, na, *worst))


# -------------------------------------------------------------------------------------------------------------------- derivatives
@pytest.mark.parametrize("key", lc.DF_SHAPES)
def test_derivative_contract(ddp, problems, key):
    """ddp_user_df / ddp_user_df_ad (and ddp_user_hessians of a const_hessian problem) on every (N, B) of the shape: all seven arrays
    against the reference; NULL and all-ones masks the same bits; under the mask with holes the inactive rows (columns of the [., ., B]
    Hessians) keep the sentinel and the active ones their bits; trajectory b is the B = 1 call bit for bit; with NULL Hessian outputs
    the same fx, fu, cx, cu and nothing else"""
    prob = problems(key)
    kw = lc.SHAPES[key][4]
    ch = bool(kw.get("const_hessian"))
    kernel = "ddp_user_df_ad" if kw.get("autodiff") else "ddp_user_df"
    tol = lc.df_tolerance(key)
    worst = 0.0
    for N, B in lc.df_NB(key):
        c = lc.df_case(key, N, B)
        prm, x, u = c["prm"], c["x"], c["u"]
        full = lc.dev_df(ddp, prob, prm, x, u, None)
        assert full[7] == ("ddp_user_hessians" if ch else kernel), full[7]
        assert not any(np.isnan(a).any() for a in full[:7]), (N, B, "an active row left a sentinel")
        bare = lc.dev_df(ddp, prob, prm, x, u, None, hessians=False)
        assert bare[7] == kernel, bare[7]
        for i in range(4):
            assert same_bits(bare[i], full[i]), (N, B, i, "NULL Hessian outputs change the rest")
        for i in range(4, 7):
            assert np.all(bits(bare[i]) == SENT[i]), (N, B, i)
        ones = lc.dev_df(ddp, prob, prm, x, u, np.ones(B, np.int32))
        for i in range(7):
            assert same_bits(ones[i], full[i]), (N, B, i, "all ones differs from NULL")
        act = lc.holes(B)
        on = act != 0
        got = lc.dev_df(ddp, prob, prm, x, u, act)
        for i in range(7):
            assert np.all(bits(got[i][..., ~on]) == SENT[i]), (N, B, i, "an inactive trajectory was written")
            assert same_bits(got[i][..., on], full[i][..., on]), (N, B, i, "active rows differ under the mask")
        for b in range(B):
            for i, ref in enumerate(c["ref"]):
                g, r = full[i][..., b], ref[..., b]
                if ch and i >= 4:
                    r = r[..., 0]
                if np.any(r):
                    e = relerr(g, r) if (g.ndim > 1 and not (ch and i >= 4)) else float(np.max(np.abs(g - r)) / np.max(np.abs(r)))
                    worst = max(worst, e)
                    assert e < tol, (N, B, b, i, e)
                else:
                    assert not np.any(g), (N, B, b, i)
        if B > 1:
            for b in range(B) if B <= 3 else (0, 1, B // 2, B - 2, B - 1):
                s = slice(b, b + 1)
                one = lc.dev_df(ddp, prob, prm[:, s] if c["batched"] else prm, x[..., s], u[..., s], None)
                for i in range(7):
                    assert same_bits(one[i][..., 0], full[i][..., b]), (N, B, b, i, "trajectory b differs from the B = 1 call")
    print("%s %s: worst relerr of the derivatives %.2e (bound %.0e)" % (key, lc.layout(key), worst, tol))


# --------------------------------------------------------------------------------------------------------------------------- cost
@pytest.mark.parametrize("key", lc.COST_SHAPES)
def test_cost_contract(ddp, problems, key):
    """ddp_user_cost, one wave per trajectory with the lanes over CL = N (+ 1) slots, CL on, one past and two rounds past the 64 lanes:
    cost against long double; csum against the long-double sum of the device's cost within (6 + ceil(CL / 64)) 2^-53 Σ|c|; csum = NULL
    leaves cost as it is; the mask rules"""
    prob = problems(key)
    worst = [0.0, 0.0]
    for N in lc.COST_N:
        c = lc.cost_case(key, N)
        prm, x, u, B = c["prm"], c["x"], c["u"], c["B"]
        cost, csum, name = lc.dev_cost(ddp, prob, prm, x, u, None)
        assert name == "ddp_user_cost", name
        CL = c["ref"].shape[0]
        assert cost.shape == (CL, B) and not np.isnan(cost).any() and not np.isnan(csum).any(), N
        for b in range(B):
            e = relerr(cost[:, b], c["ref"][:, b], 0)
            worst[0] = max(worst[0], e)
            assert e < RTOL, (N, b, e)
        acc = cost.astype(LD).sum(axis=0)
        mag = np.abs(cost).astype(LD).sum(axis=0)
        cerr = float(np.max(np.abs(csum - acc) / mag))
        worst[1] = max(worst[1], cerr)
        assert cerr <= lc.cost_csum_bound(CL), (N, cerr, lc.cost_csum_bound(CL))
        bare = lc.dev_cost(ddp, prob, prm, x, u, None, csum=False)
        assert same_bits(bare[0], cost) and np.all(bits(bare[1]) == SENT[1]), (N, "csum = NULL")
        ones = lc.dev_cost(ddp, prob, prm, x, u, np.ones(B, np.int32))
        assert same_bits(ones[0], cost) and same_bits(ones[1], csum), (N, "all ones differs from NULL")
        act = lc.holes(B)
        on = act != 0
        got = lc.dev_cost(ddp, prob, prm, x, u, act)
        for i, full in enumerate((cost, csum)):
            assert np.all(bits(got[i][..., ~on]) == SENT[i]), (N, i, "an inactive trajectory was written")
            assert same_bits(got[i][..., on], full[..., on]), (N, i, "active rows differ under the mask")
    print("%s: worst relerr of cost %.2e, csum %.2e" % (key, *worst))
