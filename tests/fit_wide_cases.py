"""Cases of fit_dynamics(..., wide=True) (tests/test_fit_wide_cpu.py, tests/test_gpu_fit_wide.py), built on the size-agnostic long double
reference of tests/fit_reference.py: no GPU, no library.  Every case is seeded from its name and computed once, with smax = 3.0 given
explicitly (fit_reference.smax_for was derived for d <= 40).  The condition of every step that is expected to succeed stays under
KAPPA_CAP_WIDE = 500, which keeps the first-order bound d (S + d) kappa 2^-53 under fit_reference.TOL for d <= 96, S <= 230."""
import functools

import numpy as np

import fit_reference as fr

KAPPA_CAP_WIDE = 500.0
SMAX = 3.0

# name -> (n, m, N, S, B, prior: None / "shared" / "per_step")
CASES = {
    "33x8": (33, 8, 3, 67, 3, None),                             # n just past the narrow box
    "32x9": (32, 9, 3, 67, 3, None),                             # m just past the narrow box
    "1x32": (1, 32, 2, 67, 2, None),                             # wide by m alone, one state
    "64x1": (64, 1, 2, 130, 2, None),                            # wide by n alone, d = 65
    "40x25": (40, 25, 2, 131, 1, None),                          # d = 65, no dimension a multiple of 16, S = 3 (mod 4)
    "48x16": (48, 16, 3, 130, 1, None),                          # d = 64 exactly, all blocks full
    "64x32": (64, 32, 2, 230, 2, None),                          # the corner; S past one staged chunk (84 samples there)
    "64x32-prior-S2": (64, 32, 3, 2, 2, "per_step"),             # the corner with a per-step prior, S = 2
    "50x31-prior": (50, 31, 2, 63, 1, "shared"),                 # shared prior, S < d
    "33x9-N1": (33, 9, 1, 64, 3, None),                          # N = 1
}


def seed_of(name):
    return sum(map(ord, name)) * 131 + 7


@functools.lru_cache(maxsize=None)
def case(name):
    """dict(n, m, N, S, B, xs, us, ridge, prior, ref) of a designed case; ref is fit_reference.fit(...) on it"""
    n, m, N, S, B, pk = CASES[name]
    seed = seed_of(name)
    xs, us, F, c = fr.designed(n, m, N, S, B, seed, smax=SMAX)
    prior = None if pk is None else fr.designed_prior(n, m, N, B, seed + 1, pk == "per_step")
    return dict(n=n, m=m, N=N, S=S, B=B, xs=xs, us=us, ridge=0.0, prior=prior, ref=fr.fit(xs, us, 0.0, prior))


@functools.lru_cache(maxsize=None)
def ridge_reference(name, ridge):
    c = case(name)
    return fr.fit(c["xs"], c["us"], ridge, c["prior"])


# ---------------------------------------------------------------------------------------------------------------------- status cases
ST_SHAPE = (40, 30, 4, 129, 2)                                   # n, m, N, S, B of the three status cases: no prior, ridge 0
ST_STEP = 2


def _status_inputs():
    n, m, N, S, B = ST_SHAPE
    xs, us, _, _ = fr.designed(n, m, N, S, B, 4270, smax=SMAX)
    return n, m, N, S, B, xs, us


@functools.lru_cache(maxsize=None)
def identical_columns_case():
    """in trajectory 1 at step 2, state 0 and control 26 (column 66 of z: past lane 63 and in another 16-block than column 0) are the
    same exact pattern, 64 samples of +2, 64 of -2, one 0, permuted: A_00 = A_66,0 = A_66,66 = 4 exactly, so pivot 66 is 4 - 2^2 minus
    squares: never positive, whatever the order of the sums.  Expected: status 67 at that step, 0 elsewhere."""
    n, m, N, S, B, xs, us = _status_inputs()
    pat = np.concatenate([np.full(64, 2.0), np.full(64, -2.0), [0.0]])
    pat = pat[np.random.default_rng(1).permutation(S)]
    xs[0, ST_STEP, :, 1] = pat
    us[26, ST_STEP, :, 1] = pat
    expect = np.zeros((N, B), dtype=np.int32)
    expect[ST_STEP, 1] = 67
    return dict(n=n, m=m, N=N, S=S, B=B, xs=xs, us=us, ref=fr.fit(xs, us), expect=expect)


@functools.lru_cache(maxsize=None)
def nan_case(which):
    """one NaN: which = "control": us[20, 2, 17, 1] -> status 61 at step 2 and nothing else; "state": xs[35, 2, 17, 1] -> status 36 at
    step 2 (its z), status 71 = d + 1 at step 1 (its y), nothing else"""
    n, m, N, S, B, xs, us = _status_inputs()
    expect = np.zeros((N, B), dtype=np.int32)
    if which == "control":
        us[20, ST_STEP, 17, 1] = np.nan
        expect[ST_STEP, 1] = n + 20 + 1
    else:
        xs[35, ST_STEP, 17, 1] = np.nan
        expect[ST_STEP, 1] = 35 + 1
        expect[ST_STEP - 1, 1] = n + m + 1
    return dict(n=n, m=m, N=N, S=S, B=B, xs=xs, us=us, ref=fr.fit(xs, us), expect=expect)


STATUS_CASES = {"identical-columns": identical_columns_case, "nan-control": lambda: nan_case("control"), "nan-state": lambda: nan_case("state")}
