"""np.longdouble restatement of the `df` closure of the two registered families — what csrc/df.hip and the C oracle
(oracle/ddp_oracle.c, ddp_oracle_df / ddp_oracle_expm) are measured with.  No tests here.

  pendcart   system_pendcart.jl:108-154: cx = Q (x - goal), cu = R u with NaN controls read as zero, and the ZoH block matrix
             [fxc h  fuc h; 0] with its exponential.  The exponential is NOT the algorithm of the kernel and the oracle (Higham's Padé
             scaling and squaring): it is the Taylor series, summed by Horner's rule, of the matrix scaled by a power of two to a 1-norm
             of at most 1/8, followed by the squarings.  A mistake the kernel and the oracle share does not pass here.
  LQ         demo_linear.jl:35-41: cx = Q x, cu = R u.

Distances.  One element (t, b) of fx / fu: max|got - ref| / max|ref| over that element's own 4 x 5 block [fx fu] — normwise per
matrix, which is what a Padé approximant promises; a norm over the whole array lets one large element hide every small one.
cx, cu, LQ: |got - ref| / (|Q| |x|) row by row, the matrix-vector product's own error scale.

Callers skip through need_longdouble() where long double is no wider than double."""
import numpy as np
import pytest

LD = np.longdouble
TAYLOR_TERMS = 24          # norm <= 1/8: term 24 is below 8^-24 / 24! = 3e-46 of the sum
BANDS = (0.015, 0.25, 0.95, 2.1, 5.4, 10.8, 43.0, 700.0, 3e4)          # upper ends; band i is (BANDS[i-1], BANDS[i]], band 0 starts at 0


def need_longdouble():
    if np.finfo(LD).eps >= 2e-16:
        pytest.skip("np.longdouble is no wider than float64 on this host (eps = %g)" % np.finfo(LD).eps)


def band_of(norm):
    """index into BANDS of a 1-norm; a norm beyond the last band is an error of the caller"""
    for i, hi in enumerate(BANDS):
        if norm <= hi:
            return i
    raise ValueError("norm %r lies in no band" % (norm,))


def expm_ld(M):
    """exp of M[..., D, D] (any float type) in long double: scale by 2^-s to a 1-norm <= 1/8, Taylor by Horner, s squarings"""
    A = np.asarray(M).astype(LD)
    D = A.shape[-1]
    nrm = np.abs(A).sum(axis=-2).max(axis=-1).astype(np.float64)              # 1-norm: the largest column sum
    s = np.zeros(nrm.shape, dtype=int)
    big = nrm > 0.125
    s[big] = np.ceil(np.log2(nrm[big] * 8.0)).astype(int)
    s[big & (np.ldexp(nrm, -s) > 0.125)] += 1                                # (log2 rounded down at a power of two)
    A = A * np.ldexp(LD(1), -s)[..., None, None]                             # exact
    eye = np.broadcast_to(np.eye(D, dtype=LD), A.shape)
    E = eye.copy()
    for k in range(TAYLOR_TERMS, 0, -1):                                      # I + A/1 (I + A/2 (I + ... ))
        E = eye + np.matmul(A, E) / LD(k)
    for q in range(int(s.max()) if s.size else 0):
        E = np.where((s > q)[..., None, None], np.matmul(E, E), E)
    return E


def pend_matrix_ld(par, x0, u):
    """the 5 x 5 block matrix of system_pendcart.jl:137-148 for angles x0[...] and controls u[...] (NaN read as zero), in long double"""
    g, l, h, d = (LD(par[k]) for k in ("g", "l", "h", "d"))
    th = np.asarray(x0, dtype=np.float64).astype(LD)
    uu = np.asarray(u, dtype=np.float64).astype(LD)
    uu = np.where(np.isnan(uu), LD(0), uu)
    M = np.zeros(th.shape + (5, 5), dtype=LD)
    M[..., 0, 1] = h
    M[..., 1, 0] = (-g / l * np.cos(th) - uu / l * np.sin(th)) * h
    M[..., 1, 1] = -d * h
    M[..., 2, 3] = h
    M[..., 1, 4] = np.cos(th) / l * h
    M[..., 3, 4] = h
    return M


def pend_df_ld(par, x, u):
    """x[4, ...], u[...] or u[1, ...] -> fx[4, 4, ...], fu[4, 1, ...], cx[4, ...], cu[1, ...] and the error scales of cx, cu ([4, ...], [1, ...]),
    all long double.  par: g, l, h, d, goal[4], Q[4, 4], R[1, 1]"""
    x = np.asarray(x, dtype=np.float64).astype(LD)
    uu = np.asarray(u, dtype=np.float64).astype(LD)
    uu = np.where(np.isnan(uu), LD(0), uu).reshape(x.shape[1:])
    Q = np.asarray(par["Q"], dtype=np.float64).astype(LD)
    R = LD(np.asarray(par["R"], dtype=np.float64).ravel()[0])
    dx = x - np.asarray(par["goal"], dtype=np.float64).astype(LD).reshape((4,) + (1,) * (x.ndim - 1))
    cx = np.tensordot(Q, dx, axes=(1, 0))
    cxs = np.tensordot(np.abs(Q), np.abs(dx), axes=(1, 0))
    cu = (R * uu)[None]
    E = expm_ld(pend_matrix_ld(par, x[0], uu))
    fx = np.moveaxis(E[..., :4, :4], (-2, -1), (0, 1))
    fu = np.moveaxis(E[..., :4, 4:5], (-2, -1), (0, 1))
    return fx, fu, cx, cu, cxs, np.abs(cu)


def lq_df_ld(Q, R, x, u):
    """x[n, ...], u[m, ...] -> cx, cu and their error scales |Q||x|, |R||u|, long double; NaN controls read as zero"""
    Q = np.asarray(Q, dtype=np.float64).astype(LD); R = np.asarray(R, dtype=np.float64).astype(LD)
    x = np.asarray(x, dtype=np.float64).astype(LD); u = np.asarray(u, dtype=np.float64).astype(LD)
    u = np.where(np.isnan(u), LD(0), u)
    sh_x, sh_u = x.shape, u.shape
    x2, u2 = x.reshape(sh_x[0], -1), u.reshape(sh_u[0], -1)
    return ((Q @ x2).reshape(sh_x), (R @ u2).reshape(sh_u), (np.abs(Q) @ np.abs(x2)).reshape(sh_x), (np.abs(R) @ np.abs(u2)).reshape(sh_u))


def block_distance(fx, fu, fx_ref, fu_ref):
    """per element: max|got - ref| / max|ref| over the 4 x 5 block [fx fu]; fx[4, 4, ...], fu[4, 1, ...] -> float64[...]"""
    got = np.concatenate([np.asarray(fx).astype(LD), np.asarray(fu).astype(LD)], axis=1)
    ref = np.concatenate([fx_ref, fu_ref], axis=1)
    num = np.abs(got - ref).max(axis=(0, 1))
    den = np.abs(ref).max(axis=(0, 1))
    return (num / den).astype(np.float64)


def row_distance(got, ref, scale):
    """|got - ref| / scale entry by entry; where the scale is zero the entry has to be exact (distance 0 or inf)"""
    err = np.abs(np.asarray(got).astype(LD) - ref)
    out = np.where(scale > 0, err / np.where(scale > 0, scale, LD(1)), np.where(err == 0, LD(0), LD(np.inf)))
    return out.astype(np.float64)
