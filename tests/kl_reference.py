"""np.longdouble restatement of the three KL operations of csrc/kl.hip, written from the Julia semantics (the way oracle/np_kl.py is):
    ∇kl                 src/klutils.jl:8-23
    forward_covariance  src/forward_pass.jl:37-56
    kl_div_wiki         src/klutils.jl:70-103
and of back_pass_gps without limits (src/backward_pass.jl:259-350) for one trajectory.
No tests here.  Every function takes the arrays of ONE trajectory or, with a trailing axis, of a batch (every trajectory is computed
independently, in one vectorised sweep: the B = 6145 case of tests/kl_narrow_cases.py is one call).  Inputs are float64 values taken
exactly; every operation on them is long double, so what comes back is the float64 problem's answer to ~1e-19 — the yardstick both the
kernels and the C oracle (oracle/ddp_oracle_kl.c) are measured with.  Callers skip through need_longdouble() where long double is no
wider than double."""
import numpy as np
import pytest

LD = np.longdouble


def need_longdouble():
    if np.finfo(LD).eps >= 2e-16:
        pytest.skip("np.longdouble is no wider than float64 on this host (eps = %g)" % np.finfo(LD).eps)


def _ld(a, nd):
    """long double copy with a batch axis: rank nd -> nd + 1"""
    a = np.asarray(a, dtype=np.float64).astype(LD)
    return (a[..., None], False) if a.ndim == nd else (a, True)


def _out(arrs, batched):
    return arrs if batched else tuple(a[..., 0] for a in arrs)


def grad_kl(K, k, Si):
    """∇kl(traj_prev) -> cx[n,T], cu[m,T], cxx[n,n,T], cxu[m,n,T] (sic), cuu[m,m,T]   (klutils.jl:14-20)"""
    (K, bt), (k, _), (Si, _) = _ld(K, 3), _ld(k, 2), _ld(Si, 3)
    Sik = np.einsum("abtz,btz->atz", Si, k)                       # Σi k
    SiK = np.einsum("abtz,bjtz->ajtz", Si, K)                     # Σi K
    cx = np.einsum("ajtz,atz->jtz", K, Sik)                       # K'Σi k
    cxx = np.einsum("artz,ajtz->rjtz", K, SiK)                    # K'Σi K
    return _out((cx, -Sik, cxx, -SiK, Si.copy()), bt)


def forward_covariance(fx, R1, K, Sigma):
    """sigmanew[(n+m),(n+m),N]: the chain Σ⁺ = (fx Σ) fx' + R1 from Σ0 = R1 (:43,:50), the policy blocks of steps 1..N-1 (:51-53);
    the last step has no policy block (`undef` upstream: zero here).  fx[n,n,N] serves every trajectory of a batch."""
    (K, bt), (Sigma, _) = _ld(K, 3), _ld(Sigma, 3)
    fx = np.asarray(fx, dtype=np.float64).astype(LD)
    R1 = np.asarray(R1, dtype=np.float64).astype(LD)
    m, n, N, B = K.shape
    F4 = fx if fx.ndim == 4 else np.broadcast_to(fx[..., None], fx.shape + (B,))
    S = np.zeros((n + m, n + m, N, B), dtype=LD)
    Sxx = np.repeat(R1[:, :, None], B, 2)
    for i in range(N):
        S[:n, :n, i] = Sxx
        if i == N - 1:
            break
        F, Ki = F4[:, :, i], K[:, :, i]
        KS = np.einsum("alz,lcz->acz", Ki, Sxx)
        S[n:, :n, i] = KS                                                         # K Σ
        S[:n, n:, i] = np.einsum("rlz,alz->raz", Sxx, Ki)                         # Σ K'
        S[n:, n:, i] = np.einsum("alz,blz->abz", KS, Ki) + Sigma[:, :, i]         # (K Σ) K' + Σ_policy
        T1 = np.einsum("rlz,lcz->rcz", F, Sxx)                                    # fx Σ
        Sxx = np.einsum("rlz,clz->rcz", T1, F) + R1[:, :, None]                   # (fx Σ) fx' + R1
    return S if bt else S[..., 0]


def lu_logdet(A, trace=None):
    """log|det A| and the sign of det A of every matrix A[m,m,X], by Gaussian elimination with partial pivoting (the first largest
    magnitude of a column is its pivot, as LAPACK's idamax).  A zero pivot: (-Inf, 0) — logdet of a singular matrix is -Inf and
    does not throw; sign -1 is what makes logdet throw.  `trace`, a list, receives per column the magnitudes the pivot was chosen
    from ([m - c, X]) and the chosen row."""
    A = np.array(A, dtype=LD)
    m, _, X = A.shape
    ar = np.arange(X)
    ld, sgn, alive = np.zeros(X, dtype=LD), np.ones(X, dtype=int), np.ones(X, dtype=bool)
    for c in range(m):
        mag = np.abs(A[c:, c, :])
        pr = c + np.argmax(mag, axis=0)
        if trace is not None:
            trace.append((mag.copy(), pr.copy()))
        rc, rp = A[c, :, ar].copy(), A[pr, :, ar].copy()               # [X, m]: rows c and pr of every matrix
        A[c, :, ar], A[pr, :, ar] = rp, rc
        sgn = np.where(alive & (pr != c), -sgn, sgn)
        d = A[c, c, :].copy()
        alive &= d != 0
        sgn = np.where(alive & (d < 0), -sgn, sgn)
        d[~alive] = 1
        ld = ld + np.log(np.abs(d))
        f = A[c + 1:, c, :] / d
        A[c + 1:, c + 1:, :] -= f[:, None, :] * A[c, c + 1:, :][None, :, :]
    return np.where(alive, ld, -np.inf), np.where(alive, sgn, 0)


def kl_div_wiki(xnew, xold, sig, Kn, kn, Sn, Kp, kp, Sp, Sip):
    """kl_div_wiki (klutils.jl:70-103) -> (kldiv[T], mean, threw): the per-step divergences after max(0, ·) — a NaN step stays NaN —
    their mean over time as calc_η takes it (:112), and whether a logdet threw (a negative determinant at any step): the reference
    then returns the scalar Inf for the whole call, so the mean is +Inf (kldiv keeps the steps' own values)."""
    (xnew, bt), (xold, _), (sig, _) = _ld(xnew, 2), _ld(xold, 2), _ld(sig, 3)
    (Kn, _), (kn, _), (Sn, _), (Kp, _), (kp, _), (Sp, _), (Sip, _) = (_ld(Kn, 3), _ld(kn, 2), _ld(Sn, 3), _ld(Kp, 3), _ld(kp, 2),
                                                                    _ld(Sp, 3), _ld(Sip, 3))
    m, n, T, B = Kn.shape
    mu, kd, Kd = xnew - xold, kp - kn, Kp - Kn
    St = sig[:n, :n]
    ldp, sp = lu_logdet(Sp.reshape(m, m, T * B))
    ldn, sn = lu_logdet(Sn.reshape(m, m, T * B))
    ldp, ldn, threw = ldp.reshape(T, B), ldn.reshape(T, B), ((sp < 0) | (sn < 0)).reshape(T, B).any(axis=0)
    with np.errstate(invalid="ignore"):
        v = (np.einsum("abtz,batz->tz", Sip, Sn) + np.einsum("atz,abtz,btz->tz", kd, Sip, kd) - m + ldp - ldn) / 2          # :89
        Kmu = np.einsum("ajtz,jtz->atz", Kd, mu)
        SKd = np.einsum("abtz,bjtz->ajtz", Sip, Kd)
        M = np.einsum("artz,actz->rctz", Kd, SKd)                                            # K_diff'Σip K_diff
        v = v + (np.einsum("atz,abtz,btz->tz", Kmu, Sip, Kmu) + np.einsum("rctz,crtz->tz", M, St)) / 2                       # :90
        v = v + np.einsum("atz,abtz,btz->tz", kd, Sip, Kmu)                                  # :91
        kld = np.where(v <= 0, LD(0), v)                                                     # max.(0, kldiv): NaN propagates (:98)
        mean = np.where(threw, LD(np.inf), kld.sum(axis=0) / T)
    return (kld, mean, threw) if bt else (kld[:, 0], mean[0], bool(threw[0]))


def _spd_solve(Q, rhs):
    """Q \\ rhs for a symmetric positive definite Q by Cholesky, in long double (numpy.linalg has no long double)"""
    m = Q.shape[0]
    Lo = np.zeros((m, m), dtype=LD)
    for j in range(m):
        d = Q[j, j] - Lo[j, :j] @ Lo[j, :j]
        assert d > 0, "the case is meant to be positive definite"
        Lo[j, j] = np.sqrt(d)
        for i in range(j + 1, m):
            Lo[i, j] = (Q[i, j] - Lo[i, :j] @ Lo[j, :j]) / Lo[j, j]
    y = np.array(rhs, dtype=LD)
    for i in range(m):
        y[i] = (y[i] - Lo[i, :i] @ y[:i]) / Lo[i, i]
    for i in range(m - 1, -1, -1):
        y[i] = (y[i] - Lo[i + 1:, i] @ y[i + 1:]) / Lo[i, i]
    return y


def back_pass_gps(cx, cu, cxx, cxu, cuu, fx, fu, terms, eta):
    """back_pass_gps of one trajectory without limits, every Quu positive definite -> K, k, Quui, Quu, Vx, Vxx, dV.  terms: ∇kl of the
    trajectory (cxu as [m,n,N]); eta: ηbracket[2], a scalar or [N]"""
    cx, cu, cxx, cxu, cuu, fx, fu = [np.asarray(a, dtype=np.float64).astype(LD) for a in (cx, cu, cxx, cxu, cuu, fx, fu)]
    kx, ku, kxx, kux, kuu = [np.asarray(a, dtype=np.float64).astype(LD) for a in terms]
    eta = np.broadcast_to(np.asarray(eta, dtype=np.float64).astype(LD), (cx.shape[1],))
    (n, N), m = cx.shape, cu.shape[0]
    K, k = np.zeros((m, n, N), dtype=LD), np.zeros((m, N), dtype=LD)
    Vx, Vxx = np.zeros((n, N), dtype=LD), np.zeros((n, n, N), dtype=LD)
    Quu, Quui, dV = np.zeros((m, m, N), dtype=LD), np.zeros((m, m, N), dtype=LD), np.zeros(2, dtype=LD)
    Vx[:, -1], Vxx[:, :, -1] = cx[:, -1], cxx[:, :, -1]
    Quu[:, :, -1] = cuu[:, :, -1] / eta[-1] + kuu[:, :, -1]
    Quui[:, :, -1] = _spd_solve(Quu[:, :, -1], np.eye(m))
    for i in range(N - 2, -1, -1):
        F, G, V, e = fx[:, :, i], fu[:, :, i], Vxx[:, :, i + 1], eta[i]
        Qu = (cu[:, i] + G.T @ Vx[:, i + 1]) / e + ku[:, i]
        Qx = (cx[:, i] + F.T @ Vx[:, i + 1]) / e + kx[:, i]
        Qux = (cxu[:, :, i].T + G.T @ V @ F) / e + kux[:, :, i]
        Q = (cuu[:, :, i] + G.T @ V @ G) / e + kuu[:, :, i]
        Qxx = (cxx[:, :, i] + F.T @ V @ F) / e + kxx[:, :, i]
        Q = (Q + Q.T) / 2
        ki, Ki = -_spd_solve(Q, Qu), -_spd_solve(Q, Qux)
        dV = dV + np.array([ki @ Qu, ki @ Q @ ki / 2])
        Vx[:, i] = Qx + Ki.T @ Q @ ki + Ki.T @ Qu + Qux.T @ ki
        M = Qxx + Ki.T @ Q @ Ki + Ki.T @ Qux + Qux.T @ Ki
        Vxx[:, :, i], k[:, i], K[:, :, i], Quu[:, :, i], Quui[:, :, i] = (M + M.T) / 2, ki, Ki, Q, _spd_solve(Q, np.eye(m))
    return dict(K=K, k=k, Quui=Quui, Quu=Quu, Vx=Vx, Vxx=Vxx, dV=dV)
