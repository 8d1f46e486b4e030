"""KL-constrained path (BASELINE config 5) behind the reference's call signatures.

    ∇kl(traj_prev)                                                   src/klutils.jl:8-23
    back_pass_gps(cx,cu,cxx,cxu,cuu,fx,fu,lims,x,u,kl_cost_terms)    src/backward_pass.jl:259-350
    forward_covariance(model,x,u,traj)                               src/forward_pass.jl:37-56
    kl_div_wiki(xnew,xold,Σ_new,traj_new,traj_prev)                  src/klutils.jl:70-103
    calc_η(xnew,xold,sigmanew,ηbracket,traj_new,traj_prev,kl_step)   src/klutils.jl:112-133   (scalar kl_step)
    iLQGkl(problem,x0,traj_prev,model; kl_step, ...)                 src/iLQGkl.jl:25-178,234-252 (single KL constraint)

All array work runs in libddp_amd.so (HIP kernels of csrc/back_pass.hip [GPS variant] and csrc/kl.hip), and so does the
outer loop of iLQGkl with its per-trajectory η bracket (``ddp_ilqgkl_f64``).  A trailing
axis is the batch of independent trajectories.  No CPU fallback.

`model`: the reference calls `df(model,x,u)` and `covariance(model,x,u)` of the un-vendored LinearTimeVaryingModelsBase;
here the model is ``Model(fx[n,n,N(,B)], fu[n,m,N(,B)], R1[n,n])`` — the arrays those calls would return (with a
``DeviceProblem``, ``Model(None, None, R1)``: the problem's own linearisation at x0, traj_prev.k) — and
``model_covariance`` is this build's documented choice for `covariance` (empirical covariance of the one-step
prediction residuals, the inline comment at forward_pass.jl:42).  The per-time-step branch (`constrain_per_step`,
iLQGkl.jl:180-232) is not offloaded.

Shapes: n <= 32, m <= 8.  ``wide=True`` on ``grad_kl``, ``back_pass_gps``, ``forward_covariance``, ``kl_div_wiki``, ``calc_η``,
``iLQGkl`` and ``demo_linear_kl`` opens n <= 64, m <= 32 (``ddp_kl_set_wide``: the shapes beyond the small box run on the kernels of
csrc/kl_wide.hip and the GPS instantiation of csrc/back_pass_wide.hip; smaller shapes keep their kernels).  The keyword sets the
handle's switch for the duration of the call and puts the previous value back.  Extents are checked before anything is launched.
"""
from __future__ import annotations

import contextlib as _contextlib
import ctypes as _C
from dataclasses import dataclass

import numpy as np

from . import _lib
from . import DDPError, DeviceProblem, GaussianPolicy, _clock, _DevProblem, _fitted_tables, _lims, _user_shapes, default_handle, df, forward_pass

__all__ = ["Model", "grad_kl", "∇kl", "back_pass_gps", "forward_covariance", "kl_div_wiki", "calc_η", "geom", "iLQGkl",
           "model_covariance", "demo_linear_kl", "kl_step_adjust"]


@dataclass
class Model:
    fx: np.ndarray          # [n,n,N] or [n,n,N,B]
    fu: np.ndarray          # [n,m,N] or [n,m,N,B]  (only used by model_covariance)
    R1: np.ndarray          # [n,n]
    fc: np.ndarray = None   # [n,N] or [n,N,B]: the offsets of a fitted model x[i+1] = fx x + fu u + fc (``iLQGkl(..., fitted=True)``)


MAX_N, MAX_M, MAX_N_WIDE, MAX_M_WIDE = 32, 8, 64, 32      # DDP_MAX_N_GENERIC, DDP_MAX_M; with the switch: 64, DDP_MAX_M_WIDE


def _kl_box(who, n, m, wide):
    """the shape box of the KL functions, checked before any launch (and before the handle is touched)"""
    nmax, mmax = (MAX_N_WIDE, MAX_M_WIDE) if wide else (MAX_N, MAX_M)
    if not (1 <= n <= nmax and 1 <= m <= mmax):
        raise DDPError("%s: n=%d m=%d has no back_pass_gps kernel (n <= %d, m <= %d; wide=True: n <= %d, m <= %d)"
                       % (who, n, m, MAX_N, MAX_M, MAX_N_WIDE, MAX_M_WIDE))


@_contextlib.contextmanager
def _wide(h, on):
    """``wide=True``: the handle's ddp_kl_set_wide switch is on inside the block; the previous value comes back in any case"""
    if not on:
        yield
        return
    was = h.set_kl_wide(True)
    try:
        yield
    finally:
        h.set_kl_wide(was)


@_contextlib.contextmanager
def _steps(h, steps):
    """``kl_step`` with one value per trajectory: the handle's table (ddp_kl_set_steps) holds them inside the block and is cleared on
    every way out"""
    if steps is None:
        yield
        return
    _lib.check(_lib.lib().ddp_kl_set_steps_f64(h.raw, int(steps.size), _lib.ptr(steps)))
    try:
        yield
    finally:
        _lib.check(_lib.lib().ddp_kl_set_steps_f64(h.raw, 0, None))


def _b(a, nd):
    """append a unit batch axis to an unbatched array of rank nd"""
    a = _lib.f64(a)
    return a.reshape(a.shape + (1,)) if a.ndim == nd else a


def grad_kl(traj_prev, *, handle=None, wide=False):
    """``∇kl(traj_prev)`` -> ``(cx,cu,cxx,cxu,cuu)`` with ``cxu`` of shape [m,n,T] like the reference (klutils.jl:20);
    ``(0,0,0,0,0)`` for an empty policy (:9)."""
    if traj_prev is None or traj_prev.isempty():
        return (0, 0, 0, 0, 0)
    h = handle or default_handle()
    batched = np.ndim(traj_prev.K) == 4
    K, k, Si = _b(traj_prev.K, 3), _b(traj_prev.k, 2), _b(traj_prev.Σi, 3)
    m, n, T, B = K.shape
    _kl_box("∇kl", n, m, wide)
    cx = _lib.result_array((n, T, B)); cu = _lib.result_array((m, T, B)); cxx = _lib.result_array((n, n, T, B))
    cxu = _lib.result_array((m, n, T, B)); cuu = _lib.result_array((m, m, T, B))
    with _wide(h, wide):
        _lib.check(_lib.lib().ddp_kl_terms_f64(h.raw, n, m, T, B, *map(_lib.ptr, (K, k, Si, cx, cu, cxx, cxu, cuu))))
    out = (cx, cu, cxx, cxu, cuu)
    return out if batched else tuple(a[..., 0] for a in out)


globals()["∇kl"] = grad_kl


def back_pass_gps(cx, cu, cxx, cxu, cuu, fx, fu, lims, x, u, kl_cost_terms, *, handle=None, wide=False):
    """Drop-in for ``back_pass_gps(cx,cu,cxx,cxu,cuu,fx,fu,lims,x,u,kl_cost_terms)`` (backward_pass.jl:259).
    ``kl_cost_terms = ((cxkl,cukl,cxxkl,cxukl,cuukl), ηbracket)``; ``ηbracket`` is a 3-vector, a [3,N] matrix (per-step η),
    or with a batch [3,B] / [3,N,B].  Returns ``(diverge, GaussianPolicy(N,n,m,K,k,Quui,Quu), Vx, Vxx, dV)``."""
    h = handle or default_handle()
    cxa = _lib.f64(cx)
    batched = cxa.ndim == 3
    cx, cu, u = _b(cx, 2), _b(cu, 2), _b(u, 2)
    n, N, B = cx.shape
    m = cu.shape[0]
    _kl_box("back_pass_gps", n, m, wide)
    fx, fu, cxx, cxu, cuu = map(_lib.f64, (fx, fu, cxx, cxu, cuu))
    assert fx.ndim in (3, 4) and cxx.ndim in (3, 4), "back_pass_gps needs 3-D fx/fu and cxx/cxu/cuu (backward_pass.jl:259)"
    assert cx.shape[:2] == (n, N) and cu.shape[:2] == (m, N) and cxx.shape[:3] == (n, n, N) and cxu.shape[:3] == (n, m, N)
    assert cuu.shape[:3] == (m, m, N)                                                     # the reference's @asserts :266-270
    kl, etab = kl_cost_terms
    kl = [_b(a, nd) for a, nd in zip(kl, (2, 2, 3, 3, 3))]
    etab = np.asarray(etab, dtype=np.float64)
    # ηbracket: [3] one η; [3,N] per-step η of an unbatched call (ηbracket[2,i], :262,293); batch: [3,B] or [3,N,B]
    if etab.ndim == 1:
        eta_tv, eta = False, np.full(B, etab[1])
    elif etab.ndim == 2 and batched:
        eta_tv, eta = False, np.ascontiguousarray(etab[1])
    elif etab.ndim == 2:
        eta_tv, eta = True, np.asfortranarray(etab[1].reshape(N, 1))
    else:
        eta_tv, eta = True, np.asfortranarray(etab[1])
    assert eta.size == (N * B if eta_tv else B), "ηbracket does not match the batch / horizon"
    L = _lims(lims)
    d = _lib.BPDesc(n, m, N, B, 1, int(fx.ndim == 4), 1, int(cxx.ndim == 4), 1, int(L is not None))
    t = _lib.KLCostTerms(*[_lib.ptr(a) for a in kl], _lib.ptr(eta), int(eta_tv))
    K = _lib.result_array((m, n, N, B)); k = _lib.result_array((m, N, B)); Quu = _lib.result_array((m, m, N, B))
    Quui = _lib.result_array((m, m, N, B)); Vx = _lib.result_array((n, N, B)); Vxx = _lib.result_array((n, n, N, B))
    dV = np.zeros((2, B), order="F"); div = np.zeros(B, dtype=np.int32)
    with _wide(h, wide):
        _lib.check(_lib.lib().ddp_back_pass_gps_f64(h.raw, _C.byref(d), *map(_lib.ptr, (cx, cu, cxx, cxu, cuu, fx, fu)), _C.byref(t),
                                                    _lib.ptr(L), _lib.ptr(u), *map(_lib.ptr, (K, k, Quu, Quui, Vx, Vxx, dV)),
                                                    div.ctypes.data_as(_lib.i32p)))
    if not batched:
        return int(div[0]), GaussianPolicy(N, n, m, K[..., 0], k[..., 0], Quui[..., 0], Quu[..., 0]), Vx[..., 0], Vxx[..., 0], dV[:, 0]
    return div, GaussianPolicy(N, n, m, K, k, Quui, Quu), Vx, Vxx, dV


def forward_covariance(model, x, u, traj, *, handle=None, wide=False):
    """``forward_covariance(model,x,u,traj)`` -> ``sigmanew[(n+m),(n+m),N(,B)]`` (forward_pass.jl:37-56); ``x``,``u`` are
    only what the reference hands to `df(model,·)`/`covariance(model,·)` — the model here already holds those arrays."""
    h = handle or default_handle()
    batched = np.ndim(traj.K) == 4
    K, Sg = _b(traj.K, 3), _b(traj.Σ, 3)
    m, n, N, B = K.shape
    _kl_box("forward_covariance", n, m, wide)
    fx, R1 = _lib.f64(model.fx), _lib.f64(model.R1)
    S = _lib.result_array((n + m, n + m, N, B))
    with _wide(h, wide):
        _lib.check(_lib.lib().ddp_forward_covariance_f64(h.raw, n, m, N, B, _lib.ptr(fx), int(fx.ndim == 4), _lib.ptr(R1), _lib.ptr(K),
                                                         _lib.ptr(Sg), _lib.ptr(S)))
    return S if batched else S[..., 0]


def model_covariance(model, x, u):
    """this build's `covariance(model,x,u)`: Julia `cov` of the residuals x[:,t+1] - fx_t x[:,t] - fu_t u[:,t] (host, n x n)"""
    x, u = np.asarray(x, float), np.asarray(u, float)
    E = np.stack([x[:, t + 1] - model.fx[:, :, t] @ x[:, t] - model.fu[:, :, t] @ u[:, t] for t in range(x.shape[1] - 1)], axis=1)
    return np.atleast_2d(np.cov(E))


def _kl_div(xnew, xold, Σ_new, traj_new, traj_prev, handle=None, wide=False):
    h = handle or default_handle()
    batched = np.ndim(traj_new.K) == 4
    Kn, kn, Sn = _b(traj_new.K, 3), _b(traj_new.k, 2), _b(traj_new.Σ, 3)
    Kp, kp, Sp, Sip = _b(traj_prev.K, 3), _b(traj_prev.k, 2), _b(traj_prev.Σ, 3), _b(traj_prev.Σi, 3)
    xnew, xold, S = _b(xnew, 2), _b(xold, 2), _b(Σ_new, 3)
    m, n, T, B = Kn.shape
    _kl_box("kl_div_wiki", n, m, wide)
    kld = np.zeros((T, B), order="F"); mean = np.zeros(B)
    with _wide(h, wide):
        _lib.check(_lib.lib().ddp_kl_div_f64(h.raw, n, m, T, B, *map(_lib.ptr, (xnew, xold, S, Kn, kn, Sn, Kp, kp, Sp, Sip, kld, mean))))
    return (kld, mean) if batched else (kld[:, 0], mean[0])


def kl_div_wiki(xnew, xold, Σ_new, traj_new, traj_prev, *, handle=None, wide=False):
    """``kl_div_wiki`` (klutils.jl:70-103): the clipped per-step divergences; ``Inf`` when a logdet throws (unbatched call)"""
    kld, mean = _kl_div(xnew, xold, Σ_new, traj_new, traj_prev, handle, wide)
    if np.ndim(mean) == 0 and np.isinf(mean) and np.all(np.isfinite(kld)):
        return np.inf
    return kld


def geom(ηbracket):
    ηbracket = np.asarray(ηbracket, float)
    return np.sqrt(ηbracket[0] * ηbracket[2])                                             # klutils.jl:154-155


def calc_η(xnew, xold, sigmanew, ηbracket, traj_new, traj_prev, kl_step, *, handle=None, _mean=None, wide=False):
    """scalar-``kl_step`` method (klutils.jl:112-133): returns ``(ηbracket, satisfied, divergence)``; mutates ``ηbracket``"""
    if not kl_step > 0:
        return ηbracket, True, 0
    divergence = _kl_div(xnew, xold, sigmanew, traj_new, traj_prev, handle, wide)[1] if _mean is None else _mean
    viol = divergence - kl_step
    satisfied = abs(viol) < 0.1 * kl_step
    if not satisfied:
        if viol < 0:                                                                      # η was too big
            ηbracket[2] = ηbracket[1]
            ηbracket[1] = max(geom(ηbracket), 0.1 * ηbracket[2])
        else:                                                                             # η was too small
            ηbracket[0] = ηbracket[1]
            ηbracket[1] = min(geom(ηbracket), 10.0 * ηbracket[0])
    return ηbracket, bool(satisfied), divergence


def iLQGkl(problem, x0, traj_prev, model, *, kl_step=1.0, lims=None, max_iter=50, cost=None, ηbracket=(1e-8, 1.0, 1e16),
           del0=1e-4, constrain_per_step=False, diff_fun=None, handle=None, params=None, wide=False, t0=None, fitted=False,
           cost_model=None):
    """``iLQGkl(dynamics,costfun,derivs,x0,traj_prev,model; kl_step, lims, max_iter, cost, ηbracket, del0)`` with a registered
    ``problem`` or a ``DeviceProblem`` (the user's closures as device source; ``params`` as in ``iLQG``) standing in for the three
    closures (single KL constraint, iLQGkl.jl:91-178).  ``x0[n,N(,B)]`` is the pre-rolled trajectory (the reference errors otherwise,
    :71-72) and ``cost`` its cost (:69).  With a ``DeviceProblem``, ``model = Model(None, None, R1)`` means the problem's own
    linearisation (the fx of STEP 1).
    Returns ``(x, u, traj_new, Vx, Vxx, cost, trace)``; ``trace`` is a dict of per-trajectory arrays
    (status 1 SUCCESS :169 / 2 η > ηmax :174 / 3 max_iter :234, iter, η bracket, divergence, n_backpass).
    The loop runs inside ONE library call (``ddp_ilqgkl_f64``); ``DDP_KL_HOSTLOOP=1`` selects the loop on host arrays instead.
    ``wide=True``: n <= 64, m <= 32 — an ``LQProblem``, or a ``DeviceProblem`` made with ``wave=True``.
    ``t0``: the clock of every trajectory of a ``DeviceProblem`` made with ``clock=True`` (an int or B ints, default 0): STEP 1 and
    every rollout evaluate the model at the absolute step ``t0 + i``.
    ``fitted=True`` (a ``DeviceProblem`` made with ``fitted=True``, or with ``wave=True, fitted_wave=True`` — the only kind that goes with
    ``wide=True``; ``model = Model(fx, fu, R1, fc)`` from ``fit_dynamics``): the whole loop plans on the fitted time-varying affine model
    ``x̂[i+1] = fx_i x̂_i + fu_i û_i + fc_i`` under the problem's cost — back_pass_gps takes ``model.fx, model.fu``, every rollout runs
    ``ddp_user_rollout_fit`` (``ddp_user_rollout_fit_wave`` on a ``fitted_wave`` problem) on the tables, forward_covariance takes
    ``model.fx``; the problem's ``dynamics`` and the fx, fu of its ``derivatives`` are not used.  ``x0`` should be the rollout of
    ``traj_prev.k`` on the tables (``forward_pass(None, x0, u, None, 1.0, problem, lims, model=(fx, fu, fc))``).  The tables must be
    finite at every step (a step ``fit_dynamics`` rejected is NaN).  ``fitted=False`` (default): the plan is made on the problem's own
    model, ``model.fx`` only shapes the state covariance.
    ``cost_model=(cx, cu, cxx, cxu, cuu)`` (a ``DeviceProblem``; ``[n,N(,B)]``, ``[m,N(,B)]``, ``[n,n,N(,B)]``, ``[n,m,N(,B)]``,
    ``[m,m,N(,B)]``, e.g. the first five arrays ``fit_cost`` returns): every backward pass of the loop takes these arrays in place of the
    cost derivatives STEP 1 evaluates at ``(x0, traj_prev.k)``; ``cost``, the problem's own cost of the rollouts (what the loop compares
    and returns) and the loop itself are as without it.  With and without ``fitted=True``; the arrays must be finite.  Together with
    ``wide=True`` on a ``DeviceProblem`` made with ``wave=True`` (``back_pass_gps_wide`` takes the five arrays).
    ``kl_step``: a scalar, or with a batched call ``B`` values, ONE STEP PER TRAJECTORY (e.g. ``kl_step_adjust(...)[0]``): trajectory
    ``b`` is held to ``kl_step[b]`` and runs as it does in a call with that scalar.  (The reference's per-time-step meaning of a
    vector ``kl_step`` belongs to ``constrain_per_step``, which stays refused.)  The values are the handle's for the duration of the call
    (``ddp_kl_set_steps``) and cleared on every way out; every loop variant reads them, ``DDP_KL_HOSTLOOP=1`` included."""
    if cost_model is not None:
        if wide and not (isinstance(problem, DeviceProblem) and problem.wave):
            raise DDPError("iLQGkl: cost_model= together with wide=True needs a DeviceProblem made with wave=True (DDP_USER_WAVE); on any "
                           "other problem it is refused (a cost model there is sized for n <= 32, m <= 8)")
        if not isinstance(problem, DeviceProblem):
            raise DDPError("iLQGkl: cost_model= needs a DeviceProblem (the registered problems bring their own quadratic cost)")
    if fitted:
        if wide and not (isinstance(problem, DeviceProblem) and problem.fitted_wave):
            raise DDPError("iLQGkl: fitted=True together with wide=True needs a DeviceProblem made with wave=True, fitted_wave=True "
                           "(DDP_USER_FITTED_WAVE); on any other problem it is refused (ddp_user_rollout_fit is sized for n <= 32, m <= 8)")
        if not isinstance(problem, DeviceProblem):
            raise DDPError("iLQGkl: fitted=True needs a DeviceProblem made with fitted=True (DDP_USER_FITTED)")
    if constrain_per_step:
        raise NotImplementedError("constrain_per_step (iLQGkl.jl:180-232) is not offloaded")
    if isinstance(problem, DeviceProblem) and problem.second_order_wave:
        raise DDPError("iLQGkl: a DeviceProblem made with second_order_wave=True is refused (back_pass_gps has no second-order variant); "
                       "make the problem without the flag for the KL loop")
    if isinstance(problem, DeviceProblem) and problem.second_order:
        raise DDPError("iLQGkl: a DeviceProblem made with second_order=True is refused (back_pass_gps has no second-order variant); "
                       "make the problem without the flag for the KL loop")
    if cost is None or np.size(cost) == 0:
        raise ValueError("Initial trajectory supplied, initial cost must also be supplied")                     # :69
    x0 = _lib.f64(x0)
    batched = x0.ndim == 3
    x = _b(x0, 2)
    n, N, B = x.shape
    u = _b(traj_prev.k, 2).copy(order="F")                                                                       # :45
    m = u.shape[0]
    if x.shape[1] != u.shape[1]:
        raise ValueError("pre-rolled initial trajectory must be of correct length (size(x0,2) == N)")            # :72
    _kl_box("iLQGkl", n, m, wide)
    steps = None
    if np.ndim(kl_step) != 0:                              # one step per trajectory
        steps = np.ascontiguousarray(kl_step, dtype=np.float64)
        if not batched or steps.shape != (B,):
            raise DDPError("iLQGkl: kl_step should be a scalar or, with a batched call, B = %d values (one step per trajectory), got shape %s"
                           % (B, np.shape(kl_step)))
        if not np.all(np.isfinite(steps)):
            raise DDPError("iLQGkl: kl_step[%d] = %r is not finite" % (int(np.flatnonzero(~np.isfinite(steps))[0]), float(steps[~np.isfinite(steps)][0])))
        kl_step = float(steps[0])                          # (the scalar of the call is not read while the table is set)
    prev0 = GaussianPolicy(N, n, m, _b(traj_prev.K, 3), np.zeros_like(u), _b(traj_prev.Σ, 3), _b(traj_prev.Σi, 3))   # k *= 0 (:51)
    user = isinstance(problem, DeviceProblem)
    prm = _user_kl_args(problem, model, prev0, x, u, cost, lims, params, diff_fun, batched) if user else None
    tables = _fitted_kl_tables(problem, model, n, m, N, B) if fitted else None
    ctabs = _cost_model_tables(cost_model, n, m, N, B) if cost_model is not None else None
    h = handle or default_handle()                         # (behind every check that needs no device)
    etab = np.asarray(ηbracket, dtype=np.float64)
    etab = etab.copy() if etab.shape == (3, B) else np.repeat(etab.reshape(3)[:, None], B, 1)                    # copy (:52); [3,B]: one bracket per trajectory
    del0 = np.full(B, float(del0))
    import os as _os
    if _os.environ.get("DDP_KL_HOSTLOOP") != "1":
        with _wide(h, wide), _clock(problem, h, t0), _steps(h, steps):
            return _ilqgkl_call(h, problem, model, prev0, lims, kl_step, max_iter, x, u, cost, etab, float(del0[0]), batched, diff_fun, prm,
                                tables, ctabs)
    with _wide(h, wide), _clock(problem, h, t0):           # (the clocks are checked here; the array calls below set their own)
        return _ilqgkl_hostloop(h, problem, model, prev0, lims, kl_step if steps is None else steps, max_iter, x, u, etab, del0, batched, diff_fun, prm, user, wide, t0,
                                tables, ctabs)


def _cost_model_tables(cost_model, n, m, N, B):
    """``cost_model=``: the five arrays as [.,.,N,B]; a malformed tuple, shape or a non-finite entry is refused by name before any launch"""
    try:
        cx, cu, cxx, cxu, cuu = cost_model
    except (TypeError, ValueError):
        raise DDPError("iLQGkl: cost_model should be five arrays (cx, cu, cxx, cxu, cuu), e.g. fit_cost(...)[:5]")
    if any(a is None for a in (cx, cu, cxx, cxu, cuu)):
        raise DDPError("iLQGkl: cost_model needs cx, cu, cxx, cxu and cuu (one of them is None)")
    tabs = tuple(_lib.f64(a) for a in (cx, cu, cxx, cxu, cuu))
    want = ((n, N), (m, N), (n, n, N), (n, m, N), (m, m, N))
    b4 = tabs[0].ndim == 3
    tb = (B,) if b4 else ()
    if any(a.shape != w + tb for a, w in zip(tabs, want)):
        raise DDPError("iLQGkl: cost_model cx, cu, cxx, cxu, cuu should be (n,N), (m,N), (n,n,N), (n,m,N), (m,m,N) = %s%s, got %s"
                       % (", ".join(str(w) for w in want), " + (B = %d,)" % B if b4 else "", ", ".join(str(a.shape) for a in tabs)))
    if not b4:                                             # one cost model for the batch (B = 1 of an unbatched call)
        if B != 1:
            raise DDPError("iLQGkl: cost_model takes one cost model per trajectory: cx should be (n,N,B) with B = %d, got %s" % (B, tabs[0].shape))
        tabs = tuple(_lib.f64(a[..., None]) for a in tabs)
    for name, a in zip(("cx", "cu", "cxx", "cxu", "cuu"), tabs):
        bad = ~np.isfinite(a)
        if bad.any():
            flat = bad.reshape(-1, N, B).any(axis=0)       # [N, B]
            b = int(np.flatnonzero(flat.any(axis=0))[0])
            i = int(np.flatnonzero(flat[:, b])[0])
            raise DDPError("iLQGkl: cost_model needs finite arrays: %s is not finite at step %d of trajectory %d" % (name, i, b))
    return tabs


def _fitted_kl_tables(problem, model, n, m, N, B):
    """``fitted=True``: the tables of ``model`` as [.,.,N,B] arrays; every missing condition is refused by name before any launch"""
    if not (problem.fitted or problem.fitted_wave):
        raise DDPError("iLQGkl: fitted=True needs a DeviceProblem made with fitted=True (DDP_USER_FITTED)%s"
                       % ("; a wave=True problem: with fitted_wave=True (DDP_USER_FITTED_WAVE)" if problem.wave else ""))
    if model.fx is None or model.fu is None:
        raise DDPError("iLQGkl: fitted=True needs model.fx, model.fu and model.fc (Model(fx, fu, R1, fc) from fit_dynamics)")
    if model.fc is None:
        raise DDPError("iLQGkl: fitted=True needs model.fc (Model(fx, fu, R1, fc)); fc=None is the model of fitted=False")
    b4 = np.ndim(model.fx) == 4
    tabs = _fitted_tables(problem, (model.fx, model.fu, model.fc), n, m, N, B, b4, "iLQGkl")
    if not b4:                                             # one set of tables for the batch (B = 1 of an unbatched call)
        if B != 1:
            raise DDPError("iLQGkl: fitted=True takes one set of tables per trajectory: fx, fu, fc should be (n,n,N,B), (n,m,N,B), (n,N,B) "
                           "with B = %d, got %s" % (B, np.shape(model.fx)))
        tabs = tuple(_lib.f64(a[..., None]) for a in tabs)
    for name, a in zip(("fx", "fu", "fc"), tabs):
        bad = ~np.isfinite(a)
        if bad.any():
            flat = bad.reshape(-1, N, B).any(axis=0)       # [N, B]
            b = int(np.flatnonzero(flat.any(axis=0))[0])
            i = int(np.flatnonzero(flat[:, b])[0])
            raise DDPError("iLQGkl: fitted=True needs finite tables: model.%s is not finite at step %d of trajectory %d (a step "
                           "fit_dynamics rejected is NaN: see its status)" % (name, i, b))
    return tabs


def _ilqgkl_hostloop(h, problem, model, prev0, lims, kl_step, max_iter, x, u, etab, del0, batched, diff_fun, prm, user, wide, t0=None,
                     tables=None, ctabs=None):
    """DDP_KL_HOSTLOOP=1 (the body of iLQGkl on host arrays)"""
    n, N, B = x.shape
    m = u.shape[0]
    # ---- DDP_KL_HOSTLOOP=1: the loop of the reference on host arrays, one library call per array operation (cross-check in the tests)
    # STEP 1 (:86): the KL demos hand 3-D arrays to back_pass_gps (demo_linear.jl:91-101)
    if user:
        fx, fu, _, _, _, cx, cu, cxx, cxu, cuu = df(problem, x, u, handle=h, params=prm[0], t0=t0)
        hb = problem.const_hessian                             # constant Hessians [.,.,B]: the time axis back_pass_gps wants
        cxx, cxu, cuu = _tv(cxx, N, hb), _tv(cxu, N, hb), _tv(cuu, N, hb)
        if ctabs is not None:                                  # cost_model=: the backward passes take the caller's cost arrays
            cx, cu, cxx, cxu, cuu = ctabs
        if tables is not None:                                 # fitted=True: the plan is made on the tables (the fx, fu of STEP 1 are dropped)
            fx, fu = tables[0], tables[1]
            if model.fx is None or np.ndim(model.fx) == 3:
                model = Model(fx, fu, model.R1)
        if model.fx is None:
            model = Model(fx, fu, model.R1)
    else:
        fx, fu, _, _, _, cx, cu, cxx, cxu, cuu = df(problem, x, u, handle=h)
        dynb = bool(getattr(problem, "dyn_batched", False))
        fx, fu = _tv(fx, N, dynb), _tv(fu, N, dynb)
        cxx, cxu, cuu = _tv(cxx, N), _tv(cxu, N), _tv(cuu, N)
    kl = grad_kl(prev0, handle=h, wide=wide)                                                                    # :90
    status = np.zeros(B, dtype=int); iters = np.zeros(B, dtype=int); nback = np.zeros(B, dtype=int)
    divergence = np.zeros(B); satisfied = np.zeros(B, dtype=bool)
    live = np.ones(B, dtype=bool)
    out = None
    for it in range(1, max_iter + 1):                                                                           # :91
        idx = np.flatnonzero(live)
        if idx.size == 0:
            break
        iters[idx] = it
        # back_pass until the KL-regularised Quu is positive definite everywhere (:95-122); each trajectory owns its η
        pend = idx.copy()
        guard = 0
        allB = idx.size == B                                   # nothing to gather or scatter while every trajectory is live
        acc = None                                             # results of this iteration, indexed like `idx`
        pos = np.full(B, -1); pos[idx] = np.arange(idx.size)
        while pend.size:
            whole = pend.size == B
            sub = (lambda a: a) if whole else (lambda a: a[..., pend])                                          # noqa: E731
            div, pol, Vx, Vxx, dV = back_pass_gps(sub(cx), sub(cu), cxx if cxx.ndim == 3 else sub(cxx), cxu if cxu.ndim == 3 else sub(cxu),
                                                  cuu if cuu.ndim == 3 else sub(cuu), fx if fx.ndim == 3 else sub(fx),
                                                  fu if fu.ndim == 3 else sub(fu), lims, sub(x), sub(u),
                                                  (tuple(sub(a) for a in kl), etab[:, pend]), handle=h, wide=wide)
            nback[pend] += 1
            good = div == 0
            got = (pol.K, pol.k, pol.Σ, pol.Σi, Vx, Vxx, dV)
            if acc is None and good.all() and pend.size == idx.size:
                acc = list(got)                                # the common case: one back pass, no copies
            else:
                if acc is None:
                    acc = [np.zeros(a_.shape[:-1] + (idx.size,), order="F") for a_ in got]
                tgt = pos[pend[good]]
                for dst, src in zip(acc, got):
                    dst[..., tgt] = src[..., good]
            bad = pend[~good]
            etab[1, bad] += del0[bad]                                                                            # :103-105
            del0[bad] *= 2
            pend = bad
            guard += 1
            if guard > 200:
                raise RuntimeError("back_pass_gps keeps diverging (the reference would loop forever)")
        new = GaussianPolicy(N, n, m, acc[0], acc[1], acc[2], acc[3])
        sel = (lambda a: a) if allB else (lambda a: a[..., idx])                                                # noqa: E731
        pb = _SubProblem(problem, idx, B, prm[0]) if user else (problem if allB else _SubProblem(problem, idx, B))
        xs = sel(x)
        ts = t0 if (t0 is None or np.size(t0) == 1) else np.asarray(t0)[idx]      # the clocks of the trajectories rolled out
        mt = None if tables is None else tuple(sel(a) for a in tables)
        xnew, unew, cnew = forward_pass(new, xs[:, 0, :], sel(u), xs, 1.0, pb, lims, diff_fun, handle=h, t0=ts, model=mt)           # :132
        del pb                                                 # (a DeviceProblem slice frees its compiled-problem pointer here)
        mdl = Model(model.fx if (np.ndim(model.fx) == 3 or allB) else model.fx[..., idx], model.fu, model.R1)
        sig = forward_covariance(mdl, xs, sel(u), new, handle=h, wide=wide)                                     # :133
        pv = prev0 if allB else GaussianPolicy(N, n, m, sel(prev0.K), sel(prev0.k), sel(prev0.Σ), sel(prev0.Σi))
        _, mean = _kl_div(xnew, xs, sig, new, pv, h, wide)
        if out is None:
            out = dict(x=np.zeros((n, N, B)), u=np.zeros((m, N, B)), K=np.zeros((m, n, N, B)), S=np.zeros((m, m, N, B)),
                       Si=np.zeros((m, m, N, B)), Vx=np.zeros((n, N, B)), Vxx=np.zeros((n, n, N, B)), cost=np.zeros((cnew.shape[0], B)),
                       dV=np.zeros((2, B)))
        if allB:
            out.update(x=xnew.reshape(n, N, B), u=unew.reshape(m, N, B), cost=cnew.reshape(-1, B), K=new.K, S=new.Σ, Si=new.Σi,
                       Vx=acc[4], Vxx=acc[5], dV=acc[6])
        else:
            out["x"][..., idx], out["u"][..., idx], out["cost"][..., idx] = xnew.reshape(n, N, -1), unew.reshape(m, N, -1), cnew.reshape(-1, idx.size)
            out["K"][..., idx], out["S"][..., idx], out["Si"][..., idx] = new.K, new.Σ, new.Σi
            out["Vx"][..., idx], out["Vxx"][..., idx], out["dV"][..., idx] = acc[4], acc[5], acc[6]
        for j, b in enumerate(idx):                                                                             # :141, :169-177
            eb, sat, dv = calc_η(None, None, None, etab[:, b], None, None, kl_step if np.ndim(kl_step) == 0 else kl_step[b], _mean=mean[j])
            etab[:, b] = eb
            divergence[b], satisfied[b] = dv, sat
            if sat:
                status[b], live[b] = 1, False
            elif etab[1, b] > 0.999 * etab[2, b]:
                status[b], live[b] = 2, False
    status[live] = 3                                                                                            # :234
    traj_new = GaussianPolicy(N, n, m, out["K"], out["u"].copy(), out["S"], out["Si"])                          # traj_new.k = copy(u) (:239)
    trace = dict(status=status, iter=iters, η=etab, divergence=divergence, satisfied=satisfied, n_backpass=nback, dV=out["dV"])
    if not batched:
        traj_new = GaussianPolicy(N, n, m, out["K"][..., 0], out["u"][..., 0].copy(), out["S"][..., 0], out["Si"][..., 0])
        trace = {k_: (v[..., 0] if isinstance(v, np.ndarray) else v) for k_, v in trace.items()}
        return out["x"][..., 0], out["u"][..., 0], traj_new, out["Vx"][..., 0], out["Vxx"][..., 0], out["cost"][..., 0], trace
    return out["x"], out["u"], traj_new, out["Vx"], out["Vxx"], out["cost"], trace



def _user_kl_args(problem, model, prev0, x, u, cost, lims, params, diff_fun, batched):
    """a DeviceProblem in iLQGkl: extents against the compiled n, m, the parameters, model.fx and cost, before any launch"""
    from . import _diff_mask
    n, N, B = x.shape
    m = u.shape[0]
    _user_shapes(problem, n, m)
    tb = (B,)
    if prev0.K.shape != (m, n, N) + tb or prev0.Σ.shape != (m, m, N) + tb or prev0.Σi.shape != (m, m, N) + tb:
        raise DDPError("traj_prev.K, Σ, Σi should be (m,n,N), (m,m,N), (m,m,N) [+ batch axis]")
    if model.fx is not None and np.shape(model.fx) not in ((n, n, N), (n, n, N, B)):
        raise DDPError("model.fx should be (n,n,N) or (n,n,N,B) (None: the problem's own linearisation), got %s" % (np.shape(model.fx),))
    if np.shape(model.R1) != (n, n):
        raise DDPError("model.R1 should be (n, n), got %s" % (np.shape(model.R1),))
    CL = problem.cost_len(N)
    cs = np.shape(cost)
    if cs not in (((CL, B), (B,)) if batched else ((CL,), (), (1,))):
        raise DDPError("cost should be %s, got %s" % ("(CL=%d, B) or (B,)" % CL if batched else "(CL=%d,)" % CL, cs))
    L = _lims(lims)
    if L is not None and L.shape != (m, 2):
        raise DDPError("lims should be (m, 2)")
    if diff_fun is not None and _diff_mask(diff_fun, n) != problem.diff_mask:
        raise DDPError("DeviceProblem: diff_fun is compiled into the problem (DeviceProblem(..., diff=...))")
    return problem._params(B, params)


def _ilqgkl_call(h, problem, model, prev0, lims, kl_step, max_iter, x, u, cost, etab, del0, batched, diff_fun=None, prm=None, tables=None, ctabs=None):
    """the whole loop of iLQGkl (iLQGkl.jl:91-178) as ONE library call: ``ddp_ilqgkl_f64`` / ``ddp_user_ilqgkl_f64`` (csrc/kl.hip)"""
    n, N, B = x.shape
    m = u.shape[0]
    user = prm is not None
    dp = None if user else _DevProblem(problem, N, B, diff_fun)
    CL = problem.cost_len(N) if user else dp.cost_len
    c0 = np.asarray(cost, dtype=np.float64)                                                      # only sum(cost) enters (:74,135)
    c0 = (c0.sum(axis=0) if c0.ndim == 2 else c0.reshape(-1)) if batched else np.array([c0.sum()])   # batch: [CL,B] per-step costs or [B] sums
    c0 = np.ascontiguousarray(np.broadcast_to(c0, (B,)))
    mfx, R1 = (None if model.fx is None else _lib.f64(model.fx)), _lib.f64(model.R1)
    Kp, Sp, Sip = _lib.f64(prev0.K), _lib.f64(prev0.Σ), _lib.f64(prev0.Σi)
    Lh = _lims(lims)
    o = _lib.ILQGKLOpts()
    _lib.lib().ddp_ilqgkl_default_opts(_C.byref(o))
    o.kl_step, o.max_iter, o.del0 = float(kl_step), int(max_iter), float(del0)
    eb = np.asfortranarray(etab)
    xo = _lib.result_array((n, N, B)); uo = _lib.result_array((m, N, B)); K = _lib.result_array((m, n, N, B))
    S = _lib.result_array((m, m, N, B)); Si = _lib.result_array((m, m, N, B)); Vx = _lib.result_array((n, N, B))
    Vxx = _lib.result_array((n, n, N, B)); co = _lib.result_array((CL, B)); dV = np.zeros((2, B), order="F")
    st = np.zeros((_lib.ILQGKL_NSTATS, B), order="F")
    mb = int(mfx is not None and mfx.ndim == 4)
    if ctabs is not None:                                  # cost_model=: ddp_user_ilqgkl_cost_f64, the tables (or three NULLs) and the five cost arrays
        _lib.check(_lib.lib().ddp_user_ilqgkl_cost_f64(h.raw, problem._ptr(h), N, B, _lib.ptr(prm[0]), prm[1], _C.byref(o), _lib.ptr(x), _lib.ptr(c0),
                                                       _lib.ptr(Kp), _lib.ptr(u), _lib.ptr(Sp), _lib.ptr(Sip), _lib.ptr(mfx), mb, _lib.ptr(R1),
                                                       _lib.ptr(Lh), _lib.ptr(eb), *map(_lib.ptr, tables if tables is not None else (None,) * 3),
                                                       *map(_lib.ptr, (xo, uo, K, S, Si, Vx, Vxx, co, dV, st)), None, *map(_lib.ptr, ctabs)))
    elif tables is not None:                               # fitted=True: ddp_user_ilqgkl_fit_f64, the same arguments and the three tables
        _lib.check(_lib.lib().ddp_user_ilqgkl_fit_f64(h.raw, problem._ptr(h), N, B, _lib.ptr(prm[0]), prm[1], _C.byref(o), _lib.ptr(x), _lib.ptr(c0),
                                                      _lib.ptr(Kp), _lib.ptr(u), _lib.ptr(Sp), _lib.ptr(Sip), _lib.ptr(mfx), mb, _lib.ptr(R1),
                                                      _lib.ptr(Lh), _lib.ptr(eb), *map(_lib.ptr, tables),
                                                      *map(_lib.ptr, (xo, uo, K, S, Si, Vx, Vxx, co, dV, st)), None))
    elif user:
        _lib.check(_lib.lib().ddp_user_ilqgkl_f64(h.raw, problem._ptr(h), N, B, _lib.ptr(prm[0]), prm[1], _C.byref(o), _lib.ptr(x), _lib.ptr(c0),
                                                  _lib.ptr(Kp), _lib.ptr(u), _lib.ptr(Sp), _lib.ptr(Sip), _lib.ptr(mfx), mb, _lib.ptr(R1),
                                                  _lib.ptr(Lh), _lib.ptr(eb), *map(_lib.ptr, (xo, uo, K, S, Si, Vx, Vxx, co, dV, st)), None))
    else:
        _lib.check(_lib.lib().ddp_ilqgkl_f64(h.raw, _C.byref(dp.struct), _C.byref(o), _lib.ptr(x), _lib.ptr(c0), _lib.ptr(Kp), _lib.ptr(u),
                                             _lib.ptr(Sp), _lib.ptr(Sip), _lib.ptr(mfx), mb, _lib.ptr(R1), _lib.ptr(Lh), _lib.ptr(eb),
                                             *map(_lib.ptr, (xo, uo, K, S, Si, Vx, Vxx, co, dV, st)), None))
    trace = dict(status=st[0].astype(int), iter=st[1].astype(int), η=eb, divergence=st[7].copy(), satisfied=st[3] != 0,
                 n_backpass=st[2].astype(int), dV=dV, cost=st[8].copy(), improvement=st[9].copy(), expected_reduction=st[10].copy(),
                 grad_norm=st[11].copy())
    if not batched:
        traj_new = GaussianPolicy(N, n, m, K[..., 0], uo[..., 0].copy(), S[..., 0], Si[..., 0])                  # traj_new.k = copy(u) (:239)
        trace = {k_: (v[..., 0] if isinstance(v, np.ndarray) else v) for k_, v in trace.items()}
        return xo[..., 0], uo[..., 0], traj_new, Vx[..., 0], Vxx[..., 0], co[..., 0], trace
    return xo, uo, GaussianPolicy(N, n, m, K, uo.copy(), S, Si), Vx, Vxx, co, trace


def kl_step_adjust(ec_prev, ec_pred, ec_act, kl_step, *, step_min=1e-2, step_max=1e2, handle=None):
    """The step rule of a guided-policy-search round, per trajectory, from three results of ``expected_cost``: ``ec_prev[N(,B)]`` the old
    policy on the old models, ``ec_pred`` the new policy on the old models, ``ec_act`` the new policy on the new models.  With
    ``J = Σ_i ec[i, b]`` summed in ascending ``i``: ``pred = J_prev − J_pred``, ``act = J_prev − J_act``,
    ``mult = clip(pred / (2 max(1e-4, pred − act)), 0.1, 5)`` (0.1 when a ``J`` is not finite) and
    ``kl_step_new = clip(kl_step · mult, step_min, step_max)``; ``kl_step`` is a scalar or ``B`` values.  Returns
    ``(kl_step_new[B], mult[B])`` (``ddp_kl_step_adjust_f64``, one thread per trajectory); ``iLQGkl(..., kl_step=kl_step_new)`` takes
    the first as it is."""
    ecs = [_lib.f64(a) for a in (ec_prev, ec_pred, ec_act)]
    if ecs[0].ndim not in (1, 2) or any(a.shape != ecs[0].shape for a in ecs):
        raise DDPError("kl_step_adjust: ec_prev, ec_pred, ec_act should be three (N,) or (N, B) arrays, got %s" % ", ".join(str(a.shape) for a in ecs))
    if ecs[0].ndim == 1:
        ecs = [_lib.f64(a[:, None]) for a in ecs]
    N, B = ecs[0].shape
    if N < 1 or B < 1:
        raise DDPError("kl_step_adjust: N = %d, B = %d (both >= 1)" % (N, B))
    ks = np.asarray(kl_step, dtype=np.float64)
    if ks.ndim != 0 and ks.shape != (B,):
        raise DDPError("kl_step_adjust: kl_step should be a scalar or B = %d values, got shape %s" % (B, ks.shape))
    ks = np.ascontiguousarray(np.broadcast_to(ks, (B,)))
    if not (0 < step_min <= step_max < np.inf):
        raise DDPError("kl_step_adjust: step_min = %r, step_max = %r should be finite with 0 < step_min <= step_max" % (step_min, step_max))
    h = handle or default_handle()                         # (behind the checks that need no device)
    new, mult = np.zeros(B), np.zeros(B)
    _lib.check(_lib.lib().ddp_kl_step_adjust_f64(h.raw, N, B, *map(_lib.ptr, ecs), _lib.ptr(ks), float(step_min), float(step_max),
                                                 _lib.ptr(new), _lib.ptr(mult)))
    return new, mult


def _tv(a, N, batched=False):
    """give a [r,c] (or, batched, [r,c,B]) array the time axis back_pass_gps wants: [r,c,N] / [r,c,N,B]"""
    a = np.asarray(a, dtype=np.float64)
    if a.ndim == 4 or (a.ndim == 3 and not batched):
        return a
    if batched:
        return np.repeat(a[:, :, None, :], N, 2)
    return np.repeat(a[:, :, None], N, 2)


class _SubProblem:
    """a registered problem restricted to a subset of the batch (per-trajectory dynamics are sliced); a DeviceProblem with its
    per-trajectory params[:, idx] (and a compiled-problem pointer of its own: the cached module is shared)"""

    def __new__(cls, problem, idx, B, params=None):
        import copy
        p = copy.copy(problem)
        if isinstance(problem, DeviceProblem):
            p._made = {}
            P = problem.params if params is None else params
            if P is not None and np.ndim(P) == 2 and np.shape(P)[1] == B:
                P = _lib.f64(np.asarray(P)[:, idx])
            p.params = P
            return p
        for name in ("A", "B"):
            a = getattr(p, name, None)
            if isinstance(a, np.ndarray) and getattr(p, "dyn_batched", False) and a.shape[-1] == B:
                setattr(p, name, a[..., idx])
        return p


def demo_linear_kl(*, kl_step=1.0, rng=None, T=1000, n=10, m=2, h=0.01, outer=5, R1=None, handle=None, wide=False, **kwargs):
    """``demo_linear_kl(;kwargs...)`` (src/demo_linear.jl:63-136): the random LTI problem of ``demo_linear``, a rollout of the random
    initial controls, the exact model ``SimpleLTVModel(repeat(A), repeat(B))`` and five outer calls of ``iLQGkl`` starting from the
    identity policy ``GaussianPolicy(Float64,T,n,m)`` (k = 0, quirk Q20).  ``R1`` is what ``covariance(model,x,u)`` of the un-vendored
    LinearTimeVaryingModelsBase would return for that model — unknown here, default 1e-3·I (it only enters Σ of the state)."""
    import scipy.linalg as _sla
    from . import LQProblem, forward_pass
    _kl_box("demo_linear_kl", n, m, wide)
    rng = rng if rng is not None else np.random.default_rng()
    A0 = rng.standard_normal((n, n))
    A = _sla.expm(h * (A0 - A0.T))
    Bm = h * rng.standard_normal((n, m))
    Q, R = h * np.eye(n), 0.1 * h * np.eye(m)
    prob = LQProblem(A, Bm, Q, R)
    u = 0.1 * rng.standard_normal((m, T))
    x, _, _ = forward_pass(None, np.ones(n), u, None, 1.0, prob, None, handle=handle)            # rollout(u) (:107-114)
    x = x.reshape(n, T)
    model = Model(np.repeat(A[:, :, None], T, 2), np.repeat(Bm[:, :, None], T, 2), 1e-3 * np.eye(n) if R1 is None else _lib.f64(R1))
    eye = np.repeat(np.eye(m)[:, :, None], T, 2)
    traj = GaussianPolicy(T, n, m, np.zeros((m, n, T)), np.zeros((m, T)), eye, eye.copy())        # identity ctor: k = 0
    out = None
    outercosts = np.zeros(outer)
    for it in range(outer):
        cost0 = 0.5 * np.sum(x * (Q @ x)) + 0.5 * np.sum(u * (R @ u))                              # :122
        out = iLQGkl(prob, x, traj, model, kl_step=kl_step, cost=cost0, handle=handle, wide=wide, **kwargs)
        x, u, traj = out[0], out[1], out[2]
        outercosts[it] = float(np.sum(out[5]))
    out[6]["outercosts"] = outercosts
    return out
