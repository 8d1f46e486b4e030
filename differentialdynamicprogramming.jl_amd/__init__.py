"""MI355X-native iLQG hot path behind the call signatures of DifferentialDynamicProgramming.jl.

Host-side mirror of the reference's interface for this path (same names, argument order and error
behaviour), written in Python because no Julia toolchain exists in the build image; the Julia
`@ccall` wrapper a maintainer would use lives in ``julia/DDPAmd.jl``.

    back_pass(cx,cu,cxx,cxu,cuu,fx,fu,λ,regType,lims,x,u)   src/backward_pass.jl:162-252
    boxQP(H,g,lower,upper,x0)                               src/boxQP.jl:29-188
    forward_pass(traj_new,x0,u,x,α,problem,lims)            src/forward_pass.jl:9-33
    iLQG(problem,x0,u0; lims, ...)                          src/iLQG.jl:143-341
    GaussianPolicy                                          src/iLQG.jl:39-53

All compute runs in libddp_amd.so (HIP, gfx950) through the C ABI of include/ddp_amd.h.  There is no
CPU fallback: without the library or without a GPU every call raises ``DDPError``.

Arrays follow the reference's shapes; an extra trailing axis is the batch of independent
trajectories (``K[m,n,N,B]``), which the reference does not have.
"""
from __future__ import annotations

import contextlib as _contextlib
import ctypes as _C
import os as _os
import time as _time
from dataclasses import dataclass, field

import numpy as np

from . import _lib
from ._lib import DDPError, Handle, default_handle  # noqa: F401

__all__ = ["GaussianPolicy", "LQProblem", "PendcartProblem", "back_pass", "boxQP", "forward_pass", "iLQG", "print_timing", "mpc_shift", "demo_linear", "demo_pendcart", "demoQP",
           "df", "costfun", "Handle", "DDPError", "DEFAULT_ALPHA", "WrappedDiff", "DeviceProblem", "example_source", "vhess", "back_pass_ddp",
           "constraints", "iLQG_al", "normal", "sample_policy", "fit_dynamics", "GMM", "fit_gmm", "gmm_prior", "fit_cost", "expected_cost"]

DEFAULT_ALPHA = 10.0 ** np.linspace(0, -3, 11)     # iLQG.jl:145


@dataclass
class GaussianPolicy:
    """src/iLQG.jl:39-53.  ``K[m,n,T]`` (quirk Q19b: the docstring of the reference says n×m),
    ``k[m,T]``, ``Σ`` = Quui (never written by back_pass in the reference — zeros here),
    ``Σi`` = the unregularised Quu."""
    T: int = 0
    n: int = 0
    m: int = 0
    K: np.ndarray = field(default_factory=lambda: np.zeros((0, 0, 0)))
    k: np.ndarray = field(default_factory=lambda: np.zeros((0, 0)))
    Σ: np.ndarray = field(default_factory=lambda: np.zeros((0, 0, 0)))
    Σi: np.ndarray = field(default_factory=lambda: np.zeros((0, 0, 0)))

    def isempty(self):
        return self.T == self.n == self.m == 0

    def __len__(self):
        return self.T


# ------------------------------------------------------------------ registered problem families
@dataclass
class LQProblem:
    """x⁺ = A x + B u, cost = ½Σ x∘(Qx) + ½Σ u∘(Ru) — the closures of src/demo_linear.jl:30-50.
    A/B may be [n,n]/[n,m] (LTI), [..,N] (LTV) and, with ``dyn_batched``, carry a trailing batch axis."""
    A: np.ndarray
    B: np.ndarray
    Q: np.ndarray
    R: np.ndarray
    dyn_batched: bool = False
    kind = 0

    @property
    def n(self):
        return self.A.shape[0]

    @property
    def m(self):
        return self.B.shape[1]

    @property
    def dyn_tv(self):
        return (self.A.ndim - (1 if self.dyn_batched else 0)) == 3


@dataclass
class PendcartProblem:
    """src/system_pendcart.jl:42-59,83-106 (explicit Euler step, quadratic cost of length N+1)."""
    g: float = 9.82
    l: float = 0.35
    h: float = 0.01
    d: float = 0.99
    Q: np.ndarray = field(default_factory=lambda: np.diag([10.0, 1.0, 2.0, 1.0]))
    R: np.ndarray = field(default_factory=lambda: np.array([[1.0]]))
    goal: np.ndarray = field(default_factory=lambda: np.array([np.pi, 0.0, 0.0, 0.0]))
    kind = 1
    n = 4
    m = 1
    dyn_tv = False
    dyn_batched = False


class WrappedDiff:
    """What stands in for a user ``diff_fun`` (forward_pass.jl:5,19; iLQG.jl:156): subtraction with the listed state coordinates
    (0-based) wrapped to [-π, π], i.e. ``rem2pi(a[j] - b[j], RoundNearest)`` — ddp_problem::diff_wrap.  ``None`` / ``np.subtract``
    mean the reference's default ``-``.  A Python closure cannot run on the device."""

    def __init__(self, *coords):
        self.coords = tuple(int(c) for c in coords)
        if any(c < 0 or c >= 32 for c in self.coords):
            raise ValueError("WrappedDiff: coordinates must be in 0..31")

    @property
    def mask(self):
        m = 0
        for c in self.coords:
            m |= 1 << c
        return m

    def __call__(self, a, b):                                   # the same function on host arrays
        d = np.asarray(a, dtype=np.float64) - np.asarray(b, dtype=np.float64)
        for c in self.coords:
            d[c] = np.remainder(d[c] + np.pi, 2 * np.pi) - np.pi
        return d


def _diff_mask(diff, n):
    if diff is None or diff is np.subtract:
        return 0
    if isinstance(diff, WrappedDiff):
        if any(c >= n for c in diff.coords):
            raise ValueError("WrappedDiff names coordinate %d of a state of length %d" % (max(diff.coords), n))
        return diff.mask
    raise TypeError("diff_fun must be None / np.subtract (the reference's `-`) or a WrappedDiff: a Python closure cannot run on the device")


class _DevProblem:
    """ddp_problem struct + the arrays it points at (host arrays for the host-pointer flavours)."""

    def __init__(self, prob, N, B, diff=None):
        P = _lib.Problem()
        P.diff_wrap = _diff_mask(diff, prob.n)
        P.kind, P.n, P.m, P.N, P.B = prob.kind, prob.n, prob.m, N, B
        self.Q, self.R = _lib.f64(prob.Q), _lib.f64(np.atleast_2d(prob.R))
        P.Q, P.R = _lib.ptr(self.Q), _lib.ptr(self.R)
        if prob.kind == 0:
            self.A, self.B = _lib.f64(prob.A), _lib.f64(prob.B)
            P.A, P.Bm = _lib.ptr(self.A), _lib.ptr(self.B)
            P.dyn_tv, P.dyn_batched = int(prob.dyn_tv), int(prob.dyn_batched)
        else:
            P.g, P.l, P.h, P.d = prob.g, prob.l, prob.h, prob.d
            for i in range(4):
                P.goal[i] = float(prob.goal[i])
        # Q and R diagonal (the reference's demos): the rollout kernels then evaluate the cost themselves (ddp_problem::cost_diag)
        P.cost_diag = int(not np.any(self.Q - np.diag(np.diag(self.Q))) and not np.any(self.R - np.diag(np.diag(self.R))))
        self.struct = P
        self.cost_len = N + 1 if prob.kind == 1 else N


# ------------------------------------------------------------------ user problems (HIP device source, compiled at run time)
_EXAMPLES = _os.path.join(_lib._HERE, "user_examples")


def example_source(name):
    """Source text of a bundled example problem: ``"lq"``, ``"pendcart"`` or ``"car"`` (``user_examples/<name>.hip``), or the same
    model written for ``autodiff=True``: ``"lq_ad"``, ``"pendcart_ad"``, ``"car_ad"``; ``"car_plant"``: the car with a plant for the
    closed loop (``plant=True``); ``"bicycle_ad"``: a kinematic bicycle whose dynamics have mixed and control curvature, for
    ``second_order=True``; ``"chain_plant_ad"``: ``chain_ad`` with a plant (per-joint actuator gain and another damping, 9 parameters),
    for ``plant=True`` at the sizes of ``wave=True``; ``"chain_ad"``: a chain of ``m`` coupled pendulums (``n = 2 m``, 7 parameters at every size), the large model
    for ``wave=True``; ``"chain_ddp_ad"``: the same chain with the torque entering as ``g tanh(u_j) cos(q_j)`` (curvature in x, u
    and mixed; ``n = 2 m``, 8 parameters), for ``second_order_wave=True``; ``"car_track"``, ``"car_track_ad"``, ``"car_track_plant"``: the
    car following a sampled reference past a moving obstacle (``7 + 4 L`` parameters, the plant ``7 + 6 L``), for ``clock=True``;
    ``"car_table"``: the car's cost on a tabulated time-varying affine model in the parameter block (``9 + 28 N`` parameters), the
    emulation of ``fitted=True`` on the kernels from before the flag."""
    with open(_os.path.join(_EXAMPLES, name + ".hip")) as f:
        return f.read()


class DeviceProblem:
    """The user's own ``f``, ``costfun`` and ``df`` (iLQG.jl:143) as HIP device source: ``dynamics``, ``stage_cost``,
    ``derivatives`` and, with ``terminal=True``, ``terminal_cost`` (``const_hessian=True``: ``cost_hessians``) — the contract is in
    include/ddp_amd.h.  ``autodiff=True`` (DDP_USER_AUTODIFF): ``dynamics``, ``stage_cost`` and ``terminal_cost`` are templates over
    the scalar type of x and u, ``derivatives`` is not needed, and the library derives df by forward-mode AD on the device.  The library compiles the source for gfx950 with hiprtc, once per handle, and runs ``forward_pass``, ``df``,
    ``costfun`` and the whole ``iLQG`` on the device.  ``params``: ``[nparam]`` shared by the batch or ``[nparam, B]`` per trajectory
    (may be replaced per call through the ``params=`` keyword of the entry points).  ``diff``: ``None`` (``-``) or a ``WrappedDiff``.
    ``plant=True`` (DDP_USER_PLANT): the source also defines ``plant``, the true system that ``iLQG_mpc`` advances its trajectories
    with instead of the model.  ``second_order=True`` (DDP_USER_SECOND_ORDER, needs ``autodiff=True``): full DDP — ``iLQG``,
    ``iLQG_queue`` and ``iLQG_mpc`` run the backward pass with the curvature of the dynamics (backward_pass.jl:81-160), derived on the
    device from the same templates; ``vhess`` and ``back_pass_ddp`` are its array-level pieces.  ``iLQGkl`` refuses such a problem.
    ``wave=True`` (DDP_USER_WAVE): large problems, ``n <= 64`` and ``m <= 32`` (without it ``n <= 32``, ``m <= 8``): the rollout runs on a
    group of lanes per rollout (``ddp_user_rollout_wave``) and, with ``autodiff=True``, df on one wave per time step and trajectory
    (``ddp_user_df_wave``).  Legal at every shape; not with ``second_order=True``; ``iLQGkl`` takes such a problem up to ``n = 32``,
    ``m = 8``.  ``second_order_wave=True`` (DDP_USER_SECOND_ORDER_WAVE, implies ``wave=True``, needs ``autodiff=True``): full DDP at the
    shapes of ``wave=True`` — the backward pass is ``ddp_user_back_pass2_wave``, the step of the wide-control kernel (four waves per
    trajectory) with the curvature phase in front of it; accepted wherever a ``second_order=True`` problem is (``vhess``,
    ``back_pass_ddp``, ``iLQG``, ``iLQG_queue``, ``iLQG_mpc``), refused by ``iLQGkl``; not together with ``second_order=True``.
    ``clock=True`` (DDP_USER_CLOCK): a time-varying model.  ``dynamics``, ``stage_cost`` and ``derivatives`` take the absolute step
    ``t = c + i`` as one more ``int`` behind ``i`` and ``terminal_cost`` takes ``t = c + N - 1`` behind ``x``; the clock ``c`` of every
    trajectory comes from the ``t0=`` keyword of ``forward_pass``, ``df``, ``costfun``, ``iLQG``, ``iLQG_queue`` (one per problem),
    ``iLQG_mpc`` (the solve at closed-loop step ``s`` runs with ``c = t0 + s``, ``plant`` gets ``t = t0 + s``) and ``kl.iLQGkl``: an int or
    one int per trajectory, default 0.  Not together with ``second_order=True`` or ``second_order_wave=True``.
    ``constraints=nc`` (DDP_USER_CONSTRAINTS, needs ``autodiff=True``): the source also defines the template
    ``constraints(x, u, i, p, g)`` writing ``g[nc]``, feasible where ``g <= 0``.  ``constraints(problem, x, u)`` evaluates it, ``iLQG_al``
    solves the constrained problem by an augmented Lagrangian on the device, and ``forward_pass``, ``df``, ``costfun`` and ``iLQG`` take
    ``multipliers=(λ[nc,N(,B)], μ)`` and then work on the augmented cost (default: the raw cost).  Not together with ``const_hessian``,
    ``clock``, ``second_order`` or ``second_order_wave``; ``iLQG_queue``, ``iLQG_mpc`` and ``kl.iLQGkl`` refuse such a problem.
    ``sample=True`` (DDP_USER_SAMPLE): the program also holds ``ddp_user_sample``, and ``sample_policy`` runs ``S`` closed-loop rollouts
    per trajectory of the linear-Gaussian policy a solve returns (``û = u + L ξ + K diff(x̂, x)``, ``L`` the lower Cholesky factor of
    ``Σ``, ``ξ`` generated on the device) on the model or, with ``plant=True``, on the plant; every other entry point ignores the flag.
    Not together with ``wave``, ``second_order_wave``, ``clock`` or ``constraints`` (deferred).
    ``fitted=True`` (DDP_USER_FITTED): the program also holds ``ddp_user_rollout_fit``, the rollout on a fitted time-varying affine model
    ``x̂[i+1] = fx_i x̂_i + fu_i û_i + fc_i`` (the tables ``fit_dynamics`` returns) under the problem's own cost:
    ``forward_pass(..., model=(fx, fu, fc))`` runs it and ``kl.iLQGkl(..., fitted=True)`` plans on that model throughout; every other
    entry point ignores the flag.  Not together with ``wave``, ``second_order_wave``, ``clock`` or ``constraints`` (deferred).
    ``cost_fit=True`` (DDP_USER_COST_FIT): the program also holds ``ddp_user_cost_fit``, and ``fit_cost`` fits the quadratic cost model of
    a guided-policy-search round to the samples ``sample_policy`` returns — the cost expanded at every sample, moved to the nominal and
    averaged; ``kl.iLQGkl(..., cost_model=...)`` plans on it.  Every other entry point ignores the flag.  Not together with ``wave``,
    ``second_order_wave``, ``clock`` or ``constraints`` (deferred).
    ``sample_wave=True`` (DDP_USER_SAMPLE_WAVE, needs ``wave=True``): the sampler at the shapes of ``wave=True``, ``n <= 64`` and
    ``m <= 32`` — the program also holds ``ddp_user_sample_wave`` (a group of lanes per sample, the vectors in LDS) and ``sample_policy``
    takes the problem, with the semantics of ``sample=True`` word for word; every other entry point ignores the flag.  Legal with
    ``terminal``, ``const_hessian``, ``autodiff``, ``plant``, ``second_order_wave`` and ``diff``; not with ``clock`` or ``constraints``
    (deferred).  ``sample=True`` stays the flag of a problem without ``wave``.
    ``fitted_wave=True`` (DDP_USER_FITTED_WAVE, needs ``wave=True``): the fitted rollout at the shapes of ``wave=True``, ``n <= 64`` and
    ``m <= 32`` — the program also holds ``ddp_user_rollout_fit_wave`` (a group of lanes per rollout, the vectors in LDS, the rows of the
    tables streamed by the group); ``forward_pass(..., model=(fx, fu, fc))`` runs it and ``kl.iLQGkl(..., fitted=True, wide=True)`` plans
    on the tables ``fit_dynamics(..., wide=True)`` returns, with the semantics of ``fitted=True`` word for word; every other entry point
    ignores the flag.  Legal with ``terminal``, ``const_hessian``, ``autodiff``, ``plant``, ``sample_wave``, ``second_order_wave`` and
    ``diff``; not with ``clock`` or ``constraints`` (deferred).  ``fitted=True`` stays the flag of a problem without ``wave``."""
    kind = 2

    def __init__(self, source, n, m, *, nparam=0, params=None, terminal=False, const_hessian=False, autodiff=False, diff=None, plant=False,
                 second_order=False, wave=False, second_order_wave=False, clock=False, constraints=0, sample=False, fitted=False, cost_fit=False,
                 sample_wave=False, fitted_wave=False):
        self.clock = bool(clock)
        self.fitted_wave = bool(fitted_wave)
        self.sample_wave = bool(sample_wave)
        self.cost_fit = bool(cost_fit)
        self.sample = bool(sample)
        self.fitted = bool(fitted)
        self.nc = int(constraints)
        if self.nc < 0:
            raise DDPError("DeviceProblem: constraints = %d (the number of constraints, 0 for none)" % self.nc)
        self.second_order_wave = bool(second_order_wave)
        self.second_order, self.wave = bool(second_order), bool(wave) or self.second_order_wave
        if self.sample_wave and not self.wave:
            raise DDPError("DeviceProblem: DDP_USER_SAMPLE_WAVE needs DDP_USER_WAVE (sample_wave=True needs wave=True; without wave the "
                           "sampler is sample=True)")
        if self.fitted_wave and not self.wave:
            raise DDPError("DeviceProblem: DDP_USER_FITTED_WAVE needs DDP_USER_WAVE (fitted_wave=True needs wave=True; without wave the "
                           "fitted rollout is fitted=True)")
        self.source, self.n, self.m, self.nparam = str(source), int(n), int(m), int(nparam)
        self.terminal, self.const_hessian, self.autodiff, self.plant = bool(terminal), bool(const_hessian), bool(autodiff), bool(plant)
        self.flags = ((1 if self.terminal else 0) | (2 if self.const_hessian else 0) | (4 if self.autodiff else 0) |
                      (8 if self.plant else 0) | (16 if self.second_order else 0) | (_lib.USER_WAVE if self.wave else 0) |
                      (_lib.USER_SECOND_ORDER_WAVE if self.second_order_wave else 0) | (_lib.USER_CLOCK if self.clock else 0) |
                      (_lib.USER_CONSTRAINTS if self.nc else 0) | (_lib.USER_SAMPLE if self.sample else 0) |
                      (_lib.USER_FITTED if self.fitted else 0) | (_lib.USER_COST_FIT if self.cost_fit else 0) |
                      (_lib.USER_SAMPLE_WAVE if self.sample_wave else 0) | (_lib.USER_FITTED_WAVE if self.fitted_wave else 0))
        self.diff_mask = _diff_mask(diff, self.n)                # WrappedDiff holds coordinates below 32 at every n
        self.params = params
        self._made = {}                                          # id(handle) -> (handle, problem pointer)

    def check(self, extra_options=None):
        """Compile for gfx950 without a device (ddp_user_check), with the problem's flags (``autodiff`` included); returns the
        compiler log, raises DDPError with it on failure."""
        L = _lib.lib()
        if self.nc:
            rc = L.ddp_user_check_c(self.source.encode(), self.n, self.m, self.nparam, self.nc, self.flags,
                                    extra_options.encode() if extra_options else None)
        else:
            rc = L.ddp_user_check(self.source.encode(), self.n, self.m, self.nparam, self.flags,
                                  extra_options.encode() if extra_options else None)
        log = L.ddp_user_compile_log().decode()
        if rc != 0:
            raise DDPError("libddp_amd: %s (rc=%d)\n%s" % (L.ddp_last_error().decode(), rc, log))
        return log

    def cost_len(self, N):
        return N + 1 if self.terminal else N

    def _ptr(self, h):
        """the compiled problem on handle `h` (compiled / loaded at first use)"""
        e = self._made.get(id(h))
        if e is None or e[0] is not h:
            up = _C.c_void_p()
            if self.nc:
                _lib.check(_lib.lib().ddp_user_create_c(h.raw, self.source.encode(), self.n, self.m, self.nparam, self.nc, self.flags,
                                                        int(self.diff_mask), _C.byref(up)))
            else:
                _lib.check(_lib.lib().ddp_user_create(h.raw, self.source.encode(), self.n, self.m, self.nparam, self.flags,
                                                      int(self.diff_mask), _C.byref(up)))
            e = self._made[id(h)] = (h, up)
        return e[1]

    def _params(self, B, params=None):
        P = self.params if params is None else params
        if self.nparam == 0:
            return None, 0
        if P is None:
            raise DDPError("DeviceProblem: nparam = %d but no params were given" % self.nparam)
        P = _lib.f64(P)
        if P.shape == (self.nparam,):
            return P, 0
        if P.shape == (self.nparam, B):
            return P, 1
        raise DDPError("DeviceProblem: params should be (%d,) or (%d, B=%d), got %s" % (self.nparam, self.nparam, B, P.shape))

    @_contextlib.contextmanager
    def _clock(self, h, t0):
        """the clocks ``t0`` (``clock=True``; an int or one int per trajectory) for the calls inside the block (ddp_user_set_t0); every
        clock is 0 again afterwards, also when the call raises"""
        if t0 is None:
            yield
            return
        if not self.clock:
            raise DDPError("t0= needs a DeviceProblem made with clock=True (DDP_USER_CLOCK)")
        t = np.atleast_1d(np.asarray(t0))
        if t.ndim != 1 or not np.issubdtype(t.dtype, np.integer):
            raise DDPError("t0 should be an int or a vector of ints (one per trajectory), got %s %s" % (t.dtype, t.shape))
        t = np.ascontiguousarray(t, dtype=np.int32)
        up = self._ptr(h)
        _lib.check(_lib.lib().ddp_user_set_t0(up, t.ctypes.data_as(_lib.vp), len(t)))
        try:
            yield
        finally:
            _lib.lib().ddp_user_set_t0(up, None, 0)

    def _multiplier_arrays(self, multipliers, N, B, batched):
        """``(λ[nc,N,B], μ[B])`` of a ``multipliers=`` keyword as the library takes them; raises on a malformed shape"""
        if not self.nc:
            raise DDPError("multipliers= needs a DeviceProblem made with constraints=nc (DDP_USER_CONSTRAINTS)")
        try:
            lam, mu = multipliers
        except (TypeError, ValueError):
            raise DDPError("multipliers should be a pair (λ, μ)")
        lam = _lib.f64(lam)
        if not batched and lam.shape == (self.nc, N):
            lam = _lib.f64(lam[..., None])
        if lam.shape != (self.nc, N, B):
            raise DDPError("multipliers: λ should be (nc = %d, N = %d%s), got %s" % (self.nc, N, ", B = %d" % B if batched else "", lam.shape))
        mu = np.asarray(mu, dtype=np.float64)
        if mu.ndim == 0:
            mu = np.full(B, float(mu))
        if mu.shape != (B,):
            raise DDPError("multipliers: μ should be a number or (B = %d,), got %s" % (B, mu.shape))
        return lam, np.ascontiguousarray(mu)

    @_contextlib.contextmanager
    def _multipliers(self, h, multipliers, N, B, batched):
        """the multipliers ``(λ, μ)`` (``constraints=nc``) for the calls inside the block (ddp_user_set_multipliers); none are set
        afterwards, also when the call raises"""
        if multipliers is None:
            yield
            return
        lam, mu = self._multiplier_arrays(multipliers, N, B, batched)
        up = self._ptr(h)
        _lib.check(_lib.lib().ddp_user_set_multipliers(up, _lib.ptr(lam), _lib.ptr(mu), N, B))
        try:
            yield
        finally:
            _lib.lib().ddp_user_set_multipliers(up, None, None, 0, 0)

    def __del__(self):
        try:
            for h, up in self._made.values():
                _lib.lib().ddp_user_destroy(up)
            self._made = {}
        except Exception:
            pass


def _no_clock(t0):
    """the registered families have no clock: ``t0=`` with one of them is refused"""
    if t0 is not None:
        raise DDPError("t0= needs a DeviceProblem made with clock=True (DDP_USER_CLOCK)")


def _no_multipliers(multipliers):
    """the registered families have no constraints: ``multipliers=`` with one of them is refused"""
    if multipliers is not None:
        raise DDPError("multipliers= needs a DeviceProblem made with constraints=nc (DDP_USER_CONSTRAINTS)")


def _clock(problem, h, t0):
    """``with _clock(problem, h, t0):`` around a call — the clocks of a ``DeviceProblem(..., clock=True)``; any other problem has none"""
    if isinstance(problem, DeviceProblem):
        return problem._clock(h, t0)
    _no_clock(t0)
    return _contextlib.nullcontext()


def _user_shapes(problem, n, m):
    if (n, m) != (problem.n, problem.m):
        raise DDPError("DeviceProblem was compiled for n = %d, m = %d; the arrays have n = %d, m = %d" % (problem.n, problem.m, n, m))


def _lims(lims):
    if lims is None or np.size(lims) == 0:
        return None
    return _lib.f64(lims)


# ---------------------------------------------------------------------------------- back_pass
def back_pass(cx, cu, cxx, cxu, cuu, fx, fu, λ, regType, lims, x, u, *, fx_batched=None, cost_batched=None,
              batched_dynamics=None, batched_cost=None, handle=None):
    """Drop-in for ``back_pass(cx,cu,cxx,cxu,cuu,fx,fu,λ,regType,lims,x,u)`` (backward_pass.jl:217).

    Dispatch on array rank like the reference (``fx`` 2-D → LTI :217, 3-D → LTV :162, ``cxx`` 3-D →
    time-varying cost :179).  ``cx`` of rank 3 means a batch ``cx[n,N,B]``; then ``λ`` may be a vector
    of length B and ``fx``/``cxx`` of rank 4 are per-trajectory.
    Returns ``(diverge, GaussianPolicy, Vx, Vxx, dV)``; with a batch every output carries a trailing
    batch axis and ``diverge`` is an int32 vector.

    Per-trajectory TIME-INVARIANT operands (``fx[n,n,B]``, ``cxx[n,n,B]``) have the rank of the reference's time-varying ones and are
    never guessed from ``shape[2] == B``: pass ``batched_dynamics=True`` / ``batched_cost=True`` (``DDPAmd.back_pass`` has the same
    keywords; ``fx_batched`` / ``cost_batched`` are the older names of the same switches)."""
    h = handle or default_handle()
    if batched_dynamics is not None:
        assert fx_batched is None or bool(fx_batched) == bool(batched_dynamics), "fx_batched and batched_dynamics disagree"
        fx_batched = bool(batched_dynamics)
    if batched_cost is not None:
        assert cost_batched is None or bool(cost_batched) == bool(batched_cost), "cost_batched and batched_cost disagree"
        cost_batched = bool(batched_cost)
    cx, cu, u = _lib.f64(cx), _lib.f64(cu), _lib.f64(u)
    batched = cx.ndim == 3
    n, N = cx.shape[0], cx.shape[1]
    m = cu.shape[0]
    B = cx.shape[2] if batched else 1
    fx, fu, cxx, cxu, cuu = map(_lib.f64, (fx, fu, cxx, np.reshape(cxu, np.shape(cxu)), cuu))
    if fx_batched is None:
        fx_batched = fx.ndim == 4
    if cost_batched is None:
        cost_batched = cxx.ndim == 4
    fx_tv = (fx.ndim - int(fx_batched)) == 3
    cost_tv = (cxx.ndim - int(cost_batched)) == 3
    # the reference's @asserts (backward_pass.jl:221-225 / :8-11 / :183-187)
    assert cu.shape[:2] == (m, N), "size(cu) should be (m, N)"
    assert fx.shape[:2] == (n, n) and fu.shape[:2] == (n, m), "size(fx), size(fu)"
    assert cxx.shape[:2] == (n, n), "size(cxx) should be (n, n)"
    assert cxu.shape[:2] == (n, m), "size(cxu) should be (n, m)"
    assert cuu.reshape((m, m) + cuu.shape[2:] if cuu.ndim >= 2 else (m, m)).shape[:2] == (m, m), "size(cuu)"
    cuu = cuu.reshape((m, m) + (cuu.shape[2:] if cuu.ndim >= 2 else ()))
    # full extents (the reference asserts size(cxx) == (n,n,N) etc.; the C side would read out of bounds otherwise)
    tail_f = ((N,) if fx_tv else ()) + ((B,) if fx_batched else ())
    tail_c = ((N,) if cost_tv else ()) + ((B,) if cost_batched else ())
    assert cu.shape == (m, N) + ((B,) if batched else ()), "size(cu) should be (m, N[, B])"
    assert u.shape == cu.shape, "size(u) should be (m, N[, B])"
    assert fx.shape == (n, n) + tail_f and fu.shape == (n, m) + tail_f, "size(fx), size(fu): time / batch extents"
    assert cxx.shape == (n, n) + tail_c and cxu.shape == (n, m) + tail_c and cuu.shape == (m, m) + tail_c, "size(cxx), size(cxu), size(cuu): time / batch extents"
    L = _lims(lims)
    assert L is None or L.shape == (m, 2), "lims should be (m, 2)"
    d = _lib.BPDesc(n, m, N, B, int(fx_tv), int(fx_batched), int(cost_tv), int(cost_batched), int(regType),
                    int(L is not None))
    lam = np.ascontiguousarray(np.broadcast_to(np.asarray(λ, dtype=np.float64), (B,)))
    K = _lib.result_array((m, n, N, B)); k = _lib.result_array((m, N, B))
    Quu = _lib.result_array((m, m, N, B)); Vx = _lib.result_array((n, N, B))
    Vxx = _lib.result_array((n, n, N, B)); dV = np.zeros((2, B), order="F")
    div = np.zeros(B, dtype=np.int32)
    _lib.check(_lib.lib().ddp_back_pass_f64(h.raw, _C.byref(d), *map(_lib.ptr, (cx, cu, cxx, cxu, cuu, fx, fu, lam, L, u,
                                                                              K, k, Quu, Vx, Vxx, dV)),
                                            div.ctypes.data_as(_lib.i32p)))
    if not batched:
        pol = GaussianPolicy(N, n, m, K[..., 0], k[..., 0], np.zeros((m, m, N)), Quu[..., 0])
        return int(div[0]), pol, Vx[..., 0], Vxx[..., 0], dV[:, 0]
    pol = GaussianPolicy(N, n, m, K, k, np.zeros((m, m, N, B)), Quu)
    return div, pol, Vx, Vxx, dV


# -------------------------------------------------------------------------------------- boxQP
def boxQP(H, g, lower, upper, x0, *, maxIter=100, minGrad=1e-8, minRelImprove=1e-8, stepDec=0.6, minStep=1e-22,
          Armijo=0.1, handle=None):
    """Drop-in for ``boxQP(H,g,lower,upper,x0; ...)`` (boxQP.jl:29-36): returns ``(x, result, Hfree, free)``.
    ``H`` of rank 3 / vectors of rank 2 solve a batch (trailing axis)."""
    h = handle or default_handle()
    H, g, lower, upper, x0 = map(_lib.f64, (H, g, lower, upper, x0))
    batched = H.ndim == 3
    m = H.shape[0]
    cnt = H.shape[2] if batched else 1
    x = np.zeros((m, cnt), order="F"); Hf = np.zeros((m, m, cnt), order="F")
    res = np.zeros(cnt, dtype=np.int32); fr = np.zeros((m, cnt), dtype=np.uint8, order="F")
    o = _lib.QPOpts(maxIter, minGrad, minRelImprove, stepDec, minStep, Armijo)
    _lib.check(_lib.lib().ddp_boxqp_f64(h.raw, m, cnt, *map(_lib.ptr, (H, g, lower, upper, x0)), _C.byref(o),
                                        _lib.ptr(x), res.ctypes.data_as(_lib.i32p), _lib.ptr(Hf),
                                        fr.ctypes.data_as(_lib.u8p)))
    if not batched:
        free = fr[:, 0].astype(bool)
        nf = int(free.sum())
        return x[:, 0], int(res[0]), Hf[:nf, :nf, 0], free
    return x, res, Hf, fr.astype(bool)


def demoQP(*, n=500, rng=None, **kwargs):
    """``demoQP(;kwargs...)`` (src/boxQP.jl:190-199): ``H = M·M'`` with ``M = randn(n,n)``, ``g = randn(n)``, bounds ±1, a random
    start; returns ``boxQP``'s tuple and the wall time of the call in seconds."""
    import time as _time
    rng = rng if rng is not None else np.random.default_rng()
    M = rng.standard_normal((n, n))
    H, g = M @ M.T, rng.standard_normal(n)
    t0 = _time.perf_counter()
    out = boxQP(H, g, -np.ones(n), np.ones(n), rng.standard_normal(n), **kwargs)
    return out + (_time.perf_counter() - t0,)


# ------------------------------------------------------------------------------- demos (problem generators + solver settings)
def demo_linear(*, B=None, rng=None, T=1000, n=10, m=2, h=0.01, **kwargs):
    """``demo_linear(;kwargs...)`` (src/demo_linear.jl:5-60): random stable LTI system ``A = exp(h(A0 - A0'))``, ``B = h·randn``,
    ``Q = h·I``, ``R = 0.1h·I``, ``x0 = ones(n)``, ``u0 = 0.1·randn(m,T)``, no control limits; runs ``iLQG`` with the given keyword
    arguments and returns its tuple.  ``B`` solves a batch of independent problems (same system, own ``u0``) — the reference
    runs one.  NumPy's generator replaces Julia's (the draws differ, the distribution does not)."""
    import scipy.linalg as _sla
    rng = rng if rng is not None else np.random.default_rng()
    A0 = rng.standard_normal((n, n))
    A = _sla.expm(h * (A0 - A0.T))                             # skew-symmetric generator: pure imaginary eigenvalues
    Bm = h * rng.standard_normal((n, m))
    Q, R = h * np.eye(n), 0.1 * h * np.eye(m)
    x0 = np.ones(n) if B is None else np.ones((n, B))
    u0 = 0.1 * rng.standard_normal((m, T) if B is None else (m, T, B))
    return iLQG(LQProblem(A, Bm, Q, R), x0, u0, **kwargs)


def demo_pendcart(*, x0=(np.pi - 0.6, 0.0, 0.0, 0.0), goal=(np.pi, 0.0, 0.0, 0.0), Q=None, R=1.0, lims=None, T=600, B=None, **kwargs):
    """``demo_pendcart(;x0, goal, Q, R, lims, T)`` (src/system_pendcart.jl:42-212) with the reference's solver settings
    (``regType=2, α=exp10.(range(0.2,stop=-3,length=6)), λmax=1e15, tol_fun=tol_grad=1e-8, max_iter=1000``) from ``u0 = 0``
    (the reference passes ``0*u00``: its LQR simulation only feeds the comparison plot).  ``B`` replicates the problem."""
    Q = np.diag([10.0, 1.0, 2.0, 1.0]) if Q is None else np.asarray(Q, dtype=np.float64)
    lims = 5.0 * np.array([[-1.0, 1.0]]) if lims is None else lims
    prob = PendcartProblem(Q=Q, R=np.array([[float(R)]]), goal=np.asarray(goal, dtype=np.float64))
    x0 = np.asarray(x0, dtype=np.float64)
    if B is not None:
        x0 = np.tile(x0[:, None], (1, B))
    u0 = np.zeros((1, T) if B is None else (1, T, B))
    kw = dict(regType=2, α=10.0 ** np.linspace(0.2, -3, 6), λmax=1e15, tol_fun=1e-8, tol_grad=1e-8, max_iter=1000)
    kw.update(kwargs)
    return iLQG(prob, x0, u0, lims=lims, **kw)


# ------------------------------------------------------------------------------- MPC warm start
def mpc_shift(a, shift=1, *, zero_tail=False, batched=None, handle=None):
    """Receding-horizon shift of a time-major array ``a[...,N(,B)]`` (controls, nominal states, gains; ``batched`` says whether the
    last axis is the batch — default: yes for more than two axes) by ``shift`` steps through
    ``ddp_mpc_shift_f64_dev``: ``out[:,i] = a[:,i+shift]``, the vacated tail repeats the last column (or is zero).  New — the
    reference has no MPC loop; its hook is the pre-rolled ``x0[n,N]`` + ``cost`` warm start (iLQG.jl:193-197)."""
    h = handle or default_handle()
    a = _lib.f64(a)
    if batched is None:
        batched = a.ndim > 2
    lead = a.shape[:-2] if batched else a.shape[:-1]
    N, B = (a.shape[-2], a.shape[-1]) if batched else (a.shape[-1], 1)
    d = int(np.prod(lead))
    src = h.to_device(a)
    dst = h.malloc(a.nbytes)
    try:
        _lib.check(_lib.lib().ddp_mpc_shift_f64_dev(h.raw, d, N, B, int(shift), int(bool(zero_tail)), src, dst))
        out = h.to_host(dst, a.shape)
    finally:
        h.free(src); h.free(dst)
    return out


def _check_problem(problem, n, m, N, B):
    """extents of a registered family's arrays against the call's sizes (the C side trusts them)"""
    if problem.kind == 1:
        if (n, m) != (4, 1):
            raise ValueError("PendcartProblem has n = 4, m = 1")
        return
    tail = ((N,) if problem.dyn_tv else ()) + ((B,) if problem.dyn_batched else ())
    A, Bm = np.asarray(problem.A), np.asarray(problem.B)
    if A.shape != (n, n) + tail or Bm.shape != (n, m) + tail:
        raise ValueError("LQProblem: A should be (n,n%s), B (n,m%s)" % ((",".join([""] + ["N"] * problem.dyn_tv + ["B"] * problem.dyn_batched),) * 2))
    if np.shape(problem.Q) != (n, n) or np.shape(np.atleast_2d(problem.R)) != (m, m):
        raise ValueError("LQProblem: Q should be (n,n), R (m,m)")


# ------------------------------------------------------------------------------- forward_pass
def forward_pass(traj_new, x0, u, x, α, problem, lims, diff=None, *, handle=None, params=None, t0=None, multipliers=None, model=None):
    """Drop-in for ``forward_pass(traj_new,x0,u,x,α,f,costfun,lims,diff)`` (forward_pass.jl:9) with a
    registered ``problem`` standing in for the closures ``f``/``costfun``; ``diff``: ``None`` (``-``) or a ``WrappedDiff``.
    ``traj_new`` may be an empty ``GaussianPolicy`` (then ``x`` is ignored, iLQG.jl:185).
    A vector ``α`` rolls all step sizes out concurrently (outputs get a trailing α axis).
    A ``DeviceProblem`` takes ``params`` (default: its own); its ``diff`` is compiled in; made with ``clock=True`` it takes ``t0``, made
    with ``constraints=nc`` it takes ``multipliers=(λ, μ)`` (the augmented cost); made with ``fitted=True`` (or with ``wave=True,
    fitted_wave=True``: ``n <= 64``, ``m <= 32``, kernel ``ddp_user_rollout_fit_wave``) it takes ``model=(fx, fu, fc)``, the tables
    ``fit_dynamics`` returns (``(n,n,N)``, ``(n,m,N)``, ``(n,N)`` [+ batch axis]): the rollout then runs
    ``x̂[i+1] = fx_i x̂_i + fu_i û_i + fc_i`` under the problem's cost (``ddp_user_rollout_fit``; slot ``N-1`` of the tables is not read).
    With ``traj_new=None`` that is the open-loop rollout which makes ``(x, u)`` consistent with the fit before ``kl.iLQGkl(..., fitted=True)``.
    Returns ``(xnew, unew, cnew)``."""
    if isinstance(problem, DeviceProblem):
        return _user_forward_pass(traj_new, x0, u, x, α, problem, lims, diff, handle=handle, params=params, t0=t0, multipliers=multipliers,
                                  model=model)
    if model is not None:
        raise DDPError("model= needs a DeviceProblem made with fitted=True (DDP_USER_FITTED) or with wave=True, fitted_wave=True (DDP_USER_FITTED_WAVE)")
    h = handle or default_handle()
    _no_clock(t0)
    _no_multipliers(multipliers)
    u, x0 = _lib.f64(u), _lib.f64(x0)
    batched = u.ndim == 3
    m, N = u.shape[:2]
    n = x0.shape[0]
    B = u.shape[2] if batched else 1
    dp = _DevProblem(problem, N, B, diff)
    if x0.shape != ((n, B) if batched else (n,)) and not (not batched and x0.shape == (n, 1)):
        raise ValueError("x0 should be (n,) — (n, B) with a batched u")
    _check_problem(problem, n, m, N, B)
    alphas = np.atleast_1d(np.asarray(α, dtype=np.float64))
    na = len(alphas)
    empty = traj_new is None or traj_new.isempty()
    K = None if empty else _lib.f64(traj_new.K)
    k = None if empty else _lib.f64(traj_new.k)
    xx = None if empty else _lib.f64(x)
    if not empty:
        tb = (B,) if batched else ()
        if K.shape != (m, n, N) + tb or k.shape != (m, N) + tb or xx.shape != (n, N) + tb:
            raise ValueError("traj_new.K, traj_new.k, x should be (m,n,N), (m,N), (n,N) [+ batch axis]")
    L = _lims(lims)
    CL = dp.cost_len
    xnew = _lib.result_array((n, N, B, na)); unew = _lib.result_array((m, N, B, na))
    cnew = _lib.result_array((CL, B, na)); csum = np.zeros((B, na), order="F")
    _lib.check(_lib.lib().ddp_forward_pass_f64(h.raw, _C.byref(dp.struct), _lib.ptr(K), _lib.ptr(k), _lib.ptr(x0),
                                               _lib.ptr(u), _lib.ptr(xx), _lib.ptr(alphas), na, _lib.ptr(L),
                                               _lib.ptr(xnew), _lib.ptr(unew), _lib.ptr(cnew), _lib.ptr(csum)))
    if not batched:
        xnew, unew, cnew = xnew[:, :, 0], unew[:, :, 0], cnew[:, 0]
    if np.ndim(α) == 0:
        xnew, unew, cnew = xnew[..., 0], unew[..., 0], cnew[..., 0]
    return xnew, unew, cnew


# ------------------------------------------------------------------------------------------ df
def df(problem, x, u, *, handle=None, params=None, t0=None, multipliers=None):
    """The ``df`` closure of the registered families (STEP 1, iLQG.jl:225-229).  Returns
    ``(fx,fu,fxx,fxu,fuu,cx,cu,cxx,cxu,cuu)`` like the reference (second-order terms are ``[]``).
    A ``DeviceProblem`` returns its ``derivatives``: ``cxx[n,n,N(,B)]`` ... (``[n,n(,B)]`` with ``const_hessian``)."""
    if isinstance(problem, DeviceProblem):
        return _user_df(problem, x, u, handle=handle, params=params, t0=t0, multipliers=multipliers)
    h = handle or default_handle()
    _no_clock(t0)
    _no_multipliers(multipliers)
    x, u = _lib.f64(x), _lib.f64(u)
    batched = u.ndim == 3
    m, N = u.shape[:2]
    n = x.shape[0]
    B = u.shape[2] if batched else 1
    dp = _DevProblem(problem, N, B)
    cx = _lib.result_array((n, N, B)); cu = _lib.result_array((m, N, B))
    pend = problem.kind == 1
    fx = _lib.result_array((n, n, N, B)) if pend else None
    fu = _lib.result_array((n, m, N, B)) if pend else None
    _lib.check(_lib.lib().ddp_df_f64(h.raw, _C.byref(dp.struct), _lib.ptr(x), _lib.ptr(u), _lib.ptr(cx), _lib.ptr(cu),
                                     _lib.ptr(fx), _lib.ptr(fu)))
    if not pend:
        fx, fu = dp.A, dp.B
    elif not batched:
        fx, fu = fx[..., 0], fu[..., 0]
    if not batched:
        cx, cu = cx[..., 0], cu[..., 0]
    e = np.zeros((0,))
    return fx, fu, e, e, e, cx, cu, dp.Q, np.zeros((n, m)), dp.R


def _user_batch(x_or_x0, u, problem, x0_has_time=False):
    u = _lib.f64(u)
    if u.ndim not in (2, 3):
        raise DDPError("u should be (m, N) or (m, N, B)")
    batched = u.ndim == 3
    m, N = u.shape[:2]
    B = u.shape[2] if batched else 1
    n = np.shape(x_or_x0)[0]
    _user_shapes(problem, n, m)
    return u, batched, n, m, N, B


def _fitted_tables(problem, model, n, m, N, B, batched, who):
    """``(fx, fu, fc)`` of a ``model=`` keyword as the library takes them, ``[.,.,N,B]``; refused by name on a problem made without
    ``fitted=True`` or ``fitted_wave=True``, or on a malformed shape, before anything is launched"""
    if not (problem.fitted or problem.fitted_wave):
        raise DDPError("%s: a fitted model needs a DeviceProblem made with fitted=True (DDP_USER_FITTED)%s"
                       % (who, "; a wave=True problem: with fitted_wave=True (DDP_USER_FITTED_WAVE)" if problem.wave else ""))
    try:
        fx, fu, fc = model
    except (TypeError, ValueError):
        raise DDPError("%s: the fitted model should be a triple (fx, fu, fc)" % who)
    if fx is None or fu is None or fc is None:
        raise DDPError("%s: the fitted model needs fx, fu and fc (fc is None?)" % who if fc is None else "%s: the fitted model needs fx, fu and fc" % who)
    fx, fu, fc = _lib.f64(fx), _lib.f64(fu), _lib.f64(fc)
    tb = (B,) if batched else ()
    if fx.shape != (n, n, N) + tb or fu.shape != (n, m, N) + tb or fc.shape != (n, N) + tb:
        raise DDPError("%s: fx, fu, fc should be (n,n,N), (n,m,N), (n,N) = (%d,%d,%d), (%d,%d,%d), (%d,%d)%s, got %s, %s, %s"
                       % (who, n, n, N, n, m, N, n, N, " + (B = %d,)" % B if batched else "", fx.shape, fu.shape, fc.shape))
    return fx, fu, fc


def _user_forward_pass(traj_new, x0, u, x, α, problem, lims, diff, *, handle=None, params=None, t0=None, multipliers=None, model=None):
    u, batched, n, m, N, B = _user_batch(x0, u, problem)
    tables = None if model is None else _fitted_tables(problem, model, n, m, N, B, batched, "forward_pass")
    h = handle or default_handle()                         # (behind the checks that need no device)
    x0 = _lib.f64(x0)
    if x0.shape != ((n, B) if batched else (n,)) and not (not batched and x0.shape == (n, 1)):
        raise DDPError("x0 should be (n,) — (n, B) with a batched u")
    if diff is not None and _diff_mask(diff, n) != problem.diff_mask:
        raise DDPError("DeviceProblem: diff is compiled into the problem (DeviceProblem(..., diff=...))")
    P, pb = problem._params(B, params)
    alphas = np.atleast_1d(np.asarray(α, dtype=np.float64))
    na = len(alphas)
    if not 1 <= na <= 16:
        raise DDPError("1 to 16 step sizes")
    empty = traj_new is None or traj_new.isempty()
    K = None if empty else _lib.f64(traj_new.K)
    k = None if empty else _lib.f64(traj_new.k)
    xx = None if empty else _lib.f64(x)
    if not empty:
        tb = (B,) if batched else ()
        if K.shape != (m, n, N) + tb or k.shape != (m, N) + tb or xx.shape != (n, N) + tb:
            raise DDPError("traj_new.K, traj_new.k, x should be (m,n,N), (m,N), (n,N) [+ batch axis]")
    L = _lims(lims)
    if L is not None and L.shape != (m, 2):
        raise DDPError("lims should be (m, 2)")
    CL = problem.cost_len(N)
    xnew = _lib.result_array((n, N, B, na)); unew = _lib.result_array((m, N, B, na))
    cnew = _lib.result_array((CL, B, na)); csum = np.zeros((B, na), order="F")
    up = problem._ptr(h)
    with problem._clock(h, t0), problem._multipliers(h, multipliers, N, B, batched):
        if tables is not None:
            _lib.check(_lib.lib().ddp_user_rollout_fit_f64(h.raw, up, N, B, _lib.ptr(P), pb, _lib.ptr(K), _lib.ptr(k), _lib.ptr(x0), _lib.ptr(u),
                                                           _lib.ptr(xx), _lib.ptr(alphas), na, _lib.ptr(L), *map(_lib.ptr, tables),
                                                           _lib.ptr(xnew), _lib.ptr(unew), _lib.ptr(cnew), _lib.ptr(csum)))
        else:
            _lib.check(_lib.lib().ddp_user_forward_pass_f64(h.raw, up, N, B, _lib.ptr(P), pb, _lib.ptr(K), _lib.ptr(k), _lib.ptr(x0), _lib.ptr(u),
                                                            _lib.ptr(xx), _lib.ptr(alphas), na, _lib.ptr(L), _lib.ptr(xnew), _lib.ptr(unew),
                                                            _lib.ptr(cnew), _lib.ptr(csum)))
    if not batched:
        xnew, unew, cnew = xnew[:, :, 0], unew[:, :, 0], cnew[:, 0]
    if np.ndim(α) == 0:
        xnew, unew, cnew = xnew[..., 0], unew[..., 0], cnew[..., 0]
    return xnew, unew, cnew


def _user_df(problem, x, u, *, handle=None, params=None, t0=None, multipliers=None):
    h = handle or default_handle()
    u, batched, n, m, N, B = _user_batch(x, u, problem)
    x = _lib.f64(x)
    if x.shape != ((n, N, B) if batched else (n, N)):
        raise DDPError("x should be (n, N) — (n, N, B) with a batched u")
    P, pb = problem._params(B, params)
    ht = () if problem.const_hessian else (N,)
    fx = _lib.result_array((n, n, N, B)); fu = _lib.result_array((n, m, N, B))
    cx = _lib.result_array((n, N, B)); cu = _lib.result_array((m, N, B))
    cxx = _lib.result_array((n, n) + ht + (B,)); cxu = _lib.result_array((n, m) + ht + (B,)); cuu = _lib.result_array((m, m) + ht + (B,))
    up = problem._ptr(h)
    with problem._clock(h, t0), problem._multipliers(h, multipliers, N, B, batched):
        _lib.check(_lib.lib().ddp_user_df_f64(h.raw, up, N, B, _lib.ptr(P), pb, _lib.ptr(x), _lib.ptr(u),
                                              *map(_lib.ptr, (fx, fu, cx, cu, cxx, cxu, cuu))))
    if not batched:
        fx, fu, cx, cu, cxx, cxu, cuu = (a[..., 0] for a in (fx, fu, cx, cu, cxx, cxu, cuu))
    e = np.zeros((0,))
    return fx, fu, e, e, e, cx, cu, cxx, cxu, cuu


def vhess(problem, x, u, v, *, handle=None, params=None):
    """``H[n+m, n+m, N(, B)] = Σ_k v[k, i] ∂²f_k/∂z∂z`` at ``(x[:, i], u[:, i], i)``, ``z = [x; u]``, of a ``DeviceProblem`` made with
    ``second_order=True`` or ``second_order_wave=True``: the ``vectens(v, fxx)`` / ``fxu`` / ``fuu`` blocks of backward_pass.jl:106-123 without the tensors,
    exactly symmetric."""
    if not isinstance(problem, DeviceProblem):
        raise TypeError("vhess: a DeviceProblem is needed")
    h = handle or default_handle()
    u, batched, n, m, N, B = _user_batch(x, u, problem)
    x, v = _lib.f64(x), _lib.f64(v)
    if x.shape != ((n, N, B) if batched else (n, N)) or v.shape != x.shape:
        raise DDPError("x and v should be (n, N) — (n, N, B) with a batched u")
    P, pb = problem._params(B, params)
    H = _lib.result_array((n + m, n + m, N, B))
    _lib.check(_lib.lib().ddp_user_vhess_f64(h.raw, problem._ptr(h), N, B, _lib.ptr(P), pb, _lib.ptr(x), _lib.ptr(u), _lib.ptr(v), _lib.ptr(H)))
    return H if batched else H[..., 0]


def back_pass_ddp(problem, cx, cu, cxx, cxu, cuu, fx, fu, λ, regType, lims, x, u, *, handle=None, params=None):
    """The second-order backward pass (backward_pass.jl:81-160) of a ``DeviceProblem`` made with ``second_order=True`` or
    ``second_order_wave=True`` (n <= 64, m <= 32, ``ddp_user_back_pass2_wave``): arguments as ``back_pass`` with the arrays ``df(problem, x, u)`` returns (time-varying, a trailing batch axis with a batched ``u``; with
    ``const_hessian`` the Hessians carry no time axis), the curvature terms derived on the device at ``(x, u)``.  Returns what
    ``back_pass`` returns: ``(diverge, GaussianPolicy, Vx, Vxx, dV)``."""
    if not isinstance(problem, DeviceProblem):
        raise TypeError("back_pass_ddp: a DeviceProblem is needed")
    h = handle or default_handle()
    u, batched, n, m, N, B = _user_batch(x, u, problem)
    tb = (B,) if batched else ()
    ht = () if problem.const_hessian else (N,)
    x, cx, cu, cxx, cxu, cuu, fx, fu = map(_lib.f64, (x, cx, cu, cxx, cxu, cuu, fx, fu))
    want = {"x": (x, (n, N)), "cx": (cx, (n, N)), "cu": (cu, (m, N)), "fx": (fx, (n, n, N)), "fu": (fu, (n, m, N)),
            "cxx": (cxx, (n, n) + ht), "cxu": (cxu, (n, m) + ht), "cuu": (cuu, (m, m) + ht)}
    for name, (arr, shp) in want.items():
        if arr.shape != shp + tb:
            raise DDPError("back_pass_ddp: %s should be %s, got %s" % (name, shp + tb, arr.shape))
    L = _lims(lims)
    if L is not None and L.shape != (m, 2):
        raise DDPError("lims should be (m, 2)")
    P, pb = problem._params(B, params)
    lam = np.ascontiguousarray(np.broadcast_to(np.asarray(λ, dtype=np.float64), (B,)))
    K = _lib.result_array((m, n, N, B)); k = _lib.result_array((m, N, B)); Quu = _lib.result_array((m, m, N, B))
    Vx = _lib.result_array((n, N, B)); Vxx = _lib.result_array((n, n, N, B)); dV = np.zeros((2, B), order="F")
    div = np.zeros(B, dtype=np.int32)
    _lib.check(_lib.lib().ddp_user_back_pass_f64(h.raw, problem._ptr(h), N, B, _lib.ptr(P), pb,
                                                 *map(_lib.ptr, (x, u, fx, fu, cx, cu, cxx, cxu, cuu, lam)), int(regType), _lib.ptr(L),
                                                 *map(_lib.ptr, (K, k, Quu, Vx, Vxx, dV)), div.ctypes.data_as(_lib.vp)))
    if not batched:
        return int(div[0]), GaussianPolicy(N, n, m, K[..., 0], k[..., 0], np.zeros((m, m, N)), Quu[..., 0]), Vx[..., 0], Vxx[..., 0], dV[:, 0]
    return div, GaussianPolicy(N, n, m, K, k, np.zeros((m, m, N, B)), Quu), Vx, Vxx, dV


def costfun(problem, x, u, *, handle=None, params=None, t0=None, multipliers=None):
    """The ``costfun`` closure of a ``DeviceProblem`` on given trajectories: ``cost[CL(,B)]`` (CL = N, N+1 with ``terminal``)."""
    if not isinstance(problem, DeviceProblem):
        raise TypeError("costfun: a DeviceProblem is needed (the registered families evaluate their cost inside forward_pass)")
    h = handle or default_handle()
    u, batched, n, m, N, B = _user_batch(x, u, problem)
    x = _lib.f64(x)
    if x.shape != ((n, N, B) if batched else (n, N)):
        raise DDPError("x should be (n, N) — (n, N, B) with a batched u")
    P, pb = problem._params(B, params)
    cost = _lib.result_array((problem.cost_len(N), B))
    csum = np.zeros(B)
    with problem._clock(h, t0), problem._multipliers(h, multipliers, N, B, batched):
        _lib.check(_lib.lib().ddp_user_costfun_f64(h.raw, problem._ptr(h), N, B, _lib.ptr(P), pb, _lib.ptr(x), _lib.ptr(u), _lib.ptr(cost),
                                                   _lib.ptr(csum)))
    return cost if batched else cost[:, 0]


def constraints(problem, x, u, *, handle=None, params=None):
    """``g[nc, N(, B)]`` of a ``DeviceProblem`` made with ``constraints=nc``: the user's ``constraints`` at every ``(x[:, i], u[:, i], i)``;
    feasible where ``g <= 0``."""
    if not isinstance(problem, DeviceProblem) or not problem.nc:
        raise DDPError("constraints: a DeviceProblem made with constraints=nc (DDP_USER_CONSTRAINTS) is needed")
    h = handle or default_handle()
    u, batched, n, m, N, B = _user_batch(x, u, problem)
    x = _lib.f64(x)
    if x.shape != ((n, N, B) if batched else (n, N)):
        raise DDPError("x should be (n, N) — (n, N, B) with a batched u")
    P, pb = problem._params(B, params)
    g = _lib.result_array((problem.nc, N, B))
    _lib.check(_lib.lib().ddp_user_constraints_f64(h.raw, problem._ptr(h), N, B, _lib.ptr(P), pb, _lib.ptr(x), _lib.ptr(u), _lib.ptr(g)))
    return g if batched else g[..., 0]


# ------------------------------------------------------------------------------ sample_policy
def _seed_words(seed):
    """the two 32-bit words of a seed in [0, 2^64), as the C ints that carry their bits"""
    seed = int(seed)
    if not 0 <= seed < 1 << 64:
        raise DDPError("seed should be an int in [0, 2^64), got %d" % seed)
    return _C.c_int32(seed & 0xffffffff).value, _C.c_int32(seed >> 32).value


def normal(seed, m, N, S, B=None, *, sample0=0, traj0=0, handle=None):
    """``ξ[m, N, S(, B)]``: the standard normals ``sample_policy(..., seed=seed)`` draws — Philox4x32-10 with counter
    ``(i, sample0 + s, traj0 + b, q)`` and key ``seed``, one Box-Muller pair per call (include/ddp_amd.h, DDP_USER_SAMPLE).  A block
    taken with ``sample0`` / ``traj0`` is the slice of the full array, bit for bit."""
    lo, hi = _seed_words(seed)
    h = handle or default_handle()
    nb = 1 if B is None else int(B)
    xi = _lib.result_array((int(m), int(N), int(S), nb))
    _lib.check(_lib.lib().ddp_normal_f64(h.raw, lo, hi, int(m), int(N), int(S), nb, int(sample0), int(traj0), _lib.ptr(xi)))
    return xi[..., 0] if B is None else xi


def sample_policy(problem, traj, x0, x, u, S, *, seed=0, noise=None, lims=None, plant=False, params=None, moments=False, sample0=0,
                  traj0=0, handle=None):
    """``S`` closed-loop rollouts per trajectory of the policy ``traj`` (``K``, ``Σ``; a solve's ``traj_new``) around the nominal
    ``(x, u)`` from ``x0``, on a ``DeviceProblem`` made with ``sample=True`` (``n <= 32``, ``m <= 8``) or with ``wave=True,
    sample_wave=True`` (``n <= 64``, ``m <= 32``): at step ``i``
    ``û = u[:, i] + L_i ξ_i + K[:, :, i] diff(x̂, x[:, i])``, clamped to ``lims``, with ``L_i`` the lower Cholesky factor of ``Σ[:, :, i]``
    (the reference's docstring uses the upper one, whose samples do not have covariance ``Σ`` for m > 1) — the sampling step of the
    guided-policy-search loop.  ``ξ`` is generated on the device from ``seed`` (an int in [0, 2^64); see ``normal``), or taken from
    ``noise[m, N, S(, B)]``.  ``traj.Σ`` all zero or empty: the noise-free closed loop.  ``plant=True`` runs the problem's ``plant``
    instead of its ``dynamics``.  Returns ``(xs[n,N,S(,B)], us[m,N,S(,B)], cs[CL,S(,B)], info)``; ``info`` holds ``csum[S(,B)]``,
    ``status`` (0, or ``i + 1`` of the first step whose ``Σ`` is not positive definite: that trajectory's outputs are NaN) and, with
    ``moments=True``, ``mean[n,N(,B)]`` and the unbiased ``cov[n,n,N(,B)]`` over the samples.  ``sample0`` / ``traj0`` offset the
    generator's sample and trajectory counters: a shard reproduces its slice of the full call bit for bit."""
    if not isinstance(problem, DeviceProblem):
        raise TypeError("sample_policy: a DeviceProblem is needed")
    h = handle or default_handle()
    u, batched, n, m, N, B = _user_batch(x0, u, problem)
    x0, x, K = _lib.f64(x0), _lib.f64(x), _lib.f64(traj.K)
    tb = (B,) if batched else ()
    if x0.shape != (n,) + tb and not (not batched and x0.shape == (n, 1)):
        raise DDPError("x0 should be (n,) — (n, B) with a batched u")
    if K.shape != (m, n, N) + tb or x.shape != (n, N) + tb:
        raise DDPError("traj.K, x should be (m,n,N), (n,N) [+ batch axis]")
    S = int(S)
    Sg = getattr(traj, "Σ", None)
    Sg = None if Sg is None or np.size(Sg) == 0 or not np.any(Sg) else _lib.f64(Sg)
    if Sg is not None and Sg.shape != (m, m, N) + tb:
        raise DDPError("traj.Σ should be (m,m,N) [+ batch axis]")
    if noise is not None:
        noise = _lib.f64(noise)
        if noise.shape != (m, N, S) + tb:
            raise DDPError("noise should be (m, N, S) [+ batch axis], got %s" % (noise.shape,))
    L = _lims(lims)
    if L is not None and L.shape != (m, 2):
        raise DDPError("lims should be (m, 2)")
    P, pb = problem._params(B, params)
    lo, hi = _seed_words(seed)
    CL = problem.cost_len(N)
    xs = _lib.result_array((n, N, S, B)); us = _lib.result_array((m, N, S, B)); cs = _lib.result_array((CL, S, B))
    csum = np.zeros((S, B), order="F"); status = np.zeros(B, dtype=np.int32)
    mean = _lib.result_array((n, N, B)) if moments else None
    cov = _lib.result_array((n, n, N, B)) if moments else None
    _lib.check(_lib.lib().ddp_user_sample_f64(h.raw, problem._ptr(h), N, B, S, _lib.ptr(P), pb, _lib.ptr(K), _lib.ptr(Sg), _lib.ptr(x0),
                                              _lib.ptr(u), _lib.ptr(x), _lib.ptr(L), _lib.ptr(noise), lo, hi, int(sample0), int(traj0),
                                              int(bool(plant)), _lib.ptr(xs), _lib.ptr(us), _lib.ptr(cs), _lib.ptr(csum), _lib.ptr(mean),
                                              _lib.ptr(cov), status.ctypes.data_as(_lib.vp)))
    info = {"csum": csum, "status": status}
    if moments:
        info["mean"], info["cov"] = mean, cov
    if not batched:
        xs, us, cs = xs[..., 0], us[..., 0], cs[..., 0]
        info = {k: (int(v[0]) if k == "status" else v[..., 0]) for k, v in info.items()}
    return xs, us, cs, info


# ------------------------------------------------------------------------------ fit_dynamics
def fit_dynamics(xs, us, *, ridge=0.0, prior=None, handle=None, wide=False):
    """Time-varying linear-Gaussian dynamics ``x̂[i+1] ≈ fx[:,:,i] x̂[i] + fu[:,:,i] û[i] + fc[:,i]`` with residual covariance
    ``cov[:,:,i]``, fitted on the device to the rollouts ``xs[n,N,S(,B)]``, ``us[m,N,S(,B)]`` that ``sample_policy`` returns — the
    step between sampling and ``kl.iLQGkl`` in a guided-policy-search round, and the way to a model of a ``plant`` whose equations
    the controller does not know.  Per step ``i < N-1`` and trajectory, with ``w = [x̂_i; û_i; x̂_{i+1}]`` (``z`` its first ``n+m``
    entries, ``y`` the last ``n``): ``μ`` the sample mean, ``C`` the unbiased covariance of the centred samples — with
    ``prior=(Φ, μ0, m0, n0)`` the normal-inverse-Wishart posterior ``(E + Φ + (S m0/(S+m0)) (μ-μ0)(μ-μ0)ᵀ)/(S+n0)``, ``E`` the centred
    sum; ``Φ[p,p]``, ``μ0[p]`` (``p = 2n+m``) serve every step, ``Φ[p,p,N(,B)]``, ``μ0[p,N(,B)]`` one each — then
    ``[fx fu] = (A⁻¹ C_zy)ᵀ`` with ``A = C_zz + ridge·I`` (Cholesky, ``ridge >= 0`` absolute), ``fc = μ_y - [fx fu] μ_z`` and
    ``cov = C_yy - [fx fu] C_zy``, symmetrised.  Returns ``(fx[n,n,N(,B)], fu[n,m,N(,B)], fc[n,N(,B)], cov[n,n,N(,B)],
    status[N(,B)])``; ``kl.Model(fx, fu, R1)`` takes the first two as they are.  ``status`` is per step: 0, or ``c + 1`` for the first
    pivot ``c`` of the factorisation that is not a positive finite number (``n + m + 1``: every pivot is fine but the results are not
    finite, a NaN in ``x̂_{i+1}``) — that step's outputs are NaN and no other step is touched.
    Every rollout of the sampler starts at the same ``x0``, so without ``ridge`` and ``prior`` step 0 reports pivot 1.  Slot ``N-1`` has
    no transition: zeros.  1 <= n <= 32, 1 <= m <= 8, S >= 2; with ``wide=True`` 1 <= n <= 64, 1 <= m <= 32 (the box of
    ``sample_policy(..., sample_wave=True)`` and ``kl.iLQGkl(..., wide=True)``): a shape inside the small box keeps its kernel and
    its bits, every other one runs the blocked kernel of ``ddp_fit_dynamics_wide_f64``, which forms ``cov`` as ``C_yy - Y1ᵀY1`` with
    ``Y1 = L⁻¹C_zy`` (the same matrix).  Two calls give the same bits, and a call on some of the trajectories gives the bits of
    their slice of the full call."""
    xs, us = _lib.f64(xs), _lib.f64(us)
    if xs.ndim not in (3, 4) or us.ndim != xs.ndim:
        raise DDPError("fit_dynamics: xs, us should be (n, N, S), (m, N, S) [+ batch axis], got %s, %s" % (xs.shape, us.shape))
    batched = xs.ndim == 4
    if not batched:
        xs, us = xs[..., None], us[..., None]
    n, N, S, B = xs.shape
    m = us.shape[0]
    if us.shape[1:] != (N, S, B):
        raise DDPError("fit_dynamics: us (m, %s) does not match xs (n, %s) in N, S [, B]" % (us.shape[1:], xs.shape[1:]))
    p = 2 * n + m
    Phi = mu0 = None
    m0 = n0 = 0.0
    layout = 0
    if prior is not None:
        Phi, mu0, m0, n0 = prior
        Phi, mu0, m0, n0 = _lib.f64(Phi), _lib.f64(mu0), float(m0), float(n0)
        tb = (B,) if batched else ()
        if Phi.shape == (p, p) and mu0.shape == (p,):
            layout = 0
        elif Phi.shape == (p, p, N) + tb and mu0.shape == (p, N) + tb:
            layout = 1
        else:
            raise DDPError("fit_dynamics: prior Φ, μ0 should be (p, p), (p,) or (p, p, N), (p, N) [+ batch axis] with p = 2n + m = %d, got %s, %s"
                           % (p, Phi.shape, mu0.shape))
    h = handle or default_handle()
    fx = _lib.result_array((n, n, N, B)); fu = _lib.result_array((n, m, N, B)); fc = _lib.result_array((n, N, B))
    cov = _lib.result_array((n, n, N, B)); status = np.zeros((N, B), dtype=np.int32, order="F")
    entry = _lib.lib().ddp_fit_dynamics_wide_f64 if wide else _lib.lib().ddp_fit_dynamics_f64
    _lib.check(entry(h.raw, n, m, N, S, B, _lib.ptr(xs), _lib.ptr(us), float(ridge), _lib.ptr(Phi), _lib.ptr(mu0), m0, n0, layout, _lib.ptr(fx),
                     _lib.ptr(fu), _lib.ptr(fc), _lib.ptr(cov), status.ctypes.data_as(_lib.vp)))
    if not batched:
        return fx[..., 0], fu[..., 0], fc[..., 0], cov[..., 0], status[..., 0]
    return fx, fu, fc, cov, status


# ------------------------------------------------------------------------------ fit_cost
def fit_cost(problem, xs, us, x, u, *, params=None, handle=None):
    """The quadratic cost model of a guided-policy-search round, fitted on the device to the rollouts ``xs[n,N,S(,B)]``, ``us[m,N,S(,B)]``
    that ``sample_policy`` returns, around the nominal ``x[n,N(,B)]``, ``u[m,N(,B)]``, for a ``DeviceProblem`` made with
    ``cost_fit=True``: the problem's cost is expanded to second order at every sample ``(x̂_s, û_s)``, the expansion is moved to the
    nominal (``δx = diff(x̂_s, x_i)`` with the problem's ``diff``, ``δu = û_s - u_i``) and the results are averaged over the samples,
    ``cxx = mean cxx_s`` (``cxu``, ``cuu`` alike), ``cx = mean (cx_s - cxx_s δx - cxu_s δu)``, ``cu = mean (cu_s - cxu_sᵀ δx - cuu_s δu)``,
    ``c0 = mean (c_s - cx_s·δx - cu_s·δu + ½ [δx; δu]ᵀ H_s [δx; δu])``.  Returns ``(cx[n,N(,B)], cu[m,N(,B)], cxx[n,n,N(,B)],
    cxu[n,m,N(,B)], cuu[m,m,N(,B)], c0[N(,B)])`` — the first five are what ``kl.iLQGkl(..., cost_model=...)`` takes; they are
    time-varying also with ``const_hessian``.  With ``terminal`` the last step holds the terminal cost as ``derivatives`` does.  Two calls
    give the same bits, and a call on some of the trajectories gives the bits of their slice of the full call; a non-finite sample makes
    the outputs of its own step and trajectory non-finite and touches nothing else."""
    if not isinstance(problem, DeviceProblem):
        raise TypeError("fit_cost: a DeviceProblem is needed")
    if not problem.cost_fit:
        raise DDPError("fit_cost: a DeviceProblem made with cost_fit=True (DDP_USER_COST_FIT) is needed")
    xs, us, x, u = _lib.f64(xs), _lib.f64(us), _lib.f64(x), _lib.f64(u)
    if xs.ndim not in (3, 4) or us.ndim != xs.ndim:
        raise DDPError("fit_cost: xs, us should be (n, N, S), (m, N, S) [+ batch axis], got %s, %s" % (xs.shape, us.shape))
    batched = xs.ndim == 4
    if x.ndim != xs.ndim - 1 or u.ndim != xs.ndim - 1:
        raise DDPError("fit_cost: x, u should be (n, N), (m, N)%s, got %s, %s" % (" + (B,)" if batched else "", x.shape, u.shape))
    if not batched:
        xs, us, x, u = (_lib.f64(a[..., None]) for a in (xs, us, x, u))
    n, N, S, B = xs.shape
    m = us.shape[0]
    _user_shapes(problem, n, m)
    if us.shape[1:] != (N, S, B):
        raise DDPError("fit_cost: us (m, %s) does not match xs (n, %s) in N, S [, B]" % (us.shape[1:], xs.shape[1:]))
    if x.shape != (n, N, B) or u.shape != (m, N, B):
        raise DDPError("fit_cost: x, u should be (n, N), (m, N) = (%d, %d), (%d, %d)%s, got %s, %s"
                       % (n, N, m, N, " + (B = %d,)" % B if batched else "", x.shape if batched else x.shape[:-1],
                          u.shape if batched else u.shape[:-1]))
    if S < 1:
        raise DDPError("fit_cost: S = %d (>= 1)" % S)
    P, pb = problem._params(B, params)
    h = handle or default_handle()                         # (behind the checks that need no device)
    cx = _lib.result_array((n, N, B)); cu = _lib.result_array((m, N, B)); cxx = _lib.result_array((n, n, N, B))
    cxu = _lib.result_array((n, m, N, B)); cuu = _lib.result_array((m, m, N, B)); c0 = _lib.result_array((N, B))
    _lib.check(_lib.lib().ddp_user_cost_fit_f64(h.raw, problem._ptr(h), N, S, B, _lib.ptr(P), pb, *map(_lib.ptr, (xs, us, x, u)),
                                                *map(_lib.ptr, (cx, cu, cxx, cxu, cuu, c0))))
    out = (cx, cu, cxx, cxu, cuu, c0)
    return out if batched else tuple(a[..., 0] for a in out)


# ------------------------------------------------------------------------------ expected_cost
def expected_cost(traj, x0, x, u, model, cost_model, *, Sigma0=None, moments=False, handle=None):
    """Moments and expected cost of the linear-Gaussian policy ``traj`` (``K[m,n,N(,B)]``, ``Σ[m,m,N(,B)]``; ``Σ=None``: deterministic)
    around the nominal ``x[n,N(,B)]``, ``u[m,N(,B)]`` under ``model = (fx, fu, fc, cov)`` — the first four results of ``fit_dynamics``
    as they are, ``cov=None``: zeros — and ``cost_model = (cx, cu, cxx, cxu, cuu, c0)``, the six results of ``fit_cost``: the step
    that closes a guided-policy-search round (``kl.kl_step_adjust`` takes three of its results).  The policy is the one
    ``sample_policy`` runs, ``û_i = u_i + K_i (x̂_i − x_i) + L_i ξ``; with ``G = [fx fu]``, ``H = [[cxx, cxu], [cxuᵀ, cuu]]``::

        μx_0 = x0 (None: x[:, 0]),  Sx_0 = Sigma0 (None: 0)
        δx_i = μx_i − x_i,  δu_i = K_i δx_i,  δz_i = [δx_i; δu_i],  Σz_i = [[Sx_i, Sx_i K_iᵀ], [K_i Sx_i, K_i Sx_i K_iᵀ + Σ_i]]
        ec_i = c0_i + cx_i·δx_i + cu_i·δu_i + ½ δz_iᵀ H_i δz_i + ½ tr(H_i Σz_i)
        μx_{i+1} = fx_i μx_i + fu_i (u_i + δu_i) + fc_i,  Sx_{i+1} = G_i Σz_i G_iᵀ + cov_i

    Plain subtraction for ``δx`` (no ``diff`` wrap: the function takes arrays and no problem); ``lims`` play no part; slot ``N−1`` of
    the dynamics tables is not used.  ``model`` and ``cost_model`` may each carry the batch axis or, with a batched policy, be shared
    by the batch (``[..., N]``).  ``cxx``, ``cuu``, ``cov``, ``Σ`` and ``Sigma0[n,n(,B)]`` are taken as symmetric; the result on input
    that is not is undefined.  Returns ``(ec[N(,B)], status[(B)])`` and, with ``moments=True``, ``mu[n+m,N(,B)]`` holding
    ``[μx_i; u_i + δu_i]`` and ``sigma[n+m,n+m,N(,B)]`` holding ``Σz_i`` in the layout of ``kl.forward_covariance``, symmetric to the
    bit and filled at every step.  ``status`` is 0, or ``i + 1`` for the first step whose ``ec`` is not finite: from that step on the
    trajectory's outputs are NaN (also when the value that was not finite, a ``c0_i`` say, does not enter the chain of moments), and
    no other trajectory is touched.  1 <= n <= 32, 1 <= m <= 8.  Two calls give the same bits, and a call on some of the trajectories
    gives the bits of their slice of the full call."""
    x, u, K = _lib.f64(x), _lib.f64(u), _lib.f64(traj.K)
    if x.ndim not in (2, 3) or u.ndim != x.ndim:
        raise DDPError("expected_cost: x, u should be (n, N), (m, N) [+ batch axis], got %s, %s" % (x.shape, u.shape))
    batched = x.ndim == 3
    if not batched:
        x, u = _lib.f64(x[..., None]), _lib.f64(u[..., None])
    n, N, B = x.shape
    m = u.shape[0]
    tb = (B,) if batched else ()
    if not (1 <= n <= 32 and 1 <= m <= 8):
        raise DDPError("expected_cost: n = %d, m = %d out of the box 1 <= n <= 32, 1 <= m <= 8" % (n, m))
    if N < 1 or u.shape[1:] != (N, B):
        raise DDPError("expected_cost: u (m, %s) does not match x (n, %s) in N [, B]" % (u.shape[1:], x.shape[1:]))
    if K.shape != (m, n, N) + tb:
        raise DDPError("expected_cost: traj.K should be (m,n,N) = (%d,%d,%d)%s, got %s" % (m, n, N, " + (B = %d,)" % B if batched else "", K.shape))
    Sg = getattr(traj, "Σ", None)
    Sg = None if Sg is None or np.size(Sg) == 0 else _lib.f64(Sg)
    if Sg is not None and Sg.shape != (m, m, N) + tb:
        raise DDPError("expected_cost: traj.Σ should be (m,m,N) [+ batch axis] or None, got %s" % (Sg.shape,))
    if x0 is not None:
        x0 = _lib.f64(x0)
        if x0.shape != (n,) + tb and not (not batched and x0.shape == (n, 1)):
            raise DDPError("expected_cost: x0 should be (n,) — (n, B) with a batched x — or None, got %s" % (x0.shape,))
    if Sigma0 is not None:
        Sigma0 = _lib.f64(Sigma0)
        if Sigma0.shape == (n, n) and batched:
            Sigma0 = _lib.f64(np.repeat(Sigma0[:, :, None], B, 2))
        if Sigma0.shape != (n, n) + tb:
            raise DDPError("expected_cost: Sigma0 should be (n, n) [+ batch axis] or None, got %s" % (Sigma0.shape,))
        if not np.all(np.isfinite(Sigma0)):
            raise DDPError("expected_cost: Sigma0 is not finite")

    def tables(name, tabs, want, optional):
        """the arrays of one model as the library takes them, and whether they carry the batch axis"""
        tabs = [None if a is None else _lib.f64(a) for a in tabs]
        for a, w, nm in zip(tabs, want, name):
            if a is None and nm not in optional:
                raise DDPError("expected_cost: %s is None" % nm)
        nd = tabs[0].ndim - len(want[0])
        own = batched and nd == 1
        for a, w, nm in zip(tabs, want, name):
            if a is not None and a.shape != w + ((B,) if own else ()):
                raise DDPError("expected_cost: %s should be %s%s, got %s" % (nm, w, " [+ (B = %d,)]" % B if batched else "", a.shape))
        return tabs, own

    try:
        fx, fu, fc, cov = model
    except (TypeError, ValueError):
        raise DDPError("expected_cost: model should be four arrays (fx, fu, fc, cov), e.g. fit_dynamics(...)[:4]")
    try:
        cx, cu, cxx, cxu, cuu, c0 = cost_model
    except (TypeError, ValueError):
        raise DDPError("expected_cost: cost_model should be six arrays (cx, cu, cxx, cxu, cuu, c0), the results of fit_cost")
    (fx, fu, fc, cov), mb = tables(("fx", "fu", "fc", "cov"), (fx, fu, fc, cov), ((n, n, N), (n, m, N), (n, N), (n, n, N)), ("cov",))
    (cx, cu, cxx, cxu, cuu, c0), cb = tables(("cx", "cu", "cxx", "cxu", "cuu", "c0"), (cx, cu, cxx, cxu, cuu, c0),
                                             ((n, N), (m, N), (n, n, N), (n, m, N), (m, m, N), (N,)), ())
    h = handle or default_handle()                         # (behind the checks that need no device)
    p = n + m
    ec = _lib.result_array((N, B)); status = np.zeros(B, dtype=np.int32)
    mu = _lib.result_array((p, N, B)) if moments else None
    sigma = _lib.result_array((p, p, N, B)) if moments else None
    _lib.check(_lib.lib().ddp_expected_cost_f64(h.raw, n, m, N, B, *map(_lib.ptr, (K, Sg, x0, x, u, fx, fu, fc, cov)), int(mb),
                                                *map(_lib.ptr, (cx, cu, cxx, cxu, cuu, c0)), int(cb), _lib.ptr(Sigma0), _lib.ptr(ec),
                                                status.ctypes.data_as(_lib.vp), _lib.ptr(mu), _lib.ptr(sigma)))
    out = (ec, status) + ((mu, sigma) if moments else ())
    if not batched:
        return (ec[..., 0], int(status[0])) + ((mu[..., 0], sigma[..., 0]) if moments else ())
    return out


# ------------------------------------------------------------------------------ fit_gmm, gmm_prior
@dataclass
class GMM:
    """A Gaussian mixture over the transition tuples ``w = [x̂_i; û_i; x̂_{i+1}]`` (``p = 2n + m``), as ``fit_gmm`` returns it:
    ``pi[K,G]``, ``mu[p,K,G]``, ``Sigma[p,p,K,G]``, ``ll[iters,G]``, ``status[G]``; ``G = 1`` with ``pool=True``, else one mixture per
    trajectory."""
    pi: np.ndarray
    mu: np.ndarray
    Sigma: np.ndarray
    ll: np.ndarray
    status: np.ndarray
    pool: bool = True


def _gmm_points(who, xs, us):
    xs, us = _lib.f64(xs), _lib.f64(us)
    if xs.ndim not in (3, 4) or us.ndim != xs.ndim:
        raise DDPError("%s: xs, us should be (n, N, S), (m, N, S) [+ batch axis], got %s, %s" % (who, xs.shape, us.shape))
    batched = xs.ndim == 4
    if not batched:
        xs, us = xs[..., None], us[..., None]
    if us.shape[1:] != xs.shape[1:]:
        raise DDPError("%s: us (m, %s) does not match xs (n, %s) in N, S [, B]" % (who, us.shape[1:], xs.shape[1:]))
    return xs, us, batched


def _gmm_mixture(who, pi, mu, Sigma, p, K, G):
    pi, mu, Sigma = _lib.f64(pi), _lib.f64(mu), _lib.f64(Sigma)
    if G == 1 and pi.ndim == 1:
        pi, mu, Sigma = pi[..., None], mu[..., None], Sigma[..., None]
    if pi.shape != (K, G) or mu.shape != (p, K, G) or Sigma.shape != (p, p, K, G):
        raise DDPError("%s: π, μ, Σ should be (K, G), (p, K, G), (p, p, K, G) with p = 2n + m = %d, K = %d, G = %d, got %s, %s, %s"
                       % (who, p, K, G, pi.shape, mu.shape, Sigma.shape))
    return _lib.f64(pi), _lib.f64(mu), _lib.f64(Sigma)


def fit_gmm(xs, us, K, *, iters=20, reg=1e-6, seed=0, init=None, pool=True, traj0=0, handle=None):
    """A ``K``-cluster Gaussian mixture fitted by EM on the device to the transition tuples ``w = [x̂_i; û_i; x̂_{i+1}]`` of all steps and
    samples of the rollouts ``xs[n,N,S(,B)]``, ``us[m,N,S(,B)]`` that ``sample_policy`` returns — the dynamics prior of the
    guided-policy-search round (Levine & Abbeel 2014; the formulas are in include/ddp_amd.h).  ``pool=True``: one mixture over all
    trajectories; ``False``: one per trajectory.  ``init=(π, μ, Σ)`` or a ``GMM`` (the mixture of the last round) is the start; without
    it an M-step from a hard assignment drawn from ``seed`` (Philox counter ``(i, s, traj0 + b, 0x80000000)``: not the sampler's
    stream).  ``reg >= 0`` is added to the diagonal of every ``Σ_k``.  Returns a ``GMM``; ``status[g]`` is 0, or ``k + 1`` for the first
    cluster that emptied or whose ``Σ_k`` is not positive definite (that mixture is NaN).  1 <= n <= 32, 1 <= m <= 8, 1 <= K <= 32.
    Two calls give the same bits; with ``pool=False`` a call on some of the trajectories (with its ``traj0``) gives their slice."""
    xs, us, _ = _gmm_points("fit_gmm", xs, us)
    n, N, S, B = xs.shape
    m, p, K, iters, pool = us.shape[0], 2 * n + us.shape[0], int(K), int(iters), bool(pool)
    G = 1 if pool else B
    if not 1 <= K <= 32 or iters < 0:
        raise DDPError("fit_gmm: K = %d out of [1, 32] or iters = %d < 0" % (K, iters))
    pi0 = mu0 = Sg0 = None
    if init is not None:
        if isinstance(init, GMM):
            init = (init.pi, init.mu, init.Sigma)
        pi0, mu0, Sg0 = _gmm_mixture("fit_gmm: init", *init, p, K, G)
    lo, hi = _seed_words(seed)
    h = handle or default_handle()
    pi = np.zeros((K, G), order="F"); mu = np.zeros((p, K, G), order="F"); Sigma = _lib.result_array((p, p, K, G))
    ll = np.zeros((iters, G), order="F"); status = np.zeros(G, dtype=np.int32)
    _lib.check(_lib.lib().ddp_gmm_fit_f64(h.raw, n, m, N, S, B, K, iters, int(pool), int(traj0), _lib.ptr(xs), _lib.ptr(us), float(reg), lo, hi,
                                          _lib.ptr(pi0), _lib.ptr(mu0), _lib.ptr(Sg0), _lib.ptr(pi), _lib.ptr(mu), _lib.ptr(Sigma),
                                          _lib.ptr(ll) if iters > 0 else None, status.ctypes.data_as(_lib.vp)))
    return GMM(pi, mu, Sigma, ll, status, pool)


def gmm_prior(gmm, xs, us, *, m0=1.0, n0=1.0, handle=None):
    """The normal-inverse-Wishart prior of every step from a mixture of ``fit_gmm``: with ``r_sk`` the responsibilities of the step's
    ``S`` points, ``ω_k = mean_s r_sk``, ``μ0 = Σ_k ω_k μ_k``, ``Φ = n0 Σ_k ω_k (Σ_k + (μ_k - μ0)(μ_k - μ0)ᵀ)``.  Returns
    ``(Φ[p,p,N(,B)], μ0[p,N(,B)], m0, n0)``, which ``fit_dynamics(xs, us, prior=...)`` takes as it is:

        gmm = fit_gmm(xs, us, K)
        fx, fu, fc, cov, status = fit_dynamics(xs, us, prior=gmm_prior(gmm, xs, us))

    A step with a point that is not finite, or a mixture that is not usable (``gmm.status != 0``), gives NaN in that step's ``Φ``,
    ``μ0``, which ``fit_dynamics`` reports in its status.  Slot ``N-1`` has no transition: zeros."""
    if not isinstance(gmm, GMM):
        raise DDPError("gmm_prior: a GMM (the result of fit_gmm) is needed")
    xs, us, batched = _gmm_points("gmm_prior", xs, us)
    n, N, S, B = xs.shape
    m = us.shape[0]
    p, K, pool = 2 * n + m, int(np.shape(gmm.pi)[0]) if np.ndim(gmm.pi) else 0, bool(gmm.pool)
    pi, mu, Sigma = _gmm_mixture("gmm_prior", gmm.pi, gmm.mu, gmm.Sigma, p, K, 1 if pool else B)
    h = handle or default_handle()
    Phi = _lib.result_array((p, p, N, B)); mu0 = _lib.result_array((p, N, B)); status = np.zeros((N, B), dtype=np.int32, order="F")
    _lib.check(_lib.lib().ddp_gmm_prior_f64(h.raw, n, m, N, S, B, K, int(pool), _lib.ptr(xs), _lib.ptr(us), _lib.ptr(pi), _lib.ptr(mu),
                                            _lib.ptr(Sigma), float(m0), float(n0), _lib.ptr(Phi), _lib.ptr(mu0),
                                            status.ctypes.data_as(_lib.vp)))
    if not batched:
        return Phi[..., 0], mu0[..., 0], float(m0), float(n0)
    return Phi, mu0, float(m0), float(n0)


# ---------------------------------------------------------------------------------------- iLQG
def print_timing(trace):
    """The timing summary of iLQG.jl:343-366 from the trace keys ``time_derivs``, ``time_backward``, ``time_forward``."""
    if "time_derivs" not in trace:
        raise KeyError("print_timing needs the time_* keys: call iLQG(..., timing=True)")
    parts = [float(np.nansum(trace[k])) for k in ("time_derivs", "time_backward", "time_forward")]
    total = float(trace.get("time_total", sum(parts)))
    it = max(int(trace.get("global_iters", 1)), 1)
    pct = [100.0 * t / total for t in parts] + [100.0 * (total - sum(parts)) / total]
    print("\n iterations:   %-3d\n time / iter:  %-5.2f ms\n total time:   %-5.3f seconds, of which\n derivs:     %-4.1f%%\n"
          " back pass:  %-4.1f%%\n fwd pass:   %-4.1f%%\n other:      %-4.1f%% (host, transfers)\n =========== end iLQG ==========="
          % (it, 1e3 * total / it, total, pct[0], pct[1], pct[2], pct[3]))


STATUS = {1: "SUCCESS: gradient norm < tol_grad", 2: "SUCCESS: cost change < tol_fun", 3: "EXIT: λ > λmax",
          4: "EXIT: Maximum iterations reached", -1: "EXIT: Initial control sequence caused divergence",
          5: "EXIT: the driver's bound on batch iterations ran out (not a state of the reference)"}


def iLQG(problem, x0, u0, *, lims=None, α=DEFAULT_ALPHA, tol_fun=1e-7, tol_grad=1e-4, max_iter=500, λ=1.0, dλ=1.0,
         λfactor=1.6, λmax=1e10, λmin=1e-6, regType=1, reduce_ratio_min=0.0, verbosity=0, trace_cap=None, cost=None,
         timing=True, diff_fun=None, handle=None, params=None, t0=None, multipliers=None):
    """Drop-in for ``iLQG(f,costfun,df,x0,u0; lims, α, tol_fun, ...)`` (iLQG.jl:143-163) with a registered
    ``problem`` standing in for the three closures (``diff_fun``: ``None`` = ``-``, or a ``WrappedDiff``).  ``u0[m,N,B]`` / ``x0[n,B]`` solve a batch of
    independent problems, each with its own λ schedule, line search and termination.
    Returns ``(x, u, traj_new, Vx, Vxx, cost, trace)``; ``trace`` is a dict with the reference's trace
    keys that survive batching (``:cost`` per iteration) plus the per-trajectory summary ``stats``.
    ``x0[n,N]`` (``x0[n,N,B]`` with a batch) is a PRE-ROLLED initial trajectory (iLQG.jl:193-197: no initial rollout;
    ``cost`` as given or ``costfun(x0,u0)``) — the warm start of an MPC loop.
    ``timing=False`` drops the ``time_*`` trace keys: the driver then synchronises with the host every fourth batch iteration only.
    ``trace_cap``: rows of the per-iteration history kept per trajectory; the default shrinks with the batch,
    ``min(4 max_iter + 64, 4096, max(64, 256e6 / (56 B)))`` (136 rows at B = 32768), so that ``history[7, cap, B]`` stays under 256 MB.
    ``trace["trace_cap"]`` is the cap used and ``trace["truncated"]`` says, per trajectory, whether it took more iterations than rows
    were kept (its later rows are missing, ``stats`` / ``iter`` are complete).
    Returns ``None`` when the initial control sequence diverges (iLQG.jl:205-210) in the unbatched case.
    A ``DeviceProblem`` (the user's own closures as device source) takes ``params`` (default: its own); its ``diff`` is compiled in;
    made with ``clock=True`` it takes ``t0``, the clock of every trajectory (an int or B ints; default 0); made with
    ``constraints=nc`` it takes ``multipliers=(λ, μ)`` and then minimises the augmented cost (``iLQG_al`` is the whole loop)."""
    h = handle or default_handle()
    user = isinstance(problem, DeviceProblem)
    if not user:
        _no_multipliers(multipliers)
    if user:
        if np.ndim(u0) not in (2, 3):
            raise DDPError("u0 should be (m, N) or (m, N, B)")
        _user_shapes(problem, np.shape(x0)[0], np.shape(u0)[0])
    u0, x0 = _lib.f64(u0), _lib.f64(x0)
    batched = u0.ndim == 3
    m, N = u0.shape[:2]
    n = x0.shape[0]
    B = u0.shape[2] if batched else 1
    prerolled = False
    if x0.ndim == (3 if batched else 2):                      # x0 has a time axis: single column or pre-rolled (iLQG.jl:181,193)
        if x0.shape[1] == N:
            prerolled = True
        elif x0.shape[1] == 1:
            x0 = _lib.f64(x0[:, 0])
        else:
            raise ValueError("pre-rolled initial trajectory must be of correct length (size(x0,2) == N)")     # iLQG.jl:199
    if x0.shape != (((n, N) if prerolled else (n,)) + ((B,) if batched else ())):
        raise ValueError("x0 should be (n,) / pre-rolled (n, N) — with a batched u0: (n, B) / (n, N, B)")
    if user:
        P, pb = problem._params(B, params)
        if diff_fun is not None and _diff_mask(diff_fun, n) != problem.diff_mask:
            raise DDPError("DeviceProblem: diff_fun is compiled into the problem (DeviceProblem(..., diff=...))")
        CL = problem.cost_len(N)
    else:
        _check_problem(problem, n, m, N, B)
        dp = _DevProblem(problem, N, B, diff_fun)
        CL = dp.cost_len
    o = _lib.ILQGOpts()
    _lib.lib().ddp_ilqg_default_opts(_C.byref(o))
    o.lambda_, o.dlambda, o.lambda_factor, o.lambda_max, o.lambda_min = λ, dλ, λfactor, λmax, λmin
    o.tol_fun, o.tol_grad, o.max_iter, o.regType, o.reduce_ratio_min = tol_fun, tol_grad, max_iter, regType, reduce_ratio_min
    alphas = np.asarray(α, dtype=np.float64)
    if len(alphas) > 16:
        raise ValueError("at most 16 line-search step sizes are supported")
    o.n_alpha = len(alphas)
    for i, a in enumerate(alphas):
        o.alpha[i] = a
    L = _lims(lims)
    if user and L is not None and L.shape != (m, 2):
        raise DDPError("lims should be (m, 2)")
    x = _lib.result_array((n, N, B)); u = _lib.result_array((m, N, B))
    K = _lib.result_array((m, n, N, B)); k = _lib.result_array((m, N, B)); Quu = _lib.result_array((m, m, N, B))
    Vx = _lib.result_array((n, N, B)); Vxx = _lib.result_array((n, n, N, B))
    stats = np.zeros((8, B), order="F")
    # rows of the per-iteration trace kept per trajectory; by default bounded so that trace7[7, cap, B] stays under 256 MB
    # (a batch of 4096 pendcart solves with cap = 4 max_iter + 64 moved 0.93 GB of mostly zeros)
    cap = trace_cap if trace_cap is not None else min(4 * max_iter + 64, 4096, max(64, int(256e6 / (56 * B))))
    cap = min(cap, 4096)
    git = _C.c_int(0)
    c0 = None if (not prerolled or cost is None or np.size(cost) == 0) else _lib.f64(np.reshape(cost, (CL, B), order="F"))
    cost = _lib.result_array((CL, B))
    tr7 = _lib.result_array((7, cap, B))
    tcap = 4 * max_iter + 1000                                 # the driver's bound on global iterations
    timing_on = bool(timing)
    timing = np.full((3, tcap), np.nan)
    t_start = _time.time()
    _lib.check(_lib.lib().ddp_ilqg_set_timing(h.raw, _lib.ptr(timing) if timing_on else None, tcap if timing_on else 0))
    try:
        if user:
            with problem._clock(h, t0), problem._multipliers(h, multipliers, N, B, batched):
                _lib.check(_lib.lib().ddp_user_ilqg_f64(h.raw, problem._ptr(h), N, B, _lib.ptr(P), pb, _C.byref(o), _lib.ptr(x0), int(prerolled),
                                                        _lib.ptr(u0), _lib.ptr(c0), _lib.ptr(L),
                                                        *map(_lib.ptr, (x, u, K, k, Quu, Vx, Vxx, cost, stats)), cap, _lib.ptr(tr7), _C.byref(git)))
        else:
            _no_clock(t0)
            _lib.check(_lib.lib().ddp_ilqg_ex_f64(h.raw, _C.byref(dp.struct), _C.byref(o), _lib.ptr(x0), int(prerolled), _lib.ptr(u0),
                                                  _lib.ptr(c0), _lib.ptr(L), *map(_lib.ptr, (x, u, K, k, Quu, Vx, Vxx, cost, stats)), cap,
                                                  _lib.ptr(tr7), _C.byref(git)))
    finally:
        _lib.lib().ddp_ilqg_set_timing(h.raw, None, 0)
    total_t = _time.time() - t_start
    tr = tr7[4]
    # the reference's trace keys (iLQG.jl:257,325-330), one row per iteration: trace["history"][key][iteration-1(, b)]
    hist = {key: tr7[c] for c, key in enumerate(("λ", "dλ", "α", "improvement", "cost", "reduce_ratio", "grad_norm"))}
    trace = dict(stats=stats, status=stats[0].astype(int), iter=stats[1].astype(int), λ=stats[5], grad_norm=stats[6],
                 cost=tr, global_iters=git.value, history=hist, trace_cap=cap, truncated=(stats[1] - 1 > cap))
    if trace["truncated"].any():
        import warnings
        warnings.warn("iLQG: %d of %d trajectories took more iterations than the %d history rows kept (trace_cap); their later rows are "
                      "missing from trace['history'] / trace['cost']" % (int(trace["truncated"].sum()), B, cap))
    # time_derivs / time_backward / time_forward (iLQG.jl:227,241,281): GPU seconds per GLOBAL iteration of the batch
    for r, key in enumerate(("time_derivs", "time_backward", "time_forward")):
        if timing_on:
            trace[key] = timing[r, : git.value].copy()
    trace["time_total"] = total_t
    if verbosity > 0:
        for b in range(min(B, 8)):
            print("[%d] %s after %d iterations, cost %.6g" % (b, STATUS.get(int(stats[0, b]), "?"), int(stats[1, b]), stats[7, b]))
        if timing_on:
            print_timing(trace)
    if not batched:
        if int(stats[0, 0]) == -1:
            return None
        it = int(stats[1, 0])
        trace["cost"] = tr[: max(it - 1, 0), 0]
        trace["history"] = {key: v[: max(it - 1, 0), 0] for key, v in hist.items()}
        pol = GaussianPolicy(N, n, m, K[..., 0], k[..., 0], np.zeros((m, m, N)), Quu[..., 0])
        return x[..., 0], u[..., 0], pol, Vx[..., 0], Vxx[..., 0], cost[:, 0], trace
    pol = GaussianPolicy(N, n, m, K, k, np.zeros((m, m, N, B)), Quu)
    return x, u, pol, Vx, Vxx, cost, trace


AL_STATUS = {1: "SUCCESS: constraint violation <= ctol", 2: "EXIT: max_outer rounds", -1: "EXIT: Initial control sequence caused divergence"}


def iLQG_al(problem, x0, u0, *, mu0=1.0, mu_factor=10.0, mu_max=1e8, ctol=1e-5, max_outer=20, multipliers=None, lims=None,
            α=DEFAULT_ALPHA, tol_fun=1e-7, tol_grad=1e-4, max_iter=500, λ=1.0, dλ=1.0, λfactor=1.6, λmax=1e10, λmin=1e-6, regType=1,
            reduce_ratio_min=0.0, handle=None, params=None):
    """The constrained solve of a ``DeviceProblem`` made with ``constraints=nc``: an augmented-Lagrangian loop around ``iLQG``, on the
    device (ddp_user_ilqg_al_f64).  Per trajectory and round: the ``iLQG`` solve under the multipliers ``(λ, μ)`` (round 0 from
    ``x0``, ``u0`` — ``x0`` may be pre-rolled as in ``iLQG`` —, later rounds from the last solution), ``cviol = max(0, g).max()``, then
    either the end (``cviol <= ctol``: status 1; ``max_outer`` rounds: 2; diverged at the start: -1) or ``λ ← max(0, λ + μ g)``,
    ``μ ← min(mu_factor μ, mu_max)``.  ``multipliers=(λ0, μ0)``: the initial ones (default zeros and ``mu0``).  The other keywords are
    ``iLQG``'s.  Returns ``iLQG``'s tuple ``(x, u, traj_new, Vx, Vxx, cost, info)``; ``cost`` is the augmented one and ``info`` holds
    ``λ``, ``μ``, ``g`` at the returned trajectory, ``al_stats`` and its columns ``status``, ``rounds``, ``inner_iters``, ``mu_last``,
    ``cviol``, ``raw_cost``, the inner ``stats`` of the last round each trajectory ran, and ``global_iters``."""
    if not isinstance(problem, DeviceProblem) or not problem.nc:
        raise DDPError("iLQG_al: a DeviceProblem made with constraints=nc (DDP_USER_CONSTRAINTS) is needed")
    h = handle or default_handle()
    if np.ndim(u0) not in (2, 3):
        raise DDPError("u0 should be (m, N) or (m, N, B)")
    _user_shapes(problem, np.shape(x0)[0], np.shape(u0)[0])
    u0, x0 = _lib.f64(u0), _lib.f64(x0)
    batched = u0.ndim == 3
    m, N = u0.shape[:2]
    n = x0.shape[0]
    B = u0.shape[2] if batched else 1
    prerolled = x0.ndim == (3 if batched else 2)
    if x0.shape != (((n, N) if prerolled else (n,)) + ((B,) if batched else ())):
        raise ValueError("x0 should be (n,) / pre-rolled (n, N) — with a batched u0: (n, B) / (n, N, B)")
    P, pb = problem._params(B, params)
    L = _lims(lims)
    if L is not None and L.shape != (m, 2):
        raise DDPError("lims should be (m, 2)")
    lam0 = mu_init = None
    if multipliers is not None:
        lam0, mu_init = problem._multiplier_arrays(multipliers, N, B, batched)
    if not (mu0 > 0 and mu_factor >= 1 and mu_max >= mu0 and ctol >= 0 and int(max_outer) >= 1):
        raise DDPError("iLQG_al: mu0 > 0, mu_factor >= 1, mu_max >= mu0, ctol >= 0 and max_outer >= 1 are needed")
    o = _ilqg_opts(α, tol_fun, tol_grad, max_iter, λ, dλ, λfactor, λmax, λmin, regType, reduce_ratio_min)
    ao = _lib.ALOpts(float(mu0), float(mu_factor), float(mu_max), float(ctol), int(max_outer))
    nc, CL = problem.nc, problem.cost_len(N)
    x = _lib.result_array((n, N, B)); u = _lib.result_array((m, N, B))
    K = _lib.result_array((m, n, N, B)); k = _lib.result_array((m, N, B)); Quu = _lib.result_array((m, m, N, B))
    Vx = _lib.result_array((n, N, B)); Vxx = _lib.result_array((n, n, N, B)); cost = _lib.result_array((CL, B))
    stats = np.zeros((8, B), order="F"); al_stats = np.zeros((6, B), order="F")
    lam = _lib.result_array((nc, N, B)); mu = np.zeros(B); g = _lib.result_array((nc, N, B))
    git = _C.c_int(0)
    _lib.check(_lib.lib().ddp_user_ilqg_al_f64(h.raw, problem._ptr(h), N, B, _lib.ptr(P), pb, _C.byref(o), _C.byref(ao), _lib.ptr(x0),
                                               int(prerolled), _lib.ptr(u0), _lib.ptr(L), _lib.ptr(lam0), _lib.ptr(mu_init),
                                               *map(_lib.ptr, (x, u, K, k, Quu, Vx, Vxx, cost, stats, lam, mu, g, al_stats)), _C.byref(git)))
    info = dict(λ=lam, μ=mu, g=g, al_stats=al_stats, status=al_stats[0].astype(int), rounds=al_stats[1].astype(int),
                inner_iters=al_stats[2].astype(int), mu_last=al_stats[3], cviol=al_stats[4], raw_cost=al_stats[5], stats=stats,
                global_iters=git.value)
    if not batched:
        info.update(λ=lam[..., 0], μ=mu[0], g=g[..., 0])
        pol = GaussianPolicy(N, n, m, K[..., 0], k[..., 0], np.zeros((m, m, N)), Quu[..., 0])
        return x[..., 0], u[..., 0], pol, Vx[..., 0], Vxx[..., 0], cost[:, 0], info
    pol = GaussianPolicy(N, n, m, K, k, np.zeros((m, m, N, B)), Quu)
    return x, u, pol, Vx, Vxx, cost, info


def _ilqg_opts(α, tol_fun, tol_grad, max_iter, λ, dλ, λfactor, λmax, λmin, regType, reduce_ratio_min):
    o = _lib.ILQGOpts()
    _lib.lib().ddp_ilqg_default_opts(_C.byref(o))
    o.lambda_, o.dlambda, o.lambda_factor, o.lambda_max, o.lambda_min = λ, dλ, λfactor, λmax, λmin
    o.tol_fun, o.tol_grad, o.max_iter, o.regType, o.reduce_ratio_min = tol_fun, tol_grad, max_iter, regType, reduce_ratio_min
    alphas = np.asarray(α, dtype=np.float64)
    if len(alphas) > 16:
        raise ValueError("at most 16 line-search step sizes are supported")
    o.n_alpha = len(alphas)
    for i, a in enumerate(alphas):
        o.alpha[i] = a
    return o


def _user_sched_args(problem, x0, u0, L, params, diff_fun):
    """a DeviceProblem in iLQG_queue / iLQG_mpc: extents against the compiled n, m and the parameters, before any launch"""
    (n, B), m = x0.shape, u0.shape[0]
    _user_shapes(problem, n, m)
    if u0.shape[2] != B:
        raise DDPError("x0[n,B] and u0[m,N,B] have different B: %s, %s" % (x0.shape, u0.shape))
    if L is not None and L.shape != (m, 2):
        raise DDPError("lims should be (m, 2)")
    if diff_fun is not None and _diff_mask(diff_fun, n) != problem.diff_mask:
        raise DDPError("DeviceProblem: diff_fun is compiled into the problem (DeviceProblem(..., diff=...))")
    return problem._params(B, params)


def iLQG_queue(problem, x0, u0, *, slots=0, lims=None, α=DEFAULT_ALPHA, tol_fun=1e-7, tol_grad=1e-4, max_iter=500, λ=1.0, dλ=1.0,
               λfactor=1.6, λmax=1e10, λmin=1e-6, regType=1, reduce_ratio_min=0.0, diff_fun=None, handle=None, params=None, t0=None):
    """``P = u0.shape[2]`` independent solves of ``iLQG`` through ``slots`` resident trajectories (``ddp_ilqg_queue_f64``): a slot whose
    solve has ended is flushed and armed with the next problem on the device, instead of idling until the slowest trajectory of a
    lock-step batch has ended.  Every solve is the solve ``iLQG`` performs at batch size ``slots``.
    A ``DeviceProblem`` takes ``params`` (default: its own), ``(nparam,)`` shared or ``(nparam, P)`` one column per problem; made with
    ``clock=True`` it takes ``t0``, an int or P ints: the slot that takes problem ``p`` runs with the clock ``t0[p]``.
    Returns ``(x, u, traj_new, Vx, Vxx, cost, trace)`` with P columns; ``trace`` holds ``stats[8,P]``, ``status``, ``iter``, ``global_iters``."""
    u0, x0 = _lib.f64(u0), _lib.f64(x0)
    if u0.ndim != 3 or x0.ndim != 2:
        raise ValueError("iLQG_queue: x0[n,P], u0[m,N,P]")
    m, N, P = u0.shape
    n = x0.shape[0]
    user = isinstance(problem, DeviceProblem)
    L = _lims(lims)
    if user:
        prm, pb = _user_sched_args(problem, x0, u0, L, params, diff_fun)
        CL = problem.cost_len(N)
    else:
        _check_problem(problem, n, m, N, P)
        dp = _DevProblem(problem, N, P, diff_fun)
        CL = dp.cost_len
    o = _ilqg_opts(α, tol_fun, tol_grad, max_iter, λ, dλ, λfactor, λmax, λmin, regType, reduce_ratio_min)
    x = _lib.result_array((n, N, P)); u = _lib.result_array((m, N, P))
    K = _lib.result_array((m, n, N, P)); k = _lib.result_array((m, N, P)); Quu = _lib.result_array((m, m, N, P))
    Vx = _lib.result_array((n, N, P)); Vxx = _lib.result_array((n, n, N, P)); cost = _lib.result_array((CL, P))
    stats = np.zeros((8, P), order="F")
    git = _C.c_int(0)
    h = handle or default_handle()
    t_start = _time.time()
    outs = tuple(map(_lib.ptr, (x, u, K, k, Quu, Vx, Vxx, cost, stats)))
    if user:
        with problem._clock(h, t0):
            _lib.check(_lib.lib().ddp_user_ilqg_queue_f64(h.raw, problem._ptr(h), N, P, _lib.ptr(prm), pb, _C.byref(o), int(slots), _lib.ptr(x0),
                                                          _lib.ptr(u0), _lib.ptr(L), *outs, _C.byref(git)))
    else:
        _no_clock(t0)
        _lib.check(_lib.lib().ddp_ilqg_queue_f64(h.raw, _C.byref(dp.struct), _C.byref(o), int(slots), _lib.ptr(x0), _lib.ptr(u0), _lib.ptr(L),
                                                 *outs, _C.byref(git)))
    trace = dict(stats=stats, status=stats[0].astype(int), iter=stats[1].astype(int), λ=stats[5], grad_norm=stats[6],
                 global_iters=git.value, time_total=_time.time() - t_start)
    return x, u, GaussianPolicy(N, n, m, K, k, np.zeros((m, m, N, P)), Quu), Vx, Vxx, cost, trace


def iLQG_mpc(problem, x0, u0, steps, *, zero_tail=False, lims=None, α=DEFAULT_ALPHA, tol_fun=1e-7, tol_grad=1e-4, max_iter=500, λ=1.0,
             dλ=1.0, λfactor=1.6, λmax=1e10, λmin=1e-6, regType=1, reduce_ratio_min=0.0, diff_fun=None, handle=None, params=None, t0=None):
    """Closed loop on the device (``ddp_ilqg_mpc_f64``): every trajectory of the batch is solved ``steps`` times; after each solve the
    first control is applied (model = plant: the next initial state is ``x[:,1]`` of the solution), the control sequence is shifted by
    one step (``mpc_shift``) and the problem is solved again without returning to the host.
    A ``DeviceProblem`` takes ``params`` (default: its own), ``(nparam,)`` or ``(nparam, B)`` per trajectory; built with
    ``plant=True`` its ``plant`` is the true system: ``xcl[:,t+1] = plant(xcl[:,t], ucl[:,t], t, p)`` starts the next solve.  Made with
    ``clock=True`` it takes ``t0`` (an int or B ints, default 0): the solve at closed-loop step ``s`` runs with the clock ``t0 + s``, advanced
    on the device, and ``plant`` gets the absolute ``t = t0 + s``.
    Returns ``(xcl[n,steps+1,B], ucl[m,steps,B], stats[8,steps,B], x_plan[n,N,B], u_plan[m,N,B], global_iters)``."""
    u0, x0 = _lib.f64(u0), _lib.f64(x0)
    if u0.ndim != 3 or x0.ndim != 2:
        raise ValueError("iLQG_mpc: x0[n,B], u0[m,N,B]")
    m, N, B = u0.shape
    n = x0.shape[0]
    user = isinstance(problem, DeviceProblem)
    L = _lims(lims)
    if user:
        prm, pb = _user_sched_args(problem, x0, u0, L, params, diff_fun)
    else:
        _check_problem(problem, n, m, N, B)
        dp = _DevProblem(problem, N, B, diff_fun)
    o = _ilqg_opts(α, tol_fun, tol_grad, max_iter, λ, dλ, λfactor, λmax, λmin, regType, reduce_ratio_min)
    steps = int(steps)
    xcl = np.zeros((n, steps + 1, B), order="F"); ucl = np.zeros((m, steps, B), order="F"); scl = np.zeros((8, steps, B), order="F")
    x = _lib.result_array((n, N, B)); u = _lib.result_array((m, N, B))
    git = _C.c_int(0)
    h = handle or default_handle()
    outs = tuple(map(_lib.ptr, (xcl, ucl, scl, x, u)))
    if user:
        with problem._clock(h, t0):
            _lib.check(_lib.lib().ddp_user_ilqg_mpc_f64(h.raw, problem._ptr(h), N, B, _lib.ptr(prm), pb, _C.byref(o), steps, int(bool(zero_tail)),
                                                        _lib.ptr(x0), _lib.ptr(u0), _lib.ptr(L), *outs, _C.byref(git)))
    else:
        _no_clock(t0)
        _lib.check(_lib.lib().ddp_ilqg_mpc_f64(h.raw, _C.byref(dp.struct), _C.byref(o), steps, int(bool(zero_tail)), _lib.ptr(x0), _lib.ptr(u0),
                                               _lib.ptr(L), *outs, _C.byref(git)))
    return xcl, ucl, scl, x, u, git.value


def runtime_info():
    """which HIP runtime the process ended up with and why (``_lib._share_torch_hip``), the library version, the devices it sees"""
    L = _lib.lib()
    return dict(version=L.ddp_version().decode(), devices=int(L.ddp_device_count()), hip_runtime=_lib.hip_runtime_note)
