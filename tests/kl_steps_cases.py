"""Inputs of tests/test_gpu_kl_steps.py (one kl_step per trajectory in iLQGkl), shared with the child process that runs the mixed call
under DDP_KL_HOSTLOOP=1: the smallest KL fixture shape of tests/test_gpu_kl.py, an LQProblem with n = 4, m = 2, a short horizon, B = 3.

    python tests/kl_steps_cases.py OUT.npz      runs the mixed call of `lq_case` and writes its results (the child process)"""
import numpy as np

STEPS = (2e-4, 1e-4, 4e-4)      # distinct steps for which the scalar calls end with status 1 (the test checks that first)
MAX_ITER = 40


def lq_case():
    """dict(prob arguments A, Bm, Q, R; x[n,T,B] the rollout of u[m,T,B]; cost0[B]; fx, fu, R1 of the model)"""
    import scipy.linalg as sla
    rng = np.random.default_rng(31)
    n, m, T, B, h = 4, 2, 20, 3, 0.01
    A0 = rng.standard_normal((n, n)); A = sla.expm(h * (A0 - A0.T)); Bm = h * rng.standard_normal((n, m))
    Q, R = h * np.eye(n), 0.1 * h * np.eye(m)
    u = 0.1 * rng.standard_normal((m, T, B)) * np.array([1.0, 2.0, 0.5])
    x = np.zeros((n, T, B)); x[:, 0, :] = 1.0 + 0.1 * rng.standard_normal((n, B))
    for t in range(T - 1):
        x[:, t + 1, :] = A @ x[:, t, :] + Bm @ u[:, t, :]
    cost0 = 0.5 * np.einsum("itb,ij,jtb->b", x, Q, x) + 0.5 * np.einsum("itb,ij,jtb->b", u, R, u)
    return dict(n=n, m=m, T=T, B=B, A=A, Bm=Bm, Q=Q, R=R, u=u, x=x, cost0=cost0, fx=np.repeat(A[:, :, None], T, 2), fu=np.repeat(Bm[:, :, None], T, 2),
                R1=1e-4 * np.eye(n))


def run(ddp, c, kl_step, **kw):
    """iLQGkl on the case -> (x, u, traj_new, Vx, Vxx, cost, trace)"""
    n, m, T, B = c["n"], c["m"], c["T"], c["B"]
    eye = np.repeat(np.repeat(np.eye(m)[:, :, None, None], T, 2), B, 3)
    prev = ddp.GaussianPolicy(T, n, m, np.zeros((m, n, T, B)), c["u"].copy(), eye, eye.copy())
    kw.setdefault("max_iter", MAX_ITER)
    return ddp.kl.iLQGkl(ddp.LQProblem(c["A"], c["Bm"], c["Q"], c["R"]), c["x"], prev, ddp.kl.Model(c["fx"], c["fu"], c["R1"]), kl_step=kl_step,
                         cost=c["cost0"], **kw)


def flat(out):
    """the arrays of a result by name"""
    x, u, pol, Vx, Vxx, cost, tr = out
    d = dict(x=x, u=u, K=pol.K, S=pol.Σ, Si=pol.Σi, Vx=Vx, Vxx=Vxx, cost=cost)
    d.update({"trace_" + k: np.asarray(v) for k, v in tr.items()})
    return d


if __name__ == "__main__":
    import os
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import ddp_amd
    import ddp_amd.kl  # noqa: F401
    assert os.environ.get("DDP_KL_HOSTLOOP") == "1"
    np.savez(sys.argv[1], **flat(run(ddp_amd, lq_case(), np.array(STEPS))))
