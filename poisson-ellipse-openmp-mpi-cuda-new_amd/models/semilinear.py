"""Newton's method for the semilinear problem -Δu + g(u) = f in D, u = 0 on ∂D, g monotone (g' >= 0), on the
solve with a reaction field: every step is one linear solve with c = g'(u_k)."""
from __future__ import annotations

import math

import numpy as np

from .problem import PoissonEllipse
from .solvers import make_session, solve


class SemilinearNewton:
    """Step k solves L_k u_{k+1} = f - g(u_k) + g'(u_k) u_k from w0 = u_k, L_k = A + (σ + g'(u_k)) I: the solve
    with reaction = g'(u_k) (make_session / solve()).  The nonlinear residual of u_k is the linear residual of
    that system AT u_k, rhs_k - L_k u_k = f - g(u_k) - (A + σ) u_k under the ellipse mask, so it is measured
    before the step's solve (h-weighted 2-norm, Session.residual_norm) and kept in `history`.  The iteration
    stops at the first k with history[k] <= newton_rtol history[0], or after max_newton steps.

    g, dg: callables on the iterate's type, returning the same type and shape; dg >= 0 (the solver checks).

    backend "hip" keeps ONE native session (session_kw as make_session; ranks = 1, residual_norm's limit): each
    step replaces its reaction field in place (Session.set_reaction) and solves; with f (and u0) float64 tensors
    on the session's device nothing passes through the host, and the result is a device tensor.  NumPy arrays
    in give a NumPy array out.  Every other backend of solve() runs NumPy end to end.  All fields are
    (M+1) x (N+1) float64.

    The linear solves stop by the problem's rule: pick stop="residual" with an rtol below newton_rtol (and
    breakdown_tol=0 with tight tolerances), or the Newton residual stalls at the accuracy of the inner solve.

    After solve(): `history` (residuals, one per step taken plus the final one), `steps` (linear solves),
    `converged`, `last` (statistics of the last linear solve).

    domain=phi in session_kw (solve()'s level-set field) poses the problem on D = {phi < 0}: the solves and the
    residual's mask take it."""

    def __init__(self, problem: PoissonEllipse, g, dg, backend: str = "hip", newton_rtol: float = 1e-8,
                 max_newton: int = 20, **session_kw):
        if not (isinstance(newton_rtol, (int, float)) and math.isfinite(newton_rtol) and newton_rtol >= 0):
            raise ValueError(f"newton_rtol must be a finite number >= 0, got {newton_rtol!r}")
        if not (isinstance(max_newton, int) and max_newton >= 1):
            raise ValueError(f"max_newton must be an integer >= 1, got {max_newton!r}")
        if "reaction" in session_kw:
            raise ValueError("SemilinearNewton sets the reaction field itself (g'(u_k)); add a fixed part to g")
        self.problem = problem
        self.g, self.dg = g, dg
        self.backend = backend
        self.newton_rtol = float(newton_rtol)
        self.max_newton = max_newton
        self.kw = session_kw
        self.session = None  # hip: built by the first solve (it needs a field to start from)
        self.history, self.steps, self.converged, self.last = [], 0, False, None

    def _residual_host(self, u, rhs, c) -> float:
        p = self.problem
        phi = self.kw.get("domain")
        e = np.where(p.inside_mask(phi), rhs, 0.0) - p.apply(u, reaction=c, domain=phi)
        e[0, :] = e[-1, :] = 0.0
        e[:, 0] = e[:, -1] = 0.0
        return math.sqrt(float((e * e).sum()) * p.h1 * p.h2)

    def solve(self, f, u0=None):
        """f: the right-hand side (masked to the ellipse by the solver); u0: the start (default 0)."""
        hip = self.backend == "hip"
        on_device = hasattr(f, "__cuda_array_interface__")
        if on_device and not hip:
            raise ValueError(f"backend {self.backend!r} takes NumPy arrays; device tensors need backend='hip'")
        u = f * 0.0 if u0 is None else u0
        self.history, self.steps, self.converged, self.last = [], 0, False, None
        while True:
            c = self.dg(u)
            rhs = f - self.g(u) + c * u
            if hip:
                if self.session is None:
                    self.session = make_session(self.problem, reaction=c, **self.kw)
                else:
                    self.session.set_reaction(c)
                if self.steps == 0:
                    self.session.init(rhs=rhs, w0=u)  # the session's w is u_k from here on
                res = float(self.session.residual_norm(rhs))
            else:
                res = self._residual_host(u, rhs, c)
            self.history.append(res)
            if not math.isfinite(res):
                raise FloatingPointError(f"Newton residual {res} at step {self.steps}")
            if res <= self.newton_rtol * self.history[0]:
                self.converged = True
                return u
            if self.steps == self.max_newton:
                return u
            if hip:
                self.last = self.session.solve(rhs=rhs, w0=u)
                u = self.session.w_tensor() if on_device else self.session.gather_local_w()
            else:
                r = solve(self.problem, self.backend, rhs=rhs, w0=u, reaction=c, **self.kw)
                self.last = dict(iters=r.iters, status=r.status, diff=r.diff, **r.extra)
                u = r.w
            self.steps += 1
