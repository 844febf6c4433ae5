"""Picard iteration for the quasilinear problem -∇·(κ(u)∇u) = f in D, u = 0 on ∂D, on the solve with a
diffusion field: every step is one linear solve with the frozen coefficient k = κ(u_k)."""
from __future__ import annotations

import math

import numpy as np

from .problem import PoissonEllipse
from .solvers import make_session, solve


class QuasilinearPicard:
    """Step k solves -∇·(κ(u_k)∇u_{k+1}) (+ σ u_{k+1}) = f from w0 = u_k: the solve with diffusion = κ(u_k)
    (make_session / solve()).  The nonlinear residual of u_k is the linear residual of that system AT u_k,
    f - L_k u_k under the ellipse mask, so it is measured before the step's solve (h-weighted 2-norm,
    Session.residual_norm) and kept in `history`.  The iteration stops at the first k with
    history[k] <= picard_rtol history[0], or after max_picard steps.

    kappa: a callable on the iterate's type, returning the same type and shape, finite and > 0 on every node
    (the solver checks; the box-boundary nodes carry u = 0, so κ(0) must be > 0).

    backend "hip" keeps ONE native session (session_kw as make_session; ranks = 1, residual_norm's limit): each
    step replaces its diffusion field in place (Session.set_diffusion) and solves; with f (and u0) float64
    tensors on the session's device nothing passes through the host, and the result is a device tensor.  NumPy
    arrays in give a NumPy array out.  Every other backend of solve() runs NumPy end to end.  All fields are
    (M+1) x (N+1) float64.

    The linear solves stop by the problem's rule: pick stop="residual" with an rtol below picard_rtol (and
    breakdown_tol=0 with tight tolerances), or the Picard residual stalls at the accuracy of the inner solve.

    After solve(): `history` (residuals, one per step taken plus the final one), `steps` (linear solves),
    `converged`, `last` (statistics of the last linear solve).

    domain=phi in session_kw (solve()'s level-set field) poses the problem on D = {phi < 0}: every step calls
    Session.set_domain(phi, diffusion=κ(u_k)) on hip, and the residual's mask is that of phi."""

    def __init__(self, problem: PoissonEllipse, kappa, backend: str = "hip", picard_rtol: float = 1e-8,
                 max_picard: int = 50, **session_kw):
        if not (isinstance(picard_rtol, (int, float)) and math.isfinite(picard_rtol) and picard_rtol >= 0):
            raise ValueError(f"picard_rtol must be a finite number >= 0, got {picard_rtol!r}")
        if not (isinstance(max_picard, int) and max_picard >= 1):
            raise ValueError(f"max_picard must be an integer >= 1, got {max_picard!r}")
        if "diffusion" in session_kw:
            raise ValueError("QuasilinearPicard sets the diffusion field itself (kappa(u_k)); fold a fixed factor "
                             "into kappa")
        self.problem = problem
        self.kappa = kappa
        self.backend = backend
        self.picard_rtol = float(picard_rtol)
        self.max_picard = max_picard
        self.kw = session_kw
        self.session = None  # hip: built by the first solve (it needs a field to start from)
        self.history, self.steps, self.converged, self.last = [], 0, False, None

    def _residual_host(self, u, f, k) -> float:
        p = self.problem
        phi = self.kw.get("domain")
        e = np.where(p.inside_mask(phi), f, 0.0) - p.apply(u, reaction=self.kw.get("reaction"), diffusion=k, domain=phi)
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
            k = self.kappa(u)
            if hip:
                if self.session is None:
                    self.session = make_session(self.problem, diffusion=k, **self.kw)
                elif self.session.has_domain:  # the faces are refolded from phi and k together
                    self.session.set_domain(self.kw["domain"], diffusion=k)
                else:
                    self.session.set_diffusion(k)
                if self.steps == 0:
                    self.session.init(rhs=f, w0=u)  # the session's w is u_k from here on
                res = float(self.session.residual_norm(f))
            else:
                res = self._residual_host(u, f, k)
            self.history.append(res)
            if not math.isfinite(res):
                raise FloatingPointError(f"Picard residual {res} at step {self.steps}")
            if res <= self.picard_rtol * self.history[0]:
                self.converged = True
                return u
            if self.steps == self.max_picard:
                return u
            if hip:
                self.last = self.session.solve(rhs=f, w0=u)
                u = self.session.w_tensor() if on_device else self.session.gather_local_w()
            else:
                r = solve(self.problem, self.backend, rhs=f, w0=u, diffusion=k, **self.kw)
                self.last = dict(iters=r.iters, status=r.status, diff=r.diff, **r.extra)
                u = r.w
            self.steps += 1
