"""Implicit time stepping on the screened solve for u_t = Δu + g in D, u = 0 on ∂D: backward Euler, and the
θ-scheme (Crank-Nicolson at θ = 1/2) on top of the operator apply."""
from __future__ import annotations

import dataclasses
import math

from .problem import PoissonEllipse
from .solvers import make_session, solve


class BackwardEuler:
    """One step solves (1/dt - Δ) u⁺ = u/dt + g with w0 = u: the problem with sigma = 1/dt (added to the
    problem's own sigma, a reaction term).  backend "hip" keeps ONE native session for all steps
    (session_kw as make_session); a device tensor in gives a device tensor out, with no pass through
    the host.  Every other backend of solve() takes and returns NumPy arrays.  All fields are
    (M+1) x (N+1) float64; g may be a scalar.  The problem's stop rule carries over: with stop="residual"
    every step solves to rtol relative to its own right-hand side u/dt + g, not to the already small
    residual of its start w0 = u.  reaction=c in session_kw (make_session's / solve()'s field, every backend)
    steps u_t = Δu - c u + g; diffusion=k likewise steps u_t = ∇·(k∇u) + g (variable conductivity); domain=phi
    poses either on D = {phi < 0} instead of the ellipse."""

    def __init__(self, problem: PoissonEllipse, dt: float, backend: str = "hip", **session_kw):
        if not (isinstance(dt, (int, float)) and math.isfinite(dt) and dt > 0):
            raise ValueError(f"dt must be a finite number > 0, got {dt!r}")
        self.dt = float(dt)
        self.backend = backend
        self.problem = dataclasses.replace(problem, sigma=problem.sigma + 1.0 / self.dt)
        self.kw = session_kw
        self.session = make_session(self.problem, **session_kw) if backend == "hip" else None
        self.last = None  # statistics of the last step's solve (iters, status, diff, ...)

    def step(self, u, g=None):
        rhs = u / self.dt if g is None else u / self.dt + g
        if self.session is None:
            r = solve(self.problem, self.backend, rhs=rhs, w0=u, **self.kw)
            self.last = dict(iters=r.iters, status=r.status, diff=r.diff, **r.extra)
            return r.w
        self.last = self.session.solve(rhs=rhs, w0=u)
        on_device = hasattr(u, "__cuda_array_interface__")
        return self.session.w_tensor() if on_device else self.session.gather_local_w()


class ThetaScheme:
    """The θ-scheme for u_t = -(A + σ_p) u + g, σ_p the problem's own sigma: θ = 1/2 is Crank-Nicolson (second
    order in dt), θ = 1 backward Euler.  With s = 1/(θ dt) and L = A + (σ_p + s) I -- the operator of this
    scheme's problem and session -- one step solves

        L u⁺ = (s/θ) u - ((1-θ)/θ) L u + g/θ          from w0 = u,

    whose right-hand side is ONE operator apply (Session.apply / PoissonEllipse.apply) with alpha = -(1-θ)/θ,
    beta = s/θ and y = g, gamma = 1/θ (a scalar g: const = g/θ).  θ = 1 needs no apply: its right-hand side is
    BackwardEuler's u/dt + g, and its steps are BackwardEuler's bitwise.  As there, the solve applies the
    ellipse mask to the right-hand side.

    backend "hip" keeps ONE native session for all steps (session_kw as make_session); device tensors in (u,
    and g unless it is a scalar) give a device tensor out, with nothing through the host; NumPy arrays in give
    a NumPy array out.  Every other backend of solve() takes and returns NumPy arrays.  All fields are
    (M+1) x (N+1) float64.  `last` holds the statistics of the last step's solve, and the problem's stop rule
    carries over as in BackwardEuler.  reaction=c in session_kw adds the field to L, on both sides of the step:
    the solve and the apply of the right-hand side; diffusion=k likewise makes A the k operator on both sides, and
    domain=phi the operator (and the mask) of D = {phi < 0}."""

    def __init__(self, problem: PoissonEllipse, dt: float, theta: float = 0.5, backend: str = "hip", **session_kw):
        if not (isinstance(dt, (int, float)) and math.isfinite(dt) and dt > 0):
            raise ValueError(f"dt must be a finite number > 0, got {dt!r}")
        if not (isinstance(theta, (int, float)) and 0 < theta <= 1):
            raise ValueError(f"theta must be a number in (0, 1], got {theta!r}")
        self.dt = float(dt)
        self.theta = float(theta)
        self.s = 1.0 / (self.theta * self.dt)
        self.backend = backend
        self.problem = dataclasses.replace(problem, sigma=problem.sigma + self.s)
        self.kw = session_kw
        self.session = make_session(self.problem, **session_kw) if backend == "hip" else None
        self.last = None  # statistics of the last step's solve (iters, status, diff, ...)

    def rhs(self, u, g=None):
        """The step's right-hand side, on u's side (device tensor or NumPy array)."""
        th = self.theta
        if th == 1.0:
            return u / self.dt if g is None else u / self.dt + g
        kw = dict(alpha=-(1.0 - th) / th, beta=self.s / th)
        if isinstance(g, (int, float)):
            kw["const"] = g / th
        elif g is not None:
            kw.update(y=g, gamma=1.0 / th)
        on_device = hasattr(u, "__cuda_array_interface__")
        if on_device and self.session is not None:
            return self.session.apply(u, **kw)  # the session's operator: its reaction field included
        return self.problem.apply(u, reaction=self.kw.get("reaction"), diffusion=self.kw.get("diffusion"),
                                  domain=self.kw.get("domain"), **kw)

    def step(self, u, g=None):
        rhs = self.rhs(u, g)
        if self.session is None:
            r = solve(self.problem, self.backend, rhs=rhs, w0=u, **self.kw)
            self.last = dict(iters=r.iters, status=r.status, diff=r.diff, **r.extra)
            return r.w
        self.last = self.session.solve(rhs=rhs, w0=u)
        on_device = hasattr(u, "__cuda_array_interface__")
        return self.session.w_tensor() if on_device else self.session.gather_local_w()
