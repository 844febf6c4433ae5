"""Implicit time stepping on the screened solve: backward Euler for u_t = Δu + g in D, u = 0 on ∂D."""
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
    residual of its start w0 = u."""

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
