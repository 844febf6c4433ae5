"""Problem family: 2D Poisson -Δu = F in an ellipse, fictitious-domain PCG.

This is the one "model family" of the reference (MSU course project, variant 9): every stage
solves the same discrete problem (stage0/Withoutopenmp1.cpp:9-61) and
differs only in execution strategy.  ``PoissonEllipse`` carries the problem; ``STAGES`` maps
each reference stage to the execution strategy that reproduces it here.
"""
from __future__ import annotations

import dataclasses
import math
from typing import Optional

import numpy as np

from ..utils.native import load as _native


@dataclasses.dataclass
class PoissonEllipse:
    M: int = 40
    N: int = 40
    A1: float = -1.0
    B1: float = 1.0
    A2: float = -0.6
    B2: float = 0.6
    ax: float = 1.0          # ellipse semi-axis along x   (reference: x^2 + 4y^2 < 1)
    by: float = 0.5          # ellipse semi-axis along y
    F: float = 1.0
    delta: float = 1e-6      # stage0/Withoutopenmp1.cpp:178
    max_iter: Optional[int] = None   # None -> (M-1)(N-1)  (stage0/Withoutopenmp1.cpp:182)
    norm: str = "weighted"   # "weighted" (stages 1-4) | "unweighted" (stage 0)
    breakdown_tol: float = 1e-15     # CG guard on (Ap,p) (stage0/Withoutopenmp1.cpp:130); see spec.hpp
    sigma: float = 0.0       # screened problem (-Δ + σ) u = f, σ >= 0 constant; 0 = the reference's problem
    # Stop rule.  "step": the reference's, ||w^{k+1} - w^k|| < delta.  "residual": the solve ends after
    # iteration k >= 0 at the first k with sqrt(rho_k) <= max(rtol sqrt(rho_B), atol), rho_k = (z^k, r^k),
    # z = (D + σ)^-1 r, rho_B = ((D + σ)^-1 B, B), B the masked right-hand side (spec.hpp); delta is ignored.
    stop: str = "step"
    rtol: float = 1e-8       # read under stop="residual" only; finite and >= 0
    atol: float = 0.0        # likewise

    def __post_init__(self):
        if self.norm not in ("weighted", "unweighted"):
            raise ValueError(f"norm must be weighted|unweighted, got {self.norm!r}")
        if self.M < 2 or self.N < 2:
            raise ValueError("grid must be at least 2x2 cells")
        try:
            self.sigma = float(self.sigma)
        except (TypeError, ValueError):
            raise ValueError(f"sigma must be a finite number >= 0, got {self.sigma!r}") from None
        if not math.isfinite(self.sigma) or self.sigma < 0:
            raise ValueError(f"sigma must be finite and >= 0, got {self.sigma!r}")
        if self.stop not in ("step", "residual"):
            raise ValueError(f"stop must be step|residual, got {self.stop!r}")
        for name in ("rtol", "atol"):
            v = getattr(self, name)
            try:
                v = float(v)
            except (TypeError, ValueError):
                raise ValueError(f"{name} must be a finite number >= 0, got {v!r}") from None
            if not math.isfinite(v) or v < 0:
                raise ValueError(f"{name} must be finite and >= 0, got {v!r}")
            setattr(self, name, v)

    def residual_threshold(self, rho_b: float) -> float:
        """The residual rule's bound on sqrt(rho): max(rtol sqrt(rho_B), atol)."""
        return max(self.rtol * math.sqrt(rho_b), self.atol)

    # ---- derived quantities (stage0/Withoutopenmp1.cpp:107-108) ----
    @property
    def h1(self) -> float:
        return (self.B1 - self.A1) / self.M

    @property
    def h2(self) -> float:
        return (self.B2 - self.A2) / self.N

    @property
    def eps(self) -> float:
        return max(self.h1, self.h2) ** 2

    @property
    def interior_points(self) -> int:
        return (self.M - 1) * (self.N - 1)

    def effective_max_iter(self) -> int:
        return self.max_iter if self.max_iter is not None else (self.M - 1) * (self.N - 1)

    def is_reference_ellipse(self) -> bool:
        return self.ax == 1.0 and self.by == 0.5

    def to_native(self):
        n = _native()
        s = n.ProblemSpec()
        for f in ("M", "N", "A1", "B1", "A2", "B2", "ax", "by", "F", "delta", "breakdown_tol", "sigma", "rtol",
                  "atol"):
            setattr(s, f, getattr(self, f))
        s.stop = n.StopRule.residual if self.stop == "residual" else n.StopRule.step
        s.max_iter = -1 if self.max_iter is None else int(self.max_iter)
        s.norm = n.Norm.weighted if self.norm == "weighted" else n.Norm.unweighted
        return s

    # ---- geometry on the host (numpy) ----
    def coords(self):
        x = self.A1 + np.arange(self.M + 1) * self.h1
        y = self.A2 + np.arange(self.N + 1) * self.h2
        return x, y

    def exact_solution(self, x, y):
        """u = F (1 - x²/ax² - y²/by²) / (2/ax² + 2/by²) inside D, 0 outside.

        For the reference ellipse this is (1 - x² - 4y²)/10 (итоговый отчёт/Этап_4_1213.pdf p.1).
        It solves the σ = 0 problem only: with sigma != 0 this raises ValueError."""
        self.require_closed_form("exact_solution")
        q = 1.0 - (x / self.ax) ** 2 - (y / self.by) ** 2
        c = self.F / (2.0 / self.ax ** 2 + 2.0 / self.by ** 2)
        return np.where(q > 0, c * q, 0.0)

    def require_closed_form(self, what: str, domain=None):
        if domain is not None:
            raise ValueError(f"{what}: the closed-form solution belongs to the ellipse, not to a level-set domain; "
                             "pass the solution of your problem as exact=")
        if self.sigma != 0.0:
            raise ValueError(f"{what}: the closed-form solution holds for sigma = 0 only (sigma = {self.sigma}); "
                             "pass the solution of your problem as exact=")

    def inside_mask(self, domain=None):
        """The nodes of D as an (M+1)x(N+1) bool array: the ellipse, or phi < 0 for a level-set field `domain`
        (domain_field()'s rules)."""
        if domain is not None:
            return self.domain_field(domain) < 0.0
        x, y = self.coords()
        X, Y = np.meshgrid(x, y, indexing="ij")
        if self.is_reference_ellipse():
            return X * X + 4.0 * Y * Y < 1.0
        return (X / self.ax) ** 2 + (Y / self.by) ** 2 < 1.0

    def local_error_stats(self, sd: dict, local: np.ndarray) -> dict:
        """Unreduced error statistics of one subdomain's interior block (nx x ny, global nodes
        i_start..i_end x j_start..j_end): the host twin of the device k_error_norms."""
        self.require_closed_form("local_error_stats")
        x, y = self.coords()
        X, Y = np.meshgrid(x[sd["i_start"]:sd["i_end"] + 1], y[sd["j_start"]:sd["j_end"] + 1], indexing="ij")
        u = self.exact_solution(X, Y)
        m = (X * X + 4.0 * Y * Y < 1.0) if self.is_reference_ellipse() else \
            ((X / self.ax) ** 2 + (Y / self.by) ** 2 < 1.0)
        e = np.where(m, local - u, 0.0)
        return {"sum_e2": float((e * e).sum()), "max_error": float(np.abs(e).max(initial=0.0)),
                "max_w": float(local.max(initial=-np.inf))}

    def field(self, a, name: str = "field") -> Optional[np.ndarray]:
        """A user field (rhs, w0, exact) as a C-contiguous float64 (M+1)x(N+1) array, or None.

        Accepts NumPy arrays and CPU torch tensors; ValueError for any other type, dtype or shape, for a
        device tensor and for non-finite values (the native entry points apply the same rules)."""
        if a is None:
            return None
        a = self._host_array(a, name, apply_hint=False)
        if not np.isfinite(a).all():
            raise ValueError(f"{name} holds non-finite values")
        return np.ascontiguousarray(a)

    def reaction_field(self, c, name: str = "reaction") -> Optional[np.ndarray]:
        """A reaction field c(x, y) as a C-contiguous float64 (M+1)x(N+1) array, or None: field()'s type, dtype
        and shape rules; finite and >= 0 on the interior nodes, the box-boundary values ignored (ValueError
        otherwise -- the native entry points apply the same rules)."""
        if c is None:
            return None
        a = self._host_array(c, name)
        inner = a[1:-1, 1:-1]
        if not (np.isfinite(inner).all() and (inner >= 0).all()):
            raise ValueError(f"{name} must be finite and >= 0 on every interior node")
        return np.ascontiguousarray(a)

    def diffusion_field(self, k, name: str = "diffusion") -> Optional[np.ndarray]:
        """A diffusion field k(x, y) as a C-contiguous float64 (M+1)x(N+1) array, or None: field()'s type, dtype
        and shape rules; finite and > 0 on EVERY node -- the faces next to the box boundary read the boundary
        values (ValueError otherwise; the native entry points apply the same rules)."""
        if k is None:
            return None
        a = self._host_array(k, name)
        if not (np.isfinite(a).all() and (a > 0).all()):
            raise ValueError(f"{name} must be finite and > 0 on every node")
        return np.ascontiguousarray(a)

    def domain_field(self, phi, name: str = "domain") -> Optional[np.ndarray]:
        """A level-set field phi(x, y) as a C-contiguous float64 (M+1)x(N+1) array, or None: field()'s rules --
        type, dtype, shape, finite on every node.  D = {phi < 0}; see solve()."""
        return self.field(phi, name)

    def ellipse_levelset(self) -> np.ndarray:
        """(x/ax)² + (y/by)² - 1 on the nodes (x² + 4y² - 1 for the reference ellipse): this problem's ellipse as
        a level-set field.  Shapes combine by np.minimum (union) and np.maximum (intersection; of phi and -psi:
        phi with psi cut out)."""
        x, y = self.coords()
        X, Y = np.meshgrid(x, y, indexing="ij")
        if self.is_reference_ellipse():
            return X * X + 4.0 * Y * Y - 1.0
        return (X / self.ax) ** 2 + (Y / self.by) ** 2 - 1.0

    def _host_array(self, a, name: str, writable: bool = False, apply_hint: bool = True) -> np.ndarray:
        """field()'s type, dtype and shape rules without its finiteness scan (apply's arguments, whose refusal of
        a device tensor points to Session.apply)."""
        if hasattr(a, "numpy") and hasattr(a, "device"):  # a torch tensor
            if a.device.type != "cpu":
                raise ValueError(f"{name}: device tensors are not supported, pass a NumPy array or a CPU tensor"
                                 + (" (Session.apply takes device tensors)" if apply_hint else ""))
            a = a.detach().numpy()
        if not isinstance(a, np.ndarray):
            raise ValueError(f"{name} must be a NumPy array or a CPU torch tensor")
        if a.dtype != np.float64:
            raise ValueError(f"{name} must have dtype float64, got {a.dtype}")
        if a.shape != (self.M + 1, self.N + 1):
            raise ValueError(f"{name} must have shape (M+1, N+1) = {(self.M + 1, self.N + 1)}, got {a.shape}")
        if writable and not a.flags.writeable:
            raise ValueError(f"{name} is read-only")
        return a

    def apply(self, x, out=None, *, alpha: float = 1.0, beta: float = 0.0, y=None, gamma: float = 1.0,
              const: float = 0.0, reaction=None, diffusion=None, domain=None) -> np.ndarray:
        """alpha L x + beta x + gamma y + const on the interior nodes and 0 on the box boundary, on the host
        (the CPU oracle's stencil); L = A + sigma I with this problem's sigma, the plain matrix on the whole
        box -- fictitious region included, no ellipse mask.  The host twin of Session.apply: NumPy arrays
        (or CPU tensors) of shape (M+1, N+1) float64 in, a NumPy array out (`out` when given; it may be y
        and must not overlap x).  Boundary values of x count as 0 and are not read.  x is not scanned for
        non-finite values: a NaN propagates to the nodes whose stencil reads it.

        reaction: optional field c(x, y) >= 0 (reaction_field()'s rules): L = A + (sigma + c) I, the operator of
        a session built with that field.

        diffusion: optional nodal field k(x, y) > 0 (diffusion_field()'s rules): A becomes -div(k grad .) with
        the face coefficients (0.5 (k + k')) a, (0.5 (k + k')) b of the two nodes of a face.

        domain: optional level-set field phi (domain_field()'s rules): a, b are the faces of D = {phi < 0} instead
        of the ellipse's (see solve()); still the matrix on the whole box, no mask."""
        xa = self._host_array(x, "x")
        ca = self.reaction_field(reaction)
        ka = self.diffusion_field(diffusion)
        pa = self.domain_field(domain)
        ya = None if y is None else self._host_array(y, "y")
        oa = None if out is None else self._host_array(out, "out", writable=True)
        for name, v in (("alpha", alpha), ("beta", beta), ("gamma", gamma), ("const", const)):
            if not (isinstance(v, (int, float)) and math.isfinite(v)):
                raise ValueError(f"{name} must be a finite number, got {v!r}")
        if oa is not None and np.may_share_memory(oa, xa):
            raise ValueError("out overlaps x")
        r = _native().cpu_apply(self.to_native(), np.ascontiguousarray(xa),
                                None if ya is None else np.ascontiguousarray(ya), float(alpha), float(beta),
                                float(gamma), float(const), reaction=ca, diffusion=ka, domain=pa)
        if oa is None:
            return r
        oa[...] = r
        return oa

    def error_norms(self, w: np.ndarray, exact: Optional[np.ndarray] = None, domain=None) -> dict:
        """L2 (h-weighted) and max error of a (M+1)x(N+1) solution in D, vs the analytic solution of the
        constant-F problem or, for another right-hand side, vs `exact` ((M+1)x(N+1) values of its solution).
        domain: the level-set field of the solve: D is its mask, and `exact` is required (ValueError without)."""
        x, y = self.coords()
        X, Y = np.meshgrid(x, y, indexing="ij")
        if exact is None:
            self.require_closed_form("error_norms", domain)
        u = self.exact_solution(X, Y) if exact is None else self.field(exact, "exact")
        m = self.inside_mask(domain)
        e = np.where(m, w - u, 0.0)
        return {
            "l2_error": float(math.sqrt(float((e * e).sum()) * self.h1 * self.h2)),
            "max_error": float(np.abs(e).max()),
            "max_w": float(w.max()),
        }


# Reference stage -> (execution strategy, stop norm).  SURVEY §0 table.
STAGES = {
    "stage0": dict(backend="cpu", threads=1, norm="unweighted",
                   ref="stage0/Withoutopenmp1.cpp"),
    "stage1": dict(backend="omp", norm="weighted", ref="stage1-openmp/Withopenmp1.cpp"),
    "stage2": dict(backend="cpu-decomposed", threads=1, norm="weighted",
                   ref="stage2-mpi/poisson_mpi_decomp.cpp"),
    "stage3": dict(backend="cpu-decomposed", norm="weighted", ref="stage3-openmp+mpi/hybrid.cpp"),
    "stage4": dict(backend="hip", norm="weighted", ref="stage4-mpi+cuda/poisson_mpi_cuda_f.cu"),
}


def stage_problem(stage: str, M: int, N: int, **kw) -> PoissonEllipse:
    if stage not in STAGES:
        raise KeyError(f"unknown stage {stage!r}; choose from {sorted(STAGES)}")
    return PoissonEllipse(M=M, N=N, norm=STAGES[stage]["norm"], **kw)
