"""TorchPCG: the plain-PyTorch PCG (device-agnostic reference / distributed CPU path).

Mirrors stage2-mpi/poisson_mpi_decomp.cpp:356-460 (weighted norm, |denom| guard) or stage 0
(unweighted) on a 2D-decomposed grid, with torch tensors and a pluggable communicator
(parallel/comm.py).  With gloo it is the multi-process CPU path exercised by the test-suite;
with RCCL it runs on GPUs.  Not the fast path: the native HIP solver is.
"""
from __future__ import annotations

import math
import time

import torch

from ..ops import reference as R
from ..parallel.comm import SingleComm, edge_view, neighbours
from ..parallel.decomp import process_grid, subdomain
from .solvers import Result


class TorchPCG:
    def __init__(self, problem, device="cpu", dtype=torch.float64, comm=None, split="reference", reaction=None,
                 diffusion=None, domain=None):
        """reaction: optional global (M+1)x(N+1) float64 field c >= 0 (NumPy or a CPU tensor; boundary values
        ignored): the operator is A + (sigma + c) I, the diagonal D + sigma + c.
        diffusion: optional global (M+1)x(N+1) float64 field k > 0 on every node: the face coefficients are
        multiplied by the mean of k over the two nodes of the face (ops.reference.assemble).
        domain: optional global (M+1)x(N+1) float64 level-set field phi: D = {phi < 0} replaces the ellipse in the
        faces and in the right-hand-side mask (ops.reference.assemble)."""
        self.p = problem
        self.comm = comm or SingleComm()
        self.device = torch.device(device)
        self.dtype = dtype
        Px, Py = process_grid(self.comm.world, problem.M, problem.N, split)
        self.sd = subdomain(problem.M, problem.N, Px, Py, self.comm.rank)
        self.a, self.b, self.B = R.assemble(problem, self.sd, self.device, dtype,
                                            diffusion=problem.diffusion_field(diffusion),
                                            domain=problem.domain_field(domain))
        self.domain = problem.domain_field(domain)
        self.nbs = neighbours(self.sd)
        self.shift = problem.sigma  # a number, or with a reaction field the (nx, ny) tensor sigma + c
        c = problem.reaction_field(reaction)
        if c is not None:
            self.shift = (problem.sigma + self._local(c)[1:-1, 1:-1].to(torch.float64)).to(dtype)

    def _exchange(self, p: torch.Tensor):
        sends = [edge_view(p, s, ghost=False).contiguous() for s in range(4)]
        recvs = [torch.zeros_like(sends[s]) for s in range(4)]
        self.comm.exchange(sends, recvs, self.nbs)
        for s in range(4):
            g = edge_view(p, s, ghost=True)
            g.copy_(recvs[s] if self.nbs[s] >= 0 else torch.zeros_like(g))

    def _allsum(self, x: torch.Tensor) -> float:
        t = x.reshape(1).to(torch.float64)
        return float(self.comm.allreduce_(t).item())

    # ---- stepwise interface (same contract as the native Session: init / step / state) ----
    def _local(self, g):
        """This rank's block of a global (M+1)x(N+1) array with its ghost ring, global boundary zeroed."""
        sd = self.sd
        t = torch.as_tensor(g[sd["i_start"] - 1:sd["i_end"] + 2, sd["j_start"] - 1:sd["j_end"] + 2].copy())
        if sd["i_start"] == 1:
            t[0, :] = 0
        if sd["i_end"] == self.p.M - 1:
            t[-1, :] = 0
        if sd["j_start"] == 1:
            t[:, 0] = 0
        if sd["j_end"] == self.p.N - 1:
            t[:, -1] = 0
        return t.to(device=self.device, dtype=self.dtype)

    def init(self, rhs=None, w0=None):
        """rhs / w0: optional global (M+1)x(N+1) float64 arrays (NumPy or CPU tensors): B = rhs inside D
        (0 elsewhere) in place of the constant F, and the initial iterate, r^0 = B - A w0."""
        P = self.p
        h1, h2 = P.h1, P.h2
        rhs, w0 = P.field(rhs, "rhs"), P.field(w0, "w0")
        self.w = torch.zeros(self.B.shape, dtype=self.dtype, device=self.device)
        self.r = self.B.clone()
        if rhs is not None:
            inside = R.inside(P, self.sd, self.device) if self.domain is None else \
                R.inside_domain(P, self.sd, self.domain, self.device)
            self.r = torch.where(inside, self._local(rhs), torch.zeros_like(self.B))
            for edge in (self.r[0, :], self.r[-1, :], self.r[:, 0], self.r[:, -1]):
                edge.zero_()
        residual_rule = P.stop == "residual"
        rho_b = None
        if w0 is not None:
            if residual_rule:  # rho_B = (D^-1 B, B) while r still holds B
                zb = R.precond(self.r, self.a, self.b, h1, h2, self.shift)
                rho_b = self._allsum(R.dot(zb, self.r[1:-1, 1:-1], h1, h2))
            wl = self._local(w0)  # the ring comes from the global array: no exchange
            self.r[1:-1, 1:-1] -= R.apply_A(wl, self.a, self.b, h1, h2, self.shift)
            self.w[1:-1, 1:-1] = wl[1:-1, 1:-1]
        self.pv = torch.zeros_like(self.w)
        z = R.precond(self.r, self.a, self.b, h1, h2, self.shift)
        self.pv[1:-1, 1:-1] = z
        self.zr_old = self._allsum(R.dot(z, self.r[1:-1, 1:-1], h1, h2))
        self.k = 1
        self.done = False
        self.status, self.iters, self.diff = "max_iter", 0, float("nan")
        self.rho_b = self.thr = None
        if residual_rule:  # rho_0 is tested too: a start that is good enough ends with 0 iterations
            self.rho_b = self.zr_old if rho_b is None else rho_b
            self.thr = P.residual_threshold(self.rho_b)
            if self.zr_old <= self.thr * self.thr:
                self.done, self.status = True, "converged"

    def step(self, n: int = 1):
        """Run up to n iterations (no-ops once the stop rule fired, like the device flag)."""
        P = self.p
        h1, h2 = P.h1, P.h2
        weighted = P.norm == "weighted"
        a, b, w, r, p = self.a, self.b, self.w, self.r, self.pv
        for _ in range(n):
            if self.done:
                return
            if self.k > P.effective_max_iter():
                self.done, self.status = True, "max_iter"
                return
            k = self.k
            self.iters = k
            self._exchange(p)
            Ap = R.apply_A(p, a, b, h1, h2, self.shift)
            denom = self._allsum(R.dot(Ap, p[1:-1, 1:-1], h1, h2))
            tol = P.breakdown_tol
            if (abs(denom) < tol) if weighted else (denom < tol):
                self.done, self.status = True, "breakdown"
                return
            alpha = self.zr_old / denom
            w_old = w[1:-1, 1:-1].clone()
            w[1:-1, 1:-1] += alpha * p[1:-1, 1:-1]
            r[1:-1, 1:-1] -= alpha * Ap
            z = R.precond(r, a, b, h1, h2, self.shift)
            zr_new = self._allsum(R.dot(z, r[1:-1, 1:-1], h1, h2))
            dw = w[1:-1, 1:-1] - w_old
            dsum = self._allsum((dw * dw).sum(dtype=torch.float64))
            self.diff = math.sqrt(dsum * h1 * h2) if weighted else math.sqrt(dsum)
            self.k = k + 1
            if (zr_new <= self.thr * self.thr) if self.thr is not None else (self.diff < P.delta):
                self.zr_old = zr_new
                self.done, self.status = True, "converged"
                return
            beta = zr_new / self.zr_old
            self.zr_old = zr_new
            p[1:-1, 1:-1] = z + beta * p[1:-1, 1:-1]

    def state(self) -> dict:
        d = dict(it=self.k, done=self.done, iters=self.iters, status=self.status, diff=self.diff, nan=False)
        if self.thr is not None:
            d.update(residual=math.sqrt(self.zr_old), residual_ref=math.sqrt(self.rho_b))
        return d

    def local_error_stats(self) -> dict:
        """Unreduced (sum e^2, max |e|, max w) of this rank's block vs the analytic solution."""
        wl = self.w[1:-1, 1:-1].to(torch.float64).cpu().numpy()
        return self.p.local_error_stats(self.sd, wl)

    def synchronize(self):
        if self.device.type == "cuda":
            torch.cuda.synchronize(self.device)

    def solve(self, keep_solution: bool = True, rhs=None, w0=None) -> Result:
        P = self.p
        t0 = time.perf_counter()
        self.init(rhs=rhs, w0=w0)
        while not self.done:
            self.step(64)
        seconds = time.perf_counter() - t0
        iters, status, diff = self.iters, self.status, self.diff
        wl = None
        if keep_solution:
            wl = self.w[1:-1, 1:-1].to(torch.float64).cpu().numpy()
        res = Result(iters, status, diff, seconds, None, backend="torch", ranks=self.comm.world)
        res.extra["local_w"] = wl
        if self.thr is not None:
            res.extra.update(residual=math.sqrt(self.zr_old), residual_ref=math.sqrt(self.rho_b))
        res.extra["subdomain"] = self.sd
        if keep_solution and self.comm.world == 1:
            import numpy as np

            g = np.zeros((P.M + 1, P.N + 1))
            g[1:P.M, 1:P.N] = wl
            res.w = g
        return res
