"""Solver entry points for every execution strategy of the reference.

=================  =====================================  ==========================================
backend            reference stage                        implementation
=================  =====================================  ==========================================
``cpu``            stage 0 serial (Withoutopenmp*.cpp)    native C++ oracle (csrc/cpu/cpu_pcg.cpp)
``omp``            stage 1 OpenMP (Withopenmp*.cpp)       native C++ oracle, OpenMP threads
``cpu-decomposed`` stage 2 MPI / stage 3 hybrid           native CpuSubdomain x P, in-process
                                                          lock-step (bin/pmx_mpi for real MPI)
``hip``            stage 4 MPI+CUDA                       native fused HIP kernels, SelfComm /
                                                          LocalComm (P subdomains on one GPU)
``torch``          (none: PyTorch reference)              models/torch_pcg.py, any device
=================  =====================================  ==========================================
Multi-process GPU runs (one rank per MI355X, RCCL) live in parallel/dist_solver.py.
"""
from __future__ import annotations

import dataclasses
import time
from typing import Optional

import numpy as np

from ..utils.native import load as _native
from .problem import PoissonEllipse


@dataclasses.dataclass
class Result:
    iters: int
    status: str
    diff: float
    seconds: float                 # solver wall time (excludes setup where measurable)
    w: Optional[np.ndarray] = None  # (M+1) x (N+1), boundary rows/cols zero (hip, keep_solution="device": a tensor)
    backend: str = ""
    ranks: int = 1
    init_seconds: float = 0.0
    extra: dict = dataclasses.field(default_factory=dict)

    @property
    def converged(self) -> bool:
        return self.status == "converged"

    def mlups(self, problem: PoissonEllipse) -> float:
        return problem.interior_points * self.iters / max(self.seconds, 1e-12) / 1e6


def solve(problem: PoissonEllipse, backend: str = "hip", **kw) -> Result:
    """rhs / w0 (every backend): optional (M+1)x(N+1) float64 arrays -- a right-hand side f(x_i, y_j) in
    place of the constant F (the solver applies the ellipse mask: values outside D and on the box
    boundary are ignored) and an initial iterate in place of w = 0.  The hip backend also takes float64
    tensors on its device for both and returns one with keep_solution="device" (solve_hip); every other
    backend rejects device tensors.

    problem.sigma != 0 (the screened problem (-Δ + σ) u = f): every backend solves it; hip runs pcg1 on the
    row march at any grid size and raises ValueError for algo="ca" / "pcg2", exact=True and block_tiles=1.

    problem.stop == "residual" (PoissonEllipse.stop / rtol / atol): every backend ends at the first k >= 0 with
    sqrt((z^k, r^k)) <= max(rtol sqrt((D^-1 B, B)), atol) -- relative to the data, also from a w0 -- and
    reports Result.extra["residual"] / ["residual_ref"]; diff keeps the last |alpha| ||p||.  hip runs it on pcg1
    (march and block tiles), pcg2 (exact=True included) and the s-step PCG; auto keeps its choice.  The
    reference's absolute breakdown guard (breakdown_tol = 1e-15) fires before a tight rtol is reached on data of
    the default size: lower it (0 = off) with such tolerances.

    reaction (every backend): an (M+1)x(N+1) float64 field c(x, y), finite and >= 0 on the interior nodes (its
    box-boundary values are ignored and never read): the solve is (-Δ + σ + c) u = f, with D + σ + c as the
    Jacobi diagonal.  hip runs it under sigma's rules (pcg1 on the row march; ValueError for algo="ca" / "pcg2",
    exact=True, block_tiles=1) and also takes a float64 tensor on its device; see make_session.

    diffusion (every backend): an (M+1)x(N+1) float64 field k(x, y) of nodal values, finite and > 0 on EVERY node
    (the faces next to the box boundary read its boundary values): the solve is (-∇·k∇ + σ + c) u = f.  The face
    coefficients become (0.5 (k[i-1,j] + k[i,j])) a[i,j] and (0.5 (k[i,j-1] + k[i,j])) b[i,j] -- the fictitious
    1/ε included, so the medium outside D is k/ε -- and D, A x and the stop rules are the same algebra on them.
    k = 1 is the solve without the argument, bitwise on the CPU backends.  hip: under reaction's rules.

    domain (every backend): an (M+1)x(N+1) float64 field phi(x, y) of nodal level-set values, finite on every node:
    D = {phi < 0} replaces the ellipse.  In fp64, in this order: phi_c[i,j] = 0.25 ((phi[i-1,j-1] + phi[i-1,j]) +
    (phi[i,j-1] + phi[i,j])) at the cell centres; the inside fraction of a face with end values p, q is 1 if both
    are < 0, 0 if neither is, else n / (n - m) with n the negative one -- ONE linear crossing per face, so features
    thinner than a cell are not resolved; the coefficient is theta + (1 - theta) / eps, without the ellipse's 1e-9
    snapping; a[i,j] takes phi_c[i,j], phi_c[i,j+1] and b[i,j] takes phi_c[i,j], phi_c[i+1,j].  The right-hand side
    is masked by phi[i,j] < 0.  diffusion scales these faces as it scales the ellipse's, and without it the solve is
    that of k = 1, bitwise.  A component of the complement of D that does not touch the box boundary is no Dirichlet
    hole: nothing anchors u there and it floats to a constant; pin it with reaction=np.where(hole, 1e8, 0).
    PoissonEllipse.ellipse_levelset() is the ellipse as such a field.  hip: under diffusion's rules."""
    if backend in ("cpu", "serial"):
        return solve_cpu(problem, threads=1, **kw)
    if backend in ("omp", "openmp"):
        return solve_cpu(problem, **kw)
    if backend in ("cpu-decomposed", "mpi", "hybrid"):
        return solve_cpu_decomposed(problem, **kw)
    if backend == "hip":
        return solve_hip(problem, **kw)
    if backend == "torch":
        from .torch_pcg import TorchPCG

        rhs, w0 = kw.pop("rhs", None), kw.pop("w0", None)
        return TorchPCG(problem, **kw).solve(rhs=rhs, w0=w0)
    raise ValueError(f"unknown backend {backend!r}")


def _residual_extra(r) -> dict:
    """The residual rule's report (absent under the step rule): sqrt(rho) at the end and sqrt(rho_B)."""
    return {k: r[k] for k in ("residual", "residual_ref") if k in r}


def solve_cpu(problem: PoissonEllipse, threads: int = 1, keep_solution: bool = True, rhs=None, w0=None,
              reaction=None, diffusion=None, domain=None) -> Result:
    r = _native().cpu_solve(problem.to_native(), int(threads), bool(keep_solution), rhs=rhs, w0=w0,
                            reaction=reaction, diffusion=diffusion, domain=domain)
    return Result(r["iters"], r["status"], r["diff"], r["seconds"], r.get("w"),
                  backend="cpu" if threads <= 1 else f"omp{threads}", extra=_residual_extra(r))


def solve_cpu_decomposed(problem: PoissonEllipse, ranks: int = 4, split: str = "reference",
                         threads: int = 1, keep_solution: bool = True, rhs=None, w0=None,
                         reaction=None, diffusion=None, domain=None) -> Result:
    n = _native()
    r = n.cpu_solve_decomposed(problem.to_native(), int(ranks), getattr(n.Split, split), int(threads),
                               bool(keep_solution), rhs=rhs, w0=w0, reaction=reaction, diffusion=diffusion,
                               domain=domain)
    return Result(r["iters"], r["status"], r["diff"], r["seconds"], r.get("w"),
                  backend="cpu-decomposed", ranks=ranks, extra=_residual_extra(r))


def make_session(problem: PoissonEllipse, ranks: int = 1, split: str = "reference", device: int = 0,
                 dtype: str = "fp64", kernel: str = "wave", block: int = 256, vec: int = 0, waves: int = 4,
                 tile_rows: int = 0, exact: bool = False, graph_batch: int = 32, check: bool = False,
                 overlap: bool = True, vec_b: int = 0, waves_b: int = 0, tile_rows_b: int = -1,
                 poison_halos: bool = False, b_ring: bool = False, placement: int = 0,
                 placement_budget_s: float = 0.5, placement_keep_free: float = 0.5, block_tiles: int = -1,
                 algo: str | int = -1, ca_s: int = 3, reaction=None, diffusion=None, domain=None):
    """Native GPU session with `ranks` subdomains on one device (LocalComm when ranks > 1).

    overlap: ghost exchange on a second stream concurrent with pcg_b (only matters for ranks > 1).

    kernel="wave": wave-tile kernels with DPP neighbour shifts (vec columns/lane, `waves` tiles per
    workgroup; the round-1 "lds" kernels are retired, bench/RETIRED.md).  vec=0 picks the measured
    best per kernel (pcg_a 4, pcg_b 2 in fp64); *_b override pcg_b's shape alone.
    pcg_b runs the ring-free 2-row kernel by default; b_ring=True selects the pipelined one.

    placement: up to this many candidate field blocks are timed and the fastest kept (0 = off, the
    default; bounded by placement_budget_s seconds and by leaving placement_keep_free of the free
    device memory free -- see GpuSubdomainSolver::place_fields).

    block_tiles: -1 = auto (block-tile sweeps, pcg1_block.hip, on small undecomposed fp64 grids), 0 = off,
    1 = on for any undecomposed fp64 grid.

    algo: -1 / "auto" (the library's choice: the s-step on grids of >= 6M points -- one GPU, row strips
    or 2-D blocks -- when its fields fit, else pcg1 / pcg2), "pcg1" / 1, "pcg2" / 2, or "ca" / 3 -- the
    s-step PCG (ca_kernels.hip: ca_s = 2 or 3 iterations per fused pass and one reduction; fp64, fp32
    or mixed storage, fp64 basis and sums).

    reaction: an (M+1)x(N+1) float64 field c(x, y), finite and >= 0 on the interior nodes (box-boundary values
    ignored and never read): the session's operator is L = A + (σ + c) I -- in its solves, residual_norm and
    apply -- with D + σ + c as the Jacobi diagonal.  A NumPy array, a CPU tensor, or a float64 tensor on the
    session's device (unit column stride, row stride >= N+1; read in place by a kernel after the work already
    enqueued on its stream).  The session keeps T(σ + c), rounded ONCE to its storage type T, in one more
    field (the shift field): with dtype "fp32" / "mixed" its operator is A + fp32(σ + c) everywhere.
    Session.set_reaction(c) replaces the field in place (captured graphs stay valid); step() then raises until
    the next init() / solve().  The rules of sigma != 0 apply at any sigma: pcg1 on the row march, ValueError
    for algo="ca" / "pcg2", exact=True, block_tiles=1 and checkpoints; error_norms needs exact=.

    diffusion: an (M+1)x(N+1) float64 field k(x, y) of nodal values, finite and > 0 on EVERY node (the box
    boundary included): the session's operator is -∇·k∇ + σ + c, see solve().  The same kinds of objects as
    reaction.  The session keeps two complete face-coefficient fields, aκ = (0.5 (k[i-1,j] + k[i,j])) a and
    bκ = (0.5 (k[i,j-1] + k[i,j])) b, formed in fp64 and rounded ONCE to its storage type, behind the shift field
    (which a diffusion session always holds: T(σ + c), c = 0 without reaction); its sweeps read them in place of
    the 1-D tables.  dtype "fp32" runs the mixed arithmetic (fp32 fields, fp64 registers) on such a session.
    Session.set_diffusion(k) replaces the fields in place, as set_reaction does; the refusals of reaction
    apply.

    domain: an (M+1)x(N+1) float64 level-set field phi, finite on every node (the same kinds of objects): D =
    {phi < 0} replaces the ellipse, see solve().  A domain session is a diffusion session -- k = 1 without
    diffusion, bitwise the session with diffusion=ones -- whose face-coefficient fields hold the faces of D (one
    setup kernel reads phi, on the device, across subdomain borders), plus one mask byte per owned node for the
    right-hand side; phi is not retained.  Session.set_domain(phi, diffusion=None) replaces faces and mask in place
    (a moving domain on captured graphs); set_diffusion raises on such a session, since the faces cannot be
    refolded without phi.  The refusals of diffusion apply."""
    n = _native()
    algo = {"auto": -1, "pcg1": 1, "pcg2": 2, "ca": 3}.get(algo, algo) if isinstance(algo, str) else algo
    return n.Session(problem.to_native(), world=int(ranks), comm="self" if ranks == 1 else "local",
                     split=getattr(n.Split, split), device=device, kernel=kernel, block=block, vec=vec,
                     waves=waves, tile_rows=tile_rows, dtype=dtype, exact=exact, graph_batch=graph_batch,
                     check=check, overlap=overlap, vec_b=vec_b, waves_b=waves_b, tile_rows_b=tile_rows_b,
                     poison_halos=poison_halos, b_ring=b_ring, placement=placement,
                     placement_budget_s=placement_budget_s, placement_keep_free=placement_keep_free,
                     block_tiles=block_tiles, algo=int(algo), ca_s=int(ca_s), reaction=reaction,
                     diffusion=diffusion, domain=domain)


def solve_hip(problem: PoissonEllipse, ranks: int = 1, keep_solution: bool = True, poll_batches: int = 1,
              rhs=None, w0=None, **session_kw) -> Result:
    """rhs / w0: see solve(); the session uploads them for this solve and retains nothing
    (Session.init(rhs=..., w0=...)).  Here they may also be float64 tensors on the session's device
    (any object with __cuda_array_interface__): kernels read them in place, after the work already
    enqueued on the current torch stream, with no synchronisation by the caller.

    keep_solution: True -- Result.w is a NumPy array; "device" -- a torch.float64 tensor on the session's
    device (Session.w_tensor(): no pass through the host, usable at once on the current torch stream);
    False -- None."""
    if not isinstance(keep_solution, bool) and keep_solution != "device":
        raise ValueError(f"keep_solution must be True, False or 'device', got {keep_solution!r}")
    t0 = time.perf_counter()
    s = make_session(problem, ranks=ranks, **session_kw)
    st = s.solve(poll_batches, rhs=rhs, w0=w0)
    w = s.w_tensor() if keep_solution == "device" else s.gather_local_w() if keep_solution else None
    r = Result(st["iters"], st["status"], st["diff"], st["solve_seconds"], w, backend="hip", ranks=ranks,
               init_seconds=st["init_seconds"],
               extra=dict(launched=st["launched"], nan=st["nan"], setup_seconds=time.perf_counter() - t0,
                          comm=s.comm_name, grid=s.grid, device_bytes=s.device_bytes, **_residual_extra(st)))
    del s
    return r
