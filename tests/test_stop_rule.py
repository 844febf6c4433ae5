"""The residual stop rule (PoissonEllipse.stop = "residual", rtol, atol) on the CPU paths: validation, the
native oracle (serial, OpenMP, decomposed), the plain-PyTorch PCG, the PyTorch s-step PCG and the CLI.

The solve ends after iteration k >= 0 at the first k with sqrt(rho_k) <= max(rtol sqrt(rho_B), atol),
rho_k = (z^k, r^k), rho_B = (D^-1 B, B).  The reference has no such rule: the yardsticks are the project's
serial oracle and, independently, TorchPCG.

Exact counts are only demanded where the threshold is not grazed: for every (grid, data, rtol) used the
oracle returns the same count at rtol (1 - 1e-3) and rtol (1 + 1e-3) -- `oracle_count` asserts it.  The
values below were picked on the serial oracle so that this holds; their counts (f = 1 / manufactured f):

    grid      rtol    f = 1   manufactured
    40x40     1e-4      57        81
    40x40     1e-8      91       122
    97x130    1e-4     176       256
    97x130    1e-8     282       380

(rtol 1e-6 grazes at 40x40 with the manufactured f: 101 / 100 iterations -- not used.)

Every residual-rule problem here sets breakdown_tol = 0.  The reference's guard |(A p, p)| < 1e-15 is an
absolute bound, so it fires before a tight relative tolerance is reached on data of this size (f = 1 at
40x40: breakdown after 75 iterations at sqrt(rho) = 1.6e-6 sqrt(rho_B)), and it is not scale covariant.
"""
import json
import math
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT, sub
from test_init_data import manufactured

BIN = os.path.join(ROOT, "poisson-ellipse-openmp-mpi-cuda-new_amd", "bin")
# (grid, rtol) -> oracle counts (f = 1, manufactured f)
COUNTS = {((40, 40), 1e-4): (57, 81), ((40, 40), 1e-8): (91, 122),
          ((97, 130), 1e-4): (176, 256), ((97, 130), 1e-8): (282, 380)}


def problem(pkg, grid, rtol=1e-8, **kw):
    kw.setdefault("breakdown_tol", 0.0)  # see the module docstring
    return pkg.PoissonEllipse(M=grid[0], N=grid[1], stop="residual", rtol=rtol, **kw)


def oracle_count(pkg, p, **data):
    """The serial oracle's solve at p.rtol, after asserting the precondition for exact counts."""
    import dataclasses

    lo = pkg.solve(dataclasses.replace(p, rtol=p.rtol * (1 - 1e-3)), "cpu", keep_solution=False, **data)
    hi = pkg.solve(dataclasses.replace(p, rtol=p.rtol * (1 + 1e-3)), "cpu", keep_solution=False, **data)
    assert lo.iters == hi.iters, f"rtol {p.rtol} grazes the threshold at {p.M}x{p.N}: {lo.iters} vs {hi.iters}"
    r = pkg.solve(p, "cpu", **data)
    assert r.iters == lo.iters and r.converged
    return r


# ---- validation -------------------------------------------------------------------------------------

@pytest.mark.parametrize("kw", [dict(stop="resid"), dict(stop=1), dict(rtol=-1e-8), dict(rtol=float("nan")),
                                dict(rtol=float("inf")), dict(atol=-1.0), dict(atol=float("nan")),
                                dict(atol=float("inf")), dict(rtol="tight")])
def test_bad_arguments_raise(pkg, kw):
    with pytest.raises(ValueError):
        pkg.PoissonEllipse(**kw)


@pytest.mark.parametrize("field,value", [("rtol", -1e-8), ("rtol", float("nan")), ("rtol", float("inf")),
                                         ("atol", -1.0), ("atol", float("nan")), ("atol", float("inf"))])
def test_native_validate_raises(native, field, value):
    s = native.ProblemSpec()
    s.stop = native.StopRule.residual
    s.validate()
    setattr(s, field, value)
    with pytest.raises(Exception, match=field):
        s.validate()


def test_to_native_round_trip(pkg, native):
    d = pkg.PoissonEllipse().to_native()
    assert d.stop == native.StopRule.step and d.rtol == 1e-8 and d.atol == 0.0
    s = pkg.PoissonEllipse(stop="residual", rtol=3e-7, atol=2e-12).to_native()
    assert s.stop == native.StopRule.residual and s.rtol == 3e-7 and s.atol == 2e-12
    s.validate()


def test_step_rule_reports_no_residual(pkg):
    r = pkg.solve(pkg.PoissonEllipse(M=40, N=40), "cpu")
    assert r.iters == 50 and "residual" not in r.extra


# ---- agreement across the CPU backends ---------------------------------------------------------------

@pytest.mark.parametrize("data", ["const", "manufactured"])
@pytest.mark.parametrize("grid,rtol", sorted(COUNTS))
def test_backends_agree(pkg, grid, rtol, data):
    p = problem(pkg, grid, rtol)
    kw = {} if data == "const" else dict(rhs=manufactured(p)[0])
    ref = oracle_count(pkg, p, **kw)
    assert ref.iters == COUNTS[(grid, rtol)][data == "manufactured"]
    assert ref.extra["residual"] <= rtol * ref.extra["residual_ref"]
    runs = {"omp": pkg.solve(p, "omp", threads=3, **kw), "torch": pkg.solve(p, "torch", **kw)}
    for ranks in (2, 4):
        for split in ("reference", "rows"):
            runs[f"dec{ranks}{split}"] = pkg.solve(p, "cpu-decomposed", ranks=ranks, split=split, **kw)
    ss = sub("models.sstep_pcg")
    for s in (2, 3):
        runs[f"sstep{s}"] = ss.TorchSStepPCG(p, s=s).solve(**kw)
    scale = np.abs(ref.w).max()
    for name, r in runs.items():
        err = np.abs(np.asarray(r.w) - ref.w).max()
        print(f"{grid} rtol {rtol} {data} {name}: iters {r.iters} (oracle {ref.iters}), max|dw| {err:.3e}")
        assert r.iters == ref.iters and r.status == "converged", name
        assert err <= 1e-10 * scale, name
        assert r.extra["residual_ref"] == pytest.approx(ref.extra["residual_ref"], rel=1e-12), name


# ---- scale covariance --------------------------------------------------------------------------------

@pytest.mark.parametrize("backend", ["cpu", "torch"])
def test_scale_covariance(pkg, backend):
    """f scaled by 2^20: the same count and bitwise 2^20 times the solution (a power of two commutes with
    every rounding); under the step rule the scaled solve needs strictly more iterations."""
    p = problem(pkg, (40, 40), 1e-8)
    f = manufactured(p)[0]
    a, b = pkg.solve(p, backend, rhs=f), pkg.solve(p, backend, rhs=f * 2.0 ** 20)
    assert a.iters == b.iters == COUNTS[((40, 40), 1e-8)][1] and a.converged and b.converged
    assert (a.w * 2.0 ** 20).tobytes() == b.w.tobytes()
    assert b.extra["residual"] == a.extra["residual"] * 2.0 ** 20
    step = pkg.PoissonEllipse(M=40, N=40)
    assert pkg.solve(step, backend, rhs=f * 2.0 ** 20).iters > pkg.solve(step, backend, rhs=f).iters


# ---- warm start, zero data, the reference norm -----------------------------------------------------------

@pytest.fixture(scope="module")
def tight(pkg):
    """The manufactured problem at 40x40 solved to rtol 1e-10, once."""
    p = problem(pkg, (40, 40), 1e-10)
    f = manufactured(p)[0]
    return f, pkg.solve(p, "cpu", rhs=f)


def _masked_interior(p, w0):
    out = np.zeros_like(w0)
    out[1:-1, 1:-1] = w0[1:-1, 1:-1]
    return out


@pytest.mark.parametrize("backend,kw", [("cpu", {}), ("omp", dict(threads=3)), ("cpu-decomposed", dict(ranks=4)),
                                        ("torch", {})])
def test_warm_start_good_enough_takes_no_iteration(pkg, tight, backend, kw):
    f, sol = tight
    p = problem(pkg, (40, 40), 1e-6)
    r = pkg.solve(p, backend, rhs=f, w0=sol.w, **kw)
    assert r.status == "converged" and r.iters == 0
    assert np.asarray(r.w).tobytes() == _masked_interior(p, sol.w).tobytes()
    assert r.extra["residual"] <= 1e-6 * r.extra["residual_ref"]
    # the same start on twice the data is not good enough
    r2 = pkg.solve(p, backend, rhs=2.0 * f, w0=sol.w, **kw)
    assert r2.converged and r2.iters > 0


@pytest.mark.parametrize("backend", ["cpu", "cpu-decomposed", "torch"])
def test_zero_data_converges_at_once(pkg, backend):
    p = problem(pkg, (40, 40))
    z = np.zeros((41, 41))
    r = pkg.solve(p, backend, rhs=z, w0=z)
    assert r.status == "converged" and r.iters == 0 and not np.asarray(r.w).any()
    cold = pkg.solve(p, backend, rhs=z)
    assert cold.status == "converged" and cold.iters == 0
    # the step rule still meets the breakdown guard there, as before
    assert pkg.solve(pkg.PoissonEllipse(M=40, N=40), backend, rhs=z).status == "breakdown"


@pytest.mark.parametrize("backend,kw", [("cpu", {}), ("cpu-decomposed", dict(ranks=4)), ("torch", {})])
def test_reference_norm_is_relative_to_the_data(pkg, tight, backend, kw):
    f, sol = tight
    p = problem(pkg, (40, 40), 1e-12)
    cold = pkg.solve(p, backend, rhs=f, **kw)
    warm = pkg.solve(p, backend, rhs=f, w0=0.5 * sol.w, **kw)
    assert warm.extra["residual_ref"] == pytest.approx(cold.extra["residual_ref"], rel=1e-14)
    # ... and not to the warm start's own rho_0: w0 = u/2 halves the residual
    r0 = pkg.solve(problem(pkg, (40, 40), 1e-12, max_iter=0), backend, rhs=f, w0=0.5 * sol.w, **kw)
    assert r0.iters == 0 and r0.status == "max_iter"
    assert r0.extra["residual"] == pytest.approx(0.5 * cold.extra["residual_ref"], rel=1e-6)
    assert r0.extra["residual_ref"] == pytest.approx(cold.extra["residual_ref"], rel=1e-14)


def test_default_breakdown_guard_fires_first(pkg):
    """What the README warns of: with the reference's absolute guard |(A p, p)| < 1e-15 left at its default,
    rtol 1e-8 is not reached for f = 1 at 40x40 -- breakdown after 75 iterations, 1.6e-6 of the data's norm."""
    r = pkg.solve(pkg.PoissonEllipse(M=40, N=40, stop="residual", rtol=1e-8), "cpu")
    assert r.status == "breakdown" and r.iters == 75
    assert 1e-6 < r.extra["residual"] / r.extra["residual_ref"] < 2e-6


def test_atol_alone(pkg):
    """rtol = 0: the absolute bound decides, and sqrt(rho) ends below it."""
    p = problem(pkg, (40, 40), 0.0, atol=1e-7)
    r = pkg.solve(p, "cpu")
    assert r.converged and 0 < r.iters < 100 and r.extra["residual"] <= 1e-7


# ---- the error regression the rule exists for -----------------------------------------------------------

def prolong(w):
    """Bilinear prolongation of a (m+1) x (n+1) nodal field to the grid with twice the cells."""
    m, n = w.shape[0] - 1, w.shape[1] - 1
    out = np.zeros((2 * m + 1, 2 * n + 1))
    out[::2, ::2] = w
    out[1::2, ::2] = 0.5 * (w[:-1, :] + w[1:, :])
    out[:, 1::2] = 0.5 * (out[:, :-1:2] + out[:, 2::2])
    return out


def test_warm_start_error_at_400x600(pkg):
    """w0 = the prolongation of the solved 200x300 problem.  Under the residual rule (rtol 1e-8) the warm solve
    reaches the cold solve's L2 error to 1%; under the step rule (delta 1e-6) it stops > 30% short."""
    def l2(p, w):
        return p.error_norms(w)["l2_error"]

    res_c, res_f = problem(pkg, (200, 300)), problem(pkg, (400, 600))
    w0 = prolong(pkg.solve(res_c, "cpu").w)
    cold, warm = pkg.solve(res_f, "cpu"), pkg.solve(res_f, "cpu", w0=w0)
    e_cold, e_warm = l2(res_f, cold.w), l2(res_f, warm.w)
    print(f"residual rule: cold {cold.iters} it, L2 {e_cold:.4e}; warm {warm.iters} it, L2 {e_warm:.4e}")
    assert cold.converged and warm.converged
    assert abs(e_warm - e_cold) <= 0.01 * e_cold
    st_c, st_f = pkg.PoissonEllipse(M=200, N=300), pkg.PoissonEllipse(M=400, N=600)
    w0 = prolong(pkg.solve(st_c, "cpu").w)
    cold, warm = pkg.solve(st_f, "cpu"), pkg.solve(st_f, "cpu", w0=w0)
    e_cold, e_warm = l2(st_f, cold.w), l2(st_f, warm.w)
    print(f"step rule: cold {cold.iters} it, L2 {e_cold:.4e}; warm {warm.iters} it, L2 {e_warm:.4e}")
    assert cold.iters == 546 and e_warm > 1.3 * e_cold


# ---- BackwardEuler and the refusals that need no GPU ----------------------------------------------------

def test_backward_euler_passes_the_rule_through(pkg):
    p = problem(pkg, (40, 40), 1e-8)
    be = sub("models.timestep").BackwardEuler(p, 0.01, backend="cpu")
    assert be.problem.stop == "residual" and be.problem.rtol == 1e-8
    u = pkg.solve(p, "cpu").w
    u1 = be.step(u)
    assert be.last["status"] == "converged" and be.last["iters"] > 0
    assert be.last["residual"] <= 1e-8 * be.last["residual_ref"]
    assert np.isfinite(u1).all()


def test_torch_orchestrated_dist_solver_refuses(pkg):
    dist = sub("parallel.dist_solver")
    with pytest.raises(ValueError, match="residual"):
        dist.DistGpuPCG(problem(pkg, (40, 40)), None, comm="torch")


# ---- CLI ------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def pmx_bin(pkg):
    exe = os.path.join(BIN, "pmx")
    if not os.path.exists(exe):
        sub("utils.build").build()
    return exe


def _run(args):
    p = subprocess.run(args, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr
    return p.stdout


def test_cli_names_the_rule(pkg, pmx_bin):
    ref = oracle_count(pkg, problem(pkg, (40, 40), 1e-8))
    flags = ["--stop", "residual", "--rtol", "1e-8", "--breakdown-tol", "0"]
    out = _run([pmx_bin, "40", "40", "--backend", "cpu", "--ranks", "4"] + flags).splitlines()
    assert out[1].startswith(f"Converged after {ref.iters} iterations (stop=residual")
    assert "rtol=1e-08" in out[1] and "atol=0" in out[1]
    assert out[2].startswith(f"M=40, N=40 | Iter={ref.iters} | Time=")
    one = _run([pmx_bin, "40", "40", "--backend", "cpu", "--json"] + flags)
    assert f"Converged after {ref.iters} iterations (stop=residual" in one
    j = json.loads(one.strip().splitlines()[-1])
    assert j["iters"] == ref.iters and j["stop"] == "residual" and j["rtol"] == 1e-8 and j["atol"] == 0


def test_cli_default_output_is_unchanged(pmx_bin):
    """Without the flags (and with --stop step) every line is the parent's; only the time differs."""
    want = ["Pure MPI 2D run with 4 processes; M=40, N=40",
            "Converged after 50 iterations (||w(k+1)-w(k)|| < 1e-06).",
            "M=40, N=40 | Iter=50 | Time=X s"]
    for extra in ([], ["--stop", "step"], ["--rtol", "1e-3", "--atol", "1"]):
        out = _run([pmx_bin, "40", "40", "--backend", "cpu", "--ranks", "4"] + extra)
        assert re.sub(r"Time=[0-9.]+ s", "Time=X s", out).splitlines() == want
    js = json.loads(_run([pmx_bin, "40", "40", "--backend", "cpu", "--json"]).strip().splitlines()[-1])
    assert "stop" not in js and "rtol" not in js and js["iters"] == 50


def test_cli_rejects_a_bad_rule(pmx_bin):
    p = subprocess.run([pmx_bin, "40", "40", "--backend", "cpu", "--stop", "energy"], capture_output=True, text=True)
    assert p.returncode != 0 and "--stop" in p.stderr


def test_pmx_mpi_takes_and_checks_the_rule(pkg, pmx_bin):
    """pmx_mpi: the oracle's count under the rule on 2 ranks, and a misspelt rule is an error, not the step rule."""
    from test_cli import _mpiexec

    exe = os.path.join(BIN, "pmx_mpi")
    if not os.path.exists(exe):
        pytest.skip("pmx_mpi not built (no MPI found at build time)")
    ref = oracle_count(pkg, problem(pkg, (40, 40), 1e-8))
    out = _run([_mpiexec(), "-n", "2", exe, "40", "40", "--stop", "residual", "--rtol", "1e-8", "--breakdown-tol", "0"])
    assert f"Converged after {ref.iters} iterations (stop=residual" in out
    bad = subprocess.run([_mpiexec(), "-n", "2", exe, "40", "40", "--stop", "residul"], capture_output=True, text=True,
                         timeout=120)
    assert bad.returncode != 0 and "--stop" in bad.stderr and "Converged" not in bad.stdout
