"""The screened problem (-Δ + σ) u = f on the CPU paths: the native oracle (serial, decomposed), the
plain-PyTorch PCG, the error contracts and the CLI.

Manufactured problem on the reference ellipse: u = (1 - x^2 - 4y^2)(1 + x/2 + y) in D, u = 0 on its
boundary, so (-Δ + σ) u = f = 10 + 7x + 26y + σ u.
"""
import json
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT, sub
from test_init_data import manufactured

SIGMAS = [1.0, 100.0, 1e4]
GRID = (97, 130)


def problem(pkg, sigma, grid=GRID, **kw):
    return pkg.PoissonEllipse(M=grid[0], N=grid[1], sigma=sigma, **kw)


def screened(p):
    """(f, u) of the manufactured problem with p's sigma."""
    f0, u = manufactured(p)
    return f0 + p.sigma * u, u


def error_in_D(p, w, u):
    e = np.where(p.inside_mask(), w - u, 0.0)
    return float(np.sqrt((e * e).sum() * p.h1 * p.h2)), float(np.abs(e).max())


@pytest.fixture(scope="module")
def oracle(pkg):
    """Serial oracle solves of the manufactured problem at 97 x 130, once per sigma (0 included)."""
    out = {}
    for sigma in [0.0] + SIGMAS:
        p = problem(pkg, sigma)
        f, u = screened(p)
        out[sigma] = dict(p=p, f=f, u=u, r=pkg.solve(p, "cpu", rhs=f))
        assert out[sigma]["r"].converged
    return out


@pytest.mark.parametrize("backend,grid", [("cpu", (40, 40)), ("cpu", GRID), ("torch", (40, 40))])
def test_sigma_zero_is_the_default_solve(pkg, backend, grid):
    plain = pkg.solve(pkg.PoissonEllipse(M=grid[0], N=grid[1]), backend)
    zero = pkg.solve(problem(pkg, 0.0, grid), backend)
    assert zero.iters == plain.iters and zero.status == plain.status == "converged"
    assert zero.w.tobytes() == plain.w.tobytes()
    assert pkg.PoissonEllipse().to_native().sigma == 0.0


@pytest.mark.parametrize("sigma", SIGMAS)
def test_oracle_and_torch_agree(pkg, oracle, sigma):
    o = oracle[sigma]
    t = sub("models.torch_pcg").TorchPCG(o["p"]).solve(rhs=o["f"])
    err = np.abs(t.w - o["r"].w).max()
    print(f"sigma {sigma}: iters cpu {o['r'].iters} torch {t.iters}, max|w_cpu - w_torch| {err:.3e}")
    assert t.iters == o["r"].iters and t.status == "converged"
    assert err <= 1e-10 * np.abs(o["r"].w).max()


@pytest.mark.parametrize("sigma", SIGMAS)
def test_error_falls_with_the_mesh(pkg, oracle, sigma):
    """Monotonicity only: the error against u at 194 x 260 is below the one at 97 x 130."""
    coarse = error_in_D(oracle[sigma]["p"], oracle[sigma]["r"].w, oracle[sigma]["u"])
    p = problem(pkg, sigma, (194, 260))
    f, u = screened(p)
    fine = error_in_D(p, pkg.solve(p, "cpu", rhs=f).w, u)
    print(f"sigma {sigma}: (L2, max) error 97x130 {coarse}, 194x260 {fine}")
    assert fine[0] < coarse[0] and fine[1] < coarse[1]
    # error_norms(w, exact=u) is the same measure and works with sigma != 0
    e = oracle[sigma]["p"].error_norms(oracle[sigma]["r"].w, exact=oracle[sigma]["u"])
    assert e["l2_error"] == pytest.approx(coarse[0], rel=1e-12) and e["max_error"] == coarse[1]


def test_the_shift_improves_the_conditioning(oracle):
    print({s: o["r"].iters for s, o in oracle.items()})
    assert oracle[1e4]["r"].iters < oracle[0.0]["r"].iters


@pytest.mark.parametrize("ranks", [2, 4])
@pytest.mark.parametrize("sigma", SIGMAS)
def test_decomposed_oracle(pkg, oracle, sigma, ranks):
    o = oracle[sigma]
    d = pkg.solve(o["p"], "cpu-decomposed", ranks=ranks, rhs=o["f"])
    assert d.iters == o["r"].iters and d.status == "converged"
    assert np.abs(d.w - o["r"].w).max() <= 1e-10 * np.abs(o["r"].w).max()


def test_warm_start_uses_the_shifted_operator(pkg, oracle):
    """r^0 = B - (A + σ I) w0: restarting from the converged iterate stops at once, on every CPU path."""
    o = oracle[100.0]
    for backend, kw in (("cpu", {}), ("cpu-decomposed", dict(ranks=4)), ("torch", {})):
        again = pkg.solve(o["p"], backend, rhs=o["f"], w0=o["r"].w, **kw)
        assert again.iters == 1 and again.status == "converged", backend


@pytest.mark.parametrize("bad", [-1.0, -1e-300, float("nan"), float("inf"), -float("inf"), "x", None])
def test_bad_sigma_raises(pkg, native, bad):
    with pytest.raises(ValueError, match="sigma"):
        pkg.PoissonEllipse(sigma=bad)
    if isinstance(bad, float):  # the native spec checks it too
        s = pkg.PoissonEllipse().to_native()
        s.sigma = bad
        with pytest.raises(native.PmxError, match="sigma"):
            s.validate()


def test_the_closed_form_is_for_sigma_zero(pkg):
    p = problem(pkg, 2.0, (40, 40))
    w = pkg.solve(p, "cpu").w
    x, y = p.coords()
    with pytest.raises(ValueError, match="sigma"):
        p.exact_solution(x[:, None], y[None, :])
    with pytest.raises(ValueError, match="sigma"):
        p.error_norms(w)
    t = sub("models.torch_pcg").TorchPCG(p)
    t.init()
    with pytest.raises(ValueError, match="sigma"):
        t.local_error_stats()
    assert p.error_norms(w, exact=np.zeros_like(w))["max_error"] == np.abs(np.where(p.inside_mask(), w, 0)).max()
    assert pkg.PoissonEllipse(M=40, N=40).error_norms(pkg.solve(pkg.PoissonEllipse(M=40, N=40), "cpu").w)["l2_error"] > 0


def test_python_orchestrated_paths_refuse_sigma(pkg):
    """DeviceOps, DistGpuPCG(comm="torch") and the s-step prototype evaluate the unshifted operator:
    ValueError before a device is touched."""
    p = problem(pkg, 3.0, (40, 40))
    with pytest.raises(ValueError, match="sigma"):
        sub("ops.kernels").DeviceOps(p)
    info = sub("parallel.launch").DistInfo(rank=0, world=1, local_rank=0, backend="gloo")
    with pytest.raises(ValueError, match="sigma"):
        sub("parallel.dist_solver").DistGpuPCG(p, info, comm="torch")
    with pytest.raises(ValueError, match="sigma"):
        sub("models.sstep_pcg").TorchSStepPCG(p)


def test_backward_euler_on_the_cpu(pkg):
    """step() is one oracle solve of (1/dt - Δ) u+ = u/dt + g from w0 = u; NumPy in and out."""
    p = pkg.PoissonEllipse(M=40, N=40)
    be = pkg.BackwardEuler(p, 1e-2, backend="cpu")
    assert be.problem.sigma == 100.0 and be.session is None
    u0 = np.zeros((41, 41))
    u1 = be.step(u0, g=1.0)
    want = pkg.solve(problem(pkg, 100.0, (40, 40)), "cpu", rhs=np.full((41, 41), 1.0), w0=u0)
    assert np.array_equal(u1, want.w) and be.last["iters"] == want.iters
    u2 = be.step(u1)  # no source: the solution decays
    assert 0 < u2.max() < u1.max()
    for bad in (0.0, -1.0, float("nan"), float("inf"), "1"):
        with pytest.raises(ValueError, match="dt"):
            pkg.BackwardEuler(p, bad, backend="cpu")


def test_cli_reports_sigma(pkg):
    exe = os.path.join(ROOT, "poisson-ellipse-openmp-mpi-cuda-new_amd", "bin", "pmx")
    if not os.path.exists(exe):
        sub("utils.build").build()
    want = pkg.solve(problem(pkg, 100.0, (40, 40)), "cpu")

    def run(*extra):
        r = subprocess.run([exe, "40", "40", "--backend", "cpu", "--json", *extra], capture_output=True, text=True,
                           timeout=300)
        assert r.returncode == 0, r.stderr
        return r.stdout.strip().splitlines()

    out = run("--sigma", "100")
    j = json.loads(out[-1])
    assert j["sigma"] == 100.0 and j["iters"] == want.iters and j["status"] == "converged"
    assert "l2_error" not in j and j["max_w"] == pytest.approx(want.w.max(), rel=1e-12)
    # sigma = 0: the reference-format lines and the error keys as without the option
    zero, plain = run("--sigma", "0"), run()
    untimed = lambda lines: [re.sub(r"Time\s*=\s*[0-9.]+", "Time=", l) for l in lines]  # noqa: E731
    assert untimed(zero[:-1]) == untimed(plain[:-1])
    jz = json.loads(zero[-1])
    assert jz["sigma"] == 0.0 and jz["iters"] == 50 and jz["l2_error"] == json.loads(plain[-1])["l2_error"]
    bad = subprocess.run([exe, "40", "40", "--backend", "cpu", "--sigma", "-1"], capture_output=True, text=True)
    assert bad.returncode != 0 and "sigma" in bad.stderr
