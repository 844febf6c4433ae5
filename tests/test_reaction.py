"""A reaction field c(x, y) >= 0: (-Δ + σ + c) u = f on the CPU paths -- the native oracle (serial, OpenMP,
decomposed), the plain-PyTorch PCG, the operator apply, the refusals -- and SemilinearNewton on top.

Fields, as functions of the node coordinates: smooth = 50 (1 + x)^2 + 200 y^2; disc = 1e6 inside the disc of
radius 0.15 about (0.3, 0.1), else 0; random = uniform [0, 1e3], seeded.
"""
import numpy as np
import pytest
import torch

from conftest import sub
from test_init_data import manufactured

GRIDS = [(40, 40), (97, 130)]


def fields(p):
    x, y = p.coords()
    X, Y = np.meshgrid(x, y, indexing="ij")
    return dict(smooth=50.0 * (1.0 + X) ** 2 + 200.0 * Y * Y,
                disc=np.where((X - 0.3) ** 2 + (Y - 0.1) ** 2 < 0.15 ** 2, 1e6, 0.0),
                random=np.random.default_rng(11).uniform(0.0, 1e3, size=X.shape))


def host_apply(p, x, c):
    """(A + (σ + c) I) x on the interior with ops/reference.py (a tensor for sigma), 0 on the boundary."""
    R = sub("ops.reference")
    sd = sub("parallel.decomp").subdomain(p.M, p.N, 1, 1, 0)
    a, b, _ = R.assemble(p, sd)
    xg = torch.as_tensor(x).clone()
    for edge in (xg[0, :], xg[-1, :], xg[:, 0], xg[:, -1]):
        edge.zero_()
    out = np.zeros_like(x)
    out[1:-1, 1:-1] = R.apply_A(xg, a, b, p.h1, p.h2, torch.as_tensor(p.sigma + c[1:-1, 1:-1])).numpy()
    return out


@pytest.fixture(scope="module")
def oracle(pkg):
    """Serial oracle solves shared by the tests: per grid and field, the constant right-hand side."""
    out = {}
    for grid in GRIDS:
        p = pkg.PoissonEllipse(M=grid[0], N=grid[1])
        for name, c in fields(p).items():
            out[(grid, name)] = dict(p=p, c=c, r=pkg.solve(p, "cpu", reaction=c))
            assert out[(grid, name)]["r"].converged
    return out


@pytest.mark.parametrize("s", [1.0, 1e4])
@pytest.mark.parametrize("backend,kw", [("cpu", {}), ("cpu-decomposed", dict(ranks=4))])
def test_constant_field_is_the_sigma_solve_bitwise(pkg, backend, kw, s):
    p0 = pkg.PoissonEllipse(M=97, N=130)
    f, _ = manufactured(p0)
    want = pkg.solve(pkg.PoissonEllipse(M=97, N=130, sigma=s), backend, rhs=f, **kw)
    got = pkg.solve(p0, backend, rhs=f, reaction=np.full((98, 131), s), **kw)
    assert got.iters == want.iters and got.status == want.status == "converged"
    assert got.w.tobytes() == want.w.tobytes()
    # and a field really changes the solve
    other = pkg.solve(p0, backend, rhs=f, reaction=fields(p0)["smooth"], **kw)
    assert np.abs(other.w - want.w).max() > 1e-3 * np.abs(want.w).max()


def test_boundary_values_are_ignored(pkg):
    """NaN, inf and negative values on the box boundary change nothing: they are never read."""
    p = pkg.PoissonEllipse(M=40, N=40)
    c = fields(p)["smooth"]
    d = c.copy()
    d[0, :], d[-1, :], d[:, 0], d[:, -1] = np.nan, np.inf, -1.0, np.nan
    for backend in ("cpu", "cpu-decomposed", "torch"):
        a, b = pkg.solve(p, backend, reaction=c), pkg.solve(p, backend, reaction=d)
        assert a.iters == b.iters and a.w.tobytes() == b.w.tobytes()
    x = np.random.default_rng(3).standard_normal((41, 41))
    assert p.apply(x, reaction=c).tobytes() == p.apply(x, reaction=d).tobytes()


@pytest.mark.parametrize("name", ["smooth", "disc", "random"])
@pytest.mark.parametrize("grid", GRIDS)
def test_oracle_paths_agree(pkg, oracle, grid, name):
    """cpu against omp and cpu-decomposed (reference split and row strips), and against torch: the same
    iteration count, w to 1e-10 max|w|."""
    o = oracle[(grid, name)]
    top = np.abs(o["r"].w).max()
    runs = [("omp", dict(threads=4)), ("cpu-decomposed", dict(ranks=4)), ("cpu-decomposed", dict(ranks=3, split="rows")),
            ("torch", {})]
    for backend, kw in runs:
        r = pkg.solve(o["p"], backend, reaction=o["c"], **kw)
        err = np.abs(r.w - o["r"].w).max()
        print(f"{grid} {name} {backend} {kw}: iters {r.iters} (cpu {o['r'].iters}) max|w - w_cpu| {err:.3e}")
        assert r.iters == o["r"].iters and r.status == "converged"
        assert err <= 1e-10 * top


def test_sigma_adds_to_the_field(pkg):
    """sigma = 3.5 plus a field is the field + 3.5 at sigma = 0, with rhs and w0, under the residual rule."""
    kw = dict(M=40, N=40, stop="residual", rtol=1e-9, breakdown_tol=0.0)  # the guard fires before a tight rtol
    p, p0 = pkg.PoissonEllipse(sigma=3.5, **kw), pkg.PoissonEllipse(**kw)
    c = fields(p)["random"]
    f, u = manufactured(p)
    a = pkg.solve(p, "cpu", rhs=f, w0=0.5 * u, reaction=c)
    b = pkg.solve(p0, "cpu", rhs=f, w0=0.5 * u, reaction=c + 3.5)
    assert a.iters == b.iters and a.status == "converged"
    assert np.abs(a.w - b.w).max() <= 1e-13 * np.abs(a.w).max()
    assert a.extra["residual_ref"] == pytest.approx(b.extra["residual_ref"], rel=1e-13)


@pytest.mark.parametrize("sigma", [0.0, 3.5])
@pytest.mark.parametrize("name", ["smooth", "disc", "random"])
def test_apply_agrees_with_the_reference_ops(pkg, name, sigma):
    """PoissonEllipse.apply(x, reaction=c) against ops/reference.py fed the shift as a tensor.  Both evaluate the
    reference's expression in fp64, so they agree to a few roundings of the largest term: 8 eps max|Lx|."""
    p = pkg.PoissonEllipse(M=33, N=70, sigma=sigma)
    c = fields(p)[name]
    x = np.random.default_rng(5).standard_normal((34, 71))
    got = p.apply(x, reaction=c)
    want = host_apply(p, x, c)
    err = np.abs(got - want).max()
    print(f"{name} sigma {sigma}: max|apply - reference| {err:.3e}, max|Lx| {np.abs(want).max():.3e}")
    assert err <= 8 * np.finfo(float).eps * np.abs(want).max()
    assert not got[0, :].any() and not got[-1, :].any() and not got[:, 0].any() and not got[:, -1].any()
    plain = p.apply(x)
    assert np.abs(got - plain).max() > 1e-6 * np.abs(plain).max()  # the field is in it
    # the combination: alpha L x + beta x + gamma y + const, as without a field
    y = np.random.default_rng(6).standard_normal((34, 71))
    comb = p.apply(x, alpha=-0.5, beta=2.0, y=y, gamma=3.0, const=0.25, reaction=c)
    ref = -0.5 * got + 2.0 * x + 3.0 * y + 0.25
    assert np.abs(comb - ref)[1:-1, 1:-1].max() <= 8 * np.finfo(float).eps * np.abs(ref).max()


def test_refusals(pkg):
    p = pkg.PoissonEllipse(M=40, N=40)
    c = fields(p)["smooth"]
    bad = {}
    for key, v in (("nan", np.nan), ("inf", np.inf), ("negative", -1e-3)):
        bad[key] = c.copy()
        bad[key][7, 9] = v
    for backend in ("cpu", "omp", "cpu-decomposed", "torch"):
        for key, field in bad.items():
            with pytest.raises(ValueError, match="reaction"):
                pkg.solve(p, backend, reaction=field)
        with pytest.raises(ValueError, match="shape"):
            pkg.solve(p, backend, reaction=c[:-1])
        with pytest.raises(ValueError, match="float64"):
            pkg.solve(p, backend, reaction=c.astype(np.float32))
        with pytest.raises(ValueError, match="reaction"):
            pkg.solve(p, backend, reaction=[[0.0]])
    for key, field in bad.items():
        with pytest.raises(ValueError, match="reaction"):
            p.apply(c, reaction=field)
    with pytest.raises(ValueError, match="reaction"):
        sub("models.sstep_pcg").TorchSStepPCG(p, reaction=c)
    with pytest.raises(ValueError, match="reaction"):
        sub("ops.kernels").DeviceOps(p, reaction=c)
    with pytest.raises(ValueError, match="reaction"):
        sub("parallel.dist_solver").DistGpuPCG(p, None, comm="torch", reaction=c)
    with pytest.raises(ValueError, match="reaction"):
        sub("parallel.dist_solver").DistGpuPCG(p, None, comm="native", reaction=c)
    with pytest.raises(ValueError, match="reaction"):
        pkg.SemilinearNewton(p, np.sin, np.cos, backend="cpu", reaction=c)
    # the closed-form error does not hold: error_norms needs exact=, as with sigma
    w = pkg.solve(p, "cpu", reaction=c).w
    assert p.error_norms(w, exact=w)["max_error"] == 0.0


def test_time_steppers_take_the_field(pkg):
    """BackwardEuler / ThetaScheme with reaction= in session_kw on the cpu backend: theta = 1 is BackwardEuler
    bitwise, one BackwardEuler step is the solve with the field and sigma = 1/dt, and the theta-scheme's
    right-hand side includes c."""
    p = pkg.PoissonEllipse(M=40, N=40)
    c = fields(p)["smooth"]
    _, u = manufactured(p)
    dt = 1e-3
    be = pkg.BackwardEuler(p, dt, backend="cpu", reaction=c)
    v = be.step(u, 1.0)
    want = pkg.solve(pkg.PoissonEllipse(M=40, N=40, sigma=1.0 / dt), "cpu", rhs=u / dt + 1.0, w0=u, reaction=c).w
    assert v.tobytes() == want.tobytes()
    assert pkg.ThetaScheme(p, dt, theta=1.0, backend="cpu", reaction=c).step(u, 1.0).tobytes() == v.tobytes()
    cn = pkg.ThetaScheme(p, dt, theta=0.5, backend="cpu", reaction=c)
    rhs = cn.rhs(u, 1.0)
    L = cn.problem.apply(u, reaction=c)
    ref = -L + 2.0 * cn.s * u + 2.0
    assert np.abs(rhs - ref)[1:-1, 1:-1].max() <= 8 * np.finfo(float).eps * np.abs(ref).max()
    assert np.abs(rhs - pkg.ThetaScheme(p, dt, theta=0.5, backend="cpu").rhs(u, 1.0)).max() > 1.0
    w = cn.step(u, 1.0)
    assert cn.last["status"] == "converged" and np.isfinite(w).all()


def newton_problem(pkg, grid=(97, 130)):
    """-Δu + 50 u^3 = f with the manufactured u = (1 - x^2 - 4y^2)(1 + x/2 + y): f = 10 + 7x + 26y + 50 u^3.  The
    linear solves run to rtol = 1e-12 of their data (breakdown guard off), far below newton_rtol."""
    p = pkg.PoissonEllipse(M=grid[0], N=grid[1], stop="residual", rtol=1e-12, breakdown_tol=0.0)
    f0, u = manufactured(p)
    return p, f0, u


def g3(u):
    return 50.0 * u ** 3


def dg3(u):
    return 150.0 * u ** 2


def error_in_D(p, w, u):
    return float(np.abs(np.where(p.inside_mask(), w - u, 0.0)).max())


NEWTON_STEPS = 7  # measured on the cpu backend at 97 x 130 (test_semilinear_newton_cpu); the GPU test pins it too


def newton_start(pkg, p, f):
    """The start of the Newton tests: the solution of the linear problem -Δu = f (g dropped).  From u0 = 0 the
    first undamped step IS that solve and overshoots (the residual rises 40.8 -> 1418 at 97 x 130), so no
    undamped Newton history from 0 is monotone; from the linear solution the iterates fall to u (g is convex
    on u >= 0) and so do the residuals."""
    return pkg.solve(p, "cpu", rhs=f).w


def test_semilinear_newton_cpu(pkg):
    """Manufactured semilinear problem at 97 x 130, started from the linear solve (newton_start): the residual
    history falls monotonically to newton_rtol = 1e-8; the error against u is within 2x that of the linear
    problem (g = 0) on the same grid, since the discretisation dominates.  Measured: 7 Newton steps, residuals
    1.418e+03 4.133e+02 1.151e+02 2.730e+01 3.883e+00 1.348e-01 1.908e-04 1.078e-09."""
    p, f0, u = newton_problem(pkg)
    f = f0 + g3(u)
    nw = pkg.SemilinearNewton(p, g3, dg3, backend="cpu", newton_rtol=1e-8)
    w = nw.solve(f, u0=newton_start(pkg, p, f))
    print(f"steps {nw.steps}, history {['%.3e' % h for h in nw.history]}")
    assert nw.converged and nw.steps == len(nw.history) - 1
    assert all(b < a for a, b in zip(nw.history, nw.history[1:]))
    assert nw.history[-1] <= 1e-8 * nw.history[0]
    lin = pkg.solve(p, "cpu", rhs=f0).w
    e_lin, e_new = error_in_D(p, lin, u), error_in_D(p, w, u)
    print(f"max error in D: linear {e_lin:.3e}, semilinear {e_new:.3e}")
    assert e_new <= 2.0 * e_lin
    assert nw.steps == NEWTON_STEPS
    # g = 0 is the linear problem: one step from 0, then the residual of the solve
    zero = pkg.SemilinearNewton(p, lambda v: 0.0 * v, lambda v: 0.0 * v, backend="cpu")
    assert np.abs(zero.solve(f0) - lin).max() <= 1e-12 * np.abs(lin).max() and zero.steps == 1


@pytest.mark.parametrize("dtype", ["fp64", "fp32"])
@pytest.mark.parametrize("grid,world,split", [((40, 40), 1, "reference"), ((97, 130), 4, "reference"),
                                              ((97, 130), 3, "rows"), ((400, 600), 1, "reference")])
def test_memory_plan_shift_field(pkg, grid, world, split, dtype):
    """The shift field of a reaction session: one more field behind the five of pcg1, with their pitch and ghost
    layers -- column 1 of every row 256-B aligned, rows -1 .. nx+2 and the vector loads' reach inside its own
    field_bytes (no overlap with r2 before it or the end of the allocation) -- and every plan without it unchanged."""
    n = pkg.load_native()
    spec = pkg.PoissonEllipse(M=grid[0], N=grid[1]).to_native()
    for rank in range(world):
        a = n.memory_plan(spec, world, getattr(n.Split, split), rank, dtype, False)
        b = n.memory_plan(spec, world, getattr(n.Split, split), rank, dtype, True)
        assert a["shift_field"] == -1 and a["nfields"] == 5 and a["fields_total"] == 5 * a["field_bytes"]
        assert b["shift_field"] == 5 and b["fields_total"] == 6 * b["field_bytes"]
        assert b["total"] - a["total"] == a["field_bytes"]
        for key in ("elem", "pitch", "gh", "field_bytes", "nfields"):
            assert a[key] == b[key]
        assert a["at"] == b["at"][:5]
        e, P, fb = b["elem"], b["pitch"], b["field_bytes"]
        assert b["gh"] == 2 and P >= b["ny"] + 2 + 8
        for f in range(6):
            lo, hi = f * fb, (f + 1) * fb
            origin = b["at"][f]
            assert (origin + e) % 256 == 0 and (P * e) % 256 == 0  # column 1 of every row
            first = origin + (-1 * P - 2) * e            # row -1, column -2 (col_ptr's base)
            last = origin + ((b["nx"] + 2) * P + b["ny"] + 3) * e  # row nx+2, the last column a clamped chunk reads
            assert lo <= first and last + e <= hi
