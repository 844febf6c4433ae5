"""A diffusion field k(x, y) > 0: (-∇·k∇ + σ + c) u = f on the CPU paths -- the native oracle (serial, OpenMP,
decomposed), the plain-PyTorch PCG, the operator apply, the refusals, the time steppers -- and QuasilinearPicard
on top.

The face coefficients are a[i,j] <- (0.5 (k[i-1,j] + k[i,j])) a[i,j], b[i,j] <- (0.5 (k[i,j-1] + k[i,j])) b[i,j].
Fields, as functions of the node coordinates: smooth = 1 + 0.5 sin(3x) cos(2y); jump = 100 inside the disc of
radius 0.2 about (0.3, 0.1), else 1; random = uniform [0.5, 2], seeded.
"""
import numpy as np
import pytest
import torch

from conftest import sub
from test_init_data import manufactured
from test_reaction import fields as reaction_fields

GRIDS = [(40, 40), (97, 130)]


def kappas(p):
    x, y = p.coords()
    X, Y = np.meshgrid(x, y, indexing="ij")
    return dict(smooth=1.0 + 0.5 * np.sin(3.0 * X) * np.cos(2.0 * Y),
                jump=np.where((X - 0.3) ** 2 + (Y - 0.1) ** 2 < 0.2 ** 2, 100.0, 1.0),
                random=np.random.default_rng(5).uniform(0.5, 2.0, size=X.shape))


def rhs_of(p, name):
    """The right-hand side that goes with a field: the manufactured one for smooth, the constant F otherwise."""
    return manufactured(p)[0] if name == "smooth" else None


def host_faces(p, k):
    """a, b of ops/reference.py (whole grid, with ghosts: (M+1) x (N+1) here) multiplied by the face means of k in
    NumPy -- the independent statement of the definition.  Row 0 of a and column 0 of b join no two nodes."""
    R = sub("ops.reference")
    sd = sub("parallel.decomp").subdomain(p.M, p.N, 1, 1, 0)
    a, b, _ = R.assemble(p, sd)
    a, b = a.numpy().copy(), b.numpy().copy()
    a[1:, :] = (0.5 * (k[:-1, :] + k[1:, :])) * a[1:, :]
    b[:, 1:] = (0.5 * (k[:, :-1] + k[:, 1:])) * b[:, 1:]
    return a, b


def host_apply(p, x, k, shift):
    """(A_k + shift I) x on the interior with ops/reference.py on host_faces, 0 on the boundary; shift: a number or
    an (M-1) x (N-1) array."""
    R = sub("ops.reference")
    a, b = host_faces(p, k)
    q = x.copy()
    q[0, :] = q[-1, :] = 0.0
    q[:, 0] = q[:, -1] = 0.0
    out = np.zeros_like(x)
    out[1:-1, 1:-1] = R.apply_A(q, a, b, p.h1, p.h2, shift)
    return out


def host_residual(p, w, rhs, k, shift):
    """sqrt((D^-1 r, r)) for r = B - (A_k + shift I) w and sqrt((D^-1 B, B)), B the masked rhs, in fp64 with
    ops/reference.py on host_faces; and sqrt(h1 h2 sum r^2)."""
    R = sub("ops.reference")
    a, b = host_faces(p, k)
    B = np.where(p.inside_mask(), rhs, 0.0)[1:-1, 1:-1]
    q = w.copy()
    q[0, :] = q[-1, :] = 0.0
    q[:, 0] = q[:, -1] = 0.0
    r = B - R.apply_A(q, a, b, p.h1, p.h2, shift)
    D = R.diag(a, b, p.h1, p.h2, shift)
    hh = p.h1 * p.h2
    return (float(np.sqrt((r * r / D).sum() * hh)), float(np.sqrt((B * B / D).sum() * hh)),
            float(np.sqrt((r * r).sum() * hh)))


@pytest.fixture(scope="module")
def oracle(pkg):
    """Serial oracle solves shared by the tests: per grid and field (manufactured rhs for smooth, else constant)."""
    out = {}
    for grid in GRIDS:
        p = pkg.PoissonEllipse(M=grid[0], N=grid[1])
        for name, k in kappas(p).items():
            f = rhs_of(p, name)
            out[(grid, name)] = dict(p=p, k=k, f=f, r=pkg.solve(p, "cpu", rhs=f, diffusion=k))
            assert out[(grid, name)]["r"].converged
    return out


@pytest.mark.parametrize("with_reaction", [False, True])
@pytest.mark.parametrize("sigma", [0.0, 3.5])
def test_oracle_against_the_independent_statement(pkg, sigma, with_reaction):
    """cpu_apply and the oracle's residuals (sqrt(rho_0) from a w0 and sqrt(rho_B), reported by a solve that stops
    at once) against ops/reference.py applied to faces multiplied in the test: 1e-12 relative."""
    p = pkg.PoissonEllipse(M=33, N=70, sigma=sigma, stop="residual", rtol=0.0, atol=1e300)
    k = kappas(p)["random"]
    c = reaction_fields(p)["random"] if with_reaction else None
    shift = sigma + c[1:-1, 1:-1] if with_reaction else sigma
    rng = np.random.default_rng(7)
    x = rng.standard_normal((34, 71))
    f = rng.standard_normal((34, 71))
    got = p.apply(x, diffusion=k, reaction=c)
    want = host_apply(p, x, k, shift)
    err = np.abs(got - want).max()
    print(f"sigma {sigma} reaction {with_reaction}: max|apply - reference| {err:.3e}, max|Lx| {np.abs(want).max():.3e}")
    assert err <= 1e-12 * np.abs(want).max()
    assert not got[0, :].any() and not got[-1, :].any() and not got[:, 0].any() and not got[:, -1].any()
    assert np.abs(got - p.apply(x, reaction=c)).max() > 1e-3 * np.abs(want).max()  # k is in it
    for backend, kw in (("cpu", {}), ("cpu-decomposed", dict(ranks=4)), ("torch", {})):
        r = pkg.solve(p, backend, rhs=f, w0=x, diffusion=k, reaction=c, **kw)
        assert r.iters == 0 and r.status == "converged"
        res, ref, _ = host_residual(p, x, f, k, shift)
        print(f"  {backend}: residual {r.extra['residual']:.16e} host {res:.16e}; ref {r.extra['residual_ref']:.16e} "
              f"host {ref:.16e}")
        assert abs(r.extra["residual"] - res) <= 1e-12 * res
        assert abs(r.extra["residual_ref"] - ref) <= 1e-12 * ref


@pytest.mark.parametrize("backend,kw", [("cpu", {}), ("omp", dict(threads=1)), ("cpu-decomposed", dict(ranks=4)),
                                        ("cpu-decomposed", dict(ranks=3, split="rows")), ("torch", {})])
def test_unit_field_is_the_plain_solve_bitwise(pkg, backend, kw):
    """k = 1 multiplies every face by exactly 1.0: the solve without the argument, bit for bit, with sigma, a
    reaction field, rhs and w0 next to it.  (omp with one thread: its reductions are order-dependent with more.)"""
    p = pkg.PoissonEllipse(M=97, N=130, sigma=3.5)
    f, u = manufactured(p)
    c = reaction_fields(p)["smooth"]
    one = np.ones((98, 131))
    want = pkg.solve(p, backend, rhs=f, w0=0.5 * u, reaction=c, **kw)
    got = pkg.solve(p, backend, rhs=f, w0=0.5 * u, reaction=c, diffusion=one, **kw)
    assert got.iters == want.iters and got.status == want.status == "converged"
    assert np.asarray(got.w).tobytes() == np.asarray(want.w).tobytes()
    x = np.random.default_rng(3).standard_normal((98, 131))
    assert p.apply(x, diffusion=one).tobytes() == p.apply(x).tobytes()
    # and a field really changes the solve
    other = pkg.solve(p, backend, rhs=f, w0=0.5 * u, reaction=c, diffusion=kappas(p)["smooth"], **kw)
    assert np.abs(other.w - want.w).max() > 1e-3 * np.abs(want.w).max()


@pytest.mark.parametrize("name", ["smooth", "jump", "random"])
@pytest.mark.parametrize("grid", GRIDS)
def test_oracle_paths_agree(pkg, oracle, grid, name):
    """cpu against omp and cpu-decomposed (reference split and row strips), and against torch: the same
    iteration count, w to 1e-10 max|w|."""
    o = oracle[(grid, name)]
    top = np.abs(o["r"].w).max()
    runs = [("omp", dict(threads=4)), ("cpu-decomposed", dict(ranks=4)),
            ("cpu-decomposed", dict(ranks=3, split="rows")), ("torch", {})]
    for backend, kw in runs:
        r = pkg.solve(o["p"], backend, rhs=o["f"], diffusion=o["k"], **kw)
        err = np.abs(r.w - o["r"].w).max()
        print(f"{grid} {name} {backend} {kw}: iters {r.iters} (cpu {o['r'].iters}) max|w - w_cpu| {err:.3e}")
        assert r.iters == o["r"].iters and r.status == "converged"
        assert err <= 1e-10 * top


@pytest.mark.parametrize("backend,kw", [("cpu", {}), ("cpu-decomposed", dict(ranks=4))])
def test_powers_of_two(pkg, backend, kw):
    """k = 2 with rhs f is k = 1 with rhs f / 2: scaling by 2 is exact, so the iterations are the same numbers up
    to the scale of r (the residual rule is scale-free; the breakdown guard is absolute, hence off)."""
    p = pkg.PoissonEllipse(M=97, N=130, stop="residual", rtol=1e-10, breakdown_tol=0.0)
    f, _ = manufactured(p)
    a = pkg.solve(p, backend, rhs=f, diffusion=np.full((98, 131), 2.0), **kw)
    b = pkg.solve(p, backend, rhs=0.5 * f, diffusion=np.ones((98, 131)), **kw)
    err = np.abs(a.w - b.w).max()
    print(f"{backend}: iters {a.iters} / {b.iters}, max|w_2 - w_1| {err:.3e}, max|w| {np.abs(b.w).max():.3e}")
    assert a.status == b.status == "converged" and a.iters == b.iters > 50
    assert err <= 1e-12 * np.abs(b.w).max()


def smooth_problem(p):
    """(f, u, k) of the manufactured variable-coefficient problem: u = (1 - x^2 - 4y^2)(1 + x/2 + y) in D,
    k = smooth, f = -(k Δu + ∇k·∇u) in closed form (Δu = -(10 + 7x + 26y))."""
    x, y = p.coords()
    X, Y = np.meshgrid(x, y, indexing="ij")
    g, h = 1.0 - X * X - 4.0 * Y * Y, 1.0 + 0.5 * X + Y
    ux, uy = -2.0 * X * h + 0.5 * g, -8.0 * Y * h + g
    lap = -(10.0 + 7.0 * X + 26.0 * Y)
    k = 1.0 + 0.5 * np.sin(3.0 * X) * np.cos(2.0 * Y)
    kx, ky = 1.5 * np.cos(3.0 * X) * np.cos(2.0 * Y), -np.sin(3.0 * X) * np.sin(2.0 * Y)
    f = -(k * lap + kx * ux + ky * uy)
    return f, np.where(p.inside_mask(), g * h, 0.0), k


def test_the_discretisation_solves_the_right_pde(pkg):
    """The L2 error in D against the closed-form u falls by >= 1.7 from 97x130 to 194x260 (first order at the cut
    boundary; measured 1.385e-2 -> 7.334e-3, ratio 1.89) and stays within 1.1x that of k = 1 with the plain
    manufactured f on the same grids (measured 1.012x)."""
    err, err1 = [], []
    for grid in ((97, 130), (194, 260)):
        p = pkg.PoissonEllipse(M=grid[0], N=grid[1])
        f, u, k = smooth_problem(p)
        assert np.array_equal(k, kappas(p)["smooth"])
        w = pkg.solve(p, "cpu", rhs=f, diffusion=k)
        f1, u1 = manufactured(p)
        w1 = pkg.solve(p, "cpu", rhs=f1)
        assert w.converged and w1.converged
        err.append(p.error_norms(w.w, exact=u)["l2_error"])
        err1.append(p.error_norms(w1.w, exact=u1)["l2_error"])
        print(f"{grid}: L2 error in D {err[-1]:.4e} (k = 1: {err1[-1]:.4e}, ratio {err[-1] / err1[-1]:.4f}), "
              f"iters {w.iters} / {w1.iters}")
        assert err[-1] <= 1.1 * err1[-1]
    print(f"refinement ratio {err[0] / err[1]:.3f}")
    assert err[0] / err[1] >= 1.7


def picard_problem(pkg, grid=(97, 130)):
    """-∇·((1 + u^2)∇u) = 10 + 7x + 26y in D: the linear solves run to rtol = 1e-12 of their data (breakdown guard
    off), far below picard_rtol."""
    p = pkg.PoissonEllipse(M=grid[0], N=grid[1], stop="residual", rtol=1e-12, breakdown_tol=0.0)
    return p, manufactured(p)[0]


def kappa_u2(u):
    return 1.0 + u * u


PICARD_STEPS = 9  # measured on the cpu backend at 97 x 130 (test_quasilinear_picard_cpu); the GPU test pins it too


def test_quasilinear_picard_cpu(pkg):
    """kappa(u) = 1 + u^2 at 97 x 130 from u = 0: the nonlinear residual history is strictly decreasing down to
    picard_rtol = 1e-8, in the pinned number of steps; kappa = 1 is the linear problem, one step.  Measured: 9
    steps, residuals 1.558e+01 7.370e+00 1.357e+00 2.322e-01 3.007e-02 3.225e-03 2.933e-04 2.316e-05 1.616e-06
    1.011e-07 (a factor of about 12 per step; max u = 0.872)."""
    p, f = picard_problem(pkg)
    pc = pkg.QuasilinearPicard(p, kappa_u2, backend="cpu", picard_rtol=1e-8)
    w = pc.solve(f)
    print(f"steps {pc.steps}, history {['%.3e' % h for h in pc.history]}, max u {w.max():.6f}")
    assert pc.converged and pc.steps == len(pc.history) - 1
    assert all(b < a for a, b in zip(pc.history, pc.history[1:]))
    assert pc.history[-1] <= 1e-8 * pc.history[0]
    assert pc.steps == PICARD_STEPS
    # the fixed point solves the frozen-coefficient problem with its own coefficient
    again = pkg.solve(p, "cpu", rhs=f, diffusion=kappa_u2(w)).w
    assert np.abs(again - w).max() <= 1e-7 * np.abs(w).max()
    lin = pkg.solve(p, "cpu", rhs=f).w
    one = pkg.QuasilinearPicard(p, lambda v: 1.0 + 0.0 * v, backend="cpu")
    assert np.abs(one.solve(f) - lin).max() <= 1e-12 * np.abs(lin).max() and one.steps == 1
    with pytest.raises(ValueError, match="diffusion"):
        pkg.QuasilinearPicard(p, kappa_u2, backend="cpu", diffusion=np.ones((98, 131)))


def test_time_steppers_take_the_field(pkg):
    """BackwardEuler / ThetaScheme with diffusion= in session_kw on the cpu backend: theta = 1 is BackwardEuler
    bitwise, one BackwardEuler step is the solve with the field and sigma = 1/dt, and the theta-scheme's
    right-hand side applies the k operator."""
    p = pkg.PoissonEllipse(M=40, N=40)
    k = kappas(p)["smooth"]
    _, u = manufactured(p)
    dt = 1e-3
    be = pkg.BackwardEuler(p, dt, backend="cpu", diffusion=k)
    v = be.step(u, 1.0)
    want = pkg.solve(pkg.PoissonEllipse(M=40, N=40, sigma=1.0 / dt), "cpu", rhs=u / dt + 1.0, w0=u, diffusion=k).w
    assert v.tobytes() == want.tobytes()
    assert pkg.ThetaScheme(p, dt, theta=1.0, backend="cpu", diffusion=k).step(u, 1.0).tobytes() == v.tobytes()
    cn = pkg.ThetaScheme(p, dt, theta=0.5, backend="cpu", diffusion=k)
    rhs = cn.rhs(u, 1.0)
    L = cn.problem.apply(u, diffusion=k)
    ref = -L + 2.0 * cn.s * u + 2.0
    assert np.abs(rhs - ref)[1:-1, 1:-1].max() <= 8 * np.finfo(float).eps * np.abs(ref).max()
    assert np.abs(rhs - pkg.ThetaScheme(p, dt, theta=0.5, backend="cpu").rhs(u, 1.0)).max() > 1e-2
    w = cn.step(u, 1.0)
    assert cn.last["status"] == "converged" and np.isfinite(w).all()


def test_refusals(pkg):
    """NaN, infinity, zero and negative values are refused on EVERY node, the box boundary included."""
    p = pkg.PoissonEllipse(M=40, N=40)
    k = kappas(p)["smooth"]
    bad = {}
    for key, v in (("nan", np.nan), ("inf", np.inf), ("zero", 0.0), ("negative", -1e-3)):
        for where, ij in (("inner", (7, 9)), ("edge", (0, 13)), ("corner", (40, 40))):
            bad[(key, where)] = k.copy()
            bad[(key, where)][ij] = v
    for backend in ("cpu", "omp", "cpu-decomposed", "torch"):
        for field in bad.values():
            with pytest.raises(ValueError, match="diffusion"):
                pkg.solve(p, backend, diffusion=field)
        with pytest.raises(ValueError, match="shape"):
            pkg.solve(p, backend, diffusion=k[:-1])
        with pytest.raises(ValueError, match="float64"):
            pkg.solve(p, backend, diffusion=k.astype(np.float32))
        with pytest.raises(ValueError, match="diffusion"):
            pkg.solve(p, backend, diffusion=[[1.0]])
    for field in bad.values():
        with pytest.raises(ValueError, match="diffusion"):
            p.apply(k, diffusion=field)
    with pytest.raises(ValueError, match="diffusion"):
        sub("models.sstep_pcg").TorchSStepPCG(p, diffusion=k)
    with pytest.raises(ValueError, match="diffusion"):
        sub("ops.kernels").DeviceOps(p, diffusion=k)
    with pytest.raises(ValueError, match="diffusion"):
        sub("parallel.dist_solver").DistGpuPCG(p, None, comm="torch", diffusion=k)
    with pytest.raises(ValueError, match="diffusion"):
        sub("parallel.dist_solver").DistGpuPCG(p, None, comm="native", diffusion=k)
    # CPU tensors pass like NumPy arrays
    a, b = pkg.solve(p, "cpu", diffusion=k), pkg.solve(p, "cpu", diffusion=torch.from_numpy(k))
    assert a.iters == b.iters and a.w.tobytes() == b.w.tobytes()


@pytest.mark.parametrize("dtype", ["fp64", "fp32"])
@pytest.mark.parametrize("grid,world,split", [((40, 40), 1, "reference"), ((97, 130), 4, "reference"),
                                              ((97, 130), 3, "rows"), ((400, 600), 1, "reference")])
def test_memory_plan_face_fields(pkg, grid, world, split, dtype):
    """A diffusion session: the shift field and two face-coefficient fields behind the five of pcg1 (bk, then ak),
    with their pitch and ghost layers, plus one row behind the last field for ak's row nx+3 -- and every plan
    without the flag, with or without the shift field, what it was."""
    n = pkg.load_native()
    spec = pkg.PoissonEllipse(M=grid[0], N=grid[1]).to_native()
    for rank in range(world):
        args = (spec, world, getattr(n.Split, split), rank, dtype)
        a, b = n.memory_plan(*args, False), n.memory_plan(*args, True)
        d = n.memory_plan(*args, False, True)
        assert n.memory_plan(*args, True, True) == d  # the shift field comes with the flag either way
        assert a == n.memory_plan(*args, False, False) and b == n.memory_plan(*args, True, False)
        assert "ndiff" not in a and "ndiff" not in b
        assert a["fields_total"] == 5 * a["field_bytes"] and b["fields_total"] == 6 * a["field_bytes"]
        e, P, fb = d["elem"], d["pitch"], d["field_bytes"]
        for key in ("elem", "pitch", "gh", "field_bytes", "nfields", "nx", "ny"):
            assert a[key] == d[key]
        assert d["at"][:6] == b["at"] and d["shift_field"] == 5 and d["ndiff"] == 2 and d["diff_field"] == (7, 6)
        assert d["diff_extra"] >= P * e and d["diff_extra"] % 256 == 0
        assert d["fields_total"] == 8 * fb + d["diff_extra"] and d["total"] - a["total"] == 3 * fb + d["diff_extra"]
        for f in (6, 7):
            origin = d["at"][f]
            assert (origin + e) % 256 == 0
            first = origin + (-1 * P - 2) * e  # row -1, column -2 (col_ptr's base)
            # the last cell read: row nx+2 (bk) / nx+3 (ak), the column after a clamped chunk (ny + 4); written:
            # the whole row, columns -1 .. P-2
            last_row = d["nx"] + (3 if f == 7 else 2)
            last = origin + (last_row * P + P - 2) * e
            assert d["ny"] + 4 <= P - 2
            assert f * fb <= first and last + e <= (f + 1) * fb + (d["diff_extra"] if f == 7 else 0)
