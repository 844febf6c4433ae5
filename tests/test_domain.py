"""Level-set domains D = {phi < 0} on the CPU paths: the face coefficients against an independent NumPy statement of
the definition, the backends against each other, accuracy against closed forms (the ellipse as a level set, a disc,
an annulus with a floating and a pinned hole), the helpers of PoissonEllipse, the refusals and the nonlinear models.

The definition (fp64, this operation order): phi_c[i,j] = 0.25 ((phi[i-1,j-1] + phi[i-1,j]) + (phi[i,j-1] +
phi[i,j])); theta(p, q) = 1 if both < 0, 0 if neither, else n / (n - m), n the negative end; g = theta +
(1 - theta) / eps; a[i,j] = g(theta(phi_c[i,j], phi_c[i,j+1])) for i = 1..M, j = 1..N-1; b[i,j] =
g(theta(phi_c[i,j], phi_c[i+1,j])) for i = 1..M-1, j = 1..N; the right-hand side is masked by phi[i,j] < 0.
"""
import numpy as np
import pytest
import torch

from conftest import sub
from test_diffusion import kappas

GRIDS = [(40, 40), (33, 70)]
R1, R2 = 0.2, 0.5  # the annulus


def domains(p):
    """The test domains of the default box as level-set fields, and the reaction field that goes with each (the pin
    of `holed`'s hole, else None)."""
    x, y = p.coords()
    X, Y = np.meshgrid(x, y, indexing="ij")
    hole = np.hypot(X - 0.3, Y - 0.1)
    phi = dict(disc=np.hypot(X - 0.2, Y - 0.05) - 0.45,
               two=np.minimum(np.hypot(X + 0.5, Y) - 0.3, np.hypot(X - 0.45, Y - 0.1) - 0.35),
               holed=np.maximum(p.ellipse_levelset(), 0.15 - hole),
               speckle=np.random.default_rng(3).standard_normal(X.shape))
    pin = dict(disc=None, two=None, speckle=None, holed=np.where(hole < 0.15, 1e8, 0.0))
    return phi, pin


def numpy_faces(p, phi):
    """a, b as (M+2) x (N+2) arrays (global node index, as cpu_assemble returns them) from the definition above,
    written with NumPy slices; faces outside the stated ranges hold 1."""
    M, N, eps = p.M, p.N, p.eps
    pc = 0.25 * ((phi[:-1, :-1] + phi[:-1, 1:]) + (phi[1:, :-1] + phi[1:, 1:]))  # pc[i-1, j-1] = phi_c[i, j]

    def g(P, Q):
        pn, qn = P < 0, Q < 0
        n, m = np.where(pn, P, Q), np.where(pn, Q, P)
        with np.errstate(all="ignore"):
            cut = n / (n - m)
        th = np.where(pn & qn, 1.0, np.where(~pn & ~qn, 0.0, cut))
        return th + (1.0 - th) / eps

    a, b = np.ones((M + 2, N + 2)), np.ones((M + 2, N + 2))
    a[1:M + 1, 1:N] = g(pc[:, :-1], pc[:, 1:])
    b[1:M, 1:N + 1] = g(pc[:-1, :], pc[1:, :])
    return a, b


def host_faces(p, phi, k=None):
    """numpy_faces on the (M+1) x (N+1) nodes, multiplied by the face means of k: what ops/reference.py's apply_A
    and diag take for the whole grid."""
    a, b = numpy_faces(p, phi)
    a, b = a[:p.M + 1, :p.N + 1].copy(), b[:p.M + 1, :p.N + 1].copy()
    if k is not None:
        a[1:, :] = (0.5 * (k[:-1, :] + k[1:, :])) * a[1:, :]
        b[:, 1:] = (0.5 * (k[:, :-1] + k[:, 1:])) * b[:, 1:]
    return a, b


def host_residual(p, phi, w, rhs, k=None, shift=0.0):
    """sqrt(h1 h2 sum r^2) and (z, r) = h1 h2 sum r^2 / D for r = B - (A + shift I) w, B = rhs under the mask
    phi < 0 (rhs: an array, or the constant F), with ops/reference.py on host_faces."""
    R = sub("ops.reference")
    a, b = host_faces(p, phi, k)
    B = np.where(phi < 0, rhs, 0.0)[1:-1, 1:-1]
    q = w.copy()
    q[0, :] = q[-1, :] = 0.0
    q[:, 0] = q[:, -1] = 0.0
    r = B - R.apply_A(q, a, b, p.h1, p.h2, shift)
    D = R.diag(a, b, p.h1, p.h2, shift)
    hh = p.h1 * p.h2
    return float(np.sqrt((r * r).sum() * hh)), float((r * r / D).sum() * hh)


@pytest.mark.parametrize("grid", GRIDS + [(97, 130)])
@pytest.mark.parametrize("name", ["disc", "two", "holed", "speckle"])
def test_faces_are_the_definition_bitwise(pkg, grid, name):
    """cpu_assemble(domain=) and ops.reference.assemble(domain=) against numpy_faces, bit for bit, on every face the
    interior stencils read (and 1 elsewhere); B is F under phi < 0 on the interior nodes."""
    p = pkg.PoissonEllipse(M=grid[0], N=grid[1], F=2.5)
    phi = domains(p)[0][name]
    M, N = grid
    a, b, B = pkg.load_native().cpu_assemble(p.to_native(), domain=phi)
    wa, wb = numpy_faces(p, phi)
    assert a.tobytes() == wa.tobytes() and b.tobytes() == wb.tobytes()
    cut = ((wa != 1.0) & (wa != 1.0 / p.eps)).sum() + ((wb != 1.0) & (wb != 1.0 / p.eps)).sum()
    assert cut > 0 and (wa == 1.0 / p.eps).any() and (wa[1:M + 1, 1:N] == 1.0).any()
    wB = np.zeros((M + 1, N + 1))
    wB[1:-1, 1:-1] = np.where(phi < 0, 2.5, 0.0)[1:-1, 1:-1]
    assert np.array_equal(B, wB)
    sd = sub("parallel.decomp").subdomain(M, N, 1, 1, 0)
    ta, tb, tB = sub("ops.reference").assemble(p, sd, domain=phi)
    assert np.array_equal(ta.numpy(), wa[:M + 1, :N + 1]) and np.array_equal(tb.numpy(), wb[:M + 1, :N + 1])
    assert np.array_equal(tB.numpy(), wB)
    # the ellipse's own faces are other numbers
    ea, _, _ = pkg.load_native().cpu_assemble(p.to_native())
    assert not np.array_equal(ea, a)


@pytest.mark.parametrize("grid", GRIDS)
@pytest.mark.parametrize("name", ["disc", "two", "holed"])
def test_backends_agree(pkg, grid, name):
    """cpu, omp, cpu-decomposed (4 ranks) and torch: the same iteration count and w within 1e-12 max|w|;
    diffusion=ones next to domain is domain alone, bitwise."""
    p = pkg.PoissonEllipse(M=grid[0], N=grid[1])
    phis, pins = domains(p)
    kw = dict(domain=phis[name], reaction=pins[name])
    ref = pkg.solve(p, "cpu", **kw)
    assert ref.converged and ref.iters > 10
    top = np.abs(ref.w).max()
    for backend, bkw in (("omp", dict(threads=4)), ("cpu-decomposed", dict(ranks=4)), ("torch", {})):
        r = pkg.solve(p, backend, **kw, **bkw)
        err = np.abs(r.w - ref.w).max()
        print(f"{grid} {name} {backend}: iters {r.iters} (cpu {ref.iters}) max|w - w_cpu| {err:.3e}, max|w| {top:.3e}")
        assert r.iters == ref.iters and r.status == "converged"
        assert err <= 1e-12 * top
    one = np.ones((grid[0] + 1, grid[1] + 1))
    for backend, bkw in (("cpu", {}), ("cpu-decomposed", dict(ranks=4)), ("torch", {})):
        x, y = pkg.solve(p, backend, **kw, **bkw), pkg.solve(p, backend, diffusion=one, **kw, **bkw)
        assert x.iters == y.iters and np.asarray(x.w).tobytes() == np.asarray(y.w).tobytes()
    # a real field composes: the faces of the domain times the means of k
    k = kappas(p)["smooth"]
    rk = pkg.solve(p, "cpu", diffusion=k, **kw)
    assert rk.converged and np.abs(rk.w - ref.w).max() > 1e-3 * top
    rng = np.random.default_rng(11)
    x = rng.standard_normal(k.shape)
    a, b = host_faces(p, phis[name], k)
    q = x.copy()
    q[0, :] = q[-1, :] = 0.0
    q[:, 0] = q[:, -1] = 0.0
    want = sub("ops.reference").apply_A(q, a, b, p.h1, p.h2)
    got = p.apply(x, diffusion=k, domain=phis[name])[1:-1, 1:-1]
    assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max()


def _tight(pkg, n, **kw):
    return pkg.PoissonEllipse(M=n, N=n, stop="residual", rtol=1e-10, breakdown_tol=0.0, **kw)


def test_the_ellipse_as_a_level_set(pkg):
    """domain = ellipse_levelset(), f = 1: the L2 error against the closed form is within 1.10 of the existing
    ellipse solve's on the same grid (prototype: 1.014, 1.0005, 1.018 at 40^2, 80^2, 160^2)."""
    for n in (40, 80, 160):
        p = _tight(pkg, n)
        a = pkg.solve(p, "cpu", domain=p.ellipse_levelset())
        b = pkg.solve(p, "cpu")
        assert a.converged and b.converged
        x, y = p.coords()
        u = p.exact_solution(*np.meshgrid(x, y, indexing="ij"))
        ea = p.error_norms(a.w, exact=u, domain=p.ellipse_levelset())["l2_error"]
        eb = p.error_norms(b.w)["l2_error"]
        print(f"{n}^2: L2 error domain {ea:.4e} ellipse {eb:.4e} ratio {ea / eb:.4f}")
        assert ea / eb <= 1.10


def test_disc_convergence(pkg):
    """disc, f = 1, u = (R^2 - r^2) / 4: the L2 error falls by >= 1.6 per halving over 40^2 -> 80^2 -> 160^2
    (prototype: 1.80e-3, 9.6e-4, 4.9e-4)."""
    err = []
    for n in (40, 80, 160):
        p = _tight(pkg, n)
        phi = domains(p)[0]["disc"]
        r = pkg.solve(p, "cpu", domain=phi)
        assert r.converged
        x, y = p.coords()
        X, Y = np.meshgrid(x, y, indexing="ij")
        u = np.where(phi < 0, (0.45 ** 2 - (X - 0.2) ** 2 - (Y - 0.05) ** 2) / 4.0, 0.0)
        err.append(p.error_norms(r.w, exact=u, domain=phi)["l2_error"])
        print(f"{n}^2: L2 error {err[-1]:.4e}, iters {r.iters}")
    print(f"ratios {err[0] / err[1]:.3f} {err[1] / err[2]:.3f}")
    assert err[0] / err[1] >= 1.6 and err[1] / err[2] >= 1.6


def _annulus(p):
    x, y = p.coords()
    X, Y = np.meshgrid(x, y, indexing="ij")
    r = np.hypot(X, Y)
    phi = np.maximum(r - R2, R1 - r)
    # -Δu = 1, u(R1) = u(R2) = 0: u = -r^2/4 + A ln r + B
    A = (R2 ** 2 - R1 ** 2) / (4.0 * np.log(R2 / R1))
    B = R1 ** 2 / 4.0 - A * np.log(R1)
    with np.errstate(divide="ignore", invalid="ignore"):
        u = np.where(phi < 0, -r * r / 4.0 + A * np.log(r) + B, 0.0)
    rm = np.sqrt(2.0 * A)  # u' = 0
    return phi, u, r < R1, float(-rm * rm / 4.0 + A * np.log(rm) + B)


def test_floating_and_pinned_holes(pkg):
    """The annulus R1 = 0.2, R2 = 0.5, f = 1.  Its hole touches no box boundary, so nothing anchors u there:
    unpinned, the centre value lies above the exact maximum (prototype: 0.033 against 0.0115 at every resolution);
    pinned with reaction = 1e8 in the hole it is below 1e-10 and the L2 error falls by >= 1.4 per halving
    (prototype: 1.21e-3, 7.5e-4, 4.0e-4)."""
    err = []
    for n in (40, 80, 160):
        p = _tight(pkg, n)
        phi, u, hole, umax = _annulus(p)
        c = (n // 2, n // 2)
        assert hole[c] and abs(p.coords()[0][c[0]]) < 1e-12
        free = pkg.solve(p, "cpu", domain=phi)
        pinned = pkg.solve(p, "cpu", domain=phi, reaction=np.where(hole, 1e8, 0.0))
        assert free.converged and pinned.converged
        err.append(p.error_norms(pinned.w, exact=u, domain=phi)["l2_error"])
        print(f"{n}^2: centre unpinned {free.w[c]:.4e} pinned {pinned.w[c]:.3e} (exact max {umax:.4e}); pinned L2 "
              f"error {err[-1]:.4e}, iters {free.iters} / {pinned.iters}")
        assert abs(pinned.w[c]) < 1e-10
        assert free.w[c] > umax
    print(f"ratios {err[0] / err[1]:.3f} {err[1] / err[2]:.3f}")
    assert err[0] / err[1] >= 1.4 and err[1] / err[2] >= 1.4


def test_helpers(pkg):
    p = pkg.PoissonEllipse(M=40, N=40)
    phis, _ = domains(p)
    phi = phis["disc"]
    x, y = p.coords()
    X, Y = np.meshgrid(x, y, indexing="ij")
    assert np.array_equal(p.ellipse_levelset(), X * X + 4.0 * Y * Y - 1.0)
    assert np.array_equal(p.ellipse_levelset() < 0, p.inside_mask())
    q = pkg.PoissonEllipse(M=40, N=40, ax=0.8, by=0.4)
    assert np.array_equal(q.ellipse_levelset(), (X / 0.8) ** 2 + (Y / 0.4) ** 2 - 1.0)
    assert np.array_equal(q.ellipse_levelset() < 0, q.inside_mask())
    assert np.array_equal(p.inside_mask(domain=phi), phi < 0) and p.inside_mask(domain=phi).dtype == bool
    assert np.array_equal(p.inside_mask(domain=torch.from_numpy(phi)), phi < 0)
    # error_norms: the mask of phi, and no closed form
    w = np.random.default_rng(1).standard_normal(phi.shape)
    e = p.error_norms(w, exact=np.zeros_like(w), domain=phi)
    assert e["l2_error"] == float(np.sqrt((np.where(phi < 0, w, 0.0) ** 2).sum() * p.h1 * p.h2))
    assert e["l2_error"] != p.error_norms(w, exact=np.zeros_like(w))["l2_error"]
    with pytest.raises(ValueError, match="exact"):
        p.error_norms(w, domain=phi)
    # apply: the matrix of the domain's faces on the whole box
    a, b = host_faces(p, phi)
    xq = w.copy()
    xq[0, :] = xq[-1, :] = 0.0
    xq[:, 0] = xq[:, -1] = 0.0
    want = sub("ops.reference").apply_A(xq, a, b, p.h1, p.h2)
    got = p.apply(w, domain=phi)
    assert np.abs(got[1:-1, 1:-1] - want).max() <= 1e-12 * np.abs(want).max()
    assert not got[0, :].any() and not got[-1, :].any() and not got[:, 0].any() and not got[:, -1].any()
    assert np.abs(got - p.apply(w)).max() > 1e-3 * np.abs(want).max()
    assert p.domain_field(None) is None and p.domain_field(phi).flags.c_contiguous


def test_refusals(pkg):
    """domain_field's rules on every entry point: type, dtype, shape, NaN and infinity on any node."""
    p = pkg.PoissonEllipse(M=40, N=40)
    phi = domains(p)[0]["disc"]
    bad = []
    for v in (np.nan, np.inf, -np.inf):
        for ij in ((7, 9), (0, 13), (40, 40)):
            bad.append(phi.copy())
            bad[-1][ij] = v
    cases = [(f, "domain") for f in bad] + [(phi[:-1], "shape"), (phi.astype(np.float32), "float64"),
                                            ([[1.0]], "domain")]
    for arg, what in cases:
        with pytest.raises(ValueError, match=what):
            p.domain_field(arg)
        with pytest.raises(ValueError, match=what):
            p.apply(phi, domain=arg)
        with pytest.raises(ValueError, match=what):
            p.inside_mask(domain=arg)
        for backend in ("cpu", "omp", "cpu-decomposed", "torch"):
            with pytest.raises(ValueError, match=what):
                pkg.solve(p, backend, domain=arg)
    with pytest.raises(ValueError, match="domain"):
        sub("models.sstep_pcg").TorchSStepPCG(p, domain=phi)
    with pytest.raises(ValueError, match="domain"):
        sub("ops.kernels").DeviceOps(p, domain=phi)
    for comm in ("torch", "native"):
        with pytest.raises(ValueError, match="domain"):
            sub("parallel.dist_solver").DistGpuPCG(p, None, comm=comm, domain=phi)
    a, b = pkg.solve(p, "cpu", domain=phi), pkg.solve(p, "cpu", domain=torch.from_numpy(phi))
    assert a.iters == b.iters and a.w.tobytes() == b.w.tobytes()


def test_time_steppers_take_the_domain(pkg):
    p = pkg.PoissonEllipse(M=40, N=40)
    phi = domains(p)[0]["disc"]
    u = np.where(phi < 0, -phi, 0.0)
    dt = 1e-3
    v = pkg.BackwardEuler(p, dt, backend="cpu", domain=phi).step(u, 1.0)
    want = pkg.solve(pkg.PoissonEllipse(M=40, N=40, sigma=1.0 / dt), "cpu", rhs=u / dt + 1.0, w0=u, domain=phi).w
    assert v.tobytes() == want.tobytes()
    assert pkg.ThetaScheme(p, dt, theta=1.0, backend="cpu", domain=phi).step(u, 1.0).tobytes() == v.tobytes()
    cn = pkg.ThetaScheme(p, dt, theta=0.5, backend="cpu", domain=phi)
    ref = -cn.problem.apply(u, domain=phi) + 2.0 * cn.s * u + 2.0
    assert np.abs(cn.rhs(u, 1.0) - ref)[1:-1, 1:-1].max() <= 8 * np.finfo(float).eps * np.abs(ref).max()
    w = cn.step(u, 1.0)
    assert cn.last["status"] == "converged" and np.isfinite(w).all()


def _nonlinear_problem(pkg):
    p = pkg.PoissonEllipse(M=40, N=40, stop="residual", rtol=1e-12, breakdown_tol=0.0)
    phi = domains(p)[0]["disc"]
    x, y = p.coords()
    X, Y = np.meshgrid(x, y, indexing="ij")
    return p, phi, 10.0 + 7.0 * X + 26.0 * Y


def test_semilinear_newton_on_a_domain(pkg):
    """-Δu + u^3 = f on the disc: Newton converges, and its last residual is that of the disc's mask and faces,
    measured here; with the ellipse's mask the same iterate leaves a residual orders above."""
    p, phi, f = _nonlinear_problem(pkg)
    nw = pkg.SemilinearNewton(p, lambda u: u ** 3, lambda u: 3.0 * u * u, backend="cpu", newton_rtol=1e-8, domain=phi)
    u = nw.solve(f)
    assert nw.converged and nw.history[-1] <= 1e-8 * nw.history[0] and 1 <= nw.steps <= 10
    res, _ = host_residual(p, phi, u, f - u ** 3)
    ell = np.where(p.inside_mask(), f - u ** 3, 0.0) - p.apply(u, domain=phi)
    ell = float(np.sqrt((ell[1:-1, 1:-1] ** 2).sum() * p.h1 * p.h2))
    print(f"steps {nw.steps}, history {['%.3e' % h for h in nw.history]}; disc-mask residual {res:.3e}, "
          f"ellipse-mask residual {ell:.3e}")
    assert abs(res - nw.history[-1]) <= 1e-6 * nw.history[0]
    assert res <= 1e-7 * nw.history[0] < 1e-3 * ell


def test_quasilinear_picard_on_a_domain(pkg):
    """-∇·((1 + u^2)∇u) = f on the disc, likewise."""
    p, phi, f = _nonlinear_problem(pkg)
    pc = pkg.QuasilinearPicard(p, lambda u: 1.0 + u * u, backend="cpu", picard_rtol=1e-8, domain=phi)
    u = pc.solve(f)
    assert pc.converged and pc.history[-1] <= 1e-8 * pc.history[0]
    assert all(b < a for a, b in zip(pc.history, pc.history[1:]))
    res, _ = host_residual(p, phi, u, f, k=1.0 + u * u)
    print(f"steps {pc.steps}, history {['%.3e' % h for h in pc.history]}; disc-mask residual {res:.3e}")
    assert abs(res - pc.history[-1]) <= 1e-6 * pc.history[0]
    assert res <= 1e-7 * pc.history[0]


@pytest.mark.parametrize("dtype", ["fp64", "fp32"])
@pytest.mark.parametrize("grid,world,split", [((40, 40), 1, "reference"), ((97, 130), 4, "reference"),
                                              ((20, 300), 3, "rows")])
def test_memory_plan_mask(pkg, grid, world, split, dtype):
    """A domain plan is the diffusion plan plus the mask behind it: one byte per node of the owned rows in the
    fields' pitch, rounded up to 256 B; every plan without the flag is what it was."""
    n = pkg.load_native()
    spec = pkg.PoissonEllipse(M=grid[0], N=grid[1]).to_native()
    for rank in range(world):
        args = (spec, world, getattr(n.Split, split), rank, dtype)
        dif, dom = n.memory_plan(*args, False, True), n.memory_plan(*args, False, False, True)
        assert n.memory_plan(*args, True, True, True) == dom and "mask_bytes" not in dif
        assert n.memory_plan(*args, False, True, False) == dif
        for key, v in dif.items():
            if key not in ("fields_total", "total"):
                assert dom[key] == v
        mb = dom["mask_bytes"]
        assert dom["pitch"] * dom["nx"] <= mb < dom["pitch"] * dom["nx"] + 256 and mb % 256 == 0
        assert dom["mask_off"] == dif["fields_total"] and dom["mask_off"] % 256 == 0
        assert dom["fields_total"] == dif["fields_total"] + mb and dom["total"] == dif["total"] + mb
        assert (dom["nx"] - 1) * dom["pitch"] + dom["ny"] < mb  # the last owned node's byte
