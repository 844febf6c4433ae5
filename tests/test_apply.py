"""The operator apply on the host -- PoissonEllipse.apply over the native cpu_apply -- and the θ-scheme time
stepper built on it (pmx.ThetaScheme, backend="cpu").

out = alpha L x + beta x + gamma y + const on the interior nodes, 0 on the box boundary, L = A + sigma I: the
plain matrix on the whole box, no ellipse mask; boundary values of x count as 0.
"""
import numpy as np
import pytest
import torch

from conftest import sub

U53 = 2.0 ** -53
SCALARS = dict(alpha=-1.75, beta=3.5, gamma=0.625, const=-2.25)
TIGHT = dict(delta=1e-13, breakdown_tol=0.0)


def fields(M, N, seed=0):
    """Random x and y, boundary lines included (x's must not matter)."""
    rng = np.random.default_rng(seed + 1000 * M + N)
    return rng.standard_normal((M + 1, N + 1)), rng.standard_normal((M + 1, N + 1))


def torch_reference(pkg, p, x, y, alpha, beta, gamma, const):
    """(ref, E) on the interior nodes from ops/reference.py::apply_A on the arrays of cpu_assemble: the
    combination, and the magnitude E = |alpha| ((|A| + sigma) |x|) + |beta| |x| + |gamma| |y| + |const| with
    |A| |x| formed as apply_A forms A x but from the absolute value of every term."""
    ref_ops = sub("ops.reference")
    a, b, _ = pkg.load_native().cpu_assemble(p.to_native())
    a = torch.from_numpy(a[:p.M + 1, :p.N + 1])
    b = torch.from_numpy(b[:p.M + 1, :p.N + 1])
    q = torch.from_numpy(x).clone()
    q[0, :] = q[-1, :] = 0.0
    q[:, 0] = q[:, -1] = 0.0
    h1, h2 = p.h1, p.h2
    Lx = ref_ops.apply_A(q, a, b, h1, h2, p.sigma)
    c = q[1:-1, 1:-1]
    yc = torch.from_numpy(y)[1:-1, 1:-1]
    ref = alpha * Lx + beta * c + gamma * yc + const
    m = q.abs()
    mc = m[1:-1, 1:-1]
    ax = 1.0 / h1 * (a[2:, 1:-1] * (m[2:, 1:-1] + mc) / h1 + a[1:-1, 1:-1] * (mc + m[:-2, 1:-1]) / h1)
    ay = 1.0 / h2 * (b[1:-1, 2:] * (m[1:-1, 2:] + mc) / h2 + b[1:-1, 1:-1] * (mc + m[1:-1, :-2]) / h2)
    E = abs(alpha) * ((ax + ay) + p.sigma * mc) + abs(beta) * mc + abs(gamma) * yc.abs() + abs(const)
    return ref.numpy(), E.numpy()


def boundary_is_zero(out):
    return not (out[0].any() or out[-1].any() or out[:, 0].any() or out[:, -1].any())


@pytest.mark.parametrize("sigma", [0.0, 100.0])
@pytest.mark.parametrize("grid", [(40, 40), (97, 130)])
def test_operator_against_the_pytorch_reference(pkg, grid, sigma):
    """Pointwise |out - ref| <= 32 * 2^-53 * E: any path from an input to the output has at most about 10
    roundings in either implementation, so the bound is loose by under 2x and still O(1) away from a wrong
    coefficient or neighbour.  With the default scalars the two are the same operations in the same order:
    that case is asserted bitwise."""
    p = pkg.PoissonEllipse(M=grid[0], N=grid[1], sigma=sigma)
    x, y = fields(*grid)
    out = p.apply(x, y=y, **SCALARS)
    assert out.dtype == np.float64 and out.shape == x.shape and boundary_is_zero(out)
    ref, E = torch_reference(pkg, p, x, y, **SCALARS)
    err = np.abs(out[1:-1, 1:-1] - ref)
    print(f"{grid} sigma {sigma}: max err/E {float((err / E).max()) / U53:.3g} x 2^-53, bitwise "
          f"{np.array_equal(out[1:-1, 1:-1], ref)}")
    assert (err <= 32 * U53 * E).all()
    plain = p.apply(x)
    ref0, _ = torch_reference(pkg, p, x, y, 1.0, 0.0, 0.0, 0.0)
    assert np.array_equal(plain[1:-1, 1:-1], ref0) and boundary_is_zero(plain)
    # boundary values of x are not read: NaN there changes nothing
    xn = x.copy()
    xn[0, :] = xn[-1, :] = np.nan
    xn[:, 0] = xn[:, -1] = np.nan
    assert np.array_equal(p.apply(xn, y=y, **SCALARS), out)
    # out=: filled and returned; it may be y
    buf = y.copy()
    assert p.apply(x, buf, y=buf, **SCALARS) is buf and np.array_equal(buf, out)
    # an interior NaN propagates to its stencil and no further
    xn = x.copy()
    xn[5, 7] = np.nan
    bad = np.isnan(p.apply(xn))
    assert bad.sum() == 5 and bad[5, 7] and bad[4, 7] and bad[6, 7] and bad[5, 6] and bad[5, 8]


def test_consistency_with_the_solver(pkg):
    """apply(w) of a tightly converged oracle solution gives back the masked right-hand side B: max|B - apply(w)|
    over the interior nodes measured 2.518e-9 at 40 x 40 (default problem, delta = 1e-13, breakdown_tol = 0);
    the bound is 10x that."""
    p = pkg.PoissonEllipse(M=40, N=40, **TIGHT)
    r = pkg.solve(p, "cpu")
    assert r.converged
    _, _, B = pkg.load_native().cpu_assemble(p.to_native())
    gap = float(np.abs(B - p.apply(r.w))[1:-1, 1:-1].max())
    print(f"max|B - apply(w)| = {gap:.3e} after {r.iters} iterations")
    assert gap <= 10 * 2.518e-9


@pytest.fixture(scope="module")
def steady(pkg):
    """The sigma = 0 steady solution at 40 x 40, the start of the decay runs."""
    return pkg.solve(pkg.PoissonEllipse(M=40, N=40, **TIGHT), "cpu").w


@pytest.mark.parametrize("theta", [0.5, 1.0])
def test_temporal_order(pkg, steady, theta):
    """u_t = -A u from the steady solution to T = 0.04 in n = 4, 8, 16 steps: max|u_4 - u_8| / max|u_8 - u_16| is
    about 4 for a second-order scheme and about 2 for a first-order one (measured with the CPU oracle: 4.06 at
    θ = 0.5, 1.85 at θ = 1)."""
    p = pkg.PoissonEllipse(M=40, N=40, **TIGHT)
    T = 0.04
    end = {}
    for n in (4, 8, 16):
        ts = pkg.ThetaScheme(p, T / n, theta=theta, backend="cpu")
        u = steady
        for _ in range(n):
            u = ts.step(u)
            assert ts.last["status"] == "converged"
        end[n] = u
    ratio = float(np.abs(end[4] - end[8]).max() / np.abs(end[8] - end[16]).max())
    print(f"theta {theta}: ratio {ratio:.3f}")
    if theta == 0.5:
        assert ratio > 3.5
    else:
        assert ratio < 2.3


def test_theta_one_is_backward_euler(pkg):
    p = pkg.PoissonEllipse(M=40, N=40, sigma=2.0)
    ts = pkg.ThetaScheme(p, 1e-2, theta=1, backend="cpu")
    be = pkg.BackwardEuler(p, 1e-2, backend="cpu")
    assert ts.problem == be.problem and ts.session is None
    g = fields(40, 40, seed=3)[1]
    u = v = np.zeros((41, 41))
    for _ in range(3):
        u, v = ts.step(u, g), be.step(v, g)
        assert u.tobytes() == v.tobytes() and ts.last["iters"] == be.last["iters"] > 1
    assert ts.step(u).tobytes() == be.step(v).tobytes()  # no source


def test_refusals(pkg):
    p = pkg.PoissonEllipse(M=40, N=40)
    for theta in (0.0, -0.5, 1.0000001, 2, float("nan"), float("inf"), "0.5", None):
        with pytest.raises(ValueError, match="theta"):
            pkg.ThetaScheme(p, 1e-2, theta=theta, backend="cpu")
    for dt in (0.0, -1.0, float("nan"), float("inf"), "1"):
        with pytest.raises(ValueError, match="dt"):
            pkg.ThetaScheme(p, dt, backend="cpu")
    x, y = fields(40, 40)
    with pytest.raises(ValueError, match="overlap"):
        p.apply(x, x)
    wide = np.zeros((41, 82))
    with pytest.raises(ValueError, match="overlap"):
        p.apply(wide[:, :41], wide[:, 20:61])
    for bad in (x[:-1], x[:, :-1], x[None], x.astype(np.float32), x.tolist()):
        with pytest.raises(ValueError):
            p.apply(bad)
        with pytest.raises(ValueError):
            p.apply(x, y=bad)
        with pytest.raises(ValueError):
            p.apply(x, bad)
    with pytest.raises(ValueError):
        p.apply(None)
    ro = np.zeros((41, 41))
    ro.flags.writeable = False
    with pytest.raises(ValueError, match="read-only"):
        p.apply(x, ro)
    for name in ("alpha", "beta", "gamma", "const"):
        for v in (float("nan"), float("inf"), "1"):
            with pytest.raises(ValueError, match=name):
                p.apply(x, y=y, **{name: v})
    # CPU tensors are host arrays; a strided view is read in place of a copy
    assert np.array_equal(p.apply(torch.from_numpy(x)), p.apply(x))
    wide[:, :41] = x
    assert np.array_equal(p.apply(wide[:, :41]), p.apply(x))
