"""A user-supplied right-hand side and initial guess on the CPU paths: the native oracle (serial,
OpenMP, decomposed) and the plain-PyTorch PCG.

Manufactured problem on the reference ellipse: u = (1 - x^2 - 4y^2)(1 + x/2 + y) in D, u = 0 on its
boundary, so -Laplace(u) = f = 10 + 7x + 26y; f changes sign in D and has no symmetry.  The solver
applies the ellipse mask itself (B = f inside D, 0 elsewhere), as it does for the constant F.
"""
import numpy as np
import pytest
import torch

from conftest import sub

GRIDS = [(40, 60), (97, 130)]
# iterations to delta = 1e-6: constant F, manufactured f, manufactured f from w0 = 10 w_const
COUNTS = {(40, 60): (68, 114, 82), (97, 130): (143, 242, 168)}
# constant F continued from the delta = 1e-6 solution to delta = 1e-9: warm, cold
CONTINUE = {(40, 60): (39, 104), (97, 130): (90, 221)}


def manufactured(p):
    """(f, u) on the (M+1) x (N+1) grid; u is zero outside D."""
    x, y = p.coords()
    X, Y = np.meshgrid(x, y, indexing="ij")
    f = 10.0 + 7.0 * X + 26.0 * Y
    u = np.where(p.inside_mask(), (1.0 - X * X - 4.0 * Y * Y) * (1.0 + 0.5 * X + Y), 0.0)
    return f, u


@pytest.fixture(scope="module")
def const_solution(pkg):
    """The converged constant-F solve (delta = 1e-6) of every grid, computed once."""
    return {g: pkg.solve(pkg.PoissonEllipse(M=g[0], N=g[1]), "cpu") for g in GRIDS}


def _torch(pkg, p, **kw):
    return sub("models.torch_pcg").TorchPCG(p).solve(**kw)


@pytest.mark.parametrize("grid", GRIDS)
def test_c1_default_data_is_the_default_solve(pkg, const_solution, grid):
    """rhs = F everywhere and w0 = 0 are the solve without data: same count, bitwise equal w.

    The OpenMP oracle is the exception: its reductions combine the threads' sums in arrival order, so
    two identical plain runs already differ in the last bits (max |dw| ~ 1e-17 at 40x60).  There the
    count is equal and w agrees to 1e-10 max|w|, the bound the GPU-vs-oracle tests use for sums taken in
    another order."""
    p = pkg.PoissonEllipse(M=grid[0], N=grid[1])
    shape = (p.M + 1, p.N + 1)
    data = dict(rhs=np.full(shape, p.F), w0=np.zeros(shape))
    ref = const_solution[grid]
    assert ref.iters == COUNTS[grid][0]
    omp = pkg.solve(p, "omp", threads=3, **data)
    assert omp.iters == ref.iters and omp.converged
    assert np.abs(omp.w - ref.w).max() <= 1e-10 * np.abs(ref.w).max()
    runs = [
        (pkg.solve(p, "cpu", **data), ref),
        (pkg.solve(p, "cpu-decomposed", ranks=4, **data), pkg.solve(p, "cpu-decomposed", ranks=4)),
        (_torch(pkg, p, **data), _torch(pkg, p)),
        (pkg.solve(p, "cpu", rhs=data["rhs"]), ref),
        (pkg.solve(p, "cpu", w0=data["w0"]), ref),
    ]
    for got, want in runs:
        assert got.iters == want.iters and got.status == want.status == "converged"
        assert np.array_equal(got.w, want.w)


@pytest.mark.parametrize("grid", GRIDS)
def test_c2_manufactured_counts(pkg, const_solution, grid):
    p = pkg.PoissonEllipse(M=grid[0], N=grid[1])
    f, _ = manufactured(p)
    cold = pkg.solve(p, "cpu", rhs=f)
    warm = pkg.solve(p, "cpu", rhs=f, w0=10.0 * const_solution[grid].w)
    assert (cold.iters, warm.iters) == COUNTS[grid][1:]
    assert cold.status == warm.status == "converged"
    # every CPU path solves the same problem: the decomposed oracle and the PyTorch PCG agree
    for other in (pkg.solve(p, "cpu-decomposed", ranks=4, rhs=f), _torch(pkg, p, rhs=f),
                  pkg.solve(p, "omp", threads=3, rhs=f)):
        assert other.iters == cold.iters
        assert np.abs(other.w - cold.w).max() <= 1e-10 * np.abs(cold.w).max()
    for other in (pkg.solve(p, "cpu-decomposed", ranks=4, rhs=f, w0=10.0 * const_solution[grid].w),
                  _torch(pkg, p, rhs=f, w0=10.0 * const_solution[grid].w)):
        assert other.iters == warm.iters
        assert np.abs(other.w - warm.w).max() <= 1e-10 * np.abs(warm.w).max()


def test_c2_manufactured_error_falls_with_refinement(pkg):
    """The fictitious-domain scheme is first order: the L2 error against u roughly halves per
    refinement (0.47-0.55 measured); below 0.7 between 40x60 and 80x120 leaves slack for the early stop."""
    err = []
    for M, N in [(40, 60), (80, 120)]:
        p = pkg.PoissonEllipse(M=M, N=N)
        f, u = manufactured(p)
        r = pkg.solve(p, "cpu", rhs=f)
        assert r.converged
        err.append(p.error_norms(r.w, exact=u)["l2_error"])
    print("manufactured L2 errors", err)
    assert 0.0 < err[1] < 0.7 * err[0]
    # the default (analytic constant-F solution) is unchanged by the new argument
    p = pkg.PoissonEllipse(M=40, N=60)
    w = pkg.solve(p, "cpu").w
    x, y = p.coords()
    X, Y = np.meshgrid(x, y, indexing="ij")
    assert p.error_norms(w) == p.error_norms(w, exact=p.exact_solution(X, Y))


@pytest.mark.parametrize("grid", GRIDS)
def test_c3_warm_start(pkg, const_solution, grid):
    M, N = grid
    p = pkg.PoissonEllipse(M=M, N=N)
    conv = const_solution[grid]
    again = pkg.solve(p, "cpu", w0=conv.w)
    assert again.iters == 1 and again.converged
    f, _ = manufactured(p)
    assert pkg.solve(p, "cpu", rhs=f, w0=pkg.solve(p, "cpu", rhs=f).w).iters == 1
    tight = pkg.PoissonEllipse(M=M, N=N, delta=1e-9)
    warm = pkg.solve(tight, "cpu", w0=conv.w)
    cold = pkg.solve(tight, "cpu")
    assert (warm.iters, cold.iters) == CONTINUE[grid]
    # (at delta = 1e-9 the warm runs end on the reference's |(A p, p)| < 1e-15 guard with a last step of
    # 1.4-1.6e-9, not on the stop test; so does the cold run at 40x60)
    assert warm.iters < cold.iters and warm.status == "breakdown"
    d = np.abs(warm.w - cold.w).max()
    print("continuation vs cold, max norm:", d)
    assert d <= 1e-6
    # the same continuation through the decomposed oracle and the PyTorch PCG
    assert pkg.solve(tight, "cpu-decomposed", ranks=4, w0=conv.w).iters == warm.iters
    assert _torch(pkg, tight, w0=torch.from_numpy(conv.w)).iters == warm.iters


@pytest.mark.parametrize("backend", ["cpu", "cpu-decomposed", "torch"])
@pytest.mark.parametrize("arg", ["rhs", "w0"])
def test_c4_bad_input(pkg, backend, arg):
    p = pkg.PoissonEllipse(M=40, N=60)
    good = np.ones((41, 61))
    nan = good.copy()
    nan[20, 30] = np.nan
    inf = good.copy()
    inf[3, 3] = np.inf
    for bad in (np.ones((40, 61)), np.ones((41, 61, 1)), np.ones(41 * 61), good.astype(np.float32), nan, inf,
                good.tolist(), torch.ones(41, 61, dtype=torch.float32)):
        with pytest.raises(ValueError):
            pkg.solve(p, backend, **{arg: bad})
    with pytest.raises(ValueError):
        p.error_norms(good, exact=good.astype(np.float32))
    # non-contiguous views and CPU tensors are accepted
    wide = np.ones((41, 122))
    assert pkg.solve(p, backend, **{arg: wide[:, ::2]}).iters == pkg.solve(p, backend, **{arg: good}).iters
    assert pkg.solve(p, backend, **{arg: torch.from_numpy(good)}).iters == \
        pkg.solve(p, backend, **{arg: good}).iters
