"""The operator apply on device tensors -- Session.apply over k_apply (apply_kernels.hip) -- and pmx.ThetaScheme
on the device.

The yardstick of the operator is the host twin PoissonEllipse.apply (checked against the PyTorch reference in
test_apply.py) under that test's pointwise bound 32 * 2^-53 * E; everything else about Session.apply --
decompositions, storage types, strides, streams -- is compared bitwise with its own one-subdomain fp64 result.
"""
import numpy as np
import pytest
import torch

from test_apply import SCALARS, U53, boundary_is_zero, fields, torch_reference
from test_gpu_init_data import ALGOS, _session
from test_init_data import manufactured

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
# k_apply's workgroup tile is 32 rows x 256 columns: 300 x 530 has 301 rows = 10 tiles and 531 columns = 3 tiles,
# both partial at the end; 97 x 130 has row stride 131 (odd) and 4 row tiles; 40 x 40 one partial tile
GRIDS = [(40, 40), (97, 130), (300, 530)]
SPLITS = [(1, "reference"), (2, "reference"), (4, "reference"), (4, "rows")]


@pytest.fixture(scope="module", autouse=True)
def gpu(pkg):
    assert torch.cuda.is_available() and pkg.load_native().device_count() > 0, "no HIP device"


@pytest.fixture(scope="module")
def host(pkg):
    """Per (grid, sigma), computed once and never modified: x, y, the host apply with SCALARS and with the
    defaults, and the bound's magnitude E."""
    out = {}
    for grid in GRIDS:
        x, y = fields(*grid)
        for sigma in (0.0, 100.0):
            p = pkg.PoissonEllipse(M=grid[0], N=grid[1], sigma=sigma)
            _, E = torch_reference(pkg, p, x, y, **SCALARS)
            _, E0 = torch_reference(pkg, p, x, y, 1.0, 0.0, 0.0, 0.0)
            out[grid, sigma] = dict(p=p, x=x, y=y, full=p.apply(x, y=y, **SCALARS), plain=p.apply(x), E=E, E0=E0)
    return out


def dev(a):
    return torch.from_numpy(a).to(DEV)


@pytest.mark.parametrize("sigma", [0.0, 100.0])
@pytest.mark.parametrize("grid", GRIDS)
def test_operator(pkg, host, grid, sigma):
    """Session.apply against PoissonEllipse.apply under 32 * 2^-53 * E, with all four scalars and y, and with the
    defaults; every decomposition and every storage type bitwise the one-subdomain fp64 result."""
    h = host[grid, sigma]
    p, N1 = h["p"], grid[1] + 1
    x, y = dev(h["x"]), dev(h["y"])
    first = None
    for ranks, split in SPLITS:
        s = pkg.make_session(p, ranks=ranks, split=split)
        out = torch.full_like(x, float("nan"))
        assert s.apply(x, out, y=y, **SCALARS) is out
        got = (out.cpu().numpy(), s.apply(x).cpu().numpy())
        if first is None:
            first = got
            for name, g, E in (("full", got[0], h["E"]), ("plain", got[1], h["E0"])):
                err = np.abs(g - h[name])[1:-1, 1:-1]
                print(f"{grid} sigma {sigma} {name}: max err/E {float((err / E).max()) / U53:.3g} x 2^-53, bitwise "
                      f"{np.array_equal(g, h[name])}")
                assert boundary_is_zero(g) and np.isfinite(g).all()
                assert (err <= 32 * U53 * E).all()
                # sigma = 0: the same operations in the same order on both sides, so the results are equal
                # bitwise; sigma enters as one fma on the device and as a product and a sum on the host
                # (measured: up to 1.94 * 2^-53 * E apart at 300 x 530)
                if sigma == 0.0:
                    assert np.array_equal(g, h[name])
        else:
            assert np.array_equal(got[0], first[0]) and np.array_equal(got[1], first[1]), (ranks, split)
    for dtype in ("fp32", "mixed"):
        s = pkg.make_session(p, dtype=dtype)
        assert np.array_equal(s.apply(x, y=y, **SCALARS).cpu().numpy(), first[0]), dtype
    # out may be y
    buf = y.clone()
    assert s.apply(x, buf, y=buf, **SCALARS) is buf and np.array_equal(buf.cpu().numpy(), first[0])
    if grid != (97, 130):
        return
    s = pkg.make_session(p, ranks=4)
    # [:, :N+1] views of wider tensors: the same values, and the padding columns of out stay as they were
    wx = torch.full((grid[0] + 1, N1 + 5), float("nan"), dtype=torch.float64, device=DEV)
    wy = torch.full((grid[0] + 1, N1 + 2), float("inf"), dtype=torch.float64, device=DEV)
    wo = torch.full((grid[0] + 1, N1 + 3), float("nan"), dtype=torch.float64, device=DEV)
    wx[:, :N1], wy[:, :N1] = x, y
    assert not wx[:, :N1].is_contiguous()
    s.apply(wx[:, :N1], wo[:, :N1], y=wy[:, :N1], **SCALARS)
    ho = wo.cpu().numpy()
    assert np.array_equal(ho[:, :N1], first[0]) and np.isnan(ho[:, N1:]).all()
    # NaN on the four boundary lines of x: never loaded
    xn = x.clone()
    xn[0, :] = xn[-1, :] = float("nan")
    xn[:, 0] = xn[:, -1] = float("nan")
    for t in (s, pkg.make_session(p)):
        assert np.array_equal(t.apply(xn, y=y, **SCALARS).cpu().numpy(), first[0])


@pytest.mark.parametrize("ranks", [1, 4])
@pytest.mark.parametrize("cfg", ALGOS)
def test_non_interference(pkg, cfg, ranks):
    """init, 7 iterations, an apply, 7 iterations: the state, the solution and the count of the run without
    the apply, bitwise, and no device memory taken."""
    grid = (97, 130)
    x = dev(fields(*grid)[0])

    def run(with_apply):
        s = _session(pkg, grid, cfg, ranks)
        before = s.device_bytes
        s.init()
        s.step(7)
        if with_apply:
            s.apply(x)
            s.apply(x, y=x, **SCALARS)
        s.step(7)
        st = [s.state(i) for i in range(s.num_local)]
        assert s.device_bytes == before
        return st, s.w_tensor().cpu().numpy()

    (want, w_want), (got, w_got) = run(False), run(True)
    assert got == want
    assert np.array_equal(w_got, w_want) and w_want.any()


def _produce(src):
    """src through a chain of kernels that takes far longer than a launch and returns src's values exactly: a
    consumer that does not wait for the chain reads NaN."""
    out = torch.full_like(src, float("nan"))
    d = torch.ones(2048, 2048, dtype=torch.float64, device=src.device)
    for _ in range(6):
        d = (d @ d) * 1e-4  # stays finite and decays
    out.copy_(src + 0.0 * d[0, 0])
    return out


@pytest.mark.parametrize("ranks", [1, 4])
def test_stream_order(pkg, host, ranks):
    h = host[(97, 130), 100.0]
    s = pkg.make_session(h["p"], ranks=ranks)
    x, y = dev(h["x"]), dev(h["y"])
    want = s.apply(x, y=y, **SCALARS)
    torch.cuda.synchronize()
    total = want.sum().item()
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        out = s.apply(_produce(x), y=_produce(y), **SCALARS)
        got = out.sum()  # no synchronisation in between
        assert got.item() == total
    assert np.array_equal(out.cpu().numpy(), want.cpu().numpy())
    torch.cuda.current_stream(DEV).wait_stream(side)


@pytest.mark.parametrize("sigma", [0.0, 100.0])
def test_residual_identity(pkg, sigma):
    """sqrt(h1 h2 sum (mask f - apply(w))^2) formed with torch is Session.residual_norm(f): the same values
    summed in another order."""
    p = pkg.PoissonEllipse(M=97, N=130, sigma=sigma)
    f = manufactured(p)[0]
    f_dev = dev(f)
    s = pkg.make_session(p, algo="pcg1", block_tiles=0)
    assert s.solve(rhs=f_dev)["status"] == "converged"
    r = dev(np.where(p.inside_mask(), f, 0.0)) - s.apply(s.w_tensor())
    mine = float(torch.sqrt(p.h1 * p.h2 * (r[1:-1, 1:-1] ** 2).sum()))
    want = s.residual_norm(f_dev)
    print(f"sigma {sigma}: {mine:.17e} vs {want:.17e}")
    assert want > 0 and abs(mine - want) <= 1e-12 * want


@pytest.mark.parametrize("ranks", [1, 4])
def test_theta_scheme_on_the_device(pkg, ranks):
    """3 Crank-Nicolson steps from u = 0 with g = 1 on device tensors against the same scheme on the CPU oracle:
    equal counts per step, fields to 1e-10 max|u| (the bound of the GPU-vs-oracle tests)."""
    p = pkg.PoissonEllipse(M=97, N=130)
    ts = pkg.ThetaScheme(p, 1e-3, theta=0.5, ranks=ranks)
    cpu = pkg.ThetaScheme(p, 1e-3, theta=0.5, backend="cpu")
    assert ts.problem.sigma == 2000.0 and ts.session.algo_name == "pcg1" and ts.session.num_local == ranks
    u = torch.zeros(98, 131, dtype=torch.float64, device=DEV)
    v = np.zeros((98, 131))
    for n in range(3):
        u, v = ts.step(u, 1.0), cpu.step(v, 1.0)
        assert isinstance(u, torch.Tensor) and u.is_cuda and u.dtype == torch.float64
        err = np.abs(u.cpu().numpy() - v).max()
        print(f"step {n + 1}: iters {ts.last['iters']} / {cpu.last['iters']}, max|u - u_cpu| {err:.3e}, max u {v.max():.6e}")
        assert ts.last["iters"] == cpu.last["iters"] and ts.last["status"] == "converged"
        assert err <= 1e-10 * np.abs(v).max()
    # a device tensor as the source is the scalar's step
    g = torch.ones_like(u)
    assert np.abs((ts.step(u, g) - ts.step(u, 1.0)).cpu().numpy()).max() <= 1e-10 * np.abs(v).max()


def test_refusals(pkg):
    p = pkg.PoissonEllipse(M=40, N=60)
    s = pkg.make_session(p, ranks=4)
    x = torch.ones(41, 61, dtype=torch.float64, device=DEV)
    want = s.apply(x).cpu().numpy()
    wide = torch.ones(41, 130, dtype=torch.float64, device=DEV)
    bad_calls = [
        dict(x=x, out=torch.ones(41, 61, dtype=torch.float64)),        # a CPU tensor for out
        dict(x=x, out=np.ones((41, 61))),
        dict(x=x.cpu()),
        dict(x=x.float()), dict(x=x, out=x.float()), dict(x=x, y=x.float()),  # float32
        dict(x=x, out=x),                                               # out is x
        dict(x=wide[:, :61], out=wide[:, 30:91]),                       # out overlaps x
        dict(x=x[:, :60]), dict(x=x, out=x.clone()[:40]), dict(x=x, y=x.t().contiguous().t()),
        dict(x=x, alpha=float("nan")), dict(x=x, const=float("inf")),
        dict(x=None),
    ]
    for kw in bad_calls:
        with pytest.raises(ValueError):
            s.apply(**kw)
    if torch.cuda.device_count() > 1:
        with pytest.raises(ValueError):
            s.apply(x.to("cuda:1"))
    # the session is still usable, and still the default one
    assert np.array_equal(s.apply(x).cpu().numpy(), want)
    assert s.solve()["status"] == "converged"
    with pytest.raises(ValueError, match="theta"):
        pkg.ThetaScheme(p, 1e-3, theta=1.5)
    with pytest.raises(ValueError):  # the host apply rejects device tensors, as field() does
        p.apply(x)
