"""The screened problem (-Δ + σ) u = f on the GPU: k_init and k_pcg1 built with the σ flag (pcg_kernels.hip,
pcg1_kernels.hip), the algorithm choice and its refusals, and BackwardEuler on device tensors.

Manufactured problem as in test_sigma.py: u = (1 - x^2 - 4y^2)(1 + x/2 + y), f = 10 + 7x + 26y + σ u.
"""
import numpy as np
import pytest
import torch

from conftest import sub
from test_sigma import problem, screened

pytestmark = pytest.mark.gpu

SIGMAS = [1.0, 100.0, 1e4]
GRIDS = [(97, 130), (40, 40)]
DECOMP = [(1, "reference"), (2, "reference"), (2, "rows"), (4, "reference"), (4, "rows")]


@pytest.fixture(scope="module", autouse=True)
def gpu(pkg):
    assert torch.cuda.is_available() and pkg.load_native().device_count() > 0, "no HIP device"


@pytest.fixture(scope="module")
def oracle(pkg):
    """CPU oracle solves shared by the tests: per grid and sigma, the manufactured and the constant rhs."""
    out = {}
    for grid in GRIDS:
        for sigma in SIGMAS:
            p = problem(pkg, sigma, grid)
            f, _ = screened(p)
            out[(grid, sigma)] = dict(p=p, f=f, manuf=pkg.solve(p, "cpu", rhs=f), const=pkg.solve(p, "cpu"))
    return out


@pytest.fixture(scope="module")
def storage_gap(pkg):
    """What fp32 / mixed storage shows at sigma = 0 on a grid (as tests/test_gpu_init_data.py test_g4 takes
    it): d = max|w_dtype - w_fp64| of the constant-F solve on the pcg1 march, and max|w_fp64|."""
    cache = {}

    def get(grid, dtype):
        if (grid, dtype) not in cache:
            p = pkg.PoissonEllipse(M=grid[0], N=grid[1])
            w = {}
            for dt in ("fp64", dtype):
                s = pkg.make_session(p, algo="pcg1", block_tiles=0, dtype=dt)
                assert s.solve()["status"] == "converged"
                w[dt] = s.gather_local_w()
            cache[(grid, dtype)] = (float(np.abs(w[dtype] - w["fp64"]).max()), float(np.abs(w["fp64"]).max()))
        return cache[(grid, dtype)]

    return get


def _host_residual(p, w, rhs):
    """sqrt(h1 h2 sum (B - (A + σ I) w)^2) and (z, r) = h1 h2 sum r^2 / (D + σ), r = B - (A + σ I) w, in fp64
    with ops/reference.py."""
    R = sub("ops.reference")
    sd = sub("parallel.decomp").subdomain(p.M, p.N, 1, 1, 0)
    a, b, _ = R.assemble(p, sd)
    a, b = a.numpy(), b.numpy()
    B = np.where(p.inside_mask(), rhs, 0.0)[1:-1, 1:-1]
    res = B - R.apply_A(w, a, b, p.h1, p.h2, p.sigma)
    zr = (res * res / R.diag(a, b, p.h1, p.h2, p.sigma)).sum() * p.h1 * p.h2
    return float(np.sqrt((res * res).sum() * p.h1 * p.h2)), float(zr)


@pytest.mark.parametrize("sigma", [0.0, 3.5, 1e4])
@pytest.mark.parametrize("grid", [(97, 130), (33, 70)])
def test_operator(pkg, grid, sigma):
    """One init(rhs, w0) with random data: the device residual of w0 is ||B - (A + σ I) w0|| (k_init's measure
    mode), and the (z0, r0) the first sweep reduces is that of r0 = B - (A + σ I) w0 with D + σ (k_init's
    data mode feeding k_pcg1's sweep 0)."""
    p = problem(pkg, sigma, grid)
    rng = np.random.default_rng(7)
    shape = (p.M + 1, p.N + 1)
    f = rng.standard_normal(shape)
    w0 = np.zeros(shape)
    w0[1:-1, 1:-1] = rng.standard_normal((p.M - 1, p.N - 1))
    s = pkg.make_session(p, algo="pcg1", block_tiles=0)
    s.init(rhs=f, w0=w0)
    s.synchronize()
    want, zr = _host_residual(p, w0, f)
    got = s.residual_norm(f)
    got_zr = s.state(0)["red_c"][0]
    print(f"{grid} sigma {sigma}: residual device {got:.16e} host {want:.16e}; (z0, r0) device {got_zr:.16e} host {zr:.16e}")
    assert abs(got - want) <= 1e-12 * want
    assert abs(got_zr - zr) <= 1e-12 * zr
    if sigma:  # and the shift is in both: the unshifted values lie 1000 tolerances away or more (the random
        # w0 makes A w0 ~ 1e7, so sigma = 3.5 moves the norms by 4e-8 of their size)
        p0 = problem(pkg, 0.0, grid)
        plain, zr0 = _host_residual(p0, w0, f)
        assert abs(got - plain) > 1e-9 * want and abs(got_zr - zr0) > 1e-9 * zr


@pytest.mark.parametrize("dtype", ["fp64", "mixed", "fp32"])
@pytest.mark.parametrize("sigma", SIGMAS)
@pytest.mark.parametrize("grid", GRIDS)
def test_solve_against_the_cpu_oracle(pkg, oracle, storage_gap, grid, sigma, dtype):
    """Both right-hand sides on 1, 2 and 4 subdomains, split by the reference rule and into row strips.
    fp64: the oracle's count and 1e-10 max|w|, the bound of the GPU-vs-oracle tests.  fp32 / mixed: the
    count is printed, and w is as close to the oracle as that storage is to fp64 at sigma = 0 on this grid
    (storage_gap), scaled by the solutions' sizes with test_g4's margin of 4."""
    o = oracle[(grid, sigma)]
    for name in ("manuf", "const"):
        ref = o[name]
        top = np.abs(ref.w).max()
        if dtype == "fp64":
            bound = 1e-10 * top
        else:
            d, top0 = storage_gap(grid, dtype)
            assert d > 0.0
            bound = 4.0 * d * top / top0
        for ranks, split in DECOMP:
            s = pkg.make_session(o["p"], ranks=ranks, split=split, dtype=dtype)
            assert s.algo_name == "pcg1" and s.tile["algo"] == "pcg1" and not s.tile.get("block_tiles")
            r = s.solve(rhs=o["f"] if name == "manuf" else None)
            err = np.abs(s.gather_local_w() - ref.w).max()
            print(f"{grid} sigma {sigma} {dtype} {name} ranks {ranks} {split}: iters {r['iters']} (oracle {ref.iters}) "
                  f"max|w - w_cpu| {err:.3e} bound {bound:.3e}")
            assert r["status"] == "converged"
            if dtype == "fp64":
                assert r["iters"] == ref.iters
            assert err <= bound


def test_solve_400x600(pkg):
    """w triples with all three w-cycle phases across several graph batches, on a grid of many tiles."""
    p = problem(pkg, 100.0, (400, 600))
    ref = pkg.solve(p, "cpu")
    s = pkg.make_session(p)
    r = s.solve()
    err = np.abs(s.gather_local_w() - ref.w).max()
    print(f"400x600 sigma 100: iters {r['iters']} (oracle {ref.iters}) max|w - w_cpu| {err:.3e}")
    assert s.algo_name == "pcg1" and not s.tile.get("block_tiles") and s.state(0)["w_cycle"] == 3
    assert r["iters"] == ref.iters > 3 * 32 and r["status"] == "converged"
    assert err <= 1e-10 * np.abs(ref.w).max()


@pytest.mark.parametrize("grid,kw", [((97, 130), {}), ((400, 600), dict(algo="pcg1")), ((400, 600), dict(algo="pcg2")),
                                     ((400, 600), dict(algo="ca"))])
def test_sigma_zero_changes_nothing(pkg, grid, kw):
    def run(p):
        s = pkg.make_session(p, **kw)
        r = s.solve()
        return r["iters"], r["status"], s.gather_local_w(), s.device_bytes, s.tile

    plain = run(pkg.PoissonEllipse(M=grid[0], N=grid[1]))
    zero = run(problem(pkg, 0.0, grid))
    assert zero[:2] == plain[:2] and plain[1] == "converged"
    assert zero[2].tobytes() == plain[2].tobytes()
    assert zero[3] == plain[3] and zero[4] == plain[4]
    if not kw:
        assert plain[4].get("block_tiles")  # auto at 97 x 130: the block tiles, as before


def test_refusals(pkg, tmp_path):
    """Every option that is not built for sigma raises ValueError naming it, before anything is allocated:
    the refused sessions would hold ~0.25 GB each."""
    big = problem(pkg, 2.0, (2000, 3000))
    small = problem(pkg, 2.0, (97, 130))
    pkg.make_session(small).solve()  # the device is initialised
    free0 = torch.cuda.mem_get_info()[0]
    for kw, name in ((dict(algo="ca"), "ca"), (dict(algo="pcg2"), "pcg2"), (dict(exact=True), "exact"),
                     (dict(block_tiles=1), "block_tiles")):
        for ranks in (1, 2):
            with pytest.raises(ValueError, match=name):
                pkg.make_session(big, ranks=ranks, **kw)
    with pytest.raises(ValueError, match="sigma"):
        sub("ops.kernels").DeviceOps(big)
    with pytest.raises(ValueError, match="sigma"):
        pkg.load_native().OpContext(big.to_native(), 1, 1, 0, 3002, 0)
    with pytest.raises(ValueError, match="sigma"):
        pkg.load_native().SubdomainSolver(big.to_native())
    with pytest.raises(ValueError, match="sigma"):
        pkg.load_native().comm_layout(big.to_native(), 1, 1, 0)
    assert free0 - torch.cuda.mem_get_info()[0] < 100 << 20
    # block_tiles=-1 resolves to off, auto to pcg1
    s = pkg.make_session(small, block_tiles=-1)
    assert s.algo_name == "pcg1" and not s.tile.get("block_tiles")
    # checkpoints do not record sigma; the analytic error does not hold
    ck = str(tmp_path / "sigma.ck")
    want = s.solve()
    w = s.gather_local_w()
    with pytest.raises(ValueError, match="sigma"):
        s.save_checkpoint(ck)
    with pytest.raises(ValueError, match="sigma"):
        s.load_checkpoint(ck)
    with pytest.raises(ValueError, match="sigma"):
        s.solve_checkpointed(ck, every=16)
    with pytest.raises(ValueError, match="sigma"):
        s.error_norms()
    assert not (tmp_path / "sigma.ck").exists()
    again = s.solve()  # the session is untouched
    assert again["iters"] == want["iters"] and np.array_equal(s.gather_local_w(), w)


def test_backward_euler_three_steps(pkg):
    """3 steps from u = 0 with g = 1 on device tensors against 3 oracle solves chained on the host."""
    p = pkg.PoissonEllipse(M=97, N=130)
    dt = 1e-3
    be = pkg.BackwardEuler(p, dt)
    assert be.session.algo_name == "pcg1" and be.problem.sigma == 1.0 / dt
    u = torch.zeros(98, 131, dtype=torch.float64, device="cuda")
    g = torch.ones_like(u)
    host = np.zeros((98, 131))
    ps = problem(pkg, 1.0 / dt)
    for n in range(3):
        u = be.step(u, g)
        assert isinstance(u, torch.Tensor) and u.is_cuda and u.dtype == torch.float64
        host = pkg.solve(ps, "cpu", rhs=host / dt + 1.0, w0=host).w
        err = np.abs(u.cpu().numpy() - host).max()
        print(f"step {n + 1}: iters {be.last['iters']} max|u - u_cpu| {err:.3e} max u {host.max():.6e}")
        assert err <= 1e-10 * np.abs(host).max()
    # NumPy in, NumPy out: the same step (the two right-hand sides are formed by different divisions)
    v = be.step(u.cpu().numpy(), 1.0)
    assert isinstance(v, np.ndarray) and v.shape == (98, 131)
    assert np.abs(v - be.step(u, g).cpu().numpy()).max() <= 1e-10 * np.abs(v).max()


def test_backward_euler_reaches_the_steady_state(pkg):
    """Stepped until max|u+ - u| < 1e-9, u approaches the solution of the sigma = 0 problem.  The two stop on
    different quantities (the time stepping ends when a step's solve moves nothing: its first (A p, p) falls
    below the breakdown guard), so they agree only to a gap.  Measured with the CPU oracle at this grid, dt and
    delta: 763 steps, max|u - w_steady| = 2.235e-6 (max w 0.0992); the bound is 10x that."""
    gap_cpu = 2.235e-6
    p = pkg.PoissonEllipse(M=97, N=130, delta=1e-9)
    steady = pkg.solve(p, "hip", keep_solution="device")
    assert steady.converged
    be = pkg.BackwardEuler(p, 1e-3)
    u = torch.zeros(98, 131, dtype=torch.float64, device="cuda")
    g = torch.ones_like(u)
    gaps, steps = [], 0
    while True:
        v = be.step(u, g)
        steps += 1
        d = float((v - u).abs().max())
        u = v
        if steps in (1, 10, 100):
            gaps.append(float((u - steady.w).abs().max()))
        if d < 1e-9:
            break
        assert steps < 3000, "the time stepping does not settle"
    gap = float((u - steady.w).abs().max())
    print(f"{steps} steps, gaps after 1 / 10 / 100 steps {gaps}, final {gap:.3e} (CPU oracle: 763 steps, {gap_cpu:.3e})")
    assert gaps[0] > gaps[1] > gaps[2] > gap
    assert gap <= 10.0 * gap_cpu
