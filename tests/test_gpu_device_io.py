"""Device-resident rhs, w0 and solution: float64 tensors of the session's device go into Session.init /
solve / residual_norm and come out of Session.w_tensor through the scatter, finite-check and gather kernels
(io_kernels.hip), never through the host.

The yardstick is this package's own host-array path: every comparison is bitwise, so there is no tolerance.
Grids 97x130 and 40x60: odd row strides, tiles that do not divide, all four splits.
"""
import numpy as np
import pytest
import torch

from test_gpu_init_data import ALGOS, CONFIGS, DEVICE_BYTES, RANKS, _session
from test_init_data import CONTINUE, COUNTS, GRIDS, manufactured

pytestmark = pytest.mark.gpu

DTYPES = ["fp64", "fp32", "mixed"]
DEV = "cuda:0"


@pytest.fixture(scope="module", autouse=True)
def gpu(pkg):
    assert torch.cuda.is_available() and pkg.load_native().device_count() > 0, "no HIP device"


@pytest.fixture(scope="module")
def data(pkg):
    """Per grid, computed once and never modified: the manufactured f and w0 = 10 w_const as NumPy arrays
    and as tensors on the device."""
    out = {}
    for M, N in GRIDS:
        p = pkg.PoissonEllipse(M=M, N=N)
        f, _ = manufactured(p)
        w0 = 10.0 * pkg.solve(p, "cpu").w
        out[(M, N)] = dict(f=f, w0=w0, f_dev=torch.from_numpy(f).to(DEV), w0_dev=torch.from_numpy(w0).to(DEV))
    torch.cuda.synchronize()
    return out


def _solve(pkg, grid, cfg, ranks, dtype, **kw):
    s = _session(pkg, grid, cfg, ranks, dtype=dtype)
    r = s.solve(**kw)
    return (r["iters"], r["status"], r["diff"]), s.gather_local_w()


def _in_bitwise(pkg, data, cfg, dtype, ranks):
    grid = (97, 130)
    d = data[grid]
    for host, dev in ((dict(rhs=d["f"], w0=d["w0"]), dict(rhs=d["f_dev"], w0=d["w0_dev"])),
                      (dict(rhs=d["f"]), dict(rhs=d["f_dev"])),
                      (dict(w0=d["w0"]), dict(w0=d["w0_dev"]))):
        want, w_want = _solve(pkg, grid, cfg, ranks, dtype, **host)
        got, w_got = _solve(pkg, grid, cfg, ranks, dtype, **dev)
        assert got == want, (list(dev), got, want)
        assert np.array_equal(w_got, w_want), list(dev)
        assert want[0] > 1


@pytest.mark.parametrize("ranks", [1, 4])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("cfg", list(CONFIGS))
def test_d1_in_bitwise(pkg, data, cfg, dtype, ranks):
    """solve(rhs=f_dev, w0=w0_dev), rhs alone and w0 alone: the count, status, diff and gathered w of the
    same call with the NumPy arrays."""
    _in_bitwise(pkg, data, cfg, dtype, ranks)


@pytest.mark.parametrize("ranks", [2, 3])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("cfg", ALGOS)
def test_d1_in_bitwise_strips(pkg, data, cfg, dtype, ranks):
    _in_bitwise(pkg, data, cfg, dtype, ranks)


@pytest.mark.parametrize("ranks", list(RANKS))
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("cfg", ALGOS)
def test_d2_out_bitwise_with_pending_steps(pkg, cfg, dtype, ranks):
    """w_tensor() against gather_local_w() n iterations after an init, for n that leave 0, 1 and 2 w steps
    pending in device memory (pcg1) or one (pcg2, odd n)."""
    grid = (97, 130)
    s = _session(pkg, grid, cfg, ranks, dtype=dtype)
    pend_n, pend = set(), set()
    for n in (0, 1, 2, 3, 4, 5, 64):
        s.init()
        s.step(n)
        st = s.state(0)
        pend_n.add(st["w_pend_n"] if st["w_pend"] > 0 else 0)
        pend.add(st["w_pend"] > 0)
        w = s.w_tensor()
        assert w.dtype == torch.float64 and w.device == torch.device(DEV) and w.shape == (grid[0] + 1, grid[1] + 1)
        assert np.array_equal(w.cpu().numpy(), s.gather_local_w()), n
    # a schedule change must not silently skip the pending paths
    if cfg.startswith("pcg1"):
        assert {1, 2} <= pend_n, pend_n
    if cfg.startswith("pcg2"):
        assert True in pend
    # out=: every element of the (M+1) x (N+1) block is written, the boundary as zero
    want = s.gather_local_w()
    out = torch.full((grid[0] + 1, grid[1] + 1), float("nan"), dtype=torch.float64, device=DEV)
    assert s.w_tensor(out=out) is out
    h = out.cpu().numpy()
    assert np.array_equal(h, want)
    assert not h[0].any() and not h[-1].any() and not h[:, 0].any() and not h[:, -1].any() and h.any()
    # a column-sliced view of a wider tensor: the padding columns stay as they were
    wide = torch.full((grid[0] + 1, grid[1] + 7), float("nan"), dtype=torch.float64, device=DEV)
    s.w_tensor(out=wide[:, :grid[1] + 1])
    hw = wide.cpu().numpy()
    assert np.array_equal(hw[:, :grid[1] + 1], want) and np.isnan(hw[:, grid[1] + 1:]).all()


@pytest.mark.parametrize("grid", GRIDS)
@pytest.mark.parametrize("cfg", ALGOS)
def test_d3_round_trip_on_the_device(pkg, cfg, grid):
    s = _session(pkg, grid, cfg)
    assert s.solve()["iters"] == COUNTS[grid][0]
    w = s.w_tensor()
    again = s.solve(w0=w)
    assert again["iters"] == 1 and again["status"] == "converged"
    t = _session(pkg, grid, cfg, problem=dict(delta=1e-9))
    assert t.solve(w0=w)["iters"] == CONTINUE[grid][0]


@pytest.mark.parametrize("ranks", [1, 4])
def test_d3_solve_keeps_the_solution_on_the_device(pkg, data, ranks):
    grid = (97, 130)
    d = data[grid]
    p = pkg.PoissonEllipse(M=grid[0], N=grid[1])
    host = pkg.solve(p, "hip", ranks=ranks, rhs=d["f"], w0=d["w0"])
    dev = pkg.solve(p, "hip", ranks=ranks, rhs=d["f_dev"], w0=d["w0_dev"], keep_solution="device")
    assert isinstance(host.w, np.ndarray)
    assert isinstance(dev.w, torch.Tensor) and dev.w.dtype == torch.float64 and dev.w.device == torch.device(DEV)
    assert (dev.iters, dev.status, dev.diff) == (host.iters, host.status, host.diff)
    assert np.array_equal(dev.w.cpu().numpy(), host.w)
    with pytest.raises(ValueError):
        pkg.solve(p, "hip", keep_solution="host")
    for backend in ("cpu", "torch"):  # the other backends keep rejecting device tensors
        with pytest.raises(ValueError):
            pkg.solve(p, backend, rhs=d["f_dev"])
    with pytest.raises(ValueError):
        p.field(d["f_dev"], "rhs")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("cfg", ALGOS)
def test_d4_residual_norm(pkg, data, cfg, dtype):
    """fp64 storage reads the tensor in place, fp32 storage rounds it on the device: the host path's value
    either way, with pending w steps (11 iterations) and at convergence."""
    grid = (97, 130)
    d = data[grid]
    for problem in (dict(max_iter=11), {}):
        s = _session(pkg, grid, cfg, dtype=dtype, problem=problem)
        s.solve(rhs=d["f_dev"])
        want = s.residual_norm(d["f"])
        assert s.residual_norm(d["f_dev"]) == want and want > 0.0
        wide = torch.zeros(grid[0] + 1, grid[1] + 4, dtype=torch.float64, device=DEV)
        wide[:, :grid[1] + 1] = d["f_dev"]
        assert s.residual_norm(wide[:, :grid[1] + 1]) == want


@pytest.mark.parametrize("cfg", ALGOS)
def test_d4_nothing_is_retained(pkg, data, cfg):
    grid = (97, 130)
    d = data[grid]
    s = _session(pkg, grid, cfg, placement=0)
    before = s.device_bytes
    s.solve(rhs=d["f_dev"], w0=d["w0_dev"])
    s.residual_norm(d["f_dev"])
    s.w_tensor()
    assert s.device_bytes == before == DEVICE_BYTES[cfg, "fp64", 1]


@pytest.mark.parametrize("ranks", [1, 4])
@pytest.mark.parametrize("dtype", ["fp64", "fp32"])
@pytest.mark.parametrize("cfg", ALGOS)
def test_d5_strided_input(pkg, data, cfg, dtype, ranks):
    """A [:, :N+1] view of a wider tensor as rhs and as w0 is the contiguous case, bitwise."""
    grid = (97, 130)
    d = data[grid]
    N1 = grid[1] + 1
    wide_f = torch.full((grid[0] + 1, N1 + 5), float("nan"), dtype=torch.float64, device=DEV)
    wide_w = torch.full((grid[0] + 1, N1 + 2), float("inf"), dtype=torch.float64, device=DEV)
    wide_f[:, :N1] = d["f_dev"]
    wide_w[:, :N1] = d["w0_dev"]
    assert not wide_f[:, :N1].is_contiguous()
    want, w_want = _solve(pkg, grid, cfg, ranks, dtype, rhs=d["f_dev"], w0=d["w0_dev"])
    got, w_got = _solve(pkg, grid, cfg, ranks, dtype, rhs=wide_f[:, :N1], w0=wide_w[:, :N1])
    assert got == want and np.array_equal(w_got, w_want)


def _produce(f_src):
    """f_src through a chain of kernels that takes far longer than a launch and returns f_src's values
    exactly: a consumer that does not wait for the chain reads NaN."""
    out = torch.full_like(f_src, float("nan"))
    d = torch.ones(2048, 2048, dtype=torch.float64, device=f_src.device)
    for _ in range(6):
        d = (d @ d) * 1e-4  # stays finite and decays
    out.copy_(f_src + 0.0 * d[0, 0])
    return out


@pytest.mark.parametrize("ranks", [1, 4])
@pytest.mark.parametrize("cfg", ALGOS)
def test_d6_stream_order(pkg, data, cfg, ranks):
    grid = (97, 130)
    d = data[grid]
    want, w_want = _solve(pkg, grid, cfg, ranks, "fp64", rhs=d["f"])
    # produced on the current stream, consumed with no synchronisation in between
    s = _session(pkg, grid, cfg, ranks)
    r = s.solve(rhs=_produce(d["f_dev"]))
    assert (r["iters"], r["status"], r["diff"]) == want
    # the solution is usable at once on the current stream.  The yardstick is the same torch reduction
    # of the downloaded array: same shape, dtype and device, so the same summation order
    total = s.w_tensor().sum()
    w = s.gather_local_w()
    assert np.array_equal(w, w_want)
    assert total.item() == torch.from_numpy(w).to(DEV).sum().item()
    # ... and on a side stream
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    t = _session(pkg, grid, cfg, ranks)
    with torch.cuda.stream(side):
        f = _produce(d["f_dev"])
        r = t.solve(rhs=f)
        total = t.w_tensor().sum()
        assert total.item() == torch.from_numpy(w).to(DEV).sum().item()
    assert (r["iters"], r["status"], r["diff"]) == want
    assert np.array_equal(t.gather_local_w(), w_want)
    torch.cuda.current_stream(DEV).wait_stream(side)


def _bad_tensors():
    good = torch.ones(41, 61, dtype=torch.float64, device=DEV)
    bad = {
        "float32": good.float(),
        "shape": torch.ones(41, 60, dtype=torch.float64, device=DEV),
        "3-d": torch.ones(1, 41, 61, dtype=torch.float64, device=DEV),
        "transposed": torch.ones(61, 41, dtype=torch.float64, device=DEV).t(),
    }
    for name, v in (("nan", float("nan")), ("inf", float("inf"))):
        for where, ij in (("interior", (7, 7)), ("ring", (0, 33)), ("last", (40, 60))):
            t = good.clone()
            t[ij] = v
            bad[f"{name}-{where}"] = t
    return good, bad


@pytest.mark.parametrize("ranks", [1, 4])
@pytest.mark.parametrize("arg", ["rhs", "w0"])
def test_d7_validation(pkg, arg, ranks):
    s = _session(pkg, (40, 60), "pcg1-march", ranks)
    good, bad = _bad_tensors()
    assert bad["transposed"].shape == good.shape
    for name, t in bad.items():
        with pytest.raises(ValueError):
            s.init(**{arg: t})
        with pytest.raises(ValueError):
            s.solve(**{arg: t})
        if ranks == 1 and arg == "rhs":
            with pytest.raises(ValueError):
                s.residual_norm(t)
        if not name.startswith(("nan", "inf")):
            with pytest.raises(ValueError):
                s.w_tensor(out=t)
    with pytest.raises(ValueError):
        s.w_tensor(out=np.ones((41, 61)))
    # the session is untouched: its plain solve is the default one
    assert s.solve()["iters"] == COUNTS[(40, 60)][0]
    assert s.solve(**{arg: good})["status"] == "converged"


def test_d7_value_rules_on_the_device(pkg):
    """One table of values through the three device checks (k_finite for rhs, k_reaction_check for a reaction
    field, k_diffusion_check for a diffusion field): a NaN, +inf, -1.0, 0.0 and -0.0, each once at an interior
    node and once on the box boundary of a [:, :N+1] view whose padding columns hold NaN.  Every call raises
    ValueError exactly where the rule of its field -- written out here in NumPy -- is broken, succeeds
    otherwise, and leaves a live session solving to the count it had."""
    M, N = 24, 20
    p = pkg.PoissonEllipse(M=M, N=N)
    rules = {
        "rhs": lambda a: np.isfinite(a).all(),
        "reaction": lambda a: np.isfinite(a[1:-1, 1:-1]).all() and (a[1:-1, 1:-1] >= 0).all(),
        "diffusion": lambda a: np.isfinite(a).all() and (a > 0).all(),
    }
    i, j = np.meshgrid(np.arange(M + 1), np.arange(N + 1), indexing="ij")
    clean = 1.0 + 0.5 * np.sin(0.3 * i) * np.cos(0.2 * j)
    plain = pkg.make_session(p)
    count = plain.solve()["iters"]

    def call(name, view):
        if name == "rhs":
            plain.init(rhs=view)
        else:
            assert pkg.make_session(p, **{name: view}).solve()["status"] == "converged"

    cases = [("clean", None, None)]
    for v in (np.nan, np.inf, -1.0, 0.0, -0.0):
        cases += [(f"{v!r} interior", (11, 7), v), (f"{v!r} boundary", (M, 5), v), (f"{v!r} corner", (0, 0), v)]
    refused = {name: 0 for name in rules}
    for label, at, v in cases:
        host = clean.copy()
        if at is not None:
            host[at] = v
        wide = torch.full((M + 1, N + 5), float("nan"), dtype=torch.float64, device=DEV)
        wide[:, :N + 1] = torch.from_numpy(host)
        view = wide[:, :N + 1]
        assert not view.is_contiguous()
        for name, ok in rules.items():
            if ok(host):
                call(name, view)
            else:
                with pytest.raises(ValueError, match=name):
                    call(name, view)
                refused[name] += 1
            assert plain.solve()["iters"] == count, (label, name)
    # interior: all five break diffusion, NaN / inf / -1 reaction, NaN / inf rhs; the boundary: none breaks reaction
    assert refused == {"rhs": 6, "reaction": 3, "diffusion": 15}


@pytest.mark.parametrize("arg", ["rhs", "w0"])
def test_d7_tensor_of_another_device(pkg, arg):
    if torch.cuda.device_count() < 2:
        pytest.skip("needs two devices")
    s = _session(pkg, (40, 60), "pcg1-march")
    other = torch.ones(41, 61, dtype=torch.float64, device="cuda:1")
    with pytest.raises(ValueError):
        s.solve(**{arg: other})
    with pytest.raises(ValueError):
        s.w_tensor(out=other)
    assert s.solve()["iters"] == COUNTS[(40, 60)][0]
