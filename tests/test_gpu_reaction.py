"""A reaction field c(x, y) on the GPU: (-Δ + σ + c) u = f on the pcg1 march -- the field state of the shift switch
in k_init, k_pcg1 and k_apply, the shift field and its scatter, set_reaction on a live session, the refusals, the
time steppers and SemilinearNewton on device tensors.

Structure and bounds are those of test_gpu_sigma.py; fields and the Newton problem those of test_reaction.py.
"""
import types

import numpy as np
import pytest
import torch

from conftest import sub
from test_apply import SCALARS, U53, boundary_is_zero, torch_reference
from test_apply import fields as xy_fields
from test_gpu_sigma import DECOMP, storage_gap  # noqa: F401  (storage_gap: a fixture)
from test_init_data import manufactured
from test_reaction import NEWTON_STEPS, dg3, fields, g3, newton_problem, newton_start

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GRIDS = [(97, 130), (40, 40)]


@pytest.fixture(scope="module", autouse=True)
def gpu(pkg):
    assert torch.cuda.is_available() and pkg.load_native().device_count() > 0, "no HIP device"


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def fp32(c):
    """What a session with fp32 storage keeps of a field (sigma = 0): rounded once."""
    return c.astype(np.float32).astype(np.float64)


@pytest.fixture(scope="module")
def oracle(pkg):
    """CPU oracle solves shared by the tests, computed once: per grid and field (smooth, disc; in fp64 and rounded
    to fp32 as the fp32 / mixed sessions hold it), the manufactured and the constant right-hand side."""
    out = {}
    for grid in GRIDS:
        p = pkg.PoissonEllipse(M=grid[0], N=grid[1])
        f, _ = manufactured(p)
        for name in ("smooth", "disc"):
            c = fields(p)[name]
            for tag, cc in (("fp64", c), ("fp32", fp32(c))):
                out[(grid, name, tag)] = dict(p=p, f=f, c=c, manuf=pkg.solve(p, "cpu", rhs=f, reaction=cc),
                                              const=pkg.solve(p, "cpu", reaction=cc))
    return out


def _host_residual(p, w, rhs, shift):
    """sqrt(h1 h2 sum (B - (A + s I) w)^2) and (z, r) = h1 h2 sum r^2 / (D + s), s the per-node shift (an array or a
    number), in fp64 with ops/reference.py."""
    R = sub("ops.reference")
    sd = sub("parallel.decomp").subdomain(p.M, p.N, 1, 1, 0)
    a, b, _ = R.assemble(p, sd)
    a, b = a.numpy(), b.numpy()
    B = np.where(p.inside_mask(), rhs, 0.0)[1:-1, 1:-1]
    res = B - R.apply_A(w, a, b, p.h1, p.h2, shift)
    zr = (res * res / R.diag(a, b, p.h1, p.h2, shift)).sum() * p.h1 * p.h2
    return float(np.sqrt((res * res).sum() * p.h1 * p.h2)), float(zr)


@pytest.mark.parametrize("sigma", [0.0, 3.5])
@pytest.mark.parametrize("grid", [(97, 130), (33, 70)])
def test_operator(pkg, grid, sigma):
    """One init(rhs, w0) with random data and the random field: residual_norm (k_init's measure mode) and the
    (z0, r0) the first sweep reduces (k_init's data mode feeding k_pcg1's sweep 0) are the fp64 host values to
    1e-12, and lie 1e-9 or more away from those of the constant field mean(c): the shift is per node."""
    p = pkg.PoissonEllipse(M=grid[0], N=grid[1], sigma=sigma)
    c = fields(p)["random"]
    rng = np.random.default_rng(7)
    shape = (p.M + 1, p.N + 1)
    f = rng.standard_normal(shape)
    w0 = np.zeros(shape)
    w0[1:-1, 1:-1] = rng.standard_normal((p.M - 1, p.N - 1))
    s = pkg.make_session(p, reaction=c)
    assert s.algo_name == "pcg1" and not s.tile.get("block_tiles") and s.has_reaction
    s.init(rhs=f, w0=w0)
    s.synchronize()
    want, zr = _host_residual(p, w0, f, sigma + c[1:-1, 1:-1])
    got = s.residual_norm(f)
    got_zr = s.state(0)["red_c"][0]
    print(f"{grid} sigma {sigma}: residual device {got:.16e} host {want:.16e}; (z0, r0) device {got_zr:.16e} host {zr:.16e}")
    assert abs(got - want) <= 1e-12 * want
    assert abs(got_zr - zr) <= 1e-12 * zr
    flat, zr_flat = _host_residual(p, w0, f, sigma + float(c[1:-1, 1:-1].mean()))
    assert abs(got - flat) > 1e-9 * want and abs(got_zr - zr_flat) > 1e-9 * zr


@pytest.mark.parametrize("s", [1.0, 1e4])
def test_constant_field_is_the_sigma_solve(pkg, s):
    """reaction = s everywhere against PoissonEllipse(sigma=s): the same count, w within 1e-12 max|w| -- not
    bitwise, the sigma sweeps multiply by a precomputed reciprocal on the uniform stencils and the field sweeps
    divide."""
    grid = (97, 130)
    p0 = pkg.PoissonEllipse(M=grid[0], N=grid[1])
    ps = pkg.PoissonEllipse(M=grid[0], N=grid[1], sigma=s)
    f, _ = manufactured(p0)
    c = np.full((grid[0] + 1, grid[1] + 1), s)
    for ranks in (1, 2, 4):
        for split in ("reference", "rows"):
            a = pkg.make_session(ps, ranks=ranks, split=split)
            b = pkg.make_session(p0, ranks=ranks, split=split, reaction=c)
            ra, rb = a.solve(rhs=f), b.solve(rhs=f)
            wa, wb = a.gather_local_w(), b.gather_local_w()
            err = np.abs(wa - wb).max()
            print(f"s {s} ranks {ranks} {split}: iters {ra['iters']} / {rb['iters']} max|w_sigma - w_field| {err:.3e} "
                  f"(max|w| {np.abs(wa).max():.3e})")
            assert ra["status"] == rb["status"] == "converged" and ra["iters"] == rb["iters"]
            assert err <= 1e-12 * np.abs(wa).max()


@pytest.mark.parametrize("dtype", ["fp64", "mixed", "fp32"])
@pytest.mark.parametrize("name", ["smooth", "disc"])
@pytest.mark.parametrize("grid", GRIDS)
def test_solve_against_the_cpu_oracle(pkg, oracle, storage_gap, grid, name, dtype):
    """Both right-hand sides on 1, 2 and 4 subdomains, split by the reference rule and into row strips.  fp64: the
    oracle's count and 1e-10 max|w|.  fp32 / mixed: the session's operator is A + fp32(c), so the oracle is fed
    the rounded field; w is as close to it as that storage is to fp64 at sigma = 0 on this grid (storage_gap),
    scaled by the solutions' sizes with the margin of 4, exactly as test_gpu_sigma.py."""
    o = oracle[(grid, name, "fp64" if dtype == "fp64" else "fp32")]
    for rhs in ("manuf", "const"):
        ref = o[rhs]
        top = np.abs(ref.w).max()
        if dtype == "fp64":
            bound = 1e-10 * top
        else:
            d, top0 = storage_gap(grid, dtype)
            assert d > 0.0
            bound = 4.0 * d * top / top0
        for ranks, split in DECOMP:
            s = pkg.make_session(o["p"], ranks=ranks, split=split, dtype=dtype, reaction=o["c"])
            assert s.algo_name == "pcg1" and s.tile["algo"] == "pcg1" and not s.tile.get("block_tiles")
            r = s.solve(rhs=o["f"] if rhs == "manuf" else None)
            err = np.abs(s.gather_local_w() - ref.w).max()
            print(f"{grid} {name} {dtype} {rhs} ranks {ranks} {split}: iters {r['iters']} (oracle {ref.iters}) "
                  f"max|w - w_cpu| {err:.3e} bound {bound:.3e}")
            assert r["status"] == "converged"
            if dtype == "fp64":
                assert r["iters"] == ref.iters
            assert err <= bound


def test_sigma_plus_field(pkg):
    """A scalar sigma = 3.5 next to the field: the shift field holds sigma + c."""
    p = pkg.PoissonEllipse(M=97, N=130, sigma=3.5)
    c = fields(p)["smooth"]
    f, _ = manufactured(p)
    ref = pkg.solve(p, "cpu", rhs=f, reaction=c)
    for ranks in (1, 4):
        s = pkg.make_session(p, ranks=ranks, reaction=c)
        r = s.solve(rhs=f)
        err = np.abs(s.gather_local_w() - ref.w).max()
        print(f"sigma 3.5 + smooth ranks {ranks}: iters {r['iters']} (oracle {ref.iters}) max|w - w_cpu| {err:.3e}")
        assert r["iters"] == ref.iters and r["status"] == "converged"
        assert err <= 1e-10 * np.abs(ref.w).max()


def test_solve_400x600(pkg):
    """w triples with all three w-cycle phases across several graph batches, on a grid of many tiles."""
    p = pkg.PoissonEllipse(M=400, N=600)
    c = fields(p)["smooth"]
    ref = pkg.solve(p, "cpu", reaction=c)
    s = pkg.make_session(p, reaction=c)
    r = s.solve()
    err = np.abs(s.gather_local_w() - ref.w).max()
    print(f"400x600 smooth: iters {r['iters']} (oracle {ref.iters}) max|w - w_cpu| {err:.3e}")
    assert s.algo_name == "pcg1" and not s.tile.get("block_tiles") and s.state(0)["w_cycle"] == 3
    assert r["iters"] == ref.iters > 3 * 32 and r["status"] == "converged"
    assert err <= 1e-10 * np.abs(ref.w).max()


@pytest.mark.parametrize("ranks", [1, 4])
def test_set_reaction(pkg, ranks):
    """smooth -> disc on one session is a fresh disc session, bitwise, on the graphs captured for the first solve;
    a device tensor, a [:, :N+1] view of a wider tensor and a NumPy array give the same bits; step() before the
    next init raises."""
    p = pkg.PoissonEllipse(M=97, N=130)
    fl = fields(p)
    N1 = p.N + 1
    fresh = pkg.make_session(p, ranks=ranks, reaction=fl["disc"])
    want = fresh.solve()
    w_want = fresh.gather_local_w()
    s = pkg.make_session(p, ranks=ranks, reaction=fl["smooth"])
    first = s.solve()
    assert first["status"] == "converged" and first["iters"] != want["iters"]
    lengths = s.path_stats()["graph_lengths"]
    wide = torch.full((p.M + 1, N1 + 3), float("nan"), dtype=torch.float64, device=DEV)
    wide[:, :N1] = dev(fl["disc"])
    assert not wide[:, :N1].is_contiguous()
    for kind, c in (("numpy", fl["disc"]), ("tensor", dev(fl["disc"])), ("view", wide[:, :N1])):
        s.set_reaction(fl["smooth"])
        s.solve()
        s.set_reaction(c)
        with pytest.raises(RuntimeError, match="set_reaction"):
            s.step(1)
        s.reset_path_stats()
        got = s.solve()
        ps = s.path_stats()
        print(f"ranks {ranks} {kind}: iters {got['iters']} (fresh {want['iters']}), path {ps}")
        assert got["iters"] == want["iters"] and got["status"] == "converged"
        assert s.gather_local_w().tobytes() == w_want.tobytes()
        # replayed from the graphs of the earlier solves: nothing eager, no new batch length
        assert ps["eager_iters"] == 0 and ps["graph_iters"] >= got["iters"] > 0
        assert set(ps["graph_lengths"]) <= set(lengths)
    s.init()
    s.step(3)  # initialised again: stepping works
    s.synchronize()
    plain = pkg.make_session(p, ranks=ranks)
    with pytest.raises(ValueError, match="reaction"):
        plain.set_reaction(fl["disc"])


def _shim(p, shift):
    """p with the per-node shift in sigma's place, for test_apply.torch_reference."""
    return types.SimpleNamespace(M=p.M, N=p.N, h1=p.h1, h2=p.h2, sigma=torch.from_numpy(shift), to_native=p.to_native)


@pytest.mark.parametrize("dtype", ["fp64", "fp32"])
@pytest.mark.parametrize("name", ["smooth", "disc", "random"])
def test_apply(pkg, name, dtype):
    """Session.apply with the field against the host twin PoissonEllipse.apply(x, reaction=c) under
    test_gpu_apply.py's bound 32 * 2^-53 * E (E with |sigma + c| |x|), on 1 and 4 subdomains (bitwise equal).  With
    fp32 storage the session's operator is A + fp32(c): the twin is fed the rounded field."""
    grid = (97, 130)
    p = pkg.PoissonEllipse(M=grid[0], N=grid[1], sigma=2.0 if name == "smooth" else 0.0)
    c = fields(p)[name]
    if dtype == "fp32":  # T(sigma + c), rounded once; the twin gets it as its field at sigma = 0
        c = fp32(p.sigma + c)
        host_p = pkg.PoissonEllipse(M=grid[0], N=grid[1])
    else:
        host_p = p
    x, y = xy_fields(*grid)
    shift = np.ascontiguousarray((host_p.sigma + c)[1:-1, 1:-1])
    first = None
    for ranks in (1, 4):
        s = pkg.make_session(p, ranks=ranks, dtype=dtype, reaction=fields(p)[name])
        got = (s.apply(dev(x), y=dev(y), **SCALARS).cpu().numpy(), s.apply(dev(x)).cpu().numpy())
        if first is not None:
            assert np.array_equal(got[0], first[0]) and np.array_equal(got[1], first[1])
            continue
        first = got
        for tag, g, kw in (("full", got[0], SCALARS), ("plain", got[1], dict(alpha=1.0, beta=0.0, gamma=0.0, const=0.0))):
            want = host_p.apply(x, y=y if tag == "full" else None, reaction=c,
                                **(SCALARS if tag == "full" else {}))
            _, E = torch_reference(pkg, _shim(host_p, shift), x, y, **kw)
            err = np.abs(g - want)[1:-1, 1:-1]
            print(f"{name} {dtype} {tag}: max err/E {float((err / E).max()) / U53:.3g} x 2^-53")
            assert boundary_is_zero(g) and np.isfinite(g).all()
            assert (err <= 32 * U53 * E).all()
        plain = pkg.make_session(p).apply(dev(x)).cpu().numpy()
        assert np.abs(got[1] - plain).max() > 1e-6 * np.abs(plain).max()  # the field is in it


@pytest.mark.parametrize("name", ["smooth", "random"])
def test_apply_reproduces_the_residual(pkg, name):
    """mask f - apply(w) of a partly converged w is the residual residual_norm(f) measures: the same operator in
    both, to 1e-12."""
    p = pkg.PoissonEllipse(M=97, N=130)
    c = fields(p)[name]
    f, _ = manufactured(p)
    s = pkg.make_session(p, reaction=dev(c))
    s.init(rhs=f)
    s.step(7)
    s.synchronize()
    want = s.residual_norm(f)
    w = s.w_tensor()
    e = torch.where(dev(p.inside_mask()), dev(f), torch.zeros_like(w)) - s.apply(w)
    got = float(torch.sqrt((e[1:-1, 1:-1] ** 2).sum() * p.h1 * p.h2))
    print(f"{name}: residual_norm {want:.16e}, from apply {got:.16e}")
    assert want > 0 and abs(got - want) <= 1e-12 * want


def test_refusals(pkg, tmp_path):
    """What is not built for a reaction field raises ValueError, before anything is allocated (the refused
    sessions would hold ~0.3 GB each) and with the live session untouched."""
    big = pkg.PoissonEllipse(M=2000, N=3000)
    cb = fields(big)["smooth"]
    small = pkg.PoissonEllipse(M=97, N=130)
    c = fields(small)["smooth"]
    s = pkg.make_session(small, reaction=c)
    want = s.solve()
    w = s.gather_local_w()
    bad = {}
    for key, v in (("nan", np.nan), ("inf", np.inf), ("negative", -1e-3)):
        bad[key] = cb.copy()
        bad[key][1234, 567] = v
    # every device tensor of the refusals exists before the free memory is read (torch keeps freed blocks)
    bad_dev = {key: dev(field) for key, field in bad.items()}
    d = dev(cb)
    d32, dt = d.float(), d.t().contiguous().t()
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info()[0]
    for kw, name in ((dict(algo="ca"), "ca"), (dict(algo="pcg2"), "pcg2"), (dict(exact=True), "exact"),
                     (dict(block_tiles=1), "block_tiles")):
        for ranks in (1, 2):
            with pytest.raises(ValueError, match=name):
                pkg.make_session(big, ranks=ranks, reaction=cb, **kw)
    for key, field in bad.items():
        for arg in (field, bad_dev[key]):  # the host scan, and the checking kernel on the device
            with pytest.raises(ValueError, match="reaction"):
                pkg.make_session(big, reaction=arg)
    for arg, what in ((d[:-1], "shape"), (d32, "float64"), (dt, "stride"),
                      (cb[:, :-1], "shape"), (cb.astype(np.float32), "float64"), (cb.tolist(), "reaction")):
        with pytest.raises(ValueError, match=what):
            pkg.make_session(big, reaction=arg)
    with pytest.raises(ValueError, match="reaction"):
        sub("ops.kernels").DeviceOps(big, reaction=cb)
    with pytest.raises(ValueError, match="reaction"):
        sub("parallel.dist_solver").DistGpuPCG(big, None, comm="torch", reaction=cb)
    with pytest.raises(ValueError, match="reaction"):
        sub("models.sstep_pcg").TorchSStepPCG(small, reaction=c)
    with pytest.raises(ValueError, match="own"):  # multi-process transports
        pkg.load_native().Session(small.to_native(), world=1, comm="ipc", reaction=c)
    torch.cuda.synchronize()
    assert free0 - torch.cuda.mem_get_info()[0] < 100 << 20
    del bad_dev, d, d32, dt
    # the live session: bad fields and checkpoints are refused and leave it as it was
    cs = fields(small)
    for key, v in (("nan", np.nan), ("inf", np.inf), ("negative", -1.0)):
        field = cs["disc"].copy()
        field[50, 60] = v
        for arg in (field, dev(field)):
            with pytest.raises(ValueError, match="reaction"):
                s.set_reaction(arg)
    s.step(1)  # no refused set_reaction has marked the state stale
    ck = str(tmp_path / "reaction.ck")
    with pytest.raises(ValueError, match="reaction"):
        s.save_checkpoint(ck)
    with pytest.raises(ValueError, match="reaction"):
        s.load_checkpoint(ck)
    with pytest.raises(ValueError, match="reaction"):
        s.solve_checkpointed(ck, every=16)
    with pytest.raises(ValueError, match="reaction"):
        s.error_norms()
    assert not (tmp_path / "reaction.ck").exists()
    again = s.solve()
    assert again["iters"] == want["iters"] and np.array_equal(s.gather_local_w(), w)
    # NaN on the box boundary of the field is never read
    edge = c.copy()
    edge[0, :] = edge[-1, :] = np.nan
    edge[:, 0] = edge[:, -1] = -np.inf
    clean = pkg.make_session(small, ranks=4, reaction=c)
    assert clean.solve()["iters"] == want["iters"]
    for arg in (edge, dev(edge)):
        t = pkg.make_session(small, ranks=4, reaction=arg)
        assert t.solve()["iters"] == want["iters"] and np.array_equal(t.gather_local_w(), clean.gather_local_w())


def test_backward_euler_three_steps(pkg):
    """3 steps from u = 0 with g = 1 on device tensors and a device field against 3 oracle solves chained on the
    host."""
    p = pkg.PoissonEllipse(M=97, N=130)
    c = fields(p)["smooth"]
    dt = 1e-3
    be = pkg.BackwardEuler(p, dt, reaction=dev(c))
    assert be.session.algo_name == "pcg1" and be.session.has_reaction
    u = torch.zeros(98, 131, dtype=torch.float64, device=DEV)
    g = torch.ones_like(u)
    host = np.zeros((98, 131))
    ps = pkg.PoissonEllipse(M=97, N=130, sigma=1.0 / dt)
    for n in range(3):
        u = be.step(u, g)
        assert isinstance(u, torch.Tensor) and u.is_cuda and u.dtype == torch.float64
        host = pkg.solve(ps, "cpu", rhs=host / dt + 1.0, w0=host, reaction=c).w
        err = np.abs(u.cpu().numpy() - host).max()
        print(f"step {n + 1}: iters {be.last['iters']} max|u - u_cpu| {err:.3e} max u {host.max():.6e}")
        assert err <= 1e-10 * np.abs(host).max()


def test_theta_scheme_one_step(pkg):
    """One Crank-Nicolson step on device tensors against the cpu backend's step: the field is in the apply of the
    right-hand side and in the solve."""
    p = pkg.PoissonEllipse(M=97, N=130)
    c = fields(p)["smooth"]
    _, u0 = manufactured(p)
    dt = 1e-3
    dv = pkg.ThetaScheme(p, dt, theta=0.5, reaction=dev(c))
    hs = pkg.ThetaScheme(p, dt, theta=0.5, backend="cpu", reaction=c)
    rhs_d, rhs_h = dv.rhs(dev(u0), 1.0).cpu().numpy(), hs.rhs(u0, 1.0)
    assert np.abs(rhs_d - rhs_h).max() <= 1e-12 * np.abs(rhs_h).max()
    u, want = dv.step(dev(u0), 1.0), hs.step(u0, 1.0)
    err = np.abs(u.cpu().numpy() - want).max()
    print(f"theta 1/2: iters {dv.last['iters']} (cpu {hs.last['iters']}) max|u - u_cpu| {err:.3e}")
    assert dv.last["status"] == "converged" and err <= 1e-10 * np.abs(want).max()


def test_semilinear_newton_on_device_tensors(pkg):
    """The Newton run of test_reaction.py on device tensors: the same step count, u within 1e-9 max|u| of the cpu
    run; one session, a device tensor out."""
    p, f0, u = newton_problem(pkg)
    f = f0 + g3(u)
    start = newton_start(pkg, p, f)
    cpu = pkg.SemilinearNewton(p, g3, dg3, backend="cpu", newton_rtol=1e-8)
    want = cpu.solve(f, u0=start)
    nw = pkg.SemilinearNewton(p, g3, dg3, newton_rtol=1e-8)
    got = nw.solve(dev(f), u0=dev(start))
    assert isinstance(got, torch.Tensor) and got.is_cuda
    err = np.abs(got.cpu().numpy() - want).max()
    print(f"steps {nw.steps} (cpu {cpu.steps}), history {['%.3e' % h for h in nw.history]}, max|u - u_cpu| {err:.3e}")
    assert nw.converged and nw.steps == cpu.steps == NEWTON_STEPS
    assert all(b < a for a, b in zip(nw.history, nw.history[1:]))
    assert err <= 1e-9 * np.abs(want).max()


@pytest.mark.parametrize("sigma", [0.0, 100.0])
def test_no_change_elsewhere(pkg, sigma):
    """Sessions without a field are what they were: device_bytes, tile and iterates of the sigma = 0 and
    sigma = 100 solves of test_gpu_sigma.py, bitwise, before and after a reaction session has lived in the
    process, and a reaction session holds exactly one more field."""
    grid = (97, 130)
    p = pkg.PoissonEllipse(M=grid[0], N=grid[1], sigma=sigma)
    kw = dict(algo="pcg1", block_tiles=0)

    def run():
        s = pkg.make_session(p, **kw)
        r = s.solve()
        return r["iters"], r["status"], s.gather_local_w().tobytes(), s.device_bytes, s.tile, s.has_reaction

    before = run()
    t = pkg.make_session(p, reaction=fields(p)["disc"], **kw)
    t.solve()
    assert t.tile == before[4]
    pitch = -(-(grid[1] - 1 + 2 + 8) // 32) * 32  # MemoryPlan: ny + 10 columns, rounded up to 256 B
    field_bytes = -(-((31 + (grid[0] - 1 + 4) * pitch) * 8) // 256) * 256
    assert t.device_bytes - before[3] == field_bytes
    del t
    after = run()
    assert after == before and before[1] == "converged" and not before[5]
    ref = pkg.solve(p, "cpu")
    assert before[0] == ref.iters
    assert np.abs(np.frombuffer(before[2]).reshape(ref.w.shape) - ref.w).max() <= 1e-10 * np.abs(ref.w).max()
