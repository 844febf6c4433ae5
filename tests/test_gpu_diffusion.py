"""A diffusion field k(x, y) on the GPU: (-∇·k∇ + σ + c) u = f on the pcg1 march -- the diffusion flag of k_init,
k_pcg1 and k_apply, the two face-coefficient fields and their setup kernel, set_diffusion on a live session, the
refusals, the θ-scheme and QuasilinearPicard on device tensors.

Structure and bounds are those of test_gpu_reaction.py; fields and the Picard problem those of test_diffusion.py.
"""
import numpy as np
import pytest
import torch

from conftest import sub
from test_apply import SCALARS, U53, boundary_is_zero
from test_apply import fields as xy_fields
from test_diffusion import (PICARD_STEPS, host_faces, host_residual, kappa_u2, kappas, picard_problem, rhs_of)
from test_gpu_sigma import DECOMP, storage_gap  # noqa: F401  (storage_gap: a fixture)
from test_init_data import manufactured
from test_reaction import fields as reaction_fields

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GRIDS = [(97, 130), (40, 40), (33, 70)]


@pytest.fixture(scope="module", autouse=True)
def gpu(pkg):
    assert torch.cuda.is_available() and pkg.load_native().device_count() > 0, "no HIP device"


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


@pytest.fixture(scope="module")
def oracle(pkg):
    """CPU oracle solves shared by the tests, computed once: per grid and field, the manufactured and the constant
    right-hand side."""
    out = {}
    for grid in GRIDS:
        p = pkg.PoissonEllipse(M=grid[0], N=grid[1])
        f, _ = manufactured(p)
        for name, k in kappas(p).items():
            out[(grid, name)] = dict(p=p, f=f, k=k, manuf=pkg.solve(p, "cpu", rhs=f, diffusion=k),
                                     const=pkg.solve(p, "cpu", diffusion=k))
    return out


@pytest.mark.parametrize("with_reaction", [False, True])
@pytest.mark.parametrize("sigma", [0.0, 3.5])
@pytest.mark.parametrize("grid", [(97, 130), (33, 70)])
def test_operator(pkg, grid, sigma, with_reaction):
    """One init(rhs, w0) with random data and the random field: residual_norm (k_init's measure mode) and the
    (z0, r0) the first sweep reduces (k_init's data mode feeding k_pcg1's sweep 0) are the fp64 host values to
    1e-12, and lie 1e-9 or more away from those of the constant field mean(k): the coefficient is per face."""
    p = pkg.PoissonEllipse(M=grid[0], N=grid[1], sigma=sigma)
    k = kappas(p)["random"]
    c = reaction_fields(p)["random"] if with_reaction else None
    shift = sigma + c[1:-1, 1:-1] if with_reaction else sigma
    rng = np.random.default_rng(7)
    shape = (p.M + 1, p.N + 1)
    f = rng.standard_normal(shape)
    w0 = np.zeros(shape)
    w0[1:-1, 1:-1] = rng.standard_normal((p.M - 1, p.N - 1))
    s = pkg.make_session(p, diffusion=k, reaction=c)
    assert s.algo_name == "pcg1" and not s.tile.get("block_tiles") and s.has_diffusion
    assert s.has_reaction == with_reaction
    s.init(rhs=f, w0=w0)
    s.synchronize()
    zr, _, want = host_residual(p, w0, f, k, shift)
    zr = zr * zr
    got = s.residual_norm(f)
    got_zr = s.state(0)["red_c"][0]
    print(f"{grid} sigma {sigma} reaction {with_reaction}: residual device {got:.16e} host {want:.16e}; (z0, r0) "
          f"device {got_zr:.16e} host {zr:.16e}")
    assert abs(got - want) <= 1e-12 * want
    assert abs(got_zr - zr) <= 1e-12 * zr
    zr_flat, _, flat = host_residual(p, w0, f, np.full(shape, k.mean()), shift)
    assert abs(got - flat) > 1e-9 * want and abs(got_zr - zr_flat * zr_flat) > 1e-9 * zr


def _magnitude(p, k, x, y, shift, alpha, beta, gamma, const):
    """E of test_apply.torch_reference on the faces multiplied by k: |alpha| ((|A_k| + shift) |x|) + |beta| |x| +
    |gamma| |y| + |const| on the interior nodes."""
    a, b = host_faces(p, k)
    m = np.abs(x).copy()
    m[0, :] = m[-1, :] = 0.0
    m[:, 0] = m[:, -1] = 0.0
    mc = m[1:-1, 1:-1]
    h1, h2 = p.h1, p.h2
    ax = 1.0 / h1 * (a[2:, 1:-1] * (m[2:, 1:-1] + mc) / h1 + a[1:-1, 1:-1] * (mc + m[:-2, 1:-1]) / h1)
    ay = 1.0 / h2 * (b[1:-1, 2:] * (m[1:-1, 2:] + mc) / h2 + b[1:-1, 1:-1] * (mc + m[1:-1, :-2]) / h2)
    return abs(alpha) * ((ax + ay) + shift * mc) + abs(beta) * mc + abs(gamma) * np.abs(y)[1:-1, 1:-1] + abs(const)


@pytest.mark.parametrize("with_reaction", [False, True])
def test_apply(pkg, with_reaction):
    """Session.apply with the random field against the host twin PoissonEllipse.apply(x, diffusion=k) under
    test_gpu_apply.py's bound 32 * 2^-53 * E, on 1, 2 and 4 subdomains (bitwise equal); the box boundary is 0."""
    grid = (97, 130)
    p = pkg.PoissonEllipse(M=grid[0], N=grid[1], sigma=2.0)
    k = kappas(p)["random"]
    c = reaction_fields(p)["smooth"] if with_reaction else None
    shift = p.sigma + c[1:-1, 1:-1] if with_reaction else p.sigma
    x, y = xy_fields(*grid)
    first = None
    for ranks in (1, 2, 4):
        s = pkg.make_session(p, ranks=ranks, diffusion=k, reaction=c)
        got = (s.apply(dev(x), y=dev(y), **SCALARS).cpu().numpy(), s.apply(dev(x)).cpu().numpy())
        assert boundary_is_zero(got[0]) and boundary_is_zero(got[1]) and np.isfinite(got[0]).all()
        if first is not None:
            assert np.array_equal(got[0], first[0]) and np.array_equal(got[1], first[1])
            continue
        first = got
        unit = dict(alpha=1.0, beta=0.0, gamma=0.0, const=0.0)
        for tag, g, kw in (("full", got[0], SCALARS), ("plain", got[1], unit)):
            want = p.apply(x, y=y if tag == "full" else None, diffusion=k, reaction=c,
                           **(SCALARS if tag == "full" else {}))
            E = _magnitude(p, k, x, y, shift, **kw)
            err = np.abs(g - want)[1:-1, 1:-1]
            print(f"reaction {with_reaction} {tag}: max err/E {float((err / E).max()) / U53:.3g} x 2^-53")
            assert (err <= 32 * U53 * E).all()
        plain = pkg.make_session(p, reaction=c).apply(dev(x)).cpu().numpy()
        assert np.abs(got[1] - plain).max() > 1e-6 * np.abs(plain).max()  # the field is in it


def test_unit_field_is_the_plain_solve(pkg):
    """k = 1 against the session without the argument (sigma = 3.5) and against the reaction-only session: the same
    count, w within 1e-12 max|w| -- not bitwise, the uniform stencils of those sweeps multiply by a reciprocal (or
    take their faces from the class) and the diffusion sweeps divide by the D they form."""
    grid = (97, 130)
    p = pkg.PoissonEllipse(M=grid[0], N=grid[1], sigma=3.5)
    f, _ = manufactured(p)
    c = reaction_fields(p)["smooth"]
    one = np.ones((grid[0] + 1, grid[1] + 1))
    for ranks in (1, 2, 4):
        for split in ("reference", "rows"):
            for tag, kw in (("plain", {}), ("reaction", dict(reaction=c))):
                a = pkg.make_session(p, ranks=ranks, split=split, **kw)
                b = pkg.make_session(p, ranks=ranks, split=split, diffusion=one, **kw)
                ra, rb = a.solve(rhs=f), b.solve(rhs=f)
                wa, wb = a.gather_local_w(), b.gather_local_w()
                err = np.abs(wa - wb).max()
                print(f"{tag} ranks {ranks} {split}: iters {ra['iters']} / {rb['iters']} max|w - w_k1| {err:.3e} "
                      f"(max|w| {np.abs(wa).max():.3e})")
                assert ra["status"] == rb["status"] == "converged" and ra["iters"] == rb["iters"]
                assert err <= 1e-12 * np.abs(wa).max()


@pytest.mark.parametrize("dtype", ["fp64", "mixed", "fp32"])
@pytest.mark.parametrize("name", ["smooth", "jump", "random"])
@pytest.mark.parametrize("grid", GRIDS)
def test_solve_against_the_cpu_oracle(pkg, oracle, storage_gap, grid, name, dtype):
    """Both right-hand sides on 1, 2 and 4 subdomains, split by the reference rule and into row strips.  fp64: the
    oracle's count and 1e-10 max|w| (the random field catches a wrong edge column or extra ghost row of the march).
    fp32 / mixed: the storage_gap rule of test_gpu_sigma.py (4 d top / top0) plus 4 * 2^-24 * top for the face
    coefficients rounded once to fp32 -- a relative perturbation eps of every coefficient moves the solution by
    about eps in the energy norm."""
    o = oracle[(grid, name)]
    for rhs in ("manuf", "const"):
        ref = o[rhs]
        assert ref.converged
        top = np.abs(ref.w).max()
        if dtype == "fp64":
            t1, t2 = 1e-10 * top, 0.0
        else:
            d, top0 = storage_gap(grid, dtype)
            assert d > 0.0
            t1, t2 = 4.0 * d * top / top0, 4.0 * 2.0 ** -24 * top
        for ranks, split in DECOMP:
            s = pkg.make_session(o["p"], ranks=ranks, split=split, dtype=dtype, diffusion=o["k"])
            assert s.algo_name == "pcg1" and s.tile["algo"] == "pcg1" and not s.tile.get("block_tiles")
            r = s.solve(rhs=o["f"] if rhs == "manuf" else None)
            err = np.abs(s.gather_local_w() - ref.w).max()
            print(f"{grid} {name} {dtype} {rhs} ranks {ranks} {split}: iters {r['iters']} (oracle {ref.iters}) "
                  f"max|w - w_cpu| {err:.3e} bound {t1:.3e} + {t2:.3e}")
            assert r["status"] == "converged"
            if dtype == "fp64":
                assert r["iters"] == ref.iters
            assert err <= t1 + t2


def test_sigma_reaction_and_diffusion_together(pkg):
    p = pkg.PoissonEllipse(M=97, N=130, sigma=3.5)
    k, c = kappas(p)["random"], reaction_fields(p)["smooth"]
    f, u = manufactured(p)
    ref = pkg.solve(p, "cpu", rhs=f, w0=0.5 * u, reaction=c, diffusion=k)
    for ranks in (1, 4):
        s = pkg.make_session(p, ranks=ranks, reaction=dev(c), diffusion=dev(k))
        r = s.solve(rhs=f, w0=0.5 * u)
        err = np.abs(s.gather_local_w() - ref.w).max()
        print(f"sigma 3.5 + smooth c + random k, ranks {ranks}: iters {r['iters']} (oracle {ref.iters}) "
              f"max|w - w_cpu| {err:.3e}")
        assert r["iters"] == ref.iters and r["status"] == "converged"
        assert err <= 1e-10 * np.abs(ref.w).max()


@pytest.mark.parametrize("name", ["smooth", "random"])
def test_solve_400x600(pkg, name):
    """FAST interior tiles and all three w-cycle phases across several graph batches, on a grid of many tiles."""
    p = pkg.PoissonEllipse(M=400, N=600)
    k = kappas(p)[name]
    ref = pkg.solve(p, "cpu", rhs=rhs_of(p, name), diffusion=k)
    s = pkg.make_session(p, diffusion=k)
    r = s.solve(rhs=rhs_of(p, name))
    err = np.abs(s.gather_local_w() - ref.w).max()
    print(f"400x600 {name}: iters {r['iters']} (oracle {ref.iters}) max|w - w_cpu| {err:.3e}")
    assert s.algo_name == "pcg1" and not s.tile.get("block_tiles") and s.state(0)["w_cycle"] == 3
    assert r["iters"] == ref.iters > 3 * 32 and r["status"] == "converged"
    assert err <= 1e-10 * np.abs(ref.w).max()


@pytest.mark.parametrize("ranks", [1, 4])
def test_set_diffusion(pkg, ranks):
    """smooth -> jump on one session is a fresh jump session, bitwise, on the graphs captured for the first solve;
    a device tensor, a [:, :N+1] view of a wider tensor and a NumPy array give the same bits; step() before the
    next init raises."""
    p = pkg.PoissonEllipse(M=97, N=130)
    fl = kappas(p)
    N1 = p.N + 1
    fresh = pkg.make_session(p, ranks=ranks, diffusion=fl["jump"])
    want = fresh.solve()
    w_want = fresh.gather_local_w()
    s = pkg.make_session(p, ranks=ranks, diffusion=fl["smooth"])
    first = s.solve()
    assert first["status"] == "converged" and first["iters"] != want["iters"]
    lengths = s.path_stats()["graph_lengths"]
    wide = torch.full((p.M + 1, N1 + 3), float("nan"), dtype=torch.float64, device=DEV)
    wide[:, :N1] = dev(fl["jump"])
    assert not wide[:, :N1].is_contiguous()
    for kind, k in (("numpy", fl["jump"]), ("tensor", dev(fl["jump"])), ("view", wide[:, :N1])):
        s.set_diffusion(fl["smooth"])
        s.solve()
        s.set_diffusion(k)
        with pytest.raises(RuntimeError, match="set_diffusion"):
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
    for kw in ({}, dict(reaction=reaction_fields(p)["smooth"])):
        plain = pkg.make_session(p, ranks=ranks, **kw)
        assert not plain.has_diffusion
        with pytest.raises(ValueError, match="diffusion"):
            plain.set_diffusion(fl["jump"])


def test_refusals(pkg, tmp_path):
    """What is not built for a diffusion field raises ValueError, before anything is allocated (the refused
    sessions would hold ~0.4 GB each) and with the live session untouched."""
    big = pkg.PoissonEllipse(M=2000, N=3000)
    kb = kappas(big)["smooth"]
    small = pkg.PoissonEllipse(M=97, N=130)
    k = kappas(small)["smooth"]
    s = pkg.make_session(small, diffusion=k)
    want = s.solve()
    w = s.gather_local_w()
    bad = {}
    for key, v, ij in (("nan", np.nan, (1234, 567)), ("inf", np.inf, (0, 0)), ("zero", 0.0, (2000, 17)),
                       ("negative", -1e-3, (5, 3000))):
        bad[key] = kb.copy()
        bad[key][ij] = v
    # every device tensor of the refusals exists before the free memory is read (torch keeps freed blocks)
    bad_dev = {key: dev(field) for key, field in bad.items()}
    d = dev(kb)
    d32, dt = d.float(), d.t().contiguous().t()
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info()[0]
    for kw, name in ((dict(algo="ca"), "ca"), (dict(algo="pcg2"), "pcg2"), (dict(exact=True), "exact"),
                     (dict(block_tiles=1), "block_tiles")):
        for ranks in (1, 2):
            with pytest.raises(ValueError, match=name):
                pkg.make_session(big, ranks=ranks, diffusion=kb, **kw)
    for key, field in bad.items():
        for arg in (field, bad_dev[key]):  # the host scan, and the checking kernel on the device
            with pytest.raises(ValueError, match="diffusion"):
                pkg.make_session(big, diffusion=arg)
    for arg, what in ((d[:-1], "shape"), (d32, "float64"), (dt, "stride"),
                      (kb[:, :-1], "shape"), (kb.astype(np.float32), "float64"), (kb.tolist(), "diffusion")):
        with pytest.raises(ValueError, match=what):
            pkg.make_session(big, diffusion=arg)
    with pytest.raises(ValueError, match="diffusion"):
        sub("ops.kernels").DeviceOps(big, diffusion=kb)
    with pytest.raises(ValueError, match="diffusion"):
        sub("parallel.dist_solver").DistGpuPCG(big, None, comm="torch", diffusion=kb)
    with pytest.raises(ValueError, match="diffusion"):
        sub("models.sstep_pcg").TorchSStepPCG(small, diffusion=k)
    with pytest.raises(ValueError, match="own"):  # multi-process transports
        pkg.load_native().Session(small.to_native(), world=1, comm="ipc", diffusion=k)
    torch.cuda.synchronize()
    assert free0 - torch.cuda.mem_get_info()[0] < 100 << 20
    del bad_dev, d, d32, dt
    # the live session: bad fields and checkpoints are refused and leave it as it was
    ks = kappas(small)
    for key, v, ij in (("nan", np.nan, (50, 60)), ("inf", np.inf, (97, 130)), ("zero", 0.0, (0, 5)),
                       ("negative", -1.0, (50, 0))):
        field = ks["jump"].copy()
        field[ij] = v
        for arg in (field, dev(field)):
            with pytest.raises(ValueError, match="diffusion"):
                s.set_diffusion(arg)
    s.step(1)  # no refused set_diffusion has marked the state stale
    ck = str(tmp_path / "diffusion.ck")
    with pytest.raises(ValueError, match="diffusion"):
        s.save_checkpoint(ck)
    with pytest.raises(ValueError, match="diffusion"):
        s.load_checkpoint(ck)
    with pytest.raises(ValueError, match="diffusion"):
        s.solve_checkpointed(ck, every=16)
    with pytest.raises(ValueError, match="diffusion"):
        s.error_norms()
    assert not (tmp_path / "diffusion.ck").exists()
    again = s.solve()
    assert again["iters"] == want["iters"] and np.array_equal(s.gather_local_w(), w)


def test_theta_scheme_one_step(pkg):
    """One Crank-Nicolson step on device tensors against the cpu backend's step: the field is in the apply of the
    right-hand side and in the solve."""
    p = pkg.PoissonEllipse(M=97, N=130)
    k = kappas(p)["smooth"]
    _, u0 = manufactured(p)
    dt = 1e-3
    dv = pkg.ThetaScheme(p, dt, theta=0.5, diffusion=dev(k))
    hs = pkg.ThetaScheme(p, dt, theta=0.5, backend="cpu", diffusion=k)
    assert dv.session.has_diffusion
    rhs_d, rhs_h = dv.rhs(dev(u0), 1.0).cpu().numpy(), hs.rhs(u0, 1.0)
    assert np.abs(rhs_d - rhs_h).max() <= 1e-12 * np.abs(rhs_h).max()
    u, want = dv.step(dev(u0), 1.0), hs.step(u0, 1.0)
    err = np.abs(u.cpu().numpy() - want).max()
    print(f"theta 1/2: iters {dv.last['iters']} (cpu {hs.last['iters']}) max|u - u_cpu| {err:.3e}")
    assert dv.last["status"] == "converged" and err <= 1e-10 * np.abs(want).max()


def test_quasilinear_picard_on_device_tensors(pkg):
    """The Picard run of test_diffusion.py on device tensors: the pinned step count, u within 1e-10 max|u| of the
    cpu run; one session, a device tensor out."""
    p, f = picard_problem(pkg)
    cpu = pkg.QuasilinearPicard(p, kappa_u2, backend="cpu", picard_rtol=1e-8)
    want = cpu.solve(f)
    pc = pkg.QuasilinearPicard(p, kappa_u2, picard_rtol=1e-8)
    got = pc.solve(dev(f))
    assert isinstance(got, torch.Tensor) and got.is_cuda
    err = np.abs(got.cpu().numpy() - want).max()
    print(f"steps {pc.steps} (cpu {cpu.steps}), history {['%.3e' % h for h in pc.history]}, max|u - u_cpu| {err:.3e}")
    assert pc.converged and pc.steps == cpu.steps == PICARD_STEPS
    assert all(b < a for a, b in zip(pc.history, pc.history[1:]))
    assert err <= 1e-10 * np.abs(want).max()


@pytest.mark.parametrize("with_reaction", [False, True])
def test_no_change_elsewhere(pkg, with_reaction):
    """Sessions without a diffusion field are what they were: device_bytes, tile and iterates, bitwise, before and
    after a diffusion session has lived in the process; the diffusion session holds the shift field (if the other
    does not), two more fields and one more row."""
    grid = (97, 130)
    p = pkg.PoissonEllipse(M=grid[0], N=grid[1])
    kw = dict(algo="pcg1", block_tiles=0)
    if with_reaction:
        kw["reaction"] = reaction_fields(p)["disc"]

    def run():
        s = pkg.make_session(p, **kw)
        r = s.solve()
        return r["iters"], r["status"], s.gather_local_w().tobytes(), s.device_bytes, s.tile, s.has_diffusion

    before = run()
    t = pkg.make_session(p, diffusion=kappas(p)["jump"], **kw)
    t.solve()
    assert t.tile == before[4]
    pitch = -(-(grid[1] - 1 + 2 + 8) // 32) * 32  # MemoryPlan: ny + 10 columns, rounded up to 256 B
    field_bytes = -(-((31 + (grid[0] - 1 + 4) * pitch) * 8) // 256) * 256
    assert t.device_bytes - before[3] == (2 if with_reaction else 3) * field_bytes + pitch * 8
    del t
    after = run()
    assert after == before and before[1] == "converged" and not before[5]
