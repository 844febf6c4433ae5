"""Level-set domains D = {phi < 0} on the GPU: the setup kernel that forms the face-coefficient fields and the
right-hand-side mask from phi (k_domain_fields), the mask in k_init's three modes, the diffusion sweeps on those
faces, set_domain on a live session, the refusals, the memory plan, and the models on device tensors.

Structure and bounds are those of test_gpu_diffusion.py; the domains and host statements those of test_domain.py.
Grids: 130 columns give two march tile columns, 300 a second workgroup column of the 256-wide setup kernel.
"""
import numpy as np
import pytest
import torch

from conftest import sub
from test_apply import SCALARS, U53, boundary_is_zero
from test_apply import fields as xy_fields
from test_diffusion import kappas
from test_domain import domains, host_faces, host_residual
from test_gpu_sigma import DECOMP, storage_gap  # noqa: F401  (storage_gap: a fixture)
from test_init_data import manufactured
from test_reaction import fields as reaction_fields

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GRIDS = [(97, 130), (33, 70), (20, 300)]


@pytest.fixture(scope="module", autouse=True)
def gpu(pkg):
    assert torch.cuda.is_available() and pkg.load_native().device_count() > 0, "no HIP device"


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


@pytest.fixture(scope="module")
def oracle(pkg):
    """CPU oracle solves shared by the tests, computed once: per grid and domain, the manufactured and the constant
    right-hand side."""
    out = {}
    for grid in GRIDS:
        p = pkg.PoissonEllipse(M=grid[0], N=grid[1])
        f, _ = manufactured(p)
        phis, pins = domains(p)
        for name in ("disc", "two", "holed"):
            kw = dict(domain=phis[name], reaction=pins[name])
            out[(grid, name)] = dict(p=p, f=f, kw=kw, manuf=pkg.solve(p, "cpu", rhs=f, **kw),
                                     const=pkg.solve(p, "cpu", **kw))
    return out


def _magnitude(p, phi, k, x, y, shift, alpha, beta, gamma, const):
    """E of test_apply.torch_reference on the faces of the domain: |alpha| ((|A| + shift) |x|) + |beta| |x| +
    |gamma| |y| + |const| on the interior nodes."""
    a, b = host_faces(p, phi, k)
    m = np.abs(x).copy()
    m[0, :] = m[-1, :] = 0.0
    m[:, 0] = m[:, -1] = 0.0
    mc = m[1:-1, 1:-1]
    h1, h2 = p.h1, p.h2
    ax = 1.0 / h1 * (a[2:, 1:-1] * (m[2:, 1:-1] + mc) / h1 + a[1:-1, 1:-1] * (mc + m[:-2, 1:-1]) / h1)
    ay = 1.0 / h2 * (b[1:-1, 2:] * (m[1:-1, 2:] + mc) / h2 + b[1:-1, 1:-1] * (mc + m[1:-1, :-2]) / h2)
    return abs(alpha) * ((ax + ay) + shift * mc) + abs(beta) * mc + abs(gamma) * np.abs(y)[1:-1, 1:-1] + abs(const)


@pytest.mark.parametrize("with_fields", [False, True])
@pytest.mark.parametrize("grid", GRIDS)
def test_apply(pkg, grid, with_fields):
    """Session.apply on the speckle domain (a random sign pattern: every face of the setup kernel matters) against
    the host twin PoissonEllipse.apply(x, domain=phi) under test_gpu_apply.py's bound 32 * 2^-53 * E, with and
    without random diffusion and reaction fields, on 1, 2 and 4 subdomains in both splits (bitwise equal); more
    than 1e-9 relative away from the apply without the domain."""
    p = pkg.PoissonEllipse(M=grid[0], N=grid[1], sigma=2.0)
    phi = domains(p)[0]["speckle"]
    k = kappas(p)["random"] if with_fields else None
    c = reaction_fields(p)["random"] if with_fields else None
    shift = p.sigma + c[1:-1, 1:-1] if with_fields else p.sigma
    x, y = xy_fields(*grid)
    first = None
    for ranks, split in DECOMP:
        s = pkg.make_session(p, ranks=ranks, split=split, domain=phi, diffusion=k, reaction=c)
        assert s.has_domain and s.has_diffusion == with_fields and s.has_reaction == with_fields
        got = (s.apply(dev(x), y=dev(y), **SCALARS).cpu().numpy(), s.apply(dev(x)).cpu().numpy())
        assert boundary_is_zero(got[0]) and boundary_is_zero(got[1]) and np.isfinite(got[0]).all()
        if first is not None:
            assert np.array_equal(got[0], first[0]) and np.array_equal(got[1], first[1])
            continue
        first = got
        unit = dict(alpha=1.0, beta=0.0, gamma=0.0, const=0.0)
        for tag, g, kw in (("full", got[0], SCALARS), ("plain", got[1], unit)):
            want = p.apply(x, y=y if tag == "full" else None, domain=phi, diffusion=k, reaction=c,
                           **(SCALARS if tag == "full" else {}))
            E = _magnitude(p, phi, k, x, y, shift, **kw)
            err = np.abs(g - want)[1:-1, 1:-1]
            print(f"{grid} fields {with_fields} {tag}: max err/E {float((err / E).max()) / U53:.3g} x 2^-53")
            assert (err <= 32 * U53 * E).all()
        other = pkg.make_session(p, diffusion=k, reaction=c).apply(dev(x)).cpu().numpy()
        assert np.abs(got[1] - other).max() > 1e-9 * np.abs(other).max()


@pytest.mark.parametrize("with_fields", [False, True])
@pytest.mark.parametrize("grid", GRIDS)
def test_init_and_residual(pkg, grid, with_fields):
    """One init(rhs, w0) with random data on the speckle domain: residual_norm (k_init's measure mode) and the
    (z0, r0) the first sweep reduces (the data mode feeding sweep 0) are the fp64 host values to 1e-12 -- mask,
    faces and D -- and lie 1e-9 or more away from the values under the ellipse's mask.  w0 is 1e-6 times a
    standard normal field: on the speckle faces (1/eps on half of them) A w0 of a unit field is 1e8 times the
    right-hand side and would bury the mask below the 1e-9 that tells the two masks apart; at 1e-6 the two terms
    are of one size and both the faces and the mask are visible at 1e-12.  Then the same with the constant F: the
    plain mode."""
    p = pkg.PoissonEllipse(M=grid[0], N=grid[1], sigma=3.5 if with_fields else 0.0, F=1.5)
    phi = domains(p)[0]["speckle"]
    k = kappas(p)["random"] if with_fields else None
    c = reaction_fields(p)["random"] if with_fields else None
    shift = p.sigma + c[1:-1, 1:-1] if with_fields else p.sigma
    rng = np.random.default_rng(7)
    shape = (p.M + 1, p.N + 1)
    f = rng.standard_normal(shape)
    w0 = np.zeros(shape)
    w0[1:-1, 1:-1] = 1e-6 * rng.standard_normal((p.M - 1, p.N - 1))
    s = pkg.make_session(p, domain=phi, diffusion=k, reaction=c)
    assert s.algo_name == "pcg1" and not s.tile.get("block_tiles") and s.has_domain
    s.init(rhs=f, w0=w0)
    s.synchronize()
    want, zr = host_residual(p, phi, w0, f, k, shift)
    got, got_zr = s.residual_norm(f), s.state(0)["red_c"][0]
    print(f"{grid} fields {with_fields}: residual device {got:.16e} host {want:.16e}; (z0, r0) device {got_zr:.16e} "
          f"host {zr:.16e}")
    assert abs(got - want) <= 1e-12 * want and abs(got_zr - zr) <= 1e-12 * zr
    a, b = host_faces(p, phi, k)  # the ellipse's mask on the domain's faces
    R = sub("ops.reference")
    r = np.where(p.inside_mask(), f, 0.0)[1:-1, 1:-1] - R.apply_A(w0, a, b, p.h1, p.h2, shift)
    ell = float(np.sqrt((r * r).sum() * p.h1 * p.h2))
    zr_ell = float((r * r / R.diag(a, b, p.h1, p.h2, shift)).sum() * p.h1 * p.h2)
    assert abs(got - ell) > 1e-9 * want and abs(got_zr - zr_ell) > 1e-9 * zr
    # the constant F
    s.init()
    s.synchronize()
    zero = np.zeros(shape)
    want, zr = host_residual(p, phi, zero, p.F, k, shift)
    got, got_zr = s.residual_norm(), s.state(0)["red_c"][0]
    print(f"  constant F: residual device {got:.16e} host {want:.16e}; (z0, r0) device {got_zr:.16e} host {zr:.16e}")
    assert abs(got - want) <= 1e-12 * want and abs(got_zr - zr) <= 1e-12 * zr
    r = np.where(p.inside_mask(), p.F, 0.0)[1:-1, 1:-1]  # w = 0: the residual is B itself
    ell = float(np.sqrt((r * r).sum() * p.h1 * p.h2))
    zr_ell = float((r * r / R.diag(a, b, p.h1, p.h2, shift)).sum() * p.h1 * p.h2)
    assert abs(got - ell) > 1e-9 * want and abs(got_zr - zr_ell) > 1e-9 * zr


@pytest.mark.parametrize("dtype", ["fp64", "mixed", "fp32"])
@pytest.mark.parametrize("name", ["disc", "two", "holed"])
@pytest.mark.parametrize("grid", GRIDS)
def test_solve_against_the_cpu_oracle(pkg, oracle, storage_gap, grid, name, dtype):
    """Both right-hand sides on 1, 2 and 4 subdomains, split by the reference rule and into row strips, under the
    rule of test_gpu_diffusion.py: fp64 the oracle's count and 1e-10 max|w|; fp32 / mixed the storage_gap bound
    (4 d top / top0) plus 4 * 2^-24 * top for the face coefficients rounded once to fp32."""
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
            s = pkg.make_session(o["p"], ranks=ranks, split=split, dtype=dtype, **o["kw"])
            assert s.algo_name == "pcg1" and s.tile["algo"] == "pcg1" and not s.tile.get("block_tiles")
            r = s.solve(rhs=o["f"] if rhs == "manuf" else None)
            err = np.abs(s.gather_local_w() - ref.w).max()
            print(f"{grid} {name} {dtype} {rhs} ranks {ranks} {split}: iters {r['iters']} (oracle {ref.iters}) "
                  f"max|w - w_cpu| {err:.3e} bound {t1:.3e} + {t2:.3e}")
            assert r["status"] == "converged"
            if dtype == "fp64":
                assert r["iters"] == ref.iters
            assert err <= t1 + t2


@pytest.mark.parametrize("ranks", [1, 4])
def test_bitwise(pkg, ranks):
    """domain alone is domain with diffusion = ones (the setup forms (0.5 (1 + 1)) a = a), and a device phi -- a
    [:, :N+1] view of a wider tensor -- is the host phi: iterations and w, bit for bit."""
    p = pkg.PoissonEllipse(M=97, N=130)
    phi = domains(p)[0]["disc"]
    N1 = p.N + 1
    wide = torch.full((p.M + 1, N1 + 3), float("nan"), dtype=torch.float64, device=DEV)
    wide[:, :N1] = dev(phi)
    assert not wide[:, :N1].is_contiguous()
    base = pkg.make_session(p, ranks=ranks, domain=phi)
    want = base.solve()
    w = base.gather_local_w()
    assert want["status"] == "converged"
    for tag, kw in (("ones", dict(domain=phi, diffusion=np.ones(phi.shape))), ("tensor", dict(domain=dev(phi))),
                    ("view", dict(domain=wide[:, :N1])), ("view + ones", dict(domain=wide[:, :N1],
                                                                             diffusion=dev(np.ones(phi.shape))))):
        s = pkg.make_session(p, ranks=ranks, **kw)
        got = s.solve()
        print(f"ranks {ranks} {tag}: iters {got['iters']} (domain alone {want['iters']})")
        assert got["iters"] == want["iters"] and s.gather_local_w().tobytes() == w.tobytes()
    assert torch.isnan(wide[:, N1:]).all()


@pytest.mark.parametrize("ranks", [1, 4])
def test_set_domain(pkg, ranks):
    """disc -> two on one session is a fresh `two` session, bitwise, on the graphs captured for the first solve --
    from a NumPy array, a device tensor and a view; with a diffusion field next to it likewise; step() before the
    next init raises; set_diffusion raises on the domain session, set_domain on sessions without a domain."""
    p = pkg.PoissonEllipse(M=97, N=130)
    phis, _ = domains(p)
    k = kappas(p)["smooth"]
    N1 = p.N + 1
    fresh = pkg.make_session(p, ranks=ranks, domain=phis["two"])
    want = fresh.solve()
    w_want = fresh.gather_local_w()
    fresh_k = pkg.make_session(p, ranks=ranks, domain=phis["two"], diffusion=k)
    want_k = fresh_k.solve()
    wk_want = fresh_k.gather_local_w()
    s = pkg.make_session(p, ranks=ranks, domain=phis["disc"])
    first = s.solve()
    assert first["status"] == "converged" and first["iters"] != want["iters"]
    lengths = s.path_stats()["graph_lengths"]
    wide = torch.full((p.M + 1, N1 + 3), float("nan"), dtype=torch.float64, device=DEV)
    wide[:, :N1] = dev(phis["two"])
    for kind, phi in (("numpy", phis["two"]), ("tensor", dev(phis["two"])), ("view", wide[:, :N1])):
        s.set_domain(phis["disc"])
        s.solve()
        s.set_domain(phi)
        assert s.has_domain and not s.has_diffusion
        with pytest.raises(RuntimeError, match="set_domain"):
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
    for kd in (k, dev(k)):
        s.set_domain(phis["two"], diffusion=kd)
        assert s.has_diffusion
        got = s.solve()
        assert got["iters"] == want_k["iters"] and s.gather_local_w().tobytes() == wk_want.tobytes()
    s.init()
    s.step(3)  # initialised again: stepping works
    s.synchronize()
    with pytest.raises(ValueError, match="set_domain"):
        s.set_diffusion(k)
    s.step(1)  # the refused call has not marked the state stale
    for kw in ({}, dict(diffusion=k), dict(reaction=reaction_fields(p)["smooth"])):
        other = pkg.make_session(p, ranks=ranks, **kw)
        assert not other.has_domain
        with pytest.raises(ValueError, match="domain"):
            other.set_domain(phis["two"])


def test_refusals(pkg, tmp_path):
    """What is not built for a domain raises ValueError, before anything is allocated (the refused sessions would
    hold ~0.4 GB each) and with the live session untouched."""
    big = pkg.PoissonEllipse(M=2000, N=3000)
    pb = domains(big)[0]["disc"]
    small = pkg.PoissonEllipse(M=97, N=130)
    phis, _ = domains(small)
    phi = phis["disc"]
    s = pkg.make_session(small, domain=phi)
    want = s.solve()
    w = s.gather_local_w()
    bad = {}
    for key, v, ij in (("nan", np.nan, (1234, 567)), ("inf", np.inf, (0, 0)), ("-inf", -np.inf, (2000, 3000))):
        bad[key] = pb.copy()
        bad[key][ij] = v
    # every device tensor of the refusals exists before the free memory is read (torch keeps freed blocks)
    bad_dev = {key: dev(field) for key, field in bad.items()}
    d = dev(pb)
    d32, dt = d.float(), d.t().contiguous().t()
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info()[0]
    for kw, name in ((dict(algo="ca"), "ca"), (dict(algo="pcg2"), "pcg2"), (dict(exact=True), "exact"),
                     (dict(block_tiles=1), "block_tiles")):
        for ranks in (1, 2):
            with pytest.raises(ValueError, match=name):
                pkg.make_session(big, ranks=ranks, domain=pb, **kw)
    for key, field in bad.items():
        for arg in (field, bad_dev[key]):  # the host scan, and the checking kernel on the device
            with pytest.raises(ValueError, match="domain"):
                pkg.make_session(big, domain=arg)
    for arg, what in ((d[:-1], "shape"), (d32, "float64"), (dt, "stride"),
                      (pb[:, :-1], "shape"), (pb.astype(np.float32), "float64"), (pb.tolist(), "domain")):
        with pytest.raises(ValueError, match=what):
            pkg.make_session(big, domain=arg)
    with pytest.raises(ValueError, match="diffusion"):  # the field next to the domain keeps its own rule
        pkg.make_session(big, domain=pb, diffusion=-np.ones(pb.shape))
    with pytest.raises(ValueError, match="domain"):
        sub("ops.kernels").DeviceOps(big, domain=pb)
    with pytest.raises(ValueError, match="domain"):
        sub("parallel.dist_solver").DistGpuPCG(big, None, comm="torch", domain=pb)
    with pytest.raises(ValueError, match="domain"):
        sub("models.sstep_pcg").TorchSStepPCG(small, domain=phi)
    with pytest.raises(ValueError, match="own"):  # multi-process transports
        pkg.load_native().Session(small.to_native(), world=1, comm="ipc", domain=phi)
    torch.cuda.synchronize()
    assert free0 - torch.cuda.mem_get_info()[0] < 100 << 20
    del bad_dev, d, d32, dt
    # the live session: bad fields and checkpoints are refused and leave it as it was
    for v, ij in ((np.nan, (50, 60)), (np.inf, (97, 130)), (-np.inf, (0, 5))):
        field = phis["two"].copy()
        field[ij] = v
        for arg in (field, dev(field)):
            with pytest.raises(ValueError, match="domain"):
                s.set_domain(arg)
    with pytest.raises(ValueError, match="diffusion"):
        s.set_domain(phis["two"], diffusion=np.zeros(phi.shape))
    s.step(1)  # no refused set_domain has marked the state stale
    ck = str(tmp_path / "domain.ck")
    with pytest.raises(ValueError, match="domain"):
        s.save_checkpoint(ck)
    with pytest.raises(ValueError, match="domain"):
        s.load_checkpoint(ck)
    with pytest.raises(ValueError, match="domain"):
        s.solve_checkpointed(ck, every=16)
    with pytest.raises(ValueError, match="domain"):
        s.error_norms()
    assert not (tmp_path / "domain.ck").exists()
    again = s.solve()
    assert again["iters"] == want["iters"] and np.array_equal(s.gather_local_w(), w)


@pytest.mark.parametrize("dtype", ["fp64", "fp32"])
@pytest.mark.parametrize("ranks", [1, 4])
def test_memory(pkg, ranks, dtype):
    """A domain session exceeds the matching diffusion session by the mask alone: at most one byte per node of the
    owned rows in the fields' pitch plus 256 B per subdomain -- and sessions without a domain report what the
    memory plan without the flag says (their own tests pin the formula)."""
    grid = (97, 130)
    p = pkg.PoissonEllipse(M=grid[0], N=grid[1])
    n = pkg.load_native()
    phi = domains(p)[0]["disc"]
    one = np.ones(phi.shape)
    a = pkg.make_session(p, ranks=ranks, dtype=dtype, diffusion=one)
    b = pkg.make_session(p, ranks=ranks, dtype=dtype, domain=phi)
    extra = b.device_bytes - a.device_bytes
    bound = 0
    for rank in range(ranks):
        plan = n.memory_plan(p.to_native(), ranks, n.Split.reference, rank, dtype, False, True)
        bound += plan["pitch"] * plan["nx"] + 256
    print(f"ranks {ranks} {dtype}: diffusion {a.device_bytes} B, domain + {extra} B (bound {bound})")
    assert 0 < extra <= bound
    assert b.tile == a.tile


def test_theta_scheme_one_step(pkg):
    """One Crank-Nicolson step on device tensors against the cpu backend's step on the disc: the domain is in the
    apply of the right-hand side, in the mask and in the solve."""
    p = pkg.PoissonEllipse(M=97, N=130)
    phi = domains(p)[0]["disc"]
    u0 = np.where(phi < 0, -phi, 0.0)
    dt = 1e-3
    dv = pkg.ThetaScheme(p, dt, theta=0.5, domain=dev(phi))
    hs = pkg.ThetaScheme(p, dt, theta=0.5, backend="cpu", domain=phi)
    assert dv.session.has_domain
    rhs_d, rhs_h = dv.rhs(dev(u0), 1.0).cpu().numpy(), hs.rhs(u0, 1.0)
    assert np.abs(rhs_d - rhs_h).max() <= 1e-12 * np.abs(rhs_h).max()
    u, want = dv.step(dev(u0), 1.0), hs.step(u0, 1.0)
    err = np.abs(u.cpu().numpy() - want).max()
    print(f"theta 1/2: iters {dv.last['iters']} (cpu {hs.last['iters']}) max|u - u_cpu| {err:.3e}")
    assert dv.last["status"] == "converged" and err <= 1e-10 * np.abs(want).max()


def test_quasilinear_picard_on_device_tensors(pkg):
    """-∇·((1 + u^2)∇u) = f on the disc on device tensors (one session, set_domain(phi, diffusion=κ(u_k)) per step)
    against the cpu backend: the same step count, u within 1e-10 max|u|; a device tensor out."""
    p = pkg.PoissonEllipse(M=40, N=40, stop="residual", rtol=1e-12, breakdown_tol=0.0)
    phi = domains(p)[0]["disc"]
    x, y = p.coords()
    X, Y = np.meshgrid(x, y, indexing="ij")
    f = 10.0 + 7.0 * X + 26.0 * Y

    def kappa(u):
        return 1.0 + u * u

    cpu = pkg.QuasilinearPicard(p, kappa, backend="cpu", picard_rtol=1e-8, domain=phi)
    want = cpu.solve(f)
    pc = pkg.QuasilinearPicard(p, kappa, picard_rtol=1e-8, domain=dev(phi))
    got = pc.solve(dev(f))
    assert isinstance(got, torch.Tensor) and got.is_cuda and pc.session.has_domain and pc.session.has_diffusion
    err = np.abs(got.cpu().numpy() - want).max()
    print(f"steps {pc.steps} (cpu {cpu.steps}), history {['%.3e' % h for h in pc.history]}, max|u - u_cpu| {err:.3e}")
    assert pc.converged and cpu.converged and pc.steps == cpu.steps
    assert all(b < a for a, b in zip(pc.history, pc.history[1:]))
    assert err <= 1e-10 * np.abs(want).max()
