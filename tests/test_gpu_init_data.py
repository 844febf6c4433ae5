"""A user-supplied right-hand side and initial guess on the GPU: Session.init(rhs=, w0=), the data
variant of k_init (pcg_kernels.hip) under all three iteration algorithms, and Session.residual_norm.

Manufactured problem as in test_init_data.py: u = (1 - x^2 - 4y^2)(1 + x/2 + y), f = 10 + 7x + 26y.
"""
import numpy as np
import pytest
import torch

from conftest import sub
from test_init_data import CONTINUE, COUNTS, GRIDS, manufactured

pytestmark = pytest.mark.gpu

# every algorithm in both of its variants (graph batches of 32), and one of each with eager launches
CONFIGS = {
    "ca-s2": dict(algo="ca", ca_s=2),
    "ca-s3": dict(algo="ca", ca_s=3),
    "pcg1-march": dict(algo="pcg1", block_tiles=0),
    "pcg1-block": dict(algo="pcg1", block_tiles=1),
    "pcg2": dict(algo="pcg2", exact=False),
    "pcg2-exact": dict(algo="pcg2", exact=True),
    "ca-s3-eager": dict(algo="ca", ca_s=3, graph_batch=0),
    "pcg1-march-eager": dict(algo="pcg1", block_tiles=0, graph_batch=0),
    "pcg2-eager": dict(algo="pcg2", graph_batch=0),
}
ALGOS = ["ca-s3", "pcg1-march", "pcg2"]
RANKS = {1: "reference", 2: "rows", 3: "rows", 4: "reference"}


@pytest.fixture(scope="module", autouse=True)
def gpu(pkg):
    assert torch.cuda.is_available() and pkg.load_native().device_count() > 0, "no HIP device"


@pytest.fixture(scope="module")
def oracle(pkg):
    """CPU oracle results shared by the tests, computed once per grid: the constant-F solve, the
    manufactured solve cold and from w0 = 10 w_const, and the continuation of w_const to delta = 1e-9."""
    out = {}
    for M, N in GRIDS:
        p = pkg.PoissonEllipse(M=M, N=N)
        f, u = manufactured(p)
        const = pkg.solve(p, "cpu")
        cold = pkg.solve(p, "cpu", rhs=f)
        warm = pkg.solve(p, "cpu", rhs=f, w0=10.0 * const.w)
        tight = pkg.solve(pkg.PoissonEllipse(M=M, N=N, delta=1e-9), "cpu", w0=const.w)
        assert (const.iters, cold.iters, warm.iters) == COUNTS[(M, N)] and tight.iters == CONTINUE[(M, N)][0]
        out[(M, N)] = dict(f=f, u=u, const=const, cold=cold, warm=warm, tight=tight)
    return out


def _session(pkg, grid, cfg, ranks=1, problem=None, **kw):
    p = pkg.PoissonEllipse(M=grid[0], N=grid[1], **(problem or {}))
    return pkg.make_session(p, ranks=ranks, split=RANKS[ranks], **{**CONFIGS[cfg], **kw})


@pytest.mark.parametrize("ranks", list(RANKS))
@pytest.mark.parametrize("dtype", ["fp64", "fp32", "mixed"])
@pytest.mark.parametrize("cfg", list(CONFIGS))
def test_g1_default_data_is_bitwise_the_plain_session(pkg, cfg, dtype, ranks):
    """init(rhs = F everywhere, w0 = 0) -- both, or either alone -- then a solve: the count and the
    gathered w of the plain session, bitwise."""
    grid = (97, 130)
    shape = (grid[0] + 1, grid[1] + 1)
    F, Z = np.full(shape, 1.0), np.zeros(shape)

    def run(**data):  # the same stepping for every run: the s-step's blocks follow the batch boundaries
        s = _session(pkg, grid, cfg, ranks, dtype=dtype)
        s.init(**data)
        while not s.state(0)["done"]:
            s.step(64)
        return s.state(0), s.gather_local_w()

    ref, wref = run()
    assert ref["status"] == "converged"
    for data in (dict(rhs=F, w0=Z), dict(rhs=F), dict(w0=Z)):
        st, w = run(**data)
        assert (st["iters"], st["status"]) == (ref["iters"], ref["status"]), (data.keys(), st, ref)
        assert np.array_equal(w, wref), data.keys()
    if dtype == "fp64":
        assert ref["iters"] == COUNTS[grid][0]


@pytest.mark.parametrize("ranks", [1, 4])
@pytest.mark.parametrize("grid", GRIDS)
@pytest.mark.parametrize("cfg", list(CONFIGS))
def test_g2_manufactured_against_the_cpu_oracle(pkg, oracle, cfg, grid, ranks):
    o = oracle[grid]
    for name, w0 in (("cold", None), ("warm", 10.0 * o["const"].w)):
        s = _session(pkg, grid, cfg, ranks)
        r = s.solve(rhs=o["f"], w0=w0)
        w = s.gather_local_w()
        err = np.abs(w - o[name].w).max()
        print(f"{cfg} {grid} ranks={ranks} {name}: iters {r['iters']} (oracle {o[name].iters}) "
              f"diff {r['diff']:.6e} (oracle {o[name].diff:.6e}) max|w - w_cpu| {err:.3e}")
        assert r["iters"] == o[name].iters and r["status"] == "converged"
        assert err <= 1e-10 * np.abs(o[name].w).max()


@pytest.mark.parametrize("grid", GRIDS)
@pytest.mark.parametrize("cfg", list(CONFIGS))
def test_g3_warm_start(pkg, oracle, cfg, grid):
    s = _session(pkg, grid, cfg)
    first = s.solve()
    assert first["iters"] == COUNTS[grid][0]
    w = s.gather_local_w()
    again = s.solve(w0=w)  # from the session's own converged iterate
    assert again["iters"] == 1 and again["status"] == "converged"
    # continuation at a tighter delta reproduces the oracle's warm count
    t = _session(pkg, grid, cfg, problem=dict(delta=1e-9))
    cont = t.solve(w0=w)
    print(f"{cfg} {grid}: continuation {cont['iters']} {cont['status']} (oracle {oracle[grid]['tight'].iters} "
          f"{oracle[grid]['tight'].status})")
    assert cont["iters"] == oracle[grid]["tight"].iters == CONTINUE[grid][0]
    assert np.abs(t.gather_local_w() - oracle[grid]["tight"].w).max() <= 1e-6
    # the data is consumed by its init: a plain init() afterwards is the cold constant-F solve again
    back = s.solve()
    fresh = _session(pkg, grid, cfg)
    assert back["iters"] == fresh.solve()["iters"] == COUNTS[grid][0]
    assert np.array_equal(s.gather_local_w(), fresh.gather_local_w())
    assert np.array_equal(s.gather_local_w(), w)


@pytest.mark.parametrize("dtype", ["fp32", "mixed"])
@pytest.mark.parametrize("cfg", ALGOS)
def test_g4_reduced_storage(pkg, oracle, cfg, dtype):
    """fp32 / mixed storage with the manufactured f: the fp64 count, and a solution as close to its fp64
    twin as the constant-F path is to its own (d), scaled by the solutions' sizes, with a margin of 4 for
    the different right-hand side."""
    grid = (97, 130)
    o = oracle[grid]

    def run(dt, **data):
        s = _session(pkg, grid, cfg, dtype=dt)
        r = s.solve(**data)
        return r, s.gather_local_w()

    r64c, w64c = run("fp64")
    rc, wc = run(dtype)
    d = np.abs(wc - w64c).max()
    r64, w64 = run("fp64", rhs=o["f"])
    r, w = run(dtype, rhs=o["f"])
    got = np.abs(w - w64).max()
    bound = 4.0 * d * np.abs(o["u"]).max() / np.abs(w64c).max()
    print(f"{cfg} {dtype}: constant-F discrepancy d = {d:.3e}, manufactured {got:.3e}, bound {bound:.3e}; "
          f"iters {r['iters']} (fp64 {r64['iters']})")
    assert r["iters"] == r64["iters"] == COUNTS[grid][1] and r["status"] == "converged"
    assert d > 0.0 and got <= bound


def _host_residual(pkg, p, w, rhs, dt):
    """sqrt(h1 h2 sum (B - A w)^2) on the host with ops/reference.apply_A, evaluated in dtype dt."""
    R = sub("ops.reference")
    sd = sub("parallel.decomp").subdomain(p.M, p.N, 1, 1, 0)
    a, b, _ = R.assemble(p, sd)
    a, b = a.numpy().astype(dt), b.numpy().astype(dt)
    B = np.where(p.inside_mask(), rhs, 0.0)[1:-1, 1:-1].astype(dt)
    res = B - R.apply_A(w.astype(dt), a, b, dt(p.h1), dt(p.h2))
    return np.sqrt((res * res).sum() * dt(p.h1) * dt(p.h2))


@pytest.mark.parametrize("grid", GRIDS)
@pytest.mark.parametrize("cfg", ALGOS + ["pcg1-block", "ca-s2"])
def test_g5_residual_norm(pkg, oracle, cfg, grid):
    """The device residual against B - A w on the host from gather_local_w(): after 10 and 11 iterations
    (pcg1 / pcg2 hold pending w steps there) and after convergence.  e = the discrepancy of the host value
    between float64 and long double; the device may differ from the float64 one by max(10 e, 1e-12 value)."""
    f = oracle[grid]["f"]

    def check(s, p, rhs_arg, rhs):
        w = s.gather_local_w()
        h64 = float(_host_residual(pkg, p, w, rhs, np.float64))
        hld = float(_host_residual(pkg, p, w, rhs, np.longdouble))
        e = abs(h64 - hld)
        got = s.residual_norm(rhs_arg)
        print(f"{cfg} {grid}: device {got:.16e} host {h64:.16e} e {e:.3e} "
              f"pending {s.state(0)['w_pend_n']} / {s.state(0)['w_pend']}")
        assert abs(got - h64) <= max(10.0 * e, 1e-12 * h64)
        assert np.array_equal(s.gather_local_w(), w)  # measuring moves nothing
        return got

    early = []
    for n in (10, 11):  # pcg1 holds pending steps after either, pcg2 after an odd count
        short = _session(pkg, grid, cfg, problem=dict(max_iter=n))
        r = short.solve(rhs=f)
        assert r["iters"] == n and r["status"] == "max_iter"
        early.append(check(short, pkg.PoissonEllipse(M=grid[0], N=grid[1], max_iter=n), f, f))
    full = _session(pkg, grid, cfg)
    p = pkg.PoissonEllipse(M=grid[0], N=grid[1])
    assert full.solve(rhs=f)["status"] == "converged"
    late = check(full, p, f, f)
    assert late < min(early)
    # rhs = None: the constant F of a default session
    default = _session(pkg, grid, cfg)
    default.solve()
    check(default, p, None, np.full((p.M + 1, p.N + 1), p.F))


def test_g5_residual_norm_needs_an_undecomposed_session(pkg, native):
    s = _session(pkg, (40, 60), "pcg1-march", ranks=2)
    s.solve()
    with pytest.raises(native.PmxError, match="world == 1"):
        s.residual_norm()


def test_g6_checkpoint_carries_the_data(pkg, oracle, tmp_path):
    """r carries the right-hand side: a checkpoint of a manufactured solve resumes in a session that
    never saw f, bitwise."""
    grid, ck = (97, 130), str(tmp_path / "manuf.ck")
    f = oracle[grid]["f"]
    whole = _session(pkg, grid, "pcg1-march")
    ref = whole.solve(rhs=f)
    a = _session(pkg, grid, "pcg1-march")
    a.init(rhs=f)
    a.step(32)
    a.synchronize()
    a.save_checkpoint(ck)
    b = _session(pkg, grid, "pcg1-march")
    r = b.solve_checkpointed(ck, every=0, resume=True)
    assert r["iters"] == ref["iters"] == COUNTS[grid][1] and r["status"] == "converged"
    assert np.array_equal(b.gather_local_w(), whole.gather_local_w())


# device_bytes of a 97 x 130 session without the placement probe by (cfg, dtype, ranks), as before this
# feature; the fp32 and 4-rank entries were recorded before the layout moved into MemoryPlan
DEVICE_BYTES = {
    ("ca-s3", "fp64", 1): 949800, ("pcg1-march", "fp64", 1): 693088, ("pcg2", "fp64", 1): 541280,
    ("ca-s3", "fp64", 4): 1565120, ("pcg1-march", "fp64", 4): 940160, ("pcg2", "fp64", 4): 730240,
    ("ca-s3", "fp32", 1): 730664, ("pcg1-march", "fp32", 1): 421472, ("pcg2", "fp32", 1): 331488,
    ("ca-s3", "fp32", 4): 1286592, ("pcg1-march", "fp32", 4): 645248, ("pcg2", "fp32", 4): 509056,
}


def _estimate(pkg, grid, cfg, dtype, ranks):
    """Sum over the ranks of native.estimate_device_bytes: an upper bound of device_bytes."""
    native = pkg.load_native()
    spec = pkg.PoissonEllipse(M=grid[0], N=grid[1]).to_native()
    algo = {"ca": 3, "pcg1": 1, "pcg2": 2}[CONFIGS[cfg]["algo"]]
    return sum(native.estimate_device_bytes(spec, ranks, getattr(native.Split, RANKS[ranks]), r, dtype, algo)
               for r in range(ranks))


@pytest.mark.parametrize("cfg", ALGOS)
def test_g7_nothing_is_retained(pkg, oracle, cfg):
    grid = (97, 130)
    s = _session(pkg, grid, cfg, placement=0)
    before = s.device_bytes
    s.solve(rhs=oracle[grid]["f"], w0=10.0 * oracle[grid]["const"].w)
    s.residual_norm(oracle[grid]["f"])
    assert s.device_bytes == before == DEVICE_BYTES[cfg, "fp64", 1]
    assert s.device_bytes <= _estimate(pkg, grid, cfg, "fp64", 1)


@pytest.mark.parametrize("ranks", [1, 4])
@pytest.mark.parametrize("dtype", ["fp64", "fp32"])
@pytest.mark.parametrize("cfg", ALGOS)
def test_allocated_bytes_are_pinned_and_below_the_estimate(pkg, cfg, dtype, ranks):
    """What a session allocates is what it allocated before the memory plan, and the estimate that sizes the
    algorithm choice bounds it (here by its 1 MiB term alone)."""
    grid = (97, 130)
    s = _session(pkg, grid, cfg, ranks, dtype=dtype, placement=0)
    assert s.device_bytes == DEVICE_BYTES[cfg, dtype, ranks]
    assert s.device_bytes <= _estimate(pkg, grid, cfg, dtype, ranks)


@pytest.mark.parametrize("arg", ["rhs", "w0"])
def test_bad_input_raises_before_anything_is_uploaded(pkg, arg):
    s = _session(pkg, (40, 60), "pcg1-march")
    good = np.ones((41, 61))
    nan = good.copy()
    nan[7, 7] = np.nan
    for bad in (np.ones((41, 60)), good.astype(np.float32), nan, good.tolist(), torch.ones(41, 61, device="cuda")):
        with pytest.raises(ValueError):
            s.init(**{arg: bad})
        with pytest.raises(ValueError):
            s.solve(**{arg: bad})
    with pytest.raises(ValueError):
        s.residual_norm(nan)
    # the session is untouched: its plain solve is the default one
    assert s.solve()["iters"] == COUNTS[(40, 60)][0]
    assert s.solve(**{arg: torch.from_numpy(good)})["status"] == "converged"
