"""The residual stop rule on the GPU: pcg1 (march and block tiles, k_pcg1 / k_pcg1_block through
pcg1_scalars), pcg2 (k_pcg_a's prologue, exact=True included), the s-step PCG (ca_finish's scalar lane), the
init's rho_B partial and threshold (k_init's data mode, k_stop_init), checkpoints, BackwardEuler and the refusals.

Yardstick: the project's CPU oracle (the reference has no such rule).  Exact counts are demanded under the
precondition of tests/test_stop_rule.py: the oracle returns the same count at rtol (1 -+ 1e-3), asserted by
the `oracle` fixture for every (grid, data, rtol) used.  Values picked on the CPU oracle, with their counts:

    400x600  f = 1           rtol 1e-5 -> 942 (0 mod 3, 0 mod 2, 0 mod 6)   1e-7 -> 1192 (1 mod 3, 0 mod 2, 4 mod 6)
                             rtol 1e-8 -> 1283 (2 mod 3, 1 mod 2, 5 mod 6)
    97x130   f = 1           rtol 1e-4 -> 176   1e-8 -> 282
    97x130   manufactured f  rtol 1e-8 -> 380
    40x40    manufactured f  rtol 1e-8 -> 122   (sigma = 100 at 97x130: counted by the oracle in the test)

Every problem sets breakdown_tol = 0: the reference's absolute guard |(A p, p)| < 1e-15 fires before a tight
relative tolerance is reached on data of this size and is not scale covariant (tests/test_stop_rule.py).
"""
import dataclasses

import numpy as np
import pytest
import torch

from conftest import sub
from test_init_data import manufactured

pytestmark = pytest.mark.gpu

COUNTS = {((400, 600), "const", 1e-5): 942, ((400, 600), "const", 1e-7): 1192, ((400, 600), "const", 1e-8): 1283,
          ((97, 130), "const", 1e-4): 176, ((97, 130), "const", 1e-8): 282, ((97, 130), "manuf", 1e-8): 380,
          ((40, 40), "manuf", 1e-8): 122}


@pytest.fixture(scope="module", autouse=True)
def gpu(pkg):
    assert torch.cuda.is_available() and pkg.load_native().device_count() > 0, "no HIP device"


def problem(pkg, grid, rtol=1e-8, **kw):
    kw.setdefault("breakdown_tol", 0.0)
    return pkg.PoissonEllipse(M=grid[0], N=grid[1], stop="residual", rtol=rtol, **kw)


def rhs_of(p, data):
    return None if data == "const" else manufactured(p)[0]


@pytest.fixture(scope="module")
def oracle(pkg):
    """CPU oracle solves, computed once per (grid, data, rtol, sigma) and shared; each asserts the
    precondition for exact counts (the OpenMP oracle runs the two probes of the big grid)."""
    cache = {}

    def get(grid, data, rtol, sigma=0.0):
        key = (grid, data, rtol, sigma)
        if key not in cache:
            p = problem(pkg, grid, rtol, sigma=sigma)
            f = rhs_of(p, data)
            big = grid[0] >= 400
            probes = [pkg.solve(dataclasses.replace(p, rtol=rtol * x), "omp" if big else "cpu", keep_solution=False,
                                rhs=f, **(dict(threads=8) if big else {})).iters for x in (1 - 1e-3, 1 + 1e-3)]
            assert probes[0] == probes[1], f"rtol {rtol} grazes the threshold at {grid}: {probes}"
            r = pkg.solve(p, "cpu", rhs=f)
            assert r.converged and r.iters == probes[0]
            if sigma == 0.0:
                assert r.iters == COUNTS[(grid, data, rtol)]
            cache[key] = dict(p=p, f=f, r=r)
        return cache[key]

    return get


def check(pkg, o, name, **session_kw):
    """One session solve against the oracle: exact count, w within 1e-10 max|w|, the reported norms."""
    ref = o["r"]
    s = pkg.make_session(o["p"], **session_kw)
    r = s.solve(rhs=o["f"])
    err = np.abs(s.gather_local_w() - ref.w).max()
    print(f"{name}: iters {r['iters']} (oracle {ref.iters}) max|w - w_cpu| {err:.3e} residual {r['residual']:.3e} "
          f"(oracle {ref.extra['residual']:.3e}) "
          f"ref {r['residual_ref']:.6e} algo {s.algo_name} tile {s.tile}")
    assert r["status"] == "converged" and r["iters"] == ref.iters
    assert err <= 1e-10 * np.abs(ref.w).max()
    assert r["residual_ref"] == pytest.approx(ref.extra["residual_ref"], rel=1e-12)
    assert r["residual"] <= o["p"].rtol * r["residual_ref"]
    st = s.state(0)
    assert st["stop"] == "residual" and st["residual"] == r["residual"] and st["residual_ref"] == r["residual_ref"]
    return s, r


# ---- counts and solution against the CPU oracle ------------------------------------------------------------

@pytest.mark.parametrize("rtol", [1e-5, 1e-8])
def test_pcg1_march_400x600(pkg, oracle, rtol):
    s, _ = check(pkg, oracle((400, 600), "const", rtol), f"march rtol {rtol}", algo="pcg1", block_tiles=0)
    assert s.algo_name == "pcg1" and not s.tile.get("block_tiles")


@pytest.mark.parametrize("data,rtol", [("const", 1e-4), ("const", 1e-8), ("manuf", 1e-8)])
def test_auto_97x130_runs_the_block_tiles(pkg, oracle, data, rtol):
    s, _ = check(pkg, oracle((97, 130), data, rtol), f"auto 97x130 {data} rtol {rtol}")
    assert s.algo_name == "pcg1" and s.tile.get("block_tiles")


@pytest.mark.parametrize("grid,data,rtol,kw", [((97, 130), "manuf", 1e-8, dict(algo="pcg2")),
                                                ((400, 600), "const", 1e-5, dict(algo="pcg2")),
                                                ((97, 130), "manuf", 1e-8, dict(exact=True)),
                                                ((400, 600), "const", 1e-5, dict(exact=True))])
def test_pcg2_and_exact(pkg, oracle, grid, data, rtol, kw):
    s, _ = check(pkg, oracle(grid, data, rtol), f"{kw} {grid}", **kw)
    assert s.algo_name == "pcg2"


@pytest.mark.parametrize("ca_s", [3, 2])
@pytest.mark.parametrize("rtol", [1e-5, 1e-7, 1e-8])
def test_sstep_400x600(pkg, oracle, ca_s, rtol):
    """The fused path as auto picks it; the three counts are 0, 1, 2 mod 3 (and 0, 0, 1 mod 2): the stop lands
    on every position inside a block."""
    s, _ = check(pkg, oracle((400, 600), "const", rtol), f"ca s {ca_s} rtol {rtol}", algo="ca", ca_s=ca_s)
    assert s.algo_name == "ca"


@pytest.mark.parametrize("ca_s", [3, 2])
@pytest.mark.parametrize("rtol", [1e-5, 1e-7])
def test_sstep_batch_boundary(pkg, oracle, ca_s, rtol):
    """Batches of 6 iterations: 942 is a multiple of the batch length (the stop is found by the batch-end
    check), 1192 is not (mid-batch)."""
    check(pkg, oracle((400, 600), "const", rtol), f"ca s {ca_s} batch 6 rtol {rtol}", algo="ca", ca_s=ca_s,
          graph_batch=6)


@pytest.mark.parametrize("graph_batch", [32, 5])
def test_pcg1_graph_batches(pkg, oracle, graph_batch):
    """380 iterations: mid-batch with batches of 32 (380 = 11 x 32 + 28), on a boundary with batches of 5."""
    for block_tiles in (0, 1):
        check(pkg, oracle((97, 130), "manuf", 1e-8), f"pcg1 batch {graph_batch} block_tiles {block_tiles}", algo="pcg1",
              block_tiles=block_tiles, graph_batch=graph_batch)


@pytest.mark.parametrize("algo", ["pcg1", "pcg2", "ca"])
@pytest.mark.parametrize("ranks,split", [(2, "rows"), (2, "reference"), (4, "rows"), (4, "reference")])
def test_decomposed(pkg, oracle, algo, ranks, split):
    grid, data, rtol = ((400, 600), "const", 1e-5) if algo == "ca" else ((97, 130), "manuf", 1e-8)
    check(pkg, oracle(grid, data, rtol), f"{algo} ranks {ranks} {split}", algo=algo, ranks=ranks, split=split)


@pytest.mark.parametrize("ranks,split", [(1, "reference"), (2, "rows"), (4, "reference")])
def test_sigma_100(pkg, oracle, ranks, split):
    s, _ = check(pkg, oracle((97, 130), "manuf", 1e-8, sigma=100.0), f"sigma 100 ranks {ranks} {split}", ranks=ranks,
                 split=split)
    assert s.algo_name == "pcg1" and not s.tile.get("block_tiles")


@pytest.mark.parametrize("dtype", ["fp32", "mixed"])
def test_fp32_and_mixed_storage(pkg, oracle, dtype):
    """pcg1 on the march at 97x130, f = 1, rtol 1e-4.  Count within 1 of fp64's.  The w bound is the existing
    storage tests' (tests/test_gpu_sigma.py storage_gap, test_gpu_init_data.py test_g4): 4 d, d = max|w_dtype -
    w_oracle| of the step-rule solve of the same problem in that storage, measured here against the fp64 CPU
    oracle (not against the path under test)."""
    o = oracle((97, 130), "const", 1e-4)
    step = pkg.PoissonEllipse(M=97, N=130)
    sref = pkg.make_session(step, algo="pcg1", block_tiles=0, dtype=dtype)
    assert sref.solve()["status"] == "converged"
    d = float(np.abs(sref.gather_local_w() - pkg.solve(step, "cpu").w).max())
    s = pkg.make_session(o["p"], algo="pcg1", block_tiles=0, dtype=dtype)
    r = s.solve()
    err = float(np.abs(s.gather_local_w() - o["r"].w).max())
    print(f"{dtype}: iters {r['iters']} (fp64 oracle {o['r'].iters}) max|w - w_cpu| {err:.3e} bound 4 d = {4 * d:.3e}")
    assert r["status"] == "converged" and abs(r["iters"] - o["r"].iters) <= 1
    assert d > 0.0 and err <= 4.0 * d


# ---- device-resident data, scale covariance -----------------------------------------------------------------

@pytest.mark.parametrize("kw", [dict(algo="pcg1", block_tiles=0), dict(algo="pcg1", block_tiles=1), dict(algo="pcg2"),
                                dict(algo="pcg1", ranks=2)])
def test_device_tensors_in_are_the_numpy_result(pkg, kw):
    p = problem(pkg, (97, 130), 1e-8)
    f = manufactured(p)[0]
    w0 = 0.5 * pkg.solve(p, "cpu", rhs=f).w
    s = pkg.make_session(p, **kw)
    a = s.solve(rhs=f, w0=w0)
    wa = s.gather_local_w()
    b = s.solve(rhs=torch.as_tensor(f).cuda(), w0=torch.as_tensor(w0).cuda())
    assert a["status"] == "converged" and a["iters"] > 0
    assert (b["iters"], b["residual"], b["residual_ref"]) == (a["iters"], a["residual"], a["residual_ref"])
    assert s.gather_local_w().tobytes() == wa.tobytes()


@pytest.mark.parametrize("block_tiles", [0, 1])
def test_scale_covariance(pkg, block_tiles):
    p = problem(pkg, (40, 40), 1e-8)
    f = manufactured(p)[0]
    s = pkg.make_session(p, algo="pcg1", block_tiles=block_tiles)
    a = s.solve(rhs=f)
    wa = s.gather_local_w()
    b = s.solve(rhs=f * 2.0 ** 20)
    assert a["iters"] == b["iters"] == COUNTS[((40, 40), "manuf", 1e-8)] and a["status"] == b["status"] == "converged"
    assert (wa * 2.0 ** 20).tobytes() == s.gather_local_w().tobytes()
    assert b["residual"] == a["residual"] * 2.0 ** 20


# ---- warm start ------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def tight(pkg):
    """The manufactured problem at 97x130 solved by the oracle to rtol 1e-10, once."""
    p = problem(pkg, (97, 130), 1e-10)
    f = manufactured(p)[0]
    return f, pkg.solve(p, "cpu", rhs=f).w


@pytest.mark.parametrize("kw", [dict(algo="pcg1", block_tiles=0), dict(algo="pcg1", block_tiles=1), dict(algo="pcg2"),
                                dict(algo="pcg1", ranks=4), dict(algo="pcg2", ranks=2, split="rows"), dict(algo="ca"),
                                dict(algo="ca", ranks=2, split="rows")])
def test_warm_start_good_enough_launches_nothing(pkg, tight, kw):
    f, w0 = tight
    p = problem(pkg, (97, 130), 1e-6)
    s = pkg.make_session(p, **kw)
    dev = torch.as_tensor(w0).cuda()
    r = s.solve(rhs=f, w0=dev)
    masked = np.zeros_like(w0)
    masked[1:-1, 1:-1] = w0[1:-1, 1:-1]
    assert r["status"] == "converged" and r["iters"] == 0 and r["launched"] == 0
    assert s.w_tensor().cpu().numpy().tobytes() == masked.tobytes()
    assert r["residual"] <= 1e-6 * r["residual_ref"]
    cold_ref = pkg.solve(p, "cpu", rhs=f, w0=w0).extra["residual_ref"]
    assert r["residual_ref"] == pytest.approx(cold_ref, rel=1e-12)
    # twice the data from the same start: iterations are needed, and the reference norm doubles
    r2 = s.solve(rhs=2.0 * f, w0=dev)
    assert r2["status"] == "converged" and r2["iters"] > 0
    assert r2["residual_ref"] == pytest.approx(2.0 * cold_ref, rel=1e-12)


def test_zero_data(pkg):
    p = problem(pkg, (40, 40))
    z = np.zeros((41, 41))
    for kw in (dict(algo="pcg1"), dict(algo="pcg2"), dict(algo="pcg1", ranks=2), dict(algo="ca")):
        r = pkg.make_session(p, **kw).solve(rhs=z, w0=z)
        assert r["status"] == "converged" and r["iters"] == 0 and r["launched"] == 0, kw


# ---- stepped use ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kw", [dict(algo="pcg1", block_tiles=0), dict(algo="pcg1", block_tiles=1), dict(algo="pcg2"),
                                dict(algo="pcg1", ranks=2), dict(algo="ca")])
def test_stepped_use_ends_at_the_same_count(pkg, oracle, kw):
    o = oracle((97, 130), "manuf", 1e-8)
    s = pkg.make_session(o["p"], **kw)
    want = s.solve(rhs=o["f"])
    w = s.gather_local_w()
    s.init(rhs=o["f"])
    for n in (7, 100, 1, 64, 200, 33):
        s.step(n)
    s.synchronize()
    while not s.state(0)["done"]:
        s.step(50)
        s.synchronize()
    st = s.state(0)
    assert want["iters"] == o["r"].iters and st["iters"] == want["iters"] and st["status"] == "converged"
    if kw["algo"] == "ca":
        # the pieces cut the blocks elsewhere than solve()'s batches do (a step of 7 is blocks of 3, 3, 1): other
        # Gram sums, so the same iterates to rounding and not bitwise -- w against the oracle as everywhere; g is
        # a quadratic form of sums that carry ~1e-13 relative rounding, compared to 1e-6
        assert st["residual"] == pytest.approx(want["residual"], rel=1e-6)
        assert np.abs(s.gather_local_w() - o["r"].w).max() <= 1e-10 * np.abs(o["r"].w).max()
    else:
        assert st["residual"] == want["residual"]
        assert s.gather_local_w().tobytes() == w.tobytes()


# ---- checkpoints ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kw", [dict(algo="pcg1"), dict(algo="pcg2"), dict(algo="pcg1", ranks=2), dict(algo="ca")])
def test_resume_is_bitwise(pkg, oracle, tmp_path, kw):
    o = oracle((400, 600), "const", 1e-5)
    path = str(tmp_path / "ck.bin")
    a = pkg.make_session(o["p"], **kw)
    ra = a.solve_checkpointed(path, every=100)
    wa = a.gather_local_w()
    b = pkg.make_session(o["p"], **kw)
    rb = b.solve_checkpointed(path, every=0, resume=True)
    assert ra["iters"] == rb["iters"] == o["r"].iters and rb["status"] == "converged"
    assert 0 < rb["launched"] < ra["launched"]
    assert b.gather_local_w().tobytes() == wa.tobytes()
    assert rb["residual"] == ra["residual"] and rb["residual_ref"] == ra["residual_ref"]


def test_checkpoint_carries_the_rule(pkg, tmp_path):
    step = pkg.PoissonEllipse(M=97, N=130)
    res = problem(pkg, (97, 130), 1e-8)
    ck_step, ck_res = str(tmp_path / "step.bin"), str(tmp_path / "res.bin")
    a = pkg.make_session(step, algo="pcg1")
    a.init()
    a.step(40)
    a.synchronize()
    a.save_checkpoint(ck_step)
    want = pkg.make_session(step, algo="pcg1").solve()
    b = pkg.make_session(step, algo="pcg1")
    rb = b.solve_checkpointed(ck_step, every=0, resume=True)  # step into step: as before
    assert rb["iters"] == want["iters"] == 143 and rb["status"] == "converged"
    c = pkg.make_session(res, algo="pcg1")
    with pytest.raises(RuntimeError, match=r"stop=step.*stop=residual rtol=1e-08"):
        c.load_checkpoint(ck_step)
    c.init()
    c.step(40)
    c.synchronize()
    c.save_checkpoint(ck_res)
    with pytest.raises(RuntimeError, match=r"stop=residual rtol=1e-08.*stop=step"):
        b.load_checkpoint(ck_res)
    other = pkg.make_session(problem(pkg, (97, 130), 1e-6), algo="pcg1")
    with pytest.raises(RuntimeError, match=r"rtol=1e-08.*rtol=1e-06"):
        other.load_checkpoint(ck_res)


# ---- layout --------------------------------------------------------------------------------------------------

def test_state_layout_is_the_parents(pkg, native):
    """320 bytes, measured on the parent build (comm_layout()["state_bytes"]); the reduction buffers sit where
    they sat (0 / 16 / 152 on the parent)."""
    L = native.comm_layout(pkg.PoissonEllipse(M=40, N=40).to_native(), 1, 1, 0)
    assert native.state_bytes == L["state_bytes"] == 320
    assert (L["red_a_off"], L["red_b_off"], L["red_c_off"]) == (0, 16, 152)


# ---- BackwardEuler ----------------------------------------------------------------------------------------------

def test_backward_euler_residual_rule(pkg):
    """Five steps at 97x130 on hip against the cpu backend: fields to 1e-10, equal per-step counts."""
    p = problem(pkg, (97, 130), 1e-8)
    dt = 1e-3
    hip, cpu = pkg.BackwardEuler(p, dt), pkg.BackwardEuler(p, dt, backend="cpu")
    assert hip.problem.stop == "residual" and hip.session.algo_name == "pcg1"
    u = torch.zeros(98, 131, dtype=torch.float64, device="cuda")
    v = np.zeros((98, 131))
    for n in range(5):
        u, v = hip.step(u, 1.0), cpu.step(v, 1.0)
        err = np.abs(u.cpu().numpy() - v).max()
        print(f"step {n + 1}: iters hip {hip.last['iters']} cpu {cpu.last['iters']} max|u - u_cpu| {err:.3e}")
        assert hip.last["status"] == cpu.last["status"] == "converged"
        assert hip.last["iters"] == cpu.last["iters"] > 0
        assert err <= 1e-10 * np.abs(v).max()
        assert hip.last["residual_ref"] == pytest.approx(cpu.last["residual_ref"], rel=1e-12)


def test_backward_euler_default_rule_is_unchanged(pkg):
    """Under the default rule a session made with the new arguments spelled out is bitwise the one made
    without them."""
    old = pkg.BackwardEuler(pkg.PoissonEllipse(M=97, N=130), 1e-3)
    new = pkg.BackwardEuler(pkg.PoissonEllipse(M=97, N=130, stop="step", rtol=1e-3, atol=1.0), 1e-3)
    u = w = torch.zeros(98, 131, dtype=torch.float64, device="cuda")
    for _ in range(5):
        u, w = old.step(u, 1.0), new.step(w, 1.0)
        assert old.last["iters"] == new.last["iters"] and old.last["diff"] == new.last["diff"]
        assert "residual" not in new.last
        assert torch.equal(u, w)
    assert "stop" not in new.session.state(0)


def test_auto_keeps_its_choice(pkg, native):
    """The rule changes no algorithm choice (choose_algo through the bindings, nothing allocated): the s-step
    from 6M points, pcg1 below."""
    for grid in ((2600, 2600), (400, 600)):
        step = native.choose_algo(pkg.PoissonEllipse(M=grid[0], N=grid[1]).to_native())
        assert native.choose_algo(problem(pkg, grid).to_native()) == step == (3 if grid[0] > 2000 else 1)


def test_python_orchestrated_paths_refuse(pkg):
    p = problem(pkg, (97, 130))
    with pytest.raises(ValueError, match="residual"):
        pkg.load_native().SubdomainSolver(p.to_native())
    with pytest.raises(ValueError, match="residual"):
        pkg.load_native().comm_layout(p.to_native(), 1, 1, 0)
