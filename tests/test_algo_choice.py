"""The iteration algorithm auto picks (choose_algo, gpu_solver.hip) and the memory plan it is sized
by -- pure host functions, no device.  SURVEY §5.7: grids sized against 288 GB of HBM per MI355X."""
import pytest


@pytest.fixture(scope="module")
def spec(pkg):
    return lambda M, N, **kw: pkg.PoissonEllipse(M=M, N=N, **kw).to_native()


def test_auto_picks_the_sstep_on_big_fp64_grids_and_strips(native, spec):
    assert native.choose_algo(spec(16384, 16384)) == 3
    assert native.choose_algo(spec(16384, 16384), world=8) == 3           # 8 row strips (split auto)
    assert native.choose_algo(spec(2600, 2600)) == 3                      # >= 6M points
    assert native.choose_algo(spec(1600, 2400)) == 1                      # the reference grids: pcg1
    assert native.choose_algo(spec(800, 1200)) == 1


def test_auto_keeps_pcg1_where_the_sstep_does_not_apply(native, spec):
    big = spec(16384, 16384)
    assert native.choose_algo(big, world=8, split=native.Split.reference) == 3  # 2 x 4 blocks (config 4)
    assert native.choose_algo(spec(3000, 3000), world=64, split=native.Split.reference) == 3  # 375 x 375 blocks
    assert native.choose_algo(spec(2600, 2600), world=1024, split=native.Split.rows) == 1  # 2-row strips
    assert native.choose_algo(big, dtype="fp32") == 3      # fp32 fields, fp64 basis and sums
    assert native.choose_algo(big, dtype="mixed") == 3
    assert native.choose_algo(spec(800, 1200), dtype="fp32") == 1
    assert native.choose_algo(big, exact=True) == 2                       # reference arithmetic order
    assert native.choose_algo(big, algo=1) == 1 and native.choose_algo(big, algo=2) == 2
    assert native.choose_algo(spec(800, 1200), algo=3) == 3                # explicit


def test_memory_fallback_to_pcg1(native, spec):
    """The s-step's 7 fields must fit (with 5% headroom), else auto falls back to pcg1's 5, then pcg2."""
    s = spec(16384, 16384)
    ca = native.estimate_device_bytes(s, algo=3)
    p1 = native.estimate_device_bytes(s, algo=1)
    p2 = native.estimate_device_bytes(s, algo=2)
    assert ca > p1 > p2
    assert 7 * 8 * 16383 ** 2 < ca < 1.05 * 7 * 8 * 16383 ** 2
    assert native.choose_algo(s, device_bytes=288e9) == 3
    assert native.choose_algo(s, device_bytes=ca / 0.95 * 1.001) == 3
    assert native.choose_algo(s, device_bytes=ca / 0.95 * 0.99) == 1     # s-step no longer fits: pcg1
    assert native.choose_algo(s, device_bytes=p1 / 0.95 * 0.99) == 2     # pcg1 neither: pcg2
    # ranks sharing one device count together
    assert native.choose_algo(s, world=8, device_bytes=288e9, per_device=8) == 3
    assert native.choose_algo(s, world=8, device_bytes=ca / 0.95, per_device=8) == 1


def test_max_square_grid_by_algorithm(native):
    g1 = native.max_square_grid(288e9, 1, "fp64", 0.1, 1)
    g3 = native.max_square_grid(288e9, 1, "fp64", 0.1, 3)
    auto = native.max_square_grid(288e9, 1, "fp64", 0.1)
    assert auto == g1 > g3 > 60000          # auto falls back to pcg1: its 5 fields bound the grid
    assert native.max_square_grid(288e9, 8, "fp64", 0.1, 3) > 2.8 * g3
    assert native.max_square_grid(288e9, 1, "fp32", 0.1, 1) > 1.4 * g1


# estimate_device_bytes for algo 1, 2, 3 by (grid, world, split, rank, dtype), recorded before the layout
# moved into MemoryPlan (pmx/memory_plan.hpp): the plan must not move a byte, or choose_algo decides otherwise
ESTIMATES = {
    ((40, 40), 1, "auto", 0, "fp64"): (1177608, 1147144, 1222992),
    ((40, 40), 1, "auto", 0, "fp32"): (1118472, 1101064, 1163856),
    ((40, 40), 4, "reference", 0, "fp64"): (1093752, 1081208, 1193136),
    ((40, 40), 4, "reference", 0, "fp32"): (1091704, 1081208, 1141936),
    ((40, 40), 4, "reference", 3, "fp64"): (1092472, 1080184, 1189552),
    ((40, 40), 4, "reference", 3, "fp32"): (1090424, 1080184, 1139632),
    ((40, 40), 8, "rows", 0, "fp64"): (1085792, 1075808, 1139728),
    ((40, 40), 8, "rows", 0, "fp32"): (1072224, 1065568, 1107728),
    ((40, 40), 8, "rows", 7, "fp64"): (1083192, 1073720, 1136144),
    ((40, 40), 8, "rows", 7, "fp32"): (1070904, 1064504, 1105424),
    ((97, 130), 1, "auto", 0, "fp64"): (1738552, 1586744, 1997920),
    ((97, 130), 1, "auto", 0, "fp32"): (1468216, 1378872, 1778784),
    ((97, 130), 4, "reference", 0, "fp64"): (1280016, 1227536, 1436528),
    ((97, 130), 4, "reference", 0, "fp32"): (1206288, 1172240, 1366896),
    ((97, 130), 4, "reference", 3, "fp64"): (1278992, 1226512, 1435504),
    ((97, 130), 4, "reference", 3, "fp32"): (1205264, 1171216, 1365872),
    ((97, 130), 8, "rows", 0, "fp64"): (1185672, 1149576, 1339264),
    ((97, 130), 8, "rows", 0, "fp32"): (1135496, 1114760, 1261440),
    ((97, 130), 8, "rows", 7, "fp64"): (1185672, 1149576, 1339264),
    ((97, 130), 8, "rows", 7, "fp32"): (1135496, 1114760, 1261440),
    ((16384, 16384), 1, "auto", 0, "fp64"): (10851075776, 8695855808, 15169038016),
    ((16384, 16384), 1, "auto", 0, "fp32"): (5479286464, 4399577792, 9805638848),
    ((16384, 16384), 4, "reference", 0, "fp64"): (2722019304, 2181212904, 3811676912),
    ((16384, 16384), 4, "reference", 0, "fp32"): (1378138088, 1106684648, 2468586224),
    ((16384, 16384), 4, "reference", 3, "fp64"): (2721526464, 2180785856, 3811192512),
    ((16384, 16384), 4, "reference", 3, "fp32"): (1377809088, 1106388672, 2468265152),
    ((16384, 16384), 8, "rows", 0, "fp64"): (1362906048, 1091649216, 1915719712),
    ((16384, 16384), 8, "rows", 0, "fp32"): (689327040, 553434816, 1238212640),
    ((16384, 16384), 8, "rows", 7, "fp64"): (1362249408, 1091123904, 1914752704),
    ((16384, 16384), 8, "rows", 7, "fp32"): (688998080, 553171648, 1237572800),
}


@pytest.mark.parametrize("case", list(ESTIMATES), ids=lambda c: "-".join(str(x) for x in c[0] + c[1:]))
def test_memory_plan_estimates_are_pinned(native, spec, case):
    (M, N), world, split, rank, dtype = case
    got = tuple(native.estimate_device_bytes(spec(M, N), world, getattr(native.Split, split), rank, dtype, algo)
                for algo in (1, 2, 3))
    assert got == ESTIMATES[case]
