"""Which tile a plane-GEMM launch takes (csrc/gemm_planes.hip: plane_geo_for) is a rule of shapes, layouts and the tile knob --
no device.  The 96 x 64 tile (geometry 4) is a solo geometry: one job, k-major A, no split-K, more than 256 and at most 512
workgroups at 64 x 64, at most 256 at 96 x 64.  Everything else -- the gradient pairs bench.py asks about in particular, whose
answers index its four-entry geometry tables -- picks what it picked before that tile existed."""
import pytest

from slnlp import ops
from slnlp._lib import GemmArgs, check, load


def job(M, N, K, a_kmajor=True, b_kmajor=True, precision=3):
    """Shapes and layouts only: the rule reads no operand (the pointers are never followed)."""
    a = GemmArgs()
    a.M, a.N, a.K, a.a_kmajor, a.b_kmajor, a.precision = M, N, K, int(a_kmajor), int(b_kmajor), precision
    a.A_hi = a.A_lo = a.B_hi = a.B_lo = a.C = 64
    a.lda_p = a.ldb_p = 64
    a.ldc = N
    return a


def pair(M, E, F, wp, dp):
    """The gradient pair of one [M, E] dY against an [E, F] weight, as bench.py's roofline probes build it."""
    return job(E, F, M, False, False, wp), job(M, F, E, True, False, dp)


# (split, separate, geometry of the weight gradient's launch, of the data gradient's): recorded from the parent of the 96 x 64 tile
PAIRS = {(2400, 512, 512): (3, 0, 0, 0),        # bench.py dominant_kernel_roofline at cfg2
         (2400, 128, 256): (8, 0, 0, 0),        # ... cfg1
         (16384, 1024, 512): (8, 0, 2, 2),      # ... cfg5
         (16384, 3072, 1024): (5, 1, 3, 3)}     # large_launch_roofline (configs[4] in_proj)


@pytest.mark.parametrize("passes", [(2, 2), (3, 3), (2, 3), (1, 1)])
def test_gradient_pairs_pick_what_they_picked(passes):
    for (M, E, F), want in PAIRS.items():
        got = ops.gemm_wd_plan(*pair(M, E, F, *passes))
        assert got == want, (M, E, F, passes)
        assert max(got[2:]) <= 3                               # bench.py indexes four-entry tables with these


def test_the_window_is_cfg2s_2400_row_products_and_nothing_else():
    geo = lambda *a, **k: ops.plane_geo([job(*a, **k)])
    # cfg2 (E 512, F 512, 2400 rows): out_proj / linear1 / linear2 forward, the encoder data gradients, the in_proj data gradient
    assert geo(2400, 512, 512) == 4 and geo(2400, 512, 512, b_kmajor=False) == 4 and geo(2400, 512, 1536, b_kmajor=False) == 4
    assert geo(2400, 512, 512, b_kmajor=False, precision=2) == 4           # (two-pass backward setting)
    assert geo(2400, 1536, 512) == 1                                       # in_proj forward: 228 tiles of 128 x 128, as before
    # the window's edges: 257 .. 512 workgroups at 64 x 64, at most 256 at 96 x 64
    assert geo(64 * 32, 512, 512) == 0 and geo(64 * 32 + 1, 512, 512) == 4                # 256 | 264 at 64 x 64
    assert geo(96 * 32, 512, 512) == 4 and geo(96 * 32 + 1, 512, 512) == 0                # 256 | 264 at 96 x 64 (392 at 64 x 64: 98 of 128 x 128)
    # cfg1 (E 128, F 256) and cfg5 (16384 rows): far outside
    for N, K in [(128, 128), (256, 128), (128, 256), (384, 128)]:
        assert geo(2400, N, K) == 0 and geo(2400, N, K, b_kmajor=False) == 0
    assert geo(16384, 1024, 1024) == 2 and geo(16384, 3072, 1024) == 3 and geo(16384, 512, 1024) == 2
    assert geo(16384, 1024, 512, b_kmajor=False) != 4 and geo(16384, 1024, 3072, b_kmajor=False) != 4


def test_never_for_split_k_groups_wgrad_layouts_or_fp8():
    j = job(2400, 512, 512)
    assert ops.plane_geo([j], [2]) != 4                                    # split-K
    assert ops.plane_geo([j, job(2400, 512, 512, b_kmajor=False)]) != 4    # a grouped launch
    assert ops.plane_geo([job(2400, 512, 512, a_kmajor=False, b_kmajor=False)]) != 4     # A m-major (a weight gradient)
    assert ops.plane_geo([job(2400, 512, 512, precision=8)]) == 0          # fp8 launches have their own geometries


def test_the_forced_knob_reaches_only_what_the_tile_can_run():
    try:
        check(load().slnlp_set_plane_tile(96), "set_plane_tile")
        assert ops.plane_geo([job(50, 64, 64)]) == 4
        assert ops.plane_geo([job(50, 64, 128)], [2]) == 0
        assert ops.plane_geo([job(64, 64, 2400, a_kmajor=False, b_kmajor=False)]) == 0
        assert ops.gemm_wd_plan(*pair(2400, 512, 512, 2, 2))[2:] == (0, 0)
        check(load().slnlp_set_plane_tile(64), "set_plane_tile")
        assert ops.plane_geo([job(2400, 512, 512)]) == 0
    finally:
        load().slnlp_set_plane_tile(0)
    assert ops.plane_geo([job(2400, 512, 512)]) == 4
