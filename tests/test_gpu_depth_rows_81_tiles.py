"""GPU: the rows sum the five depth-prior libraries share (depthprior::rows_partials, csrc/depth_prior_device.h) on
frames of MORE than 64 tiles.  Lane l of the rows kernel adds the partials of tiles l, l + 64, ...; every other shape of the suites
has at most 12 tiles per frame, so there the loop's second round never runs.  Here a frame has 81 tiles (9 x 9): 72 x 264 for the
libraries with tiles of 32 x 8 (consistency, accumulation, points) and 144 x 264 for those with tiles of 32 x 16 (completion, plane
sweep).

Gates: those of each library's own suite (tests/test_gpu_depth_*.py), through that suite's own comparison -- every output equal to
the library's reference module at this shape, the float32 planes as bits (the consistency check's std_out within its 2 ulp) -- and
every column of rows non-zero in every frame, so that no column is equal for want of anything to count.  Two frames, one
neighbour; the sweep with the fewest planes and the pixel alone as its aggregation window.  The references' rows on these inputs,
computed without a device: consistency [[19008, 17411, 15840, 3168], [19008, 17594, 15821, 3187]], accumulation [[950, 803, 799, 4],
[936, 813, 811, 2]], points [[1750, 1598, 1371, 26], [1750, 1536, 1326, 39]], completion [[1886, 22578, 350, 13202], [1944, 22712,
1016, 12344]], sweep [[19375, 15035, 731, 2875], [20678, 13988, 708, 2642]]; each reference takes under 0.3 s.
"""
import numpy as np
import pytest

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

from tests.test_gpu_mip360 import T, dev                                                 # noqa: E402
from tests.test_depth_consistency import analytic_scene, corrupted                       # noqa: E402
from tests.test_depth_accumulate import prior_of                                         # noqa: E402

S8, S16 = (2, 72, 264), (2, 144, 264)                    # 9 x 9 tiles of 32 x 8 and of 32 x 16


def one_neighbour(shape):
    s = analytic_scene(shape, box=True)
    return s, np.ascontiguousarray(s['nbr'][:, :1])


def rows_consistency():
    from outdoor_nerf_depth_amd import depth_consistency as DC
    from tests.test_gpu_depth_consistency import assert_matches
    s, nbr = one_neighbour(S8)
    return assert_matches(DC, corrupted(prior_of('exact', S8))[0], s['cams'], nbr, 'consistency, 81 tiles', min_views=1)['rows']


def rows_accumulation():
    from outdoor_nerf_depth_amd import depth_accumulate as DA
    from tests.test_gpu_depth_accumulate import assert_matches
    s, nbr = one_neighbour(S8)
    return assert_matches(DA, prior_of('sparse', S8), s['cams'], nbr, 'accumulation, 81 tiles')['rows']


def rows_points():
    from tests import depth_points_reference as R
    from tests.test_depth_points import cloud
    from tests.test_gpu_depth_points import PARAMS, assert_equal
    from outdoor_nerf_depth_amd import depth_points as DP
    c = cloud(S8)
    got = DP.splat_async(c['cams'], c['points'], None, S8, device=dev(), occl_radius=2, **PARAMS).get()
    assert_equal(got, R.splat(c['cams'], c['points'], None, S8, occl_radius=2, **PARAMS), 'points, 81 tiles')
    return got['rows']


def rows_completion():
    from tests import depth_complete_reference as R
    from tests.test_depth_complete import guide_of, std_of
    from tests.test_gpu_depth_complete import assert_equal
    from outdoor_nerf_depth_amd import depth_complete as DCP
    depth, rgb, std = prior_of('sparse', S16), guide_of(S16), std_of(S16)
    ws, wc = R.tables(2, 2.0, 300.0)                                                         # a weak guide and a tight spread gate:
    got = DCP.complete_async(T(depth), T(rgb), T(std), w_space=ws, w_colour=wc, radius=2, iters=2, max_rel_spread=0.01).get()   # windows to refuse
    assert_equal(got, R.complete(depth, rgb, std, ws, wc, 2, 2, max_rel_spread=0.01), 'completion, 81 tiles')
    return got['rows']


def rows_sweep():
    from tests import depth_mvs_reference as R
    from tests.test_depth_mvs import textured_images
    from tests.test_gpu_depth_mvs import assert_equal, run
    from outdoor_nerf_depth_amd import depth_mvs as DM
    s, nbr = one_neighbour(S16)
    rgb, table = textured_images(s['K'], s['c2w'], s['depth']), DM.planes_table(2.0, 12.0, DM.MIN_PLANES)
    got = run(DM, rgb, s['cams'], nbr, table, agg_radius=0)
    assert_equal(got, R.sweep(rgb, s['cams'], nbr, table, None, 0), 'sweep, 81 tiles')
    return got['rows']


@pytest.mark.parametrize('library', (rows_consistency, rows_accumulation, rows_points, rows_completion, rows_sweep),
                         ids=lambda f: f.__name__[5:])
def test_rows_of_frames_with_81_tiles(library):
    dev()
    rows = library()
    print('%s: rows %s' % (library.__name__[5:], rows.tolist()))
    assert rows.shape == (2, 4) and (rows > 0).all()                                        # every column has something to count
