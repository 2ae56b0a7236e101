"""GPU parity of the depth-projection association (csrc/proj.hip) on the paths tests/test_proj_gpu.py never takes:
splats three and four bitmap words wide, one-pixel splats, row groups of every length, image borders, narrow images
and word edges, several features in one pixel, the scale-selection boundaries, anisotropic submaps with negative
keys, a batch that needs two trips through the chunk loop, the grid-stride step of the feature kernels, handle
reuse, non-finite features and featureless batches.  tests/test_proj_edge_cpu.py proves on the CPU (census) that
each scene reaches the path named here, and that a second, independent reference agrees with the oracle on it.

Every comparison is the one of test_proj_gpu: found, index, dist bits and the 6-vector exactly, cam_xyz at 1e-12,
last_pairs equal.

Left out: the second chunk trigger (zoff + px > kMaxZ, 2^30 winner slots) needs more than 8 GB of winner buffer and
a 5 GB host oracle image; only the pair-list trigger (32 Mi pairs) is exercised."""
import numpy as np
import pytest

from tests import proj_edge_ref as R
from tests.test_proj_gpu import _compare, _run

pytestmark = pytest.mark.gpu


def _projector(gpu, cloud, oo):
    return gpu.Projector(cloud, depth_image_scale=oo.depth_image_scale, max_proj_scale=oo.max_proj_scale,
                         min_proj_scale=oo.min_proj_scale, min_proj_dist=oo.min_proj_dist,
                         submap_length=oo.submap_length, submap_width=oo.submap_width, submap_height=oo.submap_height,
                         choose_meter=oo.choose_meter, min_lidar_proj_dist=oo.min_lidar_proj_dist)


def _same(a, b):
    for x, y in zip(a[:5], b[:5]):
        assert np.array_equal(x.view(np.uint8), y.view(np.uint8))        # bit for bit, NaN included


def test_wide_splats(gpu, oracle):
    xyz, nrm, images, feat, okw = R.scene_wide()
    got, exp = _run(gpu, oracle, xyz, nrm, images, feat, **okw)
    assert 0.02 < exp[0].mean() < 0.98
    _compare(got, exp)


def test_single_pixel_and_unit_splats(gpu, oracle):
    for scales in ((0, 0), (1, 1)):
        xyz, nrm, images, feat, okw = R.scene_point(oracle, *scales)
        got, exp = _run(gpu, oracle, xyz, nrm, images, feat, **okw)
        assert 10 <= exp[0].sum() < exp[0].size
        _compare(got, exp)


def test_row_group_tails_and_borders(gpu, oracle):
    xyz, nrm, images, feat, okw, info = R.scene_borders(oracle)
    got, exp = _run(gpu, oracle, xyz, nrm, images, feat, **okw)
    _compare(got, exp)
    nb = info["neg_begin"]
    assert (feat[nb:nb + 20, 0] == -2.5).all() and got[0][nb:nb + 40].all()      # -0.5 / scale lands in pixel 0
    assert not got[0][nb + 40:nb + 60].any()                                     # -1 / scale is pixel -1


def test_narrow_images_and_word_edges(gpu, oracle):
    xyz, nrm, images, feat, okw = R.scene_narrow()
    got, exp = _run(gpu, oracle, xyz, nrm, images, feat, **okw)
    assert exp[0].any() and not exp[0].all()
    _compare(got, exp)


def test_duplicate_features_share_a_winner(gpu, oracle):
    xyz, nrm, images, feat, okw = R.scene_duplicates(oracle)
    got, exp = _run(gpu, oracle, xyz, nrm, images, feat, **okw)
    _compare(got, exp)
    assert got[0].all()
    idx, d = got[1].reshape(-1, 5), got[2].view(np.uint32).reshape(-1, 5)
    assert (idx == idx[:, :1]).all() and (d == d[:, :1]).all()


def test_scale_selection_boundaries(gpu, oracle):
    for lidar, part in ((0.5, "near"), (0.0, "near"), (0.5, "far")):
        xyz, nrm, images, feat, okw, names = R.scene_boundary(oracle, lidar, part)
        got, exp = _run(gpu, oracle, xyz, nrm, images, feat, **okw)
        _compare(got, exp)
        centre = dict(zip(names, got[0].reshape(len(names), -1)[:, 0]))      # the feature on each point's own pixel
        if part == "near":
            assert centre["at min_proj_dist"] and centre["just past min_proj_dist"] and not centre["behind"]
            assert bool(centre["at min_lidar_proj_dist"]) == (lidar > 0)
            assert not (centre["just below min_lidar_proj_dist"] or centre["zero"] or centre["minus zero"])
        else:
            assert centre["first zero scale"] and centre["last positive scale"] and centre["last zero scale"]
            assert not centre["first negative scale"]


def test_anisotropic_submaps_negative_coordinates(gpu, oracle):
    xyz, nrm, images, feat, okw = R.scene_anisotropic()
    oo = oracle.proj_options(**okw)
    finite, key = R.submap_keys(xyz, oo)
    cloud = gpu.Cloud(xyz, nrm, raw_lidar_frame=False)
    pj = _projector(gpu, cloud, oo)
    assert pj.num_submaps == np.unique(key[finite], axis=0).shape[0]
    pj.close()
    cloud.close()
    got, exp = _run(gpu, oracle, xyz, nrm, images, feat, **okw)
    assert 0.02 < exp[0].mean() < 0.98
    _compare(got, exp)


def test_chunked_batch(gpu, oracle):
    xyz, nrm, images, feat, okw = R.scene_chunked()
    oo = oracle.proj_options(**okw)
    coeffs = oracle.proj_scale_coeffs(oo, images[0]["params"][0], images[0]["params"][1])
    exp = oracle.proj_images(xyz, nrm, oo, coeffs, images, feat)
    assert 0.02 < exp[0].mean() < 0.98
    cloud = gpu.Cloud(xyz, nrm, raw_lidar_frame=False)
    pj = _projector(gpu, cloud, oo)
    per_chunk = (32 << 20) // pj.num_submaps
    assert per_chunk < len(images) <= 2 * per_chunk                     # exactly two trips through the chunk loop
    got = pj.set_new_images(images, feat)
    assert pj.last_pairs == exp[5]                                      # accumulated over both chunks
    _compare(got, exp)
    pj.close()
    one = _projector(gpu, cloud, oo)                                    # fresh handle, one image per call
    pairs = 0
    parts = [[] for _ in range(5)]
    for im in images:
        b, e = im["feat_begin"], im["feat_end"]
        r = one.set_new_images([dict(im, feat_begin=0, feat_end=e - b)], feat[b:e])
        pairs += one.last_pairs
        for k in range(5):
            parts[k].append(r[k])
    _same(got, [np.concatenate(p) for p in parts])
    assert pairs == exp[5]
    one.close()
    cloud.close()


def test_feature_grid_stride(gpu, oracle):
    xyz, nrm, images, feat, okw = R.scene_feature_stride()
    assert images[0]["feat_end"] - images[0]["feat_begin"] > 1024 * 256 and images[1]["feat_end"] - images[1]["feat_begin"] == 10
    got, exp = _run(gpu, oracle, xyz, nrm, images, feat, **okw)
    tail = slice(1024 * 256, images[0]["feat_end"])                     # the features only the stride step reaches
    assert exp[0][tail].any() and not exp[0][tail].all()
    _compare(got, exp)


def test_handle_reuse_shrinking_and_growing(gpu, oracle):
    xyz, nrm, images, feat, okw = R.scene_wide()
    small, sfeat = R.scene_small_images(images)
    oo = oracle.proj_options(**okw)
    coeffs = oracle.proj_scale_coeffs(oo, images[0]["params"][0], images[0]["params"][1])
    cloud = gpu.Cloud(xyz, nrm, raw_lidar_frame=False)
    batches = [(images, feat), (small, sfeat), (images, feat)]
    fresh = []
    for ims, f in batches[:2]:
        pj = _projector(gpu, cloud, oo)
        fresh.append(pj.set_new_images(ims, f))
        _compare(fresh[-1], oracle.proj_images(xyz, nrm, oo, coeffs, ims, f))
        pj.close()
    assert fresh[1][0].any()
    pj = _projector(gpu, cloud, oo)
    for (ims, f), want in zip(batches, fresh + fresh[:1]):
        _same(pj.set_new_images(ims, f), want)                          # grow-only scratch, stale bitmap / winner slots
    pj.close()
    cloud.close()


def test_featureless_batch(gpu, oracle):
    """Features that are NaN, +-inf or beyond int's range are not feature pixels and disturb nothing beside them.
    last_pairs counts the pairs of chunks that had at least one feature (include/pcdhip.h): a batch in which no
    image has a feature is not culled, because nobody would read the result, and reports 0."""
    xyz, nrm, images, feat, okw, _ = R.scene_borders(oracle)
    bad = [[np.nan, 100.0], [100.0, np.nan], [np.inf, 100.0], [-np.inf, 100.0], [1e300, 100.0], [-1e300, 100.0],
           [100.0, 1e300], [100.0, -1e300], [np.inf, -np.inf], [np.nan, np.nan], [1.1e10, 100.0], [100.0, -1.1e10]]
    rows = np.arange(5, 5 + 7 * len(bad), 7)
    f2 = feat.copy()
    f2[rows] = bad
    base, _ = _run(gpu, oracle, xyz, nrm, images, feat, **okw)
    got, exp = _run(gpu, oracle, xyz, nrm, images, f2, **okw)
    _compare(got, exp)
    assert not got[0][rows].any() and (got[1][rows] == 0xFFFFFFFF).all() and not got[4][rows].any()
    keep = np.ones(feat.shape[0], bool)
    keep[rows] = False
    _same([a[keep] for a in got], [a[keep] for a in base])
    # no image has a feature
    oo = oracle.proj_options(**okw)
    cloud = gpu.Cloud(xyz, nrm, raw_lidar_frame=False)
    pj = _projector(gpu, cloud, oo)
    pj.set_new_images(images, feat)
    assert pj.last_pairs > 0
    empty = [dict(images[0], feat_begin=0, feat_end=0), dict(images[0], feat_begin=3, feat_end=3)]
    out = pj.set_new_images(empty, feat[:10])
    assert pj.last_pairs == 0
    assert not out[0].any() and (out[1] == 0xFFFFFFFF).all() and not out[2].any() and not out[3].any()
    out = pj.set_new_images(empty[:1], np.zeros((0, 2)))
    assert pj.last_pairs == 0 and out[0].size == 0
    _same(pj.set_new_images(images, feat), base)                        # and the handle is none the worse for it
    pj.close()
    cloud.close()
