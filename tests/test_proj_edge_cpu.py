"""CPU half of the depth-projection edge suite: the census conditions that prove each scene of
tests/test_proj_edge_gpu.py reaches the kernel path it is named for, and a second, independent reference
(tests/proj_edge_ref.winners_numpy, brute force in numpy) against the C oracle on every small scene."""
import numpy as np
import pytest

from tests import proj_edge_ref as R


def _opts(oracle, images, okw):
    oo = oracle.proj_options(**okw)
    return oo, oracle.proj_scale_coeffs(oo, images[0]["params"][0], images[0]["params"][1])


def _census_all(oracle, xyz, images, okw):
    oo, c4 = _opts(oracle, images, okw)
    return [R.census(xyz, im, oo, c4) for im in images], oo, c4


def _oracle(oracle, xyz, nrm, images, feat, okw):
    oo, c4 = _opts(oracle, images, okw)
    return oracle.proj_images(xyz, nrm, oo, c4, images, feat)


def _cat(cs, name, mask="live"):
    return np.concatenate([c[name][c[mask]] for c in cs])


def test_proj_options_axes(oracle):
    oo = oracle.proj_options(submap=2.0)
    assert (oo.submap_length, oo.submap_width, oo.submap_height) == (2.0, 2.0, 2.0)
    oo = oracle.proj_options(submap=2.0, submap_length=0.5, submap_height=4.0)
    assert (oo.submap_length, oo.submap_width, oo.submap_height) == (0.5, 2.0, 4.0)


def test_wide_scene_census(oracle):
    xyz, nrm, images, feat, okw = R.scene_wide()
    assert okw == dict(max_proj_scale=40) and len(images) == 2 and xyz.shape[0] == 30000
    cs, oo, c4 = _census_all(oracle, xyz, images, okw)
    span, rows = _cat(cs, "span"), _cat(cs, "rows")
    print("spans 1..4:", [int((span == k).sum()) for k in (1, 2, 3, 4)],
          "rows%4:", [int((rows % 4 == k).sum()) for k in range(4)])
    assert (span == 3).sum() >= 100 and (span == 4).sum() >= 100
    for k in range(4):
        assert (rows % 4 == k).sum() >= 100
    # scale branches: by depth alone (window), whatever the submap cull says; a negative scale lies past
    # choose_meter + 1 / |a|, where only submaps straddling the far plane survive the cull
    branch = np.concatenate([c["branch"][c["finite"]] for c in cs])
    live_near = sum(int((c["live"] & (c["branch"] == R.NEAR)).sum()) for c in cs)
    print("near (live):", live_near, "negative:", int((branch == R.NEGATIVE).sum()))
    assert live_near >= 100 and (branch == R.NEGATIVE).sum() >= 100
    exp = _oracle(oracle, xyz, nrm, images, feat, okw)
    print("found:", exp[0].mean())
    assert 0.02 < exp[0].mean() < 0.98


def test_point_scene_census(oracle):
    xyz, nrm, images, feat, okw = R.scene_point(oracle)
    assert okw == dict(max_proj_scale=0, min_proj_scale=0)
    cs, oo, c4 = _census_all(oracle, xyz, images, okw)
    assert (_cat(cs, "span") == 1).all() and (_cat(cs, "rows") == 1).all() and _cat(cs, "span").size > 1000
    exp = _oracle(oracle, xyz, nrm, images, feat, okw)
    assert 10 <= exp[0].sum() < exp[0].size
    # scales 1/1: every unclipped splat is 3 x 3
    xyz, nrm, images, feat, okw = R.scene_point(oracle, 1, 1)
    cs, oo, c4 = _census_all(oracle, xyz, images, okw)
    assert _cat(cs, "sx").max() == 1 and _cat(cs, "sy").max() == 1 and (_cat(cs, "rows") == 3).sum() > 1000


def test_borders_scene_census(oracle):
    xyz, nrm, images, feat, okw, info = R.scene_borders(oracle)
    (c,), oo, c4 = _census_all(oracle, xyz, images, okw)
    L = c["live"]
    clipped = dict(left=L & (c["u0"] - c["sx"] < 0), right=L & (c["u0"] + c["sx"] > c["w"] - 1),
                   top=L & (c["v0"] - c["sy"] < 0), bottom=L & (c["v0"] + c["sy"] > c["h"] - 1))
    for name, m in clipped.items():
        assert m.sum() >= 50, name
    for k in range(4):
        assert (c["rows"][L] % 4 == k).sum() >= 50
    assert info["n_left"] == 20 and info["n_top"] == 20
    exp = _oracle(oracle, xyz, nrm, images, feat, okw)
    ok, u, v = R.feature_pixels(feat, oo.depth_image_scale, c["w"], c["h"])
    f = exp[0].astype(bool)
    for name, m in dict(row0=v == 0, rowH=v == c["h"] - 1, col0=u == 0, colW=u == c["w"] - 1).items():
        assert (f & ok & m).sum() >= 5, name
    nb = info["neg_begin"]
    assert (feat[nb:nb + 20, 0] < 0).all() and f[nb:nb + 40].all()       # x (then y) = -0.5 / scale: pixel 0, found
    assert not f[nb + 40:nb + 60].any()                                  # -1 / scale: pixel -1


def test_narrow_scene_census(oracle):
    xyz, nrm, images, feat, okw = R.scene_narrow()
    cs, oo, c4 = _census_all(oracle, xyz, images, okw)
    assert tuple(c["w"] for c in cs) == R.NARROW_WIDTHS and all(c["h"] == 96 for c in cs)
    exp = _oracle(oracle, xyz, nrm, images, feat, okw)
    for c, im in zip(cs, images):
        b, e = im["feat_begin"], im["feat_end"]
        ok, u, v = R.feature_pixels(feat[b:e], oo.depth_image_scale, c["w"], c["h"])
        assert ok.all() and e - b == c["w"] * 96
        f = exp[0][b:e].astype(bool)
        assert (f & (u == c["w"] - 1)).any() and (f & (u == 0)).any(), c["w"]
        assert 0 < f.sum()
    c = cs[-1]                                                           # the 64-wide image: splats on the word edges
    L = c["live"]
    for name, m in dict(starts_32=c["ulo"] == 32, ends_31=c["uhi"] == 31, ends_63=(c["uhi"] == 63) & (c["u0"] + c["sx"] == 63),
                        starts_31=c["ulo"] == 31, two_words=c["span"] == 2).items():
        assert (L & m).sum() >= 1, name
    assert (exp[0] == 0).any()


def _boundary(oracle, lidar, part):
    xyz, nrm, images, feat, okw, names = R.scene_boundary(oracle, lidar, part)
    (c,), oo, c4 = _census_all(oracle, xyz, images, okw)
    assert c4.tolist() == [-0.5, 21.0, -0.5, 22.0]                       # exact; b_y with the unscaled min_proj_scale
    assert np.array_equal(c["zc"], xyz[:, 2])                            # identity pose: zc == z bit for bit
    assert c["in_frustum"].all()                                         # every class reaches the splat kernel
    got = {n: (R.BRANCH[int(c["branch"][k])], int(c["sx"][k]), int(c["sy"][k]), bool(c["live"][k]))
           for k, n in enumerate(names)}
    return got, {n: float(xyz[k, 2]) for k, n in enumerate(names)}


def test_boundary_scene_census(oracle):
    """every boundary class is classified as the reference's if-chain (pcd_projection.cc:399-419) reads"""
    for lidar in (0.5, 0.0):
        got, z = _boundary(oracle, lidar, "near")
        assert got["at min_proj_dist"] == ("near", 20, 20, True) and z["at min_proj_dist"] == 2.0   # <=: the near scale
        assert got["just past min_proj_dist"] == ("far", 19, 20, True)
        assert z["just past min_proj_dist"] == float(np.nextafter(np.float32(2), np.float32(3)))
        assert got["behind"][0] == "behind" and not got["behind"][3] and z["behind"] < 0
        if lidar > 0:
            assert got["at min_lidar_proj_dist"] == ("near", 20, 20, True) and z["at min_lidar_proj_dist"] == 0.5
            assert got["just below min_lidar_proj_dist"] == ("too close", -1, -1, False)
            assert got["zero"][0] == "too close" and got["minus zero"][0] == "too close"
        else:
            # depth 0 passes 0 <= 0 into the near scale; its pixel is 0/0 or x/0, never finite, never splatted
            assert got["at min_lidar_proj_dist"] == ("near", 20, 20, False) and got["zero"] == ("near", 20, 20, False)
            assert got["minus zero"] == ("near", 20, 20, False)
            assert got["just below min_lidar_proj_dist"][0] == "behind"
    got, z = _boundary(oracle, 0.5, "far")
    assert got["last positive scale"] == ("far", 1, 2, True) and z["last positive scale"] == 40.0
    assert got["first zero scale"] == ("far", 0, 1, True) and z["first zero scale"] > 40.0
    assert got["last zero scale"] == ("far", 0, 0, True) and z["last zero scale"] < 44.0
    assert got["first negative scale"] == ("negative", -1, 0, False) and z["first negative scale"] == 44.0
    sweep = [v for n, v in got.items() if n.startswith("sweep")]
    assert sum(v[0] == "negative" for v in sweep) >= 10 and sum(v[3] for v in sweep) >= 10
    assert {v[1:3] for v in sweep if v[3]} >= {(0, 1), (0, 0)}


def test_anisotropic_scene_census(oracle):
    xyz, nrm, images, feat, okw = R.scene_anisotropic()
    oo, c4 = _opts(oracle, images, okw)
    finite, key = R.submap_keys(xyz, oo)
    assert (~finite).sum() == 45 and np.isnan(xyz).any() and np.isposinf(xyz).any() and np.isneginf(xyz).any()
    for a in range(3):
        assert key[finite, a].min() < -3 and key[finite, a].max() > 3
    # the three axes are told apart: pairing any two sizes the other way changes the key set
    n = np.unique(key[finite], axis=0).shape[0]
    for other in (dict(submap_length=0.7, submap_height=1.3, submap_width=2.1),
                  dict(submap_length=2.1, submap_height=0.7, submap_width=1.3)):
        _, k2 = R.submap_keys(xyz, oracle.proj_options(**dict(okw, **other)))
        assert not np.array_equal(k2[finite], key[finite])
    assert n > 1000
    exp = _oracle(oracle, xyz, nrm, images, feat, okw)
    assert 0.02 < exp[0].mean() < 0.98


def _small_scene(oracle, name):
    return {"wide": lambda: R.scene_wide(), "point": lambda: R.scene_point(oracle),
            "unit": lambda: R.scene_point(oracle, 1, 1), "borders": lambda: R.scene_borders(oracle)[:5],
            "narrow": lambda: R.scene_narrow(), "duplicates": lambda: R.scene_duplicates(oracle),
            "boundary": lambda: R.scene_boundary(oracle, 0.5)[:5], "boundary0": lambda: R.scene_boundary(oracle, 0.0)[:5],
            "boundary_far": lambda: R.scene_boundary(oracle, 0.5, "far")[:5],
            "anisotropic": lambda: R.scene_anisotropic()}[name]()


@pytest.mark.parametrize("name", ["wide", "point", "unit", "borders", "narrow", "duplicates", "boundary", "boundary0",
                                  "boundary_far", "anisotropic"])
def test_numpy_winners_equal_oracle(oracle, name):
    """Two references written apart (plain C walk in submap order with strict 'nearer replaces'; numpy brute force
    taking the minimum of (norm bits, rank)) agree on found, index, the dist bits and the surviving pairs.
    No disagreement was found on any scene, so nothing had to be settled from lidar/pcd_projection.cc."""
    xyz, nrm, images, feat, okw = _small_scene(oracle, name)
    assert xyz.shape[0] * max(im["feat_end"] - im["feat_begin"] for im in images) <= 30_000 * 2_000   # brute force stays small
    oo, c4 = _opts(oracle, images, okw)
    exp = oracle.proj_images(xyz, nrm, oo, c4, images, feat)
    found, index, dist, pairs = R.winners_numpy(xyz, images, feat, oo, c4)
    assert np.array_equal(found, exp[0])
    assert np.array_equal(index, exp[1])
    assert np.array_equal(dist.view(np.uint32), exp[2].view(np.uint32))
    assert pairs == exp[5]
    assert found.any()


def test_duplicate_scene_groups(oracle):
    xyz, nrm, images, feat, okw = R.scene_duplicates(oracle)
    exp = _oracle(oracle, xyz, nrm, images, feat, okw)
    assert exp[0].all()
    idx, d = exp[1].reshape(-1, 5), exp[2].view(np.uint32).reshape(-1, 5)
    assert (idx == idx[:, :1]).all() and (d == d[:, :1]).all() and np.unique(idx[:, 0]).size > 10


def test_oracle_rejects_unrepresentable_feature_pixels(oracle):
    """(xy * scale).cast<int>() is undefined outside int's range; the oracle's documented choice, like the kernel's:
    not a feature pixel.  The neighbours are untouched."""
    xyz, nrm, images, feat, okw, _ = R.scene_borders(oracle)
    base = _oracle(oracle, xyz, nrm, images, feat, okw)
    bad = [[np.nan, 100.0], [100.0, np.nan], [np.inf, 100.0], [-np.inf, 100.0], [1e300, 100.0], [-1e300, 100.0],
           [100.0, 1e300], [100.0, -1e300], [np.inf, -np.inf], [1.1e10, 100.0], [100.0, -1.1e10]]
    f2 = feat.copy()
    rows = np.arange(5, 5 + 7 * len(bad), 7)
    f2[rows] = bad
    got = _oracle(oracle, xyz, nrm, images, f2, okw)
    keep = np.ones(feat.shape[0], bool)
    keep[rows] = False
    assert not got[0][rows].any() and (got[1][rows] == 0xFFFFFFFF).all()
    assert np.array_equal(got[0][keep], base[0][keep]) and np.array_equal(got[1][keep], base[1][keep])
