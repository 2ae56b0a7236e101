"""The write-once outputs of the BA Jacobian pass at the edges of their stores.  W of k_ba_images<4, true> leaves under
a cache policy (csrc/ba.hip StorePolicy: non-temporal) on its contiguous path (wave_store_rows<18>: wide masked stores
of a wavefront's rows) and on its scattered path (lane_store_row<18>); H_pt / g_pt of k_ba_points<4, true, true>, whose
stores were measured under the same policy and stay plain, are held to the same checks.

A policy changes no value and no address, so what can go wrong is a wide store that covers a row too many or too few at
the end of a wavefront's rows.  The outputs are therefore device buffers with a band of sentinel rows (a NaN bit pattern)
in front and behind: every sentinel must be untouched, every row inside written (the scene gives finite values only),
and the values are held to the oracle through tests/ba_edge_ref.py's helpers at the project's 1e-9.

Scene: one shared OPENCV camera, three images, 150 points.  Image 0 has 70 observations (a full wavefront and one of 6
rows) and a constant pose: its W rows are zero and must still be written.  Image 1 has 300 (two 256-row iterations, the
second with a wavefront of 44 rows and two idle ones), image 2 has one.  One constant point, two points with a second
LiDAR term.  Image-major caller order takes the contiguous path, a seeded shuffle the scattered one; the contiguous case
is repeated with O cut to 327 and 326, so that the last wavefront of image 1 holds exactly 1 row and exactly 64."""
import numpy as np
import pytest

from tests import ba_edge_ref as er
from tests import ba_schur_ref as sr

pytestmark = pytest.mark.gpu
COUNTS = (70, 300, 1)
P = 150
GUARD = 8                                   # sentinel rows on either side (a multiple of 16 bytes for every row size)
SENTINEL = 0x7FF8DEADBEEF0001               # a quiet NaN no arithmetic produces
ROW = dict(W=18, H_pt=9, g_pt=3)


def _scene(oracle):
    rng = np.random.default_rng(9300)
    I = len(COUNTS)
    poses = np.stack([er._generic_pose(rng) for _ in range(I)])
    points = np.stack([rng.uniform(-2, 2, P), rng.uniform(-1.5, 1.5, P), rng.uniform(5, 12, P)], axis=1)
    obs_image = np.repeat(np.arange(I), COUNTS).astype(np.int32)
    # image 0: points 0..69; image 1: every point twice; image 2: one point
    obs_point = np.concatenate([np.arange(70), np.arange(300) % P, [75]]).astype(np.int32)
    lp = np.concatenate([np.flatnonzero(np.arange(P) % 3 != 1), [20, 99]]).astype(np.int32)   # 20 and 99: two terms each
    nrm = rng.normal(size=(len(lp), 3))
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    near = points[lp] + rng.normal(0, 0.05, (len(lp), 3))
    pc = np.zeros(P, np.uint8); pc[33] = 1
    s = dict(cam_model=np.array([4], np.int32), cam_params_list=[er.cam_params(4)], poses=poses,
             image_camera=np.zeros(I, np.int32), points=points, obs_image=obs_image, obs_point=obs_point,
             lidar_point=lp, lidar_abcd=np.concatenate([nrm, -np.sum(nrm * near, 1, keepdims=True)], axis=1),
             lidar_weight=np.where(rng.random(len(lp)) < 0.35, 1000.0, 100.0),
             image_const_pose=np.array([1, 0, 0], np.uint8), point_const=pc)
    return sr.reproject(oracle, s, rng, noise=2.0)


_CASES = {}


def _case(oracle, name):
    """(keyword arguments, oracle normal equations) of a case, computed once"""
    if "base" not in _CASES:
        _CASES["base"] = _scene(oracle)
    if name not in _CASES:
        kw = dict(_CASES["base"])
        O = len(kw["obs_image"])
        if name == "shuffled":
            sel = np.random.default_rng(9301).permutation(O)
        elif name.startswith("cut"):
            sel = np.arange(int(name[3:]))
        else:
            sel = np.arange(O)
        for k in ("obs_image", "obs_point", "obs_xy"):
            kw[k] = kw[k][sel]
        _CASES[name] = (kw, oracle.BA(**kw).normal_equations(want_w=True))
    return _CASES[name]


def _guarded(torch, rows, width):
    buf = torch.full(((rows + 2 * GUARD) * width,), SENTINEL, dtype=torch.int64, device="cuda:0").view(torch.float64)
    return buf, buf[GUARD * width:(GUARD + rows) * width]


@pytest.mark.parametrize("name", ["image_major", "shuffled", "cut327", "cut326"])
def test_guard_bands_and_values(gpu, oracle, name):
    import torch
    kw, (cost, Himg, gimg, Hpt, gpt, W) = _case(oracle, name)
    O, I = len(kw["obs_image"]), len(COUNTS)
    if name != "shuffled":       # what the contiguous path needs: rows of an image adjacent in the caller's order
        assert np.all(np.diff(kw["obs_image"]) >= 0)
    if name.startswith("cut"):   # rows of image 1's last wavefront
        assert (O - 70) % 256 % 64 == {"cut327": 1, "cut326": 0}[name]
    ba = gpu.BA(**kw)
    rows = dict(W=O, H_pt=P, g_pt=P)
    full, out = {}, {}
    for k in ROW:
        full[k], out[k] = _guarded(torch, rows[k], ROW[k])
    f64 = dict(dtype=torch.float64, device="cuda:0")
    out.update(cost=torch.zeros(1, **f64), H_img=torch.zeros(I * 36, **f64), g_img=torch.zeros(I * 6, **f64))
    ba.evaluate_device(out)
    torch.cuda.synchronize()
    got = {k: v.cpu().numpy() for k, v in out.items()}
    for k in ROW:
        bits = full[k].view(torch.int64).cpu().numpy()
        n = GUARD * ROW[k]
        assert (bits[:n] == SENTINEL).all(), "%s: sentinel rows in front overwritten" % k
        assert (bits[-n:] == SENTINEL).all(), "%s: sentinel rows behind overwritten" % k
        left = np.flatnonzero(np.isnan(got[k]))
        assert left.size == 0, "%s: rows not written: %r" % (k, np.unique(left // ROW[k])[:8])
    ba.close()
    assert abs(got["cost"][0] - cost) <= er.REL * abs(cost)
    er.block_close(got["H_img"].reshape(I, 6, 6), Himg, "H_img")
    er.col_close(got["g_img"].reshape(I, 6), gimg, "g_img")
    er.block_close(got["H_pt"].reshape(P, 3, 3), Hpt, "H_pt")
    er.col_close(got["g_pt"].reshape(P, 3), gpt, "g_pt")
    Wg = got["W"].reshape(O, 6, 3)
    er.block_close(Wg, W, "W")
    zero = (kw["obs_image"] == 0) | (kw["obs_point"] == 33)            # constant pose, constant point
    assert zero.sum() >= 70 and not Wg[zero].any() and np.abs(Wg[~zero]).max(axis=(1, 2)).min() > 0
    assert not got["H_pt"].reshape(P, 9)[33].any() and not got["H_img"].reshape(I, 36)[0].any()
