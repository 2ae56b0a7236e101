"""Observations and points added to a live BA handle (pcd_ba_add_observations_device), restated in numpy.

The contract is equality with a fresh handle built from the concatenated description (fresh_args_after_add).  The device
derives the two CSRs of that handle from the old ones and the stably sorted new rows (merge_csr: the rule of DESIGN
4.3e); pcd_ba_create derives them with a stable counting sort of the concatenated keys (build_csr).  tests/
test_ba_add_cpu.py shows that the two agree; tests/test_ba_add_gpu.py compares the handles."""
import numpy as np


def build_csr(key, nkeys):
    """pcd_ba_create's stable counting sort of element ids by key -> (start [nkeys + 1], list [n])"""
    key = np.asarray(key, np.int64)
    start = np.zeros(nkeys + 1, np.int64)
    for k in key:
        start[k + 1] += 1
    start = np.cumsum(start)
    cur = start[:-1].copy()
    lst = np.zeros(len(key), np.int64)
    for i, k in enumerate(key):
        lst[cur[k]] = i
        cur[k] += 1
    return start.astype(np.uint32), lst.astype(np.uint32)


def merge_csr(old_start, old_list, old_key_of, new_key, nkeys_new):
    """The CSR of the concatenated keys from the CSR of the old ones (nkeys_old = len(old_start) - 1 keys, O entries;
    old_key_of[o] = key of old element o) and the new elements' keys, the way the device does it:
      the new rows sorted stably by key; add[k] = new rows with a key below k (a lower bound on the sorted keys)
      start'[k] = start[k] + add[k], the old bound of a new key being O
      old entry e of key k          -> e + add[k]
      sorted new row of rank r, key k -> start'[k] + oldlen[k] + (r - add[k]), holding O + row"""
    old_start = np.asarray(old_start, np.int64)
    old_list = np.asarray(old_list, np.int64)
    new_key = np.asarray(new_key, np.int64)
    nold, O, A = len(old_start) - 1, len(old_list), len(new_key)
    rows = np.argsort(new_key, kind="stable")
    skey = new_key[rows]
    add = np.searchsorted(skey, np.arange(nkeys_new + 1), side="left")
    bound = np.concatenate([old_start, np.full(nkeys_new - nold, O, np.int64)])
    start = bound + add
    oldlen = np.diff(bound)
    lst = np.full(O + A, -1, np.int64)
    for e in range(O):
        lst[e + add[old_key_of[old_list[e]]]] = old_list[e]
    for r in range(A):
        k = skey[r]
        lst[start[k] + oldlen[k] + (r - add[k])] = O + rows[r]
    assert (lst >= 0).all()
    return start.astype(np.uint32), lst.astype(np.uint32)


def fresh_args_after_add(scene, current_points, new_obs, new_points=None):
    """(the description of the fresh handle, the expected info counts): the points currently on the device followed by
    the new ones, the scene's rows followed by the new rows (a dict of obs_image, obs_point, obs_xy) in the order given,
    point_const (if the scene has one) extended by zeros; everything else as it is"""
    new_points = np.zeros((0, 3)) if new_points is None else np.asarray(new_points, np.float64).reshape(-1, 3)
    kw = dict(scene)
    kw["points"] = np.concatenate([np.asarray(current_points, np.float64).reshape(-1, 3), new_points])
    kw["obs_image"] = np.concatenate([scene["obs_image"], new_obs["obs_image"]]).astype(np.int32)
    kw["obs_point"] = np.concatenate([scene["obs_point"], new_obs["obs_point"]]).astype(np.int32)
    kw["obs_xy"] = np.concatenate([np.asarray(scene["obs_xy"], np.float64).reshape(-1, 2),
                                   np.asarray(new_obs["obs_xy"], np.float64).reshape(-1, 2)])
    if scene.get("point_const") is not None:
        kw["point_const"] = np.concatenate([scene["point_const"], np.zeros(len(new_points), np.uint8)]).astype(np.uint8)
    cpose = scene.get("image_const_pose")
    rows = len(kw["obs_image"]) if cpose is None else int((np.asarray(cpose)[kw["obs_image"]] == 0).sum())
    info = dict(num_obs=len(kw["obs_image"]), num_obs_added=len(new_obs["obs_image"]), num_points=len(kw["points"]),
                num_points_added=len(new_points), num_pose_rows=rows)
    return kw, info


def split(scene, obs_frac, n_new_points, seed, shuffle=False):
    """(base, additions): the scene without a random share obs_frac of its observations and without its last
    n_new_points points, whose rows and LiDAR terms go with them -- the trailing ids, so base's points keep theirs and the
    held-out points get P .. P + n - 1 again when they are added.  additions = dict(obs_image, obs_point, obs_xy,
    new_points): the held-out rows in the scene's order, or shuffled."""
    rng = np.random.default_rng(seed)
    O, P = len(scene["obs_point"]), len(scene["points"])
    Pb = P - n_new_points
    out = (rng.random(O) < obs_frac) | (np.asarray(scene["obs_point"]) >= Pb)
    base = dict(scene)
    base["points"] = np.asarray(scene["points"])[:Pb]
    for k in ("obs_image", "obs_point", "obs_xy"):
        base[k] = np.asarray(scene[k])[~out]
    if scene.get("point_const") is not None:
        base["point_const"] = np.asarray(scene["point_const"])[:Pb]
    if scene.get("lidar_point") is not None:
        lkeep = np.asarray(scene["lidar_point"]) < Pb
        for k in ("lidar_point", "lidar_abcd", "lidar_weight"):
            base[k] = np.asarray(scene[k])[lkeep]
    rows = np.flatnonzero(out)
    if shuffle:
        rows = rng.permutation(rows)
    add = dict(obs_image=np.asarray(scene["obs_image"])[rows], obs_point=np.asarray(scene["obs_point"])[rows],
               obs_xy=np.asarray(scene["obs_xy"]).reshape(-1, 2)[rows], new_points=np.asarray(scene["points"])[Pb:])
    return base, add
