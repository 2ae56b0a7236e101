"""The co-visibility structure of the point elimination, restated from its contract (include/pcdhip.h,
pcd_ba_schur_structure_lists) in numpy: dictionaries of lists and sorted (a, b) tuples, no device, no library.

e is the image-major position of an observation: observations in ascending image, ties in the caller's order.  e is
*eliminated* when its image has a slot (a variable pose) and its point is not constant.  A point's list holds its
eliminated observations in ascending e.  Block (i, j), i <= j, holds every (a, b) with a an eliminated observation of
slot i and b an entry of the same point's list in slot j, ascending (a, b).  An (a, b) tuple is kept as the integer
a << 32 | b, whose order is the tuple's."""
from collections import defaultdict

import numpy as np

LISTS = ("slot_image", "obs_pos", "blk_start", "ent_a", "ent_b", "pair_ij", "row_start", "row_blk", "row_col")


def _mask(scene, key, n):
    m = scene.get(key)
    return np.zeros(n, bool) if m is None else np.asarray(m).astype(bool)


def structure(scene):
    """scene: obs_image, obs_point, poses [I], points [P] and the optional masks image_const_pose / point_const.
    Returns a dict of the nine lists (dtypes as the library's) and num_slots, num_pairs, num_entries, image_slot."""
    obs_image = np.asarray(scene["obs_image"], np.int64)
    obs_point = np.asarray(scene["obs_point"], np.int64)
    I, P, O = len(scene["poses"]), len(scene["points"]), len(obs_image)
    cpose, cpt = _mask(scene, "image_const_pose", I), _mask(scene, "point_const", P)
    # slots: the rank of an image among the variable-pose images
    slot_image = np.flatnonzero(~cpose)
    ns = len(slot_image)
    image_slot = np.full(I, -1, np.int64)
    image_slot[slot_image] = np.arange(ns)
    # positions
    order = np.argsort(obs_image, kind="stable")          # order[e] = observation at position e
    obs_pos = np.empty(O, np.int64)
    obs_pos[order] = np.arange(O)
    e_slot = image_slot[obs_image[order]]
    e_point = obs_point[order]
    eliminated = (e_slot >= 0) & ~cpt[e_point]
    # a point's list: its eliminated observations, ascending e
    lists = defaultdict(list)
    for e in np.flatnonzero(eliminated):
        lists[int(e_point[e])].append(int(e))
    # blocks: (i, j) -> the (a, b) tuples, gathered point by point
    blocks = defaultdict(list)
    for members in lists.values():
        sl = e_slot[members]
        m = np.asarray(members, np.uint64)
        seen = np.unique(sl)                              # the slots that see the point, ascending
        for x, i in enumerate(seen):
            a = m[sl == i]
            for j in seen[x:]:
                b = m[sl == j]
                blocks[(int(i), int(j))].append(((a[:, None] << np.uint64(32)) | b[None, :]).ravel())
    pairs = sorted(k for k in blocks if k[0] < k[1])
    keys = [(s, s) for s in range(ns)] + pairs            # the diagonal blocks (empty ones too), then the pair blocks
    ents = [np.sort(np.concatenate(blocks[k])) if k in blocks else np.zeros(0, np.uint64) for k in keys]
    blk_start = np.concatenate([[0], np.cumsum([len(x) for x in ents])])
    ent = np.concatenate(ents) if ents else np.zeros(0, np.uint64)
    # row lists: per slot the transposed (k, s) blocks in ascending k, the diagonal, the (s, j) blocks in ascending j
    row_start, row_blk, row_col = [0], [], []
    index = {k: ns + q for q, k in enumerate(pairs)}
    by_i, by_j = defaultdict(list), defaultdict(list)
    for (i, j) in pairs:
        by_i[i].append(j)
        by_j[j].append(i)
    for s in range(ns):
        for k in sorted(by_j[s]):
            row_blk.append(index[(k, s)]); row_col.append(k << 1 | 1)
        row_blk.append(s); row_col.append(s << 1)
        for j in sorted(by_i[s]):
            row_blk.append(index[(s, j)]); row_col.append(j << 1)
        row_start.append(len(row_blk))
    u32 = lambda x: np.asarray(x, np.int64).astype(np.uint32).reshape(-1)
    return dict(slot_image=slot_image.astype(np.int32), obs_pos=u32(obs_pos), blk_start=u32(blk_start),
                ent_a=(ent >> np.uint64(32)).astype(np.uint32), ent_b=(ent & np.uint64(0xFFFFFFFF)).astype(np.uint32),
                pair_ij=u32(pairs), row_start=u32(row_start), row_blk=u32(row_blk), row_col=u32(row_col),
                num_slots=ns, num_pairs=len(pairs), num_entries=len(ent), image_slot=image_slot.astype(np.int32))


def assert_equal(got, want, what=""):
    """every list and count of two structure dicts, exactly"""
    for k in ("num_slots", "num_pairs", "num_entries"):
        assert int(got[k]) == int(want[k]), (what, k, got[k], want[k])
    for k in LISTS:
        assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]), (what, k)
