"""GPU parity of guided SIFT matching (pcd_sift_match_guided[_batch], the SiftMatchGPU-shaped adapter) against the numpy
restatement of feature/sift.cc:1092-1162 (tests/sift_guided_ref.py).  Bar: identical match lists."""
import os
import subprocess

import numpy as np
import pytest

from tests import sift_edge_ref as er
from tests import sift_guided_ref as ref
from tests.test_sift_edge_gpu import _device as device_match
from tests.test_sift_guided_cpu import I3, kat_case

pytestmark = pytest.mark.gpu
PKG = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "colmap-pcd_amd")


@pytest.fixture
def sift_tuning(gpu):
    def set_(nchunk=0, batch_partials=0):
        gpu.set_sift_tuning(nchunk, batch_partials)
    yield set_
    gpu.set_sift_tuning(0, 0)


def test_known_answers_through_the_abi(gpu, oracle):
    d1, k1, d2, k2 = kat_case(oracle)
    assert gpu.sift_match_guided(d1, k1, d2, k2, H=I3).tolist() == [[0, 1], [1, 0]]
    k1[0, 0] = 100
    assert gpu.sift_match_guided(d1, k1, d2, k2, H=I3).tolist() == [[1, 0]]
    e_d, e_k = np.zeros((0, 128), np.uint8), np.zeros((0, 2), np.float32)
    for a, ka, b, kb in ((e_d, e_k, d2, k2), (d1, k1, e_d, e_k), (e_d, e_k, e_d, e_k)):
        assert len(gpu.sift_match_guided(a, ka, b, kb, H=I3)) == 0


def test_adapter_sequence_of_the_reference(gpu, oracle, tmp_path):
    subprocess.check_call(["make", "-s", "-C", PKG, "shim/test_sift_guided"])
    f = tmp_path / "desc.bin"
    f.write_bytes(oracle.sift_random_descriptors(2).tobytes())
    r = subprocess.run([os.path.join(PKG, "shim", "test_sift_guided"), str(f)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "ALL OK" in r.stdout, r.stdout + r.stderr


def _scene(n1, n2, seed):
    """SIFT-like descriptors with planted correspondences between geometrically consistent keypoints, plus geometric
    outliers whose descriptors copy a true match (the filter, not the descriptor, must decide), duplicates for ties"""
    rng = np.random.default_rng(seed)
    loc1, loc2, F, H, corr = ref.two_view_scene(rng, n1, n2)
    f = rng.random((n1 + n2, 128), dtype=np.float32) ** 2
    f /= np.linalg.norm(f, axis=1, keepdims=True)
    base = np.clip(np.round(512 * f), 0, 255).astype(np.uint8)
    d1 = base[:n1].copy()
    d2 = base[n1:].copy()
    for s, t in corr:
        d2[t] = np.clip(d1[s].astype(np.int32) + rng.integers(-5, 6, 128), 0, 255).astype(np.uint8)
    if len(corr) > 8:
        for s, t in corr[:len(corr) // 4]:          # geometric outliers: another column with a closer descriptor
            o = rng.integers(0, n2)
            d2[o] = d1[s]
        d2[corr[-1, 1]] = d2[corr[-2, 1]]          # duplicated column
    return d1, loc1, d2, loc2, F, H


@pytest.mark.parametrize("n1,n2", [(1, 1), (127, 129), (128, 128), (300, 77), (1000, 1500), (17000, 260)])
@pytest.mark.parametrize("cross", [True, False])
def test_random_geometry_exact(gpu, oracle, n1, n2, cross):
    d1, l1, d2, l2, F, H = _scene(n1, n2, n1 * 31 + n2)
    dists = oracle.sift_distance_matrix(d1, d2).astype(np.int64)
    unguided = ref.match_from_dists(dists, cross_check=cross)
    differs = 0
    for Hm, Fm, th, tf in ((H, None, 16.0, 16.0), (None, F, 16.0, 4.0), (H, F, 64.0, 16.0), (None, None, 16.0, 16.0)):
        dd = dists.copy()
        if Hm is not None or Fm is not None:
            dd[ref.guided_reject(l1, l2, Hm, Fm, th, tf)] = 0
        exp = ref.match_from_dists(dd, cross_check=cross)
        got = gpu.sift_match_guided(d1, l1, d2, l2, H=Hm, F=Fm, h_max_residual=th, f_max_residual=tf, cross_check=cross)
        assert np.array_equal(got, exp), (n1, n2, cross, Hm is not None, Fm is not None, len(got), len(exp))
        differs += not np.array_equal(exp, unguided)
    assert np.array_equal(gpu.sift_match_guided(d1, l1, d2, l2, cross_check=cross), gpu.sift_match(d1, d2, cross_check=cross))
    if n1 >= 300:
        assert differs >= 2                        # the filter decides matches


def test_points_exactly_on_the_threshold(gpu, oracle):
    """H = I with integer offsets: residual 16 == threshold is kept, 17 rejected; both directions of the walk"""
    rng = np.random.default_rng(3)
    n = 200
    d1 = rng.integers(0, 80, (n, 128), dtype=np.uint8)
    d2 = np.clip(d1.astype(np.int32) + rng.integers(-2, 3, d1.shape), 0, 255).astype(np.uint8)
    l1 = rng.integers(0, 500, (n, 2)).astype(np.float32)
    off = np.where(rng.random(n) < 0.5, 4.0, np.sqrt(17.0)).astype(np.float32)
    l2 = l1.copy()
    l2[:, 0] += np.where(off == 4.0, 4.0, 1.0)
    l2[:, 1] += np.where(off == 4.0, 0.0, 4.0)     # (1, 4): residual 17
    for cross in (True, False):
        exp = ref.sift_match_guided(oracle, d1, l1, d2, l2, H=I3, h_max_residual=16.0, cross_check=cross)
        got = gpu.sift_match_guided(d1, l1, d2, l2, H=I3, h_max_residual=16.0, cross_check=cross)
        assert np.array_equal(got, exp) and 0 < len(exp) < n, (cross, len(got), len(exp))


@pytest.mark.parametrize("nchunk", [1, 2, 5])
def test_forced_chunks_with_ties(gpu, oracle, nchunk, sift_tuning):
    sift_tuning(nchunk=nchunk)
    rng = np.random.default_rng(200 + nchunk)
    n1, n2 = 700, 1900
    base = rng.integers(0, 90, (6, 128), dtype=np.uint8)
    d1 = base[rng.integers(0, 6, n1)].copy()
    d2 = base[rng.integers(0, 6, n2)].copy()
    l1 = rng.uniform(0, 100, (n1, 2)).astype(np.float32)
    l2 = rng.uniform(0, 100, (n2, 2)).astype(np.float32)
    F = rng.normal(size=(3, 3)).astype(np.float32)
    for H, Fm in ((I3, None), (None, F), (I3, F)):
        for cross, ratio, dist in ((True, 1.0, 3.2), (False, 1.0, 3.2)):
            exp = ref.sift_match_guided(oracle, d1, l1, d2, l2, H=H, F=Fm, h_max_residual=400.0, f_max_residual=50.0,
                                        max_ratio=ratio, max_distance=dist, cross_check=cross)
            got = gpu.sift_match_guided(d1, l1, d2, l2, H=H, F=Fm, h_max_residual=400.0, f_max_residual=50.0,
                                        max_ratio=ratio, max_distance=dist, cross_check=cross)
            assert np.array_equal(got, exp), (nchunk, H is not None, Fm is not None, cross, len(got), len(exp))
    # The sets above hold so many equal rows that 12 of these 18 expectations are empty and the rest hold at most 20
    # matches; at max_ratio 1 a tie is rejected whichever column won.  Beside them: tied sets below the clamp under a
    # ratio above 1, where the guided walk's choice among equal columns that PASS the filter shows in m12 / m21.
    t1, t2 = er.tied_sets(n1, n2)
    S = er.scores(t1, t2)
    for H, Fm in ((I3, None), (None, F), (I3, F)):
        Sg = S.copy()
        Sg[ref.guided_reject(l1, l2, H, Fm, 400.0, 50.0)] = 0
        first = er.match(S, cross_check=False, **er.RATIO_PROBE)
        for cross in (True, False):
            exp = er.match(Sg, cross_check=cross, **er.RATIO_PROBE)
            assert exp[3] >= er.MARGIN and len(exp[0]) > 10 and (exp[1] != -1).sum() > 50 and (exp[2] != -1).sum() > 100
            got = device_match(gpu, t1, t2, cross_check=cross, guide=(l1, l2, H, Fm, 400.0, 50.0), **er.RATIO_PROBE)
            for g, e in zip(got, exp[:3]):
                assert np.array_equal(g, e), (nchunk, H is not None, Fm is not None, cross)
            assert np.array_equal(gpu.sift_match_guided(t1, l1, t2, l2, H=H, F=Fm, h_max_residual=400.0, f_max_residual=50.0,
                                                        cross_check=cross, **er.RATIO_PROBE), exp[0])
        assert (exp[1] != first[1]).sum() > 50          # the filter moves the winner to a later equal column


@pytest.mark.parametrize("budget", [0, 3000])
@pytest.mark.parametrize("nchunk", [0, 2])
def test_batch_mixed_modes_equal_single_pairs(gpu, oracle, budget, nchunk, sift_tuning):
    sift_tuning(nchunk=nchunk, batch_partials=budget)
    sizes = [300, 0, 129, 700, 64]
    descs, locs = [], []
    rng = np.random.default_rng(9)
    for n in sizes:
        f = rng.random((n, 128), dtype=np.float32) ** 2
        f /= np.maximum(np.linalg.norm(f, axis=1, keepdims=True), 1e-9)
        descs.append(np.clip(np.round(512 * f), 0, 255).astype(np.uint8))
        locs.append(rng.uniform(0, 60, (n, 2)).astype(np.float32))
    descs[3][:300] = np.clip(descs[0].astype(np.int32) + rng.integers(-4, 5, (300, 128)), 0, 255).astype(np.uint8)
    locs[3][:300] = locs[0] + rng.normal(0, 2, (300, 2)).astype(np.float32)
    F = rng.normal(size=(3, 3)).astype(np.float32)
    pairs = np.array([[0, 3], [3, 0], [0, 1], [2, 4], [4, 3], [0, 2], [3, 2]], np.uint32)
    guides = [(I3, None), (None, F), (I3, F), (I3, None), (None, None), (None, F), (I3, F)]
    res = gpu.sift_match_guided_batch(descs, locs, pairs, guides, h_max_residual=9.0, f_max_residual=25.0)
    for p, ((a, b), (H, Fm)) in enumerate(zip(pairs, guides)):
        exp = ref.sift_match_guided(oracle, descs[a], locs[a], descs[b], locs[b], H=H, F=Fm, h_max_residual=9.0,
                                    f_max_residual=25.0)
        one = gpu.sift_match_guided(descs[a], locs[a], descs[b], locs[b], H=H, F=Fm, h_max_residual=9.0, f_max_residual=25.0)
        assert np.array_equal(res[p], exp), (p, len(res[p]), len(exp))
        assert np.array_equal(one, exp), p
        if H is None and Fm is None:
            assert np.array_equal(res[p], gpu.sift_match(descs[a], descs[b]))
    assert len(res[0]) > 20
