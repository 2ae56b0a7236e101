"""Guided SIFT matching on the CPU: the numpy reference (tests/sift_guided_ref.py) pinned to the C oracle and to the
reference's known answers (src/feature/sift_test.cc:430-475), hand-computed filter cases, and the refusal of the new
entry points without a GPU."""
import ctypes as C

import numpy as np
import pytest

from tests import sift_guided_ref as ref
from tests.test_sift_cpu import sift_reference_cases

I3 = np.eye(3, dtype=np.float32)


def test_reference_without_filter_is_the_oracle(oracle):
    for name, d1, d2, opt, expected in sift_reference_cases(oracle):
        got = ref.sift_match_guided(oracle, d1, None, d2, None, **opt)
        assert np.array_equal(got, oracle.sift_match(d1, d2, **opt)[0]), name
        assert len(got) == expected, name
    rng = np.random.default_rng(5)
    for n1, n2 in ((1, 1), (40, 70), (300, 77), (128, 1)):
        base = rng.integers(0, 60, (max(n1, n2), 128), dtype=np.uint8)
        d1 = base[:n1].copy()
        d2 = np.clip(base[rng.permutation(max(n1, n2))[:n2]].astype(np.int32) + rng.integers(-3, 4, (n2, 128)), 0, 255).astype(np.uint8)
        if n2 > 4:
            d2[2] = d2[3]
        for cross in (True, False):
            for ratio in (0.8, 1.0):
                exp = oracle.sift_match(d1, d2, max_ratio=ratio, cross_check=cross)[0]
                got = ref.sift_match_guided(oracle, d1, None, d2, None, max_ratio=ratio, cross_check=cross)
                assert np.array_equal(got, exp), (n1, n2, cross, ratio)


def kat_case(oracle):
    """sift_test.cc:430-443: two random descriptors against the same rows reversed, keypoints x = {1, 2} vs {2, 1}"""
    d1 = oracle.sift_random_descriptors(2)
    d2 = d1[::-1].copy()
    k1 = np.array([[1, 0], [2, 0]], np.float32)
    k2 = np.array([[2, 0], [1, 0]], np.float32)
    return d1, k1, d2, k2


def test_reference_known_answers(oracle):
    d1, k1, d2, k2 = kat_case(oracle)
    got = ref.sift_match_guided(oracle, d1, k1, d2, k2, H=I3)
    assert got.tolist() == [[0, 1], [1, 0]]
    k1[0, 0] = 100
    got = ref.sift_match_guided(oracle, d1, k1, d2, k2, H=I3)
    assert got.tolist() == [[1, 0]]
    e_d, e_k = np.zeros((0, 128), np.uint8), np.zeros((0, 2), np.float32)
    for a, ka, b, kb in ((e_d, e_k, d2, k2), (d1, k1, e_d, e_k), (e_d, e_k, e_d, e_k)):
        assert len(ref.sift_match_guided(oracle, a, ka, b, kb, H=I3)) == 0


def test_filter_boundaries_by_hand():
    # H = I, integer locations: r == 16 exactly is kept, the next float above 16 as threshold's neighbour is rejected
    l1 = np.array([[10, 10]], np.float32)
    l2 = np.array([[14, 10], [10, 6], [13, 13], [15, 10]], np.float32)   # r = 16, 16, 18, 25
    assert ref.guided_reject(l1, l2, H=I3, h_max_residual=16.0).tolist() == [[False, False, True, True]]
    below = float(np.nextafter(np.float32(16), np.float32(0)))
    assert ref.guided_reject(l1, l2[:1], H=I3, h_max_residual=below).tolist() == [[True]]
    # h2 = 0: h0 / 0 = Inf, the residual is Inf: rejected (Inf > t); 0 / 0 = NaN: kept
    Hz = np.array([[1, 0, 0], [0, 1, 0], [0, 0, 0]], np.float32)
    assert ref.guided_reject(np.array([[3, 4]], np.float32), l2[:1], H=Hz).tolist() == [[True]]
    assert ref.guided_reject(np.array([[0, 0]], np.float32), l2[:1], H=Hz).tolist() == [[False]]
    # F = 0: e = 0 and a zero Sampson denominator, 0 / 0 = NaN: kept
    Fz = np.zeros((3, 3), np.float32)
    assert not ref.guided_reject(l1, l2, F=Fz, f_max_residual=0.0).any()
    # F with only F[2][2]: e = F22 != 0, denominator 0 -> Inf: rejected
    F22 = np.zeros((3, 3), np.float32)
    F22[2, 2] = 1
    assert ref.guided_reject(l1, l2, F=F22, f_max_residual=1e30).all()
    # subnormal intermediates: a_i ~ 1e-39 (subnormal) -- the squares flush nothing, the residual is exact in float32
    Fs = np.zeros((3, 3), np.float32)
    Fs[0, 2] = np.float32(1e-39)
    Fs[2, 0] = np.float32(1e-39)
    x = np.array([[1, 0]], np.float32)
    r = ref.guided_reject(x, np.array([[1, 0]], np.float32), F=Fs, f_max_residual=0.4)
    # e = x2*a0 + a2 = 1e-39 + 1e-39; den = a0^2 + b0^2 (underflow to 0 for 1e-78) -> 0: NaN or Inf decides
    e = np.float32(np.float32(1) * Fs[0, 2]) + np.float32(np.float32(1) * Fs[2, 0])
    den = np.float32(Fs[0, 2] * Fs[0, 2]) + np.float32(Fs[2, 0] * Fs[2, 0])
    with np.errstate(all="ignore"):
        assert r.tolist() == [[bool(np.float32(e * e) / den > np.float32(0.4))]]


def test_f_filter_is_asymmetric():
    """set 1 feeds a_i = F x1, set 2 b_j = F^T x2: exchanging the sets changes the answer for a non-symmetric F"""
    rng = np.random.default_rng(1)
    F = rng.normal(size=(3, 3)).astype(np.float32)
    l1 = rng.uniform(0, 50, (30, 2)).astype(np.float32)
    l2 = rng.uniform(0, 50, (40, 2)).astype(np.float32)
    a = ref.guided_reject(l1, l2, F=F, f_max_residual=4.0)
    b = ref.guided_reject(l2, l1, F=F, f_max_residual=4.0).T
    assert a.any() and (~a).any() and not np.array_equal(a, b)


def test_no_cpu_fallback_for_guided_entries(pcdhip, oracle):
    if pcdhip.device_count() > 0:
        pytest.skip("a GPU is present; the refusal path is exercised on CPU-only boxes")
    d1, k1, d2, k2 = kat_case(oracle)
    with pytest.raises(pcdhip.PcdError) as e:
        pcdhip.sift_match_guided(d1, k1, d2, k2, H=I3)
    assert e.value.status == pcdhip.PCD_ERR_NO_DEVICE
    with pytest.raises(pcdhip.PcdError) as e:
        pcdhip.sift_match_guided_batch([d1, d2], [k1, k2], [[0, 1]], [(None, I3)])
    assert e.value.status == pcdhip.PCD_ERR_NO_DEVICE
    L = pcdhip.lib()
    h = I3.reshape(9)
    L.pcd_sift_match_guided_device.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int,
                                               C.c_void_p, C.c_void_p, C.c_float, C.c_float, C.c_float, C.c_float,
                                               C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    cnt = np.zeros(1, np.int32)
    st = L.pcd_sift_match_guided_device(0, None, None, 2, None, None, 2, h.ctypes.data, None, 16.0, 16.0, 0.8, 0.7, 1,
                                        None, None, None, cnt.ctypes.data, None)
    assert st == pcdhip.PCD_ERR_NO_DEVICE
    g = (pcdhip.SiftGuide * 1)()
    g[0].mode = pcdhip.SIFT_GUIDE_H
    first = np.array([0, 2, 4], np.uint64)
    pairs = np.array([[0, 1]], np.uint32)
    off = np.zeros(1, np.uint64)
    L.pcd_sift_match_guided_batch_device.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p,
                                                     C.c_int, C.c_void_p, C.c_float, C.c_float, C.c_float, C.c_float,
                                                     C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    st = L.pcd_sift_match_guided_batch_device(0, None, None, first.ctypes.data, 2, pairs.ctypes.data, 1, C.cast(g, C.c_void_p),
                                              16.0, 16.0, 0.8, 0.7, 1, None, off.ctypes.data, cnt.ctypes.data, None)
    assert st == pcdhip.PCD_ERR_NO_DEVICE
