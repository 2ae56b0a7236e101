"""Plain reference, generators and probes for the edge tests of the SIFT matcher (test infrastructure).

The specification is feature/sift.cc:55-204: S = d1 d2^T in exact integers, per row a strict-> ascending scan that starts
at best = second = 0, arg = -1, then acos / max_distance / max_ratio in float32 and an optional cross check.  Everything
here is numpy on the int64 product; neither device code nor the C oracle is used (tests/test_sift_edge_cpu.py compares
this file with the C oracle).

The float decisions use the host libm's acosf, as tests/sift_guided_ref.py does.  The device acosf may differ from it in
the last ulps (about 1e-6 rad absolute), so a row whose decision lies within MARGIN = 1e-4 rad of a threshold is not a
fair row: one_way returns every row's margin, and the generators' committed seeds have NO row below MARGIN under the
option sets the GPU tests use (asserted by the CPU test; the GPU tests leave out nothing).  Two operands are exact on
any libm and need no margin: a score >= 512^2 clamps to acos(1) = 0, and a row without a best column takes no float
test at all.

Probes:
  ARG_PROBE    max_ratio 1e30, max_distance 4: m == arg for every row with best > 0 and second < 512^2, -1 otherwise;
               no float test is near its threshold, the integer rule (first index of equal bests) shows alone.
  RATIO_PROBE  max_ratio 1.5, max_distance 3.2: a tied row (best == second) passes; at any ratio <= 1 it cannot."""
import ctypes
import ctypes.util
import functools

import numpy as np

_LIBM = ctypes.CDLL(ctypes.util.find_library("m"))
_LIBM.acosf.restype = ctypes.c_float
_LIBM.acosf.argtypes = [ctypes.c_float]
F32 = np.float32
CLAMP = 512 * 512
MARGIN = 1e-4
ARG_PROBE = dict(max_ratio=1e30, max_distance=4.0)
RATIO_PROBE = dict(max_ratio=1.5, max_distance=3.2)
DEFAULTS = dict(max_ratio=0.8, max_distance=0.7)

# the shapes the GPU tests run (the CPU test checks the same ones against the oracle and the margin rule)
TIED_SHAPE = (700, 1900)                       # 6 row tiles x 15 column tiles
HIGH_SHAPES = ((300, 77), (1000, 1500), (129, 513))
UNIFORM_SHAPES = ((200, 150), (130, 257))
SECOND_RATIOS = (0.8, 0.95)
EDGE_NS = (31, 32, 33, 63, 64, 65, 511, 512, 513, 1023, 1024, 1025)   # MFMA row tile, wavefront rows, stripe, 2 stripes
EDGE_MS = (130, 257)
WIDE_NS = (16383, 16384, 16385)                # the one-workgroup compaction holds 16384 rows
WIDE_M = 130


def scores(d1, d2):
    """d1 d2^T in exact integers (every product sum is below 2^53, so the float64 matrix product is exact)"""
    a = np.ascontiguousarray(d1, np.uint8).reshape(-1, 128).astype(np.float64)
    b = np.ascontiguousarray(d2, np.uint8).reshape(-1, 128).astype(np.float64)
    return (a @ b.T).astype(np.int64)


def top2(S):
    """(best, second, arg) per row of the int64 scores S: start 0 / 0 / -1, strictly greater replaces the best, else
    strictly greater replaces the second; the first of equal maxima keeps the best place (argmax: first index)"""
    S = np.asarray(S, np.int64)
    rows, cols = S.shape
    if cols == 0:
        return np.zeros(rows, np.int64), np.zeros(rows, np.int64), np.full(rows, -1, np.int64)
    ar = np.arange(rows)
    idx = np.argmax(S, axis=1)
    best = S[ar, idx]
    rest = S.copy()
    rest[ar, idx] = 0                                  # the start value: nothing <= 0 ever takes a place
    second = np.maximum(rest.max(axis=1), 0)
    arg = np.where(best > 0, idx, -1)
    return np.maximum(best, 0), np.where(best > 0, second, 0), arg


def third(S):
    """the third place of the same scan (0 if there is none): what the second best would be without the runner-up"""
    S = np.asarray(S, np.int64)
    if S.shape[1] < 3:
        return np.zeros(S.shape[0], np.int64)
    return np.maximum(np.partition(S, -3, axis=1)[:, -3], 0)


def _acosf(x):
    u, inv = np.unique(np.asarray(x, F32), return_inverse=True)
    return np.array([_LIBM.acosf(float(v)) for v in u], F32)[inv.reshape(-1)]


def one_way(best, second, arg, max_ratio, max_distance):
    """sift.cc:85-104 on the scan's results: (m int32 [rows], margin float64 [rows]).  margin = min(|bn - max_distance|,
    |bn - max_ratio sn|), inf where no float test is taken (no best column) and for the ratio test of two clamped
    scores (0 >= r * 0 on any libm)."""
    best, second, arg = (np.asarray(v, np.int64) for v in (best, second, arg))
    norm = F32(1.0 / (512.0 * 512.0))
    cb = np.minimum(norm * best.astype(F32), F32(1.0))
    cs = np.minimum(norm * second.astype(F32), F32(1.0))
    bn, sn = _acosf(cb), _acosf(cs)
    with np.errstate(over="ignore"):
        lim = F32(max_ratio) * sn
    live = arg != -1
    ok = live & ~(bn > F32(max_distance)) & ~(bn >= lim)
    m = np.where(ok, arg, -1).astype(np.int32)
    md = np.abs(bn.astype(np.float64) - float(F32(max_distance)))
    mr = np.abs(bn.astype(np.float64) - float(F32(max_ratio)) * sn.astype(np.float64))
    mr[(cb == 1) & (cs == 1)] = np.inf
    margin = np.where(live, np.minimum(md, mr), np.inf)
    return m, margin


def cross(m12, m21, cross_check=True):
    """sift.cc:118-143: the match list [M][2] uint32 in ascending index of set 1"""
    keep = m12 != -1
    if cross_check:
        i = np.nonzero(keep)[0]
        keep = np.zeros(len(m12), bool)
        keep[i] = m21[m12[i]] == i
    i1 = np.nonzero(keep)[0]
    return np.stack([i1, m12[i1]], axis=1).astype(np.uint32).reshape(-1, 2)


def match(S, max_ratio=0.8, max_distance=0.7, cross_check=True):
    """(matches, m12, m21, margin): margin = the smallest margin of any row of either direction"""
    S = np.asarray(S, np.int64)
    n1, n2 = S.shape
    if n1 == 0 or n2 == 0:
        return np.zeros((0, 2), np.uint32), np.full(n1, -1, np.int32), np.full(n2, -1, np.int32), np.inf
    m12, g12 = one_way(*top2(S), max_ratio, max_distance)
    m21, g21 = one_way(*top2(S.T), max_ratio, max_distance)
    return cross(m12, m21, cross_check), m12, m21, min(g12.min(), g21.min())


# ---------------------------------------------------------------------------------------------- generators
@functools.lru_cache(maxsize=None)
def tied_sets(n1, n2, seed=1):
    """Six base descriptors (bytes 0..40, three bytes per base in 130..255); both sets are exact copies of them, every
    third column of set 2 LOWERED by 0 / 1 noise (raised columns would make the maxima unique), one all-zero row.
    Every row's best score is then tied over many columns, and at any max_ratio <= 1 nothing matches."""
    rng = np.random.default_rng(seed)
    base = rng.integers(0, 41, (6, 128)).astype(np.uint8)
    for b in range(6):
        base[b, rng.choice(128, 3, replace=False)] = rng.integers(130, 256, 3)
    d1 = base[rng.integers(0, 6, n1)].copy()
    d2 = base[rng.integers(0, 6, n2)].copy()
    low = d2[::3].astype(np.int32) - rng.integers(0, 2, (len(d2[::3]), 128))
    d2[::3] = np.clip(low, 0, 255).astype(np.uint8)
    if n1 > 10:
        d1[5] = 0
    d1.setflags(write=False)
    d2.setflags(write=False)
    return d1, d2


def tie_stats(S):
    """of the rows of S with a best > 0: (share whose best is tied over >= 2 column tiles of 128 AND both lane halves
    (col >> 2) & 1, share whose first tied column lies in the upper half)"""
    best, _, arg = top2(S)
    live = np.nonzero(arg != -1)[0]
    spread = upper = 0
    for i in live:
        c = np.nonzero(S[i] == best[i])[0]
        spread += len(np.unique(c >> 7)) >= 2 and len(np.unique((c >> 2) & 1)) == 2
        upper += (c[0] >> 2) & 1
    return spread / max(len(S), 1), upper / max(len(S), 1)


def l1_root(rng, n, power=12):
    """descriptors shaped like the reference's default normalisation (L1-root): byte = 512 sqrt(share) of a peaky
    histogram; a bin with 1/16 of the mass is a byte >= 128, and the squared norm is 512^2 up to rounding"""
    f = rng.random((n, 128)) ** power
    return np.clip(np.round(512.0 * np.sqrt(f / f.sum(axis=1, keepdims=True))), 0, 255).astype(np.uint8)


def _lowered(rng, rows, most=3):
    return np.clip(rows.astype(np.int32) - rng.integers(0, most + 1, rows.shape), 0, 255).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def high_byte_sets(n1, n2, seed=1):
    """L1-root descriptors with planted correspondences: set 2 holds lowered copies (0..3 per byte) of 60 % of the
    smaller set's size, every 8th of them an EXACT copy (its score is the squared norm, which reaches 512^2 for some
    rows: the clamp), and near-duplicates of true matches that differ by +1 / -1 in ONE byte where the row holds a byte
    >= 128: the winner is decided by a score difference of one row byte.
    Returns d1, d2, info: corr [k][2] (row, column), exact (rows), plus / minus [..][3] (row, true column, neighbour)."""
    rng = np.random.default_rng(seed)
    d1, d2 = l1_root(rng, n1), l1_root(rng, n2)
    k = min(n1, n2) * 6 // 10
    src, perm = rng.permutation(n1)[:k], rng.permutation(n2)
    dst, spare = perm[:k], list(perm[k:])
    d2[dst] = _lowered(rng, d1[src])
    d2[dst[::8]] = d1[src[::8]]
    plus, minus = [], []
    for j in range(k):
        if j % 8 not in (1, 2) or not spare:
            continue
        row, col = src[j], dst[j]
        pos = int(np.argmax(d1[row]))
        sign = 1 if j % 8 == 1 else -1
        if d1[row, pos] < 128 or not 0 < d2[col, pos] < 255:
            continue
        o = spare.pop()
        d2[o] = d2[col]
        d2[o, pos] = int(d2[col, pos]) + sign
        (plus if sign > 0 else minus).append((row, col, o))
    info = dict(corr=np.stack([src, dst], axis=1), exact=src[::8].copy(),
                plus=np.array(plus, np.int64).reshape(-1, 3), minus=np.array(minus, np.int64).reshape(-1, 3))
    d1.setflags(write=False)
    d2.setflags(write=False)
    return d1, d2, info


@functools.lru_cache(maxsize=None)
def uniform_sets(n1, n2, seed=1):
    """uniform bytes 0..255 (a full row against a full column scores about 2e6: both places clamp and the row has no
    match under any option), half of the rows thinned to 2..30 non-zero bytes so that scores straddle 512^2"""
    rng = np.random.default_rng(seed)
    out = []
    for n in (n1, n2):
        d = rng.integers(0, 256, (n, 128)).astype(np.uint8)
        for i in range(0, n, 2):
            keep = rng.choice(128, int(rng.integers(2, 31)), replace=False)
            row = np.zeros(128, np.uint8)
            row[keep] = d[i, keep]
            d[i] = row
        d.setflags(write=False)
        out.append(d)
    return tuple(out)


SECOND_KINDS = ("half", "block", "tile", "chunk")
_SECOND_DELTA = dict(half=4, block=32, tile=128, chunk=1024)


@functools.lru_cache(maxsize=None)
def second_sensitive(n1=1000, n2=2000, seed=1):
    """L1-root sets where the SECOND best decides: of every 10 rows, 4 have a true match (lowered copy) AND a planted
    runner-up (the match lowered by 1 more in two of the row's small bytes: bn / sn > 0.99, rejected at 0.8 and 0.95),
    4 have a true match only (their second best is a random column: accepted), 2 have none.  With the third best in
    the second's place the first group would be accepted.  The runner-up's column lies, relative to the best, in the
    other lane half of the same 8 columns, in another 32-column block of the tile, in another tile, or 1024 columns away
    (another chunk at 2 and at 5 chunks per walk of 2000 columns), alternately behind and before it in scan order.
    Returns d1, d2, plan [rows][4] int64 (row, best column, runner-up column or -1, kind index or -1)."""
    rng = np.random.default_rng(seed)
    d1, d2 = l1_root(rng, n1), l1_root(rng, n2)
    free = np.ones(n2, bool)
    plan = []
    for i in range(n1):
        r = i % 10
        if r >= 8:
            continue
        if r < 4:
            kind = SECOND_KINDS[r]
            delta = _SECOND_DELTA[kind]
            while True:
                a = int(rng.integers(0, n2))
                b = a + delta if kind == "chunk" else a ^ delta
                if b < n2 and free[a] and free[b]:
                    break
            lo, hi = min(a, b), max(a, b)
            t, u = (lo, hi) if (i // 10) % 2 == 0 else (hi, lo)
            free[t] = free[u] = False
            d2[t] = _lowered(rng, d1[i:i + 1])[0]
            both = np.nonzero((d1[i] > 0) & (d2[t] > 0))[0]
            d2[u] = d2[t]
            d2[u, both[np.argsort(d1[i, both], kind="stable")[:2]]] -= 1   # the row's two smallest bytes: a near tie
            plan.append((i, t, u, r))
        else:
            t = int(rng.choice(np.nonzero(free)[0]))
            free[t] = False
            d2[t] = _lowered(rng, d1[i:i + 1])[0]
            plan.append((i, t, -1, -1))
    d1.setflags(write=False)
    d2.setflags(write=False)
    return d1, d2, np.array(plan, np.int64)


def second_place(S):
    """column of the second best of every row (first index; -1 where there is none): where the runner-up really lies"""
    S = np.asarray(S, np.int64)
    best, second, arg = top2(S)
    rest = S.copy()
    rest[np.arange(len(S)), np.maximum(arg, 0)] = -1
    col = np.argmax(rest, axis=1)
    return np.where((arg != -1) & (second > 0), col, -1)


def second_relation(t, u, cols_per_chunk):
    """which of SECOND_KINDS + ("before",) hold for best column t and runner-up column u"""
    out = set()
    if t >> 3 == u >> 3 and (t >> 2) & 1 != (u >> 2) & 1:
        out.add("half")
    if t >> 7 == u >> 7 and t >> 5 != u >> 5:
        out.add("block")
    if t >> 7 != u >> 7:
        out.add("tile")
    if all(t // c != u // c for c in cols_per_chunk):
        out.add("chunk")
    if u < t:
        out.add("before")
    return out


PLACE_N = 1900            # 14 full column tiles + 108 columns; 5 chunks of 3 tiles, 2 chunks of 8
PLACE_PAIRS = ((0, 1), (3, 4), (4, 8), (7, 31), (31, 32), (127, 128), (128 + 5, 640 + 1), (0, PLACE_N - 1))
PLACE_TRIPLE = (10, 1101, 1800)   # chunks 0 / 2 / 4 of 5
PLACE_SINGLES = ((6,), (700,), (PLACE_N - 2,))
PLACE_FAR = {"none": (), "a": (0, 3, 7, 127, 128 + 5, 10), "b": (4, 31)}


@functools.lru_cache(maxsize=None)
def placements():
    """Deterministic table of two sets A, B of PLACE_N descriptors.  A "row" descriptor is h = 200 in ONE private bin
    and 0 elsewhere; its own columns in the other set hold 200 (or 199: a runner-up) in that bin over a shared
    background of 10, so its scores are 40000 / 39800 for its own columns, 2000 for every other column, 0 for the other
    set's row descriptors: the entries do not interact.  Entries, once with rows in A and columns in B (bins 0..) and
    once exchanged (bins 64..): every pair of PLACE_PAIRS and the triple as equal bests (expected: the first), the same
    with the best in the first / in the last place and the others one lower (a runner-up), three single columns.
    Returns A, B, entries: list of (direction, row, columns, index of the best among them or -1 for a tie)."""
    n, g, h = PLACE_N, 10, 200
    groups = [(c, -1) for c in PLACE_PAIRS + (PLACE_TRIPLE,)]
    groups += [(c, w) for c in PLACE_PAIRS + (PLACE_TRIPLE,) for w in (0, len(c) - 1)]
    groups += [(c, 0) for c in PLACE_SINGLES]
    used = {c for cols, _ in groups for c in cols}
    rows = [r for r in range(2, n, 61) if r not in used][:len(groups)]
    assert len(rows) == len(groups) <= 64
    sets = [np.full((n, 128), g, np.uint8), np.full((n, 128), g, np.uint8)]
    entries = []
    for direction in (0, 1):
        rset, cset = sets[direction], sets[1 - direction]
        for e, ((cols, w), r) in enumerate(zip(groups, rows)):
            b = 64 * direction + e
            rset[r] = 0
            rset[r, b] = h
            for k, c in enumerate(cols):
                cset[c, b] = h if w in (-1, k) else h - 1
            entries.append((direction, r, cols, w))
    for s in sets:
        s.setflags(write=False)
    return sets[0], sets[1], entries


def placement_locations(far):
    """locations for the guided runs (H = identity, threshold 16): every keypoint at the origin except the columns
    PLACE_FAR[far] of both sets, which lie 1000 away and are rejected for every row"""
    loc = np.zeros((PLACE_N, 2), np.float32)
    loc[list(PLACE_FAR[far]), 0] = 1000.0
    return loc


def placement_expected(entry, far="none"):
    """the column an entry's row must report under ARG_PROBE: the best of its columns that is not rejected; of equal
    ones the first"""
    _, _, cols, w = entry
    live = [(0 if w in (-1, k) else 1, c) for k, c in enumerate(cols) if c not in PLACE_FAR[far]]
    return min(live)[1] if live else None
