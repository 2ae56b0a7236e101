"""Guided SIFT matching (H / F) against the unguided matcher: per-kernel times (HIP events of the library's profiler)
for an 8192 x 8192 pair and a 50-image x 8192 block as one guided batch.  Synthetic keypoints with a real two-view
geometry (tests/sift_guided_ref.py two_view_scene: two cameras, points seen by both + distractors), thresholds
max_error^2 = 16 as colmap's defaults.  Usage: python tools/sift_guided_probe.py [--out FILE]"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "colmap-pcd_amd"))
import numpy as np  # noqa: E402
import pcdhip  # noqa: E402
from tests.sift_guided_ref import two_view_scene  # noqa: E402


def descriptors(rng, n):
    f = rng.random((n, 128), dtype=np.float32) ** 2
    f /= np.linalg.norm(f, axis=1, keepdims=True)
    return np.clip(np.round(512 * f), 0, 255).astype(np.uint8)


def timed(fn, reps):
    fn()
    pcdhip.profile_enable(True)
    pcdhip.profile_reset()
    t0 = time.perf_counter()
    for _ in range(reps):
        out = fn()
    wall = (time.perf_counter() - t0) / reps * 1e3
    p = pcdhip.profile_get()
    pcdhip.profile_enable(False)
    return {k: round(t / c, 3) for k, (c, t) in p.items()}, round(wall, 2), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    lines = []
    say = lambda s: (print(s, flush=True), lines.append(s))
    rng = np.random.default_rng(0)
    n = 8192
    l1, l2, F, H, corr = two_view_scene(rng, n, n, shared=0.5)
    d1 = descriptors(rng, n)
    d2 = descriptors(rng, n)
    for s, t in corr:
        d2[t] = np.clip(d1[s].astype(np.int32) + rng.integers(-5, 6, 128), 0, 255).astype(np.uint8)
    say(f"pair {n} x {n} (ms per call; kernel times from the library's event timers)")
    for name, kw in (("unguided", {}), ("guided H", dict(H=H)), ("guided F", dict(F=F)), ("guided H+F", dict(H=H, F=F))):
        k, wall, m = timed(lambda: pcdhip.sift_match_guided(d1, l1, d2, l2, **kw), a.reps)
        say(f"  {name:11s} matches {len(m):5d}  wall {wall:8.2f}  kernels {k}")
    # 50-image block: every image 8192 keypoints of one scene seen from the same first camera pair geometry
    imgs, locs = [], []
    for i in range(50):
        r = np.random.default_rng(100 + i)
        la, lb, Fi, Hi, _ = two_view_scene(r, n, n, shared=0.5)
        imgs.append(descriptors(r, n))
        locs.append(la if i % 2 == 0 else lb)
    pairs = np.concatenate(list(pcdhip.exhaustive_blocks(50, 50)))
    say(f"block: 50 images x {n}, {len(pairs)} pairs in one call (ms per call)")
    for name, g in (("unguided", None), ("guided H", (H, None)), ("guided F", (None, F))):
        if g is None:
            fn = lambda: pcdhip.sift_match_batch(imgs, pairs)
        else:
            fn = lambda: pcdhip.sift_match_guided_batch(imgs, locs, pairs, [g] * len(pairs))
        k, wall, res = timed(fn, 1)
        say(f"  {name:11s} matches {sum(len(x) for x in res):7d}  wall {wall:9.2f}  kernels {k}")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
