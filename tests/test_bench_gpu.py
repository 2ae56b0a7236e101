"""bench.py end to end at a small size: a plain run prints the headline line alone, --steps sets the timed steps, and
--dump-outputs writes what the last timed step computed (float32 / float64, at most 64 MB, the same in every run)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = ["--cloud", "200000", "--queries", "20000", "--cams", "20", "--points", "5000"]


def _bench(*args):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", *SMALL, *args],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    return json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])


@pytest.mark.gpu
def test_plain_run_and_dumped_outputs(gpu, tmp_path):
    from pcdhip import synth
    a = _bench("--steps", "3", "--warmup", "1", "--dump-outputs", str(tmp_path / "a"))
    b = _bench("--steps", "2", "--warmup", "0", "--dump-outputs", str(tmp_path / "b"))
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in a, k
    assert a["steps"] == 3 and a["warmup"] == 1 and a["ms_per_step"] > 0
    assert not {"kernel_ms", "roofline", "cpu_baseline", "sift_block"} & set(a)      # --full only
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == sorted(os.listdir(tmp_path / "b"))
    assert {"nn_idx.npy", "nn_sqdist.npy", "abcd.npy", "type.npy", "H_img.npy", "cost.npy", "H_pt.npy", "W.npy"} <= set(names)
    total = 0
    for n in names:
        x, y = np.load(tmp_path / "a" / n), np.load(tmp_path / "b" / n)
        assert x.dtype in (np.float32, np.float64), n
        np.testing.assert_allclose(x, y, rtol=1e-12, atol=0, err_msg=n)
        total += os.path.getsize(tmp_path / "a" / n)
    assert total <= 64 << 20
    # the dumped NN rows are the device search of the bench's own seeded queries
    xyz, nrm = synth.cloud_planes(200000)
    q = synth.queries(xyz, 20000, seed=99)
    rows = np.load(tmp_path / "a" / "query_rows.npy").astype(np.int64)
    c = gpu.Cloud(xyz, nrm, device=0, raw_lidar_frame=False)
    idx, sq, found = c.nn(q[rows])
    c.close()
    got_idx, got_sq = np.load(tmp_path / "a" / "nn_idx.npy"), np.load(tmp_path / "a" / "nn_sqdist.npy")
    f = found == 1
    assert f.any() and np.array_equal(got_idx[~f], np.full((~f).sum(), 0xFFFFFFFF, np.float64))
    assert np.array_equal(got_idx[f], idx[f].astype(np.float64))
    assert np.array_equal(got_sq[f].view(np.uint32), sq[f].view(np.uint32))
