"""integration/colmap-pcd-hip.patch is a real unified diff against the reference tree: it must
apply cleanly to the files it touches and be exactly what integration/make_patch.py generates.  Compiling the patched
tree needs COLMAP's dependencies (Qt, PCL, FLANN, Ceres, Eigen, Boost ...), none of which is installed here; the
adapters the patch calls are compiled and tested in colmap-pcd_amd/shim/test_shim.cc instead.

The reference tree is not part of this repository, so by default the touched files are rebuilt from the patch itself:
every context and removed line at its old line number, a distinct placeholder line wherever the patch carries none.
That checks the hunks' headers, counts and context against each other and the generator against the patch.  Point
COLMAP_PCD_TREE at a checkout of the reference to run the same tests on its real files."""
import hashlib
import importlib.util
import json
import os
import re
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PATCH = os.path.join(ROOT, "integration", "colmap-pcd-hip.patch")
HUNK = re.compile(r"@@ -(\d+)(?:,(\d+))? \+(\d+)(?:,(\d+))? @@")


def _touched_files():
    files = []
    for line in open(PATCH, encoding="utf-8"):
        if line.startswith("--- a/"):
            files.append(line[6:].strip())
    return files


def _pre_images():
    """{path: {old line number: text}} of every file the patch changes (new files have none)"""
    lines = open(PATCH, encoding="utf-8").read().splitlines(keepends=True)
    files, cur, i = {}, None, 0
    while i < len(lines):
        ln = lines[i]
        i += 1
        if ln.startswith("--- a/"):
            cur = ln[6:].strip()
            continue
        m = HUNK.match(ln)
        if not m:
            continue
        old, n_old, n_new = int(m.group(1)), int(m.group(2) or 1), int(m.group(4) or 1)
        rows = files.setdefault(cur, {})
        last = None
        while n_old > 0 or n_new > 0 or (i < len(lines) and lines[i].startswith("\\")):
            body = lines[i]
            i += 1
            if body.startswith("\\"):                      # "\ No newline at end of file"
                if last is not None:
                    rows[last] = rows[last].rstrip("\n")
                last = None
                continue
            tag, text = body[0], body[1:]
            if tag in " -":
                rows[old], last = text, old
                old += 1
                n_old -= 1
                n_new -= tag == " "
            else:
                assert tag == "+", body
                last = None
                n_new -= 1
        assert n_old == 0 and n_new == 0, (cur, ln)
    return {f: rows for f, rows in files.items() if rows}


@pytest.fixture
def reference_tree(tmp_path):
    """the reference's files as the patch expects them: COLMAP_PCD_TREE, else rebuilt from the patch's own lines"""
    given = os.environ.get("COLMAP_PCD_TREE")
    if given:
        return given
    tree = tmp_path / "reference"
    for f, rows in _pre_images().items():
        dst = tree / f
        dst.parent.mkdir(parents=True, exist_ok=True)
        dst.write_text("".join(rows.get(n, f"@@ line {n} of {f}: not carried by the patch @@\n")
                               for n in range(1, max(rows) + 1)), encoding="utf-8")
    return str(tree)


def test_patch_applies_to_the_reference_tree(tmp_path, reference_tree):
    files = _touched_files()
    assert {"src/optim/bundle_adjustment.cc", "src/sfm/incremental_mapper.cc", "src/controllers/bundle_adjustment.cc",
            "src/util/option_manager.cc", "src/lidar/ply.cc", "src/lidar/hip_backend.h"} <= set(files)
    work = tmp_path / "work"
    for f in files:
        src = os.path.join(reference_tree, f)
        if os.path.exists(src):                      # hip_backend.h is a new file
            dst = work / f
            dst.parent.mkdir(parents=True, exist_ok=True)
            shutil.copy(src, dst)
    subprocess.check_call(["git", "init", "-q", "."], cwd=work)
    r = subprocess.run(["git", "apply", "--check", "--verbose", PATCH], cwd=work, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    subprocess.check_call(["git", "apply", PATCH], cwd=work)
    ba = (work / "src/optim/bundle_adjustment.cc").read_text(encoding="utf-8")
    # the three association loops, LoadPointcloud's device index, Solve / Add*ToProblem, the option
    assert ba.count("hip_blocks_->AddReprojection(") == 5 and ba.count("hip_blocks_->AddLidar(") == 1
    assert "problem_options.evaluation_callback = hip_blocks_.get();" in ba
    assert "MatchClosestLidarPoints(reconstruction_, closest_ids, closest_ranges)" in \
        (work / "src/sfm/incremental_mapper.cc").read_text(encoding="utf-8")
    assert "PCD_GATE_MAPPER_GLOBAL" in (work / "src/sfm/incremental_mapper.cc").read_text(encoding="utf-8")
    assert "PCD_GATE_CONTROLLER" in (work / "src/controllers/bundle_adjustment.cc").read_text(encoding="utf-8")
    assert "InitializeFromRawCloud" in (work / "src/lidar/ply.cc").read_text(encoding="utf-8")
    assert '"Mapper.lidar_backend"' in (work / "src/util/option_manager.cc").read_text(encoding="utf-8")
    # every shim symbol the patched code calls exists in the shim headers of this repository
    shim = "".join(open(os.path.join(ROOT, "colmap-pcd_amd", "shim", h), encoding="utf-8").read()
                   for h in ("lidar_hip.h", "ceres_adapter.h"))
    for sym in ("MatchClosestLidarPointsFlat", "ToLidarPoint", "HipBlockRecorder", "AddReprojection", "AddLidar",
                "Finalize", "HipBackendEnabled", "InitializeFromRawCloud"):
        assert sym in shim, sym


def test_patch_is_what_the_generator_writes(tmp_path):
    # the generator anchors its edits on lines of the reference that the patch does not carry: regenerating needs the
    # real tree.  Without one, the pair (generator, patch) must be the one last regenerated and compared on it.
    lock = json.load(open(os.path.join(ROOT, "tests", "golden", "integration_patch.json")))
    tree = os.environ.get("COLMAP_PCD_TREE")
    if tree:
        gen = tmp_path / "make_patch.py"
        shutil.copy(os.path.join(ROOT, "integration", "make_patch.py"), gen)
        subprocess.check_call([sys.executable, str(gen), tree], cwd=tmp_path, stdout=subprocess.DEVNULL)
        assert (tmp_path / "colmap-pcd-hip.patch").read_bytes() == open(PATCH, "rb").read()
    for rel in ("integration/make_patch.py", "integration/colmap-pcd-hip.patch"):
        digest = hashlib.sha256(open(os.path.join(ROOT, rel), "rb").read()).hexdigest()
        assert digest == lock[rel], f"{rel} changed: regenerate the patch with COLMAP_PCD_TREE set, then update the lock"
    # the file the patch adds is the generator's text, byte for byte
    spec = importlib.util.spec_from_file_location("make_patch", os.path.join(ROOT, "integration", "make_patch.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    patch = open(PATCH, encoding="utf-8").read()
    for rel, text in gen.NEW_FILES.items():
        section = patch.split(f"+++ b/{rel}\n", 1)[1].split("\ndiff ", 1)[0]
        assert "".join(ln[1:] + "\n" for ln in section.splitlines()[1:]) == text, rel
