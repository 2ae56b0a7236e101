"""staged_points of k_nn_brick_clip on the sheet of tests/test_nn_brick_seed_gpu.py::test_sheet_stages_less_than_the_parent.

    python tools/brick_seed_counts.py [--model-only]

prints what tools/brick_clip_sim.py's model predicts for that input -- the kernel that leaves an empty brick's d_k at its
incoming value (rule `own`) and the substitute rule the kernel ships (`class`) -- and then staged_points of a clip-on
NN_GRID call with the statistics on, for the library of the tree the script lies in.  The test's constant is this output
on the commit before the substitute (that checkout plus this script, the model and the test file).
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "colmap-pcd_amd"), os.path.join(ROOT, "tools")):
    sys.path.insert(0, p)
import brick_clip_sim as sim  # noqa: E402
from tests import test_nn_brick_seed_gpu as t  # noqa: E402

xyz, q = t.sheet_input()
r = sim.run(sim.Model(xyz, t.SHEET_H), q, 1 << 30, 1, ("own", "class"))
print("model: own %.0f  class %.0f  ratio %.3f" % (r["own"]["staged_points"], r["class"]["staged_points"],
                                                   r["class"]["staged_points"] / r["own"]["staged_points"]), flush=True)
if "--model-only" not in sys.argv:
    import pcdhip  # noqa: E402
    print("staged_points", t.sheet_staged(pcdhip), flush=True)
