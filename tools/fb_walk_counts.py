"""Counters of k_nn_fallback's walk on the inputs of tests/test_nn_compact_pyramid_gpu.py::test_walk_is_the_parents_walk.

    python tools/fb_walk_counts.py

prints fallback_queries and fallback_points of a NN_FALLBACK_ONLY call per input, for the library of the tree the
script lies in.  The test's constants are this output on the commit before the compact pyramid (that checkout plus
this script and the test file): the compact tree has to walk the same nodes in the same order.
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "colmap-pcd_amd")):
    sys.path.insert(0, p)
import pcdhip  # noqa: E402
from tests import test_nn_compact_pyramid_gpu as t  # noqa: E402

for name in sorted(t.PARENT_WALK):
    print(name, *t.walk_counts(pcdhip, name), flush=True)
