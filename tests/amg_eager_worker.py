"""The child process of tests/test_gpu_amg.py::test_eager_vcycle_matches_the_replica_and_the_graph_replay: KNP_NO_GRAPH is read once per
process, so the eager V-cycle (what runs whenever graph capture fails) needs a process of its own.  Runs the cases of
test_gpu_amg._eager_cases on box_P1 and writes the iterates.   usage: KNP_NO_GRAPH=1 amg_eager_worker.py OUT.npz"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path[:0] = [os.path.join(ROOT, "knp-emi-dg_amd"), os.path.join(ROOT, "oracle"), ROOT, HERE]
import test_gpu_amg as T                                                                            # noqa: E402

assert os.environ.get("KNP_NO_GRAPH") == "1"
c = T.Ctx("box_P1", None)
try:
    np.savez(sys.argv[1], **T._eager_cases(c))
finally:
    c.dev.close()
