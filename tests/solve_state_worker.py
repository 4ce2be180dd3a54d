"""The child process of tests/test_gpu_solve_state.py::test_guesses_and_lag_under_the_process_wide_switches: KNP_EXTRAPOLATE,
KNP_EXTRAPOLATE_ORDER(_EMI) and KNP_BJ_LAG are read once per process.  Runs GUESS_OPS on one mesh under the environment it was started
with and writes what every solve left (fields, histories, inverses, counters); the parent checks it against the model.
usage: [KNP_...=...] solve_state_worker.py MESH OUT.npz"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path[:0] = [os.path.join(ROOT, "knp-emi-dg_amd"), os.path.join(ROOT, "oracle"), ROOT, HERE]
import solve_state_cases as T                                                                    # noqa: E402
from common import device_for, push_state                                                           # noqa: E402

pb, volt = T.problem(sys.argv[1])
dev = device_for(pb)
try:
    push_state(dev, pb)
    T.save_rec(sys.argv[2], T.run_ops(dev, pb, T.coefficient_states(pb, volt), T.GUESS_OPS))
finally:
    dev.close()
