"""Several contexts alive in one process keep their solver state apart (csrc/solve.hip: Fields and the two PrecState records are
members of knp_ctx).

Solver A runs 4 steps alone.  Then B and C of the same configuration live together and take their steps interleaved (B0 B1 C0 B2 C1
B3 C2 C3), so that at every switch their solution histories, rebuild ages and spectral bounds differ.  Every step of B and of C must
leave what A's same step left: iteration counts, c, phi, phi_M and the whole state_save() snapshot (fields, both histories, both lagged
inverse arrays, every counter and bound).  The yardstick is a second lone run A': where A and A' do not agree bit for bit themselves,
four times their measured difference bounds B and C instead (as in tests/test_gpu_checkpoint.py).
"""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
_EX = os.path.join(os.path.dirname(HERE), "examples", "idealized_geometries")
if _EX not in sys.path:
    sys.path.insert(0, _EX)

STEPS = 4


def _make():
    """The 768-tet one-axon box at P1, HH membrane with the stimulus on, block-Jacobi preconditioner only (KNP_NO_AMG set by the test)."""
    from idealized_common import make_solver, solver_parameters, Constant
    from common import small_3d
    S = make_solver(dim=3, resolution=0, n_axons=1, degree=1, mesh_tuple=small_3d())
    S._unpack_solver_params(solver_parameters(3, 0, emi_dg_chebyshev=True))
    S.save_fields = S.save_solver_stats = False
    S.splitting_scheme = True
    S.setup_varform_emi(); S.setup_varform_knp(); S.setup_solver_emi(); S.setup_solver_knp()
    assert not S.use_amg
    return S, Constant(0.0)


def _step(run, k):
    S, t = run
    S.step_membrane_models(k)
    S.solve_for_time_step(k, t)
    return {"emi_niter": np.asarray(S.emi_niter), "knp_niter": np.asarray(S.knp_niter).ravel(), "c": S.c.array().copy(),
            "phi": S.phi.array().copy(), "phi_M": S.phi_M_prev_PDE.array().copy(), "state": S.dev.state_save().copy()}


def _same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _maxdiff(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.max(np.abs(a - b))) if a.size else 0.0


def _blocks(blob):
    """The blocks of a snapshot as arrays, in the order of its block table (the counters too: they compare as numbers)."""
    from knpemidg import checkpoint as ck
    return ck.split_snapshot(blob)[1]


def _differing_blocks(a, b):
    return "snapshot blocks that differ: %s" % [i for i, (x, y) in enumerate(zip(_blocks(a), _blocks(b))) if not _same_bits(x, y)]


def test_interleaved_contexts_reproduce_a_lone_run(hip_lib, monkeypatch):
    monkeypatch.setenv("KNP_NO_AMG", "1")
    lone = []
    for _ in range(2):                                              # A and A'
        run = _make()
        lone.append([_step(run, k) for k in range(STEPS)])
        run[0].dev.close()
    A, A2 = lone
    exact = all(_same_bits(a[key], b[key]) for a, b in zip(A, A2) for key in a)
    yard = {key: max(_maxdiff(a[key], b[key]) for a, b in zip(A, A2)) for key in A[0] if key != "state"}
    pairs = [(_blocks(a["state"]), _blocks(b["state"])) for a, b in zip(A, A2)]
    yard_state = [max(_maxdiff(x[i], y[i]) for x, y in pairs) for i in range(len(pairs[0][0]))]
    print("yardstick A vs A' (max-norm per field):", {k: v for k, v in yard.items() if v}, "bit-identical:", exact)
    assert all(_same_bits(a[key], b[key]) for a, b in zip(A, A2) for key in ("emi_niter", "knp_niter"))
    assert np.abs(A[-1]["phi_M"] - A[0]["phi_M"]).max() > 0          # the stimulus is on: the steps differ from one another

    B, C = _make(), _make()
    got = {"B": [], "C": []}
    for who, k in (("B", 0), ("B", 1), ("C", 0), ("B", 2), ("C", 1), ("B", 3)):
        got[who].append(_step(B if who == "B" else C, k))
    B[0].dev.close()                                                # closing B must leave C stepping
    for k in (2, 3):
        got["C"].append(_step(C, k))
    C[0].dev.close()
    for who, snaps in got.items():
        assert len(snaps) == STEPS
        for k, (a, b) in enumerate(zip(A, snaps)):
            assert _same_bits(a["emi_niter"], b["emi_niter"]) and _same_bits(a["knp_niter"], b["knp_niter"]), (who, k, a["emi_niter"], b["emi_niter"])
            for key in a:
                if exact:
                    assert _same_bits(a[key], b[key]), (who, "step", k, key, _differing_blocks(a[key], b[key]) if key == "state" else "")
                elif key != "state":
                    assert _maxdiff(a[key], b[key]) <= 4.0 * yard[key], (who, "step", k, key, _maxdiff(a[key], b[key]), yard[key])
                else:
                    for i, (x, y) in enumerate(zip(_blocks(a[key]), _blocks(b[key]))):
                        assert x.shape == y.shape and _maxdiff(x, y) <= 4.0 * yard_state[i], (who, "step", k, "state block", i, _maxdiff(x, y), yard_state[i])
