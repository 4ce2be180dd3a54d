"""CPU check of the energy-norm half of the EMI PCG stop (csrc/krylov.hip: cg_converged, OP_CG_BETA) on the replica of its scalar
recurrence (tests/krylov_ref.py): block-Jacobi only, x0 = 0, no residual target (r_abs = 1e300), so that test (ii),
||phi - phi_k||_A <= rtol ||phi||_A, alone decides; the true energy error at the stop is measured against a direct solve."""
import os
import sys

import numpy as np
import pytest

import knpemi_oracle as ko
import krylov_ref as kr
from common import synthetic_state, small_3d

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples", "idealized_geometries"))

_REFS = {}


def _ref(name):
    if name not in _REFS:
        from knpemidg.mesh import make_mesh_3D
        m, s, f = small_3d() if name == "box" else make_mesh_3D(0, n_axons=1)
        pb = ko.build_idealized(m, s.array(), f.array(), membrane_tags=(1,))
        synthetic_state(pb)
        _REFS[name] = kr.Ref(pb)
    return _REFS[name]


@pytest.mark.parametrize("rtol", [1e-3, 1e-5])
@pytest.mark.parametrize("name", ["box", "axon"])
def test_pcg_energy_stop_bounds_the_true_error(name, rtol):
    """The one-axon mesh converges slowly under block-Jacobi (beta ~ 0.96-1.03 for hundreds of steps): the one-step estimate with beta
    capped at 0.9 stopped at 3.4x / 5.5x the asked error there; the smoothed decay rate has to keep it within 2x."""
    ref = _ref(name)
    phi, it = kr.pcg(ref, rtol, 1e300)
    err = ref.energy_error(phi)
    assert it > 0 and err <= 2.0 * rtol, (it, err / rtol)


def test_pcg_one_step_estimate_stops_early_on_slow_convergence():
    """The test above has teeth: the estimate csrc/krylov.hip used before (one beta, capped at 0.9) fails it."""
    ref = _ref("axon")
    phi, it = kr.pcg(ref, 1e-3, 1e300, rule="onestep")
    assert ref.energy_error(phi) > 2.0 * 1e-3, it


def test_host_norms_are_the_device_definitions():
    """krylov_ref's norms against direct numpy formulas (exact-rounding sums only change the last bits)."""
    ref = _ref("box")
    r = np.random.default_rng(3).standard_normal(ref.nc * ref.nd)
    rk2 = (r.reshape(ref.nc, ref.nd) ** 2).sum(axis=1)
    assert abs(ref.norm_w2(r) / np.sqrt((rk2 * ref.w).sum()) - 1.0) < 1e-13
    assert abs(ref.norm_d8(r) / (((np.sqrt(rk2) * ref.w) ** 8).sum()) ** 0.125 - 1.0) < 1e-13
    # the energy error is shift-invariant (constants span the null space of A_emi) and 0 at the direct solution
    phi = ref.phi_star()
    assert ref.energy_error(phi + 3.0) < 1e-6
