"""Per-step overhead changes that must not change a single bit: the status-poll rule of the Krylov loops past the predicted iteration
count (KNP_POLL_TAIL), BiCGStab's first iteration without the zero vectors p = v = 0 (KNP_FUSE_BI_FIRST) and the extrapolated initial
guess without the unread second history entry (KNP_FUSE_EXTRAP).  Each against its old path on three stimulated steps of the 4-axon
mesh with its AMG hierarchies (PCG for EMI; BiCGStab and GMRES for KNP): iteration counts and fields bitwise equal."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples", "idealized_geometries"))


def _three_steps(krylov):
    from idealized_common import make_solver, solver_parameters, Constant
    S = make_solver(dim=3, resolution=0, n_axons=4)
    S._unpack_solver_params(solver_parameters(3, 0))
    S.save_fields = S.save_solver_stats = False
    S.splitting_scheme = True
    S.setup_varform_emi(); S.setup_varform_knp(); S.setup_solver_emi(); S.setup_solver_knp()
    S.dev.set_knp_krylov(krylov)
    assert S.use_amg
    t = Constant(0.0)
    for k in range(3):
        S.step_membrane_models(k)
        S.solve_for_time_step(k, t)
    out = (S.phi.array().copy(), S.c.array().copy(), list(S.emi_niter), [list(n) for n in S.knp_niter])
    S.dev.close()
    return out


@pytest.mark.parametrize("switch,old", [("KNP_POLL_TAIL", "0"), ("KNP_FUSE_BI_FIRST", "0"), ("KNP_FUSE_EXTRAP", "0")])
def test_step_overhead_switches_are_bitwise(hip_lib, monkeypatch, switch, old):
    monkeypatch.setenv("KNP_AMG_MAXCOARSE", "300")
    for krylov in ("bicgstab", "gmres"):
        monkeypatch.delenv(switch, raising=False)
        a = _three_steps(krylov)
        monkeypatch.setenv(switch, old)
        b = _three_steps(krylov)
        assert a[2] == b[2] and a[3] == b[3], (krylov, a[2:], b[2:])
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), krylov


@pytest.mark.parametrize("name", ["3D_4axon_r0", "3D_4axon_r0_rho"])
def test_rhs_class_path_matches_coordinate_path(hip_lib, monkeypatch, name):
    """k_emi_rhs / k_knp_rhs with the cell geometry from the class records (default on meshes with classes) against the coordinate path
    (KNP_RHS_CLS=0) on the structured 4-axon mesh and on its run_tortuosity.py variant (rho_sub != 0, three materials, z = -1 eliminated),
    both splitting modes: equal to rounding, and both equal to the oracle's assembled right-hand sides."""
    import knpemi_oracle as ko
    from knpemidg import _abi as A
    from common import synthetic_state, device_for, push_state, relerr
    from knpemidg.mesh import make_mesh_3D
    if name == "3D_4axon_r0":
        m, s, f = make_mesh_3D(0)
        pb = ko.build_idealized(m, s.array(), f.array())
    else:
        from common import tortuosity_3d
        pb = tortuosity_3d(0)
    synthetic_state(pb, volt=1.0e3 if name.endswith("_rho") else 1.0)
    dev = device_for(pb)
    try:
        assert dev.n_geometry_classes > 0
        push_state(dev, pb)
        dev.update_kappa(); dev.update_dnphi()
        z = [ion["z"] for ion in pb.ions]
        D = np.stack([ion["D"] for ion in pb.ions])
        for splitting in (True, False):
            pb.splitting = splitting
            dev.set_params(pb.C_M, pb.dt, pb.F, pb.R, pb.T, pb.C_phi, pb.tau, pb.tau, z, D, rho=pb.rho, splitting=splitting)
            out = {}
            for flag in ("1", "0"):
                monkeypatch.setenv("KNP_RHS_CLS", flag)
                dev.emi_rhs(); dev.knp_rhs()
                out[flag] = (dev.download(A.F_B_EMI).copy(), dev.download(A.F_B_KNP).copy())
            assert relerr(out["1"][0], out["0"][0]) < 1e-12, splitting
            assert relerr(out["1"][1], out["0"][1]) < 1e-12, splitting
            assert relerr(out["1"][0], ko.emi_rhs(pb)) < 1e-11
            bk = out["1"][1].reshape(pb.N_ions, -1)
            for k in range(pb.N_ions):
                assert relerr(bk[k], ko.knp_rhs(pb, k)) < 1e-11
    finally:
        pb.splitting = True
        dev.close()
