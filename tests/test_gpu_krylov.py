"""Stopping tests of the device Krylov solves (csrc/krylov.hip, contracts in include/knpemi_hip.h: knp_emi_solve / knp_knp_solve)
against host-recomputed residuals and energy errors (tests/krylov_ref.py): the numbers a solve reports (res, niter) and the vector it
returns, at the tolerances the stops are used with, not only far below them."""
import os
import sys

import numpy as np
import pytest

import knpemi_oracle as ko
import krylov_ref as kr
from common import synthetic_state, device_for, push_state, small_3d

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples", "idealized_geometries"))

PROBLEMS = ["2D_P1", "axon_P1", "2D_P2", "box_P2", "emix_sub", "tissue_P2"]


def _problem(name):
    from knpemidg.mesh import make_mesh_2D, make_mesh_3D
    volt = 1.0
    if name == "2D_P1":
        m, s, f = make_mesh_2D(0); pb = ko.build_idealized(m, s.array(), f.array(), membrane_tags=(1,))
    elif name == "axon_P1":
        m, s, f = make_mesh_3D(0, n_axons=1); pb = ko.build_idealized(m, s.array(), f.array(), membrane_tags=(1,))
    elif name == "box_P1":
        m, s, f = small_3d(); pb = ko.build_idealized(m, s.array(), f.array(), membrane_tags=(1,))
    elif name == "2D_P2":
        m, s, f = make_mesh_2D(0); pb = ko.build_idealized(m, s.array(), f.array(), p=2, membrane_tags=(1,))
    elif name == "box_P2":
        m, s, f = small_3d((6, 3, 3)); pb = ko.build_idealized(m, s.array(), f.array(), p=2, membrane_tags=(1,))
    elif name == "tissue_P2":               # all 16 (own facet, neighbour facet) pairs, no geometry classes: the P2 block-Jacobi inverses on them
        import p2_meshes
        m, s, f = p2_meshes.tissue_piece(); pb = ko.build_tortuosity(m, s.array(), f.array(), p=2)
        volt = 1.0e3
    else:                                   # sliver cells: fp32 weights and 8th powers of the density norm matter
        import emix_sub
        m, s, f = emix_sub.emix_submesh(); pb = ko.build_tortuosity(m, s.array(), f.array())
        volt = 1.0e3                        # cm / ms / mV units
    synthetic_state(pb, volt=volt)
    return pb, (m, s, f)


class Case:
    def __init__(self, name):
        from knpemidg import _abi as A
        self.A, self.name = A, name
        self.pb, self.mt = _problem(name)
        self.phi0 = self.pb.phi.ravel().copy()
        self.ref = kr.Ref(self.pb)
        self.dev = device_for(self.pb)
        push_state(self.dev, self.pb)
        self.dev.update_kappa()
        self.dev.emi_rhs()
        self.b = self.dev.download(A.F_B_EMI)
        self.star = self.ref.solve_emi(self.b)

    def emi(self, rtol, r_abs, x0, **kw):
        self.dev.emi_residual_target(r_abs)
        self.dev.upload(self.A.F_PHI, x0)                  # also drops the extrapolation history: the solve starts from x0
        niter, res = self.dev.emi_solve(rtol, maxit=20000, **kw)
        return niter, res, self.dev.download(self.A.F_PHI)

    def upload_amg(self):
        from knpemidg import amg
        m, s, f = self.mt
        tags = f.array()
        mem = sorted({int(t) for t in np.unique(tags[self.pb.mem])})
        cs = amg.ConformingSpace(m, tags, mem)
        cs2 = amg.ConformingSpaceP2(cs) if self.pb.p != 1 else None
        levels = amg.build_emi_levels(cs, cs2, tags, mem, self.pb.kappa(), self.pb.C_phi)
        self.dev.amg_upload(0, (cs2 or cs).dof, levels)


_CASES = {}


@pytest.fixture(scope="module", autouse=True)
def _close_devices():
    yield
    for c in _CASES.values():
        c.dev.close()
    _CASES.clear()


def _case(name):
    if name not in _CASES:
        _CASES[name] = Case(name)
    return _CASES[name]


@pytest.fixture(params=PROBLEMS)
def case(request, hip_lib):
    return _case(request.param)


def _rel(a, b):
    return abs(a / b - 1.0)


# ---- EMI PCG ------------------------------------------------------------------------------------------------------------------------
def test_emi_petsc_test_reports_host_norms(case):
    """r_abs = 0: PETSc's test on the preconditioned norm; res = {||M^-1 r0||, ||M^-1 r||, ||M^-1 b||} with M = the fp32 cell blocks."""
    c, ref = case, case.ref
    niter, res, phi = c.emi(1e-6, 0.0, c.phi0)
    binv = ref.binv_emi
    r0 = c.b - ref.A_emi @ c.phi0
    assert _rel(res[0], ref.norm_pc(binv, r0)) < 1e-6 and _rel(res[2], ref.norm_pc(binv, c.b)) < 1e-6, res
    true = ref.norm_pc(binv, c.b - ref.A_emi @ phi)
    assert true <= 1.05 * 1e-6 * ref.norm_pc(binv, c.b), (niter, true / res[2])


def test_emi_residual_target_is_met_by_the_true_residual(case):
    """(i): ||(b - A phi) / vol||_8 <= r_abs for the RETURNED phi (the device tests its recursively updated r)."""
    c, ref = case, case.ref
    rn0 = ref.norm_d8(c.b - ref.A_emi @ c.phi0)
    r_abs = 1e-3 * rn0
    niter, res, phi = c.emi(0.5, r_abs, c.phi0)
    c.dev.emi_residual_target(0.0)
    assert _rel(res[0], rn0) < 1e-6, (res, rn0)
    true = ref.norm_d8(c.b - ref.A_emi @ phi)
    assert true <= r_abs * (1.0 + 1e-6), (niter, true / r_abs)


def _energy_stop(c, precond, rtol):
    """(ii) alone (r_abs = 1e300): the energy-norm error of the returned phi against a direct solve <= 2 rtol ||phi*||_A; with
    block-Jacobi only, the device's iteration count agrees with the numpy replica of its recurrence."""
    ref = c.ref
    if precond != "bj":
        c.upload_amg()
        c.dev.set_emi_dg_smoother(precond == "amg_cheb")
    try:
        niter, res, phi = c.emi(rtol, 1e300, np.zeros(c.pb.ndof))
    finally:
        c.dev.emi_residual_target(0.0)
        c.dev.set_emi_dg_smoother(None)
        if precond != "bj":
            c.dev.amg_clear(0)
    err = ref.energy_error(phi, c.star)
    assert err <= 2.0 * rtol, (precond, niter, err / rtol, res)
    if precond == "bj" and c.pb.p == 1:
        ref.b_emi = c.b
        _, n_rep = kr.pcg(ref, rtol, 1e300)
        assert abs(niter - n_rep) <= max(1, 0.02 * n_rep), (niter, n_rep)


@pytest.mark.parametrize("rtol", [1e-3, 1e-5])
@pytest.mark.parametrize("precond", ["amg_cheb", "amg_plain"])
def test_emi_energy_stop_bounds_the_true_error(case, precond, rtol):
    _energy_stop(case, precond, rtol)


# block-Jacobi alone, not on the 2D meshes: there PCG stagnates for hundreds of steps on the isolated subdomain-constant mode
# (condition ~1e8), which no estimate from the CG coefficients sees before the Krylov space holds it (the AMG variants cover them)
@pytest.mark.parametrize("rtol", [1e-3, 1e-5])
@pytest.mark.parametrize("name", ["axon_P1", "box_P2", "emix_sub"])
def test_emi_energy_stop_bounds_the_true_error_block_jacobi(hip_lib, name, rtol):
    _energy_stop(_case(name), "bj", rtol)


# ---- KNP BiCGStab / GMRES ---------------------------------------------------------------------------------------------------------
def _knp_setup(c):
    pb, A = c.pb, c.A
    pb.phi = c.star.reshape(pb.phi.shape)
    c.dev.upload(A.F_PHI, pb.phi)
    c.dev.upload(A.F_C, pb.c)
    c.dev.update_dnphi()
    c.dev.knp_rhs()
    b = c.dev.download(A.F_B_KNP).reshape(pb.N_ions, -1)
    mats = [c.ref.knp(k)[0] for k in range(pb.N_ions)]
    return b, mats


@pytest.mark.parametrize("norm2", [False, True])
@pytest.mark.parametrize("method", [("bicgstab", 30), ("gmres", 30), ("gmres", 8)])
def test_knp_stop_on_the_true_residual(case, method, norm2, monkeypatch):
    """converged when ||r / vol||_8 <= 20 rtol ||b / vol||_8 (KNP_KNP_NORM2=1: the weighted 2-norms and rtol itself), checked on the
    RETURNED c; res[:, 0] / res[:, 2] are the host's norms of r0 and b; at least min_it iterations unless the early stop fired."""
    c, ref, pb, A = case, case.ref, case.pb, case.A
    if norm2:
        monkeypatch.setenv("KNP_KNP_NORM2", "1")
    norm, fac = (ref.norm_w2, 1.0) if norm2 else (ref.norm_d8, kr.KNP_D8_FACTOR)
    b, mats = _knp_setup(c)
    c0 = pb.c.reshape(pb.N_ions, -1)
    c.dev.set_knp_krylov(*method)
    try:
        for early in ([0.0, 0.01] if method[0] == "bicgstab" else [0.0]):
            c.dev.knp_early_stop(early)
            for rtol in (1e-6, 1e-9):
                c.dev.upload(A.F_C, pb.c)
                niter, res = c.dev.knp_solve(rtol, maxit=5000, min_it=5)
                x = c.dev.download(A.F_C).reshape(pb.N_ions, -1)
                for k in range(pb.N_ions):
                    assert _rel(res[k, 0], norm(b[k] - mats[k] @ c0[k])) < 1e-6 and _rel(res[k, 2], norm(b[k])) < 1e-6, (k, res)
                    true = norm(b[k] - mats[k] @ x[k])
                    tol = fac * rtol * res[k, 2] * (1.0 + 1e-6)
                    assert true <= tol, (method, early, rtol, k, niter, true / tol)
                    if niter[k] < 5:
                        assert early > 0 and true <= early * tol, (k, niter, true / tol)
    finally:
        c.dev.knp_early_stop(0.0)
        c.dev.set_knp_krylov("bicgstab")
        c.dev.upload(A.F_C, pb.c)


# ---- bookkeeping ------------------------------------------------------------------------------------------------------------------
def test_solves_do_not_depend_on_when_the_host_looks(case):
    """Kernels enqueued past convergence are masked: fields and niter are bit-identical for check_every 1, 3, 25 and for a second
    solve from the same initial guess, whose chunks are enqueued ahead on the previous iteration count (next_chunk)."""
    c, pb, A = case, case.pb, case.A
    emi_r = c.ref.norm_d8(c.b - c.ref.A_emi @ c.phi0) * 1e-4
    out = {}
    for ce in (1, 3, 25):
        for rep in (0, 1):
            niter, _, phi = c.emi(1e-3, emi_r, c.phi0, check_every=ce)
            out[("emi", ce, rep)] = (niter, phi)
    c.dev.emi_residual_target(0.0)
    _knp_setup(c)
    for method in (("bicgstab", 30), ("gmres", 30), ("gmres", 8)):
        c.dev.set_knp_krylov(*method)
        for ce in (1, 3, 25):
            for rep in (0, 1):
                c.dev.upload(A.F_C, pb.c)
                niter, _ = c.dev.knp_solve(1e-7, maxit=5000, min_it=5, check_every=ce)
                out[(method, ce, rep)] = (list(niter), c.dev.download(A.F_C))
    c.dev.set_knp_krylov("bicgstab")
    c.dev.upload(A.F_C, pb.c)
    for kind in ["emi", ("bicgstab", 30), ("gmres", 30), ("gmres", 8)]:
        base = out[(kind, 1, 0)]
        for ce in (1, 3, 25):
            for rep in (0, 1):
                got = out[(kind, ce, rep)]
                assert got[0] == base[0] and np.array_equal(got[1], base[1]), (kind, ce, rep, got[0], base[0])


def _species_are_independent(method):
    from knpemidg import _abi as A
    out = []
    for perturb in (False, True):
        pb, _ = _problem("box_P1")
        dev = device_for(pb)
        push_state(dev, pb)
        dev.update_dnphi()
        dev.knp_rhs()
        c = pb.c.copy()
        if perturb:
            c[1] *= 1.0 + 1e-3 * np.random.default_rng(11).uniform(-1.0, 1.0, size=c[1].shape)
        dev.upload(A.F_C, c)
        dev.set_knp_krylov(*method)
        niter, _ = dev.knp_solve(1e-7, maxit=5000, min_it=5)
        out.append((niter, dev.download(A.F_C).reshape(pb.c.shape)))
        dev.close()
    assert out[0][0][0] == out[1][0][0] and np.array_equal(out[0][1][0], out[1][1][0]), (out[0][0], out[1][0])
    assert not np.array_equal(out[0][1][1], out[1][1][1])
    return out


def test_bicgstab_species_are_independent(hip_lib):
    """Batched BiCGStab: species 0's iterations and field do not depend on species 1's initial guess (separate status words, masked
    updates, per-species reductions).  The guess is set after the right-hand side: the membrane terms of every species' load depend
    on all concentrations."""
    _species_are_independent(("bicgstab", 30))


def test_gmres_species_are_independent(hip_lib):
    """The same for GMRES(8), whose species share every restart: a species whose cycle is done idles until the other's is, its
    Hessenberg matrix, rotations and column count are its own.  Restart length 8, so that several cycles run."""
    out = _species_are_independent(("gmres", 8))
    assert max(out[0][0]) > 8, out[0][0]
