"""The DG-P2 kernels (csrc/apply_p2.hip, csrc/tab_rhs.hip, csrc/tab_assembled.hip) and the 2D coordinate kernels against the CPU oracle on meshes that carry
EVERY ordered pair (own local facet I, neighbour's local facet j) -- tests/p2_meshes.py; the box meshes of the other comparisons
carry 4 of 16 (5 of 9) -- through the C ABI, on seeded inputs.  Also the first runs of: the 3D coordinate-geometry P2 instantiations on
more than two cells, the assembled-blocks switch KNP_P2_ASSEMBLED=1, P2 with rho != 0, D per subdomain / per cell and one / three
solved species, partitioned P2 on an unstructured mesh, and the P2 AMG hierarchy (ConformingSpaceP2) on an unstructured mesh.

Tolerances are the ones the project uses for the same quantities (tests/test_gpu_parity.py, tests/test_gpu_solver.py): applies and
right-hand sides 1e-11 of the max norm, kappa 1e-14, phi_M 1e-13, c_elim and traces 1e-14, Nernst 1e-12; two solver steps
c <= 1e-8, mean-free phi <= 1e-6, phi_M <= 1e-6.

Worst errors observed on the MI355X (every figure is printed before its assertion; `pytest -s` shows them):
  group                              applies   right-hand sides  kappa    phi_M    c_elim / traces  Nernst
  (a) tissue P2, matrix-free         6.4e-15   1.4e-14           1.3e-16  1.5e-16  4.3e-16          4.6e-16
  (b) tissue P2, assembled blocks    5.6e-16   --                --       --       --               --
  (c) one / three species, D(cell)   8.9e-16   5.1e-15           --       --       --               --
  (d) delaunay 2D P1                 5.1e-16   4.8e-15           2.2e-16  1.9e-16  0                5.9e-16
  (d) delaunay 2D P2                 4.4e-15   1.4e-14           2.2e-16  3.5e-16  2.7e-16          6.9e-16
  (e) tissue P2, 2 parts             6.4e-15   1.7e-14           --       1.6e-16  0                4.4e-16
  (f) two solver steps: c 1.6e-10, c_elim 2.0e-10, mean-free phi 2.0e-10, phi_M 8.1e-11, Nernst 1.2e-10
  EMI symmetry |x1.A x0 - x0.A x1| / |x1.A x0| <= 2.8e-14, A 1 <= 8.2e-16 of max |A x|.
No kernel missed a bound on any pair; the slivers cost the Newton-refined reciprocal and square root of the coordinate geometry
nothing visible (the numpy formulation sits at 5.5e-15 on the same mesh)."""
import copy
import os
import sys

import numpy as np
import pytest

import knpemi_oracle as ko
import p2_meshes
from common import synthetic_state, device_for, push_state, relerr, mean_free

pytestmark = pytest.mark.gpu
TOL = 1e-11


def _err(tag, what, got, ref, bound):
    e = relerr(got, ref)
    print("%-24s %-22s %.2e  (bound %.0e)" % (tag, what, e, bound))
    assert e < bound, (tag, what, e)


_PROBLEMS = {}


def _tissue_problem():
    """tissue_piece(), DG-P2, run_tortuosity.py coefficients (rho != 0, D per subdomain, z = -1 eliminated), seeded state; with the
    oracle's operator products (assembled once, shared and left unchanged by the tests that need them)."""
    if "tissue" not in _PROBLEMS:
        mt = p2_meshes.tissue_piece()
        pb = ko.build_tortuosity(mt[0], mt[1].array(), mt[2].array(), p=2)
        x = synthetic_state(pb, volt=1.0e3)
        Aemi, _, _ = ko.assemble_emi(pb, want_B=False)
        ye = Aemi @ x[0].ravel()
        yk = [ko.assemble_knp(pb, k) @ x[k].ravel() for k in range(pb.N_ions)]
        _PROBLEMS["tissue"] = (mt, pb, x, ye, yk)
    return _PROBLEMS["tissue"]


def _check_operators_and_updates(tag, pb, dev, x, A, ye=None, yk=None):
    """kappa; EMI apply (+ symmetry, constants in the null space); KNP apply per species; both right-hand sides with and without
    splitting; step-III updates and the two update_ode traces -- the list of tests/test_gpu_parity.py, against the oracle."""
    dev.update_kappa(); dev.update_dnphi()
    _err(tag, "kappa", dev.download(A.F_KAPPA), pb.kappa(), 1e-14)
    if ye is None:
        Aemi, _, _ = ko.assemble_emi(pb, want_B=False)
        ye = Aemi @ x[0].ravel()
    dev.upload(A.F_X, x[0]); dev.emi_apply(A.F_X, A.F_Y)
    y0 = dev.download(A.F_Y, 0, pb.ndof)
    _err(tag, "emi apply", y0, ye, TOL)
    x1 = x[1].ravel()
    dev.upload(A.F_X, x[1]); dev.emi_apply(A.F_X, A.F_Y)
    y1 = dev.download(A.F_Y, 0, pb.ndof)
    s01, s10 = float(x1 @ y0), float(x[0].ravel() @ y1)
    print("%-24s %-22s %.2e  (bound 1e-10)" % (tag, "emi symmetry", abs(s01 - s10) / abs(s01)))
    assert abs(s01 - s10) < 1e-10 * abs(s01)
    dev.upload(A.F_X, np.ones(pb.ndof)); dev.emi_apply(A.F_X, A.F_Y)
    yc = dev.download(A.F_Y, 0, pb.ndof)
    print("%-24s %-22s %.2e  (bound 1e-09)" % (tag, "emi constants", np.abs(yc).max() / np.abs(y0).max()))
    assert np.abs(yc).max() < 1e-9 * np.abs(y0).max()
    dev.upload(A.F_X, x); dev.knp_apply(A.F_X, A.F_Y)
    y = dev.download(A.F_Y).reshape(pb.N_ions, -1)
    for k in range(pb.N_ions):
        _err(tag, "knp apply[%d]" % k, y[k], yk[k] if yk is not None else ko.assemble_knp(pb, k) @ x[k].ravel(), TOL)
    z = [ion["z"] for ion in pb.ions]
    D = np.stack([ion["D"] for ion in pb.ions])
    try:
        for splitting in (False, True):
            pb.splitting = splitting
            dev.set_params(pb.C_M, pb.dt, pb.F, pb.R, pb.T, pb.C_phi, pb.tau, pb.tau, z, D, rho=pb.rho, splitting=splitting)
            dev.emi_rhs(); dev.knp_rhs()
            _err(tag, "emi rhs split=%d" % splitting, dev.download(A.F_B_EMI), ko.emi_rhs(pb), TOL)
            b = dev.download(A.F_B_KNP).reshape(pb.N_ions, -1)
            for k in range(pb.N_ions):
                _err(tag, "knp rhs[%d] split=%d" % (k, splitting), b[k], ko.knp_rhs(pb, k), TOL)
    finally:
        pb.splitting = True
        dev.set_params(pb.C_M, pb.dt, pb.F, pb.R, pb.T, pb.C_phi, pb.tau, pb.tau, z, D, rho=pb.rho, splitting=True)
    K_e = dev.facet_trace(A.F_C, 0, 0)
    _err(tag, "trace plus", K_e[pb.mem], ko.facet_average(pb, pb.mem, lambda plus, minus: plus(pb.c[0]), pb.p), 1e-14)
    X_i = dev.facet_trace(A.F_C_ELIM, 0, 1)
    _err(tag, "trace minus", X_i[pb.mem], ko.facet_average(pb, pb.mem, lambda plus, minus: minus(pb.c_elim), pb.p), 1e-14)
    q = copy.deepcopy(pb)                                  # the oracle's updates write into the problem; pb stays as seeded
    dev.step_updates()
    _err(tag, "phi_M", dev.download(A.F_PHI_M)[pb.mem], ko.update_phi_M(q).copy(), 1e-13)
    _err(tag, "c_elim", dev.download(A.F_C_ELIM), ko.update_c_elim(q), 1e-14)
    E = dev.download(A.F_E).reshape(len(pb.ions), -1)
    for k in range(len(pb.ions)):
        _err(tag, "nernst[%d]" % k, E[k][pb.mem], ko.nernst(q, k), 1e-12)


def test_tissue_piece_p2_vs_oracle(hip_lib):
    """(a) every DG-P2 kernel of the coordinate-geometry path on all 16 (I, j) pairs -- SIPG facets, both membrane tags -- with the
    tortuosity coefficients.  The block condition makes BOTH branches of load_frame (LDS for a neighbour inside the cell's 256-cell
    block, global gather otherwise) carry every permutation: checked here from the device-order neighbour table."""
    from knpemidg import _abi as A
    import connectivity as oc
    mt, pb, x, ye, yk = _tissue_problem()
    dev = device_for(pb)
    try:
        assert dev.n_geometry_classes == 0 and dev.apply_variant(0) == 8 and dev.apply_variant(1) == 8
        nc = pb.mesh.num_cells()
        nbr = dev.debug_table(A.DT_NBR).reshape(nc, 4).astype(np.int64)
        flag = dev.debug_table(A.DT_FLAG)
        fb = ((flag[:, None] >> (8 * np.arange(4, dtype=np.uint32))[None, :]) & 0xFF).astype(np.int64)
        sipg = ((fb >> 2) & 3) == oc.K_SIPG
        same = (nbr // 256) == (np.arange(nc) // 256)[:, None]
        own = np.broadcast_to(np.arange(4), (nc, 4))
        inside = set(zip(own[sipg & same].tolist(), (fb & 3)[sipg & same].tolist()))
        outside = set(zip(own[sipg & ~same].tolist(), (fb & 3)[sipg & ~same].tolist()))
        allp = {(i, j) for i in range(4) for j in range(4)}
        assert inside == allp and outside == allp, (sorted(allp - inside), sorted(allp - outside))
        assert nc % 256 != 0                               # a short last block
        push_state(dev, pb)
        _check_operators_and_updates("tissue P2", pb, dev, x, A, ye, yk)
    finally:
        dev.close()


def test_tissue_piece_p2_assembled_blocks_vs_oracle(hip_lib, monkeypatch):
    """(b) the same mesh and state through the quadrature-assembled cell blocks (KNP_P2_ASSEMBLED=1 when the context is created:
    k_tab_assemble_*, k_tab_apply): the documented A/B switch of the matrix-free applies; same forms, rules that match the oracle's."""
    from knpemidg import _abi as A
    mt, pb, x, ye, yk = _tissue_problem()
    monkeypatch.setenv("KNP_P2_ASSEMBLED", "1")
    dev = device_for(pb)
    try:
        assert dev.apply_variant(0) == 9 and dev.apply_variant(1) == 9
        monkeypatch.delenv("KNP_P2_ASSEMBLED")             # the choice belongs to the context, not to the environment of later calls
        assert dev.apply_variant(0) == 9
        push_state(dev, pb)
        dev.update_kappa(); dev.update_dnphi()
        dev.upload(A.F_X, x[0]); dev.emi_apply(A.F_X, A.F_Y)
        _err("tissue P2 assembled", "emi apply", dev.download(A.F_Y, 0, pb.ndof), ye, TOL)
        dev.upload(A.F_X, x); dev.knp_apply(A.F_X, A.F_Y)
        y = dev.download(A.F_Y).reshape(pb.N_ions, -1)
        for k in range(pb.N_ions):
            _err("tissue P2 assembled", "knp apply[%d]" % k, y[k], yk[k], TOL)
    finally:
        dev.close()
    other = device_for(pb)                                 # and a context created without the switch runs the matrix-free applies
    try:
        assert other.apply_variant(0) == 8 and other.apply_variant(1) == 8
        push_state(other, pb)
        other.update_dnphi()
        other.upload(A.F_X, x); other.knp_apply(A.F_X, A.F_Y)
        ymf = other.download(A.F_Y).reshape(pb.N_ions, -1)
        # two different kernels produced the two results: equal to rounding, not bit for bit
        assert not np.array_equal(ymf, y) and relerr(ymf, y) < TOL
    finally:
        other.close()


@pytest.mark.parametrize("which", ["one_species", "three_species", "cellwise_D"])
def test_tissue_piece_p2_species_counts_and_cellwise_diffusion(hip_lib, which):
    """(c) blockIdx.y = species and KnpP2Args::z[] with one and three solved species (valences +1, -1, +1, +2), and a diffusion
    coefficient that differs from cell to cell: KNP apply and right-hand side per species."""
    from knpemidg import _abi as A
    m, s, f = p2_meshes.tissue_piece()
    tags = s.array().astype(np.int64)
    if which == "cellwise_D":
        pb = ko.build_tortuosity(m, tags, f.array(), p=2)
        rng = np.random.default_rng(5)
        for ion in pb.ions:
            ion["D"] = np.asarray(ion["D"], dtype=float) * rng.uniform(0.5, 1.5, size=len(tags))
    else:
        names = ("K", "Cl") if which == "one_species" else ("K", "Cl", "Na", "Ca")
        P = ko.emix_params()
        nc = m.num_cells()
        z = dict(P["z"], Ca=2.0)
        Dc = dict(P["D"], Ca=0.8e-8)
        ions = [dict(name=n, z=z[n], D=np.full(nc, Dc[n]) * np.array([1.0, 0.5, 0.25])[tags]) for n in names]
        pb = ko.Problem(m, tags, f.array(), 2, ions, P, membrane_tags=(1, 2))
        rng = np.random.default_rng(11)
        pb.c = rng.uniform(50.0, 150.0, size=pb.c.shape)
        pb.c_prev_n = pb.c.copy()
        pb.c_elim = rng.uniform(50.0, 150.0, size=pb.c_elim.shape)
    x = synthetic_state(pb, volt=1.0e3)
    dev = device_for(pb)
    try:
        push_state(dev, pb)
        assert dev.n_geometry_classes == 0 and dev.apply_variant(1) == 8
        dev.update_kappa(); dev.update_dnphi()
        dev.upload(A.F_X, x); dev.knp_apply(A.F_X, A.F_Y)
        y = dev.download(A.F_Y).reshape(pb.N_ions, -1)
        dev.knp_rhs()
        b = dev.download(A.F_B_KNP).reshape(pb.N_ions, -1)
        for k in range(pb.N_ions):
            _err("tissue P2 " + which, "knp apply[%d]" % k, y[k], ko.assemble_knp(pb, k) @ x[k].ravel(), TOL)
            _err("tissue P2 " + which, "knp rhs[%d]" % k, b[k], ko.knp_rhs(pb, k), TOL)
    finally:
        dev.close()


@pytest.mark.parametrize("p", [1, 2])
def test_delaunay_2d_vs_oracle(hip_lib, p):
    """(d) the 2D coordinate kernels of both degrees on all 9 (I, j) pairs, SIPG and membrane facets: the list of (a)."""
    from knpemidg import _abi as A
    m, s, f = p2_meshes.delaunay_2d()
    pb = ko.build_idealized(m, s.array(), f.array(), p=p, membrane_tags=(1,))
    x = synthetic_state(pb)
    dev = device_for(pb)
    try:
        assert dev.n_geometry_classes == 0
        push_state(dev, pb)
        _check_operators_and_updates("delaunay 2D P%d" % p, pb, dev, x, A)
    finally:
        dev.close()


def test_tissue_piece_p2_partitioned_on_one_gpu(hip_lib, monkeypatch):
    """(e) owned + ghost sub-meshes of tissue_piece() (recursive coordinate bisection, 2 parts; one context per rank on this GPU,
    ghosts filled from the global arrays): owned rows of both applies in one launch and as interior + boundary launches, both
    right-hand sides and the step updates against the GLOBAL oracle results -- test_partitioned_kernels_on_one_gpu on the
    unstructured P2 path."""
    from knpemidg import _abi as A
    from knpemidg.partition import Partition
    (m, s, f), pbg, x, ye, yk_ = _tissue_problem()
    yg = ye.reshape(-1, pbg.nd)
    yk = np.stack([v.reshape(-1, pbg.nd) for v in yk_])
    bg = ko.emi_rhs(pbg)
    bk = np.stack([ko.knp_rhs(pbg, k).reshape(-1, pbg.nd) for k in range(pbg.N_ions)])
    q = copy.deepcopy(pbg)
    ko.update_phi_M(q); ko.update_c_elim(q)
    Eg = np.stack([ko.nernst(q, k) for k in range(3)])
    part = Partition(m, 2, method="rcb")
    for rank in range(2):
        tag = "tissue P2 rank %d/2" % rank
        loc = part.local(rank)
        sub_l, surf_l = loc.localize(s, f, (1, 2))
        pbl = ko.build_tortuosity(loc.mesh, sub_l.array(), surf_l.array(), p=2)
        cg, no = loc.cells_global, loc.nc_owned
        pbl.c, pbl.c_prev_n, pbl.c_elim, pbl.phi = pbg.c[:, cg], pbg.c_prev_n[:, cg], pbg.c_elim[cg], pbg.phi[cg]
        pbl.phi_M = pbg.phi_M[loc.facets_global]
        for name in pbg.I_ch:
            pbl.I_ch[name] = pbg.I_ch[name][loc.facets_global]
        dev = device_for(pbl, nc_owned=no)
        try:
            assert 0 < dev.n_interior < no and dev.n_geometry_classes == 0
            push_state(dev, pbl)
            dev.update_kappa(); dev.update_dnphi()
            for split in ("0", "1"):                          # one launch / interior + boundary launches (the overlapped form)
                monkeypatch.setenv("KNP_FORCE_SPLIT", split)
                dev.upload(A.F_Y, np.zeros(dev.size(A.F_Y)))
                dev.upload(A.F_X, x[0][cg]); dev.emi_apply(A.F_X, A.F_Y)
                y = dev.download(A.F_Y, 0, pbl.ndof).reshape(-1, pbl.nd)
                _err(tag, "emi apply split=" + split, y[:no], yg[cg[:no]], TOL)
                dev.upload(A.F_X, x[:, cg]); dev.knp_apply(A.F_X, A.F_Y)
                y = dev.download(A.F_Y).reshape(pbg.N_ions, -1, pbl.nd)
                _err(tag, "knp apply split=" + split, y[:, :no], yk[:, cg[:no]], TOL)
            monkeypatch.delenv("KNP_FORCE_SPLIT")
            dev.emi_rhs(); dev.knp_rhs()
            _err(tag, "emi rhs", dev.download(A.F_B_EMI).reshape(-1, pbl.nd)[:no], bg.reshape(-1, pbg.nd)[cg[:no]], TOL)
            _err(tag, "knp rhs", dev.download(A.F_B_KNP).reshape(pbg.N_ions, -1, pbl.nd)[:, :no], bk[:, cg[:no]], TOL)
            dev.step_updates()
            lmem = pbl.mem                                    # local membrane facets touching an owned cell
            gmem = loc.facets_global[lmem]
            pos = np.searchsorted(pbg.mem, gmem)
            _err(tag, "phi_M", dev.download(A.F_PHI_M)[lmem], q.phi_M[gmem], 1e-13)
            _err(tag, "nernst", dev.download(A.F_E).reshape(3, -1)[:, lmem], Eg[:, pos], 1e-12)
            _err(tag, "c_elim", dev.download(A.F_C_ELIM).reshape(-1, pbl.nd), q.c_elim[cg], 1e-14)
        finally:
            dev.close()


def test_tissue_piece_p2_two_solver_steps_vs_oracle(hip_lib):
    """(f) two full splitting steps of `Solver(degree_emi=2, degree_knp=2)` with the run_tortuosity.py configuration on tissue_piece()
    against the oracle's assembled forms and direct solves fed with the same membrane outputs -- as
    test_rho_sub_and_subdomain_diffusion_two_steps_vs_oracle, with its tight solver tolerances and its bounds.  First run of
    amg.ConformingSpaceP2, the P2 hierarchy build and k_p2_blockjacobi<3, ...> on an unstructured mesh."""
    from collections import namedtuple
    ex = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples", "emix_simulations")
    if ex not in sys.path:
        sys.path.insert(0, ex)
    import emix_common as E
    from knpemidg.models import mm_glial, mm_hh_emix
    P = ko.tortuosity_params()
    C = E.Constant
    params = namedtuple('params', ('dt', 'n_steps_ODE', 'F', 'psi', 'C_phi', 'C_M', 'R', 'temperature', 'phi_M_init_type', 'rho_sub'))(
        P["dt"], 25, P["F"], P["F"] / (P["R"] * P["temperature"]), P["C_phi"], P["C_M"], P["R"], P["temperature"], 'constant',
        {s: C(P["rho"][s]) for s in range(3)})

    def ion(name):
        return {'c_init_sub': {s: C(P["init"][name][s]) for s in range(3)}, 'c_init_sub_type': 'constant', 'bdry': C(0),
                'z': P["z"][name], 'name': name, 'D_sub': {s: C(P["D"][name] / P["lam"][s] ** 2) for s in range(3)}, 'f_source': C(0)}
    ion_list = [ion('K'), ion('Na'), ion('Cl')]
    stim = namedtuple('membrane_params', ('g_syn_bar', 'stimulus', 'stimulus_locator'))(5, {'stim_amplitude': 5}, lambda x: (x[0] < 3.5e-4))
    mt = p2_meshes.tissue_piece()
    S = E.SolverEMIx(params, ion_list, degree_emi=2, degree_knp=2)
    S.verbose = False
    S.setup_domain(*mt)
    S.setup_parameters()
    S.setup_FEM_spaces()
    S.setup_membrane_model(stim, {1: mm_glial, 2: mm_hh_emix})
    S._unpack_solver_params(E.solver_parameters()._replace(rtol_emi=1e-11, rtol_knp=1e-13))
    S.save_fields = S.save_solver_stats = False
    S.splitting_scheme = True
    S.setup_varform_emi(); S.setup_varform_knp(); S.setup_solver_emi(); S.setup_solver_knp()
    try:
        assert S.dev.n_geometry_classes == 0 and S.dev.degree == 2
        pb = ko.build_tortuosity(mt[0], mt[1].array(), mt[2].array(), p=2)
        assert relerr(S.c.array(), pb.c) < 1e-15 and relerr(S.ion_list[-1]['c'].array(), pb.c_elim) < 1e-15
        vol = pb.geom.vol
        t = E.Constant(0.0)
        for k in range(2):
            tag = "tissue P2 solver step %d" % k
            S.step_membrane_models(k)
            pb.phi_M = S.phi_M_prev_PDE.array().copy()
            for name in pb.I_ch:
                pb.I_ch[name] = np.zeros(pb.mesh.num_facets())
                for mm in S.mem_models:
                    a = mm['I_ch_k'][name].array()
                    pb.I_ch[name][mm['ode'].indices] = a[mm['ode'].indices]
            S.solve_for_time_step(k, t)
            Eo = ko.solve_for_time_step(pb, direct=True)
            _err(tag, "phi (mean-free)", mean_free(S.phi.array(), vol), mean_free(pb.phi, vol), 1e-6)
            _err(tag, "c", S.c.array(), pb.c, 1e-8)
            _err(tag, "c_elim", S.ion_list[-1]['c'].array(), pb.c_elim, 1e-8)
            _err(tag, "phi_M", S.phi_M_prev_PDE.array()[pb.mem], pb.phi_M[pb.mem], 1e-6)
            for ion_ in S.ion_list:
                _err(tag, "nernst " + ion_['name'], ion_['E'].array()[pb.mem], Eo[ion_['name']], 1e-7)
    finally:
        S.dev.close()
