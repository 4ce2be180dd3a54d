"""Manufactured-solution (MMS, splitting == 2) right-hand sides: what the host and the device tests share.

`StubMMS` stands where the oracle expects `pb.mms` (oracle/knpemi_oracle.py: emi_rhs / knp_rhs skip their own membrane terms and call
`add_emi_rhs` / `add_knp_rhs`) and states in numpy what the device forms in MMS mode from the tables of `Device.set_mms`: L_emi gets
the data term `e_emi`; L_knp of species k gets `e_knp[k]` and the solution-dependent term -(phi_i - phi_e)(C_i v_i - C_e v_e)
(reference: src/knpemidg/solver.py:649-650) with the DG0 coefficient C[k], integrated over the membrane facets with a rule of degree
2p (exact: phi and v are of degree p on a facet).  Works in any dimension and degree, on any mesh.

The mutants (`StubMMS(..., mutation=...)`) are the ways a kernel can form that term subtly wrong; tests/test_mms_cases_host.py shows
that the seeded inputs below tell every one of them from the right term, so a device test at 1e-11 on these inputs does too."""
import numpy as np

import knpemi_oracle as ko
import mms as omms
from common import synthetic_state, small_3d

MUTATIONS = ("sign", "across", "species", "factor")


class StubMMS:
    """C [n_sys, nc], e_emi [nc, nd], e_knp [n_sys, nc, nd]; deg: facet rule of the jump term (default 2p).
    mutation: None, or one of MUTATIONS -- "sign": the term with the opposite sign; "across": C of the cell behind the facet;
    "species": C of the next solved species; "factor": the P1 facet mass matrix with 1/6 for 1/12 in 3D (and 1/12 for 1/6 in 2D)."""

    def __init__(self, C, e_emi, e_knp, deg=None, mutation=None):
        self.C = np.asarray(C, dtype=np.float64)
        self.e_emi = np.asarray(e_emi, dtype=np.float64)
        self.e_knp = np.asarray(e_knp, dtype=np.float64)
        self.deg = deg
        assert mutation is None or mutation in MUTATIONS
        self.mutation = mutation

    def add_emi_rhs(self, pb, b):
        b += self.e_emi.reshape(b.shape)

    def jump_term(self, pb, idx):
        """[nc, nd]: the solution-dependent term of L_knp for solved species idx."""
        out = np.zeros((pb.mesh.num_cells(), pb.nd))
        fm = pb.mem
        if not len(fm):
            return out
        deg = 2 * pb.p if self.deg is None else self.deg
        m = self.mutation
        C = self.C[(idx + 1) % len(self.C)] if m == "species" else self.C[idx]
        scale = 1.0
        if m == "sign":
            scale = -1.0
        elif m == "factor":
            scale = 2.0 if pb.d == 3 else 0.5
        es = pb.e_side[fm].astype(np.int64)
        sides = [ko.FacetSide(pb.space, fm, 0, deg), ko.FacetSide(pb.space, fm, 1, deg)]
        ph = [sd.val(pb.phi) for sd in sides]
        wqf = sides[0].w[None, :] * pb.geom.farea[fm][:, None]
        for side, sd in enumerate(sides):
            is_e = (es == side)[:, None]
            dphi = np.where(is_e, ph[1 - side] - ph[side], ph[side] - ph[1 - side])          # phi_i - phi_e
            Cown = C[sides[1 - side].cells] if m == "across" else C[sd.cells]
            coef = scale * np.where(is_e, 1.0, -1.0) * Cown[:, None] * dphi                  # + C_e dphi v_e - C_i dphi v_i
            np.add.at(out, sd.cells, np.einsum("fq,fq,fqv->fv", wqf, coef, sd.B))
        return out

    def add_knp_rhs(self, pb, idx, b):
        b += self.e_knp[idx].reshape(b.shape)
        b += self.jump_term(pb, idx)


def closed_form_jump(pb, C):
    """The same term for P1 written out by hand, with no tabulation and no quadrature: on a facet with vertices v_1..v_d the exact P1
    facet mass matrix is |F| / (d (d + 1)) (1 + delta_mn), so the row of vertex v_m gets
    s C[cell] |F| / (d (d + 1)) (sum_n dphi_n + dphi_m), dphi_n = (phi_i - phi_e)(v_n), s = +1 on the e side and -1 on the i side
    (|F| / 6 in 2D, |F| / 12 in 3D).  P1 nodal value a of a cell sits at the cell's a-th vertex.  Returns [nc, nd]."""
    assert pb.p == 1
    mesh, d = pb.mesh, pb.d
    out = np.zeros((mesh.num_cells(), pb.nd))
    for f in pb.mem:
        verts = mesh.facets[f]
        cells = [int(c) for c in mesh.facet_cells[f]]
        e = int(pb.e_side[f])
        loc = [[int(np.nonzero(mesh.cells[c] == v)[0][0]) for v in verts] for c in cells]      # [side][m] -> local node of v_m
        phi_e = np.array([pb.phi[cells[e], a] for a in loc[e]])
        phi_i = np.array([pb.phi[cells[1 - e], a] for a in loc[1 - e]])
        dphi = phi_i - phi_e
        w = pb.geom.farea[f] / (d * (d + 1.0))
        for side in (0, 1):
            s = 1.0 if side == e else -1.0
            for mm, a in enumerate(loc[side]):
                out[cells[side], a] += s * C[cells[side]] * w * (dphi.sum() + dphi[mm])
    return out


# ------------------------------------------------------------------------------------------------------------------------------
# problems and seeded inputs
# ------------------------------------------------------------------------------------------------------------------------------
def problem(name):
    """(pb, volt).  The names of tests/test_gpu_parity.py come from its builder; "emix_sub" is the 17 920-tet piece of the tissue
    reconstruction with the EMIx coefficients (mV: volt = 1e3), as in test_unstructured_apply_kernel_variants; "box_P1" is a small
    structured 3D box; the meshes of tests/p2_meshes.py carry every pairing of local facet indices on their membrane facets (box
    meshes carry one pairing in 2D and two in 3D there, and in 2D the two indices are equal: a kernel that took the neighbour's
    trace through the OWN facet's tabulation would pass on them)."""
    if name == "emix_sub":
        import emix_sub
        m, s, f = emix_sub.emix_submesh()
        return ko.build_emix(m, s.array(), f.array()), 1.0e3
    if name in ("delaunay_2d", "delaunay_2d_P2"):          # every (own local facet, neighbour's local facet) pair on the membrane
        import p2_meshes
        m, s, f = p2_meshes.delaunay_2d()
        return ko.build_idealized(m, s.array(), f.array(), p=2 if name.endswith("P2") else 1, membrane_tags=(1,)), 1.0
    if name == "tissue_piece_P2":                          # the same in 3D: 16 of 16 pairs on both membrane tags
        import p2_meshes
        m, s, f = p2_meshes.tissue_piece()
        return ko.build_tortuosity(m, s.array(), f.array(), p=2), 1.0e3
    if name == "box_P1":
        m, s, f = small_3d((8, 4, 4))
        return ko.build_idealized(m, s.array(), f.array(), membrane_tags=(1,)), 1.0
    from test_gpu_parity import _problem
    return _problem(name), 1.0


def species_problem(names):
    """The single-axon r=0 mesh with another ion list (the last one eliminated): the lists of
    test_knp_apply_with_one_and_three_solved_species."""
    from knpemidg.mesh import make_mesh_3D
    m, s, f = make_mesh_3D(0, n_axons=1)
    P = ko.idealized_params()
    nc = m.num_cells()
    z = dict(P["z"], Ca=2.0)
    Dc = dict(P["D"], Ca=0.8e-9)
    ions = [dict(name=n, z=z[n], D=np.full(nc, Dc[n])) for n in names]
    pb = ko.Problem(m, s.array().astype(np.int64), f.array(), 1, ions, P, membrane_tags=(1, 2))
    rng = np.random.default_rng(11)
    pb.c = rng.uniform(50.0, 150.0, size=pb.c.shape)
    pb.c_prev_n = pb.c.copy()
    pb.c_elim = rng.uniform(50.0, 150.0, size=pb.c_elim.shape)
    return pb


def seed_inputs(pb, volt=1.0, seed=0, c_prev_zero=True):
    """The inputs of the kernel-level cases: state from `synthetic_state` (phi ~ 0.07 volt U(-1, 1) per node: its jump across the
    membrane is of the size of phi itself), C ~ U(0.5, 4) per cell and species, and C_PREV = 0, so that L_knp holds nothing but the
    MMS terms and a tolerance relative to its max norm bites on them.  Returns C [n_sys, nc]."""
    synthetic_state(pb, seed=seed, volt=volt)
    if c_prev_zero:
        pb.c_prev_n = np.zeros_like(pb.c)
    return np.random.default_rng(seed + 40).uniform(0.5, 4.0, size=(pb.N_ions, pb.mesh.num_cells()))


def zero_extras(pb):
    nc, nd = pb.mesh.num_cells(), pb.nd
    return np.zeros((nc, nd)), np.zeros((pb.N_ions, nc, nd))


def random_extras(pb, C, seed=0):
    """e_emi, e_knp ~ U(-1, 1) per degree of freedom, scaled to the max norm of the jump term of the state in `pb` (e_emi: to that of
    L_emi without data terms), so that neither swamps the other."""
    nc, nd = pb.mesh.num_cells(), pb.nd
    rng = np.random.default_rng(seed + 50)
    stub = StubMMS(C, *zero_extras(pb))
    jmax = max(np.abs(stub.jump_term(pb, k)).max() for k in range(pb.N_ions))
    old = pb.mms
    pb.mms = stub
    try:
        emax = np.abs(ko.emi_rhs(pb)).max()
    finally:
        pb.mms = old
    return emax * rng.uniform(-1, 1, size=(nc, nd)), jmax * rng.uniform(-1, 1, size=(pb.N_ions, nc, nd))


def membrane_cells(pb):
    """bool [nc]: cells with at least one membrane facet"""
    has = np.zeros(pb.mesh.num_cells(), dtype=bool)
    fc = pb.mesh.facet_cells[pb.mem]
    has[fc[:, 0]] = True
    has[fc[:, 1]] = True
    return has


# ------------------------------------------------------------------------------------------------------------------------------
# the reference's space MMS: the solver of examples/mms and the oracle's restatement of the same problem
# ------------------------------------------------------------------------------------------------------------------------------
def mms_example():
    import os
    import sys
    p = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples", "mms")
    if p not in sys.path:
        sys.path.insert(0, p)
    import run_MMS_space
    return run_MMS_space


def space_mms_problem(S, dt):
    """The oracle's problem on the solver's mesh, with phi interpolated from the exact solution."""
    pb = omms.build_space_mms(None, p=S.degree_knp, dt=dt, mesh_tuple=(S.mesh, S.subdomains, S.surfaces))
    X = pb.space.interp_nodes()
    ics = (pb.cell_tags == 1)[:, None]
    pb.phi = np.where(ics, pb.mms._ev(pb.mms.phi_exact["1"], X), pb.mms._ev(pb.mms.phi_exact["2"], X))
    return pb


class FlippedJumpMMS(omms.SpaceMMS):
    """`SpaceMMS` with the solution-dependent term of L_knp given the wrong sign.  The parent hook is evaluated once with the
    problem's phi and once with zeros: the difference is that term."""

    def add_knp_rhs(self, pb, idx, b):
        full, data = np.zeros_like(b), np.zeros_like(b)
        super().add_knp_rhs(pb, idx, full)
        phi = pb.phi
        pb.phi = np.zeros_like(phi)
        try:
            super().add_knp_rhs(pb, idx, data)
        finally:
            pb.phi = phi
        b += data - (full - data)


def oracle_trajectory(resolution, p, dt, nsteps, flipped=False, mesh_tuple=None):
    """c, c_elim, phi after nsteps direct-solve steps of the oracle on the space MMS."""
    pb = omms.build_space_mms(resolution, p=p, dt=dt, mesh_tuple=mesh_tuple)
    if flipped:
        pb.mms = FlippedJumpMMS(dt)
    for _ in range(nsteps):
        ko.solve_for_time_step(pb, direct=True)
    return pb


# ------------------------------------------------------------------------------------------------------------------------------
# partitioned contexts
# ------------------------------------------------------------------------------------------------------------------------------
def partitioned_box(p):
    """The boxes of test_partitioned_kernels_on_one_gpu cut in two slabs.  The cells are sorted by midpoint x, and an equal split falls
    on a plane between two layers of box cells, where no membrane facet has its two cells on different sides; a cut INSIDE a layer
    leaves tets of one box cell on both sides, and with them membrane facets of the lateral walls whose other cell is a ghost."""
    from knpemidg.partition import Partition
    m, s, f = small_3d((12, 4, 4) if p == 1 else (8, 3, 3))
    return m, s, f, Partition(m, 2, method="slab", fractions=(0.0, 0.46, 1.0))


def ghost_backed_membrane_facets(loc, facet_tags_local, membrane_tags):
    """number of local membrane facets with an owned cell on one side and a ghost cell on the other"""
    fc = loc.mesh.facet_cells
    no = loc.nc_owned
    mem = np.isin(facet_tags_local, list(membrane_tags)) & (fc[:, 1] >= 0)
    return int((mem & ((fc[:, 0] < no) != (fc[:, 1] < no))).sum())
