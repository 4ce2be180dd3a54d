"""CPU side of the (own facet I, neighbour facet j) coverage of the DG-P2 kernels: the two unstructured meshes of tests/p2_meshes.py
carry every ordered pair on every facet class (the condition of tests/test_gpu_p2_unstructured.py, checked here so that a mesh
change cannot silently shrink it), the numpy restatement of the kernels' formulation (tests/p2_formulation.py) agrees with the
oracle's assembled operators on them, and a wrong neighbour permutation is seen there for every (I, j), on the box mesh for 4 of 16."""
import numpy as np
import pytest

import knpemi_oracle as ko
import p2_formulation as pf
import p2_meshes
from common import synthetic_state, relerr, small_3d

ALL_3D = {(i, j) for i in range(4) for j in range(4)}
ALL_2D = {(i, j) for i in range(3) for j in range(3)}
_CACHE = {}


def _case(name):
    """Problem, seeded vector, Geo, tables and the oracle's products A_emi x, A_knp,k x (assembled once per mesh)."""
    if name not in _CACHE:
        if name == "tissue_piece":
            m, s, f = p2_meshes.tissue_piece()
            pb = ko.build_tortuosity(m, s.array(), f.array(), p=2)
            volt = 1.0e3
        elif name == "delaunay_2d":
            m, s, f = p2_meshes.delaunay_2d()
            pb = ko.build_idealized(m, s.array(), f.array(), p=2, membrane_tags=(1,))
            volt = 1.0
        else:
            m, s, f = small_3d((8, 4, 4))
            pb = ko.build_idealized(m, s.array(), f.array(), p=2, membrane_tags=(1,))
            volt = 1.0
        x = synthetic_state(pb, volt=volt)
        geo = pf.Geo(m, pb.cell_tags, pb.facet_tags, pb.membrane_tags)
        Aemi, _, _ = ko.assemble_emi(pb, want_B=False)
        ye = Aemi @ x[0].ravel()
        yk = [ko.assemble_knp(pb, k) @ x[k].ravel() for k in range(pb.N_ions)]
        _CACHE[name] = (pb, x, geo, pf.load_tables(m.gdim), ye, yk)
    return _CACHE[name]


def _emi(case, T):
    pb, x, geo = case[:3]
    return pf.emi_apply(geo, T, x[0].ravel(), pb.kappa(), pb.tau, pb.C_phi)


def _knp(case, T, k):
    pb, x, geo = case[:3]
    return pf.knp_apply(geo, T, x[k].ravel(), pb.phi, pb.ions[k]["D"], pb.ions[k]["z"], pb.psi, pb.tau, pb.dt)


def test_every_facet_pair_occurs_on_the_unstructured_meshes():
    m, s, f = p2_meshes.tissue_piece()
    sub = s.array()
    assert m.num_cells() == 2114 and np.bincount(sub).tolist() == [1133, 844, 137]
    ft = f.array()
    interior = m.facet_cells[:, 1] >= 0
    assert int((interior & (ft == 1)).sum()) == 351 and int((interior & (ft == 2)).sum()) == 81
    cov = p2_meshes.facet_pair_coverage(m, ft, (0, 1, 2))
    assert cov[0] == ALL_3D and cov[1] == ALL_3D and cov[2] == ALL_3D
    m, s, f = p2_meshes.delaunay_2d()
    ft = f.array()
    interior = m.facet_cells[:, 1] >= 0
    assert m.num_cells() == 781 and int((interior & (ft == 0)).sum()) == 1122 and int((interior & (ft == 1)).sum()) == 41
    assert (np.diff(m.cells.astype(np.int64), axis=1) > 0).all()
    cov = p2_meshes.facet_pair_coverage(m, ft, (0, 1))
    assert cov[0] == ALL_2D and cov[1] == ALL_2D


def test_box_meshes_carry_a_quarter_of_the_pairs():
    """Why the unstructured meshes are needed: today's counts on the meshes every other DG-P2 / 2D comparison runs on."""
    from knpemidg.mesh import make_mesh_2D
    m, s, f = small_3d((8, 4, 4))
    cov = p2_meshes.facet_pair_coverage(m, f.array(), (0, 1))
    assert (len(cov[0]), len(cov[1])) == (4, 2)
    m, s, f = make_mesh_2D(1)
    cov = p2_meshes.facet_pair_coverage(m, f.array(), (0, 1))
    assert (len(cov[0]), len(cov[1])) == (5, 1)


@pytest.mark.parametrize("name", ["tissue_piece", "delaunay_2d"])
def test_formulation_matches_the_oracle(name):
    """emi_apply and knp_apply (every solved species) against the oracle's assembled CSR operators times a seeded vector: 1e-12 of
    the max norm (observed: EMI 5.5e-15 on the tissue piece)."""
    case = _case(name)
    pb, T, ye, yk = case[0], case[3], case[4], case[5]
    e = relerr(_emi(case, T), ye)
    print("%s: emi %.2e" % (name, e))
    assert e < 1e-12
    for k in range(pb.N_ions):
        e = relerr(_knp(case, T, k), yk[k])
        print("%s: knp[%d] %.2e" % (name, k, e))
        assert e < 1e-12


def _swapped(T, j, own=None):
    """Table set whose FRAME_PACKED[j] has the nibbles of facet vertices 0 and 1 (frame slots 1 and 2) exchanged -- for every own
    facet, or only where the own local facet is `own` (one (I, j) combination, as one template instance of the kernels sees it)."""
    p = int(T["FRAME_PACKED"][j])
    a, b = (p >> 4) & 15, (p >> 8) & 15
    p = (p & ~0xff0) | (b << 4) | (a << 8)
    out = dict(T)
    table = [p if k == j else v for k, v in enumerate(T["FRAME_PACKED"])]
    if own is None:
        out["FRAME_PACKED"] = table
    else:
        out["FRAME_PACKED_OWN"] = {own: table}
    return out


def test_a_wrong_neighbour_permutation_is_seen_on_the_unstructured_meshes():
    """The gap was real.  With two facet-vertex nibbles of ONE neighbour permutation exchanged, both operators differ from the
    oracle's by more than 1e-6 of the max norm on tissue_piece() and delaunay_2d(), for every j -- and so does the EMI operator with
    the exchange confined to ONE (I, j) combination, for each of the 16 (9).
    Outcome on small_3d((8, 4, 4)), the mesh of the `3D_box_P2` comparisons (noted; `pytest -s` prints it): the j-wide mutation is
    noticed there for every j too (EMI 8e-2 ... 1e-1, KNP 8e-2 ... 1e-1), because its pairs carry each j once; confined to one
    (I, j), it is noticed for exactly the combinations the box has -- (0, 3), (1, 1), (2, 2), (3, 0); the two of its membrane facets
    are among them -- and the operator stays within 1e-12 of the oracle's for the other 12: an error in the code of any of those
    passed every DG-P2 comparison with the oracle."""
    for name in ("tissue_piece", "delaunay_2d"):
        case = _case(name)
        pb, T, ye, yk = case[0], case[3], case[4], case[5]
        for j in range(pb.d + 1):
            Tm = _swapped(T, j)
            assert relerr(_emi(case, Tm), ye) > 1e-6, (name, j)
            assert relerr(_knp(case, Tm, 0), yk[0]) > 1e-6, (name, j)
            for i in range(pb.d + 1):
                assert relerr(_emi(case, _swapped(T, j, own=i)), ye) > 1e-6, (name, i, j)
    case = _case("small_3d")
    pb, T, ye, yk = case[0], case[3], case[4], case[5]
    assert relerr(_emi(case, T), ye) < 1e-12
    for j in range(4):
        Tm = _swapped(T, j)
        print("small_3d((8, 4, 4)), FRAME_PACKED[%d] mutated: emi differs by %.1e, knp by %.1e"
              % (j, relerr(_emi(case, Tm), ye), relerr(_knp(case, Tm, 0), yk[0])))
    cov = p2_meshes.facet_pair_coverage(pb.mesh, pb.facet_tags, (0, 1))
    seen = {(i, j) for i in range(4) for j in range(4) if relerr(_emi(case, _swapped(T, j, own=i)), ye) > 1e-12}
    print("small_3d((8, 4, 4)), one (I, j) mutated: noticed for %d of 16: %s" % (len(seen), sorted(seen)))
    assert seen == cov[0] | cov[1]
