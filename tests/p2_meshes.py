"""Two small UNSTRUCTURED meshes on which every ordered pair (own local facet I, neighbour's local facet j) occurs, and the helper
that counts the pairs.  The DG-P2 kernels (csrc/apply_p2.hip, csrc/tab_rhs.hip, csrc/tab_assembled.hip) and the 2D coordinate kernels treat a facet by
that index pair: I is a template parameter, j picks the permutation the neighbour's dofs are gathered through, so each pair is
its own piece of arithmetic -- 16 in 3D, 9 in 2D.  Box meshes and their refinements carry 4 of 16 (5 of 9) on SIPG facets and
2 (1) on membrane facets; these two carry all of them, on every facet class.  Data selection only, no arithmetic of either path.

tissue_piece():  2 114 tets of the tissue reconstruction (three subdomains, both membrane tags, slivers); 16 / 16 / 16 pairs
delaunay_2d() :  781 triangles, Delaunay triangulation of 400 seeded points, a disc of tag-1 cells; 9 / 9 pairs"""
import numpy as np

# box in cm; the smallest found on which all 16 pairs occur on the SIPG facets and on both membrane tags, and on which every SIPG
# pair occurs with the neighbour inside AND outside the cell's 256-cell device block (tests/test_gpu_p2_unstructured.py checks it)
TISSUE_LO = (3.0e-4, 2.1e-4, 1.0e-4)
TISSUE_HI = (4.0e-4, 3.2e-4, 2.1e-4)


def tissue_piece():
    import emix_sub
    return emix_sub.emix_submesh(lo=np.array(TISSUE_LO), hi=np.array(TISSUE_HI))


def delaunay_2d():
    from scipy.spatial import Delaunay
    from knpemidg.mesh import Mesh, MeshFunction
    pts = np.random.default_rng(3).uniform(0, 1, size=(400, 2)) * 1e-5
    cells = np.sort(Delaunay(pts).simplices.astype(np.int64), axis=1)          # ascending vertex ids per cell: the indexing contract
    mesh = Mesh(pts, cells.astype(np.int32))
    mid = mesh.coords[mesh.cells].mean(axis=1)
    sub = (np.sqrt(((mid - 0.5e-5) ** 2).sum(axis=1)) < 0.25e-5).astype(np.uint32)
    fc = mesh.facet_cells
    interior = fc[:, 1] >= 0
    tags = np.zeros(mesh.num_facets(), dtype=np.uint32)
    tags[~interior] = 5                                                         # as make_mesh_2D
    tags[interior] = sub[fc[interior, 0]] != sub[fc[interior, 1]]
    return mesh, MeshFunction(mesh, 2, sub), MeshFunction(mesh, 1, tags)


def facet_pair_coverage(mesh, facet_tags, tags):
    """{tag: set of ordered (I, j)} over the interior facets carrying `tag` (0 = SIPG), both orientations of every facet."""
    fc, fl = mesh.facet_cells, mesh.facet_local.astype(np.int64)
    ft = np.asarray(facet_tags)
    interior = fc[:, 1] >= 0
    out = {}
    for t in tags:
        sel = interior & (ft == t)
        a, b = fl[sel, 0], fl[sel, 1]
        out[t] = set(zip(a.tolist(), b.tolist())) | set(zip(b.tolist(), a.tolist()))
    return out
