"""Inputs shared by tests/test_recorder_partition_host.py, tests/test_gpu_recorder_partition.py and its worker: the partitions to
cover and, per partition, one set of `Solver.record` arguments in the global mesh's terms that reaches every edge of the ownership
rules.  Everything is derived from the global mesh and the partition alone, so every rank and the parent build the same arguments."""
import numpy as np

#        name      world  method  fractions                n_axons  degree
CASES = {"slab3": (3, "slab", None, 4, 1),
         "thin3": (3, "slab", [0.0, 0.49, 0.51, 1.0], 4, 1),
         "rcb3": (3, "rcb", None, 1, 1),
         "slab2_p2": (2, "slab", None, 4, 2)}
FILE_CASE = "slab2"         # the two-rank P1 run that writes timeseries.h5 (not among the partitions whose rows are checked)
MORE_CASES = {FILE_CASE: (2, "slab", None, 4, 1)}
STATES = ("n", "m", "h")
EXTRA_REGION_CELLS = 40
N_STEPS = 4
# The idealized setup stimulates the axon of tag 1 on x < 20 um (examples/idealized_geometries/idealized_common.py).  The axon is 32 um
# long, far below its space constant, so it depolarises as a whole: phi_M starts near -68.4 mV and rises by about 5 mV per step (the
# figures in tests/test_gpu_recorder_membrane.py), while the unstimulated axons (tag 2, four-axon mesh) stay near rest.  A threshold
# of -64 mV is crossed in the first steps by the facets of tag 1 only.
STIM_X = 20.0e-6
MAP_THRESHOLD = -0.064
CV_SETS = (3, 4)            # two sets of stimulated facets at either end of the stimulated stretch, on different ranks


def make_case(name):
    """(mesh_tuple, partition, ode model tags, degree) of a case."""
    from knpemidg.mesh import make_mesh_3D
    from knpemidg.partition import Partition
    world, method, fractions, n_axons, degree = CASES.get(name) or MORE_CASES[name]
    mt = make_mesh_3D(0, n_axons=n_axons)
    part = Partition(mt[0], world, method=method, fractions=fractions)
    return mt, part, ((1, 2) if n_axons > 1 else (1,)), degree


def cut_facets(mesh, part, among=None):
    """Interior facets (of `among`, default all) whose two cells belong to different ranks."""
    fc = mesh.facet_cells
    f = np.nonzero(fc[:, 1] >= 0)[0] if among is None else np.asarray(among, dtype=np.int64)
    return f[part.owner[fc[f, 0]] != part.owner[fc[f, 1]]]


def record_args(mt, part, membrane_tags):
    """dict(points, point_tags, membrane_sets, regions) plus what the tests assert about them (`info`)."""
    from knpemidg import recorder as R
    mesh, sub, surf = mt[0], np.asarray(mt[1].array()), np.asarray(mt[2].array())
    owner, fc = part.owner, mesh.facet_cells
    mem = R.membrane_facets(mesh, surf, membrane_tags)
    mem_cut = cut_facets(mesh, part, mem)
    cut = cut_facets(mesh, part)
    mid = mesh.cell_midpoints()
    # membrane sets: every membrane facet (holds every cut facet); a few facets with both cells on the lowest rank that has them; a box
    whole = (owner[fc[mem, 0]] == owner[fc[mem, 1]])
    r_one = min(int(r) for r in np.unique(owner[fc[mem[whole], 0]]) if (owner[fc[mem[whole], 0]] == r).sum() >= 5)
    one_rank = mem[whole & (owner[fc[mem, 0]] == r_one)][:5]
    fm = mesh.facet_midpoints()[mem]
    fm = fm[fm[:, 0] <= np.quantile(fm[:, 0], 0.3)]                # the first stretch along x
    box = (fm.min(axis=0), fm.max(axis=0))
    stim = mem[(surf[mem] == 1) & (mesh.facet_midpoints()[mem, 0] < STIM_X)]
    stim = stim[np.argsort(mesh.facet_midpoints()[stim, 0], kind="stable")]
    sets = [mem, one_rank, box, stim[:6], stim[-6:]]
    # probes: a cell that is a ghost elsewhere; a vertex of a facet on a cut; one point on a membrane facet taken from either side;
    # the middle owned cell of every rank
    f0 = int(cut[len(cut) // 2])
    c_ghost = int(fc[f0, 0])
    vertex = mesh.coords[mesh.facets[f0][0]]
    fmem = int(mem[len(mem) // 2])
    pm = mesh.facet_midpoints()[fmem]
    pts = [mid[c_ghost], vertex, pm, pm]
    ptags = [None, None, int(sub[fc[fmem, 0]]), int(sub[fc[fmem, 1]])]
    for r in range(part.world):
        own = np.nonzero(owner == r)[0]
        pts.append(mid[own[len(own) // 2]])
        ptags.append(None)
    # regions: the subdomains, one more region made of a few cells of the last rank only, every 17th cell in none
    tags = np.unique(sub)
    region = np.searchsorted(tags, sub).astype(np.uint8)
    last = np.nonzero(owner == part.world - 1)[0]
    region[last[len(last) // 2:len(last) // 2 + EXTRA_REGION_CELLS]] = len(tags)
    region[::17] = R.REGION_NONE
    info = dict(stim=stim, mem=mem, mem_cut=mem_cut, cut_facet=f0, ghost_cell=c_ghost, one_rank=r_one, n_regions=len(tags) + 1, extra_region=len(tags))
    return dict(points=np.asarray(pts), point_tags=ptags, membrane_sets=sets, regions=region), info
