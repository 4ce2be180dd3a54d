"""Ownership tables of the recorder in a partitioned run (knpemidg/recorder.py: localize_tables), host only: over the ranks of a
partition the per-rank tables must add up to the global table -- every probe, set facet and map facet owned exactly once, the
weights of a set summing to 1, the owned region volumes to the global ones, the map positions partitioning [0, n_map).

The inputs (tests/recorder_partition_cases.py) are asserted, not assumed, to reach the edges: a set with facets of split ownership,
a set on one rank, a probe in a cell that is a ghost elsewhere, a probe on a vertex shared across a cut, a region absent from a rank
and cells outside every region.  The three-rank partitions have 64 / 64 / 16 membrane facets whose two cells lie on different ranks;
the two-rank slab has none, which is why the three-rank cases are there."""
from types import SimpleNamespace

import numpy as np
import pytest

import recorder_partition_cases as PC

N_CELLS = 15552
N_MEM = {"slab3": 1472, "thin3": 1472, "rcb3": 368, "slab2_p2": 1472}
N_MEM_CUT = {"slab3": 64, "thin3": 64, "rcb3": 16, "slab2_p2": 0}


@pytest.fixture(scope="module", params=list(PC.CASES))
def case(request):
    from knpemidg import recorder as R
    name = request.param
    mt, part, mtags, degree = PC.make_case(name)
    args, info = PC.record_args(mt, part, mtags)
    rec = R.Recorder(mt[0], mt[1].array(), mt[2].array(), degree, ["K", "Cl", "Na"], capacity=2, membrane_tags=mtags,
                     membrane_states=PC.STATES, membrane_map=dict(threshold=-0.06), **args)
    locs = [part.local(r) for r in range(part.world)]
    tables = [R.localize_tables(rec, loc) for loc in locs]
    return SimpleNamespace(name=name, mt=mt, part=part, mtags=mtags, rec=rec, locs=locs, tables=tables, info=info)


def test_the_inputs_reach_the_edges(case):
    mesh, part, rec, info = case.mt[0], case.part, case.rec, case.info
    owner, fc = part.owner, mesh.facet_cells
    assert mesh.num_cells() == N_CELLS and len(info["mem"]) == N_MEM[case.name] and len(info["mem_cut"]) == N_MEM_CUT[case.name]
    # a set with facets of split ownership (wherever the partition has any), a set entirely on one rank
    if N_MEM_CUT[case.name]:
        assert np.isin(info["mem_cut"], rec.set_facets[0]).all()
        split = rec.set_facets[0][owner[fc[rec.set_facets[0], 0]] != owner[fc[rec.set_facets[0], 1]]]
        assert len(split) == N_MEM_CUT[case.name]
        # both sides see such a facet (it is processed redundantly in the ODE step), one records it
        f = int(split[0])
        assert all(case.tables[int(owner[c])].facet_local(f) >= 0 for c in fc[f])
    assert len(np.unique(owner[fc[rec.set_facets[1]].ravel()])) == 1 and len(rec.set_facets[1]) == 5
    assert sum(len(T.set_facets[1]) > 0 for T in case.tables) == 1
    assert 0 < len(rec.set_facets[2]) < len(info["mem"])                         # the box
    # probe 0: its cell is a ghost on another rank; probe 1: exactly on a vertex of a facet on a cut, shared by cells of two ranks
    c0 = int(rec.point_cells[0])
    assert c0 == info["ghost_cell"]
    others = [loc for loc in case.locs if loc.rank != owner[c0]]
    assert any(loc.g2l[c0] >= loc.nc_owned for loc in others)
    v = int(mesh.facets[info["cut_facet"]][0])
    assert np.array_equal(rec.point_coords[1], mesh.coords[v])
    assert len(np.unique(owner[np.nonzero((mesh.cells == v).any(axis=1))[0]])) >= 2
    assert np.sort(rec.point_bary[1])[-1] == pytest.approx(1.0, abs=1e-12)
    # probes 2 and 3: the same point on a membrane, one cell on either side
    assert np.array_equal(rec.point_coords[2], rec.point_coords[3]) and rec.point_cells[2] != rec.point_cells[3]
    # regions: one absent from at least one rank, some cells in none
    assert rec.n_regions == info["n_regions"] and (rec.region == 255).sum() > 100
    present = [np.isin(info["extra_region"], T.region[:loc.nc_owned]) for T, loc in zip(case.tables, case.locs)]
    assert any(present) and not all(present)


def test_every_probe_is_owned_exactly_once(case):
    rec, part = case.rec, case.part
    owned = np.stack([T.point_cells >= 0 for T in case.tables])
    assert owned.shape == (part.world, rec.n_points) and (owned.sum(axis=0) == 1).all()
    for T, loc in zip(case.tables, case.locs):
        mine = np.nonzero(T.point_cells >= 0)[0]
        assert (T.point_cells[mine] < loc.nc_owned).all()
        assert np.array_equal(loc.cells_global[T.point_cells[mine]], rec.point_cells[mine])      # the cell the global search chose
        assert (T.point_cells[T.point_owner != T.rank] == -1).all()
    assert all(np.array_equal(T.point_owner, case.tables[0].point_owner) for T in case.tables)


def test_set_facets_and_weights_add_up(case):
    rec = case.rec
    for s in range(rec.n_sets):
        n = len(rec.set_facets[s])
        seen = np.zeros(n, dtype=int)
        wsum = 0.0
        for T, loc in zip(case.tables, case.locs):
            seen[T.set_index[s]] += 1
            assert np.array_equal(loc.facets_global[T.set_facets[s]], rec.set_facets[s][T.set_index[s]])
            assert np.array_equal(T.set_weights[s], rec.set_weights[s][T.set_index[s]])
            assert (np.diff(T.set_index[s]) > 0).all()                                             # the set's own order is kept
            # the owner holds the facet's first cell
            assert (loc.mesh.facet_cells[T.set_facets[s]] < loc.nc_owned).any(axis=1).all()
            assert (case.part.owner[case.mt[0].facet_cells[rec.set_facets[s][T.set_index[s]], 0]] == T.rank).all()
            wsum += T.set_weights[s].sum()
        assert (seen == 1).all(), (s, np.nonzero(seen != 1)[0][:5])
        assert abs(wsum - 1.0) <= 1e-15 * n, (s, wsum - 1.0)


def test_region_volumes_add_up(case):
    rec = case.rec
    glob = np.asarray([rec.vol[rec.region == r].sum() for r in range(rec.n_regions)])
    part_sum = sum(T.region_volume_owned for T in case.tables)
    assert (glob > 0).all() and np.abs(part_sum / glob - 1.0).max() < 1e-13
    for T, loc in zip(case.tables, case.locs):
        assert T.region.shape == T.vol.shape == (loc.mesh.num_cells(),)
        assert np.array_equal(T.region, rec.region[loc.cells_global]) and np.array_equal(T.vol, rec.vol[loc.cells_global])
        assert np.array_equal(T.inv_rvol, case.tables[0].inv_rvol) and np.abs(T.inv_rvol * glob - 1.0).max() < 1e-14
    # the cells in no region are in no rank's sums
    counted = sum(int((T.region[:loc.nc_owned] != 255).sum()) for T, loc in zip(case.tables, case.locs))
    assert counted == int((rec.region != 255).sum())


def test_map_positions_partition_the_map(case):
    rec = case.rec
    n = len(rec.map_facets)
    assert n == N_MEM[case.name]
    pos = np.concatenate([T.map_pos for T in case.tables])
    assert np.array_equal(np.sort(pos), np.arange(n))
    for T, loc in zip(case.tables, case.locs):
        assert np.array_equal(loc.facets_global[T.map_facets], rec.map_facets[T.map_pos])
        assert (T.facet_owner(rec.map_facets[T.map_pos]) == T.rank).all()


def test_state_channels_use_the_global_weights(case):
    """Entry lists per rank from stand-in models (facets, tag, handle, ode): over the ranks every (set, state) channel holds each
    facet of the set once and its weights sum to 1; a state that no model of a set has is refused on the global tables."""
    from knpemidg import recorder as R
    from knpemidg.models import mm_hh, mm_hh_no_stim, mm_leak
    rec = case.rec
    odes = {1: mm_hh, 2: mm_hh_no_stim}
    n_ch = rec.n_sets * len(PC.STATES)
    wsum, count = np.zeros(n_ch), np.zeros(n_ch, dtype=int)
    for T, loc in zip(case.tables, case.locs):
        _, surf_l = loc.localize(case.mt[1], case.mt[2], case.mtags)
        ft = np.asarray(surf_l.array())
        models = [SimpleNamespace(facets=np.nonzero((ft == t) & (loc.mesh.facet_cells[:, 1] >= 0))[0], ode=odes[t], handle=10 + t, tag=t)
                  for t in case.mtags]
        ptr, eh, er, ec, ew = R.state_entries_local(rec, T, models)
        assert len(ptr) == n_ch + 1 and (np.diff(ptr) >= 0).all()
        for ch in range(n_ch):
            sl = slice(ptr[ch], ptr[ch + 1])
            wsum[ch] += ew[sl].sum()
            count[ch] += ptr[ch + 1] - ptr[ch]
            k = np.asarray([case.mtags.index(h - 10) for h in eh[sl]], dtype=int)
            assert all(er[sl][i] < len(models[k[i]].facets) for i in range(len(k)))
            assert (ec[sl] == odes[1].state_indices(PC.STATES[ch % len(PC.STATES)])).all()
    for ch in range(n_ch):
        n = len(rec.set_facets[ch // len(PC.STATES)])
        assert count[ch] == n and abs(wsum[ch] - 1.0) <= 1e-15 * n, (ch, count[ch], wsum[ch] - 1.0)
    leak = [SimpleNamespace(facets=np.zeros(0, dtype=np.int64), ode=mm_leak, handle=1, tag=t) for t in case.mtags]
    with pytest.raises(ValueError, match="no facet of the set"):
        R.state_weights_global(rec.mesh, rec.facet_tags, rec.set_facets, leak, PC.STATES)
