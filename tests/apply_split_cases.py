"""Cell orders that put the boundary between the staged HEAD kernel and the thread-per-cell TAIL kernel of a 3D P1 operator apply
(csrc/apply_plan.hpp) inside the mesh, as seeded host-side recipes: tests/test_apply_split_host.py proves on the CPU that every case
has the property it exists for, tests/test_gpu_apply_split.py and tests/test_gpu_tables.py run the same orders on the device.

The head of an apply covers the leading 256-cell blocks that fit the staging limits of its kernel family:
  * structured meshes (geometry classes; ring-staged variants 3 / 7, halo-staged 2 / 6): a block's list of coupled neighbours OUTSIDE
    the block holds at most 256 entries (csrc/context_tables.hpp: halo_block_lists -> hb_long0, hb_stride); the ring kernels
    additionally want hb_stride <= 224 (apply_ring.hip: ring_usable);
  * unstructured meshes (variant 10): at most 320 list entries -- here a neighbour that is not OWNED counts as outside whatever its
    block -- and at most 256 staged vertices: the block's own ones plus the apex vertex of every coupled neighbour
    (apply_ring_u.hip: build_tables_u -> long0, hs).
`block_stats` restates both rules from the mesh alone.  A Morton-ordered box never overflows a block, so the cases start from the
device's own order (`_abi.device_cell_order`) and exchange cells between blocks; the tests hand the device the permuted mesh
(`permuted_mesh`) with KNP_NO_REORDER=1, which makes the caller's order the device order.

Numbers of the cases as the CPU test asserts them (list entries structured rule / unstructured rule, staged vertices): see CASES."""
import numpy as np

from knpemidg import _abi
from knpemidg.mesh import Mesh, MeshFunction

B = 256                      # cells per block (KNP_HALO_BLK, ring::RB)
LIST_S = 256                 # structured: list entries per block (one per thread)
RING_S = 224                 # ring-staged structured kernels: longest list they stage (ring::RH)
LIST_U, VERT_U = 320, 256    # unstructured ring: list entries (UH) and vertices (UV) per block
BOX = (16, 6, 6)             # small_3d box of the recipes: 3 456 tets, 14 blocks (the last one half full)


def _facet_keys(facets, nv):
    f = np.sort(np.asarray(facets, dtype=np.int64), axis=1)
    key = f[:, 0]
    for j in range(1, f.shape[1]):
        key = key * nv + f[:, j]
    return key


def permuted_mesh(mesh, sub, surf, perm):
    """(mesh', sub', surf'): cell i of mesh' is cell perm[i] of mesh (same vertices, same tag); a facet keeps the tag of the facet
    with the same sorted vertex tuple (the facet numbering follows the cell order, so it changes)."""
    perm = np.asarray(perm, dtype=np.int64)
    assert np.array_equal(np.sort(perm), np.arange(mesh.num_cells()))
    pm = Mesh(mesh.coords.copy(), mesh.cells[perm])
    assert np.array_equal(pm.cells, mesh.cells[perm])
    nv = mesh.num_vertices()
    old, new = _facet_keys(mesh.facets, nv), _facet_keys(pm.facets, nv)
    srt = np.argsort(old)
    pos = np.searchsorted(old[srt], new)
    assert np.array_equal(old[srt][pos], new)
    return pm, MeshFunction(pm, mesh.gdim, np.asarray(sub.array())[perm]), MeshFunction(pm, mesh.gdim - 1, np.asarray(surf.array())[srt][pos])


class _Coupling:
    """Caller-numbered tables of a tetrahedral mesh: nb [nc, 4] the COUPLED cell behind local facet a (-1: none), apex [nc, 4] the
    vertex of that cell opposite the shared facet.  facet_tags None: every interior facet couples (SIPG or membrane); else the
    facets tagged 0 (SIPG) or with one of membrane_tags do (csrc/context_tables.hpp: facet_tables)."""

    def __init__(self, mesh, facet_tags=None, membrane_tags=()):
        nc = mesh.num_cells()
        fc, fl, cf = np.asarray(mesh.facet_cells), np.asarray(mesh.facet_local).astype(np.int64), np.asarray(mesh.cell_facets)
        side = (fc[cf, 0] != np.arange(nc)[:, None]).astype(np.int64)
        nb = np.take_along_axis(fc[cf], (1 - side)[:, :, None], axis=2)[:, :, 0].astype(np.int64)
        nj = np.take_along_axis(fl[cf], (1 - side)[:, :, None], axis=2)[:, :, 0]
        if facet_tags is not None:
            t = np.asarray(facet_tags)[cf]
            nb = np.where((t == 0) | np.isin(t, list(membrane_tags)), nb, -1)
        self.cells = np.asarray(mesh.cells).astype(np.int64)
        self.nb = nb
        self.nj = np.where(nb >= 0, nj, 0)
        self.apex = np.where(nb >= 0, self.cells[np.maximum(nb, 0), np.maximum(self.nj, 0)], -1)

    def block(self, order, rank, n_own, b):
        """(list entries by the structured rule, by the unstructured rule, staged vertices) of block b of the device order"""
        cs = order[b * B:min(n_own, (b + 1) * B)]
        nbc = self.nb[cs]
        has = nbc >= 0
        nbd = rank[np.maximum(nbc, 0)]
        away = nbd // B != b
        n_s = int((has & away).sum())
        n_u = int((has & (away | (nbd >= n_own))).sum())
        n_v = len(np.unique(np.concatenate([self.cells[cs].ravel(), self.apex[cs][has]])))
        return n_s, n_u, n_v


def _rank_of(order):
    rank = np.empty(len(order), dtype=np.int64)
    rank[order] = np.arange(len(order))
    return rank


def block_stats(mesh, order, n_own, facet_tags=None, membrane_tags=()):
    """Both table builders restated from the mesh alone, for the device order `order` (device cell d = cell order[d] of mesh; the first
    n_own device cells are owned).  Returns a dict of int arrays over the ceil(n_own / 256) blocks:
      lists_s  coupled neighbours outside the block (halo_block_lists)
      lists_u  coupled neighbours outside the block or not owned (build_tables_u: nbk / B == b && nbk < no is the in-block test)
      verts    vertices the unstructured ring stages: the block's own plus the apex vertex of EVERY coupled neighbour"""
    order = np.asarray(order, dtype=np.int64)
    C, rank = _Coupling(mesh, facet_tags, membrane_tags), _rank_of(order)
    nblk = (n_own + B - 1) // B
    st = np.array([C.block(order, rank, n_own, b) for b in range(nblk)], dtype=np.int64).reshape(nblk, 3)
    return dict(lists_s=st[:, 0], lists_u=st[:, 1], verts=st[:, 2])


def _first(mask):
    hit = np.nonzero(mask)[0]
    return int(hit[0]) if len(hit) else len(mask)


def expected_structured(stats):
    """(hb_long0, hb_stride) of KNP_DT_META: the first block whose list exceeds one entry per thread, and the longest list before it
    rounded up to 8 entries -- (0, 0) when the first block overflows or no block has a neighbour outside it."""
    long0 = _first(stats["lists_s"] > LIST_S)
    hs = (int(stats["lists_s"][:long0].max()) + 7) // 8 * 8 if long0 else 0
    return (long0, hs) if hs else (0, 0)


def expected_unstructured(stats):
    """(long0, hs) of KNP_DT_RU_META: the first block over 320 list entries or 256 vertices, and the longest list before it (at least
    1) -- (0, 0) when the first block overflows: no unstructured ring."""
    long0 = _first((stats["lists_u"] > LIST_U) | (stats["verts"] > VERT_U))
    return (long0, max(int(stats["lists_u"][:long0].max()), 1)) if long0 else (0, 0)


# ---- the recipes ---------------------------------------------------------------------------------------------------------------
def base_mesh(kind, box=BOX):
    """'S': small_3d(box) as built (geometry classes); 'J': every interior vertex moved, as in test_unstructured_apply_kernel_variants
    (no classes)."""
    from common import small_3d
    m, s, f = small_3d(box)
    if kind == "J":
        rng = np.random.default_rng(11)
        inner = np.ones(m.num_vertices(), dtype=bool)
        inner[np.unique(m.facets[m.exterior_facets()])] = False
        jit = rng.uniform(-1, 1, size=m.coords.shape) * np.array([0.2e-6, 0.02e-6, 0.02e-6])
        m.coords[inner] += jit[inner]
    else:
        assert kind == "S"
    return m, s, f


def cut_points(head, n_own):
    """Interior counts that put the cut of a forced-split apply at both ends, one cell either side of a block edge, inside the head,
    exactly on head_cells, one cell either side of it, and inside the tail"""
    return sorted({n for n in (1, B - 1, B, B + 1, head - B, head - 1, head, head + 1, n_own - 1) if 0 < n < n_own})


# (mesh kind, case) -> what the device must report: on S (hb_long0, hb_stride) of KNP_DT_META, on J (long0, hs) of KNP_DT_RU_META, and
# the apply variants (EMI, KNP).  Restated from block_stats by the CPU test, read back from the device by the GPU tests.
EXPECT = {
    ("S", "A"): ((14, 168), (3, 7)), ("S", "B1"): ((1, 88), (3, 7)), ("S", "B7"): ((7, 168), (3, 7)), ("S", "C"): ((5, 168), (3, 7)),
    ("S", "E_struct"): ((8, 256), (1, 6)), ("S", "F"): ((14, 240), (1, 6)), ("S", "G"): ((0, 0), (1, 1)),
    ("J", "A"): ((14, 168), (10, 10)), ("J", "B1"): ((1, 86), (10, 10)), ("J", "B7"): ((7, 168), (10, 10)),
    ("J", "C"): ((14, 298), (10, 10)), ("J", "D1"): ((1, 86), (10, 10)), ("J", "D6"): ((6, 168), (10, 10)),
    ("J", "E_lists"): ((8, 320), (10, 10)), ("J", "E_verts"): ((8, 207), (10, 10)), ("J", "G"): ((0, 0), (0, 0)),
}


# Partitions (two slabs, the device's own order): box, mesh kind -> what the CPU test asserts for both ranks
PARTITIONS = {
    ((6, 10, 10), "S"): "hb_long0 = 6 of 8 blocks, n_interior = 1600 > head_cells = 1536: the boundary launch runs the tail kernel alone",
    ((6, 8, 8), "S"): "every list fits, the last one holds 240 entries: the ring refuses the mesh, KNP runs the halo kernel",
    ((6, 10, 10), "J"): "unstructured ring on 6 of 8 blocks",
    ((12, 4, 4), "J"): "unstructured ring on all 3 blocks; ghosts whose ids fall in the last block's range are staged through its list",
}


def partition_rank(box, kind, rank):
    """(LocalMesh, local cell tags, local facet tags, global mesh, global cell tags, global facet tags) of slab `rank` of two"""
    from knpemidg.partition import Partition
    m, s, f = base_mesh(kind, box)
    loc = Partition(m, 2, method="slab").local(rank)
    sub_l, surf_l = loc.localize(s, f, (1,))
    return loc, sub_l, surf_l, m, s, f


def _swap_blocks(order, b0, b1, n, rng):
    """n random cells of block b0 change places with n random cells of block b1"""
    i = b0 * B + rng.choice(B, size=n, replace=False)
    j = b1 * B + rng.choice(B, size=n, replace=False)
    order[i], order[j] = order[j].copy(), order[i].copy()


def _tune(C, order, n_own, b, col, target, partners, limits, rng, max_steps=6000):
    """Greedy single exchanges between block b and the blocks `partners` until statistic `col` of block b (0 lists_s, 1 lists_u,
    2 verts) equals target: an exchange is kept when it brings the statistic closer and leaves the other statistics of block b and
    all of the partner block within `limits` (None: unconstrained).  Returns the value reached (bounded search: it may stop short)."""
    rank = _rank_of(order)

    def within(st, skip=None):
        return all(lim is None or q == skip or st[q] <= lim for q, lim in enumerate(limits))
    cur = C.block(order, rank, n_own, b)[col]
    for _ in range(max_steps):
        if cur == target:
            break
        i = b * B + int(rng.integers(B))
        pb_ = int(partners[rng.integers(len(partners))])
        j = pb_ * B + int(rng.integers(min(n_own, (pb_ + 1) * B) - pb_ * B))
        ci, cj = order[i], order[j]
        order[i], order[j], rank[ci], rank[cj] = cj, ci, j, i
        sb, sp = C.block(order, rank, n_own, b), C.block(order, rank, n_own, pb_)
        if abs(sb[col] - target) < abs(cur - target) and within(sb, skip=col) and within(sp):
            cur = sb[col]
        else:
            order[i], order[j], rank[ci], rank[cj] = ci, cj, i, j
    return cur


def case_order(name, mesh):
    """The device order of case `name` on `mesh` (S or J of base_mesh): the Morton order of the device, then the seeded exchanges."""
    nc = mesh.num_cells()
    order = _abi.device_cell_order(mesh, nc, True)[0].copy()
    rng = np.random.default_rng(CASES[name]["seed"])
    kind, arg = CASES[name]["recipe"]
    if kind == "morton":
        pass
    elif kind == "shuffle_from":                      # everything from block arg on in random order
        order[arg * B:] = order[arg * B:][rng.permutation(nc - arg * B)]
    elif kind == "swap":                              # (block, block, cells) exchanges
        for b0, b1, n in arg:
            _swap_blocks(order, b0, b1, n, rng)
    elif kind == "tune":                              # (block, statistic, target, partner blocks, limits) greedy searches
        C = _Coupling(mesh)
        for b, col, target, partners, limits in arg:
            _tune(C, order, nc, b, col, target, partners, limits, rng)
    else:
        raise KeyError(kind)
    return order


_U = (None, LIST_U, VERT_U)          # a block the unstructured ring still takes
_S = (LIST_S, None, None)            # a block the structured kernels still take

# name -> mesh kinds it runs on, seed, recipe.  The expectations are asserted by tests/test_apply_split_host.py.
CASES = {
    "A": dict(on="SJ", seed=1, recipe=("morton", None)),
    "B1": dict(on="SJ", seed=2, recipe=("shuffle_from", 1)),
    "B7": dict(on="SJ", seed=3, recipe=("shuffle_from", 7)),
    "C": dict(on="SJ", seed=4, recipe=("swap", [(5, 6, 32)])),
    "D1": dict(on="J", seed=5, recipe=("swap", [(1, 2, 48)])),
    "D6": dict(on="J", seed=6, recipe=("swap", [(6, 7, 48)])),
    # exact limits: block 3 AT a limit (still staged), block 8 one PAST it (the first block of the tail): they catch an off-by-one in
    # `nh >= UH`, `nvb >= UV` and `size() > B`.  The bounded greedy searches reach all six values exactly (320 / 321 entries, 256 / 257
    # vertices, 256 / 257 entries by the structured rule) within a few hundred exchanges
    "E_lists": dict(on="J", seed=7, recipe=("tune", [(3, 1, LIST_U, (4,), _U), (8, 1, LIST_U + 1, (9,), _U)])),
    "E_verts": dict(on="J", seed=8, recipe=("tune", [(3, 2, VERT_U, (10, 11, 12), _U), (8, 2, VERT_U + 1, (10, 11, 12), _U)])),
    "E_struct": dict(on="S", seed=9, recipe=("tune", [(3, 0, LIST_S, (4,), _S), (8, 0, LIST_S + 1, (9,), _S)])),
    "F": dict(on="S", seed=10, recipe=("tune", [(5, 0, 240, (6,), (RING_S, None, None))])),
    "G": dict(on="SJ", seed=11, recipe=("shuffle_from", 0)),
}
