"""The PARTITIONED V-cycle and Krylov loops (csrc/amg_vcycle.hip: dist0_smooth, amg_vcycle_dist0, k_l0_first_nz, k_l0_step; csrc/comm.hip:
interface_accumulate, k_if_pack, k_if_add, shm_interface_exchange; the all-reduced level-1 right-hand side, inner products and spectral
bound; build_bj_table with nc_owned < nc) against the host replica tests/amg_ref.py, iterate by iterate, as tests/test_gpu_amg.py does
for one rank.

Every rank is a process with its own device context on the one GPU and the shared-memory communicator (tests/amg_partition_worker.py;
one launch per group and partition of amg_ref.PART_GROUPS).  The observable is x_k after k Krylov iterations from x_0 = 0 at a
tolerance that cannot be reached, assembled from the ranks' owned rows (every cell exactly once).  The reference is the GLOBAL replica
on the production hierarchy (KNP_AMG_MAXCOARSE = 60: levels [267, 52] on the P1 box, [679, 124, 26] on the P2 box): the partitioned
preconditioner is the replicated one -- level 0 keeps the global inverse diagonal and prolongator, and every rank's level-0 matrix is
its share of the global one, entry by entry (amg.Dist0Space.split_matrix), so the fp32 values of the ranks add up to the fp32 global
matrix.  tests/test_amg_ref_host.py shows on the CPU that the replica's row-distributed form (amg_ref.vcycle_dist0) stays within the
bound of the global one on every case below, and that six deliberate errors of the distributed form are >= 1e7 bounds away.

Partitions: two x-slabs; three x-slabs whose middle one has no interior cell; the four quadrants of the y-z plane about the box centre
-- conforming dofs with two, (P2: three) and four owners, so that k_if_add sums more than two terms, and interface peers that are no
halo peers (ranks 0 and 3).  Three columns (nil = 1) and four (nil = 2, two groups) run through the interface exchange on the
quadrants.  Also asserted: a second identical solve returns the same bits on every rank, and with several columns another right-hand
side of species 1 leaves the other species' bits alone.

Bound ("V-cycle parity"): max(32 ||x64 - x_hp||_inf, 1e-13 ||x_hp||_inf) of the global replica in float64 / extended
precision (GMRES: also the float64 run with reversed sums) -- never taken from the device's numbers.  Measured on the MI355X, as
multiples of ||x_k||_inf, worst case of each group:

  group                                                              largest bound   largest device error   worst error / bound
  ----------------------------------------------------------------------------------------------------------------------------
  EMI  3D P1 box, 2 slabs, level-0 degree 1, both DG smoothers       1.2e-10         2.4e-12                0.22
  EMI  3D P1 box, 3 slabs (a rank without interior cells)            1.2e-10         4.7e-12                0.47
  EMI  3D P1 box, 4 quadrants, level-0 degrees 0, 1, 2               4.1e-10         8.4e-12                0.38
  KNP  3D P1 box, 2 species, 2 slabs, per-cell blocks / table        8.1e-13         2.7e-14                0.08
  KNP  3D P1 box, 2 species, 4 quadrants, + level-0 degree 0         1.4e-11         1.5e-12                0.29
  GMRES(8)  table, 3D P1 box, 2 species, 4 quadrants, 6 counts       1.2e-12         4.8e-14                0.10
  KNP  3D P1 box, 3 species (cell) / 4 species (table), quadrants    8.9e-12         2.8e-13                0.64
  EMI  3D P2 box, 2 slabs                                            8.4e-10         3.5e-11                0.04
  KNP  3D P2 box, 2 species, 2 slabs                                 5.9e-12         6.1e-13                0.10
  EMI  3D P2 box, 4 quadrants                                        8.4e-10         4.8e-11                0.06
  KNP  3D P2 box, 2 species, 4 quadrants                             5.9e-12         3.0e-13                0.05
  EMI  3D P1 box, replicated level 0 (KNP_AMG_DIST0=0), 2 slabs      1.2e-10         3.1e-12                0.31
  KNP  3D P1 box, replicated level 0, 2 species, 2 slabs             4.5e-13         1.8e-14                0.07

Ill-conditioned by the rule and not run: x_2 and x_3 of EMI on the P2 box with the Chebyshev DG smoother (bounds 1.15e-9, 1.53e-9)."""
import os
import subprocess
import sys
import time
import uuid

import numpy as np
import pytest

import amg_ref as ar

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
_HOSTS, _REF = {}, {}
LIMIT = 240.0                                                           # seconds for all ranks of a launch


def _reference(mesh, case):
    """amg_ref.part_reference of a case, computed once (it does not depend on the partition)"""
    key = ar.part_host_key(mesh, case)
    if (key, case) not in _REF:
        if key not in _HOSTS:
            _HOSTS[key] = ar.Host(*key)
        h = _HOSTS[key]
        _REF[(key, case)] = ar.part_reference(h, ar.part_levels(h, case), case)
    return _HOSTS[key], _REF[(key, case)]


def _launch(tmp_path, group, pname, world, env):
    """all ranks of one launch, each writing its log to a file; the first failure or the time limit ends the others, and the tails of
    the logs go into the assertion.  Nothing more is started afterwards."""
    name = "/knp_%s" % uuid.uuid4().hex[:16]
    logs = [str(tmp_path / ("rank%d.log" % r)) for r in range(world)]
    files = [open(l, "w") for l in logs]
    procs = [subprocess.Popen([sys.executable, os.path.join(HERE, "amg_partition_worker.py"), str(r), str(world), name, str(tmp_path), group,
                               pname], stdout=f, stderr=subprocess.STDOUT, env=env) for r, f in enumerate(files)]
    t0, why = time.monotonic(), None
    try:
        while why is None and any(p.poll() is None for p in procs):
            if any(p.poll() not in (None, 0) for p in procs):
                why = "a rank failed"
            elif time.monotonic() - t0 > LIMIT:
                why = "time limit"
            else:
                time.sleep(0.05)
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
        for p in procs:
            p.wait()
        for f in files:
            f.close()
    tails = "\n".join("--- rank %d (exit %s)\n%s" % (r, p.returncode, open(l).read()[-2000:]) for r, (p, l) in enumerate(zip(procs, logs)))
    assert why is None and all(p.returncode == 0 for p in procs), "%s\n%s" % (why or "a rank failed", tails)


@pytest.mark.parametrize("group,pname", ar.PART_LAUNCHES, ids=lambda v: str(v))
def test_partitioned_iterates_match_the_global_replica(hip_lib, tmp_path, monkeypatch, group, pname):
    _, mesh, dist0, parts = ar.part_group(group)
    cases = parts[pname]
    monkeypatch.setenv("KNP_AMG_MAXCOARSE", ar.PART_MAXCOARSE)          # (the replica's hierarchies below are built under it too)
    monkeypatch.setenv("KNP_AMG_DIST0", "1" if dist0 else "0")
    for key in ("KNP_AMG_DEGREE0_EMI", "KNP_AMG_DEGREE0_KNP", "KNP_AMG_DEGREE0", "KNP_COMM_SHM"):
        monkeypatch.delenv(key, raising=False)
    refs = [_reference(mesh, case) for case in cases]
    nc, nd = refs[0][0].pb.mesh.num_cells(), refs[0][0].nd
    world = ar.part_partition(refs[0][0].mt[0], pname).world
    _launch(tmp_path, group, pname, world, dict(os.environ))
    data = [np.load(str(tmp_path / ("rank%d.npz" % r))) for r in range(world)]
    seen = np.zeros(nc, dtype=int)
    for d in data:
        seen[d["cells"]] += 1
    assert (seen == 1).all()                                            # every cell owned by exactly one rank
    bad, flags = [], []
    for case, (host, ref) in zip(cases, refs):
        cid = ar.part_case_id(case)
        for k, (x64, bds, scales) in ref.items():
            ncol = len(bds)
            x = np.full((ncol, nc, nd), np.nan)
            for r, d in enumerate(data):
                x[:, d["cells"]] = d["%s|%d" % (cid, k)]
                for flag in ("same", "independent") if case[0] == "knp" else ("same",):
                    if not bool(d["%s|%d|%s" % (cid, k, flag)]):
                        flags.append((cid, k, r, flag))
            x = x.reshape(ncol, -1)
            assert np.isfinite(x).all()
            for s in range(ncol):
                err = np.abs(x[s] - x64[s]).max()
                print("AMGPAR part %-14s %-6s %-34s col %d k=%d bound %.2e err %.2e ratio %.3f" % (group, pname, cid, s, k, bds[s] / scales[s],
                                                                                                   err / scales[s], err / bds[s]))
                if not err <= bds[s]:
                    bad.append((cid, k, s, err / bds[s]))
    assert not flags, ("a second identical solve gave other bits / species are not independent", flags)
    assert not bad, (group, pname, bad)
