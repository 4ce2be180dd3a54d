"""One rank of tests/test_gpu_amg_partition.py: the Krylov iterates x_k of a partitioned device context (several ranks on one GPU over the
shared-memory communicator) for every case of one group and partition of amg_ref.PART_GROUPS.  The rank builds the GLOBAL problem
(same seeds on every rank), takes its part -- owned cells and one ghost layer, coefficients and state sliced from the global arrays --,
joins the communicator, installs the halo tables and the shared-dof tables, uploads the localized production hierarchy and the global
right-hand side restricted to its cells, solves k iterations from x_0 = 0 at a tolerance that cannot be reached, and writes its owned
rows.  KNP_AMG_DIST0=0: the hierarchy replicated behind an all-reduce of the level-0 right-hand side.
usage: amg_partition_worker.py rank world shm_name outdir group partition"""
import os
import sys

import numpy as np

rank, world, name, outdir, group, pname = int(sys.argv[1]), int(sys.argv[2]), sys.argv[3], sys.argv[4], sys.argv[5], sys.argv[6]
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path[:0] = [os.path.join(ROOT, "knp-emi-dg_amd"), os.path.join(ROOT, "oracle"), HERE]
import amg_ref as ar                                                                                # noqa: E402
from common import device_for, push_state                                                           # noqa: E402
from knpemidg import _abi as A, amg                                                                 # noqa: E402

_, mesh_name, dist0, parts = ar.part_group(group)
assert (os.environ.get("KNP_AMG_DIST0", "1") != "0") == dist0 and os.environ.get("KNP_AMG_MAXCOARSE") == ar.PART_MAXCOARSE
cases = parts[pname]
out = {}


def fail_solve(fn):
    try:
        fn()
    except A.KnpError as e:
        assert "did not converge" in str(e), e
        return
    raise AssertionError("the solve converged at a tolerance it cannot reach")


class Rank:
    """this rank's device context of one host (mesh, ions, potential)"""

    def __init__(self, key, index):
        self.host = host = ar.Host(*key)
        mesh = host.mt[0]
        self.part = part = ar.part_partition(mesh, pname)
        assert part.world == world
        self.loc = loc = part.local(rank)
        self.pb = pbl = host.local_problem(loc)
        self.no, self.cg, self.nd, self.ns = loc.nc_owned, loc.cells_global, pbl.nd, pbl.N_ions
        self.dev = dev = device_for(pbl, nc_owned=self.no)
        if pname == "thin3":
            assert (dev.n_interior == 0) == (rank == 1), (rank, dev.n_interior)     # the middle slab: every cell touches a cut
        # segment sizes as knpemidg.partition.distribute_solver has them (from global quantities only: the same on every rank)
        ncg_bound = 4 * (mesh.coords.shape[0] + 8 * mesh.num_cells() // 4)
        most_sent = max(sum(len(sl) for sl in part.local(r).send_lists) for r in range(world))
        dev.comm_init_shm(rank, world, "%s_%d" % (name, index), max(ncg_bound, 1 << 16), max(most_sent, 1) * 7 * self.nd * 4)
        dev.halo_tables(loc.peers, loc.send_lists, loc.recv_offsets, loc.recv_counts)
        push_state(dev, pbl)
        dev.update_kappa()
        dev.emi_rhs()
        dev.update_dnphi()
        dev.knp_rhs()
        self.d0 = None
        if dist0:
            mem = np.nonzero((mesh.facet_cells[:, 1] >= 0) & np.isin(np.asarray(host.mt[2].array()), [1]))[0]
            self.d0 = amg.Dist0Space(host.cs2 or host.cs, part.owner, mem, rank, world)
            dev.amg_interface(self.d0.n, *self.d0.interface_tables())

    def local(self, v):
        """[columns, global DG dofs] -> this rank's cells (owned, then ghosts)"""
        return np.ascontiguousarray(np.asarray(v).reshape(-1, self.host.pb.mesh.num_cells(), self.nd)[:, self.cg])

    def owned(self, v, ncol):
        return np.asarray(v).reshape(ncol, -1, self.nd)[:, :self.no].copy()

    def upload_levels(self, slot, levels, ncol):
        if self.d0 is not None:
            self.dev.amg_upload(slot, self.d0.local_dg2cg(self.cg), self.d0.localize(levels), ncol=ncol, dist0=True)
        else:
            self.dev.amg_upload(slot, self.host.dg2cg[self.cg], levels, ncol=ncol)

    def emi(self, k, b):
        dev = self.dev
        dev.upload(A.F_B_EMI, b)
        dev.upload(A.F_PHI, np.zeros(self.pb.ndof))                      # x_0 = 0; also drops the extrapolation history
        fail_solve(lambda: dev.emi_solve(1e-30, maxit=k, check_every=1))
        return self.owned(dev.download(A.F_PHI), 1)

    def knp(self, k, b, keep_bound=False):
        dev = self.dev
        dev.upload(A.F_B_KNP, b)
        zero = np.zeros(self.ns * self.pb.ndof)
        if keep_bound:                                                  # x_0 = 0 without a state upload: the spectral bound is kept
            dev.upload(A.F_X, zero)
            dev.copy_field(A.F_C, A.F_X)
        else:
            dev.upload(A.F_C, zero)
        fail_solve(lambda: dev.knp_solve(1e-30, maxit=k, min_it=0, check_every=1))
        return self.owned(dev.download(A.F_C), self.ns)

    def run(self, case):
        cid, dev, host = ar.part_case_id(case), self.dev, self.host
        levels = ar.part_levels(host, case)
        if case[0] == "emi":
            b = self.local(host.ref.b_emi)
            dev.emi_residual_target(0.0)
            self.upload_levels(0, levels, 1)
            dev.set_emi_dg_smoother(case[2])
            try:
                for k in case[-1]:
                    x, again = self.emi(k, b), self.emi(k, b)
                    out["%s|%d" % (cid, k)] = x
                    out["%s|%d|same" % (cid, k)] = np.array_equal(x, again)
            finally:
                dev.set_emi_dg_smoother(None)
                dev.amg_clear(0)
            return
        ns = self.ns
        assert ns == case[1] and (host.peclet() > 0.5 if case[2] == "cell" else host.peclet() <= 0.4)
        b = self.local(np.stack(host.knp()[2]))
        b2 = b.copy()
        b2[1] *= 1.0 + 1e-3 * np.random.default_rng(17).uniform(-1.0, 1.0, size=b2[1].shape)
        for s in range(ns):
            dev.amg_clear(1 + s)
        self.upload_levels(1, levels, ns)
        if case[4] is not None:
            dev.set_knp_krylov("gmres", case[4])
        keep = [s for s in range(ns) if s != 1]
        try:
            for k in case[-1]:
                x, again, other = self.knp(k, b), self.knp(k, b), self.knp(k, b2, keep_bound=True)
                out["%s|%d" % (cid, k)] = x
                out["%s|%d|same" % (cid, k)] = np.array_equal(x, again)
                out["%s|%d|independent" % (cid, k)] = np.array_equal(other[keep], x[keep]) and not np.array_equal(other[1], x[1])
        finally:
            dev.set_knp_krylov("bicgstab")
            for s in range(ns):
                dev.amg_clear(1 + s)


ranks = {}
try:
    for case in cases:
        key = ar.part_host_key(mesh_name, case)
        if key not in ranks:
            ranks[key] = Rank(key, len(ranks))
        ranks[key].run(case)
        print("rank %d: %s done" % (rank, ar.part_case_id(case)), flush=True)
    np.savez(os.path.join(outdir, "rank%d.npz" % rank), cells=next(iter(ranks.values())).cg[:next(iter(ranks.values())).no], **out)
finally:
    for r in ranks.values():
        r.dev.close()
