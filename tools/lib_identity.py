"""Does another build of the library compute what the reference build computes?  Runs one case in one process with the library that
KNP_LIB_PATH selects (default: the in-tree one), default AMG preconditioner on, 4 time steps with the HH stimulus, and writes the
state_save() snapshot, c, phi and the iteration counts; `compare` then checks three such runs of every case -- the reference
library twice (parent, parent2: the yardstick) and the new one once (new) -- block by block.  Bit equality wherever the reference
equals itself; otherwise within four times the reference's own run-to-run difference.  (profiles/abi_split_identity.txt,
profiles/amg_split_identity.txt)

    KNP_LIB_PATH=/path/libknpemi_hip_parent.so python tools/lib_identity.py run 3d_p1 out/3d_p1_parent_r0.npz
    KNP_LIB_PATH=/path/libknpemi_hip_parent.so python tools/lib_identity.py run 3d_p1 out/3d_p1_parent2_r0.npz
    python tools/lib_identity.py run 3d_p1 out/3d_p1_new_r0.npz
    python tools/lib_identity.py compare out 3d_p1:1 dist0_2rank:2

cases: 3d_p1, 3d_p2 (3D r=0 four-axon mesh), 2d_p1 (2D r=2), emix, 3d_p1_unshared (KNP_AMG_SHARED=0: one hierarchy per species on
forked streams), 3d_p1_live (3d_p1 with everything a context may own alive: a runtime-compiled membrane model on tag 1, a recorder
with probes, sets, regions and state channels, a voxel grid; the recorder's rows and a frame per step are compared too),
dist0_2rank (3D r=1 P2 on two ranks over the shared-memory communicator, row-distributed level 0: start both ranks at once,
`run dist0_2rank OUT_r<rank>.npz <rank> 2 /shm_name`; state_save() refuses a partitioned context, so c, phi and the iteration counts
alone are compared there)."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run(case, out, rank=0, world=1, shm=None):

    sys.path[:0] = [os.path.join(ROOT, "knp-emi-dg_amd"), os.path.join(ROOT, "examples", "idealized_geometries"),
                    os.path.join(ROOT, "examples", "emix_simulations")]
    if case == "3d_p1_unshared":
        os.environ["KNP_AMG_SHARED"] = "0"
    if world > 1:
        os.environ["WORLD_SIZE"] = str(world)
        os.environ["KNP_COMM_SHM"] = shm
    from idealized_common import make_solver, solver_parameters, Constant          # noqa: E402

    if case == "emix":
        import emix_common
        S = emix_common.make_solver()
        sp = emix_common.solver_parameters()
    elif case == "dist0_2rank":
        from knpemidg.partition import make_distributed_solver
        S = make_distributed_solver(dim=3, resolution=1, rank=rank, world=world, local_rank=0, dist=None, degree=2)
        sp = solver_parameters(3, 1)
    elif case == "3d_p1_live":
        sys.path.insert(0, os.path.join(ROOT, "examples", "custom_membrane_model"))
        import mm_hh_q10
        from knpemidg.models import mm_hh_no_stim
        S = make_solver(dim=3, resolution=0, ode_models={1: mm_hh_q10, 2: mm_hh_no_stim})
        sp = solver_parameters(3, 0)
    elif case == "2d_p1":
        S = make_solver(dim=2, resolution=2)
        sp = solver_parameters(2, 2)
    else:
        S = make_solver(dim=3, resolution=0, degree=2 if case == "3d_p2" else 1)
        sp = solver_parameters(3, 0)
    S._unpack_solver_params(sp)
    S.save_fields = S.save_solver_stats = False
    S.splitting_scheme = True
    S.setup_varform_emi(); S.setup_varform_knp(); S.setup_solver_emi(); S.setup_solver_knp()
    t = Constant(0.0)
    extra = {}
    if case == "3d_p1_live":
        from knpemidg import recorder as R
        assert all(mm['ode'].on_device for mm in S.mem_models)
        mid, tags = S.mesh.cell_midpoints(), np.asarray(S.subdomains.array())
        mem = R.membrane_facets(S.mesh, S.surfaces.array(), [1])
        rec = S.record(points=[mid[np.nonzero(tags == 0)[0][3]], mid[np.nonzero(tags == 1)[0][3]]], membrane_sets=[mem[:65]], regions=True,
                       capacity=8, membrane_states=("n", "m", "h"))
        lo, hi = S.mesh.coords.min(axis=0), S.mesh.coords.max(axis=0)
        grid = S.record_grid(lo + 0.11 * (hi - lo), hi - 0.11 * (hi - lo), (13, 7, 5), fields=("phi", "K"))
        frames = []
    for k in range(4):
        S.step_membrane_models(k); S.solve_for_time_step(k, t)
        if case == "3d_p1_live":
            f = grid.sample()
            frames.append(np.stack([f["phi"], f["K"]]))
    S.dev.sync()
    if case == "3d_p1_live":
        extra = dict(rec_t=np.asarray(rec.t), rec_rows=np.asarray(rec.rows), frames=np.stack(frames))
        assert extra["rec_rows"].shape[0] == 4 and np.isfinite(extra["frames"]).all()
    np.savez(out, **extra, snapshot=S.dev.state_save() if world == 1 else np.zeros(0, dtype=np.uint8),   # (state_save: one rank only)
             c=np.asarray(S.c.array()), phi=np.asarray(S.phi.array()),
             emi=np.asarray(S.emi_niter, dtype=np.int64).ravel(), knp=np.asarray(S.knp_niter, dtype=np.int64).ravel())
    print("case %s rank %d lib %s done: emi %s knp %s" % (case, rank, os.environ.get("KNP_LIB_PATH", "in-tree"), list(S.emi_niter), [list(n) for n in S.knp_niter]), flush=True)
    S.dev.close() if hasattr(S.dev, "close") else None


def compare(d, specs):
    sys.path.insert(0, os.path.join(ROOT, "knp-emi-dg_amd"))
    from knpemidg.checkpoint import split_snapshot

    ok_all = True
    for spec in specs:
        case, nr = spec.split(":")
        for r in range(int(nr)):
            L = {w: np.load(os.path.join(d, "%s_%s_r%d.npz" % (case, w, r))) for w in ("parent", "parent2", "new")}
            tab, blocks = {}, {}
            for w in L:
                tab[w], blocks[w] = split_snapshot(L[w]["snapshot"]) if L[w]["snapshot"].size else (np.zeros(0), [])
            def same(a, b):
                return {"c": np.array_equal(L[a]["c"], L[b]["c"]), "phi": np.array_equal(L[a]["phi"], L[b]["phi"]),
                        "emi": np.array_equal(L[a]["emi"], L[b]["emi"]), "knp": np.array_equal(L[a]["knp"], L[b]["knp"]),
                        "blocks": [np.array_equal(x.view(np.uint8), y.view(np.uint8)) for x, y in zip(blocks[a], blocks[b])],
                        "table": tab[a].tobytes() == tab[b].tobytes(), "bytes": np.array_equal(L[a]["snapshot"], L[b]["snapshot"]),
                        "extra": all(np.array_equal(L[a][k], L[b][k]) for k in ("rec_t", "rec_rows", "frames") if k in L[a].files)}
            pp, pn = same("parent", "parent2"), same("parent", "new")
            yard = all(pp[k] for k in ("c", "phi", "emi", "knp", "table", "bytes", "extra")) and all(pp["blocks"])
            line = "%-15s rank %d  parent==parent' %s | new==parent: c %s phi %s, %d of %d snapshot blocks equal (whole snapshot %s, %d bytes), iteration counts emi %s knp %s (emi %s knp %s)" % (
                case, r, yard, pn["c"], pn["phi"], sum(pn["blocks"]), len(pn["blocks"]), pn["bytes"], L["new"]["snapshot"].size, pn["emi"], pn["knp"],
                L["new"]["emi"].tolist(), L["new"]["knp"].tolist())
            ok = all(pn[k] for k in ("c", "phi", "emi", "knp", "table", "bytes", "extra")) and all(pn["blocks"])
            if "frames" in L["new"].files:
                line += ", recorder rows and grid frames %s" % pn["extra"]
            if not yard:                                    # fall-back: within four times the parent's own run-to-run difference
                ok = True
                for f in ("c", "phi"):
                    own = np.abs(L["parent"][f] - L["parent2"][f]).max()
                    new = np.abs(L["parent"][f] - L["new"][f]).max()
                    line += "\n%-15s         %s: parent run-to-run max diff %.3e, new vs parent %.3e, within 4x: %s" % ("", f, own, new, new <= 4 * own)
                    ok = ok and new <= 4 * own
                for i, (x, y, z) in enumerate(zip(blocks["parent"], blocks["parent2"], blocks["new"])):
                    if x.dtype.kind == "f" and not pp["blocks"][i]:
                        own, new = np.abs(x - y).max(), np.abs(x - z).max()
                        line += "\n%-15s         block %d: parent run-to-run %.3e, new vs parent %.3e, within 4x: %s" % ("", i, own, new, new <= 4 * own)
                        ok = ok and new <= 4 * own
                    elif not pp["blocks"][i] or not pn["blocks"][i]:
                        line += "\n%-15s         block %d (not floating point): parent==parent' %s new==parent %s" % ("", i, pp["blocks"][i], pn["blocks"][i])
                        ok = ok and (pn["blocks"][i] or not pp["blocks"][i])
                line += "\n%-15s         iteration counts: parent==parent' emi %s knp %s" % ("", pp["emi"], pp["knp"])
            print(line + ("" if ok else "   <-- NOT OK"))
            ok_all &= ok
    print("ALL CASES OK" if ok_all else "SOME CASE NOT OK")
    return ok_all


if __name__ == "__main__":
    if sys.argv[1] == "run":
        run(sys.argv[2], sys.argv[3], *([int(sys.argv[4]), int(sys.argv[5]), sys.argv[6]] if len(sys.argv) > 4 else []))
    else:
        sys.exit(0 if compare(sys.argv[2], sys.argv[3:]) else 1)
