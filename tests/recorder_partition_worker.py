"""One rank of tests/test_gpu_recorder_partition.py: the partitioned idealized 3D solver on the shared-memory communicator (several
ranks on one GPU) with a recorder attached; a few stimulated steps at tight tolerances.  Writes the recorder's results as this rank
sees them and, per step, what it owns -- its cells' fields, its membrane facets' phi_M / E / I_ch and gating variables -- for the
parent to evaluate every channel on the host.
usage: recorder_partition_worker.py rank world shm_name outdir case capacity mode     (mode: steps | file)"""
import os
import sys

import numpy as np

rank, world, name, outdir, case, capacity, mode = int(sys.argv[1]), int(sys.argv[2]), sys.argv[3], sys.argv[4], sys.argv[5], int(sys.argv[6]), sys.argv[7]
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path[:0] = [os.path.join(ROOT, "knp-emi-dg_amd"), os.path.join(ROOT, "examples", "idealized_geometries"), HERE]
os.environ["WORLD_SIZE"] = str(world)
os.environ["KNP_COMM_SHM"] = name
import recorder_partition_cases as PC                                                               # noqa: E402
from idealized_common import SolverIdealized, physical_setup, solver_parameters, Constant          # noqa: E402
from knpemidg import recorder as R                                                                  # noqa: E402
from knpemidg.models import mm_hh, mm_hh_no_stim                                                    # noqa: E402
from knpemidg.partition import distribute_solver                                                    # noqa: E402

# arguments and tables first, on the host: whatever can be refused is refused here, on every rank alike, before the first collective
_, method, fractions, n_axons, deg = PC.CASES.get(case) or PC.MORE_CASES[case]
assert world == _ and mode in ("steps", "file") and capacity >= 1
mesh_tuple, part, mtags, _ = PC.make_case(case)
args, info = PC.record_args(mesh_tuple, part, mtags)
extra = dict(membrane_states=PC.STATES, membrane_map=dict(threshold=PC.MAP_THRESHOLD))
pre = R.Recorder(mesh_tuple[0], mesh_tuple[1].array(), mesh_tuple[2].array(), deg, ["K", "Cl", "Na"], capacity=capacity, membrane_tags=mtags,
                 **args, **extra)
R.localize_tables(pre, part.local(rank))

ode_models = {1: mm_hh, 2: mm_hh_no_stim} if n_axons > 1 else {1: mm_hh}
params, ion_list, stim_params = physical_setup(1.0e-4)
S = distribute_solver(lambda: SolverIdealized(params, ion_list, degree_emi=deg, degree_knp=deg), mesh_tuple, ode_models, stim_params,
                      rank, world, 0, None, method=method, fractions=fractions)
# the measured choice of the EMI smoother depends on timings: fixed here, so that two runs are the same computation
tight = solver_parameters(3, 0, emi_dg_chebyshev=True)._replace(rtol_emi=1e-10, rtol_knp=1e-12)
rec = S.record(capacity=capacity, **args, **extra)
T = rec.local
assert np.array_equal(rec.point_cells, pre.point_cells) and all(np.array_equal(a, b) for a, b in zip(rec.set_facets, pre.set_facets))
out = {}
t = Constant(0.0)
if mode == "file":
    S.solve_system_active(PC.N_STEPS * 1.0e-4, t, tight, filename=os.path.join(outdir, "run_"))
else:
    S._unpack_solver_params(tight)
    S.save_fields = S.save_solver_stats = False
    S.splitting_scheme = True
    S.setup_varform_emi(); S.setup_varform_knp(); S.setup_solver_emi(); S.setup_solver_knp()
    loc = S.local_mesh
    n_own, nc, nd = loc.nc_owned, loc.mesh.num_cells(), S.nd
    mem = info["mem"]
    mem = mem[T.facet_owner(mem) == rank]                      # the membrane facets this rank records
    lmem = T.facet_local(mem)
    models = [m['ode'] for m in S.mem_models]
    row_of = [np.searchsorted(np.asarray(m.facets), lmem) for m in models]
    of_model = [np.isin(lmem, np.asarray(m.facets)) for m in models]
    assert (np.sum(of_model, axis=0) == 1).all()
    cols = [[int(m.ode.state_indices(q)) for q in PC.STATES] for m in models]
    fields, membrane, states, times = [], [], [], []
    for k in range(PC.N_STEPS):
        S.step_membrane_models(k)
        if k == 0:
            rec.arm(float(t))
            out["v_arm"] = S.phi_M_prev_PDE.array()[lmem].copy()
        S.solve_for_time_step(k, t)
        times.append(float(t))
        f = [S.phi.array().reshape(nc, nd)] + list(S.c.array().reshape(-1, nc, nd)) + [S.ion_list[-1]['c'].array().reshape(nc, nd)]
        fields.append(np.stack([a[:n_own] for a in f]))
        E = [ion['E'].array() for ion in S.ion_list]
        Ich = [S.mem_models[0]['I_ch_k'][ion['name']].array() for ion in S.ion_list]
        membrane.append(np.stack([a[lmem] for a in [S.phi_M_prev_PDE.array()] + E + Ich]))
        st = np.full((len(PC.STATES), len(lmem)), np.nan)
        for m, rows, sel, cc in zip(models, row_of, of_model, cols):
            if sel.any():
                st[:, sel] = m.states[rows[sel]][:, cc].T
        states.append(st)
    out.update(cells=loc.cells_global[:n_own], mem=mem, fields=np.stack(fields), membrane=np.stack(membrane), states=np.stack(states),
               times=np.asarray(times))
# the reads are collective: every rank makes them, in this order
out.update(t=rec.t.copy(), rows=rec.rows.copy(), n_base=rec.n_base)
amap = rec.membrane_map
out.update({"map_" + k: v for k, v in amap.items()})
out["cv"] = rec.conduction_velocity(*PC.CV_SETS)
np.savez(os.path.join(outdir, "rank%d.npz" % rank), **out)
S.dev.close()
