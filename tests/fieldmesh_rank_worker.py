"""One rank of the several-ranks refusal in tests/test_gpu_fieldmesh.py: a partitioned solver on the shared-memory communicator must
refuse a field-mesh sampler, at the Solver level and at the C ABI, without entering a collective.
usage: fieldmesh_rank_worker.py rank world shm_name"""
import os
import sys

import numpy as np

rank, world, name = int(sys.argv[1]), int(sys.argv[2]), sys.argv[3]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "knp-emi-dg_amd"), os.path.join(ROOT, "examples", "idealized_geometries")]
os.environ["WORLD_SIZE"] = str(world)
os.environ["KNP_COMM_SHM"] = name
os.environ["KNP_NO_AMG"] = "1"          # no hierarchy helpers: this worker never solves
from idealized_common import SolverIdealized, physical_setup                                       # noqa: E402
from knpemidg import _abi as A                                                                      # noqa: E402
from knpemidg.mesh import make_mesh_3D                                                              # noqa: E402
from knpemidg.models import mm_hh, mm_hh_no_stim                                                    # noqa: E402
from knpemidg.partition import distribute_solver                                                    # noqa: E402

params, ion_list, stim_params = physical_setup(1.0e-4)
S = distribute_solver(lambda: SolverIdealized(params, ion_list), make_mesh_3D(0, n_axons=4), {1: mm_hh, 2: mm_hh_no_stim}, stim_params,
                      rank, world, 0, None, method="slab")
seen = []
# two nodes of owned cells of this rank's context: one vertex value each
for call in (lambda: S.record_fields(), lambda: S.dev.fieldmesh_create(np.arange(3), [0, 1], [0, 0], [(A.FM_PHI, -1)])):
    try:
        call()
        seen.append("no error")
    except A.KnpError as e:
        seen.append(str(e))
S.dev.close()
print("\n".join(seen))
sys.exit(0 if all("several ranks" in s for s in seen) and "(-7)" in seen[1] and S.fieldmeshes is None else 3)
