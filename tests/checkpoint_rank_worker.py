"""One rank of the several-ranks refusal in tests/test_gpu_checkpoint.py: a partitioned solver on the shared-memory communicator must
refuse to write a checkpoint, at the Solver level and at the C ABI, without entering a collective.
usage: checkpoint_rank_worker.py rank world shm_name outdir"""
import os
import sys

rank, world, name, outdir = int(sys.argv[1]), int(sys.argv[2]), sys.argv[3], sys.argv[4]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "knp-emi-dg_amd"), os.path.join(ROOT, "examples", "idealized_geometries")]
os.environ["WORLD_SIZE"] = str(world)
os.environ["KNP_COMM_SHM"] = name
os.environ["KNP_NO_AMG"] = "1"          # no hierarchy helpers: this worker never solves
from idealized_common import SolverIdealized, physical_setup                                       # noqa: E402
from knpemidg._abi import KnpError                                                                  # noqa: E402
from knpemidg.mesh import make_mesh_3D                                                              # noqa: E402
from knpemidg.models import mm_hh, mm_hh_no_stim                                                    # noqa: E402
from knpemidg.partition import distribute_solver                                                    # noqa: E402

params, ion_list, stim_params = physical_setup(1.0e-4)
S = distribute_solver(lambda: SolverIdealized(params, ion_list), make_mesh_3D(0, n_axons=4), {1: mm_hh, 2: mm_hh_no_stim}, stim_params,
                      rank, world, 0, None, method="slab")
path = os.path.join(outdir, "rank%d.h5" % rank)
seen = []
for call in (lambda: S.save_checkpoint(path), lambda: S.dev.state_save(), lambda: S.load_checkpoint(path)):
    try:
        call()
        seen.append("no error")
    except KnpError as e:
        seen.append(str(e))
S.dev.close()
print("\n".join(seen))
ok = all("several ranks" in s for s in seen) and not os.path.exists(path)
sys.exit(0 if ok else 3)
