"""Writes the arrays knp_ctx_create and knp_set_params receive for the 768-tet one-axon box (tests/common.py: small_3d), in the
caller's numbering, as the binary file tools/check_context_tables.cpp reads; behind them the map dg2cg of the conforming P1 space
(the cell's vertices; ncg = number of vertices, in the header) that knp_amg_begin receives, for tools/check_amg_tables.cpp.
usage: python tools/dump_context_mesh.py OUT.bin"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "knp-emi-dg_amd"), os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)


def main(out):
    from common import small_3d
    mesh, sub, surf = small_3d()
    ctags = np.asarray(sub.array(), dtype=np.uint32)
    nc = mesh.cells.shape[0]
    D = np.stack([np.where(ctags == 1, d_in, d_out) for d_in, d_out in ((1.33e-9, 1.33e-9), (1.96e-9, 1.0e-9), (2.03e-9, 2.03e-9))])
    mtags = np.asarray([1], dtype=np.uint32)
    arrays = [np.asarray(mesh.coords, dtype=np.float64), np.asarray(mesh.cells, dtype=np.int32), ctags,
              np.asarray(mesh.facet_cells, dtype=np.int32), np.asarray(mesh.facet_local, dtype=np.int8),
              np.asarray(surf.array(), dtype=np.uint32), mtags, np.asarray(D, dtype=np.float64),
              np.asarray(mesh.cells, dtype=np.int32)]                  # dg2cg [nc][nd] of P1
    ncg = mesh.coords.shape[0]
    head = np.asarray([mesh.gdim, mesh.coords.shape[0], nc, nc, arrays[3].shape[0], len(mtags), D.shape[0], ncg], dtype=np.int64)
    with open(out, "wb") as f:
        f.write(head.tobytes())
        for a in arrays:
            b = np.ascontiguousarray(a).tobytes()
            f.write(b + b"\0" * (-len(b) % 8))


if __name__ == "__main__":
    main(sys.argv[1])
