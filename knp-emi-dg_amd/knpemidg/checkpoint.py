"""Checkpoint files of `Solver.save_checkpoint` / `resume=`: host part (no GPU needed).

One HDF5 file written through `h5lite.H5Writer` (readable by libhdf5, like the result files):

    /header/json            the header as UTF-8 JSON (uint8): format version, t, k, dt, ion names and valences, degrees, cell and vertex
                            counts, mesh hash, mode, solver_params, chosen EMI DG smoother, hierarchy-refresh counters, membrane-model
                            names / tags / state names / parameter names / hash of a run-time compiled right-hand side
    /header/{format_version, t, k, dt}   the same four numbers as datasets, for readers without a JSON parser
    /state/table            [n_blocks, 7] int64: id, kind, type, ncomp, count, width, offset of every state block (include/knpemi_hip.h)
    /state/block_<id>       the block, [ncomp, count, width] in its own element type; per-cell and per-facet blocks in the CALLER's numbering
    /solver/<name>          host-side state of the Solver, its membrane models and its recorder (iteration histories, load norm, ODE
                            times, rows already read back)

The device snapshot (`Device.state_save`) is one byte buffer: `split_snapshot` cuts it into the blocks above, `join_snapshot` puts
the identical bytes together again for `Device.state_load`.  A file is written under a temporary name in the target directory and
renamed over the final name only when complete.
"""
import hashlib
import json
import os

import numpy as np

from knpemidg._abi import KnpError
from knpemidg.h5lite import H5Error, H5File, H5Writer

FORMAT_VERSION = 1
PROLOGUE = 32                       # KNP_STATE_PROLOGUE
MAGIC = b"KNPSTATE"
# struct knp_state_block (include/knpemi_hip.h)
BLOCK_DTYPE = np.dtype([("id", "<i4"), ("kind", "<i4"), ("type", "<i4"), ("ncomp", "<i4"), ("count", "<i8"), ("width", "<i8"),
                        ("offset", "<i8")])
BLOCK_FIELDS = BLOCK_DTYPE.names
TYPE_DTYPE = {0: np.dtype("<f8"), 1: np.dtype("<f4"), 2: np.dtype("<i4"), 3: np.dtype("<i8")}      # enum knp_state_type
KIND_NAMES = {0: "opaque", 1: "cell_dof", 2: "facet", 3: "membrane_facet"}                         # enum knp_state_kind
# order in which `check_header` compares; the first difference is the one reported
CHECKED_FIELDS = ("format_version", "mesh_hash", "n_cells", "n_vertices", "ions", "degrees", "dt", "mode", "models", "rtc_hash")


def _align256(n):
    return (int(n) + 255) & ~255


def mesh_hash(coords, cells):
    """SHA-256 of the vertex coordinates (float64) and the cell connectivity (int64), caller's numbering."""
    h = hashlib.sha256()
    h.update(np.ascontiguousarray(coords, dtype="<f8").tobytes())
    h.update(np.ascontiguousarray(cells, dtype="<i8").tobytes())
    return h.hexdigest()


def source_hash(text):
    """SHA-256 of a run-time compiled model's HIP_RHS string (None for a built-in model)."""
    return None if text is None else hashlib.sha256(str(text).encode()).hexdigest()


def split_snapshot(buf):
    """(table, arrays): the block table (BLOCK_DTYPE) of a snapshot and one array [ncomp, count, width] per block (copies)."""
    buf = np.ascontiguousarray(buf, dtype=np.uint8)
    raw = buf.tobytes()
    if len(raw) < PROLOGUE or raw[:8] != MAGIC:
        raise KnpError("not a state snapshot")
    n = int(np.frombuffer(raw, dtype="<i4", count=1, offset=12)[0])
    total = int(np.frombuffer(raw, dtype="<i8", count=1, offset=16)[0])
    if total != len(raw):
        raise KnpError("state snapshot: %d bytes announced, %d present" % (total, len(raw)))
    table = np.frombuffer(raw, dtype=BLOCK_DTYPE, count=n, offset=PROLOGUE).copy()
    arrays = []
    for b in table:
        dt = TYPE_DTYPE[int(b["type"])]
        shape = (int(b["ncomp"]), int(b["count"]), int(b["width"]))
        cnt = shape[0] * shape[1] * shape[2]
        if int(b["offset"]) + cnt * dt.itemsize > len(raw):
            raise KnpError("state snapshot: block %d runs past the end" % int(b["id"]))
        arrays.append(np.frombuffer(raw, dtype=dt, count=cnt, offset=int(b["offset"])).reshape(shape).copy())
    return table, arrays


def join_snapshot(table, arrays):
    """The snapshot bytes (uint8 array) of a block table and its arrays: what `split_snapshot` was given, byte for byte."""
    table = np.ascontiguousarray(table, dtype=BLOCK_DTYPE)
    if len(arrays) != len(table):
        raise KnpError("state snapshot: %d blocks in the table, %d arrays" % (len(table), len(arrays)))
    total = _align256(PROLOGUE + BLOCK_DTYPE.itemsize * len(table))
    for b, a in zip(table, arrays):
        dt = TYPE_DTYPE[int(b["type"])]
        shape = (int(b["ncomp"]), int(b["count"]), int(b["width"]))
        if tuple(np.shape(a)) != shape or np.asarray(a).dtype != dt:
            raise KnpError("state snapshot: block %d is %s %s, its table entry says %s %s"
                           % (int(b["id"]), np.asarray(a).dtype, tuple(np.shape(a)), dt, shape))
        total = max(total, int(b["offset"]) + _align256(dt.itemsize * shape[0] * shape[1] * shape[2]))
    out = np.zeros(total, dtype=np.uint8)
    out[:8] = np.frombuffer(MAGIC, dtype=np.uint8)
    out[8:12] = np.frombuffer(np.asarray([FORMAT_VERSION], dtype="<i4").tobytes(), dtype=np.uint8)
    out[12:16] = np.frombuffer(np.asarray([len(table)], dtype="<i4").tobytes(), dtype=np.uint8)
    out[16:24] = np.frombuffer(np.asarray([total], dtype="<i8").tobytes(), dtype=np.uint8)
    out[PROLOGUE:PROLOGUE + table.nbytes] = np.frombuffer(table.tobytes(), dtype=np.uint8)
    for b, a in zip(table, arrays):
        raw = np.ascontiguousarray(a).tobytes()
        out[int(b["offset"]):int(b["offset"]) + len(raw)] = np.frombuffer(raw, dtype=np.uint8)
    return out


def _table_rows(table):
    return np.stack([np.asarray(table[f], dtype=np.int64) for f in BLOCK_FIELDS], axis=1).reshape(len(table), len(BLOCK_FIELDS))


def _table_from_rows(rows):
    table = np.zeros(len(rows), dtype=BLOCK_DTYPE)
    for j, f in enumerate(BLOCK_FIELDS):
        table[f] = rows[:, j]
    return table


def write_checkpoint(path, header, table, arrays, extra=None):
    """Write one checkpoint.  header: JSON-serialisable dict (t, k, dt, ... ; format_version is added); table / arrays: the state
    blocks (`split_snapshot`); extra: {name: numeric array} of host-side state, stored under /solver.  The file appears under
    `path` only when it is complete: an exception on the way leaves whatever was there before."""
    header = dict(header, format_version=FORMAT_VERSION)
    path = os.fspath(path)
    folder = os.path.dirname(os.path.abspath(path))
    os.makedirs(folder, exist_ok=True)
    tmp = os.path.join(folder, ".%s.tmp%d" % (os.path.basename(path), os.getpid()))
    w = None
    try:
        w = H5Writer(tmp)
        w.write("/header/json", np.frombuffer(json.dumps(header, sort_keys=True).encode(), dtype=np.uint8))
        w.write("/header/format_version", np.asarray([FORMAT_VERSION], dtype=np.int64))
        w.write("/header/t", np.asarray([float(header["t"])]))
        w.write("/header/k", np.asarray([int(header["k"])], dtype=np.int64))
        w.write("/header/dt", np.asarray([float(header["dt"])]))
        w.write("/state/table", _table_rows(np.ascontiguousarray(table, dtype=BLOCK_DTYPE)))
        for b, a in zip(table, arrays):
            if np.size(a):
                w.write("/state/block_%d" % int(b["id"]), a)
        for name, a in (extra or {}).items():
            a = np.asarray(a)
            if a.size:
                w.write("/solver/" + name, a)
        w.close()
        w = None
        os.replace(tmp, path)
    finally:
        if w is not None and w.fh is not None:
            w.fh.close()
        if os.path.exists(tmp):
            os.remove(tmp)
    return path


def read_checkpoint(path):
    """(header dict, table, arrays, extra dict) of a file written by `write_checkpoint`."""
    try:
        f = H5File(os.fspath(path))
        header = json.loads(f.read("header/json").tobytes().decode())
    except (OSError, KeyError, ValueError, H5Error) as e:
        raise KnpError("%s is not a checkpoint file: %s" % (path, e))
    if int(header.get("format_version", -1)) != FORMAT_VERSION:
        raise KnpError("checkpoint %s: field format_version is %s, this build reads %d" % (path, header.get("format_version"), FORMAT_VERSION))
    table = _table_from_rows(f.read("state/table"))
    arrays = []
    for b in table:
        name = "state/block_%d" % int(b["id"])
        shape = (int(b["ncomp"]), int(b["count"]), int(b["width"]))
        dt = TYPE_DTYPE[int(b["type"])]
        arrays.append(f.read(name).astype(dt, copy=False).reshape(shape) if name in f.datasets else np.zeros(shape, dtype=dt))
    extra = {name[len("solver/"):]: f.read(name) for name in f.datasets if name.startswith("solver/")}
    return header, table, arrays, extra


def check_header(saved, current, what="checkpoint"):
    """KnpError naming the FIRST field of CHECKED_FIELDS in which the saved header differs from the solver's."""
    for key in CHECKED_FIELDS:
        a, b = saved.get(key), current.get(key)
        if json.dumps(a, sort_keys=True) != json.dumps(b, sort_keys=True):
            raise KnpError("%s does not match this solver: field '%s' is %s in the file and %s here"
                           % (what, key, _short(a), _short(b)))


def check_table(saved, current, what="checkpoint"):
    """KnpError naming the first state block in which a saved block table differs from the device's own."""
    n = min(len(saved), len(current))
    for i in range(n):                                             # shapes first: an offset also moves when a LATER block differs
        if tuple(saved[i])[:6] != tuple(current[i])[:6]:
            s, c = saved[i], current[i]
            raise KnpError("%s does not match this solver: state block %d (%s) is [%d][%d][%d] in the file and block %d [%d][%d][%d] here"
                           % (what, int(s["id"]), KIND_NAMES.get(int(s["kind"]), "?"), int(s["ncomp"]), int(s["count"]), int(s["width"]),
                              int(c["id"]), int(c["ncomp"]), int(c["count"]), int(c["width"])))
    if len(saved) != len(current):
        raise KnpError("%s does not match this solver: %d state blocks in the file, %d here (membrane-model or recorder layout)"
                       % (what, len(saved), len(current)))
    if saved.tobytes() != np.ascontiguousarray(current, dtype=BLOCK_DTYPE).tobytes():
        raise KnpError("%s does not match this solver: the state blocks sit at other offsets" % what)


def _short(v):
    s = json.dumps(v, sort_keys=True)
    return s if len(s) <= 120 else s[:117] + "..."
