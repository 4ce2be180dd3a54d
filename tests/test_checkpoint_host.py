"""Checkpoint files without a GPU (knpemidg/checkpoint.py): a synthetic block list survives the file byte for byte, an interrupted
write leaves the previous file, every header mismatch is named, and the library exports the state entry points."""
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _synthetic(seed=0, nc=37, nd=4, nf=91, nmf=13):
    """A snapshot as the library lays it out: device blocks first, 256-byte aligned, host counters behind them."""
    from knpemidg import checkpoint as ck
    rng = np.random.default_rng(seed)
    spec = [(1, 1, 0, 1, nc, nd), (2, 1, 0, 2, nc, nd), (10, 1, 1, 1, nc, nd * nd), (5, 2, 0, 3, nf, 1), (1000, 3, 0, 1, nmf, 4),
            (1008, 3, 0, 1, 0, 4), (2004, 3, 2, 1, nmf, 1), (12, 0, 3, 1, 11, 1)]
    table = np.zeros(len(spec), dtype=ck.BLOCK_DTYPE)
    arrays = []
    off = (ck.PROLOGUE + ck.BLOCK_DTYPE.itemsize * len(spec) + 255) & ~255
    for i, (bid, kind, typ, ncomp, count, width) in enumerate(spec):
        dt = ck.TYPE_DTYPE[typ]
        table[i] = (bid, kind, typ, ncomp, count, width, off)
        shape = (ncomp, count, width)
        a = rng.standard_normal(shape).astype(dt) if dt.kind == "f" else rng.integers(-5, 5, size=shape).astype(dt)
        if dt.kind == "f" and a.size:
            a.flat[0] = np.nan                                   # bits, not values, must survive
        arrays.append(a)
        off += (dt.itemsize * ncomp * count * width + 255) & ~255
    return table, arrays


def _header(**over):
    h = {"t": 4e-4, "k": 4, "dt": 1e-4, "ions": [["K", 1.0], ["Cl", -1.0], ["Na", 1.0]], "degrees": [1, 1], "n_cells": 37, "n_vertices": 20,
         "mesh_hash": "ab" * 32, "mode": "splitting", "models": [{"name": "mm_hh", "tag": 1, "nodes": 13, "on_device": True,
                                                                  "states": ["m", "h", "n", "V"], "parameters": 17}],
         "rtc_hash": [None], "solver_params": {"rtol_emi": 1e-5}, "emi_dg_chebyshev": True, "emi_trial_pending": False,
         "amg_refresh": {"solves": 4, "ref": 3, "high": 0, "refreshes": 0}}
    h.update(over)
    return h


def test_snapshot_split_and_join_are_inverse():
    from knpemidg import checkpoint as ck
    table, arrays = _synthetic()
    buf = ck.join_snapshot(table, arrays)
    t2, a2 = ck.split_snapshot(buf)
    assert t2.tobytes() == table.tobytes()
    assert all(x.tobytes() == y.tobytes() and x.dtype == y.dtype and x.shape == y.shape for x, y in zip(arrays, a2))
    assert ck.join_snapshot(t2, a2).tobytes() == buf.tobytes()
    assert ck.BLOCK_DTYPE.itemsize == 40                          # struct knp_state_block: 4 x int32 + 3 x int64
    hdr = open(os.path.join(ROOT, "include", "knpemi_hip.h")).read()
    assert "#define KNP_STATE_PROLOGUE %d" % ck.PROLOGUE in hdr
    with pytest.raises(ck.KnpError):
        ck.split_snapshot(np.zeros(64, dtype=np.uint8))


def test_checkpoint_file_round_trip_is_byte_identical(tmp_path):
    from knpemidg import checkpoint as ck
    table, arrays = _synthetic(seed=3)
    extra = {"emi_niter": np.arange(4, dtype=np.int64), "knp_bnorm": np.asarray([1.5, 2.5]), "empty": np.zeros(0)}
    path = str(tmp_path / "sub" / "ck.h5")
    assert ck.write_checkpoint(path, _header(), table, arrays, extra) == path
    assert os.listdir(os.path.dirname(path)) == ["ck.h5"]        # no temporary file left behind
    header, t2, a2, e2 = ck.read_checkpoint(path)
    assert header == dict(_header(), format_version=ck.FORMAT_VERSION)
    assert header["t"] == 4e-4 and header["dt"] == 1e-4           # exact: a resumed t must be the straight run's
    assert t2.tobytes() == table.tobytes()
    for x, y in zip(arrays, a2):
        assert x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes()
    assert ck.join_snapshot(t2, a2).tobytes() == ck.join_snapshot(table, arrays).tobytes()
    assert set(e2) == {"emi_niter", "knp_bnorm"} and np.array_equal(e2["emi_niter"], extra["emi_niter"])
    try:
        import h5py
    except ImportError:
        h5py = None
    if h5py is not None:                                         # libhdf5 reads what h5lite wrote
        with h5py.File(path, "r") as f:
            assert float(f["header/t"][0]) == 4e-4 and int(f["header/k"][0]) == 4
            assert np.array_equal(f["state/block_5"][...], arrays[3])
    with pytest.raises(ck.KnpError):
        ck.read_checkpoint(os.path.join(ROOT, "include", "knpemi_hip.h"))


def test_interrupted_write_keeps_the_previous_checkpoint(tmp_path, monkeypatch):
    from knpemidg import checkpoint as ck
    path = str(tmp_path / "ck.h5")
    table, arrays = _synthetic(seed=1)
    real_write = ck.H5Writer.write
    calls = []

    def failing(self, name, array):
        calls.append(name)
        if len(calls) == 9:                                      # midway through the state blocks
            raise OSError("disk full")
        return real_write(self, name, array)

    monkeypatch.setattr(ck.H5Writer, "write", failing)
    with pytest.raises(OSError):
        ck.write_checkpoint(path, _header(), table, arrays)
    assert len(calls) == 9 and calls[-1].startswith("/state/block_")
    assert os.listdir(str(tmp_path)) == []                       # neither the final name nor a temporary one
    monkeypatch.setattr(ck.H5Writer, "write", real_write)
    ck.write_checkpoint(path, _header(k=4), table, arrays)
    before = open(path, "rb").read()
    del calls[:]
    monkeypatch.setattr(ck.H5Writer, "write", failing)
    with pytest.raises(OSError):
        ck.write_checkpoint(path, _header(k=8), *_synthetic(seed=2))
    assert os.listdir(str(tmp_path)) == ["ck.h5"] and open(path, "rb").read() == before
    monkeypatch.setattr(ck.H5Writer, "write", real_write)
    assert ck.read_checkpoint(path)[0]["k"] == 4


@pytest.mark.parametrize("field,change", [
    ("mesh_hash", {"mesh_hash": "cd" * 32}),
    ("ions", {"ions": [["K", 1.0], ["Cl", -1.0], ["Ca", 2.0]]}),
    ("degrees", {"degrees": [2, 2]}),
    ("dt", {"dt": 2e-4}),
    ("mode", {"mode": "passive"}),
    ("models", {"models": [{"name": "mm_hh", "tag": 2, "nodes": 13, "on_device": True, "states": ["m", "h", "n", "V"], "parameters": 17}]}),
    ("rtc_hash", {"rtc_hash": ["0" * 64]}),
])
def test_header_mismatch_names_the_field(field, change):
    import rtc_models
    from knpemidg import checkpoint as ck
    saved = dict(_header(), format_version=ck.FORMAT_VERSION)
    ck.check_header(saved, dict(saved))                          # equal headers pass
    ck.check_header(saved, dict(saved, t=1.0, k=9, solver_params=None))   # what is not compared may differ
    with pytest.raises(ck.KnpError, match="field '%s'" % field):
        ck.check_header(saved, dict(saved, **change))
    # the first differing field in the documented order is the one named
    with pytest.raises(ck.KnpError, match="field 'mesh_hash'"):
        ck.check_header(saved, dict(saved, **dict(change, mesh_hash="ef" * 32)))
    assert ck.source_hash(None) is None and ck.source_hash(rtc_models.FHN_BODY) != ck.source_hash(rtc_models.FHN_BODY + " ")
    assert len(ck.source_hash(rtc_models.FHN_BODY)) == 64


def test_block_table_mismatch_names_the_block():
    from knpemidg import checkpoint as ck
    table, _ = _synthetic()
    ck.check_table(table, table.copy())
    other = table.copy()
    other[2]["width"] = 100                                      # another degree: nd * nd of the block inverses
    with pytest.raises(ck.KnpError, match="state block 10"):
        ck.check_table(table, other)
    with pytest.raises(ck.KnpError, match="state blocks"):
        ck.check_table(table, table[:-1])


def test_mesh_hash_sees_coordinates_and_connectivity():
    from knpemidg import checkpoint as ck
    from knpemidg.mesh import make_mesh_2D
    mesh = make_mesh_2D(0)[0]
    h = ck.mesh_hash(mesh.coords, mesh.cells)
    assert h == ck.mesh_hash(mesh.coords.copy(), mesh.cells.astype(np.int32))
    moved = mesh.coords.copy(); moved[0, 0] += 1e-12
    cells = mesh.cells.copy(); cells[[0, 1]] = cells[[1, 0]]
    assert len({h, ck.mesh_hash(moved, mesh.cells), ck.mesh_hash(mesh.coords, cells)}) == 3


def test_library_exports_the_state_entry_points():
    import build as _b
    _b.build()
    from knpemidg import _abi
    lib = _abi.load()
    hdr = open(os.path.join(ROOT, "include", "knpemi_hip.h")).read()
    declared = set(re.findall(r"\b(knp_state_[a-z0-9_]+)\s*\(", hdr))
    assert {"knp_state_describe", "knp_state_save", "knp_state_load"} <= declared
    for name in declared:
        assert hasattr(lib, name) and name in _abi.SIGNATURES, name
    for name in ("save_checkpoint", "load_checkpoint"):
        from knpemidg import Solver
        assert callable(getattr(Solver, name))
    import inspect
    for fn in (Solver.solve_system_active, Solver.solve_system_passive):
        p = inspect.signature(fn).parameters
        for name in ("checkpoint_every", "checkpoint_file", "resume"):
            assert p[name].kind is inspect.Parameter.KEYWORD_ONLY and p[name].default is None
