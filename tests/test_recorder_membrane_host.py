"""Host side of the recorder's membrane additions (knpemidg/recorder.py): the entry lists of the state channels, the conduction
velocity on analytic travelling fronts and the save / reload round trip of the new datasets.  No GPU: the device is replaced by an
object with the recorder's handful of `rec_*` methods, fed with analytic data."""
import math
from types import SimpleNamespace

import numpy as np
import pytest

from common import small_3d

IONS = ["K", "Cl", "Na"]
U = 0.8                      # front speed in m/s
DT = 1.0e-6


class FakeDevice:
    """What Recorder needs of a device.  row_of(t) -> the channels of knp_rec_create; the state channels are evaluated from
    `tables` (handle -> [n, ns]) with the uploaded entry lists, the map arrays are whatever the test put into `map_arrays`."""

    def __init__(self, row_of, tables=None):
        self.row_of, self.tables = row_of, tables or {}
        self.entries, self.map_args, self.armed_at, self.map_arrays = None, None, None, None
        self._t, self._rows = [], []

    def rec_create(self, capacity, point_cell, point_w, set_ptr, set_facet, set_w, n_regions, region, vol):
        self.n_base = len(point_cell) * (len(IONS) + 1) + (len(set_ptr) - 1) * (1 + 2 * len(IONS)) + n_regions * (len(IONS) + 1)
        return self.n_base

    def rec_add_states(self, ptr, eh, er, ec, ew):
        self.entries = (ptr, eh, er, ec, ew)
        return self.n_base + len(ptr) - 1

    def rec_add_map(self, facets, threshold, repolarisation):
        self.map_args = (np.asarray(facets).copy(), threshold, repolarisation)

    def rec_map_arm(self, t0):
        self.armed_at = t0

    def rec_sample(self, t):
        row = list(self.row_of(t))
        if self.entries is not None:
            ptr, eh, er, ec, ew = self.entries
            row += [sum(ew[i] * self.tables[eh[i]][er[i], ec[i]] for i in range(ptr[s], ptr[s + 1])) for s in range(len(ptr) - 1)]
        self._t.append(t)
        self._rows.append(row)

    def rec_read(self):
        t, rows = np.asarray(self._t), np.asarray(self._rows)
        self._t, self._rows = [], []
        return t, rows

    def rec_map_read(self):
        return self.map_arrays


@pytest.fixture(scope="module")
def strip():
    """The 64 membrane facets of small_3d((7, 4, 4)) with two patches: midpoints left of 3 um and right of 4 um."""
    from knpemidg import recorder as R
    mesh, sub, surf = small_3d((7, 4, 4))
    mem = R.membrane_facets(mesh, surf.array(), [1])
    x = mesh.facet_midpoints()[mem, 0]
    a, b = mem[x < 3.0e-6], mem[x > 4.0e-6]
    assert len(mem) == 64 and len(a) >= 4 and len(b) >= 4
    return SimpleNamespace(mesh=mesh, sub=np.asarray(sub.array()), surf=np.asarray(surf.array()), mem=mem, a=a, b=b)


def _recorder(strip, sets, row_of=None, tables=None, **kw):
    from knpemidg import recorder as R
    rec = R.Recorder(strip.mesh, strip.sub, strip.surf, 1, IONS, membrane_sets=sets, regions=False, capacity=4, membrane_tags=[1], **kw)
    dev = FakeDevice(row_of or (lambda t: [0.0] * (7 * len(sets))), tables)
    return rec, dev


# ---------------------------------------------------------------------------------------------------------------------
# entry lists
# ---------------------------------------------------------------------------------------------------------------------
def test_state_entry_lists(strip):
    from knpemidg import recorder as R
    from knpemidg.models import mm_hh, mm_glial
    mem = strip.mem
    hh = SimpleNamespace(facets=np.sort(mem[::2]), ode=mm_hh, handle=3, tag=1)            # rows follow the ascending facet ids
    gl = SimpleNamespace(facets=np.sort(mem[1::2]), ode=mm_glial, handle=5, tag=2)
    sets = [hh.facets[[4, 1, 9]], mem[[7, 2, 12, 5]], gl.facets[:3]]                      # HH only, both models, glial only
    areas = [R.facet_areas(strip.mesh, f) for f in sets]
    ptr, eh, er, ec, ew = R.state_entries(sets[:2], areas[:2], [hh, gl], ["n", "V"])
    assert list(ptr) == [0, 3, 6, 8, 12]                   # (set 0: n, V), (set 1: n over its two HH facets, V over all four)
    # set 0, both names: the set's facet order, rows = positions in hh.facets, the model's columns, weights = areas / their sum
    for q, col in ((0, 2), (1, 3)):
        sl = slice(ptr[q], ptr[q + 1])
        assert list(eh[sl]) == [3, 3, 3] and list(er[sl]) == [4, 1, 9] and list(ec[sl]) == [col] * 3
        assert np.array_equal(ew[sl], areas[0] / areas[0].sum())
    # set 1 = mem[7], mem[2], mem[12], mem[5]: odd positions are glial (row = position // 2), even ones HH
    sl = slice(ptr[2], ptr[3])
    assert list(eh[sl]) == [3, 3] and list(er[sl]) == [1, 6] and list(ec[sl]) == [2, 2]
    assert np.array_equal(ew[sl], areas[1][[1, 2]] / areas[1][[1, 2]].sum())              # renormalised over exactly the HH facets
    sl = slice(ptr[3], ptr[4])
    assert list(eh[sl]) == [5, 3, 3, 5] and list(er[sl]) == [3, 1, 6, 2] and list(ec[sl]) == [0, 3, 3, 0]
    assert np.array_equal(ew[sl], areas[1] / areas[1].sum())
    for s in range(4):
        assert abs(math.fsum(ew[ptr[s]:ptr[s + 1]]) - 1.0) < 1e-15
    assert ptr.dtype == np.int64 and eh.dtype == np.int32 and er.dtype == np.int64 and ec.dtype == np.int32
    # a set whose facets all belong to a model without that state: an error that names both
    with pytest.raises(ValueError, match="membrane set 2.*'n'"):
        R.state_entries(sets, areas, [hh, gl], ["V", "n"])


def test_recorder_builds_states_and_map_tables(strip):
    from knpemidg import _abi as A
    from knpemidg.models import mm_hh
    model = SimpleNamespace(facets=np.sort(strip.mem), ode=mm_hh, handle=0, tag=1)
    tables = {0: np.random.default_rng(3).uniform(size=(64, 4))}
    rec, dev = _recorder(strip, [strip.a, strip.b], tables=tables, membrane_states=("n", "m", "h"),
                         membrane_map=dict(threshold=-0.02, tags=[1]))
    rec.attach(dev)
    assert np.array_equal(dev.map_args[0], strip.mem) and dev.map_args[1:] == (-0.02, -0.02)        # repolarisation None = threshold
    with pytest.raises(A.KnpError, match="membrane models"):
        rec.sample(0.0)                                                  # the models have not arrived yet
    rec.attach_states([model])
    with pytest.raises(A.KnpError, match="not armed"):
        rec.sample(0.0)
    rec.arm(0.25)
    assert dev.armed_at == 0.25
    rec.sample(1.0)
    assert rec.n_channels == 14 + 6 and rec.rows.shape == (1, 20)
    m = rec.membrane
    assert set(m) == {"phi_M", "E_K", "E_Cl", "E_Na", "I_ch_K", "I_ch_Cl", "I_ch_Na", "n", "m", "h"}
    rows = np.searchsorted(model.facets, strip.b)
    assert m["h"].shape == (1, 2) and m["h"][0, 1] == pytest.approx(rec.set_weights[1] @ tables[0][rows, 1], rel=1e-14)
    assert m["n"][0, 0] == pytest.approx(rec.set_weights[0] @ tables[0][np.searchsorted(model.facets, strip.a), 2], rel=1e-14)
    # a model whose tables stayed on the host
    rec2, dev2 = _recorder(strip, [strip.a], membrane_states=("n",))
    rec2.attach(dev2)
    with pytest.raises(A.KnpError, match="not on the device"):
        rec2.attach_states([SimpleNamespace(facets=model.facets, ode=mm_hh, handle=None, tag=1)])


def test_bad_map_and_state_arguments(strip):
    from knpemidg import recorder as R
    mk = lambda **kw: R.Recorder(strip.mesh, strip.sub, strip.surf, 1, IONS, membrane_sets=[strip.a], regions=False, membrane_tags=[1], **kw)
    with pytest.raises(ValueError, match="finite"):
        mk(membrane_map=dict(threshold=float("nan")))
    with pytest.raises(ValueError, match="finite"):
        mk(membrane_map=dict(repolarisation=float("inf")))
    with pytest.raises(ValueError, match="not membrane facets"):
        mk(membrane_map=dict(tags=[5]))                                  # the exterior facets
    with pytest.raises(ValueError, match="unknown key"):
        mk(membrane_map=dict(treshold=0.0))
    with pytest.raises(ValueError, match="distinct"):
        mk(membrane_states=("n", "n"))
    with pytest.raises(ValueError, match="at least one membrane set"):
        R.Recorder(strip.mesh, strip.sub, strip.surf, 1, IONS, regions=False, membrane_tags=[1], membrane_states=("n",))


# ---------------------------------------------------------------------------------------------------------------------
# conduction velocity
# ---------------------------------------------------------------------------------------------------------------------
def _map_arrays(x, activated):
    n = len(x)
    t_act = np.where(activated, x / U, np.nan)
    return (t_act, np.full(n, np.nan), np.zeros(n), np.zeros(n), activated.astype(np.int32))


def test_conduction_velocity_from_the_map(strip):
    rec, dev = _recorder(strip, [strip.a, strip.b], membrane_map=dict(threshold=0.0))
    rec.attach(dev)
    rec.arm(0.0)
    x = strip.mesh.facet_midpoints()[rec.map_facets, 0]
    dev.map_arrays = _map_arrays(x, np.ones(len(x), dtype=bool))
    xa, xb = rec.set_centroid(0), rec.set_centroid(1)
    # activation times x / u: the weighted mean time of a set is (centroid x) / u, so distance along x over the difference is u
    v = rec.conduction_velocity(0, 1, distance=xb[0] - xa[0])
    assert abs(v - U) < 1e-12 * U
    assert rec.conduction_velocity(1, 0, distance=xb[0] - xa[0]) == pytest.approx(-U, rel=1e-12)
    # the default distance is that of the area-weighted centroids
    assert rec.conduction_velocity(0, 1) == pytest.approx(U * np.linalg.norm(xb - xa) / (xb[0] - xa[0]), rel=1e-12)
    # one facet of set b has not activated: NaN, no exception
    off = np.ones(len(x), dtype=bool)
    off[list(rec.map_facets).index(int(strip.b[0]))] = False
    dev.map_arrays = _map_arrays(x, off)
    assert math.isnan(rec.conduction_velocity(0, 1))
    # a set outside the map's facets is an error, not a wrong number
    rec2, dev2 = _recorder(strip, [strip.a, strip.b], membrane_map=dict(threshold=0.0))
    rec2.attach(dev2)
    rec2.map_facets = rec2.map_facets[~np.isin(rec2.map_facets, strip.b[:1])]
    rec2.arm(0.0)
    dev2.map_arrays = _map_arrays(x[:len(rec2.map_facets)], np.ones(len(rec2.map_facets), dtype=bool))
    with pytest.raises(ValueError, match="not in the membrane map"):
        rec2.conduction_velocity(0, 1)


def _front_rows(rec, front, n_steps):
    """phi_M of every set = area-weighted mean of front(t - x_f / U); everything else zero."""
    mid = rec.mesh.facet_midpoints()

    def row_of(t):
        row = []
        for f, w in zip(rec.set_facets, rec.set_weights):
            row += [float(w @ front(t - mid[f, 0] / U))] + [0.0] * 6
        return row
    return row_of


def test_conduction_velocity_from_the_set_mean(strip):
    # (1) a front that is linear in time: the set mean is a (t - centroid x / u), its interpolated crossing of 0 is exact
    rec, dev = _recorder(strip, [strip.a, strip.b])
    dev.row_of = _front_rows(rec, lambda s: 2.0e4 * s, 0)
    rec.attach(dev)
    for k in range(1, 9):
        rec.sample(k * DT)
    xa, xb = rec.set_centroid(0), rec.set_centroid(1)
    assert xb[0] / U < 8 * DT and xa[0] / U > DT
    v = rec.conduction_velocity(0, 1, distance=xb[0] - xa[0], method="set_mean")
    assert abs(v - U) < 1e-9 * U                            # t ~ 4e-6 known to ~1e-16 relative of t/dt terms; far below 1e-9
    # (2) single-facet sets and a tanh front G(s) = A tanh(s / tau), crossing 0 at exactly x / u.  The linear interpolant of G over
    # one step is off by at most dt^2 / 8 max|G''| <= dt^2 / 8 * 0.77 A / tau^2, and |G'| >= A / tau sech^2(dt / tau) within the
    # bracketing step, so each crossing time is off by at most e_t = 0.77 / 8 dt^2 / tau cosh^2(dt / tau)
    tau = 2.0 * DT
    rec, dev = _recorder(strip, [strip.a[:1], strip.b[:1]])
    dev.row_of = _front_rows(rec, lambda s: 0.1 * np.tanh(s / tau), 0)
    rec.attach(dev)
    for k in range(1, 9):
        rec.sample(k * DT)
    xa, xb = rec.set_centroid(0)[0], rec.set_centroid(1)[0]
    e_t = 0.77 / 8.0 * DT * DT / tau * math.cosh(DT / tau) ** 2
    dt_true = (xb - xa) / U
    v = rec.conduction_velocity(0, 1, distance=xb - xa, method="set_mean")
    assert abs(v - U) <= U * 2.0 * e_t / (dt_true - 2.0 * e_t)
    # a threshold the second set never reaches: NaN
    assert math.isnan(rec.conduction_velocity(0, 1, method="set_mean", threshold=0.2))
    with pytest.raises(ValueError, match="method"):
        rec.conduction_velocity(0, 1, method="nearest")


def test_first_upward_crossing():
    from knpemidg.recorder import first_upward_crossing
    t = np.array([1.0, 2.0, 3.0, 4.0, 5.0])
    assert first_upward_crossing(t, [-1.0, -0.5, 0.5, -1.0, 1.0], 0.0) == 2.5
    assert first_upward_crossing(t, [-1.0, 0.0, 1.0, 1.0, 1.0], 0.0) == 2.0           # lands exactly on the threshold: counts there
    assert math.isnan(first_upward_crossing(t, [0.0, 0.5, 1.0, 1.0, 1.0], 0.0))       # starts at the threshold: never crosses up
    assert math.isnan(first_upward_crossing(t, [-1.0] * 5, 0.0))


# ---------------------------------------------------------------------------------------------------------------------
# file round trip
# ---------------------------------------------------------------------------------------------------------------------
def test_save_and_reload_the_new_datasets(strip, tmp_path):
    from knpemidg.h5lite import H5File
    from knpemidg.models import mm_hh
    model = SimpleNamespace(facets=np.sort(strip.mem), ode=mm_hh, handle=0, tag=1)
    tables = {0: np.random.default_rng(4).uniform(size=(64, 4))}
    rec, dev = _recorder(strip, [strip.a, strip.b], tables=tables, membrane_states=("n", "m", "h"),
                         membrane_map=dict(threshold=-0.01, repolarisation=-0.03))
    rec.attach(dev, models=[model])
    rec.arm(0.0)
    for k in range(1, 7):                                    # capacity 4: one flush on the way
        tables[0] *= 0.9
        rec.sample(k * DT)
    rng = np.random.default_rng(5)
    n = len(rec.map_facets)
    t_act = rng.uniform(size=n)
    t_act[::3] = np.nan
    dev.map_arrays = (t_act, np.full(n, np.nan), rng.uniform(size=n), rng.uniform(size=n), rng.integers(0, 3, size=n).astype(np.int32))
    path = rec.save(str(tmp_path / "timeseries.h5"))
    h = H5File(path)
    for q in ("n", "m", "h"):
        got = h.read("timeseries/membrane/" + q)
        assert got.shape == (6, 2) and np.array_equal(got, rec.membrane[q])
    assert not np.array_equal(rec.membrane["n"][0], rec.membrane["n"][5])
    assert np.array_equal(h.read("timeseries/membrane/phi_M"), rec.membrane["phi_M"])
    m = rec.membrane_map
    assert np.array_equal(h.read("membrane_map/facets"), rec.map_facets)
    for name in ("activation_time", "repolarisation_time", "peak", "peak_time"):
        assert np.array_equal(h.read("membrane_map/" + name), m[name], equal_nan=True), name
    assert np.isnan(h.read("membrane_map/activation_time")[::3]).all()
    assert np.array_equal(h.read("membrane_map/n_activations"), m["n_activations"])
    assert list(h.read("membrane_map/threshold")) == [-0.01] and list(h.read("membrane_map/repolarisation")) == [-0.03]
    # a recorder without the new arguments writes none of it
    rec0, dev0 = _recorder(strip, [strip.a])
    rec0.attach(dev0)
    rec0.sample(1.0)
    h0 = H5File(rec0.save(str(tmp_path / "plain.h5")))
    assert set(rec0.membrane) == {"phi_M", "E_K", "E_Cl", "E_Na", "I_ch_K", "I_ch_Cl", "I_ch_Na"}
    with pytest.raises(Exception):
        h0.read("membrane_map/facets")
