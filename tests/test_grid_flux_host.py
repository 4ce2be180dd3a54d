"""Host statement of the derived grid quantities (knpemidg/grid.py: GridSpec.sample_derived) against analysis, independently of any
device: P1 with affine and P2 with quadratic nodal data, where the electric field, the diffusive and total ion fluxes and the
current density are known in closed form at every point, with D differing by subdomain so that a wrong cell's D shows; then the
names, the frame file's vector datasets and the Vector attributes of its sidecar.  No GPU."""
import os
import xml.etree.ElementTree as ET

import numpy as np
import pytest

import grid_cases as G
import grid_flux_cases as GF
from knpemidg import _abi as A
from knpemidg.grid import GridFile, resolve_fields
from knpemidg.h5lite import H5File

IONS = ["K", "Cl", "Na"]
Z = np.array([1.0, -1.0, 1.0])
D0 = np.array([1.96e-9, 2.03e-9, 1.33e-9])
F_, R_, T_ = 96485.0, 8.314, 300.0
PSI = F_ / (R_ * T_)
CASES = [("2d", "generic"), ("2d", "exact"), ("3d", "generic"), ("3d", "exact")]


def _polynomials(mesh, quadratic):
    """phi and the c_k as p^T Q p + a.p + b (Q = 0 unless quadratic), scaled by the extent of the mesh so that every term counts:
    (Q [4, d, d], a [4, d], b [4]); row 0 is phi (volts), rows 1 .. 3 the concentrations, positive on the mesh."""
    d = mesh.gdim
    L = mesh.coords.max(axis=0) - mesh.coords.min(axis=0)
    rng = np.random.default_rng(11)
    a = rng.uniform(-1.0, 1.0, size=(4, d)) / L
    Q = rng.uniform(-1.0, 1.0, size=(4, d, d))
    Q = 0.5 * (Q + Q.transpose(0, 2, 1)) / (L[:, None] * L[None, :]) if quadratic else np.zeros((4, d, d))
    amp = np.array([0.05, 4.0, 100.0, 12.0])[:, None]
    a, Q = a * amp, Q * amp[:, :, None]
    b = np.array([0.01, 60.0, 1500.0, 180.0])          # 15 amp: above the variation amp (d + d^2) over a mesh that starts at the origin
    return Q, a, b


def _poly(Q, a, b, x):
    return np.einsum("...i,ij,...j->...", x, Q, x) + x @ a + b


def _poly_grad(Q, a, x):
    return 2.0 * x @ Q + a


@pytest.mark.parametrize("p", [1, 2])
@pytest.mark.parametrize("name,kind", CASES)
def test_replica_gives_the_closed_form(name, kind, p):
    """P1 / affine: efield = -a, diffusive_flux_k = -D_tag g_k, flux_k = -D_tag (g_k + z_k psi (g_k.p + e_k) a), current =
    F sum z_k flux_k.  P2 / quadratic: the same with the gradients 2 Q p + a.  Bound 1e-11 kappa (1 + |p| / diam) S."""
    mesh, sub, _ = G.mesh_tuple(name)
    tags = np.asarray(sub.array()).astype(np.int64)
    s = G.spec(name, kind)
    owner, bary = G.located(name, kind)[:2]
    found = owner >= 0
    pts = s.points()
    D = GF.scaled_D(np.repeat(D0[:, None], mesh.num_cells(), axis=1), tags)
    assert len(np.unique(D[0])) >= 2
    Q, a, b = _polynomials(mesh, p == 2)
    nodes = GF.node_points(mesh, p)
    u = [_poly(Q[r], a[r], b[r], nodes) for r in range(4)]
    assert all((u[r] > 0).all() for r in (1, 2, 3))
    names, quantities = GF.all_quantities(IONS)
    got, scale = s.sample_derived(mesh, quantities, u[0], u[1:], Z, D, PSI, F_, p, owner, bary)
    assert got.shape == scale.shape == (len(quantities), s.npts, mesh.gdim)
    assert np.isnan(got[:, ~found]).all() and np.isfinite(got[:, found]).all() and (scale[:, ~found] == 0.0).all()
    # analysis
    P = pts[found]
    Dp = D[:, owner[found]]
    gphi = _poly_grad(Q[0], a[0], P)
    want = np.full(got.shape, np.nan)
    cur = np.zeros_like(gphi)
    for k in range(3):
        gc, ck = _poly_grad(Q[k + 1], a[k + 1], P), _poly(Q[k + 1], a[k + 1], b[k + 1], P)
        diff = -Dp[k][:, None] * gc
        flux = -Dp[k][:, None] * (gc + Z[k] * PSI * ck[:, None] * gphi)
        want[names.index("diffusive_flux_" + IONS[k])][found] = diff
        want[names.index("flux_" + IONS[k])][found] = flux
        cur += F_ * Z[k] * flux
    want[names.index("efield")][found] = -gphi
    want[names.index("current")][found] = cur
    bound = GF.vector_bound(mesh, pts, owner, scale)
    worst = GF.worst_ratio(got, want, bound, found)
    print("%s %s P%d: largest error / bound %.2e" % (name, kind, p, worst))
    assert worst < 1.0
    # a wrong cell's D would show: the extracellular D in an intracellular cell is off by far more than the bound
    q = names.index("diffusive_flux_K")
    ics = found & (tags[np.maximum(owner, 0)] >= 1)
    assert ics.any() and (np.abs(want[q][ics] * (GF.LAM[1] ** 2 - 1.0)) > 1e3 * bound[q][ics]).any()


def test_names():
    K, X = A.GD_FLUX, A.GD_FLUX_DIFFUSIVE
    assert resolve_fields(("phi", "efield", "flux_K", "diffusive_flux_Na", "current", "Cl"), IONS) == \
        [0, (A.GD_EFIELD, -1), (K, 0), (X, 2), (A.GD_CURRENT, -1), 2]
    assert resolve_fields("flux_Na", IONS) == [(K, 2)] and resolve_fields(("current",), IONS) == [(A.GD_CURRENT, -1)]
    for bad in (("flux_Ca",), ("flux_",), ("diffusive_flux_phi",), ("flux_phi",), ("efield_K",), ("gradient",)):
        with pytest.raises(ValueError, match="unknown field"):
            resolve_fields(bad, IONS)
    for twice in (("efield", "efield"), ("flux_K", "phi", "flux_K"), ("current", "current")):
        with pytest.raises(ValueError, match="twice"):
            resolve_fields(twice, IONS)
    for ions in (["K", "efield", "Na"], ["current", "Cl"]):
        with pytest.raises(ValueError, match="cannot be told"):
            resolve_fields(("phi",), ions)


@pytest.mark.parametrize("name,dtype", [("2d", np.float32), ("3d", np.float64)])
def test_vector_datasets_and_sidecar(tmp_path, name, dtype):
    """/<name>/vector_<n> of a vector quantity is [nz, ny, nx, 3] ([ny, nx, 3] with a zero third component in 2D) and the sidecar
    declares AttributeType="Vector" with those dimensions; the nodal field beside it stays a Scalar."""
    mesh, sub, _ = G.mesh_tuple(name)
    d = mesh.gdim
    s = G.spec(name, "generic")
    owner = G.located(name, "generic")[0]
    rng = np.random.default_rng(4)
    fields = ["phi", "efield", "flux_K"]
    path = str(tmp_path / "grid.h5")
    gf = GridFile(path, s, fields, owner, owner)
    frames = []
    for n in range(2):
        planes = rng.uniform(-1, 1, size=(1 + 2 * d, s.npts)).astype(dtype)
        planes[:, owner < 0] = np.nan
        fr = {"phi": planes[0].reshape(s.array_shape)}
        for q, f in enumerate(fields[1:]):
            fr[f] = np.moveaxis(planes[1 + q * d:1 + (q + 1) * d].reshape((d,) + s.array_shape), 0, -1)      # as GridSampler hands them over
        gf.add(0.25 * n, n, fr)
        frames.append(fr)
    gf.close()
    h = H5File(path)
    for n, fr in enumerate(frames):
        assert h.read("/phi/vector_%d" % n).shape == s.array_shape
        for f in fields[1:]:
            v = h.read("/%s/vector_%d" % (f, n))
            assert v.shape == s.array_shape + (3,) and v.dtype == np.dtype(dtype)
            assert np.array_equal(v[..., :d], fr[f], equal_nan=True)
            if d == 2:
                assert (v[..., 2] == 0.0).all()
    root = ET.parse(os.path.splitext(path)[0] + ".xdmf").getroot()
    dims = " ".join(str(n) for n in s.array_shape)
    seen = {}
    for g in root.find("Domain/Grid").findall("Grid"):
        for att in g.findall("Attribute"):
            item = att.find("DataItem")
            seen.setdefault(att.get("Name"), set()).add((att.get("AttributeType"), item.get("Dimensions")))
            fname, dset = item.text.strip().split(":")
            assert " ".join(str(n) for n in H5File(str(tmp_path / fname)).read(dset).shape) == item.get("Dimensions")
            assert int(item.get("Precision")) == np.dtype(dtype).itemsize
    assert seen == {"phi": {("Scalar", dims)}, "efield": {("Vector", dims + " 3")}, "flux_K": {("Vector", dims + " 3")}}
