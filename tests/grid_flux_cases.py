"""What tests/test_grid_flux_host.py and tests/test_gpu_grid_flux.py share for the derived grid quantities (electric field, ion
fluxes, current density): the list of every quantity of a problem, diffusion coefficients that differ by subdomain, nodal data of a
polynomial, and the rounding bound.  Meshes, grids and owners come from grid_cases and are computed once there."""
import numpy as np

from knpemidg import _abi as A

# tortuosity by subdomain tag, as oracle.build_tortuosity scales D_k per subdomain (D_k / lambda_sub^2): a wrong owner's D shows
LAM = np.array([1.0, 1.6, 2.2])


def scaled_D(D, tags):
    """D [n_ions][nc] divided by LAM[tag]^2 cell by cell."""
    return np.asarray(D, dtype=np.float64) / LAM[np.asarray(tags).astype(np.int64)][None, :] ** 2


def scale_problem(pb):
    """The oracle problem with D differing by subdomain; returns D [n_ions][nc]."""
    D = scaled_D(np.stack([ion["D"] for ion in pb.ions]), pb.cell_tags)
    for ion, row in zip(pb.ions, D):
        ion["D"] = row
    return D


def all_quantities(ion_names):
    """(names, (kind, ion) pairs): efield, then flux and diffusive flux of every ion, then current -- 2 n_ions + 2 quantities."""
    names, q = ["efield"], [(A.GD_EFIELD, -1)]
    for k, n in enumerate(ion_names):
        names += ["flux_%s" % n, "diffusive_flux_%s" % n]
        q += [(A.GD_FLUX, k), (A.GD_FLUX_DIFFUSIVE, k)]
    return names + ["current"], q + [(A.GD_CURRENT, -1)]


def node_points(mesh, p):
    """Coordinates [nc, nd, d] of the nodes: vertices, then (P2) the edge midpoints (a, b), a < b, in the local dof order."""
    x = mesh.coords[mesh.cells]
    if p == 2:
        nv = x.shape[1]
        x = np.concatenate([x, np.stack([0.5 * (x[:, a] + x[:, b]) for a in range(nv) for b in range(a + 1, nv)], axis=1)], axis=1)
    return x


def vector_bound(mesh, pts, owner, scale):
    """1e-11 kappa_i (1 + |p_i|_inf / diam_i) S per point and component, the form of grid_cases.value_bound with S [nq, npts, d] = the sum
    of the absolute values of the quantity's terms (GridSpec.sample_derived): a rounding bound for grad lambda = adj / det and lambda
    in fp64, four orders above the machine epsilon.  kappa_i = cond of the owning cell's edge matrix, diam_i its longest edge."""
    X = mesh.coords[mesh.cells]
    found = owner >= 0
    c = owner[found]
    T = (X[c, 1:, :] - X[c, :1, :]).transpose(0, 2, 1)
    kappa = np.linalg.cond(T)
    nv = X.shape[1]
    diam = np.max([np.linalg.norm(X[c, a] - X[c, b], axis=1) for a in range(nv) for b in range(a + 1, nv)], axis=0)
    out = np.zeros(scale.shape)
    out[:, found] = (1.0e-11 * kappa * (1.0 + np.abs(pts[found]).max(axis=1) / diam))[None, :, None] * scale[:, found]
    return out


def worst_ratio(got, want, bound, found):
    """Largest |got - want| / bound over the owned points; got, want, bound [nq, npts, d]."""
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.abs(got[:, found] - want[:, found]) / bound[:, found]
    r = np.where(np.abs(got[:, found] - want[:, found]) == 0.0, 0.0, r)      # 0 / 0: an exact zero against a zero scale
    return float(r.max())
