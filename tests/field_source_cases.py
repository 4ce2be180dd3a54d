"""Inputs of the field-source tests (tests/test_field_expression_host.py checks their conditions, tests/test_gpu_field_source.py uses
them): `knpemidg.FieldExpression`s over phi and the concentrations, each with a hand-written numpy twin.

A case is a C++ string over the fields and parameters, the twin f(X, u, t) of it and its yardstick M(X, u, t): the sum of the
absolute values of the terms of f (for "-k (c_K - c0)": |k| (|c_K| + |c0|)), so that cancellation between the terms does not shrink
what a difference is measured against.  Every case is multiplied by the indicator of a time window [T0, T1]; T_IN and T_OUT lie
strictly inside and outside it.  No case has a spatial indicator, so no quadrature point can sit on a face of one.

The reference of a row is
    row[c, a] = vol_c sum_q w_q f(x_q, u(x_q)) B[q, a],     u(x_q) = sum_b U[c, b] B[q, b],
with simplex_rule(dim, QDEG) and dgtab.tabulate, the tables the device is given, over the cells whose tag is in `subdomains`; the
bound is |device - twin| <= BOUND * scale per entry, scale = vol_c sum_q w_q M(x_q) |B[q, a]|, BOUND = 1e-12 of tests/source_cases.py
(125 points x (nd + a few) roundings of 1.1e-16 is a few 1e-14 of the term sizes; exp differs by an ulp or two between device and
numpy).  Entries with scale == 0 are exact zeros.

Fields: discontinuous pseudo-random nodal arrays, another stream per field, so every (field, cell, node) holds its own number and a
wrong field pointer, cell order or node order shows: concentrations in [1, 150], phi in [-0.1, 0.1]."""
import numpy as np

import source_cases as SC

BOUND = SC.BOUND
T0, T1, T_IN, T_OUT = SC.T0, SC.T1, SC.T_IN, SC.T_OUT
IONS = ("Na", "K", "Cl")                 # the ion list of the device-level tests: Cl is the eliminated ion
FIELD_NAMES = ("phi",) + tuple("c_" + n for n in IONS)
WINDOW = " * ((t0 <= t && t <= t1) ? 1.0 : 0.0)"
K_UP, C0, G_REL, V0, K_NA, C0_NA, W_CL = 50.0, 4.0, 3.0, 0.025, 2.0, 100.0, 0.5


def _window(t):
    return 1.0 if t is None else float(T0 <= t <= T1)


class Case:
    def __init__(self, name, code, fields, params, f, M):
        self.name, self.code, self.fields, self.params, self._f, self._M = name, code, fields, params, f, M

    def expression(self, t=T_IN, subdomains=(0,), **over):
        """With the time window, bound to `t` (a number or a Constant); t=None: the bare code, and f(., ., None) its twin."""
        from knpemidg import FieldExpression
        if t is None:
            return FieldExpression(self.code, fields=self.fields, subdomains=subdomains, **dict(self.params, **over))
        return FieldExpression("(" + self.code + ")" + WINDOW, fields=self.fields, subdomains=subdomains,
                               **dict(self.params, t0=T0, t1=T1, t=t, **over))

    def f(self, X, u, t):
        return self._f(X, u) * _window(t)

    def M(self, X, u, t):
        return self._M(X, u) * _window(t)


# NF = 1, linear in the field: first-order clearance
LINEAR = Case("linear", "-k_up * (c_K - c0)", ("c_K",), dict(k_up=K_UP, c0=C0),
              lambda X, u: -K_UP * (u["c_K"] - C0), lambda X, u: K_UP * (np.abs(u["c_K"]) + C0))
# NF = 2, nonlinear: voltage-dependent release
NONLINEAR = Case("nonlinear", "g * c_K * exp(-phi / v0)", ("c_K", "phi"), dict(g=G_REL, v0=V0),
                 lambda X, u: G_REL * u["c_K"] * np.exp(-u["phi"] / V0), lambda X, u: G_REL * np.abs(u["c_K"]) * np.exp(-u["phi"] / V0))
# NF = n_ions + 1: phi and every ion, the eliminated one included
ALL_FIELDS = Case("all", "g * c_K * exp(-phi / v0) - k_na * (c_Na - c0) + w_cl * c_Cl", ("c_K", "phi", "c_Na", "c_Cl"),
                  dict(g=G_REL, v0=V0, k_na=K_NA, c0=C0_NA, w_cl=W_CL),
                  lambda X, u: G_REL * u["c_K"] * np.exp(-u["phi"] / V0) - K_NA * (u["c_Na"] - C0_NA) + W_CL * u["c_Cl"],
                  lambda X, u: G_REL * np.abs(u["c_K"]) * np.exp(-u["phi"] / V0) + K_NA * (np.abs(u["c_Na"]) + C0_NA) + W_CL * np.abs(u["c_Cl"]))
# NF = 0: the plain-source kernel with its own cell list
NO_FIELDS = Case("none", "amp * (1.0 + 0.3 * sin(k * x[0]))", (), dict(amp=7.0, k=4.0e5),
                 lambda X, u: 7.0 * (1.0 + 0.3 * np.sin(4.0e5 * X[..., 0])), lambda X, u: 7.0 * (1.0 + 0.3 * np.abs(np.sin(4.0e5 * X[..., 0]))))
CASES = {c.name: c for c in (LINEAR, NONLINEAR, ALL_FIELDS, NO_FIELDS)}


def nd_of(dim, degree):
    return dim + 1 if degree == 1 else (dim + 1) * (dim + 2) // 2


def fields(nc, nd, seed=11, ions=IONS):
    """{name: U[nc, nd]} in the caller's cell order for phi and every ion."""
    out = {"phi": np.random.default_rng(seed).uniform(-0.1, 0.1, (nc, nd))}
    for i, n in enumerate(ions):
        out["c_" + n] = np.random.default_rng(seed + 1 + i).uniform(1.0, 150.0, (nc, nd))
    return out


def upload(dev, U, ions=IONS):
    """The fields as the device holds them at an evaluation: level-n concentrations in KNP_F_C_PREV, the eliminated ion in
    KNP_F_C_ELIM, phi in KNP_F_PHI.  KNP_F_C (the level being solved for) gets other numbers: a kernel reading it shows."""
    from knpemidg import _abi as A
    c_prev = np.stack([U["c_" + n] for n in ions[:-1]])
    dev.upload(A.F_C_PREV, c_prev)
    dev.upload(A.F_C, np.random.default_rng(99).uniform(1.0, 150.0, c_prev.shape))
    dev.upload(A.F_C_ELIM, U["c_" + ions[-1]])
    dev.upload(A.F_PHI, U["phi"])


def tables(dim, degree):
    from knpemidg.dgtab import tabulate
    from knpemidg.mms_terms import QDEG
    from knpemidg.quadrature import simplex_rule
    bary, w = simplex_rule(dim, QDEG)
    return bary, w, tabulate(degree, bary)[0]


def selection(tags, subdomains):
    return np.nonzero(np.isin(np.asarray(tags), list(subdomains)))[0]


def twin_row(mesh, tags, degree, case, U, t, subdomains=(0,)):
    """(row[nc, nd], scale[nc, nd]) of a case on the fields U over the cells whose tag is in `subdomains`."""
    from knpemidg.mms_terms import _geometry
    bary, w, B = tables(mesh.gdim, degree)
    vol = _geometry(mesh)[0]
    sel = selection(tags, subdomains)
    X = np.einsum("ql,cld->cqd", bary, mesh.coords[mesh.cells[sel]])
    u = {name: np.einsum("ca,qa->cq", U[name][sel], B) for name in case.fields}
    fv = np.broadcast_to(np.asarray(case.f(X, u, t), dtype=np.float64), X.shape[:-1])
    Mv = np.broadcast_to(np.asarray(case.M(X, u, t), dtype=np.float64), X.shape[:-1])
    row, scale = np.zeros((mesh.num_cells(), B.shape[1])), np.zeros((mesh.num_cells(), B.shape[1]))
    row[sel] = np.einsum("q,c,cq,qa->ca", w, vol[sel], fv, B)
    scale[sel] = np.einsum("q,c,cq,qa->ca", w, vol[sel], Mv, np.abs(B))
    return row, scale


def mass_row(mesh, tags, degree, Uf, subdomains=(0,)):
    """(row, scale) of the one-hot source f = u: the cell mass matrix vol sum_q w_q B[q, a] B[q, b] applied to the nodal values, and
    the same product of absolute values."""
    from knpemidg.mms_terms import _geometry
    bary, w, B = tables(mesh.gdim, degree)
    vol = _geometry(mesh)[0]
    sel = selection(tags, subdomains)
    Mloc = np.einsum("q,qa,qb->ab", w, B, B)
    Mabs = np.einsum("q,qa,qb->ab", w, np.abs(B), np.abs(B))
    row, scale = np.zeros((mesh.num_cells(), B.shape[1])), np.zeros((mesh.num_cells(), B.shape[1]))
    row[sel] = vol[sel, None] * (Uf[sel] @ Mloc.T)
    scale[sel] = vol[sel, None] * (np.abs(Uf[sel]) @ Mabs.T)
    return row, scale


worst_ratio = SC.worst_ratio
