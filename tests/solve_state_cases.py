"""What tests/test_gpu_solve_state.py (the device), tests/solve_state_worker.py (its child processes) and
tests/test_solve_state_ref_host.py (the CPU evidence) share -- test infrastructure, beside solve_state_ref.py: the problems and
coefficient states, the recorded sequence of events (GUESS_OPS) with its device side (`run_ops`) and its check against the model
(`check_ops`), the oracle's cell-block inverses with their bound, and `Boxes`, a box with its coefficient states as amg_ref hosts."""
import contextlib
import copy
import os

import numpy as np
import pytest

import amg_ref as ar
import knpemi_oracle as ko
import solve_state_ref as ss
from common import device_for, push_state, set_params_of, small_3d, synthetic_state

SB_HIST = dict(emi=8, knp=9)
SB_BINV = dict(emi=10, knp=11)
SB_COUNTERS, SB_REALS = 12, 13
worst = {}


def note(group, ratio):
    if float(ratio) > worst.get(group, -1.0):
        worst[group] = float(ratio)
        print("SOLSTATE %-52s worst error / bound %.3g" % (group, worst[group]))


# ---- problems ----------------------------------------------------------------------------------------------------------------------
def problem(name):
    """(pb, volt): the oracle's problem of a mesh of this file in the seeded synthetic state"""
    from knpemidg.mesh import make_mesh_2D, Mesh, MeshFunction
    volt = 1.0
    if name in ("box_P1", "box_P2", "2D_P1"):
        return ar.Host(name).pb, volt
    if name == "2D_P2":
        m, s, f = make_mesh_2D(0)
        pb = ko.build_idealized(m, s.array(), f.array(), p=2, membrane_tags=(1,))
    elif name == "emix":
        import emix_sub
        m, s, f = emix_sub.emix_submesh()
        pb, volt = ko.build_tortuosity(m, s.array(), f.array()), 1.0e3
    elif name.startswith("two_cell"):
        n_ions = int(name[-1])
        coords = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1], [1, 1, 1.0]]) * 1e-6
        m = Mesh(coords, np.array([[0, 1, 2, 3], [1, 2, 3, 4]]))
        s = MeshFunction(m, 3, np.array([0, 1]))
        f = MeshFunction(m, 2, 0)
        f.array()[m.interior_facets()] = 1
        P = ko.idealized_params()
        ions = [dict(name=n, z=P["z"][n], D=np.full(2, P["D"][n])) for n in ("K", "Cl", "Na")][3 - n_ions:]
        pb = ko.Problem(m, s.array(), f.array(), 1, ions, P, membrane_tags=(1,))
        rng = np.random.default_rng(5)
        pb.c = 50 + 10 * rng.uniform(size=pb.c.shape)
        pb.c_elim = 60 + 10 * rng.uniform(size=pb.c_elim.shape)
    else:
        assert name in ("box_533", "box_533_3")                         # 270 cells, 1080 dofs: the last workgroup of a 1-D kernel is partial;
        m, s, f = small_3d((5, 3, 3))                                   # four solved species, or three
        P = ko.idealized_params()
        z = dict(P["z"], **{n: v[0] for n, v in ar.EXTRA_IONS.items()})
        D = dict(P["D"], **{n: v[1] for n, v in ar.EXTRA_IONS.items()})
        ions = [dict(name=n, z=z[n], D=np.full(m.num_cells(), D[n])) for n in ar.IONS[3 if name.endswith("_3") else 4]]
        pb = ko.Problem(m, s.array().astype(np.int64), f.array(), 1, ions, P, membrane_tags=(1,))
        pb.c = np.random.default_rng(7).uniform(80.0, 120.0, size=pb.c.shape)
        pb.c_elim = np.random.default_rng(8).uniform(80.0, 120.0, size=pb.c_elim.shape)
    synthetic_state(pb, volt=volt)
    return pb, volt


def coefficient_states(pb, volt=1.0, n=4):
    """n coefficient states (c [N_ions, nc, nd], c_elim [nc, nd], phi [nc, nd]): state 0 is the problem's, the others move the
    concentrations by up to 25 % and draw another potential of the same size (cell Peclet number 5.4 on the boxes)"""
    out = [(pb.c.copy(), pb.c_elim.copy(), pb.phi.copy())]
    for i in range(1, n):
        r = np.random.default_rng(100 + i)
        out.append((pb.c * (1 + 0.25 * r.uniform(-1, 1, size=pb.c.shape)), pb.c_elim * (1 + 0.25 * r.uniform(-1, 1, size=pb.c_elim.shape)),
                    0.07 * volt * r.uniform(-1, 1, size=pb.phi.shape)))
    return out


def wide_values(seed, n):
    """values of both signs over nine decades"""
    r = np.random.default_rng(seed)
    return r.choice([-1.0, 1.0], size=n) * 10.0 ** r.uniform(-6.0, 3.0, size=n)


def oracle_blocks(pb, system, state, fp32=False):
    """(inv64 [nsys, nc, nd, nd], bound [nsys, nc]) of the cell-diagonal blocks of the oracle's matrices at a coefficient state; fp32:
    and the inverses as fp32 storage holds them (solve_state_ref.block_reference)"""
    q = copy.copy(pb)
    q.c, q.c_elim, q.phi = state
    mats = [ko.assemble_emi(q, want_B=False)[0].tocsr()] if system == "emi" else [ko.assemble_knp(q, k).tocsr() for k in range(q.N_ions)]
    refs = [ss.block_reference(ss.cell_blocks(M, pb.nd), fp32) for M in mats]
    return tuple(np.stack([r[k] for r in refs]) for k in range(3 if fp32 else 2))


# ---- the device side ---------------------------------------------------------------------------------------------------------------
def snapshot(dev):
    from knpemidg.checkpoint import split_snapshot
    table, arrays = split_snapshot(dev.state_save())
    out = {int(b["id"]): a for b, a in zip(table, arrays)}
    v, r = out[SB_COUNTERS].ravel(), out[SB_REALS].ravel()
    out["emi"] = dict(nh=int(v[0]), age=int(v[2]), lmax_age=int(v[5]), it_ref=int(v[7]), lmax=float(r[1]))
    out["knp"] = dict(nh=int(v[1]), age=int(v[3]), lmax_age=int(v[4]), it_ref=int(v[6]), lmax=float(r[0]))
    return out


def put(dev, field, values):
    """change a field on the device without an upload of it: through F_B_EMI (one system) or F_X (the species); both are scratch here"""
    from knpemidg import _abi as A
    values = np.asarray(values, dtype=np.float64).ravel()
    via = A.F_B_EMI if values.size == dev.nc * dev.nd else A.F_X
    assert via != field and values.size == dev.size(via)
    dev.upload(via, values)
    dev.copy_field(field, via)


def fail_solve(dev, system, maxit):
    """a solve at a tolerance it cannot reach: status -3, the documented "did not converge"; the field holds x_maxit"""
    from knpemidg import _abi as A
    with pytest.raises(A.KnpError, match="did not converge"):
        if system == "emi":
            dev.emi_solve(1e-30, maxit=maxit, check_every=1)
        else:
            dev.knp_solve(1e-30, maxit=maxit, min_it=0, check_every=1)
    return dev.download(A.F_PHI if system == "emi" else A.F_C)


# ---- a. the recorded sequence: guesses, histories, counters, blocks -----------------------------------------------------------------
# ("state", i): the coefficients of state i go to the device (c, c_elim -> kappa; phi -> dnphi); ("upload", field, k) / ("put", field,
# k): values k into PHI / C; ("solve", fuse): a maxit = 0 solve of both systems, fuse = False: with KNP_FUSE_EXTRAP=0 at that call
GUESS_OPS = (("state", 0), ("upload", "PHI", 0), ("upload", "C", 0), ("solve", True),
             ("put", "PHI", 1), ("put", "C", 1), ("solve", True),
             ("state", 1), ("put", "PHI", 2), ("put", "C", 2), ("solve", True),
             ("put", "PHI", 3), ("put", "C", 3), ("solve", False),
             ("state", 2), ("put", "PHI", 4), ("put", "C", 4), ("solve", True),
             ("upload", "C", 5), ("put", "PHI", 5), ("solve", True),
             ("state", 3), ("set_params",), ("put", "PHI", 6), ("put", "C", 6), ("solve", True),
             ("state", 0), ("upload", "PHI", 7), ("put", "C", 7), ("solve", True),
             ("state", 1), ("upload", "C_ELIM", 1), ("put", "PHI", 8), ("put", "C", 8), ("solve", True))
SHORT_OPS = GUESS_OPS[:4]                                               # a fresh context: one solve of each system (the blocks)


def values_of(pb, key, k):
    n = pb.ndof * (1 if key == "PHI" else pb.N_ions)
    return wide_values(1000 * (key == "C") + k, n)


def run_ops(dev, pb, states, ops, method="bicgstab"):
    """the device side of a recorded sequence: per solve and system the field, the history, the inverses and the counters afterwards"""
    from knpemidg import _abi as A
    fid = dict(PHI=A.F_PHI, C=A.F_C, C_ELIM=A.F_C_ELIM)
    if method == "gmres":
        dev.set_knp_krylov("gmres", 5)
    rec = []
    for op in ops:
        if op[0] == "state":
            c, ce, phi = states[op[1]]
            put(dev, A.F_C, c)
            put(dev, A.F_C_ELIM, ce)
            dev.update_kappa()
            put(dev, A.F_PHI, phi)
            dev.update_dnphi()
            dev.knp_rhs()                                               # (the power iteration of the KNP bound starts from B_KNP)
        elif op[0] == "upload":
            dev.upload(fid[op[1]], states[op[2]][1] if op[1] == "C_ELIM" else values_of(pb, op[1], op[2]))
        elif op[0] == "put":
            put(dev, fid[op[1]], values_of(pb, op[1], op[2]))
        elif op[0] == "set_params":
            set_params_of(dev, pb)
        else:
            keep = os.environ.pop("KNP_FUSE_EXTRAP", None)
            if not op[1]:
                os.environ["KNP_FUSE_EXTRAP"] = "0"                      # read at every call
            try:
                x = {s: fail_solve(dev, s, 0) for s in ("emi", "knp")}
            finally:
                os.environ.pop("KNP_FUSE_EXTRAP", None)
                if keep is not None:
                    os.environ["KNP_FUSE_EXTRAP"] = keep
            sn = snapshot(dev)
            for s in ("emi", "knp"):
                rec.append(dict(x=x[s], hist=sn[SB_HIST[s]], binv=sn[SB_BINV[s]], **{"n_" + k: v for k, v in sn[s].items()}))
    if method == "gmres":
        dev.set_knp_krylov("bicgstab")
    return rec


def save_rec(path, rec):
    np.savez(path, **{"%d_%s" % (i, k): np.asarray(v) for i, r in enumerate(rec) for k, v in r.items()})


def load_rec(path):
    z = np.load(path)
    n = 1 + max(int(k.split("_", 1)[0]) for k in z.files)
    return [{k.split("_", 1)[1]: z[k] for k in z.files if k.startswith("%d_" % i)} for i in range(n)]


def check_ops(tag, pb, states, ops, rec, model, blocks=None):
    """the model driven by the same events; every recorded solve against its prediction (blocks: a dict that keeps the oracle's
    inverses of `states` from one call to the next)"""
    ns, nc, nd = pb.N_ions, pb.mesh.num_cells(), pb.nd
    cur, coef, blocks, it = {}, None, ({} if blocks is None else blocks), iter(rec)
    bad, nsolve = [], 0
    for op in ops:
        if op[0] == "state":
            coef = op[1]
            cur["C"], cur["PHI"] = states[coef][0].ravel(), states[coef][2].ravel()
        elif op[0] == "upload":
            model.upload(op[1])
            if op[1] != "C_ELIM":
                cur[op[1]] = values_of(pb, op[1], op[2])
        elif op[0] == "put":
            cur[op[1]] = values_of(pb, op[1], op[2])
        elif op[0] == "set_params":
            model.set_params()
        else:
            nsolve += 1
            for s, key, n in (("emi", "PHI", 1), ("knp", "C", ns)):
                r, x = next(it), cur[key]
                S = model.sys(s)
                h1o, h2o, nho = (None if S.h1 is None else S.h1.copy()), (None if S.h2 is None else S.h2.copy()), S.nh
                plan = model.solve(s, x, coef, b=None, cheb=(s == "knp"), keep_h2=not op[1])
                model.done(s, False, 0)
                where = "%s %s solve %d" % (tag, s, nsolve)
                if nho >= 2 and model.order[s] >= 2:                      # order 2: contraction may change the last bit
                    e = np.abs(r["x"] - plan["guess"]) / ss.order2_bound(x, h1o, h2o)
                    note("guess order 2 (error / 2 ulp of the largest term)", e.max())
                    ok = e.max() <= 1.0
                else:
                    ok = np.array_equal(r["x"], plan["guess"])
                if not ok:
                    bad.append((where, "guess", float(np.abs(r["x"] - plan["guess"]).max())))
                cur[key] = r["x"]                                       # (the field now holds the guess)
                hist = np.asarray(r["hist"]).reshape(2, n * nc * nd)
                want = [np.zeros(n * nc * nd) if h is None else h for h in (S.h1, S.h2)]
                if not (np.array_equal(hist[0], want[0]) and np.array_equal(hist[1], want[1])):
                    bad.append((where, "history", float(np.abs(hist[0] - want[0]).max()), float(np.abs(hist[1] - want[1]).max())))
                got = {k: int(r["n_" + k]) for k in ("nh", "age", "lmax_age", "it_ref")}
                if got != S.counters():
                    bad.append((where, "counters", got, S.counters()))
                if (float(r["n_lmax"]) > 0.0) != (S.lmax is not None and s == "knp"):
                    bad.append((where, "bound present", float(r["n_lmax"])))
                if (s, plan["blocks"]) not in blocks:
                    blocks[s, plan["blocks"]] = oracle_blocks(pb, s, states[plan["blocks"]])
                inv, bd = blocks[s, plan["blocks"]]
                e = np.abs(np.asarray(r["binv"], dtype=np.float64).reshape(n, nc, nd, nd) - inv).max(axis=(2, 3)) / bd
                note("blocks %s %s" % (tag.split()[0], s), e.max())
                if not e.max() <= 1.0:
                    bad.append((where, "blocks of state %s" % plan["blocks"], float(e.max())))
    assert not bad, bad[:6]


TABLE = ("box_P1", "box_P2", "box_533", "box_533_3")                                 # structured 3D: set_params has the class table rebuilt
# the switches solve.hip reads once per process: a fresh child each (tests/solve_state_worker.py), one after another
ENVIRONMENTS = ({"KNP_EXTRAPOLATE": "0"}, {"KNP_EXTRAPOLATE": "2"}, {"KNP_EXTRAPOLATE": "3"}, {"KNP_EXTRAPOLATE_ORDER": "2"},
                {"KNP_EXTRAPOLATE_ORDER_EMI": "2"}, {"KNP_BJ_LAG": "1"}, {"KNP_BJ_LAG": "3"})


# ---- b. / c. 18 one-iteration solves: lagged inverses, counters, the kept bound, x_1 ----------------------------------------------------
class Boxes:
    """a box with its four coefficient states as amg_ref hosts and the hierarchy `bands` of either system; `device()`: a fresh context
    on it for one test (small, and nothing a test before left in a context -- the block set of the last KNP solve, last_it, it_ref,
    a built class table -- can then meet a model that starts from nothing)"""
    _all = {}

    def __init__(self, mesh):
        from knpemidg import _abi as A
        self.A, self.mesh = A, mesh
        self.host = ar.Host(mesh)
        pb = self.pb = self.host.pb
        self.states = coefficient_states(pb)
        self.hosts = [self.host.variant(phi=phi, c=(c, ce)) for c, ce, phi in self.states]
        self.ns, self.nc, self.nd = pb.N_ions, pb.mesh.num_cells(), pb.nd
        self._levels, self._blocks = {}, {}
        self.dev = None

    @contextlib.contextmanager
    def device(self):
        self.dev = device_for(self.pb)
        try:
            push_state(self.dev, self.pb)
            self.dev.update_kappa()
            self.dev.update_dnphi()
            yield self.dev
        finally:
            self.dev.close()
            self.dev = None

    @classmethod
    def get(cls, mesh):
        if mesh not in cls._all:
            cls._all[mesh] = cls(mesh)
        return cls._all[mesh]

    def levels(self, knp):
        if knp not in self._levels:
            self._levels[knp] = ar.synthetic_set(self.host.ncg, self.host.scale(knp))["bands"]
        return self._levels[knp]

    def blocks(self, system, state):
        """(inv64, bound, the fp32 inverses the replica applies) of a coefficient state"""
        if (system, state) not in self._blocks:
            inv, bd, b32 = oracle_blocks(self.pb, system, self.states[state], fp32=True)
            self._blocks[system, state] = inv, bd, list(b32)
        return self._blocks[system, state]

    def to_state(self, system, i):
        A, dev = self.A, self.dev
        c, ce, phi = self.states[i]
        if system == "emi":
            put(dev, A.F_C, c)
            put(dev, A.F_C_ELIM, ce)
            dev.update_kappa()
            dev.emi_rhs()
            return dev.download(A.F_B_EMI)
        put(dev, A.F_PHI, phi)
        dev.update_dnphi()
        dev.knp_rhs()
        return dev.download(A.F_B_KNP).reshape(self.ns, -1)

    def matrices(self, system, i):
        return [self.hosts[i].ref.A_emi] if system == "emi" else self.hosts[i].knp()[0]

    def lam(self, system, est, bs):
        """(1.1 lambda in float64, its comparison bound, 1.1 lambda in extended precision) of an estimate dict(matrix, blocks, b,
        factor) of the model"""
        As, Bi = self.matrices(system, est["matrix"]), self.blocks(system, est["blocks"])[2]
        bs = [np.asarray(b).ravel() for b in np.atleast_2d(bs)]
        l64 = ss.lambda_max(As, Bi, bs, np.float64, est["factor"])
        lhp = ss.lambda_max(As, Bi, bs, np.longdouble, est["factor"]) if ar.HP is not None else l64
        assert est["factor"] != 1.1 or abs(ar.bj_lambda_max(As, Bi, bs) - l64) <= 1e-14 * l64
        return float(l64), ss.lambda_bound(l64, lhp), lhp

    def x1(self, system, i, guess, blocks, lmax, b, levels, cheb, dtype):
        """the replica's x_1 [nsys, ndof] on the matrices of state i from `guess`, with the inverses of state `blocks` and the bound lmax"""
        h, b32 = self.hosts[i], self.blocks(system, blocks)[2]
        if system == "knp":
            return ar.knp_xk(h, levels, 1, dtype, bs=b, blocks=b32, lmax=lmax, x0=np.asarray(guess).reshape(self.ns, -1))
        return ar.emi_xk(h, levels, cheb, 1, dtype, b=b, binv=b32[0], lmax=lmax, x0=guess)[None]
