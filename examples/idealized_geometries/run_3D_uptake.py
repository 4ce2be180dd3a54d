#!/usr/bin/python3
"""3D idealized geometry with a K+ injection into a box of extracellular space and first-order K+ clearance on the whole ECS.

    f_K(x, t, c_K) = amp * [x in box] * [t_on <= t <= t_off]  -  k_up * (c_K - c_K0)        on the ECS (subdomain 0)
    f_Na           = -f_K                                                                    (the pair is electroneutral)

Both are `knpemidg.FieldExpression`s: they read the K+ concentration of the previous time level at the quadrature points and are
integrated on the device before every KNP solve, so the whole step stays on the GPU.  The reaction is explicit: k_up * dt = 0.05
here.  The ion list is [K, Na, Cl] with Cl eliminated (a source needs a solved species), so the membrane hook reads the
intracellular Na from the solved species, as examples/local_astrocyte_depolarization/run_tortuosity.py does.

The source has the form of the tortuosity study's (examples/local_astrocyte_depolarization/run_tortuosity.py: box indicator times
time window times strength), but not its box.  That one is a 400 nm cube around the centre of the tissue mesh; on the idealized
meshes it is shorter than one cell along x at resolution 0 (no cell midpoint of make_mesh_3D(0) or of the tests' small box lies in
it) and the centre need not be extracellular.  The box here is given in fractions of the mesh extent instead: the middle 30 % of
the x axis, against the lower y and z faces, where every idealized mesh has its extracellular rim.

    python run_3D_uptake.py [--resolution 0] [--steps 20] [--no-clearance]
"""
import argparse

import numpy as np

from idealized_common import Solver, Constant, make_mesh_3D, physical_setup, solver_parameters, pcws_constant_project, plus, minus
from knpemidg import FieldExpression
from knpemidg.models import mm_hh, mm_hh_no_stim

AMP, K_UP = 1000.0, 500.0                # mM / s injected in the box; 1 / s clearance rate
T_ON, T_OFF = 0.5e-4, 1.0                # s: the first step (t = 0) runs without the injection
# the box in fractions of the mesh extent: the middle of the x axis, against the lower y and z faces, where the ECS always is
BOX_FRACTION = ((0.35, 0.65), (0.0, 0.3), (0.0, 0.3))
INJECTION = ("amp * ((x[0] >= a0 && x[0] <= b0 && x[1] >= a1 && x[1] <= b1 && x[2] >= a2 && x[2] <= b2) ? 1.0 : 0.0)"
             " * ((t >= t_on && t <= t_off) ? 1.0 : 0.0)")
CLEARANCE = "k_up * (c_K - c_K0)"


class SolverUptake(Solver):
    """ion_list = [K, Na, Cl] with Cl eliminated: extracellular K and intracellular Na are both solved species."""

    def update_ode(self, ode_model):
        K_e = plus(self.c_prev_k.split()[0], self.n_g)
        ode_model.set_parameter('K_e', pcws_constant_project(K_e, self.Q))
        Na_i = minus(self.c_prev_k.split()[1], self.n_g)
        ode_model.set_parameter('Na_i', pcws_constant_project(Na_i, self.Q))


def box_of(mesh):
    lo, hi = mesh.coords.min(axis=0), mesh.coords.max(axis=0)
    fr = np.array(BOX_FRACTION)
    return lo + fr[:, 0] * (hi - lo), lo + fr[:, 1] * (hi - lo)


def box_integral(S, species):
    """Integral of a solved species over the ECS cells whose midpoint lies in the injection box."""
    mesh = S.mesh
    X = mesh.coords[mesh.cells]
    a, b = box_of(mesh)
    mid = X.mean(axis=1)
    sel = (S.subdomains.array() == 0) & np.all((mid >= a) & (mid <= b), axis=1)
    if not sel.any():
        raise RuntimeError("the injection box holds no extracellular cell of this mesh")
    vol = np.abs(np.linalg.det(X[:, 1:] - X[:, :1])) / 6.0
    return float((vol[sel] * S.c.array()[species][sel].mean(axis=1)).sum())


def main(steps=20, resolution=0, clearance=True, mesh_tuple=None, n_axons=4, verbose=False):
    """Run `steps` time steps; returns {'solver', 't', 'K_box', 'Na_box'} with the box integrals before the first and after every step."""
    params, ions, stim = physical_setup()
    by_name = {ion['name']: ion for ion in ions}
    ion_list = [by_name['K'], by_name['Na'], by_name['Cl']]
    mesh, subdomains, surfaces = mesh_tuple or make_mesh_3D(resolution, n_axons=n_axons)
    a, b = box_of(mesh)
    t = Constant(0.0)
    K0 = float(by_name['K']['c_init_sub'][0])
    geometry = dict(t_on=T_ON, t_off=T_OFF, t=t, **{"%s%d" % (s, d): float(v[d]) for s, v in (("a", a), ("b", b)) for d in range(3)})
    if clearance:
        code, fields, extra = "%s - %s" % (INJECTION, CLEARANCE), ("c_K",), dict(k_up=K_UP, c_K0=K0)
    else:
        code, fields, extra = INJECTION, (), {}
    ion_list[0]['f_source'] = FieldExpression(code, fields=fields, subdomains=(0,), amp=AMP, **geometry, **extra)
    ion_list[1]['f_source'] = FieldExpression("-(%s)" % code, fields=fields, subdomains=(0,), amp=AMP, **geometry, **extra)
    S = SolverUptake(params, ion_list)
    S.verbose = verbose
    S.setup_domain(mesh, subdomains, surfaces)
    S.setup_parameters()
    S.setup_FEM_spaces()
    S.setup_membrane_model(stim, {1: mm_hh, 2: mm_hh_no_stim} if n_axons > 1 else {1: mm_hh})
    S._unpack_solver_params(solver_parameters(3, resolution))
    S.save_fields = S.save_solver_stats = False
    S.splitting_scheme = True
    S.setup_varform_emi(); S.setup_varform_knp(); S.setup_solver_emi(); S.setup_solver_knp()
    hist = {"solver": S, "t": [float(t)], "K_box": [box_integral(S, 0)], "Na_box": [box_integral(S, 1)]}
    for k in range(int(steps)):
        S.step_membrane_models(k)
        S.solve_for_time_step(k, t)
        hist["t"].append(float(t))
        hist["K_box"].append(box_integral(S, 0))
        hist["Na_box"].append(box_integral(S, 1))
    return hist


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--resolution", type=int, default=0)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--no-clearance", action="store_true", help="the injection alone")
    args = ap.parse_args()
    h = main(steps=args.steps, resolution=args.resolution, clearance=not args.no_clearance)
    print("%d steps, clearance %s: K in the box %.6e -> %.6e mM m^3, Na %.6e -> %.6e"
          % (args.steps, "off" if args.no_clearance else "on", h["K_box"][0], h["K_box"][-1], h["Na_box"][0], h["Na_box"][-1]))
