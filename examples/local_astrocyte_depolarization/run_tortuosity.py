"""Local astrocyte depolarisation: the tortuosity study (reference: examples/local-astrocyte-depolarization/run_tortuosity.py) on the
bundled tissue reconstruction of examples/emix_simulations.  Synaptic activity is modelled as an ion source in a small box of
extracellular space during a time window: K enters and Na leaves at the same rate.  Both sources are `knpemidg.Expression`s bound
to the solver's time constant, so they are integrated on the device before every KNP solve.  The three variants scale the
tortuosity lambda of the intra- and extracellular space (diffusion D / lambda^2 per subdomain) and the source strength with it.

    python run_tortuosity.py [--variant baseline|2x|4x] [--Tstop 10] [--out results/]

Physical parameters: oracle/knpemi_oracle.py (tortuosity_params), which restates the reference's; mesh, tags, membrane models and
solver tolerances: examples/emix_simulations/emix_common.py.  The oracle's tuples follow the reference's tagging (1 neuronal, 2
glial), the bundled mesh is tagged 1 glial, 2 neuronal: initial concentrations, background charge and tortuosity are taken through
PARAM_COLUMN, so glial cells start at the glial values (K = 99.31 mM) under the glial membrane model and neurons at the neuronal
ones (K = 124.14 mM) under the Hodgkin-Huxley model."""
import argparse
import os
import sys
import time
from collections import namedtuple

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for _p in (os.path.join(ROOT, "examples", "emix_simulations"), os.path.join(ROOT, "oracle")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import emix_common as E                                                      # noqa: E402
from knpemidg import Constant, Expression                                    # noqa: E402
from knpemidg.models import mm_glial, mm_hh_emix                             # noqa: E402
from knpemidg.utils import pcws_constant_project, plus, minus                # noqa: E402

# variant -> (factor on the baseline tortuosities lambda_i = 3.2, lambda_e = 1.6, source strength g_syn in mM / ms)
VARIANTS = {"baseline": (1.0, 200.0), "2x": (2.0, 65.0), "4x": (4.0, 26.0)}
T_ON, T_OFF = 0.2, 1.2                                                       # the source is on for T_ON <= t <= T_OFF (ms)
BOX_HALF_WIDTH = 2.0e-5                                                      # cm: a 400 nm cube around the centre of the mesh
# The per-subdomain tuples of oracle.tortuosity_params (init, rho, lam) are indexed 0 ECS / 1 neuronal / 2 glial, the reference's
# tagging.  The bundled mesh is tagged 0 ECS / 1 GLIAL / 2 NEURONAL (emix_common.LABEL_TO_SUBDOMAIN; membrane tag 1 carries mm_glial,
# tag 2 mm_hh_emix): subdomain s of the mesh takes tuple entry PARAM_COLUMN[s].
PARAM_COLUMN = (0, 2, 1)

# one scalar C++ expression per source: indicator of the box times indicator of the time window times the strength
SOURCE = ("strength * ((fabs(x[0] - cx) <= half && fabs(x[1] - cy) <= half && fabs(x[2] - cz) <= half) ? 1.0 : 0.0)"
          " * ((t >= t_on && t <= t_off) ? 1.0 : 0.0)")


class SolverTortuosity(E.SolverEMIx):
    """ion_list = [K, Na, Cl] with Cl eliminated: the membrane models read extracellular K and intracellular Na from the solved species."""

    def update_ode(self, ode_model):
        K_e = plus(self.c_prev_k.split()[0], self.n_g)
        ode_model.set_parameter('K_e', pcws_constant_project(K_e, self.Q))
        Na_i = minus(self.c_prev_k.split()[1], self.n_g)
        ode_model.set_parameter('Na_i', pcws_constant_project(Na_i, self.Q))


def physical_setup(variant, t, centre):
    """(params, ion_list, stimulus parameters, the two source Expressions) of a variant; sources follow the Constant `t`."""
    import knpemi_oracle as ko
    factor, g_syn = VARIANTS[variant]
    P = ko.tortuosity_params()                                               # holds the 4x tortuosities: rescale to the variant's
    col = PARAM_COLUMN
    lam = [P["lam"][col[s]] * factor / 4.0 for s in range(3)]
    params = namedtuple('params', ('dt', 'n_steps_ODE', 'F', 'psi', 'C_phi', 'C_M', 'R', 'temperature', 'phi_M_init_type', 'rho_sub'))(
        P["dt"], 25, P["F"], P["F"] / (P["R"] * P["temperature"]), P["C_phi"], P["C_M"], P["R"], P["temperature"], 'constant',
        {s: Constant(P["rho"][col[s]]) for s in range(3)})
    box = dict(cx=float(centre[0]), cy=float(centre[1]), cz=float(centre[2]), half=BOX_HALF_WIDTH, t_on=T_ON, t_off=T_OFF, t=t)
    f_K = Expression(SOURCE, degree=4, strength=g_syn, **box)
    f_Na = Expression(SOURCE, degree=4, strength=-g_syn, **box)

    def ion(name, f_source):
        return {'c_init_sub': {s: Constant(P["init"][name][col[s]]) for s in range(3)}, 'c_init_sub_type': 'constant', 'bdry': Constant(0),
                'z': P["z"][name], 'name': name, 'D_sub': {s: Constant(P["D"][name] / lam[s] ** 2) for s in range(3)}, 'f_source': f_source}
    ion_list = [ion('K', f_K), ion('Na', f_Na), ion('Cl', Constant(0))]       # the last ion is eliminated
    stim = namedtuple('membrane_params', ('g_syn_bar', 'stimulus', 'stimulus_locator'))(0, {'stim_amplitude': 0}, lambda x: True)
    return params, ion_list, stim, (f_K, f_Na)


def box_integral(S, species, centre):
    """Integral of a solved species over the ECS cells whose midpoint lies in the source box (mM cm^3)."""
    mesh = S.mesh
    X = mesh.coords[mesh.cells]
    vol = np.abs(np.linalg.det(X[:, 1:] - X[:, :1])) / 6.0
    sel = (S.subdomains.array() == 0) & np.all(np.abs(X.mean(axis=1) - centre) <= BOX_HALF_WIDTH, axis=1)
    if not sel.any():
        raise RuntimeError("the source box holds no extracellular cell of this mesh")
    c = S.c.array()[species][sel]
    if S.nd == 10:                                                           # P2: the cell mean is -1/20 sum(vertices) + 1/5 sum(edges)
        mean = -0.05 * c[:, :4].sum(axis=1) + 0.2 * c[:, 4:].sum(axis=1)
    else:
        mean = c.mean(axis=1)
    return float((vol[sel] * mean).sum())


def main(steps=None, variant="baseline", mesh_tuple=None, Tstop=10.0, out=None, verbose=False):
    """Run the study (steps: stop after that many time steps instead of at Tstop; mesh_tuple: another (mesh, subdomains, surfaces)
    than the bundled reconstruction, tagged the same way).  Returns {'solver', 't', 'K_box', 'Na_box', 'K_init_by_subdomain'}: the
    integrals of K and Na over the extracellular cells of the source box before the first step and after every step, and the mean
    initial K of subdomains 0 (ECS), 1 (glial), 2 (neuronal)."""
    if variant not in VARIANTS:
        raise ValueError("variant must be one of %s" % ", ".join(VARIANTS))
    mesh, subdomains, surfaces = mesh_tuple or E.load_mesh()
    centre = 0.5 * (mesh.coords.min(axis=0) + mesh.coords.max(axis=0))
    t = Constant(0.0)
    params, ion_list, stim, _ = physical_setup(variant, t, centre)
    S = SolverTortuosity(params, ion_list)
    S.verbose = verbose
    S.setup_domain(mesh, subdomains, surfaces)
    S.setup_parameters()
    S.setup_FEM_spaces()
    S.setup_membrane_model(stim, {1: mm_glial, 2: mm_hh_emix})
    S.filename = out
    S.save_fields = out is not None
    S.save_solver_stats = False
    S._unpack_solver_params(E.solver_parameters())
    S.splitting_scheme = True
    S.setup_varform_emi(); S.setup_varform_knp(); S.setup_solver_emi(); S.setup_solver_knp()
    S._check_output_args(out)
    n = int(round(Tstop / float(S.dt))) if steps is None else int(steps)
    hist = {"solver": S, "t": [float(t)], "K_box": [box_integral(S, 0, centre)], "Na_box": [box_integral(S, 1, centre)]}
    tags, K0 = np.asarray(S.subdomains.array()), S.c.array()[0]
    hist["K_init_by_subdomain"] = [float(K0[tags == s].mean()) for s in range(3)]        # of the field the run starts from
    for k in range(n):
        S.step_membrane_models(k)
        S.solve_for_time_step(k, t)
        if S.save_fields and (k % S.sf) == 0:
            S.save_h5()
        hist["t"].append(float(t))
        hist["K_box"].append(box_integral(S, 0, centre))
        hist["Na_box"].append(box_integral(S, 1, centre))
    if S.save_fields:
        S.close_h5()
    return hist


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--variant", choices=sorted(VARIANTS), default="baseline")
    ap.add_argument("--Tstop", type=float, default=10.0, help="end time in ms (dt = 0.1 ms)")
    ap.add_argument("--steps", type=int, default=None, help="stop after this many steps instead")
    ap.add_argument("--out", default=None, help="directory prefix for results.h5")
    args = ap.parse_args()
    t0 = time.perf_counter()
    h = main(steps=args.steps, variant=args.variant, Tstop=args.Tstop, out=args.out)
    S = h["solver"]
    n = max(1, len(S.emi_niter))
    print("variant %s: %d tets, %d steps, %.1f ms/step incl. setup; K in the source box %.6e -> %.6e mM cm^3, Na %.6e -> %.6e"
          % (args.variant, S.mesh.num_cells(), n, 1e3 * (time.perf_counter() - t0) / n, h["K_box"][0], h["K_box"][-1],
             h["Na_box"][0], h["Na_box"][-1]))
