#!/usr/bin/python3
"""Space-convergence test with a manufactured solution on the HIP path (reference: tests/run_MMS_space.py:25-329):
2^r x 2^r meshes, P1, dt = 1e-10, two steps; prints L2 errors and observed rates and -- unlike the reference,
which only prints -- asserts the expected order p + 1 = 2 when called with --check."""
import os
import sys
from collections import namedtuple

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(HERE)), "knp-emi-dg_amd"))
sys.path.insert(0, HERE)

from knpemidg import Solver, Constant, make_mesh_MMS            # noqa: E402
from knpemidg.quadrature import simplex_rule                     # noqa: E402
from mms_space import setup_mms                                  # noqa: E402


def make_solver(resolution, degree=1, dt=1.0e-10, verbose=False):
    """The Solver of the space MMS after setup_domain, setup_parameters and setup_FEM_spaces (no device yet): `run` steps it;
    the tests take its data terms and its right-hand sides one by one (tests/test_mms_cases_host.py, tests/test_gpu_mms_rhs.py)."""
    names = ('D_a1', 'D_a2', 'D_b1', 'D_b2', 'D_c1', 'D_c2', 'C_a1', 'C_a2', 'C_b1', 'C_b2', 'C_c1', 'C_c2', 'C_phi',
             'z_a', 'z_b', 'z_c', 'dt', 'F', 'C_M', 'phi_M_init', 'R', 'temperature', 'phi_M_init_type', 'rho_sub')
    C_M = 1.0
    vals = (6, 5, 3, 4, 1, 2, 1, 2, 2, 4, 3, 2, C_M / dt, 1.0, -1.0, 1.0, dt, 1.0, C_M, None, 1.0, 1.0, 'expression',
            {0: 0.0, 1: 0.0, 2: 0.0})                                                      # run_MMS_space.py:32-58
    params = namedtuple('params', names)(*vals)
    mesh, subdomains, surfaces = make_mesh_MMS(resolution)
    mms = setup_mms(params)
    sol, rhs = mms.solution, mms.rhs

    def ion(s, name):
        return {'D_sub': {1: getattr(params, 'D_%s1' % s), 0: getattr(params, 'D_%s2' % s)}, 'z': getattr(params, 'z_' + s),
                'c_init_sub': {1: sol['c_%s1' % s], 0: sol['c_%s2' % s]}, 'c_init_sub_type': 'expression',
                'f1': rhs['volume_c_%s1' % s], 'f2': rhs['volume_c_%s2' % s],
                'g_robin_1': rhs['bdry']['u_%s1' % s], 'g_robin_2': rhs['bdry']['u_%s2' % s],
                'bdry': rhs['bdry']['neumann_' + s], 'C_sub': {1: getattr(params, 'C_%s1' % s), 0: getattr(params, 'C_%s2' % s)},
                'name': name, 'f_source': 0.0}
    ion_list = [ion('a', 'Na'), ion('b', 'K'), ion('c', 'Cl')]                            # the final ion is eliminated
    S = Solver(params=params, ion_list=ion_list, degree_emi=degree, degree_knp=degree, mms=mms)
    S.verbose = verbose
    S.setup_domain(mesh, subdomains, surfaces)
    S.setup_parameters()
    S.setup_FEM_spaces()
    return S


def direct_solver_params(resolution):
    """direct_emi = direct_knp = True, as the reference's run_MMS_space.py"""
    fields = ('direct_emi', 'direct_knp', 'resolution', 'rtol_emi', 'rtol_knp', 'atol_emi', 'atol_knp', 'threshold_emi', 'threshold_knp')
    return namedtuple('solver_params', fields)(True, True, resolution, 1e-6, 1e-7, 1e-40, 1e-40, 0.9, 7.5)


def run(resolution, degree=1, dt=1.0e-10, nsteps=2, verbose=False):
    S = make_solver(resolution, degree, dt, verbose)
    mesh, subdomains, sol = S.mesh, S.subdomains, S.mms.solution
    sp = direct_solver_params(resolution)
    t = Constant(0.0)
    uh, uh_cc = S.solve_system_passive(dt * nsteps, t, sp, None)
    fields = {'a': uh[0].array(), 'b': uh[1].array(), 'c': uh_cc.array(), 'phi': uh[2].array()}
    # L2 errors, degree-5 quadrature, phi mean-corrected (run_MMS_space.py:227-260)
    from knpemidg.dgtab import tabulate
    bary, w = simplex_rule(2, 5)
    Bq = tabulate(degree, bary)[0]
    x = mesh.coords[mesh.cells]
    X = np.einsum("ql,cld->cqd", bary, x)
    J = (x[:, 1:, :] - x[:, :1, :]).transpose(0, 2, 1)
    wq = w[None, :] * (np.abs(np.linalg.det(J)) / 2.0)[:, None]
    ics = (subdomains.array() == 1)[:, None]
    err = {}
    for s in "abc":
        ex = np.where(ics, sol['c_%s1' % s](X), sol['c_%s2' % s](X))
        e = ex - np.einsum("ql,cl->cq", Bq, fields[s])
        err[s] = float(np.sqrt((wq * e * e).sum()))
    ex = np.where(ics, sol['phi_1'](X), sol['phi_2'](X))
    uhq = np.einsum("ql,cl->cq", Bq, fields['phi'])
    e = ex - (wq * (ex - uhq)).sum() - uhq
    err['phi'] = float(np.sqrt((wq * e * e).sum()))
    S.dev.close()
    return err


if __name__ == '__main__':
    check = "--check" in sys.argv
    rmax = int(next((a.split("=")[1] for a in sys.argv if a.startswith("--rmax=")), 6))
    prev, rates = None, {}
    for r in range(2, rmax + 1):
        e = run(r, degree=int(next((a.split("=")[1] for a in sys.argv if a.startswith("--degree=")), 1)))
        if prev is not None:
            rates = {k: np.log(prev[k] / e[k]) / np.log(2) for k in e}
        print("r=%d  " % r + "  ".join("|%s-%sh|_0 = %.4E [%s]" % (k, k, v, ("%.2f" % rates[k]) if rates else "nan")
                                       for k, v in e.items()), flush=True)
        prev = e
    if check:
        assert all(v > 1.9 for v in rates.values()), rates
        print("rates ok")
