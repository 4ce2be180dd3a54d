"""`Solver`: the KNP-EMI splitting solver of adajel/KNP-EMI-DG with its DG assemble-and-solve
hot path running as hand-written HIP kernels on MI355X.

Same class, method names, call order, parameter field names and error behaviour as the
reference (reference: src/knpemidg/solver.py:62-1258); what changed is what sits underneath:

    reference                                     this build
    ---------                                     ----------
    UFL forms + dolfin.assemble (solver.py:477)   matrix-free operator applies  (csrc/apply_p1.hip)
    PETSc Mat build (solver.py:458-460)           nothing -- no matrix exists
    PETSc KSP cg/gmres + hypre (solver.py:509)    device PCG / BiCGStab         (csrc/krylov.hip)
    pcws_constant_project / project (808-845)     facet kernels                 (csrc/rhs_p1.hip)

dolfin objects are replaced by the array stand-ins of `knpemidg.mesh` / `knpemidg.functions`.
There is no CPU fallback: without libknpemi_hip.so and a visible GPU, setup raises.

Who owns what: `Solver` keeps the reference's setup calls and time loops, the device bring-up, the ion sources and the checkpoint of its
own state, and declares everything it holds in `__init__`.  `resolve_settings` (below) turns solver_params and the KNP_* variables into
the effective tolerances and Krylov options.  knpemidg/precond.py owns the preconditioners' host side: `Solver.emi_smoother`
(SmootherChoice: the EMI DG-level smoother, measured on the first solve) and `Solver.amg` (AmgSetup: helper processes, hierarchy builds
and uploads, refresh policy and its counters).  knpemidg/recorder.py, grid.py and checkpoint.py own time series, voxel grids and the
checkpoint file.
"""
import os
import sys
import time
from typing import NamedTuple

import numpy as np

from knpemidg import _abi, ode_rtc, precond
from knpemidg.functions import FacetSpace, FacetFunction, DeviceFacetFunction, DeviceFunction
from knpemidg.membrane import MembraneModel
from knpemidg.mesh import Constant
from knpemidg.utils import interface_normal, plus, minus, pcws_constant_project

JUMP = lambda f, n: ("JUMP", f, n)   # symbolic marker; the device evaluates minus - plus


# factor theta of the residual half of the error-controlled EMI stop (resolve_settings): the solve ends when the TRUE residual,
# in the order-8 norm of its density, is below theta / p^2 * 0.1 rtol_emi * F min|z_k| ||b_knp / vol||_8 (p = polynomial degree: the
# error behind a given residual density grows with the degree, round 2's "DG-P2 needs a 4x tighter potential"; no mesh quantity enters).
# Measured against runs converged to 1e-11 / 1e-13 with BOTH DG-level smoothers of the EMI preconditioner (tools/stop_sweep_r04.py,
# profiles/r04_stop_sweep.txt; bound asked: c <= 1e-6, phi <= 1e-4).
EMI_TARGET_SAFETY = 20.0
# factor on rtol_emi of the energy-norm half of the EMI stop: the solve ends when the estimated ||phi - phi_k||_A (Hestenes-Stiefel
# identity, valid for any SPD preconditioner; csrc/krylov.hip: cg_converged) is below PHI_ENERGY_FACTOR * rtol_emi * ||phi||_A.  It bounds
# the error of the potential itself (north_star: 1e-4 in the max norm at the reference's rtol_emi 1e-5), smooth components included.
PHI_ENERGY_FACTOR = 0.5


class bcolors:
    OKGREEN = '\033[92m'
    WARNING = '\033[93m'
    ENDC = '\033[0m'


def _f(v):
    return float(v)


def _names(ode, what):
    """State / parameter names of a model module in column order, or their count where the module has no name table."""
    key = "STATE_IND" if what == "state" else "PARAM_IND"
    table = getattr(ode, key, None)
    if table is None:                                 # the built-in HH variants share the tables of models/_hh_core.py
        fn = getattr(ode, "state_indices" if what == "state" else "parameter_indices", None)
        table = getattr(sys.modules.get(getattr(fn, "__module__", None)), key, None)
    if isinstance(table, dict):
        return [str(x) for x in sorted(table, key=table.get)]
    return int(len(ode.init_state_values() if what == "state" else ode.init_parameter_values()))


class Settings(NamedTuple):
    """Effective tolerances and Krylov options of a run (resolve_settings)."""
    max_it_emi: int
    max_it_knp: int
    rtol_emi: float
    atol_emi: float
    emi_target: object           # factor of the error-controlled EMI stop, or None: the relative test with rtol_emi alone
    rtol_knp: float
    atol_knp: float
    knp_krylov: str
    gmres_restart: int
    knp_min_it: int
    knp_early: float


def _setting(sp, field, environ, variable, default, falsy_is_unset=False):
    """Field `field` of solver_params, else the variable, else the default -- as found: the caller converts."""
    v = getattr(sp, field, None)
    if v is None or (falsy_is_unset and not v):
        v = environ.get(variable) if variable is not None else None
    return default if v is None else v


def resolve_settings(sp, *, degree_emi, rtol_emi, atol_emi, rtol_knp, atol_knp, direct_emi, direct_knp, environ=os.environ,
                     max_it_emi=50000, max_it_knp=5000):
    """The `Settings` a run solves with: every option is the field of solver_params `sp` if that is set, else its KNP_* variable (where
    it has one), else the default.  "Set" means `is not None` for emi_rtol_scale, knp_rtol_scale and knp_early_stop (0 switches the
    early stop off).  For c_tol, emi_target_safety, emi_energy_factor, knp_krylov, knp_min_it and gmres_restart a FALSY field (0, 0.0,
    "") counts as unset and falls through to the variable: that is how these were always read, and it is kept.  rtol_* / atol_* are the
    nominal tolerances of solver_params (unused, and possibly None, for a direct solve); max_it_* the caps without a field."""
    # Krylov caps: the reference sets ksp_max_it 1000 behind BoomerAMG (solver.py:429,687); the cap is a solver_params option.
    max_it_emi = int(_setting(sp, "max_it_emi", environ, None, max_it_emi))
    max_it_knp = int(_setting(sp, "max_it_knp", environ, None, max_it_knp))
    # direct solvers (MUMPS, solver.py:412-422, 671-681) have no device counterpart: emulate with a tight
    # iterative tolerance
    rtol_direct = float(_setting(sp, "rtol_direct", environ, None, 1e-10))
    # PETSc tests ||M^-1 r|| <= rtol ||M^-1 b|| with M = BoomerAMG (solver.py:425-444); with this build's preconditioner the
    # same nominal rtol 1e-5 leaves mean-free phi accurate to 1e-4 of its maximum but the concentrations only to 3e-5
    # (they inherit the RELATIVE error of phi through the drift and membrane terms), measured against direct solves
    # through an action potential (tests/test_gpu_trajectory.py, tools/tolerance_sweep.py).  The nominal tolerance is
    # therefore scaled so that the stated parity bounds (c <= 1e-6, phi <= 1e-4) hold at every step.
    # DG-P2 needs a 4x tighter potential for the same bound on c (configs[2], r=1, 40 steps: worst c 1.8e-6 / 1.1e-6 / 6.2e-7
    # at scale 2e-3 / 1e-3 / 5e-4; a tighter KNP tolerance changes nothing): profiles/r02_tolerance_p2_r1.txt
    # The factor is a property of (mesh family, degree), not a constant: the weaker the preconditioner on a mesh, the larger
    # the error behind a given residual (EMIx reconstruction, 13-36 EMI iterations per solve: worst c 7.1e-6 at the idealized
    # mesh's settings; there the KNP residual test needs tightening too).  `emi_rtol_scale` / `knp_rtol_scale` in
    # solver_params set the factors per configuration (examples/emix_simulations: 1e-4 / 0.03, profiles/r02_tolerance_emix.txt);
    # tools/tolerance_sweep.py / tools/tolerance_emix.py measure them.
    # ROUND 3: the per-mesh factors above are replaced by an error-controlled stop.  The EMI solve stops when its residual, in the
    # cell-volume-weighted norm, is small enough for the concentration accuracy wanted (knp_emi_residual_target,
    # csrc/solve.hip): r_abs = theta * c_tol * F * min_k |z_k| ||b_knp,k||_w with c_tol = 0.1 * rtol_emi (the reference pairs
    # rtol_emi 1e-5 with concentrations good to 1e-6) and ONE safety factor theta for every mesh family and degree
    # (EMI_TARGET_SAFETY above; measured: profiles/r03_error_controlled_stop.txt).  `emi_rtol_scale` in solver_params (or
    # KNP_EMI_RTOL_SCALE, tools only) selects the old preconditioned-norm test with that factor instead.
    scale = _setting(sp, "emi_rtol_scale", environ, "KNP_EMI_RTOL_SCALE", None)
    rt = float(rtol_emi) if not direct_emi else 0.0
    emi_target = None
    if direct_emi:
        rtol_e = rtol_direct
    elif scale is not None:
        rtol_e = max(rt * float(scale), min(rt, 1.0e-11))
    else:
        c_tol = float(_setting(sp, "c_tol", environ, None, 0.1 * rt, falsy_is_unset=True))
        theta = float(_setting(sp, "emi_target_safety", environ, "KNP_EMI_TARGET_SAFETY", EMI_TARGET_SAFETY / degree_emi ** 2, falsy_is_unset=True))
        emi_target = theta * c_tol
        # Second half of the stop (csrc/krylov.hip: cg_converged): the energy-norm error of the iterate, estimated from the CG
        # coefficients, relative to ||phi||_A.  Round 3 tested the preconditioned norm ||M^-1 r|| here, which under-reports the
        # error by a factor that depends on M (a better preconditioner met it with MORE error left); the Hestenes-Stiefel estimate
        # measures the error itself and holds for any SPD preconditioner.
        rtol_e = float(_setting(sp, "emi_energy_factor", environ, "KNP_EMI_ENERGY_FACTOR", PHI_ENERGY_FACTOR, falsy_is_unset=True)) * rt
    kscale = float(_setting(sp, "knp_rtol_scale", environ, "KNP_KNP_RTOL_SCALE", 1.0))
    rk = float(rtol_knp) if not direct_knp else 0.0
    # direct_knp (MUMPS in the reference) is emulated by a tightly converged solve: rtol_direct is meant for the residual itself, so the
    # factor 20 the device puts on the order-8 density test (csrc/solve.hip: KNP_D8_FACTOR) is divided out here
    rtol_k = rtol_direct / 20.0 if direct_knp else max(rk * kscale, min(rk, 1.0e-13))
    # KNP Krylov method: the device default is BiCGStab; `knp_krylov = "gmres"` (+ `gmres_restart`, default 30) in solver_params,
    # or KNP_KNP_KRYLOV=gmres, selects the reference's restarted GMRES (ksp_type gmres / ksp_gmres_restart 30, solver.py:684-701)
    meth = _setting(sp, "knp_krylov", environ, "KNP_KNP_KRYLOV", "bicgstab", falsy_is_unset=True)
    restart = int(_setting(sp, "gmres_restart", environ, "KNP_GMRES_RESTART", 30, falsy_is_unset=True))
    # ksp_min_it 5 of the reference's GMRES (solver.py:686) = at least five operator + preconditioner applications.  A BiCGStab
    # iteration makes two of each, so three iterations (six applications) would honour it; rounds 1-3 forced five iterations = ten
    # applications, and the solves of the quiet phases of a run stopped at exactly that floor.  FOUR is the measured optimum: the
    # forced iterations of the quiet steps are what keeps the per-step errors from adding up over a run (r=1, 40 steps, worst c
    # against tight solves: min_it 3: 9.0e-7 at 3.95 iterations per step, 4: 2.2e-7 at 4.47, 5: 2.1e-7 at 5.12; tightening the
    # residual test instead buys less per iteration: factor 10 at min_it 3: 5.8e-7 at 4.70; profiles/r04_min_it.txt,
    # r04_stop_sweep.txt).  KNP_KNP_MIN_IT / solver_params.knp_min_it change it.
    min_it = int(_setting(sp, "knp_min_it", environ, "KNP_KNP_MIN_IT", 5 if meth == "gmres" else 4, falsy_is_unset=True))
    # The floor is there for the quiet phases; a solve whose residual is already 100x UNDER the tolerance needs no forced iterations
    # for that purpose (knp_knp_early_stop).  Over the reference's 200-step run at r=2: 4.20 -> 3.54 KNP iterations per step, KNP time
    # -16 %, worst c / phi over 100 steps unchanged to three digits at r=1 and r=2 (2.31e-7 / 2.15e-7: they come from the action
    # potential, where the floor does not bind); a factor 0.1 instead of 0.01: 2.57 iterations but c 7.2e-7 at r=1
    # (profiles/r04_early_stop_sweep.txt).  solver_params.knp_early_stop / KNP_KNP_EARLY set the factor, 0 switches it off.
    early = 0.0 if direct_knp else float(_setting(sp, "knp_early_stop", environ, "KNP_KNP_EARLY", 0.01))
    return Settings(max_it_emi, max_it_knp, rtol_e, 1e-40 if direct_emi else float(atol_emi), emi_target, rtol_k,
                    1e-40 if direct_knp else float(atol_knp), meth, restart, min_it, early)


class Solver:
    def __init__(self, params, ion_list, degree_emi=1, degree_knp=1, mms=None, sf=1):
        self.ion_list = ion_list
        self.N_ions = len(ion_list[:-1])
        self.degree_emi = degree_emi
        self.degree_knp = degree_knp
        self.mms = mms
        self.params = params
        self.sf = sf
        # timers (solver.py:76-81)
        self.ode_solve_timer = 0
        self.emi_solve_timer = 0
        self.knp_solve_timer = 0
        self.emi_ass_timer = 0
        self.knp_ass_timer = 0
        self.verbose = True
        self.dev = None
        self.device_index = int(os.environ.get("LOCAL_RANK", "0"))
        self.mem_models = []
        self.stimulus = None
        self.stimulus_locator = None
        if mms is None and os.environ.get("KNP_NO_AMG", "0") != "1":
            from knpemidg import setup_worker
            setup_worker.prestart(2)       # the two hierarchy helpers import their modules while the caller builds mesh and device context
        self.emi_niter = []
        self.emi_targets = []            # absolute residual targets handed to the EMI solves (error-controlled stop)
        self.knp_niter = []
        # Krylov caps: the reference sets ksp_max_it 1000 behind BoomerAMG (solver.py:429,687);
        # the block-Jacobi preconditioner here needs more, so the cap is a solver_params option.
        self.max_it_emi = 50000
        self.use_amg = os.environ.get("KNP_NO_AMG", "0") != "1"
        self.use_device_ode = os.environ.get("KNP_HOST_ODE", "0") != "1"
        self.max_it_knp = 5000
        self.recorder = None             # time-series recorder (Solver.record), sampled after step III of every time step
        self.grids = None                # voxel-grid samplers (Solver.record_grid); None = off: the time loops test this once per step
        self.surfaces_rec = None         # membrane-surface samplers (Solver.record_membrane); None = off, tested once per step as well
        self.fieldmeshes = None          # volume-field samplers on the mesh (Solver.record_fields); None = off, tested once per step as well
        # a partition of a global mesh: partition.distribute_solver sets these before setup_domain
        self.nc_owned = self.local_mesh = self.global_mesh_tuple = None
        # what the setup_* calls fill in, in the reference's order
        self.mesh = self.subdomains = self.surfaces = self.n_g = self.gdim = self.tau_emi = self.tau_knp = self.lm_tags = None
        self.C_phi = self.C_M = self.dt = self.F = self.R = self.temperature = self.psi = self.phi_M_init_type = self.rho = None
        self.nd = self.Q = self._init_c = self._init_c_elim = self._init_phi_M = None
        self.membrane_tags = self.phi = self.c = self.c_prev_k = self.c_prev_n = self.phi_M_prev_PDE = self.I_ch = None
        self.amg = None                  # precond.AmgSetup, from _ensure_device on
        self.emi_smoother = None         # precond.SmootherChoice, from setup_solver_emi on (with the AMG preconditioner)
        self._device_sources, self._callable_sources, self._src_geom = {}, {}, None
        # solver_params as unpacked by _unpack_solver_params, and what resolve_settings makes of them (_read_solver_params)
        self.solver_params = None
        self.direct_emi = self.direct_knp = False
        self.rtol_emi = self.atol_emi = self.threshold_emi = self.rtol_knp = self.atol_knp = self.threshold_knp = None
        self.settings = None
        self._rtol_emi = self._atol_emi = self._emi_target = self._rtol_knp = self._atol_knp = self._knp_min_it = self._knp_early = None
        self._knp_krylov = "bicgstab"    # the method the device runs (its default until set_knp_krylov)
        # run state
        self.filename, self.save_fields, self.save_solver_stats, self.splitting_scheme = None, False, False, True
        self._t_now = 0.0                # time-dependent sources see the t of the current step
        self._knp_bnorm = None           # load norms of the last KNP solve (_knp_load_norm)
        self.knp_residuals = None
        self.picard_iters = []
        self._picard = False
        self._k_done, self._t_done = 0, 0.0                  # what a checkpoint written now continues from
        self._resume_header, self._resume_k = None, 0
        self.h5_file = self.h5_path = None
        self.h5_idx = 0
        self.file_emi_solve = self.file_emi_assem = self.file_emi_niter = None
        self.file_knp_solve = self.file_knp_assem = self.file_knp_niter = None

    @property
    def emi_dg_chebyshev_measured(self):
        """None until the smoother trial has run, then its figures (precond.SmootherChoice.measured)."""
        return None if self.emi_smoother is None else self.emi_smoother.measured

    # read-only views of `amg` and `emi_smoother` under the names tests and the rank workers read
    _emi_helper = property(lambda self: None if self.amg is None else self.amg.emi_helper)
    _knp_helper = property(lambda self: None if self.amg is None else self.amg.knp_helper)
    amg_refreshes = property(lambda self: 0 if self.amg is None else self.amg.refreshes)
    amg_dist0 = property(lambda self: 0 if self.amg is None else self.amg.dist0_uploads)
    _emi_trial = property(lambda self: True if self.emi_smoother is not None and self.emi_smoother.pending else None)
    _emi_cheb_chosen = property(lambda self: None if self.emi_smoother is None else self.emi_smoother.chosen)

    @property
    def _cspace(self):
        """The conforming space, an attribute only once it has been built in this process (the helper processes build their own)."""
        if self.amg is None or self.amg.cspace is None:
            raise AttributeError("_cspace")
        return self.amg.cspace

    # ------------------------------------------------------------------ setup_domain (solver.py:85-121)
    def setup_domain(self, mesh, subdomains, surfaces):
        self.mesh = mesh
        self.subdomains = subdomains
        self.surfaces = surfaces
        self.n_g = interface_normal(subdomains, mesh)
        self.gdim = mesh.geometry().dim()
        self.tau_emi = Constant(20 * self.gdim * self.degree_emi)
        self.tau_knp = Constant(20 * self.gdim * self.degree_knp)
        if self.mms is not None:
            self.lm_tags = [1, 2, 3, 4]
        if self.degree_emi != self.degree_knp:
            raise NotImplementedError("degree_emi must equal degree_knp on the device path")
        return

    # ------------------------------------------------------------------ setup_parameters (solver.py:124-154)
    def setup_parameters(self):
        params = self.params
        self.C_phi = Constant(_f(params.C_phi))
        self.C_M = Constant(_f(params.C_M))
        self.dt = Constant(_f(params.dt))
        self.F = Constant(_f(params.F))
        self.R = Constant(_f(params.R))
        self.temperature = Constant(_f(params.temperature))
        self.psi = _f(self.F) / (_f(self.R) * _f(self.temperature))
        self.phi_M_init_type = params.phi_M_init_type
        for idx, ion in enumerate(self.ion_list):
            ion['D'] = self.make_global(ion['D_sub'])
            self.rho = self.make_global(params.rho_sub)
            if self.mms is not None:
                ion['C'] = self.make_global(ion['C_sub'])
        return

    def make_global(self, f):
        """DG0 array from a {cell tag: value} dict (solver.py:1244-1258); tags absent from the
        dict keep 0 exactly as the reference's zero-initialised Function does."""
        tags = self.subdomains.array()
        q = np.zeros(len(tags), dtype=np.float64)
        for key, value in f.items():
            q[tags == int(key)] = float(value)
        return q

    # ------------------------------------------------------------------ setup_FEM_spaces (solver.py:157-225)
    def setup_FEM_spaces(self):
        d = self.gdim
        p = self.degree_knp
        self.nd = d + 1 if p == 1 else (d + 1) * (d + 2) // 2
        nc = self.mesh.num_cells()
        self._init_c = np.zeros((self.N_ions, nc, self.nd))
        self._init_c_elim = np.zeros((nc, self.nd))
        for idx, ion in enumerate(self.ion_list):
            t = ion['c_init_sub_type']
            if t == 'constant':
                vals = self.make_global(ion['c_init_sub'])[:, None] * np.ones((nc, self.nd))
            elif t == 'expression':
                vals = self.make_global_expression(ion['c_init_sub'])
            elif t == 'function':
                src = ion['c_init_sub']
                vals = np.asarray(src.array() if hasattr(src, "array") else src, dtype=np.float64).reshape(nc, self.nd)
            else:
                print(f"""Type of initial condition \"{t}\" not
                    recognized - please spesify whether initial condition is
                    \"constant\", \"expression\" or \"function\" """)
                sys.exit(0)
            if idx == len(self.ion_list) - 1:
                self._init_c_elim = vals
            else:
                self._init_c[idx] = vals
        self.Q = FacetSpace(self.mesh)
        self._init_phi_M = np.zeros(self.mesh.num_facets())
        if self.phi_M_init_type == 'function':
            src = self.params.phi_M_init
            self._init_phi_M = np.asarray(src.array() if hasattr(src, "array") else src, dtype=np.float64).copy()
        elif self.phi_M_init_type in ('constant', 'expression'):
            pm = getattr(self.params, "phi_M_init", None)
            if pm is not None and self.phi_M_init_type == 'constant':
                # the reference leaves phi_M_prev_PDE = 0 here and takes the value from the ODE file at
                # k == 0 (solver.py:214, 1086-1090); identical once the first ODE step has run.
                pass
        else:
            print(f"""Type of initial condition \"{self.phi_M_init_type}\" not
                recognized - please spesify whether initial condition is
                \"constant\", \"expression\" or \"function\" """)
            sys.exit(0)
        return

    def make_global_expression(self, f):
        """Nodal interpolation of per-subdomain callables f[tag](x) (solver.py:1260-1298)."""
        tags = self.subdomains.array()
        X = self._node_coordinates()
        out = np.zeros(X.shape[:2])
        matched = np.zeros(len(tags), dtype=bool)
        for tag, fun in f.items():
            sel = tags == int(tag)
            matched |= sel
            if sel.any():
                out[sel] = np.asarray(fun(X[sel]), dtype=np.float64)
        assert matched.all(), "Dictionaries for DG data must match cell tags in mesh"
        return out

    def _node_coordinates(self):
        x = self.mesh.coords[self.mesh.cells]
        if self.degree_knp == 1:
            return x
        nv = x.shape[1]
        mids = [0.5 * (x[:, a] + x[:, b]) for a in range(nv) for b in range(a + 1, nv)]
        return np.concatenate([x, np.stack(mids, axis=1)], axis=1)

    # ------------------------------------------------------------------ setup_membrane_model (solver.py:228-267)
    def setup_membrane_model(self, stim_params, odes, ode_method=None):
        """ode_method: the ODE integrator, "dp5" or "stiff" (membrane.ODE_METHODS), for every model or as {tag: method}; None, or a tag
        the dict leaves out, takes the model module's ODE_METHOD (default "dp5").  Anything else raises ValueError."""
        from knpemidg.membrane import check_ode_method
        if isinstance(ode_method, dict):
            unknown = [t for t in ode_method if int(t) not in [int(u) for u in odes.keys()]]
            if unknown:
                raise ValueError("ode_method names tags %s that have no membrane model" % unknown)
            by_tag = {int(t): m for t, m in ode_method.items()}
        else:
            by_tag = {int(t): ode_method for t in odes.keys()}
        methods = {int(t): check_ode_method(by_tag.get(int(t)) if by_tag.get(int(t)) is not None else getattr(ode, "ODE_METHOD", None))
                   for t, ode in odes.items()}
        self.stimulus = stim_params.stimulus
        self.stimulus_locator = stim_params.stimulus_locator
        self.mem_models = []
        if self.use_device_ode:
            # HIP_RHS models compile (host only) on a worker thread while the context and the helpers start; attach_device joins
            ode_rtc.prefetch(odes.values(), [methods[int(t)] for t in odes.keys()])
        self._ensure_device(membrane_tags=[int(t) for t in odes.keys()])
        for tag, ode in odes.items():
            ode_model = MembraneModel(ode, facet_f=self.surfaces, tag=int(tag), V=self.Q, ode_method=methods[int(tag)])
            ode_model.set_parameter_values({'Cm': lambda x: self.params.C_M})
            on_dev = self.use_device_ode and ode_model.attach_device(self.dev)
            I_ch_k = {}
            for i, ion in enumerate(self.ion_list):
                I_ch_k_ = DeviceFacetFunction(self.Q, self.dev, _abi.F_I_CH, row=i) if on_dev else FacetFunction(self.Q)
                ode_model.get_parameter("I_ch_" + ion['name'], I_ch_k_)
                I_ch_k[ion['name']] = I_ch_k_
            self.mem_models.append({'ode': ode_model, 'I_ch_k': I_ch_k})
        if self.recorder is not None:
            self.recorder.attach_states([m['ode'] for m in self.mem_models])     # state channels of a record() call made earlier
        self._surfaces_attach(with_states=True)                                   # record_membrane calls made earlier
        return

    # ------------------------------------------------------------------ device context
    def _ensure_device(self, membrane_tags=None):
        if self.dev is not None:
            return
        if membrane_tags is None:
            membrane_tags = list(self.lm_tags) if self.mms is not None else [m['ode'].tag for m in self.mem_models]
        self.membrane_tags = list(membrane_tags)
        nc = self.mesh.num_cells()
        _abi._stamp("solver: _ensure_device")
        self.amg = precond.AmgSetup(precond.AmgInputs(
            mesh=self.mesh, subdomains=self.subdomains, surfaces=self.surfaces, global_mesh_tuple=self.global_mesh_tuple,
            local_mesh=self.local_mesh, degree=self.degree_knp, nd=self.nd, ion_list=self.ion_list, dt=_f(self.dt), F=_f(self.F),
            psi=self.psi, C_phi=_f(self.C_phi), membrane_tags=self.membrane_tags, init_c=self._init_c, init_c_elim=self._init_c_elim,
            verbose=self.verbose))
        if self.mms is None:
            if self.use_amg:                 # the helper processes build while the device context is being created
                self.amg.start_knp_helper()
                self.amg.start_emi_helper()
            _abi._stamp("solver: helper jobs handed over")
        self.dev = _abi.Device(self.mesh, self.subdomains.array(), self.surfaces.array(), self.membrane_tags,
                               len(self.ion_list), degree=self.degree_knp, device=self.device_index, nc_owned=self.nc_owned)
        A = _abi
        dev = self.dev
        self.phi = DeviceFunction(dev, A.F_PHI, nc, self.nd)
        self.c = DeviceFunction(dev, A.F_C, nc, self.nd, n_comp=self.N_ions)
        self.c_prev_k = self.c                                       # identical between Picard levels (solver.py:809)
        self.c_prev_n = DeviceFunction(dev, A.F_C_PREV, nc, self.nd, n_comp=self.N_ions)
        self.ion_list[-1]['c'] = DeviceFunction(dev, A.F_C_ELIM, nc, self.nd)
        self.phi_M_prev_PDE = DeviceFacetFunction(self.Q, dev, A.F_PHI_M)
        for k, ion in enumerate(self.ion_list):
            ion['E'] = DeviceFacetFunction(self.Q, dev, A.F_E, row=k)
        dev.upload(A.F_C, self._init_c)
        dev.copy_field(A.F_C_PREV, A.F_C)                            # the same values: one host-to-device transfer instead of two
        dev.upload(A.F_C_ELIM, self._init_c_elim)
        dev.upload(A.F_PHI_M, self._init_phi_M)
        self._push_params(splitting=True)
        dev.nernst()                                                 # initial E_k (solver.py:299-300)
        _abi._stamp("solver: initial fields and parameters on the device")
        if self.recorder is not None:
            self.recorder.attach(dev, self.membrane_tags)
        for g in self.grids or ():
            g.attach(dev)
        self._surfaces_attach(with_states=False)     # samplers with state planes wait for the membrane models (setup_membrane_model)
        for m in self.fieldmeshes or ():
            m.attach(dev, self.membrane_tags)

    # ------------------------------------------------------------------ time series (no reference counterpart: knpemidg/recorder.py)
    def record(self, points=None, membrane_sets=None, regions=True, capacity=256, point_tags=None, membrane_states=None,
               membrane_map=None):
        """Attach a recorder of point probes, membrane-set means and region integrals, sampled on the device after step III of
        every time step (csrc/record.hip) -- the traces the reference's figure scripts compute from per-step field output
        (examples/idealized-geometries/make_figures_3D.py:28-168).  Callable once setup_domain has run; the device tables are
        created as soon as the device context exists.  Returns the `knpemidg.recorder.Recorder`; a second call replaces it.
          points         [n, dim] coordinates; point_tags[i] (optional) = subdomain of the cell to take for a point on a membrane
          membrane_sets  list of facet-id arrays or (lo, hi) boxes (the membrane facets whose midpoint lies inside)
          regions        True = one region per distinct subdomain tag, ascending; False = none
          capacity       rows of the device buffer = time steps between two device-to-host copies
          membrane_states  names of ODE states as the membrane models declare them, e.g. ("n", "m", "h"): per membrane set the
                         area-weighted mean over the facets whose model has that state, read from the state tables on the device
                         (the reference's get_time_series_gating, examples/rat-neuron/make_figures_rat_neuron.py:238-315).  The row
                         of step k holds the states after ODE step k.  Recorder.membrane['<state>'] is [n_steps][n_sets].
          membrane_map   dict(threshold=0.0, repolarisation=None, tags=None), in the units of phi_M: per membrane facet (of the
                         given surface tags) the interpolated activation and repolarisation times, the peak and its time and the
                         number of activations (Recorder.membrane_map; plot_surface / get_velocity of the same script).  Armed by
                         the time loops of solve_system_active / solve_system_passive; call Recorder.arm(t0) when stepping by hand.
        Without the last two arguments the recorder issues the same device calls and rows as before.

        Partitioned solvers (partition.distribute_solver): every rank makes the same call, with the same capacity, in the GLOBAL
        mesh's terms -- coordinates, global facet ids or boxes, a global region array (S.global_mesh_tuple is the global mesh).  Each
        rank records what it owns (a probe: the owner of its cell; a membrane facet: the owner of its first cell; a cell: its owner)
        without any communication per sample; the partial rows are summed over the ranks when the buffer is read.  The Recorder's
        results are the global ones on every rank, and reading them (flush, rows, t, points, membrane, regions, membrane_map,
        conduction_velocity, save) is collective.  Rank 0 alone writes timeseries.h5."""
        from knpemidg.recorder import Recorder
        if membrane_states and not self.use_device_ode:
            raise _abi.KnpError("Solver.record: membrane_states read the ODE state tables on the device; with KNP_HOST_ODE=1 they "
                                "live on the host")
        loc, gmt = self.local_mesh, self.global_mesh_tuple
        if (loc is None or gmt is None) and (loc is not None or self.nc_owned is not None):
            raise _abi.KnpError("Solver.record: a partitioned solver needs its LocalMesh and the global mesh (local_mesh, "
                                "global_mesh_tuple: partition.distribute_solver sets them)")
        if self.mesh is None:
            raise _abi.KnpError("Solver.record: call setup_domain first")
        mtags = self.membrane_tags if self.dev is not None else None
        mesh, sub, surf = (self.mesh, self.subdomains, self.surfaces) if loc is None else gmt
        tags = lambda f: np.asarray(f.array() if hasattr(f, "array") else f)
        rec = Recorder(mesh, tags(sub), tags(surf), self.degree_knp, [ion['name'] for ion in self.ion_list],
                       points=points, membrane_sets=membrane_sets, regions=regions, capacity=capacity, point_tags=point_tags,
                       membrane_tags=mtags, membrane_states=membrane_states, membrane_map=membrane_map, local_mesh=loc)
        if self.dev is not None:
            rec.attach(self.dev, models=[m['ode'] for m in self.mem_models] if self.mem_models else None)
        self.recorder = rec
        return rec

    # ------------------------------------------------------------------ fields on a voxel grid (no reference counterpart: knpemidg/grid.py)
    def record_grid(self, lo, hi, shape, fields=("phi",), every=1, tags=None, dtype=np.float64, name="grid", tol=1.0e-12):
        """Sample fields on the regular grid lo + i (hi - lo) / (shape - 1), i < shape (axis order x, y[, z]; an axis with
        shape 1 sits at lo: a slice of a 3D mesh) on the device (csrc/grid.hip) -- the images and coarse volumes the reference's figure
        scripts rebuild from results.h5 with FEniCS (examples/*/make_figures*.py).  Callable once setup_domain has run; the points are
        located as soon as the device context exists.  Returns the `knpemidg.grid.GridSampler`; up to 8 grids per solver.
          fields   out of "phi" and the ion names (the eliminated ion included), and out of the vector quantities "efield"
                   (-grad phi), "diffusive_flux_<ion>" (-D_k grad c_k), "flux_<ion>" (J_k = -D_k grad c_k - z_k D_k psi c_k grad phi,
                   solver.py:31-34) and "current" (F sum_k z_k J_k over every ion), in the units of the parameters; each is
                   evaluated in the cell that owns the point, with that cell's D: DG gradients are one-sided, on a facet or the
                   membrane the owner decides the side (`tags` gives ECS-only or ICS-only fluxes).  sample() returns them as
                   [nz, ny, nx, d]; the file holds [nz, ny, nx, 3] and the sidecar declares them as Vector attributes
          every    the time loops write frame 0 for the state they start from, then one frame every `every` steps, to
                   `<filename><name>.h5` (+ `<name>.xdmf` for ParaView), next to timeseries.h5; a resumed run writes
                   `<name>_from<k>.h5` with /step_offset, as the field output does
          tags     restrict the candidate cells to these subdomains: the side of a point on a membrane, ECS- or ICS-only images
          dtype    np.float64 or np.float32 frames
        A point that no cell contains is NaN in every field (owner -1): a grid may stick out of the mesh.  `sampler.sample()` returns
        {field: array [nz, ny, nx]} ([ny, nx] in 2D) of the fields as they are now; `sampler.cells` / `sampler.tags` are the owner and
        subdomain volumes.  Without a call nothing is allocated or launched.  Partitioned solvers are not supported."""
        from knpemidg.grid import GridSpec, GridSampler, resolve_fields
        if self.local_mesh is not None or self.nc_owned is not None or (self.dev is not None and self.dev.nranks > 1):
            raise _abi.KnpError("record_grid: not supported with several ranks (sample the grid in a one-GPU run)")
        if self.mesh is None:
            raise _abi.KnpError("Solver.record_grid: call setup_domain first")
        try:
            spec = GridSpec(self.mesh.gdim, lo, hi, shape, tol=tol, tags=tags)
            ids = resolve_fields(fields, [ion['name'] for ion in self.ion_list])
            names = [fields] if isinstance(fields, str) else list(fields)
            g = GridSampler(spec, names, ids, every=every, dtype=dtype, name=name)
        except ValueError as e:
            raise _abi.KnpError(str(e))
        if any(o.name == g.name for o in self.grids or ()):
            raise _abi.KnpError("record_grid: a grid named %r exists already" % g.name)
        if len(self.grids or ()) >= 8:
            raise _abi.KnpError("record_grid: at most 8 grids per solver")
        if self.dev is not None:
            g.attach(self.dev)
        self.grids = (self.grids or []) + [g]
        return g

    def _grids_begin(self, k0, t):
        if self.filename is not None:
            for g in self.grids:
                g.begin(self.filename, k0, float(t))

    def _grids_step(self, steps_done, t):
        for g in self.grids:
            g.after_step(steps_done, float(t))

    def _grids_finish(self):
        for g in self.grids:
            g.finish()

    # ------------------------------------------------------------------ membrane-surface snapshots (no reference counterpart: knpemidg/surface.py)
    def record_membrane(self, fields=("phi_M",), states=(), tags=None, facets=None, every=1, dtype=np.float64, name="membrane"):
        """Sample facet quantities on the membrane on the device (csrc/surface.hip) and write them as cell data of the membrane's
        surface mesh -- the pictures of the action potential travelling along an axon the reference's figure scripts rebuild from
        results.h5 with FEniCS (examples/rat-neuron/make_figures_rat_neuron.py, examples/idealized-geometries/make_figures_3D.py).
        Callable once setup_domain has run; the device tables are created as soon as the device context and, with `states`, the
        membrane models exist.  Returns the `knpemidg.surface.MembraneSampler`; up to 4 per solver.
          fields   out of "phi_M"; "E_<ion>" and "I_ch_<ion>" for every ion, the eliminated one included; "I_ch_total" (the sum over
                   the ions, added in ion order); "phi_e", "phi_i", "c_<ion>_e", "c_<ion>_i": the facet means of the one-sided traces,
                   `_e` from the side utils.plus gives, `_i` from the side utils.minus gives -- the values of
                   pcws_constant_project(plus(u, n_g)) / pcws_constant_project(minus(u, n_g))
          states   gating-variable names as the membrane models declare them (as record(membrane_states=...)): one plane per name,
                   NaN on the facets whose model has no such state
          tags     surface tags to select (default: every membrane tag); facets: explicit facet ids instead.  The selection is kept
                   in ascending facet id
          every    the time loops write frame 0 for the state they start from, then one frame every `every` steps, to
                   `<filename><name>.h5` (+ `<name>.xdmf` for ParaView); a resumed run writes `<name>_from<k>.h5`
          dtype    np.float64 or np.float32 frames
        Pairing: a frame is taken after step III of a time step, as the recorder's row is: phi_M, E and the traces belong to the new
        time level, I_ch and the states are those after the ODE step of that splitting step.  `sampler.sample()` returns
        {plane: array [n]} of the state as it is now; `sampler.facets`, `.points`, `.connectivity` describe the surface.  Without a
        call nothing is allocated or launched; the sampler holds no step-to-step state (checkpoints do not change).  Partitioned
        solvers are not supported."""
        from knpemidg.surface import MembraneSampler, SurfaceSpec, resolve_fields
        if self.local_mesh is not None or self.nc_owned is not None or (self.dev is not None and self.dev.nranks > 1):
            raise _abi.KnpError("record_membrane: not supported with several ranks (sample the membrane in a one-GPU run)")
        if self.mesh is None:
            raise _abi.KnpError("Solver.record_membrane: call setup_domain first")
        if states and not self.use_device_ode:
            raise _abi.KnpError("Solver.record_membrane: states read the ODE state tables on the device; with KNP_HOST_ODE=1 they "
                                "live on the host")
        ids = resolve_fields(fields, [ion['name'] for ion in self.ion_list])
        names = [fields] if isinstance(fields, str) else list(fields)
        states = [states] if isinstance(states, str) else list(states)
        if tags is not None and facets is not None:
            raise ValueError("record_membrane: tags and facets are mutually exclusive")
        make_spec = lambda mtags: SurfaceSpec(self.mesh, self.surfaces, self.subdomains, mtags, degree=self.degree_knp, tags=tags,
                                              facets=facets)
        m = MembraneSampler(make_spec, names, ids, states=states, every=every, dtype=dtype, name=name)
        if any(o.name == m.name for o in self.surfaces_rec or ()):
            raise _abi.KnpError("record_membrane: a sampler named %r exists already" % m.name)
        if len(self.surfaces_rec or ()) >= 4:
            raise _abi.KnpError("record_membrane: at most 4 surface samplers per solver")
        if self.membrane_tags is not None:
            m.resolve(self.membrane_tags)        # a bad selection is refused here, before any device call
            if m.states:
                m.spec.state_tables([x['ode'] for x in self.mem_models], m.states)
        self.surfaces_rec = (self.surfaces_rec or []) + [m]
        try:
            self._surfaces_attach(with_states=bool(self.mem_models))
        except Exception:
            self.surfaces_rec = self.surfaces_rec[:-1] or None
            raise
        return m

    def _surfaces_attach(self, with_states):
        if self.dev is None:
            return
        for m in self.surfaces_rec or ():
            if not m.attached and (with_states or not m.states):
                m.attach(self.dev, self.membrane_tags, models=[x['ode'] for x in self.mem_models])

    def _surfaces_begin(self, k0, t):
        if self.filename is not None:
            for m in self.surfaces_rec:
                if not m.attached:
                    raise _abi.KnpError("record_membrane: sampler %r has state planes but the membrane models were never set up" % m.name)
                m.begin(self.filename, k0, float(t))

    def _surfaces_step(self, steps_done, t):
        for m in self.surfaces_rec:
            m.after_step(steps_done, float(t))

    def _surfaces_finish(self):
        for m in self.surfaces_rec:
            m.finish()

    # ------------------------------------------------------------------ volume fields on the mesh (no reference counterpart: knpemidg/fieldmesh.py)
    def record_fields(self, fields=("phi",), tags=None, continuous=True, every=1, dtype=np.float32, name="fields"):
        """Sample phi and concentrations on the mesh's own cells on the device (csrc/fieldmesh.hip) and write them as node data of the
        mesh -- what save_fields holds as full fp64 DG vectors in DOLFIN's layout, in a form ParaView opens and about 24 times smaller
        on a structured 3D mesh.  Callable once setup_domain has run; the device tables are created as soon as the device context
        exists.  Returns the `knpemidg.fieldmesh.FieldSampler`; up to 4 per solver.
          fields      out of "phi" and "c_<ion>" for every ion, the eliminated one included
          tags        the cell tags whose cells are written (default: every cell), e.g. the ECS alone
          continuous  True: one node per (mesh entity, cell tag) among the selected cells -- a vertex for P1, a vertex or an edge for
                      P2 -- holding the arithmetic mean of the nodal values the selected cells of that tag have there.  Cells of
                      different tags never share a node: the membrane stays a jump.  ValueError when a membrane facet separates two
                      selected cells of the same tag.  False: one node per (selected cell, local dof) with the exact DG values
          every       the time loops write frame 0 for the state they start from, then one frame every `every` steps, to
                      `<filename><name>.h5` (+ `<name>.xdmf` for ParaView); a resumed run writes `<name>_from<k>.h5`; the file is
                      closed also when the loop raises
          dtype       np.float32 (the default: this output is for pictures) or np.float64 frames
        `sampler.sample()` returns {field: array [n_nodes]} of the state as it is now; `sampler.points`, `.connectivity`,
        `.node_entity`, `.node_tag` and `.cells` describe the output mesh once the device context exists (the nodes are numbered along
        the device's cell order).  Without a call nothing is allocated or launched; the sampler holds no step-to-step state
        (checkpoints do not change).  Partitioned solvers are not supported."""
        from knpemidg.fieldmesh import MAX_SAMPLERS, FieldMeshSpec, FieldSampler, resolve_fields
        if self.local_mesh is not None or self.nc_owned is not None or (self.dev is not None and self.dev.nranks > 1):
            raise _abi.KnpError("record_fields: not supported with several ranks (sample the fields in a one-GPU run)")
        if self.mesh is None:
            raise _abi.KnpError("Solver.record_fields: call setup_domain first")
        ids = resolve_fields(fields, [ion['name'] for ion in self.ion_list])
        names = [fields] if isinstance(fields, str) else list(fields)
        make_spec = lambda mtags, cell_rank: FieldMeshSpec(self.mesh, self.subdomains, self.surfaces, mtags, self.degree_knp, tags=tags,
                                                           continuous=continuous, cell_rank=cell_rank)
        m = FieldSampler(make_spec, names, ids, every=every, dtype=dtype, name=name)
        if any(o.name == m.name for o in self.fieldmeshes or ()):
            raise _abi.KnpError("record_fields: a sampler named %r exists already" % m.name)
        if len(self.fieldmeshes or ()) >= MAX_SAMPLERS:
            raise _abi.KnpError("record_fields: at most %d field samplers per solver" % MAX_SAMPLERS)
        if self.dev is not None:
            m.attach(self.dev, self.membrane_tags)
        else:
            make_spec(self.membrane_tags or (), None)      # a bad selection is refused here, not when the device context appears
        self.fieldmeshes = (self.fieldmeshes or []) + [m]
        return m

    def _fieldmeshes_begin(self, k0, t):
        if self.filename is not None:
            for m in self.fieldmeshes:
                m.begin(self.filename, k0, float(t))

    def _fieldmeshes_step(self, steps_done, t):
        for m in self.fieldmeshes:
            m.after_step(steps_done, float(t))

    def _fieldmeshes_finish(self):
        """Every sampler closes its file; the first failure is raised unless the loop is already leaving with an exception."""
        leaving = sys.exc_info()[0] is not None
        failed = None
        for m in self.fieldmeshes:
            try:
                m.finish()
            except Exception as e:
                failed = failed or e
        if failed is not None and not leaving:
            raise failed

    def _save_timeseries(self):
        if self.recorder is not None and self.filename is not None:
            self.recorder.save(self.filename + 'timeseries.h5')

    def _push_params(self, splitting):
        z = [float(ion['z']) for ion in self.ion_list]
        D = np.stack([ion['D'] for ion in self.ion_list])
        # ion['f_source'] v dx(0) (solver.py:599): a number / Constant or a per-cell array travels as a DG0 coefficient on the ECS
        # cells; a callable f(x) or f(x, t) (the reference accepts any UFL coefficient, e.g. the box-and-time-window Expression
        # of run_tortuosity.py:180-200) is integrated on the host before every KNP solve (_update_sources); a knpemidg.Expression
        # is compiled for the device and integrated there (csrc/source_rtc.hpp), with no host pass and no upload.  A FieldExpression
        # (an Expression that also reads phi and concentrations, on any subdomain) is a device source too.  Both kinds are
        # registered in one place, _register_device_sources, behind the parameter upload
        from knpemidg.expression import Expression
        fsrc = None
        nc = self.mesh.num_cells()
        ecs = (self.subdomains.array() == 0).astype(np.float64)
        rows, self._callable_sources = [], {}
        exprs = {k: ion['f_source'] for k, ion in enumerate(self.ion_list[:-1]) if isinstance(ion.get('f_source', 0.0), Expression)}
        if exprs and splitting == 2:
            raise ValueError("an Expression source cannot be combined with a manufactured solution (mms), which sets its own data terms")
        for k, f in exprs.items():                       # a source whose kernel the context holds already is left alone (Device.source_register)
            known = self.dev._source_kernels.get(k)
            if (known[0] if isinstance(known, tuple) else known) != f.kernel_name(self.mesh.gdim, self.nd):
                f.prefetch(self.mesh.gdim, self.nd)      # the compiles overlap each other and the parameter upload below
        for k, ion in enumerate(self.ion_list[:-1]):
            f = ion.get('f_source', 0.0)
            if k in exprs:
                rows.append(np.zeros(nc))
            elif callable(f) and not hasattr(f, '__float__'):
                self._callable_sources[k] = f
                rows.append(np.zeros(nc))
            elif isinstance(f, np.ndarray) and f.ndim >= 1 and f.size > 1:
                if f.shape != (nc,):
                    raise ValueError("f_source array of ion %s must hold one value per cell" % ion.get('name', k))
                rows.append(f.astype(np.float64) * ecs)
            else:
                rows.append(float(f) * ecs)
        if any(r.any() for r in rows):
            fsrc = np.stack(rows)
        self.dev.set_params(_f(self.C_M), _f(self.dt), _f(self.F), _f(self.R), _f(self.temperature), _f(self.C_phi),
                            _f(self.tau_emi), _f(self.tau_knp), z, D, rho=self.rho, fsrc=fsrc, splitting=splitting)
        self._register_device_sources()

    # ------------------------------------------------------------------ forms / solvers (solver.py:270-468, 534-721)
    def setup_varform_emi(self):
        """The bilinear / linear forms are fixed kernels; only the splitting flag is data."""
        self._ensure_device()
        if self.mms is not None:
            # manufactured solution (solver.py:349-374, 632-657): data terms integrated once on the host
            from knpemidg.mms_terms import extra_rhs
            Cdev, e_emi, e_knp = extra_rhs(self)
            self.dev.set_mms(Cdev, e_emi, e_knp)
            self._push_params(2)
        else:
            self._push_params(self.splitting_scheme)
        self.I_ch = [None] * len(self.mem_models)
        return

    def setup_varform_knp(self):
        """Field names of `FieldExpression` sources are resolved and a manufactured solution refuses them here, with or without a
        device; with one, the device sources are registered (again: what the context holds already is left alone)."""
        self._register_device_sources()
        return

    def _register_device_sources(self):
        """The one place where the ion sources that are `Expression`s or `FieldExpression`s reach the device.  "phi" / "c_<name>" of
        a FieldExpression are resolved against the ion list (the eliminated ion included; ValueError for an unknown name, listing
        the ones that exist) and a manufactured solution refuses either kind before anything is loaded; then species that lost their
        device source are cleared and every device source is registered (Device.source_register compiles and loads only what the
        context does not hold already).  Without a device yet, only the checks run: setup_varform_emi comes back here."""
        from knpemidg.expression import Expression, FieldExpression
        found = {k: ion['f_source'] for k, ion in enumerate(self.ion_list[:-1]) if isinstance(ion.get('f_source', 0.0), Expression)}
        if found and self.mms is not None:
            raise ValueError("an Expression source cannot be combined with a manufactured solution (mms), which sets its own data terms")
        names = [ion.get('name', str(k)) for k, ion in enumerate(self.ion_list)]
        for f in found.values():
            if isinstance(f, FieldExpression):
                f.field_ids(names)
        if self.dev is None:
            return
        before, self._device_sources = self._device_sources, found
        for k in before:
            if k not in found:
                self.dev.source_clear(k)
        for k, f in found.items():
            self.dev.source_register(k, f, ion_names=names)

    def _update_sources(self, t):
        """Load vector of the callable ion sources at time t: int f_k(x, t) v dx(0) by a degree-8 rule per ECS cell (the reference
        interpolates its Expression to the declared degree and integrates that: run_tortuosity.py:180-200, solver.py:599).
        Host callables are integrated here and uploaded first; the sources that are `Expression`s or `FieldExpression`s are then
        evaluated on the device with their current parameter values (same rule, same stream, no host pass, no copy, no wait) and
        overwrite their rows."""
        if self.mms is not None:
            return
        self._update_host_sources(t)
        for k, f in self._device_sources.items():
            self.dev.source_eval(k, f.values())

    def _update_host_sources(self, t):
        srcs = self._callable_sources
        if not srcs:
            return
        import inspect
        from knpemidg.mms_terms import _cell_source, _geometry
        if self._src_geom is None:
            self._src_geom = (_geometry(self.mesh)[0], np.nonzero(self.subdomains.array() == 0)[0])
        vol, sel = self._src_geom
        out = np.zeros((self.N_ions, self.mesh.num_cells(), self.nd))
        for k, f in srcs.items():
            two = len(inspect.signature(f).parameters) >= 2
            _cell_source(self.mesh, vol, sel, (lambda X, f=f: f(X, float(t))) if two else f, out[k], p=self.degree_knp)
        self.dev.set_source(out)

    def setup_solver_emi(self):
        self._read_solver_params()
        # direct_emi (MUMPS in the reference, solver.py:412-422) is emulated by a tightly converged PCG with the plain
        # block-Jacobi preconditioner: it stays SPD to rounding for any coefficient contrast (the MMS problem couples
        # the membrane with C_phi = 1e10), which a V-cycle does not
        if self.use_amg and not self.direct_emi:
            self.emi_smoother = precond.SmootherChoice(self.dev, getattr(self.solver_params, "emi_dg_chebyshev", None),
                                                       (self._resume_header or {}).get("emi_dg_chebyshev"), self.verbose)
            self.dev.set_emi_dg_smoother(self.emi_smoother.chosen)
            if not self.direct_knp:
                self.amg.upload_knp_if_ready(self.dev)
            self.amg.setup_emi(self.dev)
        else:
            self.amg.drop_emi_helper()
        return

    def setup_solver_knp(self):
        if self.use_amg and not self.direct_knp:
            self.amg.setup_knp(self.dev)
        else:
            self.amg.drop_knp_helper()
        return

    def _read_solver_params(self):
        s = self.settings = resolve_settings(
            self.solver_params, degree_emi=self.degree_emi, rtol_emi=self.rtol_emi, atol_emi=self.atol_emi, rtol_knp=self.rtol_knp,
            atol_knp=self.atol_knp, direct_emi=self.direct_emi, direct_knp=self.direct_knp, max_it_emi=self.max_it_emi,
            max_it_knp=self.max_it_knp)
        (self.max_it_emi, self.max_it_knp, self._rtol_emi, self._atol_emi, self._emi_target, self._rtol_knp, self._atol_knp, _, _,
         self._knp_min_it, self._knp_early) = s
        if self.verbose:
            print(" effective tolerances: EMI %s, KNP rtol %.2e (weighted residual norm)" % (
                ("residual target %.2e x F min|z| ||b_knp||" % s.emi_target) if s.emi_target else "rtol %.2e" % s.rtol_emi, s.rtol_knp))
        if self.dev is not None:
            self.dev.knp_early_stop(s.knp_early)
        if self.dev is not None and s.knp_krylov != self._knp_krylov:
            self.dev.set_knp_krylov(s.knp_krylov, s.gmres_restart)
            self._knp_krylov = s.knp_krylov

    def _sync_membrane_to_device(self):
        """phi_M and I_ch_k facet fields produced by the ODE step -> device."""
        if not self.mem_models or all(mm['ode'].on_device for mm in self.mem_models):
            return
        A = _abi
        nf = self.mesh.num_facets()
        Ich = np.zeros((len(self.ion_list), nf))
        if any(mm['ode'].on_device for mm in self.mem_models):
            Ich = self.dev.download(A.F_I_CH).reshape(len(self.ion_list), nf)
        for mm in self.mem_models:
            if mm['ode'].on_device:
                continue
            idx = mm['ode'].indices
            for k, ion in enumerate(self.ion_list):
                Ich[k, idx] = mm['I_ch_k'][ion['name']].array()[idx]
        self.dev.upload(A.F_I_CH, Ich)

    # ------------------------------------------------------------------ solve_emi (solver.py:470-531)
    def solve_emi(self):
        dev = self.dev
        ts = time.perf_counter()
        dev.update_kappa()
        dev.emi_rhs()
        dev.sync()
        te = time.perf_counter()
        res = te - ts
        if self.verbose:
            print(f"{bcolors.OKGREEN} GPU Execution time PDE assemble emi: {res:.4f} seconds {bcolors.ENDC}")
        self.emi_ass_timer += res
        if self.save_solver_stats:
            self.file_emi_assem.write("ass_time: %.4f \n" % (res))
        ts = time.perf_counter()
        if self._emi_target:
            r_abs = self._emi_target * _f(self.F) * self._knp_load_norm()
            self.emi_targets.append(r_abs)            # identical on every rank of a partitioned run (tests/test_gpu_multirank.py)
            dev.emi_residual_target(r_abs)
        amg = self.use_amg and not self.direct_emi
        if amg and self.emi_smoother.pending and self._emi_target:
            def one_solve():
                t0 = time.perf_counter()
                n_, r_ = dev.emi_solve(self._rtol_emi, self._atol_emi, maxit=self.max_it_emi)
                return time.perf_counter() - t0, n_, r_
            _, niter, r = self.emi_smoother.run_trial(one_solve)
        else:
            niter, r = dev.emi_solve(self._rtol_emi, self._atol_emi, maxit=self.max_it_emi)
        te = time.perf_counter()
        res = te - ts
        if self.verbose:
            print(f"{bcolors.OKGREEN} GPU Execution time PDE solve emi: {res:.4f} seconds ({niter} its) {bcolors.ENDC}")
        self.emi_solve_timer += res
        self.emi_niter.append(niter)
        if amg:
            self.amg.maybe_refresh_emi(dev, self.emi_niter)
        if self.save_solver_stats:
            if not self.direct_emi:
                self.file_emi_niter.write("niter: %d \n" % niter)
            self.file_emi_solve.write("solve_time: %.4f \n" % (res))
        return

    def _knp_load_norm(self):
        """min_k |z_k| ||b_knp,k / vol||_8: size of the KNP load vectors (~ M c_k / dt) in the density norm of order 8 the solvers test
        (csrc/krylov.hip) -- from the previous KNP solve; before the first one, from the right-hand side of the initial state."""
        z = np.abs([float(ion['z']) for ion in self.ion_list[:-1]])
        bn = self._knp_bnorm
        if bn is None:
            dev = self.dev
            _abi._stamp("first step: EMI right-hand side ready")
            dev.update_dnphi(); dev.knp_rhs()
            # summed over the owned cells on the device (a partition all-reduces the sums: every rank must hand the SAME target to the PCG
            # stopping test -- ranks that disagree about convergence leave the loop of collectives at different iterations); a host
            # pass over the downloaded field cost 2 s at 8 x 10^6 cells
            sums = dev.allreduce_sum(dev.knp_load_measure())
            bn = np.sqrt(sums) if os.environ.get("KNP_KNP_NORM2", "0") == "1" else sums ** 0.125      # order-8 norm of the load density
            self._knp_bnorm = bn
            _abi._stamp("first step: KNP load norm of the initial state")
        return float(np.min(z * np.asarray(bn)))

    # ------------------------------------------------------------------ solve_knp (solver.py:723-791)
    def solve_knp(self):
        dev = self.dev
        ts = time.perf_counter()
        self._update_sources(self._t_now)
        dev.update_dnphi()
        dev.knp_rhs()
        dev.sync()
        te = time.perf_counter()
        res = te - ts
        if self.verbose:
            print(f"{bcolors.OKGREEN} GPU Execution time PDE assemble knp: {res:.4f} seconds {bcolors.ENDC}")
        self.knp_ass_timer += res
        if self.save_solver_stats:
            self.file_knp_assem.write("ass_time: %.4f \n" % (res))
        ts = time.perf_counter()
        niters, r = dev.knp_solve(self._rtol_knp, self._atol_knp, maxit=self.max_it_knp, min_it=self._knp_min_it)
        self._knp_bnorm = np.asarray(r)[:, 2].copy()
        te = time.perf_counter()
        res = te - ts
        if self.verbose:
            print(f"{bcolors.OKGREEN} GPU Execution time PDE solve knp: {res:.4f} seconds ({niters} its) {bcolors.ENDC}")
        self.knp_solve_timer += res
        self.knp_niter.append(niters)
        self.knp_residuals = r                       # per species: initial residual, final residual, |b|
        if self.save_solver_stats:
            self.file_knp_solve.write("solve_time: %.4f \n" % (res))
            if not self.direct_knp:
                self.file_knp_niter.write("niter: %d \n" % max(niters))
        return

    # ------------------------------------------------------------------ solve_for_time_step (solver.py:794-847)
    def solve_for_time_step(self, k, t):
        if self.verbose:
            print("------------------------------------------------")
            print(f"{bcolors.WARNING} t = {float(t)} {bcolors.ENDC}")
            print(f"{bcolors.WARNING} k = {k} {bcolors.ENDC}")
            print("------------------------------------------------")
        if self.mms is not None and getattr(self.mms, "time_dependent", False):
            from knpemidg.mms_terms import extra_rhs       # data terms at the current t (solver.py:845 advances t last)
            self.dev.set_mms(*extra_rhs(self))
        self._t_now = float(t)              # time-dependent sources see the t of this step (solver.py:845 advances t last)
        first = k == 0 and os.environ.get("KNP_DEBUG_SETUP", "0") == "1"       # what the very first step spends on one-time work
        if first:
            self.dev.sync(); _abi._stamp("first step: start")
        self.solve_emi()                    # step I
        if first:
            self.dev.sync(); _abi._stamp("first step: EMI solve (block-Jacobi build, smoother trial, graph capture)")
        self.solve_knp()                    # step II
        if first:
            self.dev.sync(); _abi._stamp("first step: KNP solve")
        self.dev.step_updates()             # step III: c_prev <- c, phi_M, E_k, c_elim
        if first:
            self.dev.sync(); _abi._stamp("first step: step III")
        t.assign(float(t + self.dt))
        if self.recorder is not None:
            self.recorder.sample(float(t))
        self._k_done, self._t_done = k + 1, float(t)          # what a checkpoint written now continues from
        return

    # ------------------------------------------------------------------ Picard variant (solver.py:850-927)
    def solve_for_time_step_picard(self, k, t):
        """One global step with inner Picard iterations on the two PDE solves (tolerance 1e-4 on the inf-norm of the
        concentration update, at most 25 iterations, then sys.exit(2) -- reference semantics)."""
        if self.verbose:
            print(f"{bcolors.WARNING} t = {float(t)}  k = {k} (Picard) {bcolors.ENDC}")
        t.assign(float(t + self.dt))
        self._t_now = float(t)
        tol, eps, max_iter, it = 1.0e-4, 2.0, 25, 0
        A = _abi
        while eps > tol:
            it += 1
            self.dev.copy_field(A.F_X, A.F_C)               # c_prev_k of this Picard level
            self.solve_emi()
            self.solve_knp()
            eps = self.dev.max_abs_diff(A.F_X, A.F_C)
            self.dev.picard_updates()                       # c_prev_k <- c (same field), E_k, c_elim for the next level
            if it > max_iter:
                print("Picard solver diverged")
                sys.exit(2)
        self.dev.step_updates()                             # c_prev_n <- c_prev_k, phi_M, (E_k, c_elim unchanged)
        if self.recorder is not None:
            self.recorder.sample(float(t))
        self.picard_iters = self.picard_iters + [it]
        self._k_done, self._t_done, self._picard = k + 1, float(t), True
        if self.verbose:
            print(f" Summary Picard: eps = {eps}, #iters = {it}")
        return

    def _unpack_solver_params(self, solver_params):
        self.solver_params = solver_params
        self.direct_emi = solver_params.direct_emi
        if not self.direct_emi:
            self.rtol_emi = solver_params.rtol_emi
            self.atol_emi = solver_params.atol_emi
            self.threshold_emi = solver_params.threshold_emi      # accepted and ignored (no hypre)
        self.direct_knp = solver_params.direct_knp
        if not self.direct_knp:
            self.rtol_knp = solver_params.rtol_knp
            self.atol_knp = solver_params.atol_knp
            self.threshold_knp = solver_params.threshold_knp

    def _check_output_args(self, filename):
        if filename is None and (self.save_solver_stats or self.save_fields):
            print("Please specify filename when initiating Solver.solve_system_*() method")
            sys.exit(0)
        # a resumed run writes a SECOND PART next to the files of the first: results_from<k>.h5 (with /step_offset = k; its vector_0 is the
        # restored state) and solver_from<k>/; timeseries.h5 is written whole, the recorder carries the rows of the first part
        k0 = int(self._resume_k or 0)
        part = "_from%d" % k0 if k0 else ""
        if self.save_fields:
            self.init_h5_savefile(filename + 'results%s.h5' % part)                 # solver.py:978, 1063
            if k0:
                self.h5_file.write("/step_offset", np.asarray([k0], dtype=np.int64))
        if self.save_solver_stats:
            self.init_solver_stats(filename + 'solver%s/' % part)

    # ------------------------------------------------------------------ solve_system_passive (solver.py:930-1011)
    def solve_system_passive(self, Tstop, t, solver_params, membrane_params, filename=None, save_fields=False,
                             save_solver_stats=False, *, checkpoint_every=None, checkpoint_file=None, resume=None):
        """checkpoint_every / checkpoint_file / resume: see solve_system_active."""
        self.filename = filename
        self.save_fields = save_fields
        self.save_solver_stats = save_solver_stats
        self._unpack_solver_params(solver_params)
        self.splitting_scheme = False
        ckpt = self._checkpoint_args(checkpoint_every, checkpoint_file, resume)
        self.setup_varform_emi()
        self.setup_varform_knp()
        self.setup_solver_emi()
        self.setup_solver_knp()
        k0 = self.load_checkpoint(resume, t=t) if resume is not None else 0
        self._check_output_args(filename)
        if self.recorder is not None and k0 == 0:
            self.recorder.arm(float(t))
        if self.grids is not None:
            self._grids_begin(k0, t)
        if self.surfaces_rec is not None:
            self._surfaces_begin(k0, t)
        try:
            if self.fieldmeshes is not None:
                self._fieldmeshes_begin(k0, t)
            for k in range(k0, int(round(Tstop / float(self.dt)))):
                self.solve_for_time_step(k, t)
                if (k % self.sf) == 0 and self.save_fields:
                    self.save_h5()
                if self.grids is not None:
                    self._grids_step(k + 1, t)
                if self.surfaces_rec is not None:
                    self._surfaces_step(k + 1, t)
                if self.fieldmeshes is not None:
                    self._fieldmeshes_step(k + 1, t)
                if ckpt is not None and (k + 1) % ckpt[0] == 0:
                    self.save_checkpoint(ckpt[1])
        finally:
            if self.fieldmeshes is not None:
                self._fieldmeshes_finish()           # also when the loop raises: the frames taken so far are a file
        if self.save_fields:
            self.close_h5()
        if self.grids is not None:
            self._grids_finish()
        if self.surfaces_rec is not None:
            self._surfaces_finish()
        self._save_timeseries()
        if self.save_solver_stats:
            self.close_solver_stats()
        uh = self.c.split() + (self.phi,)
        return uh, self.ion_list[-1]['c']

    # ------------------------------------------------------------------ solve_system_active (solver.py:1014-1135)
    def solve_system_active(self, Tstop, t, solver_params, filename=None, save_fields=False, save_solver_stats=False, *,
                            checkpoint_every=None, checkpoint_file=None, resume=None):
        """checkpoint_every = N writes `checkpoint_file` (default <filename>checkpoint.h5) after every N-th completed step;
        resume = path continues the run a checkpoint was written from: the setups run as usual, the state is loaded, `t` is set and
        the loop runs from the stored step to round(Tstop / dt) (knpemidg/checkpoint.py).  All three default
        to off: nothing is written and no step changes."""
        self.filename = filename
        self.save_fields = save_fields
        self.save_solver_stats = save_solver_stats
        self._unpack_solver_params(solver_params)
        self.splitting_scheme = True
        ckpt = self._checkpoint_args(checkpoint_every, checkpoint_file, resume)
        self.setup_varform_emi()
        self.setup_varform_knp()
        self.setup_solver_emi()
        self.setup_solver_knp()
        k0 = self.load_checkpoint(resume, t=t) if resume is not None else 0
        self._check_output_args(filename)
        if self.grids is not None:
            self._grids_begin(k0, t)
        if self.surfaces_rec is not None:
            self._surfaces_begin(k0, t)
        try:
            if self.fieldmeshes is not None:
                self._fieldmeshes_begin(k0, t)
            for k in range(k0, int(round(Tstop / float(self.dt)))):
                self.step_membrane_models(k)
                if k == 0 and self.recorder is not None:
                    # the time loop starts: with phi_M_init_type 'constant' PHI_M holds the membrane potential only from here on (it
                    # comes from the ODE states in the first membrane step), so this is where the map takes its starting values
                    self.recorder.arm(float(t))
                self.solve_for_time_step(k, t)
                if (k % self.sf) == 0 and self.save_fields:
                    self.save_h5()
                if self.grids is not None:
                    self._grids_step(k + 1, t)
                if self.surfaces_rec is not None:
                    self._surfaces_step(k + 1, t)
                if self.fieldmeshes is not None:
                    self._fieldmeshes_step(k + 1, t)
                if ckpt is not None and (k + 1) % ckpt[0] == 0:
                    self.save_checkpoint(ckpt[1])
        finally:
            if self.fieldmeshes is not None:
                self._fieldmeshes_finish()           # also when the loop raises: the frames taken so far are a file
        if self.save_fields:
            self.close_h5()
        if self.grids is not None:
            self._grids_finish()
        if self.surfaces_rec is not None:
            self._surfaces_finish()
        self._save_timeseries()
        if self.save_solver_stats:
            self.close_solver_stats()
        return

    # ------------------------------------------------------------------ checkpoint / resume (no reference counterpart: knpemidg/checkpoint.py)
    def _checkpoint_args(self, every, path, resume):
        """(N, file) of the periodic checkpoints or None; with `resume`, reads the file's header before the setups run (the recorded
        smoother choice replaces the first-step trial)."""
        self._resume_header = None
        self._resume_k = 0
        if resume is not None:
            from knpemidg import checkpoint
            self._resume_header = checkpoint.read_checkpoint(resume)[0]
        if every is None:
            return None
        if int(every) < 1:
            raise _abi.KnpError("checkpoint_every must be a positive number of steps")
        if path is None:
            if self.filename is None:
                raise _abi.KnpError("checkpoint_every needs checkpoint_file (or filename, for <filename>checkpoint.h5)")
            path = self.filename + "checkpoint.h5"
        return int(every), path

    def _checkpoint_mode(self, picard=None):
        if picard if picard is not None else self._picard:
            return "picard"
        return "splitting" if self.splitting_scheme else "passive"

    def _checkpoint_header(self, picard=None):
        """The fields a checkpoint is checked against (checkpoint.CHECKED_FIELDS) plus what a reader wants to know about the run."""
        from knpemidg import checkpoint
        models = [{"name": getattr(m['ode'].ode, "__name__", "ode").split(".")[-1], "tag": int(m['ode'].tag), "nodes": int(m['ode'].nodes),
                   "on_device": bool(m['ode'].on_device), "states": _names(m['ode'].ode, "state"), "parameters": _names(m['ode'].ode, "parameter")}
                  for m in self.mem_models]
        for entry, m in zip(models, self.mem_models):        # only when it is not the default: files from before the choice keep loading
            if m['ode'].ode_method != "dp5":
                entry["ode_method"] = m['ode'].ode_method
        sp = self.solver_params
        smoother = self.emi_smoother
        return {
            "dt": float(self.dt),
            "ions": [[str(ion['name']), float(ion['z'])] for ion in self.ion_list],
            "degrees": [int(self.degree_emi), int(self.degree_knp)],
            "n_cells": int(self.mesh.num_cells()), "n_vertices": int(self.mesh.coords.shape[0]),
            "mesh_hash": checkpoint.mesh_hash(self.mesh.coords, self.mesh.cells),
            "mode": self._checkpoint_mode(picard),
            "models": models,
            "rtc_hash": [checkpoint.source_hash(getattr(m['ode'].ode, "HIP_RHS", None)) for m in self.mem_models],
            "solver_params": {k: (v if isinstance(v, (bool, int, float, str, type(None))) else repr(v)) for k, v in sp._asdict().items()}
            if hasattr(sp, "_asdict") else None,
            "emi_dg_chebyshev": smoother.chosen if (smoother is not None and self.use_amg and not self.direct_emi) else None,
            "emi_trial_pending": smoother is not None and smoother.pending,
            "amg_refresh": self.amg.state(),
        }

    def save_checkpoint(self, path, t=None, k=None):
        """Write the complete step-to-step state after the last completed step to one HDF5 file (knpemidg/checkpoint.py): the device
        snapshot in the caller's numbering plus the host-side state of the solver, the membrane models and the recorder.  t, k default
        to the end of the last step this solver took.  Written under a temporary name and renamed: never half a file at `path`."""
        from knpemidg import checkpoint
        if self.dev is None:
            raise _abi.KnpError("save_checkpoint: no device context yet")
        if self.local_mesh is not None or self.nc_owned is not None or self.dev.nranks > 1:
            raise _abi.KnpError("save_checkpoint: not supported with several ranks (checkpoint a one-GPU run)")
        header = self._checkpoint_header()
        header["k"] = int(self._k_done if k is None else k)
        header["t"] = float(self._t_done if t is None else t)
        table, arrays = checkpoint.split_snapshot(self.dev.state_save())
        extra = {"emi_niter": np.asarray(self.emi_niter, dtype=np.int64),
                 "knp_niter": np.asarray(self.knp_niter, dtype=np.int64).reshape(len(self.knp_niter), max(self.N_ions, 1)),
                 "emi_targets": np.asarray(self.emi_targets, dtype=np.float64),
                 "picard_iters": np.asarray(self.picard_iters, dtype=np.int64),
                 "model_time": np.asarray([float(m['ode'].time) for m in self.mem_models], dtype=np.float64)}
        if self._knp_bnorm is not None:
            extra["knp_bnorm"] = np.asarray(self._knp_bnorm, dtype=np.float64)
        for i, m in enumerate(self.mem_models):
            extra.update(m['ode'].host_state("model%d_" % i))
        if self.recorder is not None:
            extra.update(self.recorder.host_state("recorder_"))
        return checkpoint.write_checkpoint(path, header, table, arrays, extra)

    def load_checkpoint(self, path, t=None, picard=None):
        """Restore a checkpoint into this solver AFTER its setup_* calls; returns the step index k to continue with and sets `t`.
        The header is checked first (KnpError naming the first field that differs; the solver is untouched then), the state goes to
        the device without passing the invalidating upload path, and the EMI hierarchy is rebuilt from the restored kappa.  picard:
        pass True when solve_for_time_step_picard is driven by hand (the mode of a checkpoint is part of what is compared)."""
        from knpemidg import checkpoint
        if self.dev is None:
            raise _abi.KnpError("load_checkpoint: no device context yet")
        if self.local_mesh is not None or self.nc_owned is not None or self.dev.nranks > 1:
            raise _abi.KnpError("load_checkpoint: not supported with several ranks (checkpoint a one-GPU run)")
        header, table, arrays, extra = checkpoint.read_checkpoint(path)
        checkpoint.check_header(header, dict(self._checkpoint_header(picard), format_version=checkpoint.FORMAT_VERSION), "checkpoint %s" % path)
        checkpoint.check_table(table, self.dev.state_describe()[0], "checkpoint %s" % path)
        amg = self.use_amg and not self.direct_emi
        if amg and header.get("emi_dg_chebyshev") is not None and not header.get("emi_trial_pending"):
            self.emi_smoother.resume(header["emi_dg_chebyshev"])           # before the state: a change of smoother drops the spectral bound
        self.dev.state_load(checkpoint.join_snapshot(table, arrays))
        self.emi_niter = [int(v) for v in extra.get("emi_niter", [])]
        self.knp_niter = [[int(v) for v in row] for row in extra.get("knp_niter", np.zeros((0, self.N_ions)))]
        self.emi_targets = [float(v) for v in extra.get("emi_targets", [])]
        if "picard_iters" in extra:
            self.picard_iters = [int(v) for v in extra["picard_iters"]]
        self._knp_bnorm = np.asarray(extra["knp_bnorm"], dtype=np.float64).copy() if "knp_bnorm" in extra else None
        for i, m in enumerate(self.mem_models):
            m['ode'].time = float(extra["model_time"][i])
            m['ode'].load_host_state("model%d_" % i, extra)
        if self.recorder is not None:
            self.recorder.load_host_state("recorder_", extra)
        self.amg.restore(header.get("amg_refresh"))
        if amg:
            self.amg.drop_emi_helper()
            self.amg.setup_emi(self.dev)                       # from the restored kappa
        self._k_done, self._t_done = int(header["k"]), float(header["t"])
        self._resume_k = self._k_done
        if header["mode"] == "picard":
            self._picard = True
        if t is not None:
            t.assign(self._t_done)
        return self._k_done

    def step_membrane_models(self, k):
        """ODE step of every membrane model + PDE<->ODE copies (solver.py:1076-1118)."""
        ts = time.perf_counter()
        dt_ode = float(self.dt)
        for mem_model in self.mem_models:
            ode_model = mem_model['ode']
            if (self.phi_M_init_type == 'constant') and (k == 0):
                pass
            else:
                ode_model.set_membrane_potential(self.phi_M_prev_PDE)
            for i, ion in enumerate(self.ion_list):
                ode_model.set_parameter(f"E_{ion['name']}", ion['E'])
            self.update_ode(ode_model)
            ode_model.step_lsoda(dt=dt_ode, stimulus=self.stimulus, stimulus_locator=self.stimulus_locator)
            ode_model.get_membrane_potential(self.phi_M_prev_PDE)
            for ion, I_ch_k in mem_model['I_ch_k'].items():
                ode_model.get_parameter("I_ch_" + ion, I_ch_k)
        self._sync_membrane_to_device()
        res = time.perf_counter() - ts
        self.ode_solve_timer += res
        if self.verbose:
            print(f"{bcolors.OKGREEN} CPU Execution time ODE solve: {res:.4f} seconds {bcolors.ENDC}")

    def update_ode(self, ode_model):
        raise NotImplementedError("Subclasses must implement the 'update_ode' function.")

    # ------------------------------------------------------------------ solver statistics (solver.py:1146-1211)
    def init_solver_stats(self, path_timings):
        os.makedirs(path_timings, exist_ok=True)
        reso = getattr(self.solver_params, "resolution", 0)
        num_cells = self.mesh.num_cells()
        dofs_emi = num_cells * self.nd
        dofs_knp = dofs_emi * self.N_ions
        sfx_e = "_dir" if self.direct_emi else ""
        sfx_k = "_dir" if self.direct_knp else ""
        self.file_emi_solve = open(path_timings + "emi_solve%s_%d.txt" % (sfx_e, reso), "w")
        self.file_emi_assem = open(path_timings + "emi_assem%s_%d.txt" % (sfx_e, reso), "w")
        self.file_emi_niter = None if self.direct_emi else open(path_timings + "emi_niter_%d.txt" % reso, "w")
        self.file_knp_solve = open(path_timings + "knp_solve%s_%d.txt" % (sfx_k, reso), "w")
        self.file_knp_assem = open(path_timings + "knp_assem%s_%d.txt" % (sfx_k, reso), "w")
        self.file_knp_niter = None if self.direct_knp else open(path_timings + "knp_niter_%d.txt" % reso, "w")
        for f, dofs in ((self.file_emi_solve, dofs_emi), (self.file_emi_assem, dofs_emi), (self.file_emi_niter, dofs_emi),
                        (self.file_knp_solve, dofs_knp), (self.file_knp_assem, dofs_knp), (self.file_knp_niter, dofs_knp)):
            if f is not None:
                f.write("num cells: %d \n" % num_cells)
                f.write("dofs: %d \n" % dofs)

    def close_solver_stats(self):
        for f in (self.file_emi_niter, self.file_knp_niter, self.file_emi_solve, self.file_knp_solve,
                  self.file_emi_assem, self.file_knp_assem):
            if f is not None:
                f.close()

    # ------------------------------------------------------------------ field output (solver.py:1214-1242)
    # One HDF5 file `<filename>.h5` with the reference's dataset names (written by knpemidg.h5lite.H5Writer; no h5py here):
    #   /mesh/coordinates, /mesh/topology, /subdomains/values, /surfaces/values (+ /surfaces/topology: facet vertices),
    #   /concentrations/vector_n, /elim_concentration/vector_n, /potential/vector_n   (n = 0: initial state, then every sf-th step)
    # plus this build's DG dof layout per field (cell_dofs / x_cell_dofs as DOLFIN stores them): dof(c, j) = c nd + j, species-major
    # for the mixed concentration function.  A distributed run writes one file per rank (`..._rank<r>.h5`) holding its owned +
    # ghost cells and /cells_global, the local -> global cell map.
    def init_h5_savefile(self, filename):
        from knpemidg.h5lite import H5Writer
        self.h5_idx = 0
        os.makedirs(os.path.dirname(filename) or ".", exist_ok=True)
        loc = self.local_mesh
        rank_sfx = "" if loc is None else "_rank%d" % getattr(self.dev, "rank", loc.rank)
        stem, ext = os.path.splitext(filename)                      # the reference passes the full file name (solver.py:978, 1214)
        self.h5_path = stem + rank_sfx + (ext or ".h5")
        w = self.h5_file = H5Writer(self.h5_path)
        w.write("/mesh/coordinates", self.mesh.coords)
        w.write("/mesh/topology", self.mesh.cells.astype(np.int64))
        w.write("/subdomains/values", np.asarray(self.subdomains.array()).astype(np.uint64))
        w.write("/surfaces/values", np.asarray(self.surfaces.array()).astype(np.uint64))
        w.write("/surfaces/topology", self.mesh.facets.astype(np.int64))
        if loc is not None:
            w.write("/cells_global", loc.cells_global.astype(np.int64))
        nc, nd = self.mesh.num_cells(), self.nd
        base = (np.arange(nc)[:, None] * nd + np.arange(nd)[None, :]).astype(np.int64)
        for name, ncomp in (("concentrations", self.N_ions), ("elim_concentration", 1), ("potential", 1)):
            dofs = np.concatenate([base + k * nc * nd for k in range(ncomp)], axis=1)
            w.write("/%s/cell_dofs" % name, dofs.ravel())
            w.write("/%s/x_cell_dofs" % name, (np.arange(nc + 1) * dofs.shape[1]).astype(np.int64))
            w.write("/%s/cells" % name, np.arange(nc, dtype=np.int64))
        self._write_snapshot()

    def _write_snapshot(self):
        w = self.h5_file
        w.write("/concentrations/vector_%d" % self.h5_idx, self.c.array().ravel())
        w.write("/elim_concentration/vector_%d" % self.h5_idx, self.ion_list[-1]['c'].array().ravel())
        w.write("/potential/vector_%d" % self.h5_idx, self.phi.array().ravel())

    def save_h5(self):
        self.h5_idx += 1
        self._write_snapshot()

    def close_h5(self):
        self.h5_file.close()
        return
