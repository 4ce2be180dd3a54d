"""Host side of the Krylov preconditioners: what `Solver` needs around the device's V-cycles (csrc/amg_*.hip) and block-Jacobi smoothers.

    SmootherChoice   the DG-level smoother of the EMI preconditioner: explicit, recorded in a checkpoint, or measured on the first solve
    AmgSetup         the auxiliary-space hierarchies: helper processes, in-process builds, the row-distributed level 0 of a partitioned
                     run, the uploads and the refresh policy of the lagged EMI hierarchy, with its counters

Neither knows the `Solver`: SmootherChoice takes the device and its three inputs, AmgSetup one read-only record (`AmgInputs`) and the
device per call (the helper processes start before the device context exists).  Both run on the CPU against a stand-in device
(tests/test_precond_host.py)."""
import os
import time
from typing import NamedTuple

import numpy as np

from knpemidg import _abi


class SmootherChoice:
    """DG-level smoother of the EMI preconditioner at setup time: the two-step Chebyshev block-Jacobi (one more operator apply per PCG
    iteration, fewer iterations) unless `setting` (`emi_dg_chebyshev` in solver_params), else KNP_EMI_CHEB, decides explicitly.  Whether
    the extra apply pays depends on where the run sits between the launch-latency and the bandwidth regime and on the mesh quality (r=2:
    4.25 -> 4.7 iterations without it for a quarter less work per iteration; EMIx reconstruction: 9.2 -> 13.5 iterations), so it is
    MEASURED on the first EMI system of the run itself (run_trial) instead of being read off mesh-size thresholds (round 3).
      pending    a trial is still to run on the first EMI solve
      chosen     the smoother in use: True = Chebyshev step
      measured   None until a trial has run, then its {"chebyshev_s_per_decade", "plain_s_per_decade", "chosen"}"""

    def __init__(self, dev, setting=None, recorded=None, verbose=True):
        self.dev, self.setting, self.verbose = dev, setting, verbose
        explicit = setting
        if explicit is None and os.environ.get("KNP_EMI_CHEB") is not None:
            explicit = int(os.environ["KNP_EMI_CHEB"]) != 0                # the device reads the same variable as an override (csrc/solve.hip)
        if explicit is None and recorded is not None:
            explicit = bool(recorded)                                      # a resumed run keeps the choice its first part measured
        self.pending = explicit is None
        self.chosen = True if explicit is None else bool(explicit)
        self.measured = None

    def resume(self, recorded):
        """The choice a checkpoint recorded, unless solver_params decide: set on the device, and no trial solves in a resumed run."""
        self.chosen = bool(recorded) if self.setting is None else bool(self.setting)
        self.dev.set_emi_dg_smoother(self.chosen)
        self.pending = False

    def run_trial(self, solve):
        """Measured choice of the EMI DG-level smoother, on the FIRST EMI system of the run: the same right-hand side is solved from the
        same initial guess with the Chebyshev step and with plain block-Jacobi (one untimed solve each first: eigenvalue estimate, graph
        capture, code-object loads), each charged its wall time per decade of TRUE-residual reduction; the times are summed over the
        ranks of a partitioned run (one all-reduce: every rank takes the same decision and keeps ONE symmetric preconditioner).  The
        step stays unless dropping it is at least 3 % cheaper.  The time stepping itself never changes preconditioner: a trial spread
        over the first steps of the run (tried first) perturbed the extrapolated initial guesses of the steps behind it (r=2: EMI 4.6 ->
        5.2, KNP 5.1 -> 5.4 iterations per step over the next 20 steps, profiles/r04_smoother_trial.txt).  Both variants meet the same
        stopping test, which does not depend on the preconditioner (csrc/krylov.hip: cg_converged), so the last solve's result IS the
        step's solution.  solve() -> (seconds, niter, res) runs one EMI solve on the current device state."""
        dev = self.dev
        phi0 = dev.download(_abi.F_PHI)
        cost = {}
        out = None
        for timed in (False, True):
            for cheb in (True, False):
                dev.set_emi_dg_smoother(cheb)
                dev.upload(_abi.F_PHI, phi0)                       # same initial guess; a caller-supplied state is no history point
                sec, niter, res = solve()
                if timed:
                    decades = max(np.log10(max(float(res[0]), 1e-300) / max(float(res[1]), 1e-300)), 0.25)
                    cost[cheb] = sec / decades
                out = (sec, niter, res)
        on, off = dev.allreduce_sum([cost[True], cost[False]])
        keep = not (off < 0.97 * on)
        self.measured = {"chebyshev_s_per_decade": float(on), "plain_s_per_decade": float(off), "chosen": bool(keep)}
        if self.verbose:
            print(" EMI DG-level smoother: Chebyshev step %.3f ms / decade, plain block-Jacobi %.3f ms / decade -> %s"
                  % (1e3 * on, 1e3 * off, "Chebyshev" if keep else "plain"))
        self.pending = False
        self.chosen = bool(keep)
        if keep:                                                   # the last solve ran without the step: redo with the chosen one
            dev.set_emi_dg_smoother(True)
            dev.upload(_abi.F_PHI, phi0)
            out = solve()
        return out


class AmgInputs(NamedTuple):
    """What the hierarchies are built from, as the solver holds it once its device context is being created."""
    mesh: object                 # this process's mesh, cell tags and facet tags (objects with .array())
    subdomains: object
    surfaces: object
    global_mesh_tuple: object    # (mesh, subdomains, surfaces) of the global mesh when this solver holds one partition of it, else None
    local_mesh: object           # partition.LocalMesh of a partitioned run, else None
    degree: int
    nd: int                      # nodes per cell
    ion_list: list
    dt: float
    F: float
    psi: float
    C_phi: float
    membrane_tags: list
    init_c: object               # initial concentrations [N_ions, nc, nd] and [nc, nd] (eliminated ion)
    init_c_elim: object
    verbose: bool


def _by_tag(d, subdomains):
    tags = subdomains.array()
    q = np.zeros(len(tags), dtype=np.float64)
    for key, value in d.items():
        q[tags == int(key)] = float(value)
    return q


class AmgSetup:
    """The auxiliary-space hierarchies of both Krylov preconditioners, from the helper processes to the device (the reference builds
    BoomerAMG from BB_emi / BB_knp, solver.py:433, 505, 688).
      emi_helper, knp_helper   (handle, what it was started from) while a helper process runs, else None
      cspace, cspace2          the conforming spaces, None until something is built in this process
      refresh, kappa0          counters of the refresh policy {"solves", "ref", "high"}; the kappa the EMI hierarchy was built from
      refreshes, dist0_uploads, setup_seconds"""

    def __init__(self, inputs):
        self.inp = inputs
        self.emi_helper = self.knp_helper = None
        self.cspace = self.cspace2 = None
        self.dist0_space = None
        self.dg2cg_helper = None
        self.knp_uploaded_early = False
        self.refresh = {"solves": 0, "ref": None, "high": 0}
        self.kappa0 = None
        self.refreshes = 0
        self.dist0_uploads = 0           # hierarchies uploaded in the row-distributed form
        self.setup_seconds = 0.0

    # ------------------------------------------------------------------ checkpoint
    def state(self):
        """The "amg_refresh" entry of a checkpoint header."""
        ref = self.refresh
        return {"solves": int(ref.get("solves", 0)), "ref": ref.get("ref"), "high": int(ref.get("high", 0)), "refreshes": int(self.refreshes)}

    def restore(self, entry):
        ref = entry or {}
        self.refresh = {"solves": int(ref.get("solves", 0)), "ref": ref.get("ref"), "high": int(ref.get("high", 0))}
        if ref.get("refreshes"):
            self.refreshes = int(ref["refreshes"])

    # ------------------------------------------------------------------ helper processes
    def _host_initial_kappa(self):
        """kappa = F psi sum_k z_k^2 D_k c_k of the initial state, nodal [nc, nd] (what k_kappa computes on the device)."""
        p = self.inp
        kappa = np.zeros((p.mesh.num_cells(), p.nd))
        for idx, ion in enumerate(p.ion_list):
            c = p.init_c_elim if idx == len(p.ion_list) - 1 else p.init_c[idx]
            kappa += p.F * float(ion['z']) ** 2 * p.psi * np.asarray(ion['D'], dtype=np.float64)[:, None] * c
        return kappa

    def start_emi_helper(self):
        """First EMI hierarchy (from the initial state) in a helper process, next to the KNP one (knpemidg/setup_worker.py).
        Not for partitions (their hierarchy is the global one) and not for manufactured solutions (direct_emi)."""
        p = self.inp
        if os.environ.get("KNP_AMG_SERIAL_SETUP", "0") == "1" or self.emi_helper is not None or p.global_mesh_tuple is not None:
            return
        from knpemidg import setup_worker
        kappa = self._host_initial_kappa()
        job = setup_worker.emi_job(p.mesh, p.surfaces.array(), p.membrane_tags, p.degree, kappa, p.C_phi)
        self.emi_helper = (setup_worker.start(job), kappa)

    def drop_emi_helper(self):
        helper, self.emi_helper = self.emi_helper, None
        if helper is not None:
            from knpemidg import setup_worker
            setup_worker.cancel(helper[0])

    def start_knp_helper(self):
        """KNP hierarchies depend only on the mesh, D_k and dt: a helper process builds them while this process creates the device
        context and the EMI hierarchy (knpemidg/setup_worker.py: why a process and not a thread).  KNP_AMG_SERIAL_SETUP=1 or a
        failure of the helper: built in this process by setup_knp."""
        p = self.inp
        if os.environ.get("KNP_AMG_SERIAL_SETUP", "0") == "1" or self.knp_helper is not None:
            return
        from knpemidg import setup_worker
        g = p.global_mesh_tuple or (p.mesh, p.subdomains, p.surfaces)
        d0 = self._knp_level0_degree()
        job = setup_worker.job_from_solver(g[0], g[1].array(), g[2].array(), p.membrane_tags, p.degree,
                                           [ion['D_sub'] for ion in p.ion_list[:-1]], p.dt, d0)
        self.knp_helper = (setup_worker.start(job), d0)

    def drop_knp_helper(self):
        helper, self.knp_helper = self.knp_helper, None
        if helper is not None:
            from knpemidg import setup_worker
            setup_worker.cancel(helper[0])

    # ------------------------------------------------------------------ spaces
    def _amg_global(self):
        """(mesh, subdomains, surfaces) the conforming hierarchy is built on: the global mesh when this solver
        holds one partition of it (make_distributed_solver), else its own mesh."""
        from knpemidg import amg
        p = self.inp
        g = p.global_mesh_tuple or (p.mesh, p.subdomains, p.surfaces)
        if self.cspace is None:
            self.cspace = amg.ConformingSpace(g[0], g[2].array(), p.membrane_tags)
            if p.degree != 1:
                self.cspace2 = amg.ConformingSpaceP2(self.cspace)
        return g

    def _dist0(self, dev):
        """Row distribution of the finest conforming level over the ranks of a partitioned run (amg.Dist0Space; the reference's BoomerAMG
        is row-distributed by PETSc, solver.py:433, 688), with the shared-dof tables handed to the device on the first call; None on one
        rank and with KNP_AMG_DIST0=0 (replicated level 0 behind an all-reduce of the level-0 residual, rounds 1-2)."""
        p = self.inp
        loc = p.local_mesh
        if loc is None or getattr(loc, "part", None) is None or loc.part.world < 2 or os.environ.get("KNP_AMG_DIST0", "1") == "0":
            return None
        d0 = self.dist0_space
        if d0 is None:
            from knpemidg import amg
            gmesh, gsub, gsurf = self._amg_global()
            space = self.cspace if p.degree == 1 else self.cspace2
            mem = np.nonzero((gmesh.facet_cells[:, 1] >= 0) & np.isin(np.asarray(gsurf.array()), list(p.membrane_tags)))[0]
            d0 = amg.Dist0Space(space, loc.part.owner, mem, loc.rank, loc.part.world)
            dev.amg_interface(d0.n, *d0.interface_tables())
            self.dist0_space = d0
        return d0

    def _local_dg2cg(self):
        p = self.inp
        loc = p.local_mesh
        if loc is None and self.cspace is None and self.dg2cg_helper is not None:
            return self.dg2cg_helper              # spaces built by the helper process only (same deterministic numbering)
        self._amg_global()
        dof = self.cspace.dof if p.degree == 1 else self.cspace2.dof
        return dof if loc is None else dof[loc.cells_global]

    # ------------------------------------------------------------------ EMI
    def setup_emi(self, dev):
        """Preconditioner setup (the reference builds BoomerAMG from BB_emi, solver.py:433, 505): conforming
        P1 operator from the current kappa + smoothed-aggregation hierarchy, built on the host once and reused
        across time steps."""
        from knpemidg import amg
        ts = time.perf_counter()
        p = self.inp
        levels = dg2cg = None
        helper, self.emi_helper = self.emi_helper, None
        if helper is not None:
            # first build: collected from the helper process if the device state still is the initial state it was given
            from knpemidg import setup_worker
            handle, kappa_h = helper
            dev.update_kappa()
            kappa = dev.download(_abi.F_KAPPA).reshape(p.mesh.num_cells(), p.nd)
            if np.allclose(kappa, kappa_h, rtol=1e-8, atol=0.0):
                _abi._stamp("solver: waiting for the EMI helper")
                res = setup_worker.collect(handle)
                _abi._stamp("solver: EMI hierarchy collected")
                if res is not None:
                    levels, dg2cg = res["levels"], res["dof"]
                    self.kappa0 = kappa.ravel().copy()
                    self.dg2cg_helper = dg2cg
            else:
                setup_worker.cancel(handle)
        if levels is None:
            gmesh, gsub, gsurf = self._amg_global()
            if gmesh is p.mesh:
                dev.update_kappa()
                kappa = dev.download(_abi.F_KAPPA).reshape(p.mesh.num_cells(), p.nd)
                self.kappa0 = kappa.ravel().copy()               # what the hierarchy was built from (refresh policy)
            else:
                # distributed: every rank builds the SAME global hierarchy from the tag-wise initial state (no
                # communication; the preconditioner is lagged anyway)
                kappa = np.zeros(gmesh.num_cells())
                for ion in p.ion_list:
                    if ion['c_init_sub_type'] != 'constant':
                        raise NotImplementedError("distributed AMG setup needs tag-wise constant initial concentrations")
                    D = _by_tag(ion['D_sub'], gsub)
                    c0 = _by_tag(ion['c_init_sub'], gsub)
                    kappa += p.F * float(ion['z']) ** 2 * p.psi * D * c0
            levels = amg.build_emi_levels(self.cspace, self.cspace2 if p.degree != 1 else None, gsurf.array(),
                                          p.membrane_tags, kappa, p.C_phi)
            dg2cg = self._local_dg2cg()
            d0 = self._dist0(dev)
            if d0 is not None:                      # partitioned run: this rank's rows of the finest conforming level
                local = d0.localize(levels)
                if local is not None:
                    dev.amg_upload(0, d0.local_dg2cg(p.local_mesh.cells_global), local, dist0=True)
                    self.dist0_uploads += 1
                    levels = None
        if levels is not None:
            dev.amg_upload(0, dg2cg, levels)
            _abi._stamp("solver: EMI hierarchy uploaded")
            nlev = [lv.A.shape[0] for lv in levels]
        else:
            nlev = [lv.A.shape[0] for lv in local]
        self.setup_seconds = time.perf_counter() - ts
        if p.verbose:
            print(" AMG(EMI) levels:", nlev, "setup %.2f s" % self.setup_seconds)

    def maybe_refresh_emi(self, dev, emi_niter):
        """Refresh policy of the lagged EMI hierarchy, called after every EMI solve with the iteration counts so far, the last one
        included.  The reference rebuilds BoomerAMG from the freshly assembled B_emi at
        EVERY solve (solver.py:479, 505); here the hierarchy is built from kappa at setup time and rebuilt when it has gone
        stale: (a) kappa has moved by more than KNP_AMG_REFRESH_KAPPA (default 25 %) anywhere since the last build (checked
        every KNP_AMG_REFRESH_EVERY = 50 solves), or (b) the PCG iteration count has stayed above 3x its post-build level for 10 consecutive solves.
        (The KNP hierarchies depend on the mesh, D_k and dt only -- nothing to refresh.)  A partitioned run keeps the hierarchy
        of the initial state (every rank would have to gather kappa to rebuild the replicated levels): the Krylov solves still
        converge to their tolerance, only the iteration count can grow."""
        if self.inp.local_mesh is not None:
            return
        st = self.refresh
        st["solves"] += 1
        if st["ref"] is None and st["solves"] >= 3:
            st["ref"] = max(1, min(emi_niter[-2:]))
        stale = False
        if st["ref"] is not None:
            st["high"] = st["high"] + 1 if emi_niter[-1] > 3 * st["ref"] + 2 else 0
            stale = st["high"] >= 10
        if st["solves"] % int(os.environ.get("KNP_AMG_REFRESH_EVERY", 50)) == 0:
            kap, k0 = dev.download(_abi.F_KAPPA), self.kappa0
            lim = float(os.environ.get("KNP_AMG_REFRESH_KAPPA", 0.25))
            floor = 1e-12 * max(float(np.abs(k0).max()), 1e-300)                # a zero entry of kappa must not force a rebuild
            drift = np.abs(kap - k0) / np.maximum(np.abs(k0), floor)
            stale = stale or bool(np.nanmax(drift) > lim) or not bool(np.isfinite(kap).all())
        if stale:
            if self.inp.verbose:
                print(" AMG(EMI): hierarchy refreshed (kappa drift / iteration count)")
            self.setup_emi(dev)
            self.refreshes += 1
            self.refresh = {"solves": 0, "ref": None, "high": 0}

    # ------------------------------------------------------------------ KNP
    def _knp_level0_degree(self):
        # one Jacobi step on the finest conforming level, on one GPU and on partitions alike.  (With a communicator the hierarchy is
        # replicated and the restricted residual is all-reduced; a transfer-only finest level would let that happen on level 1 --
        # 6.5x fewer bytes, no replicated level-0 SpMVs -- but costs 50 % more BiCGStab iterations: 9.9 instead of 6.6 per step in
        # a 4-rank run of the r=2 mesh, which only pays for itself beyond 8 ranks.)
        return 1

    def _build_knp(self):
        """[(members, levels)] of the KNP preconditioner (amg.build_knp_groups), built in this process."""
        from knpemidg import amg
        p = self.inp
        gmesh, gsub, gsurf = self._amg_global()
        return amg.build_knp_groups(self.cspace, self.cspace2 if p.degree != 1 else None, gsub.array(),
                                    [ion['D_sub'] for ion in p.ion_list[:-1]], p.dt, self._knp_level0_degree())

    def upload_knp_if_ready(self, dev):
        """The KNP helper usually finishes first (no membrane term, one hierarchy for both species): while the EMI helper is still
        running, its result is uploaded ahead of setup_emi instead of in setup_knp (0.2 s of upload hidden behind the wait)."""
        eh, kh = self.emi_helper, self.knp_helper
        if eh is not None and kh is not None and eh[0]["thread"].is_alive() and not kh[0]["thread"].is_alive():
            self._upload_knp(dev)
            self.knp_uploaded_early = True

    def setup_knp(self, dev):
        early, self.knp_uploaded_early = self.knp_uploaded_early, False
        if not early:
            self._upload_knp(dev)

    def _upload_knp(self, dev):
        ts = time.perf_counter()
        p = self.inp
        groups = None
        helper, self.knp_helper = self.knp_helper, None
        if helper is not None:
            from knpemidg import setup_worker
            handle, d0 = helper
            if d0 == self._knp_level0_degree():
                groups = setup_worker.collect(handle)
            else:                                   # the helper was started with another guess of the communicator state
                setup_worker.cancel(handle)
        if groups is None:
            groups = self._build_knp()
        d0 = self._dist0(dev)
        for members, levels in groups:
            local = None
            if d0 is not None:                      # partitioned run: this rank's rows of the finest conforming level
                local = d0.localize(levels)
            if local is not None:
                dev.amg_upload(1 + members[0], d0.local_dg2cg(p.local_mesh.cells_global), local, ncol=len(members), dist0=True)
                self.dist0_uploads += 1
            else:
                dev.amg_upload(1 + members[0], self._local_dg2cg(), levels, ncol=len(members))
            for k in members[1:]:
                dev.amg_clear(1 + k)
            if p.verbose:
                print(" AMG(KNP %s) levels:" % "+".join(p.ion_list[k]['name'] for k in members), [lv.A.shape[0] for lv in levels])
        self.setup_seconds += time.perf_counter() - ts
