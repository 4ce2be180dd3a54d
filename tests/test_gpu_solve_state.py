"""What one linear solve hands the next (csrc/solve.hip: PrecState, Fields; csrc/context.hip: knp_upload, knp_set_params) against the host
model tests/solve_state_ref.py, and the two glue kernels of the Picard loop against numpy / the oracle.

Everything is observed through what the library already offers: Device.state_save() cut by checkpoint.split_snapshot (blocks 8 / 9 the
histories, 10 / 11 the lagged cell-block inverses, 12 the counters, 13 the reals), and solves with maxit = 0, which return the initial
guess itself (pcg_impl, bicgstab_impl and gmres_impl leave x alone and report status -3, "did not converge").  State changes ON THE
DEVICE, as a time step changes it: through a same-sized field whose upload has no side effect, then copy_field.

  a. guesses        the recorded sequence GUESS_OPS on every mesh: the field after an upload of U is U, then 2 Y_j - Y_(j-1) bitwise,
                    h1 / h2 / nh as the model says, with KNP_FUSE_EXTRAP=0 at one call, across uploads of C, PHI, C_ELIM and set_params;
                    1, 2 and 4 solved species; PCG, BiCGStab and GMRES; in child processes (tests/solve_state_worker.py) the switches
                    read once per process.  Order 2: within 2 ulp of the largest of the three terms.
  b. lagged blocks  the cell-block inverses of the snapshot against the inverses of the oracle's cell-diagonal blocks at the state the
                    model names, in the same recorded sequences (every mesh) and over 18 one-iteration solves on the two boxes, with and
                    without a set_params / an upload in mid-sequence; there x_1 is compared with the replica run from the model's guess
                    with the lagged blocks and the kept bound (float64 and extended precision each with its own).  Bound per block: 2^-23 max|B^-1| + 32 max|inv64 - inv_longdouble|.
                    The replica's fp32 blocks are rounded from the long-double inverse: numpy's float64 inverse rounds one entry of
                    the 64800 of the P2 box's KNP blocks the other way, and x_1 with that block is 95 / 809 bounds from the device's.
  c. spectral bound lmax of the snapshot against 1.1 lambda of the replica's power iteration, bound 32 |lam64 - lam_hp| (at least
                    1e-13 lam); the same bits while the model says "kept"; re-estimated after reset_lagged (EMI and KNP, in mid-sequence), at the 64th solve behind an
                    estimate, and by the iteration-jump rule on either side of 2 n > 3 it_ref + 2.
  d. glue kernels   max_abs_diff against numpy over the owned dofs; picard_updates and nernst against the oracle.

Every context is created for its test.  The cases, the recorded sequence and its check live in tests/solve_state_cases.py.
Every bound comes from the reference alone (tests/test_solve_state_ref_host.py shows what each one tells apart).  Measured on the
MI355X, worst device error / bound per group (SOLSTATE lines; DESIGN.md section 2, "Solve-to-solve state")."""
import copy
import os
import subprocess
import sys

import numpy as np
import pytest

import amg_ref as ar
import knpemi_oracle as ko
import solve_state_ref as ss
from common import device_for, push_state, set_params_of, relerr
from solve_state_cases import (ENVIRONMENTS, GUESS_OPS, SB_BINV, SB_HIST, SHORT_OPS, TABLE, Boxes, check_ops, coefficient_states, fail_solve,
                               load_rec, note, oracle_blocks, problem, put, run_ops, snapshot, values_of, wide_values, worst)

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))

GUESS_MESHES = ("box_P1", "box_P2", "2D_P1", "2D_P2", "two_cell_2", "two_cell_3", "box_533", "emix")


def _guess_case(mesh, ops, monkeypatch=None, method="bicgstab", env=None):
    pb, volt = problem(mesh)
    states = coefficient_states(pb, volt)
    dev = device_for(pb)
    try:
        push_state(dev, pb)
        rec = run_ops(dev, pb, states, ops, method)
        variant = (dev.apply_variant(0), dev.apply_variant(1))
    finally:
        dev.close()
    check_ops("%s %s" % (mesh, method), pb, states, ops, rec, ss.Model.from_env(env or {}, table=mesh in TABLE))
    return variant


@pytest.mark.parametrize("mesh", GUESS_MESHES)
def test_guesses_histories_and_lagged_blocks_follow_the_model(hip_lib, mesh):
    """GUESS_OPS with BiCGStab: 1 (two_cell_2), 2 and 4 (box_533) solved species; 8 dofs (less than a wave) to 3240 on the idealized
    meshes, and the piece of the EMIx reconstruction with its sliver cells"""
    _guess_case(mesh, GUESS_OPS)


def test_guesses_with_gmres(hip_lib):
    _guess_case("box_P1", GUESS_OPS, method="gmres")


def test_blocks_of_a_fresh_context_with_assembled_p2_blocks(hip_lib, monkeypatch):
    """the first solves of a context on the P2 box with the assembled cell blocks (k_tab_block_inverse, apply variant 9; the switch is
    read when the context is created)"""
    monkeypatch.setenv("KNP_P2_ASSEMBLED", "1")
    assert _guess_case("box_P2", SHORT_OPS) == (9, 9)


def test_block_layout_is_row_major(hip_lib):
    """on KNP blocks with drift, far from symmetric: the snapshot's [nd * nd] is the row-major inverse, as krylov_ref.block_inverses
    has it -- the transposed reading is >= 1e3 bounds away"""
    import krylov_ref as kr
    pb, volt = problem("box_P1")
    states = coefficient_states(pb, volt)
    inv, bd = oracle_blocks(pb, "knp", states[0])
    assert (np.abs(inv - inv.transpose(0, 1, 3, 2)).max(axis=(2, 3)) / bd).max() >= 1e3
    A0 = ko.assemble_knp(pb, 0).tocsr()
    assert np.abs(kr.block_inverses(A0, pb.nd) - inv[0]).max() <= 1e-6 * np.abs(inv[0]).max()
    dev = device_for(pb)
    try:
        push_state(dev, pb)
        rec = run_ops(dev, pb, states, SHORT_OPS)
    finally:
        dev.close()
    got = np.asarray(rec[1]["binv"], dtype=np.float64).reshape(inv.shape)
    assert (np.abs(got - inv).max(axis=(2, 3)) / bd).max() <= 1.0
    assert (np.abs(got.transpose(0, 1, 3, 2) - inv).max(axis=(2, 3)) / bd).max() >= 1e3


def test_mms_mode_starts_from_the_field_itself(hip_lib):
    """splitting = 2 (manufactured-solution mode, reachable through set_mms + set_params): no extrapolation, no history"""
    from knpemidg import _abi as A
    pb, _ = problem("box_533")
    dev = device_for(pb)
    try:
        push_state(dev, pb)
        nc, nd, ns = pb.mesh.num_cells(), pb.nd, pb.N_ions
        dev.set_mms(np.ones((ns, nc)), np.zeros((nc, nd)), np.zeros((ns, nc, nd)))
        pb2 = copy.copy(pb)
        pb2.splitting = 2
        set_params_of(dev, pb2)
        dev.update_kappa()
        dev.update_dnphi()
        for k in range(3):
            U, V = values_of(pb, "PHI", 20 + k), values_of(pb, "C", 20 + k)
            if k == 0:
                dev.upload(A.F_PHI, U)
                dev.upload(A.F_C, V)
            else:
                put(dev, A.F_PHI, U)
                put(dev, A.F_C, V)
            assert np.array_equal(fail_solve(dev, "emi", 0), U) and np.array_equal(fail_solve(dev, "knp", 0), V), k
        sn = snapshot(dev)
        assert sn["emi"]["nh"] == 0 and sn["knp"]["nh"] == 0 and not sn[SB_HIST["emi"]].any() and not sn[SB_HIST["knp"]].any()
    finally:
        dev.close()


@pytest.mark.parametrize("env", ENVIRONMENTS, ids=lambda e: "-".join("%s=%s" % kv for kv in e.items()))
def test_guesses_and_lag_under_the_process_wide_switches(hip_lib, tmp_path, env):
    out = str(tmp_path / "rec.npz")
    clean = {k: v for k, v in os.environ.items() if not k.startswith(("KNP_EXTRAPOLATE", "KNP_BJ_LAG", "KNP_FUSE_EXTRAP"))}
    run = subprocess.run([sys.executable, os.path.join(HERE, "solve_state_worker.py"), "box_P1", out], env=dict(clean, **env),
                         stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert run.returncode == 0, run.stdout[-3000:]                      # (a signal or the time limit ends the test here)
    pb, volt = problem("box_P1")
    check_ops("box_P1 %s" % env, pb, coefficient_states(pb, volt), GUESS_OPS, load_rec(out), ss.Model.from_env(env, table=True))


# ---- b. / c. 18 one-iteration solves: lagged inverses, counters, the kept bound, x_1 ----------------------------------------------------
@pytest.fixture(scope="module", autouse=True)
def _close_boxes():
    yield
    print("SOLSTATE summary: " + "; ".join("%s %.3g" % kv for kv in sorted(worst.items())))


def chain(B, system, nsolves, events=None, hierarchy=True, iterates=True, state_of=None, tag=""):
    """`_chain` on a fresh context of the box"""
    with B.device():
        return _chain(B, system, nsolves, events, hierarchy, iterates, state_of, tag)


def _chain(B, system, nsolves, events, hierarchy, iterates, state_of, tag):
    """nsolves one-iteration solves of `system` on the box B, the coefficients changing on the device before every one; after every
    solve the snapshot against the model and the oracle, x_1 against the replica from the model's guess (fed the device's previous
    iterate), the spectral bound against the replica's where the model says "estimated", its bits where it says "kept"."""
    A, dev, ns = B.A, B.dev, (1 if system == "emi" else B.ns)
    events = events or {}
    state_of = state_of or (lambda j: ss.LAG_STATES[j])
    knp = system == "knp"
    cheb = knp or hierarchy
    levels = B.levels(knp) if hierarchy else None
    model = ss.Model(table=True)
    group = "%s %s%s" % (B.mesh, system, tag)
    if hierarchy:
        if knp:
            dev.amg_upload(1, B.host.dg2cg, levels, ncol=ns)
        else:
            dev.amg_upload(0, B.host.dg2cg, levels)
            dev.set_emi_dg_smoother(True)
            model.set_emi_dg_smoother(True)
    bad, lams, last_lmax = [], {}, None
    try:
        dev.upload(A.F_PHI, B.pb.phi)                                   # both uploads: the context starts like a fresh one
        dev.upload(A.F_C, B.pb.c)
        model.upload("PHI")
        model.upload("C")
        for j in range(nsolves):
            ev = events.get(j)
            i = state_of(j)
            if ev == "set_params":
                set_params_of(dev, B.pb)
                model.set_params()
            b = B.to_state(system, i)
            if ev == "upload C_ELIM":                                   # (the value the field holds: only the side effects count)
                dev.upload(A.F_C_ELIM, dev.download(A.F_C_ELIM))
                model.upload("C_ELIM")
            x_prev = dev.download(A.F_PHI if not knp else A.F_C)
            plan = model.solve(system, x_prev, i, b=j, cheb=cheb)
            x1 = fail_solve(dev, system, 1)
            model.done(system, False, 1)
            sn, S = snapshot(dev), model.sys(system)
            names = ("nh", "age", "lmax_age", "it_ref") if cheb else ("nh", "age")     # (without the smoother nothing touches the other two)
            got, want = {k: sn[system][k] for k in names}, {k: S.counters()[k] for k in names}
            if got != want:
                bad.append((j, "counters", got, want))
            inv, bd, b32 = B.blocks(system, plan["blocks"])
            e = np.abs(np.asarray(sn[SB_BINV[system]], dtype=np.float64).reshape(inv.shape) - inv).max(axis=(2, 3)) / bd
            note("lagged blocks %s" % group, e.max())
            if not e.max() <= 1.0:
                bad.append((j, "blocks of state %s" % plan["blocks"], float(e.max())))
            hist = sn[SB_HIST[system]].reshape(2, -1)
            if not (np.array_equal(hist[0], S.h1) and np.array_equal(hist[1], S.h2)):
                bad.append((j, "history"))
            lmax = None
            if cheb:
                if plan["estimate"]:
                    lams[j] = B.lam(system, plan["lmax"], b)
                    e = abs(sn[system]["lmax"] - lams[j][0]) / lams[j][1]
                    note("spectral bound %s" % group, e)
                    if not e <= 1.0:
                        bad.append((j, "bound", sn[system]["lmax"], lams[j]))
                elif sn[system]["lmax"] != last_lmax:
                    bad.append((j, "kept bound changed its bits", sn[system]["lmax"], last_lmax))
                last_lmax = sn[system]["lmax"]
                lmax = lams[plan["lmax"]["b"]]
            elif sn[system]["lmax"] != 0.0:
                bad.append((j, "a bound without the smoother", sn[system]["lmax"]))
            if iterates:
                # (each run with the bound of its own precision: where the power iteration is sensitive, so is x_1)
                x64, xhp = (B.x1(system, i, plan["guess"], plan["blocks"], lmax and lmax[k], b, levels, cheb, dt)
                            for k, dt in ((0, np.float64), (2, ar.hp_dtype())))
                for s in range(ns):
                    bnd = ar.bound(x64[s], xhp[s])
                    e = np.abs(x1.reshape(ns, -1)[s] - x64[s]).max() / bnd
                    note("x_1 %s" % group, e)
                    if not e <= 1.0:
                        bad.append((j, "x_1 species %d" % s, float(e)))
    finally:
        if hierarchy:
            if knp:
                dev.amg_clear(1)
            else:
                dev.set_emi_dg_smoother(None)
                dev.amg_clear(0)
    assert not bad, bad[:6]
    return model


@pytest.mark.parametrize("events", [None, ss.LAG_EVENTS], ids=["plain", "set_params-11-upload-14"])
@pytest.mark.parametrize("system", ["emi", "knp"])
@pytest.mark.parametrize("mesh", ["box_P1", "box_P2"])
def test_lagged_inverses_over_18_solves(hip_lib, mesh, system, events):
    """EMI on the cell blocks alone (no hierarchy, no bound), KNP with the hierarchy `bands` and the kept bound at the synthetic
    Peclet number 5.4 (the per-cell set); rebuilds at solves 0, 8, 16 -- and 11, 14 with the events"""
    B = Boxes.get(mesh)
    assert B.host.peclet() > 0.5
    chain(B, system, 18, events, hierarchy=(system == "knp"), tag=" events" if events else "")


@pytest.mark.parametrize("mesh", ["box_P1", "box_P2"])
def test_emi_bound_is_kept_across_the_rebuild_at_solve_8(hip_lib, mesh):
    """with a hierarchy and the Chebyshev cell-block smoother: lmax of the first solve, the same bits to solve 9, x_1 with it"""
    chain(Boxes.get(mesh), "emi", 10, hierarchy=True, tag=" cheb")


@pytest.mark.parametrize("mesh", ["box_P1", "box_P2"])
def test_emi_bound_is_re_estimated_after_a_reset_in_mid_sequence(hip_lib, mesh):
    """the same with the set_params at solve 11 and the upload of C_ELIM at solve 14: estimates at 0, 11 and 14, kept between"""
    model = chain(Boxes.get(mesh), "emi", 16, ss.LAG_EVENTS, hierarchy=True, tag=" cheb events")
    assert model.emi.lmax["b"] == 14 and model.emi.lmax_age == 1


@pytest.mark.parametrize("system", ["emi", "knp"])
def test_bound_is_re_estimated_at_the_64th_solve_behind_an_estimate(hip_lib, system):
    """66 one-iteration solves over three coefficient states: lmax_age wraps to 0 at solve 64 and nowhere else"""
    model = chain(Boxes.get("box_P1"), system, 66, hierarchy=True, iterates=False, state_of=lambda j: j % 3, tag=" 66")
    assert model.sys(system).lmax["b"] == 64 and model.sys(system).lmax_age == 1


@pytest.mark.parametrize("system", ["emi", "knp"])
def test_bound_follows_the_iteration_jump_rule(hip_lib, system):
    """a converged solve at a loose tolerance sets it_ref = n0; then last_it = k by a solve of k iterations: the next solve keeps the
    bound for 2 k <= 3 n0 + 2 and re-estimates it for the next k; and a converged solve at a tight tolerance, whichever side its count
    falls on.  The counts are the device's, the decisions and the values the model's."""
    B = Boxes.get("box_P1")
    with B.device():
        _jump_rule(B, system)


def _jump_rule(B, system):
    A, dev, knp = B.A, B.dev, system == "knp"
    ns = B.ns if knp else 1
    if knp:                                                             # the production hierarchies: these solves converge
        groups = B.host.knp_groups()
        assert len(groups) == 1 and list(groups[0][0]) == list(range(ns))
        levels = groups[0][1]
    else:
        levels = B.host.emi_levels()
    model = ss.Model(table=True)
    if knp:
        dev.amg_upload(1, B.host.dg2cg, levels, ncol=ns)
    else:
        dev.amg_upload(0, B.host.dg2cg, levels)
        dev.set_emi_dg_smoother(True)
        model.set_emi_dg_smoother(True)
        dev.emi_residual_target(0.0)
    field = A.F_C if knp else A.F_PHI
    x0 = np.zeros(ns * B.pb.ndof)                                       # (h1 is then zero too: every guess is 0)
    seen = []
    try:
        dev.upload(A.F_PHI, B.pb.phi)
        dev.upload(A.F_C, B.pb.c)
        model.upload("PHI")
        model.upload("C")
        b = B.to_state(system, 0)

        def solve(rtol=None, maxit=None, min_it=0):
            """one solve from x0 (put there on the device) against the model's decision; returns the iteration count"""
            put(dev, field, x0)
            if not knp:
                dev.upload(A.F_B_EMI, b)                                # (the scratch field `put` went through)
            plan = model.solve(system, np.asarray(x0).ravel(), 0, b=len(seen), cheb=True)
            if rtol is None:
                fail_solve(dev, system, maxit)
                n, ok = maxit, False
            elif knp:
                n, ok = max(dev.knp_solve(rtol, maxit=1000, min_it=min_it, check_every=1)[0]), True
            else:
                n, ok = dev.emi_solve(rtol, maxit=1000, check_every=1)[0], True
            model.done(system, ok, n)
            sn = snapshot(dev)[system]
            assert {k: sn[k] for k in ("nh", "age", "lmax_age", "it_ref")} == model.sys(system).counters(), (len(seen), sn)
            if plan["estimate"]:
                l64, bd, _ = B.lam(system, plan["lmax"], b)
                note("spectral bound box_P1 %s jump rule" % system, abs(sn["lmax"] - l64) / bd)
                assert abs(sn["lmax"] - l64) <= bd, (len(seen), sn["lmax"], l64, bd)
            else:
                assert sn["lmax"] == seen[-1][1], "a kept bound changed its bits"
            seen.append((plan["estimate"], sn["lmax"], n))
            return n
        n0 = solve(rtol=1e-2)
        assert seen[-1][0] and n0 >= 1 and model.sys(system).it_ref == n0
        k = (3 * n0 + 2) // 2                                           # the largest count that keeps the bound
        solve(maxit=k)
        solve(maxit=k + 1)                                              # decided by last_it = k: kept
        assert not seen[-1][0]
        solve(maxit=0)                                                  # decided by last_it = k + 1: estimated
        assert seen[-1][0] and model.sys(system).it_ref == -1
        n1 = solve(rtol=1e-2)                                           # converged: the new it_ref
        assert model.sys(system).it_ref == n1
        n2 = solve(rtol=1e-9)                                           # tight: last_it = n2 for the solve behind it
        assert 2 * n2 > 3 * n1 + 2, (n1, n2)                             # (measured: 2 -> 32 iterations EMI, 12 -> 31 KNP)
        solve(maxit=0)
        assert seen[-1][0] and model.sys(system).it_ref == -1          # a converged solve's count forces the estimate too
        print("SOLSTATE jump rule %s: n0 %d, k %d kept / %d estimated; loose %d, tight %d -> estimated" % (system, n0, k, k + 1, n1, n2))
    finally:
        if knp:
            dev.amg_clear(1)
        else:
            dev.set_emi_dg_smoother(None)
            dev.amg_clear(0)


# ---- d. the two glue kernels -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mesh", ["box_P1", "box_P2", "box_533", "box_533_3", "two_cell_2"])
def test_max_abs_diff(hip_lib, mesh):
    """k_max_abs_diff over 1 ... 4 systems: the largest difference in the first and last lane of a wave, of a workgroup, of the field,
    in every system; equal fields give 0.0"""
    from knpemidg import _abi as A
    pb, _ = problem(mesh)
    dev = device_for(pb)
    try:
        ns, ndof = pb.N_ions, pb.ndof
        order = np.asarray(dev.cell_order)
        for nsys, fa, fb in ((1, A.F_PHI, A.F_KAPPA), (ns, A.F_C, A.F_C_PREV)):
            n = nsys * ndof
            a = wide_values(50 + nsys, n)
            dev.upload(fa, a)
            dev.upload(fb, a)
            assert dev.max_abs_diff(fa, fb) == 0.0
            r = np.random.default_rng(60 + nsys)
            base = a + 1e-3 * r.uniform(-1, 1, size=n)
            dev.upload(fb, base)
            assert dev.max_abs_diff(fa, fb) == np.abs(a - base).max()
            for pos in sorted({p for p in (0, 63, 64, 255, 256, ndof - 1) if p < ndof}):
                for s in range(nsys):
                    b = base.copy()
                    # device dof `pos` of system s in the caller's numbering
                    at = s * ndof + int(order[pos // pb.nd]) * pb.nd + pos % pb.nd
                    b[at] = a[at] - 7.0
                    dev.upload(fb, b)
                    got = dev.max_abs_diff(fa, fb)
                    assert got == np.abs(a - b).max() and got == abs(a[at] - b[at]), (nsys, pos, s, got)
    finally:
        dev.close()


def _changed(dev, before, fields):
    return [f for f in fields if not np.array_equal(dev.download(f), before[f])]


@pytest.mark.parametrize("mesh", ["box_P1", "box_P2", "2D_P1"])
def test_picard_updates_and_nernst(hip_lib, mesh):
    """picard_updates: C_ELIM and E from the current C at the tolerances of test_step_updates, PHI_M / C_PREV / PHI / C bitwise as they
    were; nernst alone: E, and nothing else"""
    from knpemidg import _abi as A
    pb, _ = problem(mesh)
    dev = device_for(pb)
    try:
        push_state(dev, pb)
        keep = (A.F_PHI, A.F_C, A.F_C_PREV, A.F_PHI_M, A.F_I_CH)
        before = {f: dev.download(f) for f in keep + (A.F_C_ELIM,)}
        dev.nernst()
        E = dev.download(A.F_E).reshape(len(pb.ions), -1)
        for k in range(len(pb.ions)):
            assert relerr(E[k][pb.mem], ko.nernst(pb, k)) < 1e-12
        assert not _changed(dev, before, keep + (A.F_C_ELIM,))
        dev.upload(A.F_E, np.zeros(E.size))
        dev.picard_updates()
        q = copy.copy(pb)
        assert relerr(dev.download(A.F_C_ELIM), ko.update_c_elim(q)) < 1e-14       # (sets q.c_elim: the Nernst potentials below see it)
        E = dev.download(A.F_E).reshape(len(pb.ions), -1)
        for k in range(len(pb.ions)):
            assert relerr(E[k][pb.mem], ko.nernst(q, k)) < 1e-12
        assert not _changed(dev, before, keep)
    finally:
        dev.close()
