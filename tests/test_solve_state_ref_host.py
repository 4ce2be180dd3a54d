"""CPU evidence that the host model of the solve-to-solve state (tests/solve_state_ref.py) and the comparisons of
tests/test_gpu_solve_state.py can tell a broken rule from the one solve.hip writes -- on the reference alone, for the sequences the device
runs.  A device that followed the rules is stood in for by the unbroken model (guesses, histories, counters) and the oracle's inverses
rounded to fp32 (blocks); each broken rule (solve_state_ref.MUTATIONS) must then give a prediction that differs to the bit (guesses,
histories, counters) or lies far from the right one: blocks and spectral bounds by >= 1e3 comparison bounds, the iterate x_1 by >= 1e6
bounds of amg_ref.bound, whose 1e-9 cap on ill-conditioned cases holds for every solve of the sequences.
No GPU is needed, but knpemidg.amg builds its hierarchies with the host routines of the built library (as tests/test_host.py does)."""
import numpy as np
import pytest

import amg_ref as ar
import solve_state_ref as ss
import solve_state_cases as T

_BOX = {}


def _box(mesh):
    if mesh not in _BOX:
        _BOX[mesh] = T.Boxes(mesh)
    return _BOX[mesh]


# ---- the Gauss-Jordan inverse and the block bound ------------------------------------------------------------------------------------
def test_gauss_jordan_inverse_is_an_inverse_in_extended_precision():
    rng = np.random.default_rng(3)
    B = rng.standard_normal((40, 6, 6))
    B[0] = np.diag([1e-8, 1.0, 1e8, 1.0, 1.0, 1.0]) + 1e-9 * B[0]       # pivoting and scales
    B[1][[0, 1]] = B[1][[1, 0]] * np.array([[1e-12], [1.0]])
    inv = ss.gauss_jordan_inverse(B)
    assert inv.dtype == np.longdouble
    I = np.einsum("bij,bjk->bik", B.astype(np.longdouble), inv)
    cond = np.linalg.cond(B)
    assert (np.abs(I - np.eye(6)).max(axis=(1, 2)) <= 1e-18 * cond + 1e-18).all()
    assert (np.abs(np.linalg.inv(B) - inv).max(axis=(1, 2)) <= 1e-15 * cond * np.abs(inv).max(axis=(1, 2))).all()


def test_lambda_max_is_the_replica_of_amg_ref():
    B = _box("box_P1")
    h = B.hosts[0]
    for As, Bi, bs in (([h.ref.A_emi], [h.ref.binv_emi], [h.ref.b_emi]), h.knp()):
        a, b = ar.bj_lambda_max(As, Bi, bs), ss.lambda_max(As, Bi, bs)
        assert abs(a - b) <= 1e-14 * a and abs(float(ss.lambda_max(As, Bi, bs, np.longdouble)) - a) <= 1e-12 * a


# ---- a. the recorded sequence ----------------------------------------------------------------------------------------------------------
def _fake_rec(pb, states, ops, model):
    """what a device that follows `model` would leave behind T.run_ops: the guesses and histories of the model, the oracle's inverses
    of the state it names rounded to fp32, its counters, a bound wherever it has one"""
    ns, cur, coef, rec, blocks = pb.N_ions, {}, None, [], {}
    for op in ops:
        if op[0] == "state":
            coef = op[1]
            cur["C"], cur["PHI"] = states[coef][0].ravel(), states[coef][2].ravel()
        elif op[0] == "upload":
            model.upload(op[1])
            if op[1] != "C_ELIM":
                cur[op[1]] = T.values_of(pb, op[1], op[2])
        elif op[0] == "put":
            cur[op[1]] = T.values_of(pb, op[1], op[2])
        elif op[0] == "set_params":
            model.set_params()
        else:
            for s, key in (("emi", "PHI"), ("knp", "C")):
                plan = model.solve(s, cur[key], coef, cheb=(s == "knp"), keep_h2=not op[1])
                model.done(s, False, 0)
                S = model.sys(s)
                cur[key] = plan["guess"]
                if (s, plan["blocks"]) not in blocks:
                    blocks[s, plan["blocks"]] = T.oracle_blocks(pb, s, states[plan["blocks"]])[0].astype(np.float32)
                z = np.zeros_like(plan["guess"])
                rec.append(dict(x=plan["guess"], hist=np.stack([z if S.h1 is None else S.h1, z if S.h2 is None else S.h2]),
                                binv=blocks[s, plan["blocks"]], n_lmax=0.0 if S.lmax is None or s == "emi" else 2.0,
                                **{"n_" + k: v for k, v in S.counters().items()}))
    return rec


_GUESS_MUTATIONS = {"guess_is_previous": "guess", "guess_3x_2h1": "guess", "h1_not_rotated": "guess", "history_kept_by_upload": "guess",
                    "history_dropped_by_set_params": "guess", "lag_7": None, "lag_9": None, "rebuild_every_solve": "blocks",
                    "age_kept_by_upload": "counters", "bound_every_solve": "counters"}


@pytest.mark.parametrize("env", ({},) + T.ENVIRONMENTS, ids=lambda e: "-".join("%s=%s" % kv for kv in e.items()) or "default")
def test_recorded_sequence_tells_the_broken_rules(env):
    """GUESS_OPS on the P1 box under every environment the device runs it with: the check of the GPU test passes on the model's own
    output and fails, naming the kind of difference, with each broken rule the sequence reaches under that environment (nine solves
    with resets between them: lags 7 and 9 are out of its reach -- the 18-solve sequences below have them)"""
    pb, volt = T.problem("box_P1")
    states = T.coefficient_states(pb, volt)
    rec = _fake_rec(pb, states, T.GUESS_OPS, ss.Model.from_env(env, table=True))
    assert len(rec) == 18
    keep = {}
    T.check_ops("true", pb, states, T.GUESS_OPS, rec, ss.Model.from_env(env, table=True), keep)
    for mut, kind in _GUESS_MUTATIONS.items():
        if kind is None:
            continue
        if kind == "guess" and env.get("KNP_EXTRAPOLATE") == "0":
            continue                                                    # no extrapolation at all: nothing of it to break
        if mut == "rebuild_every_solve" and "KNP_BJ_LAG" in env:
            continue                                                    # (the broken lags stand for the default of 8)
        with pytest.raises(AssertionError) as e:
            T.check_ops("broken", pb, states, T.GUESS_OPS, rec, ss.Model.from_env(env, table=True, mut=mut), keep)
        assert "'%s" % kind in str(e.value), (mut, kind, str(e.value)[:400])
    # the guesses the broken rules give are other bits in thousands of entries, not one
    if not env:
        wrong = _fake_rec(pb, states, T.GUESS_OPS, ss.Model(table=True, mut="guess_3x_2h1"))
        assert max(np.count_nonzero(a["x"] != b["x"]) for a, b in zip(rec, wrong)) >= pb.ndof // 2


def test_recorded_file_round_trip(tmp_path):
    pb, volt = T.problem("two_cell_3")
    states = T.coefficient_states(pb, volt)
    rec = _fake_rec(pb, states, T.GUESS_OPS, ss.Model())
    T.save_rec(str(tmp_path / "r.npz"), rec)
    T.check_ops("file", pb, states, T.GUESS_OPS, T.load_rec(str(tmp_path / "r.npz")), ss.Model())


def test_order_2_bound_tells_the_linear_guess():
    """3 (x - h1) + h2 against 2 x - h1 on the sequence's values: the bound of 2 ulp separates them in nearly every entry"""
    pb, _ = T.problem("box_P1")
    x, h1, h2 = (T.values_of(pb, "PHI", k) for k in (2, 1, 0))
    bd = ss.order2_bound(x, h1, h2)
    d = x - h1
    fused = (np.longdouble(3.0) * d.astype(np.longdouble) + h2.astype(np.longdouble)).astype(np.float64)      # fma(3, x - h1, h2)
    assert (np.abs(3.0 * d + h2 - fused) <= bd).all() and np.count_nonzero(3.0 * d + h2 != fused) > 0
    assert np.count_nonzero(np.abs(3.0 * (x - h1) + h2 - (2.0 * x - h1)) > 1e3 * bd) >= 0.99 * x.size


# ---- b. / c. the chains of one-iteration solves ------------------------------------------------------------------------------------------
def _chain(B, system, nsolves, events, hierarchy, state_of, mut=None, feed=None, iterates=True, only=None):
    """the host side of T.chain with the replica's own x_1 in the device's place (feed: the x_prev of another run instead).  Per solve:
    x_prev, the plan, the counters, the numeric bound in use and its comparison bound, x_1 in float64 (only: of that solve alone) and the bound of amg_ref.bound"""
    events = events or {}
    knp = system == "knp"
    cheb = knp or hierarchy
    levels = B.levels(knp) if hierarchy else None
    model = ss.Model(table=True, mut=mut)
    if hierarchy and not knp:
        model.set_emi_dg_smoother(True)
    model.upload("PHI")
    model.upload("C")
    x = (B.pb.c if knp else B.pb.phi).ravel()
    out, lams = [], {}
    for j in range(nsolves):
        ev = events.get(j)
        i = state_of(j)
        if ev == "set_params":
            model.set_params()
        b = np.stack(B.hosts[i].knp()[2]) if knp else B.hosts[i].ref.b_emi
        if ev == "upload C_ELIM":
            model.upload("C_ELIM")
        if feed is not None:
            x = feed[j]["x_prev"]
        plan = model.solve(system, x, i, b=j, cheb=cheb)
        model.done(system, False, 1)
        if cheb and plan["estimate"]:
            lams[j] = B.lam(system, plan["lmax"], b)
        lmax, lbd, lhp = lams[plan["lmax"]["b"]] if cheb else (None, None, None)
        r = dict(x_prev=x, i=i, b=b, plan=plan, counters=model.sys(system).counters(), lmax=lmax, lbd=lbd)
        if iterates and only in (None, j):
            r["x64"] = B.x1(system, i, plan["guess"], plan["blocks"], lmax, b, levels, cheb, np.float64)
            if mut is None:
                xhp = B.x1(system, i, plan["guess"], plan["blocks"], lhp, b, levels, cheb, ar.hp_dtype())
                r["bound"] = [ar.bound(a, h) for a, h in zip(r["x64"], xhp)]          # (asserts the 1e-9 cap)
            x = r["x64"].ravel()
        out.append(r)
    return out


def _apart(B, system, true, wrong):
    """the first solve where the broken rule's prediction differs: (solve, counters differ, blocks apart in block bounds, bound apart
    in its bounds, x_1 apart in its bounds) -- 0.0 where that part agrees"""
    for j, (t, w) in enumerate(zip(true, wrong)):
        tp, wp = t["plan"], w["plan"]
        cnt = t["counters"] != w["counters"]
        blk = lam = it = 0.0
        if tp["blocks"] != wp["blocks"]:
            (a, bd, _), (b, _, _) = B.blocks(system, tp["blocks"]), B.blocks(system, wp["blocks"])
            blk = float((np.abs(a - b).max(axis=(2, 3)) / bd).max())
        if t["lmax"] is not None and t["lmax"] != w["lmax"]:
            lam = abs(t["lmax"] - w["lmax"]) / t["lbd"]
        guess = not np.array_equal(tp["guess"], wp["guess"])
        if "x64" in t and "x64" in w:
            it = min(float(np.abs(a - b).max() / bd) for a, b, bd in zip(t["x64"], w["x64"], t["bound"]))
        if cnt or blk or lam or it or guess:
            return j, cnt, blk, lam, it
    return None


def _apart_with_iterate(B, system, true, args, mut):
    """_apart, with x_1 of the broken rule computed at the first solve where its prediction differs"""
    d = _apart(B, system, true, _chain(B, system, *args, mut=mut, feed=true, iterates=False))
    if d is None:
        return None
    j = d[0]
    wrong = _chain(B, system, j + 1, *args[1:], mut=mut, feed=true, only=j)
    return (j,) + _apart(B, system, true[j:j + 1], wrong[j:])[1:]


_SEQ = lambda j: ss.LAG_STATES[j]


@pytest.mark.parametrize("system", ["emi", "knp"])
@pytest.mark.parametrize("mesh", ["box_P1", "box_P2"])
def test_lagged_sequences_tell_the_broken_rules(mesh, system):
    """the 18 solves of test_lagged_inverses_over_18_solves, plain and with the events: every solve has its bound under the 1e-9 cap,
    the states are pairwise >= 1e3 block bounds apart in every system's blocks, and each broken rule of the lag, the resets, the guess
    and (KNP: the solve carries the bound) the bound is caught at the solve where it first matters"""
    B = _box(mesh)
    assert len(ss.LAG_STATES) == 18 and all(a != b for a, b in zip(ss.LAG_STATES, ss.LAG_STATES[1:]))
    for i in range(4):
        for k in range(i):
            (a, bd, _), (b, _, _) = B.blocks(system, i), B.blocks(system, k)
            assert (np.abs(a - b).max(axis=(2, 3)) / bd).max(axis=1).min() >= 1e3, (i, k)
    hier = system == "knp"
    seen = set()
    for events in (None, ss.LAG_EVENTS):
        true = _chain(B, system, 18, events, hier, _SEQ)
        built = [j for j, r in enumerate(true) if r["plan"]["rebuilt"]]
        assert built == ([0, 8, 16] if events is None else [0, 8, 11, 14]), built
        muts = ["guess_is_previous", "guess_3x_2h1", "h1_not_rotated", "lag_7", "lag_9", "rebuild_every_solve"]
        muts += ["age_kept_by_upload", "history_dropped_by_set_params"] if events else []
        muts += ["bound_without_1.1", "bound_every_solve"] if hier else []
        for mut in muts:
            d = _apart_with_iterate(B, system, true, (18, events, hier, _SEQ), mut)
            assert d is not None, mut
            j, cnt, blk, lam, it = d
            print("SOLSTATE-HOST %s %s %-30s solve %2d counters %d blocks %.2e bound %.2e x_1 %.2e" % (mesh, system, mut, j, cnt, blk, lam, it))
            assert it >= 1e6, (mut, d)
            if mut in ("lag_7", "lag_9", "rebuild_every_solve", "age_kept_by_upload"):
                assert blk >= 1e3 and j == {"lag_7": 7, "lag_9": 8, "rebuild_every_solve": 1, "age_kept_by_upload": 14}[mut], (mut, d)
            if mut.startswith("bound"):
                assert lam >= 1e3, (mut, d)
            seen.add(mut)
    assert len(seen) == (10 if hier else 8)


def test_emi_bound_sequence_tells_the_broken_rules():
    """test_emi_bound_is_kept_across_the_rebuild_at_solve_8: EMI with a hierarchy and the Chebyshev cell-block smoother"""
    for mesh in ("box_P1", "box_P2"):
        B = _box(mesh)
        true = _chain(B, "emi", 10, None, True, _SEQ)
        assert [r["plan"]["estimate"] for r in true] == [True] + [False] * 9 and true[8]["plan"]["rebuilt"]
        for mut in ("bound_without_1.1", "bound_every_solve"):
            j, cnt, blk, lam, it = _apart_with_iterate(B, "emi", true, (10, None, True, _SEQ), mut)
            print("SOLSTATE-HOST %s emi cheb %-20s solve %d bound %.2e x_1 %.2e" % (mesh, mut, j, lam, it))
            assert lam >= 1e3 and it >= 1e6, (mesh, mut, lam, it)
        # test_emi_bound_is_re_estimated_after_a_reset_in_mid_sequence: estimates at 0, 11, 14, every bound under the cap, and a reset
        # that forgets the bound (the broken rule drops the age alone, so here: the bound kept at 14 by lag and estimate) is told
        true = _chain(B, "emi", 16, ss.LAG_EVENTS, True, _SEQ)
        assert [j for j, r in enumerate(true) if r["plan"]["estimate"]] == [0, 11, 14]
        assert true[14]["lmax"] != true[13]["lmax"]                     # (solve 11 is at state 0 again: its estimate is that of solve 0)
        j, cnt, blk, lam, it = _apart_with_iterate(B, "emi", true, (16, ss.LAG_EVENTS, True, _SEQ), "age_kept_by_upload")
        assert j == 14 and blk >= 1e3 and lam >= 1e3 and it >= 1e6, (mesh, j, blk, lam, it)


@pytest.mark.parametrize("system", ["emi", "knp"])
def test_age_64_is_told(system):
    """66 solves over three states: the estimate at solve 64 (state 1, rebuilt blocks) is >= 1e3 bounds from the kept one of solve 0"""
    B = _box("box_P1")
    seq = lambda j: j % 3
    true = _chain(B, system, 66, None, True, seq, iterates=False)
    assert [j for j, r in enumerate(true) if r["plan"]["estimate"]] == [0, 64]
    assert true[63]["counters"]["lmax_age"] == 63 and true[64]["counters"]["lmax_age"] == 0 and true[65]["counters"]["lmax_age"] == 1
    j, cnt, blk, lam, it = _apart(B, system, true, _chain(B, system, 66, None, True, seq, mut="bound_never_at_64", feed=true, iterates=False))
    print("SOLSTATE-HOST box_P1 %s bound_never_at_64: solve %d bound %.2e" % (system, j, lam))
    assert j == 64 and cnt and lam >= 1e3


def test_jump_rule_boundary_is_told():
    """it_ref = n0 from a converged solve, last_it = k from the next: for even n0 the count k = (3 n0 + 2) / 2 keeps the bound by the
    rule and re-estimates it with >= in place of > (the counters differ; the re-estimate on the same matrix, blocks and b gives the
    same value); k + 1 re-estimates by both; odd n0 has no count on the boundary"""
    def run(mut, n0, k):
        m = ss.Model(mut=mut)
        m.upload("C")
        x = np.zeros(4)
        assert m.solve("knp", x, 0, b=0)["estimate"]
        m.done("knp", True, n0)
        assert m.knp.it_ref == n0
        m.solve("knp", x, 0, b=1)
        m.done("knp", False, k)
        return m.solve("knp", x, 0, b=2)["estimate"], m.knp.counters()
    for n0 in (2, 4, 6):
        k = (3 * n0 + 2) // 2
        assert run(None, n0, k)[0] is False and run("jump_rule_ge", n0, k)[0] is True
        assert run(None, n0, k)[1] != run("jump_rule_ge", n0, k)[1]
        assert run(None, n0, k + 1)[0] is True and run(None, n0, k - 1)[0] is False
    for n0 in (1, 3, 5):
        k = (3 * n0 + 2) // 2
        assert run(None, n0, k)[0] is False and run(None, n0, k + 1)[0] is True
    # a solve that did not converge leaves it_ref at -1: no jump, however many iterations
    m = ss.Model()
    m.upload("C")
    m.solve("knp", np.zeros(4), 0, b=0)
    m.done("knp", False, 1)
    m.solve("knp", np.zeros(4), 0, b=1)
    m.done("knp", False, 50)
    assert not m.solve("knp", np.zeros(4), 0, b=2)["estimate"] and m.knp.it_ref == -1


def test_every_listed_broken_rule_is_covered():
    covered = set(_GUESS_MUTATIONS) | {"bound_without_1.1", "bound_never_at_64", "jump_rule_ge"}
    assert covered == set(ss.MUTATIONS)
