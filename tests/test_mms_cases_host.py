"""CPU tests of what the device tests of the manufactured-solution right-hand sides stand on (tests/mms_cases.py,
tests/test_gpu_mms_rhs.py): the stub MMS object against a hand-written closed form, the seeded inputs against the ways a kernel can
be wrong, the host-integrated data terms (knpemidg.mms_terms.extra_rhs) against the oracle's independent restatement (oracle/mms.py),
and how far the solution-dependent term moves the solution."""
import numpy as np
import pytest

import knpemi_oracle as ko
from common import relerr
import mms_cases as mc


def _stub_rhs(pb, stub):
    pb.mms = stub
    try:
        return np.stack([ko.knp_rhs(pb, k) for k in range(pb.N_ions)])
    finally:
        pb.mms = None


_CASES = {}


def _seeded(name):
    """problem, C and the stub's L_knp on the seeded inputs of the device tests (built once per mesh)"""
    if name not in _CASES:
        pb, volt = mc.problem(name)
        C = mc.seed_inputs(pb, volt)
        _CASES[name] = (pb, C, _stub_rhs(pb, mc.StubMMS(C, *mc.zero_extras(pb))))
    return _CASES[name]


@pytest.mark.parametrize("name", ["box_P1", "2D_neuron_r0"])
def test_stub_matches_the_closed_form(name):
    """P1, 3D (|F| / 12) and 2D (|F| / 6): the stub's quadrature of the jump term is the exact facet mass matrix written by hand.
    Both are exact up to rounding; measured 2e-15 of the max norm."""
    pb, C, b = _seeded(name)
    ref = np.stack([mc.closed_form_jump(pb, C[k]) for k in range(pb.N_ions)])
    assert np.abs(ref).max() > 0
    err = relerr(b, ref)
    print(name, "stub vs closed form", err)
    assert err < 1e-13


@pytest.mark.parametrize("name", ["box_P1", "2D_neuron_r0", "3D_box_P2", "2D_neuron_r1_P2"])
def test_stub_rule_of_degree_2p_is_exact(name):
    """The integrand is of degree 2p on a facet: a rule of degree 2p + 3 gives the same vector (measured: a few 1e-15)."""
    pb, C, b = _seeded(name)
    hi = _stub_rhs(pb, mc.StubMMS(C, *mc.zero_extras(pb), deg=2 * pb.p + 3))
    err = relerr(b, hi)
    print(name, "degree 2p vs 2p + 3", err)
    assert err < 1e-13


@pytest.mark.parametrize("mutation", mc.MUTATIONS)
@pytest.mark.parametrize("name", ["2D_neuron_r0", "3D_1axon_r0", "emix_sub", "delaunay_2d", "2D_neuron_r1_P2", "3D_box_P2", "delaunay_2d_P2",
                                  "tissue_piece_P2"])
def test_seeded_inputs_separate_wrong_kernels(name, mutation):
    """A condition on the inputs of the device tests, not a measurement: with C ~ U(0.5, 4) per cell and species, phi from
    `synthetic_state` and C_PREV = 0, each way of forming the jump term wrong -- its sign, C of the cell across the facet, C of the
    other species, 1/6 for 1/12 -- moves L_knp by more than 1e-3 of its max norm, eight orders above the device tests' 1e-11."""
    pb, C, b = _seeded(name)
    wrong = _stub_rhs(pb, mc.StubMMS(C, *mc.zero_extras(pb), mutation=mutation))
    for k in range(pb.N_ions):
        moved = relerr(wrong[k], b[k])
        print(name, mutation, "species", k, "moved by", moved)
        assert moved > 1e-3


def test_partition_cuts_put_ghost_cells_behind_membrane_facets():
    """The cuts of the partitioned device test: each leaves owned membrane facets whose other cell is a ghost."""
    for p in (1, 2):
        m, s, f, part = mc.partitioned_box(p)
        for rank in range(2):
            loc = part.local(rank)
            _, surf_l = loc.localize(s, f, (1,))
            assert mc.ghost_backed_membrane_facets(loc, surf_l.array(), (1,)) > 0, (p, rank)


# ------------------------------------------------------------------------------------------------------------------------------
# the reference's space MMS
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", [1e-10, 1e-3])
@pytest.mark.parametrize("p", [1, 2])
def test_extra_rhs_matches_the_oracle_restatement(p, dt):
    """knpemidg.mms_terms.extra_rhs (what Solver hands to Device.set_mms) against oracle/mms.py `SpaceMMS`, r = 3: with phi = 0 and
    c_prev_n = 0 the oracle's L_knp is the data term e_knp alone; with c = c_elim = 0 its L_emi is e_emi alone.  Both integrate the
    same smooth data with the same degree-8 rules: measured 0 and <= 2e-16 of the max norm."""
    from knpemidg.mms_terms import extra_rhs
    S = mc.mms_example().make_solver(3, p, dt)
    Cdev, e_emi, e_knp = extra_rhs(S)
    pb = mc.space_mms_problem(S, dt)
    P = pb.mms.P
    for k, s in enumerate("ab"):                                   # ion['C']: C_s1 on the ICS cells (tag 1), C_s2 on the ECS
        assert np.array_equal(Cdev[k], np.where(pb.cell_tags == 1, float(P["C_%s1" % s]), float(P["C_%s2" % s])))
    pb.phi = np.zeros_like(pb.phi)
    pb.c_prev_n = np.zeros_like(pb.c)
    for k in range(pb.N_ions):
        err = relerr(e_knp[k], ko.knp_rhs(pb, k))
        print("p", p, "dt", dt, "e_knp", k, err)
        assert np.abs(e_knp[k]).max() > 0 and err < 1e-13
    pb.c = np.zeros_like(pb.c)
    pb.c_elim = np.zeros_like(pb.c_elim)
    err = relerr(e_emi, ko.emi_rhs(pb))
    print("p", p, "dt", dt, "e_emi", err)
    assert np.abs(e_emi).max() > 0 and err < 1e-13


@pytest.mark.parametrize("r,p", [(3, 1), (2, 2)])
def test_sign_of_the_jump_term_moves_the_solution(r, p):
    """Sensitivity record for the whole-step device test: the oracle's direct solves of the space MMS over four steps at dt = 1e-3,
    with `SpaceMMS` and with a subclass whose jump term has the wrong sign.  Measured displacement relative to the field's max norm,
    r = 3 P1: c 1.9e-1, c_elim 1.5e-1, phi 2.6e-2; r = 2 P2: 2.1e-1, 1.7e-1, 3.0e-2.  Each must exceed 1e-2: a device trajectory
    that agrees with the oracle's to 1e-4 cannot have the term wrong.  At dt = 1e-10 (the setting of the space-convergence tests,
    two steps) the same mutant moves the fields by under 1e-6, which is why those tests cannot stand in for this one."""
    good = mc.oracle_trajectory(r, p, 1e-3, 4)
    bad = mc.oracle_trajectory(r, p, 1e-3, 4, flipped=True)
    moved = dict(c=relerr(bad.c, good.c), c_elim=relerr(bad.c_elim, good.c_elim), phi=relerr(bad.phi, good.phi))
    print("r", r, "p", p, moved)
    for key, v in moved.items():
        assert v > 1e-2, (key, v)
    tiny = mc.oracle_trajectory(r, p, 1e-10, 2), mc.oracle_trajectory(r, p, 1e-10, 2, flipped=True)
    small = max(relerr(tiny[1].c, tiny[0].c), relerr(tiny[1].c_elim, tiny[0].c_elim), relerr(tiny[1].phi, tiny[0].phi))
    print("r", r, "p", p, "dt 1e-10:", small)
    assert small < 1e-6
