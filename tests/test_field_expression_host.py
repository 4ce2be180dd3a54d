"""knpemidg.FieldExpression (knpemidg/expression.py): everything that needs no GPU -- construction refusals, field-name resolution,
the kernel name, the generated translation unit, the hipRTC compile for gfx950 of every (dim, nd, NF) without scratch, compiler
diagnostics -- and the input conditions of the cases tests/test_gpu_field_source.py compares on the device
(tests/field_source_cases.py)."""
import os
import sys
import warnings

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import field_source_cases as FC                        # noqa: E402
import source_cases as SC                              # noqa: E402


@pytest.fixture(scope="module")
def lib():
    import build as _b
    _b.build()
    from knpemidg import _abi
    return _abi.load()


CLEAR = "-k_up * (c_K - c0)"


def test_construction_refusals():
    from knpemidg import Constant, Expression, FieldExpression
    e = FieldExpression(CLEAR, fields=("c_K",), k_up=50.0, c0=Constant(4.0))
    assert isinstance(e, Expression) and e.fields == ("c_K",) and e.subdomains == (0,) and e.names == ("k_up", "c0") and e.degree is None
    assert FieldExpression("1.0", fields=["phi"], subdomains=[2, 0], degree=4).subdomains == (2, 0)
    # what Expression refuses
    with pytest.raises(ValueError, match="vector-valued"):
        FieldExpression(("c_K", "phi"), fields=("c_K", "phi"))
    with pytest.raises(ValueError, match="not a C identifier"):
        FieldExpression("1.0", **{"a-b": 1.0})
    for name in ("x", "pi"):
        with pytest.raises(ValueError, match="collides"):
            FieldExpression("1.0", **{name: 1.0})
    for name in ("knp_params", "double"):
        with pytest.raises(ValueError, match="generated C\\+\\+"):
            FieldExpression("1.0", **{name: 1.0})
    for name in ("values", "kernel_name", "field_ids", "_code", "_fields", "_subdomains"):
        with pytest.raises(ValueError, match="attribute of the Expression"):
            FieldExpression("1.0", **{name: 1.0})
    with pytest.raises(TypeError):                                  # the constructor's own arguments
        FieldExpression("1.0", ("phi",), **{"fields": 1.0})
    with pytest.raises(ValueError, match="at most 32"):
        FieldExpression("1.0", **{"p%d" % i: 0.0 for i in range(33)})
    with pytest.raises(ValueError, match="plain arithmetic"):
        FieldExpression("c_K + __builtin_amdgcn_workitem_id_x()", fields=("c_K",))
    # its own
    for name, flds in (("c_K", ("c_K",)), ("phi", ("c_K",)), ("phi", ()), ("phi", ("phi",))):
        with pytest.raises(ValueError, match="collides with a field"):
            FieldExpression("1.0", fields=flds, **{name: 1.0})
    with pytest.raises(ValueError, match="generated C\\+\\+"):
        FieldExpression("1.0", knp_fields=1.0)
    assert FieldExpression("c_K", c_K=3.0).names == ("c_K",)        # a plain parameter as long as no such field is listed
    for bad in ("c_K", 7, None, ("c_K", 3), (b"phi",)):
        with pytest.raises(ValueError, match="fields must be"):
            FieldExpression("1.0", fields=bad)
    for bad in (("K",), ("c_",), ("c_K+",), ("Phi",), ("",)):
        with pytest.raises(ValueError, match="neither"):
            FieldExpression("1.0", fields=bad)
    with pytest.raises(ValueError, match="listed twice"):
        FieldExpression("1.0", fields=("c_K", "phi", "c_K"))
    for bad in (0, "0", (), [], (0.0,), ("0",), (True,), (-1,), None):
        with pytest.raises(ValueError, match="subdomains must be"):
            FieldExpression("1.0", subdomains=bad)
    with pytest.raises(ValueError, match="listed twice"):
        FieldExpression("1.0", subdomains=(0, 1, 0))
    names = tuple("c_i%d" % i for i in range(9))
    with pytest.raises(ValueError, match="at most 9"):
        FieldExpression("1.0", fields=("phi",) + names)
    assert len(FieldExpression("1.0", fields=("phi",) + names[:8]).fields) == 9
    # attributes: parameters and subdomains are data, everything else is refused
    e.k_up = 80.0
    e.subdomains = [0, 2]
    assert e.values()[0] == 80.0 and e.subdomains == (0, 2)
    with pytest.raises(ValueError, match="listed twice"):
        e.subdomains = (1, 1)
    with pytest.raises(AttributeError):
        e.fields = ("phi",)
    with pytest.raises(AttributeError):
        e.k_down = 1.0


def test_field_names_resolve_against_the_ion_list():
    from knpemidg import FieldExpression
    e = FieldExpression("c_Cl + c_K * phi", fields=("c_Cl", "c_K", "phi"))
    assert e.field_ids(("K", "Cl", "Na")) == [2, 1, 0]
    assert e.field_ids(("Na", "K", "Cl")) == [3, 2, 0]              # the eliminated ion is id n_ions
    assert FieldExpression("1.0").field_ids(("K", "Cl")) == []
    with pytest.raises(ValueError) as err:
        e.field_ids(("K", "Ca", "Na"))
    assert "'c_Cl'" in str(err.value) and "phi, c_K, c_Ca, c_Na" in str(err.value)


def test_solver_resolves_names_and_refuses_mms_in_setup_varform_knp():
    """Without a device: an unknown field name and a manufactured solution are refused before anything is compiled or loaded."""
    from knpemidg import FieldExpression
    from knpemidg.solver import Solver
    S = Solver.__new__(Solver)
    S.mms, S.dev = None, None
    S.ion_list = [{'name': 'K', 'f_source': FieldExpression("c_Ca", fields=("c_Ca",))}, {'name': 'Cl', 'f_source': 0.0}, {'name': 'Na'}]
    with pytest.raises(ValueError, match="no field named 'c_Ca'; the fields of this solver are phi, c_K, c_Cl, c_Na"):
        S.setup_varform_knp()
    S.ion_list[0]['f_source'] = FieldExpression("c_Na", fields=("c_Na",))
    S.mms = object()
    with pytest.raises(ValueError, match="manufactured solution"):
        S.setup_varform_knp()
    S.ion_list[0]['f_source'] = 0.0                                 # no field source: nothing to do, with or without mms
    S.setup_varform_knp()


def test_kernel_name_hashes_code_names_fields_and_basis_not_values_or_subdomains(lib):
    from knpemidg import Expression, FieldExpression
    e = FieldExpression(CLEAR, fields=("c_K",), k_up=50.0, c0=4.0)
    src, kernel = e.source(3, 4)
    same = FieldExpression(CLEAR, fields=("c_K",), subdomains=(1, 2), degree=2, k_up=1.0, c0=0.0)
    assert same.source(3, 4) == (src, kernel)
    e.subdomains = (5,)
    e.c0 = 7.0
    assert e.source(3, 4) == (src, kernel)
    names = {kernel, e.kernel_name(3, 10), e.kernel_name(2, 3), e.kernel_name(2, 6),
             FieldExpression(CLEAR, fields=("c_K", "phi"), k_up=50.0, c0=4.0).kernel_name(3, 4),
             FieldExpression(CLEAR, fields=("c_K",), c0=4.0, k_up=50.0).kernel_name(3, 4),
             FieldExpression(CLEAR + " ", fields=("c_K",), k_up=50.0, c0=4.0).kernel_name(3, 4),
             FieldExpression("k_up * c0", k_up=50.0, c0=4.0).kernel_name(3, 4), Expression("k_up * c0", k_up=50.0, c0=4.0).kernel_name(3, 4),
             # a field name cannot pass for a parameter name: ("a"; fields "c_b") and ("a", "c_b"; no fields) differ
             FieldExpression("1.0", fields=("c_b",), a=1.0).kernel_name(3, 4), FieldExpression("1.0", a=1.0, c_b=1.0).kernel_name(3, 4)}
    assert len(names) == 11
    # the generated text: fields bound in the order of `fields`, in front of the parameters; one kernel around the field template
    two = FieldExpression("g * c_K * exp(-phi / v0)", fields=("c_K", "phi"), g=1.0, v0=0.025)
    src, kernel = two.source(2, 6)
    assert "const double c_K = knp_fields[0];\n        const double phi = knp_fields[1];\n        const double g = knp_params[P_g];" in src
    assert "#line 1 \"knpemidg.FieldExpression\"\ng * c_K * exp(-phi / v0)\n" in src
    assert "source_load_vector_fields<2, 6, 2>(UserSource()" in src and src.count("extern \"C\" __global__") == 1
    assert "SourceFields fld, SourceParams p" in src
    with pytest.raises(ValueError, match="basis"):
        two.source(3, 3)
    # Expression's own text still calls the plain template
    assert "source_load_vector<3, 4>(UserSource()" in Expression("1.0").source(3, 4)[0]


@pytest.mark.parametrize("dim,nd", [(3, 4), (3, 10), (2, 3), (2, 6)])
def test_every_basis_and_field_count_compiles_for_gfx950_without_scratch(lib, dim, nd):
    """NF = 0, 1, 2 and n_ions + 1 of the shipped cases: code objects for gfx950 made without a device, no spill warning."""
    from knpemidg import ode_rtc
    for case in (FC.NO_FIELDS, FC.LINEAR, FC.NONLINEAR, FC.ALL_FIELDS):
        e = case.expression()
        assert len(e.fields) == {"none": 0, "linear": 1, "nonlinear": 2, "all": len(FC.IONS) + 1}[case.name]
        with warnings.catch_warnings():
            warnings.simplefilter("error")
            kernel, code = e.compiled(dim, nd)
        assert code[:4] == b"\x7fELF" and b"gfx950" in code and kernel.encode() in code
        use = ode_rtc.resource_usage(ode_rtc.compile_source(*e.source(dim, nd))[1])
        print("dim %d nd %d NF %d: %s" % (dim, nd, len(e.fields), use))
        assert use["scratch"] == 0 and 0 < use["vgpr"] <= 512, (case.name, use)


def test_compile_error_names_the_users_string(lib):
    from knpemidg import FieldExpression
    from knpemidg._abi import KnpError
    with pytest.raises(KnpError) as e:
        FieldExpression("k_up * c_K\n * c_Na", fields=("c_K",), k_up=1.0).compiled(3, 4)      # c_Na is not listed in fields
    text = str(e.value)
    assert "knpemidg.FieldExpression:2:" in text and "c_Na" in text and "error" in text


@pytest.mark.parametrize("name,degree", SC.ROW_CASES)
def test_field_cases_meet_their_input_conditions(name, degree):
    """The time window is open at T_IN and closed at T_OUT with room to spare; fields lie in their ranges and no two (field, cell,
    node) values coincide; the twin is non-zero on every selected cell, the yardstick is at least the row's own magnitude, and for
    the clearance term it is larger than |f| would give (cancellation in c_K - c0 does not shrink it)."""
    mesh, sub, _ = SC.mesh_of(name)
    tags = np.asarray(sub.array())
    assert FC.T0 * (1 + 1e-9) < FC.T_IN < FC.T1 * (1 - 1e-9) and FC.T_OUT < FC.T0 * (1 - 1e-9)
    nd = FC.nd_of(mesh.gdim, degree)
    U = FC.fields(mesh.num_cells(), nd)
    assert sorted(U) == sorted(FC.FIELD_NAMES)
    for key, a in U.items():
        lo, hi = (-0.1, 0.1) if key == "phi" else (1.0, 150.0)
        assert a.shape == (mesh.num_cells(), nd) and lo <= a.min() and a.max() <= hi
    allv = np.concatenate([a.ravel() for a in U.values()])
    assert len(np.unique(allv)) == allv.size
    for case in FC.CASES.values():
        # the C++ side of the case: the fields and parameters its string uses are the ones the twin is written over
        windowed, bare = case.expression(FC.T_IN, subdomains=(0, 1)), case.expression(None)
        assert windowed.fields == bare.fields == case.fields and windowed.subdomains == (0, 1) and bare.subdomains == (0,)
        assert bare.names == tuple(case.params) and windowed.names == tuple(case.params) + ("t0", "t1", "t")
        assert dict(zip(windowed.names, windowed.values())) == dict(case.params, t0=FC.T0, t1=FC.T1, t=FC.T_IN)
        assert bare.code == case.code and windowed.code == "(" + case.code + ")" + FC.WINDOW
        used = set(__import__("re").findall(r"[A-Za-z_]\w*", case.code)) - {"exp", "sin", "x"}
        assert used == set(case.fields) | set(case.params), (case.name, used)
        for subdomains in ((0,), (0, 1)):
            row, scale = FC.twin_row(mesh, tags, degree, case, U, FC.T_IN, subdomains)
            sel = FC.selection(tags, subdomains)
            assert np.all(scale[sel] > 0) and np.all(np.abs(row[sel]).max(axis=1) > 0) and np.all(scale >= np.abs(row) * (1 - 1e-12))
            out = np.ones(len(tags), bool); out[sel] = False
            assert not row[out].any() and not scale[out].any()
            assert not FC.twin_row(mesh, tags, degree, case, U, FC.T_OUT, subdomains)[0].any()
    bary, w, B = FC.tables(mesh.gdim, degree)
    u = U["c_K"] @ B.T
    M, absf = FC.K_UP * (np.abs(u) + FC.C0), np.abs(FC.K_UP * (u - FC.C0))
    assert (M >= absf).all() and (M[u > 0] > absf[u > 0] * (1 + 1e-3)).all() and (u > 0).mean() > 0.9      # a P2 interpolant may dip below 0
    for fname in FC.FIELD_NAMES:
        row, scale = FC.mass_row(mesh, tags, degree, U[fname])
        one_hot = FC.Case("one", fname, (fname,), {}, lambda X, v, f=fname: v[f], lambda X, v, f=fname: np.abs(v[f]))
        ref, _ = FC.twin_row(mesh, tags, degree, one_hot, U, FC.T_IN)
        assert FC.worst_ratio(ref, row, scale) <= FC.BOUND            # the two host references of the one-hot rows agree
