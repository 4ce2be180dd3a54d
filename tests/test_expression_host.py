"""knpemidg.Expression (knpemidg/expression.py): everything that needs no GPU -- the generated translation unit, the hipRTC compile
for gfx950 and its memo, the construction errors, compiler diagnostics, late parameter reading -- and the input conditions of the
cases tests/test_gpu_source.py compares on the device (tests/source_cases.py)."""
import os
import sys
import warnings

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import source_cases as SC                              # noqa: E402


@pytest.fixture(scope="module")
def lib():
    import build as _b
    _b.build()
    from knpemidg import _abi
    return _abi.load()


BOX = "g_syn * ((x[0] >= x_lo && x[0] <= x_hi && x[1] >= y_lo && x[1] <= y_hi) ? 1.0 : 0.0) * ((t >= t_on && t <= t_off) ? 1.0 : 0.0)"
BOX_PARAMS = dict(g_syn=40.0, x_lo=0.1, x_hi=0.2, y_lo=0.0, y_hi=0.5, t_on=1.0, t_off=2.0, t=0.0)


def test_generated_source_holds_the_enum_in_declaration_order_and_a_stable_kernel_name(lib):
    from knpemidg import Expression
    e = Expression(BOX, degree=4, **BOX_PARAMS)
    assert e.degree == 4 and e.names == tuple(BOX_PARAMS)
    src, kernel = e.source(2, 3)
    assert "enum : int { P_g_syn = 0, P_x_lo = 1, P_x_hi = 2, P_y_lo = 3, P_y_hi = 4, P_t_on = 5, P_t_off = 6, P_t = 7 };" in src
    assert "#line 1 \"knpemidg.Expression\"\n" + BOX + "\n" in src
    assert "source_load_vector<2, 3>(UserSource()" in src and ("void %s(" % kernel) in src and src.count("extern \"C\" __global__") == 1
    # the name is a function of (code, parameter names, dim, nd): not of the values, and different for each of the four
    same = Expression(BOX, **dict(BOX_PARAMS, g_syn=1.0, t=7.0))
    assert same.source(2, 3) == (src, kernel)
    names = {kernel, e.kernel_name(2, 6), e.kernel_name(3, 4), e.kernel_name(3, 10),
             Expression(BOX + " * 2.0", **BOX_PARAMS).kernel_name(2, 3),
             Expression(BOX, **dict(list(BOX_PARAMS.items())[::-1])).kernel_name(2, 3)}
    assert len(names) == 6
    with pytest.raises(ValueError, match="basis"):
        e.source(3, 3)


def test_compiles_for_gfx950_without_a_device_and_a_second_expression_hits_the_memo(lib, monkeypatch):
    from knpemidg import Expression, ode_rtc
    calls = []
    real = ode_rtc._hiprtc

    def counting(src, kernel):
        calls.append(kernel)
        return real(src, kernel)
    monkeypatch.setattr(ode_rtc, "_hiprtc", counting)
    code_text = BOX + " * (1.0 + 0.25 * cos(pi * x[0]))"            # a text no other test compiles: the memo is per process
    with warnings.catch_warnings():
        warnings.simplefilter("error")                              # a spill warning would be a finding
        kernel, code = Expression(code_text, degree=2, **BOX_PARAMS).compiled(2, 3)
        kernel2, code2 = Expression(code_text, degree=1, **dict(BOX_PARAMS, g_syn=3.0)).compiled(2, 3)
    assert calls == [kernel] and kernel2 == kernel and code2 is code
    assert code[:4] == b"\x7fELF" and b"gfx950" in code and kernel.encode() in code
    src, _ = Expression(code_text, **BOX_PARAMS).source(2, 3)
    use = ode_rtc.resource_usage(ode_rtc.compile_source(src, kernel)[1])
    assert use["scratch"] == 0 and 0 < use["vgpr"] <= 512, use
    assert calls == [kernel]
    for dim, nd in ((2, 6), (3, 4), (3, 10)):                       # every (dim, nd) a solver can ask for: all without scratch
        e = Expression(code_text if dim == 2 else code_text + " * x[2]", **BOX_PARAMS)
        s, k = e.source(dim, nd)
        assert ode_rtc.resource_usage(ode_rtc.compile_source(s, k)[1])["scratch"] == 0, (dim, nd)


def test_construction_errors():
    from knpemidg import Expression
    with pytest.raises(ValueError, match="vector-valued"):
        Expression(("x[0]", "x[1]"), degree=1)
    with pytest.raises(ValueError, match="vector-valued"):
        Expression(["x[0]"], degree=1)
    with pytest.raises(ValueError, match="not a C identifier"):
        Expression("1.0", **{"2fast": 1.0})
    with pytest.raises(ValueError, match="not a C identifier"):
        Expression("1.0", **{"a-b": 1.0})
    for name in ("x", "pi"):
        with pytest.raises(ValueError, match="collides"):
            Expression("1.0", **{name: 1.0})
    with pytest.raises(TypeError):                                  # `code` and `degree` are the constructor's own arguments
        Expression("1.0", **{"code": 1.0})
    for name in ("values", "names", "source", "compiled", "prefetch", "kernel_name", "_code", "_params", "__class__"):
        with pytest.raises(ValueError, match="attribute of the Expression"):
            Expression("1.0", **{name: 1.0})
    for name in ("knp_params", "double", "return", "class"):
        with pytest.raises(ValueError, match="generated C\\+\\+"):
            Expression("1.0", **{name: 1.0})
    with pytest.raises(ValueError, match="at most 32"):
        Expression("1.0", **{"p%d" % i: 0.0 for i in range(33)})
    assert len(Expression("1.0", **{"p%d" % i: 0.0 for i in range(32)}).values()) == 32
    from knpemidg import ode_rtc
    for bad in ("x[0] + __builtin_amdgcn_workitem_id_x()", "asm(\"\") , 1.0"):
        assert ode_rtc._FORBIDDEN.search(bad)
        with pytest.raises(ValueError, match="plain arithmetic"):
            Expression(bad)


def test_compile_error_carries_the_log_and_names_the_users_string(lib):
    from knpemidg import Expression
    from knpemidg._abi import KnpError
    with pytest.raises(KnpError) as e:
        Expression("g_syn * (x[0] > 0.0)\n * undeclared_name", g_syn=1.0).compiled(3, 4)
    text = str(e.value)
    assert "knpemidg.Expression:2:" in text and "undeclared_name" in text and "error" in text


def test_constants_are_read_late_and_assignment_changes_values_not_the_source(lib):
    from knpemidg import Constant, Expression
    t = Constant(0.0)
    e = Expression(BOX, degree=4, **dict(BOX_PARAMS, t=t))
    src, kernel = e.source(2, 3)
    assert e.values()[-1] == 0.0
    t.assign(1.5)
    assert e.values()[-1] == 1.5 and e.t is t
    e.g_syn = 65.0
    assert e.values()[0] == 65.0 and e.g_syn == 65.0
    e.x_lo = Constant(0.3)
    assert e.values()[1] == 0.3
    assert e.source(2, 3) == (src, kernel)
    assert e.values().dtype == np.float64 and e.values().shape == (8,)
    with pytest.raises(AttributeError):
        e.g_sin = 1.0                                               # a typo is not a new parameter
    with pytest.raises((TypeError, ValueError)):
        e.g_syn = "much"


@pytest.mark.parametrize("name", SC.MESHES)
def test_source_cases_meet_their_input_conditions(lib, name):
    """Strictly inside the box lie a whole ECS cell and a cut one (some but not all quadrature points inside), and no quadrature
    point of an ECS cell is closer to a box face than 1e-9 of the mesh extent along that axis: a rounding difference in x_q cannot
    flip the indicator between host and device."""
    mesh, sub, _ = SC.mesh_of(name)
    a, b = SC.box_of(mesh)
    sel, X = SC.ecs_points(mesh, sub.array())
    inside = np.all((X >= a) & (X <= b), axis=-1)
    whole, cut = inside.all(axis=1), inside.any(axis=1) & ~inside.all(axis=1)
    extent = mesh.coords.max(axis=0) - mesh.coords.min(axis=0)
    gap = np.minimum(np.abs(X - a), np.abs(X - b)) / extent
    print(name, "ECS cells", len(sel), "whole", int(whole.sum()), "cut", int(cut.sum()), "closest point / extent", gap.min())
    assert whole.sum() >= 1 and cut.sum() >= 1
    assert gap.min() > 1e-9
    f = SC.twin(mesh)
    row, scale = SC.host_row(mesh, sub.array(), 1, f, SC.T_IN)
    assert np.abs(row).max() > 0 and np.all(scale >= np.abs(row) * (1 - 1e-12))
    assert not SC.host_row(mesh, sub.array(), 1, f, SC.T_OUT)[0].any()
