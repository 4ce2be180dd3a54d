"""Runtime compilation of user-written membrane models (knpemidg/ode_rtc.py, knp_ode_rtc_compile): everything that needs no
GPU -- translation unit, protocol checks, hipRTC compile for gfx950, compiler diagnostics and the per-process memo."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "examples", "custom_membrane_model"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import rtc_models                                     # noqa: E402


@pytest.fixture(scope="module")
def rtc():
    import build as _b
    _b.build()
    from knpemidg import ode_rtc
    return ode_rtc


def _test_models():
    import mm_hh_q10
    import mm_hh_rtc
    return [rtc_models.fhn(), mm_hh_rtc, mm_hh_q10]


def test_each_model_compiles_to_a_gfx950_code_object_without_scratch(rtc):
    for ode in _test_models():
        src, kernel, ns, npar = rtc.source(ode)
        assert kernel.startswith("k_ode_rtc_" + rtc.module_name(ode) + "_") and len(kernel.rsplit("_", 1)[1]) == 8
        assert (ns, npar) == (len(ode.init_state_values()), len(ode.init_parameter_values()))
        assert "#line 1 \"%s.HIP_RHS\"" % rtc.module_name(ode) in src
        code, log = rtc.compile_source(src, kernel)
        assert code[:4] == b"\x7fELF" and len(code) > 1000
        assert b"gfx950" in code and kernel.encode() in code
        use = rtc.resource_usage(log)
        assert use["scratch"] == 0, (kernel, use)
        assert use["vgpr"] is not None and 0 < use["vgpr"] <= 512, (kernel, use)


def test_compile_error_names_the_model_and_the_users_line(rtc):
    from knpemidg._abi import KnpError
    body = rtc_models.FHN_BODY.replace("p[P_I_ch_K] = i_K;", "p[P_I_ch_K] = i_K +;")
    line = body.split("\n").index("p[P_I_ch_K] = i_K +;") + 1          # line numbers of the HIP_RHS string itself
    ode = rtc_models.make_model("mm_broken", body)
    src, kernel, _, _ = rtc.source(ode)
    with pytest.raises(KnpError) as e:
        rtc.compile_source(src, kernel)
    assert "mm_broken.HIP_RHS:%d:" % line in str(e.value), str(e.value)[:2000]
    with pytest.raises(KnpError):                     # memoised failure: the same error again, not a silent success
        rtc.compiled(ode)


def test_protocol_violations_raise_value_error(rtc):
    with pytest.raises(ValueError, match="asm"):
        rtc.source(rtc_models.make_model("mm_asm", 'asm volatile("v_nop");\n' + rtc_models.FHN_BODY))
    with pytest.raises(ValueError, match="__asm__"):
        rtc.source(rtc_models.make_model("mm_asm2", '__asm__("v_nop");\n' + rtc_models.FHN_BODY))
    with pytest.raises(ValueError, match="identifier"):
        rtc.source(rtc_models.make_model("mm_badname", rtc_models.FHN_BODY, states=("v", "w-gate")))
    many = tuple("s%d" % i for i in range(rtc.MAX_STATES + 1))
    with pytest.raises(ValueError, match="states"):
        rtc.source(rtc_models.make_model("mm_big", "dy[0] = 0.0;", states=many))
    many = tuple("q%d" % i for i in range(rtc.MAX_PARAMS + 1))
    with pytest.raises(ValueError, match="parameters"):
        rtc.source(rtc_models.make_model("mm_bigp", "dy[0] = 0.0;", params=many))
    # the checks run before any compile: prefetch raises them on the caller's thread
    with pytest.raises(ValueError):
        rtc.prefetch([rtc_models.make_model("mm_asm3", "asm(\"\");")])


def test_source_is_deterministic_and_the_memo_returns_the_same_bytes(rtc):
    a = rtc.source(rtc_models.fhn())
    b = rtc.source(rtc_models.fhn())
    assert a == b
    c1, _ = rtc.compile_source(a[0], a[1])
    c2, _ = rtc.compile_source(b[0], b[1])
    assert c1 is c2                                   # one compile per process and source text
    kernel, ns, npar, code = rtc.compiled(rtc_models.fhn())
    assert (kernel, ns, npar) == (a[1], 2, 9) and code is c1
    # a different body is a different kernel
    other = rtc_models.make_model("mm_fhn", rtc_models.FHN_BODY.replace("3.0", "3.5"))
    assert rtc.source(other)[1] != a[1]


def test_prefetch_compiles_on_a_worker_and_skips_built_in_and_host_only_models(rtc):
    from knpemidg.models import mm_hh
    host_only = rtc_models.make_model("mm_host_only", None)
    assert rtc.prefetch([mm_hh, host_only]) is None
    ode = rtc_models.make_model("mm_fhn_prefetch", rtc_models.FHN_BODY)
    th = rtc.prefetch([ode, ode])
    assert th is not None
    th.join(60)
    src, kernel, _, _ = rtc.source(ode)
    import hashlib
    fut = rtc._memo[hashlib.sha256(src.encode()).hexdigest()]
    assert fut.done() and fut.result()[0][:4] == b"\x7fELF"
