"""Space- and time-dependent ion sources on the device: `Expression`, shaped like dolfin's.

    f = Expression("g_syn * (x[0] > x0 && x[0] < x1) * (t > t0 && t < t1)", degree=4, g_syn=40.0, x0=..., x1=..., t0=..., t1=..., t=t)
    ion['f_source'] = f

`code` is one scalar C++ expression over x[0] ... x[dim-1] and the named parameters (`pi` is predefined).  This module wraps it
into a translation unit around csrc/source_rtc.hpp -- the functor `UserSource`, the parameters as an enum of indices into the
value vector, and one `extern "C"` kernel for the mesh dimension and basis size in use -- and compiles it for gfx950 through
`ode_rtc.compile_source` (hipRTC, no device needed, memoised per process by the source text).  The solver registers the kernel
with its context (knp_source_register) and launches it before every KNP solve (knp_source_eval): the load vector int f v dx(0) of
the ECS cells by the degree-8 rule of the host path (mms_terms.QDEG), written into the species' row of the buffer the right-hand-
side kernels add to L_knp.  Parameter values are kernel arguments, not source text: a `Constant` is read at every evaluation (so
`t=t` follows the solver's time constant), and `expr.g_syn = 65.0` takes effect at the next one without a recompile.

`FieldExpression` is an `Expression` that also reads phi and concentrations at the quadrature points and integrates over the cells
of any listed subdomains (source_load_vector_fields of the same header, knp_source_register_fields).
"""
import hashlib
import os
import warnings

import numpy as np

from knpemidg import ode_rtc

MAX_PARAMS = 32              # KNP_SOURCE_MAX_PARAMS of csrc/source_rtc.hpp
HEADER = os.path.join(os.path.dirname(ode_rtc.HEADER), "source_rtc.hpp")
LINE_FILE = "knpemidg.Expression"            # the file name compiler diagnostics of the user's string carry
_RESERVED = ("x", "pi")
_ARGUMENT = "knp_params"                     # the functor's second argument in the generated text
_OWN_ATTRIBUTES = ("_code", "_names", "_params", "degree")      # instance attributes; methods and properties are found on the class
_CPP_KEYWORDS = frozenset("""alignas alignof and and_eq asm auto bitand bitor bool break case catch char char8_t char16_t char32_t class
compl concept const consteval constexpr constinit const_cast continue co_await co_return co_yield decltype default delete do double
dynamic_cast else enum explicit export extern false float for friend goto if inline int long mutable namespace new noexcept not not_eq
nullptr operator or or_eq private protected public register reinterpret_cast requires return short signed sizeof static static_assert
static_cast struct switch template this thread_local throw true try typedef typeid typename union unsigned using virtual void volatile
wchar_t while xor xor_eq""".split())


class Expression:
    """Expression(code, degree=None, **params): a scalar source term f(x; params) evaluated on the device.

    `degree` is accepted and stored for source compatibility with dolfin only: the load vector is always integrated with the
    degree-8 simplex rule (mms_terms.QDEG), exactly as the host path for plain callables ignores it.  Parameter values are numbers
    or scalar `knpemidg.Constant`s; a Constant is read when the source is evaluated, not here.  Assigning to a parameter's
    attribute replaces its value.  ValueError for a vector-valued `code`, a parameter name that is no C identifier, is `x` / `pi`,
    a C++ keyword, `knp_params` (the generated functor's argument) or an attribute of this class (`values`, `code`, `source`, ...:
    `expr.<name>` must mean the parameter), more than 32 parameters, and inline assembly or target builtins in `code`."""

    def __init__(self, code, degree=None, **params):
        if isinstance(code, (tuple, list)):
            raise ValueError("Expression: vector-valued expressions (a tuple or list of strings) are not supported; a source is a scalar")
        if not isinstance(code, str) or not code.strip():
            raise ValueError("Expression: code must be a non-empty string holding one scalar C++ expression")
        m = ode_rtc._FORBIDDEN.search(code)
        if m:
            raise ValueError("Expression uses %r: a source is plain arithmetic (no inline assembly, no target builtins)" % m.group(1))
        if len(params) > MAX_PARAMS:
            raise ValueError("Expression: %d parameters; the device kernel takes at most %d" % (len(params), MAX_PARAMS))
        for name in params:
            if not ode_rtc._IDENT.match(name):
                raise ValueError("Expression: parameter name %r is not a C identifier" % name)
            if name in _RESERVED:
                raise ValueError("Expression: parameter name %r collides with the predefined %s" % (name, " / ".join(_RESERVED)))
            if name == _ARGUMENT or name in _CPP_KEYWORDS:
                raise ValueError("Expression: parameter name %r collides with a name of the generated C++ (a keyword or the functor's argument)" % name)
            if name in _OWN_ATTRIBUTES or hasattr(type(self), name):
                raise ValueError("Expression: parameter name %r collides with an attribute of the Expression object itself" % name)
        object.__setattr__(self, "_code", code)
        object.__setattr__(self, "_names", tuple(params))          # declaration order = index into the value vector
        object.__setattr__(self, "_params", dict(params))
        object.__setattr__(self, "degree", degree)
        self.values()                                               # every value converts to a float

    def __setattr__(self, name, value):
        if name in self._params:
            float(value)
            self._params[name] = value
        elif name == "degree":
            object.__setattr__(self, name, value)
        else:
            raise AttributeError("%r is not a parameter of this Expression (parameters: %s)" % (name, ", ".join(self._names) or "none"))

    def __getattr__(self, name):
        params = self.__dict__.get("_params", {})
        if name in params:
            return params[name]
        raise AttributeError(name)

    @property
    def code(self):
        return self._code

    @property
    def names(self):
        return self._names

    def values(self):
        """The parameter values as they are now (Constants are read here), in declaration order."""
        return np.array([float(self._params[n]) for n in self._names], dtype=np.float64)

    def kernel_name(self, dim, nd):
        """A function of (code, parameter names, dim, nd) -- not of the parameter values."""
        tag = hashlib.sha256("\0".join((self._code,) + self._names + (str(int(dim)), str(int(nd)))).encode()).hexdigest()[:12]
        return "k_source_%dd_%d_%s" % (int(dim), int(nd), tag)

    def source(self, dim, nd):
        """(translation unit, kernel name) for a mesh of dimension `dim` with `nd` basis functions per cell."""
        dim, nd = int(dim), int(nd)
        if dim not in (2, 3) or nd not in {2: (3, 6), 3: (4, 10)}[dim]:
            raise ValueError("Expression: no DG-P1 / P2 basis with %d functions per cell in %dD" % (nd, dim))
        kernel = self.kernel_name(dim, nd)
        enum = "enum : int { %s };\n" % ", ".join("P_%s = %d" % (n, i) for i, n in enumerate(self._names)) if self._names else ""
        head = ("// %s: ion source over x[0..%d] with %d parameters, generated by knpemidg/expression.py\n"
                "typedef long int64_t;\n"
                "typedef int int32_t;\n" % (kernel, dim - 1, len(self._names))) + enum + \
            "struct UserSource {\n" \
            "    __device__ __forceinline__ double operator()(const double* x, const double* knp_params) const {\n" \
            "        const double pi = 3.14159265358979323846;\n" + \
            "".join("        const double %s = knp_params[P_%s];\n" % (n, n) for n in self._names) + \
            "        return (\n" \
            "#line 1 \"%s\"\n" % LINE_FILE
        with open(HEADER) as fh:
            header = fh.read()
        tail_line = head.count("\n") + self._code.count("\n") + 3      # the line after the #line directive below
        tail = ("\n#line %d \"%s.cpp\"\n" % (tail_line, kernel)) + \
            "        );\n" \
            "    }\n" \
            "};\n" + header + \
            ("\nextern \"C\" __global__ __launch_bounds__(KNP_SOURCE_BLOCK) void %s(int64_t n, const int32_t* __restrict__ sel,\n"
             "        const double* __restrict__ coords, const int32_t* __restrict__ cells, int nq, const double* __restrict__ bary,\n"
             "        const double* __restrict__ w, const double* __restrict__ B, SourceParams p, double* __restrict__ out) {\n"
             "    source_load_vector<%d, %d>(UserSource(), n, sel, coords, cells, nq, bary, w, B, p, out);\n"
             "}\n" % (kernel, dim, nd))
        return head + self._code + tail, kernel

    def compiled(self, dim, nd):
        """(kernel name, code object bytes); joins a compile `prefetch` started.  A compile error raises KnpError with the log."""
        src, kernel = self.source(dim, nd)
        code, log = ode_rtc.compile_source(src, kernel)
        scratch = ode_rtc.resource_usage(log)["scratch"]
        if scratch:
            warnings.warn("Expression %r: the device kernel spills (%d bytes of scratch per lane); it runs, but slowly"
                          % (self._code, scratch), RuntimeWarning, stacklevel=2)
        return kernel, code

    def prefetch(self, dim, nd):
        """Start the compile on a worker thread (it needs no device); errors surface in `compiled`."""
        import threading
        src, kernel = self.source(dim, nd)

        def run():
            try:
                ode_rtc.compile_source(src, kernel)
            except Exception:
                pass                                 # kept in the memo; re-raised by compiled() on the caller's thread
        th = threading.Thread(target=run, name="knp-source-rtc", daemon=True)
        th.start()
        return th


MAX_FIELDS = 9               # KNP_SOURCE_MAX_FIELDS of csrc/source_rtc.hpp: phi and KNP_MAX_IONS concentrations
FIELD_LINE_FILE = "knpemidg.FieldExpression"
_FIELDS_ARGUMENT = "knp_fields"              # the functor's argument holding the field values at the quadrature point


class FieldExpression(Expression):
    """FieldExpression(code, fields=(), subdomains=(0,), degree=None, **params): a source term f(x, u(x); params) that reads the
    solution, integrated over the cells of the listed subdomains.

        ion_K['f_source'] = FieldExpression("-k_up * (c_K - c0)", fields=("c_K",), k_up=50.0, c0=4.0)
        ion_K['f_source'] = FieldExpression("amp * (t > t0 && t < t1)", subdomains=(1,), amp=..., t0=..., t1=..., t=t)

    `fields` lists distinct names out of "phi" and "c_<name>", <name> an ion['name'] of the solver's ion list (the eliminated ion
    included); inside `code` each is a double holding that field's value at the quadrature point, u(x_q) = sum_a U[a] B[q][a] with
    the cell's nodal values U.  The names are resolved against the ion list when the solver registers the source
    (Solver.setup_varform_knp); an unknown one raises ValueError there.  `subdomains` is a non-empty tuple of distinct cell tags:
    the load vector is int f v dx over the cells carrying one of them, (0,) -- the ECS -- by default.  A tag no cell carries is
    allowed: the row is zero and nothing is launched.  Parameters, `degree` and the refusals are those of `Expression`; in addition
    ValueError for a parameter named like a listed field, `phi` or `knp_fields`, for `fields` / `subdomains` that are no tuple or
    list of str / int, and for duplicates in either.  Subdomains and parameter values are data: `expr.subdomains = (0, 1)` and
    `expr.k_up = 80.0` need no recompile.

    Time level.  The source is evaluated before every KNP solve.  Concentrations, the eliminated ion's included, are those of the
    previous time level n (KNP_F_C_PREV, KNP_F_C_ELIM), phi is the one of this step's EMI solve, just done.  The reaction is
    therefore explicit in a step whose diffusion is implicit: a rate with k * dt of order one or more is unstable, and nothing
    guards against it, nor against injecting net charge.  In the Picard variant every iteration of a step sees the same level-n
    concentrations of the solved species (the eliminated ion's field is recomputed from the iterate, as it always is there).  A
    manufactured solution (mms) refuses a FieldExpression as it refuses an Expression."""

    def __init__(self, code, fields=(), subdomains=(0,), degree=None, **params):
        if not isinstance(fields, (tuple, list)) or not all(isinstance(f, str) for f in fields):
            raise ValueError("FieldExpression: fields must be a tuple or list of names (\"phi\", \"c_<ion name>\")")
        fields = tuple(fields)
        if len(set(fields)) != len(fields):
            raise ValueError("FieldExpression: a field is listed twice in %r" % (fields,))
        if len(fields) > MAX_FIELDS:
            raise ValueError("FieldExpression: %d fields; the device kernel takes at most %d (phi and every ion)" % (len(fields), MAX_FIELDS))
        for f in fields:
            if f != "phi" and not (f.startswith("c_") and len(f) > 2 and ode_rtc._IDENT.match(f)):
                raise ValueError("FieldExpression: field %r is neither \"phi\" nor \"c_<ion name>\"" % f)
        subdomains = self._checked_subdomains(subdomains)
        for name in params:
            if name in fields or name == "phi":
                raise ValueError("FieldExpression: parameter name %r collides with a field the expression reads (or phi)" % name)
            if name == _FIELDS_ARGUMENT:
                raise ValueError("FieldExpression: parameter name %r collides with a name of the generated C++ (the functor's argument)" % name)
            if name in ("_fields", "_subdomains"):
                raise ValueError("FieldExpression: parameter name %r collides with an attribute of the Expression object itself" % name)
        object.__setattr__(self, "_fields", fields)
        object.__setattr__(self, "_subdomains", subdomains)
        Expression.__init__(self, code, degree=degree, **params)

    @staticmethod
    def _checked_subdomains(subdomains):
        ok = isinstance(subdomains, (tuple, list)) and all(isinstance(s, (int, np.integer)) and not isinstance(s, bool) for s in subdomains)
        if not ok or not len(subdomains) or min(subdomains) < 0:
            raise ValueError("FieldExpression: subdomains must be a non-empty tuple or list of cell tags (non-negative ints)")
        subdomains = tuple(int(s) for s in subdomains)
        if len(set(subdomains)) != len(subdomains):
            raise ValueError("FieldExpression: a subdomain is listed twice in %r" % (subdomains,))
        return subdomains

    def __setattr__(self, name, value):
        if name == "subdomains":
            object.__setattr__(self, "_subdomains", self._checked_subdomains(value))
        else:
            Expression.__setattr__(self, name, value)

    @property
    def fields(self):
        return self._fields

    @property
    def subdomains(self):
        return self._subdomains

    def field_ids(self, ion_names):
        """The fields as the ids of knp_source_register_fields: 0 for phi, 1 + i for "c_<name>" with <name> the i-th of
        `ion_names` (the solver's ion list in order, the eliminated ion last).  ValueError for a name that is not among them."""
        known = ["phi"] + ["c_%s" % n for n in ion_names]
        missing = [f for f in self._fields if f not in known]
        if missing:
            raise ValueError("FieldExpression: no field named %s; the fields of this solver are %s"
                             % (", ".join(repr(f) for f in missing), ", ".join(known)))
        return [known.index(f) for f in self._fields]

    def kernel_name(self, dim, nd):
        """A function of (code, parameter names, field names, dim, nd) -- not of the subdomains or the parameter values."""
        parts = (self._code,) + self._names + ("fields",) + self._fields + (str(int(dim)), str(int(nd)))
        return "k_fsource_%dd_%d_%s" % (int(dim), int(nd), hashlib.sha256("\0".join(parts).encode()).hexdigest()[:12])

    def source(self, dim, nd):
        """(translation unit, kernel name) for a mesh of dimension `dim` with `nd` basis functions per cell."""
        dim, nd = int(dim), int(nd)
        if dim not in (2, 3) or nd not in {2: (3, 6), 3: (4, 10)}[dim]:
            raise ValueError("Expression: no DG-P1 / P2 basis with %d functions per cell in %dD" % (nd, dim))
        kernel = self.kernel_name(dim, nd)
        enum = "enum : int { %s };\n" % ", ".join("P_%s = %d" % (n, i) for i, n in enumerate(self._names)) if self._names else ""
        head = ("// %s: ion source over x[0..%d], %d fields and %d parameters, generated by knpemidg/expression.py\n"
                "typedef long int64_t;\n"
                "typedef int int32_t;\n" % (kernel, dim - 1, len(self._fields), len(self._names))) + enum + \
            "struct UserSource {\n" \
            "    __device__ __forceinline__ double operator()(const double* x, const double* knp_fields, const double* knp_params) const {\n" \
            "        const double pi = 3.14159265358979323846;\n" + \
            "".join("        const double %s = knp_fields[%d];\n" % (f, i) for i, f in enumerate(self._fields)) + \
            "".join("        const double %s = knp_params[P_%s];\n" % (n, n) for n in self._names) + \
            "        return (\n" \
            "#line 1 \"%s\"\n" % FIELD_LINE_FILE
        with open(HEADER) as fh:
            header = fh.read()
        tail_line = head.count("\n") + self._code.count("\n") + 3      # the line after the #line directive below
        tail = ("\n#line %d \"%s.cpp\"\n" % (tail_line, kernel)) + \
            "        );\n" \
            "    }\n" \
            "};\n" + header + \
            ("\nextern \"C\" __global__ __launch_bounds__(KNP_SOURCE_BLOCK) void %s(int64_t n, const int32_t* __restrict__ sel,\n"
             "        const double* __restrict__ coords, const int32_t* __restrict__ cells, int nq, const double* __restrict__ bary,\n"
             "        const double* __restrict__ w, const double* __restrict__ B, SourceFields fld, SourceParams p,\n"
             "        double* __restrict__ out) {\n"
             "    source_load_vector_fields<%d, %d, %d>(UserSource(), n, sel, coords, cells, nq, bary, w, B, fld, p, out);\n"
             "}\n" % (kernel, dim, nd, len(self._fields)))
        return head + self._code + tail, kernel


def rule_tables(dim, degree):
    """(bary[nq, dim+1], w[nq], B[nq, nd]) of the source rule for DG-`degree`: the numbers of mms_terms._cell_source."""
    from knpemidg.dgtab import tabulate
    from knpemidg.mms_terms import QDEG
    from knpemidg.quadrature import simplex_rule
    bary, w = simplex_rule(dim, QDEG)
    B = tabulate(degree, bary)[0]
    return np.ascontiguousarray(bary, dtype=np.float64), np.ascontiguousarray(w, dtype=np.float64), np.ascontiguousarray(B, dtype=np.float64)
