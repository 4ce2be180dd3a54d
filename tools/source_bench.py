"""Measurements of the device-evaluated ion sources.  Needs an MI355X.

    python tools/source_bench.py eval [--resolutions 1 2] [--host-resolution 1]
        time of one knp_source_eval on make_mesh_3D(r): knp_timer_begin / _end around 20 back-to-back evaluations after 3 warm-up
        ones, the algorithmic bytes over that time, and next to it the wall time of the host path (the body of Solver.
        _update_host_sources: mms_terms._cell_source on the numpy twin + the blocking upload) on make_mesh_3D(--host-resolution).
        Next to it, in the same call, two field sources: the NF = 2 nonlinear FieldExpression
        g c_K exp(-phi / v0) on the ECS, and the NF = 0 FieldExpression of the same box code on subdomains (0, 1), with pseudo-random
        fields in the device's buffers (concentrations in [1, 150], phi in [-0.1, 0.1]).
    python tools/source_bench.py step --source on|off|clearance [bench.py arguments]
        bench.py's own timing loop (its main(), unchanged) with a box source on species 0 (an Expression, active in every step), with
        the first-order clearance -k (c_K - c0) on species 0 (a FieldExpression on the ECS), or with the f_source = Constant(0)
        bench.py runs by default; prints bench.py's JSON line.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "knp-emi-dg_amd"), os.path.join(ROOT, "examples", "idealized_geometries")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

HBM_BYTES_PER_S = 8.0e12          # the peak the README's roofline figures use
G, K_WAVE = 40.0, 4.0e5
CODE = ("g * ((x[0] >= a0 && x[0] <= b0 && x[1] >= a1 && x[1] <= b1 && x[2] >= a2 && x[2] <= b2) ? 1.0 : 0.0)"
        " * ((t0 <= t && t <= t1) ? 1.0 : 0.0) * (1.0 + 0.3 * sin(k * x[0]))")


def box(mesh):
    lo, hi = mesh.coords.min(axis=0), mesh.coords.max(axis=0)
    return lo + 0.05 * (hi - lo), lo + 0.55 * (hi - lo)


def expression(mesh, t):
    from knpemidg import Expression
    a, b = box(mesh)
    return Expression(CODE, degree=4, g=G, k=K_WAVE, t0=-1.0, t1=1.0e9, t=t, a0=a[0], b0=b[0], a1=a[1], b1=b[1], a2=a[2], b2=b[2])


def twin(mesh):
    a, b = box(mesh)
    return lambda X, t: G * np.all((X >= a) & (X <= b), axis=-1) * (1.0 + 0.3 * np.sin(K_WAVE * X[..., 0]))


def timed(dev, species, values, reps=20):
    """ms of one knp_source_eval: `reps` back to back between two events, after 3 warm-up evaluations"""
    for _ in range(3):
        dev.source_eval(species, values)
    dev.sync()
    dev.timer_begin()
    for _ in range(reps):
        dev.source_eval(species, values)
    return dev.timer_end() / reps


def field_cases(dev, mesh, sub):
    """eval_ms of the two field sources on this device: {name: {...}}"""
    from knpemidg import FieldExpression
    from knpemidg import _abi as A
    ions = ("K", "Cl", "Na")
    rng = np.random.default_rng(5)
    shape = (mesh.num_cells(), dev.nd)
    dev.upload(A.F_C_PREV, rng.uniform(1.0, 150.0, (2,) + shape))
    dev.upload(A.F_C_ELIM, rng.uniform(1.0, 150.0, shape))
    dev.upload(A.F_PHI, rng.uniform(-0.1, 0.1, shape))
    a, b = box(mesh)
    geometry = dict(g=G, k=K_WAVE, t0=-1.0, t1=1.0e9, t=0.0, a0=a[0], b0=b[0], a1=a[1], b1=b[1], a2=a[2], b2=b[2])
    cases = {"nonlinear_nf2_ecs": FieldExpression("g * c_K * exp(-phi / v0)", fields=("c_K", "phi"), subdomains=(0,), g=3.0, v0=0.025),
             "box_nf0_on_0_1": FieldExpression(CODE, subdomains=(0, 1), **geometry)}
    out = {}
    for name, e in cases.items():
        dev.source_register(1, e, ion_names=ions)
        n = int(np.isin(sub.array(), e.subdomains).sum())
        ms = timed(dev, 1, e.values())
        nbytes = n * (4 + 4 * 4 + 4 * 32 + dev.nd * 8 * (1 + len(e.fields)))      # list entry, vertex ids, coordinate rows, fields read, row written
        out[name] = {"cells": n, "eval_ms": ms, "algorithmic_bytes": nbytes, "fraction_of_hbm_peak": nbytes / (ms * 1e-3) / HBM_BYTES_PER_S,
                     "expression_evaluations_per_s": n * 125 / (ms * 1e-3)}
    dev.source_clear(1)
    return out


def run_eval(args):
    from knpemidg import _abi as A
    from knpemidg.mesh import make_mesh_3D
    from knpemidg.mms_terms import _cell_source, _geometry
    out = []
    for r in args.resolutions:
        mesh, sub, surf = make_mesh_3D(r)
        dev = A.Device(mesh, sub.array(), surf.array(), (1, 2), 3)
        expr = expression(mesh, 0.0)
        dev.source_register(0, expr)
        v = expr.values()
        ms = timed(dev, 0, v)
        n = dev.source_cells()
        nbytes = n * (4 * 4 + 4 * 32 + dev.nd * 8)        # vertex ids, gathered coordinate rows, the row written
        row = {"resolution": r, "cells": mesh.num_cells(), "ecs_cells": n, "eval_ms": ms, "algorithmic_bytes": nbytes,
               "bytes_per_s": nbytes / (ms * 1e-3), "fraction_of_hbm_peak": nbytes / (ms * 1e-3) / HBM_BYTES_PER_S,
               "expression_evaluations_per_s": n * 125 / (ms * 1e-3)}
        row["field_sources"] = field_cases(dev, mesh, sub)
        row["eval_ms_again"] = timed(dev, 0, v)            # the plain Expression once more, behind the field sources: the spread
        if r == args.host_resolution:
            # the host path as Solver._update_host_sources runs it (geometry and cell list cached, as there)
            vol, sel = _geometry(mesh)[0], np.nonzero(sub.array() == 0)[0]
            f = twin(mesh)
            times = []
            for _ in range(2):
                t0 = time.perf_counter()
                buf = np.zeros((2, mesh.num_cells(), dev.nd))
                _cell_source(mesh, vol, sel, lambda X: f(X, 0.0), buf[0], p=1)
                dev.set_source(buf)
                times.append(time.perf_counter() - t0)
            dev.source_eval(0, v)
            got = dev.source_download()[0]
            row["host_path_ms"] = 1e3 * min(times)
            row["device_vs_host_max_abs_diff_over_max"] = float(np.abs(got - buf[0]).max() / np.abs(buf[0]).max())
        print(json.dumps(row), flush=True)
        out.append(row)
        dev.close()
    return out


def run_step(args, rest):
    import idealized_common
    if args.source == "on":
        real = idealized_common.make_solver

        def make_solver(*a, **kw):
            S = real(*a, **kw)
            S.ion_list[0]['f_source'] = expression(S.mesh, 0.0)     # the window is open at every t: the value of t does not matter
            return S
        idealized_common.make_solver = make_solver
    elif args.source == "clearance":
        from knpemidg import FieldExpression
        real = idealized_common.make_solver

        def make_solver(*a, **kw):
            S = real(*a, **kw)
            c0 = float(S.ion_list[0]['c_init_sub'][0])               # the extracellular K the run starts from: clearance towards rest
            S.ion_list[0]['f_source'] = FieldExpression("-k_up * (c_K - c0)", fields=("c_K",), k_up=50.0, c0=c0)
            return S
        idealized_common.make_solver = make_solver
    import bench
    sys.argv = ["bench.py"] + rest
    bench.main()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    sub = ap.add_subparsers(dest="what", required=True)
    e = sub.add_parser("eval")
    e.add_argument("--resolutions", type=int, nargs="+", default=[1, 2])
    e.add_argument("--host-resolution", type=int, default=1)
    s = sub.add_parser("step")
    s.add_argument("--source", choices=["on", "off", "clearance"], required=True)
    args, rest = ap.parse_known_args()
    if args.what == "eval":
        run_eval(args)
    else:
        run_step(args, rest)
