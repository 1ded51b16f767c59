"""Per-step time of `NavierStokes.Advance` with the direct velocity solve (`SetImplicitSolve("fdm")`) against the
Jacobi-CG velocity solve, same box, same process:

    timeout -k 10 900 python tools/fdm_implicit_rate.py --grid 64 --out profiles/fdm_implicit_n64.json

Twins of one 3-D system (SyntheticMesh(1/grid, dim=3), order 0 -- the plain staggered grid, whose A factors -- nu = 0.01,
timestep = 0.05, seeded force and start field of size 0.02), all after `SetProjection("fdm")` and with
`inner_pre="jacobi"`: for "euler" and "cnab2", fixed steps and `cfl=` steps, the default "cg" velocity solve (at its 1e-4)
and "fdm".  With `--reference`: also the order 1 system of tools/fdm_projection_rate.py with "cg" (its A does not
factor).  After `--warmup` steps each, `--rounds` interleaved windows of `--steps` steps: per-step wall time (host clock
around a window that ends in a device synchronise) and device time (events around the window), median and spread
(max - min) of the windows.  Then one more window per run with device events around every velocity solve (for CG: the
launches and the polls), summed per step.  `--trace RUN` does nothing but two warm-up steps and `--steps` steps of one
run, for a kernel trace.  Prints a markdown table and one JSON line (also written to --out)."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "navier-stokes-solver_amd"))

import numpy as np

import hipla

from time_step_rate import ACCELERATION

RUNS = {"%s-%s-%s" % (scheme, mode, implicit): (scheme, mode, implicit, 0)
        for scheme in ("euler", "cnab2") for mode in ("fixed", "cfl") for implicit in ("cg", "fdm")}
REFERENCE = {"order1-euler-fixed-cg": ("euler", "fixed", "cg", 1)}
CFL = 0.5


def fresh(grid, scheme, implicit, order):
    from templates.NavierStokesSIMPLE_iterative import NavierStokes, SyntheticMesh
    ns = NavierStokes(SyntheticMesh(1.0 / grid, dim=3), nu=0.01, inflow="inlet", outflow="outlet", wall="wall|cyl", uin=None,
                      timestep=0.05, order=order, time_scheme=scheme)
    s = ns.system
    n_u = ns.gfu.numpy().size
    ns.f.vec.data = hipla.Vector.from_numpy(ACCELERATION * s.h ** s.dim * np.random.default_rng(8).standard_normal(n_u))
    ns.gfu.data = hipla.Vector.from_numpy(ACCELERATION * np.random.default_rng(2).standard_normal(n_u))
    ns.SetProjection("fdm")
    t0 = time.perf_counter()
    ns.SetImplicitSolve(implicit)
    return ns, time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", type=int, default=64)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reference", action="store_true")
    ap.add_argument("--trace", default=None, help="one run of " + ",".join(RUNS))
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    eng = hipla.get_engine()                      # (no GPU: raises -- a timing needs the device)
    table = dict(RUNS, **(REFERENCE if args.reference else {}))
    if args.trace:
        table = {args.trace: table[args.trace]}

    runs = {}
    for name, (scheme, mode, implicit, order) in table.items():
        ns, factor_s = fresh(args.grid, scheme, implicit, order)
        last = {}

        def window(k, ns=ns, mode=mode, last=last):
            rec = ns.Advance(k, **(dict(cfl=CFL) if mode == "cfl" else {}))
            if rec.declined:
                raise RuntimeError("Advance declined: %s" % rec.declined)
            if not np.isfinite(rec.kinetic_energy).all() or max(rec.mstar_iterations) >= 500:
                raise RuntimeError("the run diverged or the velocity solve ran into its cap")
            last["rec"] = rec
        window(args.warmup)
        eng.synchronize()
        if last["rec"].implicit != implicit or last["rec"].projection != "fdm":
            raise RuntimeError("%s ran %s / %s" % (name, last["rec"].implicit, last["rec"].projection))
        runs[name] = dict(window=window, last=last, wall=[], device=[], factor_s=factor_s, ns=ns)
    if args.trace:
        runs[args.trace]["window"](args.steps)
        eng.synchronize()
        return

    for _ in range(args.rounds):                   # interleaved windows
        for r in runs.values():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            a.record()
            r["window"](args.steps)
            b.record()
            torch.cuda.synchronize()
            r["wall"].append(1e3 * (time.perf_counter() - t0) / args.steps)
            r["device"].append(a.elapsed_time(b) / args.steps)

    for r in runs.values():                        # the velocity solve alone: events around every one of a window
        stepper = next(iter(r["ns"]._steppers.values()))
        solver = stepper.fdm_u if stepper.fdm_u is not None else stepper.cg_m
        pairs, inner = [], solver.solve_resident

        def solve(*a, pairs=pairs, inner=inner, **kw):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            out = inner(*a, **kw)
            e1.record()
            pairs.append((e0, e1))
            return out
        solver.solve_resident = solve
        try:
            r["window"](args.steps)
            torch.cuda.synchronize()
        finally:
            del solver.solve_resident
        r["solve_ms"] = sum(e0.elapsed_time(e1) for e0, e1 in pairs) / args.steps

    result = {"grid": args.grid, "steps": args.steps, "rounds": args.rounds, "device": eng.device_info()["arch"]}
    print("3-D n=%d, %d windows of %d steps, SetProjection(\"fdm\"), inner_pre=\"jacobi\"" % (args.grid, args.rounds, args.steps))
    print("| run | velocity dofs | wall ms / step (spread) | device ms / step (spread) | velocity solve device ms / step | mstar its |")
    print("|---|---|---|---|---|---|")
    for name, r in runs.items():
        rec = r["last"]["rec"]
        d = result[name] = {"n_u": int(r["ns"].gfu.numpy().size), "wall_ms_per_step": float(np.median(r["wall"])),
                            "wall_spread_ms": float(np.ptp(r["wall"])), "device_ms_per_step": float(np.median(r["device"])),
                            "device_spread_ms": float(np.ptp(r["device"])), "wall_windows_ms": r["wall"],
                            "device_windows_ms": r["device"], "velocity_solve_device_ms_per_step": r["solve_ms"],
                            "set_implicit_solve_s": r["factor_s"], "mstar_iterations": rec.mstar_iterations.tolist(),
                            "timestep": None if rec.timestep is None else np.asarray(rec.timestep).tolist()}
        print("| %s | %d | %.3f (%.3f) | %.3f (%.3f) | %.3f | %s |"
              % (name, d["n_u"], d["wall_ms_per_step"], d["wall_spread_ms"], d["device_ms_per_step"], d["device_spread_ms"],
                 d["velocity_solve_device_ms_per_step"], d["mstar_iterations"]))
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
