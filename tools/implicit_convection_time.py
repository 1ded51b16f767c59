"""Linearly implicit convection (`SetConvectionTreatment("implicit")`) against the explicit step, same box, same process:

    timeout -k 10 900 python tools/implicit_convection_time.py --grid 64 --out profiles/implicit_convection_n64.json

One 3-D system (SyntheticMesh(1/grid, dim=3), order 0, nu = 0.01, seeded force and start field of size 0.02, as
tools/fdm_implicit_rate.py), all after `SetProjection("fdm")`, `Advance(cfl=)` with `max_timestep` out of the way.  Runs:
the explicit step at cfl = 0.4 with the "cg" and the "fdm" velocity solve (the baseline: the default path, which the
feature leaves launch for launch what it was), and the implicit step at cfl = 4 and 16 with both preconditioners
(`SetImplicitSolve("cg")`: point Jacobi of the whole operator; "fdm": the direct viscous inverse).

1. Per step: after `--warmup` steps, `--rounds` interleaved windows of `--steps` steps from the state the run has reached;
   device time (events around the window) and wall time (host clock around a window that ends in a synchronise) per
   step, median and spread (max - min) of the windows, the BiCGStab / CG iterations and the step sizes of the last window.
2. To a fixed physical time: every run again from the start field, `Advance(cfl=, duration=--time)`, wall clock around
   the call (it ends in the read-back of the record), `--repeats` times, median; steps taken.
3. `--cavity`: the heated 2-D cavity of profiles/cnab2_stepping.md section 2 (n = 12, walls x- at 1 and x+ at 0, kappa =
   0.02, buoyancy (0, 20), t_ref = 0.5, from rest): 200 fixed steps at each tau of a ladder, "bounded" = finite with |u|,
   |T| <= 10 throughout (checked every 20 steps and at the end); the largest bounded tau and tau * CflRate of the final flow.

Prints markdown tables and one JSON line (also written to --out)."""
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

RUNS = {"explicit-cfl0.4-cg": ("explicit", 0.4, "cg"), "explicit-cfl0.4-fdm": ("explicit", 0.4, "fdm"),
        "implicit-cfl4-jacobi": ("implicit", 4.0, "cg"), "implicit-cfl4-fdm": ("implicit", 4.0, "fdm"),
        "implicit-cfl16-jacobi": ("implicit", 16.0, "cg"), "implicit-cfl16-fdm": ("implicit", 16.0, "fdm")}
FREE = 1e6                                          # max_timestep: the controller alone chooses the step


def fresh(grid, treatment, implicit):
    from templates.NavierStokesSIMPLE_iterative import NavierStokes, SyntheticMesh
    ns = NavierStokes(SyntheticMesh(1.0 / grid, dim=3), nu=0.01, inflow="inlet", outflow="outlet", wall="wall|cyl", uin=None,
                      timestep=0.05, order=0)
    s = ns.system
    ns.f.vec.data = hipla.Vector.from_numpy(ACCELERATION * s.h ** s.dim * np.random.default_rng(8).standard_normal(s.n_u))
    start = hipla.Vector.from_numpy(ACCELERATION * np.random.default_rng(2).standard_normal(s.n_u))
    ns.gfu.data = start
    ns.SetProjection("fdm")
    ns.SetImplicitSolve(implicit)
    ns.SetConvectionTreatment(treatment)
    return ns, start


def advance(ns, steps, cfl, **kw):
    rec = ns.Advance(steps, cfl=cfl, max_timestep=FREE, **kw)
    if rec.declined:
        raise RuntimeError("Advance declined: %s" % rec.declined)
    if not np.isfinite(rec.kinetic_energy).all() or (len(rec.mstar_iterations) and max(rec.mstar_iterations) >= 500):
        raise RuntimeError("the run diverged or the velocity solve ran into its cap")
    return rec


def cavity(taus):
    """200 steps of the heated cavity at every tau, explicit and implicit: {treatment: [(tau, bounded, tau * rate)]}."""
    from templates.NavierStokesSIMPLE_iterative import NavierStokes, SyntheticMesh
    out = {}
    for treatment in ("explicit", "implicit"):
        rows = []
        for tau in taus:
            ns = NavierStokes(SyntheticMesh(1.0 / 12, dim=2), nu=0.01, inflow="inlet", outflow="outlet", wall="wall|cyl",
                              uin=None, timestep=tau, order=0)
            ns.f.vec.data = hipla.Vector.from_numpy(np.zeros(ns.system.n_u))
            ns.AddScalar(kappa=0.02, dirichlet={"x-": 1.0, "x+": 0.0}, buoyancy=(0.0, 20.0), t_ref=0.5)
            ns.SetConvectionTreatment(treatment)
            bounded, its = True, []
            try:
                for _ in range(10):
                    rec = ns.Advance(20)
                    its += list(rec.mstar_iterations)
                    u, T = ns.gfu.numpy(), ns.temperature.numpy()
                    if not (np.isfinite(u).all() and np.isfinite(T).all() and abs(u).max() <= 10 and abs(T).max() <= 10):
                        bounded = False
                        break
            except FloatingPointError:
                bounded = False
            rows.append(dict(tau=tau, bounded=bounded, cell_number=tau * ns.CflRate() if bounded else None,
                             max_iterations=int(max(its)) if its else None))
            if treatment == "explicit" and not bounded:
                break
        out[treatment] = rows
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", type=int, default=64)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--time", type=float, default=2.0, help="the physical time of part 2")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--cavity", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    eng = hipla.get_engine()                      # (no GPU: raises -- a timing needs the device)
    result = {"grid": args.grid, "steps": args.steps, "rounds": args.rounds, "time": args.time,
              "device": eng.device_info()["arch"]}

    runs = {}
    for name, (treatment, cfl, implicit) in RUNS.items():
        ns, start = fresh(args.grid, treatment, implicit)
        rec = advance(ns, args.warmup, cfl)
        eng.synchronize()
        if rec.convection_treatment != treatment or rec.implicit != implicit:
            raise RuntimeError("%s ran %s / %s" % (name, rec.convection_treatment, rec.implicit))
        runs[name] = dict(ns=ns, start=start, cfl=cfl, wall=[], device=[], rec=rec)

    for _ in range(args.rounds):                   # 1. interleaved windows
        for r in runs.values():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            a.record()
            r["rec"] = advance(r["ns"], args.steps, r["cfl"])
            b.record()
            torch.cuda.synchronize()
            r["wall"].append(1e3 * (time.perf_counter() - t0) / args.steps)
            r["device"].append(a.elapsed_time(b) / args.steps)

    for r in runs.values():                        # 2. to a fixed physical time, from the start field
        r["to_time"], ns = [], r["ns"]
        for _ in range(args.repeats):
            ns.gfu.data = r["start"]
            ns.gfup.data = hipla.Vector.from_numpy(np.zeros(ns.system.n_p))
            ns._clock.tau_prev = None
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            rec = advance(ns, 100000, r["cfl"], duration=args.time)
            torch.cuda.synchronize()
            r["to_time"].append(time.perf_counter() - t0)
        r["to_time_rec"] = rec

    print("3-D n=%d, SetProjection(\"fdm\"), %d windows of %d steps; wall time to t = %g, median of %d"
          % (args.grid, args.rounds, args.steps, args.time, args.repeats))
    print("| run | device ms / step (spread) | wall ms / step (spread) | iterations / step | tau of the last window "
          "| steps to t | wall ms to t | iterations to t |")
    print("|---|---|---|---|---|---|---|---|")
    for name, r in runs.items():
        rec, full = r["rec"], r["to_time_rec"]
        d = result[name] = {"device_ms_per_step": float(np.median(r["device"])), "device_spread_ms": float(np.ptp(r["device"])),
                            "wall_ms_per_step": float(np.median(r["wall"])), "wall_spread_ms": float(np.ptp(r["wall"])),
                            "device_windows_ms": r["device"], "wall_windows_ms": r["wall"],
                            "mstar_iterations": rec.mstar_iterations.tolist(), "timestep": np.asarray(rec.timestep).tolist(),
                            "cfl": np.asarray(rec.cfl).tolist(), "steps_to_time": int(len(full.mstar_iterations)),
                            "wall_ms_to_time": 1e3 * float(np.median(r["to_time"])),
                            "wall_ms_to_time_all": [1e3 * t for t in r["to_time"]],
                            "iterations_to_time": int(full.mstar_iterations.sum()),
                            "kinetic_energy_at_time": float(full.kinetic_energy[-1])}
        print("| %s | %.3f (%.3f) | %.3f (%.3f) | %.1f | %.4f | %d | %.1f | %d |"
              % (name, d["device_ms_per_step"], d["device_spread_ms"], d["wall_ms_per_step"], d["wall_spread_ms"],
                 np.mean(d["mstar_iterations"]), d["timestep"][-1], d["steps_to_time"], d["wall_ms_to_time"],
                 d["iterations_to_time"]))

    if args.cavity:                                # 3. the heated cavity
        ladder = [0.1, 0.1495, 0.16, 0.3, 0.6, 1.2, 2.5, 5.0, 10.0, 25.0, 50.0]
        result["cavity"] = cavity(ladder)
        print("heated 2-D cavity, n = 12, 200 steps: | treatment | tau | bounded | tau * CflRate at the end | most iterations |")
        for treatment, rows in result["cavity"].items():
            for row in rows:
                print("| %s | %g | %s | %s | %s |" % (treatment, row["tau"], row["bounded"],
                                                      "-" if row["cell_number"] is None else "%.1f" % row["cell_number"],
                                                      row["max_iterations"]))
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
