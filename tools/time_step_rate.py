"""Per-step time of the device-resident IMEX step against the statements, same box, same process:

    timeout -k 10 600 python tools/time_step_rate.py --grid 64 --out profiles/time_stepper_n64.json && \\
    timeout -k 10 1100 python tools/time_step_rate.py --grid 136 --out profiles/time_stepper_n136.json

Three runs on twins of one 3-D system (SyntheticMesh(1/grid, dim=3), order 1, nu = 0.01, timestep = 0.05; seeded force
and start field, scaled so that the explicit convection term stays stable over the run: the acceleration f / m_u and the
start velocity are both of size 0.02, |u| timestep / h below 0.3 up to grid 136 -- with an unscaled N(0, 1) force the field
overflows within eight steps and the inner solves would run on NaN): `Advance(inner_pre="jacobi")`, `Advance(inner_pre="amg")` and `DoTimeStep()` -- the statements, whose
code path this stepper does not touch.  After `--warmup` steps each, `--rounds` interleaved windows of `--steps` steps
(DoTimeStep window, jacobi window, amg window, ...): per-step wall time (host clock around a window that ends in a
device synchronise) and device time (events around the window), median and spread (max - min) of the windows, and the
inner iteration counts of the last window.  Every window checks that the velocity is finite and that no inner solve ran
into its iteration cap.  `--time-scheme cnab2` times the second-order scheme instead; `--time-scheme both` interleaves the
windows of both schemes (runs "jacobi", "amg", "DoTimeStep" and "cnab2-jacobi", "cnab2-amg", "cnab2-DoTimeStep") and adds
the ratio cnab2 / euler of every pair.  `--variable` adds the run "variable" (per scheme): `Advance(k, timesteps=[0.05] * k)`
through the variable-step stepper -- the same steps as "jacobi" with the shifted CG loop over A in the place of
M_u + timestep A, plus the rate launch -- and its ratio to "jacobi".  `--runs` keeps a subset of the runs, `--dim 2` times
the 2-D system.  Prints one markdown table and one JSON line (also written to --out).

`--cavity N` instead runs the 2-D differentially heated cavity of tools/scalar_step_rate.py (Ra = 1e3, Pr = 0.71, from
rest) on the grid N to the end time `--cavity-time`: once with the fixed step `--cavity-step`, `CflRate()` read every 50
steps, and once with `Advance(cfl=<the largest timestep * rate of the fixed run>, duration=...)`, i.e. at the CFL number
the fixed run reaches at its fastest instant; steps, wall time, and the Nusselt number and largest velocity at the end."""
import argparse
import contextlib
import io
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "navier-stokes-solver_amd"))

import numpy as np

import hipla


ACCELERATION = 0.02     # size of f / m_u and of the start velocity


def fresh(mesh, v0, time_scheme="euler"):
    from templates.NavierStokesSIMPLE_iterative import NavierStokes
    ns = NavierStokes(mesh, nu=0.01, inflow="inlet", outflow="outlet", wall="wall|cyl", uin=None, timestep=0.05, order=1,
                      time_scheme=time_scheme)
    s = ns.system
    force = ACCELERATION * s.h ** s.dim * np.random.default_rng(8).standard_normal(s.n_u)
    ns.f.vec.data = hipla.Vector.from_numpy(force)
    ns.gfu.data = hipla.Vector.from_numpy(v0)
    return ns


def check(ns, mstar_its, proj_its, caps=(500, 5000)):
    u = ns.gfu.numpy()
    if not np.isfinite(u).all():
        raise RuntimeError("the velocity is not finite: nothing to time")
    if max(mstar_its) >= caps[0] or max(proj_its) >= caps[1]:
        raise RuntimeError("an inner solve ran into its iteration cap: %s %s" % (mstar_its, proj_its))


def cavity(args):
    from templates.NavierStokesSIMPLE_iterative import NavierStokes, SyntheticMesh
    rayleigh, prandtl, tau, end = 1e3, 0.71, args.cavity_step, args.cavity_time
    eng = hipla.get_engine()

    def make():
        ns = NavierStokes(SyntheticMesh(1.0 / args.cavity, dim=2), nu=prandtl, inflow="inlet", outflow="outlet",
                          wall="wall|cyl", uin=None, timestep=tau, order=0)
        ns.f.vec.data = hipla.Vector.from_numpy(np.zeros(ns.system.n_u))
        ns.AddScalar(1.0, dirichlet={"x-": 1.0, "x+": 0.0}, buoyancy=(0.0, rayleigh * prandtl), t_ref=0.5)
        return ns

    def finish(ns, rec, t0, steps, extra):
        eng.synchronize()
        u = ns.gfu.numpy()
        if rec.declined or not np.isfinite(u).all():
            raise RuntimeError("the cavity run declined or is not finite: %s" % rec.declined)
        return dict(steps=steps, wall_s=time.perf_counter() - t0, nusselt=float(rec.wall_flux[-1]),
                    u_max=float(np.abs(u).max()), **extra)

    for ns in (make(), make()):                      # both steppers built and warm before anything is timed
        ns.Advance(2)
        ns.Advance(2, timesteps=[tau, tau])
    fixed, nsteps, rates = make(), int(round(end / tau)), []
    eng.synchronize()
    t0 = time.perf_counter()
    for _ in range(nsteps // 50):
        rec = fixed.Advance(50)
        rates.append(fixed.CflRate())
    out = {"grid": args.cavity, "end_time": end, "fixed_step": tau,
           "fixed": finish(fixed, rec, t0, 50 * (nsteps // 50), {"cfl_peak": tau * max(rates), "cfl_first": tau * rates[0]})}
    target = out["fixed"]["cfl_peak"]
    adaptive = make()
    eng.synchronize()
    t0 = time.perf_counter()
    rec = adaptive.Advance(10 * nsteps, cfl=target, max_timestep=args.cavity_max_step, duration=50 * (nsteps // 50) * tau)
    codes = {code: rec.limited_by.count(code) for code in ("max", "cfl", "growth", "end")}
    out["cfl"] = finish(adaptive, rec, t0, len(rec.timestep),
                        {"cfl_target": target, "max_timestep": args.cavity_max_step, "limited_by": codes,
                         "time": float(rec.time[-1]), "largest_step": float(rec.timestep.max()),
                         "smallest_step": float(rec.timestep.min()), "cfl_peak": float(rec.cfl.max())})
    print("| run | steps | wall s | Nu | max abs u | largest timestep * rate |\n|---|---|---|---|---|---|")
    for name in ("fixed", "cfl"):
        d = out[name]
        print("| %s | %d | %.2f | %.4f | %.3f | %.3f |" % (name, d["steps"], d["wall_s"], d["nusselt"], d["u_max"], d["cfl_peak"]))
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", type=int, default=64)
    ap.add_argument("--dim", type=int, choices=(2, 3), default=3)
    ap.add_argument("--variable", action="store_true")
    ap.add_argument("--runs", default=None, help="comma-separated subset of DoTimeStep,jacobi,amg,variable")
    ap.add_argument("--cavity", type=int, default=0)
    ap.add_argument("--cavity-step", type=float, default=1e-3)
    ap.add_argument("--cavity-time", type=float, default=0.55)
    ap.add_argument("--cavity-max-step", type=float, default=1e-2)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--time-scheme", choices=("euler", "cnab2", "both"), default="euler")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.cavity:
        return cavity(args)
    import torch
    from templates.NavierStokesSIMPLE_iterative import SyntheticMesh
    eng = hipla.get_engine()                      # (no GPU: raises -- a timing needs the device)
    mesh = SyntheticMesh(1.0 / args.grid, dim=args.dim)
    from discretizations import bdm_hybrid, system_of
    s = system_of(bdm_hybrid(1, 10)[0](mesh, velocity_dirichlet="inlet|wall|cyl")[0], 0.01)   # (cached on the mesh)
    v0 = ACCELERATION * np.random.default_rng(2).standard_normal(s.n_u)

    runs = {}
    schemes = ("euler", "cnab2") if args.time_scheme == "both" else (args.time_scheme,)
    prefix = {scheme: "cnab2-" if scheme == "cnab2" and len(schemes) == 2 else "" for scheme in schemes}
    kinds = ("DoTimeStep", "jacobi", "amg") + (("variable",) if args.variable else ())
    if args.runs:
        kinds = tuple(kind for kind in kinds if kind in args.runs.split(","))
    for scheme, kind in [(scheme, kind) for kind in kinds for scheme in schemes]:
        name = prefix[scheme] + kind
        ns = fresh(mesh, v0, scheme)
        ops = ns._time_stepping_operators() if kind == "DoTimeStep" else None
        last = {}

        def window(k, ns=ns, kind=kind, ops=ops, last=last):
            if kind == "DoTimeStep":
                ms, ps = [], []
                held, key = ns._momentum_solver()
                with contextlib.redirect_stdout(io.StringIO()):
                    for _ in range(k):
                        ns.DoTimeStep()
                        ms.append(held[key].iterations)
                        ps.append(ops["invproj"].iterations)
                last["mstar"], last["proj"] = ms, ps
            else:
                rec = ns.Advance(k, timesteps=[0.05] * k) if kind == "variable" else ns.Advance(k, inner_pre=kind)
                if rec.declined:
                    raise RuntimeError("Advance declined: %s" % rec.declined)
                last["mstar"], last["proj"] = rec.mstar_iterations.tolist(), rec.proj_iterations.tolist()
            last["ns"] = ns
        eng.synchronize()
        t0 = time.perf_counter()
        window(args.warmup)
        eng.synchronize()
        runs[name] = dict(window=window, last=last, wall=[], device=[], first_s=time.perf_counter() - t0)

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
            check(r["last"]["ns"], r["last"]["mstar"], r["last"]["proj"])      # (outside the timed window)

    result = {"grid": args.grid, "n_u": int(s.n_u), "n_p": int(s.n_p), "steps": args.steps, "rounds": args.rounds,
              "time_scheme": args.time_scheme, "device": eng.device_info()["arch"],
              "dim": args.dim, "u_max_end": float(np.abs(next(iter(runs.values()))["last"]["ns"].gfu.numpy()).max())}
    for name, r in runs.items():
        result[name] = {"wall_ms_per_step": float(np.median(r["wall"])), "wall_spread_ms": float(np.ptp(r["wall"])),
                        "device_ms_per_step": float(np.median(r["device"])), "device_spread_ms": float(np.ptp(r["device"])),
                        "wall_windows_ms": r["wall"], "device_windows_ms": r["device"],
                        "first_call_s": r["first_s"], "mstar_iterations": r["last"]["mstar"],
                        "proj_iterations": r["last"]["proj"]}
    for scheme in schemes:
        for kind, against in (("jacobi", "DoTimeStep"), ("amg", "DoTimeStep"), ("variable", "jacobi")):
            if kind in kinds and against in kinds:
                for clock in ("wall", "device"):
                    result[prefix[scheme] + kind]["%s_ratio_to_%s" % (clock, against)] = \
                        result[prefix[scheme] + kind][clock + "_ms_per_step"] / result[prefix[scheme] + against][clock + "_ms_per_step"]
    if len(schemes) == 2:
        for kind in kinds:
            for clock in ("wall", "device"):
                result["cnab2-" + kind][clock + "_ratio_to_euler"] = \
                    result["cnab2-" + kind][clock + "_ms_per_step"] / result[kind][clock + "_ms_per_step"]
    print("%d-D n=%d (%d velocity, %d pressure dofs), %d windows of %d steps" % (args.dim, args.grid, s.n_u, s.n_p, args.rounds, args.steps))
    print("| run | wall ms / step (spread) | device ms / step (spread) | mstar its | proj its |\n|---|---|---|---|---|")
    for name in runs:
        d = result[name]
        print("| %s | %.2f (%.2f) | %.2f (%.2f) | %s | %s |" % (name, d["wall_ms_per_step"], d["wall_spread_ms"],
                                                               d["device_ms_per_step"], d["device_spread_ms"],
                                                               d["mstar_iterations"], d["proj_iterations"]))
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
