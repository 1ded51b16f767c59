"""Per-step time of `NavierStokes.Advance` with the direct pressure projection (`SetProjection("fdm")`) against the CG
projections, same box, same process:

    timeout -k 10 900 python tools/fdm_projection_rate.py --grid 64 --out profiles/fdm_projection_n64.json

Four runs on twins of one 3-D system (the set-up of tools/time_step_rate.py: SyntheticMesh(1/grid, dim=3), order 1,
nu = 0.01, timestep = 0.05, seeded force and start field of size 0.02): `Advance(inner_pre="jacobi")` and
`Advance(inner_pre="amg")` -- the CG projections, whose code path this change does not touch -- and the same two after
`SetProjection("fdm")` ("fdm-jacobi", "fdm-amg").  After `--warmup` steps each, `--rounds` interleaved windows of
`--steps` steps: per-step wall time (host clock around a window that ends in a device synchronise) and device time
(events around the window), median and spread (max - min) of the windows, and the inner iteration counts of the last
window.  Then one more window per run with device events around every `project()` of the stepper (launches and, for CG,
the polls of the solve): the projection's own device time per step.  Then every one of the 2 d passes of the solve on
its own, `nss_fdm_contract_f64` on the pass's shape: the median of `--rounds` windows of 20 launches, as GB/s against
the 16 bytes per cell a pass has to move and GFlop/s against the fp64 vector peak, and the ratio of the pass to its
byte time at the measured HBM copy rate.  Prints markdown tables and one JSON line (also written to --out)."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "navier-stokes-solver_amd"))

import numpy as np

import hipla

from time_step_rate import ACCELERATION, check, fresh

FP64_VECTOR_PEAK = 78.6e12      # flop/s, data sheet
HBM_COPY_RATE = 6.29e12         # bytes/s, measured float4 copy
RUNS = {"jacobi": ("jacobi", "cg"), "amg": ("amg", "cg"), "fdm-jacobi": ("jacobi", "fdm"), "fdm-amg": ("amg", "fdm")}


def pass_shapes(extents):
    """(outer, n, inner, transpose) of the 2 d passes of a solve, in its order."""
    d, out = len(extents), []
    for k in range(2 * d):
        a = k % d
        out.append((int(np.prod(extents[:a], dtype=np.int64)), int(extents[a]),
                    int(np.prod(extents[a + 1:], dtype=np.int64)), int(k < d)))
    return out


def time_passes(eng, torch, extents, rounds, launches=20):
    cells = int(np.prod(extents, dtype=np.int64))
    rng = np.random.default_rng(0)
    x, y = eng.from_host(rng.standard_normal(cells)), eng.zeros(cells)
    rows = []
    for outer, n, inner, transpose in pass_shapes(extents):
        m = eng.from_host(rng.standard_normal(n * n))

        def launch():
            eng._check(eng.lib.nss_fdm_contract_f64(outer, n, inner, m.data_ptr(), transpose, x.data_ptr(), y.data_ptr(),
                                                    eng.stream))
        for _ in range(3):
            launch()
        times = []
        for _ in range(rounds):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            a.record()
            for _ in range(launches):
                launch()
            b.record()
            torch.cuda.synchronize()
            times.append(1e-3 * a.elapsed_time(b) / launches)
        t = float(np.median(times))
        nbytes, flops = 16.0 * cells, 2.0 * n * cells
        rows.append({"outer": outer, "n": n, "inner": inner, "transpose": transpose, "us": 1e6 * t,
                     "spread_us": 1e6 * float(np.ptp(times)), "gb_per_s": 1e-9 * nbytes / t,
                     "gflop_per_s": 1e-9 * flops / t, "share_of_fp64_vector_peak": flops / t / FP64_VECTOR_PEAK,
                     "ratio_to_byte_time": t / (nbytes / HBM_COPY_RATE)})
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", type=int, default=64)
    ap.add_argument("--dim", type=int, choices=(2, 3), default=3)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--runs", default=None, help="comma-separated subset of " + ",".join(RUNS))
    ap.add_argument("--passes-only", action="store_true", help="time the 2 d passes on the grid and nothing else")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    if args.passes_only:
        eng = hipla.get_engine()
        result = {"grid": args.grid, "dim": args.dim, "rounds": args.rounds, "device": eng.device_info()["arch"],
                  "passes": time_passes(eng, torch, (args.grid,) * args.dim, args.rounds)}
        print_passes(result["passes"])
        return finish(result, args.out)
    from discretizations import bdm_hybrid, system_of
    from templates.NavierStokesSIMPLE_iterative import SyntheticMesh
    eng = hipla.get_engine()                      # (no GPU: raises -- a timing needs the device)
    mesh = SyntheticMesh(1.0 / args.grid, dim=args.dim)
    s = system_of(bdm_hybrid(1, 10)[0](mesh, velocity_dirichlet="inlet|wall|cyl")[0], 0.01)   # (cached on the mesh)
    v0 = ACCELERATION * np.random.default_rng(2).standard_normal(s.n_u)

    runs = {}
    for name in (args.runs.split(",") if args.runs else RUNS):
        inner_pre, projection = RUNS[name]
        ns = fresh(mesh, v0)
        t0 = time.perf_counter()
        if projection == "fdm":
            ns.SetProjection("fdm")
        factor_s = time.perf_counter() - t0
        last = {}

        def window(k, ns=ns, inner_pre=inner_pre, last=last):
            rec = ns.Advance(k, inner_pre=inner_pre)
            if rec.declined:
                raise RuntimeError("Advance declined: %s" % rec.declined)
            last["mstar"], last["proj"], last["ns"], last["rec"] = \
                rec.mstar_iterations.tolist(), rec.proj_iterations.tolist(), ns, rec
        eng.synchronize()
        t0 = time.perf_counter()
        window(args.warmup)
        eng.synchronize()
        if last["rec"].projection != projection:
            raise RuntimeError("%s ran the projection %s" % (name, last["rec"].projection))
        runs[name] = dict(window=window, last=last, wall=[], device=[], first_s=time.perf_counter() - t0,
                          factor_s=factor_s, ns=ns)

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

    for r in runs.values():                        # the projection alone: events around every project() of one window
        stepper = next(iter(r["ns"]._steppers.values()))
        pairs, inner = [], stepper.project

        def project(*a, pairs=pairs, inner=inner, **kw):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            out = inner(*a, **kw)
            e1.record()
            pairs.append((e0, e1))
            return out
        stepper.project = project
        try:
            r["window"](args.steps)
            torch.cuda.synchronize()
        finally:
            del stepper.project
        r["project_ms"] = sum(e0.elapsed_time(e1) for e0, e1 in pairs) / args.steps

    result = {"grid": args.grid, "dim": args.dim, "n_u": int(s.n_u), "n_p": int(s.n_p), "steps": args.steps,
              "rounds": args.rounds, "device": eng.device_info()["arch"]}
    for name, r in runs.items():
        result[name] = {"wall_ms_per_step": float(np.median(r["wall"])), "wall_spread_ms": float(np.ptp(r["wall"])),
                        "device_ms_per_step": float(np.median(r["device"])), "device_spread_ms": float(np.ptp(r["device"])),
                        "wall_windows_ms": r["wall"], "device_windows_ms": r["device"],
                        "project_device_ms_per_step": r["project_ms"], "first_call_s": r["first_s"],
                        "set_projection_s": r["factor_s"], "mstar_iterations": r["last"]["mstar"],
                        "proj_iterations": r["last"]["proj"]}
    result["passes"] = time_passes(eng, torch, (args.grid,) * args.dim, args.rounds)
    print("%d-D n=%d (%d velocity, %d pressure dofs), %d windows of %d steps"
          % (args.dim, args.grid, s.n_u, s.n_p, args.rounds, args.steps))
    print("| run | wall ms / step (spread) | device ms / step (spread) | project() device ms / step | mstar its | proj its |")
    print("|---|---|---|---|---|---|")
    for name in runs:
        d = result[name]
        print("| %s | %.2f (%.2f) | %.2f (%.2f) | %.3f | %s | %s |"
              % (name, d["wall_ms_per_step"], d["wall_spread_ms"], d["device_ms_per_step"], d["device_spread_ms"],
                 d["project_device_ms_per_step"], d["mstar_iterations"], d["proj_iterations"]))
    print_passes(result["passes"])
    finish(result, args.out)


def print_passes(passes):
    print("| pass (outer, n, inner) | transpose | us (spread) | GB/s | GFlop/s | of fp64 vector peak | pass / byte time |")
    print("|---|---|---|---|---|---|---|")
    for p in passes:
        print("| (%d, %d, %d) | %d | %.1f (%.1f) | %.0f | %.0f | %.1f %% | %.1f |"
              % (p["outer"], p["n"], p["inner"], p["transpose"], p["us"], p["spread_us"], p["gb_per_s"], p["gflop_per_s"],
                 100 * p["share_of_fp64_vector_peak"], p["ratio_to_byte_time"]))


def finish(result, out):
    line = json.dumps(result)
    print(line)
    if out:
        with open(out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
