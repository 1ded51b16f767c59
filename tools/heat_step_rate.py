"""Per-step time of `heat.evolve` on the device-resident path against its protocol path, same box, same process:

    timeout -k 10 900 python tools/heat_step_rate.py --grid 1024 --out profiles/heat_integrator_n1024.json

Both paths run the same statements on the same engine; the protocol path is forced through ``hipla.fused.ENABLED = False``
(``record.declined`` must say so), which also sends its inner solves through the protocol CG.  A window is one `evolve`
call of `--steps` steps from the reference's seven modes; the time of a step is taken between the `on_step` callbacks
(each after a device synchronise), so the set-up of a call (matrix upload, preconditioner) is not in it.  After one
warm-up window each, `--rounds` interleaved windows (device, protocol, device, ...): median and spread (max - min) of
the windows' per-step times.  Alongside: launch counts and algorithmic bytes of the orthonormalisation and of the two
Galerkin calls on both paths.  Prints one markdown table and one JSON line (also to --out)."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "navier-stokes-solver_amd"))

import numpy as np

import hipla

KL = [(1, 1), (2, 1), (1, 3), (3, 3), (2, 3), (4, 5), (5, 2)]


def traffic(n_rows, nnz, d=5, tries=3):
    """Launches and algorithmic bytes per step of the orthonormalisation and the two Galerkin calls."""
    pairs = d * (d - 1) // 2
    device_mgs = tries * (16 * (d - 1) + 32 * (pairs - (d - 1)) + 8 + 24 * (d - 1) + 16 * d) * n_rows
    protocol_mgs = tries * (pairs * 56 + d * 32) * n_rows
    matrix = 12 * nnz + 4 * (n_rows + 1)
    diag = 12 * n_rows + 4 * (n_rows + 1)
    return {
        "device": {"mgs_launches": tries * (pairs + 2 * d), "mgs_bytes": device_mgs, "galerkin_launches": 4,
                   "galerkin_bytes": matrix + diag + 2 * 8 * d * n_rows, "host_reads": 1},
        "protocol": {"mgs_launches": tries * (3 * pairs + 2 * d), "mgs_bytes": protocol_mgs,
                     "galerkin_launches": 2 * d + 2 * d * d,
                     "galerkin_bytes": d * (matrix + diag + 4 * 8 * n_rows) + 2 * d * d * 16 * n_rows,
                     "host_reads": tries * (2 * pairs + d) + 2 * d * d + 1},
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--time-step", type=float, default=1e-3)
    ap.add_argument("--inner-pre", default="jacobi")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import heat
    from hipla import fused
    from staggered_grid import diffusion_operators_2d
    eng = hipla.get_engine()                      # (no GPU: raises -- a timing needs the device)
    n = args.grid
    start = heat.sum_of_unit_square_laplace_eigenfunctions(KL, n)
    operators = diffusion_operators_2d(n)
    end_time = (args.steps - 0.5) * args.time_step

    def window(device):
        stamps = []

        def on_step(step):
            torch.cuda.synchronize()
            stamps.append(time.perf_counter())
        fused.ENABLED = device
        try:
            temperature, _, record = heat.evolve(start, end_time, args.time_step, n=n, inner_pre=args.inner_pre,
                                                 operators=operators, on_step=on_step)
        finally:
            fused.ENABLED = True
        if (record.declined is None) != device or record.steps != args.steps:
            raise RuntimeError("wrong path or step count: declined=%r steps=%d" % (record.declined, record.steps))
        if not np.isfinite(temperature).all():
            raise RuntimeError("the temperature is not finite: nothing to time")
        return 1e3 * (stamps[-1] - stamps[0]) / (args.steps - 1), record.cg_iterations.tolist(), temperature

    runs = {"device": dict(ms=[]), "protocol": dict(ms=[])}
    for name, r in runs.items():
        _, r["its"], r["temperature"] = window(name == "device")          # warm-up window
    for _ in range(args.rounds):
        for name, r in runs.items():
            ms, r["its"], _ = window(name == "device")
            r["ms"].append(ms)
    diff = float(np.linalg.norm(runs["device"]["temperature"] - runs["protocol"]["temperature"])
                 / np.linalg.norm(runs["protocol"]["temperature"]))
    result = {"grid": n, "rows": n * n, "nnz": int(operators[0].nnz), "steps": args.steps, "rounds": args.rounds,
              "time_step": args.time_step, "inner_pre": args.inner_pre, "device_name": eng.device_info()["arch"],
              "relative_difference_of_the_paths": diff, "traffic": traffic(n * n, int(operators[0].nnz))}
    for name, r in runs.items():
        result[name] = {"ms_per_step": float(np.median(r["ms"])), "spread_ms": float(np.ptp(r["ms"])),
                        "windows_ms": r["ms"], "cg_iterations": r["its"]}
    result["ratio_device_to_protocol"] = result["device"]["ms_per_step"] / result["protocol"]["ms_per_step"]
    print("n = %d (%d rows), time step %g, %s CG, %d windows of %d steps" % (n, n * n, args.time_step, args.inner_pre,
                                                                        args.rounds, args.steps))
    print("| path | ms / step (spread) | CG iterations of the last step |\n|---|---|---|")
    for name in runs:
        print("| %s | %.2f (%.2f) | %s |" % (name, result[name]["ms_per_step"], result[name]["spread_ms"],
                                             result[name]["cg_iterations"][-1]))
    print("ratio device / protocol: %.3f; relative difference of the results: %.2e" % (result["ratio_device_to_protocol"],
                                                                                 diff))
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
