"""The Stokes solve preconditioned by the exact inverse of the velocity block (`hipla.FastDiagonalizationInverse`,
`SolveInitial(pre="fdm")`) against the default `SolveInitial()` and against Jacobi, same box, same process; one grid per
call, each call under its own time limit:

    timeout -k 10 600 python tools/fdm_stokes_rate.py --dim 3 --grid 64 --out profiles/fdm_stokes_3d_n64.json
    timeout -k 10 1100 python tools/fdm_stokes_rate.py --dim 3 --grid 136 --out profiles/fdm_stokes_3d_n136.json
    timeout -k 10 600 python tools/fdm_stokes_rate.py --dim 2 --grid 577 --out profiles/fdm_stokes_2d_n577.json
    python tools/fdm_stokes_rate.py --tables profiles/fdm_stokes_*.json

(the small grids of the profile: `--skip-default --skip-jacobi`).  The last command needs no GPU: it prints the tables of
profiles/fdm_stokes.md from the JSON lines, one row per file, which is how the tables there were made; the prose around
them is written by hand.

The system is `SyntheticMesh(1 / grid, dim)`, order 0 (the plain staggered grid, whose A factors), nu = 0.01, tol 1e-8.
Recorded, for the FMA tile (`pre.tile = 0`) and the matrix-core tile (`pre.tile = 1`), `--rounds` windows each, the two
tiles interleaved, median and spread (max - min) of the windows:

  apply      `--reps` applies of y = 1.001 A^-1 x between two device events; the TFLOP/s of its 2 dim contractions
             (2 n_a flop per entry and pass), and whether the two tiles give different bits.
  iteration  a whole fused BPCG solve (`BpcgSession` + `Bpcg2Loop.run`) between two events, divided by its iterations.

Then, once each: the set-up of the preconditioner (host wall time of `FastDiagonalizationInverse(...)`: the checks of
`inverse_factors`, 3 dim symmetric eigenproblems, the upload), and the time to solution -- wall time of the whole call,
set-up included -- of `SolveInitial(pre="fdm")`, of `SolveInitial()` as it stands (MypreA, GS=True, auxiliary term; skipped
with --skip-default) and of BramblePasciakCG with the Jacobi preconditioner (skipped with --skip-jacobi).  Prints a
markdown section (also appended to --md, a file of its own) and one JSON line (also written to --out)."""
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

TILES = (("fma", 0), ("mfma", 1))
SCALE = 1.001


class Form:
    def __init__(self, mat):
        self.mat, self.condense = mat, False


def fresh(dim, grid):
    from templates.NavierStokesSIMPLE_iterative import NavierStokes, SyntheticMesh
    with contextlib.redirect_stdout(io.StringIO()):
        return NavierStokes(SyntheticMesh(1.0 / grid, dim=dim), nu=0.01, inflow="inlet", outflow="outlet", wall="wall|cyl",
                            uin=None, timestep=0.001, order=0)


def stats(values):
    return {"median": float(np.median(values)), "spread": float(np.ptp(values)), "windows": [float(v) for v in values]}


def timed(call):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    with contextlib.redirect_stdout(io.StringIO()):
        out = call()
    torch.cuda.synchronize()
    return out, time.perf_counter() - t0


def tables(paths):
    """The tables of profiles/fdm_stokes.md from the JSON lines of earlier runs, ordered by the flop of an apply."""
    runs = sorted((json.load(open(p)) for p in paths), key=lambda r: r["apply_gflop"])
    grid = lambda r: "%d-D n = %d" % (r["dim"], r["grid"])
    cell = lambda st: "%.4f (%.4f)" % (st["median"], st["spread"])
    out = ["| grid | velocity dofs | apply GFLOP | fma: apply ms (spread) | TFLOP/s | mfma: apply ms (spread) | TFLOP/s "
           "| fma / mfma |", "|---|---|---|---|---|---|---|---|"]
    for r in runs:
        a = r["apply_ms"]
        out.append("| %s | %d | %.3g | %s | %.3g | %s | %.3g | %.2f |"
                   % (grid(r), r["n_u"], r["apply_gflop"], cell(a["fma"]), r["apply_tflops"]["fma"], cell(a["mfma"]),
                      r["apply_tflops"]["mfma"], a["fma"]["median"] / a["mfma"]["median"]))
    out += ["", "| grid | iterations to %g | fma: iteration ms (spread) | mfma: iteration ms (spread) |" % runs[0]["tol"],
            "|---|---|---|---|"]
    for r in runs:
        out.append("| %s | %d | %s | %s |" % (grid(r), r["iterations"]["mfma"], cell(r["iteration_ms"]["fma"]),
                                              cell(r["iteration_ms"]["mfma"])))
    out += ["", "| grid | `SolveInitial(pre=\"fdm\")` | `SolveInitial()` | Jacobi |", "|---|---|---|---|"]
    for r in runs:
        t = r["time_to_solution_s"]
        if "default" in t and "jacobi" in t:
            out.append("| %s | %s |" % (grid(r), " | ".join(
                "%.3f s: %d iterations, loop %.3f s" % (t[k], r[k + "_iterations"], r[k + "_loop_s"])
                for k in ("fdm", "default", "jacobi"))))
    return "\n".join(out) + "\n"


def main():
    if len(sys.argv) > 2 and sys.argv[1] == "--tables":
        print(tables(sys.argv[2:]))
        return
    ap = argparse.ArgumentParser()
    ap.add_argument("--dim", type=int, default=3)
    ap.add_argument("--grid", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--tol", type=float, default=1e-8)
    ap.add_argument("--skip-default", action="store_true")
    ap.add_argument("--skip-jacobi", action="store_true")
    ap.add_argument("--jacobi-maxsteps", type=int, default=20000)
    ap.add_argument("--md", default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    from solvers.bramblepasciak_new import BpcgSession, BramblePasciakCG
    eng = hipla.get_engine()                      # (no GPU: raises -- a timing needs the device)

    ns = fresh(args.dim, args.grid)
    s = ns.system
    A, B = ns.a.mat, ns.b.mat
    result = {"dim": args.dim, "grid": args.grid, "n_u": int(s.n_u), "n_p": int(s.n_p), "tol": args.tol,
              "rounds": args.rounds, "reps": args.reps, "device": eng.device_info()["arch"]}

    pre, setup_s = timed(lambda: hipla.FastDiagonalizationInverse(A, s.component_ids))
    result["setup_s"] = setup_s
    flop = 2 * sum(2 * e * int(np.prod(f.extents)) for f in pre.factors.factors for e in f.extents)
    result["apply_gflop"] = flop / 1e9

    # ---- the apply alone ---------------------------------------------------------------------------------------------
    x = eng.from_host(np.random.default_rng(3).standard_normal(s.n_u))
    y = {name: eng.zeros(s.n_u) for name, _ in TILES}
    apply_ms = {name: [] for name, _ in TILES}
    for name, mode in TILES:                      # warm-up
        pre.tile = mode
        pre.apply_resident(x, y[name], SCALE)
    torch.cuda.synchronize()
    result["tiles_differ_in_bits"] = bool((eng.to_host(y["fma"]) != eng.to_host(y["mfma"])).any())
    result["tiles_max_rel_diff"] = float(np.abs(eng.to_host(y["fma"]) - eng.to_host(y["mfma"])).max()
                                         / np.abs(eng.to_host(y["fma"])).max())
    for _ in range(args.rounds):
        for name, mode in TILES:
            pre.tile = mode
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(args.reps):
                pre.apply_resident(x, y[name], SCALE)
            b.record()
            torch.cuda.synchronize()
            apply_ms[name].append(a.elapsed_time(b) / args.reps)
    result["apply_ms"] = {name: stats(v) for name, v in apply_ms.items()}
    result["apply_tflops"] = {name: flop / (1e-3 * np.median(v)) / 1e12 for name, v in apply_ms.items()}

    # ---- a fused solve per window ------------------------------------------------------------------------------------
    preM = hipla.Preconditioner(ns.mp, "local")
    iter_ms = {name: [] for name, _ in TILES}
    iterations = {}
    for rnd in range(args.rounds + 1):            # (the first round warms up)
        for name, mode in TILES:
            pre.tile = mode
            with contextlib.redirect_stdout(io.StringIO()):
                sol = hipla.BlockVector([hipla.Vector(s.n_u), hipla.Vector(s.n_p)])
                ses = BpcgSession(Form(A), Form(B), None, ns.f.vec, ns.g.vec, pre, preM, sol=sol)
                if ses.fused is None:
                    raise RuntimeError("the fused loop declined: %s" % ses.fused_declined)
                ses.first_direction()
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                a.record()
                it, _, converged = ses.fused.run(ses.wdn, ses.err0, args.tol, True, 500)
                b.record()
                torch.cuda.synchronize()
            if not converged:
                raise RuntimeError("the solve did not converge")
            iterations[name] = it + 1
            if rnd:
                iter_ms[name].append(a.elapsed_time(b) / (it + 1))
    result["iterations"] = iterations
    result["k"] = float(ses.k)
    result["iteration_ms"] = {name: stats(v) for name, v in iter_ms.items()}
    u, p = sol[0].numpy(), sol[1].numpy()
    f = ns.f.vec.numpy()
    result["residual"] = float(np.linalg.norm(s.A @ u + s.B.T @ p - f) / np.linalg.norm(f))

    # ---- time to solution ----------------------------------------------------------------------------------------------
    tts = {}
    twin = fresh(args.dim, args.grid)
    _, tts["fdm"] = timed(lambda: twin.SolveInitial(tol=args.tol, maxsteps=500, pre="fdm"))
    result["fdm_iterations"] = int(twin.stokes_bpcg_iterations) + 1
    result["fdm_loop_s"] = float(twin.stokes_bpcg_time)
    if not args.skip_default:
        twin = fresh(args.dim, args.grid)
        _, tts["default"] = timed(lambda: twin.SolveInitial(tol=args.tol, maxsteps=5000))
        result["default_iterations"] = int(twin.stokes_bpcg_iterations) + 1
        result["default_loop_s"] = float(twin.stokes_bpcg_time)
    if not args.skip_jacobi:
        sol = hipla.BlockVector([hipla.Vector(s.n_u), hipla.Vector(s.n_p)])

        def jacobi():
            return BramblePasciakCG(Form(A), Form(B), None, ns.f.vec, ns.g.vec, hipla.Preconditioner(A, "local"), preM, sol,
                                    tol=args.tol, maxsteps=args.jacobi_maxsteps, printrates=False)
        out, tts["jacobi"] = timed(jacobi)
        result["jacobi_iterations"] = int(out[0]) + 1
        result["jacobi_loop_s"] = float(out[1])
    result["time_to_solution_s"] = tts

    lines = ["", "### %d-D n = %d (%d velocity dofs, %d cells)" % (args.dim, args.grid, s.n_u, s.n_p), "",
             "Set-up of the preconditioner %.3f s; k = %.6f; %s iterations to %g; final residual %.2g; one apply is "
             "%.2f GFLOP; the tiles differ in bits: %s (largest difference %.2g of the largest entry)."
             % (setup_s, result["k"], " / ".join("%d (%s)" % (iterations[n], n) for n, _ in TILES), args.tol,
                result["residual"], flop / 1e9, result["tiles_differ_in_bits"], result["tiles_max_rel_diff"]), "",
             "| tile | apply ms (spread) | apply TFLOP/s | iteration ms (spread) |", "|---|---|---|---|"]
    for name, _ in TILES:
        am, im = result["apply_ms"][name], result["iteration_ms"][name]
        lines.append("| %s | %.4f (%.4f) | %.2f | %.4f (%.4f) |"
                     % (name, am["median"], am["spread"], result["apply_tflops"][name], im["median"], im["spread"]))
    lines += ["", "| time to solution | wall s | iterations | loop s |", "|---|---|---|---|"]
    for name in ("fdm", "default", "jacobi"):
        if name in tts:
            lines.append("| %s | %.3f | %d | %.3f |"
                         % (name, tts[name], result[name + "_iterations"], result[name + "_loop_s"]))
    text = "\n".join(lines) + "\n"
    print(text)
    line = json.dumps(result)
    print(line)
    if args.md:
        with open(args.md, "a") as fh:
            fh.write(text)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
