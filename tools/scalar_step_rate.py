"""Scalar transport in `Advance`: what it costs per step, what its flux kernel reaches, and the heated cavity.

    timeout -k 10 900 python tools/scalar_step_rate.py --out profiles/scalar_transport.md

(a) Per-step time of `Advance(inner_pre="jacobi")` with and without a buoyant scalar on twins of one 3-D system
    (SyntheticMesh(1/grid, dim=3), order 0 -- the plain system a scalar needs --, nu = 0.01, timestep = 0.05; force and
    start field scaled as in tools/time_step_rate.py, the buoyancy of the same size): after `--warmup` steps each,
    `--rounds` interleaved windows of `--steps` steps, wall time (host clock around a window that ends in a device
    synchronise) and device time (events), median and spread (max - min) of the windows.  Then the flux kernel
    (nss_scalar_flux_f64, buoyant form) alone: `--reps` launches between two events, against its algorithmic bytes
    (88 per face: two column pairs, two value pairs, u, f, w_b read, G and f_eff written; plus T once) and against the
    triad z = a x + y of the same run moving the same number of bytes, at `--grid` and at `--flux-grid` (operators
    alone, no NavierStokes object).
(b) The 2-D differentially heated cavity in the scaling kappa = 1: nu = Pr = 0.71, buoyancy = (0, Ra Pr), Ra = 1e3,
    T = 1 on x-, 0 on x+, t_ref = 0.5, fluid at rest at T = 0.5; n = 32 and 64, timestep 1e-3, windows of 50 steps until
    the heat entering through the hot wall changes by less than 1e-6 of itself from one window to the next.  With
    kappa = 1, a wall of length 1 and a temperature difference of 1 that heat IS the mean Nusselt number.  Literature:
    Nu = 1.118 (mean; 1.117 at the hot wall), u_max = 3.649, v_max = 3.697 -- G. de Vahl Davis, "Natural convection of
    air in a square cavity: a bench mark numerical solution", Int. J. Numer. Meth. Fluids 3 (1983) 249-264.

Writes one markdown file (--out) and prints it."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "navier-stokes-solver_amd"))

import numpy as np

import hipla

ACCELERATION = 0.02     # size of f / m_u, of the start velocity and of the buoyant acceleration
WALLS = {"x-": 1.0, "x+": 0.0}


def fresh(mesh, v0, scalar):
    from templates.NavierStokesSIMPLE_iterative import NavierStokes
    ns = NavierStokes(mesh, nu=0.01, inflow="inlet", outflow="outlet", wall="wall|cyl", uin=None, timestep=0.05, order=0)
    s = ns.system
    ns.f.vec.data = hipla.Vector.from_numpy(ACCELERATION * s.h ** s.dim * np.random.default_rng(8).standard_normal(s.n_u))
    ns.gfu.data = hipla.Vector.from_numpy(v0)
    if scalar:
        ns.AddScalar(0.01, dirichlet=WALLS, buoyancy=(0.0, 0.0, 2 * ACCELERATION), t_ref=0.5,
                     initial=np.random.default_rng(6).random(s.n_p))
    return ns


def span(iterations):
    """The iteration counts of the last window: one number, or smallest-largest."""
    if iterations is None:
        return "-"
    lo, hi = int(min(iterations)), int(max(iterations))
    return str(lo) if lo == hi else "%d-%d" % (lo, hi)


def events(torch, body, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(reps):
        body()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps          # ms per call


def flux_rate(eng, torch, st, u, reps, rounds):
    """(flux ms, triad ms, bytes): medians of `rounds` interleaved measurements; the triad moves the flux's bytes."""
    nbytes = 88 * st.n_u + 8 * st.n_p
    n = nbytes // 24
    x, y, z = eng.zeros(n), eng.zeros(n), eng.zeros(n)
    flux = lambda: st.flux(u)
    triad = lambda: eng.stream_triad(1.5, x, y, z)
    events(torch, flux, 10), events(torch, triad, 10)            # warm-up
    tf, tt = [], []
    for _ in range(rounds):
        tf.append(events(torch, flux, reps))
        tt.append(events(torch, triad, reps))
    return float(np.median(tf)), float(np.median(tt)), nbytes, float(np.ptp(tf)), float(np.ptp(tt))


def step_times(args, eng, torch, lines):
    from templates.NavierStokesSIMPLE_iterative import SyntheticMesh
    mesh = SyntheticMesh(1.0 / args.grid, dim=3)
    from staggered_grid import mac_stokes
    n_u = 3 * args.grid ** 2 * (args.grid - 1)
    v0 = ACCELERATION * np.random.default_rng(2).standard_normal(n_u)
    runs = {}
    for name in ("velocity", "scalar"):
        ns = fresh(mesh, v0, name == "scalar")
        last = {}

        def window(k, ns=ns, last=last):
            rec = ns.Advance(k)
            if rec.declined:
                raise RuntimeError("Advance declined: %s" % rec.declined)
            last["rec"] = rec
        window(args.warmup)
        eng.synchronize()
        runs[name] = dict(ns=ns, window=window, last=last, wall=[], device=[])
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
            rec = r["last"]["rec"]
            if not np.isfinite(r["ns"].gfu.numpy()).all() or max(rec.mstar_iterations) >= 500 or max(rec.proj_iterations) >= 5000:
                raise RuntimeError("not finite, or an inner solve ran into its cap: nothing to time")
    s = runs["scalar"]["ns"].system
    lines += ["## (a) Per-step time, 3-D n = %d (%d velocity dofs, %d cells), %d windows of %d steps, %s" %
              (args.grid, s.n_u, s.n_p, args.rounds, args.steps, eng.device_info()["arch"]), "",
              "| Advance | wall ms / step (spread) | device ms / step (spread) | mstar its | proj its | scalar its |",
              "|---|---|---|---|---|---|"]
    for name, r in runs.items():
        rec = r["last"]["rec"]
        lines.append("| %s | %.3f (%.3f) | %.3f (%.3f) | %s | %s | %s |" % (
            "without a scalar" if name == "velocity" else "with a buoyant scalar", np.median(r["wall"]), np.ptp(r["wall"]),
            np.median(r["device"]), np.ptp(r["device"]), span(rec.mstar_iterations), span(rec.proj_iterations),
            span(rec.scalar_iterations)))
    extra = np.median(runs["scalar"]["wall"]) - np.median(runs["velocity"]["wall"])
    lines += ["", "Difference of the medians: %+.3f ms of wall time per step with the scalar (%+.0f %%); a difference "
              "below the spread of the windows is not resolved." % (extra, 100 * extra / np.median(runs["velocity"]["wall"])), ""]
    # ---- the flux kernel alone ----
    lines += ["## (a) The flux kernel alone (nss_scalar_flux_f64, buoyant), %d launches per measurement, median of %d" %
              (args.reps, args.rounds), "",
              "| grid | faces | algorithmic MB | flux us (spread) | GB/s | triad of the same bytes us (spread) | GB/s | flux / triad rate |",
              "|---|---|---|---|---|---|---|---|"]
    stepper = runs["scalar"]["ns"]._scalar.steppers["jacobi"]
    cases = [(args.grid, stepper, runs["scalar"]["ns"]._steppers["jacobi"].u)]
    if args.flux_grid and args.flux_grid != args.grid:
        from hipla.fused import ScalarStepper
        big = mac_stokes(3, args.flux_grid, 0.01)
        ops = big.scalar_operators(0.01, WALLS)
        B = hipla.SparseMatrix.from_scipy(big.B)
        f = hipla.Vector.from_numpy(np.random.default_rng(8).standard_normal(big.n_u))
        st = ScalarStepper(eng, ops, B, f, 0.05, "jacobi", big.buoyancy_weights((0.0, 0.0, 1.0)), 0.5,
                           ops["wall_flux"]("x-"))
        eng.upload(np.random.default_rng(6).random(big.n_p), st.T)
        cases.append((args.flux_grid, st, eng.from_host(np.random.default_rng(2).standard_normal(big.n_u))))
    for grid, st, u in cases:
        tf, tt, nbytes, sf, stt = flux_rate(eng, torch, st, u, args.reps, args.rounds)
        lines.append("| %d | %d | %.1f | %.1f (%.1f) | %.0f | %.1f (%.1f) | %.0f | %.2f |" % (
            grid, st.n_u, nbytes / 1e6, 1e3 * tf, 1e3 * sf, nbytes / tf / 1e6, 1e3 * tt, 1e3 * stt, nbytes / tt / 1e6, tt / tf))
    lines.append("")


def cavity(args, eng, lines):
    from templates.NavierStokesSIMPLE_iterative import NavierStokes, SyntheticMesh
    rayleigh, prandtl, tau = 1e3, 0.71, 1e-3
    lines += ["## (b) Differentially heated cavity, Ra = 1e3, Pr = 0.71, timestep %g, donor-cell convection" % tau, "",
              "| n | steps to steady | Nu (heat through the hot wall) | literature | u_max | literature | v_max | literature | wall s |",
              "|---|---|---|---|---|---|---|---|---|"]
    for n in (32, 64):
        ns = NavierStokes(SyntheticMesh(1.0 / n, dim=2), nu=prandtl, inflow="inlet", outflow="outlet", wall="wall|cyl",
                          uin=None, timestep=tau, order=0)
        ns.f.vec.data = hipla.Vector.from_numpy(np.zeros(ns.system.n_u))
        ns.AddScalar(1.0, dirichlet=WALLS, buoyancy=(0.0, rayleigh * prandtl), t_ref=0.5)
        t0, steps, nusselt = time.perf_counter(), 0, None
        while steps < args.cavity_steps:
            rec = ns.Advance(50)
            if rec.declined:
                raise RuntimeError("Advance declined: %s" % rec.declined)
            steps += 50
            previous, nusselt = nusselt, float(rec.wall_flux[-1])
            if not np.isfinite(nusselt):
                raise RuntimeError("the cavity run is not finite")
            if previous is not None and abs(nusselt - previous) <= 1e-6 * abs(nusselt):
                break
        else:
            steps = "> %d (not steady)" % steps
        u = ns.gfu.numpy()
        comps = ns.system.component_ids
        lines.append("| %d | %s | %.4f | 1.118 | %.3f | 3.649 | %.3f | 3.697 | %.1f |" % (
            n, steps, nusselt, np.abs(u[comps[0].ravel()]).max(), np.abs(u[comps[1].ravel()]).max(), time.perf_counter() - t0))
    lines += ["", "Literature: de Vahl Davis, Int. J. Numer. Meth. Fluids 3 (1983) 249-264 (mean Nusselt number, largest "
              "horizontal velocity on the vertical mid-plane, largest vertical velocity on the horizontal mid-plane; here "
              "u_max / v_max are taken over all faces).", ""]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", type=int, default=64)
    ap.add_argument("--flux-grid", type=int, default=136)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--cavity-steps", type=int, default=3000)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    eng = hipla.get_engine()                      # (no GPU: raises -- a timing needs the device)
    lines = ["# Scalar transport in Advance: measured (tools/scalar_step_rate.py)", ""]
    step_times(args, eng, torch, lines)
    cavity(args, eng, lines)
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
