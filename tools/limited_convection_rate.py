"""Second-order limited convection: what its two flux kernels cost beside their donor-cell twins, what a step of
`Advance` costs per scheme, and what the scheme buys on the heated cavity.

    timeout -k 10 1100 python tools/limited_convection_rate.py --out profiles/limited_convection.md

(a) The flux kernels alone on the operators of one 3-D grid (`--grid`, no NavierStokes object): F1-limited
    (nss_step_flux_limited_f64; donor, minmod, van Leer) and nss_step_flux_f64 of the same library, then S1-limited
    (nss_scalar_flux_limited_f64, buoyant) and nss_scalar_flux_f64, each followed by its extrapolating export
    (nss_*_ab2_f64: the same kernel with the extrapolating output policy) at the weights (1, 0), which does not read the
    history, and (3/2, -1/2), alternated in `--rounds` rounds of `--reps` launches between two events each: median and
    spread (max - min) of the rounds, against the algorithmic bytes (48 / 80 per flux point plus u once; 56 / 88 per
    face plus T once; extrapolating + 8 per history written and + 8 per history read).
(b) Per-step time of `Advance(inner_pre="jacobi")` for "upwind", "minmod", "vanleer" on twins of one 3-D system set up
    as in tools/scalar_step_rate.py: after `--warmup` steps each, `--rounds` interleaved windows of `--steps` steps,
    wall and device time, median and spread of the windows.
(c) The 2-D differentially heated cavity of tools/scalar_step_rate.py (kappa = 1, nu = Pr = 0.71, buoyancy =
    (0, Ra Pr), T = 1 on x-, 0 on x+) with "vanleer" beside "upwind" for velocity and scalar: Ra = 1e3 on n = 32 and
    64, and Ra = 1e5 on n = 64, windows of steps until the heat through the hot wall changes by less than 1e-6 of
    itself between windows, or `--cavity-seconds` have passed.  The timestep keeps timestep * sum_faces |u_f| / h below
    1/2 for the literature's velocities.  Literature: Nu = 1.118 (Ra = 1e3), 4.519 (Ra = 1e5) -- G. de Vahl Davis,
    Int. J. Numer. Meth. Fluids 3 (1983) 249-264.

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
SCHEMES = ("upwind", "minmod", "vanleer")


def events(torch, body, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(reps):
        body()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps          # ms per call


def alternate(torch, bodies, reps, rounds):
    """{name: (median ms, spread ms)} of `rounds` rounds in which every body is measured once, in turn."""
    for body in bodies.values():
        events(torch, body, 10)                # warm-up (the two-slot copies are built on the first call)
    times = {name: [] for name in bodies}
    for _ in range(rounds):
        for name, body in bodies.items():
            times[name].append(events(torch, body, reps))
    return {name: (float(np.median(t)), float(np.ptp(t))) for name, t in times.items()}


def kernels(args, eng, torch, lines):
    from hipla.fused import upload_stencil
    from staggered_grid import mac_stokes
    s = mac_stokes(3, args.grid, 0.01)
    lib = eng.lib
    ops = s.convection_operators()
    adv, avg, dif = (hipla.SparseMatrix.from_scipy(ops[k]) for k in ("adv", "avg", "diff"))
    nflux = ops["adv"].shape[0]
    stencil = upload_stencil(eng, s.convection_stencil(), s.n_u)
    uf = eng.from_host(np.concatenate([np.random.default_rng(2).standard_normal(s.n_u), np.zeros(nflux)]))
    flux = eng.view(uf, s.n_u, s.n_u + nflux)

    prev = eng.zeros(nflux)
    weights = {"(1, 0)": (1.0, 0.0), "(3/2, -1/2)": (1.5, -0.5)}
    limiters = ("donor", "minmod", "van Leer")

    def limited(code):
        return lambda: eng._check(lib.nss_step_flux_limited_f64(adv.handle.ptr, stencil.data_ptr(), nflux, code,
                                                                uf.data_ptr(), flux.data_ptr(), None, eng.stream))

    def donor_ab2(w):
        return lambda: eng._check(lib.nss_step_flux_ab2_f64(adv.handle.ptr, avg.handle.ptr, dif.handle.ptr, uf.data_ptr(),
                                                            w[0], w[1], prev.data_ptr(), flux.data_ptr(), None, eng.stream))

    def limited_ab2(code, w):
        return lambda: eng._check(lib.nss_step_flux_limited_ab2_f64(adv.handle.ptr, stencil.data_ptr(), nflux, code,
                                                                    uf.data_ptr(), w[0], w[1], prev.data_ptr(),
                                                                    flux.data_ptr(), None, eng.stream))
    bodies, per = {}, {}                           # name -> launch, name -> algorithmic bytes per point

    def add(name, nbytes, body, unit="point"):
        name = "%s (%d B / %s)" % (name, nbytes, unit)
        bodies[name], per[name] = body, nbytes
    add("nss_step_flux_f64", 80, lambda: eng._check(lib.nss_step_flux_f64(
        adv.handle.ptr, avg.handle.ptr, dif.handle.ptr, uf.data_ptr(), flux.data_ptr(), None, eng.stream)))
    for code, name in enumerate(limiters):
        add("limited, %s" % name, 48, limited(code))
    for label, w in weights.items():
        extra = 8 + 8 * (w[1] != 0.0)              # prev written, and read unless w_old == 0
        add("nss_step_flux_ab2_f64 %s" % label, 80 + extra, donor_ab2(w))
        for code, name in enumerate(limiters):
            add("limited ab2, %s %s" % (name, label), 48 + extra, limited_ab2(code, w))
    lines += ["## (a) The flux kernels alone, 3-D n = %d, %d launches per measurement, alternated, median of %d, %s" %
              (args.grid, args.reps, args.rounds, eng.device_info()["arch"]), "",
              "| kernel | points | algorithmic MB | us (spread) | GB/s | time / twin |", "|---|---|---|---|---|---|"]

    def table(res, count, once):
        twin = next(iter(res.values()))[0]
        for name, (t, spread) in res.items():
            nbytes = per[name] * count + once
            lines.append("| %s | %d | %.1f | %.1f (%.1f) | %.0f | %.2f |" % (name, count, nbytes / 1e6, 1e3 * t,
                                                                             1e3 * spread, nbytes / t / 1e6, t / twin))
        lines.append("")
    table(alternate(torch, bodies, args.reps, args.rounds), nflux, 8 * s.n_u)

    sops = s.scalar_operators(0.01, WALLS)
    savg, sdif = (hipla.SparseMatrix.from_scipy(sops[k]) for k in ("avg", "diff"))
    sst = upload_stencil(eng, s.scalar_stencil(), s.n_p)
    tg = eng.from_host(np.concatenate([np.random.default_rng(6).random(s.n_p), np.zeros(s.n_u)]))
    G = eng.view(tg, s.n_p, s.n_p + s.n_u)
    u, f, w_b = (eng.from_host(np.random.default_rng(k).standard_normal(s.n_u)) for k in (2, 8, 9))
    f_eff, G_prev, b_prev = eng.zeros(s.n_u), eng.zeros(s.n_u), eng.zeros(s.n_u)
    operands = (w_b.data_ptr(), u.data_ptr(), f.data_ptr(), tg.data_ptr(), 0.5)

    def scalar(code):
        return lambda: eng._check(lib.nss_scalar_flux_limited_f64(sst.data_ptr(), s.n_u, code, *operands, G.data_ptr(),
                                                                  f_eff.data_ptr(), None, eng.stream))

    def history(w):
        return (w[0], w[1], G_prev.data_ptr(), G.data_ptr(), b_prev.data_ptr(), f_eff.data_ptr(), None, eng.stream)

    def scalar_ab2(w):
        return lambda: eng._check(lib.nss_scalar_flux_ab2_f64(savg.handle.ptr, sdif.handle.ptr, *operands, *history(w)))

    def scalar_limited_ab2(code, w):
        return lambda: eng._check(lib.nss_scalar_flux_limited_ab2_f64(sst.data_ptr(), s.n_u, code, *operands, *history(w)))
    bodies, per = {}, {}
    add("nss_scalar_flux_f64, buoyant", 88, lambda: eng._check(lib.nss_scalar_flux_f64(
        savg.handle.ptr, sdif.handle.ptr, *operands, G.data_ptr(), f_eff.data_ptr(), None, eng.stream)), "face")
    for code, name in enumerate(limiters):
        add("limited, %s, buoyant" % name, 56, scalar(code), "face")
    for label, w in weights.items():
        both = 2 * (8 + 8 * (w[1] != 0.0))         # G_prev and b_prev
        add("nss_scalar_flux_ab2_f64, buoyant %s" % label, 88 + both, scalar_ab2(w), "face")
        for code, name in enumerate(limiters):
            add("limited ab2, %s, buoyant %s" % (name, label), 56 + both, scalar_limited_ab2(code, w), "face")
    table(alternate(torch, bodies, args.reps, args.rounds), s.n_u, 8 * s.n_p)


def fresh(mesh, v0, scheme):
    from templates.NavierStokesSIMPLE_iterative import NavierStokes
    ns = NavierStokes(mesh, nu=0.01, inflow="inlet", outflow="outlet", wall="wall|cyl", uin=None, timestep=0.05, order=0,
                      convection=scheme)
    s = ns.system
    ns.f.vec.data = hipla.Vector.from_numpy(ACCELERATION * s.h ** s.dim * np.random.default_rng(8).standard_normal(s.n_u))
    ns.gfu.data = hipla.Vector.from_numpy(v0)
    return ns


def span(iterations):
    lo, hi = int(min(iterations)), int(max(iterations))
    return str(lo) if lo == hi else "%d-%d" % (lo, hi)


def step_times(args, eng, torch, lines):
    from templates.NavierStokesSIMPLE_iterative import SyntheticMesh
    mesh = SyntheticMesh(1.0 / args.grid, dim=3)
    n_u = 3 * args.grid ** 2 * (args.grid - 1)
    v0 = ACCELERATION * np.random.default_rng(2).standard_normal(n_u)
    runs = {}
    for scheme in SCHEMES:
        ns = fresh(mesh, v0, scheme)
        last = {}

        def window(k, ns=ns, last=last):
            rec = ns.Advance(k)
            if rec.declined or rec.flux_declined:
                raise RuntimeError("Advance declined: %s" % (rec.declined or rec.flux_declined))
            last["rec"] = rec
        window(args.warmup)
        eng.synchronize()
        runs[scheme] = dict(ns=ns, window=window, last=last, wall=[], device=[])
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
    s = runs["upwind"]["ns"].system
    lines += ["## (b) Per-step time of Advance, 3-D n = %d (%d velocity dofs), %d windows of %d steps" %
              (args.grid, s.n_u, args.rounds, args.steps), "",
              "| convection | wall ms / step (spread) | device ms / step (spread) | mstar its | proj its |", "|---|---|---|---|---|"]
    for scheme, r in runs.items():
        rec = r["last"]["rec"]
        lines.append("| %s | %.3f (%.3f) | %.3f (%.3f) | %s | %s |" % (
            scheme, np.median(r["wall"]), np.ptp(r["wall"]), np.median(r["device"]), np.ptp(r["device"]),
            span(rec.mstar_iterations), span(rec.proj_iterations)))
    lines.append("")


def cavity(args, eng, lines):
    from templates.NavierStokesSIMPLE_iterative import NavierStokes, SyntheticMesh
    prandtl = 0.71
    literature = {1e3: (1.118, 3.649, 3.697), 1e5: (4.519, 34.73, 68.59)}
    lines += ["## (c) Differentially heated cavity, Pr = 0.71", "",
              "| Ra | n | convection | timestep | steps | steady | Nu (hot wall) | literature | u_max | literature | v_max | literature | wall s |",
              "|---|---|---|---|---|---|---|---|---|---|---|---|---|"]
    for rayleigh, n, tau, window in ((1e3, 32, 5e-4, 100), (1e3, 64, 5e-4, 100), (1e5, 64, 2.5e-5, 1000)):
        for scheme in ("upwind", "vanleer"):
            ns = NavierStokes(SyntheticMesh(1.0 / n, dim=2), nu=prandtl, inflow="inlet", outflow="outlet", wall="wall|cyl",
                              uin=None, timestep=tau, order=0, convection=scheme)
            ns.f.vec.data = hipla.Vector.from_numpy(np.zeros(ns.system.n_u))
            ns.AddScalar(1.0, dirichlet=WALLS, buoyancy=(0.0, rayleigh * prandtl), t_ref=0.5)
            t0, steps, nusselt, steady = time.perf_counter(), 0, None, False
            while time.perf_counter() - t0 < args.cavity_seconds:
                rec = ns.Advance(window)
                if rec.declined:
                    raise RuntimeError("Advance declined: %s" % rec.declined)
                steps += window
                previous, nusselt = nusselt, float(rec.wall_flux[-1])
                if steps % (10 * window) == 0:
                    print("cavity Ra %g n %d %s: %d steps, Nu %.6f" % (rayleigh, n, scheme, steps, nusselt), flush=True)
                if not np.isfinite(nusselt):
                    break
                if previous is not None and abs(nusselt - previous) <= 1e-6 * abs(nusselt):
                    steady = True
                    break
            u = ns.gfu.numpy()
            comps = ns.system.component_ids
            lit = literature[rayleigh]
            lines.append("| %g | %d | %s | %g | %d | %s | %.4f | %.3f | %.3f | %.3f | %.3f | %.3f | %.1f |" % (
                rayleigh, n, scheme, tau, steps, "yes" if steady else "NO", nusselt, lit[0],
                np.abs(u[comps[0].ravel()]).max(), lit[1], np.abs(u[comps[1].ravel()]).max(), lit[2],
                time.perf_counter() - t0))
    lines += ["", "Literature: de Vahl Davis, Int. J. Numer. Meth. Fluids 3 (1983) 249-264 (mean Nusselt number, largest "
              "horizontal velocity on the vertical mid-plane, largest vertical velocity on the horizontal mid-plane; here "
              "u_max / v_max are taken over all faces).", ""]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", type=int, default=64)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--cavity-seconds", type=float, default=150.0)
    ap.add_argument("--parts", default="abc")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    eng = hipla.get_engine()                      # (no GPU: raises -- a timing needs the device)
    lines = ["# Second-order limited convection: measured (tools/limited_convection_rate.py)", ""]
    if "a" in args.parts:
        kernels(args, eng, torch, lines)
    if "b" in args.parts:
        step_times(args, eng, torch, lines)
    if "c" in args.parts:
        cavity(args, eng, lines)
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
