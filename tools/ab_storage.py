"""Same-box A/B of the preconditioner's value storage: the default path (BPCG v2, MypreA(GS=True) with the
auxiliary-space term) with storage="fp64" against storage="fp32", uncondensed or condensed (MypreA over the Schur
complement S):  python tools/ab_storage.py [--grid 136] [--form uncondensed|condensed] [--rounds 5] [--its 40]

Per storage: set-up seconds (auxiliary term + Gauss-Seidel handle, narrowing included; then the session: the Lanczos of
k, right-hand side, first direction), ms per iteration of the fused loop as the median of interleaved windows (fp64
window, fp32 window, ... `rounds` times, `its` iterations each), iterations to 1e-8 (a full solve), the true saddle
residual, and the device times of the preconditioner's kernel groups (HIP events between launches that sweep the
caches): one Smooth call (gather, one launch per colour, scatter), the residual launch between the half-sweeps, and the
auxiliary-space term (T^T, the joint V-cycle: csr_multi_kernel, T).  Prints one markdown table and one JSON line."""
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
from staggered_grid import mac_stokes


class Form:
    def __init__(self, mat):
        self.mat, self.condense = mat, False


def build(s, form, storage, space, A):
    from discretizations import CondensedForm
    from templates.NavierStokesSIMPLE_iterative import MypreA, auxiliary_space_preconditioner, coupling_blocks
    eng = hipla.get_engine()
    eng.synchronize()
    t0 = time.perf_counter()
    _, _, aux = auxiliary_space_preconditioner(s, space, storage=storage)
    if form == "uncondensed":
        blfA = Form(A)
        preA = MypreA(None, blfA, s.facet_blocks(), GS=True, aux=aux, storage=storage)
    else:
        blfA = CondensedForm(s)
        preA = MypreA(None, blfA, coupling_blocks(s.facet_blocks(), blfA.interior), GS=True, aux=aux, storage=storage)
    eng.synchronize()
    return blfA, aux, preA, time.perf_counter() - t0


def session(s, blfA, B, preA):
    from solvers.bramblepasciak_new import BpcgSession
    f, g = s.rhs(0)
    eng = hipla.get_engine()
    sol = hipla.BlockVector([hipla.Vector(s.n_u), hipla.Vector(s.n_p)])
    eng.synchronize()
    t0 = time.perf_counter()
    with contextlib.redirect_stdout(io.StringIO()):
        ses = BpcgSession(blfA, Form(B), None, hipla.Vector.from_numpy(f), hipla.Vector.from_numpy(g), preA,
                          hipla.DiagonalMatrix(1.0 / s.mass), sol=sol)
    if ses.fused is None:
        raise RuntimeError("fused loop declined: %s" % ses.fused_declined)
    ses.first_direction()
    eng.synchronize()
    return ses, time.perf_counter() - t0


def solve(s, blfA, B, preA):
    from solvers.bramblepasciak_new import BramblePasciakCG
    f, g = s.rhs(0)
    sol = hipla.BlockVector([hipla.Vector(s.n_u), hipla.Vector(s.n_p)])
    with contextlib.redirect_stdout(io.StringIO()):
        it, seconds = BramblePasciakCG(blfA, Form(B), None, hipla.Vector.from_numpy(f), hipla.Vector.from_numpy(g),
                                       preA, hipla.DiagonalMatrix(1.0 / s.mass), sol, tol=1e-8, maxsteps=3000,
                                       rel_err=True)
    b = np.concatenate([f, g])
    res = np.linalg.norm(b - s.saddle_matrix() @ sol.numpy()) / np.linalg.norm(b)
    return int(it), float(res)


def kernel_ms(torch, eng, s, preA, aux, reps=12):
    big = [eng.zeros(1 << 25) for _ in range(3)]

    def timed(fn):
        ev = []
        for _ in range(reps + 2):
            eng.stream_triad(0.5, big[0], big[1], big[2])
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            ev.append((a, b))
        torch.cuda.synchronize()
        return sum(a.elapsed_time(b) for a, b in ev[2:]) / reps

    n = preA.Height()
    x = hipla.Vector.from_numpy(np.random.default_rng(0).standard_normal(n))
    y, r = hipla.Vector(n), hipla.Vector(n)
    out = {"sweep_call": timed(lambda: preA.Smooth(y, x)),
           "residual_launch": timed(lambda: preA.residual_mat.Mult(y, r)),
           "auxiliary_term": timed(lambda: aux.Mult(x, y))}
    out["value_bytes"] = {"sweep_matrix": preA.value_bytes() - hipla.matrix.value_bytes(preA.residual_mat),
                          "residual_matrix": hipla.matrix.value_bytes(preA.residual_mat),
                          "auxiliary_term": aux.value_bytes()}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", type=int, default=136)
    ap.add_argument("--form", choices=("uncondensed", "condensed"), default="uncondensed")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--its", type=int, default=40)
    args = ap.parse_args()
    import torch
    eng = hipla.get_engine()
    s = mac_stokes(3, args.grid, 0.01)
    space = s.auxiliary_space()
    A, B = hipla.SparseMatrix.from_scipy(s.A), hipla.SparseMatrix.from_scipy(s.B)
    runs = {}
    for storage in ("fp64", "fp32"):
        blfA, aux, preA, t_pre = build(s, args.form, storage, space, A)
        ses, t_ses = session(s, blfA, B, preA)
        runs[storage] = dict(blfA=blfA, aux=aux, preA=preA, ses=ses, setup_s=t_pre + t_ses, setup_pre_s=t_pre)
    warm = 10
    total = warm + args.rounds * args.its + 10
    for r in runs.values():
        loop = r["ses"].fused
        loop.start(r["ses"].wdn, r["ses"].err0, 0.0, True, total)
        loop.enqueue(0, warm)
        r["windows"] = []
    torch.cuda.synchronize()
    for w in range(args.rounds):                     # interleaved: fp64 window, fp32 window, ...
        for r in runs.values():
            lo = warm + w * args.its
            t0 = time.perf_counter()
            r["ses"].fused.enqueue(lo, lo + args.its)
            torch.cuda.synchronize()
            r["windows"].append(1e3 * (time.perf_counter() - t0) / args.its)
    result = {"grid": args.grid, "dof": int(s.ndof), "form": args.form, "rounds": args.rounds, "its": args.its}
    for storage, r in runs.items():
        its, res = solve(s, r["blfA"], B, r["preA"])
        result[storage] = {"ms_per_iteration": float(np.median(r["windows"])), "windows_ms": r["windows"],
                           "iterations_to_1e-8": its, "true_residual": res, "setup_s": r["setup_s"],
                           "setup_preconditioner_s": r["setup_pre_s"],
                           "kernel_ms": kernel_ms(torch, eng, s, r["preA"], r["aux"])}
    print("3-D MAC Stokes n=%d (%d DoF), %s, BPCG v2 + MypreA(GS=True) with the auxiliary-space term"
          % (args.grid, s.ndof, args.form))
    print("| storage | ms / iteration | iterations to 1e-8 | true residual | set-up s | sweep call ms | residual ms "
          "| auxiliary term ms |\n|---|---|---|---|---|---|---|---|")
    for storage in ("fp64", "fp32"):
        d = result[storage]
        k = d["kernel_ms"]
        print("| %s | %.3f | %d | %.1e | %.2f | %.3f | %.3f | %.3f |"
              % (storage, d["ms_per_iteration"], d["iterations_to_1e-8"], d["true_residual"], d["setup_s"],
                 k["sweep_call"], k["residual_launch"], k["auxiliary_term"]))
    print(json.dumps(result))


if __name__ == "__main__":
    main()
