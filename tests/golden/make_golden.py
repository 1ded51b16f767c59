#!/usr/bin/env python3
"""Generate the golden vectors under tests/golden/ (run in the BUILD CONTAINER only).

How: the reference's *unmodified* solver files are loaded from a checkout of it given on the command line
(minres.py, bramble_pasciak_cg.py, solvers/bramblepasciak_new.py, orthonormalization.py) with
``ngsolve`` resolved to a test-only stand-in, TWICE:

1. over ``tests/ngsolve_numpy`` -- a numpy/scipy-only implementation of the ``ngsolve.la``
   surface that shares no code with the product.  **These runs are what
   the fixtures store.**
2. over ``tests/ngsolve_standin`` -- the product's own protocol layer (``hipla``) with the numpy
   checker engine.  Every output of run 2 must agree with run 1 (scalars and the first
   ``HEAD`` history entries to 1e-12, histories to 1e-9 over the stable window, iteration counts
   exactly or within the recorded perturbation spread) or this script fails: a semantic
   deviation of the product's expression layer (aliasing in ``result.data += H * result``,
   assigning ``MultAdd``, evaluation into the destination) cannot hide in golden and product alike.

NGSolve itself is not installable here, so these goldens pin the
reference's control flow, operation order, recurrences, stopping rules and return values over
numpy/scipy arithmetic; against real NGSolve output parity is unpinned.

Nothing of the reference is written to the repo: only inputs (generator parameters, seed) and
outputs (k, histories, iteration counts, norms, solution samples).

    python tests/golden/make_golden.py <reference checkout>          # rewrites tests/golden/*.npz
"""

import contextlib
import importlib
import importlib.util
import io
import os
import re
import sys

import numpy as np
import scipy.sparse as sp

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = None            # the reference checkout (command line)
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "navier-stokes-solver_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

from oracle import krylov_ref as kr            # noqa: E402
from golden_cases import Case                  # noqa: E402
from staggered_grid import diffusion_2d        # noqa: E402

HEAD = 12            # leading history entries that must agree to 1e-12 between the two stand-ins


# ------------------------------------------------------------------------------------------
# the two stand-ins
# ------------------------------------------------------------------------------------------
class Backend:
    """One ``ngsolve`` stand-in + the reference modules imported over it."""

    name = path = None

    def __init__(self):
        for key in [k for k in sys.modules if k == "ngsolve" or k.startswith("ngsolve.")]:
            del sys.modules[key]
        sys.path.insert(0, self.path)
        try:
            self.ng = importlib.import_module("ngsolve")
            self.minres = self._load("minres.py")
            self.v1 = self._load("bramble_pasciak_cg.py")
            self.v2 = self._load("solvers/bramblepasciak_new.py")
            self.orth = self._load("orthonormalization.py")
        finally:
            sys.path.remove(self.path)
        self.lams = None
        for mod in (self.v1, self.v2):
            mod.EigenValues_Preconditioner = self._spy(mod.EigenValues_Preconditioner)

    def _load(self, rel):
        name = "ref_%s_%s" % (self.name, rel.replace("/", "_")[:-3])
        spec = importlib.util.spec_from_file_location(name, os.path.join(REF, rel))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        return mod

    def _spy(self, orig):
        def wrapper(*a, **kw):
            lams = orig(*a, **kw)
            self.lams = np.array(lams)
            return lams
        return wrapper

    def engine(self):
        return contextlib.nullcontext()

    # operand constructors -------------------------------------------------------------------
    def block(self, comps):
        return self.ng.BlockVector(list(comps))

    def block_matrix(self, rows):
        return self.ng.BlockMatrix(rows)

    def inner(self, a, b):
        return self.ng.InnerProduct(a, b)

    def preA(self, case):
        if case.blocks is None:
            return self.diag(case.jacobi_diagonal())
        return self.bjac(case.pre_matrix, case.blocks)

    def form(self, case):
        """BilinearForm-like operand (solvers/bramblepasciak_new.py:11-17,88,105-109)."""
        class Form:
            pass
        blf = Form()
        blf.condense = case.condense
        if case.condense:
            blf.mat = self.sparse(case.parts["mat"])
            for key in ("inner_matrix", "inner_solve", "harmonic_extension", "harmonic_extension_trans"):
                setattr(blf, key, self.sparse(case.parts[key]))
        else:
            blf.mat = self.sparse(case.system.A)
        return blf

    def plain_form(self, mat):
        class Form:
            pass
        blf = Form()
        blf.mat, blf.condense = mat, False
        return blf


class NumpyBackend(Backend):
    name, path = "numpy", os.path.join(ROOT, "tests", "ngsolve_numpy")

    def sparse(self, csr):
        return self.ng.SparseMatrix(csr)

    def vec(self, arr):
        return self.ng.Vector(np.array(arr, dtype=np.float64))

    def zeros(self, n):
        return self.ng.Vector(int(n))

    def diag(self, d):
        return self.ng.SparseMatrix(sp.diags(np.asarray(d, dtype=np.float64)).tocsr())

    def bjac(self, A, idx):
        """J = sum_b E_b A_bb^-1 E_b^T as one sparse matrix (dense inverses by numpy)."""
        A = sp.csr_matrix(A)
        rows, cols, vals = [], [], []
        for b in range(idx.shape[1]):
            dofs = idx[:, b]
            dofs = dofs[dofs >= 0]
            inv = np.linalg.inv(A[dofs][:, dofs].toarray())
            rows.append(np.repeat(dofs, dofs.size))
            cols.append(np.tile(dofs, dofs.size))
            vals.append(inv.ravel())
        J = sp.csr_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=A.shape)
        return self.ng.SparseMatrix(J)

    def numpy(self, v):
        return v.numpy()


class HiplaBackend(Backend):
    name, path = "hipla", os.path.join(ROOT, "tests", "ngsolve_standin")

    def __init__(self):
        import hipla
        from oracle.numpy_engine import NumpyEngine
        self.hipla = hipla
        hipla.set_engine(NumpyEngine())
        super().__init__()

    def sparse(self, csr):
        return self.hipla.SparseMatrix.from_scipy(sp.csr_matrix(csr))

    def vec(self, arr):
        return self.hipla.Vector.from_numpy(np.array(arr, dtype=np.float64))

    def zeros(self, n):
        return self.hipla.Vector(int(n))

    def diag(self, d):
        return self.hipla.DiagonalMatrix(np.asarray(d, dtype=np.float64))

    def bjac(self, A, idx):
        return self.hipla.BlockJacobi(self.sparse(A), idx)

    def numpy(self, v):
        return v.numpy()


# ------------------------------------------------------------------------------------------
# helpers
# ------------------------------------------------------------------------------------------
def stable_window(h1, h2, rtol=1e-10):
    m = min(len(h1), len(h2))
    rel = np.abs(h1[:m] - h2[:m]) / np.maximum(np.abs(h1[:m]), 1e-300)
    bad = np.nonzero(rel > rtol)[0]
    return int(bad[0]) if bad.size else m


class _ReversedDot:
    """Perturb only the summation order of every inner product."""

    def __enter__(self):
        self._dot = np.dot
        real = np.dot
        np.dot = lambda a, b: real(a[::-1], b[::-1])
        return self

    def __exit__(self, *exc):
        np.dot = self._dot
        return False


def samples(x, count=16):
    idx = np.linspace(0, x.size - 1, count).astype(np.int64)
    return idx, x[idx]


def parse_v2(text):
    hist = np.array([float(m) for m in re.findall(r"it =\s+\d+\s+err =\s+(\S+)", text)])
    return hist, float(re.search(r"err0 (\S+)", text).group(1))


# ------------------------------------------------------------------------------------------
# one reference run per (backend, case, solver)
# ------------------------------------------------------------------------------------------
def run_v1(be, case, tol, maxsteps, warm=None):
    s = case.system
    out = io.StringIO()
    kw = {}
    if warm is not None:
        kw["solution"] = be.block([be.vec(warm[0]), be.vec(warm[1])])
    with contextlib.redirect_stdout(out):
        sol, errors = be.v1.bramble_pasciak_cg(be.sparse(s.A), be.sparse(s.B), None, be.preA(case),
                                               be.diag(1.0 / s.mass), be.vec(case.f), be.vec(case.g),
                                               tolerance=tol, max_steps=maxsteps, print_rates=False, **kw)
    return dict(x=be.numpy(sol), hist=np.array(errors), lams=be.lams.copy(), warned="Warning" in out.getvalue(),
                aliased=bool(warm is not None and sol is kw["solution"]))


def run_v2(be, case, tol, maxsteps, warm=None, **kw):
    s = case.system
    if warm is None:
        solv = be.block([be.zeros(s.n_u), be.zeros(s.n_p)])
    else:
        solv = be.block([be.vec(warm[0]), be.vec(warm[1])])
    f = kw.pop("f", case.f)
    out = io.StringIO()
    with contextlib.redirect_stdout(out):
        ret = be.v2.BramblePasciakCG(be.form(case), be.plain_form(be.sparse(s.B)), None, be.vec(f), be.vec(case.g),
                                     be.preA(case), be.diag(1.0 / s.mass), solv, tol=tol, maxsteps=maxsteps,
                                     printrates=True, **kw)
    text = out.getvalue()
    res = dict(x=be.numpy(solv), lams=be.lams.copy(), warned="Warning" in text, returned_solution=bool(ret is solv))
    if not res["returned_solution"]:
        res["it"] = ret[0]
        res["hist"], res["err0"] = parse_v2(text)
    return res


def run_minres(be, case, tol, maxsteps, warm=None, rhs_scale=1.0, **kw):
    s = case.system
    A, B = be.sparse(s.A), be.sparse(s.B)
    K = be.block_matrix([[A, B.T], [B, None]])                 # run.py:45-46
    C = be.block_matrix([[be.preA(case), None], [None, be.diag(1.0 / s.mass)]])
    rhs = be.block([be.vec(rhs_scale * case.f), be.vec(case.g)])
    if warm is not None:
        kw["sol"] = be.block([be.vec(warm[0]), be.vec(warm[1])])
    out = io.StringIO()
    with contextlib.redirect_stdout(out):
        u, errs = be.minres.MinRes(mat=K, pre=C, rhs=rhs, maxsteps=maxsteps, tol=tol, printrates=False, **kw)
    return dict(x=be.numpy(u), hist=np.array(errs), warned="Warning" in out.getvalue(),
                aliased=bool(warm is not None and u is kw["sol"]))


def cross_check(tag, a, b, window, spread):
    """Outputs of the two stand-ins: `a` (numpy-only, stored) vs `b` (product protocol layer)."""
    report = {}
    for key in ("err0",):
        if key in a:
            rel = abs(a[key] - b[key]) / abs(a[key])
            assert rel <= 1e-12, (tag, key, rel)
    if "lams" in a:
        rel = abs(a["lams"].min() - b["lams"].min()) / abs(a["lams"].min())
        assert rel <= 1e-12, (tag, "lam_min", rel)
    if "hist" in a:
        m = min(len(a["hist"]), len(b["hist"]))
        rel = np.abs(a["hist"][:m] - b["hist"][:m]) / np.abs(a["hist"][:m])
        head = float(rel[:HEAD].max())
        inwin = float(rel[: min(m, window)].max())
        assert head <= 1e-12, (tag, "history head", head)
        assert inwin <= 1e-9, (tag, "history window", inwin)
        assert abs(len(a["hist"]) - len(b["hist"])) <= max(2, 2 * spread), (tag, len(a["hist"]), len(b["hist"]))
        report = {"standin_head_rel_diff": head, "standin_window_rel_diff": inwin,
                  "standin_iteration_diff": len(b["hist"]) - len(a["hist"])}
    xa, xb = a["x"], b["x"]
    denom = max(np.linalg.norm(xa), 1e-300)
    assert np.linalg.norm(xa - xb) <= 1e-7 * denom, (tag, "solution", np.linalg.norm(xa - xb) / denom)
    for key in ("warned", "aliased", "returned_solution"):
        if key in a:
            assert a[key] == b[key], (tag, key)
    return report


# ------------------------------------------------------------------------------------------
def main():
    backends = [NumpyBackend(), HiplaBackend()]
    written = []

    def save(name, **kw):
        path = os.path.join(HERE, name + ".npz")
        np.savez_compressed(path, **kw)
        written.append((name, os.path.getsize(path), kw.get("standin_window_rel_diff", 0.0)))

    def both(fn, *a, **kw):
        return [fn(be, *a, **kw) for be in backends]

    # (dim, n, pre, nu, inflate, condense, solvers)
    ALL = ("bpcg1", "bpcg2", "minres")
    grid = [(dim, n, pre, 0.01, 1, 0, ALL)
            for dim, n in ((2, 12), (2, 24), (2, 48), (3, 6), (3, 10)) for pre in ("jacobi", "bjac")]
    # statically condensed form (what configs 3-5 literally run; only v2 has the branch)
    grid += [(dim, n, pre, 0.01, 1, 1, ("bpcg2",)) for dim, n in ((2, 24), (3, 8)) for pre in ("jacobi", "bjac")]
    # the reference's row regime: ~25 / ~84 non-zeros per row, facet blocks of 5 / 12 dofs
    grid += [(2, 16, "facet", 0.01, 5, 0, ALL), (3, 5, "facet", 0.01, 12, 0, ALL)]
    # Re = 400, 1000 (config 5 sweeps nu; templates/NavierStokesSIMPLE_iterative.py:66,72)
    grid += [(3, 8, "bjac", 1.0 / 400.0, 1, 0, ALL), (3, 8, "bjac", 1.0 / 1000.0, 1, 0, ALL)]
    seed = 0

    for dim, n, pre, nu, inflate, condense, solvers in grid:
        params = dict(dim=dim, n=n, nu=nu, seed=seed, pre=pre, inflate=inflate, condense=condense)
        case = Case(params)
        s = case.system
        Ks, b = s.saddle_matrix(), case.rhs
        tag = "stokes%dd_n%d_%s" % (dim, n, pre)
        if inflate > 1:
            tag += "_x%d" % inflate
        if condense:
            tag += "_cond"
        if nu != 0.01:
            tag += "_re%d" % round(1.0 / nu)
        common = dict(n_u=s.n_u, n_p=s.n_p, **params)
        oA, oB, pa, ps, ocond = case.oracle_operands(kr)

        if "bpcg1" in solvers:                   # ---- BPCG v1 (bramble_pasciak_cg.py:65)
            tol, mx = 1e-10, 5000
            r, r2 = both(run_v1, case, tol, mx)
            k = 1.0 / r["lams"].min() + 1e-3
            o1 = kr.bpcg_v1(oA, oB, pa, ps, case.f, case.g, k, tolerance=tol, max_steps=mx)
            with _ReversedDot():
                o2 = kr.bpcg_v1(oA, oB, pa, ps, case.f, case.g, k, tolerance=tol, max_steps=mx)
            W = stable_window(o1[2], o2[2])
            its, itp = len(r["hist"]) - 1, len(o2[2]) - 1
            rep = cross_check(tag + "_bpcg1", r, r2, W, abs(its - itp))
            si, sv = samples(r["x"])
            save(tag + "_bpcg1", solver="bpcg1", tol=tol, maxsteps=mx, k=k, lam_min=r["lams"].min(),
                 lam_max=r["lams"].max(), errors=r["hist"], iterations=its, window=W, x_norm=np.linalg.norm(r["x"]),
                 iterations_perturbed=itp, residual=np.linalg.norm(b - Ks @ r["x"]), b_norm=np.linalg.norm(b),
                 sample_idx=si, sample_val=sv, warned=r["warned"], **rep, **common)

        if "bpcg2" in solvers:                   # ---- BPCG v2 (solvers/bramblepasciak_new.py:24)
            tol, mx = 1e-10, 5000
            r, r2 = both(run_v2, case, tol, mx)
            k = 1.0 / r["lams"].min() + 1e-3
            p1 = kr.bpcg_v2(oA, oB, pa, ps, case.f, case.g, k, tol=tol, maxsteps=mx, condensed=ocond)
            with _ReversedDot():
                p2 = kr.bpcg_v2(oA, oB, pa, ps, case.f, case.g, k, tol=tol, maxsteps=mx, condensed=ocond)
            W = stable_window(p1[3], p2[3])
            rep = cross_check(tag + "_bpcg2", r, r2, W, abs(r["it"] - p2[0]))
            si, sv = samples(r["x"])
            save(tag + "_bpcg2", solver="bpcg2", tol=tol, maxsteps=mx, k=k, lam_min=r["lams"].min(),
                 lam_max=r["lams"].max(), history=r["hist"], err0=r["err0"], iterations=r["it"], window=W,
                 x_norm=np.linalg.norm(r["x"]), iterations_perturbed=p2[0],
                 residual=np.linalg.norm(b - Ks @ r["x"]), b_norm=np.linalg.norm(b), sample_idx=si, sample_val=sv,
                 warned=r["warned"], **rep, **common)

        if "minres" in solvers:                  # ---- MINRES (minres.py:12; operands as run.py:45-46)
            tol, mx = 1e-10, 5000
            r, r2 = both(run_minres, case, tol, mx)
            q1 = kr.minres(oA, oB, pa, ps, case.f, case.g, maxsteps=mx, tol=tol)
            with _ReversedDot():
                q2 = kr.minres(oA, oB, pa, ps, case.f, case.g, maxsteps=mx, tol=tol)
            W = stable_window(q1[2], q2[2])
            its, itp = len(r["hist"]) - 1, len(q2[2]) - 1
            rep = cross_check(tag + "_minres", r, r2, W, abs(its - itp))
            si, sv = samples(r["x"])
            save(tag + "_minres", solver="minres", tol=tol, maxsteps=mx, errors=r["hist"], iterations=its,
                 iterations_perturbed=itp, window=W, x_norm=np.linalg.norm(r["x"]),
                 residual=np.linalg.norm(b - Ks @ r["x"]), b_norm=np.linalg.norm(b), sample_idx=si, sample_val=sv,
                 warned=r["warned"], **rep, **common)

    # ---- quirk cases (SURVEY.md 8c "Goldens to capture") ------------------------------------
    params = dict(dim=2, n=12, nu=0.01, seed=seed, pre="jacobi", inflate=1, condense=0)
    case = Case(params)
    s = case.system
    Ks, b = s.saddle_matrix(), case.rhs
    common = dict(n_u=s.n_u, n_p=s.n_p, **params)
    rng = np.random.default_rng(7)
    warm = (0.1 * rng.standard_normal(s.n_u), 0.1 * rng.standard_normal(s.n_p))

    # MINRES leaves through the absolute guard `ResNorm > tol` (:96) -> warning (:145-146)
    r, r2 = both(run_minres, case, 1e-6, 2000, rhs_scale=1e-3)
    cross_check("quirk_minres_absolute_guard", r, r2, 40, 0)
    save("quirk_minres_absolute_guard", solver="minres", rhs_scale=1e-3, tol=1e-6, maxsteps=2000, errors=r["hist"],
         iterations=len(r["hist"]) - 1, warned=r["warned"], x_norm=np.linalg.norm(r["x"]), **common)

    # MINRES warm start, initialize=False (:65-66)
    r, r2 = both(run_minres, case, 1e-8, 2000, warm=warm, initialize=False)
    cross_check("quirk_minres_warm_start", r, r2, 40, 0)
    save("quirk_minres_warm_start", solver="minres", tol=1e-8, maxsteps=2000, warm_seed=7, errors=r["hist"],
         iterations=len(r["hist"]) - 1, x_norm=np.linalg.norm(r["x"]), aliased=r["aliased"],
         residual=np.linalg.norm(b - Ks @ r["x"]), **common)

    # v2: zero right-hand side -> wdn == 0 -> returns the bare vector (:191-192)
    r, r2 = both(run_v2, case, 1e-10, 100, f=np.zeros(s.n_u))
    cross_check("quirk_bpcg2_zero_rhs", r, r2, 0, 0)
    save("quirk_bpcg2_zero_rhs", solver="bpcg2", returned_solution_object=r["returned_solution"],
         x_norm=np.linalg.norm(r["x"]), **common)

    # v2 warm start (initialize=False) and rel_err=False (absolute stop, :246)
    for name, kw in [("quirk_bpcg2_warm_start", dict(initialize=False, rel_err=True)),
                     ("quirk_bpcg2_abs_err", dict(initialize=True, rel_err=False))]:
        r, r2 = both(run_v2, case, 1e-6, 2000, warm=warm, **kw)
        cross_check(name, r, r2, 40, 0)
        save(name, solver="bpcg2", tol=1e-6, maxsteps=2000, warm_seed=7, k=1.0 / r["lams"].min() + 1e-3,
             history=r["hist"], err0=r["err0"], iterations=r["it"], x_norm=np.linalg.norm(r["x"]),
             residual=np.linalg.norm(b - Ks @ r["x"]), initialize=kw["initialize"], rel_err=kw["rel_err"], **common)

    # v1 warm start: `solution` given (:88-90), hits max_steps -> warning (:144-145)
    r, r2 = both(run_v1, case, 1e-12, 40, warm=warm)
    cross_check("quirk_bpcg1_warm_start_maxsteps", r, r2, 40, 0)
    save("quirk_bpcg1_warm_start_maxsteps", solver="bpcg1", tol=1e-12, maxsteps=40, warm_seed=7,
         k=1.0 / r["lams"].min() + 1e-3, errors=r["hist"], iterations=len(r["hist"]), aliased=r["aliased"],
         warned=r["warned"], x_norm=np.linalg.norm(r["x"]), **common)

    # ---- cfg1 plumbing: SpMV + InnerProduct + AXPY via orthonormalization.py ----------
    M = diffusion_2d(64)
    x0 = np.random.default_rng(3).standard_normal(M.shape[0])
    results = []
    for be in backends:
        Mh = be.sparse(M)
        basis = [be.vec(x0)]
        for _ in range(4):
            nxt = basis[-1].CreateVector()
            nxt.data = Mh * basis[-1]
            basis.append(nxt)
        basis = be.orth.orthonormalize(basis)
        galerkin = np.zeros((5, 5))
        res = basis[0].CreateVector()
        for c in range(5):
            res.data = Mh * basis[c]                        # heat.py:110
            for r_ in range(5):
                galerkin[r_, c] = be.inner(basis[r_], res)  # heat.py:112
        gram = np.array([[be.inner(a, b_) for b_ in basis] for a in basis])
        results.append((galerkin, gram))
    assert np.abs(results[0][0] - results[1][0]).max() <= 1e-12 * np.abs(results[0][0]).max()
    assert np.abs(results[0][1] - results[1][1]).max() <= 1e-12
    galerkin, gram = results[0]
    xs, hist = kr.cg(M, x0, tol=1e-10, maxsteps=500)
    save("cfg1_heat_plumbing", n=64, seed=3, galerkin=galerkin, gram=gram, rows=M.shape[0], nnz=M.nnz,
         cg_history=hist, cg_iterations=len(hist) - 1, cg_x_norm=np.linalg.norm(xs),
         cg_residual=np.linalg.norm(x0 - M @ xs))

    for name, size, diff in written:
        print("%-44s %6d B   stand-ins differ by %.1e inside the window" % (name, size, diff))


if __name__ == "__main__":
    if len(sys.argv) != 2 or not os.path.isdir(sys.argv[1]):
        raise SystemExit("usage: make_golden.py <checkout of matschiner/navier-stokes-solver>")
    REF = os.path.abspath(sys.argv[1])
    main()
