"""Reference code of the linearly implicit convection tests: the BiCGStab recurrence in numpy, the assembled operators
and the reference step (numpy, ``scipy.sparse.linalg.spsolve``, ``oracle.krylov_ref.project``).  Nothing here touches
the package's engine."""

import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spl

from oracle import krylov_ref as kr


def bicgstab(A, b, pre=None, tol=1e-10, maxsteps=200):
    """Right-preconditioned BiCGStab from x = 0 with rhat = r0 = b, as the issue writes it.  `A`: anything with ``@``;
    `pre`: callable or None.  Returns (iterates, hist, code): the x after every iteration, |r|_2 after every iteration,
    and 0 (converged, or the cap reached), 1 or 2 (the breakdowns)."""
    b = np.asarray(b, dtype=np.float64)
    pre = (lambda v: v) if pre is None else pre
    x, r, rhat, p = np.zeros_like(b), b.copy(), b.copy(), b.copy()
    rho, err0 = rhat @ r, np.linalg.norm(b)
    iterates, hist = [], []
    if err0 == 0.0:
        return iterates, hist, 0
    for _ in range(maxsteps):
        phat = pre(p)
        v = A @ phat
        rv = rhat @ v
        if rv == 0.0 or not np.isfinite(rv):
            return iterates, hist, 1
        alpha = rho / rv
        s = r - alpha * v
        shat = pre(s)
        t = A @ shat
        tt = t @ t
        omega = 0.0 if tt == 0.0 else (t @ s) / tt
        x = x + alpha * phat + omega * shat
        r = s - omega * t
        iterates.append(x.copy())
        hist.append(np.linalg.norm(r))
        if hist[-1] < tol * err0:
            return iterates, hist, 0
        if omega == 0.0:
            return iterates, hist, 2
        rho_new = rhat @ r
        if rho_new == 0.0 or not np.isfinite(rho_new):
            return iterates, hist, 1
        p = r + (rho_new / rho) * (alpha / omega) * (p - omega * v)
        rho = rho_new
    return iterates, hist, 0


def nearly_identity(n, seed):
    """A = I + 0.3 R / |R|_inf with R random, 0 to 5 entries per row (some rows empty): nonsymmetric, condition number
    below 10 (|A - I|_inf <= 0.3: the singular values lie in [0.7, 1.3] whenever |A - I|_1 <= 0.3 too; in general
    sigma_min >= 1 - sqrt(|E|_1 |E|_inf), which the caller may check).  An all-empty R gives the identity."""
    rng = np.random.default_rng(seed)
    rows, cols, vals = [], [], []
    for i in range(n):
        k = int(rng.integers(0, 6))
        if i % 7 == 3:
            k = 0
        c = rng.integers(0, n, size=k)
        rows += [i] * k
        cols += list(c)
        vals += list(rng.standard_normal(k))
    R = sp.coo_matrix((vals, (rows, cols)), shape=(n, n)).tocsr()
    R.sum_duplicates()
    norm = abs(R).sum(axis=1).max() if R.nnz else 0.0
    A = sp.identity(n, format="csr") + (0.3 / norm) * R if norm > 0 else sp.identity(n, format="csr")
    A = sp.csr_matrix(A)
    A.sort_indices()
    return A


def momentum_operator(system, a, tau, ops=None):
    """M_u + tau (A + N(a)) assembled from the grid operators alone (not through `linearised_convection`)."""
    ops = system.convection_operators() if ops is None else ops
    m_u = np.full(system.n_u, system.h ** system.dim)
    conv = ops["div"] @ (sp.diags(a) @ ops["avg"] - 0.5 * sp.diags(np.abs(a)) @ ops["diff"])
    return (sp.diags(m_u) + tau * (system.A + conv)).tocsc()


def scalar_operator(system, sops, u, tau):
    """M_p + tau (K + B G(u; .))."""
    conv = system.B @ (sp.diags(u) @ sops["avg"] - 0.5 * sp.diags(np.abs(u)) @ sops["diff"])
    return (sp.diags(sops["mass"]) + tau * (sops["K"] + conv)).tocsc()


def reference_step(system, u, f, tau, scalar=None):
    """One linearly implicit step in numpy.  `scalar`: None, or dict(ops=scalar_operators(...), T=..., w_b=... or None,
    t_ref=...) -- the buoyancy is lagged: the force of the step is f + w_b (avg T^n - t_ref).  Returns dict(u, phi[, T])."""
    ops = system.convection_operators()
    m_u = np.full(system.n_u, system.h ** system.dim)
    force = f
    if scalar is not None:
        sops, T = scalar["ops"], scalar["T"]
        if scalar.get("w_b") is not None:
            force = f + scalar["w_b"] * (sops["avg"] @ T - scalar["t_ref"])
    temp = kr.upwind_convection(ops, u) + force - system.A @ u
    raw = spl.spsolve(momentum_operator(system, ops["adv"] @ u, tau, ops), temp)
    temp2, phi = kr.project(system.B, m_u, raw)
    out = dict(u=u + tau * temp2, phi=phi)
    if scalar is not None:
        G = u * (sops["avg"] @ T) - 0.5 * np.abs(u) * (sops["diff"] @ T)
        rhs = sops["q"] - sops["K"] @ T - system.B @ G
        out["T"] = T + tau * spl.spsolve(scalar_operator(system, sops, u, tau), rhs)
    return out


def reference_run(system, u, f, taus, scalar=None):
    """`reference_step` over the step sizes `taus`; returns the last state and the kinetic energies <u, M_u u> / 2."""
    state, energy = dict(u=u, phi=None), []
    sc = None if scalar is None else dict(scalar)
    for tau in taus:
        state = reference_step(system, state["u"], f, tau, sc)
        if sc is not None:
            sc["T"] = state["T"]
        energy.append(0.5 * system.h ** system.dim * float(state["u"] @ state["u"]))
    return state, np.array(energy)
