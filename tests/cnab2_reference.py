"""numpy / scipy restatement of the second-order IMEX step (`NavierStokes(time_scheme="cnab2")`) with exact inner solves
-- a helper of the CN-AB2 tests, not a test.  It shares nothing with the product but the matrices and tables of
`StokesSystem` and `limited_flux`.  With (w_new, w_old) = (1, 0) on a quantity's first step (or after `reset`) and
(3/2, -1/2) afterwards, q the accumulated pressure:

    F = flux(u^n);  F_ext = w_new F + w_old F_prev;  F_prev = F
    [scalar]  G likewise;  b = w_b (avg T^n - t_ref);  f_step = f + w_new b + w_old b_prev;  b_prev = b
    temp = f_step - A u^n - D F_ext - B^T q;   raw = (M_u + tau/2 A)^-1 temp                      (splu)
    phi = (B M_u^-1 B^T)^+ B raw;   temp2 = raw - M_u^-1 B^T phi;   u^{n+1} = u^n + tau temp2;   q += phi
    [scalar]  temp_T = q_T - K T^n - B G_ext;  delta = (M_p + tau/2 K)^-1 temp_T;  T^{n+1} = T^n + tau delta

The pressure operator of the enclosed domain is singular (constants): its pseudo-inverse is the dense
inv(L + e e^T / n) - e e^T / n.  `time_scheme="euler"` restates the first-order step of `DoTimeStep` in the same class
(weights (1, 0) always, M + tau A, no B^T q, q = phi), for the order comparisons."""

import numpy as np
import scipy.sparse as sp
from scipy.sparse.linalg import splu


def pressure_pseudo_inverse(lap):
    n = lap.shape[0]
    e = np.full((n, n), 1.0 / n)
    return np.linalg.inv(lap.toarray() + e) - e


class Cnab2Reference:
    def __init__(self, system, tau, u0, f, convection="upwind", time_scheme="cnab2", scalar=None, T0=None, q0=None):
        """`scalar`: None or dict(kappa, dirichlet, buoyancy=None, t_ref=0.0, convection=None)."""
        from staggered_grid import limited_flux
        s = self.s = system
        self.tau, self.convection, self.cnab2 = float(tau), convection, time_scheme == "cnab2"
        self.limited_flux = limited_flux
        self.f = np.array(f, dtype=np.float64)
        self.u = np.array(u0, dtype=np.float64)
        self.q = np.zeros(s.n_p) if q0 is None else np.array(q0, dtype=np.float64)
        self.cops = s.convection_operators()
        self.stencil = s.convection_stencil() if convection != "upwind" else None
        mass_u = s.h ** s.dim
        theta = 0.5 * self.tau if self.cnab2 else self.tau
        self.solve_u = splu(sp.csc_matrix(mass_u * sp.identity(s.n_u) + theta * s.A)).solve
        self.correct = (s.B.T / mass_u).tocsr()
        self.lap_inv = pressure_pseudo_inverse((s.B @ self.correct).tocsr())
        self.Bt = s.B.T.tocsr()
        self.F_prev = self.G_prev = self.b_prev = None
        self.valid = {"momentum": False, "scalar": False}
        self.scalar = None
        if scalar is not None:
            self.add_scalar(T0=T0, **scalar)

    def add_scalar(self, kappa, dirichlet, buoyancy=None, t_ref=0.0, convection=None, T0=None):
        s = self.s
        sc = self.scalar = dict(ops=s.scalar_operators(kappa, dict(dirichlet or {})), t_ref=float(t_ref),
                                convection=self.convection if convection is None else convection)
        sc["w_b"] = None if buoyancy is None else s.buoyancy_weights(buoyancy)
        sc["stencil"] = s.scalar_stencil() if sc["convection"] != "upwind" else None
        theta = 0.5 * self.tau if self.cnab2 else self.tau
        sc["solve"] = splu(sp.csc_matrix(sp.diags(sc["ops"]["mass"]) + theta * sc["ops"]["K"])).solve
        self.T = np.full(s.n_p, float(t_ref)) if T0 is None else np.array(T0, dtype=np.float64)
        self.valid["scalar"] = False

    def reset(self):
        self.valid = dict.fromkeys(self.valid, False)

    def weights(self, quantity):
        return (1.5, -0.5) if self.cnab2 and self.valid[quantity] else (1.0, 0.0)

    def momentum_flux(self, u):
        c = self.cops
        adv = c["adv"] @ u
        if self.convection == "upwind":
            return adv * (c["avg"] @ u) - 0.5 * np.abs(adv) * (c["diff"] @ u)
        return self.limited_flux(self.stencil, adv, u, self.convection)

    def scalar_flux(self, u, T):
        sc = self.scalar
        if sc["convection"] == "upwind":
            return u * (sc["ops"]["avg"] @ T) - 0.5 * np.abs(u) * (sc["ops"]["diff"] @ T)
        return self.limited_flux(sc["stencil"], u, T, sc["convection"])

    @staticmethod
    def extrapolate(weights, now, prev):
        return weights[0] * now + (weights[1] * prev if weights[1] else 0.0)

    def step(self):
        """One step; returns the stages."""
        s, tau, u, out = self.s, self.tau, self.u, {}
        f_step = self.f
        sc = self.scalar
        if sc is not None:
            w = self.weights("scalar")
            G = self.scalar_flux(u, self.T)
            out["G"], out["G_ext"] = G, self.extrapolate(w, G, self.G_prev)
            self.G_prev = G
            if sc["w_b"] is not None:
                b = sc["w_b"] * (sc["ops"]["avg"] @ self.T - sc["t_ref"])
                f_step = self.f + self.extrapolate(w, b, self.b_prev)
                out["b"], self.b_prev = b, b
            self.valid["scalar"] = True
        out["f_step"] = f_step
        F = self.momentum_flux(u)
        out["F"], out["F_ext"] = F, self.extrapolate(self.weights("momentum"), F, self.F_prev)
        self.F_prev, self.valid["momentum"] = F, True
        temp = f_step - s.A @ u - self.cops["div"] @ out["F_ext"]
        if self.cnab2:
            temp = temp - self.Bt @ self.q
        raw = self.solve_u(temp)
        phi = self.lap_inv @ (s.B @ raw)
        temp2 = raw - self.correct @ phi
        self.u = u + tau * temp2
        self.q = self.q + phi if self.cnab2 else phi
        out.update(temp=temp, raw=raw, phi=phi, temp2=temp2, u=self.u, q=self.q)
        if sc is not None:
            temp_t = sc["ops"]["q"] - sc["ops"]["K"] @ self.T - s.B @ out["G_ext"]
            delta = sc["solve"](temp_t)
            self.T = self.T + tau * delta
            out.update(temp_T=temp_t, delta=delta, T=self.T)
        return out

    def run(self, nsteps):
        for _ in range(nsteps):
            self.step()
        return self


def smooth_start(system, seed=3, sweeps=6, peak=1.0):
    """A smooth, discretely divergence-free start field with max |u| = `peak`: a seeded field, smoothed by `sweeps`
    solves with M_u + 2 A (for nu = 0.01 a smoothing length of 0.14 per sweep), then projected."""
    s = system
    mass_u = s.h ** s.dim
    solve = splu(sp.csc_matrix(mass_u * sp.identity(s.n_u) + 2.0 * s.A)).solve
    v = np.random.default_rng(seed).standard_normal(s.n_u)
    for _ in range(sweeps):
        v = solve(mass_u * v)
    correct = (s.B.T / mass_u).tocsr()
    v = v - correct @ (pressure_pseudo_inverse((s.B @ correct).tocsr()) @ (s.B @ v))
    return peak * v / np.abs(v).max()


def order_errors(system, tau_total, steps, fine, u0, f, convection, time_scheme, scalar=None, T0=None):
    """Errors at `tau_total` of runs with `steps` steps against `fine` (the state of a fine "cnab2" run):
    list of (velocity error, temperature error or None), 2-norms relative to the fine state."""
    errs = []
    for n in steps:
        run = Cnab2Reference(system, tau_total / n, u0, f, convection, time_scheme, scalar=scalar, T0=T0).run(n)
        eu = np.linalg.norm(run.u - fine.u) / np.linalg.norm(fine.u)
        eT = None if scalar is None else np.linalg.norm(run.T - fine.T) / np.linalg.norm(fine.T)
        errs.append((eu, eT))
    return errs
