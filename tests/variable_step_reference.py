"""numpy / scipy restatement of the variable-step IMEX step (`DoTimeStep(timestep=)`, `Advance(timesteps=)` /
`Advance(cfl=)`) with exact inner solves -- a helper of the variable-step tests, not a test.  It extends
`cnab2_reference.Cnab2Reference` and shares nothing with the product but what that class shares: `step_with(tau)` is its
step with tau_n for the step size, theta = tau_n (euler) or tau_n / 2 (cnab2) in the two implicit operators (factorised
once per step size), and for "cnab2" the variable-step Adams-Bashforth weights

    (w_new, w_old) = (1 + r / 2, -r / 2),   r = tau_n / tau_{n-1}        ((1, 0) on a quantity's first step)

-- or, with ``naive=True``, the fixed-step (3/2, -1/2) whatever r, which is only first order under a variable step.
`rate()` is max_cell sum_faces |u_f| / h written as max_r (|B| |u|)_r / (M_p)_r, `run_controlled` the step-size
controller min(max_timestep, cfl / rate, growth * tau_{n-1}) with the landing on a duration, written out here
independently of `hipla.stepping.choose_timestep`."""

import numpy as np
import scipy.sparse as sp
from scipy.sparse.linalg import splu

from cnab2_reference import Cnab2Reference


class VariableStepReference(Cnab2Reference):
    def __init__(self, system, tau, u0, f, convection="upwind", time_scheme="cnab2", scalar=None, T0=None, q0=None,
                 naive=False):
        super().__init__(system, tau, u0, f, convection, time_scheme, scalar=scalar, T0=T0, q0=q0)
        self.naive, self.tau_prev, self.r = bool(naive), None, 1.0
        self.solvers = {}
        self.abs_B = abs(system.B).tocsr()

    def weights(self, quantity):
        if not (self.cnab2 and self.valid[quantity]):
            return (1.0, 0.0)
        r = 1.0 if self.naive else self.r
        return (1.0 + r / 2, -r / 2)

    def _solvers(self, tau):
        if tau not in self.solvers:
            s = self.s
            theta = 0.5 * tau if self.cnab2 else tau
            solve_u = splu(sp.csc_matrix(s.h ** s.dim * sp.identity(s.n_u) + theta * s.A)).solve
            solve_T = None
            if self.scalar is not None:
                ops = self.scalar["ops"]
                solve_T = splu(sp.csc_matrix(sp.diags(ops["mass"]) + theta * ops["K"])).solve
            self.solvers[tau] = (solve_u, solve_T)
        return self.solvers[tau]

    def step_with(self, tau):
        """One step of size `tau`; returns the stages of `Cnab2Reference.step`."""
        tau = float(tau)
        self.tau = tau
        self.solve_u, solve_T = self._solvers(tau)
        if self.scalar is not None:
            self.scalar["solve"] = solve_T
        self.r = 1.0 if self.tau_prev is None else tau / self.tau_prev
        out = self.step()
        self.tau_prev = tau
        return out

    def reset(self):
        super().reset()
        self.tau_prev = None

    def run_pattern(self, tau_mean, pattern, nsteps):
        """`nsteps` steps of sizes tau_mean * pattern[k % len(pattern)] (a pattern of mean 1 keeps the end time)."""
        for k in range(nsteps):
            self.step_with(tau_mean * pattern[k % len(pattern)])
        return self

    def rate(self, u=None):
        u = self.u if u is None else u
        return float(((self.abs_B @ np.abs(u)) / self.s.mass).max())

    def run_controlled(self, nsteps, cfl, max_timestep, growth=1.25, duration=None):
        """At most `nsteps` controlled steps; returns (sizes, codes, cfl numbers tau_n * rate(u^n))."""
        taus, codes, numbers, time = [], [], [], 0.0
        for _ in range(nsteps):
            rate = self.rate()
            if not np.isfinite(rate):
                raise FloatingPointError("rate %r" % rate)
            terms = [(float(max_timestep), "max")]
            if rate > 0.0:
                terms.append((cfl / rate, "cfl"))
            if self.tau_prev is not None:
                terms.append((growth * self.tau_prev, "growth"))
            tau, code = min(terms, key=lambda t: t[0])           # (min keeps the first of equal terms)
            if duration is not None and tau >= (duration - time) * (1.0 - 1e-12):
                tau, code = duration - time, "end"
            self.step_with(tau)
            time += tau
            taus.append(tau)
            codes.append(code)
            numbers.append(tau * rate)
            if code == "end":
                break
        return np.array(taus), codes, np.array(numbers)
