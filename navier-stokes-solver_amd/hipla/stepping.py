"""Host side of the device-resident integrators in time: the IMEX step of `NavierStokes.Advance` (`TimeStepper`, with a
scalar `ScalarStepper`; C ABI ``nss_step_*`` / ``nss_scalar_*``) and the heat exponential integrator (`HeatIntegrator`),
each around `fused.CgLoop` solves.  They follow the `try_create` convention of the fused Krylov loops (hipla/fused.py)
and read its switch, ``fused.ENABLED``, when `try_create` is called."""

import ctypes as C

import numpy as np

from . import fdm, fused
from .amg import SmoothedAggregationAMG
from .fused import NO_PRE, CgLoop, FusedLoop, _hip, pre_for
from .matrix import BaseMatrix, DiagonalMatrix, JacobiPreconditioner, ScaledMatrix, SparseMatrix, SumMatrix
from .vector import Vector


def two_entry_rows(mat):
    """Whether every row of the scipy CSR matrix `mat` holds at most two entries -- the shape the row-per-lane kernels
    take (``nss::fixed_width_copy``): (True, None) or (False, reason)."""
    longest = int(np.diff(mat.indptr).max()) if mat.shape[0] else 0
    if longest > 2:
        return False, "a row holds %d entries (the row-per-lane kernels take two)" % longest
    return True, None


def constants_in_kernel(lap):
    """The test of oracle/krylov_ref.py::project for a pressure operator with the constants in its kernel (enclosed
    domain): |L 1| <= 1e-12 sum |L|."""
    return bool(np.linalg.norm(lap @ np.ones(lap.shape[0])) <= 1e-12 * abs(lap).sum())


CONVECTION_SCHEMES = {"upwind": 0, "minmod": 1, "vanleer": 2}      # scheme -> `limiter` of nss_*_flux_limited_f64


def check_convection(scheme, who):
    if scheme not in CONVECTION_SCHEMES:
        raise ValueError("%s: convection is \"upwind\", \"minmod\" or \"vanleer\", not %r" % (who, scheme))
    return scheme


TIME_SCHEMES = ("euler", "cnab2")


def check_time_scheme(scheme, who):
    if scheme not in TIME_SCHEMES:
        raise ValueError("%s: time_scheme is \"euler\" or \"cnab2\", not %r" % (who, scheme))
    return scheme


class TimeHistory:
    """The two-step history of a `time_scheme="cnab2"` object, in flux form: `F_prev` (momentum flux, n_F), `G_prev`
    (scalar flux, n_u) and `b_prev` (buoyancy force, n_u) as `Vector`s (None until the quantity has stepped), with one
    "valid" flag per quantity -- a quantity without valid history takes the weights (1, 0), i.e. one Euler-extrapolated
    step, a quantity with it (3/2, -1/2).  `DoTimeStep` and `Advance` read and write the same object.

    `tau_prev`: the size of the last step (None until a step has run, and after `reset()`); a step of size `tau` then
    extrapolates with the variable-step weights (1 + r/2, -r/2), r = tau / tau_prev -- (3/2, -1/2) exactly for r == 1.  An
    "euler" object keeps a `TimeHistory` for `tau_prev` alone (the growth limit of the step-size controller)."""

    QUANTITIES = ("momentum", "scalar")

    def __init__(self):
        self.F_prev = self.G_prev = self.b_prev = None
        self.valid = dict.fromkeys(self.QUANTITIES, False)
        self.tau_prev = None

    @staticmethod
    def ab2_weights(valid, tau=None, tau_prev=None):
        """(w_new, w_old) of a step of size `tau` behind one of size `tau_prev` (either None: equal steps)."""
        if not valid:
            return (1.0, 0.0)
        r = 1.0 if tau is None or tau_prev is None else float(tau) / float(tau_prev)
        return (1.0 + r / 2, -r / 2)

    def weights(self, quantity, tau=None):
        return self.ab2_weights(self.valid[quantity], tau, self.tau_prev)

    def reset(self, quantity=None):
        for key in self.QUANTITIES if quantity is None else (quantity,):
            self.valid[key] = False
        if quantity is None:
            self.tau_prev = None

    def vector(self, name, n, engine):
        """The history `Vector` `name` of length `n`, allocated (zero) on first use."""
        if getattr(self, name) is None or len(getattr(self, name)) != n:
            setattr(self, name, Vector(buf=engine.zeros(n), engine=engine))
        return getattr(self, name)


def check_step_size(tau, who):
    """`tau` as a float; ``ValueError`` unless it is positive and finite."""
    tau = float(tau)
    if not (tau > 0.0 and np.isfinite(tau)):
        raise ValueError("%s: a step size is positive and finite, not %r" % (who, tau))
    return tau


def choose_timestep(rate, cfl, max_timestep, previous=None, growth=1.25, remaining=None):
    """The step size of a CFL-controlled step, on the host: (tau, code) with

        tau = min(max_timestep, cfl / rate [rate > 0], growth * previous [previous is not None])

    and `code` the binding term, "max", "cfl" or "growth" (ties in that order).  `rate`: the CFL number of the state per
    unit of step size (`NavierStokes.CflRate`); `previous`: the size of the last step.  With `remaining` (the time left
    of a duration): a tau >= remaining (1 - 1e-12) becomes `remaining`, code "end".  A rate that is not finite raises
    ``FloatingPointError``."""
    rate = float(rate)
    if not np.isfinite(rate):
        raise FloatingPointError("choose_timestep: the CFL rate is %r" % (rate,))
    tau, code = float(max_timestep), "max"
    if rate > 0.0 and cfl / rate < tau:
        tau, code = cfl / rate, "cfl"
    if previous is not None and growth * previous < tau:
        tau, code = growth * previous, "growth"
    if remaining is not None and tau >= remaining * (1.0 - 1e-12):
        tau, code = float(remaining), "end"
    return tau, code


class StepController:
    """The arguments `cfl`, `max_timestep`, `growth`, `duration` of a CFL-controlled `Advance`, and the clock of one call:
    `next(rate, previous)` returns (tau, code) of the next step, or None when the duration has been reached."""

    def __init__(self, cfl, max_timestep, growth=1.25, duration=None):
        self.cfl, self.max_timestep, self.growth = float(cfl), check_step_size(max_timestep, "Advance"), float(growth)
        self.duration = None if duration is None else float(duration)
        if not (self.cfl > 0.0 and np.isfinite(self.cfl)):
            raise ValueError("Advance: cfl is positive and finite, not %r" % (cfl,))
        if not self.growth >= 1.0:
            raise ValueError("Advance: growth is at least 1, not %r" % (growth,))
        if self.duration is not None and not (self.duration > 0.0 and np.isfinite(self.duration)):
            raise ValueError("Advance: duration is positive and finite, not %r" % (duration,))
        self.time, self.ended = 0.0, False

    def next(self, rate, previous):
        if self.ended:
            return None
        remaining = None if self.duration is None else self.duration - self.time
        tau, code = choose_timestep(rate, self.cfl, self.max_timestep, previous, self.growth, remaining)
        self.ended = code == "end"
        self.time = self.duration if self.ended else self.time + tau
        return tau, code


def variable_record(taus, rates, codes):
    """The fields `timestep`, `time`, `cfl`, `limited_by` of a variable-step `StepRecord` from the step sizes, the rates
    of the states the steps started from, and the controller's codes (None: prescribed steps)."""
    taus = np.asarray(taus, dtype=np.float64)
    return dict(timestep=taus, time=np.cumsum(taus), cfl=taus * np.asarray(rates, dtype=np.float64)[:len(taus)],
                limited_by=None if codes is None else list(codes))


def upload_stencil(eng, stencil, n):
    """The (rows, 4) stencil of a limited flux launch as device int32 (16-byte aligned: a fresh allocation), after the
    range check the kernels leave to the caller: -1 <= entry < n."""
    st = np.ascontiguousarray(stencil, dtype=np.int32)
    if st.ndim != 2 or st.shape[1] != 4:
        raise ValueError("stencil: an int array (rows, 4), not %s" % (st.shape,))
    if st.size and (st.min() < -1 or st.max() >= n):
        raise ValueError("stencil: entries outside -1 .. %d" % (n - 1))
    buf = eng.torch.from_numpy(st if st.size else np.full((1, 4), -1, dtype=np.int32)).to(eng.device)
    assert buf.data_ptr() % 16 == 0
    return buf


def pair(v, default=(None, None)):
    """`precision` / `maxsteps` of `Advance` as (mstar, projection): one value for both, a pair, or None = `default`."""
    return default if v is None else tuple(v) if isinstance(v, (tuple, list)) else (v, v)


def _ptr(buf):
    return None if buf is None else buf.data_ptr()


class ConvectiveFlux:
    """The convective flux of one transported quantity under one `scheme`: "upwind" launches the donor-cell kernel over
    two-slot copies of the operators, "minmod" / "vanleer" the limited kernel over the uploaded stencil (avg and diff are
    then not uploaded).  The device operands are looked up in, and left in, `shared` ("adv", "avg", "diff", "stencil"),
    so that the objects of one system keep them once; `launch` is the package's one caller of the two `KERNELS`,
    `launch_ab2` of `KERNELS_AB2`, the same kernels with the extrapolating output policy (all in csrc/flux.hip)."""

    avg = diff = stencil = None

    @classmethod
    def available_ab2(cls, eng, scheme):
        """Whether the engine's library has the extrapolating kernel of `scheme`."""
        return hasattr(getattr(eng, "lib", None), cls.KERNELS_AB2[scheme != "upwind"])

    @classmethod
    def available(cls, eng, scheme):
        """Whether the engine's library has the kernel of `scheme`."""
        return hasattr(getattr(eng, "lib", None), cls.KERNELS[scheme != "upwind"])

    @staticmethod
    def declined(ops, keys=("adv", "avg", "diff")):
        """Why the row-per-lane kernels refuse `ops`: the first of `keys` with a row of more than two entries, or None."""
        return next((key + ": " + why for key in keys for ok, why in [two_entry_rows(ops[key])] if not ok), None)


class MomentumFlux(ConvectiveFlux):
    """F1, from `system.convection_operators()` (`ops`: those, when the caller holds them) / `convection_stencil()`."""

    KERNELS = ("nss_step_flux_f64", "nss_step_flux_limited_f64")
    KERNELS_AB2 = ("nss_step_flux_ab2_f64", "nss_step_flux_limited_ab2_f64")

    def __init__(self, eng, system, scheme, shared, ops=None):
        self.eng, self.scheme = eng, scheme
        for key in ("adv", "avg", "diff") if scheme == "upwind" else ("adv",):
            if key not in shared:
                ops = system.convection_operators() if ops is None else ops
                shared[key] = SparseMatrix.from_scipy(ops[key], engine=eng)
        self.adv = shared["adv"]
        self.nflux = self.adv.height
        if scheme == "upwind":
            self.avg, self.diff = shared["avg"], shared["diff"]
            return
        if "stencil" not in shared:
            shared["stencil"] = upload_stencil(eng, system.convection_stencil(), self.adv.width)
        self.stencil = shared["stencil"]
        if self.stencil.shape[0] != max(1, self.nflux):
            raise ValueError("TimeStepper: the stencil holds %d rows, adv %d" % (self.stencil.shape[0], self.nflux))

    def launch(self, u, flux):
        """flux = F(u); device buffers of adv's width and height."""
        eng, tail = self.eng, (u.data_ptr(), flux.data_ptr(), None, self.eng.stream)
        if self.stencil is None:
            eng._check(eng.lib.nss_step_flux_f64(self.adv.handle.ptr, self.avg.handle.ptr, self.diff.handle.ptr, *tail))
        else:
            eng._check(eng.lib.nss_step_flux_limited_f64(self.adv.handle.ptr, self.stencil.data_ptr(), self.nflux,
                                                         CONVECTION_SCHEMES[self.scheme], *tail))

    def launch_ab2(self, u, weights, prev, ext):
        """F = F(u);  ext = w_new F + w_old prev;  prev = F.  `weights` = (w_new, w_old); w_old == 0 reads no `prev`."""
        eng, tail = self.eng, (u.data_ptr(), weights[0], weights[1], prev.data_ptr(), ext.data_ptr(), None, self.eng.stream)
        if self.stencil is None:
            eng._check(eng.lib.nss_step_flux_ab2_f64(self.adv.handle.ptr, self.avg.handle.ptr, self.diff.handle.ptr, *tail))
        else:
            eng._check(eng.lib.nss_step_flux_limited_ab2_f64(self.adv.handle.ptr, self.stencil.data_ptr(), self.nflux,
                                                             CONVECTION_SCHEMES[self.scheme], *tail))


class ScalarFlux(ConvectiveFlux):
    """S1, from avg and diff of `ops` = `StokesSystem.scalar_operators(...)` / the host array `scalar_stencil()`."""

    KERNELS = ("nss_scalar_flux_f64", "nss_scalar_flux_limited_f64")
    KERNELS_AB2 = ("nss_scalar_flux_ab2_f64", "nss_scalar_flux_limited_ab2_f64")

    def __init__(self, eng, ops, scheme, stencil, shared):
        self.eng, self.scheme = eng, check_convection(scheme, "ScalarStepper")
        self.n_u, self.n_p = ops["avg"].shape
        if scheme != "upwind":
            if not self.available(eng, scheme):
                raise ValueError("ScalarStepper: the library has no limited flux kernel")
            if "stencil" not in shared:
                if stencil is None or np.shape(stencil) != (self.n_u, 4):
                    raise ValueError("ScalarStepper: convection=%r wants the (n_u, 4) scalar stencil" % (scheme,))
                shared["stencil"] = upload_stencil(eng, stencil, self.n_p)
            self.stencil = shared["stencil"]
            return
        missing = [key for key in ("avg", "diff") if key not in shared]
        if self.declined(ops, missing):
            raise ValueError("ScalarStepper: " + self.declined(ops, missing))
        shared.update((key, SparseMatrix.from_scipy(ops[key], engine=eng)) for key in missing)
        self.avg, self.diff = shared["avg"], shared["diff"]

    def launch(self, u, f, T, t_ref, G, w_b=None, f_eff=None):
        """G = the flux of `T` carried by `u`; with the weights `w_b` also f_eff = f + w_b (avg T - t_ref).  Buffers."""
        eng = self.eng
        tail = (_ptr(w_b), u.data_ptr(), _ptr(f), T.data_ptr(), t_ref, G.data_ptr(), _ptr(f_eff), None, eng.stream)
        if self.stencil is None:
            eng._check(eng.lib.nss_scalar_flux_f64(self.avg.handle.ptr, self.diff.handle.ptr, *tail))
        else:
            eng._check(eng.lib.nss_scalar_flux_limited_f64(self.stencil.data_ptr(), self.n_u,
                                                           CONVECTION_SCHEMES[self.scheme], *tail))

    def launch_ab2(self, u, f, T, t_ref, weights, G_prev, G_ext, w_b=None, b_prev=None, f_eff=None):
        """G = the flux of `T` carried by `u`;  G_ext = w_new G + w_old G_prev;  G_prev = G; with the weights `w_b` also
        b = w_b (avg T - t_ref), f_eff = f + w_new b + w_old b_prev, b_prev = b.  `weights` = (w_new, w_old)."""
        eng = self.eng
        tail = (_ptr(w_b), u.data_ptr(), _ptr(f), T.data_ptr(), t_ref, weights[0], weights[1], G_prev.data_ptr(),
                G_ext.data_ptr(), _ptr(b_prev), _ptr(f_eff), None, eng.stream)
        if self.stencil is None:
            eng._check(eng.lib.nss_scalar_flux_ab2_f64(self.avg.handle.ptr, self.diff.handle.ptr, *tail))
        else:
            eng._check(eng.lib.nss_scalar_flux_limited_ab2_f64(self.stencil.data_ptr(), self.n_u,
                                                               CONVECTION_SCHEMES[self.scheme], *tail))


CONVECTION_TREATMENTS = ("explicit", "implicit")


def check_convection_treatment(treatment, who):
    if treatment not in CONVECTION_TREATMENTS:
        raise ValueError("%s: the convection treatment is \"explicit\" or \"implicit\", not %r" % (who, treatment))
    return treatment


def check_implicit_solve(who, inner_pre, implicit, variable, time_scheme, convection, convection_treatment,
                         projection="cg"):
    """The rules for the arguments of a stepper's implicit solve (``ValueError``), in the order of their messages:
    implicit convection goes with "euler", "upwind" and "jacobi" (any `inner_pre` once `implicit` is "fdm"); `implicit`
    is "cg" or "fdm"; variable steps take "jacobi" unless the solve is direct.  `who`: "ScalarStepper", whose messages
    carry its name, or "TimeStepper", which has the names of `inner_pre` and `projection` checked between the rules."""
    scalar = who == "ScalarStepper"
    prefix = "ScalarStepper: " if scalar else ""
    if convection_treatment == "implicit" and (time_scheme != "euler" or convection != "upwind" or
                                               (inner_pre != "jacobi" and implicit != "fdm")):
        raise ValueError(prefix + "implicit convection goes with time_scheme=\"euler\", convection=\"upwind\" and "
                         "inner_pre=\"jacobi\"")
    if not scalar and inner_pre not in ("jacobi", "amg"):
        raise ValueError("inner_pre is \"jacobi\" or \"amg\"")
    if projection not in ("cg", "fdm"):
        raise ValueError("projection is \"cg\" or \"fdm\"")
    if implicit not in ("cg", "fdm"):
        raise ValueError(prefix + "implicit is \"cg\" or \"fdm\"")
    if variable and inner_pre != "jacobi" and implicit != "fdm":
        raise ValueError(prefix + "a variable-step stepper takes inner_pre=\"jacobi\""
                         + ("" if scalar else ": a hierarchy belongs to one step size"))


class ImplicitSolve:
    """The implicit solve of one transported quantity, out = (M + sigma L)^-1 rhs with sigma = theta tau (theta = 1, or
    1/2 for "cnab2"): the velocity's (M_u, A, rows [A | D]) or the scalar's (M_p, K, rows [K | B]), of one `kind`:

      "cg"        `CgLoop` on the assembled M + theta timestep L (`assembled`) with `pre`, Jacobi or AMG (`inner_pre`)
      "shifted"   `CgLoop` on L itself with the shift (M, diag L): the sigma of each step, Jacobi written by `set_shift`
      "fdm"       the direct solve of the `ComponentFastDiagonalization` `fdm`: the sigma of each step, no iteration
      "bicgstab"  `fused.BicgstabLoop` on M + sigma (L + N(a)) read from `rows`: the advecting field `a` is allocated
                  here and written by the owner once per step; the preconditioner is the point-Jacobi diagonal `dinv`
                  of the whole operator or, given `fdm`, the direct viscous inverse

    Of `assembled`, `pre`, `cg`, `fdm`, `bicg`, `dinv`, `a`, those the kind does not use are not built and stay None.
    `lap`: L, the `SparseMatrix` the caller holds (the shifted loop runs on that very object) or a scipy matrix, which
    the shifted kind alone uploads (`keys["lap"]` of `shared`, beside `keys["assembled"]` and `keys["diag"]`, built when
    missing); `mass`: host array; `label`: the owner's name for the solve in the message of a breakdown."""

    assembled = pre = cg = fdm = bicg = dinv = a = None

    @staticmethod
    def kind_of(variable, implicit, convection_treatment):
        """The kind for a stepper's three switches; with implicit convection `implicit` names the preconditioner."""
        return "bicgstab" if convection_treatment == "implicit" else "fdm" if implicit == "fdm" else \
            "shifted" if variable else "cg"

    def __init__(self, eng, kind, label, inner_pre, timestep, theta, mass, lap, shared, keys, fdm=None, rows=None,
                 avg=None, diff=None):
        import scipy.sparse as sp
        self.kind, self.label, self.theta, self.fdm = kind, label, float(theta), fdm
        resident = isinstance(lap, SparseMatrix)
        if kind == "cg":                            # M + timestep L, or the half-step operator M + timestep/2 L
            if keys["assembled"] not in shared:
                host = sp.diags(mass) + self.theta * float(timestep) * (lap.to_scipy() if resident else lap)
                shared[keys["assembled"]] = SparseMatrix.from_scipy(host.tocsr(), engine=eng)
            self.assembled = shared[keys["assembled"]]
            self.pre = SmoothedAggregationAMG(self.assembled) if inner_pre == "amg" else JacobiPreconditioner(self.assembled)
            self.cg = CgLoop(eng, self.assembled, pre_for("cg", self.pre))
        elif kind == "shifted":
            if keys["diag"] not in shared:
                shared[keys["diag"]] = eng.from_host((lap.to_scipy() if resident else sp.csr_matrix(lap)).diagonal())
            if not resident:
                if keys["lap"] not in shared:
                    shared[keys["lap"]] = SparseMatrix.from_scipy(sp.csr_matrix(lap), engine=eng)
                lap = shared[keys["lap"]]
            self.cg = CgLoop(eng, lap, NO_PRE, shift=(mass, shared[keys["diag"]]))
        elif kind == "bicgstab":
            self.a = eng.zeros(max(1, avg.height))
            form = fused.ConvectiveForm(rows, avg, diff, self.a, fused.ConvectiveForm.mass_operand(eng, mass))
            self.dinv = None if fdm is not None else eng.zeros(rows.height)
            self.bicg = fused.BicgstabLoop(eng, rows, self.dinv, form, fdm)

    def solve(self, rhs, out, tau, precision, maxsteps, step):
        """out = (M + theta `tau` L)^-1 rhs from zero (device buffers; "bicgstab": with the N(a) of the current `a`).
        Returns the iterations (0: the direct solve); a BiCGStab breakdown raises ``FloatingPointError`` naming `step`."""
        sigma = self.theta * tau                    # ("bicgstab" is an "euler" stepper's: theta = 1, its sigma is tau)
        if self.kind == "fdm":
            return self.fdm.solve_resident(rhs, out, sigma)
        if self.kind == "bicgstab":
            self.bicg.set_sigma(sigma)
            if self.dinv is not None:
                self.bicg.write_jacobi(self.dinv)
            its = self.bicg.solve_resident(rhs, out, precision, maxsteps)
            if self.bicg.code:
                raise FloatingPointError("Advance: %s of step %d broke down, code %d (%s)"
                                         % (self.label, step, self.bicg.code, self.bicg.CODES[self.bicg.code]))
            return its
        if self.kind == "shifted":
            self.cg.set_shift(sigma)
        return self.cg.solve_resident(rhs, out, precision, maxsteps)


class LinearisedConvection(BaseMatrix):
    """The operator of the linearly implicit (Picard-linearised) convection step as a protocol operator,

        y = m v + sigma (L v + Dv F(a; v)),     F(a; v)_i = a_i (Avg v)_i - |a_i| (Diff v)_i / 2,

    form (ii) of the BiCGStab loop (csrc/bicgstab.hip).  `system_ops`: dict of scipy matrices -- "avg", "diff" (flux
    points x n), "div" = Dv (n x flux points) and, for the velocity, "adv" = I_adv (`StokesSystem.convection_operators()`
    as it stands); without "adv" the advecting vector is the frozen operand itself (the scalar: the face velocities,
    with avg, diff of `scalar_operators` and "div" = B).  `mass`: host array m; `lap`: scipy L (A, or K).
    `freeze(u)` does a = I_adv u (one SpMV; a copy without "adv"); `sigma` is a property.  On the HIP engine with native
    operands `Mult` is the loop's own apply (``nss_bicgstab_apply_f64``: the flux launch and the rows of [L | Dv]) and
    `hipla.BiCGStabSolver` runs the device-resident loop on it; on any other engine the statements go through the
    protocol.  `jacobi()`: the point-Jacobi preconditioner of the whole operator for the current a and sigma (a
    `DiagonalMatrix`, the same object every time, rewritten in place)."""

    def __init__(self, system_ops, mass, lap, sigma=0.0, engine=None):
        import scipy.sparse as sp
        super().__init__()
        if engine is None:
            from .engine import get_engine
            engine = get_engine()
        self.engine = engine
        self.ops = {key: sp.csr_matrix(system_ops[key]) for key in ("adv", "avg", "diff", "div") if key in system_ops}
        self.lap = sp.csr_matrix(lap)
        self.mass_host = np.ascontiguousarray(mass, dtype=np.float64)
        self.n, self.nflux = self.ops["avg"].shape[1], self.ops["avg"].shape[0]
        if self.lap.shape != (self.n, self.n) or self.ops["div"].shape != (self.n, self.nflux) or \
                self.ops["diff"].shape != (self.nflux, self.n) or self.mass_host.shape != (self.n,):
            raise ValueError("LinearisedConvection: the shapes of avg, diff, div, lap and mass do not fit")
        self.sigma = sigma
        self.adv = SparseMatrix.from_scipy(self.ops["adv"], engine=engine) if "adv" in self.ops else None
        self.a = Vector(self.nflux, engine=engine)
        self._protocol = self._device = self._jacobi = None
        self._frozen = False

    @property
    def sigma(self):
        return self._sigma

    @sigma.setter
    def sigma(self, value):
        value = float(value)
        if not (value >= 0.0 and np.isfinite(value)):
            raise ValueError("LinearisedConvection: sigma is non-negative and finite, not %r" % (value,))
        self._sigma = value

    def Height(self):
        return self.n

    def Width(self):
        return self.n

    def freeze(self, u):
        """a = I_adv u (without "adv": a = u), held until the next call."""
        if self.adv is not None:
            self.a.data = self.adv * u
        else:
            self.a.data = u
        self._frozen = True

    def device_form(self):
        """The `fused.ConvectiveForm` of the operator on the HIP engine (built on first use), or None: another engine,
        ``fused.ENABLED`` off, a library without the loop, or a row of avg or diff with more than two entries."""
        import scipy.sparse as sp
        eng = self.engine
        if not fused.ENABLED or not _hip(eng) or not hasattr(eng.lib, "nss_bicgstab_apply_f64") or \
                ConvectiveFlux.declined(self.ops, ("avg", "diff")) is not None or not isinstance(self.a, Vector):
            return None
        if self._device is None:
            rows = sp.hstack([self.lap, self.ops["div"]], format="csr")
            rows.sort_indices()
            form = fused.ConvectiveForm(SparseMatrix.from_scipy(rows, engine=eng),
                                        SparseMatrix.from_scipy(self.ops["avg"], engine=eng),
                                        SparseMatrix.from_scipy(self.ops["diff"], engine=eng), self.a.buf,
                                        fused.ConvectiveForm.mass_operand(eng, self.mass_host))
            self._device = (form, fused.BicgstabLoop(eng, form.rows, form=form, op=self), eng.zeros(self.n + self.nflux))
        return self._device[0]

    def _statements(self):
        if self._protocol is None:
            eng = self.engine
            self._protocol = dict(avg=SparseMatrix.from_scipy(self.ops["avg"], engine=eng),
                                  diff=SparseMatrix.from_scipy(self.ops["diff"], engine=eng),
                                  div=SparseMatrix.from_scipy(self.ops["div"], engine=eng),
                                  lap=SparseMatrix.from_scipy(self.lap, engine=eng),
                                  mass=DiagonalMatrix(self.mass_host, engine=eng))
            self._protocol.update(work=[self._protocol["avg"].CreateColVector() for _ in range(3)])
        return self._protocol

    def Mult(self, x, y):
        if not self._frozen:
            raise ValueError("LinearisedConvection: freeze(u) comes before the first product")
        if isinstance(x, Vector) and isinstance(y, Vector) and self.device_form() is not None:
            _, loop, operand = self._device
            loop.set_sigma(self._sigma)
            self.engine.copy(x.buf, self.engine.view(operand, 0, self.n))
            loop.apply(operand, y.buf)
            return
        p = self._statements()
        avg, dif, flux = p["work"]
        avg.data = p["avg"] * x
        dif.data = p["diff"] * x
        flux.engine.upwind_flux(self.a.buf, avg.buf, dif.buf, flux.buf)
        y.data = p["mass"] * x
        y.data += self._sigma * (p["lap"] * x)
        y.data += self._sigma * (p["div"] * flux)

    def to_scipy(self, a=None):
        """The operator assembled on the host for the frozen a (or the host array `a`): what tests hand to spsolve."""
        import scipy.sparse as sp
        a = self.a.numpy() if a is None else np.asarray(a, dtype=np.float64)
        conv = self.ops["div"] @ (sp.diags(a) @ self.ops["avg"] - sp.diags(0.5 * np.abs(a)) @ self.ops["diff"])
        return (sp.diags(self.mass_host) + self._sigma * (self.lap + conv)).tocsr()

    def jacobi(self):
        """The inverse diagonal of the operator for the current a and sigma: one launch on the device
        (``nss_bicgstab_jacobi_f64``), the assembled diagonal on the host otherwise."""
        if not self._frozen:
            raise ValueError("LinearisedConvection: freeze(u) comes before jacobi()")
        if self._jacobi is None:
            self._jacobi = DiagonalMatrix(np.ones(self.n), engine=self.engine)
        if self.device_form() is not None:
            loop = self._device[1]
            loop.set_sigma(self._sigma)
            loop.write_jacobi(self._jacobi.d)
        else:
            self.engine.upload(1.0 / self.to_scipy().diagonal(), self._jacobi.d)
        return self._jacobi


class StepRecord:
    """What `NavierStokes.Advance` returns: one entry per step of `mstar_iterations`, `proj_iterations` (pseudo time
    stepping: the two projections of a step added), `div_norm` = |B u| and `kinetic_energy` = <u, M_u u> / 2 after the
    step (both None with ``diagnostics=False``); `declined`: why the statements ran instead of the device-resident
    step (None when it ran); `flux_declined`: why the convection term ran through `ConvectionOperator`.  With a scalar
    (`NavierStokes.AddScalar`): `scalar_iterations` of the temperature solve and `wall_flux` = the heat entering through
    its `flux_wall` after the step (None without a scalar / diagnostics).  `convection`: the momentum flux's scheme;
    `time_scheme`: "euler" or "cnab2" (the pseudo time stepping is a relaxation and records "euler").  With a
    variable-step argument of `Advance` (None otherwise): `timestep` = the step sizes tau_n, `time` = their running sum
    within the call, `cfl` = tau_n * rate(u^n), and with `cfl=` also `limited_by` = the codes of `choose_timestep`.
    `projection`: "cg", or "fdm" -- the direct solve of `NavierStokes.SetProjection("fdm")`, whose `proj_iterations` are
    all zero.  `implicit`: "cg", or "fdm" -- the direct velocity and scalar solves of `NavierStokes.SetImplicitSolve("fdm")`,
    whose `mstar_iterations` and `scalar_iterations` are all zero.  `convection_treatment`: "explicit", or "implicit" --
    the linearly implicit convection of `NavierStokes.SetConvectionTreatment("implicit")`, whose `mstar_iterations` and
    `scalar_iterations` count BiCGStab iterations (with `implicit` = "fdm": preconditioned by the direct solve)."""

    def __init__(self, mstar_iterations, proj_iterations, div_norm, kinetic_energy, declined=None, flux_declined=None,
                 scalar_iterations=None, wall_flux=None, convection="upwind", time_scheme="euler", timestep=None,
                 time=None, cfl=None, limited_by=None, projection="cg", implicit="cg", convection_treatment="explicit"):
        self.timestep, self.time, self.cfl, self.limited_by = timestep, time, cfl, limited_by
        self.projection, self.implicit = projection, implicit
        self.convection_treatment = convection_treatment
        self.mstar_iterations = np.asarray(mstar_iterations, dtype=np.int64)
        self.proj_iterations = np.asarray(proj_iterations, dtype=np.int64)
        self.div_norm, self.kinetic_energy = div_norm, kinetic_energy
        self.declined, self.flux_declined = declined, flux_declined
        self.scalar_iterations = None if scalar_iterations is None else np.asarray(scalar_iterations, dtype=np.int64)
        self.wall_flux = wall_flux
        self.convection = convection
        self.time_scheme = time_scheme


class CflRate:
    """The CFL rate kernel (``nss_step_cfl_f64``): max_r w_r sum_p |B_rp| |u_p| over the rows of `B`, w = 1 / `m_p` (host
    array of the lumped pressure mass; None: ones; uniform: passed by value) -- on the plain grid
    max_cell sum_faces |u_f| / h, the CFL number of u per unit of step size."""

    def __init__(self, eng, B, m_p=None):
        self.eng, self.lib, self.B = eng, eng.lib, B
        w = np.ones(B.height) if m_p is None else 1.0 / np.asarray(m_p, dtype=np.float64)
        if w.shape != (B.height,):
            raise ValueError("CflRate: the mass holds %s entries, B %d rows" % (w.shape, B.height))
        uniform = bool(w.size) and bool((w == w[0]).all())
        self.inv_mass, self.scale = (None, float(w[0])) if uniform else (eng.from_host(w), 0.0)
        count = C.c_int64()
        eng._check(self.lib.nss_step_cfl_workspace(B.handle.ptr, C.byref(count)))
        self.partials = eng.zeros(max(1, count.value))
        self.out = eng.zeros(1)

    def launch(self, u, out, slot):
        """out[slot] = the rate of the device buffer `u`."""
        eng = self.eng
        eng._check(self.lib.nss_step_cfl_f64(self.B.handle.ptr, u.data_ptr(), _ptr(self.inv_mass), self.scale,
                                             self.partials.data_ptr(), self.partials.numel(), out.data_ptr(), slot, None,
                                             eng.stream))

    def __call__(self, u):
        """The rate of the device buffer `u`, read back."""
        self.launch(u, self.out, 0)
        return float(self.eng.to_host(self.out)[0])


class TimeStepper(FusedLoop):
    """Device-resident IMEX time stepping (``nss_step_*`` around two `CgLoop` solves): the statements of the reference's
    DoTimeStep / Project (templates/NavierStokesSIMPLE_iterative.py:424-443) and of its pseudo time stepping (:406-417).

    Per step: the flux kernel writes F behind u in the operand buffer [u | F]; one launch over the rows of [A | D] forms
    temp = f - A u - D F; raw = mstar^-1 temp (CG from zero); rhs = B raw; phi = (B M_u^-1 B^T)^-1 rhs (CG from zero); one
    launch over the rows of C = M_u^-1 B^T forms raw - C phi, u += timestep * that and the partials of <u, M_u u>; with
    diagnostics one launch over the rows of B gives the partials of |B u|^2 and one workgroup writes the step's record.
    Every buffer is allocated here, once; the only host synchronisations of a step are the polls of the two solves.

    `time_scheme="cnab2"` (second order): the operand is [u | F_ext | q] with the accumulated
    pressure q, the flux launch is the extrapolating one (F_ext = w_new F + w_old F_prev, F_prev = F), one launch over the
    rows of [A | D | B^T] forms temp = f - A u - D F_ext - B^T q, mstar is M_u + timestep/2 A, and one AXPY does
    q += phi after the projection tail.  `advance` then takes the object's `TimeHistory`.

    `projection="fdm"`: phi comes from the 2 dim launches of ``nss_fdm_solve_f64`` in the place of
    the second CG -- no iteration, no poll; the step then waits for the host in the velocity solve alone.

    `implicit="fdm"`: raw comes from the 2 dim launches of ``nss_fdmc_solve_f64`` in the place of
    the first CG, for every step size through the sigma of the launch; with both switches at "fdm" a fixed-step call has
    no host poll between its first launch and its read-back."""

    PRECISION, MAXSTEPS = (1e-4, 1e-8), (500, 5000)        # those of the template's CGSolvers invmstar / invproj
    momentum_flux = AD = adv = avg = diff = stencil = None # with `flux_declined`: no flux object, no flux operands
    nflux = 0
    cg_m, pre_m, mstar, fdm_u, bicg_m, dinv_m = (          # the parts of `solve_m`, where tests and tools read them
        property(lambda self, p=p: getattr(self.solve_m, p)) for p in ("cg", "pre", "assembled", "fdm", "bicg", "dinv"))

    @classmethod
    def try_create(cls, system, A, B, f, timestep, m_u, inner_pre="jacobi", conv_operator=None, shared=None,
                   convection="upwind", time_scheme="euler", variable=False, m_p=None, projection="cg", implicit="cg",
                   convection_treatment="explicit"):
        """`system`: the `StokesSystem` (its `convection_operators`); `A`, `B`: `SparseMatrix`; `f`: `Vector`;
        `m_u`: host array, the lumped velocity mass; `inner_pre`: "jacobi" | "amg", the preconditioner of both inner
        solves; `conv_operator`: callable giving the protocol `ConvectionOperator`, used when the flux kernel declines
        the convection operators (`flux_declined`).  `shared`: a dict in which the stepper looks up, and leaves, the
        device matrices that do not depend on `inner_pre` (mstar, Lp, C, adv, avg, diff, AD), so that the steppers of
        one system -- and a caller that already holds `M_u + timestep A`, `B M_u^-1 B^T`, `M_u^-1 B^T` and passes them
        under "mstar", "Lp", "C" -- keep them once.  `convection`: the scheme of F1 (`MomentumFlux`), "upwind" (donor
        cell, first order) or the second-order limited "minmod" / "vanleer".  `time_scheme`: "euler" or "cnab2"; a "cnab2"
        stepper keeps its matrices under keys of their own ("mhalf", "ADBt") and declines when the flux kernel declines the
        convection operators.  `m_p`: host array, the lumped pressure mass of the rate kernel (None: ones).  `projection`:
        "cg", or "fdm" -- `project` then launches the direct solve ``nss_fdm_solve_f64`` of a
        `hipla.fdm.FastDiagonalization` of Lp over the extents (system.n,) * system.dim, kept under "fdm" in `shared` (built
        when missing; the stepper declines with the reason when Lp is no Kronecker sum), and neither `cg_p` nor `pre_p`
        -- for "amg": the hierarchy of Lp -- is built.  `variable`, `implicit` ("cg" | "fdm") and `convection_treatment`
        ("explicit" | "implicit") choose the kind of the velocity solve `solve_m` (`ImplicitSolve`; the combinations:
        `check_implicit_solve`), with theta = 1 ("euler") or 1/2 ("cnab2").  The direct solve is that of a
        `hipla.fdm.ComponentFastDiagonalization` of A over `system.component_ids`, kept under "fdm_u" in `shared` (built
        when missing; the stepper declines with the reason when A does not factor); `inner_pre` then concerns a "cg"
        projection alone.  With implicit convection a = I_adv u^n is frozen once per step.  None: see `last_declined`."""
        return cls._decided(cls._try_create(system, A, B, f, timestep, m_u, inner_pre, conv_operator, shared, convection,
                                            time_scheme, variable, m_p, projection, implicit, convection_treatment))

    @staticmethod
    def _projection_matrices(eng, B, m_u, shared):
        """C = M_u^-1 B^T and Lp = B C into `shared`, where missing."""
        import scipy.sparse as sp
        if "C" not in shared:
            shared["C"] = SparseMatrix.from_scipy((sp.diags(1.0 / m_u) @ B.to_scipy().T).tocsr(), engine=eng)
        if "Lp" not in shared:
            lap_p = (B.to_scipy() @ shared["C"].to_scipy()).tocsr()
            lap_p.sort_indices()
            shared["Lp"] = SparseMatrix.from_scipy(lap_p, engine=eng)

    @classmethod
    def _try_create(cls, system, A, B, f, timestep, m_u, inner_pre, conv_operator, shared, convection, time_scheme,
                    variable=False, m_p=None, projection="cg", implicit="cg", convection_treatment="explicit"):
        check_convection_treatment(convection_treatment, "TimeStepper")
        check_implicit_solve("TimeStepper", inner_pre, implicit, variable, time_scheme, convection, convection_treatment,
                             projection)
        check_convection(convection, "TimeStepper")
        check_time_scheme(time_scheme, "TimeStepper")
        if not fused.ENABLED:
            return "fused loops disabled (hipla.fused.ENABLED)"
        if not isinstance(A, SparseMatrix) or not isinstance(B, SparseMatrix) or not isinstance(f, Vector):
            return "A, B are not SparseMatrix operands or f is not a plain Vector"
        if not _hip(A.engine) or not MomentumFlux.available(A.engine, "upwind"):
            return "not the HIP engine"
        if not MomentumFlux.available(A.engine, convection):
            return "the library has no limited flux kernel"
        shared = {} if shared is None else shared
        if time_scheme == "cnab2":
            if not MomentumFlux.available_ab2(A.engine, convection):
                return "the library has no extrapolating flux kernel"
            if "flux_declined" not in shared:
                shared["flux_declined"] = MomentumFlux.declined(system.convection_operators())
            if shared["flux_declined"] is not None:
                return "cnab2: the flux kernel declines the convection operators: " + shared["flux_declined"]
        if convection_treatment == "implicit":
            if not hasattr(A.engine.lib, "nss_bicgstab_iterate"):
                return "the library has no BiCGStab loop"
            if "flux_declined" not in shared:
                shared["flux_declined"] = MomentumFlux.declined(system.convection_operators())
            if shared["flux_declined"] is not None:
                return "implicit convection: the flux kernel declines the convection operators: " + shared["flux_declined"]
        if variable and not hasattr(A.engine.lib, "nss_step_cfl_f64"):
            return "the library has no CFL rate kernel"
        if projection == "fdm" and shared.get("fdm") is None:
            if not fdm.available(A.engine):
                return "the library has no fast diagonalisation"
            cls._projection_matrices(A.engine, B, np.asarray(m_u, dtype=np.float64), shared)
            made = fdm.FastDiagonalization.try_create(shared["Lp"], (system.n,) * system.dim, A.engine)
            if made is None:
                return "fdm: " + fdm.FastDiagonalization.last_declined
            shared["fdm"] = made
        if implicit == "fdm" and shared.get("fdm_u") is None:
            if not fdm.components_available(A.engine):
                return "the library has no fast diagonalisation on components"
            made = fdm.ComponentFastDiagonalization.try_create(A, system.component_ids, np.asarray(m_u, dtype=np.float64),
                                                               float(timestep), A.engine)
            if made is None:
                return "fdm: " + fdm.ComponentFastDiagonalization.last_declined
            shared["fdm_u"] = made
        return cls(system, A, B, f, timestep, m_u, inner_pre, conv_operator, shared, convection, time_scheme, variable,
                   m_p, projection, implicit, convection_treatment)

    def __init__(self, system, A, B, f, timestep, m_u, inner_pre, conv_operator, shared, convection="upwind",
                 time_scheme="euler", variable=False, m_p=None, projection="cg", implicit="cg",
                 convection_treatment="explicit"):
        import scipy.sparse as sp
        eng = self.eng = A.engine
        self.time_scheme, self.variable = time_scheme, bool(variable)
        self.projection, self.implicit = projection, implicit
        self.convection_treatment = convection_treatment
        self.fdm = shared["fdm"] if projection == "fdm" else None
        if self.fdm is not None and self.fdm.handle is None:
            raise ValueError("TimeStepper: the FastDiagonalization holds no device handle")
        fdm_u = shared["fdm_u"] if implicit == "fdm" else None
        if fdm_u is not None and fdm_u.handle is None:
            raise ValueError("TimeStepper: the ComponentFastDiagonalization holds no device handle")
        cnab2 = time_scheme == "cnab2"
        rows_key, mstar_key = ("ADBt", "mhalf") if cnab2 else ("AD", "mstar")
        self.lib, self.A, self.B, self.f, self.timestep = eng.lib, A, B, f, float(timestep)
        self.n_u, self.n_p = A.height, B.height
        m_u = np.asarray(m_u, dtype=np.float64)
        # ---- the convection term: the flux object of the scheme and the rows of [A | D] ----
        self.convection = convection
        ops = None if {"flux_declined", rows_key} <= shared.keys() else system.convection_operators()
        if "flux_declined" not in shared:
            shared["flux_declined"] = MomentumFlux.declined(ops)
        self.flux_declined = shared["flux_declined"]
        if self.flux_declined is None:
            mf = self.momentum_flux = MomentumFlux(eng, system, convection, shared, ops)
            if rows_key not in shared:              # [A | D], or [A | D | B^T] over the operand [u | F_ext | q]
                AD = sp.hstack([A.to_scipy(), ops["div"]] + ([B.to_scipy().T] if cnab2 else []), format="csr")
                AD.sort_indices()
                shared[rows_key] = SparseMatrix.from_scipy(AD, engine=eng)
            self.AD, self.conv = shared[rows_key], None
            self.adv, self.avg, self.diff, self.stencil, self.nflux = mf.adv, mf.avg, mf.diff, mf.stencil, mf.nflux
        else:
            self.conv = conv_operator()
        self.uf = eng.zeros(self.n_u + self.nflux + (self.n_p if cnab2 else 0))      # the operand [u | F] or [u | F_ext | q]
        self.u, self.F = eng.view(self.uf, 0, self.n_u), eng.view(self.uf, self.n_u, self.n_u + self.nflux)
        if cnab2:
            self.q = eng.view(self.uf, self.n_u + self.nflux, self.n_u + self.nflux + self.n_p)
            self.F_prev = eng.zeros(max(1, self.nflux))
        self.temp, self.raw, self.temp2 = eng.zeros(self.n_u), eng.zeros(self.n_u), eng.zeros(self.n_u)
        self.rhs_p, self.phi = eng.zeros(self.n_p), eng.zeros(self.n_p)
        # ---- the inner solves ----
        kind = ImplicitSolve.kind_of(variable, implicit, convection_treatment)
        self.solve_m = ImplicitSolve(eng, kind, "the velocity solve", inner_pre, self.timestep, 0.5 if cnab2 else 1.0, m_u,
                                     A, shared, dict(assembled=mstar_key, diag="diagA"), fdm_u, self.AD, self.avg, self.diff)
        if kind == "bicgstab":                      # (a breakdown of a scalar's solve puts the step's u and phi back)
            self.u_back, self.phi_back = eng.zeros(self.n_u), eng.zeros(self.n_p)
        self._projection_matrices(eng, B, m_u, shared)
        self.Lp, self.C = shared["Lp"], shared["C"]
        if "singular" not in shared:
            ok, why = two_entry_rows(self.C.to_scipy())
            if not ok:
                raise ValueError("TimeStepper: M_u^-1 B^T: " + why)
            shared["singular"] = constants_in_kernel(self.Lp.to_scipy())
        self.singular = shared["singular"]
        # The projection: direct (no cg_p, no pre_p), else CG with Jacobi or the hierarchy of Lp (never beside "shifted").
        self.pre_p = self.cg_p = None
        if self.fdm is None:
            self.pre_p = JacobiPreconditioner(self.Lp) if inner_pre != "amg" or kind == "shifted" else \
                SmoothedAggregationAMG(self.Lp, nullspace="constants" if self.singular else None)
            self.cg_p = CgLoop(eng, self.Lp, pre_for("cg", self.pre_p))
        if variable:
            self.rate = CflRate(eng, B, m_p)
        # ---- the record ----
        uniform = bool(m_u.size) and bool((m_u == m_u[0]).all())
        self.mass = None if uniform else eng.from_host(m_u)
        self.energy_scale = 0.5 * (float(m_u[0]) if uniform else 1.0)
        self.partials_e = self.partials_d = None
        self._fit_partials()

    def _fit_partials(self):
        """The partials of the record for the CURRENT launch plan of C (row blocks) and the size of B."""
        ne, nd = C.c_int64(), C.c_int64()
        self.eng._check(self.lib.nss_step_workspace(self.C.handle.ptr, self.B.handle.ptr, C.byref(ne), C.byref(nd)))
        if self.partials_e is None or self.partials_e.numel() < ne.value or self.partials_d.numel() < nd.value:
            self.partials_e, self.partials_d = self.eng.zeros(max(1, ne.value)), self.eng.zeros(max(1, nd.value))
        self.n_energy, self.n_div = ne.value, nd.value

    # ---- the launches of a step -----------------------------------------------------------------------------------
    def right_hand_side(self, f=None):
        """temp = conv(u) + f - A u from the u part of the operand buffer; `f`: the force of this step (a buffer: the
        f_eff of a buoyant scalar), None = the stepper's f."""
        eng, lib = self.eng, self.lib
        f = self.f.buf if f is None else f
        if self.flux_declined is None:
            if self.time_scheme == "cnab2":
                self.momentum_flux.launch_ab2(self.u, self.weights, self.F_prev, self.F)
            else:
                self.momentum_flux.launch(self.u, self.F)
            eng._check(lib.nss_step_rhs_f64(self.AD.handle.ptr, self.uf.data_ptr(), f.data_ptr(),
                                            self.temp.data_ptr(), None, eng.stream))
            return
        u, temp = Vector(buf=self.u, engine=eng), Vector(buf=self.temp, engine=eng)
        temp.data = self.conv * u
        temp.data += Vector(buf=f, engine=eng)
        temp.data += -self.A * u

    def project(self, vel, out=None, update=None, energy=False, tau=None):
        """out = vel - C phi with phi = (B M_u^-1 B^T)^-1 B vel (`Project`; `out` None: in place); `update`:
        u += tau * out in the same launch (`tau` None: the stepper's timestep); `energy`: also the partials of
        <e, M_u e>, e = the updated u, or out.
        Returns the CG iterations (0 for the direct solve of a "fdm" stepper, which ignores precision and maxsteps)."""
        eng, lib = self.eng, self.lib
        eng.csr_spmv(self.B.handle, 1.0, vel, 0.0, self.rhs_p)
        if self.fdm is not None:
            its = self.fdm.solve_resident(self.rhs_p, self.phi)
        else:
            its = self.cg_p.solve_resident(self.rhs_p, self.phi, self.precision[1], self.maxsteps[1])
        eng._check(lib.nss_step_project_f64(self.C.handle.ptr, self.phi.data_ptr(), vel.data_ptr(),
                                            (vel if out is None else out).data_ptr(), _ptr(update),
                                            self.timestep if tau is None else tau,
                                            _ptr(self.mass), self.partials_e.data_ptr() if energy else None,
                                            self.partials_e.numel(), None, eng.stream))
        return its

    def write_record(self, record, slot):
        eng, lib = self.eng, self.lib
        eng._check(lib.nss_step_divergence_f64(self.B.handle.ptr, self.u.data_ptr(), self.partials_d.data_ptr(),
                                               self.partials_d.numel(), None, eng.stream))
        eng._check(lib.nss_step_record_f64(self.partials_e.data_ptr(), self.n_energy, self.partials_d.data_ptr(),
                                           self.n_div, self.energy_scale, record.data_ptr(), slot, None, eng.stream))

    def advance(self, gfu, gfup, nsteps, precision=None, maxsteps=None, diagnostics=True, pseudo=False, scalar=None,
                temperature=None, history=None, timesteps=None, controller=None, clock=None):
        """`nsteps` steps on the velocity `gfu` (pressure-like potential of the last projection -> `gfup`).
        `precision` / `maxsteps`: one value for both inner solves, a pair (mstar, projection), or None = the template's.
        `scalar`: a `ScalarStepper` -- every step then begins with its flux launch on (u^n, T^n), the velocity step
        takes its f_eff for f (a buoyant scalar), and its temperature step follows; `temperature`: the `Vector` of T.
        A "cnab2" stepper: `gfup` is the accumulated pressure q, copied into the operand on entry and out on exit, and
        `history` the object's `TimeHistory`, copied in and out once (the valid flags are updated).

        A variable-step stepper takes `timesteps` (`nsteps` prescribed sizes) or `controller` (a `StepController`) and
        `clock`, the `TimeHistory` that holds `tau_prev` (`history` itself for "cnab2").  Every step begins with the rate
        launch on u^n into rates[step]; with a controller the host reads that one double back and chooses tau_n.  The
        sigma of the shifted solves, tau_n and the AB2 weights (1 + r/2, -r/2) go to the launches by value."""
        self.precision = tuple(float(p) for p in pair(precision, self.PRECISION))
        self.maxsteps = tuple(int(m) for m in pair(maxsteps, self.MAXSTEPS))
        eng = self.eng
        self._fit_partials()
        nsteps = int(nsteps)
        if scalar is not None and pseudo:
            raise ValueError("advance: the pseudo time stepping carries no scalar")
        cnab2 = self.time_scheme == "cnab2"
        if cnab2 and (pseudo or history is None):
            raise ValueError("advance: a \"cnab2\" stepper takes the object's history and does no pseudo time stepping")
        if cnab2 and scalar is not None and scalar.time_scheme != "cnab2":
            raise ValueError("advance: the scalar stepper is not a \"cnab2\" one")
        if self.variable != (timesteps is not None or controller is not None):
            raise ValueError("advance: a variable-step stepper, and no other, takes timesteps or a controller")
        if self.variable and (pseudo or (clock is None and history is None)):
            raise ValueError("advance: variable steps want the clock and do no pseudo time stepping")
        if self.variable and scalar is not None and not scalar.variable:
            raise ValueError("advance: the scalar stepper is not a variable-step one")
        implicit_conv = self.solve_m.kind == "bicgstab"
        if implicit_conv and (pseudo or (scalar is not None and scalar.solve_T.kind != "bicgstab")):
            raise ValueError("advance: implicit convection does no pseudo time stepping and takes an implicit scalar stepper")
        if timesteps is not None:
            timesteps = [check_step_size(t, "advance") for t in timesteps]
            if len(timesteps) != nsteps or controller is not None:
                raise ValueError("advance: timesteps holds one size per step, and excludes a controller")
        slots = max(1, nsteps)                 # the record: [2 slots] of the velocity | [slots] of the scalar | [slots] rates
        nrec = (2 if scalar is None else 3) * slots if diagnostics else 0
        buf = eng.zeros(nrec + (slots if self.variable else 0)) if diagnostics or self.variable else None
        record = eng.view(buf, 0, nrec) if diagnostics else None
        rates = eng.view(buf, nrec, nrec + slots) if self.variable else None
        record_s = eng.view(record, 2 * slots, 3 * slots) if diagnostics and scalar is not None and scalar.records else None
        eng.copy(gfu.buf, self.u)
        if scalar is not None:
            eng.copy(temperature.buf, scalar.T)
        if cnab2:
            eng.copy(gfup.buf, self.q)
            if history.valid["momentum"] and self.nflux:
                eng.copy(history.F_prev.buf, eng.view(self.F_prev, 0, self.nflux))
            if scalar is not None:
                scalar.load_history(history)
        its_m, its_p, its_s = [], [], None if scalar is None else []
        taus, codes, failure = [], None if controller is None else [], None
        clock = history if clock is None else clock                       # ("euler": the caller's, or none)
        tau_prev = None if clock is None else clock.tau_prev
        valid = dict(history.valid) if cnab2 else None
        if pseudo:
            self.project(self.u)                                          # :407  Project(gfu)
        for step in range(nsteps):
            tau = None                                                    # (None: the stepper's own timestep)
            if self.variable:
                self.rate.launch(self.u, rates, step)                     # R1, R2 on u^n
                if controller is None:
                    tau = timesteps[step]
                else:
                    try:
                        chosen = controller.next(float(eng.to_host(eng.view(rates, step, step + 1))[0]), tau_prev)
                    except FloatingPointError as err:
                        failure = err
                        break
                    if chosen is None:
                        break
                    tau = chosen[0]
                    codes.append(chosen[1])
                taus.append(tau)
            size = self.timestep if tau is None else tau
            if pseudo:
                eng.csr_spmv(self.A.handle, -1.0, self.u, 0.0, self.temp)         # :411  temp = -A u
            elif cnab2:
                self.weights = TimeHistory.ab2_weights(valid["momentum"], size, tau_prev)
                force = None if scalar is None else \
                    scalar.flux_ab2(self.u, TimeHistory.ab2_weights(valid["scalar"], size, tau_prev))
                valid = dict.fromkeys(valid, True)
                self.right_hand_side(force)
            else:
                self.right_hand_side(None if scalar is None else scalar.flux(self.u))     # (S1,) F1, F2  :429-431
            if implicit_conv:
                if scalar is not None:              # (a breakdown of the scalar's solve puts this state back)
                    eng.copy(self.u, self.u_back)
                    eng.copy(self.phi, self.phi_back)
                if self.nflux:                      # a = I_adv u^n, frozen for the step
                    eng.csr_spmv(self.adv.handle, 1.0, self.u, 0.0, self.solve_m.a)
            try:                                    # :433  (the pseudo time stepping is an "euler" stepper's: theta = 1)
                its_m.append(self.solve_m.solve(self.temp, self.raw, size, self.precision[0], self.maxsteps[0], step))
            except FloatingPointError as err:       # (u is still u^n: the last finished step)
                failure = err
                break
            count = self.project(self.raw, out=self.temp2, update=self.u, energy=diagnostics and not pseudo,
                                 tau=tau)                                                                       # :434,438
            if pseudo:
                count += self.project(self.u, energy=diagnostics)                # :415  Project(gfu)
            its_p.append(count)
            if cnab2:
                eng.lincomb(self.q, [(1.0, self.q), (1.0, self.phi)])             # q += phi
            if diagnostics:
                self.write_record(record, step)
            if scalar is not None:
                try:
                    its_s.append(scalar.step(record_s, step, tau))                # S2, the solve, S3, S4
                except FloatingPointError as err:   # (implicit convection: T is still T^n; u and phi go back)
                    failure = err
                    eng.copy(self.u_back, self.u)
                    eng.copy(self.phi_back, self.phi)
                    its_m.pop()
                    its_p.pop()
                    break
            if not pseudo:
                tau_prev = size
        nsteps = len(its_m)                                               # (a duration may end the call early)
        if clock is not None and nsteps:
            clock.tau_prev = tau_prev
        eng.copy(self.u, gfu.buf)
        if cnab2 and nsteps:
            eng.copy(self.q, gfup.buf)
            if self.nflux:
                eng.copy(eng.view(self.F_prev, 0, self.nflux), history.vector("F_prev", self.nflux, eng).buf)
            history.valid["momentum"] = True
            if scalar is not None:
                scalar.store_history(history)
        elif not cnab2 and (nsteps or pseudo):
            eng.copy(self.phi, gfup.buf)
        if scalar is not None:
            eng.copy(scalar.T, temperature.buf)
        if failure is not None:                                           # the state of the last finished step is back
            raise failure
        div = energy = wall = None
        extra = {}
        if buf is not None:
            host = eng.to_host(buf)                                       # the one read-back
            if diagnostics:
                vel = host[:2 * slots].reshape(-1, 2)[:nsteps]
                div, energy = vel[:, 1].copy(), vel[:, 0].copy()
                if record_s is not None:
                    wall = host[2 * slots:3 * slots][:nsteps].copy()
            if self.variable:
                extra = variable_record(taus, host[nrec:], codes)
        return StepRecord(its_m, its_p, div, energy, flux_declined=self.flux_declined, convection=self.convection,
                          scalar_iterations=its_s, wall_flux=wall, time_scheme=self.time_scheme,
                          projection=self.projection, implicit=self.implicit,
                          convection_treatment=self.convection_treatment, **extra)


class ScalarStepper:
    """The scalar part of a device-resident step (``nss_scalar_*`` around one `CgLoop` solve), driven by
    `TimeStepper.advance`: M_p dT/dt = q - K T - B G with the donor-cell flux G of T through the faces and, for a
    buoyant scalar, the force f_eff = f + w_b (avg T - t_ref) of the velocity step.

    Per step: the flux launch on (u^n, T^n) writes G behind T in the operand buffer [T | G] (and f_eff); after the
    velocity step one launch over the rows of [K | B] forms temp_T = q - K T - B G; delta = (M_p + timestep K)^-1 temp_T
    (CG from zero); one launch does T += timestep delta with the partials of <w, T>, one workgroup writes the heat
    entering through the flux wall, c0 - <w, T>.  Every buffer is allocated here, once (the cost in HBM: DESIGN.md 12).

    `time_scheme="cnab2"`: the flux launch is the extrapolating one (G_ext behind T, f_eff = the force of the step, the
    histories G_prev and b_prev), and the solve is with M_p + timestep/2 K (key "mhalf")."""

    PRECISION, MAXSTEPS = 1e-4, 500          # those of invmstar: the same kind of operator
    cg, pre, mstar, fdm, bicg = (            # the parts of `solve_T`, where tests read them
        property(lambda self, p=p: getattr(self.solve_T, p)) for p in ("cg", "pre", "assembled", "fdm", "bicg"))

    def __init__(self, eng, ops, B, f, timestep, inner_pre="jacobi", w_b=None, t_ref=0.0, flux=None, precision=None,
                 maxsteps=None, shared=None, convection="upwind", stencil=None, time_scheme="euler", variable=False,
                 implicit="cg", extents=None, convection_treatment="explicit"):
        """`ops`: `StokesSystem.scalar_operators(...)`; `B`: the divergence (`SparseMatrix`); `f`: the force `Vector`
        the flux launch reads every step; `w_b`: host array of buoyancy weights (None: passive scalar); `flux`:
        (c0, w) of `ops["wall_flux"](wall)` or None; `shared`: dict for the device matrices that do not depend on
        `inner_pre`.  `convection`, `stencil`: the scheme of S1 and, for a limited one, `scalar_stencil()` (`ScalarFlux`).
        `variable`, `implicit` and `convection_treatment` choose the kind of the solve `solve_T` (`ImplicitSolve`) as for
        the velocity.  The direct solve is that of the `hipla.fdm.ComponentFastDiagonalization` of K over the cells, kept
        under "fdm_T" in `shared` (built when missing, over the grid `extents`; ``ValueError`` with the reason when K does
        not factor); the BiCGStab loop is on M_p + sigma (K + B G(u^n; .)), u^n copied by `flux`, and a breakdown makes
        `step` raise ``FloatingPointError`` before T is touched."""
        import scipy.sparse as sp
        shared = {} if shared is None else shared
        self.variable = bool(variable)
        check_convection_treatment(convection_treatment, "ScalarStepper")
        check_implicit_solve("ScalarStepper", inner_pre, implicit, variable, time_scheme, convection, convection_treatment)
        self.implicit = implicit
        self.time_scheme = check_time_scheme(time_scheme, "ScalarStepper")
        cnab2 = time_scheme == "cnab2"
        if cnab2 and not ScalarFlux.available_ab2(eng, convection):
            raise ValueError("ScalarStepper: the library has no extrapolating flux kernel")
        self.eng, self.lib, self.f, self.timestep, self.t_ref = eng, eng.lib, f, float(timestep), float(t_ref)
        self.n_u, self.n_p = ops["avg"].shape
        self.precision = self.PRECISION if precision is None else float(precision)
        self.maxsteps = self.MAXSTEPS if maxsteps is None else int(maxsteps)
        sf = self.scalar_flux = ScalarFlux(eng, ops, convection, stencil, shared)
        self.convection, self.stencil, self.avg, self.diff = sf.scheme, sf.stencil, sf.avg, sf.diff
        if "KB" not in shared:
            KB = sp.hstack([ops["K"], B.to_scipy()], format="csr")
            KB.sort_indices()
            shared["KB"] = SparseMatrix.from_scipy(KB, engine=eng)
            shared["q"] = eng.from_host(np.asarray(ops["q"], dtype=np.float64))
            shared["w_b"] = None if w_b is None else eng.from_host(np.asarray(w_b, dtype=np.float64))
            shared["w"] = None if flux is None else eng.from_host(np.asarray(flux[1], dtype=np.float64))
        if implicit == "fdm":
            if shared.get("fdm_T") is None:
                if extents is None or int(np.prod(extents, dtype=np.int64)) != self.n_p:
                    raise ValueError("ScalarStepper: implicit=\"fdm\" wants the grid extents of the %d cells" % self.n_p)
                made = fdm.ComponentFastDiagonalization.try_create(
                    sp.csr_matrix(ops["K"]), [np.arange(self.n_p).reshape(tuple(extents))], ops["mass"], self.timestep, eng)
                if made is None:
                    raise ValueError("ScalarStepper: fdm: " + fdm.ComponentFastDiagonalization.last_declined)
                shared["fdm_T"] = made
            if shared["fdm_T"].handle is None:
                raise ValueError("ScalarStepper: the ComponentFastDiagonalization holds no device handle")
        self.KB, self.q, self.w_b, self.w = (shared[key] for key in ("KB", "q", "w_b", "w"))
        self.solve_T = ImplicitSolve(eng, ImplicitSolve.kind_of(variable, implicit, convection_treatment),
                                     "the scalar's solve", inner_pre, self.timestep, 0.5 if cnab2 else 1.0, ops["mass"],
                                     ops["K"], shared, dict(assembled="mhalf" if cnab2 else "mstar", lap="K", diag="diagK"),
                                     shared["fdm_T"] if implicit == "fdm" else None, self.KB, self.avg, self.diff)
        self.c0, self.records = (0.0 if flux is None else float(flux[0])), flux is not None
        self.tg = eng.zeros(self.n_p + self.n_u)             # the operand [T | G]
        self.T, self.G = eng.view(self.tg, 0, self.n_p), eng.view(self.tg, self.n_p, self.n_p + self.n_u)
        self.f_eff = None if w_b is None else eng.zeros(self.n_u)
        if cnab2:
            self.G_prev = eng.zeros(self.n_u)
            self.b_prev = None if w_b is None else eng.zeros(self.n_u)
        self.temp, self.delta = eng.zeros(self.n_p), eng.zeros(self.n_p)
        count = C.c_int64()
        eng._check(self.lib.nss_scalar_workspace(self.n_p, C.byref(count)))
        self.n_partials = count.value
        self.partials = eng.zeros(max(1, count.value)) if self.records else None

    def flux(self, u):
        """S1 on (u, T): G, and for a buoyant scalar f_eff.  Returns the force buffer of the velocity step (None: f)."""
        self.scalar_flux.launch(u, self.f.buf, self.T, self.t_ref, self.G, self.w_b, self.f_eff)
        if self.solve_T.a is not None:
            self.eng.copy(u, self.solve_T.a)        # u^n, frozen for the scalar's solve behind the velocity step
        return self.f_eff

    def flux_ab2(self, u, weights):
        """S1 of a "cnab2" step: G_ext behind T, the histories, and for a buoyant scalar the force of the step in f_eff."""
        self.scalar_flux.launch_ab2(u, self.f.buf, self.T, self.t_ref, weights, self.G_prev, self.G, self.w_b, self.b_prev,
                                    self.f_eff)
        return self.f_eff

    def load_history(self, history):
        if history.valid["scalar"]:
            self.eng.copy(history.G_prev.buf, self.G_prev)
            if self.b_prev is not None:
                self.eng.copy(history.b_prev.buf, self.b_prev)

    def store_history(self, history):
        self.eng.copy(self.G_prev, history.vector("G_prev", self.n_u, self.eng).buf)
        if self.b_prev is not None:
            self.eng.copy(self.b_prev, history.vector("b_prev", self.n_u, self.eng).buf)
        history.valid["scalar"] = True

    def step(self, record, slot, tau=None):
        """S2, the solve, S3 and (with `record`) S4; `tau`: the size of a variable step (None: the stepper's timestep).
        Returns the CG iterations."""
        eng, lib = self.eng, self.lib
        size = self.timestep if tau is None else tau
        eng._check(lib.nss_step_rhs_f64(self.KB.handle.ptr, self.tg.data_ptr(), self.q.data_ptr(), self.temp.data_ptr(),
                                        None, eng.stream))
        its = self.solve_T.solve(self.temp, self.delta, size, self.precision, self.maxsteps, slot)
        write = record is not None
        eng._check(lib.nss_scalar_update_f64(self.n_p, size, self.delta.data_ptr(), self.T.data_ptr(),
                                             _ptr(self.w if write else None), _ptr(self.partials if write else None),
                                             self.partials.numel() if write else 0, None, eng.stream))
        if write:
            eng._check(lib.nss_scalar_record_f64(self.partials.data_ptr(), self.n_partials, self.c0, record.data_ptr(),
                                                 slot, None, eng.stream))
        return its


class HeatRecord:
    """What `heat.evolve` returns beside the temperature: `steps`; `cg_iterations[step, i]` = iterations of the i-th
    inner solve of the step; `orthogonality[step]` = the largest entry of |V^T V - I| after the orthonormalisation (None
    without ``diagnostics``); `declined`: why the statements ran through the protocol instead of the device-resident
    step (None when it ran)."""

    def __init__(self, cg_iterations, orthogonality, declined=None):
        self.steps = len(cg_iterations)
        self.cg_iterations = np.array([list(row) for row in cg_iterations], dtype=np.int64).reshape(self.steps, -1) \
            if self.steps and len(cg_iterations[0]) else np.zeros((self.steps, 0), dtype=np.int64)
        self.orthogonality = None if orthogonality is None else np.asarray(orthogonality, dtype=np.float64)
        self.declined = declined


class HeatIntegrator(FusedLoop):
    """Device-resident step of the heat exponential integrator (``nss_mgs_f64`` / ``nss_galerkin_f64`` /
    ``nss_basis_combine_f64`` around `CgLoop` solves): the statements of the reference's heat.py:87-142.

    The basis lives in ONE buffer of d planes (plane k = vector k, stride `ld`); plane 0 holds the temperature between
    steps.  Per step: d - 1 sub-steps (SpMV with K, CG from zero with ``M + time_step K``, one AXPY into the next plane),
    the Gram-Schmidt chain, two Galerkin launches, ONE read-back of the norms and the two d x d matrices, the small
    implicit Runge-Kutta step on the host, and one launch that combines the planes into plane 0 with the d coefficients
    as kernel arguments.  Every buffer is allocated here, once; a step waits for the host in the polls of its solves and
    in that read-back."""

    TRIES = 3                 # orthonormalize(basis, tries=3)

    @classmethod
    def try_create(cls, K, M, heat, pre, dimension, diagnostics=False):
        """`K`, `M`, `heat`: `SparseMatrix` (diffusion, mass, ``M + time_step K``); `pre`: the preconditioner of the inner
        solves (a protocol operator).  Returns None with the reason in ``HeatIntegrator.last_declined``."""
        return cls._decided(cls._try_create(K, M, heat, pre, dimension, diagnostics))

    @classmethod
    def _try_create(cls, K, M, heat, pre, dimension, diagnostics):
        if not fused.ENABLED:
            return "fused loops disabled (hipla.fused.ENABLED)"
        if not all(isinstance(m, SparseMatrix) and m.height == m.width == K.height for m in (K, M, heat)):
            return "K, M, heat are not square SparseMatrix operands of one size"
        if not _hip(K.engine) or not hasattr(K.engine.lib, "nss_mgs_f64"):
            return "not the HIP engine"
        if not 1 <= dimension <= 8:
            return "the subspace dimension is not in 1 .. 8"
        pa = pre_for("cg", pre)
        if pa is None or isinstance(pre, (ScaledMatrix, SumMatrix)):
            return "the preconditioner is not native"
        return cls(K, M, heat, pa, dimension, diagnostics)

    def __init__(self, K, M, heat, pa, dimension, diagnostics):
        eng = self.eng = K.engine
        self.lib, self.K, self.M, self.heat = eng.lib, K, M, heat
        n, d = K.height, int(dimension)
        self.n, self.d = n, d
        self.ld = -(-n // 32) * 32                           # planes start on 256-byte boundaries
        self.basis = eng.zeros(d * self.ld)
        self.planes = [eng.view(self.basis, k * self.ld, k * self.ld + n) for k in range(d)]
        self.res, self.sol = eng.zeros(n), eng.zeros(n)
        self.cg = CgLoop(eng, heat, pa)
        self.eye = None
        if diagnostics:
            import scipy.sparse as sp
            self.eye = SparseMatrix.from_scipy(sp.identity(n, format="csr"), engine=eng)
        # what a step reads back: [norms (TRIES * d) | V^T K V | V^T M V | V^T V (diagnostics)]
        self.out = eng.zeros(self.TRIES * d + (3 if diagnostics else 2) * d * d)
        count = C.c_int64()
        eng._check(self.lib.nss_heat_workspace(n, d, C.byref(count)))
        self.work = eng.zeros(count.value)

    def load(self, temperature):
        self.eng.upload(np.asarray(temperature, dtype=np.float64), self.planes[0])

    def temperature(self):
        return self.eng.to_host(self.planes[0]).copy()

    def _galerkin(self, mat, slot):
        eng, d = self.eng, self.d
        g = eng.view(self.out, self.TRIES * d + slot * d * d, self.TRIES * d + (slot + 1) * d * d)
        eng._check(self.lib.nss_galerkin_f64(mat.handle.ptr, d, self.ld, self.basis.data_ptr(), g.data_ptr(),
                                             self.work.data_ptr(), self.work.numel(), eng.stream))

    def build_subspace(self, dt, precision, maxsteps):
        """Planes 1 .. d - 1 from plane 0 (heat.py:95-98), the orthonormalisation (:100) and the Galerkin matrices
        (:109-118).  Returns (CG iterations, norms[TRIES, d], V^T K V, V^T M V, V^T V or None) after the one read-back."""
        eng, lib, d, planes = self.eng, self.lib, self.d, self.planes
        its = []
        for i in range(1, d):
            eng.csr_spmv(self.K.handle, 1.0, planes[i - 1], 0.0, self.res)
            its.append(self.cg.solve_resident(self.res, self.sol, precision, maxsteps))
            eng.lincomb(planes[i], [(1.0, planes[i - 1]), (-dt, self.sol)])
        eng._check(lib.nss_mgs_f64(self.n, d, self.ld, self.basis.data_ptr(), self.TRIES, self.out.data_ptr(),
                                   self.work.data_ptr(), self.work.numel(), eng.stream))
        self._galerkin(self.K, 0)
        self._galerkin(self.M, 1)
        if self.eye is not None:
            self._galerkin(self.eye, 2)
        host = eng.to_host(self.out)                                       # the one read-back
        norms = host[:self.TRIES * d].reshape(self.TRIES, d)
        mats = host[self.TRIES * d:].reshape(-1, d, d)
        return its, norms, mats[0], mats[1], mats[2] if self.eye is not None else None

    def combine(self, coefficients):
        """plane 0 = sum_i coefficients[i] * plane i (heat.py:140-142)."""
        coeff = (C.c_double * self.d)(*[float(c) for c in coefficients])
        self.eng._check(self.lib.nss_basis_combine_f64(self.n, self.d, self.ld, self.basis.data_ptr(), coeff,
                                                       self.planes[0].data_ptr(), self.eng.stream))
