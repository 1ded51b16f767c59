"""``NavierStokes`` with the reference's constructor / ``SolveInitial`` surface
(templates/NavierStokesSIMPLE_iterative.py:13-157,168-399), reduced to what the test and sweep
drivers exercise: the *iterative Stokes initial solve*, i.e. the hand-off

    BramblePasciakCG(blfA, blfB, None, f.vec, g.vec, preA, preM, sol,
                     initialize=False, tol=1e-10, maxsteps=100000, rel_err=True)          (:397)

with ``preA = MypreA(X2, blfA, blocks, GS)`` (:364-391) and ``preM = Preconditioner(mass, 'local')``
(:197-200).  ``MypreA`` is built the way the reference builds it:

* ``blocks`` = the free dofs of every mesh facet (:360-362) -> ``a.mat.CreateBlockSmoother(blocks)``;
* the auxiliary space (:150-157): one P1-like nodal space per velocity component, its ``nu``-scaled
  Laplacian ``aH1_c`` with ``Preconditioner(aH1_c, 'h1amg')`` (:320-351), stacked by ``Embedding``
  (:334-337,353-357) to ``preAh1``, and the ``transform`` from nodal fields to the facet unknowns
  (:208-291) -- FE machinery in the reference, here their grid restatement
  (``StokesSystem.auxiliary_space``);
* ``GS=False``: ``y = ((transform @ preAh1 @ transform.T) + jacobi) * x`` (:383);
  ``GS=True`` (the reference's default): ``y = 0; jacobi.Smooth(y, x); temp = x - mat*y;
  y += (transform @ preAh1 @ transform.T) * temp; jacobi.SmoothBack(y, x)`` (:376-381), the sweeps over a
  multicolour block ordering (scope row N1).
  Both forms are applied natively inside the fused BPCG loop (one ``nss_amg_create_auxiliary`` handle
  for the auxiliary term); ``aux=False`` drops the auxiliary term (block smoother only).

``DoTimeStep`` / ``Project`` / ``SolveInitial(timesteps=N)`` (:400-443, scope row N4) are the
reference's orchestration restated on the staggered-grid operators: ``invmstar`` = CG on
``M_u + timestep * A`` (:85-96), ``Project`` = pressure projection through CG on ``B M_u^-1 B^T``
(:115-144,440-443), explicit Euler update ``u += timestep * temp2`` (:438), and the explicit
convection term ``conv_operator * gfu`` (:106-113,427-431): conservative upwind fluxes
(``ConvectionOperator``: three SpMVs, the donor-cell flux kernel, one SpMV), or with
``NavierStokes(..., convection="minmod" | "vanleer")`` second-order limited upwind fluxes (one stencil launch, one SpMV).
``NavierStokes(..., time_scheme="cnab2")`` makes the step second order in time (not in the reference): Crank-Nicolson
for the viscous term, two-step Adams-Bashforth for convection and buoyancy, an incremental pressure in ``gfup``
(`NavierStokes._do_time_step_cnab2`).  ``CflRate()`` reports the CFL number of the current velocity
per unit of step size; ``DoTimeStep(timestep=)``, ``Advance(timesteps=)`` and ``Advance(cfl=)`` take steps of other
sizes than the constructor's, the last one chosen from that rate (not in the reference).
``SetProjection("fdm")`` replaces the CG solve of the projection by the direct solve of the fast diagonalisation method
(`hipla.FastDiagonalization`; not in the reference).  ``SetImplicitSolve("fdm")`` does the same for
the velocity solve and the scalar's (`hipla.ComponentFastDiagonalization`; not in the reference).
``SetConvectionTreatment("implicit")`` makes convection and the scalar's transport linearly implicit: the velocity solve
becomes a BiCGStab solve with ``M_u + timestep (A + N(a))``, a = I_adv u^n (`hipla.BiCGStabSolver`,
`hipla.stepping.LinearisedConvection`; not in the reference).

Out of scope: the MCS/HDG assembly itself and the sparse direct branch
``iterative=False`` (raises ``NotImplementedError``)."""

import numpy as np
import scipy.sparse as sp

import hipla
from hipla import BiCGStabSolver, BlockVector, CGSolver, ComponentFastDiagonalization, FastDiagonalization, fused
from hipla.stepping import (CflRate, LinearisedConvection, MomentumFlux, ScalarFlux, ScalarStepper, StepController,
                            StepRecord, TimeHistory, TimeStepper, check_convection, check_convection_treatment,
                            check_step_size, check_time_scheme, pair, variable_record)
from discretizations import AssembledForm, CondensedForm, SyntheticMesh, assemble, bdm_hybrid
from solvers.bramblepasciak_new import BramblePasciakCG

__all__ = ["NavierStokes", "SyntheticMesh", "MypreA", "coupling_blocks"]


class ConvectionOperator(hipla.BaseMatrix):
    """``conv_operator`` of the reference (templates/NavierStokesSIMPLE_iterative.py:106-113): the
    *nonlinear* map u -> conv(u), weak form of -div(u (x) u) with upwind fluxes, used as
    ``temp.data = conv_operator * gfu.vec`` (:429).  On the staggered grid: donor-cell fluxes
    ``F = adv*avg - |adv|*diff/2`` with ``adv = I_adv u``, ``avg = Avg u``, ``diff = Diff u`` (three
    SpMVs), then ``conv = -D F`` (one SpMV); all on the device.

    `scheme` "minmod" / "vanleer": the second-order limited fluxes ``F = adv * (U + s / 2)`` of
    `staggered_grid.limited_flux` over `system.convection_stencil()` -- one launch of a `hipla.stepping.MomentumFlux`,
    then ``-D F``; an engine without that kernel (the checker engine), or an `adv` the kernel refuses (a row of more than
    two entries, which no grid of this package produces), evaluates `system.limited_convection` on the host, uploaded."""

    def __init__(self, system, scheme="upwind"):
        super().__init__()
        self.scheme = check_convection(scheme, "ConvectionOperator")
        ops = system.convection_operators()
        self.n = system.n_u
        self.stencil = self.flux = None
        if scheme != "upwind":
            self.system = system
            self.div = hipla.SparseMatrix.from_scipy(ops["div"])
            eng = self.div.engine
            if MomentumFlux.available(eng, scheme) and MomentumFlux.declined(ops, ("adv",)) is None:
                self.flux = MomentumFlux(eng, system, scheme, {}, ops)
                self.stencil = self.flux.stencil
                self._work = self.flux.adv.CreateColVector()
            return
        self.adv, self.avg, self.diff, self.div = (hipla.SparseMatrix.from_scipy(ops[k])
                                                   for k in ("adv", "avg", "diff", "div"))
        self._work = [self.adv.CreateColVector() for _ in range(4)]

    def Height(self):
        return self.n

    def Width(self):
        return self.n

    def Flux(self, x, flux):
        """flux = F(x), the flux vector (length n_F) before ``-D``: ``Mult`` is ``y = -D F(x)``.  The second-order time
        stepping keeps its history in this form."""
        if self.scheme != "upwind":
            if self.flux is None:
                from staggered_grid import limited_flux
                stencil, adv, _ = self.system._limited_tables()
                u = x.numpy()
                flux.data = hipla.Vector.from_numpy(limited_flux(stencil, adv @ u, u, self.scheme))
                return
            self.flux.launch(x.buf, flux.buf)
            return
        adv, avg, diff, _ = self._work
        adv.data = self.adv * x
        avg.data = self.avg * x
        diff.data = self.diff * x
        flux.engine.upwind_flux(adv.buf, avg.buf, diff.buf, flux.buf)

    def Mult(self, x, y):
        if self.scheme != "upwind":
            if self.flux is None:
                y.data = hipla.Vector.from_numpy(self.system.limited_convection(x.numpy(), self.scheme))
                return
            self.flux.launch(x.buf, self._work.buf)
            y.data = -self.div * self._work
            return
        adv, avg, diff, flux = self._work
        adv.data = self.adv * x
        avg.data = self.avg * x
        diff.data = self.diff * x
        flux.engine.upwind_flux(adv.buf, avg.buf, diff.buf, flux.buf)
        y.data = -self.div * flux


def auxiliary_space_preconditioner(system, space=None, storage="fp64"):
    """``transform`` and ``preAh1`` of the reference (:208-357) on the grid restatement of the auxiliary
    space: returns (transform, preAh1, aux) with ``preAh1 = sum_c emb_c @ Preconditioner(aH1_c, 'h1amg') @
    emb_c.T`` as the protocol composition the reference writes (:336-337,357) and ``aux`` = the same
    operator ``transform @ preAh1 @ transform.T`` as one native handle (`hipla.AuxiliarySpaceAMG`).
    `storage` ("fp64" | "fp32"): the value storage of the term's matrices (T, T^T, the V-cycles' operators)."""
    if space is None:                  # (`space`: an assembled `system.auxiliary_space()`, so that callers can time the
        space = system.auxiliary_space()   #  host assembly of the auxiliary operators apart from the preconditioner set-up)
    transform = hipla.SparseMatrix.from_scipy(space["transform"])
    ndof = transform.width
    comps, preAh1 = [], None
    built = {}
    for lap, rng in zip(space["laplacians"], space["ranges"]):
        if id(lap) not in built:       # components with the same boundary conditions share one matrix: one hierarchy
            aH1 = AssembledForm(hipla.SparseMatrix.from_scipy(lap))
            built[id(lap)] = hipla.Preconditioner(aH1, "h1amg", storage=storage)   # :326-329,340-349
        pre_c = built[id(lap)]
        emb = hipla.Embedding(ndof, rng)                                 # :334-335,353-355
        term = emb @ pre_c @ emb.T
        preAh1 = term if preAh1 is None else preAh1 + term               # :337,357
        comps.append(pre_c)
    import os
    if os.environ.get("NSS_AUX_FORM", "components") == "stacked":
        # measurement variant: ONE V-cycle on the slab-major stacked block-diagonal Laplacian (what the row-partitioned
        # form applies): a third of the launches on the launch-bound coarse levels, no shared hierarchy
        st = system.auxiliary_space_stacked()
        stacked = hipla.Preconditioner(AssembledForm(hipla.SparseMatrix.from_scipy(st["laplacian"])), "h1amg",
                                       storage=storage)
        return transform, preAh1, hipla.AuxiliarySpaceAMG(hipla.SparseMatrix.from_scipy(st["transform"]), [stacked],
                                                          storage=storage)
    return transform, preAh1, hipla.AuxiliarySpaceAMG(transform, comps, storage=storage)


def MypreA(space, a, jacblocks, GS, aux=None, storage="fp64"):
    """``MypreA(space, a, jacblocks, GS)`` of the reference
    (templates/NavierStokesSIMPLE_iterative.py:364-391); `aux` is the auxiliary-space term
    ``transform @ preAh1 @ transform.T`` (an `hipla.AuxiliarySpaceAMG`, or any operator), ``None`` = block
    smoother only.

    * ``GS=False`` -> additive ``y = (aux + J) x`` with ``J = a.mat.CreateBlockSmoother(jacblocks)`` (:383);
    * ``GS=True``  -> ``y = 0; J.Smooth(y, x); r = x - A y; y += aux r; J.SmoothBack(y, x)`` (:376-381)
      over a multicolour block ordering (scope row N1).
    Both are native operands of the fused BPCG loop when `aux` is an `AuxiliarySpaceAMG` (or a
    `SmoothedAggregationAMG`); other operators run through the protocol.

    `storage` ("fp64" | "fp32"): the value storage of the Gauss-Seidel handle's matrices (`hipla.BlockGaussSeidel`);
    the additive block Jacobi stores no matrix and `aux` keeps the storage it was built with."""
    hipla.matrix.check_storage(storage)
    if GS:
        op = hipla.BlockGaussSeidel(a.mat, jacblocks, middle=aux, storage=storage)
        op.space, op.GS = space, True
        return op
    op = hipla.BlockJacobi(a.mat, jacblocks)
    op.space, op.GS = space, False
    return op if aux is None else aux + op


def coupling_blocks(blocks, interior):
    """The blocks (bs, nblocks; -1 = padding) restricted to the coupling dofs -- the ``FreeDofs(True)`` of a
    condensed form (:360-362): interior entries become padding, padding last, blocks left empty are dropped."""
    idx = np.array(blocks, dtype=np.int64, copy=True)
    idx[(idx >= 0) & np.asarray(interior)[np.maximum(idx, 0)]] = -1
    order = np.argsort(idx < 0, axis=0, kind="stable")  # padding last, the dofs of a block in their order
    idx = np.take_along_axis(idx, order, axis=0)
    return np.ascontiguousarray(idx[:, (idx >= 0).any(axis=0)], dtype=np.int32)


class ScalarField:
    """What `NavierStokes.AddScalar` keeps: the protocol operands of the scalar's statements in `DoTimeStep` (K, avg,
    diff, q, the CG inverse of M_p + timestep K, the buoyancy weights as a diagonal matrix) and what a device-resident
    `hipla.stepping.ScalarStepper` is made from."""

    def __init__(self, system, b_mat, timestep, kappa, dirichlet, buoyancy, t_ref, precision, maxsteps, flux_wall,
                 convection="upwind", time_scheme="euler"):
        self.convection = check_convection(convection, "AddScalar")
        self.time_scheme = time_scheme
        self.timestep = timestep
        self.implicit = "cg"              # how `solver_for` solves (`NavierStokes.SetImplicitSolve`)
        self.extents = (system.n,) * system.dim
        self.ops = ops = system.scalar_operators(kappa, dirichlet)
        self.stencil = system.scalar_stencil() if convection != "upwind" else None    # host array; uploaded on first use
        self.device_flux = None           # the `ScalarFlux` of `DoTimeStep`'s limited G, over `shared`
        self.t_ref = float(t_ref)
        self.precision = ScalarStepper.PRECISION if precision is None else float(precision)
        self.maxsteps = ScalarStepper.MAXSTEPS if maxsteps is None else int(maxsteps)
        self.w_b = None if buoyancy is None else system.buoyancy_weights(buoyancy)
        if flux_wall is None and dirichlet:
            flux_wall = next(iter(dirichlet))
        self.flux_wall = flux_wall
        self.flux = None if flux_wall is None else ops["wall_flux"](flux_wall)
        self.K, self.avg, self.diff = (hipla.SparseMatrix.from_scipy(ops[k]) for k in ("K", "avg", "diff"))
        self.q = hipla.Vector.from_numpy(ops["q"])
        self.mstar = hipla.SparseMatrix.from_scipy((sp.diags(ops["mass"]) + timestep * ops["K"]).tocsr())
        self.inv = CGSolver(self.mstar, pre=hipla.JacobiPreconditioner(self.mstar), precision=self.precision,
                            maxsteps=self.maxsteps)
        if time_scheme == "cnab2":        # the half-step operator M_p + timestep/2 K, next to mstar
            self.mhalf = hipla.SparseMatrix.from_scipy((sp.diags(ops["mass"]) + 0.5 * timestep * ops["K"]).tocsr())
            self.inv_half = CGSolver(self.mhalf, pre=hipla.JacobiPreconditioner(self.mhalf), precision=self.precision,
                                     maxsteps=self.maxsteps)
            self.G_ext, self.b = self.avg.CreateColVector(), self.avg.CreateColVector()
        self.Wb = None if self.w_b is None else hipla.DiagonalMatrix(self.w_b)
        self.tref_u = hipla.Vector.from_numpy(np.full(system.n_u, self.t_ref))
        self.w = None if self.flux is None else hipla.Vector.from_numpy(self.flux[1])
        self.avgT, self.difT, self.G, self.f_eff = (self.avg.CreateColVector() for _ in range(4))
        self.temp, self.delta = b_mat.CreateColVector(), b_mat.CreateColVector()
        self.steppers, self.shared = {}, {}
        self.by_step = {}                 # step size -> the CG inverse of M_p + theta K (`DoTimeStep(timestep=)`)
        self.last_solver = None
        self.lin = self.lin_inv = None    # the linearly implicit transport (`implicit_solver`), built on first use

    @property
    def solver(self):
        """The CG inverse of the scheme's operator: M_p + timestep K, or M_p + timestep/2 K."""
        return self.inv_half if self.time_scheme == "cnab2" else self.inv

    def solver_for(self, tau):
        """The CG inverse for a step of size `tau` (None: the object's own), at the precision of `solver`; built with
        Jacobi-CG on the host on first use and kept by step size.  With `implicit` at "fdm": the one direct solve of
        `direct_solver()`, with the sigma of the step."""
        if self.implicit == "fdm":
            size = self.timestep if tau is None else tau
            inv = self.last_solver = self.direct_solver()
            inv.sigma = 0.5 * size if self.time_scheme == "cnab2" else size
            return inv
        if tau is None:
            self.last_solver = self.solver
            return self.solver
        if tau not in self.by_step:
            theta = 0.5 * tau if self.time_scheme == "cnab2" else tau
            mat = hipla.SparseMatrix.from_scipy((sp.diags(self.ops["mass"]) + theta * self.ops["K"]).tocsr())
            self.by_step[tau] = CGSolver(mat, pre=hipla.JacobiPreconditioner(mat))
        inv = self.last_solver = self.by_step[tau]
        inv.precision, inv.maxsteps = self.solver.precision, self.solver.maxsteps
        return inv

    def linearised(self, b_scipy):
        """The `LinearisedConvection` of the scalar over avg, diff and B = `b_scipy` (built on first use, with its
        BiCGStab inverse `lin_inv`); the caller freezes u^n into it at the head of a step."""
        if self.lin is None:
            self.lin = LinearisedConvection(dict(avg=self.ops["avg"], diff=self.ops["diff"], div=b_scipy),
                                            self.ops["mass"], self.ops["K"], self.timestep)
            self.lin_inv = BiCGStabSolver(self.lin, None, precision=self.precision, maxsteps=self.maxsteps)
        return self.lin

    def implicit_solver(self, b_scipy, tau):
        """The BiCGStab inverse of M_p + sigma (K + B G(u^n; .)) for a step of size `tau` (None: the object's own), u^n
        frozen by the caller (``self.lin.freeze``): the `LinearisedConvection` over avg, diff and B, built on first use,
        preconditioned by the point-Jacobi diagonal of the whole operator or, with `implicit` at "fdm", by
        (M_p + sigma K)^-1."""
        self.linearised(b_scipy)
        inv = self.last_solver = self.lin_inv
        self.lin.sigma = self.timestep if tau is None else tau
        if self.implicit == "fdm":
            pre = self.direct_solver()
            pre.sigma = self.lin.sigma
        else:
            pre = self.lin.jacobi()
        if inv.pre is not pre:
            inv.pre, inv._fused = pre, False
        return inv

    def direct_solver(self):
        """The `ComponentFastDiagonalization` of K over the cells ("fdm_T" of `shared`, which the scalar steppers read),
        built on first use; ``ValueError`` with the reason when K does not factor."""
        if self.shared.get("fdm_T") is None:
            cells = np.arange(int(np.prod(self.extents))).reshape(self.extents)
            made = ComponentFastDiagonalization.try_create(sp.csr_matrix(self.ops["K"]), [cells], self.ops["mass"],
                                                           self.timestep)
            if made is None:
                raise ValueError("SetImplicitSolve: the scalar: " + ComponentFastDiagonalization.last_declined)
            self.shared["fdm_T"] = made
        return self.shared["fdm_T"]

    def wall_flux(self, temperature):
        """The heat entering through `flux_wall`: c0 - <w, T>."""
        return self.flux[0] - float(hipla.InnerProduct(self.w, temperature))


class NavierStokes:
    def __init__(self, mesh, nu, inflow, outflow, wall, uin, timestep, order=2, volumeforce=None, time_scheme="euler",
                 convection="upwind"):
        """`convection`: the scheme of the explicit convection term in `DoTimeStep` and `Advance` -- "upwind" (donor
        cell, first order: numerical viscosity about |u| h / 2) or the second-order limited "minmod" / "vanleer"
        (`staggered_grid.limited_flux`; first order remains at the one flux point per grid line and direction next to
        each wall).  Explicit Euler with the limiters wants timestep * sum_faces |u_f| / h <= 1/2 per cell.

        `time_scheme`: "euler" (the reference's step: explicit Euler convection and buoyancy, backward Euler viscosity,
        a non-incremental projection -- first order in time) or "cnab2" (second order: Adams-Bashforth 2 extrapolation
        of the convective flux and the buoyancy, Crank-Nicolson viscosity and diffusion, an incremental projection whose
        accumulated pressure lives in `gfup`, in the sign convention `SolveInitial` leaves there).  `DoTimeStep`,
        `Advance` and `AddScalar` follow it; `Advance(pseudo=True)` and `SolveInitial(timesteps=)` are a relaxation and
        ignore it.  "cnab2" keeps a two-step history (`F_prev`, `G_prev`, `b_prev`, `ResetTimeHistory`) and tolerates a
        smaller convective CFL number than "euler" (README).  Pass `time_scheme` and `convection` by keyword: the
        one stands in front of the other only because `convection` is pinned as the last parameter.  The inner solvers
        keep their defaults: the 1e-4 of the velocity solve puts a floor under the accuracy of a step, and second order
        shows only with `precision` (of `Advance`, of `AddScalar`) at or below the accuracy wanted."""
        self.convection = check_convection(convection, "NavierStokes")
        self.time_scheme = check_time_scheme(time_scheme, "NavierStokes")
        self._history = TimeHistory() if time_scheme == "cnab2" else None
        self._clock = self._history or TimeHistory()      # holds `tau_prev`, the size of the last step, for both schemes
        self._by_step = {}                # step size -> the CG inverse of M_u + theta A (`DoTimeStep(timestep=)`)
        self._last_momentum_solver = None
        self._cfl_rate = None
        self.last_stages = None
        self._stepping_cnab2 = None       # the operators "cnab2" adds to `_time_stepping_operators`, built on first use
        self.mesh, self.nu, self.timestep, self.order = mesh, nu, timestep, order
        self.inflow, self.outflow, self.wall, self.uin = inflow, outflow, wall, uin
        self.V, self.Q = bdm_hybrid(order, 10)[0](mesh, velocity_dirichlet=inflow + "|" + wall)
        self.a, self.b, self.mp, self.f, self.g, self.system = assemble(self.V, self.Q, nu=nu)
        self.gfu = hipla.Vector(self.V.ndof)          # velocity dofs (zero start, inflow data not modelled)
        self.gfup = hipla.Vector(self.Q.ndof)
        self.stokes_bpcg_iterations = None
        self.stokes_bpcg_time = None
        self._conv_operator = None        # explicit convection term of the IMEX step (:106-113), built on first use
        self._stepping = None
        self._scalar = None               # the transported scalar (`AddScalar`)
        self._projection = "cg"           # how `invproj` solves (`SetProjection`)
        self._fdm = None                  # the `FastDiagonalization` of Lp, built by the first SetProjection("fdm")
        self._implicit = "cg"             # how the velocity and the scalar solve (`SetImplicitSolve`)
        self._fdm_u = None                # the `ComponentFastDiagonalization` of A, built by the first SetImplicitSolve("fdm")
        self._convection_treatment = "explicit"   # or "implicit" (`SetConvectionTreatment`)
        self._lin_conv = None             # the `LinearisedConvection` of the velocity and its BiCGStab inverse
        self._conv_replaced = False       # the user set `conv_operator`

    @property
    def projection(self):
        """"cg" or "fdm": see `SetProjection`."""
        return self._projection

    def SetProjection(self, kind):
        """How the pressure projection phi = (B M_u^-1 B^T)^-1 B vel is solved, from now on and in every entry point
        (`Project`, `DoTimeStep`, `Advance`, the pseudo time stepping): "cg" (the default: the reference's Jacobi-CG to
        1e-8, or what `Advance(inner_pre=)` asks for) or "fdm", the direct solve of the fast diagonalisation method --
        `hipla.FastDiagonalization` of Lp over the extents (n,) * dim, built here on first use; ``ValueError`` with the
        reason when Lp is not a Kronecker sum over these extents.  With "fdm" the projection reports 0 iterations and
        ignores its entries of `precision` and `maxsteps`.  For the enclosed cavity the potential has mean zero: `gfup`
        differs from the CG path's by a constant, the velocity does not (M_u^-1 B^T annihilates constants).
        `SetProjection("cg")` puts the CG solver itself back."""
        if kind not in ("cg", "fdm"):
            raise ValueError("SetProjection: the projection is \"cg\" or \"fdm\", not %r" % (kind,))
        if kind == "fdm" and self._fdm is None:
            ops, s = self._time_stepping_operators(), self.system
            made = FastDiagonalization.try_create(ops["Lp"], (s.n,) * s.dim)
            if made is None:
                raise ValueError("SetProjection: " + FastDiagonalization.last_declined)
            self._fdm = made
        self._projection = kind
        ops = self._stepping              # (built above for "fdm"; None: no solver to swap yet)
        if ops is None:
            return
        if kind == "fdm" and ops["invproj"] is not self._fdm:
            self._invproj_cg, ops["invproj"] = ops["invproj"], self._fdm
        elif kind == "cg" and ops["invproj"] is self._fdm:
            ops["invproj"] = self._invproj_cg

    @property
    def implicit_solve(self):
        """"cg" or "fdm": see `SetImplicitSolve`."""
        return self._implicit

    def SetImplicitSolve(self, kind):
        """How the implicit solves of a step -- raw = (M_u + sigma A)^-1 temp of the velocity and, with a scalar,
        delta = (M_p + sigma K)^-1 temp_T -- are done, from now on and in every entry point (`DoTimeStep`,
        `DoTimeStep(timestep=)`, `Advance` in all its modes, the pseudo time stepping): "cg" (the default: Jacobi-CG to
        1e-4, or what `Advance(inner_pre=, precision=)` and `AddScalar(precision=)` ask for) or "fdm", the direct solve
        by fast diagonalisation on the velocity components -- `hipla.ComponentFastDiagonalization` of A over
        `system.component_ids`, built here on first use, and of K over the cells when `AddScalar` has been called or is
        called later; ``ValueError`` with the reason when a system does not factor (an inflated system with order > 0
        and a permuted one do not).  The factors do not depend on sigma: the one object serves "euler" (sigma = the step
        size), "cnab2" (half of it) and every size of a variable step, so nothing is built per step size and
        `Advance(timesteps= | cfl=)` takes any `inner_pre`.  The solves report 0 iterations and ignore their `precision`
        and `maxsteps`.

        The direct solve is exact to rounding, where the default CG stops at a relative residual of 1e-4: results differ
        from the default path at that level.  That is a difference in stopping, not in the operator -- against CG solves
        at 1e-12 the two paths agree to 1e-9.  `SetImplicitSolve("cg")` puts the CG solvers back; an object that never
        calls this method, or is back at "cg", keeps the bits of the CG path in every entry point."""
        if kind not in ("cg", "fdm"):
            raise ValueError("SetImplicitSolve: the implicit solve is \"cg\" or \"fdm\", not %r" % (kind,))
        if kind == "fdm":
            if self._fdm_u is None:
                s = self.system
                m_u = np.full(s.n_u, s.h ** s.dim * self.V.dofs_per_site ** 0)
                made = ComponentFastDiagonalization.try_create(self.a.mat, s.component_ids, m_u, self.timestep)
                if made is None:
                    raise ValueError("SetImplicitSolve: " + ComponentFastDiagonalization.last_declined)
                self._fdm_u = made
            if self._scalar is not None:
                self._scalar.direct_solver()
        self._implicit = kind
        if self._scalar is not None:
            self._scalar.implicit = kind

    @property
    def convection_treatment(self):
        """"explicit" or "implicit": see `SetConvectionTreatment`."""
        return self._convection_treatment

    def _refuse_implicit_convection(self, who):
        """``ValueError`` with the reason when the object cannot step with linearly implicit convection."""
        why = None
        if self.time_scheme == "cnab2":
            why = "time_scheme=\"cnab2\" extrapolates the convective flux; the implicit treatment is first order (\"euler\")"
        elif self.convection != "upwind" or (self._scalar is not None and self._scalar.convection != "upwind"):
            why = "the limited schemes are not linear in the transported quantity; convection=\"upwind\" only"
        elif self.system.block_size > 1:
            why = "block_size > 1: an inflated system is not supported"
        elif self._conv_replaced:
            why = "conv_operator was replaced by the user; the linearisation is that of the package's donor-cell operator"
        if why is not None:
            raise ValueError("%s: implicit convection: %s" % (who, why))

    def SetConvectionTreatment(self, kind):
        """How convection (and the transport of the scalar) enters a step, from now on and in `DoTimeStep`,
        `DoTimeStep(timestep=)` and `Advance` in all its modes: "explicit" (the default: the reference's step) or
        "implicit", the linearly implicit (Picard-linearised) step

            (M_u + tau A + tau N(a)) raw = conv(u^n) + f - A u^n,    a = I_adv u^n frozen for the step,
            N(a) v = D F(a; v),   F(a; v)_i = a_i (Avg v)_i - |a_i| (Diff v)_i / 2,

        the reference's step in increment form with the donor-cell flux linearised around u^n -- the right-hand side is
        unchanged, `Project` and u += tau (raw - C phi) follow as before.  With a scalar:
        (M_p + tau K + tau B G(u^n; .)) delta = q - K T^n - B G(u^n; T^n); the buoyancy stays lagged.  The solves are
        right-preconditioned BiCGStab (`hipla.BiCGStabSolver`; in `Advance` the device-resident loop) stopping at
        |r|_2 < precision |b|_2, `precision` and `maxsteps` with the meaning and defaults they have (1e-4, 500);
        `SetImplicitSolve` picks the preconditioner: "cg" -- point Jacobi of the whole operator, "fdm" -- the direct
        viscous inverse (M_u + tau A)^-1, for the scalar (M_p + tau K)^-1.  For a discretely divergence-free a the
        symmetric part of N(a) is positive semi-definite, so the step does not raise the kinetic energy for any tau: the
        convective limit on the step size is gone (accuracy still wants a moderate CFL number).

        ``ValueError`` with the reason for `time_scheme="cnab2"`, `convection != "upwind"` (the velocity's or the
        scalar's), an inflated system and a user-replaced `conv_operator`; `Advance` refuses `pseudo=True` and
        `inner_pre="amg"` with it.  A breakdown of a solve raises ``FloatingPointError`` and leaves the state of the last
        finished step.  `SetConvectionTreatment("explicit")` puts the explicit step back: an object that never calls this
        method, or is back at "explicit", keeps its bits in every entry point."""
        check_convection_treatment(kind, "SetConvectionTreatment")
        if kind == "implicit":
            self._refuse_implicit_convection("SetConvectionTreatment")
        self._convection_treatment = kind

    def _implicit_momentum_solver(self, tau):
        """The BiCGStab inverse of M_u + sigma (A + N(a)) for a step of size `tau` (None: the object's own) with
        a = I_adv gfu frozen here; the operator and the solver are built on first use."""
        if self._lin_conv is None:
            s = self.system
            m_u = np.full(s.n_u, s.h ** s.dim * self.V.dofs_per_site ** 0)
            op = LinearisedConvection(s.convection_operators(), m_u, s.A, self.timestep)
            self._lin_conv = dict(op=op, inv=BiCGStabSolver(op, None, precision=1e-4, maxsteps=500))
        op, inv = self._lin_conv["op"], self._lin_conv["inv"]
        op.freeze(self.gfu)
        op.sigma = self.timestep if tau is None else tau
        if self._implicit == "fdm":
            pre = self._fdm_u
            pre.sigma = op.sigma
        else:
            pre = op.jacobi()
        if inv.pre is not pre:
            inv.pre, inv._fused = pre, False
        self._last_momentum_solver = inv
        return inv

    @property
    def conv_operator(self):
        if self._conv_operator is None:
            self._conv_operator = ConvectionOperator(self.system, self.convection)
        return self._conv_operator

    @conv_operator.setter
    def conv_operator(self, op):
        self._conv_operator = op
        self._conv_replaced = True

    def _time_stepping_operators(self):
        """mstar = M_u + timestep*A with its CG inverse (:85-96) and the projection operators
        (:115-144): pressure operator B M_u^-1 B^T, CG inverse, velocity correction M_u^-1 B^T."""
        if self._stepping is None:
            s = self.system
            mass_u = s.h ** s.dim * self.V.dofs_per_site ** 0       # lumped velocity mass: cell volume
            m_u = np.full(s.n_u, mass_u)
            mstar = hipla.SparseMatrix.from_scipy((sp.diags(m_u) + self.timestep * s.A).tocsr())
            invmstar = CGSolver(mstar, pre=hipla.JacobiPreconditioner(mstar), precision=1e-4, maxsteps=500)
            bt_scaled = (sp.diags(1.0 / m_u) @ s.B.T).tocsr()
            lap_p = (s.B @ bt_scaled).tocsr()
            lap_p.sort_indices()
            Lp = hipla.SparseMatrix.from_scipy(lap_p)
            invproj = CGSolver(Lp, pre=hipla.JacobiPreconditioner(Lp), precision=1e-8, maxsteps=5000)
            self._stepping = dict(invmstar=invmstar, invproj=invproj, correct=hipla.SparseMatrix.from_scipy(bt_scaled),
                                  mstar=mstar, Lp=Lp)
        return self._stepping

    def _cnab2_operators(self):
        """What `time_scheme="cnab2"` adds to `_time_stepping_operators`: mhalf = M_u + timestep/2 A with its CG inverse
        (the precision and maxsteps of invmstar), D (the flux divergence) and B^T."""
        if self._stepping_cnab2 is None:
            s = self.system
            m_u = np.full(s.n_u, s.h ** s.dim * self.V.dofs_per_site ** 0)
            mhalf = hipla.SparseMatrix.from_scipy((sp.diags(m_u) + 0.5 * self.timestep * s.A).tocsr())
            invmhalf = CGSolver(mhalf, pre=hipla.JacobiPreconditioner(mhalf), precision=1e-4, maxsteps=500)
            self._stepping_cnab2 = dict(mhalf=mhalf, invmhalf=invmhalf,
                                        div=hipla.SparseMatrix.from_scipy(s.convection_operators()["div"]),
                                        Bt=hipla.SparseMatrix.from_scipy(s.B.T.tocsr()))
        return self._stepping_cnab2

    def _momentum_solver(self, pseudo=False):
        """(dict, key) of the CG inverse of the velocity solve: invmstar, or invmhalf of a "cnab2" step."""
        if self.time_scheme == "cnab2" and not pseudo:
            return self._cnab2_operators(), "invmhalf"
        return self._time_stepping_operators(), "invmstar"

    # ---- the two-step history of "cnab2" (None / False for "euler") ----
    @property
    def F_prev(self):
        return None if self._history is None else self._history.F_prev

    @property
    def G_prev(self):
        return None if self._history is None else self._history.G_prev

    @property
    def b_prev(self):
        return None if self._history is None else self._history.b_prev

    def ResetTimeHistory(self):
        """Forget the two-step history: the next step of every quantity extrapolates with (1, 0), as a first step
        does.  The accumulated pressure in `gfup` is left alone.  (For "euler" there is nothing to forget.)"""
        if self._history is not None:
            self._history.reset()
        self._clock.tau_prev = None

    def CflRate(self):
        """max_r (|B| |u|)_r / (M_p)_r of the current `gfu`: on the plain grid max_cell sum_faces |u_f| / h, so that
        `timestep * CflRate()` is the quantity of the README's stability limits.  One kernel over the rows of B on the HIP
        engine (one double read back), numpy otherwise."""
        eng = self.gfu.engine
        if fused.ENABLED and hasattr(getattr(eng, "lib", None), "nss_step_cfl_f64") and \
                isinstance(self.b.mat, hipla.SparseMatrix):
            if self._cfl_rate is None:
                self._cfl_rate = CflRate(eng, self.b.mat, self.system.mass)
            return self._cfl_rate(self.gfu.buf)
        rate = (abs(self.system.B) @ np.abs(self.gfu.numpy())) / self.system.mass
        return float(np.inf) if not np.isfinite(rate).all() else float(rate.max(initial=0.0))

    def _momentum_solver_for(self, tau, pseudo=False):
        """The CG inverse of the velocity solve for a step of size `tau` (None: the object's own operators), at the
        precision of the object's own; built with Jacobi-CG on the host on first use and kept by step size.  After
        `SetImplicitSolve("fdm")`: the one direct solve, with the sigma of the step.  `pseudo`: the solve of a pseudo
        time step, M_u + timestep A whatever the scheme."""
        if self._implicit == "fdm":
            size = self.timestep if tau is None else tau
            inv = self._last_momentum_solver = self._fdm_u
            inv.sigma = 0.5 * size if self.time_scheme == "cnab2" and not pseudo else size
            return inv
        held, name = self._momentum_solver(pseudo)
        if tau is None:
            self._last_momentum_solver = held[name]
            return held[name]
        if tau not in self._by_step:
            s = self.system
            theta = 0.5 * tau if self.time_scheme == "cnab2" else tau
            mat = hipla.SparseMatrix.from_scipy((sp.diags(np.full(s.n_u, s.h ** s.dim * self.V.dofs_per_site ** 0))
                                                 + theta * s.A).tocsr())
            self._by_step[tau] = CGSolver(mat, pre=hipla.JacobiPreconditioner(mat))
        inv = self._last_momentum_solver = self._by_step[tau]
        inv.precision, inv.maxsteps = held[name].precision, held[name].maxsteps
        return inv

    def _step_size(self, timestep):
        """`timestep` of `DoTimeStep` as the key of the operators: None for the object's own step size."""
        if timestep is None:
            return None
        tau = check_step_size(timestep, "DoTimeStep")
        return None if tau == self.timestep else tau

    @property
    def velocity(self):
        return self.gfu

    @property
    def pressure(self):
        out = self.gfup.CreateVector()
        out.data = -self.gfup                          # reference: pressure = -gfup (:163-165)
        return out

    def SolveInitial(self, timesteps=None, iterative=True, GS=True, tol=1e-10, maxsteps=100000, printrates=False,
                     aux=True, amg=False, condense=False, pre_storage="fp64", pre="mypre_a"):
        """`aux`: build the auxiliary-space term of MypreA (:208-357) -- the reference always does; False
        keeps the block smoother alone.  `amg=True` (kept from round 1) puts a smoothed-aggregation
        V-cycle on a.mat itself in the place of the auxiliary term.  `condense=True` solves as the reference's
        default does (:188, ``condense=True, store_inner=True``): blfA is the statically condensed form, MypreA
        sweeps over its Schur complement with blocks of coupling dofs only (:360-362), and BramblePasciakCG runs
        the condensed branch of harmonic_extension.  `pre_storage="fp32"` stores the matrices of MypreA (the
        Gauss-Seidel sweep, the auxiliary-space term or the V-cycle) with fp32 values; vectors, arithmetic and the
        Krylov operator stay fp64.

        `pre`: the velocity preconditioner.  "mypre_a" (the default) is the reference's MypreA as described above.
        "fdm" takes the exact inverse of a.mat by fast diagonalisation (`hipla.FastDiagonalizationInverse` over
        `system.component_ids`) in its place: no hierarchy, colouring or permutation is built, and
        the iteration works on the pressure Schur complement alone (about 20 to 30 iterations whatever the grid).
        ``ValueError`` with the reason for a system that does not factor (an inflated one, `order` > 0, or a permuted
        one), and for `condense=True`, `amg=True` or `pre_storage="fp32"`, which have no meaning for it.  `GS` and `aux`
        shape MypreA alone: with "fdm" they have no effect."""
        if pre not in ("mypre_a", "fdm"):
            raise ValueError("SolveInitial: pre is \"mypre_a\" or \"fdm\", not %r" % (pre,))
        if timesteps:                                     # pseudo time stepping to the Stokes state (:406-417)
            ops = self._time_stepping_operators()
            self.Project(self.gfu)
            for it in range(timesteps):
                print("it =", it)
                self._pseudo_time_step(ops)
            return
        if not iterative:
            raise NotImplementedError("sparse direct initial solve is not on the Krylov path")
        if condense and amg:
            raise ValueError("SolveInitial: amg=True (a V-cycle on a.mat) does not combine with condense=True")
        if pre == "fdm":
            return self._solve_initial_fdm(tol, maxsteps, printrates, amg, condense, pre_storage)
        blocks = self.system.facet_blocks()
        if condense:
            blfA = CondensedForm(self.system)
            blocks = coupling_blocks(blocks, blfA.interior)
        else:
            blfA = AssembledForm(self.a.mat)
        blfB = AssembledForm(self.b.mat)
        preM = hipla.Preconditioner(self.mp, "local")
        middle = None
        if amg:
            middle = hipla.SmoothedAggregationAMG(blfA.mat, storage=pre_storage)
        elif aux:
            self.transform, self.preAh1, middle = auxiliary_space_preconditioner(self.system, storage=pre_storage)
        preA = self.preA = MypreA(self.V, blfA, blocks, GS=GS, aux=middle, storage=pre_storage)
        sol = BlockVector([self.gfu, self.gfup])       # aliases the grid-function storage (:206)
        out = BramblePasciakCG(blfA, blfB, None, self.f.vec, self.g.vec, preA, preM, sol, initialize=False,
                               tol=tol, maxsteps=maxsteps, rel_err=True, printrates=printrates)
        if isinstance(out, tuple):
            self.stokes_bpcg_iterations, self.stokes_bpcg_time = out
        else:                                          # zero initial residual: bare vector (:191-192)
            self.stokes_bpcg_iterations, self.stokes_bpcg_time = 0, 0.0

    def _solve_initial_fdm(self, tol, maxsteps, printrates, amg, condense, pre_storage):
        """`SolveInitial(pre="fdm")`: BramblePasciakCG with the exact inverse of a.mat as preA and the Jacobi preM."""
        for given, name, why in ((condense, "condense=True", "the condensed Schur complement is no Kronecker sum"),
                                 (amg, "amg=True", "there is no term to put a V-cycle in"),
                                 (pre_storage != "fp64", "pre_storage=\"fp32\"", "the factors are stored in fp64")):
            if given:
                raise ValueError("SolveInitial(pre=\"fdm\"): %s does not combine with it (%s)" % (name, why))
        preA = hipla.FastDiagonalizationInverse.try_create(self.a.mat, self.system.component_ids)
        if preA is None:
            raise ValueError("SolveInitial(pre=\"fdm\"): " + hipla.FastDiagonalizationInverse.last_declined)
        self.preA = preA
        preM = hipla.Preconditioner(self.mp, "local")
        sol = BlockVector([self.gfu, self.gfup])
        out = BramblePasciakCG(AssembledForm(self.a.mat), AssembledForm(self.b.mat), None, self.f.vec, self.g.vec, preA,
                               preM, sol, initialize=False, tol=tol, maxsteps=maxsteps, rel_err=True,
                               printrates=printrates)
        if isinstance(out, tuple):
            self.stokes_bpcg_iterations, self.stokes_bpcg_time = out
        else:
            self.stokes_bpcg_iterations, self.stokes_bpcg_time = 0, 0.0

    def _pseudo_time_step(self, ops):
        """One pseudo time step towards the Stokes state (:408-417): no convection, two projections.  Returns the
        iterations of the two projection solves."""
        temp = self.a.mat.CreateColVector()
        temp2 = self.a.mat.CreateColVector()
        temp.data = -self.a.mat * self.gfu
        temp2.data = self._momentum_solver_for(None, pseudo=True) * temp      # invmstar, or the direct solve
        self.Project(temp2)
        count = ops["invproj"].iterations
        self.gfu.data += self.timestep * temp2
        self.Project(self.gfu)
        return count + ops["invproj"].iterations

    def AddForce(self, force):
        """`force`: host array of nodal forces on the velocity dofs, added to f (:419-422)."""
        self.f.vec.data += hipla.Vector.from_numpy(np.asarray(force, dtype=np.float64))

    def AddScalar(self, kappa, dirichlet=None, buoyancy=None, t_ref=0.0, initial=None, precision=None, maxsteps=None,
                  flux_wall=None, convection=None):
        """Carry a cell-centred scalar T (a temperature) with the flow: M_p dT/dt = q - K T - B G with diffusivity
        `kappa`, the donor-cell flux G of T through the faces (the face velocities are the velocity dofs) and implicit
        diffusion; `DoTimeStep` and `Advance` then advance T with u, coupled explicitly (first order, like the
        convection term).  Plain systems only (``ValueError`` for an inflated one).

        `dirichlet`: wall name ("x-", "x+", "y-", "y+", "z-", "z+") -> wall temperature; every other wall is insulated.
        `buoyancy` = (beta_x, beta_y[, beta_z]): the Boussinesq force, f + beta_c h^d (avg T - `t_ref`) on the faces of
        component c, takes the place of f in the momentum equation; None = a passive scalar.  `initial`: host array of
        n_p cell values (None: `t_ref` everywhere).  `precision` / `maxsteps` of the temperature solve: None = those of
        invmstar (1e-4, 500).  `flux_wall`: the Dirichlet wall whose heat flux `Advance` records (None: the first one
        given).  `convection`: the scheme of G, "upwind" | "minmod" | "vanleer" as for the constructor (None: the
        velocity's).  The scalar is `self.temperature`; `AddForce` keeps working: f is read every step.  The scalar
        follows the object's `time_scheme`; added after some steps it starts with the weights (1, 0) of a first step."""
        dirichlet = dict(dirichlet or {})
        self._scalar = ScalarField(self.system, self.b.mat, self.timestep, kappa, dirichlet, buoyancy, t_ref, precision,
                                   maxsteps, flux_wall, self.convection if convection is None else convection,
                                   self.time_scheme)
        if self._implicit == "fdm":       # (`SetImplicitSolve` came first: the scalar follows it)
            self._scalar.direct_solver()
            self._scalar.implicit = "fdm"
        if self._history is not None:
            self._history.reset("scalar")
        start = np.full(self.system.n_p, float(t_ref)) if initial is None else np.asarray(initial, dtype=np.float64)
        if start.shape != (self.system.n_p,):
            raise ValueError("AddScalar: initial holds %s values, the grid has %d cells" % (start.shape, self.system.n_p))
        self.temperature = hipla.Vector.from_numpy(start)

    def _scalar_flux(self):
        """The first statements of a step with a scalar, on (u^n, T^n): G = u * (avg T) - |u| * (diff T) / 2 and the
        force of the step, f + w_b * (avg T - t_ref) (f itself for a passive scalar)."""
        sc = self._scalar
        sc.avgT.data = sc.avg * self.temperature
        if sc.convection == "upwind":
            sc.difT.data = sc.diff * self.temperature
            sc.G.engine.upwind_flux(self.gfu.buf, sc.avgT.buf, sc.difT.buf, sc.G.buf)
        else:
            self._limited_scalar_flux(sc)
        if sc.Wb is None:
            return self.f.vec
        sc.avgT.data -= sc.tref_u
        sc.f_eff.data = self.f.vec + sc.Wb * sc.avgT
        return sc.f_eff

    def _limited_scalar_flux(self, sc):
        """G by the scalar's limited scheme: one passive launch of a `ScalarFlux` over `sc.shared` (the device stencil of
        the scalar steppers), or -- an engine without the kernel -- `limited_flux` on the host, uploaded."""
        eng = sc.G.engine
        if not ScalarFlux.available(eng, sc.convection):
            from staggered_grid import limited_flux
            sc.G.data = hipla.Vector.from_numpy(limited_flux(sc.stencil, self.gfu.numpy(), self.temperature.numpy(),
                                                             sc.convection))
            return
        if sc.device_flux is None:
            sc.device_flux = ScalarFlux(eng, sc.ops, sc.convection, sc.stencil, sc.shared)
        sc.device_flux.launch(self.gfu.buf, None, self.temperature.buf, 0.0, sc.G.buf)

    def _scalar_step(self, tau=None):
        """The last statements of a step with a scalar: temp_T = q - K T - B G;  delta = (M_p + timestep K)^-1 temp_T;
        T += timestep * delta."""
        sc = self._scalar
        sc.temp.data = sc.q - sc.K * self.temperature
        sc.temp.data -= self.b.mat * sc.G
        if self._convection_treatment == "implicit":
            sc.delta.data = sc.implicit_solver(self.system.B, tau) * sc.temp
        else:
            sc.delta.data = sc.solver_for(tau) * sc.temp
        self.temperature.data += (self.timestep if tau is None else tau) * sc.delta

    def DoTimeStep(self, timestep=None):
        """One IMEX step (:424-438): temp = conv(u) + f - A u;  temp2 = invmstar temp;
        Project(temp2);  u += timestep * temp2.  With a scalar (`AddScalar`) its flux and force statements come first
        and its own step last.

        `timestep`: the size of this step (None: the object's).  Another size than the object's solves with
        `M_u + theta A` (and the scalar's operator) for that size, built with Jacobi-CG at the precisions of the object's
        own solvers on first use and kept by step size; "cnab2" extrapolates with the variable-step weights
        (1 + r/2, -r/2), r = timestep / the size of the last step."""
        tau = self._step_size(timestep)
        if self.time_scheme == "cnab2":
            return self._do_time_step_cnab2(tau)
        ops = self._time_stepping_operators()
        force = self.f.vec if self._scalar is None else self._scalar_flux()
        temp = self.a.mat.CreateColVector()
        temp2 = self.a.mat.CreateColVector()
        temp.data = self.conv_operator * self.gfu        # :429
        temp.data += force
        temp.data += -self.a.mat * self.gfu
        if self._convection_treatment == "implicit":
            return self._finish_implicit_step(temp, temp2, tau)
        temp2.data = self._momentum_solver_for(tau) * temp
        self.Project(temp2)
        self.gfu.data += (self.timestep if tau is None else tau) * temp2
        if self._scalar is not None:
            self._scalar_step(tau)
        self._clock.tau_prev = self.timestep if tau is None else tau

    def _finish_implicit_step(self, temp, temp2, tau):
        """The statements of `DoTimeStep` behind the right-hand side `temp` with linearly implicit convection: the
        BiCGStab solve with M_u + tau (A + N(I_adv u^n)), the projection, the update, and the scalar's step with u^n
        frozen before the update.  A breakdown leaves `gfu`, `gfup` and the temperature as they were."""
        self._refuse_implicit_convection("DoTimeStep")
        size = self.timestep if tau is None else tau
        if self._scalar is not None:
            self._scalar.linearised(self.system.B).freeze(self.gfu)   # u^n, before the update
        temp2.data = self._implicit_momentum_solver(tau) * temp       # (raises before anything is touched)
        u_back, p_back = self.gfu.CreateVector(), self.gfup.CreateVector()
        u_back.data = self.gfu
        p_back.data = self.gfup
        self.Project(temp2)
        self.gfu.data += size * temp2
        if self._scalar is not None:
            try:
                self._scalar_step(tau)
            except FloatingPointError:
                self.gfu.data = u_back
                self.gfup.data = p_back
                raise
        self._clock.tau_prev = size

    def _extrapolate(self, now, prev, weights, out):
        """out = w_new now + w_old prev;  prev = now  (w_old == 0: `prev` is not read)."""
        w_new, w_old = weights
        if w_old:
            out.data = w_new * now + w_old * prev
        else:
            out.data = w_new * now
        prev.data = now

    def _do_time_step_cnab2(self, tau=None):
        """One step of `time_scheme="cnab2"`, with (w_new, w_old) = (1, 0) on a quantity's first step and (3/2, -1/2)
        afterwards and q = `gfup`, the accumulated pressure:

            F = flux(u^n);  F_ext = w_new F + w_old F_prev;  F_prev = F
            temp = f_step - A u^n - D F_ext - B^T q;   raw = (M_u + timestep/2 A)^-1 temp
            phi = (B M_u^-1 B^T)^-1 B raw;   u^{n+1} = u^n + timestep (raw - M_u^-1 B^T phi);   q += phi

        With a scalar, before: G_ext and b = w_b (avg T^n - t_ref) extrapolated the same way, f_step = f + b_ext; after:
        delta = (M_p + timestep/2 K)^-1 (q_T - K T^n - B G_ext);  T^{n+1} = T^n + timestep delta.  `Project` is not
        called: it overwrites `gfup`.  `tau`: the size of this step (None: `timestep`, the object's); behind a step of
        another size the weights are (1 + r/2, -r/2), r = this size / that one, and `tau` stands for `timestep` above."""
        size = self.timestep if tau is None else tau
        conv = self.conv_operator
        if not hasattr(conv, "Flux"):
            raise ValueError("DoTimeStep: time_scheme=\"cnab2\" keeps its history in flux form and wants a conv_operator "
                             "with Flux(u, F)")
        ops, half, hist, eng = self._time_stepping_operators(), self._cnab2_operators(), self._history, self.gfu.engine
        force = self.f.vec if self._scalar is None else self._scalar_flux_cnab2(size)
        F, F_ext = half["div"].CreateRowVector(), half["div"].CreateRowVector()
        conv.Flux(self.gfu, F)
        self._extrapolate(F, hist.vector("F_prev", len(F), eng), hist.weights("momentum", size), F_ext)
        hist.valid["momentum"] = True
        temp, raw, temp2 = (self.a.mat.CreateColVector() for _ in range(3))
        rhs, phi = self.b.mat.CreateColVector(), self.gfup.CreateVector()
        temp.data = force - self.a.mat * self.gfu
        temp.data -= half["div"] * F_ext
        temp.data -= half["Bt"] * self.gfup
        raw.data = self._momentum_solver_for(tau) * temp
        rhs.data = self.b.mat * raw
        phi.data = ops["invproj"] * rhs
        temp2.data = raw - ops["correct"] * phi
        self.gfup.data += phi
        self.gfu.data += size * temp2
        self.last_stages = dict(F_ext=F_ext, temp=temp, raw=raw, phi=phi, temp2=temp2)      # of the last step, for checks
        if self._scalar is not None:
            sc = self._scalar
            sc.temp.data = sc.q - sc.K * self.temperature
            sc.temp.data -= self.b.mat * sc.G_ext
            sc.delta.data = sc.solver_for(tau) * sc.temp
            self.temperature.data += size * sc.delta
        hist.tau_prev = size

    def _scalar_flux_cnab2(self, size=None):
        """The scalar's first statements of a "cnab2" step on (u^n, T^n): G into G_ext / G_prev, and the force of the
        step, f + w_new b + w_old b_prev with b = w_b (avg T - t_ref) (f itself for a passive scalar)."""
        sc, hist, eng = self._scalar, self._history, self.gfu.engine
        weights = hist.weights("scalar", size)
        sc.avgT.data = sc.avg * self.temperature
        if sc.convection == "upwind":
            sc.difT.data = sc.diff * self.temperature
            sc.G.engine.upwind_flux(self.gfu.buf, sc.avgT.buf, sc.difT.buf, sc.G.buf)
        else:
            self._limited_scalar_flux(sc)
        self._extrapolate(sc.G, hist.vector("G_prev", len(sc.G), eng), weights, sc.G_ext)
        force = self.f.vec
        if sc.Wb is not None:
            sc.avgT.data -= sc.tref_u
            sc.b.data = sc.Wb * sc.avgT
            self._extrapolate(sc.b, hist.vector("b_prev", len(sc.b), eng), weights, sc.f_eff)
            sc.f_eff.data += self.f.vec
            force = sc.f_eff
        hist.valid["scalar"] = True
        return force

    def Project(self, vel):
        """Make `vel` discretely divergence-free (:440-443): phi = (B M_u^-1 B^T)^-1 B vel;
        pressure <- phi;  vel -= M_u^-1 B^T phi."""
        ops = self._time_stepping_operators()
        rhs = self.b.mat.CreateColVector()
        rhs.data = self.b.mat * vel
        self.gfup.data = ops["invproj"] * rhs
        vel.data -= ops["correct"] * self.gfup

    def Advance(self, nsteps, inner_pre="jacobi", precision=None, diagnostics=True, pseudo=False, maxsteps=None, *,
                timesteps=None, cfl=None, max_timestep=None, growth=1.25, duration=None):
        """`nsteps` IMEX steps (`pseudo=True`: the pseudo time stepping of ``SolveInitial(timesteps=nsteps)``) through
        the device-resident stepper (`hipla.stepping.TimeStepper`): the statements of `DoTimeStep` / `Project` in two
        launches for the right-hand side and one for the projection tail, every buffer allocated once, a per-step
        record on the device read back once.  Returns an `hipla.stepping.StepRecord` (mstar_iterations,
        proj_iterations, div_norm, kinetic_energy; with a scalar -- `AddScalar` -- also scalar_iterations and
        wall_flux, and `pseudo=True` raises ``ValueError``).

        `inner_pre`: "jacobi" (what `DoTimeStep` uses) or "amg" -- a smoothed-aggregation V-cycle for both inner CG
        solves; `precision` / `maxsteps`: None = those of `DoTimeStep` (1e-4 / 1e-8, 500 / 5000), one value for both
        solves, or a pair; `diagnostics=False` skips |B u| and the kinetic energy.  When the stepper declines (no HIP
        engine, ``hipla.fused.ENABLED`` off) the statements themselves run -- with Jacobi-CG, whatever `inner_pre` --
        and the reason is in ``record.declined`` (and ``self.advance_declined``).

        The steppers (one per `inner_pre`) share `M_u + timestep A`, `B M_u^-1 B^T` and `M_u^-1 B^T` with `DoTimeStep`
        and the convection matrices with each other; what a stepper adds in HBM is its work vectors, the rows of
        `[A | D]` -- a second copy of A, 12 bytes per non-zero -- and, for "amg", the two hierarchies.  Like
        `DoTimeStep`, they keep the `timestep` of their first use: these operators are built once per object.

        `time_scheme="cnab2"`: the stepper runs the statements of `_do_time_step_cnab2`; it shares `M_u + timestep/2 A`
        with `DoTimeStep`, keeps `[A | D | B^T]` in the place of `[A | D]` and reads and writes
        the object's history and `gfup`, so that `DoTimeStep` and `Advance` can be mixed freely.  It declines when the flux
        kernel declines the convection operators.  `pseudo=True` runs the "euler" stepper's relaxation, as ever.

        Variable steps: `timesteps` = `nsteps` prescribed sizes, or `cfl` = the target for
        tau_n * `CflRate()` of u^n, with tau_n = min(`max_timestep` (None: the constructor's `timestep`), cfl / rate,
        `growth` (1.25) times the last step) chosen by `hipla.stepping.choose_timestep`; `duration` ends the call when the
        time reaches it -- the last step is shortened to land on it, `nsteps` stays the cap.  The record then has
        `timestep`, `time`, `cfl` and (with `cfl=`) `limited_by`.  These steps run through steppers of their own, which
        solve with `M_u + sigma A` read from A itself (the shifted CG loop), Jacobi only: ``ValueError`` with
        `inner_pre="amg"` (a hierarchy belongs to one step size) or `pseudo=True`.  "cnab2" extrapolates with the weights
        (1 + r/2, -r/2), r = tau_n / tau_{n-1}.  A rate that is not finite leaves the state of the last finished step in
        `gfu` and raises ``FloatingPointError``.  Fixed and variable calls and `DoTimeStep` mix freely.

        After `SetProjection("fdm")` the steppers (their own, keyed by the projection too) launch the direct solve of the
        object's `FastDiagonalization` in the place of the projection's CG: ``record.projection == "fdm"``,
        `proj_iterations` all zero, the projection entries of `precision` and `maxsteps` ignored, and for
        `inner_pre="amg"` no hierarchy of the pressure operator.

        After `SetImplicitSolve("fdm")` the steppers (keyed by that switch as well) launch the direct solves of the
        object's `ComponentFastDiagonalization` in the place of the velocity's and the scalar's CG:
        ``record.implicit == "fdm"``, `mstar_iterations` and `scalar_iterations` all zero, no mstar, CG loop,
        preconditioner or velocity hierarchy in the stepper, and variable steps with any `inner_pre`, which then concerns
        a "cg" projection alone.  With both switches at "fdm" a fixed-step call does not wait for the host between its
        first launch and its read-back.

        After `SetConvectionTreatment("implicit")` the steppers (keyed by that switch too) solve the velocity, and the
        scalar, with the device-resident BiCGStab loop on the linearised operator read from `[A | D]` (`[K | B]`), a =
        I_adv u^n formed once per step; the polls of the loop are the only new host synchronisation.
        ``record.convection_treatment == "implicit"``, `mstar_iterations` and `scalar_iterations` count BiCGStab
        iterations, the velocity entries of `precision` and `maxsteps` are the loop's.  ``ValueError`` for `pseudo=True`
        and `inner_pre="amg"`; a breakdown of a solve leaves the state of the last finished step and raises
        ``FloatingPointError``."""
        if inner_pre not in ("jacobi", "amg"):
            raise ValueError("Advance: inner_pre is \"jacobi\" or \"amg\"")
        if pseudo and self._scalar is not None:
            raise ValueError("Advance: the pseudo time stepping carries no scalar")
        treatment = self._convection_treatment
        if treatment == "implicit":
            self._refuse_implicit_convection("Advance")
            if pseudo:
                raise ValueError("Advance: implicit convection: the pseudo time stepping has no convection term")
            if inner_pre == "amg":
                raise ValueError("Advance: implicit convection: inner_pre=\"amg\" is a hierarchy of the symmetric "
                                 "operator of one step size; the BiCGStab solves take point Jacobi or the direct inverse")
        nsteps = int(nsteps)
        variable = timesteps is not None or cfl is not None
        controller = None
        if timesteps is not None and cfl is not None:
            raise ValueError("Advance: timesteps and cfl exclude each other")
        if cfl is None and not (duration is None and growth == 1.25 and max_timestep is None):
            raise ValueError("Advance: duration, growth and max_timestep belong to cfl=")
        if variable and ((inner_pre == "amg" and self._implicit != "fdm") or pseudo):
            raise ValueError("Advance: variable steps take inner_pre=\"jacobi\" (a hierarchy belongs to one step size) "
                             "and no pseudo time stepping")
        if timesteps is not None:
            timesteps = [check_step_size(t, "Advance") for t in timesteps]
            if len(timesteps) != nsteps:
                raise ValueError("Advance: timesteps holds %d sizes for %d steps" % (len(timesteps), nsteps))
        if cfl is not None:
            controller = StepController(cfl, self.timestep if max_timestep is None else max_timestep,
                                        growth, duration)
        steppers = self.__dict__.setdefault("_steppers", {})
        scheme = "euler" if pseudo else self.time_scheme
        key = inner_pre if scheme == self.time_scheme else (inner_pre, scheme)
        key = ("variable", key) if variable else key
        key = (key, "fdm") if self._projection == "fdm" else key
        key = (key, "implicit fdm") if self._implicit == "fdm" else key
        key = (key, "implicit convection") if treatment == "implicit" else key
        stepper = steppers.get(key) if fused.ENABLED else None
        if stepper is None:
            s = self.system
            m_u = np.full(s.n_u, s.h ** s.dim * self.V.dofs_per_site ** 0)
            if "_stepper_shared" not in self.__dict__:      # one copy of the operators for DoTimeStep and every stepper
                ops = self._time_stepping_operators()
                self._stepper_shared = dict(mstar=ops["mstar"], Lp=ops["Lp"], C=ops["correct"])
                if self.time_scheme == "cnab2":
                    self._stepper_shared["mhalf"] = self._cnab2_operators()["mhalf"]
            if self._projection == "fdm":
                self._stepper_shared.setdefault("fdm", self._fdm)
            if self._implicit == "fdm":
                self._stepper_shared.setdefault("fdm_u", self._fdm_u)
            stepper = TimeStepper.try_create(s, self.a.mat, self.b.mat, self.f.vec, self.timestep, m_u, inner_pre,
                                             conv_operator=lambda: self.conv_operator, shared=self._stepper_shared,
                                             convection=self.convection, time_scheme=scheme, variable=variable,
                                             m_p=self.system.mass, projection=self._projection,
                                             implicit=self._implicit, convection_treatment=treatment)
            if stepper is not None:
                steppers[key] = stepper
        self.advance_declined = TimeStepper.last_declined if stepper is None else None
        if stepper is not None and self._scalar is not None:
            sc = self._scalar
            skey = "variable" if variable else inner_pre
            skey = (skey, "implicit fdm") if self._implicit == "fdm" else skey
            skey = (skey, "implicit convection") if treatment == "implicit" else skey
            if skey not in sc.steppers:
                sc.steppers[skey] = ScalarStepper(self.gfu.engine, sc.ops, self.b.mat, self.f.vec, self.timestep,
                                                  inner_pre, sc.w_b, sc.t_ref, sc.flux, sc.precision, sc.maxsteps,
                                                  shared=sc.shared, convection=sc.convection, stencil=sc.stencil,
                                                  time_scheme=self.time_scheme, variable=variable,
                                                  implicit=self._implicit, extents=sc.extents,
                                                  convection_treatment=treatment)
            return stepper.advance(self.gfu, self.gfup, nsteps, precision, maxsteps, diagnostics,
                                   scalar=sc.steppers[skey], temperature=self.temperature, history=self._history,
                                   timesteps=timesteps, controller=controller, clock=self._clock)
        if stepper is not None:
            return stepper.advance(self.gfu, self.gfup, nsteps, precision, maxsteps, diagnostics, pseudo,
                                   history=None if pseudo else self._history, timesteps=timesteps, controller=controller,
                                   clock=None if pseudo else self._clock)
        return self._advance_by_statements(nsteps, precision, maxsteps, diagnostics, pseudo, StepRecord, timesteps,
                                           controller)

    def _advance_by_statements(self, nsteps, precision, maxsteps, diagnostics, pseudo, record_type, timesteps=None,
                               controller=None):
        """`Advance` through `DoTimeStep` / `Project` themselves; the inner solvers take `precision` / `maxsteps` for
        the duration of the call.  With `timesteps` or a `controller`: the same sizes, or the same controller on
        `CflRate()`, through `DoTimeStep(timestep=tau_n)`."""
        import contextlib
        import io
        ops = self._time_stepping_operators()
        if self._convection_treatment == "implicit":
            self._implicit_momentum_solver(None)
            solvers = (self._lin_conv["inv"], ops["invproj"])
        elif self._implicit == "fdm":     # (the direct solve takes precision and maxsteps, and ignores them)
            solvers = (self._fdm_u, ops["invproj"])
        else:
            held, name = self._momentum_solver(pseudo)
            solvers = (held[name], ops["invproj"])
        saved = [(sv.precision, sv.maxsteps) for sv in solvers]
        for sv, p, m in zip(solvers, pair(precision), pair(maxsteps)):
            sv.precision = sv.precision if p is None else float(p)
            sv.maxsteps = sv.maxsteps if m is None else int(m)
        its_m, its_p, div, energy = [], [], [], []
        variable = timesteps is not None or controller is not None
        taus, rates, codes = [], [], None if controller is None else []
        sc = self._scalar
        its_s, wall = ([], []) if sc is not None else (None, None)
        mass_u = self.system.h ** self.system.dim
        try:
            with contextlib.redirect_stdout(io.StringIO()):
                if pseudo:
                    self.Project(self.gfu)
                for step in range(nsteps):
                    if pseudo:
                        count = self._pseudo_time_step(ops)
                    elif variable:
                        rate = self.CflRate()
                        chosen = (timesteps[step], None) if controller is None else \
                            controller.next(rate, self._clock.tau_prev)
                        if chosen is None:
                            break
                        taus.append(chosen[0])
                        rates.append(rate)
                        if controller is not None:
                            codes.append(chosen[1])
                        self.DoTimeStep(timestep=chosen[0])
                        count = ops["invproj"].iterations
                    else:
                        self.DoTimeStep()
                        count = ops["invproj"].iterations
                    its_m.append(solvers[0].iterations if pseudo else self._last_momentum_solver.iterations)
                    its_p.append(count)
                    if sc is not None:
                        its_s.append(sc.last_solver.iterations)
                        if diagnostics and sc.flux is not None:
                            wall.append(sc.wall_flux(self.temperature))
                    if diagnostics:
                        bu = self.b.mat.CreateColVector()
                        bu.data = self.b.mat * self.gfu
                        div.append(float(hipla.Norm(bu)))
                        energy.append(0.5 * mass_u * float(hipla.InnerProduct(self.gfu, self.gfu)))
        finally:
            for sv, (p, m) in zip(solvers, saved):
                sv.precision, sv.maxsteps = p, m
        return record_type(its_m, its_p, np.array(div) if diagnostics else None,
                           np.array(energy) if diagnostics else None, declined=self.advance_declined,
                           scalar_iterations=its_s, convection=self.convection,
                           time_scheme="euler" if pseudo else self.time_scheme, projection=self._projection,
                           implicit=self._implicit, convection_treatment=self._convection_treatment,
                           **(variable_record(taus, rates, codes) if variable else {}),
                           wall_flux=np.array(wall) if sc is not None and diagnostics and sc.flux is not None else None)
