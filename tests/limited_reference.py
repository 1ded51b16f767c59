"""numpy / scipy restatement of ONE coupled step of velocity and scalar with the second-order limited fluxes
(`NavierStokes(convection=)`, `AddScalar(convection=)`) and exact inner solves -- the twin of tests/scalar_reference.py,
a helper of the limited-convection tests, not a test.  It shares with the product the matrices and stencils of
`StokesSystem` and the vectorised `limited_flux`, both checked on their own against direct loops:

    G      = limited_flux(scalar stencil, u, T)                  ("upwind": u * (avg T) - |u| * (diff T) / 2)
    f_eff  = f + w_b * (avg T - t_ref)                           (f without buoyancy)
    temp   = conv(u) + f_eff - A u,  conv = -D limited_flux(convection stencil, I_adv u, u)   ("upwind": donor cell)
    raw    = (M_u + tau A)^-1 temp;  phi = (B M_u^-1 B^T)^+ B raw;  temp2 = raw - M_u^-1 B^T phi;  u += tau temp2
    temp_T = q - K T - B G;           delta = (M_p + tau K)^-1 temp_T;  T += tau delta
    wall_flux = c0 - <w, T>           of the new T"""

import numpy as np
import scipy.sparse as sp
from scipy.sparse.linalg import spsolve

from scalar_reference import pinned_solve


def limited_coupled_step(system, tau, u, T, f, kappa, dirichlet, buoyancy=None, t_ref=0.0, flux_wall=None,
                         convection="vanleer", scalar_convection=None):
    from staggered_grid import limited_flux
    s = system
    scalar_convection = convection if scalar_convection is None else scalar_convection
    ops = s.scalar_operators(kappa, dirichlet)
    mass_u = s.h ** s.dim
    avg_t = ops["avg"] @ T
    if scalar_convection == "upwind":
        G = u * avg_t - 0.5 * np.abs(u) * (ops["diff"] @ T)
    else:
        G = limited_flux(s.scalar_stencil(), u, T, scalar_convection)
    f_eff = f.copy() if buoyancy is None else f + s.buoyancy_weights(buoyancy) * (avg_t - t_ref)
    cops = s.convection_operators()
    adv = cops["adv"] @ u
    if convection == "upwind":
        flux = adv * (cops["avg"] @ u) - 0.5 * np.abs(adv) * (cops["diff"] @ u)
    else:
        flux = limited_flux(s.convection_stencil(), adv, u, convection)
    temp = -(cops["div"] @ flux) + f_eff - s.A @ u
    raw = spsolve(sp.csc_matrix(mass_u * sp.identity(s.n_u) + tau * s.A), temp)
    correct = (s.B.T / mass_u).tocsr()
    phi = pinned_solve((s.B @ correct).tocsr(), s.B @ raw)
    temp2 = raw - correct @ phi
    u_new = u + tau * temp2
    temp_t = ops["q"] - ops["K"] @ T - s.B @ G
    delta = spsolve(sp.csc_matrix(sp.diags(ops["mass"]) + tau * ops["K"]), temp_t)
    T_new = T + tau * delta
    out = dict(G=G, f_eff=f_eff, temp=temp, raw=raw, temp2=temp2, u=u_new, temp_T=temp_t, delta=delta, T=T_new)
    wall = flux_wall if flux_wall is not None else next(iter(dirichlet), None)
    if wall is not None:
        c0, w = ops["wall_flux"](wall)
        out["wall_flux"] = c0 - w @ T_new
    return out
