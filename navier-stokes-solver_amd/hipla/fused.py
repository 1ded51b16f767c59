"""Host side of the fused, device-resident Krylov loops (C ABI: ``nss_bpcg2_*`` ...).

``*.try_create`` return a loop object when every operand is native to the HIP engine
(CSR ``SparseMatrix`` blocks, Jacobi / block-Jacobi preconditioners, plain vectors) and
``None`` otherwise (the reason in ``last_declined``) -- the caller then drives the same algorithm through the operator
protocol (still on the GPU, one kernel per statement), which is what keeps user
``BaseMatrix`` subclasses working.

The loops enqueue ``poll_every`` iterations at a time without any host synchronisation;
alpha / beta / the stop test live on the device and a ``done`` flag freezes the state at
exactly the iteration where the reference would ``break``."""

import ctypes as C
import os
from typing import NamedTuple

import numpy as np

from .amg import SmoothedAggregationAMG
from .matrix import (BlockGaussSeidel, BlockJacobi, BlockMatrix, DiagonalMatrix, ScaledMatrix, SparseMatrix,
                     SumMatrix)
from .vector import BlockVector, Vector

POLL_EVERY = int(os.environ.get("NSS_POLL_EVERY", "32"))
ENABLED = True      # tests flip this to force the protocol path on native operands


class Bpcg2State(C.Structure):
    """ctypes mirror of ``nss_bpcg2_t`` (include/nss_krylov.h)."""
    _fields_ = ([(n, C.c_void_p) for n in ("A", "B", "BT", "pre_diag", "pre_bjac", "pre_amg", "minv")]
                + [(n, C.c_void_p) for n in ("u0", "u1", "d0", "d1", "w0", "w1", "s0", "s1", "z0", "q",
                                             "t0", "t1", "t2", "t3", "t4")]
                + [("scal", C.c_void_p), ("ctrl", C.c_void_p), ("hist", C.c_void_p),
                   ("partials_a", C.c_void_p), ("partials_b", C.c_void_p), ("partials_c", C.c_void_p),
                   ("k", C.c_double), ("n_u", C.c_int32), ("n_p", C.c_int32)]
                + [(n, C.c_void_p) for n in ("cond_HT", "cond_H", "cond_inner", "cond_f")]
                + [("ghost_mode", C.c_int32), ("ghost_n", C.c_int32), ("ghost_map", C.c_void_p),
                   ("ghost_s0", C.c_void_p), ("ghost_w0", C.c_void_p),
                   ("ghost_p_mode", C.c_int32), ("ghost_p_n", C.c_int32), ("ghost_b", C.c_void_p),
                   ("ghost_t3", C.c_void_p), ("ghost_w1", C.c_void_p), ("ghost_minv", C.c_void_p),
                   ("local_sums", C.c_int32), ("pre_dist_amg", C.c_void_p), ("dist_compact", C.c_int32),
                   ("minv_uniform", C.c_int32), ("pre_dist_aux", C.c_void_p), ("p2p", C.c_void_p)]
                + [("plan_gen", C.c_int64), ("cap_a", C.c_int64), ("cap_b", C.c_int64), ("cap_c", C.c_int64)]
                + [("pre_fdm", C.c_void_p), ("sweep_A", C.c_void_p)])


class HaloStruct(C.Structure):
    """ctypes mirror of ``nss_halo_t`` (include/nss_krylov.h)."""
    _fields_ = [("send_idx", C.c_void_p), ("sendbuf", C.c_void_p), ("ext", C.c_void_p),
                ("h_send_peer", C.c_void_p), ("h_send_off", C.c_void_p), ("h_send_cnt", C.c_void_p),
                ("h_recv_peer", C.c_void_p), ("h_recv_off", C.c_void_p), ("h_recv_cnt", C.c_void_p),
                ("n_pack", C.c_int32), ("n_send", C.c_int32), ("n_recv", C.c_int32),
                ("int_begin", C.c_int32), ("int_end", C.c_int32), ("direct", C.c_int32)]


PHASE = {"K1": 1, "K2": 2, "K3": 3, "SUM1": 4, "ALPHA": 5, "K4": 6, "SUM2": 7, "BETA": 8, "K5": 9}
CPHASE = {"C1": 1, "C23": 2, "SUMA": 3, "C4": 4, "SUMW": 5}      # compact plan (NSS_BPCG2C_*)
S_WD, S_AS, S_WDN, S_ALPHA, S_BETA, S_ERR0, S_TOL, S_REL = range(8)


def _hip(engine):
    return getattr(engine, "name", "") == "hip-gfx950" and hasattr(engine.lib, "nss_bpcg2_iterate")


class PreParts(NamedTuple):
    """What the fused loops apply natively for a preconditioner: ``scale * (amg + diag | bjac)`` with any of the three
    absent -- the additive form of the reference's MypreA (templates/NavierStokesSIMPLE_iterative.py:383) -- or, with
    `multiplicative`, the Gauss-Seidel sweeps of `bjac` around the (auxiliary-space) AMG `amg` in its middle (GS=True,
    :376-381).  Or, alone, ``scale * fdm``: the exact inverse by fast diagonalisation (`FastDiagonalizationInverse`)."""
    scale: float
    diag: object
    bjac: object
    amg: object
    multiplicative: bool
    fdm: object = None


NO_PRE = PreParts(1.0, None, None, None, False)


def native_velocity_pre(op):
    """The `PreParts` of `op`, or None when the fused loops cannot apply it natively."""
    scale = 1.0
    if isinstance(op, ScaledMatrix):
        scale, op = op.scale, op.mat
    if isinstance(op, BlockGaussSeidel) and isinstance(op.middle, SmoothedAggregationAMG):
        return PreParts(scale, None, op, op.middle, True)
    from .fdm import FastDiagonalizationInverse              # (fdm.py imports this module)
    if isinstance(op, FastDiagonalizationInverse):
        return PreParts(scale, None, None, None, False, op) if op.handle is not None else None
    parts = [op]
    if isinstance(op, SumMatrix):
        if op.sb != 1.0:
            return None
        parts = [op.a, op.b]
    diag = bjac = amg = None
    for part in parts:
        if isinstance(part, SmoothedAggregationAMG) and amg is None:
            amg = part
        elif isinstance(part, DiagonalMatrix) and diag is None and bjac is None:
            diag = part
        elif (isinstance(part, (BlockJacobi, BlockGaussSeidel)) and diag is None and bjac is None
              and getattr(part, "middle", None) is None):
            bjac = part
        else:
            return None
    if amg is not None and isinstance(bjac, BlockGaussSeidel):
        return None
    return PreParts(scale, diag, bjac, amg, False)


def own_residual_matrix(bjac):
    """The matrix the residual between the half-sweeps of a multiplicative MypreA must be formed with when it is not the
    loop's own (A, or S in the condensed form): the handle's fp32 copy of round32(A) / round32(S) under fp32 storage --
    the residual with the rounded matrix keeps the operator symmetric.  None for fp64 storage."""
    if getattr(bjac, "storage", "fp64") == "fp32":
        return bjac.residual_mat
    return None


def fp32_storage(pa):
    """Whether any part of the PreParts `pa` stores its matrices in fp32."""
    return pa is not None and any(getattr(part, "storage", "fp64") == "fp32" for part in (pa.bjac, pa.amg))


def native_diag(op):
    """The `PreParts` of a (scaled) diagonal preconditioner (preM, preS), else None."""
    p = native_velocity_pre(op)
    return p if p is not None and p.bjac is None and p.amg is None and p.fdm is None else None


# The preconditioners each fused loop takes (BPCG v2 and the Lanczos check theirs against their other operands).
# CG further declines a ScaledMatrix or a sum (CgLoop); the partitioned loops have no AMG term.  The inverse by fast
# diagonalisation (p.fdm) goes with any scale into MINRES and the textbook BPCG, and never into the partitioned loops
# (its contractions span the slabs) or into CG (an exact inverse of the loop's own operator).
ACCEPTS = {
    "minres": lambda p: not p.multiplicative and (p.scale == 1.0 or (p.bjac is None and p.amg is None)),
    "bpcg1": lambda p: not p.multiplicative and (p.scale == 1.0 or p.amg is None),     # the scale goes into k
    "cg": lambda p: not p.multiplicative and p.fdm is None,
    "partitioned minres": lambda p: p.amg is None and p.fdm is None and ACCEPTS["minres"](p),
    "partitioned bpcg1": lambda p: p.amg is None and p.fdm is None and ACCEPTS["bpcg1"](p),
}


def pre_for(kind, op):
    """The `PreParts` of `op` when the fused loop `kind` (a key of ``ACCEPTS``) applies it, else None."""
    p = native_velocity_pre(op)
    return p if p is not None and ACCEPTS[kind](p) else None


def scaled_diag(p):
    """The entries of ``p.scale * p.diag`` (p.diag's own buffer when the scale is 1)."""
    return p.diag.d if p.scale == 1.0 else p.diag.d * p.scale


def write_pre(st, p, scale_diag=False):
    """Point the ``pre_diag`` / ``pre_bjac`` / ``pre_amg`` (/ ``pre_fdm``, where the state has it) fields of loop state
    `st` at the parts of `p`.  `scale_diag`:
    pre_diag gets ``scaled_diag(p)`` instead of p.diag's entries.  Returns the buffer pre_diag points at (None without a
    diagonal), which the loop keeps alive."""
    diag = None if p.diag is None else scaled_diag(p) if scale_diag else p.diag.d
    st.pre_diag = diag.data_ptr() if diag is not None else None
    st.pre_bjac = p.bjac.handle.ptr if p.bjac is not None else None
    st.pre_amg = p.amg.handle.ptr if p.amg is not None else None
    if hasattr(type(st), "pre_fdm"):
        st.pre_fdm = p.fdm.handle.ptr if p.fdm is not None else None
    return diag


def run_chunked(enqueue, poll, begin, end, poll_every, transport=None):
    """Drive a fused loop over iterations [begin, end): `enqueue(a, b)` issues iterations [a, b) without waiting,
    `poll_every` at a time, and `poll()` after each chunk drains the stream and returns a tuple whose first entry is the
    stop flag.  `transport`: the `distributed.MailboxTransport` of a partitioned run, whose timeouts the loop's kernels
    do not see: checked after each poll.  Returns the last poll result (one poll without iterations when the range is
    empty)."""
    it, out = begin, None
    while it < end:
        chunk_end = min(end, it + poll_every)
        enqueue(it, chunk_end)
        it = chunk_end
        out = poll()
        if transport is not None and transport.timed_out():
            raise RuntimeError("mailbox transport: a peer did not arrive within the timeout (iteration %d)" % (it - 1))
        if out[0]:
            break
    return out if out is not None else poll()


class FusedLoop:
    """The `try_create` convention of the fused loops: ``_try_create`` returns the loop or the reason (one short string)
    why not, and `_decided` keeps that reason in ``last_declined`` (None after a loop was made)."""

    last_declined = None

    @classmethod
    def _decided(cls, out):
        declined = isinstance(out, str)
        cls.last_declined = out if declined else None
        return None if declined else out

    @staticmethod
    def _engine_declined(eng):
        """The reason why no fused loop runs on `eng`, or None."""
        if not ENABLED:
            return "fused loops disabled (hipla.fused.ENABLED)"
        return None if _hip(eng) else "not the HIP engine"


def plan_for_textbook_bpcg(a_matrix, pre_a):
    """Launch plans the fused textbook BPCG loop wants, made BEFORE anything multiplies with the matrices (the scale
    factor's Lanczos runs over A: with the plan changed afterwards the first solve on fresh matrices would differ from
    later ones in the last bits of k).  Block Jacobi alone: A's row blocks around the Jacobi blocks (small systems), so
    that the launch of A's rows applies it in its epilogue.  No-op for anything that is not native."""
    if not ENABLED or not isinstance(a_matrix, SparseMatrix) or not hasattr(a_matrix.handle, "plan_for_blocks"):
        return
    pa = native_velocity_pre(pre_a)
    if pa is None or pa.amg is not None or pa.multiplicative or not isinstance(pa.bjac, BlockJacobi):
        return
    a_matrix.handle.plan_for_blocks(pa.bjac.handle)


def code_values_together(eng, mats):
    """One-byte value codes (nss_csr_code_values) for ALL of `mats` or for none of them: a matrix with more than 256
    distinct value patterns leaves the others as they were.  Whether to try at all is the library's decision
    (nss_csr_value_codes_wanted: the NSS_VALUE_CODES override, else by the rows of the largest matrix).  Returns
    whether every matrix holds codes now."""
    lib = eng.lib
    if not all(hasattr(lib, name) for name in ("nss_csr_code_values", "nss_csr_value_codes_wanted")):
        return False                                 # (older A/B builds of the library)
    if not all(isinstance(m, SparseMatrix) and hasattr(m.handle, "code_values") for m in mats):
        return False
    wanted = C.c_int32()
    eng._check(lib.nss_csr_value_codes_wanted(max(m.height for m in mats), C.byref(wanted)))
    if not wanted.value:
        return False
    newly = []
    for m in mats:
        was_coded = m.handle.value_bytes() == m.handle.nnz
        # coded means: its kernels stream the codes now (value_bytes says what they read), not merely that codes exist
        if not (m.handle.code_values() and m.handle.value_bytes() == m.handle.nnz):
            for h in newly:                          # all or nothing: what this call coded goes again
                h.drop_value_codes()
            if not was_coded:
                m.handle.drop_value_codes()
            return False
        if not was_coded:
            newly.append(m.handle)
    return True


def _extension_is_in_place_safe(H):
    """`t1 += H t1` runs in place on the device: the rows of H that hold entries (interior dofs) must
    not appear among its columns (coupling dofs)."""
    rowptr, col, _ = H.host_csr()
    rows_with_entries = np.nonzero(np.diff(rowptr))[0]
    return not np.intersect1d(rows_with_entries, np.unique(col), assume_unique=True).size


def condensed_fusable(bjac, condensed):
    """Whether the fused condensed forms (csrc/bpcg2.hip, nss_cond_fuse_mode) hold for the multiplicative MypreA `bjac`
    (a BlockGaussSeidel over S) and condensed = dict(HT, H, inner, S): (True, None) or (False, reason).  Structure
    checked once, on the host: the sweep runs in the colour-major layout with dofs outside its blocks; H^T has rows only
    at block dofs (the lifted vector is t0 outside them); S has rows and columns only at block dofs (its residual is
    k f there, and P S P^T never reads its trailing columns); A_ii^-1 is diagonal with rows only outside the blocks
    (A_ii^-1 f = A_ii^-1 t0); H has rows only outside the blocks and columns only at block dofs."""
    if getattr(bjac, "layout", None) != "colour-major":
        return False, "the sweep is not in the colour-major layout"
    if bjac.mat is not condensed.get("S"):
        return False, "the sweep is not over S"
    n = bjac.n
    inside = np.zeros(n, dtype=bool)
    inside[bjac.idx_host[bjac.idx_host >= 0]] = True
    if inside.all():
        return False, "every dof is in a block"

    def rows_cols(m):
        rowptr, col, _ = m.host_csr()
        return np.repeat(np.arange(m.height), np.diff(rowptr)), np.asarray(col)

    r, c = rows_cols(condensed["HT"])
    if not inside[r].all():
        return False, "H^T has rows outside the blocks"
    r, c = rows_cols(condensed["S"])
    if not (inside[r].all() and inside[c].all()):
        return False, "S has entries outside the blocks"
    r, c = rows_cols(condensed["inner"])
    if (r != c).any() or inside[r].any():
        return False, "A_ii^-1 is not diagonal outside the blocks"
    r, c = rows_cols(condensed["H"])
    if inside[r].any() or not inside[c].all():
        return False, "H does not map block dofs to the dofs outside the blocks"
    return True, None


def attach_condensed(bjac, condensed):
    """Build P H^T and the rows of H outside the blocks in the sweep's numbering and attach them to its handle
    (nss_bjac_set_condensed) when `condensed_fusable` holds.  Returns (attached, reason)."""
    import scipy.sparse as sp
    ok, why = condensed_fusable(bjac, condensed)
    if ok and getattr(bjac, "storage", "fp64") == "fp32":
        ok, why = False, "fp32 storage: the fused condensed forms have no fp32 kernels (the straightforward sequence runs)"
    eng = bjac.engine
    if not ok:
        if hasattr(eng, "lib"):
            eng._check(eng.lib.nss_bjac_set_condensed(bjac.handle.ptr, None, None, None, None, None, None, None))
        return False, why
    live = bjac.idx_host.T >= 0
    rowdof = bjac.idx_host.T[live].astype(np.int64)                 # the sweep's permuted row order (BlockGaussSeidel)
    n, n_perm = bjac.n, rowdof.size
    outside = np.setdiff1d(np.arange(n, dtype=np.int64), rowdof)    # ascending: the handle's trailing order
    colmap = np.empty(n, dtype=np.int64)
    colmap[rowdof] = np.arange(n_perm)
    colmap[outside] = n_perm + np.arange(outside.size)
    HTp = SparseMatrix.from_scipy(condensed["HT"].to_scipy().tocsr()[rowdof], engine=eng)
    Hrows = condensed["H"].to_scipy().tocsr()[outside].tocoo()
    Hp = sp.csr_matrix((Hrows.data, (Hrows.row, colmap[Hrows.col])), shape=(outside.size, n_perm + max(1, outside.size)))
    Hp.sort_indices()
    Hp = SparseMatrix.from_scipy(Hp, engine=eng)
    dinner = np.ascontiguousarray(condensed["inner"].to_scipy().diagonal()[outside], dtype=np.float64)
    eng._check(eng.lib.nss_bjac_set_condensed(bjac.handle.ptr, condensed["HT"].handle.ptr, condensed["H"].handle.ptr,
                                              condensed["inner"].handle.ptr, condensed["S"].handle.ptr, HTp.handle.ptr,
                                              Hp.handle.ptr, dinner.ctypes.data))
    bjac.cond_keep = (HTp, Hp)                                      # the handle points at them
    return True, None


def plan_stamp(eng, *mats):
    """Largest launch-plan generation (nss_csr_plan_generation) among raw ``nss_csr_t`` pointers (None skipped): what a
    loop state records in ``plan_gen`` when it sizes its dot partials.  A re-plan of a shared matrix
    (nss_csr_plan_for_pairs / _for_blocks, nss_amg_create_auxiliary) moves it."""
    out, gen = C.c_int64(), 0
    for ptr in mats:
        if ptr:
            eng._check(eng.lib.nss_csr_plan_generation(ptr, C.byref(out)))
            gen = max(gen, out.value)
    return gen


def fit_partials(eng, st, workspace, mats, partials=None):
    """Size the dot partials of loop state `st` for the CURRENT launch plans of its matrices (field names `mats`):
    query `workspace` (nss_*_workspace), allocate one buffer per count and record ``plan_gen`` / ``cap_*`` in the
    state.  With the buffers of an earlier call in `partials` nothing happens unless a matrix was re-planned since
    (the library refuses a stale state before any launch).  Returns the buffers (the caller keeps them alive)."""
    stamp = plan_stamp(eng, *(getattr(st, m) for m in mats))
    if partials is not None and stamp == st.plan_gen:
        return partials
    names = [n for n in ("a", "b", "c") if hasattr(type(st), "cap_" + n)]
    counts = [C.c_int64() for _ in names]
    eng._check(workspace(C.byref(st), *(C.byref(c) for c in counts)))
    partials = [eng.zeros(max(1, c.value)) for c in counts]
    for n, buf in zip(names, partials):
        setattr(st, "partials_" + n, buf.data_ptr())
        setattr(st, "cap_" + n, buf.numel())
    st.plan_gen = stamp
    return partials


def _plain(v, n):
    return isinstance(v, Vector) and v.size == n


class Bpcg2Loop(FusedLoop):
    """Device-resident iteration of solvers/bramblepasciak_new.py:200-249."""

    @classmethod
    def try_create(cls, matA, matB, matBT, preA_unscaled, k, preM, vecs, distributed=False, condensed=None,
                   dist_amg=None, ghost_rows_b=0, dist_aux=None):
        """`distributed`: the matrices are the local row blocks of a partitioned run -- their
        column spaces carry halo entries behind the owned ones and t1 / t4 / s1 are the owned
        views of halo-extended buffers (same base pointer).  `condensed`: dict(HT, H, inner[, S]) of
        `SparseMatrix` for a statically condensed form (matA is then the explicit product; S = the Schur
        complement, the matrix a multiplicative MypreA sweeps over and forms its residual with).
        `ghost_rows_b` > 0: matB carries that many ghost pressure rows behind the slab's own (the compact
        partitioned plan, nss_bpcg2_t.dist_compact).  Returns None when an operand is not native, with the
        reason in ``Bpcg2Loop.last_declined``."""
        return cls._decided(cls._try_create(matA, matB, matBT, preA_unscaled, k, preM, vecs, distributed, condensed,
                                            dist_amg, ghost_rows_b, dist_aux))

    @classmethod
    def _try_create(cls, matA, matB, matBT, preA_unscaled, k, preM, vecs, distributed=False, condensed=None,
                    dist_amg=None, ghost_rows_b=0, dist_aux=None):
        """The loop, or the reason (a string) why not."""
        if not (isinstance(matA, SparseMatrix) and isinstance(matB, SparseMatrix) and isinstance(matBT, SparseMatrix)):
            return "A, B or B^T is not a SparseMatrix"
        eng = matA.engine
        if (declined := cls._engine_declined(eng)) is not None:
            return declined
        n_u, n_p = matA.height, matB.height - int(ghost_rows_b)
        if matBT.height != n_u or (ghost_rows_b and not distributed):
            return "B^T does not match A"
        if not distributed and (matA.width != n_u or matB.width != n_u or matBT.width != n_p):
            return "matrix shapes do not match"
        if distributed and (matA.width < n_u or matB.width < n_u or matBT.width < n_p):
            return "matrix shapes do not match"
        pm = native_diag(preM)
        pa = native_velocity_pre(preA_unscaled)
        if dist_aux is not None:     # row-partitioned auxiliary-space term [+ Jacobi part | around Gauss-Seidel sweeps]
            pa = pa or NO_PRE
            if pa.amg is not None or pa.multiplicative or not distributed or dist_amg is not None:
                return "partitioned auxiliary term with another AMG term"
        elif dist_amg is not None:   # row-partitioned V-cycle (native handle) [+ an additive Jacobi part]
            pa = pa or NO_PRE
            if pa.amg is not None or pa.multiplicative or not distributed:
                return "partitioned V-cycle with another AMG term"
        if pm is None:
            return "preM is not a (scaled) diagonal"
        if pa is None:
            return "preA is not native"
        if pa.fdm is not None and (distributed or dist_amg is not None or dist_aux is not None):
            return "fast diagonalisation on a partitioned run (the contractions span the slabs)"
        if pa.fdm is not None and condensed is not None:
            return "fast diagonalisation with a condensed form (the Schur complement is no Kronecker sum)"
        if distributed and fp32_storage(pa):
            return "fp32 preconditioner storage on a partitioned run (the row-partitioned preconditioners are fp64)"
        if pa.multiplicative:
            # the sweeps' residual is formed with the loop's own A -- or, condensed, with the Schur complement S
            if distributed:
                return "multiplicative preA on a partitioned run"
            if condensed is None and pa.bjac.mat is not matA:
                return "multiplicative preA sweeps over another matrix than A"
            if condensed is not None and (condensed.get("S") is None or pa.bjac.mat is not condensed["S"]):
                return "multiplicative and condensed: the sweeps are not over the Schur complement S"
        sizes = {"u0": n_u, "d0": n_u, "w0": n_u, "s0": n_u, "z0": n_u, "q": n_u, "t0": n_u, "t1": n_u,
                 "t2": n_u, "t4": n_u, "u1": n_p, "d1": n_p, "w1": n_p, "s1": n_p, "t3": n_p}
        if any(not _plain(vecs.get(name), n) for name, n in sizes.items()):
            return "a work vector is not a plain Vector of its size"
        if condensed is not None:
            # on slabs the operators carry the columns of A's operand [owned | ghosts] (`slab`: built that way by
            # distributed.DistributedCondensedForm.native_operators; the lift / extension exchange their operands)
            if distributed and not condensed.get("slab"):
                return "condensed form on a partitioned run"
            if distributed and (dist_amg is not None or pa.amg is not None):
                return "condensed form on a partitioned run with an AMG term"
            if distributed and dist_aux is not None and not isinstance(pa.bjac, BlockGaussSeidel):
                return "condensed form on a partitioned run: the auxiliary-space term only inside the multiplicative MypreA"
            width = matA.width if distributed else n_u

            def misfit(key):
                m = condensed.get(key)
                if not isinstance(m, SparseMatrix) or m.height != n_u:
                    return True
                return not (n_u <= m.width <= width) if key == "inner" else m.width != width

            keys = ("HT", "H", "inner") + (("S",) if condensed.get("S") is not None else ())
            if any(misfit(key) for key in keys):
                return "condensed operators are not n_u x n_u SparseMatrix"
            if distributed and dist_aux is not None and condensed.get("S") is None:
                return "condensed MypreA on slabs: the sweeps' residual needs S (condensed['S'])"
            if not _extension_is_in_place_safe(condensed["H"]):
                return "harmonic extension H maps into its own columns"
        return cls(eng, matA, matB, matBT, pa, k, pm, vecs, condensed, distributed, dist_amg, n_p, dist_aux)

    def __init__(self, eng, matA, matB, matBT, pa, k, pm, vecs, condensed=None, distributed=False, dist_amg=None,
                 n_p=None, dist_aux=None):
        torch = eng.torch
        self.eng, self.lib = eng, eng.lib
        self.keep = [matA, matB, matBT, vecs, pa, pm, condensed]       # keep device memory alive
        st = Bpcg2State()
        if condensed is not None:
            self.cond_f = eng.zeros(matA.width if distributed else matA.height)     # (slabs: A_ii^-1's operand width)
            st.cond_HT, st.cond_H = condensed["HT"].handle.ptr, condensed["H"].handle.ptr
            st.cond_inner, st.cond_f = condensed["inner"].handle.ptr, self.cond_f.data_ptr()
            if distributed and dist_aux is not None:
                st.sweep_A = condensed["S"].handle.ptr      # MypreA on slabs: the residual x - S_slab y between the sweeps
            if pa.multiplicative:
                st.sweep_A = condensed["S"].handle.ptr      # the residual between the sweeps: x - S y
                # the fused condensed forms (nss_cond_fuse_mode) when the structure allows them: operators attached to
                # the sweep's handle, kept alive with the loop; otherwise the straightforward sequence
                self.cond_fusable, self.cond_fuse_declined = attach_condensed(pa.bjac, condensed)
                self.keep.append(pa.bjac)
        if pa.multiplicative and not distributed and own_residual_matrix(pa.bjac) is not None:
            # fp32 storage: the residual between the sweeps with the handle's fp32 copy of the matrix of its sweeps
            st.sweep_A = own_residual_matrix(pa.bjac).handle.ptr
        # the rows of B multiply t1 - s0 (:212-213): with row blocks short enough both vectors are read from LDS copies
        self.pair_staged_b = (os.environ.get("NSS_PAIR_STAGE", "1") == "1" and hasattr(matB.handle, "plan_for_pairs")
                              and matB.handle.plan_for_pairs())
        # block Jacobi alone as preA: B^T's row blocks are planned around its blocks and C1 applies it in its epilogue
        self.c1_applies_bjac = (pa.bjac is not None and pa.diag is None and pa.amg is None and condensed is None
                                and hasattr(matBT.handle, "plan_for_blocks") and matBT.handle.plan_for_blocks(pa.bjac.handle))
        # one-byte value codes for A, B and B^T (C1 / C23 then stream 1 byte per entry instead of 8: same bits) on the
        # single-GPU compact plan, all or nothing: info() and the launches stay consistent
        self.value_coded = (condensed is None and not distributed and code_values_together(eng, (matA, matB, matBT)))
        # the row-per-lane form of C23 (eight-slot copies of A and B) where the size rule coded the matrices: the plans
        # are settled now, and a copy belongs to one plan
        self.row_slots = (self.value_coded and all(hasattr(m.handle, "plan_row_slots") for m in (matA, matB))
                          and all([m.handle.plan_row_slots(-1) for m in (matA, matB)]))
        st.A, st.B, st.BT = matA.handle.ptr, matB.handle.ptr, matBT.handle.ptr
        write_pre(st, pa)
        st.k = float(k) * pa.scale
        self.minv = scaled_diag(pm)
        st.minv = self.minv.data_ptr()
        # a lumped-mass diagonal that is one double throughout (uniform grids) goes to C4 as one value: looked for at every
        # start(), where the codes are in force (the regime bound by bytes); tests and measurements flip the attribute
        self.uniform_diagonal = self.value_coded and hasattr(self.lib, "nss_bpcg2_uniform_diagonal")
        for name in ("u0", "u1", "d0", "d1", "w0", "w1", "s0", "s1", "z0", "q", "t0", "t1", "t2", "t3", "t4"):
            setattr(st, name, vecs[name].buf.data_ptr())
        st.n_u, st.n_p = matA.height, (matB.height if n_p is None else int(n_p))
        st.local_sums = 1 if distributed else 0     # the caller all-reduces scal[9], scal[10] into scal[1], scal[2]
        st.pre_dist_amg = dist_amg
        st.pre_dist_aux = dist_aux
        self.keep.append(dist_amg)
        self.partials = fit_partials(eng, st, self.lib.nss_bpcg2_workspace, ("A", "B", "BT"))
        self.scal = eng.zeros(16)
        self.ctrl = torch.zeros(8, dtype=torch.int32, device=eng.device)
        st.scal, st.ctrl = self.scal.data_ptr(), self.ctrl.data_ptr()
        self.hist = None
        self.state = st

    # ---- driving the loop -------------------------------------------------------------------
    def start(self, wdn, err0, tol, rel_err, maxsteps):
        """Upload the scalars of iteration 0 and clear the control words / history."""
        eng, st = self.eng, self.state
        # a matrix this loop holds may have been re-planned by another consumer since (shared B, B^T, A)
        self.partials = fit_partials(eng, st, self.lib.nss_bpcg2_workspace, ("A", "B", "BT"), self.partials)
        self.maxsteps = int(maxsteps)
        self.hist = eng.zeros(max(1, self.maxsteps))
        st.hist = self.hist.data_ptr()
        scal = np.zeros(16)
        scal[S_WD], scal[S_ERR0], scal[S_TOL], scal[S_REL] = wdn, err0, tol, 1.0 if rel_err else 0.0
        eng.upload(scal, self.scal)
        self.ctrl.zero_()
        st.minv_uniform = 0
        if getattr(self, "uniform_diagonal", False):                     # one launch, one read: minv may have changed
            eng._check(self.lib.nss_bpcg2_uniform_diagonal(C.byref(st), 1, eng.stream))

    def diagonal_by_value(self):
        """Whether C4 takes the diagonal preM as one value (found uniform at the last start()) instead of streaming it."""
        return bool(self.state.minv_uniform)

    def enqueue(self, it_begin, it_end):
        """Enqueue iterations [it_begin, it_end) on the current stream; returns immediately."""
        self.eng._check(self.lib.nss_bpcg2_iterate(C.byref(self.state), int(it_begin), int(it_end), self.eng.stream))

    def phase(self, name, it):
        self.eng._check(self.lib.nss_bpcg2_phase(C.byref(self.state), PHASE[name], int(it), self.eng.stream))

    def phases(self, first, last, it):
        self.eng._check(self.lib.nss_bpcg2_phases(C.byref(self.state), PHASE[first], PHASE[last], int(it),
                                                  self.eng.stream))

    def cphases(self, first, last, it):
        """Phases first..last of iteration `it` of the compact plan (what `enqueue` issues)."""
        self.eng._check(self.lib.nss_bpcg2_cphases(C.byref(self.state), CPHASE[first], CPHASE[last], int(it),
                                                   self.eng.stream))

    def enqueue_classic(self, it_begin, it_end):
        """The same iterations in the eight-phase form (cross-checks, measurements)."""
        self.eng._check(self.lib.nss_bpcg2_iterate_classic(C.byref(self.state), int(it_begin), int(it_end),
                                                           self.eng.stream))

    def folds_sums(self):
        out = C.c_int32()
        self.eng._check(self.lib.nss_bpcg2_folds_sums(C.byref(self.state), C.byref(out)))
        return bool(out.value)

    def c1_applies_preA(self):
        """Whether the next C1 applies the block Jacobi in its epilogue (B^T planned around the blocks, and the size
        rule / override of nss_bpcg2_fuse_block_jacobi)."""
        out = C.c_int32()
        self.eng._check(self.lib.nss_bpcg2_c1_applies_preA(C.byref(self.state), C.byref(out)))
        return bool(out.value)

    def c23_form(self):
        """What the next C23 of `enqueue` launches (nss_bpcg2_c23_form): 0 = the stream kernels in one launch, 1 = the
        row-slot kernels in one launch, 2 = two launches."""
        out = C.c_int32()
        self.eng._check(self.lib.nss_bpcg2_c23_form(C.byref(self.state), C.byref(out)))
        return out.value

    def enqueue_dist(self, dist_handle, s1, t1, t4, overlap, it_begin, it_end):
        """Row-partitioned iterations issued natively (nss_bpcg2_iterate_dist); `s1`, `t1`, `t4`: the `HaloStruct` of
        that operand, or None."""
        ref = lambda h: C.byref(h) if h is not None else None     # (compact plan: only the halo of t1 is used)
        self.eng._check(self.lib.nss_bpcg2_iterate_dist(C.byref(self.state), dist_handle, ref(s1), ref(t1), ref(t4),
                                                        int(overlap), int(it_begin), int(it_end), self.eng.stream))

    def poll(self):
        """Drain the stream; returns (done, it_final, last_it)."""
        done, it_final, last = C.c_int32(), C.c_int32(), C.c_int32()
        self.eng._check(self.lib.nss_bpcg2_poll(C.byref(self.state), C.byref(done), C.byref(it_final),
                                                C.byref(last), self.eng.stream))
        if done.value == 3:
            raise RuntimeError("mailbox transport: a peer did not arrive within the timeout (iteration %d)" % it_final.value)
        if done.value == 2:      # the reference's `alpha = wd / as_s` with as_s == 0 (:226)
            raise ZeroDivisionError("float division by zero (BPCG breakdown <s, K s> = 0 at iteration %d)"
                                    % it_final.value)
        return bool(done.value), it_final.value, last.value

    def history(self, upto):
        return self.eng.to_host(self.hist)[: upto + 1]

    def run(self, wdn, err0, tol, rel_err, maxsteps, poll_every=None):
        """Returns (it, history, converged) -- `it` as the reference's loop variable after
        the loop (index of the iteration whose stop test fired, or maxsteps-1)."""
        self.start(wdn, err0, tol, rel_err, maxsteps)
        done, it_final, _ = run_chunked(self.enqueue, self.poll, 0, maxsteps, poll_every or POLL_EVERY)
        final = it_final if done else maxsteps - 1
        return final, self.history(final), done


class MinresState(C.Structure):
    """ctypes mirror of ``nss_minres_t`` (include/nss_krylov.h)."""
    _fields_ = ([(n, C.c_void_p) for n in ("A", "B", "BT", "pre_diag", "pre_bjac", "pre_amg", "minv")]
                + [("u", C.c_void_p * 2), ("v", (C.c_void_p * 2) * 3), ("w", (C.c_void_p * 2) * 3),
                   ("z", (C.c_void_p * 2) * 2), ("kz", C.c_void_p * 2),
                   ("scal", C.c_void_p), ("ctrl", C.c_void_p), ("hist", C.c_void_p),
                   ("partials_a", C.c_void_p), ("partials_b", C.c_void_p), ("partials_c", C.c_void_p),
                   ("n_u", C.c_int32), ("n_p", C.c_int32), ("local_sums", C.c_int32)]
                + [("plan_gen", C.c_int64), ("cap_a", C.c_int64), ("cap_b", C.c_int64), ("cap_c", C.c_int64)]
                + [("pre_fdm", C.c_void_p), ("pre_fdm_scale", C.c_double)]
                + [("C", C.c_void_p), ("C_work", C.c_void_p)])


(M_DELTA, M_GAMMA, M_G2, M_ETA_OLD, M_C_OLD, M_C, M_S_OLD, M_S, M_RES_OLD, M_ERR0, M_TOL) = range(11)


def _block2(v, n_u, n_p):
    return (isinstance(v, BlockVector) and v.nblocks == 2 and _plain(v[0], n_u) and _plain(v[1], n_p))


def native_c_block(c, a, b):
    """Whether the fused MINRES and textbook BPCG loops take `c` as the lower-right block of [[a, b^T], [b, c]]: None
    (the zero block), or a `SparseMatrix` of shape n_p x n_p on the engine of `a`.  Symmetry is not checked (the
    reference does not check it either); the methods want `c` symmetric negative semi-definite."""
    if c is None:
        return True
    n_p = getattr(b, "height", None)
    return (isinstance(c, SparseMatrix) and (c.height, c.width) == (n_p, n_p)
            and c.engine is getattr(a, "engine", None))


def write_c_block(eng, st, c):
    """Point the ``C`` / ``C_work`` fields of loop state `st` at `c` (`native_c_block`) and a work vector of its
    height, which is returned for the loop to keep (None without `c`)."""
    if c is None:
        return None
    work = eng.zeros(c.height)
    st.C, st.C_work = c.handle.ptr, work.data_ptr()
    return work


class MinresLoop(FusedLoop):
    """Device-resident iteration of minres.py:96-144 for K = [[A, B^T], [B, C]] and the preconditioner
    [[preA, None], [None, preS]] (the operands run.py:45-46 builds, where K[1,1] is None).  K[1,1]: None, or the
    lower-right block of a stabilised system as an n_p x n_p `SparseMatrix` (the method wants it symmetric negative
    semi-definite; nobody checks): one launch more per iteration (csrc/minres.hip)."""

    @classmethod
    def try_create(cls, mat, pre, u, v_ring, w_ring, z_ring, kz):
        return cls._decided(cls._try_create(mat, pre, u, v_ring, w_ring, z_ring, kz))

    @classmethod
    def _try_create(cls, mat, pre, u, v_ring, w_ring, z_ring, kz):
        if not (isinstance(mat, BlockMatrix) and isinstance(pre, BlockMatrix)):
            return "K or C is not a BlockMatrix"
        if (mat.nrows, mat.ncols) != (2, 2) or (pre.nrows, pre.ncols) != (2, 2):
            return "K or C is not 2 x 2"
        A, BT, B, C11 = mat[0, 0], mat[0, 1], mat[1, 0], mat[1, 1]
        if not native_c_block(C11, A, B) or pre[0, 1] is not None or pre[1, 0] is not None:
            return "K or C has another non-zero block"
        if not all(isinstance(m, SparseMatrix) for m in (A, BT, B)):
            return "A, B or B^T is not a SparseMatrix"
        eng = A.engine
        if (declined := cls._engine_declined(eng)) is not None:
            return declined
        n_u, n_p = A.height, B.height
        if (A.width, B.width, BT.height, BT.width) != (n_u, n_u, n_u, n_p):
            return "matrix shapes do not match"
        pa, ps = pre_for("minres", pre[0, 0]), native_diag(pre[1, 1])
        if ps is None:
            return "preS is not a (scaled) diagonal"
        if pa is None:
            return "preA is not native"
        vecs = [u, kz] + list(v_ring) + list(w_ring) + list(z_ring)
        if len(v_ring) != 3 or len(w_ring) != 3 or len(z_ring) != 2 or not all(_block2(x, n_u, n_p) for x in vecs):
            return "a work vector is not a plain BlockVector of its size"
        return cls(eng, A, B, BT, pa, ps, u, v_ring, w_ring, z_ring, kz, C11)

    def __init__(self, eng, A, B, BT, pa, ps, u, v_ring, w_ring, z_ring, kz, c_block=None):
        """`pa`, `ps`: the `PreParts` of preA and preS (pre_for("minres"), native_diag).  `c_block`: the lower-right
        block of K (`native_c_block`) or None."""
        torch = eng.torch
        self.eng, self.lib = eng, eng.lib
        self.keep = [A, B, BT, pa, ps, u, v_ring, w_ring, z_ring, kz, c_block]
        st = MinresState()
        st.A, st.B, st.BT = A.handle.ptr, B.handle.ptr, BT.handle.ptr
        self.c_work = write_c_block(eng, st, c_block)
        self.dinv = write_pre(st, pa, scale_diag=True)
        st.pre_fdm_scale = float(pa.scale)
        self.minv = scaled_diag(ps)
        st.minv = self.minv.data_ptr()
        for c in range(2):
            st.u[c] = u[c].buf.data_ptr()
            st.kz[c] = kz[c].buf.data_ptr()
            for j in range(3):
                st.v[j][c] = v_ring[j][c].buf.data_ptr()
                st.w[j][c] = w_ring[j][c].buf.data_ptr()
            for j in range(2):
                st.z[j][c] = z_ring[j][c].buf.data_ptr()
        st.n_u, st.n_p = A.height, B.height
        self.partials = fit_partials(eng, st, self.lib.nss_minres_workspace, ("A", "B", "BT"))
        self.scal = eng.zeros(64)           # two sets of 32 scalars, double-buffered by the parity of k
        self.ctrl = torch.zeros(4, dtype=torch.int32, device=eng.device)
        st.scal, st.ctrl = self.scal.data_ptr(), self.ctrl.data_ptr()
        self.state = st
        self.hist = None

    def enqueue(self, k_begin, k_end):
        self.eng._check(self.lib.nss_minres_iterate(C.byref(self.state), k_begin, k_end, self.eng.stream))

    def poll(self):
        """Drain the stream; returns (stop, k_stop, reason)."""
        stop, k_stop, reason, last = C.c_int32(), C.c_int32(), C.c_int32(), C.c_int32()
        self.eng._check(self.lib.nss_minres_poll(C.byref(self.state), C.byref(stop), C.byref(k_stop), C.byref(reason),
                                                 C.byref(last), self.eng.stream))
        return bool(stop.value), k_stop.value, reason.value

    def run(self, gamma, tol, maxsteps, poll_every=None, enqueue=None, transport=None):
        """Iterations k = 1.. as the reference's while loop.  Returns (errors, hit_relative_tol).  `enqueue`: the
        schedule of a partitioned run (distributed.DistributedMinres), `transport`: its mailbox transport."""
        eng, st = self.eng, self.state
        self.partials = fit_partials(eng, st, self.lib.nss_minres_workspace, ("A", "B", "BT"), self.partials)
        self.hist = eng.zeros(maxsteps + 2)
        st.hist = self.hist.data_ptr()
        scal = np.zeros(64)                 # iteration k = 1 reads the first set
        scal[M_GAMMA], scal[M_ETA_OLD], scal[M_C_OLD], scal[M_C] = gamma, gamma, 1.0, 1.0
        scal[M_RES_OLD], scal[M_ERR0], scal[M_TOL] = gamma, gamma, tol
        scal[16:19] = 1.0                   # factors of the (here: normalised) z, v, v_old -- see csrc/minres.hip
        eng.upload(scal, self.scal)
        self.ctrl.zero_()
        stop, k_stop, reason = run_chunked(enqueue or self.enqueue, self.poll, 1, maxsteps + 1, poll_every or POLL_EVERY,
                                           transport)
        last_k = k_stop if stop else maxsteps
        errors = [1.0] + [float(x) for x in eng.to_host(self.hist)[1: last_k + 1]]
        return errors, bool(stop and reason == 1)


class Bpcg1State(C.Structure):
    """ctypes mirror of ``nss_bpcg1_t`` (include/nss_krylov.h)."""
    _fields_ = ([(n, C.c_void_p) for n in ("A", "B", "BT", "pre_diag", "pre_bjac", "pre_amg", "minv")]
                + [(n, C.c_void_p * 2) for n in ("x", "r", "d", "a", "t1", "t2")]
                + [("scal", C.c_void_p), ("ctrl", C.c_void_p), ("hist", C.c_void_p),
                   ("partials_a", C.c_void_p), ("partials_b", C.c_void_p), ("partials_c", C.c_void_p),
                   ("k", C.c_double), ("n_u", C.c_int32), ("n_p", C.c_int32), ("local_sums", C.c_int32)]
                + [("plan_gen", C.c_int64), ("cap_a", C.c_int64), ("cap_b", C.c_int64), ("cap_c", C.c_int64)]
                + [("pre_fdm", C.c_void_p)]
                + [("C", C.c_void_p), ("C_work", C.c_void_p)])


class Bpcg1Loop(FusedLoop):
    """Device-resident iteration of bramble_pasciak_cg.py:110-143.  `c_matrix`: None, or the lower-right block of a
    stabilised system as an n_p x n_p `SparseMatrix` (the method wants it symmetric negative semi-definite; as in the
    reference, nobody checks): one launch more per iteration (csrc/bpcg1.hip)."""

    @classmethod
    def try_create(cls, a_matrix, b_matrix, c_matrix, pre_a, pre_s, k, vecs):
        return cls._decided(cls._try_create(a_matrix, b_matrix, c_matrix, pre_a, pre_s, k, vecs))

    @classmethod
    def _try_create(cls, a_matrix, b_matrix, c_matrix, pre_a, pre_s, k, vecs):
        if not native_c_block(c_matrix, a_matrix, b_matrix):
            return "C is given"
        if not (isinstance(a_matrix, SparseMatrix) and isinstance(b_matrix, SparseMatrix)):
            return "A or B is not a SparseMatrix"
        eng = a_matrix.engine
        if (declined := cls._engine_declined(eng)) is not None:
            return declined
        n_u, n_p = a_matrix.height, b_matrix.height
        if a_matrix.width != n_u or b_matrix.width != n_u:
            return "matrix shapes do not match"
        pa, ps = pre_for("bpcg1", pre_a), native_diag(pre_s)
        if ps is None:
            return "preS is not a (scaled) diagonal"
        if pa is None:
            return "preA is not native"
        if any(not _block2(vecs.get(name), n_u, n_p) for name in ("x", "r", "d", "a", "t1", "t2")):
            return "a work vector is not a plain BlockVector of its size"
        return cls(eng, a_matrix, b_matrix, pa, ps, k, vecs, None, c_matrix)

    def __init__(self, eng, A, B, pa, ps, k, vecs, BT=None, c_block=None):
        """`pa`, `ps`: the `PreParts` of preA and preS (pre_for("bpcg1"), native_diag).  `BT`: the rows of B^T this
        process owns, when they are not the transpose of its B (row-partitioned runs: distributed.Bpcg1DistLoop).
        `c_block`: the lower-right block C (`native_c_block`) or None."""
        torch = eng.torch
        self.eng, self.lib = eng, eng.lib
        if BT is None:
            BT = B.CreateTranspose()
        self.keep = [A, B, BT, pa, ps, vecs, c_block]
        st = Bpcg1State()
        st.A, st.B, st.BT = A.handle.ptr, B.handle.ptr, BT.handle.ptr
        self.c_work = write_c_block(eng, st, c_block)
        write_pre(st, pa)
        # block Jacobi alone: A's row blocks are planned around its blocks (small systems) and the launch of A's rows
        # applies it in its epilogue (csrc/bpcg1.hip: EpiV1Rows)
        if pa.bjac is not None and pa.amg is None and hasattr(A.handle, "plan_for_blocks"):
            A.handle.plan_for_blocks(pa.bjac.handle)
        st.k = float(k) * pa.scale
        self.minv = scaled_diag(ps)
        st.minv = self.minv.data_ptr()
        for name in ("x", "r", "d", "a", "t1", "t2"):
            arr = getattr(st, name)
            for c in range(2):
                arr[c] = vecs[name][c].buf.data_ptr()
        st.n_u, st.n_p = A.height, B.height
        self.partials = fit_partials(eng, st, self.lib.nss_bpcg1_workspace, ("A", "B", "BT"))
        self.scal = eng.zeros(16)
        self.ctrl = torch.zeros(4, dtype=torch.int32, device=eng.device)
        st.scal, st.ctrl = self.scal.data_ptr(), self.ctrl.data_ptr()
        self.state = st
        self.hist = None

    def enqueue(self, it_begin, it_end):
        self.eng._check(self.lib.nss_bpcg1_iterate(C.byref(self.state), it_begin, it_end, self.eng.stream))

    def poll(self):
        """Drain the stream; returns (stop, it_stop)."""
        stop, it_stop, last = C.c_int32(), C.c_int32(), C.c_int32()
        self.eng._check(self.lib.nss_bpcg1_poll(C.byref(self.state), C.byref(stop), C.byref(it_stop), C.byref(last),
                                                self.eng.stream))
        return bool(stop.value), it_stop.value

    def run(self, rho, err0, tolerance, max_steps, poll_every=None, enqueue=None, transport=None):
        """Returns (errors, converged): errors[i] = err_i/err_0 as appended at :118.  `enqueue`: the schedule of a
        partitioned run (distributed.Bpcg1DistLoop), `transport`: its mailbox transport."""
        eng, st = self.eng, self.state
        self.partials = fit_partials(eng, st, self.lib.nss_bpcg1_workspace, ("A", "B", "BT"), self.partials)
        self.hist = eng.zeros(max(1, max_steps))
        st.hist = self.hist.data_ptr()
        scal = np.zeros(16)
        scal[0], scal[5], scal[6] = rho, err0, tolerance
        eng.upload(scal, self.scal)
        self.ctrl.zero_()
        stop, it_stop = run_chunked(enqueue or self.enqueue, self.poll, 0, max_steps, poll_every or POLL_EVERY, transport)
        count = it_stop + 1 if stop else max_steps
        return [float(x) for x in eng.to_host(self.hist)[:count]], stop


class CgState(C.Structure):
    """ctypes mirror of ``nss_cg_t`` (include/nss_krylov.h)."""
    _fields_ = ([(n, C.c_void_p) for n in ("A", "pre_diag", "pre_bjac", "pre_amg", "x", "r", "z", "p", "q",
                                           "scal", "ctrl", "hist", "partials_a", "partials_b")]
                + [("n", C.c_int32), ("plan_gen", C.c_int64), ("cap_a", C.c_int64), ("cap_b", C.c_int64)]
                + [("shift_mass", C.c_void_p), ("shift_m0", C.c_double), ("shift_sigma", C.c_double)])


class CgLoop(FusedLoop):
    """Device-resident preconditioned CG (``nss_cg_*``) behind `hipla.CGSolver`."""

    @classmethod
    def try_create(cls, mat, pre):
        return cls._decided(cls._try_create(mat, pre))

    @classmethod
    def _try_create(cls, mat, pre):
        if not isinstance(mat, SparseMatrix) or mat.height != mat.width:
            return "the matrix is not a square SparseMatrix"
        eng = mat.engine
        if (declined := cls._engine_declined(eng)) is not None:
            return declined
        if isinstance(pre, (ScaledMatrix, SumMatrix)):
            return "the preconditioner is scaled or a sum"
        pa = NO_PRE if pre is None else pre_for("cg", pre)
        if pa is None:
            return "the preconditioner is not native"
        return cls(eng, mat, pa)

    def __init__(self, eng, mat, pa, shift=None):
        """`pa`: the `PreParts` of the preconditioner (NO_PRE: none).  `shift` = (mass, diag): the loop solves with
        ``M + sigma mat`` read from `mat` itself (the shifted C1 of csrc/cg.hip), sigma given by `set_shift` before the
        first solve; `mass`: host array of the lumped mass (uniform: passed by value) and `diag`: device buffer, the
        diagonal of `mat`.  A shifted loop takes the point-Jacobi preconditioner of its operator, which `set_shift`
        writes, and no other (`pa` is ignored)."""
        torch = eng.torch
        n = mat.height
        self.shift = self.sigma = None
        if shift is not None:
            from types import SimpleNamespace
            mass, diag = np.asarray(shift[0], dtype=np.float64), shift[1]
            if mass.shape != (n,) or diag.numel() != n:
                raise ValueError("CgLoop: the shift wants the mass and the diagonal of the matrix, %d entries each" % n)
            uniform = bool(n) and bool((mass == mass[0]).all())
            self.shift = (None if uniform else eng.from_host(mass), float(mass[0]) if uniform else 0.0, diag)
            pa = PreParts(1.0, SimpleNamespace(d=eng.zeros(n)), None, None, False)
        self.eng, self.lib, self.mat, self.pa = eng, eng.lib, mat, pa
        self.work = {name: eng.zeros(n) for name in ("r", "z", "p", "q")}
        st = CgState()
        st.A, st.n = mat.handle.ptr, n
        write_pre(st, pa)
        for name, buf in self.work.items():
            setattr(st, name, buf.data_ptr())
        self.partials = fit_partials(eng, st, self.lib.nss_cg_workspace, ("A",))
        self.scal = eng.zeros(8)
        self.ctrl = torch.zeros(4, dtype=torch.int32, device=eng.device)
        st.scal, st.ctrl = self.scal.data_ptr(), self.ctrl.data_ptr()
        if self.shift is not None:
            st.shift_mass = None if self.shift[0] is None else self.shift[0].data_ptr()
            st.shift_m0 = self.shift[1]
        self.state = st
        self.hist = None

    def set_shift(self, sigma):
        """The operator becomes M + `sigma` mat: writes the state's sigma and the Jacobi preconditioner
        1 / (m + sigma diag) (one element-wise launch).  Nothing happens when `sigma` is the current one."""
        if self.shift is None:
            raise ValueError("CgLoop.set_shift: the loop was made without a shift")
        sigma = float(sigma)
        if not (sigma > 0.0 and np.isfinite(sigma)):
            raise ValueError("CgLoop.set_shift: sigma is positive and finite, not %r" % (sigma,))
        if sigma == self.sigma:
            return
        mass, m0, diag = self.shift
        self.eng._check(self.lib.nss_cg_shift_jacobi_f64(self.mat.height, None if mass is None else mass.data_ptr(), m0,
                                                         sigma, diag.data_ptr(), self.pa.diag.d.data_ptr(),
                                                         self.eng.stream))
        self.state.shift_sigma = self.sigma = sigma

    def enqueue(self, it_begin, it_end):
        if self.shift is not None and self.sigma is None:
            raise ValueError("CgLoop: a shifted loop wants set_shift(sigma) before its first solve")
        self.eng._check(self.lib.nss_cg_iterate(C.byref(self.state), it_begin, it_end, self.eng.stream))

    def poll(self):
        """Drain the stream; returns (done, it_final)."""
        done, it_final, last = C.c_int32(), C.c_int32(), C.c_int32()
        self.eng._check(self.lib.nss_cg_poll(C.byref(self.state), C.byref(done), C.byref(it_final), C.byref(last),
                                             self.eng.stream))
        return bool(done.value), it_final.value

    def solve(self, b, x, precision, maxsteps, poll_every=None):
        """x = mat^-1 b from x = 0.  Returns (iterations, errors) with errors[0] = err0."""
        from math import sqrt
        eng, st, w, pa = self.eng, self.state, self.work, self.pa
        self.partials = fit_partials(eng, st, self.lib.nss_cg_workspace, ("A",), self.partials)
        eng.fill(x, 0.0)
        eng.copy(b, w["r"])
        if pa.diag is not None:
            eng.diag_apply(pa.diag.d, 1.0, w["r"], 0.0, w["z"])
        elif pa.bjac is not None:
            eng.bjac_apply(pa.bjac.handle, 1.0, w["r"], 0.0, w["z"])
        elif pa.amg is not None:
            eng.amg_apply(pa.amg.handle, 1.0, w["r"], w["z"])
        else:
            eng.copy(w["r"], w["z"])
        eng.copy(w["z"], w["p"])
        rz = eng.dot(w["r"], w["z"])
        err0 = sqrt(abs(rz))
        if err0 == 0.0:
            return 0, [0.0]
        self.hist = eng.zeros(max(1, maxsteps))
        st.hist, st.x = self.hist.data_ptr(), x.data_ptr()
        scal = np.zeros(8)
        scal[0], scal[3], scal[4] = rz, err0, precision
        eng.upload(scal, self.scal)
        self.ctrl.zero_()
        done, it_final = run_chunked(self.enqueue, self.poll, 0, maxsteps, poll_every or POLL_EVERY)
        count = it_final + 1 if done else maxsteps
        return count, [err0] + [float(v) for v in eng.to_host(self.hist)[:count]]

    def solve_resident(self, b, x, precision, maxsteps, poll_every=None):
        """As `solve`, started on the device (``nss_cg_start``): no dot product on the host, no upload, no allocation
        after the first call and no history download -- the only synchronisations are the polls.  Returns the iteration
        count (0 for a zero right-hand side)."""
        eng, st = self.eng, self.state
        self.partials = fit_partials(eng, st, self.lib.nss_cg_workspace, ("A",), self.partials)
        if self.hist is None or self.hist.numel() < max(1, maxsteps):
            self.hist = eng.zeros(max(1, maxsteps))
        st.hist, st.x = self.hist.data_ptr(), x.data_ptr()
        eng._check(self.lib.nss_cg_start(C.byref(st), b.data_ptr(), float(precision), eng.stream))
        done, it_final = run_chunked(self.enqueue, self.poll, 0, maxsteps, poll_every or POLL_EVERY)
        return it_final + 1 if done else maxsteps


class BicgstabState(C.Structure):
    """ctypes mirror of ``nss_bicgstab_t`` (include/nss_krylov.h)."""
    _fields_ = ([(n, C.c_void_p) for n in ("A", "avg", "diff", "adv", "shift_mass")]
                + [("shift_m0", C.c_double), ("shift_sigma", C.c_double), ("pre_diag", C.c_void_p), ("pre_fdm", C.c_void_p)]
                + [(n, C.c_void_p) for n in ("x", "r", "rhat", "p", "v", "t", "phat", "shat", "scal", "ctrl", "hist",
                                             "partials_a", "partials_b")]
                + [("n", C.c_int32), ("nflux", C.c_int32), ("plan_gen", C.c_int64), ("cap_a", C.c_int64),
                   ("cap_b", C.c_int64)])


class ConvectiveForm(NamedTuple):
    """The device operands of form (ii) of the BiCGStab loop, ``y = m v + sigma [L | Dv] [v | F(a; v)]``: `rows` = the
    `SparseMatrix` [L | Dv] (n rows, n + nflux columns), `avg` and `diff` (nflux x n, at most two entries per row), `adv`
    = the device buffer of a (nflux entries; its owner rewrites it once per step) and `mass` = (device buffer or None,
    m0): the mass vector, or its one value when it is uniform."""
    rows: object
    avg: object
    diff: object
    adv: object
    mass: tuple

    @staticmethod
    def mass_operand(eng, mass):
        mass = np.asarray(mass, dtype=np.float64)
        uniform = bool(mass.size) and bool((mass == mass[0]).all())
        return (None, float(mass[0])) if uniform else (eng.from_host(mass), 0.0)


class BicgstabLoop(FusedLoop):
    """Device-resident right-preconditioned BiCGStab (``nss_bicgstab_*``, csrc/bicgstab.hip) behind
    `hipla.BiCGStabSolver` and the linearly implicit convection step of `hipla.stepping.TimeStepper`.  Form (i): a
    square `SparseMatrix`; form (ii): a `ConvectiveForm`.  Preconditioners: none, an inverse diagonal (a device buffer),
    or -- form (ii) -- the direct viscous inverse of a `ComponentFastDiagonalization`, applied with the loop's sigma."""

    CODES = {1: "<rhat, v> or rho is zero or not finite", 2: "<t, t> is zero before convergence"}

    @classmethod
    def try_create(cls, mat, pre):
        return cls._decided(cls._try_create(mat, pre))

    @classmethod
    def _try_create(cls, mat, pre):
        from .fdm import ComponentFastDiagonalization            # (fdm.py imports this module)
        from .stepping import LinearisedConvection
        convective = isinstance(mat, LinearisedConvection)
        if not convective and (not isinstance(mat, SparseMatrix) or mat.height != mat.width):
            return "the matrix is neither a square SparseMatrix nor a LinearisedConvection"
        eng = mat.engine
        if (declined := cls._engine_declined(eng)) is not None:
            return declined
        if not hasattr(eng.lib, "nss_bicgstab_iterate"):
            return "the library has no BiCGStab loop"
        diag = fdm_pre = None
        if isinstance(pre, ComponentFastDiagonalization):
            if not convective or pre.handle is None or pre.n != mat.height:
                return "the direct viscous inverse goes with a LinearisedConvection of its size on the HIP engine"
            fdm_pre = pre
        elif isinstance(pre, DiagonalMatrix):
            if pre.n != mat.height:
                return "the diagonal preconditioner has another size"
            diag = pre.d
        elif pre is not None:
            return "the preconditioner is not native"
        if convective:
            form = mat.device_form()
            if form is None:
                return "the LinearisedConvection holds no device operands"
            return cls(eng, form.rows, diag, form, fdm_pre, op=mat)
        return cls(eng, mat, diag)

    def __init__(self, eng, mat, diag=None, form=None, fdm_pre=None, op=None):
        """`mat`: the square matrix, or [L | Dv] of `form`; `diag`: device buffer of the inverse diagonal or None;
        `fdm_pre`: a `ComponentFastDiagonalization` or None; `op`: the `LinearisedConvection` whose sigma a solve reads
        (None: `set_sigma`)."""
        torch = eng.torch
        n = mat.height
        self.eng, self.lib, self.mat, self.form, self.op = eng, eng.lib, mat, form, op
        self.keep = (diag, fdm_pre)
        self.work = {name: eng.zeros(n) for name in ("r", "rhat", "p", "v", "t")}
        self.work.update({name: eng.zeros(mat.width) for name in ("phat", "shat")})
        st = BicgstabState()
        st.A, st.n, st.nflux = mat.handle.ptr, n, mat.width - n
        if form is not None:
            st.avg, st.diff, st.adv = form.avg.handle.ptr, form.diff.handle.ptr, form.adv.data_ptr()
            st.shift_mass = None if form.mass[0] is None else form.mass[0].data_ptr()
            st.shift_m0 = form.mass[1]
        st.pre_diag = None if diag is None else diag.data_ptr()
        st.pre_fdm = None if fdm_pre is None else fdm_pre.handle.ptr
        for name, buf in self.work.items():
            setattr(st, name, buf.data_ptr())
        self.partials = fit_partials(eng, st, self.lib.nss_bicgstab_workspace, ("A",))
        self.scal = eng.zeros(16)
        self.ctrl = torch.zeros(4, dtype=torch.int32, device=eng.device)
        st.scal, st.ctrl = self.scal.data_ptr(), self.ctrl.data_ptr()
        self.state = st
        self.hist = None
        self.code = 0
        self.last_count = None        # iterations of the last solve: the size of the next solve's first chunk

    def set_sigma(self, sigma):
        """Form (ii): the operator becomes M + `sigma` (L + N(a)) -- by value, nothing is launched."""
        sigma = float(sigma)
        if self.form is None or not (sigma >= 0.0 and np.isfinite(sigma)):
            raise ValueError("BicgstabLoop.set_sigma: a form-(ii) loop, and a sigma that is non-negative and finite")
        self.state.shift_sigma = sigma

    def write_jacobi(self, dinv):
        """Form (ii): the point-Jacobi diagonal of the operator for the current a and sigma into the device buffer `dinv`
        (one launch; once per step, after a was frozen)."""
        self.eng._check(self.lib.nss_bicgstab_jacobi_f64(C.byref(self.state), dinv.data_ptr(), self.eng.stream))

    def apply(self, operand, y):
        """y = Op v for the v in the first n entries of the device buffer `operand` (the columns of `mat` long; form (ii)
        writes the flux behind v)."""
        self.eng._check(self.lib.nss_bicgstab_apply_f64(C.byref(self.state), operand.data_ptr(), y.data_ptr(),
                                                        self.eng.stream))

    def enqueue(self, it_begin, it_end):
        self.eng._check(self.lib.nss_bicgstab_iterate(C.byref(self.state), it_begin, it_end, self.eng.stream))

    def poll(self):
        """Drain the stream; returns (done, it_final, code)."""
        done, it_final, last, code = C.c_int32(), C.c_int32(), C.c_int32(), C.c_int32()
        self.eng._check(self.lib.nss_bicgstab_poll(C.byref(self.state), C.byref(done), C.byref(it_final), C.byref(last),
                                                   C.byref(code), self.eng.stream))
        return bool(done.value), it_final.value, code.value

    def solve_resident(self, b, x, precision, maxsteps, poll_every=None):
        """x = Op^-1 b from x = 0, started on the device (``nss_bicgstab_start``): no allocation after the first call, no
        history download -- the only synchronisations are the polls.  Returns the iteration count (0 for a zero
        right-hand side, `maxsteps` when the cap was reached); the breakdown code (0: none) is left in `self.code`."""
        eng, st = self.eng, self.state
        if self.op is not None:
            self.set_sigma(self.op.sigma)
        self.partials = fit_partials(eng, st, self.lib.nss_bicgstab_workspace, ("A",), self.partials)
        if self.hist is None or self.hist.numel() < max(1, maxsteps):
            self.hist = eng.zeros(max(1, maxsteps))
        st.hist, st.x = self.hist.data_ptr(), x.data_ptr()
        eng._check(self.lib.nss_bicgstab_start(C.byref(st), b.data_ptr(), float(precision), eng.stream))
        # The first chunk is what the last solve needed, plus one: a solve of a time step repeats the count of the step
        # before, and every iteration enqueued past the stop is 8 to 22 launches that return at once.  The chunking
        # changes no bit: the loop freezes in the iteration where it stops.
        every = poll_every or POLL_EVERY
        first = every if self.last_count is None else max(1, min(every, self.last_count + 1))
        out = run_chunked(self.enqueue, self.poll, 0, min(first, maxsteps), first)
        if not out[0] and first < maxsteps:
            out = run_chunked(self.enqueue, self.poll, first, maxsteps, every)
        done, it_final, self.code = out
        self.last_count = it_final + 1 if done else maxsteps
        return self.last_count

    def solve(self, b, x, precision, maxsteps, poll_every=None):
        """As `solve_resident`, with the history read back.  Returns (iterations, errors, code), errors[0] = |b|."""
        count = self.solve_resident(b, x, precision, maxsteps, poll_every)
        err0 = float(self.eng.to_host(self.scal)[9])
        return count, [err0] + [float(v) for v in self.eng.to_host(self.hist)[:count]], self.code


# The integrators in time live in hipla/stepping.py; their public names stay importable from here.
from .stepping import (CONVECTION_SCHEMES, HeatIntegrator, HeatRecord, ScalarStepper, StepRecord,  # noqa: E402,F401
                       TimeStepper, check_convection, constants_in_kernel, two_entry_rows, upload_stencil)
