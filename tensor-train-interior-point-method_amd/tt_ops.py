"""TT algebra on the MI355X -- drop-in for the reference's `cy_src/tt_ops_cy.pyx` kernels and
`src/tt_ops.py` helpers (same names, argument meaning, in-place semantics and RNG coupling).

TT cores are fp64 device tensors; every arithmetic step is a libttk HIP kernel (dev.py).  The
only host<->device traffic is the singular values that drive truncation (`prune_singular_vals`
runs on the host, exactly as the reference decides ranks) and the scalars of inner products.

Semantics kept from the reference:
  * `tt_scale` rounds alpha to fp32 and scales ONE core chosen with `np.random.randint`
    (`cy_src/tt_ops_cy.pyx:94-114`) -- the host MT19937 stream is consumed identically;
  * `tt_normalise` truncates the radius to a C int (`cy_src/tt_ops_cy.pyx:524`);
  * `tt_rl_orthogonalise` / `tt_rank_reduce` overwrite the caller's list slots in place.
"""
from functools import reduce

import ctypes
import os

import numpy as np
from . import dev as D
from . import rng as _rng
from ._lib import AffineJob, AffineTerm, SumTerm

def _const(name, arr):
    """Small constant cores, uploaded once per host thread (on that thread's stream)."""
    c = D._TL.consts
    t = c.get(name)
    if t is None:
        t = D.from_numpy(arr)
        c[name] = t
    return t


def _eye_core():
    return _const("eyecore", np.eye(2).reshape(1, 2, 2, 1))


def E(i, j):
    """`src/tt_ops.py:16-19`"""
    e = np.zeros((1, 2, 2, 1))
    e[:, i, j] += 1
    return _const(f"E{i}{j}", e)


def to_device(tt):
    return [D.from_numpy(c) for c in tt]


def to_host(tt):
    return [D.read(c) for c in tt]


# ------------------------------------------------------------------ constructors (`:19-53`)
def tt_identity(dim):
    c = _eye_core()
    return [c] * dim


def tt_zero_matrix(dim):
    c = _const("zero", np.zeros((1, 2, 2, 1)))
    return [c] * dim


def tt_one_matrix(dim):
    c = _const("one", np.ones((1, 2, 2, 1)))
    return [c] * dim


def tt_ranks(tt):
    """`cy_src/tt_ops_cy.pyx:82-92`"""
    return [int(c.shape[0]) for c in tt[1:]]


def tt_transpose(tt):
    """`cy_src/tt_ops_cy.pyx:57-78` (views)."""
    k = int(np.argmax([c.dim() for c in tt]))
    return list(tt[:k]) + [c.transpose(1, 2) for c in tt[k:]]


def tt_swap_all(tt):
    """`cy_src/tt_ops_cy.pyx:118-128` (views)."""
    return [c.transpose(0, -1) for c in tt[::-1]]


def tt_scale(alpha, tt):
    """`cy_src/tt_ops_cy.pyx:94-114`: fp32 alpha, one random core."""
    n = len(tt)
    idx = _rng.R().randint(0, n)
    out = list(tt)
    out[idx] = D.scaled(tt[idx], float(np.float32(alpha)))
    return out


DEV_JOIN = os.environ.get("TTIPM_DEV_JOIN", "1") == "1"


def _join(a, b, mode):
    """one-launch assembly (ttk_tt_join) for contiguous cores; None if not applicable."""
    if DEV_JOIN and a.is_contiguous() and b.is_contiguous() and a.dim() >= 2 and a.shape[1:-1] == b.shape[1:-1]:
        ra, Ra, rb, Rb = a.shape[0], a.shape[-1], b.shape[0], b.shape[-1]
        if (mode == 1 and ra != rb) or (mode == 2 and Ra != Rb):
            return None
        mid = int(np.prod(a.shape[1:-1])) if a.dim() > 2 else 1
        out = D.empty(ra if mode == 1 else ra + rb, *a.shape[1:-1], Ra if mode == 2 else Ra + Rb)
        D.check(D.lib.ttk_tt_join(D._stream(), a.data_ptr(), b.data_ptr(), out.data_ptr(), ra, Ra, rb, Rb, mid,
                                  mode), "tt_join")
        return out
    return None


def _block_diag(a, b):
    """`cy_src/tt_ops_cy.pyx:228-241`"""
    out = _join(a, b, 0)
    if out is not None:
        return out
    out = D.zeros(a.shape[0] + b.shape[0], *a.shape[1:-1], a.shape[-1] + b.shape[-1])
    D.copy_(out[:a.shape[0], ..., :a.shape[-1]], a)
    D.copy_(out[a.shape[0]:, ..., a.shape[-1]:], b)
    return out


def _cat(a, b, axis):
    out = _join(a, b, 2 if axis == 0 else 1)
    if out is not None:
        return out
    shp = list(a.shape)
    shp[axis] += b.shape[axis]
    out = D.empty(*shp)
    if axis == 0:
        D.copy_(out[:a.shape[0]], a)
        D.copy_(out[a.shape[0]:], b)
    else:
        D.copy_(out[..., :a.shape[-1]], a)
        D.copy_(out[..., a.shape[-1]:], b)
    return out


def tt_add(t1, t2):
    """`cy_src/tt_ops_cy.pyx:243-258`: rank-additive (block-diagonal) sum."""
    if len(t1) == 1:
        out = D.clone(t1[0])
        D.copy_(out, t2[0], 1.0, 1.0)
        return [out]
    return ([_cat(t1[0], t2[0], -1)] + [_block_diag(a, b) for a, b in zip(t1[1:-1], t2[1:-1])]
            + [_cat(t1[-1], t2[-1], 0)])


def tt_sub(t1, t2):
    """`src/tt_ops.py:189-190`"""
    return tt_add(t1, tt_scale(-1, t2))


def _inner_eq(nd):
    return "ab,aiA,biB->AB" if nd == 3 else "ab,aijA,bijB->AB"


def tt_inner_prod_dev(t1, t2):
    """Left-to-right contraction chain (`cy_src/tt_ops_cy.pyx:504-520`), result on the device."""
    res = _const("one11", np.ones((1, 1)))
    for c1, c2 in zip(t1, t2):
        res = D.einsum(_inner_eq(c1.dim()), res, c1, c2)
    return res


def tt_inner_prod(t1, t2):
    return float(D.read(tt_inner_prod_dev(t1, t2))[0, 0])


def tt_norm(tt):
    """`src/tt_ops.py:306-310`"""
    return norm_from_ip(tt_inner_prod(tt, tt))


def norm_from_ip(ip):
    """tt_norm's formula on a read-back <tt, tt>"""
    return float(np.sqrt(ip)) if ip > 0 else 0.0


def tt_scalars(specs):
    """Several TT scalars with ONE host read: ("ip", t1, t2) = tt_inner_prod(t1, t2), ("sum", tt) =
    tt_entrywise_sum(tt).  Each contraction chain is the one of the single-value function (same
    launches, same order); its last step writes straight into the chain's slot of one buffer."""
    buf = D.empty(max(len(specs), 1))
    with D.einsum_batch():  # the chains are independent: their steps grouped level by level
        _scalar_chains(specs, buf)
    return [float(v) for v in D.read(buf[:len(specs)])] if specs else []


def _scalar_chains(specs, buf):
    for i, sp in enumerate(specs):
        slot = buf[i:i + 1].view(1, 1)
        if sp[0] == "ip":
            t1, t2 = sp[1], sp[2]
            res = _const("one11", np.ones((1, 1)))
            for j, (c1, c2) in enumerate(zip(t1, t2)):
                res = D.einsum(_inner_eq(c1.dim()), res, c1, c2, out=slot if j == len(t1) - 1 else None)
        else:
            tt = sp[1]
            eq = "ab,aijm,bijn->mn" if tt[0].dim() == 4 else "ab,aim,bin->mn"
            one = _const("ones_" + "x".join(map(str, tt[0].shape[1:-1])), np.ones((1, *tt[0].shape[1:-1], 1)))
            res = _const("one11", np.ones((1, 1)))
            for j, c in enumerate(tt):
                res = D.einsum(eq, res, c, one, out=slot if j == len(tt) - 1 else None)


def tt_normalise(tt, radius=1):
    """`cy_src/tt_ops_cy.pyx:522-526` (int radius)."""
    factor = np.divide(int(radius), np.sqrt(tt_inner_prod(tt, tt)))
    return tt_scale(factor, tt)


def tt_random_gaussian(target_ranks, shape=(2,)):
    """`cy_src/tt_ops_cy.pyx:528-533` (host MT19937 draws, uploaded)."""
    rk = [1] + list(target_ranks) + [1]
    cores = [D.from_numpy(np.divide(1, a * int(np.prod(shape)) * b) * _rng.R().randn(a, *shape, b))
             for a, b in zip(rk[:-1], rk[1:])]
    return tt_normalise(cores)


def symmetric_powers_of_two(length):
    """`cy_src/tt_ops_cy.pyx:538-554`"""
    if length <= 0:
        return np.array([], dtype=np.int64)
    half = length // 2
    out = np.empty(length, dtype=np.int64)
    for i in range(half):
        out[i] = 1 << (i + 1)
    if length % 2:
        out[half] = 1 << (half + 1)
    for i in range(half):
        out[length - 1 - i] = out[i]
    return out


def add_kick_rank(u, v, r_add=2):
    """`cy_src/tt_ops_cy.pyx:557-578`"""
    old_r = u.shape[1]
    uk = D.from_numpy(_rng.R().randn(u.shape[0], r_add))
    if D.SPLIT_KICK:  # one launch (ttk_split_kick, S absent) where it fits
        out = D.split_kick(0, u, None, v, old_r, uk)
        if out is not None:
            return out
    q, rm = D.qr(_cat(u, uk, -1))
    return q, D.matmul(rm[:, :old_r], v), q.shape[1]


# ------------------------------------------------------------------ rounding (`:130-388`)
DEFL = 1e-3  # SVD deflation tolerance relative to a caller's truncation threshold


def prune_singular_vals(s, eps):
    """`cy_src/tt_ops_cy.pyx:161-177` -- host decision on the copied-back singular values."""
    if np.linalg.norm(s) == 0.0:
        return 1
    sc = np.cumsum(np.abs(s[::-1]) ** 2)[::-1]
    r = int(np.argmax(sc < eps ** 2))
    r = max(r, 1)
    if sc[-1] > eps ** 2:
        r = s.size
    return r


def _mat(t, rows):
    t = D.contig(t)
    return t.view(rows, -1)


def tt_rl_orthogonalise(tt):
    """`cy_src/tt_ops_cy.pyx:132-159` (in place, i = d-1 .. 1)."""
    d = len(tt)
    if d == 1:
        return tt
    for i in range(d - 1, 0, -1):
        si = tt[i].shape
        sm = tt[i - 1].shape
        Q, R = D.qr(D.contig(_mat(tt[i], si[0]).t()))
        nr = R.shape[0]
        tt[i] = D.clone(Q.t()).view(nr, *si[1:])
        lead = sm[:len(si) - 1]
        prev = D.contig(tt[i - 1]).view(int(np.prod(lead)), si[0])
        tt[i - 1] = D.einsum("ij,kj->ik", prev, R).view(*lead, nr)
    return tt


def tt_rl_orthogonalise_py(tt):
    """`src/tt_ops.py:30-42`: variant that also runs i = 0 (R moves into the LAST core)."""
    d = len(tt)
    if d == 1:
        return tt
    for i in range(d - 1, -1, -1):
        si = tt[i].shape
        sm = tt[i - 1].shape
        Q, R = D.qr(D.contig(_mat(tt[i], tt[i].shape[0]).t()))
        tt[i] = D.clone(Q.t()).view(-1, *si[1:-1], si[-1])
        prev = D.contig(tt[i - 1]).view(-1, R.shape[-1])
        tt[i - 1] = D.einsum("ij,kj->ik", prev, R).view(-1, *sm[1:-1], tt[i].shape[0])
    return tt


def _svd_step(tt, idx, rank, eps, track):
    ish = tt[idx].shape
    nsh = tt[idx + 1].shape
    mat = D.contig(tt[idx]).view(rank * int(np.prod(ish[1:-1])), -1)
    # deflation below 1e-3 x the truncation threshold cannot change the rank decision; the PSD /
    # mask variants (track) feed the discarded energy back, so they stay exact
    U, S, Vt, s = D.svd(mat, defl=0.0 if track else DEFL * eps)
    tail = 0.0
    if track:
        sc = np.cumsum(np.abs(s[::-1]) ** 2)[::-1]
        nr = int(np.argmax(sc < eps ** 2))
        nr = max(nr, 1)
        if sc[-1] > eps ** 2:
            nr = s.shape[0]
        if nr < s.shape[0]:
            tail = sc[nr]
    else:
        nr = prune_singular_vals(s, eps)
    tt[idx] = D.clone(U[:, :nr]).view(rank, *ish[1:-1], nr)
    nxt = D.contig(tt[idx + 1]).view(nsh[0], -1)
    tt[idx + 1] = D.einsum("r,rj,jk->rk", S[:nr], Vt[:nr], nxt).view(nr, *nsh[1:-1], -1)
    return nr, tail


NATIVE_ROUND = os.environ.get("TTIPM_NATIVE_ROUND", "1") == "1"


def _native_round(tt, eps, mode):
    """`ttk_round` (one library call per rounding, bit-identical to the Python sweep below).  The
    cores are copied first (the reference rebinds list entries and never writes the caller's
    arrays), the rounded cores are views of those copies.  Returns (tt, tail factor or None)."""
    d = len(tt)
    cs = D.clone_many(tt)
    mids = [tuple(c.shape[1:-1]) for c in tt]
    ptrs = (ctypes.c_void_p * d)(*[c.data_ptr() for c in cs])
    inner = (ctypes.c_int64 * d)(*[int(np.prod(m)) for m in mids])
    ranks = _rank_array(tt)
    tail = ctypes.c_double(0.0)
    D._stream()
    D.check(D.lib.ttk_round(D.ctx(), d, ptrs, inner, ranks, float(eps), mode, ctypes.byref(tail)), "round")
    out = [c.view(-1)[:ranks[k] * inner[k] * ranks[k + 1]].view(ranks[k], *mids[k], ranks[k + 1])
           for k, c in enumerate(cs)]
    tt[:] = out  # in place, like the reference's list mutation
    return tt, (None if np.isnan(tail.value) else tail.value)


ROUND_ONE = os.environ.get("TTIPM_ROUND_ONE", "0") == "1"


def _round_one_plan(tt):
    """(inner, ranks, bound) for `ttk_round_one` -- the ctypes extents of the train and the library's bound
    ranks -- or None when the train does not fit one workgroup's LDS."""
    d = len(tt)
    if d < 2:
        return None
    inner, ranks = _tt_extents(tt)
    bound = (ctypes.c_int64 * (d + 1))()
    if D.lib.ttk_round_one_lds(d, inner, ranks, bound) < 0:
        return None
    return inner, ranks, bound


def round_one_lds(tt):
    """Bytes of LDS `ttk_round_one` needs for this train, -1 if it does not fit one workgroup (`ttk_round`
    then runs)."""
    if len(tt) < 2:
        return -1
    return int(D.lib.ttk_round_one_lds(len(tt), *_tt_extents(tt), None))


def _round_one(tt, eps, mode, plan=None):
    """`ttk_round_one`: the QR sweep and the truncating Jacobi-SVD sweep in one launch of one workgroup, the
    ranks decided in the kernel, into one fresh buffer sized by the bound ranks (the output cores are views
    of its front parts).  One host read, after the launch: the d + 1 ranks and the tail.  The caller's
    tensors are never written and the list is rebound in place.  Returns (tt, tail factor or None)."""
    d = len(tt)
    inner, ranks, bound = plan or _round_one_plan(tt)
    assert list(bound) == retraction_ranks(inner, ranks, [1 << 62] * (d - 1)), list(bound)
    outs = _packed_flat(list(bound), inner)
    keep = [D.contig(c) for c in tt]  # the contiguous inputs stay alive until the call is enqueued
    P = ctypes.c_void_p * d
    info = D.empty(d + 2)
    D._stream()
    D.check(D.lib.ttk_round_one(D.ctx(), d, P(*[c.data_ptr() for c in keep]), inner, ranks, float(eps), mode,
                                P(*[o.data_ptr() for o in outs]), info.data_ptr()), "round_one")
    tt[:], factor = _round_one_finish(outs, D.read(info), inner, [c.shape[1:-1] for c in tt], mode, d)
    return tt, factor


def tt_rank_reduce(tt, eps=1e-18):
    """`cy_src/tt_ops_cy.pyx:179-226`: QR sweep + left-to-right truncated-SVD sweep.  With TTIPM_ROUND_ONE=1,
    on the GPU and for a train that fits (`round_one_lds`): one launch and one host read (`ttk_round_one`),
    the same tensor in another gauge.  Off by default: the whole-solve goldens are pinned to the current
    path's arithmetic."""
    d = len(tt)
    rk = [1] + tt_ranks(tt) + [1]
    if d == 1 or all(r == 1 for r in rk):
        return tt
    if ROUND_ONE and D.DEV.type == "cuda":
        plan = _round_one_plan(tt)
        if plan is not None:
            return _round_one(tt, eps, 0, plan)[0]
    if NATIVE_ROUND and D.DEV.type == "cuda":
        return _native_round(tt, eps, 0)[0]
    eps = eps / np.sqrt(d - 1)
    tt = tt_rl_orthogonalise(tt)
    rank = 1
    for idx in range(d - 1):
        rank, _ = _svd_step(tt, idx, rank, eps, False)
    return tt


def _tail_rank_reduce(tt, eps):
    d = len(tt)
    rk = [1] + tt_ranks(tt) + [1]
    if d == 1 or all(r == 1 for r in rk):
        return tt, None
    if ROUND_ONE and D.DEV.type == "cuda":
        plan = _round_one_plan(tt)
        if plan is not None:
            return _round_one(tt, eps, 1, plan)
    if NATIVE_ROUND and D.DEV.type == "cuda":
        return _native_round(tt, eps, 1)
    eps = eps / 2.0
    eps = eps / np.sqrt(d - 1)
    tt = tt_rl_orthogonalise(tt)
    rank = 1
    tail = 0.0
    for idx in range(d - 1):
        rank, t = _svd_step(tt, idx, rank, eps, True)
        tail += t
    return tt, pow(tail, 1.0 / (2 * d))


def _psd_correct(tt, factor):
    """the tracked rounding's correction, `factor` x I added (`cy_src/tt_ops_cy.pyx:311-325`)"""
    if factor is None:
        return tt
    n = tt[0].shape[1]
    eye = D.from_numpy(factor * np.eye(n).reshape(1, *tt[0].shape[1:-1], 1))
    return tt_add(tt, [eye] * len(tt))


def _mask_correct(tt, mask, factor):
    """the tracked rounding's correction, `factor` x mask added (`cy_src/tt_ops_cy.pyx:376-388`)"""
    if factor is None:
        return tt
    return tt_add(tt, [D.scaled(c, factor) for c in mask])


def tt_psd_rank_reduce(tt, eps=1e-18):
    """`cy_src/tt_ops_cy.pyx:261-325`"""
    return _psd_correct(*_tail_rank_reduce(tt, eps))


def tt_mask_rank_reduce(tt, mask, eps=1e-18):
    """`cy_src/tt_ops_cy.pyx:328-388`"""
    tt, factor = _tail_rank_reduce(tt, eps)
    return _mask_correct(tt, mask, factor)


# ------------------------------------------------------------------ rounding a weighted sum of trains
# round(sum_j c_j op_j(T_j)), op_j the identity or `tt_transpose`: the operand of the solve's
# `tt_rank_reduce(tt_add(a, tt_scale(alpha, b)))`, `tt_sub`, `tt_sum` and `_tt_symmetrise`
# (`src/tt_ops.py:321-328`, `src/tt_ipm.py:477-485`, `:612-640`).  These functions draw nothing from the
# random stream and take each weight as given: a caller that mirrors `tt_scale` passes
# float(np.float32(alpha)).
SUM_ROUND_ONE = os.environ.get("TTIPM_SUM_ROUND_ONE", "0") == "1"
SUM_TERMS = 4  # terms `ttk_sum_round_one` takes


def _sum_norm(trains, coeffs, transposed):
    n = len(trains)
    coeffs = [1.0] * n if coeffs is None else [float(c) for c in coeffs]
    transposed = [False] * n if transposed is None else [bool(t) for t in transposed]
    assert n >= 1 and len(coeffs) == n and len(transposed) == n and all(len(t) == len(trains[0]) for t in trains)
    assert all(c.dim() == 4 for t, tr in zip(trains, transposed) if tr for c in t), "a transposed term has matrix cores"
    return coeffs, transposed


def _sum_composed(trains, coeffs, transposed):
    """The sum as a train of its own: `tt_transpose` where asked, core 0 times the weight (`D.scaled`, skipped
    for a weight of 1), `tt_add` folded left to right.  A fresh list; a single unscaled term keeps its cores."""
    terms = []
    for t, c, tr in zip(trains, coeffs, transposed):
        t = tt_transpose(t) if tr else list(t)
        if c != 1.0:
            t[0] = D.scaled(t[0], c)
        terms.append(t)
    return reduce(tt_add, terms)


def _sum_round_one_plan(trains, coeffs, transposed):
    """The arguments of `ttk_sum_round_one` for these terms -- (d, inner, rows, n, terms), the summed and the
    bound ranks, the sum's middle extents, and what keeps the tables alive -- or None when the sum does not
    fit one workgroup's LDS, has more than SUM_TERMS terms or a single core."""
    d, n = len(trains[0]), len(trains)
    if d < 2 or n > SUM_TERMS:
        return None
    mids = [tuple(c.shape[1:-1])[::-1] if transposed[0] else tuple(c.shape[1:-1]) for c in trains[0]]
    I64, P, vp = ctypes.c_int64, ctypes.c_void_p * d, ctypes.c_void_p
    inner = (I64 * d)(*[int(np.prod(m)) for m in mids])
    rows = (I64 * d)(*[int(m[0]) for m in mids]) if any(transposed) else None
    keep = [[D.contig(c) for c in t] for t in trains]  # the contiguous inputs stay alive until the call is enqueued
    ptrs = [P(*[c.data_ptr() for c in t]) for t in keep]
    ranks = [_rank_array(t) for t in trains]
    terms = (SumTerm * n)(*[SumTerm(ctypes.cast(p, vp), ctypes.cast(r, vp), c, int(tr))
                            for p, r, c, tr in zip(ptrs, ranks, coeffs, transposed)])
    sums, bound = (I64 * (d + 1))(), (I64 * (d + 1))()
    if D.lib.ttk_sum_round_one_lds(d, inner, n, terms, sums, bound) < 0:
        return None
    return (d, inner, rows, n, terms), list(sums), list(bound), mids, (keep, ptrs, ranks)


def sum_round_one_lds(trains, transposed=None):
    """Bytes of LDS `ttk_sum_round_one` needs for the sum of these trains (`transposed`: one flag per train),
    -1 if it does not fit one workgroup or has more than SUM_TERMS terms (the sum is then built and rounded)."""
    coeffs, transposed = _sum_norm(trains, None, transposed)
    plan = _sum_round_one_plan(trains, coeffs, transposed)
    if plan is None:
        return -1
    d, inner, _, n, terms = plan[0]
    return int(D.lib.ttk_sum_round_one_lds(d, inner, n, terms, None, None))


def _sum_round_one(plan, eps, mode):
    """`ttk_sum_round_one`: `_round_one` on the sum, whose cores exist only inside the kernel's two loads.  One
    launch into one fresh buffer sized by the bound ranks, one host read (the ranks and the tail).  Returns
    (tt, tail factor or None); the caller's tensors are never written."""
    (d, inner, rows, n, terms), sums, bound, mids, keep = plan
    assert bound == retraction_ranks(inner, sums, [1 << 62] * (d - 1)), bound
    outs = _packed_flat(bound, inner)
    P = ctypes.c_void_p * d
    info = D.empty(d + 2)
    D._stream()
    D.check(D.lib.ttk_sum_round_one(D.ctx(), d, inner, rows, n, terms, float(eps), mode,
                                    P(*[o.data_ptr() for o in outs]), info.data_ptr()), "sum_round_one")
    return _round_one_finish(outs, D.read(info), inner, mids, mode, d)


def _sum_native(trains, coeffs, transposed, eps, mode):
    """(tt, tail factor or None) from `ttk_sum_round_one`, or None where that path is not taken: the switch is
    off, there is no GPU, the sum does not fit, or the existing functions return the input as it is (d = 1, a
    single term with every rank 1)."""
    if not (SUM_ROUND_ONE and D.DEV.type == "cuda") or len(trains[0]) < 2:
        return None
    if len(trains) == 1 and all(r == 1 for r in tt_ranks(trains[0])):
        return None
    plan = _sum_round_one_plan(trains, coeffs, transposed)
    return None if plan is None else _sum_round_one(plan, eps, mode)


def tt_sum_rank_reduce(trains, coeffs=None, transposed=None, eps=1e-18):
    """`tt_rank_reduce` of sum_j coeffs[j] op_j(trains[j]), op_j = `tt_transpose` where transposed[j].  With
    TTIPM_SUM_ROUND_ONE=1, on the GPU, for at most SUM_TERMS terms whose sum fits (`sum_round_one_lds`): one
    launch and one host read (`ttk_sum_round_one`), the sum never built.  Otherwise the sum is built
    (`_sum_composed`) and rounded as today.  Off by default, like TTIPM_ROUND_ONE."""
    coeffs, transposed = _sum_norm(trains, coeffs, transposed)
    res = _sum_native(trains, coeffs, transposed, eps, 0)
    return res[0] if res is not None else tt_rank_reduce(_sum_composed(trains, coeffs, transposed), eps)


def _sum_tail_rank_reduce(trains, coeffs, transposed, eps):
    coeffs, transposed = _sum_norm(trains, coeffs, transposed)
    res = _sum_native(trains, coeffs, transposed, eps, 1)
    return res if res is not None else _tail_rank_reduce(_sum_composed(trains, coeffs, transposed), eps)


def tt_sum_psd_rank_reduce(trains, coeffs=None, transposed=None, eps=1e-18):
    """`tt_psd_rank_reduce` of the sum (see `tt_sum_rank_reduce`)"""
    return _psd_correct(*_sum_tail_rank_reduce(trains, coeffs, transposed, eps))


def tt_sum_mask_rank_reduce(trains, coeffs=None, transposed=None, mask=None, eps=1e-18):
    """`tt_mask_rank_reduce` of the sum (see `tt_sum_rank_reduce`)"""
    tt, factor = _sum_tail_rank_reduce(trains, coeffs, transposed, eps)
    return _mask_correct(tt, mask, factor)


def retraction_ranks(inner, ranks, upper):
    """Rank list [q_0, ..., q_d] that `tt_rank_retraction` gives a train with middle extents `inner` (d
    entries) and ranks `ranks` (d+1 entries, boundaries 1) under the bounds `upper` (d-1 entries): the QR
    sweep leaves rho_d = 1, rho_k = min(inner_k rho_{k+1}, ranks_k), and the SVD sweep keeps q_0 = 1,
    q_{i+1} = min(upper_i, q_i inner_i, rho_{i+1}) (`len(abs_S > 0)` is `len(S)`).  Host arithmetic only."""
    d = len(inner)
    rho = [1] * (d + 1)
    for k in range(d - 1, 0, -1):
        rho[k] = min(int(inner[k]) * rho[k + 1], int(ranks[k]))
    q = [1] * (d + 1)
    for i in range(d - 1):
        q[i + 1] = min(int(upper[i]), q[i] * int(inner[i]), rho[i + 1])
    return q


NATIVE_RETRACT = os.environ.get("TTIPM_NATIVE_RETRACT", "0") == "1"


def _inner(c):
    return int(np.prod(c.shape[1:-1])) if c.dim() > 2 else 1


def _rank_array(t):
    """ctypes int64 bond ranks of a train: d + 1 entries, boundaries included"""
    return (ctypes.c_int64 * (len(t) + 1))(*([t[0].shape[0]] + [c.shape[-1] for c in t]))


def _tt_extents(*trains):
    """ctypes int64 arrays for the native rounding calls: the middle extents of the first train (d entries),
    then one bond-rank array per train (`_rank_array`)."""
    inner = (ctypes.c_int64 * len(trains[0]))(*[_inner(c) for c in trains[0]])
    return (inner,) + tuple(_rank_array(t) for t in trains)


def _packed(sizes):
    """One fresh buffer cut into flat slices of these sizes, every one at a 16-byte aligned offset."""
    offs = np.concatenate(([0], np.cumsum([(s + 1) & ~1 for s in sizes])))
    buf = D.empty(int(offs[-1]))
    return [buf[int(o):int(o) + s] for o, s in zip(offs, sizes)]


def _packed_flat(rk, inner):
    """One fresh buffer for the output cores of ranks `rk` and middle extents `inner`: its flat slices, one per
    core (what a native call writes)."""
    return _packed([rk[k] * inner[k] * rk[k + 1] for k in range(len(inner))])


def _round_one_finish(outs, got, inner, mids, mode, d):
    """What a one-launch rounding left behind, as the caller's result.  outs: the flat buffers it wrote, sized by
    the bound ranks; got: its info words as read -- the d + 1 decided ranks, the discarded tail and, where the entry
    has it (d + 3 words), the squared norm; mids: the middle shape of every core.  Returns (tt, tail factor or None)
    with the cores views of the written fronts, and the squared norm as a third entry where `got` holds one."""
    q = [int(v) for v in got[:d + 1]]
    tt = [o[:q[k] * inner[k] * q[k + 1]].view(q[k], *mids[k], q[k + 1]) for k, o in enumerate(outs)]
    res = tt, (pow(float(got[d + 1]), 1.0 / (2 * d)) if mode else None)
    return res + (float(got[d + 2]),) if len(got) > d + 2 else res


def _packed_out(tt, rk, inner):
    """`_packed_flat`'s slices and their views (rk[k], *middle extents of tt[k], rk[k+1])."""
    outs = _packed_flat(rk, inner)
    return outs, [o.view(rk[k], *tt[k].shape[1:-1], rk[k + 1]) for k, o in enumerate(outs)]


def _native_rounding(name, tt, rk, inner, args):
    """Calls `ttk_<name>(ctx, d, *args, out, out_ranks)` into a `_packed_out` buffer and returns the output
    cores.  In `args` a list of tensors stands for the array of their (contiguous) device pointers.  No
    host read: the ranks `rk` are host arithmetic, and the library's own rule must agree with them."""
    d = len(tt)
    P = ctypes.c_void_p * d
    outs, views = _packed_out(tt, rk, inner)
    keep, call = [], []  # keep: the contiguous inputs stay alive until the call is enqueued
    for a in args:
        if isinstance(a, list):
            keep.append([D.contig(c) for c in a])
            a = P(*[c.data_ptr() for c in keep[-1]])
        call.append(a)
    got = (ctypes.c_int64 * (d + 1))()
    D._stream()
    D.check(getattr(D.lib, "ttk_" + name)(D.ctx(), d, *call, P(*[o.data_ptr() for o in outs]), got), name)
    assert list(got) == rk, (list(got), rk)
    return views


def _retract_args(tt, upper):
    return _tt_extents(tt) + ((ctypes.c_int64 * max(len(tt) - 1, 1))(*[int(u) for u in upper]),)


def retract_lds(tt, upper):
    """Bytes of LDS `ttk_retract` needs for this train under the bounds `upper` (d-1 entries), -1 if it
    does not fit one workgroup (the composed path then runs)."""
    if len(tt) < 2 or len(upper) != len(tt) - 1:
        return -1
    return int(D.lib.ttk_retract_lds(len(tt), *_retract_args(tt, upper)))


def _retract_native(tt, args):
    """`ttk_retract`: the QR sweep and the Jacobi-SVD sweep in one launch of one workgroup, into one
    fresh buffer (the output cores are views of it).  No host read: the ranks come from
    `retraction_ranks`.  `args`: `_retract_args`."""
    inner, ranks, ub = args
    return _native_rounding("retract", tt, retraction_ranks(inner, ranks, ub), inner, (list(tt), inner, ranks, ub))


def tt_rank_retraction(tt, upper_ranks):
    """`src/tt_ops.py:132-152` (argpartition top-k on the host singular values).  With
    TTIPM_NATIVE_RETRACT=1, on the GPU, with one bound per interior bond and a train that fits
    (`retract_lds`): one launch without a host read (`ttk_retract`), the same tensor in another gauge;
    the caller's tensors are never written and the list is rebound in place.  Off by default: the
    whole-solve goldens are pinned to the composed path's arithmetic."""
    if NATIVE_RETRACT and D.DEV.type == "cuda" and len(tt) > 1 and len(upper_ranks) == len(tt) - 1:
        args = _retract_args(tt, upper_ranks)  # built once for the fit check and the call
        if D.lib.ttk_retract_lds(len(tt), *args) >= 0:
            tt[:] = _retract_native(tt, args)
            return tt
    tt = tt_rl_orthogonalise_py(tt)
    rank = 1
    for idx, up in enumerate(upper_ranks):
        ish = tt[idx].shape
        nsh = tt[idx + 1].shape
        U, S, Vt, s = D.svd(D.contig(tt[idx]).view(rank * int(np.prod(ish[1:-1])), -1))
        a = np.abs(s)
        nr = min(up, len(a > 0))
        sel = np.argpartition(a, -nr)[-nr:]
        if np.array_equal(sel, np.arange(nr)):
            Us, Ss, Vs = U[:, :nr], S[:nr], Vt[:nr]
        else:  # unsorted top-k: gather the selected singular triplets with a 0/1 contraction
            Pn = np.zeros((len(s), nr))
            Pn[sel, np.arange(nr)] = 1.0
            P = D.from_numpy(Pn)
            Us = D.matmul(U, P)
            Ss = D.einsum("i,ij->j", S, P)
            Vs = D.einsum("ij,ik->jk", P, Vt)
        tt[idx] = D.contig(Us).view(rank, *ish[1:-1], nr)
        nxt = D.contig(tt[idx + 1]).view(Vs.shape[-1], -1)
        tt[idx + 1] = D.einsum("r,rj,jk->rk", Ss, Vs, nxt).view(nr, *nsh[1:-1], -1)
        rank = nr
    return tt


# ------------------------------------------------------------------ randomised rounding (`src/tt_ops.py:51-101`)
def tt_rl_contraction(a, b):
    """`src/tt_ops.py:51-58`: the d-1 partial contractions of two trains from the right, W_k of shape
    (ra_k, rb_k) for the bonds k = 1..d-1: W_{d-1} = A_{d-1} B_{d-1}^T on the (r, inner) unfoldings, then
    W_k = unfold(A_k W_{k+1}) unfold(B_k)^T."""
    ra, rb = a[-1].shape[0], b[-1].shape[0]
    out = [D.einsum("ik,jk->ij", D.contig(a[-1]).view(ra, -1), D.contig(b[-1]).view(rb, -1))]
    for ca, cb in zip(a[-2:0:-1], b[-2:0:-1]):
        w = out[-1]
        z = D.matmul(D.contig(ca).view(-1, w.shape[0]), w)
        out.append(D.einsum("ik,jk->ij", z.view(ca.shape[0], -1), D.contig(cb).view(cb.shape[0], -1)))
    return out[::-1]


def tt_lr_contraction(a, b):
    """`src/tt_ops.py:61-65`: `tt_rl_contraction` of the mirrored trains."""
    return tt_swap_all(tt_rl_contraction(tt_swap_all(a), tt_swap_all(b)))


def randorth_ranks(r0, inner, sketch_ranks):
    """Bond ranks [r'_0, ..., r'_{d-1}] that `_tt_lr_random_orthogonalise` gives a train with leading
    rank r0 and middle extents `inner` (d entries) under a sketch with bond ranks `sketch_ranks` (d-1
    entries): r'_0 = r0, r'_{i+1} = min(r'_i * inner_i, l_{i+1}) -- the column count of the economic QR
    of the (r'_i inner_i, l_{i+1}) sketched unfolding.  Host arithmetic only; a rank grows where the
    target exceeds it."""
    out = [int(r0)]
    for n, l in zip(inner, sketch_ranks):
        out.append(min(out[-1] * int(n), int(l)))
    return out


NATIVE_RANDORTH = os.environ.get("TTIPM_NATIVE_RANDORTH", "1") == "1"


def _randorth_composed(tt, gs):
    """The sweep from D.einsum / D.matmul / D.qr (3 launches and a QR per bond); also what a train too
    large for `ttk_rand_orth` takes."""
    d = len(tt)
    W = tt_rl_contraction(tt, gs)
    rk = randorth_ranks(tt[0].shape[0], [_inner(c) for c in tt[:-1]], [w.shape[1] for w in W])
    out = [None] * d
    cur = D.contig(tt[0])
    for i, w in enumerate(W):
        nsh = tt[i + 1].shape
        Z = cur.view(-1, nsh[0])
        Q, _ = D.qr(D.matmul(Z, w))
        assert Q.shape[1] == rk[i + 1], (Q.shape, rk)
        out[i] = Q.view(rk[i], *tt[i].shape[1:-1], rk[i + 1])
        M = D.einsum("ki,kj->ij", Q, Z)
        cur = D.matmul(M, D.contig(tt[i + 1]).view(nsh[0], -1)).view(rk[i + 1], *nsh[1:])
    out[d - 1] = cur
    return out


def randorth_lds(tt, gs):
    """Bytes of LDS `ttk_rand_orth` needs for this train and sketch, -1 if they do not fit one
    workgroup (the composed path then runs)."""
    return int(D.lib.ttk_rand_orth_lds(len(tt), *_tt_extents(tt, gs)))


def _randorth_native(tt, gs, args):
    """`ttk_rand_orth`: the whole sweep in one launch of one workgroup, into one fresh buffer (the
    output cores are views of it).  No host read: the ranks come from `randorth_ranks`.  `args`:
    `_tt_extents(tt, gs)`."""
    d = len(tt)
    inner, ranks, sranks = args
    rk = randorth_ranks(ranks[0], inner[:d - 1], sranks[1:d]) + [ranks[d]]
    return _native_rounding("rand_orth", tt, rk, inner, (list(tt), inner, ranks, list(gs), sranks))


def _tt_lr_random_orthogonalise(tt, gs):
    """`src/tt_ops.py:89-101`: with W = tt_rl_contraction(tt, gs), for i = 0..d-2: Z = core i as
    (r_i n_i, R_{i+1}), Q = economic QR of Z W_{i+1}, core i <- Q, core i+1 <- (Q^T Z) core i+1.  The
    output ranks are `randorth_ranks` (fixed by the sketch's ranks, no truncation decision), every core
    but the last has an orthonormal left unfolding.  With the sketch in hand the sweep reads nothing
    back to the host (the host read of `tt_lr_random_orthogonalise` is `tt_random_gaussian`'s
    normalisation).  The caller's tensors are never written; the list is rebound in place, like the
    reference's list mutation.  One launch (`ttk_rand_orth`) when the train fits one workgroup's LDS,
    else composed from einsum / QR launches (TTIPM_NATIVE_RANDORTH=0: always composed)."""
    if len(tt) < 2:
        return tt
    out = None
    if NATIVE_RANDORTH and D.DEV.type == "cuda" and hasattr(D.lib, "ttk_rand_orth"):
        args = _tt_extents(tt, gs)  # built once for the fit check and the call
        if D.lib.ttk_rand_orth_lds(len(tt), *args) >= 0:
            out = _randorth_native(tt, gs, args)
    tt[:] = out if out is not None else _randorth_composed(tt, gs)
    return tt


def _tt_rl_random_orthogonalise(tt, gs):
    """`src/tt_ops.py:83-86`: the mirrored sweep (right unfoldings orthonormal, ranks fixed from the
    right), through `tt_swap_all`."""
    if len(tt) < 2:
        return tt
    out = tt_swap_all(_tt_lr_random_orthogonalise(tt_swap_all(tt), tt_swap_all(gs)))
    tt[:] = out
    return tt


def tt_lr_random_orthogonalise(tt, target_ranks):
    """`src/tt_ops.py:68-72`: rounding to the given bond ranks with a fresh Gaussian sketch
    (`tt_random_gaussian`: host MT19937 draws and one host read for its normalisation)."""
    if len(tt) > 1:
        gs = tt_random_gaussian(target_ranks, shape=tuple(tt[0].shape[1:-1]))
        return _tt_lr_random_orthogonalise(tt, gs)
    return tt


def tt_rl_random_orthogonalise(tt, target_ranks):
    """`src/tt_ops.py:75-80`: as above from the right; the sketch is drawn left to right and mirrored."""
    if len(tt) > 1:
        gs = tt_swap_all(tt_random_gaussian(target_ranks, shape=tuple(tt[0].shape[1:-1])))
        out = tt_swap_all(_tt_lr_random_orthogonalise(tt_swap_all(tt), gs))
        tt[:] = out
        return tt
    return tt


# ------------------------------------------------------------------ generalised Nystroem rounding (`src/tt_ops.py:232-300`)
def tt_sketch(shape, target_ranks):
    """`src/tt_ops.py:240-244`: unnormalised scaled Gaussian cores (l_k, *shape, l_{k+1}) for the full
    rank list `target_ranks` (boundaries included); host MT19937 draws, uploaded, no host read."""
    return [D.from_numpy(np.divide(1, a * np.prod(shape) * b) * _rng.R().randn(a, *shape, b))
            for a, b in zip(target_ranks[:-1], target_ranks[1:])]


def tt_sketch_like(tt, target_ranks):
    """`src/tt_ops.py:232-237`: `tt_sketch` with core i's middle extents taken from `tt[i]`."""
    return [D.from_numpy(np.divide(1, a * np.prod(tt[i].shape[1:-1]) * b) * _rng.R().randn(a, *tt[i].shape[1:-1], b))
            for i, (a, b) in enumerate(zip(target_ranks[:-1], target_ranks[1:]))]


def nystroem_ranks(ranks, lranks, rranks):
    """Rank list [r'_0, ..., r'_d] that `_tt_generalised_nystroem` gives a train with ranks `ranks` under
    sketches with ranks `lranks` (left) and `rranks` (right), all d+1 entries with the boundaries: the
    boundary ranks stay, an interior bond gets min(l_k, s_k), the length of S in the thin SVD of the
    (l_k, s_k) matrix W_L W_R.  Host arithmetic only."""
    d = len(ranks) - 1
    return [int(ranks[0])] + [min(int(a), int(b)) for a, b in zip(lranks[1:d], rranks[1:d])] + [int(ranks[d])]


NATIVE_NYSTROEM = os.environ.get("TTIPM_NATIVE_NYSTROEM", "1") == "1"


def _nystroem_composed(tt, g1, g2):
    """The rounding from D.einsum / D.matmul / D.svd: per bond a product, an SVD whose S is read on the
    host, and the two factors; then one or two products per core.  Also what a train too large for
    `ttk_nystroem` takes."""
    d = len(tt)
    Ls, Rs = [], []
    for wl, wr in zip(tt_lr_contraction(tt, g1), tt_rl_contraction(tt, g2)):
        U, _, Vt, s = D.svd(D.matmul(wl, wr))
        with np.errstate(divide="ignore", invalid="ignore"):  # like the reference: no guard on S = 0
            root_s_inv = D.from_numpy(np.diag(np.divide(1, np.sqrt(s))))
        Ls.append(D.matmul(D.einsum("ik,jk->ij", wr, Vt), root_s_inv))
        Rs.append(D.matmul(root_s_inv, D.einsum("ki,kj->ij", U, wl)))
    out = []
    for i, c in enumerate(tt):
        sh = c.shape
        x = D.contig(c)
        if i < d - 1:
            x = D.matmul(x.view(-1, sh[-1]), Ls[i])
        if i > 0:
            x = D.matmul(Rs[i - 1], x.view(sh[0], -1))
        out.append(x.view(sh[0] if i == 0 else Rs[i - 1].shape[0], *sh[1:-1], sh[-1] if i == d - 1 else Ls[i].shape[1]))
    return out


def nystroem_lds(tt, g1, g2):
    """The largest dynamic-LDS request (bytes) of `ttk_nystroem`'s launches for this train and these
    sketches, -1 if some core does not fit one workgroup (the composed path then runs)."""
    return int(D.lib.ttk_nystroem_lds(len(tt), *_tt_extents(tt, g1, g2)))


def _nystroem_native(tt, g1, g2, args):
    """`ttk_nystroem`: three launches of independent workgroups into one fresh buffer (the output cores
    are views of it).  No host read: the ranks come from `nystroem_ranks`.  `args`: `_tt_extents(tt, g1, g2)`."""
    inner, ranks, lranks, rranks = args
    return _native_rounding("nystroem", tt, nystroem_ranks(ranks, lranks, rranks), inner,
                            (list(tt), inner, ranks, list(g1), lranks, list(g2), rranks))


def _tt_generalised_nystroem(tt, g1, g2):
    """`src/tt_ops.py:273-292`: with W_L = tt_lr_contraction(tt, g1) and W_R = tt_rl_contraction(tt, g2),
    per bond P = W_L W_R = U diag(S) V^T (thin), L = W_R V diag(1/sqrt(S)), R = diag(1/sqrt(S)) U^T W_L;
    core i <- R_i core_i L_{i+1} (no R on the first core, no L on the last).  The output ranks are
    `nystroem_ranks` (fixed by the sketches' ranks, no truncation decision); like the reference, a zero
    singular value is not guarded.  The caller's tensors are never written; the list is rebound in
    place, like the reference's list mutation.  Three launches without a host read (`ttk_nystroem`)
    when every core fits one workgroup's LDS, else composed from einsum / SVD calls with S read on
    the host (TTIPM_NATIVE_NYSTROEM=0: always composed)."""
    if len(tt) < 2:
        return tt
    out = None
    if NATIVE_NYSTROEM and D.DEV.type == "cuda" and hasattr(D.lib, "ttk_nystroem"):
        args = _tt_extents(tt, g1, g2)  # built once for the fit check and the call
        if D.lib.ttk_nystroem_lds(len(tt), *args) >= 0:
            out = _nystroem_native(tt, g1, g2, args)
    tt[:] = out if out is not None else _nystroem_composed(tt, g1, g2)
    return tt


def tt_generalised_nystroem(tt, target_ranks):
    """`src/tt_ops.py:295-300`: rounding to the given bond ranks with two fresh Gaussian sketches, the
    left one with `target_ranks` and then the right one with every rank one larger
    (`tt_random_gaussian`: host MT19937 draws and one host read each for the normalisation)."""
    if len(tt) > 1:
        shape = tuple(tt[0].shape[1:-1])
        g1 = tt_random_gaussian(target_ranks, shape=shape)
        g2 = tt_random_gaussian([r + 1 for r in target_ranks], shape=shape)
        return _tt_generalised_nystroem(tt, g1, g2)
    return tt


# ------------------------------------------------------------------ zip-up products (`:391-502`)
def swap_cores(a, b, eps):
    """`cy_src/tt_ops_cy.pyx:393-426`"""
    if a.dim() == 3:
        m = D.einsum("ijr,rkl->ikjl", a, b).view(a.shape[0] * b.shape[1], -1)
        U, S, Vt, s = D.svd(m, defl=DEFL * eps)
        r = prune_singular_vals(s, eps)
        na = D.einsum("ij,j->ij", U[:, :r], S[:r]).view(a.shape[0], b.shape[1], r)
        nb = D.clone(Vt[:r]).view(r, a.shape[1], b.shape[2])
        return na, nb
    m = D.einsum("ijkr,rlmn->ilmjkn", a, b).view(a.shape[0] * b.shape[1] * b.shape[2], -1)
    U, S, Vt, s = D.svd(m, defl=DEFL * eps)
    r = prune_singular_vals(s, eps)
    na = D.einsum("ij,j->ij", U[:, :r], S[:r]).view(a.shape[0], b.shape[1], b.shape[2], r)
    nb = D.clone(Vt[:r]).view(r, a.shape[1], a.shape[2], b.shape[3])
    return na, nb


def _bubble(cores, i, eps):
    for j in range(i, -1, -1):
        cores[j], cores[j + 1] = swap_cores(cores[j], cores[j + 1], eps)


def _zipup_matrix_vec_mul(mat, vec, eps=1e-18):
    """`cy_src/tt_ops_cy.pyx:428-447` as written (bubble zip-up); kept for the parity tests."""
    d = len(mat)
    leps = eps / np.sqrt(d - 1) if d > 1 else eps
    cores = [c.permute(2, 1, 0) for c in reversed(vec)]
    for i in range(d):
        cores[0] = D.einsum("amnA,Anr->amr", mat[d - i - 1], cores[0])
        if i != d - 1:
            _bubble(cores, i, leps)
    return cores


def _zipup_mat_mat_mul(m1, m2, eps=1e-18):
    """`cy_src/tt_ops_cy.pyx:449-464` as written (bubble zip-up); kept for the parity tests."""
    d = len(m1)
    leps = eps / np.sqrt(d - 1) if d > 1 else eps
    cores = [c.permute(3, 1, 2, 0) for c in reversed(m2)]
    for i in range(d):
        cores[0] = D.einsum("amkA,Aknr->amnr", m1[d - i - 1], cores[0])
        if i != d - 1:
            _bubble(cores, i, leps)
    return cores


def _zipup_hadamard(t1, t2, eps=1e-18):
    """`cy_src/tt_ops_cy.pyx:466-502` as written (bubble zip-up); kept for the parity tests."""
    d = len(t1)
    leps = eps / np.sqrt(d - 1) if d > 1 else eps
    if t1[0].dim() == 4 and t2[0].dim() == 4:
        cores = [c.permute(3, 1, 2, 0) for c in reversed(t2)]
        for i in range(d):
            cores[0] = D.einsum("aijA,Aijb->aijb", t1[d - i - 1], cores[0])
            if i != d - 1:
                _bubble(cores, i, leps)
        return cores
    cores = [c.permute(2, 1, 0) for c in reversed(t2)]
    for i in range(d):
        cores[0] = D.einsum("aiA,Aib->aib", t1[d - i - 1], cores[0])
        if i != d - 1:
            _bubble(cores, i, leps)
    return cores


# The reference's zip-up products contract each operator core into the reversed operand and
# bubble it through the processed cores with a truncated SVD per swap (eps/sqrt(d-1), absolute),
# i.e. d(d-1)/2 SVDs whose unfoldings live in a mode-permuted order: at maxcut_10 the bonds of
# those intermediates reach ~220 (888 x 1024 swap matrices) even though the product itself has
# rank <= rank_A * rank_x.  The device path computes the same product -- the exact core-wise
# (Kronecker-bond) contraction, truncated to the same absolute accuracy by one TT rounding at eps
# (QR sweep + d-1 truncated SVDs, `tt_rank_reduce`) -- so the represented tensor agrees with the
# zip-up's to within the eps both truncate at, without the mode-swapped intermediates.  The
# output ranks are the product's numerical ranks at eps (the zip-up's can only be larger, its
# per-swap truncation is not optimal); every hot call site rounds the result again
# (`tt_mat_vec_mul`, `tt_mat_mat_mul`, the residual / Y-update / centrality chains).
# TTIPM_ZIPUP=1 restores the bubble zip-up everywhere (parity experiments).
ZIPUP = os.environ.get("TTIPM_ZIPUP") == "1"


def _kron_round(cores, eps):
    if len(cores) > 1 and eps > 0:
        return tt_rank_reduce(cores, eps)
    return cores


NATIVE_ZIPUP = os.environ.get("TTIPM_NATIVE_ZIPUP", "1") == "1"


def _zipup_modes(kind, a, b):
    """`ttk_zipup`'s modes: three physical extents per core, 1 where the kind has none"""
    mids = []
    for x, y in zip(a, b):
        if kind == 0:
            mids += [x.shape[1], x.shape[2], 1]
        elif kind == 1:
            mids += [x.shape[1], x.shape[2], y.shape[2]]
        elif kind == 2:
            mids += [x.shape[1], 1, 1]
        else:
            mids += [x.shape[1], x.shape[2], 1]
    return mids


def _native_zipup(kind, a, b, eps, out_modes):
    """`ttk_zipup` (one library call: the core-wise products into fresh buffers + one in-place
    rounding; the same einsum plans and rounding launches as the Python composition below, so
    bit-identical to it).  out_modes[k]: the product core's physical shape."""
    d = len(a)
    ar, br = _rank_array(a), _rank_array(b)
    mids = _zipup_modes(kind, a, b)
    inner = [int(np.prod(m)) for m in out_modes]
    outs = [D.empty(ar[k] * br[k] * inner[k] * ar[k + 1] * br[k + 1]) for k in range(d)]
    ca = [D.contig(c) for c in a]
    cb = [D.contig(c) for c in b]
    P = ctypes.c_void_p
    I64 = ctypes.c_int64
    ranks = (I64 * (d + 1))()
    D._stream()
    D.check(D.lib.ttk_zipup(D.ctx(), kind, d, (P * d)(*[c.data_ptr() for c in ca]), ar,
                            (P * d)(*[c.data_ptr() for c in cb]), br, (I64 * (3 * d))(*mids),
                            float(eps), (P * d)(*[o.data_ptr() for o in outs]), ranks), "zipup")
    return [o[:ranks[k] * inner[k] * ranks[k + 1]].view(ranks[k], *out_modes[k], ranks[k + 1])
            for k, o in enumerate(outs)]


def _use_native_zipup():
    return NATIVE_ZIPUP and NATIVE_ROUND and D.DEV.type == "cuda"


# ------------------------------------------------------------------ rounding a product of two trains
# The products above write d Kronecker-bond cores and round them with 2(d-1) factorisation launches and one
# host read per bond.  `ttk_prod_round_one` forms the product core inside the one-launch rounding's two loads
# (kind and modes are `ttk_zipup`'s): one launch, one host read, the product never in global memory.  Off by
# default, like TTIPM_ROUND_ONE and TTIPM_SUM_ROUND_ONE.  Nothing here draws from the random stream.
PROD_ROUND_ONE = os.environ.get("TTIPM_PROD_ROUND_ONE", "0") == "1"


def _prod_out_modes(kind, a, b):
    """the middle shape of every product core"""
    if kind == 0:
        return [(x.shape[1],) for x in a]
    if kind == 1:
        return [(x.shape[1], y.shape[2]) for x, y in zip(a, b)]
    return [tuple(x.shape[1:-1]) for x in a]


def _prod_round_one_plan(kind, a, b):
    """The arguments of `ttk_prod_round_one` for a (x), (.) or (o) b -- (kind, d, a, a_ranks, b, b_ranks, modes),
    the product and the bound ranks, the product's middle extents, and what keeps the tables alive -- or None
    when the product does not fit one workgroup's LDS or has a single core."""
    d = len(a)
    if d < 2 or len(b) != d:
        return None
    I64, P = ctypes.c_int64, ctypes.c_void_p * d
    ar, br = _rank_array(a), _rank_array(b)
    modes = (I64 * (3 * d))(*_zipup_modes(kind, a, b))
    prod, bound = (I64 * (d + 1))(), (I64 * (d + 1))()
    if D.lib.ttk_prod_round_one_lds(kind, d, ar, br, modes, prod, bound) < 0:
        return None
    keep = ([D.contig(c) for c in a], [D.contig(c) for c in b])  # alive until the call is enqueued
    pa, pb = (P(*[c.data_ptr() for c in t]) for t in keep)
    return (kind, d, pa, ar, pb, br, modes), list(prod), list(bound), (keep, pa, pb)


def prod_round_one_lds(kind, a, b):
    """Bytes of LDS `ttk_prod_round_one` needs for the product of these trains (kind: `ttk_zipup`'s, 0 matrix x
    vector, 1 matrix x matrix, 2 / 3 Hadamard of vector / matrix trains), -1 if it does not fit one workgroup
    (`ttk_zipup` then runs)."""
    plan = _prod_round_one_plan(kind, a, b)
    if plan is None:
        return -1
    kind, d, _, ar, _, br, modes = plan[0]
    return int(D.lib.ttk_prod_round_one_lds(kind, d, ar, br, modes, None, None))


def _prod_round_one(plan, out_modes, eps, mode):
    """`ttk_prod_round_one`: `_round_one` on the product, whose cores exist only inside the kernel's two loads.
    One launch into one fresh buffer sized by the bound ranks, one host read (the ranks and the tail).  Returns
    (tt, tail factor or None); the caller's tensors are never written."""
    (kind, d, pa, ar, pb, br, modes), prod, bound, keep = plan
    inner = [int(np.prod(m)) for m in out_modes]
    assert bound == retraction_ranks(inner, prod, [1 << 62] * (d - 1)), bound
    outs = _packed_flat(bound, inner)
    info = D.empty(d + 2)
    D._stream()
    D.check(D.lib.ttk_prod_round_one(D.ctx(), kind, d, pa, ar, pb, br, modes, float(eps), mode,
                                     (ctypes.c_void_p * d)(*[o.data_ptr() for o in outs]), info.data_ptr()),
            "prod_round_one")
    return _round_one_finish(outs, D.read(info), inner, out_modes, mode, d)


def _prod_native(kind, a, b, eps):
    """The rounded product from `ttk_prod_round_one`, or None where that path is not taken: the switch is off,
    there is no GPU, eps <= 0 or d = 1 (the product is returned unrounded), every product rank is 1 (nothing
    to round), or the product does not fit."""
    if not (PROD_ROUND_ONE and D.DEV.type == "cuda") or len(a) < 2 or not eps > 0:
        return None
    if all(x.shape[-1] * y.shape[-1] == 1 for x, y in zip(a[:-1], b[:-1])):
        return None
    plan = _prod_round_one_plan(kind, a, b)
    return None if plan is None else _prod_round_one(plan, _prod_out_modes(kind, a, b), eps, 0)[0]


# ------------------------------------------------------------------ rounding a sum of trains and products
# round(sum_j c_j op_j(T_j)), T_j a train or the core-wise product of two (kind: `ttk_zipup`'s), op_j the identity
# or the swap of the two middle indices: the solve's residuals L vec(X) - b and Ladj Y - Z - C, its Y update and
# bv mask + mask o X.  `ttk_affine_round_one` forms every term inside the one-launch rounding's two loads and
# also returns ||result||^2.  Off by default, like its three siblings.  Nothing here draws from the random stream.
AFFINE_ROUND_ONE = os.environ.get("TTIPM_AFFINE_ROUND_ONE", "0") == "1"
AFFINE_TERMS, AFFINE_PRODS = 4, 2  # terms `ttk_affine_round_one` takes, and how many of them may be products


def _affine_norm(terms, mids=None):
    """The terms as (coef, kind, a, b, transposed) with kind -1 and b None for a plain train, and the middle shape
    of every core of the result: `mids` (one tuple for all cores, or one per core) where given, else that of the
    first term whose cores have two middle indices (reversed where it enters transposed), else flat."""
    out = []
    for t in terms:
        coef, op, tr = (t[0], t[1], bool(t[2])) if len(t) == 3 else (t[0], t[1], False)
        if isinstance(op, tuple):
            kind, a, b = op
            assert kind in (0, 1, 2, 3) and len(a) == len(b)
        else:
            kind, a, b = -1, op, None
        out.append((float(coef), int(kind), a, b, tr))
    d = len(out[0][2])
    assert len(out) >= 1 and all(len(t[2]) == d for t in out)
    if mids is None:
        for _, kind, a, b, tr in out:
            own = _prod_out_modes(kind, a, b) if kind >= 0 else [tuple(c.shape[1:-1]) for c in a]
            if all(len(m) == 2 for m in own):
                mids = [m[::-1] if tr else m for m in own]
                break
        else:
            _, kind, a, b, _ = out[0]
            mids = [(int(np.prod(m)),) for m in (_prod_out_modes(kind, a, b) if kind >= 0
                                                 else [tuple(c.shape[1:-1]) for c in a])]
    elif isinstance(mids, tuple):
        mids = [mids] * d
    mids = [tuple(int(v) for v in m) for m in mids]
    assert all(len(m) == 2 for m in mids) or not any(t[4] for t in out), "a transposed term needs two middle indices"
    return out, mids


def _affine_composed(terms, mids):
    """The operand as a train of its own: every product exactly (the zip-up at eps 0 returns the unrounded
    Kronecker-bond cores), every term viewed with its own middle shape, then `_sum_composed`."""
    trains = []
    for _, kind, a, b, tr in terms:
        t = list(a) if kind < 0 else (tt_fast_matrix_vec_mul, tt_fast_mat_mat_mul, tt_fast_hadamard,
                                      tt_fast_hadamard)[kind](a, b, 0.0)
        trains.append([c.reshape(c.shape[0], *(m[::-1] if tr else m), c.shape[-1]) for c, m in zip(t, mids)])
    return _sum_composed(trains, [t[0] for t in terms], [t[4] for t in terms])


def _affine_round_one_plan(terms, mids):
    """The arguments of `ttk_affine_round_one` for these terms -- (d, inner, rows, n, terms) -- the summed and the
    bound ranks, and what keeps the tables alive, or None when the operand does not fit one workgroup's LDS,
    passes the term limits or has a single core."""
    d, n = len(mids), len(terms)
    if d < 2 or n > AFFINE_TERMS or sum(t[1] >= 0 for t in terms) > AFFINE_PRODS:
        return None
    I64, P, vp = ctypes.c_int64, ctypes.c_void_p * d, ctypes.c_void_p
    inner = (I64 * d)(*[int(np.prod(m)) for m in mids])
    rows = (I64 * d)(*[m[0] for m in mids]) if any(t[4] for t in terms) else None
    keep, recs = [], []
    for coef, kind, a, b, tr in terms:
        ca = [D.contig(c) for c in a]  # the contiguous inputs stay alive until the call is enqueued
        pa, ar = P(*[c.data_ptr() for c in ca]), _rank_array(a)
        keep += [ca, pa, ar]
        if kind < 0:
            recs.append(AffineTerm(-1, int(tr), coef, ctypes.cast(pa, vp), ctypes.cast(ar, vp), None, None, None))
            continue
        cb = [D.contig(c) for c in b]
        pb, br = P(*[c.data_ptr() for c in cb]), _rank_array(b)
        modes = (I64 * (3 * d))(*_zipup_modes(kind, a, b))
        keep += [cb, pb, br, modes]
        recs.append(AffineTerm(kind, int(tr), coef, ctypes.cast(pa, vp), ctypes.cast(ar, vp), ctypes.cast(pb, vp),
                               ctypes.cast(br, vp), ctypes.cast(modes, vp)))
    arr = (AffineTerm * n)(*recs)
    sums, bound = (I64 * (d + 1))(), (I64 * (d + 1))()
    if D.lib.ttk_affine_round_one_lds(d, inner, n, arr, sums, bound) < 0:
        return None
    return (d, inner, rows, n, arr), list(sums), list(bound), keep


def affine_round_one_lds(terms, mids=None):
    """Bytes of LDS `ttk_affine_round_one` needs for these terms (`tt_affine_rank_reduce`'s), -1 if the operand
    does not fit one workgroup or passes the limits (AFFINE_TERMS terms, AFFINE_PRODS of them products): the
    products and the sum are then built and rounded."""
    terms, mids = _affine_norm(terms, mids)
    plan = _affine_round_one_plan(terms, mids)
    if plan is None:
        return -1
    d, inner, _, n, arr = plan[0]
    return int(D.lib.ttk_affine_round_one_lds(d, inner, n, arr, None, None))


def _affine_native(terms, eps, mode, mids=None):
    """(tt, tail factor or None, ||tt||^2) from `ttk_affine_round_one` -- one launch into one fresh buffer sized by
    the bound ranks, one host read (the ranks, the tail and the squared norm) -- or None where that path is not
    taken: the switch is off, there is no GPU, d < 2, the operand does not fit or passes the term limits.  The
    caller's tensors are never written."""
    if not (AFFINE_ROUND_ONE and D.DEV.type == "cuda"):
        return None
    terms, mids = _affine_norm(terms, mids)
    plan = _affine_round_one_plan(terms, mids)
    if plan is None:
        return None
    (d, inner, rows, n, arr), sums, bound, keep = plan
    assert bound == retraction_ranks(inner, sums, [1 << 62] * (d - 1)), bound
    outs = _packed_flat(bound, list(inner))
    info = D.empty(d + 3)
    D._stream()
    D.check(D.lib.ttk_affine_round_one(D.ctx(), d, inner, rows, n, arr, float(eps), mode,
                                       (ctypes.c_void_p * d)(*[o.data_ptr() for o in outs]), info.data_ptr()),
            "affine_round_one")
    return _round_one_finish(outs, D.read(info), inner, mids, mode, d)


def tt_affine_rank_reduce(terms, eps=1e-18, with_norm2=False, mids=None):
    """`tt_rank_reduce` of sum_j coef_j op_j(T_j).  `terms`: (coef, train) or (coef, (kind, a, b)) -- the product of
    the trains a and b, kind 0 matrix x vector, 1 matrix x matrix, 2 / 3 Hadamard of vector / matrix trains --
    each optionally with a third entry, True where the term enters with its two middle indices swapped.  Weights
    are taken as given (a caller that mirrors `tt_scale` passes float(np.float32(alpha))).  `mids`: the result's
    middle shape (one tuple, or one per core) where the terms' own cores do not tell it, e.g. a transposed term
    stored flat.  With TTIPM_AFFINE_ROUND_ONE=1, on the GPU, for at most AFFINE_TERMS terms, AFFINE_PRODS of them
    products, that fit (`affine_round_one_lds`): one launch and one host read (`ttk_affine_round_one`), no product
    and no sum ever built.  Otherwise the products are built exactly, summed (`_sum_composed`) and rounded as
    today.  with_norm2: returns (tt, ||tt||^2) -- the kernel's own figure, or one `tt_inner_prod`."""
    res = _affine_native(terms, eps, 0, mids)
    if res is not None:
        return (res[0], res[2]) if with_norm2 else res[0]
    tt = tt_rank_reduce(_affine_composed(*_affine_norm(terms, mids)), eps)
    return (tt, tt_inner_prod(tt, tt)) if with_norm2 else tt


# Several independent affine roundings in one launch, one workgroup each (`ttk_affine_round_many`): the solve
# issues its residuals, the two Kronecker blocks and the blocks of a Newton step in groups whose members do not
# depend on each other, and each single call keeps one CU busy while the host waits once per member.  Every job's
# bits are those of its own `ttk_affine_round_one`.  Off by default, like its siblings; nothing here draws from
# the random stream.
AFFINE_ROUND_MANY = os.environ.get("TTIPM_AFFINE_ROUND_MANY", "0") == "1"
AFFINE_JOBS = 8  # jobs `ttk_affine_round_many` takes (TTK_ROUND_MANY_MAX)


def _affine_many_plan(jobs):
    """The normalised jobs [(terms, eps, mode, mids)], their `_affine_round_one_plan`s and the `ttk_affine_job`
    table with every `out` still null, or None when there are no jobs, more than AFFINE_JOBS, or one without a
    plan."""
    if not 1 <= len(jobs) <= AFFINE_JOBS:
        return None
    norm, plans, recs = [], [], []
    for terms, eps, mode, mids in jobs:
        terms, mids = _affine_norm(terms, mids)
        plan = _affine_round_one_plan(terms, mids)
        if plan is None:
            return None
        d, inner, rows, n, arr = plan[0]
        vp = ctypes.c_void_p
        norm.append((terms, float(eps), int(mode), mids))
        plans.append(plan)
        recs.append(AffineJob(d, ctypes.cast(inner, vp), None if rows is None else ctypes.cast(rows, vp), n,
                              ctypes.cast(arr, vp), float(eps), int(mode), None))
    return norm, plans, (AffineJob * len(recs))(*recs)


def affine_round_many_lds(jobs):
    """Bytes of LDS one `ttk_affine_round_many` launch of these jobs (`tt_affine_rank_reduce_many`'s) declares --
    the largest of the jobs' own requests -- or -1 when the batch cannot run as one launch: no job or more than
    AFFINE_JOBS, or a job that does not fit one workgroup or passes the term limits."""
    plan = _affine_many_plan(jobs)
    if plan is None:
        return -1
    return int(D.lib.ttk_affine_round_many_lds(len(jobs), plan[2], None, None))


def _affine_many_native(jobs):
    """[(tt, tail factor or None, ||tt||^2)] from one `ttk_affine_round_many` launch -- one fresh buffer for every
    job's output cores and one for the info block, one host read of the info block -- or None where that path is
    not taken: the switch is off, there is no GPU, fewer than 2 or more than AFFINE_JOBS jobs, or a job without a
    plan.  The callers' tensors are never written."""
    if not (AFFINE_ROUND_MANY and D.DEV.type == "cuda") or len(jobs) < 2:
        return None
    plan = _affine_many_plan(jobs)
    if plan is None:
        return None
    norm, plans, table = plan
    nj = len(norm)
    sizes, at = [], [0]
    for (d, inner, _, _, _), sums, bound, _ in plans:
        assert bound == retraction_ranks(inner, sums, [1 << 62] * (d - 1)), bound
        sizes += [bound[k] * inner[k] * bound[k + 1] for k in range(d)]
        at.append(len(sizes))
    flat = _packed(sizes)
    ioff = (ctypes.c_int64 * (nj + 1))()
    keep = []
    for j in range(nj):
        outs = flat[at[j]:at[j + 1]]
        ptrs = (ctypes.c_void_p * len(outs))(*[o.data_ptr() for o in outs])
        keep.append(ptrs)
        table[j].out = ctypes.cast(ptrs, ctypes.c_void_p)
    if D.lib.ttk_affine_round_many_lds(nj, table, ioff, None) < 0:
        return None
    info = D.empty(int(ioff[nj]))
    D._stream()
    D.check(D.lib.ttk_affine_round_many(D.ctx(), nj, table, info.data_ptr()), "affine_round_many")
    got = D.read(info)
    res = []
    for j, ((_, _, mode, mids), plan) in enumerate(zip(norm, plans)):
        d, inner = plan[0][0], plan[0][1]
        res.append(_round_one_finish(flat[at[j]:at[j + 1]], got[int(ioff[j]):int(ioff[j + 1])], inner, mids, mode, d))
    return res


def tt_affine_rank_reduce_many(jobs):
    """Several independent roundings of `tt_affine_rank_reduce`'s operand.  `jobs`: a list of (terms, eps, mode,
    mids), `terms` and `mids` as there, mode 0 `tt_rank_reduce` / 1 the tracked rounding of `tt_psd_rank_reduce`
    (at eps / 2, the discarded tail summed).  Returns one (tt, tail factor or None, ||tt||^2) per job, in order;
    the tracked variant's correction (`_psd_correct`) is the caller's.  With TTIPM_AFFINE_ROUND_MANY=1, on the
    GPU, for 2 to AFFINE_JOBS jobs every one of which has a plan (`affine_round_many_lds`): one launch with one
    workgroup per job, one host read of every job's ranks, tail and squared norm, one output allocation
    (`ttk_affine_round_many`), each job's bits those of its own `ttk_affine_round_one`.  Otherwise each job in
    turn as `tt_affine_rank_reduce` runs it: `ttk_affine_round_one` where it is taken, else the composed path."""
    jobs = list(jobs)
    res = _affine_many_native(jobs)
    if res is not None:
        return res
    res = []
    for terms, eps, mode, mids in jobs:
        one = _affine_native(terms, eps, mode, mids)
        if one is None:
            op = _affine_composed(*_affine_norm(terms, mids))
            tt, factor = _tail_rank_reduce(op, eps) if mode else (tt_rank_reduce(op, eps), None)
            one = (tt, factor, tt_inner_prod(tt, tt))
        res.append(one)
    return res


def tt_fast_matrix_vec_mul(mat, vec, eps=1e-18):
    """`cy_src/tt_ops_cy.pyx:428-447`: mat (r_A,m,n,R_A) x vec (r,n,R) -> (r_A r, m, R_A R), rounded
    at eps (see the note above)."""
    if ZIPUP:
        return _zipup_matrix_vec_mul(mat, vec, eps)
    res = _prod_native(0, mat, vec, eps)
    if res is not None:
        return res
    if _use_native_zipup():
        return _native_zipup(0, mat, vec, eps, [(a.shape[1],) for a in mat])
    cores = []
    for a, x in zip(mat, vec):
        ra, m, _, Ra = a.shape
        r, _, R = x.shape
        cores.append(D.einsum("amnA,rnR->armAR", a, x).view(ra * r, m, Ra * R))
    return _kron_round(cores, eps)


def tt_fast_mat_mat_mul(m1, m2, eps=1e-18):
    """`cy_src/tt_ops_cy.pyx:449-464`: core-wise matrix product, rounded at eps."""
    if ZIPUP:
        return _zipup_mat_mat_mul(m1, m2, eps)
    res = _prod_native(1, m1, m2, eps)
    if res is not None:
        return res
    if _use_native_zipup():
        return _native_zipup(1, m1, m2, eps, [(a.shape[1], b.shape[2]) for a, b in zip(m1, m2)])
    cores = []
    for a, b in zip(m1, m2):
        ra, m, _, Ra = a.shape
        rb, _, n, Rb = b.shape
        cores.append(D.einsum("amkA,bknB->abmnAB", a, b).view(ra * rb, m, n, Ra * Rb))
    return _kron_round(cores, eps)


def tt_fast_hadamard(t1, t2, eps=1e-18):
    """`cy_src/tt_ops_cy.pyx:466-502`: core-wise Hadamard product, rounded at eps."""
    if ZIPUP:
        return _zipup_hadamard(t1, t2, eps)
    four = t1[0].dim() == 4 and t2[0].dim() == 4
    res = _prod_native(3 if four else 2, t1, t2, eps) if four or (t1[0].dim() == 3 and t2[0].dim() == 3) else None
    if res is not None:
        return res
    if _use_native_zipup() and (four or (t1[0].dim() == 3 and t2[0].dim() == 3)):
        return _native_zipup(3 if four else 2, t1, t2, eps, [tuple(a.shape[1:-1]) for a in t1])
    cores = []
    for a, b in zip(t1, t2):
        if four:
            cores.append(D.einsum("aijA,bijB->abijAB", a, b).view(a.shape[0] * b.shape[0], a.shape[1], a.shape[2],
                                                                  a.shape[3] * b.shape[3]))
        else:
            cores.append(D.einsum("aiA,biB->abiAB", a, b).view(a.shape[0] * b.shape[0], a.shape[1],
                                                             a.shape[2] * b.shape[2]))
    return _kron_round(cores, eps)


# ------------------------------------------------------------------ `src/tt_ops.py` helpers
def tt_merge_cores(tt):
    """`src/tt_ops.py:335-339`"""
    if tt[0].dim() == 3:
        return [D.einsum("kir,rsK->kisK", a, b) for a, b in zip(tt[:-1:2], tt[1::2])]
    return [D.einsum("kijr,rsdK->kisjdK", a, b) for a, b in zip(tt[:-1:2], tt[1::2])]


def tt_reshape(tt, shape):
    """`src/tt_ops.py:330-333` (views of contiguous cores)."""
    if np.prod(shape) > np.prod(tt[0].shape[1:-1]):
        tt = tt_merge_cores(tt)
    return [D.contig(c).view(c.shape[0], *shape, c.shape[-1]) for c in tt]


def tt_IkronM(tt):
    """`src/tt_ops.py:360-363`"""
    eye = _eye_core()
    return [D.einsum("rmnR,lijL->rlminjRL", eye, c).view(c.shape[0], 4, 4, c.shape[-1]) for c in tt]


def tt_MkronI(tt):
    """`src/tt_ops.py:365-368`"""
    eye = _eye_core()
    return [D.einsum("rmnR,lijL->rlminjRL", c, eye).view(c.shape[0], 4, 4, c.shape[-1]) for c in tt]


def tt_diag_op(tt, eps=1e-18):
    """`src/tt_ops.py:371-375`"""
    n = tt[0].shape[1] * tt[0].shape[2]
    eye = _const(f"eyemat{n}", np.eye(n))
    basis = [D.einsum("ij,rjR->rijR", eye, D.contig(c).view(c.shape[0], n, c.shape[3])) for c in tt]
    return tt_rank_reduce(basis, eps)


def tt_diag(vec, eps=1e-18):
    """`src/tt_ops.py:312-316`"""
    n = vec[0].shape[1]
    eye = _const(f"eyemat{n}", np.eye(n))
    return tt_rank_reduce([D.einsum("ij,rjR->rijR", eye, c) for c in vec], eps)


def tt_entrywise_sum(tt):
    """`src/tt_ops.py:342-352`"""
    eq = "ab,aijm,bijn->mn" if tt[0].dim() == 4 else "ab,aim,bin->mn"
    one = _const("ones_" + "x".join(map(str, tt[0].shape[1:-1])), np.ones((1, *tt[0].shape[1:-1], 1)))
    res = reduce(lambda r, c: D.einsum(eq, r, c, one), tt, _const("one11", np.ones((1, 1))))
    return float(np.sum(D.read(res)))


def tt_sum(*args, op_tol=1e-18, rank_reduce=True):
    """`src/tt_ops.py:321-328`"""
    acc = args[0]
    for a in args[1:]:
        acc = tt_rank_reduce(tt_add(acc, a), op_tol) if rank_reduce else tt_add(acc, a)
    return acc


def tt_split_bonds(tt):
    """`src/tt_ops.py:247-265` (problem generators only)."""
    out = []
    for core in tt:
        sh = core.shape
        k = len(sh) // 2
        U, S, Vt, s = D.svd(D.contig(core).view(int(np.prod(sh[:k])), -1))
        keep = np.nonzero(np.abs(s) > 1e-18)[0]
        if len(keep) == 0:
            keep = np.array([0])
        r = len(keep)
        assert np.array_equal(keep, np.arange(r))  # singular values are sorted descending
        out += [D.clone(U[:, :r]).view(*sh[:k], r), D.einsum("r,rj->rj", S[:r], Vt[:r]).view(r, *sh[k:])]
    return out


def _tril_host(d, upper):
    e = lambda i, j: (lambda z: (z.__setitem__((slice(None), i, j), 1.0), z)[1])(np.zeros((1, 2, 2, 1)))  # noqa: E731
    if d == 1:
        m = np.array([[1, 1], [0, 1]] if upper else [[1, 0], [1, 1]], dtype=float)
        return [m.reshape(1, 2, 2, 1)]
    one, zero = np.ones((1, 2, 2, 1)), np.zeros((1, 2, 2, 1))
    off = e(0, 1) if upper else e(1, 0)
    dg = e(0, 0) + e(1, 1)
    return ([np.concatenate((off, dg), axis=-1)]
            + [np.concatenate((np.concatenate((one, off), axis=0), np.concatenate((zero, dg), axis=0)), axis=-1)
               for _ in range(d - 2)]
            + [np.concatenate((one, off + dg), axis=0)])


def tt_tril_one_matrix(dim):
    """`src/tt_ops.py:377-385`"""
    return to_device(_tril_host(dim, False))


def tt_triu_one_matrix(dim):
    """`src/tt_ops.py:387-395`"""
    return to_device(_tril_host(dim, True))


def tt_to_tensor(tt):
    """`src/tt_ops.py:192-196` (host reconstruction, tests / small d only)."""
    t = D.read(tt[0])
    for c in tt[1:]:
        t = np.tensordot(t, D.read(c), axes=(-1, 0))
    return np.sum(t, axis=(0, -1))


def tt_matrix_to_matrix(mtt):
    """`src/tt_ops.py:211-217`"""
    if len(mtt) == 1:
        return np.squeeze(D.read(mtt[0]))
    t = tt_to_tensor(mtt)
    n = t.ndim
    axes = list(range(0, n - 1, 2)) + list(range(1, n, 2))
    return np.transpose(t, axes).reshape(int(np.prod(t.shape[:n // 2])), -1)
