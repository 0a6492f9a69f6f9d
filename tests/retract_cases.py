"""Shared by tests/test_host_retract.py (CPU, emulated libttk) and tests/test_gpu_retract.py (MI355X): the
fixed-rank retraction fixtures of tests/golden/retract.npz (made by tests/golden/make_retract.py from the
reference's own `tt_rank_retraction`) and the checks both files apply to a result.

Tolerances.  The output cores are gauge-dependent (SVD signs, the scalar the reference's QR sweep moves
into the last core), the tensor they represent is not: it is compared, rebuilt from the reference's
stored cores, to the project's 1e-11 relative max-abs (tests/test_gpu_parity.py `_close`).  A truncated
SVD moves with the gap behind the last kept singular value, so that bound is not automatically safe:
the fixture records per case `noise`, the largest change of the reference's own dense output over 5
reruns with every train entry moved by 1.1e-16 relative, and a case takes part in value checks only if
50 x noise <= 1e-11 (50: the parity policy's multiple).  That condition is asserted here on
import, so a regenerated fixture cannot bring in an ill-posed case.  Output ranks are host arithmetic:
exact.  Left unfoldings are orthonormal to 1e-12 (the bound of tests/randorth_cases.py: a Jacobi's
rotations or its normalised rows, a few hundred flops deep at these sizes) on every case but z, whose
kept near-zero singular values give unit columns of rounding noise."""
import numpy as np

from tests.tt_cases import J_SHAPES, close, dense, load, orth_error  # noqa: F401  (re-exported)

_F = load("retract.npz")
G, _tt, train = _F.G, _F._tt, _F.train

VALUE = ("f", "a", "b", "c", "d", "h", "k", "e", "w", "z", "j")   # every case with d >= 2
FIT = ("f", "a", "b", "c", "d", "h", "k", "e", "w", "z")          # value cases that fit one workgroup's LDS
ORTH = tuple(c for c in FIT if c != "z")
REPRODUCE = ("a", "c", "k", "z")                                   # nothing but null directions dropped
RTOL = 1e-11
ORTH_TOL = 1e-12
NOISE_MULTIPLE = 50

for _c in VALUE:
    assert NOISE_MULTIPLE * float(G[f"{_c}/noise"]) <= RTOL, (_c, float(G[f"{_c}/noise"]))


_DENSE = {}


def upper(cid):
    return [int(v) for v in G[f"{cid}/upper"]]


def ranks(cid):
    """the reference's output ranks, d+1 entries with the boundaries"""
    return [int(v) for v in G[f"{cid}/ranks"]]


def inner_and_ranks(tt):
    return ([int(np.prod(c.shape[1:-1])) for c in tt], [int(tt[0].shape[0])] + [int(c.shape[-1]) for c in tt])


def reference_dense(cid):
    """The tensor the reference's output represents (computed once per case, shared, read only)."""
    if cid not in _DENSE:
        _DENSE[cid] = dense(_tt(f"{cid}/out"))
        _DENSE[cid].setflags(write=False)
    return _DENSE[cid]


def check_shapes(cid, res_host):
    """ranks exactly the reference's, bonds consistent, middle extents kept"""
    host = train(cid)
    assert [res_host[0].shape[0]] + [c.shape[-1] for c in res_host] == ranks(cid)
    assert all(a.shape[-1] == b.shape[0] for a, b in zip(res_host[:-1], res_host[1:]))
    assert [c.shape[1:-1] for c in res_host] == [c.shape[1:-1] for c in host]


def check_result(cid, res_host):
    """exact ranks, bond consistency, dense tensor to 1e-11"""
    check_shapes(cid, res_host)
    close(dense(res_host), reference_dense(cid), RTOL)


def check_left_orthonormal(res_host):
    """cores 0 .. d-2: the left unfolding (q_i n_i, q_{i+1}) has orthonormal columns"""
    assert orth_error(res_host) <= ORTH_TOL
