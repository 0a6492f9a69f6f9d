"""Shared by tests/test_host_round_one.py (CPU, emulated libttk) and tests/test_gpu_round_one.py (MI355X): the
eps-truncating rounding fixtures of tests/golden/round_one.npz (made by tests/golden/make_round_one.py from
the reference's own `tt_rank_reduce`, `tt_psd_rank_reduce` and `tt_mask_rank_reduce`) and the checks both
files apply to a result.

Tolerances.  The output cores are gauge-dependent, the tensor they represent is not: it is compared, rebuilt
from the reference's stored cores, to the project's 1e-11 relative max-abs (tests/test_gpu_parity.py
`_close`).  Output ranks are compared exactly, which is only fair where no decision is a near tie: the
fixture records per case `margin`, the smallest factor by which a tail sum of the reference's sweep
misses the squared threshold, and `noise`, the largest change of the reference's own dense output over 5
reruns with every train entry moved by 1.1e-16 relative.  A case takes part only if margin >= 3 (a Jacobi
singular value differs from gesvd's by rounding, so any factor clearly above 1 keeps the decision) and
50 x noise <= 1e-11 (50: the parity policy's multiple).  Both are asserted here on import, so a
regenerated fixture cannot bring in an ill-posed case.  Left unfoldings are orthonormal to 1e-12 (the
bound of tests/retract_cases.py) on the mode-0 cases but z and o, whose kept noise-level or null
singular values give unit columns of rounding noise."""
import numpy as np

from tests.tt_cases import J_SHAPES, close, dense, load, orth_error  # noqa: F401  (re-exported)

_F = load("round_one.npz")
G, _tt, train = _F.G, _F._tt, _F.train

VALUE = ("f", "a", "b", "p", "q", "n", "c", "d", "h", "t", "z", "o", "e", "w", "j")   # every case that is rounded
FIT = tuple(c for c in VALUE if c != "j")                           # those that fit one workgroup's LDS
UNCHANGED = ("i", "u")                                              # d = 1, all ranks 1
TRACKED = tuple(c for c in VALUE if int(G[f"{c}/mode"]) > 0)        # p, q, n
ORTH = tuple(c for c in FIT if c not in TRACKED and c not in ("z", "o"))
RTOL = 1e-11
ORTH_TOL = 1e-12
NOISE_MULTIPLE = 50
MARGIN = 3.0

for _c in VALUE:
    assert NOISE_MULTIPLE * float(G[f"{_c}/noise"]) <= RTOL, (_c, float(G[f"{_c}/noise"]))
    assert float(G[f"{_c}/margin"]) >= MARGIN, (_c, float(G[f"{_c}/margin"]))
assert TRACKED == ("p", "q", "n")
assert float(G["p/factor"]) > 0.0 and float(G["q/factor"]) > 0.0 and float(G["n/factor"]) == 0.0

_DENSE = {}


def eps(cid):
    return float(G[f"{cid}/eps"])


def mode(cid):
    """0 `tt_rank_reduce`, 1 `tt_psd_rank_reduce`, 2 `tt_mask_rank_reduce`"""
    return int(G[f"{cid}/mode"])


def mask(cid):
    return _tt(f"{cid}/mask")


def ranks(cid):
    """the ranks of the reference's public output, d+1 entries with the boundaries"""
    return [int(v) for v in G[f"{cid}/ranks"]]


def qranks(cid):
    """the rounded ranks (before a tracked variant adds its correction), d+1 entries"""
    return [int(v) for v in G[f"{cid}/qranks"]]


def factor(cid):
    """the tracked variants' factor, tail ** (1 / (2 d))"""
    return float(G[f"{cid}/factor"])


def inner_and_ranks(tt):
    return ([int(np.prod(c.shape[1:-1])) for c in tt], [int(tt[0].shape[0])] + [int(c.shape[-1]) for c in tt])


def public(T, cid, tt):
    """the case's public call on the device train `tt`"""
    if mode(cid) == 0:
        return T.tt_rank_reduce(tt, eps(cid))
    if mode(cid) == 1:
        return T.tt_psd_rank_reduce(tt, eps(cid))
    return T.tt_mask_rank_reduce(tt, T.to_device(mask(cid)), eps(cid))


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
