"""Shared by tests/test_host_nystroem.py (CPU, emulated libttk) and tests/test_gpu_nystroem.py (MI355X):
the generalised-Nystroem fixtures of tests/golden/nystroem.npz (made by tests/golden/make_nystroem.py
from the reference) and the checks both files apply to a result.

Tolerances.  The output cores are gauge-dependent (SVD signs, order within equal S), the tensor they
represent is not: it is compared, rebuilt from the reference's stored cores, to the project's 1e-11
relative max-abs (tests/test_gpu_parity.py `_close`).  Nystroem divides by sqrt(S), so that bound is
not automatically safe: the fixture records per case `noise`, the largest change of the reference's
own dense output over 5 reruns with every train entry moved by 1.1e-16 relative, and a case takes
part in value checks only if 50 x noise <= 1e-11 (50: the parity policy's multiple).
That condition is asserted here on import, so a regenerated fixture cannot bring in an ill-posed
case.  Case z (P singular at the first bond, cond ~ 1e17) is in the fixture for shapes only: the
reference's 1/sqrt(~0) output is rounding noise.  Output ranks are host arithmetic: exact."""
import numpy as np

from tests.tt_cases import J_SHAPES, close, dense, load  # noqa: F401  (re-exported)

_F = load("nystroem.npz")
G, _tt, train, check_rng_state = _F.G, _F._tt, _F.train, _F.check_rng_state

VALUE = ("a", "b", "c", "d", "e", "f", "g", "h", "k", "j")   # every case with d >= 2 but z
FIT = ("a", "b", "c", "d", "e", "f", "g", "h", "k")          # value cases whose cores fit one workgroup's LDS
PUBLIC = ("c", "g")
REPRODUCE = ("a", "e", "k")                                   # every target >= the tensor's own TT rank
RTOL = 1e-11
NOISE_MULTIPLE = 50

for _c in VALUE:
    assert NOISE_MULTIPLE * float(G[f"{_c}/noise"]) <= RTOL, (_c, float(G[f"{_c}/noise"]))
for _c in PUBLIC:
    assert NOISE_MULTIPLE * float(G[f"{_c}/pub_noise"]) <= RTOL, (_c, float(G[f"{_c}/pub_noise"]))
assert float(G["z/cond"]) > 1e15  # z stays the singular case it is meant to be


_DENSE = {}


def sketches(cid):
    """(left sketch, right sketch): the reference's tt_gaussian_1 and tt_gaussian_2"""
    return _tt(f"{cid}/sk1"), _tt(f"{cid}/sk2")


TRANSPOSED_SEED = 27   # cond(P) 5 at both bonds; 50 x noise 1.1e-13 on the CPU


def transposed_case():
    """(train, left sketch, right sketch), seeded: d = 3, middle extents (2, 2), bond ranks 6, left sketch
    ranks (1, 5, 5, 1) above the right ones (1, 3, 3, 1), so the bond SVD rotates the rows of P^T, which
    no fixture case does.  A true truncation (6 -> 3): tests/test_host_nystroem.py asserts that this
    seed is as well posed as the fixture's value cases."""
    rs = np.random.RandomState(TRANSPOSED_SEED)
    return tuple([rs.randn(a, 2, 2, b) for a, b in zip(rk[:-1], rk[1:])]
                 for rk in ((1, 6, 6, 1), (1, 5, 5, 1), (1, 3, 3, 1)))


def targets(cid):
    return [int(v) for v in G[f"{cid}/targets"]]


def contractions(cid, which):
    """the reference's tt_lr_contraction (which = "WL") or tt_rl_contraction ("WR") list"""
    return [G[f"{cid}/{which}/{k}"] for k in range(len(targets(cid)))]


def reference_dense(cid, which="out"):
    """The tensor the reference's output represents (computed once per case, shared, read only)."""
    key = f"{cid}/{which}"
    if key not in _DENSE:
        _DENSE[key] = dense(_tt(key))
        _DENSE[key].setflags(write=False)
    return _DENSE[key]


def check_shapes(cid, res_host, which=""):
    """ranks exactly the reference's, bonds consistent, boundary ranks and middle extents kept"""
    host = train(cid)
    assert [c.shape[0] for c in res_host[1:]] == [int(v) for v in G[f"{cid}/{which}ranks"]]
    assert all(a.shape[-1] == b.shape[0] for a, b in zip(res_host[:-1], res_host[1:]))
    assert res_host[0].shape[0] == host[0].shape[0] and res_host[-1].shape[-1] == host[-1].shape[-1]
    assert [c.shape[1:-1] for c in res_host] == [c.shape[1:-1] for c in host]


def check_result(cid, res_host, which=""):
    """exact ranks, bond consistency, dense tensor to 1e-11 (which = "pub_": the public call)"""
    check_shapes(cid, res_host, which)
    close(dense(res_host), reference_dense(cid, which + "out"), RTOL)
