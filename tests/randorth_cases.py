"""Shared by tests/test_host_randorth.py (CPU, emulated libttk) and tests/test_gpu_randorth.py (MI355X):
the randomised-rounding fixtures of tests/golden/randorth.npz (made by tests/golden/make_randorth.py
from the reference) and the checks both files apply to a result.

Tolerances.  The represented tensor is gauge-free; swapping the QR implementation moves it by at
most 1.4e-15 (relative Frobenius, NumPy restatement on cases b-e), so the 1e-11 the rounding and
zip-up goldens use (tests/test_gpu_parity.py `_close`) holds with margin.  Output ranks are host
arithmetic: exact.  Q is a product of Householder reflectors applied to identity columns: its
orthonormality error is a few ulps times the column count (7e-16 measured on the CPU), bound 1e-12."""
import numpy as np

from tests.tt_cases import J_SHAPES, close, dense, load, orth_error  # noqa: F401  (re-exported)

_F = load("randorth.npz")
G, _tt, train, check_rng_state = _F.G, _F._tt, _F.train, _F.check_rng_state

SWEEP = ("a", "b", "c", "d", "e", "f", "g", "h", "j")   # cases with d >= 2
FIT = ("a", "b", "c", "d", "e", "f", "g", "h")          # cases that fit one workgroup's LDS
RL = ("a", "c", "e")
PUBLIC = ("c", "g")


def sketch(cid):
    return _tt(f"{cid}/sketch")


def wide_case():
    """(train, sketch), seeded: d = 4, middle extents (4, 4), bond and sketch ranks 12, so A_k W_{k+1} has
    12 * 16 * 12 = 2304 > 2048 entries and `ttk_rand_orth` runs 1024 threads, which no fixture case does."""
    rs = np.random.RandomState(12)
    return tuple([rs.randn(a, 4, 4, b) for a, b in zip((1, 12, 12, 12), (12, 12, 12, 1))] for _ in range(2))


def targets(cid):
    return [int(v) for v in G[f"{cid}/targets"]]


def check_result(cid, res_host, which="lr"):
    """ranks exactly the reference's, dense tensor to 1e-11, orthonormal unfoldings to 1e-12"""
    assert [c.shape[0] for c in res_host[1:]] == [int(v) for v in G[f"{cid}/{which}_ranks"]]
    assert all(a.shape[-1] == b.shape[0] for a, b in zip(res_host[:-1], res_host[1:]))
    close(dense(res_host), G[f"{cid}/{which}_dense"], 1e-11)
    assert orth_error(res_host, left=which != "rl") <= 1e-12
