"""Shared by tests/test_host_randorth.py (CPU, emulated libttk) and tests/test_gpu_randorth.py (MI355X):
the randomised-rounding fixtures of tests/golden/randorth.npz (made by tests/golden/make_randorth.py
from the reference) and the checks both files apply to a result.

Tolerances.  The represented tensor is gauge-free; swapping the QR implementation moves it by at
most 1.4e-15 (relative Frobenius, NumPy restatement on cases b-e), so the 1e-11 the rounding and
zip-up goldens use (tests/test_gpu_parity.py `_close`) holds with margin.  Output ranks are host
arithmetic: exact.  Q is a product of Householder reflectors applied to identity columns: its
orthonormality error is a few ulps times the column count (7e-16 measured on the CPU), bound 1e-12."""
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
G = np.load(os.path.join(HERE, "golden", "randorth.npz"))

SWEEP = ("a", "b", "c", "d", "e", "f", "g", "h", "j")   # cases with d >= 2
FIT = ("a", "b", "c", "d", "e", "f", "g", "h")          # cases that fit one workgroup's LDS
RL = ("a", "c", "e")
PUBLIC = ("c", "g")
J_SHAPES = [(1, 4, 4, 96), (96, 4, 4, 96), (96, 4, 4, 1)]


def _tt(key):
    return [G[f"{key}/{i}"].copy() for i in range(int(G[key + "/n"]))]


_INPUTS = {}


def train(cid):
    """The case's input train (host arrays; a fresh copy per call)."""
    if cid not in _INPUTS:
        if cid == "j":  # too large to store: regenerated from the recorded seed (legacy stream: frozen)
            rs = np.random.RandomState(int(G["j/seed"]))
            _INPUTS[cid] = [rs.randn(*s) for s in J_SHAPES]
        else:
            _INPUTS[cid] = _tt(f"{cid}/in")
    return [c.copy() for c in _INPUTS[cid]]


def sketch(cid):
    return _tt(f"{cid}/sketch")


def targets(cid):
    return [int(v) for v in G[f"{cid}/targets"]]


def dense(tt):
    t = tt[0]
    for c in tt[1:]:
        t = np.tensordot(t, c, axes=(-1, 0))
    return np.sum(t, axis=(0, -1))


def close(a, b, rtol):
    scale = max(np.max(np.abs(b)), 1e-300)
    err = np.max(np.abs(np.asarray(a) - b)) / scale
    assert err <= rtol, err


def orth_error(cores, left=True):
    """max |Q^T Q - I| over every core but the last (left unfoldings), or but the first (right)."""
    worst = 0.0
    for c in (cores[:-1] if left else cores[1:]):
        q = c.reshape(-1, c.shape[-1]) if left else c.reshape(c.shape[0], -1).T
        worst = max(worst, float(np.max(np.abs(q.T @ q - np.eye(q.shape[1])))))
    return worst


def check_result(cid, res_host, which="lr"):
    """ranks exactly the reference's, dense tensor to 1e-11, orthonormal unfoldings to 1e-12"""
    assert [c.shape[0] for c in res_host[1:]] == [int(v) for v in G[f"{cid}/{which}_ranks"]]
    assert all(a.shape[-1] == b.shape[0] for a, b in zip(res_host[:-1], res_host[1:]))
    close(dense(res_host), G[f"{cid}/{which}_dense"], 1e-11)
    assert orth_error(res_host, left=which != "rl") <= 1e-12


def check_rng_state(cid):
    """NumPy's global MT19937 state equals the one the reference's public call left"""
    st = np.random.get_state()
    assert np.array_equal(st[1], G[f"{cid}/pub_key"])
    assert st[2] == int(G[f"{cid}/pub_pos"]) and st[3] == int(G[f"{cid}/pub_has_gauss"])
    assert st[4] == float(G[f"{cid}/pub_gauss"])
