"""What tests/randorth_cases.py, tests/nystroem_cases.py and tests/retract_cases.py share: reading a
fixture of tests/golden/, its input trains, and the checks on a tensor train that do not depend on the
rounding (the represented tensor, a relative max-abs comparison, orthonormal unfoldings, NumPy's stream
state).  The case tuples, the tolerances and `check_result` stay with each rounding's own module."""
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
J_SHAPES = [(1, 4, 4, 96), (96, 4, 4, 96), (96, 4, 4, 1)]


class Fixture:
    """One .npz of tests/golden/: trains stored as `<key>/n` and `<key>/<i>`, case j's input as a seed."""

    def __init__(self, npz):
        self.G = np.load(os.path.join(HERE, "golden", npz))
        self._inputs = {}

    def _tt(self, key):
        return [self.G[f"{key}/{i}"].copy() for i in range(int(self.G[key + "/n"]))]

    def train(self, cid):
        """The case's input train (host arrays; a fresh copy per call)."""
        if cid not in self._inputs:
            if cid == "j":  # too large to store: regenerated from the recorded seed (legacy stream: frozen)
                rs = np.random.RandomState(int(self.G["j/seed"]))
                self._inputs[cid] = [rs.randn(*s) for s in J_SHAPES]
            else:
                self._inputs[cid] = self._tt(f"{cid}/in")
        return [c.copy() for c in self._inputs[cid]]

    def check_rng_state(self, cid):
        """NumPy's global MT19937 state equals the one the reference's public call left"""
        st = np.random.get_state()
        assert np.array_equal(st[1], self.G[f"{cid}/pub_key"])
        assert st[2] == int(self.G[f"{cid}/pub_pos"]) and st[3] == int(self.G[f"{cid}/pub_has_gauss"])
        assert st[4] == float(self.G[f"{cid}/pub_gauss"])


def load(npz):
    return Fixture(npz)


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
