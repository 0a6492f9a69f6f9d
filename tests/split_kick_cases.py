"""Shared by tests/test_host_split_kick.py (CPU, emulated libttk) and tests/test_gpu_split_kick.py (MI355X): the
truncate-and-kick fixtures of tests/golden/split_kick.npz (made by tests/golden/make_split_kick.py from the
reference's own `_add_kick_rank` / `_add_kick_rank_rev`) and the checks both files apply to a result.

Tolerances.  The product s1 s2 does not depend on the factorisation's gauge: it is compared to the project's
1e-11 relative max-abs (`tt_cases.close`).  The factors themselves are compared elementwise to the same bound
where the recorded 2-norm condition number of the concatenated matrix is below 1e6: a Householder factor moves
by about cond x eps.  The fixture records per case `noise`, the largest change of the reference's own s1, s2
and product over 5 reruns with every input entry moved by 1.1e-16 relative, and a case takes part in value
checks only if 50 x noise <= 1e-11 (50: the parity policy's multiple); asserted here on import.
The composed path is compared in the same way in the forward direction, where both sides are LAPACK-gauged
QRs.  In the backward direction `dev.rq` factors cat^T J, which pivots each reflector on the first entry of a
row where LAPACK's dgerqf (scipy.linalg.rq, and `ttk_split_kick`) pivots on the last: the two RQs differ by a
diagonal D of +-1, Q' = D Q and Rm' = Rm D (in NumPy, on Gaussian 7 x 8, 8 x 6 and 10 x 66 matrices,
max |Q' - Q| = 1.35, 1.57, 0.58 with max ||Q'| - |Q|| <= 1e-15).  `check_same_split` therefore reads D off the
orthonormal factor (every row must match its counterpart to 1e-11 up to one sign), requires D = I in the forward
direction, and holds s1 D and D s2 elementwise, and s1 s2, to 1e-11: nothing but those signs may differ.
The rank is host arithmetic: exact.  The orthonormal factor's Gram matrix and the projection of the
concatenated matrix onto its range are held to 1e-12 (the bound of tests/randorth_cases.py: a few hundred
flops deep at these sizes)."""
import numpy as np

from tests.tt_cases import close, load  # noqa: F401  (re-exported)

G = load("split_kick.npz").G

ALL = ("a", "b", "c", "d", "e", "f", "g", "h", "z", "j")
FIT = tuple(c for c in ALL if c != "j")        # cases whose working set fits one workgroup's LDS
SPLIT = tuple(c for c in ALL if int(G[f"{c}/dims"][5]) == 4 and f"{c}/S" in G.files and c != "z")  # tt_eig._split's shape
RTOL = 1e-11
ORTH_TOL = 1e-12
COND_MAX = 1e6
NOISE_MULTIPLE = 50
LDS_MAX = 160 * 1024

for _c in ALL:
    assert NOISE_MULTIPLE * float(G[f"{_c}/noise"]) <= RTOL, (_c, float(G[f"{_c}/noise"]))


def dims(cid):
    """(rev, a, b, p, r, r_add)"""
    return tuple(int(v) for v in G[f"{cid}/dims"])


def q_of(cid):
    rev, a, b, _, r, r_add = dims(cid)
    return min(b if rev else a, r + r_add)


def seed(cid):
    return int(G[f"{cid}/seed"])


def factors(cid):
    """(U, S or None, Vt): fresh host copies"""
    return G[f"{cid}/U"].copy(), (G[f"{cid}/S"].copy() if f"{cid}/S" in G.files else None), G[f"{cid}/Vt"].copy()


def block(cid):
    """the Gaussian block the reference drew (case j: regenerated from its seed; the legacy stream is frozen)"""
    if f"{cid}/G" in G.files:
        return G[f"{cid}/G"].copy()
    rev, a, b, _, _, r_add = dims(cid)
    rs = np.random.RandomState(seed(cid))
    return rs.randn(r_add, b) if rev else rs.randn(a, r_add)


def cat(cid):
    rev, _, _, _, r, _ = dims(cid)
    U = G[f"{cid}/U"]
    return np.concatenate((U[:, :r].T, block(cid)), 0) if rev else np.concatenate((U[:, :r], block(cid)), 1)


def reference_product(cid):
    return G[f"{cid}/prod"] if f"{cid}/prod" in G.files else G[f"{cid}/s1"] @ G[f"{cid}/s2"]


def check_rank_and_product(cid, s1, s2):
    """exact rank and shapes, s1 s2 to 1e-11"""
    rev, a, b, _, _, _ = dims(cid)
    q = int(G[f"{cid}/rank"])
    assert q == q_of(cid)
    assert s1.shape == (a, q) and s2.shape == (q, b), (s1.shape, s2.shape)
    close(s1 @ s2, reference_product(cid), RTOL)


def check_orthonormal(cid, s1, s2):
    """Gram error of the orthonormal factor, and cat's distance from its range"""
    rev = dims(cid)[0]
    Q = s2.T if rev else s1            # orthonormal columns
    C = cat(cid).T if rev else cat(cid)
    assert np.max(np.abs(Q.T @ Q - np.eye(Q.shape[1]))) <= ORTH_TOL
    assert np.linalg.norm(C - Q @ (Q.T @ C)) <= ORTH_TOL * np.linalg.norm(C)


def check_factors(cid, s1, s2):
    """s1 and s2 elementwise against the reference's, where cat is well conditioned"""
    if float(G[f"{cid}/cond"]) < COND_MAX:
        close(s1, G[f"{cid}/s1"], RTOL)
        close(s2, G[f"{cid}/s2"], RTOL)


def check_same_split(cid, s1, s2, c1, c2):
    """(s1, s2) against another path's (c1, c2) on the same operands: equal shapes, equal values to 1e-11 --
    in the backward direction up to the sign of each row of Q and of the matching column of s1, the one
    freedom between `dev.rq`'s RQ and LAPACK's (module docstring); the product to 1e-11 either way"""
    rev = dims(cid)[0]
    assert s1.shape == c1.shape and s2.shape == c2.shape
    Q, Qc = (s2, c2) if rev else (s1.T, c1.T)          # orthonormal rows
    d = np.sign(np.sum(Q * Qc, axis=1))
    assert np.all(np.abs(d) == 1.0)
    if not rev:
        assert np.all(d == 1.0), d
    close(s1 * d[None, :], c1, RTOL)
    close(d[:, None] * s2, c2, RTOL)
    close(s1 @ s2, c1 @ c2, RTOL)


def public(E, T, cid, info=None):
    """The case through the path's own callers, NumPy's global stream seeded as the reference's was: the cases
    of SPLIT through `tt_eig._split` on the SVD's factors (the truncation keeps r: every singular value is far
    above the threshold and max_rank = r), the others through `tt_ops.add_kick_rank` on U[:, :r] and
    diag(S[:r]) Vt[:r].  Returns (s1 (a, q), s2 (q, b)) on the host; `info`, a dict, receives the launches the
    call took (without the uploads before it and the reads after it)."""
    D = T.D
    count = (lambda: D.lib.ttk_launch_count()) if info is not None else (lambda: 0)
    rev, a, b, _, r, r_add = dims(cid)
    U, S, Vt = factors(cid)
    np.random.seed(seed(cid))
    if cid in SPLIT:
        pre = (D.from_numpy(U), D.from_numpy(S), D.from_numpy(Vt), S.copy())
        l0 = count()
        s1, s2 = E._split(None, (a, 1, b, 1), 1e-30, r, bool(rev), pre=pre)
        if info is not None:
            info["launches"] = count() - l0
        return D.read(s1).reshape(a, -1), D.read(s2).reshape(-1, b)
    assert not rev
    v = Vt[:r] if S is None else S[:r, None] * Vt[:r]
    u, v = D.from_numpy(U[:, :r]), D.from_numpy(v)
    l0 = count()
    s1, s2, q = T.add_kick_rank(u, v, r_add)
    if info is not None:
        info["launches"] = count() - l0
    assert q == s1.shape[1] == s2.shape[0]
    return D.read(s1), D.read(s2)


def state_after(cid):
    """NumPy's MT19937 state after the composed path's one draw from the case's seed"""
    rs = np.random.RandomState(seed(cid))
    rev, a, b, _, _, r_add = dims(cid)
    rs.randn(r_add, b) if rev else rs.randn(a, r_add)
    return rs.get_state()


def same_state(x, y):
    return np.array_equal(x[1], y[1]) and tuple(x[2:]) == tuple(y[2:])
