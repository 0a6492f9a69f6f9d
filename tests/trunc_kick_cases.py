"""Shared by tests/test_host_trunc_kick.py (CPU, emulated libttk) and tests/test_gpu_trunc_kick.py (MI355X): the
fixtures of tests/golden/trunc_kick.npz (made by tests/golden/make_trunc_kick.py with the reference's own gesvd
call, `prune_singular_vals` and `_add_kick_rank` / `_add_kick_rank_rev`, the steps of src/tt_als.py:1022-1037)
and the checks both files apply to a result.

Tolerances.  The kept rank r and the output rank q are compared exactly, which is only fair where no decision is
a near tie: every tail sum sc[j] of the recorded spectrum must lie outside [eps^2 / 3, 3 eps^2] (the margin of
tests/round_one_cases.py: a Jacobi singular value differs from gesvd's by rounding, so any factor clearly above 1
keeps the decision).  The product s1 s2 does not depend on a gauge: 1e-11 relative max-abs (`tt_cases.close`).
Neither do s1 and s2 themselves: flipping a column of U[:, :r] leaves every Householder reflector unchanged and
flips a column of R, which the matching row of diag(S) Vt cancels, and the spectra here are separated (ratio
0.3), so they are compared elementwise to the same 1e-11.  The fixture records per case `noise`, the largest
change of the reference's own s1, s2 and product over 5 reruns with every entry of M moved by 1.1e-16 relative;
50 x noise <= 1e-11 must hold for EVERY case (50: the parity policy's multiple).  Both conditions
are asserted here on import, so a regenerated fixture cannot bring in an ill-posed case.  S is held to 1e-11 of
S[0].  The orthonormal factor's Gram matrix and the distance of the concatenated matrix from its range are held
to 1e-12, the bounds of tests/split_kick_cases.py."""
import numpy as np

from tests.tt_cases import close, load  # noqa: F401  (re-exported)

G = load("trunc_kick.npz").G

ALL = ("a", "c", "b", "d", "e", "f", "g", "m", "h", "k", "z", "j")
FIT = tuple(c for c in ALL if c != "j")          # cases whose working set fits one workgroup's LDS
VALUE = tuple(c for c in FIT if c != "z")        # cases with reference outputs in the fixture
CALLERS = VALUE + ("j",)                         # cases the callers are held to the reference on
R_ADD = 4
RTOL = 1e-11
ORTH_TOL = 1e-12
NOISE_MULTIPLE = 50
MARGIN = 3.0
LDS_MAX = 160 * 1024


def dims(cid):
    """(rev, a, b, max_rank, r, q)"""
    return tuple(int(v) for v in G[f"{cid}/dims"])


def trunc_tol(cid):
    return float(G[f"{cid}/trunc_tol"])


def seed(cid):
    return int(G[f"{cid}/seed"])


def tail_sums(cid):
    """sc[j] = sum_{t >= j} S[t]^2 in np.cumsum's order, as `prune_singular_vals` forms them"""
    return np.cumsum(np.abs(G[f"{cid}/S"][::-1]) ** 2)[::-1]


for _c in ALL:
    assert NOISE_MULTIPLE * float(G[f"{_c}/noise"]) <= RTOL, (_c, float(G[f"{_c}/noise"]))
    if f"{_c}/S" in G.files:
        _e2 = trunc_tol(_c) ** 2
        assert all(not (_e2 / MARGIN <= v <= MARGIN * _e2) for v in tail_sums(_c)), (_c, _e2, tail_sums(_c))


def matrix(cid):
    """the two-site solution M (a x b): a fresh host copy"""
    return G[f"{cid}/M"].copy()


def block(cid):
    """the Gaussian block the reference drew (case j: regenerated from its seed; the legacy stream is frozen)"""
    if f"{cid}/G" in G.files:
        return G[f"{cid}/G"].copy()
    rev, a, b = dims(cid)[:3]
    rs = np.random.RandomState(seed(cid))
    return rs.randn(R_ADD, b) if rev else rs.randn(a, R_ADD)


def qmax_of(cid):
    rev, a, b, max_rank, _, _ = dims(cid)
    return min(b if rev else a, min(a, b, max_rank) + R_ADD)


def lds_args(cid):
    """(rev, a, b, r_add, max_rank): `ttk_trunc_kick_lds`' arguments"""
    rev, a, b, max_rank, _, _ = dims(cid)
    return rev, a, b, R_ADD, max_rank


_CAT = {}


def cat(cid):
    """[U[:, :r] | G] (rev 0, a x (r + 4)) or [U[:, :r]^T ; G] (rev 1, (r + 4) x b) of the fixture's M: only its
    range enters a check, so NumPy's SVD serves"""
    if cid not in _CAT:
        rev, _, _, _, r, _ = dims(cid)
        M = G[f"{cid}/M"]
        U = np.linalg.svd(M.T if rev else M, full_matrices=False)[0][:, :r]
        _CAT[cid] = np.concatenate((U.T, block(cid)), 0) if rev else np.concatenate((U, block(cid)), 1)
    return _CAT[cid]


def reference_product(cid):
    return G[f"{cid}/prod"] if f"{cid}/prod" in G.files else G[f"{cid}/s1"] @ G[f"{cid}/s2"]


def check_rank_and_product(cid, s1, s2, sign=1.0):
    """exact output rank and shapes, s1 s2 to 1e-11 (`sign`: of the solution the split was given)"""
    rev, a, b, _, _, q = dims(cid)
    assert s1.shape == (a, q) and s2.shape == (q, b), (s1.shape, s2.shape)
    close(sign * (s1 @ s2), reference_product(cid), RTOL)


def check_orthonormal(cid, s1, s2):
    """Gram error of the orthonormal factor, and cat's distance from its range"""
    rev = dims(cid)[0]
    Q = s2.T if rev else s1            # orthonormal columns
    C = cat(cid).T if rev else cat(cid)
    assert np.max(np.abs(Q.T @ Q - np.eye(Q.shape[1]))) <= ORTH_TOL
    assert np.linalg.norm(C - Q @ (Q.T @ C)) <= ORTH_TOL * np.linalg.norm(C)


def check_factors(cid, s1, s2):
    """s1 and s2 elementwise against the reference's"""
    close(s1, G[f"{cid}/s1"], RTOL)
    close(s2, G[f"{cid}/s2"], RTOL)


def shape4(cid):
    _, a, b, _, _, _ = dims(cid)
    return (a, 1, b, 1)


def split(E, T, cid, info=None):
    """The case through `tt_eig._split` on the solution itself (no SVD handed in), NumPy's global stream seeded
    as the reference's was.  Returns (s1 (a, q), s2 (q, b)) on the host; `info`, a dict, receives the launches
    and host waits the call took (without the upload before it and the reads after it)."""
    D = T.D
    rev, a, b, max_rank, _, _ = dims(cid)
    sol = D.from_numpy(matrix(cid))
    D.read(sol)
    np.random.seed(seed(cid))
    l0, y0 = _counts(D, info)
    s1, s2 = E._split(sol, shape4(cid), trunc_tol(cid), max_rank, bool(rev))
    _record(D, info, l0, y0)
    return D.read(s1).reshape(a, -1), D.read(s2).reshape(-1, b)


def dense_tail(E, T, cid, negative, info=None):
    """The case through `tt_eig._dense_two_site`, the dense branch of `_step_size_local_solve` from the assembled
    pencil on, with a pencil whose solution is +-vec(M): A = I and D = -c v v^T, so that A / step + D at step 1
    has the smallest eigenpair (1 - c, +-v).  c = 0.5: ev >= 0, the speculative tail is taken.  c = 2 (`negative`):
    ev < 0, and the largest pair of -D x = lam A x is (2, +-v): the split is redone on that branch's solution.
    Returns (s1, s2, sign, step) with sign that of the solution the solver chose."""
    D = T.D
    rev, a, b, max_rank, _, _ = dims(cid)
    v = matrix(cid).reshape(-1)
    m = v.size
    Am = D.from_numpy(np.eye(m))
    Dm = D.from_numpy(-(2.0 if negative else 0.5) * np.outer(v, v))
    prev = D.from_numpy(np.full(m, 1.0 / np.sqrt(m)))
    D.read(prev)
    np.random.seed(seed(cid))
    l0, y0 = _counts(D, info)
    s1, s2, step, _ = E._dense_two_site(prev, Am, Dm, 1.0, 1e-8, shape4(cid), trunc_tol(cid), max_rank, bool(rev))
    _record(D, info, l0, y0)
    s1, s2 = D.read(s1).reshape(a, -1), D.read(s2).reshape(-1, b)
    sign = 1.0 if np.sum((s1 @ s2) * reference_product(cid)) >= 0 else -1.0
    return s1, s2, sign, step


def _counts(D, info):
    if info is None:
        return 0, 0
    return D.lib.ttk_launch_count(), D.lib.ttk_sync_count()


def _record(D, info, l0, y0):
    if info is not None:
        info["launches"] = D.lib.ttk_launch_count() - l0
        info["waits"] = D.lib.ttk_sync_count() - y0


def state_after(cid):
    """NumPy's MT19937 state after the reference's one draw from the case's seed"""
    rs = np.random.RandomState(seed(cid))
    rev, a, b = dims(cid)[:3]
    rs.randn(R_ADD, b) if rev else rs.randn(a, R_ADD)
    return rs.get_state()


def same_state(x, y):
    return np.array_equal(x[1], y[1]) and tuple(x[2:]) == tuple(y[2:])
