"""Golden vectors of the tail of the reference's two-site step-size local solve (`_step_size_local_solve`,
`src/tt_als.py:1022-1037`: normalise, gesvd, `prune_singular_vals`, `_add_kick_rank` / `_add_kick_rank_rev`), made
by the reference's own functions (build container only):

    OPENBLAS_NUM_THREADS=1 python tests/golden/make_trunc_kick.py

Writes `tests/golden/trunc_kick.npz` (data only).  Per case: the two-site solution `M` (a x b; U diag(0.3^j) V^T
with random orthonormal U and V, scaled to unit norm; case z: zeros), `trunc_tol` (its square the geometric mean
of the two tail sums on either side of the intended rank, so that no rank decision is a near tie), `max_rank`,
the seed NumPy's global stream had, the Gaussian block `G` the reference drew from it (re-drawn from the same
seed), the reference's two outputs `s1`, `s2`, the singular values `S`, the kept rank `r` and the output rank
`q`.  Case j's outputs are past what a test needs to hold: only their product is stored and its block is
regenerated from the seed.  Case z has no reference (it divides by a zero norm): the fixture holds its inputs,
r = 1 (`prune_singular_vals` on a zero spectrum) and q.

A singular vector moves with the gaps of the spectrum and a QR factor with the conditioning of its matrix, so
every case also records `noise`: the largest relative max-abs change of s1, of s2 and of s1 s2 over 5 reruns of
the same steps, from the same seed, with every entry of M multiplied by 1 + 1.1e-16 N(0, 1).
tests/trunc_kick_cases.py asserts 50 x noise <= 1e-11 for every case.
"""
import os
import sys

os.environ.setdefault("OPENBLAS_NUM_THREADS", "1")
os.environ.setdefault("OMP_NUM_THREADS", "1")

import numpy as np  # noqa: E402
import scipy.linalg  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from make_golden import _import_reference  # noqa: E402

# id: (rev, a, b, intended rank or None, max_rank, trunc_tol or None: from the intended rank)
CASES = {
    "a": (0, 8, 8, 3, 32, None),       # plain, q = 7
    "c": (1, 8, 8, 3, 32, None),
    "b": (0, 6, 10, 4, 32, None),      # q capped by the rows (6): more columns than rows in the QR
    "d": (1, 10, 6, 4, 32, None),
    "e": (0, 70, 12, 5, 32, None),     # rows past one wave's stride; the SVD on the transpose
    "f": (1, 12, 66, 5, 32, None),
    "g": (0, 2, 2, 1, 32, None),       # q = 2, p = 2: a Jacobi with one pair
    "m": (0, 16, 16, 6, 4, None),      # the pruning keeps 6, max_rank 4 decides
    "h": (0, 8, 8, None, 32, 1e-30),   # r = p, q = 8
    "k": (1, 32, 32, 8, 32, None),     # p = 32: pairs across 16 waves
    "z": (0, 8, 8, 3, 32, None),       # the zero matrix (threshold of case a's spectrum)
    "j": (0, 512, 64, 5, 32, None),    # does not fit one workgroup
}
R_ADD = 4
DECAY = 0.3
SEED0 = 4300
NOISE_RUNS, NOISE_EPS = 5, 1.1e-16


def make_input(cid, rng):
    """(M, trunc_tol)"""
    rev, a, b, want, max_rank, tol = CASES[cid]
    p = min(a, b)
    U, _ = np.linalg.qr(rng.standard_normal((a, p)))
    V, _ = np.linalg.qr(rng.standard_normal((b, p)))
    s = DECAY ** np.arange(p)
    M = (U * s) @ V.T
    M /= np.linalg.norm(M)
    if tol is None:
        sc = np.cumsum((s / np.linalg.norm(s))[::-1] ** 2)[::-1]
        tol = float(np.sqrt(np.sqrt(sc[want] * sc[want - 1])))
    return (np.zeros_like(M) if cid == "z" else M), tol


def reference(rals, cid, M, tol, seed):
    """(s1, s2, q, r, S): the steps of src/tt_als.py:1022-1037 on M, NumPy's global stream seeded"""
    rev, a, b, _, max_rank, _ = CASES[cid]
    sol = M / np.linalg.norm(M)
    np.random.seed(seed)
    if rev:
        u, s, v = scipy.linalg.svd(sol.T.copy(), full_matrices=False, check_finite=False, lapack_driver="gesvd")
        v = s.reshape(-1, 1) * v
        r = min(rals.prune_singular_vals(s, tol), max_rank)
        s1, s2, q = rals._add_kick_rank_rev(v[:r].T, u[:, :r].T, R_ADD)
    else:
        u, s, v = scipy.linalg.svd(sol.copy(), full_matrices=False, check_finite=False, lapack_driver="gesvd")
        r = min(rals.prune_singular_vals(s, tol), max_rank)
        s1, s2, q = rals._add_kick_rank(u[:, :r], s.reshape(-1, 1)[:r] * v[:r], R_ADD)
    return s1, s2, int(q), int(r), s


def block(cid, seed):
    """the Gaussian block the reference draws from `seed`"""
    rev, a, b = CASES[cid][:3]
    np.random.seed(seed)
    return np.random.randn(R_ADD, b) if rev else np.random.randn(a, R_ADD)


def _rel(x, ref):
    return float(np.max(np.abs(x - ref)) / max(np.max(np.abs(ref)), 1e-300))


def main():
    _, rals, _ = _import_reference(True)
    rng = np.random.default_rng(20261024)
    nrng = np.random.default_rng(20261025)   # the perturbations: a stream of their own
    out = {}
    for n, cid in enumerate(CASES):
        rev, a, b, want, max_rank, _ = CASES[cid]
        seed = SEED0 + n
        M, tol = make_input(cid, rng)
        out[f"{cid}/M"] = M
        out[f"{cid}/trunc_tol"] = np.array(tol)
        out[f"{cid}/seed"] = np.array(seed)
        if cid == "z":
            r, q, noise = 1, min(a, 1 + R_ADD), 0.0
            out[f"{cid}/G"] = block(cid, seed)
        else:
            s1, s2, q, r, S = reference(rals, cid, M, tol, seed)
            out[f"{cid}/S"] = S
            if cid == "j":
                out[f"{cid}/prod"] = s1 @ s2
            else:
                out[f"{cid}/G"], out[f"{cid}/s1"], out[f"{cid}/s2"] = block(cid, seed), s1, s2
            noise = 0.0
            for _ in range(NOISE_RUNS):
                t1, t2, tq, tr, _ = reference(rals, cid, M * (1.0 + NOISE_EPS * nrng.standard_normal(M.shape)), tol, seed)
                assert (tq, tr) == (q, r)
                noise = max(noise, _rel(t1, s1), _rel(t2, s2), _rel(t1 @ t2, s1 @ s2))
        out[f"{cid}/dims"] = np.array([rev, a, b, max_rank, r, q], dtype=np.int64)
        out[f"{cid}/noise"] = np.array(noise)
        print(f"{cid}: r {r} q {q} trunc_tol {tol:.6g} noise {noise:.3g}")
    path = os.path.join(HERE, "trunc_kick.npz")
    np.savez_compressed(path, **out)
    print("wrote", len(out), "arrays,", os.path.getsize(path), "bytes, to trunc_kick.npz")


if __name__ == "__main__":
    main()
