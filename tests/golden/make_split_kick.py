"""Golden vectors of the reference's truncate-and-kick split (`_add_kick_rank` / `_add_kick_rank_rev`,
`src/tt_als.py:1041-1053`, as `_step_size_local_solve` calls them, `:1023-1037`), made by the reference itself
(build container only):

    OPENBLAS_NUM_THREADS=1 python tests/golden/make_split_kick.py

Writes `tests/golden/split_kick.npz` (data only).  Per case: the truncation SVD's factors `U`, `S`, `Vt` (the
thin SVD of a unit-norm Gaussian matrix, or of its transpose for rev = 1; case f: two plain Gaussian factors
and no S; case z: S zeroed), `r`, `r_add`, the seed NumPy's global stream had, the Gaussian block the
reference drew from it (re-drawn from the same seed), the reference's two outputs, its rank, and `cond`, the
2-norm condition number of the concatenated matrix.  Case j's block and factors are past what a test needs
to hold: its block is regenerated from the seed and only the product of its outputs is stored.

A QR factor moves with the conditioning of its matrix, so every case also records `noise`: the largest
relative max-abs change of s1, of s2 and of s1 s2 over 5 reruns of the unmodified reference, from the same
seed, on the factors with every entry multiplied by 1 + 1.1e-16 N(0, 1).  tests/split_kick_cases.py admits a
case to value checks only if 50 x noise <= 1e-11.
"""
import os
import sys

os.environ.setdefault("OPENBLAS_NUM_THREADS", "1")
os.environ.setdefault("OMP_NUM_THREADS", "1")

import numpy as np  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from make_golden import _import_reference  # noqa: E402

# id: (rev, a, b, p, r, r_add, S: "given" | None | "zero")
CASES = {
    "a": (0, 8, 8, 8, 3, 4, "given"),      # q = 7
    "b": (0, 6, 10, 6, 4, 4, "given"),     # q = 6: more columns than rows
    "c": (1, 8, 8, 8, 3, 4, "given"),      # q = 7
    "d": (1, 10, 6, 6, 4, 4, "given"),     # q = 6
    "e": (0, 70, 12, 12, 5, 4, "given"),   # rows past one wave's stride
    "f": (0, 8, 5, 3, 3, 2, None),         # tt_ops.add_kick_rank(u, v)
    "g": (0, 2, 2, 2, 1, 4, "given"),      # q = 2
    "h": (1, 6, 66, 6, 6, 4, "given"),     # r = p
    "z": (0, 8, 8, 8, 3, 4, "zero"),       # the zero solution
    "j": (0, 512, 16, 16, 16, 96, "given"),  # does not fit LDS
}
SEED0 = 4100
NOISE_RUNS, NOISE_EPS = 5, 1.1e-16


def make_input(cid, rng):
    rev, a, b, p, r, r_add, kind = CASES[cid]
    if kind is None:
        return rng.standard_normal((a, p)), None, rng.standard_normal((p, b))
    mat = rng.standard_normal((b, a) if rev else (a, b))
    U, S, Vt = np.linalg.svd(mat / np.linalg.norm(mat), full_matrices=False)
    assert S.shape[0] == p
    return U, (np.zeros_like(S) if kind == "zero" else S), Vt


def reference(rals, cid, U, S, Vt, seed):
    """(s1, s2, rank) of the reference's own call on the factors, NumPy's global stream seeded"""
    rev, _, _, _, r, r_add, _ = CASES[cid]
    v = Vt if S is None else S.reshape(-1, 1) * Vt
    np.random.seed(seed)
    if rev:
        return rals._add_kick_rank_rev(v[:r].T.copy(), U[:, :r].T.copy(), r_add)
    return rals._add_kick_rank(U[:, :r].copy(), v[:r].copy(), r_add)


def block(cid, seed):
    """the Gaussian block the reference draws from `seed`"""
    rev, a, b, _, _, r_add, _ = CASES[cid]
    np.random.seed(seed)
    return np.random.randn(r_add, b) if rev else np.random.randn(a, r_add)


def _rel(x, ref):
    return float(np.max(np.abs(x - ref)) / max(np.max(np.abs(ref)), 1e-300))


def main():
    _, rals, _ = _import_reference(True)
    rng = np.random.default_rng(20261022)
    nrng = np.random.default_rng(20261023)   # the perturbations: a stream of their own
    out = {}
    for n, cid in enumerate(CASES):
        rev, a, b, p, r, r_add, kind = CASES[cid]
        seed = SEED0 + n
        U, S, Vt = make_input(cid, rng)
        G = block(cid, seed)
        s1, s2, rank = reference(rals, cid, U, S, Vt, seed)
        cat = np.concatenate((U[:, :r].T, G), 0) if rev else np.concatenate((U[:, :r], G), 1)
        out[f"{cid}/dims"] = np.array([rev, a, b, p, r, r_add], dtype=np.int64)
        out[f"{cid}/seed"] = np.array(seed)
        out[f"{cid}/U"], out[f"{cid}/Vt"] = U, Vt
        if S is not None:
            out[f"{cid}/S"] = S
        out[f"{cid}/rank"] = np.array(rank)
        out[f"{cid}/cond"] = np.array(np.linalg.cond(cat))
        if cid == "j":
            out[f"{cid}/prod"] = s1 @ s2
        else:
            out[f"{cid}/G"], out[f"{cid}/s1"], out[f"{cid}/s2"] = G, s1, s2
        noise = 0.0
        for _ in range(NOISE_RUNS):
            pert = [None if x is None else x * (1.0 + NOISE_EPS * nrng.standard_normal(x.shape)) for x in (U, S, Vt)]
            t1, t2, _ = reference(rals, cid, *pert, seed)
            noise = max(noise, _rel(t1, s1), _rel(t2, s2), _rel(t1 @ t2, s1 @ s2))
        out[f"{cid}/noise"] = np.array(noise)
        print(f"{cid}: rank {rank} cond {float(out[f'{cid}/cond']):.3g} noise {noise:.3g}")
    path = os.path.join(HERE, "split_kick.npz")
    np.savez_compressed(path, **out)
    print("wrote", len(out), "arrays,", os.path.getsize(path), "bytes, to split_kick.npz")


if __name__ == "__main__":
    main()
