"""Time `ttk_round` (tt_ops.tt_rank_reduce / _tail_rank_reduce on the native path) on trains shaped
like the IPM's: d cores of (r, 2, 2, r).  Prints per-call latency and a digest of the rounded cores,
so two libraries (TTK_LIB_PATH) can be compared for speed and for identical bits.

    python tools/bench_round.py [reps]

`one` times the one-launch path (`ttk_round_one`, TTIPM_ROUND_ONE=1) against `ttk_round` in the same run, at
the shapes of tools/bench_retract.py (d = 10, cores (r,2,2,R), ranks 8 / 12 / 24): `tt_rank_reduce` at eps = 1e-3
(the row of profiles/retract_d10.txt, which keeps the ranks at 8 and 12), and `tt_rank_reduce` and the tracked
`_tail_rank_reduce` at eps = 1e-2 ||T||, where the ranks drop.  The two paths alternate round by round so
that drift of the shared host hits both alike; each figure is a host clock around `reps` calls that end in
a device synchronise, per call; the table gives the median over the rounds and their min / max, next to
the launches and host waits per call and what was computed (ranks, distance from the input).

    python tools/bench_round.py one [reps] [rounds]

`sum` times the rounding of a weighted sum of trains, by the same method (host clock around `reps` calls ending
in a synchronise, the paths alternating round by round, median and min / max over the rounds, wrapper and read
included), at d = 10 with cores (r,2,2,R): a + alpha b at term ranks 4+4 and 6+6, and the symmetrised update
0.5 ((X + xs DX) + (X + xs DX)^T) at term ranks 3+3 (summed rank 12) and 6+6 (24).  Three paths in one run:
today's composition (`tt_scale` + `tt_add` (+ `tt_transpose`) + `ttk_round`), the same materialised sum into
`ttk_round_one`, and the fused `ttk_sum_round_one`, which never builds the sum.

    python tools/bench_round.py sum [reps] [rounds]

`prod` times the rounding of a product of two trains, by the same method, at d = 10: the matrix product of two
trains of cores (r,2,2,R) at ranks 3 x 3 and 4 x 4, an operator of cores (2,4,4,2) applied to a vector train of
ranks 4 and 6, and the Hadamard product of a rank-8 matrix train with a rank-1 mask, each at eps = 1e-2 of the
product's norm.  Three paths in one run: today's default (`ttk_zipup`: the product cores written, then
`ttk_round`), the same materialised product into `ttk_round_one`, and the fused `ttk_prod_round_one`, which
never builds the product.

    python tools/bench_round.py prod [reps] [rounds]

`affine` times the rounding of a weighted sum of trains and products, by the same method, at d = 10: the solve's
residual A x - b, an operator of cores (2,4,4,2) applied to a vector train of ranks 4 minus a train b of ranks 3, and
the 4-term Y update 0.5 (y - P y) + 0.5 (y - P y)^T on a flat train y of ranks 4 (middle 4 = (2,2)) with an operator
P of ranks 2, each at eps = 1e-2 of the operand's norm with the products formed at 1e-12.  Three paths in one run:
today's default (`ttk_zipup`, `tt_sub` / `tt_add`, `ttk_round`), the two sibling switches on (`ttk_prod_round_one`,
then `ttk_sum_round_one`), and the fused `ttk_affine_round_one`, which builds neither a product nor the sum and
also returns the squared norm.

    python tools/bench_round.py affine [reps] [rounds]

`kick` times the truncate-and-kick split that ends a two-site local solve of the step-size eigen-ALS
(`tt_eig._split` on the truncation SVD's factors, the SVD itself outside the clock), by the same method, at
(a, b, r) = (8, 8, 4), (16, 16, 8) and (64, 64, 28) in both sweep directions, kick rank 4: today's composition
(scaling, two copies, `ttk_qr`, the product, contiguous copies; the backward split also `dev.rq`'s einsums)
against the one call `ttk_split_kick` (TTIPM_SPLIT_KICK=1).  Both paths draw the same Gaussian block on the host
and upload it inside the clock.

    python tools/bench_round.py kick [reps] [rounds]

`trunc` times the whole tail of a two-site local solve (`tt_eig._two_site_tail`: normalise, truncation SVD, rank
decision, kicked QR / RQ, product), by the same method, at (a, b) = (8, 8), (16, 16) and (64, 64) in both sweep
directions, kick rank 4, on U diag(0.5^j) V^T with a threshold that keeps about half of the singular values.
Three paths alternate in one run: today's default (`normalized`, `ttk_svd` with its read, the host's rank rule,
the composed split), the same with TTIPM_SPLIT_KICK=1, and the one call `ttk_trunc_kick_read`
(TTIPM_TRUNC_KICK=1: one launch, its info read in the call).  Every path draws the same Gaussian block on the
host and uploads it inside the clock.

    python tools/bench_round.py trunc [reps] [rounds]

`many` times a group of independent roundings as one launch (`ttk_affine_round_many`, one workgroup per job, one
host read for the group: `tt_ops.tt_affine_rank_reduce_many` under TTIPM_AFFINE_ROUND_MANY=1) against the same
jobs as N `ttk_affine_round_one` calls in sequence on the same library (one launch and one host read each), by the
same method, at d = 10 with cores (r,2,2,R): 2, 3, 4 and 8 equal jobs (one plain train of ranks 8, 12 and 24 each,
eps = 1e-2 of its norm), and a mixed group shaped like a Newton step's blocks, two symmetrisations
0.5 M + 0.5 M^T and one plain train.  Every job's output bits are compared between the two paths.

    python tools/bench_round.py many [reps] [rounds]
"""
import hashlib
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from ttipm_amd import dev as D  # noqa: E402
from ttipm_amd import tt_ops as T  # noqa: E402


def train(rng, ranks):
    return [D.from_numpy(rng.standard_normal((ranks[k], 2, 2, ranks[k + 1])) * (0.5 ** np.arange(ranks[k + 1])))
            for k in range(len(ranks) - 1)]


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 200
    rng = np.random.default_rng(5)
    cases = {"d10_r8": [1] + [8] * 9 + [1], "d10_r16": [1, 4] + [16] * 7 + [4, 1], "d6_r32": [1, 4, 16, 32, 16, 4, 1]}
    h = hashlib.sha256()
    for name, ranks in cases.items():
        base = train(rng, ranks)
        for mode, eps in ((0, 1e-10), (0, 1e-3), (1, 1e-3)):
            def once():
                tt = list(base)
                return T.tt_rank_reduce(tt, eps) if mode == 0 else T._tail_rank_reduce(tt, eps)
            out = once()
            if mode == 1:
                out, tail = out
                h.update(np.float64(tail if tail is not None else np.nan).tobytes())
            for c in out:
                h.update(D.read(c).tobytes())
            for _ in range(10):
                once()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(reps):
                once()
            torch.cuda.synchronize()
            us = (time.perf_counter() - t0) / reps * 1e6
            print(f"{name:8s} mode {mode} eps {eps:g}: ranks {T.tt_ranks(out)}  {us:8.1f} us/call", flush=True)
    print("digest", h.hexdigest()[:16], flush=True)


def bench_one(d, r, eps_rel, tracked, reps, rounds):
    rng = np.random.default_rng(5)
    ranks = [1] + [r] * (d - 1) + [1]
    base = [D.from_numpy(rng.standard_normal((ranks[k], 2, 2, ranks[k + 1])) * (0.5 ** np.arange(ranks[k + 1])))
            for k in range(d)]
    lds = T.round_one_lds(base)
    assert lds >= 0
    eps = eps_rel * T.tt_norm(base) if eps_rel else 1e-3

    def call(switch):
        def f():
            T.ROUND_ONE = switch
            return T._tail_rank_reduce(list(base), eps)[0] if tracked else T.tt_rank_reduce(list(base), eps)
        return f

    what = (("ttk_round (the default)", call(False)), ("ttk_round_one", call(True)))
    ref = T.tt_to_tensor(base)
    info = {}
    for name, f in what:
        out = f()
        torch.cuda.synchronize()
        l0, s0 = D.lib.ttk_launch_count(), D.lib.ttk_sync_count()
        f()
        torch.cuda.synchronize()
        info[name] = (T.tt_ranks(out), D.lib.ttk_launch_count() - l0, D.lib.ttk_sync_count() - s0,
                      float(np.linalg.norm(T.tt_to_tensor(out) - ref) / np.linalg.norm(ref)))
        for _ in range(20):  # warm-up of every shape the timed window uses
            f()
    torch.cuda.synchronize()
    times = {name: [] for name, _ in what}
    for _ in range(rounds):
        for name, f in what:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(reps):
                f()
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t0) / reps * 1e6)
    T.ROUND_ONE = False
    fn = "_tail_rank_reduce" if tracked else "tt_rank_reduce"
    print(f"d={d} ranks {r} cores (r,2,2,R) {fn} eps {eps:g}; LDS {lds} bytes; {reps} calls x {rounds} rounds, "
          f"us per call", flush=True)
    for name, _ in what:
        t = np.array(times[name])
        rk, nl, ns, err = info[name]
        print(f"{name:24s} median {np.median(t):8.1f}  min {t.min():8.1f}  max {t.max():8.1f}  launches {nl:3d}  "
              f"host waits {ns:2d}  |out - in|/|in| {err:.2e}  ranks {rk}", flush=True)
    old, new = (np.array(times[name]) for name, _ in what)
    spread = max(old.max() - old.min(), new.max() - new.min())
    gap = float(np.median(old) - np.median(new))
    print(f"ttk_round_one: {np.median(old) / np.median(new):.2f}x ttk_round (medians {gap:.1f} us apart, min-max "
          f"spread {spread:.1f} us: {'beyond' if abs(gap) > spread else 'within'} the spread)\n", flush=True)


def main_one(argv):
    reps = int(argv[0]) if argv else 100
    rounds = int(argv[1]) if len(argv) > 1 else 7
    assert torch.cuda.is_available(), "bench_round needs an MI355X"
    for r in (8, 12, 24):
        for eps_rel, tracked in ((0, False), (1e-2, False), (1e-2, True)):
            bench_one(10, r, eps_rel, tracked, reps, rounds)


def bench_sum(d, r, symmetrise, reps, rounds):
    rng = np.random.default_rng(5)
    ranks = [1] + [r] * (d - 1) + [1]
    A, B = train(rng, ranks), train(rng, ranks)
    alpha = 0.37
    w = float(np.float32(alpha))
    if symmetrise:
        terms, coeffs, flags = [A, B, A, B], [0.5, 0.5 * w, 0.5, 0.5 * w], [False, False, True, True]
    else:
        terms, coeffs, flags = [A, B], [1.0, w], [False, False]
    lds = T.sum_round_one_lds(terms, flags)
    assert lds >= 0
    eps = 1e-2 * T.tt_norm(A)

    def composed(one):
        def f():
            T.ROUND_ONE, T.SUM_ROUND_ONE = one, False
            M = T.tt_add(A, T.tt_scale(alpha, B))
            if symmetrise:
                M = T.tt_scale(0.5, T.tt_add(M, T.tt_transpose(M)))
            return T.tt_rank_reduce(M, eps)
        return f

    def fused():
        T.ROUND_ONE, T.SUM_ROUND_ONE = False, True
        return T.tt_sum_rank_reduce(terms, coeffs, flags, eps)

    what = (("composed + ttk_round (the default)", composed(False)), ("composed + ttk_round_one", composed(True)),
            ("ttk_sum_round_one", fused))
    info = {}
    ref = None
    for name, f in what:
        out = f()
        torch.cuda.synchronize()
        l0, s0 = D.lib.ttk_launch_count(), D.lib.ttk_sync_count()
        f()
        torch.cuda.synchronize()
        nl, ns = D.lib.ttk_launch_count() - l0, D.lib.ttk_sync_count() - s0
        dense = T.tt_to_tensor(out)
        ref = dense if ref is None else ref
        info[name] = (T.tt_ranks(out), nl, ns, float(np.linalg.norm(dense - ref) / np.linalg.norm(ref)))
        for _ in range(20):  # warm-up of every shape the timed window uses
            f()
    torch.cuda.synchronize()
    times = {name: [] for name, _ in what}
    for _ in range(rounds):
        for name, f in what:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(reps):
                f()
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t0) / reps * 1e6)
    T.ROUND_ONE = T.SUM_ROUND_ONE = False
    kind = "symmetrised update, 4 terms" if symmetrise else "a + alpha b, 2 terms"
    print(f"d={d} {kind}, term ranks {r}+{r} (summed {len(terms) * r}), cores (r,2,2,R), eps {eps:g}; LDS {lds} bytes; "
          f"{reps} calls x {rounds} rounds, us per call", flush=True)
    for name, _ in what:
        t = np.array(times[name])
        rk, nl, ns, err = info[name]
        print(f"{name:36s} median {np.median(t):8.1f}  min {t.min():8.1f}  max {t.max():8.1f}  launches {nl:3d}  "
              f"host waits {ns:2d}  |out - default|/|default| {err:.2e}  ranks {rk}", flush=True)
    _, mat, new = (np.array(times[name]) for name, _ in what)
    spread = max(mat.max() - mat.min(), new.max() - new.min())
    gap = float(np.median(mat) - np.median(new))
    print(f"ttk_sum_round_one: {np.median(mat) / np.median(new):.2f}x composed + ttk_round_one (medians {gap:.1f} us "
          f"apart, min-max spread {spread:.1f} us: {'beyond' if abs(gap) > spread else 'within'} the spread)\n",
          flush=True)


def main_sum(argv):
    reps = int(argv[0]) if argv else 100
    rounds = int(argv[1]) if len(argv) > 1 else 7
    assert torch.cuda.is_available(), "bench_round needs an MI355X"
    for r, symmetrise in ((4, False), (6, False), (3, True), (6, True)):
        bench_sum(10, r, symmetrise, reps, rounds)


def bench_prod(kind, d, ra, rb, reps, rounds):
    rng = np.random.default_rng(5)

    def cores(r, mid):
        rk = [1] + [r] * (d - 1) + [1]
        return [D.from_numpy(rng.standard_normal((rk[k], *mid, rk[k + 1])) * (0.5 ** np.arange(rk[k + 1])))
                for k in range(d)]

    if kind == 0:
        A, B, what_is = cores(ra, (4, 4)), cores(rb, (4,)), "operator (r,4,4,R) x vector (r,4,R)"
    else:
        A, B = cores(ra, (2, 2)), cores(rb, (2, 2))
        what_is = "matrix product of (r,2,2,R) trains" if kind == 1 else "Hadamard product of (r,2,2,R) trains"
    fn = (T.tt_fast_matrix_vec_mul, T.tt_fast_mat_mat_mul, None, T.tt_fast_hadamard)[kind]
    lds = T.prod_round_one_lds(kind, A, B)
    assert lds >= 0
    T.ROUND_ONE = T.PROD_ROUND_ONE = False
    eps = 1e-2 * T.tt_norm(fn(A, B, 0.0))

    def default():
        T.ROUND_ONE = T.PROD_ROUND_ONE = False
        return fn(A, B, eps)

    def materialised():
        T.ROUND_ONE, T.PROD_ROUND_ONE = True, False
        return T.tt_rank_reduce(fn(A, B, 0.0), eps)

    def fused():
        T.ROUND_ONE, T.PROD_ROUND_ONE = False, True
        return fn(A, B, eps)

    what = (("ttk_zipup (the default)", default), ("product + ttk_round_one", materialised),
            ("ttk_prod_round_one", fused))
    info = {}
    ref = None
    for name, f in what:
        out = f()
        torch.cuda.synchronize()
        l0, s0 = D.lib.ttk_launch_count(), D.lib.ttk_sync_count()
        f()
        torch.cuda.synchronize()
        nl, ns = D.lib.ttk_launch_count() - l0, D.lib.ttk_sync_count() - s0
        dense = T.tt_to_tensor(out)
        ref = dense if ref is None else ref
        info[name] = (T.tt_ranks(out), nl, ns, float(np.linalg.norm(dense - ref) / np.linalg.norm(ref)))
        for _ in range(20):  # warm-up of every shape the timed window uses
            f()
    torch.cuda.synchronize()
    times = {name: [] for name, _ in what}
    for _ in range(rounds):
        for name, f in what:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(reps):
                f()
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t0) / reps * 1e6)
    T.ROUND_ONE = T.PROD_ROUND_ONE = False
    print(f"d={d} {what_is}, ranks {ra} x {rb} (product {ra * rb}), eps {eps:g}; LDS {lds} bytes; "
          f"{reps} calls x {rounds} rounds, us per call", flush=True)
    for name, _ in what:
        t = np.array(times[name])
        rk, nl, ns, err = info[name]
        print(f"{name:26s} median {np.median(t):8.1f}  min {t.min():8.1f}  max {t.max():8.1f}  launches {nl:3d}  "
              f"host waits {ns:2d}  |out - default|/|default| {err:.2e}  ranks {rk}", flush=True)
    old, mat, new = (np.array(times[name]) for name, _ in what)
    for other, t in (("ttk_zipup", old), ("product + ttk_round_one", mat)):
        spread = max(t.max() - t.min(), new.max() - new.min())
        gap = float(np.median(t) - np.median(new))
        print(f"ttk_prod_round_one: {np.median(t) / np.median(new):.2f}x {other} (medians {gap:.1f} us apart, min-max "
              f"spread {spread:.1f} us: {'beyond' if abs(gap) > spread else 'within'} the spread)", flush=True)
    print(flush=True)


def main_prod(argv):
    reps = int(argv[0]) if argv else 100
    rounds = int(argv[1]) if len(argv) > 1 else 7
    assert torch.cuda.is_available(), "bench_round needs an MI355X"
    for kind, ra, rb in ((1, 3, 3), (1, 4, 4), (0, 2, 4), (0, 2, 6), (3, 8, 1)):
        bench_prod(kind, 10, ra, rb, reps, rounds)


def bench_affine(update, d, reps, rounds):
    rng = np.random.default_rng(5)

    def cores(r, mid):
        rk = [1] + [r] * (d - 1) + [1]
        return [D.from_numpy(rng.standard_normal((rk[k], *mid, rk[k + 1])) * (0.5 ** np.arange(rk[k + 1])))
                for k in range(d)]

    A, x, b = cores(2, (4, 4)), cores(4, (4,)), cores(3, (4,))
    small = 1e-12

    def switches(prod, summ, affine):
        T.ROUND_ONE, T.PROD_ROUND_ONE, T.SUM_ROUND_ONE, T.AFFINE_ROUND_ONE = False, prod, summ, affine

    if update:
        Ax = (0, A, x)
        terms, mids = [(0.5, x), (-0.5, Ax), (0.5, x, True), (-0.5, Ax, True)], (2, 2)
        what_is = "Y update 0.5 (y - P y) + 0.5 (y - P y)^T, P ranks 2, y ranks 4 (summed 24)"
    else:
        terms, mids = [(1.0, (0, A, x)), (-1.0, b)], None
        what_is = "A x - b, operator (r,4,4,R) ranks 2 x vector ranks 4 minus b ranks 3 (summed 11)"
    lds = T.affine_round_one_lds(terms, mids)
    assert lds >= 0
    switches(False, False, False)
    eps = 1e-2 * T.tt_norm(T._affine_composed(*T._affine_norm(terms, mids)))

    def default():
        switches(False, False, False)
        if not update:
            return T.tt_rank_reduce(T.tt_sub(T.tt_fast_matrix_vec_mul(A, x, small), b), eps)
        M = T.tt_reshape(T.tt_sub(x, T.tt_fast_matrix_vec_mul(A, x, small)), (2, 2))
        return T.tt_rank_reduce(T.tt_scale(0.5, T.tt_add(M, T.tt_transpose(M))), eps)

    def siblings():
        switches(True, True, False)
        Ax_ = T.tt_fast_matrix_vec_mul(A, x, small)
        if not update:
            return T.tt_sum_rank_reduce([Ax_, b], [1.0, -1.0], [False, False], eps)
        y2, p2 = T.tt_reshape(x, (2, 2)), T.tt_reshape(Ax_, (2, 2))
        return T.tt_sum_rank_reduce([y2, p2, y2, p2], [0.5, -0.5, 0.5, -0.5], [False, False, True, True], eps)

    def fused():
        switches(False, False, True)
        return T.tt_affine_rank_reduce(terms, eps, mids=mids)

    what = (("default (ttk_zipup, ttk_round)", default), ("ttk_prod_round_one, ttk_sum_round_one", siblings),
            ("ttk_affine_round_one", fused))
    info = {}
    ref = None
    for name, f in what:
        out = f()
        torch.cuda.synchronize()
        l0, s0 = D.lib.ttk_launch_count(), D.lib.ttk_sync_count()
        f()
        torch.cuda.synchronize()
        nl, ns = D.lib.ttk_launch_count() - l0, D.lib.ttk_sync_count() - s0
        dense = T.tt_to_tensor(out)
        ref = dense if ref is None else ref
        info[name] = (T.tt_ranks(out), nl, ns, float(np.linalg.norm(dense - ref) / np.linalg.norm(ref)))
        for _ in range(20):  # warm-up of every shape the timed window uses
            f()
    torch.cuda.synchronize()
    times = {name: [] for name, _ in what}
    for _ in range(rounds):
        for name, f in what:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(reps):
                f()
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t0) / reps * 1e6)
    switches(False, False, False)
    print(f"d={d} {what_is}, eps {eps:g}; LDS {lds} bytes; {reps} calls x {rounds} rounds, us per call", flush=True)
    for name, _ in what:
        t = np.array(times[name])
        rk, nl, ns, err = info[name]
        print(f"{name:38s} median {np.median(t):8.1f}  min {t.min():8.1f}  max {t.max():8.1f}  launches {nl:3d}  "
              f"host waits {ns:2d}  |out - default|/|default| {err:.2e}  ranks {rk}", flush=True)
    old, sib, new = (np.array(times[name]) for name, _ in what)
    for other, t in (("the default", old), ("the two sibling calls", sib)):
        spread = max(t.max() - t.min(), new.max() - new.min())
        gap = float(np.median(t) - np.median(new))
        print(f"ttk_affine_round_one: {np.median(t) / np.median(new):.2f}x {other} (medians {gap:.1f} us apart, min-max "
              f"spread {spread:.1f} us: {'beyond' if abs(gap) > spread else 'within'} the spread)", flush=True)
    print(flush=True)


def main_affine(argv):
    reps = int(argv[0]) if argv else 100
    rounds = int(argv[1]) if len(argv) > 1 else 7
    assert torch.cuda.is_available(), "bench_round needs an MI355X"
    for update in (False, True):
        bench_affine(update, 10, reps, rounds)


def bench_many(name, jobs, reps, rounds):
    """jobs: `tt_affine_rank_reduce_many`'s"""
    def switches(many):
        T.ROUND_ONE = T.PROD_ROUND_ONE = T.SUM_ROUND_ONE = False
        T.AFFINE_ROUND_ONE, T.AFFINE_ROUND_MANY = True, many

    def sequence():
        switches(False)
        return [T.tt_affine_rank_reduce(t, e, True, m) for t, e, _, m in jobs]

    def batch():
        switches(True)
        return [(tt, n2) for tt, _, n2 in T.tt_affine_rank_reduce_many(jobs)]

    lds = T.affine_round_many_lds(jobs)
    assert lds >= 0
    what = ((f"{len(jobs)} x ttk_affine_round_one", sequence), ("ttk_affine_round_many", batch))
    info, outs = {}, {}
    for label, f in what:
        outs[label] = f()
        torch.cuda.synchronize()
        l0, s0 = D.lib.ttk_launch_count(), D.lib.ttk_sync_count()
        f()
        torch.cuda.synchronize()
        info[label] = (D.lib.ttk_launch_count() - l0, D.lib.ttk_sync_count() - s0)
        for _ in range(20):  # warm-up of every shape the timed window uses
            f()
    (seq, bat) = (outs[label] for label, _ in what)
    same = all(n1 == n2 and len(a) == len(b) and all(torch.equal(x, y) for x, y in zip(a, b))
               for (a, n1), (b, n2) in zip(seq, bat))
    torch.cuda.synchronize()
    times = {label: [] for label, _ in what}
    for _ in range(rounds):
        for label, f in what:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(reps):
                f()
            torch.cuda.synchronize()
            times[label].append((time.perf_counter() - t0) / reps * 1e6)
    T.AFFINE_ROUND_ONE = T.AFFINE_ROUND_MANY = False
    print(f"d=10 {name}; LDS {lds} bytes; {reps} groups x {rounds} rounds, us per group; ranks out "
          f"{[max(T.tt_ranks(tt)) for tt, _ in bat]}; bits of the two paths {'equal' if same else 'DIFFER'}",
          flush=True)
    for label, _ in what:
        t = np.array(times[label])
        nl, ns = info[label]
        print(f"{label:28s} median {np.median(t):8.1f}  min {t.min():8.1f}  max {t.max():8.1f}  launches {nl:3d}  "
              f"host waits {ns:2d}", flush=True)
    old, new = (np.array(times[label]) for label, _ in what)
    spread = max(old.max() - old.min(), new.max() - new.min())
    gap = float(np.median(old) - np.median(new))
    print(f"ttk_affine_round_many: {np.median(old) / np.median(new):.2f}x the sequence (medians {gap:.1f} us apart, "
          f"min-max spread {spread:.1f} us: {'beyond' if abs(gap) > spread else 'within'} the spread); "
          f"{np.median(new) / (np.median(old) / len(jobs)):.2f}x one member's time\n", flush=True)


def main_many(argv):
    reps = int(argv[0]) if argv else 100
    rounds = int(argv[1]) if len(argv) > 1 else 7
    assert torch.cuda.is_available(), "bench_round needs an MI355X"
    rng = np.random.default_rng(5)
    for r in (8, 12, 24):
        ranks = [1] + [r] * 9 + [1]
        trains = [train(rng, ranks) for _ in range(8)]
        for n in (2, 3, 4, 8):
            jobs = [([(1.0, t)], 1e-2 * T.tt_norm(t), 0, None) for t in trains[:n]]
            bench_many(f"{n} equal jobs: one plain train of ranks {r} each, cores (r,2,2,R), eps 1e-2 |T|", jobs, reps,
                       rounds)
    for r in (4, 6, 12):
        ranks = [1] + [r] * 9 + [1]
        M1, M2, Y = train(rng, ranks), train(rng, ranks), train(rng, ranks)
        jobs = [([(0.5, M), (0.5, M, True)], 1e-2 * T.tt_norm(M), 0, None) for M in (M1, M2)]
        jobs.append(([(1.0, Y)], 1e-2 * T.tt_norm(Y), 0, None))
        bench_many(f"mixed group: 2 x (0.5 M + 0.5 M^T) at term ranks {r}+{r} and one plain train of ranks {r}", jobs,
                   reps, rounds)


def bench_kick(a, b, r, bwd, reps, rounds):
    from ttipm_amd import tt_eig as E
    rng = np.random.default_rng(5)
    mat = rng.standard_normal((b, a) if bwd else (a, b))
    Uh, Sh, Vh = np.linalg.svd(mat / np.linalg.norm(mat), full_matrices=False)
    pre = (D.from_numpy(Uh), D.from_numpy(Sh), D.from_numpy(Vh), Sh)
    sh = (a, 1, b, 1)
    lds = D.lib.ttk_split_kick_lds(int(bwd), a, b, len(Sh), r, 4, None)
    assert lds >= 0

    def call(switch):
        def f():
            D.SPLIT_KICK = switch
            return E._split(None, sh, 1e-30, r, bwd, pre=pre)  # every singular value kept up to max_rank = r
        return f

    what = (("composed split (the default)", call(False)), ("ttk_split_kick", call(True)))
    info = {}
    ref = None
    for name, f in what:
        np.random.seed(7)
        s1, s2 = f()
        torch.cuda.synchronize()
        l0, s0 = D.lib.ttk_launch_count(), D.lib.ttk_sync_count()
        f()
        torch.cuda.synchronize()
        nl, ns = D.lib.ttk_launch_count() - l0, D.lib.ttk_sync_count() - s0
        prod = D.read(s1).reshape(a, -1) @ D.read(s2).reshape(-1, b)
        ref = prod if ref is None else ref
        info[name] = (int(s1.shape[-1]), nl, ns, float(np.max(np.abs(prod - ref)) / np.max(np.abs(ref))))
        for _ in range(20):  # warm-up of every shape the timed window uses
            f()
    torch.cuda.synchronize()
    times = {name: [] for name, _ in what}
    for _ in range(rounds):
        for name, f in what:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(reps):
                f()
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t0) / reps * 1e6)
    D.SPLIT_KICK = False
    print(f"{'backward' if bwd else 'forward'} split a={a} b={b} r={r} kick 4; LDS {lds} bytes; {reps} calls x {rounds} "
          f"rounds, us per call", flush=True)
    for name, _ in what:
        t = np.array(times[name])
        q, nl, ns, err = info[name]
        print(f"{name:30s} median {np.median(t):8.1f}  min {t.min():8.1f}  max {t.max():8.1f}  launches {nl:3d}  "
              f"host waits {ns:2d}  |s1 s2 - default|/|default| {err:.2e}  rank {q}", flush=True)
    old, new = (np.array(times[name]) for name, _ in what)
    spread = max(old.max() - old.min(), new.max() - new.min())
    gap = float(np.median(old) - np.median(new))
    print(f"ttk_split_kick: {np.median(old) / np.median(new):.2f}x the composed split (medians {gap:.1f} us apart, "
          f"min-max spread {spread:.1f} us: {'beyond' if abs(gap) > spread else 'within'} the spread)\n", flush=True)


def main_kick(argv):
    reps = int(argv[0]) if argv else 100
    rounds = int(argv[1]) if len(argv) > 1 else 7
    assert torch.cuda.is_available(), "bench_round needs an MI355X"
    for a, b, r in ((8, 8, 4), (16, 16, 8), (64, 64, 28)):
        for bwd in (False, True):
            bench_kick(a, b, r, bwd, reps, rounds)


def bench_trunc(a, b, bwd, reps, rounds):
    from ttipm_amd import tt_eig as E
    rng = np.random.default_rng(5)
    p = min(a, b)
    U, _ = np.linalg.qr(rng.standard_normal((a, p)))
    V, _ = np.linalg.qr(rng.standard_normal((b, p)))
    s = 0.5 ** np.arange(p)
    s /= np.linalg.norm(s)
    sol = D.from_numpy((U * s) @ V.T)
    sc = np.cumsum(s[::-1] ** 2)[::-1]
    keep = p // 2
    tol = float(np.sqrt(np.sqrt(sc[keep] * sc[keep - 1])))  # between the two tail sums: no near tie
    sh = (a, 1, b, 1)
    lds = D.lib.ttk_trunc_kick_lds(int(bwd), a, b, 4, p, None)
    assert lds >= 0

    def call(split_kick, trunc_kick):
        def f():
            D.SPLIT_KICK, D.TRUNC_KICK = split_kick, trunc_kick
            return E._two_site_tail(sol, sh, tol, p, bwd, 1.0, None)[:2]
        return f

    what = (("composed tail (the default)", call(False, False)), ("TTIPM_SPLIT_KICK=1", call(True, False)),
            ("ttk_trunc_kick_read", call(False, True)))
    info = {}
    ref = None
    for name, f in what:
        np.random.seed(7)
        s1, s2 = f()
        torch.cuda.synchronize()
        l0, s0 = D.lib.ttk_launch_count(), D.lib.ttk_sync_count()
        f()
        torch.cuda.synchronize()
        nl, ns = D.lib.ttk_launch_count() - l0, D.lib.ttk_sync_count() - s0
        prod = D.read(s1).reshape(a, -1) @ D.read(s2).reshape(-1, b)
        ref = prod if ref is None else ref
        info[name] = (int(s1.shape[-1]), nl, ns, float(np.max(np.abs(prod - ref)) / np.max(np.abs(ref))))
        for _ in range(20):  # warm-up of every shape the timed window uses
            f()
    torch.cuda.synchronize()
    times = {name: [] for name, _ in what}
    for _ in range(rounds):
        for name, f in what:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(reps):
                f()
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t0) / reps * 1e6)
    D.SPLIT_KICK = D.TRUNC_KICK = False
    print(f"{'backward' if bwd else 'forward'} tail a={a} b={b} kept {keep} of {p} kick 4; LDS {lds} bytes; {reps} calls x "
          f"{rounds} rounds, us per call", flush=True)
    for name, _ in what:
        t = np.array(times[name])
        q, nl, ns, err = info[name]
        print(f"{name:30s} median {np.median(t):8.1f}  min {t.min():8.1f}  max {t.max():8.1f}  launches {nl:3d}  "
              f"host waits {ns:2d}  |s1 s2 - default|/|default| {err:.2e}  rank {q}", flush=True)
    old, mid, new = (np.array(times[name]) for name, _ in what)
    for label, other in (("the composed tail", old), ("TTIPM_SPLIT_KICK=1", mid)):
        spread = max(other.max() - other.min(), new.max() - new.min())
        gap = float(np.median(other) - np.median(new))
        print(f"ttk_trunc_kick_read: {np.median(other) / np.median(new):.2f}x {label} (medians {gap:.1f} us apart, "
              f"min-max spread {spread:.1f} us: {'beyond' if abs(gap) > spread else 'within'} the spread)", flush=True)
    print(flush=True)


def main_trunc(argv):
    reps = int(argv[0]) if argv else 100
    rounds = int(argv[1]) if len(argv) > 1 else 7
    assert torch.cuda.is_available(), "bench_round needs an MI355X"
    for a, b in ((8, 8), (16, 16), (64, 64)):
        for bwd in (False, True):
            bench_trunc(a, b, bwd, reps, rounds)


if __name__ == "__main__":
    if sys.argv[1:2] == ["trunc"]:
        main_trunc(sys.argv[2:])
    elif sys.argv[1:2] == ["kick"]:
        main_kick(sys.argv[2:])
    elif sys.argv[1:2] == ["many"]:
        main_many(sys.argv[2:])
    elif sys.argv[1:2] == ["affine"]:
        main_affine(sys.argv[2:])
    elif sys.argv[1:2] == ["prod"]:
        main_prod(sys.argv[2:])
    elif sys.argv[1:2] == ["one"]:
        main_one(sys.argv[2:])
    elif sys.argv[1:2] == ["sum"]:
        main_sum(sys.argv[2:])
    else:
        main()
