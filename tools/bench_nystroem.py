"""Time the generalised Nystroem rounding against `tt_rank_reduce` and the one-launch randomised
sweep on a train shaped like the IPM's: d = 10 cores of (8, 2, 2, 8), target rank 4 (the train of
tools/bench_randorth.py), the sketches drawn beforehand (so the timed native calls have no host
read).  Four things on the same input, alternated round by round so that drift of the shared host
hits all four alike:

    tt_rank_reduce                (`ttk_round`: d-1 QRs, d-1 SVDs, d-1 host reads; the baseline)
    _tt_lr_random_orthogonalise   native   (`ttk_rand_orth`: one launch of one workgroup)
    _tt_generalised_nystroem      composed (TTIPM_NATIVE_NYSTROEM=0 path: einsum / SVD launches, S read)
    _tt_generalised_nystroem      native   (`ttk_nystroem`: three launches of 2, d-1 and d workgroups)

Each figure is a host clock around `reps` calls that end in a device synchronise, per call; the
table gives the median over the rounds and their min / max.  Also prints the launches and host
waits per call and the relative distance of each result from the input tensor (the roundings
differ: eps against fixed ranks), so the speeds are read next to what was computed.

    python tools/bench_nystroem.py [reps] [rounds]
"""
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from ttipm_amd import dev as D  # noqa: E402
from ttipm_amd import tt_ops as T  # noqa: E402


def dense(tt):
    return T.tt_to_tensor(tt)


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 300
    rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 7
    assert torch.cuda.is_available(), "bench_nystroem needs an MI355X"
    d, r, target, eps = 10, 8, 4, 1e-3
    rng = np.random.default_rng(5)
    ranks = [1] + [r] * (d - 1) + [1]
    base = [D.from_numpy(rng.standard_normal((ranks[k], 2, 2, ranks[k + 1])) * (0.5 ** np.arange(ranks[k + 1])))
            for k in range(d)]
    np.random.seed(7)
    sketch = T.tt_random_gaussian([target] * (d - 1), shape=(2, 2))   # bench_randorth's sketch, and the left one
    right = T.tt_random_gaussian([target + 1] * (d - 1), shape=(2, 2))
    assert T.randorth_lds(base, sketch) >= 0 and T.nystroem_lds(base, sketch, right) >= 0

    def round_eps():
        return T.tt_rank_reduce(list(base), eps)

    def rand_orth():
        return T._tt_lr_random_orthogonalise(list(base), sketch)

    def composed():
        T.NATIVE_NYSTROEM = False
        return T._tt_generalised_nystroem(list(base), sketch, right)

    def native():
        T.NATIVE_NYSTROEM = True
        return T._tt_generalised_nystroem(list(base), sketch, right)

    what = (("tt_rank_reduce eps=1e-3", round_eps), ("rand_orth native", rand_orth), ("nystroem composed", composed),
            ("nystroem native", native))
    ref = dense(base)
    info = {}
    for name, f in what:
        out = f()
        torch.cuda.synchronize()
        l0 = D.lib.ttk_launch_count()
        s0 = D.lib.ttk_sync_count()
        f()
        torch.cuda.synchronize()
        info[name] = (T.tt_ranks(out), D.lib.ttk_launch_count() - l0, D.lib.ttk_sync_count() - s0,
                      float(np.linalg.norm(dense(out) - ref) / np.linalg.norm(ref)))
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
    print(f"d={d} ranks {r} cores (r,2,2,R) target {target}; {reps} calls x {rounds} rounds, us per call", flush=True)
    for name, _ in what:
        t = np.array(times[name])
        rk, nl, ns, err = info[name]
        print(f"{name:24s} median {np.median(t):8.1f}  min {t.min():8.1f}  max {t.max():8.1f}  launches {nl:3d}  "
              f"host waits {ns:2d}  |out - in|/|in| {err:.2e}  ranks {rk}", flush=True)
    med = {name: float(np.median(times[name])) for name, _ in what}
    com, nat = np.array(times["nystroem composed"]), np.array(times["nystroem native"])
    spread = max(com.max() - com.min(), nat.max() - nat.min())
    print(f"nystroem native: {med['nystroem composed'] / med['nystroem native']:.2f}x nystroem composed "
          f"(medians {med['nystroem composed'] - med['nystroem native']:.1f} us apart, min-max spread {spread:.1f} us), "
          f"{med['rand_orth native'] / med['nystroem native']:.2f}x rand_orth native, "
          f"{med['tt_rank_reduce eps=1e-3'] / med['nystroem native']:.2f}x tt_rank_reduce", flush=True)


if __name__ == "__main__":
    main()
