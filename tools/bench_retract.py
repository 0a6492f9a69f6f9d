"""Time the fixed-rank retraction, composed against the one-launch `ttk_retract`, on trains shaped like
the IPM's: d = 10 cores of (r, 2, 2, R) at three shapes -- ranks 8 / upper 4 (the train of
tools/bench_nystroem.py, comparable with profiles/nystroem_d10.txt), ranks 12 / upper 10 (the solve's
first retraction, upper = dim) and ranks 24 / upper 20 (the restart retraction, 2 dim).  Three things on
the same input, alternated round by round so that drift of the shared host hits all three alike:

    tt_rank_retraction   composed (TTIPM_NATIVE_RETRACT=0, the default: d QRs, d-1 SVDs with S read on
                                   the host, the einsum / copy launches between them)
    tt_rank_retraction   native   (`ttk_retract`: one launch of one workgroup, no host read)
    tt_rank_reduce       eps=1e-3 (`ttk_round`; another rounding, for context)

Each figure is a host clock around `reps` calls that end in a device synchronise, per call; the
table gives the median over the rounds and their min / max.  Also prints the launches and host
waits per call and the relative distance of each result from the input tensor, so the speeds are
read next to what was computed.

    python tools/bench_retract.py [reps] [rounds]
"""
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from ttipm_amd import dev as D  # noqa: E402
from ttipm_amd import tt_ops as T  # noqa: E402

SHAPES = ((8, 4), (12, 10), (24, 20))   # (bond rank, upper)


def bench(d, r, upper, reps, rounds):
    rng = np.random.default_rng(5)
    ranks = [1] + [r] * (d - 1) + [1]
    base = [D.from_numpy(rng.standard_normal((ranks[k], 2, 2, ranks[k + 1])) * (0.5 ** np.arange(ranks[k + 1])))
            for k in range(d)]
    up = [upper] * (d - 1)
    assert T.retract_lds(base, up) >= 0

    def composed():
        T.NATIVE_RETRACT = False
        return T.tt_rank_retraction(list(base), up)

    def native():
        T.NATIVE_RETRACT = True
        return T.tt_rank_retraction(list(base), up)

    def round_eps():
        return T.tt_rank_reduce(list(base), 1e-3)

    what = (("retraction composed", composed), ("retraction native", native), ("tt_rank_reduce eps=1e-3", round_eps))
    ref = T.tt_to_tensor(base)
    info = {}
    for name, f in what:
        out = f()
        torch.cuda.synchronize()
        l0 = D.lib.ttk_launch_count()
        s0 = D.lib.ttk_sync_count()
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
    T.NATIVE_RETRACT = False
    print(f"d={d} ranks {r} cores (r,2,2,R) upper {upper}; LDS {T.retract_lds(base, up)} bytes; "
          f"{reps} calls x {rounds} rounds, us per call", flush=True)
    for name, _ in what:
        t = np.array(times[name])
        rk, nl, ns, err = info[name]
        print(f"{name:24s} median {np.median(t):8.1f}  min {t.min():8.1f}  max {t.max():8.1f}  launches {nl:3d}  "
              f"host waits {ns:2d}  |out - in|/|in| {err:.2e}  ranks {rk}", flush=True)
    med = {name: float(np.median(times[name])) for name, _ in what}
    com, nat = np.array(times["retraction composed"]), np.array(times["retraction native"])
    spread = max(com.max() - com.min(), nat.max() - nat.min())
    print(f"retraction native: {med['retraction composed'] / med['retraction native']:.2f}x retraction composed "
          f"(medians {med['retraction composed'] - med['retraction native']:.1f} us apart, min-max spread {spread:.1f} us), "
          f"{med['tt_rank_reduce eps=1e-3'] / med['retraction native']:.2f}x tt_rank_reduce\n", flush=True)


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 100
    rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 7
    assert torch.cuda.is_available(), "bench_retract needs an MI355X"
    for r, upper in SHAPES:
        bench(10, r, upper, reps, rounds)


if __name__ == "__main__":
    main()
