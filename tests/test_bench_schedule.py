"""bench.py's seed schedule: YAML seeds only, shard dealing across ranks and
solves in flight, maxcut_12 r=2 (configs[4]) on 8 GPUs with the vetted extra seeds."""
import json
import os
import sys

import numpy as np
import pytest
import yaml

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def _cfg(name):
    return yaml.safe_load(open(os.path.join(ROOT, "configs", name)))


def test_maxcut10_single_gpu_uses_yaml_seeds_only():
    cfg = _cfg("maxcut_10.yaml")
    for P in (1, 2, 4):
        seeds, sched, slots = bench.make_schedule(cfg, "maxcut_10.yaml", None, 5, 1, 0, P, "shard")
        assert seeds == cfg["seeds"]
        assert all(len(st) == P for st in sched)
        assert {s for st in sched for s in st} == set(cfg["seeds"])
        assert [[st[j] for st in sched] for j in range(P)] == slots


def test_maxcut12_eight_ranks_distinct_seeds_per_step():
    cfg = _cfg("maxcut_12.yaml")
    per_rank = []
    for rank in range(8):
        seeds, sched, slots = bench.make_schedule(cfg, "maxcut_12.yaml", None, 2, 8, rank, 1, "shard")
        assert len(seeds) == 8 and seeds[:5] == cfg["seeds"] and seeds[5:] == bench.EXTRA_SEEDS["maxcut_12.yaml"]
        per_rank.append(slots[0])
    for i in range(2):  # each step: the 8 ranks solve the 8 distinct seeds
        assert sorted(r[i] for r in per_rank) == sorted(seeds)
    # with two solves in flight per GPU every seed is solved exactly twice per step
    _, sched, _ = bench.make_schedule(cfg, "maxcut_12.yaml", None, 1, 8, 0, 2, "shard")
    assert sorted(sched[0]) == sorted(seeds * 2)


def test_extra_seeds_follow_the_fixed_rule():
    """bench.EXTRA_SEEDS are the first seeds in seed order, skipping the config's own, whose reference
    run as shipped is not pathological (src/utils.py:67) -- every seed before the last one chosen
    has a reference run in runs.json, so the choice is re-derived here, not taken on trust."""
    runs = json.load(open(os.path.join(ROOT, "tests", "golden", "runs.json")))
    own = set(_cfg("maxcut_12.yaml")["seeds"])
    want = bench.EXTRA_SEEDS["maxcut_12.yaml"]
    got, s = [], 0
    while len(got) < len(want):
        if s not in own:
            key = f"maxcut_12_r2_s{s}"
            assert key in runs, f"the rule needs the reference run of seed {s}"
            r = runs[key]
            assert r["num_iters"] is not None
            if not (r["gap"] > 1e-3 or r["feas"] > 1e-3):
                got.append(s)
        s += 1
    assert got == want


def test_replica_schedule():
    cfg = _cfg("maxcut_10.yaml")
    _, sched, _ = bench.make_schedule(cfg, "maxcut_10.yaml", None, 3, 2, 1, 1, "replica")
    assert sched == [[41, 41], [23, 23], [235, 235]]


def test_default_inflight_is_constant_across_gpus():
    """The same solves in flight per GPU at N = 1, 2, 4, 8 (a like-for-like 1->8 series), and a node
    never runs more than 16 solve processes (default_threads slot threads per process; one slot per
    process wherever that fits)."""
    ps = [bench.default_inflight(w) for w in (1, 2, 4, 8)]
    assert len(set(ps)) == 1 and ps[0] >= 1
    for w in (1, 2, 4, 8, 16):
        P = bench.default_inflight(w)
        T = bench.default_threads(w, P)
        assert w * -(-P // T) <= 16
        assert T == 1 or w * P > 16


def _fake_results(sched, rank_count):
    import random
    rnd = random.Random(0)
    out = []
    for st in sched:
        for s in st:
            n = rnd.randint(10, 30)
            out.append({"seed": s, "num_iters": n, "runtime": 1.2345678901234 * n, "sec_per_iter": 1.2345678901234,
                        "gap": 4.123456789e-4, "feas": 2.123456789e-7, "dual_feas": 7.123456789e-10,
                        "assembly_t": [0.1 * i for i in range(n + 1)]})
    return out


def test_bench_line_fits_the_driver_tail():
    """The ONE stdout JSON line stays below 4 KB for an 8-GPU maxcut_12 r=2 schedule (configs[4]) with
    the driver's 20 steps; per-seed / per-step / per-op detail goes to the side file instead."""
    cfg = _cfg("maxcut_12.yaml")
    P = bench.default_inflight(8)
    seeds, sched, _ = bench.make_schedule(cfg, "maxcut_12.yaml", None, 20, 8, 0, P, "shard")
    results = _fake_results(sched, 8)
    solo = results[:len(seeds)]
    roof = {"bound": "mfma", "achieved": 0.00342, "peak": 78.6, "unit": "TFLOP/s", "frac": 4.3e-5,
            "traffic": 16874.75, "kernel": "contraction kernels", "seed": 80,
            "algorithmic_flops_per_solve": 1.19e9, "launches_per_solve": 55421,
            "algorithmic_by_op": {f"op{i}": [i, 1e6 * i] for i in range(10)}}
    per = [{"seed": s, "iters": 12, "s_per_iter": 3.3, "work_s": 40.0, "full_solve_iters": 12,
            "full_solve_s_per_iter": 3.4, "assembly_t": [float(i) for i in range(13)], "threads": "1"} for s in seeds]
    cpu = bench.cpu_summary(per, per[0], solo, 300.0, "maxcut dim=12 rank=2", 16)
    line, detail = bench.compose_line("maxcut", cfg, "maxcut_12.yaml", 2, 8, P, 1, P, 20, 5, "shard", 123.4,
                                      sum(r["num_iters"] for r in results), seeds, sched, results, solo, roof, cpu,
                                      "gpurun_out/bench_detail.json")
    s = json.dumps(line)
    assert len(s) < 4096, len(s)
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
              "vs_baseline", "dtype", "data", "config", "roofline", "cpu_baseline", "sec_per_iter_per_seed_median"):
        assert k in line
    assert "algorithmic_by_op" not in line["roofline"] and "per_seed" not in line["cpu_baseline"]
    assert {"bound", "achieved", "peak", "unit", "frac", "traffic"} <= set(line["roofline"])
    assert {"value", "unit", "cores", "kind", "sample"} <= set(line["cpu_baseline"])
    assert len(detail["per_seed"]) == len(results) and detail["seeds_per_step"] == sched
    assert line["cpu_baseline"]["gpu_over_cpu_median_of_ratios"] is not None


def _claim_many(path, n, out):
    got = []
    while True:
        i = bench._claim(path)
        if i >= n:
            break
        got.append(i)
    out.extend(got)


def _claim_proc(path, n, q):
    got = []
    _claim_many(path, n, got)
    q.put(got)


def test_dynamic_balance_claims_every_solve_once(tmp_path):
    """`--balance dynamic`: the rank's processes and slot threads claim its work list through one
    counter file; every index is handed out exactly once, whoever asks."""
    import multiprocessing as mp
    import threading
    n = 200
    path = tmp_path / "q"
    path.write_text("0")
    q = mp.get_context("spawn").Queue()
    procs = [mp.get_context("spawn").Process(target=_claim_proc, args=(str(path), n, q)) for _ in range(2)]
    for p in procs:
        p.start()
    outs = [[] for _ in range(3)]
    ths = [threading.Thread(target=_claim_many, args=(str(path), n, outs[k])) for k in range(3)]
    for t in ths:
        t.start()
    for t in ths:
        t.join()
    got = [i for o in outs for i in o] + [i for _ in procs for i in q.get(timeout=60)]
    for p in procs:
        p.join(timeout=60)
    assert sorted(got) == list(range(n))


def test_dump_outputs_writes_the_last_step(tmp_path):
    """`--dump-outputs`: one float64 row per solve of the last timed step, ordered by (rank, slot),
    whatever order the processes' results arrive in; the files are the solve's returned values."""
    P, K = 4, 3
    _, sched, _ = bench.make_schedule(_cfg("maxcut_10.yaml"), "maxcut_10.yaml", None, K, 1, 0, P, "shard")
    res = []
    for j in (2, 0, 3, 1):  # slot-major, as the processes report, in a scrambled process order
        for k in range(K):
            res.append({"seed": sched[k][j], "num_iters": 10 + j + k, "gap": 1e-4 * (j + 1) + k, "feas": 1e-7 * (k + 1),
                        "dual_feas": 1e-10 * (j + 1), "ranksX": [2 + j] * 9, "ranksY": [1] * 9, "ranksZ": [3] * 9,
                        "ranksT": [0] * 9, "rank": 0, "slot": j, "nth": k, "runtime": 1.0})
    bench.dump_outputs(str(tmp_path / "out"), res)
    got = {f[:-4]: np.load(tmp_path / "out" / f) for f in sorted(os.listdir(tmp_path / "out"))}
    assert set(got) == set(bench.OUTPUT_SCALARS + bench.OUTPUT_RANKS)
    assert all(a.dtype == np.float64 for a in got.values())
    assert got["seed"].tolist() == sched[-1]
    assert got["num_iters"].tolist() == [10 + j + K - 1 for j in range(P)]
    assert got["gap"].tolist() == [1e-4 * (j + 1) + K - 1 for j in range(P)]
    assert got["ranksX"].shape == (P, 9) and got["ranksX"][:, 0].tolist() == [2.0, 3.0, 4.0, 5.0]
    assert sum(a.nbytes for a in got.values()) < 64 << 20


def test_detail_file_is_best_effort(tmp_path, capsys):
    """The `--detail` side file: written where it can be; where it cannot (here: its folder's name is
    taken by a file), the run goes on and the line says that there is no detail file."""
    line = {"value": 1.0, "detail": str(tmp_path / "d" / "detail.json")}
    bench.write_detail(line["detail"], {"line": line, "per_seed": []}, line)
    assert json.load(open(tmp_path / "d" / "detail.json"))["line"]["value"] == 1.0
    (tmp_path / "f").write_text("")
    line["detail"] = str(tmp_path / "f" / "detail.json")
    bench.write_detail(line["detail"], {"line": line}, line)
    assert line["detail"] is None and "detail file not written" in capsys.readouterr().err
