#!/usr/bin/env python
"""Headline benchmark: sec / IPM-iteration of the TT-IPM Newton/KKT path on maxcut dim=10 rank=1
(BASELINE.json `metric`, config `configs/maxcut_10.yaml`), seed-sharded over N GPUs.

    python bench.py [--gpus N --steps K --warmup W] [--dump-outputs DIR] [--full]
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 \\
        --master-port P bench.py --gpus N --steps K --warmup W

* Seeds: the config's own list (maxcut_10.yaml: 41, 23, 235, 35, 14) -- nothing else unless
  `--seeds` names them.  A "step" is one full `tt_ipm` solve of one seed per GPU (the reference's
  unit of work, `src/utils.py:245-321`).  Schedule `shard` (default): step i on rank p solves
  seeds[(i*N + p) mod S], so every rank does `--steps` solves (fixed per-GPU work: weak scaling)
  and at N=1 the steps cycle through the config's seeds.  `replica`: every rank solves step i's
  N=1 seed.  Problems are created once per distinct seed on rank 0 and delivered by ONE broadcast
  (RCCL over xGMI with the nccl backend) before the timed region; no collective inside the IPM loop.
* Solves in flight per GPU (`--inflight P`, default 4 at every N, so the 1/2/4/8-GPU series is
  like-for-like): a solve is a chain of small dependent launches that leaves most of the chip idle,
  so each GPU runs P seeds at once: P/T processes (this one plus workers spawned before the GPU is
  touched) of T = `--threads` slot threads (default `default_threads`: 1 -- one solve per process,
  on its default stream, with its own GIL -- up to N = 4; 2 at N = 8, where 16 solve processes is the
  node's limit), a process's several slots each on its own created stream and libttk context.  The bench processes get 8 HIP hardware
  queues (`GPU_MAX_HW_QUEUES`, recorded in `env_knobs`).  All slots warm up, then are released
  together at the start of the timed region.  A step is P solves per GPU: step i, rank p, slot j
  solves seeds[(i*N*P + p*P + j) mod S] (`--balance static`, the default).  With K a multiple of the
  seed count every slot solves every seed equally often at any N (maxcut_10, K = 5: slot loads equal),
  which FIFO claiming cannot beat: `--balance dynamic` (the rank's K x P solves in that order go to
  whichever slot is free next through one shared counter, `_claim`) measured 0.114 against static's
  0.108 s/IPM-iter at K = 5 (its last claims are long seeds), and helps only when K leaves the
  columns unequal.
* Timed region: barrier + device sync on both sides of the K steps, max over ranks.
  `value` = (max-over-ranks wall) / (IPM iterations of all ranks): whole-job s per IPM-iteration.
  `ms_per_step` = that wall / K.
* A plain run is set-up, warm-up, the K timed steps and the result line, nothing else.  `--full`
  adds the three untimed legs below (the one-at-a-time latency pass, `roofline`, `cpu_baseline`;
  `--no-solo`, `--no-roofline` and `--no-cpu-baseline` take them out again one by one); without it
  their keys of the line are null.
* `--dump-outputs DIR` (after the timed steps, outside the timed region): what each solve of the last
  timed step returned to its caller, as DIR/<name>.npy in float64, one row per solve ordered by
  (rank, slot): `seed`, `num_iters`, `gap`, `feas`, `dual_feas`, `ranksX/Y/Z/T` (`last_step_outputs`).
  The same arguments give the same seeds, problems and RNG states, row for row.
* `--full`, `sec_per_iter_per_seed_median`: SURVEY.md §8(d)'s statistic as the reference runner measures it
  (`src/utils.py:298-302`: one solve at a time, solve wall / its IPM iterations, median over seeds):
  after the timed region (rank 0, N=1) every distinct timed seed is solved once more ALONE on the
  GPU.  `sec_per_iter_per_seed_median_inflight` is the same statistic over the timed (contended)
  solves.
* `--full`, `roofline` (contraction kernels: the MFMA GEMM `gemm_offs*`, the fused local apply and the Schur
  multi-task apply): an untimed re-solve of each distinct seed rank 0 timed (the timed region's seed
  mix) with every contraction launch bracketed by HIP events on its stream.  achieved = ALGORITHMIC contraction FLOPs of that solve
  (NumPy `einsum_path` greedy convention per einsum call plus the chained applies of every local
  KKT operator application; `dev.ALGO`) / summed contraction kernel time; peak =
  78.6 TFLOP/s fp64 matrix.
* `--full`, `cpu_baseline` (rank 0, N=1 only): the oracle CPU restatement of the reference path (`oracle/`,
  a port) on this host: one single-thread process per distinct timed seed, all at once, each its
  seed's WHOLE solve (`--cpu-cap` is only a safety bound).  `value` = median over seeds of solve
  wall / IPM iterations; beside it the GPU's one-at-a-time figure for the same seeds, as a ratio of
  medians and as the median of per-seed ratios.  Then one seed with all the host share's cores as
  BLAS threads (bounded to 60 s).  The workers start before this process touches the GPU and wait
  on a pipe until the GPU work is done.
* Output: ONE JSON line on stdout (< 4 KB: the contract's keys and the summary statistics); the
  per-seed results, the per-step schedule, the solo solves, the CPU per-seed rows and the per-op
  FLOP split go to `--detail` (default gpurun_out/bench_detail.json).
"""
import argparse
import contextlib
import ctypes
import json
import os
import subprocess
import sys
import time

import numpy as np
import yaml

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

METRIC = "sec/IPM-iter (AMEn KKT solve), maxcut dim=10 r=1; MFMA util% on core-contract"
FP64_MATRIX_PEAK = 78.6e12  # MI355X spec, FLOP/s
HOST_SHARE = 16  # CPU share of one GPU on the box (nproc shows the whole machine)

# Seeds beyond a config's own list (maxcut_12 r=2 lists 5 seeds, the 8-GPU run
# needs 8), chosen by a rule fixed in advance that looks at nothing but the reference: the first
# seeds in seed order, skipping the config's own, whose reference run as shipped (tests/golden/
# runs.json, src/utils.py:67) is not pathological.  tests/test_bench_schedule.py re-derives them.
EXTRA_SEEDS = {"maxcut_12.yaml": [1, 9, 11]}


class _Stop(Exception):
    pass


_CHILDREN = []  # every worker Popen; terminated on any early exit of main()
_TEMP_FILES = []  # the dynamic schedule's counter files; removed on any exit of main()


def _reap_children():
    for f in _TEMP_FILES:
        with contextlib.suppress(OSError):
            os.unlink(f)
    for p in _CHILDREN:
        if p.poll() is None:
            p.terminate()
    for p in _CHILDREN:
        try:
            p.wait(timeout=10)
        except subprocess.TimeoutExpired:
            p.kill()
            p.wait()


class _BoundedTrace(list):
    """Trace sink that time-stamps each Newton-system assembly and stops the solve once `cap`
    seconds have passed since the first assembly (after at least one full iteration)."""

    def __init__(self, cap):
        super().__init__()
        self.cap, self.t = cap, []

    def append(self, item):
        self.t.append(time.perf_counter())
        super().append(item)
        if len(self.t) > 1 and self.t[-1] - self.t[0] >= self.cap:
            raise _Stop


def _cpu_worker(problem, cfg_path, seed, rank_tt, cap, cores=None):
    """Child process: wait for 'go' on stdin, run the oracle on one seed, print one JSON line."""
    import warnings
    if cores:
        os.sched_setaffinity(0, cores)
    from oracle import ipm as OI
    from oracle import problems as OP
    from oracle import tt as OT
    config = yaml.safe_load(open(cfg_path))
    with warnings.catch_warnings(), contextlib.redirect_stdout(sys.stderr):
        warnings.simplefilter("error")
        np.random.seed(seed)
        prob = OP.PROBLEMS[problem](config["dim"], rank_tt, verbose=False)
    if sys.stdin.readline().strip() != "go":  # EOF: the parent is gone -- do not run as an orphan
        sys.exit(3)
    with warnings.catch_warnings(), contextlib.redirect_stdout(sys.stderr):
        warnings.simplefilter("error")
        if len(prob) == 5:
            C, L, b, mask, lag = prob
        else:
            C, L, b, lag_y = prob
            mask, lag = None, {"y": lag_y}
        lag = {k: OT.reshape(v, (4, 4)) for k, v in lag.items()}
        C, b = OT.reshape(C, (4,)), OT.reshape(b, (4,))
        trace = _BoundedTrace(cap if cap > 0 else float("inf"))
        t_start = time.perf_counter()
        try:
            res = OI.tt_ipm(lag, C, L, b, ineq_mask=mask, max_iter=config["max_iter"], verbose=False,
                            gap_tol=float(config["gap_tol"]), op_tol=float(config["op_tol"]),
                            warm_up=config["warm_up"], abs_tol=float(config["abs_tol"]), aho_direction=False,
                            mals_restarts=config["mals_restarts"], max_refinement=config["max_refinement"],
                            lambdaStar=float(config.get("lambdaStar", 1)),
                            lambdaStarIneq=float(config.get("lambdaStarIneq", 1)), trace=trace)
            full = int(res[4]["num_iters"])
            wall = time.perf_counter() - t_start
        except _Stop:
            full, wall = None, None
    n_it = len(trace.t) - 1
    out = {"seed": seed, "iters": n_it, "s_per_iter": (trace.t[n_it] - trace.t[0]) / max(n_it, 1),
           "work_s": trace.t[n_it] - t_start,
           "assembly_t": [t - trace.t[0] for t in trace.t], "threads": os.environ.get("OPENBLAS_NUM_THREADS"),
           "cores": sorted(os.sched_getaffinity(0)), "hash_seed": os.environ.get("PYTHONHASHSEED")}
    if full is not None:
        out.update(full_solve_iters=full, full_solve_s_per_iter=wall / max(full, 1))
    print(json.dumps(out), flush=True)


def _claim(path):
    """Next index of a rank's work list: a counter in the file `path`, incremented under an exclusive
    flock (shared by the rank's processes and slot threads; a claim costs tens of microseconds)."""
    import fcntl
    with open(path, "r+") as f:
        fcntl.flock(f, fcntl.LOCK_EX)
        try:
            n = int(f.read().strip() or 0)
            f.seek(0)
            f.write(str(n + 1))
            f.truncate()
            f.flush()
        finally:
            fcntl.flock(f, fcntl.LOCK_UN)
    return n


def _cu_masked_stream(part, nparts):
    """A HIP stream whose kernels run on one of `nparts` disjoint CU sets (hipExtStreamCreateWithCUMask):
    TTIPM_CU_LAYOUT=block (default) gives part i the mask bits [i N/n, (i+1) N/n), stride the bits c
    with c % n == i.  Diagnostics (TTIPM_CU_PARTS): do the solves in flight interfere through CU
    occupancy -- a one-workgroup kernel that needs a whole CU's LDS waiting for CUs other solves'
    multi-workgroup launches hold?  Measured no: 4 one-slot processes on 4 disjoint 64-CU sets ran
    0.39-0.40 s/IPM-iter against 0.090 on their default streams (profiles/r05_inflight_layouts.txt) --
    a created stream per process costs far more than any sharing of CUs."""
    import torch
    hip = ctypes.CDLL("libamdhip64.so")
    ncu = torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count
    words = (ncu + 31) // 32
    mask = (ctypes.c_uint32 * words)()
    stride = os.environ.get("TTIPM_CU_LAYOUT", "block") == "stride"
    for c in range(ncu):
        mine = (c % nparts == part) if stride else (c * nparts // ncu == part)
        if mine:
            mask[c // 32] |= 1 << (c % 32)
    st = ctypes.c_void_p()
    rc = hip.hipExtStreamCreateWithCUMask(ctypes.byref(st), ctypes.c_uint32(words), mask)
    if rc != 0:
        raise RuntimeError(f"hipExtStreamCreateWithCUMask returned {rc}")
    return st.value


class _Slots:
    """The solves in flight of one process: one host thread per slot, each with its own HIP stream,
    libttk context (`dev`'s per-thread state) and NumPy random stream (`ttipm_amd.rng`).  Every slot
    thread warms up on its first seed, uploads its problems, then waits for `start()`, solves its
    seeds back to back and records its wall time (its own stream synchronised).  The launches
    themselves release the GIL, so the slots' host work overlaps while their kernels run."""

    def __init__(self, slot_seeds, packed, solve, warmup, device, queue=None, slot_base=0):
        """queue: None -- slot j solves slot_seeds[j] back to back (static); or (work, path) -- every
        slot claims the next index of the rank's ordered work list from the cross-process counter
        file `path` (`_claim`) until the list is exhausted (slot_seeds[j][0] is still its warm-up
        seed)."""
        import threading
        if len(slot_seeds) > 1:  # a slot waiting for the GIL asks for it after 0.5 ms, not 5 ms
            sys.setswitchinterval(SLOT_SWITCH_INTERVAL)
        self.n = len(slot_seeds)
        self.queue = queue
        self.slot_base = slot_base
        self.ready = threading.Barrier(self.n + 1)
        self.go = threading.Event()
        self.out = [None] * self.n
        self.err = []
        self.threads = [threading.Thread(target=self._run, args=(j, sl, packed, solve, warmup, device), daemon=True)
                        for j, sl in enumerate(slot_seeds)]
        for t in self.threads:
            t.start()

    def _run(self, j, seeds, packed, solve, warmup, device):
        import torch
        from ttipm_amd import rng, shard
        preps = None
        try:
            if device is not None:
                torch.cuda.set_device(device)
                # one slot per process: the default stream (measured: two processes on created streams
                # slow each other 2.6x, on their default streams not at all, profiles/r03_inflight_layouts.txt)
                parts = int(os.environ.get("TTIPM_CU_PARTS", "0"))
                if parts > 0:
                    torch.cuda.set_stream(torch.cuda.ExternalStream(
                        _cu_masked_stream((self.slot_base + j) % parts, parts)))
                elif self.n > 1 or os.environ.get("TTIPM_SLOT_STREAM", "default") != "default":
                    torch.cuda.set_stream(torch.cuda.Stream())
            rng.private()
            for _ in range(warmup):  # untimed: plans, this context's scratch, allocator, code pages
                solve(shard.unpack(*packed[seeds[0]]))
            # every problem this slot may solve, unpacked before the timed region (a dynamic slot may
            # claim any entry of the work list: one fresh copy per entry)
            work = seeds if self.queue is None else self.queue[0]
            preps = [shard.unpack(*packed[sd]) for sd in work]
            if device is not None:
                torch.cuda.current_stream().synchronize()
        except BaseException as e:  # noqa: BLE001 - re-raised by join()
            self.err.append(e)
        self.ready.wait()
        self.go.wait()
        if preps is None:
            return
        try:
            traces, res = [], []
            t0 = time.perf_counter()
            if self.queue is None:
                for pr in preps:
                    traces.append([])
                    res.append(solve(pr, trace=traces[-1]))
            else:
                while True:
                    idx = _claim(self.queue[1])
                    if idx >= len(preps):
                        break
                    traces.append([])
                    res.append(solve(preps[idx], trace=traces[-1]))
                    preps[idx] = None  # solved: let the allocator reuse its cores
            if device is not None:
                torch.cuda.current_stream().synchronize()
            elapsed = time.perf_counter() - t0
            for k, (r, tr) in enumerate(zip(res, traces)):  # per-iteration stamps (Newton-system assemblies)
                r["assembly_t"] = [e["t"] - tr[0]["t"] for e in tr] if tr else []
                r["slot"], r["nth"] = self.slot_base + j, k  # the slot that solved it, and its place among that slot's solves
            self.out[j] = (elapsed, res)
        except BaseException as e:  # noqa: BLE001
            self.err.append(e)

    def wait_ready(self):
        self.ready.wait()
        if self.err:
            raise RuntimeError(f"bench: a solve slot failed before the timed region: {self.err[0]!r}")

    def start(self):
        self.go.set()

    def join(self):
        for t in self.threads:
            t.join()
        if self.err:
            raise RuntimeError(f"bench: a solve slot failed in the timed region: {self.err[0]!r}")
        return [o[0] for o in self.out], [r for o in self.out for r in o[1]]


def _hip_schedule():
    """TTIPM_HIP_SCHED = spin | yield | blocking: hipSetDeviceFlags(hipDeviceSchedule*) before this
    process's HIP context exists (how host threads wait in hipStreamSynchronize: a spinning wait holds
    a core, a blocking one sleeps on an interrupt; diagnostics for solve processes that share the
    box's cores).  Unset: HIP's default (auto)."""
    mode = os.environ.get("TTIPM_HIP_SCHED")
    if not mode:
        return
    flag = {"spin": 1, "yield": 2, "blocking": 4}[mode]
    rc = ctypes.CDLL("libamdhip64.so").hipSetDeviceFlags(ctypes.c_uint(flag))
    if rc != 0:
        print(f"bench: hipSetDeviceFlags({mode}) returned {rc}", file=sys.stderr)


def _gpu_worker(args, slot_seeds, queue=None):
    """Child process (more solves in flight on this rank's GPU): create its seeds' problems, start
    one slot thread per seed list (`_Slots`), print 'ready' once all have warmed up, wait for 'go'
    on stdin, run the solves, print one JSON line with the slots' elapsed wall times and the
    per-seed results."""
    import torch
    local = int(os.environ.get("LOCAL_RANK", "0"))
    dev = local % torch.cuda.device_count()
    _hip_schedule()
    torch.cuda.set_device(dev)
    from ttipm_amd import shard
    from ttipm_amd.utils import create
    from ttipm_amd.utils import solve as _solve
    config = yaml.safe_load(open(args.config))
    keep = ("seed", "num_iters", "runtime", "sec_per_iter", "gap", "feas", "dual_feas", "assembly_t",
            "ranksX", "ranksY", "ranksZ", "ranksT", "slot", "nth")
    with contextlib.redirect_stdout(sys.stderr):  # once, around all slot threads (not thread-safe)
        need = [s for sl in slot_seeds for s in sl] + (list(queue[0]) if queue else [])
        packed = {s: shard.pack(create(args.problem, config, s, args.rank, verbose=False)) for s in dict.fromkeys(need)}

        def solve(prep, trace=None):
            return _solve(prep, config, quiet=True, verbose=False, trace=trace)

        slots = _Slots(slot_seeds, packed, solve, args.warmup, dev, queue=queue, slot_base=args.slot_base)
        slots.wait_ready()
        print("ready", file=sys.__stdout__, flush=True)
        if sys.stdin.readline().strip() != "go":  # EOF: the parent is gone -- do not run as an orphan
            os._exit(3)
        slots.start()
        elapsed, results = slots.join()
    print(json.dumps({"elapsed": elapsed, "results": [{k: r.get(k) for k in keep} for r in results]}), flush=True)


def _spawn_gpu_workers(args, proc_slots, queue=None, base=0):
    """Started BEFORE this process initialises the GPU; each prints 'ready' once warmed up.
    proc_slots: per worker process, its slots' seed lists; queue: (work list, counter file) of the
    dynamic schedule, or None."""
    procs = []
    for w, slots in enumerate(proc_slots):  # global slot ids: this process's own `base` slots first
        cmd = [sys.executable, os.path.abspath(__file__), "--gpu-worker",
               ";".join(",".join(map(str, sl)) for sl in slots),
               "--problem", args.problem, "--config", args.config, "--rank", str(args.rank),
               "--warmup", str(args.warmup), "--slot-base", str(base + sum(len(x) for x in proc_slots[:w]))]
        if queue is not None:
            cmd += ["--queue-work", ",".join(map(str, queue[0])), "--queue-file", queue[1]]
        procs.append(subprocess.Popen(cmd, stdin=subprocess.PIPE, stdout=subprocess.PIPE, stderr=sys.stderr,
                                      text=True))
    _CHILDREN.extend(procs)
    return procs


def _spawn_cpu_workers(args, seeds, threads, cap, cores):
    """Started BEFORE the GPU is initialised (no exec from a GPU process); each blocks on stdin.
    Pinned: PYTHONHASHSEED=0, the golden's string-hash seed -- the oracle's
    contraction order, like the reference's, follows set iteration (tests/golden/make_golden.py) --
    and each worker on its own core(s) of `cores` (disjoint sched_setaffinity sets, `--cpu-cores`)."""
    procs = []
    at = 0
    for s, th in zip(seeds, threads):
        mine = cores[at:at + th] or cores[-th:]
        at += th
        env = dict(os.environ, OPENBLAS_NUM_THREADS=str(th), OMP_NUM_THREADS=str(th), MKL_NUM_THREADS=str(th),
                   CUDA_VISIBLE_DEVICES="", HIP_VISIBLE_DEVICES="", PYTHONHASHSEED="0")
        cmd = [sys.executable, os.path.abspath(__file__), "--cpu-worker", str(s), "--problem", args.problem,
               "--config", args.config, "--rank", str(args.rank), "--cpu-cap", str(cap),
               "--cpu-cores", ",".join(str(c) for c in mine)]
        procs.append(subprocess.Popen(cmd, stdin=subprocess.PIPE, stdout=subprocess.PIPE,
                                      stderr=subprocess.DEVNULL, env=env, text=True))
    _CHILDREN.extend(procs)
    return procs


def _release(procs):
    for p in procs:
        p.stdin.write("go\n")
        p.stdin.flush()
    out = []
    for p in procs:
        line = p.stdout.read().strip().splitlines()
        p.wait()
        out.append(json.loads(line[-1]) if line else None)
    return out


def _profiled():
    """True under rocprofv3 (its tool library is preloaded and initialises the GPU before main)."""
    return any(k.startswith("ROCPROF") for k in os.environ) or "rocprof" in os.environ.get("LD_PRELOAD", "")


def _cpu_model():
    try:
        for line in open("/proc/cpuinfo"):
            if line.startswith("model name"):
                return line.split(":", 1)[1].strip()
    except OSError:
        pass
    return None


def _pmc_traffic():
    """HBM bytes per contraction launch from the committed PMC passes over the same workload
    (counters need their own rocprofv3 runs, so they cannot be read live here); the newest round's
    file wins.  Corrected as MI355X_MICROARCH.md's HBM section prescribes: gfx950's FETCH_SIZE counts
    half the bytes of a coalesced read, so bytes = (2 x FETCH_SIZE + WRITE_SIZE) KB x 1024."""
    for name in ("r06_pmc_maxcut10.json", "r05_pmc_maxcut10.json", "r04_pmc_maxcut10.json", "r03_pmc_maxcut10.json",
                 "r02_pmc_maxcut10.json", "r01_pmc_maxcut10.json"):
        try:
            ks = json.load(open(os.path.join(HERE, "profiles", name)))["kernels"]
        except (OSError, KeyError, ValueError):
            continue
        # dispatch-weighted over the gemm_offs_kernel<TS> instantiations
        num = den = 0.0
        for k, e in ks.items():
            base = k.replace("void ", "").split("<")[0].strip()
            if base == "gemm_offs_kernel" and "FETCH_SIZE_KB" in e and "WRITE_SIZE_KB" in e:
                num += (2.0 * e["FETCH_SIZE_KB"] + e["WRITE_SIZE_KB"]) * e["dispatches"]
                den += e["dispatches"]
        if den:
            return num / den * 1024.0
    return None


DEFAULT_INFLIGHT = 4  # solves in flight per GPU, the same at every N (like-for-like 1->8 series)
NODE_PROCESSES = 16  # solve processes a node may run on its GPUs at once (the box's process guard)
SLOT_SWITCH_INTERVAL = 0.0005  # sys.setswitchinterval for processes with several slot threads
HW_QUEUES = 8  # GPU_MAX_HW_QUEUES for the bench processes (HIP's default is 4; TTIPM_HW_QUEUES overrides)


def default_threads(world, P):
    """Slot threads per process: 1 (every solve its own process, default stream, own GIL) while the
    node's solve processes stay within NODE_PROCESSES (N <= 4 at 4 in flight), else the fewest that
    fit (N = 8: 2).  One box, maxcut_10, 4 in flight, alternating runs: 4 processes x 1 slot 0.092 /
    0.093 s/IPM-iter, 2 processes x 2 slots 0.107 / 0.109 (two slots of one process share its GIL;
    profiles/r05_inflight_layouts.txt)."""
    procs_per_gpu = max(1, NODE_PROCESSES // max(world, 1))
    return max(1, -(-P // procs_per_gpu))


def default_inflight(world):
    """Solves in flight per GPU: DEFAULT_INFLIGHT at every N up to 8, so the 1/2/4/8-GPU series
    carries the same per-GPU load (default_threads splits it over processes within the node's
    NODE_PROCESSES solve processes).  Why threads work since round 4:
    the launch-only library calls keep the GIL (`_lib.py`), a slot waiting for the GIL asks for it
    after 0.5 ms, and each process gets 8 HIP hardware queues -- with HIP's default 4, a process's
    two slot streams plus their libttk side streams share queues and two such processes slowed each
    other down (maxcut_10, whole job: 2 processes x 1 slot 0.190, 2 x 2 slots 0.209 with 4 queues,
    0.117-0.131 with 8 or 16; 2 x 3: 0.155, 2 x 4: 0.128; profiles/r04_inflight_layouts.txt)."""
    return max(1, min(DEFAULT_INFLIGHT, 2 * (NODE_PROCESSES // max(world, 1))))


def make_schedule(config, cfg_name, seeds_arg, steps, world, rank, P, mode):
    """(seeds, per-step seed lists, this rank's per-slot seed lists).  Step i, rank p, slot j
    solves seeds[(i*N*P + p*P + j) mod S] (`shard`) or step i's N=1 seed (`replica`); the config's
    seeds only, plus the vetted EXTRA_SEEDS when a shard step has more solves than seeds."""
    if seeds_arg:
        seeds = [int(s) for s in seeds_arg.split(",")]
    else:
        seeds = list(config["seeds"])
        if mode == "shard" and world * P > len(seeds):
            seeds += [s for s in EXTRA_SEEDS.get(cfg_name, []) if s not in seeds]
    per_step = world * P
    if mode == "shard":
        step_seeds = [seeds[(i * per_step + q) % len(seeds)] for i in range(steps) for q in range(per_step)]
    else:
        step_seeds = [seeds[i % len(seeds)] for i in range(steps) for q in range(per_step)]
    sched = [step_seeds[i * per_step:(i + 1) * per_step] for i in range(steps)]
    slot_seeds = [[sched[i][rank * P + j] for i in range(steps)] for j in range(P)]
    return seeds, sched, slot_seeds


def _median(xs):
    xs = [x for x in xs if x is not None]
    return float(np.median(xs)) if xs else None


def reference_iters(cfg_name, rank_tt, seeds):
    """the reference's own iteration count per seed (tests/golden/runs.json, the golden run: 1 BLAS
    thread, PYTHONHASHSEED=0) -- a committed fixture, not the reference"""
    try:
        runs = json.load(open(os.path.join(HERE, "tests", "golden", "runs.json")))
    except (OSError, ValueError):
        return {}
    stem = os.path.splitext(os.path.basename(cfg_name))[0]
    return {s: runs[f"{stem}_r{rank_tt}_s{s}"]["num_iters"] for s in seeds if f"{stem}_r{rank_tt}_s{s}" in runs}


def cpu_summary(per, allc, gpu_runs, cap, workload, cores_avail, ref_iters=None):
    """cpu_baseline from the oracle workers' lines (`_cpu_worker`) and the GPU's per-seed solves.
    Per seed, both sides are WHOLE-solve s/IPM-iter (solve wall / its iterations, the reference
    runner's statistic, src/utils.py:298-302); a CPU process stopped by the safety cap contributes
    its finished-iteration prefix instead and the seed is flagged."""
    gpu = {}
    for r in gpu_runs:
        gpu.setdefault(r["seed"], []).append(r["runtime"] / max(r["num_iters"], 1))
    rows = []
    for c in per:
        if c is None or c["iters"] <= 0:
            continue
        full = "full_solve_s_per_iter" in c
        cs = c["full_solve_s_per_iter"] if full else c["s_per_iter"]
        gs = _median(gpu.get(c["seed"], []))
        rows.append({"seed": c["seed"], "cpu_iters": c.get("full_solve_iters", c["iters"]), "cpu_full_solve": full,
                     "reference_iters": (ref_iters or {}).get(c["seed"]), "cpu_cores": c.get("cores"),
                     "cpu_s_per_iter": cs, "gpu_s_per_iter": gs,
                     "gpu_over_cpu": gs / cs if gs is not None and cs else None})
    cmed = _median([r["cpu_s_per_iter"] for r in rows])
    gmed = _median([r["gpu_s_per_iter"] for r in rows])
    done = [c for c in per if c is not None]
    cpu_iters = sum(c.get("full_solve_iters", c["iters"]) for c in done)
    cpu_wall = max((c["work_s"] for c in done), default=0.0)
    return {"value": cmed, "unit": "s/IPM-iter", "cores": 1, "kind": "port",
            "sample": f"oracle/ CPU restatement of the reference path, {workload}: one single-thread process per "
                      f"timed seed, all at once, each its seed's whole tt_ipm solve (safety cap {cap:g} s); "
                      f"value = median over seeds of solve wall / IPM iterations",
            "seeds_full_solve": sum(r["cpu_full_solve"] for r in rows), "seeds": len(rows),
            "iters_cpu_vs_reference": {str(r["seed"]): [r["cpu_iters"], r["reference_iters"]] for r in rows},
            "hash_seed": "0", "pinned": "one core per worker (sched_setaffinity)",
            "gpu_same_seeds_median": gmed,
            "gpu_over_cpu_ratio_of_medians": (gmed / cmed) if cmed and gmed else None,
            "gpu_over_cpu_median_of_ratios": _median([r["gpu_over_cpu"] for r in rows]),
            "throughput_s_per_iter": cpu_wall / cpu_iters if cpu_iters else None,
            "all_cores": None if allc is None else {
                "seed": allc["seed"], "threads": int(allc["threads"]), "iters": allc["iters"],
                "cpu_s_per_iter": allc["s_per_iter"]},
            "host": {"nproc": os.cpu_count(), "used_cores": len(done), "affinity": cores_avail, "model": _cpu_model()},
            "per_seed": rows}


OUTPUT_SCALARS = ("seed", "num_iters", "gap", "feas", "dual_feas")
OUTPUT_RANKS = ("ranksX", "ranksY", "ranksZ", "ranksT")


def last_step_outputs(all_results):
    """What the last timed step computed, as float64 arrays: one row per solve of that step (each
    slot's last solve), ordered by (rank, slot).  The columns are what `ttipm_amd.utils.solve`, the
    timed call, hands its caller: the seed, the IPM iteration count, the recorded duality gap and
    squared primal / dual feasibility residuals of the end point, and its TT ranks (X, Y, Z, T).
    The seeds of a step follow from the arguments alone (`make_schedule`) and each solve starts from
    its seed's problem and MT19937 state, so two runs with the same arguments solve identical inputs
    row for row.  (`--balance dynamic` hands the solves out first come first served: there a row is
    whatever its slot solved last.)"""
    last = {}
    for r in all_results:
        key = (r.get("rank", 0), r["slot"])
        if key not in last or r["nth"] > last[key]["nth"]:
            last[key] = r
    rows = [last[k] for k in sorted(last)]
    out = {k: np.array([r[k] for r in rows], dtype=np.float64) for k in OUTPUT_SCALARS}
    for k in OUTPUT_RANKS:
        out[k] = np.array([r[k] for r in rows], dtype=np.float64).reshape(len(rows), -1)
    return out


def dump_outputs(path, all_results):
    """`--dump-outputs DIR`: `last_step_outputs` as DIR/<name>.npy (a few hundred bytes each)."""
    os.makedirs(path, exist_ok=True)
    for name, a in last_step_outputs(all_results).items():
        np.save(os.path.join(path, name + ".npy"), a)


LINE_MAX = 4000  # the driver keeps a ~14.8 KB tail of stdout; the line stays far below it


def compose_line(problem, config, cfg_name, rank_tt, world, P, T, n_procs, steps, warmup, schedule, elapsed, iters,
                 seeds, sched, all_results, solo, roofline, cpu, detail_path, balance="static"):
    """(the ONE stdout JSON line, the detail dict for the side file).  The line holds the contract's
    keys plus the summary statistics and stays below LINE_MAX bytes at any N; everything per seed /
    per step / per op goes to the detail file."""
    per_seed, by_seed = [], {}
    for r in all_results:
        per_seed.append({k: r[k] for k in ("seed", "num_iters", "runtime", "sec_per_iter", "gap", "feas",
                                           "dual_feas")})
        per_seed[-1]["pathological"] = bool(r["feas"] > 1e-3 or r["gap"] > 1e-3)  # src/utils.py:67
        acc = by_seed.setdefault(r["seed"], [0.0, 0])
        acc[0] += r["runtime"]
        acc[1] += r["num_iters"]
    inflight_med = _median([t / max(n, 1) for t, n in by_seed.values()])
    solo_med = None if not solo else _median([r["runtime"] / max(r["num_iters"], 1) for r in solo])
    value = elapsed / max(iters, 1)
    rl = None
    if roofline is not None:
        rl = {k: v for k, v in roofline.items() if k != "algorithmic_by_op"}
    cb = None
    if cpu is not None:
        cb = {k: v for k, v in cpu.items() if k != "per_seed"}
    knobs = {k: v for k, v in sorted(os.environ.items()) if k.startswith(("TTK_", "TTIPM_", "GPU_MAX_HW_QUEUES"))}
    line = {"metric": METRIC, "value": value, "unit": "s/IPM-iter", "n_gpus": world,
            "steps": steps, "warmup": warmup, "ms_per_step": elapsed * 1e3 / max(steps, 1),
            "higher_is_better": False, "scaling": "weak", "vs_baseline": None, "dtype": "f64",
            "data": "synthetic: the reference's generators (seeded MT19937 graph TT), problems broadcast from rank 0",
            "config": {"workload": f"{problem} dim={config['dim']} rank={rank_tt} ({cfg_name}), {P} concurrent "
                                   f"tt_ipm solves per GPU per step ({n_procs} processes x {T} slot threads)",
                       "inflight_per_gpu": P, "seeds": seeds, "balance": balance,
                       "parallelism": f"seed-parallel x{world} GPUs x{P} in flight ({schedule})",
                       "solves": len(all_results), "total_ipm_iters": iters},
            # SURVEY.md section 8(d)'s statistic: each seed alone on the GPU, median over seeds
            "sec_per_iter_per_seed_median": solo_med,
            "sec_per_iter_per_seed_median_inflight": inflight_med,
            "roofline": rl, "cpu_baseline": cb,
            "mfma_util_pct": None if rl is None else 100.0 * rl["frac"],
            "pathological_seeds": sorted({p["seed"] for p in per_seed if p["pathological"]}),
            "env_knobs": knobs, "detail": detail_path or None}
    if len(json.dumps(line)) > LINE_MAX:  # never let the line outgrow the driver's tail
        line["env_knobs"] = {"n": len(knobs), "see": "detail"}
    detail = {"line": line, "per_seed": per_seed, "seeds_per_step": sched,
              "solo_per_seed": None if not solo else
              [{k: r[k] for k in ("seed", "num_iters", "runtime", "sec_per_iter", "gap", "feas", "dual_feas")}
               for r in solo],
              "roofline_algorithmic_by_op": None if roofline is None else roofline.get("algorithmic_by_op"),
              "cpu_per_seed": None if cpu is None else cpu["per_seed"], "env_knobs": knobs}
    return line, detail


def write_detail(path, detail, line):
    """The `--detail` side file.  Where it cannot be written (a read-only tree, say) the run and its
    line still stand: the reason goes to stderr and the line's `detail` becomes null."""
    try:
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as f:
            json.dump(detail, f, indent=1)
    except OSError as e:
        print(f"bench: detail file not written: {e}", file=sys.stderr)
        line["detail"] = None


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--config", default=os.path.join(HERE, "configs", "maxcut_10.yaml"))
    ap.add_argument("--problem", default=None, help="default: from the config file name")
    ap.add_argument("--rank", type=int, default=1, help="problem rank (create_problem rank)")
    ap.add_argument("--seeds", default=None, help="comma-separated seeds (default: the config's)")
    ap.add_argument("--cpu-cap", type=float, default=300.0,
                    help="safety bound on seconds of oracle work per seed (0: none); the default covers every "
                         "maxcut_10 seed's whole solve on the GPU box's host")
    ap.add_argument("--detail", default=os.path.join("gpurun_out", "bench_detail.json"),
                    help="side file for the per-seed / per-step / per-op detail ('' to skip)")
    ap.add_argument("--full", action="store_true",
                    help="after the timed steps also run the one-solve-at-a-time latency pass, the roofline "
                         "re-solves and the CPU baseline (each can be switched off below); without it the run is "
                         "set-up, warm-up, the timed steps and the result line only")
    ap.add_argument("--dump-outputs", default=None, metavar="DIR",
                    help="write what the last timed step's solves returned as DIR/<name>.npy (float64)")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: skip the CPU baseline")
    ap.add_argument("--no-roofline", action="store_true", help="with --full: skip the roofline re-solves")
    ap.add_argument("--no-solo", action="store_true",
                    help="with --full: skip the one-solve-at-a-time latency pass")
    ap.add_argument("--schedule", choices=("shard", "replica"), default="shard")
    ap.add_argument("--threads", type=int, default=None,
                    help="solves in flight per process (host threads; default: default_threads())")
    ap.add_argument("--inflight", type=int, default=None,
                    help="solves in flight per GPU (default: default_inflight())")
    ap.add_argument("--balance", choices=("dynamic", "static"), default="static",
                    help="static (default): slot j solves its schedule column; dynamic: the rank's slots claim "
                         "its solves one at a time from a shared counter, in schedule order")
    ap.add_argument("--queue-work", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--slot-base", type=int, default=0, help=argparse.SUPPRESS)
    ap.add_argument("--queue-file", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--cpu-worker", type=int, default=None, help=argparse.SUPPRESS)
    ap.add_argument("--cpu-cores", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--gpu-worker", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.problem is None:
        base = os.path.basename(args.config)
        args.problem = next(p for p in ("maxcut", "corr_clust", "graphm", "max_stable_set") if base.startswith(p))
    if args.cpu_worker is not None:
        return _cpu_worker(args.problem, args.config, args.cpu_worker, args.rank, args.cpu_cap,
                           [int(c) for c in args.cpu_cores.split(",")] if args.cpu_cores else None)
    if args.gpu_worker is not None:
        q = None
        if args.queue_file:
            q = ([int(x) for x in args.queue_work.split(",")], args.queue_file)
        return _gpu_worker(args, [[int(x) for x in sl.split(",")] for sl in args.gpu_worker.split(";")], q)
    if not args.full:  # a plain run: nothing but what `value` needs
        args.no_cpu_baseline = args.no_roofline = args.no_solo = True

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    hwq = int(os.environ.get("TTIPM_HW_QUEUES", str(HW_QUEUES)))
    if not _profiled() and int(os.environ.get("GPU_MAX_HW_QUEUES", "4")) != hwq:
        # before anything initialises HIP here (and inherited by the GPU worker processes)
        os.environ["GPU_MAX_HW_QUEUES"] = str(hwq)
    with open(args.config) as f:
        config = yaml.safe_load(f)
    P = args.inflight if args.inflight else default_inflight(world)
    if _profiled() and (P > 1 or not args.no_cpu_baseline):
        # a profiler's preloaded library has initialised the GPU already: no child processes
        print("bench: under a profiler -> --inflight 1 --no-cpu-baseline", file=sys.stderr)
        P, args.no_cpu_baseline = 1, True
    seeds, sched, slot_seeds = make_schedule(config, os.path.basename(args.config), args.seeds, args.steps, world,
                                             rank, P, args.schedule)
    step_seeds = [s for st in sched for s in st]
    per_step = world * P
    T = max(1, min(args.threads or default_threads(world, P), P))
    if _profiled():
        T = 1
    proc_slots = [slot_seeds[i:i + T] for i in range(0, P, T)]  # this process: proc_slots[0]
    queue = None
    if args.balance == "dynamic":
        # the rank's K x P solves in schedule order (step by step, slot by slot), claimed one at a time
        import tempfile
        work = [sched[i][rank * P + j] for i in range(args.steps) for j in range(P)]
        fd, qpath = tempfile.mkstemp(prefix=f"ttipm_bench_r{rank}_", suffix=".q")
        os.write(fd, b"0")
        os.close(fd)
        _TEMP_FILES.append(qpath)
        queue = (work, qpath)
    gpu_procs = _spawn_gpu_workers(args, proc_slots[1:], queue, base=len(proc_slots[0]))  # before any GPU call

    cpu_seeds = list(dict.fromkeys(s for sl in slot_seeds for s in sl))  # the distinct seeds this (only) rank times
    cpu_procs, allcore_proc = [], []
    do_cpu = rank == 0 and world == 1 and not args.no_cpu_baseline
    cores = min(len(os.sched_getaffinity(0)), HOST_SHARE)
    if do_cpu:  # before any GPU call
        # the host share's cores, one single-thread oracle process each, the timed seeds cycled: the
        # per-seed latency AND the CPU's whole-job throughput come from the same concurrent run
        # one single-thread oracle process per distinct timed seed, whole solves (the reference
        # runner's statistic, src/utils.py:298-302), plus one seed on all the share's cores as BLAS
        # threads (bounded: a side figure)
        # the share's last cores, one per seed (the GPU processes are done by the time they run: the
        # workers are released after the GPU's timed region and solo solves)
        share = sorted(os.sched_getaffinity(0))[-cores:]
        cpu_procs = _spawn_cpu_workers(args, cpu_seeds, [1] * len(cpu_seeds), args.cpu_cap, share[::-1])
        allcore_proc = _spawn_cpu_workers(args, cpu_seeds[:1], [cores], min(args.cpu_cap or 60.0, 60.0), share)

    import torch
    import torch.distributed as dist
    _hip_schedule()
    if torch.cuda.is_available():
        # one process per GPU; more ranks than GPUs only in rehearsals (TTIPM_BENCH_BACKEND=gloo)
        torch.cuda.set_device(local % torch.cuda.device_count())
    if world > 1:
        backend = os.environ.get("TTIPM_BENCH_BACKEND") or ("nccl" if torch.cuda.is_available() else "gloo")
        dist.init_process_group(backend)
    from ttipm_amd import dev as D
    from ttipm_amd import shard
    from ttipm_amd._lib import lib
    from ttipm_amd.utils import solve as _solve

    def solve(prep, trace=None):
        with contextlib.redirect_stdout(sys.stderr):  # stdout carries only the JSON line
            return _solve(prep, config, quiet=True, verbose=False, trace=trace)

    distinct = list(dict.fromkeys(step_seeds))
    with contextlib.redirect_stdout(sys.stderr):
        packed = dict(zip(distinct, shard.broadcast_problems(args.problem, config, distinct, args.rank)))

    def sync():
        if torch.cuda.is_available():
            torch.cuda.synchronize()

    def barrier():
        if world > 1:
            dist.barrier()

    dev_idx = torch.cuda.current_device() if torch.cuda.is_available() else None

    def solve_quiet(prep, trace=None):  # slot threads: stdout is redirected once around them all
        return _solve(prep, config, quiet=True, verbose=False, trace=trace)

    with contextlib.redirect_stdout(sys.stderr):
        sync()
        slots = _Slots(proc_slots[0], packed, solve_quiet, args.warmup, dev_idx, queue=queue)
        slots.wait_ready()
    for p in gpu_procs:  # every worker warmed up and waiting
        line = p.stdout.readline()
        while line and line.strip() != "ready":
            line = p.stdout.readline()
        if not line:
            raise RuntimeError("bench: a GPU worker failed before the timed region")
    barrier()
    sync()
    t0 = time.perf_counter()
    for p in gpu_procs:
        p.stdin.write("go\n")
        p.stdin.flush()
    with contextlib.redirect_stdout(sys.stderr):
        slots.start()
        slot_elapsed, results = slots.join()
    worker_out = []
    for p in gpu_procs:
        line = p.stdout.readline()
        while line and not line.startswith("{"):
            line = p.stdout.readline()
        if p.wait() != 0 or not line:
            raise RuntimeError("bench: a GPU worker failed in the timed region")
        worker_out.append(json.loads(line))
    sync()
    barrier()
    elapsed = time.perf_counter() - t0
    slot_elapsed = slot_elapsed + [e for w in worker_out for e in w["elapsed"]]
    results = results + [r for w in worker_out for r in w["results"]]
    iters = sum(r["num_iters"] for r in results)
    for r in results:
        r["rank"] = rank
    if world > 1:
        t = torch.tensor([elapsed], dtype=torch.float64, device="cuda" if torch.cuda.is_available() else "cpu")
        n = torch.tensor([float(iters)], dtype=torch.float64, device=t.device)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        dist.all_reduce(n, op=dist.ReduceOp.SUM)
        elapsed, iters = float(t.item()), int(n.item())
    all_results = shard.gather_results(results)
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, all_results)

    roofline = None
    if not args.no_roofline and rank == 0:
        # every distinct seed this rank timed, re-solved once with each contraction launch bracketed by
        # HIP events on its stream (untimed for `value`): the same seed mix as the timed region, so a
        # rocprofv3 --stats pass over the same command averages the same kernels
        roof_seeds = list(dict.fromkeys(s for sl in slot_seeds for s in sl))
        st = (ctypes.c_double * 5)()
        lib.ttk_contract_stats(st, 1)
        lib.ttk_contract_timing(1)
        D.ALGO = {"flops": 0.0, "calls": 0, "by": {}}
        s0, l0 = lib.ttk_sync_count(), lib.ttk_launch_count()
        its = 0
        try:
            for sd in roof_seeds:
                its += solve(shard.unpack(*packed[sd]))["num_iters"]
            sync()
        finally:
            lib.ttk_contract_timing(0)
            algo, D.ALGO = D.ALGO, None
        syncs, all_launches = lib.ttk_sync_count() - s0, lib.ttk_launch_count() - l0
        lib.ttk_contract_stats(st, 1)
        flops, launches, tflops, tl, tms = list(st)
        ns = max(len(roof_seeds), 1)
        if tms > 0:
            ach = algo["flops"] / (tms * 1e-3)
            roofline = {"bound": "mfma", "achieved": ach / 1e12, "peak": FP64_MATRIX_PEAK / 1e12,
                        "unit": "TFLOP/s", "frac": ach / FP64_MATRIX_PEAK, "traffic": _pmc_traffic(),
                        "kernel": "contraction kernels: gemm_offs* (fp64 MFMA offset-table GEMM), fused local "
                                  "apply, Schur multi-task apply; traffic = HBM bytes per gemm_offs launch",
                        "seeds": roof_seeds, "algorithmic_flops_per_solve": algo["flops"] / ns,
                        "algorithmic_calls_per_solve": algo["calls"] / ns, "device_flops_per_solve": tflops / ns,
                        "launches_per_solve": tl / ns, "kernel_ms_per_solve": tms / ns,
                        "all_launches_per_ipm_iter": all_launches / max(its, 1),
                        "host_syncs_per_ipm_iter": syncs / max(its, 1),
                        "avg_launch_us": tms * 1e3 / max(tl, 1),
                        "algorithmic_flops_per_launch": algo["flops"] / max(tl, 1),
                        "algorithmic_by_op": dict(sorted(algo["by"].items(), key=lambda kv: -kv[1][1])[:10])}

    # SURVEY.md §8(d)'s per-seed statistic as the reference runner measures it (src/utils.py:300-302:
    # one solve at a time): every distinct timed seed solved once more, alone on the GPU (untimed
    # for `value`; rank 0 at N=1)
    solo = None
    if rank == 0 and world == 1 and not args.no_solo:
        solo = []
        for sd in dict.fromkeys(step_seeds):
            tr = []
            r = solve(shard.unpack(*packed[sd]), trace=tr)
            r["assembly_t"] = [e["t"] - tr[0]["t"] for e in tr] if tr else []
            solo.append(r)
        sync()

    cpu = None
    if do_cpu:
        with contextlib.redirect_stdout(sys.stderr):
            per = _release(cpu_procs)
            allc = _release(allcore_proc)[0]
        gpu_side = solo or results  # the GPU's one-at-a-time latency when measured
        cpu = cpu_summary(per, allc, gpu_side, args.cpu_cap,
                          f"{args.problem} dim={config['dim']} rank={args.rank}", cores_avail=cores,
                          ref_iters=reference_iters(args.config, args.rank, cpu_seeds))

    if rank == 0:
        line, detail = compose_line(
            problem=args.problem, config=config, cfg_name=os.path.basename(args.config), rank_tt=args.rank,
            world=world, P=P, T=T, n_procs=len(proc_slots), steps=args.steps, warmup=args.warmup,
            schedule=args.schedule, elapsed=elapsed, iters=iters, seeds=seeds, sched=sched,
            all_results=all_results, solo=solo, roofline=roofline, cpu=cpu, detail_path=args.detail,
            balance=args.balance)
        if args.detail:
            write_detail(args.detail, detail, line)
        print(json.dumps(line), flush=True)
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    try:
        main()
    finally:
        _reap_children()
