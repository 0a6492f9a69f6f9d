"""Several independent affine roundings in one launch (`ttk_affine_round_many`, reached through
`tt_ops.tt_affine_rank_reduce_many` under TTIPM_AFFINE_ROUND_MANY), the part that needs no device: the C ABI's
declaration and binding, the host side of the plan (`ttk_affine_round_many_lds` is a host function), and the public
function on the CPU (libttk replaced by the NumPy emulator; switch off and on both go job by job through the
composed path there) against the reference's own outputs (tests/golden/affine_round.npz).  The device run:
tests/test_gpu_affine_many.py."""
import ctypes
import os
import re

import numpy as np
import pytest

from tests import affine_many_cases as MC
from tests import affine_round_cases as AC
from tests import test_host_affine_round as H
from tests.emu_ttk import emulated_ttipm

ROOT = H.ROOT
needs_lib = H.needs_lib
I64, VP = MC.I64, MC.VP
NAMES = ("ttk_affine_round_many", "ttk_affine_round_many_lds")


@pytest.fixture(scope="module")
def T():
    emulated_ttipm()
    from ttipm_amd import tt_ops
    return tt_ops


def test_header_and_binding_declare_the_calls():
    txt = open(os.path.join(ROOT, "include", "ttk.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    names = set(re.findall(r"\b(ttk_[a-z0-9_]+)\s*\(", txt))
    assert set(NAMES) <= names
    assert re.search(r"\}\s*ttk_affine_job\s*;", txt)
    assert re.search(r"#define\s+TTK_ROUND_MANY_MAX\s+8\b", txt)
    src = open(os.path.join(ROOT, "tensor-train-interior-point-method_amd", "_lib.py")).read()
    assert all(f'"{n}"' in src for n in NAMES)


@needs_lib
def test_library_exports_the_calls():
    lib = ctypes.CDLL(H.SO)
    assert all(hasattr(lib, n) for n in NAMES)


class Planner(H.Plan):
    """`ttk_affine_round_many_lds` through ctypes on the fixture cases; `ttk_affine_round_one_lds` is H.Plan's"""

    def __init__(self):
        super().__init__()
        self.lib.ttk_affine_round_many_lds.restype = I64
        self.lib.ttk_affine_round_many_lds.argtypes = [ctypes.c_int, VP, VP, VP]
        self.keep = []

    def job(self, cid, **change):
        """the case's job record (out NULL: the planner does not examine it); change: fields to overwrite"""
        trains = AC.stored(cid)
        inner, _ = AC.inner_and_ranks(cid, trains)
        d = len(inner)
        arr, keep = self.records(d, H._plan_terms(cid, trains))
        xi, xr = H._arr(inner), H._arr([AC.mids(cid)[0]] * d)
        self.keep += [arr, keep, xi, xr]
        rec = dict(d=d, inner=H._addr(xi), rows=H._addr(xr), nterms=len(AC.kinds(cid)), terms=H._addr(arr),
                   eps=AC.eps(cid), mode=AC.mode(cid), out=None)
        rec.update(change)
        return MC.Job(**rec)

    def single(self, cid):
        trains = AC.stored(cid)
        return self(AC.inner_and_ranks(cid, trains)[0], H._plan_terms(cid, trains))

    def many(self, jobs, n=None, off=None, threads=None, null=False):
        tab = (MC.Job * max(len(jobs), 1))(*jobs)
        return self.lib.ttk_affine_round_many_lds(len(jobs) if n is None else n, None if null else tab, off, threads)


@needs_lib
def test_plan_of_a_batch_is_the_largest_single_plan_with_prefix_sum_info_offsets():
    plan = Planner()
    widths = set()
    for batch in MC.BATCHES + (AC.FIT[:8], AC.FIT[2:], ("s",), ("t", "t")):
        n = len(batch)
        jobs = [plan.job(c) for c in batch]
        off, th = (I64 * (n + 1))(), (ctypes.c_int * n)()
        got = plan.many(jobs, off=off, threads=th)
        singles = [plan.single(c) for c in batch]
        assert min(singles) >= 0 and got == max(singles), (batch, got, singles)
        ds = [len(AC.ranks(c)) - 1 for c in batch]
        assert list(off) == [sum(d + 3 for d in ds[:j]) for j in range(n + 1)], batch
        assert all(t in (256, 1024) for t in th), (batch, list(th))
        if batch in MC.BATCHES:
            assert len(set(th)) == 2, (batch, list(th))   # each test batch mixes the two workgroup widths
        widths |= set(zip(batch, th))
        assert got == plan.many(jobs) == plan.many(jobs, off=off) == plan.many(jobs, threads=th)  # outputs may be NULL
    assert dict(widths)["z"] == dict(widths)["s"] == 1024 and dict(widths)["c"] == 256


@needs_lib
def test_plan_rejects_a_bad_batch():
    """`njobs` outside 1 .. 8, a NULL table, a job that does not fit (case j) and an invalid job, at every position:
    -1 for the plan call, TTK_ERR_ARG without a launch for the device call (tests/test_gpu_affine_many.py)"""
    plan = Planner()
    ok = [plan.job(c) for c in MC.BATCHES[0]]
    assert plan.many(ok) >= 0 and plan.many(ok[:1]) >= 0
    assert plan.many([], n=0) == -1 and plan.many(ok, n=0) == -1 and plan.many(ok, n=-1) == -1
    nine = [plan.job("c") for _ in range(9)]
    assert plan.many(nine[:8]) >= 0 and plan.many(nine) == -1
    assert plan.many(ok, null=True) == -1
    assert plan.single("j") == -1
    inner_g = AC.inner_and_ranks("g", AC.stored("g"))[0]
    odd = H._arr([AC.mids("g")[0], inner_g[1] + 1] + [AC.mids("g")[0]] * (len(inner_g) - 2))
    bad_jobs = [plan.job("j"),                                   # no fit
                plan.job("r", eps=-1.0), plan.job("r", eps=float("nan")), plan.job("r", mode=2),
                plan.job("r", d=1), plan.job("r", inner=None), plan.job("r", terms=None), plan.job("r", nterms=0),
                plan.job("r", nterms=5),
                plan.job("g", rows=None),                        # a transposed term needs rows
                plan.job("g", rows=H._addr(odd))]                # rows[1] does not divide inner[1]
    for bad in bad_jobs:
        assert plan.many([bad]) == -1
        for at in range(len(ok) + 1):
            assert plan.many(ok[:at] + [bad] + ok[at:]) == -1, at


def _run(T, batch):
    """the batch through the public function: (results, host trains, device trains, their lists as handed in)"""
    host = {c: AC.stored(c) for c in batch}
    dev = {c: [T.to_device(t) for t in host[c]] for c in batch}
    keep = {c: [list(t) for t in dev[c]] for c in batch}
    np.random.seed(7)
    st0 = np.random.get_state()
    res = T.tt_affine_rank_reduce_many([MC.public_job(c, dev[c]) for c in batch])
    st1 = np.random.get_state()
    assert st0[0] == st1[0] and np.array_equal(st0[1], st1[1]) and st0[2:] == st1[2:]  # the same MT19937 state
    return res, host, dev, keep


@pytest.mark.parametrize("switch", (False, True))
@pytest.mark.parametrize("batch", MC.BATCHES + (("u", "j", "t"),), ids="-".join)
def test_public_function_matches_reference(T, monkeypatch, batch, switch):
    """every job: ranks exactly the reference's and the dense tensor to 1e-11, ||tt||^2 to 1e-11 of the dense
    tensor's, a tail factor for the tracked job and for no other; switch off and on (without a GPU both go job by job);
    the callers' tensors and lists are unchanged and nothing is drawn from NumPy's stream"""
    monkeypatch.setattr(T, "AFFINE_ROUND_MANY", switch)
    res, host, dev, keep = _run(T, batch)
    assert len(res) == len(batch)
    for cid, one in zip(batch, res):
        tt, factor, n2 = one
        assert (factor is not None) == bool(AC.mode(cid)), cid
        want = float(np.sum(AC.dense(T.to_host(tt)) ** 2))
        assert abs(float(n2) - want) <= AC.RTOL * want, (cid, float(n2), want)
        AC.check_result(cid, MC.finish(T, cid, one))
        for t, k, h in zip(dev[cid], keep[cid], host[cid]):
            assert len(t) == len(k) and all(x is y for x, y in zip(t, k))
            assert all(np.array_equal(T.D.read(x), y) for x, y in zip(t, h))


def test_switch_is_off_by_default_and_not_taken_off_the_gpu(T, monkeypatch):
    """the switch reads TTIPM_AFFINE_ROUND_MANY; switched on without a GPU the batched call declines, and the
    planner function says whether a batch could run as one launch"""
    assert T.AFFINE_ROUND_MANY is (os.environ.get("TTIPM_AFFINE_ROUND_MANY", "0") == "1")
    assert T.AFFINE_JOBS == MC.MAX_JOBS
    monkeypatch.setattr(T, "AFFINE_ROUND_MANY", True)
    dev = {c: [T.to_device(t) for t in AC.stored(c)] for c in ("r", "u")}
    assert T._affine_many_native([MC.public_job(c, dev[c]) for c in ("r", "u")]) is None
    assert T.affine_round_many_lds([]) == -1
    assert T.affine_round_many_lds([MC.public_job("r", dev["r"])] * 9) == -1
