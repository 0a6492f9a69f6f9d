"""Several independent affine roundings in one launch on the MI355X (`ttk_affine_round_many`,
csrc/ttk_retract.hip: one workgroup per job, the jobs' records in a device table): every job bit for bit against its
own `ttk_affine_round_one` call in batches that mix workgroup widths, modes and term kinds, against the
reference's outputs (tests/golden/affine_round.npz), and the launch, host-wait, isolation, validation and fallback
contracts; then the rewired groups of tt_ipm.py and one whole solve, switch on against off.  Off by default
(TTIPM_AFFINE_ROUND_MANY); the tests switch it on by monkeypatch.  The CPU side: tests/test_host_affine_many.py."""
import ctypes
import json
import os

import numpy as np
import pytest

from tests import affine_many_cases as MC
from tests import affine_round_cases as AC

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def T():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from ttipm_amd import tt_ops
    assert hasattr(tt_ops.D.lib, "ttk_affine_round_many")
    return tt_ops


@pytest.fixture
def on(T, monkeypatch):
    monkeypatch.setattr(T, "AFFINE_ROUND_ONE", True)
    monkeypatch.setattr(T, "AFFINE_ROUND_MANY", True)
    return T


_DEV = {}


def _dev(T, cid):
    """the case's distinct trains on the device, uploaded once per module and never written"""
    if cid not in _DEV:
        _DEV[cid] = [T.to_device(t) for t in AC.stored(cid)]
        for t in _DEV[cid]:
            T.D.read(t[0])
    return _DEV[cid]


def _read_launches(T):
    """what one host read adds to `ttk_launch_count` besides its one host wait: the library may read through a
    copy kernel of its own (1), or through a plain copy (0).  A path's rounding launches are its launches less
    this per host wait."""
    D = T.D
    x = D.empty(4)
    D.read(x)
    l0, s0 = D.lib.ttk_launch_count(), D.lib.ttk_sync_count()
    D.read(x)
    assert D.lib.ttk_sync_count() - s0 == 1
    return D.lib.ttk_launch_count() - l0


def _bits(x):
    return np.ascontiguousarray(x).view(np.int64)


def _single(T, cid, dev=None):
    """`ttk_affine_round_one` alone on the case: (written front of every out buffer, the d + 3 info words)"""
    D = T.D
    terms, mids = T._affine_norm(AC.terms(cid, _dev(T, cid) if dev is None else dev), AC.mids(cid))
    (d, inner, rows, n, arr), sums, bound, keep = T._affine_round_one_plan(terms, mids)
    outs = T._packed_flat(bound, list(inner))
    info = D.empty(d + 3)
    D._stream()
    rc = D.lib.ttk_affine_round_one(D.ctx(), d, inner, rows, n, arr, AC.eps(cid), AC.mode(cid),
                                    (ctypes.c_void_p * d)(*[o.data_ptr() for o in outs]), info.data_ptr())
    assert rc == 0
    got = D.read(info)
    q = [int(v) for v in got[:d + 1]]
    return [D.read(o[:q[k] * inner[k] * q[k + 1]]) for k, o in enumerate(outs)], got


_SINGLE = {}


def _single_once(T, cid):
    """the single call's bits of the case, computed once per module and shared"""
    if cid not in _SINGLE:
        _SINGLE[cid] = _single(T, cid)
    return _SINGLE[cid]


def _many(T, batch, devs=None):
    """`ttk_affine_round_many` itself on the cases of `batch`: (status, per job (fronts, info words), (launches,
    waits), the planned thread counts)"""
    D = T.D
    devs = [_dev(T, c) for c in batch] if devs is None else devs
    norm, plans, table = T._affine_many_plan([MC.public_job(c, dv) for c, dv in zip(batch, devs)])
    nj = len(batch)
    outs, keep = [], []
    for j, plan in enumerate(plans):
        (d, inner, _, _, _), _, bound, _ = plan
        o = T._packed_flat(bound, list(inner))
        p = (ctypes.c_void_p * d)(*[x.data_ptr() for x in o])
        outs.append(o)
        keep.append(p)
        table[j].out = ctypes.cast(p, ctypes.c_void_p)
    off, th = (ctypes.c_int64 * (nj + 1))(), (ctypes.c_int * nj)()
    assert D.lib.ttk_affine_round_many_lds(nj, table, off, th) >= 0
    info = D.empty(int(off[nj]))
    D._stream()
    D.read(info)  # the allocations are done
    l0, s0 = D.lib.ttk_launch_count(), D.lib.ttk_sync_count()
    rc = D.lib.ttk_affine_round_many(D.ctx(), nj, table, info.data_ptr())
    counts = (D.lib.ttk_launch_count() - l0, D.lib.ttk_sync_count() - s0)
    got = D.read(info)
    res = []
    for j, plan in enumerate(plans):
        d, inner = plan[0][0], list(plan[0][1])
        g = got[int(off[j]):int(off[j + 1])]
        assert g.shape == (d + 3,)
        q = [int(v) for v in g[:d + 1]]
        res.append(([D.read(o[:q[k] * inner[k] * q[k + 1]]) for k, o in enumerate(outs[j])], g))
    return rc, res, counts, list(th)


def _assert_same(a, b, what):
    (fa, ia), (fb, ib) = a, b
    assert np.array_equal(_bits(ia), _bits(ib)), what
    assert len(fa) == len(fb)
    for x, y in zip(fa, fb):
        assert x.shape == y.shape and np.array_equal(_bits(x), _bits(y)), what


@pytest.mark.parametrize("batch", MC.BATCHES, ids="-".join)
def test_every_job_has_the_bits_of_its_single_call(T, batch):
    """a batch that mixes two workgroup widths (asserted), modes and term kinds: one launch, no host wait; every
    job's output cores and d + 3 info words are those of `ttk_affine_round_one` alone on the job, its ranks the
    reference's, its tensor the reference's to 1e-11, the tracked job's tail the reference's factor"""
    rc, res, counts, th = _many(T, batch)
    assert rc == 0 and counts == (1, 0)
    assert len(set(th)) >= 2, th
    for cid, one in zip(batch, res):
        _assert_same(one, _single_once(T, cid), cid)
        fronts, info = one
        d = len(fronts)
        assert [float(v) for v in info[:d + 1]] == [float(q) for q in AC.qranks(cid)]
        q = [int(v) for v in info[:d + 1]]
        cores = [f.reshape(q[k], *AC.mids(cid), q[k + 1]) for k, f in enumerate(fronts)]
        if AC.mode(cid) == 0:
            assert info[d + 1] == 0.0
        else:
            assert abs(info[d + 1] ** (1.0 / (2 * d)) - AC.factor(cid)) <= 1e-11 * AC.factor(cid)
        AC.check_result(cid, AC.finish(T, cid, T.to_device(cores)))
    T.D.check_handoffs()


def test_public_call_is_one_launch_and_one_wait(on):
    """the public function on N jobs: 1 launch and 1 host wait, every job the reference's result; the same jobs
    through `tt_affine_rank_reduce`: N launches and N host waits (a host wait may bring the read's own copy kernel:
    `_read_launches`)"""
    T, D = on, on.D
    r = _read_launches(T)
    batch = MC.BATCHES[1]
    jobs = [MC.public_job(c, _dev(T, c)) for c in batch]
    assert T.affine_round_many_lds(jobs) == max(T.affine_round_one_lds(j[0], j[3]) for j in jobs) > 0
    D._stream()
    l0, s0 = D.lib.ttk_launch_count(), D.lib.ttk_sync_count()
    res = T.tt_affine_rank_reduce_many(jobs)
    assert (D.lib.ttk_launch_count() - l0, D.lib.ttk_sync_count() - s0) == (1 + r, 1)
    l0, s0 = D.lib.ttk_launch_count(), D.lib.ttk_sync_count()
    seq = [T.tt_affine_rank_reduce(t, e, True, m) for t, e, _, m in jobs]  # no tracked job in this batch
    assert (D.lib.ttk_launch_count() - l0, D.lib.ttk_sync_count() - s0) == (len(batch) * (1 + r), len(batch))
    import torch
    for cid, one, (tt, n2) in zip(batch, res, seq):
        assert one[1] is None and np.float64(one[2]).view(np.int64) == np.float64(n2).view(np.int64)
        assert [c.shape for c in one[0]] == [c.shape for c in tt] and all(torch.equal(a, b) for a, b in zip(one[0], tt))
        AC.check_result(cid, MC.finish(T, cid, one))
    D.check_handoffs()


def test_jobs_are_isolated(T):
    """the same job 8 times: 8 outputs with equal bits, those of the single call; two jobs that share an input
    train leave it unchanged; two calls give the same bits; one job alone gives the single call's bits"""
    for cid in ("y", "z"):  # 256 and 1024 threads
        rc, res, counts, th = _many(T, (cid,) * 8)
        assert rc == 0 and counts == (1, 0) and len(set(th)) == 1
        for one in res:
            _assert_same(one, _single_once(T, cid), cid)
    host = AC.stored("r")
    dev = [T.to_device(t) for t in host]   # r: A x - b; the second job reads the same three trains
    rc, res, _, _ = _many(T, ("r", "r", "f"), [dev, dev, _dev(T, "f")])
    assert rc == 0
    assert all(np.array_equal(T.D.read(x), y) for t, h in zip(dev, host) for x, y in zip(t, h))
    _assert_same(res[0], res[1], "shared input")
    _assert_same(res[0], _single_once(T, "r"), "r")
    _assert_same(res[2], _single_once(T, "f"), "f")
    first = _many(T, MC.BATCHES[0])[1]
    again = _many(T, MC.BATCHES[0])[1]
    for cid, a, b in zip(MC.BATCHES[0], first, again):
        _assert_same(a, b, cid)
    for cid in ("t", "s"):
        rc, res, counts, _ = _many(T, (cid,))
        assert rc == 0 and counts == (1, 0)
        _assert_same(res[0], _single_once(T, cid), cid)
    T.D.check_handoffs()


def test_validation_returns_an_error_without_launching(T):
    """`njobs` 0 and 9, a null table, a null info, one invalid job among valid ones and one that does not fit:
    TTK_ERR_ARG from the host-side checks, the message names the function, no launch; the valid call on the same
    buffers still runs afterwards"""
    from ttipm_amd._lib import TTK_ERR_ARG, AffineJob
    D = T.D
    batch = ("r", "u", "g")
    plans = [T._affine_many_plan([MC.public_job(c, _dev(T, c))]) for c in batch]
    keep, recs, bufs = [], [], []
    for _, (plan,), table in plans:
        (d, inner, _, _, _), _, bound, _ = plan
        o = T._packed_flat(bound, list(inner))
        p = (ctypes.c_void_p * d)(*[x.data_ptr() for x in o])
        keep.append(p)
        bufs.append(o)
        table[0].out = ctypes.cast(p, ctypes.c_void_p)
        recs.append(table[0])
    # case j has no plan on the Python side (it does not fit): its record is written by hand from its ranks, the
    # core tables pointing at one host double that the rejected call never reads
    from tests import test_host_affine_round as H
    jt = AC.stored("j")
    jin, _ = AC.inner_and_ranks("j", jt)
    jarr, jkeep = H.Plan().records(3, H._plan_terms("j", jt))
    xi = H._arr(jin)
    nofit = AffineJob(3, H._addr(xi), None, len(AC.kinds("j")), H._addr(jarr), AC.eps("j"), 0, recs[0].out)
    info = D.empty(64)
    D._stream()
    D.read(info)
    l0 = D.lib.ttk_launch_count()

    def copy(rec, **change):
        new = AffineJob(*[getattr(rec, f) for f, _ in AffineJob._fields_])
        for k, v in change.items():
            setattr(new, k, v)
        return new

    def call(jobs, n=None, null=False, inf=info.data_ptr()):
        tab = (AffineJob * max(len(jobs), 1))(*jobs)
        return D.lib.ttk_affine_round_many(D.ctx(), len(jobs) if n is None else n, None if null else tab, inf)

    def bad(*a, **kw):
        assert call(*a, **kw) == TTK_ERR_ARG
        assert b"ttk_affine_round_many" in D.lib.ttk_last_error()

    bad(recs, n=0)
    bad([recs[0]] * 9)
    bad(recs, null=True)
    bad(recs, inf=None)
    for at in range(len(recs) + 1):
        bad(recs[:at] + [nofit] + recs[at:])                                  # a job that does not fit
        for change in (dict(eps=-1.0), dict(mode=2), dict(d=1), dict(inner=None), dict(terms=None), dict(nterms=5),
                       dict(out=None)):
            bad(recs[:at] + [copy(recs[0], **change)] + recs[at:])            # an invalid job among valid ones
    bad(recs[:2] + [copy(recs[2], rows=None)])                                # g has a transposed term: needs rows
    nullout = (ctypes.c_void_p * 3)(bufs[0][0].data_ptr(), None, bufs[0][2].data_ptr())
    bad([recs[1], copy(recs[0], out=ctypes.cast(nullout, ctypes.c_void_p))])  # a null out core
    assert D.lib.ttk_launch_count() == l0
    assert call(recs) == 0
    assert D.lib.ttk_launch_count() == l0 + 1
    got = D.read(info)
    assert [int(v) for v in got[:4]] == AC.qranks("r") and [int(v) for v in got[6:10]] == AC.qranks("u")
    D.check_handoffs()


def test_group_with_a_job_that_does_not_fit_goes_job_by_job(on):
    """case j among fitting cases: no batched launch, every job through the public single path (the fitting ones
    one launch each, j composed), and still every reference result"""
    T, D = on, on.D
    batch = ("u", "j", "t")
    devs = {c: (_dev(T, c) if c != "j" else [T.to_device(t) for t in AC.stored("j")]) for c in batch}
    jobs = [MC.public_job(c, devs[c]) for c in batch]
    assert T.affine_round_many_lds(jobs) == -1 and T._affine_many_native(jobs) is None
    l0, s0 = D.lib.ttk_launch_count(), D.lib.ttk_sync_count()
    res = T.tt_affine_rank_reduce_many(jobs)
    assert D.lib.ttk_launch_count() - l0 > 4 and D.lib.ttk_sync_count() - s0 > 2
    for cid, one in zip(batch, res):
        assert (one[1] is not None) == bool(AC.mode(cid))
        AC.check_result(cid, MC.finish(T, cid, one))
    _assert_same(([D.read(c).reshape(-1) for c in res[0][0]], np.zeros(0)),
                 (_single_once(T, "u")[0], np.zeros(0)), "u")  # the fitting job took `ttk_affine_round_one`
    D.check_handoffs()


# ------------------------------------------------------------------ the rewired groups of tt_ipm.py
@pytest.fixture
def siblings(T, monkeypatch):
    """the three sibling switches on: the sequential code then makes the single calls whose bits the batch keeps"""
    for name in ("ROUND_ONE", "SUM_ROUND_ONE", "AFFINE_ROUND_ONE"):
        monkeypatch.setattr(T, name, True)
    return T


def _on_off(T, monkeypatch, f):
    """f() with the switch off, then on: per run (result, launches, host waits, MT19937 state afterwards)"""
    D = T.D
    runs = []
    for switch in (False, True):
        monkeypatch.setattr(T, "AFFINE_ROUND_MANY", switch)
        np.random.seed(13)
        D._stream()
        l0, s0 = D.lib.ttk_launch_count(), D.lib.ttk_sync_count()
        res = f()
        runs.append((res, D.lib.ttk_launch_count() - l0, D.lib.ttk_sync_count() - s0, np.random.get_state()))
    (_, l_off, w_off, st_off), (_, l_on, w_on, st_on) = runs
    assert np.array_equal(st_off[1], st_on[1]) and st_off[2:] == st_on[2:]
    np.random.seed(13)
    return runs[0][0], runs[1][0], (l_off, w_off), (l_on, w_on), np.random.get_state()


def _same_trains(a, b):
    import torch
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert (x is None) == (y is None)
        if x is not None:
            assert [c.shape for c in x] == [c.shape for c in y] and all(torch.equal(c, e) for c, e in zip(x, y))


def _same_float(a, b):
    assert np.float64(a).view(np.int64) == np.float64(b).view(np.int64), (a, b)


@pytest.mark.parametrize("active", (False, True), ids=("inactive", "active"))
def test_newton_system_groups_keep_their_bits(siblings, monkeypatch, active):
    """`tt_infeasible_newton_system` on the d = 3 state: the two residuals and the two Kronecker blocks, switch on
    against off: the same bits in every train, the same residual norms, the same MT19937 state, strictly fewer
    launches and host waits.  Active: the dual residual's second rounding stays behind the batch."""
    from ttipm_amd import tt_ipm
    T = siblings
    st0, v = AC.ipm_state(T, tt_ipm, active=active)

    def run():
        s = tt_ipm.IPMStatus(3, 1e-3, 1e-3, 1e-5, 1e-12, False, False, np.inf, False, np.inf, True, np.inf, np.inf,
                             False, st0.ineq_status, False, 3.0, 2.5, 1000)
        s.lag_map_t = T.tt_diag_op(v["mask"], s.eps)
        lhs = {}
        _, rhs, s = tt_ipm.tt_infeasible_newton_system(lhs, v["C"], v["X"], v["Y"], v["Z"], v["Tt"] if active else None,
                                                       v["L"], v["Ladj"], v["b"], v["mask"], s)
        return lhs, rhs, s

    (l0, r0, s0), (l1, r1, s1), off, on, fresh = _on_off(T, monkeypatch, run)
    _same_trains([l0[2, 1], l0[2, 2]], [l1[2, 1], l1[2, 2]])
    _same_trains([r0.get_row(i) for i in (0, 1)], [r1.get_row(i) for i in (0, 1)])
    assert r0.get_row(0) is not None and r0.get_row(1) is not None
    _same_float(s0.primal_error, s1.primal_error)
    _same_float(s0.dual_error, s1.dual_error)
    assert on[0] < off[0] and on[1] < off[1], (off, on)
    r = _read_launches(T)
    assert on == (off[0] - 2 * (1 + r), off[1] - 2)  # two groups of two: one launch and one wait saved by each
    T.D.check_handoffs()


def _solution(T, blocks):
    """a synthetic Newton solution, d = 3: a block train whose middle core carries the block index"""
    rng = np.random.default_rng(20270107)
    return T.to_device([rng.standard_normal((1, 4, 2)), rng.standard_normal((2, blocks, 4, 2)),
                        rng.standard_normal((2, 4, 1))])


@pytest.mark.parametrize("active", (False, True), ids=("inactive", "active"))
def test_newton_step_groups_keep_their_bits(siblings, monkeypatch, active):
    """the predictor's and the corrector's blocks (`_step_blocks_many`) and the corrector's sums
    (`_add_round_many`) against the expressions of `_tt_ipm_newton_step` they stand for: the same bits, the same
    MT19937 state, which has moved (the two symmetrisations draw), one launch and one host wait per group"""
    from ttipm_amd import tt_ipm
    T = siblings
    st, _ = AC.ipm_state(T, tt_ipm, active=active)
    Dl, Dc = _solution(T, 4 if active else 3), _solution(T, 4 if active else 3)
    Dc = [T.D.scaled(c, 0.5) if k == 0 else c for k, c in enumerate(Dc)]
    get = tt_ipm._tt_get_block

    def blocks_old(S):
        DX = tt_ipm._tt_symmetrise(T.tt_reshape(get(1, S), (2, 2)), st.eps)
        DZ = tt_ipm._tt_symmetrise(T.tt_reshape(get(2, S), (2, 2)), st.eps)
        DY = T.tt_rank_reduce(get(0, S), eps=st.eps)
        return DX, DZ, DY, (T.tt_rank_reduce(get(3, S), eps=st.eps) if active else None)

    def blocks(S):
        res = tt_ipm._step_blocks_many(S, active, st)
        assert (res is not None) == T.AFFINE_ROUND_MANY
        return blocks_old(S) if res is None else res

    old, new, off, on, fresh = _on_off(T, monkeypatch, lambda: blocks(Dl))
    _same_trains(old, new)
    n, r = 4 if active else 3, _read_launches(T)
    assert off[1] == n and on == (off[0] - (n - 1) * (1 + r), 1), (off, on)
    monkeypatch.setattr(T, "AFFINE_ROUND_MANY", False)
    np.random.seed(13)
    blocks_old(Dl)
    moved = np.random.get_state()
    assert not (np.array_equal(fresh[1], moved[1]) and fresh[2] == moved[2])
    pre, cor = blocks_old(Dl), blocks_old(Dc)
    pairs = [(c, p) for c, p in zip(cor, pre) if c is not None]

    def sums():
        res = tt_ipm._add_round_many(pairs, st.eps)
        assert (res is not None) == T.AFFINE_ROUND_MANY
        return [tt_ipm._tt_add_round(a, b, st.eps) for a, b in pairs] if res is None else res

    old, new, off, on, _ = _on_off(T, monkeypatch, sums)
    _same_trains(old, new)
    assert off == (n * (1 + r), n) and on == (1 + r, 1), (off, on)
    T.D.check_handoffs()


def test_group_without_a_plan_or_a_sibling_runs_as_it_stands(siblings, monkeypatch):
    """`_fused_many` declines, and the call sites then run their old code: a sibling switch off, a job whose every
    rank is 1 (the sequential code returns it unrounded: it stays out of the launch), a job that does not fit"""
    import torch
    from ttipm_amd import tt_ipm
    T = siblings
    monkeypatch.setattr(T, "AFFINE_ROUND_MANY", True)
    st, v = AC.ipm_state(T, tt_ipm)
    r = _read_launches(T)
    l0 = T.D.lib.ttk_launch_count()
    ok = ([(1.0, v["b"])], st.eps, 0, (), None, "round")
    assert tt_ipm._fused_many([ok, ok]) is not None
    l1 = T.D.lib.ttk_launch_count()
    assert l1 == l0 + 1 + r
    assert tt_ipm._fused_many([ok]) is None and tt_ipm._fused_many([ok] * 9) is None
    ones = ([(1.0, T.tt_reshape(v["mask"], (4,)))], st.eps, 0, (), None, "round")   # the mask has every rank 1
    assert tt_ipm._fused_many([ok, ones]) is None    # one job would remain
    l2 = T.D.lib.ttk_launch_count()
    three = tt_ipm._fused_many([ok, ones, ok])       # it stays out of the launch and comes back as it is
    assert T.D.lib.ttk_launch_count() == l2 + 1 + r
    assert three[1][0] is ones[0][0][1] and three[1][1] is None
    assert all(torch.equal(a, b) for a, b in zip(three[0][0], three[2][0])) and three[0][1] == three[2][1]
    l1 = T.D.lib.ttk_launch_count()
    big = [T.to_device(t) for t in AC.stored("j")]
    assert tt_ipm._fused_many([ok, (AC.terms("j", big), AC.eps("j"), 0, (), AC.mids("j"), "affine")]) is None
    monkeypatch.setattr(T, "ROUND_ONE", False)
    assert tt_ipm._fused_many([ok, ok]) is None
    assert tt_ipm._kron_blocks_many(v["X"], v["Z"], st) is None
    monkeypatch.setattr(T, "ROUND_ONE", True)
    monkeypatch.setattr(T, "SUM_ROUND_ONE", False)
    assert tt_ipm._add_round_many([(v["b"], v["C"]), (v["C"], v["b"])], st.eps) is None
    monkeypatch.setattr(T, "SUM_ROUND_ONE", True)
    monkeypatch.setattr(T, "AFFINE_ROUND_ONE", False)
    assert tt_ipm._fused_many([ok, ok]) is None
    assert T.D.lib.ttk_launch_count() == l1  # nothing was launched by a declined group
    T.D.check_handoffs()


def test_maxcut_5_solve_with_the_switch_on(siblings, monkeypatch):
    """one maxcut dim-5 solve (seed 0) with the three sibling switches on, the new switch on against off: the same
    iteration count and exactly the same gap, fewer launches and fewer host waits, and the gap within smoke()'s
    bound against the reference's own run (1e-6 relative, tests/golden/runs.json)"""
    import yaml
    from ttipm_amd.utils import run_and_record
    T = siblings
    D = T.D
    cfg = yaml.safe_load(open(os.path.join(ROOT, "configs", "maxcut_5.yaml")))
    gold = json.load(open(os.path.join(ROOT, "tests", "golden", "runs.json")))["maxcut_5_r1_s0"]
    got = {}
    for switch in (False, True):
        monkeypatch.setattr(T, "AFFINE_ROUND_MANY", switch)
        l0, s0 = D.lib.ttk_launch_count(), D.lib.ttk_sync_count()
        got[switch] = run_and_record("maxcut", cfg, 0, 1)
        got[switch]["launches"] = D.lib.ttk_launch_count() - l0
        got[switch]["waits"] = D.lib.ttk_sync_count() - s0
        print("switch", switch, "iters", got[switch]["num_iters"], "gap", repr(got[switch]["gap"]), "launches",
              got[switch]["launches"], "waits", got[switch]["waits"])
    assert got[True]["num_iters"] == got[False]["num_iters"]
    assert got[True]["gap"] == got[False]["gap"]
    assert got[True]["launches"] < got[False]["launches"] and got[True]["waits"] < got[False]["waits"]
    assert abs(got[True]["gap"] - gold["gap"]) <= 1e-6 * abs(gold["gap"]), (got[True]["gap"], gold["gap"])
    D.check_handoffs()
