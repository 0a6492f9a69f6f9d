"""Rounding a weighted sum of trains on the MI355X without building it: the one-launch `ttk_sum_round_one`
(csrc/ttk_retract.hip, the summed cores formed in the kernel's two loads) against the reference's outputs
(tests/golden/sum_round.npz), against the composed path (`tt_add` + `ttk_round`), bit for bit against
`ttk_round_one` on the materialised sum, and its launch, host-wait, determinism, fallback and validation
contracts.  Off by default (TTIPM_SUM_ROUND_ONE); the tests switch it on by monkeypatch.  The same value
checks on the CPU: tests/test_host_sum_round.py."""
import ctypes

import numpy as np
import pytest

from tests import sum_round_cases as SC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def T():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from ttipm_amd import tt_ops
    assert hasattr(tt_ops.D.lib, "ttk_sum_round_one")
    return tt_ops


@pytest.fixture
def on(T, monkeypatch):
    monkeypatch.setattr(T, "SUM_ROUND_ONE", True)
    return T


def _up(T, cid):
    """(host trains, device trains); the case takes the one-launch path and its uploads are done"""
    host = SC.stored(cid)
    dev = [T.to_device(t) for t in host]
    assert T.sum_round_one_lds(SC.terms(cid, dev), SC.transposed(cid)) >= 0
    T.D.read(dev[0][0])
    return host, dev


@pytest.mark.parametrize("cid", SC.FIT)
def test_fused_matches_reference(on, cid):
    T = on
    host, dev = _up(T, cid)
    keep = [list(t) for t in dev]
    s0 = T.D.lib.ttk_sync_count()
    res = SC.public(T, cid, dev)
    assert T.D.lib.ttk_sync_count() - s0 == 1  # the one-launch path ran: one read, of the ranks
    SC.check_result(cid, T.to_host(res))
    for t, k, h in zip(dev, keep, host):  # the caller's lists and tensors are never written
        assert all(a is b for a, b in zip(t, k))
        assert all(np.array_equal(T.D.read(a), b) for a, b in zip(t, h))
    T.D.check_handoffs()


@pytest.mark.parametrize("cid", SC.FIT)
def test_fused_matches_composed_path(T, cid, monkeypatch):
    _, dev = _up(T, cid)
    monkeypatch.setattr(T, "SUM_ROUND_ONE", True)
    new = T.to_host(SC.public(T, cid, dev))
    monkeypatch.setattr(T, "SUM_ROUND_ONE", False)
    old = T.to_host(SC.public(T, cid, dev))
    assert [c.shape for c in new] == [c.shape for c in old]
    err = float(np.max(np.abs(SC.dense(new) - SC.dense(old)))) / SC.scale(cid)
    assert err <= 1e-11, err
    SC.check_result(cid, old)


def _abi_call(T, cid, dev, mode=None, info=None):
    """`ttk_sum_round_one` itself: (status, out buffers, info, d, inner, bound); info: the caller's own buffer"""
    D = T.D
    plan = T._sum_round_one_plan(SC.terms(cid, dev), SC.coeffs(cid), SC.transposed(cid))
    (d, inner, rows, n, terms), sums, bound, mids, keep = plan
    outs, _ = T._packed_out(keep[0][0], bound, inner)
    info = D.empty(d + 2) if info is None else info
    P = ctypes.c_void_p * d
    D._stream()
    D.read(info)  # the allocations are done
    l0, s0 = D.lib.ttk_launch_count(), D.lib.ttk_sync_count()
    rc = D.lib.ttk_sum_round_one(D.ctx(), d, inner, rows, n, terms, SC.eps(cid),
                                 min(SC.mode(cid), 1) if mode is None else mode, P(*[o.data_ptr() for o in outs]),
                                 info.data_ptr())
    counts = (D.lib.ttk_launch_count() - l0, D.lib.ttk_sync_count() - s0)
    return rc, outs, info, d, inner, bound, counts, keep


@pytest.mark.parametrize("cid", ("o", "t", "s", "p", "m", "z"))
def test_abi_call_is_one_launch_and_no_wait(T, cid):
    """the call alone: one launch, nothing read; `info` then holds the reference's rounded ranks and, in mode 1,
    a tail whose 1/(2d)-th power is the reference's factor"""
    _, dev = _up(T, cid)
    rc, outs, info, d, inner, bound, counts, _ = _abi_call(T, cid, dev)
    assert rc == 0 and counts == (1, 0)
    got = T.D.read(info)
    assert [float(v) for v in got[:d + 1]] == [float(q) for q in SC.qranks(cid)]
    if SC.mode(cid) == 0:
        assert got[d + 1] == 0.0
    else:
        assert abs(got[d + 1] ** (1.0 / (2 * d)) - SC.factor(cid)) <= 1e-11 * SC.factor(cid)
    T.D.check_handoffs()


SENTINEL = 0x4242424242424242  # a finite double (about 1.6e11) that no case's figures come near


@pytest.mark.parametrize("mode", (0, 1))
def test_info_is_d_plus_2_words_and_the_word_after_them_is_not_written(T, mode):
    """`info` is d + 2 doubles: given d + 3 with the last preset, the call leaves that word's bits as they are and
    writes info[0 .. d+1] with the bits it writes into a d + 2 buffer (case t, d = 3: two terms, one transposed)"""
    _, dev = _up(T, "t")
    rc, _, info, d, _, _, _, _ = _abi_call(T, "t", dev, mode)
    assert rc == 0 and d == 3
    want = T.D.read(info)
    preset = np.full(d + 3, -1.0)
    preset[d + 2:].view(np.int64)[0] = SENTINEL
    rc, _, wide, _, _, _, _, _ = _abi_call(T, "t", dev, mode, T.D.from_numpy(preset))
    assert rc == 0
    got = T.D.read(wide)
    assert want.shape == (d + 2,) and got.shape == (d + 3,)
    assert int(got.view(np.int64)[d + 2]) == SENTINEL
    assert np.array_equal(got[:d + 2].view(np.int64), want.view(np.int64))
    assert not np.any(got[:d + 2] == -1.0)  # every word before it was written: ranks >= 1, a tail >= 0
    T.D.check_handoffs()


def _round_one_bits(T, tt, eps, mode):
    """`ttk_round_one` on the contiguous device train `tt`: (the written front of every out buffer, info)"""
    D = T.D
    d = len(tt)
    inner, ranks, bound = T._round_one_plan(tt)
    outs, _ = T._packed_out(tt, list(bound), inner)
    info = D.empty(d + 2)
    P = ctypes.c_void_p * d
    D._stream()
    rc = D.lib.ttk_round_one(D.ctx(), d, P(*[c.data_ptr() for c in tt]), inner, ranks, float(eps), mode,
                             P(*[o.data_ptr() for o in outs]), info.data_ptr())
    assert rc == 0
    return _fronts(T, outs, info, inner), list(bound)


def _fronts(T, outs, info, inner):
    got = T.D.read(info)
    q = [int(v) for v in got[:-1]]
    return [T.D.read(o[:q[k] * inner[k] * q[k + 1]]) for k, o in enumerate(outs)] + [got]


def _same_bits(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert x.shape == y.shape and np.array_equal(x.view(np.int64), y.view(np.int64))


def test_one_term_of_weight_one_is_round_one_bit_for_bit(T):
    _, dev = _up(T, "w")
    rc, outs, info, d, inner, bound, _, _ = _abi_call(T, "w", dev)
    assert rc == 0
    want, wbound = _round_one_bits(T, dev[0], SC.eps("w"), 0)
    assert bound == wbound
    _same_bits(_fronts(T, outs, info, inner), want)


@pytest.mark.parametrize("cid", ("c", "o", "n", "u", "t", "s", "p", "e"))
def test_sum_is_round_one_on_the_materialised_sum_bit_for_bit(T, cid):
    """the sum built with `tt_add` and `D.scaled` on core 0 (`_sum_composed`) holds the numbers the kernel's loads
    form, so `ttk_round_one` on it gives the same bits: out and info"""
    _, dev = _up(T, cid)
    mode = min(SC.mode(cid), 1)
    built = [T.D.contig(c) for c in T._sum_composed(SC.terms(cid, dev), SC.coeffs(cid), SC.transposed(cid))]
    want, wbound = _round_one_bits(T, built, SC.eps(cid), mode)
    rc, outs, info, d, inner, bound, _, _ = _abi_call(T, cid, dev)
    assert rc == 0 and bound == wbound
    _same_bits(_fronts(T, outs, info, inner), want)
    T.D.check_handoffs()


@pytest.mark.parametrize("cid", ("u", "s"))
def test_two_calls_same_bits(on, cid):
    import torch
    T = on
    _, dev = _up(T, cid)
    a = SC.public(T, cid, dev)
    b = SC.public(T, cid, dev)
    assert [x.shape for x in a] == [y.shape for y in b]
    assert all(torch.equal(x, y) for x, y in zip(a, b))


def test_launches_and_host_waits(T, monkeypatch):
    """contiguous device inputs: the switched-on public call launches at most twice (the rounding, and a copy
    kernel if the read needs one) and waits once; switched off it builds the sum first"""
    _, dev = _up(T, "s")
    monkeypatch.setattr(T, "SUM_ROUND_ONE", True)
    l0, s0 = T.D.lib.ttk_launch_count(), T.D.lib.ttk_sync_count()
    SC.public(T, "s", dev)
    assert T.D.lib.ttk_sync_count() - s0 == 1
    assert 1 <= T.D.lib.ttk_launch_count() - l0 <= 2
    monkeypatch.setattr(T, "SUM_ROUND_ONE", False)
    l0 = T.D.lib.ttk_launch_count()
    res = SC.public(T, "s", dev)
    assert T.D.lib.ttk_launch_count() - l0 > 2
    SC.check_result("s", T.to_host(res))


def test_large_sum_takes_the_composed_path(on):
    T = on
    dev = [T.to_device(t) for t in SC.stored("j")]
    assert T.sum_round_one_lds(SC.terms("j", dev), SC.transposed("j")) == -1
    T.D.read(dev[0][0])
    l0 = T.D.lib.ttk_launch_count()
    res = SC.public(T, "j", dev)
    assert T.D.lib.ttk_launch_count() - l0 > 2
    SC.check_result("j", T.to_host(res))


def test_validation_returns_an_error_without_launching(T):
    """every rejected argument: TTK_ERR_ARG from the host-side checks, the message names the function, no launch;
    the valid call on the same buffers still runs afterwards"""
    from ttipm_amd._lib import TTK_ERR_ARG, SumTerm
    D = T.D
    _, dev = _up(T, "t")   # two terms (1,2,3,r) / (1,3,2,r), the second transposed, d = 3
    a, b = dev
    d = 3
    P, I64, vp = ctypes.c_void_p * d, ctypes.c_int64, ctypes.c_void_p
    arr = lambda v: (I64 * len(v))(*v)  # noqa: E731
    ptr = lambda ts: P(*[t.data_ptr() if t is not None else None for t in ts])  # noqa: E731
    inner, rows = arr([6, 6, 6]), arr([2, 2, 2])
    ra, rb = arr(SC.term_ranks(a)), arr(SC.term_ranks(b))
    pa, pb = ptr(a), ptr(b)
    out = [D.empty(256) for _ in range(d)]
    po = ptr(out)
    info = D.empty(d + 2)
    eps = SC.eps("t")
    keep = []

    def terms(*spec):
        t = (SumTerm * max(len(spec), 1))()
        for j, (cores, ranks, coef, tr) in enumerate(spec):
            keep.extend((cores, ranks))
            t[j] = SumTerm(ctypes.cast(cores, vp) if cores is not None else None,
                           ctypes.cast(ranks, vp) if ranks is not None else None, coef, tr)
        return t

    good = terms((pa, ra, 1.0, 0), (pb, rb, 1.0, 1))
    D._stream()
    D.read(info)
    l0 = D.lib.ttk_launch_count()

    def bad(dd, inn, rws, n, tms, e, mode, outs, inf):
        assert D.lib.ttk_sum_round_one(D.ctx(), dd, inn, rws, n, tms, e, mode, outs, inf) == TTK_ERR_ARG
        assert b"ttk_sum_round_one" in D.lib.ttk_last_error()

    ok = (eps, 0, po, info.data_ptr())
    bad(1, inner, rows, 2, good, *ok)                                               # d = 1
    bad(d, arr([6, 0, 6]), rows, 2, good, *ok)                                      # a zero extent
    bad(d, None, rows, 2, good, *ok)
    for n in (0, 5, -1):
        bad(d, inner, rows, n, good, *ok)                                           # nterms outside 1 .. 4
    bad(d, inner, rows, 2, None, *ok)                                               # no term table
    bad(d, inner, None, 2, good, *ok)                                               # transposed without rows
    bad(d, inner, arr([2, 4, 2]), 2, good, *ok)                                     # rows[1] does not divide 6
    bad(d, inner, arr([2, 0, 2]), 2, good, *ok)
    for rk in ([1, 0, 2, 1], [2, 3, 2, 1], [1, 3, 2, 2]):                           # zero rank, boundary ranks
        bad(d, inner, rows, 2, terms((pa, arr(rk), 1.0, 0), (pb, rb, 1.0, 1)), *ok)
    bad(d, inner, rows, 2, terms((pa, ra, 1.0, 0), (pb, None, 1.0, 1)), *ok)        # no rank array
    bad(d, inner, rows, 2, terms((pa, ra, 1.0, 0), (None, rb, 1.0, 1)), *ok)        # no cores table
    bad(d, inner, rows, 2, terms((pa, ra, 1.0, 0), (ptr([b[0], None, b[2]]), rb, 1.0, 1)), *ok)  # a null core
    for c in (float("nan"), float("inf")):
        bad(d, inner, rows, 2, terms((pa, ra, c, 0), (pb, rb, 1.0, 1)), *ok)        # a non-finite weight
    for tr in (2, -1):
        bad(d, inner, rows, 2, terms((pa, ra, 1.0, 0), (pb, rb, 1.0, tr)), *ok)     # a flag that is no flag
    for e, mode in ((-1.0, 0), (float("nan"), 0), (float("inf"), 1), (eps, 2), (eps, -1)):
        bad(d, inner, rows, 2, good, e, mode, po, info.data_ptr())
    bad(d, inner, rows, 2, good, eps, 0, None, info.data_ptr())
    bad(d, inner, rows, 2, good, eps, 0, ptr([out[0], None, out[2]]), info.data_ptr())
    bad(d, inner, rows, 2, good, eps, 0, po, None)
    big = arr([1, 4096, 4096, 1])                                                   # does not fit LDS
    bad(d, arr([4096] * 3), None, 2, terms((pa, big, 1.0, 0), (pa, big, 1.0, 0)), *ok)
    assert D.lib.ttk_launch_count() == l0
    assert D.lib.ttk_sum_round_one(D.ctx(), d, inner, rows, 2, good, *ok) == 0
    assert D.lib.ttk_launch_count() == l0 + 1
    assert [int(v) for v in D.read(info)[:d + 1]] == SC.qranks("t")
    D.check_handoffs()


def _helper_runs(T, monkeypatch, f):
    """f under the switch off, then on: [(host result, MT19937 state)], and the switched-on run's (launches, waits)"""
    runs = []
    for switch in (False, True):
        monkeypatch.setattr(T, "SUM_ROUND_ONE", switch)
        np.random.seed(11)
        l0, s0 = T.D.lib.ttk_launch_count(), T.D.lib.ttk_sync_count()
        res = f()
        counts = (T.D.lib.ttk_launch_count() - l0, T.D.lib.ttk_sync_count() - s0)
        runs.append((T.to_host(res), np.random.get_state()))
    return runs, counts


@pytest.mark.parametrize("name", ("sym", "psd", "mask", "step", "step_psd", "step_mask", "add", "axpy"))
def test_ipm_helpers_switched_on_match_switched_off(T, monkeypatch, name):
    """the `tt_ipm` helpers: the same tensor to 1e-11 and the same ranks with the switch on as with it off, and the
    same MT19937 state afterwards (the `randint`s of the replaced `tt_scale` calls are still drawn)"""
    from ttipm_amd import tt_ipm
    host = SC.stored("m")
    X, DX = T.to_device(host[0]), T.to_device(host[1])
    mask = T.to_device(SC.mask("m"))
    T.D.read(mask[0])
    f = SC.helper_calls(tt_ipm)[name]
    runs, counts = _helper_runs(T, monkeypatch, lambda: f(list(X), list(DX), mask, 0.37, SC.eps("m")))
    (off, s0), (on_, s1) = runs
    assert [c.shape for c in off] == [c.shape for c in on_]
    a, b = SC.dense(off), SC.dense(on_)
    assert float(np.max(np.abs(a - b))) <= 1e-11 * float(np.max(np.abs(a)))
    assert np.array_equal(s0[1], s1[1]) and s0[2:] == s1[2:]
    assert counts[1] == 1  # the fused path ran: one read
    T.D.check_handoffs()
