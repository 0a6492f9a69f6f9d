"""Eps-truncating rounding on the MI355X: the one-launch `ttk_round_one` (csrc/ttk_retract.hip, ranks decided
in the kernel) against the reference's outputs (tests/golden/round_one.npz), against the current path
(`ttk_round`), and its launch, host-wait, determinism, fallback, zero-input and validation contracts.
The path is off by default (TTIPM_ROUND_ONE); the tests switch it on by monkeypatch.  The same value
checks on the CPU (today's path, emulated libttk): tests/test_host_round_one.py."""
import ctypes

import numpy as np
import pytest

from tests import round_one_cases as RC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def T():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from ttipm_amd import tt_ops
    assert hasattr(tt_ops.D.lib, "ttk_round_one")
    return tt_ops


@pytest.fixture
def one(T, monkeypatch):
    monkeypatch.setattr(T, "ROUND_ONE", True)
    return T


def _up(T, cid):
    tt = T.to_device(RC.train(cid))
    assert T.round_one_lds(tt) >= 0  # takes the one-launch path
    T.D.read(tt[0])  # uploads done: the launch counts below see the rounding alone
    return tt


@pytest.mark.parametrize("cid", RC.FIT)
def test_one_launch_matches_reference(one, cid):
    """the public call of the case (tt_rank_reduce, or the PSD / mask variant through _tail_rank_reduce)"""
    T = one
    host = RC.train(cid)
    tt = _up(T, cid)
    keep = list(tt)
    s0 = T.D.lib.ttk_sync_count()
    res = RC.public(T, cid, tt)
    assert T.D.lib.ttk_sync_count() - s0 == 1  # the one-launch path ran: one read, of the ranks
    got = T.to_host(res)
    RC.check_result(cid, got)
    if cid in RC.ORTH:
        assert res is tt
        RC.check_left_orthonormal(got)
    for t, h in zip(keep, host):  # the caller's tensors are never written
        assert np.array_equal(T.D.read(t), h)
    T.D.check_handoffs()


@pytest.mark.parametrize("cid", RC.FIT)
def test_one_launch_matches_current_path(T, cid, monkeypatch):
    tt = _up(T, cid)
    monkeypatch.setattr(T, "ROUND_ONE", True)
    new = T.to_host(RC.public(T, cid, list(tt)))
    monkeypatch.setattr(T, "ROUND_ONE", False)
    old = T.to_host(RC.public(T, cid, list(tt)))
    assert [c.shape for c in new] == [c.shape for c in old]
    RC.close(RC.dense(new), RC.dense(old), 1e-11)
    RC.check_result(cid, old)


def test_launches_and_host_waits(T, monkeypatch):
    """contiguous device inputs: the switched-on public call waits for the device once and launches at most
    twice (the rounding, and a copy kernel if the read needs one); switched off it is today's sweep"""
    tt = _up(T, "b")
    d = len(tt)
    monkeypatch.setattr(T, "ROUND_ONE", True)
    l0, s0 = T.D.lib.ttk_launch_count(), T.D.lib.ttk_sync_count()
    T.tt_rank_reduce(list(tt), RC.eps("b"))
    assert T.D.lib.ttk_sync_count() - s0 == 1
    assert 1 <= T.D.lib.ttk_launch_count() - l0 <= 2
    monkeypatch.setattr(T, "ROUND_ONE", False)
    l0, s0 = T.D.lib.ttk_launch_count(), T.D.lib.ttk_sync_count()
    res = T.tt_rank_reduce(list(tt), RC.eps("b"))
    assert T.D.lib.ttk_launch_count() - l0 > 2
    assert T.D.lib.ttk_sync_count() - s0 == d - 1
    RC.check_result("b", T.to_host(res))


def _abi_call(T, tt, eps, mode):
    """`ttk_round_one` itself on the device train `tt`: (status, out buffers, info, inner, bound)"""
    D = T.D
    d = len(tt)
    inner, ranks, bound = T._round_one_plan(tt)
    outs, _ = T._packed_out(tt, list(bound), inner)
    info = D.empty(d + 2)
    P = ctypes.c_void_p * d
    D._stream()
    rc = D.lib.ttk_round_one(D.ctx(), d, P(*[c.data_ptr() for c in tt]), inner, ranks, float(eps), mode,
                             P(*[o.data_ptr() for o in outs]), info.data_ptr())
    return rc, outs, info, inner, bound


@pytest.mark.parametrize("cid", ("b", "t", "p", "q", "n"))
def test_abi_call_is_one_launch_and_no_wait(T, cid):
    """the call alone: one launch, nothing read; `info` then holds the reference's rounded ranks and, in
    mode 1, a tail whose 1/(2d)-th power is the reference's factor"""
    D = T.D
    tt = _up(T, cid)
    d = len(tt)
    l0, s0 = D.lib.ttk_launch_count(), D.lib.ttk_sync_count()
    rc, outs, info, inner, bound = _abi_call(T, tt, RC.eps(cid), min(RC.mode(cid), 1))
    assert rc == 0
    assert D.lib.ttk_launch_count() - l0 == 1
    assert D.lib.ttk_sync_count() - s0 == 0
    got = D.read(info)
    assert [float(v) for v in got[:d + 1]] == [float(q) for q in RC.qranks(cid)]
    if RC.mode(cid) == 0:
        assert got[d + 1] == 0.0
    elif RC.factor(cid) == 0.0:
        assert got[d + 1] == 0.0
    else:
        assert abs(got[d + 1] ** (1.0 / (2 * d)) - RC.factor(cid)) <= 1e-11 * RC.factor(cid)
    D.check_handoffs()


@pytest.mark.parametrize("cid", ("h", "t"))
def test_two_calls_same_bits(one, cid):
    import torch
    T = one
    tt = _up(T, cid)
    a = T.tt_rank_reduce(list(tt), RC.eps(cid))
    b = T.tt_rank_reduce(list(tt), RC.eps(cid))
    assert [x.shape for x in a] == [y.shape for y in b]
    assert all(torch.equal(x, y) for x, y in zip(a, b))


def test_all_zero_train_goes_to_rank_one(one):
    """every singular value is exactly 0: the rule gives rank 1 at every bond without a special case, nothing
    divides by a singular value, and the finite cores represent the zero tensor"""
    T = one
    d, r = 6, 5
    rk = [1] + [r] * (d - 1) + [1]
    tt = T.to_device([np.zeros((rk[i], 4, rk[i + 1])) for i in range(d)])
    assert T.round_one_lds(tt) >= 0
    T.D.read(tt[0])
    s0 = T.D.lib.ttk_sync_count()
    res = T.tt_rank_reduce(tt, 1e-6)
    assert T.D.lib.ttk_sync_count() - s0 == 1
    res = T.to_host(res)
    assert [1] + [c.shape[-1] for c in res] == [1] * (d + 1)
    assert all(np.all(np.isfinite(c)) for c in res)
    assert np.all(RC.dense(res) == 0.0)
    T.D.check_handoffs()


def test_large_train_takes_the_current_path(one):
    T = one
    tt = T.to_device(RC.train("j"))
    assert T.round_one_lds(tt) == -1
    T.D.read(tt[0])
    l0 = T.D.lib.ttk_launch_count()
    res = T.tt_rank_reduce(tt, RC.eps("j"))
    assert T.D.lib.ttk_launch_count() - l0 > 2
    RC.check_result("j", T.to_host(res))


@pytest.mark.parametrize("cid", RC.UNCHANGED)
def test_trivial_trains_are_returned_unchanged(one, cid):
    T = one
    tt = T.to_device(RC.train(cid))
    cores = list(tt)
    T.D.read(tt[0])
    l0 = T.D.lib.ttk_launch_count()
    for f in (T.tt_rank_reduce, T.tt_psd_rank_reduce):
        res = f(tt, RC.eps(cid))
        assert res is tt and all(a is b for a, b in zip(res, cores))
    assert T.D.lib.ttk_launch_count() == l0


def test_validation_returns_an_error_without_launching(one):
    """d = 1, a zero rank or extent, a boundary rank of 2, a train that does not fit, a bad eps or mode and a
    null pointer: TTK_ERR_ARG from the host-side checks, no launch; the valid call on the same buffers still
    runs afterwards"""
    from ttipm_amd._lib import TTK_ERR_ARG
    T = one
    D = T.D
    tt = _up(T, "f")
    out = [D.empty(64), D.empty(64)]
    info = D.empty(4)
    P, I64 = ctypes.c_void_p, ctypes.c_int64
    ptr = lambda ts: (P * len(ts))(*[t.data_ptr() if t is not None else None for t in ts])  # noqa: E731
    arr = lambda v: (I64 * len(v))(*v)  # noqa: E731
    D._stream()
    D.read(tt[0])
    l0 = D.lib.ttk_launch_count()
    eps = RC.eps("f")

    def call(d, cores, inner, ranks, e, mode, outs, inf):
        rc = D.lib.ttk_round_one(D.ctx(), d, cores, inner, ranks, e, mode, outs, inf)
        assert rc == TTK_ERR_ARG
        assert b"ttk_round_one" in D.lib.ttk_last_error()

    for d, inner, ranks in ((1, (4, 4), (1, 1, 1)), (2, (4, 4), (1, 0, 1)), (2, (4, 0), (1, 5, 1)),
                            (2, (4, 4), (2, 5, 1)), (2, (4, 4), (1, 5, 2)), (2, (4096, 4096), (1, 4096, 1))):
        call(d, ptr(tt), arr(inner), arr(ranks), eps, 0, ptr(out), info.data_ptr())
        assert D.lib.ttk_round_one_lds(d, arr(inner), arr(ranks), None) == -1
    good = (arr((4, 4)), arr((1, 5, 1)))
    for e, mode in ((-1.0, 0), (float("nan"), 0), (float("inf"), 1), (eps, 2), (eps, -1)):
        call(2, ptr(tt), *good, e, mode, ptr(out), info.data_ptr())
    for cores, outs in (([tt[0], None], out), (tt, [out[0], None])):
        call(2, ptr(cores), *good, eps, 0, ptr(outs), info.data_ptr())
    for args in ((None, good[0], good[1], eps, 0, ptr(out), info.data_ptr()),
                 (ptr(tt), None, good[1], eps, 0, ptr(out), info.data_ptr()),
                 (ptr(tt), good[0], None, eps, 0, ptr(out), info.data_ptr()),
                 (ptr(tt), good[0], good[1], eps, 0, None, info.data_ptr()),
                 (ptr(tt), good[0], good[1], eps, 0, ptr(out), None)):
        assert D.lib.ttk_round_one(D.ctx(), 2, *args) == TTK_ERR_ARG
    assert D.lib.ttk_launch_count() == l0
    rc = D.lib.ttk_round_one(D.ctx(), 2, ptr(tt), *good, eps, 0, ptr(out), info.data_ptr())
    assert rc == 0 and [int(v) for v in D.read(info)[:3]] == RC.qranks("f")
    RC.check_result("f", T.to_host(T.tt_rank_reduce(tt, eps)))
    D.check_handoffs()
