"""Fixed-rank retraction on the MI355X: the one-launch `ttk_retract` (csrc/ttk_retract.hip) against the
reference's outputs (tests/golden/retract.npz), against the composed QR / SVD path, and its launch,
determinism, fallback, zero-input and validation contracts.  The native path is off by default
(TTIPM_NATIVE_RETRACT); the tests switch it on by monkeypatch.  The same value checks on the CPU
(composed path, emulated libttk): tests/test_host_retract.py."""
import ctypes

import numpy as np
import pytest

from tests import retract_cases as RC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def T():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from ttipm_amd import tt_ops
    assert hasattr(tt_ops.D.lib, "ttk_retract")
    return tt_ops


@pytest.fixture
def native(T, monkeypatch):
    monkeypatch.setattr(T, "NATIVE_RETRACT", True)
    return T


def _up(T, cid):
    tt = T.to_device(RC.train(cid))
    assert T.retract_lds(tt, RC.upper(cid)) >= 0  # takes the one-launch path
    T.D.read(tt[0])  # uploads done: the launch counts below see the retraction alone
    return tt


@pytest.mark.parametrize("cid", RC.FIT)
def test_native_matches_reference(native, cid):
    T = native
    host = RC.train(cid)
    tt = _up(T, cid)
    keep = list(tt)
    l0 = T.D.lib.ttk_launch_count()
    res = T.tt_rank_retraction(tt, RC.upper(cid))
    assert T.D.lib.ttk_launch_count() - l0 == 1  # the native path ran
    assert res is tt
    got = T.to_host(res)
    RC.check_result(cid, got)
    if cid in RC.ORTH:
        RC.check_left_orthonormal(got)
    for t, h in zip(keep, host):  # the caller's tensors are never written
        assert np.array_equal(T.D.read(t), h)
    T.D.check_handoffs()


@pytest.mark.parametrize("cid", RC.FIT)
def test_native_matches_composed(T, cid, monkeypatch):
    tt = _up(T, cid)
    monkeypatch.setattr(T, "NATIVE_RETRACT", True)
    nat = T.to_host(T.tt_rank_retraction(list(tt), RC.upper(cid)))
    monkeypatch.setattr(T, "NATIVE_RETRACT", False)
    com = T.to_host(T.tt_rank_retraction(list(tt), RC.upper(cid)))
    assert [c.shape for c in nat] == [c.shape for c in com]
    RC.close(RC.dense(nat), RC.dense(com), 1e-11)
    RC.check_result(cid, com)


def test_one_launch_and_no_host_wait(native):
    """inputs contiguous on the device: exactly one kernel launch, nothing read back"""
    T = native
    tt = _up(T, "e")
    T.D.read(tt[0])  # uploads done
    l0, s0 = T.D.lib.ttk_launch_count(), T.D.lib.ttk_sync_count()
    T.tt_rank_retraction(tt, RC.upper("e"))
    assert T.D.lib.ttk_launch_count() - l0 == 1
    assert T.D.lib.ttk_sync_count() - s0 == 0


def test_switch_off_is_the_composed_path(T, monkeypatch):
    """with the switch off (the default) the public call is the old sweep: many launches"""
    monkeypatch.setattr(T, "NATIVE_RETRACT", False)
    tt = _up(T, "b")
    T.D.read(tt[0])
    l0 = T.D.lib.ttk_launch_count()
    res = T.tt_rank_retraction(tt, RC.upper("b"))
    assert T.D.lib.ttk_launch_count() - l0 > 1
    RC.check_result("b", T.to_host(res))


def test_two_calls_same_bits(native):
    import torch
    T = native
    tt = _up(T, "h")
    a = T.tt_rank_retraction(list(tt), RC.upper("h"))
    b = T.tt_rank_retraction(list(tt), RC.upper("h"))
    assert all(torch.equal(x, y) for x, y in zip(a, b))


def test_large_train_takes_the_composed_path(native):
    T = native
    tt = T.to_device(RC.train("j"))
    assert T.retract_lds(tt, RC.upper("j")) == -1
    l0 = T.D.lib.ttk_launch_count()
    res = T.tt_rank_retraction(tt, RC.upper("j"))
    assert T.D.lib.ttk_launch_count() - l0 > 1
    RC.check_result("j", T.to_host(res))


def test_wrong_bound_count_takes_the_composed_path(native):
    """fewer bounds than bonds: the reference's loop stops early, which only the composed body does"""
    T = native
    tt = _up(T, "a")
    l0 = T.D.lib.ttk_launch_count()
    res = T.tt_rank_retraction(tt, RC.upper("a")[:2])
    assert T.D.lib.ttk_launch_count() - l0 > 1
    RC.close(RC.dense(T.to_host(res)), RC.dense(RC.train("a")), 1e-11)


def test_length_one_train_is_returned_unchanged(native):
    T = native
    tt = T.to_device(RC.train("i"))
    first = tt[0]
    res = T.tt_rank_retraction(tt, [])
    assert res is tt and res[0] is first


def test_all_zero_train_stays_finite(native):
    """every singular value is exactly 0: zero vectors, no division, finite cores of the rule's ranks
    that represent the zero tensor"""
    T = native
    d, r, up = 6, 5, [3] * 5
    rk = [1] + [r] * (d - 1) + [1]
    tt = T.to_device([np.zeros((rk[i], 4, rk[i + 1])) for i in range(d)])
    assert T.retract_lds(tt, up) >= 0
    T.D.read(tt[0])
    l0 = T.D.lib.ttk_launch_count()
    res = T.tt_rank_retraction(tt, up)
    assert T.D.lib.ttk_launch_count() - l0 == 1
    res = T.to_host(res)
    assert [1] + [c.shape[-1] for c in res] == T.retraction_ranks([4] * d, rk, up) == [1, 3, 3, 3, 3, 3, 1]
    assert all(np.all(np.isfinite(c)) for c in res)
    assert np.all(RC.dense(res) == 0.0)
    T.D.check_handoffs()


def test_validation_returns_an_error_without_launching(native):
    """d = 1, a zero rank, extent or bound, a boundary rank of 2 and a null pointer: TTK_ERR_ARG from the
    host-side checks, no launch; the valid call on the same buffers still runs afterwards"""
    from ttipm_amd._lib import TTK_ERR_ARG
    T = native
    D = T.D
    tt = _up(T, "f")
    out = [D.empty(64), D.empty(64)]
    P, I64 = ctypes.c_void_p, ctypes.c_int64
    ptr = lambda ts: (P * len(ts))(*[t.data_ptr() if t is not None else None for t in ts])  # noqa: E731
    arr = lambda v: (I64 * len(v))(*v)  # noqa: E731
    D._stream()
    D.read(tt[0])
    l0 = D.lib.ttk_launch_count()
    got = (I64 * 3)()
    for d, inner, ranks, upper in ((1, (4, 4), (1, 1, 1), (3,)), (2, (4, 4), (1, 0, 1), (3,)), (2, (4, 0), (1, 5, 1), (3,)),
                                   (2, (4, 4), (1, 5, 1), (0,)), (2, (4, 4), (2, 5, 1), (3,)), (2, (4, 4), (1, 5, 2), (3,)),
                                   (2, (4096, 4096), (1, 4096, 1), (3,))):
        rc = D.lib.ttk_retract(D.ctx(), d, ptr(tt), arr(inner), arr(ranks), arr(upper), ptr(out), got)
        assert rc == TTK_ERR_ARG
        assert b"ttk_retract" in D.lib.ttk_last_error()
        assert D.lib.ttk_retract_lds(d, arr(inner), arr(ranks), arr(upper)) == -1
    good = (arr((4, 4)), arr((1, 5, 1)), arr((3,)))
    for cores, outs in (([tt[0], None], out), (tt, [out[0], None])):
        rc = D.lib.ttk_retract(D.ctx(), 2, ptr(cores), *good, ptr(outs), got)
        assert rc == TTK_ERR_ARG
        assert b"ttk_retract" in D.lib.ttk_last_error()
    for args in ((None, good[0], good[1], good[2], ptr(out), got), (ptr(tt), None, good[1], good[2], ptr(out), got),
                 (ptr(tt), good[0], None, good[2], ptr(out), got), (ptr(tt), good[0], good[1], None, ptr(out), got),
                 (ptr(tt), good[0], good[1], good[2], None, got), (ptr(tt), good[0], good[1], good[2], ptr(out), None)):
        assert D.lib.ttk_retract(D.ctx(), 2, *args) == TTK_ERR_ARG
    assert D.lib.ttk_launch_count() == l0
    rc = D.lib.ttk_retract(D.ctx(), 2, ptr(tt), *good, ptr(out), got)
    assert rc == 0 and list(got) == [1, 3, 1]
    RC.check_result("f", T.to_host(T.tt_rank_retraction(tt, RC.upper("f"))))
    D.check_handoffs()
