"""Generalised Nystroem rounding on the MI355X: the three-launch `ttk_nystroem` (csrc/ttk_nystroem.hip)
against the reference's outputs (tests/golden/nystroem.npz), against the composed einsum / SVD path,
and its launch, determinism, fallback and validation contracts.  The same value checks on the CPU
(composed path, emulated libttk): tests/test_host_nystroem.py."""
import ctypes

import numpy as np
import pytest

from tests import nystroem_cases as NC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def T():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from ttipm_amd import tt_ops
    assert tt_ops.NATIVE_NYSTROEM and hasattr(tt_ops.D.lib, "ttk_nystroem")
    return tt_ops


def _up(T, tt):
    return T.to_device(tt)


def _native(T, cid):
    g1, g2 = NC.sketches(cid)
    tt, g1, g2 = _up(T, NC.train(cid)), _up(T, g1), _up(T, g2)
    assert T.nystroem_lds(tt, g1, g2) >= 0  # takes the three-launch path
    return tt, g1, g2


@pytest.mark.parametrize("cid", NC.FIT)
def test_native_matches_reference(T, cid):
    host = NC.train(cid)
    tt, g1, g2 = _native(T, cid)
    keep = list(tt)
    res = T._tt_generalised_nystroem(tt, g1, g2)
    assert res is tt
    NC.check_result(cid, T.to_host(res))
    for t, h in zip(keep, host):  # the caller's tensors are never written
        assert np.array_equal(T.D.read(t), h)
    for ts, hs in zip((g1, g2), NC.sketches(cid)):
        for t, h in zip(ts, hs):
            assert np.array_equal(T.D.read(t), h)
    T.D.check_handoffs()


@pytest.mark.parametrize("cid", NC.FIT)
def test_native_matches_composed(T, cid, monkeypatch):
    tt, g1, g2 = _native(T, cid)
    nat = T.to_host(T._tt_generalised_nystroem(list(tt), g1, g2))
    monkeypatch.setattr(T, "NATIVE_NYSTROEM", False)
    com = T.to_host(T._tt_generalised_nystroem(list(tt), g1, g2))
    assert [c.shape for c in nat] == [c.shape for c in com]
    NC.close(NC.dense(nat), NC.dense(com), 1e-11)
    NC.check_result(cid, com)


@pytest.mark.parametrize("cid", NC.FIT)
def test_contractions_on_device(T, cid):
    tt, g1, g2 = _native(T, cid)
    for which, W in (("WL", T.tt_lr_contraction(tt, g1)), ("WR", T.tt_rl_contraction(tt, g2))):
        for w, v in zip(W, NC.contractions(cid, which)):
            NC.close(T.D.read(w), v, 1e-12)


@pytest.mark.parametrize("cid", NC.PUBLIC)
def test_public_call_matches_reference_and_rng_stream(T, cid):
    tt = _up(T, NC.train(cid))
    np.random.seed(int(NC.G[f"{cid}/pub_seed"]))
    res = T.tt_generalised_nystroem(tt, NC.targets(cid))
    NC.check_rng_state(cid)
    NC.check_result(cid, T.to_host(res), "pub_")


def test_right_sketch_below_the_left(T, monkeypatch):
    """rranks < lranks: the Jacobi rotates the rows of P^T.  Both sketches are at or above the tensor's
    own rank (case a: 3, so P keeps full rank): the input is reproduced, and the composed path agrees"""
    host = NC.train("a")
    rs = np.random.RandomState(5)
    g1 = _up(T, [rs.randn(a, 4, b) for a, b in zip([1, 5, 5, 5, 5], [5, 5, 5, 5, 1])])
    g2 = _up(T, [rs.randn(a, 4, b) for a, b in zip([1, 3, 3, 3, 3], [3, 3, 3, 3, 1])])
    tt = _up(T, host)
    assert T.nystroem_lds(tt, g1, g2) >= 0
    nat = T.to_host(T._tt_generalised_nystroem(list(tt), g1, g2))
    assert [c.shape[0] for c in nat[1:]] == [3, 3, 3, 3]
    NC.close(NC.dense(nat), NC.dense(host), 1e-11)
    monkeypatch.setattr(T, "NATIVE_NYSTROEM", False)
    com = T.to_host(T._tt_generalised_nystroem(list(tt), g1, g2))
    NC.close(NC.dense(nat), NC.dense(com), 1e-11)


def test_left_sketch_above_the_right_matches_composed(T, monkeypatch):
    """`NC.transposed_case()`: lranks > rranks at every bond, a true truncation (well posed:
    tests/test_host_nystroem.py); three launches, the rule's ranks, the composed path's tensor"""
    tt, g1, g2 = (_up(T, t) for t in NC.transposed_case())
    assert T.nystroem_lds(tt, g1, g2) >= 0
    T.D.read(tt[0])  # uploads done
    l0 = T.D.lib.ttk_launch_count()
    nat = T._tt_generalised_nystroem(list(tt), g1, g2)
    assert T.D.lib.ttk_launch_count() - l0 == 3
    nat = T.to_host(nat)
    assert [1] + [c.shape[-1] for c in nat] == [1, 3, 3, 1]
    monkeypatch.setattr(T, "NATIVE_NYSTROEM", False)
    com = T.to_host(T._tt_generalised_nystroem(list(tt), g1, g2))
    assert [c.shape for c in nat] == [c.shape for c in com]
    NC.close(NC.dense(nat), NC.dense(com), 1e-11)
    T.D.check_handoffs()


def test_three_launches_and_no_host_wait(T):
    """inputs contiguous on the device: at most three kernel launches, nothing read back"""
    tt, g1, g2 = _native(T, "g")
    T.D.read(tt[0])  # uploads done
    l0, s0 = T.D.lib.ttk_launch_count(), T.D.lib.ttk_sync_count()
    T._tt_generalised_nystroem(tt, g1, g2)
    assert 1 <= T.D.lib.ttk_launch_count() - l0 <= 3
    assert T.D.lib.ttk_sync_count() - s0 == 0


def test_two_calls_same_bits(T):
    import torch
    tt, g1, g2 = _native(T, "d")
    a = T._tt_generalised_nystroem(list(tt), g1, g2)
    b = T._tt_generalised_nystroem(list(tt), g1, g2)
    assert all(torch.equal(x, y) for x, y in zip(a, b))


def test_large_train_takes_the_composed_path(T):
    g1, g2 = NC.sketches("j")
    tt, g1, g2 = _up(T, NC.train("j")), _up(T, g1), _up(T, g2)
    assert T.nystroem_lds(tt, g1, g2) == -1
    NC.check_result("j", T.to_host(T._tt_generalised_nystroem(tt, g1, g2)))


def test_singular_case_returns_with_the_right_shapes(T):
    """case z: the first bond has exact rank 2 < 4, so P is singular there and the reference's own
    output is rounding noise; the call returns, ranks and shapes are right, no hand-off gave up"""
    tt, g1, g2 = _native(T, "z")
    res = T._tt_generalised_nystroem(tt, g1, g2)
    NC.check_shapes("z", T.to_host(res))
    T.D.check_handoffs()


def test_validation_returns_an_error_without_launching(T):
    """a rank of 0, d = 1, unequal boundary ranks and a null core: TTK_ERR_ARG from the host-side
    checks, no launch"""
    from ttipm_amd._lib import TTK_ERR_ARG
    D = T.D
    tt, g1, g2 = _native(T, "f")
    out = [D.empty(64), D.empty(64)]
    P, I64 = ctypes.c_void_p, ctypes.c_int64
    ptr = lambda ts: (P * len(ts))(*[t.data_ptr() if t is not None else None for t in ts])  # noqa: E731
    arr = lambda v: (I64 * len(v))(*v)  # noqa: E731
    D._stream()
    D.read(tt[0])
    l0 = D.lib.ttk_launch_count()
    got = (I64 * 3)()
    good = ((1, 5, 1), (1, 3, 1), (1, 4, 1))
    for d, ranks, lranks, rranks in ((2, (1, 0, 1), good[1], good[2]), (2, good[0], (1, 0, 1), good[2]),
                                     (2, good[0], good[1], (1, 0, 1)), (1, (1, 1), (1, 1), (1, 1)),
                                     (2, (1, 5, 2), good[1], good[2]), (2, good[0], (2, 3, 1), good[2]),
                                     (2, good[0], good[1], (1, 4, 2))):
        rc = D.lib.ttk_nystroem(D.ctx(), d, ptr(tt), arr((4, 4)), arr(ranks), ptr(g1), arr(lranks), ptr(g2),
                                arr(rranks), ptr(out), got)
        assert rc == TTK_ERR_ARG
        assert b"ttk_nystroem" in D.lib.ttk_last_error()
        assert D.lib.ttk_nystroem_lds(d, arr((4, 4)), arr(ranks), arr(lranks), arr(rranks)) == -1
    for cores, s1, s2, outs in (([tt[0], None], g1, g2, out), (tt, [None, g1[1]], g2, out), (tt, g1, [g2[0], None], out),
                                (tt, g1, g2, [out[0], None])):
        rc = D.lib.ttk_nystroem(D.ctx(), 2, ptr(cores), arr((4, 4)), arr(good[0]), ptr(s1), arr(good[1]), ptr(s2),
                                arr(good[2]), ptr(outs), got)
        assert rc == TTK_ERR_ARG
        assert b"ttk_nystroem" in D.lib.ttk_last_error()
    assert D.lib.ttk_launch_count() == l0
    # the sketch cores the chains never read may be null
    rc = D.lib.ttk_nystroem(D.ctx(), 2, ptr(tt), arr((4, 4)), arr(good[0]), ptr([g1[0], None]), arr(good[1]),
                            ptr([None, g2[1]]), arr(good[2]), ptr(out), got)
    assert rc == 0 and list(got) == [1, 3, 1]
    # and the valid call on the same buffers still runs afterwards
    NC.check_result("f", T.to_host(T._tt_generalised_nystroem(tt, g1, g2)))
    D.check_handoffs()
