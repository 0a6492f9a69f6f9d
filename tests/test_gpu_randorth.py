"""Randomised fixed-rank rounding on the MI355X: the one-launch sweep `ttk_rand_orth`
(csrc/ttk_randorth.hip) against the reference's outputs (tests/golden/randorth.npz), against the
composed einsum / QR path, and its launch, determinism, fallback and validation contracts.  The
same value checks on the CPU (composed path, emulated libttk): tests/test_host_randorth.py."""
import ctypes

import numpy as np
import pytest

from tests import randorth_cases as RC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def T():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from ttipm_amd import tt_ops
    assert tt_ops.NATIVE_RANDORTH and hasattr(tt_ops.D.lib, "ttk_rand_orth")
    return tt_ops


def _up(T, tt):
    return T.to_device(tt)


def _native(T, cid):
    tt, gs = _up(T, RC.train(cid)), _up(T, RC.sketch(cid))
    assert T.randorth_lds(tt, gs) >= 0  # takes the one-launch path
    return tt, gs


@pytest.mark.parametrize("cid", RC.FIT)
def test_native_lr_sweep_matches_reference(T, cid):
    host = RC.train(cid)
    tt, gs = _native(T, cid)
    keep = list(tt)
    res = T._tt_lr_random_orthogonalise(tt, gs)
    assert res is tt
    RC.check_result(cid, T.to_host(res))
    for t, h in zip(keep, host):  # the caller's tensors are never written
        assert np.array_equal(T.D.read(t), h)
    T.D.check_handoffs()


@pytest.mark.parametrize("cid", RC.RL)
def test_native_rl_sweep_matches_reference(T, cid):
    tt, gs = _native(T, cid)
    RC.check_result(cid, T.to_host(T._tt_rl_random_orthogonalise(tt, gs)), "rl")


@pytest.mark.parametrize("cid", RC.FIT)
def test_native_matches_composed(T, cid, monkeypatch):
    tt, gs = _native(T, cid)
    nat = T.to_host(T._tt_lr_random_orthogonalise(list(tt), gs))
    monkeypatch.setattr(T, "NATIVE_RANDORTH", False)
    com = T.to_host(T._tt_lr_random_orthogonalise(list(tt), gs))
    assert [c.shape for c in nat] == [c.shape for c in com]
    RC.close(RC.dense(nat), RC.dense(com), 1e-11)
    assert RC.orth_error(com) <= 1e-12


@pytest.mark.parametrize("cid", RC.FIT)
def test_rl_contraction_on_device(T, cid):
    W = T.tt_rl_contraction(_up(T, RC.train(cid)), _up(T, RC.sketch(cid)))
    for k, w in enumerate(W):
        RC.close(T.D.read(w), RC.G[f"{cid}/W/{k}"], 1e-12)


@pytest.mark.parametrize("cid", RC.PUBLIC)
def test_public_call_matches_reference_and_rng_stream(T, cid):
    tt = _up(T, RC.train(cid))
    np.random.seed(int(RC.G[f"{cid}/pub_seed"]))
    res = T.tt_lr_random_orthogonalise(tt, RC.targets(cid))
    RC.check_rng_state(cid)
    RC.check_result(cid, T.to_host(res), "pub")


def test_one_launch(T):
    """inputs contiguous on the device: the whole sweep is one kernel launch"""
    tt, gs = _native(T, "g")
    T.D.read(tt[0])  # uploads done
    l0 = T.D.lib.ttk_launch_count()
    T._tt_lr_random_orthogonalise(tt, gs)
    assert T.D.lib.ttk_launch_count() - l0 == 1


def test_1024_threads_match_composed(T, monkeypatch):
    """`RC.wide_case()`: a product of more than 2048 entries, so the launch has 1024 threads (every
    fixture case runs 256); one launch, the rule's ranks, the composed path's tensor, orthonormal Q"""
    tt, gs = (_up(T, t) for t in RC.wide_case())
    assert T.randorth_lds(tt, gs) >= 0
    T.D.read(tt[0])  # uploads done
    l0 = T.D.lib.ttk_launch_count()
    nat = T._tt_lr_random_orthogonalise(list(tt), gs)
    assert T.D.lib.ttk_launch_count() - l0 == 1
    nat = T.to_host(nat)
    assert [1] + [c.shape[-1] for c in nat] == [1, 12, 12, 12, 1]
    monkeypatch.setattr(T, "NATIVE_RANDORTH", False)
    com = T.to_host(T._tt_lr_random_orthogonalise(list(tt), gs))
    assert [c.shape for c in nat] == [c.shape for c in com]
    RC.close(RC.dense(nat), RC.dense(com), 1e-11)
    assert RC.orth_error(nat) <= 1e-12
    T.D.check_handoffs()


def test_two_calls_same_bits(T):
    import torch
    tt, gs = _native(T, "d")
    a = T._tt_lr_random_orthogonalise(list(tt), gs)
    b = T._tt_lr_random_orthogonalise(list(tt), gs)
    assert all(torch.equal(x, y) for x, y in zip(a, b))


def test_large_train_takes_the_composed_path(T):
    tt, gs = _up(T, RC.train("j")), _up(T, RC.sketch("j"))
    assert T.randorth_lds(tt, gs) == -1
    RC.check_result("j", T.to_host(T._tt_lr_random_orthogonalise(tt, gs)))


def test_validation_returns_an_error_without_launching(T):
    """a rank of 0, d < 2 and unequal trailing ranks: TTK_ERR_ARG from the host-side checks, no launch"""
    from ttipm_amd._lib import TTK_ERR_ARG
    D = T.D
    tt, gs = _native(T, "f")
    out = [D.empty(64), D.empty(64)]
    P, I64 = ctypes.c_void_p, ctypes.c_int64
    ptr = lambda ts: (P * len(ts))(*[t.data_ptr() for t in ts])  # noqa: E731
    D._stream()
    D.read(tt[0])
    l0 = D.lib.ttk_launch_count()
    got = (I64 * 3)()
    for d, ranks, sranks in ((2, (1, 0, 1), (1, 3, 1)), (2, (1, 5, 1), (1, 0, 1)), (1, (1, 1), (1, 1)),
                             (2, (1, 5, 2), (1, 3, 1))):
        rc = D.lib.ttk_rand_orth(D.ctx(), d, ptr(tt), (I64 * 2)(4, 4), (I64 * len(ranks))(*ranks), ptr(gs),
                                 (I64 * len(sranks))(*sranks), ptr(out), got)
        assert rc == TTK_ERR_ARG
        assert D.lib.ttk_rand_orth_lds(d, (I64 * 2)(4, 4), (I64 * len(ranks))(*ranks),
                                       (I64 * len(sranks))(*sranks)) == -1
    assert D.lib.ttk_launch_count() == l0
    assert b"ttk_rand_orth" in D.lib.ttk_last_error()
    # and the valid call on the same buffers still runs afterwards
    RC.check_result("f", T.to_host(T._tt_lr_random_orthogonalise(tt, gs)))
    D.check_handoffs()
