"""Randomised fixed-rank rounding (`tt_rl_contraction`, `_tt_lr/_rl_random_orthogonalise`,
`tt_lr/_rl_random_orthogonalise`; reference `src/tt_ops.py:51-101`): the composed path's host logic
on the CPU, libttk replaced by the NumPy emulator, against the reference's own outputs
(tests/golden/randorth.npz).  The device run of the same checks is tests/test_gpu_randorth.py."""
import numpy as np
import pytest

from tests import randorth_cases as RC
from tests.emu_ttk import emulated_ttipm


@pytest.fixture(scope="module")
def T():
    emulated_ttipm()
    from ttipm_amd import tt_ops
    return tt_ops


def _up(T, tt):
    return T.to_device(tt)


@pytest.mark.parametrize("cid", RC.SWEEP)
def test_lr_sweep_matches_reference(T, cid):
    host = RC.train(cid)
    tt = _up(T, host)
    keep = list(tt)
    res = T._tt_lr_random_orthogonalise(tt, _up(T, RC.sketch(cid)))
    assert res is tt  # rebound in place, like the reference's list mutation
    RC.check_result(cid, T.to_host(res))
    for t, h in zip(keep, host):  # the caller's tensors are never written
        assert np.array_equal(T.D.read(t), h)


@pytest.mark.parametrize("cid", RC.RL)
def test_rl_sweep_matches_reference(T, cid):
    host = RC.train(cid)
    tt = _up(T, host)
    keep = list(tt)
    res = T._tt_rl_random_orthogonalise(tt, _up(T, RC.sketch(cid)))
    RC.check_result(cid, T.to_host(res), "rl")
    for t, h in zip(keep, host):
        assert np.array_equal(T.D.read(t), h)


@pytest.mark.parametrize("cid", RC.FIT)
def test_rl_contraction_matches_reference(T, cid):
    W = T.tt_rl_contraction(_up(T, RC.train(cid)), _up(T, RC.sketch(cid)))
    assert len(W) == len(RC.targets(cid))
    for k, w in enumerate(W):
        RC.close(T.D.read(w), RC.G[f"{cid}/W/{k}"], 1e-12)


def test_lr_contraction_is_the_mirrored_rl(T):
    a, b = RC.train("h"), RC.sketch("h")
    W = T.tt_lr_contraction(_up(T, a), _up(T, b))
    # by hand: the left-to-right partial contractions V_k (ra_k, rb_k) for the bonds k = 1 .. d-1
    v = np.ones((1, 1))
    want = []
    for ca, cb in zip(a[:-1], b[:-1]):
        v = np.einsum("ab,aiA,biB->AB", v, ca, cb)
        want.append(v)
    for w, v in zip(W, want):
        RC.close(T.D.read(w), v.T, 1e-12)


def test_rank_rule(T):
    randorth_ranks = T.randorth_ranks
    assert randorth_ranks(1, [4, 4, 4, 4], [5, 5, 5, 5]) == [1, 4, 5, 5, 5]      # case a: ranks grow
    assert randorth_ranks(1, [4, 4], [9, 9]) == [1, 4, 9]                        # case e: m < n first
    assert randorth_ranks(1, [4, 4, 4, 4], [3, 2, 6, 4]) == [1, 3, 2, 6, 4]      # case h
    assert randorth_ranks(2, [2], [7]) == [2, 4]


@pytest.mark.parametrize("cid", RC.PUBLIC)
def test_public_call_matches_reference_and_rng_stream(T, cid):
    tt = _up(T, RC.train(cid))
    np.random.seed(int(RC.G[f"{cid}/pub_seed"]))
    res = T.tt_lr_random_orthogonalise(tt, RC.targets(cid))
    RC.check_rng_state(cid)
    RC.check_result(cid, T.to_host(res), "pub")


def test_public_rl_call(T):
    """the rl public call draws the same sketch (then mirrors it): same stream state afterwards,
    right unfoldings orthonormal, ranks fixed by the targets from the right"""
    host = RC.train("c")
    np.random.seed(int(RC.G["c/pub_seed"]))
    res = T.to_host(T.tt_rl_random_orthogonalise(_up(T, host), RC.targets("c")))
    RC.check_rng_state("c")
    assert [c.shape[0] for c in res[1:]] == RC.targets("c")
    assert RC.orth_error(res, left=False) <= 1e-12


def test_length_one_train_is_returned_unchanged(T):
    host = RC.train("i")
    tt = _up(T, host)
    first = tt[0]
    st = np.random.get_state()
    for f in (T.tt_lr_random_orthogonalise, T.tt_rl_random_orthogonalise):
        res = f(tt, [])
        assert res is tt and res[0] is first
    assert np.array_equal(np.random.get_state()[1], st[1])  # nothing drawn
    RC.close(RC.dense(T.to_host(tt)), RC.G["i/lr_dense"], 0.0)


def test_target_above_rank_reproduces_the_input(T):
    """cases a and e: every target is at least the tensor's own TT rank (e: bond ranks 17 on modes
    of 4 hold at most rank 4), so the sketch loses nothing (1.3e-15 in the NumPy restatement)"""
    for cid in ("a", "e"):
        host = RC.train(cid)
        res = T._tt_lr_random_orthogonalise(_up(T, host), _up(T, RC.sketch(cid)))
        RC.close(RC.dense(T.to_host(res)), RC.dense(host), 1e-11)
