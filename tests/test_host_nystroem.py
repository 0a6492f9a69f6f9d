"""Generalised Nystroem rounding (`_tt_generalised_nystroem`, `tt_generalised_nystroem`, `tt_sketch`,
`tt_sketch_like`; reference `src/tt_ops.py:232-300`): the composed path's host logic on the CPU, libttk
replaced by the NumPy emulator, against the reference's own outputs (tests/golden/nystroem.npz).  The
device run of the same checks is tests/test_gpu_nystroem.py."""
import numpy as np
import pytest

from tests import nystroem_cases as NC
from tests.emu_ttk import emulated_ttipm


@pytest.fixture(scope="module")
def T():
    emulated_ttipm()
    from ttipm_amd import tt_ops
    return tt_ops


def _up(T, tt):
    return T.to_device(tt)


def _case(T, cid):
    g1, g2 = NC.sketches(cid)
    return _up(T, NC.train(cid)), _up(T, g1), _up(T, g2)


@pytest.mark.parametrize("cid", NC.VALUE)
def test_composed_matches_reference(T, cid):
    host = NC.train(cid)
    tt, g1, g2 = _case(T, cid)
    keep, keep1, keep2 = list(tt), list(g1), list(g2)
    res = T._tt_generalised_nystroem(tt, g1, g2)
    assert res is tt  # rebound in place, like the reference's list mutation
    NC.check_result(cid, T.to_host(res))
    for t, h in zip(keep, host):  # the caller's tensors are never written
        assert np.array_equal(T.D.read(t), h)
    for ts, hs in zip((keep1, keep2), NC.sketches(cid)):
        for t, h in zip(ts, hs):
            assert np.array_equal(T.D.read(t), h)


@pytest.mark.parametrize("cid", NC.FIT)
def test_contractions_match_reference(T, cid):
    tt, g1, g2 = _case(T, cid)
    for which, W in (("WL", T.tt_lr_contraction(tt, g1)), ("WR", T.tt_rl_contraction(tt, g2))):
        want = NC.contractions(cid, which)
        assert len(W) == len(want)
        for w, v in zip(W, want):
            assert tuple(w.shape) == v.shape
            NC.close(T.D.read(w), v, 1e-12)


def test_rank_rule(T):
    f = T.nystroem_ranks
    assert f([1, 6, 6, 1], [1, 3, 3, 1], [1, 4, 4, 1]) == [1, 3, 3, 1]            # the reference's l + 1
    assert f([1, 2, 7, 3, 5, 1], [1, 2, 2, 3, 1, 1], [1, 4, 4, 5, 3, 1]) == [1, 2, 2, 3, 1, 1]   # case h
    assert f([1, 8, 8, 1], [1, 5, 2, 1], [1, 3, 4, 1]) == [1, 3, 2, 1]            # a right sketch below the left
    assert f([2, 9, 3], [2, 4, 3], [2, 4, 3]) == [2, 4, 3]                        # boundary ranks stay
    for cid in NC.VALUE + ("z",):
        rk = [[1] + [c.shape[-1] for c in t] for t in (NC.train(cid),) + NC.sketches(cid)]
        assert f(*rk)[1:-1] == [int(v) for v in NC.G[f"{cid}/ranks"]]


def test_right_sketch_below_the_left(T):
    """rranks < lranks: the output ranks follow the right sketch, and with both above the tensor's own
    rank (case a: 3, so P keeps full rank) the input is reproduced"""
    host = NC.train("a")
    rs = np.random.RandomState(5)
    g1 = [rs.randn(a, 4, b) for a, b in zip([1, 5, 5, 5, 5], [5, 5, 5, 5, 1])]
    g2 = [rs.randn(a, 4, b) for a, b in zip([1, 3, 3, 3, 3], [3, 3, 3, 3, 1])]
    res = T.to_host(T._tt_generalised_nystroem(_up(T, host), _up(T, g1), _up(T, g2)))
    assert [c.shape[0] for c in res[1:]] == [3, 3, 3, 3]
    NC.close(NC.dense(res), NC.dense(host), 1e-11)


def test_transposed_case_is_well_posed(T):
    """`NC.transposed_case()` (the device test of the bond SVD's transposed branch) by the rule the
    fixture's value cases pass on import: 50 x the largest relative max-abs change of the dense result
    over 5 reruns, every train entry multiplied by 1 + 1.1e-16 N(0, 1), stays within 1e-11"""
    tt, g1, g2 = NC.transposed_case()

    def run(train):
        res = T.to_host(T._tt_generalised_nystroem(_up(T, train), _up(T, g1), _up(T, g2)))
        assert [c.shape[0] for c in res[1:]] == [3, 3]
        return NC.dense(res)

    ref = run(tt)
    nrng = np.random.default_rng(3)
    noise = 0.0
    for _ in range(5):
        got = run([c * (1.0 + 1.1e-16 * nrng.standard_normal(c.shape)) for c in tt])
        noise = max(noise, float(np.max(np.abs(got - ref)) / np.max(np.abs(ref))))
    print("noise", noise)
    assert NC.NOISE_MULTIPLE * noise <= NC.RTOL, noise


@pytest.mark.parametrize("cid", NC.PUBLIC)
def test_public_call_matches_reference_and_rng_stream(T, cid):
    tt = _up(T, NC.train(cid))
    np.random.seed(int(NC.G[f"{cid}/pub_seed"]))
    res = T.tt_generalised_nystroem(tt, NC.targets(cid))
    NC.check_rng_state(cid)
    assert res is tt
    NC.check_result(cid, T.to_host(res), "pub_")


def test_length_one_train_is_returned_unchanged(T):
    host = NC.train("i")
    tt = _up(T, host)
    first = tt[0]
    st = np.random.get_state()
    res = T.tt_generalised_nystroem(tt, [])
    assert res is tt and res[0] is first
    st2 = np.random.get_state()
    assert np.array_equal(st2[1], st[1]) and st2[2:] == st[2:]  # nothing drawn
    NC.close(NC.dense(T.to_host(tt)), NC.reference_dense("i"), 0.0)


@pytest.mark.parametrize("cid", NC.REPRODUCE)
def test_target_at_rank_reproduces_the_input(T, cid):
    """cases a, e and k: every target is at least the tensor's own TT rank (e: bond ranks 17 on modes
    of 4 hold at most rank 4), so the two-sided sketch loses nothing"""
    host = NC.train(cid)
    tt, g1, g2 = _case(T, cid)
    res = T._tt_generalised_nystroem(tt, g1, g2)
    NC.close(NC.dense(T.to_host(res)), NC.dense(host), 1e-11)


def test_singular_case_returns_with_the_right_shapes(T):
    tt, g1, g2 = _case(T, "z")
    with np.errstate(all="ignore"):
        res = T._tt_generalised_nystroem(tt, g1, g2)
    NC.check_shapes("z", T.to_host(res))


def test_sketches_follow_numpys_stream(T):
    """tt_sketch / tt_sketch_like: the reference's formula on np.random.randn after the same seed,
    the same MT19937 state afterwards, full rank list with the boundaries"""
    ranks = [1, 3, 5, 2, 1]
    for shape, like in (((4,), None), ((2, 2), None), ((), None), (None, NC.train("b")[:4])):
        np.random.seed(31)
        got = T.tt_sketch(shape, ranks) if like is None else T.tt_sketch_like(_up(T, like), ranks)
        st = np.random.get_state()
        np.random.seed(31)
        want = []
        for i, (a, b) in enumerate(zip(ranks[:-1], ranks[1:])):
            shp = shape if like is None else like[i].shape[1:-1]
            want.append(np.divide(1, a * np.prod(shp) * b) * np.random.randn(a, *shp, b))
        st2 = np.random.get_state()
        assert np.array_equal(st[1], st2[1]) and st[2:] == st2[2:]
        assert len(got) == len(want)
        for g, w in zip(T.to_host(got), want):
            assert g.shape == w.shape and np.array_equal(g, w)
