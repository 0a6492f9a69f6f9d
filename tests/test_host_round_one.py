"""One-launch eps-truncating rounding (`ttk_round_one`, `tt_ops.round_one_lds`, TTIPM_ROUND_ONE; reference
`cy_src/tt_ops_cy.pyx:179-388`), the part that needs no device: the C ABI's declaration and binding, the
host side of the plan (`ttk_round_one_lds` is a host function), and the public roundings on the CPU
(libttk replaced by the NumPy emulator) against the reference's own outputs (tests/golden/round_one.npz)
with the switch off and on -- on the CPU, on takes today's path.  The device run of the same value checks
is tests/test_gpu_round_one.py."""
import ctypes
import os
import re

import numpy as np
import pytest

from tests import round_one_cases as RC
from tests.emu_ttk import emulated_ttipm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SO = os.path.join(ROOT, "tensor-train-interior-point-method_amd", "libttk.so")
BIG = 1 << 62


@pytest.fixture(scope="module")
def T():
    emulated_ttipm()
    from ttipm_amd import tt_ops
    return tt_ops


def test_header_declares_the_rounding():
    txt = open(os.path.join(ROOT, "include", "ttk.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    names = set(re.findall(r"\b(ttk_[a-z0-9_]+)\s*\(", txt))
    assert {"ttk_round_one", "ttk_round_one_lds"} <= names
    src = open(os.path.join(ROOT, "tensor-train-interior-point-method_amd", "_lib.py")).read()
    assert '"ttk_round_one"' in src and '"ttk_round_one_lds"' in src


def test_fixture_cases_do_what_they_are_there_for(T):
    """f truncates to 1, a and n keep everything, o goes to rank 1 everywhere, e truncates at three bonds or
    more, and in t the truncation at bond 1 flips bond 2's Jacobi orientation against the bound plan's"""
    f = T.retraction_ranks
    bound = {}
    for cid in RC.VALUE:
        inner, rk = RC.inner_and_ranks(RC.train(cid))
        bound[cid] = f(inner, rk, [BIG] * (len(inner) - 1))
        assert all(q <= b for q, b in zip(RC.qranks(cid), bound[cid])), cid
    assert RC.qranks("f") == [1, 1, 1]
    assert RC.qranks("a") == bound["a"] == [1, 3, 3, 3, 1] and RC.qranks("n") == bound["n"]
    assert RC.qranks("c") == bound["c"] == [1, 4, 4, 1]
    assert set(RC.qranks("o")) == {1}
    assert sum(q < b for q, b in zip(RC.qranks("e"), bound["e"])) >= 3
    q, b = RC.qranks("t"), bound["t"]
    rho2 = 8  # min(4 * 4, 8) after the QR sweep
    assert q[1] * 4 <= rho2 < b[1] * 4
    for cid in RC.TRACKED:
        assert RC.ranks(cid) == [1] + [v + 1 for v in RC.qranks(cid)[1:-1]] + [1]


def _lib():
    lib = ctypes.CDLL(SO)
    for f, n in (("ttk_round_one_lds", 3), ("ttk_retract_lds", 3)):
        getattr(lib, f).restype = ctypes.c_int64
        getattr(lib, f).argtypes = [ctypes.c_int] + [ctypes.c_void_p] * n
    return lib


INVALID = (([4], [1, 1]),                                   # d = 1
           ([4, 4], [1, 0, 1]),                             # a zero rank
           ([4, 0], [1, 5, 1]),                             # a zero extent
           ([4, 4], [2, 5, 1]), ([4, 4], [1, 5, 2]),        # a boundary rank of 2
           ([4] * 33, [1] + [2] * 32 + [1]))                # more than 32 cores


@pytest.mark.skipif(not os.path.exists(SO), reason="libttk.so not built (run __graft_entry__.build())")
def test_lds_fit_and_bound_ranks_are_host_arithmetic(T):
    """`ttk_round_one_lds` through ctypes, no device: every fitting case fits, its bound ranks are the
    retraction's rule with no upper bound and hold the reference's ranks, j and invalid arguments give -1"""
    lib = _lib()
    arr = lambda v: (ctypes.c_int64 * max(len(v), 1))(*v)  # noqa: E731

    def lds(inner, rk, bound=None):
        return lib.ttk_round_one_lds(len(inner), arr(inner), arr(rk), bound)

    for cid in RC.FIT:
        inner, rk = RC.inner_and_ranks(RC.train(cid))
        bound = (ctypes.c_int64 * len(rk))()
        got = lds(inner, rk, bound)
        assert 0 <= got <= 160 * 1024, (cid, got)
        assert lds(inner, rk) == got  # bound may be NULL
        assert list(bound) == T.retraction_ranks(inner, rk, [BIG] * (len(inner) - 1)), cid
        assert all(q <= b for q, b in zip(RC.qranks(cid), bound)), cid
    assert lds([16, 16, 16], [1, 96, 96, 1]) == -1          # case j: a 1.18 MB core
    for inner, rk in INVALID:
        assert lds(inner, rk) == -1, (inner, rk)
    assert lib.ttk_round_one_lds(2, None, arr([1, 5, 1]), None) == -1
    assert lib.ttk_round_one_lds(2, arr([4, 4]), None, None) == -1


@pytest.mark.skipif(not os.path.exists(SO), reason="libttk.so not built (run __graft_entry__.build())")
def test_retraction_plan_is_unchanged():
    """the adaptive plan's extra LDS words are its own: `ttk_retract_lds` at the tools/bench_retract.py shapes
    still gives the bytes of profiles/retract_d10.txt, and the adaptive plan at the same trains needs at
    least as much (its bounds are the retraction's without `upper`)"""
    lib = _lib()
    arr = lambda v: (ctypes.c_int64 * len(v))(*v)  # noqa: E731
    d = 10
    for r, t, want in ((8, 4, 7232), (12, 10, 16352), (24, 20, 64448)):
        inner, rk = arr([4] * d), arr([1] + [r] * (d - 1) + [1])
        assert lib.ttk_retract_lds(d, inner, rk, arr([t] * (d - 1))) == want
        one = lib.ttk_round_one_lds(d, inner, rk, None)
        assert want < one <= 160 * 1024, (r, one)


@pytest.mark.parametrize("switch", (False, True))
@pytest.mark.parametrize("cid", RC.VALUE)
def test_public_functions_match_reference(T, monkeypatch, cid, switch):
    """ranks exactly the reference's and the dense tensor to 1e-11, with the switch off and on (on the CPU the
    switch changes nothing: the path it guards is the GPU's)"""
    monkeypatch.setattr(T, "ROUND_ONE", switch)
    host = RC.train(cid)
    tt = T.to_device(host)
    keep = list(tt)
    res = RC.public(T, cid, tt)
    RC.check_result(cid, T.to_host(res))
    for t, h in zip(keep, host):  # the caller's tensors are never written
        assert np.array_equal(T.D.read(t), h)


@pytest.mark.parametrize("switch", (False, True))
@pytest.mark.parametrize("cid", RC.UNCHANGED)
def test_trivial_trains_are_returned_unchanged(T, monkeypatch, cid, switch):
    monkeypatch.setattr(T, "ROUND_ONE", switch)
    tt = T.to_device(RC.train(cid))
    cores = list(tt)
    for f in (T.tt_rank_reduce, T.tt_psd_rank_reduce):
        res = f(tt, RC.eps(cid))
        assert res is tt and all(a is b for a, b in zip(res, cores))
    assert T.round_one_lds(tt[:1]) == -1
