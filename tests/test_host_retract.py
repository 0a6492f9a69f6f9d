"""Fixed-rank retraction (`tt_rank_retraction`, `retraction_ranks`, `retract_lds`; reference
`src/tt_ops.py:132-152`): the rank rule, the composed path's host logic on the CPU (libttk replaced by the
NumPy emulator) against the reference's own outputs (tests/golden/retract.npz), and the host side of the
C ABI (`ttk_retract_lds` is a host function: no device needed).  The device run of the same value checks
is tests/test_gpu_retract.py."""
import ctypes
import os
import re

import numpy as np
import pytest

from tests import retract_cases as RC
from tests.emu_ttk import emulated_ttipm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SO = os.path.join(ROOT, "tensor-train-interior-point-method_amd", "libttk.so")


@pytest.fixture(scope="module")
def T():
    emulated_ttipm()
    from ttipm_amd import tt_ops
    return tt_ops


def test_rank_rule(T):
    f = T.retraction_ranks
    assert f([4, 4, 4], [1, 17, 17, 1], [20, 20]) == [1, 4, 4, 1]                 # the QR sweep lowers 17 -> 16 -> 4
    assert f([4, 4], [1, 5, 1], [3]) == [1, 3, 1]                                 # one bond
    assert f([2, 2, 2, 2], [1, 9, 9, 9, 1], [9, 9, 9]) == [1, 2, 4, 2, 1]         # q_i n_i and rho both bind
    assert f([4, 4, 4, 4, 4], [1, 4, 9, 6, 7, 1], [2, 7, 3, 5]) == [1, 2, 7, 3, 4, 1]   # case h
    assert f([3], [1, 1], []) == [1, 1]                                           # d = 1
    assert f([4] * 10, [1] + [12] * 9 + [1], [10] * 9) == [1, 4] + [10] * 7 + [4, 1]    # case e
    for cid in RC.VALUE + ("i",):
        inner, rk = RC.inner_and_ranks(RC.train(cid))
        assert f(inner, rk, RC.upper(cid)) == RC.ranks(cid), cid


@pytest.mark.parametrize("cid", RC.VALUE)
def test_composed_matches_reference(T, cid):
    host = RC.train(cid)
    tt = T.to_device(host)
    keep = list(tt)
    res = T.tt_rank_retraction(tt, RC.upper(cid))
    RC.check_result(cid, T.to_host(res))
    for t, h in zip(keep, RC.train(cid)):  # the caller's tensors are never written
        assert np.array_equal(T.D.read(t), h)


@pytest.mark.parametrize("cid", RC.REPRODUCE)
def test_full_rank_bound_reproduces_the_input(T, cid):
    """cases a, c, k and z: every bound is at least the tensor's own TT rank at its bond (c: ranks 17 on
    modes of 4 hold at most 4; z: only the null directions of the rank-2 bond go)"""
    host = RC.train(cid)
    res = T.tt_rank_retraction(T.to_device(host), RC.upper(cid))
    RC.close(RC.dense(T.to_host(res)), RC.dense(host), RC.RTOL)


def test_length_one_train_is_returned_unchanged(T):
    tt = T.to_device(RC.train("i"))
    first = tt[0]
    res = T.tt_rank_retraction(tt, RC.upper("i"))
    assert res is tt and res[0] is first
    RC.close(RC.dense(T.to_host(tt)), RC.reference_dense("i"), 0.0)


def test_header_declares_the_retraction():
    txt = open(os.path.join(ROOT, "include", "ttk.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    names = set(re.findall(r"\b(ttk_[a-z0-9_]+)\s*\(", txt))
    assert {"ttk_retract", "ttk_retract_lds"} <= names
    src = open(os.path.join(ROOT, "tensor-train-interior-point-method_amd", "_lib.py")).read()
    assert '"ttk_retract"' in src and '"ttk_retract_lds"' in src


@pytest.mark.skipif(not os.path.exists(SO), reason="libttk.so not built (run __graft_entry__.build())")
def test_lds_fit_is_host_arithmetic():
    """`ttk_retract_lds` through ctypes, no device: every value case that must fit does (w, the restart
    retraction, included), j does not, and invalid arguments give -1"""
    lib = ctypes.CDLL(SO)
    lib.ttk_retract_lds.restype = ctypes.c_int64
    lib.ttk_retract_lds.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    arr = lambda v: (ctypes.c_int64 * max(len(v), 1))(*v)  # noqa: E731

    def lds(inner, rk, up):
        return lib.ttk_retract_lds(len(inner), arr(inner), arr(rk), arr(up))

    for cid in RC.FIT:
        inner, rk = RC.inner_and_ranks(RC.train(cid))
        got = lds(inner, rk, RC.upper(cid))
        assert 0 <= got <= 160 * 1024, (cid, got)
    assert lds([16, 16, 16], [1, 96, 96, 1], [8, 8]) == -1          # case j: a 1.18 MB core
    assert lds([4, 4], [1, 0, 1], [3]) == -1                        # a zero rank
    assert lds([4, 0], [1, 5, 1], [3]) == -1                        # a zero extent
    assert lds([4, 4], [1, 5, 1], [0]) == -1                        # a zero bound
    assert lds([4], [1, 1], []) == -1                               # d = 1
    assert lds([4, 4], [2, 5, 1], [3]) == -1                        # a boundary rank of 2
    assert lds([4, 4], [1, 5, 2], [3]) == -1
    assert lds([4] * 33, [1] + [2] * 32 + [1], [2] * 32) == -1      # more than 32 cores
    assert lib.ttk_retract_lds(2, None, arr([1, 5, 1]), arr([3])) == -1


@pytest.mark.skipif(not os.path.exists(SO), reason="libttk.so not built (run __graft_entry__.build())")
def test_lds_bytes_of_the_benchmark_shapes():
    """the three plans' LDS bytes at the tools/bench_*.py shapes (d = 10, middle extent 4, bond ranks r,
    sketch ranks / bounds t, right Nystroem sketch t + 1), as measured before the planners were put on
    shared helpers; the last column also stands in profiles/retract_d10.txt"""
    lib = ctypes.CDLL(SO)
    arr = lambda v: (ctypes.c_int64 * len(v))(*v)  # noqa: E731
    for f, n in (("ttk_rand_orth_lds", 3), ("ttk_nystroem_lds", 4), ("ttk_retract_lds", 3)):
        getattr(lib, f).restype = ctypes.c_int64
        getattr(lib, f).argtypes = [ctypes.c_int] + [ctypes.c_void_p] * n
    d = 10
    for r, t, want in ((8, 4, (5152, 4448, 7232)), (12, 10, (17488, 13760, 16352)), (24, 20, (69792, 52704, 64448))):
        inner, rk = arr([4] * d), arr([1] + [r] * (d - 1) + [1])
        sk, sk1 = arr([1] + [t] * (d - 1) + [1]), arr([1] + [t + 1] * (d - 1) + [1])
        got = (lib.ttk_rand_orth_lds(d, inner, rk, sk), lib.ttk_nystroem_lds(d, inner, rk, sk, sk1),
               lib.ttk_retract_lds(d, inner, rk, arr([t] * (d - 1))))
        assert got == want, (r, t, got)
