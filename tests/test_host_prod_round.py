"""Rounding a product of two trains without building it (`ttk_prod_round_one`, reached through
`tt_ops.tt_fast_matrix_vec_mul`, `tt_fast_mat_mat_mul` and `tt_fast_hadamard` under TTIPM_PROD_ROUND_ONE), the
part that needs no device: the C ABI's declaration and binding, the host side of the plan
(`ttk_prod_round_one_lds` is a host function), and the public functions on the CPU (libttk replaced by the NumPy
emulator; switch off and on both take the composed path there) against the reference's own outputs
(tests/golden/prod_round.npz).  The device run: tests/test_gpu_prod_round.py."""
import ctypes
import os
import re

import numpy as np
import pytest

from tests import prod_round_cases as PC
from tests.emu_ttk import emulated_ttipm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SO = os.path.join(ROOT, "tensor-train-interior-point-method_amd", "libttk.so")
needs_lib = pytest.mark.skipif(not os.path.exists(SO), reason="libttk.so not built (run __graft_entry__.build())")


@pytest.fixture(scope="module")
def T():
    emulated_ttipm()
    from ttipm_amd import tt_ops
    return tt_ops


def test_header_and_binding_declare_the_calls():
    txt = open(os.path.join(ROOT, "include", "ttk.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    names = set(re.findall(r"\b(ttk_[a-z0-9_]+)\s*\(", txt))
    assert {"ttk_prod_round_one", "ttk_prod_round_one_lds"} <= names
    src = open(os.path.join(ROOT, "tensor-train-interior-point-method_amd", "_lib.py")).read()
    assert '"ttk_prod_round_one"' in src and '"ttk_prod_round_one_lds"' in src


I64 = ctypes.c_int64


def _arr(v):
    return None if v is None else (I64 * max(len(v), 1))(*v)


class Plan:
    """`ttk_prod_round_one_lds` through ctypes: host arithmetic on ranks and extents, no core pointer involved"""

    def __init__(self):
        self.lib = ctypes.CDLL(SO)
        self.lib.ttk_prod_round_one_lds.restype = I64
        self.lib.ttk_prod_round_one_lds.argtypes = [ctypes.c_int, ctypes.c_int] + [ctypes.c_void_p] * 5
        self.lib.ttk_round_one_lds.restype = I64
        self.lib.ttk_round_one_lds.argtypes = [ctypes.c_int] + [ctypes.c_void_p] * 3

    def __call__(self, kind, a_ranks, b_ranks, modes, prod=None, bound=None, d=None):
        d = len(a_ranks) - 1 if d is None else d
        return self.lib.ttk_prod_round_one_lds(kind, d, _arr(a_ranks), _arr(b_ranks), _arr(modes), prod, bound)


@needs_lib
def test_plan_is_the_round_one_plan_of_the_product_ranks(T):
    """every fitting case fits; `prod_ranks` are the products, `bound` the retraction's rule with no upper bound
    on them, the bytes those of `ttk_round_one_lds` at the product ranks; both outputs may be NULL; j does not
    fit"""
    plan = Plan()
    for cid in PC.VALUE:
        a, b = PC.factors(cid)
        k = PC.kind(cid)
        inner, rk = PC.prod_inner_and_ranks(k, a, b)
        d = len(inner)
        args = (k, PC.train_ranks(a), PC.train_ranks(b), PC.modes(k, a, b))
        prod, bound = (I64 * (d + 1))(), (I64 * (d + 1))()
        got = plan(*args, prod, bound)
        if cid == "j":
            assert got == -1 and plan(*args) == -1
            continue
        assert 0 <= got <= 160 * 1024, (cid, got)
        assert list(prod) == rk, cid
        assert list(bound) == T.retraction_ranks(inner, rk, [PC.BIG] * (d - 1)), cid
        assert all(q <= bd for q, bd in zip(PC.qranks(cid), bound)), cid
        assert got == plan.lib.ttk_round_one_lds(d, _arr(inner), _arr(rk), None), cid
        assert got == plan(*args) == plan(*args, prod, None) == plan(*args, None, bound), cid


@needs_lib
def test_plan_ignores_the_extents_a_kind_does_not_use():
    """`ttk_zipup`'s modes: kind 0 reads (m, n, -), kind 2 (i, -, -), kind 3 (i, j, -)"""
    plan = Plan()
    ra, rb = [1, 2, 1], [1, 3, 1]
    assert plan(0, ra, rb, [3, 2, 1, 3, 2, 1]) == plan(0, ra, rb, [3, 2, 0, 3, 2, -7]) >= 0
    assert plan(2, ra, rb, [4, 1, 1, 4, 1, 1]) == plan(2, ra, rb, [4, 0, 0, 4, 9, 9]) >= 0
    assert plan(3, ra, rb, [2, 3, 1, 2, 3, 1]) == plan(3, ra, rb, [2, 3, 0, 2, 3, 5]) >= 0


@needs_lib
def test_plan_rejects_invalid_arguments():
    plan = Plan()
    ra, rb, m = [1, 2, 3, 1], [1, 3, 2, 1], [2, 3, 2] * 3
    for k in range(4):
        assert plan(k, ra, rb, m) >= 0
    for k in (-1, 4, 7):
        assert plan(k, ra, rb, m) == -1                                    # kind outside 0 .. 3
    assert plan(1, [1, 1], [1, 1], m[:3]) == -1                            # d = 1
    assert plan(1, ra, rb, m, d=0) == -1 and plan(1, ra, rb, m, d=-2) == -1
    assert plan(1, None, rb, m, d=3) == -1 and plan(1, ra, None, m) == -1  # no rank array
    assert plan(1, ra, rb, None) == -1                                     # no modes
    assert plan(1, [1, 0, 3, 1], rb, m) == -1 and plan(1, ra, [1, 3, -2, 1], m) == -1   # a rank below 1
    for at in range(9):                                                    # an extent below 1, every position
        bad = list(m)
        bad[at] = 0
        assert plan(1, ra, rb, bad) == -1, at
    assert plan(0, ra, rb, [2, 0, 1] * 3) == -1 and plan(3, ra, rb, [2, 0, 1] * 3) == -1
    assert plan(2, ra, rb, [0, 1, 1] * 3) == -1
    for bad in ([2, 2, 3, 1], [1, 2, 3, 2]):                               # a boundary rank of 2, either factor
        assert plan(1, bad, rb, m) == -1 and plan(1, ra, bad, m) == -1
    assert plan(2, [1] + [2] * 32 + [1], [1] + [1] * 32 + [1], [4, 1, 1] * 33) == -1    # more than 32 cores
    assert plan(2, [1] + [2] * 31 + [1], [1] + [1] * 31 + [1], [4, 1, 1] * 32) >= 0
    assert plan(1, [1, 1 << 40, 1], [1, 2, 1], m[:6]) == -1                # a rank above the LDS capacity
    assert plan(1, [1, 1 << 33, 1], [1, 1 << 33, 1], m[:6]) == -1          # a product that leaves 64 bits
    assert plan(1, [1, 200, 1], [1, 200, 1], m[:6]) == -1                  # product rank 40000
    assert plan(1, [1, 2, 1], [1, 2, 1], [1 << 20, 2, 1 << 20] * 2) == -1  # a product of extents above it
    assert plan(0, [1, 2, 1], [1, 2, 1], [4, 1 << 40, 1] * 2) == -1        # a contracted extent above it
    assert plan(1, [1, 48, 48, 1], [1, 2, 2, 1], [4, 4, 4] * 3) == -1      # a 1.18 MB product core


def _check_public(T, cid):
    host = PC.factors(cid)
    a, b = PC.upload(T, cid, host)
    keep = (list(a), list(b))
    np.random.seed(7)
    st0 = np.random.get_state()
    res = PC.public(T, cid, a, b)
    st1 = np.random.get_state()
    assert st0[0] == st1[0] and np.array_equal(st0[1], st1[1]) and st0[2:] == st1[2:]
    PC.check_result(cid, PC.finish(T, cid, res))
    for t, k, h in zip((a, b), keep, host):
        assert len(t) == len(k) and all(x is y for x, y in zip(t, k))
        assert all(np.array_equal(T.D.read(x), y) for x, y in zip(t, h))


@pytest.mark.parametrize("switch", (False, True))
@pytest.mark.parametrize("cid", PC.VALUE)
def test_public_functions_match_reference(T, monkeypatch, cid, switch):
    """ranks exactly the reference's and the dense tensor to 1e-11, switch off and on (without a GPU both take the
    composed path); the caller's tensors and lists are unchanged, and nothing is drawn from NumPy's stream"""
    monkeypatch.setattr(T, "PROD_ROUND_ONE", switch)
    _check_public(T, cid)


def test_all_three_public_functions_are_covered():
    assert {PC.kind(c) for c in PC.FIT} == {0, 1, 2, 3}


def test_switch_is_off_by_default_and_not_taken_off_the_gpu(T, monkeypatch):
    """the switch reads TTIPM_PROD_ROUND_ONE; switched on without a GPU, `_prod_native` declines"""
    assert T.PROD_ROUND_ONE is (os.environ.get("TTIPM_PROD_ROUND_ONE", "0") == "1")
    monkeypatch.setattr(T, "PROD_ROUND_ONE", True)
    a, b = PC.upload(T, "h")
    assert T._prod_native(2, a, b, PC.eps("h")) is None


@pytest.mark.parametrize("cid", PC.FIT)
def test_materialised_product_is_the_composed_product(T, cid):
    """the test-side NumPy product has the composed path's layout and, to rounding, its numbers: the public call
    at eps = 0 returns the unrounded Kronecker-bond cores"""
    a, b = PC.factors(cid)
    k = PC.kind(cid)
    da, db = PC.upload(T, cid, (a, b))
    got = T.to_host(PC.fast(T, k)(da, db, 0.0))
    want = PC.materialised(k, a, b)
    inner, rk = PC.prod_inner_and_ranks(k, a, b)
    assert len(got) == len(want)
    for g, w, n, r0, r1 in zip(got, want, inner, rk[:-1], rk[1:]):
        assert g.shape == w.shape and g.size == r0 * n * r1
        assert np.max(np.abs(g - w)) <= 1e-14 * np.max(np.abs(w))
        if k >= 2:
            assert np.array_equal(g, w)
