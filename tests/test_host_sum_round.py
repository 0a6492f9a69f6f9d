"""Rounding a weighted sum of trains without building it (`ttk_sum_round_one`, `tt_ops.tt_sum_rank_reduce` and
its PSD / mask variants, TTIPM_SUM_ROUND_ONE), the part that needs no device: the C ABI's declaration and
binding, the host side of the plan (`ttk_sum_round_one_lds` is a host function), the public functions on the
CPU (libttk replaced by the NumPy emulator; switch off and on both build the sum there) against the
reference's own outputs (tests/golden/sum_round.npz), and the `tt_ipm` helpers, which with the switch off must
make the library calls and random draws of the expressions they replace.  The device run:
tests/test_gpu_sum_round.py."""
import ctypes
import os
import re

import numpy as np
import pytest

from tests import sum_round_cases as SC
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
    assert {"ttk_sum_round_one", "ttk_sum_round_one_lds"} <= names
    assert "ttk_sum_term" in txt
    src = open(os.path.join(ROOT, "tensor-train-interior-point-method_amd", "_lib.py")).read()
    assert '"ttk_sum_round_one"' in src and '"ttk_sum_round_one_lds"' in src


class Term(ctypes.Structure):
    _fields_ = [("cores", ctypes.c_void_p), ("ranks", ctypes.c_void_p), ("coef", ctypes.c_double),
                ("transpose", ctypes.c_int)]


I64 = ctypes.c_int64


def _arr(v):
    return (I64 * max(len(v), 1))(*v)


class Plan:
    """`ttk_sum_round_one_lds` through ctypes.  The function is host arithmetic: it checks that the core
    pointers are not null and never follows them, so the table holds a dummy address."""

    def __init__(self):
        self.lib = ctypes.CDLL(SO)
        self.lib.ttk_sum_round_one_lds.restype = I64
        self.lib.ttk_sum_round_one_lds.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_int] + [ctypes.c_void_p] * 3
        self.lib.ttk_round_one_lds.restype = I64
        self.lib.ttk_round_one_lds.argtypes = [ctypes.c_int] + [ctypes.c_void_p] * 3

    def __call__(self, inner, term_ranks, coef=None, tr=None, sums=None, bound=None, nterms=None, cores="dummy",
                 table=True):
        d, n = len(inner), len(term_ranks)
        keep = []
        terms = (Term * max(n, 1))()
        for j, rk in enumerate(term_ranks):
            ptrs = (ctypes.c_void_p * max(d, 1))(*([64] * d))
            if cores == "null entry" and j == n - 1:
                ptrs[d - 1] = None
            r = _arr(rk) if rk is not None else None
            keep += [ptrs, r]
            terms[j] = Term(None if cores == "null table" and j == 0 else ctypes.cast(ptrs, ctypes.c_void_p),
                            ctypes.cast(r, ctypes.c_void_p) if r is not None else None,
                            1.0 if coef is None else coef[j], 0 if tr is None else tr[j])
        return self.lib.ttk_sum_round_one_lds(d, _arr(inner) if inner else None, n if nterms is None else nterms,
                                              terms if table else None, sums, bound)


@needs_lib
def test_plan_is_the_round_one_plan_of_the_summed_ranks(T):
    """every fitting case fits; `sum_ranks` are the sums, `bound` the retraction's rule with no upper bound on
    them, the bytes those of `ttk_round_one_lds` at the summed ranks; both outputs may be NULL; j does not fit"""
    plan = Plan()
    for cid in SC.VALUE:
        trains = SC.stored(cid)
        ts = SC.terms(cid, trains)
        inner, rk = SC.sum_inner_and_ranks(cid, trains)
        d = len(inner)
        sums, bound = (I64 * (d + 1))(), (I64 * (d + 1))()
        got = plan(inner, [SC.term_ranks(t) for t in ts], SC.coeffs(cid), [int(t) for t in SC.transposed(cid)],
                   sums, bound)
        if cid == "j":
            assert got == -1
            continue
        assert 0 <= got <= 160 * 1024, (cid, got)
        assert list(sums) == rk, cid
        assert list(bound) == T.retraction_ranks(inner, rk, [SC.BIG] * (d - 1)), cid
        assert all(q <= b for q, b in zip(SC.qranks(cid), bound)), cid
        assert got == plan.lib.ttk_round_one_lds(d, _arr(inner), _arr(rk), None), cid
        assert got == plan(inner, [SC.term_ranks(t) for t in ts]), cid


@needs_lib
def test_plan_rejects_invalid_arguments():
    plan = Plan()
    ok = ([4, 4], [[1, 3, 1], [1, 2, 1]])
    assert plan(*ok) >= 0
    assert plan([4], [[1, 1]]) == -1                                       # d = 1
    assert plan([4, 4], [[1, 3, 1], [1, 0, 1]]) == -1                      # a zero rank, in the second term
    assert plan([4, 0], ok[1]) == -1                                       # a zero extent
    assert plan([4, 4], [[1, 3, 1], [2, 2, 1]]) == -1                      # a boundary rank of 2
    assert plan([4, 4], [[1, 3, 2], [1, 2, 1]]) == -1
    assert plan([4] * 33, [[1] + [2] * 32 + [1]] * 2) == -1                # more than 32 cores
    assert plan([4, 4], []) == -1                                          # no term
    assert plan([4, 4], [[1, 2, 1]] * 5) == -1                             # five terms
    assert plan([4, 4], [[1, 2, 1]] * 4) >= 0
    assert plan(*ok, nterms=0) == -1 and plan(*ok, nterms=-1) == -1
    for bad in (float("nan"), float("inf"), -float("inf")):
        assert plan(*ok, coef=[1.0, bad]) == -1                            # a non-finite weight
    for bad in (2, -1):
        assert plan(*ok, tr=[0, bad]) == -1                                # a transpose flag that is no flag
    assert plan(*ok, table=False) == -1                                    # no term table
    assert plan(*ok, cores="null table") == -1 and plan(*ok, cores="null entry") == -1
    assert plan([4, 4], [[1, 3, 1], None]) == -1                           # no rank array
    assert plan([], ok[1]) == -1                                           # no extents (d = 0)
    assert plan([16, 16, 16], [[1, 48, 48, 1]] * 2) == -1                  # a 1.18 MB summed core
    assert plan([4, 4], [[1, 1 << 40, 1]] * 2) == -1


def _upload(T, cid):
    host = SC.stored(cid)
    return host, [T.to_device(t) for t in host]


@pytest.mark.parametrize("switch", (False, True))
@pytest.mark.parametrize("cid", SC.VALUE)
def test_public_functions_match_reference(T, monkeypatch, cid, switch):
    """ranks exactly the reference's and the dense tensor to 1e-11, switch off and on (on the CPU both build the
    sum); the caller's tensors and lists are unchanged, and nothing is drawn from either random stream"""
    from ttipm_amd import rng as _rng
    monkeypatch.setattr(T, "SUM_ROUND_ONE", switch)
    host, dev = _upload(T, cid)
    keep = [list(t) for t in dev]
    np.random.seed(7)
    st0 = np.random.get_state()
    assert _rng.R() is np.random.mtrand._rand
    res = SC.public(T, cid, dev)
    st1 = np.random.get_state()
    assert st0[0] == st1[0] and np.array_equal(st0[1], st1[1]) and st0[2:] == st1[2:]
    SC.check_result(cid, T.to_host(res))
    for t, k, h in zip(dev, keep, host):
        assert len(t) == len(k) and all(a is b for a, b in zip(t, k))
        assert all(np.array_equal(T.D.read(a), b) for a, b in zip(t, h))


def test_a_threads_private_stream_is_left_alone(T):
    """a solve thread's own MT19937 (`rng.private()`) is what `tt_scale` draws from there; the sum roundings with
    weights (the symmetrise pattern, the tracked variants) leave it, and NumPy's global stream, as they were"""
    import threading
    from ttipm_amd import rng as _rng
    seen = {}

    def work():
        rs = _rng.private()
        rs.seed(5)
        before = rs.get_state()
        for cid in ("n", "s", "p", "m"):
            SC.check_result(cid, T.to_host(SC.public(T, cid, [T.to_device(t) for t in SC.stored(cid)])))
        after = rs.get_state()
        seen["same"] = np.array_equal(before[1], after[1]) and before[2:] == after[2:]

    np.random.seed(3)
    g0 = np.random.get_state()
    th = threading.Thread(target=work)
    th.start()
    th.join()
    g1 = np.random.get_state()
    assert seen == {"same": True}
    assert np.array_equal(g0[1], g1[1]) and g0[2:] == g1[2:]


@pytest.mark.parametrize("cid", ("c", "o", "n", "u", "t", "s", "z", "w"))
def test_composed_sum_has_tt_adds_layout(T, cid):
    """the sum the composed path builds, bit for bit: blocks at the prefix sums of the ranks, core 0 weighted,
    transposed terms swapped, exact zeros elsewhere -- the train `ttk_sum_round_one` forms in its loads"""
    host, dev = _upload(T, cid)
    got = T.to_host(T._sum_composed(SC.terms(cid, dev), SC.coeffs(cid), SC.transposed(cid)))
    want = SC.materialised(cid, host)
    assert len(got) == len(want)
    for a, b in zip(got, want):
        assert a.shape == b.shape and np.array_equal(a, b)


def test_defaults_and_trivial_inputs(T, monkeypatch):
    """coeffs and transposed default to ones and no transposition; d = 1 and a single all-rank-1 term go the way
    `tt_rank_reduce` sends them (returned as they are); the switch is off by default"""
    assert T.SUM_ROUND_ONE is (os.environ.get("TTIPM_SUM_ROUND_ONE", "0") == "1")
    for switch in (False, True):
        monkeypatch.setattr(T, "SUM_ROUND_ONE", switch)
        one = T.to_device([np.arange(4.0).reshape(1, 4, 1)])
        res = T.tt_sum_rank_reduce([one])
        assert len(res) == 1 and res[0] is one[0]
        res = T.tt_sum_rank_reduce([one, one], [1.0, 2.0])
        assert np.array_equal(T.D.read(res[0]), 3.0 * np.arange(4.0).reshape(1, 4, 1))
        flat = T.to_device([np.ones((1, 4, 1)) * (k + 1) for k in range(3)])
        res = T.tt_sum_rank_reduce([flat], eps=1e-3)
        assert all(a is b for a, b in zip(res, flat))
        host, dev = _upload(T, "c")
        a = T.to_host(T.tt_sum_rank_reduce(dev, eps=SC.eps("c")))
        b = T.to_host(T.tt_sum_rank_reduce(dev, [1.0, 1.0], [False, False], eps=SC.eps("c")))
        assert all(np.array_equal(x, y) for x, y in zip(a, b))


class Recorder:
    """the emulated library, every call noted as (name, its float arguments)"""

    def __init__(self, lib):
        self._lib, self.calls = lib, []

    def __getattr__(self, name):
        f = getattr(self._lib, name)
        if not callable(f):
            return f

        def call(*args):
            self.calls.append((name, tuple(a for a in args if isinstance(a, float))))
            return f(*args)
        return call


def _old_expressions(T):
    """the expressions of tt_ipm.py that the helpers replace, as they stood"""
    sym = lambda M, e: T.tt_rank_reduce(T.tt_scale(0.5, T.tt_add(M, T.tt_transpose(M))), eps=e)  # noqa: E731
    psd = lambda M, e: T.tt_psd_rank_reduce(T.tt_scale(0.5, T.tt_add(M, T.tt_transpose(M))), eps=e)  # noqa: E731
    msk = lambda M, m, e: T.tt_mask_rank_reduce(T.tt_scale(0.5, T.tt_add(M, T.tt_transpose(M))), m, eps=e)  # noqa: E731
    return {
        "sym": lambda X, DX, m, a, e: sym(X, e),
        "psd": lambda X, DX, m, a, e: psd(X, e),
        "mask": lambda X, DX, m, a, e: msk(X, m, e),
        "step": lambda X, DX, m, a, e: sym(T.tt_add(X, T.tt_scale(a, DX)), e),
        "step_psd": lambda X, DX, m, a, e: psd(T.tt_add(X, T.tt_scale(a, DX)), e),
        "step_mask": lambda X, DX, m, a, e: msk(T.tt_add(X, T.tt_scale(a, DX)), m, e),
        "add": lambda X, DX, m, a, e: T.tt_rank_reduce(T.tt_add(X, DX), eps=e),
        "axpy": lambda X, DX, m, a, e: T.tt_rank_reduce(T.tt_add(X, T.tt_scale(a, DX)), e),
    }


@pytest.mark.parametrize("switch", (False, True))
@pytest.mark.parametrize("name", ("sym", "psd", "mask", "step", "step_psd", "step_mask", "add", "axpy"))
def test_ipm_helpers_make_the_old_library_calls(T, monkeypatch, name, switch):
    """without the native path (switch off; on the CPU also switch on) a helper is the expression it replaced: the
    same library calls with the same scalars in the same order, the same bits out, the same MT19937 state"""
    from ttipm_amd import tt_ipm
    monkeypatch.setattr(T, "SUM_ROUND_ONE", switch)
    host = SC.stored("m")
    X, DX = T.to_device(host[0]), T.to_device(host[1])
    mask = T.to_device(SC.mask("m"))
    rec = Recorder(T.D.lib)
    monkeypatch.setattr(T.D, "lib", rec)
    runs = []
    for f in (_old_expressions(T)[name], SC.helper_calls(tt_ipm)[name]):
        np.random.seed(11)
        del rec.calls[:]
        res = T.to_host(f(list(X), list(DX), mask, 0.37, SC.eps("m")))
        runs.append((list(rec.calls), res, np.random.get_state()))
    (c0, r0, s0), (c1, r1, s1) = runs
    assert len(c0) > 3 and c0 == c1
    assert len(r0) == len(r1) and all(np.array_equal(a, b) for a, b in zip(r0, r1))
    assert np.array_equal(s0[1], s1[1]) and s0[2:] == s1[2:]
    np.random.seed(11)
    fresh = np.random.get_state()
    drew = not (np.array_equal(fresh[1], s1[1]) and fresh[2] == s1[2])
    assert drew == (name != "add")  # every expression but the plain sum goes through `tt_scale`
