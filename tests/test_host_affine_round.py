"""Rounding a weighted sum of trains and products of two trains without building it (`ttk_affine_round_one`,
reached through `tt_ops.tt_affine_rank_reduce` under TTIPM_AFFINE_ROUND_ONE), the part that needs no device: the C
ABI's declaration and binding, the host side of the plan (`ttk_affine_round_one_lds` is a host function), and the
public function on the CPU (libttk replaced by the NumPy emulator; switch off and on both take the composed path
there) against the reference's own outputs (tests/golden/affine_round.npz).  The device run:
tests/test_gpu_affine_round.py."""
import ctypes
import os
import re

import numpy as np
import pytest

from tests import affine_round_cases as AC
from tests import prod_round_cases as PC
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
    assert {"ttk_affine_round_one", "ttk_affine_round_one_lds"} <= names
    assert re.search(r"\}\s*ttk_affine_term\s*;", txt)
    src = open(os.path.join(ROOT, "tensor-train-interior-point-method_amd", "_lib.py")).read()
    assert '"ttk_affine_round_one"' in src and '"ttk_affine_round_one_lds"' in src


@needs_lib
def test_library_exports_the_calls():
    lib = ctypes.CDLL(SO)
    assert hasattr(lib, "ttk_affine_round_one") and hasattr(lib, "ttk_affine_round_one_lds")


I64, VP = ctypes.c_int64, ctypes.c_void_p


class Term(ctypes.Structure):
    """`ttk_affine_term` as include/ttk.h lays it out"""
    _fields_ = [("kind", ctypes.c_int), ("transpose", ctypes.c_int), ("coef", ctypes.c_double), ("a", VP),
                ("a_ranks", VP), ("b", VP), ("b_ranks", VP), ("modes", VP)]


def _arr(v):
    return None if v is None else (I64 * max(len(v), 1))(*v)


def _addr(x):
    return None if x is None else ctypes.cast(x, VP)


ONE = ctypes.c_double(1.0)  # what the core tables of the host tests point at: never read by the plan


class Plan:
    """`ttk_affine_round_one_lds` through ctypes: host arithmetic on ranks and extents.  A term is given as
    (kind, a_ranks, b_ranks, modes[, coef, transpose]); its core tables point at one double the plan never reads.
    A rank or modes array given as None is passed as NULL.  A seventh entry changes the tables: "no a" / "no b"
    pass a NULL table, "extra b" gives a plain term a b table, ("nullcore", k) puts a NULL at core k of a."""

    def __init__(self):
        self.lib = ctypes.CDLL(SO)
        self.lib.ttk_affine_round_one_lds.restype = I64
        self.lib.ttk_affine_round_one_lds.argtypes = [ctypes.c_int, VP, ctypes.c_int, VP, VP, VP]
        self.lib.ttk_round_one_lds.restype = I64
        self.lib.ttk_round_one_lds.argtypes = [ctypes.c_int] + [VP] * 3
        self.lib.ttk_sum_round_one_lds.restype = I64
        self.lib.ttk_sum_round_one_lds.argtypes = [ctypes.c_int, VP, ctypes.c_int, VP, VP, VP]
        self.lib.ttk_prod_round_one_lds.restype = I64
        self.lib.ttk_prod_round_one_lds.argtypes = [ctypes.c_int, ctypes.c_int] + [VP] * 5

    def records(self, d, terms):
        keep, recs = [], []
        n = max(d, 1)
        for t in terms:
            kind, ar, br, modes = t[:4]
            coef, tr = (t[4], t[5]) if len(t) > 4 else (1.0, 0)
            tab = lambda null=None: (VP * n)(*[None if k == null else ctypes.addressof(ONE)  # noqa: E731
                                               for k in range(n)])
            pa = None if t[-1] == "no a" else tab(t[-1][1] if isinstance(t[-1], tuple) and t[-1][0] == "nullcore"
                                                  else None)
            pb = tab() if (kind >= 0 and t[-1] != "no b") or t[-1] == "extra b" else None
            xa, xb, xm = _arr(ar), _arr(br), _arr(modes)
            keep += [pa, pb, xa, xb, xm]
            recs.append(Term(kind, tr, coef, _addr(pa), _addr(xa), _addr(pb), _addr(xb), _addr(xm)))
        return (Term * max(len(recs), 1))(*recs), keep

    def __call__(self, inner, terms, sums=None, bound=None, d=None, n=None, null_terms=False):
        d = len(inner) if d is None else d
        arr, keep = self.records(d, terms)
        return self.lib.ttk_affine_round_one_lds(d, _arr(inner), len(terms) if n is None else n,
                                                 None if null_terms else arr, sums, bound)


def _plan_terms(cid, trains):
    """the case's terms for `Plan`"""
    out = []
    for k, a, b, c, tr in zip(AC.kinds(cid), AC.ia(cid), AC.ib(cid), AC.coeffs(cid), AC.transposed(cid)):
        if k < 0:
            out.append((-1, AC.train_ranks(trains[a]), None, None, c, int(tr)))
        else:
            out.append((k, AC.train_ranks(trains[a]), AC.train_ranks(trains[b]), PC.modes(k, trains[a], trains[b]),
                        c, int(tr)))
    return out


@needs_lib
def test_plan_is_the_round_one_plan_of_the_summed_ranks(T):
    """every fitting case fits; `sum_ranks` are the sums of the term ranks (a product's: the products), `bound` the
    retraction's rule with no upper bound on them, the bytes those of `ttk_round_one_lds` at the summed ranks;
    both outputs may be NULL; j does not fit"""
    plan = Plan()
    for cid in AC.VALUE:
        trains = AC.stored(cid)
        inner, rk = AC.inner_and_ranks(cid, trains)
        d = len(inner)
        terms = _plan_terms(cid, trains)
        sums, bound = (I64 * (d + 1))(), (I64 * (d + 1))()
        got = plan(inner, terms, sums, bound)
        if cid == "j":
            assert rk == [1, 258, 258, 1]
            assert got == -1 and plan(inner, terms) == -1
            continue
        assert 0 <= got <= 160 * 1024, (cid, got)
        assert list(sums) == rk, cid
        assert list(bound) == T.retraction_ranks(inner, rk, [AC.BIG] * (d - 1)), cid
        assert all(q <= bd for q, bd in zip(AC.qranks(cid), bound)), cid
        assert got == plan.lib.ttk_round_one_lds(d, _arr(inner), _arr(rk), None), cid
        assert got == plan(inner, terms) == plan(inner, terms, sums, None) == plan(inner, terms, None, bound), cid


class _SumTerm(ctypes.Structure):
    """`ttk_sum_term` (include/ttk.h)"""
    _fields_ = [("cores", VP), ("ranks", VP), ("coef", ctypes.c_double), ("transpose", ctypes.c_int)]


@needs_lib
def test_plan_of_plain_terms_is_the_sum_plan_and_of_one_product_the_product_plan():
    plan = Plan()
    seen = 0
    for cid in SC.FIT:
        trains = SC.terms(cid, SC.stored(cid))
        if len(trains) > 4:
            continue
        inner, rk = SC.sum_inner_and_ranks(cid, SC.stored(cid))
        d = len(inner)
        rks = [_arr(SC.term_ranks(t)) for t in trains]
        tab = (VP * d)(*[ctypes.addressof(ONE)] * d)
        st = (_SumTerm * len(trains))(*[_SumTerm(_addr(tab), _addr(r), 1.0, 0) for r in rks])
        want_s, want_b = (I64 * (d + 1))(), (I64 * (d + 1))()
        want = plan.lib.ttk_sum_round_one_lds(d, _arr(inner), len(trains), st, want_s, want_b)
        sums, bound = (I64 * (d + 1))(), (I64 * (d + 1))()
        got = plan(inner, [(-1, SC.term_ranks(t), None, None) for t in trains], sums, bound)
        assert got == want >= 0 and list(sums) == list(want_s) == rk and list(bound) == list(want_b), cid
        seen += 1
    assert seen >= 4
    for cid in PC.FIT:
        a, b = PC.factors(cid)
        k = PC.kind(cid)
        inner, rk = PC.prod_inner_and_ranks(k, a, b)
        d = len(inner)
        args = (_arr(PC.train_ranks(a)), _arr(PC.train_ranks(b)), _arr(PC.modes(k, a, b)))
        want_s, want_b = (I64 * (d + 1))(), (I64 * (d + 1))()
        want = plan.lib.ttk_prod_round_one_lds(k, d, *args, want_s, want_b)
        sums, bound = (I64 * (d + 1))(), (I64 * (d + 1))()
        got = plan(inner, [(k, PC.train_ranks(a), PC.train_ranks(b), PC.modes(k, a, b))], sums, bound)
        assert got == want >= 0 and list(sums) == list(want_s) == rk and list(bound) == list(want_b), cid


@needs_lib
def test_plan_rejects_invalid_arguments():
    """every argument, every position; all of these are 'does not fit or invalid' for the plan call (-1), and
    TTK_ERR_ARG without a launch for the device call (tests/test_gpu_affine_round.py)"""
    plan = Plan()
    inner = [3, 3, 3]
    ra, rb, rp = [1, 2, 3, 1], [1, 3, 2, 1], [1, 2, 2, 1]
    mv = [3, 2, 1] * 3                                   # kind 0: (m, n) = (3, 2), the result's middle extent 3
    prod, plain = (0, ra, rb, mv), (-1, rp, None, None)
    assert plan(inner, [prod, plain]) >= 0 and plan(inner, [plain, prod]) >= 0 and plan(inner, [plain]) >= 0
    assert plan(inner, [prod, prod, plain, plain]) >= 0                        # the limits themselves
    assert plan(inner, [(1, ra, rb, [3, 2, 1] * 3)]) >= 0                      # kind 1: m n = 3 x 1
    assert plan(inner, [(2, ra, rb, [3, 9, 9] * 3)]) >= 0 and plan(inner, [(3, ra, rb, [3, 1, 9] * 3)]) >= 0
    for k in (-2, 4, 7):
        assert plan(inner, [(k, ra, rb, mv), plain]) == -1                     # kind outside -1 .. 3
    assert plan(inner, [prod, prod, prod]) == -1                               # three product terms
    assert plan(inner, [prod, prod, prod, plain]) == -1
    assert plan(inner, [plain] * 5) == -1 and plan(inner, [prod] + [plain] * 4) == -1   # five terms
    assert plan(inner, [plain], n=0) == -1 and plan(inner, [plain], n=-1) == -1
    assert plan(inner, [plain], null_terms=True) == -1
    assert plan(inner[:1], [(-1, [1, 1], None, None)]) == -1                   # d = 1
    assert plan(inner, [plain], d=0) == -1 and plan(inner, [plain], d=-2) == -1
    assert plan.lib.ttk_affine_round_one_lds(3, None, 1, plan.records(3, [plain])[0], None, None) == -1  # no inner
    for at in range(3):                                                        # an extent below 1
        bad = list(inner)
        bad[at] = 0
        assert plan(bad, [plain]) == -1, at
    # a mid mismatch, every kind and every core: the product's middle extent is not inner[k]
    for k, m in ((0, [3, 2, 1]), (1, [3, 2, 1]), (2, [3, 1, 1]), (3, [3, 1, 1])):
        assert plan(inner, [(k, ra, rb, m * 3), plain]) >= 0
        for at in range(3):
            bad = m * 3
            bad[3 * at] = 2
            assert plan(inner, [(k, ra, rb, bad), plain]) == -1, (k, at)
    assert plan(inner, [(1, ra, rb, [3, 2, 2] * 3)]) == -1 and plan([6] * 3, [(1, ra, rb, [3, 2, 2] * 3)]) >= 0
    assert plan(inner, [(3, ra, rb, [3, 2, 1] * 3)]) == -1 and plan([6] * 3, [(3, ra, rb, [3, 2, 1] * 3)]) >= 0
    for at in range(6):                                                        # an extent a kind uses, below 1
        bad = list(mv)
        bad[3 * (at // 2) + at % 2] = 0
        assert plan(inner, [(0, ra, rb, bad)]) == -1, at
    # b, b_ranks and modes null exactly for plain terms
    assert plan(inner, [(-1, rp, rb, None)]) == -1 and plan(inner, [(-1, rp, None, mv)]) == -1
    assert plan(inner, [(-1, rp, None, None, 1.0, 0, "extra b")]) == -1
    assert plan(inner, [(0, ra, None, mv)]) == -1 and plan(inner, [(0, ra, rb, None)]) == -1
    assert plan(inner, [(0, ra, rb, mv, 1.0, 0, "no b")]) == -1
    assert plan(inner, [(0, None, rb, mv)]) == -1 and plan(inner, [(-1, None, None, None)]) == -1
    assert plan(inner, [(-1, rp, None, None, 1.0, 0, "no a")]) == -1
    for at in range(3):                                                        # a null core, every position
        assert plan(inner, [(-1, rp, None, None, 1.0, 0, ("nullcore", at))]) == -1, at
    for rk in ([1, 0, 3, 1], [1, 2, -1, 1], [2, 2, 3, 1], [1, 2, 3, 2]):       # a rank below 1, boundary ranks
        assert plan(inner, [(-1, rk, None, None)]) == -1
        assert plan(inner, [(0, rk, rb, mv)]) == -1 and plan(inner, [(0, ra, rk, mv)]) == -1
        assert plan(inner, [plain, (-1, rk, None, None)]) == -1                # in a later term too
    for c in (float("nan"), float("inf"), -float("inf")):                     # coef finite
        assert plan(inner, [(-1, rp, None, None, c, 0)]) == -1
    for tr in (-1, 2):                                                         # transpose 0 or 1
        assert plan(inner, [(-1, rp, None, None, 1.0, tr)]) == -1
    assert plan([4] * 33, [(-1, [1] + [2] * 32 + [1], None, None)]) == -1      # more than 32 cores
    assert plan([4] * 32, [(-1, [1] + [2] * 31 + [1], None, None)]) >= 0
    assert plan(inner[:2], [(-1, [1, 1 << 40, 1], None, None)]) == -1          # a rank above the LDS capacity
    assert plan(inner[:2], [(0, [1, 200, 1], [1, 200, 1], mv[:6])]) == -1      # product rank 40000
    assert plan(inner[:2], [(0, [1, 1 << 33, 1], [1, 1 << 33, 1], mv[:6])]) == -1
    assert plan([16] * 3, [(-1, [1, 300, 300, 1], None, None)]) == -1          # a 1.4 MB core


def _check_public(T, cid, with_norm2=False):
    host = AC.stored(cid)
    dev = [T.to_device(t) for t in host]
    keep = [list(t) for t in dev]
    np.random.seed(7)
    st0 = np.random.get_state()
    res = AC.public(T, cid, dev, with_norm2)
    st1 = np.random.get_state()
    assert st0[0] == st1[0] and np.array_equal(st0[1], st1[1]) and st0[2:] == st1[2:]
    if with_norm2:
        res, n2 = res
        want = float(np.sum(AC.dense(T.to_host(res)) ** 2))
        assert abs(float(n2) - want) <= AC.RTOL * want, (cid, float(n2), want)
    AC.check_result(cid, AC.finish(T, cid, res))
    for t, k, h in zip(dev, keep, host):
        assert len(t) == len(k) and all(x is y for x, y in zip(t, k))
        assert all(np.array_equal(T.D.read(x), y) for x, y in zip(t, h))


@pytest.mark.parametrize("switch", (False, True))
@pytest.mark.parametrize("cid", AC.VALUE)
def test_public_function_matches_reference(T, monkeypatch, cid, switch):
    """ranks exactly the reference's and the dense tensor to 1e-11, switch off and on (without a GPU both take the
    composed path); the caller's tensors and lists are unchanged, and nothing is drawn from NumPy's stream"""
    monkeypatch.setattr(T, "AFFINE_ROUND_ONE", switch)
    _check_public(T, cid)


@pytest.mark.parametrize("cid", AC.FIT)
def test_public_function_returns_the_squared_norm(T, cid):
    """with_norm2: ||result||^2 to 1e-11 relative of the dense tensor's"""
    _check_public(T, cid, True)


def test_cases_cover_every_term_kind_and_both_orders():
    assert {k for c in AC.FIT for k in AC.kinds(c)} >= {-1, 0, 1, 3}
    assert AC.kinds("r")[0] >= 0 > AC.kinds("f")[0]
    assert sum(k >= 0 for k in AC.kinds("y")) == 2 and sum(AC.transposed("y")) == 2 and len(AC.kinds("y")) == 4
    assert any(c != float(np.float32(c)) or c not in (1.0, -1.0, 0.5, -0.5) for c in AC.coeffs("m"))


@pytest.mark.parametrize("cid", AC.FIT)
def test_materialised_operand_is_the_composed_operand(T, cid):
    """the test-side NumPy operand (what the GPU test feeds `ttk_round_one` for the bit comparison) has the composed
    path's layout and, to rounding, its numbers; the composed path builds the products unrounded"""
    host = AC.stored(cid)
    dev = [T.to_device(t) for t in host]
    terms, mids = T._affine_norm(AC.terms(cid, dev), AC.mids(cid))
    got = T.to_host(T._affine_composed(terms, mids))
    want = AC.materialised(cid, host)
    inner, rk = AC.inner_and_ranks(cid, host)
    assert len(got) == len(want)
    for g, w, n, r0, r1 in zip(got, want, inner, rk[:-1], rk[1:]):
        assert w.shape == (r0, n, r1) and g.size == w.size and g.shape[0] == r0 and g.shape[-1] == r1
        g = g.reshape(w.shape)
        assert np.max(np.abs(g - w)) <= 1e-14 * np.max(np.abs(w))
        assert np.array_equal(g == 0.0, w == 0.0)


def test_switch_is_off_by_default_and_not_taken_off_the_gpu(T, monkeypatch):
    """the switch reads TTIPM_AFFINE_ROUND_ONE; switched on without a GPU, `_affine_native` declines"""
    assert T.AFFINE_ROUND_ONE is (os.environ.get("TTIPM_AFFINE_ROUND_ONE", "0") == "1")
    monkeypatch.setattr(T, "AFFINE_ROUND_ONE", True)
    dev = [T.to_device(t) for t in AC.stored("r")]
    assert T._affine_native(AC.terms("r", dev), AC.eps("r"), 0, AC.mids("r")) is None


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


@pytest.mark.parametrize("switch", (False, True))
@pytest.mark.parametrize("name", ("primal", "dual", "dual_active", "y", "mx"))
def test_ipm_helpers_make_the_old_library_calls(T, monkeypatch, name, switch):
    """without the native path (switch off; on the CPU also switch on) a rewired site is the expression it
    replaced: the same library calls with the same scalars in the same order, the same bits out, the same MT19937
    state"""
    from ttipm_amd import tt_ipm
    monkeypatch.setattr(T, "AFFINE_ROUND_ONE", switch)
    st, v = AC.ipm_state(T, tt_ipm, active=name == "dual_active")
    rec = Recorder(T.D.lib)
    monkeypatch.setattr(T.D, "lib", rec)
    runs = []
    for f in (AC.old_ipm_expressions(T, tt_ipm)[name], AC.new_ipm_helpers(tt_ipm)[name]):
        np.random.seed(11)
        del rec.calls[:]
        res = T.to_host(f(st, v))
        runs.append((list(rec.calls), res, np.random.get_state()))
    (c0, r0, s0), (c1, r1, s1) = runs
    assert len(c0) > 3 and c0 == c1
    assert len(r0) == len(r1) and all(np.array_equal(a, b) for a, b in zip(r0, r1))
    assert np.array_equal(s0[1], s1[1]) and s0[2:] == s1[2:]
    np.random.seed(11)
    fresh = np.random.get_state()
    assert not (np.array_equal(fresh[1], s1[1]) and fresh[2] == s1[2])  # every site goes through `tt_scale`


def test_newton_system_reads_the_norms_it_is_not_handed(T, monkeypatch):
    """`tt_infeasible_newton_system` leaves a residual's inner product out of its `tt_scalars` call exactly where
    the fused rounding handed its squared norm on, and then takes the norm from that"""
    from ttipm_amd import tt_ipm
    st, v = AC.ipm_state(T, tt_ipm)
    pf, df = v["b"], v["C"]
    want = [T.tt_inner_prod(pf, pf), T.tt_inner_prod(df, df)]
    for handed in ((None, None), (7.0, None), (None, 5.0), (7.0, 5.0)):
        seen = []
        monkeypatch.setattr(tt_ipm, "_primal_feasibility", lambda *a, h=handed: (pf, h[0]))
        monkeypatch.setattr(tt_ipm, "_dual_feasibility", lambda *a, h=handed: (df, h[1]))
        scal = T.tt_scalars
        monkeypatch.setattr(T, "tt_scalars", lambda specs: (seen.append([s[1] for s in specs]), scal(specs))[1])
        monkeypatch.setattr(T, "tt_psd_rank_reduce", lambda tt, eps=0: tt)
        s = tt_ipm.IPMStatus(3, 1e-3, 1e-3, 1e-5, 1e-12, False, False, np.inf, False, np.inf, True, np.inf, np.inf,
                             False, tt_ipm.IneqStatus.NOT_IN_USE, False, 3.0, 2.5, 1000)
        lhs = {}
        _, rhs, s = tt_ipm.tt_infeasible_newton_system(lhs, v["C"], v["X"], v["Y"], v["Z"], None, v["L"], v["Ladj"],
                                                       v["b"], None, s)
        monkeypatch.setattr(T, "tt_scalars", scal)
        kept = [t for t, h in zip((pf, df), handed) if h is None]
        assert len(seen) == (1 if kept else 0) and all(a is b for a, b in zip(seen[0] if seen else [], kept))
        npf = np.sqrt(handed[0] if handed[0] is not None else want[0])
        ndf = np.sqrt(handed[1] if handed[1] is not None else want[1])
        assert abs(float(s.primal_error) * 3.0 - npf) <= 1e-12 * npf
        assert abs(float(s.dual_error) * 2.5 - ndf) <= 1e-12 * ndf
        assert rhs._norms[0][0] is pf and rhs._norms[1][0] is df
