"""Rounding a weighted sum of trains and products of two trains on the MI355X without building it: the one-launch
`ttk_affine_round_one` (csrc/ttk_retract.hip, every term formed in the kernel's two loads) against the reference's
outputs (tests/golden/affine_round.npz), against the composed path, bit for bit against `ttk_sum_round_one`,
`ttk_prod_round_one` and `ttk_round_one` on the materialised operand, its squared norm `info[d + 2]`, and its launch,
host-wait, determinism, fallback and validation contracts.  Off by default (TTIPM_AFFINE_ROUND_ONE); the tests
switch it on by monkeypatch.  The same value checks on the CPU: tests/test_host_affine_round.py."""
import ctypes

import numpy as np
import pytest

from tests import affine_round_cases as AC
from tests import prod_round_cases as PC
from tests import sum_round_cases as SC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def T():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from ttipm_amd import tt_ops
    assert hasattr(tt_ops.D.lib, "ttk_affine_round_one")
    return tt_ops


@pytest.fixture
def on(T, monkeypatch):
    monkeypatch.setattr(T, "AFFINE_ROUND_ONE", True)
    return T


def _up(T, cid, host=None, fits=True):
    """(host trains, device trains); the uploads are done and, unless told otherwise, the case fits"""
    host = AC.stored(cid) if host is None else host
    dev = [T.to_device(t) for t in host]
    assert (T.affine_round_one_lds(AC.terms(cid, dev), AC.mids(cid)) >= 0) == fits
    for t in dev:
        T.D.read(t[0])
    return host, dev


@pytest.mark.parametrize("cid", AC.FIT)
def test_fused_matches_reference(on, cid):
    T = on
    host, dev = _up(T, cid)
    keep = [list(t) for t in dev]
    s0 = T.D.lib.ttk_sync_count()
    res = AC.public(T, cid, dev)
    assert T.D.lib.ttk_sync_count() - s0 == 1  # the one-launch path ran: one read, of the ranks and the norm
    AC.check_result(cid, AC.finish(T, cid, res))
    for t, k, h in zip(dev, keep, host):  # the caller's lists and tensors are never written
        assert len(t) == len(k) and all(x is y for x, y in zip(t, k))
        assert all(np.array_equal(T.D.read(x), y) for x, y in zip(t, h))
    T.D.check_handoffs()


@pytest.mark.parametrize("cid", AC.FIT)
def test_fused_matches_composed_path(T, cid, monkeypatch):
    _, dev = _up(T, cid)
    monkeypatch.setattr(T, "AFFINE_ROUND_ONE", True)
    new, n2 = AC.public(T, cid, dev, True)
    want = float(np.linalg.norm(AC.dense(T.to_host(new))))
    assert abs(float(np.sqrt(n2)) - want) <= AC.RTOL * want  # with_norm2 hands on the kernel's figure
    new = AC.finish(T, cid, new)
    monkeypatch.setattr(T, "AFFINE_ROUND_ONE", False)
    old = AC.finish(T, cid, AC.public(T, cid, dev))
    assert [c.shape for c in new] == [c.shape for c in old]
    err = float(np.max(np.abs(AC.dense(new) - AC.dense(old)))) / AC.scale(cid)
    assert err <= 1e-11, err
    AC.check_result(cid, old)
    T.D.check_handoffs()


def _abi_call(T, terms, mids, eps, mode, info=None):
    """`ttk_affine_round_one` itself: (status, out buffers, info, d, inner, bound, (launches, waits), keep); info:
    the caller's own buffer"""
    D = T.D
    nt, mids = T._affine_norm(terms, mids)
    (d, inner, rows, n, arr), sums, bound, keep = T._affine_round_one_plan(nt, mids)
    outs = T._packed_flat(bound, list(inner))
    info = D.empty(d + 3) if info is None else info
    P = ctypes.c_void_p * d
    D._stream()
    D.read(info)  # the allocations are done
    l0, s0 = D.lib.ttk_launch_count(), D.lib.ttk_sync_count()
    rc = D.lib.ttk_affine_round_one(D.ctx(), d, inner, rows, n, arr, float(eps), mode,
                                    P(*[o.data_ptr() for o in outs]), info.data_ptr())
    counts = (D.lib.ttk_launch_count() - l0, D.lib.ttk_sync_count() - s0)
    return rc, outs, info, d, list(inner), bound, counts, keep


def _case_call(T, cid, dev):
    return _abi_call(T, AC.terms(cid, dev), AC.mids(cid), AC.eps(cid), AC.mode(cid))


@pytest.mark.parametrize("cid", AC.FIT)
def test_abi_call_is_one_launch_and_no_wait(T, cid):
    """the call alone: one launch, nothing read; `info` then holds the reference's rounded ranks and, in mode 1,
    a tail whose 1/(2d)-th power is the reference's factor"""
    _, dev = _up(T, cid)
    rc, outs, info, d, inner, bound, counts, _ = _case_call(T, cid, dev)
    assert rc == 0 and counts == (1, 0)
    got = T.D.read(info)
    assert [float(v) for v in got[:d + 1]] == [float(q) for q in AC.qranks(cid)]
    if AC.mode(cid) == 0:
        assert got[d + 1] == 0.0
    else:
        assert abs(got[d + 1] ** (1.0 / (2 * d)) - AC.factor(cid)) <= 1e-11 * AC.factor(cid)
    T.D.check_handoffs()


def _fronts(T, outs, info, inner):
    """the written front of every out buffer, then info[0 .. d+1] (what the four entry points share)"""
    d = len(inner)
    got = T.D.read(info)
    q = [int(v) for v in got[:d + 1]]
    return [T.D.read(o[:q[k] * inner[k] * q[k + 1]]) for k, o in enumerate(outs)] + [got[:d + 2]]


def _same_bits(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert x.shape == y.shape and np.array_equal(x.view(np.int64), y.view(np.int64))


SUM_BITS = tuple(c for c in SC.FIT if len(SC.which(c)) <= 4)


def test_sum_cases_for_the_bit_comparison_cover_weights_and_transposes():
    assert len(SUM_BITS) >= 6 and any(any(SC.transposed(c)) for c in SUM_BITS)
    assert any(any(w != 1.0 for w in SC.coeffs(c)) for c in SUM_BITS) and any(SC.mode(c) for c in SUM_BITS)


@pytest.mark.parametrize("cid", SUM_BITS)
def test_plain_terms_are_sum_round_one_bit_for_bit(T, cid):
    """plain terms only: the loader's element code is `ttk_sum_round_one`'s, so out and info[0 .. d+1] agree in
    every bit"""
    D = T.D
    dev = [T.to_device(t) for t in SC.stored(cid)]
    trains, coefs, trs = SC.terms(cid, dev), SC.coeffs(cid), SC.transposed(cid)
    mode = min(SC.mode(cid), 1)
    (d, inner, rows, n, st), sums, wbound, mids, keep = T._sum_round_one_plan(trains, coefs, trs)
    wouts, _ = T._packed_out(keep[0][0], wbound, inner)
    winfo = D.empty(d + 2)
    D._stream()
    assert D.lib.ttk_sum_round_one(D.ctx(), d, inner, rows, n, st, SC.eps(cid), mode,
                                   (ctypes.c_void_p * d)(*[o.data_ptr() for o in wouts]), winfo.data_ptr()) == 0
    want = _fronts(T, wouts, winfo, list(inner))
    rc, outs, info, d2, inner2, bound, _, _ = _abi_call(T, list(zip(coefs, trains, trs)), mids, SC.eps(cid), mode)
    assert rc == 0 and d2 == d and bound == wbound
    _same_bits(_fronts(T, outs, info, inner2), want)
    D.check_handoffs()


@pytest.mark.parametrize("cid", PC.FIT)
def test_one_product_term_is_prod_round_one_bit_for_bit(T, cid):
    """one product, weight 1.0, not transposed: the loader's element code is `ttk_prod_round_one`'s"""
    D = T.D
    a, b = PC.upload(T, cid)
    k = PC.kind(cid)
    (k, d, pa, ar, pb, br, modes), prod, wbound, keep = T._prod_round_one_plan(k, a, b)
    mids = T._prod_out_modes(k, a, b)
    inner = [int(np.prod(m)) for m in mids]
    wouts = T._packed_flat(wbound, inner)
    winfo = D.empty(d + 2)
    D._stream()
    assert D.lib.ttk_prod_round_one(D.ctx(), k, d, pa, ar, pb, br, modes, PC.eps(cid), PC.mode(cid),
                                    (ctypes.c_void_p * d)(*[o.data_ptr() for o in wouts]), winfo.data_ptr()) == 0
    want = _fronts(T, wouts, winfo, inner)
    rc, outs, info, d2, inner2, bound, _, _ = _abi_call(T, [(1.0, (k, a, b))], mids, PC.eps(cid), PC.mode(cid))
    assert rc == 0 and inner2 == inner and bound == wbound
    _same_bits(_fronts(T, outs, info, inner2), want)
    D.check_handoffs()


def _round_one_bits(T, tt, eps, mode):
    """`ttk_round_one` on the contiguous device train `tt`: (the written front of every out buffer, info)"""
    D = T.D
    d = len(tt)
    inner, ranks, bound = T._round_one_plan(tt)
    outs, _ = T._packed_out(tt, list(bound), inner)
    info = D.empty(d + 2)
    P = ctypes.c_void_p * d
    D._stream()
    rc = D.lib.ttk_round_one(D.ctx(), d, P(*[c.data_ptr() for c in tt]), inner, ranks, float(eps), mode,
                             P(*[o.data_ptr() for o in outs]), info.data_ptr())
    assert rc == 0
    return _fronts(T, outs, info, list(inner)), list(bound)


INT_WEIGHTS = {"r": [1.0, -1.0], "u": [1.0, -1.0, -1.0], "y": [0.5, -0.5, 0.5, -0.5], "g": [1.0, -0.5]}


@pytest.mark.parametrize("cid", ("r", "u", "y", "g"))
def test_mixed_terms_are_round_one_on_the_materialised_operand_bit_for_bit(T, cid):
    """integer factors (entries +-1 .. 3) and weights from {1, -1, +-0.5}: every element of the operand is exact
    whatever the order of summation, so `ttk_round_one` on the uploaded NumPy operand gives the same bits.  eps:
    1e-2 of the operand's norm, so the rounding has something to decide."""
    w = INT_WEIGHTS[cid]
    host = AC.integer_trains(cid, 20270104)
    op = AC.materialised(cid, host, w)
    assert all(np.array_equal(2 * c, np.rint(2 * c)) and np.max(np.abs(c)) < 2.0 ** 51 for c in op)
    eps = 1e-2 * float(np.linalg.norm(AC.dense(op)))
    _, dev = _up(T, cid, host)
    built = [T.D.contig(c) for c in T.to_device(op)]
    want, wbound = _round_one_bits(T, built, eps, 0)
    rc, outs, info, d, inner, bound, _, _ = _abi_call(T, AC.terms(cid, dev, w), AC.mids(cid), eps, 0)
    assert rc == 0 and bound == wbound
    got = _fronts(T, outs, info, inner)
    _same_bits(got, want)
    assert any(q < s for q, s in zip(got[-1][1:d], AC.inner_and_ranks(cid, host)[1][1:d]))  # something was cut
    T.D.check_handoffs()


@pytest.mark.parametrize("cid", AC.FIT)
def test_info_holds_the_squared_norm_of_the_output(T, cid):
    """info[d + 2] against NumPy on the kernel's own output cores: |sqrt(info[d+2]) - ||dense(out)||| <= 1e-11
    ||dense(out)||, and the same bits on a second call"""
    _, dev = _up(T, cid)
    runs = []
    for _ in range(2):
        rc, outs, info, d, inner, bound, _, _ = _case_call(T, cid, dev)
        assert rc == 0
        got = T.D.read(info)
        q = [int(v) for v in got[:d + 1]]
        cores = [T.D.read(o[:q[k] * inner[k] * q[k + 1]]).reshape(q[k], inner[k], q[k + 1])
                 for k, o in enumerate(outs)]
        runs.append((cores, got))
    (cores, got), (_, again) = runs
    assert got.shape == (d + 3,)
    want = float(np.linalg.norm(AC.dense(cores)))
    err = abs(float(np.sqrt(got[d + 2])) - want) / want
    print(f"info[d+2] case {cid}: relative error of the norm {err:.3g}")
    assert err <= AC.RTOL, (cid, err)
    assert np.array_equal(got.view(np.int64), again.view(np.int64))
    T.D.check_handoffs()


@pytest.mark.parametrize("mode", (0, 1))
def test_info_is_d_plus_3_words_and_the_last_is_overwritten(T, mode):
    """the opposite of the sum's and the product's d + 2: a preset info[d + 2] is replaced by the squared norm of the
    output, to the tolerance of the test above (case r, d = 3: a product and a plain term)"""
    _, dev = _up(T, "r")
    d = 3
    preset = np.full(d + 3, -1.0)
    preset[d + 2:].view(np.int64)[0] = 0x4242424242424242  # a finite double, about 1.6e11
    rc, outs, info, d2, inner, _, _, _ = _abi_call(T, AC.terms("r", dev), AC.mids("r"), AC.eps("r"), mode,
                                                   T.D.from_numpy(preset))
    assert rc == 0 and d2 == d
    got = T.D.read(info)
    q = [int(v) for v in got[:d + 1]]
    cores = [T.D.read(o[:q[k] * inner[k] * q[k + 1]]).reshape(q[k], inner[k], q[k + 1]) for k, o in enumerate(outs)]
    want = float(np.linalg.norm(AC.dense(cores)))
    assert int(got.view(np.int64)[d + 2]) != 0x4242424242424242 and not np.any(got == -1.0)
    assert abs(float(np.sqrt(got[d + 2])) - want) <= AC.RTOL * want
    T.D.check_handoffs()


@pytest.mark.parametrize("cid", ("y", "s"))
def test_two_calls_same_bits(on, cid):
    import torch
    T = on
    _, dev = _up(T, cid)
    r1, n1 = AC.public(T, cid, dev, True)
    r2, n2 = AC.public(T, cid, dev, True)
    assert [x.shape for x in r1] == [y.shape for y in r2]
    assert all(torch.equal(x, y) for x, y in zip(r1, r2))
    assert np.float64(n1).view(np.int64) == np.float64(n2).view(np.int64)
    T.D.check_handoffs()


def test_large_operand_takes_the_composed_path(on):
    T = on
    _, dev = _up(T, "j", fits=False)
    l0 = T.D.lib.ttk_launch_count()
    res = AC.public(T, "j", dev)
    assert T.D.lib.ttk_launch_count() - l0 > 2
    AC.check_result("j", AC.finish(T, "j", res))
    T.D.check_handoffs()


def test_validation_returns_an_error_without_launching(T):
    """every rejected argument: TTK_ERR_ARG from the host-side checks, the message names the function, no launch;
    the valid call on the same buffers still runs afterwards"""
    from ttipm_amd._lib import TTK_ERR_ARG, AffineTerm
    D = T.D
    _, (A, x, b) = _up(T, "r")   # d = 3: A (ra,3,2,Ra) x x (r,2,R) - b (rb,3,Rb)
    d = 3
    P, I64, vp = ctypes.c_void_p * d, ctypes.c_int64, ctypes.c_void_p
    arr = lambda v: (I64 * len(v))(*v)  # noqa: E731
    ptr = lambda ts: P(*[t.data_ptr() if t is not None else None for t in ts])  # noqa: E731
    cast = lambda v: None if v is None else ctypes.cast(v, vp)  # noqa: E731
    rA, rx, rb = arr(AC.train_ranks(A)), arr(AC.train_ranks(x)), arr(AC.train_ranks(b))
    modes = arr(PC.modes(0, A, x))
    pA, px, pb = ptr(A), ptr(x), ptr(b)
    inner, rows = arr([3, 3, 3]), arr([3, 3, 3])
    out = [D.empty(1024) for _ in range(d)]   # the largest bound core is far smaller
    po = ptr(out)
    info = D.empty(d + 3)
    eps = AC.eps("r")
    D._stream()
    D.read(info)
    l0 = D.lib.ttk_launch_count()
    keep = []

    def rec(kind, tr, coef, a, ar, bb, br, m):
        keep.append((a, ar, bb, br, m))
        return AffineTerm(kind, tr, coef, cast(a), cast(ar), cast(bb), cast(br), cast(m))

    prod = lambda **kw: rec(*[kw.get(k, v) for k, v in (("kind", 0), ("tr", 0), ("coef", 1.0), ("a", pA),  # noqa: E731
                                                        ("ar", rA), ("b", px), ("br", rx), ("m", modes))])
    plain = lambda **kw: rec(*[kw.get(k, v) for k, v in (("kind", -1), ("tr", 0), ("coef", -1.0), ("a", pb),  # noqa: E731
                                                         ("ar", rb), ("b", None), ("br", None), ("m", None))])

    def call(terms, dd=d, inn=inner, rw=None, e=eps, mode=0, outs=po, inf=info.data_ptr(), n=None):
        ts = (AffineTerm * max(len(terms), 1))(*terms) if terms is not None else None
        return D.lib.ttk_affine_round_one(D.ctx(), dd, inn, rw, len(terms) if n is None else n, ts, e, mode, outs, inf)

    def bad(*a, **kw):
        assert call(*a, **kw) == TTK_ERR_ARG
        assert b"ttk_affine_round_one" in D.lib.ttk_last_error()

    for kind in (-2, 4):
        bad([prod(kind=kind), plain()])                                   # kind outside -1 .. 3
    bad([prod(), plain()], dd=1)                                          # d = 1
    bad([prod(), plain()], inn=None)
    bad([prod(), plain()], inn=arr([3, 0, 3]))
    bad([plain()], n=0)
    bad(None, n=1)
    bad([prod(), prod(), prod()])                                         # three products
    bad([plain()] * 5)                                                    # five terms
    bad([prod(a=None), plain()])                                          # no core table / rank array
    bad([prod(ar=None), plain()])
    bad([prod(b=None), plain()])
    bad([prod(br=None), plain()])
    bad([prod(m=None), plain()])
    bad([prod(), plain(a=None)])
    bad([prod(), plain(ar=None)])
    bad([prod(), plain(b=px)])                                            # b, b_ranks, modes on a plain term
    bad([prod(), plain(br=rx)])
    bad([prod(), plain(m=modes)])
    bad([prod(a=ptr([A[0], None, A[2]])), plain()])                       # a null core
    bad([prod(b=ptr([x[0], x[1], None])), plain()])
    bad([prod(), plain(a=ptr([None, b[1], b[2]]))])
    for rk in ([1, 0, 3, 1], [2, 2, 3, 1], [1, 2, 3, 2]):                 # zero rank, boundary ranks
        bad([prod(ar=arr(rk)), plain()])
        bad([prod(br=arr(rk)), plain()])
        bad([prod(), plain(ar=arr(rk))])
    for at in range(d):                                                   # a mid mismatch, an extent below 1
        m = PC.modes(0, A, x)
        m[3 * at] = 2
        bad([prod(m=arr(m)), plain()])
        m[3 * at] = 0
        bad([prod(m=arr(m)), plain()])
    for c in (float("nan"), float("inf")):
        bad([prod(coef=c), plain()])
        bad([prod(), plain(coef=c)])
    bad([prod(tr=2), plain()], rw=rows)
    bad([prod(tr=1), plain()])                                            # a transposed term needs rows
    bad([prod(), plain(tr=1)])
    bad([prod(tr=1), plain()], rw=arr([3, 2, 3]))                         # rows[k] divides inner[k]
    bad([prod(), plain()], rw=arr([3, 0, 3]))
    for e, mode in ((-1.0, 0), (float("nan"), 0), (float("inf"), 1), (eps, 2), (eps, -1)):
        bad([prod(), plain()], e=e, mode=mode)
    bad([prod(), plain()], outs=None)
    bad([prod(), plain()], outs=ptr([out[0], None, out[2]]))
    bad([prod(), plain()], inf=None)
    big = arr([1, 200, 200, 1])                                           # product rank 40000: no fit
    bad([prod(ar=big, br=big), plain()])
    assert D.lib.ttk_launch_count() == l0
    assert call([prod(), plain()]) == 0
    assert D.lib.ttk_launch_count() == l0 + 1
    assert [int(v) for v in D.read(info)[:d + 1]] == AC.qranks("r")
    D.check_handoffs()


def test_switched_off_is_the_composed_expression(T, monkeypatch):
    """with the switch off the public function is products, `_sum_composed`, `tt_rank_reduce`: the same bits and
    launch count"""
    import torch
    monkeypatch.setattr(T, "AFFINE_ROUND_ONE", False)
    _, dev = _up(T, "u")
    A, x, z, c = dev
    runs = []
    for f in (lambda: AC.public(T, "u", dev),
              lambda: T.tt_rank_reduce(T._sum_composed([T.tt_fast_matrix_vec_mul(A, x, 0.0), z, c],
                                                       AC.coeffs("u"), [False] * 3), AC.eps("u"))):
        l0 = T.D.lib.ttk_launch_count()
        res = f()
        runs.append((res, T.D.lib.ttk_launch_count() - l0))
    (r0, n0), (r1, n1) = runs
    assert n0 == n1 > 2
    assert [a.shape for a in r0] == [b.shape for b in r1]
    assert all(torch.equal(a, b) for a, b in zip(r0, r1))
    T.D.check_handoffs()


# ------------------------------------------------------------------ the four rewired sites of tt_ipm.py
@pytest.fixture(scope="module")
def problem(T):
    """maxcut at the smallest configured size (dim 5, rank 1) and a generic state on it: (st, trains by name)"""
    import types
    from ttipm_amd import problems, tt_ipm
    np.random.seed(5)
    C, L, b, lag_y = problems.maxcut_create_problem(5, 1, verbose=False)
    C, L, b, P = (T.tt_rank_reduce(t, eps=1e-12) for t in (C, L, b, lag_y))
    rng = np.random.default_rng(20270106)
    d = len(C)

    def tt(mid):
        rk = [1] + [2] * (d - 1) + [1]
        return T.to_device([rng.standard_normal((rk[k], *mid, rk[k + 1])) / np.sqrt(2.0) for k in range(d)])
    v = {"C": C, "L": L, "Ladj": T.tt_transpose(L), "b": b, "P": P, "X": tt((2, 2)), "Z": tt((2, 2)), "Y": tt((4,)),
         "Tt": None, "mask": T.to_device([np.array([[1.0, 0.0], [1.0, 1.0]]).reshape(1, 2, 2, 1) for _ in range(d)])}
    st = types.SimpleNamespace(eta=1e-3, eps=1e-12, primal_error_normalisation=1 + T.tt_norm(b),
                               dual_error_normalisation=1 + T.tt_norm(C), ineq_boundary_val=0.01,
                               ineq_status=tt_ipm.IneqStatus.NOT_IN_USE)
    assert 0.01 * st.eta * min(st.primal_error_normalisation, st.dual_error_normalisation) >= 1e-5
    return st, v


def _thresholds(st):
    """per site: (the absolute thresholds of the roundings the default path performs, those of the fused path)"""
    e_p = 0.01 * st.eta * st.primal_error_normalisation
    e_df = 0.01 * st.eta * st.dual_error_normalisation
    e_d = 0.1 * st.eta * st.dual_error_normalisation
    return {"primal": ([st.eps, e_p, e_p], [e_p]),       # L vec(X) at eps and at e, the difference at e | once at e
            "dual": ([st.eps, st.eps, e_df], [e_df]),    # Ladj Y, Z + C, the difference | once
            "y": ([st.eps, e_d], [e_d]),                 # P Y, the symmetrised difference | once
            "mx": ([st.eps, st.eps], [st.eps])}          # mask o X, the sum | once


@pytest.mark.parametrize("name", ("primal", "dual", "y", "mx"))
def test_rewired_site_stays_within_the_rounding_thresholds(T, problem, monkeypatch, name):
    """Switch on against switch off.  The reference's rule bounds every rounding's Frobenius error by its eps, so
    the two results differ by at most the sum of the thresholds of both paths; 1 % on top for the 1e-12 roundings'
    own floating point (the thresholds that count are >= 1e-5; for mX, whose thresholds are all 1e-12, the
    project's relative tolerance of the tensor is added instead).  The MT19937 stream ends where it ended, one
    host wait is made, and the state's norm is the tensor's to 1e-11."""
    from ttipm_amd import tt_ipm
    st, v = problem
    f = AC.new_ipm_helpers(tt_ipm)[name]
    monkeypatch.setattr(T, "AFFINE_ROUND_ONE", False)
    np.random.seed(3)
    off = AC.dense(T.to_host(f(st, v)))
    s_off = np.random.get_state()
    monkeypatch.setattr(T, "AFFINE_ROUND_ONE", True)
    np.random.seed(3)
    w0 = T.D.lib.ttk_sync_count()
    res = f(st, v)
    assert T.D.lib.ttk_sync_count() - w0 == 1  # the fused path ran
    s_on = np.random.get_state()
    assert np.array_equal(s_off[1], s_on[1]) and s_off[2:] == s_on[2:]
    on = AC.dense(T.to_host(res))
    assert on.shape == off.shape
    a, b = _thresholds(st)[name]
    bound = 1.01 * (sum(a) + sum(b)) + (AC.RTOL * float(np.max(np.abs(off))) if name == "mx" else 0.0)
    err = float(np.linalg.norm(on - off))
    print(f"wiring {name}: |on - off|_F {err:.3g}, bound {bound:.3g}")
    assert err <= bound, (name, err, bound)
    if name in ("primal", "dual"):
        np.random.seed(3)
        g = tt_ipm._primal_feasibility if name == "primal" else tt_ipm._dual_feasibility
        tt, n2 = g(v["L"], v["b"], v["X"], st) if name == "primal" else g(v["C"], v["Ladj"], v["Z"], v["Y"], None, st)
        want = float(np.linalg.norm(AC.dense(T.to_host(tt))))
        assert n2 is not None and abs(T.norm_from_ip(n2) - want) <= AC.RTOL * want
    T.D.check_handoffs()


@pytest.mark.parametrize("name", ("primal", "dual", "y", "mx"))
def test_rewired_site_switched_off_is_the_old_expression(T, problem, monkeypatch, name):
    """with the switch off: the bits and the launch count of the expression the site replaced"""
    import torch
    from ttipm_amd import tt_ipm
    st, v = problem
    monkeypatch.setattr(T, "AFFINE_ROUND_ONE", False)
    runs = []
    for f in (AC.old_ipm_expressions(T, tt_ipm)[name], AC.new_ipm_helpers(tt_ipm)[name]):
        np.random.seed(3)
        l0 = T.D.lib.ttk_launch_count()
        res = f(st, v)
        runs.append((res, T.D.lib.ttk_launch_count() - l0, np.random.get_state()))
    (r0, n0, s0), (r1, n1, s1) = runs
    assert n0 == n1 > 2
    assert [a.shape for a in r0] == [b.shape for b in r1] and all(torch.equal(a, b) for a, b in zip(r0, r1))
    assert np.array_equal(s0[1], s1[1]) and s0[2:] == s1[2:]
    T.D.check_handoffs()
