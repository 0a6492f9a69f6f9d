"""Rounding a product of two trains on the MI355X without building it: the one-launch `ttk_prod_round_one`
(csrc/ttk_retract.hip, the product cores formed in the kernel's two loads) against the reference's outputs
(tests/golden/prod_round.npz), against the composed path (`ttk_zipup`), bit for bit against `ttk_round_one` on
the materialised product, and its launch, host-wait, determinism, fallback and validation contracts.  Off by
default (TTIPM_PROD_ROUND_ONE); the tests switch it on by monkeypatch.  The same value checks on the CPU:
tests/test_host_prod_round.py."""
import ctypes

import numpy as np
import pytest

from tests import prod_round_cases as PC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def T():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from ttipm_amd import tt_ops
    assert hasattr(tt_ops.D.lib, "ttk_prod_round_one")
    return tt_ops


@pytest.fixture
def on(T, monkeypatch):
    monkeypatch.setattr(T, "PROD_ROUND_ONE", True)
    return T


def _up(T, cid, host=None):
    """(host factors, device factors); the case takes the one-launch path and its uploads are done"""
    host = PC.factors(cid) if host is None else host
    a, b = PC.upload(T, cid, host)
    assert T.prod_round_one_lds(PC.kind(cid), a, b) >= 0
    T.D.read(a[0])
    T.D.read(b[0])
    return host, (a, b)


@pytest.mark.parametrize("cid", PC.FIT)
def test_fused_matches_reference(on, cid):
    T = on
    host, (a, b) = _up(T, cid)
    keep = (list(a), list(b))
    s0 = T.D.lib.ttk_sync_count()
    res = PC.public(T, cid, a, b)
    assert T.D.lib.ttk_sync_count() - s0 == 1  # the one-launch path ran: one read, of the ranks
    PC.check_result(cid, PC.finish(T, cid, res))
    for t, k, h in zip((a, b), keep, host):  # the caller's lists and tensors are never written
        assert len(t) == len(k) and all(x is y for x, y in zip(t, k))
        assert all(np.array_equal(T.D.read(x), y) for x, y in zip(t, h))
    T.D.check_handoffs()


@pytest.mark.parametrize("cid", PC.FIT)
def test_fused_matches_composed_path(T, cid, monkeypatch):
    _, (a, b) = _up(T, cid)
    monkeypatch.setattr(T, "PROD_ROUND_ONE", True)
    new = PC.finish(T, cid, PC.public(T, cid, a, b))
    monkeypatch.setattr(T, "PROD_ROUND_ONE", False)
    old = PC.finish(T, cid, PC.public(T, cid, a, b))
    assert [c.shape for c in new] == [c.shape for c in old]
    err = float(np.max(np.abs(PC.dense(new) - PC.dense(old)))) / PC.scale(cid)
    assert err <= 1e-11, err
    PC.check_result(cid, old)
    T.D.check_handoffs()


def _abi_call(T, kind, a, b, eps, mode, info=None):
    """`ttk_prod_round_one` itself: (status, out buffers, info, d, inner, bound, (launches, waits), keep); info: the
    caller's own buffer"""
    D = T.D
    plan = T._prod_round_one_plan(kind, a, b)
    (kind, d, pa, ar, pb, br, modes), prod, bound, keep = plan
    inner = [int(np.prod(m)) for m in T._prod_out_modes(kind, a, b)]
    outs = T._packed_flat(bound, inner)
    info = D.empty(d + 2) if info is None else info
    P = ctypes.c_void_p * d
    D._stream()
    D.read(info)  # the allocations are done
    l0, s0 = D.lib.ttk_launch_count(), D.lib.ttk_sync_count()
    rc = D.lib.ttk_prod_round_one(D.ctx(), kind, d, pa, ar, pb, br, modes, float(eps), mode,
                                  P(*[o.data_ptr() for o in outs]), info.data_ptr())
    counts = (D.lib.ttk_launch_count() - l0, D.lib.ttk_sync_count() - s0)
    return rc, outs, info, d, inner, bound, counts, keep


@pytest.mark.parametrize("cid", ("c", "v", "g", "h", "q", "x", "k", "p", "e", "l"))
def test_abi_call_is_one_launch_and_no_wait(T, cid):
    """the call alone: one launch, nothing read; `info` then holds the reference's rounded ranks and, in mode 1,
    a tail whose 1/(2d)-th power is the reference's factor"""
    _, (a, b) = _up(T, cid)
    rc, outs, info, d, inner, bound, counts, _ = _abi_call(T, PC.kind(cid), a, b, PC.eps(cid), PC.mode(cid))
    assert rc == 0 and counts == (1, 0)
    got = T.D.read(info)
    assert [float(v) for v in got[:d + 1]] == [float(q) for q in PC.qranks(cid)]
    if PC.mode(cid) == 0:
        assert got[d + 1] == 0.0
    else:
        assert abs(got[d + 1] ** (1.0 / (2 * d)) - PC.factor(cid)) <= 1e-11 * PC.factor(cid)
    T.D.check_handoffs()


SENTINEL = 0x4242424242424242  # a finite double (about 1.6e11) that no case's figures come near


@pytest.mark.parametrize("mode", (0, 1))
def test_info_is_d_plus_2_words_and_the_word_after_them_is_not_written(T, mode):
    """`info` is d + 2 doubles: given d + 3 with the last preset, the call leaves that word's bits as they are and
    writes info[0 .. d+1] with the bits it writes into a d + 2 buffer (case v, d = 3: matrix x vector)"""
    _, (a, b) = _up(T, "v")
    rc, _, info, d, _, _, _, _ = _abi_call(T, PC.kind("v"), a, b, PC.eps("v"), mode)
    assert rc == 0 and d == 3
    want = T.D.read(info)
    preset = np.full(d + 3, -1.0)
    preset[d + 2:].view(np.int64)[0] = SENTINEL
    rc, _, wide, _, _, _, _, _ = _abi_call(T, PC.kind("v"), a, b, PC.eps("v"), mode, T.D.from_numpy(preset))
    assert rc == 0
    got = T.D.read(wide)
    assert want.shape == (d + 2,) and got.shape == (d + 3,)
    assert int(got.view(np.int64)[d + 2]) == SENTINEL
    assert np.array_equal(got[:d + 2].view(np.int64), want.view(np.int64))
    assert not np.any(got[:d + 2] == -1.0)  # every word before it was written: ranks >= 1, a tail >= 0
    T.D.check_handoffs()


def _fronts(T, outs, info, inner):
    got = T.D.read(info)
    q = [int(v) for v in got[:-1]]
    return [T.D.read(o[:q[k] * inner[k] * q[k + 1]]) for k, o in enumerate(outs)] + [got]


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
    return _fronts(T, outs, info, inner), list(bound)


def _same_bits(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert x.shape == y.shape and np.array_equal(x.view(np.int64), y.view(np.int64))


def _check_bits_against_materialised(T, cid, host, eps, mode):
    k = PC.kind(cid)
    _, (a, b) = _up(T, cid, host)
    built = [T.D.contig(c) for c in T.to_device(PC.materialised(k, *host))]
    want, wbound = _round_one_bits(T, built, eps, mode)
    rc, outs, info, d, inner, bound, _, _ = _abi_call(T, k, a, b, eps, mode)
    assert rc == 0 and bound == wbound
    got = _fronts(T, outs, info, inner)
    _same_bits(got, want)
    T.D.check_handoffs()
    return got


@pytest.mark.parametrize("cid", ("h", "q", "x", "k"))
def test_hadamard_is_round_one_on_the_materialised_product_bit_for_bit(T, cid):
    """a Hadamard element is one IEEE multiply in the kernel and in NumPy, so `ttk_round_one` on the uploaded
    NumPy product gives the same bits: out and info"""
    got = _check_bits_against_materialised(T, cid, PC.factors(cid), PC.eps(cid), PC.mode(cid))
    assert [int(v) for v in got[-1][:-1]] == PC.qranks(cid)


@pytest.mark.parametrize("cid", ("v", "g", "e"))
def test_contraction_is_round_one_on_the_materialised_product_bit_for_bit(T, cid):
    """kinds 0 and 1 on integer factors: every product and partial sum of a product core is an exact integer, so
    the materialised core does not depend on the order of summation and the bits must agree.  eps: 1e-2 of the
    product's norm, so the rounding has something to decide."""
    host = PC.integer_factors(cid, 20261203)
    prod = PC.materialised(PC.kind(cid), *host)
    assert all(np.array_equal(c, np.rint(c)) and np.max(np.abs(c)) < 2.0 ** 52 for c in prod)
    eps = 1e-2 * float(np.linalg.norm(PC.dense(prod)))
    _check_bits_against_materialised(T, cid, host, eps, 0)


@pytest.mark.parametrize("cid", ("v", "x"))
def test_two_calls_same_bits(on, cid):
    import torch
    T = on
    _, (a, b) = _up(T, cid)
    r1 = PC.public(T, cid, a, b)
    r2 = PC.public(T, cid, a, b)
    assert [x.shape for x in r1] == [y.shape for y in r2]
    assert all(torch.equal(x, y) for x, y in zip(r1, r2))
    T.D.check_handoffs()


def test_large_product_takes_the_composed_path(on):
    T = on
    a, b = PC.upload(T, "j")
    assert T.prod_round_one_lds(PC.kind("j"), a, b) == -1
    T.D.read(a[0])
    T.D.read(b[0])
    l0 = T.D.lib.ttk_launch_count()
    res = PC.public(T, "j", a, b)
    assert T.D.lib.ttk_launch_count() - l0 > 2
    PC.check_result("j", PC.finish(T, "j", res))
    T.D.check_handoffs()


def test_validation_returns_an_error_without_launching(T):
    """every rejected argument: TTK_ERR_ARG from the host-side checks, the message names the function, no launch;
    the valid call on the same buffers still runs afterwards"""
    from ttipm_amd._lib import TTK_ERR_ARG
    D = T.D
    _, (a, b) = _up(T, "g")   # matmat, d = 3: a (ra,2,3,Ra), b (rb,3,2,Rb), ranks [2,3] / [3,2]
    d = 3
    P, I64 = ctypes.c_void_p * d, ctypes.c_int64
    arr = lambda v: (I64 * len(v))(*v)  # noqa: E731
    ptr = lambda ts: P(*[t.data_ptr() if t is not None else None for t in ts])  # noqa: E731
    ra, rb, modes = arr(PC.train_ranks(a)), arr(PC.train_ranks(b)), arr(PC.modes(1, a, b))
    pa, pb = ptr(a), ptr(b)
    out = [D.empty(256) for _ in range(d)]   # the largest bound core is 4 x 4 x 4
    po = ptr(out)
    info = D.empty(d + 2)
    eps = PC.eps("g")
    D._stream()
    D.read(info)
    l0 = D.lib.ttk_launch_count()

    def bad(kind, dd, xa, xra, xb, xrb, xm, e, mode, outs, inf):
        assert D.lib.ttk_prod_round_one(D.ctx(), kind, dd, xa, xra, xb, xrb, xm, e, mode, outs, inf) == TTK_ERR_ARG
        assert b"ttk_prod_round_one" in D.lib.ttk_last_error()

    ok = (eps, 0, po, info.data_ptr())
    for kind in (-1, 4):
        bad(kind, d, pa, ra, pb, rb, modes, *ok)                                    # kind outside 0 .. 3
    bad(1, 1, pa, ra, pb, rb, modes, *ok)                                           # d = 1
    bad(1, d, None, ra, pb, rb, modes, *ok)                                         # no core table
    bad(1, d, pa, ra, None, rb, modes, *ok)
    bad(1, d, pa, None, pb, rb, modes, *ok)                                         # no rank array
    bad(1, d, pa, ra, pb, None, modes, *ok)
    bad(1, d, pa, ra, pb, rb, None, *ok)                                            # no modes
    bad(1, d, ptr([a[0], None, a[2]]), ra, pb, rb, modes, *ok)                      # a null core
    bad(1, d, pa, ra, ptr([b[0], b[1], None]), rb, modes, *ok)
    for rk in ([1, 0, 3, 1], [2, 2, 3, 1], [1, 2, 3, 2]):                           # zero rank, boundary ranks
        bad(1, d, pa, arr(rk), pb, rb, modes, *ok)
        bad(1, d, pa, ra, pb, arr(rk), modes, *ok)
    for at in range(3 * d):                                                         # an extent below 1
        m = PC.modes(1, a, b)
        m[at] = 0
        bad(1, d, pa, ra, pb, rb, arr(m), *ok)
    for e, mode in ((-1.0, 0), (float("nan"), 0), (float("inf"), 1), (eps, 2), (eps, -1)):
        bad(1, d, pa, ra, pb, rb, modes, e, mode, po, info.data_ptr())
    bad(1, d, pa, ra, pb, rb, modes, eps, 0, None, info.data_ptr())
    bad(1, d, pa, ra, pb, rb, modes, eps, 0, ptr([out[0], None, out[2]]), info.data_ptr())
    bad(1, d, pa, ra, pb, rb, modes, eps, 0, po, None)
    big = arr([1, 200, 200, 1])                                                     # product rank 40000: no fit
    bad(1, d, pa, big, pb, big, modes, *ok)
    assert D.lib.ttk_launch_count() == l0
    assert D.lib.ttk_prod_round_one(D.ctx(), 1, d, pa, ra, pb, rb, modes, *ok) == 0
    assert D.lib.ttk_launch_count() == l0 + 1
    assert [int(v) for v in D.read(info)[:d + 1]] == PC.qranks("g")
    D.check_handoffs()


@pytest.mark.parametrize("cid", ("v", "g", "h", "q"))
def test_switched_off_is_the_zipup_call(T, monkeypatch, cid):
    """with the switch off each public function is `_native_zipup` as before: the same bits and launch count"""
    import torch
    monkeypatch.setattr(T, "PROD_ROUND_ONE", False)
    assert T._use_native_zipup() and not T.ZIPUP
    _, (a, b) = _up(T, cid)
    k = PC.kind(cid)
    runs = []
    for f in (lambda: PC.public(T, cid, a, b),
              lambda: T._native_zipup(k, a, b, PC.eps(cid), T._prod_out_modes(k, a, b))):
        l0 = T.D.lib.ttk_launch_count()
        res = f()
        runs.append((res, T.D.lib.ttk_launch_count() - l0))
    (r0, n0), (r1, n1) = runs
    assert n0 == n1 > 2
    assert [x.shape for x in r0] == [y.shape for y in r1]
    assert all(torch.equal(x, y) for x, y in zip(r0, r1))
    T.D.check_handoffs()
