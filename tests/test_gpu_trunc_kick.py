"""The tail of the two-site step-size local solve on the MI355X: the one-launch `ttk_trunc_kick`
(csrc/ttk_trunc_kick.hip) against the reference's outputs (tests/golden/trunc_kick.npz), and its launch,
determinism, zero-input, validation, fallback and random-stream contracts; then the step-size eigen-ALS and one
whole solve with the switch on.  The path is off by default (TTIPM_TRUNC_KICK); the tests switch it on by
monkeypatch.  The fallback's value checks on the CPU: tests/test_host_trunc_kick.py."""
import ctypes
import json
import os

import numpy as np
import pytest

from tests import step_cases as SC
from tests import trunc_kick_cases as KC

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def pkg():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from ttipm_amd import tt_eig, tt_ops
    assert hasattr(tt_ops.D.lib, "ttk_trunc_kick")
    return tt_eig, tt_ops


@pytest.fixture
def on(pkg, monkeypatch):
    monkeypatch.setattr(pkg[1].D, "TRUNC_KICK", True)
    return pkg


def _up(D, cid):
    """(M, G) on the device, uploads done: the launch counts below see the call alone"""
    ops = [D.from_numpy(KC.matrix(cid)), D.from_numpy(KC.block(cid))]
    D.read(ops[0])
    return ops


def _one(D, cid, ops=None, unit=1):
    """the one call on the case's operands: (s1, s2, info) on the host"""
    rev, a, b, max_rank, _, _ = KC.dims(cid)
    M, G = ops or _up(D, cid)
    s1buf, s2buf, info = D.trunc_kick(rev, M, G, KC.trunc_tol(cid), max_rank, unit)
    info = D.read(info)
    s1, s2, r, q = D.trunc_kick_views(s1buf, s2buf, info, a, b)
    assert (r, q) == (int(info[0]), int(info[1]))
    return D.read(s1), D.read(s2), info


_ONE = {}


def _once(D, cid):
    """the case's one call, made once for the value tests that share it (results are not modified)"""
    if cid not in _ONE:
        _ONE[cid] = _one(D, cid)
    return _ONE[cid]


@pytest.mark.parametrize("cid", KC.VALUE)
def test_one_call_matches_reference(pkg, cid):
    """r and q exactly, S to 1e-11 of S[0], s1 s2 to 1e-11, the orthonormal factor's Gram matrix and the
    concatenated matrix's distance from its range to 1e-12"""
    D = pkg[1].D
    s1, s2, info = _once(D, cid)
    rev, a, b, _, r, q = KC.dims(cid)
    S = KC.G[f"{cid}/S"]
    print(cid, "r", info[0], "q", info[1], "sweeps", info[2], "norm", info[3], "max |S - ref| / S[0]",
          float(np.max(np.abs(info[4:] - S)) / S[0]))
    assert info[0] == r and info[1] == q
    assert 0 < info[2] <= 30
    assert abs(info[3] - 1.0) <= 1e-14
    assert info[4:].shape == S.shape and np.max(np.abs(info[4:] - S)) <= KC.RTOL * S[0]
    KC.check_rank_and_product(cid, s1, s2)
    KC.check_orthonormal(cid, s1, s2)
    D.check_handoffs()


@pytest.mark.parametrize("cid", KC.VALUE)
def test_one_call_factors_match_reference_elementwise(pkg, cid):
    """s1 and s2 elementwise to 1e-11: neither depends on the signs of the singular vectors
    (tests/trunc_kick_cases.py), and the gauge of the QR / RQ is LAPACK's on both sides"""
    s1, s2, _ = _once(pkg[1].D, cid)
    for name, got in (("s1", s1), ("s2", s2)):
        ref = KC.G[f"{cid}/{name}"]
        print(cid, name, "max abs difference", float(np.max(np.abs(got - ref))), "of", float(np.max(np.abs(ref))))
    KC.check_factors(cid, s1, s2)


@pytest.mark.parametrize("cid", ("a", "c", "e", "f", "m", "k"))
def test_scaling_is_the_kernels_own(pkg, cid):
    """unit = 1 on 3 M gives what unit = 0 gives on M up to the rounding of the scaling: the same ranks, the
    product to 1e-11, and ||3 M||_F in info[3]"""
    D = pkg[1].D
    rev, a, b, max_rank, r, q = KC.dims(cid)
    M3 = D.from_numpy(3.0 * KC.matrix(cid))
    G = D.from_numpy(KC.block(cid))
    s1, s2, info = _one(D, cid, (M3, G), unit=1)
    assert abs(info[3] - 3.0) <= 1e-13 and (info[0], info[1]) == (r, q)
    KC.check_rank_and_product(cid, s1, s2)
    t1, t2, info0 = _one(D, cid, unit=0)
    assert (info0[0], info0[1]) == (r, q) and abs(info0[3] - 1.0) <= 1e-14
    KC.check_rank_and_product(cid, t1, t2)


@pytest.mark.parametrize("cid", ("a", "c", "e", "f", "k"))
def test_abi_call_is_one_launch_without_a_host_wait(pkg, cid):
    """the direct call with G on the device: one launch, no host wait, inputs unchanged, two calls the same bits"""
    D = pkg[1].D
    rev, a, b, max_rank, _, _ = KC.dims(cid)
    ops = _up(D, cid)
    host = [D.read(t) for t in ops]
    l0, y0 = D.lib.ttk_launch_count(), D.lib.ttk_sync_count()
    out = D.trunc_kick(rev, ops[0], ops[1], KC.trunc_tol(cid), max_rank, 1)
    assert D.lib.ttk_launch_count() - l0 == 1
    assert D.lib.ttk_sync_count() == y0
    first = [D.read(t) for t in out]
    q = int(first[2][1])
    again = [D.read(t) for t in D.trunc_kick(rev, ops[0], ops[1], KC.trunc_tol(cid), max_rank, 1)]
    assert np.array_equal(first[2], again[2])
    assert np.array_equal(first[0][:a * q], again[0][:a * q]) and np.array_equal(first[1][:q * b], again[1][:q * b])
    for t, h in zip(ops, host):
        assert np.array_equal(D.read(t), h)
    # `ttk_trunc_kick_read`: the same launch, its info read in the call -- one launch, one host wait, the same bits
    l0, y0 = D.lib.ttk_launch_count(), D.lib.ttk_sync_count()
    t1, t2, info = D.trunc_kick(rev, ops[0], ops[1], KC.trunc_tol(cid), max_rank, 1, read=True)
    assert D.lib.ttk_launch_count() - l0 == 1 and D.lib.ttk_sync_count() - y0 == 1
    assert isinstance(info, np.ndarray) and np.array_equal(info, first[2])
    assert np.array_equal(D.read(t1)[:a * q], first[0][:a * q]) and np.array_equal(D.read(t2)[:q * b], first[1][:q * b])


def test_info_may_point_into_a_larger_buffer(pkg):
    """`info_out`: a slice of a longer device buffer; the words around it stay as they were"""
    D = pkg[1].D
    rev, a, b, max_rank, r, q = KC.dims("a")
    M, G = _up(D, "a")
    buf = D.from_numpy(np.full(3 + 4 + min(a, b) + 2, -7.0))
    out = D.trunc_kick(rev, M, G, KC.trunc_tol("a"), max_rank, 1, info_out=buf[3:3 + 4 + min(a, b)])
    h = D.read(buf)
    assert np.all(h[:3] == -7.0) and np.all(h[-2:] == -7.0)
    assert np.array_equal(h[3:-2], _once(D, "a")[2]) and (h[3], h[4]) == (r, q)
    assert out[2].data_ptr() == buf[3:].data_ptr()


def test_zero_matrix_gives_a_finite_zero_product(pkg):
    D = pkg[1].D
    s1, s2, info = _one(D, "z")
    assert info[0] == 1 and info[1] == KC.dims("z")[5] and info[3] == 0.0 and not info[4:].any()
    assert np.all(np.isfinite(s1)) and np.all(np.isfinite(s2))
    assert not (s1 @ s2).any() and not s2.any()


def test_validation_returns_err_arg_without_launching(pkg):
    D = pkg[1].D
    from ttipm_amd import _lib as L
    M, G = _up(D, "a")
    s1, s2, info = D.empty(8 * 8), D.empty(8 * 8), D.empty(4 + 8)
    P = lambda t: None if t is None else t.data_ptr()  # noqa: E731

    def call(rev=0, a=8, b=8, r_add=4, unit=1, tol=1e-3, max_rank=32, ptrs=(M, G, s1, s2, info)):
        return D.lib.ttk_trunc_kick(D.ctx(), rev, a, b, r_add, unit, tol, max_rank, *[P(t) for t in ptrs])

    bad = [dict(rev=2), dict(rev=-1), dict(a=0), dict(b=0), dict(r_add=0), dict(max_rank=0), dict(a=-8),
           dict(tol=-1e-3), dict(tol=float("nan")), dict(tol=float("inf")),
           dict(a=512, b=64)]                                                # case j: does not fit
    bad += [dict(ptrs=tuple(None if i == k else t for i, t in enumerate((M, G, s1, s2, info)))) for k in range(5)]
    for kw in bad:
        l0 = D.lib.ttk_launch_count()
        assert call(**kw) == L.TTK_ERR_ARG, kw
        assert D.lib.ttk_launch_count() == l0, kw
        assert b"ttk_trunc_kick" in D.lib.ttk_last_error(), kw
    assert D.trunc_kick_qmax(*KC.lds_args("j")) is None
    l0, y0 = D.lib.ttk_launch_count(), D.lib.ttk_sync_count()
    for kw in (dict(a=0), dict(host=None), dict(a=512, b=64)):   # ttk_trunc_kick_read validates the same way
        args = dict(a=8, b=8, host=np.empty(12).ctypes.data_as(ctypes.c_void_p))
        args.update(kw)
        assert D.lib.ttk_trunc_kick_read(D.ctx(), 0, args["a"], args["b"], 4, 1, 1e-3, 32, P(M), P(G), P(s1), P(s2),
                                         args["host"]) == L.TTK_ERR_ARG, kw
        assert b"ttk_trunc_kick" in D.lib.ttk_last_error(), kw
    assert D.lib.ttk_launch_count() == l0 and D.lib.ttk_sync_count() == y0
    l0 = D.lib.ttk_launch_count()
    assert call(tol=KC.trunc_tol("a")) == L.TTK_OK and call(tol=0.0) == L.TTK_OK   # a zero threshold keeps all
    assert D.lib.ttk_launch_count() - l0 == 2
    assert tuple(D.read(info)[:2]) == (8, 8)


def _callers(E, T, cid, monkeypatch):
    """`_split` (every case) and the dense tail (cases with a dense pencil within reach: ev >= 0 and ev < 0)
    under the three settings: {setting: [(s1, s2, sign, launches, waits, state), ...]}"""
    D = T.D
    out = {}
    for name, sk, tk in (("default", False, False), ("split_kick", True, False), ("trunc_kick", False, True)):
        monkeypatch.setattr(D, "SPLIT_KICK", sk)
        monkeypatch.setattr(D, "TRUNC_KICK", tk)
        rows = []
        info = {}
        s1, s2 = KC.split(E, T, cid, info)
        rows.append((s1, s2, 1.0, info["launches"], info["waits"], np.random.get_state()))
        if cid != "j":
            for negative in (False, True):
                info = {}
                s1, s2, sign, _ = KC.dense_tail(E, T, cid, negative, info)
                rows.append((s1, s2, sign, info["launches"], info["waits"], np.random.get_state()))
        out[name] = rows
    return out


@pytest.mark.parametrize("cid", KC.VALUE)
def test_callers_take_the_one_call_and_leave_the_stream_as_before(pkg, monkeypatch, cid):
    """`tt_eig._split` and the dense tail of `_step_size_local_solve` with the switch on: fewer launches than with
    TTIPM_SPLIT_KICK=1, which takes fewer than the default; no more host waits; the same MT19937 state as
    with the switch off; the reference's rank and product"""
    E, T = pkg
    out = _callers(E, T, cid, monkeypatch)
    for k, what in enumerate(("_split", "dense tail, ev >= 0", "dense tail, ev < 0")):
        d, s, t = out["default"][k], out["split_kick"][k], out["trunc_kick"][k]
        print(cid, what, "launches: default", d[3], "split_kick", s[3], "trunc_kick", t[3], "| host waits", d[4],
              s[4], t[4])
        assert t[3] < s[3] < d[3]
        assert t[4] <= d[4]
        assert KC.same_state(t[5], d[5]) and KC.same_state(t[5], KC.state_after(cid))
        KC.check_rank_and_product(cid, t[0], t[1], t[2])
        KC.check_orthonormal(cid, t[0], t[1])
    assert out["trunc_kick"][0][3] == 1 and out["trunc_kick"][0][4] == 1  # _split: the call and its one read


@pytest.mark.parametrize("cid", KC.VALUE)
def test_nothing_new_runs_with_the_switch_off(pkg, monkeypatch, cid):
    E, T = pkg

    def boom(*a, **k):
        raise AssertionError("dev.trunc_kick called with the switch off")

    monkeypatch.setattr(T.D, "TRUNC_KICK", False)
    monkeypatch.setattr(T.D, "trunc_kick", boom)
    s1, s2 = KC.split(E, T, cid)
    KC.check_rank_and_product(cid, s1, s2)
    for negative in (False, True):
        s1, s2, sign, _ = KC.dense_tail(E, T, cid, negative)
        assert KC.same_state(np.random.get_state(), KC.state_after(cid))
        KC.check_rank_and_product(cid, s1, s2, sign)


def test_case_that_does_not_fit_takes_the_composed_path(on, monkeypatch):
    E, T = on

    def boom(*a, **k):
        raise AssertionError("dev.trunc_kick called on a shape that does not fit")

    monkeypatch.setattr(T.D, "trunc_kick", boom)
    info = {}
    s1, s2 = KC.split(E, T, "j", info)
    assert info["launches"] > 1
    assert KC.same_state(np.random.get_state(), KC.state_after("j"))
    KC.check_rank_and_product("j", s1, s2)


S41 = [c for c in SC.CASES if c.startswith("s41")]
S14 = [c for c in SC.CASES if c.startswith("s14")]


def _eig(E, D, case, native):
    A, Dl, x0, st, ref, xr = SC.call(case)
    up = (lambda tt: None if tt is None else [D.from_numpy(c) for c in tt])
    E._NATIVE = native
    try:
        np.random.set_state(st)
        n0 = E.NATIVE_CALLS["native"]
        l0, y0 = D.lib.ttk_launch_count(), D.lib.ttk_sync_count()
        s, x = E.tt_max_generalised_eigen(up(A), up(Dl), x0=up(x0), tol=1e-8)
        ran = E.NATIVE_CALLS["native"] - n0
    finally:
        E._NATIVE = True
    return (s, [D.read(c) for c in x], np.random.get_state(), ran, D.lib.ttk_launch_count() - l0,
            D.lib.ttk_sync_count() - y0)


@pytest.mark.parametrize("case", S41)
def test_eigen_als_with_the_switch_on(pkg, monkeypatch, case):
    """the s41 calls of tests/golden/step.npz with the switch on: the reference's step to test_gpu_step.py's
    1e-12 relative, its solution ranks, the native and the Python orchestration bit-identical, the stream state
    of the switch-off run, and fewer launches than it"""
    E, T = pkg
    ref, xr = SC.call(case)[4], SC.call(case)[5]
    monkeypatch.setattr(T.D, "TRUNC_KICK", False)
    so, xo, ro, ran_o, lo, yo = _eig(E, T.D, case, True)
    monkeypatch.setattr(T.D, "TRUNC_KICK", True)
    sn, xn, rn, ran_n, ln, yn = _eig(E, T.D, case, True)
    sp, xp, rp, ran_p, lp, yp = _eig(E, T.D, case, False)
    assert ran_o == 1 and ran_n == 1 and ran_p == 0
    print("s41-record", json.dumps({"case": case, "reference": ref, "off": {"step": so, "rel": abs(so - ref) / ref,
                                    "launches": lo, "waits": yo},
                                    "on": {"step": sn, "rel": abs(sn - ref) / ref, "launches": ln, "waits": yn}}))
    assert abs(so - ref) <= 1e-12 * ref, (so, ref)
    assert abs(sn - ref) <= 1e-12 * ref, (sn, ref)
    assert case not in SC.DEVICE_RANK_DEPARTURES
    assert [int(c.shape[-1]) for c in xn] == [c.shape[-1] for c in xr]
    assert sn == sp, (sn, sp)
    assert [c.shape for c in xn] == [c.shape for c in xp]
    assert all(np.array_equal(a, b) for a, b in zip(xn, xp))
    assert np.array_equal(rn[1], rp[1]) and rn[2:] == rp[2:]
    assert np.array_equal(rn[1], ro[1]) and rn[2:] == ro[2:]
    assert ln < lo and yn <= yo


def test_eigen_als_s14_record(pkg, monkeypatch, capsys):
    """the s14 calls with the switch off and on: their steps and ranks are printed for the profile, not asserted
    (their departures from the reference are tests/step_cases.py's and belong to the local eigenproblems)"""
    E, T = pkg
    with capsys.disabled():
        for case in S14:
            ref, xr = SC.call(case)[4], SC.call(case)[5]
            row = {"case": case, "reference": ref, "reference_ranks": [int(c.shape[-1]) for c in xr]}
            for switch in (False, True):
                monkeypatch.setattr(T.D, "TRUNC_KICK", switch)
                s, x, _, ran, launches, waits = _eig(E, T.D, case, True)
                row["on" if switch else "off"] = {"step": s, "rel": abs(s - ref) / ref, "native": ran,
                                                  "ranks": [int(c.shape[-1]) for c in x], "launches": launches,
                                                  "waits": waits}
            print("s14-record", json.dumps(row))


def test_maxcut_5_solve_with_the_switch_on(pkg, monkeypatch):
    """one maxcut dim-5 solve, switch on against off: the same iteration count as the golden run, fewer launches,
    and the gap within smoke()'s bound against the reference's own run (1e-6 relative, tests/golden/runs.json)"""
    import yaml
    from ttipm_amd.utils import run_and_record
    D = pkg[1].D
    cfg = yaml.safe_load(open(os.path.join(ROOT, "configs", "maxcut_5.yaml")))
    gold = json.load(open(os.path.join(ROOT, "tests", "golden", "runs.json")))["maxcut_5_r1_s0"]
    got = {}
    for switch in (False, True):
        monkeypatch.setattr(D, "TRUNC_KICK", switch)
        l0 = D.lib.ttk_launch_count()
        got[switch] = run_and_record("maxcut", cfg, 0, 1)
        got[switch]["launches"] = D.lib.ttk_launch_count() - l0
        print("switch", switch, "iters", got[switch]["num_iters"], "gap", got[switch]["gap"], "launches",
              got[switch]["launches"])
    assert got[True]["num_iters"] == got[False]["num_iters"] == gold["num_iters"]
    assert got[True]["launches"] < got[False]["launches"]
    assert abs(got[True]["gap"] - gold["gap"]) <= 1e-6 * abs(gold["gap"]), (got[True]["gap"], gold["gap"])
