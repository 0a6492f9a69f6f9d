"""The truncate-and-kick split on the MI355X: the one-launch `ttk_split_kick` (csrc/ttk_split_kick.hip) against
the reference's outputs (tests/golden/split_kick.npz), against the composed copy / QR / einsum path, and its
launch, determinism, fallback, zero-input, validation and random-stream contracts; then the step-size
eigen-ALS and one whole solve with the switch on.  The path is off by default (TTIPM_SPLIT_KICK); the tests
switch it on by monkeypatch.  The fallback's value checks on the CPU: tests/test_host_split_kick.py."""
import json
import os

import numpy as np
import pytest

from tests import split_kick_cases as KC
from tests import step_cases as SC

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def pkg():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from ttipm_amd import tt_eig, tt_ops
    assert hasattr(tt_ops.D.lib, "ttk_split_kick")
    return tt_eig, tt_ops


@pytest.fixture
def on(pkg, monkeypatch):
    monkeypatch.setattr(pkg[1].D, "SPLIT_KICK", True)
    return pkg


def _up(D, cid):
    """(U, S or None, Vt, G) on the device, uploads done: the launch counts below see the split alone"""
    U, S, Vt = KC.factors(cid)
    ops = [D.from_numpy(U), None if S is None else D.from_numpy(S), D.from_numpy(Vt), D.from_numpy(KC.block(cid))]
    D.read(ops[0])
    return ops


def _one(D, cid, ops=None):
    """the one call on the case's operands: (s1, s2) on the host, and the launches it took"""
    rev, _, _, _, r, _ = KC.dims(cid)
    U, S, Vt, G = ops or _up(D, cid)
    l0 = D.lib.ttk_launch_count()
    out = D.split_kick(rev, U, S, Vt, r, G)
    n = D.lib.ttk_launch_count() - l0
    assert out is not None and out[2] == KC.q_of(cid)
    return D.read(out[0]), D.read(out[1]), n


def _composed(E, D, cid):
    """today's composed path on the same operands, as `tt_eig._split` calls it: (s1, s2) on the host, launches"""
    rev, _, _, _, r, r_add = KC.dims(cid)
    U, S, Vt, G = _up(D, cid)
    l0 = D.lib.ttk_launch_count()
    if rev:
        v = D.einsum("r,rj->rj", S, Vt)
        s1, s2, _ = E._kick_rev(v[:r].t(), U[:, :r].t(), r_add, G)
    else:
        v = Vt[:r] if S is None else D.einsum("r,rj->rj", S[:r], Vt[:r])
        s1, s2, _ = E._kick(U[:, :r], v, r_add, G)
    s1, s2 = D.contig(s1), D.contig(s2)
    n = D.lib.ttk_launch_count() - l0
    return D.read(s1), D.read(s2), n


@pytest.mark.parametrize("cid", KC.FIT)
def test_one_call_matches_reference(pkg, cid):
    """the rank exactly, s1 s2 to 1e-11, the orthonormal factor's Gram matrix and cat's projection to 1e-12"""
    D = pkg[1].D
    s1, s2, n = _one(D, cid)
    assert n == 1
    KC.check_rank_and_product(cid, s1, s2)
    KC.check_orthonormal(cid, s1, s2)
    D.check_handoffs()


@pytest.mark.parametrize("cid", KC.FIT)
def test_one_call_factors_match_reference_elementwise(pkg, cid):
    """s1 and s2 elementwise to 1e-11 where cond(cat) < 1e6 (every case: the largest is 23): the gauge is
    LAPACK's on both sides, dgeqrf's forward and dgerqf's backward"""
    s1, s2, _ = _one(pkg[1].D, cid)
    for name, got in (("s1", s1), ("s2", s2)):
        ref = KC.G[f"{cid}/{name}"]
        print(cid, name, "max abs difference", float(np.max(np.abs(got - ref))), "of", float(np.max(np.abs(ref))))
    KC.check_factors(cid, s1, s2)


@pytest.mark.parametrize("cid", KC.FIT)
def test_one_call_matches_composed(pkg, cid):
    """equal shapes, values within 1e-11 (backward: up to the row signs in which `dev.rq` differs from LAPACK's
    RQ, `split_kick_cases.check_same_split`), and the composed path takes more than one launch"""
    E, T = pkg
    s1, s2, _ = _one(T.D, cid)
    c1, c2, n = _composed(E, T.D, cid)
    assert n > 1
    KC.check_same_split(cid, s1, s2, c1, c2)


@pytest.mark.parametrize("cid", ("a", "c", "e", "f", "h"))
def test_abi_call_is_one_launch_without_a_host_wait(pkg, cid):
    """the direct call with G on the device: one launch, no host wait, inputs unchanged, two calls the same bits"""
    D = pkg[1].D
    ops = _up(D, cid)
    host = [None if t is None else D.read(t) for t in ops]
    l0, y0 = D.lib.ttk_launch_count(), D.lib.ttk_sync_count()
    rev, _, _, _, r, _ = KC.dims(cid)
    out = D.split_kick(rev, *ops[:3], r, ops[3])
    assert D.lib.ttk_launch_count() - l0 == 1
    assert D.lib.ttk_sync_count() == y0
    first = D.read(out[0]), D.read(out[1])
    again = _one(D, cid, ops)
    assert np.array_equal(first[0], again[0]) and np.array_equal(first[1], again[1])
    for t, h in zip(ops, host):
        assert t is None or np.array_equal(D.read(t), h)


@pytest.mark.parametrize("cid", KC.FIT)
def test_callers_take_the_one_call_and_leave_the_stream_as_before(pkg, monkeypatch, cid):
    """`tt_eig._split` / `tt_ops.add_kick_rank` with the switch on against the switch off: fewer launches, the
    same MT19937 state afterwards, the reference's rank and product, values within 1e-11 of each other
    (`split_kick_cases.check_same_split`)"""
    E, T = pkg
    out = {}
    for switch in (False, True):
        monkeypatch.setattr(T.D, "SPLIT_KICK", switch)
        info = {}
        s1, s2 = KC.public(E, T, cid, info)
        out[switch] = (s1, s2, info["launches"], np.random.get_state())
    off, on_ = out[False], out[True]
    print(cid, "launches: composed", off[2], "one call", on_[2])
    assert off[2] > 1 and on_[2] == 1
    assert KC.same_state(off[3], on_[3]) and KC.same_state(on_[3], KC.state_after(cid))
    KC.check_rank_and_product(cid, on_[0], on_[1])
    KC.check_same_split(cid, on_[0], on_[1], off[0], off[1])


def test_case_that_does_not_fit_takes_the_composed_path(on):
    E, T = on
    D = T.D
    assert D.split_kick_q(*KC.dims("j")) is None
    ops = _up(D, "j")
    assert D.split_kick(0, *ops[:3], KC.dims("j")[4], ops[3]) is None
    info = {}
    s1, s2 = KC.public(E, T, "j", info)
    assert info["launches"] > 1
    assert KC.same_state(np.random.get_state(), KC.state_after("j"))
    KC.check_rank_and_product("j", s1, s2)


def test_zero_solution_gives_a_finite_zero_product(pkg):
    s1, s2, _ = _one(pkg[1].D, "z")
    assert np.all(np.isfinite(s1)) and np.all(np.isfinite(s2))
    assert not (s1 @ s2).any() and not s2.any()


def test_validation_returns_err_arg_without_launching(pkg):
    D = pkg[1].D
    from ttipm_amd import _lib as L
    U, S, Vt, G = _up(D, "a")
    s1, s2 = D.empty(8, 7), D.empty(7, 8)
    P = lambda t: None if t is None else t.data_ptr()  # noqa: E731

    def call(rev=0, a=8, b=8, p=8, r=3, r_add=4, ptrs=(U, S, Vt, G, s1, s2)):
        return D.lib.ttk_split_kick(D.ctx(), rev, a, b, p, r, r_add, *[P(t) for t in ptrs])

    bad = [dict(rev=2), dict(rev=-1), dict(a=0), dict(b=0), dict(p=0), dict(r=0), dict(r_add=0), dict(r=9),
           dict(a=4, r=3), dict(b=4, r=3),                                   # p > min(a, b) with S given
           dict(a=512, r=16, p=16, b=16, r_add=96)]                          # does not fit
    bad += [dict(ptrs=tuple(None if i == k else t for i, t in enumerate((U, S, Vt, G, s1, s2)))) for k in (0, 2, 3, 4, 5)]
    for kw in bad:
        l0 = D.lib.ttk_launch_count()
        assert call(**kw) == L.TTK_ERR_ARG, kw
        assert D.lib.ttk_launch_count() == l0, kw
        assert b"ttk_split_kick" in D.lib.ttk_last_error(), kw
    l0 = D.lib.ttk_launch_count()
    assert call() == L.TTK_OK and call(ptrs=(U, None, Vt, G, s1, s2)) == L.TTK_OK   # S may be NULL
    assert D.lib.ttk_launch_count() - l0 == 2
    assert np.array_equal(D.read(s1), _one(D, "a")[0])  # s1 = Q does not depend on S


S41 = [c for c in SC.CASES if c.startswith("s41")]
S14 = [c for c in SC.CASES if c.startswith("s14")]


def _eig(E, D, case, native):
    A, Dl, x0, st, ref, xr = SC.call(case)
    up = (lambda tt: None if tt is None else [D.from_numpy(c) for c in tt])
    E._NATIVE = native
    try:
        np.random.set_state(st)
        n0 = E.NATIVE_CALLS["native"]
        l0 = D.lib.ttk_launch_count()
        s, x = E.tt_max_generalised_eigen(up(A), up(Dl), x0=up(x0), tol=1e-8)
        ran = E.NATIVE_CALLS["native"] - n0
    finally:
        E._NATIVE = True
    return s, [D.read(c) for c in x], np.random.get_state(), ran, D.lib.ttk_launch_count() - l0


@pytest.mark.parametrize("case", S41)
def test_eigen_als_with_the_switch_on(on, case):
    """the s41 calls of tests/golden/step.npz with the switch on: the reference's step to test_gpu_step.py's
    1e-12 relative, its solution ranks, and the native and the Python orchestration bit-identical"""
    E, T = on
    ref, xr = SC.call(case)[4], SC.call(case)[5]
    sn, xn, rn, ran_n, ln = _eig(E, T.D, case, True)
    sp, xp, rp, ran_p, _ = _eig(E, T.D, case, False)
    assert ran_n == 1 and ran_p == 0
    print(case, "step", sn, "reference", ref, "launches", ln)
    assert abs(sn - ref) <= 1e-12 * ref, (sn, ref)
    assert case not in SC.DEVICE_RANK_DEPARTURES
    assert [int(c.shape[-1]) for c in xn] == [c.shape[-1] for c in xr]
    assert sn == sp, (sn, sp)
    assert [c.shape for c in xn] == [c.shape for c in xp]
    assert all(np.array_equal(a, b) for a, b in zip(xn, xp))
    assert np.array_equal(rn[1], rp[1]) and rn[2:] == rp[2:]


def test_eigen_als_s14_record(pkg, monkeypatch, capsys):
    """the s14 calls with the switch off and on: their steps and ranks are printed for the profile, not asserted
    (their departures from the reference are tests/step_cases.py's and belong to the local eigenproblems)"""
    E, T = pkg
    with capsys.disabled():
        for case in S14:
            ref, xr = SC.call(case)[4], SC.call(case)[5]
            row = {"case": case, "reference": ref, "reference_ranks": [int(c.shape[-1]) for c in xr]}
            for switch in (False, True):
                monkeypatch.setattr(T.D, "SPLIT_KICK", switch)
                s, x, _, ran, launches = _eig(E, T.D, case, True)
                row["on" if switch else "off"] = {"step": s, "rel": abs(s - ref) / ref, "native": ran,
                                                  "ranks": [int(c.shape[-1]) for c in x], "launches": launches}
            print("s14-record", json.dumps(row))


def test_maxcut_5_solve_with_the_switch_on(pkg, monkeypatch):
    """one maxcut dim-5 solve, switch on against off: the same iteration count, and the gap within smoke()'s
    bound against the reference's own run (1e-6 relative, tests/golden/runs.json)"""
    import yaml
    from ttipm_amd.utils import run_and_record
    D = pkg[1].D
    cfg = yaml.safe_load(open(os.path.join(ROOT, "configs", "maxcut_5.yaml")))
    gold = json.load(open(os.path.join(ROOT, "tests", "golden", "runs.json")))["maxcut_5_r1_s0"]
    got = {}
    for switch in (False, True):
        monkeypatch.setattr(D, "SPLIT_KICK", switch)
        l0 = D.lib.ttk_launch_count()
        got[switch] = run_and_record("maxcut", cfg, 0, 1)
        got[switch]["launches"] = D.lib.ttk_launch_count() - l0
        print("switch", switch, "iters", got[switch]["num_iters"], "gap", got[switch]["gap"], "launches",
              got[switch]["launches"])
    assert got[True]["num_iters"] == got[False]["num_iters"] == gold["num_iters"]
    assert got[True]["launches"] < got[False]["launches"]
    assert abs(got[True]["gap"] - gold["gap"]) <= 1e-6 * abs(gold["gap"]), (got[True]["gap"], gold["gap"])
