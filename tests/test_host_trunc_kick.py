"""The one-launch tail of the two-site step-size local solve (`ttk_trunc_kick`, `dev.trunc_kick`,
TTIPM_TRUNC_KICK; reference `src/tt_als.py:1022-1053`), the part that needs no device: the C ABI's declaration,
binding and export, the host side of the plan (`ttk_trunc_kick_lds` is a host function), the fixture's own
conditions, and the path's callers on the CPU (libttk replaced by the NumPy emulator) against the reference's
outputs (tests/golden/trunc_kick.npz) with the switch off and on -- on the CPU, on takes today's composed path.
The device run: tests/test_gpu_trunc_kick.py."""
import ctypes
import os
import re

import numpy as np
import pytest

from tests import trunc_kick_cases as KC
from tests.emu_ttk import emulated_ttipm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SO = os.path.join(ROOT, "tensor-train-interior-point-method_amd", "libttk.so")
NAMES = ("ttk_trunc_kick", "ttk_trunc_kick_lds", "ttk_trunc_kick_read")


@pytest.fixture(scope="module")
def pkg():
    emulated_ttipm()
    from ttipm_amd import tt_eig, tt_ops
    return tt_eig, tt_ops


def _planner():
    lib = ctypes.CDLL(SO)
    f = lib.ttk_trunc_kick_lds
    f.restype = ctypes.c_int64
    f.argtypes = [ctypes.c_int] * 5 + [ctypes.c_void_p]
    return f


def test_header_binding_and_library_name_the_call():
    txt = open(os.path.join(ROOT, "include", "ttk.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    names = set(re.findall(r"\b(ttk_[a-z0-9_]+)\s*\(", txt))
    assert set(NAMES) <= names
    src = open(os.path.join(ROOT, "tensor-train-interior-point-method_amd", "_lib.py")).read()
    assert all(f'"{n}"' in src for n in NAMES)
    assert os.path.exists(SO), "libttk.so not built (run __graft_entry__.build())"
    lib = ctypes.CDLL(SO)
    assert all(hasattr(lib, n) for n in NAMES)


def test_fixture_cases_do_what_they_are_there_for():
    d = {c: KC.dims(c) for c in KC.ALL}
    rq = {c: (d[c][4], d[c][5]) for c in KC.ALL}
    assert rq["a"] == rq["c"] == (3, 7)
    assert rq["b"] == rq["d"] == (4, 6)                         # q capped by the rows
    assert d["b"][1] == 6 and d["d"][2] == 6
    assert rq["e"] == rq["f"] == (5, 9)
    assert d["e"][1] > 64 and d["f"][2] > 64                    # rows past one wave's stride
    assert d["e"][1] > d["e"][2] and d["f"][1] < d["f"][2]      # the SVD on the other of M and M^T
    assert rq["g"] == (1, 2) and d["g"][1:3] == (2, 2)
    assert rq["m"] == (4, 8) and d["m"][3] == 4                 # the cap decides ...
    e2 = KC.trunc_tol("m") ** 2
    sc = KC.tail_sums("m")
    assert sc[6] < e2 < sc[5]                                   # ... where the pruning keeps 6
    assert rq["h"] == (8, 8) and KC.trunc_tol("h") == 1e-30     # r = p
    assert rq["k"] == (8, 12) and d["k"][:3] == (1, 32, 32)
    assert rq["z"] == (1, 5) and not KC.matrix("z").any()
    assert d["j"][1:3] == (512, 64)
    for c in KC.ALL:                                            # the two conditions of the module's import
        assert KC.NOISE_MULTIPLE * float(KC.G[f"{c}/noise"]) <= KC.RTOL
        rev, a, b, max_rank, r, q = d[c]
        assert q == min(b if rev else a, r + KC.R_ADD) and r <= min(a, b, max_rank)
        if c == "z":
            continue
        e2 = KC.trunc_tol(c) ** 2
        assert all(v < e2 / KC.MARGIN or v > KC.MARGIN * e2 for v in KC.tail_sums(c)), c
        assert abs(np.linalg.norm(KC.matrix(c)) - 1.0) <= 1e-14


def test_planner_is_host_arithmetic():
    """`ttk_trunc_kick_lds` through ctypes, no device: every fitting case fits with the right qmax, case j and
    every invalid argument give -1 and leave qmax_out alone"""
    f = _planner()
    for cid in KC.FIT:
        q = ctypes.c_int64(-7)
        got = f(*KC.lds_args(cid), ctypes.byref(q))
        assert 0 <= got <= KC.LDS_MAX, (cid, got)
        assert q.value == KC.qmax_of(cid), cid
        assert q.value >= KC.dims(cid)[5]
        assert f(*KC.lds_args(cid), None) == got  # qmax_out may be NULL
    q = ctypes.c_int64(-7)
    assert f(*KC.lds_args("j"), ctypes.byref(q)) == -1 and q.value == -7
    ok = (0, 8, 8, 4, 32)
    assert f(*ok, None) >= 0
    bad = [(2, 8, 8, 4, 32), (-1, 8, 8, 4, 32), (0, 0, 8, 4, 32), (0, 8, 0, 4, 32), (0, 8, 8, 0, 32),
           (0, 8, 8, 4, 0), (0, -8, 8, 4, 32), (1, 8, 8, -1, 32), (1, 8, 8, 4, -3)]
    for args in bad:
        q = ctypes.c_int64(-7)
        assert f(*args, ctypes.byref(q)) == -1 and q.value == -7, args
    # the largest square the working set admits grows with nothing but the extents: (64, 64) fits, (128, 128) not
    assert f(0, 64, 64, 4, 64, None) >= 0 and f(1, 64, 64, 4, 64, None) >= 0
    assert f(0, 128, 128, 4, 64, None) == -1


@pytest.mark.parametrize("switch", (False, True))
@pytest.mark.parametrize("cid", KC.CALLERS)
def test_split_matches_reference_on_the_emulator(pkg, monkeypatch, cid, switch):
    """`tt_eig._split` on the solution: the reference's rank, product to 1e-11, an orthonormal factor, and the
    stream left as the reference's one draw leaves it, with the switch off and on (on the CPU the switch changes
    nothing: the fallback)"""
    E, T = pkg
    monkeypatch.setattr(T.D, "TRUNC_KICK", switch)
    assert T.D.trunc_kick_qmax(*KC.lds_args(cid)) is None
    s1, s2 = KC.split(E, T, cid)
    assert KC.same_state(np.random.get_state(), KC.state_after(cid))
    KC.check_rank_and_product(cid, s1, s2)
    KC.check_orthonormal(cid, s1, s2)


@pytest.mark.parametrize("negative", (False, True))
@pytest.mark.parametrize("switch", (False, True))
@pytest.mark.parametrize("cid", ("a", "c", "b", "d", "g", "m", "h"))
def test_dense_tail_matches_reference_on_the_emulator(pkg, monkeypatch, cid, switch, negative):
    """the dense branch of `_step_size_local_solve` from the pencil on (ev >= 0, and ev < 0 where the split is
    redone on the branch's solution): the same checks, the product up to the sign the eigensolver chose"""
    E, T = pkg
    monkeypatch.setattr(T.D, "TRUNC_KICK", switch)
    s1, s2, sign, step = KC.dense_tail(E, T, cid, negative)
    assert abs(step - (0.5 if negative else 1.0)) <= 1e-12
    assert KC.same_state(np.random.get_state(), KC.state_after(cid))
    KC.check_rank_and_product(cid, s1, s2, sign)
    KC.check_orthonormal(cid, s1, s2)


@pytest.mark.parametrize("cid", ("a", "c", "m"))
def test_switch_changes_nothing_on_the_emulator(pkg, monkeypatch, cid):
    E, T = pkg
    out = {}
    for switch in (False, True):
        monkeypatch.setattr(T.D, "TRUNC_KICK", switch)
        out[switch] = KC.split(E, T, cid) + KC.dense_tail(E, T, cid, False)[:2]
    assert all(np.array_equal(x, y) for x, y in zip(out[False], out[True]))
