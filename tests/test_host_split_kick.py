"""The one-launch truncate-and-kick split (`ttk_split_kick`, `dev.split_kick`, TTIPM_SPLIT_KICK; reference
`src/tt_als.py:1023-1053`), the part that needs no device: the C ABI's declaration, binding and export, the
host side of the plan (`ttk_split_kick_lds` is a host function), and the path's callers on the CPU (libttk
replaced by the NumPy emulator) against the reference's own outputs (tests/golden/split_kick.npz) with the
switch off and on -- on the CPU, on takes today's composed path.  The device run: tests/test_gpu_split_kick.py."""
import ctypes
import os
import re

import numpy as np
import pytest

from tests import split_kick_cases as KC
from tests.emu_ttk import emulated_ttipm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SO = os.path.join(ROOT, "tensor-train-interior-point-method_amd", "libttk.so")
NAMES = ("ttk_split_kick", "ttk_split_kick_lds")


@pytest.fixture(scope="module")
def pkg():
    emulated_ttipm()
    from ttipm_amd import tt_eig, tt_ops
    return tt_eig, tt_ops


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
    q = {c: KC.q_of(c) for c in KC.ALL}
    assert (q["a"], q["b"], q["c"], q["d"], q["g"]) == (7, 6, 7, 6, 2)
    assert KC.dims("b")[1] < KC.dims("b")[4] + KC.dims("b")[5]      # more columns than rows
    assert KC.dims("e")[1] > 64                                      # rows past one wave's stride
    assert KC.dims("h")[3] == KC.dims("h")[4]                        # r = p
    assert KC.factors("f")[1] is None and not KC.factors("z")[1].any()
    assert set(KC.SPLIT) == {"a", "b", "c", "d", "e", "g", "h"}
    for c in KC.ALL:
        assert int(KC.G[f"{c}/rank"]) == q[c]


def test_planner_is_host_arithmetic():
    """`ttk_split_kick_lds` through ctypes, no device: every fitting case fits with the right q, case j and
    every invalid argument give -1"""
    lib = ctypes.CDLL(SO)
    f = lib.ttk_split_kick_lds
    f.restype = ctypes.c_int64
    f.argtypes = [ctypes.c_int] * 6 + [ctypes.c_void_p]
    for cid in KC.FIT:
        q = ctypes.c_int64(-7)
        got = f(*KC.dims(cid), ctypes.byref(q))
        assert 0 <= got <= KC.LDS_MAX, (cid, got)
        assert q.value == KC.q_of(cid), cid
        assert f(*KC.dims(cid), None) == got  # q_out may be NULL
    q = ctypes.c_int64(-7)
    assert f(*KC.dims("j"), ctypes.byref(q)) == -1 and q.value == -7
    ok = (0, 8, 8, 8, 3, 4)
    assert f(*ok, None) >= 0
    for at in (1, 2, 3, 4, 5):                     # a zero extent (r_add = 0 among them)
        bad = list(ok)
        bad[at] = 0
        assert f(*bad, None) == -1, bad
    assert f(0, 8, 8, 3, 4, 4, None) == -1         # r > p
    assert f(2, 8, 8, 8, 3, 4, None) == -1         # rev = 2
    assert f(-1, 8, 8, 8, 3, 4, None) == -1


@pytest.mark.parametrize("switch", (False, True))
@pytest.mark.parametrize("cid", KC.ALL)
def test_callers_match_reference_on_the_emulator(pkg, monkeypatch, cid, switch):
    """exact rank, product to 1e-11, orthonormal factor, and the stream left as the reference's one draw
    leaves it, with the switch off and on (on the CPU the switch changes nothing: the fallback)"""
    E, T = pkg
    monkeypatch.setattr(T.D, "SPLIT_KICK", switch)
    assert T.D.split_kick_q(*KC.dims(cid)) is None
    s1, s2 = KC.public(E, T, cid)
    assert KC.same_state(np.random.get_state(), KC.state_after(cid))
    KC.check_rank_and_product(cid, s1, s2)
    KC.check_orthonormal(cid, s1, s2)


@pytest.mark.parametrize("cid", KC.ALL)
def test_switch_changes_nothing_on_the_emulator(pkg, monkeypatch, cid):
    E, T = pkg
    out = {}
    for switch in (False, True):
        monkeypatch.setattr(T.D, "SPLIT_KICK", switch)
        out[switch] = KC.public(E, T, cid)
    assert all(np.array_equal(x, y) for x, y in zip(out[False], out[True]))
