"""The NumPy emulator of libttk (`tests/emu_ttk.py`) against the references and bounds of
`tests/elementwise_cases.py`, through the same call layer as `test_gpu_elementwise.py`: the raw entry points
with explicit pointers and strides, and `dev.*` on CPU tensors (its ctypes marshalling).  This anchors the
emulator that every `test_host_*` file trusts, and proves the case table and the references without a GPU."""
import pytest

from tests import elementwise_cases as C
from tests.emu_ttk import emulated_ttipm


@pytest.fixture(scope="module")
def B():
    import torch
    pkg = emulated_ttipm()
    from ttipm_amd import _lib, dev
    assert pkg is not None and dev.lib is _lib.lib and dev.DEV.type == "cpu"
    return C.Backend(dev, _lib.lib, torch.device("cpu"))


def _report(bad):
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("op", C.EW_OPS)
def test_elementwise(B, op):
    _report([m for c in C.EW if c["op"] == op for r in c["routes"] for m in C.run_ew(B, c, r)])


def test_recip(B):
    _report(C.run_recip(B))


def test_dot(B):
    _report([m for c in C.DOT for m in C.run_dot(B, c)])


def test_normalize(B):
    _report([m for c in C.NORMALIZE for m in C.run_normalize(B, c)])


def test_rayleigh_tail(B):
    _report([m for n in C.RED_N for m in C.run_rayleigh(B, n)])


def test_rank_scan(B):
    _report([m for n, nq in C.RANK_SCAN for m in C.run_rank_scan(B, n, nq)])


def test_sumsq_batched(B):
    _report([m for n, nb in C.SUMSQ for m in C.run_sumsq(B, n, nb)])


@pytest.mark.parametrize("layout,nb", C.SUMSQ2_LAYOUT)
def test_sumsq_batched_strided(B, layout, nb):
    _report([m for inner in C.SUMSQ2_INNER for outer in C.SUMSQ2_OUTER
             for m in C.run_sumsq_strided(B, inner, outer, layout, nb)])
    assert B.lib.ttk_sumsq_batched_strided(B.stream(), 0, 4, 1, 4, 0, 4, 0) == C.ERR_ARG


def test_tt_join(B):
    _report([m for mode, rk, mid in C.JOIN for m in C.run_join(B, mode, rk, mid)])
    _report([m for mode, rk, mid in C.JOIN_REJECTED for m in C.run_join(B, mode, rk, mid, rejected=True)])


def test_copy_many(B):
    _report([m for n in C.COPY_MANY_N for m in C.run_copy_many(B, n)])


def test_add_diag(B):
    _report([m for n, lda in C.ADD_DIAG for m in C.run_add_diag(B, n, lda)])


def test_fill(B):
    _report([m for n in C.FILL_N for m in C.run_fill(B, n)])


@pytest.mark.parametrize("route", ["abi", "dev"])
def test_read_and_upload_are_identities(B, route):
    _report(C.in_fresh_thread(lambda: C.run_read(B, route)))
    _report(C.in_fresh_thread(lambda: C.run_upload(B, route)))
