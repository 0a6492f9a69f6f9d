"""libttk's element-wise, reduction, assembly and transfer kernels on the GPU against the NumPy references and
the derived bounds of `tests/elementwise_cases.py` (its docstring states each bound and where its constant
comes from).  Every case runs by two routes where both exist: the raw C ABI through `ttipm_amd._lib.lib`
(ctypes, explicit shape and stride arrays) and the `dev.*` wrapper (the `_ttkbind` packers).  Inputs reach the
device and results leave it through torch's copies, never through the kernels under test.  All tests need an
MI355X."""
import pytest

from tests import elementwise_cases as C

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from ttipm_amd import dev as D
    return D


@pytest.fixture(scope="module")
def B(dev):
    import torch
    from ttipm_amd._lib import lib
    return C.Backend(dev, lib, torch.device("cuda"))


def _report(bad):
    assert not bad, "\n".join(bad)


def test_dev_route_takes_the_native_packers(dev):
    """the `dev` route of the cases below is the `_ttkbind` marshalling, the `abi` route the ctypes one"""
    assert dev._BIND is not None and dev._FAST2 and dev.DEV.type == "cuda"


@pytest.mark.parametrize("op", C.EW_OPS)
def test_elementwise(B, op):
    l0 = B.lib.ttk_launch_count()
    _report([m for c in C.EW if c["op"] == op for r in c["routes"] for m in C.run_ew(B, c, r)])
    # one libttk launch per accepted call, none for a rejected one
    assert B.lib.ttk_launch_count() - l0 == sum(len(c["routes"]) for c in C.EW if c["op"] == op and not c["err"])


def test_recip(B):
    _report(C.run_recip(B))


def test_dot_sync_and_dev(B):
    """`ttk_dot_nd_sync`, `ttk_dot_nd_dev`, `dev.dot` and `dev.dot_into`: each within the bound, all bit-equal"""
    _report([m for c in C.DOT for m in C.run_dot(B, c)])


def test_normalize(B):
    _report([m for c in C.NORMALIZE for m in C.run_normalize(B, c)])


def test_rayleigh_tail_sync_and_dev(B):
    _report([m for n in C.RED_N for m in C.run_rayleigh(B, n)])


def test_rank_scan(B):
    _report([m for n, nq in C.RANK_SCAN for m in C.run_rank_scan(B, n, nq)])


def test_sumsq_batched(B):
    _report([m for n, nb in C.SUMSQ for m in C.run_sumsq(B, n, nb)])


@pytest.mark.parametrize("layout,nb", C.SUMSQ2_LAYOUT)
def test_sumsq_batched_strided(B, layout, nb):
    _report([m for inner in C.SUMSQ2_INNER for outer in C.SUMSQ2_OUTER
             for m in C.run_sumsq_strided(B, inner, outer, layout, nb)])
    assert B.lib.ttk_sumsq_batched_strided(B.stream(), 0, 4, 1, 4, 0, 4, 0) == C.ERR_ARG  # inner = 0: no launch


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
def test_read_sync(B, route):
    """on a fresh context: the mapped buffer grows at the first read above 8192 doubles, the pinned copy takes
    over above 65 536, and a small read afterwards still works"""
    _report(C.in_fresh_thread(lambda: C.run_read(B, route)))


@pytest.mark.parametrize("route", ["abi", "dev"])
def test_upload_ring(B, route):
    """on a fresh context: 70 uploads through the ring of 64 pinned slots from one reused host array"""
    _report(C.in_fresh_thread(lambda: C.run_upload(B, route)))
