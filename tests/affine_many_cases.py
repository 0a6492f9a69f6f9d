"""Shared by tests/test_host_affine_many.py (CPU) and tests/test_gpu_affine_many.py (MI355X): how the cases of
tests/affine_round_cases.py (fixtures tests/golden/affine_round.npz, unchanged) are grouped into batches for
`ttk_affine_round_many` / `tt_ops.tt_affine_rank_reduce_many`, and the job records both files build.

The two batches hold every fitting case once.  Each mixes plain and product terms of several kinds, lengths d,
and the two planned workgroup widths (cases z and s plan 1024 threads, the others 256: the tests assert it through
the planner's `threads`); the first also mixes the plain and the tracked mode (case t) and holds the transposed
4-term case y and the noise-level case z, the second the transposed matrix product g and the d = 10 case s."""
import ctypes

from tests import affine_round_cases as AC

BATCHES = (("c", "r", "y", "t", "z"), ("f", "u", "m", "g", "s"))
MAX_JOBS = 8

assert sorted(c for b in BATCHES for c in b) == sorted(AC.FIT) and all(2 <= len(b) <= MAX_JOBS for b in BATCHES)
assert any(AC.mode(c) for c in BATCHES[0]) and not all(AC.mode(c) for c in BATCHES[0])
assert all(len({k for c in b for k in AC.kinds(c)}) >= 3 for b in BATCHES)

VP, I64 = ctypes.c_void_p, ctypes.c_int64


class Job(ctypes.Structure):
    """`ttk_affine_job` as include/ttk.h lays it out"""
    _fields_ = [("d", ctypes.c_int), ("inner", VP), ("rows", VP), ("nterms", ctypes.c_int), ("terms", VP),
                ("eps", ctypes.c_double), ("mode", ctypes.c_int), ("out", VP)]


def public_job(cid, dev):
    """the case as a job of `tt_affine_rank_reduce_many` on its distinct device trains: the case's own eps and
    mode (the tracked rounding halves eps itself)"""
    return AC.terms(cid, dev), AC.eps(cid), AC.mode(cid), AC.mids(cid)


def finish(T, cid, res):
    """the host cores of one returned (tt, factor, norm2) to compare with the reference's: the tracked case gets
    the reference's correction, as in AC.finish"""
    return AC.finish(T, cid, res[0])
