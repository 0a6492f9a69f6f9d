"""Dump the outputs of a fixed set of kernel calls (extreme eigenpairs, offset-table GEMMs) on seeded
inputs, so two library builds can be compared bit for bit (tools/cmp_dump.py).  A second argument
keeps only the arrays whose name starts with it and skips the sections that have none:
`python tools/dump_kernels.py out.npz round_` dumps the native TT roundings alone.

    TTK_LIB_PATH=old.so python tools/dump_kernels.py gpurun_out/a.npz
    python tools/dump_kernels.py gpurun_out/b.npz        # then compare the two files on the host"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ttipm_amd import dev as D  # noqa: E402
from ttipm_amd._lib import lib  # noqa: E402


def rounding(out):
    """The output cores of `ttk_rand_orth`, `ttk_nystroem`, `ttk_retract`, `ttk_round_one`, `ttk_sum_round_one` and
    `ttk_prod_round_one`: every fixture case that takes the native path, the two seeded inputs of the device tests
    and the all-zero train."""
    from tests import nystroem_cases as NC, randorth_cases as RO, retract_cases as RT
    from ttipm_amd import tt_ops as T

    def dump(name, launches, f, *trains):
        trains = [T.to_device(list(t)) for t in trains]
        D.read(trains[0][0])  # uploads done
        l0 = lib.ttk_launch_count()
        res = f(*trains)
        assert lib.ttk_launch_count() - l0 == launches, name  # the native path ran
        out[name] = np.concatenate([c.ravel() for c in T.to_host(res)])

    for cid in RO.FIT:
        dump(f"round_randorth_{cid}", 1, T._tt_lr_random_orthogonalise, RO.train(cid), RO.sketch(cid))
    dump("round_randorth_wide", 1, T._tt_lr_random_orthogonalise, *RO.wide_case())
    for cid in NC.FIT:
        dump(f"round_nystroem_{cid}", 3, T._tt_generalised_nystroem, NC.train(cid), *NC.sketches(cid))
    dump("round_nystroem_transposed", 3, T._tt_generalised_nystroem, *NC.transposed_case())
    old, T.NATIVE_RETRACT = T.NATIVE_RETRACT, True
    try:
        for cid in RT.FIT:
            dump(f"round_retract_{cid}", 1, lambda tt: T.tt_rank_retraction(tt, RT.upper(cid)), RT.train(cid))
        rk = [1] + [5] * 5 + [1]
        dump("round_retract_zero", 1, lambda tt: T.tt_rank_retraction(tt, [3] * 5),
             [np.zeros((rk[i], 4, rk[i + 1])) for i in range(6)])
    finally:
        T.NATIVE_RETRACT = old
    from tests import round_one_cases as R1
    old, T.ROUND_ONE = T.ROUND_ONE, True
    try:
        for cid in R1.ORTH:  # `ttk_round_one` and the copy kernel of its one read
            dump(f"round_one_{cid}", 2, lambda tt: T.tt_rank_reduce(tt, R1.eps(cid)), R1.train(cid))
    finally:
        T.ROUND_ONE = old
    from tests import prod_round_cases as PC, sum_round_cases as SC
    old, T.SUM_ROUND_ONE, T.PROD_ROUND_ONE = (T.SUM_ROUND_ONE, T.PROD_ROUND_ONE), True, True
    try:
        for cid in SC.FIT:  # `ttk_sum_round_one` / `ttk_prod_round_one` and the copy kernel of the one read
            if SC.mode(cid) == 0:
                dump(f"round_sum_{cid}", 2, lambda *ts: SC.public(T, cid, list(ts)), *SC.stored(cid))
        for cid in PC.FIT:
            a, b = PC.factors(cid)
            if b is a:
                dump(f"round_prod_{cid}", 2, lambda x: PC.public(T, cid, x, x), a)
            else:
                dump(f"round_prod_{cid}", 2, lambda x, y: PC.public(T, cid, x, y), a, b)
    finally:
        T.SUM_ROUND_ONE, T.PROD_ROUND_ONE = old


def kernels(out):
    rng = np.random.default_rng(0)
    st = D._stream()
    for n in [3, 5, 10, 17, 40, 63, 64, 80, 100, 127, 128, 129, 139, 150, 192, 200, 256, 257, 258, 300, 384, 512, 513,
              1000, 1900]:
        for which in (0, 1):
            M = rng.standard_normal((n, n))
            A = D.from_numpy(M + M.T)
            wx = D.empty(int(lib.ttk_syev_extreme_work(n)))
            buf = D.empty(n + 1)
            D.check(lib.ttk_syev_extreme(st, D._p(A), n, which, D._p(buf), D._p(buf[1:]), D._p(wx)), "syev")
            out[f"syev_{n}_{which}"] = D.read(buf)
    for M_, N_, K_ in [(212, 64, 2544), (60, 44, 2700), (30, 20, 7), (172, 600, 64), (336, 336, 336), (700, 650, 520)]:
        a = torch.randn(M_, K_, dtype=torch.float64, device="cuda", generator=torch.Generator("cuda").manual_seed(K_))
        b = torch.randn(K_, N_, dtype=torch.float64, device="cuda", generator=torch.Generator("cuda").manual_seed(N_))
        out[f"mm_{M_}_{N_}_{K_}"] = D.read(D.matmul(a, b))
        out[f"mmT_{M_}_{N_}_{K_}"] = D.read(D.matmul(b.t(), a.t()))
    # LU with the dgecon estimate (getrf + lu_rcond_kernel) and getrs
    import ctypes
    for n in (40, 300, 600, 1000, 2100, 3120, 4000, 4500):
        M = rng.standard_normal((n, n)) + np.diag(np.linspace(0.0, 3.0, n))
        A = D.from_numpy(M)
        piv = torch.empty(n, dtype=torch.int32, device="cuda")
        work = D.empty(2 * n + 16)
        rc = ctypes.c_double(0.0)
        D.check(lib.ttk_lu_sync(st, D._p(A), n, D._p(piv), D._p(work), ctypes.byref(rc)), "lu")
        b = D.from_numpy(rng.standard_normal((n, 3)))
        D.lu_solve_(A, piv, b)
        out[f"lu_{n}"] = D.read(A)
        out[f"lu_rcond_{n}"] = np.array([rc.value])
        out[f"lu_sol_{n}"] = D.read(b)
    # one-workgroup Householder QR (ttk_qr; the narrow launch for m <= 65) on the ranks' shapes
    for (m_, n_) in [(10, 5), (24, 6), (16, 4), (8, 2), (4, 5), (2, 5), (48, 12), (56, 14), (128, 8), (16, 12),
                     (65, 20), (64, 64), (66, 10), (1, 3), (3, 1), (40, 40), (20, 1200), (60, 400)]:
        Q_, R_ = D.qr(D.from_numpy(rng.standard_normal((m_, n_))))
        out[f"qr_{m_}_{n_}"] = np.concatenate([D.read(Q_).ravel(), D.read(R_).ravel()])
    # VALU local-apply rows (maxcut-sized fused applies: single launches)
    old = lib.ttk_fused_set_mfma(0)
    try:
        for eq in ("lsr,smnS,LSR,rnR->lmL", "lsr,smnS,LSR,lmL->rnR"):
            for shapes in ([(12, 3, 12), (3, 4, 4, 3), (12, 3, 12), (12, 4, 12)],
                           [(7, 5, 9), (5, 4, 4, 2), (11, 2, 13), (9, 4, 13)]):
                P, A, Q = (rng.standard_normal(s) for s in shapes[:3])
                x = rng.standard_normal(shapes[3] if eq.endswith("->lmL") else (P.shape[0], A.shape[1], Q.shape[0]))
                ops = [D.from_numpy(o) for o in (P, A, Q, x)]
                out[f"valu_{eq[-3:]}_{shapes[0]}"] = D.read(D.einsum(eq, *ops, fused=True))
                o2 = D.from_numpy(np.ones(out[f"valu_{eq[-3:]}_{shapes[0]}"].shape))
                D.einsum(eq, *ops, out=o2, alpha=0.5, beta=2.0, fused=True)
                out[f"valuab_{eq[-3:]}_{shapes[0]}"] = D.read(o2)
    finally:
        lib.ttk_fused_set_mfma(old)
    # MFMA local-apply rows (graphm-sized fused applies and environment updates)
    from ttipm_amd import tt_als
    old = lib.ttk_fused_set_mfma(1)
    try:
        for eq in ("lsr,smnS,LSR,rnR->lmL", "lsr,smnS,LSR,lmL->rnR"):
            for shapes in ([(44, 10, 44), (10, 4, 4, 10), (44, 10, 44), (44, 4, 44)],
                           [(30, 18, 25), (18, 4, 4, 9), (28, 9, 33), (25, 4, 33)],
                           [(60, 12, 60), (12, 4, 4, 12), (60, 12, 60), (60, 4, 60)]):
                P, A, Q = (rng.standard_normal(s) for s in shapes[:3])
                x = rng.standard_normal(shapes[3] if eq.endswith("->lmL") else (P.shape[0], A.shape[1], Q.shape[0]))
                ops = [D.from_numpy(o) for o in (P, A, Q, x)]
                out[f"fused_{eq[-3:]}_{shapes[0]}"] = D.read(D.einsum(eq, *ops, fused=True))
                o2 = D.from_numpy(np.ones(out[f"fused_{eq[-3:]}_{shapes[0]}"].shape))
                D.einsum(eq, *ops, out=o2, alpha=0.5, beta=2.0, fused=True)
                out[f"fusedab_{eq[-3:]}_{shapes[0]}"] = D.read(o2)
        for backward, shapes in [(True, [(64, 3, 64), (78, 4, 64), (4, 4, 4, 3), (78, 4, 64)]),
                                 (False, [(47, 5, 47), (47, 4, 97), (5, 4, 4, 4), (47, 4, 97)]),
                                 (False, [(2, 12, 97), (2, 4, 2), (12, 4, 4, 13), (97, 4, 50)]),
                                 (True, [(44, 10, 44), (44, 4, 44), (10, 4, 4, 10), (44, 4, 44)])]:
            items = [tuple(D.from_numpy(rng.standard_normal(s)) for s in shapes)]
            out[f"env_{backward}_{shapes[0]}"] = D.read(tt_als.env_update_many(backward, items)[0])
    finally:
        lib.ttk_fused_set_mfma(old)
    # one-workgroup SVDs (QRCP + Jacobi) on plain and graded matrices, tall and wide
    for (m_, n_) in [(39, 52), (52, 39), (64, 63), (63, 64), (96, 80), (80, 96), (20, 17), (128, 40), (60, 90),
                     (12, 8), (8, 12), (96, 96), (4, 3), (8, 6), (6, 6), (16, 16), (40, 10), (30, 33),
                     (72, 72), (100, 75), (75, 100), (90, 70), (64, 65)]:
        for graded in (0, 1):
            M = rng.standard_normal((m_, n_))
            if graded:
                k = min(m_, n_)
                Uq, _ = np.linalg.qr(rng.standard_normal((m_, k)))
                Vq, _ = np.linalg.qr(rng.standard_normal((n_, k)))
                M = (Uq * np.logspace(0, -15, k)) @ Vq.T
            U_, S_, Vt_, _ = D.svd(D.from_numpy(M), host=False)
            out[f"svd_{m_}_{n_}_{graded}"] = np.concatenate([D.read(U_).ravel(), D.read(S_).ravel(), D.read(Vt_).ravel()])
    # multi-workgroup SVDs (QRCP launches + Jacobi sweeps), min(m, n) > 96
    for (m_, n_) in [(150, 120), (120, 150), (300, 200), (97, 97), (400, 130), (260, 255)]:
        for graded in (0, 1):
            M = rng.standard_normal((m_, n_))
            if graded:
                k = min(m_, n_)
                Uq, _ = np.linalg.qr(rng.standard_normal((m_, k)))
                Vq, _ = np.linalg.qr(rng.standard_normal((n_, k)))
                M = (Uq * np.logspace(0, -15, k)) @ Vq.T
            U_, S_, Vt_, _ = D.svd(D.from_numpy(M), host=False)
            out[f"svdbig_{m_}_{n_}_{graded}"] = np.concatenate([D.read(U_).ravel(), D.read(S_).ravel(),
                                                                 D.read(Vt_).ravel()])
    # Schur-reduced local KKT matvecs (VALU rows, side by side or not; MFMA rows), chained
    from ttipm_amd import tt_ipm
    for ineq in (False, True):
        for (r_, R_, s_, S_) in [(12, 16, 10, 9), (3, 4, 5, 5), (16, 20, 12, 12), (14, 96, 10, 9)]:
            cls = tt_ipm.IneqMatVecWrapper if ineq else tt_ipm.MatVecWrapper
            Lb = {k: D.from_numpy(rng.standard_normal((r_, s_, r_)) * 0.1) for k in cls.keys}
            Ab = {k: D.from_numpy(rng.standard_normal((s_, 4, 4, S_)) * 0.1) for k in cls.keys}
            Rb = {k: D.from_numpy(rng.standard_normal((R_, S_, R_)) * 0.1) for k in cls.keys}
            invI = D.from_numpy(rng.uniform(0.5, 2.0, (r_, 4, R_)))
            v = D.from_numpy(rng.standard_normal((3 if ineq else 2) * r_ * 4 * R_))
            op = cls(Lb, Ab, Rb, invI, (r_, 4, R_))
            y = op.matvec(op.matvec(v))
            out[f"schur_{int(ineq)}_{r_}_{R_}"] = D.read(y)
            if R_ < 50:  # whole LGMRES solves, every Arnoldi step on the multi-workgroup path
                from ttipm_amd import lgmres
                old = lib.ttk_lgmres_set_mw_threshold(0)
                try:
                    m_ = r_ * 4 * R_
                    info = {}
                    x = lgmres.lgmres(op.matvec_into, v, rtol=1e-10, max_it=300, restart=min(m_, 100),
                                      augment=max(min(m_, 100) // 10, 3), info=info, native=op.h)
                    out[f"lgmres_{int(ineq)}_{r_}_{R_}"] = np.concatenate([D.read(x), [info["its"], info["res"]]])
                finally:
                    lib.ttk_lgmres_set_mw_threshold(old)


def save(path, out):
    torch.cuda.synchronize()
    import hashlib
    for k in list(out):  # big arrays as a SHA-256 digest (keeps gpurun_out small); bitwise comparison still
        if out[k].size > 100000:
            out[k] = np.frombuffer(hashlib.sha256(np.ascontiguousarray(out[k]).tobytes()).digest(), dtype=np.uint8)
    np.savez(path, **out)
    print("dumped", len(out), "arrays to", path)


def main(path, prefix=""):
    out = {}
    if "round_".startswith(prefix[:6]):
        rounding(out)
    if not prefix.startswith("round_"):
        kernels(out)
    save(path, {k: v for k, v in out.items() if k.startswith(prefix)})


if __name__ == "__main__":
    main(*sys.argv[1:3])
