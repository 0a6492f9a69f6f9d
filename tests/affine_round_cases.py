"""Shared by tests/test_host_affine_round.py (CPU, emulated libttk) and tests/test_gpu_affine_round.py (MI355X):
the fixtures of tests/golden/affine_round.npz (made by tests/golden/make_affine_round.py from the reference's own
`tt_rank_reduce` / `tt_psd_rank_reduce` of `tt_add`, `tt_scale`, `tt_transpose` of plain trains and `tt_fast_*`
products) and the checks both files apply to a rounded weighted sum of trains and products of two trains.

Tolerances are tests/round_one_cases.py's: the represented tensor to 1e-11 relative max-abs against the tensor
of the reference's stored cores, ranks exactly, which is fair because the fixture records per case the
decision `margin` (>= 3) and the reference's own `noise` (50 x noise <= 1e-11), both asserted here on import.
Case z (A x - b with b the exact product) has an output at noise level: its error is measured against `scale`
= max |dense A x|.

The public function has no tracked variant.  The tracked rounding at eps is the plain rounding at eps / 2 (the
halving is exact) that also sums the discarded tail, so for case t the public call rounds at eps / 2 and `finish`
adds the reference's correction, the fixture's `factor` x I; the kernel's own tail is checked against that factor
by the GPU test of the ABI call."""
import numpy as np

from tests import prod_round_cases as PC
from tests.tt_cases import close, dense, load  # noqa: F401  (re-exported)

_F = load("affine_round.npz")
G, _tt = _F.G, _F._tt

VALUE = ("c", "r", "f", "u", "y", "m", "g", "t", "z", "s", "j")   # every case
FIT = tuple(c for c in VALUE if c != "j")                          # those that fit one workgroup's LDS
TRACKED = tuple(c for c in VALUE if int(G[f"{c}/mode"]) > 0)
# case j's trains: a (4, 4) operator of ranks 16, a vector of ranks 16 (product rank 256), b of ranks 2
J_SHAPES = ([(1, 4, 4, 16), (16, 4, 4, 16), (16, 4, 4, 1)], [(1, 4, 16), (16, 4, 16), (16, 4, 1)],
            [(1, 4, 2), (2, 4, 2), (2, 4, 1)])
RTOL = 1e-11
NOISE_MULTIPLE = 50
MARGIN = 3.0
BIG = 1 << 62

for _c in VALUE:
    assert NOISE_MULTIPLE * float(G[f"{_c}/noise"]) <= RTOL, (_c, float(G[f"{_c}/noise"]))
    assert float(G[f"{_c}/margin"]) >= MARGIN, (_c, float(G[f"{_c}/margin"]))
assert TRACKED == ("t",) and float(G["t/factor"]) > 0.0

_STORED, _DENSE = {}, {}


def stored(cid):
    """The case's distinct trains (host arrays, fresh copies); `kinds`, `ia`, `ib` say which each term uses."""
    if cid not in _STORED:
        if cid == "j":  # too large to store: regenerated from the recorded seed (legacy stream: frozen)
            seed = int(G["j/seed"])
            _STORED[cid] = [[np.random.RandomState(seed + i).randn(*s) for s in ss] for i, ss in enumerate(J_SHAPES)]
        else:
            _STORED[cid] = [_tt(f"{cid}/t{i}") for i in range(int(G[f"{cid}/nt"]))]
    return [[c.copy() for c in t] for t in _STORED[cid]]


def kinds(cid):
    """per term: -1 a plain train, else `ttk_zipup`'s product kind"""
    return [int(v) for v in G[f"{cid}/kind"]]


def ia(cid):
    return [int(v) for v in G[f"{cid}/ia"]]


def ib(cid):
    return [int(v) for v in G[f"{cid}/ib"]]


def coeffs(cid):
    """the weight of each term as the reference applied it (after `tt_scale`'s fp32 cast)"""
    return [float(v) for v in G[f"{cid}/coef"]]


def transposed(cid):
    return [bool(v) for v in G[f"{cid}/tr"]]


def mids(cid):
    """the middle shape of every core of the result"""
    return tuple(int(v) for v in G[f"{cid}/mids"])


def terms(cid, trains, coefs=None):
    """`tt_affine_rank_reduce`'s term list of the case from its distinct trains"""
    out = []
    for k, a, b, c, tr in zip(kinds(cid), ia(cid), ib(cid), coeffs(cid) if coefs is None else coefs, transposed(cid)):
        out.append((c, trains[a] if k < 0 else (k, trains[a], trains[b]), tr))
    return out


def eps(cid):
    return float(G[f"{cid}/eps"])


def mode(cid):
    """0 `tt_rank_reduce` of the operand, 1 `tt_psd_rank_reduce` of it"""
    return int(G[f"{cid}/mode"])


def ranks(cid):
    return [int(v) for v in G[f"{cid}/ranks"]]


def qranks(cid):
    """the rounded ranks (before the tracked variant adds its correction), d+1 entries"""
    return [int(v) for v in G[f"{cid}/qranks"]]


def factor(cid):
    return float(G[f"{cid}/factor"])


def scale(cid):
    """what the dense error is measured against: max |dense output|, in case z max |dense A x|"""
    return float(G[f"{cid}/scale"])


def train_ranks(t):
    return [int(t[0].shape[0])] + [int(c.shape[-1]) for c in t]


def term_ranks(cid, trains):
    """the bond ranks of every term: the train's own, or the products of the two factors'"""
    out = []
    for k, a, b in zip(kinds(cid), ia(cid), ib(cid)):
        ra = train_ranks(trains[a])
        out.append(ra if k < 0 else [x * y for x, y in zip(ra, train_ranks(trains[b]))])
    return out


def inner_and_ranks(cid, trains):
    """middle extents (products) and bond ranks of the summed train"""
    tr = term_ranks(cid, trains)
    d = len(tr[0]) - 1
    return [int(np.prod(mids(cid)))] * d, [1] + [sum(r[k] for r in tr) for k in range(1, d)] + [1]


def public(T, cid, trains, with_norm2=False):
    """the case's public call on the device trains `trains` (the distinct ones); see the module's note on the
    tracked case"""
    return T.tt_affine_rank_reduce(terms(cid, trains), eps=eps(cid) / 2.0 if mode(cid) else eps(cid),
                                   with_norm2=with_norm2, mids=mids(cid))


def finish(T, cid, res):
    """the host cores to compare with the reference's: the tracked case gets the reference's correction"""
    if mode(cid):
        assert [res[0].shape[0]] + [c.shape[-1] for c in res] == qranks(cid)
        res = T._psd_correct(list(res), factor(cid))
    return T.to_host(res)


def materialised(cid, trains, coefs=None):
    """The operand on the host with flat middle indices, `tt_add`'s layout of the terms, every product in the
    composed path's layout (PC.materialised), a transposed term with its two middle indices swapped, the weight
    applied to core 0 (skipped for a weight of 1): what the kernel's loads produce (test-side NumPy)."""
    m = mids(cid)
    ts = []
    for k, a, b, c, tr in zip(kinds(cid), ia(cid), ib(cid), coeffs(cid) if coefs is None else coefs, transposed(cid)):
        t = [x for x in trains[a]] if k < 0 else PC.materialised(k, trains[a], trains[b])
        t = [x.reshape(x.shape[0], -1, x.shape[-1]) for x in t]
        if tr:
            t = [x.reshape(x.shape[0], m[1], m[0], x.shape[-1]).transpose(0, 2, 1, 3).reshape(x.shape) for x in t]
        ts.append([t[0] * c if c != 1.0 else t[0]] + list(t[1:]))
    d = len(ts[0])
    out = []
    for k in range(d):
        cs = [t[k] for t in ts]
        R0 = 1 if k == 0 else sum(c.shape[0] for c in cs)
        R1 = 1 if k == d - 1 else sum(c.shape[-1] for c in cs)
        core = np.zeros((R0, cs[0].shape[1], R1))
        a = b = 0
        for c in cs:
            core[(slice(0, 1) if k == 0 else slice(a, a + c.shape[0])), :,
                 (slice(0, 1) if k == d - 1 else slice(b, b + c.shape[-1]))] = c
            a, b = a + c.shape[0], b + c.shape[-1]
        out.append(core)
    return out


def integer_trains(cid, seed):
    """trains of the case's shapes with entries from the non-zero integers of magnitude <= 3 (PC.integer_factors'
    rule): every product, partial sum and weighted element of the operand is exact, whatever the order"""
    rng = np.random.default_rng(seed)
    return [[(rng.integers(1, 4, c.shape) * rng.choice((-1, 1), c.shape)).astype(np.float64) for c in t]
            for t in stored(cid)]


def reference_dense(cid):
    """The tensor the reference's output represents (computed once per case, shared, read only)."""
    if cid not in _DENSE:
        _DENSE[cid] = dense(_tt(f"{cid}/out"))
        _DENSE[cid].setflags(write=False)
    return _DENSE[cid]


def check_result(cid, res_host):
    """ranks exactly the reference's, bonds consistent, dense tensor to 1e-11 of `scale`"""
    assert [res_host[0].shape[0]] + [c.shape[-1] for c in res_host] == ranks(cid)
    assert all(a.shape[-1] == b.shape[0] for a, b in zip(res_host[:-1], res_host[1:]))
    ref = reference_dense(cid)
    got = dense(res_host)
    assert got.shape == ref.shape
    err = float(np.max(np.abs(got - ref))) / scale(cid)
    assert err <= RTOL, (cid, err)


def ipm_state(T, ipm, active=False):
    """a small synthetic solver state, d = 3: (st, trains by name), everything of rank 2 but the rank-1 mask"""
    import types
    rng = np.random.default_rng(20270105)

    def tt(mid, r=2):
        rk = [1, r, r, 1]
        return T.to_device([rng.standard_normal((rk[k], *mid, rk[k + 1])) for k in range(3)])
    v = {"L": tt((4, 4)), "b": tt((4,)), "X": tt((2, 2)), "C": tt((4,)), "Z": tt((2, 2)), "Y": tt((4,)),
         "P": tt((4, 4)), "Tt": tt((2, 2)), "mask": tt((2, 2), 1)}
    v["Ladj"] = T.tt_transpose(v["L"])
    st = types.SimpleNamespace(eta=1e-3, eps=1e-12, primal_error_normalisation=3.0, dual_error_normalisation=2.5,
                               ineq_boundary_val=0.01,
                               ineq_status=ipm.IneqStatus.ACTIVE if active else ipm.IneqStatus.NOT_IN_USE)
    return st, v


def old_ipm_expressions(T, ipm):
    """the expressions of tt_ipm.py that the four rewired sites replace, as they stood"""
    from ttipm_amd.tt_als import tt_mat_vec_mul

    def primal(st, v):
        e = 0.01 * st.eta * st.primal_error_normalisation
        return T.tt_rank_reduce(T.tt_sub(tt_mat_vec_mul(v["L"], T.tt_reshape(v["X"], (4,)), e, st.eps), v["b"]), e)

    def dual(st, v):
        act = st.ineq_status is ipm.IneqStatus.ACTIVE
        df = T.tt_rank_reduce(T.tt_sub(T.tt_fast_matrix_vec_mul(v["Ladj"], v["Y"], st.eps),
                                       T.tt_rank_reduce(T.tt_add(T.tt_reshape(v["Z"], (4,)), v["C"]), st.eps)),
                              st.eps if act else 0.01 * st.eta * st.dual_error_normalisation)
        if act and v["Tt"] is not None:
            df = T.tt_rank_reduce(T.tt_sub(df, T.tt_reshape(v["Tt"], (4,))),
                                  0.01 * st.eta * st.dual_error_normalisation)
        return df

    def yupd(st, v):
        e_d = 0.1 * st.eta * st.dual_error_normalisation
        Y = v["Y"]
        return T.tt_reshape(ipm._tt_symmetrise(T.tt_reshape(T.tt_sub(Y, T.tt_fast_matrix_vec_mul(v["P"], Y, st.eps)),
                                                            (2, 2)), e_d), (4,))

    def mx(st, v):
        return T.tt_rank_reduce(T.tt_add(T.tt_scale(st.ineq_boundary_val, v["mask"]),
                                         T.tt_fast_hadamard(v["mask"], v["X"], st.eps)), eps=st.eps)
    return {"primal": primal, "dual": dual, "dual_active": dual, "y": yupd, "mx": mx}


def new_ipm_helpers(ipm):
    """the four rewired sites of tt_ipm.py by name, each as f(st, trains)"""
    return {
        "primal": lambda st, v: ipm.tt_compute_primal_feasibility(v["L"], v["b"], v["X"], st),
        "dual": lambda st, v: ipm.tt_compute_dual_feasibility(v["C"], v["Ladj"], v["Z"], v["Y"], v["Tt"], st),
        "dual_active": lambda st, v: ipm.tt_compute_dual_feasibility(v["C"], v["Ladj"], v["Z"], v["Y"], v["Tt"], st),
        "y": lambda st, v: ipm._tt_project_symmetrise(v["Y"], v["P"], 0.1 * st.eta * st.dual_error_normalisation, st),
        "mx": lambda st, v: ipm._tt_boundary_masked(v["mask"], v["X"], st),
    }
