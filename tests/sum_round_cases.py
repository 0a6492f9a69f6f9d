"""Shared by tests/test_host_sum_round.py (CPU, emulated libttk) and tests/test_gpu_sum_round.py (MI355X): the
fixtures of tests/golden/sum_round.npz (made by tests/golden/make_sum_round.py from the reference's own
`tt_rank_reduce(tt_add(a, tt_scale(alpha, b)))`, `tt_sub`, `tt_sum` and `_tt_*symmetrise`) and the checks both
files apply to a rounded weighted sum of trains.

Tolerances are tests/round_one_cases.py's: the represented tensor to 1e-11 relative max-abs against the tensor
of the reference's stored cores, ranks exactly, which is fair because the fixture records per case the
decision `margin` (>= 3) and the reference's own `noise` (50 x noise <= 1e-11), both asserted here on import.
Case z (a - a) has a zero output: its error is measured against `scale` = max |dense a|, not against the
output."""
import numpy as np

from tests.tt_cases import close, dense, load  # noqa: F401  (re-exported)

_F = load("sum_round.npz")
G, _tt = _F.G, _F._tt

VALUE = ("c", "o", "n", "u", "t", "s", "p", "m", "z", "w", "e", "j")   # every case
FIT = tuple(c for c in VALUE if c != "j")                                # those that fit one workgroup's LDS
TRACKED = tuple(c for c in VALUE if int(G[f"{c}/mode"]) > 0)
J_SHAPES = [(1, 4, 4, 64), (64, 4, 4, 64), (64, 4, 4, 1)]
RTOL = 1e-11
NOISE_MULTIPLE = 50
MARGIN = 3.0
BIG = 1 << 62

for _c in VALUE:
    assert NOISE_MULTIPLE * float(G[f"{_c}/noise"]) <= RTOL, (_c, float(G[f"{_c}/noise"]))
    assert float(G[f"{_c}/margin"]) >= MARGIN, (_c, float(G[f"{_c}/margin"]))
assert TRACKED == ("p", "m") and all(float(G[f"{c}/factor"]) > 0.0 for c in TRACKED)

_STORED, _DENSE = {}, {}


def stored(cid):
    """The case's distinct trains (host arrays, fresh copies); `which(cid)` names the one each term uses."""
    if cid not in _STORED:
        if cid == "j":  # too large to store: regenerated from the recorded seed (legacy stream: frozen)
            seed = int(G["j/seed"])
            _STORED[cid] = [[np.random.RandomState(seed + i).randn(*s) for s in J_SHAPES] for i in range(2)]
        else:
            _STORED[cid] = [_tt(f"{cid}/t{i}") for i in range(int(G[f"{cid}/nt"]))]
    return [[c.copy() for c in t] for t in _STORED[cid]]


def which(cid):
    return [int(v) for v in G[f"{cid}/which"]]


def coeffs(cid):
    """the weight of each term as the reference applied it (after `tt_scale`'s fp32 cast)"""
    return [float(v) for v in G[f"{cid}/coef"]]


def transposed(cid):
    return [bool(v) for v in G[f"{cid}/tr"]]


def terms(cid, trains):
    """the term list of the case from its distinct trains (the symmetrise pattern passes X and DX twice)"""
    return [trains[w] for w in which(cid)]


def eps(cid):
    return float(G[f"{cid}/eps"])


def mode(cid):
    """0 `tt_sum_rank_reduce`, 1 `tt_sum_psd_rank_reduce`, 2 `tt_sum_mask_rank_reduce`"""
    return int(G[f"{cid}/mode"])


def mask(cid):
    return _tt(f"{cid}/mask")


def ranks(cid):
    return [int(v) for v in G[f"{cid}/ranks"]]


def qranks(cid):
    """the rounded ranks (before a tracked variant adds its correction), d+1 entries"""
    return [int(v) for v in G[f"{cid}/qranks"]]


def factor(cid):
    return float(G[f"{cid}/factor"])


def scale(cid):
    """what the dense error is measured against: max |dense output|, in case z max |dense a|"""
    return float(G[f"{cid}/scale"])


def term_ranks(t):
    return [int(t[0].shape[0])] + [int(c.shape[-1]) for c in t]


def sum_inner_and_ranks(cid, trains):
    """middle extents (products) and bond ranks of the summed train"""
    ts = terms(cid, trains)
    d = len(ts[0])
    rk = [1] + [sum(term_ranks(t)[k] for t in ts) for k in range(1, d)] + [1]
    return [int(np.prod(c.shape[1:-1])) for c in ts[0]], rk


def public(T, cid, trains):
    """the case's public call on the device trains `trains` (the distinct ones)"""
    args = (terms(cid, trains), coeffs(cid), transposed(cid))
    if mode(cid) == 0:
        return T.tt_sum_rank_reduce(*args, eps=eps(cid))
    if mode(cid) == 1:
        return T.tt_sum_psd_rank_reduce(*args, eps=eps(cid))
    return T.tt_sum_mask_rank_reduce(*args, mask=T.to_device(mask(cid)), eps=eps(cid))


def materialised(cid, trains):
    """The summed train on the host, `tt_add`'s layout: what the kernel's loads produce (test-side NumPy)."""
    ts = []
    for t, c, tr in zip(terms(cid, trains), coeffs(cid), transposed(cid)):
        t = [x.transpose(0, 2, 1, 3) if tr else x for x in t]
        ts.append([t[0] * c if c != 1.0 else t[0]] + list(t[1:]))
    d = len(ts[0])
    out = []
    for k in range(d):
        cs = [t[k] for t in ts]
        R0 = 1 if k == 0 else sum(c.shape[0] for c in cs)
        R1 = 1 if k == d - 1 else sum(c.shape[-1] for c in cs)
        core = np.zeros((R0, *cs[0].shape[1:-1], R1))
        a = b = 0
        for c in cs:
            core[(slice(0, 1) if k == 0 else slice(a, a + c.shape[0])), ...,
                 (slice(0, 1) if k == d - 1 else slice(b, b + c.shape[-1]))] = c
            a, b = a + c.shape[0], b + c.shape[-1]
        out.append(core)
    return out


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


def helper_calls(ipm):
    """the `tt_ipm` helpers by name, each as f(X, DX, mask, alpha, eps)"""
    return {
        "sym": lambda X, DX, m, a, e: ipm._tt_symmetrise(X, e),
        "psd": lambda X, DX, m, a, e: ipm._tt_psd_symmetrise(X, e),
        "mask": lambda X, DX, m, a, e: ipm._tt_mask_symmetrise(X, m, e),
        "step": lambda X, DX, m, a, e: ipm._tt_step_symmetrise(X, a, DX, e),
        "step_psd": lambda X, DX, m, a, e: ipm._tt_step_symmetrise(X, a, DX, e, 1),
        "step_mask": lambda X, DX, m, a, e: ipm._tt_step_symmetrise(X, a, DX, e, 2, m),
        "add": lambda X, DX, m, a, e: ipm._tt_add_round(X, DX, e),
        "axpy": lambda X, DX, m, a, e: ipm._tt_add_round(X, DX, e, a),
    }
