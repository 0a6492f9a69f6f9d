"""Shared by tests/test_host_prod_round.py (CPU, emulated libttk) and tests/test_gpu_prod_round.py (MI355X): the
fixtures of tests/golden/prod_round.npz (made by tests/golden/make_prod_round.py from the reference's own
`tt_rank_reduce(tt_fast_matrix_vec_mul(a, b), eps)`, `tt_fast_mat_mat_mul`, `tt_fast_hadamard`, and
`tt_psd_rank_reduce` of the product for the tracked case) and the checks both files apply to a rounded product
of two trains.

Tolerances are tests/round_one_cases.py's: the represented tensor to 1e-11 relative max-abs against the tensor
of the reference's stored cores, ranks exactly, which is fair because the fixture records per case the
decision `margin` (>= 3) and the reference's own `noise` (50 x noise <= 1e-11), both asserted here on import.

The public products have no tracked variant.  The tracked rounding at eps is the plain rounding at eps / 2 (the
halving is exact) that also sums the discarded tail, so for case p the public call is the product at eps / 2,
and `finish` adds the reference's correction, the fixture's `factor` x I; the kernel's own tail is checked
against that factor by the GPU test of the ABI call."""
import numpy as np

from tests.tt_cases import close, dense, load  # noqa: F401  (re-exported)

_F = load("prod_round.npz")
G, _tt = _F.G, _F._tt

VALUE = ("c", "v", "g", "h", "q", "x", "k", "p", "e", "l", "j")   # every case
FIT = tuple(c for c in VALUE if c != "j")                          # those that fit one workgroup's LDS
TRACKED = tuple(c for c in VALUE if int(G[f"{c}/mode"]) > 0)
J_SHAPES = ([(1, 4, 4, 16), (16, 4, 4, 16), (16, 4, 4, 1)],) * 2
RTOL = 1e-11
NOISE_MULTIPLE = 50
MARGIN = 3.0
BIG = 1 << 62

for _c in VALUE:
    assert NOISE_MULTIPLE * float(G[f"{_c}/noise"]) <= RTOL, (_c, float(G[f"{_c}/noise"]))
    assert float(G[f"{_c}/margin"]) >= MARGIN, (_c, float(G[f"{_c}/margin"]))
assert TRACKED == ("p",) and float(G["p/factor"]) > 0.0

_STORED, _DENSE = {}, {}


def kind(cid):
    """`ttk_zipup`'s: 0 matrix x vector, 1 matrix x matrix, 2 / 3 Hadamard of vector / matrix trains"""
    return int(G[f"{cid}/kind"])


def same(cid):
    """the case multiplies a train with itself (x o x)"""
    return bool(int(G[f"{cid}/same"]))


def factors(cid):
    """(a, b), host arrays, fresh copies; b is the list a itself where the case multiplies a train with itself"""
    if cid not in _STORED:
        if cid == "j":  # too large a product to store: regenerated from the recorded seed (legacy stream: frozen)
            seed = int(G["j/seed"])
            _STORED[cid] = tuple([np.random.RandomState(seed + i).randn(*s) for s in ss]
                                 for i, ss in enumerate(J_SHAPES))
        else:
            _STORED[cid] = (_tt(f"{cid}/a"), None if same(cid) else _tt(f"{cid}/b"))
    a, b = _STORED[cid]
    a = [c.copy() for c in a]
    return a, (a if b is None else [c.copy() for c in b])


def upload(T, cid, host=None):
    """the factors on the device; one list passed twice where the case multiplies a train with itself"""
    a, b = factors(cid) if host is None else host
    da = T.to_device(a)
    return da, (da if b is a else T.to_device(b))


def eps(cid):
    return float(G[f"{cid}/eps"])


def mode(cid):
    """0 `tt_rank_reduce` of the product, 1 `tt_psd_rank_reduce` of it"""
    return int(G[f"{cid}/mode"])


def ranks(cid):
    return [int(v) for v in G[f"{cid}/ranks"]]


def qranks(cid):
    """the rounded ranks (before the tracked variant adds its correction), d+1 entries"""
    return [int(v) for v in G[f"{cid}/qranks"]]


def factor(cid):
    return float(G[f"{cid}/factor"])


def scale(cid):
    return float(G[f"{cid}/scale"])


def train_ranks(t):
    return [int(t[0].shape[0])] + [int(c.shape[-1]) for c in t]


def modes(k, a, b):
    """`ttk_zipup`'s modes for these factors: three physical extents per core, 1 where the kind has none"""
    out = []
    for x, y in zip(a, b):
        out += {0: [x.shape[1], x.shape[2], 1], 1: [x.shape[1], x.shape[2], y.shape[2]],
                2: [x.shape[1], 1, 1], 3: [x.shape[1], x.shape[2], 1]}[k]
    return [int(v) for v in out]


def prod_inner_and_ranks(k, a, b):
    """middle extents (products) and bond ranks of the product train"""
    inner = [int(x.shape[1] * (y.shape[2] if k == 1 else x.shape[2] if k == 3 else 1)) for x, y in zip(a, b)]
    return inner, [ra * rb for ra, rb in zip(train_ranks(a), train_ranks(b))]


def fast(T, k):
    return (T.tt_fast_matrix_vec_mul, T.tt_fast_mat_mat_mul, T.tt_fast_hadamard, T.tt_fast_hadamard)[k]


def public(T, cid, a, b):
    """the case's public product of the device trains, rounded to the reference's rounded ranks (see the
    module's note on the tracked case)"""
    return fast(T, kind(cid))(a, b, eps(cid) / 2.0 if mode(cid) else eps(cid))


def finish(T, cid, res):
    """the host cores to compare with the reference's: the tracked case gets the reference's correction"""
    if mode(cid):
        assert [res[0].shape[0]] + [c.shape[-1] for c in res] == qranks(cid)
        res = T._psd_correct(list(res), factor(cid))
    return T.to_host(res)


def materialised(k, a, b):
    """The product train on the host in the composed path's layout, row a rb + b, column A Rb + B: what the
    kernel's loads produce (test-side NumPy).  A Hadamard element is one IEEE multiply; a contraction is
    summed in NumPy's order, which only matters where the partial sums are not exact."""
    out = []
    for x, y in zip(a, b):
        if k == 0:
            c = np.einsum("amnA,rnR->armAR", x, y)
        elif k == 1:
            c = np.einsum("amkA,bknB->abmnAB", x, y)
        elif k == 2:
            c = x[:, None, :, :, None] * y[None, :, :, None, :]
        else:
            c = x[:, None, :, :, :, None] * y[None, :, :, :, None, :]
        out.append(np.ascontiguousarray(c.reshape(c.shape[0] * c.shape[1], *c.shape[2:-2], c.shape[-2] * c.shape[-1])))
    return out


def integer_factors(cid, seed):
    """factors of the case's shapes with entries from the non-zero integers of magnitude <= 3: every product and
    partial sum of a product core is an exact integer, whatever the order of summation, and never a signed zero
    by cancellation of inexact terms"""
    rng = np.random.default_rng(seed)
    a, b = factors(cid)

    def draw(t):
        return [(rng.integers(1, 4, c.shape) * rng.choice((-1, 1), c.shape)).astype(np.float64) for c in t]
    a2 = draw(a)
    return a2, (a2 if b is a else draw(b))


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
