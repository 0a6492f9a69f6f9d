"""Cases, NumPy references and derived bounds for libttk's element-wise, reduction, assembly and transfer
kernels (`csrc/ttk_contract.hip`, `csrc/ttk_runtime.hip`), shared by `test_host_elementwise.py` (the NumPy
emulator `tests/emu_ttk.py` on the CPU) and `test_gpu_elementwise.py` (libttk on the GPU).

Nothing here imports the package: a test hands a `Backend` (the `dev` module, the library object and the torch
device) to the `run_*` functions, which make every call by two routes where both exist: the raw C ABI (explicit
pointers, shape and stride arrays) and the `dev.*` wrapper.  Data travels to and from the device through torch's
own copies, so `ttk_upload` / `ttk_read_sync` are tested by, not relied on for, the comparison.

References are written from the operations' definitions in `include/ttk.h`, in plain NumPy.  Sums and every
value that is compared through a bound are formed in `np.longdouble` (64-bit mantissa asserted below), so the
reference's own error is about 2^-11 of any bound.  No kernel, `dev.*` call or emulator builds a reference.

Bounds (u = 2^-53; all derived from the kernels' code, none measured)

* bit-equal to NumPy: pure copies (`copy_many`, `tt_join`, `fill`, upload / read round trips); `copy_nd` and
  `axpby_nd` with beta == 0 (one IEEE multiply, alpha * s); `mul_nd` with beta == 0 (two multiplies in the
  written order, (alpha * s1) * s2, which is NumPy's order for `alpha * s1 * s2`); `scale_axis` (one multiply);
  `add_diag` (one add); `rank_scan`'s running residual (-1.0 * g and 1.0 * r are exact, so r <- v + 1.0 * r is
  the single rounding of r - g whether or not the compiler contracts it into an FMA).
* element-wise with an add (`copy_nd` / `mul_nd` with beta != 0, `axpby_nd`): the device build leaves
  contraction on, so v + beta * t is either two roundings or one FMA.  The alpha term passes through at most
  three roundings (for `mul_nd`: alpha * s1, * s2, the add), the beta term through at most three (`axpby_nd`:
  gamma * s2, beta * t, the add).  With round-to-nearest's |delta| <= u / (1 + u) per operation,
  (1 + delta)^3 - 1 <= 3u, so every element is within 3u * (|alpha s| + |beta t|) of the exact value, where
  alpha s stands for alpha s1 s2 (`mul_nd`) and beta t for beta gamma s2 (`axpby_nd`).
* through sqrt or a division (`recip`, `scale_axis_ss`, `normalize`'s final scaling): 2 ulp per such operation,
  that is a relative 4u each (one ulp is at most 2u of the value), plus u for the multiply that follows:
  `recip` 4u |ref|; `scale_axis_ss` 5u |ref| (invert = 0: sqrt, multiply) or 9u |ref| (invert = 1: sqrt,
  division, multiply).  A clamped entry (sqrt(ss) <= 1e-10) uses the constant 1e-10 and only loses the sqrt.
  The bounds are not tightened to equality: nothing here proves the device's sqrt and division correctly rounded.
* reductions: |got - ref| <= k u sum|x_i y_i|, k the depth of the chain of roundings a term passes through.
  One workgroup of T threads (`dot_nd`, `normalize`, `rayleigh_tail`, `rank_scan`: T = 1024; `sumsq_batched*`:
  T = 256): thread t multiplies (1 rounding) and adds its ceil(n / T) terms one after another (ceil(n / T)
  roundings; an FMA only removes the product's), `ttk::wave_sum` adds four DPP levels within a 16-lane row and
  two levels over the four rows (6), `ttk::block_sum` adds the T / 64 wave sums serially (16, or 4).  That is
  ceil(n / 1024) + 23 roundings, respectively ceil(n / 256) + 11; with (1 + u)^d - 1 < (d + 1) u for these d:
      k_1024(n) = ceil(n / 1024) + 24,        k_256(n) = ceil(n / 256) + 12.
* composites:
  - `normalize`: s = sum x^2 has relative error k u (all terms positive), sqrt halves it, then sqrt and division
    (4u each) and the multiply (u); one u for second-order terms: |got_i - ref_i| <= (k / 2 + 10) u |ref_i|.
  - `rayleigh_tail`: E = k u sum|v_i Mv_i| bounds ev.  The update w_i = -ev v_i + Mv_i is an element-wise
    add: |w_i - wref_i| <= B_i = E |v_i| (1 + 3u) + 3u (|ev v_i| + |Mv_i|).  res2 = sum w_i^2 over the computed
    w: |res2 - sum wref_i^2| <= k u sum (|wref_i| + B_i)^2 + sum (2 |wref_i| B_i + B_i^2).
  - `rank_scan`: the residual is bit-equal (above), so out[q] is a plain reduction over it: k u sum r_i^2.

Poisoning: every source is a view into a larger base whose other entries are NaN, so a read outside the view
poisons the result; every destination is a view into a larger base filled with a NaN of a fixed bit pattern,
and every byte outside the view must be unchanged after the call.
"""
import ctypes
import threading
import zlib

import numpy as np

LD = np.longdouble
assert np.finfo(LD).nmant >= 63, "the references need an extended-precision long double"
U = 2.0 ** -53
ERR_ARG = 1  # TTK_ERR_ARG (include/ttk.h)
SENT_BITS = np.uint64(0x7FF8C0DEC0DEC0DE)
SENT = np.array([SENT_BITS]).view(np.float64)[0]
BIG = (5, 7, 6, 8, 9, 70)  # 1 058 400 elements: above the 4096 x 256 grid cap, 6-D, all extents distinct
GRID_CAP = 4096 * 256
c_dp = ctypes.POINTER(ctypes.c_double)


def k1024(n):
    return -(-n // 1024) + 24


def k256(n):
    return -(-n // 256) + 12


def _i64(vals):
    return (ctypes.c_int64 * len(vals))(*[int(v) for v in vals])


def _rng(name):
    return np.random.default_rng(zlib.crc32(name.encode()))


def _prod(shape):
    return int(np.prod(shape, dtype=np.int64)) if len(shape) else 1


class View:
    """`shape` / `strides` (in doubles) at `offset` of a base buffer of `size` doubles"""

    def __init__(self, shape, strides, offset, size):
        self.shape, self.strides, self.offset, self.size = tuple(shape), tuple(strides), int(offset), int(size)
        self.n = _prod(self.shape)
        idx = self.index()
        assert idx.size == 0 or (idx.min() >= 0 and idx.max() < self.size)

    def index(self):
        """flat base indices of the view's elements, in the view's C order"""
        i = np.full((), self.offset, dtype=np.int64)
        for e, s in zip(self.shape, self.strides):
            i = i[..., None] + np.arange(e, dtype=np.int64) * s
        return i.reshape(-1)

    def ptr(self, t):
        return t.data_ptr() + 8 * self.offset

    def tensor(self, t):
        import torch
        return torch.as_strided(t, self.shape, self.strides, self.offset)


def _cstrides(shape):
    st, acc = [], 1
    for e in reversed(shape):
        st.insert(0, acc)
        acc *= e
    return st


def contig(shape, pad=3):
    return View(shape, _cstrides(shape), pad, _prod(shape) + 2 * pad)


def permuted(shape, order, pad=3):
    """the view of `shape` whose axes lie in memory in `order` (slowest first)"""
    mem = _cstrides([shape[a] for a in order])
    st = [0] * len(shape)
    for pos, a in enumerate(order):
        st[a] = mem[pos]
    return View(shape, st, pad, _prod(shape) + 2 * pad)


def gapped(shape, pad=3):
    """contiguous strides of a tensor one larger along every axis: NaN (or sentinel) gaps inside the view's span"""
    st = _cstrides([e + 1 for e in shape])
    return View(shape, st, pad, 1 + sum((e - 1) * s for e, s in zip(shape, st)) + 2 * pad)


def src_base(v, rng):
    """NaN everywhere but the view's elements (standard normal)"""
    base = np.full(v.size, np.nan)
    ui = np.unique(v.index())
    base[ui] = rng.standard_normal(ui.size)
    return base


def dst_base(v, rng, init):
    """the sentinel everywhere; the view's elements standard normal when the call reads them (`init`)"""
    base = np.full(v.size, SENT)
    if init:
        base[v.index()] = rng.standard_normal(v.n)
    return base


def untouched(before, after, views):
    """every double of `after` outside `views` has the bits it had in `before`"""
    keep = np.ones(before.size, dtype=bool)
    for v in views:
        keep[v.index()] = False
    return np.array_equal(before.view(np.uint64)[keep], after.view(np.uint64)[keep])


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


class Backend:
    """what a `run_*` function needs of the code under test: the `dev` module, the library object behind it
    (libttk through ctypes, or the emulator) and the torch device its tensors live on"""

    def __init__(self, dev, lib, device):
        self.dev, self.lib, self.device = dev, lib, device

    def put(self, a):
        import torch
        return torch.from_numpy(np.array(a, dtype=np.float64, order="C", copy=True).reshape(-1)).to(self.device)

    def get(self, t):
        return t.detach().cpu().numpy().copy()

    def stream(self):
        return self.dev._stream()


def in_fresh_thread(fn):
    """run fn() on a new host thread: `dev` keeps a stream and a libttk context per thread, so the thread starts
    with an empty upload ring and an unallocated mapped read buffer whatever ran before"""
    box = []

    def body():
        try:
            box.append((True, fn()))
        except BaseException as e:  # re-raised on the caller's thread
            box.append((False, e))

    th = threading.Thread(target=body)
    th.start()
    th.join()
    ok, val = box[0]
    if not ok:
        raise val
    return val


# ------------------------------------------------------------------------------------------- element-wise
EW_OPS = ("copy", "mul", "axpby", "scale", "scale_ss")


def _case(name, op, s1, d, s2=None, alpha=1.0, beta=0.0, gamma=1.0, alias=False, axis=0, special=False, invert=0,
          err=False, routes=("abi", "dev")):
    d = s1 if d is None else d  # in place
    return dict(name=f"{op}-{name}", op=op, shape=d.shape, s1=s1, s2=s2, d=d, alpha=alpha, beta=beta, gamma=gamma,
                alias=alias, axis=axis, special=special, invert=invert, err=err, routes=routes)


def _bcast(m, pad=3):
    return View((m, m), (0, 1), pad, m + 2 * pad)


def _slice_dst(r=3, n=5, R=6, pad=3):
    """base[:, 2] of a contiguous (r, 4, n, R) tensor"""
    return View((r, n, R), (4 * n * R, R, 1), pad + 2 * n * R, r * 4 * n * R + 2 * pad)


_P1, _P2 = (3, 0, 5, 1, 4, 2), (5, 2, 4, 0, 3, 1)
_SEVEN = (2, 1, 2, 1, 2, 1, 2)


def _layouts(op):
    """the layouts shared by copy / mul / axpby: (name, s1, s2, d, keywords)"""
    two = op != "copy"
    out = []
    for n in (1, 255, 256, 257):
        out.append((f"n{n}", contig((n,)), contig((n,), 5), contig((n,), 4), {}))
    out.append(("big6", permuted(BIG, _P1), permuted(BIG, _P2, 2), contig(BIG), {}))
    out.append(("big6-acc", permuted(BIG, _P2), permuted(BIG, _P1, 1), contig(BIG), dict(alpha=0.5, beta=-1.25)))
    if two:  # inv_I.view(1, m).expand(m, m) is the second operand (tt_ipm.py)
        out.append(("bcast37", contig((37, 37)), _bcast(37), contig((37, 37), 2), {}))
    else:
        out.append(("bcast37", _bcast(37), None, contig((37, 37), 2), {}))
    out.append(("slice-dst", contig((3, 5, 6)), gapped((3, 5, 6)), _slice_dst(), {}))
    out.append(("slice-dst-acc", contig((3, 5, 6)), gapped((3, 5, 6)), _slice_dst(), dict(alpha=2.0, beta=1.0)))
    out.append(("T-in", permuted((9, 13), (1, 0)), contig((9, 13)), contig((9, 13)), {}))
    out.append(("T-out", contig((9, 13)), permuted((9, 13), (1, 0)), permuted((9, 13), (1, 0), 4), {}))
    out.append(("gapped", gapped((4, 3, 5)), permuted((4, 3, 5), (2, 0, 1)), gapped((4, 3, 5), 2), dict(alpha=-3.0)))
    al = contig((6, 7, 5))
    out.append(("alias", al, contig((6, 7, 5), 1), al, dict(alias=True, alpha=0.37)))
    out.append(("alias-acc", al, contig((6, 7, 5), 1), al, dict(alias=True, alpha=0.37, beta=1.0)))
    out.append(("acc", contig((300,)), contig((300,), 2), contig((300,), 1), dict(beta=1.0)))
    out.append(("acc-ev", contig((300,)), contig((300,), 2), contig((300,), 1), dict(alpha=-0.7318249, beta=1.0)))
    out.append(("0d", contig(()), contig((), 2), contig((), 1), dict(routes=("dev",), alpha=1.5)))
    out.append(("0d-acc", contig(()), contig((), 2), contig((), 1), dict(routes=("dev",), alpha=1.5, beta=-2.0)))
    out.append(("7d", contig(_SEVEN), contig(_SEVEN), contig(_SEVEN), dict(routes=("abi",), err=True)))
    return out


def _ew_cases():
    cases = []
    for op in ("copy", "mul", "axpby"):
        for name, s1, s2, d, kw in _layouts(op):
            kw = dict(kw)
            if op == "axpby":
                kw.setdefault("gamma", 0.75)
                if name in ("n255", "n257", "big6", "T-in"):  # axpby has no dst term: give beta a value
                    kw.setdefault("beta", 1.0)
                if kw.get("alias"):
                    continue  # dev.axpby's callers never alias
            cases.append(_case(name, op, s1, d, s2=s2 if op != "copy" else None, **kw))
    for op in ("scale", "scale_ss"):
        inv = dict(invert=1) if op == "scale_ss" else {}
        cases += [
            _case("n1", op, contig((1,)), contig((1,), 2)),
            _case("n255-last", op, contig((85, 3)), contig((85, 3), 2), axis=1),
            _case("n256-first16", op, permuted((16, 16), (1, 0)), contig((16, 16)), axis=0, **inv),
            _case("n257-extent1", op, contig((257, 1)), contig((257, 1)), axis=1),
            _case("first", op, gapped((4, 5, 6)), contig((4, 5, 6)), axis=0, **inv),
            _case("middle16", op, contig((5, 16, 3)), _slice_dst(5, 16, 3), axis=1),
            _case("last", op, permuted((6, 7, 3), (2, 0, 1)), gapped((6, 7, 3)), axis=2, **inv),
            _case("big6", op, permuted(BIG, _P1), contig(BIG), axis=3),
            _case("alias", op, contig((6, 7, 5)), None, axis=1, alias=True, **inv),
            _case("7d", op, contig(_SEVEN), contig(_SEVEN), axis=0, err=True, routes=("abi",)),
        ]
    cases.append(_case("extent17", "scale", contig((3, 17)), contig((3, 17)), axis=1, err=True, routes=("abi",)))
    for invert in (0, 1):
        cases += [
            _case(f"special-inv{invert}", "scale_ss", contig((7, 5, 4)), contig((7, 5, 4)), axis=1, special=True,
                  invert=invert),
            _case(f"extent70-inv{invert}", "scale_ss", permuted(BIG, _P2), contig(BIG), axis=5, invert=invert),
            _case(f"extent17-inv{invert}", "scale_ss", contig((3, 17)), gapped((3, 17)), axis=1, invert=invert),
        ]
    return cases


EW = _ew_cases()
# the table reaches what it is for
assert any(_prod(c["shape"]) > GRID_CAP for c in EW)
assert any(len(c["shape"]) == 6 for c in EW)
assert any(0 in v.strides and v.n > 1 for c in EW for v in (c["s1"], c["s2"]) if v is not None)
assert any(c["alias"] for c in EW)
assert all(any(c["op"] == op and _prod(c["shape"]) > GRID_CAP for c in EW) for op in EW_OPS)


def _ss_values(c, rng):
    ext = c["shape"][c["axis"]]
    ss = rng.random(ext) * 4.0 + 0.05
    if c["special"]:
        ss[1], ss[3] = 1e-30, 0.0  # both below the 1e-10 floor of sqrt(ss)
    return ss


def _coord(shape, axis):
    sh = [1] * len(shape)
    sh[axis] = shape[axis]
    return np.broadcast_to(np.arange(shape[axis]).reshape(sh), shape).reshape(-1)


def ew_reference(c, S1, S2, D0, aux):
    """('exact', values) or ('bound', longdouble values, per-element bound) from the operation's definition"""
    a, b, g = c["alpha"], c["beta"], c["gamma"]
    op = c["op"]
    if op == "scale":
        return "exact", S1 * aux[_coord(c["shape"], c["axis"])]
    if op == "scale_ss":
        nr = np.sqrt(aux.astype(LD))
        clamped = ~(nr > LD(1e-10))
        sc = np.where(clamped, LD(1e-10), nr)
        f = LD(1) / sc if c["invert"] else sc
        nops = (1.0 - clamped) + (1.0 if c["invert"] else 0.0)  # sqrt (unless clamped), division
        co = _coord(c["shape"], c["axis"])
        ref = S1.astype(LD) * f[co]
        return "bound", ref, (4.0 * nops[co] + 1.0) * U * np.abs(ref)
    if b == 0.0:
        return "exact", (a * S1 * S2 if op == "mul" else a * S1)
    t1 = LD(a) * S1.astype(LD) * (S2.astype(LD) if op == "mul" else LD(1))
    t2 = LD(b) * (LD(g) * S2.astype(LD) if op == "axpby" else D0.astype(LD))
    return "bound", t1 + t2, 3.0 * U * (np.abs(t1) + np.abs(t2))


def run_ew(B, c, route):
    """one element-wise case by one route; a list of failure texts"""
    rng = _rng(c["name"])
    op, d, s1, s2 = c["op"], c["d"], c["s1"], c["s2"]
    init = c["alias"] or (c["beta"] != 0.0 and op != "axpby")
    hd = dst_base(d, rng, init)
    h1 = hd if c["alias"] else src_base(s1, rng)
    h2 = src_base(s2, rng) if s2 is not None else None
    aux = None
    if op == "scale":
        aux = rng.standard_normal(max(c["shape"][c["axis"]], 16))
    elif op == "scale_ss":
        aux = _ss_values(c, rng)
    td = B.put(hd)
    t1 = td if c["alias"] else B.put(h1)
    t2 = B.put(h2) if s2 is not None else None
    tss = B.put(np.concatenate([[np.nan] * 2, aux, [np.nan] * 2])) if op == "scale_ss" else None
    S1 = h1[s1.index()]
    S2 = h2[s2.index()] if s2 is not None else None
    D0 = hd[d.index()]
    a, b, g = float(c["alpha"]), float(c["beta"]), float(c["gamma"])
    nd, shp = len(c["shape"]), _i64(c["shape"])
    lib, D = B.lib, B.dev
    rc = 0
    if route == "abi":
        st = B.stream()
        if op == "copy":
            rc = lib.ttk_copy_nd(st, s1.ptr(t1), d.ptr(td), nd, shp, _i64(s1.strides), _i64(d.strides), a, b)
        elif op == "mul":
            rc = lib.ttk_mul_nd(st, s1.ptr(t1), s2.ptr(t2), d.ptr(td), nd, shp, _i64(s1.strides), _i64(s2.strides),
                                _i64(d.strides), a, b)
        elif op == "axpby":
            rc = lib.ttk_axpby_nd(st, s1.ptr(t1), s2.ptr(t2), d.ptr(td), nd, shp, _i64(s1.strides),
                                  _i64(s2.strides), _i64(d.strides), a, b, g)
        elif op == "scale":
            sc = (ctypes.c_double * len(aux))(*aux)
            rc = lib.ttk_scale_axis(st, s1.ptr(t1), d.ptr(td), nd, shp, _i64(s1.strides), _i64(d.strides),
                                    c["axis"], sc)
        else:
            rc = lib.ttk_scale_axis_ss(st, s1.ptr(t1), d.ptr(td), nd, shp, _i64(s1.strides), _i64(d.strides),
                                       c["axis"], tss.data_ptr() + 16, c["invert"])
    else:
        T1, TD = s1.tensor(t1), d.tensor(td)
        T2 = s2.tensor(t2) if s2 is not None else None
        if op == "copy":
            D.copy_(TD, T1, a, b)
        elif op == "mul":
            D.mul_(TD, T1, T2, a, b)
        elif op == "axpby":
            D.axpby(T1, T2, a, b, g, out=TD)
        elif op == "scale":
            D.scale_axis(T1, c["axis"], aux[:c["shape"][c["axis"]]], out=TD)
        else:
            D.scale_axis_ss(T1, c["axis"], tss[2:2 + aux.size], bool(c["invert"]), out=TD)
    after = B.get(td)
    tag = f"{c['name']}[{route}]"
    if c["err"]:
        bad = []
        if rc != ERR_ARG:
            bad.append(f"{tag}: status {rc}, expected TTK_ERR_ARG")
        if not same_bits(after, hd):
            bad.append(f"{tag}: a rejected call wrote to its destination")
        return bad
    bad = []
    if rc != 0:
        return [f"{tag}: status {rc}"]
    if not untouched(hd, after, [d]):
        bad.append(f"{tag}: wrote outside the destination view")
    for t, h, nm in ((t1, h1, "src"), (t2, h2, "src2")):
        if t is not None and t is not td and not same_bits(B.get(t), h):
            bad.append(f"{tag}: {nm} changed")
    got = after[d.index()]
    ref = ew_reference(c, S1, S2, D0, aux)
    if ref[0] == "exact":
        if not same_bits(got, ref[1]):
            bad.append(f"{tag}: not bit-equal to NumPy ({int(np.sum(got != ref[1]))} of {got.size} differ)")
    else:
        err = np.abs(got.astype(LD) - ref[1])
        if not np.all(err <= ref[2]):
            w = int(np.argmax(np.where(np.isnan(err), np.inf, err - ref[2])))
            bad.append(f"{tag}: element {w}: |got - ref| = {float(err[w]):.3e} > bound {float(ref[2][w]):.3e}")
    return bad


def run_recip(B):
    """`ttk_recip` / `dev.recip`: contiguous, 4u |ref| (one division)"""
    bad = []
    for n in (1, 255, 256, 257, _prod(BIG)):
        v, d = contig((n,)), contig((n,), 2)
        rng = _rng(f"recip{v.n}")
        hs, hd = src_base(v, rng), dst_base(d, rng, False)
        ts, td = B.put(hs), B.put(hd)
        ref = LD(1) / hs[v.index()].astype(LD)
        rc = B.lib.ttk_recip(B.stream(), v.ptr(ts), d.ptr(td), v.n)
        after = B.get(td)
        outs = [("abi", after[d.index()]), ("dev", B.get(B.dev.recip(v.tensor(ts))))]
        if rc or not untouched(hd, after, [d]):
            bad.append(f"recip n={v.n}: status {rc} or a write outside the destination")
        for nm, got in outs:
            if not np.all(np.abs(got.astype(LD) - ref) <= 4.0 * U * np.abs(ref)):
                bad.append(f"recip n={v.n} [{nm}]: outside 4u |ref|")
    return bad


# ------------------------------------------------------------------------------------------- reductions
RED_N = (1, 63, 64, 65, 1023, 1024, 1025, 1500, 5000)


def _cancel(x):
    y = x.copy()
    y[x.size // 2:] *= -1.0
    return y


def _dot_cases():
    cs = [(f"n{n}", contig((n,)), contig((n,), 7), False) for n in RED_N]
    cs.append(("6d-small", gapped((3, 2, 4, 3, 2, 5)), permuted((3, 2, 4, 3, 2, 5), (4, 1, 5, 0, 3, 2)), False))
    cs.append(("6d-big", permuted(BIG, _P1), permuted(BIG, _P2, 5), False))
    cs.append(("bcast", _bcast(37), permuted((37, 37), (1, 0)), False))
    cs.append(("cancel-1500", contig((1500,)), contig((1500,), 1), True))
    cs.append(("cancel-big", contig((_prod(BIG),)), contig((_prod(BIG),), 1), True))
    cs.append(("0d", contig(()), contig((), 1), False))
    cs.append(("empty-1d", View((0,), (1,), 2, 4), View((0,), (1,), 1, 4), False))
    cs.append(("empty-3d", View((3, 0, 2), (0, 2, 1), 2, 4), View((3, 0, 2), (0, 2, 1), 1, 4), False))
    return cs


DOT = _dot_cases()


def run_dot(B, c):
    name, vx, vy, cancel = c
    rng = _rng("dot" + name)
    hx, hy = src_base(vx, rng), src_base(vy, rng)
    if cancel:
        hy[vy.index()] = _cancel(hx[vx.index()])
    tx, ty = B.put(hx), B.put(hy)
    hout = np.full(3, SENT)
    X, Y = hx[vx.index()].astype(LD), hy[vy.index()].astype(LD)
    ref, mag = np.sum(X * Y), float(np.sum(np.abs(X * Y)))
    bound = k1024(vx.n) * U * mag
    lib, D, st = B.lib, B.dev, B.stream()
    res, bad = {}, []
    nd, shp = len(vx.shape), _i64(vx.shape)
    if nd:  # ndim 0 goes through dev.* only
        out = ctypes.c_double(np.nan)
        rc = lib.ttk_dot_nd_sync(st, vx.ptr(tx), vy.ptr(ty), nd, shp, _i64(vx.strides), _i64(vy.strides),
                                 ctypes.byref(out))
        res["abi-sync"] = out.value
        tout = B.put(hout)
        rc |= lib.ttk_dot_nd_dev(st, vx.ptr(tx), vy.ptr(ty), nd, shp, _i64(vx.strides), _i64(vy.strides),
                                 tout.data_ptr() + 8)
        after = B.get(tout)
        res["abi-dev"] = after[1]
        if rc or not untouched(hout, after, [View((1,), (1,), 1, 3)]):
            bad.append(f"dot-{name}: status {rc} or a write beside the device scalar")
    res["dev.dot"] = D.dot(vx.tensor(tx), vy.tensor(ty))
    tout = B.put(hout)
    D.dot_into(vx.tensor(tx), vy.tensor(ty), tout[1:2])
    res["dev.dot_into"] = B.get(tout)[1]
    for k, v in res.items():
        if vx.n == 0:
            if not (v == 0.0):
                bad.append(f"dot-{name} [{k}]: {v!r} for an empty shape, expected 0.0")
        elif not abs(LD(v) - ref) <= bound:
            bad.append(f"dot-{name} [{k}]: |got - ref| = {float(abs(LD(v) - ref)):.3e} > {bound:.3e} "
                       f"(k = {k1024(vx.n)}, sum|xy| = {mag:.3e})")
    if len({np.float64(v).tobytes() for v in res.values()}) != 1:
        bad.append(f"dot-{name}: the routes disagree bit for bit: {res}")
    if cancel and not abs(float(ref)) < 1e-2 * mag:
        bad.append(f"dot-{name}: the input does not cancel")
    return bad


def _norm_cases():
    cs = [(f"n{n}", contig((n,)), False) for n in RED_N]
    cs.append(("permuted", permuted((7, 5, 9), (2, 0, 1)), False))
    cs.append(("6d", gapped((3, 2, 4, 3, 2, 5)), False))
    cs.append(("0d", contig(()), False))
    cs.append(("zero", contig((65,)), True))
    return cs


NORMALIZE = _norm_cases()


def run_normalize(B, c):
    name, vx, zero = c
    rng = _rng("normalize" + name)
    hx = src_base(vx, rng)
    if zero:
        hx[vx.index()] = 0.0
    vo = contig(vx.shape, 4)
    ho = dst_base(vo, rng, False)
    tx, to = B.put(hx), B.put(ho)
    X = hx[vx.index()].astype(LD)
    ref = X / np.sqrt(np.sum(X * X)) if not zero else None
    bound = (k1024(vx.n) / 2.0 + 10.0) * U * np.abs(ref) if not zero else None
    outs, bad = [], []
    if len(vx.shape):
        rc = B.lib.ttk_normalize(B.stream(), vx.ptr(tx), vo.ptr(to), len(vx.shape), _i64(vx.shape), _i64(vx.strides))
        after = B.get(to)
        if rc or not untouched(ho, after, [vo]):
            bad.append(f"normalize-{name}: status {rc} or a write outside the output")
        outs.append(("abi", after[vo.index()]))
    got = B.dev.normalized(vx.tensor(tx))
    if tuple(got.shape) != vx.shape or not got.is_contiguous():
        bad.append(f"normalize-{name}: dev.normalized returned shape {tuple(got.shape)}")
    outs.append(("dev", B.get(got.reshape(-1))))
    if not same_bits(B.get(tx), hx):
        bad.append(f"normalize-{name}: the input changed")
    for nm, g in outs:
        if zero:
            if np.any(np.isfinite(g)):
                bad.append(f"normalize-{name} [{nm}]: finite output for the zero vector")
        elif not np.all(np.abs(g.astype(LD) - ref) <= bound):
            bad.append(f"normalize-{name} [{nm}]: outside (k/2 + 10) u |ref|, k = {k1024(vx.n)}")
    if len(outs) == 2 and not same_bits(outs[0][1], outs[1][1]):
        bad.append(f"normalize-{name}: the two routes disagree bit for bit")
    return bad


def rayleigh_reference(v, Mv):
    """(ev, E_ev, wref, B, res2, bound on res2) of the module docstring"""
    n = v.size
    k = k1024(n)
    V, M = v.astype(LD), Mv.astype(LD)
    ev = np.sum(V * M)
    E = k * U * np.sum(np.abs(V * M))
    w = M - ev * V
    Bi = E * np.abs(V) * (1 + 3 * U) + 3 * U * (np.abs(ev * V) + np.abs(M))
    res2 = np.sum(w * w)
    b2 = k * U * np.sum((np.abs(w) + Bi) ** 2) + np.sum(2 * np.abs(w) * Bi + Bi * Bi)
    return ev, E, w, Bi, res2, b2


def run_rayleigh(B, n):
    rng = _rng(f"rayleigh{n}")
    vv, vm = contig((n,)), contig((n,), 5)
    hv = src_base(vv, rng)
    hv[vv.index()] /= np.sqrt(np.sum(hv[vv.index()] ** 2))
    hm = dst_base(vm, rng, True)
    hm[vm.index()] = 1.7 * hv[vv.index()] + 0.3 * hm[vm.index()]
    ev, E, w, Bi, res2, b2 = rayleigh_reference(hv[vv.index()], hm[vm.index()])
    lib, D = B.lib, B.dev
    tv = B.put(hv)
    res, bad = {}, []

    def finish(route, tm, e, r2):
        after = B.get(tm)
        if not untouched(hm, after, [vm]):
            bad.append(f"rayleigh n={n} [{route}]: wrote outside Mv")
        res[route] = (e, r2, after[vm.index()])

    tm = B.put(hm)
    e, r = ctypes.c_double(np.nan), ctypes.c_double(np.nan)
    rc = lib.ttk_rayleigh_tail_sync(B.stream(), vv.ptr(tv), vm.ptr(tm), n, ctypes.byref(e), ctypes.byref(r))
    finish("abi-sync", tm, e.value, r.value)
    tm, hout = B.put(hm), np.full(4, SENT)
    tout = B.put(hout)
    rc |= lib.ttk_rayleigh_tail_dev(B.stream(), vv.ptr(tv), vm.ptr(tm), n, tout.data_ptr() + 8)
    o = B.get(tout)
    if rc or not untouched(hout, o, [View((2,), (1,), 1, 4)]):
        bad.append(f"rayleigh n={n}: status {rc} or a write beside out2")
    finish("abi-dev", tm, o[1], o[2])
    tm = B.put(hm)
    e1, nr = D.rayleigh_tail_(vv.tensor(tv), vm.tensor(tm))
    finish("dev.rayleigh_tail_", tm, e1, None)
    if nr != float(np.sqrt(max(res["abi-sync"][1], 0.0))):
        bad.append(f"rayleigh n={n}: dev.rayleigh_tail_ returned {nr!r}, not sqrt of the synced res2")
    tm, tout = B.put(hm), B.put(hout)
    D.rayleigh_tail_into(vv.tensor(tv), vm.tensor(tm), tout[1:3])
    o = B.get(tout)
    finish("dev.rayleigh_tail_into", tm, o[1], o[2])
    if not same_bits(B.get(tv), hv):
        bad.append(f"rayleigh n={n}: v changed")
    first = res["abi-sync"]
    for route, (e, r2, mv) in res.items():
        if not abs(LD(e) - ev) <= E:
            bad.append(f"rayleigh n={n} [{route}]: ev off by {float(abs(LD(e) - ev)):.3e} > {float(E):.3e}")
        if not np.all(np.abs(mv.astype(LD) - w) <= Bi):
            bad.append(f"rayleigh n={n} [{route}]: updated Mv outside its bound")
        if r2 is not None and not abs(LD(r2) - res2) <= b2:
            bad.append(f"rayleigh n={n} [{route}]: res2 off by {float(abs(LD(r2) - res2)):.3e} > {float(b2):.3e}")
        if e != first[0] or (r2 is not None and r2 != first[1]) or not same_bits(mv, first[2]):
            bad.append(f"rayleigh n={n}: {route} and abi-sync disagree bit for bit")
    return bad


RANK_SCAN = [(n, nq) for n in (360, 1500) for nq in (1, 7)]


def run_rank_scan(B, n, nq):
    rng = _rng(f"rank_scan{n}-{nq}")
    vr, vn = contig((n,), 4), contig((nq, n))
    hr, hn = dst_base(vr, rng, True), src_base(vn, rng)
    r = hr[vr.index()].copy()
    G = hn[vn.index()].reshape(nq, n)
    sums, bounds = [], []
    for q in range(nq):  # the definition: one IEEE subtraction per element, then <r, r>
        r = r - G[q]
        R2 = r.astype(LD) ** 2
        sums.append(np.sum(R2))
        bounds.append(k1024(n) * U * np.sum(R2))
    bad = []
    tn = B.put(hn)
    for route in ("abi", "dev"):
        tr = B.put(hr)
        if route == "abi":
            out = np.full(nq + 2, SENT)
            rc = B.lib.ttk_rank_scan_sync(B.stream(), vr.ptr(tr), vn.ptr(tn), n, nq,
                                          ctypes.cast(out.ctypes.data + 8, c_dp))
            if rc or out[0:1].view(np.uint64)[0] != SENT_BITS or out[-1:].view(np.uint64)[0] != SENT_BITS:
                bad.append(f"rank_scan n={n} nq={nq}: status {rc} or a write beside host_out")
            out = out[1:-1]
        else:
            out = B.dev.rank_scan(vr.tensor(tr), vn.tensor(tn))
        after = B.get(tr)
        if not untouched(hr, after, [vr]):
            bad.append(f"rank_scan n={n} nq={nq} [{route}]: wrote outside res")
        if not same_bits(after[vr.index()], r):
            bad.append(f"rank_scan n={n} nq={nq} [{route}]: the residual is not bit-equal to the NumPy loop")
        for q in range(nq):
            if not abs(LD(out[q]) - sums[q]) <= bounds[q]:
                bad.append(f"rank_scan n={n} nq={nq} [{route}]: out[{q}] off by "
                           f"{float(abs(LD(out[q]) - sums[q])):.3e} > {float(bounds[q]):.3e}")
    if not same_bits(B.get(tn), hn):
        bad.append(f"rank_scan n={n} nq={nq}: negs changed")
    return bad


SUMSQ = [(n, nb) for n in (1, 255, 256, 257, 1000) for nb in (1, 5)]


def _sumsq_check(B, tag, hx, idx, call):
    """idx (nb, n): base indices of every batch's elements in summation order"""
    nb, n = idx.shape
    hout = np.full(nb + 2, SENT)
    tx, tout = B.put(hx), B.put(hout)
    rc = call(tx.data_ptr(), tout.data_ptr() + 8)
    after = B.get(tout)
    bad = []
    if rc or not untouched(hout, after, [View((nb,), (1,), 1, nb + 2)]) or not same_bits(B.get(tx), hx):
        bad.append(f"{tag}: status {rc}, a write beside out, or a changed input")
    for b in range(nb):
        X2 = hx[idx[b]].astype(LD) ** 2
        ref = np.sum(X2)
        if not abs(LD(after[1 + b]) - ref) <= k256(n) * U * ref:
            bad.append(f"{tag}: batch {b}: |got - ref| = {float(abs(LD(after[1 + b]) - ref)):.3e} > "
                       f"{float(k256(n) * U * ref):.3e}")
    return bad


def run_sumsq(B, n, nb):
    bstride = n + 5
    idx = 2 + np.arange(nb)[:, None] * bstride + np.arange(n)[None, :]
    hx = np.full(int(idx.max()) + 3, np.nan)
    hx[idx.reshape(-1)] = _rng(f"sumsq{n}-{nb}").standard_normal(idx.size)
    return _sumsq_check(B, f"sumsq_batched n={n} nb={nb}", hx, idx,
                        lambda x, o: B.lib.ttk_sumsq_batched(B.stream(), x + 16, n, nb, bstride, o))


SUMSQ2_INNER = (1, 7, 100, 255, 256, 257, 300)
SUMSQ2_OUTER = (1, 3, 11)
# (layout, nb): 'interleaved' is tt_als._block_sumsq's (bstride = inner, ostride = nb * inner); 'padded' adds a
# gap after every row of batches (ostride > nb * inner); 'batch-major' keeps each batch's rows together
SUMSQ2_LAYOUT = (("interleaved", 2), ("interleaved", 5), ("padded", 2), ("padded", 5), ("batch-major", 3))
assert min(SUMSQ2_INNER) < 256 < max(SUMSQ2_INNER) and 256 in SUMSQ2_INNER


def run_sumsq_strided(B, inner, outer, layout, nb):
    if layout == "interleaved":
        bstride, ostride = inner, nb * inner
    elif layout == "padded":
        bstride, ostride = inner, nb * inner + 3
    else:
        ostride = inner + 2
        bstride = outer * ostride + 1
    n = inner * outer
    i = np.arange(n)
    idx = 2 + np.arange(nb)[:, None] * bstride + ((i // inner) * ostride + i % inner)[None, :]
    assert np.unique(idx).size == idx.size
    hx = np.full(int(idx.max()) + 3, np.nan)
    hx[idx.reshape(-1)] = _rng(f"sumsq2-{inner}-{outer}-{layout}-{nb}").standard_normal(idx.size)
    return _sumsq_check(B, f"sumsq_batched_strided inner={inner} outer={outer} {layout} nb={nb}", hx, idx,
                        lambda x, o: B.lib.ttk_sumsq_batched_strided(B.stream(), x + 16, n, nb, bstride, inner,
                                                                     ostride, o))


# ------------------------------------------------------------------------------------------- assembly
_JOIN_RANKS = ((1, 1, 1, 1), (1, 3, 1, 2), (3, 1, 2, 1), (3, 4, 2, 5))
JOIN = [(mode, rk, mid) for mode in (0, 1, 2) for rk in _JOIN_RANKS for mid in (1, 4, 16)
        if (mode != 1 or rk[0] == rk[2]) and (mode != 2 or rk[1] == rk[3])]
JOIN_REJECTED = [(1, (3, 1, 2, 1), 4), (2, (1, 3, 1, 2), 4), (3, (1, 1, 1, 1), 4), (-1, (1, 1, 1, 1), 4),
                 (1, (3, 4, 2, 5), 1), (2, (3, 4, 2, 5), 1)]
assert any((rk[0] + rk[2]) * mid * (rk[1] + rk[3]) > 256 for mode, rk, mid in JOIN if mode == 0)


def join_reference(A, Bm, mode):
    (ra, mid, Ra), (rb, _, Rb) = A.shape, Bm.shape
    if mode == 0:
        o = np.zeros((ra + rb, mid, Ra + Rb))
        o[:ra, :, :Ra], o[ra:, :, Ra:] = A, Bm
        return o
    return np.concatenate([A, Bm], axis=2 if mode == 1 else 0)


def run_join(B, mode, rk, mid, rejected=False):
    ra, Ra, rb, Rb = rk
    tag = f"tt_join mode={mode} ranks={rk} mid={mid}"
    rng = _rng(tag)
    va, vb = contig((ra, mid, Ra)), contig((rb, mid, Rb), 2)
    ha, hb = src_base(va, rng), src_base(vb, rng)
    ro, Ro = (ra if mode == 1 else ra + rb), (Ra if mode == 2 else Ra + Rb)
    vo = contig((ro, mid, Ro), 4)
    ho = dst_base(vo, rng, False)
    ta, tb, to = B.put(ha), B.put(hb), B.put(ho)
    rc = B.lib.ttk_tt_join(B.stream(), va.ptr(ta), vb.ptr(tb), vo.ptr(to), ra, Ra, rb, Rb, mid, mode)
    after = B.get(to)
    if rejected:
        return [] if rc == ERR_ARG and same_bits(after, ho) else [f"{tag}: status {rc} (expected TTK_ERR_ARG) or a write"]
    bad = []
    if rc or not untouched(ho, after, [vo]):
        bad.append(f"{tag}: status {rc} or a write outside the output")
    ref = join_reference(ha[va.index()].reshape(va.shape), hb[vb.index()].reshape(vb.shape), mode)
    if not same_bits(after[vo.index()], ref.reshape(-1)):
        bad.append(f"{tag}: not the assembled core")
    return bad


COPY_MANY_N = (2, 32, 33, 70)
_SEG_LEN = (257, 0, 1, 255, 256, 1000)


def run_copy_many(B, n):
    tag = f"copy_many n={n}"
    rng = _rng(tag)
    counts = [_SEG_LEN[(j + n) % len(_SEG_LEN)] for j in range(n)]
    counts[-1] = counts[-1] or 3  # the last segment always copies something
    soff = np.cumsum([3] + [c + 2 for c in counts])[:-1]  # sources two NaNs apart
    doff = np.cumsum([4] + counts)[:-1]                   # destinations adjacent
    hs = np.full(int(soff[-1] + counts[-1] + 3), np.nan)
    for o, c in zip(soff, counts):
        hs[o:o + c] = rng.standard_normal(c)
    hd = np.full(4 + sum(counts) + 4, SENT)
    ts, td = B.put(hs), B.put(hd)
    vps = (ctypes.c_void_p * n)(*[ts.data_ptr() + 8 * int(o) for o in soff])
    vpd = (ctypes.c_void_p * n)(*[td.data_ptr() + 8 * int(o) for o in doff])
    rc = B.lib.ttk_copy_many(B.stream(), n, vps, vpd, _i64(counts))
    after = B.get(td)
    exp = hd.copy()
    for so, do, c in zip(soff, doff, counts):
        exp[do:do + c] = hs[so:so + c]
    bad = []
    if rc or not same_bits(after, exp) or not same_bits(B.get(ts), hs):
        wrong = [j for j, (do, c) in enumerate(zip(doff, counts)) if not same_bits(after[do:do + c], exp[do:do + c])]
        bad.append(f"{tag}: status {rc}; segments not copied exactly: {wrong}")
    srcs = [ts[int(o):int(o) + c] for o, c in zip(soff, counts)]
    outs = B.dev.clone_many(srcs)
    for j, (t, o) in enumerate(zip(srcs, outs)):
        if tuple(o.shape) != tuple(t.shape) or not same_bits(B.get(o), B.get(t)):
            bad.append(f"{tag}: dev.clone_many segment {j} differs")
            break
    return bad


ADD_DIAG = [(n, lda) for n in (1, 256, 257, 600) for lda in (n, n + 3)]


def run_add_diag(B, n, lda):
    tag = f"add_diag n={n} lda={lda}"
    rng = _rng(tag)
    v = View((n, n), (lda, 1), 3, (n - 1) * lda + n + 6)
    span = View(((n - 1) * lda + n,), (1,), 3, v.size)  # the pad columns between rows hold data too
    h = dst_base(span, rng, True)
    val = 0.8125 + 1e-3 * rng.standard_normal()
    exp = h.copy()
    di = 3 + np.arange(n) * (lda + 1)
    exp[di] = h[di] + val
    bad = []
    for route in ("abi", "dev"):
        t = B.put(h)
        if route == "abi":
            rc = B.lib.ttk_add_diag(B.stream(), v.ptr(t), n, lda, val)
        else:
            rc = 0
            B.dev.add_diag_(v.tensor(t), val)
        if rc or not same_bits(B.get(t), exp):
            bad.append(f"{tag} [{route}]: status {rc}, a diagonal entry that is not a + v, or a touched off-diagonal")
    return bad


FILL_N = (1, 257, _prod(BIG))


def run_fill(B, n):
    v = contig((n,), 5)
    h = dst_base(v, None, False)
    exp = h.copy()
    exp[v.index()] = -3.25
    bad = []
    for route in ("abi", "dev"):
        t = B.put(h)
        if route == "abi":
            rc = B.lib.ttk_fill(B.stream(), v.ptr(t), n, -3.25)
        else:
            rc = 0
            B.dev.fill_(v.tensor(t), -3.25)
        if rc or not same_bits(B.get(t), exp):
            bad.append(f"fill n={n} [{route}]: status {rc}, a missed element or a write outside")
    z = B.dev.zeros(3, n)
    if tuple(z.shape) != (3, n) or not same_bits(B.get(z.reshape(-1)), np.zeros(3 * n)):
        bad.append(f"fill n={n}: dev.zeros is not all +0.0")
    return bad


# ------------------------------------------------------------------------------------------- transfer
# 8192 doubles: the mapped buffer's first size; 65 536: the last size read through it
READ_N = (1, 255, 257, 8192, 8193, 16384, 16385, 65536, 65537, 5)


def run_read(B, route):
    """the reads in READ_N's order on one context: growing, across both thresholds, then small again"""
    bad = []
    rng = _rng("read")
    for n in READ_N:
        v = contig((n,), 3)
        hs = src_base(v, rng)
        ts = B.put(hs)
        if route == "abi":
            out = np.full(n + 4, SENT)
            rc = B.lib.ttk_read_sync(B.stream(), v.ptr(ts), ctypes.cast(out.ctypes.data + 16, c_dp), n)
            ok = rc == 0 and same_bits(out[2:-2], hs[3:3 + n]) and same_bits(out[[0, 1, -2, -1]], np.full(4, SENT))
        else:
            ok = same_bits(B.dev.read(v.tensor(ts)), hs[3:3 + n])
        if not ok:
            bad.append(f"read_sync n={n} [{route}]: not the device's doubles, or a write beside the host buffer")
    return bad


UPLOAD_SIZES = (1, 4095, 4096, 4097, 10000)
UPLOAD_COUNT = 70  # more than the ring's 64 slots: the first slots are reused, and regrown


def run_upload(B, route):
    rng = _rng("upload")
    host = np.empty(max(UPLOAD_SIZES))
    sent, tensors = [], []
    for j in range(UPLOAD_COUNT):
        n = UPLOAD_SIZES[j % len(UPLOAD_SIZES)]
        host[:] = rng.standard_normal(host.size)  # the one host array, overwritten between the calls
        sent.append(host[:n].copy())
        if route == "abi":
            t = B.put(np.full(n + 4, SENT))
            rc = B.lib.ttk_upload(B.stream(), host.ctypes.data, t.data_ptr() + 16, n)
            if rc:
                return [f"upload {j} (n={n}): status {rc}"]
        else:
            t = B.dev.from_numpy(host[:n])
        tensors.append(t)
    bad = []
    for j, (s, t) in enumerate(zip(sent, tensors)):
        exp = np.concatenate([[SENT] * 2, s, [SENT] * 2]) if route == "abi" else s
        if not same_bits(B.get(t), exp):
            bad.append(f"upload {j} (n={s.size}) [{route}]: the tensor does not hold what was sent")
    return bad
