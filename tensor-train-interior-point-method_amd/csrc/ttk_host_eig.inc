// Step-size eigen-ALS (`tt_max_generalised_eigen`, src/tt_als.py:1132-1283) orchestrated in C++.
//
// tt_eig.py runs the same algorithm as Python over libttk; its host side (~40 wrapper calls per
// two-site local solve, ~400 local solves per IPM iteration) costs about as much as the kernels on
// the small seeds (DESIGN.md §0).  This is the same sequence of libttk calls, with the same
// operands, views, strides and allocation shapes, in the same order -- bit-identical results
// (tests/test_gpu_step.py compares the two on the reference's recorded calls) -- with no Python in
// between and the GIL released for the whole call.
//
// Cases tt_eig.py handles off the dense path (the LOBPCG branch at r*R > size_limit, the dense-size
// cap, the ZeroDivisionError of a zero step) and any libttk failure make this return a non-zero
// status with nothing visible changed: the input cores are never written, the random state is only
// returned on success, and the caller reruns the call in Python from the same state (which then
// takes that branch, or raises what the Python path raises).
//
// Included inside ttk_host_bind.cpp's anonymous namespace (uses its einsum / copy_ / axpby /
// normalized packers and the thread's launch stream g_stream).

namespace eig {

using svd_work_fn = int64_t (*)(int, int);
using svd_tol_fn = int (*)(void *, const double *, int, int, double *, double *, double *, double *, double);
using svd_read_fn = int (*)(void *, const double *, int, int, double *, double *, double *, double *, double,
                            double *);
using qr_work_fn = int64_t (*)(int, int);
using qr_fn = int (*)(void *, const double *, int, int, double *, double *, double *);
using syev_work_fn = int64_t (*)(int);
using syev_fn = int (*)(void *, const double *, int, int, double *, double *, double *);
using read_fn = int (*)(void *, const double *, double *, int64_t);
using upload_fn = int (*)(void *, const double *, double *, int64_t);
using chol_fn = int (*)(void *, double *, int);
using trsm_fn = int (*)(void *, const double *, int, double *, int, int, int);
using ray_dev_fn = int (*)(void *, const double *, double *, int64_t, double *);
using ray_sync_fn = int (*)(void *, const double *, double *, int64_t, double *, double *);
using batch_fn = int (*)(void *);
using split_kick_lds_fn = int64_t (*)(int, int, int, int, int, int, int64_t *);
using split_kick_fn = int (*)(void *, int, int, int, int, int, int, const double *, const double *, const double *,
                              const double *, double *, double *);
using trunc_kick_lds_fn = int64_t (*)(int, int, int, int, int, int64_t *);
using trunc_kick_fn = int (*)(void *, int, int, int, int, int, double, int, const double *, const double *, double *,
                              double *, double *);

struct Fns {
  svd_work_fn svd_work = nullptr;
  svd_tol_fn svd_tol = nullptr;
  svd_read_fn svd_read = nullptr;  // ttk_svd_tol_read (optional 15th address)
  qr_work_fn qr_work = nullptr;
  qr_fn qr = nullptr;
  syev_work_fn syev_work = nullptr;
  syev_fn syev = nullptr;
  read_fn read = nullptr;
  upload_fn upload = nullptr;
  chol_fn chol = nullptr;
  trsm_fn trsm = nullptr;
  ray_dev_fn ray_dev = nullptr;
  ray_sync_fn ray_sync = nullptr;
  batch_fn batch_begin = nullptr, batch_end = nullptr;
  split_kick_lds_fn split_kick_lds = nullptr;  // ttk_split_kick_lds, ttk_split_kick (optional 16th, 17th address)
  split_kick_fn split_kick = nullptr;
  // ttk_trunc_kick_lds, ttk_trunc_kick, ttk_trunc_kick_read (optional 18th to 20th address)
  trunc_kick_lds_fn trunc_kick_lds = nullptr;
  trunc_kick_fn trunc_kick = nullptr, trunc_kick_read = nullptr;
} F;

// ---------------------------------------------------------------- NumPy's legacy Gaussian stream
// RandomState.randn: MT19937 (numpy/random/src/mt19937), doubles from two 32-bit draws (53 bits),
// Marsaglia's polar method keeping the second value (legacy_gauss).  State in and out as
// RandomState.get_state() gives it: key[624], pos, has_gauss, cached_gaussian.
struct MT {
  uint32_t key[624];
  int pos = 624;
  int has_gauss = 0;
  double gauss = 0.0;

  void regen() {
    constexpr int n = 624, m = 397;
    constexpr uint32_t hi = 0x80000000u, lo = 0x7fffffffu, mat = 0x9908b0dfu;
    int i = 0;
    for (; i < n - m; ++i) {
      const uint32_t y = (key[i] & hi) | (key[i + 1] & lo);
      key[i] = key[i + m] ^ (y >> 1) ^ ((0u - (y & 1u)) & mat);
    }
    for (; i < n - 1; ++i) {
      const uint32_t y = (key[i] & hi) | (key[i + 1] & lo);
      key[i] = key[i + m - n] ^ (y >> 1) ^ ((0u - (y & 1u)) & mat);
    }
    const uint32_t y = (key[n - 1] & hi) | (key[0] & lo);
    key[n - 1] = key[m - 1] ^ (y >> 1) ^ ((0u - (y & 1u)) & mat);
    pos = 0;
  }
  uint32_t next32() {
    if (pos >= 624) regen();
    uint32_t y = key[pos++];
    y ^= (y >> 11);
    y ^= (y << 7) & 0x9d2c5680u;
    y ^= (y << 15) & 0xefc60000u;
    y ^= (y >> 18);
    return y;
  }
  double next_double() {
    const int32_t a = (int32_t)(next32() >> 5), b = (int32_t)(next32() >> 6);
    return (a * 67108864.0 + b) / 9007199254740992.0;
  }
  double next_gauss() {
    if (has_gauss) {
      const double t = gauss;
      has_gauss = 0;
      gauss = 0.0;
      return t;
    }
    double x1, x2, r2;
    do {
      x1 = 2.0 * next_double() - 1.0;
      x2 = 2.0 * next_double() - 1.0;
      r2 = x1 * x1 + x2 * x2;
    } while (r2 >= 1.0 || r2 == 0.0);
    const double f = std::sqrt(-2.0 * std::log(r2) / r2);
    gauss = f * x1;
    has_gauss = 1;
    return f * x2;
  }
};

// ---------------------------------------------------------------- host rules restated
// T.prune_singular_vals (cy_src/tt_ops_cy.pyx:161-177): smallest r whose discarded tail has
// squared norm < eps^2 (tail sums accumulated from the last value, as np.cumsum over s[::-1])
int64_t prune(const double *s, int64_t n, double eps) {
  bool zero = true;
  for (int64_t i = 0; i < n; ++i)
    if (s[i] * s[i] != 0.0) zero = false;
  if (zero) return 1;
  const double e2 = eps * eps;
  std::vector<double> sc((size_t)n);
  double c = 0.0;
  for (int64_t j = n - 1; j >= 0; --j) {
    c = c + std::fabs(s[j]) * std::fabs(s[j]);
    sc[(size_t)j] = c;
  }
  int64_t r = 0;
  for (int64_t j = 0; j < n; ++j)
    if (sc[(size_t)j] < e2) {
      r = j;
      break;
    }
  r = std::max<int64_t>(r, 1);
  if (sc[(size_t)n - 1] > e2) r = n;
  return r;
}

// Python's min(a, b) / max(a, b) (the first argument unless the second compares strictly
// smaller / larger: NaN operands keep the first)
double pymin(double a, double b) { return b < a ? b : a; }
double pymax(double a, double b) { return b > a ? b : a; }

// np.max over the residual table (NaN propagates)
double npmax(const std::vector<double> &v) {
  double m = -INFINITY;
  for (double x : v) {
    if (std::isnan(x)) return x;
    if (x > m) m = x;
  }
  return m;
}

struct Bail {};     // a case the Python path handles: status 1, rerun there
struct GenFail {};  // _gen_max_eig raised (not positive definite, or 1/lam at lam = 0)

// ---------------------------------------------------------------- device ops (dev.py's wrappers)
struct Ops {
  at::TensorOptions opt;
  int batch = 0;
  std::vector<at::Tensor> keep;  // operands and outputs of recorded batch steps, until the batch ends

  void ok(int rc, const char *what) { check(rc, what); }
  at::Tensor emp(at::IntArrayRef shape) { return at::empty(shape, opt); }

  at::Tensor E(const std::string &eq, std::vector<at::Tensor> ops, int64_t flags = 0) {
    if (batch) {  // dev.einsum inside einsum_batch: output allocated up front, kept to the flush
      const OutMap &m = out_map(eq);
      std::vector<int64_t> shp(m.src.size());
      for (size_t i = 0; i < m.src.size(); ++i) shp[i] = ops[m.src[i].first].size(m.src[i].second);
      at::Tensor out = emp(shp);
      for (auto &o : ops) keep.push_back(o);
      keep.push_back(out);
      return einsum_impl(eq, ops, out, 1.0, 0.0, flags, false);
    }
    return einsum_impl(eq, ops, c10::nullopt, 1.0, 0.0, flags, false);
  }
  void begin() {
    ok(F.batch_begin(g_stream), "einsum_batch_begin");
    ++batch;
  }
  void end() {
    --batch;
    ok(F.batch_end(g_stream), "einsum_batch_end");
    if (!batch) keep.clear();
  }
  at::Tensor matmul(const at::Tensor &a, const at::Tensor &b) { return E("ik,kj->ij", {a, b}); }
  at::Tensor clone(const at::Tensor &t) {
    at::Tensor o = emp(t.sizes());
    return copy_(o, t, 1.0, 0.0);
  }
  at::Tensor scaled(const at::Tensor &t, double a) {
    at::Tensor o = emp(t.sizes());
    return copy_(o, t, a, 0.0);
  }
  at::Tensor contig(const at::Tensor &t) { return t.is_contiguous() ? t : clone(t); }
  std::vector<double> read(const at::Tensor &t0) {
    at::Tensor t = t0.contiguous();
    std::vector<double> h((size_t)t.numel());
    if (t.numel()) ok(F.read(g_stream, t.data_ptr<double>(), h.data(), t.numel()), "read");
    return h;
  }
  at::Tensor upload(const std::vector<double> &h, at::IntArrayRef shape) {
    at::Tensor o = emp(shape);
    if (!h.empty()) ok(F.upload(g_stream, h.data(), o.data_ptr<double>(), (int64_t)h.size()), "upload");
    return o;
  }

  struct SVD {
    at::Tensor U, S, Vt;
    std::vector<double> s;
  };
  SVD svd(at::Tensor A, bool host, c10::optional<at::Tensor> S_out) {
    A = A.contiguous();
    const int m = (int)A.size(0), n = (int)A.size(1), k = std::min(m, n);
    SVD r;
    r.U = emp({m, k});
    r.S = S_out.has_value() ? *S_out : emp({k});
    r.Vt = emp({k, n});
    at::Tensor work = emp({F.svd_work(m, n)});
    if (host && F.svd_read) {  // dev.svd(host=True): the SVD and its read of S in one call
      r.s.assign((size_t)k, 0.0);
      ok(F.svd_read(g_stream, A.data_ptr<double>(), m, n, r.U.data_ptr<double>(), r.S.data_ptr<double>(),
                    r.Vt.data_ptr<double>(), work.data_ptr<double>(), 0.0, r.s.data()),
         "svd");
      return r;
    }
    ok(F.svd_tol(g_stream, A.data_ptr<double>(), m, n, r.U.data_ptr<double>(), r.S.data_ptr<double>(),
                 r.Vt.data_ptr<double>(), work.data_ptr<double>(), 0.0),
       "svd");
    if (host) r.s = read(r.S);
    return r;
  }
  std::pair<at::Tensor, at::Tensor> qr(at::Tensor A) {
    A = A.contiguous();
    const int m = (int)A.size(0), n = (int)A.size(1), k = std::min(m, n);
    at::Tensor Q = emp({m, k}), R = emp({k, n});
    at::Tensor work = emp({F.qr_work(m, n)});
    ok(F.qr(g_stream, A.data_ptr<double>(), m, n, Q.data_ptr<double>(), R.data_ptr<double>(),
            work.data_ptr<double>()),
       "qr");
    return {Q, R};
  }
  std::unordered_map<int64_t, at::Tensor> anti;  // dev._anti_identity's cache (exact 0 / 1 values)
  at::Tensor anti_identity(int64_t n) {
    auto it = anti.find(n);
    if (it != anti.end()) return it->second;
    std::vector<double> h((size_t)(n * n), 0.0);
    for (int64_t i = 0; i < n; ++i) h[(size_t)(i * n + (n - 1 - i))] = 1.0;
    at::Tensor t = upload(h, {n, n});
    anti.emplace(n, t);
    return t;
  }
  // dev.rq: M = R Q via QR of the row-reversed transpose
  std::pair<at::Tensor, at::Tensor> rq(const at::Tensor &M) {
    const int64_t p = M.size(0), q = M.size(1), k = std::min(p, q);
    at::Tensor Jp = anti_identity(p), Jk = anti_identity(k);
    auto QR = qr(E("ji,jk->ik", {M, Jp}));
    at::Tensor R = E("ij,lj,lk->ik", {Jp, QR.second, Jk});
    at::Tensor Q = E("ij,lj->il", {Jk, QR.first});
    return {R, Q};
  }
  // dev.syev_extreme: (eigenvalue, vector); with lam_out the eigenvalue stays on the device (NaN here)
  std::pair<double, at::Tensor> syev_extreme(at::Tensor A, bool largest, c10::optional<at::Tensor> lam_out) {
    A = A.contiguous();
    const int n = (int)A.size(0);
    at::Tensor buf, lam_p, vec;
    if (lam_out.has_value()) {
      lam_p = *lam_out;
      vec = emp({n});
    } else {
      buf = emp({n + 1});
      lam_p = buf.slice(0, 0, 1);
      vec = buf.slice(0, 1, n + 1);
    }
    at::Tensor work = emp({F.syev_work(n)});
    ok(F.syev(g_stream, A.data_ptr<double>(), n, largest ? 1 : 0, lam_p.data_ptr<double>(), vec.data_ptr<double>(),
              work.data_ptr<double>()),
       "syev_extreme");
    if (lam_out.has_value()) return {NAN, vec};
    const double lam = read(buf.slice(0, 0, 1))[0];
    return {lam, vec};
  }
  // dev.trsm_: B <- op(L)^-1 B (any failure is _gen_max_eig's exception)
  void trsm(const at::Tensor &L, at::Tensor B, bool trans) {
    if (F.trsm(g_stream, L.data_ptr<double>(), (int)L.size(0), B.data_ptr<double>(), (int)B.size(1), (int)B.stride(0),
               trans ? 1 : 0))
      throw GenFail{};
  }
};

// ---------------------------------------------------------------- the eigen-ALS (tt_eig.py)
const char *TWO_SITE = "lsr,smnk,kptS,LSR->lmpLrntR";
const char *ONE_SITE = "lsr,smnS,LSR->lmLrnR";
const char *APPLY = "lsr,smnS,LSR,rnR->lmL";

struct Res {  // a local residual: a value, or a slot of the deferred buffer
  double v = INFINITY;
  int slot = -1;
};

struct Solver {
  Ops o;
  MT mt;
  double tol = 1e-8, trunc_tol = 0.0;
  int64_t size_limit = 256, max_rank = 1, max_dense = 4096;
  bool split_kick = false;  // dev.SPLIT_KICK as this call found it
  bool trunc_kick = false;  // dev.TRUNC_KICK as this call found it
  // _Deferred: (ev, ||r||^2) per dense local solve of a half-sweep, read once after it
  at::Tensor dbuf;
  int dn = 0;
  bool skip = false;  // _ET.defer == "skip" (finish sweeps: residuals discarded)
  std::vector<std::tuple<int, int, int>> pending;

  at::Tensor sym(const at::Tensor &Mt, int64_t m) {
    at::Tensor M = Mt.view({m, m});
    return axpby(M.t(), M, 0.5, 0.5, 1.0, c10::nullopt);
  }
  at::Tensor shifted(const at::Tensor &Am, const at::Tensor &Dm, double step) {
    return axpby(Dm, Am, 1.0, 1.0, 1.0 / step, c10::nullopt);
  }

  std::pair<double, at::Tensor> gen_max_eig(const at::Tensor &Dm, const at::Tensor &Am) {
    const int64_t m = Am.size(0);
    at::Tensor L = o.clone(Am);
    if (F.chol(g_stream, L.data_ptr<double>(), (int)m)) throw GenFail{};
    at::Tensor C = o.scaled(Dm, -1.0);
    o.trsm(L, C, false);
    at::Tensor Ct = o.clone(C.t());
    o.trsm(L, Ct, false);
    at::Tensor S = o.clone(Ct);
    copy_(S, Ct.t(), 0.5, 0.5);
    auto lw = o.syev_extreme(S, true, c10::nullopt);
    at::Tensor y = lw.second.view({m, 1});
    o.trsm(L, y, true);
    return {lw.first, y.view({-1})};
  }

  Res rayleigh_now(const at::Tensor &Am, const at::Tensor &Dm, double step, const at::Tensor &v) {
    at::Tensor M = shifted(Am, Dm, step);
    at::Tensor Mv = o.matmul(M, v.view({-1, 1})).view({-1});
    double ev = 0.0, r2 = 0.0;
    o.ok(F.ray_sync(g_stream, v.data_ptr<double>(), Mv.data_ptr<double>(), v.numel(), &ev, &r2), "rayleigh_tail");
    Res r;
    r.v = std::sqrt(std::max(r2, 0.0));
    return r;
  }
  Res rayleigh_deferred(const at::Tensor &Am, const at::Tensor &Dm, double step, const at::Tensor &v) {
    at::Tensor M = shifted(Am, Dm, step);
    at::Tensor Mv = o.matmul(M, v.view({-1, 1})).view({-1});
    if (dn * 2 + 2 > dbuf.numel()) return rayleigh_now(Am, Dm, step, v);
    o.ok(F.ray_dev(g_stream, v.data_ptr<double>(), Mv.data_ptr<double>(), v.numel(),
                   dbuf.data_ptr<double>() + 2 * dn),
         "rayleigh_tail_dev");
    Res r;
    r.slot = dn++;
    return r;
  }
  void put(std::vector<double> &res, int64_t cols, int i, int j, const Res &r) {
    if (r.slot >= 0)
      pending.emplace_back(i, j, r.slot);
    else
      res[(size_t)(i * cols + j)] = r.v;
  }
  void resolve(std::vector<double> &res, int64_t cols) {
    if (!pending.empty()) {
      std::vector<double> h = o.read(dbuf.slice(0, 0, 2 * dn));
      for (auto &p : pending)
        res[(size_t)(std::get<0>(p) * cols + std::get<1>(p))] =
            std::sqrt(std::max(h[(size_t)(2 * std::get<2>(p) + 1)], 0.0));
    }
    pending.clear();
    dn = 0;
  }

  // dev.trunc_kick's result: the two output buffers and the info block on the device
  struct TK {
    at::Tensor s1, s2, info;
  };
  // the caller's truncation SVD, enqueued behind the eigensolve (tt_eig._dense_step's `post`); tk instead: the
  // caller's whole tail (ttk_trunc_kick), which takes the eigenvector as the solver left it
  using PostFn = std::function<Ops::SVD(const at::Tensor &, const at::Tensor &)>;
  using PostTk = std::function<TK(const at::Tensor &, const at::Tensor &)>;
  struct Post {
    int64_t k;
    PostFn fn;
    PostTk tk;
  };
  struct StepOut {
    at::Tensor sol;
    double step;
    Res res;
    bool has_pre = false;
    Ops::SVD pre;
    bool has_tk = false;
    TK tk;
    std::vector<double> tkinfo;  // the info block as read with the eigenvalue
  };

  // tt_eig._dense_step (src/tt_als.py:957-996,1060-1101)
  StepOut dense_step(const at::Tensor &prev, const at::Tensor &Am, const at::Tensor &Dm, double step, double eps,
                     bool two_site, const Post *post) {
    at::Tensor M = shifted(Am, Dm, step);
    StepOut out;
    double ev;
    at::Tensor sol;
    if (post) {
      at::Tensor comb = o.emp({1 + post->k});
      sol = o.syev_extreme(M, false, comb.slice(0, 0, 1)).second;
      if (post->tk) {
        TK t = post->tk(sol, comb.slice(0, 1, 1 + post->k));
        std::vector<double> h = o.read(comb);
        ev = h[0];
        if (!(ev < 0)) {
          out.tkinfo.assign(h.begin() + 1, h.end());
          out.tk = std::move(t);
          out.has_tk = true;
        }
      } else {
        if (two_site) sol = normalized(sol);
        Ops::SVD p = post->fn(sol, comb.slice(0, 1, 1 + post->k));
        std::vector<double> h = o.read(comb);
        ev = h[0];
        if (!(ev < 0)) {
          p.s.assign(h.begin() + 1, h.end());
          out.pre = std::move(p);
          out.has_pre = true;
        }
      }
    } else {
      auto r = o.syev_extreme(M, false, c10::nullopt);
      ev = r.first;
      sol = r.second;
      if (two_site) sol = normalized(sol);
    }
    if (ev < 0) {
      try {
        auto g = gen_max_eig(Dm, Am);
        sol = g.second;
        if (g.first == 0.0) throw GenFail{};  // 1 / lam raises
        step = pymax(0.0, pymin(step, 1.0 / g.first));
      } catch (const GenFail &) {
        sol = prev;
        step *= (1 - eps);
      } catch (const std::exception &) {
        sol = prev;
        step *= (1 - eps);
      }
    }
    out.sol = sol;
    out.step = step;
    if (skip) {  // residual discarded; 1 / step raises at step 0
      if (step == 0.0) throw Bail{};
      return out;
    }
    if (step == 0.0) throw Bail{};  // A / step in the residual raises ZeroDivisionError
    out.res = rayleigh_deferred(Am, Dm, step, prev);
    return out;
  }

  Ops::SVD split_svd(const at::Tensor &sol, const std::array<int64_t, 4> &sh, bool bwd,
                     c10::optional<at::Tensor> S_out) {
    const int64_t a = sh[0] * sh[1], b = sh[2] * sh[3];
    at::Tensor mat = bwd ? o.clone(sol.view({a, b}).t()) : sol.view({a, b});
    return o.svd(mat, !S_out.has_value(), S_out);
  }

  struct Kick {
    at::Tensor a, b;
    int64_t r;
  };
  at::Tensor gauss(int64_t rows, int64_t cols) {  // RandomState.randn(rows, cols), uploaded
    std::vector<double> h((size_t)(rows * cols));
    for (auto &e : h) e = mt.next_gauss();
    return o.upload(h, {rows, cols});
  }
  // src/tt_als.py:1041-1046; uk0: the Gaussian block when already drawn
  Kick kick(const at::Tensor &u, const at::Tensor &v, int64_t r_add, const at::Tensor &uk0) {
    const int64_t old = u.size(-1), rows = u.size(0);
    at::Tensor uk = uk0.defined() ? uk0 : gauss(rows, r_add);
    at::Tensor cat = o.emp({rows, old + r_add});
    copy_(cat.slice(1, 0, old), u, 1.0, 0.0);
    copy_(cat.slice(1, old, old + r_add), uk, 1.0, 0.0);
    auto QR = o.qr(cat);
    return {QR.first, o.matmul(QR.second.slice(1, 0, old), v), QR.first.size(-1)};
  }
  // src/tt_als.py:1048-1053; uk0 as in kick
  Kick kick_rev(const at::Tensor &u, const at::Tensor &v, int64_t r_add, const at::Tensor &uk0) {
    const int64_t old = v.size(0), cols = v.size(-1);
    at::Tensor uk = uk0.defined() ? uk0 : gauss(r_add, cols);
    at::Tensor cat = o.emp({old + r_add, cols});
    copy_(cat.slice(0, 0, old), v, 1.0, 0.0);
    copy_(cat.slice(0, old, old + r_add), uk, 1.0, 0.0);
    auto RQ = o.rq(cat);
    return {o.matmul(u, RQ.first.slice(0, 0, old)), RQ.second, RQ.second.size(0)};
  }

  std::pair<at::Tensor, at::Tensor> split(const at::Tensor &sol, const std::array<int64_t, 4> &sh, bool bwd,
                                          const Ops::SVD *pre) {
    Ops::SVD p = pre ? *pre : split_svd(sol, sh, bwd, c10::nullopt);
    at::Tensor G;
    if (split_kick && F.split_kick && F.split_kick_lds) {  // tt_eig._split under dev.SPLIT_KICK: one launch
      const int64_t r = std::min(prune(p.s.data(), (int64_t)p.s.size(), trunc_tol), max_rank);
      const int a = (int)(sh[0] * sh[1]), b = (int)(sh[2] * sh[3]), pp = (int)p.U.size(1);
      int64_t q = 0;
      if (F.split_kick_lds(bwd ? 1 : 0, a, b, pp, (int)r, 4, &q) >= 0) {
        G = bwd ? gauss(4, b) : gauss(a, 4);
        if (p.U.is_contiguous() && p.S.is_contiguous() && p.Vt.is_contiguous()) {
          at::Tensor s1 = o.emp({a, q}), s2 = o.emp({q, b});
          // a null context: the one dev._stream() bound to this thread
          o.ok(F.split_kick(nullptr, bwd ? 1 : 0, a, b, pp, (int)r, 4, p.U.data_ptr<double>(), p.S.data_ptr<double>(),
                            p.Vt.data_ptr<double>(), G.data_ptr<double>(), s1.data_ptr<double>(),
                            s2.data_ptr<double>()),
               "split_kick");
          return {s1.view({sh[0], sh[1], q}), s2.view({q, sh[2], sh[3]})};
        }
      }
    }
    if (bwd) {
      at::Tensor v = o.E("r,rj->rj", {p.S, p.Vt});
      const int64_t r = std::min(prune(p.s.data(), (int64_t)p.s.size(), trunc_tol), max_rank);
      Kick k = kick_rev(v.slice(0, 0, r).t(), p.U.slice(1, 0, r).t(), 4, G);
      return {o.contig(k.a).view({sh[0], sh[1], k.r}), o.contig(k.b).view({k.r, sh[2], sh[3]})};
    }
    const int64_t r = std::min(prune(p.s.data(), (int64_t)p.s.size(), trunc_tol), max_rank);
    at::Tensor s2 = o.E("r,rj->rj", {p.S.slice(0, 0, r), p.Vt.slice(0, 0, r)});
    Kick k = kick(p.U.slice(1, 0, r), s2, 4, G);
    return {o.contig(k.a).view({sh[0], sh[1], k.r}), o.contig(k.b).view({k.r, sh[2], sh[3]})};
  }

  // tt_eig._trunc_kick_fits: the output bound of ttk_trunc_kick where this split takes it, else -1
  int64_t tk_qmax(const std::array<int64_t, 4> &sh, bool bwd) {
    if (!trunc_kick || !F.trunc_kick || !F.trunc_kick_read || !F.trunc_kick_lds) return -1;
    int64_t q = 0;
    if (F.trunc_kick_lds(bwd ? 1 : 0, (int)(sh[0] * sh[1]), (int)(sh[2] * sh[3]), 4, (int)max_rank, &q) < 0) return -1;
    return q;
  }
  // dev.trunc_kick: one launch, no read; info into info_out when given
  TK tk_call(const at::Tensor &M, const std::array<int64_t, 4> &sh, bool bwd, int unit, const at::Tensor &G,
             int64_t qmax, c10::optional<at::Tensor> info_out) {
    const int64_t a = sh[0] * sh[1], b = sh[2] * sh[3];
    TK t{o.emp({a * qmax}), o.emp({qmax * b}), info_out.has_value() ? *info_out : o.emp({4 + std::min(a, b)})};
    // a null context: the one dev._stream() bound to this thread
    o.ok(F.trunc_kick(nullptr, bwd ? 1 : 0, (int)a, (int)b, 4, unit, trunc_tol, (int)max_rank, M.data_ptr<double>(),
                      G.data_ptr<double>(), t.s1.data_ptr<double>(), t.s2.data_ptr<double>(),
                      t.info.data_ptr<double>()),
         "trunc_kick");
    return t;
  }
  // dev.trunc_kick_views on the info block as read back
  std::pair<at::Tensor, at::Tensor> tk_views(const TK &t, const std::vector<double> &info,
                                             const std::array<int64_t, 4> &sh) {
    const int64_t a = sh[0] * sh[1], b = sh[2] * sh[3], q = (int64_t)info[1];
    return {t.s1.slice(0, 0, a * q).view({sh[0], sh[1], q}), t.s2.slice(0, 0, q * b).view({q, sh[2], sh[3]})};
  }
  // tt_eig._trunc_split: ttk_trunc_kick_read, the call with its info read in it
  std::pair<at::Tensor, at::Tensor> tk_split(const at::Tensor &sol, const std::array<int64_t, 4> &sh, bool bwd,
                                             int unit, const at::Tensor &G, int64_t qmax) {
    const int64_t a = sh[0] * sh[1], b = sh[2] * sh[3];
    at::Tensor M = o.contig(sol);
    TK t{o.emp({a * qmax}), o.emp({qmax * b}), at::Tensor()};
    std::vector<double> info((size_t)(4 + std::min(a, b)));
    o.ok(F.trunc_kick_read(nullptr, bwd ? 1 : 0, (int)a, (int)b, 4, unit, trunc_tol, (int)max_rank,
                           M.data_ptr<double>(), G.data_ptr<double>(), t.s1.data_ptr<double>(),
                           t.s2.data_ptr<double>(), info.data()),
         "trunc_kick");
    return tk_views(t, info, sh);
  }

  struct Local {
    at::Tensor s1, s2;
    double step;
    Res res;
  };
  // tt_eig._step_size_local_solve (src/tt_als.py:931-1038), dense branch
  Local local_solve(const at::Tensor &p1, const at::Tensor &p2, const at::Tensor &XAX_k, const at::Tensor &A_k,
                    const at::Tensor &A_kp1, const at::Tensor &XAX_k2, const at::Tensor &XDX_k, const at::Tensor &D_k,
                    const at::Tensor &D_kp1, const at::Tensor &XDX_k2, double step, bool bwd) {
    if (!std::isfinite(step) || step <= 0) {
      Local l{p1, p2, 0.0, Res{}};
      return l;
    }
    at::Tensor prev = o.E("rny,ytR->rntR", {p1, p2});
    const std::array<int64_t, 4> sh{prev.size(0), prev.size(1), prev.size(2), prev.size(3)};
    const int64_t m = sh[0] * sh[1] * sh[2] * sh[3];
    if (!(sh[0] * sh[3] <= size_limit) || m > max_dense) throw Bail{};  // LOBPCG branch / dense cap
    at::Tensor pv = prev.view({-1});
    o.begin();
    at::Tensor Dr = o.E(TWO_SITE, {XDX_k, D_k, D_kp1, XDX_k2});
    at::Tensor Ar = o.E(TWO_SITE, {XAX_k, A_k, A_kp1, XAX_k2});
    o.end();
    at::Tensor Dm = sym(Dr, m), Am = sym(Ar, m);
    const int64_t qmax = tk_qmax(sh, bwd);
    if (qmax >= 0) {  // tt_eig._step_size_local_solve under dev.TRUNC_KICK: the block first, then the whole tail
      at::Tensor G = bwd ? gauss(4, sh[2] * sh[3]) : gauss(sh[0] * sh[1], 4);
      Post post{4 + std::min(sh[0] * sh[1], sh[2] * sh[3]), nullptr,
                [&](const at::Tensor &v, const at::Tensor &info) { return tk_call(v, sh, bwd, 1, G, qmax, info); }};
      StepOut so = dense_step(pv, Am, Dm, step, tol, true, &post);
      auto s = so.has_tk ? tk_views(so.tk, so.tkinfo, sh) : tk_split(so.sol, sh, bwd, 1, G, qmax);
      return {s.first, s.second, so.step, so.res};
    }
    Post post{std::min(sh[0] * sh[1], sh[2] * sh[3]),
              [&](const at::Tensor &v, const at::Tensor &S_out) { return split_svd(normalized(v), sh, bwd, S_out); },
              nullptr};
    StepOut so = dense_step(pv, Am, Dm, step, tol, true, &post);
    if (so.has_pre) {
      auto s = split(at::Tensor(), sh, bwd, &so.pre);
      return {s.first, s.second, so.step, so.res};
    }
    at::Tensor sol = normalized(so.sol);
    auto s = split(sol, sh, bwd, nullptr);
    return {s.first, s.second, so.step, so.res};
  }

  // tt_eig._step_size_local_solve_last (src/tt_als.py:1056-1129), dense branch
  StepOut local_last(const at::Tensor &prev, const at::Tensor &XDX_k, const at::Tensor &Dk, const at::Tensor &XDX_k1,
                     const at::Tensor &XAX_k, const at::Tensor &Ak, const at::Tensor &XAX_k1, bool dense, double step,
                     const Post *post) {
    if (!std::isfinite(step) || step <= 0) {
      StepOut so;
      so.sol = prev.is_contiguous() ? prev.reshape({-1}) : o.clone(prev).view({-1});
      so.step = 0.0;
      return so;
    }
    const int64_t m = prev.numel();
    at::Tensor pv = o.contig(prev).view({-1});
    if (!dense || m > max_dense) throw Bail{};
    o.begin();
    at::Tensor Dr = o.E(ONE_SITE, {XDX_k, Dk, XDX_k1});
    at::Tensor Ar = o.E(ONE_SITE, {XAX_k, Ak, XAX_k1});
    o.end();
    at::Tensor Dm = sym(Dr, m), Am = sym(Ar, m);
    return dense_step(pv, Am, Dm, step, tol, false, post);
  }

  at::Tensor phi_bck(const at::Tensor &P, const at::Tensor &x, const at::Tensor &A) {  // src/tt_als.py:252-253
    return o.E(APPLY, {x, A.permute({1, 0, 3, 2}), x, P}, 256 | 512);
  }
  at::Tensor phi_fwd(const at::Tensor &P, const at::Tensor &x, const at::Tensor &A) {  // src/tt_als.py:256-257
    return o.E(APPLY, {x.permute({2, 1, 0}), A.permute({1, 3, 0, 2}), x.permute({2, 1, 0}), P}, 256 | 512);
  }

  static bool res_stalled(double prev, double res, double tol) {
    return std::isfinite(prev) && std::isfinite(res) && res <= 50 * tol && res >= 0.8 * prev;
  }

  struct Result {
    double step, max_res;
    int64_t swp;
  };

  // tt_eig.tt_max_generalised_eigen's sweep loop (src/tt_als.py:1132-1283), up to tt_normalise
  Result run(const std::vector<at::Tensor> &A, const std::vector<at::Tensor> &Dl, std::vector<at::Tensor> &x,
             const at::Tensor &o3, int64_t nswp) {
    const int64_t d = (int64_t)x.size();
    std::vector<int64_t> rx((size_t)d + 1), N((size_t)d);
    rx[0] = 1;
    for (int64_t k = 0; k < d; ++k) {
      N[(size_t)k] = x[(size_t)k].size(1);
      if (k + 1 < d) rx[(size_t)k + 1] = x[(size_t)k].size(2);
    }
    rx[(size_t)d] = 1;
    std::vector<at::Tensor> XAX((size_t)d + 1), XDX((size_t)d + 1);
    XAX[0] = XDX[0] = XAX[(size_t)d] = XDX[(size_t)d] = o3;
    double step = 1.0;
    const int64_t cols = d - 1;
    std::vector<double> local_res((size_t)(2 * cols), INFINITY);
    bool have_prev_step = false;
    double prev_step = 0.0, prev_res = INFINITY;
    int64_t swp = 0;
    dbuf = o.emp({2 * std::max<int64_t>(d, 1)});
    dn = 0;
    skip = false;

    auto svd_left = [&](int64_t k) {  // tt_eig._svd_left
      at::Tensor mat = o.clone(o.contig(x[(size_t)k]).view({rx[(size_t)k], N[(size_t)k] * rx[(size_t)k + 1]}).t());
      Ops::SVD p = o.svd(mat, true, c10::nullopt);
      at::Tensor v = o.E("r,rj->rj", {p.S, p.Vt});
      const int64_t r = std::min(prune(p.s.data(), (int64_t)p.s.size(), trunc_tol), max_rank);
      x[(size_t)k] = o.clone(p.U.slice(1, 0, r).t()).view({r, N[(size_t)k], rx[(size_t)k + 1]});
      return v.slice(0, 0, r);
    };
    auto dense_flag = [&](int64_t k) { return std::sqrt((double)(rx[(size_t)k] * rx[(size_t)k + 1])) < (double)size_limit; };

    auto finish_fwd = [&]() {
      skip = true;
      for (int64_t k = 0; k < d; ++k) {
        const int64_t a = rx[(size_t)k] * N[(size_t)k], b = rx[(size_t)k + 1];
        Post post{std::min(a, b), [&, a, b](const at::Tensor &v, const at::Tensor &S_out) {
                    return o.svd(v.view({a, b}), false, S_out);
                  }};
        StepOut so = local_last(x[(size_t)k], XDX[(size_t)k], Dl[(size_t)k], XDX[(size_t)k + 1], XAX[(size_t)k],
                                A[(size_t)k], XAX[(size_t)k + 1], dense_flag(k), step, k < d - 1 ? &post : nullptr);
        step = so.step;
        at::Tensor sol = so.sol.view({rx[(size_t)k] * N[(size_t)k], rx[(size_t)k + 1]});
        if (k < d - 1) {
          Ops::SVD p = so.has_pre ? so.pre : o.svd(sol, true, c10::nullopt);
          at::Tensor v = o.E("r,rj->rj", {p.S, p.Vt});
          const int64_t r = std::min(prune(p.s.data(), (int64_t)p.s.size(), trunc_tol), max_rank);
          x[(size_t)k] = o.clone(p.U.slice(1, 0, r)).view({rx[(size_t)k], N[(size_t)k], r});
          x[(size_t)k + 1] = o.E("ij,jkl->ikl", {v.slice(0, 0, r), x[(size_t)k + 1]});
          rx[(size_t)k + 1] = r;
          o.begin();
          XAX[(size_t)k + 1] = phi_fwd(XAX[(size_t)k], x[(size_t)k], A[(size_t)k]);
          XDX[(size_t)k + 1] = phi_fwd(XDX[(size_t)k], x[(size_t)k], Dl[(size_t)k]);
          o.end();
        } else {
          x[(size_t)k] = o.contig(sol).view({rx[(size_t)k], N[(size_t)k], rx[(size_t)k + 1]});
        }
      }
    };
    auto finish_bck = [&]() {
      skip = true;
      for (int64_t k = d - 1; k >= 0; --k) {
        const int64_t a = rx[(size_t)k], b = N[(size_t)k] * rx[(size_t)k + 1];
        Post post{std::min(a, b), [&, a, b](const at::Tensor &v, const at::Tensor &S_out) {
                    return o.svd(o.clone(v.view({a, b}).t()), false, S_out);
                  }};
        StepOut so = local_last(x[(size_t)k], XDX[(size_t)k], Dl[(size_t)k], XDX[(size_t)k + 1], XAX[(size_t)k],
                                A[(size_t)k], XAX[(size_t)k + 1], dense_flag(k), step, k > 0 ? &post : nullptr);
        step = so.step;
        if (k > 0) {
          Ops::SVD p;
          if (so.has_pre) {
            p = so.pre;
          } else {
            at::Tensor mat = o.clone(so.sol.view({rx[(size_t)k], N[(size_t)k] * rx[(size_t)k + 1]}).t());
            p = o.svd(mat, true, c10::nullopt);
          }
          at::Tensor v = o.E("r,rj->rj", {p.S, p.Vt});
          const int64_t r = std::min(prune(p.s.data(), (int64_t)p.s.size(), trunc_tol), max_rank);
          x[(size_t)k] = o.clone(p.U.slice(1, 0, r).t()).view({r, N[(size_t)k], rx[(size_t)k + 1]});
          x[(size_t)k - 1] = o.E("rdc,Rc->rdR", {x[(size_t)k - 1], v.slice(0, 0, r)});
          rx[(size_t)k] = r;
          o.begin();
          XAX[(size_t)k] = phi_bck(XAX[(size_t)k + 1], x[(size_t)k], A[(size_t)k]);
          XDX[(size_t)k] = phi_bck(XDX[(size_t)k + 1], x[(size_t)k], Dl[(size_t)k]);
          o.end();
        } else {
          x[(size_t)k] = o.contig(so.sol).view({rx[(size_t)k], N[(size_t)k], rx[(size_t)k + 1]});
        }
      }
    };

    for (swp = 0; swp < nswp; ++swp) {
      bool zero = false;
      for (int64_t k = d - 1; k > 0; --k) {
        if (swp > 0) {
          Local l = local_solve(x[(size_t)k - 1], x[(size_t)k], XAX[(size_t)k - 1], A[(size_t)k - 1], A[(size_t)k],
                                XAX[(size_t)k + 1], XDX[(size_t)k - 1], Dl[(size_t)k - 1], Dl[(size_t)k],
                                XDX[(size_t)k + 1], step, true);
          x[(size_t)k - 1] = l.s1;
          x[(size_t)k] = l.s2;
          step = l.step;
          put(local_res, cols, 0, (int)(k - 1), l.res);
          if (step <= 0) {
            zero = true;
            break;
          }
        } else {
          at::Tensor vr = svd_left(k);
          x[(size_t)k - 1] = o.E("rdc,Rc->rdR", {x[(size_t)k - 1], vr});
        }
        rx[(size_t)k] = x[(size_t)k].size(0);
        XAX[(size_t)k] = phi_bck(XAX[(size_t)k + 1], x[(size_t)k], A[(size_t)k]);
        XDX[(size_t)k] = phi_bck(XDX[(size_t)k + 1], x[(size_t)k], Dl[(size_t)k]);
      }
      resolve(local_res, cols);
      if (zero) break;
      if (npmax(local_res) < tol || swp == nswp - 1) {
        finish_fwd();
        break;
      }
      for (int64_t k = 0; k < d - 1; ++k) {
        Local l = local_solve(x[(size_t)k], x[(size_t)k + 1], XAX[(size_t)k], A[(size_t)k], A[(size_t)k + 1],
                              XAX[(size_t)k + 2], XDX[(size_t)k], Dl[(size_t)k], Dl[(size_t)k + 1], XDX[(size_t)k + 2],
                              step, false);
        x[(size_t)k] = l.s1;
        x[(size_t)k + 1] = l.s2;
        step = l.step;
        put(local_res, cols, 1, (int)k, l.res);
        if (step <= 0) {
          zero = true;
          break;
        }
        rx[(size_t)k + 1] = x[(size_t)k + 1].size(0);
        XAX[(size_t)k + 1] = phi_fwd(XAX[(size_t)k], x[(size_t)k], A[(size_t)k]);
        XDX[(size_t)k + 1] = phi_fwd(XDX[(size_t)k], x[(size_t)k], Dl[(size_t)k]);
      }
      resolve(local_res, cols);
      if (zero) break;
      if (npmax(local_res) < tol) {
        finish_bck();
        break;
      }
      const double sres = npmax(local_res);
      if (swp >= 2 && have_prev_step) {  // tt_eig._step_stalled
        const double sc = pymax(pymax(std::fabs(step), std::fabs(prev_step)), 1.0);
        if (std::fabs(step - prev_step) <= pymax(10 * tol, 1e-12) * sc && res_stalled(prev_res, sres, tol)) break;
      }
      have_prev_step = true;
      prev_step = step;
      prev_res = sres;
    }
    if (swp == nswp && nswp > 0) swp = nswp - 1;  // Python's loop variable keeps its last value
    return {step, npmax(local_res), swp};
  }
};

// entry: (status, step, max_res, swp, cores, key, pos, has_gauss, gauss, message); status != 0 =
// rerun in Python
pybind11::tuple eig_als(const std::vector<at::Tensor> &A, const std::vector<at::Tensor> &Dl,
                        const std::vector<at::Tensor> &x0, const at::Tensor &o3, int64_t nswp, double tol,
                        int64_t size_limit, double trunc_tol, int64_t max_rank, int64_t max_dense,
                        pybind11::array_t<uint32_t, pybind11::array::c_style | pybind11::array::forcecast> key,
                        int64_t pos, int64_t has_gauss, double gauss, bool split_kick, bool trunc_kick) {
  TORCH_CHECK(F.svd_tol && F.batch_end, "ttk_host_bind: bind_eig() not called");
  TORCH_CHECK(g_einsum && g_axpby, "ttk_host_bind: bind() / bind2() not called");  // (g_stream may be the null stream)
  TORCH_CHECK(key.size() == 624, "eig_als: MT19937 key of ", key.size(), " words");
  TORCH_CHECK(A.size() == x0.size() && Dl.size() == x0.size() && x0.size() >= 2, "eig_als: operand lists");
  Solver s;
  s.o.opt = o3.options();
  std::memcpy(s.mt.key, key.data(), sizeof(s.mt.key));
  s.mt.pos = (int)pos;
  s.mt.has_gauss = (int)has_gauss;
  s.mt.gauss = gauss;
  s.tol = tol;
  s.trunc_tol = trunc_tol;
  s.size_limit = size_limit;
  s.max_rank = max_rank;
  s.max_dense = max_dense;
  s.split_kick = split_kick;
  s.trunc_kick = trunc_kick;
  std::vector<at::Tensor> x = x0;
  int status = 0;
  std::string why;
  Solver::Result r{0.0, 0.0, 0};
  {
    pybind11::gil_scoped_release nogil;
    // status 1: a Bail; 2: a libttk failure -- the Python rerun then raises whatever tt_eig.py
    // raises there, with its own exception types (LinAlgError / TTKError / ZeroDivisionError ...)
    try {
      r = s.run(A, Dl, x, o3, nswp);
    } catch (const Bail &) {
      status = 1;
    } catch (const std::exception &e) {
      status = 2;
      why = e.what();
    } catch (...) {
      status = 2;
    }
    if (s.o.batch) {  // left inside a batch: close it (recorded steps still launch, in order)
      s.o.batch = 1;
      try {
        s.o.end();
      } catch (...) {
      }
    }
    s.dbuf = at::Tensor();
  }
  pybind11::array_t<uint32_t> kout(624);
  std::memcpy(kout.mutable_data(), s.mt.key, sizeof(s.mt.key));
  pybind11::list xs;
  for (auto &t : x) xs.append(t);
  return pybind11::make_tuple(status, r.step, r.max_res, r.swp, xs, kout, s.mt.pos, s.mt.has_gauss, s.mt.gauss,
                              why.substr(0, 400));
}

// RandomState.randn(n) from a state (tests: the restated stream against NumPy's)
pybind11::tuple legacy_randn(pybind11::array_t<uint32_t, pybind11::array::c_style | pybind11::array::forcecast> key,
                             int64_t pos, int64_t has_gauss, double gauss, int64_t n) {
  TORCH_CHECK(key.size() == 624, "legacy_randn: MT19937 key of ", key.size(), " words");
  MT mt;
  std::memcpy(mt.key, key.data(), sizeof(mt.key));
  mt.pos = (int)pos;
  mt.has_gauss = (int)has_gauss;
  mt.gauss = gauss;
  pybind11::array_t<double> out(n);
  double *p = out.mutable_data();
  for (int64_t i = 0; i < n; ++i) p[i] = mt.next_gauss();
  pybind11::array_t<uint32_t> kout(624);
  std::memcpy(kout.mutable_data(), mt.key, sizeof(mt.key));
  return pybind11::make_tuple(out, kout, mt.pos, mt.has_gauss, mt.gauss);
}

// T.prune_singular_vals restated (tests)
int64_t prune_singular_vals(pybind11::array_t<double, pybind11::array::c_style | pybind11::array::forcecast> s,
                            double eps) {
  return prune(s.data(), (int64_t)s.size(), eps);
}

void bind_eig(const std::vector<int64_t> &a) {
  TORCH_CHECK(a.size() == 14 || a.size() == 15 || a.size() == 17 || a.size() == 20, "bind_eig: ", a.size(), " addresses");
  F.svd_work = reinterpret_cast<svd_work_fn>(a[0]);
  F.svd_tol = reinterpret_cast<svd_tol_fn>(a[1]);
  F.qr_work = reinterpret_cast<qr_work_fn>(a[2]);
  F.qr = reinterpret_cast<qr_fn>(a[3]);
  F.syev_work = reinterpret_cast<syev_work_fn>(a[4]);
  F.syev = reinterpret_cast<syev_fn>(a[5]);
  F.read = reinterpret_cast<read_fn>(a[6]);
  F.upload = reinterpret_cast<upload_fn>(a[7]);
  F.chol = reinterpret_cast<chol_fn>(a[8]);
  F.trsm = reinterpret_cast<trsm_fn>(a[9]);
  F.ray_dev = reinterpret_cast<ray_dev_fn>(a[10]);
  F.ray_sync = reinterpret_cast<ray_sync_fn>(a[11]);
  F.batch_begin = reinterpret_cast<batch_fn>(a[12]);
  F.batch_end = reinterpret_cast<batch_fn>(a[13]);
  F.svd_read = a.size() > 14 ? reinterpret_cast<svd_read_fn>(a[14]) : nullptr;  // 0 where the library lacks it
  F.split_kick_lds = a.size() > 16 ? reinterpret_cast<split_kick_lds_fn>(a[15]) : nullptr;
  F.split_kick = a.size() > 16 ? reinterpret_cast<split_kick_fn>(a[16]) : nullptr;
  F.trunc_kick_lds = a.size() > 19 ? reinterpret_cast<trunc_kick_lds_fn>(a[17]) : nullptr;
  F.trunc_kick = a.size() > 19 ? reinterpret_cast<trunc_kick_fn>(a[18]) : nullptr;
  F.trunc_kick_read = a.size() > 19 ? reinterpret_cast<trunc_kick_fn>(a[19]) : nullptr;
}

}  // namespace eig
