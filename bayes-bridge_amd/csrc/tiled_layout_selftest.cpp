// Self-test of the tiled layout builder + emulator for the sanitizer builds
// (make sanitize: -fsanitize=address,undefined and -fsanitize=thread; the
// builder is multi-threaded over panels).  Generates CSR matrices with an LCG,
// builds the layout with several worker threads (value-free and valued),
// emulates the kernel's walk and compares with a plain CSR product.  Mixed
// designs (split by value into B + D + S) go through the same by shape class,
// and every layout built is also walked load by load (emulate_tiled_loads,
// -DBBX_EMU_SHADOW_LOADS) on buffers of exactly the uploaded sizes.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <utility>
#include <vector>

#include "tiled_layout.hpp"

namespace {

struct Lcg {
  uint64_t s;
  uint32_t next() {
    s = s * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)(s >> 33);
  }
  double unit() { return (next() + 0.5) / 2147483648.0; }
};

int run_case(int64_t R, int64_t C, double density, bool binary,
             int force_PR, int force_G, uint64_t seed, int packed = -1) {
  Lcg g{seed};
  std::vector<int64_t> rowptr((size_t)R + 1, 0);
  std::vector<int32_t> colidx;
  std::vector<double> vals;
  for (int64_t r = 0; r < R; ++r) {
    // skewed columns (hot ones recur), ascending, duplicates allowed
    int64_t c = 0;
    const double row_density = density * (0.25 + 1.5 * g.unit());
    while (true) {
      const double u = g.unit();
      c += 1 + (int64_t)(-std::log(u) / row_density * (c < C / 8 ? 0.2 : 1.0));
      if (c >= C) break;
      colidx.push_back((int32_t)c);
      vals.push_back(binary ? 1.0 : g.unit() - 0.5);
      if (g.unit() < 0.01) {  // duplicate entry
        colidx.push_back((int32_t)c);
        vals.push_back(binary ? 1.0 : g.unit() - 0.5);
      }
    }
    rowptr[(size_t)r + 1] = (int64_t)colidx.size();
  }
  const int64_t nnz = (int64_t)colidx.size();
  std::vector<double> x((size_t)C), ref((size_t)R, 0.);
  for (auto& v : x) v = g.unit() - 0.5;
  for (int64_t r = 0; r < R; ++r)
    for (int64_t k = rowptr[(size_t)r]; k < rowptr[(size_t)r + 1]; ++k)
      ref[(size_t)r] += vals[(size_t)k] * x[(size_t)colidx[(size_t)k]];
  bbx::TiledOptions opt;
  opt.force_PR = force_PR;
  opt.force_G = force_G;
  opt.max_threads = 4;
  opt.packed = packed;
  bbx::TiledHost m;
  std::string err;
  if (colidx.empty()) colidx.push_back(0);
  if (bbx::build_tiled_host(R, C, nnz, rowptr.data(), colidx.data(),
                            binary ? nullptr : vals.data(), opt, &m, &err) != 0) {
    fprintf(stderr, "build failed: %s\n", err.c_str());
    return 1;
  }
  std::vector<double> slab;
  bbx::emulate_tiled_spmv(m, x.data(), &slab);
#ifdef BBX_EMU_SHADOW_LOADS
  bbx::emulate_tiled_loads(m, x.data(), false);
  bbx::emulate_tiled_loads(m, x.data(), true);
#endif
  double worst = 0.;
  for (int64_t r = 0; r < R; ++r) {
    double a = 0.;
    for (int gq = 0; gq < m.G; ++gq) a += slab[(size_t)gq * (size_t)R + (size_t)r];
    worst = std::fmax(worst, std::fabs(a - ref[(size_t)r]));
  }
  const double cyc = bbx::tiled_mean_gather_cycles(m);
  printf("R=%lld C=%lld nnz=%lld %s%s PR=%d G=%d W=%d blocks=%d extras=%d: "
         "max err %.2e, %.2f LDS cycles per gather\n",
         (long long)R, (long long)C, (long long)nnz, binary ? "binary" : "valued",
         m.packed ? " packed" : "", m.PR, m.G, m.W, m.n_block, m.n_extra, worst, cyc);
  return worst <= 1e-10 ? 0 : 1;
}

// The 64-bit constructor's host utilities: the threaded transposition against
// a serial one, the transposed matrix through the layout + emulator, and the
// structure check on a broken copy.
int run_transpose_case(int64_t R, int64_t C, double density, uint64_t seed) {
  Lcg g{seed};
  std::vector<int64_t> rowptr((size_t)R + 1, 0), col64;
  std::vector<int32_t> colidx;
  std::vector<double> vals;
  for (int64_t r = 0; r < R; ++r) {
    for (int64_t c = 0; c < C; ++c)
      if (g.unit() < density) {
        colidx.push_back((int32_t)c);
        col64.push_back(c);
        vals.push_back(g.unit() - .5);
      }
    rowptr[(size_t)r + 1] = (int64_t)colidx.size();
  }
  const int64_t nnz = (int64_t)colidx.size();
  if (nnz == 0) return 0;
  if (bbx::check_csr64_host(R, C, nnz, rowptr.data(), col64.data(), 8) != 0) return 1;
  bbx::HostCsr t;
  bbx::transpose_csr_host(R, C, rowptr.data(), colidx.data(), vals.data(), 8, &t);
  // serial reference: entries of column j in row order
  std::vector<int64_t> at((size_t)C + 1, 0);
  for (int64_t k = 0; k < nnz; ++k) at[(size_t)colidx[(size_t)k] + 1] += 1;
  for (int64_t j = 0; j < C; ++j) at[(size_t)j + 1] += at[(size_t)j];
  int bad = 0;
  for (int64_t j = 0; j <= C; ++j) bad += t.rowptr[(size_t)j] != at[(size_t)j];
  std::vector<int64_t> pos(at.begin(), at.end() - 1);
  for (int64_t r = 0; r < R; ++r)
    for (int64_t k = rowptr[(size_t)r]; k < rowptr[(size_t)r + 1]; ++k) {
      const int64_t w = pos[(size_t)colidx[(size_t)k]]++;
      bad += t.colidx[(size_t)w] != (int32_t)r || t.vals[(size_t)w] != vals[(size_t)k];
    }
  // broken copies: a column id out of range, a row out of order
  std::vector<int64_t> broken = col64;
  broken[(size_t)(nnz / 2)] = C;
  bad += (bbx::check_csr64_host(R, C, nnz, rowptr.data(), broken.data(), 8) & 2) == 0;
  if (rowptr[1] >= 2) {
    broken = col64;
    std::swap(broken[0], broken[1]);
    bad += (bbx::check_csr64_host(R, C, nnz, rowptr.data(), broken.data(), 8) & 4) == 0;
  }
  printf("transpose R=%lld C=%lld nnz=%lld: %s\n", (long long)R, (long long)C,
         (long long)nnz, bad ? "MISMATCH" : "equal to the serial transposition");
  return bad ? 1 : 0;
}

// ---- mixed designs: X = B + D + S (spmv_tiled.hip HybridParts) by shape.
//
// plan_hybrid -> split_rows -> build_tiled_host of B and S in both
// orientations -> emulate_tiled_spmv; B v + D v + S v and the transposed sum
// against a plain CSR product; X rebuilt from the parts exactly; and, for every
// layout built, emulate_tiled_loads: the kernel's loads INCLUDING those that
// contribute nothing to a sum, on heap blocks of exactly the uploaded sizes.
struct MixedShape {
  const char* cls;   // shape class (printed)
  int64_t n, p_bin;
  double dens_b;     // density of the 1.0 entries of the binary columns
  int kd;            // full continuous columns (about a tenth of their entries is 1.0)
  int s_mode;        // valued rest: 0 none, 1 at most four entries in each of the
                     // FIRST min(n, 128) - 2 rows (one step, one slice; the rows
                     // behind stay empty), 2 a third of the rows of every valued column
  int s_cols;        // columns (spread over the binary ones) that carry S
  int force_PR;      // 0: the builder's choice
  // expected counts of the case-[8] shape (0: not checked)
  int64_t quads_B, quads_S, quads_St;
};

struct Mixed {
  std::vector<int64_t> rowptr;
  std::vector<int32_t> colidx;
  std::vector<double> vals;
};

void mixed_generate(const MixedShape& sh, uint64_t seed, Mixed* X) {
  Lcg g{seed};
  const int64_t n = sh.n, pb = sh.p_bin;
  std::vector<int32_t> scol;
  for (int k = 0; k < sh.s_cols && pb > 0; ++k)
    scol.push_back((int32_t)((pb * (2 * (int64_t)k + 1)) / (2 * sh.s_cols)));
  X->rowptr.assign((size_t)n + 1, 0);
  X->colidx.clear();
  X->vals.clear();
  const int64_t s_rows = std::max<int64_t>(std::min<int64_t>(n, 128) - 2, 1);
  for (int64_t r = 0; r < n; ++r) {
    // (column, value) of the row; sorted by column afterwards (stable: the
    // duplicates keep their order)
    std::vector<std::pair<int32_t, double>> row;
    if (r == 0 && pb > 0) row.push_back({0, 1.0});
    int64_t c = -1;
    while (pb > 0) {
      c += 1 + (int64_t)(-std::log(g.unit()) / sh.dens_b);
      if (c >= pb) break;
      row.push_back({(int32_t)c, 1.0});
      if (g.unit() < 0.02) row.push_back({(int32_t)c, 1.0});  // duplicate
    }
    if (sh.s_mode == 1 && r < s_rows) {
      const int cnt = 1 + (int)(g.next() % 4u);
      for (int k = 0; k < cnt && k < (int)scol.size(); ++k)
        if (g.unit() < 0.5 || k == 0)
          row.push_back({scol[(size_t)((r + k) % (int64_t)scol.size())], g.unit() - 0.5});
    } else if (sh.s_mode == 2) {
      for (int32_t j : scol)
        if (g.unit() < 0.33) {
          row.push_back({j, 4. * (g.unit() - 0.5)});
          if (g.unit() < 0.05) row.push_back({j, g.unit() - 0.5});  // duplicate
        }
    }
    for (int k = 0; k < sh.kd; ++k) {
      // the even rows keep a value other than 1.0, so that the column is a
      // dense one at every n; a tenth of the rest is exactly 1.0 and belongs to B
      const bool one = (r & 1) && g.unit() < 0.2;
      row.push_back({(int32_t)(pb + k), one ? 1.0 : 2. * (g.unit() - 0.5)});
      if (!one && g.unit() < 0.02)
        row.push_back({(int32_t)(pb + k), g.unit() - 0.5});  // duplicate in D
    }
    std::stable_sort(row.begin(), row.end(),
                     [](const std::pair<int32_t, double>& a,
                        const std::pair<int32_t, double>& b) { return a.first < b.first; });
    for (auto& e : row) {
      X->colidx.push_back(e.first);
      X->vals.push_back(e.second);
    }
    X->rowptr[(size_t)r + 1] = (int64_t)X->colidx.size();
  }
}

// Layout + emulator product of one part (and the shadow walk of the kernel's
// loads in both forms of the slice fill); out += part x
int mixed_part_product(int64_t R, int64_t C, const bbx::HostCsr& part, bool valued,
                       int force_PR, const std::vector<double>& x,
                       std::vector<double>* out, bbx::TiledHost* keep) {
  bbx::TiledOptions opt;
  opt.force_PR = force_PR;
  opt.max_threads = 4;
  std::string err;
  bbx::TiledHost& m = *keep;
  const int64_t nnz = part.rowptr[(size_t)R];
  if (bbx::build_tiled_host(R, C, nnz, part.rowptr.data(), part.colidx.data(),
                            valued ? part.vals.data() : nullptr, opt, &m, &err) != 0) {
    fprintf(stderr, "mixed: build failed: %s\n", err.c_str());
    return 1;
  }
  std::vector<double> slab;
  bbx::emulate_tiled_spmv(m, x.data(), &slab);
  for (int64_t r = 0; r < R; ++r)
    for (int gq = 0; gq < m.G; ++gq)
      (*out)[(size_t)r] += slab[(size_t)gq * (size_t)R + (size_t)r];
#ifdef BBX_EMU_SHADOW_LOADS
  bbx::emulate_tiled_loads(m, x.data(), false);
  bbx::emulate_tiled_loads(m, x.data(), true);
#endif
  return 0;
}

int run_mixed(const MixedShape& sh, uint64_t seed) {
  Mixed X;
  mixed_generate(sh, seed, &X);
  const int64_t n = sh.n, p = sh.p_bin + sh.kd, nnz = X.rowptr[(size_t)n];
  bbx::HybridPlan plan;
  bbx::plan_hybrid(n, p, nnz, X.colidx.data(), X.vals.data(), &plan);
  int bad = 0;
  if (!plan.split || (int)plan.dense_cols.size() != sh.kd ||
      (plan.rest_nnz > 0) != (sh.s_mode != 0)) {
    fprintf(stderr, "mixed %s n=%lld: plan split=%d kd=%zu rest=%lld, expected kd=%d S %s\n",
            sh.cls, (long long)n, (int)plan.split, plan.dense_cols.size(),
            (long long)plan.rest_nnz, sh.kd, sh.s_mode ? "present" : "absent");
    return 1;
  }
  bbx::HostCsr Xt;
  bbx::transpose_csr_host(n, p, X.rowptr.data(), X.colidx.data(), X.vals.data(), 4, &Xt);
  std::vector<double> D;
  bbx::hybrid_dense_block(n, p, X.rowptr.data(), X.colidx.data(), X.vals.data(),
                          plan.dense_cols, &D);
  Lcg g{seed ^ 0x9E3779B97F4A7C15ull};
  std::vector<double> v((size_t)p), w((size_t)n);
  for (auto& a : v) a = g.unit() - 0.5;
  for (auto& a : w) a = g.unit() - 0.5;
  bbx::TiledHost lay[2][2];   // [orientation][B, S]
  int64_t quads[2][2] = {{0, 0}, {0, 0}};
  for (int t = 0; t < 2; ++t) {
    const int64_t R = t ? p : n, C = t ? n : p;
    const int64_t* rp = t ? Xt.rowptr.data() : X.rowptr.data();
    const int32_t* ci = t ? Xt.colidx.data() : X.colidx.data();
    const double* va = t ? Xt.vals.data() : X.vals.data();
    const std::vector<double>& in = t ? w : v;
    bbx::HostCsr ones, rest;
    bbx::split_rows(R, rp, ci, va, t != 0, plan.is_dense, &ones, &rest);
    if (ones.rowptr[(size_t)R] != plan.ones_nnz || rest.rowptr[(size_t)R] != plan.rest_nnz) {
      fprintf(stderr, "mixed %s: split_rows counts differ from the plan\n", sh.cls);
      ++bad;
    }
    // X rebuilt from the parts, exactly: per row the entries of B and S in
    // stored order interleave back into the row's entries outside D, and D
    // holds the in-order sum of the others
    for (int64_t r = 0; r < R && !bad; ++r) {
      int64_t k1 = ones.rowptr[(size_t)r], k2 = rest.rowptr[(size_t)r];
      for (int64_t k = rp[r]; k < rp[r + 1]; ++k) {
        const int32_t j = ci[k];
        const double val = va[k];
        const bool dense_col = plan.is_dense[(size_t)(t ? r : j)] != 0;
        if (val == 1.0) {
          if (k1 >= ones.rowptr[(size_t)r + 1] || ones.colidx[(size_t)k1] != j) ++bad;
          ++k1;
        } else if (!dense_col) {
          if (k2 >= rest.rowptr[(size_t)r + 1] || rest.colidx[(size_t)k2] != j ||
              rest.vals[(size_t)k2] != val) ++bad;
          ++k2;
        }
      }
      if (k1 != ones.rowptr[(size_t)r + 1] || k2 != rest.rowptr[(size_t)r + 1]) ++bad;
    }
    if (t == 0) {
      // (the rows are sorted by column: the entries of one column are a run)
      std::vector<int32_t> slot_of((size_t)p, -1);
      for (size_t s_ = 0; s_ < plan.dense_cols.size(); ++s_)
        slot_of[(size_t)plan.dense_cols[s_]] = (int32_t)s_;
      std::vector<uint8_t> seen(plan.dense_cols.size());
      for (int64_t r = 0; r < n; ++r) {
        std::fill(seen.begin(), seen.end(), 0);
        for (int64_t k = rp[r]; k < rp[r + 1];) {
          const int32_t j = ci[k];
          double a = 0.;
          for (; k < rp[r + 1] && ci[k] == j; ++k)
            if (va[k] != 1.0) a += va[k];
          const int32_t s_ = slot_of[(size_t)j];
          if (s_ < 0) continue;
          seen[(size_t)s_] = 1;
          if (a != D[(size_t)s_ * (size_t)n + (size_t)r]) ++bad;
        }
        for (size_t s_ = 0; s_ < seen.size(); ++s_)
          if (!seen[s_] && D[s_ * (size_t)n + (size_t)r] != 0.) ++bad;
      }
    }
    if (bad) {
      fprintf(stderr, "mixed %s n=%lld: X is NOT the sum of its parts\n", sh.cls, (long long)n);
      return 1;
    }
    std::vector<double> out((size_t)R, 0.), ref((size_t)R, 0.);
    bad += mixed_part_product(R, C, ones, false, sh.force_PR, in, &out, &lay[t][0]);
    quads[t][0] = lay[t][0].n_quad;
    if (plan.rest_nnz > 0) {
      bad += mixed_part_product(R, C, rest, true, sh.force_PR, in, &out, &lay[t][1]);
      quads[t][1] = lay[t][1].n_quad;
    }
    for (size_t s_ = 0; s_ < plan.dense_cols.size(); ++s_) {
      const int32_t j = plan.dense_cols[s_];
      if (t == 0) {
        for (int64_t r = 0; r < n; ++r) out[(size_t)r] += D[s_ * (size_t)n + (size_t)r] * v[(size_t)j];
      } else {
        double a = 0.;
        for (int64_t r = 0; r < n; ++r) a += D[s_ * (size_t)n + (size_t)r] * w[(size_t)r];
        out[(size_t)j] += a;
      }
    }
    double worst = 0., scale = 1.;
    for (int64_t r = 0; r < R; ++r) {
      for (int64_t k = rp[r]; k < rp[r + 1]; ++k) ref[(size_t)r] += va[k] * in[(size_t)ci[k]];
      scale = std::fmax(scale, std::fabs(ref[(size_t)r]));
      worst = std::fmax(worst, std::fabs(out[(size_t)r] - ref[(size_t)r]));
    }
    printf("mixed %-14s %s n=%lld p=%lld kd=%d nnz=%lld = %lld + %lld + %lld; B: PR=%d "
           "panels=%d G=%d quads=%lld slices=%lld; S: panels=%d G=%d quads=%lld "
           "slices=%lld: max err %.2e\n",
           sh.cls, t ? "X^T w" : "X v  ", (long long)n, (long long)p, sh.kd,
           (long long)nnz, (long long)plan.ones_nnz, (long long)plan.dense_nnz,
           (long long)plan.rest_nnz, lay[t][0].PR, lay[t][0].n_panel, lay[t][0].G,
           (long long)lay[t][0].n_quad, (long long)lay[t][0].n_slice,
           lay[t][1].n_panel, lay[t][1].G, (long long)lay[t][1].n_quad,
           (long long)lay[t][1].n_slice, worst);
    if (!(worst <= 1e-10 * scale)) ++bad;
  }
  if (sh.quads_B &&
      (quads[0][0] != sh.quads_B || quads[0][1] != sh.quads_S ||
       quads[1][1] != sh.quads_St || lay[0][1].n_slice != 1 ||
       lay[0][1].n_panel != 2)) {
    fprintf(stderr, "mixed %s: not the shape it names (B %lld quads, S %lld, S^T %lld)\n",
            sh.cls, (long long)quads[0][0], (long long)quads[0][1], (long long)quads[1][1]);
    ++bad;
  }
  return bad;
}

int run_mixed_all() {
  int bad = 0;
  uint64_t seed = 100;
  // The shape from which an illegal memory access was recorded (tests/
  // test_hip_operator.py, mixed case [8]): 130 x 65 without dense columns, S of
  // one step in one slice whose SECOND panel (rows 128, 129) is empty -- a
  // workgroup without a single step at the very end of the id and value
  // streams --, S^T of 2 steps, B of 6.
  bad += run_mixed({"case-8", 130, 65, .135, 0, 1, 7, 0, 6, 1, 2}, 8);
  // the 24 randomised mixed cases of the GPU suite, by shape class: rows from
  // 3 to 9000, one to four column blocks, 0 to 3 dense columns, S present
  {
    Lcg g{77};
    const int64_t ns[] = {3, 17, 130, 1000, 4097, 9000};
    const int64_t ps[] = {2, 65, 900, 16128, 16130, 33000, 50000};
    for (int c = 0; c < 24; ++c) {
      const int64_t n = ns[g.next() % 6u], p = ps[g.next() % 7u];
      const double dens = p > 1000 ? (g.next() % 2u ? .0003 : .001)
                                   : (g.next() % 2u ? .05 : .3);
      const int kd = n >= 130 ? c % 4 : 0;
      // (n = 3: a valued column of a third of the rows would be a dense one)
      const int s_mode = (p >= 65 && n >= 17) ? 1 + c % 2 : 0;
      bad += run_mixed({"random", n, p, dens, kd, s_mode, p >= 900 ? 40 : 7, 0, 0, 0, 0},
                       ++seed);
    }
  }
  // separate kernels: the addend kernel's four-column unroll and its tail, the
  // even-rounded row chunks of the dense transposed product (n around one
  // panel and around 2 x 256 chunks), S absent / one step / two slices
  for (int64_t n : {2, 129, 130, 131, 255, 256, 257, 511, 512, 513})
    for (int kd : {0, 1, 3, 4, 5, 8, 9})
      for (int s_mode : {0, 1, 2}) {
        if (n == 2 && s_mode) continue;   // (a valued entry in 2 rows is a dense column)
        if (n != 130 && n != 257 && kd != 0 && kd != 5 && kd != 9) continue;
        bad += run_mixed({"separate", n, 65, .3, kd, s_mode, 7, 0, 0, 0, 0}, ++seed);
      }
  bad += run_mixed({"addend-lap2", 262145, 4, .3, 2, 0, 0, 0, 0, 0, 0}, ++seed);
  // slabs: two column groups of B with S in both, more panels than partial slots
  bad += run_mixed({"slabs-G2", 130, 16130, .004, 0, 2, 40, 0, 0, 0, 0}, ++seed);
  bad += run_mixed({"slabs-panels", 32769, 63, .1, 2, 0, 0, 128, 0, 0, 0}, ++seed);
  // dense epilogue (kd <= 8) and the one-pass kernels: no S
  for (int64_t n : {1, 2, 127, 128, 129, 1025, 32768})
    bad += run_mixed({"epi", n, 40, .3, n == 1 ? 1 : n == 2 ? 7 : 8, 0, 0,
                      n >= 32768 ? 128 : 0, 0, 0, 0}, ++seed);
  for (int kd : {9, 127, 128, 129, 256, 257, 512, 513, 1023, 1024})
    for (int64_t n : {1, 3, 63, 64, 65})
      if (n == 65 || kd == 9 || kd == 1024)
        bad += run_mixed({"fused-wave", n, 40, .3, kd, 0, 0, 0, 0, 0, 0}, ++seed);
  for (int64_t n : {16383, 16384, 16385})
    bad += run_mixed({"fused-wave-lap", n, 40, .3, 9, 0, 0, 0, 0, 0, 0}, ++seed);
  for (int kd : {1025, 2048, 2049, 4096, 4097, 8191, 8192})
    for (int64_t n : {1, 2, 5, 65})
      if (n == 5 || kd == 1025 || kd == 8192)
        bad += run_mixed({"fused-wg", n, 40, .3, kd, 0, 0, 0, 0, 0, 0}, ++seed);
  return bad;
}

}  // namespace

int main() {
  int bad = 0;
  bad += run_mixed_all();
  bad += run_case(3000, 900, .05, true, 0, 0, 1);
  bad += run_case(3000, 900, .05, false, 256, 0, 2);
  bad += run_case(700, 40000, .002, true, 128, 2, 3);
  bad += run_case(700, 40000, .002, true, 128, 3, 4);
  bad += run_case(5000, 17000, .004, false, 512, 2, 5);
  bad += run_case(17, 3, .6, true, 0, 0, 6);
  bad += run_case(1, 70000, .001, true, 0, 0, 7);
  // packed groups forced on and off (the builder picks by step count)
  bad += run_case(3000, 900, .05, true, 0, 0, 1, 1);
  bad += run_case(3000, 900, .05, true, 0, 0, 1, 0);
  bad += run_case(700, 40000, .002, true, 128, 2, 3, 1);
  bad += run_case(900, 33000, .0004, true, 0, 0, 8, 1);  // gaps beyond 4095 slots
  bad += run_case(1, 70000, .001, true, 0, 0, 7, 1);
  bad += run_transpose_case(3000, 900, .05, 11);
  bad += run_transpose_case(5, 40000, .01, 12);
  bad += run_transpose_case(20000, 7, .3, 13);
  if (bad) fprintf(stderr, "%d case(s) FAILED\n", bad);
  return bad ? 1 : 0;
}
