// Host build of the per-item code of thaler-study_amd/csrc/kernels/r1cs.hpp (what spmv_kernel and spmv_carry_kernel run per
// thread and per row total: spmv_item, seg_place; the image construction, image_sort; and the cubic pass's item, zc_fold4 and
// zc_accumulate), compiled for the CPU and run stand-alone: a whole product - block by block, then the walk over the carries -
// against a naive loop, on block runs that start and end inside a row, hold only one row, or skip rows that are all empty; and
// the cubic item against its definition in 128-bit integers.  Every array is allocated at its exact size: this is the build that
// runs under -fsanitize=address,undefined.
#include <cstdio>
#include <cstdlib>
#include <map>
#include <vector>

#include "../../thaler-study_amd/csrc/kernels/r1cs.hpp"
using namespace sc;

namespace {

u64 rnd_state = 0x1234567;
u64 rnd() { return rnd_state = splitmix64(rnd_state); }

template <class F>
u64 rnd_word(const F& f) {
  const u64 edge[6] = {0, 1, f.modulus() - 1, f.modulus() - 2, f.one(), 0xFFFFFFFFull};
  const u64 r = rnd();
  return (r & 7) == 0 ? edge[(r >> 3) % 6] % f.modulus() : (r >> 3) % f.modulus();
}

int failures = 0;
void check(bool ok, const char* what, size_t a = 0, size_t b = 0) {
  if (!ok) {
    if (++failures < 20) printf("FAIL %s (%zu, %zu)\n", what, a, b);
  }
}

// the block's 2 x threads parts summed by row (what seg_block_reduce's scan computes), each total placed by seg_place
template <class F>
void block_totals(const F& f, const std::vector<SegPart>& parts, u32 first_row, u32 last_row, u64* y, SegPart (&open)[2]) {
  open[0] = SegPart{first_row, 0};
  open[1] = SegPart{last_row, 0};
  for (size_t q = 0; q + 1 < parts.size(); ++q) check(parts[q].row <= parts[q + 1].row, "parts sorted by row", q);
  size_t q = 0;
  while (q < parts.size() && parts[q].row != kSpmvNoRow) {
    u64 total = 0;
    const u32 row = parts[q].row;
    for (; q < parts.size() && parts[q].row == row; ++q) total = f.add(total, parts[q].val);
    seg_place(row, total, first_row, last_row, y, open);
  }
}

// one block of spmv_kernel / one chunk of spmv_carry_kernel over entries [base, end): `vec` null = the carry walk (val * 1)
template <class F>
void run_block(const F& f, const u32* row, const u32* col, const u64* val, size_t base, size_t end, const u64* vec, u64* y, SegPart (&open)[2]) {
  constexpr int K = kSpmvRun;
  std::vector<SegPart> parts;
  for (int t = 0; t < kSpmvThreads; ++t) {
    const size_t lo = base + (size_t)t * K;
    u32 r[K];
    u64 x[K], g[K];
    int n = 0;
    for (int k = 0; k < K; ++k) {
      const bool in = lo + k < end;
      r[k] = in ? row[lo + k] : kSpmvNoRow;
      x[k] = in ? val[lo + k] : 0;
      g[k] = in ? (vec ? vec[col[lo + k]] : f.one()) : 0;
      n += in ? 1 : 0;
    }
    SegPart head, tail;
    spmv_item<F, K>(f, r, x, g, n, y, head, tail);
    parts.push_back(head);
    parts.push_back(tail);
  }
  block_totals(f, parts, row[base], row[end - 1], y, open);
}

// the two launches of a product: y zeroed, every block, then the walk over the carries as spmv_carry_kernel does it
template <class F>
void product(const F& f, const std::vector<u32>& row, const std::vector<u32>& col, const std::vector<u64>& val, const std::vector<u64>& vec,
             std::vector<u64>& y) {
  const size_t nnz = row.size(), n_blocks = (nnz + kSpmvBlockEntries - 1) / kSpmvBlockEntries;
  std::fill(y.begin(), y.end(), 0);
  if (!n_blocks) return;
  std::vector<u32> crow(2 * n_blocks);
  std::vector<u64> cval(2 * n_blocks);
  for (size_t b = 0; b < n_blocks; ++b) {
    SegPart open[2];
    const size_t base = b * kSpmvBlockEntries, end = base + kSpmvBlockEntries < nnz ? base + kSpmvBlockEntries : nnz;
    run_block(f, row.data(), col.data(), val.data(), base, end, vec.data(), y.data(), open);
    for (int h = 0; h < 2; ++h) {
      crow[2 * b + h] = open[h].row;
      cval[2 * b + h] = open[h].val;
    }
  }
  SegPart run{kSpmvNoRow, 0};
  const size_t n = 2 * n_blocks;
  for (size_t base = 0; base < n; base += kSpmvBlockEntries) {
    SegPart open[2];
    const size_t end = base + kSpmvBlockEntries < n ? base + kSpmvBlockEntries : n;
    run_block(f, crow.data(), nullptr, cval.data(), base, end, nullptr, y.data(), open);
    SegPart first = open[0];
    if (run.row == first.row) first.val = f.add(first.val, run.val);
    else if (run.row != kSpmvNoRow) y[run.row] = run.val;
    if (open[1].row == first.row) {
      run = first;
    } else {
      y[first.row] = first.val;
      run = open[1];
    }
  }
  if (run.row != kSpmvNoRow) y[run.row] = run.val;
}

// triples in any order -> image_sort -> product, against the naive loop over the triples
template <class F>
void one_case(const F& f, const char* name, int log_rows, int log_cols, const std::vector<u32>& ti, const std::vector<u32>& tj) {
  const size_t nnz = ti.size(), n_rows = (size_t)1 << log_rows, n_cols = (size_t)1 << log_cols;
  std::vector<u64> tv(nnz), vec(n_cols), want(n_rows, 0), y(n_rows, 0xDEADBEEF);
  for (auto& v : tv) v = rnd_word(f);
  for (auto& v : vec) v = rnd_word(f);
  for (size_t e = 0; e < nnz; ++e) want[ti[e]] = f.add(want[ti[e]], f.mul(tv[e], vec[tj[e]]));
  std::vector<u32> row(nnz), col(nnz);
  std::vector<u64> val(nnz);
  image_sort(ti.data(), tj.data(), tv.data(), nnz, n_rows, row.data(), col.data(), val.data());
  // sorted, stable, a permutation
  std::map<u32, std::vector<std::pair<u32, u64>>> by_row;
  for (size_t e = 0; e < nnz; ++e) by_row[ti[e]].push_back({tj[e], tv[e]});
  size_t at = 0;
  for (auto& kv : by_row)
    for (auto& cv : kv.second) {
      check(at < nnz && row[at] == kv.first && col[at] == cv.first && val[at] == cv.second, name, at);
      ++at;
    }
  check(at == nnz, name);
  product(f, row, col, val, vec, y);
  for (size_t i = 0; i < n_rows; ++i) check(y[i] == want[i], name, i, nnz);
}

template <class F>
void spmv_cases(const F& f) {
  const int Nb = kSpmvBlockEntries;
  // uniform random rows at the sizes around a block
  for (size_t nnz : {(size_t)0, (size_t)1, (size_t)7, (size_t)8, (size_t)9, (size_t)Nb - 1, (size_t)Nb, (size_t)Nb + 1, (size_t)3 * Nb + 5}) {
    for (int log_rows : {1, 4, 9, 13}) {
      std::vector<u32> ti(nnz), tj(nnz);
      for (size_t e = 0; e < nnz; ++e) {
        ti[e] = (u32)(rnd() % ((size_t)1 << log_rows));
        tj[e] = (u32)(rnd() % 64);
      }
      one_case(f, "random rows", log_rows, 6, ti, tj);
    }
  }
  // one row holds everything: every block starts and ends inside it and holds only that row
  {
    std::vector<u32> ti(3 * Nb + 5, 5), tj(3 * Nb + 5);
    for (auto& j : tj) j = (u32)(rnd() % 16);
    one_case(f, "one row", 4, 4, ti, tj);
  }
  // 2 * Nb carries of one row and more: the carry walk crosses its own chunk boundary inside a row
  {
    const size_t nnz = (size_t)Nb * (Nb + 3) + 11;
    std::vector<u32> ti(nnz, 2), tj(nnz);
    for (size_t e = 0; e < nnz; ++e) tj[e] = (u32)(e % 8);
    for (size_t e = nnz - 40; e < nnz; ++e) ti[e] = 3;
    one_case(f, "one long row, many carries", 2, 3, ti, tj);
  }
  // every row empty but the last; and empty rows between the rows of a block
  {
    std::vector<u32> ti(Nb + 7, (1u << 13) - 1), tj(Nb + 7, 1);
    one_case(f, "only the last row", 13, 2, ti, tj);
    std::vector<u32> si, sj;
    for (u32 i = 0; i < (1u << 13); i += 97)
      for (int k = 0; k < 3; ++k) {
        si.push_back(i);
        sj.push_back((u32)k);
      }
    one_case(f, "rows far apart", 13, 2, si, sj);
  }
  // row ends that fall exactly on block boundaries, and on thread-run boundaries
  {
    std::vector<u32> ti, tj;
    for (u32 r = 0; r < 4; ++r)
      for (int e = 0; e < Nb; ++e) {
        ti.push_back(r);
        tj.push_back((u32)(e % 32));
      }
    one_case(f, "rows = blocks", 2, 5, ti, tj);
    ti.clear();
    tj.clear();
    for (u32 r = 0; r < 600; ++r)
      for (int e = 0; e < kSpmvRun; ++e) {
        ti.push_back(r);
        tj.push_back((u32)e);
      }
    one_case(f, "rows = thread runs", 10, 3, ti, tj);
  }
  // rows of every length 0 .. 40 in turn, duplicated (row, col) among them, given in reverse order
  {
    std::vector<u32> ti, tj;
    for (u32 r = 0; r < 400; ++r)
      for (u32 e = 0; e < r % 41; ++e) {
        ti.push_back(399 - r);
        tj.push_back(e % 5);
      }
    one_case(f, "mixed lengths", 9, 3, ti, tj);
  }
}

// zc_fold4 and zc_accumulate against the definition: H(t) = sum_i e_i(t) (a_i(t) b_i(t) - c_i(t)), u_i(t) = u[2i] + t (u[2i+1] - u[2i])
template <class F>
void zc_cases(const F& f) {
  for (int rep = 0; rep < 200; ++rep) {
    const int n = 1 + (int)(rnd() % 9);
    const u64 r = rnd_word(f);
    std::vector<u64> T[4];
    for (auto& t : T) {
      t.resize(4 * (size_t)n);
      for (auto& v : t) v = rnd_word(f);
    }
    typename F::Acc acc[4];
    for (auto& a : acc) f.acc_zero(a);
    u64 want[4] = {0, 0, 0, 0};
    for (int i = 0; i < n; ++i) {
      u64 p[4][2];
      for (int k = 0; k < 4; ++k) {
        const u64 u[4] = {T[k][4 * i], T[k][4 * i + 1], T[k][4 * i + 2], T[k][4 * i + 3]};
        zc_fold4(f, r, u, p[k]);
        for (int h = 0; h < 2; ++h)
          check(p[k][h] == f.add(u[2 * h], f.mul(r, f.sub(u[2 * h + 1], u[2 * h]))), "zc_fold4");
      }
      zc_accumulate(f, acc, p[0], p[1], p[2], p[3]);
      for (int t = 0; t < 4; ++t) {
        u64 at[4];
        for (int k = 0; k < 4; ++k) {
          u64 x = p[k][0];
          const u64 d = f.sub(p[k][1], p[k][0]);
          for (int q = 0; q < t; ++q) x = f.add(x, d);
          at[k] = x;
        }
        want[t] = f.add(want[t], f.mul(at[0], f.sub(f.mul(at[1], at[2]), at[3])));
      }
    }
    for (int t = 0; t < 4; ++t) check(f.acc_get(acc[t]) == want[t], "zc_accumulate", (size_t)rep, (size_t)t);
  }
}

}  // namespace

int main() {
  FieldParams gp, wp;
  field_params_from_modulus(GoldilocksMont::P, &gp);
  field_params_from_modulus(0xFFFFFFFFFFFFFFC5ull, &wp);   // 2^64 - 59
  const GoldilocksMont g(gp);
  const MontGeneric w(wp);
  spmv_cases(g);
  spmv_cases(w);
  zc_cases(g);
  zc_cases(w);
  if (failures) {
    printf("%d failures\n", failures);
    return 1;
  }
  printf("r1cs host harness ok\n");
  return 0;
}
