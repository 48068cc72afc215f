// Host build of the per-element code of thaler-study_amd/csrc/kernels/spark.hpp (the gather item of spark_gather_kernel at both of
// its widths; the tuple item of spark_tuple_kernel with a key stream and with the index as the key, on the edge words 0, 1 and
// p - 1 for alpha, beta and v; the index-to-Montgomery step of spark_index_kernel; the length, validation and padding routines of
// sc_spark_create), compiled for the CPU and run stand-alone against naive loops in 128-bit integers, both fields.  Every array is
// allocated at its exact size: this is the build that runs under -fsanitize=address,undefined.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../thaler-study_amd/csrc/kernels/spark.hpp"
using namespace sc;

namespace {

typedef unsigned __int128 u128;

u64 rnd_state = 0x51A4C;
u64 rnd() { return rnd_state = splitmix64(rnd_state); }

int failures = 0;
void check(bool ok, const char* what, size_t a = 0, size_t b = 0) {
  if (!ok) {
    if (++failures < 20) printf("FAIL %s (%zu, %zu)\n", what, a, b);
  }
}

// the naive side works on CANONICAL residues with 128-bit products
struct Naive {
  u64 p, rinv;   // rinv = 2^-64 mod p
  u64 mulc(u64 a, u64 b) const { return (u64)((u128)a * b % p); }
  u64 subc(u64 a, u64 b) const { return (u64)(((u128)a + p - b) % p); }
  u64 canon(u64 w) const { return mulc(w, rinv); }
};
template <class F>
Naive naive_of(const F& f) {
  Naive nv;
  nv.p = f.modulus();
  nv.rinv = f.from_mont(1);   // 1 * R^-1
  return nv;
}

// a Montgomery word below p, an edge word in about a third of the draws
template <class F>
u64 rnd_word(const F& f) {
  const u64 p = f.modulus();
  const u64 edge[8] = {0, 1, p - 1, p - 2, (p - 1) / 2, f.one(), 0xFFFFFFFFull, 0x8000000000000000ull};
  const u64 r = rnd();
  return r % 3 == 0 ? edge[(r >> 2) % 8] % p : (r >> 2) % p;
}

// spark_key_word: the Montgomery word of an integer below 2^28 - and of the largest u32, which no index reaches
template <class F>
void key_cases(const F& f) {
  const Naive nv = naive_of(f);
  const u32 fixed[10] = {0, 1, 2, 3, 255, 256, (1u << 28) - 1, 1u << 28, 0x7FFFFFFFu, 0xFFFFFFFFu};
  for (int rep = 0; rep < 2000; ++rep) {
    const u32 k = rep < 10 ? fixed[rep] : (u32)(rnd() >> (32 + rnd() % 32));
    const u64 w = spark_key_word(f, k);
    check(w < nv.p && nv.canon(w) == (u64)k % nv.p, "spark_key_word", (size_t)k);
  }
}

// spark_gather_item at S = 4 (a thread's unit) and S = 2 (the tail of a list of two): the words of the table, as they are
template <class F, int S>
void gather_cases(const F& f) {
  for (int log_m = 0; log_m <= 9; ++log_m) {
    const size_t m_len = (size_t)1 << log_m;
    std::vector<u64> table(m_len);
    for (auto& v : table) v = rnd_word(f);
    for (int rep = 0; rep < 50; ++rep) {
      u32 idx[S];
      u64 out[S];
      for (int s = 0; s < S; ++s) idx[s] = rep == 0 ? 0 : rep == 1 ? (u32)(m_len - 1) : (u32)(rnd() % m_len);
      spark_gather_item<S>(table.data(), idx, out);
      for (int s = 0; s < S; ++s) check(out[s] == table[idx[s]], "spark_gather_item", (size_t)log_m, (size_t)s);
    }
  }
}

// spark_tuple_item: alpha - key - beta v, the key from a stream and the key as the index, alpha, beta, v over the edge words
template <class F>
void tuple_cases(const F& f) {
  const Naive nv = naive_of(f);
  const u64 p = nv.p;
  const u64 edge[3] = {0, 1 % p, p - 1};   // canonical
  // a table of eight entries under the index as key, entry by entry, every combination of edge words
  for (int ia = 0; ia < 4; ++ia)
    for (int ib = 0; ib < 4; ++ib)
      for (int iv = 0; iv < 4; ++iv) {
        const u64 alpha = ia < 3 ? f.to_mont(edge[ia]) : rnd_word(f), beta = ib < 3 ? f.to_mont(edge[ib]) : rnd_word(f);
        std::vector<u64> v(8), out(8);
        std::vector<u32> key(8);
        for (size_t i = 0; i < 8; ++i) {
          v[i] = iv < 3 ? f.to_mont(edge[iv]) : rnd_word(f);
          key[i] = i == 0 ? 0 : i == 1 ? (1u << 28) - 1 : (u32)(rnd() % (1u << 28));
        }
        for (int iota = 0; iota < 2; ++iota) {
          for (size_t i = 0; i < 8; ++i) out[i] = spark_tuple_item(f, alpha, beta, iota ? (u32)i : key[i], v[i]);
          for (size_t i = 0; i < 8; ++i) {
            const u64 k = (u64)(iota ? (u32)i : key[i]) % p;
            const u64 want = nv.subc(nv.subc(nv.canon(alpha), k), nv.mulc(nv.canon(beta), nv.canon(v[i])));
            check(out[i] < p && nv.canon(out[i]) == want, "spark_tuple_item", (size_t)(16 * ia + 4 * ib + iv), i);
          }
        }
      }
}

// spark_log_len, spark_first_bad and spark_pad
void list_cases(u64 p) {
  const size_t nnzs[12] = {1, 2, 3, 4, 5, 7, 8, 9, 1023, 1024, 1025, 8191};
  const int logs[12] = {1, 1, 2, 2, 3, 3, 3, 4, 10, 10, 11, 13};
  for (int c = 0; c < 12; ++c) {
    const size_t nnz = nnzs[c];
    check(spark_log_len(nnz) == logs[c], "spark_log_len", nnz);
    const int a = 1 + (int)(rnd() % 9), b = 1 + (int)(rnd() % 9);
    std::vector<u32> row(nnz), col(nnz);
    std::vector<u64> val(nnz);
    for (size_t k = 0; k < nnz; ++k) {
      row[k] = (u32)(rnd() % ((u64)1 << a));
      col[k] = (u32)(rnd() % ((u64)1 << b));
      val[k] = rnd() % p;
    }
    row[0] = ((u32)1 << a) - 1;
    col[nnz - 1] = ((u32)1 << b) - 1;
    val[nnz / 2] = p - 1;
    check(spark_first_bad(row.data(), col.data(), val.data(), nnz, a, b, p) == nnz, "spark_first_bad accepts", nnz);
    // one bad entry: a row, a column and a value just outside, at the first, a middle and the last entry
    const size_t at[3] = {0, nnz / 2, nnz - 1};
    for (int w = 0; w < 3; ++w)
      for (int q = 0; q < 3; ++q) {
        std::vector<u32> r2 = row, c2 = col;
        std::vector<u64> v2 = val;
        if (w == 0) r2[at[q]] = (u32)1 << a;
        else if (w == 1) c2[at[q]] = (u32)1 << b;
        else v2[at[q]] = p;
        check(spark_first_bad(r2.data(), c2.data(), v2.data(), nnz, a, b, p) == at[q], "spark_first_bad finds", nnz, (size_t)(3 * w + q));
      }
    // the padding
    const size_t n = (size_t)1 << spark_log_len(nnz);
    std::vector<u32> prow(n), pcol(n);
    std::vector<u64> pval(n);
    spark_pad(row.data(), col.data(), val.data(), nnz, n, prow.data(), pcol.data(), pval.data());
    for (size_t k = 0; k < n; ++k) {
      const bool in = k < nnz;
      check(prow[k] == (in ? row[k] : 0) && pcol[k] == (in ? col[k] : 0) && pval[k] == (in ? val[k] : 0), "spark_pad", nnz, k);
    }
  }
}

template <class F>
void all_cases(const F& f) {
  key_cases(f);
  gather_cases<F, 4>(f);
  gather_cases<F, 2>(f);
  tuple_cases(f);
  list_cases(f.modulus());
}

}  // namespace

int main() {
  FieldParams gp, wp;
  field_params_from_modulus(GoldilocksMont::P, &gp);
  field_params_from_modulus(0xFFFFFFFFFFFFFFC5ull, &wp);   // 2^64 - 59
  const GoldilocksMont g(gp);
  const MontGeneric gm(gp);
  const MontGeneric w(wp);
  all_cases(g);
  all_cases(gm);
  all_cases(w);
  if (failures) {
    printf("%d failures\n", failures);
    return 1;
  }
  printf("spark host harness ok\n");
  return 0;
}
