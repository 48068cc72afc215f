// Host build of the per-item and host-finish code of thaler-study_amd/csrc/kernels/fraction.hpp (the tree item of fr_tree_kernel
// at LV = 1, 2, 3, general and all-ones; the cubic pass's items, fr_accumulate and fr_accumulate_ones; fr_host_sums and
// fr_host_rounds, which the engine runs for the small layers and the tails), compiled for the CPU and run stand-alone against
// naive loops in 128-bit integers on edge words, both fields.  Every array is allocated at its exact size: this is the build
// that runs under -fsanitize=address,undefined.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../thaler-study_amd/csrc/kernels/fraction.hpp"
using namespace sc;

namespace {

typedef unsigned __int128 u128;

u64 rnd_state = 0x9E3779B9;
u64 rnd() { return rnd_state = splitmix64(rnd_state); }

// a Montgomery word below p: an edge word (0, 1, p-1, p-2, (p-1)/2, R mod p, 2^32-1, 2^32, 2^32+1, 2^63, 0xFFFFFFFF00000000) in
// about a quarter of the draws
template <class F>
u64 rnd_word(const F& f) {
  const u64 p = f.modulus();
  const u64 edge[11] = {0, 1, p - 1, p - 2, (p - 1) / 2, f.one(), 0xFFFFFFFFull, 0x100000000ull, 0x100000001ull, 0x8000000000000000ull, 0xFFFFFFFF00000000ull};
  const u64 r = rnd();
  return (r & 3) == 0 ? edge[(r >> 2) % 11] % p : (r >> 2) % p;
}

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
  u64 addc(u64 a, u64 b) const { return (u64)(((u128)a + b) % p); }
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

// fr_tree_item against the definition, level by level: a node is (p_a q_b + p_b q_a, q_a q_b) of the two nodes at distance h
template <class F, int LV, bool ONES>
void tree_cases(const F& f) {
  const Naive nv = naive_of(f);
  constexpr int W = 1 << LV;
  for (int rep = 0; rep < 400; ++rep) {
    u64 pin[W], qin[W], pout[W], qout[W];
    for (int j = 0; j < W; ++j) {
      pin[j] = ONES ? 0x1234 : rnd_word(f);   // (ONES: not read)
      qin[j] = rnd_word(f);
    }
    if (rep % 7 == 0) qin[rnd() % W] = 0;
    pout[0] = qout[0] = 0x5A5A5A5A5A5A5A5Aull;
    fr_tree_item<F, LV, ONES>(f, pin, qin, pout, qout);
    check(pout[0] == 0x5A5A5A5A5A5A5A5Aull && qout[0] == 0x5A5A5A5A5A5A5A5Aull, "fr_tree_item leaves [0]");
    // the naive heap: level W holds the inputs
    std::vector<u64> np(2 * W), nq(2 * W);
    for (int j = 0; j < W; ++j) {
      np[W + j] = ONES ? 1 % nv.p : nv.canon(pin[j]);
      nq[W + j] = nv.canon(qin[j]);
    }
    for (int h = W / 2; h >= 1; h /= 2)
      for (int j = 0; j < h; ++j) {
        const int a = 2 * h + j, b = 3 * h + j;
        np[h + j] = nv.addc(nv.mulc(np[a], nq[b]), nv.mulc(np[b], nq[a]));
        nq[h + j] = nv.mulc(nq[a], nq[b]);
        check(nv.canon(pout[h + j]) == np[h + j] && pout[h + j] < nv.p, "fr_tree_item p", (size_t)LV, (size_t)(h + j));
        check(nv.canon(qout[h + j]) == nq[h + j] && qout[h + j] < nv.p, "fr_tree_item q", (size_t)LV, (size_t)(h + j));
      }
  }
}

// H(t) = sum_i e_i(t) (pl_i(t) qr_i(t) + pr_i(t) ql_i(t) + lambda ql_i(t) qr_i(t)); tb in the order kFrE .. kFrPR, 3 tables: pl = pr = 1
void naive_sums(const Naive& nv, const std::vector<std::vector<u64>>& tb, u64 lambda, u64 (&out)[4]) {
  const u64 lam = nv.canon(lambda);
  for (int t = 0; t < 4; ++t) {
    u64 h = 0;
    for (size_t i = 0; i < tb[0].size() / 2; ++i) {
      u64 at[5] = {0, 0, 0, 1 % nv.p, 1 % nv.p};
      for (size_t k = 0; k < tb.size(); ++k) {
        const u64 lo = nv.canon(tb[k][2 * i]), hi = nv.canon(tb[k][2 * i + 1]);
        at[k] = nv.addc(lo, nv.mulc((u64)t, nv.subc(hi, lo)));
      }
      const u64 inner = nv.addc(nv.addc(nv.mulc(at[kFrPL], at[kFrQR]), nv.mulc(at[kFrPR], at[kFrQL])), nv.mulc(lam, nv.mulc(at[kFrQL], at[kFrQR])));
      h = nv.addc(h, nv.mulc(at[kFrE], inner));
    }
    out[t] = h;
  }
}

template <class F>
std::vector<std::vector<u64>> random_tables(const F& f, int n_tables, size_t len) {
  std::vector<std::vector<u64>> tb((size_t)n_tables, std::vector<u64>(len));
  for (auto& t : tb)
    for (auto& v : t) v = rnd_word(f);
  return tb;
}

std::vector<u64*> pointers(std::vector<std::vector<u64>>& tb) {
  std::vector<u64*> out;
  for (auto& t : tb) out.push_back(t.data());
  return out;
}

// fr_accumulate and fr_accumulate_ones (through fr_host_sums) against the definition
template <class F>
void accumulate_cases(const F& f) {
  const Naive nv = naive_of(f);
  for (int rep = 0; rep < 300; ++rep) {
    const size_t n = 1 + rnd() % 17;
    const int n_tables = (rep & 1) ? 3 : 5;
    auto tb = random_tables(f, n_tables, 2 * n);
    const u64 lambda = rnd_word(f);
    u64 got[4], want[4];
    auto ptr = pointers(tb);
    fr_host_sums(f, ptr.data(), n_tables, lambda, n, got);
    naive_sums(nv, tb, lambda, want);
    for (int t = 0; t < 4; ++t) check(nv.canon(got[t]) == want[t] && got[t] < nv.p, "fr_accumulate", (size_t)rep, (size_t)t);
  }
}

template <class F>
std::vector<u64> naive_fold(const F& f, const Naive& nv, const std::vector<u64>& u, u64 c) {
  std::vector<u64> o(u.size() / 2);
  for (size_t i = 0; i < o.size(); ++i) {
    const u64 lo = nv.canon(u[2 * i]), hi = nv.canon(u[2 * i + 1]);
    o[i] = f.to_mont(nv.addc(lo, nv.mulc(nv.canon(c), nv.subc(hi, lo))));
  }
  return o;
}

// fr_host_rounds - every round's message, the folds, the finals, the `given` first message and a refusing next() - against
// naive rounds, over five and over three tables
template <class F>
void rounds_cases(const F& f) {
  const Naive nv = naive_of(f);
  for (int k = 0; k <= 7; ++k)
    for (int rep = 0; rep < 12; ++rep) {
      const size_t len = (size_t)1 << k;
      const int n_tables = (rep & 2) ? 3 : 5;
      const auto start = random_tables(f, n_tables, len);
      const u64 lambda = rnd_word(f);
      std::vector<u64> cs((size_t)k);
      for (auto& v : cs) v = rnd_word(f);
      // the naive rounds
      std::vector<std::vector<u64>> msgs;
      auto naive = start;
      for (int j = 0; j < k; ++j) {
        u64 m[4];
        naive_sums(nv, naive, lambda, m);
        msgs.push_back(std::vector<u64>(m, m + 4));
        for (auto& t : naive) t = naive_fold(f, nv, t, cs[(size_t)j]);
      }
      const size_t first = rnd() % 5;
      const bool give = k > 0 && (rep & 1);
      u64 given[4] = {0, 0, 0, 0};
      if (give)
        for (int t = 0; t < 4; ++t) given[t] = f.to_mont(msgs[0][(size_t)t]);
      auto host = start;
      auto ptr = pointers(host);
      std::vector<u64> drawn(first + (size_t)k);
      size_t calls = 0;
      const bool ok = fr_host_rounds(f, ptr.data(), n_tables, lambda, k, first, give ? given : nullptr, drawn.data(), [&](size_t round, const u64* msg, u64* c) {
        const size_t j = round - first;
        check(j == calls && j < (size_t)k, "fr_host_rounds order", j, calls);
        for (int t = 0; t < 4; ++t) check(nv.canon(msg[t]) == msgs[j][(size_t)t], "fr_host_rounds message", j, (size_t)t);
        calls += 1;
        *c = cs[j];
        return true;
      });
      check(ok && calls == (size_t)k, "fr_host_rounds ran every round", (size_t)k, calls);
      for (int j = 0; j < k; ++j) check(drawn[first + (size_t)j] == cs[(size_t)j], "fr_host_rounds challenges", (size_t)j);
      for (int q = 1; q < n_tables; ++q) check(host[(size_t)q][0] == naive[(size_t)q][0], "fr_host_rounds finals", (size_t)k, (size_t)q);
      // a next() that refuses at round `stop` ends the call there
      if (k > 0) {
        const size_t stop = rnd() % (size_t)k;
        auto again = start;
        auto ptr2 = pointers(again);
        std::vector<u64> qd((size_t)k);
        size_t seen = 0;
        const bool went = fr_host_rounds(f, ptr2.data(), n_tables, lambda, k, 0, nullptr, qd.data(), [&](size_t round, const u64*, u64* c) {
          seen += 1;
          *c = cs[round];
          return round != stop;
        });
        check(!went && seen == stop + 1, "fr_host_rounds stops", stop, seen);
      }
    }
}

template <class F>
void all_cases(const F& f) {
  tree_cases<F, 1, false>(f);
  tree_cases<F, 1, true>(f);
  tree_cases<F, 2, false>(f);
  tree_cases<F, 2, true>(f);
  tree_cases<F, 3, false>(f);
  tree_cases<F, 3, true>(f);
  accumulate_cases(f);
  rounds_cases(f);
}

}  // namespace

int main() {
  FieldParams gp, wp;
  field_params_from_modulus(GoldilocksMont::P, &gp);
  field_params_from_modulus(0xFFFFFFFFFFFFFFC5ull, &wp);   // 2^64 - 59
  const GoldilocksMont g(gp);
  const MontGeneric gm(gp);                                  // what the engine's host finish runs on every field
  const MontGeneric w(wp);
  all_cases(g);
  all_cases(gm);
  all_cases(w);
  if (failures) {
    printf("%d failures\n", failures);
    return 1;
  }
  printf("fr host harness ok\n");
  return 0;
}
