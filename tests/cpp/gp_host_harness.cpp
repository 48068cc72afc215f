// Host build of the per-item and host-finish code of thaler-study_amd/csrc/kernels/grand_product.hpp (the tree item of
// gp_tree_kernel at LV = 1, 2, 3; the cubic pass's item, gp_accumulate; gp_host_eq, gp_host_fold, gp_host_sums and
// gp_host_rounds, which the engine runs for the small layers and the tails), compiled for the CPU and run stand-alone against
// naive loops in 128-bit integers on edge words, both fields.  Every array is allocated at its exact size: this is the build
// that runs under -fsanitize=address,undefined.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../thaler-study_amd/csrc/kernels/grand_product.hpp"
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

// gp_tree_item against the definition: out[h + j] = prod over the inputs j, j + h, j + 2h, ..
template <class F, int LV>
void tree_cases(const F& f) {
  const Naive nv = naive_of(f);
  constexpr int W = 1 << LV;
  for (int rep = 0; rep < 400; ++rep) {
    u64 in[W], out[W];
    for (int j = 0; j < W; ++j) in[j] = rnd_word(f);
    if (rep % 7 == 0) in[rnd() % W] = 0;
    out[0] = 0x5A5A5A5A5A5A5A5Aull;
    gp_tree_item<F, LV>(f, in, out);
    check(out[0] == 0x5A5A5A5A5A5A5A5Aull, "gp_tree_item leaves out[0]");
    for (int h = W / 2; h >= 1; h /= 2)
      for (int j = 0; j < h; ++j) {
        u64 want = 1 % nv.p;
        for (int q = j; q < W; q += h) want = nv.mulc(want, nv.canon(in[q]));
        check(nv.canon(out[h + j]) == want, "gp_tree_item", (size_t)LV, (size_t)(h + j));
      }
  }
}

template <class F>
void naive_sums(const Naive& nv, const std::vector<u64>& e, const std::vector<u64>& l, const std::vector<u64>& r, u64 (&out)[4]) {
  for (int t = 0; t < 4; ++t) {
    u64 h = 0;
    for (size_t i = 0; i < e.size() / 2; ++i) {
      u64 at[3];
      const std::vector<u64>* tb[3] = {&e, &l, &r};
      for (int k = 0; k < 3; ++k) {
        const u64 lo = nv.canon((*tb[k])[2 * i]), hi = nv.canon((*tb[k])[2 * i + 1]);
        at[k] = nv.addc(lo, nv.mulc((u64)t, nv.subc(hi, lo)));
      }
      h = nv.addc(h, nv.mulc(at[0], nv.mulc(at[1], at[2])));
    }
    out[t] = h;
  }
}

// gp_accumulate (through gp_host_sums) against H(t) = sum_i e_i(t) l_i(t) r_i(t)
template <class F>
void accumulate_cases(const F& f) {
  const Naive nv = naive_of(f);
  for (int rep = 0; rep < 300; ++rep) {
    const size_t n = 1 + rnd() % 17;
    std::vector<u64> e(2 * n), l(2 * n), r(2 * n);
    for (size_t i = 0; i < 2 * n; ++i) {
      e[i] = rnd_word(f);
      l[i] = rnd_word(f);
      r[i] = rnd_word(f);
    }
    u64 got[4], want[4];
    gp_host_sums(f, e.data(), l.data(), r.data(), n, got);
    naive_sums<F>(nv, e, l, r, want);
    for (int t = 0; t < 4; ++t) check(nv.canon(got[t]) == want[t], "gp_accumulate", (size_t)rep, (size_t)t);
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

// gp_host_eq against the definition, and gp_host_rounds - every round's message, the folds, the finals, the `given` first
// message and a refusing next() - against naive rounds
template <class F>
void rounds_cases(const F& f) {
  const Naive nv = naive_of(f);
  for (int k = 0; k <= 7; ++k)
    for (int rep = 0; rep < 12; ++rep) {
      const size_t len = (size_t)1 << k;
      std::vector<u64> z((size_t)k), e(len), l(len), r(len);
      for (auto& v : z) v = rnd_word(f);
      for (auto& v : l) v = rnd_word(f);
      for (auto& v : r) v = rnd_word(f);
      gp_host_eq(f, z.data(), k, e.data());
      for (size_t i = 0; i < len; ++i) {
        u64 want = 1 % nv.p;
        for (int j = 0; j < k; ++j) {
          const u64 zj = nv.canon(z[(size_t)j]);
          want = nv.mulc(want, ((i >> j) & 1) ? zj : nv.subc(1 % nv.p, zj));
        }
        check(nv.canon(e[i]) == want, "gp_host_eq", (size_t)k, i);
      }
      std::vector<u64> cs((size_t)k);
      for (auto& v : cs) v = rnd_word(f);
      // the naive rounds
      std::vector<std::vector<u64>> msgs;
      std::vector<u64> ne = e, nl = l, nr = r;
      for (int j = 0; j < k; ++j) {
        u64 m[4];
        naive_sums<F>(nv, ne, nl, nr, m);
        msgs.push_back(std::vector<u64>(m, m + 4));
        ne = naive_fold(f, nv, ne, cs[(size_t)j]);
        nl = naive_fold(f, nv, nl, cs[(size_t)j]);
        nr = naive_fold(f, nv, nr, cs[(size_t)j]);
      }
      const size_t first = rnd() % 5;
      const bool give = k > 0 && (rep & 1);
      u64 given[4] = {0, 0, 0, 0};
      if (give)
        for (int t = 0; t < 4; ++t) given[t] = f.to_mont(msgs[0][(size_t)t]);
      std::vector<u64> he = e, hl = l, hr = r, drawn(first + (size_t)k);
      size_t calls = 0;
      const bool ok = gp_host_rounds(f, he.data(), hl.data(), hr.data(), k, first, give ? given : nullptr, drawn.data(), [&](size_t round, const u64* msg, u64* c) {
        const size_t j = round - first;
        check(j == calls && j < (size_t)k, "gp_host_rounds order", j, calls);
        for (int t = 0; t < 4; ++t) check(nv.canon(msg[t]) == msgs[j][(size_t)t], "gp_host_rounds message", j, (size_t)t);
        calls += 1;
        *c = cs[j];
        return true;
      });
      check(ok && calls == (size_t)k, "gp_host_rounds ran every round", (size_t)k, calls);
      for (int j = 0; j < k; ++j) check(drawn[first + (size_t)j] == cs[(size_t)j], "gp_host_rounds challenges", (size_t)j);
      check(hl[0] == nl[0] && hr[0] == nr[0], "gp_host_rounds finals", (size_t)k, (size_t)rep);
      // a next() that refuses at round `stop` ends the call there
      if (k > 0) {
        const size_t stop = rnd() % (size_t)k;
        std::vector<u64> qe = e, ql = l, qr = r, qd((size_t)k);
        size_t seen = 0;
        const bool went = gp_host_rounds(f, qe.data(), ql.data(), qr.data(), k, 0, nullptr, qd.data(), [&](size_t round, const u64*, u64* c) {
          seen += 1;
          *c = cs[round];
          return round != stop;
        });
        check(!went && seen == stop + 1, "gp_host_rounds stops", stop, seen);
      }
    }
}

template <class F>
void all_cases(const F& f) {
  tree_cases<F, 1>(f);
  tree_cases<F, 2>(f);
  tree_cases<F, 3>(f);
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
  printf("gp host harness ok\n");
  return 0;
}
