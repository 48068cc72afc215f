// Host build of the per-element code of thaler-study_amd/csrc/kernels/ext_sumprod.hpp (the product in K = F_p[X] / (X^2 - w), the
// two folds, the accumulate with its nine-to-six map, and the host rounds that finish a proof), compiled for the CPU and run
// stand-alone against naive schoolbook loops in 128-bit integers on the component words 0, 1 and p - 1, both fields.  Every array
// is allocated at its exact size: this is the build that runs under -fsanitize=address,undefined.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../thaler-study_amd/csrc/kernels/ext_sumprod.hpp"
using namespace sc;

namespace {

typedef unsigned __int128 u128;

u64 rnd_state = 0x457874;
u64 rnd() { return rnd_state = splitmix64(rnd_state); }

int failures = 0;
void check(bool ok, const char* what, size_t a = 0, size_t b = 0) {
  if (!ok) {
    if (++failures < 20) printf("FAIL %s (%zu, %zu)\n", what, a, b);
  }
}

// the naive side works on CANONICAL residues with 128-bit products and plain schoolbook K-products
struct K2 {
  u64 c[2];
};
struct Naive {
  u64 p, rinv, w;   // rinv = 2^-64 mod p; w canonical
  u64 mulc(u64 a, u64 b) const { return (u64)((u128)a * b % p); }
  u64 addc(u64 a, u64 b) const { return (u64)(((u128)a + b) % p); }
  u64 subc(u64 a, u64 b) const { return (u64)(((u128)a + p - b) % p); }
  u64 canon(u64 x) const { return mulc(x, rinv); }
  K2 kadd(K2 a, K2 b) const { return K2{{addc(a.c[0], b.c[0]), addc(a.c[1], b.c[1])}}; }
  K2 ksub(K2 a, K2 b) const { return K2{{subc(a.c[0], b.c[0]), subc(a.c[1], b.c[1])}}; }
  K2 kmul(K2 a, K2 b) const {
    return K2{{addc(mulc(a.c[0], b.c[0]), mulc(w, mulc(a.c[1], b.c[1]))), addc(mulc(a.c[0], b.c[1]), mulc(a.c[1], b.c[0]))}};
  }
  K2 kfold(K2 r, K2 u0, K2 u1) const { return kadd(u0, kmul(r, ksub(u1, u0))); }
};
template <class F>
Naive naive_of(const F& f, u64 w_canon) {
  Naive nv;
  nv.p = f.modulus();
  nv.rinv = f.from_mont(1);   // 1 * R^-1
  nv.w = w_canon;
  return nv;
}
template <class F>
bool same(const F& f, const Naive& nv, const u64 (&got)[2], K2 want) {
  return got[0] < nv.p && got[1] < nv.p && nv.canon(got[0]) == want.c[0] && nv.canon(got[1]) == want.c[1];
}

// a canonical word: an edge word (0, 1, p - 1) for sel < 3, else random
u64 pick(u64 p, int sel) { return sel == 0 ? 0 : sel == 1 ? 1 % p : sel == 2 ? p - 1 : rnd() % p; }
// sel < 3: mostly that edge word; otherwise a mix of the edge words and random ones
u64 pick_mixed(u64 p, int sel) { return pick(p, sel < 3 ? (rnd() % 4 == 0 ? 3 : sel) : (int)(rnd() % 6 < 3 ? rnd() % 3 : 3)); }

// ext_mul and both folds on every combination of the component words 0, 1, p - 1 and a random one
template <class F>
void element_cases(const F& f, u64 w_canon) {
  const Naive nv = naive_of(f, w_canon);
  const u64 w = f.to_mont(w_canon);
  for (int code = 0; code < 4 * 4 * 4 * 4 * 4 * 4; ++code) {
    u64 cw[6], mw[6];
    for (int k = 0, c = code; k < 6; ++k, c /= 4) {
      cw[k] = pick(nv.p, c % 4);
      mw[k] = f.to_mont(cw[k]);
    }
    const K2 x = {{cw[0], cw[1]}}, y = {{cw[2], cw[3]}}, z = {{cw[4], cw[5]}};
    const u64 mx[2] = {mw[0], mw[1]}, my[2] = {mw[2], mw[3]}, mz[2] = {mw[4], mw[5]};
    u64 o[2];
    ext_mul(f, w, mx, my, o);
    check(same(f, nv, o, nv.kmul(x, y)), "ext_mul", (size_t)code);
    ext_fold(f, w, mx, my, mz, o);   // r = x, u0 = y, u1 = z
    check(same(f, nv, o, nv.kfold(x, y, z)), "ext_fold", (size_t)code);
    ext_fold_base(f, mx, my[0], mz[0], o);
    check(same(f, nv, o, nv.kfold(x, K2{{y.c[0], 0}}, K2{{z.c[0], 0}})), "ext_fold_base", (size_t)code);
  }
  // X^2 = w
  const u64 X[2] = {0, f.one()};
  u64 o[2];
  ext_mul(f, w, X, X, o);
  check(o[0] == w && o[1] == 0, "X^2 = w");
}

// the item of the pass (fold of a unit of four entries per table, accumulate over T pairs, the nine-to-six map) in its base-in and
// extension-in forms - and ext_host_rounds, a whole proof on the host, against the naive sums, folds and finals
template <class F>
void sumprod_cases(const F& f, u64 w_canon, int n, int T, int sel) {
  const Naive nv = naive_of(f, w_canon);
  const u64 w = f.to_mont(w_canon);
  const size_t len = (size_t)1 << n;
  // 2T tables of K elements: planes [q][component][index], canonical and Montgomery; the base tables are their c0 planes
  std::vector<std::vector<std::vector<u64>>> ct(2 * T, std::vector<std::vector<u64>>(2, std::vector<u64>(len))), mt = ct;
  for (int q = 0; q < 2 * T; ++q)
    for (int c = 0; c < 2; ++c)
      for (size_t i = 0; i < len; ++i) {
        ct[q][c][i] = pick_mixed(nv.p, sel);
        mt[q][c][i] = f.to_mont(ct[q][c][i]);
      }
  const K2 cr = {{pick(nv.p, sel % 4), pick(nv.p, (sel + 1) % 4)}};
  const u64 r[2] = {f.to_mont(cr.c[0]), f.to_mont(cr.c[1])};
  if (n >= 2) {
    for (int base = 0; base < 2; ++base) {
      typename F::Acc acc[9];
      for (int s = 0; s < 9; ++s) f.acc_zero(acc[s]);
      K2 want[3] = {{{0, 0}}, {{0, 0}}, {{0, 0}}};
      for (size_t i = 0; i < len / 4; ++i)
        for (int t = 0; t < T; ++t) {
          u64 p2[2][2][2];
          K2 c2[2][2];
          for (int k = 0; k < 2; ++k) {
            const int q = k ? T + t : t;
            for (int h = 0; h < 2; ++h) {
              const size_t e = 4 * i + 2 * h;
              K2 u0 = {{ct[q][0][e], base ? 0 : ct[q][1][e]}}, u1 = {{ct[q][0][e + 1], base ? 0 : ct[q][1][e + 1]}};
              if (base) {
                ext_fold_base(f, r, mt[q][0][e], mt[q][0][e + 1], p2[k][h]);
              } else {
                const u64 m0[2] = {mt[q][0][e], mt[q][1][e]}, m1[2] = {mt[q][0][e + 1], mt[q][1][e + 1]};
                ext_fold(f, w, r, m0, m1, p2[k][h]);
              }
              c2[k][h] = nv.kfold(cr, u0, u1);
              check(same(f, nv, p2[k][h], c2[k][h]), base ? "unit fold, base in" : "unit fold, extension in", i, (size_t)t);
            }
          }
          ext_accumulate(f, acc, p2[0], p2[1]);
          want[0] = nv.kadd(want[0], nv.kmul(c2[0][0], c2[1][0]));
          want[1] = nv.kadd(want[1], nv.kmul(c2[0][1], c2[1][1]));
          const K2 a2 = nv.ksub(nv.kadd(c2[0][1], c2[0][1]), c2[0][0]), b2 = nv.ksub(nv.kadd(c2[1][1], c2[1][1]), c2[1][0]);
          want[2] = nv.kadd(want[2], nv.kmul(a2, b2));
        }
      u64 cells[9];
      for (int s = 0; s < 9; ++s) cells[s] = f.acc_get(acc[s]);
      for (int s = 0; s < 3; ++s) {
        const u64 got[2] = {ext_cells_to_word(f, w, cells, 2 * s), ext_cells_to_word(f, w, cells, 2 * s + 1)};
        check(same(f, nv, got, want[s]), "ext_accumulate and the nine-to-six map", (size_t)n, (size_t)s);
      }
    }
  }
  // the host rounds over the whole tables: from base words (the c0 planes; the c1 planes zero) and from extension tables
  for (int base = 0; base < 2; ++base) {
    std::vector<std::vector<u64>> planes(4 * T, std::vector<u64>(len, 0));
    std::vector<std::vector<K2>> nt(2 * T, std::vector<K2>(len));
    std::vector<u64*> pl(4 * T);
    for (int q = 0; q < 2 * T; ++q) {
      for (size_t i = 0; i < len; ++i) {
        planes[2 * q][i] = mt[q][0][i];
        planes[2 * q + 1][i] = base ? 0 : mt[q][1][i];
        nt[q][i] = K2{{ct[q][0][i], base ? 0 : ct[q][1][i]}};
      }
      pl[2 * q] = planes[2 * q].data();
      pl[2 * q + 1] = planes[2 * q + 1].data();
    }
    std::vector<u64> rs(2 * n);
    std::vector<K2> crs(n);
    bool ok = true;
    auto next = [&](size_t round, const u64* msg, u64* out) {
      const size_t units = nt[0].size() / 2;
      K2 want[3] = {{{0, 0}}, {{0, 0}}, {{0, 0}}};
      for (int t = 0; t < T; ++t)
        for (size_t i = 0; i < units; ++i) {
          const K2 a0 = nt[t][2 * i], a1 = nt[t][2 * i + 1], b0 = nt[T + t][2 * i], b1 = nt[T + t][2 * i + 1];
          want[0] = nv.kadd(want[0], nv.kmul(a0, b0));
          want[1] = nv.kadd(want[1], nv.kmul(a1, b1));
          want[2] = nv.kadd(want[2], nv.kmul(nv.ksub(nv.kadd(a1, a1), a0), nv.ksub(nv.kadd(b1, b1), b0)));
        }
      for (int s = 0; s < 3; ++s) {
        const u64 got[2] = {msg[2 * s], msg[2 * s + 1]};
        ok = ok && same(f, nv, got, want[s]);
      }
      crs[round] = K2{{pick(nv.p, (int)((round + (size_t)sel) % 4)), pick(nv.p, (int)((round / 2 + (size_t)sel + 1) % 4))}};
      out[0] = f.to_mont(crs[round].c[0]);
      out[1] = f.to_mont(crs[round].c[1]);
      for (int q = 0; q < 2 * T; ++q) {
        std::vector<K2> v(units);
        for (size_t i = 0; i < units; ++i) v[i] = nv.kfold(crs[round], nt[q][2 * i], nt[q][2 * i + 1]);
        nt[q] = v;
      }
      return true;
    };
    const MontGeneric hf = [&] {
      FieldParams fp = {};
      field_params_from_modulus(nv.p, &fp);
      return MontGeneric(fp);
    }();
    check(ext_host_rounds(hf, w, (size_t)T, pl.data(), n, 0, base != 0, nullptr, rs.data(), next), "ext_host_rounds ran", (size_t)n);
    check(ok, "ext_host_rounds messages", (size_t)n, (size_t)T);
    for (int q = 0; q < 2 * T; ++q) {
      const u64 got[2] = {planes[2 * q][0], planes[2 * q + 1][0]};
      check(same(f, nv, got, nt[q][0]), "ext_host_rounds finals", (size_t)n, (size_t)q);
    }
    for (int j = 0; j < n; ++j)
      check(rs[2 * j] == f.to_mont(crs[j].c[0]) && rs[2 * j + 1] == f.to_mont(crs[j].c[1]), "ext_host_rounds challenges", (size_t)j);
    // ext_host_evaluate of table 0 at the same point: the same final
    std::vector<u64> e0(len), e1(len, 0);
    for (size_t i = 0; i < len; ++i) {
      e0[i] = mt[0][0][i];
      if (!base) e1[i] = mt[0][1][i];
    }
    ext_host_evaluate(hf, w, e0.data(), e1.data(), n, rs.data(), base != 0);
    check(e0[0] == planes[0][0] && e1[0] == planes[1][0], "ext_host_evaluate", (size_t)n);
  }
}

template <class F>
void all_cases(const F& f, u64 w_canon) {
  element_cases(f, w_canon);
  for (int n = 1; n <= 6; ++n)
    for (int T : {1, 2, 3, 5, kSumprodMaxPairs})
      for (int sel = 0; sel < 4; ++sel) sumprod_cases(f, w_canon, n, T, sel);
}

}  // namespace

int main() {
  FieldParams gp, wp;
  field_params_from_modulus(GoldilocksMont::P, &gp);
  field_params_from_modulus(0xFFFFFFFFFFFFFFC5ull, &wp);   // 2^64 - 59
  const GoldilocksMont g(gp);
  const MontGeneric gm(gp);
  const MontGeneric w(wp);
  all_cases(g, 7);    // 7 is no square mod the Goldilocks prime
  all_cases(gm, 7);
  all_cases(w, 2);    // 2 is none mod 2^64 - 59
  if (failures) {
    printf("%d failures\n", failures);
    return 1;
  }
  printf("ext host harness ok\n");
  return 0;
}
