// Host build of the per-element code of thaler-study_amd/csrc/kernels/ext_grand_product.hpp (the leaf map and its folded form, the
// tree item at LV = 1, 2, 3, the accumulate with its twelve-to-eight map, the eq table and the host rounds that finish a layer),
// compiled for the CPU and run stand-alone against naive schoolbook loops in 128-bit integers on the component words 0, 1, p - 1
// and random ones, both field types.  Every array is allocated at its exact size: this is the build that runs under
// -fsanitize=address,undefined.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../thaler-study_amd/csrc/kernels/ext_grand_product.hpp"
using namespace sc;

namespace {

typedef unsigned __int128 u128;

u64 rnd_state = 0x4578744770;
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
  K2 leaf(K2 alpha, K2 beta, u64 t) const { return kadd(beta, kmul(alpha, K2{{t, 0}})); }
  // u0 + t (u1 - u0), t a small integer
  K2 at(K2 u0, K2 u1, int t) const { return kfold(K2{{(u64)t % p, 0}}, u0, u1); }
};
template <class F>
Naive naive_of(const F& f, u64 w_canon) {
  Naive nv;
  nv.p = f.modulus();
  nv.rinv = f.from_mont(1);   // 1 * R^-1
  nv.w = w_canon;
  return nv;
}
bool same(const Naive& nv, const u64 (&got)[2], K2 want) {
  return got[0] < nv.p && got[1] < nv.p && nv.canon(got[0]) == want.c[0] && nv.canon(got[1]) == want.c[1];
}
bool same2(const Naive& nv, u64 g0, u64 g1, K2 want) {
  const u64 got[2] = {g0, g1};
  return same(nv, got, want);
}

// a canonical word: an edge word (0, 1, p - 1) for sel < 3, else random
u64 pick(u64 p, int sel) { return sel == 0 ? 0 : sel == 1 ? 1 % p : sel == 2 ? p - 1 : rnd() % p; }
// sel < 3: mostly that edge word; otherwise a mix of the edge words and random ones
u64 pick_mixed(u64 p, int sel) { return pick(p, sel < 3 ? (rnd() % 4 == 0 ? 3 : sel) : (int)(rnd() % 6 < 3 ? rnd() % 3 : 3)); }

template <class F>
void to_mont2(const F& f, K2 x, u64 (&o)[2]) {
  o[0] = f.to_mont(x.c[0]);
  o[1] = f.to_mont(x.c[1]);
}

// ext_gp_leaf and ext_gp_fold_leaf on every combination of the component words 0, 1, p - 1 and a random one
template <class F>
void leaf_cases(const F& f, u64 w_canon) {
  const Naive nv = naive_of(f, w_canon);
  const u64 w = f.to_mont(w_canon);
  for (int code = 0; code < 4 * 4 * 4 * 4 * 4 * 4 * 4 * 4; ++code) {
    u64 cw[8];
    for (int k = 0, c = code; k < 8; ++k, c /= 4) cw[k] = pick(nv.p, c % 4);
    const K2 alpha = {{cw[0], cw[1]}}, beta = {{cw[2], cw[3]}}, r = {{cw[4], cw[5]}};
    u64 ma[2], mb[2], mr[2], ra[2], o[2];
    to_mont2(f, alpha, ma);
    to_mont2(f, beta, mb);
    to_mont2(f, r, mr);
    ext_gp_leaf(f, ma, mb, f.to_mont(cw[6]), o);
    check(same(nv, o, nv.leaf(alpha, beta, cw[6])), "ext_gp_leaf", (size_t)code);
    ext_mul(f, w, mr, ma, ra);
    ext_gp_fold_leaf(f, ma, mb, ra, f.to_mont(cw[6]), f.to_mont(cw[7]), o);
    check(same(nv, o, nv.kfold(r, nv.leaf(alpha, beta, cw[6]), nv.leaf(alpha, beta, cw[7]))), "ext_gp_fold_leaf", (size_t)code);
  }
}

template <class F, int LV>
void tree_item_cases(const F& f, u64 w_canon) {
  const Naive nv = naive_of(f, w_canon);
  const u64 w = f.to_mont(w_canon);
  constexpr int W = 1 << LV;
  for (int rep = 0; rep < 64; ++rep) {
    K2 cin[W];
    u64 in[W][2], out[W][2];
    for (int j = 0; j < W; ++j) {
      cin[j] = K2{{pick_mixed(nv.p, rep % 4), pick_mixed(nv.p, (rep / 4) % 4)}};
      to_mont2(f, cin[j], in[j]);
    }
    ext_gp_tree_item<F, LV>(f, w, in, out);
    // the naive heap above the index: level of h entries from the level of 2 h by halves
    std::vector<K2> level(cin, cin + W);
    for (int h = W / 2; h >= 1; h /= 2) {
      std::vector<K2> up((size_t)h);
      for (int j = 0; j < h; ++j) up[(size_t)j] = nv.kmul(level[(size_t)j], level[(size_t)(j + h)]);
      for (int j = 0; j < h; ++j) check(same(nv, out[h + j], up[(size_t)j]), "ext_gp_tree_item", (size_t)LV, (size_t)(h + j));
      level = up;
    }
  }
}

// the accumulate with its map over whole tables, the eq table, and ext_gp_host_rounds: one whole layer of n rounds on the host,
// against the naive sums, folds and finals
template <class F>
void layer_cases(const F& f, u64 w_canon, int n, int sel) {
  const Naive nv = naive_of(f, w_canon);
  const u64 w = f.to_mont(w_canon);
  const size_t len = (size_t)1 << n;
  const MontGeneric hf = [&] {
    FieldParams fp = {};
    field_params_from_modulus(nv.p, &fp);
    return MontGeneric(fp);
  }();
  // the point of the eq table and the naive eq by its definition
  std::vector<K2> cz((size_t)n);
  std::vector<u64> mz((size_t)2 * n);
  for (int j = 0; j < n; ++j) {
    cz[(size_t)j] = K2{{pick(nv.p, (j + sel) % 4), pick(nv.p, (j / 2 + sel + 1) % 4)}};
    mz[(size_t)2 * j] = f.to_mont(cz[(size_t)j].c[0]);
    mz[(size_t)2 * j + 1] = f.to_mont(cz[(size_t)j].c[1]);
  }
  std::vector<std::vector<K2>> nt(3, std::vector<K2>(len));
  for (size_t i = 0; i < len; ++i) {
    K2 e = {{1 % nv.p, 0}};
    for (int j = 0; j < n; ++j) e = nv.kmul(e, ((i >> j) & 1) ? cz[(size_t)j] : nv.ksub(K2{{1 % nv.p, 0}}, cz[(size_t)j]));
    nt[0][i] = e;
    for (int q = 1; q < 3; ++q) nt[(size_t)q][i] = K2{{pick_mixed(nv.p, sel), pick_mixed(nv.p, (sel + q) % 4)}};
  }
  std::vector<std::vector<u64>> planes(6, std::vector<u64>(len));
  std::vector<u64*> pl(6);
  for (int q = 0; q < 6; ++q) pl[(size_t)q] = planes[(size_t)q].data();
  ext_gp_host_eq(f, w, mz.data(), n, pl[0], pl[1]);
  for (size_t i = 0; i < len; ++i) {
    check(same2(nv, planes[0][i], planes[1][i], nt[0][i]), "ext_gp_host_eq", (size_t)n, i);
    for (int q = 1; q < 3; ++q)
      for (int c = 0; c < 2; ++c) planes[(size_t)(2 * q + c)][i] = f.to_mont(nt[(size_t)q][i].c[c]);
  }
  // one item at a time: ext_gp_accumulate and the map over the whole tables
  {
    typename F::Acc acc[2][6];
    for (int h = 0; h < 2; ++h)
      for (int s = 0; s < 6; ++s) f.acc_zero(acc[h][s]);
    K2 want[4] = {{{0, 0}}, {{0, 0}}, {{0, 0}}, {{0, 0}}};
    for (size_t i = 0; i < len / 2; ++i) {
      u64 p3[3][2][2];
      for (int q = 0; q < 3; ++q)
        for (int h = 0; h < 2; ++h)
          for (int c = 0; c < 2; ++c) p3[q][h][c] = planes[(size_t)(2 * q + c)][2 * i + (size_t)h];
      ext_gp_accumulate(f, w, acc, p3[0], p3[1], p3[2]);
      for (int t = 0; t < 4; ++t)
        want[t] = nv.kadd(want[t], nv.kmul(nv.at(nt[0][2 * i], nt[0][2 * i + 1], t),
                                           nv.kmul(nv.at(nt[1][2 * i], nt[1][2 * i + 1], t), nv.at(nt[2][2 * i], nt[2][2 * i + 1], t))));
    }
    u64 cells[12];
    for (int h = 0; h < 2; ++h)
      for (int s = 0; s < 6; ++s) cells[6 * h + s] = f.acc_get(acc[h][s]);
    for (int t = 0; t < 4; ++t)
      check(same2(nv, ext_gp_cells_to_word(f, w, cells, 2 * t), ext_gp_cells_to_word(f, w, cells, 2 * t + 1), want[t]),
            "ext_gp_accumulate and the twelve-to-eight map", (size_t)n, (size_t)t);
  }
  // the whole layer
  std::vector<u64> rs((size_t)2 * n);
  std::vector<K2> crs((size_t)n);
  bool ok = true;
  auto next = [&](size_t round, const u64* msg, u64* out) {
    const size_t units = nt[0].size() / 2;
    for (int t = 0; t < 4; ++t) {
      K2 want = {{0, 0}};
      for (size_t i = 0; i < units; ++i)
        want = nv.kadd(want, nv.kmul(nv.at(nt[0][2 * i], nt[0][2 * i + 1], t),
                                     nv.kmul(nv.at(nt[1][2 * i], nt[1][2 * i + 1], t), nv.at(nt[2][2 * i], nt[2][2 * i + 1], t))));
      ok = ok && same2(nv, msg[2 * t], msg[2 * t + 1], want);
    }
    crs[round] = K2{{pick(nv.p, (int)((round + (size_t)sel) % 4)), pick(nv.p, (int)((round / 2 + (size_t)sel + 1) % 4))}};
    out[0] = f.to_mont(crs[round].c[0]);
    out[1] = f.to_mont(crs[round].c[1]);
    for (int q = 0; q < 3; ++q) {
      std::vector<K2> v(units);
      for (size_t i = 0; i < units; ++i) v[i] = nv.kfold(crs[round], nt[(size_t)q][2 * i], nt[(size_t)q][2 * i + 1]);
      nt[(size_t)q] = v;
    }
    return true;
  };
  check(ext_gp_host_rounds(hf, w, pl.data(), n, 0, nullptr, rs.data(), next), "ext_gp_host_rounds ran", (size_t)n);
  check(ok, "ext_gp_host_rounds messages", (size_t)n, (size_t)sel);
  for (int q = 1; q < 3; ++q) check(same2(nv, planes[(size_t)(2 * q)][0], planes[(size_t)(2 * q + 1)][0], nt[(size_t)q][0]), "ext_gp_host_rounds finals", (size_t)n, (size_t)q);
  for (int j = 0; j < n; ++j)
    check(rs[(size_t)2 * j] == f.to_mont(crs[(size_t)j].c[0]) && rs[(size_t)2 * j + 1] == f.to_mont(crs[(size_t)j].c[1]), "ext_gp_host_rounds challenges", (size_t)j);
}

template <class F>
void all_cases(const F& f, u64 w_canon) {
  leaf_cases(f, w_canon);
  tree_item_cases<F, 1>(f, w_canon);
  tree_item_cases<F, 2>(f, w_canon);
  tree_item_cases<F, 3>(f, w_canon);
  for (int n = 1; n <= 6; ++n)
    for (int sel = 0; sel < 4; ++sel) layer_cases(f, w_canon, n, sel);
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
  printf("ext gp host harness ok\n");
  return 0;
}
