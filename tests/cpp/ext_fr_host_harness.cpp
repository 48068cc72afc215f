// Host build of the per-element code of thaler-study_amd/csrc/kernels/ext_fraction.hpp (the tree item at LV = 1, 2, 3 in its three
// forms, the two accumulate forms with their twelve-to-eight map, the leaf-in folds and the host rounds that finish a layer),
// compiled for the CPU and run stand-alone against naive schoolbook loops in 128-bit integers on the component words 0, 1, p - 1
// and random ones, both field types.  Every array is allocated at its exact size: this is the build that runs under
// -fsanitize=address,undefined.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../thaler-study_amd/csrc/kernels/ext_fraction.hpp"
using namespace sc;

namespace {

typedef unsigned __int128 u128;

u64 rnd_state = 0x457874467261;
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
  K2 one() const { return K2{{1 % p, 0}}; }
  K2 kadd(K2 a, K2 b) const { return K2{{addc(a.c[0], b.c[0]), addc(a.c[1], b.c[1])}}; }
  K2 ksub(K2 a, K2 b) const { return K2{{subc(a.c[0], b.c[0]), subc(a.c[1], b.c[1])}}; }
  K2 kmul(K2 a, K2 b) const {
    return K2{{addc(mulc(a.c[0], b.c[0]), mulc(w, mulc(a.c[1], b.c[1]))), addc(mulc(a.c[0], b.c[1]), mulc(a.c[1], b.c[0]))}};
  }
  K2 kfold(K2 r, K2 u0, K2 u1) const { return kadd(u0, kmul(r, ksub(u1, u0))); }
  K2 leaf(K2 alpha, K2 beta, u64 t) const { return kadd(beta, kmul(alpha, K2{{t, 0}})); }
  // u0 + t (u1 - u0), t a small integer
  K2 at(K2 u0, K2 u1, int t) const { return kfold(K2{{(u64)t % p, 0}}, u0, u1); }
  // e (pl qr + pr ql + lambda ql qr)
  K2 term(K2 e, K2 pl, K2 pr, K2 ql, K2 qr, K2 lambda) const {
    return kmul(e, kadd(kadd(kmul(pl, qr), kmul(pr, ql)), kmul(lambda, kmul(ql, qr))));
  }
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

// The leaf-in folds of the pass: QL, QR by ext_gp_fold_leaf (r alpha formed once), PL, PR by ext_fold_base, against the fold in K
// of the leaves themselves, on every combination of the component words 0, 1, p - 1 and a random one
template <class F>
void leaf_fold_cases(const F& f, u64 w_canon) {
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
    ext_mul(f, w, mr, ma, ra);
    ext_gp_fold_leaf(f, ma, mb, ra, f.to_mont(cw[6]), f.to_mont(cw[7]), o);
    check(same(nv, o, nv.kfold(r, nv.leaf(alpha, beta, cw[6]), nv.leaf(alpha, beta, cw[7]))), "the leaf-in fold of a denominator", (size_t)code);
    ext_fold_base(f, mr, f.to_mont(cw[6]), f.to_mont(cw[7]), o);
    check(same(nv, o, nv.kfold(r, K2{{cw[6], 0}}, K2{{cw[7], 0}})), "the leaf-in fold of a numerator", (size_t)code);
  }
}

// ext_fr_tree_item in one form: planes in; LEAF_IN, the numerators base words; LEAF_IN and ONES
template <class F, int LV, bool LEAF_IN, bool ONES>
void tree_item_cases(const F& f, u64 w_canon) {
  const Naive nv = naive_of(f, w_canon);
  const u64 w = f.to_mont(w_canon);
  constexpr int W = 1 << LV;
  for (int rep = 0; rep < 64; ++rep) {
    K2 cp[W], cq[W];
    u64 pin[W][2], qin[W][2], pout[W][2], qout[W][2];
    for (int j = 0; j < W; ++j) {
      cq[j] = K2{{pick_mixed(nv.p, rep % 4), pick_mixed(nv.p, (rep / 4) % 4)}};
      cp[j] = ONES ? nv.one() : K2{{pick_mixed(nv.p, (rep / 16) % 4), LEAF_IN ? 0 : pick_mixed(nv.p, (rep / 2) % 4)}};
      to_mont2(f, cq[j], qin[j]);
      to_mont2(f, cp[j], pin[j]);
      if (LEAF_IN) pin[j][1] = 0xDEADBEEFDEADBEEFull;   // (not read)
      if (ONES) pin[j][0] = 0xDEADBEEFDEADBEEFull;      // (not read)
    }
    ext_fr_tree_item<F, LV, LEAF_IN, ONES>(f, w, pin, qin, pout, qout);
    // the naive heaps above the index: level of h entries from the level of 2 h by halves
    std::vector<K2> lp(cp, cp + W), lq(cq, cq + W);
    for (int h = W / 2; h >= 1; h /= 2) {
      std::vector<K2> up((size_t)h), uq((size_t)h);
      for (int j = 0; j < h; ++j) {
        up[(size_t)j] = nv.kadd(nv.kmul(lp[(size_t)j], lq[(size_t)(j + h)]), nv.kmul(lp[(size_t)(j + h)], lq[(size_t)j]));
        uq[(size_t)j] = nv.kmul(lq[(size_t)j], lq[(size_t)(j + h)]);
      }
      for (int j = 0; j < h; ++j) {
        check(same(nv, pout[h + j], up[(size_t)j]), "ext_fr_tree_item numerator", (size_t)(LV * 4 + LEAF_IN * 2 + ONES), (size_t)(h + j));
        check(same(nv, qout[h + j], uq[(size_t)j]), "ext_fr_tree_item denominator", (size_t)(LV * 4 + LEAF_IN * 2 + ONES), (size_t)(h + j));
      }
      lp = up;
      lq = uq;
    }
  }
}

// the accumulate forms with their map over whole tables, and ext_fr_host_rounds: one whole layer of n rounds on the host, against
// the naive sums, folds and finals.  ones: three tables, pl = pr = 1
template <class F>
void layer_cases(const F& f, u64 w_canon, int n, int sel, bool ones) {
  const Naive nv = naive_of(f, w_canon);
  const u64 w = f.to_mont(w_canon);
  const size_t len = (size_t)1 << n;
  const int ntab = ones ? 3 : 5;
  const MontGeneric hf = [&] {
    FieldParams fp = {};
    field_params_from_modulus(nv.p, &fp);
    return MontGeneric(fp);
  }();
  const K2 clam = {{pick(nv.p, (sel + 2) % 4), pick(nv.p, (sel + n) % 4)}};
  u64 lam[2];
  to_mont2(f, clam, lam);
  // nt: the naive tables in the order kFrE .. kFrPR, always five (ones: PL = PR = 1)
  std::vector<std::vector<K2>> nt(5, std::vector<K2>(len));
  for (size_t i = 0; i < len; ++i)
    for (int q = 0; q < 5; ++q)
      nt[(size_t)q][i] = ones && q >= kFrPL ? nv.one() : K2{{pick_mixed(nv.p, (sel + q) % 4), pick_mixed(nv.p, (sel + 2 * q + 1) % 4)}};
  std::vector<std::vector<u64>> planes((size_t)2 * ntab, std::vector<u64>(len));
  std::vector<u64*> pl((size_t)2 * ntab);
  for (int q = 0; q < 2 * ntab; ++q) pl[(size_t)q] = planes[(size_t)q].data();
  for (size_t i = 0; i < len; ++i)
    for (int q = 0; q < ntab; ++q)
      for (int c = 0; c < 2; ++c) planes[(size_t)(2 * q + c)][i] = f.to_mont(nt[(size_t)q][i].c[c]);
  auto naive_sum = [&](int t) {
    K2 want = {{0, 0}};
    for (size_t i = 0; i < nt[0].size() / 2; ++i) {
      K2 v[5];
      for (int q = 0; q < 5; ++q) v[q] = nv.at(nt[(size_t)q][2 * i], nt[(size_t)q][2 * i + 1], t);
      want = nv.kadd(want, nv.term(v[kFrE], v[kFrPL], v[kFrPR], v[kFrQL], v[kFrQR], clam));
    }
    return want;
  };
  // one item at a time: the accumulate and the map over the whole tables
  {
    typename F::Acc acc[2][6];
    for (int h = 0; h < 2; ++h)
      for (int s = 0; s < 6; ++s) f.acc_zero(acc[h][s]);
    for (size_t i = 0; i < len / 2; ++i) {
      u64 u[5][2][2];
      for (int q = 0; q < ntab; ++q)
        for (int h = 0; h < 2; ++h)
          for (int c = 0; c < 2; ++c) u[q][h][c] = planes[(size_t)(2 * q + c)][2 * i + (size_t)h];
      if (ones) ext_fr_accumulate_ones(f, w, acc, lam, u[kFrE], u[kFrQL], u[kFrQR]);
      else ext_fr_accumulate(f, w, acc, lam, u[kFrE], u[kFrPL], u[kFrPR], u[kFrQL], u[kFrQR]);
    }
    u64 cells[12];
    for (int h = 0; h < 2; ++h)
      for (int s = 0; s < 6; ++s) cells[6 * h + s] = f.acc_get(acc[h][s]);
    for (int t = 0; t < 4; ++t)
      check(same2(nv, ext_gp_cells_to_word(f, w, cells, 2 * t), ext_gp_cells_to_word(f, w, cells, 2 * t + 1), naive_sum(t)),
            ones ? "ext_fr_accumulate_ones and the twelve-to-eight map" : "ext_fr_accumulate and the twelve-to-eight map", (size_t)n, (size_t)t);
  }
  // the whole layer
  std::vector<u64> rs((size_t)2 * n);
  std::vector<K2> crs((size_t)n);
  bool ok = true;
  auto next = [&](size_t round, const u64* msg, u64* out) {
    const size_t units = nt[0].size() / 2;
    for (int t = 0; t < 4; ++t) ok = ok && same2(nv, msg[2 * t], msg[2 * t + 1], naive_sum(t));
    crs[round] = K2{{pick(nv.p, (int)((round + (size_t)sel) % 4)), pick(nv.p, (int)((round / 2 + (size_t)sel + 1) % 4))}};
    out[0] = f.to_mont(crs[round].c[0]);
    out[1] = f.to_mont(crs[round].c[1]);
    for (int q = 0; q < 5; ++q) {
      std::vector<K2> v(units);
      for (size_t i = 0; i < units; ++i) v[i] = nv.kfold(crs[round], nt[(size_t)q][2 * i], nt[(size_t)q][2 * i + 1]);
      nt[(size_t)q] = v;
    }
    return true;
  };
  u64 hlam[2] = {lam[0], lam[1]};
  check(ext_fr_host_rounds(hf, w, pl.data(), ntab, hlam, n, 0, nullptr, rs.data(), next), "ext_fr_host_rounds ran", (size_t)n);
  check(ok, "ext_fr_host_rounds messages", (size_t)n, (size_t)sel);
  for (int q = 1; q < ntab; ++q)
    check(same2(nv, planes[(size_t)(2 * q)][0], planes[(size_t)(2 * q + 1)][0], nt[(size_t)q][0]), "ext_fr_host_rounds finals", (size_t)n, (size_t)q);
  for (int j = 0; j < n; ++j)
    check(rs[(size_t)2 * j] == f.to_mont(crs[(size_t)j].c[0]) && rs[(size_t)2 * j + 1] == f.to_mont(crs[(size_t)j].c[1]), "ext_fr_host_rounds challenges", (size_t)j);
}

template <class F, int LV>
void tree_item_forms(const F& f, u64 w_canon) {
  tree_item_cases<F, LV, false, false>(f, w_canon);
  tree_item_cases<F, LV, true, false>(f, w_canon);
  tree_item_cases<F, LV, true, true>(f, w_canon);
}

template <class F>
void all_cases(const F& f, u64 w_canon) {
  leaf_fold_cases(f, w_canon);
  tree_item_forms<F, 1>(f, w_canon);
  tree_item_forms<F, 2>(f, w_canon);
  tree_item_forms<F, 3>(f, w_canon);
  for (int n = 1; n <= 6; ++n)
    for (int sel = 0; sel < 4; ++sel)
      for (int ones = 0; ones < 2; ++ones) layer_cases(f, w_canon, n, sel, ones != 0);
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
  printf("ext fr host harness ok\n");
  return 0;
}
