// Host build of the per-element code of thaler-study_amd/csrc/kernels/multiopen.hpp (the low table entry, the high factor and the
// per-entry multiply-add sum of eq_sum_kernel, laid out as the kernel lays them out in LDS; the item of sumprod_pass_kernel - fold
// and accumulate - and the host rounds that finish a proof), compiled for the CPU and run stand-alone against naive loops in
// 128-bit integers on the edge words 0, 1 and p - 1, both fields.  Every array is allocated at its exact size: this is the build
// that runs under -fsanitize=address,undefined.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../thaler-study_amd/csrc/kernels/multiopen.hpp"
using namespace sc;

namespace {

typedef unsigned __int128 u128;

u64 rnd_state = 0x6D4F70;
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
  u64 addc(u64 a, u64 b) const { return (u64)(((u128)a + b) % p); }
  u64 subc(u64 a, u64 b) const { return (u64)(((u128)a + p - b) % p); }
  u64 canon(u64 w) const { return mulc(w, rinv); }
  // eq(point, x) over n bits
  u64 eq(const u64* point, int n, size_t x) const {
    u64 v = 1 % p;
    for (int j = 0; j < n; ++j) v = mulc(v, ((x >> j) & 1) ? point[j] : subc(1 % p, point[j]));
    return v;
  }
};
template <class F>
Naive naive_of(const F& f) {
  Naive nv;
  nv.p = f.modulus();
  nv.rinv = f.from_mont(1);   // 1 * R^-1
  return nv;
}

// a canonical word: an edge word (0, 1, p - 1) for sel < 3, else random
u64 pick(u64 p, int sel) { return sel == 0 ? 0 : sel == 1 ? 1 % p : sel == 2 ? p - 1 : rnd() % p; }

// eq_sum_kernel's arithmetic for `count` points of n variables, with the kernel's layout of the low tables and the factors
template <class F>
void eq_sum_cases(const F& f, int n, int count, int sel) {
  const Naive nv = naive_of(f);
  const int lo = n < kEqSumLoLog ? n : kEqSumLoLog;
  std::vector<u64> pc((size_t)count * n + count), canon_pc(pc.size());
  for (size_t i = 0; i < pc.size(); ++i) {
    canon_pc[i] = pick(nv.p, sel < 4 ? (int)(rnd() % 3 == 0 ? 3 : sel) : (int)(rnd() % 4));
    pc[i] = f.to_mont(canon_pc[i]);
  }
  const u64* coeffs = pc.data() + (size_t)count * n;
  std::vector<u64> low((size_t)count << lo);
  for (int k = 0; k < count; ++k)
    for (unsigned x = 0; x < (1u << lo); ++x) {
      low[((size_t)k << lo) + x] = eq_sum_low(f, pc.data() + (size_t)k * n, lo, x);
      check(nv.canon(low[((size_t)k << lo) + x]) == nv.eq(canon_pc.data() + (size_t)k * n, lo, x), "eq_sum_low", (size_t)n, x);
    }
  const size_t n_high = (size_t)1 << (n - lo);
  std::vector<u64> fac((size_t)count * n_high);
  for (int k = 0; k < count; ++k)
    for (size_t h = 0; h < n_high; ++h) fac[(size_t)k * n_high + h] = eq_sum_high(f, pc.data() + (size_t)k * n, lo, n, h, coeffs[k]);
  for (size_t x = 0; x < ((size_t)1 << n); ++x) {
    const size_t h = x >> lo, xl = x & (((size_t)1 << lo) - 1);
    const u64 got = eq_sum_entry(f, count, fac.data() + h, n_high, low.data() + xl, (size_t)1 << lo);
    u64 want = 0;
    for (int k = 0; k < count; ++k)
      want = nv.addc(want, nv.mulc(canon_pc[(size_t)count * n + k], nv.eq(canon_pc.data() + (size_t)k * n, n, x)));
    check(got < nv.p && nv.canon(got) == want, "eq_sum_entry", (size_t)n, x);
  }
}

// the item of the pass: zc_fold4 of four entries per table, sp_accumulate of the folded pairs, over T pairs - and sp_host_rounds, a
// whole proof on the host, against the naive sums, folds and finals
template <class F>
void sumprod_cases(const F& f, int n, int T, int sel) {
  const Naive nv = naive_of(f);
  const size_t len = (size_t)1 << n;
  std::vector<std::vector<u64>> a(T, std::vector<u64>(len)), b(T, std::vector<u64>(len)), ca(T, std::vector<u64>(len)), cb(T, std::vector<u64>(len));
  for (int t = 0; t < T; ++t)
    for (size_t i = 0; i < len; ++i) {
      ca[t][i] = pick(nv.p, sel < 3 ? sel : (int)(rnd() % 6 < 3 ? rnd() % 3 : 3));
      cb[t][i] = pick(nv.p, sel < 3 ? sel : (int)(rnd() % 6 < 3 ? rnd() % 3 : 3));
      a[t][i] = f.to_mont(ca[t][i]);
      b[t][i] = f.to_mont(cb[t][i]);
    }
  // one FOLD launch's items: fold by r, then the sums of the folded tables
  if (n >= 2) {
    const u64 cr = pick(nv.p, sel), r = f.to_mont(cr);
    typename F::Acc acc[3];
    for (int s = 0; s < 3; ++s) f.acc_zero(acc[s]);
    u64 want[3] = {0, 0, 0};
    for (size_t i = 0; i < len / 4; ++i)
      for (int t = 0; t < T; ++t) {
        u64 p2[2][2], c2[2][2];
        for (int k = 0; k < 2; ++k) {
          const std::vector<u64>& src = k ? b[t] : a[t];
          const std::vector<u64>& csrc = k ? cb[t] : ca[t];
          const u64 u[4] = {src[4 * i], src[4 * i + 1], src[4 * i + 2], src[4 * i + 3]};
          zc_fold4(f, r, u, p2[k]);
          for (int h = 0; h < 2; ++h) {
            c2[k][h] = nv.addc(csrc[4 * i + 2 * h], nv.mulc(cr, nv.subc(csrc[4 * i + 2 * h + 1], csrc[4 * i + 2 * h])));
            check(p2[k][h] < nv.p && nv.canon(p2[k][h]) == c2[k][h], "zc_fold4", i, (size_t)t);
          }
        }
        sp_accumulate(f, acc, p2[0], p2[1]);
        want[0] = nv.addc(want[0], nv.mulc(c2[0][0], c2[1][0]));
        want[1] = nv.addc(want[1], nv.mulc(c2[0][1], c2[1][1]));
        const u64 a2 = nv.subc(nv.addc(c2[0][1], c2[0][1]), c2[0][0]), b2 = nv.subc(nv.addc(c2[1][1], c2[1][1]), c2[1][0]);
        want[2] = nv.addc(want[2], nv.mulc(a2, b2));
      }
    // (a sum of Montgomery products carries one factor R: acc_get takes it out)
    for (int s = 0; s < 3; ++s) check(nv.canon(f.acc_get(acc[s])) == want[s], "sp_accumulate", (size_t)n, (size_t)s);
  }
  // the host rounds over the whole tables
  std::vector<u64*> pa(T), pb(T);
  std::vector<std::vector<u64>> wa = a, wb = b;
  for (int t = 0; t < T; ++t) {
    pa[t] = wa[t].data();
    pb[t] = wb[t].data();
  }
  std::vector<u64> rs(n), crs(n);
  std::vector<std::vector<u64>> na = ca, nb = cb;
  bool ok = true;
  auto next = [&](size_t round, const u64* msg, u64* out) {
    // the naive message of this round from the naive tables
    const size_t units = na[0].size() / 2;
    u64 want[3] = {0, 0, 0};
    for (int t = 0; t < T; ++t)
      for (size_t i = 0; i < units; ++i) {
        const u64 a0 = na[t][2 * i], a1 = na[t][2 * i + 1], b0 = nb[t][2 * i], b1 = nb[t][2 * i + 1];
        want[0] = nv.addc(want[0], nv.mulc(a0, b0));
        want[1] = nv.addc(want[1], nv.mulc(a1, b1));
        want[2] = nv.addc(want[2], nv.mulc(nv.subc(nv.addc(a1, a1), a0), nv.subc(nv.addc(b1, b1), b0)));
      }
    for (int s = 0; s < 3; ++s) ok = ok && msg[s] < nv.p && nv.canon(msg[s]) == want[s];
    crs[round] = pick(nv.p, (int)((round + (size_t)sel) % 4));
    *out = f.to_mont(crs[round]);
    for (int t = 0; t < T; ++t)
      for (int k = 0; k < 2; ++k) {
        std::vector<u64>& u = k ? nb[t] : na[t];
        std::vector<u64> v(units);
        for (size_t i = 0; i < units; ++i) v[i] = nv.addc(u[2 * i], nv.mulc(crs[round], nv.subc(u[2 * i + 1], u[2 * i])));
        u = v;
      }
    return true;
  };
  const MontGeneric hf = [&] {
    FieldParams fp = {};
    field_params_from_modulus(nv.p, &fp);
    return MontGeneric(fp);
  }();
  check(sp_host_rounds(hf, (size_t)T, pa.data(), pb.data(), n, 0, nullptr, rs.data(), next), "sp_host_rounds ran", (size_t)n);
  check(ok, "sp_host_rounds messages", (size_t)n, (size_t)T);
  for (int t = 0; t < T; ++t)
    check(nv.canon(wa[t][0]) == na[t][0] && nv.canon(wb[t][0]) == nb[t][0], "sp_host_rounds finals", (size_t)n, (size_t)t);
  for (int j = 0; j < n; ++j) check(rs[j] == f.to_mont(crs[j]), "sp_host_rounds challenges", (size_t)j);
}

template <class F>
void all_cases(const F& f) {
  for (int n = 1; n <= kEqSumLoLog + 2; ++n)
    for (int count : {1, 2, 3, kEqSumMaxCount})
      for (int sel = 0; sel < 5; ++sel) {
        if (n > kEqSumLoLog && sel < 3 && count == 3) continue;   // (the edge selections once per width above the split)
        eq_sum_cases(f, n, count, sel);
      }
  for (int n = 1; n <= 6; ++n)
    for (int T : {1, 2, 3, 5, kSumprodMaxPairs})
      for (int sel = 0; sel < 4; ++sel) sumprod_cases(f, n, T, sel);
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
  printf("multiopen host harness ok\n");
  return 0;
}
