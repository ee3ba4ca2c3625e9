// Stand-alone check of the host part of the set tests (miraculix_amd/csrc/mxa_assoc_set_host.h: assoc_set_args, set_plan, skat_pvalue_host), for a CPU build
// under sanitizers:
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -static-libasan -static-libubsan tools/assoc_set_host_check.cpp \
//       -o assoc_set_host_check && ./assoc_set_host_check
// (the runtimes linked statically: the program is self-contained and runs in whatever environment it is started in)
// Every error path of mxa_assoc_set's argument rules is driven once and must name its cause.  The rules dereference set_ptr and set_idx and nothing else:
// every other operand is a heap block of ONE byte (a read of it would be reported), and the CSR arrays are heap blocks of exactly their length (a read one
// entry too far would be reported).  The batch plan must cover every set once, in order, and never split one; the p-value is checked at its edges and
// against closed forms (l = 2: exp(-x / 2); l = 1: erfc(sqrt(x / 2))).
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <memory>
#include <vector>
#include "../miraculix_amd/csrc/mxa_assoc_set_host.h"

namespace {

struct Args {
  const void *plink, *R, *Wt, *H, *score, *var, *zstat, *stat;
  std::vector<long> ptr{0, 2, 2, 5};
  std::vector<int> idx{4, 0, 1, 1, 3};
  bool null_ptr = false, null_idx = false;
  long snps = 5, indiv = 12, ldr = 12, ldw = 12, ldh = 12, ldo = 5, lds = 3;
  int n = 2, kh = 3, nsets = 3;
  char msg[192];
  int check() {
    // exact-length heap copies: the sanitizer sees every read beyond the arrays
    std::unique_ptr<long[]> p(new long[ptr.size()]);
    std::unique_ptr<int[]> i(new int[idx.size() ? idx.size() : 1]);
    std::memcpy(p.get(), ptr.data(), sizeof(long) * ptr.size());
    if (!idx.empty()) std::memcpy(i.get(), idx.data(), sizeof(int) * idx.size());
    msg[0] = 0;
    return mxa::assoc_set_args(plink, snps, indiv, R, ldr, Wt, ldw, H, ldh, n, kh, nsets, null_ptr ? nullptr : p.get(), null_idx ? nullptr : i.get(), score, var, zstat,
                               ldo, stat, lds, msg, sizeof(msg));
  }
};

int failures = 0;

void accepted(const char *what, Args a) {
  if (a.check()) { std::printf("FAIL: %s was refused: %s\n", what, a.msg); failures++; }
}
void refused(const char *what, Args a, const char *word) {
  if (!a.check()) { std::printf("FAIL: %s was accepted\n", what); failures++; }
  else if (!std::strstr(a.msg, word)) { std::printf("FAIL: %s: the message \"%s\" does not name \"%s\"\n", what, a.msg, word); failures++; }
}
void expect(bool ok, const char *what) {
  if (!ok) { std::printf("FAIL: %s\n", what); failures++; }
}

void check_plan(const std::vector<long> &sizes, int n, long indiv, long max_entries, size_t budget, size_t want_batches) {
  std::vector<long> ptr(sizes.size() + 1, 0);
  for (size_t k = 0; k < sizes.size(); k++) ptr[k + 1] = ptr[k] + sizes[k];
  const std::vector<mxa::SetBatch> plan = mxa::set_plan((int)sizes.size(), ptr.data(), n, indiv, max_entries, budget);
  int at = 0;
  long entries = 0;
  for (const mxa::SetBatch &b : plan) {
    expect(b.k0 == at && b.k1 > b.k0, "a batch begins where the one before it ended and holds a whole set");
    expect(b.entries == ptr[b.k1] - ptr[b.k0], "the entries of a batch");
    expect(b.k1 - b.k0 == 1 || (b.entries <= max_entries && mxa::set_batch_bytes(b, mxa::set_pieces(indiv)) <= budget), "a batch of several sets keeps both limits");
    expect(b.items == (long)n * (b.k1 - b.k0), "the items of a batch");
    at = b.k1;
    entries += b.entries;
  }
  expect(at == (int)sizes.size() && entries == ptr.back(), "the batches cover every set once");
  if (want_batches) expect(plan.size() == want_batches, "the number of batches");
}

}  // namespace

int main() {
  std::unique_ptr<char[]> blocks[8];
  for (auto &b : blocks) b.reset(new char[1]);
  Args ok;
  ok.plink = blocks[0].get(); ok.R = blocks[1].get(); ok.Wt = blocks[2].get(); ok.H = blocks[3].get();
  ok.score = blocks[4].get(); ok.var = blocks[5].get(); ok.zstat = blocks[6].get(); ok.stat = blocks[7].get();
  const long big = mxa::kAssocMaxIndiv;
  Args a;

  accepted("the plain call", ok);
  a = ok; a.score = a.var = a.zstat = nullptr; accepted("score, var and zstat all NULL", a);
  a = ok; a.H = nullptr; a.kh = 0; a.ldh = 0; accepted("kh = 0 with a NULL H", a);
  a = ok; a.ptr = {0, 0, 0, 0}; a.idx = {}; accepted("empty sets only", a);
  a = ok; a.nsets = 1; a.lds = 1; a.ptr = {0, 1024}; a.idx.assign(1024, 4); accepted("one set of 1024 entries, one SNP repeated", a);
  a = ok; a.indiv = a.ldr = a.ldw = a.ldh = big; accepted("the largest indiv", a);
  a = ok; a.lds = 100; accepted("lds beyond nsets", a);

  // the errors of mxa_assoc_score
  a = ok; a.plink = nullptr; refused("a NULL plink", a, "plink");
  a = ok; a.R = nullptr; refused("a NULL R", a, "R and Wt");
  a = ok; a.Wt = nullptr; refused("a NULL Wt", a, "R and Wt");
  a = ok; a.snps = 0; refused("snps = 0", a, "positive");
  a = ok; a.indiv = 0; refused("indiv = 0", a, "positive");
  a = ok; a.n = 0; refused("n = 0", a, "positive");
  a = ok; a.kh = -1; refused("kh = -1", a, "kh");
  a = ok; a.H = nullptr; refused("a NULL H with kh > 0", a, "H is NULL");
  a = ok; a.n = 65535 / 5 + 1; refused("n (kh + 2) = 65540", a, "65535");
  a = ok; a.ldr = 11; refused("ldr below indiv", a, "ldr");
  a = ok; a.ldw = 11; refused("ldw below indiv", a, "ldw");
  a = ok; a.ldh = 11; refused("ldh below indiv", a, "ldh");
  a = ok; a.indiv = a.ldr = a.ldw = a.ldh = big + 1; refused("indiv beyond the limit", a, "47 453 132");
  a = ok; a.ldo = 4; refused("ldo below snps", a, "ldo");
  // its own
  a = ok; a.nsets = 0; refused("nsets = 0", a, "nsets");
  a = ok; a.nsets = -5; refused("nsets = -5", a, "nsets");
  a = ok; a.null_ptr = true; refused("a NULL set_ptr", a, "set_ptr");
  a = ok; a.null_idx = true; refused("a NULL set_idx", a, "set_idx");
  a = ok; a.stat = nullptr; refused("a NULL stat", a, "stat");
  a = ok; a.lds = 2; refused("lds below nsets", a, "lds");
  a = ok; a.ptr = {1, 2, 2, 5}; refused("set_ptr[0] = 1", a, "set_ptr[0]");
  a = ok; a.ptr = {0, 3, 2, 5}; refused("a decreasing set_ptr", a, "decreases at set 1");
  a = ok; a.idx = {4, 0, 1, 1, 5}; refused("an index of snps", a, "entry 2 of set 2");
  a = ok; a.idx = {4, -1, 1, 1, 3}; refused("a negative index", a, "entry 1 of set 0");
  a = ok; a.ptr = {0, 0, 1025, 1025}; a.idx.assign(1025, 0); refused("a set of 1025 entries", a, "set 1 has 1025");
  // the order: the scan's rules first; the sizes before the indices (no index is read of a list whose set_ptr is wrong)
  a = ok; a.nsets = 0; a.snps = 0; refused("snps = 0 with nsets = 0", a, "positive");
  a = ok; a.ptr = {0, 2, 1, 5}; a.idx = {9, 9}; refused("a decreasing set_ptr before a wrong index", a, "decreases");

  // the batches
  check_plan({0, 1, 2, 15, 16, 17, 33}, 1, 4099, std::numeric_limits<long>::max(), mxa::kSetBudget, 1);
  check_plan({0, 1, 2, 15, 16, 17, 33}, 3, 4099, 1, mxa::kSetBudget, 6);          // the empty set joins the one behind it
  check_plan({0, 1, 2, 15, 16, 17, 33}, 2, 257, 18, mxa::kSetBudget, 4);
  check_plan({1024, 1024, 3}, 2, 1000000, std::numeric_limits<long>::max(), mxa::kSetBudget, 3);   // one set beyond the budget is a batch of its own
  check_plan(std::vector<long>(1563, 32), 1, 1000000, std::numeric_limits<long>::max(), mxa::kSetBudget, 0);
  check_plan({5}, 1, 1, 1, 1, 1);

  // the p-value
  const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
  double df = -1.0;
  expect(mxa::skat_pvalue_host(1.0, 3.0, 2.0, 2.0, &df) == 1.0 && df == 2.0, "x = 0 gives exactly 1 and df = l");
  expect(mxa::skat_pvalue_host(-5.0, 3.0, 2.0, 2.0, nullptr) == 1.0, "x < 0 gives exactly 1, df optional");
  const double bads[][4] = {{nan, 1, 1, 1}, {1, nan, 1, 1}, {1, 1, nan, 1}, {1, 1, 1, nan}, {inf, 1, 1, 1}, {1, -inf, 1, 1}, {1, 1, inf, 1}, {1, 1, 1, inf}, {1, 1, 0, 1},
                            {1, 1, -1, 1}, {1, 1, 1, 0}, {1, 1, 1, -2}};
  for (const auto &bad : bads) {
    df = 0.0;
    expect(std::isnan(mxa::skat_pvalue_host(bad[0], bad[1], bad[2], bad[3], &df)) && std::isnan(df), "moments that are not finite and positive give NaN");
  }
  for (double x : {1e-8, 0.5, 3.0, 50.0, 700.0, 1400.0}) {
    const double p2 = mxa::skat_pvalue_host(x - 2.0, 0.0, 2.0, 2.0, nullptr), want2 = std::exp(-0.5 * x);          // l = 2
    expect(std::fabs(p2 - want2) <= 0x1p-40 * want2, "l = 2: exp(-x / 2)");
    const double p1 = mxa::skat_pvalue_host(x - 1.0, 0.0, 1.0, 1.0, nullptr), want1 = std::erfc(std::sqrt(0.5 * x));   // l = 1
    expect(std::fabs(p1 - want1) <= 0x1p-40 * want1, "l = 1: erfc(sqrt(x / 2))");
  }
  expect(mxa::skat_pvalue_host(1e300, 0.0, 1.0, 1.0, nullptr) == 0.0, "a statistic beyond every tail gives 0, not NaN");

  if (failures) return 1;
  std::printf("assoc_set_host_check: PASS\n");
  return 0;
}
