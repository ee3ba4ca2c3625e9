// Stand-alone check of the argument rules of mxa_assoc_score_firth (miraculix_amd/csrc/mxa_assoc_host.h: assoc_score_firth_args), for a CPU build under sanitizers:
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -static-libasan -static-libubsan tools/assoc_firth_host_check.cpp \
//       -o assoc_firth_host_check && ./assoc_firth_host_check
// (the runtimes linked statically: the program is self-contained and runs in whatever environment it is started in)
// Every error path of the entry is driven once and must name its cause; the rules dereference no pointer, so every operand is a heap block of ONE byte: a read
// of an operand would be reported.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <memory>
#include "../miraculix_amd/csrc/mxa_assoc_host.h"

namespace {

struct Args {
  const void *plink, *P, *R, *Wt, *H, *score, *var, *zstat, *beta;
  long snps = 5, indiv = 12, ldp = 12, ldr = 12, ldw = 12, ldh = 12, ldo = 5;
  int n = 2, kh = 3, penalty = 1, max_iter = 50;
  double z_cutoff = 2.0, tol = 0x1p-30;
  const char *check() const {
    return mxa::assoc_score_firth_args(plink, snps, indiv, P, ldp, R, ldr, Wt, ldw, H, ldh, n, kh, z_cutoff, penalty, tol, max_iter, score, var, zstat, beta, ldo);
  }
};

int failures = 0;

void accepted(const char *what, const Args &a) {
  const char *bad = a.check();
  if (bad) { std::printf("FAIL: %s was refused: %s\n", what, bad); failures++; }
}

void refused(const char *what, const Args &a, const char *word) {
  const char *bad = a.check();
  if (!bad) { std::printf("FAIL: %s was accepted\n", what); failures++; }
  else if (!std::strstr(bad, word)) { std::printf("FAIL: %s: the message \"%s\" does not name \"%s\"\n", what, bad, word); failures++; }
}

}  // namespace

int main() {
  std::unique_ptr<char[]> blocks[9];
  for (auto &b : blocks) b.reset(new char[1]);
  Args ok;
  ok.plink = blocks[0].get(); ok.P = blocks[1].get(); ok.R = blocks[2].get(); ok.Wt = blocks[3].get(); ok.H = blocks[4].get();
  ok.score = blocks[5].get(); ok.var = blocks[6].get(); ok.zstat = blocks[7].get(); ok.beta = blocks[8].get();
  const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
  const long big = mxa::kAssocMaxIndiv;
  Args a;

  accepted("the plain call", ok);
  a = ok; a.penalty = 0; accepted("penalty 0", a);
  a = ok; a.z_cutoff = inf; accepted("an infinite cutoff", a);
  a = ok; a.z_cutoff = 0.0; accepted("a cutoff of zero", a);
  a = ok; a.H = nullptr; a.kh = 0; a.ldh = 0; accepted("kh = 0 with a NULL H", a);
  a = ok; a.var = nullptr; a.zstat = nullptr; accepted("score alone beside beta", a);
  a = ok; a.tol = 0.5; a.max_iter = 1; accepted("tol 0.5 and one evaluation", a);
  a = ok; a.indiv = a.ldp = a.ldr = a.ldw = a.ldh = big; accepted("the largest indiv", a);
  a = ok; a.n = 65535 / 5; accepted("n (kh + 2) = 65535", a);

  // the errors of mxa_assoc_score
  a = ok; a.plink = nullptr; refused("a NULL plink", a, "plink");
  a = ok; a.R = nullptr; refused("a NULL R", a, "R and Wt");
  a = ok; a.Wt = nullptr; refused("a NULL Wt", a, "R and Wt");
  a = ok; a.snps = 0; refused("snps = 0", a, "positive");
  a = ok; a.indiv = 0; refused("indiv = 0", a, "positive");
  a = ok; a.n = 0; refused("n = 0", a, "positive");
  a = ok; a.n = -1; refused("n = -1", a, "positive");
  a = ok; a.kh = -1; refused("kh = -1", a, "kh");
  a = ok; a.H = nullptr; refused("a NULL H with kh > 0", a, "H is NULL");
  a = ok; a.n = 65535 / 5 + 1; refused("n (kh + 2) = 65540", a, "65535");
  a = ok; a.n = 1; a.kh = 65534; refused("kh = 65534", a, "65535");
  a = ok; a.ldr = 11; refused("ldr below indiv", a, "ldr");
  a = ok; a.ldw = 11; refused("ldw below indiv", a, "ldw");
  a = ok; a.ldh = 11; refused("ldh below indiv", a, "ldh");
  a = ok; a.indiv = a.ldp = a.ldr = a.ldw = a.ldh = big + 1; refused("indiv beyond the limit", a, "47 453 132");
  a = ok; a.score = a.var = a.zstat = nullptr; refused("score, var and zstat all NULL", a, "all NULL");
  a = ok; a.ldo = 4; refused("ldo below snps", a, "ldo");
  // those of mxa_assoc_score_spa, with beta in pval's place
  a = ok; a.P = nullptr; refused("a NULL P", a, "P and beta");
  a = ok; a.beta = nullptr; refused("a NULL beta", a, "P and beta");
  a = ok; a.ldp = 11; refused("ldp below indiv", a, "ldp");
  a = ok; a.z_cutoff = -1e-300; refused("a negative cutoff", a, "z_cutoff");
  a = ok; a.z_cutoff = -inf; refused("a cutoff of -inf", a, "z_cutoff");
  a = ok; a.z_cutoff = nan; refused("a NaN cutoff", a, "z_cutoff");
  for (double tol : {0.0, 1.0, -0.5, nan, inf}) { a = ok; a.tol = tol; refused("a tol outside (0, 1)", a, "tol"); }
  a = ok; a.max_iter = 0; refused("max_iter = 0", a, "max_iter");
  a = ok; a.max_iter = -3; refused("max_iter = -3", a, "max_iter");
  // its own
  for (int penalty : {-1, 2, 3, std::numeric_limits<int>::min(), std::numeric_limits<int>::max()}) { a = ok; a.penalty = penalty; refused("a penalty that is not 0 or 1", a, "penalty"); }
  // the order: the scan's rules come first, the penalty last
  a = ok; a.penalty = 2; a.snps = 0; refused("snps = 0 with a wrong penalty", a, "positive");
  a = ok; a.penalty = 2; a.max_iter = 0; refused("max_iter = 0 with a wrong penalty", a, "max_iter");

  if (failures) return 1;
  std::printf("assoc_firth_host_check: PASS\n");
  return 0;
}
