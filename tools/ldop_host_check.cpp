// Stand-alone check of the host-only part of the LD operator object (miraculix_amd/csrc/mxa_ldop_host.h: the check of `last`, first / rowptr / ptr, the byte
// count) against a brute-force restatement, for a CPU build under sanitizers:
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/ldop_host_check.cpp -o ldop_host_check && ./ldop_host_check
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>
#include "../miraculix_amd/csrc/mxa_ldop_host.h"

static int fail(const char *what, long snps, long i) {
  std::printf("FAIL: %s (snps %ld, index %ld)\n", what, snps, i);
  return 1;
}

int main() {
  std::mt19937_64 rng(12345);
  for (int trial = 0; trial < 2000; trial++) {
    const long snps = 1 + (long)(rng() % 300);
    std::vector<int> last((size_t)snps);
    long reach = 0;
    for (long i = 0; i < snps; i++) {                       // a valid window: the end never moves back and never lies before i
      if (rng() % 7 == 0) reach = (long)(rng() % 40);
      long l = i + reach;
      if (i > 0 && l < last[(size_t)i - 1]) l = last[(size_t)i - 1];
      if (l >= snps || rng() % 50 == 0) l = rng() % 3 ? snps - 1 : (i > 0 && last[(size_t)i - 1] > i ? last[(size_t)i - 1] : i);
      last[(size_t)i] = (int)l;
    }
    if (mxa::ldop_check_last(snps, last.data()) != -1) return fail("a valid window was rejected", snps, mxa::ldop_check_last(snps, last.data()));
    std::vector<int> first((size_t)snps);
    std::vector<long> rowptr((size_t)snps + 1), ptr((size_t)snps + 1);
    long mirrored = -1;
    const long entries = mxa::ldop_layout(snps, last.data(), first.data(), rowptr.data(), ptr.data(), &mirrored);
    long up = 0, full = 0;
    for (long i = 0; i < snps; i++) {
      long k = 0;
      while (last[(size_t)k] < i) k++;                      // first[i] from the definition
      if (first[(size_t)i] != k) return fail("first", snps, i);
      if (rowptr[(size_t)i] != up || ptr[(size_t)i] != full) return fail("prefix sums", snps, i);
      up += last[(size_t)i] - i + 1;
      full += last[(size_t)i] - k + 1;
    }
    if (entries != up || rowptr[(size_t)snps] != up || ptr[(size_t)snps] != full || mirrored != full) return fail("totals", snps, snps);
    if (mirrored != 2 * entries - snps) return fail("mirrored != 2 entries - snps", snps, snps);
    if (mxa::ldop_layout(snps, last.data(), nullptr, nullptr, nullptr, nullptr) != entries) return fail("layout without outputs", snps, 0);
    if (mxa::ldop_object_bytes(snps, mirrored) < 8 * mirrored) return fail("bytes", snps, 0);
    // one broken entry: out of range above, below the diagonal, or decreasing -- found at its index
    const long b = (long)(rng() % (unsigned long)snps);
    std::vector<int> bad = last;
    const int kind = (int)(rng() % 3);
    if (kind == 0) bad[(size_t)b] = (int)snps;
    else if (kind == 1) bad[(size_t)b] = (int)b - 1;
    else if (b > 0 && last[(size_t)b - 1] > b) bad[(size_t)b] = last[(size_t)b - 1] - 1;
    else bad[(size_t)b] = (int)b - 1;
    const long at = mxa::ldop_check_last(snps, bad.data());
    if (at < 0 || at > b) return fail("a broken window was accepted", snps, b);
  }
  std::printf("ldop_host_check: PASS\n");
  return 0;
}
