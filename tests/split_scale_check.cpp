// Stand-alone host check of the split-precision scale helpers (csrc/rgcn_split.h): scale_exponent() maps a tensor
// maximum to the exponent s with amax * 2^s in [2^14, 2^15), clamped to +-100, and to 0 for a maximum that is zero,
// denormal, infinite or NaN (scale 1: the rule include/rgcn_hip.h states for non-finite operands); pow2f(s) is 2^s as a
// normal float.  Prints one line per input and "split_scale_check ok"; exits non-zero on the first mismatch.
#include <cfloat>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>

#include "primekg_rgcn_linkprediction_amd/csrc/rgcn_split.h"

static int failures = 0;

static void expect(const char* what, float amax, int want) {
  const int got = scale_exponent(amax);
  std::printf("%-12s %-14g exponent %4d scale %g\n", what, (double)amax, got, (double)pow2f(got));
  if (got != want) {
    std::printf("  MISMATCH: want %d\n", want);
    ++failures;
  }
}

int main() {
  const float inf = std::numeric_limits<float>::infinity();
  expect("nan", std::numeric_limits<float>::quiet_NaN(), 0);
  expect("-nan", -std::numeric_limits<float>::quiet_NaN(), 0);
  expect("+inf", inf, 0);
  expect("-inf", -inf, 0);
  expect("zero", 0.f, 0);
  expect("-zero", -0.f, 0);
  expect("denormal", std::numeric_limits<float>::denorm_min(), 0);
  expect("denormal max", FLT_MIN / 2, 0);
  expect("FLT_MIN", FLT_MIN, 100);                 // 2^-126: 141 - 1 = 140, clamped
  expect("FLT_MAX", FLT_MAX, -100);                // [2^127, 2^128): 141 - 254 = -113, clamped
  expect("one", 1.f, 14);
  expect("-one", -1.f, 14);                        // the sign bit is not part of the exponent field
  expect("1.99", 1.99f, 14);
  expect("2^14", 16384.f, 0);
  expect("2^15", 32768.f, -1);
  expect("2^-86", std::ldexp(1.f, -86), 100);      // the last exponent before the clamp
  expect("2^-87", std::ldexp(1.f, -87), 100);
  expect("2^114", std::ldexp(1.f, 114), -100);
  expect("2^113", std::ldexp(1.f, 113), -99);
  // pow2f: exact powers of two over the clamped range, both it and its inverse normal
  for (int s = -100; s <= 100; ++s) {
    const float p = pow2f(s), q = pow2f(-s);
    if (p != std::ldexp(1.f, s) || !std::isnormal(p) || p * q != 1.f) {
      std::printf("pow2f(%d) = %g\n", s, (double)p);
      ++failures;
    }
  }
  // every finite normal maximum lands in [2^14, 2^15) unless the clamp binds
  for (int e = -126; e <= 127; ++e) {
    const float lo = std::ldexp(1.f, e), hi = std::nextafter(std::ldexp(1.f, e + 1 > 127 ? 127 : e + 1), 0.f);
    for (float a : {lo, e < 127 ? hi : FLT_MAX}) {
      const int s = scale_exponent(a);
      const double scaled = (double)a * std::ldexp(1.0, s);
      const bool clamped = s == 100 || s == -100;
      if (!clamped && !(scaled >= 16384.0 && scaled < 32768.0)) {
        std::printf("amax %g: scaled to %g\n", (double)a, scaled);
        ++failures;
      }
    }
  }
  if (failures) return 1;
  std::printf("split_scale_check ok\n");
  return 0;
}
