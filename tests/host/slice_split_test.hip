// The three-slice split of an fp32 operand (csrc/bf16_slice.h: slice3, slice_pack) that the sliced weight-gradient tile of gemm.hip
// feeds to the bf16 matrix pipe, on the host:
//   - hi + mid + lo == x exactly (both association orders) for every finite x: +-0, +-FLT_MIN, subnormals, +-FLT_MAX, values with
//     all 24 significand bits set at every exponent, 10^6 random bit patterns;
//   - hi and mid are bf16-exact (low 16 bits clear) always; lo is bf16-exact whenever x is a multiple of 2^-133, the spacing of
//     bf16 subnormals -- every |x| >= 2^-110 and FLT_MIN among them.  A finer x cannot be a sum of bf16 numbers at all; there the
//     packed slices (what the MFMA sees) miss x by less than 2^-133;
//   - slice_pack puts the first slice's upper half in the low 16 bits and the second's in the high 16 bits;
//   - +-inf gives hi = +-inf and NaN mid / lo; a NaN gives NaN mid / lo (hi is NaN, or inf when the payload lies in the low 16 bits).
#include "bf16_slice.h"
#include <cfloat>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
using namespace blvm;

static int errors = 0, checks = 0;
static float from_bits(uint32_t u) {
  float f;
  std::memcpy(&f, &u, 4);
  return f;
}
static uint32_t bits(float f) {
  uint32_t u;
  std::memcpy(&u, &f, 4);
  return u;
}
static bool bf16_exact(float f) { return (bits(f) & 0xFFFFu) == 0; }
static float unpack(uint32_t w, int half) { return from_bits(half ? (w & 0xFFFF0000u) : (w << 16)); }
#define CHECK(c, ...) do { ++checks; if (!(c)) { if (++errors <= 20) { std::printf("FAIL %s: ", #c); std::printf(__VA_ARGS__); std::printf("\n"); } } } while (0)

static void check_finite(float x) {
  const uint32_t u = bits(x);
  const Slices3 s = slice3(x);
  volatile float a = s.hi + s.mid;
  a = a + s.lo;
  volatile float b = s.mid + s.lo;
  b = s.hi + b;
  CHECK(bits(a) == u || (x == 0.f && a == 0.f), "x=%08x hi+mid+lo=%08x", u, bits(a));
  CHECK(bits(b) == u || (x == 0.f && b == 0.f), "x=%08x hi+(mid+lo)=%08x", u, bits(b));
  CHECK(bf16_exact(s.hi) && bf16_exact(s.mid), "x=%08x hi=%08x mid=%08x", u, bits(s.hi), bits(s.mid));
  if (std::fabs(x) >= 0x1p-110f)  // (below, x - hi is an fp32 subnormal and its mask cuts at 2^-133 instead of after 8 bits)
    CHECK(std::fabs(s.mid) <= std::fabs(s.hi) * 0x1p-7f && std::fabs(s.lo) <= std::fabs(s.hi) * 0x1p-15f, "x=%08x slice sizes", u);
  // x is a multiple of 2^-133 iff its scaled value is an integer (exact: a power-of-two scaling in double)
  const double q = std::ldexp((double)x, 133);
  const bool coarse = q == std::floor(q);
  const uint32_t w = slice_pack(s.lo, s.lo);
  if (coarse) {
    CHECK(bf16_exact(s.lo), "x=%08x lo=%08x", u, bits(s.lo));
  } else {
    CHECK(std::fabs(x) < 0x1p-110f, "x=%08x finer than 2^-133 above 2^-110", u);
    const double packed = (double)s.hi + (double)s.mid + (double)unpack(w, 0);
    CHECK(std::fabs(packed - (double)x) < 0x1p-133, "x=%08x packed slices off by %g", u, packed - (double)x);
  }
  const uint32_t p = slice_pack(s.hi, s.mid);
  CHECK(bits(unpack(p, 0)) == bits(s.hi) && bits(unpack(p, 1)) == bits(s.mid), "x=%08x pack=%08x", u, p);
  CHECK(bits(unpack(w, 0)) == (bits(s.lo) & 0xFFFF0000u) && unpack(w, 1) == unpack(w, 0), "x=%08x pack(lo,lo)=%08x", u, w);
}

int main() {
  const float special[] = {0.f, -0.f, FLT_MIN, -FLT_MIN, FLT_MAX, -FLT_MAX, 1.f, -1.f, 0x1p-110f, 0x1.fffffep-111f, 0x1p-133f, 0x1p-134f,
                           FLT_TRUE_MIN, -FLT_TRUE_MIN, from_bits(0x007FFFFFu), from_bits(0x807FFFFFu), from_bits(0x00010000u),
                           from_bits(0x0000FFFFu), from_bits(0x00800001u), from_bits(0x00FFFFFFu)};
  for (const float x : special) check_finite(x);
  for (uint32_t e = 0; e < 255; ++e)  // all 24 significand bits set (e = 0: every fraction bit of a subnormal), both signs
    for (uint32_t sgn = 0; sgn < 2; ++sgn) {
      check_finite(from_bits(sgn << 31 | e << 23 | 0x7FFFFFu));
      check_finite(from_bits(sgn << 31 | e << 23 | 0x7F7F7Fu));
      check_finite(from_bits(sgn << 31 | e << 23 | 0x00FFFFu));
      check_finite(from_bits(sgn << 31 | e << 23 | 0x0000FFu));
    }
  uint64_t rng = 0x9E3779B97F4A7C15ull;
  int nonfinite = 0;
  for (int i = 0; i < 1000000; ++i) {
    rng = rng * 6364136223846793005ull + 1442695040888963407ull;
    const uint32_t u = (uint32_t)(rng >> 32);
    const float x = from_bits(u);
    if (std::isfinite(x)) {
      check_finite(x);
    } else {
      ++nonfinite;
      const Slices3 s = slice3(x);
      CHECK(std::isnan(s.mid) && std::isnan(s.lo) && !std::isfinite(s.hi), "x=%08x nonfinite", u);
    }
  }
  // the documented non-finite behaviour
  for (const float inf : {INFINITY, -INFINITY}) {
    const Slices3 s = slice3(inf);
    CHECK(s.hi == inf && std::isnan(s.mid) && std::isnan(s.lo), "inf");
    CHECK(std::isnan(s.hi * 1.f + s.mid * 1.f), "inf operand: the kept terms sum to NaN");
  }
  {
    const Slices3 q = slice3(from_bits(0x7FC00000u)), p = slice3(from_bits(0x7F800001u));
    CHECK(std::isnan(q.hi) && std::isnan(q.mid) && std::isnan(q.lo), "quiet NaN");
    CHECK(std::isinf(p.hi) && std::isnan(p.mid) && std::isnan(p.lo), "NaN with a low payload");
  }
  std::printf("slice_split_test: %d checks (%d non-finite random patterns): %d errors\n", checks, nonfinite, errors);
  return errors ? 1 : 0;
}
