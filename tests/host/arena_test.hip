#include "common.h"
#include <cstdio>
namespace blvm { void set_error(const char*, ...) {} }
using blvm::Arena;
int main() {
  int bad = 0;
  const size_t counts[] = {1, 4, 5, 0, 7, 64, 3, 0, 1023, 2};
  auto rounded = [](size_t c) { return (c + 3) / 4 * 4; };
  // a null base gives sizes only: every piece is null, the offsets advance all the same
  Arena sizes;
  size_t want = 0;
  for (size_t c : counts) {
    bad += sizes.take(c) != nullptr;
    want += rounded(c);
    bad += sizes.floats() != want || sizes.floats() % 4 != 0;
  }
  bad += sizes.bytes_from(nullptr) != 0;
  // a real base: pieces at offsets rounded to 4 floats, take(0) = the running end, the same total as the null arena
  static float buf[2048];
  Arena ar{buf};
  const float* piece[10];
  size_t at = 0;
  for (int i = 0; i < 10; ++i) {
    piece[i] = ar.take(counts[i]);
    bad += piece[i] != buf + at || (piece[i] - buf) % 4 != 0;
    at += rounded(counts[i]);
    bad += ar.take(0) != buf + at || ar.floats() != at;  // take(0) returns the running end and moves nothing
  }
  bad += ar.floats() != sizes.floats();
  // bytes_from(p) = the rounded sizes taken since p, for every earlier piece
  for (int i = 0; i < 10; ++i) {
    size_t since = 0;
    for (int k = i; k < 10; ++k) since += rounded(counts[k]);
    bad += ar.bytes_from(piece[i]) != sizeof(float) * since;
  }
  bad += ar.bytes_from(ar.take(0)) != 0;
  // the offset form hands out the same places, from any starting offset
  Arena offs{nullptr, 40};
  at = 40;
  for (size_t c : counts) {
    bad += offs.take_off(c) != at;
    at += rounded(c);
  }
  bad += offs.floats() != at;
  printf("arena: %d errors\n", bad);
  return bad != 0;
}
