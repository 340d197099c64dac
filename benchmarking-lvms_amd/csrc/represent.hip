// represent.hip — K8r: the last launch of every `represent()` level: the mean of the latents over the particles of a pass, with the
// frames past each utterance's length zeroed.
//   z [T, c*B, Z] time-major, row k*B + b (particle-major, as the iw_bound passes lay their rows)  ->  out [T, B, Z]
//   acc = first ? 0 : out;  acc += z[t, k*B+b, :] for k = 0 .. c-1, one fp32 add each;  last ? (t < lens[b] ? acc * scale : 0) : acc
// so the K particles of an utterance are ONE chain of fp32 adds in particle order however they were split into passes: the result
// is bit-identical for every split.  K = 1 (c = 1, first = last = 1, scale = 1) is z itself with the padding zeroed; with `last` the
// dead frames are written as +0 whatever z and out held there (NaN, inf), and with `first` out is never read.
// Evaluation only: no backward.
//
// Mapping: pure streaming, one thread per 4 consecutive latent dimensions of one (t, b) (16-byte loads and stores, Z % 4 == 0),
// grid-stride over the T*B*Z/4 items, no LDS, no atomics, nothing polled.  HBM-bound at (c + 1 [+ 1]) x 4 B per output element.
#include "common.h"

namespace blvm {
namespace {

// n4 = T*B*Z/4 items, zq = Z/4 items per (t, b) row
__global__ __launch_bounds__(256) void particle_mean_kernel(const float4* __restrict__ z, const int32_t* __restrict__ lens, size_t n4,
                                                            int c, int B, int zq, int first, int last, float scale, float4* out) {
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (size_t)gridDim.x * 256) {
    const size_t row = i / zq;  // t * B + b
    const int q = (int)(i - row * zq);
    const size_t t = row / B;
    const int b = (int)(row - t * B);
    float4 acc = first ? make_float4(0.f, 0.f, 0.f, 0.f) : out[i];
    const float4* src = z + ((t * c) * B + b) * zq + q;  // z[t, 0*B + b, 4q]
    for (int k = 0; k < c; ++k) {
      const float4 v = src[(size_t)k * B * zq];
      acc.x += v.x; acc.y += v.y; acc.z += v.z; acc.w += v.w;
    }
    if (last) {
      if ((long long)t < (long long)lens[b]) {
        acc.x *= scale; acc.y *= scale; acc.z *= scale; acc.w *= scale;
      } else {
        acc = make_float4(0.f, 0.f, 0.f, 0.f);
      }
    }
    out[i] = acc;
  }
}

}  // namespace
}  // namespace blvm

extern "C" int blvm_particle_mean(const float* z, const int32_t* lens, int T, int c, int B, int Z, int first, int last, float scale,
                                  float* out, void* stream) {
  using namespace blvm;
  BLVM_REQUIRE(z && lens && out, "particle_mean: null pointer");
  BLVM_REQUIRE(T > 0 && B > 0 && Z > 0 && c >= 1, "particle_mean: bad shape T=%d c=%d B=%d Z=%d", T, c, B, Z);
  BLVM_REQUIRE(Z % 4 == 0, "particle_mean: Z=%d must be a multiple of 4 (16-byte loads and stores)", Z);
  BLVM_REQUIRE(aligned16(z) && aligned16(out), "particle_mean: z and out must be 16-byte aligned");
  BLVM_REQUIRE((long long)c * B < (1ll << 31) && (long long)T * B < (1ll << 31), "particle_mean: too many rows");
  const size_t n4 = (size_t)T * B * (Z / 4);
  size_t blocks = (n4 + 255) / 256;
  if (blocks > 4096) blocks = 4096;
  hipLaunchKernelGGL(particle_mean_kernel, dim3((unsigned)blocks), dim3(256), 0, static_cast<hipStream_t>(stream),
                     reinterpret_cast<const float4*>(z), lens, n4, c, B, Z / 4, first ? 1 : 0, last ? 1 : 0, scale,
                     reinterpret_cast<float4*>(out));
  BLVM_CHECK_LAUNCH("particle_mean");
  return BLVM_OK;
}
