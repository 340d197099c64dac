// logmel.hip — K10: the probe's log-mel spectrogram front end.  A batch of padded waveforms [B,Lmax] goes in, the features
// [B,n_mels,T_max] in dB (and, per utterance and mel bin, normalised) come out.  Two launches (DESIGN "K10"):
//   a. logmel_kernel: one workgroup per (utterance, tile of 32 frames).  The span of waveform under the tile's frames is staged
//      into LDS once, reflected about the utterance's own ends; the windowed DFT is an exact-f32 MFMA product whose A operand is
//      read straight from that span (an implicit frame matrix of row stride hop_length) and whose B operand is the host-built
//      basis [win_length, cos | sin, n_bins] with the window folded in, so the reduction depth is win_length, not n_fft.  The four
//      waves each own a 32 x 32 tile of bins; cos and sin halves are squared and added in registers and the power tile is parked in
//      LDS, 128 bins at a time, where the mel product (32 frames x 32 mels per wave) picks it up as its A operand and accumulates
//      over the chunks of bins in registers.  Neither the [T,n_fft] frame matrix nor the [T,n_bins] power spectrum ever exists in
//      memory.  The dB tile goes back through LDS so that the stores run along T.
//   b. logmel_norm_kernel: one wave per (utterance, mel) row: mean and unbiased standard deviation of the row's T_b frames as
//      deviations from the row's first value (a constant row is exactly 0 and never a rounded mean over 1e-10), in place, zeros
//      behind T_b, out_lens.  The deviation needs every frame of the utterance: hence a second launch.
// No atomics anywhere: bit-identical from call to call, and a row's result does not depend on the rows batched with it.
#include <math.h>

#include "common.h"

namespace blvm {
namespace {

constexpr int LM_ROWS = 32;                // frames per workgroup: one 32x32x2 MFMA row tile
constexpr int LM_CHUNK = 128;              // bins per power chunk: one 32-bin tile per wave
constexpr int LM_PS = LM_CHUNK + 1;        // row stride of the power chunk [32 frames][129]: odd, the A reads of the mel product hit 32 banks
constexpr int LM_OS = LM_ROWS + 1;         // row stride of the output tile [128 mels][33]
constexpr int LM_TILE_FLOATS = 128 * LM_OS;  // >= 32 * LM_PS: the power chunk and the output tile share this piece
constexpr int LM_MAX_FFT = 1024, LM_MIN_WIN = 16, LM_MAX_MELS = 128;

__host__ __device__ inline int round_up(int v, int m) { return (v + m - 1) / m * m; }

// Geometry of the LDS span of one tile: frame i, tap n lives at float i * SP + n + (n / S) * pad.  S = min(hop, win): frames
// that overlap (hop < win) share their samples, frames that do not are staged back to back.  An even S gets one float of padding
// per S (pad = 1), so SP = S + pad is always odd: the 32 lanes of a half wave, one frame each, read 32 different banks.  At
// hop = 64 unpadded they would all read the same one.
struct Span {
  int S, pad, SP, WP, floats;
  __host__ __device__ Span(int win, int hop) {
    S = hop < win ? hop : win;
    pad = (S & 1) ? 0 : 1;
    SP = S + pad;
    WP = round_up(win, 8);  // taps the product walks: the basis rows [win, WP) are zero
    const int last = (LM_ROWS - 1) * S + WP - 1;
    floats = round_up(last + (last / S) * pad + 1, 4);
  }
};

// sample j of an utterance of L samples, reflected about its own ends; 0 where one reflection does not reach (only under frames
// beyond the utterance's last, which are never stored)
__device__ __forceinline__ float reflected(const float* __restrict__ x, long j, int L) {
  if (j < 0) j = -j;
  if (j >= L) j = 2 * ((long)L - 1) - j;
  return (j >= 0 && j < L) ? x[j] : 0.f;
}

__device__ __forceinline__ bool row_ok(int L, int Lmax, int n_fft) { return L > n_fft / 2 && L <= Lmax; }

// ---- a. frames -> windowed DFT -> power -> mel -> dB ---------------------------------------------------------------------------
// basis [WP][2][NBP], fbank [NBP][NMP]; NBP = n_bins rounded up to 32, NMP = n_mels rounded up to 32, both zero-padded.
__global__ __launch_bounds__(256) void logmel_kernel(const float* __restrict__ wave, const int32_t* __restrict__ lens, int Lmax, int n_fft,
                                                     int win, int hop, int n_mels, int tiles, int Tmax,
                                                     const float* __restrict__ basis, const float* __restrict__ fbank,
                                                     float* __restrict__ out) {
  extern __shared__ __align__(16) float smem[];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, li = lane & 31, lh = lane >> 5;
  const int b = blockIdx.x / tiles, t0 = (blockIdx.x % tiles) * LM_ROWS;
  const int L = lens[b];
  if (!row_ok(L, Lmax, n_fft)) return;  // the normalisation kernel marks the row
  const int Tb = 1 + L / hop;
  if (t0 >= Tb) return;  // uniform over the workgroup
  const Span sp(win, hop);
  const int NBP = round_up(n_fft / 2 + 1, 32), NMP = round_up(n_mels, 32);
  float* span = smem;
  float* tile = smem + sp.floats;

  // stage the span: logical element j = i * S + n is sample start + i * hop + n
  {
    const float* x = wave + (size_t)b * Lmax;
    const long start = (long)t0 * hop - n_fft / 2 + (n_fft - win) / 2;
    const int J = (LM_ROWS - 1) * sp.S + sp.WP;
    for (int j = tid; j < J; j += 256) {
      const int i = j / sp.S, n = j - i * sp.S;
      span[j + i * sp.pad] = reflected(x, start + (long)i * hop + n, L);
    }
  }
  __syncthreads();

  f32x16 macc;
#pragma unroll
  for (int r = 0; r < 16; ++r) macc[r] = 0.f;
  const bool mel_wave = w * 32 < NMP;
  const float* ap = span + li * sp.SP + lh;

  for (int c0 = 0; c0 < NBP; c0 += LM_CHUNK) {
    const int bin0 = c0 + w * 32;
    if (bin0 < NBP) {
      f32x16 ac, as;
#pragma unroll
      for (int r = 0; r < 16; ++r) ac[r] = as[r] = 0.f;
      const float* bp = basis + (size_t)lh * 2 * NBP + bin0 + li;
      // q, r: quotient and remainder of the uniform tap k by S; the odd half wave's tap k + 1 crosses into the next S when r + 1 == S
      int q = 0, r = 0;
      for (int k = 0; k < sp.WP; k += 8) {
        float a[4], bc[4], bs[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const int kk = k + 2 * u;
          const int skew = sp.pad ? q + ((lh && r + 1 >= sp.S) ? 1 : 0) : 0;
          a[u] = ap[kk + skew];
          const float* row = bp + (size_t)kk * 2 * NBP;
          bc[u] = row[0];
          bs[u] = row[NBP];
          r += 2;
          while (r >= sp.S) { r -= sp.S; ++q; }
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          ac = __builtin_amdgcn_mfma_f32_32x32x2f32(a[u], bc[u], ac, 0, 0, 0);
          as = __builtin_amdgcn_mfma_f32_32x32x2f32(a[u], bs[u], as, 0, 0, 0);
        }
      }
      // D: column (bin) = li, row (frame) = (r & 3) + 8 (r >> 2) + 4 lh
#pragma unroll
      for (int r2 = 0; r2 < 16; ++r2) {
        const int f = (r2 & 3) + 8 * (r2 >> 2) + 4 * lh;
        tile[f * LM_PS + w * 32 + li] = ac[r2] * ac[r2] + as[r2] * as[r2];
      }
    }
    __syncthreads();
    if (mel_wave) {
      const int depth = min(LM_CHUNK, NBP - c0);  // a multiple of 32: only bins this trip computed
      const float* pp = tile + li * LM_PS + lh;
      const float* fp = fbank + (size_t)(c0 + lh) * NMP + w * 32 + li;
      for (int k = 0; k < depth; k += 8) {
        float a[4], f[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          a[u] = pp[k + 2 * u];
          f[u] = fp[(size_t)(k + 2 * u) * NMP];
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) macc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[u], f[u], macc, 0, 0, 0);
      }
    }
    __syncthreads();  // the tile is free again: the next chunk's powers, or the output tile
  }

  // transpose through LDS: tile[mel][frame], so that consecutive lanes store consecutive frames of one mel row
  if (mel_wave) {
#pragma unroll
    for (int r2 = 0; r2 < 16; ++r2) {
      const int f = (r2 & 3) + 8 * (r2 >> 2) + 4 * lh;
      tile[(w * 32 + li) * LM_OS + f] = macc[r2];
    }
  }
  __syncthreads();
  const int nf = min(LM_ROWS, Tb - t0);
  for (int idx = tid; idx < n_mels * LM_ROWS; idx += 256) {
    const int m = idx >> 5, f = idx & 31;
    if (f < nf) {
      // the floor is -100 dB by definition: an empty filter or digital silence gives that value itself, not log10f's rounding of it
      const float v = tile[m * LM_OS + f];
      out[((size_t)b * n_mels + m) * Tmax + t0 + f] = v <= 1e-10f ? -100.f : 10.f * log10f(v);  // a NaN stays NaN
    }
  }
}

// ---- b. per-row normalisation, zero fill, lengths --------------------------------------------------------------------------------
__device__ __forceinline__ float wave_sum(float v) {
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

__global__ __launch_bounds__(256) void logmel_norm_kernel(const int32_t* __restrict__ lens, int Lmax, int n_fft, int hop, int n_mels,
                                                          size_t rows, int Tmax, int normalize, float* __restrict__ out,
                                                          int32_t* __restrict__ out_lens) {
  const int lane = threadIdx.x & 63;
  const size_t row = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  const int b = (int)(row / n_mels);
  const int L = lens[b];
  const bool ok = row_ok(L, Lmax, n_fft);
  const int Tb = ok ? 1 + L / hop : 0;
  float* x = out + row * Tmax;
  if (lane == 0 && row == (size_t)b * n_mels) out_lens[b] = Tb;
  if (!ok) {  // a length the front end does not take: the row is NaN throughout, its length 0
    for (int t = lane; t < Tmax; t += 64) x[t] = NAN;
    return;
  }
  if (normalize) {
    const float x0 = x[0];
    float s = 0.f;
    for (int t = lane; t < Tb; t += 64) s += x[t] - x0;
    const float shift = wave_sum(s) / (float)Tb;  // mean - x0
    float ss = 0.f;
    for (int t = lane; t < Tb; t += 64) {
      const float d = (x[t] - x0) - shift;
      ss += d * d;
    }
    const float sd = sqrtf(wave_sum(ss) / (float)(Tb - 1));  // Tb = 1: 0 / 0, NaN as torch.std gives
    const float den = sd + 1e-10f;
    for (int t = lane; t < Tb; t += 64) x[t] = ((x[t] - x0) - shift) / den;
  }
  for (int t = Tb + lane; t < Tmax; t += 64) x[t] = 0.f;
}

}  // namespace
}  // namespace blvm

using namespace blvm;

extern "C" int blvm_logmel(const float* wave, const int32_t* lens, int B, int Lmax, int n_fft, int win_length, int hop_length,
                           int n_mels, const float* basis, const float* fbank, int normalize, float* out, int32_t* out_lens,
                           void* stream) {
  BLVM_REQUIRE(n_fft >= 2 && n_fft % 2 == 0 && n_fft <= LM_MAX_FFT, "blvm_logmel: n_fft = %d: need an even n_fft of at most %d", n_fft,
               LM_MAX_FFT);
  BLVM_REQUIRE(win_length >= LM_MIN_WIN && win_length <= n_fft, "blvm_logmel: win_length = %d: need %d <= win_length <= n_fft = %d",
               win_length, LM_MIN_WIN, n_fft);
  BLVM_REQUIRE(hop_length >= 1, "blvm_logmel: hop_length = %d: need hop_length >= 1", hop_length);
  BLVM_REQUIRE(n_mels >= 1 && n_mels <= LM_MAX_MELS, "blvm_logmel: n_mels = %d: need 1 <= n_mels <= %d", n_mels, LM_MAX_MELS);
  BLVM_REQUIRE(B >= 1 && Lmax > n_fft / 2, "blvm_logmel: B = %d, Lmax = %d: need B >= 1 and more than n_fft / 2 = %d samples per row", B,
               Lmax, n_fft / 2);
  const int Tmax = 1 + Lmax / hop_length;
  BLVM_REQUIRE((size_t)B * Tmax < ((size_t)1 << 31), "blvm_logmel: B * T_max = %zu frames: need fewer than 2^31", (size_t)B * Tmax);
  const size_t rows = (size_t)B * n_mels;
  BLVM_REQUIRE(rows < ((size_t)1 << 31), "blvm_logmel: B * n_mels = %zu rows: need fewer than 2^31", rows);
  BLVM_REQUIRE(normalize == 0 || normalize == 1, "blvm_logmel: normalize = %d: 0 or 1", normalize);
  BLVM_REQUIRE(wave && lens && basis && fbank && out && out_lens, "blvm_logmel: NULL wave, lens, basis, fbank, out or out_lens");
  hipStream_t s = (hipStream_t)stream;
  const int tiles = (Tmax + LM_ROWS - 1) / LM_ROWS;
  const size_t lds = sizeof(float) * ((size_t)Span(win_length, hop_length).floats + LM_TILE_FLOATS);
  if (lds > 64 * 1024)
    BLVM_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(logmel_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  hipLaunchKernelGGL(logmel_kernel, dim3((unsigned)((size_t)B * tiles)), dim3(256), lds, s, wave, lens, Lmax, n_fft, win_length,
                     hop_length, n_mels, tiles, Tmax, basis, fbank, out);
  BLVM_CHECK_LAUNCH("logmel_kernel");
  hipLaunchKernelGGL(logmel_norm_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, s, lens, Lmax, n_fft, hop_length, n_mels, rows,
                     Tmax, normalize, out, out_lens);
  BLVM_CHECK_LAUNCH("logmel_norm_kernel");
  return BLVM_OK;
}
