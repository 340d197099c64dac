// decode_tiles.h — the arithmetic the one-launch generators share (device side only).
//
// K10c (wavenet_decode.hip), K10d (stcn_decode.hip), K1c (vrnn_decode.hip), the chain engine's K_DMOLS tile (pchain.h) and
// mix_sample_kernel (dmol.hip) all end in the same draw, and the two convolutional decoders walk the same gated residual block.
// Each of these is written once here; a kernel supplies its buffers, its widths and the last line of an epilogue.
//   mix_pick / logistic_draw   the DMoL draw
//   gauss_draw                 the draw of the GMM head (behind the same pick) and of the plain Gaussian head
//   cat_pick                   the categorical draw of K10c's softmax head
//   tile16 / tile_layer        "16x16 tiles over the waves, product from an LDS operand, + bias, epilogue"
//   gated_ring_block           one gated residual block on one new frame, with its ring buffer
// Nothing here holds a barrier the caller does not see, except gated_ring_block, whose four are part of its contract.
// Deliberately NOT here: the compile-time-width path of K10c (block_fast and its register sets) and K1c's weight stream — tuned
// instruction by instruction and without a second copy anywhere.
#pragma once
#include "common.h"

namespace blvm {

// ---- the DMoL draw (blvm/utils/variational.py:309-349) -----------------------------------------------------------------------
// Gumbel-max component pick over the K logits p[0..K): argmax of p[m] - log(-log u(m)); !noisy: of the logits alone (the mode).
// First maximum, as torch.argmax.  u is a callable m -> float, so the draws may sit in global memory or, with a compile-time
// count KC (the loop is unrolled, every index static), in a register array of the caller.
template <int KC = 0, class U>
__device__ __forceinline__ int mix_pick_from(const float* p, int K, bool noisy, U u) {
  int best = 0;
  float bv = -INFINITY;
  auto step = [&](int m) {
    float s = p[m];
    if (noisy) s -= logf(-logf(u(m)));
    if (s > bv) { bv = s; best = m; }
  };
  if constexpr (KC > 0) {
#pragma unroll
    for (int m = 0; m < KC; ++m) step(m);
  } else {
    for (int m = 0; m < K; ++m) step(m);
  }
  return best;
}

// the same with the draws u[0..K) behind a pointer; NULL: the arg-max-logit component
template <int KC = 0>
__device__ __forceinline__ int mix_pick(const float* p, int K, const float* u) {
  return mix_pick_from<KC>(p, K, u != nullptr, [u](int m) { return u[m]; });
}

// x = loc + exp(max(raw, log_eps)) * logit(v), clamped to [-1, 1] (variational.py:283-305); v uniform in (0, 1)
__device__ __forceinline__ float logistic_draw(float loc, float raw, float v, float log_eps) {
  const float x = loc + expf(fmaxf(raw, log_eps)) * (logf(v) - logf(1.f - v));
  return fminf(fmaxf(x, -1.f), 1.f);
}

// x = mu + sd(raw) * n, n standard normal: sd = softplus_beta(raw) + sd_eps, or raw itself when sd_beta == 0 (the scales are
// standard deviations already).  No clamp.  The draw of the GMM and Gaussian heads (variational.py:156-195).
__device__ __forceinline__ float gauss_draw(float mu, float raw, float n, float sd_beta, float sd_eps) {
  return mu + (sd_beta > 0.f ? softplus_beta(raw, sd_beta, 1.f / sd_beta) + sd_eps : raw) * n;
}

// ---- the categorical draw (the rule of tests/cat_cases.py::check_draws) ---------------------------------------------------------
// One class from the V logits l[0..V) of a row in LDS, by the LANES consecutive lanes (a power of two <= 64, aligned) that call it
// together; every lane returns the class.  Lane j owns the classes [j chunk, (j + 1) chunk), chunk = ceil(V / LANES).
// !noisy: the arg-max, first maximum (as torch.argmax; 0 when no logit compares above -inf).
// noisy: inverse CDF of e = exp(l - max l) at u — the first class whose prefix sum reaches u * total, V - 1 if none does (u next to
// 1, or a non-finite logit: the class comes from comparisons only, never from arithmetic on a logit, so it is always in [0, V)).
// The order of every sum is fixed — in a lane class after class, across lanes a Hillis-Steele scan — so two launches agree to the
// bit; no atomics.  l is overwritten with e.  No barrier: a lane re-reads only what it wrote itself.
template <int LANES>
__device__ __forceinline__ int cat_pick(float* l, int V, bool noisy, float u) {
  const int j = threadIdx.x & (LANES - 1);
  const int chunk = (V + LANES - 1) / LANES;
  const int lo = min(j * chunk, V), hi = min(lo + chunk, V);
  float bv = -INFINITY;
  int best = lo < V ? lo : V - 1;
  for (int k = lo; k < hi; ++k) {
    const float s = l[k];
    if (s > bv) { bv = s; best = k; }
  }
#pragma unroll
  for (int m = LANES / 2; m > 0; m >>= 1) {
    const float ov = __shfl_xor(bv, m, LANES);
    const int oi = __shfl_xor(best, m, LANES);
    if (ov > bv || (ov == bv && oi < best)) { bv = ov; best = oi; }
  }
  if (!noisy) return best;
  float part = 0.f;
  for (int k = lo; k < hi; ++k) {
    const float e = expf(l[k] - bv);
    l[k] = e;
    part += e;
  }
  float inc = part;  // -> the prefix sum up to and including this lane's classes
#pragma unroll
  for (int d = 1; d < LANES; d <<= 1) {
    const float o = __shfl_up(inc, d, LANES);
    if (j >= d) inc += o;
  }
  const float target = u * __shfl(inc, LANES - 1, LANES);
  float cum = __shfl_up(inc, 1, LANES);
  if (j == 0) cum = 0.f;
  int found = V;
  for (int k = lo; k < hi; ++k) {
    cum += l[k];
    if (found == V && cum >= target) found = k;
  }
#pragma unroll
  for (int m = LANES / 2; m > 0; m >>= 1) found = min(found, __shfl_xor(found, m, LANES));
  return found < V ? found : V - 1;
}

// ---- the tile layer ----------------------------------------------------------------------------------------------------------
// Output tile `tile` (columns 16 tile .. +15) of A [16, K] (LDS, leading dimension lda) times W [N, K]^T (row-major, or its T16
// operand copy), computed by the calling wave: epi(row, col, product + bias[col]) for the four rows this lane holds.
template <bool T16, class Epi>
__device__ __forceinline__ void tile16(const float* A, int lda, const float* W, int K, int tile, const float* bias, Epi epi) {
  const int lane = threadIdx.x & 63, q = lane >> 4, col = tile * 16 + (lane & 15);
  const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
  const f32x4 acc = wave_gemm16<1, T16>(A, lda, 0, 16, W, K, tile * 16, K, 0, zero4);
  const float b = bias[col];
#pragma unroll
  for (int r = 0; r < 4; ++r) epi(4 * q + r, col, acc[r] + b);
}

// tiles [lo, hi) dealt over the NW waves of the workgroup.  No barrier: the caller places its own after the layer.
template <int NW, bool T16, class Epi>
__device__ __forceinline__ void tile_layer(const float* A, int lda, const float* W, int K, int lo, int hi, const float* bias, Epi epi) {
  for (int tile = lo + (int)(threadIdx.x >> 6); tile < hi; tile += NW) tile16<T16>(A, lda, W, K, tile, bias, epi);
}

// ---- the gated residual block of the cached formulation (arXiv:1611.09482) -----------------------------------------------------
// LDS of a decoder that runs gated blocks on 16 rows of width C (floats; ldV, ldP, ldA multiples of 4):
struct GateLds {
  float* sH;   int ldH;  // [16][ldH >= C]     the block's input; the residual output replaces it
  float* sV;   int ldV;  // [16][ldV >= 2C]    interleaved taps: k = 2c + tap
  float* sPre; int ldP;  // [16][ldP >= 2C]    gate pre-activations
  float* sAct; int ldA;  // [16][ldA >= C]     gated activations
};

// One block on the frame in sH, for rows b0 .. b0+15 of B.  ring [d, B, C] holds the block's input over the last d frames, the
// frame d back in `slot`: read it, put the new frame in its place (a ring element is read and rewritten by the same thread),
//   sV = (old, new) interleaved;  sPre = conv_t sV + conv_b;  sAct = tanh(sPre[:C]) * sigmoid(sPre[C:]);
//   tiles [rs_lo, rs_hi) of rs_t sAct + rs_b:  column o < C: sH = (value + sH) * inv_std;  o >= C: skip(row, o - C, value).
// steady: the response to an input constant in time — both taps = sH, every slot of the ring filled with sH.
// conv_t [2C, 2C] and rs_t [C + skip width, C] are T16 operand copies.  rs_lo = C/16 leaves the residual half out (a last
// block), rs_hi = C/16 the skip half.  Four workgroup barriers, the last one after the epilogue.
template <int NW, class Skip>
__device__ __forceinline__ void gated_ring_block(const GateLds& g, int C, const float* conv_t, const float* conv_b, const float* rs_t,
                                                 const float* rs_b, float* ring, int d, int slot, bool steady, int b0, int B,
                                                 float inv_std, int rs_lo, int rs_hi, Skip skip) {
  constexpr int NT = NW * 64;
  const int tid = threadIdx.x;
  for (int idx = tid; idx < 16 * C; idx += NT) {
    const int r = idx / C, c = idx - r * C;
    const float cur = g.sH[r * g.ldH + c];
    float old = cur;
    if (b0 + r < B) {
      if (steady) {
        for (int s = 0; s < d; ++s) ring[((size_t)s * B + b0 + r) * C + c] = cur;
      } else {
        float* p = ring + ((size_t)slot * B + b0 + r) * C + c;
        old = *p;
        *p = cur;
      }
    }
    g.sV[r * g.ldV + 2 * c] = old;
    g.sV[r * g.ldV + 2 * c + 1] = cur;
  }
  __syncthreads();
  tile_layer<NW, true>(g.sV, g.ldV, conv_t, 2 * C, 0, 2 * C / 16, conv_b, [&](int row, int o, float val) { g.sPre[row * g.ldP + o] = val; });
  __syncthreads();
  for (int idx = tid; idx < 16 * C; idx += NT) {
    const int r = idx / C, c = idx - r * C;
    g.sAct[r * g.ldA + c] = tanhf(g.sPre[r * g.ldP + c]) * sigmoidf_(g.sPre[r * g.ldP + C + c]);
  }
  __syncthreads();
  tile_layer<NW, true>(g.sAct, g.ldA, rs_t, C, rs_lo, rs_hi, rs_b, [&](int row, int o, float val) {
    if (o < C) g.sH[row * g.ldH + o] = (val + g.sH[row * g.ldH + o]) * inv_std;
    else skip(row, o - C, val);
  });
  __syncthreads();
}

}  // namespace blvm
