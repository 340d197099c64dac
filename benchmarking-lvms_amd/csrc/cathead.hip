// cathead.hip — K7d: the categorical (softmax) output head fused with its Linear(C -> V).  The [frames, V] logits are never stored:
// every kernel recomputes 32-class x 32-frame tiles of them with v_mfma_f32_32x32x2_f32 (exact fp32 fma chains) and consumes each
// tile where it was made.
//
// Orientation.  A tile is W_tile [32 classes, C] . X^T [C, 32 frames]: classes on the MFMA's M axis, frames on its N axis.  The
// C/D map (col = lane & 31, row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5)) then gives lane (li, lh) frame li and 16 of the tile's
// classes in its 16 accumulator registers, so a frame's running maximum / sum of exponentials / target logit live in the registers
// of two lanes (li, li + 32): 16 in-register steps per tile and ONE cross-half exchange per frame at the very end.
// Operand k order: lane half lh feeds k = chunk + 4 lh + c to the c-th MFMA of an 8-k chunk from one 16-byte load (A and B alike,
// as wave_gemm32 in common.h).
//
//   cat_rows_kernel<false>  forward: a workgroup stages 32 frames' activations once (masked frames as zeros), its 4 waves walk the
//                           class tiles (tile w, w + 4, ...) with an online max / sum-exp, then merge.  Writes lse and ll.
//   cat_rows_kernel<true>   d_dec: the same walk 128 classes at a time; d = g mask (onehot - exp(l - lse)) goes to LDS as
//                           [128 classes][32 frames], which is the B operand of d_dec^T [C, 32] += W_s^T [C, 128] . d with no
//                           transposition; each wave owns 32-channel chunks of C.
//   cat_cls_kernel          dW, db: a workgroup owns 32 classes (its W rows in LDS) and walks a range of 128-frame blocks; d goes to
//                           LDS as [32 classes][128 frames] (padded rows), the A operand of dW_tile [32, C] += d . X.  The frame
//                           range is split only as far as fills the chip; partials go to the workspace and cat_reduce_kernel sums
//                           them in split order.  No float atomics anywhere: results are identical from run to run.
//   cat_sum_kernel          log_prob[b] += sum of ll[b, :] in float64, in a fixed order.
//   cat_sample_kernel       arg-max / inverse-CDF draw on materialised logits, one workgroup per row.
#include <math.h>

#include "common.h"

namespace blvm {
namespace {

constexpr int CAT_FT = 32;        // frames per logits tile (MFMA N)
constexpr int CAT_CT = 32;        // classes per logits tile (MFMA M)
constexpr int CAT_NW = 4;         // waves per workgroup
constexpr int CAT_SUPER = CAT_NW * CAT_CT;  // classes per d_dec step | frames per dW step
constexpr int CAT_DLD = CAT_SUPER + 1;      // row stride of the dW kernel's d tile: odd, so a column read hits 32 banks
constexpr int CAT_FILL = 512;     // workgroups the dW kernel aims for (2 per CU)

struct CatArgs {
  const float* dec;
  const float* W;
  const float* bias;
  const int32_t* y;
  const int32_t* x_sl;
  const float* g;       // [B] (backward)
  const float* lse_in;  // [frames] (backward)
  float* lse;           // [frames] (forward)
  float* ll;            // [B,T] (forward)
  float* d_dec;         // [frames, C]
  float* dW_out;        // [V, C] or the partials [splits, V, C]
  float* db_out;        // [V] or [splits, V]
  int B, T, S, C, V;
  int frames;           // rows * S
  int nblocks, splits;  // dW kernel: 128-frame blocks, row splits
};

__device__ __forceinline__ int tile_row(int reg, int lh) { return (reg & 3) + 8 * (reg >> 2) + 4 * lh; }

// frame f (= row * S + j, row = t * B + b) -> utterance b, target y[b][tau]; counted iff tau < min(x_sl[b], T)
struct Frame {
  int b, tau;
  bool counted;
};
__device__ __forceinline__ Frame frame_of(const CatArgs& a, int f) {
  Frame fr{0, 0, false};
  if (f >= a.frames) return fr;
  const int row = f / a.S, j = f - row * a.S;
  const int t = row / a.B;
  fr.b = row - t * a.B;
  fr.tau = t * a.S + j;
  const int len = a.x_sl[fr.b];
  fr.counted = fr.tau < (len < a.T ? len : a.T);
  return fr;
}

// The 32x32 tile D[i][j] = sum_k A[i][k] Bm[j][k]; ap / bp: this lane's row of each operand plus 4 * lh.  K a multiple of 16.  Two
// 8-k chunks per trip, the next trip's four 16-byte loads issued before this trip's eight MFMAs (the last trip reloads itself).
__device__ __forceinline__ f32x16 tile_product(const float* __restrict__ ap, const float* __restrict__ bp, int K) {
  f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;
  float4 a0 = *reinterpret_cast<const float4*>(ap), a1 = *reinterpret_cast<const float4*>(ap + 8);
  float4 b0 = *reinterpret_cast<const float4*>(bp), b1 = *reinterpret_cast<const float4*>(bp + 8);
  for (int kc = 0; kc < K; kc += 16) {
    const int kn = kc + 16 < K ? kc + 16 : kc;
    const float4 na0 = *reinterpret_cast<const float4*>(ap + kn), na1 = *reinterpret_cast<const float4*>(ap + kn + 8);
    const float4 nb0 = *reinterpret_cast<const float4*>(bp + kn), nb1 = *reinterpret_cast<const float4*>(bp + kn + 8);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a0.x, b0.x, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a0.y, b0.y, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a0.z, b0.z, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a0.w, b0.w, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a1.x, b1.x, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a1.y, b1.y, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a1.z, b1.z, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a1.w, b1.w, acc, 0, 0, 0);
    a0 = na0; a1 = na1; b0 = nb0; b1 = nb1;
  }
  return acc;
}

// the biases of this lane's 16 classes of the tile at v0 (a class beyond V reads the last one: the caller masks it)
__device__ __forceinline__ void tile_bias(const float* __restrict__ bias, int V, int v0, int lh, float (&br)[16]) {
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int cls = v0 + tile_row(r, lh);
    br[r] = bias[cls < V ? cls : V - 1];
  }
}

// (m, s) <- the running maximum and sum of exp(. - m) of both operands' terms
__device__ __forceinline__ void lse_merge(float& m, float& s, float m2, float s2) {
  const float M = fmaxf(m, m2);
  if (M == -INFINITY) return;
  s = s * expf(m - M) + s2 * expf(m2 - M);
  m = M;
}

// ---- row-tile-stationary: forward (lse, ll) | backward (d_dec) ------------------------------------------------------------------
template <bool BWD>
__global__ __launch_bounds__(CAT_NW * 64) void cat_rows_kernel(CatArgs a) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  __shared__ int s_y[CAT_FT];
  __shared__ float s_g[CAT_FT], s_lse[CAT_FT];  // g * mask, lse (backward)
  __shared__ int s_cnt[CAT_FT], s_b[CAT_FT], s_tau[CAT_FT];
  const int C = a.C, V = a.V, ldx = C + 4;
  float* xs = smem;                // [32 frames][C + 4]
  float* dl = xs + CAT_FT * ldx;   // BWD: d [128 classes][32 frames]; forward: the waves' (m, s, l_y) [4][3][32]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 31, lh = lane >> 5;
  const int f0 = blockIdx.x * CAT_FT;

  if (tid < CAT_FT) {
    const Frame fr = frame_of(a, f0 + tid);
    s_cnt[tid] = fr.counted;
    s_b[tid] = fr.b;
    s_tau[tid] = fr.tau;
    s_y[tid] = fr.counted ? a.y[(size_t)fr.b * a.T + fr.tau] : -1;
    if (BWD) {
      s_g[tid] = fr.counted ? a.g[fr.b] : 0.f;
      s_lse[tid] = fr.counted ? a.lse_in[f0 + tid] : 0.f;
    }
  }
  __syncthreads();
  {  // activations of the tile; frames that do not count enter as zeros (whatever they hold, NaN included, changes nothing)
    const int c4n = C >> 2;
    for (int idx = tid; idx < CAT_FT * c4n; idx += CAT_NW * 64) {
      const int fr = idx / c4n, c4 = idx - fr * c4n;
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (s_cnt[fr]) v = *reinterpret_cast<const float4*>(a.dec + (size_t)(f0 + fr) * C + 4 * c4);
      *reinterpret_cast<float4*>(xs + fr * ldx + 4 * c4) = v;
    }
  }
  __syncthreads();

  const int ntiles = (V + CAT_CT - 1) / CAT_CT;
  const int yv = s_y[li];
  const float* xp = xs + li * ldx + 4 * lh;

  if constexpr (!BWD) {
    float m = -INFINITY, s = 0.f, ly = -INFINITY;
    for (int vt = wave; vt < ntiles; vt += CAT_NW) {
      const int v0 = vt * CAT_CT;
      const int vr = v0 + li < V ? v0 + li : V - 1;
      float br[16];
      tile_bias(a.bias, V, v0, lh, br);
      f32x16 acc = tile_product(a.W + (size_t)vr * C + 4 * lh, xp, C);
      float tm = -INFINITY;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int cls = v0 + tile_row(r, lh);
        const float l = cls < V ? acc[r] + br[r] : -INFINITY;
        acc[r] = l;
        if (cls == yv) ly = l;  // the target is found by comparison, never used as an index
        tm = fmaxf(tm, l);
      }
      if (tm > m) {
        s *= expf(m - tm);
        m = tm;
      }
      if (m > -INFINITY) {
#pragma unroll
        for (int r = 0; r < 16; ++r) s += expf(acc[r] - m);
      }
    }
    // the frame's other 16 classes per tile sit in lane li + 32 (or li - 32)
    lse_merge(m, s, __shfl_xor(m, 32), __shfl_xor(s, 32));
    ly = fmaxf(ly, __shfl_xor(ly, 32));
    if (lh == 0) {
      dl[(wave * 3 + 0) * CAT_FT + li] = m;
      dl[(wave * 3 + 1) * CAT_FT + li] = s;
      dl[(wave * 3 + 2) * CAT_FT + li] = ly;
    }
    __syncthreads();
    if (tid < CAT_FT && f0 + tid < a.frames) {
      float M = dl[tid], Ssum = dl[CAT_FT + tid], L = dl[2 * CAT_FT + tid];
      for (int w = 1; w < CAT_NW; ++w) {
        lse_merge(M, Ssum, dl[(w * 3 + 0) * CAT_FT + tid], dl[(w * 3 + 1) * CAT_FT + tid]);
        L = fmaxf(L, dl[(w * 3 + 2) * CAT_FT + tid]);
      }
      const bool counted = s_cnt[tid] != 0;
      const float lse = M + logf(Ssum);
      a.lse[f0 + tid] = counted ? lse : 0.f;
      if (s_tau[tid] < a.T) a.ll[(size_t)s_b[tid] * a.T + s_tau[tid]] = counted ? L - lse : 0.f;
    }
  } else {
    const float gm = s_g[li], lse = s_lse[li];
    const int nchunks = (C + 31) >> 5;
    f32x16 out[4];
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
      for (int r = 0; r < 16; ++r) out[q][r] = 0.f;
    const int nsuper = (ntiles + CAT_NW - 1) / CAT_NW;
    for (int st = 0; st < nsuper; ++st) {
      const int vs0 = st * CAT_SUPER;
      const int vt = st * CAT_NW + wave;
      if (vt < ntiles) {
        const int v0 = vt * CAT_CT;
        const int vr = v0 + li < V ? v0 + li : V - 1;
        float br[16];
        tile_bias(a.bias, V, v0, lh, br);
        const f32x16 acc = tile_product(a.W + (size_t)vr * C + 4 * lh, xp, C);
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int cls = v0 + tile_row(r, lh);
          float d = 0.f;
          if (cls < V && gm != 0.f) d = gm * ((cls == yv ? 1.f : 0.f) - expf(acc[r] + br[r] - lse));
          dl[(wave * CAT_CT + tile_row(r, lh)) * CAT_FT + li] = d;
        }
      }
      __syncthreads();
      // d_dec^T [channel, frame] += sum over this step's classes of W[class][channel] * d[class][frame]
      const int ncls = (ntiles - st * CAT_NW < CAT_NW ? ntiles - st * CAT_NW : CAT_NW) * CAT_CT;
      for (int kk = 0; kk < ncls; kk += 2) {
        const int cls = vs0 + kk + lh;
        const float dv = dl[(kk + lh) * CAT_FT + li];
        const float* wrow = a.W + (size_t)(cls < V ? cls : V - 1) * C;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int ch = (wave + CAT_NW * q) * 32 + li;
          if (wave + CAT_NW * q < nchunks) {  // wave-uniform
            const float wl = wrow[ch < C ? ch : C - 1];  // always in bounds: loaded without a branch, masked after
            const float wv = (ch < C && cls < V) ? wl : 0.f;
            out[q] = __builtin_amdgcn_mfma_f32_32x32x2f32(wv, dv, out[q], 0, 0, 0);
          }
        }
      }
      __syncthreads();
    }
    if (f0 + li < a.frames) {
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        if (wave + CAT_NW * q >= nchunks) continue;
#pragma unroll
        for (int gq = 0; gq < 4; ++gq) {
          const int ch = (wave + CAT_NW * q) * 32 + 8 * gq + 4 * lh;  // channels ch .. ch + 3 = registers 4 gq .. 4 gq + 3
          if (ch < C)
            *reinterpret_cast<float4*>(a.d_dec + (size_t)(f0 + li) * C + ch) =
                make_float4(out[q][4 * gq], out[q][4 * gq + 1], out[q][4 * gq + 2], out[q][4 * gq + 3]);
        }
      }
    }
  }
}

// ---- class-tile-stationary: dW, db ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(CAT_NW * 64) void cat_cls_kernel(CatArgs a) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  __shared__ int s_y[CAT_SUPER], s_cnt[CAT_SUPER];
  __shared__ float s_g[CAT_SUPER], s_lse[CAT_SUPER];
  const int C = a.C, V = a.V, ldw = C + 4;
  float* wt = smem;                // [32 classes][C + 4]
  float* dl = wt + CAT_CT * ldw;   // d [32 classes][129]; at the end the db partials [8][32]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 31, lh = lane >> 5;
  const int v0 = blockIdx.x * CAT_CT, split = blockIdx.y;
  const int blk0 = (int)((long long)a.nblocks * split / a.splits), blk1 = (int)((long long)a.nblocks * (split + 1) / a.splits);
  const bool want_w = a.dW_out != nullptr;

  {
    const int c4n = C >> 2;
    for (int idx = tid; idx < CAT_CT * c4n; idx += CAT_NW * 64) {
      const int r = idx / c4n, c4 = idx - r * c4n;
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (v0 + r < V) v = *reinterpret_cast<const float4*>(a.W + (size_t)(v0 + r) * C + 4 * c4);
      *reinterpret_cast<float4*>(wt + r * ldw + 4 * c4) = v;
    }
  }
  float bias_r[16];
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int cls = v0 + tile_row(r, lh);
    bias_r[r] = cls < V ? a.bias[cls] : 0.f;
  }
  const int nchunks = (C + 31) >> 5;
  f32x16 out[4];
#pragma unroll
  for (int q = 0; q < 4; ++q)
#pragma unroll
    for (int r = 0; r < 16; ++r) out[q][r] = 0.f;
  float dbp = 0.f;  // thread (class tid & 31, part tid >> 5): column sum of d over 16 of a block's 128 frames

  for (int blk = blk0; blk < blk1; ++blk) {
    const int f0 = blk * CAT_SUPER;
    if (tid < CAT_SUPER) {
      const Frame fr = frame_of(a, f0 + tid);
      s_cnt[tid] = fr.counted;
      s_y[tid] = fr.counted ? a.y[(size_t)fr.b * a.T + fr.tau] : -1;
      s_g[tid] = fr.counted ? a.g[fr.b] : 0.f;
      s_lse[tid] = fr.counted ? a.lse_in[f0 + tid] : 0.f;
    }
    __syncthreads();
    {  // wave w: the logits of frames f0 + 32 w .. + 31 against the 32 classes, then d
      const int fl = wave * CAT_FT + li;
      const int f = f0 + fl < a.frames ? f0 + fl : a.frames - 1;  // address only: such a frame has g = 0
      const float gm = s_g[fl], lse = s_lse[fl];
      const int yv = s_y[fl];
      const f32x16 acc = tile_product(wt + li * ldw + 4 * lh, a.dec + (size_t)f * C + 4 * lh, C);
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int cls = v0 + tile_row(r, lh);
        float d = 0.f;
        if (cls < V && gm != 0.f) d = gm * ((cls == yv ? 1.f : 0.f) - expf(acc[r] + bias_r[r] - lse));
        dl[tile_row(r, lh) * CAT_DLD + fl] = d;
      }
    }
    __syncthreads();
    {
      const int cl = tid & 31, part = tid >> 5;
#pragma unroll
      for (int i = 0; i < 16; ++i) dbp += dl[cl * CAT_DLD + part * 16 + i];
    }
    if (want_w) {
      // dW_tile [class, channel] += sum over the block's frames of d[class][frame] * X[frame][channel]
#pragma unroll 4
      for (int kk = 0; kk < CAT_SUPER; kk += 2) {
        const int fl = kk + lh;
        const float dv = dl[li * CAT_DLD + fl];
        const bool live = s_cnt[fl] != 0;  // a frame that does not count may hold anything: it enters as zero
        const float* xrow = a.dec + (size_t)(live ? f0 + fl : 0) * C;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int ch = (wave + CAT_NW * q) * 32 + li;
          if (wave + CAT_NW * q < nchunks) {
            const float xl = xrow[ch < C ? ch : C - 1];  // always in bounds: loaded without a branch, masked after
            const float xv = (live && ch < C) ? xl : 0.f;
            out[q] = __builtin_amdgcn_mfma_f32_32x32x2f32(dv, xv, out[q], 0, 0, 0);
          }
        }
      }
    }
    __syncthreads();
  }

  if (want_w) {
    float* dst = a.dW_out + (size_t)split * V * C;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int ch = (wave + CAT_NW * q) * 32 + li;
      if (wave + CAT_NW * q >= nchunks || ch >= C) continue;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int cls = v0 + tile_row(r, lh);
        if (cls < V) dst[(size_t)cls * C + ch] = out[q][r];
      }
    }
  }
  if (a.db_out != nullptr) {
    dl[(tid >> 5) * CAT_CT + (tid & 31)] = dbp;
    __syncthreads();
    if (tid < CAT_CT && v0 + tid < V) {
      float sum = 0.f;
      for (int p = 0; p < 8; ++p) sum += dl[p * CAT_CT + tid];
      a.db_out[(size_t)split * V + v0 + tid] = sum;
    }
  }
}

// out[i] = sum over the splits, in split order, of part[s * n + i]
__global__ __launch_bounds__(256) void cat_reduce_kernel(const float* __restrict__ part, size_t n, int splits, float* __restrict__ out) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  float sum = 0.f;
  for (int s = 0; s < splits; ++s) sum += part[(size_t)s * n + i];
  out[i] = sum;
}

// log_prob[b] += sum_t ll[b][t] in float64: thread-strided partial sums, then a tree over the 256 threads (a fixed order)
__global__ __launch_bounds__(256) void cat_sum_kernel(const float* __restrict__ ll, int T, double* __restrict__ log_prob) {
  __shared__ double part[256];
  const int b = blockIdx.x, tid = threadIdx.x;
  double sum = 0.0;
  for (int t = tid; t < T; t += 256) sum += (double)ll[(size_t)b * T + t];
  part[tid] = sum;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if (tid < w) part[tid] += part[tid + w];
    __syncthreads();
  }
  if (tid == 0) log_prob[b] += part[0];
}

// ---- sampler on materialised logits: thread t owns the classes [t * chunk, (t + 1) * chunk) ----------------------------------------
__global__ __launch_bounds__(256) void cat_sample_kernel(const float* __restrict__ logits, const float* __restrict__ u, int V,
                                                         int32_t* __restrict__ out) {
  __shared__ float s_val[256];
  __shared__ int s_idx[256];
  __shared__ int s_found;
  const int tid = threadIdx.x;
  const float* l = logits + (size_t)blockIdx.x * V;
  const int chunk = (V + 255) / 256;
  const int k0 = tid * chunk < V ? tid * chunk : V, k1 = k0 + chunk < V ? k0 + chunk : V;
  float best = -INFINITY;
  int arg = V;
  for (int k = k0; k < k1; ++k) {
    const float v = l[k];
    if (v > best || arg == V) {  // the first maximum of the chunk
      best = v;
      arg = k;
    }
  }
  s_val[tid] = best;
  s_idx[tid] = arg;
  if (tid == 0) s_found = V - 1;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if (tid < w) {
      const float v2 = s_val[tid + w];
      const int i2 = s_idx[tid + w];
      // the larger value; on a tie the lower index (an empty chunk has index V)
      if (i2 < V && (s_idx[tid] == V || v2 > s_val[tid] || (v2 == s_val[tid] && i2 < s_idx[tid]))) {
        s_val[tid] = v2;
        s_idx[tid] = i2;
      }
    }
    __syncthreads();
  }
  const float m = s_val[0];
  const int amax = s_idx[0];
  if (u == nullptr) {
    if (tid == 0) out[blockIdx.x] = amax;
    return;
  }
  __syncthreads();
  float part = 0.f;
  for (int k = k0; k < k1; ++k) part += expf(l[k] - m);
  s_val[tid] = part;
  __syncthreads();
  // the same chain for every thread: prefix(t + 1) = prefix(t) + part(t) exactly, total = prefix(256)
  float prefix = 0.f, total = 0.f;
  for (int t = 0; t < 256; ++t) {
    if (t == tid) prefix = total;
    total += s_val[t];
  }
  const float target = u[blockIdx.x] * total;
  float c = prefix;
  for (int k = k0; k < k1; ++k) {
    c += expf(l[k] - m);
    if (c >= target) {
      atomicMin(&s_found, k);
      break;
    }
  }
  __syncthreads();
  if (tid == 0) out[blockIdx.x] = s_found;
}

int cat_check(const char* who, const float* dec, const float* W, const float* bias, const int32_t* y, const int32_t* x_sl, int B, int T, int Tp,
              int S, int C, int V) {
  BLVM_REQUIRE(dec && W && bias && y && x_sl, "%s: null pointer", who);
  BLVM_REQUIRE(B > 0 && T > 0 && Tp > 0 && S > 0 && (long long)Tp * S >= T, "%s: B = %d, T = %d, Tp = %d, S = %d: need T <= Tp * S", who, B, T, Tp, S);
  BLVM_REQUIRE((long long)B * Tp * S < INT_MAX - CAT_SUPER && (long long)B * T < INT_MAX, "%s: more than 2^31 frames", who);
  if (C % 16 != 0 || C < 16 || C > 512 || V < 2 || V > 65536) {
    set_error("%s: C = %d, V = %d: this build takes C %% 16 == 0, 16 <= C <= 512, 2 <= V <= 65536", who, C, V);
    return BLVM_ENOSUP;
  }
  BLVM_REQUIRE(aligned16(dec) && aligned16(W), "%s: dec and W must be 16-byte aligned", who);
  return BLVM_OK;
}

CatArgs cat_args(const float* dec, const float* W, const float* bias, const int32_t* y, const int32_t* x_sl, int B, int T, int Tp, int S, int C,
                 int V) {
  CatArgs a{};
  a.dec = dec; a.W = W; a.bias = bias; a.y = y; a.x_sl = x_sl;
  a.B = B; a.T = T; a.S = S; a.C = C; a.V = V;
  a.frames = B * Tp * S;
  return a;
}

int cat_max_splits(int V) {
  const int tiles = (V + CAT_CT - 1) / CAT_CT;
  return tiles >= CAT_FILL ? 1 : (CAT_FILL + tiles - 1) / tiles;
}
int cat_splits(long long frames, int V) {
  const long long nblocks = (frames + CAT_SUPER - 1) / CAT_SUPER;
  const int ms = cat_max_splits(V);
  return (int)(nblocks < ms ? (nblocks < 1 ? 1 : nblocks) : ms);
}

template <class K>
int cat_lds(K kernel, size_t lds) {
  if (lds > 64 * 1024) BLVM_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  return BLVM_OK;
}

}  // namespace
}  // namespace blvm

extern "C" int blvm_cat_fwd(const float* dec, const float* W, const float* bias, const int32_t* y, const int32_t* x_sl, int B, int T, int Tp,
                            int S, int C, int V, float* lse, float* ll, double* log_prob, void* stream) {
  using namespace blvm;
  BLVM_TRY(cat_check("cat_fwd", dec, W, bias, y, x_sl, B, T, Tp, S, C, V));
  BLVM_REQUIRE(lse && ll, "cat_fwd: null output");
  hipStream_t s = static_cast<hipStream_t>(stream);
  CatArgs a = cat_args(dec, W, bias, y, x_sl, B, T, Tp, S, C, V);
  a.lse = lse;
  a.ll = ll;
  const size_t lds = sizeof(float) * ((size_t)CAT_FT * (C + 4) + CAT_NW * 3 * CAT_FT);
  BLVM_TRY(cat_lds(cat_rows_kernel<false>, lds));
  hipLaunchKernelGGL(cat_rows_kernel<false>, dim3((unsigned)((a.frames + CAT_FT - 1) / CAT_FT)), dim3(CAT_NW * 64), lds, s, a);
  BLVM_CHECK_LAUNCH("cat_fwd");
  if (log_prob) {
    hipLaunchKernelGGL(cat_sum_kernel, dim3(B), dim3(256), 0, s, ll, T, log_prob);
    BLVM_CHECK_LAUNCH("cat_fwd (sums)");
  }
  return BLVM_OK;
}

extern "C" size_t blvm_cat_bwd_workspace_floats(long long frames, int C, int V) {
  if (frames < 1 || C < 1 || V < 1) return 0;
  const int splits = blvm::cat_splits(frames, V);
  return splits > 1 ? (size_t)splits * V * ((size_t)C + 1) : 0;
}

extern "C" int blvm_cat_bwd(const float* dec, const float* W, const float* bias, const int32_t* y, const int32_t* x_sl, const float* lse,
                            const float* g_b, int B, int T, int Tp, int S, int C, int V, float* d_dec, float* dW, float* db,
                            float* workspace, void* stream) {
  using namespace blvm;
  BLVM_TRY(cat_check("cat_bwd", dec, W, bias, y, x_sl, B, T, Tp, S, C, V));
  BLVM_REQUIRE(lse && g_b, "cat_bwd: null pointer");
  BLVM_REQUIRE((!d_dec || aligned16(d_dec)) && (!dW || aligned16(dW)), "cat_bwd: d_dec and dW must be 16-byte aligned");
  hipStream_t s = static_cast<hipStream_t>(stream);
  CatArgs a = cat_args(dec, W, bias, y, x_sl, B, T, Tp, S, C, V);
  a.lse_in = lse;
  a.g = g_b;
  a.nblocks = (a.frames + CAT_SUPER - 1) / CAT_SUPER;
  a.splits = cat_splits(a.frames, V);
  BLVM_REQUIRE(a.splits == 1 || workspace || (!dW && !db), "cat_bwd: dW / db need the workspace (blvm_cat_bwd_workspace_floats)");
  if (d_dec) {
    a.d_dec = d_dec;
    const size_t lds = sizeof(float) * ((size_t)CAT_FT * (C + 4) + CAT_SUPER * CAT_FT);
    BLVM_TRY(cat_lds(cat_rows_kernel<true>, lds));
    hipLaunchKernelGGL(cat_rows_kernel<true>, dim3((unsigned)((a.frames + CAT_FT - 1) / CAT_FT)), dim3(CAT_NW * 64), lds, s, a);
    BLVM_CHECK_LAUNCH("cat_bwd (d_dec)");
  }
  if (dW || db) {
    const bool direct = a.splits == 1;
    float* ws_w = workspace;
    float* ws_b = workspace ? workspace + (size_t)a.splits * V * C : nullptr;
    a.dW_out = dW ? (direct ? dW : ws_w) : nullptr;
    a.db_out = db ? (direct ? db : ws_b) : nullptr;
    const int tiles = (V + CAT_CT - 1) / CAT_CT;
    const size_t lds = sizeof(float) * ((size_t)CAT_CT * (C + 4) + CAT_CT * CAT_DLD);
    BLVM_TRY(cat_lds(cat_cls_kernel, lds));
    hipLaunchKernelGGL(cat_cls_kernel, dim3((unsigned)tiles, (unsigned)a.splits), dim3(CAT_NW * 64), lds, s, a);
    BLVM_CHECK_LAUNCH("cat_bwd (dW, db)");
    if (!direct) {
      if (dW) {
        const size_t n = (size_t)V * C;
        hipLaunchKernelGGL(cat_reduce_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, ws_w, n, a.splits, dW);
      }
      if (db) hipLaunchKernelGGL(cat_reduce_kernel, dim3((unsigned)((V + 255) / 256)), dim3(256), 0, s, ws_b, (size_t)V, a.splits, db);
      BLVM_CHECK_LAUNCH("cat_bwd (reduce)");
    }
  }
  return BLVM_OK;
}

extern "C" int blvm_cat_sample(const float* logits, const float* u, long long n, int V, int32_t* out, void* stream) {
  using namespace blvm;
  BLVM_REQUIRE(logits && out && n >= 0 && n < INT_MAX, "cat_sample: bad arguments");
  if (V < 2 || V > 65536) {
    set_error("cat_sample: V = %d: this build takes 2 <= V <= 65536", V);
    return BLVM_ENOSUP;
  }
  if (n == 0) return BLVM_OK;
  hipLaunchKernelGGL(cat_sample_kernel, dim3((unsigned)n), dim3(256), 0, static_cast<hipStream_t>(stream), logits, u, V, out);
  BLVM_CHECK_LAUNCH("cat_sample");
  return BLVM_OK;
}
