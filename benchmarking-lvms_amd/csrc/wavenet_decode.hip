// wavenet_decode.hip — K10c: autoregressive WaveNet sampling, every frame of every utterance in ONE launch.
//
// Replaces the per-frame loop of WaveNet.generate (blvm/models/wavenet/wavenet.py:254-293).  The reference re-runs the
// causal convolution and all residual blocks over a receptive-field window for each new sample; its TODO names the cached
// formulation (arXiv:1611.09482), which this kernel is: block i keeps a ring buffer of its own input over the last
// `dilation_i` frames, so one new frame costs one [2C]x[2C] and one [C+S]x[C] product per block.
//
// Decoding is a chain of ~2 * n_blocks dependent small products per frame — pure latency.  One workgroup owns 16
// utterances (the M dimension of v_mfma_f32_16x16x4_f32) and walks the whole network for them with all activations in
// LDS; the only global traffic is the weights (which stay L2 / Infinity-Cache resident across frames, the kernel is never
// left), one ring-buffer row per block, the two uniform draws and the sample.  No launch, no host, no inter-workgroup
// synchronisation inside the loop.
//
// A window of zeros is an all-zero past; under it every block input is constant in time (the network's response to zero
// input, biases included).  The prologue evaluates that steady state once — each block with both taps on the same vector —
// and fills the ring buffers with it, which makes frame 0 identical to the reference's first window evaluation.
//
// The any-width block, the tile layers and the draw are the ones K10d (stcn_decode.hip) uses: decode_tiles.h.  The compile-time-
// width path below (block_fast) is this kernel's own.
//
// Heads (a template parameter, so each keeps its own code): the Gaussian-mixture and Gaussian heads (the DMoL head's padded 32 head
// rows; mix_pick then gauss_draw, or gauss_draw on (mu, raw); unclamped), the DMoL head (3 * num_mix <= 32 outputs, Gumbel-max + logistic
// draw) and the categorical head of the original paper (K7d's softmax over V classes, 16 <= V <= 1024): its Linear goes through the
// same tile layer into an LDS logits buffer [16][V + 4], 32 lanes per row draw one class (cat_pick, decode_tiles.h), and the class
// is fed back and written out as levels[k] — the model's table, copied to LDS once; no arithmetic on it.
// On an embedded model (K10e, wavenet_embed.hip) the categorical head feeds the class back as a CLASS: sX holds the two newest classes
// and the front reads two rows of the lookup tables from global memory; a third HEAD, so the arms above keep their code.
#include "common.h"
#include "decode_tiles.h"

namespace blvm {
namespace {

constexpr int DEC_ROWS = 16;        // utterances per workgroup
constexpr int DEC_MAX_BLOCKS = 64;  // dilations travel by value in the kernel arguments
constexpr int DEC_HEAD_ROWS = 32;   // head weight rows in the packed image (3 * num_mix <= 30, zero padded)

// Offsets (floats) into the packed weight image; every region starts on a 16-byte boundary (C, S, O multiples of 16).
struct DecodeLayout {
  size_t causal_w, causal_b, in_w, in_b, blocks, block_stride, out_w, out_b, head_w, head_b, total;
  size_t conv_b, rs_w, rs_b;  // relative to a block's start (conv_w is at 0)
};

__host__ __device__ inline DecodeLayout decode_layout(int C, int S, int O, int n_blocks, int head_rows = DEC_HEAD_ROWS) {
  DecodeLayout L;
  size_t o = 0;
  L.causal_w = o; o += (size_t)C * 2;  // [C,1,2]
  L.causal_b = o; o += C;
  L.in_w = o; o += (size_t)C * C;
  L.in_b = o; o += C;
  L.conv_b = (size_t)2 * C * 2 * C;
  L.rs_w = L.conv_b + 2 * C;
  L.rs_b = L.rs_w + (size_t)(C + S) * C;
  L.block_stride = L.rs_b + (C + S);
  L.blocks = o; o += L.block_stride * n_blocks;
  L.out_w = o; o += (size_t)O * S;
  L.out_b = o; o += O;
  L.head_w = o; o += (size_t)head_rows * O;
  L.head_b = o; o += head_rows;
  L.total = o;
  return L;
}

struct DecodeArgs {
  const float* w;
  const float* wt;  // T16 operand copies (common.h) of the blocks' matrices: block i at i * ((2C)^2 + (C+S) C): conv [2C,2C], rs [C+S,C]
  int dil[DEC_MAX_BLOCKS];
  int n_blocks, B, C, S, O, n_frames, num_mix;
  float inv_std, skip_scale, log_eps;
  const float* u;  // [n_frames,B,num_mix] or NULL
  const float* v;  // [n_frames,B] or NULL
  float* queues;   // block i: [dil_i,B,C] at B*C*sum(dil[:i])
  float* x_out;    // [B,n_frames]
  // entry from a given state (RESUME): the rings hold every block's input over absolute frames t0 - dil_i .. t0 - 1
  int t0;             // absolute index of this call's frame 0; frame tau lives in slot tau mod dil_i
  const float* x_in;  // [B,2] (previous, newest) sample in front of frame t0
  float* x_state;     // [B,2] the same pair after the last frame
};

// The categorical head: u is [n_frames,B] (one draw per frame and row, NULL: the arg-max class); num_mix, log_eps and v are unused.
struct CatDecodeArgs : DecodeArgs {
  int V;                // classes: the head Linear is [V,O] in the packed image
  const float* levels;  // [V] the value of class k, fed back and written to x_out as it stands
  int* k_out;           // [B,n_frames] the classes, or NULL
};

// The embedded model: x_in / x_state hold int32 classes; the zero start is a past of class 0.
struct EmbCatDecodeArgs : CatDecodeArgs {
  const float* tab;  // [2,V+1,C] the lookup tables of wavenet_embed.hip
};

// The Gaussian heads: v is [n_frames,B] standard normals (NULL: the mean); the mixture keeps u and num_mix, the plain Gaussian
// head's two outputs are (mu, raw) and u is unused.  log_eps is unused.
struct GaussDecodeArgs : DecodeArgs {
  float sd_beta, sd_eps;  // sd = softplus_beta(raw) + sd_eps
};

// `gauss`: 0 none, 1 the Gaussian mixture (the DMoL head's layout and pick, gauss_draw), 2 the plain Gaussian (mu, raw)
struct DmolHead {
  using Args = DecodeArgs;
  static constexpr bool categorical = false, embedded = false;
  static constexpr int gauss = 0;
};
struct CatHead {
  using Args = CatDecodeArgs;
  static constexpr bool categorical = true, embedded = false;
  static constexpr int gauss = 0;
};
struct EmbCatHead {
  using Args = EmbCatDecodeArgs;
  static constexpr bool categorical = true, embedded = true;
  static constexpr int gauss = 0;
};
struct GmmHead {
  using Args = GaussDecodeArgs;
  static constexpr bool categorical = false, embedded = false;
  static constexpr int gauss = 1;
};
struct GaussHead {
  using Args = GaussDecodeArgs;
  static constexpr bool categorical = false, embedded = false;
  static constexpr int gauss = 2;
};
constexpr int CAT_MIN_V = 16, CAT_MAX_V = 1024, CAT_LOGIT_PAD = 4;

// LDS-only barrier: waits for this wave's LDS traffic, not for its global loads.  No thread of the decoder ever reads
// global memory another thread wrote (ring-buffer elements are read and rewritten by the same thread, weights and draws are
// read-only), so weight / ring-buffer loads issued for the NEXT block stay in flight across it.
__device__ __forceinline__ void lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

// 16x16 output tile from an LDS operand and weights already in registers: wreg[j] holds W[col][16 j + 4 q .. +3]
template <int KCH>
__device__ __forceinline__ f32x4 tile_from_regs(const float* __restrict__ A, int lda, const float4 (&wreg)[KCH]) {
  const int lane = threadIdx.x & 63;
  const float* ap = A + (lane & 15) * lda + 4 * (lane >> 4);
  f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int j = 0; j < KCH; ++j) {
    const float4 x = *reinterpret_cast<const float4*>(ap + 16 * j);
    f32x4& acc = (j & 1) ? acc1 : acc0;
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(x.x, wreg[j].x, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(x.y, wreg[j].y, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(x.z, wreg[j].z, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(x.w, wreg[j].w, acc, 0, 0, 0);
  }
  return acc0 + acc1;
}

// CC, SS > 0: widths known at compile time — the main loop keeps each wave's weight tiles, biases and ring-buffer taps of
// the NEXT block in registers, loaded while the current block computes.  CC == 0: any width, loads where they are used.
// RESUME: no steady-state prologue — rings and the last two samples are the caller's, frame t is absolute frame t0 + t, and
// the sample pair is handed back; with the rings left in scratch that is the whole state.  A separate instantiation, so the
// zero-start entry keeps its code.  HEAD: one of the head types above, separate instantiations for the same reason.
template <int NW, int CC, int SS, bool RESUME, class HEAD>
__global__ __launch_bounds__(NW * 64) void wn_decode_kernel(typename HEAD::Args a) {
  extern __shared__ __align__(16) float smem[];
  constexpr int NT = NW * 64;
  const int C = CC > 0 ? CC : a.C, S = SS > 0 ? SS : a.S, O = a.O, B = a.B;
  const int CA = C > O ? C : O;
  const int ldV = 2 * C + 4, ldA = CA + 4, ldS = S + 4, ldP = 2 * C;
  float* sV = smem;                    // [16][2C+4]  interleaved taps: k = 2c + tap
  float* sPre = sV + DEC_ROWS * ldV;   // [16][2C]    gate pre-activations
  float* sAct = sPre + DEC_ROWS * ldP; // [16][max(C,O)+4]
  float* sH = sAct + DEC_ROWS * ldA;   // [16][C]     current block input
  float* sSkip = sH + DEC_ROWS * C;    // [16][S+4]
  const int head_rows = [&] {
    if constexpr (HEAD::categorical) return a.V;
    else return DEC_HEAD_ROWS;
  }();
  const int ldL = HEAD::categorical ? head_rows + CAT_LOGIT_PAD : DEC_HEAD_ROWS;
  float* sPar = sSkip + DEC_ROWS * ldS;  // [16][32]  head outputs; categorical: [16][V+4] the logits
  float* sX = sPar + DEC_ROWS * ldL;     // [16][2] previous / newest sample
  [[maybe_unused]] float* sLev = sX + DEC_ROWS * 2;  // categorical: [V] the class values

  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, q = lane >> 4, cc = lane & 15;
  const int b0 = blockIdx.x * DEC_ROWS;
  const DecodeLayout L = decode_layout(C, S, O, a.n_blocks, head_rows);
  const float* w = a.w;

  const int t0 = RESUME ? a.t0 : 0;
  [[maybe_unused]] int* sK = reinterpret_cast<int*>(sX);  // embedded: the pair as classes
  if constexpr (HEAD::embedded) {
    const int* k_in = reinterpret_cast<const int*>(a.x_in);
    for (int i = tid; i < DEC_ROWS * 2; i += NT) sK[i] = (RESUME && b0 + i / 2 < B) ? min(max(k_in[(size_t)2 * b0 + i], 0), a.V - 1) : 0;
  } else {
    for (int i = tid; i < DEC_ROWS * 2; i += NT) sX[i] = (RESUME && b0 + i / 2 < B) ? a.x_in[(size_t)2 * b0 + i] : 0.f;
  }
  if constexpr (HEAD::categorical)
    for (int i = tid; i < head_rows; i += NT) sLev[i] = a.levels[i];
  __syncthreads();

  // causal conv on (previous, newest) sample -> 1x1 in_transform -> sH; clears the skip accumulators
  auto front = [&]() {
    const float* cw = w + L.causal_w;
    const float* cb = w + L.causal_b;
    if constexpr (HEAD::embedded) {
      const float* p0 = a.tab;
      const float* p1 = a.tab + (size_t)(a.V + 1) * C;
      for (int idx = tid; idx < DEC_ROWS * C; idx += NT) {
        const int r = idx / C, o = idx - r * C;
        sAct[r * ldA + o] = (p0[(size_t)sK[2 * r] * C + o] + p1[(size_t)sK[2 * r + 1] * C + o]) + cb[o];
      }
    } else {
      for (int idx = tid; idx < DEC_ROWS * C; idx += NT) {
        const int r = idx / C, o = idx - r * C;
        sAct[r * ldA + o] = cw[2 * o] * sX[2 * r] + cw[2 * o + 1] * sX[2 * r + 1] + cb[o];
      }
    }
    for (int idx = tid; idx < DEC_ROWS * S; idx += NT) {
      const int r = idx / S;
      sSkip[r * ldS + (idx - r * S)] = 0.f;
    }
    __syncthreads();
    tile_layer<NW, false>(sAct, ldA, w + L.in_w, C, 0, C / 16, w + L.in_b, [&](int row, int o, float val) { sH[row * C + o] = val; });
    __syncthreads();
  };

  // one gated residual block (decode_tiles.h) on the frame in sH; the skip half is added into sSkip.  steady: both taps = sH,
  // ring buffer filled with sH, skip untouched.
  const size_t wt_stride = (size_t)2 * C * 2 * C + (size_t)(C + S) * C;
  const GateLds gl = {sH, C, sV, ldV, sPre, ldP, sAct, ldA};
  auto block = [&](int i, float* qi, int slot, bool steady) {
    const float* bw = w + L.blocks + (size_t)i * L.block_stride;
    const float* bt = a.wt + (size_t)i * wt_stride;
    gated_ring_block<NW>(gl, C, bt, bw + L.conv_b, bt + (size_t)2 * C * 2 * C, bw + L.rs_b, qi, a.dil[i], slot, steady, b0, B, a.inv_std, 0,
                         (steady ? C : C + S) / 16, [&](int row, int j, float val) { sSkip[row * ldS + j] += val; });
  };

  // steady state under an all-zero past
  if constexpr (!RESUME) {
    front();
    float* qi = a.queues;
    for (int i = 0; i < a.n_blocks; ++i) {
      block(i, qi, 0, true);
      qi += (size_t)a.dil[i] * B * C;
    }
  }

  // ---- register-resident prefetch state of the compile-time-width path
  constexpr int C_ = CC > 0 ? CC : 16, S_ = SS > 0 ? SS : 16;
  constexpr int NT1 = 2 * C_ / 16, T1 = (NT1 + NW - 1) / NW, K1 = 2 * C_ / 16;  // conv: tiles, tiles per wave, k chunks
  constexpr int NT2 = (C_ + S_) / 16, T2 = (NT2 + NW - 1) / NW, K2 = C_ / 16;   // rs
  constexpr int NQ = (DEC_ROWS * C_ + NT - 1) / NT;                             // ring-buffer elements per thread
  struct BlockRegs {
    float4 wc[T1][K1], wr[T2][K2];
    float bc[T1], br[T2], oldv[NQ];
  };
  BlockRegs R0, R1;  // ping-pong: one block computes from one set while the next block's operands land in the other
  auto load_block = [&](BlockRegs& R, int i, const float* qi, int slot) {
    const float* bw = w + L.blocks + (size_t)i * L.block_stride;
    const float* bt = a.wt + (size_t)i * wt_stride;
#pragma unroll
    for (int n = 0; n < NQ; ++n) {
      const int idx = tid + n * NT;
      const int r = idx / C_, c = idx - r * C_;
      R.oldv[n] = (idx < DEC_ROWS * C_ && b0 + r < B) ? qi[((size_t)slot * B + b0 + r) * C_ + c] : 0.f;
    }
#pragma unroll
    for (int tt = 0; tt < T1; ++tt) {
      const int tile = wave + tt * NW;
      if (tile < NT1) {
        const float* wp = bt + (size_t)(tile * 16) * (2 * C_) + 4 * lane;  // T16: chunk j of the tile is one contiguous 1 KB
#pragma unroll
        for (int j = 0; j < K1; ++j) R.wc[tt][j] = *reinterpret_cast<const float4*>(wp + 256 * j);
        R.bc[tt] = bw[L.conv_b + tile * 16 + cc];
      }
    }
#pragma unroll
    for (int tt = 0; tt < T2; ++tt) {
      const int tile = wave + tt * NW;
      if (tile < NT2) {
        const float* wp = bt + (size_t)2 * C_ * 2 * C_ + (size_t)(tile * 16) * C_ + 4 * lane;
#pragma unroll
        for (int j = 0; j < K2; ++j) R.wr[tt][j] = *reinterpret_cast<const float4*>(wp + 256 * j);
        R.br[tt] = bw[L.rs_b + tile * 16 + cc];
      }
    }
  };
#ifdef DEC_PROF
  long long prof[6] = {0, 0, 0, 0, 0, 0};
#define DEC_TICK(k) { const long long now__ = __builtin_readcyclecounter(); prof[k] += now__ - tick__; tick__ = now__; }
#else
#define DEC_TICK(k)
#endif
  // the block of the main loop: operands in `cur` (loaded one block ago); issues every load of the next block
  // (ni, nqi, nslot) into `nxt` right after staging — a whole block ahead of their first use
  auto block_fast = [&](BlockRegs& cur, BlockRegs& nxt, float* qi, int slot, int ni, const float* nqi, int nslot) {
#ifdef DEC_PROF
    long long tick__ = __builtin_readcyclecounter();
#endif
#pragma unroll
    for (int n = 0; n < NQ; ++n) {
      const int idx = tid + n * NT;
      if (idx < DEC_ROWS * C_) {
        const int r = idx / C_, c = idx - r * C_;
        *reinterpret_cast<float2*>(sV + r * ldV + 2 * c) = make_float2(cur.oldv[n], sH[idx]);
      }
    }
    // vmcnt counts loads and stores in order: the ring-buffer store goes out AFTER the last use of a loaded tap, or the
    // wait for the tap would also wait for the store's acknowledgement
    asm volatile("" ::: "memory");
#pragma unroll
    for (int n = 0; n < NQ; ++n) {
      const int idx = tid + n * NT;
      const int r = idx / C_, c = idx - r * C_;
      if (idx < DEC_ROWS * C_ && b0 + r < B) qi[((size_t)slot * B + b0 + r) * C_ + c] = sH[idx];
    }
    load_block(nxt, ni, nqi, nslot);
    DEC_TICK(0)
    lds_barrier();
    DEC_TICK(1)
#pragma unroll
    for (int tt = 0; tt < T1; ++tt) {
      const int tile = wave + tt * NW;
      if (tile < NT1) {
        const f32x4 acc = tile_from_regs<K1>(sV, ldV, cur.wc[tt]);
        const int o = tile * 16 + cc;
#pragma unroll
        for (int r = 0; r < 4; ++r) sPre[(4 * q + r) * ldP + o] = acc[r] + cur.bc[tt];
      }
    }
    DEC_TICK(2)
    lds_barrier();
    DEC_TICK(1)
    for (int idx = tid; idx < DEC_ROWS * C_; idx += NT) {
      const int r = idx / C_, c = idx - r * C_;
      sAct[r * ldA + c] = tanhf(sPre[r * ldP + c]) * sigmoidf_(sPre[r * ldP + C_ + c]);
    }
    DEC_TICK(3)
    lds_barrier();
    DEC_TICK(1)
#pragma unroll
    for (int tt = 0; tt < T2; ++tt) {
      const int tile = wave + tt * NW;
      if (tile < NT2) {
        const f32x4 acc = tile_from_regs<K2>(sAct, ldA, cur.wr[tt]);
        const int o = tile * 16 + cc;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int row = 4 * q + r;
          const float val = acc[r] + cur.br[tt];
          if (o < C_) sH[row * C_ + o] = (val + sH[row * C_ + o]) * a.inv_std;
          else sSkip[row * ldS + (o - C_)] += val;
        }
      }
    }
    DEC_TICK(4)
    lds_barrier();
    DEC_TICK(1)
  };
  if constexpr (CC > 0) load_block(R0, 0, a.queues, t0 % a.dil[0]);

  for (int t = 0; t < a.n_frames; ++t) {
    front();
    float* qi = a.queues;
    if constexpr (CC > 0) {
      // two blocks per trip (n_blocks is even on this path): the register sets swap roles by position in the code, not by
      // a run-time choice the compiler would turn into register copies behind a full vmcnt wait
      for (int i = 0; i < a.n_blocks; i += 2) {
        const int d0 = a.dil[i], d1 = a.dil[i + 1];
        float* q1 = qi + (size_t)d0 * B * C;
        float* q2 = q1 + (size_t)d1 * B * C;
        const bool last = i + 2 == a.n_blocks;
        const int ni = last ? 0 : i + 2;
        block_fast(R0, R1, qi, (t0 + t) % d0, i + 1, q1, (t0 + t) % d1);
        block_fast(R1, R0, q1, (t0 + t) % d1, ni, last ? a.queues : q2, (last ? t0 + t + 1 : t0 + t) % a.dil[ni]);
        qi = q2;
      }
    } else {
      for (int i = 0; i < a.n_blocks; ++i) {
        block(i, qi, (t0 + t) % a.dil[i], false);
        qi += (size_t)a.dil[i] * B * C;
      }
    }
    // relu(skip * scale) -> Linear -> relu -> head Linear -> sample
    for (int idx = tid; idx < DEC_ROWS * S; idx += NT) {
      const int r = idx / S, c = idx - r * S;
      sSkip[r * ldS + c] = fmaxf(sSkip[r * ldS + c] * a.skip_scale, 0.f);
    }
    __syncthreads();
    tile_layer<NW, false>(sSkip, ldS, w + L.out_w, S, 0, O / 16, w + L.out_b, [&](int row, int o, float val) { sAct[row * ldA + o] = fmaxf(val, 0.f); });
    __syncthreads();
    if constexpr (HEAD::categorical) {
      // logits -> one class per row, drawn by the row's 32 lanes (rows >= B draw too, from finite logits, and write nothing)
      constexpr int LANES = NT / DEC_ROWS;
      static_assert(LANES == 32, "the categorical draw gives each of the 16 rows half a wave");
      const int row = tid / LANES;
      const bool live = b0 + row < B, noisy = a.u != nullptr;
      const float u = (noisy && live) ? a.u[(size_t)t * B + b0 + row] : 0.f;  // issued ahead of the head's product
      tile_layer<NW, false>(sAct, ldA, w + L.head_w, O, 0, head_rows / 16, w + L.head_b, [&](int r, int o, float val) { sPar[r * ldL + o] = val; });
      __syncthreads();
      const int k = cat_pick<LANES>(sPar + row * ldL, head_rows, noisy, u);
      if ((tid & (LANES - 1)) == 0 && live) {
        const float x = sLev[k];
        a.x_out[(size_t)(b0 + row) * a.n_frames + t] = x;
        if (a.k_out != nullptr) a.k_out[(size_t)(b0 + row) * a.n_frames + t] = k;
        if constexpr (HEAD::embedded) {
          sK[2 * row] = sK[2 * row + 1];
          sK[2 * row + 1] = k;
        } else {
          sX[2 * row] = sX[2 * row + 1];
          sX[2 * row + 1] = x;
        }
      }
    } else {
      tile_layer<NW, false>(sAct, ldA, w + L.head_w, O, 0, DEC_HEAD_ROWS / 16, w + L.head_b, [&](int row, int o, float val) { sPar[row * DEC_HEAD_ROWS + o] = val; });
      __syncthreads();
      if (tid < DEC_ROWS && b0 + tid < B) {
        const float* p = sPar + tid * DEC_HEAD_ROWS;
        const size_t f = (size_t)t * B + b0 + tid;
        float x;
        if constexpr (HEAD::gauss == 2) {
          // (mu, raw): the unclamped Gaussian draw (decode_tiles.h); no n: the mean
          x = p[0];
          if (a.v != nullptr) x = gauss_draw(x, p[1], a.v[f], a.sd_beta, a.sd_eps);
        } else if constexpr (HEAD::gauss == 1) {
          // Gumbel-max component pick + the component's unclamped Gaussian draw; no u, no n: the arg-max component's mean
          const int K = a.num_mix;
          const int best = mix_pick(p, K, a.u != nullptr ? a.u + f * K : nullptr);
          x = p[K + best];
          if (a.v != nullptr) x = gauss_draw(x, p[2 * K + best], a.v[f], a.sd_beta, a.sd_eps);
        } else {
          // Gumbel-max component pick + clamped logistic draw (decode_tiles.h)
          const int K = a.num_mix;
          const int best = mix_pick(p, K, a.u != nullptr ? a.u + f * K : nullptr);
          x = p[K + best];
          if (a.v != nullptr) x = logistic_draw(x, p[2 * K + best], a.v[f], a.log_eps);
        }
        a.x_out[(size_t)(b0 + tid) * a.n_frames + t] = x;
        sX[2 * tid] = sX[2 * tid + 1];
        sX[2 * tid + 1] = x;
      }
    }
    __syncthreads();
  }
  if constexpr (RESUME)
    for (int i = tid; i < DEC_ROWS * 2; i += NT)
      if (b0 + i / 2 < B) {
        if constexpr (HEAD::embedded) reinterpret_cast<int*>(a.x_state)[(size_t)2 * b0 + i] = sK[i];
        else a.x_state[(size_t)2 * b0 + i] = sX[i];
      }
#ifdef DEC_PROF
  if (blockIdx.x == 0 && (tid == 0 || tid == NT - 1))
    for (int k = 0; k < 6; ++k) a.x_out[(size_t)B * a.n_frames + (tid ? 6 : 0) + k] = (float)(prof[k] / 1000);
#endif
}

// Ring fill for the entry from a state: src = the last d frames [d, B*C/4] (float4) of a block's time-major input, whose frame
// j is absolute frame t0 - d + j; it goes to slot (t0 - d + j) mod d = (first + j) mod d.  One float4 per thread, both sides
// contiguous in B*C.
__global__ __launch_bounds__(256) void wn_ring_fill_kernel(const float4* __restrict__ src, float4* __restrict__ ring, unsigned row4,
                                                           unsigned d, unsigned first, unsigned n4) {
  const unsigned idx = blockIdx.x * 256u + threadIdx.x;
  if (idx >= n4) return;
  const unsigned j = idx / row4, e = idx - j * row4;
  unsigned slot = first + j;
  if (slot >= d) slot -= d;
  ring[(size_t)slot * row4 + e] = src[idx];
}

// V == 0: the DMoL head; else the categorical head's logits [16][V+4] in place of the 32 head outputs, and its V class values
inline size_t decode_lds_bytes(int C, int S, int O, int V) {
  const int CA = C > O ? C : O;
  const size_t head = V > 0 ? (size_t)DEC_ROWS * (V + CAT_LOGIT_PAD) + V : (size_t)DEC_ROWS * DEC_HEAD_ROWS;
  return sizeof(float) * ((size_t)DEC_ROWS * ((2 * C + 4) + 2 * C + (CA + 4) + C + (S + 4)) + head + 2 * DEC_ROWS);
}

template <class HEAD>
int decode_launch(bool resume, bool even, const typename HEAD::Args& a, size_t lds, hipStream_t stream) {
  constexpr int NW = 8;
  auto kern = resume ? wn_decode_kernel<NW, 0, 0, true, HEAD> : wn_decode_kernel<NW, 0, 0, false, HEAD>;
  if (even && a.C == 64 && a.S == 64) kern = resume ? wn_decode_kernel<NW, 64, 64, true, HEAD> : wn_decode_kernel<NW, 64, 64, false, HEAD>;
  else if (even && a.C == 32 && a.S == 32) kern = resume ? wn_decode_kernel<NW, 32, 32, true, HEAD> : wn_decode_kernel<NW, 32, 32, false, HEAD>;
  if (lds > 64 * 1024) BLVM_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  hipLaunchKernelGGL(kern, dim3((unsigned)((a.B + DEC_ROWS - 1) / DEC_ROWS)), dim3(NW * 64), lds, stream, a);
  BLVM_CHECK_LAUNCH("wavenet_decode");
  return BLVM_OK;
}

}  // namespace
}  // namespace blvm

extern "C" size_t blvm_wavenet_decode_pack_floats(int C, int S, int O, int n_blocks) {
  if (C <= 0 || S <= 0 || O <= 0 || n_blocks <= 0) return 0;
  return blvm::decode_layout(C, S, O, n_blocks).total;
}

extern "C" size_t blvm_wavenet_decode_scratch_floats(const int* dilations, int n_blocks, int B, int C, int S) {
  if (!dilations || n_blocks <= 0 || B <= 0 || C <= 0 || S <= 0) return 0;
  return blvm::ring_floats(dilations, n_blocks, B, C) + (size_t)n_blocks * ((size_t)2 * C * 2 * C + (size_t)(C + S) * C);
}

extern "C" size_t blvm_wavenet_decode_ring_offset_floats(int n_blocks, int C, int S) {
  if (n_blocks <= 0 || C <= 0 || S <= 0) return 0;
  return (size_t)n_blocks * ((size_t)2 * C * 2 * C + (size_t)(C + S) * C);
}

// resume: the kernel starts from the rings in `scratch` and x_in at absolute frame t0 and hands the sample pair back.
// V > 0: the categorical head (levels [V], u [n_frames,B], k_out or NULL; num_mix, log_eps and v unused), V == 0: the DMoL head.
static int decode_run(bool resume, const float* packed, const int* dilations, int n_blocks, int B, int C, int S, int O, int num_mix,
                      int n_frames, int t0, float inv_std, float skip_scale, float log_eps, const float* u, const float* v,
                      const float* x_in, float* scratch, float* x_out, float* x_state, void* stream, int V = 0,
                      const float* levels = nullptr, int32_t* k_out = nullptr, const float* tables = nullptr, int gauss = 0,
                      float sd_beta = 0.f, float sd_eps = 0.f) {
  using namespace blvm;
  const bool cat = V > 0;
  BLVM_REQUIRE(packed && dilations && scratch && x_out && aligned16(packed) && aligned16(scratch), "wavenet_decode: NULL or misaligned argument");
  BLVM_REQUIRE(B > 0 && n_frames >= 0 && n_blocks > 0 && n_blocks <= DEC_MAX_BLOCKS, "wavenet_decode: need B > 0, 1 <= n_blocks <= %d", DEC_MAX_BLOCKS);
  BLVM_REQUIRE(C > 0 && S > 0 && O > 0 && C % 16 == 0 && S % 16 == 0 && O % 16 == 0, "wavenet_decode: C, S, O must be multiples of 16");
  if (cat) {
    BLVM_REQUIRE(levels, "wavenet_cat_decode: NULL levels");
  } else if (gauss == 2) {
    BLVM_REQUIRE(u == nullptr, "wavenet_gauss_decode: the Gaussian head (head_kind 2) takes no component draws u");
  } else {
    BLVM_REQUIRE(num_mix > 0 && 3 * num_mix <= DEC_HEAD_ROWS, "wavenet_decode: num_mix must be in [1, %d] (got %d)", DEC_HEAD_ROWS / 3, num_mix);
    BLVM_REQUIRE((u == nullptr) == (v == nullptr), "wavenet_decode: u and v are given together (both NULL: the mode)");
  }
  if (gauss) BLVM_REQUIRE(sd_beta > 0.f && sd_eps >= 0.f, "wavenet_gauss_decode: need sd_beta > 0, sd_eps >= 0");
  if (resume) BLVM_TRY(check_resume("wavenet_decode_resume", "sample", "n_frames", t0, n_frames, x_in, x_state));
  const size_t lds = decode_lds_bytes(C, S, O, V);
  if (cat) BLVM_REQUIRE(lds <= 160 * 1024, "wavenet_cat_decode: C=%d, S=%d, O=%d, V=%d need %zu bytes of LDS (> 160 KB)", C, S, O, V, lds);
  BLVM_REQUIRE(lds <= 160 * 1024, "wavenet_decode: C=%d, S=%d, O=%d need %zu bytes of LDS (> 160 KB)", C, S, O, lds);
  if (n_frames == 0) return resume ? hand_back_state(x_state, x_in, (size_t)2 * B, static_cast<hipStream_t>(stream)) : BLVM_OK;
  EmbCatDecodeArgs a;  // (the other kernels take its bases)
  a.V = V; a.levels = levels; a.k_out = k_out; a.tab = tables;
  a.w = packed;
  for (int i = 0; i < n_blocks; ++i) {
    BLVM_REQUIRE(dilations[i] >= 1, "wavenet_decode: dilation %d of block %d", dilations[i], i);
    a.dil[i] = dilations[i];
  }
  for (int i = n_blocks; i < DEC_MAX_BLOCKS; ++i) a.dil[i] = 1;
  a.n_blocks = n_blocks; a.B = B; a.C = C; a.S = S; a.O = O; a.n_frames = n_frames; a.num_mix = num_mix;
  a.inv_std = inv_std; a.skip_scale = skip_scale; a.log_eps = log_eps;
  a.u = u; a.v = v; a.x_out = x_out;
  a.t0 = t0; a.x_in = x_in; a.x_state = x_state;
  // scratch = [T16 operand copies of the blocks' matrices | ring buffers]
  const DecodeLayout L = decode_layout(C, S, O, n_blocks, cat ? V : DEC_HEAD_ROWS);
  const size_t wt_stride = (size_t)2 * C * 2 * C + (size_t)(C + S) * C;
  for (int i = 0; i < n_blocks; ++i) {
    const float* bw = packed + L.blocks + (size_t)i * L.block_stride;
    float* bt = scratch + (size_t)i * wt_stride;
    BLVM_TRY(t16_pack_rows(bw, 2 * C, 2 * C, 2 * C, bt, static_cast<hipStream_t>(stream)));
    BLVM_TRY(t16_pack_rows(bw + L.rs_w, C, C + S, C, bt + (size_t)2 * C * 2 * C, static_cast<hipStream_t>(stream)));
  }
  a.wt = scratch;
  a.queues = scratch + (size_t)n_blocks * wt_stride;
  const bool even = n_blocks % 2 == 0;
  if (tables) return decode_launch<EmbCatHead>(resume, even, a, lds, static_cast<hipStream_t>(stream));
  if (cat) return decode_launch<CatHead>(resume, even, a, lds, static_cast<hipStream_t>(stream));
  if (gauss) {
    GaussDecodeArgs g;
    static_cast<DecodeArgs&>(g) = a;
    g.sd_beta = sd_beta; g.sd_eps = sd_eps;
    if (gauss == 1) return decode_launch<GmmHead>(resume, even, g, lds, static_cast<hipStream_t>(stream));
    return decode_launch<GaussHead>(resume, even, g, lds, static_cast<hipStream_t>(stream));
  }
  return decode_launch<DmolHead>(resume, even, a, lds, static_cast<hipStream_t>(stream));
}

extern "C" int blvm_wavenet_decode(const float* packed, const int* dilations, int n_blocks, int B, int C, int S, int O,
                                   int num_mix, int n_frames, float inv_std, float skip_scale, float log_eps,
                                   const float* u, const float* v, float* scratch, float* x_out, void* stream) {
  return decode_run(false, packed, dilations, n_blocks, B, C, S, O, num_mix, n_frames, 0, inv_std, skip_scale, log_eps, u, v, nullptr,
                    scratch, x_out, nullptr, stream);
}

extern "C" int blvm_wavenet_decode_resume(const float* packed, const int* dilations, int n_blocks, int B, int C, int S, int O,
                                          int num_mix, int n_frames, int t0, float inv_std, float skip_scale, float log_eps,
                                          const float* u, const float* v, const float* x_in, float* scratch, float* x_out,
                                          float* x_state, void* stream) {
  return decode_run(true, packed, dilations, n_blocks, B, C, S, O, num_mix, n_frames, t0, inv_std, skip_scale, log_eps, u, v, x_in,
                    scratch, x_out, x_state, stream);
}

// The Gaussian heads: head_kind 1 the mixture (num_mix components, 3 * num_mix <= 32 head rows), 2 the plain Gaussian (2 head rows).
static int gauss_kind_ok(int head_kind) {
  BLVM_REQUIRE(head_kind == 1 || head_kind == 2, "wavenet_gauss_decode: head_kind must be 1 (Gaussian mixture) or 2 (Gaussian), got %d", head_kind);
  return BLVM_OK;
}

extern "C" int blvm_wavenet_gauss_decode(const float* packed, const int* dilations, int n_blocks, int B, int C, int S, int O, int head_kind,
                                         int num_mix, int n_frames, float inv_std, float skip_scale, float sd_beta, float sd_eps,
                                         const float* u, const float* n, float* scratch, float* x_out, void* stream) {
  BLVM_TRY(gauss_kind_ok(head_kind));
  return decode_run(false, packed, dilations, n_blocks, B, C, S, O, num_mix, n_frames, 0, inv_std, skip_scale, 0.f, u, n, nullptr, scratch,
                    x_out, nullptr, stream, 0, nullptr, nullptr, nullptr, head_kind, sd_beta, sd_eps);
}

extern "C" int blvm_wavenet_gauss_decode_resume(const float* packed, const int* dilations, int n_blocks, int B, int C, int S, int O,
                                                int head_kind, int num_mix, int n_frames, int t0, float inv_std, float skip_scale,
                                                float sd_beta, float sd_eps, const float* u, const float* n, const float* x_in,
                                                float* scratch, float* x_out, float* x_state, void* stream) {
  BLVM_TRY(gauss_kind_ok(head_kind));
  return decode_run(true, packed, dilations, n_blocks, B, C, S, O, num_mix, n_frames, t0, inv_std, skip_scale, 0.f, u, n, x_in, scratch,
                    x_out, x_state, stream, 0, nullptr, nullptr, nullptr, head_kind, sd_beta, sd_eps);
}

// The categorical head is built for 16 <= V <= 1024 in multiples of 16: one workgroup streams the whole head weight per frame, which
// at V = 65 536 needs a head split across workgroups — another kernel.
static int cat_widths_ok(int V) {
  if (V < blvm::CAT_MIN_V || V > blvm::CAT_MAX_V || V % 16 != 0) {
    blvm::set_error("wavenet_cat_decode: V = %d classes: the one-launch categorical head is built for %d <= V <= %d, V a multiple of 16",
                    V, blvm::CAT_MIN_V, blvm::CAT_MAX_V);
    return BLVM_ENOSUP;
  }
  return BLVM_OK;
}

extern "C" size_t blvm_wavenet_cat_decode_pack_floats(int C, int S, int O, int n_blocks, int V) {
  if (C <= 0 || S <= 0 || O <= 0 || n_blocks <= 0 || V <= 0) return 0;
  return blvm::decode_layout(C, S, O, n_blocks, V).total;
}

extern "C" int blvm_wavenet_cat_decode(const float* packed, const int* dilations, int n_blocks, int B, int C, int S, int O, int V,
                                       int n_frames, float inv_std, float skip_scale, const float* levels, const float* u,
                                       float* scratch, float* x_out, int32_t* k_out, void* stream) {
  BLVM_TRY(cat_widths_ok(V));
  return decode_run(false, packed, dilations, n_blocks, B, C, S, O, 0, n_frames, 0, inv_std, skip_scale, 0.f, u, nullptr, nullptr, scratch,
                    x_out, nullptr, stream, V, levels, k_out);
}

extern "C" int blvm_wavenet_cat_decode_resume(const float* packed, const int* dilations, int n_blocks, int B, int C, int S, int O, int V,
                                              int n_frames, int t0, float inv_std, float skip_scale, const float* levels,
                                              const float* u, const float* x_in, float* scratch, float* x_out, int32_t* k_out,
                                              float* x_state, void* stream) {
  BLVM_TRY(cat_widths_ok(V));
  return decode_run(true, packed, dilations, n_blocks, B, C, S, O, 0, n_frames, t0, inv_std, skip_scale, 0.f, u, nullptr, x_in, scratch,
                    x_out, x_state, stream, V, levels, k_out);
}

// The embedded model: the class pair travels through x_in / x_state as int32 words; the kernel clamps what it reads to [0, V).
extern "C" int blvm_wavenet_embed_cat_decode(const float* packed, const float* tables, const int* dilations, int n_blocks, int B, int C, int S,
                                             int O, int V, int n_frames, float inv_std, float skip_scale, const float* levels, const float* u,
                                             float* scratch, float* x_out, int32_t* k_out, void* stream) {
  BLVM_TRY(cat_widths_ok(V));
  BLVM_REQUIRE(tables && blvm::aligned16(tables), "wavenet_embed_cat_decode: NULL or misaligned tables");
  return decode_run(false, packed, dilations, n_blocks, B, C, S, O, 0, n_frames, 0, inv_std, skip_scale, 0.f, u, nullptr, nullptr, scratch,
                    x_out, nullptr, stream, V, levels, k_out, tables);
}

extern "C" int blvm_wavenet_embed_cat_decode_resume(const float* packed, const float* tables, const int* dilations, int n_blocks, int B, int C,
                                                    int S, int O, int V, int n_frames, int t0, float inv_std, float skip_scale,
                                                    const float* levels, const float* u, const int32_t* k_in, float* scratch, float* x_out,
                                                    int32_t* k_out, int32_t* k_state, void* stream) {
  BLVM_TRY(cat_widths_ok(V));
  BLVM_REQUIRE(tables && blvm::aligned16(tables), "wavenet_embed_cat_decode_resume: NULL or misaligned tables");
  return decode_run(true, packed, dilations, n_blocks, B, C, S, O, 0, n_frames, t0, inv_std, skip_scale, 0.f, u, nullptr,
                    reinterpret_cast<const float*>(k_in), scratch, x_out, reinterpret_cast<float*>(k_state), stream, V, levels, k_out, tables);
}

extern "C" int blvm_wavenet_decode_ring_fill(const float* h, int L, int B, int C, int dilation, int t0, float* ring, void* stream) {
  using namespace blvm;
  BLVM_REQUIRE(h && ring && aligned16(h) && aligned16(ring), "wavenet_decode_ring_fill: NULL or misaligned argument");
  BLVM_REQUIRE(B > 0 && C > 0 && C % 4 == 0 && dilation >= 1 && L >= dilation && t0 >= dilation,
               "wavenet_decode_ring_fill: need B > 0, C a multiple of 4, 1 <= dilation <= min(L, t0) (L %d, dilation %d, t0 %d)", L, dilation, t0);
  const size_t n4 = (size_t)dilation * B * (C / 4);
  BLVM_REQUIRE(n4 < (1ull << 31), "wavenet_decode_ring_fill: ring too large");
  hipLaunchKernelGGL(wn_ring_fill_kernel, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream),
                     reinterpret_cast<const float4*>(h + (size_t)(L - dilation) * B * C), reinterpret_cast<float4*>(ring),
                     (unsigned)(B * (C / 4)), (unsigned)dilation, (unsigned)((t0 - dilation) % dilation), (unsigned)n4);
  BLVM_CHECK_LAUNCH("wavenet_decode_ring_fill");
  return BLVM_OK;
}
