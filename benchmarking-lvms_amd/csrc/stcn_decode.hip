// stcn_decode.hip — K10d: ancestral sampling from the STCN, every step of every row in ONE launch.
//
// The reference leaves `STCN.generate` unimplemented (blvm/models/stcn/stcn.py:435-442); the generative model is the one its
// `forward` / `infer` define (stcn.py:299-326, 389-409) with every latent drawn from its prior.  One model step t:
//   c_t  = causal conv (kernel 2) of the stacks x_{t-2}, x_{t-1}            -> 1x1 in_transform -> the dilated gated blocks;
//   d[l] = the skip half of the block `forward` selects for level l         (features that have seen x[<t] only);
//   z[l] = mu + sd * eps[l][t], (mu, sd) = prior[l](cat[d[l], z[previous level visited]])   in the model's visiting order;
//   x_t  = DMoL draw per stacked sample from head(relu(out_upsample(inv_std * sum of the output stack's skips))), the output
//          stack (1x1 in_transform + n_out gated blocks of dilation 1) running on cat(z) (dense) or z[0].
// This is a chain of ~2 (n_blocks + n_out) + 3 n dependent small products per step — pure latency — so, as in K10c
// (wavenet_decode.hip), one workgroup owns 16 rows (the M of v_mfma_f32_16x16x4_f32) and never leaves the kernel: activations
// in LDS, every block a ring buffer [dil_i,B,C] of its own input in scratch, weights streamed from their T16 operand copies.
// Rows are independent: no inter-workgroup traffic.  The gated block, the tile layer and the draw are the ones K10c uses
// (decode_tiles.h).
//
// Zero past: `forward` pads x with receptive_field zero stacks and the output stack's input with n_out zero frames, exactly the
// windows of the first output.  Under an all-zero past every block input is constant in time, so the prologue evaluates that
// steady state once per stack (both taps on the same vector) and fills the rings with it.
//
// From a state (blvm_stcn_generate_resume: a prompt, or an earlier call): the rings and the two newest stacks ARE the state, so the
// entry skips that prologue, loads sX from x_in [B,2,S], counts ring slots from t0 and hands sX back in x_state after the last step —
// one branch, uniform over the grid.  The host primes the rings of a prompt with the time-parallel kernels (contract in the header).
//
// Widths: C and every latent size multiples of 16, 3 * num_mix <= 32, n <= 8, n_blocks, n_out <= 64.  S is any
// positive stack size: the causal convolution is an MFMA product when 2 S is a multiple of 16 and a scalar loop otherwise (S = 1).
// The packed image carries out_upsample zero-padded to a multiple of 16 rows and the head zero-padded to [32,32]; the kernel
// lays the up-sampled activations out as [sample][32] with two zero columns, so the head's K is 32.
//
// LDS map (floats; C = 256, S = 64, latents 256/128/64/32/16: 157 440 bytes):
//   sV   [16][max(2C, C + max Z)+4]  block taps (k = 2c + tap) | prior input cat[d, z_cond]
//   sPre [16][max(2C, 2 max Z)+4]    gate pre-activations      | prior hidden layer 1 (mu | sd), then the raw (mu | sd) of the level
//   sAct [16][C+4]   gated activations, causal conv output | prior hidden layer 2 (mu)
//   sH   [16][C+4]   current block input                   | prior hidden layer 2 (sd)
//   sSkip[16][C+4]   sum of the output stack's skips
//   sX   [16][2S+4]  the two previous stacks, interleaved (k = 2s + tap)
//   sZ   [16][sum Z + 4]  cat(z) of the step;  dead once the output stack's in_transform has read it, so the head's buffers
//   sUp  [16][8*32+4], sPar [16][8*32] (8 stacked samples per pass) alias it.
// The n selected skips [16][C] do not fit beside these: they are parked in scratch ([n,B,C]) and read back by the same
// workgroup after a barrier.
#include "common.h"
#include "decode_tiles.h"

namespace blvm {
namespace {

constexpr int SG_ROWS = 16;         // rows per workgroup
constexpr int SG_MAX_BLOCKS = 64;   // dilations and the level of every block travel by value in the kernel arguments
constexpr int SG_MAX_LEVELS = 8;
constexpr int SG_HEAD = 32;         // head rows / columns in the packed image (3 * num_mix <= 30, zero padded)
constexpr int SG_CHUNK = 8;         // stacked samples per head pass
constexpr int SG_NW = 8;            // waves per workgroup

// Offsets (floats) into the packed weight image.  Every matrix is a multiple of 256 floats or at least of 4, so every region starts
// on a 16-byte boundary.  The T16 operand copy of a matrix sits at the SAME offset of the copy image (a T16 copy has the size of its
// matrix), the bias regions of that image are unused.
struct StcnLayout {
  size_t causal_w, causal_b, in_w, in_b, blocks, block_stride, conv_b, rs_w, rs_b;  // conv_b, rs_w, rs_b relative to a block's start
  size_t prior[SG_MAX_LEVELS];  // level l: mu branch then sd branch, each w0 [C,Kin] b0 [C] w1 [C,C] b1 [C] w2 [Z,C] b2 [Z]
  size_t oin_w, oin_b, oblocks, up_w, up_b, head_w, head_b, total;
  int kin[SG_MAX_LEVELS], zoff[SG_MAX_LEVELS];  // prior input width; offset of z[l] in cat(z)
  int zin, zsum, zmax, up_rows;                 // output stack input width; sum and largest of the latent sizes; padded rows of out_upsample
};

inline size_t prior_branch_floats(int C, int kin, int Z) { return (size_t)C * kin + C + (size_t)C * C + C + (size_t)Z * C + Z; }

// order[i] = the level visited i-th; it conditions on order[i-1]
inline StcnLayout stcn_layout(int C, int S, int n_blocks, int n_out, const int* latent, const int* order, int n, int dense, int num_mix) {
  StcnLayout L{};
  size_t o = 0;
  L.causal_w = o; o += (size_t)C * 2 * S;  // [C,S,2]
  L.causal_b = o; o += C;
  L.in_w = o; o += (size_t)C * C;
  L.in_b = o; o += C;
  L.conv_b = (size_t)2 * C * 2 * C;
  L.rs_w = L.conv_b + 2 * C;
  L.rs_b = L.rs_w + (size_t)2 * C * C;
  L.block_stride = L.rs_b + 2 * C;
  L.blocks = o; o += L.block_stride * n_blocks;
  int off = 0;
  for (int l = 0; l < n; ++l) { L.zoff[l] = off; off += latent[l]; L.zmax = latent[l] > L.zmax ? latent[l] : L.zmax; }
  L.zsum = off;
  for (int i = 0; i < n; ++i) L.kin[order[i]] = C + (i > 0 ? latent[order[i - 1]] : 0);
  for (int l = 0; l < n; ++l) { L.prior[l] = o; o += 2 * prior_branch_floats(C, L.kin[l], latent[l]); }
  L.zin = dense ? L.zsum : latent[0];
  L.oin_w = o; o += (size_t)C * L.zin;
  L.oin_b = o; o += C;
  L.oblocks = o; o += L.block_stride * n_out;
  L.up_rows = (S * 3 * num_mix + 15) / 16 * 16;
  L.up_w = o; o += (size_t)L.up_rows * C;
  L.up_b = o; o += L.up_rows;
  L.head_w = o; o += (size_t)SG_HEAD * SG_HEAD;
  L.head_b = o; o += SG_HEAD;
  L.total = o;
  return L;
}

struct StcnArgs {
  const float* w;   // packed image
  const float* wt;  // T16 operand copies, same offsets
  StcnLayout L;
  int dil[SG_MAX_BLOCKS];
  signed char level[SG_MAX_BLOCKS];  // the latent level that reads block i's skip half, or -1
  int order[SG_MAX_LEVELS], Z[SG_MAX_LEVELS];
  int n_blocks, n_out, n, B, C, S, K, T;
  float inv_std, out_scale, sd_beta, sd_inv_beta, sd_eps, slope, log_eps;
  const float* eps[SG_MAX_LEVELS];  // [T,B,Z_l]
  const float* u;                   // [T,B,S,K] or NULL
  const float* v;                   // [T,B,S] or NULL
  float* x_out;                     // [B,T,S]
  float* z_out[SG_MAX_LEVELS];      // [T,B,Z_l]
  float* mu_out[SG_MAX_LEVELS];
  float* sd_out[SG_MAX_LEVELS];
  float* rings;   // dilated block i: [dil_i,B,C] at B*C*sum(dil[:i])
  float* orings;  // output block j: [B,C] at j*B*C
  float* dskip;   // [n,B,C] the selected skips of the step
  // the entry from a state: no steady-state prologue, the rings hold the blocks' inputs up to absolute step t0 - 1
  int resume, t0;        // t0 reduced modulo every dilation by the host; 0 on the zero start
  const float* x_in;     // [B,2,S] (previous stack, newest stack)
  float* x_state;        // [B,2,S] the two newest stacks after the last step (may be x_in)
};

struct StcnLds {
  int ldV, ldP, ldA, ldK, ldX, ldZ, ldU;
  size_t oV, oPre, oAct, oH, oSkip, oX, oR2, oPar, total;  // floats
};

__host__ __device__ inline StcnLds stcn_lds(int C, int S, int zsum, int zmax) {
  StcnLds m;
  m.ldV = (2 * C > C + zmax ? 2 * C : C + zmax) + 4; m.ldP = (C > zmax ? 2 * C : 2 * zmax) + 4; m.ldA = C + 4; m.ldK = C + 4; m.ldX = 2 * S + 4; m.ldZ = zsum + 4; m.ldU = SG_CHUNK * SG_HEAD + 4;
  size_t o = 0;
  m.oV = o; o += (size_t)SG_ROWS * m.ldV;
  m.oPre = o; o += (size_t)SG_ROWS * m.ldP;
  m.oAct = o; o += (size_t)SG_ROWS * m.ldA;
  m.oH = o; o += (size_t)SG_ROWS * m.ldA;
  m.oSkip = o; o += (size_t)SG_ROWS * m.ldK;
  m.oX = o; o += (size_t)SG_ROWS * m.ldX;
  m.oR2 = o;
  const size_t zf = (size_t)SG_ROWS * m.ldZ, hf = (size_t)SG_ROWS * m.ldU + (size_t)SG_ROWS * SG_CHUNK * SG_HEAD;
  m.oPar = o + (size_t)SG_ROWS * m.ldU;
  o += zf > hf ? zf : hf;
  m.total = o;
  return m;
}

__global__ __launch_bounds__(SG_NW * 64) void stcn_decode_kernel(StcnArgs a) {
  extern __shared__ __align__(16) float smem[];
  constexpr int NW = SG_NW, NT = SG_NW * 64;
  const int C = a.C, S = a.S, B = a.B, K = a.K, F = 3 * a.K;
  const StcnLds m = stcn_lds(C, S, a.L.zsum, a.L.zmax);
  const int ldV = m.ldV, ldP = m.ldP, ldA = m.ldA, ldH = m.ldA, ldK = m.ldK, ldX = m.ldX, ldZ = m.ldZ, ldU = m.ldU;
  float* sV = smem + m.oV;
  float* sPre = smem + m.oPre;
  float* sAct = smem + m.oAct;
  float* sH = smem + m.oH;
  float* sSkip = smem + m.oSkip;
  float* sX = smem + m.oX;
  float* sZ = smem + m.oR2;
  float* sUp = smem + m.oR2;
  float* sPar = smem + m.oPar;

  const int tid = threadIdx.x, wave = tid >> 6;
  const int b0 = blockIdx.x * SG_ROWS;
  const float* w = a.w;
  const float* wt = a.wt;
  const int CT = C / 16;

  for (int i = tid; i < SG_ROWS * ldX; i += NT) sX[i] = 0.f;
  for (int i = tid; i < SG_ROWS * ldZ; i += NT) sZ[i] = 0.f;
  __syncthreads();
  if (a.resume) {  // uniform over the grid: the two newest stacks of the state, rows >= B stay zero
    for (int idx = tid; idx < SG_ROWS * 2 * S; idx += NT) {
      const int r = idx / (2 * S), k = idx - r * 2 * S, tap = k / S, s = k - tap * S;
      if (b0 + r < B) sX[r * ldX + 2 * s + tap] = a.x_in[(size_t)(b0 + r) * 2 * S + k];
    }
    __syncthreads();
  }

  // causal conv on the two previous stacks -> 1x1 in_transform -> sH
  auto front = [&]() {
    if ((2 * S) % 16 == 0) {
      tile_layer<NW, true>(sX, ldX, wt + a.L.causal_w, 2 * S, 0, CT, w + a.L.causal_b, [&](int row, int o, float val) { sAct[row * ldA + o] = val; });
    } else {
      const float* cw = w + a.L.causal_w;
      for (int idx = tid; idx < SG_ROWS * C; idx += NT) {
        const int r = idx / C, o = idx - r * C;
        float acc = w[a.L.causal_b + o];
        for (int k = 0; k < 2 * S; ++k) acc = fmaf(cw[(size_t)o * 2 * S + k], sX[r * ldX + k], acc);
        sAct[r * ldA + o] = acc;
      }
    }
    __syncthreads();
    tile_layer<NW, true>(sAct, ldA, wt + a.L.in_w, C, 0, CT, w + a.L.in_b, [&](int row, int o, float val) { sH[row * ldH + o] = val; });
    __syncthreads();
  };

  // 1x1 in_transform of the output stack on sZ -> sH
  auto out_in = [&]() {
    tile_layer<NW, true>(sZ, ldZ, wt + a.L.oin_w, a.L.zin, 0, CT, w + a.L.oin_b, [&](int row, int o, float val) { sH[row * ldH + o] = val; });
    __syncthreads();
  };

  // One gated residual block (decode_tiles.h; packed offset boff) on the frame in sH; its ring qi [d,B,C].  steady: both taps = sH
  // and the ring is filled with sH.  skip_mode 0: no skip half; 1: added into sSkip; 2: stored to gskip [B,C].  need_res: the
  // residual half.
  const GateLds gl = {sH, ldH, sV, ldV, sPre, ldP, sAct, ldA};
  auto block = [&](size_t boff, float* qi, int d, int slot, bool steady, int skip_mode, float* gskip, bool need_res) {
    const float* bw = w + boff;
    const float* bt = wt + boff;
    gated_ring_block<NW>(gl, C, bt, bw + a.L.conv_b, bt + a.L.rs_w, bw + a.L.rs_b, qi, d, slot, steady, b0, B, a.inv_std, need_res ? 0 : CT,
                         skip_mode ? 2 * CT : CT, [&](int row, int j, float val) {
                           if (skip_mode == 1) sSkip[row * ldK + j] += val;
                           else if (b0 + row < B) gskip[(size_t)(b0 + row) * C + j] = val;
                         });
  };

  // ---- steady state under an all-zero past: both stacks
  if (!a.resume) {
    front();
    float* qi = a.rings;
    for (int i = 0; i < a.n_blocks; ++i) {
      block(a.L.blocks + (size_t)i * a.L.block_stride, qi, a.dil[i], 0, true, 0, nullptr, true);
      qi += (size_t)a.dil[i] * B * C;
    }
    out_in();  // sZ = 0: the response to the zero padding of the output stack's input
    for (int j = 0; j < a.n_out; ++j)
      block(a.L.oblocks + (size_t)j * a.L.block_stride, a.orings + (size_t)j * B * C, 1, 0, true, 0, nullptr, true);
  }

  for (int t = 0; t < a.T; ++t) {
    // ---- A: deterministic features; the selected skips go to scratch
    front();
    {
      float* qi = a.rings;
      for (int i = 0; i < a.n_blocks; ++i) {
        const int lvl = a.level[i], d = a.dil[i];
        block(a.L.blocks + (size_t)i * a.L.block_stride, qi, d, (a.t0 + t) % d, false, lvl >= 0 ? 2 : 0,
              lvl >= 0 ? a.dskip + (size_t)lvl * B * C : nullptr, i + 1 < a.n_blocks);
        qi += (size_t)d * B * C;
      }
    }
    // ---- B: the latents in the model's visiting order, each from its prior
    for (int i = 0; i < a.n; ++i) {
      const int l = a.order[i], Zl = a.Z[l], kin = a.L.kin[l];
      const float* dl = a.dskip + (size_t)l * B * C;
      for (int idx = tid; idx < SG_ROWS * C; idx += NT) {
        const int r = idx / C, c = idx - r * C;
        sV[r * ldV + c] = b0 + r < B ? dl[(size_t)(b0 + r) * C + c] : 0.f;
      }
      if (i > 0) {
        const int lc = a.order[i - 1], Zc = a.Z[lc], zo = a.L.zoff[lc];
        for (int idx = tid; idx < SG_ROWS * Zc; idx += NT) {
          const int r = idx / Zc, j = idx - r * Zc;
          sV[r * ldV + C + j] = sZ[r * ldZ + zo + j];
        }
      }
      __syncthreads();
      const size_t bs = (size_t)C * kin + C + (size_t)C * C + C + (size_t)Zl * C + Zl;  // one branch
      const size_t o_b0 = (size_t)C * kin, o_w1 = o_b0 + C, o_b1 = o_w1 + (size_t)C * C, o_w2 = o_b1 + C, o_b2 = o_w2 + (size_t)Zl * C;
      for (int tile = wave; tile < 2 * CT; tile += NW) {  // layer 1 of both branches: sV -> sPre (mu | sd)
        const int br = tile >= CT, tt = tile - br * CT;
        const size_t P = a.L.prior[l] + br * bs;
        tile16<true>(sV, ldV, wt + P, kin, tt, w + P + o_b0, [&](int row, int o, float val) { sPre[row * ldP + br * C + o] = val > 0.f ? val : a.slope * val; });
      }
      __syncthreads();
      for (int tile = wave; tile < 2 * CT; tile += NW) {  // layer 2: sPre -> sAct (mu), sH (sd)
        const int br = tile >= CT, tt = tile - br * CT;
        const size_t P = a.L.prior[l] + br * bs;
        float* dst = br ? sH : sAct;
        tile16<true>(sPre + br * C, ldP, wt + P + o_w1, C, tt, w + P + o_b1, [&](int row, int o, float val) { dst[row * ldA + o] = val > 0.f ? val : a.slope * val; });
      }
      __syncthreads();
      const int ZT = Zl / 16;
      for (int tile = wave; tile < 2 * ZT; tile += NW) {  // layer 3: raw (mu | sd) -> sPre
        const int br = tile >= ZT, tt = tile - br * ZT;
        const size_t P = a.L.prior[l] + br * bs;
        tile16<true>(br ? sH : sAct, ldA, wt + P + o_w2, C, tt, w + P + o_b2, [&](int row, int o, float val) { sPre[row * ldP + br * Zl + o] = val; });
      }
      __syncthreads();
      for (int idx = tid; idx < SG_ROWS * Zl; idx += NT) {
        const int r = idx / Zl, j = idx - r * Zl;
        const float mu = sPre[r * ldP + j];
        const float sd = softplus_beta(sPre[r * ldP + Zl + j], a.sd_beta, a.sd_inv_beta) + a.sd_eps;
        float z = mu;
        if (b0 + r < B) {
          const size_t at = ((size_t)t * B + b0 + r) * Zl + j;
          z = fmaf(sd, a.eps[l][at], mu);
          a.mu_out[l][at] = mu;
          a.sd_out[l][at] = sd;
          a.z_out[l][at] = z;
        }
        sZ[r * ldZ + a.L.zoff[l] + j] = z;
      }
      __syncthreads();
    }
    // ---- C: the output stack on cat(z) (or z[0]); rings of depth 1
    for (int idx = tid; idx < SG_ROWS * C; idx += NT) {
      const int r = idx / C;
      sSkip[r * ldK + (idx - r * C)] = 0.f;
    }
    out_in();
    for (int j = 0; j < a.n_out; ++j)
      block(a.L.oblocks + (size_t)j * a.L.block_stride, a.orings + (size_t)j * B * C, 1, 0, false, 1, nullptr, j + 1 < a.n_out);
    // ---- D: * inv_std -> out_upsample + ReLU -> head -> draw, SG_CHUNK stacked samples per pass (sZ is dead: sUp / sPar alias it)
    for (int idx = tid; idx < SG_ROWS * C; idx += NT) {
      const int r = idx / C;
      sSkip[r * ldK + (idx - r * C)] *= a.out_scale;
    }
    __syncthreads();
    for (int s0 = 0; s0 < S; s0 += SG_CHUNK) {
      const int ns = S - s0 < SG_CHUNK ? S - s0 : SG_CHUNK;
      const int col_lo = s0 * F, col_hi = (s0 + ns) * F;
      for (int idx = tid; idx < SG_ROWS * SG_CHUNK * (SG_HEAD - F); idx += NT) {  // the zero columns F .. 31 of every sample
        const int pw = SG_HEAD - F, r = idx / (SG_CHUNK * pw), rem = idx - r * SG_CHUNK * pw;
        sUp[r * ldU + (rem / pw) * SG_HEAD + F + rem % pw] = 0.f;
      }
      // (a tile may straddle the chunk's columns; the bias region is padded to whole tiles like the matrix)
      tile_layer<NW, true>(sSkip, ldK, wt + a.L.up_w, C, col_lo / 16, (col_hi + 15) / 16, w + a.L.up_b, [&](int row, int col, float val) {
        if (col >= col_lo && col < col_hi) sUp[row * ldU + (col / F - s0) * SG_HEAD + col % F] = fmaxf(val, 0.f);
      });
      __syncthreads();
      for (int job = wave; job < ns * (SG_HEAD / 16); job += NW) {
        const int sl = job / (SG_HEAD / 16), ht = job % (SG_HEAD / 16);
        tile16<true>(sUp + sl * SG_HEAD, ldU, wt + a.L.head_w, SG_HEAD, ht, w + a.L.head_b,
                     [&](int row, int o, float val) { sPar[row * (SG_CHUNK * SG_HEAD) + sl * SG_HEAD + o] = val; });
      }
      __syncthreads();
      if (tid < SG_ROWS * ns) {
        // Gumbel-max component pick + clamped logistic draw (decode_tiles.h)
        const int r = tid % SG_ROWS, sl = tid / SG_ROWS, s = s0 + sl;
        float x = 0.f;
        if (b0 + r < B) {
          const float* p = sPar + r * (SG_CHUNK * SG_HEAD) + sl * SG_HEAD;
          const size_t f = ((size_t)t * B + b0 + r) * S + s;
          const int best = mix_pick(p, K, a.u != nullptr ? a.u + f * K : nullptr);
          x = p[K + best];
          if (a.v != nullptr) x = logistic_draw(x, p[2 * K + best], a.v[f], a.log_eps);
          a.x_out[((size_t)(b0 + r) * a.T + t) * S + s] = x;
        }
        sX[r * ldX + 2 * s] = sX[r * ldX + 2 * s + 1];
        sX[r * ldX + 2 * s + 1] = x;
      }
      __syncthreads();
    }
  }
  if (a.resume) {  // the last update of sX is behind the barrier that ends the step
    for (int idx = tid; idx < SG_ROWS * 2 * S; idx += NT) {
      const int r = idx / (2 * S), k = idx - r * 2 * S, tap = k / S, s = k - tap * S;
      if (b0 + r < B) a.x_state[(size_t)(b0 + r) * 2 * S + k] = sX[r * ldX + 2 * s + tap];
    }
  }
}

// Everything the entry points refuse, before anything is touched
int stcn_check_shape(int C, int S, int n_blocks, int n_out, const int* latent, const int* order, int n, int num_mix) {
  BLVM_REQUIRE(latent && order, "stcn_generate: NULL latent sizes or visiting order");
  BLVM_REQUIRE(n >= 1 && n <= SG_MAX_LEVELS, "stcn_generate: n_latents = %d, need 1 .. %d", n, SG_MAX_LEVELS);
  BLVM_REQUIRE(n_blocks >= 1 && n_blocks <= SG_MAX_BLOCKS && n_out >= 1 && n_out <= SG_MAX_BLOCKS,
               "stcn_generate: n_blocks = %d, n_out = %d, need 1 .. %d each", n_blocks, n_out, SG_MAX_BLOCKS);
  BLVM_REQUIRE(C > 0 && C % 16 == 0 && C <= 4096, "stcn_generate: C = %d must be a multiple of 16 (at most 4096)", C);
  BLVM_REQUIRE(S > 0 && S <= 4096, "stcn_generate: S = %d, need 1 .. 4096", S);
  BLVM_REQUIRE(num_mix > 0 && 3 * num_mix <= SG_HEAD, "stcn_generate: num_mix = %d, need 1 .. %d", num_mix, SG_HEAD / 3);
  unsigned seen = 0;
  for (int i = 0; i < n; ++i) {
    BLVM_REQUIRE(latent[i] > 0 && latent[i] % 16 == 0 && latent[i] <= 4096, "stcn_generate: latent size %d of level %d must be a multiple of 16 (at most 4096)", latent[i], i);
    BLVM_REQUIRE(order[i] >= 0 && order[i] < n && !(seen & (1u << order[i])), "stcn_generate: the visiting order is no permutation of the levels");
    seen |= 1u << order[i];
  }
  return BLVM_OK;
}

}  // namespace
}  // namespace blvm

extern "C" size_t blvm_stcn_generate_pack_floats(int C, int S, int n_blocks, int n_out, const int* latent, const int* order, int n_latents,
                                                 int dense, int num_mix) {
  using namespace blvm;
  if (stcn_check_shape(C, S, n_blocks, n_out, latent, order, n_latents, num_mix) != BLVM_OK) return 0;
  return stcn_layout(C, S, n_blocks, n_out, latent, order, n_latents, dense, num_mix).total;
}

extern "C" size_t blvm_stcn_generate_scratch_floats(const int* dilations, int C, int S, int n_blocks, int n_out, const int* latent,
                                                    const int* order, int n_latents, int dense, int num_mix, int B) {
  using namespace blvm;
  if (!dilations || B <= 0 || stcn_check_shape(C, S, n_blocks, n_out, latent, order, n_latents, num_mix) != BLVM_OK) return 0;
  // [T16 operand copies | rings of the dilated blocks | rings of the output blocks | the selected skips]
  return stcn_layout(C, S, n_blocks, n_out, latent, order, n_latents, dense, num_mix).total + ring_floats(dilations, n_blocks, B, C) +
         (size_t)n_out * B * C + (size_t)n_latents * B * C;
}

extern "C" size_t blvm_stcn_generate_ring_offset_floats(int C, int S, int n_blocks, int n_out, const int* latent, const int* order,
                                                        int n_latents, int dense, int num_mix) {
  return blvm_stcn_generate_pack_floats(C, S, n_blocks, n_out, latent, order, n_latents, dense, num_mix);  // the T16 copies mirror the image
}

// resume: the kernel starts from the rings in `scratch` and x_in at absolute step t0 and hands the two newest stacks back
static int stcn_run(bool resume, const float* packed, const int* dilations, const int* groups, int n_blocks, int n_out, const int* latent,
                    const int* order, int n_latents, int dense, int B, int C, int S, int num_mix, int T, float inv_std, float out_scale,
                    float sd_beta, float sd_eps, float slope, float log_eps, const float* const* eps, const float* u, const float* v,
                    float* x_out, float* const* z_out, float* const* mu_out, float* const* sd_out, float* scratch, int t0,
                    const float* x_in, float* x_state, void* stream) {
  using namespace blvm;
  hipStream_t s = static_cast<hipStream_t>(stream);
  BLVM_REQUIRE(packed && dilations && groups && eps && x_out && z_out && mu_out && sd_out && scratch && aligned16(packed) && aligned16(scratch),
               "stcn_generate: NULL or misaligned argument");
  BLVM_TRY(stcn_check_shape(C, S, n_blocks, n_out, latent, order, n_latents, num_mix));
  BLVM_REQUIRE(B > 0 && T >= 0, "stcn_generate: need B > 0, T >= 0");
  BLVM_REQUIRE((u == nullptr) == (v == nullptr), "stcn_generate: u and v are given together (both NULL: the mode)");
  BLVM_REQUIRE(sd_beta > 0.f, "stcn_generate: the softplus beta must be positive");
  if (resume) BLVM_TRY(check_resume("stcn_generate_resume", "stack", "T", t0, T, x_in, x_state));
  const int n = n_latents;
  StcnArgs a{};
  unsigned selected = 0;
  for (int i = 0; i < n_blocks; ++i) {
    BLVM_REQUIRE(dilations[i] >= 1, "stcn_generate: dilation %d of block %d", dilations[i], i);
    BLVM_REQUIRE(groups[i] >= -1 && groups[i] < n, "stcn_generate: block %d feeds level %d of %d", i, groups[i], n);
    if (groups[i] >= 0) {
      BLVM_REQUIRE(!(selected & (1u << groups[i])), "stcn_generate: level %d reads more than one block", groups[i]);
      selected |= 1u << groups[i];
    }
    a.dil[i] = dilations[i];
    a.level[i] = (signed char)groups[i];
  }
  BLVM_REQUIRE(selected == (1u << n) - 1u, "stcn_generate: every level needs the skip of one block");
  for (int i = n_blocks; i < SG_MAX_BLOCKS; ++i) { a.dil[i] = 1; a.level[i] = -1; }
  for (int l = 0; l < n; ++l)
    BLVM_REQUIRE(eps[l] && z_out[l] && mu_out[l] && sd_out[l], "stcn_generate: NULL eps / z / mu / sd of level %d", l);
  a.L = stcn_layout(C, S, n_blocks, n_out, latent, order, n, dense, num_mix);
  const StcnLds m = stcn_lds(C, S, a.L.zsum, a.L.zmax);
  const size_t lds = sizeof(float) * m.total;
  BLVM_REQUIRE(lds <= 160 * 1024, "stcn_generate: C=%d, S=%d, %d latent dimensions need %zu bytes of LDS (> 160 KB)", C, S, a.L.zsum, lds);
  if (T == 0) return resume ? hand_back_state(x_state, x_in, (size_t)2 * S * B, s) : BLVM_OK;

  a.w = packed;
  a.wt = scratch;
  {
    // T16 operand copies, same offsets as the packed image
    T16PackScope pack_scope(OP_F32, s);
#define PACK(off, rows, k) BLVM_TRY(t16_pack_rows(packed + (off), (k), (rows), (k), scratch + (off), s))
    if ((2 * S) % 16 == 0) PACK(a.L.causal_w, C, 2 * S);
    PACK(a.L.in_w, C, C);
    for (int i = 0; i < n_blocks + n_out; ++i) {
      const size_t bo = i < n_blocks ? a.L.blocks + (size_t)i * a.L.block_stride : a.L.oblocks + (size_t)(i - n_blocks) * a.L.block_stride;
      PACK(bo, 2 * C, 2 * C);
      PACK(bo + a.L.rs_w, 2 * C, C);
    }
    for (int l = 0; l < n; ++l) {
      const int kin = a.L.kin[l], Z = latent[l];
      const size_t bs = prior_branch_floats(C, kin, Z);
      for (int br = 0; br < 2; ++br) {
        const size_t P = a.L.prior[l] + br * bs;
        PACK(P, C, kin);
        PACK(P + (size_t)C * kin + C, C, C);
        PACK(P + (size_t)C * kin + C + (size_t)C * C + C, Z, C);
      }
    }
    PACK(a.L.oin_w, C, a.L.zin);
    PACK(a.L.up_w, a.L.up_rows, C);
    PACK(a.L.head_w, SG_HEAD, SG_HEAD);
#undef PACK
    BLVM_TRY(pack_scope.flush());
  }
  for (int l = 0; l < n; ++l) {
    a.order[l] = order[l]; a.Z[l] = latent[l];
    a.eps[l] = eps[l]; a.z_out[l] = z_out[l]; a.mu_out[l] = mu_out[l]; a.sd_out[l] = sd_out[l];
  }
  a.n_blocks = n_blocks; a.n_out = n_out; a.n = n; a.B = B; a.C = C; a.S = S; a.K = num_mix; a.T = T;
  a.inv_std = inv_std; a.out_scale = out_scale; a.sd_beta = sd_beta; a.sd_inv_beta = 1.f / sd_beta; a.sd_eps = sd_eps;
  a.slope = slope; a.log_eps = log_eps;
  a.u = u; a.v = v; a.x_out = x_out;
  a.rings = scratch + a.L.total;
  a.orings = a.rings + ring_floats(dilations, n_blocks, B, C);
  a.dskip = a.orings + (size_t)n_out * B * C;
  a.resume = resume ? 1 : 0; a.t0 = resume ? t0 : 0; a.x_in = x_in; a.x_state = x_state;
  auto kern = stcn_decode_kernel;
  if (lds > 64 * 1024) BLVM_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  hipLaunchKernelGGL(kern, dim3((unsigned)((B + SG_ROWS - 1) / SG_ROWS)), dim3(SG_NW * 64), lds, s, a);
  BLVM_CHECK_LAUNCH("stcn_generate");
  return BLVM_OK;
}

extern "C" int blvm_stcn_generate(const float* packed, const int* dilations, const int* groups, int n_blocks, int n_out, const int* latent,
                                  const int* order, int n_latents, int dense, int B, int C, int S, int num_mix, int T, float inv_std,
                                  float out_scale, float sd_beta, float sd_eps, float slope, float log_eps, const float* const* eps,
                                  const float* u, const float* v, float* x_out, float* const* z_out, float* const* mu_out,
                                  float* const* sd_out, float* scratch, void* stream) {
  return stcn_run(false, packed, dilations, groups, n_blocks, n_out, latent, order, n_latents, dense, B, C, S, num_mix, T, inv_std, out_scale,
                  sd_beta, sd_eps, slope, log_eps, eps, u, v, x_out, z_out, mu_out, sd_out, scratch, 0, nullptr, nullptr, stream);
}

extern "C" int blvm_stcn_generate_resume(const float* packed, const int* dilations, const int* groups, int n_blocks, int n_out,
                                         const int* latent, const int* order, int n_latents, int dense, int B, int C, int S, int num_mix,
                                         int T, float inv_std, float out_scale, float sd_beta, float sd_eps, float slope, float log_eps,
                                         const float* const* eps, const float* u, const float* v, float* x_out, float* const* z_out,
                                         float* const* mu_out, float* const* sd_out, float* scratch, int t0, const float* x_in,
                                         float* x_state, void* stream) {
  return stcn_run(true, packed, dilations, groups, n_blocks, n_out, latent, order, n_latents, dense, B, C, S, num_mix, T, inv_std, out_scale,
                  sd_beta, sd_eps, slope, log_eps, eps, u, v, x_out, z_out, mu_out, sd_out, scratch, t0, x_in, x_state, stream);
}
