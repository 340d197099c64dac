// gemm.hip — K6: fp32 GEMM on v_mfma_f32_32x32x2_f32 with fused bias / activation / activation-derivative epilogue.
//
// Replaces the nn.Linear(+LeakyReLU/ReLU) chains of the reference's encoder/decoder MLPs
// (blvm/models/vrnn.py:487-505, srnn.py:456-474, lstm.py:38-64) and their autograd backward (dgrad / wgrad).
//
// Design (gfx950): 256-thread workgroups = 4 waves in a 2x2 arrangement, block tile BMxBN (128x128 or 64x64),
// BK = 16.  Both operands are staged k-major in LDS (As[k][m], Bs[k][n], row pad 4 floats) so that every MFMA
// operand fetch is a conflict-free ds_read_b32 whatever the global layout (op_a/op_b) was; the transposition is
// done by the global->LDS stage.  Next tile is prefetched into registers while the current one is multiplied.
// f32-in MFMA is an exact fp32 fma chain (guide §3 'FP32-input MFMA'), so results are bit-reproducible except
// for split-K (atomic) accumulation order.
#include <algorithm>
#include <atomic>
#include <type_traits>

#include <vector>

#include "bf16_slice.h"
#include "common.h"

namespace blvm {

namespace {

constexpr int BK = 16;    // k-tile depth of the 128-wide tiles (and the unit of the host's split arithmetic)
constexpr int BK64 = 32;  // k-tile depth of the 64 x 64 tiles (64 deep measured: slower)
constexpr int tile_bk(int bm, int bn) { return (bm == 64 && bn == 64) ? BK64 : BK; }

constexpr int PAD = 4;
constexpr int PAD_T = 2;

struct GemmArgs {
  const float* A;
  const float* B;
  float* C;
  const float* bias;
  const float* gate;
  int M, N, K, lda, ldb, ldc, ldg;
  int act;
  float slope;
  int accumulate;
  int k_per_split;  // multiple of BK
  int a_vec, b_vec;  // 16-byte vector loads allowed for A / B
  float* colsum;     // op_a == 1 only: [M] += column sums of A over k (the bias gradient of a weight-gradient GEMM), or null
};

// Load 4 consecutive elements p[0..3] with element-wise validity n_valid (0..4).
__device__ __forceinline__ float4 ld4(const float* p, int n_valid, bool vec) {
  float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
  if (n_valid >= 4 && vec) {
    v = *reinterpret_cast<const float4*>(p);
  } else {
    if (n_valid > 0) v.x = p[0];
    if (n_valid > 1) v.y = p[1];
    if (n_valid > 2) v.z = p[2];
    if (n_valid > 3) v.w = p[3];
  }
  return v;
}

// one BM x BN output tile over the k range of split `bz` of `nz` (the body of gemm_kernel)
template <int BM, int BN, int OPA, int OPB>
__device__ __forceinline__ void gemm_tile(const GemmArgs& g, const int bx, const int by, const int bz, const int nz) {
  // k-tile depth by tile size: 64 x 64 tiles (8 MFMAs per wave and 16 k, 49 VGPRs at depth 32: still 7 waves per SIMD) run 32 deep --
  // half the barriers per MFMA: weight-gradient forms +4..5 %, WaveNet's K = 96 convs +4 %; the 128-wide tiles would drop from 3 to
  // 2 waves per SIMD at depth 32 (dec L3 forward 195 -> 218 us) and stay at 16.
  constexpr int BK = tile_bk(BM, BN), KV = BK / 4;
  // row pad of the k-major LDS tiles: 4 floats keep the 16-byte stores of an OP == 1 operand aligned; an OP == 0 operand is written
  // by scalar stores whose lanes are 4 k apart (4 rows): with a pad of 2, 4 rows are 8 banks apart and the 32 lanes of a store hit
  // 32 banks (pad 4: 16 banks twice -- SQ_LDS_BANK_CONFLICT was 70 % of the kernel's LDS cycles)
  // (32-deep tiles: 8 lanes per row, a pad of 1 puts 4 rows 4 banks apart)
  constexpr int PT = BK == 32 ? (PAD_T + 1) / 2 : PAD_T;
  constexpr int LDA_S = BM + (OPA == 0 ? PT : PAD), LDB_S = BN + (OPB == 0 ? PT : PAD);
  constexpr int TM = BM / 64, TN = BN / 64;  // 32x32 MFMA tiles per wave in m / n
  constexpr int A_V = BM * BK / 4 / 256;     // float4 per thread per stage
  constexpr int B_V = BN * BK / 4 / 256;
  __shared__ __attribute__((aligned(16))) float As[BK * LDA_S];
  __shared__ __attribute__((aligned(16))) float Bs[BK * LDB_S];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int m0 = by * BM, n0 = bx * BN;
  const int kbeg = bz * g.k_per_split;
  const int kend = min(g.K, kbeg + g.k_per_split);

  f32x16 acc[TM][TN];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  float4 ra[A_V], rb[B_V];

  auto load_tiles = [&](int k0) {
#pragma unroll
    for (int v = 0; v < A_V; ++v) {
      const int id = tid + v * 256;
      if (OPA == 0) {  // A[m][k], k contiguous: 4 float4 per row of the tile
        const int m = id / KV, k4 = (id % KV) * 4;
        const int gm = m0 + m, gk = k0 + k4;
        const int nv = (gm < g.M) ? max(0, min(4, kend - gk)) : 0;
        ra[v] = ld4(g.A + (size_t)(gm < g.M ? gm : 0) * g.lda + gk, nv, g.a_vec);
      } else {  // A[k][m], m contiguous
        const int k = id / (BM / 4), m4 = (id % (BM / 4)) * 4;
        const int gm = m0 + m4, gk = k0 + k;
        const int nv = (gk < kend) ? max(0, min(4, g.M - gm)) : 0;
        ra[v] = ld4(g.A + (size_t)(gk < kend ? gk : 0) * g.lda + gm, nv, g.a_vec);
      }
    }
#pragma unroll
    for (int v = 0; v < B_V; ++v) {
      const int id = tid + v * 256;
      if (OPB == 0) {  // B[n][k], k contiguous
        const int n = id / KV, k4 = (id % KV) * 4;
        const int gn = n0 + n, gk = k0 + k4;
        const int nv = (gn < g.N) ? max(0, min(4, kend - gk)) : 0;
        rb[v] = ld4(g.B + (size_t)(gn < g.N ? gn : 0) * g.ldb + gk, nv, g.b_vec);
      } else {  // B[k][n], n contiguous
        const int k = id / (BN / 4), n4 = (id % (BN / 4)) * 4;
        const int gn = n0 + n4, gk = k0 + k;
        const int nv = (gk < kend) ? max(0, min(4, g.N - gn)) : 0;
        rb[v] = ld4(g.B + (size_t)(gk < kend ? gk : 0) * g.ldb + gn, nv, g.b_vec);
      }
    }
  };

  auto store_tiles = [&]() {
#pragma unroll
    for (int v = 0; v < A_V; ++v) {
      const int id = tid + v * 256;
      if (OPA == 0) {
        const int m = id / KV, k4 = (id % KV) * 4;
        As[(k4 + 0) * LDA_S + m] = ra[v].x;
        As[(k4 + 1) * LDA_S + m] = ra[v].y;
        As[(k4 + 2) * LDA_S + m] = ra[v].z;
        As[(k4 + 3) * LDA_S + m] = ra[v].w;
      } else {
        const int k = id / (BM / 4), m4 = (id % (BM / 4)) * 4;
        *reinterpret_cast<float4*>(&As[k * LDA_S + m4]) = ra[v];
      }
    }
#pragma unroll
    for (int v = 0; v < B_V; ++v) {
      const int id = tid + v * 256;
      if (OPB == 0) {
        const int n = id / KV, k4 = (id % KV) * 4;
        Bs[(k4 + 0) * LDB_S + n] = rb[v].x;
        Bs[(k4 + 1) * LDB_S + n] = rb[v].y;
        Bs[(k4 + 2) * LDB_S + n] = rb[v].z;
        Bs[(k4 + 3) * LDB_S + n] = rb[v].w;
      } else {
        const int k = id / (BN / 4), n4 = (id % (BN / 4)) * 4;
        *reinterpret_cast<float4*>(&Bs[k * LDB_S + n4]) = rb[v];
      }
    }
  };

  if (kbeg < kend) load_tiles(kbeg);
  const int li = lane & 31, lh = lane >> 5;
  // bias gradient riding on a weight-gradient GEMM: the workgroups of the first column block also sum their A tiles over k
  // (A = the pre-activation gradients [rows, M]; the staged tile is k-major, so thread m reads a conflict-free column)
  const bool do_csum = OPA == 1 && g.colsum != nullptr && bx == 0;
  constexpr int CS = BM <= 64 ? 4 : (BM <= 128 ? 2 : 1);
  float csum = 0.f;
  for (int k0 = kbeg; k0 < kend; k0 += BK) {
    __syncthreads();  // previous tile fully consumed
    store_tiles();
    __syncthreads();
    if (k0 + BK < kend) load_tiles(k0 + BK);  // prefetch next tile into registers
    if (do_csum && tid / BM < CS) {  // CS threads share a column: every wave carries the same few extra LDS reads
#pragma unroll
      for (int kk = 0; kk < BK / CS; ++kk) csum += As[(kk * CS + tid / BM) * LDA_S + tid % BM];
    }
    // the operands of k-pair s + 1 are requested from LDS BEFORE the MFMAs of k-pair s are issued (two register sets): the LDS
    // round trip hides behind TM x TN matrix instructions instead of standing in front of them.  The order is pinned with
    // sched_group_barrier: without the pins the compiler sinks the reads back next to their use.  Measured r03 against the plain
    // loop: VRNN 15.23 -> 15.18, STCN 32.93 -> 32.51, CW-VAE 86.3 -> 85.9 ms/step; the weight-gradient forms +3..4 %, the K = 256
    // forward forms -1 %.
    float a[2][TM], b[2][TN];
    auto lds_ab = [&](int kk, float (&a_)[TM], float (&b_)[TN]) {
#pragma unroll
      for (int i = 0; i < TM; ++i) a_[i] = As[(kk + lh) * LDA_S + wm * (BM / 2) + i * 32 + li];
#pragma unroll
      for (int j = 0; j < TN; ++j) b_[j] = Bs[(kk + lh) * LDB_S + wn * (BN / 2) + j * 32 + li];
    };
    lds_ab(0, a[0], b[0]);
#pragma unroll
    for (int st = 0; st < BK / 2; ++st) {
      if (st + 1 < BK / 2) lds_ab(2 * (st + 1), a[(st + 1) & 1], b[(st + 1) & 1]);
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[st & 1][i], b[st & 1][j], acc[i][j], 0, 0, 0);
      __builtin_amdgcn_sched_group_barrier(0x100, TM + TN, 0);   // the DS reads of the next pair first ...
      __builtin_amdgcn_sched_group_barrier(0x008, TM * TN, 0);   // ... then this pair's MFMAs
    }
  }

  if (do_csum && tid / BM < CS && m0 + tid % BM < g.M) atomicAdd(g.colsum + m0 + tid % BM, csum);
  // epilogue: C/D layout col = lane&31, row = (reg&3) + 8*(reg>>2) + 4*(lane>>5)
  const bool atomic = nz > 1;
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j) {
      const int n = n0 + wn * (BN / 2) + j * 32 + li;
      if (n >= g.N) continue;
      const float bv = (g.bias != nullptr && bz == 0) ? g.bias[n] : 0.f;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int m = m0 + wm * (BM / 2) + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
        if (m >= g.M) continue;
        float v = acc[i][j][r] + bv;
        if (g.act == 1) v = v > 0.f ? v : 0.f;
        else if (g.act == 2) v = v > 0.f ? v : v * g.slope;
        if (g.gate != nullptr) v *= (g.gate[(size_t)m * g.ldg + n] > 0.f) ? 1.f : g.slope;
        float* cp = g.C + (size_t)m * g.ldc + n;
        if (atomic) atomicAdd(cp, v);
        else if (g.accumulate) *cp += v;
        else *cp = v;
      }
    }
}

template <int BM, int BN, int OPA, int OPB>
__global__ __launch_bounds__(256) void gemm_kernel(GemmArgs g) {
  gemm_tile<BM, BN, OPA, OPB>(g, blockIdx.x, blockIdx.y, blockIdx.z, gridDim.z);
}

// ---- weight gradients: dW[M, N] (+)= D^T Act with D [rows, M] and Act [rows, N] both row-major (op_a = op_b = 1) ----------------
// Both operands keep the reduction (rows) as their slow index, so the k-major LDS image of a 128-wide tile IS the global layout: one
// contiguous 512-byte row per k.  The tile is filled by LDS-DMA (global_load_lds_dwordx4: no staging VGPRs, no ds_write pass, no
// transposition) into a ring of WST stages of WBK rows held in ONE __shared__ array (a second LDS object can make hipcc wait for
// every DMA before the first ds_read of a k-step).  Per k-step: a counted vmcnt retires this wave's DMAs of stage s, a raw s_barrier
// (no __syncthreads: its fence would drain the DMAs still in flight) makes every wave's stage s visible and retires every read of
// stage s - 1, then the DMAs of stage s + WST - 1 go into the slot of s - 1 and the MFMAs consume stage s.  Reads are conflict-free
// ds_read_b32: lanes 0-31 read 32 consecutive floats of row k, lanes 32-63 row k + 1 (the other lane group of the instruction).
// Two bodies share everything but the fragment gather and the MFMA block:
//  * SLICED = false: the exact fp32 chain on v_mfma_f32_32x32x2_f32 in gemm_tile's k order, so an unsplit launch matches gemm_tile
//    bit for bit.  It serves the unsplit (split_k == 1, deterministic) launches of gemm_f32.
//  * SLICED = true: every operand is split in registers into three bf16 slices (bf16_slice.h: x = hi + mid + lo exactly) and a
//    16-row stage of a 32 x 32 output is six v_mfma_f32_32x32x16_bf16 with fp32 accumulation instead of eight fp32 MFMAs of twice
//    the cycles each.  Term order per stage and output tile (0 = hi, 1 = mid, 2 = lo):
//        a0 b0, a0 b1, a1 b0, a0 b2, a1 b1, a2 b0
//    a1 b2, a2 b1, a2 b2 (each < 2^-22 of the product, 2^-24 in all on average) are dropped.  The six go into ONE accumulator that
//    starts from zero in every stage, and the stage's sum is added to the running sum with fp32 VALU adds: every update of the
//    bf16 MFMA's accumulator errs toward minus infinity by ~0.015 ulp of the accumulator, which on a running sum over the whole k
//    range is a one-signed error that grows with it (measured) and on a 16-row sum is 3e-8 of the result.  The
//    tiles of a wave go one after the other, so one stage sum (16 registers) is live beside the MFMAs of the next.  The k
//    grouping differs from gemm_tile's, so results agree with it to rounding, not bit for bit; an infinite operand gives NaN.
//    The grouped launch and gemm_f32 with split_k != 1 take this body.
// Requirements (host-checked; others take gemm_tile): 16-byte aligned operands, M, N, ldd, lda multiples of 4.  Columns past M / N
// are staged from a clamped (valid) column and never stored; rows past the k range are staged from a clamped row and zeroed at read.
constexpr int WBM = 128, WBK = 16;         // square tile, k rows per stage
constexpr int WST = 4;                      // ring depth: 4 x 16 KiB = 64 KiB -> 2 workgroups (2 waves per SIMD) per CU
                                            // (3 stages, 3 workgroups per CU, measured: chain group 707 -> 774 us)
constexpr int WDMA = 4;                     // DMA instructions per wave per stage (2 for D, 2 for Act: 2 rows of 512 B each)

template <int N>
__device__ __forceinline__ void wait_vm() { asm volatile("s_waitcnt vmcnt(%0)" ::"I"(N) : "memory"); }
__device__ __forceinline__ void ring_barrier() {  // (the LDS reads of the stage before are retired first: its slot is refilled next)
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();
  asm volatile("" ::: "memory");
}

typedef __bf16 wg_bf16x8 __attribute__((ext_vector_type(8)));
typedef uint32_t wg_u32x4 __attribute__((ext_vector_type(4)));

template <bool SLICED>
__device__ __forceinline__ void wgrad_tile(const GemmArgs& g, const int bx, const int by, const int bz, const int nz) {
  constexpr int SLOT = 2 * WBK * WBM;  // floats per stage: D rows then Act rows
  __shared__ __attribute__((aligned(16))) float ring[WST * SLOT];

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave >> 1, wn = wave & 1;
  const int m0 = by * WBM, n0 = bx * WBM;
  const int kbeg = bz * g.k_per_split;
  const int kend = min(g.K, kbeg + g.k_per_split);
  const int nst = (kend - kbeg + WBK - 1) / WBK;  // >= 1: the host launches no empty k range

  // DMA source of this lane: column (lane & 31) * 4 of the tile, row 2 r + (lane >> 5) of instruction r (r = 2 wave + j)
  const int lr = lane >> 5, lc = (lane & 31) * 4;
  const float* pa = g.A + min(m0 + lc, g.M - 4);
  const float* pb = g.B + min(n0 + lc, g.N - 4);
  auto issue = [&](int s) {
    float* sa = ring + (s % WST) * SLOT;
    float* sb = sa + WBK * WBM;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int r = (wave * 2 + j) * 2;  // first of the instruction's two k rows (wave-uniform)
      const size_t k = (size_t)min(kbeg + s * WBK + r + lr, kend - 1);
      __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(pa + k * g.lda),
                                       (__attribute__((address_space(3))) void*)(sa + r * WBM), 16, 0, 0);
      __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(pb + k * g.ldb),
                                       (__attribute__((address_space(3))) void*)(sb + r * WBM), 16, 0, 0);
    }
  };

  f32x16 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  const int li = lane & 31, lh = lane >> 5;
  const bool do_csum = g.colsum != nullptr && bx == 0;  // bias gradient: the first column block also sums its D tiles over k
  float csum = 0.f;

#pragma unroll
  for (int s = 0; s < WST - 1; ++s)
    if (s < nst) issue(s);
  auto advance = [&](int s) -> const float* {
    // this wave's DMAs of stage s have landed once at most WST - 2 younger stages are outstanding (none near the end)
    if (s + WST - 2 < nst) wait_vm<WDMA * (WST - 2)>();
    else wait_vm<0>();
    ring_barrier();  // every wave's stage s is in LDS; every wave has finished reading stage s - 1
    if (s + WST - 1 < nst) issue(s + WST - 1);  // into the slot of stage s - 1
    return ring + (s % WST) * SLOT;
  };
  const int nfull = (kend - kbeg) / WBK;
  if constexpr (SLICED) {
    // Lane l holds row l & 31 and the 8 consecutive k from 8 (l >> 5) of a 32x32x16 fragment: eight ds_read_b32 down one LDS column
    // per fragment (32 lanes read 32 consecutive floats of a row: conflict-free), 32 per stage as in the exact body.  The raw
    // values of stage s + 1 are requested BEFORE the MFMAs of stage s (its barrier, DMA issue and LDS round trip run under them)
    // and sliced after them, over the fragments they have consumed: one set of fragment registers, no copies.
    float ra[2][8], rb[2][8];
    // MASK: the last stage of a ragged k range — rows >= nv are clamped copies and enter as zeros, before slicing
    auto gather = [&](const float* sa, auto mask_tag, int nv) {
      constexpr bool MASK = decltype(mask_tag)::value;
      const float* sb = sa + WBK * WBM;
      if (do_csum) {  // 2 threads per column, 8 rows each: the bias gradient stays an fp32 sum of the unsliced values
#pragma unroll
        for (int kk = 0; kk < WBK / 2; ++kk) {
          const int k = kk * 2 + (tid >> 7);
          const float v = sa[k * WBM + (tid & 127)];
          csum += (!MASK || k < nv) ? v : 0.f;
        }
      }
#pragma unroll
      for (int q = 0; q < 8; ++q) {
        const int k = 8 * lh + q;
        const bool ok = !MASK || k < nv;
#pragma unroll
        for (int i = 0; i < 2; ++i) {
          const float va = sa[k * WBM + wm * 64 + i * 32 + li], vb = sb[k * WBM + wn * 64 + i * 32 + li];
          ra[i][q] = ok ? va : 0.f;
          rb[i][q] = ok ? vb : 0.f;
        }
      }
    };
    auto fetch = [&](int s) {
      const float* sa = advance(s);
      if (s < nfull) gather(sa, std::false_type{}, WBK);
      else gather(sa, std::true_type{}, kend - kbeg - nfull * WBK);
    };
    auto slice = [&](const float (&r)[8], wg_bf16x8 (&f)[3]) {
      Slices3 c[8];
#pragma unroll
      for (int q = 0; q < 8; ++q) c[q] = slice3(r[q]);
      wg_u32x4 h, m, l;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        h[q] = slice_pack(c[2 * q].hi, c[2 * q + 1].hi);
        m[q] = slice_pack(c[2 * q].mid, c[2 * q + 1].mid);
        l[q] = slice_pack(c[2 * q].lo, c[2 * q + 1].lo);
      }
      f[0] = __builtin_bit_cast(wg_bf16x8, h);
      f[1] = __builtin_bit_cast(wg_bf16x8, m);
      f[2] = __builtin_bit_cast(wg_bf16x8, l);
    };
    wg_bf16x8 fa[2][3], fb[2][3];
    auto slice_all = [&]() {
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        slice(ra[i], fa[i]);
        slice(rb[i], fb[i]);
      }
    };
    fetch(0);
    slice_all();
    for (int s = 0; s < nst; ++s) {
      if (s + 1 < nst) fetch(s + 1);
      constexpr int TA[6] = {0, 0, 1, 0, 1, 2}, TB[6] = {0, 1, 0, 2, 1, 0};  // a0 b0, a0 b1, a1 b0, a0 b2, a1 b1, a2 b0
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          f32x16 part;
#pragma unroll
          for (int r = 0; r < 16; ++r) part[r] = 0.f;
#pragma unroll
          for (int t = 0; t < 6; ++t) part = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[i][TA[t]], fb[j][TB[t]], part, 0, 0, 0);
          acc[i][j] += part;  // fp32 VALU adds, round to nearest even
        }
      if (s + 1 < nst) slice_all();  // the next stage's fragments over the ones just consumed
    }
  } else {
    // one stage: 8 k-pairs x 2 x 2 MFMAs; the operands of pair p + 1 are requested before the MFMAs of pair p (as in gemm_tile).
    // MASK: the last stage of a ragged k range — rows >= nv are clamped copies and enter as zeros
    auto stage = [&](const float* sa, auto mask_tag, int nv) {
      constexpr bool MASK = decltype(mask_tag)::value;
      const float* sb = sa + WBK * WBM;
      if (do_csum) {  // 2 threads per column, 8 rows each
#pragma unroll
        for (int kk = 0; kk < WBK / 2; ++kk) {
          const int k = kk * 2 + (tid >> 7);
          const float v = sa[k * WBM + (tid & 127)];
          csum += (!MASK || k < nv) ? v : 0.f;
        }
      }
      float a[2][2], b[2][2];
      auto lds_ab = [&](int kk, float (&a_)[2], float (&b_)[2]) {
        const bool ok = !MASK || kk + lh < nv;
#pragma unroll
        for (int i = 0; i < 2; ++i) {
          const float v = sa[(kk + lh) * WBM + wm * 64 + i * 32 + li];
          a_[i] = ok ? v : 0.f;
        }
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          const float v = sb[(kk + lh) * WBM + wn * 64 + j * 32 + li];
          b_[j] = ok ? v : 0.f;
        }
      };
      lds_ab(0, a[0], b[0]);
#pragma unroll
      for (int p = 0; p < WBK / 2; ++p) {
        if (p + 1 < WBK / 2) lds_ab(2 * (p + 1), a[(p + 1) & 1], b[(p + 1) & 1]);
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
          for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[p & 1][i], b[p & 1][j], acc[i][j], 0, 0, 0);
        __builtin_amdgcn_sched_group_barrier(0x100, 4, 0);
        __builtin_amdgcn_sched_group_barrier(0x008, 4, 0);
      }
    };

    // the ragged last stage is peeled: a masked stage inside the loop makes the compiler shuttle the accumulators between register
    // files on every k-step
    for (int s = 0; s < nfull; ++s) stage(advance(s), std::false_type{}, WBK);
    if (nfull < nst) stage(advance(nfull), std::true_type{}, kend - kbeg - nfull * WBK);
  }

  if (do_csum && m0 + (tid & 127) < g.M) atomicAdd(g.colsum + m0 + (tid & 127), csum);
  // epilogue: C/D layout col = lane&31, row = (reg&3) + 8*(reg>>2) + 4*(lane>>5); rows / columns past M / N are dropped
  const bool atomic = nz > 1;
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int n = n0 + wn * 64 + j * 32 + li;
      if (n >= g.N) continue;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int m = m0 + wm * 64 + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
        if (m >= g.M) continue;
        float* cp = g.C + (size_t)m * g.ldc + n;
        if (atomic) atomicAdd(cp, acc[i][j][r]);
        else if (g.accumulate) *cp += acc[i][j][r];
        else *cp = acc[i][j][r];
      }
    }
}

// ---- grouped weight gradients --------------------------------------------------------------------------------------------------
// Up to kMaxGroup problems dW_p (+)= D_p^T Act_p of ONE reduction length K (the rows of a sequence) as one launch on wgrad_tile: the
// small ones (256 x 256 outputs: 4 tiles) cannot fill 256 CUs on their own without a split so fine that a workgroup's k range is a
// few stages and many workgroups contend for every output word.  Together they are ~100 tiles: a coarse split, long k ranges, one
// launch.  Work item = (problem, split, tile); first[p] = first work item of problem p (first[n] = all); a workgroup finds its
// problem by scanning that table.
constexpr int kMaxGroup = 20;
struct GemmGroup {
  GemmArgs p[kMaxGroup];
  int first[kMaxGroup + 1];
  int n, split;
};
// (amdgpu_waves_per_eu(2): the ring's 64 KiB allow two workgroups per CU; without the hint hipcc interleaves the four tiles' stage
// sums and takes 234 VGPRs + 64 AGPRs, one workgroup per CU.  With it the sliced body takes 248 of the 256 registers two workgroups
// allow: no headroom, one more live value spills or halves the occupancy)
// WGRAD_SCALAR_ADDS: the two sliced kernels are compiled without packed fp32 VALU, so that `acc[i][j] += part` is 16 v_add_f32 per
// tile and not 8 v_pk_add_f32, the form the backend gives a vector add by default: beside MFMAs a packed add costs the issue port
// several plain ones.  Same add, same order, same bits; still 248 VGPRs, no scratch, two workgroups per CU, and no v_pk_add_f32
// left in either kernel.  Measured (tools/wgrad_tile_bench.py groups, MI355X, packed -> scalar, three alternated rounds): the VRNN
// chain group 614 .. 627 -> 551 .. 561 us, the decoder group 166 .. 172 -> 162 .. 163 us.  The attribute sits on the kernels whose
// whole body is that loop; every other kernel of the file keeps the packed forms.
#if defined(__HIP_DEVICE_COMPILE__)
#define WGRAD_SCALAR_ADDS __attribute__((target("no-packed-fp32-ops")))
#else
#define WGRAD_SCALAR_ADDS  // (the host pass knows no such feature)
#endif
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2))) WGRAD_SCALAR_ADDS void wgrad_group_kernel(GemmGroup gg) {
  const int item = blockIdx.x;
  int p = 0;
  while (p + 1 < gg.n && item >= gg.first[p + 1]) ++p;
  const GemmArgs g = gg.p[p];
  const int local = item - gg.first[p];
  const int tiles_n = (g.N + WBM - 1) / WBM, tiles = tiles_n * ((g.M + WBM - 1) / WBM);
  const int bz = local / tiles, t = local - bz * tiles;
  wgrad_tile<true>(g, t % tiles_n, t / tiles_n, bz, gg.split);
}

// the same work items on the register-staged 64 x 64 tile: groups whose outputs would leave much of a 128 x 128 tile as padding
__global__ __launch_bounds__(256) void gemm_group_kernel(GemmGroup gg) {
  const int item = blockIdx.x;
  int p = 0;
  while (p + 1 < gg.n && item >= gg.first[p + 1]) ++p;
  const GemmArgs g = gg.p[p];
  const int local = item - gg.first[p];
  const int tiles_n = (g.N + 63) / 64, tiles = tiles_n * ((g.M + 63) / 64);
  const int bz = local / tiles, t = local - bz * tiles;
  gemm_tile<64, 64, 1, 1>(g, t % tiles_n, t / tiles_n, bz, gg.split);
}

__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2))) WGRAD_SCALAR_ADDS void wgrad_kernel(GemmArgs g) {
  wgrad_tile<true>(g, blockIdx.x, blockIdx.y, blockIdx.z, gridDim.z);
}
__global__ __launch_bounds__(256) void wgrad_exact_kernel(GemmArgs g) {  // unsplit requests of gemm_f32
  wgrad_tile<false>(g, blockIdx.x, blockIdx.y, blockIdx.z, gridDim.z);
}

// ---- 16-bit operand variant (operand_type() OP_BF16 / OP_F16: the reference's --use_amp regime) ----------------------------------
// Same tiling, arguments and epilogue; the global -> LDS stage rounds both operands to bf16 / fp16 (OT; nearest even) and lays them
// out k-group-major — element (m, k) at ((k / 8) * LD + m) * 8 + k % 8 — so that the 8 consecutive k a lane feeds
// v_mfma_f32_32x32x16_bf16 / _f16 (gfx950's full-rate forms, same cycles) are one ds_read_b128.  BK = 32: two MFMAs per 32x32 tile
// and staged k-tile (16x the fp32 pipe's rate, so this kernel is bound by the operand stream: what it buys is the matrix pipe's
// time).  Accumulation and epilogue are fp32.
constexpr int BKB = 32;
typedef __bf16 bf16x8_t __attribute__((ext_vector_type(8)));
typedef _Float16 f16x8_t __attribute__((ext_vector_type(8)));
typedef float f2_t __attribute__((ext_vector_type(2)));
typedef __bf16 b2_t __attribute__((ext_vector_type(2)));
typedef _Float16 h2_t __attribute__((ext_vector_type(2)));
template <int OT>  // v_cvt_pk_bf16_f32 / v_cvt_pk_f16_f32 (nearest even; fp16: |x| >= 65520 -> inf, as torch's .half())
__device__ __forceinline__ unsigned pk2(float a, float b) {
  if constexpr (OT == OP_F16) return __builtin_bit_cast(unsigned, __builtin_convertvector((f2_t){a, b}, h2_t));
  else return __builtin_bit_cast(unsigned, __builtin_convertvector((f2_t){a, b}, b2_t));
}

template <int BM, int BN, int OPA, int OPB, int OT>
__global__ __launch_bounds__(256) void gemm_bf16_kernel(GemmArgs g) {
  constexpr int LDA_S = BM + PAD, LDB_S = BN + PAD;
  constexpr int TM = BM / 64, TN = BN / 64;
  constexpr int KVB = BKB / 4;
  constexpr int A_V = BM * BKB / 4 / 256;  // float4 per thread per stage (2, 4 or 6)
  constexpr int B_V = BN * BKB / 4 / 256;
  static_assert(A_V % 2 == 0 && B_V % 2 == 0, "pairs of k rows");
  __shared__ __attribute__((aligned(16))) unsigned short As[(BKB / 8) * LDA_S * 8];
  __shared__ __attribute__((aligned(16))) unsigned short Bs[(BKB / 8) * LDB_S * 8];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int m0 = blockIdx.y * BM, n0 = blockIdx.x * BN;
  const int kbeg = blockIdx.z * g.k_per_split;
  const int kend = min(g.K, kbeg + g.k_per_split);

  f32x16 acc[TM][TN];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  float4 ra[A_V], rb[B_V];
  // operand X (rows of length `ext` along m or n): OP == 0: X[row][k], a thread holds 4 consecutive k of one row;
  // OP == 1: X[k][row], a thread holds 4 consecutive rows of k rows 2p and 2p + 1 (items v, v + 1)
  auto load_op = [&](auto op_tag, const float* X, int ldx, int ext, int base, bool vec, int BT, float4* r, int NV, int k0) {
    constexpr int OP = decltype(op_tag)::value;
#pragma unroll
    for (int v = 0; v < NV; ++v) {
      if (OP == 0) {
        const int id = tid + v * 256;
        const int m = id / KVB, k4 = (id % KVB) * 4;
        const int gm = base + m, gk = k0 + k4;
        const int nv = (gm < ext) ? max(0, min(4, kend - gk)) : 0;
        r[v] = ld4(X + (size_t)(gm < ext ? gm : 0) * ldx + gk, nv, vec);
      } else {
        const int id = tid + (v >> 1) * 256;
        const int k = 2 * (id / (BT / 4)) + (v & 1), m4 = (id % (BT / 4)) * 4;
        const int gm = base + m4, gk = k0 + k;
        const int nv = (gk < kend) ? max(0, min(4, ext - gm)) : 0;
        r[v] = ld4(X + (size_t)(gk < kend ? gk : 0) * ldx + gm, nv, vec);
      }
    }
  };
  auto store_op = [&](auto op_tag, unsigned short* S, int LD, int BT, const float4* r, int NV) {
    constexpr int OP = decltype(op_tag)::value;
#pragma unroll
    for (int v = 0; v < NV; ++v) {
      if (OP == 0) {
        const int id = tid + v * 256;
        const int m = id / KVB, k4 = (id % KVB) * 4;
        uint2 q;
        q.x = pk2<OT>(r[v].x, r[v].y); q.y = pk2<OT>(r[v].z, r[v].w);
        *reinterpret_cast<uint2*>(&S[((k4 >> 3) * LD + m) * 8 + (k4 & 7)]) = q;
      } else if ((v & 1) == 0) {
        const int id = tid + (v >> 1) * 256;
        const int k = 2 * (id / (BT / 4)), m4 = (id % (BT / 4)) * 4;
        unsigned short* d = &S[((k >> 3) * LD + m4) * 8 + (k & 7)];
        *reinterpret_cast<unsigned*>(d + 0) = pk2<OT>(r[v].x, r[v + 1].x);
        *reinterpret_cast<unsigned*>(d + 8) = pk2<OT>(r[v].y, r[v + 1].y);
        *reinterpret_cast<unsigned*>(d + 16) = pk2<OT>(r[v].z, r[v + 1].z);
        *reinterpret_cast<unsigned*>(d + 24) = pk2<OT>(r[v].w, r[v + 1].w);
      }
    }
  };
  using OA = std::integral_constant<int, OPA>;
  using OB = std::integral_constant<int, OPB>;
  auto load_tiles = [&](int k0) {
    load_op(OA{}, g.A, g.lda, g.M, m0, g.a_vec != 0, BM, ra, A_V, k0);
    load_op(OB{}, g.B, g.ldb, g.N, n0, g.b_vec != 0, BN, rb, B_V, k0);
  };
  auto store_tiles = [&]() {
    store_op(OA{}, As, LDA_S, BM, ra, A_V);
    store_op(OB{}, Bs, LDB_S, BN, rb, B_V);
  };

  if (kbeg < kend) load_tiles(kbeg);
  const int li = lane & 31, lh = lane >> 5;
  for (int k0 = kbeg; k0 < kend; k0 += BKB) {
    __syncthreads();
    store_tiles();
    __syncthreads();
    if (k0 + BKB < kend) load_tiles(k0 + BKB);
#pragma unroll
    for (int st = 0; st < BKB / 16; ++st) {
      bf16x8_t a[TM], b[TN];
#pragma unroll
      for (int i = 0; i < TM; ++i) a[i] = *reinterpret_cast<const bf16x8_t*>(&As[((2 * st + lh) * LDA_S + wm * (BM / 2) + i * 32 + li) * 8]);
#pragma unroll
      for (int j = 0; j < TN; ++j) b[j] = *reinterpret_cast<const bf16x8_t*>(&Bs[((2 * st + lh) * LDB_S + wn * (BN / 2) + j * 32 + li) * 8]);
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j) {
          if constexpr (OT == OP_F16)
            acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8_t, a[i]), __builtin_bit_cast(f16x8_t, b[j]), acc[i][j], 0, 0, 0);
          else acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[i], b[j], acc[i][j], 0, 0, 0);
        }
    }
  }

  const bool atomic = gridDim.z > 1;
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j) {
      const int n = n0 + wn * (BN / 2) + j * 32 + li;
      if (n >= g.N) continue;
      const float bv = (g.bias != nullptr && blockIdx.z == 0) ? g.bias[n] : 0.f;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int m = m0 + wm * (BM / 2) + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
        if (m >= g.M) continue;
        float v = acc[i][j][r] + bv;
        if (g.act == 1) v = v > 0.f ? v : 0.f;
        else if (g.act == 2) v = v > 0.f ? v : v * g.slope;
        if (g.gate != nullptr) v *= (g.gate[(size_t)m * g.ldg + n] > 0.f) ? 1.f : g.slope;
        float* cp = g.C + (size_t)m * g.ldc + n;
        if (atomic) atomicAdd(cp, v);
        else if (g.accumulate) *cp += v;
        else *cp = v;
      }
    }
}

// launches per arm (blvm_gemm_arm_counts; numbering at GemmArm, common.h): counted beside every hipLaunchKernelGGL of K6, keyed by
// the kernel that launch names, never by the routing's answer
std::atomic<unsigned long long> g_arm_count[ARM_COUNT];
constexpr int tile_index(int bm, int bn) { return bm == 64 ? 0 : (bn == 192 ? 2 : (bm == 192 ? 3 : 1)); }
constexpr int staged_arm(int bm, int bn, int ot) { return ARM_STAGED + 3 * tile_index(bm, bn) + ot; }

template <int BM, int BN, int OT>
void launch_gemm16(const GemmArgs& g, int op_a, int op_b, dim3 grid, hipStream_t s) {
  if (op_a == 0 && op_b == 0) hipLaunchKernelGGL((gemm_bf16_kernel<BM, BN, 0, 0, OT>), grid, dim3(256), 0, s, g);
  else if (op_a == 0 && op_b == 1) hipLaunchKernelGGL((gemm_bf16_kernel<BM, BN, 0, 1, OT>), grid, dim3(256), 0, s, g);
  else if (op_a == 1 && op_b == 0) hipLaunchKernelGGL((gemm_bf16_kernel<BM, BN, 1, 0, OT>), grid, dim3(256), 0, s, g);
  else hipLaunchKernelGGL((gemm_bf16_kernel<BM, BN, 1, 1, OT>), grid, dim3(256), 0, s, g);
  gemm_count_arm(staged_arm(BM, BN, OT));
}

template <int BM, int BN>
void launch_gemm(const GemmArgs& g, int op_a, int op_b, dim3 grid, hipStream_t s, OpType ot) {
  if (ot == OP_BF16) return launch_gemm16<BM, BN, OP_BF16>(g, op_a, op_b, grid, s);
  if (ot == OP_F16) return launch_gemm16<BM, BN, OP_F16>(g, op_a, op_b, grid, s);
  if (op_a == 0 && op_b == 0) hipLaunchKernelGGL((gemm_kernel<BM, BN, 0, 0>), grid, dim3(256), 0, s, g);
  else if (op_a == 0 && op_b == 1) hipLaunchKernelGGL((gemm_kernel<BM, BN, 0, 1>), grid, dim3(256), 0, s, g);
  else if (op_a == 1 && op_b == 0) hipLaunchKernelGGL((gemm_kernel<BM, BN, 1, 0>), grid, dim3(256), 0, s, g);
  else hipLaunchKernelGGL((gemm_kernel<BM, BN, 1, 1>), grid, dim3(256), 0, s, g);
  gemm_count_arm(staged_arm(BM, BN, OP_F32));
}

__global__ __launch_bounds__(256) void colsum_kernel(int M, int N, const float* __restrict__ X, int ldx,
                                                     float* __restrict__ out, int rows_per_block) {
  // block (bx, by): columns bx*64.., rows by*rows_per_block..; 4 row-lanes x 64 columns (scalar fallback: any ldx / alignment)
  __shared__ float part[4][64];
  const int c = blockIdx.x * 64 + (threadIdx.x & 63);
  const int rl = threadIdx.x >> 6;
  const int r0 = blockIdx.y * rows_per_block, r1 = min(M, r0 + rows_per_block);
  float s = 0.f;
  if (c < N)
    for (int r = r0 + rl; r < r1; r += 4) s += X[(size_t)r * ldx + c];
  part[rl][threadIdx.x & 63] = s;
  __syncthreads();
  if (rl == 0 && c < N) atomicAdd(out + c, part[0][threadIdx.x] + part[1][threadIdx.x] + part[2][threadIdx.x] + part[3][threadIdx.x]);
}

// 16-byte loads: a lane owns 4 adjacent columns, a wave 256 columns of one row (1 KiB contiguous); 4 row-lanes (waves)
// nmod: the sums of columns c, c + nmod, c + 2 nmod ... land in out[c % nmod] (a dense [M, n] matrix with n % 4 != 0 read as
// [M / g, n g]: g consecutive rows per "row")
__global__ __launch_bounds__(256) void colsum4_kernel(int M, int N, const float* __restrict__ X, int ldx,
                                                      float* __restrict__ out, int rows_per_block, int nmod) {
  __shared__ float part[4][4][64];
  const int lane = threadIdx.x & 63, rl = threadIdx.x >> 6;
  const int c = (blockIdx.x * 64 + lane) * 4;
  const int r0 = blockIdx.y * rows_per_block, r1 = min(M, r0 + rows_per_block);
  float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
  if (c < N) {
#pragma unroll 4
    for (int r = r0 + rl; r < r1; r += 4) {
      const float4 v = *reinterpret_cast<const float4*>(X + (size_t)r * ldx + c);
      s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w;
    }
  }
  part[rl][0][lane] = s.x; part[rl][1][lane] = s.y; part[rl][2][lane] = s.z; part[rl][3][lane] = s.w;
  __syncthreads();
  if (rl == 0 && c < N) {
#pragma unroll
    for (int q = 0; q < 4; ++q) atomicAdd(out + (c + q) % nmod, part[0][q][lane] + part[1][q][lane] + part[2][q][lane] + part[3][q][lane]);
  }
}

__global__ __launch_bounds__(256) void act_bwd_kernel(const float* dy, const float* y, float slope, float* dz, size_t n4,
                                                      size_t n) {
  // 16 bytes per lane, grid-stride
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (size_t)gridDim.x * 256) {
    const float4 g = reinterpret_cast<const float4*>(dy)[i];
    const float4 v = reinterpret_cast<const float4*>(y)[i];
    float4 o;
    o.x = v.x > 0.f ? g.x : g.x * slope;
    o.y = v.y > 0.f ? g.y : g.y * slope;
    o.z = v.z > 0.f ? g.z : g.z * slope;
    o.w = v.w > 0.f ? g.w : g.w * slope;
    reinterpret_cast<float4*>(dz)[i] = o;
  }
  if (blockIdx.x == 0) {
    const size_t i = n4 * 4 + threadIdx.x;
    if (i < n) dz[i] = y[i] > 0.f ? dy[i] : dy[i] * slope;
  }
}

__global__ __launch_bounds__(256) void transpose_kernel(int M, int N, const float* __restrict__ X, int ldx,
                                                        float* __restrict__ out, int ldo) {
  __shared__ float t[32][33];
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;  // 32 x 8
  const int m0 = blockIdx.y * 32, n0 = blockIdx.x * 32;
  for (int i = ty; i < 32; i += 8)
    if (m0 + i < M && n0 + tx < N) t[i][tx] = X[(size_t)(m0 + i) * ldx + n0 + tx];
  __syncthreads();
  for (int i = ty; i < 32; i += 8)
    if (n0 + i < N && m0 + tx < M) out[(size_t)(n0 + i) * ldo + m0 + tx] = t[tx][i];
}

// ---- wgrad_tile host side ----
// operands it can stage by 16-byte DMA (and clamp inside a row), and reductions long enough to pipeline
bool wgrad_fits(uintptr_t d_addr, int ldd, int M, uintptr_t act_addr, int lda, int N, int K) {
  return (d_addr & 15u) == 0 && (act_addr & 15u) == 0 && ldd % 4 == 0 && lda % 4 == 0 && M % 4 == 0 && N % 4 == 0 && K >= 1024;
}
int wgrad_tiles(int M, int N) { return ((M + WBM - 1) / WBM) * ((N + WBM - 1) / WBM); }
// k splits over `tiles` output tiles: as many as keep every workgroup in the first wave (the workgroups per CU that the ring's LDS
// allows: 2 at 64 KiB), k ranges of at least 32 stages (512 rows)
int wgrad_split(long tiles, int K) {
  static const int cus = [] {
    int dev = 0, n = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) n = 0;
    return n > 0 ? n : 256;
  }();
  long split = (160 / (WST * 16)) * (long)cus / std::max(1L, tiles);
  split = std::min<long>(split, K / (32 * WBK));
  return (int)std::max(1L, split);
}
int wgrad_k_per_split(int K, int split) {
  const int ksteps = (K + WBK - 1) / WBK;
  return ((ksteps + split - 1) / split) * WBK;
}
// The sliced body is the faster one wherever both were measured (tools/wgrad_tile_bench.py on MI355X, us, exact -> sliced): the VRNN
// chain group 704 -> 624 (ragged rows 705 -> 629), a 256 x 512 + 2 x 256 x 256 group 85.1 -> 76.2, 1536 x 512 x 16000 215 -> 182,
// 384 x 192 x 49152 88.8 -> 77.3, 256 x 256 x 64000 83.0 -> 72.4, 768 x 192 x 393216 1194 -> 1061.  Only a request for NO split keeps
// the exact body: it asks for a reproducible result, the 64 x 64 tile's bits.  (Those figures are with packed accumulator adds; with
// WGRAD_SCALAR_ADDS the sliced body gives: chain group 551 .. 561, ragged rows 566 .. 573, the decoder's 3-job group 162 .. 164,
// 1536 x 512 x 16000 168, 256 x 256 x 64000 74.  A second sliced body on 64 x 128 wave tiles, one workgroup per CU, was built and
// measured slower at all of these -- chain group 630 .. 641, 1536 x 512 x 16000 179 .. 188 -- and is not here: DESIGN.md §0.)

}  // namespace

void gemm_count_arm(int arm) { g_arm_count[arm].fetch_add(1, std::memory_order_relaxed); }
int gemm_force_tile() {  // BLVM_GEMM_TILE, experiments only: 1 the 64 x 64 tile, 2 no 128 x 192, 3 no weight-stationary path
  static const int force_tile = [] { const char* e = getenv("BLVM_GEMM_TILE"); return e ? atoi(e) : 0; }();
  return force_tile;
}

// Which kernel gemm_f32 launches for a request: host arithmetic only, and the ONE place where the choice is made -- gemm_f32 asks
// this function and launches what it answers (exported as blvm_gemm_arm; tests/test_gemm_arms_cpu.py walks its conditions).
int gemm_arm(int op_a, int op_b, int M, int N, int K, uintptr_t a_addr, int lda, uintptr_t b_addr, int ldb, int split_k, bool has_bias,
             int act, bool has_gate, bool has_colsum, int operand, int min_rows, int force_tile) {
  if (M <= 0 || N <= 0) return ARM_COUNT;  // nothing is launched
  if (split_k < 1) split_k = 1;
  // weight-gradient form (both operands [rows, features]) on wgrad_tile where it fits and measured faster than the 64 x 64 tile
  // (tools/wgrad_tile_bench.py on MI355X, split as the callers request it; us, 64 x 64 -> wgrad_tile):
  //   1536 x 512 x 16000  257 -> 215      768 x 192 x 393216  1451 -> 1203      384 x 192 x 49152  94.0 -> 88.9
  //   256 x 256 x 64000  92.5 -> 83.5     256 x 256 x 16000   36.4 -> 44.1      768 x 256 x 16000  72.0 -> 75.7
  //   192 x 192 x 98304  89.7 -> 108
  // i.e. large outputs, or long reductions on outputs whose 128-wide tiles are not mostly padding.  split_k == 1 stays unsplit
  // (deterministic); any other request takes the body's own split.
  const bool wgrad_wins = (long)M * N >= 512L * 512 || (K >= 32768 && std::max(M, N) >= 256);
  if (op_a == 1 && op_b == 1 && operand == OP_F32 && act == 0 && !has_gate && !has_bias && wgrad_wins &&
      wgrad_fits(a_addr, lda, M, b_addr, ldb, N, K)) {
    // a request for no split asks for a reproducible result: the exact fp32 body, bit-identical to the 64 x 64 tile.  That includes
    // the callers that pass gemm_pick_split() where it returns 1 (outputs of >= 768 64 x 64 tiles, e.g. 2048 x 2048)
    return split_k != 1 ? ARM_WGRAD_SLICED : ARM_WGRAD_EXACT;
  }
  // forward / data-gradient forms with a short reduction and many rows: the weight-stationary path (gemm_ws.hip; the routing
  // table is at gemm_ws_route).  BLVM_GEMM_TILE=3 keeps them on the staged tiles (A/B runs of one library).
  if (force_tile != 3 && gemm_ws_route(op_a, M, N, K, a_addr, lda, split_k, has_colsum, operand, min_rows)) return ARM_WS;
  // (the tile count takes the split as requested, before gemm_f32 clamps it to the k-tiles there are)
  bool big = (M >= 128 && N >= 128 && (size_t)((M + 127) / 128) * ((N + 127) / 128) * split_k >= 192);
  // 192-wide tiles for the conv coders' channel counts (192 = 1.5 x 128 would waste a quarter of a 128-tile pair and
  // re-read the other operand): N % 192 == 0 -> 128x192, else M % 192 == 0 -> 192x128
  // Measured on MI355X (tools/gemm_bench.py, tools/gemm_cw.py with BLVM_GEMM_TILE forcing each variant): of the register-staged
  // tiles the 64x64 one wins for every weight-gradient form (76 -> 91 TF/s at 768x192x4e5, 71 -> 91 at 1536x512x16000; those that
  // wgrad_tile takes left above)
  // and for short reductions on narrow outputs (K <= 256 and N <= 256: 43 -> 65 TF/s at K = 96, 53 -> 61 at 256x256); the
  // 128-wide tiles win once N >= 512 or K >= 512 (84 vs 74 TF/s at N = 768, K = 192; 114 vs 95 at 4096^3).
  if ((op_a == 1 && op_b == 1) || (K <= 256 && N <= 256)) big = false;
  if (force_tile == 1) big = false;
  const bool n192 = big && N % 192 == 0 && N % 128 != 0 && force_tile != 2;
  const bool m192 = big && !n192 && M % 192 == 0 && M % 128 != 0;
  // (128 x 64 tiles for narrow outputs whose 128 x 128 tiles are fewer than two per CU, measured r03: dec L1 forward 89 -> 85 us, dec L3
  // dgrad unchanged, the VRNN step within noise: not worth a fourth tile shape)
  return ARM_STAGED + 3 * (big ? (n192 ? 2 : (m192 ? 3 : 1)) : 0) + operand;
}

// The grouped entry point's choice, per job and for the group (host arithmetic only; exported as blvm_wgrad_group_route):
// fits[i] = 1 for the jobs wgrad_tile can take (at most kMaxGroup of them); two or more of those run as ONE launch, on
// wgrad_group_kernel or, where their 128 x 128 tiles would be mostly padding, on gemm_group_kernel -- the arm returned.  ARM_COUNT:
// no grouped launch (fewer than two fit); then, as every job with fits[i] == 0, those jobs go through gemm_f32 one by one.
int wgrad_group_route(const WgradJob* jobs, int njobs, int K, int operand, int* fits) {
  int ntake = 0;
  long tiles = 0, area = 0;
  for (int i = 0; i < njobs; ++i) {
    const WgradJob& j = jobs[i];
    fits[i] = 0;
    if (!j.dW) continue;
    if (operand == OP_F32 && wgrad_fits(reinterpret_cast<uintptr_t>(j.D), j.ldd, j.M, reinterpret_cast<uintptr_t>(j.Act), j.lda, j.N, K) &&
        ntake < kMaxGroup) {
      fits[i] = 1;
      ++ntake;
      tiles += wgrad_tiles(j.M, j.N);
      area += (long)j.M * j.N;
    }
  }
  if (ntake < 2) return ARM_COUNT;
  // wgrad_tile unless its tiles would be mostly padding.  Measured (tools/wgrad_tile_bench.py, us, 64 x 64 group -> wgrad_tile): the
  // VRNN chain (16 jobs, 164 full tiles) 920 -> 766, a 256 x 512 + 2 x 256 x 256 group 94.5 -> 85.6, but a 256 x 64 + 2 x 256 x 256
  // group (90 % of its tile area used) 66.2 -> 79.5, and STCN's narrow latent MLPs 31.84 -> 32.32 ms/step
  return area * 100 >= tiles * WBM * WBM * 95L ? ARM_WGRAD_GROUP : ARM_GEMM_GROUP;
}

int gemm_f32(int op_a, int op_b, int M, int N, int K, const float* A, int lda, const float* B, int ldb, float* C,
             int ldc, const float* bias, int act, float slope, const float* gate, int ldg, int accumulate,
             int split_k, hipStream_t stream, float* colsum) {
  BLVM_REQUIRE(M >= 0 && N >= 0 && K >= 0, "gemm: negative dimension");
  if (M == 0 || N == 0) return BLVM_OK;
  BLVM_REQUIRE(A && B && C, "gemm: null operand");
  BLVM_REQUIRE(act >= 0 && act <= 2, "gemm: unknown activation %d", act);
  BLVM_REQUIRE(lda >= (op_a ? M : K) && ldb >= (op_b ? N : K) && ldc >= N, "gemm: leading dimension too small");
  GemmArgs g;
  g.A = A; g.B = B; g.C = C; g.bias = bias; g.gate = gate;
  g.M = M; g.N = N; g.K = K; g.lda = lda; g.ldb = ldb; g.ldc = ldc; g.ldg = ldg;
  g.act = act; g.slope = slope; g.accumulate = accumulate;
  g.a_vec = aligned16(A) && (lda % 4 == 0);
  g.b_vec = aligned16(B) && (ldb % 4 == 0);
  if (split_k < 1) split_k = 1;
  const OpType ot = operand_type();
  const int arm = gemm_arm(op_a, op_b, M, N, K, reinterpret_cast<uintptr_t>(A), lda, reinterpret_cast<uintptr_t>(B), ldb, split_k,
                           bias != nullptr, act, gate != nullptr, colsum != nullptr, ot, gemm_ws_min_rows(), gemm_force_tile());
  if (arm == ARM_WGRAD_EXACT || arm == ARM_WGRAD_SLICED) {
    g.colsum = colsum;
    const int split = arm == ARM_WGRAD_EXACT ? 1 : wgrad_split(wgrad_tiles(M, N), K);
    g.k_per_split = wgrad_k_per_split(K, split);
    const int nz = (K + g.k_per_split - 1) / g.k_per_split;
    const dim3 grid((N + WBM - 1) / WBM, (M + WBM - 1) / WBM, nz);
    if (nz > 1 && !accumulate)  // atomic accumulation needs a zeroed destination
      BLVM_HIP(hipMemset2DAsync(C, sizeof(float) * (size_t)ldc, 0, sizeof(float) * (size_t)N, (size_t)M, stream));
    if (arm == ARM_WGRAD_SLICED) {
      hipLaunchKernelGGL(wgrad_kernel, grid, dim3(256), 0, stream, g);
      gemm_count_arm(ARM_WGRAD_SLICED);
    } else {
      hipLaunchKernelGGL(wgrad_exact_kernel, grid, dim3(256), 0, stream, g);
      gemm_count_arm(ARM_WGRAD_EXACT);
    }
    BLVM_CHECK_LAUNCH("gemm_f32");
    return BLVM_OK;
  }
  if (arm == ARM_WS) {
    gemm_count_path(1);
    return gemm_ws_f32(op_b, M, N, K, A, lda, B, ldb, C, ldc, bias, act, slope, gate, ldg, accumulate, stream);
  }
  gemm_count_path(0);
  const int tile = (arm - ARM_STAGED) / 3;  // 0: 64 x 64, 1: 128 x 128, 2: 128 x 192, 3: 192 x 128
  const bool big = tile != 0, n192 = tile == 2, m192 = tile == 3;
  const int bm = big ? (m192 ? 192 : 128) : 64;
  const int bn = big ? (n192 ? 192 : 128) : 64;
  const int bk = ot != OP_F32 ? BKB : tile_bk(bm, bn);
  if (colsum != nullptr && (ot != OP_F32 || op_a != 1 || K == 0)) {  // (the 16-bit kernel stages ROUNDED operands: the bias gradient stays an fp32 sum)
    BLVM_TRY(op_a == 1 ? colsum_f32(K, M, A, lda, colsum, 1, stream) : BLVM_EINVAL);
    colsum = nullptr;
  }
  g.colsum = colsum;
  int ksteps = (K + bk - 1) / bk;
  if (split_k > ksteps) split_k = ksteps > 0 ? ksteps : 1;
  g.k_per_split = ((ksteps + split_k - 1) / split_k) * bk;
  if (g.k_per_split == 0) g.k_per_split = bk;
  split_k = (K + g.k_per_split - 1) / g.k_per_split;
  if (split_k < 1) split_k = 1;
  BLVM_REQUIRE(split_k == 1 || (act == 0 && gate == nullptr), "gemm: split-K needs a linear epilogue");
  dim3 grid((N + bn - 1) / bn, (M + bm - 1) / bm, split_k);
  BLVM_REQUIRE(grid.y <= 65535 && grid.z <= 65535, "gemm: grid too large");
  if (split_k > 1 && !accumulate)  // atomic accumulation needs a zeroed destination
    BLVM_HIP(hipMemset2DAsync(C, sizeof(float) * (size_t)ldc, 0, sizeof(float) * (size_t)N, (size_t)M, stream));
  if (n192) launch_gemm<128, 192>(g, op_a, op_b, grid, stream, ot);
  else if (m192) launch_gemm<192, 128>(g, op_a, op_b, grid, stream, ot);
  else if (big) launch_gemm<128, 128>(g, op_a, op_b, grid, stream, ot);
  else launch_gemm<64, 64>(g, op_a, op_b, grid, stream, ot);
  BLVM_CHECK_LAUNCH("gemm_f32");
  return BLVM_OK;
}

int gemm_wgrad_group(const WgradJob* jobs, int njobs, int K, hipStream_t stream) {
  // the problems wgrad_tile takes, largest first; the others (unaligned, K < 1024, the 16-bit operand modes) one by one through gemm_f32
  std::vector<int> take, fits((size_t)std::max(njobs, 0));
  const int arm = wgrad_group_route(jobs, njobs, K, operand_type(), fits.data());
  for (int i = 0; i < njobs; ++i) {
    const WgradJob& j = jobs[i];
    if (!j.dW) {
      if (j.db) BLVM_TRY(colsum_f32(K, j.M, j.D, j.ldd, j.db, 1, stream));
      continue;
    }
    BLVM_REQUIRE(j.D && j.Act && j.M > 0 && j.N > 0 && j.ldd >= j.M && j.lda >= j.N && j.ldw >= j.N, "gemm_wgrad_group: bad job %d", i);
    if (fits[(size_t)i]) {
      take.push_back(i);
      continue;
    }
    BLVM_TRY(gemm_f32(1, 1, j.M, j.N, K, j.D, j.ldd, j.Act, j.lda, j.dW, j.ldw, nullptr, 0, 0.f, nullptr, 0, 1, gemm_pick_split(j.M, j.N, K), stream, j.db));
  }
  if (arm == ARM_COUNT) {  // a group of one: gemm_f32 picks tile and split (measured: 256 x 256 x 16000 alone 40 us there, 47 in a group)
    for (const int i : take) {
      const WgradJob& j = jobs[i];
      BLVM_TRY(gemm_f32(1, 1, j.M, j.N, K, j.D, j.ldd, j.Act, j.lda, j.dW, j.ldw, nullptr, 0, 0.f, nullptr, 0, 1, gemm_pick_split(j.M, j.N, K), stream, j.db));
    }
    return BLVM_OK;
  }
  std::stable_sort(take.begin(), take.end(), [&](int x, int y) { return (long)jobs[x].M * jobs[x].N > (long)jobs[y].M * jobs[y].N; });
  GemmGroup gg;
  gg.n = 0;
  long tiles = 0;
  for (const int i : take) {
    const WgradJob& j = jobs[i];
    GemmArgs& g = gg.p[gg.n++];
    g = GemmArgs{};
    g.A = j.D; g.B = j.Act; g.C = j.dW;
    g.M = j.M; g.N = j.N; g.K = K; g.lda = j.ldd; g.ldb = j.lda; g.ldc = j.ldw;
    g.accumulate = 1;
    g.colsum = j.db;
    tiles += wgrad_tiles(j.M, j.N);
  }
  const bool dma = arm == ARM_WGRAD_GROUP;  // (the tile-area rule is at wgrad_group_route)
  const int bk = dma ? WBK : tile_bk(64, 64);
  int split;
  if (dma) {
    split = wgrad_split(tiles, K);
  } else {  // ~6 workgroups per CU, k ranges of at least 16 stages (512 rows)
    long tiles64 = 0;
    for (int p = 0; p < gg.n; ++p) tiles64 += (long)((gg.p[p].M + 63) / 64) * ((gg.p[p].N + 63) / 64);
    split = (int)std::max(1L, std::min<long>((1536 + tiles64 - 1) / tiles64, (K + bk - 1) / bk / 16));
  }
  const int ksteps = (K + bk - 1) / bk;
  const int k_per_split = ((ksteps + split - 1) / split) * bk;
  gg.split = (K + k_per_split - 1) / k_per_split;
  int first = 0;
  for (int p = 0; p < gg.n; ++p) {
    gg.p[p].k_per_split = k_per_split;
    gg.p[p].a_vec = 1; gg.p[p].b_vec = 1;  // (wgrad_fits: aligned, leading dimensions multiples of 4)
    gg.first[p] = first;
    first += (dma ? wgrad_tiles(gg.p[p].M, gg.p[p].N) : ((gg.p[p].M + 63) / 64) * ((gg.p[p].N + 63) / 64)) * gg.split;
  }
  gg.first[gg.n] = first;
  if (dma) {
    hipLaunchKernelGGL(wgrad_group_kernel, dim3((unsigned)first), dim3(256), 0, stream, gg);
    gemm_count_arm(ARM_WGRAD_GROUP);
  } else {
    hipLaunchKernelGGL(gemm_group_kernel, dim3((unsigned)first), dim3(256), 0, stream, gg);
    gemm_count_arm(ARM_GEMM_GROUP);
  }
  BLVM_CHECK_LAUNCH("gemm_wgrad_group");
  return BLVM_OK;
}

int colsum_f32(int M, int N, const float* X, int ldx, float* out, int accumulate, hipStream_t stream) {
  if (N == 0) return BLVM_OK;
  BLVM_REQUIRE(X && out, "colsum: null operand");
  if (!accumulate) BLVM_HIP(hipMemsetAsync(out, 0, sizeof(float) * (size_t)N, stream));
  if (M == 0) return BLVM_OK;
  int nmod = N;
  if (N % 4 != 0 && ldx == N && aligned16(X)) {  // dense and narrow (the 30-wide DMoL parameter rows): fold g rows into one
    const int g = N % 2 == 0 ? 2 : 4;
    const int tail = M % g;
    if (tail) {  // the last M % g rows through the scalar kernel
      hipLaunchKernelGGL(colsum_kernel, dim3((N + 63) / 64, 1), dim3(256), 0, stream, tail, N, X + (size_t)(M - tail) * ldx, ldx, out, 64);
      M -= tail;
    }
    if (M == 0) return BLVM_OK;
    M /= g; N *= g; ldx *= g;
  }
  if (N % 4 == 0 && ldx % 4 == 0 && aligned16(X)) {
    const int col_blocks = (N / 4 + 63) / 64;
    // every row block ends in one float atomic per column: many row blocks on few columns serialise on the same addresses
    // (1 320 blocks on 192 columns took 135 us for a 35-us stream), so cap the row blocks at 128 and let each wave stream longer
    int row_blocks = 1024 / col_blocks;
    if (row_blocks > 128) row_blocks = 128;
    if (row_blocks < 32) row_blocks = 32;
    int rows_per_block = (M + row_blocks - 1) / row_blocks;
    if (rows_per_block < 64) rows_per_block = 64;
    rows_per_block = (rows_per_block + 3) / 4 * 4;
    dim3 grid(col_blocks, (M + rows_per_block - 1) / rows_per_block);
    hipLaunchKernelGGL(colsum4_kernel, grid, dim3(256), 0, stream, M, N, X, ldx, out, rows_per_block, nmod);
    BLVM_CHECK_LAUNCH("colsum_f32");
    return BLVM_OK;
  }
  int rows_per_block = 64;
  while ((M + rows_per_block - 1) / rows_per_block > 32768) rows_per_block *= 2;
  dim3 grid((N + 63) / 64, (M + rows_per_block - 1) / rows_per_block);
  hipLaunchKernelGGL(colsum_kernel, grid, dim3(256), 0, stream, M, N, X, ldx, out, rows_per_block);
  BLVM_CHECK_LAUNCH("colsum_f32");
  return BLVM_OK;
}

__global__ __launch_bounds__(256) void t16_pack_kernel(const float* __restrict__ src, long rs, long cs, int KB, size_t n,
                                                       float* __restrict__ dst) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int e = (int)(i & 3), lane = (int)((i >> 2) & 63);
  const size_t blk = i >> 8;
  const int j = (int)(blk % KB);
  const size_t t = blk / KB;
  const size_t r = 16 * t + (lane & 15);
  const int k = 16 * j + 4 * (lane >> 4) + e;
  dst[i] = src[r * rs + (size_t)k * cs];
}

// the same block order with 16-bit elements H (__bf16 / _Float16: two per 32-bit word, round to nearest even): the weights of the
// 16-bit operand chains
template <typename H>
__global__ __launch_bounds__(256) void t16_pack16_kernel(const float* __restrict__ src, long rs, long cs, int KB, size_t n2,
                                                            unsigned* __restrict__ dst) {
  const size_t w = (size_t)blockIdx.x * 256 + threadIdx.x;  // output word = elements 2w, 2w + 1
  if (w >= n2) return;
  const size_t i = 2 * w;
  const int e = (int)(i & 3), lane = (int)((i >> 2) & 63);
  const size_t blk = i >> 8;
  const int j = (int)(blk % KB);
  const size_t t = blk / KB;
  const size_t r = 16 * t + (lane & 15);
  const int k = 16 * j + 4 * (lane >> 4) + e;
  typedef float f2 __attribute__((ext_vector_type(2)));
  typedef H b2 __attribute__((ext_vector_type(2)));
  const f2 v = {src[r * rs + (size_t)k * cs], src[r * rs + (size_t)(k + 1) * cs]};
  dst[w] = __builtin_bit_cast(unsigned, __builtin_convertvector(v, b2));
}

// Several packs in ONE launch (a recurrent sequence packs 13-15 weight matrices per call, ~4 us of launch each): while a
// T16PackScope is alive on this thread, t16_pack() only records its job; flush() (or the scope's end) launches them together.
constexpr int kPackJobs = 40;
struct PackJob { const float* src; float* dst; long rs, cs; int KB; unsigned n; };  // n: output words of the job
struct PackJobs { PackJob j[kPackJobs]; };
static_assert(sizeof(PackJobs) <= 4000, "kernel argument size");

// half != 0: 16-bit elements H (fp32 packs take the __bf16 instantiation with half = 0)
template <typename H>
__global__ __launch_bounds__(256) void t16_pack_jobs_kernel(PackJobs a, int half) {
  const PackJob q = a.j[blockIdx.y];
  for (size_t w = (size_t)blockIdx.x * 256 + threadIdx.x; w < q.n; w += (size_t)gridDim.x * 256) {
    const size_t i = half ? 2 * w : w;
    const int e = (int)(i & 3), lane = (int)((i >> 2) & 63);
    const size_t blk = i >> 8;
    const int j = (int)(blk % q.KB);
    const size_t t = blk / q.KB;
    const size_t r = 16 * t + (lane & 15);
    const int k = 16 * j + 4 * (lane >> 4) + e;
    if (half) {
      typedef float f2 __attribute__((ext_vector_type(2)));
      typedef H b2 __attribute__((ext_vector_type(2)));
      const f2 v = {q.src[r * q.rs + (size_t)k * q.cs], q.src[r * q.rs + (size_t)(k + 1) * q.cs]};
      reinterpret_cast<unsigned*>(q.dst)[w] = __builtin_bit_cast(unsigned, __builtin_convertvector(v, b2));
    } else {
      q.dst[w] = q.src[r * q.rs + (size_t)k * q.cs];
    }
  }
}

namespace {
struct PackState {
  bool active = false;
  OpType ot = OP_F32;
  int n = 0;
  hipStream_t stream = nullptr;
  PackJobs jobs;
};
thread_local PackState g_pack;
int pack_flush() {
  PackState& p = g_pack;
  if (p.n == 0) return BLVM_OK;
  unsigned most = 0;
  for (int i = 0; i < p.n; ++i) most = std::max(most, p.jobs.j[i].n);
  const unsigned bx = std::min<unsigned>((most + 255) / 256, 512);
  if (p.ot == OP_F16) hipLaunchKernelGGL(t16_pack_jobs_kernel<_Float16>, dim3(bx, (unsigned)p.n), dim3(256), 0, p.stream, p.jobs, 1);
  else hipLaunchKernelGGL(t16_pack_jobs_kernel<__bf16>, dim3(bx, (unsigned)p.n), dim3(256), 0, p.stream, p.jobs, p.ot == OP_BF16 ? 1 : 0);
  p.n = 0;
  BLVM_CHECK_LAUNCH("t16_pack_jobs");
  return BLVM_OK;
}
}  // namespace
T16PackScope::T16PackScope(OpType ot, hipStream_t stream) : prev_(g_pack.ot), prev_active_(g_pack.active) {
  g_pack.ot = ot; g_pack.active = true; g_pack.stream = stream;
}
int T16PackScope::flush() {
  const int rc = pack_flush();
  g_pack.active = false;  // packs requested after the flush run at once again (their consumers may follow immediately)
  return rc;
}
T16PackScope::~T16PackScope() {
  (void)pack_flush();  // (a caller that returned early; an error here resurfaces at the next checked launch)
  g_pack.ot = prev_; g_pack.active = prev_active_;
}

int t16_pack(const float* src, long rs, long cs, int R, int K, float* dst, hipStream_t stream) {
  BLVM_REQUIRE(src && dst && R > 0 && K > 0 && R % 16 == 0 && K % 16 == 0 && aligned16(dst), "t16_pack: R=%d, K=%d must be multiples of 16", R, K);
  const size_t n = (size_t)R * K;
  BLVM_REQUIRE(n < (1ull << 31), "t16_pack: matrix too large");
  if (g_pack.active && g_pack.stream == stream) {  // deferred: one launch for all packs of the scope
    if (g_pack.n == kPackJobs) BLVM_TRY(pack_flush());
    g_pack.jobs.j[g_pack.n++] = PackJob{src, dst, rs, cs, K / 16, (unsigned)(g_pack.ot != OP_F32 ? n / 2 : n)};
    return BLVM_OK;
  }
  if (g_pack.ot != OP_F32) {
    const dim3 grid((unsigned)((n / 2 + 255) / 256));
    if (g_pack.ot == OP_F16) hipLaunchKernelGGL(t16_pack16_kernel<_Float16>, grid, dim3(256), 0, stream, src, rs, cs, K / 16, n / 2, reinterpret_cast<unsigned*>(dst));
    else hipLaunchKernelGGL(t16_pack16_kernel<__bf16>, grid, dim3(256), 0, stream, src, rs, cs, K / 16, n / 2, reinterpret_cast<unsigned*>(dst));
    BLVM_CHECK_LAUNCH("t16_pack16");
    return BLVM_OK;
  }
  hipLaunchKernelGGL(t16_pack_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, src, rs, cs, K / 16, n, dst);
  BLVM_CHECK_LAUNCH("t16_pack");
  return BLVM_OK;
}

int transpose_f32(int M, int N, const float* X, int ldx, float* out, int ldo, hipStream_t stream) {
  if (M == 0 || N == 0) return BLVM_OK;
  dim3 grid((N + 31) / 32, (M + 31) / 32);
  hipLaunchKernelGGL(transpose_kernel, grid, dim3(256), 0, stream, M, N, X, ldx, out, ldo);
  BLVM_CHECK_LAUNCH("transpose_f32");
  return BLVM_OK;
}

}  // namespace blvm

extern "C" int blvm_gemm_f32(int op_a, int op_b, int M, int N, int K, const float* A, int lda, const float* B,
                             int ldb, float* C, int ldc, const float* bias, int act, float slope,
                             const float* gate, int ldg, int accumulate, int split_k, void* stream) {
  return blvm::gemm_f32(op_a, op_b, M, N, K, A, lda, B, ldb, C, ldc, bias, act, slope, gate, ldg, accumulate,
                        split_k, static_cast<hipStream_t>(stream));
}

extern "C" int blvm_wgrad_f32(int N_out, int K_in, int rows, const float* D, int ldd, const float* X, int ldx, float* dW, int lddw, float* db,
                              int split_k, void* stream) {
  using namespace blvm;
  hipStream_t s = static_cast<hipStream_t>(stream);
  BLVM_REQUIRE(N_out >= 0 && K_in >= 0 && rows >= 0, "wgrad: negative dimension");
  if (dW == nullptr) return db ? colsum_f32(rows, N_out, D, ldd, db, 1, s) : BLVM_OK;
  if (split_k < 1) split_k = gemm_pick_split(N_out, K_in, rows);
  return gemm_f32(1, 1, N_out, K_in, rows, D, ldd, X, ldx, dW, lddw, nullptr, 0, 0.f, nullptr, 0, 1, split_k, s, db);
}

extern "C" int blvm_wgrad_group_f32(int n, const int* N_out, const int* K_in, int rows, const float* const* D, const int* ldd, const float* const* X,
                                    const int* ldx, float* const* dW, const int* lddw, float* const* db, void* stream) {
  using namespace blvm;
  BLVM_REQUIRE(n >= 0 && rows >= 0 && (n == 0 || (N_out && K_in && D && ldd && X && ldx && dW && lddw && db)), "wgrad_group: bad arguments");
  if (n == 0 || rows == 0) return BLVM_OK;
  std::vector<WgradJob> jobs((size_t)n);
  for (int i = 0; i < n; ++i) {
    BLVM_REQUIRE(N_out[i] > 0 && K_in[i] > 0 && D[i] && (dW[i] == nullptr || X[i]), "wgrad_group: bad job %d", i);
    jobs[(size_t)i] = WgradJob{D[i], ldd[i], N_out[i], X[i], ldx[i], K_in[i], dW[i], lddw[i], db[i]};
  }
  return gemm_wgrad_group(jobs.data(), n, rows, static_cast<hipStream_t>(stream));
}

extern "C" int blvm_act_bwd_f32(const float* dy, const float* y, float slope, float* dz, size_t n, void* stream) {
  using namespace blvm;
  if (n == 0) return BLVM_OK;
  BLVM_REQUIRE(dy && y && dz, "act_bwd: null pointer");
  BLVM_REQUIRE(aligned16(dy) && aligned16(y) && aligned16(dz), "act_bwd: buffers must be 16-byte aligned");
  const size_t n4 = n / 4;
  size_t blocks = (n4 + 255) / 256;
  if (blocks > 2048) blocks = 2048;
  if (blocks < 1) blocks = 1;
  hipLaunchKernelGGL(act_bwd_kernel, dim3((unsigned)blocks), dim3(256), 0, static_cast<hipStream_t>(stream), dy, y,
                     slope, dz, n4, n);
  BLVM_CHECK_LAUNCH("act_bwd_f32");
  return BLVM_OK;
}

extern "C" int blvm_colsum_f32(int M, int N, const float* X, int ldx, float* out, int accumulate, void* stream) {
  return blvm::colsum_f32(M, N, X, ldx, out, accumulate, static_cast<hipStream_t>(stream));
}

extern "C" int blvm_gemm_arm(int op_a, int op_b, int M, int N, int K, size_t a_addr, int lda, size_t b_addr, int ldb, int split_k, int has_bias,
                             int act, int has_gate, int has_colsum, int operand, int min_rows) {
  return blvm::gemm_arm(op_a, op_b, M, N, K, (uintptr_t)a_addr, lda, (uintptr_t)b_addr, ldb, split_k, has_bias != 0, act, has_gate != 0,
                        has_colsum != 0, operand, min_rows, blvm::gemm_force_tile());
}

extern "C" int blvm_wgrad_group_route(int n, const int* N_out, const int* K_in, int rows, const size_t* d_addr, const int* ldd,
                                      const size_t* x_addr, const int* ldx, const int* has_dw, int operand, int* joins) {
  using namespace blvm;
  if (n < 0 || (n > 0 && !(N_out && K_in && d_addr && ldd && x_addr && ldx && has_dw && joins))) return ARM_COUNT;
  std::vector<WgradJob> jobs((size_t)n);
  static float some_dw;  // (never dereferenced: a job's dW only has to be non-null)
  for (int i = 0; i < n; ++i)
    jobs[(size_t)i] = WgradJob{reinterpret_cast<const float*>((uintptr_t)d_addr[i]), ldd[i], N_out[i],
                               reinterpret_cast<const float*>((uintptr_t)x_addr[i]), ldx[i], K_in[i], has_dw[i] ? &some_dw : nullptr, K_in[i], nullptr};
  const int arm = wgrad_group_route(jobs.data(), n, rows, operand, joins);
  for (int i = 0; i < n; ++i) joins[i] = !has_dw[i] ? -1 : (arm != ARM_COUNT && joins[i] ? 1 : 0);
  return arm;
}

extern "C" int blvm_gemm_arm_counts(unsigned long long out[17]) {
  static_assert(blvm::ARM_COUNT == 17, "the header's numbering");
  BLVM_REQUIRE(out != nullptr, "blvm_gemm_arm_counts: null pointer");
  for (int a = 0; a < blvm::ARM_COUNT; ++a) out[a] = blvm::g_arm_count[a].load(std::memory_order_relaxed);
  return BLVM_OK;
}
