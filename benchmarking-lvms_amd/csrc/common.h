// common.h — shared host/device helpers for libblvm_hip (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <limits.h>
#include <stdint.h>
#include <stdio.h>

#include "blvm_hip.h"

namespace blvm {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

void set_error(const char* fmt, ...);

#define BLVM_REQUIRE(cond, ...)            \
  do {                                     \
    if (!(cond)) {                         \
      blvm::set_error(__VA_ARGS__);        \
      return BLVM_EINVAL;                  \
    }                                      \
  } while (0)

#define BLVM_CHECK_LAUNCH(what)                                                     \
  do {                                                                              \
    hipError_t e__ = hipGetLastError();                                             \
    if (e__ != hipSuccess) {                                                        \
      blvm::set_error("%s: launch failed: %s", what, hipGetErrorString(e__));       \
      return BLVM_ELAUNCH;                                                          \
    }                                                                               \
  } while (0)

#define BLVM_HIP(call)                                                              \
  do {                                                                              \
    hipError_t e__ = (call);                                                        \
    if (e__ != hipSuccess) {                                                        \
      blvm::set_error("%s failed: %s", #call, hipGetErrorString(e__));              \
      return BLVM_ELAUNCH;                                                          \
    }                                                                               \
  } while (0)

// BLVM_TRY(expr): evaluates an int status and returns it from the enclosing function (or int lambda) when it is non-zero
// (variadic only so that expr may hold the commas of a template argument list)
#define BLVM_TRY(...)                      \
  do {                                     \
    const int rc__ = (__VA_ARGS__);        \
    if (rc__) return rc__;                 \
  } while (0)

static inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

// Carves one caller-owned buffer of floats into 16-byte aligned pieces.  A null base gives sizes only (the *_floats exports).
struct Arena {
  float* base = nullptr;
  size_t off = 0;  // floats taken so far
  size_t take_off(size_t count) { const size_t at = off; off += (count + 3) & ~(size_t)3; return at; }  // the piece as an offset
  float* take(size_t count) { const size_t at = take_off(count); return base ? base + at : nullptr; }   // take(0): the running end
  size_t floats() const { return off; }
  // bytes from p (a piece taken earlier) to the running end: the region a persistent launch polls, sentinel-filled in one go
  size_t bytes_from(const float* p) const { return base ? sizeof(float) * (size_t)(base + off - p) : 0; }
};

// initial states: dst = src, or zeros where the caller passes none (contiguous | `rows` rows of `width` bytes at `dpitch`)
inline hipError_t copy_or_zero(void* dst, const void* src, size_t bytes, hipStream_t s) {
  return src ? hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, s) : hipMemsetAsync(dst, 0, bytes, s);
}
inline hipError_t copy_or_zero_2d(void* dst, size_t dpitch, const void* src, size_t width, size_t rows, hipStream_t s) {
  return src ? hipMemcpy2DAsync(dst, dpitch, src, width, width, rows, hipMemcpyDeviceToDevice, s) : hipMemset2DAsync(dst, dpitch, 0, width, rows, s);
}

// ---- host side of the ring decoders' entry points (wavenet_decode.hip, stcn_decode.hip) ----
// floats of the rings of n gated blocks: block i keeps its own input over the last dilations[i] frames, [dil_i,B,C]
inline size_t ring_floats(const int* dilations, int n, int B, int C) {
  size_t frames = 0;
  for (int i = 0; i < n; ++i) frames += (size_t)(dilations[i] > 0 ? dilations[i] : 0);
  return frames * B * C;
}

// the arguments of an entry from a state: `who` the entry, `state` what x_in / x_state hold, `count` the name of the step count T
inline int check_resume(const char* who, const char* state, const char* count, int t0, int T, const void* x_in, const void* x_state) {
  BLVM_REQUIRE(x_in && x_state, "%s: NULL %s state", who, state);
  BLVM_REQUIRE(t0 >= 0 && T < INT_MAX - t0, "%s: t0 = %d, %s = %d: need 0 <= t0, t0 + %s < 2^31 - 1", who, t0, count, T, count);
  return BLVM_OK;
}

// zero steps from a state: the state goes back as it came
inline int hand_back_state(float* x_state, const float* x_in, size_t floats, hipStream_t s) {
  if (x_state != x_in) BLVM_HIP(hipMemcpyAsync(x_state, x_in, sizeof(float) * floats, hipMemcpyDeviceToDevice, s));
  return BLVM_OK;
}

// beta of the Gaussian heads' softplus (softplus_beta below): ln2 / (initial_sd - eps), initial_sd = 1
inline float softplus_beta_of(float sd_eps) { return (float)(0.6931471805599453 / (1.0 - (double)sd_eps)); }

// kernel<NW> for nw = 16 | 8 | 4 waves (tried, and so instantiated, in that order).  `kernel` is written with NW_ for its wave
// count: gru_stage_kernel<NW_>, or in parentheses when its template arguments hold a comma: (lin_stage_kernel<NW_, NSEG>)
#define LAUNCH_NW(kernel, nw, grid, stream, ...)                                                                                  \
  do {                                                                                                                            \
    if ((nw) == 16) { constexpr int NW_ = 16; hipLaunchKernelGGL(kernel, grid, dim3(NW_ * 64), 0, stream, __VA_ARGS__); }         \
    else if ((nw) == 8) { constexpr int NW_ = 8; hipLaunchKernelGGL(kernel, grid, dim3(NW_ * 64), 0, stream, __VA_ARGS__); }      \
    else { constexpr int NW_ = 4; hipLaunchKernelGGL(kernel, grid, dim3(NW_ * 64), 0, stream, __VA_ARGS__); }                     \
  } while (0)

// ---- device math -----------------------------------------------------------------------------------------------
// Accurate libm forms (parity first: ELBO must match the fp32 CPU path to 1e-4 relative over ~1e6 frames).
__device__ __forceinline__ float exp_(float x) { return expf(x); }
__device__ __forceinline__ float log_(float x) { return logf(x); }
__device__ __forceinline__ float sigmoidf_(float x) { return 1.0f / (1.0f + expf(-x)); }

// torch.nn.functional.softplus(x) (beta=1, threshold=20): x > 20 ? x : log1p(exp(x))
__device__ __forceinline__ float softplusf_(float x) { return x > 20.0f ? x : log1pf(expf(x)); }

// softplus with beta (threshold on beta*x, as torch does)
__device__ __forceinline__ float softplus_beta(float x, float beta, float inv_beta) {
  float bx = beta * x;
  return bx > 20.0f ? x : inv_beta * log1pf(expf(bx));
}

// Split-K factor of a weight-gradient GEMM [M,N] += A^T B over K rows: gemm_f32 cuts that form into 64x64 tiles; ask for
// ~3 workgroups per CU, at least 256 k per slice.
inline int gemm_pick_split(int M, int N, int K) {
  const int bm = 64;
  const long tiles = (long)((M + bm - 1) / bm) * ((N + bm - 1) / bm);
  int s = (int)((768 + tiles - 1) / tiles);
  const int kmax = (K + 255) / 256;
  if (s > kmax) s = kmax;
  return s < 1 ? 1 : s;
}

// ---- 16x16 output tile, K split over the NW waves of a workgroup ------------------------------------------------
// acc += A[r0+i][k] * W[c0+j][k] for the k-chunks owned by `wave` (chunk = 16 k, waves interleave chunks).
// A rows >= nrows read as zero.  A, W must be 16-byte aligned with lda, ldw multiples of 4 and K a multiple of 16.
// v_mfma_f32_16x16x4_f32: lane l supplies A[i=l&15][k=l>>4], B[k=l>>4][j=l&15]; D: col=l&15, row=(l>>4)*4+reg.
// Each lane fetches 4 consecutive k as one 16-byte load and feeds them to 4 MFMAs; A and B use the same
// k-permutation, so the sum over k is complete.
//
// WT16: W is in the T16 OPERAND LAYOUT (t16_pack below) instead of row-major.  Row-major, one wave load of the operand
// touches 16 rows x 64 bytes — 16 half-used cache lines — and a workgroup ingests ~38 GB/s from L2; in T16 every
// (16 rows x 16 k) block is stored as the 64 lanes' 16-byte fragments back to back, so the same load is ONE contiguous
// 1 KB read (~150 GB/s per workgroup, tools/cu_ingest.hip).  Block (row tile t, k chunk j) of a [R,K] matrix sits at
// ((t * K/16 + j) * 256) floats, element (rr, 4q+e) of it at (rr + 16 q) * 4 + e: the fragment address of lane
// (rr = lane & 15, q = lane >> 4) is W + c0 * ldw + 16 * k0 + 4 * lane with ldw = the packed matrix's K.
// `mid` hook of the product helpers: runs once, right after the first trip's operand loads are issued (see wave_gemm16_multi)
struct NoMid {
  __device__ __forceinline__ void operator()() const {}
};

// keeps the scheduler from hoisting the hook's argument wait (s_waitcnt lgkmcnt) above the operand loads issued before it
template <class Mid>
__device__ __forceinline__ void mid_fence() {
  if constexpr (!__is_same(Mid, NoMid)) __builtin_amdgcn_sched_barrier(0);
}

// U consecutive k-chunks of one wave: all 2U fragment loads first, then the 4U MFMAs in ascending k
template <int U, int STEP, int WS, class Mid>
__device__ __forceinline__ f32x4 gemm16_chunks(const float* __restrict__ ap, const float* __restrict__ wp, int kc, bool aok,
                                                f32x4 acc, bool& pending, Mid& mid) {
  float4 a[U], w[U];
#pragma unroll
  for (int u = 0; u < U; ++u) a[u] = *reinterpret_cast<const float4*>(ap + kc + u * STEP);
#pragma unroll
  for (int u = 0; u < U; ++u) w[u] = *reinterpret_cast<const float4*>(wp + (size_t)WS * (kc + u * STEP));
  if (pending) { mid_fence<Mid>(); mid(); pending = false; }
  if (!aok) {
#pragma unroll
    for (int u = 0; u < U; ++u) a[u] = make_float4(0.f, 0.f, 0.f, 0.f);
  }
#pragma unroll
  for (int u = 0; u < U; ++u) {
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[u].x, w[u].x, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[u].y, w[u].y, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[u].z, w[u].z, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[u].w, w[u].w, acc, 0, 0, 0);
  }
  return acc;
}

template <int NW, bool WT16 = false, class Mid = NoMid>
__device__ __forceinline__ f32x4 wave_gemm16(const float* __restrict__ A, int lda, int r0, int nrows,
                                              const float* __restrict__ W, int ldw, int c0, int K, int wave,
                                              f32x4 acc, Mid mid = Mid()) {
  bool pending = true;
  constexpr int STEP = NW * 16;
  const int lane = threadIdx.x & 63;
  const int rr = lane & 15, q = lane >> 4;
  const bool aok = (r0 + rr) < nrows;
  const float* ap = A + (size_t)(aok ? r0 + rr : 0) * lda + 4 * q;
  const float* wp = WT16 ? W + (size_t)c0 * ldw + 4 * lane : W + (size_t)(c0 + rr) * ldw + 4 * q;
  constexpr int WS = WT16 ? 16 : 1;  // k stride of the W fragment address
  int kc = wave * 16;
  // 4 chunks per trip keeps 8 x 16-byte loads in flight; left-over chunks are one dependent round trip EACH, so the host picks
  // NW such that a wave owns 4 chunks or 1 (stages.h pick_nw).  Handling 2-3 left-over chunks in one trip here was tried: the
  // extra code costs every link ~0.06 us (VRNN +0.3 ms/step) and only the 3-chunk shapes gain (tools/chain_bench.hip).
  for (; kc + 3 * STEP < K; kc += 4 * STEP) acc = gemm16_chunks<4, STEP, WS>(ap, wp, kc, aok, acc, pending, mid);
  for (; kc < K; kc += STEP) acc = gemm16_chunks<1, STEP, WS>(ap, wp, kc, aok, acc, pending, mid);
  if (pending) mid();
  return acc;
}

// ---- G products of the same K in ONE loop -----------------------------------------------------------------------------
// acc[g] += A[g][r0+i][k] * W[g][c0[g]+j][k], W in T16.  A stage that needs several products (the 4 LSTM gates, the 3 GRU
// gates, both Gaussian heads ...) must not call wave_gemm16 once per product: K is a run-time value, so every call is its own
// loop nest and the loads of product g+1 are issued only after product g's MFMAs — G dependent memory round trips (~1 us each
// from the Infinity Cache) instead of one.  Here all 2G (SAMEA: G+1) fragment loads of a k-chunk are issued together, two
// chunks per trip.  Every acc[g] still sums its chunks in ascending order, element by element, exactly as wave_gemm16 does:
// results are bit-identical.  The MFMAs of the G products are interleaved, so consecutive MFMAs are independent.
//
// `mid` runs once, right after the first trip's operand loads are issued (or at the end for a wave without chunks): a kernel
// whose operand pointers are preloaded SGPRs (stages.h, launch-latency note 4) puts there the epilogue prefetches whose pointers
// still come by s_load, so the operand loads never wait for the argument fetch.
template <int NW, int G, bool SAMEA, class Mid = NoMid>
__device__ __forceinline__ void wave_gemm16_multi(const float* const (&A)[G], const int (&lda)[G], int r0, int nrows,
                                                  const float* const (&W)[G], const int (&ldw)[G], const int (&c0)[G], int K,
                                                  int wave, f32x4 (&acc)[G], Mid mid = Mid()) {
  bool pending = true;
  constexpr int STEP = NW * 16;
  constexpr int GA = SAMEA ? 1 : G;
  const int lane = threadIdx.x & 63;
  const int rr = lane & 15, q = lane >> 4;
  const bool aok = (r0 + rr) < nrows;
  const float* ap[GA];
  const float* wp[G];
#pragma unroll
  for (int g = 0; g < GA; ++g) ap[g] = A[g] + (size_t)(aok ? r0 + rr : 0) * lda[g] + 4 * q;
#pragma unroll
  for (int g = 0; g < G; ++g) wp[g] = W[g] + (size_t)c0[g] * ldw[g] + 4 * lane;
  const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
  int kc = wave * 16;
  for (; kc + STEP < K; kc += 2 * STEP) {
    float4 a0[GA], a1[GA], w0[G], w1[G];
#pragma unroll
    for (int g = 0; g < GA; ++g) {
      a0[g] = *reinterpret_cast<const float4*>(ap[g] + kc);
      a1[g] = *reinterpret_cast<const float4*>(ap[g] + kc + STEP);
    }
#pragma unroll
    for (int g = 0; g < G; ++g) {
      w0[g] = *reinterpret_cast<const float4*>(wp[g] + 16 * (size_t)kc);
      w1[g] = *reinterpret_cast<const float4*>(wp[g] + 16 * (size_t)(kc + STEP));
    }
    if (pending) { mid_fence<Mid>(); mid(); pending = false; }
    if (!aok) {
#pragma unroll
      for (int g = 0; g < GA; ++g) a0[g] = a1[g] = zero;
    }
#pragma unroll
    for (int g = 0; g < G; ++g) acc[g] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0[SAMEA ? 0 : g].x, w0[g].x, acc[g], 0, 0, 0);
#pragma unroll
    for (int g = 0; g < G; ++g) acc[g] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0[SAMEA ? 0 : g].y, w0[g].y, acc[g], 0, 0, 0);
#pragma unroll
    for (int g = 0; g < G; ++g) acc[g] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0[SAMEA ? 0 : g].z, w0[g].z, acc[g], 0, 0, 0);
#pragma unroll
    for (int g = 0; g < G; ++g) acc[g] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0[SAMEA ? 0 : g].w, w0[g].w, acc[g], 0, 0, 0);
#pragma unroll
    for (int g = 0; g < G; ++g) acc[g] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1[SAMEA ? 0 : g].x, w1[g].x, acc[g], 0, 0, 0);
#pragma unroll
    for (int g = 0; g < G; ++g) acc[g] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1[SAMEA ? 0 : g].y, w1[g].y, acc[g], 0, 0, 0);
#pragma unroll
    for (int g = 0; g < G; ++g) acc[g] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1[SAMEA ? 0 : g].z, w1[g].z, acc[g], 0, 0, 0);
#pragma unroll
    for (int g = 0; g < G; ++g) acc[g] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1[SAMEA ? 0 : g].w, w1[g].w, acc[g], 0, 0, 0);
  }
  for (; kc < K; kc += STEP) {
    float4 a0[GA], w0[G];
#pragma unroll
    for (int g = 0; g < GA; ++g) a0[g] = *reinterpret_cast<const float4*>(ap[g] + kc);
#pragma unroll
    for (int g = 0; g < G; ++g) w0[g] = *reinterpret_cast<const float4*>(wp[g] + 16 * (size_t)kc);
    if (pending) { mid_fence<Mid>(); mid(); pending = false; }
    if (!aok) {
#pragma unroll
      for (int g = 0; g < GA; ++g) a0[g] = zero;
    }
#pragma unroll
    for (int g = 0; g < G; ++g) acc[g] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0[SAMEA ? 0 : g].x, w0[g].x, acc[g], 0, 0, 0);
#pragma unroll
    for (int g = 0; g < G; ++g) acc[g] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0[SAMEA ? 0 : g].y, w0[g].y, acc[g], 0, 0, 0);
#pragma unroll
    for (int g = 0; g < G; ++g) acc[g] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0[SAMEA ? 0 : g].z, w0[g].z, acc[g], 0, 0, 0);
#pragma unroll
    for (int g = 0; g < G; ++g) acc[g] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0[SAMEA ? 0 : g].w, w0[g].w, acc[g], 0, 0, 0);
  }
  if (pending) mid();
}

// ---- 32x32 output tile (large batches), K split over the NW waves of a workgroup ---------------------------------------
// acc += A[r0+i][k] * W[c0+j][k] with v_mfma_f32_32x32x2_f32: lane (li = lane & 31, lh = lane >> 5) loads 4 consecutive k at
// offset 4*lh of every 8-k chunk as one 16-byte load and feeds them to 4 MFMAs (MFMA c sums k = chunk + c and chunk + 4 + c;
// A and B use the same permutation).  Compared with the 16x16 tile every operand byte fetched from L2 feeds twice the FLOPs:
// at B >= 128 the links are bound by those bytes, not by launch latency.  K must be a multiple of 8.
template <int NW, bool WT16 = false>
__device__ __forceinline__ f32x16 wave_gemm32(const float* __restrict__ A, int lda, int r0, int nrows,
                                               const float* __restrict__ W, int ldw, int c0, int K, int wave, f32x16 acc) {
  constexpr int STEP = NW * 8;
  const int lane = threadIdx.x & 63, li = lane & 31, lh = lane >> 5;
  const bool aok = (r0 + li) < nrows;
  const float* ap = A + (size_t)(aok ? r0 + li : 0) * lda + 4 * lh;
  // T16: rows c0 + li live in row tile c0/16 + (li >> 4); k = kc + 4 lh is quad 2 * ((kc >> 3) & 1) + lh of chunk kc >> 4
  const float* wp = WT16 ? W + (size_t)(c0 / 16 + (li >> 4)) * ldw * 16 + ((li & 15) + 16 * lh) * 4 : W + (size_t)(c0 + li) * ldw + 4 * lh;
  constexpr int WS = WT16 ? 16 : 1;
  const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
  int kc = wave * 8;
  for (; kc + 3 * STEP < K; kc += 4 * STEP) {
    float4 a0 = *reinterpret_cast<const float4*>(ap + kc);
    float4 a1 = *reinterpret_cast<const float4*>(ap + kc + STEP);
    float4 a2 = *reinterpret_cast<const float4*>(ap + kc + 2 * STEP);
    float4 a3 = *reinterpret_cast<const float4*>(ap + kc + 3 * STEP);
    const float4 w0 = *reinterpret_cast<const float4*>(wp + WS * (kc));
    const float4 w1 = *reinterpret_cast<const float4*>(wp + WS * (kc + STEP));
    const float4 w2 = *reinterpret_cast<const float4*>(wp + WS * (kc + 2 * STEP));
    const float4 w3 = *reinterpret_cast<const float4*>(wp + WS * (kc + 3 * STEP));
    if (!aok) { a0 = a1 = a2 = a3 = zero; }
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a0.x, w0.x, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a0.y, w0.y, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a0.z, w0.z, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a0.w, w0.w, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a1.x, w1.x, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a1.y, w1.y, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a1.z, w1.z, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a1.w, w1.w, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a2.x, w2.x, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a2.y, w2.y, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a2.z, w2.z, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a2.w, w2.w, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a3.x, w3.x, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a3.y, w3.y, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a3.z, w3.z, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a3.w, w3.w, acc, 0, 0, 0);
  }
  for (; kc < K; kc += STEP) {
    float4 a0 = *reinterpret_cast<const float4*>(ap + kc);
    const float4 w0 = *reinterpret_cast<const float4*>(wp + WS * (kc));
    if (!aok) a0 = zero;
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a0.x, w0.x, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a0.y, w0.y, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a0.z, w0.z, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a0.w, w0.w, acc, 0, 0, 0);
  }
  return acc;
}

// Combine the NW waves' partial 16x16 tiles of G groups through LDS.  `red` must hold G*NW*256 floats.
// After the call threads 0..255 own element (i = tid>>4, j = tid&15) of every group: out[g]; other threads get 0.
template <int G, int NW>
__device__ __forceinline__ void reduce_tiles(const f32x4 (&acc)[G], float* __restrict__ red, float (&out)[G]) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
#pragma unroll
  for (int g = 0; g < G; ++g) {
    // element (row=(lane>>4)*4+reg, col=lane&15) stored at [g][wave][row*16+col]
#pragma unroll
    for (int r = 0; r < 4; ++r) red[(g * NW + wave) * 256 + ((lane >> 4) * 4 + r) * 16 + (lane & 15)] = acc[g][r];
  }
  __syncthreads();
#pragma unroll
  for (int g = 0; g < G; ++g) {
    float s = 0.f;
    if (tid < 256) {
#pragma unroll
      for (int w = 0; w < NW; ++w) s += red[(g * NW + w) * 256 + tid];
    }
    out[g] = s;
  }
}

}  // namespace blvm

namespace blvm {
// persistent chains (pchain.h): the process-wide control block and a fresh launch epoch (core.hip)
int pchain_ctl(unsigned** dev, unsigned** host_dev, unsigned* epoch);
// largest batch the recurrent sequences run as ONE persistent launch for (0 = never; env BLVM_PCHAIN=0 / BLVM_PCHAIN_MAX_B=n, or
// blvm_pchain_configure).  Beyond it the links are bound by MFMA / operand bytes, not latency, and the 32x32-tile launch-per-link
// kernels fit better.
int pchain_max_batch();
int pchain_tune();  // placement bits (env BLVM_PCHAIN_TUNE / blvm_pchain_tune): 4 XCD-aware tile placement, 16 canary polls of deferred tiles,
                     // 32 / 64 placement of the static walks' launches (vrnn_static.h Place: plain / local where it applies),
                     // 128 no look-ahead arming in the static walks: the host fills every polled slab (vrnn_static.h kArmAhead)
unsigned long long* pchain_profile_buffer();  // diagnostics: null unless blvm_pchain_profile() installed a device buffer

// internal launchers shared between translation units (defined in gemm.hip)
int gemm_f32(int op_a, int op_b, int M, int N, int K, const float* A, int lda, const float* B, int ldb, float* C,
             int ldc, const float* bias, int act, float slope, const float* gate, int ldg, int accumulate,
             int split_k, hipStream_t stream, float* colsum = nullptr);  // colsum (op_a == 1): [M] += sum over k of A[k][:]
// the weight-stationary forward / data-gradient path (gemm_ws.hip): its routing predicate (host arithmetic only), the row threshold
// in force (blvm_gemm_ws_min_rows), the launcher gemm_f32 hands such a product to, and gemm_f32's per-path launch counter
bool gemm_ws_route(int op_a, int M, int N, int K, uintptr_t a_addr, int lda, int split_k, bool has_colsum, int operand, int min_rows);
int gemm_ws_min_rows();
int gemm_ws_f32(int op_b, int M, int N, int K, const float* A, int lda, const float* B, int ldb, float* C, int ldc, const float* bias,
                int act, float slope, const float* gate, int ldg, int accumulate, hipStream_t stream);
void gemm_count_path(int path);  // 0: the staged tiles of gemm.hip, 1: gemm_ws.hip
// The kernels K6 chooses among (the BLVM_GEMM_ARM_* numbers of include/blvm_hip.h).  ARM_STAGED + 3 * tile + operand with tile 0 the
// 64 x 64, 1 the 128 x 128, 2 the 128 x 192, 3 the 192 x 128 register-staged tile and operand an OpType value; ARM_COUNT doubles as
// "nothing is launched".  gemm_arm (gemm.hip) is gemm_f32's dispatch as host arithmetic; gemm_count_arm counts one launch.
enum GemmArm { ARM_WS = 0, ARM_STAGED = 1, ARM_WGRAD_EXACT = 13, ARM_WGRAD_SLICED = 14, ARM_WGRAD_GROUP = 15, ARM_GEMM_GROUP = 16, ARM_COUNT = 17 };
int gemm_arm(int op_a, int op_b, int M, int N, int K, uintptr_t a_addr, int lda, uintptr_t b_addr, int ldb, int split_k, bool has_bias,
             int act, bool has_gate, bool has_colsum, int operand, int min_rows, int force_tile);
void gemm_count_arm(int arm);
int colsum_f32(int M, int N, const float* X, int ldx, float* out, int accumulate, hipStream_t stream);
// Weight gradients of one reduction length as ONE launch: dW[M,N] += D^T[M,K] Act[K,N] and, with db, db[M] += column sums of D, for
// every job with dW (a job without dW only sums its columns).  Jobs with 16-byte aligned operands, M, N and leading dimensions
// multiples of 4 and K >= 1024 run together on gemm.hip wgrad_group_kernel (the LDS-DMA 128 x 128 tile), or on gemm_group_kernel
// (64 x 64) when they would fill under 95 % of their 128 x 128 tile area; a group of one, the other jobs (up to 20 per group) and
// the 16-bit operand modes go one by one through gemm_f32.
struct WgradJob {
  const float* D; int ldd, M;
  const float* Act; int lda, N;
  float* dW; int ldw;
  float* db;
};
int gemm_wgrad_group(const WgradJob* jobs, int njobs, int K, hipStream_t stream);
int transpose_f32(int M, int N, const float* X, int ldx, float* out, int ldo, hipStream_t stream);
// Operand type of the matrix products (core.hip; blvm_set_operand_dtype / env BLVM_DTYPE=bf16|f16; values = BLVM_DTYPE_*): OP_F32
// (the default); OP_BF16 / OP_F16: operands rounded to bf16 / fp16 (nearest even) with fp32 accumulation for the persistent chains,
// the sequence kernels, the WaveNet block kernels and K6 — the reference's `--use_amp True` regime (experiments/
// experiment_vrnn_audio.py:219-230; fp16 is its autocast type).  Everything stored, every epilogue and every reduction stays fp32.
enum OpType { OP_F32 = 0, OP_BF16 = 1, OP_F16 = 2 };
OpType operand_type();
inline bool operand_16bit() { return operand_type() != OP_F32; }  // 16-bit operand packs (either type)
// While one is alive on this thread, t16_pack() calls on `stream` are collected and launched TOGETHER by flush() (or at the scope's
// end); ot != OP_F32: the packs are written as 16-bit elements of that type (the first half of each dst).
struct T16PackScope {
  T16PackScope(OpType ot, hipStream_t stream);
  ~T16PackScope();
  int flush();
  T16PackScope(const T16PackScope&) = delete;
  T16PackScope& operator=(const T16PackScope&) = delete;
 private:
  OpType prev_;
  bool prev_active_;
};
// dst = T16 operand layout (see wave_gemm16) of the [R,K] matrix M[r][k] = src[r * rs + k * cs]; R, K multiples of 16.
int t16_pack(const float* src, long rs, long cs, int R, int K, float* dst, hipStream_t stream);
inline int t16_pack_rows(const float* W, int ldw, int R, int K, float* dst, hipStream_t s) { return t16_pack(W, ldw, 1, R, K, dst, s); }
// the transpose of X[:M,:N] (row stride ldx): a [N,M] matrix
inline int t16_pack_transposed(const float* X, int ldx, int M, int N, float* dst, hipStream_t s) { return t16_pack(X, 1, ldx, N, M, dst, s); }

}  // namespace blvm
