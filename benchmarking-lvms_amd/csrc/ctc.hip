// ctc.hip — K9: CTC loss on un-normalised logits (log-softmax fused), its gradient wrt the logits, and the greedy decode.
//
// Three launches for loss + gradient (DESIGN "K9"):
//   1. ctc_lse_kernel: one wave per (t, b) row, lse[t,b] = log sum_c exp(logits[t,b,c]).  No [T,B,C] log-probability tensor exists.
//   2. ctc_ab_kernel<NS>: one workgroup per utterance; wave 0 runs the alpha recursion, wave 1 the beta recursion, concurrently.
//      The S = 2 L + 1 extended-label states are lane-contiguous in registers (lane l owns states l*NS .. l*NS+NS-1), neighbours
//      come by cross-lane moves, and since ONE wave owns all states of its direction no state ever crosses a wave boundary: there
//      is no LDS and no barrier in the serial part.  A step's emission loads do not depend on the recursion and are issued ahead of its
//      arithmetic (beta: one step ahead); a ring of registers running four steps ahead measured slower (DESIGN "K9").
//      beta is kept WITHOUT the emission of its own step, so alpha_t(s) + beta_t(s) + nll is the log posterior of state s at t.
//   3. ctc_grad_kernel: fully parallel over (b, tile of t): one wave per row forms softmax - occupation.  The occupation of a
//      class is the sum over the states that carry it, walked in a fixed order through a per-utterance list built in LDS; the
//      blank's even states are summed lane-strided and combined by a butterfly.  No atomics: bit-identical from call to call.
#include <math.h>

#include "common.h"

namespace blvm {
namespace {

constexpr int CTC_MAX_L = 512;   // labels per row: S <= 1025 states = 17 per lane
constexpr int CTC_MAX_C = 4096;  // classes: the gradient kernel keeps one list head per class in LDS
constexpr int CTC_ROWS = 16;     // time steps per workgroup of the gradient kernel

__device__ __forceinline__ float neg_inf() { return -INFINITY; }

__device__ __forceinline__ float lse3(float a, float b, float c) {
  const float m = fmaxf(a, fmaxf(b, c));
  if (m == neg_inf()) return m;
  return m + log_(exp_(a - m) + exp_(b - m) + exp_(c - m));
}

// ---- 1. per-step log-sum-exp ----------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void ctc_lse_kernel(const float* __restrict__ logits, size_t rows, int C, float* __restrict__ lse) {
  const int lane = threadIdx.x & 63;
  const size_t row = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  const float* x = logits + row * C;
  float m = neg_inf();
  for (int c = lane; c < C; c += 64) m = fmaxf(m, x[c]);
  for (int off = 32; off > 0; off >>= 1) m = fmaxf(m, __shfl_xor(m, off, 64));
  float s = 0.f;
  for (int c = lane; c < C; c += 64) s += exp_(x[c] - m);
  for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off, 64);
  if (lane == 0) lse[row] = m + log_(s);
}

// ---- 2. the two recursions ---------------------------------------------------------------------------------------------------------
// extended label of state s of row b: blank at even s, targets[(s-1)/2] at odd s.  `bad` is raised by a label outside [0,C), which
// is then replaced by the blank so that it is never used as an index.
__device__ __forceinline__ int ext_label(const int32_t* __restrict__ tg, int s, int C, int blank, bool& bad) {
  if (!(s & 1)) return blank;
  const int l = tg[s >> 1];
  if (l < 0 || l >= C) { bad = true; return blank; }
  return l;
}

template <int NS>
__global__ __launch_bounds__(128) void ctc_ab_kernel(const float* __restrict__ logits, const int32_t* __restrict__ targets,
                                                     const int32_t* __restrict__ input_lens, const int32_t* __restrict__ target_lens,
                                                     int T, int B, int C, int Lmax, int blank, const float* __restrict__ lse,
                                                     float* __restrict__ alpha, float* __restrict__ beta, float* __restrict__ nll) {
  const int b = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int il = input_lens[b], tl = target_lens[b];
  const bool bad_len = il < 0 || il > T || tl < 0 || tl > Lmax;
  const int S = bad_len ? 1 : 2 * tl + 1, Sp = 2 * Lmax + 1;
  const int32_t* tg = targets + (size_t)b * Lmax;

  int lab[NS];
  bool ok[NS], skip[NS];  // skip: alpha may come from s - 2 (wave 0) | beta may go to s + 2 (wave 1)
  bool bad = false;
#pragma unroll
  for (int j = 0; j < NS; ++j) {
    const int s = lane * NS + j;
    ok[j] = s < S;
    lab[j] = ok[j] ? ext_label(tg, s, C, blank, bad) : blank;
    if (wave == 0) skip[j] = ok[j] && s >= 2 && lab[j] != ext_label(tg, s - 2, C, blank, bad);
    else skip[j] = s + 2 < S && lab[j] != ext_label(tg, s + 2, C, blank, bad);
  }
  bad = __any(bad) || bad_len;
  if (bad || il == 0) {  // nothing to recurse over: NaN marks a refused row for the gradient kernel
    if (threadIdx.x == 0) nll[b] = bad ? NAN : (tl == 0 ? 0.f : INFINITY);
    return;
  }

  const size_t step = (size_t)B * C;
  const float* lg = logits + (size_t)b * C;
  const float* ls = lse + b;
  float* const dst = (wave == 0 ? alpha : beta) + (size_t)b * T * Sp + (size_t)lane * NS;
  float a[NS], e[NS], raw[NS];

  if (wave == 0) {
    float l0 = ls[0];
#pragma unroll
    for (int j = 0; j < NS; ++j) e[j] = ok[j] ? lg[lab[j]] - l0 : 0.f;
#pragma unroll
    for (int j = 0; j < NS; ++j) {
      const int s = lane * NS + j;
      a[j] = (ok[j] && s < 2) ? e[j] : neg_inf();
      if (ok[j]) dst[j] = a[j];
    }
    for (int t = 1; t < il; ++t) {
      // this step's emissions do not depend on alpha: their loads are issued first and land under the step's arithmetic
      const float* row = lg + (size_t)t * step;
      const float lt = ls[(size_t)t * B];
#pragma unroll
      for (int j = 0; j < NS; ++j) raw[j] = ok[j] ? row[lab[j]] : 0.f;
      // states s - 1 and s - 2 of this lane's first state live in the lane below
      float p1 = __shfl_up(a[NS - 1], 1, 64), p2 = NS >= 2 ? __shfl_up(a[NS >= 2 ? NS - 2 : 0], 1, 64) : __shfl_up(a[0], 2, 64);
      if (lane < 1) p1 = neg_inf();
      if (lane < (NS >= 2 ? 1 : 2)) p2 = neg_inf();
      float n[NS];
#pragma unroll
      for (int j = 0; j < NS; ++j) {
        const float x1 = j >= 1 ? a[j >= 1 ? j - 1 : 0] : p1;
        const float x2 = j >= 2 ? a[j >= 2 ? j - 2 : 0] : (j == 1 ? p1 : p2);
        n[j] = ok[j] ? lse3(a[j], x1, skip[j] ? x2 : neg_inf()) + (raw[j] - lt) : neg_inf();
      }
      float* o = dst + (size_t)t * Sp;
#pragma unroll
      for (int j = 0; j < NS; ++j) {
        a[j] = n[j];
        if (ok[j]) o[j] = a[j];
      }
    }
    // nll = -log(alpha(S-1) + alpha(S-2)) at the row's last frame
    float v1 = neg_inf(), v2 = neg_inf();
    {
      const int s1 = S - 1, s2 = S - 2;
      float x1 = a[0], x2 = a[0];
#pragma unroll
      for (int j = 1; j < NS; ++j) {
        if (s1 % NS == j) x1 = a[j];
        if (s2 >= 0 && s2 % NS == j) x2 = a[j];
      }
      v1 = __shfl(x1, s1 / NS, 64);
      if (s2 >= 0) v2 = __shfl(x2, s2 / NS, 64);
    }
    if (lane == 0) nll[b] = -lse3(v1, v2, neg_inf());
  } else {
    // beta_t(s) = log P(labels after t | state s at t), the emission at t left out
#pragma unroll
    for (int j = 0; j < NS; ++j) {
      const int s = lane * NS + j;
      a[j] = (ok[j] && s >= S - 2) ? 0.f : neg_inf();
      if (ok[j]) dst[(size_t)(il - 1) * Sp + j] = a[j];
    }
    if (il < 2) return;
    {
      const float* row = lg + (size_t)(il - 1) * step;
      const float lt = ls[(size_t)(il - 1) * B];
#pragma unroll
      for (int j = 0; j < NS; ++j) e[j] = ok[j] ? row[lab[j]] - lt : 0.f;
    }
    for (int t = il - 2; t >= 0; --t) {
      // the emissions of step t, needed by the NEXT trip
      const float* row = lg + (size_t)t * step;
      const float lt = ls[(size_t)t * B];
#pragma unroll
      for (int j = 0; j < NS; ++j) raw[j] = ok[j] ? row[lab[j]] : 0.f;
      float x[NS];
#pragma unroll
      for (int j = 0; j < NS; ++j) x[j] = a[j] + e[j];  // through state s at t + 1, its emission included
      float q1 = __shfl_down(x[0], 1, 64), q2 = NS >= 2 ? __shfl_down(x[NS >= 2 ? 1 : 0], 1, 64) : __shfl_down(x[0], 2, 64);
      if (lane > 62) q1 = neg_inf();
      if (lane > (NS >= 2 ? 62 : 61)) q2 = neg_inf();
      float* o = dst + (size_t)t * Sp;
#pragma unroll
      for (int j = 0; j < NS; ++j) {
        const float x1 = j + 1 < NS ? x[j + 1 < NS ? j + 1 : 0] : q1;
        const float x2 = j + 2 < NS ? x[j + 2 < NS ? j + 2 : 0] : (j + 2 == NS ? q1 : q2);
        a[j] = ok[j] ? lse3(x[j], x1, skip[j] ? x2 : neg_inf()) : neg_inf();
        if (ok[j]) o[j] = a[j];
      }
#pragma unroll
      for (int j = 0; j < NS; ++j) e[j] = ok[j] ? raw[j] - lt : 0.f;
    }
  }
}

// ---- 3. gradient: softmax - occupation ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void ctc_grad_kernel(const float* __restrict__ logits, const int32_t* __restrict__ targets,
                                                       const int32_t* __restrict__ input_lens, const int32_t* __restrict__ target_lens,
                                                       int T, int B, int C, int Lmax, int blank, int tiles, const float* __restrict__ lse,
                                                       const float* __restrict__ alpha, const float* __restrict__ beta,
                                                       const float* __restrict__ nll, const float* __restrict__ d_nll,
                                                       float* __restrict__ d_logits) {
  extern __shared__ int lds[];
  int* tg = lds;               // [Lmax] the row's labels
  int* prev = lds + Lmax;      // [Lmax] previous position with the same label, -1 at a chain's end
  int* head = lds + 2 * Lmax;  // [C] last position of each label, -1: the label does not occur
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int b = blockIdx.x / tiles, t0 = (blockIdx.x % tiles) * CTC_ROWS;
  const int t1 = min(t0 + CTC_ROWS, T);
  const int il = min(max(input_lens[b], 0), T);
  const float nl = nll[b];
  const bool finite = isfinite(nl);  // a finite nll: lengths and labels passed the recursion kernel's checks
  const int tl = finite ? min(max(target_lens[b], 0), Lmax) : 0;
  const bool walk = finite && t0 < il;  // uniform over the workgroup
  if (walk) {
    for (int c = tid; c < C; c += 256) head[c] = -1;
    for (int i = tid; i < tl; i += 256) tg[i] = targets[(size_t)b * Lmax + i];
  }
  __syncthreads();
  if (walk) {
    for (int i = tid; i < tl; i += 256) {
      const int ti = tg[i];
      int p = -1;
      bool later = false;
      for (int k = 0; k < tl; ++k) {
        if (tg[k] != ti) continue;
        if (k < i) p = k;
        if (k > i) later = true;
      }
      prev[i] = p;
      if (!later && ti >= 0 && ti < C) head[ti] = i;
    }
  }
  __syncthreads();
  const float g = d_nll ? d_nll[b] : 1.f;
  const int Sp = 2 * Lmax + 1;
  for (int t = t0 + wave; t < t1; t += 4) {
    const size_t r = (size_t)t * B + b;
    float* out = d_logits + r * C;
    if (t >= il) {
      for (int c = lane; c < C; c += 64) out[c] = 0.f;
      continue;
    }
    if (!finite) {
      for (int c = lane; c < C; c += 64) out[c] = NAN;
      continue;
    }
    const float* al = alpha + ((size_t)b * T + t) * Sp;
    const float* be = beta + ((size_t)b * T + t) * Sp;
    float occ_blank = 0.f;
    for (int k = lane; k <= tl; k += 64) occ_blank += exp_(al[2 * k] + be[2 * k] + nl);
    for (int off = 32; off > 0; off >>= 1) occ_blank += __shfl_xor(occ_blank, off, 64);
    const float* x = logits + r * C;
    const float lt = lse[r];
    for (int c = lane; c < C; c += 64) {
      float occ = c == blank ? occ_blank : 0.f;
      for (int i = head[c]; i >= 0; i = prev[i]) occ += exp_(al[2 * i + 1] + be[2 * i + 1] + nl);
      out[c] = g * (exp_(x[c] - lt) - occ);
    }
  }
}

// ---- greedy decode -----------------------------------------------------------------------------------------------------------------
// one workgroup per utterance: the four waves take the arg-max of the frames (lowest index wins a tie) into hyp[b,:], then wave 0
// collapses repeats and drops blanks in place, 64 frames a trip (a trip's loads all precede its stores, and it stores at or
// below the positions it loaded)
__global__ __launch_bounds__(256) void ctc_greedy_kernel(const float* __restrict__ logits, const int32_t* __restrict__ input_lens, int T,
                                                         int B, int C, int blank, int32_t* __restrict__ hyp,
                                                         int32_t* __restrict__ hyp_lens) {
  const int b = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int il = min(max(input_lens[b], 0), T);
  int32_t* h = hyp + (size_t)b * T;
  for (int t = wave; t < il; t += 4) {
    const float* x = logits + ((size_t)t * B + b) * C;
    float best = neg_inf();
    int at = INT_MAX;
    if (lane < C) { best = x[lane]; at = lane; }
    for (int c = lane + 64; c < C; c += 64) {
      const float v = x[c];
      if (v > best) { best = v; at = c; }
    }
    for (int off = 32; off > 0; off >>= 1) {
      const float ov = __shfl_xor(best, off, 64);
      const int oa = __shfl_xor(at, off, 64);
      if (ov > best || (ov == best && oa < at)) { best = ov; at = oa; }
    }
    if (lane == 0) h[t] = at;
  }
  __syncthreads();
  if (wave != 0) return;
  int count = 0, last = -1;  // last: the arg-max of the frame before this trip's first
  for (int base = 0; base < il; base += 64) {
    const int t = base + lane;
    const int p = t < il ? h[t] : -1;
    int before = __shfl_up(p, 1, 64);
    if (lane == 0) before = last;
    const bool keep = t < il && p != blank && (t == 0 || p != before);
    const unsigned long long m = __ballot(keep);
    last = __shfl(p, 63, 64);
    if (keep) h[count + __popcll(m & ((1ull << lane) - 1ull))] = p;
    count += __popcll(m);
  }
  for (int k = count + lane; k < T; k += 64) h[k] = -1;
  if (lane == 0) hyp_lens[b] = count;
}

int check_shape(const char* who, int T, int B, int C, int blank) {
  BLVM_REQUIRE(T >= 1 && B >= 1 && C >= 2, "%s: T = %d, B = %d, C = %d: need T >= 1, B >= 1, C >= 2", who, T, B, C);
  BLVM_REQUIRE(blank >= 0 && blank < C, "%s: blank = %d is outside [0, C = %d)", who, blank, C);
  return BLVM_OK;
}

struct CtcScratch {
  float *lse, *alpha, *beta;
  size_t floats;
  CtcScratch(float* base, int T, int B, int Lmax) {
    Arena ar{base};
    const size_t states = (size_t)B * T * (2 * (size_t)Lmax + 1);
    lse = ar.take((size_t)T * B);
    alpha = ar.take(states);
    beta = ar.take(states);
    floats = ar.floats();
  }
};

}  // namespace
}  // namespace blvm

using namespace blvm;

extern "C" size_t blvm_ctc_scratch_floats(int T, int B, int C, int Lmax) {
  (void)C;
  if (T < 1 || B < 1 || Lmax < 0) return 0;
  return CtcScratch(nullptr, T, B, Lmax).floats;
}

extern "C" int blvm_ctc_loss(const float* logits, const int32_t* targets, const int32_t* input_lens, const int32_t* target_lens, int T,
                             int B, int C, int Lmax, int blank, const float* d_nll, float* nll, float* d_logits, float* scratch,
                             void* stream) {
  BLVM_TRY(check_shape("blvm_ctc_loss", T, B, C, blank));
  BLVM_REQUIRE(Lmax >= 0 && Lmax <= CTC_MAX_L, "blvm_ctc_loss: Lmax = %d: at most %d labels per row are supported", Lmax, CTC_MAX_L);
  BLVM_REQUIRE(C <= CTC_MAX_C, "blvm_ctc_loss: C = %d: at most %d classes are supported", C, CTC_MAX_C);
  BLVM_REQUIRE((size_t)T * B < ((size_t)1 << 31), "blvm_ctc_loss: T * B = %zu rows: need fewer than 2^31", (size_t)T * B);
  BLVM_REQUIRE(logits && input_lens && target_lens && nll && scratch, "blvm_ctc_loss: NULL logits, lengths, nll or scratch");
  BLVM_REQUIRE(targets || Lmax == 0, "blvm_ctc_loss: NULL targets with Lmax = %d", Lmax);
  hipStream_t s = (hipStream_t)stream;
  const CtcScratch sc(scratch, T, B, Lmax);
  const size_t rows = (size_t)T * B;
  hipLaunchKernelGGL(ctc_lse_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, s, logits, rows, C, sc.lse);
  BLVM_CHECK_LAUNCH("ctc_lse_kernel");
  const int per_lane = (2 * Lmax + 1 + 63) / 64;
  const dim3 block(d_logits ? 128 : 64);  // loss only: the alpha wave alone
#define CTC_AB(NS_)                                                                                                               \
  hipLaunchKernelGGL(ctc_ab_kernel<NS_>, dim3(B), block, 0, s, logits, targets, input_lens, target_lens, T, B, C, Lmax, blank,   \
                     sc.lse, sc.alpha, sc.beta, nll)
  if (per_lane <= 1) CTC_AB(1);
  else if (per_lane <= 2) CTC_AB(2);
  else if (per_lane <= 3) CTC_AB(3);
  else if (per_lane <= 5) CTC_AB(5);
  else if (per_lane <= 9) CTC_AB(9);
  else CTC_AB(17);
#undef CTC_AB
  BLVM_CHECK_LAUNCH("ctc_ab_kernel");
  if (d_logits) {
    const int tiles = (T + CTC_ROWS - 1) / CTC_ROWS;
    const size_t lds = sizeof(int) * (2 * (size_t)Lmax + C);
    hipLaunchKernelGGL(ctc_grad_kernel, dim3((unsigned)((size_t)tiles * B)), dim3(256), lds, s, logits, targets, input_lens, target_lens,
                       T, B, C, Lmax, blank, tiles, sc.lse, sc.alpha, sc.beta, nll, d_nll, d_logits);
    BLVM_CHECK_LAUNCH("ctc_grad_kernel");
  }
  return BLVM_OK;
}

extern "C" int blvm_ctc_greedy(const float* logits, const int32_t* input_lens, int T, int B, int C, int blank, int32_t* hyp,
                               int32_t* hyp_lens, void* stream) {
  BLVM_TRY(check_shape("blvm_ctc_greedy", T, B, C, blank));
  BLVM_REQUIRE(logits && input_lens && hyp && hyp_lens, "blvm_ctc_greedy: NULL logits, input_lens, hyp or hyp_lens");
  hipLaunchKernelGGL(ctc_greedy_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, logits, input_lens, T, B, C, blank, hyp, hyp_lens);
  BLVM_CHECK_LAUNCH("ctc_greedy_kernel");
  return BLVM_OK;
}
