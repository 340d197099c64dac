// editdist.hip — K9: batched Levenshtein distance between integer sequences, with an optional token -> unit expansion, and the batch
// sums the error-rate metrics need.  The probe's word and character error rates without a trip to the host (DESIGN "K9").
//
// edit_distance_kernel: one wave per (row, table), the shape of ctc_ab_kernel.  With D[i][j] the distance between the first i
// reference units and the first j hypothesis units, the hypothesis is walked in strips of EDIT_STRIP = 64 * EDIT_NS columns, lane l
// owning the EDIT_NS columns l * EDIT_NS .. of the strip in registers.  The walk is skewed along anti-diagonals: at step s lane l
// works on row s - l, takes D[row][its first column - 1] from lane l - 1 by __shfl_up (lane 0: from the strip's boundary column in
// LDS) and keeps the diagonal from the step before; the step's reference unit and boundary value are loaded one step ahead (they do
// not depend on the recursion).  Lane 63 writes the strip's last column back over the boundary column, in place:
// it stores row s - 63 after lane 0 has loaded row s + 1.  The expanded reference (at most EDIT_MAX_REF units) is built once in LDS, the
// expanded hypothesis one strip at a time; no expanded sequence ever goes to global memory.  No atomics; every output element is
// written by exactly one lane on every call.
// edit_totals_kernel: one wave per table sums the rows in a fixed order.
#include "common.h"

namespace blvm {
namespace {

constexpr int EDIT_NS = 8;               // columns per lane
constexpr int EDIT_STRIP = 64 * EDIT_NS; // hypothesis units per strip
constexpr int EDIT_MAX_REF = 8192;       // expanded reference units: CTC_MAX_L = 512 labels of 15 units and a separator

struct EditTable {
  const int32_t* off;    // [V + 1] CSR offsets into units, NULL: the sequences are compared as they are
  const int32_t* units;
  int V, sep;            // sep < 0: no separator between consecutive tokens
};

__device__ __forceinline__ int wave_sum(int v) {
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

// expanded length of seq[0 .. n); bad is raised by a token outside [0, V), which is never used as an index
__device__ int expanded_length(const EditTable& tb, const int32_t* __restrict__ seq, int n, int lane, bool& bad) {
  if (!tb.off) return n;
  int total = 0;
  for (int i = lane; i < n; i += 64) {
    const int tok = seq[i];
    if (tok < 0 || tok >= tb.V) bad = true;
    else total += tb.off[tok + 1] - tb.off[tok];
  }
  total = wave_sum(total);
  if (tb.sep >= 0 && n > 0) total += n - 1;
  return total;
}

// Writes the units at positions [w0, w0 + W) of the expansion of seq[0 .. n) to buf[0 .. W).  (tk, pos): a token that starts at or
// before w0 and its position in the expansion, both wave-uniform; they advance 64 tokens at a time and stay on the chunk that reaches
// the window's end, so that the next window starts from there.  Every token of seq has passed expanded_length's check.
__device__ void expand_window(const EditTable& tb, const int32_t* __restrict__ seq, int n, int w0, int W, int* buf, int& tk, int& pos,
                              int lane) {
  while (tk < n) {
    const int i = tk + lane;
    const bool in = i < n;
    const int tok = in ? seq[i] : 0;
    int base = 0, cnt = in ? 1 : 0;
    if (in && tb.off) { base = tb.off[tok]; cnt = max(tb.off[tok + 1] - base, 0); }
    const bool sep = in && tb.sep >= 0 && i + 1 < n;
    const int len = cnt + (sep ? 1 : 0);
    int inc = len;  // inclusive prefix sum over the lanes
    for (int d = 1; d < 64; d <<= 1) {
      const int v = __shfl_up(inc, d, 64);
      if (lane >= d) inc += v;
    }
    const int start = pos + inc - len;
    if (start < w0 + W && start + len > w0) {
      for (int k = 0; k < cnt; ++k) {
        const int p = start + k - w0;
        if (p >= 0 && p < W) buf[p] = tb.off ? tb.units[base + k] : tok;
      }
      const int p = start + cnt - w0;
      if (sep && p >= 0 && p < W) buf[p] = tb.sep;
    }
    const int chunk = __shfl(inc, 63, 64);
    if (pos + chunk >= w0 + W) break;
    pos += chunk;
    tk += 64;
  }
}

__global__ __launch_bounds__(64) void edit_distance_kernel(const int32_t* __restrict__ ref, const int32_t* __restrict__ ref_len,
                                                           int ref_stride, const int32_t* __restrict__ hyp,
                                                           const int32_t* __restrict__ hyp_len, int hyp_stride, int B, int V,
                                                           const int32_t* __restrict__ unit_offsets, const int32_t* __restrict__ units,
                                                           const int32_t* __restrict__ separators, int ref_cap,
                                                           int32_t* __restrict__ edits, int32_t* __restrict__ ref_units) {
  extern __shared__ int lds[];
  int* refu = lds;                      // [ref_cap] the expanded reference
  int* left = lds + ref_cap;            // [ref_cap + 1] D[i][first column of the strip - 1]
  int* hs = lds + 2 * ref_cap + 1;      // [EDIT_STRIP] the strip's hypothesis units
  const int b = blockIdx.x, tbl = blockIdx.y, lane = threadIdx.x;
  const size_t o = (size_t)tbl * B + b;
  EditTable tb;
  tb.off = unit_offsets ? unit_offsets + (size_t)tbl * (V + 1) : nullptr;
  tb.units = units;
  tb.V = V;
  tb.sep = unit_offsets ? separators[tbl] : -1;
  const int32_t* rs = ref + (size_t)b * ref_stride;
  const int32_t* hy = hyp + (size_t)b * hyp_stride;
  const int rl = ref_len[b], hl = hyp_len[b];
  bool bad = rl < 0 || rl > ref_stride || hl < 0 || hl > hyp_stride;
  int R = 0, H = 0;
  if (!bad) {
    R = expanded_length(tb, rs, rl, lane, bad);
    H = expanded_length(tb, hy, hl, lane, bad);
  }
  R = __builtin_amdgcn_readfirstlane(R);  // the sums are the same in every lane: say so, the loops below are then scalar
  H = __builtin_amdgcn_readfirstlane(H);
  bad = __any(bad) || R > ref_cap;  // wave-uniform from here on
  if (bad || R == 0 || H == 0) {
    if (lane == 0) {
      edits[o] = bad ? -1 : max(R, H);
      ref_units[o] = bad ? -1 : R;
    }
    return;
  }

  {
    int tk = 0, pos = 0;
    expand_window(tb, rs, rl, 0, R, refu, tk, pos, lane);
  }
  for (int i = lane; i <= R; i += 64) left[i] = i;

  int tk = 0, pos = 0, result = 0;
  for (int j0 = 0; j0 < H; j0 += EDIT_STRIP) {
    const int cols = min(H - j0, EDIT_STRIP), lanes = (cols + EDIT_NS - 1) / EDIT_NS;
    __syncthreads();  // one wave: the previous strip's loads of hs are done (and, first trip, refu and left are written)
    expand_window(tb, hy, hl, j0, cols, hs, tk, pos, lane);
    __syncthreads();
    int h[EDIT_NS], cur[EDIT_NS];
#pragma unroll
    for (int k = 0; k < EDIT_NS; ++k) {
      const int c = lane * EDIT_NS + k;
      h[k] = c < cols ? hs[c] : 0;  // columns past the hypothesis' end feed nothing to their left
      cur[k] = j0 + c + 1;          // D[0][column]
    }
    int last = 0;                     // D[row][this lane's last column] after its latest step
    int diag0 = j0 + lane * EDIT_NS;  // D[row - 1][this lane's first column - 1]
    const int steps = R + lanes - 1;
    // the reference unit and the boundary value of a step do not depend on the step before: they are loaded one step ahead
    int r_next = refu[min(max(-lane, 0), R - 1)], left_next = left[1];
    for (int s = 1; s <= steps; ++s) {
      const int i = s - lane;
      const bool active = i >= 1 && i <= R && lane < lanes;
      const int r = r_next, lf = left_next;
      r_next = refu[min(max(i, 0), R - 1)];
      left_next = left[min(s + 1, R)];
      const int below = __shfl_up(last, 1, 64);
      if (active) {
        // D[i][c_k] = min(a_k, D[i][c_k - 1] + 1) with a_k = min(D[i-1][c_k] + 1, D[i-1][c_k - 1] + (r != h_k)), which does not depend
        // on this row; unrolled over the lane's columns, D[i][c_k] = min(p_k, in + k + 1) with p_k = min(a_k, p_(k-1) + 1).  Only
        // that last min waits for the neighbour's value: the shuffle's latency is spent on the p_k.
        int p[EDIT_NS];
        p[0] = min(cur[0] + 1, diag0 + (r != h[0] ? 1 : 0));
#pragma unroll
        for (int k = 1; k < EDIT_NS; ++k) p[k] = min(min(cur[k] + 1, cur[k - 1] + (r != h[k] ? 1 : 0)), p[k - 1] + 1);
        const int in = lane == 0 ? lf : below;
#pragma unroll
        for (int k = 0; k < EDIT_NS; ++k) cur[k] = min(p[k], in + k + 1);
        last = cur[EDIT_NS - 1];
        diag0 = in;
        if (lane == 63) left[i] = last;
      }
    }
    if (j0 + EDIT_STRIP >= H) {
      const int c = cols - 1;
      int v = cur[0];
#pragma unroll
      for (int k = 1; k < EDIT_NS; ++k)
        if (c % EDIT_NS == k) v = cur[k];
      result = __shfl(v, c / EDIT_NS, 64);
    }
  }
  if (lane == 0) {
    edits[o] = result;
    ref_units[o] = R;
  }
}

// totals[t] = (sum of edits, sum of ref_units, number of refused rows) over the rows of table t; refused rows add to neither sum
__global__ __launch_bounds__(64) void edit_totals_kernel(const int32_t* __restrict__ edits, const int32_t* __restrict__ ref_units, int B,
                                                         int32_t* __restrict__ totals) {
  const int t = blockIdx.x, lane = threadIdx.x;
  int e = 0, r = 0, bad = 0;
  for (int b = lane; b < B; b += 64) {
    const int v = edits[(size_t)t * B + b];
    if (v < 0) ++bad;
    else { e += v; r += ref_units[(size_t)t * B + b]; }
  }
  e = wave_sum(e);
  r = wave_sum(r);
  bad = wave_sum(bad);
  if (lane == 0) {
    totals[3 * t] = e;
    totals[3 * t + 1] = r;
    totals[3 * t + 2] = bad;
  }
}

}  // namespace
}  // namespace blvm

using namespace blvm;

extern "C" int blvm_edit_distance(const int32_t* ref, const int32_t* ref_len, int ref_stride, const int32_t* hyp, const int32_t* hyp_len,
                                  int hyp_stride, int B, int n_tables, int V, const int32_t* unit_offsets, const int32_t* units,
                                  const int32_t* separators, int max_units, int32_t* edits, int32_t* ref_units, int32_t* totals,
                                  void* stream) {
  BLVM_REQUIRE(B >= 1 && ref_stride >= 0 && hyp_stride >= 0, "blvm_edit_distance: B = %d, ref_stride = %d, hyp_stride = %d: need B >= 1 and strides >= 0",
               B, ref_stride, hyp_stride);
  BLVM_REQUIRE(n_tables >= 0 && n_tables <= 65535, "blvm_edit_distance: n_tables = %d: need 0 (no expansion) to 65535", n_tables);
  BLVM_REQUIRE(ref_len && hyp_len && edits && ref_units, "blvm_edit_distance: NULL ref_len, hyp_len, edits or ref_units");
  BLVM_REQUIRE((ref || ref_stride == 0) && (hyp || hyp_stride == 0), "blvm_edit_distance: NULL ref or hyp with a stride above 0");
  size_t per_token = 1;  // most units a token can add to its sequence
  bool any_sep = false;
  if (n_tables > 0) {
    BLVM_REQUIRE(unit_offsets && separators && V >= 1 && max_units >= 0, "blvm_edit_distance: %d table(s) need unit_offsets, separators, V >= 1 and max_units >= 0 (V = %d, max_units = %d)",
                 n_tables, V, max_units);
    BLVM_REQUIRE(units || max_units == 0, "blvm_edit_distance: NULL units with max_units = %d", max_units);
    per_token = (size_t)max_units + 1;
    any_sep = true;
  }
  const size_t ref_bound = ref_stride == 0 ? 0 : (size_t)ref_stride * per_token - (any_sep ? 1 : 0);
  BLVM_REQUIRE(ref_bound <= (size_t)EDIT_MAX_REF, "blvm_edit_distance: a reference row may expand to %zu units (%d tokens of up to %d units and a separator): at most %d are supported",
               ref_bound, ref_stride, n_tables > 0 ? max_units : 1, EDIT_MAX_REF);
  BLVM_REQUIRE((size_t)hyp_stride * per_token < ((size_t)1 << 30), "blvm_edit_distance: a hypothesis row may expand to %zu units: need fewer than 2^30",
               (size_t)hyp_stride * per_token);
  BLVM_REQUIRE((size_t)B * (n_tables > 0 ? n_tables : 1) < ((size_t)1 << 31), "blvm_edit_distance: B * n_tables = %zu: need fewer than 2^31",
               (size_t)B * (n_tables > 0 ? n_tables : 1));
  hipStream_t s = (hipStream_t)stream;
  const int nt = n_tables > 0 ? n_tables : 1, ref_cap = (int)ref_bound;
  const size_t lds = sizeof(int) * (2 * (size_t)ref_cap + 1 + EDIT_STRIP);
  if (lds > 64 * 1024)
    BLVM_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(edit_distance_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  hipLaunchKernelGGL(edit_distance_kernel, dim3(B, nt), dim3(64), lds, s, ref, ref_len, ref_stride, hyp, hyp_len, hyp_stride, B, V,
                     n_tables > 0 ? unit_offsets : nullptr, units, separators, ref_cap, edits, ref_units);
  BLVM_CHECK_LAUNCH("edit_distance_kernel");
  if (totals) {
    hipLaunchKernelGGL(edit_totals_kernel, dim3(nt), dim3(64), 0, s, edits, ref_units, B, totals);
    BLVM_CHECK_LAUNCH("edit_totals_kernel");
  }
  return BLVM_OK;
}
