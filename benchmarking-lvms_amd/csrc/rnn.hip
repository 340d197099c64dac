// rnn.hip — K4 / K2: single-layer LSTM and GRU over a whole sequence (forward + BPTT) as stage-kernel chains.
//
// Replaces the vendor RNN calls of the reference:
//   nn.LSTM on a packed sequence        blvm/models/lstm.py:46-55,96-98   (pack_padded_sequence semantics via `lens`)
//   nn.GRU forward / time-reversed      blvm/models/srnn.py:113-116,196,200-206 (reverse_sequences folded into an
//                                        index map: operations.py:56-87 — per-row reversal, right padding in place)
// One launch per recurrent step in each direction: the hidden projection (M = batch, K = hidden) runs on
// v_mfma_f32_16x16x4_f32 with the K split over the waves of a workgroup, and ALL gate math (forward) / gate
// derivatives (backward, fused into the dgrad that completes dL/dh of the step) lives in the epilogue.  The input
// projection and every weight gradient are hoisted out of the loop into the big MFMA GEMM (gemm.hip).
#include "common.h"
#include "pchain.h"
#include "seqchain.h"

#include <atomic>

namespace blvm {
namespace {

inline int pick_nw(int K, int groups) {
  const int chunks = (K / 16) * groups;
  if (chunks > 32) return 16;
  if (chunks > 16) return 8;
  return 4;
}

inline int pick_split(int M, int N, int K) { return gemm_pick_split(M, N, K); }

// time index processed by row `b` at recurrence step j: forward j; reversed: len-1-j inside the row's length, j in
// the right padding (reverse_sequences leaves padding where it is).
__device__ __forceinline__ int time_index(int j, int reverse, const int32_t* lens, int row) {
  if (!reverse) return j;
  const int n = lens[row];
  return j < n ? n - 1 - j : j;
}

// ===================================================================================================================
// LSTM
// ===================================================================================================================
struct LstmFwdArgs {
  const float *hprev, *cprev;   // [B,H]
  const float* Whh;             // [4H,H] rows [i|f|g|o], in T16 (common.h)
  const float* bhh;             // [4H]
  const float* xg;              // [B,4H] input projection incl. b_ih
  const int32_t* lens;          // [B] valid steps per row (packed-sequence semantics) or null
  float *hnext, *cnext;         // [B,H]
  float* out;                   // [B,H]   zero where the row is past its length (pad_packed_sequence)
  float* gates;                 // [B,4H]  saved i,f,g,o (zero where masked)
  int B, H, t;
};

template <int NW>
__global__ __launch_bounds__(NW * 64) void lstm_fwd_kernel(const float* hprev, const float* cprev, const float* Whh,
                                                           const float* bhh, const float* xg, const int32_t* lens, unsigned b_h,
                                                           int t_step, float* hnext, float* cnext, float* out, float* gates) {
  // scalar arguments (LstmFwdArgs documents them): the 6 input pointers, B:16|H:16 and the step are the 14 dwords the command
  // processor preloads into SGPRs (stages.h, launch-latency note 4); the outputs come by s_load
  const int B = b_h & 0xffff, H = b_h >> 16;
  __shared__ float red[4 * NW * 256];
  const int r0 = blockIdx.y * 16, c0 = blockIdx.x * 16, wave = threadIdx.x >> 6;
  const int t = threadIdx.x & 255;
  const int row = r0 + (t >> 4), col = c0 + (t & 15);
  const bool own = threadIdx.x < 256 && row < B;
  const int rowc = row < B ? row : r0;
  const size_t o = (size_t)rowc * H + col, o4 = (size_t)rowc * 4 * H + col;
  const float x0 = xg[o4] + bhh[col], x1 = xg[o4 + H] + bhh[H + col];
  const float x2 = xg[o4 + 2 * H] + bhh[2 * H + col], x3 = xg[o4 + 3 * H] + bhh[3 * H + col];
  const float hp = hprev[o], cp = cprev[o];
  const bool live = lens == nullptr || t_step < lens[rowc];
  f32x4 acc[4];
#pragma unroll
  for (int g = 0; g < 4; ++g) acc[g] = (f32x4){0.f, 0.f, 0.f, 0.f};
  {
    const float* const As[4] = {hprev, hprev, hprev, hprev};
    const float* const Ws[4] = {Whh, Whh, Whh, Whh};
    const int ld[4] = {H, H, H, H}, cs[4] = {c0, H + c0, 2 * H + c0, 3 * H + c0};
    wave_gemm16_multi<NW, 4, true>(As, ld, r0, B, Ws, ld, cs, H, wave, acc);
  }
  float v[4];
  reduce_tiles<4, NW>(acc, red, v);
  if (!own) return;
  const float i = sigmoidf_(v[0] + x0), f = sigmoidf_(v[1] + x1), g = tanhf(v[2] + x2), og = sigmoidf_(v[3] + x3);
  const float c2 = f * cp + i * g;
  const float h2 = og * tanhf(c2);
  cnext[o] = live ? c2 : cp;
  hnext[o] = live ? h2 : hp;
  out[o] = live ? h2 : 0.f;
  gates[o4] = live ? i : 0.f;
  gates[o4 + H] = live ? f : 0.f;
  gates[o4 + 2 * H] = live ? g : 0.f;
  gates[o4 + 3 * H] = live ? og : 0.f;
}

struct LstmBwdArgs {
  const float* DGn;     // [B,4H] gate pre-activation grads of step s+1 (unused when has_gemm == 0)
  const float* WhhT;    // [H,4H] in T16
  const float* dout;    // [B,H] grad wrt out_s
  const float* gates;   // [B,4H] step s
  const float *c_s, *c_s1;  // cell state entering / leaving step s
  float* DC;            // [B,H] running grad wrt the cell state (in/out)
  float* DG;            // [B,4H] out: gate pre-activation grads of step s
  float* dh0;           // [B,H] out when has_gates == 0
  int B, H, has_gemm, has_gates;
};

template <int NW>
__global__ __launch_bounds__(NW * 64) void lstm_bwd_kernel(const float* DGn, const float* WhhT, const float* dout,
                                                           const float* gates, const float* c_s, float* DC, unsigned b_h,
                                                           unsigned has, float* DG, float* dh0) {
  // scalar arguments (LstmBwdArgs documents them; c_s1 = c_s + B*H, consecutive steps of the saved cell states): 14 preloaded dwords
  const int B = b_h & 0xffff, H0 = b_h >> 16;
  const int has_gemm = has & 1, has_gates = (has >> 1) & 1;
  const float* c_s1 = c_s + (size_t)B * H0;
  __shared__ float red[NW * 256];
  const int r0 = blockIdx.y * 16, c0 = blockIdx.x * 16, H = H0;
  const int t = threadIdx.x & 255;
  const int row = r0 + (t >> 4), col = c0 + (t & 15);
  const bool own = threadIdx.x < 256 && row < B;
  const int rowc = row < B ? row : r0;
  const size_t o = (size_t)rowc * H + col, o4 = (size_t)rowc * 4 * H + col;
  float dh = 0.f, ig = 0.f, fg = 0.f, gg = 0.f, og = 0.f, cs = 0.f, cs1 = 0.f, dc = 0.f;
  if (has_gates) {  // wave-uniform
    dh = dout[o];
    ig = gates[o4]; fg = gates[o4 + H]; gg = gates[o4 + 2 * H]; og = gates[o4 + 3 * H];
    cs = c_s[o]; cs1 = c_s1[o]; dc = DC[o];
  }
  float v[1] = {0.f};
  if (has_gemm) {
    f32x4 acc[1] = {{0.f, 0.f, 0.f, 0.f}};
    acc[0] = wave_gemm16<NW, true>(DGn, 4 * H, r0, B, WhhT, 4 * H, c0, 4 * H, threadIdx.x >> 6, acc[0]);
    reduce_tiles<1, NW>(acc, red, v);
  }
  if (!own) return;
  dh += v[0];
  if (!has_gates) { dh0[o] = dh; return; }
  const float tc = tanhf(cs1);
  const float d_o = dh * tc;
  const float dct = dc + dh * og * (1.f - tc * tc);
  DG[o4] = dct * gg * ig * (1.f - ig);
  DG[o4 + H] = dct * cs * fg * (1.f - fg);
  DG[o4 + 2 * H] = dct * ig * (1.f - gg * gg);
  DG[o4 + 3 * H] = d_o * og * (1.f - og);
  DC[o] = dct * fg;
}

// sequences of at most this many rows may run as ONE persistent launch (pchain.h): their buffers get the T16 operand copies
inline size_t t16_rows(int B) { return (size_t)((B + 15) / 16) * 16; }
// Backward sequences take the register-resident kernel up to this K (= 3R | 4H).  At K >= 1536 a step is bound by every tile pulling
// the whole [B, K] gradient slab through the fabric (GRU R = 512: 12 MB per step); there the kernel reads the slab once per XCD
// (seqchain.hip, SHARED): GRU R = 512 backward 5.8 (engine tile) / 6.2 (every tile its own sc1 reads) -> ~5.5 us per step
constexpr int kSeqRegsMaxKBwd = 1536;
inline bool seq_persistent(int T, int B) { return pchain_applies(B) && device_cus() >= 32 && T >= 4; }

struct LstmReserve { float *XG, *Hs, *Cs, *GATES, *WhhP, *H16; };  // WhhP: T16 copy of Whh; H16: (T+1) T16 slabs of the state
size_t carve_lstm(float* base, int T, int B, int H, LstmReserve* r) {
  Arena ar{base};
  LstmReserve t;
  t.XG = ar.take((size_t)T * B * 4 * H);
  t.Hs = ar.take((size_t)(T + 1) * B * H);
  t.Cs = ar.take((size_t)(T + 1) * B * H);
  t.GATES = ar.take((size_t)T * B * 4 * H);
  t.WhhP = ar.take((size_t)4 * H * H);
  t.H16 = B <= kPchainCarveMaxB ? ar.take((size_t)(T + 1) * t16_rows(B) * H) : nullptr;
  if (r) *r = t;
  return ar.floats();
}
struct LstmWs { float *WhhT, *DG, *DC, *DG16; };
size_t carve_lstm_ws(float* base, int T, int B, int H, LstmWs* w) {
  Arena ar{base};
  LstmWs t;
  t.WhhT = ar.take((size_t)H * 4 * H);
  t.DG = ar.take((size_t)T * B * 4 * H);
  t.DC = ar.take((size_t)B * H);
  t.DG16 = B <= kPchainCarveMaxB ? ar.take((size_t)(T + 1) * t16_rows(B) * 4 * H) : nullptr;
  if (w) *w = t;
  return ar.floats();
}

// ===================================================================================================================
// GRU
// ===================================================================================================================
struct GruFwdArgs {
  const float* hprev;    // [B,R] state entering recurrence step j
  const float* Whh;      // [3R,R] rows [r|z|n], in T16
  const float* bhh;      // [3R]
  const float* xg;       // [T,B,3R] input projection incl. b_ih, TIME indexed
  const int32_t* lens;   // [B] (reverse map) or null
  float* hnext;          // [B,R]
  float* out;            // time-indexed output base: element (idx,row,col) at out + idx*out_ts + row*out_ld + col
  float *rg, *ug, *ng, *ghn;  // [B,R] saves of recurrence step j
  long long out_ts;
  int out_ld, B, R, j, reverse;
};

template <int NW>
__global__ __launch_bounds__(NW * 64) void gru_fwd_kernel(const float* hprev, const float* Whh, const float* bhh,
                                                          const float* xg, const int32_t* lens, unsigned b_r, unsigned j_rev,
                                                          float* hnext, float* out, float* rg, float* ug, float* ng, float* ghn,
                                                          long long out_ts, int out_ld) {
  // scalar arguments (GruFwdArgs documents them): the 5 input pointers, B:16|R:16 and j<<1|reverse are the first 12 dwords,
  // preloaded into SGPRs (stages.h, launch-latency note 4); the outputs come by s_load
  const int B = b_r & 0xffff, R0 = b_r >> 16, j = j_rev >> 1, reverse = j_rev & 1;
  __shared__ float red[3 * NW * 256];
  const int r0 = blockIdx.y * 16, c0 = blockIdx.x * 16, wave = threadIdx.x >> 6, R = R0;
  const int t = threadIdx.x & 255;
  const int row = r0 + (t >> 4), col = c0 + (t & 15);
  const bool own = threadIdx.x < 256 && row < B;
  const int rowc = row < B ? row : r0;
  const int idx = time_index(j, reverse, lens, rowc);
  const size_t o = (size_t)rowc * R + col;
  const size_t ox = ((size_t)idx * B + rowc) * 3 * R + col;
  const float x0 = xg[ox], x1 = xg[ox + R], x2 = xg[ox + 2 * R];
  const float b0 = bhh[col], b1 = bhh[R + col], b2 = bhh[2 * R + col];
  const float hp = hprev[o];
  f32x4 acc[3];
#pragma unroll
  for (int g = 0; g < 3; ++g) acc[g] = (f32x4){0.f, 0.f, 0.f, 0.f};
  {
    const float* const As[3] = {hprev, hprev, hprev};
    const float* const Ws[3] = {Whh, Whh, Whh};
    const int ld[3] = {R, R, R}, cs[3] = {c0, R + c0, 2 * R + c0};
    wave_gemm16_multi<NW, 3, true>(As, ld, r0, B, Ws, ld, cs, R, wave, acc);
  }
  float v[3];
  reduce_tiles<3, NW>(acc, red, v);
  if (!own) return;
  const float hn = v[2] + b2;
  const float r = sigmoidf_(x0 + v[0] + b0);
  const float u = sigmoidf_(x1 + v[1] + b1);
  const float n = tanhf(x2 + r * hn);
  const float h2 = (1.f - u) * n + u * hp;
  hnext[o] = h2;
  out[(size_t)idx * out_ts + (size_t)row * out_ld + col] = h2;
  rg[o] = r; ug[o] = u; ng[o] = n; ghn[o] = hn;
}

struct GruBwdArgs {
  const float* DGHn;    // [B,3R] hidden-projection grads of recurrence step j+1 (unused when has_gemm == 0)
  const float* WhhT;    // [R,3R] in T16
  const float* dout;    // time-indexed grad wrt the outputs (same addressing as GruFwdArgs::out)
  const float *rg, *ug, *ng, *ghn, *hprev;  // saves of step j; hprev = state entering step j
  const int32_t* lens;
  float* G;             // [B,R] running grad through the u-gate path (in/out)
  float* DGI;           // [T,B,3R] TIME indexed: grads wrt the input projection
  float* DGH;           // [B,3R] step j: grads wrt the hidden projection
  float* dh0;           // [B,R] out when has_gates == 0
  long long out_ts;
  int out_ld, B, R, j, reverse, has_gemm, has_gates;
};

template <int NW>
__global__ __launch_bounds__(NW * 64) void gru_bwd_kernel(const float* DGHn, const float* WhhT, float* G, unsigned b_r, unsigned has,
                                                          GruBwdArgs a) {
  // the leading scalars (operand pointers, G, sizes, flags) are preloaded into SGPRs; the struct comes by s_load and the saves of
  // the step are prefetched by wave_gemm16's `mid` hook, after the operand loads have been issued (stages.h head_stage_kernel)
  __shared__ float red[NW * 256];
  const int B = b_r & 0xffff, R = b_r >> 16;
  const int has_gemm = has & 1, has_gates = (has >> 1) & 1;
  const int r0 = blockIdx.y * 16, c0 = blockIdx.x * 16;
  const int t = threadIdx.x & 255;
  const int row = r0 + (t >> 4), col = c0 + (t & 15);
  const bool own = threadIdx.x < 256 && row < B;
  const int rowc = row < B ? row : r0;
  const size_t o = (size_t)rowc * R + col;
  float g = G[o];
  float dout = 0.f, r = 0.f, u = 0.f, n = 0.f, hn = 0.f, hp = 0.f;
  int idx = 0;
  auto prefetch = [&]() {
    if (has_gates) {  // wave-uniform
      idx = time_index(a.j, a.reverse, a.lens, rowc);
      dout = a.dout[(size_t)idx * a.out_ts + (size_t)rowc * a.out_ld + col];
      r = a.rg[o]; u = a.ug[o]; n = a.ng[o]; hn = a.ghn[o]; hp = a.hprev[o];
    }
  };
  float v[1] = {0.f};
  if (has_gemm) {
    f32x4 acc[1] = {{0.f, 0.f, 0.f, 0.f}};
    acc[0] = wave_gemm16<NW, true>(DGHn, 3 * R, r0, B, WhhT, 3 * R, c0, 3 * R, threadIdx.x >> 6, acc[0], prefetch);
    reduce_tiles<1, NW>(acc, red, v);
  } else {
    prefetch();
  }
  if (!own) return;
  g += dout;
  g += v[0];
  if (!has_gates) { a.dh0[o] = g; return; }
  const float dn_pre = g * (1.f - u) * (1.f - n * n);
  const float du_pre = g * (hp - n) * u * (1.f - u);
  const float dr_pre = dn_pre * hn * r * (1.f - r);
  const size_t oi = ((size_t)idx * B + row) * 3 * R + col, oh = (size_t)row * 3 * R + col;
  a.DGI[oi] = dr_pre; a.DGI[oi + R] = du_pre; a.DGI[oi + 2 * R] = dn_pre;
  a.DGH[oh] = dr_pre; a.DGH[oh + R] = du_pre; a.DGH[oh + 2 * R] = dn_pre * r;
  G[o] = g * u;
}

struct GruReserve { float *XG, *Hs, *RG, *UG, *NG, *GHN, *WhhP, *H16; };  // WhhP: T16 copy of Whh; H16: (T+1) T16 slabs of the state
size_t carve_gru(float* base, int T, int B, int R, GruReserve* r) {
  Arena ar{base};
  GruReserve t;
  const size_t n = (size_t)T * B;
  t.XG = ar.take(n * 3 * R);
  t.Hs = ar.take((size_t)(T + 1) * B * R);
  t.RG = ar.take(n * R); t.UG = ar.take(n * R); t.NG = ar.take(n * R); t.GHN = ar.take(n * R);
  t.WhhP = ar.take((size_t)3 * R * R);
  t.H16 = B <= kPchainCarveMaxB ? ar.take((size_t)(T + 1) * t16_rows(B) * R) : nullptr;
  if (r) *r = t;
  return ar.floats();
}
struct GruWs { float *WhhT, *DGI, *DGH, *G, *DGH16; };
size_t carve_gru_ws(float* base, int T, int B, int R, GruWs* w) {
  Arena ar{base};
  GruWs t;
  const size_t n = (size_t)T * B;
  t.WhhT = ar.take((size_t)R * 3 * R);
  t.DGI = ar.take(n * 3 * R);
  t.DGH = ar.take(n * 3 * R);
  t.G = ar.take((size_t)B * R);
  t.DGH16 = B <= kPchainCarveMaxB ? ar.take((size_t)(T + 1) * t16_rows(B) * 3 * R) : nullptr;
  if (w) *w = t;
  return ar.floats();
}

// which implementation each sequence entry point took (blvm_rnn_path_counts): host-side counts, one per call
enum { RNN_LSTM_FWD = 0, RNN_LSTM_BWD = 1, RNN_GRU_FWD = 2, RNN_GRU_BWD = 3 };
enum { PATH_REGS = 0, PATH_PROGRAM = 1, PATH_PER_STEP = 2 };
std::atomic<unsigned long long> g_path_counts[12];
inline void count_path(int op, int path) { g_path_counts[op * 3 + path].fetch_add(1, std::memory_order_relaxed); }

int check_rnn(int T, int B, int I, int H) {
  BLVM_REQUIRE(T > 0 && B > 0 && I > 0 && H > 0, "rnn: bad shape T=%d B=%d I=%d H=%d", T, B, I, H);
  BLVM_REQUIRE(H % 16 == 0, "rnn: hidden size must be a multiple of 16 (got %d)", H);
  BLVM_REQUIRE((B + 15) / 16 <= 65535, "rnn: batch too large");
  return BLVM_OK;
}

}  // namespace
}  // namespace blvm

using namespace blvm;

// --------------------------------------------------------------------------------------------------------------------
extern "C" int blvm_rnn_path_counts(unsigned long long out[12]) {
  BLVM_REQUIRE(out, "rnn_path_counts: null pointer");
  for (int k = 0; k < 12; ++k) out[k] = g_path_counts[k].load(std::memory_order_relaxed);
  return BLVM_OK;
}

extern "C" size_t blvm_lstm_reserve_floats(int T, int B, int H) { return carve_lstm(nullptr, T, B, H, nullptr); }
extern "C" size_t blvm_lstm_bwd_workspace_floats(int T, int B, int H) { return carve_lstm_ws(nullptr, T, B, H, nullptr); }

extern "C" int blvm_lstm_seq_fwd(const float* Wih, const float* Whh, const float* bih, const float* bhh, const float* in,
                                 const float* h0, const float* c0, const int32_t* lens, int T, int B, int I, int H,
                                 float* out, float* hn, float* cn, float* reserve, void* stream_) {
  hipStream_t s = static_cast<hipStream_t>(stream_);
  BLVM_TRY(check_rnn(T, B, I, H));
  BLVM_REQUIRE(Wih && Whh && bih && bhh && in && out && reserve, "lstm_fwd: null pointer");
  BLVM_REQUIRE(aligned16(reserve) && aligned16(Whh), "lstm_fwd: buffers must be 16-byte aligned");
  BLVM_REQUIRE(B < 65536 && H < 65536, "lstm_fwd: B and H must be below 65536 (packed kernel arguments)");
  LstmReserve rs;
  carve_lstm(reserve, T, B, H, &rs);
  const size_t n = (size_t)T * B, bh = (size_t)B * H;
  BLVM_TRY(gemm_f32(0, 0, (int)n, 4 * H, I, in, I, Wih, I, rs.XG, 4 * H, bih, 0, 0.f, nullptr, 0, 0, 1, s));
  BLVM_HIP(copy_or_zero(rs.Hs, h0, sizeof(float) * bh, s));
  BLVM_HIP(copy_or_zero(rs.Cs, c0, sizeof(float) * bh, s));
  const OpType seq_ot = seq_persistent(T, B) ? pchain_optype(B) : OP_F32;  // 16-bit operand mode of the persistent path
  T16PackScope pack_scope(seq_ot, s);
  BLVM_TRY(t16_pack_rows(Whh, H, 4 * H, H, rs.WhhP, s));  // operand layout of the chain (once per sequence)
  BLVM_TRY(pack_scope.flush());
  if (seq_persistent(T, B) && (seq_regs_mask() & 1) && seq_regs_applies(H, 4 * H, H, B, 4)) {
    count_path(RNN_LSTM_FWD, PATH_REGS);
    // one persistent launch with the workgroup's weight slice in registers (seqchain.hip)
    const long xH = (long)((B + 15) / 16) * 16 * H;
    SeqLstmFwd q{rs.H16, rs.WhhP, bhh, rs.XG, lens, rs.Hs, rs.Cs, out, rs.GATES, T, B, H, seq_ot, {}};
    BLVM_HIP(pchain_fill_sentinel(rs.H16 + xH, sizeof(float) * (size_t)T * xH, s));
    BLVM_TRY(pchain_rows_to_t16(rs.Hs, H, B, H, rs.H16, s));
    BLVM_TRY(seq_lstm_fwd(q, s));
  } else if (seq_persistent(T, B)) {
    count_path(RNN_LSTM_FWD, PATH_PROGRAM);
    // one persistent launch for the whole sequence (pchain.hip): one link per step — the hidden projection with the gate math
    using namespace pchain;
    const int rt = (B + 15) / 16, ctH = H / 16;
    const long sH = (long)bh, s4H = 4 * sH, xH = (long)rt * 16 * H;
    Builder bld;
    bld.begin(seq_ot, T, B, 4, false, 1);
    Desc& d = bld.add(K_LSTMS, ctH, 0, range_for(ctH * rt, device_cus() & ~7), H, 0, 0, T);
    bld.ptr(d, LSTMS_H16, {rs.H16, xH}); bld.ptr(d, LSTMS_WHH, rs.WhhP); bld.ptr(d, LSTMS_BHH, bhh); bld.ptr(d, LSTMS_XG, {rs.XG, s4H}); bld.ptr(d, LSTMS_LENS, lens);
    bld.ptr(d, LSTMS_HPREV, {rs.Hs, sH}); bld.ptr(d, LSTMS_HNEXT, {rs.Hs + sH, sH}); bld.ptr(d, LSTMS_HNEXT16, {rs.H16 + xH, xH}); bld.ptr(d, LSTMS_CPREV, {rs.Cs, sH});
    bld.ptr(d, LSTMS_CNEXT, {rs.Cs + sH, sH}); bld.ptr(d, LSTMS_OUT, {out, sH}); bld.ptr(d, LSTMS_GATES, {rs.GATES, s4H}); d.ld[LD_OUT] = H; d.n16[N16_OUT] = ctH;
    d.i[LSTMS_I_H] = H;
    BLVM_HIP(pchain_fill_sentinel(rs.H16 + xH, sizeof(float) * (size_t)T * xH, s));
    BLVM_TRY(pchain_rows_to_t16(rs.Hs, H, B, H, rs.H16, s));
    BLVM_TRY(pchain_launch(bld, "lstm_fwd", s));
  } else {
    count_path(RNN_LSTM_FWD, PATH_PER_STEP);
    const int nw = pick_nw(H, 4);
    const dim3 grid(H / 16, (B + 15) / 16);
    for (int t = 0; t < T; ++t) {
      const float *hp = rs.Hs + t * bh, *cp = rs.Cs + t * bh, *xg_t = rs.XG + (size_t)t * B * 4 * H;
      float *hnx = rs.Hs + (t + 1) * bh, *cnx = rs.Cs + (t + 1) * bh, *out_t = out + t * bh, *gates_t = rs.GATES + (size_t)t * B * 4 * H;
      const unsigned b_h = (unsigned)B | ((unsigned)H << 16);
      LAUNCH_NW(lstm_fwd_kernel<NW_>, nw, grid, s, hp, cp, (const float*)rs.WhhP, bhh, xg_t, lens, b_h, t, hnx, cnx, out_t, gates_t);
    }
  }
  BLVM_CHECK_LAUNCH("lstm_seq_fwd");
  if (hn) BLVM_HIP(hipMemcpyAsync(hn, rs.Hs + T * bh, sizeof(float) * bh, hipMemcpyDeviceToDevice, s));
  if (cn) BLVM_HIP(hipMemcpyAsync(cn, rs.Cs + T * bh, sizeof(float) * bh, hipMemcpyDeviceToDevice, s));
  return BLVM_OK;
}

extern "C" int blvm_lstm_seq_bwd(const float* Wih, const float* Whh, const float* in, const float* reserve,
                                 const float* d_out, int T, int B, int I, int H, float* d_in, float* d_h0, float* d_c0,
                                 float* dWih, float* dWhh, float* dbih, float* dbhh, float* workspace, void* stream_) {
  hipStream_t s = static_cast<hipStream_t>(stream_);
  BLVM_TRY(check_rnn(T, B, I, H));
  BLVM_REQUIRE(Wih && Whh && in && reserve && d_out && workspace, "lstm_bwd: null pointer");
  BLVM_REQUIRE(aligned16(reserve) && aligned16(workspace), "lstm_bwd: buffers must be 16-byte aligned");
  BLVM_REQUIRE(B < 65536 && H < 65536, "lstm_bwd: B and H must be below 65536 (packed kernel arguments)");
  LstmReserve rs;
  carve_lstm(const_cast<float*>(reserve), T, B, H, &rs);
  LstmWs ws;
  carve_lstm_ws(workspace, T, B, H, &ws);
  const size_t n = (size_t)T * B, bh = (size_t)B * H;
  const OpType seq_ot = seq_persistent(T, B) ? pchain_optype(B) : OP_F32;  // 16-bit operand mode of the persistent path
  T16PackScope pack_scope(seq_ot, s);
  BLVM_TRY(t16_pack_transposed(Whh, H, 4 * H, H, ws.WhhT, s));
  BLVM_TRY(pack_scope.flush());
  BLVM_HIP(hipMemsetAsync(ws.DC, 0, sizeof(float) * bh, s));
  if (seq_persistent(T, B) && (seq_regs_mask() & 2) && 4 * H <= kSeqRegsMaxKBwd && seq_regs_applies(H, 4 * H, H, B, 4)) {
    count_path(RNN_LSTM_BWD, PATH_REGS);
    const long x4H = (long)((B + 15) / 16) * 16 * 4 * H;
    SeqLstmBwd q{ws.DG16, ws.WhhT, d_out, rs.GATES, rs.Cs, ws.DC, ws.DG, d_h0 ? d_h0 : ws.DC, T, B, H, d_h0 ? T + 1 : T, seq_ot, {}};
    BLVM_HIP(pchain_fill_sentinel(ws.DG16, sizeof(float) * (size_t)T * x4H, s));
    BLVM_TRY(seq_lstm_bwd(q, s));
  } else if (seq_persistent(T, B)) {
    count_path(RNN_LSTM_BWD, PATH_PROGRAM);
    using namespace pchain;
    const int rt = (B + 15) / 16, ctH = H / 16;
    const long sH = (long)bh, s4H = 4 * sH, x4H = (long)rt * 16 * 4 * H;
    Builder bld;
    bld.begin(seq_ot, d_h0 ? T + 1 : T, B, 1, true, 1);
    Desc& d = bld.add(K_LSTMSB, ctH, 0, range_for(ctH * rt, device_cus() & ~7), 4 * H, 0, 0, T + 1);
    // step s handles t = T-1-s: time-indexed slabs start at the last step and walk backwards; the T16 slabs are indexed by s
    bld.ptr(d, LSTMSB_DG16_IN, {ws.DG16 - x4H, x4H}); bld.ptr(d, LSTMSB_WHHT, ws.WhhT); bld.ptr(d, LSTMSB_DOUT, rev(d_out, sH, T - 1));
    bld.ptr(d, LSTMSB_GATES, rev(rs.GATES, s4H, T - 1)); bld.ptr(d, LSTMSB_CS, rev(rs.Cs, sH, T - 1)); bld.ptr(d, LSTMSB_DC, ws.DC);
    bld.ptr(d, LSTMSB_DG, rev(ws.DG, s4H, T - 1)); bld.ptr(d, LSTMSB_DG16, {ws.DG16, x4H}); bld.ptr(d, LSTMSB_DH0, d_h0 ? d_h0 : ws.DC); d.ld[LD_OUT] = 4 * H;
    d.n16[N16_OUT] = 4 * ctH; d.n16[LSTMSB_N16_T] = T; d.i[LSTMSB_I_H] = H;
    BLVM_HIP(pchain_fill_sentinel(ws.DG16, sizeof(float) * (size_t)T * x4H, s));
    BLVM_TRY(pchain_launch(bld, "lstm_bwd", s));
  } else {
    count_path(RNN_LSTM_BWD, PATH_PER_STEP);
    const int nw = pick_nw(4 * H, 1);
    const dim3 grid(H / 16, (B + 15) / 16);
    for (int st = T - 1; st >= -1; --st) {
      const unsigned has = (st < T - 1 ? 1u : 0u) | (st >= 0 ? 2u : 0u);
      const int sg = st >= 0 ? st : 0;
      const float* DGn = ws.DG + (size_t)(st + 1 < T ? st + 1 : 0) * B * 4 * H;
      const float *dout_s = d_out + sg * bh, *gates_s = rs.GATES + (size_t)sg * B * 4 * H, *c_s = rs.Cs + sg * bh;
      float* DG_s = ws.DG + (size_t)sg * B * 4 * H;
      const unsigned b_h = (unsigned)B | ((unsigned)H << 16);
      if (st == -1 && d_h0 == nullptr) break;
      LAUNCH_NW(lstm_bwd_kernel<NW_>, nw, grid, s, DGn, (const float*)ws.WhhT, dout_s, gates_s, c_s, ws.DC, b_h, has, DG_s, d_h0);
    }
  }
  BLVM_CHECK_LAUNCH("lstm_seq_bwd");
  if (d_c0) BLVM_HIP(hipMemcpyAsync(d_c0, ws.DC, sizeof(float) * bh, hipMemcpyDeviceToDevice, s));
  if (d_in) {
    BLVM_TRY(gemm_f32(0, 1, (int)n, I, 4 * H, ws.DG, 4 * H, Wih, I, d_in, I, nullptr, 0, 0.f, nullptr, 0, 0, 1, s));
  }
  // weight + bias gradients: the bias sums ride on the weight-gradient GEMMs (gemm.hip: column sums of the staged D tiles)
  if (dWih) BLVM_TRY(gemm_f32(1, 1, 4 * H, I, (int)n, ws.DG, 4 * H, in, I, dWih, I, nullptr, 0, 0.f, nullptr, 0, 1, pick_split(4 * H, I, (int)n), s, dbih));
  else if (dbih) BLVM_TRY(colsum_f32((int)n, 4 * H, ws.DG, 4 * H, dbih, 1, s));
  if (dWhh) BLVM_TRY(gemm_f32(1, 1, 4 * H, H, (int)n, ws.DG, 4 * H, rs.Hs, H, dWhh, H, nullptr, 0, 0.f, nullptr, 0, 1, pick_split(4 * H, H, (int)n), s, dbhh));
  else if (dbhh) BLVM_TRY(colsum_f32((int)n, 4 * H, ws.DG, 4 * H, dbhh, 1, s));
  return BLVM_OK;
}

// --------------------------------------------------------------------------------------------------------------------
// Bidirectional LSTM layer, both directions in one launch (seqchain.hip lstm_bidir_*_kernel).  Each direction owns one LstmReserve /
// LstmWs carve plus its leaving cell states; of the carve, Hs and Cs hold the states ENTERING the step of each time index (their first
// T slabs), and DC is unused (the running cell gradient starts at zero in a register).
namespace blvm {
namespace {
struct LstmBidirReserve { LstmReserve d[2]; float* Cout[2]; };
size_t carve_lstm_bidir(float* base, int T, int B, int H, LstmBidirReserve* r) {
  Arena ar{base};
  LstmBidirReserve t;
  for (int k = 0; k < 2; ++k) {
    float* at = ar.take(carve_lstm(nullptr, T, B, H, nullptr));
    carve_lstm(at, T, B, H, &t.d[k]);
    t.Cout[k] = ar.take((size_t)T * B * H);
  }
  if (r) *r = t;
  return ar.floats();
}
size_t carve_lstm_bidir_ws(float* base, int T, int B, int H, LstmWs (*w)[2]) {
  Arena ar{base};
  for (int k = 0; k < 2; ++k) {
    float* at = ar.take(carve_lstm_ws(nullptr, T, B, H, nullptr));
    if (w) carve_lstm_ws(at, T, B, H, &(*w)[k]);
  }
  return ar.floats();
}
// The one-launch form: the register-resident forward AND backward kernels take the shape (H in {128, 256, 384}), and BOTH directions'
// tiles are resident at once — a workgroup that was never scheduled would leave the polling ones spinning.
inline bool lstm_bidir_applies(int T, int B, int H) {
  return seq_persistent(T, B) && (seq_regs_mask() & 3) == 3 && 4 * H <= kSeqRegsMaxKBwd && seq_regs_applies(H, 4 * H, H, B, 4) &&
         2 * (H / 16) * ((B + 15) / 16) <= device_cus();
}
std::atomic<unsigned long long> g_bidir_counts[2];
}  // namespace
}  // namespace blvm

extern "C" size_t blvm_lstm_bidir_reserve_floats(int T, int B, int H) { return carve_lstm_bidir(nullptr, T, B, H, nullptr); }
extern "C" size_t blvm_lstm_bidir_bwd_workspace_floats(int T, int B, int H) { return carve_lstm_bidir_ws(nullptr, T, B, H, nullptr); }

extern "C" int blvm_lstm_bidir_applies(int T, int B, int H) { return T > 0 && B > 0 && H > 0 && lstm_bidir_applies(T, B, H) ? 1 : 0; }

extern "C" int blvm_lstm_bidir_path_counts(unsigned long long out[2]) {
  BLVM_REQUIRE(out, "lstm_bidir_path_counts: null pointer");
  for (int k = 0; k < 2; ++k) out[k] = g_bidir_counts[k].load(std::memory_order_relaxed);
  return BLVM_OK;
}

extern "C" int blvm_lstm_bidir_fwd(const float* Wih_f, const float* Whh_f, const float* bih_f, const float* bhh_f, const float* Wih_r,
                                   const float* Whh_r, const float* bih_r, const float* bhh_r, const float* in, const int32_t* lens,
                                   int T, int B, int I, int H, float* out, float* reserve, void* stream_) {
  hipStream_t s = static_cast<hipStream_t>(stream_);
  BLVM_TRY(check_rnn(T, B, I, H));
  BLVM_REQUIRE(Wih_f && Whh_f && bih_f && bhh_f && Wih_r && Whh_r && bih_r && bhh_r && in && lens && out && reserve, "lstm_bidir_fwd: null pointer");
  BLVM_REQUIRE(aligned16(reserve) && aligned16(Whh_f) && aligned16(Whh_r), "lstm_bidir_fwd: buffers must be 16-byte aligned");
  if (!lstm_bidir_applies(T, B, H)) return BLVM_NOT_APPLICABLE;
  LstmBidirReserve rs;
  carve_lstm_bidir(reserve, T, B, H, &rs);
  const float *Wih[2] = {Wih_f, Wih_r}, *Whh[2] = {Whh_f, Whh_r}, *bih[2] = {bih_f, bih_r}, *bhh[2] = {bhh_f, bhh_r};
  const size_t n = (size_t)T * B;
  const long xH = (long)t16_rows(B) * H;
  for (int k = 0; k < 2; ++k) BLVM_TRY(gemm_f32(0, 0, (int)n, 4 * H, I, in, I, Wih[k], I, rs.d[k].XG, 4 * H, bih[k], 0, 0.f, nullptr, 0, 0, 1, s));
  const OpType seq_ot = pchain_optype(B);
  T16PackScope pack_scope(seq_ot, s);
  for (int k = 0; k < 2; ++k) BLVM_TRY(t16_pack_rows(Whh[k], H, 4 * H, H, rs.d[k].WhhP, s));
  BLVM_TRY(pack_scope.flush());
  SeqLstmBidirFwd q{};
  for (int k = 0; k < 2; ++k) {
    q.d[k] = SeqLstmBidirFwdDir{rs.d[k].H16, rs.d[k].WhhP, bhh[k], rs.d[k].XG, rs.d[k].Hs, rs.d[k].Cs, rs.Cout[k], rs.d[k].GATES};
    BLVM_HIP(pchain_fill_sentinel(rs.d[k].H16 + xH, sizeof(float) * (size_t)T * xH, s));
    BLVM_TRY(pchain_rows_to_t16(nullptr, H, B, H, rs.d[k].H16, s));  // zero initial state
  }
  q.lens = lens; q.out = out; q.T = T; q.B = B; q.H = H; q.ot = seq_ot;
  BLVM_TRY(seq_lstm_bidir_fwd(q, s));
  g_bidir_counts[0].fetch_add(1, std::memory_order_relaxed);
  return BLVM_OK;
}

extern "C" int blvm_lstm_bidir_bwd(const float* Wih_f, const float* Whh_f, const float* Wih_r, const float* Whh_r, const float* in,
                                   const int32_t* lens, const float* reserve, const float* d_out, int T, int B, int I, int H,
                                   float* d_in, float* dWih_f, float* dWhh_f, float* dbih_f, float* dbhh_f, float* dWih_r,
                                   float* dWhh_r, float* dbih_r, float* dbhh_r, float* workspace, void* stream_) {
  hipStream_t s = static_cast<hipStream_t>(stream_);
  BLVM_TRY(check_rnn(T, B, I, H));
  BLVM_REQUIRE(Wih_f && Whh_f && Wih_r && Whh_r && in && lens && reserve && d_out && workspace, "lstm_bidir_bwd: null pointer");
  BLVM_REQUIRE(aligned16(reserve) && aligned16(workspace), "lstm_bidir_bwd: buffers must be 16-byte aligned");
  if (!lstm_bidir_applies(T, B, H)) return BLVM_NOT_APPLICABLE;
  LstmBidirReserve rs;
  carve_lstm_bidir(const_cast<float*>(reserve), T, B, H, &rs);
  LstmWs ws[2];
  carve_lstm_bidir_ws(workspace, T, B, H, &ws);
  const float *Wih[2] = {Wih_f, Wih_r}, *Whh[2] = {Whh_f, Whh_r};
  float *dWih[2] = {dWih_f, dWih_r}, *dWhh[2] = {dWhh_f, dWhh_r}, *dbih[2] = {dbih_f, dbih_r}, *dbhh[2] = {dbhh_f, dbhh_r};
  const size_t n = (size_t)T * B;
  const long x4H = (long)t16_rows(B) * 4 * H;
  const OpType seq_ot = pchain_optype(B);
  T16PackScope pack_scope(seq_ot, s);
  for (int k = 0; k < 2; ++k) BLVM_TRY(t16_pack_transposed(Whh[k], H, 4 * H, H, ws[k].WhhT, s));
  BLVM_TRY(pack_scope.flush());
  SeqLstmBidirBwd q{};
  for (int k = 0; k < 2; ++k) {
    q.d[k] = SeqLstmBidirBwdDir{ws[k].DG16, ws[k].WhhT, rs.d[k].GATES, rs.d[k].Cs, rs.Cout[k], ws[k].DG};
    BLVM_HIP(pchain_fill_sentinel(ws[k].DG16, sizeof(float) * (size_t)T * x4H, s));
  }
  q.lens = lens; q.dout = d_out; q.T = T; q.B = B; q.H = H; q.ot = seq_ot;
  BLVM_TRY(seq_lstm_bidir_bwd(q, s));
  g_bidir_counts[1].fetch_add(1, std::memory_order_relaxed);
  // DG, Hs (the entering states) and `in` are all TIME indexed: the unidirectional driver's GEMMs, once per direction
  for (int k = 0; k < 2; ++k) {
    if (d_in) BLVM_TRY(gemm_f32(0, 1, (int)n, I, 4 * H, ws[k].DG, 4 * H, Wih[k], I, d_in, I, nullptr, 0, 0.f, nullptr, 0, k, 1, s));
    if (dWih[k]) BLVM_TRY(gemm_f32(1, 1, 4 * H, I, (int)n, ws[k].DG, 4 * H, in, I, dWih[k], I, nullptr, 0, 0.f, nullptr, 0, 1, pick_split(4 * H, I, (int)n), s, dbih[k]));
    else if (dbih[k]) BLVM_TRY(colsum_f32((int)n, 4 * H, ws[k].DG, 4 * H, dbih[k], 1, s));
    if (dWhh[k]) BLVM_TRY(gemm_f32(1, 1, 4 * H, H, (int)n, ws[k].DG, 4 * H, rs.d[k].Hs, H, dWhh[k], H, nullptr, 0, 0.f, nullptr, 0, 1, pick_split(4 * H, H, (int)n), s, dbhh[k]));
    else if (dbhh[k]) BLVM_TRY(colsum_f32((int)n, 4 * H, ws[k].DG, 4 * H, dbhh[k], 1, s));
  }
  return BLVM_OK;
}

// --------------------------------------------------------------------------------------------------------------------
extern "C" size_t blvm_gru_reserve_floats(int T, int B, int R) { return carve_gru(nullptr, T, B, R, nullptr); }
extern "C" size_t blvm_gru_bwd_workspace_floats(int T, int B, int R) { return carve_gru_ws(nullptr, T, B, R, nullptr); }

extern "C" int blvm_gru_seq_fwd(const float* Wih, const float* Whh, const float* bih, const float* bhh, const float* in,
                                int ld_in, const float* h0, const int32_t* lens, int reverse, int T, int B, int I, int R,
                                float* out, long long out_ts, int out_ld, float* hn, float* reserve, void* stream_) {
  hipStream_t s = static_cast<hipStream_t>(stream_);
  BLVM_TRY(check_rnn(T, B, I, R));
  BLVM_REQUIRE(Wih && Whh && bih && bhh && in && out && reserve, "gru_fwd: null pointer");
  BLVM_REQUIRE(!reverse || lens, "gru_fwd: reverse needs lens");
  BLVM_REQUIRE(aligned16(reserve) && aligned16(Whh), "gru_fwd: buffers must be 16-byte aligned");
  BLVM_REQUIRE(B < 65536 && R < 65536, "gru_fwd: B and R must be below 65536 (packed kernel arguments)");
  GruReserve rs;
  carve_gru(reserve, T, B, R, &rs);
  const size_t n = (size_t)T * B, br = (size_t)B * R;
  BLVM_TRY(gemm_f32(0, 0, (int)n, 3 * R, I, in, ld_in, Wih, I, rs.XG, 3 * R, bih, 0, 0.f, nullptr, 0, 0, 1, s));
  BLVM_HIP(copy_or_zero(rs.Hs, h0, sizeof(float) * br, s));
  const OpType seq_ot = seq_persistent(T, B) ? pchain_optype(B) : OP_F32;  // 16-bit operand mode of the persistent path
  T16PackScope pack_scope(seq_ot, s);
  BLVM_TRY(t16_pack_rows(Whh, R, 3 * R, R, rs.WhhP, s));  // operand layout of the chain (once per sequence)
  BLVM_TRY(pack_scope.flush());
  if (seq_persistent(T, B) && (seq_regs_mask() & 1) && seq_regs_applies(R, 3 * R, R, B, 3)) {
    count_path(RNN_GRU_FWD, PATH_REGS);
    const long xR = (long)((B + 15) / 16) * 16 * R;
    SeqGruFwd q{rs.H16, rs.WhhP, bhh, rs.XG, lens, rs.Hs, out, rs.RG, rs.UG, rs.NG, rs.GHN, (long)out_ts, out_ld, T, B, R, reverse ? 1 : 0, seq_ot, {}};
    BLVM_HIP(pchain_fill_sentinel(rs.H16 + xR, sizeof(float) * (size_t)T * xR, s));
    BLVM_TRY(pchain_rows_to_t16(rs.Hs, R, B, R, rs.H16, s));
    BLVM_TRY(seq_gru_fwd(q, s));
  } else if (seq_persistent(T, B)) {
    count_path(RNN_GRU_FWD, PATH_PROGRAM);
    using namespace pchain;
    BLVM_REQUIRE(out_ts >= 0 && out_ts < (1ll << 31), "gru_fwd: output step stride out of range");
    const int rt = (B + 15) / 16, ctR = R / 16;
    const long sR = (long)br, xR = (long)rt * 16 * R;
    Builder bld;
    bld.begin(seq_ot, T, B, 3, false, 1);
    Desc& d = bld.add(K_GRUS, ctR, 0, range_for(ctR * rt, device_cus() & ~7), R, 0, 0, T);
    bld.ptr(d, GRUS_H16, {rs.H16, xR}); bld.ptr(d, GRUS_WHH, rs.WhhP); bld.ptr(d, GRUS_BHH, bhh); bld.ptr(d, GRUS_XG, rs.XG); bld.ptr(d, GRUS_LENS, lens);
    bld.ptr(d, GRUS_HPREV, {rs.Hs, sR}); bld.ptr(d, GRUS_HNEXT, {rs.Hs + sR, sR}); bld.ptr(d, GRUS_HNEXT16, {rs.H16 + xR, xR}); bld.ptr(d, GRUS_OUT, out);
    bld.ptr(d, GRUS_RG, {rs.RG, sR}); bld.ptr(d, GRUS_UG, {rs.UG, sR}); bld.ptr(d, GRUS_NG, {rs.NG, sR}); bld.ptr(d, GRUS_GHN, {rs.GHN, sR}); d.ld[LD_OUT] = R;
    d.n16[N16_OUT] = ctR; d.i[GRUS_I_R] = R; d.i[GRUS_I_REVERSE] = reverse ? 1 : 0; d.i[GRUS_I_OUT_TS] = (int)out_ts; d.i[GRUS_I_OUT_LD] = out_ld;
    BLVM_HIP(pchain_fill_sentinel(rs.H16 + xR, sizeof(float) * (size_t)T * xR, s));
    BLVM_TRY(pchain_rows_to_t16(rs.Hs, R, B, R, rs.H16, s));
    BLVM_TRY(pchain_launch(bld, "gru_fwd", s));
  } else {
    count_path(RNN_GRU_FWD, PATH_PER_STEP);
    const int nw = pick_nw(R, 3);
    const dim3 grid(R / 16, (B + 15) / 16);
    for (int j = 0; j < T; ++j) {
      const float* hp = rs.Hs + j * br;
      float *hnx = rs.Hs + (j + 1) * br, *rg_j = rs.RG + j * br, *ug_j = rs.UG + j * br, *ng_j = rs.NG + j * br, *ghn_j = rs.GHN + j * br;
      const unsigned b_r = (unsigned)B | ((unsigned)R << 16), j_rev = ((unsigned)j << 1) | (reverse ? 1u : 0u);
      LAUNCH_NW(gru_fwd_kernel<NW_>, nw, grid, s, hp, (const float*)rs.WhhP, bhh, (const float*)rs.XG, lens, b_r, j_rev, hnx, out, rg_j, ug_j, ng_j, ghn_j, out_ts, out_ld);
    }
  }
  BLVM_CHECK_LAUNCH("gru_seq_fwd");
  if (hn) BLVM_HIP(hipMemcpyAsync(hn, rs.Hs + T * br, sizeof(float) * br, hipMemcpyDeviceToDevice, s));
  return BLVM_OK;
}

extern "C" int blvm_gru_seq_bwd(const float* Wih, const float* Whh, const float* in, int ld_in, const int32_t* lens,
                                int reverse, const float* reserve, const float* d_out, long long out_ts, int out_ld,
                                int T, int B, int I, int R, float* d_in, int ld_din, int accumulate_din, float* d_h0,
                                float* dWih, float* dWhh, float* dbih, float* dbhh, float* workspace, void* stream_) {
  hipStream_t s = static_cast<hipStream_t>(stream_);
  BLVM_TRY(check_rnn(T, B, I, R));
  BLVM_REQUIRE(Wih && Whh && in && reserve && d_out && workspace, "gru_bwd: null pointer");
  BLVM_REQUIRE(!reverse || lens, "gru_bwd: reverse needs lens");
  BLVM_REQUIRE(B < 65536 && R < 65536, "gru_bwd: B and R must be below 65536 (packed kernel arguments)");
  BLVM_REQUIRE(aligned16(reserve) && aligned16(workspace), "gru_bwd: buffers must be 16-byte aligned");
  GruReserve rs;
  carve_gru(const_cast<float*>(reserve), T, B, R, &rs);
  GruWs ws;
  carve_gru_ws(workspace, T, B, R, &ws);
  const size_t n = (size_t)T * B, br = (size_t)B * R;
  const OpType seq_ot = seq_persistent(T, B) ? pchain_optype(B) : OP_F32;  // 16-bit operand mode of the persistent path
  T16PackScope pack_scope(seq_ot, s);
  BLVM_TRY(t16_pack_transposed(Whh, R, 3 * R, R, ws.WhhT, s));
  BLVM_TRY(pack_scope.flush());
  BLVM_HIP(hipMemsetAsync(ws.G, 0, sizeof(float) * br, s));
  if (seq_persistent(T, B) && (seq_regs_mask() & 2) && 3 * R <= kSeqRegsMaxKBwd && seq_regs_applies(R, 3 * R, R, B, 3)) {
    count_path(RNN_GRU_BWD, PATH_REGS);
    const long x3R = (long)((B + 15) / 16) * 16 * 3 * R;
    SeqGruBwd q{ws.DGH16, ws.WhhT, d_out, rs.RG, rs.UG, rs.NG, rs.GHN, rs.Hs, lens, ws.G, ws.DGI, ws.DGH, d_h0 ? d_h0 : ws.G, (long)out_ts, out_ld, T, B, R,
                reverse ? 1 : 0, d_h0 ? T + 1 : T, seq_ot, {}};
    BLVM_HIP(pchain_fill_sentinel(ws.DGH16, sizeof(float) * (size_t)T * x3R, s));
    BLVM_TRY(seq_gru_bwd(q, s));
  } else if (seq_persistent(T, B)) {
    count_path(RNN_GRU_BWD, PATH_PROGRAM);
    using namespace pchain;
    BLVM_REQUIRE(out_ts >= 0 && out_ts < (1ll << 31), "gru_bwd: output step stride out of range");
    const int rt = (B + 15) / 16, ctR = R / 16;
    const long sR = (long)br, s3R = 3 * sR, x3R = (long)rt * 16 * 3 * R;
    Builder bld;
    bld.begin(seq_ot, d_h0 ? T + 1 : T, B, 1, true, 1);
    Desc& d = bld.add(K_GRUSB, ctR, 0, range_for(ctR * rt, device_cus() & ~7), 3 * R, 0, 0, T + 1);
    // step s handles recurrence step j = T-1-s: the saves walk backwards from their last slab; the T16 slabs are indexed by s
    bld.ptr(d, GRUSB_DGH16_IN, {ws.DGH16 - x3R, x3R}); bld.ptr(d, GRUSB_WHHT, ws.WhhT); bld.ptr(d, GRUSB_DOUT, d_out); bld.ptr(d, GRUSB_RG, rev(rs.RG, sR, T - 1));
    bld.ptr(d, GRUSB_UG, rev(rs.UG, sR, T - 1)); bld.ptr(d, GRUSB_NG, rev(rs.NG, sR, T - 1)); bld.ptr(d, GRUSB_GHN, rev(rs.GHN, sR, T - 1));
    bld.ptr(d, GRUSB_HPREV, rev(rs.Hs, sR, T - 1)); bld.ptr(d, GRUSB_LENS, lens); bld.ptr(d, GRUSB_G, ws.G); bld.ptr(d, GRUSB_DGI, ws.DGI);
    bld.ptr(d, GRUSB_DGH, rev(ws.DGH, s3R, T - 1)); bld.ptr(d, GRUSB_DGH16, {ws.DGH16, x3R}); bld.ptr(d, GRUSB_DH0, d_h0 ? d_h0 : ws.G); d.ld[LD_OUT] = 3 * R;
    d.n16[N16_OUT] = 3 * ctR; d.n16[GRUSB_N16_T] = T; d.i[GRUSB_I_R] = R; d.i[GRUSB_I_REVERSE] = reverse ? 1 : 0; d.i[GRUSB_I_OUT_TS] = (int)out_ts;
    d.i[GRUSB_I_OUT_LD] = out_ld;
    BLVM_HIP(pchain_fill_sentinel(ws.DGH16, sizeof(float) * (size_t)T * x3R, s));
    BLVM_TRY(pchain_launch(bld, "gru_bwd", s));
  } else {
    count_path(RNN_GRU_BWD, PATH_PER_STEP);
    const int nw = pick_nw(3 * R, 1);
    const dim3 grid(R / 16, (B + 15) / 16);
    for (int j = T - 1; j >= -1; --j) {
      if (j == -1 && d_h0 == nullptr) break;
      GruBwdArgs a;
      a.has_gemm = j < T - 1; a.has_gates = j >= 0;
      a.DGHn = ws.DGH + (size_t)(j + 1 < T ? j + 1 : 0) * B * 3 * R;
      a.WhhT = ws.WhhT; a.dout = d_out;
      const int jg = j >= 0 ? j : 0;
      a.rg = rs.RG + jg * br; a.ug = rs.UG + jg * br; a.ng = rs.NG + jg * br; a.ghn = rs.GHN + jg * br;
      a.hprev = rs.Hs + jg * br; a.lens = lens;
      a.G = ws.G; a.DGI = ws.DGI; a.DGH = ws.DGH + (size_t)jg * B * 3 * R; a.dh0 = d_h0;
      a.out_ts = out_ts; a.out_ld = out_ld; a.B = B; a.R = R; a.j = jg; a.reverse = reverse;
      const unsigned b_r = (unsigned)B | ((unsigned)R << 16), has = (a.has_gemm ? 1u : 0u) | (a.has_gates ? 2u : 0u);
      LAUNCH_NW(gru_bwd_kernel<NW_>, nw, grid, s, a.DGHn, a.WhhT, a.G, b_r, has, a);
    }
  }
  BLVM_CHECK_LAUNCH("gru_seq_bwd");
  if (d_in) {
    BLVM_TRY(gemm_f32(0, 1, (int)n, I, 3 * R, ws.DGI, 3 * R, Wih, I, d_in, ld_din, nullptr, 0, 0.f, nullptr, 0, accumulate_din, 1, s));
  }
  if (dWih) BLVM_TRY(gemm_f32(1, 1, 3 * R, I, (int)n, ws.DGI, 3 * R, in, ld_in, dWih, I, nullptr, 0, 0.f, nullptr, 0, 1, pick_split(3 * R, I, (int)n), s, dbih));
  else if (dbih) BLVM_TRY(colsum_f32((int)n, 3 * R, ws.DGI, 3 * R, dbih, 1, s));
  if (dWhh) BLVM_TRY(gemm_f32(1, 1, 3 * R, R, (int)n, ws.DGH, 3 * R, rs.Hs, R, dWhh, R, nullptr, 0, 0.f, nullptr, 0, 1, pick_split(3 * R, R, (int)n), s, dbhh));
  else if (dbhh) BLVM_TRY(colsum_f32((int)n, 3 * R, ws.DGH, 3 * R, dbhh, 1, s));
  return BLVM_OK;
}
