// vrnn.hip — K1: the VRNN recurrent cell over a whole sequence, forward and BPTT, as hand-written gfx950 kernels.
//
// Replaces the scripted per-step loop of the reference (blvm/models/vrnn.py:305-308 calling VRNNCell.forward,
// vrnn.py:109-141: prior MLP + DiagonalGaussianDense, posterior MLP + DiagonalGaussianDense on cat[h,x], residual
// posterior, rsample, phi_z MLP, nn.GRUCell on cat[x,phi_z]) and the autograd backward of that loop.
//
// Structure (v1, "stage kernels"): every recurrent step is a chain of nine dependent small GEMMs with M = batch.
// Each link is ONE launch whose workgroups own a 16(batch) x 16(feature) output tile; the four waves of a
// workgroup split K and combine through LDS, so one launch spreads over (B/16) x (N/16) workgroups and a wave
// issues only K/64 v_mfma_f32_16x16x4_f32.  All element-wise work (bias, ReLU, softplus head, residual mean,
// reparameterisation, GRU gates, and in the backward pass the KL/free-nats gradient, activation derivatives and the
// GRU gate derivatives) is fused into the epilogue of the producing GEMM.  Everything that does not depend on the
// recurrent state is hoisted out of the loop into large MFMA GEMMs (gemm.hip): the x-halves of the posterior's
// first layer and of the GRU input projection before the loop; all weight gradients and d(enc) after it.
//
// Numerics: fp32 operands, fp32 MFMA accumulation (an exact fma chain), so a sequence is reproducible run-to-run.
#include <vector>
#include <stdlib.h>

#include <algorithm>
#include <atomic>

#include "common.h"
#include "pchain.h"
#include "vrnn_static.h"

namespace blvm {
namespace {

#include "stages.h"

// ---------------------------------------------------------------------------------------------------------------
// F9: GRU input projection of phi + gates + state update
// ---------------------------------------------------------------------------------------------------------------
// arguments: decin_t [B,H+R] row block t of decin = [phi | h_prev]; Wih [3R,H] the phi columns of the GRU input weight, in T16;
// xg [B,3R] x-part of the input projection incl. b_ih; gh [B,3R] hidden projection incl. b_hh; decin_next = row block t+1 (h-part
// written); rg, ug, ng [B,R] saved gates

template <int NW>
__global__ __launch_bounds__(NW * 64) void gru_stage_kernel(const float* decin_t, const float* Wih, const float* xg,
                                                            const float* gh, int B, int H, int R, float* decin_next,
                                                            float* rg, float* ug, float* ng) {
  // scalar arguments: the operand pointers and sizes are the first 11 dwords, preloaded into SGPRs (stages.h, launch-latency note 4)
  __shared__ float red[3 * NW * 256];
  const int r0 = blockIdx.y * 16, c0 = blockIdx.x * 16, wave = threadIdx.x >> 6;
  const int ldd = H + R;
  const int t = threadIdx.x & 255;
  const int row = r0 + (t >> 4), col = c0 + (t & 15);
  const bool own = threadIdx.x < 256 && row < B;
  const int rowc = row < B ? row : r0;  // clamped: unconditional prefetch
  const size_t o3 = (size_t)rowc * 3 * R + col;
  const float x0 = xg[o3], x1 = xg[o3 + R], x2 = xg[o3 + 2 * R];
  const float hr = gh[o3], hz = gh[o3 + R], hn = gh[o3 + 2 * R];
  const float hp = decin_t[(size_t)rowc * ldd + H + col];
  f32x4 acc[3];
#pragma unroll
  for (int g = 0; g < 3; ++g) acc[g] = (f32x4){0.f, 0.f, 0.f, 0.f};
  {
    const float* const As[3] = {decin_t, decin_t, decin_t};
    const float* const Ws[3] = {Wih, Wih, Wih};
    const int la[3] = {ldd, ldd, ldd}, lw[3] = {H, H, H}, cs[3] = {c0, R + c0, 2 * R + c0};
    wave_gemm16_multi<NW, 3, true>(As, la, r0, B, Ws, lw, cs, H, wave, acc);
  }
  float v[3];
  reduce_tiles<3, NW>(acc, red, v);
  if (!own) return;
  const float r = sigmoidf_(v[0] + x0 + hr);
  const float u = sigmoidf_(v[1] + x1 + hz);
  const float n = tanhf(v[2] + x2 + r * hn);
  decin_next[(size_t)row * ldd + H + col] = (1.f - u) * n + u * hp;
  const size_t o = (size_t)row * R + col;
  rg[o] = r; ug[o] = u; ng[o] = n;
}

// ---------------------------------------------------------------------------------------------------------------
// B10 (+ gate derivatives of the PREVIOUS step): G <- G + DP0 W_p0 + DQ0 W_q0h, then GRU backward of step s = t-1
// ---------------------------------------------------------------------------------------------------------------
struct DhArgs {
  const float *DP0, *DQ0;   // [B,H]   (null when has_gemm == 0)
  const float *WpT, *WqT;   // [R,H] in T16
  float* G;                 // [B,R] running gradient wrt the recurrent state (in/out)
  // step s (the step whose OUTPUT state G refers to); has_gates == 0 for the very first state
  const float *rg, *ug, *ng, *gh;   // [B,R] x3, [B,3R]
  const float* decin_s;             // [B,H+R] (h-part = state entering step s)
  const float* ddecin_s;            // [B,H+R] decoder gradient wrt decin row s
  float *dgi, *dgh;                 // [B,3R]
  int B, H, R, has_gemm, has_gates;
};

template <int NW>
__global__ __launch_bounds__(NW * 64) void dh_stage_kernel(const float* DP0, const float* DQ0, const float* WpT, const float* WqT,
                                                           float* G, unsigned b_h, int R, unsigned has, DhArgs a) {
  // the leading scalars (operand pointers, G, sizes) are preloaded into SGPRs; the struct comes by s_load and the saved gates are
  // prefetched by `mid`, after the operand loads have been issued (stages.h head_stage_kernel)
  const int B = b_h & 0xffff, H = b_h >> 16;
  const int has_gemm = has & 1, has_gates = (has >> 1) & 1;
  __shared__ float red[2 * NW * 256];
  const int r0 = blockIdx.y * 16, c0 = blockIdx.x * 16, wave = threadIdx.x >> 6;
  const int ldd = H + R;
  const int t = threadIdx.x & 255;
  const int row = r0 + (t >> 4), col = c0 + (t & 15);
  const bool own = threadIdx.x < 256 && row < B;
  const int rowc = row < B ? row : r0;  // clamped: unconditional prefetch
  const size_t o = (size_t)rowc * R + col, o3 = (size_t)rowc * 3 * R + col;
  const float g0 = G[o];
  float r = 0.f, u = 0.f, n = 0.f, hn = 0.f, hp = 0.f, dd = 0.f;
  auto prefetch = [&]() {
    if (has_gates) {  // wave-uniform
      r = a.rg[o]; u = a.ug[o]; n = a.ng[o]; hn = a.gh[o3 + 2 * R];
      hp = a.decin_s[(size_t)rowc * ldd + H + col];
      dd = a.ddecin_s[(size_t)rowc * ldd + H + col];
    }
  };
  float v[2] = {0.f, 0.f};
  if (has_gemm) {
    f32x4 acc[2];
    acc[0] = (f32x4){0.f, 0.f, 0.f, 0.f};
    acc[1] = (f32x4){0.f, 0.f, 0.f, 0.f};
    {
      const float* const As[2] = {DP0, DQ0};
      const float* const Ws[2] = {WpT, WqT};
      const int ld[2] = {H, H}, cs[2] = {c0, c0};
      wave_gemm16_multi<NW, 2, false>(As, ld, r0, B, Ws, ld, cs, H, wave, acc, prefetch);
    }
    reduce_tiles<2, NW>(acc, red, v);
  } else {
    prefetch();
  }
  if (!own) return;
  const float g = g0 + v[0] + v[1];
  if (!has_gates) { G[o] = g; return; }
  const float dn_pre = g * (1.f - u) * (1.f - n * n);
  const float du_pre = g * (hp - n) * u * (1.f - u);
  const float dr_pre = dn_pre * hn * r * (1.f - r);
  a.dgi[o3] = dr_pre; a.dgi[o3 + R] = du_pre; a.dgi[o3 + 2 * R] = dn_pre;
  a.dgh[o3] = dr_pre; a.dgh[o3 + R] = du_pre; a.dgh[o3 + 2 * R] = dn_pre * r;
  G[o] = g * u + dd;
}

// Batches of 65 .. 256 utterances run the VRNN programs on ROW GROUPS of two row tiles (pchain_rt.h: 32-row tiles, the weight
// fragments fetched once per group).  Measured per train step on one box, [B,16000] fp32: B = 128 22.6 ms (24.7 on 16-row tiles,
// two per workgroup and link), B = 192 28.7 (36.9 as a launch per link), B = 256 38.6 (40.1).  Groups of FOUR row tiles were slower
// everywhere (B = 128: 34.8, 256: 40.7; removed): a tile costs ~1.3 us + ~1.1 us per row tile it carries (polled fragments, MFMAs, reduction,
// epilogue stores), so fatter tiles only trade workgroups for latency; beyond 256 utterances a link has more 32-row tiles than the
// chip has workgroups for it and the launch-per-link path on 32 x 32 tiles takes over.  fp32 operands only.
// env BLVM_PCHAIN_RT_MIN_B / BLVM_PCHAIN_RT_MAX_B: the batch range (default 65 .. 256; MAX_B = 0: never).
inline int vrnn_rt_max_b() {
  static int v = [] {
    const char* e = getenv("BLVM_PCHAIN_RT_MAX_B");
    return e ? atoi(e) : 256;
  }();
  return v;
}
inline int vrnn_rt(int B) {
  static const int min_b = [] { const char* e = getenv("BLVM_PCHAIN_RT_MIN_B"); return e ? atoi(e) : 65; }();
  if (B < min_b || B > vrnn_rt_max_b() || pchain_max_batch() <= 0 || operand_16bit()) return 0;
  if (B <= kPchainCarveMaxB && B > pchain_max_batch()) return 0;
  return 2;
}
inline bool vrnn_row_groups(int B) { return vrnn_rt(B) > 0; }
// SHARED deal of the row-group programs: the gentle link (hidden projection; backward: the hidden-gradient product) owns no range of
// workgroups -- the chip is two halves (prior | posterior) and the gentle link runs on the posterior half right after that half's
// run, in the window in which only the prior half works (heads + phi_z run; backward: dphi + phi_z run + dz).  Pays from 7 row groups
// per link (B > 208), where a link is throughput-bound and an own range for the gentle link starves the halves; at 4..6 groups the
// own range is as good or better, and on 16-row tiles (B <= 64: a link is one hand-off latency, not tile throughput) it LOSES --
// measured r03, [64,16000]: forward 5.68 -> 7.30 ms, the three serial gentle tiles end after the prior half's run and the GRU waits.
// env BLVM_PCHAIN_SHARED = 0 | 1 overrides (any batch); BLVM_PCHAIN_RT_SHARED_TL: the row-group threshold.
inline bool vrnn_shared_deal(bool groups, int tl) {
  static const int forced = [] { const char* e = getenv("BLVM_PCHAIN_SHARED"); return e ? atoi(e) : -1; }();
  static const int rt_tl = [] { const char* e = getenv("BLVM_PCHAIN_RT_SHARED_TL"); return e ? atoi(e) : 7; }();
  if (forced >= 0) return forced != 0;
  return groups && rt_tl > 0 && tl >= rt_tl;  // (threshold 0: never)
}
inline bool vrnn_persistent(int B) { return pchain_applies(B) || vrnn_row_groups(B); }

// ---------------------------------------------------------------------------------------------------------------
// reserve / workspace carving
// ---------------------------------------------------------------------------------------------------------------
struct Reserve {
  float *P[3], *Q[3], *FZ[3], *GHb, *RG, *UG, *NG, *XQ, *XG, *RAWQ, *RAWP;
  float *Wp[3], *Wq[3], *Wph, *Wqh, *Wf[4], *Wih, *Whh;  // T16 copies of the weights the forward chain multiplies by
  // persistent forward (B <= kPchainCarveMaxB): T16 copies of every activation a link multiplies, per step [rt*16, width]
  float *H16, *P16[3], *Q16[3], *Z16, *FZ16[3], *PHI16;
  // decoder range of the forward launch (SF > 0; vrnn_static.h): the hand-off slabs of the decoder's first two layers, the polled
  // row-major partial sum of the first, and T16 copies of the three weights.  Carved behind everything else, so the pieces above
  // sit where the backward (which carves with SF = 0) looks for them.
  float *Y116, *Y216, *Y1P, *Wd[3];
  size_t x16_bytes;  // from the first piece a launch polls to the end of the T16 copies: sentinel-filled in one go
};

size_t carve_reserve(float* base, int Tp, int B, int H, int Z, int R, Reserve* r, int SF = 0) {
  const size_t n = (size_t)Tp * B;
  Arena ar{base};
  Reserve tmp;
  for (int i = 0; i < 3; ++i) tmp.P[i] = ar.take(n * H);
  for (int i = 0; i < 3; ++i) tmp.Q[i] = ar.take(n * H);
  for (int i = 0; i < 3; ++i) tmp.FZ[i] = ar.take(n * H);
  tmp.GHb = ar.take(n * 3 * R);
  tmp.RG = ar.take(n * R); tmp.UG = ar.take(n * R); tmp.NG = ar.take(n * R);
  tmp.XQ = ar.take(n * H);
  tmp.XG = ar.take(n * 3 * R);
  tmp.RAWQ = ar.take(n * Z); tmp.RAWP = ar.take(n * Z);
  tmp.Wp[0] = ar.take((size_t)H * R); tmp.Wq[0] = ar.take((size_t)H * R);
  for (int i = 1; i < 3; ++i) { tmp.Wp[i] = ar.take((size_t)H * H); tmp.Wq[i] = ar.take((size_t)H * H); }
  tmp.Wph = ar.take((size_t)2 * Z * H); tmp.Wqh = ar.take((size_t)2 * Z * H);
  tmp.Wf[0] = ar.take((size_t)H * Z);
  for (int i = 1; i < 4; ++i) tmp.Wf[i] = ar.take((size_t)H * H);
  tmp.Wih = ar.take((size_t)3 * R * H); tmp.Whh = ar.take((size_t)3 * R * R);
  tmp.H16 = nullptr;
  if (B <= kPchainCarveMaxB || B <= vrnn_rt_max_b()) {
    const size_t rows = (size_t)((B + 15) / 16) * 16, m = (size_t)Tp * rows;
    tmp.H16 = ar.take((m + rows) * R);
    for (int i = 0; i < 3; ++i) tmp.P16[i] = ar.take(m * H);
    for (int i = 0; i < 3; ++i) tmp.Q16[i] = ar.take(m * H);
    tmp.Z16 = ar.take(m * Z);
    for (int i = 0; i < 3; ++i) tmp.FZ16[i] = ar.take(m * H);
    tmp.PHI16 = ar.take(m * H);
    tmp.Y116 = tmp.Y216 = tmp.Y1P = nullptr;
    if (SF > 0) { tmp.Y116 = ar.take(m * H); tmp.Y216 = ar.take(m * H); tmp.Y1P = ar.take(n * H); }
    tmp.x16_bytes = ar.bytes_from(tmp.H16);
    if (SF > 0) { tmp.Wd[0] = ar.take((size_t)H * (H + R)); tmp.Wd[1] = ar.take((size_t)H * H); tmp.Wd[2] = ar.take((size_t)SF * H); }
  }
  if (r) *r = tmp;
  return ar.floats();
}

struct BwdWs {
  float *pT[3], *phT, *qT[3], *qhT, *fT[4], *wihT, *whhT;   // transposed weights, T16
  float *DGI, *DGH, *DPHI[4], *DQH, *DPH, *DP[3], *DQ[3], *G;
  // persistent backward (B <= kPchainCarveMaxB): the running state gradient as per-step slabs (written once each), [T',B,R], and
  // T16 copies of every gradient a link multiplies, per step [rt*16, width]
  float *GA, *GB, *DP16[3], *DQ16[3], *DGI16, *DGH16, *DPHI16[4], *DPH16, *DQH16, *DPHI16b, *DPHI16c;
  size_t x16_bytes;  // from the first piece a launch polls to the end of the T16 copies: sentinel-filled in one go
  float *DPHI3b, *DPHI3c;  // row-major partial sums of DPHI[3] when its K = 3R product is split over three links (added up after the launch)
  // decoder leader of the backward launch (SF > 0; vrnn_static.h): the hand-off slabs of the decoder's two hidden gradients, the polled
  // row-major gradient of the decoder's input [T',B,H+R] (inside the sentinel-filled stretch), and the transposed T16 copies of the
  // three weights (behind everything else)
  float *DY216, *DY116, *DD, *dT[3];
  // d_enc follower of the backward launch (enc; vrnn_static.h): the transposed T16 copies of the encoding's columns of the GRU input
  // weight and of the posterior's first layer, and the polled row-major product EP = DGI W_ih[:, :X] [T',B,X] — behind everything
  // else, so the pieces above sit where a call that does not fold looks for them
  float *wixT, *qxT, *EP;
};

size_t carve_ws(float* base, int Tp, int B, int X, int H, int Z, int R, BwdWs* w, int SF = 0, bool enc = false) {
  const size_t n = (size_t)Tp * B;
  Arena ar{base};
  BwdWs t;
  t.pT[0] = ar.take((size_t)R * H); t.pT[1] = ar.take((size_t)H * H); t.pT[2] = ar.take((size_t)H * H);
  t.phT = ar.take((size_t)H * 2 * Z);
  t.qT[0] = ar.take((size_t)R * H); t.qT[1] = ar.take((size_t)H * H); t.qT[2] = ar.take((size_t)H * H);
  t.qhT = ar.take((size_t)H * 2 * Z);
  t.fT[0] = ar.take((size_t)Z * H);
  for (int i = 1; i < 4; ++i) t.fT[i] = ar.take((size_t)H * H);
  t.wihT = ar.take((size_t)H * 3 * R);
  t.whhT = ar.take((size_t)R * 3 * R);
  t.DGI = ar.take(n * 3 * R); t.DGH = ar.take(n * 3 * R);
  for (int i = 0; i < 4; ++i) t.DPHI[i] = ar.take(n * H);
  t.DQH = ar.take(n * 2 * Z); t.DPH = ar.take(n * 2 * Z);
  for (int i = 0; i < 3; ++i) t.DP[i] = ar.take(n * H);
  for (int i = 0; i < 3; ++i) t.DQ[i] = ar.take(n * H);
  t.G = ar.take((size_t)B * R);
  t.GA = nullptr;
  if (B <= kPchainCarveMaxB || B <= vrnn_rt_max_b()) {
    const size_t m = (size_t)Tp * ((B + 15) / 16) * 16;
    t.GA = ar.take(n * R); t.GB = ar.take(n * R);
    for (int i = 0; i < 3; ++i) { t.DP16[i] = ar.take(m * H); t.DQ16[i] = ar.take(m * H); }
    t.DGI16 = ar.take(m * 3 * R); t.DGH16 = ar.take(m * 3 * R);
    for (int i = 0; i < 4; ++i) t.DPHI16[i] = ar.take(m * H);
    t.DPH16 = ar.take(m * 2 * Z); t.DQH16 = ar.take(m * 2 * Z);
    t.DPHI16b = ar.take(m * H); t.DPHI16c = ar.take(m * H);
    t.DY216 = t.DY116 = t.DD = nullptr;
    if (SF > 0) { t.DY216 = ar.take(m * H); t.DY116 = ar.take(m * H); t.DD = ar.take(n * (H + R)); }
    t.x16_bytes = ar.bytes_from(t.GA);
    t.DPHI3b = ar.take(n * H); t.DPHI3c = ar.take(n * H);
    if (SF > 0) { t.dT[0] = ar.take((size_t)(H + R) * H); t.dT[1] = ar.take((size_t)H * H); t.dT[2] = ar.take((size_t)H * SF); }
  }
  t.wixT = t.qxT = t.EP = nullptr;
  if (enc) { t.wixT = ar.take((size_t)3 * R * X); t.qxT = ar.take((size_t)H * X); t.EP = ar.take(n * X); }
  if (w) *w = t;
  return ar.floats();
}

// a += b + c over n4 float4 (the three partial sums of DPHI[3])
__global__ __launch_bounds__(256) void add3_kernel(float4* __restrict__ a, const float4* __restrict__ b, const float4* __restrict__ c, size_t n4) {
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (size_t)gridDim.x * 256) {
    float4 x = a[i];
    const float4 y = b[i], z = c[i];
    x.x += y.x + z.x; x.y += y.y + z.y; x.z += y.z + z.z; x.w += y.w + z.w;
    a[i] = x;
  }
}

// the K = 3R link of the persistent backward as three K = R links (env BLVM_PCHAIN_SPLIT3=0: one link)
inline bool pchain_split3() {
  static int v = [] {
    const char* e = getenv("BLVM_PCHAIN_SPLIT3");
    return e ? atoi(e) : 1;
  }();
  return v != 0;
}

struct VrnnDecoder {  // blvm_vrnn_seq_fwd_dec's three layers and the activations it writes
  const float *w[3], *b[3];
  float* y[3];
};
// the decoder MLP inside the forward launch (blvm_vrnn_seq_fwd_dec; blvm_vrnn_dec_fold; env BLVM_VRNN_DEC_FOLD=0: never)
// 0: never; 1: all three layers; 2: the first two only (the last layer stays a K6 launch of the caller's)
int g_dec_fold = [] { const char* e = getenv("BLVM_VRNN_DEC_FOLD"); const int v = e ? atoi(e) : 1; return v >= 0 && v <= 2 ? v : 1; }();
long g_dec_folded = 0;  // forward calls that computed the decoder inside the launch
// How many layers of the decoder a forward call folds (0 | 2 | 3; the deal it then runs on is dec_ct's).  Needed: fp32 operands,
// 16-row tiles without row groups, the own-range deal, Z == H (the phi_z run is one descriptor), a decoder of hidden width H whose
// output is whole 16-column tiles, and a decoder range in which every link fits (vrnn_static.h).
int dec_ct(int layers, int SF) { return layers == 3 ? SF / 16 : layers == 2 ? 1 : 0; }  // vrnn_fwd_deal's ctD (two layers: dec[3] is not used)
int vrnn_dec_folds(int B, int H, int Z, int R, int DH, int SF) {
  if (!g_dec_fold || !vrnn_persistent(B) || device_cus() < 32 || operand_16bit() || pchain_optype(B) != OP_F32) return 0;
  if (B > 64 || vrnn_row_groups(B) || Z != H || DH != H || SF <= 0 || SF % 16 != 0) return 0;
  const int tl = (B + 15) / 16, layers = g_dec_fold == 2 ? 2 : 3;
  const bool fits = pchain::vrnn_fwd_deal(H / 16, Z / 16, R / 16, tl, device_cus() & ~7, vrnn_shared_deal(false, tl), dec_ct(layers, SF)).dec[0].nwg > 0;
  return fits ? layers : 0;
}

// blvm_vrnn_seq_bwd_dec: the decoder's data gradients on the backward walk's spare range (vrnn_static.h "decoder leader")
struct VrnnDecBwd {
  const float *dz3, *y1, *y2, *w[3];  // gradient of the last pre-activation [T'B, SF]; the two hidden activations; the three weights
  float *dy2, *dy1;                   // out: gradients of the hidden pre-activations [T'B, DH] (the caller's weight gradients read them)
  int DH, SF;
  float slope;
};
// blvm_vrnn_dec_bwd_fold; env BLVM_VRNN_DEC_BWD_FOLD=0: never
int g_dec_bwd_fold = [] { const char* e = getenv("BLVM_VRNN_DEC_BWD_FOLD"); return e ? (atoi(e) != 0 ? 1 : 0) : 1; }();
long g_dec_bwd_folded = 0;  // backward calls that computed the decoder's data gradients inside the launch
// Whether a backward call folds: where the forward fold applies (vrnn_dec_folds' conditions) and in addition the walk has the
// static kernels' widths, the backward program takes its split3 form on the own-range deal, the deal has a leader range, and the
// walk is long enough to arm its slabs (vrnn_static.h kArmAhead) and to lead (kBdecAhead).
bool vrnn_dec_bwd_folds(int Tp, int B, int H, int Z, int R, int DH, int SF) {
  if (!g_dec_bwd_fold || !vrnn_persistent(B) || device_cus() < 32 || operand_16bit() || pchain_optype(B) != OP_F32) return false;
  if (B > 64 || vrnn_row_groups(B) || Z != H || DH != H || H != 256 || R != 512 || SF <= 0 || SF % 16 != 0) return false;
  if (Tp + 1 <= pchain::kArmAhead || Tp <= pchain::kBdecAhead) return false;
  const int tl = (B + 15) / 16;
  if (vrnn_shared_deal(false, tl)) return false;
  const pchain::VrnnBwdDeal dl = pchain::vrnn_bwd_deal(H / 16, Z / 16, R / 16, tl, device_cus() & ~7, false, pchain_split3(), (H + R) / 16);
  return dl.split3 && dl.bdec[0].nwg > 0;
}

// d_enc = DQ0 Wq0[:, R:] + DGI W_ih[:, :X] on the backward walk's posterior half (vrnn_static.h "d_enc follower") instead of two K6
// launches behind the walk.  blvm_vrnn_enc_bwd_fold; env BLVM_VRNN_ENC_BWD_FOLD=0: never
int g_enc_bwd_fold = [] { const char* e = getenv("BLVM_VRNN_ENC_BWD_FOLD"); return e ? (atoi(e) != 0 ? 1 : 0) : 1; }();
long g_enc_bwd_folded = 0;  // backward calls that computed d_enc inside the launch
// Whether a backward call that asks for d_enc folds it: fp32 operands on 16-row tiles without row groups, the static walk's widths
// with X = H, the split3 program on its own-range deal, a deal that gives every workgroup of the posterior half one follower tile,
// and a walk long enough to arm its slabs (vrnn_static.h kArmAhead).  The workspace is grown under the same conditions.
bool vrnn_enc_bwd_folds(int Tp, int B, int X, int H, int Z, int R) {
  if (!g_enc_bwd_fold || !vrnn_persistent(B) || device_cus() < 32 || operand_16bit() || pchain_optype(B) != OP_F32) return false;
  if (B > 64 || vrnn_row_groups(B) || Z != H || X != H || H != 256 || R != 512 || Tp <= pchain::kArmAhead) return false;
  const int tl = (B + 15) / 16;
  if (vrnn_shared_deal(false, tl)) return false;
  const pchain::VrnnBwdDeal dl = pchain::vrnn_bwd_deal(H / 16, Z / 16, R / 16, tl, device_cus() & ~7, false, pchain_split3(), 0, X / 16);
  return dl.split3 && dl.benc[0].nwg > 0;
}

// which implementation the sequence entry points took and which tiles their per-link loops ran on (blvm_vrnn_path_counts):
// host-side counts, [0..4] one per call ([4]: the calls of [0] and [2] whose program ran on row groups), [5..6] one per launch_lin
enum { VRNN_FWD_PROGRAM = 0, VRNN_FWD_PER_LINK = 1, VRNN_BWD_PROGRAM = 2, VRNN_BWD_PER_LINK = 3, VRNN_ROW_GROUPS = 4, VRNN_LIN16 = 5, VRNN_LIN32 = 6 };
std::atomic<unsigned long long> g_vrnn_counts[7];
inline void count_vrnn(int k) { g_vrnn_counts[k].fetch_add(1, std::memory_order_relaxed); }
inline void count_lin(int tile_width) { count_vrnn(tile_width == 32 ? VRNN_LIN32 : VRNN_LIN16); }

int check_dims(int Tp, int B, int X, int H, int Z, int R) {
  BLVM_REQUIRE(Tp > 0 && B > 0, "vrnn: bad Tp=%d B=%d", Tp, B);
  BLVM_REQUIRE(X > 0 && H > 0 && Z > 0 && R > 0 && X % 16 == 0 && H % 16 == 0 && Z % 16 == 0 && R % 16 == 0,
               "vrnn: X,H,Z,R must be positive multiples of 16 (got %d,%d,%d,%d)", X, H, Z, R);
  BLVM_REQUIRE(B < 65536 && H < 65536 && R < 65536, "vrnn: B, H and R must be below 65536 (packed kernel arguments)");
  return BLVM_OK;
}

}  // namespace
}  // namespace blvm

using namespace blvm;

extern "C" int blvm_vrnn_path_counts(unsigned long long out[7]) {
  BLVM_REQUIRE(out, "vrnn_path_counts: null pointer");
  for (int k = 0; k < 7; ++k) out[k] = g_vrnn_counts[k].load(std::memory_order_relaxed);
  return BLVM_OK;
}

extern "C" size_t blvm_vrnn_reserve_floats(int Tp, int B, int X, int H, int Z, int R) {
  (void)X;
  return carve_reserve(nullptr, Tp, B, H, Z, R, nullptr);
}
extern "C" size_t blvm_vrnn_fwd_reserve_floats(int Tp, int B, int X, int H, int Z, int R, int DH, int SF) {
  (void)X;
  return carve_reserve(nullptr, Tp, B, H, Z, R, nullptr, vrnn_dec_folds(B, H, Z, R, DH, SF) ? SF : 0);  // (grown only where the call folds)
}
extern "C" int blvm_vrnn_dec_fold(int mode) {
  if (mode == -2) return (int)std::min<long>(g_dec_folded, 0x7fffffffL);
  const int was = g_dec_fold;
  if (mode >= 0) g_dec_fold = mode <= 2 ? mode : 1;
  return was;
}

extern "C" size_t blvm_vrnn_bwd_workspace_floats(int Tp, int B, int X, int H, int Z, int R) {
  return carve_ws(nullptr, Tp, B, X, H, Z, R, nullptr, 0, vrnn_enc_bwd_folds(Tp, B, X, H, Z, R));  // (grown only where d_enc folds)
}
extern "C" size_t blvm_vrnn_bwd_dec_workspace_floats(int Tp, int B, int X, int H, int Z, int R, int DH, int SF) {
  return carve_ws(nullptr, Tp, B, X, H, Z, R, nullptr, vrnn_dec_bwd_folds(Tp, B, H, Z, R, DH, SF) ? SF : 0,  // (grown only where the call folds)
                  vrnn_enc_bwd_folds(Tp, B, X, H, Z, R));
}
extern "C" int blvm_vrnn_enc_bwd_fold(int mode) {
  if (mode == -2) return (int)std::min<long>(g_enc_bwd_folded, 0x7fffffffL);
  const int was = g_enc_bwd_fold;
  if (mode >= 0) g_enc_bwd_fold = mode != 0;
  return was;
}
extern "C" int blvm_vrnn_dec_bwd_fold(int mode) {
  if (mode == -2) return (int)std::min<long>(g_dec_bwd_folded, 0x7fffffffL);
  const int was = g_dec_bwd_fold;
  if (mode >= 0) g_dec_bwd_fold = mode != 0;
  return was;
}

static int vrnn_seq_fwd_impl(const BlvmVrnnWeights* w, const float* enc, const float* h0, const float* eps,
                             int Tp, int B, int X, int H, int Z, int R, int residual_posterior, float sd_eps,
                             float* decin, float* mu_q, float* sd_q, float* mu_p, float* sd_p, float* z,
                             float* reserve, hipStream_t s, const VrnnDecoder* dec = nullptr, int DH = 0, int SF = 0,
                             float dec_slope = 0.f, int* folded = nullptr) {
  BLVM_TRY(check_dims(Tp, B, X, H, Z, R));
  BLVM_REQUIRE(w && enc && eps && decin && mu_q && sd_q && mu_p && sd_p && z && reserve, "vrnn_fwd: null pointer");
  BLVM_REQUIRE(aligned16(enc) && aligned16(decin) && aligned16(reserve) && aligned16(z),
               "vrnn_fwd: buffers must be 16-byte aligned");
  if (folded) *folded = 0;
  // dec != null: the reserve is blvm_vrnn_fwd_reserve_floats(..., DH, SF) floats; the decoder runs inside the launch where that applies
  const int fold = dec != nullptr ? vrnn_dec_folds(B, H, Z, R, DH, SF) : 0;  // layers of the decoder inside the launch
  Reserve rs;
  carve_reserve(reserve, Tp, B, H, Z, R, &rs, fold ? SF : 0);
  const size_t n = (size_t)Tp * B;
  const int ldd = H + R;
  const float beta = softplus_beta_of(sd_eps);  // ln2 / (initial_sd - eps), initial_sd = 1

  // hoisted, state-independent halves of the two concatenated-input layers
  BLVM_TRY(gemm_f32(0, 0, (int)n, H, X, enc, X, w->post_w[0] + R, R + X, rs.XQ, H, w->post_b[0], 0, 0.f, nullptr, 0, 0, 1, s));
  BLVM_TRY(gemm_f32(0, 0, (int)n, 3 * R, X, enc, X, w->gru_wih, X + H, rs.XG, 3 * R, w->gru_bih, 0, 0.f, nullptr, 0, 0, 1, s));

  // T16 operand copies of the chain's weights (once per sequence)
  T16PackScope pack_scope(pchain_optype(B), s);  // 16-bit operand modes: the persistent launch multiplies 16-bit weight packs
  BLVM_TRY(t16_pack_rows(w->prior_w[0], R, H, R, rs.Wp[0], s));
  BLVM_TRY(t16_pack_rows(w->post_w[0], R + X, H, R, rs.Wq[0], s));  // the h columns
  for (int l = 1; l < 3; ++l) {
    BLVM_TRY(t16_pack_rows(w->prior_w[l], H, H, H, rs.Wp[l], s));
    BLVM_TRY(t16_pack_rows(w->post_w[l], H, H, H, rs.Wq[l], s));
  }
  BLVM_TRY(t16_pack_rows(w->prior_hw, H, 2 * Z, H, rs.Wph, s));
  BLVM_TRY(t16_pack_rows(w->post_hw, H, 2 * Z, H, rs.Wqh, s));
  BLVM_TRY(t16_pack_rows(w->phi_w[0], Z, H, Z, rs.Wf[0], s));
  for (int l = 1; l < 4; ++l) BLVM_TRY(t16_pack_rows(w->phi_w[l], H, H, H, rs.Wf[l], s));
  BLVM_TRY(t16_pack_rows(w->gru_wih + X, X + H, 3 * R, H, rs.Wih, s));  // the phi columns
  BLVM_TRY(t16_pack_rows(w->gru_whh, R, 3 * R, R, rs.Whh, s));
  if (fold) {
    BLVM_TRY(t16_pack_rows(dec->w[0], H + R, H, H + R, rs.Wd[0], s));
    BLVM_TRY(t16_pack_rows(dec->w[1], H, H, H, rs.Wd[1], s));
    if (fold == 3) BLVM_TRY(t16_pack_rows(dec->w[2], H, SF, H, rs.Wd[2], s));
  }
  BLVM_TRY(pack_scope.flush());  // all packs above in one launch

  // initial state -> h-part of decin row 0 (the persistent path writes it behind its sentinel fill of decin, below)
  if (!(vrnn_persistent(B) && device_cus() >= 32)) BLVM_HIP(copy_or_zero_2d(decin + H, sizeof(float) * ldd, h0, sizeof(float) * R, B, s));
  // the phi-part of the extra row T' has no producer (there is no step T'): zeros, so that no word of decin keeps the caller's bytes
  BLVM_HIP(hipMemset2DAsync(decin + n * ldd, sizeof(float) * ldd, 0, sizeof(float) * H, B, s));

  const int rt = (B + 15) / 16;
  if (vrnn_persistent(B) && device_cus() >= 32) {
    // Persistent path (pchain.h / pchain.hip): the nine links of a step as a program of 13 descriptors, one launch for the whole
    // sequence.  Links on the critical path share the workgroups [0, g); the GRU's hidden projection gh_t = h_{t-1} W_hh^T + b_hh
    // (3R columns, first needed by the GRU link's epilogue eight links later) has its own range behind them and polls gently.
    using namespace pchain;
    const int ctH = H / 16, ctZ = Z / 16, ctR = R / 16, cus = device_cus() & ~7;
    const long sH = (long)B * H, sZ = (long)B * Z, sR = (long)B * R, s3R = 3 * sR, sD = (long)B * ldd;
    const long xH = (long)rt * 16 * H, xZ = (long)rt * 16 * Z, xR = (long)rt * 16 * R;
    // tiles of a link per column tile: row tiles, or (65 <= B <= 256) groups of row tiles (pchain_rt.h)
    const bool groups = vrnn_row_groups(B);
    count_vrnn(VRNN_FWD_PROGRAM);
    if (groups) count_vrnn(VRNN_ROW_GROUPS);
    const int RTG = groups ? vrnn_rt(B) : 1;
    const int tl = (rt + RTG - 1) / RTG;
    // hidden projection: up to a quarter of the chip
    // shared deal (row groups, many row tiles): no range of its own for the hidden projection -- it runs on the posterior half after that
    // half's run, in the window where only the prior half works on the heads and the phi_z run
    const bool shared = vrnn_shared_deal(groups, tl);
    const VrnnFwdDeal dl = vrnn_fwd_deal(ctH, ctZ, ctR, tl, cus, shared, dec_ct(fold, SF));  // (vrnn_static.h: the ranges of every link)
    Builder bld;
    bld.begin(pchain_optype(B), Tp, B, groups ? 8 : 4, false, dl.g);
    bld.p.rt_group = RTG;
    // F1: hidden projection (the first prior layer and the h-half of the first posterior layer open the runs below)
    Operands hp;
    hp.p[LIN_A] = {rs.H16, xR}; hp.p[LIN_W] = rs.Whh; hp.p[LIN_BIAS] = w->gru_bhh; hp.p[LIN_ORM] = {rs.GHb, s3R}; hp.ld[LD_OUT] = 3 * R;
    auto hproj = [&]() { add_desc(bld, K_LIN, dl.hproj.ct, dl.hproj.wg0, dl.hproj.nwg, R, DF_RM_SC1 | DF_GENTLE | ((pchain_tune() & 16) ? DF_CANARY : 0), 0, Tp, hp); };
    if (!shared) hproj();
    // F1 .. F3 of a chain: one visit.  The link in front of a run of same-shape links joins the run's descriptor visit (its own K = R,
    // the posterior's with its x-part addend): one visit less per chain and step (~1 us each, tools/probe_engine_chain.py)
    {
      const SeqLink lp[3] = {{rs.Wp[0], w->prior_b[0], rs.P[0], sH, H, rs.P16[0]}, {rs.Wp[1], w->prior_b[1], rs.P[1], sH, H, rs.P16[1]}, {rs.Wp[2], w->prior_b[2], rs.P[2], sH, H, rs.P16[2]}};
      const SeqLink lq[3] = {{rs.Wq[0], nullptr, rs.Q[0], sH, H, rs.Q16[0]}, {rs.Wq[1], w->post_b[1], rs.Q[1], sH, H, rs.Q16[1]}, {rs.Wq[2], w->post_b[2], rs.Q[2], sH, H, rs.Q16[2]}};
      add_linseq(bld, ctH, dl.prior.wg0, dl.prior.nwg, H, true, false, 0, Tp, {rs.H16, xR}, 3, lp, 0, xH, ctH, 0.f, 0, R);
      add_linseq(bld, ctH, dl.post.wg0, dl.post.nwg, H, true, false, 0, Tp, {rs.H16, xR}, 3, lq, 0, xH, ctH, 0.f, 0, R, {rs.XQ, sH}, H);
    }
    if (shared) hproj();
    {  // F4: heads + sample
      Operands o;
      o.p[HEAD_P16] = {rs.P16[2], xH}; o.p[HEAD_Q16] = {rs.Q16[2], xH}; o.p[HEAD_WP] = rs.Wph; o.p[HEAD_BP] = w->prior_hb; o.p[HEAD_WQ] = rs.Wqh;
      o.p[HEAD_BQ] = w->post_hb; o.p[HEAD_EPS] = {eps, sZ}; o.p[HEAD_MU_P] = {mu_p, sZ}; o.p[HEAD_SD_P] = {sd_p, sZ}; o.p[HEAD_MU_Q] = {mu_q, sZ};
      o.p[HEAD_SD_Q] = {sd_q, sZ}; o.p[HEAD_RAW_P] = {rs.RAWP, sZ}; o.p[HEAD_RAW_Q] = {rs.RAWQ, sZ}; o.p[HEAD_Z] = {z, sZ}; o.p[HEAD_Z16] = {rs.Z16, xZ};
      o.ld[LD_OUT] = Z; o.n16[N16_OUT] = ctZ; o.i[HEAD_I_Z] = Z; o.i[HEAD_I_RESIDUAL] = residual_posterior; o.f[HEAD_F_BETA] = beta; o.f[HEAD_F_INV_BETA] = 1.f / beta;
      o.f[HEAD_F_SD_EPS] = sd_eps;
      add_desc(bld, K_HEAD, ctZ, dl.head.wg0, dl.head.nwg, H, 0, 0, Tp, o);
    }
    // F5..F8: phi_z MLP (the last layer writes phi into decin row t)
    const int first_seq = Z == H ? 0 : 1;  // (the first layer's K is Z: part of the run only when Z == H)
    if (first_seq) {
      Operands o;
      o.p[LIN_A] = {rs.Z16, xZ}; o.p[LIN_W] = rs.Wf[0]; o.p[LIN_BIAS] = w->phi_b[0]; o.p[LIN_ORM] = {rs.FZ[0], sH}; o.ld[LD_OUT] = H; o.p[LIN_O16] = {rs.FZ16[0], xH};
      o.n16[N16_OUT] = ctH;
      add_desc(bld, K_LIN, ctH, dl.phi.wg0, dl.phi.nwg, Z, DF_RELU, 0, Tp, o);
    }
    {
      SeqLink lf[4];
      for (int l = first_seq; l < 4; ++l)
        lf[l - first_seq] = SeqLink{rs.Wf[l], w->phi_b[l], l == 3 ? decin : rs.FZ[l], l == 3 ? sD : sH, l == 3 ? ldd : H, l == 3 ? rs.PHI16 : rs.FZ16[l]};
      add_linseq(bld, ctH, dl.phi.wg0, dl.phi.nwg, H, true, false, 0, Tp, first_seq == 0 ? Ptr(rs.Z16, xZ) : Ptr(rs.FZ16[0], xH), 4 - first_seq,
                 lf, 0, xH, ctH, 0.f, 0);
    }
    {  // F9: GRU
      Operands o;
      o.p[GRU_X16] = {rs.PHI16, xH}; o.p[GRU_WIH] = rs.Wih; o.p[GRU_XG] = {rs.XG, s3R}; o.p[GRU_GH] = {rs.GHb, s3R}; o.p[GRU_HPREV] = {decin + H, sD};
      o.p[GRU_HRM] = {decin + sD + H, sD}; o.p[GRU_H16] = {rs.H16 + xR, xR}; o.p[GRU_RG] = {rs.RG, sR}; o.p[GRU_UG] = {rs.UG, sR}; o.p[GRU_NG] = {rs.NG, sR};
      o.ld[GRU_LD_HPREV] = ldd; o.ld[LD_OUT] = ldd; o.n16[N16_OUT] = ctR; o.i[GRU_I_R] = R;
      add_desc(bld, K_GRU, ctR, dl.gru.wg0, dl.gru.nwg, H, 0, 0, Tp, o);
    }
    if (fold) {
      // The decoder of step t behind the chain, on the workgroups the deal leaves free (vrnn_static.h): row t of decin = [phi_t | h_t]
      // arrives as the slabs PHI16[t] and H16[t].  The first layer's K = H + R product is two links over the two K-ranges of its packed
      // rows: the h-part (with the bias) can run as soon as the step begins, the phi-part adds it in its epilogue.  Every layer ends in
      // the activation, as the K6 chain's does.  Outputs: the activations the decoder's backward reads (y[0], y[1], y[2] row-major).
      const long sF = (long)B * SF;
      const int canary = (pchain_tune() & 16) ? DF_CANARY : 0, ldw = H + R;
      Operands o;
      o.p[LIN_A] = {rs.H16, xR}; o.p[LIN_W] = rs.Wd[0] + (size_t)ctH * 256; o.i[LIN_I_W_WIDTH] = ldw; o.p[LIN_BIAS] = dec->b[0];
      o.p[LIN_ORM] = {rs.Y1P, sH}; o.ld[LD_OUT] = H;
      add_desc(bld, K_LIN, dl.dec[0].ct, dl.dec[0].wg0, dl.dec[0].nwg, R, DF_RM_SC1 | DF_GENTLE | canary, 0, Tp, o);
      o = Operands();
      o.p[LIN_A] = {rs.PHI16, xH}; o.p[LIN_W] = rs.Wd[0]; o.i[LIN_I_W_WIDTH] = ldw; o.p[LIN_ADD] = {rs.Y1P, sH}; o.ld[LIN_LD_ADD] = H;
      o.p[LIN_ORM] = {dec->y[0], sH}; o.ld[LD_OUT] = H; o.p[LIN_O16] = {rs.Y116, xH}; o.n16[N16_OUT] = ctH; o.f[LIN_F_SLOPE] = dec_slope;
      add_desc(bld, K_LIN, dl.dec[1].ct, dl.dec[1].wg0, dl.dec[1].nwg, H, DF_ADD_POLLED | DF_RELU | DF_GENTLE | canary, 0, Tp, o);
      o = Operands();
      o.p[LIN_A] = {rs.Y116, xH}; o.p[LIN_W] = rs.Wd[1]; o.p[LIN_BIAS] = dec->b[1]; o.p[LIN_ORM] = {dec->y[1], sH}; o.ld[LD_OUT] = H;
      o.p[LIN_O16] = {rs.Y216, xH}; o.n16[N16_OUT] = ctH; o.f[LIN_F_SLOPE] = dec_slope;
      add_desc(bld, K_LIN, dl.dec[2].ct, dl.dec[2].wg0, dl.dec[2].nwg, H, DF_RELU | DF_GENTLE | canary, 0, Tp, o);
      if (fold == 3) {  // (2: the last layer stays the caller's K6 launch on y[1])
        o = Operands();
        o.p[LIN_A] = {rs.Y216, xH}; o.p[LIN_W] = rs.Wd[2]; o.p[LIN_BIAS] = dec->b[2]; o.p[LIN_ORM] = {dec->y[2], sF}; o.ld[LD_OUT] = SF;
        o.f[LIN_F_SLOPE] = dec_slope;
        add_desc(bld, K_LIN, dl.dec[3].ct, dl.dec[3].wg0, dl.dec[3].nwg, H, DF_RELU | DF_GENTLE | canary, 0, Tp, o);
      }
    }
    // what the launch polls gets sentinels: the T16 copies, the hidden projection, and decin (the GRU link polls words of h).  Who
    // stores them is the launch's decision (vrnn_static.h ArmPlan): the full regions, or the table's buffers slab by slab.
    ArmPlan plan;
    plan.fill(rs.H16, rs.x16_bytes);
    plan.fill(rs.GHb, sizeof(float) * n * 3 * R);
    plan.fill(decin, sizeof(float) * n * ldd);  // rows 0..T'-1; row T' only receives h_n
    if (!groups) {
      plan.add(arm_t16(rs.H16, R, rt, Tp + 1));
      for (int i = 0; i < 3; ++i) { plan.add(arm_t16(rs.P16[i], H, rt, Tp)); plan.add(arm_t16(rs.Q16[i], H, rt, Tp)); plan.add(arm_t16(rs.FZ16[i], H, rt, Tp)); }
      plan.add(arm_t16(rs.Z16, Z, rt, Tp));
      plan.add(arm_t16(rs.PHI16, H, rt, Tp));
      plan.add(arm_t16(rs.Y116, H, rt, Tp)); plan.add(arm_t16(rs.Y216, H, rt, Tp));  // (null without the decoder range: not added)
      plan.add(arm_rm(rs.Y1P, H, B, Tp));
      plan.add(arm_rm(rs.GHb, 3 * R, B, Tp));
      plan.add(arm_rm(decin, ldd, B, Tp));
    }
    // the initial state is step 0's operand: both writes go behind the fill
    auto pre = [&]() -> int {
      BLVM_HIP(copy_or_zero_2d(decin + H, sizeof(float) * ldd, h0, sizeof(float) * R, B, s));
      return pchain_rows_to_t16(h0, R, B, R, rs.H16, s);
    };
    BLVM_TRY(vrnn_launch(bld, true, "vrnn_fwd", s, plan, pre));
    if (fold) { ++g_dec_folded; if (folded) *folded = fold; }
    return BLVM_OK;
  }
  count_vrnn(VRNN_FWD_PER_LINK);
  for (int t = 0; t < Tp; ++t) {
    const size_t oH = (size_t)t * B * H, oZ = (size_t)t * B * Z, oR = (size_t)t * B * R, o3R = (size_t)t * B * 3 * R;
    const float* dec_t = decin + (size_t)t * B * ldd;
    float* dec_n = decin + (size_t)(t + 1) * B * ldd;
    const float* hprev = dec_t + H;
    LinLaunch a;
    a.B = B;
    // F1: first prior layer | h-half of first posterior layer | GRU hidden projection
    a.nseg = 3;
    a.seg[0] = seg(hprev, ldd, rs.Wp[0], R, w->prior_b[0], nullptr, 0, nullptr, 0, rs.P[0] + oH, H, H, R, 1);
    a.seg[1] = seg(hprev, ldd, rs.Wq[0], R, nullptr, rs.XQ + oH, H, nullptr, 0, rs.Q[0] + oH, H, H, R, 1);
    a.seg[2] = seg(hprev, ldd, rs.Whh, R, w->gru_bhh, nullptr, 0, nullptr, 0, rs.GHb + o3R, 3 * R, 3 * R, R, 0);
    count_lin(launch_lin(a, s));
    // F2, F3
    a.nseg = 2;
    for (int l = 1; l < 3; ++l) {
      a.seg[0] = seg(rs.P[l - 1] + oH, H, rs.Wp[l], H, w->prior_b[l], nullptr, 0, nullptr, 0, rs.P[l] + oH, H, H, H, 1);
      a.seg[1] = seg(rs.Q[l - 1] + oH, H, rs.Wq[l], H, w->post_b[l], nullptr, 0, nullptr, 0, rs.Q[l] + oH, H, H, H, 1);
      count_lin(launch_lin(a, s));
    }
    // F4: heads + sample
    HeadArgs h;
    h.P = rs.P[2] + oH; h.Q = rs.Q[2] + oH;
    h.Wp = rs.Wph; h.bp = w->prior_hb; h.Wq = rs.Wqh; h.bq = w->post_hb;
    h.eps = eps + oZ;
    h.mu_p = mu_p + oZ; h.sd_p = sd_p + oZ; h.mu_q = mu_q + oZ; h.sd_q = sd_q + oZ; h.z = z + oZ;
    h.raw_p = rs.RAWP + oZ; h.raw_q = rs.RAWQ + oZ;
    h.B = B; h.H = H; h.Z = Z; h.residual = residual_posterior;
    h.beta = beta; h.inv_beta = 1.f / beta; h.sd_eps = sd_eps; h.muq_raw = nullptr;
    launch_head(h, pick_nw(H, 4), dim3(Z / 16, rt), s);
    // F5..F8: phi_z MLP (last layer writes phi into decin row t)
    a.nseg = 1;
    a.seg[0] = seg(z + oZ, Z, rs.Wf[0], Z, w->phi_b[0], nullptr, 0, nullptr, 0, rs.FZ[0] + oH, H, H, Z, 1);
    count_lin(launch_lin(a, s));
    a.seg[0] = seg(rs.FZ[0] + oH, H, rs.Wf[1], H, w->phi_b[1], nullptr, 0, nullptr, 0, rs.FZ[1] + oH, H, H, H, 1);
    count_lin(launch_lin(a, s));
    a.seg[0] = seg(rs.FZ[1] + oH, H, rs.Wf[2], H, w->phi_b[2], nullptr, 0, nullptr, 0, rs.FZ[2] + oH, H, H, H, 1);
    count_lin(launch_lin(a, s));
    a.seg[0] = seg(rs.FZ[2] + oH, H, rs.Wf[3], H, w->phi_b[3], nullptr, 0, nullptr, 0, decin + (size_t)t * B * ldd, ldd, H, H, 1);
    count_lin(launch_lin(a, s));
    // F9: GRU
    {
      const int nw = pick_nw(H, 3);
      const dim3 grid(R / 16, rt);
      const float *xg_t = rs.XG + o3R, *gh_t = rs.GHb + o3R;
      float *rg_t = rs.RG + oR, *ug_t = rs.UG + oR, *ng_t = rs.NG + oR;
      LAUNCH_NW(gru_stage_kernel<NW_>, nw, grid, s, dec_t, (const float*)rs.Wih, xg_t, gh_t, B, H, R, dec_n, rg_t, ug_t, ng_t);
    }
  }
  BLVM_CHECK_LAUNCH("vrnn_seq_fwd");
  return BLVM_OK;
}

extern "C" int blvm_vrnn_seq_fwd(const BlvmVrnnWeights* w, const float* enc, const float* h0, const float* eps,
                                 int Tp, int B, int X, int H, int Z, int R, int residual_posterior, float sd_eps,
                                 float* decin, float* mu_q, float* sd_q, float* mu_p, float* sd_p, float* z,
                                 float* reserve, void* stream_) {
  return vrnn_seq_fwd_impl(w, enc, h0, eps, Tp, B, X, H, Z, R, residual_posterior, sd_eps, decin, mu_q, sd_q, mu_p, sd_p, z, reserve,
                           static_cast<hipStream_t>(stream_));
}

extern "C" int blvm_vrnn_seq_fwd_dec(const BlvmVrnnWeights* w, const float* enc, const float* h0, const float* eps,
                                     int Tp, int B, int X, int H, int Z, int R, int residual_posterior, float sd_eps,
                                     float* decin, float* mu_q, float* sd_q, float* mu_p, float* sd_p, float* z,
                                     float* reserve, const float* const* dec_w, const float* const* dec_b, float* const* dec_y,
                                     int DH, int SF, float slope, int* folded, void* stream_) {
  BLVM_REQUIRE(dec_w && dec_b && dec_y && folded, "vrnn_seq_fwd_dec: null pointer");
  VrnnDecoder d;
  for (int l = 0; l < 3; ++l) {
    d.w[l] = dec_w[l]; d.b[l] = dec_b[l]; d.y[l] = dec_y[l];
    BLVM_REQUIRE(d.w[l] && d.b[l] && d.y[l] && aligned16(d.y[l]), "vrnn_seq_fwd_dec: decoder layer %d: null or unaligned pointer", l);
  }
  BLVM_REQUIRE(DH > 0 && SF > 0, "vrnn_seq_fwd_dec: bad decoder widths %d, %d", DH, SF);
  return vrnn_seq_fwd_impl(w, enc, h0, eps, Tp, B, X, H, Z, R, residual_posterior, sd_eps, decin, mu_q, sd_q, mu_p, sd_p, z, reserve,
                           static_cast<hipStream_t>(stream_), &d, DH, SF, slope, folded);
}

static int vrnn_seq_bwd_impl(const BlvmVrnnWeights* w, const float* enc, const float* eps, const float* decin,
                             const float* mu_q, const float* sd_q, const float* mu_p, const float* sd_p,
                             const float* z, const float* reserve, const float* d_decin, const int32_t* x_sl,
                             const float* c_raw, const float* c_fn, int stride, float fn_floor, int Tp, int B, int X, int H, int Z,
                             int R, int residual_posterior, float sd_eps, float* d_enc, float* d_h0,
                             const BlvmVrnnGrads* gr, float* workspace, hipStream_t s, const VrnnDecBwd* dec = nullptr) {
  // dec: the caller has checked vrnn_dec_bwd_folds — the decoder's data gradients run on the walk and d_decin is not read
  BLVM_TRY(check_dims(Tp, B, X, H, Z, R));
  BLVM_REQUIRE(w && enc && eps && decin && mu_q && sd_q && mu_p && sd_p && z && reserve && (d_decin || dec) && workspace && gr,
               "vrnn_bwd: null pointer");
  BLVM_REQUIRE((c_fn == nullptr && c_raw == nullptr) || x_sl != nullptr, "vrnn_bwd: KL coefficients need x_sl");
  BLVM_REQUIRE(aligned16(workspace) && aligned16(reserve) && aligned16(d_decin), "vrnn_bwd: buffers must be 16-byte aligned");
  Reserve rs;
  carve_reserve(const_cast<float*>(reserve), Tp, B, H, Z, R, &rs);
  // d_enc inside the launch: the workspace is blvm_vrnn_bwd_workspace_floats' under the same blvm_vrnn_enc_bwd_fold mode
  const bool encf = d_enc != nullptr && vrnn_enc_bwd_folds(Tp, B, X, H, Z, R);
  BLVM_REQUIRE(!encf || aligned16(d_enc), "vrnn_bwd: d_enc must be 16-byte aligned");
  BwdWs ws;
  carve_ws(workspace, Tp, B, X, H, Z, R, &ws, dec ? dec->SF : 0, encf);
  const size_t n = (size_t)Tp * B;
  const int ldd = H + R;
  const float beta = softplus_beta_of(sd_eps);

  // transposed T16 operand copies of every weight the chain multiplies from the right
  T16PackScope pack_scope(pchain_optype(B), s);  // 16-bit operand modes: the persistent launch multiplies 16-bit weight packs
  BLVM_TRY(t16_pack_transposed(w->prior_w[0], R, H, R, ws.pT[0], s));
  BLVM_TRY(t16_pack_transposed(w->prior_w[1], H, H, H, ws.pT[1], s));
  BLVM_TRY(t16_pack_transposed(w->prior_w[2], H, H, H, ws.pT[2], s));
  BLVM_TRY(t16_pack_transposed(w->prior_hw, H, 2 * Z, H, ws.phT, s));
  BLVM_TRY(t16_pack_transposed(w->post_w[0], R + X, H, R, ws.qT[0], s));
  BLVM_TRY(t16_pack_transposed(w->post_w[1], H, H, H, ws.qT[1], s));
  BLVM_TRY(t16_pack_transposed(w->post_w[2], H, H, H, ws.qT[2], s));
  BLVM_TRY(t16_pack_transposed(w->post_hw, H, 2 * Z, H, ws.qhT, s));
  BLVM_TRY(t16_pack_transposed(w->phi_w[0], Z, H, Z, ws.fT[0], s));
  for (int i = 1; i < 4; ++i) BLVM_TRY(t16_pack_transposed(w->phi_w[i], H, H, H, ws.fT[i], s));
  BLVM_TRY(t16_pack_transposed(w->gru_wih + X, X + H, 3 * R, H, ws.wihT, s));
  BLVM_TRY(t16_pack_transposed(w->gru_whh, R, 3 * R, R, ws.whhT, s));
  if (dec) {  // the decoder's three, in the same launch
    BLVM_TRY(t16_pack_transposed(dec->w[0], H + R, H, H + R, ws.dT[0], s));
    BLVM_TRY(t16_pack_transposed(dec->w[1], H, H, H, ws.dT[1], s));
    BLVM_TRY(t16_pack_transposed(dec->w[2], H, dec->SF, H, ws.dT[2], s));
  }
  if (encf) {  // the follower's two: the encoding's columns of the GRU input weight and of the posterior's first layer
    BLVM_TRY(t16_pack_transposed(w->gru_wih, X + H, 3 * R, X, ws.wixT, s));
    BLVM_TRY(t16_pack_transposed(w->post_w[0] + R, R + X, H, X, ws.qxT, s));
  }
  BLVM_TRY(pack_scope.flush());  // all packs above in one launch

  BLVM_HIP(hipMemsetAsync(ws.G, 0, sizeof(float) * (size_t)B * R, s));
  const int rt = (B + 15) / 16;

  auto launch_dh = [&](int t_gemm, int s_gates) {
    DhArgs d;
    d.has_gemm = t_gemm >= 0; d.has_gates = s_gates >= 0;
    d.DP0 = d.has_gemm ? ws.DP[0] + (size_t)t_gemm * B * H : nullptr;
    d.DQ0 = d.has_gemm ? ws.DQ[0] + (size_t)t_gemm * B * H : nullptr;
    d.WpT = ws.pT[0]; d.WqT = ws.qT[0]; d.G = ws.G;
    const size_t sg = d.has_gates ? (size_t)s_gates : 0;
    d.rg = rs.RG + sg * B * R; d.ug = rs.UG + sg * B * R; d.ng = rs.NG + sg * B * R;
    d.gh = rs.GHb + sg * B * 3 * R;
    d.decin_s = decin + sg * B * ldd; d.ddecin_s = d_decin + sg * B * ldd;
    d.dgi = ws.DGI + sg * B * 3 * R; d.dgh = ws.DGH + sg * B * 3 * R;
    d.B = B; d.H = H; d.R = R;
    {
      const int nw = pick_nw(H, 2);
      const dim3 grid(R / 16, rt);
      const unsigned b_h = (unsigned)B | ((unsigned)H << 16), has = (d.has_gemm ? 1u : 0u) | (d.has_gates ? 2u : 0u);
      LAUNCH_NW(dh_stage_kernel<NW_>, nw, grid, s, d.DP0, d.DQ0, d.WpT, d.WqT, d.G, b_h, R, has, d);
    }
  };

  // ---- batched, state-independent part: d(enc) and every weight gradient as large MFMA GEMMs over all rows ----
  // (Running them on a second stream under the latency-bound chain, in ranges of finished steps, measured slower on MI355X at
  // [64,16000]: 24.3 ms/step without overlap, 26.1 / 25.3 / 27.2 ms with ranges of 50 / 25 / 125 steps -- the big GEMM workgroups take
  // CU slots and memory-pipeline share from the chain's links; removed.)
  const float* hprev_all = decin + H;  // [n rows, ld = H+R]
  auto batched = [&]() -> int {
    if (d_enc && !encf) {
      BLVM_TRY(gemm_f32(0, 1, (int)n, X, H, ws.DQ[0], H, w->post_w[0] + R, R + X, d_enc, X, nullptr, 0, 0.f, nullptr, 0, 0, 1, s));
      BLVM_TRY(gemm_f32(0, 1, (int)n, X, 3 * R, ws.DGI, 3 * R, w->gru_wih, X + H, d_enc, X, nullptr, 0, 0.f, nullptr, 0, 1, 1, s));
    }
    // every weight gradient of the chain as ONE grouped launch (gemm.hip gemm_wgrad_group; D [rows, M] x Act [rows, N] -> dW [M, N], db [M])
    {
      WgradGroup grp;
      auto job = [&](const float* D, int ldd_, int n_out, const float* Act, int lda, int k_in, float* dW, int ldw, float* db = nullptr) {
        grp.add(D, ldd_, n_out, Act, lda, k_in, dW, ldw, db);
      };
      job(ws.DGI, 3 * R, 3 * R, enc, X, X, gr->gru_wih, X + H, gr->gru_bih);
      job(ws.DGI, 3 * R, 3 * R, decin, ldd, H, gr->gru_wih ? gr->gru_wih + X : nullptr, X + H);
      job(ws.DGH, 3 * R, 3 * R, hprev_all, ldd, R, gr->gru_whh, R, gr->gru_bhh);
      job(ws.DPHI[0], H, H, z, Z, Z, gr->phi_w[0], Z, gr->phi_b[0]);
      for (int l = 1; l < 4; ++l) job(ws.DPHI[l], H, H, rs.FZ[l - 1], H, H, gr->phi_w[l], H, gr->phi_b[l]);
      job(ws.DPH, 2 * Z, 2 * Z, rs.P[2], H, H, gr->prior_hw, H, gr->prior_hb);
      job(ws.DQH, 2 * Z, 2 * Z, rs.Q[2], H, H, gr->post_hw, H, gr->post_hb);
      for (int l = 2; l >= 1; --l) {
        job(ws.DP[l], H, H, rs.P[l - 1], H, H, gr->prior_w[l], H, gr->prior_b[l]);
        job(ws.DQ[l], H, H, rs.Q[l - 1], H, H, gr->post_w[l], H, gr->post_b[l]);
      }
      job(ws.DP[0], H, H, hprev_all, ldd, R, gr->prior_w[0], R, gr->prior_b[0]);
      job(ws.DQ[0], H, H, hprev_all, ldd, R, gr->post_w[0], R + X);
      job(ws.DQ[0], H, H, enc, X, X, gr->post_w[0] ? gr->post_w[0] + R : nullptr, R + X, gr->post_b[0]);
      BLVM_TRY(grp.run(n, s));
    }
    return BLVM_OK;
  };
  if (vrnn_persistent(B) && device_cus() >= 32) {
    // Persistent path: the whole BPTT chain as a program of 13 descriptors walked for s = 0 .. T' (t = T'-1-s: last-step slabs and
    // negative strides), then the batched weight-gradient GEMMs.  The running gradient wrt the recurrent state lives in per-step
    // slabs so that every location is written once: GA[t] = g_t * u_t + decoder gradient (written by the GRU-backward link),
    // GB[t] = GA[t] + DGH[t] W_hh (a K = 3R product nothing needs before the NEXT step's GRU-backward link: own range, gentle polls).
    using namespace pchain;
    const int ctH = H / 16, ctZ = Z / 16, ctR = R / 16, cus = device_cus() & ~7, T = Tp;
    const long sH = (long)B * H, sZ = (long)B * Z, sR = (long)B * R, s3R = 3 * sR, s2Z = 2 * sZ, sD = (long)B * ldd;
    const long xH = (long)rt * 16 * H, x2Z = (long)rt * 16 * 2 * Z, x3R = (long)rt * 16 * 3 * R;
    const bool groups = vrnn_row_groups(B);
    count_vrnn(VRNN_BWD_PROGRAM);
    if (groups) count_vrnn(VRNN_ROW_GROUPS);
    const int RTG = groups ? vrnn_rt(B) : 1;
    const int tl = (rt + RTG - 1) / RTG;  // tiles of a link per column tile: row tiles, or groups of them (pchain_rt.h)
    // (shared deal: see vrnn_fwd -- here the gentle link is GB, which the posterior half runs while the prior half
    // takes the gradient back through the phi_z run and the heads)
    const bool shared = vrnn_shared_deal(groups, tl);
    const VrnnBwdDeal dl = vrnn_bwd_deal(ctH, ctZ, ctR, tl, cus, shared, pchain_split3(), dec ? (H + R) / 16 : 0, encf ? X / 16 : 0);  // (vrnn_static.h: the ranges of every link)
    BLVM_REQUIRE(!dec || (dl.split3 && dl.bdec[0].nwg > 0 && !groups), "vrnn_bwd: the deal has no decoder leader range");
    BLVM_REQUIRE(!encf || (dl.split3 && dl.benc[0].nwg > 0 && !groups), "vrnn_bwd: the deal has no range for the d_enc follower");
    Builder bld;
    bld.begin(pchain_optype(B), T + 1, B, groups ? 8 : 2, true, dl.g);
    bld.p.rt_group = RTG;
    auto last = [&](const float* base, long step) { return rev(base, step, T - 1); };  // slab of t = T'-1, walked backwards
    {  // Ba: complete the gradient wrt h_t, GRU gate derivatives of step t (s = T': only the gradient wrt the initial state)
      Operands o;
      o.p[GRUB_D0_16] = rev(ws.DP16[0], xH, T); o.p[GRUB_D1_16] = rev(ws.DQ16[0], xH, T); o.p[GRUB_W0] = ws.pT[0]; o.p[GRUB_W1] = ws.qT[0];
      o.p[GRUB_G_IN] = rev(ws.GB, sR, T); o.p[GRUB_RG] = last(rs.RG, sR); o.p[GRUB_UG] = last(rs.UG, sR); o.p[GRUB_NG] = last(rs.NG, sR);
      o.p[GRUB_GH] = last(rs.GHb, s3R); o.p[GRUB_HPREV] = last(decin + H, sD); o.p[GRUB_DD] = dec ? Ptr() : last(d_decin + H, sD); o.p[GRUB_DGI] = last(ws.DGI, s3R);
      o.p[GRUB_DGI16] = last(ws.DGI16, x3R); o.p[GRUB_DGH] = last(ws.DGH, s3R); o.p[GRUB_DGH16] = last(ws.DGH16, x3R); o.p[GRUB_GA] = last(ws.GA, sR);
      o.p[GRUB_G_OUT] = d_h0 ? d_h0 : ws.G; o.ld[GRUB_LD_H] = ldd; o.ld[LD_OUT] = 3 * R; o.n16[N16_OUT] = 3 * ctR; o.i[GRUB_I_R] = R; o.i[GRUB_I_GEMM_FROM] = 1;
      o.i[GRUB_I_GATES_TO] = T; o.i[GRUB_I_GIN_FROM] = 1;
      add_desc(bld, K_GRUB, ctR, dl.grub.wg0, dl.grub.nwg, H, 0, 0, T + 1, o);
    }
    // Bb: dphi through the GRU input projection (+ the decoder's gradient, through phi's ReLU) | GB[t] = GA[t] + DGH[t] W_hh
    // The K = 3R product is the fattest link of the step (96 KB of operands per tile): when a third range of workgroups is free it
    // runs as three K = R links side by side (the r | u | n thirds of DGI and of W_ih^T), each writing a full slab of partial sums
    // (the derivative mask distributes over the sum; the decoder's gradient joins the first), and B3 adds the three slabs up as it
    // loads them.
    const bool split3 = dl.split3;
    Operands o;  // (ld[LIN_LD_A], i[LIN_I_W_WIDTH] of a part: widths of the slab / of the packed rows the K-range is taken from)
    o.p[LIN_GATE] = last(decin, sD); o.ld[LIN_LD_ADD] = ldd; o.ld[LIN_LD_GATE] = ldd; o.ld[LD_OUT] = H; o.n16[N16_OUT] = ctH;
    if (split3) {
      const size_t wthird = (size_t)ctR * 256 / (bld.p.ot != OP_F32 ? 2 : 1);  // the packed weight's k-chunks [ctR * part, ...) (16-bit packs: half the floats)
      float* const orm[3] = {ws.DPHI[3], ws.DPHI3b, ws.DPHI3c};
      float* const o16[3] = {ws.DPHI16[3], ws.DPHI16b, ws.DPHI16c};
      o.ld[LIN_LD_A] = 3 * R; o.i[LIN_I_W_WIDTH] = 3 * R;
      for (int part = 0; part < 3; ++part) {
        // (the decoder's gradient: from outside the launch it joins the first partial sum; from the leader, which runs on the third
        // part's range, the third — polled, stored kBdecAhead steps earlier)
        o.p[LIN_A] = last(ws.DGI16 + (size_t)part * ctR * 256, x3R); o.p[LIN_W] = ws.wihT + part * wthird;
        o.p[LIN_ADD] = dec ? (part == 2 ? last(ws.DD, sD) : Ptr()) : (part == 0 ? last(d_decin, sD) : Ptr());
        o.p[LIN_ORM] = last(orm[part], sH); o.p[LIN_O16] = last(o16[part], xH);
        add_desc(bld, K_LIN, ctH, dl.part[part].wg0, dl.part[part].nwg, R, dec && part == 2 ? DF_ADD_POLLED | DF_ADD_EARLY : 0, 0, T, o);
      }
    } else {
      o.p[LIN_A] = last(ws.DGI16, x3R); o.p[LIN_W] = ws.wihT; o.p[LIN_ADD] = last(d_decin, sD); o.p[LIN_ORM] = last(ws.DPHI[3], sH);
      o.p[LIN_O16] = last(ws.DPHI16[3], xH);
      add_desc(bld, K_LIN, ctH, dl.dphi.wg0, dl.dphi.nwg, 3 * R, 0, 0, T, o);
    }
    Operands gb;
    gb.p[LIN_A] = last(ws.DGH16, x3R); gb.p[LIN_W] = ws.whhT; gb.p[LIN_ADD] = last(ws.GA, sR); gb.ld[LIN_LD_ADD] = R; gb.p[LIN_ORM] = last(ws.GB, sR); gb.ld[LD_OUT] = R;
    if (dec) { gb.p[LIN_ADD2] = last(ws.DD + H, sD); gb.i[LIN_I_LD_ADD2] = ldd; }  // GB = GA + (the decoder's gradient wrt h) + DGH W_hh, GA = g u
    add_desc(bld, K_LIN, ctR, dl.gb.wg0, dl.gb.nwg, 3 * R,
             DF_ADD_POLLED | DF_RM_SC1 | DF_GENTLE | ((pchain_tune() & 16) ? DF_CANARY : 0) | (dec ? DF_ADD2_POLLED : 0), 0, T, gb);
    // B3..B5: back through phi_z layers 3, 2, 1: runs of backward links (K_LINSEQ), D_{i+1} = (D_i W_i) masked by the saved activation
    auto blink = [&](const float* W, const float* gate, float* orm, float* o16) { return rev_link(W, gate, orm, o16, T - 1, sH, H, xH); };
    const SeqLink lf[3] = {blink(ws.fT[3], rs.FZ[2], ws.DPHI[2], ws.DPHI16[2]), blink(ws.fT[2], rs.FZ[1], ws.DPHI[1], ws.DPHI16[1]),
                           blink(ws.fT[1], rs.FZ[0], ws.DPHI[0], ws.DPHI16[0])};
    if (split3) {  // the link that adds the three partial-sum slabs up is a K_LIN of its own (a run's links are plain), the other two a run
      Operands o3;
      o3.p[LIN_A] = last(ws.DPHI16[3], xH); o3.p[LIN_W] = ws.fT[3]; o3.p[LIN_GATE] = last(rs.FZ[2], sH); o3.ld[LIN_LD_GATE] = H; o3.p[LIN_ORM] = last(ws.DPHI[2], sH);
      o3.ld[LD_OUT] = H; o3.p[LIN_O16] = last(ws.DPHI16[2], xH); o3.n16[N16_OUT] = ctH; o3.p[LIN_A2] = last(ws.DPHI16b, xH); o3.p[LIN_A3] = last(ws.DPHI16c, xH);
      add_desc(bld, K_LIN, ctH, dl.wide_h.wg0, dl.wide_h.nwg, H, DF_A_SUM3, 0, T, o3);
    }
    add_linseq(bld, ctH, dl.wide_h.wg0, dl.wide_h.nwg, H, false, true, 0, T, last(ws.DPHI16[split3 ? 2 : 3], xH), split3 ? 2 : 3, lf + (split3 ? 1 : 0), -sH,
               -xH, ctH, 0.f, H);
    {  // B6: dz and the heads
      Operands z;
      z.p[DZ_D16] = last(ws.DPHI16[0], xH); z.p[DZ_WT] = ws.fT[0]; z.p[DZ_MU_Q] = last(mu_q, sZ); z.p[DZ_SD_Q] = last(sd_q, sZ); z.p[DZ_MU_P] = last(mu_p, sZ);
      z.p[DZ_SD_P] = last(sd_p, sZ); z.p[DZ_EPS] = last(eps, sZ); z.p[DZ_RAW_Q] = last(rs.RAWQ, sZ); z.p[DZ_RAW_P] = last(rs.RAWP, sZ); z.p[DZ_X_SL] = x_sl;
      z.p[DZ_C_RAW] = c_raw; z.p[DZ_C_FN] = c_fn; z.p[DZ_DQH] = last(ws.DQH, s2Z); z.p[DZ_DQH16] = last(ws.DQH16, x2Z); z.p[DZ_DPH] = last(ws.DPH, s2Z);
      z.p[DZ_DPH16] = last(ws.DPH16, x2Z); z.ld[LD_OUT] = 2 * Z; z.n16[N16_OUT] = 2 * ctZ; z.i[DZ_I_Z] = Z; z.i[DZ_I_RESIDUAL] = residual_posterior;
      z.i[DZ_I_STRIDE] = stride; z.i[DZ_I_T0] = T - 1; z.f[DZ_F_FN_FLOOR] = fn_floor; z.f[DZ_F_BETA] = beta; z.f[DZ_F_SD_EPS] = sd_eps;
      add_desc(bld, K_DZ, ctZ, dl.dz.wg0, dl.dz.nwg, H, 0, 0, T, z);
    }
    // B7: heads -> last hidden layers;  B8, B9: hidden layers 2, 1  (prior | posterior).  B7 .. B9 of a chain: one visit (the heads'
    // gradient link, K = 2Z, joins the run's descriptor visit)
    {
      const SeqLink lp[3] = {blink(ws.phT, rs.P[2], ws.DP[2], ws.DP16[2]), blink(ws.pT[2], rs.P[1], ws.DP[1], ws.DP16[1]), blink(ws.pT[1], rs.P[0], ws.DP[0], ws.DP16[0])};
      const SeqLink lq[3] = {blink(ws.qhT, rs.Q[2], ws.DQ[2], ws.DQ16[2]), blink(ws.qT[2], rs.Q[1], ws.DQ[1], ws.DQ16[1]), blink(ws.qT[1], rs.Q[0], ws.DQ[0], ws.DQ16[0])};
      add_linseq(bld, ctH, dl.prior.wg0, dl.prior.nwg, H, false, true, 0, T, last(ws.DPH16, x2Z), 3, lp, -sH, -xH, ctH, 0.f, H, 2 * Z);
      add_linseq(bld, ctH, dl.post.wg0, dl.post.nwg, H, false, true, 0, T, last(ws.DQH16, x2Z), 3, lq, -sH, -xH, ctH, 0.f, H, 2 * Z);
    }
    if (dec) {
      // the decoder leader (vrnn_static.h): walk step s runs the decoder's data gradients of walk step s + kBdecAhead — the pointers
      // start there and the links end kBdecAhead steps early; the first kBdecAhead walk steps' rows come from K6 in front of the launch
      const int L = kBdecAhead, SF = dec->SF;
      const long sF = (long)B * SF;
      auto lead = [&](const float* base, long step) { return rev(base, step, T - 1 - L); };
      Operands b0, b1, b2;
      b0.p[LIN_A] = lead(dec->dz3, sF); b0.ld[LIN_LD_A] = SF; b0.p[LIN_W] = ws.dT[2]; b0.p[LIN_GATE] = lead(dec->y2, sH); b0.ld[LIN_LD_GATE] = H;
      b0.p[LIN_ORM] = lead(dec->dy2, sH); b0.ld[LD_OUT] = H; b0.p[LIN_O16] = lead(ws.DY216, xH); b0.n16[N16_OUT] = ctH; b0.f[LIN_F_SLOPE] = dec->slope;
      add_desc(bld, K_LIN, ctH, dl.bdec[0].wg0, dl.bdec[0].nwg, SF, DF_A_PLAIN | DF_GENTLE, 0, T - L, b0);
      b1.p[LIN_A] = lead(ws.DY216, xH); b1.p[LIN_W] = ws.dT[1]; b1.p[LIN_GATE] = lead(dec->y1, sH); b1.ld[LIN_LD_GATE] = H;
      b1.p[LIN_ORM] = lead(dec->dy1, sH); b1.ld[LD_OUT] = H; b1.p[LIN_O16] = lead(ws.DY116, xH); b1.n16[N16_OUT] = ctH; b1.f[LIN_F_SLOPE] = dec->slope;
      add_desc(bld, K_LIN, ctH, dl.bdec[1].wg0, dl.bdec[1].nwg, H, DF_GENTLE | DF_CANARY, 0, T - L, b1);
      b2.p[LIN_A] = lead(ws.DY116, xH); b2.p[LIN_W] = ws.dT[0]; b2.p[LIN_ORM] = lead(ws.DD, sD); b2.ld[LD_OUT] = ldd;
      add_desc(bld, K_LIN, (H + R) / 16, dl.bdec[2].wg0, dl.bdec[2].nwg, H, DF_RM_SC1 | DF_GENTLE | DF_CANARY, 0, T - L, b2);
    }
    if (encf) {
      // the d_enc follower (vrnn_static.h): walk step s computes the rows of the time step of walk step s - kBencLag, whose DQ0 the
      // posterior run published at the end of that step — the pointers start a slab back, the links begin a step late and use the
      // walk's last step.  EP: the K = 3R product, polled by the K = H link of the same tile on the same workgroup.
      const long sX = (long)B * X;
      auto lag = [&](const float* base, long step) { return rev(base, step, T - 1 + kBencLag); };
      Operands e0, e1;
      e0.p[LIN_A] = lag(ws.DGI16, x3R); e0.p[LIN_W] = ws.wixT; e0.p[LIN_ORM] = lag(ws.EP, sX); e0.ld[LD_OUT] = X;
      add_desc(bld, K_LIN, X / 16, dl.benc[0].wg0, dl.benc[0].nwg, 3 * R, DF_RM_SC1 | DF_GENTLE | DF_CANARY, kBencLag, T + 1, e0);
      e1.p[LIN_A] = lag(ws.DQ16[0], xH); e1.p[LIN_W] = ws.qxT; e1.p[LIN_ADD] = lag(ws.EP, sX); e1.ld[LIN_LD_ADD] = X;
      e1.p[LIN_ORM] = lag(d_enc, sX); e1.ld[LD_OUT] = X;
      add_desc(bld, K_LIN, X / 16, dl.benc[1].wg0, dl.benc[1].nwg, H, DF_ADD_POLLED | DF_GENTLE | DF_CANARY, kBencLag, T + 1, e1);
    }
    // what the launch polls gets sentinels: GA, GB (single words) and the T16 copies, from the host or slab by slab from the walk
    // (vrnn_static.h ArmPlan; the table's walk step j is time step T' - 1 - j)
    ArmPlan plan;
    plan.fill(ws.GA, ws.x16_bytes);
    if (encf) plan.fill(ws.EP, sizeof(float) * n * X);
    if (!groups) {
      plan.add(arm_rm(ws.GA, R, B, T, true)); plan.add(arm_rm(ws.GB, R, B, T, true));
      for (int i = 0; i < 3; ++i) { plan.add(arm_t16(ws.DP16[i], H, rt, T, true)); plan.add(arm_t16(ws.DQ16[i], H, rt, T, true)); }
      plan.add(arm_t16(ws.DGI16, 3 * R, rt, T, true)); plan.add(arm_t16(ws.DGH16, 3 * R, rt, T, true));
      for (int i = 0; i < 4; ++i) plan.add(arm_t16(ws.DPHI16[i], H, rt, T, true));
      plan.add(arm_t16(ws.DPH16, 2 * Z, rt, T, true)); plan.add(arm_t16(ws.DQH16, 2 * Z, rt, T, true));
      plan.add(arm_t16(ws.DPHI16b, H, rt, T, true)); plan.add(arm_t16(ws.DPHI16c, H, rt, T, true));
      if (dec) { plan.add(arm_t16(ws.DY216, H, rt, T, true)); plan.add(arm_t16(ws.DY116, H, rt, T, true)); plan.add(arm_rm(ws.DD, ldd, B, T, true)); }
      if (encf) plan.add(arm_rm(ws.EP, X, B, T, true));  // (the slab of the table's walk step j is stored at walk step j + kBencLag)
    }
    // the leader's first rows (time steps T' - kBdecAhead .. T' - 1) as K6 products, behind the fill: the walk polls their DD slabs
    auto lead_rows = [&]() -> int {
      if (!dec) return BLVM_OK;
      const int L = kBdecAhead, M = L * B, SF = dec->SF;
      const size_t r0 = (size_t)(T - L) * B;
      BLVM_TRY(gemm_f32(0, 1, M, H, SF, dec->dz3 + r0 * SF, SF, dec->w[2], H, dec->dy2 + r0 * H, H, nullptr, 0, dec->slope, dec->y2 + r0 * H, H, 0, 1, s));
      BLVM_TRY(gemm_f32(0, 1, M, H, H, dec->dy2 + r0 * H, H, dec->w[1], H, dec->dy1 + r0 * H, H, nullptr, 0, dec->slope, dec->y1 + r0 * H, H, 0, 1, s));
      return gemm_f32(0, 1, M, H + R, H, dec->dy1 + r0 * H, H, dec->w[0], H + R, ws.DD + r0 * ldd, ldd, nullptr, 0, 0.f, nullptr, 0, 0, 1, s);
    };
    BLVM_TRY(vrnn_launch(bld, false, "vrnn_bwd", s, plan, lead_rows));
    if (dec) ++g_dec_bwd_folded;
    if (encf) ++g_enc_bwd_folded;
    if (split3) {  // DPHI[3] += the two other partial sums
      const size_t n4 = n * H / 4;
      hipLaunchKernelGGL(add3_kernel, dim3((unsigned)std::min<size_t>((n4 + 255) / 256, 2048)), dim3(256), 0, s, reinterpret_cast<float4*>(ws.DPHI[3]),
                         reinterpret_cast<const float4*>(ws.DPHI3b), reinterpret_cast<const float4*>(ws.DPHI3c), n4);
    }
    return batched();
  }

  BLVM_REQUIRE(!dec, "vrnn_bwd: the decoder leader needs the persistent path");
  count_vrnn(VRNN_BWD_PER_LINK);
  launch_dh(-1, Tp - 1);  // G(T') = 0: gate derivatives of the last step, G <- d_decin h-part of row T'-1
  for (int t = Tp - 1; t >= 0; --t) {
    const size_t oH = (size_t)t * B * H, oZ = (size_t)t * B * Z, o3R = (size_t)t * B * 3 * R, o2Z = (size_t)t * B * 2 * Z;
    const float* dec_t = decin + (size_t)t * B * ldd;
    const float* ddec_t = d_decin + (size_t)t * B * ldd;
    LinLaunch a;
    a.B = B;
    // B2: dphi (through ReLU of phi, plus the decoder's gradient) | G += DGH Whh
    a.nseg = 2;
    a.seg[0] = seg(ws.DGI + o3R, 3 * R, ws.wihT, 3 * R, nullptr, ddec_t, ldd, dec_t, ldd, ws.DPHI[3] + oH, H, H, 3 * R, 0);
    a.seg[1] = seg(ws.DGH + o3R, 3 * R, ws.whhT, 3 * R, nullptr, ws.G, R, nullptr, 0, ws.G, R, R, 3 * R, 0);
    count_lin(launch_lin(a, s));
    // B3..B5: back through phi_z layers 3,2,1
    a.nseg = 1;
    for (int l = 3; l >= 1; --l) {
      a.seg[0] = seg(ws.DPHI[l] + oH, H, ws.fT[l], H, nullptr, nullptr, 0, rs.FZ[l - 1] + oH, H, ws.DPHI[l - 1] + oH, H, H, H, 0);
      count_lin(launch_lin(a, s));
    }
    // B6: dz and the heads
    DzArgs d;
    d.D = ws.DPHI[0] + oH; d.WT = ws.fT[0]; d.D2 = nullptr; d.WT2 = nullptr; d.dz_add = nullptr; d.ld_add = 0; d.has_gemm = 1;
    d.mu_q = mu_q + oZ; d.sd_q = sd_q + oZ; d.mu_p = mu_p + oZ; d.sd_p = sd_p + oZ; d.eps = eps + oZ;
    d.raw_q = rs.RAWQ + oZ; d.raw_p = rs.RAWP + oZ;
    d.x_sl = x_sl; d.c_raw = c_raw; d.c_fn = c_fn;
    d.dqh = ws.DQH + o2Z; d.dph = ws.DPH + o2Z;
    d.B = B; d.H = H; d.Z = Z; d.residual = residual_posterior; d.t = t; d.stride = stride;
    d.fn_floor = fn_floor; d.beta = beta; d.sd_eps = sd_eps; d.muq_raw = nullptr;
    launch_dz(d, pick_nw(H, 1), dim3(Z / 16, rt), s);
    // B7: heads -> last hidden layers
    a.nseg = 2;
    a.seg[0] = seg(ws.DPH + o2Z, 2 * Z, ws.phT, 2 * Z, nullptr, nullptr, 0, rs.P[2] + oH, H, ws.DP[2] + oH, H, H, 2 * Z, 0);
    a.seg[1] = seg(ws.DQH + o2Z, 2 * Z, ws.qhT, 2 * Z, nullptr, nullptr, 0, rs.Q[2] + oH, H, ws.DQ[2] + oH, H, H, 2 * Z, 0);
    count_lin(launch_lin(a, s));
    // B8, B9
    for (int l = 2; l >= 1; --l) {
      a.seg[0] = seg(ws.DP[l] + oH, H, ws.pT[l], H, nullptr, nullptr, 0, rs.P[l - 1] + oH, H, ws.DP[l - 1] + oH, H, H, H, 0);
      a.seg[1] = seg(ws.DQ[l] + oH, H, ws.qT[l], H, nullptr, nullptr, 0, rs.Q[l - 1] + oH, H, ws.DQ[l - 1] + oH, H, H, H, 0);
      count_lin(launch_lin(a, s));
    }
    // B10 (+ gate derivatives of step t-1)
    launch_dh(t, t - 1);
  }
  BLVM_CHECK_LAUNCH("vrnn_seq_bwd");
  if (d_h0) BLVM_HIP(hipMemcpyAsync(d_h0, ws.G, sizeof(float) * (size_t)B * R, hipMemcpyDeviceToDevice, s));

  return batched();
}

extern "C" int blvm_vrnn_seq_bwd(const BlvmVrnnWeights* w, const float* enc, const float* eps, const float* decin,
                                 const float* mu_q, const float* sd_q, const float* mu_p, const float* sd_p,
                                 const float* z, const float* reserve, const float* d_decin, const int32_t* x_sl,
                                 const float* c_raw, const float* c_fn, int stride, float fn_floor, int Tp, int B, int X, int H, int Z,
                                 int R, int residual_posterior, float sd_eps, float* d_enc, float* d_h0,
                                 const BlvmVrnnGrads* gr, float* workspace, void* stream_) {
  return vrnn_seq_bwd_impl(w, enc, eps, decin, mu_q, sd_q, mu_p, sd_p, z, reserve, d_decin, x_sl, c_raw, c_fn, stride, fn_floor, Tp, B, X,
                           H, Z, R, residual_posterior, sd_eps, d_enc, d_h0, gr, workspace, static_cast<hipStream_t>(stream_));
}

extern "C" int blvm_vrnn_seq_bwd_dec(const BlvmVrnnWeights* w, const float* enc, const float* eps, const float* decin,
                                     const float* mu_q, const float* sd_q, const float* mu_p, const float* sd_p, const float* z,
                                     const float* reserve, const int32_t* x_sl, const float* c_raw, const float* c_fn, int stride,
                                     float fn_floor, int Tp, int B, int X, int H, int Z, int R, int residual_posterior, float sd_eps,
                                     float* d_enc, float* d_h0, const BlvmVrnnGrads* gr, float* workspace, const float* dz3,
                                     const float* dec_y1, const float* dec_y2, const float* const* dec_w, float* dy2, float* dy1, int DH,
                                     int SF, float slope, int* folded, void* stream_) {
  BLVM_REQUIRE(folded != nullptr, "vrnn_bwd_dec: null pointer");
  *folded = 0;
  BLVM_TRY(check_dims(Tp, B, X, H, Z, R));
  if (!vrnn_dec_bwd_folds(Tp, B, H, Z, R, DH, SF)) return BLVM_OK;  // nothing done: the caller takes blvm_vrnn_seq_bwd's path
  BLVM_REQUIRE(dz3 && dec_y1 && dec_y2 && dec_w && dec_w[0] && dec_w[1] && dec_w[2] && dy2 && dy1, "vrnn_bwd_dec: null pointer");
  BLVM_REQUIRE(aligned16(dz3) && aligned16(dy2) && aligned16(dy1), "vrnn_bwd_dec: buffers must be 16-byte aligned");
  const VrnnDecBwd dec{dz3, dec_y1, dec_y2, {dec_w[0], dec_w[1], dec_w[2]}, dy2, dy1, DH, SF, slope};
  BLVM_TRY(vrnn_seq_bwd_impl(w, enc, eps, decin, mu_q, sd_q, mu_p, sd_p, z, reserve, nullptr, x_sl, c_raw, c_fn, stride, fn_floor, Tp, B, X,
                             H, Z, R, residual_posterior, sd_eps, d_enc, d_h0, gr, workspace, static_cast<hipStream_t>(stream_), &dec));
  *folded = 1;
  return BLVM_OK;
}
