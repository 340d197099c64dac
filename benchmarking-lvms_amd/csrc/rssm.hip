// rssm.hip — K5: the recurrent state-space cell of the Clockwork-VAE over a whole sequence, forward + BPTT.
//
// Replaces the per-level time loop `clockwork_vae.py:272-281` over the scripted `RSSMCell.forward`
// (blvm/modules/rssm.py:79-104):
//   g = ReLU(Linear(cat[z_{t-1}, context_t]));  h_t = GRUCell(g, h_{t-1})
//   posterior = MLP(cat[h_t, enc_t]) -> (mu_q, sd_q);  prior = MLP(h_t) -> (mu_p, sd_p)
//   residual / precision-weighted combination (variational.py:125-138);  z_t = rsample
// Six dependent links per step in each direction (stages.h kernels + the two GRU links below); the context / encoding
// halves of the concatenated-input layers, every weight gradient and d(context), d(enc) are batched MFMA GEMMs
// outside the loop.  Same design and numerics as vrnn.hip.
#include <atomic>

#include "common.h"
#include "pchain.h"

namespace blvm {
namespace {

#include "stages.h"

// ---- GRU link: gi = A Wih^T + bih (3 gate tiles) ; gates with the precomputed hidden projection ; state update ------
struct GruCellArgs {
  const float* A;      int lda;   // [B,K] GRU input
  const float* Wih;    int ldw;   // [3H,K] in T16 (ldw = K)
  const float* bih;               // [3H]
  const float* gh;                // [B,3H] hidden projection incl. b_hh
  const float* hprev;  int ldh;   // [B,H]
  float* hnext;        int ldn;   // [B,H]
  float *rg, *ug, *ng;            // [B,H]
  int B, H, K;
};

template <int NW>
__global__ __launch_bounds__(NW * 64) void gru_cell_stage_kernel(const float* A, const float* Wih, const float* bih,
                                                                 const float* gh, const float* hprev, unsigned lda_ldh,
                                                                 unsigned b_h, int K, float* hnext, int ldn, float* rg, float* ug,
                                                                 float* ng) {
  // scalar arguments (GruCellArgs documents them; ldw = K for a T16 weight): 5 input pointers, lda:16|ldh:16, B:16|H:16 and K are
  // the first 13 dwords, preloaded into SGPRs (stages.h, launch-latency note 4)
  const int lda = lda_ldh & 0xffff, ldh = lda_ldh >> 16, B = b_h & 0xffff, H0 = b_h >> 16, ldw = K;
  __shared__ float red[3 * NW * 256];
  const int r0 = blockIdx.y * 16, c0 = blockIdx.x * 16, wave = threadIdx.x >> 6, H = H0;
  const int t = threadIdx.x & 255;
  const int row = r0 + (t >> 4), col = c0 + (t & 15);
  const bool own = threadIdx.x < 256 && row < B;
  const int rowc = row < B ? row : r0;
  const size_t o3 = (size_t)rowc * 3 * H + col;
  const float b0 = bih[col], b1 = bih[H + col], b2 = bih[2 * H + col];
  const float hr = gh[o3], hz = gh[o3 + H], hn = gh[o3 + 2 * H];
  const float hp = hprev[(size_t)rowc * ldh + col];
  f32x4 acc[3];
#pragma unroll
  for (int g = 0; g < 3; ++g) acc[g] = (f32x4){0.f, 0.f, 0.f, 0.f};
  {
    const float* const As[3] = {A, A, A};
    const float* const Ws[3] = {Wih, Wih, Wih};
    const int la[3] = {lda, lda, lda}, lw[3] = {ldw, ldw, ldw}, cs[3] = {c0, H + c0, 2 * H + c0};
    wave_gemm16_multi<NW, 3, true>(As, la, r0, B, Ws, lw, cs, K, wave, acc);
  }
  float v[3];
  reduce_tiles<3, NW>(acc, red, v);
  if (!own) return;
  const float r = sigmoidf_(v[0] + b0 + hr);
  const float u = sigmoidf_(v[1] + b1 + hz);
  const float n = tanhf(v[2] + b2 + r * hn);
  hnext[(size_t)row * ldn + col] = (1.f - u) * n + u * hp;
  const size_t o = (size_t)row * H + col;
  rg[o] = r; ug[o] = u; ng[o] = n;
}

// ---- backward GRU link: complete dL/dh_t, then the gate derivatives of step t -------------------------------------------
struct RssmDhArgs {
  const float *DQ0, *DP0;   // [B,H] grads wrt the first posterior / prior layer pre-activations of step t
  const float *WqT, *WpT;   // [H,H] h-part of post_w0 / prior_w0, transposed, in T16
  const float* dh_add;      // [B,H] direct gradient wrt h_t (from the level below / the decoder) or null
  float* G;                 // [B,H] running gradient wrt h (in: from step t+1; out: towards step t-1 through the u gate)
  const float *rg, *ug, *ng, *gh;  // step t saves; gh [B,3H]
  const float* hprev;       // [B,H] h_{t-1}
  float *dgi, *dgh;         // [B,3H]
  int B, H;
};

template <int NW>
__global__ __launch_bounds__(NW * 64) void rssm_dh_stage_kernel(const float* DQ0, const float* DP0, const float* WqT,
                                                                const float* WpT, float* G, unsigned b_h, RssmDhArgs a) {
  // leading scalars preloaded into SGPRs, the struct by s_load, the saves prefetched in the `mid` hook (stages.h head_stage_kernel)
  __shared__ float red[2 * NW * 256];
  const int B = b_h & 0xffff, H = b_h >> 16;
  const int r0 = blockIdx.y * 16, c0 = blockIdx.x * 16, wave = threadIdx.x >> 6;
  const int t = threadIdx.x & 255;
  const int row = r0 + (t >> 4), col = c0 + (t & 15);
  const bool own = threadIdx.x < 256 && row < B;
  const int rowc = row < B ? row : r0;
  const size_t o = (size_t)rowc * H + col, o3 = (size_t)rowc * 3 * H + col;
  const float gG = G[o];
  float gadd = 0.f, r = 0.f, u = 0.f, n = 0.f, hn = 0.f, hp = 0.f;
  auto prefetch = [&]() {
    gadd = a.dh_add != nullptr ? a.dh_add[o] : 0.f;
    r = a.rg[o]; u = a.ug[o]; n = a.ng[o]; hn = a.gh[o3 + 2 * H]; hp = a.hprev[o];
  };
  f32x4 acc[2];
  acc[0] = (f32x4){0.f, 0.f, 0.f, 0.f};
  acc[1] = (f32x4){0.f, 0.f, 0.f, 0.f};
  {
    const float* const As[2] = {DQ0, DP0};
    const float* const Ws[2] = {WqT, WpT};
    const int ld[2] = {H, H}, cs[2] = {c0, c0};
    wave_gemm16_multi<NW, 2, false>(As, ld, r0, B, Ws, ld, cs, H, wave, acc, prefetch);
  }
  float v[2];
  reduce_tiles<2, NW>(acc, red, v);
  if (!own) return;
  const float g0 = gG + gadd;
  const float g = g0 + v[0] + v[1];
  const float dn_pre = g * (1.f - u) * (1.f - n * n);
  const float du_pre = g * (hp - n) * u * (1.f - u);
  const float dr_pre = dn_pre * hn * r * (1.f - r);
  a.dgi[o3] = dr_pre; a.dgi[o3 + H] = du_pre; a.dgi[o3 + 2 * H] = dn_pre;
  a.dgh[o3] = dr_pre; a.dgh[o3 + H] = du_pre; a.dgh[o3 + 2 * H] = dn_pre * r;
  G[o] = g * u;
}

struct RssmReserve {
  float *GIN, *GHb, *RG, *UG, *NG, *Q[3], *P[3], *RAWQ, *RAWP, *MUQR, *XGIN, *XQ;
  float *Wgz, *Wih, *Whh, *Wq[3], *Wp[3], *Wqh, *Wph;  // T16 copies of the weights the forward chain multiplies by
  // persistent forward (B <= kPchainCarveMaxB): T16 copies of every activation a link multiplies, per step [rt*16, width]
  float *Z16, *H16, *GIN16, *Q16[3], *P16[3];
  size_t x16_bytes;  // from the first piece a launch polls to the end of the T16 copies: sentinel-filled in one go
};
size_t carve_rssm(float* base, int T, int B, int H, int Z, RssmReserve* r) {
  const size_t n = (size_t)T * B;
  Arena ar{base};
  RssmReserve t;
  t.GIN = ar.take(n * H); t.GHb = ar.take(n * 3 * H);
  t.RG = ar.take(n * H); t.UG = ar.take(n * H); t.NG = ar.take(n * H);
  for (int i = 0; i < 3; ++i) t.Q[i] = ar.take(n * H);
  for (int i = 0; i < 3; ++i) t.P[i] = ar.take(n * H);
  t.RAWQ = ar.take(n * Z); t.RAWP = ar.take(n * Z); t.MUQR = ar.take(n * Z);
  t.XGIN = ar.take(n * H); t.XQ = ar.take(n * H);
  t.Wgz = ar.take((size_t)H * Z); t.Wih = ar.take((size_t)3 * H * H); t.Whh = ar.take((size_t)3 * H * H);
  for (int i = 0; i < 3; ++i) { t.Wq[i] = ar.take((size_t)H * H); t.Wp[i] = ar.take((size_t)H * H); }
  t.Wqh = ar.take((size_t)2 * Z * H); t.Wph = ar.take((size_t)2 * Z * H);
  t.Z16 = nullptr;
  if (B <= kPchainCarveMaxB) {
    const size_t rows = (size_t)((B + 15) / 16) * 16, m = (size_t)T * rows;
    t.Z16 = ar.take((m + rows) * Z); t.H16 = ar.take((m + rows) * H); t.GIN16 = ar.take(m * H);
    for (int i = 0; i < 3; ++i) { t.Q16[i] = ar.take(m * H); t.P16[i] = ar.take(m * H); }
    t.x16_bytes = ar.bytes_from(t.Z16);
  }
  if (r) *r = t;
  return ar.floats();
}

struct RssmWs {
  float *gzT, *wihT, *whhT, *qT[3], *pT[3], *qhT, *phT, *DGIN, *DGI, *DGH, *DQH, *DPH, *DQ[3], *DP[3], *G;
  // persistent backward (B <= kPchainCarveMaxB): the running state gradient as per-step slabs [T,B,H] and T16 copies of every
  // gradient a link multiplies, per step [rt*16, width]
  float *GA, *GB, *DGIN16, *DGI16, *DGH16, *DQH16, *DPH16, *DQ16[3], *DP16[3];
  size_t x16_bytes;  // from the first piece a launch polls to the end of the T16 copies: sentinel-filled in one go
};
size_t carve_rssm_ws(float* base, int T, int B, int H, int Z, RssmWs* w) {
  const size_t n = (size_t)T * B;
  Arena ar{base};
  RssmWs t;
  t.gzT = ar.take((size_t)Z * H); t.wihT = ar.take((size_t)H * 3 * H); t.whhT = ar.take((size_t)H * 3 * H);
  for (int i = 0; i < 3; ++i) { t.qT[i] = ar.take((size_t)H * H); t.pT[i] = ar.take((size_t)H * H); }
  t.qhT = ar.take((size_t)H * 2 * Z); t.phT = ar.take((size_t)H * 2 * Z);
  t.DGIN = ar.take(n * H); t.DGI = ar.take(n * 3 * H); t.DGH = ar.take(n * 3 * H);
  t.DQH = ar.take(n * 2 * Z); t.DPH = ar.take(n * 2 * Z);
  for (int i = 0; i < 3; ++i) { t.DQ[i] = ar.take(n * H); t.DP[i] = ar.take(n * H); }
  t.G = ar.take((size_t)B * H);
  t.GA = nullptr;
  if (B <= kPchainCarveMaxB) {
    const size_t m = (size_t)T * ((B + 15) / 16) * 16;
    t.GA = ar.take(n * H); t.GB = ar.take(n * H);
    t.DGIN16 = ar.take(m * H); t.DGI16 = ar.take(m * 3 * H); t.DGH16 = ar.take(m * 3 * H);
    t.DQH16 = ar.take(m * 2 * Z); t.DPH16 = ar.take(m * 2 * Z);
    for (int i = 0; i < 3; ++i) { t.DQ16[i] = ar.take(m * H); t.DP16[i] = ar.take(m * H); }
    t.x16_bytes = ar.bytes_from(t.GA);
  }
  if (w) *w = t;
  return ar.floats();
}

// which implementation the sequence entry points took and which tiles their per-link loops ran on (blvm_rssm_path_counts):
// host-side counts, [0..3] one per call, [4..5] one per launch_lin of the launch-per-link loops
enum { RSSM_FWD_PROGRAM = 0, RSSM_FWD_PER_LINK = 1, RSSM_BWD_PROGRAM = 2, RSSM_BWD_PER_LINK = 3, RSSM_LIN16 = 4, RSSM_LIN32 = 5 };
std::atomic<unsigned long long> g_rssm_counts[6];
inline void count_rssm(int k) { g_rssm_counts[k].fetch_add(1, std::memory_order_relaxed); }
inline void count_lin(int tile_width) { count_rssm(tile_width == 32 ? RSSM_LIN32 : RSSM_LIN16); }

int check_rssm(int T, int B, int H, int Z, int C, int E) {
  BLVM_REQUIRE(T > 0 && B > 0, "rssm: bad T=%d B=%d", T, B);
  BLVM_REQUIRE(H > 0 && Z > 0 && H % 16 == 0 && Z % 16 == 0, "rssm: H, Z must be positive multiples of 16 (got %d, %d)", H, Z);
  BLVM_REQUIRE(C >= 0 && E > 0 && C % 4 == 0 && E % 4 == 0, "rssm: context / encoding sizes must be multiples of 4 (got %d, %d)", C, E);
  BLVM_REQUIRE(B < 65536 && H < 65536, "rssm: B and H must be below 65536 (packed kernel arguments)");
  return BLVM_OK;
}

}  // namespace
}  // namespace blvm

using namespace blvm;

extern "C" int blvm_rssm_path_counts(unsigned long long out[6]) {
  BLVM_REQUIRE(out, "rssm_path_counts: null pointer");
  for (int k = 0; k < 6; ++k) out[k] = g_rssm_counts[k].load(std::memory_order_relaxed);
  return BLVM_OK;
}

extern "C" size_t blvm_rssm_reserve_floats(int T, int B, int H, int Z) { return carve_rssm(nullptr, T, B, H, Z, nullptr); }
extern "C" size_t blvm_rssm_bwd_workspace_floats(int T, int B, int H, int Z) { return carve_rssm_ws(nullptr, T, B, H, Z, nullptr); }

extern "C" int blvm_rssm_seq_fwd(const BlvmRssmWeights* w, const float* enc, const float* ctx, const float* z0,
                                 const float* h0, const float* eps, int T, int B, int H, int Z, int C, int E, int mode,
                                 float sd_eps, float* zs, float* hs, float* mu_q, float* sd_q, float* mu_p, float* sd_p,
                                 float* reserve, void* stream_) {
  hipStream_t s = static_cast<hipStream_t>(stream_);
  BLVM_TRY(check_rssm(T, B, H, Z, C, E));
  BLVM_REQUIRE(w && enc && eps && zs && hs && mu_q && sd_q && mu_p && sd_p && reserve, "rssm_fwd: null pointer");
  BLVM_REQUIRE(C == 0 || ctx != nullptr, "rssm_fwd: context missing");
  BLVM_REQUIRE(mode >= 0 && mode <= 3, "rssm_fwd: mode must be 0 (plain), 1 (residual), 2 (precision-weighted) or 3 (generate: z from the prior)");
  BLVM_REQUIRE(aligned16(zs) && aligned16(hs) && aligned16(reserve), "rssm_fwd: buffers must be 16-byte aligned");
  RssmReserve rs;
  carve_rssm(reserve, T, B, H, Z, &rs);
  const size_t n = (size_t)T * B;
  const int ldg = Z + C, ldq = H + E;
  const float beta = softplus_beta_of(sd_eps);
  if (C > 0) {
    BLVM_TRY(gemm_f32(0, 0, (int)n, H, C, ctx, C, w->gin_w + Z, ldg, rs.XGIN, H, w->gin_b, 0, 0.f, nullptr, 0, 0, 1, s));
  }
  BLVM_TRY(gemm_f32(0, 0, (int)n, H, E, enc, E, w->post_w[0] + H, ldq, rs.XQ, H, w->post_b[0], 0, 0.f, nullptr, 0, 0, 1, s));
  // T16 operand copies of the chain's weights (once per sequence): z columns of the GRU input layer, h columns of post_w0
  T16PackScope pack_scope(pchain_optype(B), s);  // 16-bit operand modes: the persistent launch multiplies 16-bit weight packs
  BLVM_TRY(t16_pack_rows(w->gin_w, ldg, H, Z, rs.Wgz, s));
  BLVM_TRY(t16_pack_rows(w->gru_wih, H, 3 * H, H, rs.Wih, s));
  BLVM_TRY(t16_pack_rows(w->gru_whh, H, 3 * H, H, rs.Whh, s));
  BLVM_TRY(t16_pack_rows(w->post_w[0], ldq, H, H, rs.Wq[0], s));
  BLVM_TRY(t16_pack_rows(w->prior_w[0], H, H, H, rs.Wp[0], s));
  for (int k = 1; k < 3; ++k) {
    BLVM_TRY(t16_pack_rows(w->post_w[k], H, H, H, rs.Wq[k], s));
    BLVM_TRY(t16_pack_rows(w->prior_w[k], H, H, H, rs.Wp[k], s));
  }
  BLVM_TRY(t16_pack_rows(w->post_hw, H, 2 * Z, H, rs.Wqh, s));
  BLVM_TRY(t16_pack_rows(w->prior_hw, H, 2 * Z, H, rs.Wph, s));
  BLVM_TRY(pack_scope.flush());  // all packs above in one launch
  BLVM_HIP(copy_or_zero(zs, z0, sizeof(float) * (size_t)B * Z, s));
  BLVM_HIP(copy_or_zero(hs, h0, sizeof(float) * (size_t)B * H, s));
  const int rt = (B + 15) / 16;
  if (pchain_applies(B) && device_cus() >= 32) {
    // Persistent path (pchain.h / pchain.hip): the six links of a step as a program of 10 descriptors, one launch per sequence.
    using namespace pchain;
    count_rssm(RSSM_FWD_PROGRAM);
    const int ctH = H / 16, ctZ = Z / 16, cus = device_cus() & ~7;
    const long sH = (long)B * H, sZ = (long)B * Z, s3H = 3 * sH, xH = (long)rt * 16 * H, xZ = (long)rt * 16 * Z;
    const int r_h = range_for(ctH * rt, cus / 4);              // one H-wide link (or one half of a posterior | prior pair)
    const int r_gh = range_for(3 * ctH * rt, cus - 2 * r_h);   // the hidden projection, beside the GRU input layer
    Builder bld;
    bld.begin(pchain_optype(B), T, B, 4, false, r_h);
    // L1: GRU input layer (z half; the context half is hoisted) | hidden projection of the GRU
    Operands gi, gh;
    gi.p[LIN_A] = {rs.Z16, xZ}; gi.p[LIN_W] = rs.Wgz; gi.p[LIN_BIAS] = C > 0 ? nullptr : w->gin_b; gi.p[LIN_ADD] = {C > 0 ? rs.XGIN : nullptr, sH}; gi.ld[LIN_LD_ADD] = H;
    gi.p[LIN_ORM] = {rs.GIN, sH}; gi.ld[LD_OUT] = H; gi.p[LIN_O16] = {rs.GIN16, xH}; gi.n16[N16_OUT] = ctH;
    add_desc(bld, K_LIN, ctH, 0, r_h, Z, DF_RELU, 0, T, gi);
    gh.p[LIN_A] = {rs.H16, xH}; gh.p[LIN_W] = rs.Whh; gh.p[LIN_BIAS] = w->gru_bhh; gh.ld[LIN_LD_ADD] = H; gh.p[LIN_ORM] = {rs.GHb, s3H}; gh.ld[LD_OUT] = 3 * H;
    gh.n16[N16_OUT] = ctH;
    add_desc(bld, K_LIN, 3 * ctH, r_h, r_gh, H, DF_RM_SC1, 0, T, gh);
    {  // L2: GRU
      Operands o;
      o.p[GRU_X16] = {rs.GIN16, xH}; o.p[GRU_WIH] = rs.Wih; o.p[GRU_GH] = {rs.GHb, s3H}; o.p[GRU_HPREV] = {hs, sH}; o.p[GRU_HRM] = {hs + sH, sH};
      o.p[GRU_H16] = {rs.H16 + xH, xH}; o.p[GRU_RG] = {rs.RG, sH}; o.p[GRU_UG] = {rs.UG, sH}; o.p[GRU_NG] = {rs.NG, sH}; o.p[GRU_BIH] = w->gru_bih;
      o.ld[GRU_LD_HPREV] = H; o.ld[LD_OUT] = H; o.n16[N16_OUT] = ctH; o.i[GRU_I_R] = H;
      add_desc(bld, K_GRU, ctH, 0, r_h, H, 0, 0, T, o);
    }
    {  // L3..L5: posterior | prior MLPs on h_t, one visit per branch and step (the first layer opens the run)
      const SeqLink lq[3] = {{rs.Wq[0], nullptr, rs.Q[0], sH, H, rs.Q16[0]}, {rs.Wq[1], w->post_b[1], rs.Q[1], sH, H, rs.Q16[1]}, {rs.Wq[2], w->post_b[2], rs.Q[2], sH, H, rs.Q16[2]}};
      const SeqLink lp[3] = {{rs.Wp[0], w->prior_b[0], rs.P[0], sH, H, rs.P16[0]}, {rs.Wp[1], w->prior_b[1], rs.P[1], sH, H, rs.P16[1]}, {rs.Wp[2], w->prior_b[2], rs.P[2], sH, H, rs.P16[2]}};
      add_linseq(bld, ctH, 0, r_h, H, true, false, 0, T, {rs.H16 + xH, xH}, 3, lq, 0, xH, ctH, 0.f, 0, 0, {rs.XQ, sH}, H);
      add_linseq(bld, ctH, r_h, r_h, H, true, false, 0, T, {rs.H16 + xH, xH}, 3, lp, 0, xH, ctH, 0.f, 0);
    }
    {  // L6: heads, combination, sample
      Operands o;
      o.p[HEAD_P16] = {rs.P16[2], xH}; o.p[HEAD_Q16] = {rs.Q16[2], xH}; o.p[HEAD_WP] = rs.Wph; o.p[HEAD_BP] = w->prior_hb; o.p[HEAD_WQ] = rs.Wqh;
      o.p[HEAD_BQ] = w->post_hb; o.p[HEAD_EPS] = {eps, sZ}; o.p[HEAD_MU_P] = {mu_p, sZ}; o.p[HEAD_SD_P] = {sd_p, sZ}; o.p[HEAD_MU_Q] = {mu_q, sZ};
      o.p[HEAD_SD_Q] = {sd_q, sZ}; o.p[HEAD_RAW_P] = {rs.RAWP, sZ}; o.p[HEAD_RAW_Q] = {rs.RAWQ, sZ}; o.p[HEAD_MUQ_RAW] = {rs.MUQR, sZ}; o.p[HEAD_Z] = {zs + sZ, sZ};
      o.p[HEAD_Z16] = {rs.Z16 + xZ, xZ}; o.ld[LD_OUT] = Z; o.n16[N16_OUT] = ctZ; o.i[HEAD_I_Z] = Z; o.i[HEAD_I_RESIDUAL] = mode; o.f[HEAD_F_BETA] = beta;
      o.f[HEAD_F_INV_BETA] = 1.f / beta; o.f[HEAD_F_SD_EPS] = sd_eps;
      add_desc(bld, K_HEAD, ctZ, 0, range_for(ctZ * rt, 2 * r_h), H, 0, 0, T, o);
    }
    // sentinel-fill what the launch polls: the T16 copies, the hidden projection, the states h_1 .. h_T (the GRU link polls words)
    BLVM_HIP(pchain_fill_sentinel(rs.Z16, rs.x16_bytes, s));
    BLVM_HIP(pchain_fill_sentinel(rs.GHb, sizeof(float) * n * 3 * H, s));
    BLVM_HIP(pchain_fill_sentinel(hs + sH, sizeof(float) * n * H, s));
    BLVM_TRY(pchain_rows_to_t16(zs, Z, B, Z, rs.Z16, s));
    BLVM_TRY(pchain_rows_to_t16(hs, H, B, H, rs.H16, s));
    return pchain_launch(bld, "rssm_fwd", s);
  }
  count_rssm(RSSM_FWD_PER_LINK);
  for (int t = 0; t < T; ++t) {
    const size_t oH = (size_t)t * B * H, oZ = (size_t)t * B * Z, o3 = (size_t)t * B * 3 * H;
    const float* zprev = zs + oZ;
    const float* hprev = hs + oH;
    float* hnew = hs + oH + (size_t)B * H;
    LinLaunch l;
    l.B = B; l.nseg = 2;
    // L1: GRU input layer (z half; context half hoisted) | hidden projection of the GRU
    l.seg[0] = seg(zprev, Z, rs.Wgz, Z, C > 0 ? nullptr : w->gin_b, C > 0 ? rs.XGIN + oH : nullptr, H, nullptr, 0, rs.GIN + oH, H, H, Z, 1);
    l.seg[1] = seg(hprev, H, rs.Whh, H, w->gru_bhh, nullptr, 0, nullptr, 0, rs.GHb + o3, 3 * H, 3 * H, H, 0);
    count_lin(launch_lin(l, s));
    // L2: GRU
    {
      const int nw = pick_nw(H, 3);
      const dim3 grid(H / 16, rt);
      const float *gin_t = rs.GIN + oH, *gh_t = rs.GHb + o3;
      float *rg_t = rs.RG + oH, *ug_t = rs.UG + oH, *ng_t = rs.NG + oH;
      const unsigned lda_ldh = (unsigned)H | ((unsigned)H << 16), b_h = (unsigned)B | ((unsigned)H << 16);
      LAUNCH_NW(gru_cell_stage_kernel<NW_>, nw, grid, s, gin_t, (const float*)rs.Wih, w->gru_bih, gh_t, hprev, lda_ldh, b_h, H, hnew, H, rg_t, ug_t, ng_t);
    }
    // L3..L5: posterior | prior MLPs on h_t
    l.seg[0] = seg(hnew, H, rs.Wq[0], H, nullptr, rs.XQ + oH, H, nullptr, 0, rs.Q[0] + oH, H, H, H, 1);
    l.seg[1] = seg(hnew, H, rs.Wp[0], H, w->prior_b[0], nullptr, 0, nullptr, 0, rs.P[0] + oH, H, H, H, 1);
    count_lin(launch_lin(l, s));
    for (int k = 1; k < 3; ++k) {
      l.seg[0] = seg(rs.Q[k - 1] + oH, H, rs.Wq[k], H, w->post_b[k], nullptr, 0, nullptr, 0, rs.Q[k] + oH, H, H, H, 1);
      l.seg[1] = seg(rs.P[k - 1] + oH, H, rs.Wp[k], H, w->prior_b[k], nullptr, 0, nullptr, 0, rs.P[k] + oH, H, H, H, 1);
      count_lin(launch_lin(l, s));
    }
    // L6: heads, combination, sample
    HeadArgs h;
    h.P = rs.P[2] + oH; h.Q = rs.Q[2] + oH;
    h.Wp = rs.Wph; h.bp = w->prior_hb; h.Wq = rs.Wqh; h.bq = w->post_hb;
    h.eps = eps + oZ;
    h.mu_p = mu_p + oZ; h.sd_p = sd_p + oZ; h.mu_q = mu_q + oZ; h.sd_q = sd_q + oZ;
    h.z = zs + oZ + (size_t)B * Z;
    h.raw_p = rs.RAWP + oZ; h.raw_q = rs.RAWQ + oZ; h.muq_raw = rs.MUQR + oZ;
    h.B = B; h.H = H; h.Z = Z; h.residual = mode;
    h.beta = beta; h.inv_beta = 1.f / beta; h.sd_eps = sd_eps;
    launch_head(h, pick_nw(H, 4), dim3(Z / 16, rt), s);
  }
  BLVM_CHECK_LAUNCH("rssm_seq_fwd");
  return BLVM_OK;
}

extern "C" int blvm_rssm_seq_bwd(const BlvmRssmWeights* w, const float* enc, const float* ctx, const float* eps,
                                 const float* zs, const float* hs, const float* mu_q, const float* sd_q,
                                 const float* mu_p, const float* sd_p, const float* reserve, const float* d_zs,
                                 const float* d_hs, const int32_t* x_sl, const float* c_raw, const float* c_fn, int stride,
                                 float fn_floor, int T, int B, int H, int Z, int C, int E, int mode, float sd_eps,
                                 float* d_enc, float* d_ctx, float* d_z0, float* d_h0, const BlvmRssmGrads* gr,
                                 float* workspace, void* stream_) {
  hipStream_t s = static_cast<hipStream_t>(stream_);
  BLVM_TRY(check_rssm(T, B, H, Z, C, E));
  BLVM_REQUIRE(w && enc && eps && zs && hs && mu_q && sd_q && mu_p && sd_p && reserve && d_zs && d_hs && gr && workspace,
               "rssm_bwd: null pointer");
  BLVM_REQUIRE((c_fn == nullptr && c_raw == nullptr) || x_sl != nullptr, "rssm_bwd: KL coefficients need x_sl");
  BLVM_REQUIRE(aligned16(workspace) && aligned16(reserve), "rssm_bwd: buffers must be 16-byte aligned");
  RssmReserve rs;
  carve_rssm(const_cast<float*>(reserve), T, B, H, Z, &rs);
  RssmWs ws;
  carve_rssm_ws(workspace, T, B, H, Z, &ws);
  const size_t n = (size_t)T * B, bh = (size_t)B * H, bz = (size_t)B * Z;
  const int ldg = Z + C, ldq = H + E;
  const float beta = softplus_beta_of(sd_eps);
  T16PackScope pack_scope(pchain_optype(B), s);  // 16-bit operand modes: the persistent launch multiplies 16-bit weight packs
  BLVM_TRY(t16_pack_transposed(w->gin_w, ldg, H, Z, ws.gzT, s));
  BLVM_TRY(t16_pack_transposed(w->gru_wih, H, 3 * H, H, ws.wihT, s));
  BLVM_TRY(t16_pack_transposed(w->gru_whh, H, 3 * H, H, ws.whhT, s));
  BLVM_TRY(t16_pack_transposed(w->post_w[0], ldq, H, H, ws.qT[0], s));
  BLVM_TRY(t16_pack_transposed(w->prior_w[0], H, H, H, ws.pT[0], s));
  for (int k = 1; k < 3; ++k) {
    BLVM_TRY(t16_pack_transposed(w->post_w[k], H, H, H, ws.qT[k], s));
    BLVM_TRY(t16_pack_transposed(w->prior_w[k], H, H, H, ws.pT[k], s));
  }
  BLVM_TRY(t16_pack_transposed(w->post_hw, H, 2 * Z, H, ws.qhT, s));
  BLVM_TRY(t16_pack_transposed(w->prior_hw, H, 2 * Z, H, ws.phT, s));
  BLVM_TRY(pack_scope.flush());
  BLVM_HIP(hipMemsetAsync(ws.G, 0, sizeof(float) * bh, s));
  const int rt = (B + 15) / 16;
  const bool persistent = pchain_applies(B) && device_cus() >= 32;
  count_rssm(persistent ? RSSM_BWD_PROGRAM : RSSM_BWD_PER_LINK);
  if (persistent) {
    // Persistent path: the BPTT chain as a program of 12 descriptors walked for s = 0 .. T (t = T-1-s; s = T: the gradients wrt the
    // initial state).  The running gradient wrt h lives in per-step slabs, each written once: GA[t] = g_t * u_t (GRU-backward link),
    // GB[t] = GA[t+1] + DGH[t+1] W_hh (a K = 3H product nothing needs before the GRU-backward link three links later: own range).
    using namespace pchain;
    const int ctH = H / 16, ctZ = Z / 16, cus = device_cus() & ~7;
    const long sH = (long)B * H, sZ = (long)B * Z, s3H = 3 * sH, s2Z = 2 * sZ;
    const long xH = (long)rt * 16 * H, x3H = 3 * xH, x2Z = (long)rt * 16 * 2 * Z;
    const int r_h = range_for(ctH * rt, cus / 4), r_gb = range_for(ctH * rt, cus - 2 * r_h);
    Builder bld;
    bld.begin(pchain_optype(B), T + 1, B, 2, true, 2 * r_h);
    auto last = [&](const float* base, long step) { return rev(base, step, T - 1); };  // slab of t = T-1, walked backwards
    {  // B1: dz_t (direct + through the GRU input layer of step t+1), rsample / combination / KL / softplus heads
      Operands z;
      z.p[DZ_D16] = rev(ws.DGIN16, xH, T); z.p[DZ_WT] = ws.gzT; z.p[DZ_ADD] = rev(d_zs, sZ, T); z.ld[DZ_LD_ADD] = Z; z.p[DZ_MU_Q] = last(mu_q, sZ);
      z.p[DZ_SD_Q] = last(sd_q, sZ); z.p[DZ_MU_P] = last(mu_p, sZ); z.p[DZ_SD_P] = last(sd_p, sZ); z.p[DZ_EPS] = last(eps, sZ); z.p[DZ_RAW_Q] = last(rs.RAWQ, sZ);
      z.p[DZ_RAW_P] = last(rs.RAWP, sZ); z.p[DZ_MUQ_RAW] = last(rs.MUQR, sZ); z.p[DZ_X_SL] = x_sl; z.p[DZ_C_RAW] = c_raw; z.p[DZ_C_FN] = c_fn;
      z.p[DZ_DQH] = last(ws.DQH, s2Z); z.p[DZ_DQH16] = last(ws.DQH16, x2Z); z.p[DZ_DPH] = last(ws.DPH, s2Z); z.p[DZ_DPH16] = last(ws.DPH16, x2Z); z.ld[LD_OUT] = 2 * Z;
      z.n16[N16_OUT] = 2 * ctZ; z.i[DZ_I_Z] = Z; z.i[DZ_I_RESIDUAL] = mode; z.i[DZ_I_STRIDE] = stride; z.i[DZ_I_T0] = T - 1; z.f[DZ_F_FN_FLOOR] = fn_floor;
      z.f[DZ_F_BETA] = beta; z.f[DZ_F_SD_EPS] = sd_eps; z.f[DZ_F_GEMM_FROM] = 1.f;
      add_desc(bld, K_DZ, ctZ, 0, range_for(ctZ * rt, 2 * r_h), H, 0, 0, T, z);
    }
    // B2: heads -> third layers (posterior | prior), B3, B4 | GB[t] = GA[t+1] + DGH[t+1] W_hh
    auto blink = [&](const float* W, const float* gate, float* orm, float* o16) { return rev_link(W, gate, orm, o16, T - 1, sH, H, xH); };
    {  // B2 .. B4 of a branch: one visit
      const SeqLink lq[3] = {blink(ws.qhT, rs.Q[2], ws.DQ[2], ws.DQ16[2]), blink(ws.qT[2], rs.Q[1], ws.DQ[1], ws.DQ16[1]), blink(ws.qT[1], rs.Q[0], ws.DQ[0], ws.DQ16[0])};
      const SeqLink lp[3] = {blink(ws.phT, rs.P[2], ws.DP[2], ws.DP16[2]), blink(ws.pT[2], rs.P[1], ws.DP[1], ws.DP16[1]), blink(ws.pT[1], rs.P[0], ws.DP[0], ws.DP16[0])};
      add_linseq(bld, ctH, 0, r_h, H, false, true, 0, T, last(ws.DQH16, x2Z), 3, lq, -sH, -xH, ctH, 0.f, H, 2 * Z);
      add_linseq(bld, ctH, r_h, r_h, H, false, true, 0, T, last(ws.DPH16, x2Z), 3, lp, -sH, -xH, ctH, 0.f, H, 2 * Z);
    }
    Operands gb;  // (also the h0 link below)
    gb.p[LIN_A] = rev(ws.DGH16, x3H, T); gb.p[LIN_W] = ws.whhT; gb.p[LIN_ADD] = rev(ws.GA, sH, T); gb.ld[LIN_LD_ADD] = H; gb.ld[LIN_LD_GATE] = H;
    gb.p[LIN_ORM] = last(ws.GB, sH); gb.ld[LD_OUT] = H;
    add_desc(bld, K_LIN, ctH, 2 * r_h, r_gb, 3 * H, DF_GENTLE | DF_ADD_POLLED | DF_RM_SC1, 1, T, gb);
    {  // B5: complete dL/dh_t, gate derivatives of step t
      Operands o;
      o.p[GRUB_D0_16] = last(ws.DQ16[0], xH); o.p[GRUB_D1_16] = last(ws.DP16[0], xH); o.p[GRUB_W0] = ws.qT[0]; o.p[GRUB_W1] = ws.pT[0]; o.p[GRUB_G_IN] = last(ws.GB, sH);
      o.p[GRUB_RG] = last(rs.RG, sH); o.p[GRUB_UG] = last(rs.UG, sH); o.p[GRUB_NG] = last(rs.NG, sH); o.p[GRUB_GH] = last(rs.GHb, s3H); o.p[GRUB_HPREV] = last(hs, sH);
      o.p[GRUB_DGI] = last(ws.DGI, s3H); o.p[GRUB_DGI16] = last(ws.DGI16, x3H); o.p[GRUB_DGH] = last(ws.DGH, s3H); o.p[GRUB_DGH16] = last(ws.DGH16, x3H);
      o.p[GRUB_GA] = last(ws.GA, sH); o.p[GRUB_G_OUT] = ws.G; o.p[GRUB_G_ADD] = rev(d_hs, sH, T); o.ld[GRUB_LD_H] = H; o.ld[GRUB_LD_GADD] = H; o.ld[LD_OUT] = 3 * H;
      o.n16[N16_OUT] = 3 * ctH; o.i[GRUB_I_R] = H; o.i[GRUB_I_GEMM_FROM] = 0; o.i[GRUB_I_GATES_TO] = T; o.i[GRUB_I_GIN_FROM] = 1;
      add_desc(bld, K_GRUB, ctH, 0, r_h, H, 0, 0, T, o);
    }
    {  // B6: through the GRU input projection to the (ReLU) GRU input layer
      Operands o;
      o.p[LIN_A] = last(ws.DGI16, x3H); o.p[LIN_W] = ws.wihT; o.p[LIN_GATE] = last(rs.GIN, sH); o.ld[LIN_LD_GATE] = H; o.p[LIN_ORM] = last(ws.DGIN, sH); o.ld[LD_OUT] = H;
      o.p[LIN_O16] = last(ws.DGIN16, xH); o.n16[N16_OUT] = ctH;
      add_desc(bld, K_LIN, ctH, 0, r_h, 3 * H, 0, 0, T, o);
    }
    // s = T: gradients wrt the initial state: z0 through the GRU input layer of step 0 (+ its direct gradient), h0 through the GRU
    // of step 0 (the caller adds the direct gradient d_hs[0])
    if (d_z0) {
      Operands o;
      o.p[LIN_A] = rev(ws.DGIN16, xH, T); o.p[LIN_W] = ws.gzT; o.p[LIN_ADD] = rev(d_zs, sZ, T); o.ld[LIN_LD_ADD] = Z; o.ld[LIN_LD_GATE] = H; o.p[LIN_ORM] = d_z0;
      o.ld[LD_OUT] = Z;
      add_desc(bld, K_LIN, ctZ, 0, range_for(ctZ * rt, 2 * r_h), H, 0, T, T + 1, o);
    }
    if (d_h0) {
      gb.p[LIN_ORM] = d_h0;
      add_desc(bld, K_LIN, ctH, 2 * r_h, r_gb, 3 * H, DF_ADD_POLLED, T, T + 1, gb);
    }
    BLVM_HIP(pchain_fill_sentinel(ws.GA, ws.x16_bytes, s));
    BLVM_TRY(pchain_launch(bld, "rssm_bwd", s));
  }
  for (int t = T - 1; t >= 0 && !persistent; --t) {
    const size_t oH = (size_t)t * B * H, oZ = (size_t)t * B * Z, o3 = (size_t)t * B * 3 * H, o2Z = (size_t)t * B * 2 * Z;
    const bool last = t == T - 1;
    // B1: dz_t (direct + through the GRU input layer of step t+1), then rsample / combination / KL / softplus heads
    DzArgs dz;
    dz.has_gemm = !last;
    dz.D = ws.DGIN + (last ? 0 : oH + bh); dz.WT = ws.gzT; dz.D2 = nullptr; dz.WT2 = nullptr;
    dz.dz_add = d_zs + oZ + bz; dz.ld_add = Z;
    dz.mu_q = mu_q + oZ; dz.sd_q = sd_q + oZ; dz.mu_p = mu_p + oZ; dz.sd_p = sd_p + oZ; dz.eps = eps + oZ;
    dz.raw_q = rs.RAWQ + oZ; dz.raw_p = rs.RAWP + oZ; dz.muq_raw = rs.MUQR + oZ;
    dz.x_sl = x_sl; dz.c_raw = c_raw; dz.c_fn = c_fn;
    dz.dqh = ws.DQH + o2Z; dz.dph = ws.DPH + o2Z;
    dz.B = B; dz.H = H; dz.Z = Z; dz.residual = mode; dz.t = t; dz.stride = stride;
    dz.fn_floor = fn_floor; dz.beta = beta; dz.sd_eps = sd_eps;
    launch_dz(dz, pick_nw(H, 1), dim3(Z / 16, rt), s);
    // B2: heads -> third layers | G += DGH[t+1] Whh (the recurrent path of step t+1, off the critical chain)
    LinLaunch l;
    l.B = B; l.nseg = last ? 2 : 3;
    l.seg[0] = seg(ws.DQH + o2Z, 2 * Z, ws.qhT, 2 * Z, nullptr, nullptr, 0, rs.Q[2] + oH, H, ws.DQ[2] + oH, H, H, 2 * Z, 0);
    l.seg[1] = seg(ws.DPH + o2Z, 2 * Z, ws.phT, 2 * Z, nullptr, nullptr, 0, rs.P[2] + oH, H, ws.DP[2] + oH, H, H, 2 * Z, 0);
    if (!last) l.seg[2] = seg(ws.DGH + o3 + (size_t)B * 3 * H, 3 * H, ws.whhT, 3 * H, nullptr, ws.G, H, nullptr, 0, ws.G, H, H, 3 * H, 0);
    count_lin(launch_lin(l, s));
    // B3, B4
    l.nseg = 2;
    for (int k = 2; k >= 1; --k) {
      l.seg[0] = seg(ws.DQ[k] + oH, H, ws.qT[k], H, nullptr, nullptr, 0, rs.Q[k - 1] + oH, H, ws.DQ[k - 1] + oH, H, H, H, 0);
      l.seg[1] = seg(ws.DP[k] + oH, H, ws.pT[k], H, nullptr, nullptr, 0, rs.P[k - 1] + oH, H, ws.DP[k - 1] + oH, H, H, H, 0);
      count_lin(launch_lin(l, s));
    }
    // B5: complete dL/dh_t and the gate derivatives of step t
    RssmDhArgs d;
    d.DQ0 = ws.DQ[0] + oH; d.DP0 = ws.DP[0] + oH; d.WqT = ws.qT[0]; d.WpT = ws.pT[0];
    d.dh_add = d_hs + oH + bh; d.G = ws.G;
    d.rg = rs.RG + oH; d.ug = rs.UG + oH; d.ng = rs.NG + oH; d.gh = rs.GHb + o3; d.hprev = hs + oH;
    d.dgi = ws.DGI + o3; d.dgh = ws.DGH + o3; d.B = B; d.H = H;
    {
      const int nw = pick_nw(H, 2);
      const dim3 grid(H / 16, rt);
      const unsigned b_h = (unsigned)B | ((unsigned)H << 16);
      LAUNCH_NW(rssm_dh_stage_kernel<NW_>, nw, grid, s, d.DQ0, d.DP0, d.WqT, d.WpT, d.G, b_h, d);
    }
    // B6: through the GRU input projection to the (ReLU) GRU input layer
    l.nseg = 1;
    l.seg[0] = seg(ws.DGI + o3, 3 * H, ws.wihT, 3 * H, nullptr, nullptr, 0, rs.GIN + oH, H, ws.DGIN + oH, H, H, 3 * H, 0);
    count_lin(launch_lin(l, s));
  }
  BLVM_CHECK_LAUNCH("rssm_seq_bwd");
  // gradients wrt the initial state: z0 through the GRU input layer of step 0 (+ its direct gradient), h0 through the
  // GRU of step 0 (the caller adds the direct gradient d_hs[0])
  if (d_z0 && !persistent) {
    LinLaunch l;
    l.B = B; l.nseg = 1;
    l.seg[0] = seg(ws.DGIN, H, ws.gzT, H, nullptr, d_zs, Z, nullptr, 0, d_z0, Z, Z, H, 0);
    count_lin(launch_lin(l, s));
  }
  if (d_h0 && !persistent) {
    LinLaunch l;
    l.B = B; l.nseg = 1;
    l.seg[0] = seg(ws.DGH, 3 * H, ws.whhT, 3 * H, nullptr, ws.G, H, nullptr, 0, d_h0, H, H, 3 * H, 0);
    count_lin(launch_lin(l, s));
  }
  BLVM_CHECK_LAUNCH("rssm_seq_bwd tail");
  // batched, state-independent part
  const float* hnew_all = hs + bh;  // h_1..h_T
  if (d_ctx && C > 0) BLVM_TRY(gemm_f32(0, 1, (int)n, C, H, ws.DGIN, H, w->gin_w + Z, ldg, d_ctx, C, nullptr, 0, 0.f, nullptr, 0, 0, 1, s));
  if (d_enc) BLVM_TRY(gemm_f32(0, 1, (int)n, E, H, ws.DQ[0], H, w->post_w[0] + H, ldq, d_enc, E, nullptr, 0, 0.f, nullptr, 0, 0, 1, s));
  WgradGroup grp;  // every weight gradient of the sequence: one grouped launch
  grp.add(ws.DGIN, H, H, zs, Z, Z, gr->gin_w, ldg, gr->gin_b);
  if (C > 0) grp.add(ws.DGIN, H, H, ctx, C, C, gr->gin_w ? gr->gin_w + Z : nullptr, ldg);
  grp.add(ws.DGI, 3 * H, 3 * H, rs.GIN, H, H, gr->gru_wih, H, gr->gru_bih);
  grp.add(ws.DGH, 3 * H, 3 * H, hs, H, H, gr->gru_whh, H, gr->gru_bhh);
  grp.add(ws.DQ[0], H, H, hnew_all, H, H, gr->post_w[0], ldq);
  grp.add(ws.DQ[0], H, H, enc, E, E, gr->post_w[0] ? gr->post_w[0] + H : nullptr, ldq, gr->post_b[0]);
  grp.add(ws.DP[0], H, H, hnew_all, H, H, gr->prior_w[0], H, gr->prior_b[0]);
  for (int k = 1; k < 3; ++k) {
    grp.add(ws.DQ[k], H, H, rs.Q[k - 1], H, H, gr->post_w[k], H, gr->post_b[k]);
    grp.add(ws.DP[k], H, H, rs.P[k - 1], H, H, gr->prior_w[k], H, gr->prior_b[k]);
  }
  grp.add(ws.DQH, 2 * Z, 2 * Z, rs.Q[2], H, H, gr->post_hw, H, gr->post_hb);
  grp.add(ws.DPH, 2 * Z, 2 * Z, rs.P[2], H, H, gr->prior_hw, H, gr->prior_hb);
  BLVM_TRY(grp.run(n, s));
  return BLVM_OK;
}
