// srnn.hip — K3: the SRNN latent chain (forward + BPTT) as a stage-kernel chain.
//
// Replaces the Python loop over time of the reference (blvm/models/srnn.py:224-253): per step
//   h_p = cat[d_t, z_{t-1}], h_q = cat[a_t, z_{t-1}];  prior / posterior = 3 x (Linear + LeakyReLU) + DiagonalGaussianDense
//   (srnn.py:92-111);  enc_mu += prior_mu (residual posterior);  z_t = rsample
// and its autograd backward.  Only the z-halves of the two first layers are recurrent: the d/a halves are hoisted
// into one MFMA GEMM each before the loop, so a step is 4 dependent links (first layers | second | third | heads +
// sample) forward and 4 backward, every element-wise piece fused into an epilogue (stages.h).  The KL(+free nats)
// gradient is folded into the backward chain exactly as for the VRNN cell.
#include <atomic>

#include "common.h"
#include "pchain.h"

namespace blvm {
namespace {

#include "stages.h"

struct SrnnReserve {
  float *P[3], *Q[3], *XP, *XQ, *RAWP, *RAWQ, *Wp[3], *Wq[3], *Wph, *Wqh;  // W*: T16 weight copies
  float *Z16, *P16[3], *Q16[3];  // persistent forward (B <= kPchainCarveMaxB): T16 copies of what the links multiply
  size_t x16_bytes;  // from the first piece a launch polls to the end of the T16 copies: sentinel-filled in one go
};
size_t carve_srnn(float* base, int Tp, int B, int H, int Z, SrnnReserve* r) {
  const size_t n = (size_t)Tp * B;
  Arena ar{base};
  SrnnReserve t;
  for (int i = 0; i < 3; ++i) t.P[i] = ar.take(n * H);
  for (int i = 0; i < 3; ++i) t.Q[i] = ar.take(n * H);
  t.XP = ar.take(n * H); t.XQ = ar.take(n * H);
  t.RAWP = ar.take(n * Z); t.RAWQ = ar.take(n * Z);
  t.Wp[0] = ar.take((size_t)H * Z); t.Wq[0] = ar.take((size_t)H * Z);
  for (int i = 1; i < 3; ++i) { t.Wp[i] = ar.take((size_t)H * H); t.Wq[i] = ar.take((size_t)H * H); }
  t.Wph = ar.take((size_t)2 * Z * H); t.Wqh = ar.take((size_t)2 * Z * H);
  t.Z16 = nullptr;
  if (B <= kPchainCarveMaxB) {
    const size_t rows = (size_t)((B + 15) / 16) * 16, m = (size_t)Tp * rows;
    t.Z16 = ar.take((m + rows) * Z);
    for (int i = 0; i < 3; ++i) { t.P16[i] = ar.take(m * H); t.Q16[i] = ar.take(m * H); }
    t.x16_bytes = ar.bytes_from(t.Z16);
  }
  if (r) *r = t;
  return ar.floats();
}

struct SrnnWs {
  float *pzT, *qzT, *pT[3], *qT[3], *phT, *qhT, *DPH, *DQH, *DP[3], *DQ[3];
  float *DZ0, *DPH16, *DQH16, *DP16[3], *DQ16[3];  // persistent backward (B <= kPchainCarveMaxB)
  size_t x16_bytes;  // from the first piece a launch polls to the end of the T16 copies: sentinel-filled in one go
};
size_t carve_srnn_ws(float* base, int Tp, int B, int H, int Z, SrnnWs* w) {
  const size_t n = (size_t)Tp * B;
  Arena ar{base};
  SrnnWs t;
  t.pzT = ar.take((size_t)Z * H); t.qzT = ar.take((size_t)Z * H);
  t.pT[0] = t.qT[0] = nullptr;
  for (int i = 1; i < 3; ++i) { t.pT[i] = ar.take((size_t)H * H); t.qT[i] = ar.take((size_t)H * H); }
  t.phT = ar.take((size_t)H * 2 * Z); t.qhT = ar.take((size_t)H * 2 * Z);
  t.DPH = ar.take(n * 2 * Z); t.DQH = ar.take(n * 2 * Z);
  for (int i = 0; i < 3; ++i) { t.DP[i] = ar.take(n * H); t.DQ[i] = ar.take(n * H); }
  t.DZ0 = nullptr;
  if (B <= kPchainCarveMaxB) {
    const size_t m = (size_t)Tp * ((B + 15) / 16) * 16;
    t.DZ0 = ar.take((size_t)B * Z);
    t.DPH16 = ar.take(m * 2 * Z); t.DQH16 = ar.take(m * 2 * Z);
    for (int i = 0; i < 3; ++i) { t.DP16[i] = ar.take(m * H); t.DQ16[i] = ar.take(m * H); }
    t.x16_bytes = ar.bytes_from(t.DZ0);
  }
  if (w) *w = t;
  return ar.floats();
}

// which implementation the entry points took and which tiles their per-link loops ran on (blvm_srnn_path_counts): host-side
// counts, [0..3] one per call, [4..5] one per launch_lin of the launch-per-link loops
enum { SRNN_FWD_PROGRAM = 0, SRNN_FWD_PER_LINK = 1, SRNN_BWD_PROGRAM = 2, SRNN_BWD_PER_LINK = 3, SRNN_LIN16 = 4, SRNN_LIN32 = 5 };
std::atomic<unsigned long long> g_srnn_counts[6];
inline void count_srnn(int k) { g_srnn_counts[k].fetch_add(1, std::memory_order_relaxed); }
inline void count_lin(int tile_width) { count_srnn(tile_width == 32 ? SRNN_LIN32 : SRNN_LIN16); }

int check_srnn(int Tp, int B, int H, int Z, int R) {
  BLVM_REQUIRE(Tp > 0 && B > 0, "srnn: bad Tp=%d B=%d", Tp, B);
  BLVM_REQUIRE(H > 0 && Z > 0 && R > 0 && H % 16 == 0 && Z % 16 == 0 && R % 16 == 0,
               "srnn: H,Z,R must be positive multiples of 16 (got %d,%d,%d)", H, Z, R);
  BLVM_REQUIRE(B < 65536 && H < 65536, "srnn: B and H must be below 65536 (packed kernel arguments)");
  return BLVM_OK;
}

}  // namespace
}  // namespace blvm

using namespace blvm;

extern "C" int blvm_srnn_path_counts(unsigned long long out[6]) {
  BLVM_REQUIRE(out, "srnn_path_counts: null pointer");
  for (int k = 0; k < 6; ++k) out[k] = g_srnn_counts[k].load(std::memory_order_relaxed);
  return BLVM_OK;
}

extern "C" size_t blvm_srnn_reserve_floats(int Tp, int B, int H, int Z, int R) {
  (void)R;
  return carve_srnn(nullptr, Tp, B, H, Z, nullptr);
}
extern "C" size_t blvm_srnn_bwd_workspace_floats(int Tp, int B, int H, int Z, int R) {
  (void)R;
  return carve_srnn_ws(nullptr, Tp, B, H, Z, nullptr);
}

extern "C" int blvm_srnn_latent_fwd(const BlvmSrnnWeights* w, const float* d, const float* a, const float* z0,
                                    const float* eps, int Tp, int B, int H, int Z, int R, int residual_posterior,
                                    float sd_eps, float slope, float* zs, float* mu_q, float* sd_q, float* mu_p,
                                    float* sd_p, float* reserve, void* stream_) {
  hipStream_t s = static_cast<hipStream_t>(stream_);
  BLVM_TRY(check_srnn(Tp, B, H, Z, R));
  BLVM_REQUIRE(w && d && a && eps && zs && mu_q && sd_q && mu_p && sd_p && reserve, "srnn_fwd: null pointer");
  BLVM_REQUIRE(aligned16(zs) && aligned16(reserve) && aligned16(d) && aligned16(a), "srnn_fwd: buffers must be 16-byte aligned");
  SrnnReserve rs;
  carve_srnn(reserve, Tp, B, H, Z, &rs);
  const size_t n = (size_t)Tp * B;
  const int ldw0 = R + Z;
  const float beta = softplus_beta_of(sd_eps);
  // hoisted d / a halves of the two first layers (incl. bias)
  BLVM_TRY(gemm_f32(0, 0, (int)n, H, R, d, R, w->prior_w[0], ldw0, rs.XP, H, w->prior_b[0], 0, 0.f, nullptr, 0, 0, 1, s));
  BLVM_TRY(gemm_f32(0, 0, (int)n, H, R, a, R, w->post_w[0], ldw0, rs.XQ, H, w->post_b[0], 0, 0.f, nullptr, 0, 0, 1, s));
  // T16 operand copies of the chain's weights (once per sequence); layer 0: the z columns
  T16PackScope pack_scope(pchain_optype(B), s);  // 16-bit operand modes: the persistent launch multiplies 16-bit weight packs
  BLVM_TRY(t16_pack_rows(w->prior_w[0] + R, ldw0, H, Z, rs.Wp[0], s));
  BLVM_TRY(t16_pack_rows(w->post_w[0] + R, ldw0, H, Z, rs.Wq[0], s));
  for (int k = 1; k < 3; ++k) {
    BLVM_TRY(t16_pack_rows(w->prior_w[k], H, H, H, rs.Wp[k], s));
    BLVM_TRY(t16_pack_rows(w->post_w[k], H, H, H, rs.Wq[k], s));
  }
  BLVM_TRY(t16_pack_rows(w->prior_hw, H, 2 * Z, H, rs.Wph, s));
  BLVM_TRY(t16_pack_rows(w->post_hw, H, 2 * Z, H, rs.Wqh, s));
  BLVM_TRY(pack_scope.flush());  // all packs above in one launch
  BLVM_HIP(copy_or_zero(zs, z0, sizeof(float) * (size_t)B * Z, s));
  const int rt = (B + 15) / 16;
  if (pchain_applies(B) && device_cus() >= 32) {
    // Persistent path (pchain.h / pchain.hip): the four links of a step as a program of 7 descriptors, one launch per sequence
    using namespace pchain;
    count_srnn(SRNN_FWD_PROGRAM);
    const int ctH = H / 16, ctZ = Z / 16, cus = device_cus() & ~7;
    const long sH = (long)B * H, sZ = (long)B * Z, xH = (long)rt * 16 * H, xZ = (long)rt * 16 * Z;
    const int half = range_for(ctH * rt, cus / 2);
    Builder bld;
    bld.begin(pchain_optype(B), Tp, B, 4, false, half);
    {  // the three layers of the prior | posterior MLP: one visit per chain and step (the first layer, K = Z, opens the run)
      const SeqLink lp[3] = {{rs.Wp[0], nullptr, rs.P[0], sH, H, rs.P16[0]}, {rs.Wp[1], w->prior_b[1], rs.P[1], sH, H, rs.P16[1]}, {rs.Wp[2], w->prior_b[2], rs.P[2], sH, H, rs.P16[2]}};
      const SeqLink lq[3] = {{rs.Wq[0], nullptr, rs.Q[0], sH, H, rs.Q16[0]}, {rs.Wq[1], w->post_b[1], rs.Q[1], sH, H, rs.Q16[1]}, {rs.Wq[2], w->post_b[2], rs.Q[2], sH, H, rs.Q16[2]}};
      add_linseq(bld, ctH, 0, half, H, true, false, 0, Tp, {rs.Z16, xZ}, 3, lp, 0, xH, ctH, slope, 0, Z, {rs.XP, sH}, H);
      add_linseq(bld, ctH, half, half, H, true, false, 0, Tp, {rs.Z16, xZ}, 3, lq, 0, xH, ctH, slope, 0, Z, {rs.XQ, sH}, H);
    }
    {
      Operands o;
      o.p[HEAD_P16] = {rs.P16[2], xH}; o.p[HEAD_Q16] = {rs.Q16[2], xH}; o.p[HEAD_WP] = rs.Wph; o.p[HEAD_BP] = w->prior_hb; o.p[HEAD_WQ] = rs.Wqh;
      o.p[HEAD_BQ] = w->post_hb; o.p[HEAD_EPS] = {eps, sZ}; o.p[HEAD_MU_P] = {mu_p, sZ}; o.p[HEAD_SD_P] = {sd_p, sZ}; o.p[HEAD_MU_Q] = {mu_q, sZ};
      o.p[HEAD_SD_Q] = {sd_q, sZ}; o.p[HEAD_RAW_P] = {rs.RAWP, sZ}; o.p[HEAD_RAW_Q] = {rs.RAWQ, sZ}; o.p[HEAD_Z] = {zs + sZ, sZ}; o.p[HEAD_Z16] = {rs.Z16 + xZ, xZ};
      o.ld[LD_OUT] = Z; o.n16[N16_OUT] = ctZ; o.i[HEAD_I_Z] = Z; o.i[HEAD_I_RESIDUAL] = residual_posterior; o.f[HEAD_F_BETA] = beta; o.f[HEAD_F_INV_BETA] = 1.f / beta;
      o.f[HEAD_F_SD_EPS] = sd_eps;
      add_desc(bld, K_HEAD, ctZ, 0, range_for(ctZ * rt, 2 * half), H, 0, 0, Tp, o);
    }
    BLVM_HIP(pchain_fill_sentinel(rs.Z16, rs.x16_bytes, s));
    BLVM_TRY(pchain_rows_to_t16(zs, Z, B, Z, rs.Z16, s));
    return pchain_launch(bld, "srnn_fwd", s);
  }
  count_srnn(SRNN_FWD_PER_LINK);
  for (int t = 0; t < Tp; ++t) {
    const size_t oH = (size_t)t * B * H, oZ = (size_t)t * B * Z;
    const float* zprev = zs + oZ;
    LinLaunch l;
    l.B = B; l.slope = slope; l.nseg = 2;
    l.seg[0] = seg(zprev, Z, rs.Wp[0], Z, nullptr, rs.XP + oH, H, nullptr, 0, rs.P[0] + oH, H, H, Z, 1);
    l.seg[1] = seg(zprev, Z, rs.Wq[0], Z, nullptr, rs.XQ + oH, H, nullptr, 0, rs.Q[0] + oH, H, H, Z, 1);
    count_lin(launch_lin(l, s));
    for (int k = 1; k < 3; ++k) {
      l.seg[0] = seg(rs.P[k - 1] + oH, H, rs.Wp[k], H, w->prior_b[k], nullptr, 0, nullptr, 0, rs.P[k] + oH, H, H, H, 1);
      l.seg[1] = seg(rs.Q[k - 1] + oH, H, rs.Wq[k], H, w->post_b[k], nullptr, 0, nullptr, 0, rs.Q[k] + oH, H, H, H, 1);
      count_lin(launch_lin(l, s));
    }
    HeadArgs h;
    h.P = rs.P[2] + oH; h.Q = rs.Q[2] + oH;
    h.Wp = rs.Wph; h.bp = w->prior_hb; h.Wq = rs.Wqh; h.bq = w->post_hb;
    h.eps = eps + oZ;
    h.mu_p = mu_p + oZ; h.sd_p = sd_p + oZ; h.mu_q = mu_q + oZ; h.sd_q = sd_q + oZ;
    h.z = zs + (size_t)(t + 1) * B * Z;
    h.raw_p = rs.RAWP + oZ; h.raw_q = rs.RAWQ + oZ;
    h.B = B; h.H = H; h.Z = Z; h.residual = residual_posterior;
    h.beta = beta; h.inv_beta = 1.f / beta; h.sd_eps = sd_eps; h.muq_raw = nullptr;
    launch_head(h, pick_nw(H, 4), dim3(Z / 16, rt), s);
  }
  BLVM_CHECK_LAUNCH("srnn_latent_fwd");
  return BLVM_OK;
}

extern "C" int blvm_srnn_latent_bwd(const BlvmSrnnWeights* w, const float* d, const float* a, const float* eps,
                                    const float* zs, const float* mu_q, const float* sd_q, const float* mu_p,
                                    const float* sd_p, const float* reserve, const float* d_z, const int32_t* x_sl,
                                    const float* c_raw, const float* c_fn, int stride, float fn_floor, int Tp, int B,
                                    int H, int Z, int R, int residual_posterior, float sd_eps, float slope, float* d_d,
                                    float* d_a, float* d_z0, const BlvmSrnnGrads* gr, float* workspace, void* stream_) {
  hipStream_t s = static_cast<hipStream_t>(stream_);
  BLVM_TRY(check_srnn(Tp, B, H, Z, R));
  BLVM_REQUIRE(w && d && a && eps && zs && mu_q && sd_q && mu_p && sd_p && reserve && d_z && workspace && gr, "srnn_bwd: null pointer");
  BLVM_REQUIRE((c_fn == nullptr && c_raw == nullptr) || x_sl != nullptr, "srnn_bwd: KL coefficients need x_sl");
  BLVM_REQUIRE(aligned16(workspace) && aligned16(reserve), "srnn_bwd: buffers must be 16-byte aligned");
  SrnnReserve rs;
  carve_srnn(const_cast<float*>(reserve), Tp, B, H, Z, &rs);
  SrnnWs ws;
  carve_srnn_ws(workspace, Tp, B, H, Z, &ws);
  const size_t n = (size_t)Tp * B;
  const int ldw0 = R + Z;
  const float beta = softplus_beta_of(sd_eps);
  T16PackScope pack_scope(pchain_optype(B), s);  // 16-bit operand modes: the persistent launch multiplies 16-bit weight packs
  BLVM_TRY(t16_pack_transposed(w->prior_w[0] + R, ldw0, H, Z, ws.pzT, s));
  BLVM_TRY(t16_pack_transposed(w->post_w[0] + R, ldw0, H, Z, ws.qzT, s));
  for (int k = 1; k < 3; ++k) {
    BLVM_TRY(t16_pack_transposed(w->prior_w[k], H, H, H, ws.pT[k], s));
    BLVM_TRY(t16_pack_transposed(w->post_w[k], H, H, H, ws.qT[k], s));
  }
  BLVM_TRY(t16_pack_transposed(w->prior_hw, H, 2 * Z, H, ws.phT, s));
  BLVM_TRY(t16_pack_transposed(w->post_hw, H, 2 * Z, H, ws.qhT, s));
  BLVM_TRY(pack_scope.flush());
  const int rt = (B + 15) / 16;
  const bool persistent = pchain_applies(B) && device_cus() >= 32;
  count_srnn(persistent ? SRNN_BWD_PROGRAM : SRNN_BWD_PER_LINK);
  if (persistent) {
    // Persistent path: the BPTT chain as a program of 9 descriptors walked for s = 0 .. T' (t = T'-1-s; s = T': the gradient wrt z_0)
    using namespace pchain;
    const int ctH = H / 16, ctZ = Z / 16, cus = device_cus() & ~7, T = Tp;
    const long sH = (long)B * H, sZ = (long)B * Z, s2Z = 2 * sZ, xH = (long)rt * 16 * H, x2Z = (long)rt * 16 * 2 * Z;
    const int half = range_for(ctH * rt, cus / 2);
    Builder bld;
    bld.begin(pchain_optype(B), T + 1, B, 2, true, half);
    auto last = [&](const float* base, long step) { return rev(base, step, T - 1); };  // slab of t = T'-1, walked backwards
    {  // B1: dz_t = decoder gradient + the two first layers of step t+1, then rsample / residual / KL / softplus heads
      Operands z;
      z.p[DZ_D16] = rev(ws.DP16[0], xH, T); z.p[DZ_WT] = ws.pzT; z.p[DZ_D2_16] = rev(ws.DQ16[0], xH, T); z.p[DZ_WT2] = ws.qzT; z.p[DZ_ADD] = last(d_z, sZ);
      z.ld[DZ_LD_ADD] = Z; z.p[DZ_MU_Q] = last(mu_q, sZ); z.p[DZ_SD_Q] = last(sd_q, sZ); z.p[DZ_MU_P] = last(mu_p, sZ); z.p[DZ_SD_P] = last(sd_p, sZ);
      z.p[DZ_EPS] = last(eps, sZ); z.p[DZ_RAW_Q] = last(rs.RAWQ, sZ); z.p[DZ_RAW_P] = last(rs.RAWP, sZ); z.p[DZ_X_SL] = x_sl; z.p[DZ_C_RAW] = c_raw; z.p[DZ_C_FN] = c_fn;
      z.p[DZ_DQH] = last(ws.DQH, s2Z); z.p[DZ_DQH16] = last(ws.DQH16, x2Z); z.p[DZ_DPH] = last(ws.DPH, s2Z); z.p[DZ_DPH16] = last(ws.DPH16, x2Z); z.ld[LD_OUT] = 2 * Z;
      z.n16[N16_OUT] = 2 * ctZ; z.i[DZ_I_Z] = Z; z.i[DZ_I_RESIDUAL] = residual_posterior; z.i[DZ_I_STRIDE] = stride; z.i[DZ_I_T0] = T - 1; z.f[DZ_F_FN_FLOOR] = fn_floor;
      z.f[DZ_F_BETA] = beta; z.f[DZ_F_SD_EPS] = sd_eps; z.f[DZ_F_GEMM_FROM] = 1.f;
      add_desc(bld, K_DZ, ctZ, 0, range_for(ctZ * rt, 2 * half), H, 0, 0, T, z);
    }
    // B2: heads -> third layers;  B3, B4: down to the first layers (LeakyReLU derivatives fused)
    auto blink = [&](const float* W, const float* gate, float* orm, float* o16) { return rev_link(W, gate, orm, o16, T - 1, sH, H, xH); };
    {  // B2 .. B4 of a chain: one visit
      const SeqLink lp[3] = {blink(ws.phT, rs.P[2], ws.DP[2], ws.DP16[2]), blink(ws.pT[2], rs.P[1], ws.DP[1], ws.DP16[1]), blink(ws.pT[1], rs.P[0], ws.DP[0], ws.DP16[0])};
      const SeqLink lq[3] = {blink(ws.qhT, rs.Q[2], ws.DQ[2], ws.DQ16[2]), blink(ws.qT[2], rs.Q[1], ws.DQ[1], ws.DQ16[1]), blink(ws.qT[1], rs.Q[0], ws.DQ[0], ws.DQ16[0])};
      add_linseq(bld, ctH, 0, half, H, false, true, 0, T, last(ws.DPH16, x2Z), 3, lp, -sH, -xH, ctH, slope, H, 2 * Z);
      add_linseq(bld, ctH, half, half, H, false, true, 0, T, last(ws.DQH16, x2Z), 3, lq, -sH, -xH, ctH, slope, H, 2 * Z);
    }
    if (d_z0) {  // s = T': gradient wrt the initial latent through both first layers of step 0 (two links: every word written once)
      const int r_z = range_for(ctZ * rt, half);
      Operands o;
      o.p[LIN_A] = rev(ws.DP16[0], xH, T); o.p[LIN_W] = ws.pzT; o.p[LIN_ORM] = ws.DZ0; o.ld[LD_OUT] = Z;
      add_desc(bld, K_LIN, ctZ, 0, r_z, H, DF_RM_SC1, T, T + 1, o);
      o.p[LIN_A] = rev(ws.DQ16[0], xH, T); o.p[LIN_W] = ws.qzT; o.p[LIN_ADD] = ws.DZ0; o.ld[LIN_LD_ADD] = Z; o.p[LIN_ORM] = d_z0;
      add_desc(bld, K_LIN, ctZ, half, r_z, H, DF_ADD_POLLED, T, T + 1, o);
    }
    BLVM_HIP(pchain_fill_sentinel(ws.DZ0, ws.x16_bytes, s));
    BLVM_TRY(pchain_launch(bld, "srnn_bwd", s));
  }
  for (int t = Tp - 1; t >= 0 && !persistent; --t) {
    const size_t oH = (size_t)t * B * H, oZ = (size_t)t * B * Z, o2Z = (size_t)t * B * 2 * Z;
    // B1: dz_t = decoder gradient + the two first layers of step t+1, then rsample / residual / KL / softplus heads
    DzArgs dz;
    dz.has_gemm = t < Tp - 1;
    dz.D = ws.DP[0] + (dz.has_gemm ? oH + (size_t)B * H : 0); dz.WT = ws.pzT;
    dz.D2 = ws.DQ[0] + (dz.has_gemm ? oH + (size_t)B * H : 0); dz.WT2 = ws.qzT;
    dz.dz_add = d_z + oZ; dz.ld_add = Z;
    dz.mu_q = mu_q + oZ; dz.sd_q = sd_q + oZ; dz.mu_p = mu_p + oZ; dz.sd_p = sd_p + oZ; dz.eps = eps + oZ;
    dz.raw_q = rs.RAWQ + oZ; dz.raw_p = rs.RAWP + oZ;
    dz.x_sl = x_sl; dz.c_raw = c_raw; dz.c_fn = c_fn;
    dz.dqh = ws.DQH + o2Z; dz.dph = ws.DPH + o2Z;
    dz.B = B; dz.H = H; dz.Z = Z; dz.residual = residual_posterior; dz.t = t; dz.stride = stride;
    dz.fn_floor = fn_floor; dz.beta = beta; dz.sd_eps = sd_eps; dz.muq_raw = nullptr;
    launch_dz(dz, pick_nw(H, 2), dim3(Z / 16, rt), s);
    // B2: heads -> third layers;  B3, B4: down to the first layers (LeakyReLU derivatives fused)
    LinLaunch l;
    l.B = B; l.slope = slope; l.nseg = 2;
    l.seg[0] = seg(ws.DPH + o2Z, 2 * Z, ws.phT, 2 * Z, nullptr, nullptr, 0, rs.P[2] + oH, H, ws.DP[2] + oH, H, H, 2 * Z, 0);
    l.seg[1] = seg(ws.DQH + o2Z, 2 * Z, ws.qhT, 2 * Z, nullptr, nullptr, 0, rs.Q[2] + oH, H, ws.DQ[2] + oH, H, H, 2 * Z, 0);
    count_lin(launch_lin(l, s));
    for (int k = 2; k >= 1; --k) {
      l.seg[0] = seg(ws.DP[k] + oH, H, ws.pT[k], H, nullptr, nullptr, 0, rs.P[k - 1] + oH, H, ws.DP[k - 1] + oH, H, H, H, 0);
      l.seg[1] = seg(ws.DQ[k] + oH, H, ws.qT[k], H, nullptr, nullptr, 0, rs.Q[k - 1] + oH, H, ws.DQ[k - 1] + oH, H, H, H, 0);
      count_lin(launch_lin(l, s));
    }
  }
  BLVM_CHECK_LAUNCH("srnn_latent_bwd");
  if (d_z0 && !persistent) {  // gradient wrt the initial latent: both first layers of step 0
    LinLaunch l;
    l.B = B; l.slope = 0.f; l.nseg = 1;
    l.seg[0] = seg(ws.DP[0], H, ws.pzT, H, nullptr, nullptr, 0, nullptr, 0, d_z0, Z, Z, H, 0);
    count_lin(launch_lin(l, s));
    l.seg[0] = seg(ws.DQ[0], H, ws.qzT, H, nullptr, d_z0, Z, nullptr, 0, d_z0, Z, Z, H, 0);
    count_lin(launch_lin(l, s));
  }
  // batched, state-independent part
  if (d_d) BLVM_TRY(gemm_f32(0, 1, (int)n, R, H, ws.DP[0], H, w->prior_w[0], ldw0, d_d, R, nullptr, 0, 0.f, nullptr, 0, 0, 1, s));
  if (d_a) BLVM_TRY(gemm_f32(0, 1, (int)n, R, H, ws.DQ[0], H, w->post_w[0], ldw0, d_a, R, nullptr, 0, 0.f, nullptr, 0, 0, 1, s));
  WgradGroup grp;  // every weight gradient of the sequence: one grouped launch
  grp.add(ws.DP[0], H, H, d, R, R, gr->prior_w[0], ldw0);
  grp.add(ws.DP[0], H, H, zs, Z, Z, gr->prior_w[0] ? gr->prior_w[0] + R : nullptr, ldw0, gr->prior_b[0]);
  grp.add(ws.DQ[0], H, H, a, R, R, gr->post_w[0], ldw0);
  grp.add(ws.DQ[0], H, H, zs, Z, Z, gr->post_w[0] ? gr->post_w[0] + R : nullptr, ldw0, gr->post_b[0]);
  for (int k = 1; k < 3; ++k) {
    grp.add(ws.DP[k], H, H, rs.P[k - 1], H, H, gr->prior_w[k], H, gr->prior_b[k]);
    grp.add(ws.DQ[k], H, H, rs.Q[k - 1], H, H, gr->post_w[k], H, gr->post_b[k]);
  }
  grp.add(ws.DPH, 2 * Z, 2 * Z, rs.P[2], H, H, gr->prior_hw, H, gr->prior_hb);
  grp.add(ws.DQH, 2 * Z, 2 * Z, rs.Q[2], H, H, gr->post_hw, H, gr->post_hb);
  BLVM_TRY(grp.run(n, s));
  return BLVM_OK;
}
