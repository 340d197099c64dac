// srnn_decode.hip — K3c: ancestral sampling from SRNNAudio, every step of every utterance in ONE persistent launch.
//
// Replaces the loop of `SRNN.generate` (blvm/models/srnn.py:304-403): enc = encoder(x_t) -> d_t = GRU(enc, d_{t-1}) (srnn.py:113) ->
// prior(cat[d_t, z_{t-1}]) -> z_t = mu + sd eps (srnn.py:92-111) -> decoder(cat[z_t, d_t]) -> DMoL head per sample -> draw -> x_{t+1}.
// A step is a program of 13 links for the persistent-chain engine (pchain.h / pchain.hip), every link's 16x16 tiles dealt over the
// whole chip; the 13.6 MB of weights stay in the L2s, activations travel as sentinel-polled T16 copies in per-step slabs.  The two
// concatenated inputs are ONE T16 slab each, written in parts by the links that produce the parts:
//   CP[s] = cat[d_s | z_{s-1}] (GRU link of step s, head link of step s-1; also the hidden-projection input of step s+1),
//   DC[s] = cat[z_s | d_s]     (head link, GRU link).
#include "common.h"
#include "pchain.h"

namespace blvm {
namespace {
constexpr int SD_F = 30, SD_K = 10;  // DMoL head: 3 * num_mix parameters per sample

// (S % 16 != 0 — pchain.h stack_pad: enc[0] is [H, Sp] and dec[2] [Np, H], packed from zero-padded row-major copies staged behind the
// packs, and the last decoder layer reads the zero-padded bias dec_b2)
struct SdPack { size_t enc[3], wih, whh, prior[3], prior_h, dec[3], st_enc0, st_dec2, dec_b2, total; };
SdPack sd_pack_layout(int S, int H, int Z, int R) {
  SdPack p{};
  Arena ar;
  const StackPad sp = stack_pad(S, SD_F);
  p.enc[0] = ar.take_off((size_t)H * sp.Sp); p.enc[1] = ar.take_off((size_t)H * H); p.enc[2] = ar.take_off((size_t)H * H);
  p.wih = ar.take_off((size_t)3 * R * H); p.whh = ar.take_off((size_t)3 * R * R);
  p.prior[0] = ar.take_off((size_t)H * (R + Z)); p.prior[1] = ar.take_off((size_t)H * H); p.prior[2] = ar.take_off((size_t)H * H);
  p.prior_h = ar.take_off((size_t)2 * Z * H);
  p.dec[0] = ar.take_off((size_t)H * (Z + R)); p.dec[1] = ar.take_off((size_t)H * H); p.dec[2] = ar.take_off((size_t)sp.Np * H);
  if (sp.padded()) { p.st_enc0 = ar.take_off(sp.stage_in(H)); p.st_dec2 = ar.take_off(sp.stage_dec(H)); p.dec_b2 = ar.take_off(sp.stage_bias()); }
  p.total = ar.floats();
  return p;
}
struct SdBufs { size_t X16, E16[2], ENC16, CP16, DS, GHb, P16[3], DC16, D16[2], DEC, ZS, dummyZ, dummyR, end; };
SdBufs sd_layout(size_t base, int T, int B, int S, int H, int Z, int R) {
  SdBufs b;
  Arena ar{nullptr, base};
  const size_t rows = (size_t)((B + 15) / 16) * 16, m = (size_t)T * rows;
  const StackPad sp = stack_pad(S, SD_F);  // X16 slabs [rows, Sp], DEC slabs [B, Np] (padded when S % 16 != 0)
  b.X16 = ar.take_off((m + rows) * sp.Sp);
  b.E16[0] = ar.take_off(m * H); b.E16[1] = ar.take_off(m * H); b.ENC16 = ar.take_off(m * H);
  b.CP16 = ar.take_off((m + 2 * rows) * (R + Z));
  b.DS = ar.take_off((size_t)(T + 1) * B * R);
  b.GHb = ar.take_off((size_t)T * B * 3 * R);
  for (int i = 0; i < 3; ++i) b.P16[i] = ar.take_off(m * H);
  b.DC16 = ar.take_off(m * (Z + R));
  b.D16[0] = ar.take_off(m * H); b.D16[1] = ar.take_off(m * H);
  b.DEC = ar.take_off((size_t)T * B * sp.Np);
  b.ZS = ar.take_off((size_t)T * B * Z);  // z_t row-major (an output)
  b.dummyZ = ar.take_off((size_t)B * Z);
  b.dummyR = ar.take_off((size_t)B * R);
  b.end = ar.floats();
  return b;
}
}  // namespace
}  // namespace blvm

using namespace blvm;

extern "C" size_t blvm_srnn_generate_scratch_floats(int T, int B, int S, int H, int Z, int R) {
  if (T <= 0 || B <= 0 || S <= 0 || H <= 0 || Z <= 0 || R <= 0) return 0;
  return sd_layout(sd_pack_layout(S, H, Z, R).total, T, B, S, H, Z, R).end;
}

extern "C" int blvm_srnn_generate(const BlvmSrnnDecodeWeights* w, const float* x0, const float* d0, const float* z0, const float* eps, const float* u,
                                  const float* v, int T, int B, int S, int H, int Z, int R, int num_mix, float sd_eps, float slope, float log_eps,
                                  float* x_out, float* d_out, float* z_out, float* scratch, void* stream_) {
  using namespace pchain;
  hipStream_t s = static_cast<hipStream_t>(stream_);
  BLVM_REQUIRE(w && w->chain && x0 && eps && x_out && scratch, "srnn_generate: null pointer");
  BLVM_REQUIRE(T >= 0 && B > 0 && B <= kPchainCarveMaxB, "srnn_generate: bad T=%d B=%d (at most %d utterances)", T, B, kPchainCarveMaxB);
  BLVM_REQUIRE(H % 16 == 0 && Z % 16 == 0 && R % 16 == 0 && S > 0 && H > 0 && Z > 0 && R > 0,
               "srnn_generate: S must be positive and H, Z, R positive multiples of 16 (got %d, %d, %d, %d)", S, H, Z, R);
  BLVM_REQUIRE(num_mix == SD_K, "srnn_generate: the DMoL head has %d components", SD_K);
  BLVM_REQUIRE((u == nullptr) == (v == nullptr), "srnn_generate: u and v are given together (both NULL: the mode)");
  BLVM_REQUIRE(aligned16(scratch), "srnn_generate: scratch must be 16-byte aligned");
  BLVM_REQUIRE(device_cus() >= 32, "srnn_generate: needs a device with at least 32 CUs");
  if (T == 0) return BLVM_OK;
  const BlvmSrnnWeights* c = w->chain;
  const SdPack p = sd_pack_layout(S, H, Z, R);
  const SdBufs b = sd_layout(p.total, T, B, S, H, Z, R);
  const StackPad sp = stack_pad(S, SD_F);
  const int Sp = sp.Sp, Np = sp.Np;
  if (sp.padded()) {  // the ragged stack's weights and bias, zero-padded to the tile boundaries
    BLVM_TRY(pad_copy(scratch + p.st_enc0, H, Sp, w->enc_w[0], H, S, s));
    BLVM_TRY(pad_copy(scratch + p.st_dec2, Np, H, w->dec_w[2], sp.N, H, s));
    BLVM_TRY(pad_copy(scratch + p.dec_b2, 1, Np, w->dec_b[2], 1, sp.N, s));
  }
  T16PackScope pack_scope(pchain_optype(B), s);
#define PACK(dst, src, ld, rows, k) BLVM_TRY(t16_pack_rows(src, ld, rows, k, scratch + (dst), s))
  PACK(p.enc[0], sp.padded() ? scratch + p.st_enc0 : w->enc_w[0], sp.Sp, H, sp.Sp); PACK(p.enc[1], w->enc_w[1], H, H, H); PACK(p.enc[2], w->enc_w[2], H, H, H);
  PACK(p.wih, w->gru_wih, H, 3 * R, H); PACK(p.whh, w->gru_whh, R, 3 * R, R);
  PACK(p.prior[0], c->prior_w[0], R + Z, H, R + Z); PACK(p.prior[1], c->prior_w[1], H, H, H); PACK(p.prior[2], c->prior_w[2], H, H, H);
  PACK(p.prior_h, c->prior_hw, H, 2 * Z, H);
  PACK(p.dec[0], w->dec_w[0], Z + R, H, Z + R); PACK(p.dec[1], w->dec_w[1], H, H, H); PACK(p.dec[2], sp.padded() ? scratch + p.st_dec2 : w->dec_w[2], H, sp.Np, H);
#undef PACK
  BLVM_TRY(pack_scope.flush());  // all packs above in one launch
  const int rt = (B + 15) / 16, ctS = Sp / 16, ctH = H / 16, ctZ = Z / 16, ctR = R / 16, cus = device_cus() & ~7;
  const int nCP = (R + Z) / 16, nDC = (Z + R) / 16;
  const long rows = (long)rt * 16, xS = rows * Sp, xH = rows * H, xCP = rows * (R + Z), xDC = rows * (Z + R);
  const long sR = (long)B * R, s3R = 3 * sR, sZ = (long)B * Z, sF = (long)B * Np;
  float* const sc = scratch;
  const float beta = softplus_beta_of(sd_eps);
  const int r_side = range_for(3 * ctR * rt, std::min(cus / 4, 64));  // the hidden projection of the NEXT step: off the critical path
  const int r_main = cus - r_side;
  Builder bld;
  bld.begin(pchain_optype(B), T, B, 4, false, r_main);
  // out = leaky(A W^T + bias): A a polled T16 slab of `a_n16` blocks per row tile, outputs: T16 slab(s) and / or row-major (polled words)
  auto lin = [&](size_t A16, long a_step, int a_n16, size_t W, int K, const float* bias, int ct, int flags, float* orm, long rm_step, int ldo, size_t o16,
                 long o16_step, int n16, int wg0, int nwg) {
    Operands o;
    o.p[LIN_A] = {sc + A16, a_step}; o.p[LIN_W] = sc + W; o.p[LIN_BIAS] = bias; o.p[LIN_ORM] = {orm, rm_step}; o.p[LIN_O16] = {o16 ? sc + o16 : nullptr, o16_step};
    o.ld[LIN_LD_A] = a_n16 * 16; o.ld[LD_OUT] = ldo; o.n16[N16_OUT] = n16; o.f[LIN_F_SLOPE] = slope;
    add_desc(bld, K_LIN, ct, wg0, nwg, K, flags, 0, T, o);
  };
  const int rH = range_for(ctH * rt, r_main);
  // CP slab index: slab 0 = [d_0 | -], slab s + 1 = cat[d_s | z_{s-1}] of step s
  lin(b.X16, xS, ctS, p.enc[0], Sp, w->enc_b[0], ctH, DF_RELU, nullptr, 0, 0, b.E16[0], xH, ctH, 0, rH);
  {  // the next two layers: one descriptor (K_LINSEQ)
    const SeqLink le[2] = {{sc + p.enc[1], w->enc_b[1], nullptr, 0, 0, sc + b.E16[1]}, {sc + p.enc[2], w->enc_b[2], nullptr, 0, 0, sc + b.ENC16}};
    add_linseq(bld, ctH, 0, rH, H, true, false, 0, T, {sc + b.E16[0], xH}, 2, le, 0, xH, ctH, slope, 0);
  }
  // gh_s = d_{s-1} Whh^T + b_hh: reads the d-part of slab s, first needed by the GRU link's epilogue
  lin(b.CP16, xCP, nCP, p.whh, R, w->gru_bhh, 3 * ctR, DF_RM_SC1 | DF_GENTLE | ((pchain_tune() & 16) ? DF_CANARY : 0), sc + b.GHb, s3R, 3 * R, 0, 0, 0, r_main,
      r_side);
  {  // d_s = GRU(enc_s, d_{s-1})
    Operands o;
    o.p[GRU_X16] = {sc + b.ENC16, xH}; o.p[GRU_WIH] = sc + p.wih; o.p[GRU_GH] = {sc + b.GHb, s3R}; o.p[GRU_HPREV] = {sc + b.DS, sR}; o.p[GRU_HRM] = {sc + b.DS + sR, sR};
    o.p[GRU_H16] = {sc + b.CP16 + xCP, xCP}; o.p[GRU_RG] = o.p[GRU_UG] = o.p[GRU_NG] = sc + b.dummyR; o.p[GRU_BIH] = w->gru_bih;
    o.p[GRU_H16B] = {sc + b.DC16 + (size_t)ctZ * 256, xDC}; o.ld[GRU_LD_HPREV] = R; o.ld[LD_OUT] = R; o.n16[N16_OUT] = nCP; o.n16[N16_OUTB] = nDC; o.i[GRU_I_R] = R;
    add_desc(bld, K_GRU, ctR, 0, range_for(ctR * rt, r_main), H, 0, 0, T, o);
  }
  // prior(cat[d_s, z_{s-1}])
  lin(b.CP16 + xCP, xCP, nCP, p.prior[0], R + Z, c->prior_b[0], ctH, DF_RELU, nullptr, 0, 0, b.P16[0], xH, ctH, 0, rH);
  {  // the next two prior layers: one descriptor (K_LINSEQ)
    const SeqLink lp[2] = {{sc + p.prior[1], c->prior_b[1], nullptr, 0, 0, sc + b.P16[1]}, {sc + p.prior[2], c->prior_b[2], nullptr, 0, 0, sc + b.P16[2]}};
    add_linseq(bld, ctH, 0, rH, H, true, false, 0, T, {sc + b.P16[0], xH}, 2, lp, 0, xH, ctH, slope, 0);
  }
  {  // z_s ~ prior: into the decoder input and into the NEXT step's prior input
    Operands o;
    o.p[HEAD_P16] = o.p[HEAD_Q16] = {sc + b.P16[2], xH}; o.p[HEAD_WP] = o.p[HEAD_WQ] = sc + p.prior_h; o.p[HEAD_BP] = o.p[HEAD_BQ] = c->prior_hb;
    o.p[HEAD_EPS] = {eps, sZ}; o.p[HEAD_MU_P] = o.p[HEAD_SD_P] = o.p[HEAD_MU_Q] = o.p[HEAD_SD_Q] = o.p[HEAD_RAW_P] = o.p[HEAD_RAW_Q] = sc + b.dummyZ;
    o.p[HEAD_Z] = {sc + b.ZS, sZ}; o.p[HEAD_Z16] = {sc + b.DC16, xDC}; o.p[HEAD_Z16B] = {sc + b.CP16 + 2 * xCP + (size_t)ctR * 256, xCP}; o.ld[LD_OUT] = Z;
    o.n16[N16_OUT] = nDC; o.n16[N16_OUTB] = nCP; o.i[HEAD_I_Z] = Z; o.i[HEAD_I_RESIDUAL] = 3; o.f[HEAD_F_BETA] = beta; o.f[HEAD_F_INV_BETA] = 1.f / beta;
    o.f[HEAD_F_SD_EPS] = sd_eps;
    add_desc(bld, K_HEAD, ctZ, 0, range_for(ctZ * rt, r_main), H, 0, 0, T, o);
  }
  // decoder(cat[z_s, d_s]); the last layer (S * F columns) on every workgroup
  lin(b.DC16, xDC, nDC, p.dec[0], Z + R, w->dec_b[0], ctH, DF_RELU, nullptr, 0, 0, b.D16[0], xH, ctH, 0, rH);
  lin(b.D16[0], xH, ctH, p.dec[1], H, w->dec_b[1], ctH, DF_RELU, nullptr, 0, 0, b.D16[1], xH, ctH, 0, rH);
  lin(b.D16[1], xH, ctH, p.dec[2], H, sp.padded() ? sc + p.dec_b2 : w->dec_b[2], Np / 16, DF_RELU | DF_RM_SC1, sc + b.DEC, sF, Np, 0, 0, 0, 0, range_for(Np / 16 * rt, cus));
  {  // per sample: head Linear -> DMoL draw -> x_{s+1}
    Operands o;
    o.p[DMOLS_DEC] = {sc + b.DEC, sF}; o.p[DMOLS_W] = w->lik_w; o.p[DMOLS_B] = w->lik_b; o.p[DMOLS_U] = {u, (long)B * S * SD_K}; o.p[DMOLS_V] = {v, (long)B * S};
    o.p[DMOLS_X] = {x_out, S}; o.p[DMOLS_X16] = {sc + b.X16 + xS, xS}; o.ld[DMOLS_LD_DEC] = Np; o.ld[LD_OUT] = T * S; o.n16[N16_OUT] = ctS; o.i[DMOLS_I_S] = S;
    o.i[DMOLS_I_F] = SD_F; o.i[DMOLS_I_NMIX] = SD_K; o.f[DMOLS_F_LOG_EPS] = log_eps;
    add_desc(bld, K_DMOLS, Sp / 4, 0, range_for(Sp / 4 * rt, r_main), 16, 0, 0, T, o);
  }
  // sentinel-fill everything the launch polls, then the initial frame stack and states
  BLVM_HIP(pchain_fill_sentinel(sc + b.X16, sizeof(float) * (b.ZS - b.X16), s));
  BLVM_TRY(pchain_rows_to_t16(x0, S, B, Sp, sc + b.X16, s, 0, S));
  BLVM_TRY(pchain_rows_to_t16(d0, R, B, R, sc + b.CP16, s, nCP));
  BLVM_TRY(pchain_rows_to_t16(z0, Z, B, Z, sc + b.CP16 + xCP + (size_t)ctR * 256, s, nCP));
  BLVM_HIP(copy_or_zero(sc + b.DS, d0, sizeof(float) * (size_t)B * R, s));
  BLVM_TRY(pchain_launch(bld, "srnn_generate", s));
  if (d_out) BLVM_HIP(hipMemcpyAsync(d_out, sc + b.DS + (size_t)T * sR, sizeof(float) * (size_t)B * R, hipMemcpyDeviceToDevice, s));
  if (z_out) BLVM_HIP(hipMemcpyAsync(z_out, sc + b.ZS, sizeof(float) * (size_t)T * B * Z, hipMemcpyDeviceToDevice, s));
  return BLVM_OK;
}
