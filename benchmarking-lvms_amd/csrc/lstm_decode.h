// lstm_decode.h — the host arithmetic of the LSTMAudio roll-out (lstm_decode.hip) shared with its host test
// (tests/host/lstm_decode_plan_test.hip): where every buffer of the launch lies in the caller's scratch, what the host writes there
// before the launch, and the step program itself.  Nothing here touches a device: the operand type and the CU count are arguments.
#pragma once
#include <algorithm>
#include <vector>

#include "blvm_hip.h"
#include "pchain.h"

namespace blvm {
namespace pchain {

constexpr int LD_F = 30, LD_K = 10;    // DMoL head: 3 * num_mix parameters per sample
constexpr int kLstmDecodeMaxLayers = 8;  // 6 + 2 per layer descriptors of kMaxDesc

// a piece of the scratch, in floats from its base (the layouts below list theirs in ascending order)
struct LstmDecodeRegion {
  const char* name;
  size_t off, floats;
};

// T16 weight copies at the front of the scratch.  S % 16 != 0 (stack_pad, pchain.h): emb0 is [H, Sp] and dec2 [Np, H], packed from
// zero-padded row-major copies staged behind them (st_emb0, st_dec2), and the last decoder layer reads the zero-padded bias dec_b2.
struct LstmDecodePack {
  size_t emb[3], wih[kLstmDecodeMaxLayers], whh[kLstmDecodeMaxLayers], dec[3], st_emb0, st_dec2, dec_b2, total;
  std::vector<LstmDecodeRegion> regions;
};
inline LstmDecodePack lstm_decode_pack_layout(int S, int H, int L) {
  LstmDecodePack p{};
  Arena ar;
  auto take = [&](const char* name, size_t n) { const size_t at = ar.take_off(n); p.regions.push_back({name, at, n}); return at; };
  const StackPad sp = stack_pad(S, LD_F);
  p.emb[0] = take("emb0", (size_t)H * sp.Sp); p.emb[1] = take("emb1", (size_t)H * H); p.emb[2] = take("emb2", (size_t)H * H);
  for (int l = 0; l < L; ++l) { p.wih[l] = take("wih", (size_t)4 * H * H); p.whh[l] = take("whh", (size_t)4 * H * H); }
  p.dec[0] = take("dec0", (size_t)H * H); p.dec[1] = take("dec1", (size_t)H * H); p.dec[2] = take("dec2", (size_t)sp.Np * H);
  if (sp.padded()) { p.st_emb0 = take("st_emb0", sp.stage_in(H)); p.st_dec2 = take("st_dec2", sp.stage_dec(H)); p.dec_b2 = take("dec_b2", sp.stage_bias()); }
  p.total = ar.floats();
  return p;
}

// One slab per step of every activation, offsets in floats from the scratch base.  [X16, polled_end) is what the launch polls (the
// host fills it with sentinels); HS and CS are written and read with plain accesses.
//   X16    T+1 slabs [rows,Sp] T16: slab 0 = x0, slab s+1 = the stack drawn in step s (the embedding's operand of step s+1); the
//          columns S..Sp-1 (Sp = 16 ceil(S/16)) are zeros: slab 0's from the prefill, the others' from the draw link, every step
//   E16    the embedding's three layers, T slabs [rows,H] T16 each (E16[2]: layer 0's input)
//   HP16   per layer, T+1 slabs [rows,H] T16: slab s = h_{s-1}, the operand of step s's hidden projection (slab 0 = h0)
//   HN16   per layer, T slabs [rows,H] T16: h_s, the operand of the layer above or of the decoder
//   GH     per layer, T slabs [B,4H] row-major: h_{s-1} Whh^T + b_hh (polled words)
//   D16    the decoder's first two layers, T slabs [rows,H] T16 each;  DEC  T slabs [B,Np] row-major (polled words;
//          Np = S*30 rounded up to 16 when S % 16 != 0, a padded leading dimension: the last layer writes zeros into the pad columns)
//   HS     per layer, T slabs [B,H] row-major h_s;  CS  per layer, T+1 slabs [B,H]: slab s = c_{s-1} (slab 0 = c0)
struct LstmDecodeBufs {
  size_t X16, E16[3], HP16[kLstmDecodeMaxLayers], HN16[kLstmDecodeMaxLayers], GH[kLstmDecodeMaxLayers], D16[2], DEC, polled_end;
  size_t HS[kLstmDecodeMaxLayers], CS[kLstmDecodeMaxLayers], end;
  std::vector<LstmDecodeRegion> regions;
};
inline LstmDecodeBufs lstm_decode_layout(size_t base, int T, int B, int S, int H, int L) {
  LstmDecodeBufs b{};
  Arena ar{nullptr, base};
  auto take = [&](const char* name, size_t n) { const size_t at = ar.take_off(n); b.regions.push_back({name, at, n}); return at; };
  const size_t rows = (size_t)((B + 15) / 16) * 16, m = (size_t)T * rows;
  const StackPad sp = stack_pad(S, LD_F);
  b.X16 = take("X16", (m + rows) * sp.Sp);
  b.E16[0] = take("E16.0", m * H); b.E16[1] = take("E16.1", m * H); b.E16[2] = take("E16.2", m * H);
  for (int l = 0; l < L; ++l) {
    b.HP16[l] = take("HP16", (m + rows) * H);
    b.HN16[l] = take("HN16", m * H);
    b.GH[l] = take("GH", (size_t)T * B * 4 * H);
  }
  b.D16[0] = take("D16.0", m * H); b.D16[1] = take("D16.1", m * H);
  b.DEC = take("DEC", (size_t)T * B * sp.Np);
  b.polled_end = ar.floats();
  for (int l = 0; l < L; ++l) {
    b.HS[l] = take("HS", (size_t)T * B * H);
    b.CS[l] = take("CS", (size_t)(T + 1) * B * H);
  }
  b.end = ar.floats();
  return b;
}

// what the host writes into the scratch between the sentinel fill and the launch: the rows of `src` (null: zeros) as a T16 slab or
// row-major at `off`; the source has src_cols <= cols columns, the rest of a row is zeros (the padded frame stack)
struct LstmDecodePrefill {
  enum Src { X0, H0, C0 } src;
  int layer;   // of h0 / c0 ([L,B,H])
  bool t16;
  size_t off;
  int cols, src_cols;
};
inline std::vector<LstmDecodePrefill> lstm_decode_prefills(const LstmDecodeBufs& b, int S, int H, int L) {
  std::vector<LstmDecodePrefill> v;
  v.push_back({LstmDecodePrefill::X0, 0, true, b.X16, stack_pad(S, LD_F).Sp, S});
  for (int l = 0; l < L; ++l) {
    v.push_back({LstmDecodePrefill::H0, l, true, b.HP16[l], H, H});
    v.push_back({LstmDecodePrefill::C0, l, false, b.CS[l], H, H});
  }
  return v;
}

// The step program: per step s, 6 + 2 L links
//   embedding: K_LIN, K_LINSEQ x2 (ReLU)                                   X16[s] -> E16[0..2][s]
//   per layer: K_LIN  gh = h_{s-1} Whh^T + b_hh on the side range (gentle)  HP16[l][s] -> GH[l][s]
//              K_LSTM                                                       E16[2][s] | HN16[l-1][s], GH[l][s], CS[l][s] -> HN16[l][s], HP16[l][s+1], HS[l][s], CS[l][s+1]
//   decoder:   K_LIN x3 (ReLU), the last Np columns wide, row-major         HN16[L-1][s] -> D16[0..1][s] -> DEC[s]
//   K_DMOLS: head Linear + draw per sample, Sp / 4 tiles                    DEC[s] -> x_out[:, s], X16[s+1] (pad columns included)
// `sc`: the scratch base; `cus`: CUs of the device (at least 32); ot: the operand type of the packed weights.
inline void lstm_decode_program(Builder& bld, int ot, int cus_all, const BlvmLstmDecodeWeights* w, const LstmDecodePack& p, const LstmDecodeBufs& b, float* sc,
                                const float* u, const float* v, float* x_out, int T, int B, int S, int H, int L, float log_eps) {
  const StackPad sp = stack_pad(S, LD_F);
  const int Sp = sp.Sp, Np = sp.Np;
  const int rt = (B + 15) / 16, ctS = Sp / 16, ctH = H / 16, cus = cus_all & ~7;
  const long rows = (long)rt * 16, xS = rows * Sp, xH = rows * H;
  const long sH = (long)B * H, s4H = 4 * sH, sF = (long)B * Np;
  const int r_side = range_for(4 * ctH * rt, std::min(cus / 4, 64));  // the hidden projections of the NEXT step: off the critical path
  const int r_main = cus - r_side;
  bld.begin(ot, T, B, 4, false, r_main);
  auto lin = [&](size_t A16, long a_step, size_t W, int K, const float* bias, int ct, int flags, size_t orm, long rm_step, int ldo, size_t o16, int wg0, int nwg) {
    Operands o;
    o.p[LIN_A] = {sc + A16, a_step}; o.p[LIN_W] = sc + W; o.p[LIN_BIAS] = bias; o.p[LIN_ORM] = {orm ? sc + orm : nullptr, rm_step};
    o.p[LIN_O16] = {o16 ? sc + o16 : nullptr, xH}; o.ld[LIN_LD_A] = K; o.ld[LD_OUT] = ldo; o.n16[N16_OUT] = ctH; o.f[LIN_F_SLOPE] = 0.f;
    add_desc(bld, K_LIN, ct, wg0, nwg, K, flags, 0, T, o);
  };
  const int rH = range_for(ctH * rt, r_main);
  lin(b.X16, xS, p.emb[0], Sp, w->emb_b[0], ctH, DF_RELU, 0, 0, 0, b.E16[0], 0, rH);
  {
    const SeqLink le[2] = {{sc + p.emb[1], w->emb_b[1], nullptr, 0, 0, sc + b.E16[1]}, {sc + p.emb[2], w->emb_b[2], nullptr, 0, 0, sc + b.E16[2]}};
    add_linseq(bld, ctH, 0, rH, H, true, false, 0, T, {sc + b.E16[0], xH}, 2, le, 0, xH, ctH, 0.f, 0);
  }
  for (int l = 0; l < L; ++l) {
    lin(b.HP16[l], xH, p.whh[l], H, w->bhh[l], 4 * ctH, DF_RM_SC1 | DF_GENTLE, b.GH[l], s4H, 4 * H, 0, r_main, r_side);
    Operands o;
    o.p[LSTM_X16] = {sc + (l == 0 ? b.E16[2] : b.HN16[l - 1]), xH}; o.p[LSTM_WIH] = sc + p.wih[l]; o.p[LSTM_BIH] = w->bih[l]; o.p[LSTM_GH] = {sc + b.GH[l], s4H};
    o.p[LSTM_CPREV] = {sc + b.CS[l], sH}; o.p[LSTM_CNEXT] = {sc + b.CS[l] + sH, sH}; o.p[LSTM_HRM] = {sc + b.HS[l], sH}; o.p[LSTM_H16] = {sc + b.HN16[l], xH};
    o.p[LSTM_H16B] = {sc + b.HP16[l] + xH, xH}; o.ld[LD_OUT] = H; o.n16[N16_OUT] = ctH; o.n16[N16_OUTB] = ctH; o.i[LSTM_I_H] = H;
    add_desc(bld, K_LSTM, ctH, 0, rH, H, 0, 0, T, o);
  }
  lin(b.HN16[L - 1], xH, p.dec[0], H, w->dec_b[0], ctH, DF_RELU, 0, 0, 0, b.D16[0], 0, rH);
  lin(b.D16[0], xH, p.dec[1], H, w->dec_b[1], ctH, DF_RELU, 0, 0, 0, b.D16[1], 0, rH);
  lin(b.D16[1], xH, p.dec[2], H, sp.padded() ? sc + p.dec_b2 : w->dec_b[2], Np / 16, DF_RELU | DF_RM_SC1, b.DEC, sF, Np, 0, 0, range_for(Np / 16 * rt, cus));
  {
    Operands o;
    o.p[DMOLS_DEC] = {sc + b.DEC, sF}; o.p[DMOLS_W] = w->lik_w; o.p[DMOLS_B] = w->lik_b; o.p[DMOLS_U] = {u, (long)B * S * LD_K}; o.p[DMOLS_V] = {v, (long)B * S};
    o.p[DMOLS_X] = {x_out, S}; o.p[DMOLS_X16] = {sc + b.X16 + xS, xS}; o.ld[DMOLS_LD_DEC] = Np; o.ld[LD_OUT] = T * S; o.n16[N16_OUT] = ctS; o.i[DMOLS_I_S] = S;
    o.i[DMOLS_I_F] = LD_F; o.i[DMOLS_I_NMIX] = LD_K; o.f[DMOLS_F_LOG_EPS] = log_eps;
    add_desc(bld, K_DMOLS, Sp / 4, 0, range_for(Sp / 4 * rt, r_main), 16, 0, 0, T, o);
  }
}

}  // namespace pchain
}  // namespace blvm
