// lstm_decode.h — the LSTMAudio roll-out (lstm_decode.hip) on the shared host plan (rollout_plan.h): its pack table, where every buffer
// of the launch lies in the caller's scratch, what the host writes there before the launch, and the step program.  Read by the host
// tests too (tests/host/lstm_decode_plan_test.hip, lstm_decode_ragged_plan_test.hip).  Nothing here touches a device.
#pragma once
#include "rollout_plan.h"

namespace blvm {
namespace pchain {

constexpr int kLstmDecodeMaxLayers = 8;  // 6 + 2 per layer descriptors of kMaxDesc

// emb[0..2], then per layer wih, whh, then dec[0..2]
inline int lp_emb(int i) { return i; }
inline int lp_wih(int l) { return 3 + 2 * l; }
inline int lp_whh(int l) { return 4 + 2 * l; }
inline int lp_dec(int L, int i) { return 3 + 2 * L + i; }
inline PackTable lstm_pack_table(const BlvmLstmDecodeWeights& w, int S, int H, int L) {
  const StackPad sp = stack_pad(S, kDmolF);
  std::vector<PackEntry> e = {{"emb0", w.emb_w[0], sp.Sp, H, sp.Sp}, {"emb1", w.emb_w[1], H, H, H}, {"emb2", w.emb_w[2], H, H, H}};
  for (int l = 0; l < L; ++l) {
    e.push_back({"wih", w.wih ? w.wih[l] : nullptr, H, 4 * H, H});
    e.push_back({"whh", w.whh ? w.whh[l] : nullptr, H, 4 * H, H});
  }
  e.insert(e.end(), {{"dec0", w.dec_w[0], H, H, H}, {"dec1", w.dec_w[1], H, H, H}, {"dec2", w.dec_w[2], H, sp.Np, H}});
  return pack_table(sp, std::move(e), lp_emb(0), lp_dec(L, 2), w.dec_b[2]);
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
  std::vector<Region> regions;
};
inline LstmDecodeBufs lstm_decode_layout(size_t base, int T, int B, int S, int H, int L) {
  LstmDecodeBufs b{};
  RegionArena ar(base);
  const size_t rows = (size_t)((B + 15) / 16) * 16, m = (size_t)T * rows;
  const StackPad sp = stack_pad(S, kDmolF);
  b.X16 = ar.take("X16", (m + rows) * sp.Sp);
  b.E16[0] = ar.take("E16.0", m * H); b.E16[1] = ar.take("E16.1", m * H); b.E16[2] = ar.take("E16.2", m * H);
  for (int l = 0; l < L; ++l) {
    b.HP16[l] = ar.take("HP16", (m + rows) * H);
    b.HN16[l] = ar.take("HN16", m * H);
    b.GH[l] = ar.take("GH", (size_t)T * B * 4 * H);
  }
  b.D16[0] = ar.take("D16.0", m * H); b.D16[1] = ar.take("D16.1", m * H);
  b.DEC = ar.take("DEC", (size_t)T * B * sp.Np);
  b.polled_end = ar.floats();
  for (int l = 0; l < L; ++l) {
    b.HS[l] = ar.take("HS", (size_t)T * B * H);
    b.CS[l] = ar.take("CS", (size_t)(T + 1) * B * H);
  }
  b.end = ar.floats();
  b.regions = std::move(ar.regions);
  return b;
}
enum LstmSrc : int { LS_X0, LS_H0, LS_C0 };  // h0, c0: [L,B,H]
inline std::vector<Prefill> lstm_decode_prefills(const LstmDecodeBufs& b, int B, int S, int H, int L) {
  std::vector<Prefill> v = {{LS_X0, 0, true, b.X16, stack_pad(S, kDmolF).Sp, S, 0}};
  for (int l = 0; l < L; ++l) {
    v.push_back({LS_H0, (size_t)l * B * H, true, b.HP16[l], H, H, 0});
    v.push_back({LS_C0, (size_t)l * B * H, false, b.CS[l], H, H, 0});
  }
  return v;
}

// The step program: per step s, 6 + 2 L links
//   embedding: K_LIN, K_LINSEQ x2 (ReLU)                                   X16[s] -> E16[0..2][s]
//   per layer: K_LIN  gh = h_{s-1} Whh^T + b_hh on the side range (gentle)  HP16[l][s] -> GH[l][s]
//              K_LSTM                                                       E16[2][s] | HN16[l-1][s], GH[l][s], CS[l][s] -> HN16[l][s], HP16[l][s+1], HS[l][s], CS[l][s+1]
//   decoder:   K_LIN x2 (ReLU), the tail                                    HN16[L-1][s] -> D16[0..1][s] -> DEC[s] -> x_out[:, s], X16[s+1]
// `sc`: the scratch base; `cus_all`: CUs of the device (at least 32); ot: the operand type of the packed weights.
// Every K_LIN of this program has slope 0 (plain ReLU), ld[LIN_LD_A] = K and n16[N16_OUT] = H / 16, whether or not it has a T16
// output; its hidden projections take no canary flag.
inline void lstm_decode_program(Builder& bld, int ot, int cus_all, const BlvmLstmDecodeWeights* w, const PackTable& p, const LstmDecodeBufs& b, float* sc,
                                const float* u, const float* v, float* x_out, int T, int B, int S, int H, int L, float log_eps) {
  const int ctH = H / 16;
  const Deal d = deal(T, B, H, cus_all, 4 * ctH * ((B + 15) / 16));
  const long xS = d.rows * p.sp.Sp, xH = d.xH, sH = (long)B * H, s4H = 4 * sH;
  bld.begin(ot, T, B, 4, false, d.r_main);
  auto W = [&](int i) { return sc + p.off(i); };
  add_mlp3(bld, d, {.A = {sc + b.X16, xS}, .K = p.sp.Sp, .W = {W(lp_emb(0)), W(lp_emb(1)), W(lp_emb(2))}, .bias = {w->emb_b[0], w->emb_b[1], w->emb_b[2]},
                    .out = {sc + b.E16[0], sc + b.E16[1], sc + b.E16[2]}, .slope = 0.f});
  for (int l = 0; l < L; ++l) {
    add_lin(bld, T, {.A = {sc + b.HP16[l], xH}, .ld_a = H, .W = W(lp_whh(l)), .bias = w->bhh[l], .K = H, .ct = 4 * ctH, .flags = DF_RM_SC1 | DF_GENTLE,
                     .orm = {sc + b.GH[l], s4H}, .ldo = 4 * H, .n16 = ctH, .wg0 = d.r_main, .nwg = d.r_side});
    Operands o;
    o.p[LSTM_X16] = {sc + (l == 0 ? b.E16[2] : b.HN16[l - 1]), xH}; o.p[LSTM_WIH] = W(lp_wih(l)); o.p[LSTM_BIH] = w->bih[l]; o.p[LSTM_GH] = {sc + b.GH[l], s4H};
    o.p[LSTM_CPREV] = {sc + b.CS[l], sH}; o.p[LSTM_CNEXT] = {sc + b.CS[l] + sH, sH}; o.p[LSTM_HRM] = {sc + b.HS[l], sH}; o.p[LSTM_H16] = {sc + b.HN16[l], xH};
    o.p[LSTM_H16B] = {sc + b.HP16[l] + xH, xH}; o.ld[LD_OUT] = H; o.n16[N16_OUT] = ctH; o.n16[N16_OUTB] = ctH; o.i[LSTM_I_H] = H;
    add_desc(bld, K_LSTM, ctH, 0, d.rH, H, 0, 0, T, o);
  }
  for (int i = 0; i < 2; ++i)
    add_lin(bld, T, {.A = {sc + (i == 0 ? b.HN16[L - 1] : b.D16[0]), xH}, .ld_a = H, .W = W(lp_dec(L, i)), .bias = w->dec_b[i], .K = H, .ct = ctH, .flags = DF_RELU,
                     .o16 = {sc + b.D16[i], xH}, .n16 = ctH, .nwg = d.rH});
  add_tail(bld, d, p.sp, {.D16 = sc + b.D16[1], .ld_a = H, .n16 = ctH, .W = W(lp_dec(L, 2)), .bias = p.bias, .slope = 0.f, .DEC = sc + b.DEC, .X16 = sc + b.X16,
                          .lik_w = w->lik_w, .lik_b = w->lik_b, .u = u, .v = v, .x_out = x_out, .log_eps = log_eps});
}

}  // namespace pchain
}  // namespace blvm
