// rollout_plan.h — the host arithmetic of the one-launch roll-outs (vrnn_decode.hip, srnn_decode.hip, lstm_decode.hip) shared with
// their host tests (tests/host/*_plan_test.hip) and tools/dump_rollout_program.hip: which weights are packed where, where every buffer
// of a launch lies in the caller's scratch, what the host writes there before the launch, and the step programs themselves.  The parts
// the three models share exist once; the VRNN and SRNN models follow below, the LSTM's are in lstm_decode.h.  Nothing here touches a
// device: the operand type, the CU count and the tune bits (common.h pchain_tune) are arguments.
#pragma once
#include <algorithm>
#include <vector>

#include "blvm_hip.h"
#include "pchain.h"

namespace blvm {
namespace pchain {

constexpr int kDmolF = 30, kDmolK = 10;  // DMoL head: 3 * num_mix parameters per sample, num_mix
// The head of the draw tile as the plans see it (pchain.h dmols_draw): F head inputs per sample (the last decoder layer is S F wide,
// the head Linear [F,F]), K pick draws per sample (the u stream; 0: none).  The default is the DMoL head of every program so far.
struct DrawPlan { int kind = DRAW_DMOL, F = kDmolF, K = kDmolK; float sd_beta = 0.f, sd_eps = 0.f; };
// A caller's head (the five scalars of blvm_hip.h), checked: null and *dp unless it is one the tile does not draw — the kind
// unknown, another count than 10 components where there is a pick, a negative sd_beta.
inline const char* draw_plan(int kind, int num_mix, float sd_beta, float sd_eps, DrawPlan* dp) {
  if (kind != DRAW_DMOL && kind != DRAW_GMM && kind != DRAW_GAUSS) return "unknown head kind (0 DMoL, 1 GMM, 2 Gaussian)";
  if (kind != DRAW_GAUSS && num_mix != kDmolK) return "the mixture heads have 10 components";
  if (!(sd_beta >= 0.f)) return "head_sd_beta must not be negative";
  if (kind == DRAW_GAUSS) *dp = DrawPlan{DRAW_GAUSS, 2, 0, sd_beta, sd_eps};
  else if (kind == DRAW_GMM) *dp = DrawPlan{DRAW_GMM, kDmolF, kDmolK, sd_beta, sd_eps};
  else *dp = DrawPlan{};
  return nullptr;
}
// the u and v streams a head takes: a pick's u comes with v (both null: the mode), the Gaussian head has no u
inline bool draw_streams_ok(const DrawPlan& dp, const float* u, const float* v) { return dp.K > 0 ? (u == nullptr) == (v == nullptr) : u == nullptr; }

// a piece of the scratch, in floats from its base, and an arena that records the pieces it hands out (in ascending order)
struct Region { const char* name; size_t off, floats; };
struct RegionArena {
  Arena ar;
  std::vector<Region> regions;
  explicit RegionArena(size_t base = 0) : ar{nullptr, base} {}
  size_t take(const char* name, size_t n) { const size_t at = ar.take_off(n); regions.push_back({name, at, n}); return at; }
  size_t floats() const { return ar.floats(); }
};

// one T16 weight copy: rows [rows, k] of src (row stride ld) packed at scratch + off
struct PackEntry { const char* name; const float* src; int ld, rows, k; size_t off; };
// The T16 weight copies at the front of the scratch, as data: offsets (rows * k floats each, in table order), the total and the pack
// calls (rollout_launch.h stage_and_pack) all come from `e`.  S % 16 != 0 (pchain.h stack_pad): the first layer [H, Sp] and the last decoder
// layer [Np, H] are packed from zero-padded row-major copies staged behind the packs (stage_in, stage_dec) and
// the last decoder layer reads the zero-padded bias stage_bias.
struct PackTable {
  StackPad sp;
  std::vector<PackEntry> e;
  int first = 0, last = 0;      // the entries of the first layer (K = Sp) and of the last decoder layer (rows = Np)
  const float* bias = nullptr;  // the last decoder layer's bias
  size_t stage_in = 0, stage_dec = 0, stage_bias = 0, total = 0;
  std::vector<Region> regions;
  size_t off(int i) const { return e[i].off; }
  // after the staging copies are enqueued (or on the host, where nothing is copied): the two packs and the bias read them
  void use_staged(float* sc) {
    if (sp.padded()) { e[first].src = sc + stage_in; e[last].src = sc + stage_dec; bias = sc + stage_bias; }
  }
};
inline PackTable pack_table(const StackPad& sp, std::vector<PackEntry> e, int first, int last, const float* bias) {
  PackTable t{sp, std::move(e), first, last, bias};
  RegionArena ar;
  for (PackEntry& p : t.e) p.off = ar.take(p.name, (size_t)p.rows * p.k);
  if (sp.padded()) {
    t.stage_in = ar.take("stage_in", sp.stage_in(t.e[first].rows));
    t.stage_dec = ar.take("stage_dec", sp.stage_dec(t.e[last].k));
    t.stage_bias = ar.take("stage_bias", sp.stage_bias());
  }
  t.total = ar.floats();
  t.regions = std::move(ar.regions);
  return t;
}

// what the host writes into the scratch between the sentinel fill and the launch: B rows of srcs[src] + src_off (a null source: zeros) as
// a T16 slab of n16 blocks per row tile (a part of a concatenated slab when n16 > cols / 16; 0: cols / 16) or row-major at `off`; the
// source has src_cols <= cols columns, the rest of a row is zeros (the padded frame stack)
struct Prefill { int src; size_t src_off; bool t16; size_t off; int cols, src_cols, n16; };  // src: X0, then the model's states

// out = leaky(A W^T + bias): A a polled T16 slab, outputs row-major (polled words) and / or one or two T16 slabs
struct Lin {
  Ptr A; int ld_a = 0;  // ld[LIN_LD_A]: A's width where the model states it (0: K)
  const float *W = nullptr, *bias = nullptr; int K = 0, ct = 0, flags = 0; float slope = 0.f;
  Ptr orm; int ldo = 0; Ptr o16; int n16 = 0; Ptr o16b; int n16b = 0; int wg0 = 0, nwg = 0;
};
inline Desc& add_lin(Builder& bld, int T, const Lin& l) {
  Operands o;
  o.p[LIN_A] = l.A; o.p[LIN_W] = l.W; o.p[LIN_BIAS] = l.bias; o.p[LIN_ORM] = l.orm; o.p[LIN_O16] = l.o16; o.p[LIN_O16B] = l.o16b;
  o.ld[LIN_LD_A] = l.ld_a; o.ld[LD_OUT] = l.ldo; o.n16[N16_OUT] = l.n16; o.n16[N16_OUTB] = l.n16b; o.f[LIN_F_SLOPE] = l.slope;
  return add_desc(bld, K_LIN, l.ct, l.wg0, l.nwg, l.K, l.flags, 0, T, o);
}

// what every step program is dealt over: rt row tiles of B utterances, ctH column tiles of an H-wide layer on rH workgroups of the
// main range [0, r_main), the side range [r_main, r_main + r_side) for the hidden projection of the NEXT step, `cus` for the wide layer
struct Deal {
  int T, B, H, rt, ctH, cus, r_side, r_main, rH;
  long rows, xH;  // rows of a T16 slab, floats of an [rows, H] slab
};
// side_tiles: column tiles x row tiles of the hidden projection
inline Deal deal(int T, int B, int H, int cus_all, int side_tiles) {
  Deal d{T, B, H, (B + 15) / 16, H / 16, cus_all & ~7};
  d.r_side = range_for(side_tiles, std::min(d.cus / 4, 64));
  d.r_main = d.cus - d.r_side;
  d.rH = range_for(d.ctH * d.rt, d.r_main);
  d.rows = (long)d.rt * 16; d.xH = d.rows * H;
  return d;
}

// a three-layer front (an embedding, an encoder, a prior MLP): K_LIN over A [rows, K], then the two H-wide layers as ONE K_LINSEQ;
// out[i]: T slabs [rows, H] T16 of layer i
struct Mlp3 { Ptr A; int K; const float *W[3], *bias[3]; float* out[3]; float slope; };
inline void add_mlp3(Builder& bld, const Deal& d, const Mlp3& m) {
  add_lin(bld, d.T, {.A = m.A, .ld_a = m.K, .W = m.W[0], .bias = m.bias[0], .K = m.K, .ct = d.ctH, .flags = DF_RELU, .slope = m.slope, .o16 = {m.out[0], d.xH},
                     .n16 = d.ctH, .nwg = d.rH});
  const SeqLink l[2] = {{m.W[1], m.bias[1], nullptr, 0, 0, m.out[1]}, {m.W[2], m.bias[2], nullptr, 0, 0, m.out[2]}};
  add_linseq(bld, d.ctH, 0, d.rH, d.H, true, false, 0, d.T, {m.out[0], d.xH}, 2, l, 0, d.xH, d.ctH, m.slope, 0);
}

// the tail of every step: the last decoder layer (Np / 16 column tiles on every workgroup, row-major polled words, the padded bias),
// then K_DMOLS: head Linear + draw per sample, Sp / 4 tiles                  D16 -> DEC[s] -> x_out[:, s], X16[s+1] (pad columns included)
struct Tail {
  const float* D16;  // the operand: T slabs [rows, H] T16
  int ld_a, n16;     // the last layer's ld[LIN_LD_A] and n16[N16_OUT], as each model states them (neither is read: A is H wide, no T16 output)
  const float *W, *bias; float slope; float *DEC, *X16; const float *lik_w, *lik_b, *u, *v; float* x_out; float log_eps;
  DrawPlan head = {};  // (sp is stack_pad(S, head.F))
};
inline void add_tail(Builder& bld, const Deal& d, const StackPad& sp, const Tail& t) {
  const int S = sp.S, Sp = sp.Sp, Np = sp.Np;
  const long sF = (long)d.B * Np, xS = d.rows * Sp;
  add_lin(bld, d.T, {.A = {t.D16, d.xH}, .ld_a = t.ld_a, .W = t.W, .bias = t.bias, .K = d.H, .ct = Np / 16, .flags = DF_RELU | DF_RM_SC1, .slope = t.slope,
                     .orm = {t.DEC, sF}, .ldo = Np, .n16 = t.n16, .nwg = range_for(Np / 16 * d.rt, d.cus)});
  Operands o;
  o.p[DMOLS_DEC] = {t.DEC, sF}; o.p[DMOLS_W] = t.lik_w; o.p[DMOLS_B] = t.lik_b; o.p[DMOLS_U] = {t.u, (long)d.B * S * t.head.K}; o.p[DMOLS_V] = {t.v, (long)d.B * S};
  o.p[DMOLS_X] = {t.x_out, S}; o.p[DMOLS_X16] = {t.X16 + xS, xS}; o.ld[DMOLS_LD_DEC] = Np; o.ld[LD_OUT] = d.T * S; o.n16[N16_OUT] = Sp / 16; o.i[DMOLS_I_S] = S;
  o.i[DMOLS_I_F] = t.head.F; o.i[DMOLS_I_NMIX] = t.head.K; o.i[DMOLS_I_HEAD] = t.head.kind; o.f[DMOLS_F_LOG_EPS] = t.log_eps;
  o.f[DMOLS_F_SD_BETA] = t.head.sd_beta; o.f[DMOLS_F_SD_EPS] = t.head.sd_eps;
  add_desc(bld, K_DMOLS, Sp / 4, 0, range_for(Sp / 4 * d.rt, d.r_main), 16, 0, 0, d.T, o);
}

// z ~ prior (K_HEAD in generation mode: the posterior operands are the prior's; the statistics go to `dummy`)
struct PriorHead { const float *P16, *W, *bias, *eps, *dummy; Ptr z, z16; int n16 = 0; Ptr z16b; int n16b = 0; };
inline void add_prior_head(Builder& bld, const Deal& d, int Z, float sd_eps, const PriorHead& h) {
  const float beta = softplus_beta_of(sd_eps);
  Operands o;
  o.p[HEAD_P16] = o.p[HEAD_Q16] = {h.P16, d.xH}; o.p[HEAD_WP] = o.p[HEAD_WQ] = h.W; o.p[HEAD_BP] = o.p[HEAD_BQ] = h.bias;
  o.p[HEAD_EPS] = {h.eps, (long)d.B * Z}; o.p[HEAD_MU_P] = o.p[HEAD_SD_P] = o.p[HEAD_MU_Q] = o.p[HEAD_SD_Q] = o.p[HEAD_RAW_P] = o.p[HEAD_RAW_Q] = h.dummy;
  o.p[HEAD_Z] = h.z; o.p[HEAD_Z16] = h.z16; o.p[HEAD_Z16B] = h.z16b; o.ld[LD_OUT] = Z; o.n16[N16_OUT] = h.n16; o.n16[N16_OUTB] = h.n16b; o.i[HEAD_I_Z] = Z;
  o.i[HEAD_I_RESIDUAL] = 3; o.f[HEAD_F_BETA] = beta; o.f[HEAD_F_INV_BETA] = 1.f / beta; o.f[HEAD_F_SD_EPS] = sd_eps;
  add_desc(bld, K_HEAD, Z / 16, 0, range_for(Z / 16 * d.rt, d.r_main), d.H, 0, 0, d.T, o);
}

// h_s = GRU(x, h_{s-1}) (K_GRU): HS holds T + 1 row-major slabs [B, R] (slab 0 = h0, polled words), the gates go to `dummy`
struct GruCell { Ptr X16; int K; const float *Wih, *bih, *GH; float* HS; const float* dummy; Ptr h16; int n16; Ptr h16b; int n16b; };
inline void add_gru_cell(Builder& bld, const Deal& d, int R, const GruCell& g) {
  const long sR = (long)d.B * R;
  Operands o;
  o.p[GRU_X16] = g.X16; o.p[GRU_WIH] = g.Wih; o.p[GRU_GH] = {g.GH, 3 * sR}; o.p[GRU_HPREV] = {g.HS, sR}; o.p[GRU_HRM] = {g.HS + sR, sR}; o.p[GRU_H16] = g.h16;
  o.p[GRU_RG] = o.p[GRU_UG] = o.p[GRU_NG] = g.dummy; o.p[GRU_BIH] = g.bih; o.p[GRU_H16B] = g.h16b; o.ld[GRU_LD_HPREV] = R; o.ld[LD_OUT] = R;
  o.n16[N16_OUT] = g.n16; o.n16[N16_OUTB] = g.n16b; o.i[GRU_I_R] = R;
  add_desc(bld, K_GRU, R / 16, 0, range_for(R / 16 * d.rt, d.r_main), g.K, 0, 0, d.T, o);
}

// =================================================================================================================================
// VRNNAudio (vrnn_decode.hip): 17 links per step, 16 when Z == H
// =================================================================================================================================
enum VrnnPack : int { VP_ENC0, VP_ENC1, VP_ENC2, VP_PRIOR0, VP_PRIOR1, VP_PRIOR2, VP_PRIOR_H, VP_PHI0, VP_PHI1, VP_PHI2, VP_PHI3, VP_WIH, VP_WHH, VP_DEC0, VP_DEC1, VP_DEC2 };
// (both entry points: the per-CU blvm_vrnn_decode takes S % 16 == 0 only, where nothing is staged)
inline PackTable vrnn_pack_table(const BlvmVrnnDecodeWeights& w, const BlvmVrnnWeights& c, int S, int H, int Z, int R, int F = kDmolF) {
  const StackPad sp = stack_pad(S, F);
  return pack_table(sp,
                    {{"enc0", w.enc_w[0], sp.Sp, H, sp.Sp}, {"enc1", w.enc_w[1], H, H, H}, {"enc2", w.enc_w[2], H, H, H},
                     {"prior0", c.prior_w[0], R, H, R}, {"prior1", c.prior_w[1], H, H, H}, {"prior2", c.prior_w[2], H, H, H},
                     {"prior_h", c.prior_hw, H, 2 * Z, H},
                     {"phi0", c.phi_w[0], Z, H, Z}, {"phi1", c.phi_w[1], H, H, H}, {"phi2", c.phi_w[2], H, H, H}, {"phi3", c.phi_w[3], H, H, H},
                     {"wih", c.gru_wih, 2 * H, 3 * R, 2 * H}, {"whh", c.gru_whh, R, 3 * R, R},
                     {"dec0", w.dec_w[0], H + R, H, H + R}, {"dec1", w.dec_w[1], H, H, H}, {"dec2", w.dec_w[2], H, sp.Np, H}},
                    VP_ENC0, VP_DEC2, w.dec_b[2]);
}

// One slab per step of every activation, offsets in floats from the scratch base; [X16, polled_end) is what the launch polls (the host
// fills it with sentinels).  Nothing is kept for a backward pass, but every word is written once per launch.
//   X16    T+1 slabs [rows,Sp] T16: slab 0 = x0, slab s+1 = the stack drawn in step s (pad columns S..Sp-1: zeros, pchain.h stack_pad)
//   E16    the encoder's first two layers;  CAT16  cat[enc | phi] [rows,2H] T16, written in parts by enc[2] and phi[3]
//   H16    T+1 slabs [rows,R] T16: slab s = h_{s-1};  HS  T+1 slabs [B,R] row-major (polled words), slab 0 = h0
//   P16    the prior's three layers;  GHb  [B,3R] row-major: h_{s-1} Whh^T + b_hh (polled words);  Z16  z_s
//   F16    phi's first three layers;  DC16  cat[phi | h_s] [rows,H+R] T16, written in parts by phi[3] and the GRU link
//   D16    the decoder's first two layers;  DEC  [B,Np] row-major (polled words)
//   dummyZ, dummyR  where the head's statistics and the GRU's gates go: never read, the one place written more than once
struct VrnnBufs {
  size_t X16, E16[2], CAT16, H16, HS, P16[3], GHb, Z16, F16[3], DC16, D16[2], DEC, polled_end, dummyZ, dummyR, end;
  std::vector<Region> regions;
};
inline VrnnBufs vrnn_generate_layout(size_t base, int T, int B, int S, int H, int Z, int R, int F = kDmolF) {
  VrnnBufs b{};
  RegionArena ar(base);
  const size_t rows = (size_t)((B + 15) / 16) * 16, m = (size_t)T * rows, X = H;
  const StackPad sp = stack_pad(S, F);
  b.X16 = ar.take("X16", (m + rows) * sp.Sp);
  b.E16[0] = ar.take("E16.0", m * H); b.E16[1] = ar.take("E16.1", m * H);
  b.CAT16 = ar.take("CAT16", m * (X + H));
  b.H16 = ar.take("H16", (m + rows) * R);
  b.HS = ar.take("HS", (size_t)(T + 1) * B * R);
  for (int i = 0; i < 3; ++i) b.P16[i] = ar.take("P16", m * H);
  b.GHb = ar.take("GHb", (size_t)T * B * 3 * R);
  b.Z16 = ar.take("Z16", m * Z);
  for (int i = 0; i < 3; ++i) b.F16[i] = ar.take("F16", m * H);
  b.DC16 = ar.take("DC16", m * (H + R));
  b.D16[0] = ar.take("D16.0", m * H); b.D16[1] = ar.take("D16.1", m * H);
  b.DEC = ar.take("DEC", (size_t)T * B * sp.Np);
  b.polled_end = ar.floats();
  b.dummyZ = ar.take("dummyZ", (size_t)B * Z);
  b.dummyR = ar.take("dummyR", (size_t)B * R);
  b.end = ar.floats();
  b.regions = std::move(ar.regions);
  return b;
}
enum VrnnSrc : int { VS_X0, VS_H0 };
inline std::vector<Prefill> vrnn_generate_prefills(const VrnnBufs& b, int S, int R) {
  return {{VS_X0, 0, true, b.X16, stack_pad(S, kDmolF).Sp, S, 0}, {VS_H0, 0, true, b.H16, R, R, 0}, {VS_H0, 0, false, b.HS, R, R, 0}};
}

//   encoder: K_LIN x3 (leaky), the third into cat[enc | .]                  X16[s] -> E16[0..1][s] -> CAT16[s]
//   prior:   K_LIN, K_LINSEQ x2, K_HEAD                                     H16[s] -> P16[0..2][s] -> Z16[s]
//   K_LIN    gh = h_{s-1} Whh^T + b_hh on the side range (gentle)           H16[s] -> GHb[s]
//   phi:     (Z != H: K_LIN) K_LINSEQ x2 | x3, K_LIN into both cats         Z16[s] -> F16[0..2][s] -> CAT16[s], DC16[s]
//   K_GRU                                                                   CAT16[s], GHb[s], HS[s] -> HS[s+1], H16[s+1], DC16[s]
//   decoder and draw: K_LIN x2, the tail                                    DC16[s] -> D16[0..1][s] -> ...
inline void vrnn_generate_program(Builder& bld, int ot, int cus_all, int tune, const BlvmVrnnDecodeWeights* w, const PackTable& p, const VrnnBufs& b, float* sc,
                                  const float* eps, const float* u, const float* v, float* x_out, int T, int B, int S, int H, int Z, int R, float sd_eps,
                                  float slope, float log_eps, const DrawPlan& head = {}) {
  const BlvmVrnnWeights* c = w->cell;
  const int ctH = H / 16, ctR = R / 16, X = H;
  Deal d = deal(T, B, H, cus_all, 3 * ctR * ((B + 15) / 16));
  // VRNN alone narrows the main range to its widest critical link (the others keep every workgroup left of the side range)
  d.r_main = range_for(std::max(ctR * d.rt, ctH * d.rt), d.cus - d.r_side);
  d.rH = range_for(ctH * d.rt, d.r_main);
  const long xS = d.rows * p.sp.Sp, xH = d.xH, xZ = d.rows * Z, xR = d.rows * R, xC = d.rows * (X + H), xD = d.rows * (H + R);
  bld.begin(ot, T, B, 4, false, d.r_main);
  auto W = [&](int i) { return sc + p.off(i); };
  // an H-wide layer on the main range into one T16 slab (ld[LIN_LD_A] stays 0 in this program: every operand's width is its link's K)
  auto layer = [&](Ptr A, int pack, int K, const float* bias, float sl, Ptr o16, int n16) {
    return Lin{.A = A, .W = W(pack), .bias = bias, .K = K, .ct = ctH, .flags = DF_RELU, .slope = sl, .o16 = o16, .n16 = n16, .nwg = d.rH};
  };
  // encoder(x_t): three separate links (the third writes the enc part of cat[enc | phi])
  add_lin(bld, T, layer({sc + b.X16, xS}, VP_ENC0, p.sp.Sp, w->enc_b[0], slope, {sc + b.E16[0], xH}, ctH));
  add_lin(bld, T, layer({sc + b.E16[0], xH}, VP_ENC1, H, w->enc_b[1], slope, {sc + b.E16[1], xH}, ctH));
  add_lin(bld, T, layer({sc + b.E16[1], xH}, VP_ENC2, H, w->enc_b[2], slope, {sc + b.CAT16, xC}, (X + H) / 16));
  // prior(h_{t-1}) | hidden projection of the GRU (between the prior's first layer and the run of its other two; slope 0: plain ReLU
  // MLPs in the cell).  The canary bit (tune & 16) applies to this program's and the SRNN's hidden projection, not the LSTM's.
  add_lin(bld, T, layer({sc + b.H16, xR}, VP_PRIOR0, R, c->prior_b[0], 0.f, {sc + b.P16[0], xH}, ctH));
  add_lin(bld, T, {.A = {sc + b.H16, xR}, .W = W(VP_WHH), .bias = c->gru_bhh, .K = R, .ct = 3 * ctR, .flags = DF_RM_SC1 | DF_GENTLE | ((tune & 16) ? DF_CANARY : 0),
                   .orm = {sc + b.GHb, 3L * B * R}, .ldo = 3 * R, .wg0 = d.r_main, .nwg = d.r_side});
  {
    const SeqLink lp[2] = {{W(VP_PRIOR1), c->prior_b[1], nullptr, 0, 0, sc + b.P16[1]}, {W(VP_PRIOR2), c->prior_b[2], nullptr, 0, 0, sc + b.P16[2]}};
    add_linseq(bld, ctH, 0, d.rH, H, true, false, 0, T, {sc + b.P16[0], xH}, 2, lp, 0, xH, ctH, 0.f, 0);
  }
  add_prior_head(bld, d, Z, sd_eps, {.P16 = sc + b.P16[2], .W = W(VP_PRIOR_H), .bias = c->prior_hb, .eps = eps, .dummy = sc + b.dummyZ, .z = sc + b.dummyZ,
                                     .z16 = {sc + b.Z16, xZ}, .n16 = Z / 16});
  // phi_z(z): layers 0..2 as one run when Z == H (the first layer's K is Z: part of the run only then), else layer 0 on its own
  {
    const int f0 = Z == H ? 0 : 1;
    if (f0) add_lin(bld, T, layer({sc + b.Z16, xZ}, VP_PHI0, Z, c->phi_b[0], 0.f, {sc + b.F16[0], xH}, ctH));
    SeqLink lf[3];
    for (int l = f0; l < 3; ++l) lf[l - f0] = SeqLink{W(VP_PHI0 + l), c->phi_b[l], nullptr, 0, 0, sc + b.F16[l]};
    add_linseq(bld, ctH, 0, d.rH, H, true, false, 0, T, f0 ? Ptr(sc + b.F16[0], xH) : Ptr(sc + b.Z16, xZ), 3 - f0, lf, 0, xH, ctH, 0.f, 0);
  }
  // the last layer feeds the GRU input cat[enc | phi] and the decoder input cat[phi | h_t]
  {
    Lin l = layer({sc + b.F16[2], xH}, VP_PHI3, H, c->phi_b[3], 0.f, {sc + b.CAT16 + (size_t)(X / 16) * 256, xC}, (X + H) / 16);
    l.o16b = {sc + b.DC16, xD}; l.n16b = (H + R) / 16;
    add_lin(bld, T, l);
  }
  add_gru_cell(bld, d, R, {.X16 = {sc + b.CAT16, xC}, .K = X + H, .Wih = W(VP_WIH), .bih = c->gru_bih, .GH = sc + b.GHb, .HS = sc + b.HS, .dummy = sc + b.dummyR,
                           .h16 = {sc + b.H16 + xR, xR}, .n16 = ctR, .h16b = {sc + b.DC16 + (size_t)(H / 16) * 256, xD}, .n16b = (H + R) / 16});
  // decoder(cat[phi, h_t])
  add_lin(bld, T, layer({sc + b.DC16, xD}, VP_DEC0, H + R, w->dec_b[0], slope, {sc + b.D16[0], xH}, ctH));
  add_lin(bld, T, layer({sc + b.D16[0], xH}, VP_DEC1, H, w->dec_b[1], slope, {sc + b.D16[1], xH}, ctH));
  add_tail(bld, d, p.sp, {.D16 = sc + b.D16[1], .ld_a = 0, .n16 = 0, .W = W(VP_DEC2), .bias = p.bias, .slope = slope, .DEC = sc + b.DEC, .X16 = sc + b.X16,
                          .lik_w = w->lik_w, .lik_b = w->lik_b, .u = u, .v = v, .x_out = x_out, .log_eps = log_eps, .head = head});
}

// =================================================================================================================================
// SRNNAudio (srnn_decode.hip): 13 links per step.  The two concatenated inputs are ONE T16 slab each, written in parts:
//   CP16  T+2 slabs [rows,R+Z]: slab 0 = [d_0 | -], slab s+1 = cat[d_s | z_{s-1}] (GRU link of step s; head link of step s-1, which so
//         writes into slab s+2; also the hidden projection's operand of step s+1);  DC16  cat[z_s | d_s] (head link, GRU link)
// =================================================================================================================================
enum SrnnPack : int { SP_ENC0, SP_ENC1, SP_ENC2, SP_WIH, SP_WHH, SP_PRIOR0, SP_PRIOR1, SP_PRIOR2, SP_PRIOR_H, SP_DEC0, SP_DEC1, SP_DEC2 };
inline PackTable srnn_pack_table(const BlvmSrnnDecodeWeights& w, const BlvmSrnnWeights& c, int S, int H, int Z, int R, int F = kDmolF) {
  const StackPad sp = stack_pad(S, F);
  return pack_table(sp,
                    {{"enc0", w.enc_w[0], sp.Sp, H, sp.Sp}, {"enc1", w.enc_w[1], H, H, H}, {"enc2", w.enc_w[2], H, H, H},
                     {"wih", w.gru_wih, H, 3 * R, H}, {"whh", w.gru_whh, R, 3 * R, R},
                     {"prior0", c.prior_w[0], R + Z, H, R + Z}, {"prior1", c.prior_w[1], H, H, H}, {"prior2", c.prior_w[2], H, H, H},
                     {"prior_h", c.prior_hw, H, 2 * Z, H},
                     {"dec0", w.dec_w[0], Z + R, H, Z + R}, {"dec1", w.dec_w[1], H, H, H}, {"dec2", w.dec_w[2], H, sp.Np, H}},
                    SP_ENC0, SP_DEC2, w.dec_b[2]);
}
// (as VrnnBufs;  DS  T+1 slabs [B,R] row-major d (polled words), slab 0 = d0;  ZS  z_s row-major, an output: written, never polled)
struct SrnnBufs {
  size_t X16, E16[2], ENC16, CP16, DS, GHb, P16[3], DC16, D16[2], DEC, polled_end, ZS, dummyZ, dummyR, end;
  std::vector<Region> regions;
};
inline SrnnBufs srnn_generate_layout(size_t base, int T, int B, int S, int H, int Z, int R, int F = kDmolF) {
  SrnnBufs b{};
  RegionArena ar(base);
  const size_t rows = (size_t)((B + 15) / 16) * 16, m = (size_t)T * rows;
  const StackPad sp = stack_pad(S, F);
  b.X16 = ar.take("X16", (m + rows) * sp.Sp);
  b.E16[0] = ar.take("E16.0", m * H); b.E16[1] = ar.take("E16.1", m * H); b.ENC16 = ar.take("ENC16", m * H);
  b.CP16 = ar.take("CP16", (m + 2 * rows) * (R + Z));
  b.DS = ar.take("DS", (size_t)(T + 1) * B * R);
  b.GHb = ar.take("GHb", (size_t)T * B * 3 * R);
  for (int i = 0; i < 3; ++i) b.P16[i] = ar.take("P16", m * H);
  b.DC16 = ar.take("DC16", m * (Z + R));
  b.D16[0] = ar.take("D16.0", m * H); b.D16[1] = ar.take("D16.1", m * H);
  b.DEC = ar.take("DEC", (size_t)T * B * sp.Np);
  b.polled_end = ar.floats();
  b.ZS = ar.take("ZS", (size_t)T * B * Z);
  b.dummyZ = ar.take("dummyZ", (size_t)B * Z);
  b.dummyR = ar.take("dummyR", (size_t)B * R);
  b.end = ar.floats();
  b.regions = std::move(ar.regions);
  return b;
}
enum SrnnSrc : int { SS_X0, SS_D0, SS_Z0 };
inline std::vector<Prefill> srnn_generate_prefills(const SrnnBufs& b, int B, int S, int Z, int R) {
  const int nCP = (R + Z) / 16;
  const size_t xCP = (size_t)((B + 15) / 16) * 16 * (R + Z);
  return {{SS_X0, 0, true, b.X16, stack_pad(S, kDmolF).Sp, S, 0},
          {SS_D0, 0, true, b.CP16, R, R, nCP},                               // the d part of slab 0
          {SS_Z0, 0, true, b.CP16 + xCP + (size_t)(R / 16) * 256, Z, Z, nCP},  // the z part of slab 1
          {SS_D0, 0, false, b.DS, R, R, 0}};
}

//   encoder: K_LIN, K_LINSEQ x2 (leaky)                                     X16[s] -> E16[0..1][s] -> ENC16[s]
//   K_LIN    gh = d_{s-1} Whh^T + b_hh on the side range (gentle): the d part of CP16[s] -> GHb[s]
//   K_GRU                                                                   ENC16[s], GHb[s], DS[s] -> DS[s+1], CP16[s+1], DC16[s]
//   prior:   K_LIN, K_LINSEQ x2, K_HEAD                                     CP16[s+1] -> P16[0..2][s] -> ZS[s], DC16[s], CP16[s+2]
//   decoder and draw: K_LIN x2, the tail                                    DC16[s] -> D16[0..1][s] -> ...
// Every link of this program carries the caller's slope and states its operand's width in ld[LIN_LD_A].
inline void srnn_generate_program(Builder& bld, int ot, int cus_all, int tune, const BlvmSrnnDecodeWeights* w, const PackTable& p, const SrnnBufs& b, float* sc,
                                  const float* eps, const float* u, const float* v, float* x_out, int T, int B, int S, int H, int Z, int R, float sd_eps,
                                  float slope, float log_eps, const DrawPlan& head = {}) {
  const BlvmSrnnWeights* c = w->chain;
  const int ctH = H / 16, ctZ = Z / 16, ctR = R / 16, nCP = (R + Z) / 16, nDC = (Z + R) / 16;
  const Deal d = deal(T, B, H, cus_all, 3 * ctR * ((B + 15) / 16));
  const long xS = d.rows * p.sp.Sp, xH = d.xH, xCP = d.rows * (R + Z), xDC = d.rows * (Z + R);
  bld.begin(ot, T, B, 4, false, d.r_main);
  auto W = [&](int i) { return sc + p.off(i); };
  add_mlp3(bld, d, {.A = {sc + b.X16, xS}, .K = p.sp.Sp, .W = {W(SP_ENC0), W(SP_ENC1), W(SP_ENC2)}, .bias = {w->enc_b[0], w->enc_b[1], w->enc_b[2]},
                    .out = {sc + b.E16[0], sc + b.E16[1], sc + b.ENC16}, .slope = slope});
  // reads the d part of slab s, first needed by the GRU link's epilogue (canary: as the VRNN's)
  add_lin(bld, T, {.A = {sc + b.CP16, xCP}, .ld_a = nCP * 16, .W = W(SP_WHH), .bias = w->gru_bhh, .K = R, .ct = 3 * ctR,
                   .flags = DF_RM_SC1 | DF_GENTLE | ((tune & 16) ? DF_CANARY : 0), .slope = slope, .orm = {sc + b.GHb, 3L * B * R}, .ldo = 3 * R, .wg0 = d.r_main,
                   .nwg = d.r_side});
  add_gru_cell(bld, d, R, {.X16 = {sc + b.ENC16, xH}, .K = H, .Wih = W(SP_WIH), .bih = w->gru_bih, .GH = sc + b.GHb, .HS = sc + b.DS, .dummy = sc + b.dummyR,
                           .h16 = {sc + b.CP16 + xCP, xCP}, .n16 = nCP, .h16b = {sc + b.DC16 + (size_t)ctZ * 256, xDC}, .n16b = nDC});
  add_mlp3(bld, d, {.A = {sc + b.CP16 + xCP, xCP}, .K = R + Z, .W = {W(SP_PRIOR0), W(SP_PRIOR1), W(SP_PRIOR2)}, .bias = {c->prior_b[0], c->prior_b[1], c->prior_b[2]},
                    .out = {sc + b.P16[0], sc + b.P16[1], sc + b.P16[2]}, .slope = slope});
  // z_s into the decoder input and into the NEXT step's prior input
  add_prior_head(bld, d, Z, sd_eps, {.P16 = sc + b.P16[2], .W = W(SP_PRIOR_H), .bias = c->prior_hb, .eps = eps, .dummy = sc + b.dummyZ, .z = {sc + b.ZS, (long)B * Z},
                                     .z16 = {sc + b.DC16, xDC}, .n16 = nDC, .z16b = {sc + b.CP16 + 2 * xCP + (size_t)ctR * 256, xCP}, .n16b = nCP});
  // decoder(cat[z_s, d_s])
  add_lin(bld, T, {.A = {sc + b.DC16, xDC}, .ld_a = nDC * 16, .W = W(SP_DEC0), .bias = w->dec_b[0], .K = Z + R, .ct = ctH, .flags = DF_RELU, .slope = slope,
                   .o16 = {sc + b.D16[0], xH}, .n16 = ctH, .nwg = d.rH});
  add_lin(bld, T, {.A = {sc + b.D16[0], xH}, .ld_a = H, .W = W(SP_DEC1), .bias = w->dec_b[1], .K = H, .ct = ctH, .flags = DF_RELU, .slope = slope,
                   .o16 = {sc + b.D16[1], xH}, .n16 = ctH, .nwg = d.rH});
  add_tail(bld, d, p.sp, {.D16 = sc + b.D16[1], .ld_a = H, .n16 = 0, .W = W(SP_DEC2), .bias = p.bias, .slope = slope, .DEC = sc + b.DEC, .X16 = sc + b.X16,
                          .lik_w = w->lik_w, .lik_b = w->lik_b, .u = u, .v = v, .x_out = x_out, .log_eps = log_eps, .head = head});
}

}  // namespace pchain
}  // namespace blvm
