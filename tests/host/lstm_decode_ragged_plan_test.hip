// The LSTMAudio roll-out's program (csrc/lstm_decode.h) for frame stacks that are NO multiple of 16, replayed on the host word by word
// (rollout_replay.h) as lstm_decode_plan_test.hip replays the unpadded one.  The frame-stack operand is padded to Sp = 16 ceil(S / 16)
// columns and the last decoder layer's rows to Np = 16 ceil(30 S / 16) floats (pchain.h stack_pad), and a consumer polls EVERY word of
// an operand block: so every pad word must be prefilled or written by exactly one earlier link, every step — a pad column left as a
// sentinel is a launch that spins to its bound.  Checked besides: no word written twice, one owner per tile, x_out complete at width S
// and nothing stored beyond it, u / v / bias reads inside the caller's arrays (the last layer's bias must be the padded copy), the draw
// tile reads only the 16-byte pieces that lie inside a padded row, the regions of the layout disjoint.  No GPU call.
#include "lstm_decode.h"
#include "rollout_replay.h"

namespace {
// one case: the program for (S, B, L, T) on `cus` CUs; returns the errors
// mutate (the check must bite): 1 the draw link covers the live samples only (ceil(S / 4) tiles: the operand's pad columns stay
// sentinels); 2 the last decoder layer reads the caller's bias [30 S] (past its end in the ragged tile)
int run_case(int S, int B, int L, int T, int cus, bool xcd, int mutate = 0) {
  const int H = 48;
  const blvm::StackPad sp = blvm::stack_pad(S, kDmolF);
  const int Sp = sp.Sp, N = sp.N, Np = sp.Np;
  // (the arrays the caller owns have their exact sizes: a read past an end is an error)
  std::vector<float> xout((size_t)B * T * S), dummy(4 * H + kDmolF * kDmolF), bH(H), bN(N), uu((size_t)T * B * S * kDmolK), vv((size_t)T * B * S);
  const float* lay[kLstmDecodeMaxLayers];
  for (int l = 0; l < kLstmDecodeMaxLayers; ++l) lay[l] = dummy.data();
  BlvmLstmDecodeWeights w{};
  for (int i = 0; i < 3; ++i) { w.emb_w[i] = w.dec_w[i] = dummy.data(); w.emb_b[i] = w.dec_b[i] = bH.data(); }
  w.dec_b[2] = bN.data();
  w.wih = w.whh = w.bih = w.bhh = lay; w.lik_w = w.lik_b = dummy.data();
  PackTable pk = lstm_pack_table(w, S, H, L);
  const LstmDecodeBufs b = lstm_decode_layout(pk.total, T, B, S, H, L);
  int bad = check_regions(pk.regions, pk.total, b.regions, b.end, b.X16, b.polled_end);
  bad += b.regions.size() != (size_t)(7 + 5 * L) || pk.regions.size() != (size_t)(6 + 2 * L + (sp.padded() ? 3 : 0));
  bad += Sp % 16 != 0 || Np % 16 != 0 || Sp < S || Np < N || Sp - S >= 16 || Np - N >= 16 || sp.padded() != (S % 16 != 0);
  std::vector<float> scratch(b.end);
  pk.use_staged(scratch.data());
  Builder bld;
  lstm_decode_program(bld, blvm::OP_F32, cus, &w, pk, b, scratch.data(), uu.data(), vv.data(), xout.data(), T, B, S, H, L, -7.f);
  bld.p.xcd = xcd;
  if (mutate == 1) bld.p.d[bld.p.ndesc - 1].ct = (S + 3) / 4;
  if (mutate == 2) bld.p.d[bld.p.ndesc - 2].p[LIN_BIAS] = w.dec_b[2];
  const Program& p = bld.p;
  bad += bld.overflow || p.ndesc != 6 + 2 * L || p.S != T || p.B != B;
  Replay r(p, scratch, b.X16, b.polled_end, xout);
  r.own(dummy); r.own(bH); r.own(bN); r.own(uu); r.own(vv);
  const std::vector<Prefill> pre = lstm_decode_prefills(b, B, S, H, L);
  bad += pre[0].src != LS_X0 || pre[0].cols != Sp || pre[0].src_cols != S;
  replay_prefills(r, pre, B);
  replay_program(r, T, B, S, H, cus);
  bad += r.bad;
  // what the caller gets back is written completely: x_out (replay_program), and per layer the last h and c slabs
  for (int l = 0; l < L; ++l) bad += unwritten(r, b.HS[l] + (size_t)(T - 1) * B * H, (size_t)B * H) + unwritten(r, b.CS[l] + (size_t)T * B * H, (size_t)B * H);
  return bad;
}
}  // namespace

int main() {
  int bad = 0, cases = 0;
  for (int S : {1, 5, 8, 24})
    for (int cus : {256, 32})
      for (int L : {1, 2})
        for (int B : {1, 17})
          for (bool xcd : {false, true}) {
            const int e = run_case(S, B, L, 3, cus, xcd);
            if (e) printf("S %d B %d layers %d cus %d xcd %d: %d errors\n", S, B, L, cus, (int)xcd, e);
            bad += e;
            ++cases;
          }
  for (int S : {1, 5, 8, 24}) bad += run_case(S, 17, 2, 3, 256, false, 1) == 0;  // every S has pad columns in its operand
  for (int S : {1, 5}) bad += run_case(S, 17, 2, 3, 256, false, 2) == 0;           // ... and these a ragged last decoder tile
  bad += run_case(16, 17, 1, 3, 256, false) != 0;  // a multiple of 16: nothing padded, the same checks hold
  printf("lstm decode ragged plan: %d cases, %d errors\n", cases, bad);
  return bad != 0;
}
