// The LSTMAudio roll-out's program (csrc/lstm_decode.h, what lstm_decode.hip launches) replayed on the host, word by word
// (rollout_replay.h): every polled word a link reads lies in the sentinel-filled part of the scratch and was prefilled before the
// launch or written by exactly one link earlier in (step, program) order; no word is written twice; every tile of every link has
// exactly one owner; the c a cell tile reads was written by the same descriptor one step earlier (the same workgroup and thread: tile
// lists are per launch) or prefilled; the outputs are written completely; the regions of the scratch layout do not overlap.  A
// persistent launch whose wiring breaks one of these spins until its bound: this runs first, on the CPU, with no GPU call.
#include "lstm_decode.h"
#include "rollout_replay.h"

namespace {
// one case: the program for (B, L, T) on `cus` CUs; returns the errors
// mutate (the check must bite): 1 the first cell link reads the NEXT step's hidden projection; 2 the draw stores into the slab it came from
int run_case(int B, int L, int T, int cus, bool xcd, int mutate = 0) {
  const int S = 32, H = 48;
  std::vector<float> dummy(4 * H + S * kDmolF + kDmolF * kDmolF), uu((size_t)T * B * S * kDmolK), vv((size_t)T * B * S), xout((size_t)B * T * S);
  const float* lay[kLstmDecodeMaxLayers];
  for (int l = 0; l < kLstmDecodeMaxLayers; ++l) lay[l] = dummy.data();
  BlvmLstmDecodeWeights w{};
  for (int i = 0; i < 3; ++i) w.emb_w[i] = w.emb_b[i] = w.dec_w[i] = w.dec_b[i] = dummy.data();
  w.wih = w.whh = w.bih = w.bhh = lay; w.lik_w = w.lik_b = dummy.data();
  PackTable pk = lstm_pack_table(w, S, H, L);
  const LstmDecodeBufs b = lstm_decode_layout(pk.total, T, B, S, H, L);
  int bad = check_regions(pk.regions, pk.total, b.regions, b.end, b.X16, b.polled_end);
  bad += b.regions.size() != (size_t)(7 + 5 * L) || pk.regions.size() != (size_t)(6 + 2 * L);
  std::vector<float> scratch(b.end);
  pk.use_staged(scratch.data());
  Builder bld;
  lstm_decode_program(bld, blvm::OP_F32, cus, &w, pk, b, scratch.data(), uu.data(), vv.data(), xout.data(), T, B, S, H, L, -7.f);
  bld.p.xcd = xcd;
  if (mutate == 1) bld.p.d[3].p[LSTM_GH] += (long)B * 4 * H;
  if (mutate == 2) bld.p.d[bld.p.ndesc - 1].p[DMOLS_X16] -= (long)((B + 15) / 16) * 16 * S;
  const Program& p = bld.p;
  bad += bld.overflow || p.ndesc != 6 + 2 * L || p.S != T || p.B != B;
  Replay r(p, scratch, b.X16, b.polled_end, xout);
  r.own(dummy); r.own(uu); r.own(vv);
  replay_prefills(r, lstm_decode_prefills(b, B, S, H, L), B);
  replay_program(r, T, B, S, H, cus);
  bad += r.bad;
  // what the caller gets back is written completely: x_out (replay_program), and per layer the last h and c slabs
  for (int l = 0; l < L; ++l) bad += unwritten(r, b.HS[l] + (size_t)(T - 1) * B * H, (size_t)B * H) + unwritten(r, b.CS[l] + (size_t)T * B * H, (size_t)B * H);
  return bad;
}
}  // namespace

int main() {
  int bad = 0, cases = 0;
  for (int cus : {256, 32})
    for (int L : {1, 2})
      for (int B : {1, 16, 17, 128})
        for (bool xcd : {false, true}) {
          const int e = run_case(B, L, 3, cus, xcd);
          if (e) printf("B %d layers %d cus %d xcd %d: %d errors\n", B, L, cus, (int)xcd, e);
          bad += e;
          ++cases;
        }
  bad += run_case(17, 2, 3, 256, false, 1) == 0;
  bad += run_case(17, 2, 3, 256, false, 2) == 0;
  printf("lstm decode plan: %d cases, %d errors\n", cases, bad);
  return bad != 0;
}
