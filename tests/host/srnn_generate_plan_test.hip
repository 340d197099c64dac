// The SRNNAudio roll-out's program (csrc/rollout_plan.h, what blvm_srnn_generate launches) replayed on the host word by word
// (rollout_replay.h), for frame stacks of any size.  Its two concatenated slabs are written in parts: CP[s+1] = cat[d_s | z_{s-1}] by the
// GRU link of step s and the head link of step s-1 (which so stores into slab s+2; slab 1's z part is the prefilled z0), DC[s] = cat[z_s |
// d_s] by the head and the GRU link.  Besides the checks of the LSTM replays: the head's statistics and the GRU's gates go to the dummy
// regions only (outside the polled range, never read), d_prev comes from the prefill or from the GRU link one step earlier, eps is read
// inside the caller's array, d_out's slab and all of z_out are written.  No GPU call.
#include "rollout_replay.h"

namespace {
// one case: the program for (S, B, H, Z, R) on `cus` CUs, T steps; returns the errors
// mutate (the check must bite): 1 the head loses its second T16 output, so the next step's prior operand keeps sentinels in its z part
int run_case(int S, int B, int H, int Z, int R, int T, int cus, bool xcd, int mutate = 0) {
  const blvm::StackPad sp = blvm::stack_pad(S, kDmolF);
  // (the arrays the caller owns have their exact sizes: a read past an end is an error)
  std::vector<float> wts(1), bH(H), b2Z(2 * Z), b3R(3 * R), bN(sp.N), lik(kDmolF * kDmolF), eps((size_t)T * B * Z), uu((size_t)T * B * S * kDmolK), vv((size_t)T * B * S),
      xout((size_t)B * T * S);
  BlvmSrnnWeights c{};
  BlvmSrnnDecodeWeights w{};
  for (int i = 0; i < 3; ++i) { w.enc_w[i] = w.dec_w[i] = c.prior_w[i] = wts.data(); w.enc_b[i] = w.dec_b[i] = c.prior_b[i] = bH.data(); }
  w.dec_b[2] = bN.data(); c.prior_hw = w.gru_wih = w.gru_whh = wts.data(); c.prior_hb = b2Z.data(); w.gru_bih = w.gru_bhh = b3R.data();
  w.lik_w = w.lik_b = lik.data(); w.chain = &c;
  PackTable pk = srnn_pack_table(w, c, S, H, Z, R);
  const SrnnBufs b = srnn_generate_layout(pk.total, T, B, S, H, Z, R);
  int bad = check_regions(pk.regions, pk.total, b.regions, b.end, b.X16, b.polled_end);
  bad += pk.regions.size() != (size_t)(12 + (sp.padded() ? 3 : 0)) || b.polled_end != b.ZS || b.ZS >= b.dummyZ || b.dummyZ >= b.dummyR || b.dummyR >= b.end;
  std::vector<float> scratch(b.end);
  pk.use_staged(scratch.data());
  Builder bld;
  srnn_generate_program(bld, blvm::OP_F32, cus, 0, &w, pk, b, scratch.data(), eps.data(), uu.data(), vv.data(), xout.data(), T, B, S, H, Z, R, 1e-6f, 0.01f, -7.f);
  bld.p.xcd = xcd;
  const int head = 6;  // encoder x2, hidden projection, K_GRU, prior x2, K_HEAD, ...
  bad += bld.overflow || bld.p.ndesc != 11 || bld.p.S != T || bld.p.B != B || bld.p.d[head].kind != K_HEAD || bld.p.d[head].p[HEAD_Z16B] == nullptr;
  if (mutate == 1) bld.p.d[head].p[HEAD_Z16B] = nullptr;
  Replay r(bld.p, scratch, b.X16, b.polled_end, xout);
  r.dummy0 = b.dummyZ; r.dummy1 = b.end;
  for (const std::vector<float>* a : {&bH, &b2Z, &b3R, &bN, &lik, &eps, &uu, &vv}) r.own(*a);
  replay_prefills(r, srnn_generate_prefills(b, B, S, Z, R), B);
  replay_program(r, T, B, S, H, cus);
  bad += r.bad;
  bad += unwritten(r, b.DS + (size_t)T * B * R, (size_t)B * R) + unwritten(r, b.ZS, (size_t)T * B * Z);  // d_out, z_out
  return bad;
}
}  // namespace

int main() {
  int bad = 0, cases = 0;
  for (int S : {1, 5, 8, 16, 24})
    for (int B : {1, 17})
      for (int cus : {256, 32})
        for (bool xcd : {false, true}) {
          const int e = run_case(S, B, 48, 16, 32, 3, cus, xcd);
          if (e) printf("S %d B %d cus %d xcd %d: %d errors\n", S, B, cus, (int)xcd, e);
          bad += e;
          ++cases;
        }
  bad += run_case(5, 17, 48, 16, 32, 3, 256, false, 1) == 0;
  printf("srnn generate plan: %d cases, %d errors\n", cases, bad);
  return bad != 0;
}
