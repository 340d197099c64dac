// The VRNNAudio roll-out's program (csrc/rollout_plan.h, what blvm_vrnn_generate launches) replayed on the host word by word
// (rollout_replay.h), for frame stacks of any size and both arms of the phi MLP (Z == H: its first layer joins the run; Z != H: a link of
// its own).  Its concatenated slabs are written in parts by different links: cat[enc | phi] by the encoder's last layer and phi's, cat[phi
// | h] by phi's last layer (its second T16 output) and the GRU link.  Besides the checks of the LSTM replays: the head's statistics and
// the GRU's gates go to the dummy regions only (outside the polled range, never read), h_prev comes from the prefill or from the GRU link
// one step earlier, eps is read inside the caller's array, h_out's slab is written.  No GPU call.
#include "rollout_replay.h"

namespace {
// one case: the program for (S, B, H, Z, R) on `cus` CUs, T steps; returns the errors
// mutate (the check must bite): 1 the phi[3] link loses its second T16 output, so the decoder input's phi part is never written
int run_case(int S, int B, int H, int Z, int R, int T, int cus, bool xcd, int mutate = 0) {
  const blvm::StackPad sp = blvm::stack_pad(S, kDmolF);
  // (the arrays the caller owns have their exact sizes: a read past an end is an error)
  std::vector<float> wts(1), bH(H), b2Z(2 * Z), b3R(3 * R), bN(sp.N), lik(kDmolF * kDmolF), eps((size_t)T * B * Z), uu((size_t)T * B * S * kDmolK), vv((size_t)T * B * S),
      xout((size_t)B * T * S);
  BlvmVrnnWeights c{};
  BlvmVrnnDecodeWeights w{};
  for (int i = 0; i < 3; ++i) { w.enc_w[i] = w.dec_w[i] = c.prior_w[i] = wts.data(); w.enc_b[i] = w.dec_b[i] = c.prior_b[i] = bH.data(); }
  for (int i = 0; i < 4; ++i) { c.phi_w[i] = wts.data(); c.phi_b[i] = bH.data(); }
  w.dec_b[2] = bN.data(); c.prior_hw = c.gru_wih = c.gru_whh = wts.data(); c.prior_hb = b2Z.data(); c.gru_bih = c.gru_bhh = b3R.data();
  w.lik_w = w.lik_b = lik.data(); w.cell = &c;
  PackTable pk = vrnn_pack_table(w, c, S, H, Z, R);
  const VrnnBufs b = vrnn_generate_layout(pk.total, T, B, S, H, Z, R);
  int bad = check_regions(pk.regions, pk.total, b.regions, b.end, b.X16, b.polled_end);
  bad += pk.regions.size() != (size_t)(16 + (sp.padded() ? 3 : 0)) || b.polled_end != b.dummyZ || b.dummyZ >= b.dummyR || b.dummyR >= b.end;
  std::vector<float> scratch(b.end);
  pk.use_staged(scratch.data());
  Builder bld;
  vrnn_generate_program(bld, blvm::OP_F32, cus, 0, &w, pk, b, scratch.data(), eps.data(), uu.data(), vv.data(), xout.data(), T, B, S, H, Z, R, 1e-6f, 0.01f, -7.f);
  bld.p.xcd = xcd;
  const int nd = Z == H ? 14 : 15, phi3 = nd - 6;  // (descriptors: the runs count once) ... phi[3], K_GRU, dec[0], dec[1], dec[2], K_DMOLS
  bad += bld.overflow || bld.p.ndesc != nd || bld.p.S != T || bld.p.B != B || bld.p.d[phi3].kind != K_LIN || bld.p.d[phi3].p[LIN_O16B] == nullptr;
  if (mutate == 1) bld.p.d[phi3].p[LIN_O16B] = nullptr;
  Replay r(bld.p, scratch, b.X16, b.polled_end, xout);
  r.dummy0 = b.dummyZ; r.dummy1 = b.end;
  for (const std::vector<float>* a : {&bH, &b2Z, &b3R, &bN, &lik, &eps, &uu, &vv}) r.own(*a);
  replay_prefills(r, vrnn_generate_prefills(b, S, R), B);
  replay_program(r, T, B, S, H, cus);
  bad += r.bad;
  bad += unwritten(r, b.HS + (size_t)T * B * R, (size_t)B * R);  // h_out
  return bad;
}
}  // namespace

int main() {
  int bad = 0, cases = 0;
  for (int Z : {48, 16})
    for (int S : {1, 5, 8, 16, 24})
      for (int B : {1, 17})
        for (int cus : {256, 32})
          for (bool xcd : {false, true}) {
            const int e = run_case(S, B, 48, Z, 32, 3, cus, xcd);
            if (e) printf("S %d B %d Z %d cus %d xcd %d: %d errors\n", S, B, Z, cus, (int)xcd, e);
            bad += e;
            ++cases;
          }
  for (int Z : {48, 16}) bad += run_case(5, 17, 48, Z, 32, 3, 256, false, 1) == 0;
  printf("vrnn generate plan: %d cases, %d errors\n", cases, bad);
  return bad != 0;
}
