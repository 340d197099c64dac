// srnn_decode.hip — K3c: ancestral sampling from SRNNAudio, every step of every utterance in ONE persistent launch.
//
// Replaces the loop of `SRNN.generate` (blvm/models/srnn.py:304-403): enc = encoder(x_t) -> d_t = GRU(enc, d_{t-1}) (srnn.py:113) ->
// prior(cat[d_t, z_{t-1}]) -> z_t = mu + sd eps (srnn.py:92-111) -> decoder(cat[z_t, d_t]) -> DMoL head per sample -> draw -> x_{t+1}.
// A step is a program of 13 links for the persistent-chain engine (pchain.h / pchain.hip), every link's 16x16 tiles dealt over the
// whole chip; the 13.6 MB of weights stay in the L2s, activations travel as sentinel-polled T16 copies in per-step slabs.  The two
// concatenated inputs are ONE T16 slab each, written in parts by the links that produce the parts:
//   CP[s] = cat[d_s | z_{s-1}] (GRU link of step s, head link of step s-1; also the hidden-projection input of step s+1),
//   DC[s] = cat[z_s | d_s]     (head link, GRU link).
// The pack table, the layout of the scratch and the descriptor list are in rollout_plan.h, which tests/host/srnn_generate_plan_test.hip
// replays on the host.
#include "common.h"
#include "rollout_launch.h"

using namespace blvm;

extern "C" size_t blvm_srnn_generate_scratch_floats_head(int T, int B, int S, int H, int Z, int R, int head_kind) {
  pchain::DrawPlan dp;
  if (T <= 0 || B <= 0 || S <= 0 || H <= 0 || Z <= 0 || R <= 0 || pchain::draw_plan(head_kind, pchain::kDmolK, 0.f, 0.f, &dp) != nullptr) return 0;
  const BlvmSrnnWeights c{};  // sizes only: the pack table of no weights
  return pchain::srnn_generate_layout(pchain::srnn_pack_table(BlvmSrnnDecodeWeights{}, c, S, H, Z, R, dp.F).total, T, B, S, H, Z, R, dp.F).end;
}
extern "C" size_t blvm_srnn_generate_scratch_floats(int T, int B, int S, int H, int Z, int R) {
  return blvm_srnn_generate_scratch_floats_head(T, B, S, H, Z, R, pchain::DRAW_DMOL);
}

extern "C" int blvm_srnn_generate_head(const BlvmSrnnDecodeWeights* w, const float* x0, const float* d0, const float* z0, const float* eps, const float* u,
                                       const float* v, int T, int B, int S, int H, int Z, int R, int head_kind, int num_mix, float log_eps, float head_sd_beta,
                                       float head_sd_eps, float sd_eps, float slope, float* x_out, float* d_out, float* z_out, float* scratch, void* stream_) {
  using namespace pchain;
  hipStream_t s = static_cast<hipStream_t>(stream_);
  BLVM_REQUIRE(w && w->chain && x0 && eps && x_out && scratch, "srnn_generate: null pointer");
  BLVM_REQUIRE(T >= 0 && B > 0 && B <= kPchainCarveMaxB, "srnn_generate: bad T=%d B=%d (at most %d utterances)", T, B, kPchainCarveMaxB);
  BLVM_REQUIRE(H % 16 == 0 && Z % 16 == 0 && R % 16 == 0 && S > 0 && H > 0 && Z > 0 && R > 0,
               "srnn_generate: S must be positive and H, Z, R positive multiples of 16 (got %d, %d, %d, %d)", S, H, Z, R);
  DrawPlan dp;
  const char* const why = draw_plan(head_kind, num_mix, head_sd_beta, head_sd_eps, &dp);
  BLVM_REQUIRE(why == nullptr, "srnn_generate: %s (kind %d, num_mix %d, head_sd_beta %g)", why, head_kind, num_mix, (double)head_sd_beta);
  BLVM_REQUIRE(draw_streams_ok(dp, u, v), "srnn_generate: u and v are given together (both NULL: the mode); the Gaussian head takes no u");
  BLVM_REQUIRE(aligned16(scratch), "srnn_generate: scratch must be 16-byte aligned");
  BLVM_REQUIRE(device_cus() >= 32, "srnn_generate: needs a device with at least 32 CUs");
  if (T == 0) return BLVM_OK;
  PackTable p = srnn_pack_table(*w, *w->chain, S, H, Z, R, dp.F);
  const SrnnBufs b = srnn_generate_layout(p.total, T, B, S, H, Z, R, dp.F);
  float* const sc = scratch;
  const OpType ot = pchain_optype(B);
  BLVM_TRY(stage_and_pack(p, ot, sc, s));
  Builder bld;
  srnn_generate_program(bld, ot, device_cus(), pchain_tune(), w, p, b, sc, eps, u, v, x_out, T, B, S, H, Z, R, sd_eps, slope, log_eps, dp);
  const float* const srcs[] = {x0, d0, z0};
  BLVM_TRY(fill_and_prefill(b.X16, b.polled_end, srnn_generate_prefills(b, B, S, Z, R), srcs, B, sc, s));
  BLVM_TRY(pchain_launch(bld, "srnn_generate", s));
  if (d_out) BLVM_HIP(hipMemcpyAsync(d_out, sc + b.DS + (size_t)T * B * R, sizeof(float) * (size_t)B * R, hipMemcpyDeviceToDevice, s));
  if (z_out) BLVM_HIP(hipMemcpyAsync(z_out, sc + b.ZS, sizeof(float) * (size_t)T * B * Z, hipMemcpyDeviceToDevice, s));
  return BLVM_OK;
}

extern "C" int blvm_srnn_generate(const BlvmSrnnDecodeWeights* w, const float* x0, const float* d0, const float* z0, const float* eps, const float* u,
                                  const float* v, int T, int B, int S, int H, int Z, int R, int num_mix, float sd_eps, float slope, float log_eps,
                                  float* x_out, float* d_out, float* z_out, float* scratch, void* stream) {
  return blvm_srnn_generate_head(w, x0, d0, z0, eps, u, v, T, B, S, H, Z, R, pchain::DRAW_DMOL, num_mix, log_eps, 0.f, 0.f, sd_eps, slope, x_out, d_out, z_out, scratch, stream);
}
