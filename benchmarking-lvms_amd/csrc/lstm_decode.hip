// lstm_decode.hip — sampling from LSTMAudio, every step of every utterance in ONE persistent launch.
//
// The loop of `LSTMAudio.generate` (blvm/models/lstm.py): emb = embedding(x_{s-1}) -> per layer (h, c) = LSTMCell(input, (h, c)) -> decoder(h of the
// last layer) -> DMoL head per sample -> draw (or the mode) -> x_s.  A step is a program of 6 + 2 * num_layers links for the persistent-chain
// engine (pchain.h / pchain.hip); the pack table, the layout of the scratch and the descriptor list are in lstm_decode.h (on the plan
// shared with the VRNN and SRNN roll-outs, rollout_plan.h), which the host plan tests (tests/host/lstm_decode*_plan_test.hip) replay.  Each layer's hidden projection h_{s-1} Whh^T + b_hh depends only on the previous step,
// so it runs as a gentle link on a side range of workgroups and the cell link picks its words up in its epilogue (tile_lstm).
#include "lstm_decode.h"

#include "common.h"
#include "rollout_launch.h"

using namespace blvm;

extern "C" size_t blvm_lstm_generate_scratch_floats(int T, int B, int S, int H, int num_layers) {
  if (T <= 0 || B <= 0 || S <= 0 || H <= 0 || num_layers <= 0 || num_layers > pchain::kLstmDecodeMaxLayers) return 0;
  return pchain::lstm_decode_layout(pchain::lstm_pack_table(BlvmLstmDecodeWeights{}, S, H, num_layers).total, T, B, S, H, num_layers).end;
}

extern "C" int blvm_lstm_generate_any_stack(const BlvmLstmDecodeWeights* w, const float* x0, const float* h0, const float* c0, const float* u, const float* v, int T,
                                            int B, int S, int H, int num_layers, int num_mix, float log_eps, float* x_out, float* h_out, float* c_out, float* scratch,
                                            void* stream_) {
  using namespace pchain;
  hipStream_t s = static_cast<hipStream_t>(stream_);
  const int L = num_layers;
  BLVM_REQUIRE(w && w->wih && w->whh && w->bih && w->bhh && x_out && scratch, "lstm_generate: null pointer");
  BLVM_REQUIRE(T >= 0 && B >= 1 && B <= kPchainCarveMaxB, "lstm_generate: bad T=%d B=%d (at most %d utterances)", T, B, kPchainCarveMaxB);
  BLVM_REQUIRE(S > 0 && H > 0 && H % 16 == 0, "lstm_generate: S must be positive and H a positive multiple of 16 (got %d, %d)", S, H);
  BLVM_REQUIRE(L >= 1 && L <= kLstmDecodeMaxLayers, "lstm_generate: 1 to %d layers (got %d)", kLstmDecodeMaxLayers, L);
  BLVM_REQUIRE(num_mix == kDmolK, "lstm_generate: the DMoL head has %d components", kDmolK);
  BLVM_REQUIRE((u == nullptr) == (v == nullptr), "lstm_generate: u and v are given together (both NULL: the mode)");
  BLVM_REQUIRE(aligned16(scratch), "lstm_generate: scratch must be 16-byte aligned");
  BLVM_REQUIRE(device_cus() >= 32, "lstm_generate: needs a device with at least 32 CUs");
  if (T == 0) return BLVM_OK;
  PackTable p = lstm_pack_table(*w, S, H, L);
  const LstmDecodeBufs b = lstm_decode_layout(p.total, T, B, S, H, L);
  float* const sc = scratch;
  const OpType ot = pchain_optype(B);
  BLVM_TRY(stage_and_pack(p, ot, sc, s));
  Builder bld;
  lstm_decode_program(bld, ot, device_cus(), w, p, b, sc, u, v, x_out, T, B, S, H, L, log_eps);
  const float* const srcs[] = {x0, h0, c0};
  BLVM_TRY(fill_and_prefill(b.X16, b.polled_end, lstm_decode_prefills(b, B, S, H, L), srcs, B, sc, s));
  BLVM_TRY(pchain_launch(bld, "lstm_generate", s));
  const size_t sH = (size_t)B * H;
  for (int l = 0; l < L; ++l) {
    if (h_out) BLVM_HIP(hipMemcpyAsync(h_out + l * sH, sc + b.HS[l] + (size_t)(T - 1) * sH, sizeof(float) * sH, hipMemcpyDeviceToDevice, s));
    if (c_out) BLVM_HIP(hipMemcpyAsync(c_out + l * sH, sc + b.CS[l] + (size_t)T * sH, sizeof(float) * sH, hipMemcpyDeviceToDevice, s));
  }
  return BLVM_OK;
}

// The entry point as it was published: frame stacks in multiples of 16 only.  A caller that passes another S to THIS symbol gets the
// refusal it always got (its arrays may be sized for the rule it knew); stacks of any size go through blvm_lstm_generate_any_stack.
extern "C" int blvm_lstm_generate(const BlvmLstmDecodeWeights* w, const float* x0, const float* h0, const float* c0, const float* u, const float* v, int T, int B, int S,
                                  int H, int num_layers, int num_mix, float log_eps, float* x_out, float* h_out, float* c_out, float* scratch, void* stream_) {
  BLVM_REQUIRE(S > 0 && S % 16 == 0, "lstm_generate: S must be a positive multiple of 16 (got %d); blvm_lstm_generate_any_stack takes any S", S);
  return blvm_lstm_generate_any_stack(w, x0, h0, c0, u, v, T, B, S, H, num_layers, num_mix, log_eps, x_out, h_out, c_out, scratch, stream_);
}
