// lstm_decode.hip — sampling from LSTMAudio, every step of every utterance in ONE persistent launch.
//
// The loop of `LSTMAudio.generate` (blvm/models/lstm.py): emb = embedding(x_{s-1}) -> per layer (h, c) = LSTMCell(input, (h, c)) -> decoder(h of the
// last layer) -> DMoL head per sample -> draw (or the mode) -> x_s.  A step is a program of 6 + 2 * num_layers links for the persistent-chain
// engine (pchain.h / pchain.hip); the layout of the scratch and the descriptor list are in lstm_decode.h, which the host plan test
// (tests/host/lstm_decode_plan_test.hip) reads too.  Each layer's hidden projection h_{s-1} Whh^T + b_hh depends only on the previous step,
// so it runs as a gentle link on a side range of workgroups and the cell link picks its words up in its epilogue (tile_lstm).
#include "lstm_decode.h"

#include "common.h"

using namespace blvm;

extern "C" size_t blvm_lstm_generate_scratch_floats(int T, int B, int S, int H, int num_layers) {
  if (T <= 0 || B <= 0 || S <= 0 || H <= 0 || num_layers <= 0 || num_layers > pchain::kLstmDecodeMaxLayers) return 0;
  return pchain::lstm_decode_layout(pchain::lstm_decode_pack_layout(S, H, num_layers).total, T, B, S, H, num_layers).end;
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
  BLVM_REQUIRE(num_mix == LD_K, "lstm_generate: the DMoL head has %d components", LD_K);
  BLVM_REQUIRE((u == nullptr) == (v == nullptr), "lstm_generate: u and v are given together (both NULL: the mode)");
  BLVM_REQUIRE(aligned16(scratch), "lstm_generate: scratch must be 16-byte aligned");
  BLVM_REQUIRE(device_cus() >= 32, "lstm_generate: needs a device with at least 32 CUs");
  if (T == 0) return BLVM_OK;
  const LstmDecodePack p = lstm_decode_pack_layout(S, H, L);
  const LstmDecodeBufs b = lstm_decode_layout(p.total, T, B, S, H, L);
  float* const sc = scratch;
  const OpType ot = pchain_optype(B);
  T16PackScope pack_scope(ot, s);
#define PACK(dst, src, ld, rows, k) BLVM_TRY(t16_pack_rows(src, ld, rows, k, sc + (dst), s))
  const StackPad sp = stack_pad(S, LD_F);
  if (sp.padded()) {  // the ragged stack's weights and bias, zero-padded to the tile boundaries (lstm_decode.h)
    BLVM_TRY(pad_copy(sc + p.st_emb0, H, sp.Sp, w->emb_w[0], H, S, s));
    BLVM_TRY(pad_copy(sc + p.st_dec2, sp.Np, H, w->dec_w[2], sp.N, H, s));
    BLVM_TRY(pad_copy(sc + p.dec_b2, 1, sp.Np, w->dec_b[2], 1, sp.N, s));
  }
  PACK(p.emb[0], sp.padded() ? sc + p.st_emb0 : w->emb_w[0], sp.Sp, H, sp.Sp); PACK(p.emb[1], w->emb_w[1], H, H, H); PACK(p.emb[2], w->emb_w[2], H, H, H);
  for (int l = 0; l < L; ++l) { PACK(p.wih[l], w->wih[l], H, 4 * H, H); PACK(p.whh[l], w->whh[l], H, 4 * H, H); }
  PACK(p.dec[0], w->dec_w[0], H, H, H); PACK(p.dec[1], w->dec_w[1], H, H, H); PACK(p.dec[2], sp.padded() ? sc + p.st_dec2 : w->dec_w[2], H, sp.Np, H);
#undef PACK
  BLVM_TRY(pack_scope.flush());  // all packs above in one launch
  Builder bld;
  lstm_decode_program(bld, ot, device_cus(), w, p, b, sc, u, v, x_out, T, B, S, H, L, log_eps);
  // sentinel-fill everything the launch polls, then the initial frame stack and states
  BLVM_HIP(pchain_fill_sentinel(sc + b.X16, sizeof(float) * (b.polled_end - b.X16), s));
  const size_t sH = (size_t)B * H;
  for (const LstmDecodePrefill& f : lstm_decode_prefills(b, S, H, L)) {
    const float* src = f.src == LstmDecodePrefill::X0 ? x0 : f.src == LstmDecodePrefill::H0 ? (h0 ? h0 + f.layer * sH : nullptr) : (c0 ? c0 + f.layer * sH : nullptr);
    if (f.t16) BLVM_TRY(pchain_rows_to_t16(src, f.src_cols, B, f.cols, sc + f.off, s, 0, f.src_cols));
    else BLVM_HIP(copy_or_zero(sc + f.off, src, sizeof(float) * (size_t)B * f.cols, s));
  }
  BLVM_TRY(pchain_launch(bld, "lstm_generate", s));
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
