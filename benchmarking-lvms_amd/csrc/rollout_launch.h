// rollout_launch.h — the device side of the shared roll-out plan (rollout_plan.h): what vrnn_decode.hip, srnn_decode.hip and
// lstm_decode.hip enqueue around their step programs.
#pragma once
#include "rollout_plan.h"

namespace blvm {
namespace pchain {

// every weight copy of the table in one launch; S % 16 != 0 (pchain.h stack_pad): first the zero-padded row-major copies that the first
// layer's and the last decoder layer's packs and the last layer (its bias) then read instead of the caller's arrays
inline int stage_and_pack(PackTable& t, OpType ot, float* sc, hipStream_t s) {
  if (t.sp.padded()) {
    const PackEntry &in = t.e[t.first], &dec = t.e[t.last];
    BLVM_TRY(pad_copy(sc + t.stage_in, in.rows, t.sp.Sp, in.src, in.rows, t.sp.S, s));
    BLVM_TRY(pad_copy(sc + t.stage_dec, t.sp.Np, dec.k, dec.src, t.sp.N, dec.k, s));
    BLVM_TRY(pad_copy(sc + t.stage_bias, 1, t.sp.Np, t.bias, 1, t.sp.N, s));
    t.use_staged(sc);
  }
  T16PackScope pack_scope(ot, s);
  for (const PackEntry& p : t.e) BLVM_TRY(t16_pack_rows(p.src, p.ld, p.rows, p.k, sc + p.off, s));
  return pack_scope.flush();
}

// sentinel-fill everything the launch polls, [X16, polled_end), then the initial frame stack and states from the caller's arrays srcs[]
inline int fill_and_prefill(size_t X16, size_t polled_end, const std::vector<Prefill>& list, const float* const* srcs, int B, float* sc, hipStream_t s) {
  BLVM_HIP(pchain_fill_sentinel(sc + X16, sizeof(float) * (polled_end - X16), s));
  for (const Prefill& f : list) {
    const float* src = srcs[f.src] ? srcs[f.src] + f.src_off : nullptr;
    if (f.t16) BLVM_TRY(pchain_rows_to_t16(src, f.src_cols, B, f.cols, sc + f.off, s, f.n16, f.src_cols));
    else BLVM_HIP(copy_or_zero(sc + f.off, src, sizeof(float) * (size_t)B * f.cols, s));
  }
  return BLVM_OK;
}

}  // namespace pchain
}  // namespace blvm
