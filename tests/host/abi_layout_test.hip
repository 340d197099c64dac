// Host-only: what the compiler makes of the structs of include/blvm_hip.h.  Prints `Name <sizeof>` per struct and `Name.member <offsetof>`
// per member; tests/test_abi_cpu.py compares the numbers with the ctypes classes blvm/_hip.py generates from the same header.
#include <cstddef>
#include <cstdio>

#include "blvm_hip.h"

#define S(T) std::printf("%s %zu\n", #T, sizeof(T))
#define M(T, m) std::printf("%s.%s %zu\n", #T, #m, offsetof(T, m))
#define HEADS(T) M(T, prior_w), M(T, prior_b), M(T, prior_hw), M(T, prior_hb), M(T, post_w), M(T, post_b), M(T, post_hw), M(T, post_hb)
#define GRU(T) M(T, gru_wih), M(T, gru_whh), M(T, gru_bih), M(T, gru_bhh)
#define TAIL(T) M(T, dec_w), M(T, dec_b), M(T, lik_w), M(T, lik_b)

int main() {
  S(BlvmVrnnWeights), HEADS(BlvmVrnnWeights), M(BlvmVrnnWeights, phi_w), M(BlvmVrnnWeights, phi_b), GRU(BlvmVrnnWeights);
  S(BlvmVrnnGrads), HEADS(BlvmVrnnGrads), M(BlvmVrnnGrads, phi_w), M(BlvmVrnnGrads, phi_b), GRU(BlvmVrnnGrads);
  S(BlvmSrnnWeights), HEADS(BlvmSrnnWeights);
  S(BlvmSrnnGrads), HEADS(BlvmSrnnGrads);
  S(BlvmRssmWeights), M(BlvmRssmWeights, gin_w), M(BlvmRssmWeights, gin_b), GRU(BlvmRssmWeights), HEADS(BlvmRssmWeights);
  S(BlvmRssmGrads), M(BlvmRssmGrads, gin_w), M(BlvmRssmGrads, gin_b), GRU(BlvmRssmGrads), HEADS(BlvmRssmGrads);
  S(BlvmVrnnDecodeWeights), M(BlvmVrnnDecodeWeights, enc_w), M(BlvmVrnnDecodeWeights, enc_b), M(BlvmVrnnDecodeWeights, cell),
      TAIL(BlvmVrnnDecodeWeights);
  S(BlvmSrnnDecodeWeights), M(BlvmSrnnDecodeWeights, enc_w), M(BlvmSrnnDecodeWeights, enc_b), GRU(BlvmSrnnDecodeWeights),
      M(BlvmSrnnDecodeWeights, chain), TAIL(BlvmSrnnDecodeWeights);
  S(BlvmLstmDecodeWeights), M(BlvmLstmDecodeWeights, emb_w), M(BlvmLstmDecodeWeights, emb_b), M(BlvmLstmDecodeWeights, wih),
      M(BlvmLstmDecodeWeights, whh), M(BlvmLstmDecodeWeights, bih), M(BlvmLstmDecodeWeights, bhh), TAIL(BlvmLstmDecodeWeights);
  return 0;
}
