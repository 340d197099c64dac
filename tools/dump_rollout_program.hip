// Prints the step programs of the three one-launch roll-outs (csrc/rollout_plan.h, csrc/lstm_decode.h) built over host vectors: the
// Program header, the stride table and every Desc, each pointer as (name of the array it falls in, offset in floats) so that two
// builds of the plan can be compared with diff.  Host only, no GPU call.
//   hipcc --offload-arch=gfx950 -O1 -std=c++17 -w -Iinclude -Ibenchmarking-lvms_amd/csrc tools/dump_rollout_program.hip -o dump_rollout_program
// Grid: S in {1, 5, 8, 16, 24, 64} x B in {1, 17, 64, 128} x CUs in {32, 256}, T = 3; VRNN with Z == H and Z != H, LSTM with 1 and 2 layers.
// Without arguments: the DMoL programs (head kind 0), the output every earlier build of the plan can be compared with.  `--heads`: after
// them the VRNN and SRNN programs of the GMM head (kind 1) and the Gaussian head (kind 2), each title with its `head <kind>`; in every
// dump the draw link's head kind is i[3] and its sd_beta, sd_eps are f[1], f[2] of the last descriptor (pchain.h DMOLS_I_HEAD).
#include "lstm_decode.h"

#include <cstdio>
#include <cstring>
#include <deque>
#include <string>
#include <vector>
namespace blvm {
void set_error(const char*, ...) {}
int pchain_tune() { return 0; }
unsigned long long* pchain_profile_buffer() { return nullptr; }
}  // namespace blvm
using namespace blvm::pchain;

namespace {
struct Arrays {  // the caller's arrays of one case, by name
  std::deque<std::vector<float>> mem;
  std::vector<std::pair<std::string, const std::vector<float>*>> names;
  float* add(const std::string& name, size_t n) {
    mem.emplace_back(n);
    names.push_back({name, &mem.back()});
    return mem.back().data();
  }
  void print_ptr(const float* q) const {
    if (!q) { printf(" -"); return; }
    for (const auto& [name, v] : names)
      if (q >= v->data() && q <= v->data() + v->size()) { printf(" %s+%ld", name.c_str(), (long)(q - v->data())); return; }
    printf(" ?");
  }
};
unsigned bits(float f) { unsigned u; memcpy(&u, &f, 4); return u; }
void dump(const char* title, const Builder& bld, const Arrays& a) {
  const Program& p = bld.p;
  printf("== %s\nprogram ot %d rt_group %d s_first %d ndesc %d S %d B %d xcd %d prof_wg %d lds_products %d overflow %d nstride %d\nstrides", title, p.ot, p.rt_group,
         p.s_first, p.ndesc, p.S, p.B, p.xcd, p.prof_wg, p.lds_products, (int)bld.overflow, bld.nstride);
  for (int i = 0; i < 16; ++i) printf(" %ld", p.stride[i]);
  printf("\n");
  for (int i = 0; i < p.ndesc; ++i) {
    const Desc& d = p.d[i];
    printf("desc %d kind %d ct %d wg0 %d nwg %d flags %d K %d s %d..%d ld %d %d %d %d n16 %d %d i %d %d %d %d f %08x %08x %08x %08x\n  sidx", i, d.kind, d.ct, d.wg0, d.nwg,
           d.flags, d.K, d.s_begin, d.s_end, d.ld[0], d.ld[1], d.ld[2], d.ld[3], d.n16[0], d.n16[1], d.i[0], d.i[1], d.i[2], d.i[3], bits(d.f[0]), bits(d.f[1]),
           bits(d.f[2]), bits(d.f[3]));
    for (int k = 0; k < kMaxPtr; ++k) printf(" %d", d.sidx[k]);
    printf("\n  p");
    for (int k = 0; k < kMaxPtr; ++k) a.print_ptr(d.p[k]);
    printf("\n");
  }
}
constexpr int T = 3;
constexpr float kSdEps = 1e-6f, kSlope = 0.01f, kLogEps = -7.f;

// the head of kind `kind` as the entry points plan it (sd_beta ln 2, sd_eps 1e-4: the audio models' Gaussian heads)
DrawPlan head_of(int kind) {
  DrawPlan dp;
  draw_plan(kind, kDmolK, 0.6931472f, 1e-4f, &dp);
  return dp;
}
void vrnn(int S, int B, int H, int Z, int R, int cus, int tune, int kind = 0) {
  const DrawPlan dp = head_of(kind);
  const int kDmolF = dp.F, kDmolK = dp.K;  // (the head's widths under the names the sizes below use)
  Arrays a;
  BlvmVrnnWeights c{};
  BlvmVrnnDecodeWeights w{};
  const size_t big = (size_t)3 * R * (2 * H + R) + (size_t)S * kDmolF * H + (size_t)H * (H + R + S + Z);  // any weight fits
  for (int i = 0; i < 3; ++i) {
    const std::string n = std::to_string(i);
    w.enc_w[i] = a.add("enc_w" + n, big); w.enc_b[i] = a.add("enc_b" + n, H); w.dec_w[i] = a.add("dec_w" + n, big); w.dec_b[i] = a.add("dec_b" + n, i == 2 ? S * kDmolF : H);
    c.prior_w[i] = a.add("prior_w" + n, big); c.prior_b[i] = a.add("prior_b" + n, H);
  }
  for (int i = 0; i < 4; ++i) { c.phi_w[i] = a.add("phi_w" + std::to_string(i), big); c.phi_b[i] = a.add("phi_b" + std::to_string(i), H); }
  c.prior_hw = a.add("prior_hw", big); c.prior_hb = a.add("prior_hb", 2 * Z); c.gru_wih = a.add("gru_wih", big); c.gru_whh = a.add("gru_whh", big);
  c.gru_bih = a.add("gru_bih", 3 * R); c.gru_bhh = a.add("gru_bhh", 3 * R); w.lik_w = a.add("lik_w", kDmolF * kDmolF); w.lik_b = a.add("lik_b", kDmolF);
  w.cell = &c;
  auto p = vrnn_pack_table(w, c, S, H, Z, R, dp.F);
  const auto b = vrnn_generate_layout(p.total, T, B, S, H, Z, R, dp.F);
  float* sc = a.add("scratch", b.end);
  p.use_staged(sc);
  const float *eps = a.add("eps", (size_t)T * B * Z), *u = kDmolK ? a.add("u", (size_t)T * B * S * kDmolK) : nullptr, *v = a.add("v", (size_t)T * B * S);
  float* x_out = a.add("x_out", (size_t)B * T * S);
  Builder bld;
  vrnn_generate_program(bld, blvm::OP_F32, cus, tune, &w, p, b, sc, eps, u, v, x_out, T, B, S, H, Z, R, kSdEps, kSlope, kLogEps, dp);
  char title[128], head[16] = "";
  if (kind) snprintf(head, sizeof head, " head %d", kind);
  snprintf(title, sizeof title, "vrnn S %d B %d H %d Z %d R %d cus %d tune %d scratch %zu%s", S, B, H, Z, R, cus, tune, (size_t)b.end, head);
  dump(title, bld, a);
}
void srnn(int S, int B, int H, int Z, int R, int cus, int tune, int kind = 0) {
  const DrawPlan dp = head_of(kind);
  const int kDmolF = dp.F, kDmolK = dp.K;
  Arrays a;
  BlvmSrnnWeights c{};
  BlvmSrnnDecodeWeights w{};
  const size_t big = (size_t)3 * R * (H + R) + (size_t)S * kDmolF * H + (size_t)H * (H + R + S + Z);
  for (int i = 0; i < 3; ++i) {
    const std::string n = std::to_string(i);
    w.enc_w[i] = a.add("enc_w" + n, big); w.enc_b[i] = a.add("enc_b" + n, H); w.dec_w[i] = a.add("dec_w" + n, big); w.dec_b[i] = a.add("dec_b" + n, i == 2 ? S * kDmolF : H);
    c.prior_w[i] = a.add("prior_w" + n, big); c.prior_b[i] = a.add("prior_b" + n, H);
  }
  c.prior_hw = a.add("prior_hw", big); c.prior_hb = a.add("prior_hb", 2 * Z); w.gru_wih = a.add("gru_wih", big); w.gru_whh = a.add("gru_whh", big);
  w.gru_bih = a.add("gru_bih", 3 * R); w.gru_bhh = a.add("gru_bhh", 3 * R); w.lik_w = a.add("lik_w", kDmolF * kDmolF); w.lik_b = a.add("lik_b", kDmolF);
  w.chain = &c;
  auto p = srnn_pack_table(w, c, S, H, Z, R, dp.F);
  const auto b = srnn_generate_layout(p.total, T, B, S, H, Z, R, dp.F);
  float* sc = a.add("scratch", b.end);
  p.use_staged(sc);
  const float *eps = a.add("eps", (size_t)T * B * Z), *u = kDmolK ? a.add("u", (size_t)T * B * S * kDmolK) : nullptr, *v = a.add("v", (size_t)T * B * S);
  float* x_out = a.add("x_out", (size_t)B * T * S);
  Builder bld;
  srnn_generate_program(bld, blvm::OP_F32, cus, tune, &w, p, b, sc, eps, u, v, x_out, T, B, S, H, Z, R, kSdEps, kSlope, kLogEps, dp);
  char title[128], head[16] = "";
  if (kind) snprintf(head, sizeof head, " head %d", kind);
  snprintf(title, sizeof title, "srnn S %d B %d H %d Z %d R %d cus %d tune %d scratch %zu%s", S, B, H, Z, R, cus, tune, (size_t)b.end, head);
  dump(title, bld, a);
}
void lstm(int S, int B, int H, int L, int cus) {
  Arrays a;
  BlvmLstmDecodeWeights w{};
  const size_t big = (size_t)4 * H * H + (size_t)S * kDmolF * H + (size_t)H * S;
  for (int i = 0; i < 3; ++i) {
    const std::string n = std::to_string(i);
    w.emb_w[i] = a.add("emb_w" + n, big); w.emb_b[i] = a.add("emb_b" + n, H); w.dec_w[i] = a.add("dec_w" + n, big); w.dec_b[i] = a.add("dec_b" + n, i == 2 ? S * kDmolF : H);
  }
  const float* lay[4][kLstmDecodeMaxLayers] = {};
  for (int l = 0; l < L; ++l) {
    const std::string n = std::to_string(l);
    lay[0][l] = a.add("wih" + n, big); lay[1][l] = a.add("whh" + n, big); lay[2][l] = a.add("bih" + n, 4 * H); lay[3][l] = a.add("bhh" + n, 4 * H);
  }
  w.wih = lay[0]; w.whh = lay[1]; w.bih = lay[2]; w.bhh = lay[3]; w.lik_w = a.add("lik_w", kDmolF * kDmolF); w.lik_b = a.add("lik_b", kDmolF);
  auto p = lstm_pack_table(w, S, H, L);
  const auto b = lstm_decode_layout(p.total, T, B, S, H, L);
  float* sc = a.add("scratch", b.end);
  p.use_staged(sc);
  const float *u = a.add("u", (size_t)T * B * S * kDmolK), *v = a.add("v", (size_t)T * B * S);
  float* x_out = a.add("x_out", (size_t)B * T * S);
  Builder bld;
  lstm_decode_program(bld, blvm::OP_F32, cus, &w, p, b, sc, u, v, x_out, T, B, S, H, L, kLogEps);
  char title[128];
  snprintf(title, sizeof title, "lstm S %d B %d H %d layers %d cus %d scratch %zu", S, B, H, L, cus, (size_t)b.end);
  dump(title, bld, a);
}
}  // namespace

int main(int argc, char** argv) {
  for (int S : {1, 5, 8, 16, 24, 64})
    for (int B : {1, 17, 64, 128})
      for (int cus : {32, 256}) {
        for (int Z : {48, 16}) vrnn(S, B, 48, Z, 32, cus, 0);
        vrnn(S, B, 48, 16, 32, cus, 16);  // the canary bit of pchain_tune
        srnn(S, B, 48, 16, 32, cus, 0);
        srnn(S, B, 48, 16, 32, cus, 16);
        for (int L : {1, 2}) lstm(S, B, 48, L, cus);
      }
  if (argc > 1 && !strcmp(argv[1], "--heads"))
    for (int kind : {1, 2})
      for (int S : {1, 6, 16, 24})
        for (int B : {3, 17}) {
          vrnn(S, B, 48, 16, 32, 256, 0, kind);
          srnn(S, B, 48, 16, 32, 256, 0, kind);
        }
  return 0;
}
