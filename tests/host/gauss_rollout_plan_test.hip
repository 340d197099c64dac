// The roll-out plans of the GMM (kind 1) and Gaussian (kind 2) heads (csrc/rollout_plan.h: DrawPlan, draw_plan, add_tail) for the
// VRNNAudio and SRNNAudio programs, on the host.  Per (model, kind, S, B): the padded sizes Sp and Np of the head's F, the pack table
// and the layout built on them, the draw link's descriptor (S, F, num_mix, kind, sd_beta, sd_eps; the strides of dec, u, v and the
// frame-stack slab), the floats of LDS the tile needs against what the launch gives it, and every 16-byte piece the tile reads against
// the dec slab.  Kind 1 (F = 30, as the DMoL head) is also replayed word by word (rollout_replay.h).  Kind 0 through draw_plan is,
// field for field, the program the defaulted arguments build (what the entry points without a head launch), and the heads the tile
// does not draw are refused.  Prints `scratch <model> <kind> <T> <B> <S> <floats>` per case for tests/test_gauss_rollout_cpu.py to hold
// against the library's *_scratch_floats_head.  No GPU call; also built with the address and undefined-behaviour sanitizers.
#include <cstring>

#include "rollout_replay.h"

namespace {
constexpr int H = 48, Z = 16, R = 32, T = 3, CUS = 256;
constexpr float kSdBeta = 0.6931f, kHeadEps = 1e-4f;

struct Built {
  Builder bld;
  PackTable pk;
  std::vector<Region> regions;
  size_t X16, DEC, polled_end, end, dummy0;
  std::vector<float> scratch, bH, b2Z, b3R, bN, lik, eps, uu, vv, xout, wts;
  std::vector<Prefill> prefills;
  size_t state_out;  // the slab the final state is copied from
};

// the program of `srnn ? SRNNAudio : VRNNAudio` for head dp at (S, B); head == nullptr: the defaulted arguments
void build(Built& o, bool srnn, const DrawPlan* head, int S, int B) {
  const DrawPlan dp = head ? *head : DrawPlan{};
  const blvm::StackPad sp = blvm::stack_pad(S, dp.F);
  o.wts.assign(1, 0.f); o.bH.assign(H, 0.f); o.b2Z.assign(2 * Z, 0.f); o.b3R.assign(3 * R, 0.f); o.bN.assign(sp.N, 0.f); o.lik.assign(dp.F * dp.F, 0.f);
  o.eps.assign((size_t)T * B * Z, 0.f); o.uu.assign((size_t)T * B * S * dp.K + 1, 0.f); o.vv.assign((size_t)T * B * S, 0.f); o.xout.assign((size_t)B * T * S, 0.f);
  const float* u = dp.K ? o.uu.data() : nullptr;
  static BlvmVrnnWeights vc;
  static BlvmSrnnWeights sc_;
  static BlvmVrnnDecodeWeights vw;
  static BlvmSrnnDecodeWeights sw;
  if (!srnn) {
    vc = BlvmVrnnWeights{}; vw = BlvmVrnnDecodeWeights{};
    for (int i = 0; i < 3; ++i) { vw.enc_w[i] = vw.dec_w[i] = vc.prior_w[i] = o.wts.data(); vw.enc_b[i] = vw.dec_b[i] = vc.prior_b[i] = o.bH.data(); }
    for (int i = 0; i < 4; ++i) { vc.phi_w[i] = o.wts.data(); vc.phi_b[i] = o.bH.data(); }
    vw.dec_b[2] = o.bN.data(); vc.prior_hw = vc.gru_wih = vc.gru_whh = o.wts.data(); vc.prior_hb = o.b2Z.data(); vc.gru_bih = vc.gru_bhh = o.b3R.data();
    vw.lik_w = vw.lik_b = o.lik.data(); vw.cell = &vc;
    o.pk = head ? vrnn_pack_table(vw, vc, S, H, Z, R, dp.F) : vrnn_pack_table(vw, vc, S, H, Z, R);
    const VrnnBufs b = head ? vrnn_generate_layout(o.pk.total, T, B, S, H, Z, R, dp.F) : vrnn_generate_layout(o.pk.total, T, B, S, H, Z, R);
    o.regions = b.regions; o.X16 = b.X16; o.DEC = b.DEC; o.polled_end = b.polled_end; o.end = b.end; o.dummy0 = b.dummyZ;
    o.scratch.assign(b.end, 0.f);
    o.pk.use_staged(o.scratch.data());
    if (head) vrnn_generate_program(o.bld, blvm::OP_F32, CUS, 0, &vw, o.pk, b, o.scratch.data(), o.eps.data(), u, o.vv.data(), o.xout.data(), T, B, S, H, Z, R, 1e-6f, 0.01f, -7.f, dp);
    else vrnn_generate_program(o.bld, blvm::OP_F32, CUS, 0, &vw, o.pk, b, o.scratch.data(), o.eps.data(), u, o.vv.data(), o.xout.data(), T, B, S, H, Z, R, 1e-6f, 0.01f, -7.f);
    o.prefills = vrnn_generate_prefills(b, S, R);
    o.state_out = b.HS + (size_t)T * B * R;
  } else {
    sc_ = BlvmSrnnWeights{}; sw = BlvmSrnnDecodeWeights{};
    for (int i = 0; i < 3; ++i) { sw.enc_w[i] = sw.dec_w[i] = sc_.prior_w[i] = o.wts.data(); sw.enc_b[i] = sw.dec_b[i] = sc_.prior_b[i] = o.bH.data(); }
    sw.dec_b[2] = o.bN.data(); sc_.prior_hw = sw.gru_wih = sw.gru_whh = o.wts.data(); sc_.prior_hb = o.b2Z.data(); sw.gru_bih = sw.gru_bhh = o.b3R.data();
    sw.lik_w = sw.lik_b = o.lik.data(); sw.chain = &sc_;
    o.pk = head ? srnn_pack_table(sw, sc_, S, H, Z, R, dp.F) : srnn_pack_table(sw, sc_, S, H, Z, R);
    const SrnnBufs b = head ? srnn_generate_layout(o.pk.total, T, B, S, H, Z, R, dp.F) : srnn_generate_layout(o.pk.total, T, B, S, H, Z, R);
    o.regions = b.regions; o.X16 = b.X16; o.DEC = b.DEC; o.polled_end = b.polled_end; o.end = b.end; o.dummy0 = b.dummyZ;
    o.scratch.assign(b.end, 0.f);
    o.pk.use_staged(o.scratch.data());
    if (head) srnn_generate_program(o.bld, blvm::OP_F32, CUS, 0, &sw, o.pk, b, o.scratch.data(), o.eps.data(), u, o.vv.data(), o.xout.data(), T, B, S, H, Z, R, 1e-6f, 0.01f, -7.f, dp);
    else srnn_generate_program(o.bld, blvm::OP_F32, CUS, 0, &sw, o.pk, b, o.scratch.data(), o.eps.data(), u, o.vv.data(), o.xout.data(), T, B, S, H, Z, R, 1e-6f, 0.01f, -7.f);
    o.prefills = srnn_generate_prefills(b, B, S, Z, R);
    o.state_out = b.DS + (size_t)T * B * R;
  }
}

int run_case(bool srnn, int kind, int S, int B) {
  DrawPlan dp;
  int bad = draw_plan(kind, kDmolK, kSdBeta, kHeadEps, &dp) != nullptr;
  const int F = kind == DRAW_GAUSS ? 2 : 30, K = kind == DRAW_GAUSS ? 0 : 10;
  bad += dp.kind != kind || dp.F != F || dp.K != K || dp.sd_beta != kSdBeta || dp.sd_eps != kHeadEps;
  Built o;
  build(o, srnn, &dp, S, B);
  // the geometry
  const int Sp = (S + 15) / 16 * 16, Np = S % 16 ? (S * F + 15) / 16 * 16 : S * F, rows = (B + 15) / 16 * 16;
  const blvm::StackPad& sp = o.pk.sp;
  bad += sp.S != S || sp.Sp != Sp || sp.N != S * F || sp.Np != Np || Np % 16 != 0 || Sp % 16 != 0;
  bad += o.pk.e[o.pk.first].k != Sp || o.pk.e[o.pk.last].rows != Np || o.pk.e[o.pk.last].k != H;
  bad += check_regions(o.pk.regions, o.pk.total, o.regions, o.end, o.X16, o.polled_end);
  for (const Region& g : o.regions) {
    if (!strcmp(g.name, "X16")) bad += g.floats != (size_t)(T + 1) * rows * Sp;
    if (!strcmp(g.name, "DEC")) bad += g.floats != (size_t)T * B * Np || g.off != o.DEC;
  }
  if (sp.padded()) bad += o.pk.stage_dec + (size_t)Np * H > o.pk.total || o.pk.stage_bias + Np > o.pk.total;
  // the last two links: the last decoder layer over Np columns, then the draw
  const Program& p = o.bld.p;
  bad += o.bld.overflow || p.ndesc < 3 || p.S != T || p.B != B;
  const Desc& lin = p.d[p.ndesc - 2];
  const Desc& d = p.d[p.ndesc - 1];
  bad += lin.kind != K_LIN || lin.ct != Np / 16 || lin.ld[LD_OUT] != Np || lin.p[LIN_ORM] != o.scratch.data() + o.DEC || p.stride[lin.sidx[LIN_ORM]] != (long)B * Np;
  bad += d.kind != K_DMOLS || d.ct != Sp / 4 || d.i[DMOLS_I_S] != S || d.i[DMOLS_I_F] != F || d.i[DMOLS_I_NMIX] != K || d.i[DMOLS_I_HEAD] != kind;
  bad += d.f[DMOLS_F_SD_BETA] != kSdBeta || d.f[DMOLS_F_SD_EPS] != kHeadEps || d.ld[DMOLS_LD_DEC] != Np || d.n16[N16_OUT] != Sp / 16 || d.ld[LD_OUT] != T * S;
  bad += d.p[DMOLS_DEC] != o.scratch.data() + o.DEC || p.stride[d.sidx[DMOLS_DEC]] != (long)B * Np;
  bad += K ? (d.p[DMOLS_U] != o.uu.data() || p.stride[d.sidx[DMOLS_U]] != (long)B * S * K) : (d.p[DMOLS_U] != nullptr || d.sidx[DMOLS_U] != 0);
  bad += d.p[DMOLS_V] != o.vv.data() || (T * B * S > 0 && p.stride[d.sidx[DMOLS_V]] != (long)B * S);
  bad += d.p[DMOLS_X] != o.xout.data() || p.stride[d.sidx[DMOLS_X]] != S;
  bad += d.p[DMOLS_X16] != o.scratch.data() + o.X16 + (size_t)rows * Sp || p.stride[d.sidx[DMOLS_X16]] != (long)rows * Sp;
  bad += d.p[DMOLS_W] != o.lik.data() || d.p[DMOLS_B] != o.lik.data();
  // the tile's LDS: [16][4 F] head inputs + [64][32] head outputs, inside one reduction buffer of the launch (lds_products x 16 waves x 256)
  bad += 16 * 4 * F + 64 * 32 > p.lds_products * 16 * 256 || F > 32;
  // every 16-byte piece a tile reads lies inside its row of the dec slab, a live sample's F inputs inside the pieces that are read
  for (int s0 = 0; s0 < Sp; s0 += 4)
    for (int row = 0; row < B; ++row)
      for (int cq = 0; cq < F; ++cq) {  // 4 F / 4 pieces per tile row
        const int cd = s0 * F + 4 * cq;
        if (cd < Np) bad += cd % 4 != 0 || cd + 4 > Np || (size_t)row * Np + cd + 4 > (size_t)B * Np;
        else bad += s0 + (4 * cq) / F < S;
      }
  for (int smp = 0; smp < S; ++smp) bad += smp * F + F > Np;
  // the last step's last draw stays inside u, v and x_out
  bad += K && (size_t)(T - 1) * B * S * K + ((size_t)(B - 1) * S + S - 1) * K + K > o.uu.size();
  bad += (size_t)(T - 1) * B * S + (size_t)(B - 1) * S + S > o.vv.size() || (size_t)(B - 1) * T * S + (size_t)(T - 1) * S + S > o.xout.size();
  if (kind == DRAW_GMM) {  // the word-by-word replay (F = 30: the geometry the replay knows)
    Replay r(p, o.scratch, o.X16, o.polled_end, o.xout);
    r.dummy0 = o.dummy0; r.dummy1 = o.end;
    for (const std::vector<float>* a : {&o.bH, &o.b2Z, &o.b3R, &o.bN, &o.lik, &o.eps, &o.uu, &o.vv}) r.own(*a);
    replay_prefills(r, o.prefills, B);
    replay_program(r, T, B, S, H, CUS);
    bad += r.bad;
    for (size_t k = 0; k < (size_t)B * R; ++k) bad += r.wsc[o.state_out + k] == 0;
  }
  printf("scratch %s %d %d %d %d %zu\n", srnn ? "srnn" : "vrnn", kind, T, B, S, o.end);
  return bad;
}

bool same_desc(const Desc& a, const Desc& b) {
  bool same = a.kind == b.kind && a.ct == b.ct && a.wg0 == b.wg0 && a.nwg == b.nwg && a.flags == b.flags && a.K == b.K && a.s_begin == b.s_begin && a.s_end == b.s_end;
  same = same && !memcmp(a.ld, b.ld, sizeof a.ld) && !memcmp(a.n16, b.n16, sizeof a.n16) && !memcmp(a.i, b.i, sizeof a.i) && !memcmp(a.f, b.f, sizeof a.f);
  return same && !memcmp(a.sidx, b.sidx, sizeof a.sidx);
}
// kind 0 through draw_plan against the defaulted arguments: every field, pointers as offsets into each build's own arrays
int kind0_case(bool srnn, int S, int B) {
  DrawPlan dp;
  int bad = draw_plan(DRAW_DMOL, kDmolK, 0.25f, 0.5f, &dp) != nullptr;  // (a DMoL head's sd fields are not read: the plan drops them)
  Built a, b;
  build(a, srnn, nullptr, S, B);
  build(b, srnn, &dp, S, B);
  const Program &p = a.bld.p, &q = b.bld.p;
  bad += p.ot != q.ot || p.rt_group != q.rt_group || p.s_first != q.s_first || p.ndesc != q.ndesc || p.S != q.S || p.B != q.B || p.xcd != q.xcd ||
         p.prof_wg != q.prof_wg || p.lds_products != q.lds_products || a.bld.nstride != b.bld.nstride || memcmp(p.stride, q.stride, sizeof p.stride) != 0;
  bad += a.end != b.end || a.pk.total != b.pk.total || a.X16 != b.X16 || a.DEC != b.DEC || a.polled_end != b.polled_end;
  auto where = [](const Built& o, const float* ptr) -> long {
    if (!ptr) return -1;
    const std::vector<float>* arrays[] = {&o.scratch, &o.bH, &o.b2Z, &o.b3R, &o.bN, &o.lik, &o.eps, &o.uu, &o.vv, &o.xout, &o.wts};
    long base = 0;
    for (const std::vector<float>* v : arrays) {
      if (ptr >= v->data() && ptr <= v->data() + v->size()) return base + (ptr - v->data());
      base += (long)v->size() + 1;
    }
    return -2;
  };
  for (int i = 0; i < p.ndesc && i < q.ndesc; ++i) {
    bad += !same_desc(p.d[i], q.d[i]);
    for (int k = 0; k < kMaxPtr; ++k) bad += where(a, p.d[i].p[k]) != where(b, q.d[i].p[k]) || where(a, p.d[i].p[k]) == -2;
  }
  const Desc& d = q.d[q.ndesc - 1];
  bad += d.i[DMOLS_I_HEAD] != 0 || d.f[DMOLS_F_SD_BETA] != 0.f || d.f[DMOLS_F_SD_EPS] != 0.f || d.f[DMOLS_F_LOG_EPS] != -7.f;
  return bad;
}
}  // namespace

int main() {
  int bad = 0, cases = 0;
  for (bool srnn : {false, true})
    for (int kind : {(int)DRAW_GMM, (int)DRAW_GAUSS})
      for (int S : {1, 6, 16, 24})
        for (int B : {3, 17}) {
          const int e = run_case(srnn, kind, S, B);
          if (e) printf("%s kind %d S %d B %d: %d errors\n", srnn ? "srnn" : "vrnn", kind, S, B, e);
          bad += e;
          ++cases;
        }
  for (bool srnn : {false, true})
    for (int S : {1, 6, 16, 24}) {
      const int e = kind0_case(srnn, S, 17);
      if (e) printf("%s kind 0 S %d: %d differences from the defaulted program\n", srnn ? "srnn" : "vrnn", S, e);
      bad += e;
      ++cases;
    }
  // what the tile does not draw is refused, whatever else is given
  DrawPlan dp;
  bad += draw_plan(3, 10, 1.f, 0.f, &dp) == nullptr || draw_plan(-1, 10, 1.f, 0.f, &dp) == nullptr;
  bad += draw_plan(DRAW_DMOL, 5, 0.f, 0.f, &dp) == nullptr || draw_plan(DRAW_GMM, 5, 1.f, 0.f, &dp) == nullptr || draw_plan(DRAW_GMM, 11, 1.f, 0.f, &dp) == nullptr;
  bad += draw_plan(DRAW_GMM, 10, -1.f, 0.f, &dp) == nullptr || draw_plan(DRAW_GAUSS, 0, -0.5f, 0.f, &dp) == nullptr;
  bad += draw_plan(DRAW_GAUSS, 0, 0.f, 0.f, &dp) != nullptr || draw_plan(DRAW_GAUSS, 7, 1.f, 1e-4f, &dp) != nullptr;  // (the Gaussian head has no num_mix)
  const float one = 1.f;
  DrawPlan gmm, gauss;
  draw_plan(DRAW_GMM, 10, 1.f, 0.f, &gmm); draw_plan(DRAW_GAUSS, 0, 1.f, 0.f, &gauss);
  bad += !draw_streams_ok(gmm, &one, &one) || !draw_streams_ok(gmm, nullptr, nullptr) || draw_streams_ok(gmm, &one, nullptr) || draw_streams_ok(gmm, nullptr, &one);
  bad += !draw_streams_ok(gauss, nullptr, &one) || !draw_streams_ok(gauss, nullptr, nullptr) || draw_streams_ok(gauss, &one, &one);
  printf("gauss rollout plan: %d cases, %d errors\n", cases, bad);
  return bad != 0;
}
