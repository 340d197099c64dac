// The LSTMAudio roll-out's program (csrc/lstm_decode.h) for frame stacks that are NO multiple of 16, replayed on the host word by word
// as lstm_decode_plan_test.hip replays the unpadded one.  The frame-stack operand is padded to Sp = 16 ceil(S / 16) columns and the last
// decoder layer's rows to Np = 16 ceil(30 S / 16) floats (pchain.h stack_pad), and a consumer polls EVERY word of an operand block: so
// every pad word must be prefilled or written by exactly one earlier link, every step — a pad column left as a sentinel is a launch
// that spins to its bound.  Checked besides: no word written twice, one owner per tile, x_out complete at width S and nothing stored
// beyond it, u / v / bias reads inside the caller's arrays (the last layer's bias must be the padded copy), the draw tile reads only the
// 16-byte pieces that lie inside a padded row, the regions of the layout disjoint.  No GPU call.
#include "lstm_decode.h"

#include <cstdio>
#include <vector>
namespace blvm {
void set_error(const char*, ...) {}
int pchain_tune() { return 0; }
unsigned long long* pchain_profile_buffer() { return nullptr; }
}  // namespace blvm
using namespace blvm::pchain;

namespace {
constexpr int PRE = -1;  // written by the host before the launch
struct Replay {
  const Program& p;
  const float* sc;
  size_t sc_floats, poll0, poll1;
  const float* xo;
  size_t xo_floats;
  std::vector<int> wsc, wxo;  // writer of every word: 0 none, PRE, or 1 + step * ndesc + link
  int bad = 0;
  Replay(const Program& p_, const float* sc_, size_t n, size_t poll0_, size_t poll1_, const float* xo_, size_t nx)
      : p(p_), sc(sc_), sc_floats(n), poll0(poll0_), poll1(poll1_), xo(xo_), xo_floats(nx), wsc(n, 0), wxo(nx, 0) {}
  const float* at(const Desc& d, int k, int s) const { return d.p[k] ? d.p[k] + (long)s * p.stride[d.sidx[k]] : nullptr; }
  int* slot(const float* q) {
    if (q >= sc && q < sc + sc_floats) return &wsc[q - sc];
    if (q >= xo && q < xo + xo_floats) return &wxo[q - xo];
    ++bad;
    return nullptr;
  }
  void write(const float* q, int id) {
    int* w = slot(q);
    if (!w) return;
    bad += *w != 0;
    *w = id;
  }
  int read(const float* q, bool polled) {  // returns the writer
    int* w = slot(q);
    if (!w) return 0;
    bad += *w == 0;
    if (polled) bad += !(q >= sc + poll0 && q < sc + poll1);
    return *w;
  }
};
inline size_t t16(int row, int col, int n16) {
  return ((size_t)(row >> 4) * n16 + (col >> 4)) * 256 + ((row & 15) + 16 * ((col & 15) >> 2)) * 4 + (col & 3);
}
void put_words(Replay& r, const float* rm, int ld, const float* x16, int n16, const float* x16b, int n16b, int row, int col, int id) {
  if (rm) r.write(rm + (size_t)row * ld + col, id);
  if (x16) r.write(x16 + t16(row, col, n16), id);
  if (x16b) r.write(x16b + t16(row, col, n16b), id);
}

// one case: the program for (S, B, L, T) on `cus` CUs; returns the errors
// mutate (the check must bite): 1 the draw link covers the live samples only (ceil(S / 4) tiles: the operand's pad columns stay
// sentinels); 2 the last decoder layer reads the caller's bias [30 S] (past its end in the ragged tile)
int run_case(int S, int B, int L, int T, int cus, bool xcd, int mutate = 0) {
  const int H = 48;
  const blvm::StackPad sp = blvm::stack_pad(S, LD_F);
  const int Sp = sp.Sp, N = sp.N, Np = sp.Np;
  const LstmDecodePack pk = lstm_decode_pack_layout(S, H, L);
  const LstmDecodeBufs b = lstm_decode_layout(pk.total, T, B, S, H, L);
  int bad = 0;
  {  // the layout: regions in ascending order, none overlapping, the weight copies in front, all inside the scratch
    size_t end = 0;
    for (const LstmDecodeRegion& g : pk.regions) { bad += g.off < end || g.off % 4 != 0; end = g.off + g.floats; }
    bad += end > pk.total;
    end = pk.total;
    for (const LstmDecodeRegion& g : b.regions) { bad += g.off < end || g.off % 4 != 0; end = g.off + g.floats; }
    bad += end > b.end || b.regions.size() != (size_t)(7 + 5 * L) || pk.regions.size() != (size_t)(6 + 2 * L + (sp.padded() ? 3 : 0));
    bad += Sp % 16 != 0 || Np % 16 != 0 || Sp < S || Np < N || Sp - S >= 16 || Np - N >= 16 || sp.padded() != (S % 16 != 0);
    bad += !(b.X16 >= pk.total && b.X16 < b.polled_end && b.polled_end <= b.end);
  }
  // (the arrays the caller owns have their exact sizes: a read past an end is an error)
  std::vector<float> scratch(b.end), xout((size_t)B * T * S), dummy(4 * H + LD_F * LD_F), bH(H), bN(N), uu((size_t)T * B * S * LD_K), vv((size_t)T * B * S);
  const float* lay[kLstmDecodeMaxLayers];
  for (int l = 0; l < kLstmDecodeMaxLayers; ++l) lay[l] = dummy.data();
  BlvmLstmDecodeWeights w{};
  for (int i = 0; i < 3; ++i) { w.emb_w[i] = w.dec_w[i] = dummy.data(); w.emb_b[i] = w.dec_b[i] = bH.data(); }
  w.dec_b[2] = bN.data();
  w.wih = w.whh = w.bih = w.bhh = lay; w.lik_w = w.lik_b = dummy.data();
  Builder bld;
  lstm_decode_program(bld, blvm::OP_F32, cus, &w, pk, b, scratch.data(), uu.data(), vv.data(), xout.data(), T, B, S, H, L, -7.f);
  bld.p.xcd = xcd;
  if (mutate == 1) bld.p.d[bld.p.ndesc - 1].ct = (S + 3) / 4;
  if (mutate == 2) bld.p.d[bld.p.ndesc - 2].p[LIN_BIAS] = w.dec_b[2];
  const Program& p = bld.p;
  bad += bld.overflow || p.ndesc != 6 + 2 * L || p.S != T || p.B != B;
  Replay r(p, scratch.data(), b.end, b.X16, b.polled_end, xout.data(), xout.size());
  for (const LstmDecodePrefill& f : lstm_decode_prefills(b, S, H, L))
    for (int row = 0; row < B; ++row)
      for (int col = 0; col < f.cols; ++col)  // (columns >= f.src_cols are the zeros of the padded stack: written all the same)
        r.write(scratch.data() + f.off + (f.t16 ? t16(row, col, f.cols / 16) : (size_t)row * f.cols + col), PRE);
  for (const LstmDecodePrefill& f : lstm_decode_prefills(b, S, H, L)) bad += f.src_cols > f.cols || (f.src == LstmDecodePrefill::X0 && (f.cols != Sp || f.src_cols != S));
  const int rt = (B + 15) / 16, grid = cus & ~7;
  // a bias of `n` floats must lie inside the scratch or inside one of the caller's arrays
  auto bias_ok = [&](const float* q, int n) {
    auto in = [&](const std::vector<float>& a) { return q >= a.data() && q + n <= a.data() + a.size(); };
    return in(scratch) || in(bH) || in(bN) || in(dummy);
  };
  for (int s = 0; s < T; ++s)
    for (int i = 0; i < p.ndesc; ++i) {
      const Desc& d = p.d[i];
      const int id = 1 + s * p.ndesc + i;
      bad += d.wg0 < 0 || d.nwg <= 0 || d.wg0 + d.nwg > grid || d.s_begin != 0 || d.s_end != T;
      // the tiles, each with exactly one owner
      std::vector<int> cnt(rt * d.ct, 0);
      std::vector<std::pair<int, int>> tiles;
      for (int wg = 0; wg < grid; ++wg)
        for (TileIter it(wg, d.wg0, d.nwg, rt, d.ct, p.xcd != 0); it.valid(); it.next()) {
          const int tr = it.r0() / 16, c = it.c();
          if (tr < 0 || tr >= rt || c < 0 || c >= d.ct) { ++bad; continue; }
          cnt[c * rt + tr]++;
          tiles.push_back({it.r0(), c});
        }
      for (int v : cnt) bad += v != 1;
      auto rows_of = [&](int r0) { return std::min(16, B - r0); };
      auto read_slab = [&](const float* A, int r0, int K, int n16) {  // the polled T16 operand of a product
        for (int rr = 0; rr < rows_of(r0); ++rr)
          for (int k = 0; k < K; ++k) r.read(A + t16(r0 + rr, k, n16), true);
      };
      if (d.kind == K_LIN) {
        const int n16a = (d.ld[LIN_LD_A] > 0 ? d.ld[LIN_LD_A] : d.K) / 16;
        bad += (d.flags & (DF_A_PLAIN | DF_A_SUM3 | DF_ADD_POLLED)) != 0 || r.at(d, LIN_ADD, s) != nullptr || r.at(d, LIN_GATE, s) != nullptr;
        bad += !bias_ok(d.p[LIN_BIAS], d.ct * 16);  // a tile reads bias[col] of all its 16 columns
        if (i == 0) bad += d.K != Sp;
        if (i == p.ndesc - 2) bad += d.ct * 16 != Np || d.ld[LD_OUT] != Np;
        for (auto [r0, c] : tiles) read_slab(r.at(d, LIN_A, s), r0, d.K, n16a);
        for (auto [r0, c] : tiles)
          for (int rr = 0; rr < rows_of(r0); ++rr)
            for (int cc = 0; cc < 16; ++cc)
              put_words(r, r.at(d, LIN_ORM, s), d.ld[LD_OUT], r.at(d, LIN_O16, s), d.n16[N16_OUT], r.at(d, LIN_O16B, s), d.n16[N16_OUTB], r0 + rr, c * 16 + cc, id);
      } else if (d.kind == K_LINSEQ) {
        const float* A = r.at(d, LINSEQ_A0, s);
        bad += d.i[LINSEQ_I_K0] != 0 || r.at(d, LINSEQ_ADD0, s) != nullptr;
        for (int li = 0; li < d.i[LINSEQ_I_N]; ++li) {  // links outside, tiles inside, as the interpreter runs a run
          for (auto [r0, c] : tiles) read_slab(A, r0, d.K, d.K / 16);
          for (auto [r0, c] : tiles)
            for (int rr = 0; rr < rows_of(r0); ++rr)
              for (int cc = 0; cc < 16; ++cc)
                put_words(r, r.at(d, LINSEQ_ORM + li, s), d.ld[LINSEQ_LD_ORM + li], r.at(d, LINSEQ_O16 + li, s), d.n16[N16_OUT], nullptr, 0, r0 + rr, c * 16 + cc, id);
          A = r.at(d, LINSEQ_O16 + li, s);
        }
      } else if (d.kind == K_LSTM) {
        const int Hh = d.i[LSTM_I_H];
        bad += Hh != H;
        for (auto [r0, c] : tiles) {
          read_slab(r.at(d, LSTM_X16, s), r0, d.K, d.K / 16);
          for (int rr = 0; rr < rows_of(r0); ++rr)
            for (int cc = 0; cc < 16; ++cc) {
              const int row = r0 + rr, col = c * 16 + cc;
              for (int g = 0; g < 4; ++g) r.read(r.at(d, LSTM_GH, s) + (size_t)row * 4 * Hh + g * Hh + col, true);
              const int wr = r.read(r.at(d, LSTM_CPREV, s) + (size_t)row * Hh + col, false);
              bad += !(wr == PRE || wr == id - p.ndesc);  // this very tile, one step earlier
            }
        }
        for (auto [r0, c] : tiles)
          for (int rr = 0; rr < rows_of(r0); ++rr)
            for (int cc = 0; cc < 16; ++cc) {
              const int row = r0 + rr, col = c * 16 + cc;
              r.write(r.at(d, LSTM_CNEXT, s) + (size_t)row * Hh + col, id);
              put_words(r, r.at(d, LSTM_HRM, s), d.ld[LD_OUT], r.at(d, LSTM_H16, s), d.n16[N16_OUT], r.at(d, LSTM_H16B, s), d.n16[N16_OUTB], row, col, id);
            }
      } else if (d.kind == K_DMOLS) {  // a tile: 16 rows x 4 samples
        const int F = d.i[DMOLS_I_F], ldd = d.ld[DMOLS_LD_DEC];
        bad += F != LD_F || d.i[DMOLS_I_NMIX] != LD_K || d.i[DMOLS_I_S] != S || ldd != Np || d.n16[N16_OUT] != Sp / 16 || d.ld[LD_OUT] != T * S;
        for (auto [r0, c] : tiles)
          for (int rr = 0; rr < rows_of(r0); ++rr)
            for (int k = 0; k < 4 * F; ++k) {  // 16-byte pieces: one past the padded row's end is neither read nor checked
              const int cd = c * 4 * F + (k & ~3);
              if (cd < ldd) r.read(r.at(d, DMOLS_DEC, s) + (size_t)(r0 + rr) * ldd + c * 4 * F + k, true);
              else bad += c * 4 + k / F < S;  // ... and it belongs to no live sample
            }
        for (auto [r0, c] : tiles)
          for (int rr = 0; rr < rows_of(r0); ++rr)
            for (int ss = 0; ss < 4; ++ss) {
              const int row = r0 + rr, smp = c * 4 + ss;
              const bool live = smp < S;  // a live sample reads its u and v and stores x; a pad column gets its zero in the T16 slab only
              if (live) {
                const float* uq = r.at(d, DMOLS_U, s) + ((size_t)row * S + smp) * LD_K;
                const float* vq = r.at(d, DMOLS_V, s) + (size_t)row * S + smp;
                bad += !(uq >= uu.data() && uq + LD_K <= uu.data() + uu.size()) || !(vq >= vv.data() && vq < vv.data() + vv.size());
              }
              bad += smp >= Sp;
              put_words(r, live ? r.at(d, DMOLS_X, s) : nullptr, d.ld[LD_OUT], r.at(d, DMOLS_X16, s), d.n16[N16_OUT], nullptr, 0, row, smp, id);
            }
      } else {
        ++bad;  // a kind the roll-out kernel does not have
      }
    }
  bad += r.bad;
  // what the caller gets back is written completely: x_out, and per layer the last h and c slabs
  for (int v : r.wxo) bad += v <= 0;
  for (int l = 0; l < L; ++l)
    for (size_t e = 0; e < (size_t)B * H; ++e) bad += r.wsc[b.HS[l] + (size_t)(T - 1) * B * H + e] <= 0 || r.wsc[b.CS[l] + (size_t)T * B * H + e] <= 0;
  return bad;
}
}  // namespace

int main() {
  int bad = 0, cases = 0;
  for (int S : {1, 5, 8, 24})
    for (int cus : {256, 32})
      for (int L : {1, 2})
        for (int B : {1, 17})
          for (bool xcd : {false, true}) {
            const int e = run_case(S, B, L, 3, cus, xcd);
            if (e) printf("S %d B %d layers %d cus %d xcd %d: %d errors\n", S, B, L, cus, (int)xcd, e);
            bad += e;
            ++cases;
          }
  for (int S : {1, 5, 8, 24}) bad += run_case(S, 17, 2, 3, 256, false, 1) == 0;  // every S has pad columns in its operand
  for (int S : {1, 5}) bad += run_case(S, 17, 2, 3, 256, false, 2) == 0;           // ... and these a ragged last decoder tile
  bad += run_case(16, 17, 1, 3, 256, false) != 0;  // a multiple of 16: nothing padded, the same checks hold
  printf("lstm decode ragged plan: %d cases, %d errors\n", cases, bad);
  return bad != 0;
}
