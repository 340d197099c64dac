// The LSTMAudio roll-out's program (csrc/lstm_decode.h, what lstm_decode.hip launches) replayed on the host, word by word: every
// polled word a link reads lies in the sentinel-filled part of the scratch and was prefilled before the launch or written by exactly
// one link earlier in (step, program) order; no word is written twice; every tile of every link has exactly one owner; the c a cell
// tile reads was written by the same descriptor one step earlier (the same workgroup and thread: tile lists are per launch) or
// prefilled; the outputs are written completely; the regions of the scratch layout do not overlap.  A persistent launch whose wiring
// breaks one of these spins until its bound: this runs first, on the CPU, with no GPU call.
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

// one case: the program for (B, L, T) on `cus` CUs; returns the errors
// mutate (the check must bite): 1 the first cell link reads the NEXT step's hidden projection; 2 the draw stores into the slab it came from
int run_case(int B, int L, int T, int cus, bool xcd, int mutate = 0) {
  const int S = 32, H = 48;
  const LstmDecodePack pk = lstm_decode_pack_layout(S, H, L);
  const LstmDecodeBufs b = lstm_decode_layout(pk.total, T, B, S, H, L);
  int bad = 0;
  {  // the layout: regions in ascending order, none overlapping, the weight copies in front, all inside the scratch
    size_t end = 0;
    for (const LstmDecodeRegion& g : pk.regions) { bad += g.off < end || g.off % 4 != 0; end = g.off + g.floats; }
    bad += end > pk.total;
    end = pk.total;
    for (const LstmDecodeRegion& g : b.regions) { bad += g.off < end || g.off % 4 != 0; end = g.off + g.floats; }
    bad += end > b.end || b.regions.size() != (size_t)(7 + 5 * L) || pk.regions.size() != (size_t)(6 + 2 * L);
    bad += !(b.X16 >= pk.total && b.X16 < b.polled_end && b.polled_end <= b.end);
  }
  std::vector<float> scratch(b.end), xout((size_t)B * T * S), dummy(4 * H + S * LD_F + LD_F * LD_F), uu((size_t)T * B * S * LD_K), vv((size_t)T * B * S);
  const float* lay[kLstmDecodeMaxLayers];
  for (int l = 0; l < kLstmDecodeMaxLayers; ++l) lay[l] = dummy.data();
  BlvmLstmDecodeWeights w{};
  for (int i = 0; i < 3; ++i) w.emb_w[i] = w.emb_b[i] = w.dec_w[i] = w.dec_b[i] = dummy.data();
  w.wih = w.whh = w.bih = w.bhh = lay; w.lik_w = w.lik_b = dummy.data();
  Builder bld;
  lstm_decode_program(bld, blvm::OP_F32, cus, &w, pk, b, scratch.data(), uu.data(), vv.data(), xout.data(), T, B, S, H, L, -7.f);
  bld.p.xcd = xcd;
  if (mutate == 1) bld.p.d[3].p[LSTM_GH] += (long)B * 4 * H;
  if (mutate == 2) bld.p.d[bld.p.ndesc - 1].p[DMOLS_X16] -= (long)((B + 15) / 16) * 16 * S;
  const Program& p = bld.p;
  bad += bld.overflow || p.ndesc != 6 + 2 * L || p.S != T || p.B != B;
  Replay r(p, scratch.data(), b.end, b.X16, b.polled_end, xout.data(), xout.size());
  for (const LstmDecodePrefill& f : lstm_decode_prefills(b, S, H, L))
    for (int row = 0; row < B; ++row)
      for (int col = 0; col < f.cols; ++col) r.write(scratch.data() + f.off + (f.t16 ? t16(row, col, f.cols / 16) : (size_t)row * f.cols + col), PRE);
  const int rt = (B + 15) / 16, grid = cus & ~7;
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
        bad += F != LD_F || d.i[DMOLS_I_NMIX] != LD_K || d.i[DMOLS_I_S] != S;
        for (auto [r0, c] : tiles)
          for (int rr = 0; rr < rows_of(r0); ++rr)
            for (int k = 0; k < 4 * F; ++k) r.read(r.at(d, DMOLS_DEC, s) + (size_t)(r0 + rr) * ldd + c * 4 * F + k, true);
        for (auto [r0, c] : tiles)
          for (int rr = 0; rr < rows_of(r0); ++rr)
            for (int ss = 0; ss < 4; ++ss) put_words(r, r.at(d, DMOLS_X, s), d.ld[LD_OUT], r.at(d, DMOLS_X16, s), d.n16[N16_OUT], nullptr, 0, r0 + rr, c * 4 + ss, id);
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
  for (int cus : {256, 32})
    for (int L : {1, 2})
      for (int B : {1, 16, 17, 128})
        for (bool xcd : {false, true}) {
          const int e = run_case(B, L, 3, cus, xcd);
          if (e) printf("B %d layers %d cus %d xcd %d: %d errors\n", B, L, cus, (int)xcd, e);
          bad += e;
          ++cases;
        }
  bad += run_case(17, 2, 3, 256, false, 1) == 0;
  bad += run_case(17, 2, 3, 256, false, 2) == 0;
  printf("lstm decode plan: %d cases, %d errors\n", cases, bad);
  return bad != 0;
}
