// rollout_replay.h — the host replay of a one-launch roll-out's step program (csrc/rollout_plan.h, csrc/lstm_decode.h), shared by the
// four plan tests in this directory.  A program is walked word by word in (step, link) order:
//   every polled word a link reads lies in the sentinel-filled part of the scratch and was prefilled before the launch or written by
//   exactly one earlier link; no word is written twice, except in the layout's dummy regions (gates and statistics nobody reads:
//   they lie outside the polled range and no link may read them); every tile of every link has exactly one owner; a state a cell tile
//   reads (c of K_LSTM, h_prev of K_GRU) was prefilled or written by the same descriptor one step earlier; x_out is stored at width S
//   and nothing beyond it; reads of u, v, eps and every bias stay inside the caller's arrays or the scratch; the draw tile reads only
//   the 16-byte pieces that lie inside a padded row.
// A persistent launch whose wiring breaks one of these spins until its poll bound: this runs first, on the CPU, with no GPU call.
#pragma once
#include <cstdio>
#include <utility>
#include <vector>

#include "rollout_plan.h"

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
  size_t sc_floats, poll0, poll1, dummy0 = 0, dummy1 = 0;  // [dummy0, dummy1): the layout's dummy regions
  const float* xo;
  size_t xo_floats;
  std::vector<int> wsc, wxo;  // writer of every word: 0 none, PRE, or 1 + step * ndesc + link
  std::vector<std::pair<const float*, size_t>> owned;  // the caller's read-only arrays (exact sizes: a read past an end is an error)
  int bad = 0;
  Replay(const Program& p_, const std::vector<float>& scratch, size_t poll0_, size_t poll1_, const std::vector<float>& xout)
      : p(p_), sc(scratch.data()), sc_floats(scratch.size()), poll0(poll0_), poll1(poll1_), xo(xout.data()), xo_floats(xout.size()), wsc(scratch.size(), 0),
        wxo(xout.size(), 0) {}
  void own(const std::vector<float>& a) { owned.push_back({a.data(), a.size()}); }
  const float* at(const Desc& d, int k, int s) const { return d.p[k] ? d.p[k] + (long)s * p.stride[d.sidx[k]] : nullptr; }
  bool in_dummy(const float* q) const { return q >= sc + dummy0 && q < sc + dummy1; }
  int* slot(const float* q) {
    if (q >= sc && q < sc + sc_floats) return &wsc[q - sc];
    if (q >= xo && q < xo + xo_floats) return &wxo[q - xo];
    ++bad;
    return nullptr;
  }
  void write(const float* q, int id) {
    int* w = slot(q);
    if (!w) return;
    bad += *w != 0 && !in_dummy(q);
    *w = id;
  }
  int read(const float* q, bool polled) {  // returns the writer
    int* w = slot(q);
    if (!w) return 0;
    bad += *w == 0 || in_dummy(q);
    if (polled) bad += !(q >= sc + poll0 && q < sc + poll1);
    return *w;
  }
  // `n` floats at q that the launch only reads: inside one of the caller's arrays or (a bias: the padded copy) inside the scratch
  bool readable(const float* q, size_t n, bool scratch_too = true) const {
    if (scratch_too && q >= sc && q + n <= sc + sc_floats) return true;
    for (const auto& [a, m] : owned)
      if (q >= a && q + n <= a + m) return true;
    return false;
  }
};
inline size_t t16(int row, int col, int n16) {
  return ((size_t)(row >> 4) * n16 + (col >> 4)) * 256 + ((row & 15) + 16 * ((col & 15) >> 2)) * 4 + (col & 3);
}
inline void put_words(Replay& r, const float* rm, int ld, const float* x16, int n16, const float* x16b, int n16b, int row, int col, int id) {
  if (rm) r.write(rm + (size_t)row * ld + col, id);
  if (x16) r.write(x16 + t16(row, col, n16), id);
  if (x16b) r.write(x16b + t16(row, col, n16b), id);
}

// the layout: regions in ascending order, none overlapping, the weight copies in front, all inside the scratch; returns the errors
inline int check_regions(const std::vector<Region>& packs, size_t pack_total, const std::vector<Region>& bufs, size_t end_all, size_t X16, size_t polled_end) {
  int bad = 0;
  size_t end = 0;
  for (const Region& g : packs) { bad += g.off < end || g.off % 4 != 0; end = g.off + g.floats; }
  bad += end > pack_total;
  end = pack_total;
  for (const Region& g : bufs) { bad += g.off < end || g.off % 4 != 0; end = g.off + g.floats; }
  bad += end > end_all;
  bad += !(X16 >= pack_total && X16 < polled_end && polled_end <= end_all);
  return bad;
}
// the prefills of a layout, as the entry point writes them (columns >= src_cols are the zeros of the padded stack: written all the same)
inline void replay_prefills(Replay& r, const std::vector<blvm::pchain::Prefill>& list, int B) {
  for (const Prefill& f : list) {
    r.bad += f.src_cols > f.cols || f.cols % 16 != 0;
    for (int row = 0; row < B; ++row)
      for (int col = 0; col < f.cols; ++col) r.write(r.sc + f.off + (f.t16 ? t16(row, col, f.n16 ? f.n16 : f.cols / 16) : (size_t)row * f.cols + col), PRE);
  }
}

// The program of r for T steps of B utterances at stack S and width H on `cus` CUs; errors go to r.bad.  In every roll-out the first
// link takes the padded frame stack in (K = Sp), the last but one is the last decoder layer (Np columns) and the last the draw.
inline void replay_program(Replay& r, int T, int B, int S, int H, int cus) {
  const Program& p = r.p;
  const blvm::StackPad sp = blvm::stack_pad(S, kDmolF);
  const int Sp = sp.Sp, Np = sp.Np;
  const int rt = (B + 15) / 16, grid = cus & ~7;
  int& bad = r.bad;
  bad += p.ndesc < 3 || p.d[p.ndesc - 1].kind != K_DMOLS || p.d[p.ndesc - 2].kind != K_LIN || p.d[0].kind != K_LIN;
  bad += r.dummy0 < r.dummy1 && !(r.dummy0 >= r.poll1 || r.dummy1 <= r.poll0);
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
        bad += !r.readable(d.p[LIN_BIAS], d.ct * 16);  // a tile reads bias[col] of all its 16 columns
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
          bad += !r.readable(d.p[LINSEQ_AUX + li], d.ct * 16);
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
      } else if (d.kind == K_GRU) {  // tile_gru: X16 [rows, K], 3 words of gh and h_prev per element (polled); h_new three ways, the gates to a dummy
        const int R = d.i[GRU_I_R];
        bad += d.ct * 16 != R || r.at(d, GRU_XG, s) != nullptr || !r.readable(d.p[GRU_BIH], 3 * R);
        for (auto [r0, c] : tiles) {
          read_slab(r.at(d, GRU_X16, s), r0, d.K, d.K / 16);
          for (int rr = 0; rr < rows_of(r0); ++rr)
            for (int cc = 0; cc < 16; ++cc) {
              const int row = r0 + rr, col = c * 16 + cc;
              for (int g = 0; g < 3; ++g) r.read(r.at(d, GRU_GH, s) + (size_t)row * 3 * R + g * R + col, true);
              const int wr = r.read(r.at(d, GRU_HPREV, s) + (size_t)row * d.ld[GRU_LD_HPREV] + col, true);
              bad += !(wr == PRE || wr == id - p.ndesc);  // the prefill, or this descriptor one step earlier
            }
        }
        for (auto [r0, c] : tiles)
          for (int rr = 0; rr < rows_of(r0); ++rr)
            for (int cc = 0; cc < 16; ++cc) {
              const int row = r0 + rr, col = c * 16 + cc;
              put_words(r, r.at(d, GRU_HRM, s), d.ld[LD_OUT], r.at(d, GRU_H16, s), d.n16[N16_OUT], r.at(d, GRU_H16B, s), d.n16[N16_OUTB], row, col, id);
              for (int k : {GRU_RG, GRU_UG, GRU_NG}) {
                const float* q = r.at(d, k, s) + (size_t)row * R + col;
                bad += !r.in_dummy(q);
                r.write(q, id);
              }
            }
      } else if (d.kind == K_HEAD) {  // tile_head: P16 / Q16 [rows, K] polled, eps of the step; z three ways, the statistics to a dummy
        const int Z = d.i[HEAD_I_Z];
        bad += d.ct * 16 != Z || d.i[HEAD_I_RESIDUAL] != 3 || !r.readable(d.p[HEAD_BP], 2 * Z) || !r.readable(d.p[HEAD_BQ], 2 * Z) || r.at(d, HEAD_MUQ_RAW, s) != nullptr;
        for (auto [r0, c] : tiles) {
          read_slab(r.at(d, HEAD_P16, s), r0, d.K, d.K / 16);
          read_slab(r.at(d, HEAD_Q16, s), r0, d.K, d.K / 16);
          for (int rr = 0; rr < rows_of(r0); ++rr) bad += !r.readable(r.at(d, HEAD_EPS, s) + (size_t)(r0 + rr) * Z + c * 16, 16, false);
        }
        for (auto [r0, c] : tiles)
          for (int rr = 0; rr < rows_of(r0); ++rr)
            for (int cc = 0; cc < 16; ++cc) {
              const int row = r0 + rr, col = c * 16 + cc;
              put_words(r, r.at(d, HEAD_Z, s), d.ld[LD_OUT], r.at(d, HEAD_Z16, s), d.n16[N16_OUT], r.at(d, HEAD_Z16B, s), d.n16[N16_OUTB], row, col, id);
              for (int k : {HEAD_MU_P, HEAD_SD_P, HEAD_MU_Q, HEAD_SD_Q, HEAD_RAW_P, HEAD_RAW_Q}) {
                const float* q = r.at(d, k, s) + (size_t)row * Z + col;
                bad += !r.in_dummy(q);
                r.write(q, id);
              }
            }
      } else if (d.kind == K_DMOLS) {  // a tile: 16 rows x 4 samples
        const int F = d.i[DMOLS_I_F], ldd = d.ld[DMOLS_LD_DEC];
        bad += F != kDmolF || d.i[DMOLS_I_NMIX] != kDmolK || d.i[DMOLS_I_S] != S || ldd != Np || d.n16[N16_OUT] != Sp / 16 || d.ld[LD_OUT] != T * S;
        bad += !r.readable(d.p[DMOLS_W], F * F) || !r.readable(d.p[DMOLS_B], F);
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
              if (live) bad += !r.readable(r.at(d, DMOLS_U, s) + ((size_t)row * S + smp) * kDmolK, kDmolK, false) || !r.readable(r.at(d, DMOLS_V, s) + (size_t)row * S + smp, 1, false);
              bad += smp >= Sp;
              put_words(r, live ? r.at(d, DMOLS_X, s) : nullptr, d.ld[LD_OUT], r.at(d, DMOLS_X16, s), d.n16[N16_OUT], nullptr, 0, row, smp, id);
            }
      } else {
        ++bad;  // a kind the roll-out kernels do not have
      }
    }
  for (int v : r.wxo) bad += v <= 0;  // x_out is written completely
}
// `n` floats of the scratch at `off` that the entry point copies out after the launch are written by the launch
inline int unwritten(const Replay& r, size_t off, size_t n) {
  int bad = 0;
  for (size_t e = 0; e < n; ++e) bad += r.wsc[off + e] <= 0;
  return bad;
}
}  // namespace
