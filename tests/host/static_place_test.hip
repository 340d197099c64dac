// The placement of the static walk's launches (csrc/vrnn_static.h Place) against the deal of the VRNN step programs, B = 1 .. 64 on 256
// CUs and on 64 CUs: place_wg is a bijection of [0, grid) that keeps every link's range; in the TileIter mode a placement deals with,
// every tile has one owner and a resident link deals a workgroup at most one tile wherever the converter's condition says so; and
// where the local placement applies (four row tiles, halves of 64) every tile of the prior (posterior) run of row tile r, forward and
// backward, is computed by a block with index % 8 == r (r + 4).  Where it does not apply the launch falls back to the placement it names
// for that: the plain one or the program's.
#include "vrnn_static.h"
#include <cstdio>
#include <vector>
namespace blvm { void set_error(const char*, ...) {} }
using namespace blvm::pchain;

static Program program(int B, std::initializer_list<LinkRange> links) {
  Program p{};
  p.B = B; p.xcd = 1;  // (the program as built by default: the placement of the launch must not read it past kPlaceProgram)
  for (const LinkRange& l : links) {
    Desc& d = p.d[p.ndesc++];
    d.ct = l.ct; d.wg0 = l.wg0; d.nwg = l.nwg;
  }
  return p;
}
static Program fwd_program(int B, int cus) {
  const VrnnFwdDeal d = vrnn_fwd_deal(16, 16, 32, (B + 15) / 16, cus, false);
  return program(B, {d.hproj, d.prior, d.post, d.head, d.phi, d.gru});
}
static Program bwd_program(int B, int cus) {
  const VrnnBwdDeal d = vrnn_bwd_deal(16, 16, 32, (B + 15) / 16, cus, false, true);
  return program(B, {d.grub, d.part[0], d.part[1], d.part[2], d.gb, d.wide_h, d.wide_h, d.dz, d.prior, d.post});
}

// one program under the placement the host would launch it with when asked for `want`; returns the errors
static int check(const Program& p, std::initializer_list<int> resident, int prior, int post, std::initializer_list<int> prior_half,
                 std::initializer_list<int> post_half, int want, int fallback, bool expect_local) {
  int bad = 0;
  const int rt = (p.B + 15) / 16, grid = grid_of(p);
  const int place = place_for(want, fallback, p, prior, post, grid);
  const bool xcd = place_xcd(place, p);
  bad += want == kPlaceLocal && place != (expect_local ? kPlaceLocal : fallback);
  bad += want != kPlaceLocal && place != want;
  bad += xcd != (place == kPlaceProgram);
  // block -> workgroup: a bijection of [0, grid)
  std::vector<int> wg(grid), hits(grid, 0);
  for (int b = 0; b < grid; ++b) {
    wg[b] = place == kPlaceLocal ? place_wg(b) : b;
    if (wg[b] < 0 || wg[b] >= grid) { ++bad; wg[b] = b; continue; }
    hits[wg[b]]++;
  }
  for (int v : hits) bad += v != 1;
  const bool one_each = one_tile_each(p, resident, xcd);
  for (int i = 0; i < p.ndesc; ++i) {
    const Desc& d = p.d[i];
    if (d.nwg == 0) continue;  // (the third partial sum of a backward deal without a spare range: not a link of that program)
    // it keeps every range: the blocks that run a gentle or spare range are that range itself, and the blocks that run a range of
    // the two halves are blocks of the two halves (the same CUs as before, dealt differently), as many as the range has workgroups
    int runs = 0;
    for (int b = 0; b < grid; ++b) {
      if (wg[b] < d.wg0 || wg[b] >= d.wg0 + d.nwg) continue;
      ++runs;
      if (place == kPlaceLocal) bad += d.wg0 >= kPlaceSpan ? wg[b] != b : b >= kPlaceSpan;
      else bad += wg[b] != b;
    }
    bad += runs != d.nwg;
    std::vector<int> cnt(rt * d.ct, 0);
    int most = 0;
    for (int b = 0; b < grid; ++b) {
      int mine = 0;
      for (TileIter it(wg[b], d.wg0, d.nwg, rt, d.ct, xcd); it.valid(); it.next()) {
        const int r = it.r0() / 16, c = it.c();
        if (r < 0 || r >= rt || c < 0 || c >= d.ct) { ++bad; continue; }
        cnt[c * rt + r]++; ++mine;
        if (place == kPlaceLocal) {  // the halves' own links: row tile r on XCD r (prior) or r + 4 (posterior)
          for (int k : prior_half) bad += k == i && b % 8 != r;
          for (int k : post_half) bad += k == i && b % 8 != r + 4;
          bad += b % 4 != r;  // and every permuted link keeps a row tile on XCDs r and r + 4
        }
      }
      most = mine > most ? mine : most;
    }
    for (int v : cnt) bad += v != 1;
    bad += most > tiles_per_workgroup(rt, d.ct, d.nwg, xcd);
    for (int k : resident) bad += k == i && one_each && most > 1;
  }
  return bad;
}

int main() {
  int bad = 0, local = 0;
  for (int cus : {256, 64})
    for (int B = 1; B <= 64; ++B) {
      const Program f = fwd_program(B, cus), b = bwd_program(B, cus);
      const bool expect_local = cus == 256 && B > 48;  // four row tiles on halves of 64
      local += expect_local;
      for (int fallback : {kPlacePlain, kPlaceProgram})  // (of the local placement where it does not apply)
        for (int want : {kPlaceProgram, kPlacePlain, kPlaceLocal}) {
          bad += check(f, kFwdResident, 1, 2, {1}, {2}, want, fallback, expect_local);
          bad += check(b, kBwdResident, 8, 9, {1, 8}, {2, 9}, want, fallback, expect_local);
          // 256 CUs: no placement may send the programs to the interpreter
          if (cus == 256) {
            const bool xf = place_xcd(place_for(want, fallback, f, 1, 2, grid_of(f)), f), xb = place_xcd(place_for(want, fallback, b, 8, 9, grid_of(b)), b);
            bad += !one_tile_each(f, kFwdResident, xf) || !one_tile_each(b, kBwdResident, xb);
          }
        }
    }
  bad += local != 16;
  // the permutation itself: block p of XCD x = p % 8 -> a workgroup of [0, 64) with row tile x, or of [64, 128) with row tile x - 4
  for (int p = 0; p < 512; ++p) {
    const int w = place_wg(p), x = p % 8;
    if (p >= kPlaceSpan) bad += w != p;
    else bad += x < 4 ? !(w >= 0 && w < 64 && w % 4 == x) : !(w >= 64 && w < 128 && w % 4 == x - 4);
  }
  printf("static place: %d errors\n", bad);
  return bad != 0;
}
