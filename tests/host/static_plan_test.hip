// The deal of the VRNN step programs (csrc/vrnn_static.h, what vrnn.hip builds its descriptors from) against the static walk's
// condition for register-resident weights: on 256 CUs every batch 1 .. 64 gives every resident link at most one tile per workgroup,
// every tile of every link has exactly one owner, and a chip too small for that makes the condition fail (the interpreter runs).
#include "vrnn_static.h"
#include <cstdio>
#include <vector>
namespace blvm { void set_error(const char*, ...) {} }
using namespace blvm::pchain;

// the programs' descriptors in vrnn.hip's order, ranges only (the condition reads nothing else)
static Program program(int B, bool xcd, std::initializer_list<LinkRange> links) {
  Program p{};
  p.B = B; p.xcd = xcd;
  for (const LinkRange& l : links) {
    Desc& d = p.d[p.ndesc++];
    d.ct = l.ct; d.wg0 = l.wg0; d.nwg = l.nwg;
  }
  return p;
}
static Program fwd_program(int B, int cus, bool xcd) {
  const int rt = (B + 15) / 16;
  const VrnnFwdDeal d = vrnn_fwd_deal(16, 16, 32, rt, cus, false);
  return program(B, xcd, {d.hproj, d.prior, d.post, d.head, d.phi, d.gru});
}
static Program bwd_program(int B, int cus, bool xcd, bool* split3) {
  const int rt = (B + 15) / 16;
  const VrnnBwdDeal d = vrnn_bwd_deal(16, 16, 32, rt, cus, false, true);
  *split3 = d.split3;
  return program(B, xcd, {d.grub, d.part[0], d.part[1], d.part[2], d.gb, d.wide_h, d.wide_h, d.dz, d.prior, d.post});
}
// every tile of every link owned exactly once and inside the grid; the most tiles of a link on one workgroup is what
// tiles_per_workgroup says; returns the errors
static int owners(const Program& p, int grid) {
  int bad = 0;
  const int rt = (p.B + 15) / 16;
  for (int i = 0; i < p.ndesc; ++i) {
    const Desc& d = p.d[i];
    std::vector<int> cnt(rt * d.ct, 0);
    int most = 0;
    bad += d.wg0 < 0 || d.nwg <= 0 || d.wg0 + d.nwg > grid;
    for (int w = 0; w < grid; ++w) {
      int mine = 0;
      for (TileIter it(w, d.wg0, d.nwg, rt, d.ct, p.xcd != 0); it.valid(); it.next()) {
        const int r = it.r0() / 16, c = it.c();
        if (r < 0 || r >= rt || c < 0 || c >= d.ct) { ++bad; continue; }
        cnt[c * rt + r]++; ++mine;
      }
      most = mine > most ? mine : most;
    }
    for (int v : cnt) bad += v != 1;
    bad += most > tiles_per_workgroup(rt, d.ct, d.nwg, p.xcd != 0);  // (an upper bound; exact without XCD placement)
    if (!p.xcd) bad += most != tiles_per_workgroup(rt, d.ct, d.nwg, false);
  }
  return bad;
}
int main() {
  int bad = 0;
  for (int B = 1; B <= 64; ++B) {
    bool split3 = false;
    const Program f = fwd_program(B, 256, false), b = bwd_program(B, 256, false, &split3);
    bad += !one_tile_each(f, kFwdResident) || !one_tile_each(b, kBwdResident) || !split3;
    bad += owners(f, 256) + owners(b, 256);
    const Program fx = fwd_program(B, 256, true), bx = bwd_program(B, 256, true, &split3);  // XCD-aware placement of the same ranges
    bad += owners(fx, 256) + owners(bx, 256);
    bad += !one_tile_each(fx, kFwdResident) || !one_tile_each(bx, kBwdResident);  // (XCD placement must not send the programs to the interpreter)
  }
  // chips that cannot give every tile a workgroup of its own.  Forward, B = 64 on 64 CUs: the GRU's 128 tiles on 48 workgroups.
  // Backward, B = 64 on 192 CUs: the spare range of the third partial sum is 16 workgroups for 64 tiles (on 64 CUs there is no spare
  // range at all: the program is not the three-way split the static walk was built for)
  bool split3 = false;
  bad += one_tile_each(fwd_program(64, 64, false), kFwdResident);
  bad += owners(fwd_program(64, 64, false), 64);
  const Program b192 = bwd_program(64, 192, false, &split3);
  bad += !split3 || one_tile_each(b192, kBwdResident);
  bad += owners(b192, 192);
  vrnn_bwd_deal(16, 16, 32, 4, 64, false, true).split3 ? ++bad : 0;
  printf("static plan: %d errors\n", bad);
  return bad != 0;
}
