// The decoder range of the VRNN forward deal (csrc/vrnn_static.h vrnn_fwd_deal with ctD > 0): on 256 / 128 / 64 workgroups and
// 1 .. 4 row tiles, with 15 and 120 decoder column tiles.  Where the range exists it starts behind the gentle range, is disjoint
// from every other range and inside the chip, the three resident links get one tile per workgroup and the last layer at most
// kMaxTiles, in both TileIter modes, with every tile owned exactly once; where fewer than 8 workgroups are free, or with the shared
// deal, the range is empty and the program is the six descriptors it was.  The other ranges never depend on ctD.
#include "vrnn_static.h"
#include <cstdio>
#include <vector>
namespace blvm { void set_error(const char*, ...) {} }
using namespace blvm::pchain;

static bool same(const LinkRange& a, const LinkRange& b) { return a.ct == b.ct && a.wg0 == b.wg0 && a.nwg == b.nwg; }

// every tile of the link owned exactly once by a workgroup of [0, cus); returns the most tiles one workgroup owns (-1: an error)
static int most_tiles(const LinkRange& l, int rt, int cus, bool xcd) {
  std::vector<int> cnt(rt * l.ct, 0);
  int most = 0;
  for (int w = 0; w < cus; ++w) {
    int mine = 0;
    for (TileIter it(w, l.wg0, l.nwg, rt, l.ct, xcd); it.valid(); it.next()) {
      const int r = it.r0() / 16, c = it.c();
      if (r < 0 || r >= rt || c < 0 || c >= l.ct) return -1;
      cnt[c * rt + r]++; ++mine;
    }
    most = mine > most ? mine : most;
  }
  for (int v : cnt)
    if (v != 1) return -1;
  return most;
}

int main() {
  int bad = 0, folded = 0, empty = 0;
  for (int cus : {256, 128, 64})
    for (int tl = 1; tl <= 4; ++tl)
      for (int ctD : {15, 120}) {
        const VrnnFwdDeal d0 = vrnn_fwd_deal(16, 16, 32, tl, cus, false), d = vrnn_fwd_deal(16, 16, 32, tl, cus, false, ctD);
        bad += !same(d0.hproj, d.hproj) || !same(d0.prior, d.prior) || !same(d0.post, d.post) || !same(d0.head, d.head) || !same(d0.phi, d.phi) ||
               !same(d0.gru, d.gru) || d0.g != d.g || d0.def_n != d.def_n;
        for (const LinkRange& r : d0.dec) bad += r.nwg != 0;  // no decoder asked for: no range
        const int spare = cus - d.g - d.def_n;
        bad += d.spare != spare;
        if (d.dec[0].nwg == 0) {  // the program stays six descriptors: all four ranges empty
          ++empty;
          for (const LinkRange& r : d.dec) bad += r.nwg != 0;
          // ... and only for a reason: too few free workgroups, or a link that does not fit them
          const bool fits = spare >= 8 && 16 * tl <= range_for(16 * tl, spare) && ctD * tl <= kMaxTiles * range_for(ctD * tl, spare);
          bad += fits;
          continue;
        }
        ++folded;
        bad += spare < 8;
        const int w0 = d.g + d.def_n;  // behind the halves and the gentle range
        bad += d.hproj.wg0 + d.hproj.nwg != w0;
        for (int k = 0; k < 4; ++k) {
          const LinkRange& r = d.dec[k];
          bad += r.wg0 != w0 || r.nwg < 8 || r.nwg % 8 != 0 || r.wg0 + r.nwg > cus || r.ct != (k < 3 ? 16 : ctD);
          for (bool xcd : {false, true}) {
            const int most = most_tiles(r, tl, cus, xcd);
            bad += most < 1 || most > (k < 3 ? 1 : kMaxTiles) || most > tiles_per_workgroup(tl, r.ct, r.nwg, xcd);
          }
        }
        // the program as vrnn.hip builds it: ten descriptors, the resident ones on one tile each
        Program p{};
        p.B = 16 * tl;
        for (const LinkRange& l : {d.hproj, d.prior, d.post, d.head, d.phi, d.gru, d.dec[0], d.dec[1], d.dec[2], d.dec[3]}) {
          Desc& q = p.d[p.ndesc++];
          q.ct = l.ct; q.wg0 = l.wg0; q.nwg = l.nwg;
        }
        bad += p.ndesc != kFwdDecDesc || grid_of(p) > cus;
        for (bool xcd : {false, true}) bad += !one_tile_each(p, kFwdDecResident, xcd);
      }
  // the flagship deal: B = 64 on 256 workgroups, 120 column tiles -> [192, 256), 7.5 tiles of the last layer per workgroup
  const VrnnFwdDeal f = vrnn_fwd_deal(16, 16, 32, 4, 256, false, 120);
  bad += f.dec[0].wg0 != 192 || f.dec[0].nwg != 64 || f.dec[3].wg0 != 192 || f.dec[3].nwg != 64 || tiles_per_workgroup(4, 120, 64, false) != 8;
  // a full chip (B = 64 on 128 workgroups) and the shared deal leave no range
  bad += vrnn_fwd_deal(16, 16, 32, 4, 128, false, 120).dec[0].nwg != 0;
  bad += vrnn_fwd_deal(16, 16, 32, 4, 256, true, 120).dec[3].nwg != 0;
  bad += folded == 0 || empty == 0;  // both outcomes were seen
  printf("decoder deal: %d errors (%d deals with the range, %d without)\n", bad, folded, empty);
  return bad != 0;
}
