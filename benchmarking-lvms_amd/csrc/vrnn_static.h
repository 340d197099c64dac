// vrnn_static.h — the host arithmetic the static walk (vrnn_static.hip) shares with its host test (tests/host/static_plan_test.hip):
// the deal of the VRNN step programs, and which of their links keep their weights in registers.
#pragma once
#include <algorithm>
#include <initializer_list>

#include "pchain.h"

namespace blvm {
namespace pchain {

// ---- the deal of the VRNN step programs (vrnn.hip builds its descriptors from it, in this order) -------------------------------
// tl: tiles of a link per column tile (row tiles, or row groups); cus: workgroups available (a multiple of 8); shared: the gentle
// link owns no range (vrnn.hip vrnn_shared_deal).  A link's tiles (ct column tiles x tl) go to the workgroups [wg0, wg0 + nwg).
struct LinkRange {
  int ct, wg0, nwg;
};
// forward: the hidden projection (gentle: up to a quarter of the chip behind the halves, or with `shared` the posterior half), the
// prior | posterior runs on a half each, heads, phi_z links and GRU from workgroup 0
struct VrnnFwdDeal {
  int def_n, half, g;
  LinkRange hproj, prior, post, head, phi, gru;
};
inline VrnnFwdDeal vrnn_fwd_deal(int ctH, int ctZ, int ctR, int tl, int cus, bool shared) {
  VrnnFwdDeal d;
  d.def_n = shared ? 0 : range_for(3 * ctR * tl, std::min(cus / 4, 64));
  d.half = range_for(ctH * tl, (cus - d.def_n) / 2);  // prior | posterior halves of a link
  d.g = 2 * d.half;
  const int wide = shared ? d.half : d.g;
  d.hproj = shared ? LinkRange{3 * ctR, d.half, d.half} : LinkRange{3 * ctR, d.g, d.def_n};
  d.prior = LinkRange{ctH, 0, d.half};
  d.post = LinkRange{ctH, d.half, d.half};
  d.head = LinkRange{ctZ, 0, range_for(ctZ * tl, wide)};
  d.phi = LinkRange{ctH, 0, range_for(ctH * tl, wide)};
  d.gru = LinkRange{ctR, 0, range_for(ctR * tl, d.g)};
  return d;
}
// backward: GRU backward; dphi as one link or (split3: a third range is free) three K = R partial-sum links side by side; GB
// (gentle); the summing link, the phi_z run and dz on the wide range; the prior | posterior runs on a half each
struct VrnnBwdDeal {
  int def_n, half, g, spare;
  bool split3;
  LinkRange grub, part[3], dphi, gb, wide_h, dz, prior, post;
};
inline VrnnBwdDeal vrnn_bwd_deal(int ctH, int ctZ, int ctR, int tl, int cus, bool shared, bool allow_split3) {
  VrnnBwdDeal d;
  d.def_n = shared ? 0 : range_for(ctR * tl, std::min(cus / 4, 64));  // GB link
  d.half = range_for(ctH * tl, (cus - d.def_n) / 2);
  d.g = 2 * d.half;
  const int wide = shared ? d.half : d.g;  // range of the links between the GRU backward and the heads
  d.spare = cus - d.g - d.def_n;
  d.split3 = !shared && d.spare >= 8 && d.half >= 8 && allow_split3;
  d.grub = LinkRange{ctR, 0, range_for(ctR * tl, d.g)};
  d.part[0] = LinkRange{ctH, 0, range_for(ctH * tl, d.half)};
  d.part[1] = LinkRange{ctH, d.half, range_for(ctH * tl, d.half)};
  d.part[2] = LinkRange{ctH, d.g + d.def_n, d.split3 ? range_for(ctH * tl, d.spare) : 0};
  d.dphi = LinkRange{ctH, 0, range_for(ctH * tl, wide)};
  d.gb = shared ? LinkRange{ctR, d.half, d.half} : LinkRange{ctR, d.g, d.def_n};
  d.wide_h = LinkRange{ctH, 0, range_for(ctH * tl, wide)};
  d.dz = LinkRange{ctZ, 0, range_for(ctZ * tl, wide)};
  d.prior = LinkRange{ctH, 0, d.half};
  d.post = LinkRange{ctH, d.half, d.half};
  return d;
}

// descriptors of the forward / backward program (vrnn.hip) whose tiles run on resident weights: every link of the critical path.
// The gentle links (forward 0: hidden projection; backward 4: GB) deal several tiles per workgroup and read theirs per tile.
constexpr std::initializer_list<int> kFwdResident = {1, 2, 3, 4, 5};
constexpr std::initializer_list<int> kBwdResident = {0, 1, 2, 3, 5, 6, 7, 8, 9};
// the converter's condition: every resident link deals a workgroup at most one tile (else the interpreter runs the program)
inline bool one_tile_each(const Program& p, std::initializer_list<int> links) {
  for (int i : links)
    if (tiles_per_workgroup((p.B + 15) / 16, p.d[i].ct, p.d[i].nwg, p.xcd != 0) > 1) return false;
  return true;
}

}  // namespace pchain
}  // namespace blvm
