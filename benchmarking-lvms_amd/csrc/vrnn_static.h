// vrnn_static.h — the host arithmetic the static walk (vrnn_static.hip) shares with its host test (tests/host/static_plan_test.hip):
// the deal of the VRNN step programs, which of their links keep their weights in registers, and the placement of a static launch
// (tests/host/static_place_test.hip).
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
// forward, decoder range (ctD > 0: the decoder MLP's last layer has ctD column tiles): the workgroups the deal leaves free behind
// the gentle range run the decoder of step t as a follower of the chain, four gentle links from workgroup g + def_n:
//   dec[0]  Y1P = h_t Wd1[:, H:]^T + b1          (K = R; h_t enters step t, so this link runs ahead of the step's phi)
//   dec[1]  Y1  = act(phi_t Wd1[:, :H]^T + Y1P)  (K = H, polled addend: the two column ranges of the first layer's K = H + R product)
//   dec[2]  Y2  = act(Y1 Wd2^T + b2)             (K = H)
//   dec[3]  dec = act(Y2 Wd3^T + b3)             (K = H, ctD column tiles)
// dec[0 .. 2] keep their weights in registers and need one tile per workgroup; dec[3] reads its weights per tile, at most kMaxTiles
// tiles per workgroup (checked in both TileIter modes: a launch's placement picks one).  The range is empty (nwg = 0 in all four)
// when fewer than 8 workgroups are free, with the shared deal, or when a link does not fit.
constexpr int kMaxTiles = 8;  // most tiles of a link the static walk deals one workgroup (vrnn_static.hip tile_lanes)
struct VrnnFwdDeal {
  int def_n, half, g, spare;
  LinkRange hproj, prior, post, head, phi, gru, dec[4];
};
inline VrnnFwdDeal vrnn_fwd_deal(int ctH, int ctZ, int ctR, int tl, int cus, bool shared, int ctD = 0) {
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
  d.spare = shared ? 0 : cus - d.g - d.def_n;
  for (LinkRange& r : d.dec) r = LinkRange{0, 0, 0};
  if (ctD > 0 && d.spare >= 8) {
    const int w0 = d.g + d.def_n, n12 = range_for(ctH * tl, d.spare), n3 = range_for(ctD * tl, d.spare);
    bool fits = true;
    for (bool xcd : {false, true})
      fits = fits && tiles_per_workgroup(tl, ctH, n12, xcd) <= 1 && tiles_per_workgroup(tl, ctD, n3, xcd) <= kMaxTiles;
    if (fits) {
      d.dec[0] = d.dec[1] = d.dec[2] = LinkRange{ctH, w0, n12};
      d.dec[3] = LinkRange{ctD, w0, n3};
    }
  }
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
// the forward program with the decoder range: descriptors 6 .. 9 are dec[0 .. 3] of the deal; the first three are resident too
constexpr int kFwdDesc = 6, kFwdDecDesc = 10;
constexpr std::initializer_list<int> kFwdDecResident = {6, 7, 8};
// the converter's condition: every resident link deals a workgroup at most one tile (else the interpreter runs the program)
// (xcd: the TileIter mode the kernel will deal with — the program's own, or plain under a placement of the launch, below)
inline bool one_tile_each(const Program& p, std::initializer_list<int> links, bool xcd) {
  for (int i : links)
    if (tiles_per_workgroup((p.B + 15) / 16, p.d[i].ct, p.d[i].nwg, xcd) > 1) return false;
  return true;
}
inline bool one_tile_each(const Program& p, std::initializer_list<int> links) { return one_tile_each(p, links, p.xcd != 0); }

// ---- placement: a property of the static launch, not of the program (the interpreter runs the program as built) -----------------
// Workgroups are dealt round-robin over the 8 XCDs (observed, as in TileIter: a wrong guess only costs speed), so workgroup p sits
// on XCD p % 8.  The program's XCD-aware TileIter mode puts column tile c on XCD c % 8 so that an L2 holds 1/8 of every weight
// matrix; the resident links read no weights in the step loop, and what that mode costs them is that the 16 producers of every
// [16, K] slab sit on all eight XCDs.  Plain TileIter on ranges that start at multiples of 8 gives workgroup w row tile w % rt:
// with rt = 4 a row tile lives on XCDs r and r + 4.  kPlaceLocal adds a bijection of the block index on top (place_wg) that
// gathers the prior half of row tile r on XCD r and the posterior half on XCD r + 4.  Which workgroup computes a tile changes no
// operand and no summation order: results do not depend on the placement.
enum Place {
  kPlaceProgram = 0,  // the program's TileIter mode, identity block index
  kPlacePlain = 1,    // plain TileIter, identity block index
  kPlaceLocal = 2,    // plain TileIter, workgroup = place_wg(block index)
};
constexpr int kPlaceSpan = 128;  // place_wg permutes the block indices below it
// block index -> workgroup of the deal.  Block p < 128 on XCD x = p % 8: x < 4 -> workgroup 4 (p / 8) + x of [0, 64), row tile x;
// x >= 4 -> workgroup 64 + 4 (p / 8) + x - 4 of [64, 128), row tile x - 4.
__host__ __device__ __forceinline__ int place_wg(int p) { return p < kPlaceSpan ? 64 * ((p & 7) >> 2) + 4 * (p >> 3) + (p & 3) : p; }
// place_wg is a bijection of [0, grid) for any grid >= 128: it permutes the blocks of the two halves among themselves and leaves
// the gentle and spare ranges behind them alone, so every workgroup of the deal still runs on exactly one block.  kPlaceLocal
// applies to a program when the halves are what the permutation was made for and every range it touches deals row tile (w % 4):
// rt = 4, the links `prior` and `post` on [0, 64) and [64, 128), and every other link on one of those, on their union, or past them.
inline bool place_local_applies(const Program& p, int prior, int post, int grid) {
  if ((p.B + 15) / 16 != 4 || grid < kPlaceSpan) return false;
  if (p.d[prior].wg0 != 0 || p.d[prior].nwg != 64 || p.d[post].wg0 != 64 || p.d[post].nwg != 64) return false;
  for (int i = 0; i < p.ndesc; ++i) {
    const int lo = p.d[i].wg0, hi = lo + p.d[i].nwg;
    const bool kept = (lo == 0 && (hi == 64 || hi == kPlaceSpan)) || (lo == 64 && hi == kPlaceSpan) || lo >= kPlaceSpan;
    if (!kept) return false;
  }
  return true;
}
// the placement a launch runs with: kPlaceLocal falls back to `fallback` (kPlacePlain or kPlaceProgram) where it does not apply
inline int place_for(int want, int fallback, const Program& p, int prior, int post, int grid) {
  if (want == kPlaceLocal) return place_local_applies(p, prior, post, grid) ? kPlaceLocal : (fallback == kPlacePlain ? kPlacePlain : kPlaceProgram);
  return want == kPlacePlain ? kPlacePlain : kPlaceProgram;
}
inline bool place_xcd(int place, const Program& p) { return place == kPlaceProgram && p.xcd != 0; }  // the TileIter mode of a launch
inline int grid_of(const Program& p) {
  int g = 0;
  for (int i = 0; i < p.ndesc; ++i) g = std::max(g, p.d[i].wg0 + p.d[i].nwg);
  return g;
}

}  // namespace pchain
}  // namespace blvm
