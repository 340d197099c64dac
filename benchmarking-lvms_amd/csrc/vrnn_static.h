// vrnn_static.h — the host arithmetic the static walk (vrnn_static.hip) shares with its host test (tests/host/static_plan_test.hip):
// the deal of the VRNN step programs, which of their links keep their weights in registers, and the placement of a static launch
// (tests/host/static_place_test.hip), and the plan by which a static walk stores its own sentinels (tests/host/arm_plan_test.hip).
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
// backward, decoder leader (ctD > 0 = the column tiles of the decoder's input, (H + R) / 16; split3 only): the spare range, which
// owns one partial-sum tile per workgroup and then waits for the rest of the step, runs the decoder MLP's data gradients of the
// time step kBdecAhead walk steps ahead of the chain, three gentle links on the range of part[2]:
//   bdec[0]  dY2 = gate_Y2(dZ3 Wd3)   (K = S F: dZ3 is complete before the launch, row-major, not polled)
//   bdec[1]  dY1 = gate_Y1(dY2 Wd2)   (K = H, resident weights: one tile per workgroup)
//   bdec[2]  dD  = dY1 Wd1            (K = H, ctD column tiles: the phi part | the h part)
// dD's phi part is the polled addend of part[2], its h part the second polled addend of GB.  On the range of part[2] (16 tl
// workgroups) TileIter gives the workgroup of part[2]'s tile (r, c) the tile (r, c) of bdec[2] too, in both modes: the addend a
// partial-sum tile polls is the one its own workgroup stored.  Empty (nwg = 0 in all three) where a link does not fit.
constexpr int kBdecAhead = 2;  // walk steps the leader runs ahead (at most kArmAhead - 2: see arm_applies)
// backward, d_enc follower (ctX > 0 = the column tiles of the encoding, X / 16; split3 only): the posterior half, which owns no tile
// of the summing link, the phi_z run or dz and waits between its partial-sum tile and its run, computes the gradient wrt the
// encoding of the time step one walk step BEHIND the chain (DQ0[t] is published at the end of its own walk step), two gentle links
// on the range of `post`:
//   benc[0]  EP    = DGI W_ih[:, :X]          (K = 3R, weights read per tile; row-major, write-through, polled by benc[1])
//   benc[1]  d_enc = DQ0 Wq0[:, R:] + EP      (K = H, resident weights; plain stores into the caller's buffer)
// Both deal ctX tl tiles over the same range, so TileIter gives a workgroup the same tile (r, c) of both, in both modes: the addend
// a tile polls is the one its own workgroup stored, and every word of EP and d_enc is written once (no atomics: the sum has one
// order).  Empty (nwg = 0 in both) unless every workgroup of the half gets exactly one tile and none of the wide links reaches it.
constexpr int kBencLag = 1;  // walk steps the follower runs behind: active on s in [kBencLag, T' + 1), the walk's existing last step
struct VrnnBwdDeal {
  int def_n, half, g, spare;
  bool split3;
  LinkRange grub, part[3], dphi, gb, wide_h, dz, prior, post, bdec[3], benc[2];
};
inline VrnnBwdDeal vrnn_bwd_deal(int ctH, int ctZ, int ctR, int tl, int cus, bool shared, bool allow_split3, int ctD = 0, int ctX = 0) {
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
  for (LinkRange& r : d.bdec) r = LinkRange{0, 0, 0};
  if (ctD > 0 && d.split3) {
    const int w0 = d.part[2].wg0, n = d.part[2].nwg;
    bool fits = n == ctH * tl;  // (one partial-sum tile on every workgroup of the range: the leader's tiles line up with them)
    for (bool xcd : {false, true})
      fits = fits && tiles_per_workgroup(tl, ctH, n, xcd) <= 1 && tiles_per_workgroup(tl, ctD, n, xcd) <= kMaxTiles;
    if (fits) {
      d.bdec[0] = d.bdec[1] = LinkRange{ctH, w0, n};
      d.bdec[2] = LinkRange{ctD, w0, n};
    }
  }
  for (LinkRange& r : d.benc) r = LinkRange{0, 0, 0};
  if (ctX > 0 && d.split3) {
    bool fits = ctX * tl == d.post.nwg && d.wide_h.wg0 + d.wide_h.nwg <= d.post.wg0 && d.dz.wg0 + d.dz.nwg <= d.post.wg0;
    for (bool xcd : {false, true}) fits = fits && tiles_per_workgroup(tl, ctX, d.post.nwg, xcd) <= 1;
    if (fits) d.benc[0] = d.benc[1] = LinkRange{ctX, d.post.wg0, d.post.nwg};
  }
  return d;
}

// descriptors of the forward / backward program (vrnn.hip) whose tiles run on resident weights: every link of the critical path.
// The gentle links (forward 0: hidden projection; backward 4: GB) deal several tiles per workgroup and read theirs per tile.
constexpr std::initializer_list<int> kFwdResident = {1, 2, 3, 4, 5};
constexpr std::initializer_list<int> kBwdResident = {0, 1, 2, 3, 5, 6, 7, 8, 9};
// the forward program with the decoder range: descriptors 6 .. 9 are dec[0 .. 3] of the deal; the first three are resident too
constexpr int kFwdDesc = 6, kFwdDecDesc = 10;
constexpr std::initializer_list<int> kFwdDecResident = {6, 7, 8};
// the backward program with the decoder leader: descriptors 10 .. 12 are bdec[0 .. 2] of the deal; bdec[1] is resident
constexpr int kBwdDesc = 10, kBwdDecDesc = 13;
constexpr std::initializer_list<int> kBwdDecResident = {11};
// the backward program with the d_enc follower: benc[0 .. 1] of the deal are the program's LAST two descriptors (10, 11 | behind the
// decoder leader 13, 14), both on one tile per workgroup; benc[1] is resident
constexpr int kBwdEncLinks = 2, kBwdEncDesc = kBwdDesc + kBwdEncLinks, kBwdDecEncDesc = kBwdDecDesc + kBwdEncLinks;
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

// ---- look-ahead arming: the walk's idle workgroups store the sentinels of walk step s + kArmAhead ----------------------
// The host fills the polled buffers of a persistent launch with sentinels.  Under a static walk only walk steps [0, kArmAhead) are
// filled in front of the launch; the slabs of step s + kArmAhead are armed at step s by workgroups that wait anyway (forward: the
// posterior half between its run and its GRU tile; backward: the spare range between its partial-sum tiles).  Three rules:
//   1. a workgroup arms only words of the row tile its own tile of the role's link belongs to: row tiles are independent chains,
//      and inside one every producer of step s + kArmAhead is causally behind this workgroup's next published tile;
//   2. the stores are write-through (sc1) 16-byte stores and the wave drains them (vmcnt(0)) before its next tile publishes;
//   3. only a program that arm_applies() has verified is armed; any other launch gets the full host fill.
constexpr int kArmAhead = 4;
constexpr int kArmMax = 24;        // entries of a table
constexpr int kArmCandidates = 64;  // workgroups of an arming role (one wave ranks them with a ballot)
// one polled buffer: walk step j's slab starts at base + j * step (floats; step < 0: the backward walks time in reverse), row tile r
// of it at + r * tile and holds n4 16-byte words (the last row tile of a row-major buffer: n4_last); the buffer has nslabs slabs
struct ArmEntry {
  float* base;
  int step, tile, n4, n4_last, nslabs;
};
struct ArmTable {
  ArmEntry e[kArmMax];
  int n;  // 0: the launch arms nothing
};
// a T16 slab [rt * 16, width] (1 KB blocks, a row tile is 16 * width contiguous floats) | a row-major slab [B, ld]
// reversed: walk step j is time step nslabs - 1 - j
inline ArmEntry arm_t16(float* buf, int width, int rt, int nslabs, bool reversed = false) {
  const int step = rt * 16 * width;
  return ArmEntry{reversed ? buf + (long)(nslabs - 1) * step : buf, reversed ? -step : step, 16 * width, 4 * width, 4 * width, nslabs};
}
inline ArmEntry arm_rm(float* buf, int ld, int B, int nslabs, bool reversed = false) {
  const int step = B * ld, rt = (B + 15) / 16;
  return ArmEntry{reversed ? buf + (long)(nslabs - 1) * step : buf, reversed ? -step : step, 16 * ld, 4 * ld, (B - 16 * (rt - 1)) * ld / 4, nslabs};
}
// what a launch's host code hands vrnn_launch: the table, and the regions of the full fill (the interpreter; unverified programs)
struct ArmPlan {
  ArmTable tab{};
  struct Region { void* p; size_t bytes; } full[3] = {};
  int nfull = 0;
  void add(const ArmEntry& e) { if (e.base != nullptr && tab.n < kArmMax) tab.e[tab.n++] = e; else if (e.base != nullptr) tab.n = kArmMax + 1; }
  void fill(void* p, size_t bytes) { full[nfull++] = Region{p, bytes}; }
};
// the armer's share of row tile r of an entry: 16-byte words [*first, *first + *count) of the row tile, armer k of n = 1 << log2n
// (a power of two: the step loop of a walk divides by shifting)
__host__ __device__ __forceinline__ void arm_share(const ArmEntry& e, int r, int rt, int k, int log2n, int* first, int* count) {
  const int total = r == rt - 1 ? e.n4_last : e.n4, per = (total + (1 << log2n) - 1) >> log2n;
  *first = k * per < total ? k * per : total;
  *count = per < total - *first ? per : total - *first;
}
// the workgroups that arm: those of [cand0, cand0 + ncand) with a tile of `link`, ranked k of n among the ones of the same row tile
// false: workgroup w does not arm
inline bool arm_rank(const Program& p, int link, int cand0, int ncand, bool xcd, int w, int* r, int* k, int* n) {
  const int rt = (p.B + 15) / 16;
  const Desc& d = p.d[link];
  TileIter mine(w, d.wg0, d.nwg, rt, d.ct, xcd);
  if (w < cand0 || w >= cand0 + ncand || !mine.valid()) return false;
  *r = mine.r0() / 16; *k = 0; *n = 0;
  for (int c = cand0; c < cand0 + ncand; ++c) {
    TileIter it(c, d.wg0, d.nwg, rt, d.ct, xcd);
    if (!it.valid() || it.r0() != mine.r0()) continue;
    ++*n;
    if (c < w) ++*k;
  }
  return true;
}
// the descriptor slot of a link's polled activation operand (-1: a kind the static walks do not run)
inline int arm_operand_slot(int kind) {
  switch (kind) {
    case K_LIN: return LIN_A;
    case K_LINSEQ: return LINSEQ_A0;
    case K_HEAD: return HEAD_P16;
    case K_GRU: return GRU_X16;
    case K_GRUB: return GRUB_D0_16;
    case K_DZ: return DZ_D16;
    default: return -1;
  }
}
// Rule 3, next to one_tile_each: the converter's condition for arming a launch.  `link`: the arming role's link, whose tiles the
// workgroups [cand0, cand0 + ncand) arm around; idle: the links those workgroups must own no tile of (they wait while others walk
// them: the window the stores go into, and the registers — vrnn_static.hip fwd_post_arming); xcd: the launch's TileIter mode.
//   - every link multiplies a stepped operand that lies in a buffer of the table: it polls, so nothing runs ahead of the chain;
//     the one exemption is a K_LIN whose operand is complete before the launch (DF_A_PLAIN: dZ3 of the decoder leader) — every
//     workgroup with a tile of it must own a tile of the arming role's link, whose poll it runs behind in every step;
//   - every arming workgroup owns exactly one tile of the role's link, and every row tile has armers, a power of two of them;
//   - every buffer of the table has the program's row-tile geometry: 16-byte aligned pieces, row tiles inside their slab.
inline bool arm_applies(const Program& p, const ArmTable& t, int link, std::initializer_list<int> idle, int cand0, int ncand, bool xcd) {
  const int rt = (p.B + 15) / 16;
  if (t.n <= 0 || t.n > kArmMax || ncand <= 0 || ncand > kArmCandidates || p.S <= kArmAhead || p.rt_group != 1) return false;
  for (int i = 0; i < t.n; ++i) {
    const ArmEntry& e = t.e[i];
    const long span = e.step < 0 ? -(long)e.step : e.step;
    if (e.base == nullptr || (reinterpret_cast<unsigned long long>(e.base) & 15) != 0 || e.step % 4 != 0 || e.tile % 4 != 0) return false;
    if (e.n4 <= 0 || e.n4_last <= 0 || e.n4_last > e.n4 || 4L * e.n4 > e.tile || (long)(rt - 1) * e.tile + 4L * e.n4_last > span) return false;
    if (e.nslabs < p.S - 1 || e.nslabs > p.S + 1) return false;  // (a slab per step; the state's T16 copy has one more)
  }
  for (int i = 0; i < p.ndesc; ++i) {
    const Desc& d = p.d[i];
    const int slot = arm_operand_slot(d.kind);
    if (slot < 0 || d.p[slot] == nullptr || p.stride[d.sidx[slot]] == 0) return false;
    if (d.kind == K_LIN && (d.flags & DF_A_PLAIN) != 0) {
      const Desc& role = p.d[link];
      for (int w = d.wg0; w < d.wg0 + d.nwg; ++w)
        if (TileIter(w, d.wg0, d.nwg, rt, d.ct, xcd).valid() && !TileIter(w, role.wg0, role.nwg, rt, role.ct, xcd).valid()) return false;
      continue;
    }
    bool inside = false;
    for (int k = 0; k < t.n && !inside; ++k) {
      const ArmEntry& e = t.e[k];
      const long span = e.step < 0 ? -(long)e.step : e.step;
      const float* lo = e.step < 0 ? e.base - (long)(e.nslabs - 1) * span : e.base;
      inside = d.p[slot] >= lo && d.p[slot] <= lo + (long)e.nslabs * span;  // (<=: a reversed operand may start one slab past the end)
    }
    if (!inside) return false;
  }
  const Desc& d = p.d[link];
  int armers[4] = {0, 0, 0, 0};
  if (rt > 4) return false;
  for (int w = cand0; w < cand0 + ncand; ++w) {
    int tiles = 0, r = 0;
    for (TileIter it(w, d.wg0, d.nwg, rt, d.ct, xcd); it.valid(); it.next()) { ++tiles; r = it.r0() / 16; }
    if (tiles > 1) return false;
    if (tiles == 1) ++armers[r];
    for (int i : idle)
      if (TileIter(w, p.d[i].wg0, p.d[i].nwg, rt, p.d[i].ct, xcd).valid()) return false;
  }
  for (int r = 0; r < rt; ++r)
    if (armers[r] == 0 || (armers[r] & (armers[r] - 1)) != 0) return false;
  return true;
}

}  // namespace pchain
}  // namespace blvm
