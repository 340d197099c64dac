// The decoder leader of the VRNN backward deal (csrc/vrnn_static.h vrnn_bwd_deal with ctD > 0, kBdecAhead, arm_applies' exemption),
// replayed on the host for 1 .. 4 row tiles on 256 / 128 / 64 workgroups, in both TileIter modes:
//   - the other ranges never depend on ctD, and without ctD there is no leader range;
//   - where the range exists every leader tile is owned exactly once, bdec[0] and bdec[1] on one tile per workgroup, bdec[2] within
//     kMaxTiles; the workgroup that owns tile (r, c) of the third partial sum owns tile (r, c) of bdec[2]'s phi part;
//   - the spare range still has exactly one partial-sum tile per armer and a power of two of armers per row tile;
//   - every polled word of the thirteen-descriptor program (DY216, DY116 and the decoder's gradient DD among them) is covered by the
//     prefix fill plus the armers' chunks where the launch arms, by the full fill where it does not;
//   - the deal has no leader range under the shared deal, without split3, or without a spare range, and the arming rule refuses a
//     program whose unpolled link runs on workgroups without a partial-sum tile, whose polled operand lies outside the table, or
//     whose table is full.
// The buffers are addresses in a reserved, never touched mapping: nothing is dereferenced.
#include "vrnn_static.h"
#include <sys/mman.h>
#include <cstdio>
#include <vector>
namespace blvm { void set_error(const char*, ...) {} }
using namespace blvm::pchain;

constexpr int H = 256, Z = 256, R = 512, ctH = H / 16, ctZ = Z / 16, ctR = R / 16, ctD = (H + R) / 16;

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

struct Case {
  Program p{};
  ArmPlan plan;
  std::vector<float*> base;     // buffer of table entry i
  std::vector<size_t> floats;
  float* arena;
  size_t off = 0;
  int nstride = 1, spare0 = 0, nspare = 0;
  float* take(size_t n) { float* q = arena + off; off += (n + 3) & ~(size_t)3; return q; }
  void t16(int width, int rt, int T) {
    float* b = take((size_t)T * rt * 16 * width);
    base.push_back(b); floats.push_back((size_t)T * rt * 16 * width);
    plan.add(arm_t16(b, width, rt, T, true));
  }
  void rm(int ld, int B, int T) {
    float* b = take((size_t)T * B * ld);
    base.push_back(b); floats.push_back((size_t)T * B * ld);
    plan.add(arm_rm(b, ld, B, T, true));
  }
  Desc& desc(int kind, const LinkRange& l, const float* operand, long stride, int flags = 0) {
    Desc& d = p.d[p.ndesc++];
    d = Desc{};
    d.kind = kind; d.ct = l.ct; d.wg0 = l.wg0; d.nwg = l.nwg; d.flags = flags;
    const int slot = arm_operand_slot(kind);
    d.p[slot] = operand;
    p.stride[nstride] = stride;
    d.sidx[slot] = (unsigned char)nstride++;
    return d;
  }
};

// the backward program with the leader as vrnn.hip lays it out: 21 table entries, 13 descriptors
static Case leader_case(float* mem, int B, int T, int cus) {
  Case c;
  c.arena = mem;
  const int rt = (B + 15) / 16, L = kBdecAhead;
  const VrnnBwdDeal d = vrnn_bwd_deal(ctH, ctZ, ctR, rt, cus, false, true, ctD);
  c.p.B = B; c.p.S = T + 1; c.p.rt_group = 1;
  c.rm(R, B, T); c.rm(R, B, T);                          // 0, 1: GA, GB
  for (int i = 0; i < 6; ++i) c.t16(H, rt, T);            // 2 .. 7: DP16[3], DQ16[3]
  c.t16(3 * R, rt, T); c.t16(3 * R, rt, T);                // 8, 9: DGI16, DGH16
  for (int i = 0; i < 4; ++i) c.t16(H, rt, T);            // 10 .. 13: DPHI16[4]
  c.t16(2 * Z, rt, T); c.t16(2 * Z, rt, T);                // 14, 15: DPH16, DQH16
  c.t16(H, rt, T); c.t16(H, rt, T);                        // 16, 17: DPHI16b, DPHI16c
  c.t16(H, rt, T); c.t16(H, rt, T); c.rm(H + R, B, T);     // 18 .. 20: DY216, DY116, DD
  c.plan.fill(c.base[0], sizeof(float) * c.off);
  float* dz3 = c.take((size_t)T * B * 1920);  // complete before the launch: not in the table
  const long xH = (long)rt * 16 * H, x3R = (long)rt * 16 * 3 * R, x2Z = (long)rt * 16 * 2 * Z;
  auto last = [&](int i, long step, int ahead = 0) { return c.base[i] + (long)(T - 1 - ahead) * step; };
  c.desc(K_GRUB, d.grub, c.base[2] + (long)T * xH, -xH);
  for (int k = 0; k < 3; ++k) c.desc(K_LIN, d.part[k], last(8, x3R) + (size_t)k * ctR * 256, -x3R, k == 2 ? DF_ADD_POLLED | DF_ADD_EARLY : 0);
  c.desc(K_LIN, d.gb, last(9, x3R), -x3R, DF_ADD_POLLED | DF_ADD2_POLLED | DF_RM_SC1 | DF_GENTLE | DF_CANARY);
  c.desc(K_LIN, d.wide_h, last(13, xH), -xH, DF_A_SUM3);
  c.desc(K_LINSEQ, d.wide_h, last(12, xH), -xH);
  c.desc(K_DZ, d.dz, last(10, xH), -xH);
  c.desc(K_LINSEQ, d.prior, last(14, x2Z), -x2Z);
  c.desc(K_LINSEQ, d.post, last(15, x2Z), -x2Z);
  c.desc(K_LIN, d.bdec[0], dz3 + (long)(T - 1 - L) * B * 1920, -(long)B * 1920, DF_A_PLAIN | DF_GENTLE);
  c.desc(K_LIN, d.bdec[1], last(18, xH, L), -xH, DF_GENTLE | DF_CANARY);
  c.desc(K_LIN, d.bdec[2], last(19, xH, L), -xH, DF_RM_SC1 | DF_GENTLE | DF_CANARY);
  c.spare0 = d.part[2].wg0; c.nspare = d.part[2].nwg;
  return c;
}
static bool applies(const Case& c, bool xcd) { return arm_applies(c.p, c.plan.tab, 3, {}, c.spare0, c.nspare, xcd); }

// every polled word of every table entry written by the host's part or by an armer's chunk, no chunk outside its buffer
static int coverage(const Case& c, bool xcd, bool armed) {
  int bad = 0;
  const int rt = (c.p.B + 15) / 16;
  const ArmTable& t = c.plan.tab;
  std::vector<unsigned char> hit(c.off / 4 + 1, 0);
  auto mark = [&](const float* p, long n4, int e) {
    if (n4 <= 0) return;
    if ((reinterpret_cast<unsigned long long>(p) & 15) != 0 || p < c.base[e] || p + 4 * n4 > c.base[e] + c.floats[e]) { ++bad; return; }
    for (long i = 0; i < n4; ++i) hit[(size_t)(p - c.arena) / 4 + i] = 1;
  };
  if (!armed) {
    for (int i = 0; i < c.plan.nfull; ++i) {
      const float* p = static_cast<const float*>(c.plan.full[i].p);
      for (size_t k = 0; k < c.plan.full[i].bytes / 16; ++k) hit[(size_t)(p - c.arena) / 4 + k] = 1;
    }
  } else {
    for (int e = 0; e < t.n; ++e)
      for (int j = 0; j < std::min(t.e[e].nslabs, kArmAhead); ++j)
        for (int r = 0; r < rt; ++r) mark(t.e[e].base + (long)j * t.e[e].step + (long)r * t.e[e].tile, r == rt - 1 ? t.e[e].n4_last : t.e[e].n4, e);
    for (int w = c.spare0; w < c.spare0 + c.nspare; ++w) {
      int r, k, n;
      if (!arm_rank(c.p, 3, c.spare0, c.nspare, xcd, w, &r, &k, &n)) continue;
      bad += (n & (n - 1)) != 0;
      for (int s = 0; s < c.p.S; ++s)
        for (int e = 0; e < t.n; ++e) {
          const int j = s + kArmAhead;
          if (j >= t.e[e].nslabs) continue;
          int first, count;
          arm_share(t.e[e], r, rt, k, __builtin_ctz(n), &first, &count);
          mark(t.e[e].base + (long)j * t.e[e].step + (long)r * t.e[e].tile + 4L * first, count, e);
        }
    }
  }
  for (int e = 0; e < t.n; ++e)
    for (int j = 0; j < t.e[e].nslabs; ++j)
      for (int r = 0; r < rt; ++r) {
        const float* p = t.e[e].base + (long)j * t.e[e].step + (long)r * t.e[e].tile;
        const int n4 = r == rt - 1 ? t.e[e].n4_last : t.e[e].n4;
        for (int i = 0; i < n4; ++i) bad += !hit[(size_t)(p - c.arena) / 4 + i];
      }
  return bad;
}

int main() {
  int bad = 0, with = 0, without = 0, armed_n = 0, filled_n = 0, refused = 0;
  static_assert(kBdecAhead >= 1 && kBdecAhead <= kArmAhead - 2, "the leader's stores must be ordered behind the sentinels of their slab");
  for (int cus : {256, 128, 64})
    for (int tl = 1; tl <= 4; ++tl) {
      const VrnnBwdDeal d0 = vrnn_bwd_deal(ctH, ctZ, ctR, tl, cus, false, true), d = vrnn_bwd_deal(ctH, ctZ, ctR, tl, cus, false, true, ctD);
      bad += !same(d0.grub, d.grub) || !same(d0.gb, d.gb) || !same(d0.wide_h, d.wide_h) || !same(d0.dz, d.dz) || !same(d0.prior, d.prior) ||
             !same(d0.post, d.post) || d0.split3 != d.split3 || d0.g != d.g || d0.def_n != d.def_n || d0.spare != d.spare;
      for (int k = 0; k < 3; ++k) bad += !same(d0.part[k], d.part[k]) || d0.bdec[k].nwg != 0;
      if (d.bdec[0].nwg == 0) {
        ++without;
        for (const LinkRange& r : d.bdec) bad += r.nwg != 0;
        bad += d.split3 && d.part[2].nwg == ctH * tl;  // ... and only for a reason: no third range, or not one partial-sum tile on each of its workgroups
        continue;
      }
      ++with;
      bad += !d.split3 || d.spare < 8;
      for (int k = 0; k < 3; ++k) {
        const LinkRange& r = d.bdec[k];
        bad += !same(LinkRange{k < 2 ? ctH : ctD, d.part[2].wg0, d.part[2].nwg}, r) || r.wg0 + r.nwg > cus;
        for (bool xcd : {false, true}) {
          const int most = most_tiles(r, tl, cus, xcd);
          bad += most < 1 || most > (k < 2 ? 1 : kMaxTiles);
        }
      }
      for (bool xcd : {false, true}) {
        int armers[4] = {0, 0, 0, 0};
        for (int w = d.part[2].wg0; w < d.part[2].wg0 + d.part[2].nwg; ++w) {
          TileIter mine(w, d.part[2].wg0, d.part[2].nwg, tl, ctH, xcd);
          int tiles = 0;
          for (TileIter it = mine; it.valid(); it.next()) ++tiles;
          bad += tiles != 1;  // exactly one partial-sum tile per armer
          if (tiles != 1) continue;
          ++armers[mine.r0() / 16];
          bool found = false;  // the phi part's tile (r, c) of this workgroup is its partial-sum tile
          for (TileIter it(w, d.bdec[2].wg0, d.bdec[2].nwg, tl, ctD, xcd); it.valid(); it.next())
            if (it.c() < ctH) { bad += found || it.c() != mine.c() || it.r0() != mine.r0(); found = true; }
          bad += !found;
        }
        for (int r = 0; r < tl; ++r) bad += armers[r] == 0 || (armers[r] & (armers[r] - 1)) != 0;
      }
    }
  // the flagship deal: B = 64 on 256 workgroups -> the leader on [192, 256), three tiles of bdec[2] per workgroup
  const VrnnBwdDeal f = vrnn_bwd_deal(ctH, ctZ, ctR, 4, 256, false, true, ctD);
  bad += f.bdec[0].wg0 != 192 || f.bdec[0].nwg != 64 || f.bdec[2].nwg != 64 || tiles_per_workgroup(4, ctD, 64, false) != 3;
  // no leader range: the shared deal, the K = 3R link unsplit, a chip without a spare range
  bad += vrnn_bwd_deal(ctH, ctZ, ctR, 4, 256, true, true, ctD).bdec[0].nwg != 0;
  bad += vrnn_bwd_deal(ctH, ctZ, ctR, 4, 256, false, false, ctD).bdec[0].nwg != 0;
  bad += vrnn_bwd_deal(ctH, ctZ, ctR, 4, 128, false, true, ctD).bdec[2].nwg != 0;

  // arming: the program's polled words, T' around the look-ahead and the lead
  const size_t cap = (size_t)3 << 30;
  void* const mem = mmap(nullptr, cap, PROT_NONE, MAP_PRIVATE | MAP_ANONYMOUS | MAP_NORESERVE, -1, 0);
  if (mem == MAP_FAILED) { printf("backward decoder deal: cannot reserve addresses\n"); return 2; }
  for (int B : {5, 17, 33, 49, 64})
    for (int T : {kBdecAhead + 1, kArmAhead - 1, kArmAhead, kArmAhead + 1, 2 * kArmAhead + 3, 250})
      for (bool xcd : {false, true}) {
        const Case c = leader_case(static_cast<float*>(mem), B, T, 256);
        if (c.off > cap / 4 || c.p.ndesc != kBwdDecDesc || c.plan.tab.n != 21) { ++bad; continue; }
        bad += !one_tile_each(c.p, kBwdResident, xcd) || !one_tile_each(c.p, kBwdDecResident, xcd) || grid_of(c.p) > 256;
        const bool armed = applies(c, xcd);
        bad += armed != (T + 1 > kArmAhead);
        armed ? ++armed_n : ++filled_n;
        const int b = coverage(c, xcd, armed);
        if (b) printf("  B %d T' %d xcd %d: %d violations\n", B, T, (int)xcd, b);
        bad += b;
      }
  {
    const Case c = leader_case(static_cast<float*>(mem), 64, 11, 256);
    const bool ok = applies(c, false);
    Case wide = c;  // the unpolled link on workgroups that own no partial-sum tile: nothing would hold it behind the chain
    wide.p.d[10].wg0 = c.p.d[4].wg0; wide.p.d[10].nwg = 128;
    refused += !applies(wide, false);
    Case polled = c;  // the same operand as a polled one: not in the table
    polled.p.d[10].flags = DF_GENTLE;
    refused += !applies(polled, false);
    Case out = c;  // a leader operand that is not one of the table's buffers
    out.p.d[11].p[LIN_A] = static_cast<float*>(mem) + c.off + 1024;
    refused += !applies(out, false);
    Case full = c;  // more buffers than the table holds
    for (int i = 0; i < 4; ++i) full.plan.add(c.plan.tab.e[18]);
    refused += !applies(full, false);
    bad += !ok || refused != 4;
  }
  munmap(mem, cap);
  bad += with == 0 || without == 0 || armed_n == 0 || filled_n == 0;  // every outcome was seen
  printf("backward decoder deal: %d errors (%d deals with the leader, %d without; %d armed launches, %d filled by the host, %d of 4 bad programs refused)\n",
         bad, with, without, armed_n, filled_n, refused);
  return bad != 0;
}
