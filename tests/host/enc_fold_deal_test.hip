// The d_enc follower of the VRNN backward deal (csrc/vrnn_static.h vrnn_bwd_deal with ctX > 0, kBencLag), replayed on the host for
// B = 1 .. 64, T' = 3, 4, 5, 6, 11, both TileIter modes, with and without the decoder leader:
//   - the other ranges never depend on ctX, and without ctX there is no follower range;
//   - where the range exists it is the posterior half: every workgroup of the half owns exactly one tile of benc[0] and the SAME tile
//     (r, c) of benc[1], no other workgroup owns any, and the half owns no tile of the summing link, the phi_z run or dz;
//   - replaying the walk (steps kBencLag .. T', the slab of walk step s - kBencLag), every word of EP and of d_enc is written exactly once;
//   - every polled word of the extended program (EP among them) gets its sentinel exactly once — from the prefix fill or from one
//     armer's chunk where the launch arms, from the full fill where it does not — and an armed slab is armed before its producer can
//     store it: the armer's stores of slab j drain in front of its partial-sum tile of walk step j - kArmAhead + 1, and the follower's
//     tile of slab j runs at walk step j + kBencLag behind the GRU-backward tiles of walk step j, which need that row tile's partial
//     sums of walk step j - 1;
//   - arm_applies accepts the extended programs where T' + 1 > kArmAhead and refuses the mutated ones;
//   - the arming table with the follower's entry fits (kArmMax), and a table of kArmMax entries is what the kernel arguments were
//     sized for (the static_assert on the whole argument structs is vrnn_static.hip's: the build checks it).
// The buffers are addresses in a reserved, never touched mapping: nothing is dereferenced.
#include "vrnn_static.h"
#include <sys/mman.h>
#include <cstdio>
#include <vector>
namespace blvm { void set_error(const char*, ...) {} }
using namespace blvm::pchain;

constexpr int H = 256, Z = 256, R = 512, X = 256, ctH = H / 16, ctZ = Z / 16, ctR = R / 16, ctD = (H + R) / 16, ctX = X / 16;

static bool same(const LinkRange& a, const LinkRange& b) { return a.ct == b.ct && a.wg0 == b.wg0 && a.nwg == b.nwg; }

struct Case {
  Program p{};
  ArmPlan plan;
  std::vector<float*> base;  // buffer of table entry i
  std::vector<size_t> floats;
  float* arena;
  size_t off = 0;
  int nstride = 1, spare0 = 0, nspare = 0, ep = -1, benc0 = -1;
  VrnnBwdDeal deal;
  float* take(size_t n) { float* q = arena + off; off += (n + 3) & ~(size_t)3; return q; }
  int t16(int width, int rt, int T) {
    float* b = take((size_t)T * rt * 16 * width);
    base.push_back(b); floats.push_back((size_t)T * rt * 16 * width);
    plan.add(arm_t16(b, width, rt, T, true));
    return (int)base.size() - 1;
  }
  int rm(int ld, int B, int T) {
    float* b = take((size_t)T * B * ld);
    base.push_back(b); floats.push_back((size_t)T * B * ld);
    plan.add(arm_rm(b, ld, B, T, true));
    return (int)base.size() - 1;
  }
  Desc& desc(int kind, const LinkRange& l, const float* operand, long stride, int flags, int s_begin, int s_end) {
    Desc& d = p.d[p.ndesc++];
    d = Desc{};
    d.kind = kind; d.ct = l.ct; d.wg0 = l.wg0; d.nwg = l.nwg; d.flags = flags; d.s_begin = s_begin; d.s_end = s_end;
    const int slot = arm_operand_slot(kind);
    d.p[slot] = operand;
    p.stride[nstride] = stride;
    d.sidx[slot] = (unsigned char)nstride++;
    return d;
  }
};

// the backward program as vrnn.hip lays it out: 18 table entries and 10 descriptors, + 3 and 3 with the decoder leader, + 1 and 2
// with the follower (the last two descriptors)
static Case program(float* mem, int B, int T, int cus, bool lead, bool enc) {
  Case c;
  c.arena = mem;
  const int rt = (B + 15) / 16, L = kBdecAhead;
  const VrnnBwdDeal d = vrnn_bwd_deal(ctH, ctZ, ctR, rt, cus, false, true, lead ? ctD : 0, enc ? ctX : 0);
  c.deal = d;
  c.p.B = B; c.p.S = T + 1; c.p.rt_group = 1;
  c.rm(R, B, T); c.rm(R, B, T);                          // 0, 1: GA, GB
  for (int i = 0; i < 6; ++i) c.t16(H, rt, T);            // 2 .. 7: DP16[0], DQ16[0], DP16[1], DQ16[1], DP16[2], DQ16[2]
  c.t16(3 * R, rt, T); c.t16(3 * R, rt, T);                // 8, 9: DGI16, DGH16
  for (int i = 0; i < 4; ++i) c.t16(H, rt, T);            // 10 .. 13: DPHI16[4]
  c.t16(2 * Z, rt, T); c.t16(2 * Z, rt, T);                // 14, 15: DPH16, DQH16
  c.t16(H, rt, T); c.t16(H, rt, T);                        // 16, 17: DPHI16b, DPHI16c
  int dy2 = -1, dy1 = -1;
  if (lead) { dy2 = c.t16(H, rt, T); dy1 = c.t16(H, rt, T); c.rm(H + R, B, T); }  // 18 .. 20: DY216, DY116, DD
  const size_t polled = c.off;
  float* dz3 = c.take((size_t)T * B * 1920);  // complete before the launch: not in the table
  if (enc && d.benc[0].nwg > 0) c.ep = c.rm(X, B, T);  // EP: behind everything else, a fill region of its own
  c.plan.fill(c.base[0], sizeof(float) * polled);
  if (c.ep >= 0) c.plan.fill(c.base[c.ep], sizeof(float) * c.floats[c.ep]);
  const long xH = (long)rt * 16 * H, x3R = (long)rt * 16 * 3 * R, x2Z = (long)rt * 16 * 2 * Z;
  auto last = [&](int i, long step, int ahead = 0) { return c.base[i] + (long)(T - 1 - ahead) * step; };
  c.desc(K_GRUB, d.grub, c.base[2] + (long)T * xH, -xH, 0, 0, T + 1);
  for (int k = 0; k < 3; ++k) c.desc(K_LIN, d.part[k], last(8, x3R) + (size_t)k * ctR * 256, -x3R, lead && k == 2 ? DF_ADD_POLLED | DF_ADD_EARLY : 0, 0, T);
  c.desc(K_LIN, d.gb, last(9, x3R), -x3R, DF_ADD_POLLED | (lead ? DF_ADD2_POLLED : 0) | DF_RM_SC1 | DF_GENTLE | DF_CANARY, 0, T);
  c.desc(K_LIN, d.wide_h, last(13, xH), -xH, DF_A_SUM3, 0, T);
  c.desc(K_LINSEQ, d.wide_h, last(12, xH), -xH, DF_SEQ_GATE, 0, T);
  c.desc(K_DZ, d.dz, last(10, xH), -xH, 0, 0, T);
  c.desc(K_LINSEQ, d.prior, last(14, x2Z), -x2Z, DF_SEQ_GATE, 0, T);
  c.desc(K_LINSEQ, d.post, last(15, x2Z), -x2Z, DF_SEQ_GATE, 0, T);
  if (lead) {
    c.desc(K_LIN, d.bdec[0], dz3 + (long)(T - 1 - L) * B * 1920, -(long)B * 1920, DF_A_PLAIN | DF_GENTLE, 0, T - L);
    c.desc(K_LIN, d.bdec[1], last(dy2, xH, L), -xH, DF_GENTLE | DF_CANARY, 0, T - L);
    c.desc(K_LIN, d.bdec[2], last(dy1, xH, L), -xH, DF_RM_SC1 | DF_GENTLE | DF_CANARY, 0, T - L);
  }
  if (c.ep >= 0) {  // a slab back: walk step s multiplies the slabs of walk step s - kBencLag
    c.benc0 = c.p.ndesc;
    c.desc(K_LIN, d.benc[0], last(8, x3R, -kBencLag), -x3R, DF_RM_SC1 | DF_GENTLE | DF_CANARY, kBencLag, T + 1);
    c.desc(K_LIN, d.benc[1], last(3, xH, -kBencLag), -xH, DF_ADD_POLLED | DF_GENTLE | DF_CANARY, kBencLag, T + 1);
  }
  c.spare0 = d.part[2].wg0; c.nspare = d.part[2].nwg;
  return c;
}
static bool applies(const Case& c, bool xcd) { return arm_applies(c.p, c.plan.tab, 3, {}, c.spare0, c.nspare, xcd); }

// every polled word of every table entry gets its sentinel exactly once, no chunk outside its buffer; armed: the slab of walk step
// j >= kArmAhead is armed at walk step j - kArmAhead, and for the follower's EP that is in front of the store (see the head)
static int sentinels(const Case& c, bool xcd, bool armed) {
  int bad = 0;
  const int rt = (c.p.B + 15) / 16;
  const ArmTable& t = c.plan.tab;
  std::vector<unsigned char> hit(c.off / 4 + 1, 0);
  auto mark = [&](const float* p, long n4, int e) {
    if (n4 <= 0) return;
    if ((reinterpret_cast<unsigned long long>(p) & 15) != 0 || p < c.base[e] || p + 4 * n4 > c.base[e] + c.floats[e]) { ++bad; return; }
    for (long i = 0; i < n4; ++i) {
      unsigned char& h = hit[(size_t)(p - c.arena) / 4 + i];
      if (h < 255) ++h;
    }
  };
  if (!armed) {
    for (int i = 0; i < c.plan.nfull; ++i) {
      const float* p = static_cast<const float*>(c.plan.full[i].p);
      for (size_t k = 0; k < c.plan.full[i].bytes / 16; ++k) ++hit[(size_t)(p - c.arena) / 4 + k];
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
          // causal order for EP: armed behind the armer's partial-sum tile of walk step s, drained in front of the one of s + 1; the
          // producer of slab j runs at walk step j + kBencLag behind partial sums of walk step j - 1 of the same row tile
          if (e == c.ep) bad += !(s + 1 <= j - 1) || j + kBencLag >= c.p.S;
        }
    }
  }
  for (int e = 0; e < t.n; ++e)
    for (int j = 0; j < t.e[e].nslabs; ++j)
      for (int r = 0; r < rt; ++r) {
        const float* p = t.e[e].base + (long)j * t.e[e].step + (long)r * t.e[e].tile;
        const int n4 = r == rt - 1 ? t.e[e].n4_last : t.e[e].n4;
        for (int i = 0; i < n4; ++i) bad += hit[(size_t)(p - c.arena) / 4 + i] != 1;
      }
  return bad;
}

// the follower's ownership and the walk replayed: writes of EP and d_enc per (time step, row, column tile)
static int replay(const Case& c, int cus, bool xcd) {
  int bad = 0;
  const int B = c.p.B, rt = (B + 15) / 16, T = c.p.S - 1;
  const VrnnBwdDeal& d = c.deal;
  const Desc &e0 = c.p.d[c.benc0], &e1 = c.p.d[c.benc0 + 1];
  bad += !same(d.benc[0], d.benc[1]) || !same(d.benc[0], LinkRange{ctX, d.post.wg0, d.post.nwg}) || c.benc0 != c.p.ndesc - kBwdEncLinks;
  bad += e0.s_begin != kBencLag || e0.s_end != T + 1 || e1.s_begin != kBencLag || e1.s_end != T + 1;
  std::vector<int> ep((size_t)T * B * ctX, 0), de((size_t)T * B * ctX, 0);
  for (int w = 0; w < cus; ++w) {
    const bool post = w >= d.post.wg0 && w < d.post.wg0 + d.post.nwg;
    int n0 = 0, n1 = 0, r_ = -1, c_ = -1;
    for (TileIter it(w, e0.wg0, e0.nwg, rt, e0.ct, xcd); it.valid(); it.next()) { ++n0; r_ = it.r0(); c_ = it.c(); }
    for (TileIter it(w, e1.wg0, e1.nwg, rt, e1.ct, xcd); it.valid(); it.next()) { ++n1; bad += it.r0() != r_ || it.c() != c_; }
    bad += n0 != (post ? 1 : 0) || n1 != n0;
    if (post)  // the role runs no visit of the links between the partial sum and the run
      for (int i : {5, 6, 7}) bad += TileIter(w, c.p.d[i].wg0, c.p.d[i].nwg, rt, c.p.d[i].ct, xcd).valid();
    if (n0 != 1 || r_ < 0 || c_ < 0 || c_ >= ctX) continue;
    for (int s = 0; s < c.p.S; ++s) {
      const int t = T - 1 - (s - kBencLag);  // the time step of walk step s - kBencLag
      for (const Desc* e : {&e0, &e1}) {
        if (s < e->s_begin || s >= e->s_end) continue;
        if (t < 0 || t >= T) { ++bad; continue; }
        for (int row = r_; row < r_ + 16 && row < B; ++row) ++(e == &e0 ? ep : de)[((size_t)t * B + row) * ctX + c_];
      }
    }
  }
  for (int v : ep) bad += v != 1;
  for (int v : de) bad += v != 1;
  return bad;
}

int main() {
  int bad = 0, with = 0, without = 0, armed_n = 0, filled_n = 0, refused = 0;
  static_assert(kBencLag >= 1, "DQ0 of a time step is published at the end of its own walk step");
  static_assert(kBwdEncDesc == kBwdDesc + 2 && kBwdDecEncDesc == kBwdDecDesc + 2 && kBwdDecEncDesc <= kMaxDesc && kBwdDecEncDesc <= 16, "the follower's links are the last two; a poll's code names a descriptor in four bits");
  static_assert(sizeof(ArmTable) <= 4096 - 3320, "what the backward walk's other arguments leave of the 4 KB of a launch");
  for (int cus : {256, 128, 64})
    for (int tl = 1; tl <= 4; ++tl)
      for (int lead : {0, 1}) {
        const VrnnBwdDeal d0 = vrnn_bwd_deal(ctH, ctZ, ctR, tl, cus, false, true, lead ? ctD : 0), d = vrnn_bwd_deal(ctH, ctZ, ctR, tl, cus, false, true, lead ? ctD : 0, ctX);
        bad += !same(d0.grub, d.grub) || !same(d0.gb, d.gb) || !same(d0.wide_h, d.wide_h) || !same(d0.dz, d.dz) || !same(d0.prior, d.prior) ||
               !same(d0.post, d.post) || d0.split3 != d.split3 || d0.g != d.g || d0.def_n != d.def_n || d0.spare != d.spare;
        for (int k = 0; k < 3; ++k) bad += !same(d0.part[k], d.part[k]) || !same(d0.bdec[k], d.bdec[k]);
        bad += d0.benc[0].nwg != 0 || d0.benc[1].nwg != 0;
        if (d.benc[0].nwg == 0) {
          ++without;
          bad += d.benc[1].nwg != 0;
          bad += d.split3 && ctX * tl == d.post.nwg && d.wide_h.nwg <= d.post.wg0 && d.dz.nwg <= d.post.wg0;  // ... and only for a reason
          continue;
        }
        ++with;
        bad += !d.split3 || d.benc[0].wg0 + d.benc[0].nwg > cus;
        for (bool xcd : {false, true}) bad += tiles_per_workgroup(tl, ctX, d.benc[0].nwg, xcd) != 1;
      }
  // the flagship deal: B = 64 on 256 workgroups -> the follower on [64, 128); none under the shared deal or with the K = 3R link unsplit
  const VrnnBwdDeal f = vrnn_bwd_deal(ctH, ctZ, ctR, 4, 256, false, true, ctD, ctX);
  bad += f.benc[0].wg0 != 64 || f.benc[0].nwg != 64 || f.bdec[0].wg0 != 192;
  bad += vrnn_bwd_deal(ctH, ctZ, ctR, 4, 256, true, true, ctD, ctX).benc[0].nwg != 0;
  bad += vrnn_bwd_deal(ctH, ctZ, ctR, 4, 256, false, false, ctD, ctX).benc[0].nwg != 0;

  const size_t cap = (size_t)3 << 30;
  void* const mem = mmap(nullptr, cap, PROT_NONE, MAP_PRIVATE | MAP_ANONYMOUS | MAP_NORESERVE, -1, 0);
  if (mem == MAP_FAILED) { printf("d_enc follower deal: cannot reserve addresses\n"); return 2; }
  for (int B = 1; B <= 64; ++B)
    for (int T : {3, 4, 5, 6, 11})
      for (int lead : {0, 1})
        for (bool xcd : {false, true}) {
          const Case c = program(static_cast<float*>(mem), B, T, 256, lead, true);
          const int want_desc = lead ? kBwdDecEncDesc : kBwdEncDesc, want_tab = (lead ? 21 : 18) + 1;
          if (c.off > cap / 4 || c.ep < 0 || c.p.ndesc != want_desc || c.plan.tab.n != want_tab || c.plan.tab.n > kArmMax) { ++bad; continue; }
          bad += !one_tile_each(c.p, kBwdResident, xcd) || (lead && !one_tile_each(c.p, kBwdDecResident, xcd)) ||
                 !one_tile_each(c.p, {c.benc0, c.benc0 + 1}, xcd) || grid_of(c.p) > 256;
          const bool armed = applies(c, xcd);
          bad += armed != (T + 1 > kArmAhead);
          armed ? ++armed_n : ++filled_n;
          int b = sentinels(c, xcd, armed) + replay(c, 256, xcd);
          if (b) printf("  B %d T' %d leader %d xcd %d: %d violations\n", B, T, lead, (int)xcd, b);
          bad += b;
        }
  for (int lead : {0, 1}) {
    const Case c = program(static_cast<float*>(mem), 64, 11, 256, lead, true);
    const bool ok = applies(c, false);
    int r = 0;
    Case plain = c;  // the follower's first link on an operand nothing holds behind the chain: its workgroups own no partial-sum tile of the armers' link
    plain.p.d[c.benc0].flags |= DF_A_PLAIN;
    r += !applies(plain, false);
    Case out = c;  // an operand that is not one of the table's buffers
    out.p.d[c.benc0 + 1].p[LIN_A] = static_cast<float*>(mem) + c.off + 1024;
    r += !applies(out, false);
    Case full = c;  // more buffers than the table holds
    for (int i = 0; i < kArmMax; ++i) full.plan.add(c.plan.tab.e[c.ep]);
    r += !applies(full, false);
    Case groups = c;  // row groups
    groups.p.rt_group = 2;
    r += !applies(groups, false);
    Case stepless = c;  // an operand that does not step: every step would poll the same slab
    stepless.p.stride[c.p.d[c.benc0].sidx[LIN_A]] = 0;
    r += !applies(stepless, false);
    bad += !ok || r != 5;
    refused += r;
  }
  munmap(mem, cap);
  bad += with == 0 || without == 0 || armed_n == 0 || filled_n == 0;  // every outcome was seen
  printf("d_enc follower deal: %d errors (%d deals with the follower, %d without; %d armed launches, %d filled by the host, %d of 10 bad programs refused)\n",
         bad, with, without, armed_n, filled_n, refused);
  return bad != 0;
}
