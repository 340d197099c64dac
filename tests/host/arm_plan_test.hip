// The look-ahead arming plan of the static VRNN walks (csrc/vrnn_static.h: ArmEntry, arm_share, arm_rank, arm_applies), replayed on
// the host exactly as the kernels and the prefix fill compute it: the deals of B = 5, 17, 33, 49, 64 on 256 workgroups, T' = 1,
// kArmAhead - 1, kArmAhead, kArmAhead + 1, 2 kArmAhead + 3 and 250, forward and backward, in both TileIter modes.
//   - the host's part (the prefix of an armed launch, the full regions of any other) plus all workgroups' chunks cover every polled
//     16-byte word at least once;
//   - no chunk leaves its buffer, every chunk lies in its workgroup's row tile, every chunk is 16-byte aligned;
//   - a program the rules do not cover (two tiles per armer, a row tile without armer, an operand outside the table, a misaligned
//     buffer, armers that own tiles of the links they are meant to wait through) is refused.
// The buffers are addresses in a reserved, never touched mapping: nothing is dereferenced.
#include "vrnn_static.h"
#include <sys/mman.h>
#include <cstdio>
#include <cstring>
#include <vector>
namespace blvm { void set_error(const char*, ...) {} }
using namespace blvm::pchain;

constexpr int H = 256, Z = 256, R = 512, ctH = H / 16, ctZ = Z / 16, ctR = R / 16;

struct Buf {
  float* p;
  size_t floats;
};
struct Arena {
  float* base;
  size_t off = 0, cap;
  Buf take(size_t n) {
    Buf b{base + off, n};
    off += (n + 3) & ~(size_t)3;
    return b;
  }
};

struct Case {
  Program p{};
  ArmPlan plan;
  std::vector<Buf> bufs;  // buffer of table entry i
  int link, cand0, ncand;
  bool fwd;
  int nstride = 1;
  void desc(int kind, const LinkRange& l, const float* operand, long stride) {
    Desc& d = p.d[p.ndesc++];
    d = Desc{};
    d.kind = kind; d.ct = l.ct; d.wg0 = l.wg0; d.nwg = l.nwg;
    const int slot = arm_operand_slot(kind);
    d.p[slot] = operand;
    p.stride[nstride] = stride;
    d.sidx[slot] = (unsigned char)nstride++;
  }
  void t16(Arena& ar, int width, int rt, int nslabs, bool rev) {
    const Buf b = ar.take((size_t)nslabs * rt * 16 * width);
    bufs.push_back(b);
    plan.add(arm_t16(b.p, width, rt, nslabs, rev));
  }
  void rm(Arena& ar, int ld, int B, int nslabs, bool rev, int extra_slabs = 0) {
    const Buf b = ar.take((size_t)(nslabs + extra_slabs) * B * ld);
    bufs.push_back(Buf{b.p, (size_t)nslabs * B * ld});
    plan.add(arm_rm(b.p, ld, B, nslabs, rev));
  }
};

// the forward program's ranges and polled buffers as vrnn.hip lays them out (decoder range included)
static Case forward_case(Arena& ar, int B, int T, int cus = 256) {
  Case c;
  const int rt = (B + 15) / 16;
  const VrnnFwdDeal d = vrnn_fwd_deal(ctH, ctZ, ctR, rt, cus, false, 120);
  c.p.B = B; c.p.S = T; c.p.rt_group = 1;
  c.rm(ar, 3 * R, B, T, false);         // GHb
  c.rm(ar, H + R, B, T, false, 1);      // decin rows 0 .. T'-1 (row T' is not polled)
  c.t16(ar, R, rt, T + 1, false);       // H16
  for (int i = 0; i < 13; ++i) c.t16(ar, H, rt, T, false);  // P16[3], Q16[3], Z16, FZ16[3], PHI16, Y116, Y216
  c.rm(ar, H, B, T, false);             // Y1P
  c.plan.fill(c.bufs[0].p, sizeof(float) * c.bufs[0].floats);
  c.plan.fill(c.bufs[1].p, sizeof(float) * c.bufs[1].floats);
  c.plan.fill(c.bufs[2].p, sizeof(float) * (size_t)(c.bufs.back().p + c.bufs.back().floats - c.bufs[2].p));
  const float* h16 = c.bufs[2].p;
  const long xR = (long)rt * 16 * R, xH = (long)rt * 16 * H;
  c.desc(K_LIN, d.hproj, h16, xR);
  c.desc(K_LINSEQ, d.prior, h16, xR);
  c.desc(K_LINSEQ, d.post, h16, xR);
  c.desc(K_HEAD, d.head, c.bufs[5].p, xH);
  c.desc(K_LINSEQ, d.phi, c.bufs[9].p, xH);
  c.desc(K_GRU, d.gru, c.bufs[13].p, xH);
  c.fwd = true; c.link = 5; c.cand0 = d.post.wg0; c.ncand = d.hproj.wg0 - d.post.wg0;
  return c;
}
// the backward program (split3 form): S = T' + 1 steps, every buffer walked in reverse
static Case backward_case(Arena& ar, int B, int T) {
  Case c;
  const int rt = (B + 15) / 16;
  const VrnnBwdDeal d = vrnn_bwd_deal(ctH, ctZ, ctR, rt, 256, false, true);
  c.p.B = B; c.p.S = T + 1; c.p.rt_group = 1;
  c.rm(ar, R, B, T, true); c.rm(ar, R, B, T, true);             // GA, GB
  for (int i = 0; i < 6; ++i) c.t16(ar, H, rt, T, true);        // DP16[3], DQ16[3]
  c.t16(ar, 3 * R, rt, T, true); c.t16(ar, 3 * R, rt, T, true);  // DGI16, DGH16
  for (int i = 0; i < 4; ++i) c.t16(ar, H, rt, T, true);        // DPHI16[4]
  c.t16(ar, 2 * Z, rt, T, true); c.t16(ar, 2 * Z, rt, T, true);  // DPH16, DQH16
  c.t16(ar, H, rt, T, true); c.t16(ar, H, rt, T, true);          // DPHI16b, DPHI16c
  c.plan.fill(c.bufs[0].p, sizeof(float) * (size_t)(c.bufs.back().p + c.bufs.back().floats - c.bufs[0].p));
  const long xH = (long)rt * 16 * H, x3R = (long)rt * 16 * 3 * R, x2Z = (long)rt * 16 * 2 * Z;
  auto last = [&](int i, long step) { return c.bufs[i].p + (long)(T - 1) * step; };
  c.desc(K_GRUB, d.grub, c.bufs[2].p + (long)T * xH, -xH);  // (one slab past the end at step 0: the step has no product)
  for (int k = 0; k < 3; ++k) c.desc(K_LIN, d.part[k], last(8, x3R) + (size_t)k * ctR * 256, -x3R);
  c.desc(K_LIN, d.gb, last(9, x3R), -x3R);
  c.desc(K_LIN, d.wide_h, last(13, xH), -xH);
  c.desc(K_LINSEQ, d.wide_h, last(12, xH), -xH);
  c.desc(K_DZ, d.dz, last(10, xH), -xH);
  c.desc(K_LINSEQ, d.prior, last(14, x2Z), -x2Z);
  c.desc(K_LINSEQ, d.post, last(15, x2Z), -x2Z);
  c.fwd = false; c.link = 3; c.cand0 = d.part[2].wg0; c.ncand = d.part[2].nwg;
  return c;
}

static bool applies(const Case& c, bool xcd) {
  return c.fwd ? arm_applies(c.p, c.plan.tab, c.link, {3, 4}, c.cand0, c.ncand, xcd) : arm_applies(c.p, c.plan.tab, c.link, {}, c.cand0, c.ncand, xcd);
}

// replays one launch; returns the number of violations
static int replay(const Case& c, const Arena& ar, bool xcd, bool* armed_out) {
  int bad = 0;
  const int rt = (c.p.B + 15) / 16;
  const ArmTable& t = c.plan.tab;
  std::vector<unsigned char> hit(ar.off / 4, 0);  // per 16-byte word of the arena
  auto mark = [&](const float* p, long n4, int entry, int r, const ArmEntry* e, int j) {
    if (n4 <= 0) return;
    const Buf& b = c.bufs[entry];
    bad += (reinterpret_cast<unsigned long long>(p) & 15) != 0;
    if (p < b.p || p + 4 * n4 > b.p + b.floats) { ++bad; return; }  // leaves its buffer (not marked: the map ends with the arena)
    if (e != nullptr) {  // a workgroup's chunk: inside row tile r of slab j
      const float* lo = e->base + (long)j * e->step + (long)r * e->tile;
      bad += p < lo || p + 4 * n4 > lo + 4L * (r == rt - 1 ? e->n4_last : e->n4);
    }
    for (long i = 0; i < n4; ++i) hit[(size_t)(p - ar.base) / 4 + i] = 1;
  };
  const bool armed = applies(c, xcd);
  *armed_out = armed;
  if (!armed) {
    for (int i = 0; i < c.plan.nfull; ++i) {
      const float* p = static_cast<const float*>(c.plan.full[i].p);
      const size_t n4 = c.plan.full[i].bytes / 16;
      bad += (reinterpret_cast<unsigned long long>(p) & 15) != 0 || p < ar.base || p + 4 * n4 > ar.base + ar.off;
      for (size_t k = 0; k < n4; ++k) hit[(size_t)(p - ar.base) / 4 + k] = 1;
    }
  } else {
    for (int e = 0; e < t.n; ++e)  // the prefix fill (arm_prefix_kernel)
      for (int j = 0; j < std::min(t.e[e].nslabs, kArmAhead); ++j)
        for (int r = 0; r < rt; ++r) mark(t.e[e].base + (long)j * t.e[e].step + (long)r * t.e[e].tile, r == rt - 1 ? t.e[e].n4_last : t.e[e].n4, e, r, nullptr, j);
    for (int w = c.cand0; w < c.cand0 + c.ncand; ++w) {  // the armers (arm_rank_dev, arm_ahead)
      int r, k, n;
      if (!arm_rank(c.p, c.link, c.cand0, c.ncand, xcd, w, &r, &k, &n)) continue;
      bad += r < 0 || r >= rt || k < 0 || k >= n;
      for (int s = 0; s < c.p.S; ++s)
        for (int e = 0; e < t.n; ++e) {
          const int j = s + kArmAhead;
          if (j >= t.e[e].nslabs) continue;
          int first, count;
          bad += (n & (n - 1)) != 0;
          arm_share(t.e[e], r, rt, k, __builtin_ctz(n), &first, &count);
          mark(t.e[e].base + (long)j * t.e[e].step + (long)r * t.e[e].tile + 4L * first, count, e, r, &t.e[e], j);
        }
    }
  }
  // every polled word: all slabs of every buffer, the rows of every row tile
  for (int e = 0; e < t.n; ++e)
    for (int j = 0; j < t.e[e].nslabs; ++j)
      for (int r = 0; r < rt; ++r) {
        const float* p = t.e[e].base + (long)j * t.e[e].step + (long)r * t.e[e].tile;
        const int n4 = r == rt - 1 ? t.e[e].n4_last : t.e[e].n4;
        for (int i = 0; i < n4; ++i) bad += !hit[(size_t)(p - ar.base) / 4 + i];
      }
  return bad;
}

int main() {
  const size_t cap = (size_t)3 << 30;
  void* const mem = mmap(nullptr, cap, PROT_NONE, MAP_PRIVATE | MAP_ANONYMOUS | MAP_NORESERVE, -1, 0);
  if (mem == MAP_FAILED) { printf("arm plan: cannot reserve addresses\n"); return 2; }
  int bad = 0, armed_n = 0, filled_n = 0, refused = 0;
  for (int B : {5, 17, 33, 49, 64})
    for (int T : {1, kArmAhead - 1, kArmAhead, kArmAhead + 1, 2 * kArmAhead + 3, 250})
      for (bool fwd : {true, false})
        for (bool xcd : {false, true}) {
          Arena ar{static_cast<float*>(mem), 0, cap / 4};
          const Case c = fwd ? forward_case(ar, B, T) : backward_case(ar, B, T);
          if (ar.off > ar.cap) { ++bad; continue; }
          bool armed = false;
          const int b = replay(c, ar, xcd, &armed);
          if (b) printf("  B %d T' %d %s xcd %d: %d violations\n", B, T, fwd ? "forward" : "backward", (int)xcd, b);
          bad += b;
          armed ? ++armed_n : ++filled_n;
          bad += armed != (T > kArmAhead - (fwd ? 0 : 1)) ;  // armed exactly where the walk has more steps than the look-ahead (S = T' | T' + 1)
        }
  // programs the rules do not cover are refused
  {
    Arena ar{static_cast<float*>(mem), 0, cap / 4};
    Case c = forward_case(ar, 64, 11);
    bool ok = applies(c, false);
    Case two = c;  // half the workgroups for the GRU link: two tiles per armer
    two.p.d[5].nwg /= 2; two.cand0 = 0; two.ncand = two.p.d[5].nwg;
    refused += !applies(two, false);
    Case none = c;  // candidates that own no tile of the link: a row tile without armer
    none.cand0 = c.p.d[0].wg0; none.ncand = 8;
    refused += !applies(none, false);
    Case out = c;  // an operand that is not one of the table's buffers
    out.p.d[3].p[HEAD_P16] = static_cast<float*>(mem) + ar.off + 1024;
    refused += !applies(out, false);
    Case odd = c;  // a buffer off the 16-byte grid
    odd.plan.tab.e[4].base += 1;
    refused += !applies(odd, false);
    Case still = c;  // an operand that does not step: nothing to poll
    still.p.stride[still.p.d[4].sidx[LINSEQ_A0]] = 0;
    refused += !applies(still, false);
    Case wide = c;  // more candidates than one ballot ranks
    wide.ncand = kArmCandidates + 8;
    refused += !applies(wide, false);
    Arena ar2{static_cast<float*>(mem), 0, cap / 4};
    const Case busy = forward_case(ar2, 64, 11, 128);  // on 128 workgroups the posterior half owns tiles of the heads: it does not wait
    refused += !applies(busy, false);
    bad += !ok || refused != 7;
  }
  bad += armed_n == 0 || filled_n == 0;  // both outcomes were seen
  munmap(mem, cap);
  printf("arm plan: %d errors (%d armed launches, %d filled by the host, %d of 7 bad programs refused)\n", bad, armed_n, filled_n, refused);
  return bad != 0;
}
