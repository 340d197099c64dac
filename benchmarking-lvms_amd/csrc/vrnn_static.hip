// vrnn_static.hip — persistent chains whose walk is fixed at compile time (the "static walk"), against pchain.hip's interpreter.
//
// pchain_kernel walks a program of descriptors: every visit of a descriptor extracts its fields with v_readlane, switches on the
// tile kind and selects flags and pointers — ≈ 350 scalar instructions that all 16 waves of a workgroup execute, ≈ 1 µs per visit
// against a 1.5–1.7 µs tile.  A static walk knows the kinds, flags, K values and run lengths of its program as
// constants; only base pointers and per-step strides arrive as kernel arguments (s_load), and a step's address is base + s * stride
// in scalar registers at the point of use.  The tiles (pchain.h) and the hand-off protocol are the interpreter's, unchanged.
//
// The host builds the same pchain::Program as for the interpreter and converts it here; a program of any other shape is "not
// applicable" (return value 1) and vrnn_launch falls back to the interpreter (pchain_run).
//
// Here: the VRNN forward and backward programs of vrnn.hip at B <= 64 on 16-row tiles, fp32, H = Z = 256, R = 512 (the backward in
// its split3 form), and the gate the design passed first — the dependent linear chain of blvm_pchain_chain_probe as a static walk
// (blvm_pchain_static_chain_probe), priced per link against the engine and the bare tile loop (tools/probe_static_chain.py).
// A workgroup picks its role once from its index (prior half, posterior half, gentle range, spare range); each role's step loop
// is its own branch, a straight sequence of visits, and a visit is skipped when the deal gives the workgroup no tile of the link.
// The deal is fixed for the launch, so a workgroup owns the same tile of a link in every step: the links of the critical path keep that
// tile's weight fragments in registers (loaded once in front of the step loop; see "Resident weights" below and pchain.h) and a visit
// issues no weight load.  The converter refuses a program whose deal gives a workgroup two tiles of such a link.
// blvm_pchain_static(0) sends the VRNN programs to the interpreter (tests compare both paths in one process).
#include <algorithm>
#include <mutex>

#include "common.h"
#include "pchain.h"
#include "vrnn_static.h"

namespace blvm {
namespace {
using namespace pchain;

// a stepped pointer of a program: element (s, ...) at base + s * stride floats (|stride| < 2^31: checked on the host)
struct SPtr {
  float* base;
  int stride;
  __device__ __forceinline__ float* at(int s) const { return base + (long)s * stride; }
};

// A workgroup's tiles of one link, dealt by pchain.h's TileIter exactly as the interpreter deals them: lane k < kMaxTiles of the
// returned value holds tile k as r0 | column tile << 16 (-1: none), so a tile costs one v_readlane in the step loop.
// (kMaxTiles: vrnn_static.h)
// the workgroup of the deal this block is under the launch's placement (vrnn_static.h)
__device__ __forceinline__ int placed_wg(int place) { return place == kPlaceLocal ? place_wg((int)blockIdx.x) : (int)blockIdx.x; }
__device__ __forceinline__ int tile_lanes(int w, int wg0, int nwg, int rt, int ct, bool xcd) {
  TileIter it(w, wg0, nwg, rt, ct, xcd);
  const int lane = threadIdx.x & 63;
  it.j += lane * it.step;
  return (lane < kMaxTiles && it.valid()) ? (it.r0() | (it.c() << 16)) : -1;
}
__device__ __forceinline__ int tile_count(int lanes) { return __popcll(__ballot(lanes >= 0)); }  // (the valid lanes are 0 .. n-1)

// ---- anatomy of the resident path (-DPCHAIN_TPROF builds only; tools/probe_static_anatomy.py) ---------------------------------
// Every wave adds, per visit kind (slot) and wave class (0: the epilogue waves 0 .. 3, 1: waves 4 .. 15), {tiles, polls, ticks from
// the first issue to the successful poll, ticks from there to the tile's last T16 store (waves that store nothing: to the tile's
// end)} to a table in LDS; the first workgroup of each role copies its table to the blvm_pchain_profile buffer when it is done:
// words [kAnatBase + role * kAnatRole + (slot * 2 + class) * 4 + j].  Roles: 0 / 1 forward halves (or the chain probe), 2 / 3
// backward halves, 4 the backward's spare range.  Slot = 4 * (index of the link in its program) + link of the run.  (With the decoder
// leader the spare role also leaves, in slots 13 and 14, its walk steps and the ticks it spent in the leader's links, in the arming
// stores and in the whole loop: bwd_spare_leader; with the d_enc follower the backward's posterior half does the same for the
// follower's links: bwd_post_follower.)
constexpr int kAnatBase = 128, kAnatRole = 512, kAnatSlots = 64;  // (slots: 4 per descriptor of the longest program, 8 words each: a role's whole stretch)
#ifdef PCHAIN_TPROF
__device__ __forceinline__ void anat_begin(unsigned* tab) {
  for (int i = threadIdx.x; i < kAnatSlots * 8; i += blockDim.x) tab[i] = 0u;
  __syncthreads();
}
__device__ __forceinline__ void anat_arm(Poll& pl) { pl.rpolls = 0; pl.t_st = 0; }
__device__ __forceinline__ void anat_note(unsigned* tab, int slot, const Poll& pl) {
  const unsigned long long now = wall_clock64();
  if ((threadIdx.x & 63) == 0 && pl.rpolls != 0) {
    unsigned* q = tab + (slot * 2 + (threadIdx.x < 256 ? 0 : 1)) * 4;
    atomicAdd(q, 1u); atomicAdd(q + 1, pl.rpolls); atomicAdd(q + 2, (unsigned)(pl.t_ok - pl.t_issue));
    atomicAdd(q + 3, (unsigned)((pl.t_st != 0 ? pl.t_st : now) - pl.t_ok));
  }
}
__device__ __forceinline__ void anat_end(const unsigned* tab, unsigned long long* prof, int role, bool chosen) {
  __syncthreads();
  if (prof != nullptr && chosen)
    for (int i = threadIdx.x; i < kAnatSlots * 8; i += blockDim.x) prof[kAnatBase + role * kAnatRole + i] = tab[i];
}
#define ANAT(x) x
#else
#define ANAT(x)
#endif

// ---- gate: a linear-only chain ---------------------------------------------------------------------------------------------
// x_{s+1} = relu(x_s W^T + b) as ONE K_LIN link per step (the program of blvm_pchain_chain_probe), K = 256 or 512 at compile time
struct LinChainArgs {
  SPtr a16, orm, o16;
  const float *W, *bias;
  int ldo, n16, B, s0, S, wg0, nwg, ct, xcd, place;  // place: vrnn_static.h Place
  Ctl ctl;
  int pace_early, pace_epi;  // the run-time pacing policy's delays (PaceRt; the probe's sweep)
  ANAT(unsigned long long* prof;)
};
template <class PC>
__device__ __forceinline__ PC chain_pace(const LinChainArgs& a) {
  if constexpr (PC::paced) return PC{a.pace_early, a.pace_epi};
  else return PC();
}

// RES: the workgroup owns one tile; its weight fragments are loaded once, in front of the step loop (pchain.h "resident weights"),
// and a step is poll -> MFMA -> reduce -> epilogue.  !RES re-reads them every step (the form the probe prices the resident one against).
// PC: the poll pacing policy of the resident form (pchain.h): PaceOff, or PaceRt with the delays of the arguments.
template <int NW, int K, bool RES, class PC = PaceOff>
__global__ __launch_bounds__(NW * 64, 1) void static_lin_chain_kernel(LinChainArgs a) {
  __shared__ __attribute__((aligned(16))) float red[2][NW * 256];
  ANAT(__shared__ unsigned anat[kAnatSlots * 8]; anat_begin(anat);)
  const int w = placed_wg(a.place), B = a.B;
  const int tiles = tile_lanes(w, a.wg0, a.nwg, (B + 15) / 16, a.ct, a.place == kPlaceProgram && a.xcd != 0);
  const int nt = tile_count(tiles);
  if (nt == 0) return;
  Poll pl{a.ctl, 0u, false, 1};
  int par = 0;
  if constexpr (RES) {
    const int trc = __builtin_amdgcn_readlane(tiles, 0), r0 = trc & 0xffff, c0 = (trc >> 16) * 16;
    WRegs<OP_F32, 1, K / (16 * NW)> ws;
    const float* const Ws[1] = {a.W};
    const int cs[1] = {c0};
    load_w<NW, OP_F32, 1, K / (16 * NW)>(ws.w, Ws, cs, K);
    const PC pace = chain_pace<PC>(a);
    for (int s = a.s0; s < a.S; ++s) {
      pl.code = (unsigned)s << 4;
      auto late = [&]() { return LinLate{a.bias, nullptr, nullptr, 0, 0, false, true, 0.f, Out{a.orm.at(s), a.ldo, false, a.o16.at(s), a.n16}}; };
      ANAT(anat_arm(pl);)
      tile_lin_late<NW, OP_F32>(a.a16.at(s), 0, true, a.W, K, late, r0, c0, B, red[par], pl, nullptr, nullptr, 0, ws, pace);
      ANAT(anat_note(anat, 0, pl);)
      par ^= 1;
    }
    ANAT(anat_end(anat, a.prof, 0, w == a.wg0);)
    return;
  }
  for (int s = a.s0; s < a.S; ++s) {
    pl.code = (unsigned)s << 4;
    const float* A = a.a16.at(s);
    auto late = [&]() { return LinLate{a.bias, nullptr, nullptr, 0, 0, false, true, 0.f, Out{a.orm.at(s), a.ldo, false, a.o16.at(s), a.n16}}; };
    for (int tk = 0; tk < nt; ++tk) {
      const int trc = __builtin_amdgcn_readlane(tiles, tk);
      tile_lin_late<NW, false>(A, 0, true, a.W, K, late, trc & 0xffff, (trc >> 16) * 16, B, red[par], pl);
      par ^= 1;
    }
  }
}

// ---- the VRNN step programs (vrnn.hip), 16-row tiles, fp32, H = Z = 256, R = 512 ---------------------------------------------
constexpr int kH = 256, kR = 512;

// K_LIN (pchain.hip's pointer roles): the flags of a link are a template argument, everything else is data
struct LinArgs {
  SPtr a, a2, a3, add, gate, orm, o16, o16b;
  const float *W, *bias;
  int ld0, ld1, ld2, ld3, n16, n16b, w_width;
  float slope;
};
// K_LINSEQ: a run of N links, link 0 of K0 and the others of K
struct SeqArgs {
  SPtr a0, add0, aux[4], orm[4], o16[4];
  const float* W[4];
  int ld[4], ldadd0, ldgate, n16;
  float slope;
};
struct HeadArgs {
  SPtr P, Q, eps, mu_p, sd_p, mu_q, sd_q, raw_p, raw_q, muq_raw, z, z16, z16b;
  const float *Wp, *bp, *Wq, *bq;
  int ld3, n16, n16b, Z, residual;
  float beta, inv_beta, sd_eps;
};
struct GruArgs {
  SPtr X, xg, gh, hprev, hrm, h16, h16b, rg, ug, ng;
  const float *Wih, *bih;
  int ld0, ld3, n16, n16b, R;
};
struct DzArgs {
  SPtr D, add, mu_q, sd_q, mu_p, sd_p, eps, raw_q, raw_p, muq_raw, dqh, dqh16, dph, dph16;
  const float *WT, *c_raw, *c_fn;
  const int32_t* x_sl;
  int ld1, ld3, n16, Z, residual, stride, t0, first_gemm;
  float fn_floor, beta, sd_eps;
};
struct GrubArgs {
  SPtr D0, D1, g_in, rg, ug, ng, gh, hprev, dd, dgi, dgi16, dgh, dgh16, ga, g_add;
  const float *W0, *W1, *g_out;
  int ld0, ld1, ld3, n16, R, first_gemm, end_gates, first_gin;
};
// where a link runs: its workgroup range and column tiles (the same TileIter deal as the interpreter), the steps it is active in,
// and its index in the program (the abort code names it)
struct Deal {
  int wg0, nwg, ct, s_begin, s_end, idx;
};

// one visit = this workgroup's tiles of one link in one step.  `tiles`: tile_lanes of the link.  Every tile alternates the two
// reduction scratch buffers as pchain_kernel does.
struct Walk {
  float* red0;
  float* red1;
  int par, B;
  Poll pl;
  ANAT(unsigned* anat;)
  __device__ __forceinline__ float* red() { par ^= 1; return par ? red0 : red1; }
  __device__ __forceinline__ void at(const Deal& d, int s, bool gentle, unsigned li = 0) {
    pl.nap = gentle ? 16 : 1;
    pl.code = ((unsigned)s << 4) | (unsigned)d.idx | (li << 28);
  }
};

// Resident weights (pchain.h): a link of the critical path deals a workgroup at most ONE tile (the converter refuses any other
// deal), the same tile in every step, so the role loads that tile's weight fragments once in front of its step loop — load_* below,
// skipped where the deal gives the workgroup no tile — and a visit issues no weight load.  Per lane, 16 waves: 4 registers per
// product and 256 k.  The gentle links (several tiles per workgroup, off the critical path) keep reading theirs (WMem).
template <int K, int G = 1>
using Res = WRegs<OP_F32, G, K / 256>;
template <int N, int K0, int K>
struct RunRes {  // a run of N links, link 0 of K0 and the others of K
  Res<K0> first;
  Res<K> rest[N - 1];
};
__device__ __forceinline__ int tile_c0(int tiles) { return (__builtin_amdgcn_readlane(tiles, 0) >> 16) * 16; }  // the workgroup's one tile: lane 0

template <int NW, int K>
__device__ __forceinline__ void load_lin(Res<K>& r, const float* W, int ldw, int tiles, int nt) {
  if (nt == 0) return;
  const float* const Ws[1] = {W};
  const int cs[1] = {tile_c0(tiles)};
  load_w<NW, OP_F32, 1, K / 256>(r.w, Ws, cs, ldw > 0 ? ldw : K);  // (ldw: the packed rows' length where the link takes a K-range of them)
}
template <int NW, int N, int K0, int K>
__device__ __forceinline__ void load_run(RunRes<N, K0, K>& r, const SeqArgs& q, int tiles, int nt) {
  load_lin<NW, K0>(r.first, q.W[0], K0, tiles, nt);
#pragma unroll
  for (int li = 1; li < N; ++li) load_lin<NW, K>(r.rest[li - 1], q.W[li], K, tiles, nt);
}
template <int NW>
__device__ __forceinline__ void load_head(Res<kH, 4>& r, const HeadArgs& q, int tiles, int nt) {
  if (nt == 0) return;
  const int c0 = tile_c0(tiles);
  const float* const Ws[4] = {q.Wp, q.Wp, q.Wq, q.Wq};
  const int cs[4] = {c0, q.Z + c0, c0, q.Z + c0};
  load_w<NW, OP_F32, 4, 1>(r.w, Ws, cs, kH);
}
template <int NW>
__device__ __forceinline__ void load_gru(Res<kH, 3>& r, const GruArgs& q, int tiles, int nt) {
  if (nt == 0) return;
  const int c0 = tile_c0(tiles);
  const float* const Ws[3] = {q.Wih, q.Wih, q.Wih};
  const int cs[3] = {c0, q.R + c0, 2 * q.R + c0};
  load_w<NW, OP_F32, 3, 1>(r.w, Ws, cs, kH);
}
template <int NW>
__device__ __forceinline__ void load_grub(Res<kH, 2>& r, const GrubArgs& q, int tiles, int nt) {
  if (nt == 0) return;
  const int c0 = tile_c0(tiles);
  const float* const Ws[2] = {q.W0, q.W1};
  const int cs[2] = {c0, c0};
  load_w<NW, OP_F32, 2, 1>(r.w, Ws, cs, kH);
}

// Poll pacing (pchain.h): a link in lock step with its producers delays its first poll (Paced), by the same amount whatever the
// producer: longer delays behind the fat tiles (heads, GRU, GRU backward, dz), whose store comes later, measured no better.  Roles
// that reach a visit links before its operand exists (the posterior half's GRU tile; in the backward the posterior half's run and
// the spare range's partial sum) are not paced: a delay cannot fix the phase of a poll that started long ago.  The gentle links
// (WMem) are not paced either.  The values come from tools/probe_static_chain.py --paced, tools/probe_static_anatomy.py and a
// sweep of bench.py; -D overrides them for such sweeps.
#ifndef VRNN_PACE_EARLY
#define VRNN_PACE_EARLY 8  // s_sleep units, the waves that leave the previous tile at its barrier
#endif
#ifndef VRNN_PACE_EPI
#define VRNN_PACE_EPI 4  // the epilogue waves
#endif
typedef PaceK<VRNN_PACE_EARLY, VRNN_PACE_EPI> Paced;

// WS: Res<K> — the link's one tile on resident weights; WMem — every tile the deal gives, weights read per tile
// ROW_ONCE: the canary wait only in front of the first tile of a row tile.  A workgroup's tiles of a visit that share their row tile
// read the same [16, K] slab (with four row tiles on a range of 8 k workgroups: all of them), and once its canary words have arrived
// the later tiles' operand polls succeed at once; a canary per tile is a round trip and a barrier each for nothing.
// KT: the link's K, or 0: the descriptor's, passed as kdyn (the weights are then read per tile).  DF_A_PLAIN: A is row-major and
// complete before the launch.  add2, ldadd2: the second addend of a DF_ADD2_POLLED link (kept out of LinArgs: a launch's
// arguments are 4 KB at most).
template <int NW, int KT, int FLAGS, class PC = PaceOff, bool ROW_ONCE = false, class WS>
__device__ __forceinline__ void visit_lin(const LinArgs& q, const Deal& d, int s, int tiles, int nt, Walk& wk, const WS& ws, int kdyn = 0,
                                          const SPtr& add2 = SPtr{nullptr, 0}, int ldadd2 = 0) {
  if (nt == 0 || s < d.s_begin || s >= d.s_end) return;
  static_assert(KT != 0 || !WS::resident, "resident weights hold a K fixed at compile time");
  const int K = KT != 0 ? KT : kdyn;
  constexpr bool sum3 = (FLAGS & DF_A_SUM3) != 0, a_polled = (FLAGS & DF_A_PLAIN) == 0;
  wk.at(d, s, (FLAGS & DF_GENTLE) != 0);
  const float* A = q.a.at(s);
  const float* A2 = sum3 ? q.a2.at(s) : nullptr;
  const float* A3 = sum3 ? q.a3.at(s) : nullptr;
  auto late = [&]() {
    return LinLate{q.bias, q.add.at(s), q.gate.at(s), q.ld1, q.ld2, (FLAGS & DF_ADD_POLLED) != 0, (FLAGS & DF_RELU) != 0, q.slope,
                   Out{q.orm.at(s), q.ld3, (FLAGS & DF_RM_SC1) != 0, q.o16.at(s), q.n16, q.o16b.at(s), q.n16b},
                   (FLAGS & DF_ADD_EARLY) != 0, (FLAGS & DF_ADD2_POLLED) != 0 ? add2.at(s) : nullptr, ldadd2};
  };
  int seen_r0 = -1;  // (wave-uniform, as tr0: the branch around the canary's barrier is uniform)
  for (int tk = 0; tk < (WS::resident ? 1 : nt); ++tk) {
    const int trc = __builtin_amdgcn_readlane(tiles, tk), tr0 = trc & 0xffff, tc0 = (trc >> 16) * 16;
    if constexpr ((FLAGS & DF_CANARY) != 0 && a_polled) {
      if (!ROW_ONCE || tr0 != seen_r0) canary_wait(A, tr0, K, wk.pl, q.ld0);
      seen_r0 = tr0;
    }
    ANAT(anat_arm(wk.pl);)
    tile_lin_late<NW, OP_F32>(A, q.ld0, a_polled, q.W, K, late, tr0, tc0, wk.B, wk.red(), wk.pl, A2, A3, q.w_width, ws, PC());
    ANAT(anat_note(wk.anat, 4 * d.idx, wk.pl);)
  }
}

template <int NW, int N, int K0, int K, bool GATED, class P0 = PaceOff>  // P0: the first link's pacing; the others are Paced
__device__ __forceinline__ void visit_run(const SeqArgs& q, const Deal& d, int s, int tiles, int nt, Walk& wk, const RunRes<N, K0, K>& rr) {
  if (nt == 0 || s < d.s_begin || s >= d.s_end) return;
  const int trc = __builtin_amdgcn_readlane(tiles, 0), tr0 = trc & 0xffff, tc0 = (trc >> 16) * 16;
  const float* A = q.a0.at(s);
#pragma unroll
  for (int li = 0; li < N; ++li) {
    wk.at(d, s, false, (unsigned)li);
    auto late = [&]() {
      const float* aux = q.aux[li].at(s);
      return LinLate{GATED ? nullptr : aux, li == 0 ? q.add0.at(s) : nullptr, GATED ? aux : nullptr, q.ldadd0, q.ldgate, false, !GATED, q.slope,
                     Out{q.orm[li].at(s), q.ld[li], false, q.o16[li].at(s), q.n16}};
    };
    ANAT(anat_arm(wk.pl);)
    if (li == 0) tile_lin_late<NW, OP_F32>(A, 0, true, q.W[li], K0, late, tr0, tc0, wk.B, wk.red(), wk.pl, nullptr, nullptr, 0, rr.first, P0());
    else tile_lin_late<NW, OP_F32>(A, 0, true, q.W[li], K, late, tr0, tc0, wk.B, wk.red(), wk.pl, nullptr, nullptr, 0, rr.rest[li > 0 ? li - 1 : 0], Paced());
    ANAT(anat_note(wk.anat, 4 * d.idx + li, wk.pl);)
    A = q.o16[li].at(s);  // the next link multiplies what this one stored
  }
}

template <int NW, class PC = PaceOff>
__device__ __forceinline__ void visit_head(const HeadArgs& q, const Deal& d, int s, int tiles, int nt, Walk& wk, const Res<kH, 4>& ws) {
  if (nt == 0 || s < d.s_begin || s >= d.s_end) return;
  wk.at(d, s, false);
  const HeadOut o{q.mu_p.at(s), q.sd_p.at(s), q.mu_q.at(s), q.sd_q.at(s), q.raw_p.at(s), q.raw_q.at(s), q.muq_raw.at(s),
                  Out{q.z.at(s), q.ld3, false, q.z16.at(s), q.n16, q.z16b.at(s), q.n16b}};
  const int trc = __builtin_amdgcn_readlane(tiles, 0);
  ANAT(anat_arm(wk.pl);)
  tile_head<NW, OP_F32>(q.P.at(s), q.Q.at(s), true, q.Wp, q.bp, q.Wq, q.bq, q.eps.at(s), o, kH, q.Z, q.residual, q.beta, q.inv_beta, q.sd_eps,
                        trc & 0xffff, (trc >> 16) * 16, wk.B, wk.red(), wk.pl, ws, PC());
  ANAT(anat_note(wk.anat, 4 * d.idx, wk.pl);)
}

template <int NW, class PC = PaceOff>
__device__ __forceinline__ void visit_gru(const GruArgs& q, const Deal& d, int s, int tiles, int nt, Walk& wk, const Res<kH, 3>& ws) {
  if (nt == 0 || s < d.s_begin || s >= d.s_end) return;
  wk.at(d, s, false);
  const Out o{q.hrm.at(s), q.ld3, true, q.h16.at(s), q.n16, q.h16b.at(s), q.n16b};
  const int trc = __builtin_amdgcn_readlane(tiles, 0);
  ANAT(anat_arm(wk.pl);)
  tile_gru<NW, OP_F32>(q.X.at(s), 0, true, q.Wih, kH, q.xg.at(s), q.bih, q.gh.at(s), q.hprev.at(s), q.ld0, q.R, o, q.rg.at(s), q.ug.at(s), q.ng.at(s),
                       trc & 0xffff, (trc >> 16) * 16, wk.B, wk.red(), wk.pl, ws, PC());
  ANAT(anat_note(wk.anat, 4 * d.idx, wk.pl);)
}

template <int NW, class PC = PaceOff>
__device__ __forceinline__ void visit_dz(const DzArgs& q, const Deal& d, int s, int tiles, int nt, Walk& wk, const Res<kH>& ws) {
  if (nt == 0 || s < d.s_begin || s >= d.s_end) return;
  wk.at(d, s, false);
  DzIn z;
  z.mu_q = q.mu_q.at(s); z.sd_q = q.sd_q.at(s); z.mu_p = q.mu_p.at(s); z.sd_p = q.sd_p.at(s); z.eps = q.eps.at(s); z.raw_q = q.raw_q.at(s);
  z.raw_p = q.raw_p.at(s); z.muq_raw = q.muq_raw.at(s);
  z.x_sl = q.x_sl; z.c_raw = q.c_raw; z.c_fn = q.c_fn;
  z.t = q.t0 - s; z.stride = q.stride; z.residual = q.residual;
  z.fn_floor = q.fn_floor; z.beta = q.beta; z.sd_eps = q.sd_eps;
  z.has_gemm = s >= q.first_gemm;
  const Out oq{q.dqh.at(s), q.ld3, false, q.dqh16.at(s), q.n16}, op{q.dph.at(s), q.ld3, false, q.dph16.at(s), q.n16};
  const int trc = __builtin_amdgcn_readlane(tiles, 0);
  ANAT(anat_arm(wk.pl);)
  tile_dz<NW, OP_F32>(q.D.at(s), q.WT, nullptr, nullptr, true, q.add.at(s), q.ld1, false, z, oq, op, kH, q.Z, trc & 0xffff, (trc >> 16) * 16, wk.B,
                      wk.red(), wk.pl, ws, PC());
  ANAT(anat_note(wk.anat, 4 * d.idx, wk.pl);)
  // ws holds ONE product's fragments (Res<kH>), so tile_dz runs its single-operand form whatever D2 is: vrnn_static_bwd returns
  // "not applicable" for a program whose dz descriptor has a second operand (DZ_D2_16 != null).  Keep the two in step.
}

template <int NW, class PC = PaceOff>
__device__ __forceinline__ void visit_grub(const GrubArgs& q, const Deal& d, int s, int tiles, int nt, Walk& wk, const Res<kH, 2>& ws) {
  if (nt == 0 || s < d.s_begin || s >= d.s_end) return;
  wk.at(d, s, false);
  GrubIn g;
  g.D0 = q.D0.at(s); g.D1 = q.D1.at(s); g.W0 = q.W0; g.W1 = q.W1; g.g_in = q.g_in.at(s); g.g_add = q.g_add.at(s); g.ld_gadd = q.ld1;
  g.rg = q.rg.at(s); g.ug = q.ug.at(s); g.ng = q.ng.at(s); g.gh = q.gh.at(s); g.hprev = q.hprev.at(s); g.dd = q.dd.at(s); g.ldh = q.ld0;
  g.dgi = Out{q.dgi.at(s), q.ld3, false, q.dgi16.at(s), q.n16};
  g.dgh = Out{q.dgh.at(s), q.ld3, false, q.dgh16.at(s), q.n16};
  g.ga = q.ga.at(s); g.g_out = const_cast<float*>(q.g_out);
  g.has_gemm = s >= q.first_gemm; g.has_gates = s < q.end_gates; g.has_gin = s >= q.first_gin;
  const int trc = __builtin_amdgcn_readlane(tiles, 0);
  ANAT(anat_arm(wk.pl);)
  tile_grub<NW, OP_F32>(g, kH, q.R, trc & 0xffff, (trc >> 16) * 16, wk.B, wk.red(), wk.pl, ws, PC());
  ANAT(anat_note(wk.anat, 4 * d.idx, wk.pl);)
}

// ---- look-ahead arming (vrnn_static.h: the table, the three rules, the host's mirror of the arithmetic below) --------------------
// This workgroup's place among the armers of its row tile: the workgroups [cand0, cand0 + ncand) with a tile of the role's link in
// that row tile, ranked in one ballot (ncand <= kArmCandidates: arm_applies).  `tiles`, nt: this workgroup's tile_lanes of the link.
struct Armer {
  int r, k, log2n;  // row tile, rank, armers of the row tile (a power of two: arm_applies; -1: this workgroup arms nothing)
};
__device__ __forceinline__ Armer arm_rank_dev(int w, const Deal& link, int cand0, int ncand, int rt, bool xcd, int tiles, int nt, int entries) {
  if (entries == 0 || nt != 1 || w < cand0 || w >= cand0 + ncand) return Armer{0, 0, -1};
  const int lane = threadIdx.x & 63, my_r0 = __builtin_amdgcn_readlane(tiles, 0) & 0xffff;
  const TileIter it(cand0 + lane, link.wg0, link.nwg, rt, link.ct, xcd);
  const unsigned long long same = __ballot(lane < ncand && it.valid() && it.r0() == my_r0);
  const int n = (int)__popcll(same);  // (>= 1: this workgroup's own bit; a power of two: arm_applies)
  return Armer{my_r0 >> 4, (int)__popcll(same & ((1ull << (w - cand0)) - 1ull)), __builtin_ctz((unsigned)n)};
}
// store the sentinels of walk step j into this workgroup's share of its row tile (rule 1), entry e on wave e % NW, as write-through
// 16-byte stores that the wave drains before it goes on to its next tile (rule 2)
template <int NW>
__device__ __forceinline__ void arm_ahead(const ArmTable& t, int j, int rt, const Armer& a) {
  if (a.log2n < 0) return;
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const u32x4 ff = {SENTINEL, SENTINEL, SENTINEL, SENTINEL};
  for (int e = wave; e < t.n; e += NW) {
    const ArmEntry& en = t.e[e];
    if (j >= en.nslabs) continue;
    int first, count;
    arm_share(en, a.r, rt, a.k, a.log2n, &first, &count);
    const rsrc_t dst = make_rsrc(en.base + (long)j * en.step + (long)a.r * en.tile + 4L * first);
    for (int i = lane; i < count; i += 64) __builtin_amdgcn_raw_buffer_store_b128(ff, dst, 16 * i, 0, PCHAIN_STORE_AUX);
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}

// The kernel's own argument block (offset 0 of the kernarg segment) through a pointer the compiler cannot see through: every visit
// reads the fields it needs with s_load at its point of use.  Read through the by-value parameter instead, the compiler hoists every
// pointer of a role's loop into SGPRs for the whole launch and, past 106 of them, parks them in VGPR lanes (forward 514 -> 34,
// backward 797 -> 110 SGPR spills).
template <class A>
__device__ __forceinline__ const A& kargs() {
  typedef const __attribute__((address_space(4))) char kchar;
  kchar* p = (kchar*)__builtin_amdgcn_kernarg_segment_ptr();
  asm volatile("" : "+s"(p));
  return *(const A*)p;
}

// Forward program (vrnn.hip vrnn_seq_fwd_impl, own range for the hidden projection): 0 hidden projection (gentle, K = R), 1 prior
// run (K = R, H, H), 2 posterior run (the same with the x-part addend), 3 heads, 4 phi_z run of four, 5 GRU; with the decoder range
// (ndec = 4, vrnn_static.h) 6 .. 9 the decoder MLP's four gentle links behind the gentle range.
struct FwdArgs {
  LinArgs hproj;
  SeqArgs run[2];  // prior, posterior
  HeadArgs head;
  SeqArgs phi;
  GruArgs gru;
  LinArgs dec[4];
  Deal deal[kFwdDecDesc];
  int ndec;  // 0 | 3 | 4 (the last layer's Deal stays empty)
  int B, s0, S, xcd, place;  // place: vrnn_static.h Place
  Ctl ctl;
  ArmTable arm;  // look-ahead arming by the posterior half (n = 0: off)
  ANAT(unsigned long long* prof;)
};
constexpr int kFwdProducts = 4, kBwdProducts = 2;

// a workgroup of the prior (HALF 0) or posterior (1) half: its half's run of three and whatever tile of the heads, the phi_z run and
// the GRU the deal gives it, all on resident weights
template <int NW, int HALF>
__device__ __forceinline__ void fwd_half(const FwdArgs& a, int w, int rt, bool xcd, Walk& wk) {
  const int t1 = tile_lanes(w, a.deal[1 + HALF].wg0, a.deal[1 + HALF].nwg, rt, a.deal[1 + HALF].ct, xcd), n1 = tile_count(t1);
  const int t3 = tile_lanes(w, a.deal[3].wg0, a.deal[3].nwg, rt, a.deal[3].ct, xcd), n3 = tile_count(t3);
  const int t4 = tile_lanes(w, a.deal[4].wg0, a.deal[4].nwg, rt, a.deal[4].ct, xcd), n4 = tile_count(t4);
  const int t5 = tile_lanes(w, a.deal[5].wg0, a.deal[5].nwg, rt, a.deal[5].ct, xcd), n5 = tile_count(t5);
  RunRes<3, kR, kH> run;
  Res<kH, 4> head;
  RunRes<4, kH, kH> phi;
  Res<kH, 3> gru;
  load_run<NW>(run, kargs<FwdArgs>().run[HALF], t1, n1);
  load_head<NW>(head, kargs<FwdArgs>().head, t3, n3);
  load_run<NW>(phi, kargs<FwdArgs>().phi, t4, n4);
  load_gru<NW>(gru, kargs<FwdArgs>().gru, t5, n5);
  for (int s = a.s0; s < a.S; ++s) {
    visit_run<NW, 3, kR, kH, false, Paced>(kargs<FwdArgs>().run[HALF], kargs<FwdArgs>().deal[1 + HALF], s, t1, n1, wk, run);
    visit_head<NW, Paced>(kargs<FwdArgs>().head, kargs<FwdArgs>().deal[3], s, t3, n3, wk, head);
    visit_run<NW, 4, kH, kH, false, Paced>(kargs<FwdArgs>().phi, kargs<FwdArgs>().deal[4], s, t4, n4, wk, phi);
    // (the posterior half reaches its GRU tile while the prior half still walks the heads and the phi_z run: not paced)
    if constexpr (HALF == 0) visit_gru<NW, Paced>(kargs<FwdArgs>().gru, kargs<FwdArgs>().deal[5], s, t5, n5, wk, gru);
    else visit_gru<NW>(kargs<FwdArgs>().gru, kargs<FwdArgs>().deal[5], s, t5, n5, wk, gru);
  }
  ANAT(anat_end(wk.anat, kargs<FwdArgs>().prof, HALF, w == kargs<FwdArgs>().deal[1 + HALF].wg0);)
}

// a workgroup of the posterior half that arms (vrnn_static.h): the deal gives it no tile of the heads or the phi_z run, so between its
// run and its GRU tile it waits while the prior half walks those — and stores the sentinels of step s + kArmAhead in that window.
// A role of its own, not a branch of fwd_half: without the heads' and the run's fragments it has the registers for the stores,
// and the other workgroups' code stays what it was.
template <int NW>
__device__ __forceinline__ void fwd_post_arming(const FwdArgs& a, int w, int rt, bool xcd, Walk& wk) {
  const int t1 = tile_lanes(w, a.deal[2].wg0, a.deal[2].nwg, rt, a.deal[2].ct, xcd), n1 = tile_count(t1);
  const int t5 = tile_lanes(w, a.deal[5].wg0, a.deal[5].nwg, rt, a.deal[5].ct, xcd), n5 = tile_count(t5);
  const Armer armer = arm_rank_dev(w, a.deal[5], a.deal[2].wg0, a.deal[0].wg0 - a.deal[2].wg0, rt, xcd, t5, n5, a.arm.n);
  RunRes<3, kR, kH> run;
  Res<kH, 3> gru;
  load_run<NW>(run, kargs<FwdArgs>().run[1], t1, n1);
  load_gru<NW>(gru, kargs<FwdArgs>().gru, t5, n5);
  for (int s = a.s0; s < a.S; ++s) {
    visit_run<NW, 3, kR, kH, false, Paced>(kargs<FwdArgs>().run[1], kargs<FwdArgs>().deal[2], s, t1, n1, wk, run);
    arm_ahead<NW>(kargs<FwdArgs>().arm, s + kArmAhead, rt, armer);
    visit_gru<NW>(kargs<FwdArgs>().gru, kargs<FwdArgs>().deal[5], s, t5, n5, wk, gru);  // (not paced: see fwd_half)
  }
  ANAT(anat_end(wk.anat, kargs<FwdArgs>().prof, 1, w == kargs<FwdArgs>().deal[2].wg0);)
}

// a workgroup of the decoder range: a follower of the chain.  Step t's decoder row needs [phi_t | h_t] only, so nothing the critical
// roles poll is written here.  The first layer's two column ranges and the second layer run on resident weights (one tile each: the
// converter checks it), the last layer's up to kMaxTiles tiles read theirs per tile.
constexpr int kDecFlags = DF_RELU | DF_GENTLE | DF_CANARY;
template <int NW>
__device__ __forceinline__ void fwd_dec(const FwdArgs& a, int w, int rt, bool xcd, Walk& wk) {
  const int t6 = tile_lanes(w, a.deal[6].wg0, a.deal[6].nwg, rt, a.deal[6].ct, xcd), n6 = tile_count(t6);
  const int t7 = tile_lanes(w, a.deal[7].wg0, a.deal[7].nwg, rt, a.deal[7].ct, xcd), n7 = tile_count(t7);
  const int t8 = tile_lanes(w, a.deal[8].wg0, a.deal[8].nwg, rt, a.deal[8].ct, xcd), n8 = tile_count(t8);
  const int t9 = tile_lanes(w, a.deal[9].wg0, a.deal[9].nwg, rt, a.deal[9].ct, xcd), n9 = tile_count(t9);
  if ((n6 | n7 | n8 | n9) == 0) return;
  Res<kR> w1h;
  Res<kH> w1p, w2;
  load_lin<NW, kR>(w1h, kargs<FwdArgs>().dec[0].W, kargs<FwdArgs>().dec[0].w_width, t6, n6);
  load_lin<NW, kH>(w1p, kargs<FwdArgs>().dec[1].W, kargs<FwdArgs>().dec[1].w_width, t7, n7);
  load_lin<NW, kH>(w2, kargs<FwdArgs>().dec[2].W, kH, t8, n8);
  for (int s = a.s0; s < a.S; ++s) {
    visit_lin<NW, kR, DF_RM_SC1 | DF_GENTLE | DF_CANARY>(kargs<FwdArgs>().dec[0], kargs<FwdArgs>().deal[6], s, t6, n6, wk, w1h);
    visit_lin<NW, kH, DF_ADD_POLLED | kDecFlags>(kargs<FwdArgs>().dec[1], kargs<FwdArgs>().deal[7], s, t7, n7, wk, w1p);
    visit_lin<NW, kH, kDecFlags>(kargs<FwdArgs>().dec[2], kargs<FwdArgs>().deal[8], s, t8, n8, wk, w2);
    visit_lin<NW, kH, kDecFlags, PaceOff, true>(kargs<FwdArgs>().dec[3], kargs<FwdArgs>().deal[9], s, t9, n9, wk, WMem());
  }
}

template <int NW>
__global__ __launch_bounds__(NW * 64, 1) void vrnn_static_fwd_kernel(FwdArgs a) {
  extern __shared__ __attribute__((aligned(16))) float lds_red[];
  const int w = placed_wg(a.place), rt = (a.B + 15) / 16;
  const bool xcd = a.place == kPlaceProgram && a.xcd != 0;
  Walk wk{lds_red, lds_red + kFwdProducts * NW * 256, 0, a.B, Poll{a.ctl, 0u, false, 1}};
  ANAT(__shared__ unsigned anat[kAnatSlots * 8]; anat_begin(anat); wk.anat = anat;)
  // roles, picked once: the decoder range (if any) follows the chain, the gentle range runs the hidden projection alone, the others
  // are a half's workgroups (fwd_half)
  if (a.ndec != 0 && w >= a.deal[6].wg0) {
    fwd_dec<NW>(a, w, rt, xcd, wk);
    return;
  }
  if (w >= a.deal[0].wg0) {
    const int t0 = tile_lanes(w, a.deal[0].wg0, a.deal[0].nwg, rt, a.deal[0].ct, xcd), n0 = tile_count(t0);
    if (n0 == 0) return;
    for (int s = a.s0; s < a.S; ++s) visit_lin<NW, kR, DF_RM_SC1 | DF_GENTLE | DF_CANARY>(kargs<FwdArgs>().hproj, kargs<FwdArgs>().deal[0], s, t0, n0, wk, WMem());
    return;
  }
  if (w < a.deal[2].wg0) fwd_half<NW, 0>(a, w, rt, xcd, wk);
  else if (a.arm.n != 0) fwd_post_arming<NW>(a, w, rt, xcd, wk);  // (an armed launch: no workgroup of this half has a heads or phi_z tile, arm_applies)
  else fwd_half<NW, 1>(a, w, rt, xcd, wk);
}

// The d_enc follower's two links (vrnn_static.h benc) in a compact form — a launch's arguments are 4 KB at most and BwdArgs is
// close to it: only what an empty LinArgs and the rest of BwdArgs do not say already.  The links' operands are the GRU backward's
// DGI16 and the posterior run's last output DQ16[0], a walk step back; their range is the posterior run's (the converter checks both).
struct EncArgs {
  float *ep, *out;       // benc[0]: EP = DGI16 W0;  benc[1]: out = DQ16[0] W1 + EP  (at walk step 0: a slab behind the chain's)
  const float *W0, *W1;
  int stride;            // of both, per walk step (floats)
};

// Backward program (vrnn.hip vrnn_seq_bwd_impl, split3 form): 0 GRU backward (steps 0 .. T'), 1 .. 3 the K = 3R dphi product as
// three K = R partial-sum links (prior half | posterior half | spare range), 4 GB (gentle, K = 3R), 5 the summing link, 6 phi_z
// run of two, 7 dz, 8 prior run (K = 2Z, H, H), 9 posterior run; with the decoder leader (nbdec = 3, vrnn_static.h) 10 .. 12 the
// decoder MLP's three data-gradient links on the spare range; with the d_enc follower (nenc = 2) the program's last two descriptors
// are its links on the posterior half.
struct BwdArgs {
  GrubArgs grub;
  LinArgs part[3], gb, sum;
  SeqArgs phi;
  DzArgs dz;
  SeqArgs run[2];
  LinArgs bdec[3];
  Deal deal[kBwdDecDesc];
  EncArgs enc;
  int nenc;   // 0 | 2: the d_enc follower on the posterior half
  int nbdec;  // 0 | 3: the decoder leader on the spare range
  int bdec_k, gb_ldadd2;  // K of bdec[0] (the decoder's output width); GB's second addend, the h part of the decoder's gradient
  SPtr gb_add2;
  int B, s0, S, xcd, place;  // place: vrnn_static.h Place
  Ctl ctl;
  ArmTable arm;  // look-ahead arming by the spare range (n = 0: off)
  ANAT(unsigned long long* prof;)
};

static_assert(sizeof(BwdArgs) <= 4096 && sizeof(FwdArgs) <= 4096, "kernel argument size");
__device__ __forceinline__ SPtr lagged(const SPtr& p) { return SPtr{p.base - (long)kBencLag * p.stride, p.stride}; }  // walk step s -> the slab of step s - kBencLag
__device__ __forceinline__ LinArgs enc_lin(const BwdArgs& a, int k) {
  LinArgs q{};
  q.a = lagged(k == 0 ? a.grub.dgi16 : a.run[1].o16[2]);
  q.orm = SPtr{k == 0 ? a.enc.ep : a.enc.out, a.enc.stride};
  if (k == 1) { q.add = SPtr{a.enc.ep, a.enc.stride}; q.ld1 = kH; }
  q.W = k == 0 ? a.enc.W0 : a.enc.W1;
  q.ld3 = kH;  // (X = H: the converter checks it)
  return q;
}
__device__ __forceinline__ Deal enc_deal(const BwdArgs& a, int k) {
  return Deal{a.deal[9].wg0, a.deal[9].nwg, kH / 16, kBencLag, a.S, (a.nbdec != 0 ? kBwdDecDesc : kBwdDesc) + k};
}

// a workgroup of the prior (HALF 0) or posterior (1) half: its half's partial sum and run of three and whatever tile of the GRU
// backward, the summing link, the phi_z run and dz the deal gives it, all on resident weights
template <int NW, int HALF>
__device__ __forceinline__ void bwd_half(const BwdArgs& a, int w, int rt, bool xcd, Walk& wk) {
  const int t0 = tile_lanes(w, a.deal[0].wg0, a.deal[0].nwg, rt, a.deal[0].ct, xcd), n0 = tile_count(t0);
  const int t1 = tile_lanes(w, a.deal[1 + HALF].wg0, a.deal[1 + HALF].nwg, rt, a.deal[1 + HALF].ct, xcd), n1 = tile_count(t1);
  const int t5 = tile_lanes(w, a.deal[5].wg0, a.deal[5].nwg, rt, a.deal[5].ct, xcd), n5 = tile_count(t5);
  const int t6 = tile_lanes(w, a.deal[6].wg0, a.deal[6].nwg, rt, a.deal[6].ct, xcd), n6 = tile_count(t6);
  const int t7 = tile_lanes(w, a.deal[7].wg0, a.deal[7].nwg, rt, a.deal[7].ct, xcd), n7 = tile_count(t7);
  const int t8 = tile_lanes(w, a.deal[8 + HALF].wg0, a.deal[8 + HALF].nwg, rt, a.deal[8 + HALF].ct, xcd), n8 = tile_count(t8);
  Res<kH, 2> grub;
  Res<kR> part;
  Res<kH> sum, dz;
  RunRes<2, kH, kH> phi;
  RunRes<3, 2 * kH, kH> run;
  load_grub<NW>(grub, kargs<BwdArgs>().grub, t0, n0);
  load_lin<NW, kR>(part, kargs<BwdArgs>().part[HALF].W, kargs<BwdArgs>().part[HALF].w_width, t1, n1);
  load_lin<NW, kH>(sum, kargs<BwdArgs>().sum.W, kH, t5, n5);
  load_run<NW>(phi, kargs<BwdArgs>().phi, t6, n6);
  load_lin<NW, kH>(dz, kargs<BwdArgs>().dz.WT, kH, t7, n7);
  load_run<NW>(run, kargs<BwdArgs>().run[HALF], t8, n8);
  for (int s = a.s0; s < a.S; ++s) {
    visit_grub<NW, Paced>(kargs<BwdArgs>().grub, kargs<BwdArgs>().deal[0], s, t0, n0, wk, grub);
    visit_lin<NW, kR, 0, Paced>(kargs<BwdArgs>().part[HALF], kargs<BwdArgs>().deal[1 + HALF], s, t1, n1, wk, part);
    visit_lin<NW, kH, DF_A_SUM3, Paced>(kargs<BwdArgs>().sum, kargs<BwdArgs>().deal[5], s, t5, n5, wk, sum);
    visit_run<NW, 2, kH, kH, true, Paced>(kargs<BwdArgs>().phi, kargs<BwdArgs>().deal[6], s, t6, n6, wk, phi);
    visit_dz<NW, Paced>(kargs<BwdArgs>().dz, kargs<BwdArgs>().deal[7], s, t7, n7, wk, dz);
    // (the posterior half reaches its run while the prior half still walks the summing link, the phi_z run and dz: not paced)
    if constexpr (HALF == 0) visit_run<NW, 3, 2 * kH, kH, true, Paced>(kargs<BwdArgs>().run[HALF], kargs<BwdArgs>().deal[8 + HALF], s, t8, n8, wk, run);
    else visit_run<NW, 3, 2 * kH, kH, true>(kargs<BwdArgs>().run[HALF], kargs<BwdArgs>().deal[8 + HALF], s, t8, n8, wk, run);
  }
  ANAT(anat_end(wk.anat, kargs<BwdArgs>().prof, 2 + HALF, w == kargs<BwdArgs>().deal[1 + HALF].wg0);)
}

// a workgroup of the spare range with the decoder leader (vrnn_static.h): per walk step its partial-sum tile, which is on the chain
// and now takes the phi part of the decoder's gradient as its addend (stored kBdecAhead steps ago: requested under the operand wait),
// then the decoder's three data-gradient links of the time step kBdecAhead walk steps ahead (their descriptors' pointers start
// there: the interpreter walks the same descriptors in the same order), then the sentinels of step s + kArmAhead.
// (the flags of GB, of the third partial sum under the leader, and of the leader's links: the converter checks the program against them)
constexpr int kGbFlags = DF_ADD_POLLED | DF_RM_SC1 | DF_GENTLE | DF_CANARY;
constexpr int kPartLeadFlags = DF_ADD_POLLED | DF_ADD_EARLY;
constexpr int kBdec0Flags = DF_A_PLAIN | DF_GENTLE, kBdec1Flags = DF_GENTLE | DF_CANARY, kBdec2Flags = DF_RM_SC1 | DF_GENTLE | DF_CANARY;
template <int NW>
__device__ __forceinline__ void bwd_spare_leader(const BwdArgs& a, int w, int rt, bool xcd, Walk& wk) {
  const int t = tile_lanes(w, a.deal[3].wg0, a.deal[3].nwg, rt, a.deal[3].ct, xcd), n = tile_count(t);
  const int t10 = tile_lanes(w, a.deal[10].wg0, a.deal[10].nwg, rt, a.deal[10].ct, xcd), n10 = tile_count(t10);
  const int t11 = tile_lanes(w, a.deal[11].wg0, a.deal[11].nwg, rt, a.deal[11].ct, xcd), n11 = tile_count(t11);
  const int t12 = tile_lanes(w, a.deal[12].wg0, a.deal[12].nwg, rt, a.deal[12].ct, xcd), n12 = tile_count(t12);
  if ((n | n10 | n11 | n12) == 0) return;
  Res<kR> part;
  Res<kH> w2;
  load_lin<NW, kR>(part, kargs<BwdArgs>().part[2].W, kargs<BwdArgs>().part[2].w_width, t, n);
  load_lin<NW, kH>(w2, kargs<BwdArgs>().bdec[1].W, kH, t11, n11);
  const Armer armer = arm_rank_dev(w, a.deal[3], a.deal[3].wg0, a.deal[3].nwg, rt, xcd, t, n, a.arm.n);
#ifdef PCHAIN_TPROF
  unsigned long long lead = 0, arming = 0;
  const unsigned long long tb = wall_clock64();
#endif
  for (int s = a.s0; s < a.S; ++s) {
    visit_lin<NW, kR, kPartLeadFlags>(kargs<BwdArgs>().part[2], kargs<BwdArgs>().deal[3], s, t, n, wk, part);
    ANAT(const unsigned long long t0 = wall_clock64();)
    visit_lin<NW, 0, kBdec0Flags>(kargs<BwdArgs>().bdec[0], kargs<BwdArgs>().deal[10], s, t10, n10, wk, WMem(), kargs<BwdArgs>().bdec_k);
    visit_lin<NW, kH, kBdec1Flags>(kargs<BwdArgs>().bdec[1], kargs<BwdArgs>().deal[11], s, t11, n11, wk, w2);
    visit_lin<NW, kH, kBdec2Flags, PaceOff, true>(kargs<BwdArgs>().bdec[2], kargs<BwdArgs>().deal[12], s, t12, n12, wk, WMem());
    ANAT(const unsigned long long t1 = wall_clock64();)
    arm_ahead<NW>(kargs<BwdArgs>().arm, s + kArmAhead, rt, armer);
    ANAT(const unsigned long long t2 = wall_clock64(); lead += t1 - t0; arming += t2 - t1;)
  }
#ifdef PCHAIN_TPROF
  // slot 13 of the role's table: {walk steps, -, ticks in the leader's links, ticks in the arming stores}; slot 14: {1, -, ticks of the whole loop, -}
  const unsigned long long whole = wall_clock64() - tb;
  if (threadIdx.x == 0) {
    unsigned* q = wk.anat + 13 * 2 * 4;
    q[0] = (unsigned)(a.S - a.s0); q[2] = (unsigned)lead; q[3] = (unsigned)arming;
    q[8] = 1u; q[10] = (unsigned)whole;
  }
  anat_end(wk.anat, kargs<BwdArgs>().prof, 4, w == kargs<BwdArgs>().deal[3].wg0);
#endif
}

// a workgroup of the posterior half with the d_enc follower (vrnn_static.h): the deal gives it no tile of the summing link, the phi_z
// run or dz, so between its partial-sum tile and its run it waits while the prior half walks those — and computes its tile of the
// gradient wrt the encoding of the previous walk step's time step in that window: EP = DGI W_ih[:, :X] (weights read per tile), then
// d_enc = DQ0 Wq0[:, R:] + EP on resident weights, the addend polled where its own threads stored it.  Both operands were published
// a walk step ago, so neither link waits.  A role of its own, as fwd_post_arming: without the fragments of the links it never runs
// it has the registers, and the other workgroups' code stays what it was.
constexpr int kBenc0Flags = DF_RM_SC1 | DF_GENTLE | DF_CANARY, kBenc1Flags = DF_ADD_POLLED | DF_GENTLE | DF_CANARY;
template <int NW>
__device__ __forceinline__ void bwd_post_follower(const BwdArgs& a, int w, int rt, bool xcd, Walk& wk) {
  const int t0 = tile_lanes(w, a.deal[0].wg0, a.deal[0].nwg, rt, a.deal[0].ct, xcd), n0 = tile_count(t0);
  const int t1 = tile_lanes(w, a.deal[2].wg0, a.deal[2].nwg, rt, a.deal[2].ct, xcd), n1 = tile_count(t1);
  const int t8 = tile_lanes(w, a.deal[9].wg0, a.deal[9].nwg, rt, a.deal[9].ct, xcd), n8 = tile_count(t8);
  const int te = tile_lanes(w, a.deal[9].wg0, a.deal[9].nwg, rt, kH / 16, xcd), ne = tile_count(te);
  Res<kH, 2> grub;
  Res<kR> part;
  RunRes<3, 2 * kH, kH> run;
  Res<kH> wq;
  load_grub<NW>(grub, kargs<BwdArgs>().grub, t0, n0);
  load_lin<NW, kR>(part, kargs<BwdArgs>().part[1].W, kargs<BwdArgs>().part[1].w_width, t1, n1);
  load_run<NW>(run, kargs<BwdArgs>().run[1], t8, n8);
  load_lin<NW, kH>(wq, kargs<BwdArgs>().enc.W1, kH, te, ne);
#ifdef PCHAIN_TPROF
  unsigned long long follow = 0;
  const unsigned long long tb = wall_clock64();
#endif
  for (int s = a.s0; s < a.S; ++s) {
    visit_grub<NW, Paced>(kargs<BwdArgs>().grub, kargs<BwdArgs>().deal[0], s, t0, n0, wk, grub);
    visit_lin<NW, kR, 0, Paced>(kargs<BwdArgs>().part[1], kargs<BwdArgs>().deal[2], s, t1, n1, wk, part);
    ANAT(const unsigned long long f0 = wall_clock64();)
    visit_lin<NW, 3 * kR, kBenc0Flags>(enc_lin(kargs<BwdArgs>(), 0), enc_deal(kargs<BwdArgs>(), 0), s, te, ne, wk, WMem());
    visit_lin<NW, kH, kBenc1Flags>(enc_lin(kargs<BwdArgs>(), 1), enc_deal(kargs<BwdArgs>(), 1), s, te, ne, wk, wq);
    ANAT(follow += wall_clock64() - f0;)
    visit_run<NW, 3, 2 * kH, kH, true>(kargs<BwdArgs>().run[1], kargs<BwdArgs>().deal[9], s, t8, n8, wk, run);  // (not paced: see bwd_half)
  }
#ifdef PCHAIN_TPROF
  // slot 13 of the role's table: {walk steps, -, ticks in the follower's links, -}; slot 14: {1, -, ticks of the whole loop, -}
  const unsigned long long whole = wall_clock64() - tb;
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned* q = wk.anat + 13 * 2 * 4;
    q[0] = (unsigned)(a.S - a.s0); q[2] = (unsigned)follow;
    q[8] = 1u; q[10] = (unsigned)whole;
  }
  anat_end(wk.anat, kargs<BwdArgs>().prof, 3, w == kargs<BwdArgs>().deal[2].wg0);
#endif
}

// ENC: the launch runs the d_enc follower (a.nenc != 0).  An instantiation of its own, so that the kernel of every other launch is
// the code it was: with the role as a run-time branch of one kernel the unfolded step measured 0.05 ms slower than before it existed.
template <int NW, bool ENC = false>
__global__ __launch_bounds__(NW * 64, 1) void vrnn_static_bwd_kernel(BwdArgs a) {
  extern __shared__ __attribute__((aligned(16))) float lds_red[];
  const int w = placed_wg(a.place), rt = (a.B + 15) / 16;
  const bool xcd = a.place == kPlaceProgram && a.xcd != 0;
  Walk wk{lds_red, lds_red + kBwdProducts * NW * 256, 0, a.B, Poll{a.ctl, 0u, false, 1}};
  ANAT(__shared__ unsigned anat[kAnatSlots * 8]; anat_begin(anat); wk.anat = anat;)
  if (a.nbdec != 0 && w >= a.deal[3].wg0) {
    bwd_spare_leader<NW>(a, w, rt, xcd, wk);
    return;
  }
  if (w >= a.deal[3].wg0) {  // spare range: the third partial sum alone
    const int t = tile_lanes(w, a.deal[3].wg0, a.deal[3].nwg, rt, a.deal[3].ct, xcd), n = tile_count(t);
    if (n == 0) return;
    Res<kR> part;
    load_lin<NW, kR>(part, kargs<BwdArgs>().part[2].W, kargs<BwdArgs>().part[2].w_width, t, n);
    const Armer armer = arm_rank_dev(w, a.deal[3], a.deal[3].wg0, a.deal[3].nwg, rt, xcd, t, n, a.arm.n);
    for (int s = a.s0; s < a.S; ++s) {
      visit_lin<NW, kR, 0>(kargs<BwdArgs>().part[2], kargs<BwdArgs>().deal[3], s, t, n, wk, part);
      arm_ahead<NW>(kargs<BwdArgs>().arm, s + kArmAhead, rt, armer);
    }
    ANAT(anat_end(wk.anat, kargs<BwdArgs>().prof, 4, w == kargs<BwdArgs>().deal[3].wg0);)
    return;
  }
  if (w >= a.deal[4].wg0) {  // gentle range: GB alone
    const int t = tile_lanes(w, a.deal[4].wg0, a.deal[4].nwg, rt, a.deal[4].ct, xcd), n = tile_count(t);
    if (n == 0) return;
    if (a.nbdec != 0) {  // (with the leader: the h part of the decoder's gradient is GB's second polled addend)
      for (int s = a.s0; s < a.S; ++s)
        visit_lin<NW, 3 * kR, kGbFlags | DF_ADD2_POLLED>(kargs<BwdArgs>().gb, kargs<BwdArgs>().deal[4], s, t, n, wk, WMem(), 0, kargs<BwdArgs>().gb_add2,
                                                         kargs<BwdArgs>().gb_ldadd2);
      return;
    }
    for (int s = a.s0; s < a.S; ++s)
      visit_lin<NW, 3 * kR, kGbFlags>(kargs<BwdArgs>().gb, kargs<BwdArgs>().deal[4], s, t, n, wk, WMem());
    return;
  }
  if (w < a.deal[2].wg0) bwd_half<NW, 0>(a, w, rt, xcd, wk);
  else if constexpr (ENC) bwd_post_follower<NW>(a, w, rt, xcd, wk);  // (no workgroup of this half has a tile of the summing link, the phi_z run or dz: the converter)
  else bwd_half<NW, 1>(a, w, rt, xcd, wk);
}

// the placement the static launches ask for (vrnn_static.h Place): bits 32 (plain) and 64 (local) of pchain_tune; neither: the
// program's TileIter mode.  Where the local placement does not apply the launch falls back to the plain one if bit 32 is set too,
// else to the program's mode: plain alone measured slower than that at B = 32 and 64.
int static_place_fallback() { return (pchain_tune() & 32) ? kPlacePlain : kPlaceProgram; }
int static_place_wanted() { return (pchain_tune() & 64) ? kPlaceLocal : static_place_fallback(); }

// the program's pointer k of descriptor d as a stepped pointer
bool int_strides(const Program& p) {  // SPtr keeps 32-bit strides
  for (long v : p.stride)
    if (v < -2147483647L || v > 2147483647L) return false;
  return true;
}
SPtr sptr(const Program& p, const Desc& d, int k) { return SPtr{const_cast<float*>(d.p[k]), (int)p.stride[d.sidx[k]]}; }

// every workgroup of `grid` resident at once (one 16-wave workgroup per CU with `lds` bytes of dynamic LDS), as pchain_run
// checks it; the dynamic-LDS limit is raised once per process and device.  slot: 0 forward, 1 backward, 2 the probe's chain,
// 3 the backward with the d_enc follower
template <class Kern>
int static_go(Kern kernel, int slot, int grid, size_t lds, const char* what) {
  static std::mutex mu;
  static int attr_dev[4] = {-1, -1, -1, -1}, occ[4] = {0, 0, 0, 0};
  int dev = 0, cus = 0;
  BLVM_HIP(hipGetDevice(&dev));
  BLVM_HIP(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
  {
    std::lock_guard<std::mutex> lock(mu);
    if (attr_dev[slot] != dev) {
      BLVM_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
      BLVM_HIP(hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ[slot], kernel, 1024, lds));
      attr_dev[slot] = dev;
    }
    BLVM_REQUIRE((long)occ[slot] * cus >= grid, "%s: %d workgroups are not co-resident (%d per CU x %d CUs)", what, grid, occ[slot], cus);
  }
  return BLVM_OK;
}

// 1: the program is not the linear chain the static kernel was compiled for (resident: or it deals a workgroup more than one tile)
// pace (resident only): the first-poll delays of early / epi s_sleep units instead of the plain poll loop
int static_lin_chain_launch(const Program& p, hipStream_t stream, bool resident, bool pace = false, int early = 0, int epi = 0) {
  if (p.ndesc != 1 || p.ot != OP_F32 || p.rt_group != 1 || !int_strides(p)) return 1;
  const Desc& d = p.d[0];
  if (d.kind != K_LIN || d.flags != DF_RELU || d.f[LIN_F_SLOPE] != 0.f || (d.K != 256 && d.K != 512) || d.s_begin != 0 || d.s_end != p.S) return 1;
  if (d.ld[LIN_LD_A] != 0 || d.i[LIN_I_W_WIDTH] != 0 || d.p[LIN_ADD] || d.p[LIN_GATE] || d.p[LIN_O16B] || d.p[LIN_A2] || d.p[LIN_A3] || d.n16[N16_OUTB] != 0)
    return 1;
  const int rt = (p.B + 15) / 16;
  // placement (vrnn_static.h): the chain's one range [0, 64) or [0, 128) on four row tiles is one place_wg keeps — row tile r on
  // XCD r (64 tiles; the blocks of XCDs 4 .. 7 get none) or on XCDs r and r + 4 (128 tiles, as plain).  The resident form only: the
  // fetch form reads its weights through L2 every link, which is what the program's mode places for.
  int place = resident ? static_place_wanted() : kPlaceProgram;
  if (place == kPlaceLocal && !(rt == 4 && d.wg0 == 0 && (d.nwg == 64 || d.nwg == kPlaceSpan) && device_cus() >= kPlaceSpan)) place = static_place_fallback();
  const bool xcd = place == kPlaceProgram && p.xcd != 0;
  if (d.nwg <= 0 || (p.xcd && d.nwg % 8 != 0) || tiles_per_workgroup(rt, d.ct, d.nwg, xcd) > (resident ? 1 : kMaxTiles)) return 1;
  LinChainArgs a{sptr(p, d, LIN_A), sptr(p, d, LIN_ORM), sptr(p, d, LIN_O16), d.p[LIN_W], d.p[LIN_BIAS], d.ld[LD_OUT], d.n16[N16_OUT], p.B, p.s_first, p.S,
                 d.wg0, d.nwg, d.ct, p.xcd, place, p.ctl, early, epi};
  ANAT(a.prof = pchain_profile_buffer();)
  const int grid = place == kPlaceLocal ? kPlaceSpan : d.wg0 + d.nwg;
  auto go = [&](auto kernel) -> int {
    BLVM_TRY(static_go(kernel, 2, grid, 0, "static_lin_chain"));
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(1024), 0, stream, a);
    BLVM_CHECK_LAUNCH("static_lin_chain");
    return BLVM_OK;
  };
  if (resident && pace) return d.K == 256 ? go(&static_lin_chain_kernel<16, 256, true, PaceRt>) : go(&static_lin_chain_kernel<16, 512, true, PaceRt>);
  if (resident) return d.K == 256 ? go(&static_lin_chain_kernel<16, 256, true>) : go(&static_lin_chain_kernel<16, 512, true>);
  return d.K == 256 ? go(&static_lin_chain_kernel<16, 256, false>) : go(&static_lin_chain_kernel<16, 512, false>);
}

// the selector between the static walk and the interpreter for the VRNN programs (blvm_pchain_static)
int g_static = 1;
long g_static_launches = 0;  // VRNN programs launched on the static kernels (blvm_pchain_static(-2))
long g_armed_launches = 0;   // ... of which armed their polled slabs themselves (blvm_pchain_static(-3))
bool pchain_static_on() { return g_static != 0; }

// ---- host: the interpreter's program -> the static kernels' arguments -------------------------------------------------------
SPtr sp(const Program& p, const Desc& d, int k) { return SPtr{const_cast<float*>(d.p[k]), d.p[k] ? (int)p.stride[d.sidx[k]] : 0}; }
Deal deal_of(const Desc& d, int idx) { return Deal{d.wg0, d.nwg, d.ct, d.s_begin, d.s_end, idx}; }
bool within(const Desc& d, int lo, int hi) { return d.wg0 >= lo && d.wg0 + d.nwg <= hi; }
bool few_tiles(const Program& p, const Desc& d, bool xcd) {  // at most kMaxTiles tiles of the link per workgroup in the launch's TileIter mode
  if (d.nwg <= 0 || (p.xcd && d.nwg % 8 != 0)) return false;
  return tiles_per_workgroup((p.B + 15) / 16, d.ct, d.nwg, xcd) <= kMaxTiles;
}
bool shaped(const Desc& d, int kind, int flags, int K) { return d.kind == kind && d.flags == flags && d.K == K; }
bool run(const Desc& d, int n, int K0) { return d.i[LINSEQ_I_N] == n && d.i[LINSEQ_I_K0] == K0; }  // a K_LINSEQ of n links, first link's K0

LinArgs lin_args(const Program& p, const Desc& d) {
  return LinArgs{sp(p, d, LIN_A), sp(p, d, LIN_A2), sp(p, d, LIN_A3), sp(p, d, LIN_ADD), sp(p, d, LIN_GATE), sp(p, d, LIN_ORM), sp(p, d, LIN_O16),
                 sp(p, d, LIN_O16B), d.p[LIN_W], d.p[LIN_BIAS], d.ld[LIN_LD_A], d.ld[LIN_LD_ADD], d.ld[LIN_LD_GATE], d.ld[LD_OUT], d.n16[N16_OUT], d.n16[N16_OUTB],
                 d.i[LIN_I_W_WIDTH], d.f[LIN_F_SLOPE]};
}
SeqArgs seq_args(const Program& p, const Desc& d) {
  SeqArgs q{};
  q.a0 = sp(p, d, LINSEQ_A0); q.add0 = sp(p, d, LINSEQ_ADD0);
  for (int i = 0; i < d.i[LINSEQ_I_N]; ++i) {
    q.W[i] = d.p[LINSEQ_W + i]; q.aux[i] = sp(p, d, LINSEQ_AUX + i); q.orm[i] = sp(p, d, LINSEQ_ORM + i); q.o16[i] = sp(p, d, LINSEQ_O16 + i);
    q.ld[i] = d.ld[LINSEQ_LD_ORM + i];
  }
  q.ldadd0 = d.i[LINSEQ_I_LD_ADD0]; q.ldgate = d.i[LINSEQ_I_LD_GATE]; q.n16 = d.n16[N16_OUT]; q.slope = d.f[LINSEQ_F_SLOPE];
  return q;
}

// ---- host: who stores the sentinels (vrnn_static.h) ----------------------------------------------------------------------------
// walk steps [0, kArmAhead) of every buffer of the table, in one launch: block (x, e) strides over the 16-byte words of entry e
__global__ __launch_bounds__(256) void arm_prefix_kernel(ArmTable t, int rt) {
  const ArmEntry& en = t.e[blockIdx.y];
  const uint4 ff = make_uint4(SENTINEL, SENTINEL, SENTINEL, SENTINEL);
  const int slabs = en.nslabs < kArmAhead ? en.nslabs : kArmAhead;
  for (int j = 0; j < slabs; ++j)
    for (int r = 0; r < rt; ++r) {
      uint4* const dst = reinterpret_cast<uint4*>(en.base + (long)j * en.step + (long)r * en.tile);
      const int n4 = r == rt - 1 ? en.n4_last : en.n4;
      for (int i = blockIdx.x * 256 + threadIdx.x; i < n4; i += gridDim.x * 256) dst[i] = ff;
    }
}
int full_fill(const ArmPlan& plan, hipStream_t stream) {
  for (int i = 0; i < plan.nfull; ++i) BLVM_HIP(pchain_fill_sentinel(plan.full[i].p, plan.full[i].bytes, stream));
  return BLVM_OK;
}
// An armed launch (bit 128 of pchain_tune clear and arm_applies: rule 3): *arm = the table, and the host fills only the steps in
// front of the first armed one.  Any other launch: *arm stays empty and the host fills everything the launch polls.
int arm_or_fill(const Program& p, const ArmPlan& plan, int link, std::initializer_list<int> idle, int cand0, int ncand, bool xcd, hipStream_t stream,
                ArmTable* arm) {
  arm->n = 0;
  if ((pchain_tune() & 128) != 0 || !arm_applies(p, plan.tab, link, idle, cand0, ncand, xcd)) return full_fill(plan, stream);
  *arm = plan.tab;
  hipLaunchKernelGGL(arm_prefix_kernel, dim3(8, plan.tab.n), dim3(256), 0, stream, plan.tab, (p.B + 15) / 16);
  BLVM_CHECK_LAUNCH("arm_prefix");
  return BLVM_OK;
}

// 1: not the shape the static kernels were compiled for (vrnn_launch runs the interpreter).  *place: the launch's placement
// (prior, post: the descriptors of the two halves' runs); every count of tiles is taken in the TileIter mode that placement deals with
int vrnn_static_check(const Program& p, int ndesc, int products, int prior, int post, int* place) {
  if (!pchain_static_on() || p.ndesc != ndesc || p.ot != OP_F32 || p.rt_group != 1 || p.s_first != 0 || p.B > 64) return 1;
  if (p.lds_products != products || !int_strides(p)) return 1;  // (the kernels' reduction scratch is sized for `products`)
  *place = place_for(static_place_wanted(), static_place_fallback(), p, prior, post, grid_of(p));
  for (int i = 0; i < p.ndesc; ++i)
    if (!few_tiles(p, p.d[i], place_xcd(*place, p))) return 1;
  return 0;
}

int vrnn_static_fwd(const Program& p, hipStream_t stream, const ArmPlan& plan, const std::function<int()>& pre) {
  int place = kPlaceProgram;
  const bool dec = p.ndesc == kFwdDecDesc || p.ndesc == kFwdDecDesc - 1;  // with the decoder range (all three layers | the first two)
  if (vrnn_static_check(p, dec ? p.ndesc : kFwdDesc, kFwdProducts, 1, 2, &place)) return 1;
  const Desc* d = p.d;
  const int S = p.S;
  for (int i = 0; i < p.ndesc; ++i)
    if (d[i].s_begin != 0 || d[i].s_end != S) return 1;
  if (!shaped(d[0], K_LIN, DF_RM_SC1 | DF_GENTLE | DF_CANARY, kR) || !shaped(d[1], K_LINSEQ, DF_RELU, kH) || !shaped(d[2], K_LINSEQ, DF_RELU, kH) ||
      !shaped(d[3], K_HEAD, 0, kH) || !shaped(d[4], K_LINSEQ, DF_RELU, kH) || !shaped(d[5], K_GRU, 0, kH))
    return 1;
  if (!run(d[1], 3, kR) || !run(d[2], 3, kR) || !run(d[4], 4, 0)) return 1;
  if (!one_tile_each(p, kFwdResident, place_xcd(place, p))) return 1;
  // roles: prior half [0, d1 end) | posterior half [d2.wg0, d0.wg0) | gentle range [d0.wg0, ...): nothing else there
  const int half = d[2].wg0, gentle = d[0].wg0;
  if (d[1].wg0 != 0 || !within(d[1], 0, half) || !within(d[2], half, gentle) || d[0].nwg <= 0) return 1;
  if (dec && !within(d[0], gentle, d[6].wg0)) return 1;
  for (int i = 3; i < 6; ++i)
    if (!within(d[i], 0, gentle)) return 1;
  if (dec) {
    // the decoder's links: plain single-operand K_LIN, the first layer as the two K-ranges of rows kH + kR wide, all from the first
    // workgroup behind the gentle range, the resident three on one tile per workgroup
    const int from = gentle + d[0].nwg;
    if (!shaped(d[6], K_LIN, DF_RM_SC1 | DF_GENTLE | DF_CANARY, kR) || !shaped(d[7], K_LIN, DF_ADD_POLLED | kDecFlags, kH) ||
        !shaped(d[8], K_LIN, kDecFlags, kH) || (p.ndesc == kFwdDecDesc && !shaped(d[9], K_LIN, kDecFlags, kH)))
      return 1;
    for (int i = 6; i < p.ndesc; ++i) {
      if (d[i].wg0 != from || d[i].ld[LIN_LD_A] != 0 || d[i].p[LIN_A2] || d[i].p[LIN_A3] || d[i].p[LIN_O16B] || d[i].p[LIN_GATE]) return 1;
      if (d[i].i[LIN_I_W_WIDTH] != (i < 8 ? kH + kR : 0)) return 1;
    }
    if (!one_tile_each(p, kFwdDecResident, place_xcd(place, p))) return 1;
  }
  FwdArgs a{};
  a.hproj = lin_args(p, d[0]);
  a.run[0] = seq_args(p, d[1]); a.run[1] = seq_args(p, d[2]); a.phi = seq_args(p, d[4]);
  const Desc &h = d[3], &g = d[5];
  a.head = HeadArgs{sp(p, h, HEAD_P16), sp(p, h, HEAD_Q16), sp(p, h, HEAD_EPS), sp(p, h, HEAD_MU_P), sp(p, h, HEAD_SD_P), sp(p, h, HEAD_MU_Q),
                    sp(p, h, HEAD_SD_Q), sp(p, h, HEAD_RAW_P), sp(p, h, HEAD_RAW_Q), sp(p, h, HEAD_MUQ_RAW), sp(p, h, HEAD_Z), sp(p, h, HEAD_Z16),
                    sp(p, h, HEAD_Z16B), h.p[HEAD_WP], h.p[HEAD_BP], h.p[HEAD_WQ], h.p[HEAD_BQ], h.ld[LD_OUT], h.n16[N16_OUT], h.n16[N16_OUTB],
                    h.i[HEAD_I_Z], h.i[HEAD_I_RESIDUAL], h.f[HEAD_F_BETA], h.f[HEAD_F_INV_BETA], h.f[HEAD_F_SD_EPS]};
  a.gru = GruArgs{sp(p, g, GRU_X16), sp(p, g, GRU_XG), sp(p, g, GRU_GH), sp(p, g, GRU_HPREV), sp(p, g, GRU_HRM), sp(p, g, GRU_H16), sp(p, g, GRU_H16B),
                  sp(p, g, GRU_RG), sp(p, g, GRU_UG), sp(p, g, GRU_NG), g.p[GRU_WIH], g.p[GRU_BIH], g.ld[GRU_LD_HPREV], g.ld[LD_OUT], g.n16[N16_OUT],
                  g.n16[N16_OUTB], g.i[GRU_I_R]};
  a.ndec = dec ? p.ndesc - kFwdDesc : 0;
  for (int k = 0; k < a.ndec; ++k) a.dec[k] = lin_args(p, d[6 + k]);
  int grid = 0;
  for (int i = 0; i < p.ndesc; ++i) { a.deal[i] = deal_of(d[i], i); grid = std::max(grid, d[i].wg0 + d[i].nwg); }
  a.B = p.B; a.s0 = p.s_first; a.S = S; a.xcd = p.xcd; a.place = place; a.ctl = p.ctl;
  ANAT(a.prof = pchain_profile_buffer();)
  // the posterior half's workgroups [half, gentle) arm around their GRU tiles (descriptor 5) where none of them has a tile of the
  // heads or the phi_z run (3, 4)
  BLVM_TRY(arm_or_fill(p, plan, 5, {3, 4}, half, gentle - half, place_xcd(place, p), stream, &a.arm));
  BLVM_TRY(pre());
  const size_t lds = sizeof(float) * 2 * kFwdProducts * 16 * 256;
  BLVM_TRY(static_go(&vrnn_static_fwd_kernel<16>, 0, grid, lds, "vrnn_static_fwd"));
  hipLaunchKernelGGL(vrnn_static_fwd_kernel<16>, dim3(grid), dim3(1024), lds, stream, a);
  BLVM_CHECK_LAUNCH("vrnn_static_fwd");
  ++g_static_launches;
  if (a.arm.n != 0) ++g_armed_launches;
  return BLVM_OK;
}

int vrnn_static_bwd(const Program& p, hipStream_t stream, const ArmPlan& plan, const std::function<int()>& pre) {
  int place = kPlaceProgram;
  const bool enc = p.ndesc == kBwdEncDesc || p.ndesc == kBwdDecEncDesc;  // with the d_enc follower on the posterior half (the last two descriptors)
  const bool lead = p.ndesc - (enc ? kBwdEncLinks : 0) == kBwdDecDesc;    // with the decoder leader on the spare range
  const int nbase = lead ? kBwdDecDesc : kBwdDesc;
  if (vrnn_static_check(p, nbase + (enc ? kBwdEncLinks : 0), kBwdProducts, 8, 9, &place)) return 1;
  const Desc* d = p.d;
  const int S = p.S;  // T' + 1
  for (int i = 0; i < kBwdDesc; ++i)
    if (d[i].s_begin != 0 || d[i].s_end != (i == 0 ? S : S - 1)) return 1;
  if (!shaped(d[0], K_GRUB, 0, kH) || !shaped(d[1], K_LIN, 0, kR) || !shaped(d[2], K_LIN, 0, kR) || !shaped(d[3], K_LIN, lead ? kPartLeadFlags : 0, kR) ||
      !shaped(d[4], K_LIN, lead ? kGbFlags | DF_ADD2_POLLED : kGbFlags, 3 * kR) || !shaped(d[5], K_LIN, DF_A_SUM3, kH) ||
      !shaped(d[6], K_LINSEQ, DF_SEQ_GATE, kH) || !shaped(d[7], K_DZ, 0, kH) || !shaped(d[8], K_LINSEQ, DF_SEQ_GATE, kH) ||
      !shaped(d[9], K_LINSEQ, DF_SEQ_GATE, kH))
    return 1;
  if (!run(d[6], 2, 0) || !run(d[8], 3, 2 * kH) || !run(d[9], 3, 2 * kH)) return 1;
  if (!one_tile_each(p, kBwdResident, place_xcd(place, p)) || d[7].p[DZ_D2_16] != nullptr) return 1;  // (dz holds the fragments of its one product)
  // roles: prior half [0, d2.wg0) | posterior half [d2.wg0, d4.wg0) | gentle range (GB) [d4.wg0, d3.wg0) | spare range [d3.wg0, ...)
  const int half = d[2].wg0, gentle = d[4].wg0, spare = d[3].wg0;
  if (!within(d[1], 0, half) || !within(d[8], 0, half) || !within(d[2], half, gentle) || !within(d[9], half, gentle) || !within(d[4], gentle, spare) ||
      d[3].nwg <= 0)
    return 1;
  for (int i : {0, 5, 6, 7})
    if (!within(d[i], 0, gentle)) return 1;
  if (lead) {
    // the leader's links: on the range of the third partial sum, active while there is a time step kBdecAhead walk steps ahead; the
    // first reads its row-major operand as it is (K: the descriptor's), the second is resident on one tile per workgroup
    for (int i = kBwdDesc; i < kBwdDecDesc; ++i) {
      if (d[i].s_begin != 0 || d[i].s_end != S - 1 - kBdecAhead || d[i].wg0 != spare || d[i].nwg != d[3].nwg) return 1;
      if (d[i].p[LIN_A2] || d[i].p[LIN_A3] || d[i].p[LIN_O16B] || d[i].p[LIN_ADD] || d[i].p[LIN_ADD2] || d[i].p[LIN_BIAS] || d[i].i[LIN_I_W_WIDTH] != 0) return 1;
    }
    if (d[10].kind != K_LIN || d[10].flags != kBdec0Flags || d[10].K <= 0 || d[10].K % 16 != 0 || d[10].ld[LIN_LD_A] != d[10].K) return 1;
    if (!shaped(d[11], K_LIN, kBdec1Flags, kH) || !shaped(d[12], K_LIN, kBdec2Flags, kH) || d[11].ld[LIN_LD_A] != 0 || d[12].ld[LIN_LD_A] != 0) return 1;
    if (!one_tile_each(p, kBwdDecResident, place_xcd(place, p))) return 1;
    if (d[3].p[LIN_ADD] == nullptr || d[4].p[LIN_ADD2] == nullptr || d[1].p[LIN_ADD] != nullptr || d[0].p[GRUB_DD] != nullptr) return 1;
  }
  if (enc) {
    // the follower's links: one tile of each on every workgroup of the posterior half, which owns no tile of the links between the
    // partial sum and the run; a walk step behind the chain from step kBencLag to the walk's last; X = H; the second link's addend
    // is the first one's output; their operands are the GRU backward's DGI16 and the posterior run's last output, a step back
    const Desc &e0 = d[nbase], &e1 = d[nbase + 1];
    const long st_dgi = p.stride[d[0].sidx[GRUB_DGI16]], st_dq = p.stride[d[9].sidx[LINSEQ_O16 + 2]], st_ep = p.stride[e0.sidx[LIN_ORM]];
    if (e0.p[LIN_A] != d[0].p[GRUB_DGI16] - kBencLag * st_dgi || p.stride[e0.sidx[LIN_A]] != st_dgi) return 1;
    if (e1.p[LIN_A] != d[9].p[LINSEQ_O16 + 2] - kBencLag * st_dq || p.stride[e1.sidx[LIN_A]] != st_dq || p.stride[e1.sidx[LIN_ORM]] != st_ep) return 1;
    for (const Desc* e : {&e0, &e1}) {
      if (e->s_begin != kBencLag || e->s_end != S || e->wg0 != d[9].wg0 || e->nwg != d[9].nwg || e->wg0 != half || e->nwg != gentle - half || e->ct != kH / 16 || e->ct * ((p.B + 15) / 16) != e->nwg) return 1;
      if (e->p[LIN_A2] || e->p[LIN_A3] || e->p[LIN_O16] || e->p[LIN_O16B] || e->p[LIN_GATE] || e->p[LIN_BIAS] || e->p[LIN_ADD2] || !e->p[LIN_ORM]) return 1;
      if (e->i[LIN_I_W_WIDTH] != 0 || e->ld[LIN_LD_A] != 0 || e->ld[LD_OUT] != kH) return 1;
    }
    if (!shaped(e0, K_LIN, kBenc0Flags, 3 * kR) || !shaped(e1, K_LIN, kBenc1Flags, kH) || e0.p[LIN_ADD] != nullptr) return 1;
    if (e1.p[LIN_ADD] != e0.p[LIN_ORM] || p.stride[e1.sidx[LIN_ADD]] != st_ep || e1.ld[LIN_LD_ADD] != kH) return 1;
    if (!one_tile_each(p, {nbase, nbase + 1}, place_xcd(place, p))) return 1;
    for (int i : {5, 6, 7})
      if (!within(d[i], 0, half)) return 1;
  }
  BwdArgs a{};
  const Desc& g = d[0];
  a.grub = GrubArgs{sp(p, g, GRUB_D0_16), sp(p, g, GRUB_D1_16), sp(p, g, GRUB_G_IN), sp(p, g, GRUB_RG), sp(p, g, GRUB_UG), sp(p, g, GRUB_NG), sp(p, g, GRUB_GH),
                    sp(p, g, GRUB_HPREV), sp(p, g, GRUB_DD), sp(p, g, GRUB_DGI), sp(p, g, GRUB_DGI16), sp(p, g, GRUB_DGH), sp(p, g, GRUB_DGH16), sp(p, g, GRUB_GA),
                    sp(p, g, GRUB_G_ADD), g.p[GRUB_W0], g.p[GRUB_W1], g.p[GRUB_G_OUT], g.ld[GRUB_LD_H], g.ld[GRUB_LD_GADD], g.ld[LD_OUT], g.n16[N16_OUT],
                    g.i[GRUB_I_R], g.i[GRUB_I_GEMM_FROM], g.i[GRUB_I_GATES_TO], g.i[GRUB_I_GIN_FROM]};
  for (int k = 0; k < 3; ++k) a.part[k] = lin_args(p, d[1 + k]);
  a.gb = lin_args(p, d[4]); a.sum = lin_args(p, d[5]);
  a.phi = seq_args(p, d[6]); a.run[0] = seq_args(p, d[8]); a.run[1] = seq_args(p, d[9]);
  const Desc& z = d[7];
  a.dz = DzArgs{sp(p, z, DZ_D16), sp(p, z, DZ_ADD), sp(p, z, DZ_MU_Q), sp(p, z, DZ_SD_Q), sp(p, z, DZ_MU_P), sp(p, z, DZ_SD_P),
                sp(p, z, DZ_EPS), sp(p, z, DZ_RAW_Q), sp(p, z, DZ_RAW_P), sp(p, z, DZ_MUQ_RAW), sp(p, z, DZ_DQH), sp(p, z, DZ_DQH16), sp(p, z, DZ_DPH),
                sp(p, z, DZ_DPH16), z.p[DZ_WT], z.p[DZ_C_RAW], z.p[DZ_C_FN], reinterpret_cast<const int32_t*>(z.p[DZ_X_SL]), z.ld[DZ_LD_ADD],
                z.ld[LD_OUT], z.n16[N16_OUT], z.i[DZ_I_Z], z.i[DZ_I_RESIDUAL], z.i[DZ_I_STRIDE], z.i[DZ_I_T0], (int)z.f[DZ_F_GEMM_FROM], z.f[DZ_F_FN_FLOOR],
                z.f[DZ_F_BETA], z.f[DZ_F_SD_EPS]};
  a.nbdec = lead ? 3 : 0;
  if (lead) { a.bdec_k = d[kBwdDesc].K; a.gb_add2 = sp(p, d[4], LIN_ADD2); a.gb_ldadd2 = d[4].i[LIN_I_LD_ADD2]; }
  for (int k = 0; k < a.nbdec; ++k) a.bdec[k] = lin_args(p, d[kBwdDesc + k]);
  a.nenc = enc ? kBwdEncLinks : 0;
  if (enc) {
    const Desc &e0 = d[nbase], &e1 = d[nbase + 1];
    a.enc = EncArgs{const_cast<float*>(e0.p[LIN_ORM]), const_cast<float*>(e1.p[LIN_ORM]), e0.p[LIN_W], e1.p[LIN_W], (int)p.stride[e0.sidx[LIN_ORM]]};
  }
  int grid = 0;
  for (int i = 0; i < p.ndesc; ++i) {
    if (i < nbase) a.deal[i] = deal_of(d[i], i);
    grid = std::max(grid, d[i].wg0 + d[i].nwg);
  }
  a.B = p.B; a.s0 = p.s_first; a.S = S; a.xcd = p.xcd; a.place = place; a.ctl = p.ctl;
  ANAT(a.prof = pchain_profile_buffer();)
  // the spare range's workgroups arm around their partial-sum tiles (descriptor 3)
  BLVM_TRY(arm_or_fill(p, plan, 3, {}, spare, d[3].nwg, place_xcd(place, p), stream, &a.arm));
  BLVM_TRY(pre());
  const size_t lds = sizeof(float) * 2 * kBwdProducts * 16 * 256;
  if (enc) {
    BLVM_TRY(static_go(&vrnn_static_bwd_kernel<16, true>, 3, grid, lds, "vrnn_static_bwd"));
    hipLaunchKernelGGL((vrnn_static_bwd_kernel<16, true>), dim3(grid), dim3(1024), lds, stream, a);
  } else {
    BLVM_TRY(static_go(&vrnn_static_bwd_kernel<16, false>, 1, grid, lds, "vrnn_static_bwd"));
    hipLaunchKernelGGL((vrnn_static_bwd_kernel<16, false>), dim3(grid), dim3(1024), lds, stream, a);
  }
  BLVM_CHECK_LAUNCH("vrnn_static_bwd");
  ++g_static_launches;
  if (a.arm.n != 0) ++g_armed_launches;
  return BLVM_OK;
}

}  // namespace

int vrnn_launch(pchain::Builder& bld, bool forward, const char* who, hipStream_t stream, const pchain::ArmPlan& plan, const std::function<int()>& pre) {
  BLVM_TRY(pchain_prepare(bld, who));
  const int rc = forward ? vrnn_static_fwd(bld.p, stream, plan, pre) : vrnn_static_bwd(bld.p, stream, plan, pre);
  if (rc != 1) return rc;
  BLVM_TRY(full_fill(plan, stream));  // (the static converters return 1 in front of any fill)
  BLVM_TRY(pre());
  return pchain_run(bld.p, stream);
}

}  // namespace blvm

extern "C" int blvm_pchain_static(int mode) {
  if (mode == -2) return (int)std::min<long>(blvm::g_static_launches, 0x7fffffffL);
  if (mode == -3) return (int)std::min<long>(blvm::g_armed_launches, 0x7fffffffL);
  const int was = blvm::g_static;
  if (mode >= 0) blvm::g_static = mode != 0;
  return was;
}

// blvm_pchain_chain_probe's chain (one K_LIN descriptor per link, the same Builder program) walked by the static kernel.  N = 256 or 512.
// resident: the weights stay in registers for the launch (at most one tile per workgroup), else they are re-read every link.
static int static_chain_probe(const float* W16, const float* bias, float* x16, float* xs, int B, int N, int L, int nwg, void* stream_, bool resident,
                              bool pace = false, int early = 0, int epi = 0) {
  using namespace blvm;
  using namespace blvm::pchain;
  hipStream_t s = static_cast<hipStream_t>(stream_);
  BLVM_REQUIRE(W16 && bias && x16 && xs && B > 0 && N > 0 && N % 16 == 0 && L > 0, "pchain_static_chain_probe: bad arguments");
  const int rt = (B + 15) / 16;
  const long x = (long)rt * 16 * N, sN = (long)B * N;
  Builder bld;
  bld.begin(OP_F32, L, B, 1, false, 0);
  const int nw = nwg > 0 ? nwg : range_for((N / 16) * rt, device_cus() & ~7);
  Operands o;
  o.p[LIN_A] = {x16, x}; o.p[LIN_W] = W16; o.p[LIN_BIAS] = bias; o.p[LIN_ORM] = {xs, sN}; o.p[LIN_O16] = {x16 + x, x}; o.ld[LD_OUT] = N; o.n16[N16_OUT] = N / 16;
  add_desc(bld, K_LIN, N / 16, 0, nw, N, DF_RELU, 0, L, o);
  BLVM_HIP(pchain_fill_sentinel(x16 + x, sizeof(float) * (size_t)x * L, s));
  BLVM_TRY(pchain_prepare(bld, "pchain_static_chain_probe"));
  const int rc = static_lin_chain_launch(bld.p, s, resident, pace, early, epi);
  BLVM_REQUIRE(rc != 1, "pchain_static_chain_probe: no static kernel for N = %d (256, 512) or this deal", N);
  return rc;
}
extern "C" int blvm_pchain_static_chain_probe(const float* W16, const float* bias, float* x16, float* xs, int B, int N, int L, int nwg, void* stream) {
  return static_chain_probe(W16, bias, x16, xs, B, N, L, nwg, stream, true);
}
extern "C" int blvm_pchain_static_chain_probe_fetch(const float* W16, const float* bias, float* x16, float* xs, int B, int N, int L, int nwg, void* stream) {
  return static_chain_probe(W16, bias, x16, xs, B, N, L, nwg, stream, false);
}
// The resident form under a poll pacing policy (pchain.h): the first poll of a tile waits `early_delay` s_sleep units on the waves that
// leave the previous tile at its barrier and `epi_delay` on the epilogue waves (0 .. 64 each).  Both zero is
// blvm_pchain_static_chain_probe's plain loop.  Probe only: the VRNN walks take their pacing at compile time.
extern "C" int blvm_pchain_static_chain_probe_paced(const float* W16, const float* bias, float* x16, float* xs, int B, int N, int L, int nwg,
                                                    int early_delay, int epi_delay, void* stream) {
  using namespace blvm;
  BLVM_REQUIRE(early_delay >= 0 && early_delay <= 64 && epi_delay >= 0 && epi_delay <= 64,
               "pchain_static_chain_probe_paced: delays are 0 .. 64 s_sleep units");
  return static_chain_probe(W16, bias, x16, xs, B, N, L, nwg, stream, true, (early_delay | epi_delay) != 0, early_delay, epi_delay);
}
