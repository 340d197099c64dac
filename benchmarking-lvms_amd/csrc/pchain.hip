// pchain.hip — the persistent-chain engine: ONE kernel that executes a host-built program of link descriptors (pchain.h) for a
// whole recurrent sequence.  Replaces, per model, thousands of dependent launches (VRNN [64,16000]: 4 500 per train step) by one
// forward and one backward launch.  What the slots of a descriptor hold, by tile kind: pchain.h.
#include <algorithm>
#include <mutex>

#include "common.h"
#include "pchain.h"
#include "pchain_rt.h"

namespace blvm {
namespace {
using namespace pchain;

// A descriptor as the kernel reads it: 128 dwords, resolved (strides per pointer) by pchain_resolve_kernel right before the launch
// and copied into LDS by every workgroup.  Every wave keeps the descriptor of its current tile in TWO VGPRs (lane l holds dword l /
// 64 + l: two ds_read_b32) and reads a field with v_readlane; the NEXT descriptor's two LDS reads are issued at the top of the
// current tile.  LDS, not global memory: on gfx9 vector loads AND stores share the vmcnt counter, so waiting for a prefetched
// global load at the top of the next tile also sat out the previous tile's write-through stores (~0.9 us per tile, found with
// blvm_pchain_chain_probe against tools/pchain_probe.hip); LDS reads are counted by lgkmcnt.
//   dword 0 kind  1 ct  2 wg0  3 nwg  4 flags  5 K  6 s_begin  7 s_end  8..11 ld  12..13 n16  14..17 i  18..21 f
//         24 + 2k, 25 + 2k: pointer k (k < 20)        64 + k: its per-step stride in floats (int32)
//         84: number of tiles of THIS workgroup, 85 ..: its tiles as r0 | column tile << 16 — written once by each workgroup into
//         its own LDS copy (TileIter involves integer divisions: ~0.5 us per tile when run inside the step loop)
constexpr int kDescWords = 128;
enum { RD_KIND = 0, RD_CT, RD_WG0, RD_NWG, RD_FLAGS, RD_K, RD_SBEGIN, RD_SEND, RD_LD = 8, RD_N16 = 12, RD_I = 14, RD_F = 18, RD_P = 24, RD_ST = 64,
       RD_NT = 84, RD_TILE = 85 };
constexpr int kMaxTilesPerWg = kDescWords - RD_TILE;
struct Hdr {
  int ndesc, s0, S, B, xcd, prof_wg, lds_products;  // steps [s0, S)
  Ctl ctl;
  unsigned long long* prof;
};

// descriptors reach the device a few per launch (kernel arguments are limited to 4 KB)
constexpr int kResolveChunk = 12;
struct ProgramPart {
  int ndesc, first;
  long stride[16];
  Desc d[kResolveChunk];
};
static_assert(sizeof(ProgramPart) <= 4096, "kernel argument size");

__global__ void pchain_resolve_kernel(ProgramPart a, int* __restrict__ out) {
  out += (size_t)a.first * kDescWords;
  for (int e = threadIdx.x; e < a.ndesc * kDescWords; e += blockDim.x) {
    const int i = e / kDescWords, k = e % kDescWords;
    const Desc& d = a.d[i];
    int v = 0;
    if (k == RD_KIND) v = d.kind;
    else if (k == RD_CT) v = d.ct;
    else if (k == RD_WG0) v = d.wg0;
    else if (k == RD_NWG) v = d.nwg;
    else if (k == RD_FLAGS) v = d.flags;
    else if (k == RD_K) v = d.K;
    else if (k == RD_SBEGIN) v = d.s_begin;
    else if (k == RD_SEND) v = d.s_end;
    else if (k >= RD_LD && k < RD_LD + 4) v = d.ld[k - RD_LD];
    else if (k >= RD_N16 && k < RD_N16 + 2) v = d.n16[k - RD_N16];
    else if (k >= RD_I && k < RD_I + 4) v = d.i[k - RD_I];
    else if (k >= RD_F && k < RD_F + 4) v = __float_as_int(d.f[k - RD_F]);
    else if (k >= RD_P && k < RD_P + 2 * kMaxPtr) {
      const unsigned long long q = reinterpret_cast<unsigned long long>(d.p[(k - RD_P) >> 1]);
      v = (int)(((k - RD_P) & 1) ? (q >> 32) : (q & 0xffffffffull));
    } else if (k >= RD_ST && k < RD_ST + kMaxPtr) {
      v = (int)a.stride[d.sidx[k - RD_ST]];
    }
    out[e] = v;
  }
}

// the descriptor of the current tile, one dword per lane in two VGPRs, plus the pointers OF THE STEP it will be used in: lane k of
// (plo, phi) = pointer k + step * stride k, computed for all twenty pointers at once by four vector instructions when the
// descriptor is fetched (one tile ahead) — as scalar code in front of the tile it was ~7 dependent SALU instructions per pointer,
// ~0.3 us of every link
struct DescRegs {
  int v0, v1;
  unsigned plo, phi;
  __device__ __forceinline__ void fetch(const int* tab_lds, int i, int step) {
    const int lane = threadIdx.x & 63;
    const int* q = tab_lds + i * kDescWords;
    v0 = q[lane];
    v1 = q[64 + lane];
    const int k = lane < kMaxPtr ? lane : 0;
    const unsigned long long base = ((unsigned long long)(unsigned)q[RD_P + 2 * k + 1] << 32) | (unsigned)q[RD_P + 2 * k];
    const unsigned long long p = base + (unsigned long long)((long long)step * (long long)q[RD_ST + k] * 4);
    plo = (unsigned)p;
    phi = (unsigned)(p >> 32);
  }
  template <int IDX>
  __device__ __forceinline__ int w() const {
    return IDX < 64 ? __builtin_amdgcn_readlane(v0, IDX & 63) : __builtin_amdgcn_readlane(v1, IDX & 63);
  }
  __device__ __forceinline__ int tile(int k) const { return __builtin_amdgcn_readlane(v1, RD_TILE - 64 + k); }  // k wave-uniform
  template <int IDX>
  __device__ __forceinline__ float f() const { return __int_as_float(w<RD_F + IDX>()); }
  template <int K>
  __device__ __forceinline__ const float* base() const {
    const unsigned long long lo = (unsigned)w<RD_P + 2 * K>(), hi = (unsigned)w<RD_P + 2 * K + 1>();
    return reinterpret_cast<const float*>((hi << 32) | lo);
  }
  // pointer k at the step the descriptor was fetched for (null stays null: its stride is 0)
  template <int K>
  __device__ __forceinline__ const float* p(int) const {
    const unsigned long long lo = (unsigned)__builtin_amdgcn_readlane((int)plo, K), hi = (unsigned)__builtin_amdgcn_readlane((int)phi, K);
    return reinterpret_cast<const float*>((hi << 32) | lo);
  }
  template <int K>
  __device__ __forceinline__ float* m(int s) const { return const_cast<float*>(p<K>(s)); }
  // the same with a wave-uniform RUN-TIME pointer index (v_readlane takes the lane from an SGPR)
  __device__ __forceinline__ const float* pdyn(int k) const {
    const unsigned long long lo = (unsigned)__builtin_amdgcn_readlane((int)plo, k), hi = (unsigned)__builtin_amdgcn_readlane((int)phi, k);
    return reinterpret_cast<const float*>((hi << 32) | lo);
  }
  __device__ __forceinline__ const float* basedyn(int k) const {  // (RD_P + 2k < 64: pointers live in v0)
    const unsigned long long lo = (unsigned)__builtin_amdgcn_readlane(v0, RD_P + 2 * k), hi = (unsigned)__builtin_amdgcn_readlane(v0, RD_P + 2 * k + 1);
    return reinterpret_cast<const float*>((hi << 32) | lo);
  }
  __device__ __forceinline__ int wdyn(int idx) const { return __builtin_amdgcn_readlane(v0, idx); }  // idx < 64
};

// ROLL: the instantiation that runs the LSTM roll-out (lstm_decode.hip) — the tile kinds of that program only (K_LIN, K_LINSEQ, K_LSTM,
// K_DMOLS).  The cell arm inside the shared instantiation cost the fp32 one 4 bytes of scratch per lane, and that kernel
// is the training kernel: it has every kind but K_LSTM and is the same code with or without the roll-out.
template <int NW, int OT, bool ROLL = false>
__global__ __launch_bounds__(NW * 64, 1) void pchain_kernel(const int* __restrict__ tab, Hdr a) {
  extern __shared__ __attribute__((aligned(16))) char lds_all[];  // [descriptors | profile | 2 x (lds_products x NW x 256) floats]
  int* const ltab = reinterpret_cast<int*>(lds_all);
  unsigned long long* const pacc = reinterpret_cast<unsigned long long*>(lds_all + sizeof(int) * kDescWords * kMaxDesc);
  float* const red0 = reinterpret_cast<float*>(lds_all + sizeof(int) * kDescWords * kMaxDesc + 32 * sizeof(unsigned long long));
  float* const red1 = red0 + a.lds_products * NW * 256;
  const int w = blockIdx.x, B = a.B, rt = (B + 15) / 16;
  const bool xcd = a.xcd != 0;
  for (int e = threadIdx.x; e < a.ndesc * kDescWords; e += NW * 64) ltab[e] = tab[e];
  if (threadIdx.x < 32) pacc[threadIdx.x] = 0ull;
  unsigned mine = 0;  // the descriptors this workgroup has tiles of
  for (int i = 0; i < a.ndesc; ++i) {
    const int* q = tab + (size_t)i * kDescWords;
    if (TileIter(w, q[RD_WG0], q[RD_NWG], rt, q[RD_CT], xcd).valid()) mine |= 1u << i;
  }
  __syncthreads();
  if (threadIdx.x < a.ndesc) {  // this workgroup's tiles of descriptor threadIdx.x, into its own copy of the table
    int* q = ltab + threadIdx.x * kDescWords;
    int k = 0;
    for (TileIter it(w, q[RD_WG0], q[RD_NWG], rt, q[RD_CT], xcd); it.valid() && k < kMaxTilesPerWg; it.next()) q[RD_TILE + k++] = it.r0() | (it.c() << 16);
    q[RD_NT] = k;
  }
  __syncthreads();
  if (mine == 0) return;
  int par = 0;
  auto red = [&]() { par ^= 1; return par ? red0 : red1; };
  Poll pl{a.ctl, 0u, false, 1};
  // per-descriptor tick counters (blvm_pchain_profile) only in -DPCHAIN_PROF builds (and the stamped -DPCHAIN_TPROF* ones): in the
  // product kernel their state would sit in registers the walk needs (tools/probe_engine_chain.py: every live scalar costs)
#if defined(PCHAIN_PROF) || defined(PCHAIN_TPROF) || defined(PCHAIN_TPROF2)
  const bool profiled = a.prof != nullptr && (w == 0 || w == a.prof_wg) && threadIdx.x == 0;
#else
  constexpr bool profiled = false;
#endif
  unsigned long long tprev = profiled ? wall_clock64() : 0ull;
#ifdef PCHAIN_TPROF2
  unsigned long long tq[6] = {0ull, 0ull, 0ull, 0ull, 0ull, 0ull}, tq_end = 0ull;
#endif
  DescRegs d, nx;
  d.fetch(ltab, __builtin_ctz(mine), a.s0);
  for (int s = a.s0; s < a.S; ++s) {
    for (unsigned m = mine; m != 0; m &= m - 1) {
      const int i = __builtin_ctz(m);
#ifdef PCHAIN_TPROF2
      const unsigned long long tq0 = wall_clock64();
      if (tq_end) tq[2] += tq0 - tq_end;
#endif
      // request the next descriptor of this workgroup's walk now; it lands while this tile runs
      const unsigned rest = m & (m - 1);
      const int nx_i = __builtin_ctz(rest != 0 ? rest : mine), nx_s = rest != 0 ? s : s + 1;
      const int kind = d.w<RD_KIND>(), flags = d.w<RD_FLAGS>(), K = d.w<RD_K>();
      const bool active = s >= d.w<RD_SBEGIN>() && s < d.w<RD_SEND>();
#ifdef PCHAIN_TPROF2
      const unsigned long long tqa = wall_clock64();
      tq[3] += tqa - tq0;
#endif
      // (a linear tile fetches the next descriptor itself, in the shadow of its operand wait)
      if (!active || (kind != K_LIN && kind != K_LINSEQ)) nx.fetch(ltab, nx_i, nx_s);
      if (active) {
        const int nt = d.w<RD_NT>();
        pl.nap = (flags & DF_GENTLE) ? 16 : 1;
        pl.code = ((unsigned)s << 4) | (unsigned)i;
        switch (kind) {
          case K_LIN: {
            // Only what the operand loads need is taken out of the descriptor here; everything the epilogue needs (and the next
            // descriptor's fetch) is done by `late`, which the tile calls once its first loads are in flight.
            const bool a_polled = !(flags & DF_A_PLAIN);
            const float *A = d.p<LIN_A>(s), *W = d.base<LIN_W>();
            const float *A2 = (flags & DF_A_SUM3) ? d.p<LIN_A2>(s) : nullptr, *A3 = (flags & DF_A_SUM3) ? d.p<LIN_A3>(s) : nullptr;
            const int ld0 = d.w<RD_LD + LIN_LD_A>(), w_width = d.w<RD_I + LIN_I_W_WIDTH>();
#ifdef PCHAIN_TPROF2
            const unsigned long long tqb = wall_clock64();
            tq[4] += tqb - tqa;
#endif
            auto late = [&]() {
              __builtin_amdgcn_sched_barrier(0);
              nx.fetch(ltab, nx_i, nx_s);  // (per tile: the same lanes again — cheaper than a flag carried through the visit)
              // (the early and the second addend: the fp32 training instantiation only — pchain_run refuses them elsewhere; in the 16-bit
              // kernels the three extra fields cost 35 SGPR spills and 0.25 ms of a bf16 VRNN step, used or not)
              if constexpr (OT == OP_F32 && !ROLL)
                return LinLate{d.base<LIN_BIAS>(), d.p<LIN_ADD>(s), d.p<LIN_GATE>(s), d.w<RD_LD + LIN_LD_ADD>(), d.w<RD_LD + LIN_LD_GATE>(), (flags & DF_ADD_POLLED) != 0,
                               (flags & DF_RELU) != 0, d.f<LIN_F_SLOPE>(), Out{d.m<LIN_ORM>(s), d.w<RD_LD + LD_OUT>(), (flags & DF_RM_SC1) != 0, d.m<LIN_O16>(s),
                                                                               d.w<RD_N16 + N16_OUT>(), d.m<LIN_O16B>(s), d.w<RD_N16 + N16_OUTB>()},
                               (flags & DF_ADD_EARLY) != 0, (flags & DF_ADD2_POLLED) ? d.p<LIN_ADD2>(s) : nullptr, d.w<RD_I + LIN_I_LD_ADD2>()};
              else
                return LinLate{d.base<LIN_BIAS>(), d.p<LIN_ADD>(s), d.p<LIN_GATE>(s), d.w<RD_LD + LIN_LD_ADD>(), d.w<RD_LD + LIN_LD_GATE>(), (flags & DF_ADD_POLLED) != 0,
                               (flags & DF_RELU) != 0, d.f<LIN_F_SLOPE>(), Out{d.m<LIN_ORM>(s), d.w<RD_LD + LD_OUT>(), (flags & DF_RM_SC1) != 0, d.m<LIN_O16>(s),
                                                                               d.w<RD_N16 + N16_OUT>(), d.m<LIN_O16B>(s), d.w<RD_N16 + N16_OUTB>()}};
            };
            for (int tk = 0; tk < nt; ++tk) {
              const int trc = d.tile(tk), tr0 = trc & 0xffff, tc0 = (trc >> 16) * 16;
              if ((flags & DF_CANARY) && a_polled) canary_wait(A, tr0, K, pl, ld0);
#ifdef PCHAIN_TPROF2
              const unsigned long long tq1 = wall_clock64();
              tq[0] += tq1 - tq0;
#endif
              tile_lin_late<NW, OT>(A, ld0, a_polled, W, K, late, tr0, tc0, B, red(), pl, A2, A3, w_width);
#ifdef PCHAIN_TPROF2
              tq_end = wall_clock64();
              tq[1] += tq_end - tq1;
#endif
            }
            if (nt == 0) nx.fetch(ltab, nx_i, nx_s);  // (a visit without tiles)
          } break;
          case K_LINSEQ: {
            const int n = d.w<RD_I + LINSEQ_I_N>();
            const bool gated = (flags & DF_SEQ_GATE) != 0;
            const float* A = d.p<LINSEQ_A0>(s);
            const int K0 = d.w<RD_I + LINSEQ_I_K0>();  // the FIRST link's K when it is not the run's (0: it is): the link in front of a run joins its visit
            for (int lq = 0; lq < n; ++lq) {  // (links outside, tiles inside: link li+1 of any tile needs link li of ALL tiles of its row tile)
              int li = lq;
              asm volatile("" : "+s"(li));  // opaque: the five lane indices below are li + constant where they are used, not five more loop counters in SGPRs
              pl.code = ((unsigned)s << 4) | (unsigned)i | ((unsigned)li << 28);
              const float* W = d.basedyn(LINSEQ_W + li);
              const int Kl = (li == 0 && K0 != 0) ? K0 : K;
              auto late = [&]() {
                __builtin_amdgcn_sched_barrier(0);
                if (li == 0) nx.fetch(ltab, nx_i, nx_s);  // the next descriptor, once per visit, behind the first link's operand loads (every tile of it: the same lanes again)
                const float* aux = d.pdyn(LINSEQ_AUX + li);  // bias (stride 0: the stepped pointer IS the base) | gate (stepped)
                const float* add0 = li == 0 ? d.p<LINSEQ_ADD0>(s) : nullptr;  // the first link's row-major addend (null: none)
                return LinLate{gated ? nullptr : aux, add0, gated ? aux : nullptr, d.w<RD_I + LINSEQ_I_LD_ADD0>(), d.w<RD_I + LINSEQ_I_LD_GATE>(), false,
                               (flags & DF_RELU) != 0, d.f<LINSEQ_F_SLOPE>(), Out{const_cast<float*>(d.pdyn(LINSEQ_ORM + li)), d.wdyn(RD_LD + LINSEQ_LD_ORM + li),
                                                                                  false, const_cast<float*>(d.pdyn(LINSEQ_O16 + li)), d.w<RD_N16 + N16_OUT>()}};
              };
              // (a run's links are plain: a partial-sum operand or a K-range is a K_LIN in front of the run.  The summing link as a run's first
              // link was built and measured, r03: the three-slab product inlined at this call site costs the WHOLE kernel +0.4 ms per
              // VRNN step, used or not, and saves 0.08)
              for (int tk = 0; tk < nt; ++tk) {
                const int trc = d.tile(tk), tr0 = trc & 0xffff, tc0 = (trc >> 16) * 16;
                tile_lin_late<NW, OT>(A, 0, true, W, Kl, late, tr0, tc0, B, red(), pl);
              }
              A = d.pdyn(LINSEQ_O16 + li);  // the next link multiplies what this one stored
            }
            if (nt == 0) nx.fetch(ltab, nx_i, nx_s);  // (a visit without tiles)
          } break;
          case K_HEAD: if constexpr (!ROLL) {
            const int ld3 = d.w<RD_LD + LD_OUT>(), n16 = d.w<RD_N16 + N16_OUT>();
            const HeadOut o{d.m<HEAD_MU_P>(s), d.m<HEAD_SD_P>(s), d.m<HEAD_MU_Q>(s), d.m<HEAD_SD_Q>(s), d.m<HEAD_RAW_P>(s), d.m<HEAD_RAW_Q>(s), d.m<HEAD_MUQ_RAW>(s),
                            Out{d.m<HEAD_Z>(s), ld3, false, d.m<HEAD_Z16>(s), n16, d.m<HEAD_Z16B>(s), d.w<RD_N16 + N16_OUTB>()}};
            const int Z = d.w<RD_I + HEAD_I_Z>(), residual = d.w<RD_I + HEAD_I_RESIDUAL>();
            for (int tk = 0; tk < nt; ++tk) {
              const int trc = d.tile(tk);
              tile_head<NW, OT>(d.p<HEAD_P16>(s), d.p<HEAD_Q16>(s), true, d.base<HEAD_WP>(), d.base<HEAD_BP>(), d.base<HEAD_WQ>(), d.base<HEAD_BQ>(), d.p<HEAD_EPS>(s), o,
                                K, Z, residual, d.f<HEAD_F_BETA>(), d.f<HEAD_F_INV_BETA>(), d.f<HEAD_F_SD_EPS>(), trc & 0xffff, (trc >> 16) * 16, B, red(), pl);
            }
          } break;
          case K_GRU: if constexpr (!ROLL) {
            const int ld0 = d.w<RD_LD + GRU_LD_HPREV>(), ld3 = d.w<RD_LD + LD_OUT>(), n16 = d.w<RD_N16 + N16_OUT>();
            const Out o{d.m<GRU_HRM>(s), ld3, true, d.m<GRU_H16>(s), n16, d.m<GRU_H16B>(s), d.w<RD_N16 + N16_OUTB>()};
            const int R = d.w<RD_I + GRU_I_R>();
            for (int tk = 0; tk < nt; ++tk) {
              const int trc = d.tile(tk);
              tile_gru<NW, OT>(d.p<GRU_X16>(s), 0, true, d.base<GRU_WIH>(), K, d.p<GRU_XG>(s), d.base<GRU_BIH>(), d.p<GRU_GH>(s), d.p<GRU_HPREV>(s), ld0, R, o,
                               d.m<GRU_RG>(s), d.m<GRU_UG>(s), d.m<GRU_NG>(s), trc & 0xffff, (trc >> 16) * 16, B, red(), pl);
            }
          } break;
          case K_DZ: if constexpr (!ROLL) {
            const int ld1 = d.w<RD_LD + DZ_LD_ADD>(), ld3 = d.w<RD_LD + LD_OUT>(), n16 = d.w<RD_N16 + N16_OUT>();
            DzIn z;
            z.mu_q = d.p<DZ_MU_Q>(s); z.sd_q = d.p<DZ_SD_Q>(s); z.mu_p = d.p<DZ_MU_P>(s); z.sd_p = d.p<DZ_SD_P>(s); z.eps = d.p<DZ_EPS>(s); z.raw_q = d.p<DZ_RAW_Q>(s);
            z.raw_p = d.p<DZ_RAW_P>(s); z.muq_raw = d.p<DZ_MUQ_RAW>(s); z.x_sl = reinterpret_cast<const int32_t*>(d.base<DZ_X_SL>()); z.c_raw = d.base<DZ_C_RAW>();
            z.c_fn = d.base<DZ_C_FN>(); z.t = d.w<RD_I + DZ_I_T0>() - s; z.stride = d.w<RD_I + DZ_I_STRIDE>(); z.residual = d.w<RD_I + DZ_I_RESIDUAL>();
            z.fn_floor = d.f<DZ_F_FN_FLOOR>(); z.beta = d.f<DZ_F_BETA>(); z.sd_eps = d.f<DZ_F_SD_EPS>(); z.has_gemm = s >= (int)d.f<DZ_F_GEMM_FROM>();
            const int Z = d.w<RD_I + DZ_I_Z>();
            const Out oq{d.m<DZ_DQH>(s), ld3, false, d.m<DZ_DQH16>(s), n16}, op{d.m<DZ_DPH>(s), ld3, false, d.m<DZ_DPH16>(s), n16};
            for (int tk = 0; tk < nt; ++tk) {
              const int trc = d.tile(tk);
              tile_dz<NW, OT>(d.p<DZ_D16>(s), d.base<DZ_WT>(), d.p<DZ_D2_16>(s), d.base<DZ_WT2>(), true, d.p<DZ_ADD>(s), ld1, (flags & DF_ADD_POLLED) != 0, z, oq,
                              op, K, Z, trc & 0xffff, (trc >> 16) * 16, B, red(), pl);
            }
          } break;
          case K_GRUB: if constexpr (!ROLL) {
            const int ld0 = d.w<RD_LD + GRUB_LD_H>(), ld1 = d.w<RD_LD + GRUB_LD_GADD>(), ld3 = d.w<RD_LD + LD_OUT>(), n16 = d.w<RD_N16 + N16_OUT>();
            GrubIn g;
            g.D0 = d.p<GRUB_D0_16>(s); g.D1 = d.p<GRUB_D1_16>(s); g.W0 = d.base<GRUB_W0>(); g.W1 = d.base<GRUB_W1>(); g.g_in = d.p<GRUB_G_IN>(s);
            g.g_add = d.p<GRUB_G_ADD>(s); g.ld_gadd = ld1; g.rg = d.p<GRUB_RG>(s); g.ug = d.p<GRUB_UG>(s); g.ng = d.p<GRUB_NG>(s); g.gh = d.p<GRUB_GH>(s);
            g.hprev = d.p<GRUB_HPREV>(s); g.dd = d.p<GRUB_DD>(s); g.ldh = ld0; g.dgi = Out{d.m<GRUB_DGI>(s), ld3, false, d.m<GRUB_DGI16>(s), n16};
            g.dgh = Out{d.m<GRUB_DGH>(s), ld3, false, d.m<GRUB_DGH16>(s), n16}; g.ga = d.m<GRUB_GA>(s); g.g_out = const_cast<float*>(d.base<GRUB_G_OUT>());
            g.has_gemm = s >= d.w<RD_I + GRUB_I_GEMM_FROM>(); g.has_gates = s < d.w<RD_I + GRUB_I_GATES_TO>(); g.has_gin = s >= d.w<RD_I + GRUB_I_GIN_FROM>();
            const int R = d.w<RD_I + GRUB_I_R>();
            for (int tk = 0; tk < nt; ++tk) {
              const int trc = d.tile(tk);
              tile_grub<NW, OT>(g, K, R, trc & 0xffff, (trc >> 16) * 16, B, red(), pl);
            }
          } break;
          case K_GRUS: if constexpr (!ROLL) {
            const int ld3 = d.w<RD_LD + LD_OUT>(), n16 = d.w<RD_N16 + N16_OUT>();
            const int R = d.w<RD_I + GRUS_I_R>();
            GruSeqIn g;
            g.H16 = d.p<GRUS_H16>(s); g.Whh = d.base<GRUS_WHH>(); g.bhh = d.base<GRUS_BHH>(); g.xg = d.base<GRUS_XG>();
            g.lens = reinterpret_cast<const int32_t*>(d.base<GRUS_LENS>()); g.hprev = d.p<GRUS_HPREV>(s); g.out = const_cast<float*>(d.base<GRUS_OUT>());
            g.rg = d.m<GRUS_RG>(s); g.ug = d.m<GRUS_UG>(s); g.ng = d.m<GRUS_NG>(s); g.ghn = d.m<GRUS_GHN>(s); g.out_ts = d.w<RD_I + GRUS_I_OUT_TS>();
            g.out_ld = d.w<RD_I + GRUS_I_OUT_LD>(); g.j = s; g.reverse = d.w<RD_I + GRUS_I_REVERSE>();
            const Out o{d.m<GRUS_HNEXT>(s), ld3, false, d.m<GRUS_HNEXT16>(s), n16};
            for (int tk = 0; tk < nt; ++tk) {
              const int trc = d.tile(tk);
              tile_gru_seq<NW, OT>(g, o, R, trc & 0xffff, (trc >> 16) * 16, B, red(), pl);
            }
          } break;
          case K_GRUSB: if constexpr (!ROLL) {
            const int ld3 = d.w<RD_LD + LD_OUT>(), n16 = d.w<RD_N16 + N16_OUT>();
            const int R = d.w<RD_I + GRUSB_I_R>(), T = d.w<RD_N16 + GRUSB_N16_T>();
            GruSeqBwdIn g;
            g.DGHn16 = d.p<GRUSB_DGH16_IN>(s); g.WhhT = d.base<GRUSB_WHHT>(); g.dout = d.base<GRUSB_DOUT>(); g.rg = d.p<GRUSB_RG>(s); g.ug = d.p<GRUSB_UG>(s);
            g.ng = d.p<GRUSB_NG>(s); g.ghn = d.p<GRUSB_GHN>(s); g.hprev = d.p<GRUSB_HPREV>(s); g.lens = reinterpret_cast<const int32_t*>(d.base<GRUSB_LENS>());
            g.G = const_cast<float*>(d.base<GRUSB_G>()); g.DGI = const_cast<float*>(d.base<GRUSB_DGI>()); g.dh0 = const_cast<float*>(d.base<GRUSB_DH0>());
            g.out_ts = d.w<RD_I + GRUSB_I_OUT_TS>(); g.out_ld = d.w<RD_I + GRUSB_I_OUT_LD>(); g.j = T - 1 - s; g.reverse = d.w<RD_I + GRUSB_I_REVERSE>();
            g.has_gemm = s >= 1; g.has_gates = s < T;
            const Out o{d.m<GRUSB_DGH>(s), ld3, false, d.m<GRUSB_DGH16>(s), n16};
            for (int tk = 0; tk < nt; ++tk) {
              const int trc = d.tile(tk);
              tile_gru_seq_bwd<NW, OT>(g, o, R, trc & 0xffff, (trc >> 16) * 16, B, red(), pl);
            }
          } break;
          case K_LSTMS: if constexpr (!ROLL) {
            const int ld3 = d.w<RD_LD + LD_OUT>(), n16 = d.w<RD_N16 + N16_OUT>();
            const int H = d.w<RD_I + LSTMS_I_H>();
            LstmSeqIn g;
            g.H16 = d.p<LSTMS_H16>(s); g.Whh = d.base<LSTMS_WHH>(); g.bhh = d.base<LSTMS_BHH>(); g.xg = d.p<LSTMS_XG>(s);
            g.lens = reinterpret_cast<const int32_t*>(d.base<LSTMS_LENS>()); g.hprev = d.p<LSTMS_HPREV>(s); g.cprev = d.p<LSTMS_CPREV>(s); g.cnext = d.m<LSTMS_CNEXT>(s);
            g.out = d.m<LSTMS_OUT>(s); g.gates = d.m<LSTMS_GATES>(s); g.t = s;
            const Out o{d.m<LSTMS_HNEXT>(s), ld3, false, d.m<LSTMS_HNEXT16>(s), n16};
            for (int tk = 0; tk < nt; ++tk) {
              const int trc = d.tile(tk);
              tile_lstm_seq<NW, OT>(g, o, H, trc & 0xffff, (trc >> 16) * 16, B, red(), pl);
            }
          } break;
          case K_LSTMSB: if constexpr (!ROLL) {
            const int ld3 = d.w<RD_LD + LD_OUT>(), n16 = d.w<RD_N16 + N16_OUT>();
            const int H = d.w<RD_I + LSTMSB_I_H>(), T = d.w<RD_N16 + LSTMSB_N16_T>();
            LstmSeqBwdIn g;
            g.DGn16 = d.p<LSTMSB_DG16_IN>(s); g.WhhT = d.base<LSTMSB_WHHT>(); g.dout = d.p<LSTMSB_DOUT>(s); g.gates = d.p<LSTMSB_GATES>(s); g.c_s = d.p<LSTMSB_CS>(s);
            g.c_s1 = g.c_s + (size_t)B * H; g.DC = const_cast<float*>(d.base<LSTMSB_DC>()); g.dh0 = const_cast<float*>(d.base<LSTMSB_DH0>()); g.has_gemm = s >= 1;
            g.has_gates = s < T;
            const Out o{d.m<LSTMSB_DG>(s), ld3, false, d.m<LSTMSB_DG16>(s), n16};
            for (int tk = 0; tk < nt; ++tk) {
              const int trc = d.tile(tk);
              tile_lstm_seq_bwd<NW, OT>(g, o, H, trc & 0xffff, (trc >> 16) * 16, B, red(), pl);
            }
          } break;
          case K_LSTM: if constexpr (ROLL) {
            const int ld3 = d.w<RD_LD + LD_OUT>(), n16 = d.w<RD_N16 + N16_OUT>();
            const Out o{d.m<LSTM_HRM>(s), ld3, false, d.m<LSTM_H16>(s), n16, d.m<LSTM_H16B>(s), d.w<RD_N16 + N16_OUTB>()};
            const int H = d.w<RD_I + LSTM_I_H>();
            for (int tk = 0; tk < nt; ++tk) {
              const int trc = d.tile(tk);
              tile_lstm<NW, OT>(d.p<LSTM_X16>(s), d.base<LSTM_WIH>(), K, d.base<LSTM_BIH>(), d.p<LSTM_GH>(s), d.p<LSTM_CPREV>(s), d.m<LSTM_CNEXT>(s), H, o, trc & 0xffff,
                                (trc >> 16) * 16, B, red(), pl);
            }
          } break;
          case K_DMOLS: {
            const int ld0 = d.w<RD_LD + DMOLS_LD_DEC>(), ld3 = d.w<RD_LD + LD_OUT>(), n16 = d.w<RD_N16 + N16_OUT>();
            const Out o{d.m<DMOLS_X>(s), ld3, false, d.m<DMOLS_X16>(s), n16};
            const int S = d.w<RD_I + DMOLS_I_S>(), F = d.w<RD_I + DMOLS_I_F>(), nmix = d.w<RD_I + DMOLS_I_NMIX>();
            for (int tk = 0; tk < nt; ++tk) {
              const int trc = d.tile(tk);
              // the head's fields are read at the draw (wave 0, after the product): nothing of them is live before
              tile_dmol_sample<NW>(d.p<DMOLS_DEC>(s), ld0, d.base<DMOLS_W>(), d.base<DMOLS_B>(), d.p<DMOLS_U>(s), d.p<DMOLS_V>(s), S, F, nmix,
                                   [&] { return DrawFields{d.w<RD_I + DMOLS_I_HEAD>(), d.f<DMOLS_F_LOG_EPS>(), d.f<DMOLS_F_SD_BETA>(), d.f<DMOLS_F_SD_EPS>()}; },
                                   o, trc & 0xffff, (trc >> 16) * 4, B, red0, pl);
            }
          } break;
          default: break;
        }
        if (profiled) {
          const unsigned long long now = wall_clock64();
          pacc[i] += now - tprev;
          tprev = now;
        }
      }
      d = nx;
    }
  }
  if (profiled) {
    for (int i = 0; i < a.ndesc; ++i) a.prof[(w == 0 ? 0 : 32) + i] += pacc[i];
#ifdef PCHAIN_TPROF
    if (w == 0) for (int l = 0; l < 8; ++l) a.prof[56 + l] += pl.tp[l];
#endif
#ifdef PCHAIN_TPROF2
    if (w == 0) for (int l = 0; l < 3; ++l) a.prof[60 + l] += tq[l];
    if (w == 0) for (int l = 3; l < 6; ++l) a.prof[70 + l] += tq[l];
#endif
  }
}

// The same walk on ROW GROUPS (pchain_rt.h): a tile is up to RT row tiles of one column tile, the program's tile lists count
// groups (rt = row groups here), and only the tile kinds of the VRNN programs exist.  A separate kernel on purpose: the 16-row
// kernel above is sensitive to every live scalar (tools/probe_engine_chain.py) and must not change when this one does.
template <int NW, int OT, int RT>
__global__ __launch_bounds__(NW * 64, 1) void pchain_rt_kernel(const int* __restrict__ tab, Hdr a) {
  extern __shared__ __attribute__((aligned(16))) char lds_all[];
  int* const ltab = reinterpret_cast<int*>(lds_all);
  float* const red0 = reinterpret_cast<float*>(lds_all + sizeof(int) * kDescWords * kMaxDesc + 32 * sizeof(unsigned long long));
  float* const red1 = red0 + a.lds_products * NW * 256;
  const int w = blockIdx.x, B = a.B, rt = ((B + 15) / 16 + RT - 1) / RT;  // row groups
  const bool xcd = a.xcd != 0;
  for (int e = threadIdx.x; e < a.ndesc * kDescWords; e += NW * 64) ltab[e] = tab[e];
  unsigned mine = 0;
  for (int i = 0; i < a.ndesc; ++i) {
    const int* q = tab + (size_t)i * kDescWords;
    if (TileIter(w, q[RD_WG0], q[RD_NWG], rt, q[RD_CT], xcd).valid()) mine |= 1u << i;
  }
  __syncthreads();
  if (threadIdx.x < a.ndesc) {
    int* q = ltab + threadIdx.x * kDescWords;
    int k = 0;
    for (TileIter it(w, q[RD_WG0], q[RD_NWG], rt, q[RD_CT], xcd); it.valid() && k < kMaxTilesPerWg; it.next()) q[RD_TILE + k++] = (it.r0() * RT) | (it.c() << 16);
    q[RD_NT] = k;
  }
  __syncthreads();
  if (mine == 0) return;
  int par = 0;
  auto red = [&]() { par ^= 1; return par ? red0 : red1; };
  Poll pl{a.ctl, 0u, false, 1};
  DescRegs d, nx;
  d.fetch(ltab, __builtin_ctz(mine), a.s0);
  for (int s = a.s0; s < a.S; ++s) {
    for (unsigned m = mine; m != 0; m &= m - 1) {
      const int i = __builtin_ctz(m);
      const unsigned rest = m & (m - 1);
      const int nx_i = __builtin_ctz(rest != 0 ? rest : mine), nx_s = rest != 0 ? s : s + 1;
      const int kind = d.w<RD_KIND>(), flags = d.w<RD_FLAGS>(), K = d.w<RD_K>();
      const bool active = s >= d.w<RD_SBEGIN>() && s < d.w<RD_SEND>();
      nx.fetch(ltab, nx_i, nx_s);
      if (active) {
        const int nt = d.w<RD_NT>();
        pl.nap = (flags & DF_GENTLE) ? 16 : 1;
        pl.code = ((unsigned)s << 4) | (unsigned)i;
        const int ld0 = d.w<RD_LD + LIN_LD_A>(), ld1 = d.w<RD_LD + LIN_LD_ADD>(), ld3 = d.w<RD_LD + LD_OUT>(), n16 = d.w<RD_N16 + N16_OUT>();
        static_assert(LIN_LD_A == GRU_LD_HPREV && LIN_LD_A == GRUB_LD_H && LIN_LD_ADD == DZ_LD_ADD && LIN_LD_ADD == GRUB_LD_GADD, "ld0, ld1: every kind's");
        switch (kind) {
          case K_LIN: {
            const bool a_polled = !(flags & DF_A_PLAIN);
            const float *A = d.p<LIN_A>(s), *W = d.base<LIN_W>();
            const float *A2 = (flags & DF_A_SUM3) ? d.p<LIN_A2>(s) : nullptr, *A3 = (flags & DF_A_SUM3) ? d.p<LIN_A3>(s) : nullptr;
            const int w_width = d.w<RD_I + LIN_I_W_WIDTH>();
            auto late = [&]() {
              return LinLate{d.base<LIN_BIAS>(), d.p<LIN_ADD>(s), d.p<LIN_GATE>(s), ld1, d.w<RD_LD + LIN_LD_GATE>(), (flags & DF_ADD_POLLED) != 0, (flags & DF_RELU) != 0,
                             d.f<LIN_F_SLOPE>(), Out{d.m<LIN_ORM>(s), ld3, (flags & DF_RM_SC1) != 0, d.m<LIN_O16>(s), n16, d.m<LIN_O16B>(s), d.w<RD_N16 + N16_OUTB>()}};
            };
            for (int tk = 0; tk < nt; ++tk) {
              const int trc = d.tile(tk), tr0 = trc & 0xffff, tc0 = (trc >> 16) * 16;
              if ((flags & DF_CANARY) && a_polled) {
                for (int q = 0; q < RT && tr0 + 16 * q < B; ++q) canary_wait(A, tr0 + 16 * q, K, pl, ld0);
              }
              tile_lin_rt<NW, OT, RT, 1>(A, ld0, a_polled, W, K, late, tr0, tc0, B, red, pl, A2, A3, w_width);
            }
          } break;
          case K_LINSEQ: {
            const int n = d.w<RD_I + LINSEQ_I_N>();
            const bool gated = (flags & DF_SEQ_GATE) != 0;
            const float* A = d.p<LINSEQ_A0>(s);
            const int K0 = d.w<RD_I + LINSEQ_I_K0>();  // the first link's own K (0: the run's), as in pchain_kernel
            for (int li = 0; li < n; ++li) {
              pl.code = ((unsigned)s << 4) | (unsigned)i | ((unsigned)li << 28);
              const float* W = d.basedyn(LINSEQ_W + li);
              const int Kl = (li == 0 && K0 != 0) ? K0 : K;
              auto late = [&]() {
                const float* aux = d.pdyn(LINSEQ_AUX + li);
                const float* add0 = li == 0 ? d.p<LINSEQ_ADD0>(s) : nullptr;
                return LinLate{gated ? nullptr : aux, add0, gated ? aux : nullptr, d.w<RD_I + LINSEQ_I_LD_ADD0>(), d.w<RD_I + LINSEQ_I_LD_GATE>(), false,
                               (flags & DF_RELU) != 0, d.f<LINSEQ_F_SLOPE>(), Out{const_cast<float*>(d.pdyn(LINSEQ_ORM + li)), d.wdyn(RD_LD + LINSEQ_LD_ORM + li),
                                                                                  false, const_cast<float*>(d.pdyn(LINSEQ_O16 + li)), n16}};
              };
              for (int tk = 0; tk < nt; ++tk) {
                const int trc = d.tile(tk), tr0 = trc & 0xffff, tc0 = (trc >> 16) * 16;
                tile_lin_rt<NW, OT, RT, 1>(A, 0, true, W, Kl, late, tr0, tc0, B, red, pl);
              }
              A = d.pdyn(LINSEQ_O16 + li);
            }
          } break;
          case K_HEAD: {
            const HeadOut o{d.m<HEAD_MU_P>(s), d.m<HEAD_SD_P>(s), d.m<HEAD_MU_Q>(s), d.m<HEAD_SD_Q>(s), d.m<HEAD_RAW_P>(s), d.m<HEAD_RAW_Q>(s), d.m<HEAD_MUQ_RAW>(s),
                            Out{d.m<HEAD_Z>(s), ld3, false, d.m<HEAD_Z16>(s), n16, d.m<HEAD_Z16B>(s), d.w<RD_N16 + N16_OUTB>()}};
            const int Z = d.w<RD_I + HEAD_I_Z>(), residual = d.w<RD_I + HEAD_I_RESIDUAL>();
            for (int tk = 0; tk < nt; ++tk) {
              const int trc = d.tile(tk);
              tile_head_rt<NW, OT, RT>(d.p<HEAD_P16>(s), d.p<HEAD_Q16>(s), true, d.base<HEAD_WP>(), d.base<HEAD_BP>(), d.base<HEAD_WQ>(), d.base<HEAD_BQ>(),
                                       d.p<HEAD_EPS>(s), o, K, Z, residual, d.f<HEAD_F_BETA>(), d.f<HEAD_F_INV_BETA>(), d.f<HEAD_F_SD_EPS>(), trc & 0xffff,
                                       (trc >> 16) * 16, B, red, pl);
            }
          } break;
          case K_GRU: {
            const Out o{d.m<GRU_HRM>(s), ld3, true, d.m<GRU_H16>(s), n16, d.m<GRU_H16B>(s), d.w<RD_N16 + N16_OUTB>()};
            const int R = d.w<RD_I + GRU_I_R>();
            for (int tk = 0; tk < nt; ++tk) {
              const int trc = d.tile(tk);
              tile_gru_rt<NW, OT, RT>(d.p<GRU_X16>(s), 0, true, d.base<GRU_WIH>(), K, d.p<GRU_XG>(s), d.base<GRU_BIH>(), d.p<GRU_GH>(s), d.p<GRU_HPREV>(s), ld0, R, o,
                                      d.m<GRU_RG>(s), d.m<GRU_UG>(s), d.m<GRU_NG>(s), trc & 0xffff, (trc >> 16) * 16, B, red, pl);
            }
          } break;
          case K_DZ: {
            DzIn z;
            z.mu_q = d.p<DZ_MU_Q>(s); z.sd_q = d.p<DZ_SD_Q>(s); z.mu_p = d.p<DZ_MU_P>(s); z.sd_p = d.p<DZ_SD_P>(s); z.eps = d.p<DZ_EPS>(s); z.raw_q = d.p<DZ_RAW_Q>(s);
            z.raw_p = d.p<DZ_RAW_P>(s); z.muq_raw = d.p<DZ_MUQ_RAW>(s); z.x_sl = reinterpret_cast<const int32_t*>(d.base<DZ_X_SL>()); z.c_raw = d.base<DZ_C_RAW>();
            z.c_fn = d.base<DZ_C_FN>(); z.t = d.w<RD_I + DZ_I_T0>() - s; z.stride = d.w<RD_I + DZ_I_STRIDE>(); z.residual = d.w<RD_I + DZ_I_RESIDUAL>();
            z.fn_floor = d.f<DZ_F_FN_FLOOR>(); z.beta = d.f<DZ_F_BETA>(); z.sd_eps = d.f<DZ_F_SD_EPS>(); z.has_gemm = s >= (int)d.f<DZ_F_GEMM_FROM>();
            const int Z = d.w<RD_I + DZ_I_Z>();
            const Out oq{d.m<DZ_DQH>(s), ld3, false, d.m<DZ_DQH16>(s), n16}, op{d.m<DZ_DPH>(s), ld3, false, d.m<DZ_DPH16>(s), n16};
            for (int tk = 0; tk < nt; ++tk) {
              const int trc = d.tile(tk);
              tile_dz_rt<NW, OT, RT>(d.p<DZ_D16>(s), d.base<DZ_WT>(), true, d.p<DZ_ADD>(s), ld1, (flags & DF_ADD_POLLED) != 0, z, oq, op, K, Z, trc & 0xffff,
                                     (trc >> 16) * 16, B, red, pl);
            }
          } break;
          case K_GRUB: {
            GrubIn g;
            g.D0 = d.p<GRUB_D0_16>(s); g.D1 = d.p<GRUB_D1_16>(s); g.W0 = d.base<GRUB_W0>(); g.W1 = d.base<GRUB_W1>(); g.g_in = d.p<GRUB_G_IN>(s);
            g.g_add = d.p<GRUB_G_ADD>(s); g.ld_gadd = ld1; g.rg = d.p<GRUB_RG>(s); g.ug = d.p<GRUB_UG>(s); g.ng = d.p<GRUB_NG>(s); g.gh = d.p<GRUB_GH>(s);
            g.hprev = d.p<GRUB_HPREV>(s); g.dd = d.p<GRUB_DD>(s); g.ldh = ld0; g.dgi = Out{d.m<GRUB_DGI>(s), ld3, false, d.m<GRUB_DGI16>(s), n16};
            g.dgh = Out{d.m<GRUB_DGH>(s), ld3, false, d.m<GRUB_DGH16>(s), n16}; g.ga = d.m<GRUB_GA>(s); g.g_out = const_cast<float*>(d.base<GRUB_G_OUT>());
            g.has_gemm = s >= d.w<RD_I + GRUB_I_GEMM_FROM>(); g.has_gates = s < d.w<RD_I + GRUB_I_GATES_TO>(); g.has_gin = s >= d.w<RD_I + GRUB_I_GIN_FROM>();
            const int R = d.w<RD_I + GRUB_I_R>();
            for (int tk = 0; tk < nt; ++tk) {
              const int trc = d.tile(tk);
              tile_grub_rt<NW, OT, RT>(g, K, R, trc & 0xffff, (trc >> 16) * 16, B, red, pl);
            }
          } break;
          default: break;
        }
      }
      d = nx;
    }
  }
}

__global__ void rows_to_t16_kernel(const float* src, int ld, int B, int K, float* dst, int n16, int k_src) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= B * K) return;
  const int row = i / K, k = i % K;
  dst[((size_t)(row >> 4) * n16 + (k >> 4)) * 256 + ((row & 15) + 16 * ((k & 15) >> 2)) * 4 + (k & 3)] = src && k < k_src ? src[(size_t)row * ld + k] : 0.f;
}

}  // namespace

int pchain_rows_to_t16(const float* src, int ld, int B, int K, float* dst, hipStream_t stream, int n16, int k_src) {
  BLVM_REQUIRE(B > 0 && K > 0 && K % 16 == 0 && dst != nullptr && (n16 == 0 || n16 >= K / 16) && k_src >= 0 && k_src <= K, "pchain_rows_to_t16: bad arguments");
  hipLaunchKernelGGL(rows_to_t16_kernel, dim3((B * K + 255) / 256), dim3(256), 0, stream, src, ld, B, K, dst, n16 > 0 ? n16 : K / 16, k_src > 0 ? k_src : K);
  BLVM_CHECK_LAUNCH("pchain_rows_to_t16");
  return BLVM_OK;
}

namespace {
__global__ __launch_bounds__(256) void fill_sentinel_kernel(unsigned* __restrict__ p, size_t n) {
  const size_t head = std::min<size_t>(n, ((16 - (reinterpret_cast<unsigned long long>(p) & 15)) & 15) / 4);  // words in front of the first 16-byte boundary
  uint4* const v = reinterpret_cast<uint4*>(p + head);
  const size_t nv = (n - head) / 4;
  const uint4 ff = make_uint4(pchain::SENTINEL, pchain::SENTINEL, pchain::SENTINEL, pchain::SENTINEL);
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < nv; i += (size_t)gridDim.x * 256) v[i] = ff;
  if (blockIdx.x == 0) {
    if (threadIdx.x < head) p[threadIdx.x] = pchain::SENTINEL;
    const size_t t0 = head + nv * 4;
    if (t0 + threadIdx.x < n) p[t0 + threadIdx.x] = pchain::SENTINEL;
  }
}
}  // namespace

hipError_t pchain_fill_sentinel(void* p, size_t bytes, hipStream_t stream) {
  if (bytes == 0) return hipSuccess;
  if ((reinterpret_cast<unsigned long long>(p) & 3) != 0 || (bytes & 3) != 0) return hipMemsetAsync(p, 0xFF, bytes, stream);
  const size_t n = bytes / 4;
  const unsigned grid = (unsigned)std::max<size_t>(1, std::min<size_t>((n / 4 + 255) / 256, 2048));
  hipLaunchKernelGGL(fill_sentinel_kernel, dim3(grid), dim3(256), 0, stream, static_cast<unsigned*>(p), n);
  return hipGetLastError();
}

int pchain_prepare(pchain::Builder& bld, const char* who) {
  BLVM_REQUIRE(!bld.overflow, "%s: persistent program overflow", who);
  return pchain_ctl(bld.p.ctl);
}

int pchain_run(const pchain::Program& prog, hipStream_t stream) {
  BLVM_REQUIRE(prog.ndesc > 0 && prog.ndesc <= pchain::kMaxDesc && prog.S > 0 && prog.B > 0, "pchain: bad program (%d descriptors, %d steps)", prog.ndesc, prog.S);
  int grid = 0;
  for (int i = 0; i < prog.ndesc; ++i) {
    const pchain::Desc& d = prog.d[i];
    BLVM_REQUIRE(d.nwg > 0 && d.wg0 >= 0 && d.ct > 0 && d.K > 0 && d.K % 16 == 0, "pchain: bad descriptor %d", i);
    BLVM_REQUIRE(!prog.xcd || d.nwg % 8 == 0, "pchain: XCD-aware placement needs ranges of 8 k workgroups (descriptor %d has %d)", i, d.nwg);
    grid = std::max(grid, d.wg0 + d.nwg);
    const int rt = ((prog.B + 15) / 16 + prog.rt_group - 1) / prog.rt_group;  // row tiles, or row groups
    const int per_wg = pchain::tiles_per_workgroup(rt, d.ct, d.nwg, prog.xcd != 0);
    BLVM_REQUIRE(per_wg <= kMaxTilesPerWg, "pchain: descriptor %d gives a workgroup %d tiles (at most %d)", i, per_wg, kMaxTilesPerWg);
  }
  int dev = 0, cus = 0;
  BLVM_HIP(hipGetDevice(&dev));
  BLVM_HIP(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
  BLVM_REQUIRE(grid <= cus, "pchain: the program names %d workgroups, the device has %d CUs (every workgroup must be resident)", grid, cus);
  // the resolved table: a slot of a small ring in library-owned device memory (launches on one stream are ordered; the ring keeps
  // launches that overlap on different streams apart)
  int* tab = nullptr;
  {
    static std::mutex mu;
    static int tab_dev = -1;
    static int* ring = nullptr;
    static unsigned next = 0;
    constexpr unsigned kSlots = 8;
    std::lock_guard<std::mutex> lock(mu);
    if (tab_dev != dev) {
      BLVM_HIP(hipMalloc(reinterpret_cast<void**>(&ring), sizeof(int) * kDescWords * pchain::kMaxDesc * kSlots));
      tab_dev = dev;
    }
    tab = ring + (size_t)(next++ % kSlots) * kDescWords * pchain::kMaxDesc;
  }
  for (int first = 0; first < prog.ndesc; first += kResolveChunk) {
    ProgramPart part;
    part.ndesc = std::min(kResolveChunk, prog.ndesc - first);
    part.first = first;
    for (int k = 0; k < 16; ++k) part.stride[k] = prog.stride[k];
    for (int k = 0; k < part.ndesc; ++k) part.d[k] = prog.d[first + k];
    hipLaunchKernelGGL(pchain_resolve_kernel, dim3(1), dim3(256), 0, stream, part, tab);
  }
  BLVM_REQUIRE(prog.s_first >= 0 && prog.s_first < prog.S, "pchain: empty step range [%d, %d)", prog.s_first, prog.S);
  Hdr h{prog.ndesc, prog.s_first, prog.S, prog.B, prog.xcd, prog.prof_wg, prog.lds_products, prog.ctl, prog.prof};
  const int nw = prog.rt_group > 1 ? 8 : 16;  // (the row-group kernel is built for 8 waves: 512 threads finish row-tile pairs)
  const size_t lds_fixed = sizeof(int) * kDescWords * pchain::kMaxDesc + 32 * sizeof(unsigned long long);
  const size_t lds = lds_fixed + sizeof(float) * 2 * (size_t)prog.lds_products * nw * 256;
  // the dynamic-LDS limit of the kernels is raised once per process and device (the call is far from free), and the launch's
  // residency — every workgroup of the grid must be on a CU at the same time — is checked against the occupancy the runtime
  // computes for this kernel, block size and LDS size (cached per kernel and number of products: a train step alternates sizes)
  constexpr int kMaxProducts = 8;
  static std::mutex attr_mu;
  static int attr_dev[7] = {-1, -1, -1, -1, -1, -1, -1};
  static int occ_blocks[7][kMaxProducts + 1];  // workgroups per CU; 0: not asked yet
  const size_t lds_max = lds_fixed + sizeof(float) * 2 * (prog.rt_group > 1 ? 8 : 4) * (size_t)nw * 256;  // (row groups reduce two row tiles per barrier)
  BLVM_REQUIRE(prog.lds_products >= 1 && lds <= lds_max, "pchain: %d products per tile do not fit the reduction scratch", prog.lds_products);
  auto go = [&](auto kernel, int slot, int threads) -> int {
    {
      std::lock_guard<std::mutex> lock(attr_mu);
      int* const occ = occ_blocks[slot];
      if (attr_dev[slot] != dev) {
        BLVM_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_max));
        attr_dev[slot] = dev;
        std::fill(occ, occ + kMaxProducts + 1, 0);
      }
      if (occ[prog.lds_products] == 0) BLVM_HIP(hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ[prog.lds_products], kernel, threads, lds));
      BLVM_REQUIRE((long)occ[prog.lds_products] * cus >= grid,
                   "pchain: %d workgroups of %d threads + %zu B LDS are not co-resident (%d per CU x %d CUs)", grid, threads, lds, occ[prog.lds_products], cus);
    }
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(threads), lds, stream, (const int*)tab, h);
    return BLVM_OK;
  };
  BLVM_REQUIRE(prog.rt_group == 1 || prog.rt_group == 2, "pchain: row groups of %d row tiles are not built", prog.rt_group);
  if (prog.rt_group > 1) {
    for (int i = 0; i < prog.ndesc; ++i) {
      const int k = prog.d[i].kind;
      BLVM_REQUIRE(k == pchain::K_LIN || k == pchain::K_LINSEQ || k == pchain::K_HEAD || k == pchain::K_GRU || k == pchain::K_DZ || k == pchain::K_GRUB,
                   "pchain: tile kind %d has no row-group form", k);
      BLVM_REQUIRE(k != pchain::K_DZ || prog.d[i].p[2] == nullptr, "pchain: the row-group dz tile is the single-product form");
      BLVM_REQUIRE(k != pchain::K_LIN || (prog.d[i].flags & (pchain::DF_ADD_EARLY | pchain::DF_ADD2_POLLED)) == 0,
                   "pchain: the row-group linear tile has one addend, polled behind its product");
    }
    BLVM_REQUIRE(prog.ot == OP_F32, "pchain: row groups multiply fp32 operands only");
    BLVM_TRY(go(&pchain_rt_kernel<8, OP_F32, 2>, 2, 512));
    BLVM_CHECK_LAUNCH("pchain_launch (row groups)");
    return BLVM_OK;
  }
  bool roll = false;
  for (int i = 0; i < prog.ndesc; ++i) roll |= prog.d[i].kind == pchain::K_LSTM;
  for (int i = 0; i < prog.ndesc; ++i)
    BLVM_REQUIRE(prog.d[i].kind != pchain::K_LIN || (prog.d[i].flags & (pchain::DF_ADD_EARLY | pchain::DF_ADD2_POLLED)) == 0 || (prog.ot == OP_F32 && !roll),
                 "pchain: an early or a second polled addend runs in the fp32 training kernel only");
  if (roll) {  // the roll-out's own instantiation
    for (int i = 0; i < prog.ndesc; ++i) {
      const int k = prog.d[i].kind;
      BLVM_REQUIRE(k == pchain::K_LIN || k == pchain::K_LINSEQ || k == pchain::K_LSTM || k == pchain::K_DMOLS, "pchain: tile kind %d is not part of the roll-out kernel", k);
    }
    BLVM_TRY(prog.ot == OP_BF16  ? go(&pchain_kernel<16, OP_BF16, true>, 5, 1024)
             : prog.ot == OP_F16 ? go(&pchain_kernel<16, OP_F16, true>, 6, 1024)
                                 : go(&pchain_kernel<16, OP_F32, true>, 4, 1024));
    BLVM_CHECK_LAUNCH("pchain_launch (roll-out)");
    return BLVM_OK;
  }
  BLVM_TRY(prog.ot == OP_BF16  ? go(&pchain_kernel<16, OP_BF16>, 1, 1024)
           : prog.ot == OP_F16 ? go(&pchain_kernel<16, OP_F16>, 3, 1024)
                               : go(&pchain_kernel<16, OP_F32>, 0, 1024));
  BLVM_CHECK_LAUNCH("pchain_launch");
  return BLVM_OK;
}

}  // namespace blvm

// Diagnostics / unit test of the engine: a chain of L links x_{s+1} = relu(x_s W^T + b), [B,N] x [N,N], as a one-descriptor program.
// x16: (L+1) T16 slabs [ceil(B/16)*16, N] — slab 0 must hold x_0 (pchain_rows_to_t16 / blvm_pchain_rows_to_t16), slabs 1..L are
// sentinel-filled here; xs: L row-major slabs [B,N] (outputs).  W in the T16 operand layout.
extern "C" int blvm_pchain_chain_probe(const float* W16, const float* bias, float* x16, float* xs, int B, int N, int L, int nwg, void* stream_) {
  using namespace blvm;
  using namespace blvm::pchain;
  hipStream_t s = static_cast<hipStream_t>(stream_);
  BLVM_REQUIRE(W16 && bias && x16 && xs && B > 0 && N > 0 && N % 16 == 0 && L > 0, "pchain_chain_probe: bad arguments");
  const int rt = (B + 15) / 16;
  const long x = (long)rt * 16 * N, sN = (long)B * N;
  Builder bld;
  bld.begin(OP_F32, L, B, 1, false, 1);
  static const int run = [] { const char* e = getenv("BLVM_PCHAIN_PROBE_RUN"); return e ? atoi(e) : 1; }();  // links per K_LINSEQ visit
  const int nw = nwg > 0 ? nwg : range_for((N / 16) * rt, device_cus() & ~7);
  if (run >= 2 && run <= 4 && L % run == 0) {  // the same chain as runs of `run` links in one descriptor visit
    bld.p.S = L / run;
    SeqLink lk[4];
    for (int i = 0; i < run; ++i) lk[i] = SeqLink{W16, bias, xs + (long)i * sN, run * sN, N, x16 + (long)(i + 1) * x};
    add_linseq(bld, N / 16, 0, nw, N, true, false, 0, L / run, {x16, run * x}, run, lk, 0, run * x, N / 16, 0.f, 0);
  } else {
    Operands o;
    o.p[LIN_A] = {x16, x}; o.p[LIN_W] = W16; o.p[LIN_BIAS] = bias; o.p[LIN_ORM] = {xs, sN}; o.p[LIN_O16] = {x16 + x, x}; o.ld[LD_OUT] = N; o.n16[N16_OUT] = N / 16;
    add_desc(bld, K_LIN, N / 16, 0, nw, N, DF_RELU, 0, L, o);
  }
  BLVM_HIP(pchain_fill_sentinel(x16 + x, sizeof(float) * (size_t)x * L, s));
  return pchain_launch(bld, "pchain_chain_probe", s);
}

extern "C" int blvm_pchain_rows_to_t16(const float* src, int ld, int B, int K, float* dst, void* stream) {
  return blvm::pchain_rows_to_t16(src, ld, B, K, dst, static_cast<hipStream_t>(stream));
}
