// gemm_ws.hip — K6, weight-stationary path: forward / data-gradient GEMMs C[M,N] = epi(A[M,K] · B) with K <= 256 and many rows.
//
// gemm_tile (gemm.hip) stages BOTH operands through LDS: per 16 k two barriers, 16 transposing ds_write_b32 and 32 ds_read_b32 per
// thread, at most three waves per SIMD.  With K <= 256 a 16-column slab of the weight is K / 4 <= 64 registers per lane as
// v_mfma_f32_16x16x4_f32 fragments, so here
//   * a wave loads its weight slab ONCE (op_b = 0, W[N,K]: one 16-byte load per 16 k; op_b = 1, W[K,N]: four 4-byte loads per 16 k)
//     and keeps it for its whole row range;
//   * the 8 waves of a workgroup own 8 neighbouring slabs (128 columns) and share the activations: the workgroup copies WS_RB
//     16-row blocks of A (whole rows, k-contiguous, 16 bytes per thread and load: full cache lines) into one of two LDS stages
//     while the other one is multiplied — one barrier per stage, no transposition;
//   * lane (i = lane & 15, q = lane >> 4) reads its fragments of a row as one ds_read_b128 per 16 k and feeds the four words to
//     four consecutive MFMAs.  The copy into LDS permutes every 16-k chunk (k = 4 j + x goes to slot 4 x + j) so that MFMA (c, e)
//     multiplies k = 16 c + 4 e .. + 3, lane row q holding k = 16 c + 4 e + q: every output is ONE fp32 fma chain in ascending k,
//     the chain gemm_tile runs on v_mfma_f32_32x32x2_f32.  Results are bit-identical to gemm_tile's (measured on every shape of
//     the table at gemm_ws_route; tests/test_gpu_gemm_ws.py), so routing a product here changes no result anywhere.
//     The LDS row stride is K + 8 floats: with a stride of 8 mod 16 floats the 16-byte slot of lane (i, q) is 2 i + q mod 16,
//     distinct within each of the instruction's four 16-lane groups (rows {0-3, 12-15} of one q with rows {4-11} of the next).
//   * the two blocks of a stage are multiplied together, their MFMAs alternating: two independent chains per wave (a dependent MFMA
//     issues every 40 cycles, an independent one every 32).
// The weight is the MFMA's first operand, so a lane ends up with four CONSECUTIVE columns of one output row: C[r0 + i][n0 + 4 q ..
// + 3] is one 16-byte store (and the gate one 16-byte load).  No atomics, no split.
// Two forms were measured before this one and are recorded at gemm_ws_route: A streamed from global memory straight into the
// fragments (no LDS) lost to gemm_tile; the k order of the 16-byte loads with two accumulators per output was 3-8 % faster than this
// form on the wide outputs but not bit-identical to gemm_tile, and CW-VAE's ill-conditioned C4 parity test moved past its bound.
#include <atomic>

#include "common.h"

namespace blvm {

namespace {

constexpr int WS_WAVES = 8;  // per workgroup = 2 per SIMD (16 waves = 128 registers each: the K = 256 form spills)
constexpr int WS_RB = 2;     // 16-row blocks per LDS stage
constexpr int WS_THREADS = WS_WAVES * 64;

struct WsArgs {
  const float* A;
  const float* B;
  float* C;
  const float* bias;
  const float* gate;
  int M, N, lda, ldb, ldc, ldg;
  int act;
  float slope;
  int accumulate;
  int ncg, nranges, stages_per_range;  // column groups of 8 slabs; row ranges of stages_per_range stages each
  int b_vec, c_vec, g_vec;             // 16-byte accesses allowed: B rows (op_b = 0), C rows, gate rows
};

// a and b exchange 16-lane rows: rows 1 and 3 of a with rows 0 and 2 of b (swap16), rows 2-3 of a with rows 0-1 of b (swap32).
// Written as assembly: through __builtin_amdgcn_permlane16_swap / 32_swap this compiler folded the four results of a chunk into
// copies of one register.  The s_nop is the two wait states a swap needs behind a VALU write of its operands (the compiler does not
// see into the string).
__device__ __forceinline__ void lane_swap16(float& a, float& b) {
  asm volatile("s_nop 1\n\tv_permlane16_swap_b32 %0, %1" : "+v"(a), "+v"(b));
}
__device__ __forceinline__ void lane_swap32(float& a, float& b) {
  asm volatile("s_nop 1\n\tv_permlane32_swap_b32 %0, %1" : "+v"(a), "+v"(b));
}

// NC = K / 16 (1 .. 16); OPB as gemm_f32's op_b
template <int NC, int OPB>
__global__ __launch_bounds__(WS_THREADS) __attribute__((amdgpu_waves_per_eu(2, 2))) void gemm_ws_kernel(WsArgs g) {
  constexpr int K = 16 * NC, S = K + 8, ROWS = 16 * WS_RB;
  constexpr int ITEMS = ROWS * (K / 4);  // 16-byte pieces of a stage
  constexpr int NV = (ITEMS + WS_THREADS - 1) / WS_THREADS;
  __shared__ __attribute__((aligned(16))) float lds[2][ROWS * S];

  const int tid = threadIdx.x, lane = tid & 63, i = lane & 15, q = lane >> 4;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int cg = blockIdx.x % g.ncg, range = blockIdx.x / g.ncg;
  const int slab = cg * WS_WAVES + wave;
  const bool active = slab * 16 < g.N;  // (a spare wave of the last column group only helps with the copies)
  const int n0 = slab * 16;

  const int nblocks = (g.M + 15) >> 4, nstages = (nblocks + WS_RB - 1) / WS_RB;
  const int s0 = range * g.stages_per_range, s1 = min(nstages, s0 + g.stages_per_range);

  // global -> registers -> LDS: piece id = (row, 4 k) of the stage; rows past M are copies of row M - 1 (valid memory, never stored)
  f32x4 r[NV];
  auto gload = [&](int st) {
#pragma unroll
    for (int v = 0; v < NV; ++v) {
      const int id = tid + v * WS_THREADS;
      if (ITEMS % WS_THREADS == 0 || id < ITEMS) {
        const int row = id / (K / 4), c4 = id % (K / 4);
        r[v] = *reinterpret_cast<const f32x4*>(g.A + (size_t)min(st * ROWS + row, g.M - 1) * g.lda + 4 * c4);
      }
    }
  };
  auto swrite = [&](float* dst) {
#pragma unroll
    for (int v = 0; v < NV; ++v) {
      const int id = tid + v * WS_THREADS;
      if (ITEMS % WS_THREADS == 0 || id < ITEMS) {
        const int j = id % (K / 4);  // k = 4 j + x goes to slot 4 x + j % 4 of its 16-k chunk: a lane's 16-byte read is k = 4 e + q
        float* d = dst + (id / (K / 4)) * S + 16 * (j >> 2) + (j & 3);
#pragma unroll
        for (int x = 0; x < 4; ++x) d[4 * x] = r[v][x];
      }
    }
  };

  gload(s0);  // in flight beside the weight loads

  // the weight slab: lane (i, q) holds W'(k = 16 c + 4 e + q, n = n0 + i) in w[c][e] (MFMA (c, e) multiplies k = 16 c + 4 e .. + 3)
  f32x4 w[NC];
  f32x4 bv = {0.f, 0.f, 0.f, 0.f};
  const int nq = n0 + 4 * q;  // this lane's four output columns
  if (active) {
    if (OPB == 0 && g.b_vec) {
      // 16-byte loads give lane (i, q) the words k = 16 c + 4 q + x; a 4 x 4 transposition across the four lanes of a row (x <-> q:
      // two v_permlane16_swap and two v_permlane32_swap per chunk) turns them into k = 16 c + 4 e + q.  (64 strided 4-byte loads
      // instead, 16 cache lines each, cost every launch 10 us.)
      const float* wp = g.B + (size_t)(n0 + i) * g.ldb + 4 * q;
#pragma unroll
      for (int c = 0; c < NC; ++c) {
        const f32x4 t = *reinterpret_cast<const f32x4*>(wp + 16 * c);
        float t0 = t[0], t1 = t[1], t2 = t[2], t3 = t[3];
        lane_swap16(t0, t1);
        lane_swap16(t2, t3);
        lane_swap32(t0, t2);
        lane_swap32(t1, t3);
        w[c] = f32x4{t0, t1, t2, t3};
      }
    } else {
      const float* wp = OPB == 0 ? g.B + (size_t)(n0 + i) * g.ldb + q : g.B + (size_t)q * g.ldb + n0 + i;
      const size_t ks = OPB == 0 ? 1 : (size_t)g.ldb;  // stride of k
#pragma unroll
      for (int c = 0; c < NC; ++c)
#pragma unroll
        for (int e = 0; e < 4; ++e) w[c][e] = wp[(size_t)(16 * c + 4 * e) * ks];
    }
    if (g.bias != nullptr) {
#pragma unroll
      for (int e = 0; e < 4; ++e) bv[e] = g.bias[nq + e];
    }
  } else {
#pragma unroll
    for (int c = 0; c < NC; ++c) w[c] = bv;
  }

  // One stage = WS_RB blocks.  Order of a stage (pinned with sched_barrier; left alone, the compiler interleaves reads and MFMAs
  // pairwise to save registers and every pair exposes an LDS round trip):
  //   the next stage's global loads and the epilogue operands of every block (gate, C under accumulate) are requested first;
  //   block s + 1 is read from LDS into a second register set while block s is multiplied;
  //   the next stage goes to LDS after the first block's MFMAs and BEFORE the first store: vmcnt counts loads and stores in one
  //   order, so behind a store the wait for those loads would also wait for the store's round trip.
  // D: row (4 q + reg) of the MFMA's first operand = column nq + reg, column i of the second = row b * 16 + i.
  auto lds_read = [&](f32x4 (&a)[NC], const float* src) {
    const float* ap = src + i * S + 4 * q;
#pragma unroll
    for (int c = 0; c < NC; ++c) a[c] = *reinterpret_cast<const f32x4*>(ap + 16 * c);
  };
  auto epilogue = [&](f32x4 v, f32x4 gt, f32x4 cv, float* cp, bool ok) {
    v += bv;
    if (g.act == 1) {
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] = v[e] > 0.f ? v[e] : 0.f;
    } else if (g.act == 2) {
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] = v[e] > 0.f ? v[e] : v[e] * g.slope;
    }
    if (g.gate != nullptr) {
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] *= gt[e] > 0.f ? 1.f : g.slope;
    }
    if (g.accumulate) v += cv;
    if (!ok) return;
    if (g.c_vec) *reinterpret_cast<f32x4*>(cp) = v;
    else {
#pragma unroll
      for (int e = 0; e < 4; ++e) cp[e] = v[e];
    }
  };

  swrite(lds[0]);
  __syncthreads();
  for (int st = s0; st < s1; ++st) {
    const float* cur = lds[(st - s0) & 1];
    float* nxt = lds[((st - s0) & 1) ^ 1];  // (every wave left that stage at the previous barrier)
    gload(min(st + 1, nstages - 1));        // (past the range: a valid stage that nobody reads)
    if (active) {
      f32x4 gt[WS_RB], cv[WS_RB], a[WS_RB][NC], acc[WS_RB];
      float* cp[WS_RB];
      bool ok[WS_RB];
#pragma unroll
      for (int s = 0; s < WS_RB; ++s) {
        const int m = (st * WS_RB + s) * 16 + i;
        ok[s] = m < g.M;  // (a block past the last one: every row is)
        cp[s] = g.C + (size_t)(ok[s] ? m : 0) * g.ldc + nq;
        gt[s] = cv[s] = bv;
        if (g.gate != nullptr && ok[s]) {
          const float* gp = g.gate + (size_t)m * g.ldg + nq;
          if (g.g_vec) gt[s] = *reinterpret_cast<const f32x4*>(gp);
          else {
#pragma unroll
            for (int e = 0; e < 4; ++e) gt[s][e] = gp[e];
          }
        }
        if (g.accumulate && ok[s]) {
          if (g.c_vec) cv[s] = *reinterpret_cast<const f32x4*>(cp[s]);
          else {
#pragma unroll
            for (int e = 0; e < 4; ++e) cv[s][e] = cp[s][e];
          }
        }
      }
#pragma unroll
      for (int s = 0; s < WS_RB; ++s) {
        lds_read(a[s], cur + s * 16 * S);
        acc[s] = f32x4{0.f, 0.f, 0.f, 0.f};
      }
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int c = 0; c < NC; ++c)
#pragma unroll
        for (int e = 0; e < 4; ++e)
#pragma unroll
          for (int s = 0; s < WS_RB; ++s) acc[s] = __builtin_amdgcn_mfma_f32_16x16x4f32(w[c][e], a[s][c][e], acc[s], 0, 0, 0);
      __builtin_amdgcn_sched_barrier(0);
      swrite(nxt);
#pragma unroll
      for (int s = 0; s < WS_RB; ++s) epilogue(acc[s], gt[s], cv[s], cp[s], ok[s]);
    } else {
      swrite(nxt);
    }
    __syncthreads();
  }
}

std::atomic<unsigned long long> g_path_count[2];  // launches of gemm_f32: [0] staged tiles (gemm.hip), [1] this path
// Row threshold: the smallest row count measured; the path won there as well (table at gemm_ws_route), fewer rows were not measured
// and stay on the staged tiles.
constexpr int kWsMinRowsDefault = 256;
std::atomic<int> g_ws_min_rows{kWsMinRowsDefault};

int cu_count() {
  static const int cus = [] {
    int dev = 0, n = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) n = 0;
    return n > 0 ? n : 256;
  }();
  return cus;
}

template <int OPB>
void launch_ws(int nc, const WsArgs& g, dim3 grid, hipStream_t s) {
#define WS_CASE(n) case n: hipLaunchKernelGGL((gemm_ws_kernel<n, OPB>), grid, dim3(WS_THREADS), 0, s, g); gemm_count_arm(ARM_WS); break;
  switch (nc) {
    WS_CASE(1) WS_CASE(2) WS_CASE(3) WS_CASE(4) WS_CASE(5) WS_CASE(6) WS_CASE(7) WS_CASE(8)
    WS_CASE(9) WS_CASE(10) WS_CASE(11) WS_CASE(12) WS_CASE(13) WS_CASE(14) WS_CASE(15) WS_CASE(16)
  }
#undef WS_CASE
}

}  // namespace

void gemm_count_path(int path) { g_path_count[path != 0].fetch_add(1, std::memory_order_relaxed); }
int gemm_ws_min_rows() { return g_ws_min_rows.load(std::memory_order_relaxed); }

// Which products of gemm_f32 run here.  Measured on MI355X with tools/gemm_bench.py ws (one library, both paths; 10 warm-up launches,
// operand sets rotated so that no launch finds A or C in the Infinity Cache; us per launch, gemm_tile -> this path, and TF/s):
//   VRNN [64, 16000], rows = 16 000                              op_b  N x K       epilogue
//     enc L1 forward                                              0     256 x 64   bias, leaky     14.6 ->   11.8    36 ->  44
//     enc L2 / L3, dec L2 forward                                 0     256 x 256  bias, leaky     31.6 ->   29.4    66 ->  71
//     XQ forward                                                  0     256 x 256  -               30.7 ->   28.4    68 ->  74
//     XG forward                                                  0    1536 x 256  -              145.2 ->  119.7    87 -> 105
//     dec L3 forward                                              0    1920 x 256  -              186.1 ->  145.5    85 -> 108
//     dec L2, enc L3, enc L2 data gradient                        1     256 x 256  gate            41.9 ->   31.6    50 ->  66
//     d_enc from DQ0                                              1     256 x 256  accumulate      39.2 ->   24.8    54 ->  85
//     dec L1 data gradient                                        1     768 x 256  -               74.2 ->   59.7    85 -> 105
//   CW-VAE C4, rows = 398 848
//     1x1 C -> 4C forward                                         0     768 x 192  bias, leaky   1270   -> 1066      93 -> 110
//     1x1 4C -> C data gradient                                   1     768 x 192  gate          2011   -> 1096      59 -> 107
//   fewer rows (256 x 256 forward, bias, leaky): 4096 rows 12.5 -> 12.3, 1024 rows 11.5 -> 10.6, 256 rows 11.4 -> 10.2;
//     1024 rows 1536 x 256 17.3 -> 16.5, 1024 rows 256 x 64 6.6 -> 5.7
// No measured shape lost to gemm_tile.  What lost, on the eight VRNN rows and the two CW-VAE rows above:
//   A streamed from global memory into the fragments by every wave (each load touches 16 rows x 64 bytes and all 8 waves of a
//   workgroup repeat it: the L1 sets the pace): 15.9 / 44.0 / 42.8 / 198.3 / 238.0 / 42.6 / 43.3 / 103.2, 1795 / 2026 us;
//   this form with the weights fetched by 64 strided 4-byte loads per lane instead of 16-byte loads + lane swaps: 14.4 / 42.2 /
//   40.2 / 145.2 / 174.2 / 25.7 / 26.7 / 67.7 us (10 us per op_b = 0 launch).
//   Not a loss in time: the 16-byte k order with two accumulators per output, 11.9 / 28.0 / 26.4 / 115.9 / 138.6 / 24.7 / 24.6 /
//   58.1, 1053 / 1130 us — dropped for bit-identity with gemm_tile (see the head of this file).
bool gemm_ws_route(int op_a, int M, int N, int K, uintptr_t a_addr, int lda, int split_k, bool has_colsum, int operand, int min_rows) {
  return operand == OP_F32 && op_a == 0 && split_k == 1 && !has_colsum && K > 0 && K % 16 == 0 && K <= 256 && N > 0 && N % 16 == 0 &&
         (a_addr & 15u) == 0 && lda % 4 == 0 && M >= min_rows && M >= 1;
}

int gemm_ws_f32(int op_b, int M, int N, int K, const float* A, int lda, const float* B, int ldb, float* C, int ldc, const float* bias,
                int act, float slope, const float* gate, int ldg, int accumulate, hipStream_t stream) {
  BLVM_REQUIRE(M <= INT_MAX - 16 * WS_RB, "gemm: too many rows");
  WsArgs g;
  g.A = A; g.B = B; g.C = C; g.bias = bias; g.gate = gate;
  g.M = M; g.N = N; g.lda = lda; g.ldb = ldb; g.ldc = ldc; g.ldg = ldg;
  g.act = act; g.slope = slope; g.accumulate = accumulate;
  g.b_vec = aligned16(B) && ldb % 4 == 0;
  g.c_vec = aligned16(C) && ldc % 4 == 0;
  g.g_vec = gate != nullptr && aligned16(gate) && ldg % 4 == 0;
  // one workgroup per (column group of 8 slabs, row range); as many row ranges as give every CU one workgroup (its 8 waves are
  // the 2 per SIMD that the registers allow)
  const int nstages = ((M + 15) / 16 + WS_RB - 1) / WS_RB;
  g.ncg = (N / 16 + WS_WAVES - 1) / WS_WAVES;
  const long nranges = std::max(1L, std::min<long>(nstages, cu_count() / g.ncg));
  g.stages_per_range = (int)((nstages + nranges - 1) / nranges);
  g.nranges = (nstages + g.stages_per_range - 1) / g.stages_per_range;
  const long groups = (long)g.ncg * g.nranges;
  BLVM_REQUIRE(groups < (1L << 31) - 1, "gemm: grid too large");
  const dim3 grid((unsigned)groups);
  if (op_b == 0) launch_ws<0>(K / 16, g, grid, stream);
  else launch_ws<1>(K / 16, g, grid, stream);
  BLVM_CHECK_LAUNCH("gemm_f32");
  return BLVM_OK;
}

}  // namespace blvm

extern "C" int blvm_gemm_path_counts(unsigned long long* out) {
  BLVM_REQUIRE(out != nullptr, "blvm_gemm_path_counts: null pointer");
  for (int p = 0; p < 2; ++p) out[p] = blvm::g_path_count[p].load(std::memory_order_relaxed);
  return BLVM_OK;
}

extern "C" int blvm_gemm_ws_min_rows(int rows) {
  return blvm::g_ws_min_rows.exchange(rows < 0 ? blvm::kWsMinRowsDefault : rows, std::memory_order_relaxed);
}

extern "C" int blvm_gemm_ws_route(int op_a, int M, int N, int K, size_t a_addr, int lda, int split_k, int has_colsum, int operand,
                                  int min_rows) {
  return blvm::gemm_ws_route(op_a, M, N, K, (uintptr_t)a_addr, lda, split_k, has_colsum != 0, operand, min_rows) ? 1 : 0;
}
