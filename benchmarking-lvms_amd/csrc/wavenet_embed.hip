// wavenet_embed.hip — K10e: the embedded class input of WaveNet, fused with its grouped causal convolution.
//
// The reference's WaveNet(embedding_dim=E, num_bins=V) feeds sample classes through nn.Embedding(V, E) and a causal convolution of
// kernel size 2 with groups = C (blvm/models/wavenet/wavenet.py:105-113,182): output channel o reads the m = E / C embedding columns
// o m .. o m + m - 1 only.  Both collapse into two lookup tables [V, C]:
//
//   P_tap[k][o]  = sum_{j<m} cw[o, j, tap] * Emb[k, o m + j]                (summed in index order)
//   out[t, b, o] = (P_0[k[t, b]][o] + P_1[k[t+1, b]][o]) + bias[o]
//
// so the front is a gather with no [T, B, E] tensor in memory, and in the decoder (wavenet_decode.hip) two table rows per frame.  The
// reference pads AFTER embedding, so a left-padded frame is a zero row: row V of either table, which every index outside [0, V) reads.
//
// Backward: G_0[k] = sum of d_out[t] over frames with k[t] = k, G_1[k] the same over k[t+1] = k; then
//   dEmb[k, o m + j] = cw[o,j,0] G_0[k,o] + cw[o,j,1] G_1[k,o]       dcw[o,j,tap] = sum_k G_tap[k,o] Emb[k, o m + j]      db = sum d_out.
// No float atomics (two calls agree to the bit) and no one-hot: the caller hands in a stable sort of the flattened classes; fixed
// chunks of the sorted frame list are summed into partial rows (one workgroup per chunk, whatever the class sizes: a class that holds
// most frames is spread over its chunks), and a second pass adds each class's partials in chunk order.
#include "common.h"

namespace blvm {
namespace {

constexpr int EMB_CHUNK = 128;            // sorted frames per partial row
constexpr int EMB_KCHUNK = 128;           // classes per partial of the dcw reduction
constexpr int EMB_LDS_BYTES = 32 * 1024;  // tables up to this size are gathered from LDS (five workgroups still share a CU)

__global__ __launch_bounds__(256) void embed_tables_kernel(const float* __restrict__ emb, const float* __restrict__ cw, int V, int C, int m,
                                                           float* __restrict__ P) {
  const size_t per_tap = (size_t)(V + 1) * C, n = 2 * per_tap;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
    const int tap = i >= per_tap;
    const size_t r = i - tap * per_tap;
    const int k = (int)(r / C), o = (int)(r - (size_t)k * C);
    float s = 0.f;
    if (k < V)
      for (int j = 0; j < m; ++j) s += cw[((size_t)o * m + j) * 2 + tap] * emb[(size_t)k * C * m + (size_t)o * m + j];
    P[i] = s;
  }
}

// 16 bytes per lane; LDS: the tables are copied to LDS once per workgroup (a persistent grid), else gathered from global memory (L2)
template <bool LDS>
__global__ __launch_bounds__(256) void embed_front_kernel(const float4* __restrict__ P, const float4* __restrict__ bias,
                                                          const int32_t* __restrict__ k, size_t rows, int B, int V, int c4,
                                                          float4* __restrict__ out) {
  extern __shared__ __align__(16) float4 sP[];
  const float4* tab = P;
  const size_t per_tap = (size_t)(V + 1) * c4;
  if constexpr (LDS) {
    for (size_t i = threadIdx.x; i < 2 * per_tap; i += 256) sP[i] = P[i];
    __syncthreads();
    tab = sP;
  }
  const size_t n4 = rows * c4;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (size_t)gridDim.x * 256) {
    const size_t row = i / c4;
    const int q = (int)(i - row * c4);
    int k0 = k[row], k1 = k[row + B];
    k0 = (unsigned)k0 < (unsigned)V ? k0 : V;
    k1 = (unsigned)k1 < (unsigned)V ? k1 : V;
    const float4 a = tab[(size_t)k0 * c4 + q], b = tab[per_tap + (size_t)k1 * c4 + q], c = bias[q];
    out[i] = make_float4((a.x + b.x) + c.x, (a.y + b.y) + c.y, (a.z + b.z) + c.z, (a.w + b.w) + c.w);
  }
}

// Pass 1.  Workgroup c sums the sorted frames [c CH, (c+1) CH) per class run: thread (tap, o) walks the chunk; sorted entry i is input
// frame f = perm[i] (f = tau B + b), which feeds d_out[f] into G_0 (tau < L_out) and d_out[f - B] into G_1 (tau >= 1).  The run that
// starts the chunk goes to parts[c][0], a later run that ends it to parts[c][1]; a run strictly inside is a whole class: straight to G.
// csum[c] = the chunk's tap-0 total over all its runs (every d_out row is in exactly one chunk: db).
__global__ __launch_bounds__(256) void embed_chunk_sums_kernel(const float* __restrict__ d_out, const int32_t* __restrict__ skeys,
                                                               const int32_t* __restrict__ perm, int n, int B, size_t rows, int C, int V,
                                                               float* __restrict__ G, float* __restrict__ parts, float* __restrict__ csum) {
  constexpr int U = 4;
  const int c = blockIdx.x, lo = c * EMB_CHUNK, hi = min(n, lo + EMB_CHUNK);
  for (int e = threadIdx.x; e < 2 * C; e += 256) {
    const int tap = e >= C, o = e - tap * C;
    auto flush = [&](int key, int s, int end, float acc) {
      if (s == lo) parts[(((size_t)c * 2 + 0) * 2 + tap) * C + o] = acc;
      else if (end == hi) parts[(((size_t)c * 2 + 1) * 2 + tap) * C + o] = acc;
      else if ((unsigned)key < (unsigned)V) G[((size_t)tap * V + key) * C + o] = acc;
    };
    float acc = 0.f, total = 0.f;
    int start = lo, cur = skeys[lo];
    for (int i = lo; i < hi; i += U) {
      int key[U];
      float val[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const bool ok = i + u < hi;
        key[u] = ok ? skeys[i + u] : cur;
        const int f = ok ? perm[i + u] : 0;
        const bool valid = ok && (unsigned)f < (unsigned)n && (tap ? f >= B : (size_t)f < rows);
        val[u] = valid ? d_out[((size_t)f - (size_t)(tap ? B : 0)) * C + o] : 0.f;
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        if (i + u < hi) {
          if (key[u] != cur) {
            flush(cur, start, i + u, acc);
            acc = 0.f; start = i + u; cur = key[u];
          }
          acc += val[u];
          total += val[u];
        }
      }
    }
    flush(cur, start, hi, acc);
    if (tap == 0) csum[(size_t)c * C + o] = total;
  }
}

// Pass 2.  Thread (tap, class, o): the class's sorted range is [starts[k], starts[k+1]); its partials are added in chunk order.  A
// class with no frame gets an exact zero; one strictly inside a single chunk was written by pass 1.
__global__ __launch_bounds__(256) void embed_class_sums_kernel(const int32_t* __restrict__ starts, int n, int C, int V,
                                                               const float* __restrict__ parts, float* __restrict__ G) {
  const size_t total = (size_t)2 * V * C;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
    const int o = (int)(i % C);
    const size_t r = i / C;
    const int tap = r >= (size_t)V, k = (int)(r - (size_t)tap * V);
    const int S = starts[k], E = starts[k + 1];
    if (S >= E || S < 0 || E > n) { G[i] = 0.f; continue; }
    const int c0 = S / EMB_CHUNK, c1 = (E - 1) / EMB_CHUNK;
    const int lo = c0 * EMB_CHUNK, hi = min(n, lo + EMB_CHUNK);
    const size_t row = (size_t)4 * C;  // floats per chunk: (opening | closing run) x tap x C
    const float* p = parts + (size_t)c0 * row + (size_t)tap * C + o;
    float acc;
    if (S == lo) acc = p[0];
    else if (E >= hi) acc = p[2 * C];
    else continue;  // strictly inside chunk c0: pass 1 wrote G
    // every later chunk opens with this class: a branch-free walk, so a class that holds most frames (silence) streams its partials
#pragma unroll 8
    for (int c = c0 + 1; c <= c1; ++c) acc += p[(size_t)(c - c0) * row];
    G[i] = acc;
  }
}

// db[o] = the chunk totals added in a fixed order: group g of the workgroup takes chunks g, g + NG, ...; the groups are added in order
__global__ __launch_bounds__(1024) void embed_bias_grad_kernel(const float* __restrict__ csum, int n_chunks, int C, float* __restrict__ db) {
  __shared__ float part[1024];
  const int NG = 1024 / C, g = threadIdx.x / C, o = threadIdx.x - g * C;
  float s = 0.f;
  if (g < NG)
    for (int c = g; c < n_chunks; c += NG) s += csum[(size_t)c * C + o];
  part[threadIdx.x] = s;
  __syncthreads();
  if (threadIdx.x < C) {
    float t = 0.f;
    for (int j = 0; j < NG; ++j) t += part[j * C + threadIdx.x];
    db[threadIdx.x] = t;
  }
}

__global__ __launch_bounds__(256) void embed_table_grad_kernel(const float* __restrict__ G, const float* __restrict__ cw, int V, int C, int m,
                                                               float* __restrict__ dE) {
  const int E = C * m;
  const size_t total = (size_t)V * E;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
    const size_t k = i / E;
    const int e = (int)(i - k * E), o = e / m;
    dE[i] = cw[2 * e] * G[k * C + o] + cw[2 * e + 1] * G[((size_t)V + k) * C + o];
  }
}

// dcw, stage 1: workgroup kb sums classes [kb KC, (kb+1) KC) for every (tap, e) -> wpart[kb][e][tap]
__global__ __launch_bounds__(256) void embed_conv_grad_parts_kernel(const float* __restrict__ G, const float* __restrict__ emb, int V, int C,
                                                                    int m, float* __restrict__ wpart) {
  const int E = C * m, k0 = blockIdx.x * EMB_KCHUNK, k1 = min(V, k0 + EMB_KCHUNK);
  for (int t = threadIdx.x; t < 2 * E; t += 256) {
    const int tap = t >= E, e = t - tap * E, o = e / m;
    float s = 0.f;
#pragma unroll 4
    for (int k = k0; k < k1; ++k) s += G[((size_t)tap * V + k) * C + o] * emb[(size_t)k * E + e];
    wpart[(size_t)blockIdx.x * 2 * E + 2 * e + tap] = s;
  }
}

// stage 2: the partials in order
__global__ __launch_bounds__(256) void embed_conv_grad_kernel(const float* __restrict__ wpart, int n_parts, int E2, float* __restrict__ dcw) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= E2) return;
  float s = 0.f;
  for (int p = 0; p < n_parts; ++p) s += wpart[(size_t)p * E2 + i];
  dcw[i] = s;
}

inline unsigned grid_for(size_t items, unsigned cap = 2048) {
  const size_t b = (items + 255) / 256;
  return (unsigned)(b < 1 ? 1 : (b > cap ? cap : b));
}

struct EmbedBwdSpace {
  size_t parts, csum, wpart, total;
};
inline EmbedBwdSpace embed_bwd_space(int n, int V, int C, int m) {
  const size_t n_chunks = ((size_t)n + EMB_CHUNK - 1) / EMB_CHUNK, n_kparts = ((size_t)V + EMB_KCHUNK - 1) / EMB_KCHUNK;
  Arena a;
  EmbedBwdSpace s;
  s.parts = a.take_off(n_chunks * 4 * C);
  s.csum = a.take_off(n_chunks * C);
  s.wpart = a.take_off(n_kparts * 2 * C * m);
  s.total = a.floats();
  return s;
}

int embed_shape_ok(const char* who, int V, int C, int m) {
  BLVM_REQUIRE(V > 0 && C > 0 && m > 0 && C % 4 == 0 && C <= 1024, "%s: need V > 0, m > 0, C a multiple of 4 up to 1024 (V %d, C %d, m %d)", who, V, C, m);
  BLVM_REQUIRE((size_t)2 * (V + 1) * C < (1ull << 31), "%s: tables of 2 (V + 1) C = 2 * %d * %d floats are too large", who, V + 1, C);
  return BLVM_OK;
}

}  // namespace
}  // namespace blvm

extern "C" int blvm_wavenet_embed_tables(const float* emb, const float* cw, int V, int C, int m, float* P, void* stream) {
  using namespace blvm;
  BLVM_REQUIRE(emb && cw && P && aligned16(P), "wavenet_embed_tables: NULL or misaligned argument");
  BLVM_TRY(embed_shape_ok("wavenet_embed_tables", V, C, m));
  hipLaunchKernelGGL(embed_tables_kernel, dim3(grid_for((size_t)2 * (V + 1) * C)), dim3(256), 0, static_cast<hipStream_t>(stream), emb, cw, V,
                     C, m, P);
  BLVM_CHECK_LAUNCH("wavenet_embed_tables");
  return BLVM_OK;
}

extern "C" int blvm_wavenet_embed_fwd(const float* P, const float* bias, const int32_t* k, int L_in, int B, int V, int C, int pad_causal,
                                      float* out, void* stream) {
  using namespace blvm;
  BLVM_REQUIRE(P && bias && k && out && aligned16(P) && aligned16(bias) && aligned16(out), "wavenet_embed_fwd: NULL or misaligned argument");
  BLVM_TRY(embed_shape_ok("wavenet_embed_fwd", V, C, 1));
  const int L_out = L_in - 1 - (pad_causal ? 1 : 0);
  BLVM_REQUIRE(B > 0 && L_out >= 0, "wavenet_embed_fwd: L_in = %d, B = %d: need B > 0 and L_in >= %d", L_in, B, pad_causal ? 2 : 1);
  if (L_out == 0) return BLVM_OK;
  const size_t rows = (size_t)L_out * B, lds = sizeof(float) * 2 * (size_t)(V + 1) * C;
  const int c4 = C / 4;
  auto s = static_cast<hipStream_t>(stream);
  const float4* P4 = reinterpret_cast<const float4*>(P);
  const float4* b4 = reinterpret_cast<const float4*>(bias);
  float4* o4 = reinterpret_cast<float4*>(out);
  if (lds <= EMB_LDS_BYTES)
    hipLaunchKernelGGL(embed_front_kernel<true>, dim3(grid_for(rows * c4, 1024)), dim3(256), lds, s, P4, b4, k, rows, B, V, c4, o4);
  else
    hipLaunchKernelGGL(embed_front_kernel<false>, dim3(grid_for(rows * c4, 8192)), dim3(256), 0, s, P4, b4, k, rows, B, V, c4, o4);
  BLVM_CHECK_LAUNCH("wavenet_embed_fwd");
  return BLVM_OK;
}

extern "C" size_t blvm_wavenet_embed_bwd_workspace_floats(int n, int V, int C, int m) {
  if (n <= 0 || V <= 0 || C <= 0 || m <= 0) return 0;
  return blvm::embed_bwd_space(n, V, C, m).total;
}

extern "C" int blvm_wavenet_embed_bwd(const float* d_out, const int32_t* sorted_keys, const int32_t* perm, const int32_t* starts, int L_out,
                                      int B, int V, int C, int m, const float* emb, const float* cw, float* G, float* workspace, float* d_emb,
                                      float* d_cw, float* d_bias, void* stream) {
  using namespace blvm;
  BLVM_REQUIRE(d_out && sorted_keys && perm && starts && emb && cw && G && workspace && d_emb && d_cw && d_bias && aligned16(workspace),
               "wavenet_embed_bwd: NULL or misaligned argument");
  BLVM_TRY(embed_shape_ok("wavenet_embed_bwd", V, C, m));
  BLVM_REQUIRE(L_out > 0 && B > 0 && ((size_t)L_out + 1) * B < (1ull << 31) - EMB_CHUNK, "wavenet_embed_bwd: need L_out > 0, B > 0, (L_out + 1) B < 2^31 (L_out %d, B %d)", L_out, B);
  const int n = (L_out + 1) * B, n_chunks = (n + EMB_CHUNK - 1) / EMB_CHUNK, n_kparts = (V + EMB_KCHUNK - 1) / EMB_KCHUNK;
  const EmbedBwdSpace sp = embed_bwd_space(n, V, C, m);
  float* parts = workspace + sp.parts;
  float* csum = workspace + sp.csum;
  float* wpart = workspace + sp.wpart;
  auto s = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(embed_chunk_sums_kernel, dim3((unsigned)n_chunks), dim3(256), 0, s, d_out, sorted_keys, perm, n, B, (size_t)L_out * B, C, V,
                     G, parts, csum);
  hipLaunchKernelGGL(embed_class_sums_kernel, dim3(grid_for((size_t)2 * V * C, 65536)), dim3(256), 0, s, starts, n, C, V, parts, G);
  hipLaunchKernelGGL(embed_bias_grad_kernel, dim3(1), dim3(1024), 0, s, csum, n_chunks, C, d_bias);
  hipLaunchKernelGGL(embed_table_grad_kernel, dim3(grid_for((size_t)V * C * m, 65536)), dim3(256), 0, s, G, cw, V, C, m, d_emb);
  hipLaunchKernelGGL(embed_conv_grad_parts_kernel, dim3((unsigned)n_kparts), dim3(256), 0, s, G, emb, V, C, m, wpart);
  hipLaunchKernelGGL(embed_conv_grad_kernel, dim3((unsigned)((2 * C * m + 255) / 256)), dim3(256), 0, s, wpart, n_kparts, 2 * C * m, d_cw);
  BLVM_CHECK_LAUNCH("wavenet_embed_bwd");
  return BLVM_OK;
}
