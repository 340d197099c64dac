// seqchain.hip — register-resident persistent kernels for GRU / LSTM sequences (see seqchain.h).
#include "seqchain.h"

namespace blvm {
namespace {
using namespace pchain;
constexpr int NW = 8;

// The resident product is pchain.h's (load_w / product_regs): one operand slab, every product reads it, weights from registers.
template <int OT, int G, int NCH>
__device__ __forceinline__ void load_w(typename WFrag<OT>::type (&w)[G][NCH], const float* W, const int (&c0)[G], int K) {
  const float* Ws[G];
#pragma unroll
  for (int g = 0; g < G; ++g) Ws[g] = W;
  pchain::load_w<NW, OT, G, NCH>(w, Ws, c0, K);
}
template <int OT, int G, int NCH, bool SHARED, class Mid>
__device__ __forceinline__ void product(const float* A16, int r0, int nrows, int K, const typename WFrag<OT>::type (&w)[G][NCH], f32x4 (&acc)[G], Poll& pl,
                                        Mid mid) {
  const float* const As[1] = {A16};
  product_regs<NW, OT, 1, G, MapSame, NCH, SHARED>(As, r0, nrows, K, w, acc, pl, mid);
}

struct TileAt { int r0, c0; };
__device__ __forceinline__ TileAt my_tile(int B) {
  const int rt = (B + 15) / 16;
  return TileAt{(int)(blockIdx.x % rt) * 16, (int)(blockIdx.x / rt) * 16};
}

template <int OT, int NCH>
__global__ __launch_bounds__(NW * 64, 1) void gru_fwd_kernel(SeqGruFwd a) {
  __shared__ float red[2][3 * NW * 256];
  const TileAt tl = my_tile(a.B);
  const int R = a.R, B = a.B, r0 = tl.r0, c0 = tl.c0;
  const int t = threadIdx.x & 255, row = r0 + (t >> 4), col = c0 + (t & 15);
  const bool own = threadIdx.x < 256 && row < B;
  const int rowc = row < B ? row : r0;
  const size_t o = (size_t)rowc * R + col, sR = (size_t)B * R, xR = (size_t)((B + 15) / 16) * 16 * R;
  typename WFrag<OT>::type w[3][NCH];
  {
    const int cs[3] = {c0, R + c0, 2 * R + c0};
    load_w<OT, 3, NCH>(w, a.Whh, cs, R);
  }
  const float b0 = a.bhh[col], b1 = a.bhh[R + col], b2 = a.bhh[2 * R + col];
  Poll pl{a.ctl, 0u, false, 1};
  const Out hn{nullptr, R, false, nullptr, R / 16};
  for (int j = 0; j < a.T; ++j) {
    pl.code = ((unsigned)j << 4) | 1u;
    int idx = 0;
    float x0 = 0.f, x1 = 0.f, x2 = 0.f, hp = 0.f;
    auto prefetch = [&]() {
      idx = seq_time_index(j, a.reverse, a.lens, rowc);
      const size_t ox = ((size_t)idx * B + rowc) * 3 * R + col;
      x0 = a.xg[ox]; x1 = a.xg[ox + R]; x2 = a.xg[ox + 2 * R];
      hp = a.Hs[(size_t)j * sR + o];
    };
    f32x4 acc[3] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
    product<OT, 3, NCH, false>(a.H16 + (size_t)j * xR, r0, B, R, w, acc, pl, prefetch);
    float v[3];
    reduce_tiles<3, NW>(acc, red[j & 1], v);
    if (!own) continue;
    const float hnn = v[2] + b2;
    const float r = sigmoidf_(x0 + v[0] + b0);
    const float u = sigmoidf_(x1 + v[1] + b1);
    const float n = tanhf(x2 + r * hnn);
    const float h2 = (1.f - u) * n + u * hp;
    Out oo = hn;
    oo.rm = a.Hs + (size_t)(j + 1) * sR; oo.x16 = const_cast<float*>(a.H16) + (size_t)(j + 1) * xR;
    put(oo, r0, c0, row, col, h2);
    a.out[(size_t)idx * a.out_ts + (size_t)row * a.out_ld + col] = h2;
    const size_t os = (size_t)j * sR + o;
    a.rg[os] = r; a.ug[os] = u; a.ng[os] = n; a.ghn[os] = hnn;
  }
}

template <int OT, int NCH>
__global__ __launch_bounds__(NW * 64, 1) void gru_bwd_kernel(SeqGruBwd a) {
  __shared__ float red[2][NW * 256];
  const TileAt tl = my_tile(a.B);
  const int R = a.R, B = a.B, T = a.T, r0 = tl.r0, c0 = tl.c0;
  const int t = threadIdx.x & 255, row = r0 + (t >> 4), col = c0 + (t & 15);
  const bool own = threadIdx.x < 256 && row < B;
  const int rowc = row < B ? row : r0;
  const size_t o = (size_t)rowc * R + col, sR = (size_t)B * R, x3R = (size_t)((B + 15) / 16) * 16 * 3 * R;
  typename WFrag<OT>::type w[1][NCH];
  {
    const int cs[1] = {c0};
    load_w<OT, 1, NCH>(w, a.WhhT, cs, 3 * R);
  }
  Poll pl{a.ctl, 0u, false, 1};
  float g = own ? a.G[o] : 0.f;  // the running gradient through the u-gate path: this thread's for the whole sequence
  for (int s = 0; s < a.steps; ++s) {
    const int j = T - 1 - s;
    const bool has_gemm = s >= 1, has_gates = s < T;
    pl.code = ((unsigned)s << 4) | 2u;
    float dout = 0.f, r = 0.f, u = 0.f, n = 0.f, hn = 0.f, hp = 0.f;
    int idx = 0;
    auto prefetch = [&]() {
      if (has_gates) {  // uniform
        idx = seq_time_index(j, a.reverse, a.lens, rowc);
        dout = a.dout[(size_t)idx * a.out_ts + (size_t)rowc * a.out_ld + col];
        const size_t os = (size_t)j * sR + o;
        r = a.rg[os]; u = a.ug[os]; n = a.ng[os]; hn = a.ghn[os]; hp = a.Hs[os];
      }
    };
    float v[1] = {0.f};
    if (has_gemm) {  // uniform
      f32x4 acc[1] = {{0.f, 0.f, 0.f, 0.f}};
      product<OT, 1, NCH, (NCH >= 12)>(a.DGH16 + (size_t)(s - 1) * x3R, r0, B, 3 * R, w, acc, pl, prefetch);
      reduce_tiles<1, NW>(acc, red[s & 1], v);
    } else {
      prefetch();
    }
    if (!own) continue;
    g += dout + v[0];
    if (!has_gates) { a.dh0[o] = g; continue; }
    const float dn_pre = g * (1.f - u) * (1.f - n * n);
    const float du_pre = g * (hp - n) * u * (1.f - u);
    const float dr_pre = dn_pre * hn * r * (1.f - r);
    const size_t oi = ((size_t)idx * B + row) * 3 * R + col;
    a.DGI[oi] = dr_pre; a.DGI[oi + R] = du_pre; a.DGI[oi + 2 * R] = dn_pre;
    const Out od{a.DGH + (size_t)j * 3 * sR, 3 * R, false, const_cast<float*>(a.DGH16) + (size_t)s * x3R, 3 * R / 16};
    put(od, r0, c0, row, col, dr_pre);
    put(od, r0, R + c0, row, R + col, du_pre);
    put(od, r0, 2 * R + c0, row, 2 * R + col, dn_pre * r);
    g *= u;
  }
  if (own) a.G[o] = g;
}

template <int OT, int NCH>
__global__ __launch_bounds__(NW * 64, 1) void lstm_fwd_kernel(SeqLstmFwd a) {
  __shared__ float red[2][4 * NW * 256];
  const TileAt tl = my_tile(a.B);
  const int H = a.H, B = a.B, r0 = tl.r0, c0 = tl.c0;
  const int tt = threadIdx.x & 255, row = r0 + (tt >> 4), col = c0 + (tt & 15);
  const bool own = threadIdx.x < 256 && row < B;
  const int rowc = row < B ? row : r0;
  const size_t o = (size_t)rowc * H + col, o4 = (size_t)rowc * 4 * H + col, sH = (size_t)B * H, xH = (size_t)((B + 15) / 16) * 16 * H;
  typename WFrag<OT>::type w[4][NCH];
  {
    const int cs[4] = {c0, H + c0, 2 * H + c0, 3 * H + c0};
    load_w<OT, 4, NCH>(w, a.Whh, cs, H);
  }
  const float b0 = a.bhh[col], b1 = a.bhh[H + col], b2 = a.bhh[2 * H + col], b3 = a.bhh[3 * H + col];
  const int len = a.lens != nullptr ? a.lens[rowc] : a.T;
  float cp = a.Cs[o];  // the cell state of this element lives in a register for the whole sequence (and is saved per step)
  Poll pl{a.ctl, 0u, false, 1};
  for (int t = 0; t < a.T; ++t) {
    pl.code = ((unsigned)t << 4) | 3u;
    float x0 = 0.f, x1 = 0.f, x2 = 0.f, x3 = 0.f, hp = 0.f;
    auto prefetch = [&]() {
      const float* xg = a.xg + (size_t)t * 4 * sH;
      x0 = xg[o4] + b0; x1 = xg[o4 + H] + b1; x2 = xg[o4 + 2 * H] + b2; x3 = xg[o4 + 3 * H] + b3;
      hp = a.Hs[(size_t)t * sH + o];
    };
    f32x4 acc[4] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
    product<OT, 4, NCH, false>(a.H16 + (size_t)t * xH, r0, B, H, w, acc, pl, prefetch);
    float v[4];
    reduce_tiles<4, NW>(acc, red[t & 1], v);
    if (!own) continue;
    const bool live = t < len;
    const float i = sigmoidf_(v[0] + x0), f = sigmoidf_(v[1] + x1), g = tanhf(v[2] + x2), og = sigmoidf_(v[3] + x3);
    const float c2 = f * cp + i * g;
    const float h2 = og * tanhf(c2);
    cp = live ? c2 : cp;
    a.Cs[(size_t)(t + 1) * sH + o] = cp;
    const Out oo{a.Hs + (size_t)(t + 1) * sH, H, false, const_cast<float*>(a.H16) + (size_t)(t + 1) * xH, H / 16};
    put(oo, r0, c0, row, col, live ? h2 : hp);
    a.out[(size_t)t * sH + o] = live ? h2 : 0.f;
    float* gt = a.gates + (size_t)t * 4 * sH;
    gt[o4] = live ? i : 0.f; gt[o4 + H] = live ? f : 0.f; gt[o4 + 2 * H] = live ? g : 0.f; gt[o4 + 3 * H] = live ? og : 0.f;
  }
}

template <int OT, int NCH>
__global__ __launch_bounds__(NW * 64, 1) void lstm_bwd_kernel(SeqLstmBwd a) {
  __shared__ float red[2][NW * 256];
  const TileAt tl = my_tile(a.B);
  const int H = a.H, B = a.B, T = a.T, r0 = tl.r0, c0 = tl.c0;
  const int tt = threadIdx.x & 255, row = r0 + (tt >> 4), col = c0 + (tt & 15);
  const bool own = threadIdx.x < 256 && row < B;
  const int rowc = row < B ? row : r0;
  const size_t o = (size_t)rowc * H + col, o4 = (size_t)rowc * 4 * H + col, sH = (size_t)B * H, x4H = (size_t)((B + 15) / 16) * 16 * 4 * H;
  typename WFrag<OT>::type w[1][NCH];
  {
    const int cs[1] = {c0};
    load_w<OT, 1, NCH>(w, a.WhhT, cs, 4 * H);
  }
  Poll pl{a.ctl, 0u, false, 1};
  float dc = own ? a.DC[o] : 0.f;  // running gradient wrt the cell state
  for (int s = 0; s < a.steps; ++s) {
    const int t = T - 1 - s;
    const bool has_gemm = s >= 1, has_gates = s < T;
    pl.code = ((unsigned)s << 4) | 4u;
    float dh = 0.f, ig = 0.f, fg = 0.f, gg = 0.f, og = 0.f, cs = 0.f, cs1 = 0.f;
    auto prefetch = [&]() {
      if (has_gates) {  // uniform
        dh = a.dout[(size_t)t * sH + o];
        const float* gt = a.gates + (size_t)t * 4 * sH;
        ig = gt[o4]; fg = gt[o4 + H]; gg = gt[o4 + 2 * H]; og = gt[o4 + 3 * H];
        cs = a.Cs[(size_t)t * sH + o]; cs1 = a.Cs[(size_t)(t + 1) * sH + o];
      }
    };
    float v[1] = {0.f};
    if (has_gemm) {  // uniform
      f32x4 acc[1] = {{0.f, 0.f, 0.f, 0.f}};
      product<OT, 1, NCH, (NCH >= 12)>(a.DG16 + (size_t)(s - 1) * x4H, r0, B, 4 * H, w, acc, pl, prefetch);
      reduce_tiles<1, NW>(acc, red[s & 1], v);
    } else {
      prefetch();
    }
    if (!own) continue;
    dh += v[0];
    if (!has_gates) { a.dh0[o] = dh; continue; }
    const float tc = tanhf(cs1);
    const float d_o = dh * tc;
    const float dct = dc + dh * og * (1.f - tc * tc);
    const Out od{a.DG + (size_t)t * 4 * sH, 4 * H, false, const_cast<float*>(a.DG16) + (size_t)s * x4H, 4 * H / 16};
    put(od, r0, c0, row, col, dct * gg * ig * (1.f - ig));
    put(od, r0, H + c0, row, H + col, dct * cs * fg * (1.f - fg));
    put(od, r0, 2 * H + c0, row, 2 * H + col, dct * ig * (1.f - gg * gg));
    put(od, r0, 3 * H + c0, row, 3 * H + col, d_o * og * (1.f - og));
    dc = dct * fg;
  }
  if (own) a.DC[o] = dc;
}

// ---- both directions of a bidirectional LSTM layer in one launch (seqchain.h) ---------------------------------------------------
// The workgroup's direction and tile, once at entry.  tiles = (H/16) rt is a multiple of 8 rt for the widths these kernels take, so
// blockIdx % 8 still fixes the row tile (what the SHARED product of the backward kernel relies on) and every XCD serves both chains.
struct BidirAt { int dir, r0, c0; };
__device__ __forceinline__ BidirAt my_bidir_tile(int B, int H) {
  const int rt = (B + 15) / 16, tiles = (H / 16) * rt;
  const int dir = (int)blockIdx.x >= tiles ? 1 : 0, tile = (int)blockIdx.x - dir * tiles;
  return BidirAt{dir, (tile % rt) * 16, (tile / rt) * 16};
}
// seq_time_index (pchain.h) with the row's length already in a register
__device__ __forceinline__ int bidir_time_index(int j, int dir, int len) { return dir != 0 && j < len ? len - 1 - j : j; }

// The arithmetic of lstm_fwd_kernel, product for product; h and c of this thread's element stay in registers for the whole sequence.
template <int OT, int NCH>
__global__ __launch_bounds__(NW * 64, 1) void lstm_bidir_fwd_kernel(SeqLstmBidirFwd a) {
  __shared__ float red[2][4 * NW * 256];
  const BidirAt tl = my_bidir_tile(a.B, a.H);
  const SeqLstmBidirFwdDir q = a.d[tl.dir];
  const int H = a.H, B = a.B, r0 = tl.r0, c0 = tl.c0, dir = tl.dir;
  const int tt = threadIdx.x & 255, row = r0 + (tt >> 4), col = c0 + (tt & 15);
  const bool own = threadIdx.x < 256 && row < B;
  const int rowc = row < B ? row : r0;
  const size_t o = (size_t)rowc * H + col, o4 = (size_t)rowc * 4 * H + col, sH = (size_t)B * H, xH = (size_t)((B + 15) / 16) * 16 * H;
  const size_t oo2 = (size_t)rowc * 2 * H + (size_t)dir * H + col;
  typename WFrag<OT>::type w[4][NCH];
  {
    const int cs[4] = {c0, H + c0, 2 * H + c0, 3 * H + c0};
    load_w<OT, 4, NCH>(w, q.Whh, cs, H);
  }
  const float b0 = q.bhh[col], b1 = q.bhh[H + col], b2 = q.bhh[2 * H + col], b3 = q.bhh[3 * H + col];
  const int len = min(max(a.lens[rowc], 0), a.T);
  float cp = 0.f, hp = 0.f;
  Poll pl{a.ctl, 0u, false, 1};
  for (int t = 0; t < a.T; ++t) {
    pl.code = ((unsigned)t << 4) | 5u;
    const int idx = bidir_time_index(t, dir, len);
    float x0 = 0.f, x1 = 0.f, x2 = 0.f, x3 = 0.f;
    auto prefetch = [&]() {
      const float* xg = q.xg + (size_t)idx * 4 * sH;
      x0 = xg[o4] + b0; x1 = xg[o4 + H] + b1; x2 = xg[o4 + 2 * H] + b2; x3 = xg[o4 + 3 * H] + b3;
    };
    f32x4 acc[4] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
    product<OT, 4, NCH, false>(q.H16 + (size_t)t * xH, r0, B, H, w, acc, pl, prefetch);
    float v[4];
    reduce_tiles<4, NW>(acc, red[t & 1], v);
    if (!own) continue;
    const bool live = t < len;
    const float i = sigmoidf_(v[0] + x0), f = sigmoidf_(v[1] + x1), g = tanhf(v[2] + x2), og = sigmoidf_(v[3] + x3);
    const float c2 = f * cp + i * g;
    const float h2 = og * tanhf(c2);
    const float cn = live ? c2 : cp, hn = live ? h2 : hp;
    const Out oo{nullptr, H, false, const_cast<float*>(q.H16) + (size_t)(t + 1) * xH, H / 16};
    put_t16(oo, r0, c0, row, col, hn);  // the hand-off first; the saves below sit at the row's TIME index
    const size_t os = (size_t)idx * sH + o;
    q.Hin[os] = hp; q.Cin[os] = cp; q.Cout[os] = cn;
    a.out[(size_t)idx * 2 * sH + oo2] = live ? h2 : 0.f;
    float* gt = q.gates + (size_t)idx * 4 * sH;
    gt[o4] = live ? i : 0.f; gt[o4 + H] = live ? f : 0.f; gt[o4 + 2 * H] = live ? g : 0.f; gt[o4 + 3 * H] = live ? og : 0.f;
    cp = cn; hp = hn;
  }
}

template <int OT, int NCH>
__global__ __launch_bounds__(NW * 64, 1) void lstm_bidir_bwd_kernel(SeqLstmBidirBwd a) {
  __shared__ float red[2][NW * 256];
  const BidirAt tl = my_bidir_tile(a.B, a.H);
  const SeqLstmBidirBwdDir q = a.d[tl.dir];
  const int H = a.H, B = a.B, T = a.T, r0 = tl.r0, c0 = tl.c0, dir = tl.dir;
  const int tt = threadIdx.x & 255, row = r0 + (tt >> 4), col = c0 + (tt & 15);
  const bool own = threadIdx.x < 256 && row < B;
  const int rowc = row < B ? row : r0;
  const size_t o = (size_t)rowc * H + col, o4 = (size_t)rowc * 4 * H + col, sH = (size_t)B * H, x4H = (size_t)((B + 15) / 16) * 16 * 4 * H;
  const size_t oo2 = (size_t)rowc * 2 * H + (size_t)dir * H + col;
  typename WFrag<OT>::type w[1][NCH];
  {
    const int cs[1] = {c0};
    load_w<OT, 1, NCH>(w, q.WhhT, cs, 4 * H);
  }
  const int len = min(max(a.lens[rowc], 0), T);
  Poll pl{a.ctl, 0u, false, 1};
  float dc = 0.f;  // running gradient wrt the cell state
  for (int s = 0; s < T; ++s) {
    const int j = T - 1 - s, idx = bidir_time_index(j, dir, len);
    const bool has_gemm = s >= 1;
    pl.code = ((unsigned)s << 4) | 6u;
    float dh = 0.f, ig = 0.f, fg = 0.f, gg = 0.f, og = 0.f, cs = 0.f, cs1 = 0.f;
    auto prefetch = [&]() {
      dh = a.dout[(size_t)idx * 2 * sH + oo2];
      const float* gt = q.gates + (size_t)idx * 4 * sH;
      ig = gt[o4]; fg = gt[o4 + H]; gg = gt[o4 + 2 * H]; og = gt[o4 + 3 * H];
      cs = q.Cin[(size_t)idx * sH + o]; cs1 = q.Cout[(size_t)idx * sH + o];
    };
    float v[1] = {0.f};
    if (has_gemm) {  // uniform
      f32x4 acc[1] = {{0.f, 0.f, 0.f, 0.f}};
      product<OT, 1, NCH, (NCH >= 12)>(q.DG16 + (size_t)(s - 1) * x4H, r0, B, 4 * H, w, acc, pl, prefetch);
      reduce_tiles<1, NW>(acc, red[s & 1], v);
    } else {
      prefetch();
    }
    if (!own) continue;
    dh += v[0];
    const float tc = tanhf(cs1);
    const float d_o = dh * tc;
    const float dct = dc + dh * og * (1.f - tc * tc);
    const float di = dct * gg * ig * (1.f - ig), df = dct * cs * fg * (1.f - fg), dg = dct * ig * (1.f - gg * gg), dog = d_o * og * (1.f - og);
    const Out od{nullptr, 4 * H, false, const_cast<float*>(q.DG16) + (size_t)s * x4H, 4 * H / 16};
    put_t16(od, r0, c0, row, col, di);
    put_t16(od, r0, H + c0, row, H + col, df);
    put_t16(od, r0, 2 * H + c0, row, 2 * H + col, dg);
    put_t16(od, r0, 3 * H + c0, row, 3 * H + col, dog);
    float* dgt = q.DG + (size_t)idx * 4 * sH;  // row-major at the row's TIME index: a per-row address, so not through put()
    dgt[o4] = di; dgt[o4 + H] = df; dgt[o4 + 2 * H] = dg; dgt[o4 + 3 * H] = dog;
    dc = dct * fg;
  }
}

inline bool nch_ok(int nch) { return nch == 1 || nch == 2 || nch == 3 || nch == 4 || nch == 6 || nch == 8 || nch == 12; }

#define SEQ_LAUNCH_OT(kernel, N, ot, grid, s, args)                                                                  \
  if ((ot) == OP_BF16) hipLaunchKernelGGL((kernel<OP_BF16, N>), grid, dim3(NW * 64), 0, s, args);                     \
  else if ((ot) == OP_F16) hipLaunchKernelGGL((kernel<OP_F16, N>), grid, dim3(NW * 64), 0, s, args);                  \
  else hipLaunchKernelGGL((kernel<OP_F32, N>), grid, dim3(NW * 64), 0, s, args)
#define SEQ_LAUNCH(kernel, nch, ot, grid, s, args)                                                                     \
  do {                                                                                                                 \
    switch (nch) {                                                                                                     \
      case 1: SEQ_LAUNCH_OT(kernel, 1, ot, grid, s, args); break;                                                      \
      case 2: SEQ_LAUNCH_OT(kernel, 2, ot, grid, s, args); break;                                                      \
      case 3: SEQ_LAUNCH_OT(kernel, 3, ot, grid, s, args); break;                                                      \
      case 4: SEQ_LAUNCH_OT(kernel, 4, ot, grid, s, args); break;                                                      \
      case 6: SEQ_LAUNCH_OT(kernel, 6, ot, grid, s, args); break;                                                      \
      case 8: SEQ_LAUNCH_OT(kernel, 8, ot, grid, s, args); break;                                                      \
      case 12: SEQ_LAUNCH_OT(kernel, 12, ot, grid, s, args); break;                                                    \
      default: set_error("seqchain: %d k-chunks per wave are not instantiated", nch); return BLVM_ENOSUP;              \
    }                                                                                                                  \
  } while (0)

}  // namespace

// env BLVM_SEQ_REGS: bit 0 forward, bit 1 backward sequences on these kernels (default: see seq_regs_mask)
int seq_regs_mask() {
  static const int v = [] { const char* e = getenv("BLVM_SEQ_REGS"); return e ? atoi(e) : 3; }();
  return v;
}
bool seq_regs_applies(int K_fwd, int K_bwd, int hidden, int B, int gates) {
  if (K_fwd % (NW * 16) != 0 || K_bwd % (NW * 16) != 0 || hidden % 16 != 0) return false;
  if (!nch_ok(K_fwd / (NW * 16)) || !nch_ok(K_bwd / (NW * 16))) return false;
  if (gates * (K_fwd / (NW * 16)) > 24) return false;  // the forward slice (gates x k-chunks fragments per lane) must fit the registers
  return (hidden / 16) * ((B + 15) / 16) <= device_cus();
}

int seq_gru_fwd(SeqGruFwd a, hipStream_t s) {
  BLVM_TRY(pchain_ctl(a.ctl));
  const dim3 grid((unsigned)((a.R / 16) * ((a.B + 15) / 16)));
  SEQ_LAUNCH(gru_fwd_kernel, a.R / (NW * 16), a.ot, grid, s, a);
  BLVM_CHECK_LAUNCH("seq_gru_fwd");
  return BLVM_OK;
}
int seq_gru_bwd(SeqGruBwd a, hipStream_t s) {
  BLVM_TRY(pchain_ctl(a.ctl));
  const dim3 grid((unsigned)((a.R / 16) * ((a.B + 15) / 16)));
  SEQ_LAUNCH(gru_bwd_kernel, 3 * a.R / (NW * 16), a.ot, grid, s, a);
  BLVM_CHECK_LAUNCH("seq_gru_bwd");
  return BLVM_OK;
}
int seq_lstm_fwd(SeqLstmFwd a, hipStream_t s) {
  BLVM_TRY(pchain_ctl(a.ctl));
  const dim3 grid((unsigned)((a.H / 16) * ((a.B + 15) / 16)));
  SEQ_LAUNCH(lstm_fwd_kernel, a.H / (NW * 16), a.ot, grid, s, a);
  BLVM_CHECK_LAUNCH("seq_lstm_fwd");
  return BLVM_OK;
}
int seq_lstm_bwd(SeqLstmBwd a, hipStream_t s) {
  BLVM_TRY(pchain_ctl(a.ctl));
  const dim3 grid((unsigned)((a.H / 16) * ((a.B + 15) / 16)));
  SEQ_LAUNCH(lstm_bwd_kernel, 4 * a.H / (NW * 16), a.ot, grid, s, a);
  BLVM_CHECK_LAUNCH("seq_lstm_bwd");
  return BLVM_OK;
}
int seq_lstm_bidir_fwd(SeqLstmBidirFwd a, hipStream_t s) {
  BLVM_TRY(pchain_ctl(a.ctl));
  const dim3 grid((unsigned)(2 * (a.H / 16) * ((a.B + 15) / 16)));
  SEQ_LAUNCH(lstm_bidir_fwd_kernel, a.H / (NW * 16), a.ot, grid, s, a);
  BLVM_CHECK_LAUNCH("seq_lstm_bidir_fwd");
  return BLVM_OK;
}
int seq_lstm_bidir_bwd(SeqLstmBidirBwd a, hipStream_t s) {
  BLVM_TRY(pchain_ctl(a.ctl));
  const dim3 grid((unsigned)(2 * (a.H / 16) * ((a.B + 15) / 16)));
  SEQ_LAUNCH(lstm_bidir_bwd_kernel, 4 * a.H / (NW * 16), a.ot, grid, s, a);
  BLVM_CHECK_LAUNCH("seq_lstm_bidir_bwd");
  return BLVM_OK;
}

}  // namespace blvm
