// iwbound.hip — K8m: the two reductions of the K-sample importance-weighted bound (IWAE, Burda et al. 2016)
//   L_K = log (1/K) sum_k p(x, z_k) / q(z_k | x),  z_k ~ q.
// (1) blvm_gauss_logratio_fwd: the Monte-Carlo log-density ratio log q(z) - log p(z) at the DRAWN z, summed per utterance in float64
//     (K8 has the analytic KL only).  (2) blvm_iw_reduce: log-mean-exp over the particle axis and the effective sample size.
// Evaluation only: no backward.  Both are written (not accumulated) and bit-identical from call to call: fixed reduction orders, no
// floating-point atomics.
//
// Mapping (1): a workgroup owns ONE utterance and all of its latent steps — the four waves take steps in turn, a lane 4 consecutive
// latent dimensions (16-byte loads) or one (scalar path) — and accumulates in a float64 register; wave shuffle tree + LDS, then one
// plain store.  Particles fill the batch axis (B = particles x utterances rows), so one workgroup per row fills the chip at the
// shapes this runs on; HBM-bound at 5 x 4 B per latent element (mu_q is not read).
// The per-element terms are fp32 (as K8's); they are ADDED in float64 one by one, so the cancellation between the two quadratic terms
// (they are equal where q = p) happens in float64.
#include "common.h"

namespace blvm {
namespace {

struct LogRatioArgs {
  const float *mu_q, *sd_q, *mu_p, *sd_p, *z, *eps;
  const int32_t* x_sl;
  double* out;
  int layout, B, Tp, Z, stride;
};

// log q(z) - log p(z) for one element, q = N(mu_q, sd_q) with z = mu_q + sd_q eps (the q-term from eps: that IS how z was drawn),
// p = N(mu_p, sd_p) at the stored z (the value the decoder saw).  The log(2 pi) halves cancel.
__device__ __forceinline__ double logratio_elem(float sq, float mp, float sp, float z, float e) {
  const double d = (double)((z - mp) / sp), ed = (double)e;
  return (((double)log_(sp) - (double)log_(sq)) - 0.5 * ed * ed) + 0.5 * d * d;
}

// grid (B); VEC: Z % 4 == 0 and 16-byte aligned bases (then every row is aligned)
template <bool VEC>
__global__ __launch_bounds__(256) void gauss_logratio_kernel(LogRatioArgs a) {
  __shared__ double part[4];
  const int b = blockIdx.x, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const long long xs = a.x_sl[b];
  double s = 0.0;
  // masked steps are never loaded: whatever they hold (NaN, inf) stays out of the sum.  Live steps are a prefix of 0 .. Tp-1.
  for (int t = wave; t < a.Tp && (long long)t * a.stride < xs; t += 4) {
    const size_t base = ((a.layout == 0) ? (size_t)b * a.Tp + t : (size_t)t * a.B + b) * a.Z;
    if (VEC) {
      for (int c = lane * 4; c < a.Z; c += 256) {
        const float4 sq = *reinterpret_cast<const float4*>(a.sd_q + base + c), mp = *reinterpret_cast<const float4*>(a.mu_p + base + c);
        const float4 sp = *reinterpret_cast<const float4*>(a.sd_p + base + c), zz = *reinterpret_cast<const float4*>(a.z + base + c);
        const float4 e = *reinterpret_cast<const float4*>(a.eps + base + c);
        s += logratio_elem(sq.x, mp.x, sp.x, zz.x, e.x);
        s += logratio_elem(sq.y, mp.y, sp.y, zz.y, e.y);
        s += logratio_elem(sq.z, mp.z, sp.z, zz.z, e.z);
        s += logratio_elem(sq.w, mp.w, sp.w, zz.w, e.w);
      }
    } else {
      for (int c = lane; c < a.Z; c += 64)
        s += logratio_elem(a.sd_q[base + c], a.mu_p[base + c], a.sd_p[base + c], a.z[base + c], a.eps[base + c]);
    }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off, 64);
  if (lane == 0) part[wave] = s;
  __syncthreads();
  if (threadIdx.x == 0) a.out[b] = (part[0] + part[1]) + (part[2] + part[3]);  // every row is written, a row without live steps 0
}

// One thread per utterance; k ascending.  bound = m + log sum_k exp(lw - m) - log K, ess = (sum w)^2 / sum w^2 with w = exp(lw - m).
__global__ __launch_bounds__(256) void iw_reduce_kernel(const double* __restrict__ log_w, int K, int B, double* __restrict__ bound,
                                                        double* __restrict__ ess) {
  const int b = blockIdx.x * 256 + threadIdx.x;
  if (b >= B) return;
  double m = -INFINITY;
  bool nan = false;
  for (int k = 0; k < K; ++k) {
    const double v = log_w[(size_t)k * B + b];
    nan |= v != v;
    m = v > m ? v : m;
  }
  double s1 = 0.0, s2 = 0.0;
  if (!nan && m != -INFINITY) {
    for (int k = 0; k < K; ++k) {
      const double w = exp(log_w[(size_t)k * B + b] - m);  // (the largest weight is exp(0) = 1 exactly)
      s1 += w;
      s2 += w * w;
    }
  }
  double bd, es;
  if (nan) {
    bd = es = NAN;
  } else if (m == -INFINITY) {  // no weight at all
    bd = -INFINITY;
    es = 0.0;
  } else {
    bd = m + (log(s1) - log((double)K));  // K equal weights: s1 = K exactly, the bracket is 0 and the bound is the weight itself
    es = (s1 * s1) / s2;
  }
  bound[b] = bd;
  if (ess != nullptr) ess[b] = es;
}

}  // namespace
}  // namespace blvm

extern "C" int blvm_gauss_logratio_fwd(const float* mu_q, const float* sd_q, const float* mu_p, const float* sd_p, const float* z,
                                       const float* eps, int layout, const int32_t* x_sl, int B, int Tp, int Z, int stride, double* out,
                                       void* stream) {
  using namespace blvm;
  BLVM_REQUIRE(mu_q && sd_q && mu_p && sd_p && z && eps && x_sl && out, "gauss_logratio_fwd: null pointer");
  BLVM_REQUIRE(B > 0 && Tp > 0 && Z > 0 && stride > 0, "gauss_logratio_fwd: bad shape B=%d Tp=%d Z=%d stride=%d", B, Tp, Z, stride);
  BLVM_REQUIRE(layout == 0 || layout == 1, "gauss_logratio_fwd: layout must be 0 or 1");
  BLVM_REQUIRE((long long)B * Tp < (1ll << 31), "gauss_logratio_fwd: too many rows");
  LogRatioArgs a{};
  a.mu_q = mu_q; a.sd_q = sd_q; a.mu_p = mu_p; a.sd_p = sd_p; a.z = z; a.eps = eps; a.x_sl = x_sl; a.out = out;
  a.layout = layout; a.B = B; a.Tp = Tp; a.Z = Z; a.stride = stride;
  // (mu_q is not read: z - mu_q = sd_q eps.  It is part of the call so that the call names the whole posterior.)
  const bool vec = Z % 4 == 0 && aligned16(sd_q) && aligned16(mu_p) && aligned16(sd_p) && aligned16(z) && aligned16(eps);
  if (vec) hipLaunchKernelGGL((gauss_logratio_kernel<true>), dim3(B), dim3(256), 0, static_cast<hipStream_t>(stream), a);
  else hipLaunchKernelGGL((gauss_logratio_kernel<false>), dim3(B), dim3(256), 0, static_cast<hipStream_t>(stream), a);
  BLVM_CHECK_LAUNCH("gauss_logratio_fwd");
  return BLVM_OK;
}

extern "C" int blvm_iw_reduce(const double* log_w, int K, int B, double* bound, double* ess, void* stream) {
  using namespace blvm;
  BLVM_REQUIRE(log_w && bound, "iw_reduce: null pointer");
  BLVM_REQUIRE(K > 0 && B > 0, "iw_reduce: bad shape K=%d B=%d", K, B);
  hipLaunchKernelGGL(iw_reduce_kernel, dim3((B + 255) / 256), dim3(256), 0, static_cast<hipStream_t>(stream), log_w, K, B, bound, ess);
  BLVM_CHECK_LAUNCH("iw_reduce");
  return BLVM_OK;
}
