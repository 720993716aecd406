// srk_eval.hip -- per-image jet observables of the evaluation loop (evaluation/eval.py's MultHist modes) and the per-pixel
// counts behind SumRaster / MeanImage (utils.py:275-328).
//
// srk_eval_image_stats: one 256-thread workgroup per image.  The image is never held: it is read from global memory (L2 after
// the first pass) in passes of 256 consecutive pixels, which serves 40^2 and 512^2 alike:
//   pass 0      basic statistics, the jet four-momentum (fp64, cosh / sinh / cos / sin of the bin centres from LDS tables) and
//               the histogram of the top 8 bits of every pixel's order key;
//   passes 1-3  the histogram of the next 8 bits among the pixels whose key matches the prefix selected so far.  After pass 3 the
//               key T of the K-th largest value is known, with the count of keys > T (< K) and the count of keys == T;
//   collect     an ordered compaction (per 256-pixel tile: ballots + a 4-wave scan) of every key > T and of the first
//               K - #(> T) keys == T in position order; it stops once both are complete;
//   sort        K <= 64 candidates ranked by (key desc, position asc) in LDS; ties and the Fox-Wolfram moments follow from them.
// Histogram adds are wave-aggregated (one LDS atomic per distinct bin per wave-instruction): the jets' zero pixels all share a
// bin, which plain per-lane atomics would serialise 64-fold.  Nothing depends on arrival order: the counts are integers and
// every floating-point sum is a fixed tree (per-thread strided sums -> xor shuffles -> the four wave sums in order).
#include "srk_internal.h"
#include <math.h>

namespace {

constexpr int EV_THREADS = 256;
constexpr int EV_WAVES = EV_THREADS / 64;
constexpr int EV_MAX_SIDE = 512;

// order-preserving key: larger float -> larger key; -0 folds onto +0 (they compare equal, as np.where(tmp == value) has it)
__device__ __forceinline__ uint32_t order_key(float f) {
  uint32_t u = __float_as_uint(f);
  if ((u << 1) == 0) u = 0;
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// fixed-order block sum of N doubles; every thread gets the totals
template <int N>
__device__ __forceinline__ void block_sum(double (&v)[N], double* s_red) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
  for (int n = 0; n < N; ++n) v[n] = wave_sum(v[n]);
  if (lane == 0)
#pragma unroll
    for (int n = 0; n < N; ++n) s_red[w * N + n] = v[n];
  __syncthreads();
#pragma unroll
  for (int n = 0; n < N; ++n) {
    double s = 0.0;
#pragma unroll
    for (int k = 0; k < EV_WAVES; ++k) s += s_red[k * N + n];
    v[n] = s;
  }
  __syncthreads();
}

// add one to hist[bin] for every active lane, one atomic per distinct bin of the wave (match-any by 8 ballots)
__device__ __forceinline__ void hist_add(uint32_t* hist, uint32_t bin, bool active) {
  unsigned long long peers = __ballot(active);
  if (peers == 0) return;                           // wave-uniform
#pragma unroll
  for (int b = 0; b < 8; ++b) {
    const bool bit = (bin >> b) & 1u;
    const unsigned long long m = __ballot(active && bit);
    peers &= bit ? m : ~m;
  }
  const int lane = threadIdx.x & 63;
  if (active && lane == __ffsll((long long)peers) - 1) atomicAdd(&hist[bin], (uint32_t)__popcll(peers));
}

__device__ __forceinline__ double legendre(int l, double x) {
  if (l == 0) return 1.0;
  double p0 = 1.0, p1 = x;
  for (int n = 1; n < l; ++n) {
    const double p2 = ((2 * n + 1) * x * p1 - n * p0) / (n + 1);
    p0 = p1;
    p1 = p2;
  }
  return p1;
}

__global__ void __launch_bounds__(EV_THREADS) image_stats_kernel(srk_eval_args a) {
  __shared__ double s_ch[EV_MAX_SIDE], s_sh[EV_MAX_SIDE], s_cp[EV_MAX_SIDE], s_sp[EV_MAX_SIDE];
  __shared__ double s_red[EV_WAVES * 8];
  __shared__ uint32_t s_hist[256];
  __shared__ uint32_t s_wsum[EV_WAVES];
  __shared__ uint32_t s_sel[3];
  __shared__ uint32_t s_cnt[2][2][EV_WAVES];
  __shared__ uint32_t s_ckey[SRK_EVAL_MAX_K], s_skey[SRK_EVAL_MAX_K];
  __shared__ int32_t s_cidx[SRK_EVAL_MAX_K], s_sidx[SRK_EVAL_MAX_K];
  __shared__ double s_th[SRK_EVAL_MAX_K], s_ph[SRK_EVAL_MAX_K], s_pt[SRK_EVAL_MAX_K];
  __shared__ float s_fred[2][EV_WAVES];
  __shared__ int s_ired[2][EV_WAVES];

  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  const int b = blockIdx.x, H = a.H, W = a.W, HW = H * W, K = a.K;
  const float* x = a.x + (int64_t)b * a.sb;
  auto at = [&](int i) -> float {
    const int r = i / W, c = i - r * W;
    return x[(int64_t)r * a.sh + (int64_t)c * a.sw];
  };

  // bin centres of eval.py:52-53 (JetMass: etarange = phirange = 1, bins = H on both axes), in the reference's order of operations
  const double bins = (double)H;
  for (int r = t; r < H; r += EV_THREADS) {
    const double eta = (double)(r * 2) / bins - 1.0 + 1.0 / bins;
    s_ch[r] = cosh(eta);
    s_sh[r] = sinh(eta);
  }
  for (int c = t; c < W; c += EV_THREADS) {
    const double phi = (double)(c * 2) / bins - 1.0 + 1.0 / bins;
    s_cp[c] = cos(phi);
    s_sp[c] = sin(phi);
  }
  s_hist[t] = 0;
  __syncthreads();

  // ---- pass 0: statistics + top-byte histogram
  float vmax = -INFINITY, vmin = INFINITY;
  int nnz = 0, nan = 0;
  double acc[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};   // sum, nnz sum, E, px, py, pz
  for (int base = 0; base < HW; base += EV_THREADS) {
    const int i = base + t;
    const bool in = i < HW;
    uint32_t key = 0;
    if (in) {
      const float v = at(i);
      key = order_key(v);
      vmax = fmaxf(vmax, v);
      vmin = fminf(vmin, v);
      nan |= (v != v);
      acc[0] += (double)v;
      if (v > a.thr) { ++nnz; acc[1] += (double)v; }
      if (v != 0.f) {
        const int r = i / W, c = i - r * W;
        const double pt = (double)v;
        acc[2] += pt * s_ch[r];
        acc[3] += pt * s_cp[c];
        acc[4] += pt * s_sp[c];
        acc[5] += pt * s_sh[r];
      }
    }
    hist_add(s_hist, key >> 24, in);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    vmax = fmaxf(vmax, __shfl_xor(vmax, o, 64));
    vmin = fminf(vmin, __shfl_xor(vmin, o, 64));
    nnz += __shfl_xor(nnz, o, 64);
    nan |= __shfl_xor(nan, o, 64);
  }
  if (lane == 0) { s_fred[0][w] = vmax; s_fred[1][w] = vmin; s_ired[0][w] = nnz; s_ired[1][w] = nan; }
  block_sum(acc, s_red);                            // (its barriers also publish s_fred / s_ired and the histogram)
  if (t == 0) {
    float mx = s_fred[0][0], mn = s_fred[1][0];
    int nz = s_ired[0][0], nn = s_ired[1][0];
    for (int k = 1; k < EV_WAVES; ++k) {
      mx = fmaxf(mx, s_fred[0][k]); mn = fminf(mn, s_fred[1][k]); nz += s_ired[0][k]; nn |= s_ired[1][k];
    }
    double* st = a.stats + (int64_t)b * SRK_EVAL_NSTAT;
    st[SRK_EVAL_MAX] = mx; st[SRK_EVAL_MIN] = mn; st[SRK_EVAL_SUM] = acc[0]; st[SRK_EVAL_NNZ] = nz; st[SRK_EVAL_NNZ_SUM] = acc[1];
    st[SRK_EVAL_NAN] = nn ? 1.0 : 0.0;
    st[SRK_EVAL_E] = acc[2]; st[SRK_EVAL_PX] = acc[3]; st[SRK_EVAL_PY] = acc[4]; st[SRK_EVAL_PZ] = acc[5];
  }

  // ---- radix select of the K-th largest key, 8 bits per pass
  uint32_t prefix = 0, mask = 0, need = (uint32_t)K, n_eq = 0;
  for (int pass = 0; pass < 4; ++pass) {
    const int shift = 24 - 8 * pass;
    if (pass > 0) {
      for (int base = 0; base < HW; base += EV_THREADS) {
        const int i = base + t;
        uint32_t key = 0;
        bool m = false;
        if (i < HW) { key = order_key(at(i)); m = (key & mask) == prefix; }
        hist_add(s_hist, (key >> shift) & 255u, m);
      }
      __syncthreads();
    }
    // inclusive suffix sums over bins (bin t at thread t); select the bin holding the need-th largest
    const uint32_t h = s_hist[t];
    uint32_t s = h;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const uint32_t y = __shfl_down(s, o, 64);
      if (lane + o < 64) s += y;
    }
    if (lane == 0) s_wsum[w] = s;
    __syncthreads();
    for (int k = w + 1; k < EV_WAVES; ++k) s += s_wsum[k];
    if (s >= need && s - h < need) { s_sel[0] = (uint32_t)t; s_sel[1] = s - h; s_sel[2] = h; }
    __syncthreads();
    const uint32_t bin = s_sel[0];
    need -= s_sel[1];
    n_eq = s_sel[2];
    prefix |= bin << shift;
    mask |= 255u << shift;
    s_hist[t] = 0;
    __syncthreads();
  }
  const uint32_t T = prefix;
  const int n_gt = K - (int)need;                   // keys > T, all taken; then the first `need` keys == T by position

  // ---- ordered compaction of the candidates
  {
    const unsigned long long lt = (1ull << lane) - 1ull;
    int run_gt = 0, run_eq = 0, it = 0;
    for (int base = 0; base < HW; base += EV_THREADS, ++it) {
      const int i = base + t;
      uint32_t key = 0;
      if (i < HW) key = order_key(at(i));
      const bool gt = i < HW && key > T, eq = i < HW && key == T;
      const unsigned long long bg = __ballot(gt), be = __ballot(eq);
      const int buf = it & 1;
      if (lane == 0) { s_cnt[buf][0][w] = (uint32_t)__popcll(bg); s_cnt[buf][1][w] = (uint32_t)__popcll(be); }
      __syncthreads();
      int og = run_gt, oe = run_eq, tg = 0, te = 0;
      for (int k = 0; k < EV_WAVES; ++k) {
        const int cg = (int)s_cnt[buf][0][k], ce = (int)s_cnt[buf][1][k];
        if (k < w) { og += cg; oe += ce; }
        tg += cg; te += ce;
      }
      if (gt) {
        const int p = og + __popcll(bg & lt);
        s_ckey[p] = key; s_cidx[p] = i;
      }
      if (eq) {
        const int p = oe + __popcll(be & lt);
        if (p < (int)need) { s_ckey[n_gt + p] = key; s_cidx[n_gt + p] = i; }
      }
      run_gt += tg; run_eq += te;
      if (run_gt >= n_gt && run_eq >= (int)need) break;   // block-uniform
    }
  }
  __syncthreads();

  // ---- rank the K candidates: key descending, position ascending
  if (t < K) {
    const uint32_t kt = s_ckey[t];
    const int itx = s_cidx[t];
    int rank = 0;
    for (int u = 0; u < K; ++u) {
      const uint32_t ku = s_ckey[u];
      rank += (ku > kt) || (ku == kt && s_cidx[u] < itx);
    }
    s_skey[rank] = kt; s_sidx[rank] = itx;
  }
  __syncthreads();
  if (t < K) {
    s_sidx[t] = min(max(s_sidx[t], 0), HW - 1);     // (always in range: a guard for the reads below, not a path)
  }
  __syncthreads();
  if (t < K) {
    const int64_t o = (int64_t)b * K + t;
    a.topv[o] = at(s_sidx[t]);
    a.topi[o] = s_sidx[t];
    if (t < SRK_EVAL_TIES) {
      // every pixel with a key > T is a candidate; the count of keys == T came out of the last radix pass
      const uint32_t kt = s_skey[t];
      int cnt = 0;
      if (kt == T) cnt = (int)n_eq;
      else
        for (int u = 0; u < K; ++u) cnt += s_skey[u] == kt;
      a.ties[(int64_t)b * SRK_EVAL_TIES + t] = cnt;
    }
  }

  // ---- Fox-Wolfram moments over the top j (eval.py:78-95: no half-bin offset, bins = H, |pt|^0.5)
  for (int p = 0; p < a.n_fwm; ++p) {
    const int l = a.fwm_l[p], j = a.fwm_j[p];
    if (t < j) {
      const int i = s_sidx[t], r = i / W, c = i - r * W;
      const double eta = (double)(r * 2) / bins - 1.0;
      s_th[t] = 2.0 * atan(exp(-eta));
      s_ph[t] = (double)(c * 2) / bins - 1.0;
      s_pt[t] = (double)sqrtf(fabsf(at(i)));
    }
    __syncthreads();
    double ptsum = 0.0;
    for (int u = 0; u < j; ++u) ptsum += s_pt[u];
    double acc1[1] = {0.0};
    for (int q = t; q < j * j; q += EV_THREADS) {
      const int u = q / j, v = q - u * j;
      const double dth = s_th[u] - s_th[v], sth = s_th[u] + s_th[v], dph = s_ph[u] - s_ph[v];
      const double cd = cos(dth), cs = cos(sth);
      const double cosang = 0.5 * (cd - cs) * cos(dph) + 0.5 * (cd + cs);
      acc1[0] += s_pt[u] * s_pt[v] / (ptsum * ptsum) * legendre(l, cosang);
    }
    block_sum(acc1, s_red);
    if (t == 0) a.fwm[(int64_t)b * a.n_fwm + p] = acc1[0];
  }
}

__global__ void __launch_bounds__(256) pixel_counts_kernel(const float* __restrict__ x, int B, int H, int W, int64_t sb, int64_t sh,
                                                           int64_t sw, float thr, double* __restrict__ count,
                                                           double* __restrict__ energy) {
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (p >= H * W) return;
  const int r = p / W, c = p - r * W;
  const float* px = x + (int64_t)r * sh + (int64_t)c * sw;
  int cnt = 0;
  double clip = 0.0;
#pragma unroll 8
  for (int b = 0; b < B; ++b) {
    const float v = px[(int64_t)b * sb];
    cnt += v > thr;
    clip += (double)(v < thr ? thr : v);             // np.clip(x, thr, None): NaN stays NaN
  }
  count[p] += (double)cnt;
  if (energy) energy[p] += clip * (double)cnt;
}

}  // namespace

extern "C" int srk_eval_image_stats(const srk_eval_args* a, void* stream) {
  if (!a || !a->x || !a->stats || !a->topv || !a->topi || !a->ties || a->B <= 0 || a->H <= 0 || a->W <= 0) return SRK_ERR_BAD_ARG;
  if (a->H > EV_MAX_SIDE || a->W > EV_MAX_SIDE || a->K < 1 || a->K > SRK_EVAL_MAX_K || a->K > a->H * a->W) return SRK_ERR_BAD_ARG;
  if (a->n_fwm < 0 || a->n_fwm > SRK_EVAL_MAX_FWM || (a->n_fwm > 0 && !a->fwm)) return SRK_ERR_BAD_ARG;
  for (int p = 0; p < a->n_fwm; ++p)
    if (a->fwm_l[p] < 0 || a->fwm_l[p] > SRK_EVAL_MAX_L || a->fwm_j[p] < 1 || a->fwm_j[p] > a->K) return SRK_ERR_BAD_ARG;
  hipLaunchKernelGGL(image_stats_kernel, dim3(a->B), dim3(EV_THREADS), 0, (hipStream_t)stream, *a);
  SRK_CHECK_LAUNCH();
  return SRK_OK;
}

extern "C" int srk_eval_pixel_counts(const float* x, int B, int H, int W, int64_t sb, int64_t sh, int64_t sw, float thr, double* count,
                                     double* energy, void* stream) {
  if (!x || !count || B <= 0 || H <= 0 || W <= 0 || (int64_t)H * W > (int64_t)EV_MAX_SIDE * EV_MAX_SIDE) return SRK_ERR_BAD_ARG;
  hipLaunchKernelGGL(pixel_counts_kernel, dim3((H * W + 255) / 256), dim3(256), 0, (hipStream_t)stream, x, B, H, W, sb, sh, sw, thr,
                     count, energy);
  SRK_CHECK_LAUNCH();
  return SRK_OK;
}
