// Sinkhorn Wasserstein loss head (esrgan.py:321,539-542; utils.py:147-257) on gfx950: device sort-and-cut of the images, the
// log-domain Sinkhorn iterations over an IMPLICIT cost matrix C_ij = (x_i - y_j)^2 (never stored), and the reverse sweep through
// the unrolled iterations.  See include/srk.h for the contract of each entry point.
//
// Layout: per image b, the points of one side live in a row of `cap` floats (x[b*cap_x + i], i < n_x), n_x / n_y on the DEVICE
// (n[0], n[1]) so the data-dependent cut never reaches the host.  Kernels are launched for the capacity and return early past n.
//
// Work unit of the O(N'M') kernels: one wave per RPW lines ("line" = a row i over all j, or a column j over all i); the lanes stride
// over the other side, and a line's partial sums are combined by an xor butterfly (every lane ends up with the same bits: a fixed
// order, so repeated runs are bit-identical).  All exponentials are exp2 of log2-scaled arguments (one v_exp_f32 each).
//
// Saved history: the row / column log-sum-exp of every iteration (log2 units), [max_iter][B][cap].  u^k and v^k are not kept:
// u^k = fma(eps, a - L^k ln2, u^{k-1}) from u^0 = 0 is replayed bit-exactly from that history in the backward (sk_step below is the
// ONE place both sweeps compute it), which halves the saved state (B = 8, 80^2, all pixels kept: 41 MB instead of 83 MB).
#include "srk_internal.h"

// No floating-point contraction anywhere in this file: __fmul_rn / __fsub_rn are plain operators in the HIP headers, and the backend
// would otherwise fuse u - d*d or marg - lse2*ln2 into an FMA at some sites and not at others.  The replay below is bit-exact only if
// every site rounds the same way; the one FMA wanted (sk_step) is written as one.
#pragma clang fp contract(off)

namespace {

constexpr int SK_WAVE = 64;
constexpr int SK_WAVES = 4;                 // waves per workgroup
constexpr int SK_RPW = 4;                   // lines per wave: each value loaded from the other side serves RPW lines
constexpr int SK_LINES = SK_WAVES * SK_RPW; // lines per workgroup
constexpr float SK_LOG2E = 1.4426950408889634f;
constexpr float SK_LN2 = 0.6931471805599453f;
constexpr float SK_THRESH = 0.1f;           // utils.py:201: stop once err < 1e-1

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, SK_WAVE);
  return v;
}

__device__ __forceinline__ double wave_sum_d(double v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, SK_WAVE);
  return v;
}

__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, SK_WAVE));
  return v;
}

// The exponent (u_i - C_ij + v_j) log2e/eps, rounded the same way wherever it is formed (no contraction): the backward's row and
// column softmaxes are normalised by the forward's log-sum-exps, and an exponent that differed from the forward's by one rounding
// would leave them off 1 by ~1e-5, which the reverse sweep amplifies (measured: 2e-3 of the largest gradient at eps 0.1, K 33).
__device__ __forceinline__ float sk_w(float u, float d, float v, float s) {
  return __fmul_rn(__fadd_rn(__fsub_rn(u, __fmul_rn(d, d)), v), s);
}

// u^k = eps * (a - LSE) + u^{k-1}, LSE = lse2 * ln 2.  The forward and the backward's replay both go through here.
// Every rounding is spelled out: the replay must reproduce the forward's potentials to the bit (one ulp off in u or v moves the
// gradient by ~1e-2 of itself at eps 0.1, K 33: the reverse sweep cancels large terms).
__device__ __forceinline__ float sk_step(float pot, float marg, float lse2, float eps) {
  return __fmaf_rn(eps, __fsub_rn(marg, __fmul_rn(lse2, SK_LN2)), pot);
}

// log(1/n + 1e-8): the reference's log(mu + 1e-8)
__device__ __forceinline__ float sk_marg(int n) { return logf(__fadd_rn(__fdiv_rn(1.f, (float)n), 1e-8f)); }

// ---------------------------------------------------------------- sort and cut
// total order of torch.sort: -0 == +0, NaN after +inf (all NaNs equal); ties broken by the flat index (stable sort)
__device__ __forceinline__ uint32_t order_key(float f) {
  if (f != f) return 0xffffffffu;
  if (f == 0.f) f = 0.f;
  const uint32_t b = __float_as_uint(f);
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

// n_out = max over the batch of #{t > thr}, or P when that is 0 (t[:, -0:] keeps the whole row).  One workgroup.
__global__ __launch_bounds__(256) void sort_count_kernel(const float* __restrict__ t, int B, int P, float thr, int* __restrict__ n_out) {
  __shared__ int red[256];
  int best = 0;
  for (int b = 0; b < B; ++b) {
    int c = 0;
    for (int i = threadIdx.x; i < P; i += 256) c += t[(size_t)b * P + i] > thr;
    red[threadIdx.x] = c;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
      if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
      __syncthreads();
    }
    best = max(best, red[0]);
    __syncthreads();
  }
  if (threadIdx.x == 0) *n_out = best > 0 ? best : P;
}

// rank of every element within its image (stable ascending order) by counting; the last n land at vals / idx [b][rank - (P - n)]
__global__ __launch_bounds__(256) void sort_tail_kernel(const float* __restrict__ t, int P, const int* __restrict__ n_in,
                                                        float* __restrict__ vals, int* __restrict__ idx) {
  __shared__ uint32_t tile[256];
  const int b = blockIdx.y;
  const int i = blockIdx.x * 256 + threadIdx.x;
  const float* row = t + (size_t)b * P;
  const float xi = i < P ? row[i] : 0.f;
  const uint32_t ki = order_key(xi);
  int rank = 0;
  for (int j0 = 0; j0 < P; j0 += 256) {
    const int j = j0 + threadIdx.x;
    tile[threadIdx.x] = j < P ? order_key(row[j]) : 0u;
    __syncthreads();
    const int m = min(256, P - j0);
    for (int q = 0; q < m; ++q) {
      const uint32_t kj = tile[q];
      rank += (kj < ki) | ((kj == ki) & (j0 + q < i));
    }
    __syncthreads();
  }
  if (i >= P) return;
  const int pos = rank - (P - *n_in);
  if (pos >= 0) {
    vals[(size_t)b * P + pos] = xi;
    idx[(size_t)b * P + pos] = i;
  }
}

// ---------------------------------------------------------------- forward
__global__ __launch_bounds__(256) void sk_zero_kernel(float* __restrict__ u, int nu, float* __restrict__ v, int nv, int* __restrict__ state) {
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t < nu) u[t] = 0.f;
  if (t < nv) v[t] = 0.f;
  if (t < 2) state[t] = 0;
}

// One half-iteration k: for each line i of the "self" side, lse2_i = log2 sum_j exp2((pot_i + opot_j - (p_i - q_j)^2) log2e/eps),
// pot_i <- sk_step(pot_i, log(1/n_self + 1e-8), lse2_i).  delta: the line's |u^k - u^{k-1}| (u half) or v^{k-1} (v half).  A no-op
// after convergence.
// SIDE 0: rows (self = x, u); SIDE 1: columns (self = y, v).  The exponent is always formed as (u_i - C_ij) + v_j.
template <int SIDE>
__global__ __launch_bounds__(256) void sk_lse_kernel(const float* __restrict__ pts, float* __restrict__ pot, int cap,
                                                     const float* __restrict__ opts, const float* __restrict__ opot, int ocap,
                                                     const int* __restrict__ n, float eps, float* __restrict__ hist,
                                                     float* __restrict__ delta, const int* __restrict__ state) {
  if (state[1]) return;
  const int b = blockIdx.y;
  const int ns = n[SIDE], no = n[1 - SIDE];
  const int lane = threadIdx.x & (SK_WAVE - 1);
  const int i0 = blockIdx.x * SK_LINES + (threadIdx.x / SK_WAVE) * SK_RPW;
  if (i0 >= ns) return;
  const float s = SK_LOG2E / eps;
  float p[SK_RPW], ps[SK_RPW];
#pragma unroll
  for (int r = 0; r < SK_RPW; ++r) {
    const int i = min(i0 + r, ns - 1);
    p[r] = pts[(size_t)b * cap + i];
    ps[r] = pot[(size_t)b * cap + i];
  }
  const float* q = opts + (size_t)b * ocap;
  const float* qp = opot + (size_t)b * ocap;
  float m[SK_RPW];
#pragma unroll
  for (int r = 0; r < SK_RPW; ++r) m[r] = -INFINITY;
  for (int j = lane; j < no; j += SK_WAVE) {
    const float qj = q[j], vj = qp[j];
#pragma unroll
    for (int r = 0; r < SK_RPW; ++r) {
      const float d = p[r] - qj;
      m[r] = fmaxf(m[r], SIDE ? sk_w(vj, d, ps[r], s) : sk_w(ps[r], d, vj, s));
    }
  }
  float acc[SK_RPW];
#pragma unroll
  for (int r = 0; r < SK_RPW; ++r) {
    m[r] = wave_max(m[r]);
    acc[r] = 0.f;
  }
  for (int j = lane; j < no; j += SK_WAVE) {
    const float qj = q[j], vj = qp[j];
#pragma unroll
    for (int r = 0; r < SK_RPW; ++r) {
      const float d = p[r] - qj;
      acc[r] += exp2f((SIDE ? sk_w(vj, d, ps[r], s) : sk_w(ps[r], d, vj, s)) - m[r]);
    }
  }
  const float marg = sk_marg(ns);
#pragma unroll
  for (int r = 0; r < SK_RPW; ++r) {
    const float lse2 = m[r] + log2f(wave_sum(acc[r]));
    const int i = i0 + r;
    if (lane == 0 && i < ns) {
      const float nu = sk_step(ps[r], marg, lse2, eps);
      hist[(size_t)b * cap + i] = lse2;
      pot[(size_t)b * cap + i] = nu;
      if (delta) delta[(size_t)b * cap + i] = SIDE ? ps[r] : fabsf(nu - ps[r]);
    }
  }
}

// err_k = mean_b sum_i |u^k_i - u^{k-1}_i| (fixed order); state = {K, done}.  One workgroup.
__global__ __launch_bounds__(256) void sk_err_kernel(const float* __restrict__ delta, int B, int cap, const int* __restrict__ n, int k,
                                                     int* __restrict__ state, float* __restrict__ err_out) {
  __shared__ float red[256];
  if (state[1]) return;
  const int nx = n[0];
  float tot = 0.f;
  for (int b = 0; b < B; ++b) {
    float a = 0.f;
    for (int i = threadIdx.x; i < nx; i += 256) a += delta[(size_t)b * cap + i];
    red[threadIdx.x] = a;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
      if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
      __syncthreads();
    }
    tot += red[0];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const float err = tot / (float)B;
    if (err_out) err_out[k - 1] = err;
    state[0] = k;
    if (err < SK_THRESH) state[1] = 1;
  }
}

// Per line: sum pi_ij C_ij (forward: the cost) -- or, with g (backward seed), ubar_i = g_b sum_j pi C / eps and
// grad_i = +-g_b sum_j pi (1 - C/eps) 2 (x_i - y_j) (rows; for columns 2(p - q) flips the sign by itself).
// pi is formed as exp(M(u^K, v^{K-1}) - R^K_j + b), which is exp(M(u^K, v^K)) since v^K = v^{K-1} + eps (b - R^K): the backward
// then needs only what the replay of iteration K gives.  pot / opot: u^K on the x side, v^{K-1} on the y side; Rh: the saved column
// log-sum-exps, K from state.
template <int SIDE>
__global__ __launch_bounds__(256) void sk_plan_line_kernel(const float* __restrict__ pts, const float* __restrict__ pot, int cap,
                                                           const float* __restrict__ opts, const float* __restrict__ opot, int ocap,
                                                           const int* __restrict__ n, float eps, const float* __restrict__ Rh, int B,
                                                           const int* __restrict__ state, float* __restrict__ cost_line,
                                                           const float* __restrict__ g, float* __restrict__ bar, float* __restrict__ grad) {
  const int b = blockIdx.y;
  const int ns = n[SIDE], no = n[1 - SIDE];
  const int lane = threadIdx.x & (SK_WAVE - 1);
  const int i0 = blockIdx.x * SK_LINES + (threadIdx.x / SK_WAVE) * SK_RPW;
  if (i0 >= ns) return;
  const float s = SK_LOG2E / eps, ie = 1.f / eps;
  const float bl2 = __fmul_rn(sk_marg(n[1]), SK_LOG2E);
  const float* Rk = Rh + ((size_t)(state[0] - 1) * B + b) * (SIDE ? cap : ocap);
  float p[SK_RPW], ps[SK_RPW], rs[SK_RPW], a[SK_RPW], gg[SK_RPW];
#pragma unroll
  for (int r = 0; r < SK_RPW; ++r) {
    const int i = min(i0 + r, ns - 1);
    p[r] = pts[(size_t)b * cap + i];
    ps[r] = pot[(size_t)b * cap + i];
    rs[r] = SIDE ? Rk[i] : 0.f;
    a[r] = 0.f;
    gg[r] = 0.f;
  }
  const float* q = opts + (size_t)b * ocap;
  const float* qp = opot + (size_t)b * ocap;
  for (int j = lane; j < no; j += SK_WAVE) {
    const float qj = q[j], vj = qp[j], rj = SIDE ? 0.f : Rk[j];
#pragma unroll
    for (int r = 0; r < SK_RPW; ++r) {
      const float d = p[r] - qj, c = d * d;
      const float pi = exp2f((SIDE ? sk_w(vj, d, ps[r], s) - rs[r] : sk_w(ps[r], d, vj, s) - rj) + bl2);
      a[r] += pi * c;
      if (g) gg[r] += pi * (1.f - c * ie) * (2.f * d);
    }
  }
#pragma unroll
  for (int r = 0; r < SK_RPW; ++r) {
    const float sa = wave_sum(a[r]);
    const float sg = g ? wave_sum(gg[r]) : 0.f;
    const int i = i0 + r;
    if (lane == 0 && i < ns) {
      if (cost_line) cost_line[(size_t)b * cap + i] = sa;
      if (g) {
        bar[(size_t)b * cap + i] = g[b] * sa * ie;
        if (grad) grad[(size_t)b * cap + i] = g[b] * sg;
      }
    }
  }
}

// cost[b] = sum_i cost_line[b][i] in a fixed order (one workgroup per image)
__global__ __launch_bounds__(256) void sk_cost_kernel(const float* __restrict__ cost_line, int cap, const int* __restrict__ n,
                                                      float* __restrict__ cost) {
  __shared__ float red[256];
  const int b = blockIdx.x, nx = n[0];
  float a = 0.f;
  for (int i = threadIdx.x; i < nx; i += 256) a += cost_line[(size_t)b * cap + i];
  red[threadIdx.x] = a;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
    __syncthreads();
  }
  if (threadIdx.x == 0) cost[b] = red[0];
}

// ---------------------------------------------------------------- backward
// u^{k-1}, u^k (rows) and v^{k-1} (columns) of iteration k, replayed from the saved log-sum-exps
__global__ __launch_bounds__(256) void sk_replay_kernel(const float* __restrict__ hL, const float* __restrict__ hR, int B, int capx, int capy,
                                                        const int* __restrict__ n, float eps, int k, const int* __restrict__ state,
                                                        float* __restrict__ uprev, float* __restrict__ ucur, float* __restrict__ vprev) {
  if (k <= 0) k = state[0];          // (the seed of the backward: iteration K)
  if (k > state[0]) return;
  const int b = blockIdx.y, t = blockIdx.x * 256 + threadIdx.x;
  const int nx = n[0], ny = n[1];
  if (t < nx) {
    const float a = sk_marg(nx);
    float u = 0.f, up = 0.f;
    for (int it = 0; it < k; ++it) {
      up = u;
      u = sk_step(u, a, hL[((size_t)it * B + b) * capx + t], eps);
    }
    uprev[(size_t)b * capx + t] = up;
    ucur[(size_t)b * capx + t] = u;
  }
  if (t < ny) {
    const float bb = sk_marg(ny);
    float v = 0.f;
    for (int it = 0; it < k - 1; ++it) v = sk_step(v, bb, hR[((size_t)it * B + b) * capy + t], eps);
    vprev[(size_t)b * capy + t] = v;
  }
}

// The reverse sweep's sums run in fp64 (P and Q themselves in fp32): at k = K the seed's direct term and the term through the last
// v update cancel to ~1e-4 of themselves where a point lies far from the other cloud, and fp32 line sums left 2e-4 of the largest
// gradient there (G18 sd_b4_mean_eps01; fp64 sums: 1e-5, the reference's own fp32 autograd: 7e-5).
// Rows of iteration k:  P_ij = exp(M(u^{k-1}, v^{k-1}) - L^k_i),  Q_ij = exp(M(u^k, v^{k-1}) - R^k_j)
//   ubar^k_i = [k == K] ubar_i - sum_j Q_ij vbar^k_j
//   gx_i += sum_j Q_ij vbar^k_j 2(x_i - y_j) + ubar^k_i sum_j P_ij 2(x_i - y_j)
__global__ __launch_bounds__(256) void sk_bwd_row_kernel(const float* __restrict__ x, const float* __restrict__ y, int capx, int capy,
                                                         const int* __restrict__ n, float eps, int k, const int* __restrict__ state,
                                                         const float* __restrict__ uprev, const float* __restrict__ ucur,
                                                         const float* __restrict__ vprev, const float* __restrict__ L2,
                                                         const float* __restrict__ R2, const float* __restrict__ vbar,
                                                         float* __restrict__ ubar, float* __restrict__ gx) {
  const int K = state[0];
  if (k > K) return;
  const int b = blockIdx.y, nx = n[0], ny = n[1];
  const int lane = threadIdx.x & (SK_WAVE - 1);
  const int i0 = blockIdx.x * SK_LINES + (threadIdx.x / SK_WAVE) * SK_RPW;
  if (i0 >= nx) return;
  const float s = SK_LOG2E / eps;
  float xi[SK_RPW], up[SK_RPW], uc[SK_RPW], li[SK_RPW];
  double s1[SK_RPW], s2[SK_RPW], s3[SK_RPW];
#pragma unroll
  for (int r = 0; r < SK_RPW; ++r) {
    const size_t o = (size_t)b * capx + min(i0 + r, nx - 1);
    xi[r] = x[o];
    up[r] = uprev[o];
    uc[r] = ucur[o];
    li[r] = L2[o];
    s1[r] = s2[r] = s3[r] = 0.0;
  }
  const size_t ob = (size_t)b * capy;
  for (int j = lane; j < ny; j += SK_WAVE) {
    const float yj = y[ob + j], vj = vprev[ob + j], rj = R2[ob + j], vb = vbar[ob + j];
#pragma unroll
    for (int r = 0; r < SK_RPW; ++r) {
      const float d = xi[r] - yj;
      const float P = exp2f(sk_w(up[r], d, vj, s) - li[r]);
      const float Q = exp2f(sk_w(uc[r], d, vj, s) - rj);
      const double qv = (double)Q * vb;
      s1[r] += qv;
      s2[r] += qv * (2.0 * d);
      s3[r] += (double)P * (2.0 * d);
    }
  }
#pragma unroll
  for (int r = 0; r < SK_RPW; ++r) {
    const double t1 = wave_sum_d(s1[r]), t2 = wave_sum_d(s2[r]), t3 = wave_sum_d(s3[r]);
    const int i = i0 + r;
    if (lane == 0 && i < nx) {
      const size_t o = (size_t)b * capx + i;
      const double ub = (k == K ? (double)ubar[o] : 0.0) - t1;
      ubar[o] = (float)ub;
      gx[o] = (float)((double)gx[o] + t2 + ub * t3);
    }
  }
}

// Columns of iteration k:  vbar^{k-1}_j = -sum_i P_ij ubar^k_i,
//   gy_j -= vbar^k_j sum_i Q_ij 2(x_i - y_j) + sum_i P_ij ubar^k_i 2(x_i - y_j)     (gy may be null)
__global__ __launch_bounds__(256) void sk_bwd_col_kernel(const float* __restrict__ x, const float* __restrict__ y, int capx, int capy,
                                                         const int* __restrict__ n, float eps, int k, const int* __restrict__ state,
                                                         const float* __restrict__ uprev, const float* __restrict__ ucur,
                                                         const float* __restrict__ vprev, const float* __restrict__ L2,
                                                         const float* __restrict__ R2, const float* __restrict__ ubar,
                                                         float* __restrict__ vbar, float* __restrict__ gy) {
  if (k > state[0]) return;
  const int b = blockIdx.y, nx = n[0], ny = n[1];
  const int lane = threadIdx.x & (SK_WAVE - 1);
  const int j0 = blockIdx.x * SK_LINES + (threadIdx.x / SK_WAVE) * SK_RPW;
  if (j0 >= ny) return;
  const float s = SK_LOG2E / eps;
  float yj[SK_RPW], vj[SK_RPW], rj[SK_RPW];
  double t1[SK_RPW], t2[SK_RPW], t3[SK_RPW];
#pragma unroll
  for (int r = 0; r < SK_RPW; ++r) {
    const size_t o = (size_t)b * capy + min(j0 + r, ny - 1);
    yj[r] = y[o];
    vj[r] = vprev[o];
    rj[r] = R2[o];
    t1[r] = t2[r] = t3[r] = 0.0;
  }
  const size_t ob = (size_t)b * capx;
  for (int i = lane; i < nx; i += SK_WAVE) {
    const float xi = x[ob + i], up = uprev[ob + i], uc = ucur[ob + i], li = L2[ob + i], ub = ubar[ob + i];
#pragma unroll
    for (int r = 0; r < SK_RPW; ++r) {
      const float d = xi - yj[r];
      const float P = exp2f(sk_w(up, d, vj[r], s) - li);
      const float Q = exp2f(sk_w(uc, d, vj[r], s) - rj[r]);
      const double pu = (double)P * ub;
      t1[r] += pu;
      t2[r] += (double)Q * (2.0 * d);
      t3[r] += pu * (2.0 * d);
    }
  }
#pragma unroll
  for (int r = 0; r < SK_RPW; ++r) {
    const double a1 = wave_sum_d(t1[r]);
    const double a2 = gy ? wave_sum_d(t2[r]) : 0.0, a3 = gy ? wave_sum_d(t3[r]) : 0.0;
    const int j = j0 + r;
    if (lane == 0 && j < ny) {
      const size_t o = (size_t)b * capy + j;
      if (gy) gy[o] = (float)((double)gy[o] - ((double)vbar[o] * a2 + a3));
      vbar[o] = (float)-a1;
    }
  }
}

// pi and C materialised, [B][n_x][n_y] (SinkhornDistance's second and third outputs only)
__global__ __launch_bounds__(256) void sk_plan_kernel(const float* __restrict__ x, const float* __restrict__ y, const float* __restrict__ u,
                                                      const float* __restrict__ v, int B, int nx, int ny, float eps,
                                                      float* __restrict__ pi, float* __restrict__ Cm) {
  const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
  const size_t per = (size_t)nx * ny;
  if (t >= per * B) return;
  const int b = (int)(t / per);
  const int i = (int)((t % per) / ny), j = (int)(t % ny);
  const float d = x[(size_t)b * nx + i] - y[(size_t)b * ny + j];
  Cm[t] = d * d;
  pi[t] = exp2f(sk_w(u[(size_t)b * nx + i], d, v[(size_t)b * ny + j], SK_LOG2E / eps));
}

__global__ __launch_bounds__(256) void scatter_kernel(const float* __restrict__ g, const int* __restrict__ idx, int P,
                                                      const int* __restrict__ n_in, float* __restrict__ out) {
  const int b = blockIdx.y, p = blockIdx.x * 256 + threadIdx.x;
  if (p >= *n_in) return;
  const int src = idx[(size_t)b * P + p];
  if (src >= 0 && src < P) out[(size_t)b * P + src] = g[(size_t)b * P + p];
}

bool sk_dims_ok(int B, int capx, int capy, float eps, int max_iter) {
  return B > 0 && capx > 0 && capy > 0 && B <= 65535 && (int64_t)capx + SK_LINES <= 0x7fffffff && (int64_t)capy + SK_LINES <= 0x7fffffff &&
         eps > 0.f && eps < INFINITY && max_iter > 0;
}

// SRK_POISON_LDS=1 (test runs): NaN bit patterns into every CU's LDS in front of EVERY launch of the entry points below
bool sk_poison() {
  const char* e = getenv("SRK_POISON_LDS");
  return e && e[0] == '1';
}

}  // namespace

#define SK_POISON() \
  do {              \
    if (poison) srk_debug_poison_lds(st); \
  } while (0)

extern "C" int srk_sort_cut(const float* t, int B, int P, float threshold, float* vals, int* idx, int* n_out, void* stream) {
  if (!t || !vals || !idx || !n_out || B <= 0 || P <= 0 || B > 65535 || P > SRK_SORT_CUT_MAX) return SRK_ERR_BAD_ARG;
  hipStream_t st = (hipStream_t)stream;
  const bool poison = sk_poison();
  SK_POISON();
  hipLaunchKernelGGL(sort_count_kernel, dim3(1), dim3(256), 0, st, t, B, P, threshold, n_out);
  SRK_CHECK_LAUNCH();
  SK_POISON();
  hipLaunchKernelGGL(sort_tail_kernel, dim3(srk_div_up(P, 256), B), dim3(256), 0, st, t, P, (const int*)n_out, vals, idx);
  SRK_CHECK_LAUNCH();
  return SRK_OK;
}

extern "C" int srk_sinkhorn_fwd(const float* x, const float* y, const int* n, int B, int cap_x, int cap_y, float eps, int max_iter,
                                float* u, float* v, float* hist_L, float* hist_R, float* work, int* state, float* err, float* cost,
                                void* stream) {
  if (!x || !y || !n || !u || !v || !hist_L || !hist_R || !work || !state || !cost || !sk_dims_ok(B, cap_x, cap_y, eps, max_iter))
    return SRK_ERR_BAD_ARG;
  hipStream_t st = (hipStream_t)stream;
  const bool poison = sk_poison();
  const int nu = B * cap_x, nv = B * cap_y;
  float* vprev = work + (size_t)B * cap_x;     // v^{k-1} of the last iteration that ran
  SK_POISON();
  hipLaunchKernelGGL(sk_zero_kernel, dim3(srk_div_up(max(max(nu, nv), 2), 256)), dim3(256), 0, st, u, nu, v, nv, state);
  SRK_CHECK_LAUNCH();
  const dim3 gx(srk_div_up(cap_x, SK_LINES), B), gy(srk_div_up(cap_y, SK_LINES), B);
  for (int k = 1; k <= max_iter; ++k) {
    float* hL = hist_L + (size_t)(k - 1) * B * cap_x;
    float* hR = hist_R + (size_t)(k - 1) * B * cap_y;
    SK_POISON();
    hipLaunchKernelGGL(sk_lse_kernel<0>, gx, dim3(256), 0, st, x, u, cap_x, y, (const float*)v, cap_y, n, eps, hL, work, (const int*)state);
    SRK_CHECK_LAUNCH();
    SK_POISON();
    hipLaunchKernelGGL(sk_lse_kernel<1>, gy, dim3(256), 0, st, y, v, cap_y, x, (const float*)u, cap_x, n, eps, hR, vprev,
                       (const int*)state);
    SRK_CHECK_LAUNCH();
    SK_POISON();
    hipLaunchKernelGGL(sk_err_kernel, dim3(1), dim3(256), 0, st, (const float*)work, B, cap_x, n, k, state, err);
    SRK_CHECK_LAUNCH();
  }
  SK_POISON();
  hipLaunchKernelGGL(sk_plan_line_kernel<0>, gx, dim3(256), 0, st, x, (const float*)u, cap_x, y, (const float*)vprev, cap_y, n, eps,
                     (const float*)hist_R, B, (const int*)state, work, (const float*)nullptr, (float*)nullptr, (float*)nullptr);
  SRK_CHECK_LAUNCH();
  SK_POISON();
  hipLaunchKernelGGL(sk_cost_kernel, dim3(B), dim3(256), 0, st, (const float*)work, cap_x, n, cost);
  SRK_CHECK_LAUNCH();
  return SRK_OK;
}

extern "C" int srk_sinkhorn_bwd(const float* x, const float* y, const int* n, int B, int cap_x, int cap_y, float eps, int max_iter,
                                const float* hist_L, const float* hist_R, const int* state, const float* g_cost, float* gx, float* gy,
                                float* work, void* stream) {
  if (!x || !y || !n || !hist_L || !hist_R || !state || !g_cost || !gx || !work || !sk_dims_ok(B, cap_x, cap_y, eps, max_iter))
    return SRK_ERR_BAD_ARG;
  hipStream_t st = (hipStream_t)stream;
  const bool poison = sk_poison();
  float* ubar = work;
  float* uprev = ubar + (size_t)B * cap_x;
  float* ucur = uprev + (size_t)B * cap_x;
  float* vbar = ucur + (size_t)B * cap_x;
  float* vprev = vbar + (size_t)B * cap_y;
  const dim3 gX(srk_div_up(cap_x, SK_LINES), B), gY(srk_div_up(cap_y, SK_LINES), B);
  // seed: the cost's own dependence on C, u^K, v^K
  const dim3 gR(srk_div_up(max(cap_x, cap_y), 256), B);
  SK_POISON();
  hipLaunchKernelGGL(sk_replay_kernel, gR, dim3(256), 0, st, hist_L, hist_R, B, cap_x, cap_y, n, eps, 0, state, uprev, ucur, vprev);
  SRK_CHECK_LAUNCH();
  SK_POISON();
  hipLaunchKernelGGL(sk_plan_line_kernel<0>, gX, dim3(256), 0, st, x, (const float*)ucur, cap_x, y, (const float*)vprev, cap_y, n, eps,
                     hist_R, B, state, (float*)nullptr, g_cost, ubar, gx);
  SRK_CHECK_LAUNCH();
  SK_POISON();
  hipLaunchKernelGGL(sk_plan_line_kernel<1>, gY, dim3(256), 0, st, y, (const float*)vprev, cap_y, x, (const float*)ucur, cap_x, n, eps,
                     hist_R, B, state, (float*)nullptr, g_cost, vbar, gy);
  SRK_CHECK_LAUNCH();
  for (int k = max_iter; k >= 1; --k) {
    const float* hL = hist_L + (size_t)(k - 1) * B * cap_x;
    const float* hR = hist_R + (size_t)(k - 1) * B * cap_y;
    SK_POISON();
    hipLaunchKernelGGL(sk_replay_kernel, gR, dim3(256), 0, st, hist_L, hist_R, B, cap_x, cap_y, n, eps, k, state, uprev, ucur, vprev);
    SRK_CHECK_LAUNCH();
    SK_POISON();
    hipLaunchKernelGGL(sk_bwd_row_kernel, gX, dim3(256), 0, st, x, y, cap_x, cap_y, n, eps, k, state, (const float*)uprev,
                       (const float*)ucur, (const float*)vprev, hL, hR, (const float*)vbar, ubar, gx);
    SRK_CHECK_LAUNCH();
    SK_POISON();
    hipLaunchKernelGGL(sk_bwd_col_kernel, gY, dim3(256), 0, st, x, y, cap_x, cap_y, n, eps, k, state, (const float*)uprev,
                       (const float*)ucur, (const float*)vprev, hL, hR, (const float*)ubar, vbar, gy);
    SRK_CHECK_LAUNCH();
  }
  return SRK_OK;
}

extern "C" int srk_sinkhorn_plan(const float* x, const float* y, const float* u, const float* v, int B, int n_x, int n_y, float eps,
                                 float* pi, float* cost_matrix, void* stream) {
  if (!x || !y || !u || !v || !pi || !cost_matrix || !sk_dims_ok(B, n_x, n_y, eps, 1)) return SRK_ERR_BAD_ARG;
  const size_t tot = (size_t)B * n_x * n_y;
  if (tot / 256 + 1 > 0x7fffffffu) return SRK_ERR_UNSUPPORTED;
  hipStream_t st = (hipStream_t)stream;
  const bool poison = sk_poison();
  SK_POISON();
  hipLaunchKernelGGL(sk_plan_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, st, x, y, u, v, B, n_x, n_y, eps,
                     pi, cost_matrix);
  SRK_CHECK_LAUNCH();
  return SRK_OK;
}

extern "C" int srk_scatter_rows(const float* g, const int* idx, const int* n, int B, int P, float* out, void* stream) {
  if (!g || !idx || !n || !out || B <= 0 || P <= 0 || B > 65535 || P > SRK_SORT_CUT_MAX) return SRK_ERR_BAD_ARG;
  hipStream_t st = (hipStream_t)stream;
  const bool poison = sk_poison();
  if (hipMemsetAsync(out, 0, (size_t)B * P * sizeof(float), st) != hipSuccess) return SRK_ERR_LAUNCH;
  SK_POISON();
  hipLaunchKernelGGL(scatter_kernel, dim3(srk_div_up(P, 256), B), dim3(256), 0, st, g, idx, P, n, out);
  SRK_CHECK_LAUNCH();
  return SRK_OK;
}
