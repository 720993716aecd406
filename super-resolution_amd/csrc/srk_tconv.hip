// nn.ConvTranspose2d(Cin, Cout, kernel_size=2, stride=2) on fp32 MFMAs: forward, data gradient, weight / bias gradient
// (the reference's transposed-conv upsampling stages, models.py:69-83).  NCHW in, NCHW out, PyTorch's [Cin, Cout, 2, 2] weights.
//
// Kernel 2 / stride 2 / no padding: output pixel (2i+a, 2j+b) depends on input pixel (i, j) alone, so with m = 4 co + 2 a + b
//   forward   y[n, m, (i, j)]  = bias[co] + sum_ci x[n, ci, i, j] W[ci, m]        GEMM [P, Cin] x [Cin, 4 Cout], P = N H W
//   dgrad     dx[n, ci, i, j]  = sum_m dy[n, m, (i, j)] W[ci, m]                 GEMM [P, 4 Cout] x [4 Cout, Cin]
//   wgrad     dW[ci, m]        = sum_p x[n, ci, i, j] dy[n, m, (i, j)]           GEMM [Cin, P] x [P, 4 Cout], split over P
// where dy[n, m, (i, j)] is dy[n, co, 2i + a, 2j + b].
//
// Forward and dgrad share one kernel: a wave owns 32 input pixels (the MFMA's columns: one pixel per lane) and up to 8 tiles of 32
// GEMM outputs (the rows); the weights of a 32-deep K slice sit in LDS, the activations go from global memory straight into the
// B operand (32 consecutive pixels per half-wave).  The forward's accumulator rows 4g..4g+3 of a lane are the 2 x 2 sub-pixels of one
// output channel, stored as two float2 (the two output rows); the dgrad stores one coalesced row of 32 pixels per register.
// The weight gradient stages 32-pixel chunks of x and dy in LDS (pixel-major, so the MFMA operand reads are conflict-free), every
// workgroup of a split writes its partial [Cin, 4 Cout] tile (+ the partial bias sums), and a second kernel adds the splits in a
// fixed order: two runs give bit-identical dW / db.
#include "srk_internal.h"

namespace {

constexpr int TC_WAVES = 8;                 // fwd / dgrad: waves per workgroup, 32 pixels each
constexpr int TC_THREADS = 64 * TC_WAVES;
constexpr int TC_KC = 32;                   // K depth of one LDS weight slice

// act: x [N, Cin, H, W] (forward) or dy [N, Cout, 2H, 2W] (dgrad); w: [Cin, 4 Cout]; out: y [N, Cout, 2H, 2W] or dx [N, Cin, H, W]
template <int NT, bool DGRAD>
__global__ __launch_bounds__(TC_THREADS) void tconv2x2_gemm_kernel(const float* __restrict__ act, const float* __restrict__ w,
                                                                   const float* __restrict__ bias, float* __restrict__ out,
                                                                   int N, int H, int W, int Cin, int Cout, float slope) {
  constexpr int MT = NT * 32;               // GEMM outputs per workgroup
  constexpr int WLS = MT + 1;               // LDS row stride (odd: the dgrad's transposing writes are conflict-free)
  __shared__ float wl[TC_KC * WLS];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, h = lane >> 5, col = lane & 31;
  const int HW = H * W;
  const int64_t P = (int64_t)N * HW;
  const int64_t p = ((int64_t)blockIdx.x * TC_WAVES + wave) * 32 + col;
  const bool pok = p < P;
  const int64_t n = pok ? p / HW : 0;
  const int r = pok ? (int)(p - n * HW) : 0;
  const int i = r / W, j = r - (r / W) * W;
  const int M = DGRAD ? Cin : 4 * Cout;
  const int K = DGRAD ? 4 * Cout : Cin;
  const int m0 = blockIdx.y * MT;
  // lane half h supplies k = k0 + h of each k pair; in the dgrad that is the sub-pixel column b
  const float* abase = DGRAD ? act + n * Cout * 4 * HW + (int64_t)(2 * i) * (2 * W) + 2 * j + h : act + n * Cin * HW + r;
  f32x16 acc[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) acc[t] = f32x16{};
  for (int kc = 0; kc < K; kc += TC_KC) {
    __syncthreads();
    for (int e = threadIdx.x; e < TC_KC * MT; e += TC_THREADS) {
      int kk, mm;
      if (DGRAD) { kk = e % TC_KC; mm = e / TC_KC; } else { kk = e / MT; mm = e % MT; }    // global reads along W's rows
      const int k = kc + kk, m = m0 + mm;
      float v = 0.f;
      if (k < K && m < M) v = DGRAD ? w[(int64_t)m * K + k] : w[(int64_t)k * M + m];
      wl[kk * WLS + mm] = v;
    }
    __syncthreads();
    const int steps = min(TC_KC, K - kc + 1) / 2;   // k pairs of this slice that hold real K rows (wave-uniform)
    float b[TC_KC / 2];
#pragma unroll
    for (int s = 0; s < TC_KC / 2; ++s) {
      const int k = kc + 2 * s + h;
      float v = 0.f;
      if (pok && k < K) v = DGRAD ? abase[(int64_t)(k >> 2) * 4 * HW + ((k >> 1) & 1) * 2 * W] : abase[(int64_t)k * HW];
      b[s] = v;
    }
#pragma unroll
    for (int s = 0; s < TC_KC / 2; ++s) {
      if (s < steps) {
#pragma unroll
        for (int t = 0; t < NT; ++t)
          acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(wl[(2 * s + h) * WLS + t * 32 + col], b[s], acc[t], 0, 0, 0);
      }
    }
  }
  if (!pok) return;
  // D: column = pixel (lane & 31), row = 8g + 4h + q in register 4g + q
#pragma unroll
  for (int t = 0; t < NT; ++t) {
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const int mr = m0 + t * 32 + 8 * g + 4 * h;
      if (DGRAD) {
#pragma unroll
        for (int q = 0; q < 4; ++q)
          if (mr + q < Cin) out[(n * Cin + mr + q) * HW + r] = acc[t][4 * g + q];
      } else {
        const int co = mr >> 2;
        if (co >= Cout) continue;
        const float bv = bias ? bias[co] : 0.f;
        float v[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          v[q] = acc[t][4 * g + q] + bv;
          if (slope != 1.f) v[q] = v[q] > 0.f ? v[q] : v[q] * slope;
        }
        float* yp = out + ((n * Cout + co) * 2 * H + 2 * i) * (int64_t)(2 * W) + 2 * j;
        *reinterpret_cast<float2*>(yp) = make_float2(v[0], v[1]);
        *reinterpret_cast<float2*>(yp + 2 * W) = make_float2(v[2], v[3]);
      }
    }
  }
}

constexpr int WG_THREADS = 256;
constexpr int WG_PC = 32;                   // pixels per LDS chunk
constexpr int WG_CT = 64;                   // input channels per workgroup tile
constexpr int WG_KT = 256;                  // GEMM columns m = 4 co + 2 a + b per workgroup tile (64 output channels)
constexpr int WG_XS = WG_CT + 1;            // LDS row strides: x rows are written by 32 pixels (odd stride), dy rows by 16 pixel
constexpr int WG_DS = WG_KT + 2;            // pairs (stride = 2 mod 32): both conflict-free
constexpr int WG_TARGET_BLOCKS = 512;

struct WgradPlan { int ci_tiles, k_tiles, chunks, cps, splits; };

WgradPlan wgrad_plan(int N, int H, int W, int Cin, int Cout) {
  WgradPlan pl;
  pl.ci_tiles = srk_div_up(Cin, WG_CT);
  pl.k_tiles = srk_div_up(4 * Cout, WG_KT);
  const int64_t P = (int64_t)N * H * W;
  pl.chunks = (int)((P + WG_PC - 1) / WG_PC);
  int want = WG_TARGET_BLOCKS / (pl.ci_tiles * pl.k_tiles);
  want = want < 1 ? 1 : want;
  const int by_len = srk_div_up(pl.chunks, 4);       // at least 4 chunks per split where the problem allows it
  if (want > by_len) want = by_len;
  pl.cps = srk_div_up(pl.chunks, want);
  pl.splits = srk_div_up(pl.chunks, pl.cps);
  return pl;
}

// partial sums of split blockIdx.x: pw[split][Cin][4 Cout], pb[split][4 Cout] (pb from the ci-tile 0 workgroups only)
__global__ __launch_bounds__(WG_THREADS) void tconv2x2_wgrad_kernel(const float* __restrict__ x, const float* __restrict__ dy,
                                                                    int N, int H, int W, int Cin, int Cout, int cps,
                                                                    float* __restrict__ pw, float* __restrict__ pb) {
  __shared__ float xl[WG_PC * WG_XS];
  __shared__ float dl[WG_PC * WG_DS];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, h = lane >> 5, col = lane & 31;
  const int HW = H * W, K4 = 4 * Cout;
  const int64_t P = (int64_t)N * HW;
  const int ci0 = blockIdx.y * WG_CT, k0 = blockIdx.z * WG_KT;
  const int split = blockIdx.x;
  // wave: one 32-channel half of the ci tile x four 32-column tiles of the m tile
  const int wci = ci0 + (wave >> 1) * 32, wk = k0 + (wave & 1) * 128;
  const bool wave_live = wci < Cin;
  f32x16 acc[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) acc[t] = f32x16{};
  float dbacc = 0.f;
  const int64_t pbeg = (int64_t)split * cps * WG_PC;
  const int64_t pend = min(P, pbeg + (int64_t)cps * WG_PC);
  // chunk staging, software-pipelined: the global loads of chunk c + 1 go out into registers before the MFMAs of chunk c
  float xr[WG_CT / 8], dr[WG_KT / 8];
  const int xpx = tid & 31;                                 // x: pixel tid & 31, channels (tid >> 5) + 8 q
  const int dpx = (tid & 63) >> 1, db_b = tid & 1;          // dy: pixel, column b, rows (co, a) = (tid >> 6) + 4 q
  auto load = [&](int64_t pc) {
    {
      const int64_t p = pc + xpx;
      const bool ok = p < pend;
      const int64_t n = ok ? p / HW : 0;
      const int r = ok ? (int)(p - n * HW) : 0;
      const float* xb = x + n * Cin * HW + r;
#pragma unroll
      for (int q = 0; q < WG_CT / 8; ++q) {
        const int ci = ci0 + (tid >> 5) + 8 * q;
        xr[q] = (ok && ci < Cin) ? xb[(int64_t)ci * HW] : 0.f;
      }
    }
    {
      const int64_t p = pc + dpx;
      const bool ok = p < pend;
      const int64_t n = ok ? p / HW : 0;
      const int r = ok ? (int)(p - n * HW) : 0;
      const int i = r / W, j = r - (r / W) * W;
      const float* dyb = dy + n * Cout * 4 * HW + (int64_t)(2 * i) * (2 * W) + 2 * j + db_b;
#pragma unroll
      for (int q = 0; q < WG_KT / 8; ++q) {            // WG_KT / 2 rows (co, a), 4 per pass
        const int row = (tid >> 6) + 4 * q;            // = 2 co_local + a
        const int co = (k0 >> 2) + (row >> 1), a = row & 1;
        dr[q] = (ok && co < Cout) ? dyb[(int64_t)co * 4 * HW + a * 2 * W] : 0.f;
      }
    }
  };
  if (pbeg < pend) load(pbeg);
  for (int64_t pc = pbeg; pc < pend; pc += WG_PC) {
    __syncthreads();
#pragma unroll
    for (int q = 0; q < WG_CT / 8; ++q) xl[xpx * WG_XS + (tid >> 5) + 8 * q] = xr[q];
#pragma unroll
    for (int q = 0; q < WG_KT / 8; ++q) dl[dpx * WG_DS + 2 * ((tid >> 6) + 4 * q) + db_b] = dr[q];
    __syncthreads();
    if (pc + WG_PC < pend) load(pc + WG_PC);
    if (blockIdx.y == 0) {
#pragma unroll 8
      for (int px = 0; px < WG_PC; ++px) dbacc += dl[px * WG_DS + tid];
    }
    if (wave_live) {
#pragma unroll
      for (int s = 0; s < WG_PC / 2; ++s) {
        const float av = xl[(2 * s + h) * WG_XS + (wci - ci0) + col];
#pragma unroll
        for (int t = 0; t < 4; ++t)
          if (wk + t * 32 < K4)
            acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, dl[(2 * s + h) * WG_DS + (wk - k0) + t * 32 + col], acc[t], 0, 0, 0);
      }
    }
  }
  float* pws = pw + (int64_t)split * Cin * K4;
  if (wave_live) {
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const int k = wk + t * 32 + col;
      if (k >= K4) continue;
#pragma unroll
      for (int g = 0; g < 4; ++g)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int ci = wci + 8 * g + 4 * h + q;
          if (ci < Cin) pws[(int64_t)ci * K4 + k] = acc[t][4 * g + q];
        }
    }
  }
  if (blockIdx.y == 0 && k0 + tid < K4) pb[(int64_t)split * K4 + k0 + tid] = dbacc;
}

constexpr int RD_PARTS = 8;                 // reduce: 8 groups of splits x 32 outputs per workgroup

// dw[e] = scale * sum over splits (+ dw[e]), e < Cin * 4 Cout; db[co] likewise from the partial column sums of its 4 sub-pixels.
// Split s goes to group s * RD_PARTS / splits; groups are added in order: a fixed summation tree.
__global__ __launch_bounds__(256) void tconv2x2_wgrad_reduce_kernel(const float* __restrict__ pw, const float* __restrict__ pb,
                                                                    int splits, int Cin, int Cout, float* __restrict__ dw,
                                                                    float* __restrict__ db, float scale, int accumulate) {
  __shared__ float part[RD_PARTS][32];
  const int K4 = 4 * Cout;
  const int64_t nw = (int64_t)Cin * K4;
  const int64_t ntot = nw + (db ? Cout : 0);
  const int c = threadIdx.x & 31, g = threadIdx.x >> 5;
  const int64_t e = (int64_t)blockIdx.x * 32 + c;
  const int sb = (int)((int64_t)splits * g / RD_PARTS), se = (int)((int64_t)splits * (g + 1) / RD_PARTS);
  float s = 0.f;
  if (e < nw) {
    for (int sp = sb; sp < se; ++sp) s += pw[(int64_t)sp * nw + e];
  } else if (e < ntot) {
    const int co = (int)(e - nw);
    for (int sp = sb; sp < se; ++sp) {
      const float* q = pb + (int64_t)sp * K4 + 4 * co;
      s += (q[0] + q[1]) + (q[2] + q[3]);
    }
  }
  part[g][c] = s;
  __syncthreads();
  if (g != 0 || e >= ntot) return;
  float t = part[0][c];
#pragma unroll
  for (int q = 1; q < RD_PARTS; ++q) t += part[q][c];
  t *= scale;
  float* dst = e < nw ? dw + e : db + (e - nw);
  *dst = accumulate ? *dst + t : t;
}

template <bool DGRAD>
int launch_gemm(const float* act, const float* w, const float* bias, float* out, int N, int H, int W, int Cin, int Cout, float slope,
                hipStream_t st) {
  const int M = DGRAD ? Cin : 4 * Cout;
  const int64_t P = (int64_t)N * H * W;
  const int64_t gx = (P + TC_WAVES * 32 - 1) / (TC_WAVES * 32);
  if (gx > 0x7fffffff) return SRK_ERR_UNSUPPORTED;
  const int nt = M <= 64 ? 2 : (M <= 128 ? 4 : 8);
  dim3 grid((unsigned)gx, srk_div_up(M, nt * 32));
  if (grid.y > 65535) return SRK_ERR_UNSUPPORTED;
  if (nt == 2) hipLaunchKernelGGL((tconv2x2_gemm_kernel<2, DGRAD>), grid, dim3(TC_THREADS), 0, st, act, w, bias, out, N, H, W, Cin, Cout, slope);
  else if (nt == 4) hipLaunchKernelGGL((tconv2x2_gemm_kernel<4, DGRAD>), grid, dim3(TC_THREADS), 0, st, act, w, bias, out, N, H, W, Cin, Cout, slope);
  else hipLaunchKernelGGL((tconv2x2_gemm_kernel<8, DGRAD>), grid, dim3(TC_THREADS), 0, st, act, w, bias, out, N, H, W, Cin, Cout, slope);
  SRK_CHECK_LAUNCH();
  return SRK_OK;
}

bool dims_ok(int N, int H, int W, int Cin, int Cout) {
  // element offsets are 64-bit; per-image planes and the pixel count of one launch must fit the 32-bit index math
  return N > 0 && H > 0 && W > 0 && Cin > 0 && Cout > 0 && (int64_t)4 * H * W <= 0x7fffffff && (int64_t)4 * Cout <= 0x7fffffff;
}

}  // namespace

size_t srk_tconv2x2_wgrad_ws_bytes(int N, int H, int W, int Cin, int Cout) {
  const WgradPlan pl = wgrad_plan(N, H, W, Cin, Cout);
  return (size_t)pl.splits * ((size_t)Cin * 4 * Cout + (size_t)4 * Cout) * sizeof(float);
}

extern "C" int srk_tconv2x2_fwd(const float* x, const float* w, const float* bias, float* y, int N, int H, int W, int Cin, int Cout,
                                float slope, void* stream) {
  if (!x || !w || !y || !dims_ok(N, H, W, Cin, Cout)) return SRK_ERR_BAD_ARG;
  if ((uintptr_t)y & 7) return SRK_ERR_ALIGNMENT;           // float2 stores of the sub-pixel pairs
  return launch_gemm<false>(x, w, bias, y, N, H, W, Cin, Cout, slope, (hipStream_t)stream);
}

extern "C" int srk_tconv2x2_dgrad(const float* dy, const float* w, float* dx, int N, int H, int W, int Cin, int Cout, void* stream) {
  if (!dy || !w || !dx || !dims_ok(N, H, W, Cin, Cout)) return SRK_ERR_BAD_ARG;
  return launch_gemm<true>(dy, w, nullptr, dx, N, H, W, Cin, Cout, 1.f, (hipStream_t)stream);
}

extern "C" int srk_tconv2x2_wgrad(const float* x, const float* dy, float* dw, float* db, int N, int H, int W, int Cin, int Cout,
                                  float scale, int accumulate, void* workspace, size_t ws_bytes, void* stream) {
  if (!x || !dy || !dw || !workspace || !dims_ok(N, H, W, Cin, Cout)) return SRK_ERR_BAD_ARG;
  const WgradPlan pl = wgrad_plan(N, H, W, Cin, Cout);
  if (ws_bytes < srk_tconv2x2_wgrad_ws_bytes(N, H, W, Cin, Cout)) return SRK_ERR_WORKSPACE;
  if (pl.ci_tiles > 65535 || pl.k_tiles > 65535) return SRK_ERR_UNSUPPORTED;
  hipStream_t st = (hipStream_t)stream;
  float* pw = (float*)workspace;
  float* pb = pw + (size_t)pl.splits * Cin * 4 * Cout;
  hipLaunchKernelGGL(tconv2x2_wgrad_kernel, dim3(pl.splits, pl.ci_tiles, pl.k_tiles), dim3(WG_THREADS), 0, st, x, dy, N, H, W, Cin,
                     Cout, pl.cps, pw, pb);
  SRK_CHECK_LAUNCH();
  const int64_t ntot = (int64_t)Cin * 4 * Cout + (db ? Cout : 0);
  const int64_t blocks = (ntot + 31) / 32;
  if (blocks > 0x7fffffff) return SRK_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(tconv2x2_wgrad_reduce_kernel, dim3((unsigned)blocks), dim3(256), 0, st, pw, pb, pl.splits, Cin, Cout, dw, db,
                     scale, accumulate);
  SRK_CHECK_LAUNCH();
  return SRK_OK;
}
