// ResNet (reference utils/models.py:261-332, ResNet(ResidualBlock, [2, 2, 2], classes, linear_features)) on gfx950:
// stem conv3x3(1->16) BN relu; layer1 two blocks 16->16; layer2 a stride-2 block 16->32 with a conv3x3 + BN
// downsample, then 32->32; layer3 the same 32->64, 64->64; conv2d 1x1 64->64 stride (2, 1) with bias;
// AvgPool2d(4); fc on the (C, PH, PW) flatten; raw logits.  A block is relu(bn2(conv2(relu(bn1(conv1(x))))) + r),
// r = x or downsample(x).  Every 3x3 conv has padding 1 and no bias.  fp32 only.
//
// Activations are channels-last (B, H, W, C) in the workspace.  The fifteen conv + BatchNorm units are numbered in
// named_parameters() order (kUnit); unit u keeps z<u>, the conv output, and a<u>, what its BatchNorm pass wrote
// (after the residual add and the relu where the unit has them).  The fourteen convs behind the stem are implicit
// GEMMs on v_mfma_f32_16x16x4_f32 (conv_kernel), a 64-row block tile with the whole N (16, 32 or 64 channels) in
// 1, 2 or 4 accumulators per wave and a K-step of 16, so a step never straddles two taps even at Cin = 16:
//   forward        M = output pixels, N = Cout, K = 9 Cin; A = the nine gathered pixel rows, zero outside the image
//   data gradient  M = input pixels,  N = Cin,  K = 9 Cout; the transposed gather (stride 2: matching parity only)
//   weight grad    M = 9 Cin (tap, channel), N = Cout, K = output pixels: the forward's gathered A, transposed
// The weight gradients' pixel reduction is cut into slices (plan_slices) summed in slice order; BatchNorm sums are
// per-block double partials summed in block order: no float atomics anywhere, two runs are bit-equal.
// The stem (Cin = 1) is a direct kernel; its weight gradient is per-block partials summed in block order.
#include <algorithm>
#include <cmath>

#include "abd_common.h"

struct abd_resnet {
  int H, W, K;
  int T;             // H * W: the rows per batch element the shared make_ctx checks against 32 bits
  int Hs[4], Ws[4];  // sides of stage 1..3 ([0] unused)
  int H4, PH, PW;
  int64_t lf;        // fc's inputs: 64 * PH * PW
  int64_t off[50];
  int64_t roff[16];
};

namespace {

constexpr int kT = 256;
constexpr int kBM = 64;            // rows of a block tile
constexpr int kBK = 16;            // K-step: one tap's channels, or sixteen pixels of a weight gradient
constexpr int kLd = kBK + 1;       // LDS row pitch of the A tile
constexpr int kSliceRows = 512;    // least pixels of one weight-gradient slice
constexpr int kMaxSlices = 128;
constexpr int kStatRows = 1024;    // least pixels of one BatchNorm partial block
constexpr int kStatBlocks = 256;   // most partial blocks of one BatchNorm reduction
constexpr int kColsumRows = 512;   // above this many rows the column sums run in two stages
constexpr int kW0Blocks = 512;     // most partial blocks of the stem's weight gradient
constexpr int kC0 = 16;            // the stem's channels
constexpr int kCT = 64;            // channels of layer3, conv2d and the pooled map
constexpr int kMaxDim = 4096;
constexpr int kUnits = 15;
constexpr float kBnEps = 1e-5f, kBnMomentum = 0.1f;

// conv + BatchNorm unit: channels, stride, the stage (1..3) of its input and output maps
struct Unit {
  int Cin, Cout, stride, sin, sout;
};
constexpr Unit kUnit[kUnits] = {
    {1, 16, 1, 1, 1},                                                                   // conv, bn
    {16, 16, 1, 1, 1},  {16, 16, 1, 1, 1},  {16, 16, 1, 1, 1},  {16, 16, 1, 1, 1},      // layer1.0, layer1.1
    {16, 32, 2, 1, 2},  {32, 32, 1, 2, 2},  {16, 32, 2, 1, 2},                          // layer2.0 + downsample
    {32, 32, 1, 2, 2},  {32, 32, 1, 2, 2},                                              // layer2.1
    {32, 64, 2, 2, 3},  {64, 64, 1, 3, 3},  {32, 64, 2, 2, 3},                          // layer3.0 + downsample
    {64, 64, 1, 3, 3},  {64, 64, 1, 3, 3}};                                             // layer3.1
// residual block: the unit whose a-map it reads, conv1 / conv2 units, the downsample unit or -1
struct Block {
  int in, u1, u2, ud;
};
constexpr Block kBlock[6] = {{0, 1, 2, -1}, {2, 3, 4, -1}, {4, 5, 6, 7}, {6, 8, 9, -1}, {9, 10, 11, 12}, {11, 13, 14, -1}};
// parameters: unit u has 3u (conv weight), 3u + 1 (BN weight), 3u + 2 (BN bias)
enum { P_C2DW = 3 * kUnits, P_C2DB, P_FCW, P_FCB, P_COUNT };

// GemmArgs and its three forms, the host helpers; colsum_kernel, ce_kernel, metrics_kernel
#include "net_common.inc"
// f4v, tile_mfma, wgrad_reduce_kernel, blocks, stat_plan, the ABI entries of a net with running statistics
#include "conv16_common.inc"

// ------------------------------------------------------------------ 3x3 conv as an implicit GEMM
// The gather: pixel (b, h, w) of the Hr x Wr index map and a tap read source pixel
// ((mul h + sign (tap / 3 - 1)) / div, (mul w + sign (tap % 3 - 1)) / div) of the Hs x Ws map, nothing when a
// quotient is fractional or outside.  Forward and weight gradient of stride s: mul = s, sign = 1, div = 1 over the
// output pixels; data gradient: mul = 1, sign = -1, div = s over the input pixels.
// MODE 1: out (pixels, N) = A mat [+ add], A(m, tap C + c) = channel c of the gathered pixel, mat (9 C, N).
// MODE 2: out + z (9 C) N, (9 C, N) = A^T mat over the pixels [z kchunk, (z + 1) kchunk), mat (pixels, N).
struct ConvArgs {
  const float* src;
  const float* mat;
  const float* add;
  float* out;
  int Hr, Wr, Hs, Ws, C, mul, sign, div;
  int pixels, kchunk;
};

__device__ __forceinline__ int64_t src_pixel(const ConvArgs& a, int b, int h, int w, int tap) {
  int nh = a.mul * h + a.sign * (tap / 3 - 1), nw = a.mul * w + a.sign * (tap % 3 - 1);
  if (a.div == 2) {
    if ((nh | nw) & 1) return -1;
    nh >>= 1, nw >>= 1;
  }
  if ((unsigned)nh >= (unsigned)a.Hs || (unsigned)nw >= (unsigned)a.Ws) return -1;
  return ((int64_t)b * a.Hs + nh) * a.Ws + nw;
}

template <int TN, int MODE>
__global__ void __launch_bounds__(kT) conv_kernel(ConvArgs a) {
  constexpr int BN = 16 * TN, LDB = BN + 8;
  __shared__ float As[kBM * kLd];
  __shared__ float Bs[kBK * LDB];
  const int tid = threadIdx.x, lane = tid & 63, wm = (tid >> 6) * 16;
  const int lo = tid & 15, hi = tid >> 4;
  const int m0 = blockIdx.x * kBM;
  const int HW = a.Hr * a.Wr, C = a.C;
  const int M = MODE == 1 ? a.pixels : 9 * C;
  const int k0 = MODE == 1 ? 0 : blockIdx.z * a.kchunk;
  const int k1 = MODE == 1 ? 9 * C : min(a.pixels, k0 + a.kchunk);
  // MODE 1: this thread's four pixel rows (hi + 16 i), channel lo of the step.
  // MODE 2: its pixel k0 + hi of the step and its four (tap, channel) columns (lo + 16 i).
  int pb[4], phw[4];
  int qb = 0, qh = 0, qw = 0;
  if (MODE == 1) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int gm = m0 + hi + 16 * i;
      pb[i] = -1, phw[i] = 0;
      if (gm < M) {
        const int b = gm / HW, r = gm - b * HW, h = r / a.Wr;
        pb[i] = b, phw[i] = h << 16 | (r - h * a.Wr);
      }
    }
  } else {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int gm = m0 + lo + 16 * i;
      pb[i] = gm < M ? gm / C : -1;        // tap
      phw[i] = gm - (gm / C) * C;          // channel
    }
    const int p = k0 + hi;
    qb = p / HW;
    const int r = p - qb * HW;
    qh = r / a.Wr, qw = r - qh * a.Wr;
  }
  f4v acc[TN];
#pragma unroll
  for (int j = 0; j < TN; ++j)
#pragma unroll
    for (int r = 0; r < 4; ++r) acc[j][r] = 0.0f;
  for (int kb = k0; kb < k1; kb += kBK) {
    float ar[4], br[TN];
    if (MODE == 1) {
      const int tap = kb / C, c0 = kb - tap * C;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int64_t sp = pb[i] >= 0 ? src_pixel(a, pb[i], phw[i] >> 16, phw[i] & 0xffff, tap) : -1;
        ar[i] = sp >= 0 ? a.src[sp * C + c0 + lo] : 0.0f;
      }
#pragma unroll
      for (int j = 0; j < TN; ++j) {
        const int e = tid + j * kT;
        br[j] = a.mat[(int64_t)(kb + e / BN) * BN + e % BN];
      }
    } else {
      const bool ok = kb + hi < k1;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int64_t sp = (ok && pb[i] >= 0) ? src_pixel(a, qb, qh, qw, pb[i]) : -1;
        ar[i] = sp >= 0 ? a.src[sp * C + phw[i]] : 0.0f;
      }
#pragma unroll
      for (int j = 0; j < TN; ++j) {
        const int e = tid + j * kT;
        const int p = kb + e / BN;
        br[j] = p < k1 ? a.mat[(int64_t)p * BN + e % BN] : 0.0f;
      }
      qw += kBK;   // the same lane of the next step is sixteen pixels on
      while (qw >= a.Wr) {
        qw -= a.Wr;
        if (++qh == a.Hr) qh = 0, ++qb;
      }
    }
    __syncthreads();   // the previous tile's operand reads are done
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      if (MODE == 1) As[(hi + 16 * i) * kLd + lo] = ar[i];
      else As[(lo + 16 * i) * kLd + hi] = ar[i];
    }
#pragma unroll
    for (int j = 0; j < TN; ++j) {
      const int e = tid + j * kT;
      Bs[(e / BN) * LDB + e % BN] = br[j];
    }
    __syncthreads();
    tile_mfma<TN, kBK>(As, Bs, LDB, wm, lane, acc);
  }
  float* out = MODE == 1 ? a.out : a.out + (int64_t)blockIdx.z * M * BN;
#pragma unroll
  for (int j = 0; j < TN; ++j)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int m = m0 + wm + (lane >> 4) * 4 + r;
      if (m < M) {
        const int64_t o = (int64_t)m * BN + j * 16 + (lane & 15);
        float v = acc[j][r];
        if (MODE == 1 && a.add) v += a.add[o];
        out[o] = v;
      }
    }
}

// ------------------------------------------------------------------ the plain GEMM of GemmArgs (conv2d, fc)
// 64 x 64 block tile on the same product; bias1 and the z-sliced reduction are honoured, nothing else is used here
__global__ void __launch_bounds__(kT) gemm_kernel(GemmArgs a) {
  constexpr int BN = 64, LDB = BN + 8;
  __shared__ float As[kBM * kLd];
  __shared__ float Bs[kBK * LDB];
  const int tid = threadIdx.x, lane = tid & 63, wm = (tid >> 6) * 16;
  const int m0 = blockIdx.x * kBM, n0 = blockIdx.y * BN;
  const int k0 = blockIdx.z * a.kchunk, k1 = min(a.K, k0 + a.kchunk);
  const bool a_kc = a.sak == 1, b_kc = a.sbk == 1;
  f4v acc[4];
#pragma unroll
  for (int j = 0; j < 4; ++j)
#pragma unroll
    for (int r = 0; r < 4; ++r) acc[j][r] = 0.0f;
  for (int kb = k0; kb < k1; kb += kBK) {
    float ar[4], br[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int e = tid + i * kT;
      const int m = a_kc ? e >> 4 : e & 63, k = a_kc ? e & 15 : e >> 6;
      const int gm = m0 + m, gk = kb + k;
      ar[i] = (gm < a.M && gk < k1) ? a.A[(int64_t)gm * a.sam + (int64_t)gk * a.sak] : 0.0f;
      const int n = b_kc ? e >> 4 : e & 63, kk = b_kc ? e & 15 : e >> 6;
      const int gn = n0 + n, gk2 = kb + kk;
      br[i] = (gn < a.N && gk2 < k1) ? a.B[(int64_t)gk2 * a.sbk + (int64_t)gn * a.sbn] : 0.0f;
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int e = tid + i * kT;
      As[(a_kc ? e >> 4 : e & 63) * kLd + (a_kc ? e & 15 : e >> 6)] = ar[i];
      Bs[(b_kc ? e & 15 : e >> 6) * LDB + (b_kc ? e >> 4 : e & 63)] = br[i];
    }
    __syncthreads();
    tile_mfma<4, kBK>(As, Bs, LDB, wm, lane, acc);
  }
  float* Cz = a.C + (int64_t)blockIdx.z * a.cz;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int n = n0 + j * 16 + (lane & 15);
    if (n >= a.N) continue;
    const float bias = a.bias1 ? a.bias1[n] : 0.0f;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int m = m0 + wm + (lane >> 4) * 4 + r;
      if (m < a.M) Cz[(int64_t)m * a.ldc + n] = acc[j][r] + bias;
    }
  }
}

// ------------------------------------------------------------------ small kernels
// one launch for the fourteen GEMM convs: (Cout, Cin, 3, 3) -> wf (tap, Cin, Cout) and wd (tap, Cout, Cin)
struct RepackArgs {
  const float* params;
  float* ws;
  int64_t w[kUnits], wf[kUnits], wd[kUnits];   // element offsets into params / the float workspace
  int cin[kUnits], cout[kUnits];
  int need_wd;
};

__global__ void __launch_bounds__(kT) repack_kernel(RepackArgs a) {
  const int u = blockIdx.y + 1;
  const int Cin = a.cin[u], Cout = a.cout[u];
  const int e = blockIdx.x * kT + threadIdx.x;
  if (e >= Cout * Cin * 9) return;
  const int tap = e % 9, ci = (e / 9) % Cin, co = e / (9 * Cin);
  const float v = a.params[a.w[u] + e];
  a.ws[a.wf[u] + ((int64_t)tap * Cin + ci) * Cout + co] = v;
  if (a.need_wd) a.ws[a.wd[u] + ((int64_t)tap * Cout + co) * Cin + ci] = v;
}

// out[n] = the sum over slices, in slice order, of slab (slice, n)
__global__ void __launch_bounds__(kT) slab_sum_kernel(const float* slab, int slices, int n, float* out) {
  const int e = blockIdx.x * kT + threadIdx.x;
  if (e >= n) return;
  double s = 0.0;
  for (int z = 0; z < slices; ++z) s += (double)slab[(int64_t)z * n + e];
  out[e] = (float)s;
}

// the stem: z (B, H, W, 16) = the nine taps of x (B, H, W); one thread per output value
__global__ void __launch_bounds__(kT) stem_fwd_kernel(const float* x, const float* w, float* z, int64_t n, int H, int W) {
  const int64_t e = (int64_t)blockIdx.x * kT + threadIdx.x;
  if (e >= n) return;
  const int c = (int)(e % kC0);
  const int64_t p = e / kC0;
  const int r = (int)(p % ((int64_t)H * W));
  const int h = r / W, xw = r - h * W;
  float s = 0.0f;
#pragma unroll
  for (int tap = 0; tap < 9; ++tap) {
    const int hh = h + tap / 3 - 1, ww = xw + tap % 3 - 1;
    const float v = ((unsigned)hh < (unsigned)H && (unsigned)ww < (unsigned)W) ? x[p + (tap / 3 - 1) * W + tap % 3 - 1] : 0.0f;
    s = fmaf(v, w[c * 9 + tap], s);
  }
  z[e] = s;
}

// the stem's weight gradient: block i takes pixels [i chunk, (i + 1) chunk); thread (lane, channel) walks its
// lane's pixels; part (blocks, 16, 9) holds the sixteen lanes summed in lane order
__global__ void __launch_bounds__(kT) stem_wgrad_kernel(const float* x, const float* dz, float* part, int64_t pixels,
                                                        int64_t chunk, int H, int W) {
  constexpr int kLanes = kT / kC0;
  __shared__ float red[kLanes][kC0][9];
  const int c = threadIdx.x % kC0, l = threadIdx.x / kC0;
  const int64_t q0 = (int64_t)blockIdx.x * chunk, q1 = min(pixels, q0 + chunk);
  float acc[9];
#pragma unroll
  for (int t = 0; t < 9; ++t) acc[t] = 0.0f;
  for (int64_t q = q0 + l; q < q1; q += kLanes) {
    const float g = dz[q * kC0 + c];
    const int r = (int)(q % ((int64_t)H * W));
    const int h = r / W, xw = r - h * W;
#pragma unroll
    for (int t = 0; t < 9; ++t) {
      const int hh = h + t / 3 - 1, ww = xw + t % 3 - 1;
      const float v = ((unsigned)hh < (unsigned)H && (unsigned)ww < (unsigned)W) ? x[q + (t / 3 - 1) * W + t % 3 - 1] : 0.0f;
      acc[t] = fmaf(g, v, acc[t]);
    }
  }
#pragma unroll
  for (int t = 0; t < 9; ++t) red[l][c][t] = acc[t];
  __syncthreads();
  if (l == 0) {
#pragma unroll
    for (int t = 0; t < 9; ++t) {
      float s = red[0][c][t];
      for (int j = 1; j < kLanes; ++j) s += red[j][c][t];
      part[((int64_t)blockIdx.x * kC0 + c) * 9 + t] = s;
    }
  }
}

// ------------------------------------------------------------------ BatchNorm
// Two sums per channel over a (pixels, C) map, block i over pixels [i chunk, (i + 1) chunk), thread (lane, channel)
// over its lane's pixels in double; part (blocks, 2, C) holds the lanes summed in lane order.
//   g == NULL: sum z and sum z^2 (the batch statistics)
//   else:      sum g' and sum g' xhat, g' = g where mask > 0 (or no mask), xhat = (z - mean) invstd
__global__ void __launch_bounds__(kT) bn_reduce_kernel(const float* z, const float* g, const float* mask,
                                                       const float* stat, double* part, int64_t pixels, int64_t chunk,
                                                       int C) {
  __shared__ double red[2][kT];
  const int c = threadIdx.x % C, l = threadIdx.x / C, lanes = kT / C;
  const int64_t p0 = (int64_t)blockIdx.x * chunk, p1 = min(pixels, p0 + chunk);
  const float mean = g ? stat[c] : 0.0f, invstd = g ? stat[C + c] : 0.0f;
  double s0 = 0.0, s1 = 0.0;
  for (int64_t p = p0 + l; p < p1; p += lanes) {
    const int64_t i = p * C + c;
    const float v = z[i];
    if (g) {
      const float gv = (mask && !(mask[i] > 0.0f)) ? 0.0f : g[i];
      s0 += (double)gv;
      s1 += (double)gv * (double)((v - mean) * invstd);
    } else {
      s0 += (double)v;
      s1 += (double)v * (double)v;
    }
  }
  red[0][threadIdx.x] = s0, red[1][threadIdx.x] = s1;
  __syncthreads();
  if (l == 0) {
    for (int j = 1; j < lanes; ++j) s0 += red[0][j * C + c], s1 += red[1][j * C + c];
    part[((int64_t)blockIdx.x * 2 + 0) * C + c] = s0;
    part[((int64_t)blockIdx.x * 2 + 1) * C + c] = s1;
  }
}

// the batch statistics from the partials, in block order and in double: stat = mean[C], invstd[C]; the running
// statistics (momentum 0.1, unbiased variance) and num_batches_tracked when given
__global__ void __launch_bounds__(kCT) bn_finalize_kernel(const double* part, int nb, int C, int64_t n, float* stat,
                                                          float* rmean, float* rvar, int64_t* nbt) {
  const int c = threadIdx.x;
  if (c >= C) return;
  double s = 0.0, q = 0.0;
  for (int b = 0; b < nb; ++b) s += part[((int64_t)b * 2 + 0) * C + c], q += part[((int64_t)b * 2 + 1) * C + c];
  const double mean = s / (double)n;
  const double var = fmax(q / (double)n - mean * mean, 0.0);
  stat[c] = (float)mean;
  stat[C + c] = (float)(1.0 / sqrt(var + (double)kBnEps));
  if (rmean) {
    const double unbiased = n > 1 ? var * (double)n / (double)(n - 1) : var;
    rmean[c] = (float)((1.0 - (double)kBnMomentum) * (double)rmean[c] + (double)kBnMomentum * mean);
    rvar[c] = (float)((1.0 - (double)kBnMomentum) * (double)rvar[c] + (double)kBnMomentum * unbiased);
  }
  if (nbt && c == 0) *nbt += 1;
}

// eval mode: stat = running mean, 1 / sqrt(running var + eps)
__global__ void __launch_bounds__(kCT) bn_eval_stat_kernel(const float* rmean, const float* rvar, int C, float* stat) {
  const int c = threadIdx.x;
  if (c >= C) return;
  stat[c] = rmean[c];
  stat[C + c] = (float)(1.0 / sqrt((double)rvar[c] + (double)kBnEps));
}

// d(gamma) = sum g' xhat, d(beta) = sum g', from the partials in block order
__global__ void __launch_bounds__(kCT) bn_bwd_finalize_kernel(const double* part, int nb, int C, float* dgamma,
                                                              float* dbeta) {
  const int c = threadIdx.x;
  if (c >= C) return;
  double s = 0.0, q = 0.0;
  for (int b = 0; b < nb; ++b) s += part[((int64_t)b * 2 + 0) * C + c], q += part[((int64_t)b * 2 + 1) * C + c];
  dbeta[c] = (float)s;
  dgamma[c] = (float)q;
}

// a = gamma xhat + beta [+ res] [relu]
__global__ void __launch_bounds__(kT) bn_apply_kernel(const float* z, const float* stat, const float* gamma,
                                                      const float* beta, const float* res, int relu, float* a,
                                                      int64_t n, int C) {
  const int64_t e = (int64_t)blockIdx.x * kT + threadIdx.x;
  if (e >= n) return;
  const int c = (int)(e % C);
  float v = (z[e] - stat[c]) * stat[C + c] * gamma[c] + beta[c];
  if (res) v += res[e];
  if (relu) v = fmaxf(v, 0.0f);
  a[e] = v;
}

// dz = gamma invstd / n (n g' - d(beta) - xhat d(gamma)); gm (optional) = g', the gradient the residual branch takes
__global__ void __launch_bounds__(kT) bn_bwd_apply_kernel(const float* z, const float* g, const float* mask,
                                                          const float* stat, const float* gamma, const float* dgamma,
                                                          const float* dbeta, float count, float* dz, float* gm,
                                                          int64_t n, int C) {
  const int64_t e = (int64_t)blockIdx.x * kT + threadIdx.x;
  if (e >= n) return;
  const int c = (int)(e % C);
  const float gv = (mask && !(mask[e] > 0.0f)) ? 0.0f : g[e];
  const float xh = (z[e] - stat[c]) * stat[C + c];
  dz[e] = gamma[c] * stat[C + c] / count * (count * gv - dbeta[c] - xh * dgamma[c]);
  if (gm) gm[e] = gv;
}

// ------------------------------------------------------------------ the tail
// sub (B, H4, W, 64) = rows 0, 2, 4, .. of a (B, H, W, 64): conv2d's stride (2, 1)
__global__ void __launch_bounds__(kT) subsample_fwd_kernel(const float* a, float* sub, int64_t n, int H, int H4, int W) {
  const int64_t e = (int64_t)blockIdx.x * kT + threadIdx.x;
  if (e >= n) return;
  const int64_t row = (int64_t)W * kCT;
  const int64_t in = e % row, q = e / row;
  const int64_t h4 = q % H4, b = q / H4;
  sub[e] = a[(b * H + 2 * h4) * row + in];
}

// g (B, H, W, 64) = dsub on the even rows, zero on the odd ones
__global__ void __launch_bounds__(kT) subsample_bwd_kernel(const float* dsub, float* g, int64_t n, int H, int H4, int W) {
  const int64_t e = (int64_t)blockIdx.x * kT + threadIdx.x;
  if (e >= n) return;
  const int64_t row = (int64_t)W * kCT;
  const int64_t in = e % row, q = e / row;
  const int64_t h = q % H, b = q / H;
  g[e] = (h & 1) ? 0.0f : dsub[(b * H4 + (h >> 1)) * row + in];
}

// AvgPool2d(4) of c2 (B, H4, W, 64) into pool (B, 64, PH, PW): the reference's flatten order
__global__ void __launch_bounds__(kT) avgpool_fwd_kernel(const float* c2, float* pool, int64_t n, int H4, int W, int PH,
                                                         int PW) {
  const int64_t e = (int64_t)blockIdx.x * kT + threadIdx.x;
  if (e >= n) return;
  const int c = (int)(e % kCT);
  int64_t q = e / kCT;
  const int pw = (int)(q % PW);
  q /= PW;
  const int ph = (int)(q % PH);
  const int64_t b = q / PH;
  const float* s = c2 + ((b * H4 + 4 * ph) * W + 4 * pw) * kCT + c;
  float v = 0.0f;
#pragma unroll
  for (int k = 0; k < 16; ++k) v += s[((int64_t)(k / 4) * W + k % 4) * kCT];
  pool[((b * kCT + c) * PH + ph) * PW + pw] = v * (1.0f / 16.0f);
}

// dc2 (B, H4, W, 64) = dpool / 16 under each window, zero on the dropped rows and columns
__global__ void __launch_bounds__(kT) avgpool_bwd_kernel(const float* dpool, float* dc2, int64_t n, int H4, int W, int PH,
                                                         int PW) {
  const int64_t e = (int64_t)blockIdx.x * kT + threadIdx.x;
  if (e >= n) return;
  const int c = (int)(e % kCT);
  int64_t q = e / kCT;
  const int xw = (int)(q % W);
  q /= W;
  const int h = (int)(q % H4);
  const int64_t b = q / H4;
  const int ph = h >> 2, pw = xw >> 2;
  dc2[e] = (ph < PH && pw < PW) ? dpool[((b * kCT + c) * PH + ph) * PW + pw] * (1.0f / 16.0f) : 0.0f;
}

// ------------------------------------------------------------------ host side
// workspace map (byte offsets); every buffer 256-byte aligned
struct Layout {
  size_t z[kUnits], a[kUnits], stat[kUnits], wf[kUnits], wd[kUnits];
  size_t sub, c2, pool, logits, dlogits, rowinfo;
  size_t part, g[4], dpool, dc2, dsub, slab, w0part, colp, total;
};

inline int64_t px(const abd_resnet* n, int64_t B, int stage) { return B * n->Hs[stage] * n->Ws[stage]; }

Layout make_layout(const abd_resnet* n, int64_t B) {
  Layout L{};
  Take take;
  for (int u = 0; u < kUnits; ++u) {
    const size_t e = (size_t)px(n, B, kUnit[u].sout) * kUnit[u].Cout;
    L.z[u] = take(4 * e);
    L.a[u] = take(4 * e);
    L.stat[u] = take(4 * 2 * kUnit[u].Cout);
  }
  const size_t tail = (size_t)B * n->H4 * n->Ws[3] * kCT;
  L.sub = take(4 * tail);
  L.c2 = take(4 * tail);
  L.pool = take(4 * (size_t)B * n->lf);
  L.logits = take(4 * (size_t)B * n->K);
  L.dlogits = take(4 * (size_t)B * n->K);
  L.rowinfo = take(4 * (size_t)B * 4);
  size_t slab = (size_t)kCT * kCT * plan_slices((int64_t)B * n->H4 * n->Ws[3], kMaxSlices, kSliceRows, kBK).ksplit;
  for (int u = 1; u < kUnits; ++u) {
    const size_t w = (size_t)9 * kUnit[u].Cin * kUnit[u].Cout;
    L.wf[u] = take(4 * w);
    L.wd[u] = take(4 * w);
    slab = std::max(slab, w * plan_slices(px(n, B, kUnit[u].sout), kMaxSlices, kSliceRows, kBK).ksplit);
  }
  L.part = take(8 * (size_t)kStatBlocks * 2 * kCT);
  for (int i = 0; i < 4; ++i) L.g[i] = take(4 * (size_t)px(n, B, 1) * kC0);   // stage 1 holds the most values
  L.dpool = take(4 * (size_t)B * n->lf);
  L.dc2 = take(4 * tail);
  L.dsub = take(4 * tail);
  L.slab = take(4 * slab);
  L.w0part = take(4 * (size_t)kW0Blocks * kC0 * 9);
  L.colp = take(4 * (size_t)64 * kCT);
  L.total = take.o;
  return L;
}

struct Ctx : CtxBase {
  const abd_resnet* n;
  Layout L;
  float* running;     // NULL: leave the running statistics alone
  int64_t* nbt;
  const float* p(int i) const { return params + n->off[i]; }
  float* g(int i) const { return grads + n->off[i]; }
  float* z(int u) const { return at<float>(L.z[u]); }
  float* a(int u) const { return at<float>(L.a[u]); }
  float* stat(int u) const { return at<float>(L.stat[u]); }
  float* gb(int i) const { return at<float>(L.g[i]); }
};

int launch_gemm(const Ctx& c, GemmArgs g, int nz = 1) {
  if (g.M <= 0 || g.N <= 0) return ABD_OK;
  if (nz == 1) g.kchunk = std::max(g.K, 1);
  dim3 grid((g.M + kBM - 1) / kBM, (g.N + 63) / 64, nz);
  gemm_kernel<<<grid, kT, 0, c.s>>>(g);
  ABD_LAUNCH_CHECK();
  return ABD_OK;
}

template <int MODE>
int launch_conv(const Ctx& c, const ConvArgs& a, int N, int M, int nz) {
  dim3 grid((M + kBM - 1) / kBM, 1, nz);
  switch (N) {
    case 16: conv_kernel<1, MODE><<<grid, kT, 0, c.s>>>(a); break;
    case 32: conv_kernel<2, MODE><<<grid, kT, 0, c.s>>>(a); break;
    default: conv_kernel<4, MODE><<<grid, kT, 0, c.s>>>(a); break;
  }
  ABD_LAUNCH_CHECK();
  return ABD_OK;
}

// y (output pixels, Cout) = conv(x (input pixels, Cin))
int conv_fwd(const Ctx& c, int u, const float* x, float* y) {
  const Unit& cv = kUnit[u];
  ConvArgs a{};
  a.src = x, a.mat = c.at<float>(c.L.wf[u]), a.out = y;
  a.Hr = c.n->Hs[cv.sout], a.Wr = c.n->Ws[cv.sout], a.Hs = c.n->Hs[cv.sin], a.Ws = c.n->Ws[cv.sin];
  a.C = cv.Cin, a.mul = cv.stride, a.sign = 1, a.div = 1;
  a.pixels = (int)px(c.n, c.B, cv.sout);
  return launch_conv<1>(c, a, cv.Cout, a.pixels, 1);
}

// dx (input pixels, Cin) = the transposed conv of dy [+ add]
int conv_dgrad(const Ctx& c, int u, const float* dy, float* dx, const float* add) {
  const Unit& cv = kUnit[u];
  ConvArgs a{};
  a.src = dy, a.mat = c.at<float>(c.L.wd[u]), a.add = add, a.out = dx;
  a.Hr = c.n->Hs[cv.sin], a.Wr = c.n->Ws[cv.sin], a.Hs = c.n->Hs[cv.sout], a.Ws = c.n->Ws[cv.sout];
  a.C = cv.Cout, a.mul = 1, a.sign = -1, a.div = cv.stride;
  a.pixels = (int)px(c.n, c.B, cv.sin);
  return launch_conv<1>(c, a, cv.Cin, a.pixels, 1);
}

// dW[co][ci][tap] = sum over output pixels of dy[p][co] x[the tap's pixel][ci], sliced
int conv_wgrad(const Ctx& c, int u, const float* dy, const float* x) {
  const Unit& cv = kUnit[u];
  const int64_t pixels = px(c.n, c.B, cv.sout);
  const Slices sl = plan_slices(pixels, kMaxSlices, kSliceRows, kBK);
  ConvArgs a{};
  a.src = x, a.mat = dy, a.out = c.at<float>(c.L.slab);
  a.Hr = c.n->Hs[cv.sout], a.Wr = c.n->Ws[cv.sout], a.Hs = c.n->Hs[cv.sin], a.Ws = c.n->Ws[cv.sin];
  a.C = cv.Cin, a.mul = cv.stride, a.sign = 1, a.div = 1;
  a.pixels = (int)pixels, a.kchunk = (int)sl.kchunk;
  if (int rc = launch_conv<2>(c, a, cv.Cout, 9 * cv.Cin, sl.ksplit)) return rc;
  wgrad_reduce_kernel<9><<<blocks(9 * cv.Cin * cv.Cout), kT, 0, c.s>>>(a.out, sl.ksplit, cv.Cout, cv.Cin, c.g(3 * u));
  ABD_LAUNCH_CHECK();
  return ABD_OK;
}

// a<u> = BatchNorm(z<u>) [+ res] [relu]; train: batch statistics, running statistics updated when c.running
int bn_fwd(const Ctx& c, int u, int train, const float* res, int relu) {
  const int C = kUnit[u].Cout;
  const int64_t pixels = px(c.n, c.B, kUnit[u].sout);
  float* rm = c.running ? c.running + c.n->roff[u] : nullptr;
  if (train) {
    const StatPlan sp = stat_plan(pixels);
    double* part = c.at<double>(c.L.part);
    bn_reduce_kernel<<<sp.nb, kT, 0, c.s>>>(c.z(u), nullptr, nullptr, nullptr, part, pixels, sp.chunk, C);
    ABD_LAUNCH_CHECK();
    bn_finalize_kernel<<<1, kCT, 0, c.s>>>(part, sp.nb, C, pixels, c.stat(u), rm, rm ? rm + C : nullptr,
                                           c.nbt ? c.nbt + u : nullptr);
    ABD_LAUNCH_CHECK();
  } else {
    bn_eval_stat_kernel<<<1, kCT, 0, c.s>>>(rm, rm + C, C, c.stat(u));
    ABD_LAUNCH_CHECK();
  }
  bn_apply_kernel<<<blocks(pixels * C), kT, 0, c.s>>>(c.z(u), c.stat(u), c.p(3 * u + 1), c.p(3 * u + 2), res, relu,
                                                      c.a(u), pixels * C, C);
  ABD_LAUNCH_CHECK();
  return ABD_OK;
}

// dz = the gradient at z<u> from g at a<u>; masked: g passes where a<u> > 0; gm (optional) takes the masked g
int bn_bwd(const Ctx& c, int u, const float* g, bool masked, float* dz, float* gm) {
  const int C = kUnit[u].Cout;
  const int64_t pixels = px(c.n, c.B, kUnit[u].sout);
  const StatPlan sp = stat_plan(pixels);
  double* part = c.at<double>(c.L.part);
  const float* mask = masked ? c.a(u) : nullptr;
  bn_reduce_kernel<<<sp.nb, kT, 0, c.s>>>(c.z(u), g, mask, c.stat(u), part, pixels, sp.chunk, C);
  ABD_LAUNCH_CHECK();
  bn_bwd_finalize_kernel<<<1, kCT, 0, c.s>>>(part, sp.nb, C, c.g(3 * u + 1), c.g(3 * u + 2));
  ABD_LAUNCH_CHECK();
  bn_bwd_apply_kernel<<<blocks(pixels * C), kT, 0, c.s>>>(c.z(u), g, mask, c.stat(u), c.p(3 * u + 1), c.g(3 * u + 1),
                                                          c.g(3 * u + 2), (float)pixels, dz, gm, pixels * C, C);
  ABD_LAUNCH_CHECK();
  return ABD_OK;
}

// the shared ABI entries pass the call's args struct or NULL: this forward reads nothing of it
int run_forward(const Ctx& c, const float* x, int train, const abd_resnet_args*) {
  const abd_resnet* n = c.n;
  const int64_t B = c.B;
  RepackArgs ra{};
  ra.params = c.params, ra.ws = c.at<float>(0), ra.need_wd = train;
  for (int u = 1; u < kUnits; ++u) {
    ra.w[u] = n->off[3 * u], ra.wf[u] = c.L.wf[u] / 4, ra.wd[u] = c.L.wd[u] / 4;
    ra.cin[u] = kUnit[u].Cin, ra.cout[u] = kUnit[u].Cout;
  }
  repack_kernel<<<dim3(blocks(9 * kCT * kCT), kUnits - 1), kT, 0, c.s>>>(ra);
  ABD_LAUNCH_CHECK();
  int64_t e = px(n, B, 1) * kC0;
  stem_fwd_kernel<<<blocks(e), kT, 0, c.s>>>(x, c.p(0), c.z(0), e, n->H, n->W);
  ABD_LAUNCH_CHECK();
  if (int rc = bn_fwd(c, 0, train, nullptr, 1)) return rc;
  for (const Block& b : kBlock) {
    if (int rc = conv_fwd(c, b.u1, c.a(b.in), c.z(b.u1))) return rc;
    if (int rc = bn_fwd(c, b.u1, train, nullptr, 1)) return rc;
    if (int rc = conv_fwd(c, b.u2, c.a(b.u1), c.z(b.u2))) return rc;
    const float* res = c.a(b.in);
    if (b.ud >= 0) {
      if (int rc = conv_fwd(c, b.ud, c.a(b.in), c.z(b.ud))) return rc;
      if (int rc = bn_fwd(c, b.ud, train, nullptr, 0)) return rc;
      res = c.a(b.ud);
    }
    if (int rc = bn_fwd(c, b.u2, train, res, 1)) return rc;
  }
  // tail
  const int H3 = n->Hs[3], W3 = n->Ws[3];
  const int64_t rows = B * n->H4 * W3;
  float *sub = c.at<float>(c.L.sub), *c2 = c.at<float>(c.L.c2), *pool = c.at<float>(c.L.pool);
  subsample_fwd_kernel<<<blocks(rows * kCT), kT, 0, c.s>>>(c.a(kUnits - 1), sub, rows * kCT, H3, n->H4, W3);
  ABD_LAUNCH_CHECK();
  GemmArgs g = gemm_nt(sub, kCT, c.p(P_C2DW), c2, (int)rows, kCT, kCT);
  g.bias1 = c.p(P_C2DB);
  if (int rc = launch_gemm(c, g)) return rc;
  avgpool_fwd_kernel<<<blocks(B * n->lf), kT, 0, c.s>>>(c2, pool, B * n->lf, n->H4, W3, n->PH, n->PW);
  ABD_LAUNCH_CHECK();
  g = gemm_nt(pool, n->lf, c.p(P_FCW), c.at<float>(c.L.logits), (int)B, n->K, (int)n->lf);
  g.bias1 = c.p(P_FCB);
  return launch_gemm(c, g);
}

int run_backward(const Ctx& c, const float* x, const float* dlogits) {
  const abd_resnet* n = c.n;
  const int64_t B = c.B;
  const int K = n->K, H3 = n->Hs[3], W3 = n->Ws[3];
  const int64_t rows = B * n->H4 * W3;
  const float *sub = c.at<float>(c.L.sub), *pool = c.at<float>(c.L.pool);
  float *dpool = c.at<float>(c.L.dpool), *dc2 = c.at<float>(c.L.dc2), *dsub = c.at<float>(c.L.dsub);
  float* slab = c.at<float>(c.L.slab);
  // fc
  if (int rc = launch_gemm(c, gemm_tn(dlogits, pool, n->lf, c.g(P_FCW), K, (int)n->lf, B))) return rc;
  if (int rc = launch_colsum(c, dlogits, B, K, K, c.g(P_FCB), 0, kCT, kColsumRows)) return rc;
  if (int rc = launch_gemm(c, gemm_nn(dlogits, K, c.p(P_FCW), dpool, (int)B, (int)n->lf, K))) return rc;
  avgpool_bwd_kernel<<<blocks(rows * kCT), kT, 0, c.s>>>(dpool, dc2, rows * kCT, n->H4, W3, n->PH, n->PW);
  ABD_LAUNCH_CHECK();
  // conv2d: the weight gradient's row reduction in slices
  const Slices sl = plan_slices(rows, kMaxSlices, kSliceRows, kBK);
  GemmArgs g = gemm_tn(dc2, sub, kCT, slab, kCT, kCT, rows);
  g.cz = (int64_t)kCT * kCT, g.kchunk = (int)sl.kchunk;
  if (int rc = launch_gemm(c, g, sl.ksplit)) return rc;
  slab_sum_kernel<<<blocks(kCT * kCT), kT, 0, c.s>>>(slab, sl.ksplit, kCT * kCT, c.g(P_C2DW));
  ABD_LAUNCH_CHECK();
  if (int rc = launch_colsum(c, dc2, rows, kCT, kCT, c.g(P_C2DB), 0, kCT, kColsumRows)) return rc;
  if (int rc = launch_gemm(c, gemm_nn(dc2, kCT, c.p(P_C2DW), dsub, (int)rows, kCT, kCT))) return rc;
  // g0 holds the gradient at the current block's output; g1 = dz, g2 = the residual branch's gradient, g3 = scratch
  float *G = c.gb(0), *Q = c.gb(1), *R = c.gb(2), *S = c.gb(3);
  const int64_t e3 = px(n, B, 3) * kCT;
  subsample_bwd_kernel<<<blocks(e3), kT, 0, c.s>>>(dsub, G, e3, H3, n->H4, W3);
  ABD_LAUNCH_CHECK();
  for (int i = 5; i >= 0; --i) {
    const Block& b = kBlock[i];
    if (int rc = bn_bwd(c, b.u2, G, true, Q, R)) return rc;          // Q = dz2, R = the masked gradient
    if (int rc = conv_wgrad(c, b.u2, Q, c.a(b.u1))) return rc;
    if (int rc = conv_dgrad(c, b.u2, Q, S, nullptr)) return rc;      // S = d a<u1>
    if (int rc = bn_bwd(c, b.u1, S, true, Q, nullptr)) return rc;    // Q = dz1
    if (int rc = conv_wgrad(c, b.u1, Q, c.a(b.in))) return rc;
    if (b.ud >= 0) {
      if (int rc = bn_bwd(c, b.ud, R, false, S, nullptr)) return rc;  // S = dz of the downsample
      if (int rc = conv_wgrad(c, b.ud, S, c.a(b.in))) return rc;
      if (int rc = conv_dgrad(c, b.ud, S, R, nullptr)) return rc;     // R = the downsample's input gradient
    }
    // the block input's gradient: conv1's branch first, the residual branch added to it
    if (int rc = conv_dgrad(c, b.u1, Q, G, R)) return rc;
  }
  // stem
  if (int rc = bn_bwd(c, 0, G, true, Q, nullptr)) return rc;
  const int64_t pixels = px(n, B, 1);
  const int nb = (int)std::min<int64_t>(kW0Blocks, (pixels + 63) / 64);
  const int64_t chunk = (pixels + nb - 1) / nb;
  float* part = c.at<float>(c.L.w0part);
  stem_wgrad_kernel<<<nb, kT, 0, c.s>>>(x, Q, part, pixels, chunk, n->H, n->W);
  ABD_LAUNCH_CHECK();
  colsum_kernel<<<dim3(blocks(kC0 * 9), 1), kRedT, 0, c.s>>>(part, nb, kC0 * 9, kC0 * 9, nb, c.g(0), 0, 0);
  ABD_LAUNCH_CHECK();
  return ABD_OK;
}

int make_ctx(const abd_resnet* net, int64_t B, const float* params, float* grads, void* ws, size_t bytes,
             abd_stream_t stream, Ctx* c) {
  return make_ctx(net, B, params, grads, ws, bytes, stream, kC0, make_layout, c);
}

}  // namespace

extern "C" {

int abd_resnet_tile_info(int what) {
  switch (what) {
    case 0: return kBM;
    case 1: return kBK;
    case 2: return kSliceRows;
    case 3: return kMaxSlices;
    case 4: return kStatRows;
    case 5: return kStatBlocks;
    default: return -1;
  }
}

int64_t abd_resnet_linear_features(int H, int W) {
  if (H < 25 || W < 13) return -1;
  const int H3 = ((H - 1) / 2 + 1 - 1) / 2 + 1, W3 = ((W - 1) / 2 + 1 - 1) / 2 + 1;
  const int H4 = (H3 - 1) / 2 + 1;
  return (int64_t)kCT * (H4 / 4) * (W3 / 4);
}

int abd_resnet_create(int H, int W, int num_classes, abd_resnet** net) {
  ABD_CHECK(net != nullptr, ABD_E_INVALID, "NULL out pointer");
  ABD_CHECK(H >= 25 && W >= 13, ABD_E_UNSUPPORTED,
            "ResNet: input %d x %d leaves the average pool no 4 x 4 window (25 x 13 is the smallest)", H, W);
  ABD_CHECK(H <= kMaxDim && W <= kMaxDim, ABD_E_UNSUPPORTED, "ResNet: input %d x %d beyond %d per side", H, W, kMaxDim);
  ABD_CHECK(num_classes >= 1 && num_classes <= 4096, ABD_E_UNSUPPORTED, "num_classes must be in [1, 4096]");
  const int64_t lf = abd_resnet_linear_features(H, W);
  ABD_CHECK((int64_t)H * W * kC0 < (1LL << 31) && lf * num_classes < (1LL << 31), ABD_E_UNSUPPORTED,
            "ResNet: input %d x %d takes the kernels' indices past 32 bits", H, W);
  auto* n = new abd_resnet();
  n->H = H, n->W = W, n->K = num_classes, n->T = H * W;
  n->Hs[0] = n->Ws[0] = 0;
  n->Hs[1] = H, n->Ws[1] = W;
  for (int s = 2; s <= 3; ++s) n->Hs[s] = (n->Hs[s - 1] - 1) / 2 + 1, n->Ws[s] = (n->Ws[s - 1] - 1) / 2 + 1;
  n->H4 = (n->Hs[3] - 1) / 2 + 1;
  n->PH = n->H4 / 4, n->PW = n->Ws[3] / 4;
  n->lf = lf;
  n->off[0] = 0, n->roff[0] = 0;
  for (int u = 0; u < kUnits; ++u) {
    n->off[3 * u + 1] = n->off[3 * u] + (int64_t)kUnit[u].Cout * kUnit[u].Cin * 9;
    n->off[3 * u + 2] = n->off[3 * u + 1] + kUnit[u].Cout;
    n->off[3 * u + 3] = n->off[3 * u + 2] + kUnit[u].Cout;
    n->roff[u + 1] = n->roff[u] + 2 * kUnit[u].Cout;
  }
  n->off[P_C2DB] = n->off[P_C2DW] + kCT * kCT;
  n->off[P_FCW] = n->off[P_C2DB] + kCT;
  n->off[P_FCB] = n->off[P_FCW] + lf * num_classes;
  n->off[P_COUNT] = n->off[P_FCB] + num_classes;
  *net = n;
  return ABD_OK;
}

void abd_resnet_destroy(abd_resnet* net) { delete net; }

int64_t abd_resnet_param_count(const abd_resnet* net) { return net ? net->off[P_COUNT] : 0; }

int abd_resnet_param_offsets(const abd_resnet* net, int64_t* offsets) {
  ABD_CHECK(net && offsets, ABD_E_INVALID, "NULL argument");
  for (int i = 0; i <= P_COUNT; ++i) offsets[i] = net->off[i];
  return ABD_OK;
}

int64_t abd_resnet_running_count(const abd_resnet* net) { return net ? net->roff[kUnits] : 0; }

int abd_resnet_running_offsets(const abd_resnet* net, int64_t* offsets) {
  ABD_CHECK(net && offsets, ABD_E_INVALID, "NULL argument");
  for (int i = 0; i <= kUnits; ++i) offsets[i] = net->roff[i];
  return ABD_OK;
}

size_t abd_resnet_workspace_bytes(const abd_resnet* net, int64_t batch) {
  if (!net || batch < 1) return 0;
  return make_layout(net, batch).total;
}

int64_t abd_resnet_workspace_offset(const abd_resnet* net, int64_t batch, const char* name) {
  if (!net || !name || batch < 1) return -1;
  const Layout L = make_layout(net, batch);
  if ((name[0] == 'z' || name[0] == 'a' || name[0] == 's') && name[1] >= '0' && name[1] <= '9') {
    const int u = name[2] == 0 ? name[1] - '0' : (name[2] >= '0' && name[2] <= '9' && name[3] == 0)
                                                      ? (name[1] - '0') * 10 + name[2] - '0' : -1;
    if (u < 0 || u >= kUnits) return -1;
    return (int64_t)(name[0] == 'z' ? L.z[u] : name[0] == 'a' ? L.a[u] : L.stat[u]);
  }
  const NamedOffset tab[] = {{"sub", L.sub},       {"c2", L.c2},           {"pool", L.pool},
                             {"logits", L.logits}, {"dlogits", L.dlogits}, {"rowinfo", L.rowinfo}};
  return find_offset(tab, name);
}

int abd_resnet_forward(abd_resnet* net, const abd_resnet_args* a, int train_mode, void* workspace,
                       size_t workspace_bytes, abd_stream_t stream) {
  return stat_net_forward<Ctx>(net, a, train_mode, workspace, workspace_bytes, stream);
}

int abd_resnet_backward(abd_resnet* net, const abd_resnet_args* a, const float* dlogits, void* workspace,
                        size_t workspace_bytes, abd_stream_t stream) {
  return stat_net_backward<Ctx>(net, a, dlogits, workspace, workspace_bytes, stream);
}

int abd_resnet_train_step(abd_resnet* net, const abd_resnet_args* a, void* workspace, size_t workspace_bytes,
                          abd_stream_t stream) {
  return stat_net_train_step<Ctx>(net, a, workspace, workspace_bytes, stream);
}

int abd_resnet_eval(abd_resnet* net, const float* x, int64_t batch, const float* params, const float* running,
                    const int64_t* labels, const int64_t* indicators, float* logits, int64_t* metrics, void* workspace,
                    size_t workspace_bytes, abd_stream_t stream) {
  return stat_net_eval<Ctx>(net, x, batch, params, running, labels, indicators, logits, metrics, workspace,
                            workspace_bytes, stream);
}

}  // extern "C"
