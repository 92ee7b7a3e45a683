// largecnn (reference utils/models.py:68-119) on gfx950: conv1(1->96) pool 2x2, conv2(96->256) pool 2x2,
// relu conv3(256->384), relu conv4(384->384), relu conv5(384->256), pool 3x3 stride 2, flatten (C, H, W),
// relu fc1 dropout, relu fc2 dropout, fc3, log_softmax; cross entropy on the log-probabilities (log_softmax
// twice, as the reference trains it).  Every conv is 3x3, stride 1, padding 1.  fp32 only.
//
// Activations are channels-last (B, H, W, C) in the workspace; only the pooled 256-channel map is written in
// the reference's (B, C, H, W) order, which is fc1's input row.  conv2..conv5 are implicit GEMMs on
// v_mfma_f32_32x32x2_f32 (conv_gemm_kernel: the LDS-tiled block of gemm_tiled.inc written out with a pixel gather
// in each loader; handing the gathers to the shared body as a policy compiled to a slower schedule):
//   forward        M = pixels, N = Cout, K = 9 Cin; A = the nine shifted pixel rows, zero outside the image
//   data gradient  M = pixels, N = Cin,  K = 9 Cout; the same gather with the tap offsets negated
//   weight grad    M = Cout,   N = Cin,  K = pixels, one z-slab per (slice, tap); B = the shifted pixel rows
// The weights are repacked once per step to (Cout, tap, Cin) and (tap, Cout, Cin), so both B operands are
// plain matrices.  The weight gradients' pixel reduction is cut into slices (plan_slices) whose slabs
// wgrad_reduce_kernel sums in slice order into the reference's (Cout, Cin, 3, 3): no float atomics anywhere,
// two runs are bit-equal.  The fc head runs the same kernel without a gather.
// conv1 (Cin = 1) is a direct VALU kernel; its weight gradient is per-block partials summed in block order.
// The pools' backward passes recompute the argmax from the saved conv output with torch's rule (the first
// maximum in row-major window order wins); nothing is stored for them.
#include <algorithm>
#include <cmath>

#include "abd_common.h"

struct abd_largecnn {
  int H, W, K;
  int T;             // H * W: the rows per batch element the shared make_ctx checks against 32 bits
  int H2, W2, H4, W4, PH, PW;
  int64_t lf;        // fc1's inputs: 256 * PH * PW
  int64_t off[17];
  int large_min_blocks;   // least count of 128 x 128 blocks for which the large tile is used
};

namespace {

constexpr int kT = 256;
constexpr int kLargeMinBlocks = 96;  // below this many 128 x 128 blocks the 64 x 64 tile fills more CUs
constexpr int kSliceRows = 256;    // least pixels of one weight-gradient slice
constexpr int kMaxSlices = 16;
constexpr int kColsumRows = 512;   // above this many rows the column sums run in two stages
constexpr int kC1 = 96, kC2 = 256, kC3 = 384, kC4 = 384, kC5 = 256, kF1 = 256, kF2 = 128;
constexpr int kMaxC = 384;
constexpr int kW1Blocks = 512;     // most partial blocks of conv1's weight gradient
constexpr int kW1Lanes = 2;        // pixel lanes of one such block (kW1Lanes * 96 threads)
// H, W at most: the weight-gradient loader splits a pixel's row / column with (int)((n + 0.5f) * (1.0f / side)),
// which equals n / side for every side up to this and every n < side + 32 (the quotient's distance from an integer
// is at least 0.5 / 4096 = 1.2e-4 against about 1e-6 of rounding; tests/test_largecnn_cpu.py checks every pair)
constexpr int kMaxDim = 4096;

enum { P_C1W, P_C1B, P_C2W, P_C2B, P_C3W, P_C3B, P_C4W, P_C4B, P_C5W, P_C5B, P_F1W, P_F1B, P_F2W, P_F2B, P_F3W,
       P_F3B, P_COUNT };

// GemmArgs and its three forms, the host helpers; colsum_kernel, ce_kernel, metrics_kernel
#include "net_common.inc"
#include "gemm_tiled.inc"   // kBK, the tile sizes, f16v and launch_tiled
#include "log_softmax.inc"  // lsm_fwd_kernel, lsm_bwd_kernel

// ------------------------------------------------------------------ LDS-tiled fp32 MFMA GEMM with a pixel gather
// mode 0: the plain GEMM of GemmArgs.
// mode 1: row m of A is pixel m of a (.., H, W, C) map and k = tap * C + c: A(m, k) is channel c of the pixel
//         sign * (tap / 3 - 1) rows and sign * (tap % 3 - 1) columns away, zero outside the image.  C is a multiple
//         of kBK, so one K-step stays inside one tap.
// mode 2: k is a pixel; blockIdx.z = slice * 9 + tap; B(k, n) is channel n of the pixel that tap away from k.
struct ConvGemm {
  GemmArgs g;
  int mode, H, W, C, sign, relu;
  const float* mask;   // epilogue: keep v where mask[m][n] > 0 (the ReLU of the layer below), same ldc
  float invH, invW;
};

template <int TM, int TN>
__global__ void __launch_bounds__(kT) conv_gemm_kernel(ConvGemm cg) {
  const GemmArgs& a = cg.g;
  constexpr int BM = 64 * TM, BN = 64 * TN;
  constexpr int NA = BM * kBK / kT, NB = BN * kBK / kT;
  __shared__ float As[kBK * (BM + 32)];
  __shared__ float Bs[kBK * (BN + 32)];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int wm = (w >> 1) * TM * 32, wn = (w & 1) * TN * 32;
  const int m0 = blockIdx.x * BM, n0 = blockIdx.y * BN;
  const int zs = cg.mode == 2 ? blockIdx.z / 9 : blockIdx.z;
  const int ztap = cg.mode == 2 ? blockIdx.z % 9 : 0;
  const int k0 = zs * a.kchunk;
  const int k1 = min(a.K, k0 + a.kchunk);
  const bool a_kc = a.sak == 1, b_kc = a.sbk == 1;
  const int a_sm = a_kc ? kBK + 1 : 1, a_sk = a_kc ? 1 : BM + 32;
  const int b_sn = b_kc ? kBK + 1 : 1, b_sk = b_kc ? 1 : BN + 32;
  const int HW = cg.mode ? cg.H * cg.W : 1;
  // mode 1: (row << 16 | column) of this thread's A rows, -1 past M (a_kc holds: m = e >> 5)
  int hw[NA];
  if (cg.mode == 1) {
#pragma unroll
    for (int i = 0; i < NA; ++i) {
      const int gm = m0 + ((tid + i * kT) >> 5);
      const int r = gm % HW;
      hw[i] = gm < a.M ? ((r / cg.W) << 16 | (r % cg.W)) : -1;
    }
  }
  const int tdy = cg.sign * (ztap / 3 - 1), tdx = cg.sign * (ztap % 3 - 1);   // mode 2
  f16v acc[TM][TN];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.0f;
  for (int kb = k0; kb < k1; kb += kBK) {
    float ar[NA], br[NB];
    if (cg.mode == 1) {
      const int tap = kb / cg.C, c0 = kb - tap * cg.C;
      const int dy = cg.sign * (tap / 3 - 1), dx = cg.sign * (tap % 3 - 1);
#pragma unroll
      for (int i = 0; i < NA; ++i) {
        const int e = tid + i * kT;
        const int gm = m0 + (e >> 5), k = e & 31;
        const int h = (hw[i] >> 16) + dy, x = (hw[i] & 0xffff) + dx;
        const bool ok = hw[i] >= 0 && (unsigned)h < (unsigned)cg.H && (unsigned)x < (unsigned)cg.W;
        ar[i] = ok ? a.A[((int64_t)gm + dy * cg.W + dx) * a.sam + c0 + k] : 0.0f;
      }
    } else {
#pragma unroll
      for (int i = 0; i < NA; ++i) {
        const int e = tid + i * kT;
        const int m = a_kc ? e >> 5 : e % BM, k = a_kc ? e & 31 : e / BM;
        const int gm = m0 + m, gk = kb + k;
        ar[i] = (gm < a.M && gk < k1) ? a.A[(int64_t)gm * a.sam + (int64_t)gk * a.sak] : 0.0f;
      }
    }
    if (cg.mode == 2) {
      // the K-step's first pixel is uniform; each of its 32 pixels is at most 32 columns further
      const int r0 = kb % HW;
      const int h0 = r0 / cg.W, w0 = r0 - h0 * cg.W;
#pragma unroll
      for (int i = 0; i < NB; ++i) {
        const int e = tid + i * kT;
        const int n = e % BN, k = e / BN;
        const int gn = n0 + n, gk = kb + k;
        const int wc = w0 + k;
        const int wq = (int)(((float)wc + 0.5f) * cg.invW);
        const int hc = h0 + wq;
        const int hq = (int)(((float)hc + 0.5f) * cg.invH);
        const int h = hc - hq * cg.H + tdy, x = wc - wq * cg.W + tdx;
        const bool ok = gn < a.N && gk < k1 && (unsigned)h < (unsigned)cg.H && (unsigned)x < (unsigned)cg.W;
        br[i] = ok ? a.B[((int64_t)gk + tdy * cg.W + tdx) * a.sbk + gn] : 0.0f;
      }
    } else {
#pragma unroll
      for (int i = 0; i < NB; ++i) {
        const int e = tid + i * kT;
        const int n = b_kc ? e >> 5 : e % BN, k = b_kc ? e & 31 : e / BN;
        const int gn = n0 + n, gk = kb + k;
        br[i] = (gn < a.N && gk < k1) ? a.B[(int64_t)gk * a.sbk + (int64_t)gn * a.sbn] : 0.0f;
      }
    }
    __syncthreads();   // the previous tile's operand reads are done
#pragma unroll
    for (int i = 0; i < NA; ++i) {
      const int e = tid + i * kT;
      const int m = a_kc ? e >> 5 : e % BM, k = a_kc ? e & 31 : e / BM;
      As[m * a_sm + k * a_sk] = ar[i];
    }
#pragma unroll
    for (int i = 0; i < NB; ++i) {
      const int e = tid + i * kT;
      const int n = b_kc ? e >> 5 : e % BN, k = b_kc ? e & 31 : e / BN;
      Bs[n * b_sn + k * b_sk] = br[i];
    }
    __syncthreads();
#pragma unroll 4
    for (int kk = 0; kk < kBK / 2; ++kk) {
      const int k = 2 * kk + (lane >> 5);
      float av[TM], bv[TN];
#pragma unroll
      for (int i = 0; i < TM; ++i) av[i] = As[(wm + i * 32 + (lane & 31)) * a_sm + k * a_sk];
#pragma unroll
      for (int j = 0; j < TN; ++j) bv[j] = Bs[(wn + j * 32 + (lane & 31)) * b_sn + k * b_sk];
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[i], bv[j], acc[i][j], 0, 0, 0);
    }
  }
  float* C = a.C + (int64_t)blockIdx.z * a.cz;
#pragma unroll
  for (int j = 0; j < TN; ++j) {
    const int n = n0 + wn + j * 32 + (lane & 31);
    if (n >= a.N) continue;
    const float bias = a.bias1 ? a.bias1[n] : 0.0f;
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int m = m0 + wm + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
        if (m < a.M) {
          const int64_t o = (int64_t)m * a.ldc + n;
          float v = acc[i][j][r] + bias;
          if (cg.relu) v = fmaxf(v, 0.0f);
          if (cg.mask) v = cg.mask[o] > 0.0f ? v : 0.0f;
          C[o] = v;
        }
      }
  }
}

// ------------------------------------------------------------------ small kernels
// (Cout, Cin, 3, 3) -> wf (Cout, tap, Cin) and wd (tap, Cout, Cin)
__global__ void __launch_bounds__(kT) repack_kernel(const float* w, float* wf, float* wd, int Cout, int Cin) {
  const int e = blockIdx.x * kT + threadIdx.x;
  if (e >= Cout * 9 * Cin) return;
  const int ci = e % Cin, tap = (e / Cin) % 9, co = e / (9 * Cin);
  const float v = w[((int64_t)co * Cin + ci) * 9 + tap];
  wf[e] = v;
  if (wd) wd[((int64_t)tap * Cout + co) * Cin + ci] = v;
}

// dw (Cout, Cin, 3, 3) = the sum over slices, in slice order, of slab (slice, tap, Cout, Cin)
__global__ void __launch_bounds__(kT) wgrad_reduce_kernel(const float* slab, int slices, int Cout, int Cin, float* dw) {
  const int e = blockIdx.x * kT + threadIdx.x;
  const int per = 9 * Cout * Cin;
  if (e >= per) return;
  double s = 0.0;
  for (int z = 0; z < slices; ++z) s += (double)slab[(int64_t)z * per + e];
  const int ci = e % Cin, co = (e / Cin) % Cout, tap = e / (Cin * Cout);
  dw[((int64_t)co * Cin + ci) * 9 + tap] = (float)s;
}

// conv1: y (B, H, W, 96) = the nine taps of x (B, H, W) + bias; one thread per output value
__global__ void __launch_bounds__(kT) conv1_fwd_kernel(const float* x, const float* w, const float* bias, float* y,
                                                       int64_t n, int H, int W) {
  const int64_t e = (int64_t)blockIdx.x * kT + threadIdx.x;
  if (e >= n) return;
  const int c = (int)(e % kC1);
  const int64_t p = e / kC1;
  const int r = (int)(p % ((int64_t)H * W));
  const int h = r / W, xw = r - h * W;
  float s = bias[c];
#pragma unroll
  for (int tap = 0; tap < 9; ++tap) {
    const int hh = h + tap / 3 - 1, ww = xw + tap % 3 - 1;
    const float v = ((unsigned)hh < (unsigned)H && (unsigned)ww < (unsigned)W) ? x[p + (tap / 3 - 1) * W + tap % 3 - 1] : 0.0f;
    s = fmaf(v, w[c * 9 + tap], s);
  }
  y[e] = s;
}

// non-overlapping 2x2 max pool of a (B, H, W, C) map; the odd trailing row / column is dropped
__global__ void __launch_bounds__(kT) pool2_fwd_kernel(const float* a, float* p, int64_t n, int H, int W, int C) {
  const int64_t e = (int64_t)blockIdx.x * kT + threadIdx.x;
  if (e >= n) return;
  const int PH = H / 2, PW = W / 2;
  const int c = (int)(e % C);
  int64_t q = e / C;
  const int pw = (int)(q % PW);
  q /= PW;
  const int ph = (int)(q % PH);
  const int64_t b = q / PH;
  const float* s = a + (((b * H + 2 * ph) * W) + 2 * pw) * C + c;
  p[e] = fmaxf(fmaxf(s[0], s[C]), fmaxf(s[(int64_t)W * C], s[(int64_t)W * C + C]));
}

// offset (0..3, row-major) of the first maximum of a 2x2 window: torch's tie rule
__device__ __forceinline__ int argmax4(float v0, float v1, float v2, float v3) {
  int k = 0;
  float m = v0;
  if (v1 > m) m = v1, k = 1;
  if (v2 > m) m = v2, k = 2;
  if (v3 > m) k = 3;
  return k;
}

// da (B, H, W, C): dp at the window's first maximum of a, zero elsewhere and on the dropped row / column
__global__ void __launch_bounds__(kT) pool2_bwd_kernel(const float* a, const float* dp, float* da, int64_t n, int H,
                                                       int W, int C) {
  const int64_t e = (int64_t)blockIdx.x * kT + threadIdx.x;
  if (e >= n) return;
  const int PH = H / 2, PW = W / 2;
  const int c = (int)(e % C);
  int64_t q = e / C;
  const int xw = (int)(q % W);
  q /= W;
  const int h = (int)(q % H);
  const int64_t b = q / H;
  const int ph = h >> 1, pw = xw >> 1;
  float g = 0.0f;
  if (ph < PH && pw < PW) {
    const float* s = a + (((b * H + 2 * ph) * W) + 2 * pw) * C + c;
    const int k = argmax4(s[0], s[C], s[(int64_t)W * C], s[(int64_t)W * C + C]);
    if (k == (h & 1) * 2 + (xw & 1)) g = dp[((b * PH + ph) * PW + pw) * C + c];
  }
  da[e] = g;
}

// 3x3 stride-2 max pool of a (B, H, W, 256) into flat (B, 256, PH, PW): the reference's flatten order
__global__ void __launch_bounds__(kT) pool3_fwd_kernel(const float* a, float* flat, int64_t n, int H, int W, int PH,
                                                       int PW) {
  const int64_t e = (int64_t)blockIdx.x * kT + threadIdx.x;
  if (e >= n) return;
  const int c = (int)(e % kC5);
  int64_t q = e / kC5;
  const int pw = (int)(q % PW);
  q /= PW;
  const int ph = (int)(q % PH);
  const int64_t b = q / PH;
  const float* s = a + ((b * H + 2 * ph) * W + 2 * pw) * kC5 + c;
  float m = s[0];
#pragma unroll
  for (int k = 1; k < 9; ++k) m = fmaxf(m, s[((int64_t)(k / 3) * W + k % 3) * kC5]);
  flat[((b * kC5 + c) * PH + ph) * PW + pw] = m;
}

// da5 (B, H, W, 256): each position gathers dflat of the (at most four) windows whose first maximum it is,
// through relu (a > 0)
__global__ void __launch_bounds__(kT) pool3_bwd_kernel(const float* a, const float* dflat, float* da, int64_t n, int H,
                                                       int W, int PH, int PW) {
  const int64_t e = (int64_t)blockIdx.x * kT + threadIdx.x;
  if (e >= n) return;
  const int c = (int)(e % kC5);
  int64_t q = e / kC5;
  const int xw = (int)(q % W);
  q /= W;
  const int h = (int)(q % H);
  const int64_t b = q / H;
  const float self = a[e];
  float g = 0.0f;
  if (self > 0.0f) {
    for (int ph = max(0, (h - 1) >> 1); ph <= min(PH - 1, h >> 1); ++ph)
      for (int pw = max(0, (xw - 1) >> 1); pw <= min(PW - 1, xw >> 1); ++pw) {
        const float* s = a + ((b * H + 2 * ph) * W + 2 * pw) * kC5 + c;
        float m = s[0];
        int arg = 0;
#pragma unroll
        for (int k = 1; k < 9; ++k) {
          const float v = s[((int64_t)(k / 3) * W + k % 3) * kC5];
          if (v > m) m = v, arg = k;
        }
        if (arg == (h - 2 * ph) * 3 + (xw - 2 * pw)) g += dflat[((b * kC5 + c) * PH + ph) * PW + pw];
      }
  }
  da[e] = g;
}

// h = relu(h), then dropout: keep ? 2 h : 0.  keep (B, n) is written; it comes from mask_in or the hash of
// (seed, counter, global row * (256 + 128) + first + unit), first = 0 for fc1's units and 256 for fc2's.
// train == 0: relu only.
__global__ void __launch_bounds__(kT) act_fwd_kernel(float* h, int64_t total, int n, int first, int train,
                                                     const uint8_t* mask_in, uint8_t* keep, uint8_t* mask_out,
                                                     uint64_t seed, uint64_t counter, int64_t row_offset) {
  const int64_t e = (int64_t)blockIdx.x * kT + threadIdx.x;
  if (e >= total) return;
  float v = fmaxf(h[e], 0.0f);
  if (train) {
    const int64_t b = e / n;
    const int u = (int)(e - b * n);
    const uint8_t k = mask_in ? (mask_in[e] != 0)
                              : keep_hash(seed, counter, (uint64_t)(row_offset + b) * (kF1 + kF2) + first + u, 0.5f);
    v = k ? v * 2.0f : 0.0f;
    keep[e] = k;
    if (mask_out) mask_out[e] = k;
  }
  h[e] = v;
}

// through dropout (scale 2 where kept) and relu: the saved h is positive exactly where both let the value pass
__global__ void __launch_bounds__(kT) act_bwd_kernel(float* dh, const float* h, int64_t total) {
  const int64_t e = (int64_t)blockIdx.x * kT + threadIdx.x;
  if (e >= total) return;
  dh[e] = h[e] > 0.0f ? dh[e] * 2.0f : 0.0f;
}

// conv1's weight gradient: block i takes pooled pixels [i * chunk, (i + 1) * chunk); thread (lane, channel) walks
// its lane's pixels, finds pool1's first maximum in a1 and adds dp1 times the nine taps of x around it.
// part (blocks, 96, 9) holds the lanes summed in lane order.
__global__ void __launch_bounds__(kW1Lanes * kC1) conv1_wgrad_kernel(const float* x, const float* a1, const float* dp1,
                                                                   float* part, int64_t pixels, int64_t chunk, int H,
                                                                   int W) {
  __shared__ float red[kW1Lanes][kC1][9];
  const int c = threadIdx.x % kC1, l = threadIdx.x / kC1;
  const int PH = H / 2, PW = W / 2;
  const int64_t q0 = (int64_t)blockIdx.x * chunk, q1 = min(pixels, q0 + chunk);
  float acc[9];
#pragma unroll
  for (int t = 0; t < 9; ++t) acc[t] = 0.0f;
  for (int64_t q = q0 + l; q < q1; q += kW1Lanes) {
    const float g = dp1[q * kC1 + c];
    const int pw = (int)(q % PW);
    const int ph = (int)((q / PW) % PH);
    const int64_t b = q / ((int64_t)PW * PH);
    const float* s = a1 + ((b * H + 2 * ph) * W + 2 * pw) * kC1 + c;
    const int k = argmax4(s[0], s[kC1], s[(int64_t)W * kC1], s[(int64_t)W * kC1 + kC1]);
    const int h = 2 * ph + (k >> 1), xw = 2 * pw + (k & 1);
    const float* xp = x + (b * H + h) * W + xw;
#pragma unroll
    for (int t = 0; t < 9; ++t) {
      const int hh = h + t / 3 - 1, ww = xw + t % 3 - 1;
      const float v = ((unsigned)hh < (unsigned)H && (unsigned)ww < (unsigned)W) ? xp[(t / 3 - 1) * W + t % 3 - 1] : 0.0f;
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
      for (int j = 1; j < kW1Lanes; ++j) s += red[j][c][t];
      part[((int64_t)blockIdx.x * kC1 + c) * 9 + t] = s;
    }
  }
}

// ------------------------------------------------------------------ host side
struct ConvLayer {
  int Cin, Cout, pw, pb;   // channels, parameter indices
};
constexpr ConvLayer kConv[4] = {{kC1, kC2, P_C2W, P_C2B}, {kC2, kC3, P_C3W, P_C3B}, {kC3, kC4, P_C4W, P_C4B},
                                {kC4, kC5, P_C5W, P_C5B}};

// workspace map (byte offsets); every buffer 256-byte aligned
struct Layout {
  size_t a1, p1, a2, p2, a3, a4, a5, p3, h1, h2, z3, logits, dlogits, rowinfo, keep1, keep2;
  size_t wf[4], wd[4];
  size_t dz3, dh2, dh1, dflat, da5, da4, da3, dp2, da2, dp1, slab, w1part, colp, total;
};

int64_t conv_pixels(const abd_largecnn* n, int64_t B, int layer) {   // output pixels of kConv[layer]
  return layer == 0 ? B * n->H2 * n->W2 : B * n->H4 * n->W4;
}

Layout make_layout(const abd_largecnn* n, int64_t B) {
  Layout L{};
  Take take;
  const size_t px1 = (size_t)B * n->H * n->W, px2 = (size_t)B * n->H2 * n->W2, px4 = (size_t)B * n->H4 * n->W4;
  L.a1 = take(4 * px1 * kC1);
  L.p1 = take(4 * px2 * kC1);
  L.a2 = take(4 * px2 * kC2);
  L.p2 = take(4 * px4 * kC2);
  L.a3 = take(4 * px4 * kC3);
  L.a4 = take(4 * px4 * kC4);
  L.a5 = take(4 * px4 * kC5);
  L.p3 = take(4 * (size_t)B * n->lf);
  L.h1 = take(4 * (size_t)B * kF1);
  L.h2 = take(4 * (size_t)B * kF2);
  L.z3 = take(4 * (size_t)B * n->K);
  L.logits = take(4 * (size_t)B * n->K);    // the log-probabilities the model returns
  L.dlogits = take(4 * (size_t)B * n->K);
  L.rowinfo = take(4 * (size_t)B * 4);
  L.keep1 = take((size_t)B * kF1);
  L.keep2 = take((size_t)B * kF2);
  size_t slab = 0;
  for (int l = 0; l < 4; ++l) {
    const size_t w = (size_t)9 * kConv[l].Cin * kConv[l].Cout;
    L.wf[l] = take(4 * w);
    L.wd[l] = take(4 * w);
    slab = std::max(slab, w * plan_slices(conv_pixels(n, B, l), kMaxSlices, kSliceRows, kBK).ksplit);
  }
  L.dz3 = take(4 * (size_t)B * n->K);
  L.dh2 = take(4 * (size_t)B * kF2);
  L.dh1 = take(4 * (size_t)B * kF1);
  L.dflat = take(4 * (size_t)B * n->lf);
  L.da5 = take(4 * px4 * kC5);
  L.da4 = take(4 * px4 * kC4);
  L.da3 = take(4 * px4 * kC3);
  L.dp2 = take(4 * px4 * kC2);
  L.da2 = take(4 * px2 * kC2);
  L.dp1 = take(4 * px2 * kC1);
  L.slab = take(4 * slab);
  L.w1part = take(4 * (size_t)kW1Blocks * kC1 * 9);
  L.colp = take(4 * (size_t)64 * kMaxC);
  L.total = take.o;
  return L;
}

struct Ctx : CtxBase {
  const abd_largecnn* n;
  Layout L;
  const float* p(int i) const { return params + n->off[i]; }
  float* g(int i) const { return grads + n->off[i]; }
};

struct Fwd {
  const float* x;
  int train;
  const uint8_t* mask1_in;
  const uint8_t* mask2_in;
  uint8_t* mask1_out;
  uint8_t* mask2_out;
  uint64_t seed, counter;
  int64_t row_offset;
};

inline unsigned blocks(int64_t n) { return (unsigned)((n + kT - 1) / kT); }

int launch_gemm(const Ctx& c, ConvGemm cg, int nz = 1) {
  GemmArgs& g = cg.g;
  if (g.M <= 0 || g.N <= 0) return ABD_OK;
  if (cg.mode != 2) g.kchunk = std::max(g.K, 1);
  if (cg.mode) {
    cg.invH = 1.0f / (float)cg.H;
    cg.invW = 1.0f / (float)cg.W;
  }
  return launch_tiled(c.s, g.M, g.N, nz, c.n->large_min_blocks, conv_gemm_kernel<1, 1>, conv_gemm_kernel<2, 2>, cg);
}

int launch_gemm(const Ctx& c, const GemmArgs& g) {
  ConvGemm cg{};
  cg.g = g;
  return launch_gemm(c, cg);
}

// out[cols] = column sums of A; two fixed-order stages past kColsumRows rows
int colsum(const Ctx& c, const float* A, int64_t rows, int64_t cols, float* out) {
  return launch_colsum(c, A, rows, cols, cols, out, 0, kMaxC, kColsumRows);
}

// y (pixels, Cout) = conv(x (pixels, Cin)) + bias [relu]
int conv_fwd(const Ctx& c, int l, const float* x, float* y, int H, int W, int relu) {
  const ConvLayer& cv = kConv[l];
  ConvGemm cg{};
  cg.g = gemm_nt(x, cv.Cin, c.at<float>(c.L.wf[l]), y, (int)(c.B * H * W), cv.Cout, 9 * cv.Cin);
  cg.g.bias1 = c.p(cv.pb);
  cg.mode = 1, cg.H = H, cg.W = W, cg.C = cv.Cin, cg.sign = 1, cg.relu = relu;
  return launch_gemm(c, cg);
}

// dx (pixels, Cin) = conv(dy, the flipped kernel), kept where mask > 0
int conv_dgrad(const Ctx& c, int l, const float* dy, float* dx, const float* mask, int H, int W) {
  const ConvLayer& cv = kConv[l];
  ConvGemm cg{};
  cg.g = gemm_nn(dy, cv.Cout, c.at<float>(c.L.wd[l]), dx, (int)(c.B * H * W), cv.Cin, 9 * cv.Cout);
  cg.mode = 1, cg.H = H, cg.W = W, cg.C = cv.Cout, cg.sign = -1, cg.mask = mask;
  return launch_gemm(c, cg);
}

// dW[co][ci][tap] = sum over pixels of dy[p][co] x[p + tap][ci], sliced; the bias gradient = column sums of dy
int conv_wgrad(const Ctx& c, int l, const float* dy, const float* x, int H, int W) {
  const ConvLayer& cv = kConv[l];
  const int64_t px = c.B * H * W;
  const Slices sl = plan_slices(px, kMaxSlices, kSliceRows, kBK);
  ConvGemm cg{};
  cg.g = gemm_tn(dy, x, cv.Cin, c.at<float>(c.L.slab), cv.Cout, cv.Cin, px);
  cg.g.cz = (int64_t)cv.Cout * cv.Cin;
  cg.g.kchunk = (int)sl.kchunk;
  cg.mode = 2, cg.H = H, cg.W = W, cg.C = cv.Cin, cg.sign = 1;
  if (int rc = launch_gemm(c, cg, 9 * sl.ksplit)) return rc;
  wgrad_reduce_kernel<<<blocks(9 * cg.g.cz), kT, 0, c.s>>>(c.at<float>(c.L.slab), sl.ksplit, cv.Cout, cv.Cin,
                                                          c.g(cv.pw));
  ABD_LAUNCH_CHECK();
  return colsum(c, dy, px, cv.Cout, c.g(cv.pb));
}

int run_forward(const Ctx& c, const Fwd& f, bool need_wd) {
  const abd_largecnn* n = c.n;
  const int64_t B = c.B;
  for (int l = 0; l < 4; ++l) {
    const int e = 9 * kConv[l].Cin * kConv[l].Cout;
    repack_kernel<<<blocks(e), kT, 0, c.s>>>(c.p(kConv[l].pw), c.at<float>(c.L.wf[l]),
                                             need_wd ? c.at<float>(c.L.wd[l]) : nullptr, kConv[l].Cout, kConv[l].Cin);
    ABD_LAUNCH_CHECK();
  }
  float *a1 = c.at<float>(c.L.a1), *p1 = c.at<float>(c.L.p1), *a2 = c.at<float>(c.L.a2), *p2 = c.at<float>(c.L.p2);
  float *a3 = c.at<float>(c.L.a3), *a4 = c.at<float>(c.L.a4), *a5 = c.at<float>(c.L.a5), *p3 = c.at<float>(c.L.p3);
  int64_t e = B * n->H * n->W * kC1;
  conv1_fwd_kernel<<<blocks(e), kT, 0, c.s>>>(f.x, c.p(P_C1W), c.p(P_C1B), a1, e, n->H, n->W);
  ABD_LAUNCH_CHECK();
  e = B * n->H2 * n->W2 * kC1;
  pool2_fwd_kernel<<<blocks(e), kT, 0, c.s>>>(a1, p1, e, n->H, n->W, kC1);
  ABD_LAUNCH_CHECK();
  if (int rc = conv_fwd(c, 0, p1, a2, n->H2, n->W2, 0)) return rc;
  e = B * n->H4 * n->W4 * kC2;
  pool2_fwd_kernel<<<blocks(e), kT, 0, c.s>>>(a2, p2, e, n->H2, n->W2, kC2);
  ABD_LAUNCH_CHECK();
  if (int rc = conv_fwd(c, 1, p2, a3, n->H4, n->W4, 1)) return rc;
  if (int rc = conv_fwd(c, 2, a3, a4, n->H4, n->W4, 1)) return rc;
  if (int rc = conv_fwd(c, 3, a4, a5, n->H4, n->W4, 1)) return rc;
  e = B * n->lf;
  pool3_fwd_kernel<<<blocks(e), kT, 0, c.s>>>(a5, p3, e, n->H4, n->W4, n->PH, n->PW);
  ABD_LAUNCH_CHECK();
  // head
  float *h1 = c.at<float>(c.L.h1), *h2 = c.at<float>(c.L.h2), *z3 = c.at<float>(c.L.z3);
  GemmArgs g = gemm_nt(p3, n->lf, c.p(P_F1W), h1, (int)B, kF1, (int)n->lf);
  g.bias1 = c.p(P_F1B);
  if (int rc = launch_gemm(c, g)) return rc;
  act_fwd_kernel<<<blocks(B * kF1), kT, 0, c.s>>>(h1, B * kF1, kF1, 0, f.train, f.mask1_in, c.at<uint8_t>(c.L.keep1),
                                                  f.mask1_out, f.seed, f.counter, f.row_offset);
  ABD_LAUNCH_CHECK();
  g = gemm_nt(h1, kF1, c.p(P_F2W), h2, (int)B, kF2, kF1);
  g.bias1 = c.p(P_F2B);
  if (int rc = launch_gemm(c, g)) return rc;
  act_fwd_kernel<<<blocks(B * kF2), kT, 0, c.s>>>(h2, B * kF2, kF2, kF1, f.train, f.mask2_in, c.at<uint8_t>(c.L.keep2),
                                                  f.mask2_out, f.seed, f.counter, f.row_offset);
  ABD_LAUNCH_CHECK();
  g = gemm_nt(h2, kF2, c.p(P_F3W), z3, (int)B, n->K, kF2);
  g.bias1 = c.p(P_F3B);
  if (int rc = launch_gemm(c, g)) return rc;
  lsm_fwd_kernel<<<(unsigned)B, 64, 0, c.s>>>(z3, c.at<float>(c.L.logits), n->K);
  ABD_LAUNCH_CHECK();
  return ABD_OK;
}

// dlogp: the gradient of the log-probabilities the forward returned
int run_backward(const Ctx& c, const float* x, const float* dlogp) {
  const abd_largecnn* n = c.n;
  const int64_t B = c.B;
  const int K = n->K;
  float *dz3 = c.at<float>(c.L.dz3), *dh2 = c.at<float>(c.L.dh2), *dh1 = c.at<float>(c.L.dh1);
  float* dflat = c.at<float>(c.L.dflat);
  const float *h1 = c.at<float>(c.L.h1), *h2 = c.at<float>(c.L.h2), *p3 = c.at<float>(c.L.p3);
  lsm_bwd_kernel<<<(unsigned)B, 64, 0, c.s>>>(c.at<float>(c.L.logits), dlogp, dz3, K);
  ABD_LAUNCH_CHECK();
  if (int rc = launch_gemm(c, gemm_tn(dz3, h2, kF2, c.g(P_F3W), K, kF2, B))) return rc;
  if (int rc = colsum(c, dz3, B, K, c.g(P_F3B))) return rc;
  if (int rc = launch_gemm(c, gemm_nn(dz3, K, c.p(P_F3W), dh2, (int)B, kF2, K))) return rc;
  act_bwd_kernel<<<blocks(B * kF2), kT, 0, c.s>>>(dh2, h2, B * kF2);
  ABD_LAUNCH_CHECK();
  if (int rc = launch_gemm(c, gemm_tn(dh2, h1, kF1, c.g(P_F2W), kF2, kF1, B))) return rc;
  if (int rc = colsum(c, dh2, B, kF2, c.g(P_F2B))) return rc;
  if (int rc = launch_gemm(c, gemm_nn(dh2, kF2, c.p(P_F2W), dh1, (int)B, kF1, kF2))) return rc;
  act_bwd_kernel<<<blocks(B * kF1), kT, 0, c.s>>>(dh1, h1, B * kF1);
  ABD_LAUNCH_CHECK();
  if (int rc = launch_gemm(c, gemm_tn(dh1, p3, n->lf, c.g(P_F1W), kF1, (int)n->lf, B))) return rc;
  if (int rc = colsum(c, dh1, B, kF1, c.g(P_F1B))) return rc;
  if (int rc = launch_gemm(c, gemm_nn(dh1, kF1, c.p(P_F1W), dflat, (int)B, (int)n->lf, kF1))) return rc;
  // trunk
  const float *a1 = c.at<float>(c.L.a1), *p1 = c.at<float>(c.L.p1), *a2 = c.at<float>(c.L.a2);
  const float *p2 = c.at<float>(c.L.p2), *a3 = c.at<float>(c.L.a3), *a4 = c.at<float>(c.L.a4);
  const float* a5 = c.at<float>(c.L.a5);
  float *da5 = c.at<float>(c.L.da5), *da4 = c.at<float>(c.L.da4), *da3 = c.at<float>(c.L.da3);
  float *dp2 = c.at<float>(c.L.dp2), *da2 = c.at<float>(c.L.da2), *dp1 = c.at<float>(c.L.dp1);
  const int H4 = n->H4, W4 = n->W4, H2 = n->H2, W2 = n->W2;
  int64_t e = B * H4 * W4 * kC5;
  pool3_bwd_kernel<<<blocks(e), kT, 0, c.s>>>(a5, dflat, da5, e, H4, W4, n->PH, n->PW);
  ABD_LAUNCH_CHECK();
  if (int rc = conv_wgrad(c, 3, da5, a4, H4, W4)) return rc;
  if (int rc = conv_dgrad(c, 3, da5, da4, a4, H4, W4)) return rc;
  if (int rc = conv_wgrad(c, 2, da4, a3, H4, W4)) return rc;
  if (int rc = conv_dgrad(c, 2, da4, da3, a3, H4, W4)) return rc;
  if (int rc = conv_wgrad(c, 1, da3, p2, H4, W4)) return rc;
  if (int rc = conv_dgrad(c, 1, da3, dp2, nullptr, H4, W4)) return rc;
  e = B * H2 * W2 * kC2;
  pool2_bwd_kernel<<<blocks(e), kT, 0, c.s>>>(a2, dp2, da2, e, H2, W2, kC2);
  ABD_LAUNCH_CHECK();
  if (int rc = conv_wgrad(c, 0, da2, p1, H2, W2)) return rc;
  if (int rc = conv_dgrad(c, 0, da2, dp1, nullptr, H2, W2)) return rc;
  // conv1: pool1's backward is folded into the weight-gradient kernel; the bias sums dp1 (the pool only moves
  // each value to its maximum's position)
  const int64_t px = B * H2 * W2;
  const int nb = (int)std::min<int64_t>(kW1Blocks, (px + 63) / 64);
  const int64_t chunk = (px + nb - 1) / nb;
  float* part = c.at<float>(c.L.w1part);
  conv1_wgrad_kernel<<<nb, kW1Lanes * kC1, 0, c.s>>>(x, a1, dp1, part, px, chunk, n->H, n->W);
  ABD_LAUNCH_CHECK();
  colsum_kernel<<<dim3(blocks(kC1 * 9), 1), kRedT, 0, c.s>>>(part, nb, kC1 * 9, kC1 * 9, nb, c.g(P_C1W), 0, 0);
  ABD_LAUNCH_CHECK();
  return colsum(c, dp1, px, kC1, c.g(P_C1B));
}

int make_ctx(const abd_largecnn* net, int64_t B, const float* params, float* grads, void* ws, size_t bytes,
             abd_stream_t stream, Ctx* c) {
  return make_ctx(net, B, params, grads, ws, bytes, stream, kC1, make_layout, c);
}

int run_loss(const Ctx& c, const int64_t* labels, const int64_t* ind, bool grad, float scale, float* out,
             int64_t* metrics) {
  return run_ce(c, labels, ind, grad, scale, out, metrics);
}

Fwd fwd_of(const abd_largecnn_args* a, int train) {
  return Fwd{a->x, train, a->mask1_in, a->mask2_in, a->mask1_out, a->mask2_out, a->seed, a->counter, a->row_offset};
}

}  // namespace

extern "C" {

int abd_largecnn_tile_info(int what) {
  switch (what) {
    case 0: return kSmallTile;
    case 1: return kLargeTile;
    case 2: return kSliceRows;
    case 3: return kColsumRows;
    case 4: return kLargeMinBlocks;
    case 5: return kMaxSlices;
    default: return -1;
  }
}

int64_t abd_largecnn_linear_features(int H, int W) {
  if (H / 4 < 3 || W / 4 < 3) return -1;
  return (int64_t)kC5 * ((H / 4 - 3) / 2 + 1) * ((W / 4 - 3) / 2 + 1);
}

int abd_largecnn_create(int H, int W, int num_classes, abd_largecnn** net) {
  ABD_CHECK(net != nullptr, ABD_E_INVALID, "NULL out pointer");
  ABD_CHECK(H >= 1 && W >= 1 && H / 4 >= 3 && W / 4 >= 3, ABD_E_UNSUPPORTED,
            "largecnn: input %d x %d leaves pool3 no 3 x 3 window (12 x 12 is the smallest)", H, W);
  ABD_CHECK(H <= kMaxDim && W <= kMaxDim, ABD_E_UNSUPPORTED, "largecnn: input %d x %d beyond %d per side", H, W,
            kMaxDim);
  ABD_CHECK(num_classes >= 1 && num_classes <= 4096, ABD_E_UNSUPPORTED, "num_classes must be in [1, 4096]");
  const int64_t lf = abd_largecnn_linear_features(H, W);
  ABD_CHECK((int64_t)H * W * kC1 < (1LL << 31) && lf * kF1 < (1LL << 31), ABD_E_UNSUPPORTED,
            "largecnn: input %d x %d takes the kernels' indices past 32 bits", H, W);
  auto* n = new abd_largecnn();
  n->H = H, n->W = W, n->K = num_classes, n->T = H * W;
  n->H2 = H / 2, n->W2 = W / 2, n->H4 = n->H2 / 2, n->W4 = n->W2 / 2;
  n->PH = (n->H4 - 3) / 2 + 1, n->PW = (n->W4 - 3) / 2 + 1;
  n->lf = lf;
  n->large_min_blocks = kLargeMinBlocks;
  const int64_t sz[P_COUNT] = {kC1 * 9, kC1, (int64_t)kC2 * kC1 * 9, kC2, (int64_t)kC3 * kC2 * 9, kC3,
                               (int64_t)kC4 * kC3 * 9, kC4, (int64_t)kC5 * kC4 * 9, kC5, kF1 * lf, kF1,
                               kF2 * kF1, kF2, (int64_t)num_classes * kF2, num_classes};
  n->off[0] = 0;
  for (int i = 0; i < P_COUNT; ++i) n->off[i + 1] = n->off[i] + sz[i];
  *net = n;
  return ABD_OK;
}

void abd_largecnn_destroy(abd_largecnn* net) { delete net; }

int abd_largecnn_set_large_min_blocks(abd_largecnn* net, int min_blocks) {
  ABD_CHECK(net != nullptr && min_blocks >= 1, ABD_E_INVALID, "NULL network or min_blocks < 1");
  net->large_min_blocks = min_blocks;
  return ABD_OK;
}

int64_t abd_largecnn_param_count(const abd_largecnn* net) { return net ? net->off[P_COUNT] : 0; }

int abd_largecnn_param_offsets(const abd_largecnn* net, int64_t* offsets) {
  ABD_CHECK(net && offsets, ABD_E_INVALID, "NULL argument");
  for (int i = 0; i <= P_COUNT; ++i) offsets[i] = net->off[i];
  return ABD_OK;
}

size_t abd_largecnn_workspace_bytes(const abd_largecnn* net, int64_t batch) {
  if (!net || batch < 1) return 0;
  return make_layout(net, batch).total;
}

int64_t abd_largecnn_workspace_offset(const abd_largecnn* net, int64_t batch, const char* name) {
  if (!net || !name || batch < 1) return -1;
  const Layout L = make_layout(net, batch);
  const NamedOffset tab[] = {
      {"a1", L.a1}, {"p1", L.p1}, {"a2", L.a2}, {"p2", L.p2}, {"a3", L.a3}, {"a4", L.a4}, {"a5", L.a5},
      {"p3", L.p3}, {"h1", L.h1}, {"h2", L.h2}, {"z3", L.z3}, {"logits", L.logits}, {"dlogits", L.dlogits},
      {"rowinfo", L.rowinfo}, {"keep1", L.keep1}, {"keep2", L.keep2}, {"da2", L.da2}};
  return find_offset(tab, name);
}

int abd_largecnn_forward(abd_largecnn* net, const abd_largecnn_args* a, int train_mode, void* workspace,
                         size_t workspace_bytes, abd_stream_t stream) {
  ABD_CHECK(a != nullptr && a->x, ABD_E_INVALID, "NULL x");
  Ctx c;
  if (int rc = make_ctx(net, a->batch, a->params, a->grads, workspace, workspace_bytes, stream, &c)) return rc;
  if (int rc = run_forward(c, fwd_of(a, train_mode ? 1 : 0), train_mode != 0)) return rc;
  return run_loss(c, nullptr, nullptr, false, 1.0f, a->logits_out, nullptr);
}

int abd_largecnn_backward(abd_largecnn* net, const abd_largecnn_args* a, const float* dlogits, void* workspace,
                          size_t workspace_bytes, abd_stream_t stream) {
  ABD_CHECK(a != nullptr && a->x && a->grads && dlogits, ABD_E_INVALID, "NULL x / grads / dlogits");
  Ctx c;
  if (int rc = make_ctx(net, a->batch, a->params, a->grads, workspace, workspace_bytes, stream, &c)) return rc;
  return run_backward(c, a->x, dlogits);
}

int abd_largecnn_train_step(abd_largecnn* net, const abd_largecnn_args* a, void* workspace, size_t workspace_bytes,
                            abd_stream_t stream) {
  if (int rc = check_train_args(a)) return rc;
  Ctx c;
  if (int rc = make_ctx(net, a->batch, a->params, a->grads, workspace, workspace_bytes, stream, &c)) return rc;
  if (int rc = run_forward(c, fwd_of(a, 1), true)) return rc;
  if (int rc = run_loss(c, a->labels, a->indicators, true, a->grad_scale, a->logits_out, a->metrics)) return rc;
  if (int rc = run_backward(c, a->x, c.at<float>(c.L.dlogits))) return rc;
  return adam_tail(a, net->off[P_COUNT], stream);
}

int abd_largecnn_eval(abd_largecnn* net, const float* x, int64_t batch, const float* params, const int64_t* labels,
                      const int64_t* indicators, float* logits, int64_t* metrics, void* workspace,
                      size_t workspace_bytes, abd_stream_t stream) {
  ABD_CHECK(x && logits, ABD_E_INVALID, "NULL x / logits");
  Ctx c;
  if (int rc = make_ctx(net, batch, params, nullptr, workspace, workspace_bytes, stream, &c)) return rc;
  const Fwd f{x, 0, nullptr, nullptr, nullptr, nullptr, 0, 0, 0};
  if (int rc = run_forward(c, f, false)) return rc;
  return run_loss(c, labels, indicators, false, 1.0f, logits, metrics);
}

}  // extern "C"
