// smalllstm (reference utils/models.py:121-178) on gfx950: conv1 2x2 (1->64) relu bn1 pool(1,3); conv2 2x2 (64->64)
// relu bn2 pool(2,2) padding (1,1); conv3 2x2 (64->32) relu bn3 pool(2,2) padding (0,1); Dropout(0.4); the pooled map
// in channels-last layout is the input of nn.LSTM(32 Wf, 128, 2, batch_first); fc2 on the top layer's last step;
// log_softmax; cross entropy on the log-probabilities.  fc1 is a parameter the forward never reads: its gradient
// is written as zero.  fp32 only.
//
// Activations are channels-last (B, H, W, C) in the workspace.  ReLU comes BEFORE BatchNorm: z<i> is the conv
// output after bias and ReLU (what BatchNorm reads), a<i> the BatchNorm output, p<i> the pooled map.  The pools'
// argmax is torch's: the first maximum of the row-major window scan over the positions inside the map, so a window
// of ReLU zeros (equal values after the affine map, whatever gamma's sign) gives its gradient to its first
// position; backward recomputes it from a<i>.
//
// conv1 (Cin = 1) is a direct kernel.  conv2 and conv3 are implicit GEMMs on v_mfma_f32_16x16x4_f32 (conv_kernel):
// a 64-row block tile with the whole N in 2 or 4 accumulators per wave, K = 4 Cin in steps of 16 (one tap's channels):
//   forward        M = output pixels, N = Cout, K = 4 Cin; A = the four gathered pixel rows
//   data gradient  M = input pixels,  N = Cin,  K = 4 Cout; the same gather mirrored, zero outside the map
//   weight grad    M = 4 Cin (tap, channel), N = Cout, K = output pixels in slices (plan_slices) summed in order
// BatchNorm sums are per-block double partials summed in block order.  The LSTM's input projections, data and
// weight gradients are gemm_tiled_kernel (GemmArgs, launch_tiled).
//
// Recurrence: ONE launch per layer for all T steps, forward and BPTT alike.  A workgroup of 8 waves owns 16 batch
// rows for the whole sequence and never looks at another workgroup.  W_hh (512 x 128 fp32 = 256 KiB, more than the
// LDS) stays in registers for all steps as the B operands of v_mfma_f32_16x16x4_f32, 128 per lane:
//   forward  wave w owns hidden units 16 w .. 16 w + 15 in all four gates (4 N tiles x 32 K steps); h_{t-1} goes
//            through LDS (double buffered: one barrier per step); a lane ends up with i, f, g, o of its (4 rows,
//            1 unit), so c_t stays in registers and the cell is finished in the lane.
//   BPTT     wave w owns the same units of dh_{t-1} = dG_t W_hh (1 N tile x 128 K steps, K = 512 in four chains of
//            32 steps, one per gate block, added in a fixed order); dG_t goes through LDS; dh and dc stay in the lane.
// No float atomics anywhere; two runs are bit-equal.
#include <algorithm>
#include <cmath>

#include "abd_common.h"

struct abd_smalllstm {
  int H, W, K;
  int T;                 // H1 * W1: the rows per batch element the shared make_ctx checks against 32 bits
  int H1, W1, Wp1, H2, W2, Hp2, Wp2, H3, W3, TS, Wf;   // TS: the sequence length
  int F;                 // 32 * Wf
  int64_t off[25];
  int64_t roff[4];
};

namespace {

constexpr int kT = 256;
constexpr int kBM = 64;            // rows of a conv block tile
constexpr int kCK = 16;            // the convs' K-step: sixteen channels of one tap, or sixteen pixels
constexpr int kLd = kCK + 1;       // LDS row pitch of the conv A tile
constexpr int kSliceRows = 256;    // least rows of one weight-gradient slice
constexpr int kMaxSlices = 128;    // most slices of a conv weight gradient
constexpr int kGemmSlices = 8;     // most slices of an LSTM weight gradient
constexpr int kStatRows = 512;     // least pixels of one BatchNorm partial block
constexpr int kStatBlocks = 256;   // most partial blocks of one BatchNorm reduction
constexpr int kLargeMinBlocks = 96;  // below this many 128 x 128 blocks the 64 x 64 GEMM tile fills more CUs
constexpr int kW1Blocks = 512;     // most partial blocks of conv1's weight gradient
constexpr int kC1 = 64, kC2 = 64, kC3 = 32;
constexpr int kHid = 128;          // LSTM hidden size
constexpr int kGates = 4 * kHid;   // gate rows, torch order i f g o
constexpr int kLayers = 2;
constexpr int kFc1In = 224;        // fc1 (224 -> 128): in state_dict(), unused by forward
constexpr int kRT = 512;           // threads of a recurrent workgroup: 8 waves
constexpr int kRecRows = 16;       // batch rows of a recurrent workgroup
constexpr int kHp = kHid + 4;      // LDS pitch of an h row
constexpr int kGp = kGates + 4;    // LDS pitch of a dG row
constexpr int kMaxDim = 4096;
constexpr float kBnEps = 1e-5f, kBnMomentum = 0.1f;
constexpr float kDropP = 0.4f;

enum { P_C1W, P_C1B, P_BN1W, P_BN1B, P_C2W, P_C2B, P_BN2W, P_BN2B, P_C3W, P_C3B, P_BN3W, P_BN3B,
       P_WIH0, P_WHH0, P_BIH0, P_BHH0, P_WIH1, P_WHH1, P_BIH1, P_BHH1, P_F1W, P_F1B, P_F2W, P_F2B, P_COUNT };

// backward cell, sigmoid_acc, colsum, weight_grad; GemmArgs and its three forms, keep_hash, the host helpers;
// colsum_kernel, ce_kernel, metrics_kernel
#include "lstm_common.inc"
#include "gemm_tiled_kernel.inc"   // kBK, the tile sizes, f16v, gemm_tiled_kernel and launch_gemm
// f4v, tile_mfma, wgrad_reduce_kernel, blocks, stat_plan, the ABI entries of a net with running statistics
#include "conv16_common.inc"
#include "log_softmax.inc"   // lsm_fwd_kernel, lsm_bwd_kernel

// ------------------------------------------------------------------ 2x2 conv as an implicit GEMM
// The gather: pixel (b, h, w) of the Hr x Wr index map and tap (dy, dx) = (tap / 2, tap % 2) read pixel
// (h + sign dy, w + sign dx) of the Hs x Ws source map, nothing outside it.  Forward and weight gradient: sign = 1
// over the output pixels (always inside); data gradient: sign = -1 over the input pixels (full correlation).
// MODE 1: out (pixels, N) = A mat [+ bias] [relu], A(m, tap C + c) = channel c of the gathered pixel, mat (4 C, N).
// MODE 2: out + z (4 C) N, (4 C, N) = A^T mat over the pixels [z kchunk, (z + 1) kchunk), mat (pixels, N).
struct ConvArgs {
  const float* src;
  const float* mat;
  const float* bias;
  float* out;
  int Hr, Wr, Hs, Ws, C, sign, relu;
  int pixels, kchunk;
};

__device__ __forceinline__ int64_t src_pixel(const ConvArgs& a, int b, int h, int w, int tap) {
  const int nh = h + a.sign * (tap >> 1), nw = w + a.sign * (tap & 1);
  if ((unsigned)nh >= (unsigned)a.Hs || (unsigned)nw >= (unsigned)a.Ws) return -1;
  return ((int64_t)b * a.Hs + nh) * a.Ws + nw;
}

template <int TN, int MODE>
__global__ void __launch_bounds__(kT) conv_kernel(ConvArgs a) {
  constexpr int BN = 16 * TN, LDB = BN + 8;
  __shared__ float As[kBM * kLd];
  __shared__ float Bs[kCK * LDB];
  const int tid = threadIdx.x, lane = tid & 63, wm = (tid >> 6) * 16;
  const int lo = tid & 15, hi = tid >> 4;
  const int m0 = blockIdx.x * kBM;
  const int HW = a.Hr * a.Wr, C = a.C;
  const int M = MODE == 1 ? a.pixels : 4 * C;
  const int k0 = MODE == 1 ? 0 : blockIdx.z * a.kchunk;
  const int k1 = MODE == 1 ? 4 * C : min(a.pixels, k0 + a.kchunk);
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
  // the sixteen products of one K-step are chained on the matrix pipe in fp32 from zero; the K-steps are summed in
  // double, in order, so a 256-term sum rounds like a 16-term one
  typedef double d4v __attribute__((ext_vector_type(4)));
  d4v acc[TN];
#pragma unroll
  for (int j = 0; j < TN; ++j)
#pragma unroll
    for (int r = 0; r < 4; ++r) acc[j][r] = 0.0;
  for (int kb = k0; kb < k1; kb += kCK) {
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
      qw += kCK;   // the same lane of the next step is sixteen pixels on
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
    f4v part[TN];
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) part[j][r] = 0.0f;
    tile_mfma<TN, kCK>(As, Bs, LDB, wm, lane, part);
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) acc[j][r] += (double)part[j][r];
  }
  float* out = MODE == 1 ? a.out : a.out + (int64_t)blockIdx.z * M * BN;
#pragma unroll
  for (int j = 0; j < TN; ++j) {
    const int n = j * 16 + (lane & 15);
    const float bias = (MODE == 1 && a.bias) ? a.bias[n] : 0.0f;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int m = m0 + wm + (lane >> 4) * 4 + r;
      if (m < M) {
        float v = (float)(acc[j][r] + (double)bias);
        if (MODE == 1 && a.relu) v = fmaxf(v, 0.0f);
        out[(int64_t)m * BN + n] = v;
      }
    }
  }
}

// ------------------------------------------------------------------ small kernels
// (Cout, Cin, 2, 2) -> wf (tap, Cin, Cout) and wd (tap, Cout, Cin); blockIdx.y: conv2, conv3
struct RepackArgs {
  const float* w[2];
  float* wf[2];
  float* wd[2];
  int cin[2], cout[2];
  int need_wd;
};

__global__ void __launch_bounds__(kT) repack_kernel(RepackArgs a) {
  const int u = blockIdx.y;
  const int Cin = a.cin[u], Cout = a.cout[u];
  const int e = blockIdx.x * kT + threadIdx.x;
  if (e >= Cout * Cin * 4) return;
  const int tap = e & 3, ci = (e >> 2) % Cin, co = e / (4 * Cin);
  const float v = a.w[u][e];
  a.wf[u][((int64_t)tap * Cin + ci) * Cout + co] = v;
  if (a.need_wd) a.wd[u][((int64_t)tap * Cout + co) * Cin + ci] = v;
}

// conv1: z (B, H1, W1, 64) = relu(bias + the four taps of x (B, H, W)); one thread per output value
__global__ void __launch_bounds__(kT) conv1_fwd_kernel(const float* x, const float* w, const float* bias, float* z,
                                                       int64_t n, int H, int W) {
  const int64_t e = (int64_t)blockIdx.x * kT + threadIdx.x;
  if (e >= n) return;
  const int H1 = H - 1, W1 = W - 1;
  const int c = (int)(e % kC1);
  const int64_t p = e / kC1;
  const int r = (int)(p % ((int64_t)H1 * W1));
  const int64_t b = p / ((int64_t)H1 * W1);
  const int h = r / W1, xw = r - h * W1;
  const float* s = x + (b * H + h) * W + xw;
  // four products and the bias in double, rounded once: an input far from zero costs no more than the rounding
  double v = (double)bias[c];
  v += (double)s[0] * (double)w[c * 4 + 0];
  v += (double)s[1] * (double)w[c * 4 + 1];
  v += (double)s[W] * (double)w[c * 4 + 2];
  v += (double)s[W + 1] * (double)w[c * 4 + 3];
  z[e] = fmaxf((float)v, 0.0f);
}

// conv1's weight gradient: block i takes output pixels [i chunk, (i + 1) chunk); thread (lane, channel) walks its
// lane's pixels; part (blocks, 64, 4) holds the four lanes summed in lane order
__global__ void __launch_bounds__(kT) conv1_wgrad_kernel(const float* x, const float* dz, float* part, int64_t pixels,
                                                         int64_t chunk, int H, int W) {
  constexpr int kLanes = kT / kC1;
  __shared__ float red[kLanes][kC1][4];
  const int c = threadIdx.x % kC1, l = threadIdx.x / kC1;
  const int H1 = H - 1, W1 = W - 1;
  const int64_t q0 = (int64_t)blockIdx.x * chunk, q1 = min(pixels, q0 + chunk);
  float acc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
  for (int64_t q = q0 + l; q < q1; q += kLanes) {
    const float g = dz[q * kC1 + c];
    const int r = (int)(q % ((int64_t)H1 * W1));
    const int64_t b = q / ((int64_t)H1 * W1);
    const int h = r / W1, xw = r - h * W1;
    const float* s = x + (b * H + h) * W + xw;
    acc[0] = fmaf(g, s[0], acc[0]);
    acc[1] = fmaf(g, s[1], acc[1]);
    acc[2] = fmaf(g, s[W], acc[2]);
    acc[3] = fmaf(g, s[W + 1], acc[3]);
  }
#pragma unroll
  for (int t = 0; t < 4; ++t) red[l][c][t] = acc[t];
  __syncthreads();
  if (l == 0) {
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      float s = red[0][c][t];
      for (int j = 1; j < kLanes; ++j) s += red[j][c][t];
      part[((int64_t)blockIdx.x * kC1 + c) * 4 + t] = s;
    }
  }
}

// ------------------------------------------------------------------ BatchNorm (its input z is already the ReLU's output)
// Two sums per channel over a (pixels, C) map, block i over pixels [i chunk, (i + 1) chunk), thread (lane, channel)
// over its lane's pixels in double; part (blocks, 2, C) holds the lanes summed in lane order.
//   mode 0: sum z and sum z^2 (the batch statistics)
//   mode 1: sum g and sum g xhat, xhat = (z - mean) invstd
//   mode 2: sum g (a conv bias gradient)
__global__ void __launch_bounds__(kT) bn_reduce_kernel(const float* z, const float* g, const float* stat, double* part,
                                                       int64_t pixels, int64_t chunk, int C, int mode) {
  __shared__ double red[2][kT];
  const int c = threadIdx.x % C, l = threadIdx.x / C, lanes = kT / C;
  const int64_t p0 = (int64_t)blockIdx.x * chunk, p1 = min(pixels, p0 + chunk);
  const float mean = mode == 1 ? stat[c] : 0.0f, invstd = mode == 1 ? stat[C + c] : 0.0f;
  double s0 = 0.0, s1 = 0.0;
  for (int64_t p = p0 + l; p < p1; p += lanes) {
    const int64_t i = p * C + c;
    if (mode == 0) {
      const float v = z[i];
      s0 += (double)v;
      s1 += (double)v * (double)v;
    } else if (mode == 1) {
      const float gv = g[i];
      s0 += (double)gv;
      s1 += (double)gv * (double)((z[i] - mean) * invstd);
    } else {
      s0 += (double)g[i];
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
__global__ void __launch_bounds__(64) bn_finalize_kernel(const double* part, int nb, int C, int64_t n, float* stat,
                                                         double* statd, float* rmean, float* rvar, int64_t* nbt) {
  const int c = threadIdx.x;
  if (c >= C) return;
  double s = 0.0, q = 0.0;
  for (int b = 0; b < nb; ++b) s += part[((int64_t)b * 2 + 0) * C + c], q += part[((int64_t)b * 2 + 1) * C + c];
  const double mean = s / (double)n;
  const double var = fmax(q / (double)n - mean * mean, 0.0);
  stat[c] = (float)mean;
  stat[C + c] = (float)(1.0 / sqrt(var + (double)kBnEps));
  statd[c] = mean;   // what bn_apply_kernel normalises with
  statd[C + c] = 1.0 / sqrt(var + (double)kBnEps);
  if (rmean) {
    const double unbiased = n > 1 ? var * (double)n / (double)(n - 1) : var;
    rmean[c] = (float)((1.0 - (double)kBnMomentum) * (double)rmean[c] + (double)kBnMomentum * mean);
    rvar[c] = (float)((1.0 - (double)kBnMomentum) * (double)rvar[c] + (double)kBnMomentum * unbiased);
  }
  if (nbt && c == 0) *nbt += 1;
}

// eval mode: stat = running mean, 1 / sqrt(running var + eps)
__global__ void __launch_bounds__(64) bn_eval_stat_kernel(const float* rmean, const float* rvar, int C, float* stat,
                                                          double* statd) {
  const int c = threadIdx.x;
  if (c >= C) return;
  stat[c] = rmean[c];
  stat[C + c] = (float)(1.0 / sqrt((double)rvar[c] + (double)kBnEps));
  statd[c] = (double)rmean[c];
  statd[C + c] = 1.0 / sqrt((double)rvar[c] + (double)kBnEps);
}

// out0[c] = the first sums, out1[c] (optional) = the second sums of the partials, in block order
__global__ void __launch_bounds__(64) part_sum_kernel(const double* part, int nb, int C, float* out0, float* out1) {
  const int c = threadIdx.x;
  if (c >= C) return;
  double s = 0.0, q = 0.0;
  for (int b = 0; b < nb; ++b) s += part[((int64_t)b * 2 + 0) * C + c], q += part[((int64_t)b * 2 + 1) * C + c];
  out0[c] = (float)s;
  if (out1) out1[c] = (float)q;
}

// a = gamma xhat + beta, in double from the double statistics, rounded once
__global__ void __launch_bounds__(kT) bn_apply_kernel(const float* z, const double* stat, const float* gamma,
                                                      const float* beta, float* a, int64_t n, int C) {
  const int64_t e = (int64_t)blockIdx.x * kT + threadIdx.x;
  if (e >= n) return;
  const int c = (int)(e % C);
  a[e] = (float)(((double)z[e] - stat[c]) * stat[C + c] * (double)gamma[c] + (double)beta[c]);
}

// the gradient at the conv output in front of the ReLU: gamma invstd / n (n g - d(beta) - xhat d(gamma)) where z > 0
__global__ void __launch_bounds__(kT) bn_bwd_apply_kernel(const float* z, const float* g, const float* stat,
                                                          const float* gamma, const float* dgamma, const float* dbeta,
                                                          float count, float* dz, int64_t n, int C) {
  const int64_t e = (int64_t)blockIdx.x * kT + threadIdx.x;
  if (e >= n) return;
  const int c = (int)(e % C);
  const float v = z[e];
  const float xh = (v - stat[c]) * stat[C + c];
  const float d = gamma[c] * stat[C + c] / count * (count * g[e] - dbeta[c] - xh * dgamma[c]);
  dz[e] = v > 0.0f ? d : 0.0f;
}

// ------------------------------------------------------------------ max pools (kernel == stride: windows do not overlap)
struct PoolArgs {
  int H, W, OH, OW, C, kh, kw, ph, pw;
};

// the first maximum of window (oh, ow) in torch's row-major scan over the positions inside the map: its pixel index
// h W + w.  Every window of an accepted geometry has at least one position inside.
__device__ __forceinline__ int pool_argmax(const float* a, const PoolArgs& g, int64_t b, int oh, int ow, int c,
                                           float& best) {
  int arg = -1;
  best = -INFINITY;
  for (int i = 0; i < g.kh; ++i) {
    const int h = oh * g.kh - g.ph + i;
    if ((unsigned)h >= (unsigned)g.H) continue;
    for (int j = 0; j < g.kw; ++j) {
      const int w = ow * g.kw - g.pw + j;
      if ((unsigned)w >= (unsigned)g.W) continue;
      const float v = a[((b * g.H + h) * g.W + w) * g.C + c];
      if (arg < 0 || v > best) best = v, arg = h * g.W + w;
    }
  }
  return arg;
}

__global__ void __launch_bounds__(kT) pool_fwd_kernel(const float* a, float* p, int64_t n, PoolArgs g) {
  const int64_t e = (int64_t)blockIdx.x * kT + threadIdx.x;
  if (e >= n) return;
  const int c = (int)(e % g.C);
  int64_t q = e / g.C;
  const int ow = (int)(q % g.OW);
  q /= g.OW;
  const int oh = (int)(q % g.OH);
  float best;
  pool_argmax(a, g, q / g.OH, oh, ow, c, best);
  p[e] = best;
}

// da (B, H, W, C) = dp of the window the position is the argmax of, zero elsewhere and on dropped rows / columns
__global__ void __launch_bounds__(kT) pool_bwd_kernel(const float* a, const float* dp, float* da, int64_t n, PoolArgs g) {
  const int64_t e = (int64_t)blockIdx.x * kT + threadIdx.x;
  if (e >= n) return;
  const int c = (int)(e % g.C);
  int64_t q = e / g.C;
  const int w = (int)(q % g.W);
  q /= g.W;
  const int h = (int)(q % g.H);
  const int64_t b = q / g.H;
  const int oh = (h + g.ph) / g.kh, ow = (w + g.pw) / g.kw;
  float v = 0.0f;
  if (oh < g.OH && ow < g.OW) {
    float best;
    if (pool_argmax(a, g, b, oh, ow, c, best) == h * g.W + w) v = dp[((b * g.OH + oh) * g.OW + ow) * g.C + c];
  }
  da[e] = v;
}

// ------------------------------------------------------------------ dropout, log_softmax
// seq (B, T, Wf, 32) = p3 kept and scaled by 1 / 0.6 (train) or p3 (eval).  keep is in the reference's
// (B, 32, T, Wf) element order; it comes from mask_in or the hash of (seed, counter, global element).
__global__ void __launch_bounds__(kT) dropout_fwd_kernel(const float* p3, float* seq, int64_t n, int TS, int Wf, int train,
                                                         const uint8_t* mask_in, uint8_t* keep, uint8_t* mask_out,
                                                         uint64_t seed, uint64_t counter, int64_t row_offset) {
  const int64_t e = (int64_t)blockIdx.x * kT + threadIdx.x;
  if (e >= n) return;
  if (!train) {
    seq[e] = p3[e];
    return;
  }
  const int c = (int)(e % kC3);
  int64_t q = e / kC3;
  const int w = (int)(q % Wf);
  q /= Wf;
  const int t = (int)(q % TS);
  const int64_t b = q / TS;
  const int64_t per = (int64_t)kC3 * TS * Wf;
  const int64_t in = ((int64_t)c * TS + t) * Wf + w;
  const uint8_t k = mask_in ? (mask_in[b * per + in] != 0)
                            : keep_hash(seed, counter, (uint64_t)((row_offset + b) * per + in), kDropP);
  keep[b * per + in] = k;
  if (mask_out) mask_out[b * per + in] = k;
  seq[e] = k ? p3[e] * (1.0f / (1.0f - kDropP)) : 0.0f;
}

// dseq -> d(p3), in place
__global__ void __launch_bounds__(kT) dropout_bwd_kernel(float* dseq, const uint8_t* keep, int64_t n, int TS, int Wf) {
  const int64_t e = (int64_t)blockIdx.x * kT + threadIdx.x;
  if (e >= n) return;
  const int c = (int)(e % kC3);
  int64_t q = e / kC3;
  const int w = (int)(q % Wf);
  q /= Wf;
  const int t = (int)(q % TS);
  const int64_t b = q / TS;
  const int64_t per = (int64_t)kC3 * TS * Wf;
  dseq[e] = keep[b * per + ((int64_t)c * TS + t) * Wf + w] ? dseq[e] * (1.0f / (1.0f - kDropP)) : 0.0f;
}

// ------------------------------------------------------------------ recurrence
struct RecArgs {
  float* gates;        // [B*T][512]: x_t W_ih^T + b_ih + b_hh on entry; activated i f g o after the forward
                       // launch; the pre-activation gate gradients after the BPTT launch
  float* h;            // [B][T][128]
  float* c;            // [B][T][128]
  const float* whh;    // [512][128]
  const float* dy;     // BPTT: [B][T][128] gradient of this layer's output, or NULL
  const float* dlast;  // BPTT: [B][128] added to dh at the last step (the head's gradient), or NULL
  int B, T;
};

// All T steps of one layer for batch rows [16 blockIdx.x, +16).  Lane (col = lane & 15, kq = lane >> 4) of wave w:
// unit u = 16 w + col; B operands wr[gate][kk] = W_hh[gate 128 + u][4 kk + kq]; after the products acc[gate][r] is
// gate `gate` of row 4 kq + r, unit u.
__global__ void __launch_bounds__(kRT) lstm_rec_fwd_kernel(RecArgs a) {
  __shared__ float hs[2][kRecRows * kHp];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int col = lane & 15, kq = lane >> 4;
  const int u = w * 16 + col;
  const int b0 = blockIdx.x * kRecRows;
  const int T = a.T;
  float wr[4][kHid / 4];
#pragma unroll
  for (int g = 0; g < 4; ++g)
#pragma unroll
    for (int kk = 0; kk < kHid / 4; ++kk) wr[g][kk] = a.whh[(int64_t)(g * kHid + u) * kHid + kk * 4 + kq];
  float cp[4] = {0.0f, 0.0f, 0.0f, 0.0f};
  for (int t = 0; t < T; ++t) {
    f4v acc[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int b = b0 + kq * 4 + r;
      const float* gp = a.gates + ((int64_t)b * T + t) * kGates + u;
#pragma unroll
      for (int g = 0; g < 4; ++g) acc[g][r] = b < a.B ? gp[g * kHid] : 0.0f;
    }
    if (t > 0) {   // h_{-1} = 0: nothing to multiply at the first step
      const float* hb = hs[t & 1];
#pragma unroll
      for (int kk = 0; kk < kHid / 4; ++kk) {
        const float av = hb[col * kHp + kk * 4 + kq];   // A[row col][k]
#pragma unroll
        for (int g = 0; g < 4; ++g) acc[g] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, wr[g][kk], acc[g], 0, 0, 0);
      }
    }
    float* hn = hs[(t + 1) & 1];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = kq * 4 + r, b = b0 + row;
      const float ig = sigmoid_acc(acc[0][r]);
      const float fg = sigmoid_acc(acc[1][r]);
      const float gg = tanhf(acc[2][r]);
      const float og = sigmoid_acc(acc[3][r]);
      const float ct = fg * cp[r] + ig * gg;
      const float ht = og * tanhf(ct);
      cp[r] = ct;
      hn[row * kHp + u] = b < a.B ? ht : 0.0f;
      if (b < a.B) {
        const int64_t bt = (int64_t)b * T + t;
        float* gp = a.gates + bt * kGates + u;
        gp[0] = ig;
        gp[kHid] = fg;
        gp[2 * kHid] = gg;
        gp[3 * kHid] = og;
        a.c[bt * kHid + u] = ct;
        a.h[bt * kHid + u] = ht;
      }
    }
    __syncthreads();   // h_t is in hs[(t + 1) & 1]; every read of hs[t & 1] is done
  }
}

// BPTT of one layer for the same rows, t = T-1 .. 0.  B operands wr[kk] = W_hh[4 kk + kq][u], kk = 0 .. 127; the
// four chains of 32 K-steps (one per gate block of dG) are added as (i + f) + (g + o).
__global__ void __launch_bounds__(kRT) lstm_rec_bwd_kernel(RecArgs a) {
  __shared__ float ds[kRecRows * kGp];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int col = lane & 15, kq = lane >> 4;
  const int u = w * 16 + col;
  const int b0 = blockIdx.x * kRecRows;
  const int T = a.T;
  float wr[kGates / 4];
#pragma unroll
  for (int kk = 0; kk < kGates / 4; ++kk) wr[kk] = a.whh[(int64_t)(kk * 4 + kq) * kHid + u];
  float dc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
  f4v dh;
#pragma unroll
  for (int r = 0; r < 4; ++r) dh[r] = 0.0f;
  for (int t = T - 1; t >= 0; --t) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = kq * 4 + r, b = b0 + row;
      float di = 0.0f, df = 0.0f, dg = 0.0f, dob = 0.0f;
      if (b < a.B) {
        const int64_t bt = (int64_t)b * T + t;
        float* gp = a.gates + bt * kGates + u;
        const float ig = gp[0], fg = gp[kHid], gg = gp[2 * kHid], og = gp[3 * kHid];
        const float ct = a.c[bt * kHid + u];
        const float cprev = t > 0 ? a.c[(bt - 1) * kHid + u] : 0.0f;
        float dht = dh[r];
        if (a.dy) dht += a.dy[bt * kHid + u];
        if (a.dlast && t == T - 1) dht += a.dlast[(int64_t)b * kHid + u];
        const float dcin = t < T - 1 ? dc[r] : 0.0f;
        lstm_cell_bwd(ig, fg, gg, og, ct, cprev, dht, dcin, di, df, dg, dob, dc[r]);
        gp[0] = di;
        gp[kHid] = df;
        gp[2 * kHid] = dg;
        gp[3 * kHid] = dob;
      }
      float* dr = ds + row * kGp + u;
      dr[0] = di;
      dr[kHid] = df;
      dr[2 * kHid] = dg;
      dr[3 * kHid] = dob;
    }
    if (t > 0) {   // dh_{t-1} = dG_t W_hh
      __syncthreads();
      f4v p[4];
#pragma unroll
      for (int g = 0; g < 4; ++g) {
#pragma unroll
        for (int r = 0; r < 4; ++r) p[g][r] = 0.0f;
#pragma unroll
        for (int kk = 0; kk < kHid / 4; ++kk) {
          const float av = ds[col * kGp + g * kHid + kk * 4 + kq];   // A[row col][k]
          p[g] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, wr[g * (kHid / 4) + kk], p[g], 0, 0, 0);
        }
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) dh[r] = (p[0][r] + p[1][r]) + (p[2][r] + p[3][r]);
      __syncthreads();   // the reads of ds are done before the next step overwrites it
    }
  }
}

// ------------------------------------------------------------------ host side
// workspace map (byte offsets); every buffer 256-byte aligned
struct Layout {
  size_t z[3], a[3], p[3], stat[3], statd[3], seq, keep, h[kLayers], c[kLayers], gates[kLayers], zfc, logits, dlogits, rowinfo;
  size_t wf[2], wd[2], part, g[2], dzfc, dhtop, dy, slab, w1part, colp, total;
  int ksplit;       // slices of the LSTM weight gradients
  int64_t kchunk;
};

struct Maps {   // pixels per clip of the z / a maps and the p maps, and their channels
  int64_t za[3], pp[3];
  int C[3];
};

Maps maps_of(const abd_smalllstm* n) {
  Maps m;
  m.za[0] = (int64_t)n->H1 * n->W1, m.pp[0] = (int64_t)n->H1 * n->Wp1, m.C[0] = kC1;
  m.za[1] = (int64_t)n->H2 * n->W2, m.pp[1] = (int64_t)n->Hp2 * n->Wp2, m.C[1] = kC2;
  m.za[2] = (int64_t)n->H3 * n->W3, m.pp[2] = (int64_t)n->TS * n->Wf, m.C[2] = kC3;
  return m;
}

Layout make_layout(const abd_smalllstm* n, int64_t B) {
  Layout L{};
  Take take;
  const Maps m = maps_of(n);
  for (int i = 0; i < 3; ++i) {
    L.z[i] = take(4 * (size_t)(B * m.za[i] * m.C[i]));
    L.a[i] = take(4 * (size_t)(B * m.za[i] * m.C[i]));
    L.p[i] = take(4 * (size_t)(B * m.pp[i] * m.C[i]));
    L.stat[i] = take(4 * 2 * m.C[i]);
    L.statd[i] = take(8 * 2 * m.C[i]);   // the same statistics unrounded
  }
  const size_t BT = (size_t)B * n->TS;
  L.seq = take(4 * BT * n->F);
  L.keep = take(BT * n->F);
  for (int l = 0; l < kLayers; ++l) {
    L.h[l] = take(4 * BT * kHid);
    L.c[l] = take(4 * BT * kHid);
    L.gates[l] = take(4 * BT * kGates);
  }
  L.zfc = take(4 * (size_t)B * n->K);
  L.logits = take(4 * (size_t)B * n->K);
  L.dlogits = take(4 * (size_t)B * n->K);
  L.rowinfo = take(4 * (size_t)B * 4);
  L.wf[0] = take(4 * 4 * kC1 * kC2), L.wd[0] = take(4 * 4 * kC1 * kC2);
  L.wf[1] = take(4 * 4 * kC2 * kC3), L.wd[1] = take(4 * 4 * kC2 * kC3);
  L.part = take(8 * (size_t)kStatBlocks * 2 * 64);
  // two gradient maps, each as large as the largest map (z1) or the sequence gradient
  const size_t gmax = std::max((size_t)(B * m.za[0] * kC1), BT * n->F);
  L.g[0] = take(4 * gmax), L.g[1] = take(4 * gmax);
  L.dzfc = take(4 * (size_t)B * n->K);
  L.dhtop = take(4 * (size_t)B * kHid);
  L.dy = take(4 * BT * kHid);
  const Slices sl = plan_slices((int64_t)BT, kGemmSlices, kSliceRows, kBK);
  L.ksplit = sl.ksplit;
  L.kchunk = sl.kchunk;
  size_t slab = L.ksplit > 1 ? (size_t)L.ksplit * kGates * std::max(kHid, n->F) : 0;
  slab = std::max(slab, (size_t)4 * kC1 * kC2 * plan_slices(B * m.za[1], kMaxSlices, kSliceRows, kCK).ksplit);
  slab = std::max(slab, (size_t)4 * kC2 * kC3 * plan_slices(B * m.za[2], kMaxSlices, kSliceRows, kCK).ksplit);
  L.slab = take(4 * slab);
  L.w1part = take(4 * (size_t)kW1Blocks * kC1 * 4);
  L.colp = take(4 * (size_t)64 * kGates);
  L.total = take.o;
  return L;
}

struct Ctx : CtxBase {
  const abd_smalllstm* n;
  Layout L;
  float* running;     // NULL: leave the running statistics alone
  int64_t* nbt;
  const float* p(int i) const { return params + n->off[i]; }
  float* g(int i) const { return grads + n->off[i]; }
  float* gb(int i) const { return at<float>(L.g[i]); }
};

template <int MODE>
int launch_conv(const Ctx& c, const ConvArgs& a, int N, int M, int nz) {
  dim3 grid((M + kBM - 1) / kBM, 1, nz);
  if (N == 32) conv_kernel<2, MODE><<<grid, kT, 0, c.s>>>(a);
  else conv_kernel<4, MODE><<<grid, kT, 0, c.s>>>(a);
  ABD_LAUNCH_CHECK();
  return ABD_OK;
}

// the geometry of conv i (1: conv2, 2: conv3): input map (p<i>), output map (z<i+1>), channels
struct ConvGeo {
  int Hi, Wi, Ho, Wo, Cin, Cout;
};
ConvGeo conv_geo(const abd_smalllstm* n, int i) {
  if (i == 1) return {n->H1, n->Wp1, n->H2, n->W2, kC1, kC2};
  return {n->Hp2, n->Wp2, n->H3, n->W3, kC2, kC3};
}

// z<i+1> = relu(conv(p<i>) + bias)
int conv_fwd(const Ctx& c, int i) {
  const ConvGeo q = conv_geo(c.n, i);
  ConvArgs a{};
  a.src = c.at<float>(c.L.p[i - 1]), a.mat = c.at<float>(c.L.wf[i - 1]), a.bias = c.p(4 * i + 1);
  a.out = c.at<float>(c.L.z[i]);
  a.Hr = q.Ho, a.Wr = q.Wo, a.Hs = q.Hi, a.Ws = q.Wi, a.C = q.Cin, a.sign = 1, a.relu = 1;
  a.pixels = (int)(c.B * q.Ho * q.Wo);
  return launch_conv<1>(c, a, q.Cout, a.pixels, 1);
}

// dx (input pixels, Cin) = the full correlation of dz with the kernel
int conv_dgrad(const Ctx& c, int i, const float* dz, float* dx) {
  const ConvGeo q = conv_geo(c.n, i);
  ConvArgs a{};
  a.src = dz, a.mat = c.at<float>(c.L.wd[i - 1]), a.out = dx;
  a.Hr = q.Hi, a.Wr = q.Wi, a.Hs = q.Ho, a.Ws = q.Wo, a.C = q.Cout, a.sign = -1;
  a.pixels = (int)(c.B * q.Hi * q.Wi);
  return launch_conv<1>(c, a, q.Cin, a.pixels, 1);
}

// dW[co][ci][tap] = sum over output pixels of dz[p][co] x[the tap's pixel][ci], sliced
int conv_wgrad(const Ctx& c, int i, const float* dz) {
  const ConvGeo q = conv_geo(c.n, i);
  const int64_t pixels = c.B * q.Ho * q.Wo;
  const Slices sl = plan_slices(pixels, kMaxSlices, kSliceRows, kCK);
  ConvArgs a{};
  a.src = c.at<float>(c.L.p[i - 1]), a.mat = dz, a.out = c.at<float>(c.L.slab);
  a.Hr = q.Ho, a.Wr = q.Wo, a.Hs = q.Hi, a.Ws = q.Wi, a.C = q.Cin, a.sign = 1;
  a.pixels = (int)pixels, a.kchunk = (int)sl.kchunk;
  if (int rc = launch_conv<2>(c, a, q.Cout, 4 * q.Cin, sl.ksplit)) return rc;
  wgrad_reduce_kernel<4><<<blocks(4 * q.Cin * q.Cout), kT, 0, c.s>>>(a.out, sl.ksplit, q.Cout, q.Cin, c.g(4 * i));
  ABD_LAUNCH_CHECK();
  return ABD_OK;
}

PoolArgs pool_geo(const abd_smalllstm* n, int i) {
  if (i == 0) return {n->H1, n->W1, n->H1, n->Wp1, kC1, 1, 3, 0, 0};
  if (i == 1) return {n->H2, n->W2, n->Hp2, n->Wp2, kC2, 2, 2, 1, 1};
  return {n->H3, n->W3, n->TS, n->Wf, kC3, 2, 2, 0, 1};
}

// a<i> = BatchNorm(z<i>), p<i> = pool(a<i>); train: batch statistics, running statistics updated when c.running
int bn_pool_fwd(const Ctx& c, int i, int train) {
  const Maps m = maps_of(c.n);
  const int C = m.C[i];
  const int64_t pixels = c.B * m.za[i];
  float *z = c.at<float>(c.L.z[i]), *a = c.at<float>(c.L.a[i]), *stat = c.at<float>(c.L.stat[i]);
  double* statd = c.at<double>(c.L.statd[i]);
  float* rm = c.running ? c.running + c.n->roff[i] : nullptr;
  if (train) {
    const StatPlan sp = stat_plan(pixels);
    double* part = c.at<double>(c.L.part);
    bn_reduce_kernel<<<sp.nb, kT, 0, c.s>>>(z, nullptr, nullptr, part, pixels, sp.chunk, C, 0);
    ABD_LAUNCH_CHECK();
    bn_finalize_kernel<<<1, 64, 0, c.s>>>(part, sp.nb, C, pixels, stat, statd, rm, rm ? rm + C : nullptr,
                                          (rm && c.nbt) ? c.nbt + i : nullptr);   // the counter advances only together with the statistics
    ABD_LAUNCH_CHECK();
  } else {
    bn_eval_stat_kernel<<<1, 64, 0, c.s>>>(rm, rm + C, C, stat, statd);
    ABD_LAUNCH_CHECK();
  }
  bn_apply_kernel<<<blocks(pixels * C), kT, 0, c.s>>>(z, statd, c.p(4 * i + 2), c.p(4 * i + 3), a, pixels * C, C);
  ABD_LAUNCH_CHECK();
  const int64_t e = c.B * m.pp[i] * C;
  pool_fwd_kernel<<<blocks(e), kT, 0, c.s>>>(a, c.at<float>(c.L.p[i]), e, pool_geo(c.n, i));
  ABD_LAUNCH_CHECK();
  return ABD_OK;
}

// dp (the gradient at p<i>) -> da in tmp -> dz (the gradient at conv i's output in front of its ReLU); the
// BatchNorm gradients and the conv's bias gradient on the way
int bn_pool_bwd(const Ctx& c, int i, const float* dp, float* tmp, float* dz) {
  const Maps m = maps_of(c.n);
  const int C = m.C[i];
  const int64_t pixels = c.B * m.za[i];
  const float *z = c.at<float>(c.L.z[i]), *a = c.at<float>(c.L.a[i]), *stat = c.at<float>(c.L.stat[i]);
  pool_bwd_kernel<<<blocks(pixels * C), kT, 0, c.s>>>(a, dp, tmp, pixels * C, pool_geo(c.n, i));
  ABD_LAUNCH_CHECK();
  const StatPlan sp = stat_plan(pixels);
  double* part = c.at<double>(c.L.part);
  bn_reduce_kernel<<<sp.nb, kT, 0, c.s>>>(z, tmp, stat, part, pixels, sp.chunk, C, 1);
  ABD_LAUNCH_CHECK();
  part_sum_kernel<<<1, 64, 0, c.s>>>(part, sp.nb, C, c.g(4 * i + 3), c.g(4 * i + 2));
  ABD_LAUNCH_CHECK();
  bn_bwd_apply_kernel<<<blocks(pixels * C), kT, 0, c.s>>>(z, tmp, stat, c.p(4 * i + 2), c.g(4 * i + 2), c.g(4 * i + 3),
                                                          (float)pixels, dz, pixels * C, C);
  ABD_LAUNCH_CHECK();
  bn_reduce_kernel<<<sp.nb, kT, 0, c.s>>>(z, dz, stat, part, pixels, sp.chunk, C, 2);
  ABD_LAUNCH_CHECK();
  part_sum_kernel<<<1, 64, 0, c.s>>>(part, sp.nb, C, c.g(4 * i + 1), nullptr);
  ABD_LAUNCH_CHECK();
  return ABD_OK;
}

RecArgs rec_args(const Ctx& c, int l) {
  RecArgs r{};
  r.gates = c.at<float>(c.L.gates[l]);
  r.h = c.at<float>(c.L.h[l]);
  r.c = c.at<float>(c.L.c[l]);
  r.whh = c.p(P_WHH0 + 4 * l);
  r.B = (int)c.B;
  r.T = c.n->TS;
  return r;
}

// a: the call's args struct, whose dropout fields a train-mode forward reads; NULL for eval
int run_forward(const Ctx& c, const float* x, int train, const abd_smalllstm_args* a) {
  const abd_smalllstm* n = c.n;
  const int64_t B = c.B;
  RepackArgs ra{};
  for (int u = 0; u < 2; ++u) {
    ra.w[u] = c.p(u ? P_C3W : P_C2W);
    ra.wf[u] = c.at<float>(c.L.wf[u]), ra.wd[u] = c.at<float>(c.L.wd[u]);
    ra.cin[u] = u ? kC2 : kC1, ra.cout[u] = u ? kC3 : kC2;
  }
  ra.need_wd = train;
  repack_kernel<<<dim3(blocks(4 * kC1 * kC2), 2), kT, 0, c.s>>>(ra);
  ABD_LAUNCH_CHECK();
  int64_t e = B * n->H1 * n->W1 * kC1;
  conv1_fwd_kernel<<<blocks(e), kT, 0, c.s>>>(x, c.p(P_C1W), c.p(P_C1B), c.at<float>(c.L.z[0]), e, n->H, n->W);
  ABD_LAUNCH_CHECK();
  if (int rc = bn_pool_fwd(c, 0, train)) return rc;
  if (int rc = conv_fwd(c, 1)) return rc;
  if (int rc = bn_pool_fwd(c, 1, train)) return rc;
  if (int rc = conv_fwd(c, 2)) return rc;
  if (int rc = bn_pool_fwd(c, 2, train)) return rc;
  const int TS = n->TS;
  const int64_t BT = B * TS;
  float* seq = c.at<float>(c.L.seq);
  e = BT * n->F;
  const abd_smalllstm_args none{};
  const abd_smalllstm_args& d = a ? *a : none;
  dropout_fwd_kernel<<<blocks(e), kT, 0, c.s>>>(c.at<float>(c.L.p[2]), seq, e, TS, n->Wf, train, d.mask_in,
                                                c.at<uint8_t>(c.L.keep), d.mask_out, d.seed, d.counter, d.row_offset);
  ABD_LAUNCH_CHECK();
  const float* in = seq;
  int width = n->F;
  for (int l = 0; l < kLayers; ++l) {
    // x W_ih^T + b_ih + b_hh over all B*T rows
    GemmArgs g = gemm_nt(in, width, c.p(P_WIH0 + 4 * l), c.at<float>(c.L.gates[l]), (int)BT, kGates, width);
    g.bias1 = c.p(P_BIH0 + 4 * l);
    g.bias2 = c.p(P_BHH0 + 4 * l);
    if (int rc = launch_gemm(c.s, g)) return rc;
    const RecArgs r = rec_args(c, l);
    lstm_rec_fwd_kernel<<<(unsigned)((B + kRecRows - 1) / kRecRows), kRT, 0, c.s>>>(r);
    ABD_LAUNCH_CHECK();
    in = r.h;
    width = kHid;
  }
  // fc2 on the top layer's last step, then log_softmax
  float* zfc = c.at<float>(c.L.zfc);
  GemmArgs f = gemm_nt(c.at<float>(c.L.h[kLayers - 1]) + (int64_t)(TS - 1) * kHid, (int64_t)TS * kHid, c.p(P_F2W), zfc,
                       (int)B, n->K, kHid);
  f.bias1 = c.p(P_F2B);
  if (int rc = launch_gemm(c.s, f)) return rc;
  lsm_fwd_kernel<<<(unsigned)B, 64, 0, c.s>>>(zfc, c.at<float>(c.L.logits), n->K);
  ABD_LAUNCH_CHECK();
  return ABD_OK;
}

// dlogp: the gradient of the log-probabilities the forward returned
int run_backward(const Ctx& c, const float* x, const float* dlogp) {
  const abd_smalllstm* n = c.n;
  const int64_t B = c.B;
  const int TS = n->TS, K = n->K;
  const int64_t BT = B * TS;
  float *dzfc = c.at<float>(c.L.dzfc), *dhtop = c.at<float>(c.L.dhtop), *dy = c.at<float>(c.L.dy);
  float *G0 = c.gb(0), *G1 = c.gb(1);
  // fc1 is not in the graph: its gradient is exactly zero
  ABD_HIP(hipMemsetAsync(c.g(P_F1W), 0, sizeof(float) * (n->off[P_F2W] - n->off[P_F1W]), c.s));
  lsm_bwd_kernel<<<(unsigned)B, 64, 0, c.s>>>(c.at<float>(c.L.logits), dlogp, dzfc, K);
  ABD_LAUNCH_CHECK();
  const float* hlast = c.at<float>(c.L.h[kLayers - 1]) + (int64_t)(TS - 1) * kHid;
  if (int rc = launch_gemm(c.s, gemm_tn(dzfc, hlast, (int64_t)TS * kHid, c.g(P_F2W), K, kHid, B))) return rc;
  if (int rc = colsum(c, dzfc, B, K, K, c.g(P_F2B))) return rc;
  if (int rc = launch_gemm(c.s, gemm_nn(dzfc, K, c.p(P_F2W), dhtop, (int)B, kHid, K))) return rc;
  for (int l = kLayers - 1; l >= 0; --l) {
    const bool top = l == kLayers - 1;
    RecArgs r = rec_args(c, l);
    r.dy = top ? nullptr : dy;
    r.dlast = top ? dhtop : nullptr;
    lstm_rec_bwd_kernel<<<(unsigned)((B + kRecRows - 1) / kRecRows), kRT, 0, c.s>>>(r);
    ABD_LAUNCH_CHECK();
    const float* in = l ? c.at<float>(c.L.h[l - 1]) : c.at<float>(c.L.seq);
    const int width = l ? kHid : n->F;
    const int base = P_WIH0 + 4 * l;
    if (int rc = weight_grad(c, TS, r.gates, in, width, 0, c.g(base))) return rc;
    if (TS > 1) {
      if (int rc = weight_grad(c, TS, r.gates, r.h, kHid, -1, c.g(base + 1))) return rc;
    } else {
      ABD_HIP(hipMemsetAsync(c.g(base + 1), 0, sizeof(float) * kGates * kHid, c.s));
    }
    if (int rc = colsum(c, r.gates, BT, kGates, kGates, c.g(base + 2))) return rc;
    ABD_HIP(hipMemcpyAsync(c.g(base + 3), c.g(base + 2), sizeof(float) * kGates, hipMemcpyDeviceToDevice, c.s));
    // the gradient of this layer's input: dG W_ih
    float* din = l ? dy : G0;
    if (int rc = launch_gemm(c.s, gemm_nn(r.gates, kGates, c.p(base), din, (int)BT, width, kGates))) return rc;
  }
  // trunk: G0 holds d(seq)
  int64_t e = BT * n->F;
  dropout_bwd_kernel<<<blocks(e), kT, 0, c.s>>>(G0, c.at<uint8_t>(c.L.keep), e, TS, n->Wf);
  ABD_LAUNCH_CHECK();
  // dz3 may overwrite d(p3): pool_bwd has consumed it into G1 by the time bn_bwd_apply writes
  if (int rc = bn_pool_bwd(c, 2, G0, G1, G0)) return rc;       // G0 = dz3
  if (int rc = conv_wgrad(c, 2, G0)) return rc;
  if (int rc = conv_dgrad(c, 2, G0, G1)) return rc;             // G1 = d(p2)
  if (int rc = bn_pool_bwd(c, 1, G1, G0, G1)) return rc;       // G1 = dz2
  if (int rc = conv_wgrad(c, 1, G1)) return rc;
  if (int rc = conv_dgrad(c, 1, G1, G0)) return rc;             // G0 = d(p1)
  if (int rc = bn_pool_bwd(c, 0, G0, G1, G0)) return rc;       // G0 = dz1
  const int64_t pixels = B * n->H1 * n->W1;
  const int nb = (int)std::min<int64_t>(kW1Blocks, (pixels + 63) / 64);
  const int64_t chunk = (pixels + nb - 1) / nb;
  float* part = c.at<float>(c.L.w1part);
  conv1_wgrad_kernel<<<nb, kT, 0, c.s>>>(x, G0, part, pixels, chunk, n->H, n->W);
  ABD_LAUNCH_CHECK();
  colsum_kernel<<<dim3(blocks(kC1 * 4), 1), kRedT, 0, c.s>>>(part, nb, kC1 * 4, kC1 * 4, nb, c.g(P_C1W), 0, 0);
  ABD_LAUNCH_CHECK();
  return ABD_OK;
}

int make_ctx(const abd_smalllstm* net, int64_t B, const float* params, float* grads, void* ws, size_t bytes,
             abd_stream_t stream, Ctx* c) {
  return make_ctx(net, B, params, grads, ws, bytes, stream, kC1, make_layout, c);
}

}  // namespace

extern "C" {

int abd_smalllstm_tile_info(int what) {
  switch (what) {
    case 0: return kBM;
    case 1: return kCK;
    case 2: return kSliceRows;
    case 3: return kMaxSlices;
    case 4: return kStatRows;
    case 5: return kStatBlocks;
    case 6: return kRecRows;
    case 7: return kSmallTile;
    case 8: return kLargeTile;
    case 9: return kBK;
    case 10: return kGemmSlices;
    case 11: return kColsumRows;
    case 12: return kLargeMinBlocks;
    default: return -1;
  }
}

int64_t abd_smalllstm_rnn_features(int H, int W) {
  if (H < 6 || W < 10) return -1;
  const int Wp1 = (W - 1) / 3, W2 = Wp1 - 1, Wp2 = W2 / 2 + 1, W3 = Wp2 - 1;
  return (int64_t)kC3 * (W3 / 2 + 1);
}

int abd_smalllstm_create(int H, int W, int num_classes, abd_smalllstm** net) {
  ABD_CHECK(net != nullptr, ABD_E_INVALID, "NULL out pointer");
  ABD_CHECK(H >= 6 && W >= 10, ABD_E_UNSUPPORTED,
            "smalllstm: input %d x %d leaves conv3 or pool3 no window (6 x 10 is the smallest)", H, W);
  ABD_CHECK(H <= kMaxDim && W <= kMaxDim, ABD_E_UNSUPPORTED, "smalllstm: input %d x %d beyond %d per side", H, W,
            kMaxDim);
  ABD_CHECK(num_classes >= 1 && num_classes <= 4096, ABD_E_UNSUPPORTED, "num_classes must be in [1, 4096]");
  ABD_CHECK((int64_t)H * W * kC1 < (1LL << 31), ABD_E_UNSUPPORTED,
            "smalllstm: input %d x %d takes the kernels' indices past 32 bits", H, W);
  auto* n = new abd_smalllstm();
  n->H = H, n->W = W, n->K = num_classes;
  n->H1 = H - 1, n->W1 = W - 1, n->Wp1 = n->W1 / 3;
  n->H2 = n->H1 - 1, n->W2 = n->Wp1 - 1;
  n->Hp2 = n->H2 / 2 + 1, n->Wp2 = n->W2 / 2 + 1;
  n->H3 = n->Hp2 - 1, n->W3 = n->Wp2 - 1;
  n->TS = (n->H3 - 2) / 2 + 1, n->Wf = n->W3 / 2 + 1;
  n->F = kC3 * n->Wf;
  n->T = n->H1 * n->W1;
  const int64_t sz[P_COUNT] = {kC1 * 4, kC1, kC1, kC1, (int64_t)kC2 * kC1 * 4, kC2, kC2, kC2, (int64_t)kC3 * kC2 * 4, kC3,
                               kC3, kC3, (int64_t)kGates * n->F, (int64_t)kGates * kHid, kGates, kGates,
                               (int64_t)kGates * kHid, (int64_t)kGates * kHid, kGates, kGates, (int64_t)kHid * kFc1In,
                               kHid, (int64_t)num_classes * kHid, num_classes};
  n->off[0] = 0;
  for (int i = 0; i < P_COUNT; ++i) n->off[i + 1] = n->off[i] + sz[i];
  n->roff[0] = 0, n->roff[1] = 2 * kC1, n->roff[2] = n->roff[1] + 2 * kC2, n->roff[3] = n->roff[2] + 2 * kC3;
  *net = n;
  return ABD_OK;
}

void abd_smalllstm_destroy(abd_smalllstm* net) { delete net; }

int64_t abd_smalllstm_param_count(const abd_smalllstm* net) { return net ? net->off[P_COUNT] : 0; }

int abd_smalllstm_param_offsets(const abd_smalllstm* net, int64_t* offsets) {
  ABD_CHECK(net && offsets, ABD_E_INVALID, "NULL argument");
  for (int i = 0; i <= P_COUNT; ++i) offsets[i] = net->off[i];
  return ABD_OK;
}

int64_t abd_smalllstm_running_count(const abd_smalllstm* net) { return net ? net->roff[3] : 0; }

int abd_smalllstm_running_offsets(const abd_smalllstm* net, int64_t* offsets) {
  ABD_CHECK(net && offsets, ABD_E_INVALID, "NULL argument");
  for (int i = 0; i <= 3; ++i) offsets[i] = net->roff[i];
  return ABD_OK;
}

size_t abd_smalllstm_workspace_bytes(const abd_smalllstm* net, int64_t batch) {
  if (!net || batch < 1) return 0;
  return make_layout(net, batch).total;
}

int64_t abd_smalllstm_workspace_offset(const abd_smalllstm* net, int64_t batch, const char* name) {
  if (!net || !name || batch < 1) return -1;
  const Layout L = make_layout(net, batch);
  const NamedOffset tab[] = {
      {"z1", L.z[0]}, {"z2", L.z[1]}, {"z3", L.z[2]}, {"a1", L.a[0]}, {"a2", L.a[1]}, {"a3", L.a[2]},
      {"p1", L.p[0]}, {"p2", L.p[1]}, {"p3", L.p[2]}, {"s1", L.stat[0]}, {"s2", L.stat[1]}, {"s3", L.stat[2]},
      {"seq", L.seq}, {"keep", L.keep}, {"h0", L.h[0]}, {"c0", L.c[0]}, {"g0", L.gates[0]}, {"h1", L.h[1]},
      {"c1", L.c[1]}, {"g1", L.gates[1]}, {"logits", L.logits}, {"dlogits", L.dlogits}, {"rowinfo", L.rowinfo}};
  return find_offset(tab, name);
}

int abd_smalllstm_forward(abd_smalllstm* net, const abd_smalllstm_args* a, int train_mode, void* workspace,
                          size_t workspace_bytes, abd_stream_t stream) {
  return stat_net_forward<Ctx>(net, a, train_mode, workspace, workspace_bytes, stream);
}

int abd_smalllstm_backward(abd_smalllstm* net, const abd_smalllstm_args* a, const float* dlogits, void* workspace,
                           size_t workspace_bytes, abd_stream_t stream) {
  return stat_net_backward<Ctx>(net, a, dlogits, workspace, workspace_bytes, stream);
}

int abd_smalllstm_train_step(abd_smalllstm* net, const abd_smalllstm_args* a, void* workspace, size_t workspace_bytes,
                             abd_stream_t stream) {
  return stat_net_train_step<Ctx>(net, a, workspace, workspace_bytes, stream);
}

int abd_smalllstm_eval(abd_smalllstm* net, const float* x, int64_t batch, const float* params, const float* running,
                       const int64_t* labels, const int64_t* indicators, float* logits, int64_t* metrics,
                       void* workspace, size_t workspace_bytes, abd_stream_t stream) {
  return stat_net_eval<Ctx>(net, x, batch, params, running, labels, indicators, logits, metrics, workspace,
                            workspace_bytes, stream);
}

}  // extern "C"
