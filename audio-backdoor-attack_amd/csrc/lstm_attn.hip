// lstmwithattention (reference utils/models.py:180-228) on gfx950: (5,1) convs + BatchNorm, two
// bidirectional LSTM layers, the attention head, the dense classifier, cross entropy, BPTT.
//
// Recurrent kernels (lstm_fwd_kernel / lstm_bwd_kernel): ONE launch per layer and pass covers both
// directions and all T steps.  A workgroup owns one direction and kTile batch rows for the whole
// sequence; W_hh of its direction (256 x 64 fp32 = 64 KiB) stays in LDS -- more than a 64 KiB CU
// could hold next to anything else, gfx950's 160 KiB takes it -- with the tile's h (forward) or
// dgates (backward); c, dc and dh stay in registers.  Rows do not couple, so nothing waits on another
// workgroup and no float atomics are used.  The input projections x_t W_ih^T + b_ih + b_hh of all
// B*T rows are one GEMM in front of the time loop; dW_hh, dW_ih, dx are GEMMs behind it.
//
// GEMMs: gemm_kernel, v_mfma_f32_32x32x2_f32 (fp32 operands and accumulation), strides select the
// NN / NT / TN forms; a long reduction dimension is split into slices whose partial products are
// summed by colsum_kernel in slice order, so two runs are bit-equal.
#include <algorithm>
#include <atomic>
#include <cmath>

#include "abd_common.h"

struct abd_lstmattn {
  int T, F, K;
  int64_t off[35];
};

namespace {

constexpr int kT = 256;
constexpr int kHid = 64;     // LSTM hidden size
constexpr int kGates = 256;  // 4 * kHid gate rows, torch order i f g o
constexpr int kTile = 8;     // batch rows of one recurrent workgroup
constexpr int kRpw = kTile / 4;  // rows per wave (4 waves: lane = hidden unit)
constexpr int kWtLd = 257;   // padded row of the transposed W_hh in LDS
constexpr int kC1 = 10;      // conv1 channels
constexpr int kMaxSlabs = 128;
constexpr int kQ = 8;        // doubles per (channel, slab) partial
constexpr float kBnEps = 1e-5f;
constexpr float kBnMomentum = 0.1f;

enum {
  P_C1W, P_C1B, P_BN1W, P_BN1B, P_C2W, P_C2B, P_BN2W, P_BN2B,
  P_R1 = 8,   // w_ih, w_hh, b_ih, b_hh, then the four _reverse ones
  P_R2 = 16,
  P_D1W = 24, P_D1B, P_ATW, P_ATB, P_D2W, P_D2B, P_D3W, P_D3B, P_OW, P_OB, P_COUNT
};

// the 35 parameter offsets, passed to the kernels by value
struct Offs {
  int64_t v[35];
  __host__ __device__ int64_t operator[](int i) const { return v[i]; }
};

// shared with rnn.hip and smalllstm.hip: backward cell, colsum; GemmArgs and its three forms, keep_hash, the host
// helpers; colsum_kernel, ce_kernel, metrics_kernel
#include "lstm_common.inc"

// ------------------------------------------------------------------ fp32 MFMA GEMM (GemmArgs)
// One wave per 32x32 tile.
__global__ void __launch_bounds__(64) gemm_kernel(GemmArgs a) {
  const int lane = threadIdx.x;
  const int m = blockIdx.x * 32 + (lane & 31);
  const int n = blockIdx.y * 32 + (lane & 31);
  const int kh = lane >> 5;
  const int k0 = blockIdx.z * a.kchunk;
  const int k1 = min(a.K, k0 + a.kchunk);
  const bool mok = m < a.M, nok = n < a.N;
  const float* ap = a.A + (int64_t)(mok ? m : 0) * a.sam;
  const float* bp = a.B + (int64_t)(nok ? n : 0) * a.sbn;
  typedef float f16v __attribute__((ext_vector_type(16)));
  f16v acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.0f;
  for (int kb = k0; kb < k1; kb += 8) {
    float av[4], bv[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int k = kb + 2 * i + kh;
      av[i] = 0.0f;
      bv[i] = 0.0f;
      if (k < k1) {
        if (mok) av[i] = ap[(int64_t)k * a.sak];
        if (nok) {
          if (a.shift == 0) {
            bv[i] = bp[(int64_t)k * a.sbk];
          } else {
            const int ts = k % a.T + a.shift;
            if (ts >= 0 && ts < a.T) bv[i] = bp[(int64_t)(k + a.shift) * a.sbk];
          }
        }
      }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av[i], bv[i], acc, 0, 0, 0);
  }
  float* C = a.C + (int64_t)blockIdx.z * a.cz;
  if (nok) {
    float bias = 0.0f;
    if (a.bias1) bias += a.bias1[n];
    if (a.bias2) bias += a.bias2[n];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int mr = blockIdx.x * 32 + (r & 3) + 8 * (r >> 2) + 4 * kh;
      if (mr < a.M) {
        float* c = C + (int64_t)mr * a.ldc + n;
        const float v = acc[r] + bias;
        *c = a.accumulate ? *c + v : v;
      }
    }
  }
}

// ------------------------------------------------------------------ recurrent kernels
struct LstmArgs {
  const float* xp;     // forward: [2][B*T][256] input projections (+ both biases)
  const float* whh[2];
  float* y;            // forward: [B][T][128] h_t, forward half | reverse half
  float* gates;        // [2][B*T][256] activated i f g o
  float* c;            // [2][B*T][64]
  const float* dy;     // backward: [B][T][128]
  float* dg;           // backward: [2][B*T][256] pre-activation gate gradients
  int B, T;
};

__global__ void __launch_bounds__(kT) lstm_fwd_kernel(LstmArgs a) {
  extern __shared__ __attribute__((aligned(16))) float lds_rec[];
  float* Wt = lds_rec;                    // [64 k][kWtLd]: Wt[k][j] = W_hh[j][k]
  float* hs = lds_rec + kHid * kWtLd;     // [kTile][64]
  const int tid = threadIdx.x, u = tid & 63, w = tid >> 6;
  const int dir = blockIdx.y;
  const int b0 = blockIdx.x * kTile + w * kRpw;
  const float* whh = dir ? a.whh[1] : a.whh[0];
  for (int i = tid; i < kGates * kHid; i += kT) Wt[(i & 63) * kWtLd + (i >> 6)] = whh[i];
  for (int i = tid; i < kTile * kHid; i += kT) hs[i] = 0.0f;
  __syncthreads();
  const int64_t BT = (int64_t)a.B * a.T;
  float c[kRpw];
#pragma unroll
  for (int r = 0; r < kRpw; ++r) c[r] = 0.0f;
  for (int step = 0; step < a.T; ++step) {
    const int t = dir ? a.T - 1 - step : step;
    float acc[kRpw][4];
#pragma unroll
    for (int r = 0; r < kRpw; ++r) {
      const int b = b0 + r;
      const float* xp = a.xp + ((int64_t)dir * BT + (int64_t)(b < a.B ? b : 0) * a.T + t) * kGates + u;
#pragma unroll
      for (int g = 0; g < 4; ++g) acc[r][g] = b < a.B ? xp[g * kHid] : 0.0f;
    }
    for (int k = 0; k < kHid; k += 4) {
      float4 hv[kRpw];
#pragma unroll
      for (int r = 0; r < kRpw; ++r) hv[r] = *reinterpret_cast<const float4*>(hs + (w * kRpw + r) * kHid + k);
#pragma unroll
      for (int kk = 0; kk < 4; ++kk) {
        const float* wr = Wt + (k + kk) * kWtLd + u;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const float wv = wr[g * kHid];
#pragma unroll
          for (int r = 0; r < kRpw; ++r) {
            const float h = kk == 0 ? hv[r].x : kk == 1 ? hv[r].y : kk == 2 ? hv[r].z : hv[r].w;
            acc[r][g] = fmaf(wv, h, acc[r][g]);
          }
        }
      }
    }
    float hn[kRpw];
#pragma unroll
    for (int r = 0; r < kRpw; ++r) {
      const int b = b0 + r;
      const float ig = sigmoid_acc(acc[r][0]), fg = sigmoid_acc(acc[r][1]);
      const float gg = tanhf(acc[r][2]), og = sigmoid_acc(acc[r][3]);
      c[r] = fg * c[r] + ig * gg;
      hn[r] = og * tanhf(c[r]);
      if (b < a.B) {
        const int64_t row = (int64_t)b * a.T + t;
        float* gp = a.gates + ((int64_t)dir * BT + row) * kGates + u;
        gp[0] = ig;
        gp[kHid] = fg;
        gp[2 * kHid] = gg;
        gp[3 * kHid] = og;
        a.c[((int64_t)dir * BT + row) * kHid + u] = c[r];
        a.y[row * (2 * kHid) + dir * kHid + u] = hn[r];
      }
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < kRpw; ++r) hs[(w * kRpw + r) * kHid + u] = hn[r];
    __syncthreads();
  }
}

__global__ void __launch_bounds__(kT) lstm_bwd_kernel(LstmArgs a) {
  extern __shared__ __attribute__((aligned(16))) float lds_rec[];
  float* Ws = lds_rec;                    // [256 j][64 k] as stored
  float* dgs = lds_rec + kGates * kHid;   // [kTile][256]
  const int tid = threadIdx.x, u = tid & 63, w = tid >> 6;
  const int dir = blockIdx.y;
  const int b0 = blockIdx.x * kTile + w * kRpw;
  const float* whh = dir ? a.whh[1] : a.whh[0];
  for (int i = tid; i < kGates * kHid; i += kT) Ws[i] = whh[i];
  __syncthreads();
  const int64_t BT = (int64_t)a.B * a.T;
  float dh[kRpw], dc[kRpw];
#pragma unroll
  for (int r = 0; r < kRpw; ++r) dh[r] = dc[r] = 0.0f;
  for (int step = 0; step < a.T; ++step) {
    const int t = dir ? step : a.T - 1 - step;   // the forward pass's order, reversed
    const int tp = dir ? t + 1 : t - 1;          // the step that fed this one
#pragma unroll
    for (int r = 0; r < kRpw; ++r) {
      const int b = b0 + r;
      float di = 0.0f, df = 0.0f, dgg = 0.0f, dob = 0.0f;
      if (b < a.B) {
        const int64_t row = (int64_t)b * a.T + t;
        const float* gp = a.gates + ((int64_t)dir * BT + row) * kGates + u;
        const float ig = gp[0], fg = gp[kHid], gg = gp[2 * kHid], og = gp[3 * kHid];
        const float ct = a.c[((int64_t)dir * BT + row) * kHid + u];
        const float cp = (tp >= 0 && tp < a.T) ? a.c[((int64_t)dir * BT + (int64_t)b * a.T + tp) * kHid + u] : 0.0f;
        const float dht = a.dy[row * (2 * kHid) + dir * kHid + u] + dh[r];
        lstm_cell_bwd(ig, fg, gg, og, ct, cp, dht, dc[r], di, df, dgg, dob, dc[r]);
        float* dp = a.dg + ((int64_t)dir * BT + row) * kGates + u;
        dp[0] = di;
        dp[kHid] = df;
        dp[2 * kHid] = dgg;
        dp[3 * kHid] = dob;
      }
      float* ds = dgs + (w * kRpw + r) * kGates + u;
      ds[0] = di;
      ds[kHid] = df;
      ds[2 * kHid] = dgg;
      ds[3 * kHid] = dob;
    }
    __syncthreads();
    float acc[kRpw];
#pragma unroll
    for (int r = 0; r < kRpw; ++r) acc[r] = 0.0f;
    for (int j = 0; j < kGates; j += 4) {
      float4 dv[kRpw];
#pragma unroll
      for (int r = 0; r < kRpw; ++r) dv[r] = *reinterpret_cast<const float4*>(dgs + (w * kRpw + r) * kGates + j);
#pragma unroll
      for (int jj = 0; jj < 4; ++jj) {
        const float wv = Ws[(j + jj) * kHid + u];
#pragma unroll
        for (int r = 0; r < kRpw; ++r) {
          const float d = jj == 0 ? dv[r].x : jj == 1 ? dv[r].y : jj == 2 ? dv[r].z : dv[r].w;
          acc[r] = fmaf(d, wv, acc[r]);
        }
      }
    }
#pragma unroll
    for (int r = 0; r < kRpw; ++r) dh[r] = acc[r];
    __syncthreads();
  }
}

// ------------------------------------------------------------------ convs + BatchNorm
struct ConvArgs {
  const float* x;      // (B, T, F)
  float* a1;           // (B, 10, T, F) relu(conv1)
  float* a2;           // (B, T, F) relu(conv2)
  float* x0;           // (B, T, F) batchnorm2 output
  const float* params;
  Offs off;
  float* coef;         // [0..19] bn1 (mean, invstd) per channel, [20..21] bn2, [24..43] bn1 backward
                       // (mean dy, mean dy*xhat), [44..45] bn2 backward
  double* part;        // [C][S][kQ]
  float* grads;
  const float* dx0;    // (B, T, F) gradient of the batchnorm2 output
  float* dz2;          // (B, T, F) gradient of conv2's pre-activation
  float* running;
  int64_t* nbt;
  int64_t N;           // B*T*F
  int T, F, S, train;
};

template <int Q>
__device__ __forceinline__ void block_reduce_store(double (&v)[Q], double* out) {
  __shared__ double red[4][Q];
#pragma unroll
  for (int q = 0; q < Q; ++q) v[q] = abd::wave_sum_d(v[q]);
  if ((threadIdx.x & 63) == 0)
    for (int q = 0; q < Q; ++q) red[threadIdx.x >> 6][q] = v[q];
  __syncthreads();
  if (threadIdx.x < Q) out[threadIdx.x] = red[0][threadIdx.x] + red[1][threadIdx.x] + red[2][threadIdx.x] + red[3][threadIdx.x];
}

__global__ void __launch_bounds__(kT) conv1_kernel(ConvArgs a) {
  const int64_t e = (int64_t)blockIdx.x * kT + threadIdx.x;
  if (e >= a.N) return;
  const int TF = a.T * a.F;
  const int64_t b = e / TF;
  const int r = (int)(e - b * TF), t = r / a.F;
  const float* w = a.params + a.off[P_C1W];
  const float* bias = a.params + a.off[P_C1B];
  float xv[5];
#pragma unroll
  for (int d = 0; d < 5; ++d) {
    const int tt = t + d - 2;
    xv[d] = (tt >= 0 && tt < a.T) ? a.x[e + (int64_t)(d - 2) * a.F] : 0.0f;
  }
  for (int c = 0; c < kC1; ++c) {
    float v = bias[c];
#pragma unroll
    for (int d = 0; d < 5; ++d) v = fmaf(w[c * 5 + d], xv[d], v);
    a.a1[(b * kC1 + c) * TF + r] = fmaxf(v, 0.0f);
  }
}

// MODE 0: sums of v, v^2 of src channel blockIdx.y ((B, C, T*F) layout, C = gridDim.y)
// MODE 1: batchnorm2 backward sums of dy, dy * xhat
template <int MODE>
__global__ void __launch_bounds__(kT) bn_stats_kernel(ConvArgs a, const float* src) {
  const int c = blockIdx.y, C = gridDim.y, TF = a.T * a.F;
  const int64_t chunk = (a.N + a.S - 1) / a.S;
  const int64_t e0 = (int64_t)blockIdx.x * chunk, e1 = min(a.N, e0 + chunk);
  double v[2] = {0.0, 0.0};
  const float mean = MODE ? a.coef[20] : 0.0f, invstd = MODE ? a.coef[21] : 0.0f;
  for (int64_t e = e0 + threadIdx.x; e < e1; e += kT) {
    if (MODE == 0) {
      const int64_t b = e / TF;
      const double x = src[(b * C + c) * TF + (e - b * TF)];
      v[0] += x;
      v[1] += x * x;
    } else {
      const float dy = a.dx0[e], xh = (a.a2[e] - mean) * invstd;
      v[0] += dy;
      v[1] += (double)dy * xh;
    }
  }
  block_reduce_store<2>(v, a.part + ((int64_t)c * a.S + blockIdx.x) * kQ);
}

// one thread per channel: statistics -> (mean, invstd), running update
__global__ void bn_finalize_kernel(ConvArgs a, int C, int coef0, int run0, int nbt_idx) {
  const int c = threadIdx.x;
  if (c >= C) return;
  float* rm = a.running + run0;
  float* rv = rm + C;
  if (!a.train) {
    a.coef[coef0 + 2 * c] = rm[c];
    a.coef[coef0 + 2 * c + 1] = 1.0f / sqrtf(rv[c] + kBnEps);
    return;
  }
  double s = 0.0, s2 = 0.0;
  for (int i = 0; i < a.S; ++i) {
    s += a.part[((int64_t)c * a.S + i) * kQ];
    s2 += a.part[((int64_t)c * a.S + i) * kQ + 1];
  }
  const double n = (double)a.N;
  const double mean = s / n;
  double var = s2 / n - mean * mean;
  if (var < 0.0) var = 0.0;
  a.coef[coef0 + 2 * c] = (float)mean;
  a.coef[coef0 + 2 * c + 1] = (float)(1.0 / sqrt(var + (double)kBnEps));
  rm[c] = (1.0f - kBnMomentum) * rm[c] + kBnMomentum * (float)mean;
  rv[c] = (1.0f - kBnMomentum) * rv[c] + kBnMomentum * (float)(var * n / (n - 1.0));
  if (c == 0 && a.nbt) a.nbt[nbt_idx] += 1;
}

__global__ void __launch_bounds__(kT) conv2_kernel(ConvArgs a) {
  const int64_t e = (int64_t)blockIdx.x * kT + threadIdx.x;
  if (e >= a.N) return;
  const int TF = a.T * a.F;
  const int64_t b = e / TF;
  const int r = (int)(e - b * TF), t = r / a.F;
  const float* w = a.params + a.off[P_C2W];
  const float* g1 = a.params + a.off[P_BN1W];
  const float* be1 = a.params + a.off[P_BN1B];
  float v = a.params[a.off[P_C2B]];
  for (int c = 0; c < kC1; ++c) {
    const float sc = a.coef[2 * c + 1] * g1[c], sh = be1[c] - a.coef[2 * c] * sc;
    const float* p = a.a1 + (b * kC1 + c) * TF + r;
#pragma unroll
    for (int d = 0; d < 5; ++d) {
      const int tt = t + d - 2;
      if (tt >= 0 && tt < a.T) v = fmaf(w[c * 5 + d], fmaf(p[(d - 2) * a.F], sc, sh), v);
    }
  }
  a.a2[e] = fmaxf(v, 0.0f);
}

__global__ void __launch_bounds__(kT) bn2_apply_kernel(ConvArgs a) {
  const int64_t e = (int64_t)blockIdx.x * kT + threadIdx.x;
  if (e >= a.N) return;
  const float sc = a.coef[21] * a.params[a.off[P_BN2W]];
  a.x0[e] = fmaf(a.a2[e] - a.coef[20], sc, a.params[a.off[P_BN2B]]);
}

// batchnorm2 backward sums -> its weight / bias gradients and the input-gradient coefficients
__global__ void bn2_bwd_finalize_kernel(ConvArgs a) {
  if (threadIdx.x != 0) return;
  double s = 0.0, sx = 0.0;
  for (int i = 0; i < a.S; ++i) {
    s += a.part[(int64_t)i * kQ];
    sx += a.part[(int64_t)i * kQ + 1];
  }
  a.grads[a.off[P_BN2W]] = (float)sx;
  a.grads[a.off[P_BN2B]] = (float)s;
  a.coef[44] = (float)(s / (double)a.N);
  a.coef[45] = (float)(sx / (double)a.N);
}

__global__ void __launch_bounds__(kT) dz2_kernel(ConvArgs a) {
  const int64_t e = (int64_t)blockIdx.x * kT + threadIdx.x;
  if (e >= a.N) return;
  const float v = a.a2[e];
  const float invstd = a.coef[21], xh = (v - a.coef[20]) * invstd;
  const float d = a.params[a.off[P_BN2W]] * invstd * (a.dx0[e] - a.coef[44] - xh * a.coef[45]);
  a.dz2[e] = v > 0.0f ? d : 0.0f;
}

// channel blockIdx.y, element slab blockIdx.x.  PASS 0: conv2's weight gradient, batchnorm1's backward
// sums, conv2's bias gradient.  PASS 1: conv1's weight and bias gradients (batchnorm1's input
// gradient is formed on the fly and never stored).
template <int PASS>
__global__ void __launch_bounds__(kT) conv_bwd_kernel(ConvArgs a) {
  const int c = blockIdx.y, TF = a.T * a.F;
  const int64_t chunk = (a.N + a.S - 1) / a.S;
  const int64_t e0 = (int64_t)blockIdx.x * chunk, e1 = min(a.N, e0 + chunk);
  const float* w2 = a.params + a.off[P_C2W] + c * 5;
  const float g1 = a.params[a.off[P_BN1W] + c], be1 = a.params[a.off[P_BN1B] + c];
  const float mean = a.coef[2 * c], invstd = a.coef[2 * c + 1];
  const float m1 = a.coef[24 + 2 * c], m2 = a.coef[24 + 2 * c + 1];
  double v[kQ];
#pragma unroll
  for (int q = 0; q < kQ; ++q) v[q] = 0.0;
  for (int64_t e = e0 + threadIdx.x; e < e1; e += kT) {
    const int64_t b = e / TF;
    const int r = (int)(e - b * TF), t = r / a.F;
    const float av = a.a1[(b * kC1 + c) * TF + r];
    const float xh = (av - mean) * invstd;
    // bn1out[b,c,t,f] feeds conv2's outputs t - d + 2 through tap d
    float dz[5], g = 0.0f;
#pragma unroll
    for (int d = 0; d < 5; ++d) {
      const int to = t - d + 2;
      dz[d] = (to >= 0 && to < a.T) ? a.dz2[e + (int64_t)(2 - d) * a.F] : 0.0f;
      g = fmaf(w2[d], dz[d], g);
    }
    if (PASS == 0) {
      const float bo = fmaf(xh, g1, be1);
#pragma unroll
      for (int d = 0; d < 5; ++d) v[d] += (double)(bo * dz[d]);
      v[5] += g;
      v[6] += (double)(g * xh);
      v[7] += a.dz2[e];
    } else {
      const float da = av > 0.0f ? g1 * invstd * (g - m1 - xh * m2) : 0.0f;
#pragma unroll
      for (int d = 0; d < 5; ++d) {
        const int tt = t + d - 2;
        if (tt >= 0 && tt < a.T) v[d] += (double)(da * a.x[e + (int64_t)(d - 2) * a.F]);
      }
      v[5] += da;
    }
  }
  block_reduce_store<kQ>(v, a.part + ((int64_t)c * a.S + blockIdx.x) * kQ);
}

template <int PASS>
__global__ void conv_bwd_finalize_kernel(ConvArgs a) {
  const int c = threadIdx.x;
  if (c >= kC1) return;
  double v[kQ];
  for (int q = 0; q < kQ; ++q) v[q] = 0.0;
  for (int i = 0; i < a.S; ++i)
    for (int q = 0; q < kQ; ++q) v[q] += a.part[((int64_t)c * a.S + i) * kQ + q];
  if (PASS == 0) {
    for (int d = 0; d < 5; ++d) a.grads[a.off[P_C2W] + c * 5 + d] = (float)v[d];
    a.grads[a.off[P_BN1B] + c] = (float)v[5];
    a.grads[a.off[P_BN1W] + c] = (float)v[6];
    if (c == 0) a.grads[a.off[P_C2B]] = (float)v[7];
    a.coef[24 + 2 * c] = (float)(v[5] / (double)a.N);
    a.coef[24 + 2 * c + 1] = (float)(v[6] / (double)a.N);
  } else {
    for (int d = 0; d < 5; ++d) a.grads[a.off[P_C1W] + c * 5 + d] = (float)v[d];
    a.grads[a.off[P_C1B] + c] = (float)v[5];
  }
}

// ------------------------------------------------------------------ per-utterance front end
// conv1 -> BatchNorm1 -> conv2 -> BatchNorm2 of ONE utterance per workgroup, each BatchNorm over the
// utterance's own T*F values per channel (a batch-1 train-mode forward).  x sits in LDS; the ten a1 planes
// are recomputed from it where they are needed and never stored: 4*T*F bytes read and 4*T*F written per
// utterance.  A thread owns the elements e = tid, tid + 256, ...; tap d of either convolution reads
// e + (d - 2) * F, so every LDS access of a wave is unit-stride (no bank conflicts for any F).
// The arithmetic restates conv1_kernel / bn_finalize_kernel / conv2_kernel / bn2_apply_kernel term by
// term; only the reduction trees of the sums differ (fixed order here too).
constexpr int kPuMaxTF = ABD_LSTMATTN_PER_UTTERANCE_MAX_TF;

struct FrontArgs {
  const float* x;      // (B, T, F)
  float* x0;           // (B, T, F) batchnorm2 output
  const float* params;
  Offs off;
  int T, F;
};

__global__ void __launch_bounds__(kT) front_per_utterance_kernel(FrontArgs a) {
  extern __shared__ __attribute__((aligned(16))) float lds_front[];
  __shared__ double stat[2 * kC1];
  __shared__ float sc1[kC1], sh1[kC1], bn2[2];
  const int tid = threadIdx.x, T = a.T, F = a.F, TF = T * F;
  float* xs = lds_front;         // [T][F] the utterance
  float* a2s = lds_front + TF;   // [T][F] relu(conv2)
  const float* xg = a.x + (int64_t)blockIdx.x * TF;
  const float* w1 = a.params + a.off[P_C1W];
  const float* b1 = a.params + a.off[P_C1B];
  const float* w2 = a.params + a.off[P_C2W];
  for (int e = tid; e < TF; e += kT) xs[e] = xg[e];
  __syncthreads();
  // pass 1: per-channel sums of relu(conv1) and its square
  {
    double v[2 * kC1];
#pragma unroll
    for (int q = 0; q < 2 * kC1; ++q) v[q] = 0.0;
    for (int e = tid; e < TF; e += kT) {
      const int t = e / F;
      float xv[5];
#pragma unroll
      for (int d = 0; d < 5; ++d) {
        const int tt = t + d - 2;
        xv[d] = (tt >= 0 && tt < T) ? xs[e + (d - 2) * F] : 0.0f;
      }
#pragma unroll
      for (int c = 0; c < kC1; ++c) {
        float s = b1[c];
#pragma unroll
        for (int d = 0; d < 5; ++d) s = fmaf(w1[c * 5 + d], xv[d], s);
        const double r = fmaxf(s, 0.0f);
        v[2 * c] += r;
        v[2 * c + 1] += r * r;
      }
    }
    block_reduce_store<2 * kC1>(v, stat);
  }
  __syncthreads();
  if (tid < kC1) {
    const double n = (double)TF;
    const double mean = stat[2 * tid] / n;
    double var = stat[2 * tid + 1] / n - mean * mean;
    if (var < 0.0) var = 0.0;
    const float sc = (float)(1.0 / sqrt(var + (double)kBnEps)) * a.params[a.off[P_BN1W] + tid];
    sc1[tid] = sc;
    sh1[tid] = a.params[a.off[P_BN1B] + tid] - (float)mean * sc;
  }
  __syncthreads();
  // pass 2: relu(conv2) of the normalised planes; conv1 recomputed at the five rows an output needs
  {
    double v[2] = {0.0, 0.0};
    const float bias2 = a.params[a.off[P_C2B]];
    for (int e = tid; e < TF; e += kT) {
      const int t = e / F;
      float xr[9];   // rows t - 4 .. t + 4; zero outside the utterance (conv1's padding)
#pragma unroll
      for (int j = 0; j < 9; ++j) {
        const int tt = t + j - 4;
        xr[j] = (tt >= 0 && tt < T) ? xs[e + (j - 4) * F] : 0.0f;
      }
      float s2 = bias2;
      for (int c = 0; c < kC1; ++c) {
        const float bc = b1[c], sc = sc1[c], sh = sh1[c];
#pragma unroll
        for (int d = 0; d < 5; ++d) {
          const int tt = t + d - 2;
          // outside the utterance the normalised plane is conv2's zero padding, not bn1(conv1(0))
          if (tt < 0 || tt >= T) continue;
          float s = bc;
#pragma unroll
          for (int dd = 0; dd < 5; ++dd) s = fmaf(w1[c * 5 + dd], xr[d + dd], s);
          s2 = fmaf(w2[c * 5 + d], fmaf(fmaxf(s, 0.0f), sc, sh), s2);
        }
      }
      const float r = fmaxf(s2, 0.0f);
      a2s[e] = r;
      v[0] += (double)r;
      v[1] += (double)r * r;
    }
    block_reduce_store<2>(v, stat);
  }
  __syncthreads();
  if (tid == 0) {
    const double n = (double)TF;
    const double mean = stat[0] / n;
    double var = stat[1] / n - mean * mean;
    if (var < 0.0) var = 0.0;
    bn2[0] = (float)mean;
    bn2[1] = (float)(1.0 / sqrt(var + (double)kBnEps));
  }
  __syncthreads();
  // pass 3: batchnorm2
  {
    const float mean = bn2[0], sc = bn2[1] * a.params[a.off[P_BN2W]], sh = a.params[a.off[P_BN2B]];
    float* x0 = a.x0 + (int64_t)blockIdx.x * TF;
    for (int e = tid; e < TF; e += kT) x0[e] = fmaf(a2s[e] - mean, sc, sh);
  }
}

// ------------------------------------------------------------------ attention head + classifier
struct HeadArgs {
  const float* params;
  Offs off;
  const float* y;      // (B, T, 128) rnn2 output
  float* q;            // (B, 128) relu(dense1)
  float* att;          // (B, 128) softmax
  float* av;           // (B, T) att_vector
  float* d2;           // (B, 64) relu(dense2), before dropout
  float* d2m;          // (B, 64) after dropout
  float* d3;           // (B, 32)
  float* logits;       // (B, K)
  uint8_t* keep;       // (B, 64) mask used
  const uint8_t* mask_in;
  uint8_t* mask_out;
  uint64_t seed, counter;
  int64_t row_offset;
  // backward
  const float* dlogits;
  float* dz3;          // (B, 32)
  float* dz2;          // (B, 64)
  float* dsc;          // (B, 128)
  float* dzq;          // (B, 128)
  float* dy;           // (B, T, 128)
  int T, K, train;
};

__device__ __forceinline__ float block128_sum(float v, float* red) {
  v = abd::wave_sum(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return red[0] + red[1];
}

__device__ __forceinline__ float block128_max(float v, float* red) {
  v = abd::wave_max(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return fmaxf(red[0], red[1]);
}

__global__ void __launch_bounds__(128) head_fwd_kernel(HeadArgs a) {
  __shared__ float xl[128], q[128], att[128], av[1024], d2m[64], d3[32], red[2];
  const int b = blockIdx.x, tid = threadIdx.x, T = a.T;
  const float* P = a.params;
  const float* y = a.y + (int64_t)b * T * 128;
  xl[tid] = y[(int64_t)(T - 1) * 128 + tid];
  __syncthreads();
  {
    const float* w = P + a.off[P_D1W] + tid * 128;
    float s = P[a.off[P_D1B] + tid];
    for (int k = 0; k < 128; ++k) s = fmaf(w[k], xl[k], s);
    q[tid] = fmaxf(s, 0.0f);
    a.q[(int64_t)b * 128 + tid] = q[tid];
  }
  __syncthreads();
  float sc;
  {
    const float* w = P + a.off[P_ATW] + tid * 128;
    sc = P[a.off[P_ATB] + tid];
    for (int k = 0; k < 128; ++k) sc = fmaf(w[k], q[k], sc);
  }
  const float mx = block128_max(sc, red);
  const float ex = expf(sc - mx);
  const float den = block128_sum(ex, red);
  att[tid] = ex / den;
  a.att[(int64_t)b * 128 + tid] = att[tid];
  __syncthreads();
  {
    const int lane = tid & 63, wv = tid >> 6;
    for (int t = wv; t < T; t += 2) {
      const float* yr = y + (int64_t)t * 128;
      const float s = abd::wave_sum(fmaf(att[lane], yr[lane], att[lane + 64] * yr[lane + 64]));
      if (lane == 0) {
        av[t] = s;
        a.av[(int64_t)b * T + t] = s;
      }
    }
  }
  __syncthreads();
  if (tid < 64) {
    const float* w = P + a.off[P_D2W] + (int64_t)tid * T;
    float s = P[a.off[P_D2B] + tid];
    for (int t = 0; t < T; ++t) s = fmaf(w[t], av[t], s);
    s = fmaxf(s, 0.0f);
    const int64_t i = (int64_t)b * 64 + tid;
    a.d2[i] = s;
    uint8_t keep = 1;
    if (a.train) {
      keep = a.mask_in ? (a.mask_in[i] != 0)
                       : keep_hash(a.seed, a.counter, (uint64_t)(a.row_offset + b) * 64 + tid, 0.5f);
      s = keep ? s * 2.0f : 0.0f;
    }
    a.keep[i] = keep;
    if (a.mask_out) a.mask_out[i] = keep;
    d2m[tid] = s;
    a.d2m[i] = s;
  }
  __syncthreads();
  if (tid < 32) {
    const float* w = P + a.off[P_D3W] + tid * 64;
    float s = P[a.off[P_D3B] + tid];
    for (int k = 0; k < 64; ++k) s = fmaf(w[k], d2m[k], s);
    d3[tid] = fmaxf(s, 0.0f);
    a.d3[(int64_t)b * 32 + tid] = d3[tid];
  }
  __syncthreads();
  for (int j = tid; j < a.K; j += 128) {
    const float* w = P + a.off[P_OW] + j * 32;
    float s = P[a.off[P_OB] + j];
    for (int k = 0; k < 32; ++k) s = fmaf(w[k], d3[k], s);
    a.logits[(int64_t)b * a.K + j] = s;
  }
}

__global__ void __launch_bounds__(128) head_bwd_kernel(HeadArgs a) {
  __shared__ float dz3[32], dz2[64], dav[1024], dsc[128], dzq[128], red[2];
  const int b = blockIdx.x, tid = threadIdx.x, T = a.T, K = a.K;
  const float* P = a.params;
  const float* y = a.y + (int64_t)b * T * 128;
  float* dy = a.dy + (int64_t)b * T * 128;
  const float* dl = a.dlogits + (int64_t)b * K;
  if (tid < 32) {
    const float* w = P + a.off[P_OW] + tid;
    float s = 0.0f;
    for (int j = 0; j < K; ++j) s = fmaf(dl[j], w[j * 32], s);
    s = a.d3[(int64_t)b * 32 + tid] > 0.0f ? s : 0.0f;
    dz3[tid] = s;
    a.dz3[(int64_t)b * 32 + tid] = s;
  }
  __syncthreads();
  if (tid < 64) {
    const float* w = P + a.off[P_D3W] + tid;
    float s = 0.0f;
    for (int j = 0; j < 32; ++j) s = fmaf(dz3[j], w[j * 64], s);
    const int64_t i = (int64_t)b * 64 + tid;
    if (a.train) s = a.keep[i] ? s * 2.0f : 0.0f;
    s = a.d2[i] > 0.0f ? s : 0.0f;
    dz2[tid] = s;
    a.dz2[i] = s;
  }
  __syncthreads();
  for (int t = tid; t < T; t += 128) {
    const float* w = P + a.off[P_D2W] + t;
    float s = 0.0f;
    for (int j = 0; j < 64; ++j) s = fmaf(dz2[j], w[(int64_t)j * T], s);
    dav[t] = s;
  }
  __syncthreads();
  const float at = a.att[(int64_t)b * 128 + tid];
  float datt = 0.0f;
  for (int t = 0; t < T - 1; ++t) {
    const float d = dav[t];
    datt = fmaf(d, y[(int64_t)t * 128 + tid], datt);
    dy[(int64_t)t * 128 + tid] = d * at;
  }
  datt = fmaf(dav[T - 1], y[(int64_t)(T - 1) * 128 + tid], datt);
  const float dot = block128_sum(at * datt, red);
  dsc[tid] = at * (datt - dot);
  a.dsc[(int64_t)b * 128 + tid] = dsc[tid];
  __syncthreads();
  {
    const float* w = P + a.off[P_ATW] + tid;
    float s = 0.0f;
    for (int j = 0; j < 128; ++j) s = fmaf(dsc[j], w[j * 128], s);
    s = a.q[(int64_t)b * 128 + tid] > 0.0f ? s : 0.0f;
    dzq[tid] = s;
    a.dzq[(int64_t)b * 128 + tid] = s;
  }
  __syncthreads();
  {
    const float* w = P + a.off[P_D1W] + tid;
    float s = 0.0f;
    for (int j = 0; j < 128; ++j) s = fmaf(dzq[j], w[j * 128], s);
    dy[(int64_t)(T - 1) * 128 + tid] = dav[T - 1] * at + s;
  }
}

// ------------------------------------------------------------------ host side
void param_sizes(int T, int F, int K, int64_t* sz) {
  const int64_t head[8] = {50, 10, 10, 10, 50, 1, 1, 1};
  for (int i = 0; i < 8; ++i) sz[i] = head[i];
  for (int layer = 0; layer < 2; ++layer)
    for (int dir = 0; dir < 2; ++dir) {
      int64_t* s = sz + 8 + layer * 8 + dir * 4;
      s[0] = (int64_t)kGates * (layer ? 2 * kHid : F);
      s[1] = kGates * kHid;
      s[2] = kGates;
      s[3] = kGates;
    }
  const int64_t tail[10] = {128 * 128, 128, 128 * 128, 128, 64LL * T, 64, 32 * 64, 32, 32LL * K, K};
  for (int i = 0; i < 10; ++i) sz[24 + i] = tail[i];
}

// workspace map (byte offsets); every buffer 256-byte aligned
struct Layout {
  size_t a1, a2, x0, xp, y1, gates1, c1, y2, gates2, c2, dy2, dy1, dx0, dz2, q, att, av, d2, d2m, d3, logits,
      dlogits, dz3, dzh2, dsc, dzq, mask, rowinfo, coef, part, slab, colp, total;
  int ksplit;
  int64_t kchunk;
};

int slabs_for(int64_t N) { return (int)std::max<int64_t>(1, std::min<int64_t>(kMaxSlabs, (N + 2047) / 2048)); }

Layout make_layout(const abd_lstmattn* n, int64_t B) {
  Layout L{};
  Take take;
  const int64_t BT = B * n->T, N = BT * n->F;
  L.a1 = take(4 * N * kC1);
  L.a2 = take(4 * N);
  L.x0 = take(4 * N);
  L.xp = take(4 * 2 * BT * kGates);   // input projections forward, gate gradients backward
  L.y1 = take(4 * BT * 128);
  L.gates1 = take(4 * 2 * BT * kGates);
  L.c1 = take(4 * 2 * BT * kHid);
  L.y2 = take(4 * BT * 128);
  L.gates2 = take(4 * 2 * BT * kGates);
  L.c2 = take(4 * 2 * BT * kHid);
  L.dy2 = take(4 * BT * 128);
  L.dy1 = take(4 * BT * 128);
  L.dx0 = take(4 * N);
  L.dz2 = take(4 * N);
  L.q = take(4 * B * 128);
  L.att = take(4 * B * 128);
  L.av = take(4 * BT);
  L.d2 = take(4 * B * 64);
  L.d2m = take(4 * B * 64);
  L.d3 = take(4 * B * 32);
  L.logits = take(4 * B * n->K);
  L.dlogits = take(4 * B * n->K);
  L.dz3 = take(4 * B * 32);
  L.dzh2 = take(4 * B * 64);
  L.dsc = take(4 * B * 128);
  L.dzq = take(4 * B * 128);
  L.mask = take(B * 64);
  L.rowinfo = take(4 * B * 4);
  L.coef = take(4 * 64);
  L.part = take(8 * (size_t)kC1 * kMaxSlabs * kQ);
  // weight-gradient GEMMs: B*T rows of reduction split into slices of >= 256 rows
  const Slices sl = plan_slices(BT, 64, 256, 8);
  L.ksplit = sl.ksplit;
  L.kchunk = sl.kchunk;
  L.slab = take(4 * (size_t)L.ksplit * kGates * 128);
  L.colp = take(4 * (size_t)64 * kGates);
  L.total = take.o;
  return L;
}

struct Ctx : CtxBase {
  const abd_lstmattn* n;
  Layout L;
  Offs offs() const {
    Offs o;
    for (int i = 0; i < 35; ++i) o.v[i] = n->off[i];
    return o;
  }
};

int launch_gemm(hipStream_t s, GemmArgs g, int ksplit) {
  if (g.M <= 0 || g.N <= 0) return ABD_OK;
  if (ksplit <= 1) g.kchunk = (g.K + 7) & ~7;
  dim3 grid((g.M + 31) / 32, (g.N + 31) / 32, std::max(1, ksplit));
  gemm_kernel<<<grid, 64, 0, s>>>(g);
  ABD_LAUNCH_CHECK();
  return ABD_OK;
}

// Raise the kernel's dynamic-LDS limit once per device (bit d of *done = device d has it; devices past
// 63 set it on every call).
template <class K>
int ensure_lds(K kern, size_t bytes, std::atomic<unsigned long long>* done) {
  int dev = 0;
  ABD_HIP(hipGetDevice(&dev));
  const unsigned long long bit = (dev >= 0 && dev < 64) ? 1ull << dev : 0ull;
  if (bit && (done->load(std::memory_order_acquire) & bit)) return ABD_OK;
  ABD_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize,
                              (int)bytes));
  done->fetch_or(bit, std::memory_order_release);
  return ABD_OK;
}

constexpr size_t kFwdLds = sizeof(float) * (kHid * kWtLd + kTile * kHid);
constexpr size_t kBwdLds = sizeof(float) * (kGates * kHid + kTile * kGates);

ConvArgs conv_args(const Ctx& c, const float* x, float* running, int64_t* nbt, int train) {
  ConvArgs a{};
  a.x = x;
  a.a1 = c.at<float>(c.L.a1);
  a.a2 = c.at<float>(c.L.a2);
  a.x0 = c.at<float>(c.L.x0);
  a.params = c.params;
  a.off = c.offs();
  a.coef = c.at<float>(c.L.coef);
  a.part = c.at<double>(c.L.part);
  a.grads = c.grads;
  a.dx0 = c.at<float>(c.L.dx0);
  a.dz2 = c.at<float>(c.L.dz2);
  a.running = running;
  a.nbt = nbt;
  a.N = c.B * c.n->T * c.n->F;
  a.T = c.n->T;
  a.F = c.n->F;
  a.S = slabs_for(a.N);
  a.train = train;
  return a;
}

HeadArgs head_args(const Ctx& c, int train) {
  HeadArgs h{};
  h.params = c.params;
  h.off = c.offs();
  h.y = c.at<float>(c.L.y2);
  h.q = c.at<float>(c.L.q);
  h.att = c.at<float>(c.L.att);
  h.av = c.at<float>(c.L.av);
  h.d2 = c.at<float>(c.L.d2);
  h.d2m = c.at<float>(c.L.d2m);
  h.d3 = c.at<float>(c.L.d3);
  h.logits = c.at<float>(c.L.logits);
  h.keep = c.at<uint8_t>(c.L.mask);
  h.dz3 = c.at<float>(c.L.dz3);
  h.dz2 = c.at<float>(c.L.dzh2);
  h.dsc = c.at<float>(c.L.dsc);
  h.dzq = c.at<float>(c.L.dzq);
  h.dy = c.at<float>(c.L.dy2);
  h.T = c.n->T;
  h.K = c.n->K;
  h.train = train;
  return h;
}

// one bidirectional layer forward: projections (one GEMM per direction), then the recurrence
int lstm_layer_fwd(const Ctx& c, int layer, const float* x, int in, float* y, float* gates, float* cs) {
  static std::atomic<unsigned long long> lds_ok{0};
  if (int rc = ensure_lds(&lstm_fwd_kernel, kFwdLds, &lds_ok)) return rc;
  const int64_t BT = c.B * c.n->T;
  const int p0 = layer ? P_R2 : P_R1;
  float* xp = c.at<float>(c.L.xp);
  LstmArgs la{};
  for (int dir = 0; dir < 2; ++dir) {
    const int64_t* off = c.n->off + p0 + dir * 4;
    GemmArgs g = gemm_nt(x, in, c.params + off[0], xp + (int64_t)dir * BT * kGates, (int)BT, kGates, in);
    g.bias1 = c.params + off[2];
    g.bias2 = c.params + off[3];
    if (int rc = launch_gemm(c.s, g)) return rc;
    la.whh[dir] = c.params + off[1];
  }
  la.xp = xp;
  la.y = y;
  la.gates = gates;
  la.c = cs;
  la.B = (int)c.B;
  la.T = c.n->T;
  lstm_fwd_kernel<<<dim3((unsigned)((c.B + kTile - 1) / kTile), 2), kT, kFwdLds, c.s>>>(la);
  ABD_LAUNCH_CHECK();
  return ABD_OK;
}

// one layer backward: the recurrence -> dgates, then dW_hh, dW_ih, the bias gradients and dx
int lstm_layer_bwd(const Ctx& c, int layer, const float* x, int in, const float* y, const float* gates,
                   const float* cs, const float* dy, float* dx) {
  static std::atomic<unsigned long long> lds_ok{0};
  if (int rc = ensure_lds(&lstm_bwd_kernel, kBwdLds, &lds_ok)) return rc;
  const int64_t BT = c.B * c.n->T;
  const int p0 = layer ? P_R2 : P_R1;
  float* dg = c.at<float>(c.L.xp);
  LstmArgs la{};
  for (int dir = 0; dir < 2; ++dir) la.whh[dir] = c.params + c.n->off[p0 + dir * 4 + 1];
  la.gates = const_cast<float*>(gates);
  la.c = const_cast<float*>(cs);
  la.dy = dy;
  la.dg = dg;
  la.B = (int)c.B;
  la.T = c.n->T;
  lstm_bwd_kernel<<<dim3((unsigned)((c.B + kTile - 1) / kTile), 2), kT, kBwdLds, c.s>>>(la);
  ABD_LAUNCH_CHECK();
  float* slab = c.at<float>(c.L.slab);
  for (int dir = 0; dir < 2; ++dir) {
    const int64_t* off = c.n->off + p0 + dir * 4;
    const float* dgd = dg + (int64_t)dir * BT * kGates;
    // dW_ih[j][i] = sum_rows dg[row][j] x[row][i]
    GemmArgs g = gemm_tn(dgd, x, in, slab, kGates, in, BT);
    g.cz = (int64_t)kGates * in;
    g.kchunk = (int)c.L.kchunk;
    if (int rc = launch_gemm(c.s, g, c.L.ksplit)) return rc;
    if (int rc = colsum(c, slab, c.L.ksplit, g.cz, g.cz, c.grads + off[0])) return rc;
    // dW_hh[j][k] = sum_rows dg[row][j] h_prev[row][k]; h_prev is the y row one step back in this
    // direction's order (t-1 forward, t+1 reverse), zero at the sequence start
    g = gemm_tn(dgd, y + dir * kHid, 2 * kHid, slab, kGates, kHid, BT);
    g.cz = (int64_t)kGates * kHid;
    g.kchunk = (int)c.L.kchunk;
    g.T = c.n->T;
    g.shift = dir ? 1 : -1;
    if (c.n->T > 1) {
      if (int rc = launch_gemm(c.s, g, c.L.ksplit)) return rc;
      if (int rc = colsum(c, slab, c.L.ksplit, g.cz, g.cz, c.grads + off[1])) return rc;
    } else {
      ABD_HIP(hipMemsetAsync(c.grads + off[1], 0, sizeof(float) * kGates * kHid, c.s));
    }
    if (int rc = colsum(c, dgd, BT, kGates, kGates, c.grads + off[2])) return rc;
    ABD_HIP(hipMemcpyAsync(c.grads + off[3], c.grads + off[2], sizeof(float) * kGates, hipMemcpyDeviceToDevice, c.s));
    // dx[row][i] (+)= sum_j dg[row][j] W_ih[j][i]
    GemmArgs d = gemm_nn(dgd, kGates, c.params + off[0], dx, (int)BT, in, kGates);
    d.accumulate = dir;
    if (int rc = launch_gemm(c.s, d)) return rc;
  }
  return ABD_OK;
}

struct Fwd {
  const float* x;
  float* running;
  int64_t* nbt;
  int train;
  const uint8_t* mask_in;
  uint8_t* mask_out;
  uint64_t seed, counter;
  int64_t row_offset;
};

// the batched front end: conv1 -> BatchNorm1 -> conv2 -> BatchNorm2 over the whole batch -> x0
int run_front(const Ctx& c, const Fwd& f) {
  ConvArgs a = conv_args(c, f.x, f.running, f.nbt, f.train);
  const unsigned nblk = (unsigned)((a.N + kT - 1) / kT);
  conv1_kernel<<<nblk, kT, 0, c.s>>>(a);
  ABD_LAUNCH_CHECK();
  if (f.train) {
    bn_stats_kernel<0><<<dim3(a.S, kC1), kT, 0, c.s>>>(a, a.a1);
    ABD_LAUNCH_CHECK();
  }
  bn_finalize_kernel<<<1, 64, 0, c.s>>>(a, kC1, 0, 0, 0);
  ABD_LAUNCH_CHECK();
  conv2_kernel<<<nblk, kT, 0, c.s>>>(a);
  ABD_LAUNCH_CHECK();
  if (f.train) {
    bn_stats_kernel<0><<<dim3(a.S, 1), kT, 0, c.s>>>(a, a.a2);
    ABD_LAUNCH_CHECK();
  }
  bn_finalize_kernel<<<1, 64, 0, c.s>>>(a, 1, 20, 2 * kC1, 1);
  ABD_LAUNCH_CHECK();
  bn2_apply_kernel<<<nblk, kT, 0, c.s>>>(a);
  ABD_LAUNCH_CHECK();
  return ABD_OK;
}

// behind x0: the two bidirectional layers and the head.  logits: where the head writes them.
int run_tail(const Ctx& c, const Fwd& f, float* logits) {
  if (int rc = lstm_layer_fwd(c, 0, c.at<float>(c.L.x0), c.n->F, c.at<float>(c.L.y1), c.at<float>(c.L.gates1),
                              c.at<float>(c.L.c1)))
    return rc;
  if (int rc = lstm_layer_fwd(c, 1, c.at<float>(c.L.y1), 2 * kHid, c.at<float>(c.L.y2), c.at<float>(c.L.gates2),
                              c.at<float>(c.L.c2)))
    return rc;
  HeadArgs h = head_args(c, f.train);
  h.logits = logits;
  h.mask_in = f.mask_in;
  h.mask_out = f.mask_out;
  h.seed = f.seed;
  h.counter = f.counter;
  h.row_offset = f.row_offset;
  head_fwd_kernel<<<(unsigned)c.B, 128, 0, c.s>>>(h);
  ABD_LAUNCH_CHECK();
  return ABD_OK;
}

int run_forward(const Ctx& c, const Fwd& f) {
  if (int rc = run_front(c, f)) return rc;
  return run_tail(c, f, c.at<float>(c.L.logits));
}

// The per-utterance forward's workspace: x0, one layer's projections / gates / cell states (the second layer
// overwrites the first's: nothing reads them back without a backward pass) and the head's outputs.  No a1, no
// gradient, statistics or slab buffers.  Fields it leaves 0 belong to kernels this path never launches.
Layout make_pu_layout(const abd_lstmattn* n, int64_t B) {
  Layout L{};
  Take take;
  const int64_t BT = B * n->T;
  L.x0 = take(4 * BT * n->F);
  L.xp = take(4 * 2 * BT * kGates);
  L.y1 = take(4 * BT * 128);
  L.gates1 = L.gates2 = take(4 * 2 * BT * kGates);
  L.c1 = L.c2 = take(4 * 2 * BT * kHid);
  L.y2 = take(4 * BT * 128);
  L.q = take(4 * B * 128);
  L.att = take(4 * B * 128);
  L.av = take(4 * BT);
  L.d2 = take(4 * B * 64);
  L.d2m = take(4 * B * 64);
  L.d3 = take(4 * B * 32);
  L.mask = take(B * 64);
  L.total = take.o;
  return L;
}

// dW[o][i] = sum_b delta[b][o] act[b*act_ld + i], db[o] = sum_b delta[b][o]
int dense_grads(const Ctx& c, const float* delta, int out, const float* act, int in, int64_t act_ld, int pw) {
  if (int rc = launch_gemm(c.s, gemm_tn(delta, act, act_ld, c.grads + c.n->off[pw], out, in, c.B))) return rc;
  return colsum(c, delta, c.B, out, out, c.grads + c.n->off[pw + 1]);
}

int run_backward(const Ctx& c, const float* x, const float* dlogits) {
  const int T = c.n->T, F = c.n->F, K = c.n->K;
  HeadArgs h = head_args(c, 1);
  h.dlogits = dlogits;
  head_bwd_kernel<<<(unsigned)c.B, 128, 0, c.s>>>(h);
  ABD_LAUNCH_CHECK();
  if (int rc = dense_grads(c, dlogits, K, h.d3, 32, 32, P_OW)) return rc;
  if (int rc = dense_grads(c, h.dz3, 32, h.d2m, 64, 64, P_D3W)) return rc;
  if (int rc = dense_grads(c, h.dz2, 64, h.av, T, T, P_D2W)) return rc;
  if (int rc = dense_grads(c, h.dsc, 128, h.q, 128, 128, P_ATW)) return rc;
  if (int rc = dense_grads(c, h.dzq, 128, h.y + (int64_t)(T - 1) * 128, 128, (int64_t)T * 128, P_D1W)) return rc;
  if (int rc = lstm_layer_bwd(c, 1, c.at<float>(c.L.y1), 2 * kHid, c.at<float>(c.L.y2), c.at<float>(c.L.gates2),
                              c.at<float>(c.L.c2), c.at<float>(c.L.dy2), c.at<float>(c.L.dy1)))
    return rc;
  if (int rc = lstm_layer_bwd(c, 0, c.at<float>(c.L.x0), F, c.at<float>(c.L.y1), c.at<float>(c.L.gates1),
                              c.at<float>(c.L.c1), c.at<float>(c.L.dy1), c.at<float>(c.L.dx0)))
    return rc;
  ConvArgs a = conv_args(c, x, nullptr, nullptr, 1);
  const unsigned nblk = (unsigned)((a.N + kT - 1) / kT);
  bn_stats_kernel<1><<<dim3(a.S, 1), kT, 0, c.s>>>(a, nullptr);
  ABD_LAUNCH_CHECK();
  bn2_bwd_finalize_kernel<<<1, 64, 0, c.s>>>(a);
  ABD_LAUNCH_CHECK();
  dz2_kernel<<<nblk, kT, 0, c.s>>>(a);
  ABD_LAUNCH_CHECK();
  conv_bwd_kernel<0><<<dim3(a.S, kC1), kT, 0, c.s>>>(a);
  ABD_LAUNCH_CHECK();
  conv_bwd_finalize_kernel<0><<<1, 64, 0, c.s>>>(a);
  ABD_LAUNCH_CHECK();
  conv_bwd_kernel<1><<<dim3(a.S, kC1), kT, 0, c.s>>>(a);
  ABD_LAUNCH_CHECK();
  conv_bwd_finalize_kernel<1><<<1, 64, 0, c.s>>>(a);
  ABD_LAUNCH_CHECK();
  return ABD_OK;
}

int make_ctx(const abd_lstmattn* net, int64_t B, const float* params, float* grads, void* ws, size_t bytes,
             abd_stream_t stream, Ctx* c) {
  return make_ctx(net, B, params, grads, ws, bytes, stream, kGates * 2, make_layout, c);
}

}  // namespace

extern "C" {

int abd_lstmattn_tile_rows(void) { return kTile; }

int abd_lstmattn_create(int T, int F, int num_classes, abd_lstmattn** net) {
  ABD_CHECK(net != nullptr, ABD_E_INVALID, "NULL out pointer");
  ABD_CHECK(F >= 1 && F <= 128, ABD_E_UNSUPPORTED, "lstmwithattention: time_len %d outside [1, 128]", F);
  ABD_CHECK(T >= 1 && T <= 1024, ABD_E_UNSUPPORTED, "lstmwithattention: seq_len %d outside [1, 1024]", T);
  ABD_CHECK(num_classes >= 1 && num_classes <= 4096, ABD_E_UNSUPPORTED, "num_classes must be in [1, 4096]");
  auto* n = new abd_lstmattn();
  n->T = T;
  n->F = F;
  n->K = num_classes;
  int64_t sz[P_COUNT];
  param_sizes(T, F, num_classes, sz);
  n->off[0] = 0;
  for (int i = 0; i < P_COUNT; ++i) n->off[i + 1] = n->off[i] + sz[i];
  *net = n;
  return ABD_OK;
}

void abd_lstmattn_destroy(abd_lstmattn* net) { delete net; }

int64_t abd_lstmattn_param_count(const abd_lstmattn* net) { return net ? net->off[P_COUNT] : 0; }

int abd_lstmattn_param_offsets(const abd_lstmattn* net, int64_t* offsets) {
  ABD_CHECK(net && offsets, ABD_E_INVALID, "NULL argument");
  for (int i = 0; i <= P_COUNT; ++i) offsets[i] = net->off[i];
  return ABD_OK;
}

size_t abd_lstmattn_workspace_bytes(const abd_lstmattn* net, int64_t batch) {
  if (!net || batch < 1) return 0;
  return make_layout(net, batch).total;
}

int64_t abd_lstmattn_workspace_offset(const abd_lstmattn* net, int64_t batch, const char* name) {
  if (!net || !name || batch < 1) return -1;
  const Layout L = make_layout(net, batch);
  const NamedOffset tab[] = {
      {"a1", L.a1}, {"a2", L.a2}, {"x0", L.x0}, {"y1", L.y1}, {"gates1", L.gates1}, {"c1", L.c1}, {"y2", L.y2},
      {"gates2", L.gates2}, {"c2", L.c2}, {"dy2", L.dy2}, {"dy1", L.dy1}, {"dx0", L.dx0}, {"q", L.q}, {"att", L.att},
      {"av", L.av}, {"d2", L.d2}, {"d3", L.d3}, {"logits", L.logits}, {"dlogits", L.dlogits}, {"mask", L.mask},
      {"rowinfo", L.rowinfo}};
  return find_offset(tab, name);
}

int abd_lstmattn_forward(abd_lstmattn* net, const abd_lstmattn_args* a, int train_mode, void* workspace,
                         size_t workspace_bytes, abd_stream_t stream) {
  ABD_CHECK(a != nullptr && a->x && a->running, ABD_E_INVALID, "NULL x / running");
  ABD_CHECK(!train_mode || net == nullptr || a->batch * net->T * net->F > 1, ABD_E_INVALID,
            "train-mode BatchNorm needs more than one value per channel (B*T*F = 1)");
  Ctx c;
  if (int rc = make_ctx(net, a->batch, a->params, a->grads, workspace, workspace_bytes, stream, &c)) return rc;
  const Fwd f{a->x, a->running, a->num_batches_tracked, train_mode ? 1 : 0, a->mask_in, a->mask_out,
              a->seed, a->counter, a->row_offset};
  if (int rc = run_forward(c, f)) return rc;
  return run_ce(c, nullptr, nullptr, false, 1.0f, a->logits_out, nullptr);
}

int abd_lstmattn_backward(abd_lstmattn* net, const abd_lstmattn_args* a, const float* dlogits, void* workspace,
                          size_t workspace_bytes, abd_stream_t stream) {
  ABD_CHECK(a != nullptr && a->x && a->grads && dlogits, ABD_E_INVALID, "NULL x / grads / dlogits");
  Ctx c;
  if (int rc = make_ctx(net, a->batch, a->params, a->grads, workspace, workspace_bytes, stream, &c)) return rc;
  return run_backward(c, a->x, dlogits);
}

int abd_lstmattn_train_step(abd_lstmattn* net, const abd_lstmattn_args* a, void* workspace, size_t workspace_bytes,
                            abd_stream_t stream) {
  ABD_CHECK(a != nullptr && a->x && a->running && a->grads, ABD_E_INVALID, "NULL x / running / grads");
  if (int rc = check_train_args(a)) return rc;
  ABD_CHECK(net == nullptr || a->batch * net->T * net->F > 1, ABD_E_INVALID,
            "train-mode BatchNorm needs more than one value per channel (B*T*F = 1)");
  Ctx c;
  if (int rc = make_ctx(net, a->batch, a->params, a->grads, workspace, workspace_bytes, stream, &c)) return rc;
  const Fwd f{a->x, a->running, a->num_batches_tracked, 1, a->mask_in, a->mask_out, a->seed, a->counter,
              a->row_offset};
  if (int rc = run_forward(c, f)) return rc;
  if (int rc = run_ce(c, a->labels, a->indicators, true, a->grad_scale, a->logits_out, a->metrics)) return rc;
  if (int rc = run_backward(c, a->x, c.at<float>(c.L.dlogits))) return rc;
  return adam_tail(a, net->off[P_COUNT], stream);
}

int abd_lstmattn_eval(abd_lstmattn* net, const float* x, int64_t batch, const float* params, const float* running,
                      const int64_t* labels, const int64_t* indicators, float* logits, int64_t* metrics,
                      void* workspace, size_t workspace_bytes, abd_stream_t stream) {
  ABD_CHECK(x && running && logits, ABD_E_INVALID, "NULL x / running / logits");
  Ctx c;
  if (int rc = make_ctx(net, batch, params, nullptr, workspace, workspace_bytes, stream, &c)) return rc;
  const Fwd f{x, const_cast<float*>(running), nullptr, 0, nullptr, nullptr, 0, 0, 0};
  if (int rc = run_forward(c, f)) return rc;
  return run_ce(c, labels, indicators, false, 1.0f, logits, metrics);
}

size_t abd_per_utterance_lstmattn_workspace_bytes(const abd_lstmattn* net, int64_t batch) {
  if (!net || batch < 1) return 0;
  return make_pu_layout(net, batch).total;
}

int abd_per_utterance_lstmattn_forward(abd_lstmattn* net, const float* x, int64_t batch, const float* params,
                                       uint64_t seed, uint64_t counter, const uint8_t* mask_in, float* logits,
                                       void* workspace, size_t workspace_bytes, abd_stream_t stream) {
  ABD_CHECK(net != nullptr, ABD_E_INVALID, "NULL network");
  ABD_CHECK(x && logits, ABD_E_INVALID, "NULL x / logits");
  const int64_t TF = (int64_t)net->T * net->F;
  ABD_CHECK(TF > 1, ABD_E_INVALID, "train-mode BatchNorm needs more than one value per channel (T*F = 1)");
  ABD_CHECK(TF <= kPuMaxTF, ABD_E_UNSUPPORTED,
            "per-utterance forward: T*F = %lld exceeds %d (the utterance and relu(conv2) stay in LDS)", (long long)TF,
            kPuMaxTF);
  Ctx c;
  if (int rc = make_ctx(net, batch, params, nullptr, workspace, workspace_bytes, stream, kGates * 2, make_pu_layout,
                        &c))
    return rc;
  const size_t lds = sizeof(float) * 2 * (size_t)TF;
  if (lds > 64 * 1024) {
    static std::atomic<unsigned long long> lds_ok{0};
    if (int rc = ensure_lds(&front_per_utterance_kernel, sizeof(float) * 2 * kPuMaxTF, &lds_ok)) return rc;
  }
  FrontArgs a{};
  a.x = x;
  a.x0 = c.at<float>(c.L.x0);
  a.params = params;
  a.off = c.offs();
  a.T = net->T;
  a.F = net->F;
  front_per_utterance_kernel<<<(unsigned)batch, kT, lds, c.s>>>(a);
  ABD_LAUNCH_CHECK();
  const Fwd f{x, nullptr, nullptr, 1, mask_in, nullptr, seed, counter, 0};
  return run_tail(c, f, logits);
}

}  // extern "C"
