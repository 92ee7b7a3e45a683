// Included by smallcnn.hip (anonymous namespace): the fused fc head of the train step.
//
// utils/models.py:52-65 -- pool3 -> drop1 -> flatten -> fc1 -> relu -> drop2 -> fc2 -> log_softmax,
// CrossEntropy on the log-probs (utils/training_tools.py:65-67) and their backward down to conv3's
// input gradient, in FOUR launches (round 2: seven), each sized for the whole chip:
//
//   head_fwd_kernel<PP>  grid (row tiles of 32, position splits of PP pooled positions)
//       BN3 + max-pool3 + dropout1 straight from r3 into an LDS A tile (32 rows x 32 channels x PP
//       positions) -> p3d, the dropout mask and xhat of each pool-selected element (xh3: BN3's
//       backward sums need no division by gamma) -> fc1 split-K partial on v_mfma_f32_32x32x2_f32
//       against fc1^T (one coalesced 128-B row per K step) -> slab[split][row][unit]
//   head_row_kernel      grid (row pairs)
//       the rows' split-K sums in split order + bias + ReLU + dropout2 (d2), fc2, log_softmax, CE on
//       the log-probs, dL/dz through both log_softmaxes, da = (dz W2) * drop2' * relu' (stored row-
//       major for the weight gradient and transposed, daT, as the next GEMM's A operand)
//   head_dgrad_kernel    grid (32-feature tiles, 128-row blocks)
//       dp3 = (da W1) * drop1' on v_mfma_f32_32x32x2_f32 (W1's 128 x 32 slice staged in LDS once per
//       block) and BN3's backward sums sum dy, sum dy * xhat per (row block, feature tile, channel)
//   head_bwd_kernel      one launch, block roles by index:
//       fc1 weight gradient in 32 x 32 tiles over the whole batch (4 waves split the rows, summed in
//       order), fc2 weight / bias and fc1 bias gradients, the batch counters (metrics_body) with
//       BN3's dgamma / dbeta, and BN3's backward applied to dz3 (every apply block reduces the few
//       per-channel partials of head_dgrad itself) with the conv3 bias-gradient partials
//
// Every reduction has a fixed order (no atomics): the results are deterministic.

struct HeadArgs {
  int B, F, P, K;        // rows, flat features = 32 channels x P pooled positions, classes
  int ks;                // head_fwd: position splits (PP positions each)
  int nft, nrb;          // head_dgrad: 32-feature tiles, 128-row blocks
  PoolArgs pool;         // pool3 geometry, r3, BN3 coefficients (coef + 128), flat_n = F
  DropArgs drop1, drop2;
  const float* f1t;      // fc1.weight^T (F, 128)
  const float* w1;       // fc1.weight (128, F)
  const float* b1;
  const float* w2;       // fc2.weight (K, 128)
  const float* b2;
  const float* bn3w;     // BN3 gamma
  const int64_t* labels;
  const int64_t* ind;
  float inv_batch;       // grad_scale / B
  float* p3d;
  float* xh3;
  float* slab;           // (ks, B, 128)
  float* d2;
  float* logp;
  float* dz;
  float* rowinfo;
  float* da;             // (B, 128)
  float* daT;            // (128, B)
  float* dp3;
  const uint8_t* mask1;  // written by head_fwd (drop1.mask_out)
  float* part3;          // BN3 backward partials [(rb * nft + ft) * 64 + 2 * slot + {0: sum dy, 1: sum dy xhat}]
  // head_bwd
  float* g_f1w;
  float* g_f1b;
  float* g_f2w;
  float* g_f2b;
  float* g_bn3w;
  float* g_bn3b;
  int64_t* metrics;
  double loss_w;
  float* dz3;            // BN3 backward output (NHWC)
  float* partb3;         // conv3 bias-gradient partials [32][n_apply]
  int n_w1, n_w2, n_apply;
  int hx, wx;            // BN3 apply: extended window grid (win_ext_h / win_ext_w)
};
typedef float f32x4v __attribute__((ext_vector_type(4)));

constexpr int kHeadRows = 2;   // rows per head_row block
constexpr int kHeadRB = 128;   // rows per head_dgrad block (4 waves x 32)
constexpr int kHeadW2 = 64;    // fc2 / bias gradient outputs per head_bwd block
constexpr int kHeadIT = 2;     // BN3 apply windows per thread

__device__ __forceinline__ bool drop_keep(const DropArgs& d, int64_t idx) {
  return d.mask_in ? (d.mask_in[idx] != 0) : keep_hash(d.seed, d.stream, d.base + (uint64_t)idx, d.p);
}

// ---------------------------------------------------------------- launch 1
// A tile row-major per batch row with the K index permuted as k' = (k & 1) * STEPS + (k >> 1), so the
// 32x32x2 MFMA's operand of lane (row, kh) for four consecutive K steps is one ds_read_b128; row
// stride KS + 4 floats puts each 8-lane phase of that read on distinct banks.
template <int PP>
__global__ void __launch_bounds__(kT) head_fwd_kernel(HeadArgs a) {
  constexpr int KS = 32 * PP, STEPS = KS / 2, AS = KS + 4, XS = KS + 1;
  __shared__ __attribute__((aligned(16))) float As[32 * AS];  // p3d values (A operand)
  __shared__ float Xs[32 * XS];                                // xhat of the selected elements [row][c * PP + pl]
  __shared__ uint8_t Ms[32 * XS];                              // dropout1 keep bits, same layout
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int b0 = blockIdx.x * 32;
  const int pos0 = blockIdx.y * PP, npos = min(PP, a.P - pos0);
  const PoolArgs& pa = a.pool;
  // ---- B operand (fc1^T rows of this split), all K steps in flight: wave w -> units [32 w, 32 w + 32)
  const int u = 32 * wave + (lane & 31), kh = lane >> 5;
  float bv[STEPS];
  {
    const float* lb = a.f1t + (int64_t)kh * a.P * 128 + u;
#pragma unroll
    for (int st = 0; st < STEPS; ++st) {
      // k = 2 st + kh: pooled position pl = st >> 4, channel c = (2 st & 31) + kh (zero A rows past P)
      const int pos = min(pos0 + (st >> 4), a.P - 1);
      bv[st] = lb[(int64_t)((2 * st) & 31) * a.P * 128 + (int64_t)pos * 128];
    }
  }
  // ---- BN3 + pool3 + dropout1 (thread: 4 channels of one row, every position of the split)
  const int cg = tid & 7, rloc = tid >> 3;
  const int c0 = cg * 4, b = b0 + rloc;
  const bool brow = b < a.B;
  float4 cf[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) cf[q] = pa.coef[c0 + q];
#pragma unroll
  for (int pl = 0; pl < PP; ++pl) {
    float v[4] = {0.f, 0.f, 0.f, 0.f}, xh[4] = {0.f, 0.f, 0.f, 0.f};
    bool kp[4] = {false, false, false, false};
    if (pl < npos) {
      const int pos = pos0 + pl, ho = pos / pa.Wo, wo = pos - ho * pa.Wo;
      float4 rv[4];
      bool in[4];
#pragma unroll
      for (int slot = 0; slot < 4; ++slot) {
        const int h = ho * pa.sh - pa.ph + slot / 2, w = wo * pa.sw - pa.pw + slot % 2;
        in[slot] = h >= 0 && h < pa.H && w >= 0 && w < pa.W;
        rv[slot] = (brow && in[slot]) ? *reinterpret_cast<const float4*>(pa.r + (((int64_t)b * pa.H + h) * pa.W + w) * pa.C + c0)
                                      : make_float4(0.f, 0.f, 0.f, 0.f);
      }
      if (brow) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          // first maximum in scan order of bn(r) over the window (win_argmax's rule)
          float best = -INFINITY, rs = 0.0f;
#pragma unroll
          for (int slot = 0; slot < 4; ++slot) {
            const float r = f4get(rv[slot], q);
            const float yv = fmaf(cf[q].z, r, cf[q].w);
            if (in[slot] && yv > best) {
              best = yv;
              rs = r;
            }
          }
          const int64_t oi = (int64_t)b * a.F + (int64_t)(c0 + q) * a.P + pos;
          kp[q] = a.drop1.enabled ? drop_keep(a.drop1, oi) : true;
          v[q] = a.drop1.enabled ? (kp[q] ? best * a.drop1.scale : 0.0f) : best;
          xh[q] = (rs - cf[q].x) * cf[q].y;  // xhat of the pool-selected element
        }
      }
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int k = pl * 32 + c0 + q;
      As[rloc * AS + (k & 1) * STEPS + (k >> 1)] = v[q];
      Xs[rloc * XS + (c0 + q) * PP + pl] = xh[q];
      Ms[rloc * XS + (c0 + q) * PP + pl] = kp[q] ? 1 : 0;
    }
  }
  __syncthreads();
  // ---- p3d / xh3 / mask: runs of npos consecutive features per (row, channel)
  if (PP >= 4 && a.P % PP == 0) {
    // whole splits: one 16-B store per (row, channel) and array (PP = 4), positions in a register quad
#pragma unroll
    for (int it = 0; it < 4; ++it) {
      const int i = it * kT + tid, c = i & 31, row = i >> 5;
      if (b0 + row < a.B) {
        const int64_t oi = (int64_t)(b0 + row) * a.F + (int64_t)c * a.P + pos0;
#pragma unroll
        for (int h = 0; h < PP / 4; ++h) {
          float4 pv, xv;
          uint32_t mv = 0;
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            const int pl = 4 * h + q, k = pl * 32 + c;
            f4set(pv, q, As[row * AS + (k & 1) * STEPS + (k >> 1)]);
            f4set(xv, q, Xs[row * XS + c * PP + pl]);
            mv |= (uint32_t)Ms[row * XS + c * PP + pl] << (8 * q);
          }
          *reinterpret_cast<float4*>(a.p3d + oi + 4 * h) = pv;
          *reinterpret_cast<float4*>(a.xh3 + oi + 4 * h) = xv;
          if (a.drop1.mask_out) *reinterpret_cast<uint32_t*>(a.drop1.mask_out + oi + 4 * h) = mv;
        }
      }
    }
  } else {
#pragma unroll
    for (int it = 0; it < 4 * PP; ++it) {
      const int i = it * kT + tid;
      const int pl = i % PP, c = (i / PP) & 31, row = i / (32 * PP);
      if (pl < npos && b0 + row < a.B) {
        const int k = pl * 32 + c;
        const int64_t oi = (int64_t)(b0 + row) * a.F + (int64_t)c * a.P + pos0 + pl;
        a.p3d[oi] = As[row * AS + (k & 1) * STEPS + (k >> 1)];
        a.xh3[oi] = Xs[row * XS + c * PP + pl];
        if (a.drop1.mask_out) a.drop1.mask_out[oi] = Ms[row * XS + c * PP + pl];
      }
    }
  }
  // ---- fc1 split-K partial: wave w -> units [32 w, 32 w + 32), all 32 rows, K = 32 * PP
  f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.0f;
  const float* arow = As + (lane & 31) * AS + kh * STEPS;
#pragma unroll
  for (int j = 0; j < STEPS / 4; ++j) {
    const float4 av = *reinterpret_cast<const float4*>(arow + 4 * j);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av.x, bv[4 * j + 0], acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av.y, bv[4 * j + 1], acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av.z, bv[4 * j + 2], acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av.w, bv[4 * j + 3], acc, 0, 0, 0);
  }
  float* out = a.slab + ((int64_t)blockIdx.y * a.B) * 128;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int row = (r & 3) + 8 * (r >> 2) + 4 * kh;
    if (b0 + row < a.B) out[(int64_t)(b0 + row) * 128 + u] = acc[r];
  }
}

// ---------------------------------------------------------------- launch 2
// Two rows per block (thread: row tid >> 7, unit tid & 127).
__global__ void __launch_bounds__(kT) head_row_kernel(HeadArgs a) {
  constexpr int R = kHeadRows;
  __shared__ float w2s[64][129];  // fc2.weight [k][u]
  __shared__ float d2s[R][128];
  __shared__ float zs[R][64];     // fc2 logits, then dL/dz
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r = tid >> 7, u = tid & 127;
  const int b = blockIdx.x * R + r;
  const bool ok = b < a.B;
  // ---- fc1: split-K sums in split order (up to 32 partials in flight) + bias + ReLU + dropout2;
  // fc2.weight's loads are issued first
  float wv[(64 * 128) / kT];
#pragma unroll
  for (int q = 0; q < (64 * 128) / kT; ++q) {
    const int e = q * kT + tid;
    wv[q] = e < a.K * 128 ? a.w2[e] : 0.0f;
  }
  float v = 0.0f;
  if (ok) {
    const float* sp = a.slab + (int64_t)b * 128 + u;
    const int64_t st = (int64_t)a.B * 128;
    for (int s0 = 0; s0 < a.ks; s0 += 32) {
      float t[32];
#pragma unroll
      for (int q = 0; q < 32; ++q) t[q] = (s0 + q < a.ks) ? sp[(s0 + q) * st] : 0.0f;
#pragma unroll
      for (int q = 0; q < 32; ++q) v += t[q];  // past ks: + 0
    }
  }
  const float bias = a.b1[u];
#pragma unroll
  for (int q = 0; q < (64 * 128) / kT; ++q) {
    const int e = q * kT + tid;
    if (e < a.K * 128) w2s[e >> 7][e & 127] = wv[q];
  }
  float d = 0.0f;
  if (ok) {
    const int64_t e = (int64_t)b * 128 + u;
    d = drop_apply(a.drop2, e, fmaxf(v + bias, 0.0f));
    a.d2[e] = d;
  }
  d2s[r][u] = d;
  __syncthreads();
  // ---- fc2 logits z[r][k]: four interleaved fma chains over the 128 units
  if (tid < R * a.K) {
    const int rr = tid / a.K, k = tid - rr * a.K;
    float c4[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 8
    for (int j = 0; j < 32; ++j) {
#pragma unroll
      for (int q = 0; q < 4; ++q) c4[q] = fmaf(d2s[rr][4 * j + q], w2s[k][4 * j + q], c4[q]);
    }
    zs[rr][k] = ((c4[0] + c4[1]) + (c4[2] + c4[3])) + a.b2[k];
  }
  __syncthreads();
  // ---- log_softmax, CE on the log-probs, dL/dz through both log_softmaxes: one wave per row
  if (wave < R) {
    const int rr = wave, bb = blockIdx.x * R + rr;
    if (bb < a.B) {
      const bool act = lane < a.K;
      const float z = act ? zs[rr][lane] : -INFINITY;
      const float mz = abd::wave_max(z);
      const float ez = act ? expf(z - mz) : 0.0f;
      const float lse = mz + logf(abd::wave_sum(ez));
      const float o = act ? z - lse : -INFINITY;
      const float mo = abd::wave_max(o);
      const float eo = act ? expf(o - mo) : 0.0f;
      const float so = abd::wave_sum(eo);
      const float lse2 = mo + logf(so);
      const int y = (int)a.labels[bb];
      const float oy = __shfl(o, y, 64);
      const unsigned long long ball = __ballot(act && o == mo);
      const int pred = __ffsll((long long)ball) - 1;
      float dov = 0.0f;
      if (act) dov = (eo / so - (lane == y ? 1.0f : 0.0f)) * a.inv_batch;
      const float sdo = abd::wave_sum(dov);
      const float dzl = act ? dov - expf(o) * sdo : 0.0f;
      zs[rr][lane] = dzl;  // lanes >= K: 0
      if (act) {
        a.logp[(int64_t)bb * a.K + lane] = o;
        a.dz[(int64_t)bb * a.K + lane] = dzl;
      }
      if (lane == 0) {
        const bool pois = a.ind != nullptr && a.ind[bb] == 1;
        float* ri = a.rowinfo + (int64_t)bb * 4;
        ri[0] = lse2 - oy;
        ri[1] = (pred == y) ? 1.0f : 0.0f;
        ri[2] = pois ? 1.0f : 0.0f;
        ri[3] = (pois && pred == y) ? 1.0f : 0.0f;
      }
    } else {
      zs[rr][lane] = 0.0f;
    }
  }
  __syncthreads();
  // ---- da = (dz . W2) * scale2 * [d2 > 0]   (fc2_bwd_body's order over k)
  if (ok) {
    float s = 0.0f;
    for (int k = 0; k < a.K; ++k) s = fmaf(zs[r][k], w2s[k][u], s);
    const float dav = d > 0.0f ? s * a.drop2.scale : 0.0f;
    a.da[(int64_t)b * 128 + u] = dav;
    a.daT[(int64_t)u * a.B + b] = dav;
  }
}

// ---------------------------------------------------------------- launch 3
// dp3[b][f] = drop1'(sum_u da[b][u] W1[u][f]): block = 128 rows x 32 features, wave w = rows
// [32 w, 32 w + 32) of the block.  BN3's backward sums per (row block, tile, channel slot):
// slot j of tile ft is channel (32 ft) / P + j.
__global__ void __launch_bounds__(kT) head_dgrad_kernel(HeadArgs a) {
  __shared__ float Ws[128][33];     // W1[u][f0 + j]
  __shared__ float cs[4][2][32];    // per-wave column sums
  __shared__ float col[2][32];      // block column sums
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int f0 = blockIdx.x * 32, rb0 = blockIdx.y * kHeadRB;
  const int kh = lane >> 5, cl = lane & 31;
  const int brow = min(rb0 + 32 * wave + cl, a.B - 1);  // A-operand row (clamped; stores are masked)
  float av[64];
#pragma unroll
  for (int s = 0; s < 64; ++s) av[s] = a.daT[(int64_t)(2 * s + kh) * a.B + brow];
  // epilogue operands in flight too: dropout1 keep bits and xhat of this lane's 16 outputs
  float xh[16];
  uint8_t km[16];
  const int fo = f0 + cl;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int row = rb0 + 32 * wave + (r & 3) + 8 * (r >> 2) + 4 * kh;
    const int64_t oi = (int64_t)min(row, a.B - 1) * a.F + fo;
    xh[r] = a.xh3[oi];
    km[r] = a.drop1.enabled ? a.mask1[oi] : (uint8_t)1;
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int e = i * kT + tid, uu = e >> 3, j4 = (e & 7) * 4;
    const float4 w4 = *reinterpret_cast<const float4*>(a.w1 + (int64_t)uu * a.F + f0 + j4);
    Ws[uu][j4 + 0] = w4.x;
    Ws[uu][j4 + 1] = w4.y;
    Ws[uu][j4 + 2] = w4.z;
    Ws[uu][j4 + 3] = w4.w;
  }
  __syncthreads();
  f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.0f;
#pragma unroll
  for (int s = 0; s < 64; ++s) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av[s], Ws[2 * s + kh][cl], acc, 0, 0, 0);
  const float sc = a.drop1.enabled ? a.drop1.scale : 1.0f;
  float s1 = 0.0f, s2 = 0.0f;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int row = rb0 + 32 * wave + (r & 3) + 8 * (r >> 2) + 4 * kh;
    if (row < a.B) {
      const float dy = km[r] ? acc[r] * sc : 0.0f;
      a.dp3[(int64_t)row * a.F + fo] = dy;
      s1 += dy;
      s2 = fmaf(dy, xh[r], s2);
    }
  }
  s1 += __shfl_xor(s1, 32, 64);
  s2 += __shfl_xor(s2, 32, 64);
  if (lane < 32) {
    cs[wave][0][lane] = s1;
    cs[wave][1][lane] = s2;
  }
  __syncthreads();
  if (tid < 64) {
    const int m = tid >> 5, j = tid & 31;
    col[m][j] = ((cs[0][m][j] + cs[1][m][j]) + cs[2][m][j]) + cs[3][m][j];
  }
  __syncthreads();
  // channel slots of this tile: columns of one channel summed in column order
  const int clo = f0 / a.P, nslot = (f0 + 31) / a.P - clo + 1;
  if (tid < 2 * nslot) {
    const int j = tid >> 1, m = tid & 1, c = clo + j;
    const int t0 = max(0, c * a.P - f0), t1 = min(32, (c + 1) * a.P - f0);
    float sacc = 0.0f;
    for (int t = t0; t < t1; ++t) sacc += col[m][t];
    a.part3[((int64_t)blockIdx.y * a.nft + blockIdx.x) * 64 + 2 * j + m] = sacc;
  }
}

// ---------------------------------------------------------------- launch 4
// BN3 backward sums of channel c (m = 0: sum dy, 1: sum dy * xhat) from head_dgrad's partials, in a
// fixed order (row blocks, then tiles)
__device__ __forceinline__ double head_bn3_sum(const HeadArgs& a, int c, int m) {
  const int ft0 = (c * a.P) / 32, ft1 = ((c + 1) * a.P - 1) / 32;
  double s = 0.0;
  for (int rb = 0; rb < a.nrb; ++rb)
    for (int ft = ft0; ft <= ft1; ++ft) {
      const int j = c - (32 * ft) / a.P;
      s += (double)a.part3[((int64_t)rb * a.nft + ft) * 64 + 2 * j + m];
    }
  return s;
}

// out[m][n] = sum_b A[b][m] Bm[b][n] over all rows for the 32 x 32 tile at (m0, n0) (m < arows,
// n < bcols): 4 waves each take a quarter of the rows on v_mfma_f32_32x32x2_f32, summed in wave order.
// The next 32-row chunk's operands are in flight while the current chunk's MFMAs run.
__device__ __forceinline__ void grad_tile(const float* __restrict__ A, int lda, int arows,
                                          const float* __restrict__ Bm, int ldb, int bcols, int nrows, int m0, int n0,
                                          float* __restrict__ out, int ldo) {
  __shared__ float rw[4][32][33];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int rows = (nrows + 3) / 4, r0 = wave * rows, r1 = min(nrows, r0 + rows);
  f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.0f;
  const int kh = lane >> 5, col = lane & 31;
  const bool mok = m0 + col < arows, nok = n0 + col < bcols;
  constexpr int CH = 16;
  float a0[CH], b0v[CH], a1[CH], b1v[CH];
  auto fetch = [&](float (&av)[CH], float (&bv)[CH], int bb) {
#pragma unroll
    for (int s = 0; s < CH; ++s) {
      const int b = bb + 2 * s + kh;
      const bool ok = b < r1;
      av[s] = (ok && mok) ? A[(int64_t)b * lda + m0 + col] : 0.0f;
      bv[s] = (ok && nok) ? Bm[(int64_t)b * ldb + n0 + col] : 0.0f;
    }
  };
  auto mma = [&](const float (&av)[CH], const float (&bv)[CH]) {
#pragma unroll
    for (int s = 0; s < CH; ++s) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av[s], bv[s], acc, 0, 0, 0);
  };
  if (r0 < r1) fetch(a0, b0v, r0);
  for (int bb = r0; bb < r1; bb += 4 * CH) {
    if (bb + 2 * CH < r1) fetch(a1, b1v, bb + 2 * CH);
    mma(a0, b0v);
    if (bb + 2 * CH >= r1) break;
    if (bb + 4 * CH < r1) fetch(a0, b0v, bb + 4 * CH);
    mma(a1, b1v);
  }
#pragma unroll
  for (int r = 0; r < 16; ++r) rw[wave][(r & 3) + 8 * (r >> 2) + 4 * kh][col] = acc[r];
  __syncthreads();
  for (int o = tid; o < 32 * 32; o += kT) {
    const int mm = o >> 5, nn = o & 31;
    if (m0 + mm < arows && n0 + nn < bcols)
      out[(int64_t)(m0 + mm) * ldo + n0 + nn] = ((rw[0][mm][nn] + rw[1][mm][nn]) + rw[2][mm][nn]) + rw[3][mm][nn];
  }
}

__global__ void __launch_bounds__(kT) head_bwd_kernel(HeadArgs a) {
  const int tid = threadIdx.x;
  int bid = blockIdx.x;
  if (bid < a.n_w1) {  // ---- fc1 weight gradient: dW1[u][f] = sum_b da[b][u] p3d[b][f]
    grad_tile(a.da, 128, 128, a.p3d, a.F, a.F, a.B, 32 * (bid & 3), 32 * (bid >> 2), a.g_f1w, a.F);
    return;
  }
  bid -= a.n_w1;
  const int nt2 = 4 * ((a.K + 31) / 32);
  if (bid < nt2) {  // ---- fc2 weight gradient: dW2[k][u] = sum_b dz[b][k] d2[b][u]
    grad_tile(a.dz, a.K, a.K, a.d2, 128, 128, a.B, 32 * (bid >> 2), 32 * (bid & 3), a.g_f2w, 128);
    return;
  }
  if (bid < a.n_w2) {
    // ---- fc2 / fc1 bias gradients: column sums of dz (K) and da (128); 64 outputs x 4 row quarters
    __shared__ float rq[4][kHeadW2];
    const int o = (bid - nt2) * kHeadW2 + (tid & 63), qr = tid >> 6;
    const int total = a.K + 128;
    const int rows = (a.B + 3) / 4, r0 = qr * rows, r1 = min(a.B, r0 + rows);
    const float* src = (o < a.K) ? a.dz + o : a.da + (o - a.K);
    const int ld = (o < a.K) ? a.K : 128;
    float sacc = 0.0f;
    if (o < total) {
      int b = r0;
      for (; b + 8 <= r1; b += 8) {
        float t[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) t[j] = src[(int64_t)(b + j) * ld];
#pragma unroll
        for (int j = 0; j < 8; ++j) sacc += t[j];
      }
      for (; b < r1; ++b) sacc += src[(int64_t)b * ld];
    }
    rq[qr][tid & 63] = sacc;
    __syncthreads();
    if (tid < 64 && o < total) {
      const float v = ((rq[0][tid] + rq[1][tid]) + rq[2][tid]) + rq[3][tid];
      if (o < a.K) a.g_f2b[o] = v;
      else a.g_f1b[o - a.K] = v;
    }
    return;
  }
  bid -= a.n_w2;
  if (bid == 0) {
    // ---- batch counters (as the round-2 train step: metrics_body over rowinfo) + BN3 dgamma / dbeta
    if (a.metrics) metrics_body(a.rowinfo, a.B, a.metrics, a.loss_w);
    if (tid < 64) {
      const double v = head_bn3_sum(a, tid >> 1, tid & 1);
      if (tid & 1) a.g_bn3w[tid >> 1] = (float)v;
      else a.g_bn3b[tid >> 1] = (float)v;
    }
    return;
  }
  bid -= 1;
  // ---- BN3 backward applied: dz3 = relu'(r3) * bn_dx(dy routed to the pool argmax) (bn_bwd_apply_kernel)
  // kHeadIT windows per thread; their r3 / dp3 loads are issued before the block reduces the BN3
  // partials, so the reduction's latency overlaps them
  const PoolArgs& pa = a.pool;
  const int hx = a.hx, wx = a.wx;
  const int CG = pa.C / 4;
  const int total = pa.B * hx * wx * CG;
  const int c0 = (tid % CG) * 4;
  float4 rv[kHeadIT][4];
  bool in[kHeadIT][4];
  float dy[kHeadIT][4];
  WinIdx wi[kHeadIT];
  bool val[kHeadIT];
#pragma unroll
  for (int it = 0; it < kHeadIT; ++it) {
    const int o = (bid * kHeadIT + it) * kT + tid;
    val[it] = o < total;
    wi[it] = win_index(val[it] ? o : 0, CG, wx, hx);
    const bool real = val[it] && wi[it].ho < pa.Ho && wi[it].wo < pa.Wo;
#pragma unroll
    for (int slot = 0; slot < 4; ++slot) {
      const int h = wi[it].ho * pa.sh - pa.ph + slot / 2, w = wi[it].wo * pa.sw - pa.pw + slot % 2;
      in[it][slot] = val[it] && h >= 0 && h < pa.H && w >= 0 && w < pa.W;
      rv[it][slot] = in[it][slot] ? *reinterpret_cast<const float4*>(pa.r + ((wi[it].b * pa.H + h) * pa.W + w) * pa.C + c0)
                                  : make_float4(0.f, 0.f, 0.f, 0.f);
    }
    load_dy4(pa, wi[it].b, wi[it].ho, wi[it].wo, c0, real, dy[it]);
  }
  __shared__ double sums[32][2];
  __shared__ BCoef bcs[32];
  if (tid < 64) sums[tid >> 1][tid & 1] = head_bn3_sum(a, tid >> 1, tid & 1);
  __syncthreads();
  if (tid < 32) {
    const double count = (double)a.B * pa.H * pa.W;
    const float4 cc = pa.coef[tid];
    const double g = (double)a.bn3w[tid] * (double)cc.y, mdy = sums[tid][0] / count, mdyx = sums[tid][1] / count;
    const double mean = (double)cc.x, invstd = (double)cc.y;
    bcs[tid] = BCoef{g, g * (mdyx * invstd * mean - mdy), -g * mdyx * invstd, 0.0};
  }
  __syncthreads();
  float4 cf[4];
  BCoef bc[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    cf[q] = pa.coef[c0 + q];
    bc[q] = bcs[c0 + q];
  }
  float v[1][4] = {};
#pragma unroll
  for (int it = 0; it < kHeadIT; ++it) {
    if (!val[it]) continue;
    const bool real = wi[it].ho < pa.Ho && wi[it].wo < pa.Wo;
    int arg[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {  // first maximum in scan order (win_argmax's rule)
      float best = -INFINITY;
      arg[q] = -1;
#pragma unroll
      for (int slot = 0; slot < 4; ++slot) {
        const float y = fmaf(cf[q].z, f4get(rv[it][slot], q), cf[q].w);
        if (in[it][slot] && y > best) {
          best = y;
          arg[q] = slot;
        }
      }
    }
#pragma unroll
    for (int slot = 0; slot < 4; ++slot) {
      if (!in[it][slot]) continue;
      const int h = wi[it].ho * pa.sh - pa.ph + slot / 2, w = wi[it].wo * pa.sw - pa.pw + slot % 2;
      float4 dzv;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const float r = f4get(rv[it][slot], q);
        const float d = (real && arg[q] == slot) ? dy[it][q] : 0.0f;
        const float zz = r > 0.0f ? bn_dx(d, r, cf[q], bc[q]) : 0.0f;
        f4set(dzv, q, zz);
        v[0][q] += zz;
      }
      *reinterpret_cast<float4*>(a.dz3 + ((wi[it].b * pa.H + h) * pa.W + w) * pa.C + c0) = dzv;
    }
  }
  cgroup_partials<1>(v, pa.C, a.partb3, a.n_apply, bid);
}
