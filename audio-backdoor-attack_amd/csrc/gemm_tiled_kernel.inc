// The LDS-tiled fp32 GEMM of rnn.hip and smalllstm.hip: gemm_tiled_kernel and the launch_gemm that lstm_common.inc
// declares.  Included after lstm_common.inc (GemmArgs) and the file's kT and kLargeMinBlocks.  largecnn.hip includes
// gemm_tiled.inc alone: a launcher that names gemm_tiled_kernel<1, 1> and <2, 2> would add them to its object.
#include "gemm_tiled.inc"   // kBK, the tile sizes, f16v and launch_tiled

// ------------------------------------------------------------------ LDS-tiled fp32 MFMA GEMM (GemmArgs)
// An operand tile in LDS: [row][kBK + 1] when k is the contiguous index in memory, [k][rows + 32] when
// the row is.  Either way consecutive threads write consecutive words, and the MFMA's operand read
// (lanes 0..31: 32 rows at k, lanes 32..63: the same rows at k + 1) touches 64 different banks.
template <int TM, int TN>
__global__ void __launch_bounds__(kT) gemm_tiled_kernel(GemmArgs a) {
  constexpr int BM = 64 * TM, BN = 64 * TN;
  constexpr int NA = BM * kBK / kT, NB = BN * kBK / kT;
  __shared__ float As[kBK * (BM + 32)];
  __shared__ float Bs[kBK * (BN + 32)];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int wm = (w >> 1) * TM * 32, wn = (w & 1) * TN * 32;
  const int m0 = blockIdx.x * BM, n0 = blockIdx.y * BN;
  const int k0 = blockIdx.z * a.kchunk;
  const int k1 = min(a.K, k0 + a.kchunk);
  const bool a_kc = a.sak == 1, b_kc = a.sbk == 1;
  const int a_sm = a_kc ? kBK + 1 : 1, a_sk = a_kc ? 1 : BM + 32;
  const int b_sn = b_kc ? kBK + 1 : 1, b_sk = b_kc ? 1 : BN + 32;
  f16v acc[TM][TN];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.0f;
  for (int kb = k0; kb < k1; kb += kBK) {
    float ar[NA], br[NB];
#pragma unroll
    for (int i = 0; i < NA; ++i) {
      const int e = tid + i * kT;
      const int m = a_kc ? e >> 5 : e % BM, k = a_kc ? e & 31 : e / BM;
      const int gm = m0 + m, gk = kb + k;
      ar[i] = (gm < a.M && gk < k1) ? a.A[(int64_t)gm * a.sam + (int64_t)gk * a.sak] : 0.0f;
    }
#pragma unroll
    for (int i = 0; i < NB; ++i) {
      const int e = tid + i * kT;
      const int n = b_kc ? e >> 5 : e % BN, k = b_kc ? e & 31 : e / BN;
      const int gn = n0 + n, gk = kb + k;
      float v = 0.0f;
      if (gn < a.N && gk < k1) {
        if (a.shift == 0) {
          v = a.B[(int64_t)gk * a.sbk + (int64_t)gn * a.sbn];
        } else {
          const int ts = gk % a.T + a.shift;
          if (ts >= 0 && ts < a.T) v = a.B[(int64_t)(gk + a.shift) * a.sbk + (int64_t)gn * a.sbn];
        }
      }
      br[i] = v;
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
    float bias = 0.0f;
    if (a.bias1) bias += a.bias1[n];
    if (a.bias2) bias += a.bias2[n];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int m = m0 + wm + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
        if (m < a.M) {
          float* c = C + (int64_t)m * a.ldc + n;
          const float v = acc[i][j][r] + bias;
          *c = a.accumulate ? *c + v : v;
        }
      }
  }
}

int launch_gemm(hipStream_t s, GemmArgs g, int ksplit) {
  if (g.M <= 0 || g.N <= 0) return ABD_OK;
  ksplit = std::max(1, ksplit);
  if (ksplit == 1) g.kchunk = std::max(g.K, 1);
  return launch_tiled(s, g.M, g.N, ksplit, kLargeMinBlocks, gemm_tiled_kernel<1, 1>, gemm_tiled_kernel<2, 2>, g);
}
