// Fixed-order column sums, cross entropy and the ABD_METRICS_WORDS counters, shared by lstm_attn.hip, rnn.hip,
// largecnn.hip and resnet.hip.  Included by net_common.inc, inside each file's anonymous namespace, after
// abd_common.h.

constexpr int kRedT = 256;   // threads of colsum_kernel / metrics_kernel

// The device library's natural logarithm, used by ce_kernel only.  It is what torch's std::log resolves to,
// so d(logits) equals torch's CrossEntropyLoss backward bit for bit.  Plain logf would be just as accurate
// (both within an ulp); the only thing it loses is last-bit equality of the autograd path with the fused
// step, which tests/test_gpu_lstm_attention.py::test_autograd_path_bit_equal_to_train_step watches.
extern "C" __device__ float __ocml_log_f32(float);

// out[s*out_ld + col] (+)= sum over rows [s*chunk, (s+1)*chunk) of A[row*ld + col], in row order
__global__ void __launch_bounds__(kRedT) colsum_kernel(const float* A, int64_t rows, int64_t cols, int64_t ld,
                                                       int64_t chunk, float* out, int64_t out_ld, int accumulate) {
  const int64_t col = (int64_t)blockIdx.x * kRedT + threadIdx.x;
  if (col >= cols) return;
  const int64_t r0 = (int64_t)blockIdx.y * chunk, r1 = min(rows, r0 + chunk);
  double s = 0.0;
  for (int64_t r = r0; r < r1; ++r) s += (double)A[r * ld + col];
  float* o = out + (int64_t)blockIdx.y * out_ld + col;
  *o = accumulate ? *o + (float)s : (float)s;
}

// ------------------------------------------------------------------ cross entropy + counters
struct CeArgs {
  const float* logits;
  const int64_t* labels;
  const int64_t* ind;
  float* dlogits;   // optional
  float* rowinfo;   // (B, 4): loss, correct, poisoned, poisoned & correct
  float* logits_out;
  int K;
  float scale;      // grad_scale / B
};

// one wave per row; the predicted class is the first index of the maximum (torch max(dim=1))
__global__ void __launch_bounds__(64) ce_kernel(CeArgs a) {
  const int row = blockIdx.x, lane = threadIdx.x, K = a.K;
  const float* z = a.logits + (int64_t)row * K;
  float mx = -INFINITY;
  int arg = K;
  for (int j = lane; j < K; j += 64) {
    const float v = z[j];
    if (a.logits_out) a.logits_out[(int64_t)row * K + j] = v;
    if (v > mx) {
      mx = v;
      arg = j;
    }
  }
  const float m = abd::wave_max(mx);
  int cand = (mx == m) ? arg : K;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) cand = min(cand, __shfl_xor(cand, o, 64));
  if (!a.labels) return;
  float se = 0.0f;
  for (int j = lane; j < K; j += 64) se += expf(z[j] - m);
  se = abd::wave_sum(se);
  const int y = (int)a.labels[row];
  // d(logits) in the arithmetic of torch's log_softmax / nll_loss backward (grad - exp(log_softmax) * sum(grad)
  // with grad = -scale at the label), so the autograd path (torch's CrossEntropyLoss) and the fused step agree
  // The logarithm is the device library's __ocml_log_f32, which torch's std::log resolves to; logf here
  // expands to the compiler's own sequence, which differs from it in the last bit for about a third of
  // the arguments (expf agrees with torch's std::exp bit for bit).
  const float lse = __ocml_log_f32(se);
  if (a.dlogits)
    for (int j = lane; j < K; j += 64) {
      const float o = (z[j] - m) - lse;
      const float g = (j == y) ? -a.scale : 0.0f;
      a.dlogits[(int64_t)row * K + j] = g - expf(o) * (-a.scale);
    }
  if (lane == 0) {
    const bool pois = a.ind != nullptr && a.ind[row] == 1;
    float* ri = a.rowinfo + (int64_t)row * 4;
    ri[0] = (y >= 0 && y < K) ? -((z[y] - m) - lse) : 0.0f;
    ri[1] = cand == y ? 1.0f : 0.0f;
    ri[2] = pois ? 1.0f : 0.0f;
    ri[3] = (pois && cand == y) ? 1.0f : 0.0f;
  }
}

// one block: batch reduction in a fixed order -> the ABD_METRICS_WORDS counters
__global__ void __launch_bounds__(kRedT) metrics_kernel(const float* rowinfo, int B, int64_t* metrics, double lw) {
  double s = 0.0;
  long long c = 0, p = 0, h = 0;
  for (int i = threadIdx.x; i < B; i += kRedT) {
    s += rowinfo[i * 4 + 0];
    c += (long long)rowinfo[i * 4 + 1];
    p += (long long)rowinfo[i * 4 + 2];
    h += (long long)rowinfo[i * 4 + 3];
  }
  __shared__ double rs[kRedT];
  __shared__ long long rc[3][kRedT];
  rs[threadIdx.x] = s;
  rc[0][threadIdx.x] = c;
  rc[1][threadIdx.x] = p;
  rc[2][threadIdx.x] = h;
  __syncthreads();
  for (int o = kRedT / 2; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) {
      rs[threadIdx.x] += rs[threadIdx.x + o];
      for (int j = 0; j < 3; ++j) rc[j][threadIdx.x] += rc[j][threadIdx.x + o];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    double acc = __longlong_as_double(metrics[0]);
    acc += rs[0] * lw / B;
    metrics[0] = __double_as_longlong(acc);
    metrics[1] += B;
    metrics[2] += rc[0][0];
    metrics[3] += rc[1][0];
    metrics[4] += rc[2][0];
    metrics[5] += 1;
  }
}
