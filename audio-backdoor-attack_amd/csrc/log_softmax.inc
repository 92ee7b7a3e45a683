// log_softmax over the K classes of a row and its gradient, for the nets whose reference ends in one (largecnn.hip,
// smalllstm.hip).  Included after abd_common.h.  Not in net_common.inc: a __global__ function is emitted into every
// object that includes its text, also into those that never launch it.

// one wave per row: lp = z - max - log(sum exp(z - max))
__global__ void __launch_bounds__(64) lsm_fwd_kernel(const float* z, float* lp, int K) {
  const int row = blockIdx.x, lane = threadIdx.x;
  const float* zr = z + (int64_t)row * K;
  float mx = -INFINITY;
  for (int j = lane; j < K; j += 64) mx = fmaxf(mx, zr[j]);
  mx = abd::wave_max(mx);
  float se = 0.0f;
  for (int j = lane; j < K; j += 64) se += expf(zr[j] - mx);
  se = abd::wave_sum(se);
  const float lse = __ocml_log_f32(se);
  for (int j = lane; j < K; j += 64) lp[(int64_t)row * K + j] = (zr[j] - mx) - lse;
}

// dz = dlp - exp(lp) * sum(dlp)
__global__ void __launch_bounds__(64) lsm_bwd_kernel(const float* lp, const float* dlp, float* dz, int K) {
  const int row = blockIdx.x, lane = threadIdx.x;
  const int64_t o = (int64_t)row * K;
  float s = 0.0f;
  for (int j = lane; j < K; j += 64) s += dlp[o + j];
  s = abd::wave_sum(s);
  for (int j = lane; j < K; j += 64) dz[o + j] = dlp[o + j] - expf(lp[o + j]) * s;
}
