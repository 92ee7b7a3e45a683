// correlation_analysis.py:102-158 (unlearning_correlation_analysis): the backdoored model is unlearned once on
// clean and once on poisoned rows, always on the same first batch of an unshuffled loader, and the two
// neuron-weight-change vectors are correlated.
//   * abd_smallcnn_unlearn_run sequences n_steps public abd_smallcnn_unlearn_step calls on one batch: one
//     host call for the whole loop of :141-143, nothing of the step re-implemented;
//   * abd_nwc_pair_f32 is :146-157 for both models at once: the row kernel of tsbd.hip with the original
//     read once for two unlearned parameter sets and the unrounded double row sums kept (the values the
//     reference's Python ``sum()`` makes for its CSV), then a one-block kernel for the two columns' means,
//     centred sums, Pearson r and the least-squares line.
// Every launch is asynchronous on the caller's stream, allocates nothing and copies nothing from the host.
// No atomics, no cross-block waits: the statistics kernel is a second launch, and its reductions walk LDS
// in a fixed order, so equal inputs give bit-equal results.
#include <cmath>
#include <type_traits>

#include "abd_common.h"

namespace {

// kT, RowTab / make_rowtab / row_abs_sums_body
#include "defense_common.inc"

constexpr int kMaxRows = ABD_MAX_REINIT_ROWS;

// tsbd.hip's row_abs_sums_kernel for two buffers against one original: the one shared row body, hence the
// same fp32 row sums bit for bit; the double sums are kept before that rounding.
__global__ void __launch_bounds__(kT) nwc_pair_rows_kernel(const float* __restrict__ orig,
                                                           const float* __restrict__ pa,
                                                           const float* __restrict__ pb, RowTab t,
                                                           float* __restrict__ absdiff_a, float* __restrict__ absdiff_b,
                                                           float* __restrict__ sums32_a, float* __restrict__ sums32_b,
                                                           double* __restrict__ sums64, int total_rows) {
  const float* const ps[2] = {pa, pb};
  float* const ad[2] = {absdiff_a, absdiff_b};
  double acc[2];
  const int r = row_abs_sums_body<2>(t, ps, orig, ad, acc);
  if (r >= 0) {
    sums32_a[r] = (float)acc[0];
    sums32_b[r] = (float)acc[1];
    sums64[r] = acc[0];
    sums64[total_rows + r] = acc[1];
  }
}

// Block-wide sum in a fixed order: thread i's value into LDS slot i, then halving strides.  Not
// finetune.hip's block_sum_d, which adds in another order.
__device__ __forceinline__ double block_sum(double v, double* sm) {
  const int tid = threadIdx.x;
  __syncthreads();  // the previous reduction's readers are done with sm
  sm[tid] = v;
  __syncthreads();
  for (int o = kT >> 1; o > 0; o >>= 1) {
    if (tid < o) sm[tid] += sm[tid + o];
    __syncthreads();
  }
  return sm[0];
}

// One block over the n <= kMaxRows pairs (x[i], y[i]) = (sums64[i], sums64[n + i]): the means, then the
// centred sums; thread i takes elements i, i + kT, ... of each pass.
__global__ void __launch_bounds__(kT) nwc_pair_stats_kernel(const double* __restrict__ sums64, int n,
                                                            double* __restrict__ stats) {
  __shared__ double sm[kT];
  const int tid = threadIdx.x;
  const double* x = sums64;
  const double* y = sums64 + n;
  double ax = 0.0, ay = 0.0;
  for (int i = tid; i < n; i += kT) {
    ax += x[i];
    ay += y[i];
  }
  const double mean_x = block_sum(ax, sm) / (double)n;
  const double mean_y = block_sum(ay, sm) / (double)n;
  double axx = 0.0, ayy = 0.0, axy = 0.0;
  for (int i = tid; i < n; i += kT) {
    const double dx = x[i] - mean_x, dy = y[i] - mean_y;
    axx += dx * dx;
    ayy += dy * dy;
    axy += dx * dy;
  }
  const double sxx = block_sum(axx, sm);
  const double syy = block_sum(ayy, sm);
  const double sxy = block_sum(axy, sm);
  if (tid == 0) {
    const double nan = __builtin_nan("");
    const double prod = sxx * syy;
    const double r = (n < 2 || prod == 0.0) ? nan : sxy / sqrt(prod);
    const double slope = sxx == 0.0 ? nan : sxy / sxx;
    stats[0] = (double)n;
    stats[1] = mean_x;
    stats[2] = mean_y;
    stats[3] = sxx;
    stats[4] = syy;
    stats[5] = sxy;
    stats[6] = r;
    stats[7] = slope;
    stats[8] = sxx == 0.0 ? nan : mean_y - slope * mean_x;
  }
}

}  // namespace

extern "C" {

int abd_smallcnn_unlearn_run(abd_cnn* net, const abd_unlearn_args* a, int64_t n_steps, void* workspace,
                             size_t workspace_bytes, abd_stream_t stream) {
  ABD_CHECK(net && a, ABD_E_INVALID, "NULL argument");
  ABD_CHECK(n_steps >= 1, ABD_E_INVALID, "unlearning run needs n_steps >= 1, got %lld", (long long)n_steps);
  ABD_CHECK(a->record_rows == 0 && a->record_abs_sums == nullptr, ABD_E_INVALID,
            "an unlearning run records no layer: record_rows and record_abs_sums must be unset");
  const int64_t B = a->batch;
  const int64_t flat = abd_smallcnn_flat_features(net);
  for (int64_t i = 0; i < n_steps; ++i) {
    abd_unlearn_args s = *a;
    s.adam_step = a->adam_step + i;
    s.counter = a->counter + (uint64_t)i;
    if (a->mask1_in) s.mask1_in = a->mask1_in + i * B * flat;
    if (a->mask2_in) s.mask2_in = a->mask2_in + i * B * 128;
    if (a->mask1_out) s.mask1_out = a->mask1_out + i * B * flat;
    if (a->mask2_out) s.mask2_out = a->mask2_out + i * B * 128;
    if (a->metrics) s.metrics = a->metrics + i * ABD_METRICS_WORDS;
    if (int rc = abd_smallcnn_unlearn_step(net, &s, workspace, workspace_bytes, stream)) return rc;
  }
  return ABD_OK;
}

int abd_nwc_pair_f32(const float* orig, const float* params_a, const float* params_b, const abd_row_segment* table,
                     int n_seg, float* absdiff_a, float* absdiff_b, float* sums32_a, float* sums32_b, double* sums64,
                     double* stats, abd_stream_t stream) {
  RowTab t;
  if (int rc = make_rowtab(table, n_seg, &t)) return rc;
  ABD_CHECK(orig && params_a && params_b && sums32_a && sums32_b && sums64 && stats, ABD_E_INVALID, "NULL argument");
  const int total_rows = t.rowfirst[n_seg];
  ABD_CHECK(total_rows <= kMaxRows, ABD_E_INVALID, "row table has %d rows, at most %d", total_rows, kMaxRows);
  hipStream_t s = static_cast<hipStream_t>(stream);
  nwc_pair_rows_kernel<<<(unsigned)t.first[n_seg], kT, 0, s>>>(orig, params_a, params_b, t, absdiff_a, absdiff_b,
                                                              sums32_a, sums32_b, sums64, total_rows);
  ABD_LAUNCH_CHECK();
  nwc_pair_stats_kernel<<<1, kT, 0, s>>>(sums64, total_rows, stats);
  ABD_LAUNCH_CHECK();
  return ABD_OK;
}

}  // extern "C"
