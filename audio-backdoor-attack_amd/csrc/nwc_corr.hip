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

#include "abd_common.h"

namespace {

constexpr int kT = 256;
constexpr int kMaxSeg = ABD_MAX_SEGMENTS;
constexpr int kMaxRows = ABD_MAX_REINIT_ROWS;

// tsbd.hip's row table, its builder and absdiff_one, restated unchanged: abd_common.h belongs to the
// benchmarked step's sources (scripts/traffic_json.py's csrc_sha1) and stays as it is.
// Segment s: rows[s] rows of len[s] floats from element off[s] of the flat buffer.  Its rows are
// rows rowfirst[s].. of the table, its values start at packfirst[s] of the packed |a - b| buffer.
// In the row-sum kernel a row is handled by group[s] lanes (a power of two <= 64) and the segment by
// blocks [first[s], first[s + 1]).
struct RowTab {
  int64_t off[kMaxSeg];
  int64_t packfirst[kMaxSeg + 1];
  int rows[kMaxSeg];
  int len[kMaxSeg];
  int rowfirst[kMaxSeg + 1];
  int group[kMaxSeg];
  int first[kMaxSeg + 1];
  int n;
};

int make_rowtab(const abd_row_segment* table, int n_seg, RowTab* t) {
  ABD_CHECK(table != nullptr, ABD_E_INVALID, "NULL row table");
  ABD_CHECK(n_seg >= 1 && n_seg <= kMaxSeg, ABD_E_INVALID, "n_seg must be in [1, %d], got %d", kMaxSeg, n_seg);
  int64_t rows = 0, packed = 0, blocks = 0, end = 0;
  for (int s = 0; s < n_seg; ++s) {
    const abd_row_segment& g = table[s];
    ABD_CHECK(g.rows >= 1 && g.row_len >= 1, ABD_E_INVALID, "segment %d has empty rows (%lld rows of %lld)", s,
              (long long)g.rows, (long long)g.row_len);
    ABD_CHECK(g.rows < (1LL << 24) && g.row_len < (1LL << 24), ABD_E_INVALID, "segment %d is too large", s);
    ABD_CHECK(g.offset >= end, ABD_E_INVALID, "segment %d starts at %lld, inside or before its predecessor (ends %lld)",
              s, (long long)g.offset, (long long)end);
    end = g.offset + g.rows * g.row_len;
    int group = 1;
    while (group < 64 && group < g.row_len) group <<= 1;
    const int64_t rows_per_block = (int64_t)kT / group;
    t->off[s] = g.offset;
    t->packfirst[s] = packed;
    t->rows[s] = (int)g.rows;
    t->len[s] = (int)g.row_len;
    t->rowfirst[s] = (int)rows;
    t->group[s] = group;
    t->first[s] = (int)blocks;
    rows += g.rows;
    packed += g.rows * g.row_len;
    blocks += (g.rows + rows_per_block - 1) / rows_per_block;
    ABD_CHECK(rows < (1LL << 30) && packed < (1LL << 40) && blocks < (1LL << 30), ABD_E_INVALID, "row table too large");
  }
  for (int s = n_seg; s < kMaxSeg; ++s) {
    t->off[s] = end;
    t->rows[s] = t->len[s] = 0;
    t->group[s] = 1;
  }
  for (int s = n_seg; s <= kMaxSeg; ++s) {
    t->packfirst[s] = packed;
    t->rowfirst[s] = (int)rows;
    t->first[s] = (int)blocks;
  }
  t->n = n_seg;
  return ABD_OK;
}

// |a - b|: one fp32 subtraction and a sign clear (torch's (a - b).abs())
__device__ __forceinline__ float absdiff_one(const float* a, const float* b, int64_t i) {
  const float d = b ? a[i] - b[i] : a[i];
  return __builtin_fabsf(d);
}

// row_abs_sums_kernel (tsbd.hip) for two buffers against one original: the same lane groups, the same
// per-lane strided double sums and butterfly, hence the same fp32 row sums bit for bit.
__global__ void __launch_bounds__(kT) nwc_pair_rows_kernel(const float* __restrict__ orig,
                                                           const float* __restrict__ pa,
                                                           const float* __restrict__ pb, RowTab t,
                                                           float* __restrict__ absdiff_a, float* __restrict__ absdiff_b,
                                                           float* __restrict__ sums32_a, float* __restrict__ sums32_b,
                                                           double* __restrict__ sums64, int total_rows) {
  const int bid = blockIdx.x, tid = threadIdx.x;
  int s = 0;
  while (s + 1 < t.n && t.first[s + 1] <= bid) ++s;
  const int group = t.group[s], len = t.len[s];
  const int row = (bid - t.first[s]) * (kT / group) + tid / group;
  const int j = tid & (group - 1);
  const bool live = row < t.rows[s];
  double acc_a = 0.0, acc_b = 0.0;
  if (live) {
    const int64_t src = t.off[s] + (int64_t)row * len;
    const int64_t dst = t.packfirst[s] + (int64_t)row * len;
    for (int e = j; e < len; e += group) {
      const float va = absdiff_one(pa, orig, src + e);
      const float vb = absdiff_one(pb, orig, src + e);
      if (absdiff_a) absdiff_a[dst + e] = va;
      if (absdiff_b) absdiff_b[dst + e] = vb;
      acc_a += (double)va;
      acc_b += (double)vb;
    }
  }
  // lanes of a group share a wave (group divides 64); dead rows carry zeros and write nothing
  for (int o = group >> 1; o > 0; o >>= 1) {
    acc_a += __shfl_xor(acc_a, o, 64);
    acc_b += __shfl_xor(acc_b, o, 64);
  }
  if (live && j == 0) {
    const int r = t.rowfirst[s] + row;
    sums32_a[r] = (float)acc_a;
    sums32_b[r] = (float)acc_b;
    sums64[r] = acc_a;
    sums64[total_rows + r] = acc_b;
  }
}

// Block-wide sum in a fixed order: thread i's value into LDS slot i, then halving strides.
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
