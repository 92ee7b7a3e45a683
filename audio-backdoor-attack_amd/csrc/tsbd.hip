// TSBD (tsbd.py:108-138 train_unlearning, :342-363 neuron weight change, :49-63 zero_reinit_weight and
// the 11-ratio sweep of :365-380; correlation_analysis.py:41-99): the flat-buffer arithmetic around the
// smallcnn passes -- per-row |a - b| sums, the gradient-ascent Adam step, the k-th largest weight change
// of a set of neurons and the re-initialised parameter sets of all ratios -- and the entry point that
// sequences one unlearning batch.  The network pass goes through the public C ABI of smallcnn.hip
// (abd_smallcnn_train_step with do_update = 0); nothing of it is re-implemented.
//
// Every launch is asynchronous on the caller's stream, allocates nothing and copies nothing from the
// host: the row table (at most 32 segments), the row selections (bit-packed) and the ranks k travel as
// kernel arguments.  Reductions run in a fixed order (per-lane strided sums, butterfly inside the
// row's lane group); the only atomics are integer ones (the LDS histograms of the radix select and the
// zeroed-weight count), so equal inputs give bit-equal results.
#include <cmath>

#include "abd_common.h"

namespace {

constexpr int kT = 256;
constexpr int kMaxSeg = ABD_MAX_SEGMENTS;
constexpr int kMaxVar = ABD_MAX_REINIT_VARIANTS;
constexpr int kMaxRows = ABD_MAX_REINIT_ROWS;

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

// ---------------------------------------------------------------- row abs sums
// |a - b|: one fp32 subtraction and a sign clear (torch's (a - b).abs())
__device__ __forceinline__ float absdiff_one(const float* a, const float* b, int64_t i) {
  const float d = b ? a[i] - b[i] : a[i];
  return __builtin_fabsf(d);
}

// A row is summed by `group` adjacent lanes: lane j of the group takes elements j, j + group, ... in
// double, then a butterfly over the group's lanes.  group = 1 (row_len 1) is a copy, group = 4 packs 64
// rows of conv1.weight into one block, group = 64 gives a 256-long row one wave.
__global__ void __launch_bounds__(kT) row_abs_sums_kernel(const float* __restrict__ a, const float* __restrict__ b,
                                                          RowTab t, float* __restrict__ absdiff,
                                                          float* __restrict__ row_sums) {
  const int bid = blockIdx.x, tid = threadIdx.x;
  int s = 0;
  while (s + 1 < t.n && t.first[s + 1] <= bid) ++s;
  const int group = t.group[s], len = t.len[s];
  const int row = (bid - t.first[s]) * (kT / group) + tid / group;
  const int j = tid & (group - 1);
  const bool live = row < t.rows[s];
  double acc = 0.0;
  if (live) {
    const int64_t src = t.off[s] + (int64_t)row * len;
    const int64_t dst = t.packfirst[s] + (int64_t)row * len;
    for (int e = j; e < len; e += group) {
      const float v = absdiff_one(a, b, src + e);
      if (absdiff) absdiff[dst + e] = v;
      acc += (double)v;
    }
  }
  // lanes of a group share a wave (group divides 64); dead rows carry zeros and write nothing
  for (int o = group >> 1; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
  if (live && j == 0) row_sums[t.rowfirst[s] + row] = (float)acc;
}

// ---------------------------------------------------------------- gradient ascent + Adam
struct AscentArgs {
  float* p;
  float* g;
  float* m;
  float* v;
  int64_t n;
  float omb1, beta2, omb2, step_size, bc2_sqrt, eps;
};

// grads <- -grads (what (-loss).backward() leaves in .grad), then smallcnn.hip's adam_elem on it.
// adam_elem is compiled with contraction on; its fused form is spelled out here with contraction off,
// so the store of -g in between cannot make the compiler pick other products to fuse:
//   m = fma(1 - beta1, g - m, m);  v = fma(g, (1 - beta2) g, beta2 v);  p = fma(-step, m / denom, p)
__global__ void __launch_bounds__(kT) ascent_adam_kernel(AscentArgs a) {
#pragma clang fp contract(off)
  for (int64_t i = blockIdx.x * (int64_t)kT + threadIdx.x; i < a.n; i += (int64_t)gridDim.x * kT) {
    const float gi = -a.g[i];
    a.g[i] = gi;
    const float m0 = a.m[i];
    const float dm = gi - m0;
    const float mi = __builtin_fmaf(a.omb1, dm, m0);
    const float vb = a.v[i] * a.beta2;
    const float og = a.omb2 * gi;
    const float vi = __builtin_fmaf(gi, og, vb);
    a.m[i] = mi;
    a.v[i] = vi;
    const float root = sqrtf(vi) / a.bc2_sqrt;
    const float denom = root + a.eps;
    const float q = mi / denom;
    a.p[i] = __builtin_fmaf(-a.step_size, q, a.p[i]);
  }
}

// ---------------------------------------------------------------- re-initialisation
struct Selection {
  uint32_t bits[kMaxVar][kMaxRows / 32];  // bit r of variant v: table row r is among its top neurons
  int64_t k[kMaxVar];
};

__device__ __forceinline__ bool selected(const Selection& sel, int v, int row) {
  return (sel.bits[v][row >> 5] >> (row & 31)) & 1u;
}

// One block per variant: the k-th largest of the selected rows' values by radix select on their bit
// patterns (non-negative floats order like their unsigned patterns), 8 bits per pass from the top.
__global__ void __launch_bounds__(kT) reinit_select_kernel(const float* __restrict__ absdiff, RowTab t, Selection sel,
                                                           float* __restrict__ thr, int64_t* __restrict__ zeroed) {
  __shared__ unsigned hist[256];
  __shared__ unsigned prefix_sm;
  __shared__ unsigned long long k_sm;
  const int v = blockIdx.x, tid = threadIdx.x;
  const uint32_t* bits = reinterpret_cast<const uint32_t*>(absdiff);
  if (tid == 0) {
    prefix_sm = 0u;
    k_sm = (unsigned long long)sel.k[v];
    zeroed[v] = 0;
  }
  for (int shift = 24; shift >= 0; shift -= 8) {
    hist[tid] = 0u;
    __syncthreads();
    const unsigned prefix = prefix_sm;
    const unsigned known = shift == 24 ? 0u : ~0u << (shift + 8);
    for (int s = 0; s < t.n; ++s) {
      const int len = t.len[s];
      const int64_t count = (int64_t)t.rows[s] * len;
      for (int64_t e = tid; e < count; e += kT) {
        if (!selected(sel, v, t.rowfirst[s] + (int)(e / len))) continue;
        const unsigned u = bits[t.packfirst[s] + e];
        if ((u & known) == prefix) atomicAdd(&hist[(u >> shift) & 255u], 1u);
      }
    }
    __syncthreads();
    if (tid == 0) {
      unsigned long long k = k_sm, above = 0;
      int b = 255;
      for (; b > 0; --b) {
        if (above + hist[b] >= k) break;
        above += hist[b];
      }
      k_sm = k - above;
      prefix_sm = prefix | ((unsigned)b << shift);
    }
    __syncthreads();
  }
  if (tid == 0) thr[v] = __uint_as_float(prefix_sm);
}

// out[v][i] = 0 where i lies in a selected row of variant v and its |change| >= thr[v], else params[i]
__global__ void __launch_bounds__(kT) reinit_apply_kernel(const float* __restrict__ params,
                                                          const float* __restrict__ absdiff, RowTab t, Selection sel,
                                                          const float* __restrict__ thr, int64_t n_params,
                                                          float* __restrict__ out, int64_t* __restrict__ zeroed) {
  __shared__ int count_sm;
  const int v = blockIdx.y, tid = threadIdx.x;
  if (tid == 0) count_sm = 0;
  __syncthreads();
  const float limit = thr[v];
  float* o = out + (int64_t)v * n_params;
  int hits = 0;
  for (int64_t i = blockIdx.x * (int64_t)kT + tid; i < n_params; i += (int64_t)gridDim.x * kT) {
    float p = params[i];
    for (int s = 0; s < t.n; ++s) {
      const int64_t e = i - t.off[s];
      if (e < 0) break;  // segments ascend
      if (e >= (int64_t)t.rows[s] * t.len[s]) continue;
      if (selected(sel, v, t.rowfirst[s] + (int)(e / t.len[s])) && absdiff[t.packfirst[s] + e] >= limit) {
        p = 0.0f;
        ++hits;
      }
      break;
    }
    o[i] = p;
  }
  if (hits) atomicAdd(&count_sm, hits);
  __syncthreads();
  if (tid == 0 && count_sm)
    atomicAdd(reinterpret_cast<unsigned long long*>(zeroed + v), (unsigned long long)count_sm);
}

inline unsigned grid_for(int64_t n, int64_t cap) {
  int64_t b = (n + kT - 1) / kT;
  if (b > cap) b = cap;
  return (unsigned)(b < 1 ? 1 : b);
}

}  // namespace

extern "C" {

int abd_row_abs_sums_f32(const float* a, const float* b, const abd_row_segment* table, int n_seg, float* absdiff_out,
                         float* row_sums, abd_stream_t stream) {
  RowTab t;
  if (int rc = make_rowtab(table, n_seg, &t)) return rc;
  ABD_CHECK(a && row_sums, ABD_E_INVALID, "NULL argument");
  row_abs_sums_kernel<<<(unsigned)t.first[n_seg], kT, 0, static_cast<hipStream_t>(stream)>>>(a, b, t, absdiff_out,
                                                                                            row_sums);
  ABD_LAUNCH_CHECK();
  return ABD_OK;
}

size_t abd_smallcnn_unlearn_workspace_bytes(const abd_cnn* net, int64_t batch) {
  if (!net || batch < 1) return 0;
  return abd_smallcnn_workspace_bytes(net, batch);
}

int abd_smallcnn_unlearn_step(abd_cnn* net, const abd_unlearn_args* a, void* workspace, size_t workspace_bytes,
                              abd_stream_t stream) {
  ABD_CHECK(net && a && a->x && a->labels && a->params && a->grads && a->exp_avg && a->exp_avg_sq && a->running,
            ABD_E_INVALID, "NULL argument");
  const int64_t B = a->batch;
  ABD_CHECK(B >= 1, ABD_E_INVALID, "unlearning step needs batch >= 1, got %lld", (long long)B);
  ABD_CHECK(a->adam_step >= 1, ABD_E_INVALID, "adam_step is the 1-based step index, got %lld", (long long)a->adam_step);
  const int64_t n = abd_smallcnn_param_count(net);
  abd_row_segment rec{a->record_offset, a->record_rows, a->record_row_len};
  if (a->record_rows != 0) {
    ABD_CHECK(a->record_abs_sums, ABD_E_INVALID, "record layer without record_abs_sums");
    ABD_CHECK(a->record_rows > 0 && a->record_row_len > 0 && a->record_offset >= 0 &&
                  a->record_rows <= n && a->record_row_len <= n &&
                  a->record_offset + a->record_rows * a->record_row_len <= n,
              ABD_E_INVALID, "record layer (%lld + %lld x %lld) reaches outside the %lld parameters",
              (long long)a->record_offset, (long long)a->record_rows, (long long)a->record_row_len, (long long)n);
  }
  const size_t need = abd_smallcnn_workspace_bytes(net, B);
  ABD_CHECK(workspace && workspace_bytes >= need, ABD_E_WORKSPACE, "workspace too small (%zu < %zu)", workspace_bytes,
            need);
  // 1. forward, loss, backward: the gradient of +loss; metrics get the positive loss and the hits
  abd_train_args t{};
  t.x = a->x;
  t.labels = a->labels;
  t.batch = B;
  t.params = a->params;
  t.grads = a->grads;
  t.running = a->running;
  t.num_batches_tracked = a->num_batches_tracked;
  t.do_update = 0;
  t.mask1_in = a->mask1_in;
  t.mask2_in = a->mask2_in;
  t.mask1_out = a->mask1_out;
  t.mask2_out = a->mask2_out;
  t.seed = a->seed;
  t.counter = a->counter;
  t.row_offset = a->row_offset;
  t.logprobs_out = a->logprobs_out;
  t.metrics = a->metrics;
  t.grad_scale = 1.0f;
  if (int rc = abd_smallcnn_train_step(net, &t, workspace, workspace_bytes, stream)) return rc;
  // 2. grads <- -grads, Adam on it (abd_adam_f32's host constants)
  const double bc1 = 1.0 - pow((double)a->beta1, (double)a->adam_step);
  const double bc2 = 1.0 - pow((double)a->beta2, (double)a->adam_step);
  const AscentArgs aa{a->params, a->grads, a->exp_avg, a->exp_avg_sq, n, (float)(1.0 - (double)a->beta1), a->beta2,
                      (float)(1.0 - (double)a->beta2), (float)((double)a->lr / bc1), (float)sqrt(bc2), a->eps};
  ascent_adam_kernel<<<grid_for(n, 2048), kT, 0, static_cast<hipStream_t>(stream)>>>(aa);
  ABD_LAUNCH_CHECK();
  // 3. the record layer's per-row |grad| sums (sign-invariant)
  if (a->record_rows != 0)
    return abd_row_abs_sums_f32(a->grads, nullptr, &rec, 1, nullptr, a->record_abs_sums, stream);
  return ABD_OK;
}

int abd_reinit_weights_f32(const float* params, int64_t n_params, const float* absdiff, const abd_row_segment* table,
                           int n_seg, const uint8_t* row_select, const int64_t* k, int n_variants, float* out,
                           float* thr, int64_t* zeroed, abd_stream_t stream) {
  RowTab t;
  if (int rc = make_rowtab(table, n_seg, &t)) return rc;
  ABD_CHECK(params && absdiff && row_select && k && out && thr && zeroed, ABD_E_INVALID, "NULL argument");
  ABD_CHECK(n_variants >= 1 && n_variants <= kMaxVar, ABD_E_INVALID, "n_variants must be in [1, %d], got %d", kMaxVar,
            n_variants);
  const int total_rows = t.rowfirst[n_seg];
  ABD_CHECK(total_rows <= kMaxRows, ABD_E_INVALID, "row table has %d rows, at most %d", total_rows, kMaxRows);
  const int last = n_seg - 1;
  ABD_CHECK(n_params >= 1 && t.off[last] + (int64_t)t.rows[last] * t.len[last] <= n_params, ABD_E_INVALID,
            "row table reaches past the %lld parameters", (long long)n_params);
  Selection sel{};
  for (int v = 0; v < n_variants; ++v) {
    int64_t m = 0;
    for (int s = 0; s < n_seg; ++s)
      for (int r = 0; r < t.rows[s]; ++r) {
        const int row = t.rowfirst[s] + r;
        if (!row_select[(size_t)v * total_rows + row]) continue;
        sel.bits[v][row >> 5] |= 1u << (row & 31);
        m += t.len[s];
      }
    ABD_CHECK(m > 0, ABD_E_INVALID, "variant %d selects no row", v);
    ABD_CHECK(k[v] >= 1 && k[v] <= m, ABD_E_INVALID, "variant %d: k = %lld outside [1, %lld]", v, (long long)k[v],
              (long long)m);
    sel.k[v] = k[v];
  }
  hipStream_t s = static_cast<hipStream_t>(stream);
  reinit_select_kernel<<<(unsigned)n_variants, kT, 0, s>>>(absdiff, t, sel, thr, zeroed);
  ABD_LAUNCH_CHECK();
  reinit_apply_kernel<<<dim3(grid_for(n_params, 256), (unsigned)n_variants), kT, 0, s>>>(params, absdiff, t, sel, thr,
                                                                                        n_params, out, zeroed);
  ABD_LAUNCH_CHECK();
  return ABD_OK;
}

}  // extern "C"
