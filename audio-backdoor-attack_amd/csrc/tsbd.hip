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
#include <type_traits>

#include "abd_common.h"

namespace {

// kT, grid_for, RowTab / make_rowtab / row_abs_sums_body, AdamConsts / adam_elem_stored, no_update_args, checks
#include "defense_common.inc"

constexpr int kMaxVar = ABD_MAX_REINIT_VARIANTS;
constexpr int kMaxRows = ABD_MAX_REINIT_ROWS;

// ---------------------------------------------------------------- row abs sums
__global__ void __launch_bounds__(kT) row_abs_sums_kernel(const float* __restrict__ a, const float* __restrict__ b,
                                                          RowTab t, float* __restrict__ absdiff,
                                                          float* __restrict__ row_sums) {
  const float* const as[1] = {a};
  float* const ad[1] = {absdiff};
  double acc[1];
  const int r = row_abs_sums_body<1>(t, as, b, ad, acc);
  if (r >= 0) row_sums[r] = (float)acc[0];
}

// ---------------------------------------------------------------- gradient ascent + Adam
struct AscentArgs {
  float* p;
  float* g;
  float* m;
  float* v;
  int64_t n;
  AdamConsts c;
};

// grads <- -grads (what (-loss).backward() leaves in .grad), then Adam on it
__global__ void __launch_bounds__(kT) ascent_adam_kernel(AscentArgs a) {
  for (int64_t i = blockIdx.x * (int64_t)kT + threadIdx.x; i < a.n; i += (int64_t)gridDim.x * kT) {
    const float gi = -a.g[i];
    a.g[i] = gi;
    adam_elem_stored(gi, a.c, a.m, a.v, a.p, i);
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
  if (int rc = check_adam_batch("unlearning step", B, a->adam_step)) return rc;
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
  if (int rc = check_workspace(workspace, workspace_bytes, abd_smallcnn_workspace_bytes(net, B))) return rc;
  // 1. forward, loss, backward: the gradient of +loss; metrics get the positive loss and the hits
  const abd_train_args t = no_update_args(*a);
  if (int rc = abd_smallcnn_train_step(net, &t, workspace, workspace_bytes, stream)) return rc;
  // 2. grads <- -grads, Adam on it
  const AscentArgs aa{a->params, a->grads, a->exp_avg, a->exp_avg_sq, n,
                      adam_consts(a->lr, a->beta1, a->beta2, a->eps, a->adam_step)};
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
