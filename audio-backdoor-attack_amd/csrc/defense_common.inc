// What the four smallcnn defences share (finetune.hip, tsbd.hip, nwc_corr.hip, fineprune.hip): launch
// geometry and alignment helpers, the row table with its row-sum body, the Adam element that follows a
// stored gradient, the abd_train_args of a no-update pass, and the argument checks.  Included inside each
// file's anonymous namespace, after abd_common.h (one of the benchmarked step's hashed sources, which is
// why none of this lives there).
//
// Kept apart on purpose: block_sum_d (finetune.hip: wave butterflies, then the waves in index order) and
// block_sum (nwc_corr.hip: halving strides over LDS) add in different orders, so one of them for both
// would change bits; abl_reduce_kernel belongs to ablate.hip, which compiles smallcnn.hip whole.

constexpr int kT = 256;
constexpr int kMaxSeg = ABD_MAX_SEGMENTS;

inline unsigned grid_for(int64_t n, int64_t cap) {
  int64_t b = (n + kT - 1) / kT;
  if (b > cap) b = cap;
  return (unsigned)(b < 1 ? 1 : b);
}

inline size_t round256(size_t b) { return (b + 255) & ~(size_t)255; }

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

// ---------------------------------------------------------------- argument checks
inline int check_workspace(const void* workspace, size_t workspace_bytes, size_t need) {
  ABD_CHECK(workspace && workspace_bytes >= need, ABD_E_WORKSPACE, "workspace too small (%zu < %zu)", workspace_bytes,
            need);
  return ABD_OK;
}

// what: "unlearning step", "fine-tuning step"
inline int check_batch(const char* what, int64_t batch) {
  ABD_CHECK(batch >= 1, ABD_E_INVALID, "%s needs batch >= 1, got %lld", what, (long long)batch);
  return ABD_OK;
}

inline int check_adam_batch(const char* what, int64_t batch, int64_t adam_step) {
  if (int rc = check_batch(what, batch)) return rc;
  ABD_CHECK(adam_step >= 1, ABD_E_INVALID, "adam_step is the 1-based step index, got %lld", (long long)adam_step);
  return ABD_OK;
}

// ---------------------------------------------------------------- block -> segment
// first[s] .. first[s + 1] are the blocks of segment s of n (RowTab below, finetune.hip's SegTab)
__device__ __forceinline__ int segment_of(const int* first, int n, int bid) {
  int s = 0;
  while (s + 1 < n && first[s + 1] <= bid) ++s;
  return s;
}

// ---------------------------------------------------------------- row table
// Segment s: rows[s] rows of len[s] floats from element off[s] of the flat buffer.  Its rows are
// rows rowfirst[s].. of the table, its values start at packfirst[s] of the packed |a - b| buffer.
// In the row-sum kernels a row is handled by group[s] lanes (a power of two <= 64) and the segment by
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

// The row sums of NB buffers a[0..NB) against one b (NULL: the buffers themselves).  A row is summed by
// `group` adjacent lanes: lane j of the group takes elements j, j + group, ... in double, then a butterfly
// over the group's lanes.  group = 1 (row_len 1) is a copy, group = 4 packs 64 rows of conv1.weight into
// one block, group = 64 gives a 256-long row one wave.  absdiff[k] (or NULL) receives buffer k's packed
// rows.  Returns the table row whose sums this lane holds in acc[0..NB) (lane 0 of a live row's group),
// else -1.
template <int NB>
__device__ __forceinline__ int row_abs_sums_body(const RowTab& t, const float* const (&a)[NB], const float* b,
                                                 float* const (&absdiff)[NB], double (&acc)[NB]) {
  const int bid = blockIdx.x, tid = threadIdx.x;
  const int s = segment_of(t.first, t.n, bid);
  const int group = t.group[s], len = t.len[s];
  const int row = (bid - t.first[s]) * (kT / group) + tid / group;
  const int j = tid & (group - 1);
  const bool live = row < t.rows[s];
#pragma unroll
  for (int k = 0; k < NB; ++k) acc[k] = 0.0;
  if (live) {
    const int64_t src = t.off[s] + (int64_t)row * len;
    const int64_t dst = t.packfirst[s] + (int64_t)row * len;
    for (int e = j; e < len; e += group) {
      float v[NB];
#pragma unroll
      for (int k = 0; k < NB; ++k) v[k] = absdiff_one(a[k], b, src + e);
#pragma unroll
      for (int k = 0; k < NB; ++k)
        if (absdiff[k]) absdiff[k][dst + e] = v[k];
#pragma unroll
      for (int k = 0; k < NB; ++k) acc[k] += (double)v[k];
    }
  }
  // lanes of a group share a wave (group divides 64); dead rows carry zeros and write nothing
  for (int o = group >> 1; o > 0; o >>= 1) {
#pragma unroll
    for (int k = 0; k < NB; ++k) acc[k] += __shfl_xor(acc[k], o, 64);
  }
  return live && j == 0 ? t.rowfirst[s] + row : -1;
}

// ---------------------------------------------------------------- Adam on a stored gradient
struct AdamConsts {
  float omb1, beta2, omb2, step_size, bc2_sqrt, eps;
};

// abd_adam_f32's host constants
inline AdamConsts adam_consts(float lr, float beta1, float beta2, float eps, int64_t adam_step) {
  const double bc1 = 1.0 - pow((double)beta1, (double)adam_step);
  const double bc2 = 1.0 - pow((double)beta2, (double)adam_step);
  return AdamConsts{(float)(1.0 - (double)beta1), beta2, (float)(1.0 - (double)beta2), (float)((double)lr / bc1),
                    (float)sqrt(bc2), eps};
}

// smallcnn.hip's adam_elem on element i for a gradient gi that the caller has just changed and stored.
// adam_elem is compiled with contraction on; its fused form is spelled out here with contraction off, so
// the store of gi in between cannot make the compiler pick other products to fuse:
//   m = fma(1 - beta1, g - m, m);  v = fma(g, (1 - beta2) g, beta2 v);  p = fma(-step, m / denom, p)
__device__ __forceinline__ void adam_elem_stored(float gi, const AdamConsts& c, float* m, float* v, float* p,
                                                 int64_t i) {
#pragma clang fp contract(off)
  const float m0 = m[i];
  const float dm = gi - m0;
  const float mi = __builtin_fmaf(c.omb1, dm, m0);
  const float vb = v[i] * c.beta2;
  const float og = c.omb2 * gi;
  const float vi = __builtin_fmaf(gi, og, vb);
  m[i] = mi;
  v[i] = vi;
  const float root = sqrtf(vi) / c.bc2_sqrt;
  const float denom = root + c.eps;
  const float q = mi / denom;
  p[i] = __builtin_fmaf(-c.step_size, q, p[i]);
}

// ---------------------------------------------------------------- a no-update smallcnn pass
// The abd_train_args of "one train step without an update" (do_update = 0, grad_scale = 1) from a defence's
// argument struct; the three structs name their common fields alike.  abd_unlearn_args and
// abd_pruned_finetune_args carry one mask set and metrics.  abd_finetune_reg_args carries a mask set per
// pass and no metrics: pass k takes slice k and counter + k, and says where its parameters, gradient, BN
// buffers and log-probs live.
template <class A>
abd_train_args no_update_args(const A& a, int k, float* params, float* grads, float* running,
                              int64_t* num_batches_tracked, float* logprobs_out) {
  abd_train_args t{};
  t.x = a.x;
  t.labels = a.labels;
  t.batch = a.batch;
  t.params = params;
  t.grads = grads;
  t.running = running;
  t.num_batches_tracked = num_batches_tracked;
  t.do_update = 0;
  t.seed = a.seed;
  t.counter = a.counter + (uint64_t)k;
  t.row_offset = a.row_offset;
  t.logprobs_out = logprobs_out;
  t.grad_scale = 1.0f;
  if constexpr (std::is_array_v<decltype(a.mask1_in)>) {
    t.mask1_in = a.mask1_in[k];
    t.mask2_in = a.mask2_in[k];
    t.mask1_out = a.mask1_out[k];
    t.mask2_out = a.mask2_out[k];
  } else {
    t.mask1_in = a.mask1_in;
    t.mask2_in = a.mask2_in;
    t.mask1_out = a.mask1_out;
    t.mask2_out = a.mask2_out;
    t.metrics = a.metrics;
  }
  return t;
}

template <class A>
abd_train_args no_update_args(const A& a) {
  return no_update_args(a, 0, a.params, a.grads, a.running, a.num_batches_tracked, a.logprobs_out);
}
