// Regularised fine-tuning (ft_reg.py:83-123 train_finetuning_reg, :57-81 train_finetuning): the
// flat-buffer arithmetic between the smallcnn passes -- per-tensor L2 norms, the parameter
// displacement, torch.optim.SGD with momentum, loss / accuracy of a log-prob batch -- and the entry
// point that sequences one batch.  The network passes go through the public C ABI of smallcnn.hip
// (abd_smallcnn_train_step with do_update = 0, abd_smallcnn_forward); nothing of it is re-implemented.
//
// Every launch is asynchronous on the caller's stream, allocates nothing and copies nothing from the
// host: the segment table (at most 32 offsets) travels as a kernel argument.  Element offsets are
// 64-bit.  Reductions run in a fixed order (per-thread strided sums, wave butterfly, waves in index
// order), no floating-point atomics, so equal inputs give bit-equal results.
#include <cmath>
#include <type_traits>

#include "abd_common.h"

namespace {

using abd::wave_sum_d;

// kT, kMaxSeg, round256, aligned16, segment_of, no_update_args, checks
#include "defense_common.inc"

constexpr int64_t kChunk = 4096;  // elements of one segment per block (16 per thread, 4 float4)

// Segment s is [off[s], off[s + 1]) and is covered by blocks [first[s], first[s + 1]), kChunk
// elements each (the last one shorter): a block never straddles two segments.
struct SegTab {
  int64_t off[kMaxSeg + 1];
  int first[kMaxSeg + 1];
  int n;
};

int make_segtab(const int64_t* offsets, int n_seg, SegTab* t) {
  ABD_CHECK(offsets != nullptr, ABD_E_INVALID, "NULL segment offsets");
  ABD_CHECK(n_seg >= 1 && n_seg <= kMaxSeg, ABD_E_INVALID, "n_seg must be in [1, %d], got %d", kMaxSeg, n_seg);
  ABD_CHECK(offsets[0] >= 0, ABD_E_INVALID, "negative segment offset");
  int64_t blocks = 0;
  for (int s = 0; s < n_seg; ++s) {
    const int64_t len = offsets[s + 1] - offsets[s];
    ABD_CHECK(len > 0, ABD_E_INVALID, "segment %d is empty or descending (%lld .. %lld)", s, (long long)offsets[s],
              (long long)offsets[s + 1]);
    t->off[s] = offsets[s];
    t->first[s] = (int)blocks;
    blocks += (len + kChunk - 1) / kChunk;
    ABD_CHECK(blocks < (1LL << 31), ABD_E_INVALID, "segments too long (block index exceeds int32)");
  }
  t->off[n_seg] = offsets[n_seg];
  t->first[n_seg] = (int)blocks;
  for (int s = n_seg + 1; s <= kMaxSeg; ++s) {
    t->off[s] = offsets[n_seg];
    t->first[s] = (int)blocks;
  }
  t->n = n_seg;
  return ABD_OK;
}

// A block's slice of its segment, split for 16-byte vector access relative to `ref`'s address:
// [0, head) scalars, nvec float4 from head, then [tail, len) scalars.  head, len - tail <= 3.
struct Slice {
  int64_t begin, len, head, nvec, tail;
};

__device__ __forceinline__ Slice slice_of(const SegTab& t, int s, int bid, const float* ref, bool vec) {
  Slice c;
  c.begin = t.off[s] + (int64_t)(bid - t.first[s]) * kChunk;
  const int64_t end = c.begin + kChunk < t.off[s + 1] ? c.begin + kChunk : t.off[s + 1];
  c.len = end - c.begin;
  if (!vec) {
    c.head = c.len;
    c.nvec = 0;
    c.tail = c.len;
    return c;
  }
  const uintptr_t addr = reinterpret_cast<uintptr_t>(ref + c.begin);
  c.head = (int64_t)(((16u - (unsigned)(addr & 15u)) & 15u) >> 2);
  if (c.head > c.len) c.head = c.len;
  c.nvec = (c.len - c.head) >> 2;
  c.tail = c.head + 4 * c.nvec;
  return c;
}

// Sum over the block in a fixed order (wave butterflies, then the waves in index order); the result is
// valid in thread 0.  Not nwc_corr.hip's block_sum, which adds in another order.
__device__ __forceinline__ double block_sum_d(double v, double* sm) {
  v = wave_sum_d(v);
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) sm[wave] = v;
  __syncthreads();
  double total = 0.0;
  if (threadIdx.x == 0)
    for (int i = 0; i < kT / 64; ++i) total += sm[i];
  return total;
}

// ---------------------------------------------------------------- segment norms
__global__ void __launch_bounds__(kT) seg_sumsq_kernel(const float* __restrict__ buf, SegTab t,
                                                       double* __restrict__ part) {
  __shared__ double sm[kT / 64];
  const int bid = blockIdx.x, tid = threadIdx.x;
  const int s = segment_of(t.first, t.n, bid);
  const Slice c = slice_of(t, s, bid, buf, true);
  const float* q = buf + c.begin;
  double acc = 0.0;
  for (int64_t i = tid; i < c.head; i += kT) {
    const double v = q[i];
    acc += v * v;
  }
  const float4* q4 = reinterpret_cast<const float4*>(q + c.head);
  for (int64_t i = tid; i < c.nvec; i += kT) {
    const float4 v = q4[i];
    acc += (double)v.x * v.x;
    acc += (double)v.y * v.y;
    acc += (double)v.z * v.z;
    acc += (double)v.w * v.w;
  }
  for (int64_t i = c.tail + tid; i < c.len; i += kT) {
    const double v = q[i];
    acc += v * v;
  }
  const double total = block_sum_d(acc, sm);
  if (tid == 0) part[bid] = total;
}

__global__ void __launch_bounds__(kT) seg_norm_kernel(const double* __restrict__ part, SegTab t,
                                                      float* __restrict__ norms) {
  __shared__ double sm[kT / 64];
  const int s = blockIdx.x;
  const int b = t.first[s], e = t.first[s + 1];
  double acc = 0.0;
  for (int i = b + (int)threadIdx.x; i < e; i += kT) acc += part[i];
  const double total = block_sum_d(acc, sm);
  if (threadIdx.x == 0) norms[s] = (float)sqrt(total);
}

// ---------------------------------------------------------------- perturb
// param.data += r * (grad / grad.norm()): three separately rounded fp32 operations
__device__ __forceinline__ float perturb_one(float p, float g, float norm, float r) {
#pragma clang fp contract(off)
  const float q = g / norm;
  const float d = r * q;
  return p + d;
}

__global__ void __launch_bounds__(kT) perturb_kernel(const float* p, const float* g, const float* __restrict__ norms,
                                                     SegTab t, float r, float* out, int vec) {
  const int bid = blockIdx.x, tid = threadIdx.x;
  const int s = segment_of(t.first, t.n, bid);
  const Slice c = slice_of(t, s, bid, out, vec != 0);
  const float norm = norms[s];
  const float* pp = p + c.begin;
  const float* gg = g + c.begin;
  float* oo = out + c.begin;
  for (int64_t i = tid; i < c.head; i += kT) oo[i] = perturb_one(pp[i], gg[i], norm, r);
  const float4* p4 = reinterpret_cast<const float4*>(pp + c.head);
  const float4* g4 = reinterpret_cast<const float4*>(gg + c.head);
  float4* o4 = reinterpret_cast<float4*>(oo + c.head);
  for (int64_t i = tid; i < c.nvec; i += kT) {
    const float4 a = p4[i], b = g4[i];
    float4 o;
    o.x = perturb_one(a.x, b.x, norm, r);
    o.y = perturb_one(a.y, b.y, norm, r);
    o.z = perturb_one(a.z, b.z, norm, r);
    o.w = perturb_one(a.w, b.w, norm, r);
    o4[i] = o;
  }
  for (int64_t i = c.tail + tid; i < c.len; i += kT) oo[i] = perturb_one(pp[i], gg[i], norm, r);
}

// ---------------------------------------------------------------- SGD
struct SgdArgs {
  float* p;
  const float* g;
  const float* g2;
  float* buf;
  float* gout;
  int64_t n;
  float one_minus_alpha, alpha, mu, lr;
};

// buf.mul_(momentum).add_(d); param.add_(buf, alpha=-lr) -- each operation rounded on its own
__device__ __forceinline__ void sgd_one(float& p, float g, float g2, float& buf, float& d, const SgdArgs& a) {
#pragma clang fp contract(off)
  d = g;
  if (a.g2) {
    const float t1 = a.one_minus_alpha * g;
    const float t2 = a.alpha * g2;
    d = t1 + t2;
  }
  float step = d;
  if (a.buf) {
    const float mb = a.mu * buf;
    buf = mb + d;
    step = buf;
  }
  const float ls = a.lr * step;
  p = p - ls;
}

template <bool VEC>
__global__ void __launch_bounds__(kT) sgd_kernel(SgdArgs a) {
  const int64_t stride = (int64_t)gridDim.x * kT;
  const int64_t t0 = (int64_t)blockIdx.x * kT + threadIdx.x;
  if (VEC) {
    const int64_t nvec = a.n >> 2;
    for (int64_t i = t0; i < nvec; i += stride) {
      float4 p = reinterpret_cast<float4*>(a.p)[i];
      const float4 g = reinterpret_cast<const float4*>(a.g)[i];
      float4 g2 = make_float4(0.f, 0.f, 0.f, 0.f), b = g2, d;
      if (a.g2) g2 = reinterpret_cast<const float4*>(a.g2)[i];
      if (a.buf) b = reinterpret_cast<float4*>(a.buf)[i];
      sgd_one(p.x, g.x, g2.x, b.x, d.x, a);
      sgd_one(p.y, g.y, g2.y, b.y, d.y, a);
      sgd_one(p.z, g.z, g2.z, b.z, d.z, a);
      sgd_one(p.w, g.w, g2.w, b.w, d.w, a);
      reinterpret_cast<float4*>(a.p)[i] = p;
      if (a.buf) reinterpret_cast<float4*>(a.buf)[i] = b;
      if (a.gout) reinterpret_cast<float4*>(a.gout)[i] = d;
    }
  }
  for (int64_t i = (VEC ? (a.n & ~(int64_t)3) : 0) + t0; i < a.n; i += stride) {
    float p = a.p[i], b = a.buf ? a.buf[i] : 0.f, d;
    sgd_one(p, a.g[i], a.g2 ? a.g2[i] : 0.f, b, d, a);
    a.p[i] = p;
    if (a.buf) a.buf[i] = b;
    if (a.gout) a.gout[i] = d;
  }
}

// ---------------------------------------------------------------- loss / accuracy of a log-prob batch
// nn.CrossEntropyLoss()(logp, labels) (mean over the rows of -log_softmax(logp)[label]) and
// logp.max(1)[1] == labels (first maximum), in double; one block, rows strided over its threads.
__global__ void __launch_bounds__(kT) ce_accuracy_kernel(const float* __restrict__ logp,
                                                         const int64_t* __restrict__ labels, int64_t B, int K,
                                                         double* loss_sum, int64_t* correct) {
  __shared__ double sm[kT / 64];
  __shared__ int hits_sm[kT];
  const int tid = threadIdx.x;
  double acc = 0.0;
  int hits = 0;
  for (int64_t row = tid; row < B; row += kT) {
    const float* lp = logp + row * K;
    float m = lp[0];
    int arg = 0;
    for (int k = 1; k < K; ++k)
      if (lp[k] > m) {
        m = lp[k];
        arg = k;
      }
    double se = 0.0;
    for (int k = 0; k < K; ++k) se += exp((double)lp[k] - (double)m);
    const int64_t y = labels[row];
    const bool ok = y >= 0 && y < K;
    acc += ok ? -((double)lp[ok ? y : 0] - (double)m - log(se)) : (double)NAN;
    hits += (ok && arg == (int)y) ? 1 : 0;
  }
  hits_sm[tid] = hits;
  const double total = block_sum_d(acc, sm);  // its barrier also publishes hits_sm
  if (tid == 0) {
    int64_t h = 0;
    for (int i = 0; i < kT; ++i) h += hits_sm[i];
    *loss_sum += total / (double)B;
    *correct += h;
  }
}

// The composite's workspace: the smallcnn workspace first, then the flat buffers it adds.
struct RegWork {
  char* cnn;
  size_t cnn_bytes;
  float *g1, *moved, *running, *norms, *logp;
  double* part;
  size_t part_bytes, bytes;
};

RegWork reg_layout(const abd_cnn* net, int64_t B, const int64_t* off, char* base) {
  RegWork w{};
  const int64_t n = off[16];
  const int64_t K = off[16] - off[15];
  size_t o = 0;
  auto take = [&](size_t bytes) {
    char* p = base ? base + o : nullptr;
    o += round256(bytes);
    return p;
  };
  w.cnn_bytes = abd_smallcnn_workspace_bytes(net, B);
  w.cnn = take(w.cnn_bytes);
  w.g1 = reinterpret_cast<float*>(take((size_t)n * 4));
  w.moved = reinterpret_cast<float*>(take((size_t)n * 4));
  w.running = reinterpret_cast<float*>(take(320 * 4));
  w.norms = reinterpret_cast<float*>(take(kMaxSeg * 4));
  w.part_bytes = abd_segment_norms_workspace_bytes(off, 16);
  w.part = reinterpret_cast<double*>(take(w.part_bytes));
  w.logp = reinterpret_cast<float*>(take((size_t)B * (size_t)K * 4));
  w.bytes = o;
  return w;
}

}  // namespace

extern "C" {

size_t abd_segment_norms_workspace_bytes(const int64_t* offsets, int n_seg) {
  SegTab t;
  if (make_segtab(offsets, n_seg, &t)) return 0;
  return (size_t)t.first[n_seg] * sizeof(double);
}

int abd_segment_norms_f32(const float* buf, const int64_t* offsets, int n_seg, float* norms, void* workspace,
                          size_t workspace_bytes, abd_stream_t stream) {
  SegTab t;
  if (int rc = make_segtab(offsets, n_seg, &t)) return rc;
  ABD_CHECK(buf && norms, ABD_E_INVALID, "NULL argument");
  const size_t need = (size_t)t.first[n_seg] * sizeof(double);
  if (int rc = check_workspace(workspace, workspace_bytes, need)) return rc;
  ABD_CHECK((reinterpret_cast<uintptr_t>(workspace) & 7u) == 0, ABD_E_INVALID, "workspace must be 8-byte aligned");
  hipStream_t s = static_cast<hipStream_t>(stream);
  double* part = static_cast<double*>(workspace);
  seg_sumsq_kernel<<<(unsigned)t.first[n_seg], kT, 0, s>>>(buf, t, part);
  ABD_LAUNCH_CHECK();
  seg_norm_kernel<<<(unsigned)n_seg, kT, 0, s>>>(part, t, norms);
  ABD_LAUNCH_CHECK();
  return ABD_OK;
}

int abd_perturb_f32(const float* p, const float* g, const float* norms, const int64_t* offsets, int n_seg, float r,
                    float* out, abd_stream_t stream) {
  SegTab t;
  if (int rc = make_segtab(offsets, n_seg, &t)) return rc;
  ABD_CHECK(p && g && norms && out, ABD_E_INVALID, "NULL argument");
  ABD_CHECK(out != p && out != g, ABD_E_INVALID, "perturb output may not alias its inputs");
  // vector access needs the three buffers equally placed inside a 16-byte line
  const uintptr_t mp = reinterpret_cast<uintptr_t>(p) & 15u, mg = reinterpret_cast<uintptr_t>(g) & 15u,
                  mo = reinterpret_cast<uintptr_t>(out) & 15u;
  const int vec = (mp == mg && mg == mo) ? 1 : 0;
  perturb_kernel<<<(unsigned)t.first[n_seg], kT, 0, static_cast<hipStream_t>(stream)>>>(p, g, norms, t, r, out, vec);
  ABD_LAUNCH_CHECK();
  return ABD_OK;
}

int abd_sgd_f32(float* p, const float* g, const float* g2, float alpha, float* buf, float momentum, float lr,
                float* grad_out, int64_t n, abd_stream_t stream) {
  ABD_CHECK(p && g, ABD_E_INVALID, "NULL argument");
  ABD_CHECK(n >= 0, ABD_E_INVALID, "negative element count");
  ABD_CHECK(buf != nullptr || momentum == 0.0f, ABD_E_INVALID, "momentum %g needs a momentum buffer", (double)momentum);
  if (n == 0) return ABD_OK;
  const SgdArgs a{p, g, g2, momentum != 0.0f ? buf : nullptr, grad_out, n, (float)(1.0 - (double)alpha), alpha,
                  momentum, lr};
  const bool vec = aligned16(p) && aligned16(g) && (!g2 || aligned16(g2)) && (!a.buf || aligned16(a.buf)) &&
                   (!grad_out || aligned16(grad_out));
  const int64_t per_block = (int64_t)kT * (vec ? 4 : 1);
  int64_t blocks = (n + per_block - 1) / per_block;
  if (blocks > 2048) blocks = 2048;
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (vec)
    sgd_kernel<true><<<(unsigned)blocks, kT, 0, s>>>(a);
  else
    sgd_kernel<false><<<(unsigned)blocks, kT, 0, s>>>(a);
  ABD_LAUNCH_CHECK();
  return ABD_OK;
}

size_t abd_smallcnn_finetune_reg_workspace_bytes(const abd_cnn* net, int64_t batch) {
  if (!net || batch < 1) return 0;
  int64_t off[17];
  if (abd_smallcnn_param_offsets(net, off)) return 0;
  return reg_layout(net, batch, off, nullptr).bytes;
}

int abd_smallcnn_finetune_reg_step(abd_cnn* net, const abd_finetune_reg_args* a, void* workspace,
                                   size_t workspace_bytes, abd_stream_t stream) {
  ABD_CHECK(net && a && a->x && a->labels && a->params && a->grads && a->running && a->loss_sum && a->correct,
            ABD_E_INVALID, "NULL argument");
  const int64_t B = a->batch;
  if (int rc = check_batch("fine-tuning step", B)) return rc;
  ABD_CHECK(a->momentum_buf != nullptr || a->momentum == 0.0f, ABD_E_INVALID, "momentum %g needs a momentum buffer",
            (double)a->momentum);
  int64_t off[17];
  if (int rc = abd_smallcnn_param_offsets(net, off)) return rc;
  const int64_t n = off[16];
  const int K = (int)(off[16] - off[15]);
  ABD_CHECK((reinterpret_cast<uintptr_t>(workspace) & 255u) == 0, ABD_E_INVALID, "workspace must be 256-byte aligned");
  const RegWork w = reg_layout(net, B, off, static_cast<char*>(workspace));
  if (int rc = check_workspace(workspace, workspace_bytes, w.bytes)) return rc;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const size_t lp_elems = (size_t)B * (size_t)K;

  // forwards 1 and 2 run on the reference's discarded copy: their BN statistics update a scratch copy
  ABD_HIP(hipMemcpyAsync(w.running, a->running, 320 * sizeof(float), hipMemcpyDeviceToDevice, s));
  // 1. g1 at params
  abd_train_args t = no_update_args(*a, 0, a->params, w.g1, w.running, nullptr, a->logprobs_out);
  if (int rc = abd_smallcnn_train_step(net, &t, w.cnn, w.cnn_bytes, stream)) return rc;
  // 2. the displaced parameters
  if (int rc = abd_segment_norms_f32(w.g1, off, 16, w.norms, w.part, w.part_bytes, stream)) return rc;
  if (int rc = abd_perturb_f32(a->params, w.g1, w.norms, off, 16, a->r, w.moved, stream)) return rc;
  // 3. g2 at the displaced parameters, into grads
  t = no_update_args(*a, 1, w.moved, a->grads, w.running, nullptr,
                     a->logprobs_out ? a->logprobs_out + lp_elems : nullptr);
  if (int rc = abd_smallcnn_train_step(net, &t, w.cnn, w.cnn_bytes, stream)) return rc;
  // 4. SGD on the real parameters; grads <- (1 - alpha) g1 + alpha g2
  if (int rc = abd_sgd_f32(a->params, w.g1, a->grads, a->alpha, a->momentum_buf, a->momentum, a->lr, a->grads, n,
                           stream))
    return rc;
  // 5. the reference's third forward: the only one that touches the real BN buffers
  float* lp3 = a->logprobs_out ? a->logprobs_out + 2 * lp_elems : w.logp;
  t = no_update_args(*a, 2, a->params, nullptr, a->running, a->num_batches_tracked, lp3);
  if (int rc = abd_smallcnn_forward(net, &t, 1, w.cnn, w.cnn_bytes, stream)) return rc;
  // 6. loss / accuracy of that forward
  ce_accuracy_kernel<<<1, kT, 0, s>>>(lp3, a->labels, B, K, a->loss_sum, a->correct);
  ABD_LAUNCH_CHECK();
  return ABD_OK;
}

}  // extern "C"
