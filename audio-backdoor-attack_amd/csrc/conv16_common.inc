// What the two implicit-GEMM conv nets with BatchNorm (resnet.hip, smalllstm.hip) share: the 16x16x4 tile product
// of a 16-wide K-step, the weight-gradient slab sum, the BatchNorm partial-block plan and the four ABI entries of a
// net with running statistics.  Included after net_common.inc and the file's kT, kStatRows, kStatBlocks and P_COUNT.
// The conv_kernels and the BatchNorm kernels differ between the files and stay there.

typedef float f4v __attribute__((ext_vector_type(4)));

// ------------------------------------------------------------------ the 16x16x4 tile product
// As: (block rows) x BK, pitch BK + 1; Bs: BK x (16 TN), pitch ldb.  The wave at rows wm..wm+15 adds the K-step to
// its TN accumulators.  Operand lanes: A[row lane & 15][k lane >> 4], B[k lane >> 4][col lane & 15]; acc[r] is row
// 4 (lane >> 4) + r, col lane & 15.
template <int TN, int BK>
__device__ __forceinline__ void tile_mfma(const float* As, const float* Bs, int ldb, int wm, int lane, f4v (&acc)[TN]) {
#pragma unroll
  for (int kk = 0; kk < BK / 4; ++kk) {
    const int k = kk * 4 + (lane >> 4);
    const float av = As[(wm + (lane & 15)) * (BK + 1) + k];
#pragma unroll
    for (int j = 0; j < TN; ++j)
      acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, Bs[k * ldb + j * 16 + (lane & 15)], acc[j], 0, 0, 0);
  }
}

// dw (Cout, Cin, TAPS) = the sum over slices, in slice order, of slab (slice, tap, Cin, Cout)
template <int TAPS>
__global__ void __launch_bounds__(kT) wgrad_reduce_kernel(const float* slab, int slices, int Cout, int Cin, float* dw) {
  const int e = blockIdx.x * kT + threadIdx.x;
  const int per = TAPS * Cout * Cin;
  if (e >= per) return;
  double s = 0.0;
  for (int z = 0; z < slices; ++z) s += (double)slab[(int64_t)z * per + e];
  const int co = e % Cout, ci = (e / Cout) % Cin, tap = e / (Cout * Cin);
  dw[((int64_t)co * Cin + ci) * TAPS + tap] = (float)s;
}

// ------------------------------------------------------------------ host side
inline unsigned blocks(int64_t n) { return (unsigned)((n + kT - 1) / kT); }

// a BatchNorm reduction over `pixels` pixels: nb partial blocks of chunk pixels each
struct StatPlan {
  int nb;
  int64_t chunk;
};
StatPlan stat_plan(int64_t pixels) {
  StatPlan p;
  p.nb = (int)std::max<int64_t>(1, std::min<int64_t>(kStatBlocks, (pixels + kStatRows - 1) / kStatRows));
  p.chunk = (pixels + p.nb - 1) / p.nb;
  return p;
}

// ------------------------------------------------------------------ the ABI of a net with running statistics
// abd_<net>_forward / _backward / _train_step / _eval forward here.  The file gives, in this namespace: Ctx (with
// members running: NULL leaves the running statistics alone, and nbt), make_ctx(net, B, params, grads, ws, bytes,
// stream, Ctx*), run_forward(c, x, train, the call's args struct or NULL) and run_backward(c, x, dlogits).
template <class Net, class Ctx>
int make_stat_ctx(const Net* net, int64_t B, const float* params, float* grads, float* running, int64_t* nbt,
                  void* ws, size_t bytes, abd_stream_t stream, Ctx* c) {
  if (int rc = make_ctx(net, B, params, grads, ws, bytes, stream, c)) return rc;
  c->running = running;
  c->nbt = nbt;
  return ABD_OK;
}

template <class Ctx, class Net, class Args>
int stat_net_forward(Net* net, const Args* a, int train_mode, void* workspace, size_t workspace_bytes,
                     abd_stream_t stream) {
  ABD_CHECK(a != nullptr && a->x, ABD_E_INVALID, "NULL x");
  ABD_CHECK(train_mode || a->running, ABD_E_INVALID, "an eval forward needs the running statistics");
  Ctx c;
  if (int rc = make_stat_ctx(net, a->batch, a->params, a->grads, a->running,
                             train_mode ? a->num_batches_tracked : nullptr, workspace, workspace_bytes, stream, &c))
    return rc;
  if (int rc = run_forward(c, a->x, train_mode ? 1 : 0, a)) return rc;
  return run_ce(c, nullptr, nullptr, false, 1.0f, a->logits_out, nullptr);
}

template <class Ctx, class Net, class Args>
int stat_net_backward(Net* net, const Args* a, const float* dlogits, void* workspace, size_t workspace_bytes,
                      abd_stream_t stream) {
  ABD_CHECK(a != nullptr && a->x && a->grads && dlogits, ABD_E_INVALID, "NULL x / grads / dlogits");
  Ctx c;
  if (int rc = make_stat_ctx(net, a->batch, a->params, a->grads, nullptr, nullptr, workspace, workspace_bytes, stream,
                             &c))
    return rc;
  return run_backward(c, a->x, dlogits);
}

template <class Ctx, class Net, class Args>
int stat_net_train_step(Net* net, const Args* a, void* workspace, size_t workspace_bytes, abd_stream_t stream) {
  if (int rc = check_train_args(a)) return rc;
  Ctx c;
  if (int rc = make_stat_ctx(net, a->batch, a->params, a->grads, a->running, a->num_batches_tracked, workspace,
                             workspace_bytes, stream, &c))
    return rc;
  if (int rc = run_forward(c, a->x, 1, a)) return rc;
  if (int rc = run_ce(c, a->labels, a->indicators, true, a->grad_scale, a->logits_out, a->metrics)) return rc;
  if (int rc = run_backward(c, a->x, c.template at<float>(c.L.dlogits))) return rc;
  return adam_tail(a, net->off[P_COUNT], stream);
}

template <class Ctx, class Net>
int stat_net_eval(Net* net, const float* x, int64_t batch, const float* params, const float* running,
                  const int64_t* labels, const int64_t* indicators, float* logits, int64_t* metrics, void* workspace,
                  size_t workspace_bytes, abd_stream_t stream) {
  ABD_CHECK(x && logits && running, ABD_E_INVALID, "NULL x / logits / running");
  Ctx c;
  if (int rc = make_stat_ctx(net, batch, params, nullptr, const_cast<float*>(running), nullptr, workspace,
                             workspace_bytes, stream, &c))
    return rc;
  if (int rc = run_forward(c, x, 0, nullptr)) return rc;
  return run_ce(c, labels, indicators, false, 1.0f, logits, metrics);
}
