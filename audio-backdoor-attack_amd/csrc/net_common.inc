// What the five flat-buffer networks (lstm_attn.hip, rnn.hip, largecnn.hip, resnet.hip, smalllstm.hip) share: the
// description of a GEMM and its three forms, the dropout hash, the host helpers around the workspace, the cross
// entropy and the two ends of a train step.  Included inside each file's anonymous namespace, after abd_common.h (the
// three LSTM files include it through lstm_common.inc).  Each file keeps its Layout / make_layout
// and a Ctx derived from CtxBase with members n (the net) and L (the layout; logits, dlogits, rowinfo and colp
// are read here).

// colsum_kernel, ce_kernel, metrics_kernel
#include "reduce_ce.inc"

// ------------------------------------------------------------------ GEMM description
// C[m][n] (+)= sum_k A(m,k) B(k,n) (+ bias1[n] + bias2[n]); A(m,k) = A[m*sam + k*sak],
// B(k,n) = B[kb*sbk + n*sbn].  shift != 0: kb = k + shift when k's step (k % T) + shift stays inside
// [0, T), else the term is zero (h_{t-1} / h_{t+1} of the recurrent weight gradient).  blockIdx.z takes the
// k-slice [z*kchunk, (z+1)*kchunk) and writes C + z*cz.
struct GemmArgs {
  const float* A;
  const float* B;
  float* C;
  int M, N, K;
  int64_t sam, sak, sbk, sbn, ldc, cz;
  const float* bias1;
  const float* bias2;
  int accumulate, kchunk, T, shift;
};

// C[M][N] = A W^T: A's rows lda apart, W [N][K] and C dense (projections, fc)
GemmArgs gemm_nt(const float* A, int64_t lda, const float* W, float* C, int M, int N, int K) {
  GemmArgs g{};
  g.A = A, g.B = W, g.C = C;
  g.M = M, g.N = N, g.K = K;
  g.sam = lda, g.sak = 1, g.sbk = 1, g.sbn = K, g.ldc = N;
  return g;
}

// C[M][N] = A W: A's rows lda apart, W [K][N] and C dense (data gradients)
GemmArgs gemm_nn(const float* A, int64_t lda, const float* W, float* C, int M, int N, int K) {
  GemmArgs g{};
  g.A = A, g.B = W, g.C = C;
  g.M = M, g.N = N, g.K = K;
  g.sam = lda, g.sak = 1, g.sbk = N, g.sbn = 1, g.ldc = N;
  return g;
}

// C[M][N] = D^T X over `rows` rows: D [rows][M] dense, X's rows ldx apart, C dense (weight gradients).
// The caller sets T / shift for a time-shifted X, and C / cz / kchunk for a sliced reduction.
GemmArgs gemm_tn(const float* D, const float* X, int64_t ldx, float* C, int M, int N, int64_t rows) {
  GemmArgs g{};
  g.A = D, g.B = X, g.C = C;
  g.M = M, g.N = N, g.K = (int)rows;
  g.sam = 1, g.sak = M, g.sbk = ldx, g.sbn = 1, g.ldc = N;
  return g;
}

// ------------------------------------------------------------------ dropout hash
// the dropout hash of the smallcnn kernels: keep with probability 1 - p
__device__ __forceinline__ bool keep_hash(uint64_t seed, uint64_t stream, uint64_t idx, float p) {
  uint64_t z = seed ^ (stream * 0x9E3779B97F4A7C15ull) ^ (idx * 0xD1B54A32D192ED03ull);
  z += 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  z ^= z >> 31;
  const float u = (float)(uint32_t)(z >> 40) * (1.0f / 16777216.0f);
  return u >= p;
}

// ------------------------------------------------------------------ host helpers
// workspace byte offsets, every buffer 256-byte aligned: off = take(bytes), the total is take.o
struct Take {
  size_t o = 0;
  size_t operator()(size_t bytes) {
    const size_t r = o;
    o += (bytes + 255) & ~(size_t)255;
    return r;
  }
};

// a reduction over `rows` rows in at most max_slices slices of at least min_rows rows, each a multiple of
// the GEMM kernel's k_step
struct Slices {
  int ksplit;
  int64_t kchunk;
};

Slices plan_slices(int64_t rows, int max_slices, int min_rows, int k_step) {
  Slices p;
  p.ksplit = (int)std::max<int64_t>(1, std::min<int64_t>(max_slices, rows / min_rows));
  p.kchunk = (rows + p.ksplit - 1) / p.ksplit;
  p.kchunk = (p.kchunk + k_step - 1) / k_step * k_step;
  p.ksplit = (int)((rows + p.kchunk - 1) / p.kchunk);
  return p;
}

struct CtxBase {
  char* ws;
  hipStream_t s;
  int64_t B;
  const float* params;
  float* grads;
  template <class Tp> Tp* at(size_t off) const { return reinterpret_cast<Tp*>(ws + off); }
};

// layout: the file's make_layout.  row_factor: the widest per-(row, step) index the kernels form in 32 bits.
template <class Net, class Ctx, class LayoutFn>
int make_ctx(const Net* net, int64_t B, const float* params, float* grads, void* ws, size_t bytes,
             abd_stream_t stream, int64_t row_factor, LayoutFn layout, Ctx* c) {
  ABD_CHECK(net != nullptr, ABD_E_INVALID, "NULL network");
  ABD_CHECK(B >= 1 && B * (int64_t)net->T * row_factor < (1LL << 31), ABD_E_INVALID,
            "batch %lld outside the kernels' 32-bit row range", (long long)B);
  ABD_CHECK(params != nullptr, ABD_E_INVALID, "NULL params");
  c->n = net;
  c->L = layout(net, B);
  ABD_CHECK(ws != nullptr && bytes >= c->L.total, ABD_E_WORKSPACE, "workspace %zu < %zu bytes", bytes, c->L.total);
  ABD_CHECK((reinterpret_cast<uintptr_t>(ws) & 15) == 0, ABD_E_INVALID, "workspace must be 16-byte aligned");
  c->ws = static_cast<char*>(ws);
  c->s = static_cast<hipStream_t>(stream);
  c->B = B;
  c->params = params;
  c->grads = grads;
  return ABD_OK;
}

// out[cols] (+)= column sums of A (rows x cols, leading dimension ld).  Past two_stage_rows rows, and for at
// most two_stage_cols columns (what the colp buffer holds), two fixed-order stages.
template <class Ctx>
int launch_colsum(const Ctx& c, const float* A, int64_t rows, int64_t cols, int64_t ld, float* out, int accumulate,
                  int64_t two_stage_cols, int64_t two_stage_rows) {
  const int nb = (int)((cols + kRedT - 1) / kRedT);
  const int S = (cols <= two_stage_cols && rows > two_stage_rows) ? (int)std::min<int64_t>(64, rows / 256) : 1;
  if (S <= 1) {
    colsum_kernel<<<dim3(nb, 1), kRedT, 0, c.s>>>(A, rows, cols, ld, rows, out, 0, accumulate);
    ABD_LAUNCH_CHECK();
    return ABD_OK;
  }
  const int64_t chunk = (rows + S - 1) / S;
  float* part = c.template at<float>(c.L.colp);
  colsum_kernel<<<dim3(nb, S), kRedT, 0, c.s>>>(A, rows, cols, ld, chunk, part, cols, 0);
  ABD_LAUNCH_CHECK();
  colsum_kernel<<<dim3(nb, 1), kRedT, 0, c.s>>>(part, S, cols, cols, S, out, 0, accumulate);
  ABD_LAUNCH_CHECK();
  return ABD_OK;
}

template <class Ctx>
int run_ce(const Ctx& c, const int64_t* labels, const int64_t* ind, bool grad, float grad_scale, float* logits_out,
           int64_t* metrics) {
  CeArgs ce{};
  ce.logits = c.template at<float>(c.L.logits);
  ce.labels = labels;
  ce.ind = ind;
  ce.dlogits = grad ? c.template at<float>(c.L.dlogits) : nullptr;
  ce.rowinfo = c.template at<float>(c.L.rowinfo);
  ce.logits_out = logits_out;
  ce.K = c.n->K;
  ce.scale = grad_scale / (float)c.B;
  if (!labels && !logits_out) return ABD_OK;
  ce_kernel<<<(unsigned)c.B, 64, 0, c.s>>>(ce);
  ABD_LAUNCH_CHECK();
  if (labels && metrics) {
    metrics_kernel<<<1, kRedT, 0, c.s>>>(ce.rowinfo, (int)c.B, metrics, (double)grad_scale);
    ABD_LAUNCH_CHECK();
  }
  return ABD_OK;
}

// the abd_*_workspace_offset lookup: -1 for a name the table does not have
struct NamedOffset {
  const char* name;
  size_t off;
};

template <size_t N>
int64_t find_offset(const NamedOffset (&tab)[N], const char* name) {
  for (const auto& e : tab)
    if (!strcmp(e.name, name)) return (int64_t)e.off;
  return -1;
}

// ------------------------------------------------------------------ the two ends of a train step
// what every abd_*_train_step checks of its args struct before it touches the network
template <class Args>
int check_train_args(const Args* a) {
  ABD_CHECK(a != nullptr && a->x && a->grads, ABD_E_INVALID, "NULL x / grads");
  ABD_CHECK(a->labels != nullptr, ABD_E_INVALID, "train_step needs labels");
  ABD_CHECK(!a->do_update || (a->exp_avg && a->exp_avg_sq && a->adam_step >= 1), ABD_E_INVALID,
            "do_update needs the Adam moments and adam_step >= 1");
  return ABD_OK;
}

// Adam over the n parameters when the step asks for the update
template <class Args>
int adam_tail(const Args* a, int64_t n, abd_stream_t stream) {
  if (!a->do_update) return ABD_OK;
  return abd_adam_f32(a->params, a->grads, a->exp_avg, a->exp_avg_sq, n, a->adam_step, a->lr, a->beta1, a->beta2,
                      a->eps, stream);
}
