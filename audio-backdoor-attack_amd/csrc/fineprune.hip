// Fine-Pruning (fp.py:131-203): the mean activation of fc2's input over a clean batch, the prune sweep
// of fp.py:164-195 (temp_test of the model with the lowest-activation units masked out of fc2.weight,
// every step of the sweep from ONE eval forward of the batch) and one batch of the masked Adam
// fine-tuning (train_finetuning, fp.py:52-76, under prune.custom_from_mask).  The network passes go
// through the public C ABI of smallcnn.hip (abd_smallcnn_eval, abd_smallcnn_train_step with
// do_update = 0); nothing of it is re-implemented.  The eval forward leaves fc2's input,
// relu(fc1(...)), in the workspace buffer "d2" (abd_smallcnn_workspace_offset).
//
// Every launch is asynchronous on the caller's stream, allocates nothing and copies nothing from the
// host: one pass's unit masks (bit-packed, 2 KB) travel as a kernel argument.  Reductions run in a
// fixed order (per-lane strided sums in double, a butterfly over the wave); there are no
// floating-point atomics, so equal inputs give bit-equal results.
#include <cmath>
#include <type_traits>

#include "abd_common.h"

namespace {

// kT, grid_for, round256, AdamConsts / adam_elem_stored, no_update_args, checks
#include "defense_common.inc"

constexpr int kUnits = ABD_FCPRUNE_UNITS;
constexpr int kPass = ABD_FCPRUNE_PASS_VARIANTS;

// ---------------------------------------------------------------- hidden sums
// sums[u] += sum_b d2[b][u]: block of 256 threads = 128 units x 2 row phases; a thread adds its rows
// in ascending order in double, the two phases are added phase 0 first.
__global__ void __launch_bounds__(kT) hidden_sums_kernel(const float* __restrict__ d2, int B,
                                                         double* __restrict__ sums) {
  __shared__ double half[kUnits];
  const int u = threadIdx.x & (kUnits - 1), phase = threadIdx.x >> 7;
  double acc = 0.0;
  for (int b = phase; b < B; b += 2) acc += (double)d2[(int64_t)b * kUnits + u];
  if (phase == 1) half[u] = acc;
  __syncthreads();
  if (phase == 0) sums[u] += acc + half[u];
}

// ---------------------------------------------------------------- prune sweep head
// bit u of variant v: unit u is pruned (fc2.weight[:, u] removed)
struct PruneMasks {
  uint32_t bits[kPass][kUnits / 32];
};

struct PruneArgs {
  const float* d2;  // (B, 128) fc2's input of the baseline forward
  const float* w;   // fc2.weight (K, 128)
  const float* b;   // (K)
  const int64_t* labels;
  int B, K, n;      // n variants in this pass
  float* rowloss;   // (n, B)
  float* rowhit;    // (n, B)
};

// A block takes rows blockIdx.x, + gridDim.x, ...; lane k of every wave keeps fc2.weight[k][:] in
// registers (read once per block), a row's 128 activations are staged in LDS once for all variants,
// and wave w evaluates variants w, w + 4, ... of the row: logits in fc2_loss_kernel's order (bias
// first, units ascending, fma) with the pruned units skipped, then its log_softmax / CrossEntropyLoss
// / first-index arg-max arithmetic.
__global__ void __launch_bounds__(kT) fcprune_head_kernel(PruneArgs a, PruneMasks m) {
  __shared__ float4 xs[kUnits / 4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const bool act = lane < a.K;
  float4 wr[kUnits / 4];
  const float4* wsrc = reinterpret_cast<const float4*>(a.w + (int64_t)(act ? lane : 0) * kUnits);
#pragma unroll
  for (int q = 0; q < kUnits / 4; ++q) wr[q] = wsrc[q];
  const float bias = act ? a.b[lane] : 0.0f;
  for (int row = blockIdx.x; row < a.B; row += gridDim.x) {
    __syncthreads();  // the previous row's readers are done
    if (threadIdx.x < kUnits / 4) xs[threadIdx.x] = reinterpret_cast<const float4*>(a.d2 + (int64_t)row * kUnits)[threadIdx.x];
    __syncthreads();
    const int y = (int)a.labels[row];
    for (int v = wave; v < a.n; v += kT / 64) {
      float acc = bias;
#pragma unroll
      for (int q = 0; q < kUnits / 4; ++q) {
        const uint32_t nib = (m.bits[v][q >> 3] >> ((q & 7) * 4)) & 15u;  // wave-uniform
        const float4 x = xs[q], wq = wr[q];
        const float t0 = fmaf(x.x, wq.x, acc);
        acc = (nib & 1u) ? acc : t0;
        const float t1 = fmaf(x.y, wq.y, acc);
        acc = (nib & 2u) ? acc : t1;
        const float t2 = fmaf(x.z, wq.z, acc);
        acc = (nib & 4u) ? acc : t2;
        const float t3 = fmaf(x.w, wq.w, acc);
        acc = (nib & 8u) ? acc : t3;
      }
      const float z = act ? acc : -INFINITY;
      // o = log_softmax(z) (model output); loss = CE(o) = logsumexp(o) - o[y]
      const float mz = abd::wave_max(z);
      const float ez = act ? expf(z - mz) : 0.0f;
      const float lse = mz + logf(abd::wave_sum(ez));
      const float o = act ? z - lse : -INFINITY;
      const float mo = abd::wave_max(o);
      const float eo = act ? expf(o - mo) : 0.0f;
      const float lse2 = mo + logf(abd::wave_sum(eo));
      const float oy = __shfl(o, y, 64);
      // first index of the maximum (torch max(dim=1))
      const unsigned long long ball = __ballot(act && o == mo);
      const int pred = __ffsll((long long)ball) - 1;
      if (lane == 0) {
        const int64_t at = (int64_t)v * a.B + row;
        a.rowloss[at] = lse2 - oy;
        a.rowhit[at] = pred == y ? 1.0f : 0.0f;
      }
    }
  }
}

// one wave per variant of the pass: the rows' losses / hits summed in a fixed order (double; counts
// <= B < 2^31 are exact in double) into the accumulators of variant v0 + blockIdx.x.  ablate.hip's
// abl_reduce_kernel has this shape; that file compiles smallcnn.hip whole and keeps its own.
__global__ void __launch_bounds__(64) fcprune_reduce_kernel(const float* __restrict__ rowloss,
                                                            const float* __restrict__ rowhit, int B, int v0,
                                                            double* __restrict__ loss_sum,
                                                            int64_t* __restrict__ correct) {
  const int v = blockIdx.x, lane = threadIdx.x;
  double s = 0.0, c = 0.0;
  for (int i = lane; i < B; i += 64) {
    s += (double)rowloss[(int64_t)v * B + i];
    c += (double)rowhit[(int64_t)v * B + i];
  }
  s = abd::wave_sum_d(s);
  c = abd::wave_sum_d(c);
  if (lane == 0) {
    loss_sum[v0 + v] += s;
    correct[v0 + v] += (int64_t)c;
  }
}

// ---------------------------------------------------------------- masked gradient + Adam
struct MaskedAdamArgs {
  float* p;
  float* g;
  float* m;
  float* v;
  int64_t n;
  int64_t w_off, w_end;  // fc2.weight's elements [w_off, w_end) of the flat buffers, (K, 128) row-major
  const uint8_t* pruned;  // device uint8[128], nonzero = pruned
  AdamConsts c;
};

// grads[fc2.weight[:, j]] <- 0 for every pruned unit j (the .grad torch leaves on weight_orig under
// prune.custom_from_mask), then Adam on the result
__global__ void __launch_bounds__(kT) masked_adam_kernel(MaskedAdamArgs a) {
  for (int64_t i = blockIdx.x * (int64_t)kT + threadIdx.x; i < a.n; i += (int64_t)gridDim.x * kT) {
    float gi = a.g[i];
    if (i >= a.w_off && i < a.w_end && a.pruned[(i - a.w_off) & (kUnits - 1)]) {
      gi = 0.0f;
      a.g[i] = gi;
    }
    adam_elem_stored(gi, a.c, a.m, a.v, a.p, i);
  }
}

// the baseline eval forward of a batch into the workspace's first part; returns its d2 buffer
int baseline_forward(abd_cnn* net, const float* x, int64_t B, const float* params, const float* running, void* workspace,
                     size_t cnn_bytes, abd_stream_t stream, const float** d2) {
  const int64_t off = abd_smallcnn_workspace_offset(net, B, "d2");
  const int64_t lp = abd_smallcnn_workspace_offset(net, B, "logp");
  ABD_CHECK(off >= 0 && lp >= 0, ABD_E_INVALID, "the workspace has no d2 / logp buffer");
  char* base = static_cast<char*>(workspace);
  if (int rc = abd_smallcnn_eval(net, x, B, params, running, nullptr, nullptr, reinterpret_cast<float*>(base + lp),
                                 nullptr, workspace, cnn_bytes, stream))
    return rc;
  *d2 = reinterpret_cast<const float*>(base + off);
  return ABD_OK;
}

}  // namespace

extern "C" {

int abd_smallcnn_hidden_sums(abd_cnn* net, const float* x, int64_t batch, const float* params, const float* running,
                             double* sums, void* workspace, size_t workspace_bytes, abd_stream_t stream) {
  ABD_CHECK(net != nullptr, ABD_E_INVALID, "NULL net");
  ABD_CHECK(batch >= 0, ABD_E_INVALID, "negative batch");
  if (batch == 0) return ABD_OK;
  ABD_CHECK(x && params && running && sums, ABD_E_INVALID, "NULL argument");
  ABD_CHECK(batch < (1LL << 31), ABD_E_INVALID, "batch too large");
  const size_t need = abd_smallcnn_workspace_bytes(net, batch);
  if (int rc = check_workspace(workspace, workspace_bytes, need)) return rc;
  const float* d2 = nullptr;
  if (int rc = baseline_forward(net, x, batch, params, running, workspace, need, stream, &d2)) return rc;
  hidden_sums_kernel<<<1, kT, 0, static_cast<hipStream_t>(stream)>>>(d2, (int)batch, sums);
  ABD_LAUNCH_CHECK();
  return ABD_OK;
}

size_t abd_smallcnn_fcprune_workspace_bytes(const abd_cnn* net, int64_t batch, int n_variants) {
  if (!net || batch < 1 || n_variants < 1) return 0;
  const size_t pass = (size_t)(n_variants < kPass ? n_variants : kPass);
  return round256(abd_smallcnn_workspace_bytes(net, batch)) + 2 * round256(pass * (size_t)batch * sizeof(float));
}

int abd_smallcnn_fcprune_eval(abd_cnn* net, const float* x, int64_t batch, const float* params, const float* running,
                              const int64_t* labels, const uint8_t* masks, int n_variants, double* loss_sum,
                              int64_t* correct, void* workspace, size_t workspace_bytes, abd_stream_t stream) {
  ABD_CHECK(net != nullptr, ABD_E_INVALID, "NULL net");
  ABD_CHECK(batch >= 0 && n_variants >= 0, ABD_E_INVALID, "negative batch / variant count");
  if (batch == 0 || n_variants == 0) return ABD_OK;
  ABD_CHECK(x && params && running && labels && masks && loss_sum && correct, ABD_E_INVALID, "NULL argument");
  ABD_CHECK(batch < (1LL << 24), ABD_E_INVALID, "batch too large");
  const int64_t B = batch;
  const size_t cnn = abd_smallcnn_workspace_bytes(net, B);
  const size_t need = abd_smallcnn_fcprune_workspace_bytes(net, B, n_variants);
  if (int rc = check_workspace(workspace, workspace_bytes, need)) return rc;
  int64_t off[17];
  if (int rc = abd_smallcnn_param_offsets(net, off)) return rc;
  const int K = (int)(off[16] - off[15]);
  ABD_CHECK(off[15] - off[14] == (int64_t)K * kUnits && K >= 1 && K <= 64, ABD_E_UNSUPPORTED,
            "fc2 is not a (K <= 64) x %d layer", kUnits);
  ABD_CHECK((reinterpret_cast<uintptr_t>(params + off[14]) & 15u) == 0, ABD_E_INVALID,
            "fc2.weight must be 16-byte aligned inside params");
  hipStream_t s = static_cast<hipStream_t>(stream);
  const float* d2 = nullptr;
  if (int rc = baseline_forward(net, x, B, params, running, workspace, cnn, stream, &d2)) return rc;
  const size_t pass = (size_t)(n_variants < kPass ? n_variants : kPass);
  char* base = static_cast<char*>(workspace) + round256(cnn);
  PruneArgs a{};
  a.d2 = d2;
  a.w = params + off[14];
  a.b = params + off[15];
  a.labels = labels;
  a.B = (int)B;
  a.K = K;
  a.rowloss = reinterpret_cast<float*>(base);
  a.rowhit = reinterpret_cast<float*>(base + round256(pass * (size_t)B * sizeof(float)));
  for (int v0 = 0; v0 < n_variants; v0 += kPass) {
    const int n = n_variants - v0 < kPass ? n_variants - v0 : kPass;
    PruneMasks m{};
    for (int v = 0; v < n; ++v)
      for (int u = 0; u < kUnits; ++u)
        if (masks[(size_t)(v0 + v) * kUnits + u]) m.bits[v][u >> 5] |= 1u << (u & 31);
    a.n = n;
    fcprune_head_kernel<<<(unsigned)(B < 1024 ? B : 1024), kT, 0, s>>>(a, m);
    ABD_LAUNCH_CHECK();
    fcprune_reduce_kernel<<<(unsigned)n, 64, 0, s>>>(a.rowloss, a.rowhit, (int)B, v0, loss_sum, correct);
    ABD_LAUNCH_CHECK();
  }
  return ABD_OK;
}

size_t abd_smallcnn_pruned_finetune_workspace_bytes(const abd_cnn* net, int64_t batch) {
  if (!net || batch < 1) return 0;
  return abd_smallcnn_workspace_bytes(net, batch);
}

int abd_smallcnn_pruned_finetune_step(abd_cnn* net, const abd_pruned_finetune_args* a, void* workspace,
                                      size_t workspace_bytes, abd_stream_t stream) {
  ABD_CHECK(net && a && a->x && a->labels && a->params && a->grads && a->exp_avg && a->exp_avg_sq && a->running &&
                a->pruned,
            ABD_E_INVALID, "NULL argument");
  const int64_t B = a->batch;
  if (int rc = check_adam_batch("fine-tuning step", B, a->adam_step)) return rc;
  const size_t need = abd_smallcnn_workspace_bytes(net, B);
  if (int rc = check_workspace(workspace, workspace_bytes, need)) return rc;
  int64_t off[17];
  if (int rc = abd_smallcnn_param_offsets(net, off)) return rc;
  ABD_CHECK((off[15] - off[14]) % kUnits == 0, ABD_E_UNSUPPORTED, "fc2 does not have %d inputs", kUnits);
  // 1. forward, loss, backward with the (already masked) parameters: the gradient of the effective weight
  const abd_train_args t = no_update_args(*a);
  if (int rc = abd_smallcnn_train_step(net, &t, workspace, workspace_bytes, stream)) return rc;
  // 2. + 3. the pruned columns' gradient zeroed and written back, Adam on it
  const MaskedAdamArgs ma{a->params, a->grads, a->exp_avg, a->exp_avg_sq, off[16], off[14], off[15], a->pruned,
                          adam_consts(a->lr, a->beta1, a->beta2, a->eps, a->adam_step)};
  masked_adam_kernel<<<grid_for(off[16], 2048), kT, 0, static_cast<hipStream_t>(stream)>>>(ma);
  ABD_LAUNCH_CHECK();
  return ABD_OK;
}

}  // extern "C"
