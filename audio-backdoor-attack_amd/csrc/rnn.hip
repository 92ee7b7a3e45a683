// RNN (reference utils/models.py:231-257) on gfx950: nn.LSTM(F, 768, 3, batch_first) -> nn.Linear(768, K)
// on the last time step, cross entropy, BPTT.  Every product is fp32 (v_mfma_f32_32x32x2_f32).
//
// GEMMs: gemm_tiled_kernel, an LDS-tiled block of 4 waves (2 x 2), each wave TM x TN accumulator tiles
// of 32 x 32; the block tile is (64 TM) x (64 TN) x 32.  Both operands are staged through LDS; strides
// select the NN / NT / TN forms, ragged M / N / K are zero-filled on load and masked on store.  A long
// reduction (the weight gradients' B*T rows) is split over blockIdx.z into slices whose partial products
// colsum_kernel sums in slice order: no float atomics, two runs are bit-equal.
//
// Recurrence: one launch per time step and layer, the kernel boundary being the only synchronisation
// between steps.  One layer's W_hh is 4*768*768*4 B = 9.4 MB, so it cannot stay in LDS as lstm_attn.hip's
// 64 KiB one does; each step streams it (from L2 / MALL) through LDS.  rnn_step_fwd_kernel: a workgroup
// owns kRecRows batch rows and 32 hidden units; wave g accumulates gate g of those units, so the
// workgroup holds i, f, g and o of its units and finishes c_t and h_t in its epilogue.
#include <algorithm>
#include <cmath>

#include "abd_common.h"

struct abd_rnn {
  int T, F, K;
  int64_t off[15];
};

namespace {

constexpr int kT = 256;
constexpr int kHid = 768;          // LSTM hidden size
constexpr int kGates = 4 * kHid;   // gate rows, torch order i f g o
constexpr int kLayers = 3;
constexpr int kRecRows = 32;       // batch rows of one recurrent workgroup
constexpr int kRecUnits = 32;      // hidden units of one recurrent workgroup
constexpr int kLargeMinBlocks = 96;  // below this many 128 x 128 blocks the 64 x 64 tile fills more CUs
constexpr int kSliceRows = 256;    // least rows of one weight-gradient slice
constexpr int kMaxSlices = 8;

enum { P_FCW = 4 * kLayers, P_FCB, P_COUNT };

// backward cell, colsum, weight_grad; GemmArgs and its three forms, the host helpers; colsum_kernel, ce_kernel,
// metrics_kernel
#include "lstm_common.inc"
#include "gemm_tiled_kernel.inc"   // kBK, the tile sizes, f16v, gemm_tiled_kernel and launch_gemm

// ------------------------------------------------------------------ recurrence
struct StepArgs {
  float* gates;        // [B*T][3072]: x_t W_ih^T + b_ih + b_hh on entry, activated i f g o on exit
  float* h;            // [B][T][768]
  float* c;            // [B][T][768]
  const float* whh;    // [3072][768]
  const float* dy;     // backward: [B][T][768] gradient of this layer's output, or NULL
  const float* dhrec;  // backward: [B][768] dG_{t+1} W_hh (the head's dh at the top layer's last step), or NULL
  float* dc;           // backward: [B][768] carried cell gradient
  int B, T, t;
};

// step t of one layer: G_t = XP_t + h_{t-1} W_hh^T, activations, c_t, h_t.  grid (ceil(B / 32), 24).
__global__ void __launch_bounds__(kT) rnn_step_fwd_kernel(StepArgs a) {
  __shared__ float Hs[kRecRows * (kBK + 1)];
  __shared__ float Ws[4 * kRecUnits * (kBK + 1)];
  __shared__ float Es[4][kRecRows][kRecUnits + 1];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int b0 = blockIdx.x * kRecRows, u0 = blockIdx.y * kRecUnits;
  const int T = a.T, t = a.t;
  f16v acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.0f;
  if (t > 0) {   // h_{-1} = 0: nothing to multiply at the first step
    for (int kb = 0; kb < kHid; kb += kBK) {
      float hr[kRecRows * kBK / kT], wr[4 * kRecUnits * kBK / kT];
#pragma unroll
      for (int i = 0; i < kRecRows * kBK / kT; ++i) {
        const int e = tid + i * kT, k = e & 31, m = e >> 5, b = b0 + m;
        hr[i] = b < a.B ? a.h[((int64_t)b * T + t - 1) * kHid + kb + k] : 0.0f;
      }
#pragma unroll
      for (int i = 0; i < 4 * kRecUnits * kBK / kT; ++i) {
        const int e = tid + i * kT, k = e & 31, j = e >> 5;   // j = gate * 32 + unit
        wr[i] = a.whh[((int64_t)(j >> 5) * kHid + u0 + (j & 31)) * kHid + kb + k];
      }
      __syncthreads();
#pragma unroll
      for (int i = 0; i < kRecRows * kBK / kT; ++i) {
        const int e = tid + i * kT;
        Hs[(e >> 5) * (kBK + 1) + (e & 31)] = hr[i];
      }
#pragma unroll
      for (int i = 0; i < 4 * kRecUnits * kBK / kT; ++i) {
        const int e = tid + i * kT;
        Ws[(e >> 5) * (kBK + 1) + (e & 31)] = wr[i];
      }
      __syncthreads();
#pragma unroll
      for (int kk = 0; kk < kBK / 2; ++kk) {
        const int k = 2 * kk + (lane >> 5);
        const float av = Hs[(lane & 31) * (kBK + 1) + k];
        const float bv = Ws[(w * kRecUnits + (lane & 31)) * (kBK + 1) + k];
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bv, acc, 0, 0, 0);
      }
    }
  }
#pragma unroll
  for (int r = 0; r < 16; ++r) Es[w][(r & 3) + 8 * (r >> 2) + 4 * (lane >> 5)][lane & 31] = acc[r];
  __syncthreads();
#pragma unroll
  for (int i = 0; i < kRecRows * kRecUnits / kT; ++i) {
    const int e = tid + i * kT, u = e & 31, m = e >> 5, b = b0 + m;
    if (b >= a.B) continue;
    const int64_t row = (int64_t)b * T + t;
    float* gp = a.gates + row * kGates + u0 + u;
    const float ig = sigmoid_acc(gp[0] + Es[0][m][u]);
    const float fg = sigmoid_acc(gp[kHid] + Es[1][m][u]);
    const float gg = tanhf(gp[2 * kHid] + Es[2][m][u]);
    const float og = sigmoid_acc(gp[3 * kHid] + Es[3][m][u]);
    const float cp = t > 0 ? a.c[(row - 1) * kHid + u0 + u] : 0.0f;
    const float ct = fg * cp + ig * gg;
    gp[0] = ig;
    gp[kHid] = fg;
    gp[2 * kHid] = gg;
    gp[3 * kHid] = og;
    a.c[row * kHid + u0 + u] = ct;
    a.h[row * kHid + u0 + u] = og * tanhf(ct);
  }
}

// step t of one layer's BPTT: the pre-activation gate gradients dG_t, written over the activated gates of
// that step (nothing reads them again), and the carried cell gradient.  One thread per (row, unit).
__global__ void __launch_bounds__(kT) rnn_gate_bwd_kernel(StepArgs a) {
  const int64_t e = (int64_t)blockIdx.x * kT + threadIdx.x;
  if (e >= (int64_t)a.B * kHid) return;
  const int b = (int)(e / kHid), u = (int)(e - (int64_t)b * kHid);
  const int T = a.T, t = a.t;
  const int64_t row = (int64_t)b * T + t;
  float* gp = a.gates + row * kGates + u;
  const float ig = gp[0], fg = gp[kHid], gg = gp[2 * kHid], og = gp[3 * kHid];
  const float ct = a.c[row * kHid + u];
  const float cp = t > 0 ? a.c[(row - 1) * kHid + u] : 0.0f;
  float dht = a.dy ? a.dy[row * kHid + u] : 0.0f;
  if (a.dhrec) dht += a.dhrec[e];
  const float dcin = t < T - 1 ? a.dc[e] : 0.0f;
  lstm_cell_bwd(ig, fg, gg, og, ct, cp, dht, dcin, gp[0], gp[kHid], gp[2 * kHid], gp[3 * kHid], a.dc[e]);
}

// ------------------------------------------------------------------ host side
// workspace map (byte offsets); every buffer 256-byte aligned
struct Layout {
  size_t h[kLayers], c[kLayers], gates[kLayers], dy, dhtop, dhrec, dc, logits, dlogits, rowinfo, slab, colp, total;
  int ksplit;
  int64_t kchunk;
};

Layout make_layout(const abd_rnn* n, int64_t B) {
  Layout L{};
  Take take;
  const size_t BT = (size_t)B * n->T;
  for (int l = 0; l < kLayers; ++l) {
    L.h[l] = take(4 * BT * kHid);
    L.c[l] = take(4 * BT * kHid);
    L.gates[l] = take(4 * BT * kGates);   // input projections, activated gates, then gate gradients
  }
  L.dy = take(4 * BT * kHid);             // gradient of the output of the layer below the one in hand
  L.dhtop = take(4 * (size_t)B * kHid);
  L.dhrec = take(4 * (size_t)B * kHid);
  L.dc = take(4 * (size_t)B * kHid);
  L.logits = take(4 * (size_t)B * n->K);
  L.dlogits = take(4 * (size_t)B * n->K);
  L.rowinfo = take(4 * (size_t)B * 4);
  // weight-gradient GEMMs: B*T rows of reduction split into slices of >= kSliceRows rows
  const Slices sl = plan_slices((int64_t)BT, kMaxSlices, kSliceRows, kBK);
  L.ksplit = sl.ksplit;
  L.kchunk = sl.kchunk;
  L.slab = take(L.ksplit > 1 ? 4 * (size_t)L.ksplit * kGates * kHid : 0);
  L.colp = take(4 * (size_t)64 * kGates);
  L.total = take.o;
  return L;
}

struct Ctx : CtxBase {
  const abd_rnn* n;
  Layout L;
  const float* p(int i) const { return params + n->off[i]; }
  float* g(int i) const { return grads + n->off[i]; }
};

int run_forward(const Ctx& c, const float* x) {
  const int T = c.n->T;
  const int64_t BT = c.B * T;
  const float* in = x;
  int width = c.n->F;
  for (int l = 0; l < kLayers; ++l) {
    float* gates = c.at<float>(c.L.gates[l]);
    // x W_ih^T + b_ih + b_hh over all B*T rows
    GemmArgs g = gemm_nt(in, width, c.p(4 * l), gates, (int)BT, kGates, width);
    g.bias1 = c.p(4 * l + 2);
    g.bias2 = c.p(4 * l + 3);
    if (int rc = launch_gemm(c.s, g)) return rc;
    StepArgs sa{};
    sa.gates = gates;
    sa.h = c.at<float>(c.L.h[l]);
    sa.c = c.at<float>(c.L.c[l]);
    sa.whh = c.p(4 * l + 1);
    sa.B = (int)c.B;
    sa.T = T;
    const dim3 grid((unsigned)((c.B + kRecRows - 1) / kRecRows), kHid / kRecUnits);
    for (int t = 0; t < T; ++t) {
      sa.t = t;
      rnn_step_fwd_kernel<<<grid, kT, 0, c.s>>>(sa);
      ABD_LAUNCH_CHECK();
    }
    in = sa.h;
    width = kHid;
  }
  // fc on the top layer's last step
  GemmArgs f = gemm_nt(c.at<float>(c.L.h[kLayers - 1]) + (int64_t)(T - 1) * kHid, (int64_t)T * kHid, c.p(P_FCW),
                       c.at<float>(c.L.logits), (int)c.B, c.n->K, kHid);
  f.bias1 = c.p(P_FCB);
  return launch_gemm(c.s, f);
}

int run_backward(const Ctx& c, const float* x, const float* dlogits) {
  const int T = c.n->T, K = c.n->K;
  const int64_t BT = c.B * T;
  const float* hlast = c.at<float>(c.L.h[kLayers - 1]) + (int64_t)(T - 1) * kHid;
  // dfc.weight[j][i] = sum_b dlogits[b][j] h_{T-1}[b][i]
  if (int rc = launch_gemm(c.s, gemm_tn(dlogits, hlast, (int64_t)T * kHid, c.g(P_FCW), K, kHid, c.B))) return rc;
  if (int rc = colsum(c, dlogits, c.B, K, K, c.g(P_FCB))) return rc;
  // dh_{T-1} of the top layer = dlogits fc.weight; its dy is zero everywhere else
  if (int rc = launch_gemm(c.s, gemm_nn(dlogits, K, c.p(P_FCW), c.at<float>(c.L.dhtop), (int)c.B, kHid, K))) return rc;
  float* dy = c.at<float>(c.L.dy);
  float* dhrec = c.at<float>(c.L.dhrec);
  for (int l = kLayers - 1; l >= 0; --l) {
    const bool top = l == kLayers - 1;
    float* gates = c.at<float>(c.L.gates[l]);
    const float* h = c.at<float>(c.L.h[l]);
    const float* in = l ? c.at<float>(c.L.h[l - 1]) : x;
    const int width = l ? kHid : c.n->F;
    StepArgs sa{};
    sa.gates = gates;
    sa.c = c.at<float>(c.L.c[l]);
    sa.dy = top ? nullptr : dy;
    sa.dc = c.at<float>(c.L.dc);
    sa.B = (int)c.B;
    sa.T = T;
    // dh_{t-1} = dG_t W_hh; A is set per step
    GemmArgs r = gemm_nn(nullptr, (int64_t)T * kGates, c.p(4 * l + 1), dhrec, (int)c.B, kHid, kGates);
    const unsigned nblk = (unsigned)((c.B * kHid + kT - 1) / kT);
    for (int t = T - 1; t >= 0; --t) {
      sa.t = t;
      sa.dhrec = t == T - 1 ? (top ? c.at<float>(c.L.dhtop) : nullptr) : dhrec;
      rnn_gate_bwd_kernel<<<nblk, kT, 0, c.s>>>(sa);
      ABD_LAUNCH_CHECK();
      if (t > 0) {
        r.A = gates + (int64_t)t * kGates;
        if (int rc = launch_gemm(c.s, r)) return rc;
      }
    }
    if (int rc = weight_grad(c, T, gates, in, width, 0, c.g(4 * l))) return rc;
    if (T > 1) {
      if (int rc = weight_grad(c, T, gates, h, kHid, -1, c.g(4 * l + 1))) return rc;
    } else {
      ABD_HIP(hipMemsetAsync(c.g(4 * l + 1), 0, sizeof(float) * kGates * kHid, c.s));
    }
    if (int rc = colsum(c, gates, BT, kGates, kGates, c.g(4 * l + 2))) return rc;
    ABD_HIP(hipMemcpyAsync(c.g(4 * l + 3), c.g(4 * l + 2), sizeof(float) * kGates, hipMemcpyDeviceToDevice, c.s));
    if (l > 0) {
      // gradient of the layer below's output: dG W_ih
      if (int rc = launch_gemm(c.s, gemm_nn(gates, kGates, c.p(4 * l), dy, (int)BT, kHid, kGates))) return rc;
    }
  }
  return ABD_OK;
}

int make_ctx(const abd_rnn* net, int64_t B, const float* params, float* grads, void* ws, size_t bytes,
             abd_stream_t stream, Ctx* c) {
  return make_ctx(net, B, params, grads, ws, bytes, stream, kGates, make_layout, c);
}

}  // namespace

extern "C" {

int abd_rnn_tile_info(int what) {
  switch (what) {
    case 0: return kRecRows;
    case 1: return kSmallTile;
    case 2: return kLargeTile;
    case 3: return kSliceRows;
    case 4: return kColsumRows;
    case 5: return kLargeMinBlocks;
    default: return -1;
  }
}

int abd_rnn_create(int T, int F, int num_classes, abd_rnn** net) {
  ABD_CHECK(net != nullptr, ABD_E_INVALID, "NULL out pointer");
  ABD_CHECK(F >= 1 && F <= 128, ABD_E_UNSUPPORTED, "RNN: time_len %d outside [1, 128]", F);
  ABD_CHECK(T >= 1 && T <= 1024, ABD_E_UNSUPPORTED, "RNN: sequence length %d outside [1, 1024]", T);
  ABD_CHECK(num_classes >= 1 && num_classes <= 4096, ABD_E_UNSUPPORTED, "num_classes must be in [1, 4096]");
  auto* n = new abd_rnn();
  n->T = T;
  n->F = F;
  n->K = num_classes;
  n->off[0] = 0;
  for (int l = 0; l < kLayers; ++l) {
    const int64_t sz[4] = {(int64_t)kGates * (l ? kHid : F), (int64_t)kGates * kHid, kGates, kGates};
    for (int i = 0; i < 4; ++i) n->off[4 * l + i + 1] = n->off[4 * l + i] + sz[i];
  }
  n->off[P_FCW + 1] = n->off[P_FCW] + (int64_t)num_classes * kHid;
  n->off[P_FCB + 1] = n->off[P_FCB] + num_classes;
  *net = n;
  return ABD_OK;
}

void abd_rnn_destroy(abd_rnn* net) { delete net; }

int64_t abd_rnn_param_count(const abd_rnn* net) { return net ? net->off[P_COUNT] : 0; }

int abd_rnn_param_offsets(const abd_rnn* net, int64_t* offsets) {
  ABD_CHECK(net && offsets, ABD_E_INVALID, "NULL argument");
  for (int i = 0; i <= P_COUNT; ++i) offsets[i] = net->off[i];
  return ABD_OK;
}

size_t abd_rnn_workspace_bytes(const abd_rnn* net, int64_t batch) {
  if (!net || batch < 1) return 0;
  return make_layout(net, batch).total;
}

int64_t abd_rnn_workspace_offset(const abd_rnn* net, int64_t batch, const char* name) {
  if (!net || !name || batch < 1) return -1;
  const Layout L = make_layout(net, batch);
  const NamedOffset tab[] = {
      {"h1", L.h[0]}, {"h2", L.h[1]}, {"h3", L.h[2]}, {"c1", L.c[0]}, {"c2", L.c[1]}, {"c3", L.c[2]},
      {"gates1", L.gates[0]}, {"gates2", L.gates[1]}, {"gates3", L.gates[2]}, {"logits", L.logits},
      {"dlogits", L.dlogits}, {"rowinfo", L.rowinfo}};
  return find_offset(tab, name);
}

int abd_rnn_forward(abd_rnn* net, const abd_rnn_args* a, void* workspace, size_t workspace_bytes,
                    abd_stream_t stream) {
  ABD_CHECK(a != nullptr && a->x, ABD_E_INVALID, "NULL x");
  Ctx c;
  if (int rc = make_ctx(net, a->batch, a->params, a->grads, workspace, workspace_bytes, stream, &c)) return rc;
  if (int rc = run_forward(c, a->x)) return rc;
  return run_ce(c, nullptr, nullptr, false, 1.0f, a->logits_out, nullptr);
}

int abd_rnn_backward(abd_rnn* net, const abd_rnn_args* a, const float* dlogits, void* workspace,
                     size_t workspace_bytes, abd_stream_t stream) {
  ABD_CHECK(a != nullptr && a->x && a->grads && dlogits, ABD_E_INVALID, "NULL x / grads / dlogits");
  Ctx c;
  if (int rc = make_ctx(net, a->batch, a->params, a->grads, workspace, workspace_bytes, stream, &c)) return rc;
  return run_backward(c, a->x, dlogits);
}

int abd_rnn_train_step(abd_rnn* net, const abd_rnn_args* a, void* workspace, size_t workspace_bytes,
                       abd_stream_t stream) {
  if (int rc = check_train_args(a)) return rc;
  Ctx c;
  if (int rc = make_ctx(net, a->batch, a->params, a->grads, workspace, workspace_bytes, stream, &c)) return rc;
  if (int rc = run_forward(c, a->x)) return rc;
  if (int rc = run_ce(c, a->labels, a->indicators, true, a->grad_scale, a->logits_out, a->metrics)) return rc;
  if (int rc = run_backward(c, a->x, c.at<float>(c.L.dlogits))) return rc;
  return adam_tail(a, net->off[P_COUNT], stream);
}

int abd_rnn_eval(abd_rnn* net, const float* x, int64_t batch, const float* params, const int64_t* labels,
                 const int64_t* indicators, float* logits, int64_t* metrics, void* workspace,
                 size_t workspace_bytes, abd_stream_t stream) {
  ABD_CHECK(x && logits, ABD_E_INVALID, "NULL x / logits");
  Ctx c;
  if (int rc = make_ctx(net, batch, params, nullptr, workspace, workspace_bytes, stream, &c)) return rc;
  if (int rc = run_forward(c, x)) return rc;
  return run_ce(c, labels, indicators, false, 1.0f, logits, metrics);
}

}  // extern "C"
