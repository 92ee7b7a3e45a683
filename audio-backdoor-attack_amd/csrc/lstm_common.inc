// What lstm_attn.hip, rnn.hip and smalllstm.hip share on top of net_common.inc (GemmArgs, the host helpers, the
// cross entropy): the backward cell, the gate column sums and the sliced weight gradient.  Included inside each
// file's anonymous namespace, after abd_common.h and the file's kGates.  Each file keeps its recurrent kernels.

#include "net_common.inc"

constexpr int kColsumRows = 512;   // above this many rows the column sums run in two stages

// ------------------------------------------------------------------ cell arithmetic
__device__ __forceinline__ float sigmoid_acc(float x) { return 1.0f / (1.0f + expf(-x)); }

// The forward cell (c_t = f c_{t-1} + i g, h_t = o tanh(c_t)) stays written out in lstm_fwd_kernel and
// rnn_step_fwd_kernel: the build contracts the c_t sum to one FMA and picks the product to fuse by where
// c_{t-1} is defined (a register in front of the gates there, a load behind them here), fma(c, f, i g) against
// fma(i, g, f c).  One shared expression gives both kernels the same choice and moves one model's last bits.

// activated gates, c_t, c_{t-1}, dh_t (every contribution already summed) and the incoming dc -> the
// pre-activation gate gradients and the dc handed to the step before
__device__ __forceinline__ void lstm_cell_bwd(float ig, float fg, float gg, float og, float ct, float cp, float dht,
                                              float dcin, float& di, float& df, float& dgg, float& dob, float& dcout) {
  const float tc = tanhf(ct);
  const float dct = dcin + dht * og * (1.0f - tc * tc);
  di = dct * gg * ig * (1.0f - ig);
  df = dct * cp * fg * (1.0f - fg);
  dgg = dct * ig * (1.0f - gg * gg);
  dob = dht * tc * og * (1.0f - og);
  dcout = dct * fg;
}

// ------------------------------------------------------------------ host side
// the file's GEMM: lstm_attn.hip's one-wave kernel, gemm_tiled_kernel.inc's for the other two
int launch_gemm(hipStream_t s, GemmArgs g, int ksplit = 1);

// out[cols] = column sums of A; two fixed-order stages past kColsumRows rows
template <class Ctx>
int colsum(const Ctx& c, const float* A, int64_t rows, int64_t cols, int64_t ld, float* out) {
  return launch_colsum(c, A, rows, cols, ld, out, 0, kGates, kColsumRows);
}

// dW[j][i] = sum_rows dg[row][j] act[row][i] over all B*T rows of T-step sequences, sliced by the layout's ksplit /
// kchunk through its slab (shift -1: act one step back)
template <class Ctx>
int weight_grad(const Ctx& c, int T, const float* dg, const float* act, int in, int shift, float* out) {
  const int64_t BT = c.B * T;
  GemmArgs g = gemm_tn(dg, act, in, out, kGates, in, BT);
  g.T = T;
  g.shift = shift;
  if (c.L.ksplit <= 1) return launch_gemm(c.s, g);
  g.C = c.template at<float>(c.L.slab);
  g.cz = (int64_t)kGates * in;
  g.kchunk = (int)c.L.kchunk;
  if (int rc = launch_gemm(c.s, g, c.L.ksplit)) return rc;
  return colsum(c, g.C, c.L.ksplit, g.cz, g.cz, out);
}
