// The LSTM cell arithmetic shared by lstm_attn.hip and rnn.hip, on top of net_common.inc (GemmArgs, the host
// helpers, the cross entropy).  Included inside each file's anonymous namespace, after abd_common.h.  Each file
// keeps its recurrent kernels.

#include "net_common.inc"

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
