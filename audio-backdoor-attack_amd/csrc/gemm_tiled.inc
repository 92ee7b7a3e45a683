// The tile geometry and the choice of tile that gemm_tiled_kernel (gemm_tiled_kernel.inc: rnn.hip, smalllstm.hip) and
// largecnn.hip's conv_gemm_kernel share; included after the file's kT.  Those are the two texts of the tile loop:
// one shared body with the loaders as a compile-time policy compiled to a schedule 0.4 to 1.9 % slower per largecnn
// step (profiles/conv_core/equal.md).

constexpr int kBK = 32;            // K-step of the tiled kernels
constexpr int kSmallTile = 64, kLargeTile = 128;

typedef float f16v __attribute__((ext_vector_type(16)));

// The 128 tile when its grid (ceil(M / 128) x ceil(N / 128) x nz blocks) has at least min_blocks blocks, else
// the 64 tile, which fills more CUs.  small / large: the file's kernel at <1, 1> and <2, 2>.
template <class Args>
int launch_tiled(hipStream_t s, int M, int N, int nz, int min_blocks, void (*small)(Args), void (*large)(Args),
                 const Args& args) {
  const int64_t blocks = (int64_t)((M + kLargeTile - 1) / kLargeTile) * ((N + kLargeTile - 1) / kLargeTile) * nz;
  const int tile = blocks >= min_blocks ? kLargeTile : kSmallTile;
  const dim3 grid((M + tile - 1) / tile, (N + tile - 1) / tile, nz);
  (tile == kLargeTile ? large : small)<<<grid, kT, 0, s>>>(args);
  ABD_LAUNCH_CHECK();
  return ABD_OK;
}
