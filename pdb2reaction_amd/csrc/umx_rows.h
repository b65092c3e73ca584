// umx_rows.h -- the three float64 ROW kernels of a batched dimer on umx_hvp (umx_row_dot_dev / umx_row_axpby_dev / umx_row_absmax_dev,
// include/umx.h; the solver is pdb2reaction_amd/dimer.py).  umx_modes.h mixes the rows of a block through a p x q matrix; a batch of K
// independent saddle searches needs the DIAGONAL case -- K vectors [K][n], n = 3 * n_atoms, each with scalars of its own -- which through
// k_blk_gram / k_blk_combine would cost K^2 dots, K-fold products and a read-back of K^2 numbers.  Written as umx_modes.h is: plain device
// buffers, no atomics, no fused multiply-add (`#pragma clang fp contract(off)`; that header says why __dmul_rn is not enough), 64-bit
// indexing: the bits depend on the inputs only, and a row's result does not depend on the rows beside it.  The NumPy functions row_dot /
// row_axpby / row_absmax of dimer.py state the same operation orders and are held to these kernels bit for bit.
//
//   k_row_dot     out[r] = sum_c X[r][c] * Y[r][c]: one 256-thread workgroup per row in k_blk_gram's order -- lane t adds c = t, t + 256, ...
//                 ascending from 0.0, the 256 partials are added in the LDS tree s = 128 ... 1 -- so out[r] is k_blk_gram's G[r][r] bit for
//                 bit.  X == Y is allowed.
//   k_row_axpby   out[r][c] = fl(fl(a[r] * X[r][c]) + fl(b[r] * Y[r][c])), or fl(a[r] * X[r][c]) without (b, Y): one thread per element,
//                 which reads before it writes, so out may be X or Y.
//   k_row_absmax  out[r] = max_c |X[r][c]|, NaN when the row holds one (numpy.max(numpy.abs(x), axis=1)): a maximum does not depend on the
//                 order, the tree is k_row_dot's.
//
// All three are memory-trivial next to the batched evaluation they sit beside: rows are read coalesced, nothing is tuned beyond that.
#pragma once

namespace umx {

// x and y may alias (no __restrict__)
__global__ __launch_bounds__(256) void k_row_dot(const double* x, const double* y, long n, double* __restrict__ out) {
#pragma clang fp contract(off)
  __shared__ double sp[256];
  const long r = blockIdx.x;
  const int t = threadIdx.x;
  const double* xr = x + r * n;
  const double* yr = y + r * n;
  double acc = 0.0;
  for (long c = t; c < n; c += 256) acc = acc + xr[c] * yr[c];
  sp[t] = acc;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (t < s) sp[t] = sp[t] + sp[t + s];
    __syncthreads();
  }
  if (t == 0) out[r] = sp[0];
}

// out may be x or y (no __restrict__ on the three); b and y are both given or both nullptr
__global__ __launch_bounds__(256) void k_row_axpby(const double* __restrict__ a, const double* x, const double* __restrict__ b, const double* y, long k, long n,
                                                  double* out) {
#pragma clang fp contract(off)
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= k * n) return;
  const long r = i / n;
  const double ax = a[r] * x[i];
  if (y) {
    const double by = b[r] * y[i];
    out[i] = ax + by;
  } else {
    out[i] = ax;
  }
}

// the larger of two magnitudes; a NaN wins over any number
__device__ inline double absmax2(double u, double v) { return (u != u) ? u : ((v != v) ? v : (u > v ? u : v)); }

__global__ __launch_bounds__(256) void k_row_absmax(const double* __restrict__ x, long n, double* __restrict__ out) {
  __shared__ double sp[256];
  const long r = blockIdx.x;
  const int t = threadIdx.x;
  const double* xr = x + r * n;
  double acc = 0.0;
  for (long c = t; c < n; c += 256) acc = absmax2(acc, fabs(xr[c]));
  sp[t] = acc;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (t < s) sp[t] = absmax2(sp[t], sp[t + s]);
    __syncthreads();
  }
  if (t == 0) out[r] = sp[0];
}

}  // namespace umx

namespace {

// the refusals the three entries share: the sizes (k rows of a batch, at most BLK_MAX of them)
int row_check(umx_engine* eng, const char* who, int k, long n) {
  if (k <= 0 || n <= 0) return fail(eng, UMX_ERR_ARG, std::string(who) + ": k = " + std::to_string(k) + " and n = " + std::to_string(n) + " must be positive");
  if (k > umx::BLK_MAX) return fail(eng, UMX_ERR_ARG, std::string(who) + ": k = " + std::to_string(k) + " must not exceed " + std::to_string(umx::BLK_MAX) + " rows");
  return UMX_OK;
}

}  // namespace
