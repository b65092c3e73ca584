// umx_rowblocks.h -- the six float64 kernels of the Hessian-free solvers on umx_hvp (include/umx.h; the row-block algebra and its NumPy
// statements are pdb2reaction_amd/rowblocks.py, the solvers modes.py and dimer.py).  They work on plain device buffers of ROW vectors
// [p][n], n = 3 * n_atoms; no atomics, no fused multiply-add, 64-bit indexing: the bits depend on the inputs only, and the NumPy functions
// of rowblocks.py state the same operation orders and are held to these kernels bit for bit.
//
// Block kernels (umx_blk_*_dev) mix the rows of a block through a p x q matrix or a weight vector:
//   k_blk_gram     G[a][b] = sum_c X[a][c] * Y[b][c]: one 256-thread workgroup per entry, lane_tree_dot's order (k_hvp_curv's).  X == Y is
//                  allowed: a product commutes, so G[a][b] and G[b][a] are then the same sums of the same numbers in the same order.
//   k_blk_combine  Y[j][c] = Z[j][c] -+ sum_i C[i][j] * X[i][c]: one thread per (j, c); acc = Z[j][c] (0.0 without Z), then i = 0 ... p - 1
//                  ascending, acc = fl(acc -+ fl(C * X)).  Y may be Z (every thread reads its own element before it writes it), not X.
//   k_blk_scale    Y[a][c] = fl(w[c] * X[a][c]); in place allowed.
// Row kernels (umx_row_*_dev) treat K rows as K independent vectors with scalars of their own -- the DIAGONAL case, which through the
// block kernels would cost K^2 dots, K-fold products and a read-back of K^2 numbers; a row's result does not depend on the rows beside it:
//   k_row_dot      out[r] = sum_c X[r][c] * Y[r][c]: one workgroup per row through lane_tree_dot, so out[r] is k_blk_gram's G[r][r] bit for
//                  bit.  X == Y is allowed.
//   k_row_axpby    out[r][c] = fl(fl(a[r] * X[r][c]) + fl(b[r] * Y[r][c])), or fl(a[r] * X[r][c]) without (b, Y): one thread per element,
//                  which reads before it writes, so out may be X or Y.
//   k_row_absmax   out[r] = max_c |X[r][c]|, NaN when the row holds one (numpy.max(numpy.abs(x), axis=1)): a maximum does not depend on the
//                  order; lanes and tree are lane_tree_dot's.
//
// No fused multiply-add, and that takes more than __dmul_rn / __dadd_rn: the HIP headers define the two as plain `x * y` and `x + y`,
// inlined with the contraction the headers are compiled under, and the compiler does fuse them into v_fmac_f64 in a loop like
// lane_tree_dot's (from a lane's second product on -- n > 256 -- such a sum differs from the NumPy statement in the last bits).  So the
// code below writes * and + itself under `#pragma clang fp contract(off)`: every product is rounded before it is added.
//
// All six are memory-trivial next to the batched evaluation they sit beside: rows are read coalesced, nothing is tuned beyond that.
#pragma once

#include <initializer_list>

namespace umx {

constexpr int BLK_MAX = 64;          // rows of a block (p, q, k): the Rayleigh-Ritz matrix read back per iteration stays <= 64 x 64 doubles

// The 256 lanes' partials folded in the LDS tree s = 128 ... 1 (sp[t] = fold(sp[t], sp[t + s]) for t < s); every lane returns the result.
// ONE call per kernel: no barrier stands between a lane's read of the result and the next write to sp.
template <class Fold>
__device__ inline double tree_fold(double acc, Fold fold) {
  __shared__ double sp[256];
  const int t = threadIdx.x;
  sp[t] = acc;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (t < s) sp[t] = fold(sp[t], sp[t + s]);
    __syncthreads();
  }
  return sp[0];
}

// sum_c xr[c] * yr[c] by one 256-thread workgroup, THE summation order of a dot product here: lane t adds the rounded products c = t,
// t + 256, ... ascending from 0.0, then the tree.  xr and yr may alias (no __restrict__).
__device__ inline double lane_tree_dot(const double* xr, const double* yr, long n) {
#pragma clang fp contract(off)
  double acc = 0.0;
  for (long c = threadIdx.x; c < n; c += 256) acc = acc + xr[c] * yr[c];
  return tree_fold(acc, [](double u, double v) { return u + v; });
}

// the larger of two magnitudes; a NaN wins over any number
__device__ inline double absmax2(double u, double v) { return (u != u) ? u : ((v != v) ? v : (u > v ? u : v)); }

__global__ __launch_bounds__(256) void k_blk_gram(const double* x, const double* y, long q, long n, double* __restrict__ g) {
  const long e = blockIdx.x;
  const long a = e / q, b = e - a * q;
  const double sum = lane_tree_dot(x + a * n, y + b * n, n);
  if (threadIdx.x == 0) g[e] = sum;
}

__global__ __launch_bounds__(256) void k_row_dot(const double* x, const double* y, long n, double* __restrict__ out) {
  const long r = blockIdx.x;
  const double sum = lane_tree_dot(x + r * n, y + r * n, n);
  if (threadIdx.x == 0) out[r] = sum;
}

__global__ __launch_bounds__(256) void k_row_absmax(const double* __restrict__ x, long n, double* __restrict__ out) {
  const long r = blockIdx.x;
  const double* xr = x + r * n;
  double acc = 0.0;
  for (long c = threadIdx.x; c < n; c += 256) acc = absmax2(acc, fabs(xr[c]));
  acc = tree_fold(acc, [](double u, double v) { return absmax2(u, v); });
  if (threadIdx.x == 0) out[r] = acc;
}

// z may be nullptr or y itself (no __restrict__ on the two)
__global__ __launch_bounds__(256) void k_blk_combine(const double* __restrict__ x, const double* __restrict__ cm, const double* z, long p, long q, long n,
                                                    int subtract, double* y) {
#pragma clang fp contract(off)
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= q * n) return;
  const long j = i / n, c = i - j * n;
  double acc = z ? z[i] : 0.0;
  for (long r = 0; r < p; ++r) {
    const double t = cm[r * q + j] * x[r * n + c];
    acc = subtract ? acc - t : acc + t;
  }
  y[i] = acc;
}

// x may be y (no __restrict__ on the two)
__global__ __launch_bounds__(256) void k_blk_scale(const double* x, const double* __restrict__ w, long p, long n, double* y) {
#pragma clang fp contract(off)
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= p * n) return;
  y[i] = w[i % n] * x[i];
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

}  // namespace umx

namespace {

// the refusal the six entries share, the sizes: p and q rows of a block entry; a row entry (`row`) has p = k, q = 1 and speaks of k
int blk_check(umx_engine* eng, const char* who, int p, int q, long n, bool row = false) {
  const bool positive = p > 0 && q > 0 && n > 0;
  if (positive && p <= umx::BLK_MAX && q <= umx::BLK_MAX) return UMX_OK;
  const std::string sp = std::to_string(p), sq = std::to_string(q);
  const std::string sizes = row ? "k = " + sp : "p = " + sp + (positive ? " and q = " : ", q = ") + sq;
  return fail(eng, UMX_ERR_ARG, std::string(who) + ": " + sizes + (positive ? " must not exceed " + std::to_string(umx::BLK_MAX) + " rows"
                                                                             : " and n = " + std::to_string(n) + " must be positive"));
}

inline bool blk_overlap(const double* a, size_t na, const double* b, size_t nb) {
  const uintptr_t a0 = reinterpret_cast<uintptr_t>(a), b0 = reinterpret_cast<uintptr_t>(b);
  return a0 < b0 + nb * sizeof(double) && b0 < a0 + na * sizeof(double);
}

// The name of the first given operand that overlaps the output [out, out + n_out) -- `may_be`: an operand that IS the output does not
// count (a thread reads its own element before it writes it; a shifted overlap would race) --, or nullptr.
struct BlkOperand { const char* name; const double* p; size_t n; };
inline const char* blk_overlapped(const double* out, size_t n_out, std::initializer_list<BlkOperand> operands, bool may_be = false) {
  for (const BlkOperand& o : operands)
    if (o.p && !(may_be && o.p == out) && blk_overlap(out, n_out, o.p, o.n)) return o.name;
  return nullptr;
}

// what every entry ends with once nothing is left to refuse: `groups` workgroups of 256 threads on the caller's stream
template <class... P, class... A>
int blk_launch(umx_engine* eng, void (*kernel)(P...), unsigned groups, void* hip_stream, A... args) {
  HIPCHK(eng, hipSetDevice(eng->dev));
  hipLaunchKernelGGL(kernel, dim3(groups), dim3(256), 0, static_cast<hipStream_t>(hip_stream), static_cast<P>(args)...);
  HIPCHK(eng, hipGetLastError());
  return UMX_OK;
}

}  // namespace
