// umx_modes.h -- the three float64 block kernels of a matrix-free eigensolver on umx_hvp (umx_blk_gram_dev / umx_blk_combine_dev /
// umx_blk_scale_dev, include/umx.h; the solver is pdb2reaction_amd/modes.py).  They work on plain device buffers of ROW vectors [p][n],
// n = 3 * n_atoms; no atomics, no fused multiply-add, 64-bit indexing: the bits depend on the inputs only.  The NumPy functions
// blk_gram / blk_combine / blk_scale of modes.py state the same operation orders and are held to these kernels bit for bit.
//
//   k_blk_gram     G[a][b] = sum_c X[a][c] * Y[b][c]: one 256-thread workgroup per entry, k_hvp_curv's order -- lane t adds c = t, t + 256,
//                  ... ascending, the 256 partials are added in the LDS tree s = 128 ... 1.  X == Y is allowed: a product commutes, so
//                  G[a][b] and G[b][a] are then the same sums of the same numbers in the same order.
//   k_blk_combine  Y[j][c] = Z[j][c] -+ sum_i C[i][j] * X[i][c]: one thread per (j, c); acc = Z[j][c] (0.0 without Z), then i = 0 ... p - 1
//                  ascending, acc = fl(acc -+ fl(C * X)).  Y may be Z (every thread reads its own element before it writes it), not X.
//   k_blk_scale    Y[a][c] = fl(w[c] * X[a][c]); in place allowed.
//
// No fused multiply-add, and that takes more than __dmul_rn / __dadd_rn: the HIP headers define the two as plain `x * y` and `x + y`,
// inlined with the contraction the headers are compiled under, and the compiler does fuse them into v_fmac_f64 in a loop like
// k_blk_gram's (from a lane's second product on -- n > 256 -- such a sum differs from the NumPy statement in the last bits).  So the
// kernels below write * and + themselves under `#pragma clang fp contract(off)`: every product is rounded before it is added.
//
// All three are memory-trivial next to the batched evaluation they sit beside: rows are read coalesced, nothing is tuned beyond that.
#pragma once

namespace umx {

constexpr int BLK_MAX = 64;          // rows of a block (p, q): the Rayleigh-Ritz matrix read back per iteration stays <= 64 x 64 doubles

// x and y may alias (no __restrict__)
__global__ __launch_bounds__(256) void k_blk_gram(const double* x, const double* y, long q, long n, double* __restrict__ g) {
#pragma clang fp contract(off)
  __shared__ double sp[256];
  const long e = blockIdx.x;
  const long a = e / q, b = e - a * q;
  const int t = threadIdx.x;
  const double* xa = x + a * n;
  const double* yb = y + b * n;
  double acc = 0.0;
  for (long c = t; c < n; c += 256) acc = acc + xa[c] * yb[c];
  sp[t] = acc;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (t < s) sp[t] = sp[t] + sp[t + s];
    __syncthreads();
  }
  if (t == 0) g[e] = sp[0];
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

}  // namespace umx

namespace {

// the refusals the three entries share: the sizes
int blk_check(umx_engine* eng, const char* who, int p, int q, long n) {
  if (p <= 0 || q <= 0 || n <= 0)
    return fail(eng, UMX_ERR_ARG, std::string(who) + ": p = " + std::to_string(p) + ", q = " + std::to_string(q) + " and n = " + std::to_string(n) + " must be positive");
  if (p > umx::BLK_MAX || q > umx::BLK_MAX)
    return fail(eng, UMX_ERR_ARG, std::string(who) + ": p = " + std::to_string(p) + " and q = " + std::to_string(q) + " must not exceed " + std::to_string(umx::BLK_MAX) + " rows");
  return UMX_OK;
}

inline bool blk_overlap(const double* a, size_t na, const double* b, size_t nb) {
  const uintptr_t a0 = reinterpret_cast<uintptr_t>(a), b0 = reinterpret_cast<uintptr_t>(b);
  return a0 < b0 + nb * sizeof(double) && b0 < a0 + na * sizeof(double);
}

}  // namespace
