// umx_bonds.h -- bond-change EVENTS for many pairs of geometries in one call (umx_bond_events): the formed / broken pairs of
// k_bond_changes / k_bond_changes_cell as a compact list, without the N x N matrices.
//
// Three passes over the upper triangle (i < j) of every requested pair of geometries, one wave per row (pair p, atom i):
//   count  k_bond_count   the events among j > i of every row (ballot + popcount per 64 columns)        -> int32 counts[rows]
//   scan   k_bond_scan_*  exclusive prefix over the rows, 1024 rows per block, block sums by one block  -> int64 offsets[rows], pair_off
//   fill   k_bond_fill    the same traversal; an event goes to offsets[row] + its rank within the row (ballot, lanes below), so the
//                         list ascends in (pair, i, j); a store happens only for an index below the capacity, event by event
// No atomics: the order is fixed.  rows = n_pairs * n can exceed 2^31: rows, offsets and totals are 64-bit.
//
// The arithmetic is that of the two matrix kernels (umx_kernels.h), expression by expression -- explicit __dmul_rn / __dadd_rn /
// __dsub_rn sums in the same order, the same rint, the same candidate search with its early stop -- written once below as
// bond_distance<B> and bond_code, so an event's d1, d2 and code are the bits those kernels write at [i, j].
#pragma once
#include "umx_common.h"
#include "umx_kernels.h"        // BondCell
#include "umx_graph.h"          // lanes_below

namespace umx {

// the boundary tag of the bond kernels, as NoCells / Cells of the graph kernels
struct BondOpen {};
struct BondPeriodic { BondCell cell; const double* cand; int n_cand; };   // cand: [n_cand][4] (tx, ty, tz, lb2) of bond_cell_candidates

// D_ij of one geometry r [n][3]: k_bond_changes' dist (open) or k_bond_changes_cell's (minimum image over the candidate table)
template <typename B>
__device__ __forceinline__ double bond_distance(const B& bc, const double* __restrict__ r, size_t i, size_t j) {
  if constexpr (std::is_same_v<B, BondOpen>) {
    const double dx = r[i * 3 + 0] - r[j * 3 + 0], dy = r[i * 3 + 1] - r[j * 3 + 1], dz = r[i * 3 + 2] - r[j * 3 + 2];
    return sqrt(__dadd_rn(__dadd_rn(__dmul_rn(dx, dx), __dmul_rn(dy, dy)), __dmul_rn(dz, dz)));
  } else {
    auto sum3 = [](double x, double y, double z) { return __dadd_rn(__dadd_rn(x, y), z); };
    const BondCell& cell = bc.cell;
    const double dx = r[j * 3 + 0] - r[i * 3 + 0], dy = r[j * 3 + 1] - r[i * 3 + 1], dz = r[j * 3 + 2] - r[i * 3 + 2];
    double m[3];
    for (int k = 0; k < 3; ++k) m[k] = rint(sum3(__dmul_rn(dx, cell.b[k][0]), __dmul_rn(dy, cell.b[k][1]), __dmul_rn(dz, cell.b[k][2])));
    const double x0 = __dsub_rn(dx, sum3(__dmul_rn(m[0], cell.a[0][0]), __dmul_rn(m[1], cell.a[1][0]), __dmul_rn(m[2], cell.a[2][0])));
    const double y0 = __dsub_rn(dy, sum3(__dmul_rn(m[0], cell.a[0][1]), __dmul_rn(m[1], cell.a[1][1]), __dmul_rn(m[2], cell.a[2][1])));
    const double z0 = __dsub_rn(dz, sum3(__dmul_rn(m[0], cell.a[0][2]), __dmul_rn(m[1], cell.a[1][2]), __dmul_rn(m[2], cell.a[2][2])));
    double best = sum3(__dmul_rn(x0, x0), __dmul_rn(y0, y0), __dmul_rn(z0, z0));      // cand[0]: the zero translation
    for (int t = 1; t < bc.n_cand; ++t) {
      const double* c = bc.cand + (size_t)t * 4;
      if (c[3] > best) break;
      const double x = __dadd_rn(x0, c[0]), y = __dadd_rn(y0, c[1]), z = __dadd_rn(z0, c[2]);
      best = fmin(best, sum3(__dmul_rn(x, x), __dmul_rn(y, y), __dmul_rn(z, z)));
    }
    return sqrt(best);
  }
}

// the code of a pair i < j with lengths a (first geometry) and b (second): 1 = formed, 2 = broken, 0 = neither
__device__ __forceinline__ int bond_code(double a, double b, double ci, double cj, double bf, double mf, double df) {
  const double T = __dmul_rn(bf, __dadd_rn(ci, cj));
  const double thr = __dsub_rn(T, __dmul_rn(mf, T));
  const bool A1 = a <= thr, A2 = b <= thr;
  const bool need = fabs(__dsub_rn(b, a)) >= __dmul_rn(df, T);
  return need ? ((!A1 && A2) ? 1 : (A1 && !A2) ? 2 : 0) : 0;
}

// what both traversals read: geometries r [n_geoms][n][3], radii cov [n], the pairs (geom_a[p], geom_b[p]) -- range-checked on the
// host -- and the three fractions
struct BondJob {
  const double* r; const double* cov; const int* geom_a; const int* geom_b;
  int n; long rows;                                  // rows = n_pairs * n; row = p * n + i
  double bf, mf, df;
};

// One row's columns j > i, 64 at a time: f(j, code, a, b, in) runs on every lane, in = the lane has a column (code 0 otherwise).  The
// row is wave-uniform, so every ballot inside f sees the whole wave.  f returns false to stop the row.
template <typename B, typename F>
__device__ __forceinline__ void bond_row(const BondJob& jb, const B& bc, long row, int lane, F&& f) {
  const long p = row / jb.n;
  const size_t i = (size_t)(row - p * jb.n), n = (size_t)jb.n;
  const double* ra = jb.r + (size_t)jb.geom_a[p] * n * 3;
  const double* rb = jb.r + (size_t)jb.geom_b[p] * n * 3;
  const double ci = jb.cov[i];
  for (size_t j0 = i + 1; j0 < n; j0 += 64) {
    const size_t j = j0 + (size_t)lane;
    const bool in = j < n;
    double a = 0.0, b = 0.0;
    int c = 0;
    if (in) {
      a = bond_distance(bc, ra, i, j);
      b = bond_distance(bc, rb, i, j);
      c = bond_code(a, b, ci, jb.cov[j], jb.bf, jb.mf, jb.df);
    }
    if (!f((int)j, c, a, b)) break;
  }
}

// blocks of 4 waves stride over the rows (a grid of nblk(rows, 4) blocks, capped, covers them in one step in every practical call)
#define UMX_BOND_ROWS(row, rows)                                                                        \
  const int lane = threadIdx.x & 63;                                                                    \
  const long wave0 = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));                           \
  for (long row = (long)blockIdx.x * 4 + wave0; row < (rows); row += (long)gridDim.x * 4)

template <typename B>
__global__ __launch_bounds__(256) void k_bond_count(const BondJob jb, const B bc, int* __restrict__ counts) {
  UMX_BOND_ROWS(row, jb.rows) {
    int cnt = 0;
    bond_row(jb, bc, row, lane, [&](int, int c, double, double) { cnt += __popcll(__ballot(c != 0)); return true; });
    if (lane == 0) counts[row] = cnt;
  }
}

// rows with count 0 are skipped without a distance; a row stops after its last event, or once its next slot is past the capacity
template <typename B>
__global__ __launch_bounds__(256) void k_bond_fill(const BondJob jb, const B bc, const int* __restrict__ counts, const long long* __restrict__ offsets,
                                                   long long capacity, umx_bond_event* __restrict__ events) {
  UMX_BOND_ROWS(row, jb.rows) {
    const int cnt = counts[row];
    const long long base = offsets[row];
    if (cnt == 0 || base >= capacity) continue;
    const int p = (int)(row / jb.n), i = (int)(row - (long)p * jb.n);
    int w = 0;
    bond_row(jb, bc, row, lane, [&](int j, int c, double a, double b) {
      const unsigned long long m = __ballot(c != 0);
      if (c != 0) {
        const long long at = base + w + lanes_below(m, lane);
        if (at < capacity) {                                          // event by event: the one bound of the one indexed store
          umx_bond_event ev;
          ev.pair = p; ev.i = i; ev.j = j; ev.code = c; ev.d1 = a; ev.d2 = b;
          events[at] = ev;
        }
      }
      w += __popcll(m);
      return w < cnt && base + w < capacity;
    });
  }
}

// ---- the scan: counts[rows] int32 -> offsets[rows] int64 (exclusive), in three steps ------------------------------------------------
constexpr int BOND_SCAN = 1024;      // rows per block of the first step

// 1. every block scans its 1024 rows: offsets = the prefix within the block, block_sum[block] = its total
__global__ __launch_bounds__(BOND_SCAN) void k_bond_scan_rows(const int* __restrict__ counts, long rows, long long* __restrict__ offsets,
                                                              long long* __restrict__ block_sum) {
  __shared__ long long part[BOND_SCAN];
  const int t = threadIdx.x;
  const long row = (long)blockIdx.x * BOND_SCAN + t;
  const long long c = row < rows ? counts[row] : 0;
  part[t] = c;
  __syncthreads();
  for (int off = 1; off < BOND_SCAN; off <<= 1) {
    const long long v = (t >= off) ? part[t - off] : 0;
    __syncthreads();
    part[t] += v;
    __syncthreads();
  }
  if (row < rows) offsets[row] = part[t] - c;
  if (t == BOND_SCAN - 1) block_sum[blockIdx.x] = part[t];
}

// 2. k_scan's pattern (umx_graph.h) in 64 bits: ONE block turns block_sum[0..nb) into its exclusive prefix in place; *total = the sum
__global__ __launch_bounds__(1024) void k_bond_scan_blocks(long long* __restrict__ block_sum, long nb, long long* __restrict__ total) {
  __shared__ long long part[1024];
  const int t = threadIdx.x;
  const long chunk = (nb + 1023) / 1024;
  const long lo = t * chunk, hi = (lo + chunk < nb) ? lo + chunk : nb;
  long long s = 0;
  for (long i = lo; i < hi; ++i) s += block_sum[i];
  part[t] = s;
  __syncthreads();
  for (int off = 1; off < 1024; off <<= 1) {
    const long long v = (t >= off) ? part[t - off] : 0;
    __syncthreads();
    part[t] += v;
    __syncthreads();
  }
  long long run = (t == 0) ? 0 : part[t - 1];
  for (long i = lo; i < hi; ++i) { const long long v = block_sum[i]; block_sum[i] = run; run += v; }
  if (t == 1023) *total = part[1023];
}

// 3. add every block's base; the first row of pair p leaves its offset in pair_off[p] (pair_off[n_pairs] is step 2's total)
__global__ __launch_bounds__(256) void k_bond_scan_add(long long* __restrict__ offsets, long rows, const long long* __restrict__ block_base, int n,
                                                       long long* __restrict__ pair_off) {
  const long row = (long)blockIdx.x * 256 + threadIdx.x;
  if (row >= rows) return;
  const long long v = offsets[row] + block_base[row / BOND_SCAN];
  offsets[row] = v;
  if (row % n == 0) pair_off[row / n] = v;
}

}  // namespace umx

namespace {

// the three passes on the engine's stream; the tag B carries the cell.  *total and pair_off (host, [n_pairs + 1]) after the scan,
// then the first min(total, capacity) events to the host.
template <typename B>
int bond_events_passes(umx_engine* eng, const umx::BondJob& jb, const B& bc, long n_pairs, int* d_counts, long long* d_offsets, long long* d_blocks,
                       long long* d_pair_off, std::vector<long long>* pair_off, int64_t capacity, umx_bond_event* events) {
  hipStream_t s = eng->stream;
  for (hipEvent_t& e : eng->ev_bond) if (!e) HIPCHK(eng, hipEventCreate(&e));
  eng->bond_timed = false;
  const long rows = jb.rows, nb = (rows + umx::BOND_SCAN - 1) / umx::BOND_SCAN;
  const unsigned grid = (unsigned)std::min<long>((rows + 3) / 4, 1L << 22);
  HIPCHK(eng, hipEventRecord(eng->ev_bond[0], s));
  umx::k_bond_count<B><<<grid, 256, 0, s>>>(jb, bc, d_counts);
  HIPCHK(eng, hipGetLastError());
  HIPCHK(eng, hipEventRecord(eng->ev_bond[1], s));
  umx::k_bond_scan_rows<<<(unsigned)nb, umx::BOND_SCAN, 0, s>>>(d_counts, rows, d_offsets, d_blocks);
  HIPCHK(eng, hipGetLastError());
  umx::k_bond_scan_blocks<<<1, 1024, 0, s>>>(d_blocks, nb, d_pair_off + n_pairs);
  HIPCHK(eng, hipGetLastError());
  umx::k_bond_scan_add<<<nblk(rows, 256), 256, 0, s>>>(d_offsets, rows, d_blocks, jb.n, d_pair_off);
  HIPCHK(eng, hipGetLastError());
  HIPCHK(eng, hipEventRecord(eng->ev_bond[2], s));
  pair_off->resize((size_t)n_pairs + 1);
  HIPCHK(eng, hipMemcpyAsync(pair_off->data(), d_pair_off, pair_off->size() * sizeof(long long), hipMemcpyDeviceToHost, s));
  HIPCHK(eng, hipStreamSynchronize(s));
  const long long total = pair_off->back(), m = std::min<long long>(total, capacity);
  umx_bond_event* d_ev = nullptr;
  if (m > 0) {
    if (hipMalloc(&d_ev, (size_t)m * sizeof(umx_bond_event)) != hipSuccess)
      return fail(eng, UMX_ERR_HIP, "umx_bond_events: hipMalloc of " + std::to_string(m) + " events failed");
    umx::k_bond_fill<B><<<grid, 256, 0, s>>>(jb, bc, d_counts, d_offsets, m, d_ev);       // m, the size of d_ev, is the bound of the stores
  }
  int st = UMX_OK;
  auto ok = [&](hipError_t e, const char* what) { if (e != hipSuccess && st == UMX_OK) st = fail(eng, UMX_ERR_HIP, std::string(what) + ": " + hipGetErrorName(e)); };
  if (m > 0) ok(hipGetLastError(), "k_bond_fill");
  ok(hipEventRecord(eng->ev_bond[3], s), "record");
  if (m > 0) ok(hipMemcpyAsync(events, d_ev, (size_t)m * sizeof(umx_bond_event), hipMemcpyDeviceToHost, s), "copy the events");
  ok(hipStreamSynchronize(s), "sync");
  if (d_ev) (void)hipFree(d_ev);
  eng->bond_timed = st == UMX_OK;
  return st;
}

// umx_bond_events behind its argument checks: `cell` == nullptr runs the open kernels, else the minimum-image ones on `cand`
int bond_events_run(umx_engine* eng, int n, int n_geoms, const double* r, long n_pairs, const int32_t* ga, const int32_t* gb, const double* cov,
                    const umx::BondCell* cell, const std::vector<double>& cand, double bf, double mf, double df, int64_t capacity, umx_bond_event* events,
                    int64_t* n_events, int64_t* per_pair) {
  HIPCHK(eng, hipSetDevice(eng->dev));
  const long rows = n_pairs * (long)n, nb = (rows + umx::BOND_SCAN - 1) / umx::BOND_SCAN;
  const size_t n_r = (size_t)n_geoms * (size_t)n * 3, n_dbl = n_r + (size_t)n + cand.size();
  // one block of doubles (geometries, radii, candidates), one of int64 (offsets, block sums, pair offsets), one of int32 (counts, pairs)
  double* d_dbl = nullptr; long long* d_ll = nullptr; int* d_i = nullptr;
  const size_t n_ll = (size_t)rows + (size_t)nb + (size_t)n_pairs + 1, n_i = (size_t)rows + 2 * (size_t)n_pairs;
  hipError_t e0 = hipMalloc(&d_dbl, n_dbl * sizeof(double)), e1 = hipMalloc(&d_ll, n_ll * sizeof(long long)), e2 = hipMalloc(&d_i, n_i * sizeof(int));
  auto release = [&] { if (d_dbl) (void)hipFree(d_dbl); if (d_ll) (void)hipFree(d_ll); if (d_i) (void)hipFree(d_i); };
  if (e0 != hipSuccess || e1 != hipSuccess || e2 != hipSuccess) {
    release();
    return fail(eng, UMX_ERR_HIP, "umx_bond_events: hipMalloc of the geometries and row counters failed");
  }
  double* d_cov = d_dbl + n_r; double* d_cand = d_cov + n;
  long long *d_offsets = d_ll, *d_blocks = d_ll + rows, *d_pair_off = d_blocks + nb;
  int *d_counts = d_i, *d_ga = d_i + rows, *d_gb = d_ga + n_pairs;
  hipStream_t s = eng->stream;
  int st = UMX_OK;
  auto ok = [&](hipError_t e, const char* what) { if (e != hipSuccess && st == UMX_OK) st = fail(eng, UMX_ERR_HIP, std::string(what) + ": " + hipGetErrorName(e)); };
  ok(hipMemcpyAsync(d_dbl, r, n_r * sizeof(double), hipMemcpyHostToDevice, s), "copy the geometries");
  ok(hipMemcpyAsync(d_cov, cov, (size_t)n * sizeof(double), hipMemcpyHostToDevice, s), "copy cov");
  if (cell) ok(hipMemcpyAsync(d_cand, cand.data(), cand.size() * sizeof(double), hipMemcpyHostToDevice, s), "copy the candidate translations");
  ok(hipMemcpyAsync(d_ga, ga, (size_t)n_pairs * sizeof(int), hipMemcpyHostToDevice, s), "copy geom_a");
  ok(hipMemcpyAsync(d_gb, gb, (size_t)n_pairs * sizeof(int), hipMemcpyHostToDevice, s), "copy geom_b");
  std::vector<long long> pair_off;
  if (st == UMX_OK) {
    const umx::BondJob jb{d_dbl, d_cov, d_ga, d_gb, n, rows, bf, mf, df};
    if (cell) st = bond_events_passes(eng, jb, umx::BondPeriodic{*cell, d_cand, (int)(cand.size() / 4)}, n_pairs, d_counts, d_offsets, d_blocks, d_pair_off, &pair_off, capacity, events);
    else st = bond_events_passes(eng, jb, umx::BondOpen{}, n_pairs, d_counts, d_offsets, d_blocks, d_pair_off, &pair_off, capacity, events);
  }
  (void)hipStreamSynchronize(s);                       // the pageable host copies above have been consumed before ga / gb / r go out of the caller's hands
  release();
  if (st != UMX_OK) return st;
  *n_events = (int64_t)pair_off.back();
  if (per_pair) for (long p = 0; p < n_pairs; ++p) per_pair[p] = (int64_t)(pair_off[(size_t)p + 1] - pair_off[(size_t)p]);
  return UMX_OK;
}

}  // namespace
