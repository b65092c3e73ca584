// umx_graph.h -- K1, the neighbour graph: the wrap into the cell, the degree pass, the scan, the fill (and the replay of a pinned
// graph in its place), the out-edge lists.  A wrong graph is not a rounding error but another model, so every piece of arithmetic a
// decision rests on is written ONCE here: the edge vector of a candidate (open_delta / pbc_delta), its squared distance (dist2_f), the
// candidate test and its rank key (candidate), the wrap (wrap_count / wrap_by), the store of an edge (store_edge).
//
// A kernel is instantiated for the position type P (float, or double: umx_energy_forces_f64) and for the boundary argument B: NoCells
// (open boundaries) or Cells<P> (umx_set_cell / umx_set_cells).  The host side is umx_periodic.h.
#pragma once
#include <type_traits>
#include "umx_common.h"         // UMX_WAVE_ITEM

namespace umx {

// one definition of the squared distance so every site rounds identically (the candidate ranking compares them)
__device__ __forceinline__ float dist2_f(float dx, float dy, float dz) { return fmaf(dz, dz, fmaf(dy, dy, dx * dx)); }

// ------------------------------------------------------------------------------------------------
// Periodic boundary conditions: what the periodic instantiations read.  Built on the host in float64 from the cell (umx_periodic.h),
// one entry per bound cell in device memory.  A candidate of target i is (source j, translation t) with 0 < |r_j + t - r_i| <= cutoff;
// t runs over the table, entry k = ((na + Na) (2 Nb + 1) + (nb + Nb)) (2 Nc + 1) + (nc + Nc) for t = na a + nb b + nc c, |n| <= N per
// periodic axis (N = 0 on an open axis).  The kernels read positions WRAPPED into the cell (k_wrap_cell), so the fractional
// coordinates of two atoms differ by less than one along every periodic axis.
// ------------------------------------------------------------------------------------------------
constexpr int GF_MAXC = 1024;                     // candidates the truncating fill ranks in LDS (see k_graph_fill)
constexpr int PBC_MAX_AXIS = 4;                   // the cap: lattice translations -4 .. +4 per periodic axis
constexpr int PBC_MAX_SHIFTS = 729;               // (2 * PBC_MAX_AXIS + 1)^3 table entries
struct Periodic {
  float a[3][3];          // lattice vectors (rows); zero for an open axis
  float b[3][3];          // dual vectors of the periodic sub-lattice: fractional coordinate k = r . b[k]; zero for an open axis
  float gmax[3];          // pruning: a translated cell whose nearest face is more than gmax[k] (fractional, cutoff / plane distance + margin) away is skipped
  int n_shifts, zero;     // table entries, index of the zero translation
  const float4* shifts;   // (tx, ty, tz, bits of (na + 8) | (nb + 8) << 8 | (nc + 8) << 16); points into one packed buffer for all cells
};
// Double positions: the lattice and the dual vectors once more, in float64.  The wrap and the translation of a candidate are formed
// from these; the table, the pruning and everything that is decided on the rounded edge vector stay with the float32 struct.
struct Lattice64 {
  double a[3][3];         // lattice vectors (rows); zero for an open axis
  double b[3][3];         // dual vectors, as Periodic::b
};
struct NoLattice {};      // P = float: the table entry IS the translation

// The boundary argument of a kernel.  Open boundaries: an empty tag.  Cells: the device array of the bound cells; image k of the
// launch reads cell img0 + stride * k -- stride 1 and img0 the index within the call of the launch's first image (a chunk, a lane, one
// partitioned image) for per-image cells (umx_set_cells), stride 0 and img0 0 for the one cell all images share (umx_set_cell).
struct NoCells {};
template <typename P> struct Cells;
template <> struct Cells<float> { const Periodic* cells; int img0, stride; };
template <> struct Cells<double> { const Periodic* cells; const Lattice64* lats; int img0, stride; };   // lats: one per cell, next to cells
template <typename B> constexpr bool is_periodic = !std::is_same_v<B, NoCells>;

template <typename P> __device__ __forceinline__ int cell_index(const Cells<P>& c, long image) { return c.img0 + c.stride * (int)image; }
// the lattice a position of type P is wrapped in: a and b in P's own precision
__device__ __forceinline__ const Periodic& lattice_of(const Cells<float>& c, int k) { return c.cells[k]; }
__device__ __forceinline__ const Lattice64& lattice_of(const Cells<double>& c, int k) { return c.lats[k]; }

// The cell of a wave's node, image = node / natoms of the launch.  The cell index is wave-uniform, and taken through readfirstlane so
// that the struct (and, through its `shifts`, the table entries) arrive through scalar loads, as a kernel argument does.
template <typename P> struct WaveCell {
  Periodic per;
  std::conditional_t<std::is_same_v<P, double>, Lattice64, NoLattice> lat;
};
template <typename P>
__device__ __forceinline__ WaveCell<P> cell_of_image(const Cells<P>& c, long image) {
  const int k = __builtin_amdgcn_readfirstlane(cell_index(c, image));
  if constexpr (std::is_same_v<P, double>) return {c.cells[k], c.lats[k]};
  else return {c.cells[k], {}};
}

// ---- the edge vector of a candidate ----------------------------------------------------------------------------------------------
// periodic, float positions: the float32 difference plus the table entry (the lattice argument is not read)
template <typename L>
__device__ __forceinline__ void pbc_delta(const float* __restrict__ pj, float xi, float yi, float zi, const float4 sh, const L&, float& dx, float& dy, float& dz) {
  dx = (pj[0] - xi) + sh.x; dy = (pj[1] - yi) + sh.y; dz = (pj[2] - zi) + sh.z;
}
// periodic, double positions: the translation n_a a + n_b b + n_c c in float64 from the integer triple packed in sh.w and the float64
// lattice, r_j + t - r_i in float64, ONE rounding to float32 -- from there on the candidate is decided and stored as above
__device__ __forceinline__ void pbc_delta(const double* __restrict__ pj, double xi, double yi, double zi, const float4 sh, const Lattice64& lat, float& dx, float& dy, float& dz) {
  const unsigned code = __float_as_uint(sh.w);
  const double na = (double)((int)(code & 255u) - 8), nb = (double)((int)((code >> 8) & 255u) - 8), nc = (double)((int)((code >> 16) & 255u) - 8);
  dx = (float)((pj[0] + fma(nc, lat.a[2][0], fma(nb, lat.a[1][0], na * lat.a[0][0]))) - xi);
  dy = (float)((pj[1] + fma(nc, lat.a[2][1], fma(nb, lat.a[1][1], na * lat.a[0][1]))) - yi);
  dz = (float)((pj[2] + fma(nc, lat.a[2][2], fma(nb, lat.a[1][2], na * lat.a[0][2]))) - zi);
}
// open boundaries: the difference in the positions' own type, rounded to float32 (P = float: nothing to round).  No zero translation
// is added: -0.0f + 0.0f would be +0.0f in evec.
template <typename P>
__device__ __forceinline__ float open_delta(P a, P b) { return (float)(a - b); }

// ---- the wrap ----------------------------------------------------------------------------------------------------------------------
// n_k = floor(fractional coordinate k) and r - (n_a a + n_b b + n_c c), over a lattice view L with a and b in T (Periodic and float,
// Lattice64 and double).  k_wrap_cell applies both, k_wrap_index keeps n, k_graph_replay applies the kept n in the cell at hand: the
// pinned replay is right because these are the same expressions.  n = 0 leaves the coordinate bits as they are.
template <typename L, typename T>
__device__ __forceinline__ void wrap_count(const L& lat, T x, T y, T z, T n[3]) {
#pragma unroll
  for (int k = 0; k < 3; ++k) n[k] = floor(fma(z, (T)lat.b[k][2], fma(y, (T)lat.b[k][1], x * (T)lat.b[k][0])));
}
template <typename L, typename T>
__device__ __forceinline__ void wrap_by(const L& lat, const T n[3], T& x, T& y, T& z) {
  x = x - fma(n[2], (T)lat.a[2][0], fma(n[1], (T)lat.a[1][0], n[0] * (T)lat.a[0][0]));
  y = y - fma(n[2], (T)lat.a[2][1], fma(n[1], (T)lat.a[1][1], n[0] * (T)lat.a[0][1]));
  z = z - fma(n[2], (T)lat.a[2][2], fma(n[1], (T)lat.a[1][2], n[0] * (T)lat.a[0][2]));
}

// wrap every atom into the cell of its image along the periodic axes (a scratch copy only the graph kernels read: a per-atom lattice
// translation changes no edge vector, hence no energy or force).  A thread per atom: a wave may span two images, so here the cell
// comes in through vector loads.
template <typename P>
__global__ void k_wrap_cell(const P* __restrict__ pos, P* __restrict__ out, long nt, int natoms, const Cells<P> cells) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nt) return;
  const auto& lat = lattice_of(cells, cell_index(cells, i / natoms));
  P x = pos[i * 3 + 0], y = pos[i * 3 + 1], z = pos[i * 3 + 2], n[3];
  wrap_count(lat, x, y, z, n);
  wrap_by(lat, n, x, y, z);
  out[i * 3 + 0] = x; out[i * 3 + 1] = y; out[i * 3 + 2] = z;
}
// the wrap offsets of k_wrap_cell as integers: out[3 i + k] = n_k of atom i.  Run once, by the pinning call.
template <typename P>
__global__ void k_wrap_index(const P* __restrict__ pos, int* __restrict__ out, long nt, int natoms, const Cells<P> cells) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nt) return;
  P n[3];
  wrap_count(lattice_of(cells, cell_index(cells, i / natoms)), pos[i * 3 + 0], pos[i * 3 + 1], pos[i * 3 + 2], n);
#pragma unroll
  for (int k = 0; k < 3; ++k) out[i * 3 + k] = (int)n[k];
}

// ---- wave helpers ------------------------------------------------------------------------------------------------------------------
// Publish what the wave wrote to its own LDS slice to its own later reads.  The slice is private to the wave and its DS operations
// execute in order: only the compiler must not move the reads up.
__device__ __forceinline__ void wave_lds_publish() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
// set lanes of a ballot below this lane: the lane's place in a ballot compaction
__device__ __forceinline__ int lanes_below(unsigned long long m, int lane) { return __popcll(m & ((1ull << lane) - 1ull)); }

// one edge: source, target, unit vector and distance from the edge vector and its squared distance
__device__ __forceinline__ void store_edge(int* __restrict__ esrc, int* __restrict__ edst, float* __restrict__ evec, long slot, int src, int dst,
                                           float dx, float dy, float dz, float d2) {
  const float d = sqrtf(d2), inv = 1.0f / d;
  esrc[slot] = src;
  edst[slot] = dst;
  *reinterpret_cast<float4*>(evec + slot * 4) = make_float4(dx * inv, dy * inv, dz * inv, d);
}

// The translations that can reach the target at (x, y, z) within the cutoff, compacted in ascending index order into the wave's
// LDS slice `act`; returns their number.  Wave-uniform decision per translation: the translated cell holds fractional coordinates
// [n, n + 1) along axis k, the target sits at f, so every source of that image is at least gap = max(n - f, f - (n + 1), 0) plane
// distances away.  The margin inside gmax covers the float32 rounding of the wrap and of f (1e-3 of a plane distance against 1e-6).
__device__ __forceinline__ int pbc_active_shifts(const Periodic& per, float x, float y, float z, int lane, unsigned short* act) {
  float f[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) f[k] = fmaf(z, per.b[k][2], fmaf(y, per.b[k][1], x * per.b[k][0]));
  int na = 0;
  for (int t0 = 0; t0 < per.n_shifts; t0 += 64) {
    const int t = t0 + lane;
    bool ok = t < per.n_shifts;
    if (ok) {
      const unsigned code = __float_as_uint(per.shifts[t].w);
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        const float n = (float)((int)((code >> (8 * k)) & 255u) - 8);
        const float gap = fmaxf(fmaxf(n - f[k], f[k] - (n + 1.0f)), 0.0f);
        ok = ok && gap <= per.gmax[k];
      }
    }
    const unsigned long long m = __ballot(ok);
    if (ok) act[na + lanes_below(m, lane)] = (unsigned short)t;
    na += __popcll(m);
  }
  wave_lds_publish();
  return na;
}

// ---- the target of a wave and its candidates ---------------------------------------------------------------------------------------
// The boundary policy: what a wave knows of its target node, which translations it searches, how the edge vector of (source j,
// translation t) is formed, which candidate is the node itself, and the low word of the rank key.
// Open boundaries: ONE translation, which is absent -- no table, no LDS; the plain difference.
template <typename P> struct OpenTarget {
  const P* img;           // the positions of the node's image
  P xi, yi, zi;
  int natoms, self;       // self: the node within its image
  __device__ __forceinline__ int n_active() const { return 1; }
  __device__ __forceinline__ int active(int) const { return 0; }
  __device__ __forceinline__ float4 shift(int) const { return make_float4(0.f, 0.f, 0.f, 0.f); }   // (not read)
  __device__ __forceinline__ void delta(int j, const float4, float& dx, float& dy, float& dz) const {
    dx = open_delta(img[(long)j * 3 + 0], xi); dy = open_delta(img[(long)j * 3 + 1], yi); dz = open_delta(img[(long)j * 3 + 2], zi);
  }
  __device__ __forceinline__ bool is_self(int j, int) const { return j == self; }
  __device__ __forceinline__ unsigned index(int j, int) const { return (unsigned)j; }
};
// Cells: the translations of the node's cell that can reach it (pbc_active_shifts, a conservative filter: on the rounded coordinate for
// P = double); pos is the wrapped copy.  An atom's own image (t != 0) is an edge.  Equal-distance images of one source cannot tie: the
// key carries translation index * natoms + source.
template <typename P> struct CellTarget {
  const P* img;
  P xi, yi, zi;
  int natoms, self;
  WaveCell<P> cell;
  const unsigned short* act;   // the wave's LDS slice: active translations, ascending
  int na;
  __device__ __forceinline__ int n_active() const { return na; }
  __device__ __forceinline__ int active(int a) const { return __builtin_amdgcn_readfirstlane((int)act[a]); }
  __device__ __forceinline__ float4 shift(int t) const { return cell.per.shifts[t]; }
  __device__ __forceinline__ void delta(int j, const float4 sh, float& dx, float& dy, float& dz) const {
    pbc_delta(img + (long)j * 3, xi, yi, zi, sh, cell.lat, dx, dy, dz);
  }
  __device__ __forceinline__ bool is_self(int j, int t) const { return j == self && t == cell.per.zero; }
  __device__ __forceinline__ unsigned index(int j, int t) const { return (unsigned)t * (unsigned)natoms + (unsigned)j; }
};
template <typename P>
__device__ __forceinline__ OpenTarget<P> make_target(const NoCells&, const P* __restrict__ pos, long node, int natoms, P xi, P yi, P zi, int) {
  const long base = (node / natoms) * natoms;
  return {pos + base * 3, xi, yi, zi, natoms, (int)(node - base)};
}
template <typename P>
__device__ __forceinline__ CellTarget<P> make_target(const Cells<P>& cells, const P* __restrict__ pos, long node, int natoms, P xi, P yi, P zi, int lane) {
  __shared__ unsigned short act_s[4][PBC_MAX_SHIFTS];
  unsigned short* act = act_s[threadIdx.x >> 6];
  const long image = node / natoms, base = image * natoms;
  CellTarget<P> tg{pos + base * 3, xi, yi, zi, natoms, (int)(node - base), cell_of_image(cells, image), act, 0};
  tg.na = pbc_active_shifts(tg.cell.per, (float)xi, (float)yi, (float)zi, lane, act);
  return tg;
}

// THE candidate (source j, translation t, table entry sh) of a target: its edge vector, its squared distance as the high word of the
// rank key (d^2 bits << 32 | index: unique, ordered like the oracle's stable argsort), and whether it is one: 0 < d <= cutoff, not
// the node itself.  The degree pass and every path of the fill decide through this one function, so the rows the count sized are the
// rows the fill writes.
template <typename T>
__device__ __forceinline__ bool candidate(const T& tg, int j, int t, const float4 sh, float rc2, float& dx, float& dy, float& dz, unsigned long long& key) {
  tg.delta(j, sh, dx, dy, dz);
  const float d2 = dist2_f(dx, dy, dz);
  key = ((unsigned long long)__float_as_uint(d2) << 32) | tg.index(j, t);
  return (d2 <= rc2) && (d2 > 0.0f) && !tg.is_self(j, t);
}
__device__ __forceinline__ float key_d2(unsigned long long key) { return __uint_as_float((unsigned)(key >> 32)); }

// The loop nest over (active translations x sources, 64 sources at a time): f(j, ok, dx, dy, dz, key) for every lane of every step, in
// ascending (translation index, source) order; ok is false beyond the image's last atom.  t and sh are wave-uniform (scalar loads).
template <typename T, typename F>
__device__ __forceinline__ void for_candidates(const T& tg, float rc2, int lane, F&& f) {
  for (int a = 0; a < tg.n_active(); ++a) {
    const int t = tg.active(a);
    const float4 sh = tg.shift(t);
    for (int j0 = 0; j0 < tg.natoms; j0 += 64) {
      const int j = j0 + lane;
      float dx = 0.f, dy = 0.f, dz = 0.f;
      unsigned long long key = 0ull;
      const bool ok = j < tg.natoms && candidate(tg, j, t, sh, rc2, dx, dy, dz, key);
      f(j, ok, dx, dy, dz, key);
    }
  }
}

// Every key of the wave's LDS slice ranked among the others with broadcast reads (c^2 / 64 compares per lane): f(have, key, rank), 64
// keys at a time in slice order.  Keys are unique, so ranks are.
template <typename F>
__device__ __forceinline__ void for_ranked_keys(const unsigned long long* keys, int c, int lane, F&& f) {
  for (int c0 = 0; c0 < c; c0 += 64) {
    const int ci = c0 + lane;
    const bool have = ci < c;
    const unsigned long long k = have ? keys[ci] : ~0ull;
    int rank = 0;
    for (int q = 0; q < c; ++q) rank += keys[q] < k ? 1 : 0;
    f(have, k, rank);
  }
}

// ------------------------------------------------------------------------------------------------
// The degree pass: brute force inside each image, wave per target.  pos: [NT][3] in P; for P = double the edge vector is the float64
// difference rounded once to float32, and everything decided on it (d^2, the cutoff test, the rank key) is float32 arithmetic.
// [lo, hi): the target nodes whose incoming edges this engine builds (all of them normally; one rank's share in the graph-parallel
// single-image mode, where every other node gets an empty row).
// flag: the engine's sticky status word.  Bit 1: a non-finite coordinate (every comparison with it is false, so the atom would just
// lose its edges); the device-pointer entries read the word right behind this kernel and refuse the evaluation.  Bit 2 (cells): a
// target has more candidates than the truncating fill can rank (GF_MAXC) while max_neigh binds -- refused by the host.
// ------------------------------------------------------------------------------------------------
template <typename P, typename B>
__global__ __launch_bounds__(256) void k_graph_count(const P* __restrict__ pos, int natoms, long nt, float rc2, int max_neigh,
                                                     int* __restrict__ deg, int* __restrict__ cand, long lo, long hi, int* __restrict__ flag,
                                                     const B cells) {
  UMX_WAVE_ITEM(node, nt)
  const P xi = pos[node * 3 + 0], yi = pos[node * 3 + 1], zi = pos[node * 3 + 2];
  if (lane == 0 && !(isfinite(xi) && isfinite(yi) && isfinite(zi))) atomicOr(flag, 2);
  if (node < lo || node >= hi) {                 // wave-uniform
    if (lane == 0) { cand[node] = 0; deg[node] = 0; }
    return;
  }
  const auto tg = make_target(cells, pos, node, natoms, xi, yi, zi, lane);
  int cnt = 0;
  for_candidates(tg, rc2, lane, [&](int, bool ok, float, float, float, unsigned long long) { cnt += __popcll(__ballot(ok)); });
  if constexpr (is_periodic<B>)
    if (lane == 0 && cnt > max_neigh && cnt > GF_MAXC) atomicOr(flag, 4);
  if (lane == 0) { cand[node] = cnt; deg[node] = cnt < max_neigh ? cnt : max_neigh; }
}

// exclusive scan of deg[0..n) into row_ptr[0..n]; single block of 1024 threads; also max degree
__global__ __launch_bounds__(1024) void k_scan(const int* __restrict__ deg, long n, int* __restrict__ row_ptr,
                                               int* __restrict__ stats /*[0]=total,[1]=maxdeg*/) {
  __shared__ int part[1024];
  __shared__ int pmax[1024];
  const int t = threadIdx.x;
  const long chunk = (n + 1023) / 1024;
  const long lo = t * chunk, hi = (lo + chunk < n) ? lo + chunk : n;
  int s = 0, mx = 0;
  for (long i = lo; i < hi; ++i) { s += deg[i]; mx = deg[i] > mx ? deg[i] : mx; }
  part[t] = s; pmax[t] = mx;
  __syncthreads();
  for (int off = 1; off < 1024; off <<= 1) {
    int v = (t >= off) ? part[t - off] : 0;
    int m = (t >= off) ? pmax[t - off] : 0;
    __syncthreads();
    part[t] += v; pmax[t] = pmax[t] > m ? pmax[t] : m;
    __syncthreads();
  }
  int run = (t == 0) ? 0 : part[t - 1];
  for (long i = lo; i < hi; ++i) { row_ptr[i] = run; run += deg[i]; }
  if (t == 1023) { row_ptr[n] = part[1023]; stats[0] = part[1023]; stats[1] = pmax[1023]; }
}

// ------------------------------------------------------------------------------------------------
// The fill: the rows the degree pass sized, written.  A target with more than max_neigh candidates keeps its max_neigh nearest (rank
// by key: (d^2, index), the oracle's stable argsort).  With a binding cap EVERY atom takes that path, so the wave compacts the
// target's keys into its own LDS slice and ranks each against the others (for_ranked_keys).
// TRUNC = false (the common case: the host knows the batch's largest candidate count, read with the edge counts, and it is below
// max_neigh): no truncation code, and for open boundaries NO LDS -- the static 32-KiB key array would cap the resident blocks of this
// HBM-bound kernel on every launch for a path that is never taken.
// Open boundaries: rows in ascending source order, by ballot compaction.  The truncating form writes the kept keys in slice order,
// which is source order.  More than GF_MAXC candidates (> 1 atom / A^3 at a 6 A cutoff) take the slow form inside the plain loop: every
// candidate is ranked by a scan of the whole image, ties to the lower source.
// Cells: rows in ascending (source, translation index) order.  The truncating form finds the key of rank max_neigh - 1 (kth) and keeps
// every candidate up to it; then (both forms) every lane counts the kept candidates of its source over the active translations, a
// prefix sum over the lanes gives its first slot, and it writes them in translation order.  More than GF_MAXC candidates under a
// binding cap: the degree pass has refused.
// TOUT = true (cells only; the pinning calls umx_pin_graph / umx_pin_graphs alone): etr[slot] receives the translation the edge took, as the bits of its
// table entry's w ((na + 8) | (nb + 8) << 8 | (nc + 8) << 16).
// ------------------------------------------------------------------------------------------------
template <bool TRUNC, bool TOUT, typename P, typename B>
__global__ __launch_bounds__(256) void k_graph_fill(const P* __restrict__ pos, int natoms, long nt, float rc2, int max_neigh,
                                                    const int* __restrict__ cand, const int* __restrict__ row_ptr, int* __restrict__ esrc,
                                                    int* __restrict__ edst, float* __restrict__ evec, long lo, long hi, const B cells,
                                                    int* __restrict__ etr) {
  constexpr bool PBC = is_periodic<B>;
  static_assert(PBC || !TOUT, "open boundaries have no translation to report");
  UMX_WAVE_ITEM(node, nt)
  if (node < lo || node >= hi) return;           // wave-uniform: rows outside the owned target range are empty
  const long base = (node / natoms) * natoms;
  const auto tg = make_target(cells, pos, node, natoms, pos[node * 3 + 0], pos[node * 3 + 1], pos[node * 3 + 2], lane);
  const int nc = cand[node];
  const bool truncate = TRUNC && nc > max_neigh;
  int w = row_ptr[node];
  unsigned long long kth = ~0ull;                                      // cells: the largest key kept
  if constexpr (TRUNC) if (truncate && (PBC || nc <= GF_MAXC)) {       // wave-uniform
    __shared__ unsigned long long gf_keys[4][GF_MAXC];
    unsigned long long* keys = gf_keys[threadIdx.x >> 6];
    int c = 0;
    for_candidates(tg, rc2, lane, [&](int, bool ok, float, float, float, unsigned long long key) {
      const unsigned long long m = __ballot(ok);
      const int at = c + lanes_below(m, lane);
      if (ok && (!PBC || at < GF_MAXC)) keys[at] = key;                // open: the count is nc <= GF_MAXC
      c += __popcll(m);
    });
    if constexpr (PBC) c = c < GF_MAXC ? c : GF_MAXC;
    wave_lds_publish();
    for_ranked_keys(keys, c, lane, [&](bool have, unsigned long long k, int rank) {
      if constexpr (PBC) {
        const unsigned long long m = __ballot(have && rank == max_neigh - 1);     // at most one lane
        if (m) {
          const int from = __ffsll((long long)m) - 1;
          const unsigned hi32 = __shfl((unsigned)(k >> 32), from, 64), lo32 = __shfl((unsigned)(k & 0xffffffffull), from, 64);
          kth = ((unsigned long long)hi32 << 32) | lo32;
        }
      } else {
        const bool keep = have && rank < max_neigh;
        const unsigned long long m = __ballot(keep);
        if (keep) {
          const int j = (int)(unsigned)(k & 0xffffffffull);
          float dx, dy, dz;
          tg.delta(j, tg.shift(0), dx, dy, dz);
          store_edge(esrc, edst, evec, w + lanes_below(m, lane), (int)(base + j), (int)node, dx, dy, dz, key_d2(k));
        }
        w += __popcll(m);
      }
    });
    if constexpr (!PBC) return;
  }
  if constexpr (PBC) {
    const int wend = row_ptr[node + 1];
    for (int j0 = 0; j0 < natoms; j0 += 64) {
      const int j = j0 + lane;
      int mine = 0;
      if (j < natoms)
#pragma clang loop vectorize(disable) interleave(disable)   // (two translations per lane would come out as packed-fp32 instructions: build.py refuses them)
        for (int a = 0; a < tg.na; ++a) {
          const int t = tg.act[a];
          float dx, dy, dz;
          unsigned long long key;
          if (candidate(tg, j, t, tg.shift(t), rc2, dx, dy, dz, key) && key <= kth) ++mine;
        }
      int incl = mine;                                                 // inclusive prefix sum over the lanes
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) { const int v = __shfl_up(incl, o, 64); if (lane >= o) incl += v; }
      int slot = w + incl - mine;
      if (mine)
#pragma clang loop vectorize(disable) interleave(disable)
        for (int a = 0; a < tg.na; ++a) {
          const int t = tg.act[a];
          float dx, dy, dz;
          unsigned long long key;
          if (candidate(tg, j, t, tg.shift(t), rc2, dx, dy, dz, key) && key <= kth && slot < wend) {
            store_edge(esrc, edst, evec, slot, (int)(base + j), (int)node, dx, dy, dz, key_d2(key));
            if constexpr (TOUT) etr[slot] = (int)__float_as_uint(tg.shift(t).w);
            ++slot;
          }
        }
      w += __shfl(incl, 63, 64);
    }
  } else {
    for_candidates(tg, rc2, lane, [&](int j, bool ok, float dx, float dy, float dz, unsigned long long key) {
      const float d2 = key_d2(key);
      if (truncate && __ballot(ok)) {                                  // the slow form
        int rank = 0;
        for (int q0 = 0; q0 < natoms; q0 += 64) {
          const int q = q0 + lane;
          float e2 = -1.0f;                                            // -1 marks "not a candidate"
          float ex, ey, ez;
          unsigned long long qkey;
          if (q < natoms && candidate(tg, q, 0, tg.shift(0), rc2, ex, ey, ez, qkey)) e2 = key_d2(qkey);
          for (int l = 0; l < 64; ++l) {
            const float o2 = __shfl(e2, l, 64);
            if (o2 >= 0.0f && q0 + l != j && (o2 < d2 || (o2 == d2 && q0 + l < j))) ++rank;
          }
        }
        ok = ok && rank < max_neigh;
      }
      const unsigned long long m = __ballot(ok);
      if (ok) store_edge(esrc, edst, evec, w + lanes_below(m, lane), (int)(base + j), (int)node, dx, dy, dz, d2);
      w += __popcll(m);
    });
  }
}

// ------------------------------------------------------------------------------------------------
// Pinned graphs (umx_pin_graph / umx_pin_graphs): the edge sets of R reference images, kept, and one of them replayed for every image
// of every evaluation while the pin holds.  Per directed edge of a reference the engine keeps the source and the target (atom indices
// within the image), and an index into the distinct lattice translations the reference edges took (one list for all references); per
// atom of every reference the integer wrap offset n of pin time (k_wrap_index).  The references' edges lie one behind the other.
//
// The replay: one thread per edge of the chunk, ONE launch per chunk.  img[k] says of image k of the chunk which reference it replays,
// where that reference's edges start (src0), how many they are (cnt), and where the image's edges start among those of the call (out0:
// the chunk's own offsets are out0 - img[0].out0).  Images differ in their edge counts, so a thread finds its image by a binary search
// for the last k with out0 - img[0].out0 <= its edge: an image without edges shares its offset with its successor and is never found,
// and a chunk without edges launches nothing.  A target-node partition (one image; sub_cnt >= 0) replays the contiguous rows of its
// reference that start sub0 edges into it instead.  Output edge out0 + (e - src0) gets source and target with the image's node offset,
// and the edge vector r_src + t - r_dst of the image's positions: open_delta, or pbc_delta on positions shifted by the stored wrap
// offsets in the image's cell (wrap_by), with the translation read from pshift -- [cells][nd] entries the host forms with the routine
// that fills the translation table, so at the pin-time cell they are the table's bits.  No cutoff test, no ranking: an edge that has
// grown beyond the cutoff stays, k_edge_geom gives it envelope 0.
// flag: bit 1 of the sticky status word for a non-finite coordinate, as k_graph_count sets it.
// ------------------------------------------------------------------------------------------------
struct PinImage {
  long long out0;         // edges of the call's images before this one
  long long src0;         // the first edge of the image's reference in psrc / pdst / ptix
  int cnt, ref;           // the reference's edges; the reference (its wrap offsets: pwrap + ref * natoms * 3)
};
template <typename P, typename B>
__global__ __launch_bounds__(256) void k_graph_replay(const P* __restrict__ pos, int natoms, const PinImage* __restrict__ img, int nimg, long sub0, long sub_cnt,
                                                      long total, const int* __restrict__ psrc, const int* __restrict__ pdst, const int* __restrict__ ptix,
                                                      const int* __restrict__ pwrap, const float4* __restrict__ pshift, int nd,
                                                      int* __restrict__ esrc, int* __restrict__ edst, float* __restrict__ evec, int* __restrict__ flag,
                                                      const B cells) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  int k = 0;
  long at = i;                                     // the edge within its image
  if (sub_cnt < 0) {
    const long long first = img[0].out0;
    int hi = nimg;                                 // the last k in [0, nimg) with img[k].out0 - first <= i
    while (hi - k > 1) {
      const int mid = (k + hi) >> 1;
      if (img[mid].out0 - first <= (long long)i) k = mid; else hi = mid;
    }
    at = i - (long)(img[k].out0 - first);
  }
  const PinImage im = img[k];
  const long e = (long)im.src0 + (sub_cnt < 0 ? 0 : sub0) + at;
  const int js = psrc[e], jd = pdst[e];
  const long base = (long)k * natoms;
  const P* ps = pos + (base + js) * 3;
  const P* pd = pos + (base + jd) * 3;
  P sx = ps[0], sy = ps[1], sz = ps[2], xi = pd[0], yi = pd[1], zi = pd[2];
  if (!(isfinite(sx) && isfinite(sy) && isfinite(sz) && isfinite(xi) && isfinite(yi) && isfinite(zi))) atomicOr(flag, 2);
  float dx, dy, dz;
  if constexpr (is_periodic<B>) {
    const int cell = cell_index(cells, k);
    const float4 sh = pshift[(long)cell * nd + ptix[e]];
    const auto& lat = lattice_of(cells, cell);
    const int* wrap = pwrap + (long)im.ref * natoms * 3;
    const P ws[3] = {(P)wrap[js * 3 + 0], (P)wrap[js * 3 + 1], (P)wrap[js * 3 + 2]};
    const P wd[3] = {(P)wrap[jd * 3 + 0], (P)wrap[jd * 3 + 1], (P)wrap[jd * 3 + 2]};
    wrap_by(lat, ws, sx, sy, sz);
    wrap_by(lat, wd, xi, yi, zi);
    const P pj[3] = {sx, sy, sz};
    pbc_delta(pj, xi, yi, zi, sh, lat, dx, dy, dz);
  } else {
    dx = open_delta(sx, xi); dy = open_delta(sy, yi); dz = open_delta(sz, zi);
  }
  store_edge(esrc, edst, evec, i, (int)(base + js), (int)(base + jd), dx, dy, dz, dist2_f(dx, dy, dz));
}
// the pinning call, several references: the fill wrote sources and targets as nodes of the batch -- back to atoms within their image
__global__ void k_pin_local(int* __restrict__ src, int* __restrict__ dst, long ne, int natoms) {
  const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= ne) return;
  const int base = (dst[e] / natoms) * natoms;
  src[e] -= base; dst[e] -= base;
}

// CSR by SOURCE (out-edges), valid for any graph (max_neigh truncation makes it asymmetric): count, scan (k_scan), fill
// through per-row cursors, then sort every row by edge id so the summation order is deterministic.
__global__ void k_out_count(const int* __restrict__ esrc, long ne, int* __restrict__ out_deg) {
  const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (e < ne) atomicAdd(out_deg + esrc[e], 1);
}
__global__ void k_out_fill(const int* __restrict__ esrc, long ne, const int* __restrict__ out_ptr, int* __restrict__ cursor,
                           int* __restrict__ out_edge) {
  const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= ne) return;
  const int n = esrc[e];
  out_edge[out_ptr[n] + atomicAdd(cursor + n, 1)] = (int)e;
}
// sort each node's out-edge list by edge id (deterministic summation order): one wave per node, rank sort -- every lane counts the
// entries smaller than its own (ids are unique), all reads finish before the first write because the wave runs in lockstep
__global__ __launch_bounds__(256) void k_out_sort(const int* __restrict__ out_ptr, long nt, int* __restrict__ out_edge) {
  UMX_WAVE_ITEM(n, nt)
  const int b = out_ptr[n], d = out_ptr[n + 1] - b;
  if (d <= 1) return;
  if (d <= 320) {
    int v[5], rk[5];
#pragma unroll
    for (int t = 0; t < 5; ++t) { const int i = lane + 64 * t; v[t] = i < d ? out_edge[b + i] : 0x7fffffff; rk[t] = 0; }
    for (int j = 0; j < d; ++j) {
      const int u = out_edge[b + j];
#pragma unroll
      for (int t = 0; t < 5; ++t) rk[t] += (u < v[t]) ? 1 : 0;
    }
#pragma unroll
    for (int t = 0; t < 5; ++t) if (lane + 64 * t < d) out_edge[b + rk[t]] = v[t];
  } else if (lane == 0) {          // very long lists (neighbour cap raised above 320): plain insertion sort
    for (int i = b + 1; i < b + d; ++i) {
      const int v = out_edge[i];
      int k = i - 1;
      while (k >= b && out_edge[k] > v) { out_edge[k + 1] = out_edge[k]; --k; }
      out_edge[k + 1] = v;
    }
  }
}

}  // namespace umx
