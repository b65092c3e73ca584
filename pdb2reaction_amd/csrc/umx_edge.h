// umx_edge.h -- the HBM-bound edge links between the large GEMMs, of every precision mode: gather + rotate (+ radial modulation), the
// SO(2) gate, and in the reverse pass rotate-back^T, gate^T and the modulation / rotation backward.  What a link writes is the A operand
// of the GEMM behind it, written ONCE in the layout that GEMM reads.  There are three operand layouts and nothing else:
//   float32 rows   `cols` floats per edge (fp32 mode; g_rad of the bf16x3 reverse pass, which the fc3^T GEMM splits in registers)
//   PL planes      P = 2 or 3 bf16 planes of x, interleaved per 32 columns (umx_gemm_pl.h):
//                    element (row, k, plane q) -> 16-bit index row * (cols*P) + (k / 32) * (32*P) + q * 32 + (k % 32)
//   quad-row       256-byte blocks of 4 rows x 16 columns, 4 bytes per element (umx_gemm_q.h):
//                    element (row, k) -> byte ((row/4) * (cols/16) + k/16) * 256 + (row%4) * 64 + the dword's own order (QFmt below)
//                  written directly (q_store2: the radial head, umx_radial.h) or through LDS in whole blocks (QuadStage).
// Every link's per-edge arithmetic is one __device__ function, shared by the kernels that differ in the layout they write and in their
// iteration shape: the staged kernels need whole workgroups at their barriers, the direct ones are grid-stride waves or threads.
// Kernel names: `_pl` writes PL planes, `_q3` quad-row blocks (the name is from the three-bf16-plane block format of round 4, which is
// gone: the blocks hold float32 or two fp16 halves), no suffix float32 rows (k_rotate_back_bwd: rows or PL planes, by its argument).
// Fusions relative to the fp32 mode's forward pass: the radial modulation is applied by the gather / rotate producer (the conv-1 GEMM no
// longer reads `rad`), and the reverse pass re-derives the rotated message inside k_modrot_bwd_pl instead of round-tripping a 9 KB/edge
// buffer through HBM.
#pragma once
#include "umx_common.h"

namespace umx {

// SIGN-ALTERNATING ROWS (round 4).  The adder of the 16-bit matrix cores aligns the products of one MFMA against the fp32 accumulator and
// drops the bits below ~2^-32 of the largest addend with a FLOOR (toward -infinity, whatever the signs: csrc/mfma_bias.hip) -- a one-sided
// error of a few 1e-9 of the accumulator per MFMA, i.e. -1e-8 ... -3e-8 relative on a GEMM output after 50-300 MFMAs, the SAME sign for
// every edge: a systematic energy error that grows like N.  floor(-S) = -ceil(S): with every operand row of ODD edge index stored negated
// (`odd_sign` = -1 in the producers below) and the sign restored in the GEMM epilogue (GemmPL::odd_sign), the error of odd rows has the
// opposite sign, and what was a bias is now noise that cancels between neighbouring edges.  Free: a sign flip before the split, a
// multiply by +-1 in the epilogue.  The kernels apply the sign; the writers below store what they are given.  (fp32 mode: odd_sign = +1.)
__device__ __forceinline__ float row_sign(long e, float odd_sign) { return (e & 1) ? odd_sign : 1.0f; }

// dev switch (-DUMX_NT=1): non-temporal stores for the write-once operand planes (A/B measurement in NOTES.md section 9)
#ifndef UMX_NT
#define UMX_NT 0
#endif
typedef unsigned int u32x2_t __attribute__((ext_vector_type(2)));
typedef unsigned int u32x4_t __attribute__((ext_vector_type(4)));
__device__ __forceinline__ void st_stream(unsigned int* p, unsigned int v) {
  if (UMX_NT) __builtin_nontemporal_store(v, p); else *p = v;
}
__device__ __forceinline__ void st_stream(uint2* p, uint2 v) {
  if (UMX_NT) __builtin_nontemporal_store(u32x2_t{v.x, v.y}, reinterpret_cast<u32x2_t*>(p)); else *p = v;
}
__device__ __forceinline__ void st_stream(uint4* p, uint4 v) {
  if (UMX_NT) __builtin_nontemporal_store(u32x4_t{v.x, v.y, v.z, v.w}, reinterpret_cast<u32x4_t*>(p)); else *p = v;
}

// ---- layout 2: PL planes ---------------------------------------------------------------------------------------------------------
template <int P> __device__ __forceinline__ long pl_index(int k) { return (long)(k >> 5) * (32 * P) + (k & 31); }
// split 2 adjacent values into P planes and store them (k even): 4-byte store per plane
template <int P> __device__ __forceinline__ void pl_store2(unsigned short* row, int k, float x0, float x1) {
  unsigned short* d = row + pl_index<P>(k);
#pragma unroll
  for (int q = 0; q < P; ++q) {
    const __bf16 h0 = (__bf16)x0, h1 = (__bf16)x1;
    const unsigned int pk = (unsigned int)__builtin_bit_cast(unsigned short, h0) | ((unsigned int)__builtin_bit_cast(unsigned short, h1) << 16);
    st_stream(reinterpret_cast<unsigned int*>(d + q * 32), pk);
    x0 -= (float)h0; x1 -= (float)h1;
  }
}
// split 4 adjacent values (k multiple of 4): 8-byte store per plane
template <int P> __device__ __forceinline__ void pl_store4(unsigned short* row, int k, float4 v) {
  unsigned short* d = row + pl_index<P>(k);
  float x[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
  for (int q = 0; q < P; ++q) {
    unsigned short hb[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) { const __bf16 h = (__bf16)x[c]; hb[c] = __builtin_bit_cast(unsigned short, h); x[c] -= (float)h; }
    st_stream(reinterpret_cast<uint2*>(d + q * 32), make_uint2((unsigned int)hb[0] | ((unsigned int)hb[1] << 16), (unsigned int)hb[2] | ((unsigned int)hb[3] << 16)));
  }
}

// The two row-wise layouts as writers: row(base, e, cols) = edge e's row of a `cols`-column operand, store2 / store4 = two / four adjacent
// values at column k of that row.  RowOut<0> = float32 rows, RowOut<2>, RowOut<3> = PL planes.
struct RowsF32 {
  typedef float T;
  static __device__ __forceinline__ T* row(T* base, long e, int cols) { return base + e * (long)cols; }
  static __device__ __forceinline__ void store2(T* row, int k, float x0, float x1) { *reinterpret_cast<float2*>(row + k) = make_float2(x0, x1); }
  static __device__ __forceinline__ void store4(T* row, int k, float4 v) { *reinterpret_cast<float4*>(row + k) = v; }
};
template <int P> struct Planes {
  typedef unsigned short T;
  static __device__ __forceinline__ T* row(T* base, long e, int cols) { return base + e * (long)(cols * P); }
  static __device__ __forceinline__ void store2(T* row, int k, float x0, float x1) { pl_store2<P>(row, k, x0, x1); }
  static __device__ __forceinline__ void store4(T* row, int k, float4 v) { pl_store4<P>(row, k, v); }
};
template <int P> struct RowOutOf { typedef Planes<P> W; };
template <> struct RowOutOf<0> { typedef RowsF32 W; };
template <int P> using RowOut = typename RowOutOf<P>::W;

// ---- layout 3: quad-row blocks ---------------------------------------------------------------------------------------------------
// Both formats are 4 bytes per element, so the block geometry is the same; QFmt says what one dword of a row's 64-byte piece holds:
//   FMT 3: a float32 -- dword k%16 is element k.  The A operand of the bf16x3 GEMMs (forward: bf16x3 and split-bf16; reverse: bf16x3):
//          umx_gemm_q.h (AF = 1) splits it into three bf16 planes in registers.
//   FMT 1 ("Q2H"): two IEEE halves of QF16_SCALE * x of two adjacent elements, in two 32-byte plane pieces -- dword (k%16)/2 holds the
//          high halves (RNE) of elements k, k+1, dword 8 + (k%16)/2 the low halves (RNE of the residual): 22 significant bits, and below
//          2^-14 / QF16_SCALE a fixed absolute resolution of 2^-25 / QF16_SCALE (half subnormals are kept by the conversion and by the
//          MFMA).  |x| >= 65520 / QF16_SCALE converts to inf, the low plane to -inf and the GEMM output to NaN: a range violation cannot
//          pass silently (the energy comes out non-finite).  The forward operands of split-f16.
constexpr float QF16_SCALE = 16.f;
constexpr int Q_BLK = 256, Q_ROWB = 64;             // bytes of a block, and of one row's piece of it
template <int FMT> struct QFmt { static_assert(FMT == 1 || FMT == 3, "quad-row formats: 1 (fp16 halves), 3 (float32)"); static constexpr bool F32 = (FMT == 3); };
// two adjacent values -> the dword of their high halves and the dword of their low halves (FMT 1)
__device__ __forceinline__ void q_split2(float x0, float x1, unsigned int (&out)[2]) {
  x0 *= QF16_SCALE; x1 *= QF16_SCALE;
  const _Float16 h0 = (_Float16)x0, h1 = (_Float16)x1;
  const _Float16 l0 = (_Float16)(x0 - (float)h0), l1 = (_Float16)(x1 - (float)h1);
  out[0] = (unsigned int)__builtin_bit_cast(unsigned short, h0) | ((unsigned int)__builtin_bit_cast(unsigned short, h1) << 16);
  out[1] = (unsigned int)__builtin_bit_cast(unsigned short, l0) | ((unsigned int)__builtin_bit_cast(unsigned short, l1) << 16);
}
// direct form: two adjacent values at (row, k), k even
template <int FMT> __device__ __forceinline__ unsigned short* q_ptr(unsigned short* base, long row, int cols, int k) {
  return reinterpret_cast<unsigned short*>(reinterpret_cast<unsigned char*>(base) + ((row >> 2) * (cols >> 4) + (k >> 4)) * Q_BLK +
                                           (row & 3) * Q_ROWB + (k & 15) * (QFmt<FMT>::F32 ? 4 : 2));
}
template <int FMT> __device__ __forceinline__ void q_store2(unsigned short* base, long row, int cols, int k, float x0, float x1) {
  unsigned short* d = q_ptr<FMT>(base, row, cols, k);
  if constexpr (QFmt<FMT>::F32) { st_stream(reinterpret_cast<uint2*>(d), make_uint2(__builtin_bit_cast(unsigned int, x0), __builtin_bit_cast(unsigned int, x1))); return; }
  unsigned int w[2];
  q_split2(x0, x1, w);
#pragma unroll
  for (int q = 0; q < 2; ++q) st_stream(reinterpret_cast<unsigned int*>(d + q * 16), w[q]);
}

// LDS-staged form.  Direct stores from the compute layout would be 8- or 16-byte pieces at a 64-byte (and, between the waves of a row
// group, 256-byte) stride (measured 60 ms instead of 42 ms per iteration for y1); instead a workgroup of 256 threads puts one ROW of its
// edges -- G row groups (4 edges each) x NB 16-column blocks -- into LDS in exactly the byte order of the G x NB consecutive blocks that
// hold it and writes them with coalesced 16-byte stores.  Two buffers: the values of row it + 1 are staged while row it is still being
// copied, and the barrier of flush(it + 1) is what frees the buffer of row it for row it + 2.  Per virtual block: begin(), then for
// it = 0, 1, ... in turn put2 / put4 by every thread and flush(it).
// The tail rules, for every staged kernel: the rows of a group's padding (edges >= ne of a group that holds an edge < ne) are computed
// from the group's first edge e0 (src_edge) -- the GEMM reads whole groups, the rows must be finite; a row group wholly beyond ne is not
// stored (the buffer ends with the last group that holds an edge); accumulators (dedd, tau) are written for valid edges only.
template <int G, int NB> struct QuadStage {
  static constexpr int CPG = NB * (Q_BLK / 16);         // 16-byte chunks of one row group's NB blocks
  static_assert(G * CPG <= 256, "one chunk per thread");
  typedef unsigned int Buf[2][G][NB][4][Q_ROWB / 4];    // [buffer][row group][16-column block][row in group][dword of the piece]
  Buf& lds;
  unsigned char* gbase;                                 // the first block of the virtual block's first row group
  long e0, ne, cols16;
  static __device__ __forceinline__ Buf& buffer() { __shared__ __attribute__((aligned(16))) Buf b; return b; }
  static __device__ __forceinline__ long src_edge(long e, long e0, long ne) { return e < ne ? e : e0; }
  __device__ __forceinline__ QuadStage() : lds(buffer()) {}
  // e0_: the first edge of the virtual block (a multiple of 4 G, < ne); cols: columns of the operand
  __device__ __forceinline__ void begin(unsigned short* out, long e0_, long ne_, int cols) {
    __syncthreads();                                    // the previous virtual block's last buffer is free
    e0 = e0_; ne = ne_; cols16 = cols / 16;
    gbase = reinterpret_cast<unsigned char*>(out) + (e0 >> 2) * cols16 * Q_BLK;
  }
  // le: the edge within the virtual block (0 .. 4 G - 1), col: the column within the staged row (0 .. 16 NB - 1; even / a multiple of 4)
  __device__ __forceinline__ unsigned int* piece(int it, int le, int col) { return &lds[it & 1][le >> 2][col >> 4][le & 3][0]; }
  template <int FMT> __device__ __forceinline__ void put2(int it, int le, int col, float x0, float x1) {
    unsigned int* p = piece(it, le, col);
    const int k15 = col & 15;
    if constexpr (QFmt<FMT>::F32) *reinterpret_cast<uint2*>(p + k15) = make_uint2(__builtin_bit_cast(unsigned int, x0), __builtin_bit_cast(unsigned int, x1));
    else {
      unsigned int w[2];
      q_split2(x0, x1, w);
#pragma unroll
      for (int q = 0; q < 2; ++q) p[(k15 >> 1) + q * 8] = w[q];
    }
  }
  template <int FMT> __device__ __forceinline__ void put4(int it, int le, int col, const float (&x)[4]) {
    unsigned int* p = piece(it, le, col);
    const int k15 = col & 15;
    if constexpr (QFmt<FMT>::F32)
      *reinterpret_cast<uint4*>(p + k15) = make_uint4(__builtin_bit_cast(unsigned int, x[0]), __builtin_bit_cast(unsigned int, x[1]), __builtin_bit_cast(unsigned int, x[2]), __builtin_bit_cast(unsigned int, x[3]));
    else {
      unsigned int wa[2], wb[2];
      q_split2(x[0], x[1], wa); q_split2(x[2], x[3], wb);
#pragma unroll
      for (int q = 0; q < 2; ++q) *reinterpret_cast<uint2*>(p + (k15 >> 1) + q * 8) = make_uint2(wa[q], wb[q]);
    }
  }
  // the staged row lies in the blocks blk0 .. blk0 + NB - 1 of every row group: thread t copies chunk t % CPG of group t / CPG
  __device__ __forceinline__ void flush(int it, int blk0) {
    __syncthreads();
    const int g = threadIdx.x / CPG, o = threadIdx.x % CPG;
    if ((G * CPG == 256 || threadIdx.x < G * CPG) && (G == 1 || e0 + 4 * g < ne)) {      // (G = 1: the virtual block's one group holds edge e0 < ne)
      const uint4 val = reinterpret_cast<const uint4*>(&lds[it & 1][g][0][0][0])[o];
      st_stream(reinterpret_cast<uint4*>(gbase + ((long)g * cols16 + blk0) * Q_BLK) + o, val);
    }
  }
};

// ---- iteration shapes ------------------------------------------------------------------------------------------------------------
// Grid-stride over the row groups (4 edges) of `count` edges, consecutive groups on the SAME XCD (blocks are dealt round-robin over the 8
// XCDs, each with its own L2): XCD x walks the contiguous range [x * per, (x+1) * per) -- rows gathered by neighbouring edges are then
// shared in one L2.  Virtual block v = blockIdx.x + k * gridDim.x has v & 7 == blockIdx.x & 7 when gridDim.x is a multiple of 8, so a
// physical workgroup only ever works for its own XCD's range; any grid size does the same work.  The groups are padded to a multiple of
// 8: the body runs for groups that hold an edge (block-uniform).  UMX_WAVE_LOOP_PL_XCD: the same with one wave per edge of the group.
#define UMX_GROUP_LOOP_XCD(grp, count)                                                \
  const long _nvb = ((((count) + 3) / 4 + 7) / 8) * 8;                                \
  const long _per = _nvb >> 3;                                                        \
  for (long _vb = blockIdx.x; _vb < _nvb; _vb += gridDim.x)                           \
    if (const long grp = (_vb & 7) * _per + (_vb >> 3); grp * 4 < (count))
#define UMX_WAVE_LOOP_PL_XCD(idx, count)                                              \
  const int lane = threadIdx.x & 63;                                                  \
  const long _nvb = ((((count) + 3) / 4 + 7) / 8) * 8;                                \
  const long _per = _nvb >> 3;                                                        \
  for (long _vb = blockIdx.x; _vb < _nvb; _vb += gridDim.x)                           \
    if (const long idx = __builtin_amdgcn_readfirstlane((int)(((_vb & 7) * _per + (_vb >> 3)) * 4 + (threadIdx.x >> 6))); idx < (count))

// ---- K7a gather + rotate: xrot[e] = W_e [xn[src] | xn[dst]]   (m-primary rows, 256 channels) ----------------------------------------
// a lane's two channels c0, c0 + 1 of the source half (ps, qs) and of the target half (pd, qd)
__device__ __forceinline__ void gather_rotate_edge(const float* xn, const int* esrc, const int* edst,
                                                   const float* frame, long e, int c0, float (&ps)[9], float (&qs)[9],
                                                   float (&pd)[9], float (&qd)[9]) {
  const float* f = frame + e * FRAME;
  const long js = esrc[e], jd = edst[e];
  float sx[9], sy[9], dx[9], dy[9];
#pragma unroll
  for (int r = 0; r < 9; ++r) {
    const float2 a = *reinterpret_cast<const float2*>(xn + js * ROW + r * C + c0);
    const float2 b = *reinterpret_cast<const float2*>(xn + jd * ROW + r * C + c0);
    sx[r] = a.x; sy[r] = a.y; dx[r] = b.x; dy[r] = b.y;
  }
  rot_fwd(f, sx, ps); rot_fwd(f, sy, qs); rot_fwd(f, dx, pd); rot_fwd(f, dy, qd);
}
// fp32 mode: the bare rotation as float32 rows (conv 1 applies the modulation); also what the unfused reverse pass reads
__global__ __launch_bounds__(256) void k_gather_rotate(const float* __restrict__ xn, const int* __restrict__ esrc,
                                                       const int* __restrict__ edst, const float* __restrict__ frame,
                                                       float* __restrict__ xrot, long ne) {
  UMX_WAVE_ITEM(e, ne)
  const int c0 = lane * 2;
  float ps[9], qs[9], pd[9], qd[9];
  gather_rotate_edge(xn, esrc, edst, frame, e, c0, ps, qs, pd, qd);
  float* out = RowsF32::row(xrot, e, XROT);
#pragma unroll
  for (int r = 0; r < 9; ++r) RowsF32::store2(out, r * 2 * C + c0, ps[r], qs[r]);
#pragma unroll
  for (int r = 0; r < 9; ++r) RowsF32::store2(out, r * 2 * C + C + c0, pd[r], qd[r]);
}
// split modes: + the radial modulation -> y1 in quad-row blocks.  A workgroup = the four edges of one row group, a wave each; per
// m-primary row r the four waves stage their 256 modulated columns (the 16 blocks of columns r*256 ... r*256+255).
template <int FMT>
__global__ __launch_bounds__(256) void k_gather_rotate_mod_q3(const float* __restrict__ xn, const int* __restrict__ esrc,
                                                              const int* __restrict__ edst, const float* __restrict__ frame,
                                                              const float* __restrict__ rad, unsigned short* __restrict__ y1, long ne, float odd_sign) {
  typedef QuadStage<1, 16> Stage;
  Stage st;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  UMX_GROUP_LOOP_XCD(grp, ne) {
  const long e0 = grp * 4;
  st.begin(y1, e0, ne, XROT);
  const long e = e0 + wave;
  const long ee = Stage::src_edge(e, e0, ne);
  const int c0 = lane * 2;
  const float sg = row_sign(e, odd_sign);
  float ps[9], qs[9], pd[9], qd[9];
  const float* rd = rad + ee * RAD;
  gather_rotate_edge(xn, esrc, edst, frame, ee, c0, ps, qs, pd, qd);
#pragma unroll
  for (int r = 0; r < 9; ++r) {
    const float2 ms = *reinterpret_cast<const float2*>(rd + RAD_ROW.of[r] * 2 * C + c0);
    const float2 md = *reinterpret_cast<const float2*>(rd + RAD_ROW.of[r] * 2 * C + C + c0);
    st.put2<FMT>(r, wave, c0, sg * (ps[r] * ms.x), sg * (qs[r] * ms.y));       // (the product rounded first, then the sign: the unsigned planes, negated)
    st.put2<FMT>(r, wave, C + c0, sg * (pd[r] * md.x), sg * (qd[r] * md.y));
    st.flush(r, r * 16);
  }
  }
}

// ---- the SO(2) gate on the edge hidden state hg = [gate l1 (128) | gate l2 (128) | hpre (9x128)] -> hid (9x128) ----------------------
// the two gates of a thread's four columns c .. c+3 of the edge row p
__device__ __forceinline__ void gate_sigmoids(const float* p, int c, float (&s1)[4], float (&s2)[4]) {
  const float4 g1 = *reinterpret_cast<const float4*>(p + c), g2 = *reinterpret_cast<const float4*>(p + H + c);
  s1[0] = sigmoid_f(g1.x); s1[1] = sigmoid_f(g1.y); s1[2] = sigmoid_f(g1.z); s1[3] = sigmoid_f(g1.w);
  s2[0] = sigmoid_f(g2.x); s2[1] = sigmoid_f(g2.y); s2[2] = sigmoid_f(g2.z); s2[3] = sigmoid_f(g2.w);
}
// row r of hid from row r of hpre: SiLU on the l = 0 row, the gate of the row's degree on the others
__device__ __forceinline__ void gate_fwd_row(int r, const float4 v, const float (&s1)[4], const float (&s2)[4], float (&x)[4]) {
  if (r == 0) { x[0] = silu_f(v.x); x[1] = silu_f(v.y); x[2] = silu_f(v.z); x[3] = silu_f(v.w); }
  else {
    const float (&s)[4] = row_is_l1(r) ? s1 : s2;
    x[0] = v.x * s[0]; x[1] = v.y * s[1]; x[2] = v.z * s[2]; x[3] = v.w * s[3];
  }
}
// fp32 mode: float32 rows, four columns per thread
__global__ void k_gate_edge_fwd(const float* __restrict__ hg, float* __restrict__ hid, long ne) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= ne * (H / 4)) return;
  const long e = i / (H / 4);
  const int c = (int)(i % (H / 4)) * 4;
  const float* p = hg + e * HG;
  float s1[4], s2[4];
  gate_sigmoids(p, c, s1, s2);
  float* o = RowsF32::row(hid, e, ROW);
#pragma unroll
  for (int r = 0; r < 9; ++r) {
    float x[4];
    gate_fwd_row(r, *reinterpret_cast<const float4*>(p + 2 * H + r * H + c), s1, s2, x);
    RowsF32::store4(o, r * H + c, make_float4(x[0], x[1], x[2], x[3]));
  }
}
// split modes: quad-row blocks.  A workgroup = 8 edges = two row groups, 32 threads per edge; per m-primary row the gated 128 columns
// (8 blocks) of the 8 edges are staged.
template <int FMT>
__global__ __launch_bounds__(256) void k_gate_edge_fwd_q3(const float* __restrict__ hg, unsigned short* __restrict__ hid, long ne, float odd_sign) {
  typedef QuadStage<2, 8> Stage;
  Stage st;
  const long nvb = (ne + 7) / 8;
  for (long vb = blockIdx.x; vb < nvb; vb += gridDim.x) {                        // grid-stride over groups of 8 edges: any grid size works
  const long e0 = vb * 8;
  st.begin(hid, e0, ne, ROW);
  const int le = threadIdx.x >> 5;                                               // edge within the workgroup
  const int c = (threadIdx.x & 31) * 4;
  const float* p = hg + Stage::src_edge(e0 + le, e0, ne) * HG;
  float s1[4], s2[4];
  gate_sigmoids(p, c, s1, s2);
  const float rs = row_sign(le, odd_sign);                                       // e0 is a multiple of 8: the edge's parity is le's
  float4 vr[9];                                                                  // all nine rows requested up front: the barriers in the loop
#pragma unroll                                                                   // below are memory fences the compiler will not move a load across
  for (int r = 0; r < 9; ++r) vr[r] = *reinterpret_cast<const float4*>(p + 2 * H + r * H + c);
#pragma unroll
  for (int r = 0; r < 9; ++r) {
    float x[4];
    gate_fwd_row(r, vr[r], s1, s2, x);
    x[0] *= rs; x[1] *= rs; x[2] *= rs; x[3] *= rs;
    st.put4<FMT>(r, le, c, x);
    st.flush(r, r * 8);
  }
  }
}

// ---- gate^T: ghid (9x128), hg (forward) -> g_hg = [ggate l1 | ggate l2 | ghpre 9x128] (1408 columns) -----------------------------------
// row r of ghpre (w) from row r of ghid (gv4) and of hpre (hv4); a1 / a2 collect <ghid, hpre> over the rows of degree 1 / 2
__device__ __forceinline__ void gate_bwd_row(int r, const float4 gv4, const float4 hv4, const float (&s1)[4], const float (&s2)[4],
                                             float (&a1)[4], float (&a2)[4], float (&w)[4]) {
  const float gv[4] = {gv4.x, gv4.y, gv4.z, gv4.w}, hv[4] = {hv4.x, hv4.y, hv4.z, hv4.w};
  const bool l1 = row_is_l1(r);
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    if (r == 0) w[k] = gv[k] * silu_grad_f(hv[k]);
    else {
      w[k] = gv[k] * (l1 ? s1[k] : s2[k]);
      if (l1) a1[k] += gv[k] * hv[k]; else a2[k] += gv[k] * hv[k];
    }
  }
}
// the gradient of a gate's pre-activation from its collected a and its sigmoid s
__device__ __forceinline__ void gate_bwd_gate(const float (&a)[4], const float (&s)[4], float (&q)[4]) {
#pragma unroll
  for (int k = 0; k < 4; ++k) q[k] = a[k] * s[k] * (1.0f - s[k]);
}
// float32 rows (k_gate_edge_bwd: fp32 mode) or PL planes (k_gate_edge_bwd_pl: the 16-bit reverse modes): grid-stride, four columns per thread
template <class W>
__device__ __forceinline__ void gate_edge_bwd_direct(const float* ghid, const float* hg, typename W::T* ghg,
                                                     long ne, float odd_sign) {
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < ne * (H / 4); i += (long)gridDim.x * blockDim.x) {
  const long e = i / (H / 4);
  const float sg = row_sign(e, odd_sign);
  const int c = (int)(i % (H / 4)) * 4;
  const float* p = hg + e * HG;
  float s1[4], s2[4];
  gate_sigmoids(p, c, s1, s2);
  typename W::T* o = W::row(ghg, e, HG);
  float a1[4] = {0.f, 0.f, 0.f, 0.f}, a2[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int r = 0; r < 9; ++r) {
    float w[4];
    gate_bwd_row(r, *reinterpret_cast<const float4*>(ghid + e * ROW + r * H + c), *reinterpret_cast<const float4*>(p + 2 * H + r * H + c), s1, s2, a1, a2, w);
    W::store4(o, 2 * H + r * H + c, make_float4(sg * w[0], sg * w[1], sg * w[2], sg * w[3]));
  }
  float q1[4], q2[4];
  gate_bwd_gate(a1, s1, q1); gate_bwd_gate(a2, s2, q2);
  W::store4(o, c, make_float4(sg * q1[0], sg * q1[1], sg * q1[2], sg * q1[3]));
  W::store4(o, H + c, make_float4(sg * q2[0], sg * q2[1], sg * q2[2], sg * q2[3]));
  }
}
__global__ void k_gate_edge_bwd(const float* __restrict__ ghid, const float* __restrict__ hg, float* __restrict__ ghg, long ne, float odd_sign) {
  gate_edge_bwd_direct<RowsF32>(ghid, hg, ghg, ne, odd_sign);
}
template <int P>
__global__ void k_gate_edge_bwd_pl(const float* __restrict__ ghid, const float* __restrict__ hg, unsigned short* __restrict__ ghg, long ne, float odd_sign) {
  gate_edge_bwd_direct<Planes<P>>(ghid, hg, ghg, ne, odd_sign);
}
// quad-row blocks (the bf16x3 reverse pass): a workgroup = 8 edges = two row groups; the staged rows are the nine m-primary rows of ghpre
// (blocks 16 + 8 r ...), then the two gate rows (blocks 0 and 8)
template <int FMT>
__global__ __launch_bounds__(256) void k_gate_edge_bwd_q3(const float* __restrict__ ghid, const float* __restrict__ hg, unsigned short* __restrict__ ghg,
                                                          long ne, float odd_sign) {
  typedef QuadStage<2, 8> Stage;
  Stage st;
  const long nvb = (ne + 7) / 8;
  for (long vb = blockIdx.x; vb < nvb; vb += gridDim.x) {
  const long e0 = vb * 8;
  st.begin(ghg, e0, ne, HG);
  const int le = threadIdx.x >> 5;
  const int c = (threadIdx.x & 31) * 4;
  const long e = Stage::src_edge(e0 + le, e0, ne);
  const float* p = hg + e * HG;
  float s1[4], s2[4];
  gate_sigmoids(p, c, s1, s2);
  const float rs = row_sign(le, odd_sign);                                       // e0 is a multiple of 8
  float4 gv4[9], hv4[9];                                                         // all loads up front (the barriers below fence loads)
#pragma unroll
  for (int r = 0; r < 9; ++r) {
    gv4[r] = *reinterpret_cast<const float4*>(ghid + e * ROW + r * H + c);
    hv4[r] = *reinterpret_cast<const float4*>(p + 2 * H + r * H + c);
  }
  float a1[4] = {0.f, 0.f, 0.f, 0.f}, a2[4] = {0.f, 0.f, 0.f, 0.f};
  auto emit = [&](int it, int blk0, const float (&x)[4]) {
    const float xs[4] = {rs * x[0], rs * x[1], rs * x[2], rs * x[3]};
    st.put4<FMT>(it, le, c, xs);
    st.flush(it, blk0);
  };
#pragma unroll
  for (int r = 0; r < 9; ++r) {
    float w[4];
    gate_bwd_row(r, gv4[r], hv4[r], s1, s2, a1, a2, w);
    emit(r, (2 * H + r * H) / 16, w);
  }
  float q1[4], q2[4];
  gate_bwd_gate(a1, s1, q1); gate_bwd_gate(a2, s2, q2);
  emit(9, 0, q1);
  emit(10, H / 16, q2);
  }
}

// ---- rotate-back^T: g_msg[e] = scale env_e (W_e g[dst e]); dedd[e] += denv_e scale <W g, msg>; tau[e] -= <g_msg, L msg> ----------------
// msg has NROWS rows (9: the SO(2) messages; 3: the edge-degree embedding, m = 0 rows only, scale = 1 / div; rows >= NROWS are zero).
// A lane's two channels c0, c0 + 1: lx / ly = g_msg (rows < NROWS are what is stored), s / tx / ty / tz = the lane's share of the sums.
template <int NROWS>
__device__ __forceinline__ void rotate_back_bwd_edge(const float* gnode, const float* msg, const float* frame,
                                                     const int* edst, long e, int c0, float div, float (&lx)[9], float (&ly)[9],
                                                     float& s, float& tx, float& ty, float& tz) {
  const float* f = frame + e * FRAME;
  const long jd = edst[e];
  float gx[9], gy[9], mx[9], my[9];
#pragma unroll
  for (int r = 0; r < 9; ++r) {
    const float2 t = *reinterpret_cast<const float2*>(gnode + jd * ROW + r * C + c0);
    gx[r] = t.x; gy[r] = t.y;
    if (r < NROWS) { const float2 m = *reinterpret_cast<const float2*>(msg + e * (NROWS * C) + r * C + c0); mx[r] = m.x; my[r] = m.y; }
    else { mx[r] = 0.f; my[r] = 0.f; }
  }
  rot_fwd(f, gx, lx); rot_fwd(f, gy, ly);
  const float sc = f[34] / div;
  s = 0.f; tx = 0.f; ty = 0.f; tz = 0.f;
#pragma unroll
  for (int r = 0; r < 9; ++r) {
    s += lx[r] * mx[r] + ly[r] * my[r];
    lx[r] *= sc; ly[r] *= sc;
  }
  torque_acc(lx, mx, -1.0f, tx, ty, tz);
  torque_acc(ly, my, -1.0f, tx, ty, tz);
}
// the wave's sums into the edge's accumulators (f: the edge's frame record).  The shared per-edge functions of this file take plain pointers:
// `__restrict__` on the parameters of an inlined function changes what the scheduler may reorder and cost k_rotate_back_bwd_pl<2> a register;
// the kernels keep theirs (profiles/edge_family_isa.txt).
__device__ __forceinline__ void rotate_back_bwd_sums(const float* f, float div, int lane, bool valid, long e, float s, float tx, float ty,
                                                     float tz, float* dedd, float* tau) {
  s = wave_sum(s); tx = wave_sum(tx); ty = wave_sum(ty); tz = wave_sum(tz);
  if (lane == 0 && valid) {
    dedd[e] += f[35] / div * s;
    tau[e * 4 + 0] += tx; tau[e * 4 + 1] += ty; tau[e * 4 + 2] += tz;
  }
}
// one wave per edge; P = 0: float32 rows (fp32 mode; the edge-degree link without planes), P = 2, 3: PL planes (the edge-degree link of
// the split modes: the A operand of the split fc3^T GEMM of the edge-degree MLP)
template <int NROWS, int P = 0>
__global__ __launch_bounds__(256) void k_rotate_back_bwd(const float* __restrict__ gnode, const float* __restrict__ msg,
                                                         const float* __restrict__ frame, const int* __restrict__ edst,
                                                         typename RowOut<P>::T* __restrict__ gmsg, float* __restrict__ dedd,
                                                         float* __restrict__ tau, long ne, float div, float odd_sign) {
  UMX_WAVE_ITEM(e, ne)
  const int c0 = lane * 2;
  float lx[9], ly[9], s, tx, ty, tz;
  rotate_back_bwd_edge<NROWS>(gnode, msg, frame, edst, e, c0, div, lx, ly, s, tx, ty, tz);
  typename RowOut<P>::T* o = RowOut<P>::row(gmsg, e, NROWS * C);
  const float sg = row_sign(e, odd_sign);
#pragma unroll
  for (int r = 0; r < NROWS; ++r) RowOut<P>::store2(o, r * C + c0, sg * lx[r], sg * ly[r]);
  rotate_back_bwd_sums(frame + e * FRAME, div, lane, true, e, s, tx, ty, tz, dedd, tau);
}
// the SO(2) messages as PL planes (the 16-bit reverse modes): grid-stride waves, XCD-contiguous
template <int P>
__global__ __launch_bounds__(256) void k_rotate_back_bwd_pl(const float* __restrict__ gnode, const float* __restrict__ msg,
                                                            const float* __restrict__ frame, const int* __restrict__ edst,
                                                            unsigned short* __restrict__ gmsg, float* __restrict__ dedd,
                                                            float* __restrict__ tau, long ne, float odd_sign) {
  UMX_WAVE_LOOP_PL_XCD(e, ne) {
  const int c0 = lane * 2;
  float lx[9], ly[9], s, tx, ty, tz;
  rotate_back_bwd_edge<9>(gnode, msg, frame, edst, e, c0, 1.0f, lx, ly, s, tx, ty, tz);
  unsigned short* o = Planes<P>::row(gmsg, e, ROW);
  const float sg = row_sign(e, odd_sign);
#pragma unroll
  for (int r = 0; r < 9; ++r) Planes<P>::store2(o, r * C + c0, sg * lx[r], sg * ly[r]);
  rotate_back_bwd_sums(frame + e * FRAME, 1.0f, lane, true, e, s, tx, ty, tz, dedd, tau);
  }
}
// ... as quad-row blocks (the bf16x3 reverse pass: the conv-2^T GEMMs then run on the 256 x 256-tile kernel like the forward ones).  A
// workgroup = the four edges of one row group, a wave each; per m-primary row the four waves stage their 128 columns (8 blocks).
template <int FMT>
__global__ __launch_bounds__(256) void k_rotate_back_bwd_q3(const float* __restrict__ gnode, const float* __restrict__ msg,
                                                            const float* __restrict__ frame, const int* __restrict__ edst,
                                                            unsigned short* __restrict__ gmsg, float* __restrict__ dedd,
                                                            float* __restrict__ tau, long ne, float odd_sign) {
  typedef QuadStage<1, 8> Stage;
  Stage st;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  UMX_GROUP_LOOP_XCD(grp, ne) {
  const long e0 = grp * 4;
  st.begin(gmsg, e0, ne, ROW);
  const long e = e0 + wave;
  const long ee = Stage::src_edge(e, e0, ne);
  const int c0 = lane * 2;
  float lx[9], ly[9], s, tx, ty, tz;
  rotate_back_bwd_edge<9>(gnode, msg, frame, edst, ee, c0, 1.0f, lx, ly, s, tx, ty, tz);
  rotate_back_bwd_sums(frame + ee * FRAME, 1.0f, lane, e < ne, e, s, tx, ty, tz, dedd, tau);
  const float sg = row_sign(ee, odd_sign);
#pragma unroll
  for (int r = 0; r < 9; ++r) {
    st.put2<FMT>(r, wave, c0, sg * lx[r], sg * ly[r]);
    st.flush(r, r * 8);
  }
  }
}

// ---- the unfused modulation / rotation backward (fp32 mode with captures on: it exposes xrot / g_xrot to the stage tests) ---------------
// backward of the radial modulation: gy1 (9x256, in/out -> gxrot), xrot, rad -> grad (1536); tau += <gxrot, L xrot>
__global__ __launch_bounds__(256) void k_modulate_bwd(float* __restrict__ gy1, const float* __restrict__ xrot,
                                                      const float* __restrict__ rad, float* __restrict__ grad,
                                                      float* __restrict__ tau, long ne) {
  UMX_WAVE_ITEM(e, ne)
  const int c0 = lane * 4;
  float* g = gy1 + e * XROT + c0;
  const float* x = xrot + e * XROT + c0;
  const float* rd = rad + e * RAD + c0;
  float* gr = grad + e * RAD + c0;
  float4 gv[9], xv[9];
#pragma unroll
  for (int r = 0; r < 9; ++r) {
    gv[r] = *reinterpret_cast<const float4*>(g + r * 2 * C);
    xv[r] = *reinterpret_cast<const float4*>(x + r * 2 * C);
  }
  float4 rv[6];
#pragma unroll
  for (int k = 0; k < 6; ++k) rv[k] = *reinterpret_cast<const float4*>(rd + k * 2 * C);
  float4 gacc[6];
#pragma unroll
  for (int k = 0; k < 6; ++k) gacc[k] = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
  for (int r = 0; r < 9; ++r) {
    const int k = RAD_ROW.of[r];
    gacc[k].x += gv[r].x * xv[r].x; gacc[k].y += gv[r].y * xv[r].y; gacc[k].z += gv[r].z * xv[r].z; gacc[k].w += gv[r].w * xv[r].w;
    gv[r].x *= rv[k].x; gv[r].y *= rv[k].y; gv[r].z *= rv[k].z; gv[r].w *= rv[k].w;
    *reinterpret_cast<float4*>(g + r * 2 * C) = gv[r];
  }
#pragma unroll
  for (int k = 0; k < 6; ++k) *reinterpret_cast<float4*>(gr + k * 2 * C) = gacc[k];
  float tx = 0.f, ty = 0.f, tz = 0.f;
  float ga[9], xa[9];
#pragma unroll
  for (int comp = 0; comp < 4; ++comp) {
#pragma unroll
    for (int r = 0; r < 9; ++r) {
      ga[r] = comp == 0 ? gv[r].x : comp == 1 ? gv[r].y : comp == 2 ? gv[r].z : gv[r].w;
      xa[r] = comp == 0 ? xv[r].x : comp == 1 ? xv[r].y : comp == 2 ? xv[r].z : xv[r].w;
    }
    torque_acc(ga, xa, 1.0f, tx, ty, tz);
  }
  tx = wave_sum(tx); ty = wave_sum(ty); tz = wave_sum(tz);
  if (lane == 0) { tau[e * 4 + 0] += tx; tau[e * 4 + 1] += ty; tau[e * 4 + 2] += tz; }
}

// backward of K7a (gather+rotate): g_xn[n] = sum_{e in in(n)} W_e^T gxrot[e][:, dst half] + sum_{e in out(n)} W_e^T gxrot[e][:, src half]
__global__ __launch_bounds__(256) void k_gather_rotate_bwd(const float* __restrict__ gxrot, const float* __restrict__ frame,
                                                           const int* __restrict__ row_ptr, const int* __restrict__ out_ptr,
                                                           const int* __restrict__ out_edge, float* __restrict__ gxn, long nt) {
  UMX_WAVE_ITEM(node, nt)
  const int c0 = lane * 2;
  float ax[9], ay[9];
#pragma unroll
  for (int r = 0; r < 9; ++r) { ax[r] = 0.f; ay[r] = 0.f; }
  float vx[9], vy[9];
  for (int e = row_ptr[node]; e < row_ptr[node + 1]; ++e) {
    const float* a = gxrot + (long)e * XROT + C + c0;
#pragma unroll
    for (int r = 0; r < 9; ++r) { const float2 t = *reinterpret_cast<const float2*>(a + r * 2 * C); vx[r] = t.x; vy[r] = t.y; }
    const float* f = frame + (long)e * FRAME;
    rot_bwd_acc(f, vx, 1.0f, ax); rot_bwd_acc(f, vy, 1.0f, ay);
  }
  for (int k = out_ptr[node]; k < out_ptr[node + 1]; ++k) {
    const long e = out_edge[k];
    const float* b = gxrot + e * XROT + c0;
#pragma unroll
    for (int r = 0; r < 9; ++r) { const float2 t = *reinterpret_cast<const float2*>(b + r * 2 * C); vx[r] = t.x; vy[r] = t.y; }
    const float* f = frame + e * FRAME;
    rot_bwd_acc(f, vx, 1.0f, ax); rot_bwd_acc(f, vy, 1.0f, ay);
  }
#pragma unroll
  for (int r = 0; r < 9; ++r) *reinterpret_cast<float2*>(gxn + node * ROW + r * C + c0) = make_float2(ax[r], ay[r]);
}

// ---- the fused modulation / rotation backward ------------------------------------------------------------------------------------------
// Reverse pass of K7a in ONE node-centric kernel (in place of an edge-wise modulation backward + k_gather_rotate_bwd): for every node n the wave
// walks its incoming edges (n is the target: columns C..2C of the 256-wide [src | dst] rows) and its outgoing edges (n is the
// source: columns 0..C).  In both walks the un-rotated feature is the node's OWN xn[n], so the rotated message is re-derived
// in registers, and
//   g_rad[e][k]  = sum_{rows r of block k} gy1[e][r] * xrot[r]        -> PL planes (A operand of the w3^T GEMM; P = 0: float32 rows, fp32 mode and bf16x3)
//   g_xrot[e][r] = gy1[e][r] * rad[e][k(r)]                            (never leaves the registers: -18 KB/edge of HBM traffic)
//   tau[e]      += <g_xrot, L xrot>                                    (target half -> tau, source half -> tau2: two writers)
//   g_xn[n]      = sum_e W_e^T g_xrot[e][half]                         (deterministic segmented sum, fixed edge order)
template <int P>
__global__ __launch_bounds__(256) void k_modrot_bwd_pl(const float* __restrict__ gy1, const float* __restrict__ xn,
                                                       const float* __restrict__ frame, const float* __restrict__ rad,
                                                       const int* __restrict__ row_ptr, const int* __restrict__ out_ptr,
                                                       const int* __restrict__ out_edge, unsigned short* __restrict__ grad,
                                                       float* __restrict__ tau, float* __restrict__ tau2, float* __restrict__ gxn, long nt, float odd_sign) {
  // one BLOCK per node: its four waves take every fourth edge of the two lists (4x shorter dependent loops, 4x more loads in
  // flight) and their partial g_xn rows are added through LDS in wave order -- still a fixed summation order
  __shared__ float part[3][9][C];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long node = blockIdx.x;
  if (node >= nt) return;
  const int c0 = lane * 2;
  float xx[9], xy[9], ax[9], ay[9];
#pragma unroll
  for (int r = 0; r < 9; ++r) {
    const float2 t = *reinterpret_cast<const float2*>(xn + node * ROW + r * C + c0);
    xx[r] = t.x; xy[r] = t.y; ax[r] = 0.f; ay[r] = 0.f;
  }
  // (This kernel's body and its g_rad store are kept as they were written, on purpose: with both walks inlined, which product of
  //  a sum the compiler rounds and which it fuses follows the order its passes meet the code in.  Reading RAD_ROW in place instead of this
  //  local copy, for one, swaps the rounded product in rot_bwd_acc's sums: other bits in g_xn.)
  const RadRow ridx = RAD_ROW;
  auto one_edge = [&](long e, int half, float* __restrict__ tdst) {
    const float* f = frame + e * FRAME;
    const float* g = gy1 + e * XROT + half + c0;
    const float* rd = rad + e * RAD + half + c0;
    float2 gv[9], rv[6];
#pragma unroll
    for (int r = 0; r < 9; ++r) gv[r] = *reinterpret_cast<const float2*>(g + r * 2 * C);
#pragma unroll
    for (int k = 0; k < 6; ++k) rv[k] = *reinterpret_cast<const float2*>(rd + k * 2 * C);
    float px[9], py[9];
    rot_fwd(f, xx, px); rot_fwd(f, xy, py);
    float gax[6], gay[6];
#pragma unroll
    for (int k = 0; k < 6; ++k) { gax[k] = 0.f; gay[k] = 0.f; }
    float hx[9], hy[9];
#pragma unroll
    for (int r = 0; r < 9; ++r) {
      const int k = ridx.of[r];
      gax[k] += gv[r].x * px[r]; gay[k] += gv[r].y * py[r];
      hx[r] = gv[r].x * rv[k].x; hy[r] = gv[r].y * rv[k].y;
    }
    if constexpr (P == 0) {      // g_rad as plain float32 rows: the A operand of the fp32-MFMA fc3^T GEMM (fp32 mode, odd_sign = +1) or of
      float* gr = reinterpret_cast<float*>(grad) + e * (long)RAD;      // umx_gemm_pl_kernel<16, .., AF = 1> (bf16x3, sign-alternating rows)
      const float sg = row_sign(e, odd_sign);
#pragma unroll
      for (int k = 0; k < 6; ++k) *reinterpret_cast<float2*>(gr + k * 2 * C + half + c0) = make_float2(sg * gax[k], sg * gay[k]);
    } else {
      unsigned short* gr = grad + e * (long)(RAD * P);
      const float sg = row_sign(e, odd_sign);
#pragma unroll
      for (int k = 0; k < 6; ++k) pl_store2<(P ? P : 2)>(gr, k * 2 * C + half + c0, sg * gax[k], sg * gay[k]);
    }
    float tx = 0.f, ty = 0.f, tz = 0.f;
    torque_acc(hx, px, 1.0f, tx, ty, tz); torque_acc(hy, py, 1.0f, tx, ty, tz);
    tx = wave_sum(tx); ty = wave_sum(ty); tz = wave_sum(tz);
    if (lane == 0) { tdst[e * 4 + 0] += tx; tdst[e * 4 + 1] += ty; tdst[e * 4 + 2] += tz; }
    rot_bwd_acc(f, hx, 1.0f, ax); rot_bwd_acc(f, hy, 1.0f, ay);
  };
  for (int e = row_ptr[node] + wave; e < row_ptr[node + 1]; e += 4) one_edge((long)e, C, tau);
  for (int k = out_ptr[node] + wave; k < out_ptr[node + 1]; k += 4) one_edge((long)out_edge[k], 0, tau2);
  if (wave > 0) {
#pragma unroll
    for (int r = 0; r < 9; ++r) *reinterpret_cast<float2*>(&part[wave - 1][r][c0]) = make_float2(ax[r], ay[r]);
  }
  __syncthreads();
  if (wave == 0) {
#pragma unroll
    for (int r = 0; r < 9; ++r) {
      float sx = ax[r], sy = ay[r];
#pragma unroll
      for (int w = 0; w < 3; ++w) { const float2 t = *reinterpret_cast<const float2*>(&part[w][r][c0]); sx += t.x; sy += t.y; }
      *reinterpret_cast<float2*>(gxn + node * ROW + r * C + c0) = make_float2(sx, sy);
    }
  }
}

// tau += tau2 (the two halves of k_modrot_bwd_pl's torque are written by different waves)
__global__ void k_add4(float* __restrict__ a, const float* __restrict__ b, long n4) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n4) return;
  float4 x = *reinterpret_cast<float4*>(a + i * 4);
  const float4 y = *reinterpret_cast<const float4*>(b + i * 4);
  x.x += y.x; x.y += y.y; x.z += y.z; x.w += y.w;
  *reinterpret_cast<float4*>(a + i * 4) = x;
}

}  // namespace umx
