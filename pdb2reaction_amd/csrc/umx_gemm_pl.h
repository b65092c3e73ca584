// umx_gemm_pl.h -- multi-plane bf16 MFMA GEMM with an asynchronous LDS-DMA ring (gfx950).
//
//   C[M x N] (fp32) = sum_{i+j<P} A_i[M x K] . B_j[N x K]^T ,   A_i, B_j bf16 planes in HBM
//
// Both operands arrive already split into P bf16 planes (x = x0 + x1 (+ x2), exact): weights once at
// load time, activations by the HBM-bound producer kernel that writes them (one conversion per element
// instead of one per N tile).  P = 3 -> 6 MFMAs per product (fp32-equivalent, forward pass),
// P = 2 -> 3 MFMAs (reverse pass).
//
// PLANE-INTERLEAVED ROW LAYOUT ("PL" layout).  A matrix X[rows][K] is stored as rows of K*P bf16:
//   element (r, k, plane q)  ->  r * (K*P) + (k / 32) * (32*P) + q * 32 + (k % 32)
// so the P planes of one 32-column block of a row are contiguous (128 B for P=2, 192 B for P=3): one
// global_load_lds wave-instruction then fetches whole 128-B lines.  (With separate planes and a 16-wide
// k-step every line was requested four separate times and the fill, not the MFMA, set the pace.)
//
// Structure (cdna_hip_programming.md section 5; measured steps in NOTES.md section 5):
//  * 256 x (64*WNT) block tile, BK = 32, 4 waves (2x2), ONE block per CU, each wave owns a
//    128 x (32*WNT) C tile = 4 x WNT v_mfma_f32_32x32x16_bf16 tiles (up to 256 accumulator registers;
//    the wave has the whole 512-entry register file).
//  * Operand tiles go global -> LDS with global_load_lds_dwordx4 (no VGPR staging, no VALU): a ring of S
//    stages, tile kt+S-1 is requested while tile kt is consumed; the only waits are a counted
//    s_waitcnt vmcnt((S-2)*G) and ONE raw s_barrier per k-step (never __syncthreads(), which would drain
//    the DMA queue).  All LDS lives in one __shared__ array.
//  * LDS image = the DMA's flat chunk order (row-major, 4P 16-B slots per row, no padding possible);
//    bank conflicts are removed by permuting the SOURCE chunk with a per-row XOR and applying the same
//    involution to fragment reads (conflict-free ds_read_b128).
//  * Rows past M / N are clamped on the source side (their results are masked in the epilogue).
//  * CPLX: rows are (re/im, edge), weight rows (A/B half, channel); every wave holds both re/im row
//    groups and both A/B column groups of its edges x channels and combines them in the accumulators.
#pragma once
#include "umx_gemm.h"

namespace umx {

typedef float f32x4 __attribute__((ext_vector_type(4)));

struct GemmPL {
  const unsigned short* Apl; long lda; int offA0, offA1;   // PL layout: lda = row pitch in bf16 (= K_total*P); offsets in COLUMNS (multiples of 32)
  const unsigned short* Bpl; long ldb; int bHalf;          // weights, PL layout (ldb = K*P)
  float* Cp; long ldc; int offC, offCi;
  const float* bias;
  float conj;
  int M, N, K;       // CPLX: M = edges, N = channels per half
  float cscale;      // fp16-plane kernels only (umx_gemm_q.h, F16 = 1): C = cscale * (A' . B'^T) undoes the power-of-two operand scales
  float odd_sign;    // +1, or -1 when the producer stored the A rows of ODD index negated (sign-alternating rows, umx_edge.h): the
                     // epilogue multiplies the accumulators of odd rows by it, so C is what it would be -- with the matrix core's one-sided
                     // rounding error reversed on every second row.  0 is read as +1 (dev programs that memset the struct).
  // the gate-reverse epilogue of the conv-2^T products (umx_gemm_q.h, EP = 1; unused elsewhere): hg = the forward [gate | hpre] rows,
  // ghg = g_hg as float32 quad-row blocks, gate_acc = the per-edge gate sums (2 x 128 floats), ep_mode = which product of the convolution
  // (0: m = 0 starts the sums, 1: m = 1 completes degree 1, 2: m = 2 completes degree 2)
  const float* hg; float* ghg; float* gate_acc; int ep_mode;
};

template <int N> __device__ __forceinline__ void wait_vmcnt() {
  asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}

// per-row slot permutation (an involution): LDS slot s of row r holds source chunk pl_perm(s, r)
template <int P> __device__ __forceinline__ int pl_perm(int s, int r) {
  return P == 2 ? (s ^ ((r >> 1) & 7)) : ((s & ~3) | ((s & 3) ^ ((r >> 2) & 3)));
}

// request one k-tile (32 columns, all planes) of A and B into the ring stage at `sbase`; kofs_a / kofs = the k-tile's offset in the
// rows of A / B (float32 A rows advance by 64 shorts per k-tile, the planes of B by 32 P).
// (A plain __device__ function: a lambda calling the LDS-DMA builtin silently drops the host-side kernel stub, and
//  hipcc 7.2 rejects a second kernel re-using one specialization of such a function -- hence TAG = kernel_tag of the caller.)
template <int JA, int JB, int TA_B, int WSTR, long TAG>
__device__ __forceinline__ void pl_issue(const GemmPL& p, unsigned char* sbase, const long (&a_off)[JA], const long (&b_off)[JB], long kofs_a, long kofs, int piece) {
#pragma unroll
  for (int j = 0; j < JA; ++j)
    __builtin_amdgcn_global_load_lds(p.Apl + a_off[j] + kofs_a, (__attribute__((address_space(3))) void*)(sbase + piece + j * WSTR), 16, 0, 0);
#pragma unroll
  for (int j = 0; j < JB; ++j)
    __builtin_amdgcn_global_load_lds(p.Bpl + b_off[j] + kofs, (__attribute__((address_space(3))) void*)(sbase + TA_B + piece + j * WSTR), 16, 0, 0);
}

// The two MFMA shapes of the PL kernel.  E = tile edge, NR = accumulator registers per tile, KSTEPS = MFMA k-steps per 32-wide k-tile;
// a lane supplies row `row(lane)` and the 16-B k-chunk `kc(lane)` of a k-step (8 bf16), and owns the C/D rows cd_row<NR>(reg) + 4 kc.
template <int E> struct PlMfma;
template <> struct PlMfma<32> {      // v_mfma_f32_32x32x16_bf16: two k-steps per k-tile
  static constexpr int NR = 16, KSTEPS = 2;
  typedef f32x16 Acc;
  static __device__ __forceinline__ int row(int lane) { return lane & 31; }
  static __device__ __forceinline__ int kc(int lane) { return lane >> 5; }
  static __device__ __forceinline__ Acc mfma(const bf16x8_t& a, const bf16x8_t& b, const Acc& c) { return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0); }
};
template <> struct PlMfma<16> {      // v_mfma_f32_16x16x32_bf16: one k-step covers the k-tile (the chip may hold a different clock on this shape)
  static constexpr int NR = 4, KSTEPS = 1;
  typedef f32x4 Acc;
  static __device__ __forceinline__ int row(int lane) { return lane & 15; }
  static __device__ __forceinline__ int kc(int lane) { return lane >> 4; }
  static __device__ __forceinline__ Acc mfma(const bf16x8_t& a, const bf16x8_t& b, const Acc& c) { return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0); }
};

// Geometry: WVM x WVN waves, each owning a (32*WMT) x (32*WNT) C tile: block tile = (32*WVM*WMT) x (32*WVN*WNT).
//   <.., WVM=2, WVN=2, WMT=4, WNT=2>  256x128, 4 waves (one per SIMD, 128 accumulator registers)
//   <.., WVM=4, WVN=2, WMT=2, WNT=2>  256x128, 8 waves (two per SIMD: one wave's LDS-read latency hides under the other's MFMAs)
//   <.., WVM=2, WVN=4, WMT=4, WNT=2>  256x256, 8 waves (half the fill bytes per FLOP; P=2 only, LDS)
// E = MFMA tile edge (PlMfma above).
// AF = 1 (round 4): the A operand as plain float32 ROWS (row pitch lda shorts = 2 x columns; what the node-centric k_modrot_bwd_pl<0>
// writes edge by edge), split into the three bf16 planes in registers as in umx_gemm_q.h.  A row of a k-tile is 32 floats = 128 B = the
// geometry of the two-plane rows: the LDS slot of the lane's piece i (k = 8 h + 4 i ...) is the two-plane image's slot of (plane i,
// k-chunk h), so the proven conflict-free pl_perm<2> serves; source chunk = 2 h + i.
template <int E, int CPLX, int P, int S, int WVM, int WVN, int WMT, int WNT, int AF = 0>
__global__ __launch_bounds__(64 * WVM * WVN, 1) void umx_gemm_pl_kernel(const GemmPL p) {
  typedef PlMfma<E> MF;
  static_assert(!AF || (E == 16 && P == 3), "AF: the six-product form on the 16x16x32 shape (a lane's two float pieces are one k-step)");
  constexpr int NT = 64 * WVM * WVN;           // threads
  constexpr int BM = 32 * WVM * WMT;           // block tile rows (A rows)
  constexpr int BN = 32 * WVN * WNT;           // block tile columns (B rows)
  static_assert(!CPLX || (WMT % 2 == 0 && WNT % 2 == 0), "complex tiles need re/im and A/B halves in every wave");
  constexpr int SEG = 4 * P;                   // 16-B chunks per row per k-tile
  constexpr int ROWB = SEG * 16;               // bytes per row per k-tile (128 or 192)
  constexpr int SEGA = AF ? 8 : SEG, ROWA = SEGA * 16;
  constexpr int TA_B = BM * ROWA;
  constexpr int TB_B = BN * ROWB;
  constexpr int STAGE_B = TA_B + TB_B;
  static_assert(S * STAGE_B <= 160 * 1024, "ring does not fit the 160 KiB LDS");
  __shared__ __attribute__((aligned(1024))) unsigned char ring[S * STAGE_B];
  constexpr int BMR = CPLX ? BM / 2 : BM;      // logical rows (edges) per block
  constexpr int BNC = CPLX ? BN / 2 : BN;      // logical cols (channels) per block
  constexpr int JA = BM * SEGA / NT;           // A chunks per lane per k-tile
  constexpr int JB = BN * SEG / NT;
  static_assert(BM * SEGA % NT == 0 && BN * SEG % NT == 0, "tile does not divide over the threads");
  constexpr int G = JA + JB;                   // global_load_lds instructions per wave per k-tile
  constexpr int WSTR = NT * 16;                // LDS bytes covered by one DMA round of the whole block
  constexpr int TM = WMT * 32 / E, TN = WNT * 32 / E;   // MFMA tiles per wave
  constexpr int KA = AF ? 64 : 32 * P;         // shorts per k-tile in a row of A
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave / WVN, wn = wave % WVN;
  const int lr = MF::row(lane), h = MF::kc(lane);

  int mt, nt;
  if (!xcd_tile<BMR, BNC>(p.M, p.N, mt, nt)) return;

  // ---- per-lane source offsets (bf16 elements): flat chunk id c = tid + 256 j -> row = c / SEG, LDS slot = c % SEG
  long a_off[JA], b_off[JB];
#pragma unroll
  for (int j = 0; j < JA; ++j) {
    const int c = tid + NT * j, trow = c / SEGA, s = c % SEGA;
    long grow; int offA;
    if (CPLX) { grow = (long)mt * BMR + cplx_idx<BMR>(trow); offA = cplx_half<BMR>(trow) ? p.offA1 : p.offA0; }
    else      { grow = (long)mt * BM + trow;                 offA = p.offA0; }
    if (grow >= p.M) grow = p.M - 1;
    if (AF) { const int u = pl_perm<2>(s, trow); a_off[j] = grow * p.lda + (long)offA * 2 + (2 * (u & 3) + (u >> 2)) * 8; }
    else a_off[j] = grow * p.lda + (long)offA * P + pl_perm<P>(s, trow) * 8;
  }
#pragma unroll
  for (int j = 0; j < JB; ++j) {
    const int c = tid + NT * j, trow = c / SEG, s = c % SEG;
    int brow;
    if (CPLX) { int cc = nt * BNC + cplx_idx<BNC>(trow); if (cc >= p.N) cc = p.N - 1; brow = cplx_half<BNC>(trow) * p.bHalf + cc; }
    else      { brow = nt * BN + trow; if (brow >= p.N) brow = p.N - 1; }
    b_off[j] = (long)brow * p.ldb + pl_perm<P>(s, trow) * 8;
  }
  const int piece = __builtin_amdgcn_readfirstlane(wave * 1024);   // this wave's 1-KiB piece inside one DMA round

  typename MF::Acc acc[TM][TN];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
      for (int r = 0; r < MF::NR; ++r) acc[i][j][r] = 0.f;

  // fragment rows inside the tile
  int a_row[TM], b_row[TN];
#pragma unroll
  for (int t = 0; t < TM; ++t) a_row[t] = frag_row0<CPLX, TM, E, BMR>(wm, t) + lr;
#pragma unroll
  for (int t = 0; t < TN; ++t) b_row[t] = frag_row0<CPLX, TN, E, BNC>(wn, t) + lr;

  const int nk = p.K / 32;
  constexpr long TAG = kernel_tag<E / 16, CPLX, P, S, WVM, WVN, WMT, WNT, AF>();
#pragma unroll
  for (int s = 0; s < S - 1; ++s)
    if (s < nk) pl_issue<JA, JB, TA_B, WSTR, TAG>(p, ring + s * STAGE_B, a_off, b_off, (long)s * KA, (long)s * 32 * P, piece);

  for (int kt = 0; kt < nk; ++kt) {
    if (kt + S - 2 < nk) wait_vmcnt<(S - 2) * G>(); else wait_vmcnt<0>();
    __builtin_amdgcn_s_barrier();   // everyone's tile kt landed; everyone finished reading tile kt-1
    if (kt + S - 1 < nk)
      pl_issue<JA, JB, TA_B, WSTR, TAG>(p, ring + ((kt + S - 1) % S) * STAGE_B, a_off, b_off, (long)(kt + S - 1) * KA, (long)(kt + S - 1) * 32 * P, piece);
    const unsigned char* sbase = ring + (kt % S) * STAGE_B;
#pragma unroll
    for (int ks = 0; ks < MF::KSTEPS; ++ks) {
      bf16x8_t a[TM][P], b[TN][P];
      if constexpr (AF) {
#pragma unroll
        for (int t = 0; t < TM; ++t)
          qf_split<0>(*reinterpret_cast<const f32x4q_t*>(sbase + a_row[t] * ROWA + pl_perm<2>(h, a_row[t]) * 16),
                      *reinterpret_cast<const f32x4q_t*>(sbase + a_row[t] * ROWA + pl_perm<2>(4 + h, a_row[t]) * 16), a[t]);
      }
#pragma unroll
      for (int q = 0; q < P; ++q) {
        const int u = q * 4 + ks * (4 / MF::KSTEPS) + h;      // source chunk wanted: plane q, k-chunk of this k-step and lane
        if constexpr (!AF) {
#pragma unroll
          for (int t = 0; t < TM; ++t) a[t][q] = *reinterpret_cast<const bf16x8_t*>(sbase + a_row[t] * ROWB + pl_perm<P>(u, a_row[t]) * 16);
        }
#pragma unroll
        for (int t = 0; t < TN; ++t) b[t][q] = *reinterpret_cast<const bf16x8_t*>(sbase + TA_B + b_row[t] * ROWB + pl_perm<P>(u, b_row[t]) * 16);
      }
#pragma unroll
      for (int ord = P - 1; ord >= 0; --ord)     // smallest terms first
#pragma unroll
        for (int qa = 0; qa <= ord; ++qa) {
          const int qb = ord - qa;
#pragma unroll
          for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int j = 0; j < TN; ++j) acc[i][j] = MF::mfma(a[i][qa], b[j][qb], acc[i][j]);
        }
    }
  }

  // ---- epilogue: the sign of the odd rows (row parity = r & 1), the bias added to the finished sum.  The two store forms: cd_row in
  //      umx_gemm.h
  constexpr int NR = MF::NR;
  const bool full = ((long)mt * BMR + BMR <= p.M) && (nt * BNC + BNC <= p.N);
  const float osg = p.odd_sign < 0.f ? -1.0f : 1.0f;
  if (CPLX) {
#pragma unroll
    for (int eg = 0; eg < TM / 2; ++eg)
#pragma unroll
      for (int cg = 0; cg < TN / 2; ++cg) {
        const int chan = nt * BNC + wn * (16 * WNT) + cg * E + lr;
        const long e0 = (long)mt * BMR + wm * (16 * WMT) + eg * E + 4 * h;
        float* c = p.Cp + e0 * p.ldc + chan;
        if (full) {
#pragma unroll
          for (int r = 0; r < NR; ++r) {
            float* cr = c + (long)cd_row<NR>(r) * p.ldc;
            const float sg = (r & 1) ? osg : 1.0f;
            cr[p.offC] = sg * (acc[eg][cg][r] - p.conj * acc[TM / 2 + eg][TN / 2 + cg][r]);
            cr[p.offCi] = sg * (acc[TM / 2 + eg][cg][r] + p.conj * acc[eg][TN / 2 + cg][r]);
          }
        } else if (chan < p.N) {
#pragma unroll
          for (int r = 0; r < NR; ++r) {
            const int dr = cd_row<NR>(r);
            if (e0 + dr < p.M) {
              float* cr = c + (long)dr * p.ldc;
              const float sg = (r & 1) ? osg : 1.0f;
              cr[p.offC] = sg * (acc[eg][cg][r] - p.conj * acc[TM / 2 + eg][TN / 2 + cg][r]);
              cr[p.offCi] = sg * (acc[TM / 2 + eg][cg][r] + p.conj * acc[eg][TN / 2 + cg][r]);
            }
          }
        }
      }
  } else {
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
      for (int j = 0; j < TN; ++j) {
        const int col = nt * BN + wn * (32 * WNT) + j * E + lr;
        const float bv = (p.bias && col < p.N) ? p.bias[col] : 0.f;
        const long row0 = (long)mt * BM + wm * (32 * WMT) + i * E + 4 * h;
        float* c = p.Cp + row0 * p.ldc + p.offC + col;
        if (full) {
#pragma unroll
          for (int r = 0; r < NR; ++r) c[(long)cd_row<NR>(r) * p.ldc] = ((r & 1) ? osg : 1.0f) * acc[i][j][r] + bv;
        } else if (col < p.N) {
#pragma unroll
          for (int r = 0; r < NR; ++r) {
            const int dr = cd_row<NR>(r);
            if (row0 + dr < p.M) c[(long)dr * p.ldc] = ((r & 1) ? osg : 1.0f) * acc[i][j][r] + bv;
          }
        }
      }
  }
}

}  // namespace umx
