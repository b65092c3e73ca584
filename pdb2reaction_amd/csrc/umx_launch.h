// umx_launch.h -- host side, part 2 of 5: the profiling bracket and the GEMM launchers (fp32 MFMA / float64-accumulating node kernel:
// launch_gemm; split-precision plane GEMMs: gemm_pl = choose_pl + the table of instantiations + one launch site), and the SO(2)
// convolutions: their column layouts stated once (So2Layout) and the one function that issues a convolution's three products (so2_conv).
#pragma once

namespace {

// HIP-event bracket around one launch for umx_profile_read (prec: > 0 split-precision GEMM family, 0 fp32 GEMM, < 0 fused radial kernels).
// *out stays null while profiling is off.
int prof_open(umx_engine* eng, ProfRec** out, double flops, int prec, long M, int N, int K, int amode = 0, int cplx = 0, int gz = 1) {
  *out = nullptr;
  if (!eng->prof_on) return UMX_OK;
  if (eng->prof_used == eng->prof.size()) {
    ProfRec r; HIPCHK(eng, hipEventCreate(&r.a)); HIPCHK(eng, hipEventCreate(&r.b)); r.flops = 0; eng->prof.push_back(r);
  }
  ProfRec* pr = &eng->prof[eng->prof_used++];
  pr->flops = flops; pr->M = (int)M; pr->N = N; pr->K = K; pr->amode = amode; pr->cplx = cplx; pr->gz = gz; pr->prec = prec;
  HIPCHK(eng, hipEventRecord(pr->a, eng->stream));
  *out = pr;
  return UMX_OK;
}
int prof_close(umx_engine* eng, ProfRec* pr) {
  if (pr) HIPCHK(eng, hipEventRecord(pr->b, eng->stream));
  return UMX_OK;
}
// grid of a grid-stride ("virtual block") kernel: all blocks normally, capped in throttled two-lane mode
inline unsigned vgrid(const umx_engine* eng, unsigned blocks) {
  return (eng->throttle && eng->stream_cap > 0 && blocks > (unsigned)eng->stream_cap) ? (unsigned)eng->stream_cap : blocks;
}

// k_scan is a single block of 1024 threads (umx_graph.h)
inline void launch_scan(hipStream_t s, const int* deg, long n, int* row_ptr, int* stats) {
  hipLaunchKernelGGL(k_scan, dim3(1), dim3(1024), 0, s, deg, n, row_ptr, stats);
}

// ---- fp32 GEMM launcher ------------------------------------------------------------------------
GemmP gp_zero() { GemmP p; std::memset(&p, 0, sizeof(p)); p.conj = 1.0f; return p; }

int launch_gemm(umx_engine* eng, const GemmP& p, int amode, int cplx, int gz = 1) {
  if (p.M <= 0) return UMX_OK;
  if (p.K % G_BK != 0) return fail(eng, UMX_ERR_ARG, "gemm: K not a multiple of 32");
  const int bmr = cplx ? 64 : 128, bnc = cplx ? 64 : 128;
  const long nM = (p.M + bmr - 1) / bmr, nN = (p.N + bnc - 1) / bnc;
  const long blocks = ((nM + 7) / 8) * 8 * nN;
  dim3 grid((unsigned)blocks, 1, (unsigned)gz), block(256);
  ProfRec* pr;
  CHK(prof_open(eng, &pr, cplx ? 8.0 * p.M * (double)p.N * p.K : 2.0 * p.M * (double)p.N * p.K * gz, 0, p.M, p.N, p.K, amode, cplx, gz));
  if (eng->node_f64_on && eng->node_ctx && !cplx && (amode == A_PLAIN || amode == A_SILU)) {
    const dim3 g64((unsigned)(((p.M + 63) / 64) * ((p.N + 63) / 64)), 1, (unsigned)gz);
    if (amode == A_SILU) hipLaunchKernelGGL(k_gemm_f64acc<A_SILU>, g64, block, 0, eng->stream, p);
    else hipLaunchKernelGGL(k_gemm_f64acc<A_PLAIN>, g64, block, 0, eng->stream, p);
    HIPCHK(eng, hipGetLastError());
    return prof_close(eng, pr);
  }
  switch (amode * 10 + cplx) {
    case A_PLAIN * 10 + 0: hipLaunchKernelGGL((umx_gemm_kernel<A_PLAIN, 0>), grid, block, 0, eng->stream, p); break;
    case A_PLAIN * 10 + 1: hipLaunchKernelGGL((umx_gemm_kernel<A_PLAIN, 1>), grid, block, 0, eng->stream, p); break;
    case A_MODUL * 10 + 0: hipLaunchKernelGGL((umx_gemm_kernel<A_MODUL, 0>), grid, block, 0, eng->stream, p); break;
    case A_MODUL * 10 + 1: hipLaunchKernelGGL((umx_gemm_kernel<A_MODUL, 1>), grid, block, 0, eng->stream, p); break;
    case A_SILU * 10 + 0: hipLaunchKernelGGL((umx_gemm_kernel<A_SILU, 0>), grid, block, 0, eng->stream, p); break;
    default: return fail(eng, UMX_ERR_ARG, "gemm: variant not instantiated");
  }
  HIPCHK(eng, hipGetLastError());
  return prof_close(eng, pr);
}

struct NodeCtx { umx_engine* e; explicit NodeCtx(umx_engine* eng) : e(eng) { e->node_ctx = true; } ~NodeCtx() { e->node_ctx = false; } };

// plain C = A . B^T (+bias, +resid)
int gemm_plain(umx_engine* eng, const float* A, long lda, int offA, const float* B, long ldb, const float* bias, float* Cp,
               long ldc, int offC, long M, int N, int K, int amode = A_PLAIN, int gz = 1, long zA = 0, long zC = 0,
               const float* resid = nullptr, long ldres = 0, int offRes = 0, long zRes = 0) {
  GemmP p = gp_zero();
  p.A = A; p.lda = lda; p.offA0 = offA; p.B = B; p.ldb = ldb; p.bias = bias; p.Cp = Cp; p.ldc = ldc; p.offC = offC;
  p.M = (int)M; p.N = N; p.K = K; p.zA = zA; p.zC = zC; p.resid = resid; p.ldres = ldres; p.offRes = offRes; p.zRes = zRes;
  return launch_gemm(eng, p, amode, 0, gz);
}

// the same for a NODE-level linear (rows = atoms): float64 accumulation when the engine asks for it (umx_engine::node_f64_on)
template <class... Args> int gemm_node(umx_engine* eng, Args... args) {
  NodeCtx node(eng);
  return gemm_plain(eng, args...);
}

// ... and for the (node x grid point) rows of the grid feed-forward: float64-accumulated like the other node-level linears unless
// UMX_GRID_F64=0 (fp32 MFMA)
template <class... Args> int gemm_grid(umx_engine* eng, Args... args) {
  if (!eng->grid_f64) return gemm_plain(eng, args...);
  NodeCtx node(eng);
  return gemm_plain(eng, args...);
}

// SO(2) complex linear on (edge, re/im) rows
int gemm_cplx(umx_engine* eng, const float* A, long lda, int offRe, int offIm, const float* R, long ldr, int offR, const float* B,
              long ldb, int bHalf, float* Cp, long ldc, int offCre, int offCim, long M, int N, int K, float conj) {
  GemmP p = gp_zero();
  p.A = A; p.lda = lda; p.offA0 = offRe; p.offA1 = offIm; p.R = R; p.ldr = ldr; p.offR = offR; p.B = B; p.ldb = ldb; p.bHalf = bHalf;
  p.Cp = Cp; p.ldc = ldc; p.offC = offCre; p.offCi = offCim; p.M = (int)M; p.N = N; p.K = K; p.conj = conj;
  return launch_gemm(eng, p, R ? A_MODUL : A_PLAIN, 1);
}

// SO(3) linear on l-primary node rows: ONE launch, gridDim.z = 9 coefficients, the weights of degree l(z) picked per z (zBl);
// the bias acts on the l = 0 row only
int so3_linear(umx_engine* eng, const float* A, const float* Wl, const float* bias, float* Cp, long nn, const float* resid) {
  GemmP p = gp_zero();
  p.A = A; p.lda = ROW; p.offA0 = 0; p.B = Wl; p.ldb = C; p.bias = bias; p.Cp = Cp; p.ldc = ROW; p.offC = 0;
  p.M = (int)nn; p.N = C; p.K = C; p.zA = C; p.zC = C; p.resid = resid; p.ldres = ROW; p.offRes = 0; p.zRes = C; p.zBl = (long)C * C;
  NodeCtx node(eng);
  return launch_gemm(eng, p, A_PLAIN, 0, S);
}

// ---- split-precision GEMM of the large SO(2) / radial linears ----------------------------------
// Operand formats and plane counts follow the pass and the engine's precision mode:
//   forward, bf16x3 / split-bf16 : A = float32 quad-row blocks split into three bf16 planes by the GEMM in registers, B = three bf16 planes (6 products)
//   forward, split-f16           : A = two fp16 planes of 16 x activation, B = three exact fp16 planes (4 products)
//   reverse, bf16x3              : conv^T: A = float32 quad-row blocks (g_msg / g_hg), B = three bf16 planes, 6 products (umx_gemm_q.h);
//                                  fc3^T: A = float32 ROWS (g_rad, a_f32rows) split by umx_gemm_pl_kernel<16, .., AF = 1>
//   reverse, split-* modes       : A, B = two PL bf16 planes, 3 products (umx_gemm_pl.h)
// Kernel families: Q_F16 quad-row, two fp16 planes x three fp16 weight planes; Q_BF16 quad-row, float32 A blocks x three bf16 weight
// planes; PL3_ROWS three PL planes, A = float32 rows (bf16x3 layer fc3^T); PL3 three PL planes (bf16x3 edge-degree fc3^T); PL2_* two PL
// planes: 256-wide tiles / narrow tiles on the 16x16x32 MFMA / narrow tiles on the 32x32x16 MFMA
enum PlFamily { Q_F16, Q_BF16, PL3_ROWS, PL3, PL2_WIDE, PL2_M16, PL2_M32 };

// What selects an instantiation: the family, complex or plain, and for Q_BF16 -- ls = the low-order plane products accumulate apart, in
// the form that goes with the tile width (template LS = 1: 256 x 256 tiles, one spare accumulator folded in every k-step; LS = 2:
// 256 x 128 tiles, a second accumulator set for the whole k loop); al = aligned leading plane of A; half = the half-height form (template
// MW = 2: 128-row tiles, 256 threads, two workgroups per CU), bit for bit its full-height form.
struct PlKey {
  PlFamily fam = Q_F16; bool cplx = false, wide = false, ls = false, al = false, half = false;
  bool operator==(const PlKey& o) const { return fam == o.fam && cplx == o.cplx && wide == o.wide && ls == o.ls && al == o.al && half == o.half; }
};
struct PlKernel { PlKey key; void (*fn)(const GemmPL); };

// Every instantiated plane GEMM, exactly once: the 39 keys choose_pl can return over the precision modes, both passes, the engine's product
// shapes (N x K of the radial fc3 / fc3^T and of the SO(2) blocks, So2Layout below), every documented value of UMX_LOW_SEP,
// UMX_ALIGN_PLANES and UMX_GEMM_HALF and both sides of `fills` (enumerated with choose_pl itself on the host):
//   Q_F16     plain and complex, narrow and wide                                  4
//   Q_BF16    plain: every (wide, ls, al, half); complex: the same without the     28
//             narrow LS forms -- a complex product has N in {128, 256, 512}, a
//             multiple of 128, so a complex LS product is always wide
//   PL3_ROWS, PL3  plain, narrow                                                   2
//   PL2_WIDE  plain and complex; PL2_M16 plain (K >= 512) and complex;             5
//             PL2_M32 plain only (a complex narrow product takes PL2_M16)
#define UMX_Q(cplx, wide, ls, al, half) \
  {{Q_BF16, cplx != 0, wide != 0, ls != 0, al != 0, half != 0}, umx_gemm_q_kernel<cplx, wide, 3, 2, 0, 6, 3, 1, (ls ? (wide ? 1 : 2) : 0), al, (half ? 2 : 4)>}
#define UMX_Q4(cplx, wide, ls) UMX_Q(cplx, wide, ls, 0, 0), UMX_Q(cplx, wide, ls, 1, 0), UMX_Q(cplx, wide, ls, 0, 1), UMX_Q(cplx, wide, ls, 1, 1)
const PlKernel pl_kernels[] = {
    {{Q_F16, false, false}, umx_gemm_q_kernel<0, 0, 2, 2, 1, 4, 3>}, {{Q_F16, true, false}, umx_gemm_q_kernel<1, 0, 2, 2, 1, 4, 3>},
    {{Q_F16, false, true}, umx_gemm_q_kernel<0, 1, 2, 2, 1, 4, 3>},  {{Q_F16, true, true}, umx_gemm_q_kernel<1, 1, 2, 2, 1, 4, 3>},
    UMX_Q4(0, 0, 0), UMX_Q4(0, 0, 1), UMX_Q4(0, 1, 0), UMX_Q4(0, 1, 1),
    UMX_Q4(1, 0, 0), UMX_Q4(1, 1, 0), UMX_Q4(1, 1, 1),
    {{PL3_ROWS}, umx_gemm_pl_kernel<16, 0, 3, 2, 4, 2, 2, 2, 1>},     // (an 8 x 1 wave layout measured the same)
    {{PL3}, umx_gemm_pl_kernel<32, 0, 3, 2, 4, 2, 2, 2>},
    {{PL2_WIDE, false, true}, umx_gemm_pl_kernel<16, 0, 2, 2, 4, 2, 2, 4>}, {{PL2_WIDE, true, true}, umx_gemm_pl_kernel<16, 1, 2, 2, 4, 2, 2, 4>},
    {{PL2_M16, false}, umx_gemm_pl_kernel<16, 0, 2, 3, 4, 2, 2, 2>},        {{PL2_M16, true}, umx_gemm_pl_kernel<16, 1, 2, 3, 4, 2, 2, 2>},
    {{PL2_M32, false}, umx_gemm_pl_kernel<32, 0, 2, 3, 4, 2, 2, 2>},
};
// The conv-2^T products of the bf16x3 reverse pass with the gate-reverse epilogue (umx_gemm_q.h EP = 1): a table of their own, the forms
// choose_pl can pick for a reverse Q_BF16 product of those shapes (plain: N = 384, narrow; complex: N = 256 / 128, narrow or wide; either
// height).  Logged as family "Q_BF16_GATE" (umx_debug_fetch "gemm:table_gate", "gemm:launches").
struct GateEpi { const float* hg; float* ghg; float* acc; int mode; };     // GemmPL::hg, ghg, gate_acc, ep_mode
#define UMX_QG(cplx, wide, half) {{Q_BF16, cplx != 0, wide != 0, false, false, half != 0}, umx_gemm_q_kernel<cplx, wide, 3, 2, 0, 6, 3, 1, 0, 0, (half ? 2 : 4), 1>}
const PlKernel pl_gate_kernels[] = {UMX_QG(0, 0, 0), UMX_QG(0, 0, 1), UMX_QG(1, 0, 0), UMX_QG(1, 0, 1), UMX_QG(1, 1, 0), UMX_QG(1, 1, 1)};
#undef UMX_QG
#undef UMX_Q
#undef UMX_Q4
// a key as text, "fam cplx wide ls al half" (umx_debug_fetch "gemm:table", "gemm:launches")
std::string pl_key_text(const PlKey& k, bool gate = false) {
  static const char* const fam[] = {"Q_F16", "Q_BF16", "PL3_ROWS", "PL3", "PL2_WIDE", "PL2_M16", "PL2_M32"};
  return std::string(fam[k.fam]) + (gate ? "_GATE " : " ") + std::to_string(k.cplx) + " " + std::to_string(k.wide) + " " + std::to_string(k.ls) + " " + std::to_string(k.al) + " " +
         std::to_string(k.half);
}
std::string pl_table_text() {
  std::string t;
  for (const PlKernel& e : pl_kernels) t += pl_key_text(e.key) + "\n";
  return t;
}
std::string pl_gate_table_text() {
  std::string t;
  for (const PlKernel& e : pl_gate_kernels) t += pl_key_text(e.key, true) + "\n";
  return t;
}

// which instantiation runs one product, with which grid and which leading dimensions (in 2-byte units)
// (prec: ProfRec::prec -- 24: two fp16 planes, 4 products; 3 / 2: bf16 planes, 6 / 3 products; err: the product has no instantiation)
struct PlChoice { PlKey key; unsigned blocks = 0; long lda = 0, ldb = 0; int prec = 0; const char* err = nullptr; };
PlChoice choose_pl(const Precision& pm, Pass pass, bool w_quad, int cplx, long M, int N, int K, int a_cols, bool a_f32rows, int low_sep, int align, int half) {
  PlChoice c;
  c.key.cplx = cplx != 0;
  const bool fwd = pass == FWD;
  const int P = fwd ? 3 : pm.rev_planes;
  c.prec = (fwd && pm.fwd_fmt == 1) ? 24 : P;
  c.lda = (long)a_cols * P; c.ldb = (long)K * P;
  // 256 x 256 tiles (two ring stages fit the LDS) wherever N fills whole tiles: a third less L2->LDS fill per FLOP, 9-11 % faster.
  // Small systems (c1: 50 atoms x 8 images = 13 k edges = 51 row tiles): a launch whose wide grid does not even put one workgroup on
  // every CU is bound by ONE tile's k-loop, so the narrow tiles (twice the workgroups, half the work each) finish sooner.
  const int bmr = cplx ? 128 : 256;
  const long nM = (M + bmr - 1) / bmr;
  const bool fills = nM * (N / (cplx ? 128 : 256)) >= 256;          // wide grid >= one workgroup per CU
  // LS: the three plane products of order 2^-16 of a forward bf16x3 GEMM accumulate apart from the large ones (umx_gemm_q.h) -- on every
  // PLAIN product (radial fc3, conv-1 / conv-2 m = 0: operands with one-signed columns -- SiLU outputs, gated scalars, element embeddings);
  // the complex m > 0 products take rotated l >= 1 components whose signs follow the edge direction, and measured no different with it
  // (c5 energy error, three fixtures: none +1.0e-3 eV, fc3 only +5.9e-4, plain -7e-6, all -3e-5; c3 step 497 / 500 / 511 / 522 ms).
  // UMX_LOW_SEP (dev A/B): 0 none, 1 fc3 only, 2 every forward product, 3 the plain ones (default).
  c.key.ls = fwd && pm.fwd_fmt == 3 && (low_sep == 2 || (low_sep == 3 && !cplx) || (low_sep == 1 && !cplx && K == RH));
  // (an LS product picks its tile from N alone: the two LS forms fold the small products in at different points, and an image must get the
  //  same bits whether it is evaluated alone or in a batch -- tests/test_gpu_graph_parallel.py, test_gpu_parity.py batch independence)
  c.key.wide = N % (cplx ? 128 : 256) == 0 && (fills || c.key.ls);
  int bnc = c.key.wide ? (cplx ? 128 : 256) : (cplx ? 64 : 128);
  if (fwd && pm.fwd_fmt == 1) {
    // two fp16 planes of 16 x (activations), three exact planes of s_w x (weights): C = (A' . B'^T) / (16 s_w)
    c.key.fam = Q_F16; c.lda = (long)a_cols * 2; c.ldb = (long)K * 3;
  } else if (fwd || (P == 3 && w_quad)) {
    // A = float32 quad-row blocks, split into the three bf16 planes in registers; weights as three bf16 planes.  The 256 x 128 LS form
    // keeps a second accumulator set for the whole k loop (190 VGPRs: one 8-wave workgroup per CU instead of two -- +10 ms at c3 for conv-1 /
    // conv-2 m = 0 when it went in; deeper rings do not buy it back: S = 3 / 4 measured +5 / +6 ms, and neither do two 4-wave workgroups
    // of half the height, which fit the same registers: -0.1 ms, see UMX_GEMM_HALF below -- the 10 ms are not tile turnover.  Round 6 measured the per-k-step fold of the wide
    // tiles there too: 167-172 VGPRs as compiled (one workgroup per CU all the same); forced into the 128 VGPRs a second workgroup needs
    // it spills 19 registers: +40 ms, and 48 float32 folds per output instead of one move the 20 000-atom energies to -9e-5 eV on two of
    // four cases -- profiles/r06_ls_ab.txt; removed)
    c.key.fam = Q_BF16; c.lda = (long)a_cols * 3; c.ldb = (long)K * 3;
    c.key.al = fwd && (align == 1 || (align == 2 && !cplx));      // aligned planes: forward products only (the weights' planes were built to match, umx_load_weights)
  } else if (P == 3) {
    // three-plane PL products of the bf16x3 reverse pass: the radial fc3^T of the layers (A = float32 rows, split in registers) and of the
    // edge-degree embedding (A = three PL planes written by k_rotate_back_bwd<3, 3>); both plain, N = 128, 256 x 128 tiles
    if (cplx || N > 128) { c.err = "gemm_pl: three-plane PL products are instantiated for the plain N <= 128 (radial fc3^T) products only"; return c; }
    c.key.fam = a_f32rows ? PL3_ROWS : PL3;                       // (wide is false here: N is no multiple of 256)
    if (a_f32rows) c.lda = (long)a_cols * 2;                  // row pitch in 2-byte units
  } else if (c.key.wide) {
    c.key.fam = PL2_WIDE;
  } else {
    // MFMA shape per GEMM (measured in the c3 pipeline): 16x16x32 wins 1-7 % on the complex SO(2) GEMMs and on K >= 512,
    // 32x32x16 wins 5-10 % on the short-K plain ones (radial fc3^T, conv-2^T m = 0)
    c.key.fam = (cplx || K >= 512) ? PL2_M16 : PL2_M32;
  }
  // Half-height tiles (umx_gemm_q.h MW = 2; Q_BF16 only): two 4-wave workgroups per CU, each running while the other waits for its
  // prologue or drains its stores, at the price of fetching the B tile twice as often.  The bits are the same in either form, so this
  // choice MAY depend on M (unlike the LS tile width above) -- and half tiles would also suit the small-M rule (`fills`), which is left as
  // measured.  UMX_GEMM_HALF (dev A/B): 0 none, 1 the forward LS products on narrow tiles (conv-1 / conv-2 m = 0, edge-degree fc3), 2 + the
  // forward LS products on wide tiles (fc3), 3 every Q_BF16 product, 4 the complex (m > 0) products only, 5 (default) the products that
  // measured a gain: those WITHOUT LS and with K >= 256 -- the complex m > 0 products of both passes (c3, per launch: N 256 K 512 -4.2 %,
  // 256 x 256 -2.5 %, 512 x 256 -1.5 ... -3.3 %, 128 x 256 -1 %) and the plain conv^T m = 0 products of the bf16x3 reverse pass (768 x 640
  // -3.9 %); the short-K complex products lose (128 x 128 +4 %, 256 x 128 +-0).  The forward LS products, for which the second workgroup
  // was expected to pay (their 190 / 239 VGPRs cost them their co-resident partner in round 5), measured NO gain: c3 step -0.1 ms
  // (narrow) / -0.4 ms (+ fc3) against an A/A spread of 0.8 ms; every Q_BF16 product -6.4 ms, complex only -5.1 ms
  // (profiles/half_tile_ab.txt; NOTES.md section 13).
  // The conv-2^T products with the gate-reverse epilogue (pl_gate_kernels) INHERIT this rule through the same key: under the default 5 the
  // plain 384 x 384 and the complex 256 x 256 product run on half-height tiles, the complex 128 x 128 product (K < 256) at full height.  The
  // rule is not re-fitted to the fused forms: tests/test_gpu_gate_epilogue.py requires a fused launch to have the tile form of the unfused
  // product.  The per-launch times of the three fused shapes at full against half height (UMX_GEMM_HALF 0 / 3), as far as they were
  // measured, are in profiles/gate_epilogue_ab.txt section 3.
  c.key.half = c.key.fam == Q_BF16 && (half == 3 || (half == 4 && cplx) || (half == 5 && !c.key.ls && K >= 256) ||
                               (fwd && c.key.ls && (half == 2 || (half == 1 && !c.key.wide))));
  const long nMf = c.key.half ? (M + bmr / 2 - 1) / (bmr / 2) : nM;     // row tiles of the form that runs
  c.blocks = (unsigned)(((nMf + 7) / 8) * 8 * ((N + bnc - 1) / bnc));
  return c;
}

// Wkey = fp32 device pointer of the weight (its plane copy is looked up); a_cols = total columns of the A matrix; offsets in columns.
int gemm_pl(umx_engine* eng, int cplx, Pass pass, const unsigned short* Apl, int a_cols, int offA0, int offA1, const float* Wkey, int bHalf,
            const float* bias, float* Cp, long ldc, int offC, int offCi, long M, int N, int K, float conj, bool a_f32rows = false,
            const GateEpi* gate = nullptr) {
  if (M <= 0) return UMX_OK;
  auto it = eng->planes.find(Wkey);
  if (it == eng->planes.end()) return fail(eng, UMX_ERR_ARG, "gemm_pl: weight has no PL copy");
  if (K % 32 != 0) return fail(eng, UMX_ERR_ARG, "gemm_pl: K not a multiple of 32");
  const PlaneCopy& w = it->second;
  const PlChoice c = choose_pl(eng->prec, pass, w.quad, cplx, M, N, K, a_cols, a_f32rows, eng->low_sep, eng->align, eng->gemm_half);
  if (c.err) return fail(eng, UMX_ERR_ARG, c.err);
  const PlKernel* k = nullptr;
  // gate: the product's elements go through gate^T into g_hg (so2_conv, conv 2^T of the bf16x3 reverse pass) -- the same key, and so the
  // same tile form, looked up in the table of the kernels with that epilogue
  if (gate && (c.key.fam != Q_BF16 || pass != REV || N % 128 != 0)) return fail(eng, UMX_ERR_ARG, "gemm_pl: the gate-reverse epilogue goes with the reverse Q_BF16 products");
  if (gate) { for (const PlKernel& e : pl_gate_kernels) if (e.key == c.key) { k = &e; break; } }
  else for (const PlKernel& e : pl_kernels)
    if (e.key == c.key) { k = &e; break; }
  if (!k) return fail(eng, UMX_ERR_ARG, "gemm_pl: variant not instantiated");
  GemmPL q;
  std::memset(&q, 0, sizeof(q));
  q.Apl = Apl; q.lda = c.lda; q.offA0 = offA0; q.offA1 = offA1; q.Bpl = w.ptr; q.ldb = c.ldb; q.bHalf = bHalf;
  q.Cp = Cp; q.ldc = ldc; q.offC = offC; q.offCi = offCi; q.bias = bias; q.conj = conj; q.M = (int)M; q.N = N; q.K = K;
  q.odd_sign = eng->odd_sign;
  if (gate) { q.hg = gate->hg; q.ghg = gate->ghg; q.gate_acc = gate->acc; q.ep_mode = gate->mode; }
  if (c.key.fam == Q_F16) q.cscale = 1.0f / (QF16_SCALE * w.scale);
  ProfRec* pr;
  CHK(prof_open(eng, &pr, cplx ? 8.0 * M * (double)N * K : 2.0 * M * (double)N * K, c.prec, M, N, K, 9, cplx));
  hipLaunchKernelGGL(k->fn, dim3(c.blocks), dim3(c.key.half ? 256 : 512), 0, eng->stream, q);
  HIPCHK(eng, hipGetLastError());
  if (eng->dbg_on)
    eng->gemm_log += std::string(pass == FWD ? "fwd " : "rev ") + pl_key_text(c.key, gate != nullptr) + " " + std::to_string(M) + " " + std::to_string(N) + " " + std::to_string(K) + " " +
                     std::to_string(c.blocks) + "\n";
  return prof_close(eng, pr);
}

// ---- the SO(2) convolutions ----------------------------------------------------------------------
// The m-primary column layout of an edge row that an SO(2) convolution reads or writes: the m = 0 block first, then re | im of m = 1 and
// of m = 2.  ld = the row's columns, m0 = the width of the m = 0 block, re / im / w = the column offsets and the width of one half.
struct So2Layout { int ld, m0, m1re, m1im, m1w, m2re, m2im, m2w; };
constexpr So2Layout SO2_Y1 = {XROT, 768, 768, 1280, 512, 1792, 2048, 256};    // y1 / g_y1 (and xrot): the rotated [src | dst] message
constexpr So2Layout SO2_HG = {HG, 640, 640, 896, 256, 1152, 1280, 128};       // hg / g_hg: [gate scalars | hidden m = 0], hidden m = 1, m = 2
constexpr So2Layout SO2_MSG = {ROW, 384, 384, 640, 256, 896, 1024, 128};      // hid / msg / g_msg
// the radial weights (RAD columns) that modulate the three blocks of an fp32 conv-1's A operand: one column per (re, im) pair
constexpr int SO2_RAD_M1 = 768, SO2_RAD_M2 = 1280;

// One SO(2) convolution C = conv(A): the plain m = 0 product and the complex m = 1 and m = 2 products, in this order.  N and K of every
// product are the block widths of C's and A's layout; every weight is (N x K) row-major per half, so ldb == K and bHalf == N.  A
// transposed convolution is the same call with the layouts of A and C swapped, the transposed weights, pass REV and conj = -1.
// Split-precision modes: A = the pre-split operand planes (gemm_pl).  fp32 mode: A = float32 rows; R != nullptr (conv 1 forward): the
// A operand is modulated by the radial rows R while it is staged.
int so2_conv(umx_engine* eng, Pass pass, const void* A, const So2Layout& la, float* Cp, const So2Layout& lc, const float* Wm0, const float* Wm1,
             const float* Wm2, const float* bias, long ne, float conj, const float* R = nullptr, const GateEpi* gate = nullptr) {
  if (eng->prec.planes) {
    const unsigned short* Apl = static_cast<const unsigned short*>(A);
    // gate (conv 2^T, bf16x3 reverse): C = g_hid is not written; the three products apply gate^T and write g_hg (GateEpi::mode = m)
    GateEpi g[3];
    for (int m = 0; m < 3 && gate; ++m) { g[m] = *gate; g[m].mode = m; }
    CHK(gemm_pl(eng, 0, pass, Apl, la.ld, 0, 0, Wm0, 0, bias, Cp, lc.ld, 0, 0, ne, lc.m0, la.m0, 1.0f, false, gate ? &g[0] : nullptr));
    CHK(gemm_pl(eng, 1, pass, Apl, la.ld, la.m1re, la.m1im, Wm1, lc.m1w, nullptr, Cp, lc.ld, lc.m1re, lc.m1im, ne, lc.m1w, la.m1w, conj, false, gate ? &g[1] : nullptr));
    return gemm_pl(eng, 1, pass, Apl, la.ld, la.m2re, la.m2im, Wm2, lc.m2w, nullptr, Cp, lc.ld, lc.m2re, lc.m2im, ne, lc.m2w, la.m2w, conj, false, gate ? &g[2] : nullptr);
  }
  const float* Af = static_cast<const float*>(A);
  GemmP p = gp_zero();
  p.A = Af; p.lda = la.ld; p.R = R; p.ldr = R ? RAD : 0; p.B = Wm0; p.ldb = la.m0; p.bias = bias;
  p.Cp = Cp; p.ldc = lc.ld; p.M = (int)ne; p.N = lc.m0; p.K = la.m0;
  CHK(launch_gemm(eng, p, R ? A_MODUL : A_PLAIN, 0));
  CHK(gemm_cplx(eng, Af, la.ld, la.m1re, la.m1im, R, R ? RAD : 0, R ? SO2_RAD_M1 : 0, Wm1, la.m1w, lc.m1w, Cp, lc.ld, lc.m1re, lc.m1im, ne, lc.m1w, la.m1w, conj));
  return gemm_cplx(eng, Af, la.ld, la.m2re, la.m2im, R, R ? RAD : 0, R ? SO2_RAD_M2 : 0, Wm2, la.m2w, lc.m2w, Cp, lc.ld, lc.m2re, lc.m2im, ne, lc.m2w, la.m2w, conj);
}

}  // namespace
