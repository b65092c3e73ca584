// umx_api.hip -- host orchestration and C ABI (include/umx.h) of the UMA-S engine for gfx950.
//
// One engine = one GPU.  umx_energy_forces[_dev] evaluates K images of one system as a block
// diagonal graph: K1 radius graph -> K2 frames -> K4/K5 node init + edge-degree embedding ->
// 4 x (K6 norm, K7 edgewise SO(2) message passing, K8 atom-wise FF) -> K9 readout -> K10 analytic
// reverse pass (no autograd) -> K11 normaliser/element references.  Images are processed in
// chunks sized to the HBM workspace budget; activations needed by the reverse pass stay resident
// in HBM (the 288 GB part makes store-not-recompute the cheaper choice).
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <chrono>
#include <cstring>
#include <functional>
#include <map>
#include <set>
#include <string>
#include <vector>

#include "../../include/umx.h"
#include "umx_common.h"
#include "umx_gemm.h"
#include "umx_gemm_pl.h"
#include "umx_gemm_q.h"
#include "umx_kernels_pl.h"
#include "umx_kernels.h"
#include "umx_radial.h"
#include "umx_peer.h"

using namespace umx;

namespace {

std::string g_create_err;

struct Tensor { size_t off = 0; std::vector<int> shape; size_t count = 0; };

struct RadialW {          // one RadialMLP (forward + transposed copies)
  const float *w1g, *w1gT, *ln1w, *ln1b, *w2, *w2T, *b2, *ln2w, *ln2b, *w3, *w3T, *b3;
  const double *tsd, *ttd;     // the element tables of fc1 in double (fused radial head)
  int out;
};
struct LayerW {
  const float *n1w, *n1b, *n2w, *n2b;
  const float *c1m0, *c1m0b, *c1m0T, *c1m1, *c1m1T, *c1m2, *c1m2T;
  const float *c2m0, *c2m0b, *c2m0T, *c2m1, *c2m1T, *c2m2, *c2m2T;
  const float *smlp, *smlpb, *smlpT, *l1w, *l1b, *l1T, *l2w, *l2b, *l2T;       // K8 spectral feed-forward
  const float *g1w, *g1b, *g1T, *g2w, *g2b, *g2T, *g3w, *g3b, *g3T;            // K8 grid feed-forward (ff_grid): grid_mlp.{0,2,4} (+ optional biases), transposes
  RadialW rad;
};

struct ProfRec { hipEvent_t a, b; double flops; int M, N, K, amode, cplx, prec, gz; };

}  // namespace

struct umx_engine {
  int dev = 0;
  hipStream_t stream = nullptr;
  hipEvent_t ev_done = nullptr;    // recorded at the end of every evaluation on the stream it ran on: umx_synchronize waits on THIS, never
                                   // on a caller's stream handle kept from an earlier call (the caller may have destroyed that stream since)
  bool ran_on_caller = false;
  int* d_flags = nullptr;          // [0]: sticky range flag -- an image's energy was not finite (set by k_energy, read at the next host sync)
  hipStream_t stream2 = nullptr;   // second lane: half-chunks alternate streams so HBM-bound producers overlap the other lane's GEMMs
  hipEvent_t ev_fork = nullptr, ev_join = nullptr;
  hipEvent_t ev_tok[2] = {nullptr, nullptr};   // matrix-pipe token of the two lanes (run_plans_alternating)
  // Round 5 pruned the development levers whose A/B is settled (NOTES.md sections 5, 9, 10 keep the measurements): the PL-layout forward
  // operands, pre-split A planes, three-plane PL reverse operands, ring depth 3, two-plane fp16 weights, hardware transcendentals / fp16
  // products inside the fused radial kernels, the side stream, the unfused radial layers, the f16x2b8 mode.  What is left below is what runs.
  std::map<const float*, bool> planes_q;                  // weight plane copies stored in the quad-row layout (else PL)
  int low_sep = 3;                 // UMX_LOW_SEP (gemm_pl): which forward bf16x3 products chain their 2^-16-order plane products from zero
  int align = 2;                   // UMX_ALIGN_PLANES (round 6): "aligned planes" -- the leading bf16 plane of both operands of a FORWARD bf16x3 product is
                                   // quantised to its pass group (8 consecutive k of one row), so that stage 1 of the matrix core's adder (a cut TOWARD
                                   // ZERO at 2^-24 of the pass's largest product, i.e. an error that follows the product's sign) has nothing to cut:
                                   // umx_gemm_pl.h qf_align_magic (A, in registers), want_planes below (weights, at load).  The remainder goes
                                   // down the planes: elements far below their group's largest keep 16-23 bits instead of 24, with an unbiased error.  2 (default): A's leading plane in the PLAIN products (fc3, conv m = 0) -- the complex m > 0
                                   // products take rotated l >= 1 components whose signs follow the edge direction, nothing coherent to remove -- the
                                   // weights' planes in every forward product (free); 1: A's in every forward product; 0: the plain nearest-bf16 leading
                                   // planes of rounds 4-5.  20 000 atoms, four cases (profiles/r06_energy_bias.txt): 0: -9e-7 ... -1.63e-4 eV, 1: -1.3e-5 ...
                                   // +3.9e-5, 2: +4e-7 ... -5.0e-5; c3 step 517.9 / 526.3 / 523.0 ms
  float odd_sign = -1.0f;          // sign-alternating operand rows (umx_kernels_pl.h): -1 = on (default), +1 = off (UMX_ALT_ROWS=0, dev A/B)
  int rev_planes = 2;              // bf16 planes of the REVERSE-pass operands: 2 (3 products, 16-bit) or 3 (6 products, 24-bit: UMX_PRECISION=bf16x3)
  int fwd_fmt = 3;                 // forward operand format (QFmt, umx_kernels_pl.h): 1 = two fp16 planes (UMX_PRECISION=split),
                                   // 3 = plain float32 quad-row blocks, split into three bf16 planes by the GEMM in registers (bf16x3, split-bf16)
  bool rev_qf = false;             // derived at load: reverse quad-row operands (g_msg, g_hg) as float32 blocks (bf16x3)
  std::string precision;           // umx_set_precision: overrides UMX_PRECISION when non-empty
  bool node_ctx = false;           // set around the node-level launches (NodeCtx): only those take the float64-accumulating kernel
  bool node_f64_on = true;         // UMX_NODE_F64=0: node-level linears (atom-wise SO(3) linears, scalar MLP, readout and their transposes) on the
                                   // fp32 MFMA instead of the float64-accumulating kernel (k_gemm_f64acc).  Measured (round 3): the fp32-MFMA form of
                                   // these 14 chained GEMMs shifts the energy by a one-signed -2e-8 eV per atom; the double form costs +1 % at c3
  std::map<const float*, float> plane_scale;             // fp16 form: power-of-two scale folded into the weight planes
  int n_lanes = 0;                 // UMX_STREAMS: 1 / unset = one lane, 2 = two chunks in flight (matrix segments alternating between the lanes; bitwise the
                                   // same results).  Mid-round 5 the engine chose two lanes by itself for batches of >= 1.2 M directed edges (c3 505.2 ->
                                   // 499.0 ms, c4 string 761.2 -> 751.4 ms, profiles/r05_lanes_ab.txt); with the LS forward kernels (one workgroup per CU)
                                   // the gain is gone -- c3 511.1 vs 510.6 ms, c4 string 766.4 vs 773.2 ms, c2 +2 %, c1 +25 % (same file, second part) --
                                   // so the rule is off by default; UMX_LANES_AUTO_EDGES=<n> turns it back on with that threshold
  long lanes_auto_edges = 0;       // UMX_LANES_AUTO_EDGES (0 = no automatic choice)
  int stream_cap = 512;            // two-lane mode caps the grids of the grid-stride streaming kernels at this many workgroups (two per CU) so
                                   // that they run BESIDE the other lane's GEMM
  bool throttle = false;           // set while a two-lane evaluation is being issued
  // graph-parallel single-image mode (umx_gp_begin / umx_gp_step): this rank builds the incoming edges of targets [gp_lo, gp_hi)
  bool gp = false; long gp_lo = 0, gp_hi = 0;
  void* gp_plan = nullptr;         // Plan* of the evaluation in progress (opaque here: Plan is defined below)
  size_t gp_at = 0;
  hipStream_t gp_stream = nullptr;
  void* gp_ws = nullptr;           // WS* kept alive between the steps
  std::string err;
  // weights
  bool have_weights = false;
  float* d_w = nullptr;          // raw blob data section
  float* d_dw = nullptr;         // derived weights
  double* d_dtab = nullptr;      // derived double tables (per-element fc1 contributions of every radial MLP)
  unsigned short* d_bw = nullptr; // plane-interleaved (PL) bf16 copies of the large SO(2)/radial weights
  std::map<const float*, const unsigned short*> planes;   // fp32 weight ptr -> PL planes (P=3 forward weights, P=2 transposed)
  bool pl = true;                 // UMX_PRECISION=split / split-bf16: split-precision plane GEMMs; fp32: fp32-MFMA everywhere
  std::map<std::string, Tensor> wt;
  std::vector<float> h_w;        // host copy of the data section (needed to build derived weights)
  RadialW rdeg{};
  LayerW lw[NL]{};
  const float *emb_sphere = nullptr, *normw = nullptr, *normb = nullptr, *e0 = nullptr, *e0b = nullptr, *e0T = nullptr,
              *e2 = nullptr, *e2b = nullptr, *e2T = nullptr, *e4 = nullptr, *e4b = nullptr;
  double rmsd = 1.0;
  std::vector<double> elem_refs;
  // model variant, read off the tensors of the blob (umx_load_weights; SURVEY.md section 2.4 K8 / Appendix A.5 list them as possible for UMA-S)
  bool ff_grid = false;            // K8 = GridAtomwise (to-grid -> point-wise SiLU MLP -> from-grid) instead of SpectralAtomwise
  int grid_G = 0;                  // grid points (rows of so3_grid.to_grid_mat / from_grid_mat)
  const float *to_grid = nullptr, *from_grid = nullptr;
  bool grid_f64 = true;            // UMX_GRID_F64=0: the grid MLP's three GEMMs on the fp32 MFMA instead of the float64-accumulating node kernel
  int emb_type = 0;                // charge / spin embedding: 0 rand_emb (lookup tables), 1 pos_emb (sin / cos of 2 pi v W), 2 lin_emb (Linear(1 -> C))
  int n_datasets = 5;              // rows of dataset_embedding.weight (0: the model has no dataset embedding, mix_csd takes [charge | spin])
  std::string variant;             // "ff=...;emb=...;datasets=N" (umx_model_variant)
  // system
  bool have_system = false;
  int natoms = 0;
  float cutoff = 6.0f;
  int max_neigh = 300;
  int* d_z = nullptr;
  double* d_sysemb = nullptr;    // system embedding in DOUBLE (added to every atom: a float32 copy's error would be shared by all atoms)
  double* d_gmu = nullptr;       // gaussian centres mu_k = k * cutoff/63 in double
  double gcoef = 0.0;
  double refsum = 0.0;
  // workspace
  size_t ws_limit = 0;
  size_t ws_cap_default = (size_t)160 << 30;
  char* arena = nullptr;
  size_t arena_bytes = 0;
  long cap_nodes = 0, cap_edges = 0;
  int* d_deg_all = nullptr; int* d_cand_all = nullptr; long deg_all_cap = 0;
  int* d_img_edges = nullptr; long img_edges_cap = 0;
  // partitioned evaluation of ONE oversized image on one GPU (eval_partitioned): per-partition degree arrays and partial forces
  int force_parts = 0;             // UMX_FORCE_PARTS (dev / tests): evaluate every image in this many target-node partitions
  int* d_part_deg = nullptr; float* d_part_f = nullptr; long part_cap = 0;
  int last_parts = 0;              // partitions used by the most recent evaluation (0: the ordinary path)
  int last_lanes = 1;              // lanes (chunks in flight) of the most recent evaluation (umx_last_lanes)
  int arena_allocs = 0;            // how often the workspace has been (re-)allocated (umx_workspace_stats)
  bool ws_eager = false;           // UMX_WS_EAGER=1: size the workspace for the whole batch at once (the behaviour before ABI v8)
  long ws_soft_edges = 320000;     // UMX_WS_SOFT_EDGES: directed edges per chunk the workspace starts with when nothing else is known
  double t_first_eval = -1.0;      // steady-clock seconds of the first evaluation (amortised workspace growth)
  int hint_applied = 0;            // the hint value the workspace has been sized for already
  int hint_images = 0;             // umx_reserve_images: size the workspace for this many images at the next growth
  // host io staging for the host-pointer entry point
  float* d_io_pos = nullptr; double* d_io_e = nullptr; float* d_io_f = nullptr; long io_cap = 0, io_img_cap = 0;
  // stats / profiling / debug
  int64_t last_edges = 0; int32_t last_maxdeg = 0;
  bool may_truncate = true;      // the largest degree of the evaluation being planned reaches max_neigh: k_graph_fill takes its truncating (LDS) form
  bool prof_on = false;
  std::vector<ProfRec> prof;
  size_t prof_used = 0;
  bool dbg_on = false;
  std::map<std::string, std::vector<char>> dbg;
};

namespace {

#define HIPCHK(eng, expr)                                                                         \
  do {                                                                                            \
    hipError_t _e = (expr);                                                                       \
    if (_e != hipSuccess) {                                                                       \
      (eng)->err = std::string(#expr) + ": " + hipGetErrorName(_e) + " (" + hipGetErrorString(_e) + ")"; \
      return UMX_ERR_HIP;                                                                         \
    }                                                                                             \
  } while (0)

#define CHK(expr) do { int _s = (expr); if (_s != UMX_OK) return _s; } while (0)

int fail(umx_engine* e, int code, const std::string& msg) { e->err = msg; return code; }

inline unsigned nblk(long n, int per) { return (unsigned)((n + per - 1) / per); }

// HIP-event bracket around one launch for umx_profile_read (prec: > 0 split-precision GEMM family, 0 fp32 GEMM, < 0 fused radial kernels)
ProfRec* prof_open(umx_engine* eng, double flops, int prec, long M, int N, int K) {
  if (!eng->prof_on) return nullptr;
  if (eng->prof_used == eng->prof.size()) {
    ProfRec r;
    if (hipEventCreate(&r.a) != hipSuccess || hipEventCreate(&r.b) != hipSuccess) return nullptr;
    r.flops = 0; eng->prof.push_back(r);
  }
  ProfRec* pr = &eng->prof[eng->prof_used++];
  pr->flops = flops; pr->M = (int)M; pr->N = N; pr->K = K; pr->amode = 0; pr->cplx = 0; pr->gz = 1; pr->prec = prec;
  (void)hipEventRecord(pr->a, eng->stream);
  return pr;
}
inline void prof_close(umx_engine* eng, ProfRec* pr) { if (pr) (void)hipEventRecord(pr->b, eng->stream); }
// grid of a grid-stride ("virtual block") kernel: all blocks normally, capped in throttled two-lane mode
inline unsigned vgrid(const umx_engine* eng, unsigned blocks) {
  return (eng->throttle && eng->stream_cap > 0 && blocks > (unsigned)eng->stream_cap) ? (unsigned)eng->stream_cap : blocks;
}

// ---- GEMM launcher -----------------------------------------------------------------------------
GemmP gp_zero() { GemmP p; std::memset(&p, 0, sizeof(p)); p.conj = 1.0f; return p; }

int launch_gemm(umx_engine* eng, const GemmP& p, int amode, int cplx, int epi, int gz = 1) {
  if (p.M <= 0) return UMX_OK;
  if (p.K % G_BK != 0) return fail(eng, UMX_ERR_ARG, "gemm: K not a multiple of 32");
  const int bmr = cplx ? 64 : 128, bnc = cplx ? 64 : 128;
  const long nM = (p.M + bmr - 1) / bmr, nN = (p.N + bnc - 1) / bnc;
  const long blocks = ((nM + 7) / 8) * 8 * nN;
  dim3 grid((unsigned)blocks, 1, (unsigned)gz), block(256);
  ProfRec* pr = nullptr;
  if (eng->prof_on) {
    if (eng->prof_used == eng->prof.size()) {
      ProfRec r; HIPCHK(eng, hipEventCreate(&r.a)); HIPCHK(eng, hipEventCreate(&r.b)); r.flops = 0; eng->prof.push_back(r);
    }
    pr = &eng->prof[eng->prof_used++];
    pr->flops = cplx ? 8.0 * p.M * (double)p.N * p.K : 2.0 * p.M * (double)p.N * p.K * gz;
    pr->M = p.M; pr->N = p.N; pr->K = p.K; pr->amode = amode; pr->cplx = cplx; pr->gz = gz; pr->prec = 0;
    HIPCHK(eng, hipEventRecord(pr->a, eng->stream));
  }
  if (eng->node_f64_on && eng->node_ctx && !cplx && epi == E_BIAS && (amode == A_PLAIN || amode == A_SILU)) {
    const dim3 g64((unsigned)(((p.M + 63) / 64) * ((p.N + 63) / 64)), 1, (unsigned)gz);
    if (amode == A_SILU) hipLaunchKernelGGL(k_gemm_f64acc<A_SILU>, g64, block, 0, eng->stream, p);
    else hipLaunchKernelGGL(k_gemm_f64acc<A_PLAIN>, g64, block, 0, eng->stream, p);
    HIPCHK(eng, hipGetLastError());
    if (pr) HIPCHK(eng, hipEventRecord(pr->b, eng->stream));
    return UMX_OK;
  }
  const int key = amode * 100 + cplx * 10 + epi;
  switch (key) {
    case A_PLAIN * 100 + 0 + E_BIAS: hipLaunchKernelGGL((umx_gemm_kernel<A_PLAIN, 0, E_BIAS>), grid, block, 0, eng->stream, p); break;
    case A_PLAIN * 100 + 10 + E_BIAS: hipLaunchKernelGGL((umx_gemm_kernel<A_PLAIN, 1, E_BIAS>), grid, block, 0, eng->stream, p); break;
    case A_MODUL * 100 + 0 + E_BIAS: hipLaunchKernelGGL((umx_gemm_kernel<A_MODUL, 0, E_BIAS>), grid, block, 0, eng->stream, p); break;
    case A_MODUL * 100 + 10 + E_BIAS: hipLaunchKernelGGL((umx_gemm_kernel<A_MODUL, 1, E_BIAS>), grid, block, 0, eng->stream, p); break;
    case A_SILU * 100 + 0 + E_BIAS: hipLaunchKernelGGL((umx_gemm_kernel<A_SILU, 0, E_BIAS>), grid, block, 0, eng->stream, p); break;
    default: return fail(eng, UMX_ERR_ARG, "gemm: variant not instantiated");
  }
  HIPCHK(eng, hipGetLastError());
  if (pr) HIPCHK(eng, hipEventRecord(pr->b, eng->stream));
  return UMX_OK;
}

struct NodeCtx { umx_engine* e; explicit NodeCtx(umx_engine* eng) : e(eng) { e->node_ctx = true; } ~NodeCtx() { e->node_ctx = false; } };

// plain C = A . B^T (+bias, +resid)
int gemm_plain(umx_engine* eng, const float* A, long lda, int offA, const float* B, long ldb, const float* bias, float* Cp,
               long ldc, int offC, long M, int N, int K, int amode = A_PLAIN, int gz = 1, long zA = 0, long zC = 0,
               const float* resid = nullptr, long ldres = 0, int offRes = 0, long zRes = 0) {
  GemmP p = gp_zero();
  p.A = A; p.lda = lda; p.offA0 = offA; p.B = B; p.ldb = ldb; p.bias = bias; p.Cp = Cp; p.ldc = ldc; p.offC = offC;
  p.M = (int)M; p.N = N; p.K = K; p.zA = zA; p.zC = zC; p.resid = resid; p.ldres = ldres; p.offRes = offRes; p.zRes = zRes;
  return launch_gemm(eng, p, amode, 0, E_BIAS, gz);
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
  return launch_gemm(eng, p, R ? A_MODUL : A_PLAIN, 1, E_BIAS);
}

// Split-precision GEMM of the large SO(2) / radial linears.  P = 3 at the call site: a FORWARD product, P = 2: a reverse-pass product (the
// operand formats and plane counts are the engine's, fixed by the precision mode at umx_load_weights):
//   forward, bf16x3 / split-bf16 : A = float32 quad-row blocks split into three bf16 planes by the GEMM in registers, B = three bf16 planes (6 products)
//   forward, split (fp16)        : A = two fp16 planes of 16 x activation, B = three exact fp16 planes (4 products)
//   reverse, bf16x3              : conv^T: A = float32 quad-row blocks (g_msg / g_hg), B = three bf16 planes, 6 products (umx_gemm_q.h);
//                                  fc3^T: A = float32 ROWS (g_rad, a_f32rows) split by umx_gemm_pl16_kernel<.., AF = 1>
//   reverse, split / split-bf16  : A, B = two PL bf16 planes, 3 products (umx_gemm_pl.h)
// Wkey = fp32 device pointer of the weight (its plane copy is looked up); a_cols = total columns of the A matrix; offsets in columns.
int gemm_pl(umx_engine* eng, int cplx, int P, const unsigned short* Apl, int a_cols, int offA0, int offA1, const float* Wkey, int bHalf,
            const float* bias, float* Cp, long ldc, int offC, int offCi, long M, int N, int K, float conj, bool a_f32rows = false) {
  if (M <= 0) return UMX_OK;
  auto it = eng->planes.find(Wkey);
  if (it == eng->planes.end()) return fail(eng, UMX_ERR_ARG, "gemm_pl: weight has no PL copy");
  if (K % 32 != 0) return fail(eng, UMX_ERR_ARG, "gemm_pl: K not a multiple of 32");
  const bool fwd = (P == 3);
  if (!fwd) P = eng->rev_planes;
  GemmPL q;
  std::memset(&q, 0, sizeof(q));
  q.Apl = Apl; q.lda = (long)a_cols * P; q.offA0 = offA0; q.offA1 = offA1; q.Bpl = it->second; q.ldb = (long)K * P; q.bHalf = bHalf;
  q.Cp = Cp; q.ldc = ldc; q.offC = offC; q.offCi = offCi; q.bias = bias; q.conj = conj; q.M = (int)M; q.N = N; q.K = K;
  q.odd_sign = eng->odd_sign;
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
  const bool ls = fwd && eng->fwd_fmt == 3 && (eng->low_sep == 2 || (eng->low_sep == 3 && !cplx) || (eng->low_sep == 1 && !cplx && K == RH));
  // (an LS product picks its tile from N alone: the two LS forms fold the small products in at different points, and an image must get the
  //  same bits whether it is evaluated alone or in a batch -- tests/test_gpu_graph_parallel.py, test_gpu_parity.py batch independence)
  const bool wide = N % (cplx ? 128 : 256) == 0 && (fills || ls);
  const int bnc = wide ? (cplx ? 128 : 256) : (cplx ? 64 : 128);
  const long nN = (N + bnc - 1) / bnc;
  const dim3 grid((unsigned)(((nM + 7) / 8) * 8 * nN)), block(512);
  const auto pq = eng->planes_q.find(Wkey);
  const bool quad = fwd || (P == 3 && pq != eng->planes_q.end() && pq->second);      // quad-row operands (umx_gemm_q.h)
  ProfRec* pr = nullptr;
  if (eng->prof_on) {
    if (eng->prof_used == eng->prof.size()) {
      ProfRec r; HIPCHK(eng, hipEventCreate(&r.a)); HIPCHK(eng, hipEventCreate(&r.b)); r.flops = 0; eng->prof.push_back(r);
    }
    pr = &eng->prof[eng->prof_used++];
    pr->flops = cplx ? 8.0 * M * (double)N * K : 2.0 * M * (double)N * K;
    pr->M = (int)M; pr->N = N; pr->K = K; pr->amode = 9; pr->cplx = cplx; pr->gz = 1;
    pr->prec = (fwd && eng->fwd_fmt == 1) ? 24 : P;      // 24: two fp16 planes, 4 products; 3 / 2: bf16 planes, 6 / 3 products
    HIPCHK(eng, hipEventRecord(pr->a, eng->stream));
  }
#define UMX_Q(...)                                                                                                             \
  do {                                                                                                                         \
    if (cplx) { if (wide) hipLaunchKernelGGL((umx_gemm_q_kernel<1, 1, __VA_ARGS__>), grid, block, 0, eng->stream, q);          \
                else hipLaunchKernelGGL((umx_gemm_q_kernel<1, 0, __VA_ARGS__>), grid, block, 0, eng->stream, q); }             \
    else      { if (wide) hipLaunchKernelGGL((umx_gemm_q_kernel<0, 1, __VA_ARGS__>), grid, block, 0, eng->stream, q);          \
                else hipLaunchKernelGGL((umx_gemm_q_kernel<0, 0, __VA_ARGS__>), grid, block, 0, eng->stream, q); }             \
  } while (0)
  if (quad && fwd && eng->fwd_fmt == 1) {
    // two fp16 planes of 16 x (activations), three exact planes of s_w x (weights): C = (A' . B'^T) / (16 s_w)
    q.lda = (long)a_cols * 2; q.ldb = (long)K * 3;
    const auto sc = eng->plane_scale.find(Wkey);
    if (sc == eng->plane_scale.end()) return fail(eng, UMX_ERR_ARG, "gemm_pl: weight has no fp16 plane copy");
    q.cscale = 1.0f / (QF16_SCALE * sc->second);
    UMX_Q(2, 2, 1, 4, 3);
  } else if (quad) {
    // A = float32 quad-row blocks, split into the three bf16 planes in registers; weights as three bf16 planes
    if (fwd && eng->fwd_fmt != 3) return fail(eng, UMX_ERR_ARG, "gemm_pl: unknown forward operand format");
    if (!fwd && !eng->rev_qf) return fail(eng, UMX_ERR_ARG, "gemm_pl: quad-row reverse operands exist in the bf16x3 mode only");
    q.lda = (long)a_cols * 3; q.ldb = (long)K * 3;
    const bool al = fwd && (eng->align == 1 || (eng->align == 2 && !cplx));      // aligned planes: forward products only (the weights' planes were built to match, umx_load_weights)
    if (!ls) { if (al) UMX_Q(3, 2, 0, 6, 3, 1, 0, 1); else UMX_Q(3, 2, 0, 6, 3, 1); }
    else if (wide) {      // 256 x 256 tiles: one spare accumulator, folded in every k-step
      if (al) { if (cplx) hipLaunchKernelGGL((umx_gemm_q_kernel<1, 1, 3, 2, 0, 6, 3, 1, 1, 1>), grid, block, 0, eng->stream, q);
                else hipLaunchKernelGGL((umx_gemm_q_kernel<0, 1, 3, 2, 0, 6, 3, 1, 1, 1>), grid, block, 0, eng->stream, q); }
      else if (cplx) hipLaunchKernelGGL((umx_gemm_q_kernel<1, 1, 3, 2, 0, 6, 3, 1, 1>), grid, block, 0, eng->stream, q);
      else hipLaunchKernelGGL((umx_gemm_q_kernel<0, 1, 3, 2, 0, 6, 3, 1, 1>), grid, block, 0, eng->stream, q);
    } else {              // 256 x 128 tiles: a second accumulator set for the whole k loop (190 VGPRs: one workgroup per CU instead of two --
                          // +10 ms at c3 for conv-1 / conv-2 m = 0; deeper rings do not buy it back: S = 3 / 4 measured +5 / +6 ms.  Round 6 measured the
                          // per-k-step fold of the wide tiles here too: 167-172 VGPRs as compiled (one workgroup per CU all the same); forced into the
                          // 128 VGPRs a second workgroup needs it spills 19 registers: +40 ms, and 48 float32 folds per output instead of one move
                          // the 20 000-atom energies to -9e-5 eV on two of four cases -- profiles/r06_ls_ab.txt; removed)
      if (al) { if (cplx) hipLaunchKernelGGL((umx_gemm_q_kernel<1, 0, 3, 2, 0, 6, 3, 1, 2, 1>), grid, block, 0, eng->stream, q);
                else hipLaunchKernelGGL((umx_gemm_q_kernel<0, 0, 3, 2, 0, 6, 3, 1, 2, 1>), grid, block, 0, eng->stream, q); }
      else if (cplx) hipLaunchKernelGGL((umx_gemm_q_kernel<1, 0, 3, 2, 0, 6, 3, 1, 2>), grid, block, 0, eng->stream, q);
      else hipLaunchKernelGGL((umx_gemm_q_kernel<0, 0, 3, 2, 0, 6, 3, 1, 2>), grid, block, 0, eng->stream, q);
    }
  } else if (P == 3) {
    // three-plane PL products of the bf16x3 reverse pass: the radial fc3^T of the layers (A = float32 rows, split in registers) and of the
    // edge-degree embedding (A = three PL planes written by k_rotate_back_bwd<3, 3>); both plain, N = 128, 256 x 128 tiles
    if (cplx || N > 128) return fail(eng, UMX_ERR_ARG, "gemm_pl: three-plane PL products are instantiated for the plain N <= 128 (radial fc3^T) products only");
    const dim3 g128((unsigned)(((nM + 7) / 8) * 8 * ((N + 127) / 128)));
    if (a_f32rows) {
      q.lda = (long)a_cols * 2;                  // row pitch in 2-byte units
      hipLaunchKernelGGL((umx_gemm_pl16_kernel<0, 3, 2, 4, 2, 2, 2, 0, 1>), g128, block, 0, eng->stream, q);     // (an 8 x 1 wave layout measured the same)
    } else {
      hipLaunchKernelGGL((umx_gemm_pl_kernel<0, 3, 2, 4, 2, 2, 2>), g128, block, 0, eng->stream, q);
    }
  } else if (wide) {
    if (cplx) hipLaunchKernelGGL((umx_gemm_pl16_kernel<1, 2, 2, 4, 2, 2, 4>), grid, block, 0, eng->stream, q);
    else hipLaunchKernelGGL((umx_gemm_pl16_kernel<0, 2, 2, 4, 2, 2, 4>), grid, block, 0, eng->stream, q);
  } else {
    // MFMA shape per GEMM (measured in the c3 pipeline): 16x16x32 wins 1-7 % on the complex SO(2) GEMMs and on K >= 512,
    // 32x32x16 wins 5-10 % on the short-K plain ones (radial fc3^T, conv-2^T m = 0)
    if (cplx || K >= 512) {
      if (cplx) hipLaunchKernelGGL((umx_gemm_pl16_kernel<1, 2, 3, 4, 2, 2, 2>), grid, block, 0, eng->stream, q);
      else hipLaunchKernelGGL((umx_gemm_pl16_kernel<0, 2, 3, 4, 2, 2, 2>), grid, block, 0, eng->stream, q);
    } else {
      if (cplx) hipLaunchKernelGGL((umx_gemm_pl_kernel<1, 2, 3, 4, 2, 2, 2>), grid, block, 0, eng->stream, q);
      else hipLaunchKernelGGL((umx_gemm_pl_kernel<0, 2, 3, 4, 2, 2, 2>), grid, block, 0, eng->stream, q);
    }
  }
#undef UMX_Q
  HIPCHK(eng, hipGetLastError());
  if (pr) HIPCHK(eng, hipEventRecord(pr->b, eng->stream));
  return UMX_OK;
}

// ---- workspace ---------------------------------------------------------------------------------
struct WS {
  // node level
  int *deg, *row_ptr, *stats;
  float* xs[2 * NL + 1];
  float* xn[NL];
  float *xn2, *ffhg, *xf, *pre1, *pre2, *enode;
  float* gspre[NL];
  float* ffh[NL];
  float* ffg1[NL];                 // grid feed-forward: pre-activations of the two hidden layers, (nodes x G) rows x H, kept for the reverse pass
  float* ffg2[NL];
  float *gridA, *gridB;            // grid feed-forward: (nodes x G) x C temporaries
  float *G0, *G1, *G2, *ggs, *n128a, *n128b;
  // edge level
  int *esrc, *edst, *ez, *out_ptr, *out_cur, *out_edge;
  float *evec, *frame, *dedd, *dedd_rad, *tau, *tau2, *gvec;
  float* h1pre[NL + 1];
  float* h2pre[NL + 1];
  float *ra, *rad_deg;
  float* rad[NL];
  float* hg[NL];
  float* msg[NL];
  float *xrot, *hid, *gmsg, *ghg, *gy1, *grad, *e128a;
  unsigned short *y1pl, *hidpl, *a2pl, *gmsgpl, *ghgpl, *gradpl;   // split path: pre-split GEMM operands (forward: quad-row planes, reverse: PL)
};

struct Bump {
  char* base; size_t off = 0;
  template <class T> T* take(size_t n) {
    off = (off + 255) & ~size_t(255);
    T* p = base ? reinterpret_cast<T*>(base + off) : nullptr;
    off += n * sizeof(T);
    return p;
  }
};

// workspace mode: 0 = fp32 path, else (planes of the forward operands) + 16 when the reverse operands have three planes
inline int ws_mode(const umx_engine* eng) { return !eng->pl ? 0 : 2 + (eng->rev_planes == 3 ? 16 : 0) + (eng->rev_qf ? 32 : 0); }   // (forward operands: 4 B per element in both split formats)
// ... + the grid points of the grid feed-forward in bits 8+ (its per-node buffers scale with G; 0 = spectral feed-forward)
inline int ws_mode_g(const umx_engine* eng) { return ws_mode(eng) | ((eng->ff_grid ? eng->grid_G : 0) << 8); }

// Workspace layout.  PERSISTENT buffers live from the forward to the reverse pass of an evaluation (node-level state, the graph, and the
// per-edge activations of all four layers: ~72 KB per directed edge); TRANSIENT buffers are the operands between a producer and a GEMM
// (~48 KB per edge) and are dead at every exchange point of the plan -- which is what lets the partitions of ONE oversized image share a
// single transient region (eval_partitioned).  pl: 0 = fp32 path, else the number of planes of the forward operands (3 bf16 / 2 fp16).
void carve_persist(Bump& b, long nn, long ne, WS& t, int gridG = 0) {
  t.deg = nullptr;  // deg comes from the per-call array
  t.row_ptr = b.take<int>(nn + 1); t.stats = b.take<int>(4);
  for (auto& x : t.xs) x = b.take<float>(nn * ROW);
  for (auto& x : t.xn) x = b.take<float>(nn * ROW);
  t.xn2 = b.take<float>(nn * ROW); t.ffhg = b.take<float>(nn * ROW); t.xf = b.take<float>(nn * ROW);
  t.pre1 = b.take<float>(nn * H); t.pre2 = b.take<float>(nn * H); t.enode = b.take<float>(nn);
  for (auto& x : t.gspre) x = b.take<float>(nn * 2 * H);
  for (auto& x : t.ffh) x = b.take<float>(nn * ROW);
  for (auto& x : t.ffg1) x = gridG ? b.take<float>(nn * gridG * H) : nullptr;
  for (auto& x : t.ffg2) x = gridG ? b.take<float>(nn * gridG * H) : nullptr;
  t.gridA = gridG ? b.take<float>(nn * gridG * C) : nullptr; t.gridB = gridG ? b.take<float>(nn * gridG * C) : nullptr;
  t.G0 = b.take<float>(nn * ROW); t.G1 = b.take<float>(nn * ROW); t.G2 = b.take<float>(nn * ROW);
  t.ggs = b.take<float>(nn * 2 * H); t.n128a = b.take<float>(nn * H); t.n128b = b.take<float>(nn * H);
  t.esrc = b.take<int>(ne); t.edst = b.take<int>(ne); t.ez = b.take<int>(ne); t.out_edge = b.take<int>(ne);
  t.out_ptr = b.take<int>(nn + 1); t.out_cur = b.take<int>(nn + 1);
  t.evec = b.take<float>(ne * 4); t.frame = b.take<float>(ne * FRAME); t.dedd = b.take<float>(ne); t.dedd_rad = b.take<float>(ne);
  t.tau = b.take<float>(ne * 4); t.tau2 = b.take<float>(ne * 4); t.gvec = b.take<float>(ne * 4);
  for (auto& x : t.h1pre) x = b.take<float>(ne * RH);
  for (auto& x : t.h2pre) x = b.take<float>(ne * RH);
  t.rad_deg = b.take<float>(ne * 3 * C);
  for (auto& x : t.rad) x = b.take<float>(ne * RAD);
  for (auto& x : t.hg) x = b.take<float>(ne * HG);
  for (auto& x : t.msg) x = b.take<float>(ne * ROW);
}
void carve_trans(Bump& b, long ne, WS& t, int pl) {
  t.ra = b.take<float>(ne * RH);
  t.hid = b.take<float>(ne * ROW); t.gy1 = b.take<float>(ne * XROT);
  t.e128a = b.take<float>(ne * RH);
  t.xrot = t.ghg = t.grad = nullptr;
  t.y1pl = t.hidpl = t.a2pl = t.gmsgpl = t.ghgpl = t.gradpl = nullptr;
  if (pl) {
    t.gmsg = b.take<float>(ne * 3 * C);                      // only the edge-degree backward uses fp32 g_msg (E x 384)
    const long ne4 = (ne + 3) / 4 * 4;          // the quad-row (Q3) layout stores rows in groups of four
    const long fp = pl & 15, rp = (pl & 16) ? 3 : 2;             // 2-byte units per element of the forward / reverse operands
    const long rq = (pl & 32) ? 2 : rp;                          // ... of the quad-row reverse operands (float32 blocks: 2)
    t.y1pl = b.take<unsigned short>(ne4 * XROT * fp); t.hidpl = b.take<unsigned short>(ne4 * ROW * fp);
    t.a2pl = b.take<unsigned short>(ne4 * RH * fp); t.gmsgpl = b.take<unsigned short>(ne4 * ROW * rq);      // (ne4: the quad-row form of the bf16x3 reverse operands)
    t.ghgpl = b.take<unsigned short>(ne4 * HG * rq); t.gradpl = b.take<unsigned short>(ne * RAD * rp);
  } else {
    t.xrot = b.take<float>(ne * XROT); t.gmsg = b.take<float>(ne * ROW);
    t.ghg = b.take<float>(ne * HG); t.grad = b.take<float>(ne * RAD);
  }
}
size_t carve(char* base, long nn, long ne, WS* w, int pl) {
  Bump b{base};
  WS t;
  carve_persist(b, nn, ne, t, pl >> 8);
  carve_trans(b, ne, t, pl & 255);
  if (w) *w = t;
  return (b.off + 255) & ~size_t(255);
}

// UMX_DEBUG_ONLY (tests): a comma-separated list of name prefixes; with captures on, only the names that start with one of them are kept
// (a 44 k-edge system holds ~1 GB of captures per layer and pass)
bool dbg_wanted(const std::string& name) {
  const char* ev = std::getenv("UMX_DEBUG_ONLY");
  if (!ev || !*ev) return true;
  const std::string only(ev);
  for (size_t a = 0; a <= only.size();) {
    size_t b = only.find(',', a);
    if (b == std::string::npos) b = only.size();
    if (b > a && name.compare(0, b - a, only, a, b - a) == 0) return true;
    a = b + 1;
  }
  return false;
}

int dbg_capture(umx_engine* eng, const std::string& name, const void* dptr, size_t bytes) {
  if (!eng->dbg_on || !dbg_wanted(name)) return UMX_OK;
  std::vector<char>& v = eng->dbg[name];
  v.resize(bytes);
  HIPCHK(eng, hipStreamSynchronize(eng->stream));
  if (bytes) HIPCHK(eng, hipMemcpy(v.data(), dptr, bytes, hipMemcpyDeviceToHost));
  return UMX_OK;
}
#define DBG(name, ptr, count) CHK(dbg_capture(eng, name, ptr, (size_t)(count) * sizeof(*(ptr))))

// ---- radial MLP forward / backward -------------------------------------------------------------
// Each is split into its small layers (fp32 GEMMs + LayerNorm/SiLU kernels: "streaming" work) and the one large fc3 GEMM, so that
// the two-lane executor can treat the large GEMM as a matrix-pipe segment (see Plan below).
int radial_fwd_head(umx_engine* eng, const WS& w, const RadialW& r, int slot, long ne) {
  // one persistent kernel: gaussians -> fc1 -> LN+SiLU -> fc2 -> LN+SiLU -> the fc3 operand (fp16 planes / float32 quad-row blocks of the
  // split modes, or fp32 rows in w.ra); the intermediate rows never reach HBM
  const bool planes = eng->pl && eng->planes.count(r.w3);
  const unsigned tiles = nblk(ne, 64);                      // two 32-row MFMA tiles per workgroup tile, two workgroups per CU
  const dim3 grid(vgrid(eng, tiles < 512u ? tiles : 512u));
  ProfRec* pr = prof_open(eng, 2.0 * ne * ((double)NG * RH + (double)RH * RH), -1, ne, RH, NG + RH);
#define UMX_RH_LAUNCH(Q, OUT) hipLaunchKernelGGL((k_radial_head<Q>), grid, dim3(256), 0, eng->stream, w.evec, w.ez, eng->gcoef, eng->d_gmu, r.w1g, r.tsd, r.ttd, r.ln1w, \
                                                 r.ln1b, r.w2, r.b2, r.ln2w, r.ln2b, w.h1pre[slot], w.h2pre[slot], (void*)(OUT), ne, eng->odd_sign)
  if (planes && eng->fwd_fmt == 1) UMX_RH_LAUNCH(2, w.a2pl); else if (planes) UMX_RH_LAUNCH(4, w.a2pl); else UMX_RH_LAUNCH(0, w.ra);
#undef UMX_RH_LAUNCH
  prof_close(eng, pr);
  HIPCHK(eng, hipGetLastError());
  return UMX_OK;
}
int radial_fwd_fc3(umx_engine* eng, const WS& w, const RadialW& r, long ne, float* rad_out) {
  if (eng->pl && eng->planes.count(r.w3)) return gemm_pl(eng, 0, 3, w.a2pl, RH, 0, 0, r.w3, 0, r.b3, rad_out, r.out, 0, 0, ne, r.out, RH, 1.0f);
  return gemm_plain(eng, w.ra, RH, 0, r.w3, RH, r.b3, rad_out, r.out, 0, ne, r.out, RH);
}
int radial_fwd(umx_engine* eng, const WS& w, const RadialW& r, int slot, long ne, float* rad_out) {
  CHK(radial_fwd_head(eng, w, r, slot, ne));
  return radial_fwd_fc3(eng, w, r, ne, rad_out);
}

int radial_bwd_fc3(umx_engine* eng, const WS& w, const RadialW& r, long ne, const float* grad, const unsigned short* gradpl, bool f32rows = false) {
  if (gradpl) return gemm_pl(eng, 0, 2, gradpl, r.out, 0, 0, r.w3T, 0, nullptr, w.e128a, RH, 0, 0, ne, RH, r.out, 1.0f, f32rows);
  return gemm_plain(eng, grad, r.out, 0, r.w3T, r.out, nullptr, w.e128a, RH, 0, ne, RH, r.out);
}
int radial_bwd_tail(umx_engine* eng, const WS& w, const RadialW& r, int slot, long ne) {
  // one persistent kernel: LN+SiLU bwd -> fc2^T -> LN+SiLU bwd -> fc1^T -> dE/dd through the gaussians (accumulated into dedd_rad)
  const unsigned tiles = nblk(ne, 64);
  const dim3 grid(vgrid(eng, tiles < 512u ? tiles : 512u));
  ProfRec* pr = prof_open(eng, 2.0 * ne * ((double)NG * RH + (double)RH * RH), -1, ne, RH, NG + RH);
  const std::string t = slot == NL ? ".deg" : "." + std::to_string(slot);
  DBG("g_a2" + t, w.e128a, ne * RH);           // (debug) the output of fc3^T, the tail's input
  hipLaunchKernelGGL(k_radial_tail, grid, dim3(256), 0, eng->stream, w.e128a, w.h2pre[slot], w.h1pre[slot], w.evec, eng->gcoef, eng->d_gmu, r.ln2w, r.ln2b, r.ln1w, r.ln1b,
                     r.w2T, r.w1gT, w.dedd_rad, ne);
  prof_close(eng, pr);
  HIPCHK(eng, hipGetLastError());
  DBG("dedd_rad" + t, w.dedd_rad, ne);         // (debug) accumulated over the layers (NL - 1 first, then the edge-degree MLP)
  return UMX_OK;
}
int radial_bwd(umx_engine* eng, const WS& w, const RadialW& r, int slot, long ne, const float* grad, const unsigned short* gradpl = nullptr) {
  CHK(radial_bwd_fc3(eng, w, r, ne, grad, gradpl));
  return radial_bwd_tail(eng, w, r, slot, ne);
}

// SO(3) linear on l-primary node rows: ONE launch, gridDim.z = 9 coefficients, the weights of degree l(z) picked per z (zBl);
// the bias acts on the l = 0 row only
int so3_linear(umx_engine* eng, const float* A, const float* Wl, const float* bias, float* Cp, long nn, const float* resid) {
  GemmP p = gp_zero();
  p.A = A; p.lda = ROW; p.offA0 = 0; p.B = Wl; p.ldb = C; p.bias = bias; p.Cp = Cp; p.ldc = ROW; p.offC = 0;
  p.M = (int)nn; p.N = C; p.K = C; p.zA = C; p.zC = C; p.resid = resid; p.ldres = ROW; p.offRes = 0; p.zRes = C; p.zBl = (long)C * C;
  NodeCtx node(eng);
  return launch_gemm(eng, p, A_PLAIN, 0, E_BIAS, S);
}

// ---- one chunk: nn nodes (= images * natoms), edges counted on the fly --------------------------
// The chunk's launch sequence is recorded as a PLAN of segments instead of being issued directly.  A segment is either
// "matrix" (a group of the large split-precision GEMMs: MFMA-bound, one LDS-filling workgroup per CU) or "stream" (everything
// else: the HBM-bound gather / rotate / gate / reduce kernels and the small fp32 GEMMs).  With one lane the executor simply
// issues the segments in order.  With two lanes (UMX_STREAMS=2) it issues the plans of two chunks alternately and hands a
// TOKEN from matrix segment to matrix segment across the lanes (events), so that at any time at most one lane occupies the
// matrix pipe while the other lane's stream segments run beside it on the same CUs -- the two bounds (MFMA and HBM)
// overlap instead of adding up (NOTES.md section 5).
struct Seg { bool matrix; std::function<int()> fn; float* sync_buf = nullptr; size_t sync_count = 0; };
struct Plan {
  std::vector<Seg> segs;
  void stream(std::function<int()> f) { segs.push_back({false, std::move(f)}); }
  void matrix(std::function<int()> f) { segs.push_back({true, std::move(f)}); }
  // graph-parallel single-image mode: an exchange point -- the buffer holds this rank's partial sums over ITS edges and must be
  // summed over the ranks (all-reduce, done by the caller between two umx_gp_step calls) before the next segment runs
  void sync(float* buf, size_t count) { Seg sg{false, nullptr}; sg.sync_buf = buf; sg.sync_count = count; segs.push_back(std::move(sg)); }
};

void plan_chunk(umx_engine* eng, WS& w, const float* d_pos, const int* d_deg, const int* d_cand, long nimg, long ne, double* d_energy,
                float* d_forces, Plan& P) {
  const int N = eng->natoms;
  const long nn = nimg * N;
  const float rc2 = eng->cutoff * eng->cutoff;
  const dim3 B256(256);
  const bool pl = eng->pl;
  const bool gp = eng->gp;                                       // graph-parallel: partial sums over this rank's edges + exchange points
  const bool may_trunc = eng->may_truncate;                      // some node of this call has more candidates than max_neigh (known on the host)
  const bool fused_rev = eng->pl || !eng->dbg_on;     // k_modrot_bwd_pl produces g_xn itself (fp32 mode with debug captures: the unfused kernels, which expose xrot / g_xrot)
  const long g_lo = gp ? eng->gp_lo : 0, g_hi = gp ? eng->gp_hi : nn;
  // every closure reads eng->stream when it RUNS (the executor points it at the lane's stream)
  // K1 graph, K4 + K5
  P.stream([=, &w]() -> int {
    hipStream_t s = eng->stream;
    hipLaunchKernelGGL(k_scan, dim3(1), dim3(1024), 0, s, d_deg, nn, w.row_ptr, w.stats);
    if (may_trunc) hipLaunchKernelGGL(k_graph_fill<true>, dim3(nblk(nn, 4)), B256, 0, s, d_pos, N, nn, rc2, eng->max_neigh, d_cand, w.row_ptr, w.esrc, w.edst, w.evec, g_lo, g_hi);
    else hipLaunchKernelGGL(k_graph_fill<false>, dim3(nblk(nn, 4)), B256, 0, s, d_pos, N, nn, rc2, eng->max_neigh, d_cand, w.row_ptr, w.esrc, w.edst, w.evec, g_lo, g_hi);
    HIPCHK(eng, hipMemsetAsync(w.out_cur, 0, (nn + 1) * sizeof(int), s));
    if (ne > 0) hipLaunchKernelGGL(k_out_count, dim3(nblk(ne, 256)), B256, 0, s, w.esrc, ne, w.out_cur);
    hipLaunchKernelGGL(k_scan, dim3(1), dim3(1024), 0, s, w.out_cur, nn, w.out_ptr, w.stats + 2);
    HIPCHK(eng, hipMemsetAsync(w.out_cur, 0, (nn + 1) * sizeof(int), s));
    if (ne > 0) {
      hipLaunchKernelGGL(k_out_fill, dim3(nblk(ne, 256)), B256, 0, s, w.esrc, ne, w.out_ptr, w.out_cur, w.out_edge);
      hipLaunchKernelGGL(k_out_sort, dim3(nblk(nn, 4)), B256, 0, s, w.out_ptr, nn, w.out_edge);
      hipLaunchKernelGGL(k_edge_geom, dim3(nblk(ne, 256)), B256, 0, s, w.evec, ne, eng->cutoff, w.frame);
      hipLaunchKernelGGL(k_edge_z, dim3(nblk(ne, 256)), B256, 0, s, w.esrc, w.edst, eng->d_z, N, w.ez, ne);
    }
    HIPCHK(eng, hipGetLastError());
    DBG("row_ptr", w.row_ptr, nn + 1); DBG("src", w.esrc, ne); DBG("dst", w.edst, ne); DBG("out_ptr", w.out_ptr, nn + 1); DBG("out_edge", w.out_edge, ne);
    DBG("evec", w.evec, ne * 4); DBG("frame", w.frame, ne * FRAME);
    if (ne > 0) {
      CHK(radial_fwd_head(eng, w, eng->rdeg, NL, ne));
      // (debug) the fc3 A operand exactly as the GEMM reads it: float32 quad-row blocks, odd rows negated -- tests/test_gpu_mfma_model.py holds the
      // GEMM's output against the bit-exact model of the matrix core on exactly these bits
      if (eng->pl && eng->fwd_fmt == 3) DBG("a2q.deg", reinterpret_cast<const float*>(w.a2pl), (ne + 3) / 4 * 4 * RH);
      CHK(radial_fwd_fc3(eng, w, eng->rdeg, ne, w.rad_deg));
    }
    // x0 = node init + sum over incoming edges (one kernel, the base added in double); graph-parallel: the bare partial sum goes to G1 and is
    // all-reduced first, the base is added by k_node_init_add behind the exchange point
    if (gp) hipLaunchKernelGGL(k_rotate_back_reduce<3>, dim3(nblk(nn, 4)), B256, 0, s, w.rad_deg, w.frame, w.row_ptr, (const float*)nullptr, w.G1, nn, DEG_RESCALE,
                               (const int*)nullptr, 0, (const float*)nullptr, (const double*)nullptr);
    else hipLaunchKernelGGL(k_rotate_back_reduce<3>, dim3(nblk(nn, 4)), B256, 0, s, w.rad_deg, w.frame, w.row_ptr, (const float*)nullptr, w.xs[0], nn, DEG_RESCALE,
                            (const int*)eng->d_z, N, eng->emb_sphere, (const double*)eng->d_sysemb);
    HIPCHK(eng, hipGetLastError());
    if (!gp) { DBG("rad.deg", w.rad_deg, ne * 3 * C); DBG("x0", w.xs[0], nn * ROW); DBG("h1pre.deg", w.h1pre[NL], ne * RH); DBG("h2pre.deg", w.h2pre[NL], ne * RH); }
    return UMX_OK;
  });
  if (gp) {
    P.sync(w.G1, (size_t)nn * ROW);
    P.stream([=, &w]() -> int {
      hipLaunchKernelGGL(k_node_init_add, dim3(nblk(nn * ROW, 256)), B256, 0, eng->stream, eng->d_z, N, nn, eng->emb_sphere, eng->d_sysemb, w.G1, w.xs[0]);
      HIPCHK(eng, hipGetLastError());
      return UMX_OK;
    });
  }

  for (int i = 0; i < NL; ++i) {
    const LayerW* Lp = &eng->lw[i];
    float* xin = w.xs[2 * i];
    float* xmid = w.xs[2 * i + 1];
    float* xout = w.xs[2 * i + 2];
    if (ne > 0 && pl) {
      P.stream([=, &w]() -> int {
        hipStream_t s = eng->stream;
        hipLaunchKernelGGL(k_norm_fwd, dim3(nblk(nn, 4)), B256, 0, s, xin, Lp->n1w, Lp->n1b, eng->d_sysemb, w.xn[i], nn);
        return radial_fwd_head(eng, w, Lp->rad, i, ne);
      });
      P.matrix([=, &w]() -> int {
        if (eng->fwd_fmt == 3) DBG("a2q." + std::to_string(i), reinterpret_cast<const float*>(w.a2pl), (ne + 3) / 4 * 4 * RH);
        return radial_fwd_fc3(eng, w, Lp->rad, ne, w.rad[i]);
      });
      P.stream([=, &w]() -> int {
        hipStream_t s = eng->stream;
        if (eng->fwd_fmt == 1) hipLaunchKernelGGL(k_gather_rotate_mod_q3<1>, dim3(vgrid(eng, (nblk(ne, 4) + 7) / 8 * 8)), B256, 0, s, w.xn[i], w.esrc, w.edst, w.frame, w.rad[i], w.y1pl, ne, eng->odd_sign);
        else hipLaunchKernelGGL(k_gather_rotate_mod_q3<3>, dim3(vgrid(eng, (nblk(ne, 4) + 7) / 8 * 8)), B256, 0, s, w.xn[i], w.esrc, w.edst, w.frame, w.rad[i], w.y1pl, ne, eng->odd_sign);
        HIPCHK(eng, hipGetLastError());
        return UMX_OK;
      });
      // SO(2) conv 1 on the pre-modulated planes -> hg = [gate | hpre]
      P.matrix([=, &w]() -> int {
        if (eng->fwd_fmt == 3) DBG("y1q." + std::to_string(i), reinterpret_cast<const float*>(w.y1pl), (ne + 3) / 4 * 4 * XROT);     // (debug) conv-1's A operand as the GEMMs read it
        CHK(gemm_pl(eng, 0, 3, w.y1pl, XROT, 0, 0, Lp->c1m0, 0, Lp->c1m0b, w.hg[i], HG, 0, 0, ne, 640, 768, 1.0f));
        CHK(gemm_pl(eng, 1, 3, w.y1pl, XROT, 768, 1280, Lp->c1m1, 256, nullptr, w.hg[i], HG, 640, 896, ne, 256, 512, 1.0f));
        return gemm_pl(eng, 1, 3, w.y1pl, XROT, 1792, 2048, Lp->c1m2, 128, nullptr, w.hg[i], HG, 1152, 1280, ne, 128, 256, 1.0f);
      });
      P.stream([=, &w]() -> int {
        hipStream_t s = eng->stream;
        if (eng->fwd_fmt == 1) hipLaunchKernelGGL(k_gate_edge_fwd_q3<1>, dim3(vgrid(eng, nblk(ne, 8))), B256, 0, s, w.hg[i], w.hidpl, ne, eng->odd_sign);
        else hipLaunchKernelGGL(k_gate_edge_fwd_q3<3>, dim3(vgrid(eng, nblk(ne, 8))), B256, 0, s, w.hg[i], w.hidpl, ne, eng->odd_sign);
        HIPCHK(eng, hipGetLastError());
        return UMX_OK;
      });
      P.matrix([=, &w]() -> int {
        if (eng->fwd_fmt == 3) DBG("hidq." + std::to_string(i), reinterpret_cast<const float*>(w.hidpl), (ne + 3) / 4 * 4 * ROW);      // (debug) conv-2's A operand
        CHK(gemm_pl(eng, 0, 3, w.hidpl, ROW, 0, 0, Lp->c2m0, 0, Lp->c2m0b, w.msg[i], ROW, 0, 0, ne, 384, 384, 1.0f));
        CHK(gemm_pl(eng, 1, 3, w.hidpl, ROW, 384, 640, Lp->c2m1, 256, nullptr, w.msg[i], ROW, 384, 640, ne, 256, 256, 1.0f));
        return gemm_pl(eng, 1, 3, w.hidpl, ROW, 896, 1024, Lp->c2m2, 128, nullptr, w.msg[i], ROW, 896, 1024, ne, 128, 128, 1.0f);
      });
    } else {
      P.stream([=, &w]() -> int {
        hipStream_t s = eng->stream;
        const LayerW& L = *Lp;
        hipLaunchKernelGGL(k_norm_fwd, dim3(nblk(nn, 4)), B256, 0, s, xin, L.n1w, L.n1b, eng->d_sysemb, w.xn[i], nn);
        if (ne > 0) {
          hipLaunchKernelGGL(k_gather_rotate, dim3(nblk(ne, 4)), B256, 0, s, w.xn[i], w.esrc, w.edst, w.frame, w.xrot, ne);
          CHK(radial_fwd(eng, w, L.rad, i, ne, w.rad[i]));
          // SO(2) conv 1 (radially modulated) -> hg = [gate | hpre]
          {
            GemmP p = gp_zero();
            p.A = w.xrot; p.lda = XROT; p.R = w.rad[i]; p.ldr = RAD; p.B = L.c1m0; p.ldb = 3 * 2 * C; p.bias = L.c1m0b;
            p.Cp = w.hg[i]; p.ldc = HG; p.M = (int)ne; p.N = 2 * H + 3 * H; p.K = 3 * 2 * C;
            CHK(launch_gemm(eng, p, A_MODUL, 0, E_BIAS));
          }
          CHK(gemm_cplx(eng, w.xrot, XROT, 768, 1280, w.rad[i], RAD, 768, L.c1m1, 512, 256, w.hg[i], HG, 640, 896, ne, 256, 512, 1.0f));
          CHK(gemm_cplx(eng, w.xrot, XROT, 1792, 2048, w.rad[i], RAD, 1280, L.c1m2, 256, 128, w.hg[i], HG, 1152, 1280, ne, 128, 256, 1.0f));
          hipLaunchKernelGGL(k_gate_edge_fwd, dim3(nblk(ne * (H / 4), 256)), B256, 0, s, w.hg[i], w.hid, ne);
          // SO(2) conv 2 -> msg
          CHK(gemm_plain(eng, w.hid, ROW, 0, L.c2m0, 3 * H, L.c2m0b, w.msg[i], ROW, 0, ne, 3 * C, 3 * H));
          CHK(gemm_cplx(eng, w.hid, ROW, 384, 640, nullptr, 0, 0, L.c2m1, 256, 256, w.msg[i], ROW, 384, 640, ne, 256, 256, 1.0f));
          CHK(gemm_cplx(eng, w.hid, ROW, 896, 1024, nullptr, 0, 0, L.c2m2, 128, 128, w.msg[i], ROW, 896, 1024, ne, 128, 128, 1.0f));
        }
        HIPCHK(eng, hipGetLastError());
        return UMX_OK;
      });
    }
    if (gp) {      // partial aggregate of this rank's edges -> xn2 (free until the norm below), all-reduce, xmid = xin + sum
      P.stream([=, &w]() -> int {
        hipLaunchKernelGGL(k_rotate_back_reduce<9>, dim3(nblk(nn, 4)), B256, 0, eng->stream, w.msg[i], w.frame, w.row_ptr, (const float*)nullptr, w.xn2, nn, 1.0f,
                           (const int*)nullptr, 0, (const float*)nullptr, (const double*)nullptr);
        HIPCHK(eng, hipGetLastError());
        return UMX_OK;
      });
      P.sync(w.xn2, (size_t)nn * ROW);
    }
    P.stream([=, &w]() -> int {
      hipStream_t s = eng->stream;
      const LayerW& L = *Lp;
      const std::string t = "." + std::to_string(i);
      if (gp) hipLaunchKernelGGL(k_add_rows, dim3(nblk(nn * ROW / 4, 256)), B256, 0, s, xmid, xin, w.xn2, nn * ROW / 4);
      else hipLaunchKernelGGL(k_rotate_back_reduce<9>, dim3(vgrid(eng, nblk(nn, 4))), B256, 0, s, w.msg[i], w.frame, w.row_ptr, xin, xmid, nn, 1.0f,
                              (const int*)nullptr, 0, (const float*)nullptr, (const double*)nullptr);
      HIPCHK(eng, hipGetLastError());
      DBG("xn" + t, w.xn[i], nn * ROW); DBG("rad" + t, w.rad[i], ne * RAD); DBG("h1pre" + t, w.h1pre[i], ne * RH); DBG("h2pre" + t, w.h2pre[i], ne * RH);
      if (!eng->pl) { DBG("xrot" + t, w.xrot, ne * XROT); DBG("hid" + t, w.hid, ne * ROW); }
      DBG("hg" + t, w.hg[i], ne * HG); DBG("msg" + t, w.msg[i], ne * ROW); DBG("xmid" + t, xmid, nn * ROW);
      // K8 atom-wise
      hipLaunchKernelGGL(k_norm_fwd, dim3(nblk(nn, 4)), B256, 0, s, xmid, L.n2w, L.n2b, (const double*)nullptr, w.xn2, nn);
      if (eng->ff_grid) {
        // GridAtomwise: to-grid -> Linear, SiLU, Linear, SiLU, Linear over the channels of every grid point -> from-grid (+ residual).
        // The hidden pre-activations stay resident for the reverse pass; the SiLUs are applied while the next GEMM stages its A operand.
        const int G = eng->grid_G;
        const long ng = nn * G;
        hipLaunchKernelGGL(k_grid_expand, dim3(nblk(nn, 4)), B256, 0, s, w.xn2, eng->to_grid, G, w.gridA, nn);
        CHK(gemm_grid(eng, w.gridA, C, 0, L.g1w, C, L.g1b, w.ffg1[i], H, 0, ng, H, C));
        CHK(gemm_grid(eng, w.ffg1[i], H, 0, L.g2w, H, L.g2b, w.ffg2[i], H, 0, ng, H, H, A_SILU));
        CHK(gemm_grid(eng, w.ffg2[i], H, 0, L.g3w, H, L.g3b, w.gridA, C, 0, ng, C, H, A_SILU));
        hipLaunchKernelGGL(k_grid_contract, dim3(nblk(nn, 4)), B256, 0, s, w.gridA, eng->from_grid, G, xmid, xout, nn);
        HIPCHK(eng, hipGetLastError());
        DBG("xn2" + t, w.xn2, nn * ROW); DBG("ffg1" + t, w.ffg1[i], ng * H); DBG("ffg2" + t, w.ffg2[i], ng * H); DBG("x" + t, xout, nn * ROW);
        return UMX_OK;
      }
      CHK(gemm_node(eng, w.xn2, ROW, 0, L.smlp, C, L.smlpb, w.gspre[i], 2 * H, 0, nn, 2 * H, C));
      CHK(so3_linear(eng, w.xn2, L.l1w, L.l1b, w.ffh[i], nn, nullptr));
      hipLaunchKernelGGL(k_gate_node_fwd, dim3(nblk(nn * H, 256)), B256, 0, s, w.ffh[i], w.gspre[i], w.ffhg, nn);
      CHK(so3_linear(eng, w.ffhg, L.l2w, L.l2b, xout, nn, xmid));
      HIPCHK(eng, hipGetLastError());
      DBG("xn2" + t, w.xn2, nn * ROW); DBG("gspre" + t, w.gspre[i], nn * 2 * H); DBG("ffh" + t, w.ffh[i], nn * ROW); DBG("x" + t, xout, nn * ROW);
      return UMX_OK;
    });
  }
  // K9 readout (+ the node-level head of the reverse pass)
  float* xlast = w.xs[2 * NL];
  P.stream([=, &w]() -> int {
    hipStream_t s = eng->stream;
    hipLaunchKernelGGL(k_norm_fwd, dim3(nblk(nn, 4)), B256, 0, s, xlast, eng->normw, eng->normb, (const double*)nullptr, w.xf, nn);
    CHK(gemm_node(eng, w.xf, ROW, 0, eng->e0, C, eng->e0b, w.pre1, H, 0, nn, H, C));
    CHK(gemm_node(eng, w.pre1, H, 0, eng->e2, H, eng->e2b, w.pre2, H, 0, nn, H, H, A_SILU));
    hipLaunchKernelGGL(k_energy_node, dim3(nblk(nn, 4)), B256, 0, s, w.pre2, eng->e4, eng->e4b, w.enode, nn);
    hipLaunchKernelGGL(k_energy, dim3((unsigned)nimg), B256, 0, s, w.enode, N, eng->rmsd, eng->refsum, d_energy, eng->d_flags);
    HIPCHK(eng, hipGetLastError());
    DBG("e_node", w.enode, nn); DBG("pre1", w.pre1, nn * H); DBG("pre2", w.pre2, nn * H);
    if (!d_forces) return UMX_OK;
    // ---------------- K10: analytic reverse pass ----------------
    if (ne > 0) {
      HIPCHK(eng, hipMemsetAsync(w.dedd, 0, ne * sizeof(float), s));
      HIPCHK(eng, hipMemsetAsync(w.dedd_rad, 0, ne * sizeof(float), s));
      HIPCHK(eng, hipMemsetAsync(w.tau, 0, ne * 4 * sizeof(float), s));
      HIPCHK(eng, hipMemsetAsync(w.tau2, 0, ne * 4 * sizeof(float), s));
    }
    hipLaunchKernelGGL(k_silu_bwd, dim3(nblk(nn * H, 256)), B256, 0, s, eng->e4, 0L, w.pre2, w.n128a, nn, H);
    CHK(gemm_node(eng, w.n128a, H, 0, eng->e2T, H, nullptr, w.n128b, H, 0, nn, H, H));
    hipLaunchKernelGGL(k_silu_bwd, dim3(nblk(nn * H, 256)), B256, 0, s, w.n128b, (long)H, w.pre1, w.n128a, nn, H);
    HIPCHK(eng, hipMemsetAsync(w.G1, 0, nn * ROW * sizeof(float), s));
    CHK(gemm_node(eng, w.n128a, H, 0, eng->e0T, H, nullptr, w.G1, ROW, 0, nn, C, H));
    hipLaunchKernelGGL(k_norm_bwd, dim3(nblk(nn, 4)), B256, 0, s, w.G1, xlast, eng->normw, (const float*)nullptr, w.G0, nn);
    HIPCHK(eng, hipGetLastError());
    DBG("g_xfinal", w.G0, nn * ROW);
    return UMX_OK;
  });
  if (!d_forces) return;

  for (int i = NL - 1; i >= 0; --i) {
    const LayerW* Lp = &eng->lw[i];
    float* xin = w.xs[2 * i];
    float* xmid = w.xs[2 * i + 1];
    // atom-wise backward: G0 = dE/dx_out  (+ the first edge kernel of the layer)
    P.stream([=, &w]() -> int {
      hipStream_t s = eng->stream;
      const LayerW& L = *Lp;
      const std::string t = "." + std::to_string(i);
      if (eng->ff_grid) {
        // reverse of GridAtomwise: from-grid^T -> W3^T, SiLU', W2^T, SiLU', W1^T -> to-grid^T
        const int G = eng->grid_G;
        const long ng = nn * G;
        hipLaunchKernelGGL(k_grid_expand, dim3(nblk(nn, 4)), B256, 0, s, w.G0, eng->from_grid, G, w.gridA, nn);
        CHK(gemm_grid(eng, w.gridA, C, 0, L.g3T, C, nullptr, w.gridB, H, 0, ng, H, C));
        hipLaunchKernelGGL(k_silu_bwd, dim3(nblk(ng * H, 256)), B256, 0, s, w.gridB, (long)H, w.ffg2[i], w.gridA, ng, H);
        CHK(gemm_grid(eng, w.gridA, H, 0, L.g2T, H, nullptr, w.gridB, H, 0, ng, H, H));
        hipLaunchKernelGGL(k_silu_bwd, dim3(nblk(ng * H, 256)), B256, 0, s, w.gridB, (long)H, w.ffg1[i], w.gridA, ng, H);
        CHK(gemm_grid(eng, w.gridA, H, 0, L.g1T, H, nullptr, w.gridB, C, 0, ng, C, H));
        hipLaunchKernelGGL(k_grid_contract, dim3(nblk(nn, 4)), B256, 0, s, w.gridB, eng->to_grid, G, (const float*)nullptr, w.G1, nn);     // G1 = g_xn2
      } else {
      CHK(so3_linear(eng, w.G0, L.l2T, nullptr, w.G1, nn, nullptr));                         // G1 = g_ffhg
      hipLaunchKernelGGL(k_gate_node_bwd, dim3(nblk(nn * H, 256)), B256, 0, s, w.G1, w.ffh[i], w.gspre[i], w.G2, w.ggs, nn);
      CHK(so3_linear(eng, w.G2, L.l1T, nullptr, w.G1, nn, nullptr));                         // G1 = g_xn2
      CHK(gemm_node(eng, w.ggs, 2 * H, 0, L.smlpT, 2 * H, nullptr, w.G1, ROW, 0, nn, C, 2 * H, A_PLAIN, 1, 0, 0, w.G1, ROW, 0, 0));
      }
      hipLaunchKernelGGL(k_norm_bwd, dim3(nblk(nn, 4)), B256, 0, s, w.G1, xmid, L.n2w, w.G0, w.G2, nn);   // G2 = g_xmid
      HIPCHK(eng, hipGetLastError());
      DBG("g_xmid" + t, w.G2, nn * ROW);
      if (ne > 0 && eng->pl)
      {
        if (eng->rev_qf) hipLaunchKernelGGL(k_rotate_back_bwd_q3<3>, dim3(vgrid(eng, (nblk(ne, 4) + 7) / 8 * 8)), B256, 0, s, w.G2, w.msg[i], w.frame, w.edst, w.gmsgpl, w.dedd, w.tau, ne, eng->odd_sign);
        else hipLaunchKernelGGL(k_rotate_back_bwd_pl<2>, dim3(vgrid(eng, (nblk(ne, 4) + 7) / 8 * 8)), B256, 0, s, w.G2, w.msg[i], w.frame, w.edst, w.gmsgpl, w.dedd, w.tau, ne, eng->odd_sign);
        // (debug) conv-2^T's A operand as the GEMMs read it: float32 quad-row blocks (bf16x3) or two PL planes (split-bf16); odd rows negated
        if (eng->rev_qf) DBG("gmsgq" + t, reinterpret_cast<const float*>(w.gmsgpl), (ne + 3) / 4 * 4 * ROW);
        else DBG("gmsgpl" + t, w.gmsgpl, ne * ROW * 2);
      }
      HIPCHK(eng, hipGetLastError());
      return UMX_OK;
    });
    if (ne > 0 && pl) {
      P.matrix([=, &w]() -> int {
        CHK(gemm_pl(eng, 0, 2, w.gmsgpl, ROW, 0, 0, Lp->c2m0T, 0, nullptr, w.hid, ROW, 0, 0, ne, 384, 384, 1.0f));
        CHK(gemm_pl(eng, 1, 2, w.gmsgpl, ROW, 384, 640, Lp->c2m1T, 256, nullptr, w.hid, ROW, 384, 640, ne, 256, 256, -1.0f));
        return gemm_pl(eng, 1, 2, w.gmsgpl, ROW, 896, 1024, Lp->c2m2T, 128, nullptr, w.hid, ROW, 896, 1024, ne, 128, 128, -1.0f);
      });
      P.stream([=, &w]() -> int {
        hipStream_t s = eng->stream;
        DBG("g_hid." + std::to_string(i), w.hid, ne * ROW);
        if (eng->rev_qf) hipLaunchKernelGGL(k_gate_edge_bwd_q3<3>, dim3(vgrid(eng, nblk(ne, 8))), B256, 0, s, w.hid, w.hg[i], w.ghgpl, ne, eng->odd_sign);
        else hipLaunchKernelGGL(k_gate_edge_bwd_pl<2>, dim3(vgrid(eng, nblk(ne * (H / 4), 256))), B256, 0, s, w.hid, w.hg[i], w.ghgpl, ne, eng->odd_sign);
        HIPCHK(eng, hipGetLastError());
        // (debug) conv-1^T's A operand, in the format of gmsgq / gmsgpl
        if (eng->rev_qf) DBG("ghgq." + std::to_string(i), reinterpret_cast<const float*>(w.ghgpl), (ne + 3) / 4 * 4 * HG);
        else DBG("ghgpl." + std::to_string(i), w.ghgpl, ne * HG * 2);
        return UMX_OK;
      });
      P.matrix([=, &w]() -> int {
        CHK(gemm_pl(eng, 0, 2, w.ghgpl, HG, 0, 0, Lp->c1m0T, 0, nullptr, w.gy1, XROT, 0, 0, ne, 768, 640, 1.0f));
        CHK(gemm_pl(eng, 1, 2, w.ghgpl, HG, 640, 896, Lp->c1m1T, 512, nullptr, w.gy1, XROT, 768, 1280, ne, 512, 256, -1.0f));
        return gemm_pl(eng, 1, 2, w.ghgpl, HG, 1152, 1280, Lp->c1m2T, 256, nullptr, w.gy1, XROT, 1792, 2048, ne, 256, 128, -1.0f);
      });
      // (a matrix-token segment although it is HBM-bound: at 240 VGPRs its waves cannot share a SIMD with a GEMM wave, so beside
      //  the other lane's GEMM it would only take CUs away from it; the other lane's throttled stream kernels do fit beside it)
      P.matrix([=, &w]() -> int {
        hipStream_t s = eng->stream;
        const std::string t = "." + std::to_string(i);
        DBG("g_y1" + t, w.gy1, ne * XROT);        // (debug) conv-1^T's output
        // one node-centric kernel: modulation backward + rotate-back + segmented sum (g_xrot stays in registers); g_rad as float32 rows
        // (sign-alternating; split by the fc3^T GEMM in registers) in the bf16x3 mode, as two PL bf16 planes in the 16-bit-reverse modes
        if (eng->rev_qf) hipLaunchKernelGGL(k_modrot_bwd_pl<0>, dim3((unsigned)nn), B256, 0, s, w.gy1, w.xn[i], w.frame, w.rad[i], w.row_ptr, w.out_ptr, w.out_edge,
                                            w.gradpl, w.tau, w.tau2, w.G1, nn, eng->odd_sign);
        else hipLaunchKernelGGL(k_modrot_bwd_pl<2>, dim3((unsigned)nn), B256, 0, s, w.gy1, w.xn[i], w.frame, w.rad[i], w.row_ptr, w.out_ptr, w.out_edge,
                                w.gradpl, w.tau, w.tau2, w.G1, nn, eng->odd_sign);
        HIPCHK(eng, hipGetLastError());
        // (debug) fc3^T's A operand: float32 rows (bf16x3) or two PL planes (split-bf16); odd rows negated
        if (eng->rev_qf) DBG("gradq" + t, reinterpret_cast<const float*>(w.gradpl), ne * RAD);
        else DBG("gradpl" + t, w.gradpl, ne * RAD * 2);
        return UMX_OK;
      });
      P.matrix([=, &w]() -> int { return radial_bwd_fc3(eng, w, Lp->rad, ne, nullptr, w.gradpl, eng->rev_qf); });
      P.stream([=, &w]() -> int { return radial_bwd_tail(eng, w, Lp->rad, i, ne); });     // feeds only the scalar dE/dd (own accumulator dedd_rad)
    } else if (ne > 0) {
      P.stream([=, &w]() -> int {
        hipStream_t s = eng->stream;
        const LayerW& L = *Lp;
        const std::string t = "." + std::to_string(i);
        hipLaunchKernelGGL(k_rotate_back_bwd<9>, dim3(nblk(ne, 4)), B256, 0, s, w.G2, w.msg[i], w.frame, w.edst, w.gmsg, w.dedd, w.tau, ne, 1.0f);
        CHK(gemm_plain(eng, w.gmsg, ROW, 0, L.c2m0T, 3 * C, nullptr, w.hid, ROW, 0, ne, 3 * H, 3 * C));
        CHK(gemm_cplx(eng, w.gmsg, ROW, 384, 640, nullptr, 0, 0, L.c2m1T, 256, 256, w.hid, ROW, 384, 640, ne, 256, 256, -1.0f));
        CHK(gemm_cplx(eng, w.gmsg, ROW, 896, 1024, nullptr, 0, 0, L.c2m2T, 128, 128, w.hid, ROW, 896, 1024, ne, 128, 128, -1.0f));
        DBG("g_msg" + t, w.gmsg, ne * ROW); DBG("g_hid" + t, w.hid, ne * ROW);
        hipLaunchKernelGGL(k_gate_edge_bwd, dim3(nblk(ne * H, 256)), B256, 0, s, w.hid, w.hg[i], w.ghg, ne);
        CHK(gemm_plain(eng, w.ghg, HG, 0, L.c1m0T, 640, nullptr, w.gy1, XROT, 0, ne, 768, 640));
        CHK(gemm_cplx(eng, w.ghg, HG, 640, 896, nullptr, 0, 0, L.c1m1T, 256, 512, w.gy1, XROT, 768, 1280, ne, 512, 256, -1.0f));
        CHK(gemm_cplx(eng, w.ghg, HG, 1152, 1280, nullptr, 0, 0, L.c1m2T, 128, 256, w.gy1, XROT, 1792, 2048, ne, 256, 128, -1.0f));
        DBG("g_hg" + t, w.ghg, ne * HG); DBG("g_y1" + t, w.gy1, ne * XROT);      // (k_modulate_bwd below turns g_y1 into g_xrot in place)
        if (!eng->dbg_on) {
          // round 4: the fp32 mode takes the node-centric fused kernel of the split path too (P = 0: g_rad as float32 rows) instead of
          // k_gather_rotate + k_modulate_bwd + k_gather_rotate_bwd -- the rotated message and g_xrot never touch HBM (-27 KB per edge and
          // layer).  With debug captures on the unfused kernels run: they expose xrot / g_xrot to the stage-by-stage test.
          hipLaunchKernelGGL(k_modrot_bwd_pl<0>, dim3((unsigned)nn), B256, 0, s, w.gy1, w.xn[i], w.frame, w.rad[i], w.row_ptr, w.out_ptr, w.out_edge,
                             reinterpret_cast<unsigned short*>(w.grad), w.tau, w.tau2, w.G1, nn, 1.0f);
          HIPCHK(eng, hipGetLastError());
        } else {
          hipLaunchKernelGGL(k_gather_rotate, dim3(nblk(ne, 4)), B256, 0, s, w.xn[i], w.esrc, w.edst, w.frame, w.xrot, ne);
          hipLaunchKernelGGL(k_modulate_bwd, dim3(nblk(ne, 4)), B256, 0, s, w.gy1, w.xrot, w.rad[i], w.grad, w.tau, ne);
          DBG("g_xrot" + t, w.gy1, ne * XROT); DBG("g_rad" + t, w.grad, ne * RAD);
        }
        return radial_bwd(eng, w, L.rad, i, ne, w.grad);
      });
    }
    if (gp) {
      // g_xn: every rank holds the contributions of its own edges only.  A rank WITHOUT edges (fewer atoms than ranks, or only isolated
      // targets) has run no edge kernel: G1 still holds g_xn2 of the atom-wise backward and must not enter the sum
      if (ne == 0) P.stream([=, &w]() -> int { HIPCHK(eng, hipMemsetAsync(w.G1, 0, (size_t)nn * ROW * sizeof(float), eng->stream)); return UMX_OK; });
      else if (!fused_rev)                     // unfused reverse: the partial g_xn of this rank's edges has to exist BEFORE the exchange
        P.stream([=, &w]() -> int {
          hipLaunchKernelGGL(k_gather_rotate_bwd, dim3(nblk(nn, 4)), B256, 0, eng->stream, w.gy1, w.frame, w.row_ptr, w.out_ptr, w.out_edge, w.G1, nn);
          HIPCHK(eng, hipGetLastError());
          return UMX_OK;
        });
      P.sync(w.G1, (size_t)nn * ROW);
    }
    P.stream([=, &w]() -> int {
      hipStream_t s = eng->stream;
      const std::string t = "." + std::to_string(i);
      if (!(ne > 0 && fused_rev) && !gp)
        hipLaunchKernelGGL(k_gather_rotate_bwd, dim3(nblk(nn, 4)), B256, 0, s, w.gy1, w.frame, w.row_ptr, w.out_ptr, w.out_edge, w.G1, nn);   // G1 = g_xn
      hipLaunchKernelGGL(k_norm_bwd, dim3(nblk(nn, 4)), B256, 0, s, w.G1, xin, Lp->n1w, w.G2, w.G0, nn);                      // G0 = g_xin
      HIPCHK(eng, hipGetLastError());
      DBG("g_xn" + t, w.G1, nn * ROW); DBG("g_xin" + t, w.G0, nn * ROW);
      return UMX_OK;
    });
  }
  P.stream([=, &w]() -> int {
    hipStream_t s = eng->stream;
    if (ne > 0) {
      // split path: the gradient of the edge-degree radial output goes straight into the PL planes of the fc3^T GEMM (gmsgpl is free here)
      const bool dpl = eng->pl && eng->planes.count(eng->rdeg.w3T) != 0;
      if (dpl && eng->rev_planes == 3) hipLaunchKernelGGL((k_rotate_back_bwd<3, 3>), dim3(nblk(ne, 4)), B256, 0, s, w.G0, w.rad_deg, w.frame, w.edst,
                                                          reinterpret_cast<float*>(w.gmsgpl), w.dedd, w.tau, ne, DEG_RESCALE, eng->odd_sign);
      else if (dpl) hipLaunchKernelGGL((k_rotate_back_bwd<3, 2>), dim3(nblk(ne, 4)), B256, 0, s, w.G0, w.rad_deg, w.frame, w.edst,
                                       reinterpret_cast<float*>(w.gmsgpl), w.dedd, w.tau, ne, DEG_RESCALE, eng->odd_sign);
      if (dpl) DBG("gradpl.deg", w.gmsgpl, ne * 3 * C * eng->rev_planes);      // (debug) the PL planes of the edge-degree fc3^T operand
      else hipLaunchKernelGGL(k_rotate_back_bwd<3>, dim3(nblk(ne, 4)), B256, 0, s, w.G0, w.rad_deg, w.frame, w.edst, w.gmsg, w.dedd, w.tau, ne,
                              DEG_RESCALE);
      CHK(radial_bwd(eng, w, eng->rdeg, NL, ne, w.gmsg, dpl ? w.gmsgpl : nullptr));
      if (fused_rev) hipLaunchKernelGGL(k_add4, dim3(nblk(ne, 256)), B256, 0, s, w.tau, w.tau2, ne);
      hipLaunchKernelGGL(k_force_edge, dim3(nblk(ne, 256)), B256, 0, s, w.dedd, w.dedd_rad, w.tau, w.frame, w.evec, w.gvec, ne);
    }
    hipLaunchKernelGGL(k_force_node, dim3(nblk(nn, 4)), B256, 0, s, w.gvec, w.row_ptr, w.out_ptr, w.out_edge, (float)eng->rmsd, d_forces, nn);
    HIPCHK(eng, hipGetLastError());
    DBG("dedd", w.dedd, ne); DBG("tau", w.tau, ne * 4); DBG("gvec", w.gvec, ne * 4);
    return UMX_OK;
  });
  if (gp) P.sync(d_forces, (size_t)nn * 3);           // forces: sum of the ranks' edge contributions
}

// Issue one plan on the stream eng->stream points at.
int run_plan(umx_engine* eng, Plan& P) {
  for (auto& sg : P.segs) CHK(sg.fn());
  return UMX_OK;
}

// Issue two plans on two streams, alternating between the lanes after every matrix segment and passing the matrix token:
// lane L's matrix segment waits (on the device) for the other lane's most recent matrix segment to finish and nothing else,
// so the other lane's stream segments run beside it.  Host-side issue order == token order, which is what makes the
// hipStreamWaitEvent calls see an already-recorded event.
int run_plans_alternating(umx_engine* eng, Plan (&P)[2], hipStream_t (&st)[2], hipEvent_t (&tok)[2]) {
  size_t at[2] = {0, 0};
  bool recorded[2] = {false, false};
  hipStream_t keep = eng->stream;
  int stt = UMX_OK;
  while (stt == UMX_OK && (at[0] < P[0].segs.size() || at[1] < P[1].segs.size())) {
    for (int l = 0; l < 2 && stt == UMX_OK; ++l) {
      eng->stream = st[l];
      // stream segments up to and including the next matrix segment of this lane
      while (at[l] < P[l].segs.size()) {
        Seg& sg = P[l].segs[at[l]++];
        if (sg.matrix && recorded[1 - l]) {
          hipError_t e = hipStreamWaitEvent(st[l], tok[1 - l], 0);
          if (e != hipSuccess) { stt = fail(eng, UMX_ERR_HIP, std::string("token wait: ") + hipGetErrorName(e)); break; }
        }
        stt = sg.fn();
        if (stt != UMX_OK) break;
        if (sg.matrix) {
          hipError_t e = hipEventRecord(tok[l], st[l]);
          if (e != hipSuccess) { stt = fail(eng, UMX_ERR_HIP, std::string("token record: ") + hipGetErrorName(e)); break; }
          recorded[l] = true;
          break;
        }
      }
    }
  }
  eng->stream = keep;
  return stt;
}

// per-image edge totals from the per-node degrees
__global__ void k_image_edges(const int* __restrict__ deg, int natoms, int* __restrict__ out, int* __restrict__ maxdeg) {
  __shared__ int part[256];
  __shared__ int pm[256];
  const int img = blockIdx.x;
  int s = 0, m = 0;
  for (int a = threadIdx.x; a < natoms; a += 256) { const int d = deg[(long)img * natoms + a]; s += d; m = d > m ? d : m; }
  part[threadIdx.x] = s; pm[threadIdx.x] = m;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) { part[threadIdx.x] += part[threadIdx.x + o]; pm[threadIdx.x] = max(pm[threadIdx.x], pm[threadIdx.x + o]); }
    __syncthreads();
  }
  if (threadIdx.x == 0) { out[img] = part[0]; atomicMax(maxdeg, pm[0]); }
}

// ---- weights -----------------------------------------------------------------------------------
std::vector<float> transpose(const float* src, int rows, int cols) {
  std::vector<float> t((size_t)rows * cols);
  for (int r = 0; r < rows; ++r)
    for (int c = 0; c < cols; ++c) t[(size_t)c * rows + r] = src[(size_t)r * cols + c];
  return t;
}

}  // namespace

// ================================================================================================
//                                           C ABI
// ================================================================================================
extern "C" {

int umx_abi_version(void) { return 10; }

#ifndef UMX_SRC_DIGEST
#define UMX_SRC_DIGEST "unknown"
#endif
const char* umx_build_digest(void) { return UMX_SRC_DIGEST; }

const char* umx_last_error(const umx_engine* eng) { return eng ? eng->err.c_str() : g_create_err.c_str(); }

int umx_create(umx_engine** out, int device_ordinal) {
  if (!out) { g_create_err = "umx_create: null out pointer"; return UMX_ERR_ARG; }
  *out = nullptr;
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) { g_create_err = "umx_create: no HIP device visible"; return UMX_ERR_NO_DEVICE; }
  if (device_ordinal < 0 || device_ordinal >= n) { g_create_err = "umx_create: device ordinal out of range"; return UMX_ERR_ARG; }
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, device_ordinal) != hipSuccess) { g_create_err = "umx_create: hipGetDeviceProperties failed"; return UMX_ERR_HIP; }
  if (std::string(prop.gcnArchName).rfind("gfx950", 0) != 0) {
    g_create_err = std::string("umx_create: device is ") + prop.gcnArchName + ", this library is built for gfx950 only";
    return UMX_ERR_NO_DEVICE;
  }
  umx_engine* e = new umx_engine();
  e->dev = device_ordinal;
  if (const char* ev = std::getenv("UMX_STREAMS")) e->n_lanes = std::atoi(ev) >= 2 ? 2 : (std::atoi(ev) == 1 ? 1 : 0);
  if (const char* ev = std::getenv("UMX_LANES_AUTO_EDGES")) e->lanes_auto_edges = std::max(0L, std::atol(ev));
  if (const char* ev = std::getenv("UMX_FORCE_PARTS")) e->force_parts = std::max(0, std::min(16, std::atoi(ev)));
  if (const char* ev = std::getenv("UMX_WS_GB")) e->ws_cap_default = (size_t)std::max(0L, std::atol(ev)) << 30;
  if (const char* ev = std::getenv("UMX_WS_EAGER")) e->ws_eager = std::atoi(ev) != 0;
  if (const char* ev = std::getenv("UMX_WS_SOFT_EDGES")) e->ws_soft_edges = std::max(1L, std::atol(ev));
  if (const char* ev = std::getenv("UMX_NODE_F64")) e->node_f64_on = std::atoi(ev) != 0;
  if (const char* ev = std::getenv("UMX_GRID_F64")) e->grid_f64 = std::atoi(ev) != 0;
  if (const char* ev = std::getenv("UMX_ALT_ROWS")) e->odd_sign = std::atoi(ev) != 0 ? -1.0f : 1.0f;
  if (const char* ev = std::getenv("UMX_LOW_SEP")) e->low_sep = std::atoi(ev);
  if (const char* ev = std::getenv("UMX_ALIGN_PLANES")) e->align = std::atoi(ev);
  // stream2 (the second lane) is created with the highest priority (as measured in rounds 3-5; priorities change little on this pool)
  int prio_lo = 0, prio_hi = 0;
  if (hipSetDevice(device_ordinal) != hipSuccess || hipDeviceGetStreamPriorityRange(&prio_lo, &prio_hi) != hipSuccess ||
      hipStreamCreateWithFlags(&e->stream, hipStreamNonBlocking) != hipSuccess ||
      hipStreamCreateWithPriority(&e->stream2, hipStreamNonBlocking, prio_hi) != hipSuccess ||
      hipEventCreateWithFlags(&e->ev_fork, hipEventDisableTiming) != hipSuccess || hipEventCreateWithFlags(&e->ev_join, hipEventDisableTiming) != hipSuccess ||
      hipEventCreateWithFlags(&e->ev_tok[0], hipEventDisableTiming) != hipSuccess || hipEventCreateWithFlags(&e->ev_tok[1], hipEventDisableTiming) != hipSuccess ||
      hipEventCreateWithFlags(&e->ev_done, hipEventDisableTiming) != hipSuccess || hipMalloc(&e->d_flags, 4 * sizeof(int)) != hipSuccess ||
      hipMemset(e->d_flags, 0, 4 * sizeof(int)) != hipSuccess) {
    g_create_err = "umx_create: hipSetDevice/hipStreamCreate failed";
    delete e;
    return UMX_ERR_HIP;
  }
  *out = e;
  return UMX_OK;
}

static void gp_clear(umx_engine* eng);

int umx_destroy(umx_engine* eng) {
  if (!eng) return UMX_OK;
  if (eng->gp_plan) gp_clear(eng);
  (void)hipSetDevice(eng->dev);
  (void)hipStreamSynchronize(eng->stream);
  for (auto& r : eng->prof) { (void)hipEventDestroy(r.a); (void)hipEventDestroy(r.b); }
  void* ptrs[] = {eng->d_w, eng->d_dw, eng->d_bw, eng->d_gmu, eng->d_z, eng->d_sysemb, eng->arena, eng->d_deg_all, eng->d_cand_all, eng->d_img_edges, eng->d_io_pos, eng->d_io_e, eng->d_io_f, eng->d_flags, eng->d_dtab, eng->d_part_deg, eng->d_part_f};
  for (void* p : ptrs) if (p) (void)hipFree(p);
  (void)hipStreamSynchronize(eng->stream2);
  (void)hipEventDestroy(eng->ev_fork); (void)hipEventDestroy(eng->ev_join);
  (void)hipEventDestroy(eng->ev_tok[0]); (void)hipEventDestroy(eng->ev_tok[1]);
  if (eng->ev_done) (void)hipEventDestroy(eng->ev_done);
  (void)hipStreamDestroy(eng->stream2);
  (void)hipStreamDestroy(eng->stream);
  delete eng;
  return UMX_OK;
}

int umx_set_workspace_limit(umx_engine* eng, size_t bytes) {
  if (!eng) return UMX_ERR_ARG;
  eng->ws_limit = bytes;
  return UMX_OK;
}

static int load_weights_impl(umx_engine* eng, const void* blob, size_t nbytes) {
  HIPCHK(eng, hipSetDevice(eng->dev));
  const char* b = static_cast<const char*>(blob);
  if (nbytes < 16 || std::memcmp(b, "UMXW0001", 8) != 0) return fail(eng, UMX_ERR_WEIGHTS, "weight blob: bad magic");
  uint32_t n;
  std::memcpy(&n, b + 8, 4);
  const size_t esz = 96 + 4 + 16 + 8 + 8;
  if (nbytes < 16 + (size_t)n * esz) return fail(eng, UMX_ERR_WEIGHTS, "weight blob: truncated table");
  size_t pos = 16;
  eng->wt.clear();
  size_t max_end = 0;
  for (uint32_t i = 0; i < n; ++i) {
    char name[97]; std::memcpy(name, b + pos, 96); name[96] = 0;
    uint32_t ndim, dims[4]; uint64_t off, nb;
    std::memcpy(&ndim, b + pos + 96, 4); std::memcpy(dims, b + pos + 100, 16);
    std::memcpy(&off, b + pos + 116, 8); std::memcpy(&nb, b + pos + 124, 8);
    if (ndim < 1 || ndim > 4) return fail(eng, UMX_ERR_WEIGHTS, std::string("weight blob: bad ndim for ") + name);
    Tensor t; t.off = off / 4; t.count = nb / 4;
    size_t cnt = 1;
    for (uint32_t d = 0; d < ndim; ++d) { t.shape.push_back((int)dims[d]); cnt *= dims[d]; }
    if (cnt != t.count) return fail(eng, UMX_ERR_WEIGHTS, std::string("weight blob: size mismatch for ") + name);
    eng->wt[name] = t;
    max_end = std::max(max_end, (size_t)(off + nb));
    pos += esz;
  }
  const size_t data0 = (pos + 63) & ~size_t(63);
  if (nbytes < data0 + max_end) return fail(eng, UMX_ERR_WEIGHTS, "weight blob: truncated data");
  eng->h_w.assign(reinterpret_cast<const float*>(b + data0), reinterpret_cast<const float*>(b + data0) + (max_end + 3) / 4);
  for (const auto& kv : eng->wt)            // a non-finite parameter would only show up later as a non-finite energy
    for (size_t i = 0; i < kv.second.count; ++i)
      if (!std::isfinite(eng->h_w[kv.second.off + i])) return fail(eng, UMX_ERR_WEIGHTS, "weight blob: non-finite value in " + kv.first);

  auto need = [&](const std::string& nm, std::vector<int> shape) -> const Tensor* {
    auto it = eng->wt.find(nm);
    if (it == eng->wt.end() || it->second.shape != shape) { eng->err = "weight blob: missing or mis-shaped tensor " + nm; return nullptr; }
    return &it->second;
  };
  // ---- derived weights (host) ----
  std::vector<float> dw;
  auto push = [&](const std::vector<float>& v) -> size_t {
    size_t o = (dw.size() + 63) & ~size_t(63);
    dw.resize(o + v.size());
    std::copy(v.begin(), v.end(), dw.begin() + o);
    return o;
  };
  const float* hw = eng->h_w.data();
  struct RadOff { size_t w1g, w1gT, w2T, w3T, tsd, ttd; };
  std::vector<double> dtab;
  std::map<std::string, RadOff> roff;
  const Tensor* tsrc = need("source_embedding.weight", {NZ, 128});
  const Tensor* ttgt = need("target_embedding.weight", {NZ, 128});
  if (!tsrc || !ttgt) return UMX_ERR_WEIGHTS;
  auto radial_derive = [&](const std::string& pre, int out) -> int {
    const Tensor* w1 = need(pre + ".fc1.weight", {RH, NG + 256});
    const Tensor* b1 = need(pre + ".fc1.bias", {RH});
    const Tensor* w2 = need(pre + ".fc2.weight", {RH, RH});
    const Tensor* w3 = need(pre + ".fc3.weight", {out, RH});
    for (const char* s : {".fc2.bias", ".ln1.weight", ".ln1.bias", ".ln2.weight", ".ln2.bias"})
      if (!need(pre + s, {RH})) return UMX_ERR_WEIGHTS;
    if (!w1 || !b1 || !w2 || !w3 || !need(pre + ".fc3.bias", {out})) return UMX_ERR_WEIGHTS;
    const float* W1 = hw + w1->off;
    std::vector<float> w1g((size_t)RH * NG);
    RadOff o;
    o.tsd = dtab.size(); dtab.resize(dtab.size() + (size_t)NZ * RH);
    o.ttd = dtab.size(); dtab.resize(dtab.size() + (size_t)NZ * RH);
    for (int h = 0; h < RH; ++h)
      for (int k = 0; k < NG; ++k) w1g[(size_t)h * NG + k] = W1[(size_t)h * (NG + 256) + k];
    for (int z = 0; z < NZ; ++z)
      for (int h = 0; h < RH; ++h) {
        double a = 0.0, c = hw[b1->off + h];
        for (int k = 0; k < 128; ++k) {
          a += (double)W1[(size_t)h * (NG + 256) + NG + k] * hw[tsrc->off + (size_t)z * 128 + k];
          c += (double)W1[(size_t)h * (NG + 256) + NG + 128 + k] * hw[ttgt->off + (size_t)z * 128 + k];
        }
        dtab[o.tsd + (size_t)z * RH + h] = a;
        dtab[o.ttd + (size_t)z * RH + h] = c;
      }
    o.w1g = push(w1g); o.w1gT = push(transpose(w1g.data(), RH, NG));
    o.w2T = push(transpose(hw + w2->off, RH, RH)); o.w3T = push(transpose(hw + w3->off, out, RH));
    roff[pre] = o;
    return UMX_OK;
  };
  CHK(radial_derive("edge_degree_embedding.rad_func", 3 * C));
  // ---- model variant: what the blob carries decides (pdb2reaction_amd/weights.py variant_of applies the same rule)
  const bool ff_grid = eng->wt.count("blocks.0.atom_wise.grid_mlp.0.weight") != 0;
  int grid_G = 0;
  if (ff_grid) {
    auto it = eng->wt.find("so3_grid.to_grid_mat");
    if (it == eng->wt.end() || it->second.shape.size() != 2 || it->second.shape[1] != S || it->second.shape[0] < 1 || it->second.shape[0] > 128)
      return fail(eng, UMX_ERR_WEIGHTS, "weight blob: the grid feed-forward needs so3_grid.to_grid_mat of shape (G <= 128, 9)");
    grid_G = it->second.shape[0];
    if (!need("so3_grid.from_grid_mat", {grid_G, S})) return UMX_ERR_WEIGHTS;
  }
  const int emb_type = eng->wt.count("charge_embedding.W") ? 1 : eng->wt.count("charge_embedding.lin_emb.weight") ? 2 : 0;
  int n_datasets = 0;
  if (eng->wt.count("dataset_embedding.weight")) {
    const Tensor& t = eng->wt["dataset_embedding.weight"];
    if (t.shape.size() != 2 || t.shape[1] != C || t.shape[0] < 1 || t.shape[0] > 32)
      return fail(eng, UMX_ERR_WEIGHTS, "weight blob: dataset_embedding.weight must be (1..32, 128)");
    n_datasets = t.shape[0];
  }
  struct LayOff { size_t c1m0T, c1m1T, c1m2T, c2m0T, c2m1T, c2m2T, smlpT, l1T, l2T, g1T, g2T, g3T; };
  LayOff loff[NL];
  auto half_T = [&](const float* src, int half, int kin) {   // W (2*half x kin) -> (2, kin, half)
    std::vector<float> t((size_t)2 * half * kin);
    for (int ab = 0; ab < 2; ++ab)
      for (int hh = 0; hh < half; ++hh)
        for (int k = 0; k < kin; ++k) t[((size_t)ab * kin + k) * half + hh] = src[((size_t)ab * half + hh) * kin + k];
    return t;
  };
  auto per_l_T = [&](const float* src) {                     // (3, out, in) -> (3, in, out)
    std::vector<float> t((size_t)3 * C * C);
    for (int l = 0; l < 3; ++l)
      for (int o = 0; o < C; ++o)
        for (int i = 0; i < C; ++i) t[((size_t)l * C + i) * C + o] = src[((size_t)l * C + o) * C + i];
    return t;
  };
  for (int i = 0; i < NL; ++i) {
    const std::string bpre = "blocks." + std::to_string(i);
    const std::string c1 = bpre + ".edge_wise.so2_conv_1", c2 = bpre + ".edge_wise.so2_conv_2", aw = bpre + ".atom_wise";
    const Tensor *a = need(c1 + ".fc_m0.weight", {640, 768}), *b1m = need(c1 + ".so2_m_conv.0.fc.weight", {512, 512}),
                 *c = need(c1 + ".so2_m_conv.1.fc.weight", {256, 256}), *d = need(c2 + ".fc_m0.weight", {384, 384}),
                 *e = need(c2 + ".so2_m_conv.0.fc.weight", {512, 256}), *f = need(c2 + ".so2_m_conv.1.fc.weight", {256, 128});
    if (!a || !b1m || !c || !d || !e || !f) return UMX_ERR_WEIGHTS;
    const Tensor *g = nullptr, *h1 = nullptr, *h2 = nullptr, *q1 = nullptr, *q2 = nullptr, *q3 = nullptr;
    if (ff_grid) {
      q1 = need(aw + ".grid_mlp.0.weight", {128, 128}); q2 = need(aw + ".grid_mlp.2.weight", {128, 128}); q3 = need(aw + ".grid_mlp.4.weight", {128, 128});
      if (!q1 || !q2 || !q3) return UMX_ERR_WEIGHTS;
      for (const char* li : {".grid_mlp.0.bias", ".grid_mlp.2.bias", ".grid_mlp.4.bias"})
        if (eng->wt.count(aw + li) && !need(aw + li, {128})) return UMX_ERR_WEIGHTS;
    } else {
      g = need(aw + ".scalar_mlp.weight", {256, 128}); h1 = need(aw + ".so3_linear_1.weight", {3, 128, 128}); h2 = need(aw + ".so3_linear_2.weight", {3, 128, 128});
      if (!g || !h1 || !h2 || !need(aw + ".scalar_mlp.bias", {256}) || !need(aw + ".so3_linear_1.bias", {128}) || !need(aw + ".so3_linear_2.bias", {128}))
        return UMX_ERR_WEIGHTS;
    }
    if (!need(c1 + ".fc_m0.bias", {640}) || !need(c2 + ".fc_m0.bias", {384}) ||
        !need(bpre + ".norm_1.affine_weight", {3, 128}) || !need(bpre + ".norm_1.affine_bias", {128}) ||
        !need(bpre + ".norm_2.affine_weight", {3, 128}) || !need(bpre + ".norm_2.affine_bias", {128}))
      return UMX_ERR_WEIGHTS;
    CHK(radial_derive(c1 + ".rad_func", RAD));
    loff[i].c1m0T = push(transpose(hw + a->off, 640, 768));
    loff[i].c1m1T = push(half_T(hw + b1m->off, 256, 512));
    loff[i].c1m2T = push(half_T(hw + c->off, 128, 256));
    loff[i].c2m0T = push(transpose(hw + d->off, 384, 384));
    loff[i].c2m1T = push(half_T(hw + e->off, 256, 256));
    loff[i].c2m2T = push(half_T(hw + f->off, 128, 128));
    loff[i].smlpT = loff[i].l1T = loff[i].l2T = loff[i].g1T = loff[i].g2T = loff[i].g3T = 0;
    if (ff_grid) {
      loff[i].g1T = push(transpose(hw + q1->off, 128, 128)); loff[i].g2T = push(transpose(hw + q2->off, 128, 128)); loff[i].g3T = push(transpose(hw + q3->off, 128, 128));
    } else {
      loff[i].smlpT = push(transpose(hw + g->off, 256, 128));
      loff[i].l1T = push(per_l_T(hw + h1->off));
      loff[i].l2T = push(per_l_T(hw + h2->off));
    }
  }
  const Tensor *te0 = need("energy_block.0.weight", {128, 128}), *te2 = need("energy_block.2.weight", {128, 128}),
               *te4 = need("energy_block.4.weight", {1, 128});
  if (!te0 || !te2 || !te4 || !need("energy_block.0.bias", {128}) || !need("energy_block.2.bias", {128}) ||
      !need("energy_block.4.bias", {1}) || !need("norm.affine_weight", {3, 128}) || !need("norm.affine_bias", {128}) ||
      !need("sphere_embedding.weight", {NZ, 128}) ||
      !need("mix_csd.weight", {128, (n_datasets ? 3 : 2) * 128}) || !need("mix_csd.bias", {128}) || !need("normalizer.rmsd", {1}) ||
      !need("element_refs", {NZ}))
    return UMX_ERR_WEIGHTS;
  if (emb_type == 0 && (!need("charge_embedding.weight", {201, 128}) || !need("spin_embedding.weight", {101, 128}))) return UMX_ERR_WEIGHTS;
  if (emb_type == 1 && (!need("charge_embedding.W", {64}) || !need("spin_embedding.W", {64}))) return UMX_ERR_WEIGHTS;
  if (emb_type == 2 && (!need("charge_embedding.lin_emb.weight", {128, 1}) || !need("charge_embedding.lin_emb.bias", {128}) ||
                        !need("spin_embedding.lin_emb.weight", {128, 1}) || !need("spin_embedding.lin_emb.bias", {128})))
    return UMX_ERR_WEIGHTS;
  const size_t oe0T = push(transpose(hw + te0->off, 128, 128)), oe2T = push(transpose(hw + te2->off, 128, 128));

  // ---- upload ----
  if (eng->d_w) { HIPCHK(eng, hipFree(eng->d_w)); eng->d_w = nullptr; }
  if (eng->d_dw) { HIPCHK(eng, hipFree(eng->d_dw)); eng->d_dw = nullptr; }
  HIPCHK(eng, hipMalloc(&eng->d_w, eng->h_w.size() * sizeof(float)));
  HIPCHK(eng, hipMemcpy(eng->d_w, eng->h_w.data(), eng->h_w.size() * sizeof(float), hipMemcpyHostToDevice));
  HIPCHK(eng, hipMalloc(&eng->d_dw, dw.size() * sizeof(float)));
  HIPCHK(eng, hipMemcpy(eng->d_dw, dw.data(), dw.size() * sizeof(float), hipMemcpyHostToDevice));
  if (eng->d_dtab) { HIPCHK(eng, hipFree(eng->d_dtab)); eng->d_dtab = nullptr; }
  HIPCHK(eng, hipMalloc(&eng->d_dtab, dtab.size() * sizeof(double)));
  HIPCHK(eng, hipMemcpy(eng->d_dtab, dtab.data(), dtab.size() * sizeof(double), hipMemcpyHostToDevice));
  auto W = [&](const std::string& nm) -> const float* { return eng->d_w + eng->wt[nm].off; };
  auto D = [&](size_t o) -> const float* { return eng->d_dw + o; };
  // ---- plane-interleaved bf16 copies (umx_gemm_pl.h "PL" layout) of the large weights: P=3 for the forward
  //      orientation, P=2 for the transposed (reverse-pass) orientation; RNE split with exact residuals ----
  std::vector<unsigned short> bw;
  struct PlaneReq { const float* dev; size_t off; };
  std::vector<PlaneReq> preq;
  // precision mode (read here: the weight planes below are packed in the forward operand format it selects)
  {
    const char* pv = std::getenv("UMX_PRECISION");
    const std::string mode = !eng->precision.empty() ? eng->precision : (pv && *pv ? pv : "auto");
    // "auto" (the default) = bf16x3: the reference runs fairchem's float32 inference settings (uma_pysis.py:229,246-250), and bf16x3 is the
    // mode whose every product, forward and reverse, carries >= 24 significant bits -- the like-for-like arithmetic.  The faster split-f16
    // (22-bit forward activations, 16-bit reverse products) meets the tolerances with margin but is narrower: an explicit choice.
    bool rev3 = false;
    if (mode == "fp32") eng->pl = false;
    else if (mode == "auto" || mode == "bf16x3" || mode == "split-exact") { eng->pl = true; eng->fwd_fmt = 3; rev3 = true; }   // 24-bit products in BOTH passes
    else if (mode == "split" || mode == "split-f16") { eng->pl = true; eng->fwd_fmt = 1; }
    else if (mode == "split-bf16") { eng->pl = true; eng->fwd_fmt = 3; }
    else return fail(eng, UMX_ERR_ARG, "UMX_PRECISION must be auto, bf16x3 (= split-exact), split (= split-f16), split-bf16 or fp32");
    eng->rev_planes = (eng->pl && rev3) ? 3 : 2;
    eng->rev_qf = eng->pl && eng->rev_planes == 3;
    // a precision change alters the workspace carve-up: force a re-carve on the next call
    eng->cap_nodes = 0; eng->cap_edges = 0;
  }
  eng->plane_scale.clear();
  // IEEE binary16 <- binary32, round to nearest even, subnormals kept (what v_cvt_f16_f32 does for the activations)
  auto to_half = [](float f) -> unsigned short {
    uint32_t x; std::memcpy(&x, &f, 4);
    const unsigned short sign = (unsigned short)((x >> 16) & 0x8000u);
    x &= 0x7FFFFFFFu;
    if (x > 0x7F800000u) return (unsigned short)(sign | 0x7E00u);
    if (x >= 0x477FF000u) return (unsigned short)(sign | 0x7C00u);            // >= 65520 rounds to infinity
    if (x < 0x38800000u) {                                                    // below 2^-14: a multiple of 2^-24
      float a; std::memcpy(&a, &x, 4);
      return (unsigned short)(sign | (unsigned short)std::lrintf(a * 16777216.0f));
    }
    uint32_t h = (((x >> 23) - 112u) << 10) | ((x & 0x7FFFFFu) >> 13);
    const uint32_t rem = x & 0x1FFFu;
    if (rem > 0x1000u || (rem == 0x1000u && (h & 1u))) ++h;                   // a carry moves into the exponent as it should
    return (unsigned short)(sign | h);
  };
  auto from_half = [](unsigned short h) -> float {
    const uint32_t sign = (uint32_t)(h & 0x8000u) << 16, e = (h >> 10) & 0x1Fu, m = h & 0x3FFu;
    float v;
    if (e == 0) v = (float)m * (1.0f / 16777216.0f);
    else { const uint32_t u = ((e + 112u) << 23) | (m << 13); std::memcpy(&v, &u, 4); }     // (weights are finite: no inf/nan case)
    uint32_t u; std::memcpy(&u, &v, 4); u |= sign; std::memcpy(&v, &u, 4);
    return v;
  };
  // fp16 quad-row copy of a forward weight: three half planes of s * w, s = the power of two that puts max|w| into [2^14, 2^15):
  // 33 significand bits -- exact for every weight above max|w| * 2^-16, an absolute 2^-39 max|w| below.
  auto want_planes_f16 = [&](const float* host, const float* dev, int rows, int K) {
    const int PB = 3;
    PlaneReq r{dev, (bw.size() + 63) & ~size_t(63)};
    bw.resize(r.off + (size_t)rows * K * PB);
    float mx = 0.f;
    for (size_t i = 0; i < (size_t)rows * K; ++i) mx = std::max(mx, std::fabs(host[i]));
    int ex = 0;
    if (mx > 0.f && std::isfinite(mx)) { std::frexp(mx, &ex); ex = std::max(-24, std::min(40, 15 - ex)); }   // mx = f * 2^ex', f in [0.5, 1)
    const float sc = std::ldexp(1.0f, ex);
    eng->plane_scale[dev] = sc;
    for (int rr = 0; rr < rows; ++rr)
      for (int k = 0; k < K; ++k) {
        float x = host[(size_t)rr * K + k] * sc;
        const size_t o = r.off + (((size_t)(rr / 4) * (K / 16) + k / 16) * (128 * PB) + (size_t)(rr % 4) * (32 * PB) + (size_t)(k % 16) * 2) / 2;
        for (int q = 0; q < PB; ++q) { const unsigned short hq = to_half(x); bw[o + 16 * q] = hq; x -= from_half(hq); }
      }
    preq.push_back(r);
  };
  // P = 3: a forward weight (quad-row layout / fp16 planes as the mode says); P = 2: a transposed (reverse-pass) weight -- always the PL
  // layout, with the engine's reverse plane count
  eng->planes_q.clear();
  auto want_planes = [&](const float* host, const float* dev, int rows, int K, int P, bool rev_quad = false) {
    const bool fwdw = (P == 3);
    if (!fwdw) P = eng->rev_planes;
    const bool quad = fwdw || (rev_quad && P == 3);
    eng->planes_q[dev] = quad;
    if (fwdw && eng->fwd_fmt == 1) { want_planes_f16(host, dev, rows, K); return; }
    PlaneReq r{dev, (bw.size() + 63) & ~size_t(63)};
    bw.resize(r.off + (size_t)rows * K * P);
    // aligned planes (forward bf16 weights): the value that goes into plane q < 2 is first rounded to a multiple of 2^(e_max - 12), e_max =
    // exponent of the largest magnitude of what is left of the 8 weights the matrix core sees in one pass (k = 8 g ... 8 g + 7 of one row);
    // the exact remainder goes down the planes, so w0 + w1 + w2 is what it was (umx_gemm_pl.h qf_align_magic does the same to A's leading plane)
    const bool alignw = fwdw && quad && eng->align != 0;
    for (int rr = 0; rr < rows; ++rr)
      for (int k0 = 0; k0 < K; k0 += 8) {                 // (K is a multiple of 32 everywhere)
        float rem[8];
        for (int j = 0; j < 8; ++j) rem[j] = host[(size_t)rr * K + k0 + j];
        for (int q = 0; q < P; ++q) {
          float quantum = 0.f;
          if (alignw && q < 2) {
            float gm = 0.f;
            for (int j = 0; j < 8; ++j) gm = std::max(gm, std::fabs(rem[j]));
            if (gm > 0.f && std::isfinite(gm)) { int eg; std::frexp(gm, &eg); quantum = std::ldexp(1.0f, eg - 1 - 12); }
          }
          for (int j = 0; j < 8; ++j) {
            const int k = k0 + j;
            const float lead = quantum > 0.f ? std::nearbyint(rem[j] / quantum) * quantum : rem[j];
            uint32_t u; std::memcpy(&u, &lead, 4);
            const uint32_t rnd = u + 0x7FFFu + ((u >> 16) & 1u);
            const unsigned short hb = (unsigned short)(rnd >> 16);
            if (quad)                  // quad-row layout (umx_gemm_q.h), index in bf16 units; rows are multiples of 4 here
              bw[r.off + (((size_t)(rr / 4) * (K / 16) + k / 16) * 384 + (size_t)(rr % 4) * 96 + (size_t)q * 32 + (size_t)(k % 16) * 2) / 2] = hb;
            else
              bw[r.off + (size_t)rr * K * P + (size_t)(k / 32) * 32 * P + (size_t)q * 32 + (k % 32)] = hb;
            const uint32_t back = (uint32_t)hb << 16; float fb; std::memcpy(&fb, &back, 4);
            rem[j] -= fb;
          }
        }
      }
    preq.push_back(r);
  };
  const float* hd = dw.data();
  for (int i = 0; i < NL; ++i) {
    const std::string bpre = "blocks." + std::to_string(i);
    const std::string c1 = bpre + ".edge_wise.so2_conv_1", c2 = bpre + ".edge_wise.so2_conv_2";
    auto WH = [&](const std::string& nm, int rows, int K) { want_planes(hw + eng->wt[nm].off, W(nm), rows, K, 3); };
    WH(c1 + ".fc_m0.weight", 640, 768); WH(c1 + ".so2_m_conv.0.fc.weight", 512, 512); WH(c1 + ".so2_m_conv.1.fc.weight", 256, 256);
    WH(c2 + ".fc_m0.weight", 384, 384); WH(c2 + ".so2_m_conv.0.fc.weight", 512, 256); WH(c2 + ".so2_m_conv.1.fc.weight", 256, 128);
    WH(c1 + ".rad_func.fc3.weight", RAD, RH);
    // the conv^T weights follow their A operands (g_msg / g_hg): quad-row layout in the bf16x3 mode; fc3^T stays PL (g_rad comes from the
    // node-centric k_modrot_bwd_pl, whose rows are written edge by edge)
    want_planes(hd + loff[i].c1m0T, D(loff[i].c1m0T), 768, 640, 2, true); want_planes(hd + loff[i].c1m1T, D(loff[i].c1m1T), 2 * 512, 256, 2, true);
    want_planes(hd + loff[i].c1m2T, D(loff[i].c1m2T), 2 * 256, 128, 2, true); want_planes(hd + loff[i].c2m0T, D(loff[i].c2m0T), 384, 384, 2, true);
    want_planes(hd + loff[i].c2m1T, D(loff[i].c2m1T), 2 * 256, 256, 2, true); want_planes(hd + loff[i].c2m2T, D(loff[i].c2m2T), 2 * 128, 128, 2, true);
    want_planes(hd + roff[c1 + ".rad_func"].w3T, D(roff[c1 + ".rad_func"].w3T), RH, RAD, 2);
  }
  {   // the edge-degree radial MLP's fc3 (128 -> 384) and its transpose run on the split path too
    const std::string nm = "edge_degree_embedding.rad_func.fc3.weight";
    want_planes(hw + eng->wt[nm].off, W(nm), 3 * C, RH, 3);
    const size_t t = roff["edge_degree_embedding.rad_func"].w3T;
    want_planes(hd + t, D(t), RH, 3 * C, 2);
  }
  if (eng->d_bw) { HIPCHK(eng, hipFree(eng->d_bw)); eng->d_bw = nullptr; }
  HIPCHK(eng, hipMalloc(&eng->d_bw, bw.size() * sizeof(unsigned short)));
  HIPCHK(eng, hipMemcpy(eng->d_bw, bw.data(), bw.size() * sizeof(unsigned short), hipMemcpyHostToDevice));
  eng->planes.clear();
  for (const auto& r : preq) eng->planes[r.dev] = eng->d_bw + r.off;
  auto fill_rad = [&](RadialW& r, const std::string& pre, int out) {
    const RadOff& o = roff[pre];
    r.w1g = D(o.w1g); r.w1gT = D(o.w1gT); r.w2T = D(o.w2T); r.w3T = D(o.w3T);
    r.tsd = eng->d_dtab + o.tsd; r.ttd = eng->d_dtab + o.ttd;
    r.ln1w = W(pre + ".ln1.weight"); r.ln1b = W(pre + ".ln1.bias"); r.w2 = W(pre + ".fc2.weight"); r.b2 = W(pre + ".fc2.bias");
    r.ln2w = W(pre + ".ln2.weight"); r.ln2b = W(pre + ".ln2.bias"); r.w3 = W(pre + ".fc3.weight"); r.b3 = W(pre + ".fc3.bias");
    r.out = out;
  };
  fill_rad(eng->rdeg, "edge_degree_embedding.rad_func", 3 * C);
  for (int i = 0; i < NL; ++i) {
    const std::string bpre = "blocks." + std::to_string(i);
    const std::string c1 = bpre + ".edge_wise.so2_conv_1", c2 = bpre + ".edge_wise.so2_conv_2", aw = bpre + ".atom_wise";
    LayerW& L = eng->lw[i];
    L.n1w = W(bpre + ".norm_1.affine_weight"); L.n1b = W(bpre + ".norm_1.affine_bias");
    L.n2w = W(bpre + ".norm_2.affine_weight"); L.n2b = W(bpre + ".norm_2.affine_bias");
    L.c1m0 = W(c1 + ".fc_m0.weight"); L.c1m0b = W(c1 + ".fc_m0.bias"); L.c1m0T = D(loff[i].c1m0T);
    L.c1m1 = W(c1 + ".so2_m_conv.0.fc.weight"); L.c1m1T = D(loff[i].c1m1T);
    L.c1m2 = W(c1 + ".so2_m_conv.1.fc.weight"); L.c1m2T = D(loff[i].c1m2T);
    L.c2m0 = W(c2 + ".fc_m0.weight"); L.c2m0b = W(c2 + ".fc_m0.bias"); L.c2m0T = D(loff[i].c2m0T);
    L.c2m1 = W(c2 + ".so2_m_conv.0.fc.weight"); L.c2m1T = D(loff[i].c2m1T);
    L.c2m2 = W(c2 + ".so2_m_conv.1.fc.weight"); L.c2m2T = D(loff[i].c2m2T);
    L.smlp = L.smlpb = L.smlpT = L.l1w = L.l1b = L.l1T = L.l2w = L.l2b = L.l2T = nullptr;
    L.g1w = L.g1b = L.g1T = L.g2w = L.g2b = L.g2T = L.g3w = L.g3b = L.g3T = nullptr;
    if (ff_grid) {
      auto WB = [&](const std::string& nm) -> const float* { return eng->wt.count(nm) ? W(nm) : nullptr; };
      L.g1w = W(aw + ".grid_mlp.0.weight"); L.g1b = WB(aw + ".grid_mlp.0.bias"); L.g1T = D(loff[i].g1T);
      L.g2w = W(aw + ".grid_mlp.2.weight"); L.g2b = WB(aw + ".grid_mlp.2.bias"); L.g2T = D(loff[i].g2T);
      L.g3w = W(aw + ".grid_mlp.4.weight"); L.g3b = WB(aw + ".grid_mlp.4.bias"); L.g3T = D(loff[i].g3T);
    } else {
      L.smlp = W(aw + ".scalar_mlp.weight"); L.smlpb = W(aw + ".scalar_mlp.bias"); L.smlpT = D(loff[i].smlpT);
      L.l1w = W(aw + ".so3_linear_1.weight"); L.l1b = W(aw + ".so3_linear_1.bias"); L.l1T = D(loff[i].l1T);
      L.l2w = W(aw + ".so3_linear_2.weight"); L.l2b = W(aw + ".so3_linear_2.bias"); L.l2T = D(loff[i].l2T);
    }
    fill_rad(L.rad, c1 + ".rad_func", RAD);
  }
  eng->emb_sphere = W("sphere_embedding.weight");
  eng->normw = W("norm.affine_weight"); eng->normb = W("norm.affine_bias");
  eng->e0 = W("energy_block.0.weight"); eng->e0b = W("energy_block.0.bias"); eng->e0T = D(oe0T);
  eng->e2 = W("energy_block.2.weight"); eng->e2b = W("energy_block.2.bias"); eng->e2T = D(oe2T);
  eng->e4 = W("energy_block.4.weight"); eng->e4b = W("energy_block.4.bias");
  eng->rmsd = (double)hw[eng->wt["normalizer.rmsd"].off];
  eng->elem_refs.assign(NZ, 0.0);
  for (int z = 0; z < NZ; ++z) eng->elem_refs[z] = (double)hw[eng->wt["element_refs"].off + z];
  if (ff_grid != eng->ff_grid || grid_G != eng->grid_G) { eng->cap_nodes = 0; eng->cap_edges = 0; }     // the per-node workspace changes with the variant
  eng->ff_grid = ff_grid; eng->grid_G = grid_G; eng->emb_type = emb_type; eng->n_datasets = n_datasets;
  eng->to_grid = ff_grid ? W("so3_grid.to_grid_mat") : nullptr; eng->from_grid = ff_grid ? W("so3_grid.from_grid_mat") : nullptr;
  eng->variant = std::string("ff=") + (ff_grid ? "grid(G=" + std::to_string(grid_G) + ")" : std::string("spectral")) + ";emb=" +
                 (emb_type == 1 ? "pos_emb" : emb_type == 2 ? "lin_emb" : "rand_emb") + ";datasets=" + std::to_string(n_datasets);
  eng->have_weights = true;
  eng->have_system = false;
  return UMX_OK;
}

int umx_load_weights(umx_engine* eng, const void* blob, size_t nbytes) {
  if (!eng || !blob) return UMX_ERR_ARG;
  return load_weights_impl(eng, blob, nbytes);
}

const char* umx_precision_mode(const umx_engine* eng) {
  if (!eng || !eng->have_weights) return "";
  return !eng->pl ? "fp32" : eng->fwd_fmt == 1 ? "split-f16" : eng->rev_planes == 3 ? "bf16x3" : "split-bf16";
}

const char* umx_model_variant(const umx_engine* eng) {
  if (!eng || !eng->have_weights) return "";
  return eng->variant.c_str();
}

int umx_set_system(umx_engine* eng, int n_atoms, const int32_t* z, int charge, int spin, int task_index, float radius, int max_neigh) {
  if (!eng) return UMX_ERR_ARG;
  if (!eng->have_weights) return fail(eng, UMX_ERR_ARG, "umx_set_system: load weights first");
  if (n_atoms <= 0 || !z) return fail(eng, UMX_ERR_ARG, "umx_set_system: empty system");
  if (charge < -100 || charge > 100) return fail(eng, UMX_ERR_ARG, "umx_set_system: charge outside [-100, 100]");
  if (spin < 0 || spin > 100) return fail(eng, UMX_ERR_ARG, "umx_set_system: spin multiplicity outside [0, 100]");
  if (eng->n_datasets > 0 && (task_index < 0 || task_index >= eng->n_datasets))
    return fail(eng, UMX_ERR_ARG, "umx_set_system: task index outside [0, " + std::to_string(eng->n_datasets - 1) + "] (rows of the blob's dataset_embedding.weight)");
  HIPCHK(eng, hipSetDevice(eng->dev));
  double rs = 0.0;
  for (int i = 0; i < n_atoms; ++i) {
    if (z[i] < 0 || z[i] >= NZ) return fail(eng, UMX_ERR_ARG, "umx_set_system: atomic number outside [0, 99]");
    rs += eng->elem_refs[z[i]];
  }
  HIPCHK(eng, hipStreamSynchronize(eng->stream));
  if (eng->d_z) { HIPCHK(eng, hipFree(eng->d_z)); eng->d_z = nullptr; }
  HIPCHK(eng, hipMalloc(&eng->d_z, n_atoms * sizeof(int)));
  HIPCHK(eng, hipMemcpy(eng->d_z, z, n_atoms * sizeof(int), hipMemcpyHostToDevice));
  if (!eng->d_sysemb) HIPCHK(eng, hipMalloc(&eng->d_sysemb, C * sizeof(double)));
  {
    // system embedding silu(mix_csd [chg | spin | dataset]) in double on the host (setup, once per system): it is
    // added to EVERY atom in every layer, so any error in it is a same-sign energy bias that grows with N.
    const float* hw = eng->h_w.data();
    auto HW = [&](const std::string& nm) -> const float* { return hw + eng->wt[nm].off; };
    // ChgSpinEmbedding in the blob's form (fairchem chg_spin_emb_type [3P-UNVERIFIED]): rand_emb = table row (charge + 100 / multiplicity);
    // pos_emb = [sin(2 pi v W) | cos(2 pi v W)], the null spin 0 embedding to zero; lin_emb = Linear(1 -> C) of v (null spin 0 -> -100)
    double chg[C], spn[C], dst[C];
    auto emb = [&](const char* which, int v, bool is_spin, double* out) {
      const std::string pre = std::string(which) + "_embedding.";
      if (eng->emb_type == 1) {
        const float* w = HW(pre + "W");
        for (int k = 0; k < C / 2; ++k) {
          const double ang = 2.0 * 3.14159265358979323846 * (double)v * (double)w[k];
          out[k] = (is_spin && v == 0) ? 0.0 : std::sin(ang);
          out[C / 2 + k] = (is_spin && v == 0) ? 0.0 : std::cos(ang);
        }
      } else if (eng->emb_type == 2) {
        const float *w = HW(pre + "lin_emb.weight"), *b = HW(pre + "lin_emb.bias");
        const double x = (is_spin && v == 0) ? -100.0 : (double)v;
        for (int k = 0; k < C; ++k) out[k] = (double)w[k] * x + (double)b[k];
      } else {
        const float* t = HW(pre + "weight") + (size_t)(v + (is_spin ? 0 : 100)) * C;
        for (int k = 0; k < C; ++k) out[k] = t[k];
      }
    };
    emb("charge", charge, false, chg);
    emb("spin", spin, true, spn);
    const int nd = eng->n_datasets;
    for (int k = 0; k < C; ++k) dst[k] = nd ? (double)HW("dataset_embedding.weight")[(size_t)task_index * C + k] : 0.0;
    const float* mw = HW("mix_csd.weight");
    const float* mb = HW("mix_csd.bias");
    const size_t ldm = (size_t)(nd ? 3 : 2) * C;
    double se[C];
    for (int o = 0; o < C; ++o) {
      double acc = mb[o];
      for (int k = 0; k < C; ++k) {
        if (nd) acc += (double)mw[o * ldm + k] * chg[k] + (double)mw[o * ldm + C + k] * spn[k] + (double)mw[o * ldm + 2 * C + k] * dst[k];
        else acc += (double)mw[o * ldm + k] * chg[k] + (double)mw[o * ldm + C + k] * spn[k];
      }
      se[o] = acc / (1.0 + std::exp(-acc));
    }
    HIPCHK(eng, hipMemcpy(eng->d_sysemb, se, sizeof(se), hipMemcpyHostToDevice));
  }
  eng->natoms = n_atoms;
  eng->refsum = rs;
  eng->cutoff = radius > 0.f ? radius : 6.0f;
  {
    const double delta = (double)eng->cutoff / (NG - 1);
    double mu[NG];
    for (int k = 0; k < NG; ++k) mu[k] = k * delta;
    eng->gcoef = -0.5 / ((2.0 * delta) * (2.0 * delta));
    if (!eng->d_gmu) HIPCHK(eng, hipMalloc(&eng->d_gmu, NG * sizeof(double)));
    HIPCHK(eng, hipMemcpy(eng->d_gmu, mu, sizeof(mu), hipMemcpyHostToDevice));
  }
  eng->max_neigh = max_neigh > 0 ? max_neigh : 300;
  eng->have_system = true;
  return UMX_OK;
}

int umx_synchronize(umx_engine* eng) {
  if (!eng) return UMX_ERR_ARG;
  HIPCHK(eng, hipSetDevice(eng->dev));
  HIPCHK(eng, hipStreamSynchronize(eng->stream));
  if (eng->ran_on_caller) HIPCHK(eng, hipEventSynchronize(eng->ev_done));     // the engine's own event, not the caller's stream handle
  // the device-pointer entries cannot look at their results: a non-finite energy left the sticky flag behind
  int flag = 0;
  HIPCHK(eng, hipMemcpy(&flag, eng->d_flags, sizeof(int), hipMemcpyDeviceToHost));
  if (flag) {
    HIPCHK(eng, hipMemset(eng->d_flags, 0, sizeof(int)));
    return fail(eng, UMX_ERR_RANGE, std::string("a device-pointer evaluation produced a non-finite energy") +
                (eng->pl && eng->fwd_fmt == 1 ? " (an activation beyond the fp16 operand range of the split-f16 forward planes: re-load with UMX_PRECISION=split-bf16, bf16x3 or fp32)"
                                              : " (non-finite input or an overflow in float32)"));
  }
  return UMX_OK;
}

// ---- one image in P target-node partitions on ONE GPU ----------------------------------------------------------------------------
// The graph-parallel plan (exchange points, partial sums over a rank's own edges) run for P "virtual ranks" one after another: each
// partition keeps its own PERSISTENT workspace (node-level state + the per-edge activations of its edges), all of them share ONE
// TRANSIENT region (the producer -> GEMM operands are dead at every exchange point), and the all-reduce of an exchange point is a local
// sum.  Memory per directed edge drops from ~120 KB to ~72 KB + 48 KB / P, i.e. a single image of up to ~1.5x the atoms fits the same
// HBM; node-level work (< 3 %) is done P times.  Used automatically when one image exceeds the workspace budget.
struct PartPtrs { float* p[16]; int n; };
__global__ void k_sum_parts(PartPtrs pp, size_t count, float* __restrict__ also) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= count) return;
  float sum = 0.f;
  for (int k = 0; k < pp.n; ++k) sum += pp.p[k][i];          // fixed order: deterministic
  for (int k = 0; k < pp.n; ++k) pp.p[k][i] = sum;
  if (also) also[i] = sum;
}

static int eval_partitioned(umx_engine* eng, hipStream_t s, const float* d_pos, double* d_energy, float* d_forces, int P, size_t budget,
                            int64_t* edges_out, int* maxdeg_out) {
  const int N = eng->natoms;
  if (P < 2 || P > 16) return fail(eng, UMX_ERR_ARG, "eval_partitioned: 2..16 partitions");
  if (eng->part_cap < (long)P * N) {
    HIPCHK(eng, hipStreamSynchronize(s));
    if (eng->d_part_deg) HIPCHK(eng, hipFree(eng->d_part_deg));
    if (eng->d_part_f) HIPCHK(eng, hipFree(eng->d_part_f));
    eng->d_part_deg = nullptr; eng->d_part_f = nullptr; eng->part_cap = 0;
    HIPCHK(eng, hipMalloc(&eng->d_part_deg, ((size_t)2 * P * N + 32) * sizeof(int)));
    HIPCHK(eng, hipMalloc(&eng->d_part_f, (size_t)P * N * 3 * sizeof(float)));
    eng->part_cap = (long)P * N;
  }
  int* d_cnt = eng->d_part_deg + (size_t)2 * P * N;           // [P] edge totals, [P] = max degree
  HIPCHK(eng, hipMemsetAsync(d_cnt, 0, (P + 1) * sizeof(int), s));
  std::vector<long> lo(P), hi(P);
  for (int p = 0; p < P; ++p) {
    lo[p] = (long)N * p / P; hi[p] = (long)N * (p + 1) / P;
    int* deg = eng->d_part_deg + (size_t)(2 * p) * N;
    hipLaunchKernelGGL(k_graph_count, dim3(nblk(N, 4)), dim3(256), 0, s, d_pos, N, (long)N, eng->cutoff * eng->cutoff, eng->max_neigh, deg, deg + N,
                       lo[p], hi[p], eng->d_flags);
    hipLaunchKernelGGL(k_image_edges, dim3(1), dim3(256), 0, s, deg, N, d_cnt + p, d_cnt + P);
  }
  HIPCHK(eng, hipGetLastError());
  std::vector<int> cnt(P + 1);
  int flag = 0;
  HIPCHK(eng, hipMemcpyAsync(cnt.data(), d_cnt, (P + 1) * sizeof(int), hipMemcpyDeviceToHost, s));
  HIPCHK(eng, hipMemcpyAsync(&flag, eng->d_flags, sizeof(int), hipMemcpyDeviceToHost, s));
  HIPCHK(eng, hipStreamSynchronize(s));
  if (flag & 2) { HIPCHK(eng, hipMemsetAsync(eng->d_flags, 0, sizeof(int), s)); return fail(eng, UMX_ERR_ARG, "umx_energy_forces: non-finite position (device buffer)"); }
  eng->may_truncate = cnt[P] >= eng->max_neigh;
  // layout: P persistent regions, then one transient region sized for the largest partition
  const int mode = ws_mode(eng);
  const int gridG = eng->ff_grid ? eng->grid_G : 0;
  std::vector<size_t> off(P + 1, 0);
  size_t tmax = 0;
  for (int p = 0; p < P; ++p) {
    Bump bp{nullptr}; WS t; carve_persist(bp, N, cnt[p], t, gridG);
    off[p + 1] = off[p] + ((bp.off + 255) & ~size_t(255));
    Bump bt{nullptr}; carve_trans(bt, cnt[p], t, mode);
    tmax = std::max(tmax, (bt.off + 255) & ~size_t(255));
  }
  const size_t total = off[P] + tmax;
  if (total > budget) return UMX_ERR_CAPACITY;              // (the caller tries more partitions)
  if (eng->arena_bytes < total) {
    HIPCHK(eng, hipStreamSynchronize(s));
    HIPCHK(eng, hipStreamSynchronize(eng->stream2));
    if (eng->arena) { HIPCHK(eng, hipFree(eng->arena)); eng->arena = nullptr; eng->arena_bytes = 0; }
    HIPCHK(eng, hipMalloc(&eng->arena, total));
    ++eng->arena_allocs;
    eng->arena_bytes = total;
  }
  eng->cap_nodes = 0; eng->cap_edges = 0;                    // the ordinary path re-carves (and re-sizes) the arena on its next call
  std::vector<WS> ws(P);
  for (int p = 0; p < P; ++p) {
    Bump bp{eng->arena + off[p]}; carve_persist(bp, N, cnt[p], ws[p], gridG);
    Bump bt{eng->arena + off[P]}; carve_trans(bt, cnt[p], ws[p], mode);
  }
  std::vector<Plan> plans(P);
  const bool gp_keep = eng->gp; const long lo_keep = eng->gp_lo, hi_keep = eng->gp_hi;
  for (int p = 0; p < P; ++p) {
    eng->gp = true; eng->gp_lo = lo[p]; eng->gp_hi = hi[p];
    int* deg = eng->d_part_deg + (size_t)(2 * p) * N;
    plan_chunk(eng, ws[p], d_pos, deg, deg + N, 1, cnt[p], d_energy, d_forces ? eng->d_part_f + (size_t)p * N * 3 : nullptr, plans[p]);
  }
  eng->gp = gp_keep; eng->gp_lo = lo_keep; eng->gp_hi = hi_keep;
  std::vector<size_t> at(P, 0);
  int st = UMX_OK;
  for (;;) {
    PartPtrs pp; pp.n = P;
    size_t count = 0; int waiting = 0;
    for (int p = 0; p < P && st == UMX_OK; ++p) {
      pp.p[p] = nullptr;
      while (at[p] < plans[p].segs.size()) {
        Seg& sg = plans[p].segs[at[p]++];
        if (sg.sync_buf) { pp.p[p] = sg.sync_buf; count = sg.sync_count; ++waiting; break; }
        st = sg.fn();
        if (st != UMX_OK) break;
      }
    }
    if (st != UMX_OK || waiting == 0) break;
    if (waiting != P) { st = fail(eng, UMX_ERR_ARG, "eval_partitioned: the partitions' plans disagree on their exchange points"); break; }
    const bool is_forces = d_forces && pp.p[0] == eng->d_part_f;
    hipLaunchKernelGGL(k_sum_parts, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, s, pp, count, is_forces ? d_forces : (float*)nullptr);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) { st = fail(eng, UMX_ERR_HIP, std::string("k_sum_parts: ") + hipGetErrorName(e)); break; }
  }
  if (st != UMX_OK) return st;
  *edges_out = 0;
  for (int p = 0; p < P; ++p) *edges_out += cnt[p];
  *maxdeg_out = cnt[P];
  return UMX_OK;
}

// Evaluate on `run_stream` (may be the legacy default stream 0).  eng->stream is swapped for the duration so that every
// helper launches there; it is restored on every exit path.
static int energy_forces_on(umx_engine* eng, hipStream_t run_stream, int n_images, const float* d_pos, double* d_energy, float* d_forces) {
  hipStream_t own = eng->stream;
  eng->stream = run_stream;
  eng->ran_on_caller = (run_stream != own);
  struct Restore { umx_engine* e; hipStream_t s; ~Restore() { e->stream = s; } } restore{eng, own};
  hipStream_t s = eng->stream;
  const int N = eng->natoms;
  const long K = n_images, nt = K * N;
  // pass 1: degrees of every node of every image, per-image edge totals
  if (eng->deg_all_cap < nt) {
    HIPCHK(eng, hipStreamSynchronize(s));
    if (eng->d_deg_all) HIPCHK(eng, hipFree(eng->d_deg_all));
    if (eng->d_cand_all) HIPCHK(eng, hipFree(eng->d_cand_all));
    eng->d_deg_all = nullptr; eng->d_cand_all = nullptr; eng->deg_all_cap = 0;
    HIPCHK(eng, hipMalloc(&eng->d_deg_all, nt * sizeof(int)));
    HIPCHK(eng, hipMalloc(&eng->d_cand_all, nt * sizeof(int)));
    eng->deg_all_cap = nt;
  }
  if (eng->img_edges_cap < K + 1) {
    HIPCHK(eng, hipStreamSynchronize(s));
    if (eng->d_img_edges) HIPCHK(eng, hipFree(eng->d_img_edges));
    eng->d_img_edges = nullptr; eng->img_edges_cap = 0;          // a failed hipMalloc below must not leave a dangling pointer
    HIPCHK(eng, hipMalloc(&eng->d_img_edges, (K + 1) * sizeof(int)));
    eng->img_edges_cap = K + 1;
  }
  HIPCHK(eng, hipMemsetAsync(eng->d_img_edges + K, 0, sizeof(int), s));
  hipLaunchKernelGGL(k_graph_count, dim3(nblk(nt, 4)), dim3(256), 0, s, d_pos, N, nt, eng->cutoff * eng->cutoff, eng->max_neigh, eng->d_deg_all, eng->d_cand_all,
                     eng->gp ? eng->gp_lo : 0L, eng->gp ? eng->gp_hi : nt, eng->d_flags);
  hipLaunchKernelGGL(k_image_edges, dim3((unsigned)K), dim3(256), 0, s, eng->d_deg_all, N, eng->d_img_edges, eng->d_img_edges + K);
  HIPCHK(eng, hipGetLastError());
  std::vector<int> img_edges(K + 1);
  int range_flag = 0;
  HIPCHK(eng, hipMemcpyAsync(img_edges.data(), eng->d_img_edges, (K + 1) * sizeof(int), hipMemcpyDeviceToHost, s));
  HIPCHK(eng, hipMemcpyAsync(&range_flag, eng->d_flags, sizeof(int), hipMemcpyDeviceToHost, s));
  HIPCHK(eng, hipStreamSynchronize(s));
  if (range_flag) {
    HIPCHK(eng, hipMemsetAsync(eng->d_flags, 0, sizeof(int), s));
    if (range_flag & 2)      // set by THIS call's k_graph_count
      return fail(eng, UMX_ERR_ARG, "umx_energy_forces: non-finite position (device buffer)" +
                  std::string((range_flag & 1) ? "; the previous device-pointer evaluation had already produced a non-finite energy" : ""));
    // bit 0: set by an EARLIER evaluation through a device-pointer entry (this one has not computed an energy yet; on this stream that
    // evaluation is complete): its caller got NaN energies / forces and, most likely, derived these positions from them
    return fail(eng, UMX_ERR_RANGE, std::string("the previous device-pointer evaluation produced a non-finite energy") +
                (eng->pl && eng->fwd_fmt == 1 ? " (an activation beyond the fp16 operand range of the split-f16 forward planes: re-load with UMX_PRECISION=split-bf16, bf16x3 or fp32)"
                                              : " (non-finite input or an overflow in float32)"));
  }
  eng->last_maxdeg = img_edges[K];
  eng->may_truncate = img_edges[K] >= eng->max_neigh;          // (degrees are min(candidates, max_neigh): below the cap nothing was cut)
  eng->last_edges = 0;
  for (long k = 0; k < K; ++k) eng->last_edges += img_edges[k];
  // chunk planning under the workspace budget
  size_t budget = eng->ws_limit;
  if (!budget) {
    size_t fr = 0, tot = 0;
    HIPCHK(eng, hipMemGetInfo(&fr, &tot));
    budget = (size_t)((fr + eng->arena_bytes) * 0.85);
    // default cap (UMX_WS_GB, 0 = none): chunks beyond a few images buy no speed (NOTES.md section 4), and an engine that takes
    // 85 % of the HBM starves every other engine of the process (a second calculator, the FD-Hessian helper, ...)
    if (eng->ws_cap_default && budget > eng->ws_cap_default) {
      long emax = 0;
      for (long k = 0; k < K; ++k) emax = std::max(emax, (long)img_edges[k]);
      if (carve(nullptr, N, emax, nullptr, ws_mode_g(eng)) <= eng->ws_cap_default) budget = eng->ws_cap_default;   // (a single image larger than the cap keeps the full budget)
    }
  }
  int lanes = (eng->n_lanes >= 2 && K >= 2 && !eng->dbg_on && !eng->gp) ? 2 : 1;      // debug captures name ONE chunk's buffers
  if (eng->n_lanes == 0 && K >= 2 && !eng->dbg_on && !eng->gp && eng->force_parts < 2 && eng->lanes_auto_edges > 0 && eng->last_edges >= eng->lanes_auto_edges) {
    long emax = 0;
    for (long k = 0; k < K; ++k) emax = std::max(emax, (long)img_edges[k]);
    if (carve(nullptr, N, emax, nullptr, ws_mode_g(eng)) <= budget / 2) lanes = 2;
  }
  budget /= lanes;
  // Amortised workspace (ABI v8).  Allocating device memory costs ~45 ms per GiB on this driver (it is cleared), so a workspace sized for the
  // whole batch -- up to the 160 GiB cap: 7 s -- is only worth it for a run that lasts: a one-off finite-difference Hessian of a 500-atom
  // system spent 11 of its 15 s allocating.  Chunks of ~320 k directed edges already run within 3 % of the largest ones (DESIGN.md section
  // 7), so without a hint (umx_reserve_images, which announces a long run of known batches) the workspace starts at that size and grows to
  // what the batch would like only once the engine has been evaluating for 8x as long as the larger allocation takes.
  {
    const double now = std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count();
    if (eng->t_first_eval < 0.0) eng->t_first_eval = now;
    if (!eng->ws_eager && eng->hint_images == 0 && !eng->gp && !eng->dbg_on && eng->force_parts < 2) {
      long emax = 1, etot = 0;
      for (long k = 0; k < K; ++k) { emax = std::max(emax, (long)img_edges[k]); etot += img_edges[k]; }
      const long per = std::max(1L, (eng->ws_soft_edges + emax - 1) / emax);                      // images per chunk for ~ws_soft_edges
      const size_t want = carve(nullptr, per * N, per * (emax + emax / 20 + 64), nullptr, ws_mode_g(eng));
      const size_t cur = eng->cap_nodes > 0 ? carve(nullptr, eng->cap_nodes, eng->cap_edges, nullptr, ws_mode_g(eng)) : 0;
      size_t soft = std::min(budget, std::max(want, cur));
      const size_t full = std::min(budget, carve(nullptr, K * N, etot + etot / 50 + 1024, nullptr, ws_mode_g(eng)));
      if (full > soft && (now - eng->t_first_eval) >= 8.0 * 0.045 * (double)(full >> 20) / 1024.0) soft = full;
      budget = soft;
    }
  }
  long max_chunk = (K + lanes - 1) / lanes;          // at least `lanes` chunks so both streams have work
  if (const char* ev = std::getenv("UMX_MAX_CHUNK_IMAGES")) { long v = std::atol(ev); if (v > 0) max_chunk = std::min(max_chunk, v); }
  std::vector<std::pair<long, long>> chunks;   // [k0, k1)
  long need_nodes = 0, need_edges = 0;
  auto plan = [&](long cap) -> int {
    chunks.clear(); need_nodes = 0; need_edges = 0;
    for (long k0 = 0; k0 < K;) {
      long k1 = k0, e = 0;
      while (k1 < K && (k1 - k0) < cap) {
        const long e2 = e + img_edges[k1];
        if (k1 > k0 && carve(nullptr, (k1 - k0 + 1) * N, e2, nullptr, ws_mode_g(eng)) > budget) break;
        e = e2; ++k1;
      }
      if (carve(nullptr, (k1 - k0) * N, e, nullptr, ws_mode_g(eng)) > budget)
        return fail(eng, UMX_ERR_CAPACITY, "one image (" + std::to_string(N) + " atoms, " + std::to_string(e) + " directed edges) needs " +
                                               std::to_string(carve(nullptr, N, e, nullptr, ws_mode_g(eng)) >> 20) + " MiB of workspace, budget is " +
                                               std::to_string(budget >> 20) + " MiB: a structure of this size has to be evaluated in the graph-parallel mode, its edges "
                                               "partitioned over several GPUs (umx_gp_begin / umx_gp_step; uma_pysis(workers=<ranks>) under torch.distributed, one rank per GPU)");
      chunks.push_back({k0, k1});
      need_nodes = std::max(need_nodes, (k1 - k0) * N);
      need_edges = std::max(need_edges, e);
      k0 = k1;
    }
    return UMX_OK;
  };
  {
    const int pst = eng->force_parts >= 2 ? UMX_ERR_CAPACITY : plan(max_chunk);
    if (pst == UMX_ERR_CAPACITY && !eng->gp && !eng->dbg_on) {
      // One image does not fit the budget in one piece (or UMX_FORCE_PARTS): image by image, in as few target-node partitions as fit
      const std::string why = eng->err;
      int64_t etot = 0; int mdeg = 0;
      for (long k = 0; k < K; ++k) {
        int stp = UMX_ERR_CAPACITY;
        for (int parts = eng->force_parts >= 2 ? eng->force_parts : 2; parts <= 16 && stp == UMX_ERR_CAPACITY; parts = eng->force_parts >= 2 ? 17 : parts + 1) {
          int64_t e1 = 0; int m1 = 0;
          stp = eval_partitioned(eng, s, d_pos + k * N * 3, d_energy + k, d_forces ? d_forces + k * N * 3 : nullptr, parts, budget * lanes, &e1, &m1);
          if (stp == UMX_OK) { etot += e1; mdeg = std::max(mdeg, m1); eng->last_parts = parts; }
        }
        if (stp == UMX_ERR_CAPACITY) return fail(eng, UMX_ERR_CAPACITY, why + " -- and not in 16 partitions on this GPU either");
        if (stp != UMX_OK) return stp;
      }
      eng->last_edges = etot; eng->last_maxdeg = mdeg;
      HIPCHK(eng, hipEventRecord(eng->ev_done, s));
      return UMX_OK;
    }
    if (pst != UMX_OK) return pst;
    eng->last_parts = 0;
  }
  if (lanes == 2 && chunks.size() > 1) {
    // the lanes work in pairs of chunks: an even number of chunks of (nearly) equal size, so that no chunk runs without a partner
    const long n_even = (long)((chunks.size() + 1) / 2 * 2);
    CHK(plan((K + n_even - 1) / n_even));
  }
  // umx_reserve_images: the caller announced batches of up to hint_images images -- size the workspace once for that many images of the
  // densest image at hand (+5 %) instead of growing it batch by batch (every growth re-allocates the whole region); ignored when it
  // does not fit the budget
  long hint_nodes = 0, hint_edges = 0;
  if (eng->hint_images > 0 && !eng->gp && lanes == 1) {
    long emax = 0;
    for (long k = 0; k < K; ++k) emax = std::max(emax, (long)img_edges[k]);
    long hint_img = eng->hint_images;                                       // (a chunk never holds more than UMX_MAX_CHUNK_IMAGES images)
    if (const char* ev = std::getenv("UMX_MAX_CHUNK_IMAGES")) { const long v = std::atol(ev); if (v > 0) hint_img = std::min(hint_img, v); }
    hint_nodes = hint_img * N;
    hint_edges = hint_img * (emax + emax / 20 + 64);
    if ((hint_nodes <= eng->cap_nodes && hint_edges <= eng->cap_edges) || carve(nullptr, hint_nodes, hint_edges, nullptr, ws_mode_g(eng)) > budget) hint_nodes = hint_edges = 0;
  }
  // (the hint alone triggers ONE allocation; after that it only enlarges a growth the batches themselves ask for -- otherwise every batch
  // whose densest image is a little denser than the last one's would re-allocate)
  const bool hint_now = eng->hint_applied != eng->hint_images && (hint_nodes > eng->cap_nodes || hint_edges > eng->cap_edges);
  if (eng->hint_images > 0 && (hint_nodes || hint_edges || eng->cap_nodes >= (long)eng->hint_images * N)) eng->hint_applied = eng->hint_images;
  if (need_nodes > eng->cap_nodes || need_edges > eng->cap_edges || hint_now) {
    HIPCHK(eng, hipStreamSynchronize(s));
    HIPCHK(eng, hipStreamSynchronize(eng->stream2));
    if (eng->arena) { HIPCHK(eng, hipFree(eng->arena)); eng->arena = nullptr; eng->arena_bytes = 0; }
    long cn = std::max(std::max(need_nodes, hint_nodes), eng->cap_nodes), ce = std::max(std::max(need_edges + need_edges / 50 + 1024, hint_edges), eng->cap_edges);
    size_t bytes = carve(nullptr, cn, ce, nullptr, ws_mode_g(eng));
    if (bytes > budget && (hint_nodes || hint_edges)) {      // hint and need combined overshoot: size for the need alone
      cn = std::max(need_nodes, eng->cap_nodes); ce = std::max(need_edges + need_edges / 50 + 1024, eng->cap_edges);
      bytes = carve(nullptr, cn, ce, nullptr, ws_mode_g(eng));
    }
    long ce2 = ce;
    if (bytes > budget) { ce2 = std::max(need_edges, 1L); bytes = carve(nullptr, cn, ce2, nullptr, ws_mode_g(eng)); }
    HIPCHK(eng, hipMalloc(&eng->arena, lanes * bytes));     // one workspace per lane
    ++eng->arena_allocs;
    eng->arena_bytes = lanes * bytes; eng->cap_nodes = cn; eng->cap_edges = ce2;
  }
  WS wl[2];
  long use_nodes = eng->cap_nodes, use_edges = eng->cap_edges;
  if (lanes == 2 && eng->arena_bytes < 2 * carve(nullptr, use_nodes, use_edges, nullptr, ws_mode_g(eng))) {
    // the arena was sized for ONE lane of larger chunks (an engine that has seen smaller batches, or one lane, before): two lanes of THIS
    // call's chunks may still fit it -- else one lane
    const long ce = need_edges + need_edges / 50 + 1024;
    if (2 * carve(nullptr, need_nodes, ce, nullptr, ws_mode_g(eng)) <= eng->arena_bytes) { use_nodes = need_nodes; use_edges = ce; }
    else lanes = 1;
  }
  const size_t lane_bytes = carve(eng->arena, use_nodes, use_edges, &wl[0], ws_mode_g(eng));
  if (lanes == 2) carve(eng->arena + lane_bytes, use_nodes, use_edges, &wl[1], ws_mode_g(eng));
  if (eng->dbg_on) eng->dbg.clear();
  eng->last_lanes = (lanes == 2 && chunks.size() > 1) ? 2 : 1;
  if (lanes == 2) {          // lane 1 starts after everything enqueued so far on the primary stream (degree pass, caller's work)
    HIPCHK(eng, hipEventRecord(eng->ev_fork, s));
    HIPCHK(eng, hipStreamWaitEvent(eng->stream2, eng->ev_fork, 0));
  }
  if (eng->gp) {
    // graph-parallel: record the plan of the one chunk and hand control back; umx_gp_step issues it segment by segment, pausing at
    // every exchange point.  The workspace view must outlive this call (the closures hold a reference to it).
    WS* keep = new WS(wl[0]);
    Plan* P = new Plan();
    plan_chunk(eng, *keep, d_pos, eng->d_deg_all, eng->d_cand_all, 1, img_edges[0], d_energy, d_forces, *P);
    eng->gp_ws = keep; eng->gp_plan = P; eng->gp_at = 0; eng->gp_stream = s;
    return UMX_OK;
  }
  int st = UMX_OK;
  auto plan_of = [&](size_t ci, int lane, Plan& P) {
    const long k0 = chunks[ci].first, k1 = chunks[ci].second;
    long e = 0;
    for (long k = k0; k < k1; ++k) e += img_edges[k];
    plan_chunk(eng, wl[lane], d_pos + k0 * N * 3, eng->d_deg_all + k0 * N, eng->d_cand_all + k0 * N, k1 - k0, e, d_energy + k0,
               d_forces ? d_forces + k0 * N * 3 : nullptr, P);
  };
  if (lanes == 2) {          // chunks in pairs, one per lane, matrix segments alternating between the lanes (run_plans_alternating)
    // UMX_LANES_ONE_STREAM=1 (tests): both lanes' segments in the same alternating order on ONE stream -- the two-lane plan without any
    // concurrency (what results must be bitwise equal to; with real concurrency see NOTES.md section 5, item 14)
    hipStream_t sts[2] = {s, std::getenv("UMX_LANES_ONE_STREAM") ? s : eng->stream2};
    hipEvent_t tok[2] = {eng->ev_tok[0], eng->ev_tok[1]};
    for (size_t ci = 0; ci < chunks.size() && st == UMX_OK; ci += 2) {
      Plan P[2];
      plan_of(ci, 0, P[0]);
      if (ci + 1 < chunks.size()) {
        plan_of(ci + 1, 1, P[1]);
        eng->throttle = true;
        st = run_plans_alternating(eng, P, sts, tok);
        eng->throttle = false;
      } else {
        eng->stream = s;
        st = run_plan(eng, P[0]);
      }
    }
  } else {
    for (size_t ci = 0; ci < chunks.size() && st == UMX_OK; ++ci) {
      Plan P;
      plan_of(ci, 0, P);
      eng->stream = s;
      st = run_plan(eng, P);
    }
  }
  eng->stream = s;
  if (lanes == 2) {          // join: the primary stream continues only after lane 1 has drained
    HIPCHK(eng, hipEventRecord(eng->ev_join, eng->stream2));
    HIPCHK(eng, hipStreamWaitEvent(s, eng->ev_join, 0));
  }
  if (st != UMX_OK) return st;
  HIPCHK(eng, hipEventRecord(eng->ev_done, s));
  return UMX_OK;
}

int umx_energy_forces_dev(umx_engine* eng, int n_images, const float* d_pos, double* d_energy, float* d_forces, void* hip_stream) {
  if (!eng) return UMX_ERR_ARG;
  if (!eng->have_system) return fail(eng, UMX_ERR_ARG, "umx_energy_forces: bind a system first (umx_set_system)");
  if (n_images <= 0 || !d_pos || !d_energy) return fail(eng, UMX_ERR_ARG, "umx_energy_forces: bad arguments");
  if (eng->gp_plan) return fail(eng, UMX_ERR_ARG, "umx_energy_forces: a graph-parallel evaluation is in progress (finish it with umx_gp_step)");
  HIPCHK(eng, hipSetDevice(eng->dev));
  // NULL = the legacy default stream (hipStream_t 0): the work is then ordered after everything the caller has enqueued on
  // the default stream (the producer of d_pos) and before whatever it enqueues next (the consumer of d_energy / d_forces),
  // exactly as with an explicit stream.  The engine's private non-blocking stream is never used for caller-owned buffers.
  return energy_forces_on(eng, static_cast<hipStream_t>(hip_stream), n_images, d_pos, d_energy, d_forces);
}

static void gp_clear(umx_engine* eng) {
  delete static_cast<Plan*>(eng->gp_plan);
  delete static_cast<WS*>(eng->gp_ws);
  eng->gp_plan = nullptr; eng->gp_ws = nullptr; eng->gp_at = 0; eng->gp = false;
}

int umx_gp_begin(umx_engine* eng, const float* d_pos, int node_lo, int node_hi, double* d_energy, float* d_forces, void* hip_stream) {
  if (!eng) return UMX_ERR_ARG;
  if (!eng->have_system) return fail(eng, UMX_ERR_ARG, "umx_gp_begin: bind a system first (umx_set_system)");
  if (!d_pos || !d_energy || !d_forces) return fail(eng, UMX_ERR_ARG, "umx_gp_begin: bad arguments (forces are part of the exchange)");
  if (node_lo < 0 || node_hi > eng->natoms || node_lo > node_hi) return fail(eng, UMX_ERR_ARG, "umx_gp_begin: node range outside [0, n_atoms]");
  if (eng->gp_plan) gp_clear(eng);                       // an abandoned evaluation
  HIPCHK(eng, hipSetDevice(eng->dev));
  eng->gp = true; eng->gp_lo = node_lo; eng->gp_hi = node_hi;
  const int st = energy_forces_on(eng, static_cast<hipStream_t>(hip_stream), 1, d_pos, d_energy, d_forces);
  if (st != UMX_OK) gp_clear(eng);
  return st;
}

int umx_gp_step(umx_engine* eng, float** d_buf, size_t* count, int* done) {
  if (!eng || !d_buf || !count || !done) return UMX_ERR_ARG;
  if (!eng->gp_plan) return fail(eng, UMX_ERR_ARG, "umx_gp_step: no graph-parallel evaluation in progress (umx_gp_begin)");
  HIPCHK(eng, hipSetDevice(eng->dev));
  Plan* P = static_cast<Plan*>(eng->gp_plan);
  hipStream_t own = eng->stream;
  eng->stream = eng->gp_stream;
  int st = UMX_OK;
  *d_buf = nullptr; *count = 0; *done = 0;
  while (eng->gp_at < P->segs.size()) {
    Seg& sg = P->segs[eng->gp_at++];
    if (sg.sync_buf) { *d_buf = sg.sync_buf; *count = sg.sync_count; eng->stream = own; return UMX_OK; }
    st = sg.fn();
    if (st != UMX_OK) break;
  }
  eng->stream = own;
  if (st == UMX_OK) {
    *done = 1;
    eng->ran_on_caller = true;
    hipError_t e = hipEventRecord(eng->ev_done, eng->gp_stream);
    if (e != hipSuccess) st = fail(eng, UMX_ERR_HIP, std::string("umx_gp_step: ") + hipGetErrorName(e));
  }
  gp_clear(eng);
  return st;
}

// ---- in-process peer sum (umx_peer.h) -----------------------------------------------------------------------------------------------
namespace {
struct PeerState {
  hipEvent_t ev_in[PEER_MAX] = {}, ev_out[PEER_MAX] = {};   // per participant: "my buffer is ready" / "my slice has landed everywhere"
  int ev_dev[PEER_MAX];
  std::set<std::pair<int, int>> enabled;                    // device pairs whose peer access is on
  PeerState() { for (int& d : ev_dev) d = -1; }
} g_peer;

int peer_fail(int code, const std::string& msg) { g_create_err = msg; return code; }

#define PEERCHK(expr)                                                                                          \
  do {                                                                                                         \
    hipError_t _e = (expr);                                                                                    \
    if (_e != hipSuccess) { (void)hipSetDevice(dev0); return peer_fail(UMX_ERR_HIP, std::string("umx_peer_sum: " #expr ": ") + hipGetErrorName(_e)); } \
  } while (0)
}  // namespace

int umx_peer_sum(int n_peers, float* const* d_bufs, size_t count, const int* device_ordinals, void* const* hip_streams) {
  if (n_peers < 1 || n_peers > PEER_MAX || !d_bufs || !device_ordinals || !hip_streams)
    return peer_fail(UMX_ERR_ARG, "umx_peer_sum: 1.." + std::to_string(PEER_MAX) + " participants with buffers, device ordinals and streams");
  int ndev = 0, dev0 = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0 || hipGetDevice(&dev0) != hipSuccess) return peer_fail(UMX_ERR_NO_DEVICE, "umx_peer_sum: no HIP device visible");
  PeerBufs b{};
  for (int r = 0; r < n_peers; ++r) {
    if (!d_bufs[r] || (reinterpret_cast<uintptr_t>(d_bufs[r]) & 15) != 0) return peer_fail(UMX_ERR_ARG, "umx_peer_sum: buffer " + std::to_string(r) + " is null or not 16-byte aligned");
    if (device_ordinals[r] < 0 || device_ordinals[r] >= ndev) return peer_fail(UMX_ERR_ARG, "umx_peer_sum: device ordinal of participant " + std::to_string(r) + " out of range");
    for (int q = 0; q < r; ++q)
      if (d_bufs[q] == d_bufs[r]) return peer_fail(UMX_ERR_ARG, "umx_peer_sum: participants " + std::to_string(q) + " and " + std::to_string(r) + " list the same buffer");
    b.p[r] = d_bufs[r];
  }
  if (n_peers == 1 || count == 0) return UMX_OK;
  // peer access, once per ordered device pair (nothing to do when all buffers share a device)
  for (int r = 0; r < n_peers; ++r)
    for (int q = 0; q < n_peers; ++q) {
      const int a = device_ordinals[r], c = device_ordinals[q];
      if (a == c || g_peer.enabled.count({a, c})) continue;
      int can = 0;
      PEERCHK(hipDeviceCanAccessPeer(&can, a, c));
      if (!can) return peer_fail(UMX_ERR_HIP, "umx_peer_sum: device " + std::to_string(a) + " cannot access the memory of device " + std::to_string(c) +
                                 " (hipDeviceCanAccessPeer = 0): the in-process pool needs peer access between all of its devices");
      PEERCHK(hipSetDevice(a));
      const hipError_t e = hipDeviceEnablePeerAccess(c, 0);
      if (e != hipSuccess && e != hipErrorPeerAccessAlreadyEnabled) {
        (void)hipSetDevice(dev0);
        return peer_fail(UMX_ERR_HIP, "umx_peer_sum: peer access from device " + std::to_string(a) + " to device " + std::to_string(c) + " cannot be enabled: " + hipGetErrorName(e));
      }
      (void)hipGetLastError();
      g_peer.enabled.insert({a, c});
    }
  for (int r = 0; r < n_peers; ++r) {
    if (g_peer.ev_dev[r] == device_ordinals[r]) continue;
    if (g_peer.ev_dev[r] >= 0) { PEERCHK(hipSetDevice(g_peer.ev_dev[r])); (void)hipEventDestroy(g_peer.ev_in[r]); (void)hipEventDestroy(g_peer.ev_out[r]); g_peer.ev_dev[r] = -1; }
    PEERCHK(hipSetDevice(device_ordinals[r]));
    PEERCHK(hipEventCreateWithFlags(&g_peer.ev_in[r], hipEventDisableTiming));
    PEERCHK(hipEventCreateWithFlags(&g_peer.ev_out[r], hipEventDisableTiming));
    g_peer.ev_dev[r] = device_ordinals[r];
  }
  // opening barrier: every buffer is complete (and no longer read by its owner's earlier work) before a peer reads or writes it
  for (int r = 0; r < n_peers; ++r) {
    PEERCHK(hipSetDevice(device_ordinals[r]));
    PEERCHK(hipEventRecord(g_peer.ev_in[r], static_cast<hipStream_t>(hip_streams[r])));
  }
  for (int r = 0; r < n_peers; ++r) {
    hipStream_t s = static_cast<hipStream_t>(hip_streams[r]);
    PEERCHK(hipSetDevice(device_ordinals[r]));
    for (int q = 0; q < n_peers; ++q)
      if (q != r) PEERCHK(hipStreamWaitEvent(s, g_peer.ev_in[q], 0));
    size_t lo, hi;
    peer_slice(count, n_peers, r, &lo, &hi);
    PEERCHK(launch_peer_sum(b, n_peers, lo, hi, s));
    PEERCHK(hipEventRecord(g_peer.ev_out[r], s));
  }
  // closing barrier: a participant goes on only when every peer's slice has landed in its buffer
  for (int r = 0; r < n_peers; ++r) {
    PEERCHK(hipSetDevice(device_ordinals[r]));
    for (int q = 0; q < n_peers; ++q)
      if (q != r) PEERCHK(hipStreamWaitEvent(static_cast<hipStream_t>(hip_streams[r]), g_peer.ev_out[q], 0));
  }
  (void)hipSetDevice(dev0);
  return UMX_OK;
}

int umx_energy_forces(umx_engine* eng, int n_images, const float* pos, double* energy, float* forces) {
  if (!eng) return UMX_ERR_ARG;
  if (!eng->have_system) return fail(eng, UMX_ERR_ARG, "umx_energy_forces: bind a system first (umx_set_system)");
  if (n_images <= 0 || !pos || !energy) return fail(eng, UMX_ERR_ARG, "umx_energy_forces: bad arguments");
  if (eng->gp_plan) return fail(eng, UMX_ERR_ARG, "umx_energy_forces: a graph-parallel evaluation is in progress (finish it with umx_gp_step)");
  HIPCHK(eng, hipSetDevice(eng->dev));
  const long nt = (long)n_images * eng->natoms;
  if (eng->io_cap < nt) {
    HIPCHK(eng, hipStreamSynchronize(eng->stream));
    if (eng->d_io_pos) HIPCHK(eng, hipFree(eng->d_io_pos));
    if (eng->d_io_f) HIPCHK(eng, hipFree(eng->d_io_f));
    eng->d_io_pos = nullptr; eng->d_io_f = nullptr; eng->io_cap = 0;
    HIPCHK(eng, hipMalloc(&eng->d_io_pos, nt * 3 * sizeof(float)));
    HIPCHK(eng, hipMalloc(&eng->d_io_f, nt * 3 * sizeof(float)));
    eng->io_cap = nt;
  }
  if (eng->io_img_cap < n_images) {
    HIPCHK(eng, hipStreamSynchronize(eng->stream));
    if (eng->d_io_e) HIPCHK(eng, hipFree(eng->d_io_e));
    eng->d_io_e = nullptr; eng->io_img_cap = 0;
    HIPCHK(eng, hipMalloc(&eng->d_io_e, (size_t)n_images * sizeof(double)));
    eng->io_img_cap = n_images;
  }
  for (long i = 0; i < nt * 3; ++i)         // a NaN coordinate would silently drop its atom from the radius graph (every comparison false)
    if (!std::isfinite(pos[i])) return fail(eng, UMX_ERR_ARG, "umx_energy_forces: non-finite position (image " + std::to_string(i / ((long)eng->natoms * 3)) + ")");
  HIPCHK(eng, hipMemcpyAsync(eng->d_io_pos, pos, nt * 3 * sizeof(float), hipMemcpyHostToDevice, eng->stream));
  CHK(energy_forces_on(eng, eng->stream, n_images, eng->d_io_pos, eng->d_io_e, forces ? eng->d_io_f : nullptr));
  HIPCHK(eng, hipMemcpyAsync(energy, eng->d_io_e, (size_t)n_images * sizeof(double), hipMemcpyDeviceToHost, eng->stream));
  if (forces) HIPCHK(eng, hipMemcpyAsync(forces, eng->d_io_f, nt * 3 * sizeof(float), hipMemcpyDeviceToHost, eng->stream));
  HIPCHK(eng, hipStreamSynchronize(eng->stream));
  for (int k = 0; k < n_images; ++k)
    if (!std::isfinite(energy[k])) {
      (void)hipMemset(eng->d_flags, 0, sizeof(int));         // reported right here: do not fail the NEXT call for it as well
      return fail(eng, UMX_ERR_RANGE, "image " + std::to_string(k) + ": non-finite energy" +
                  (eng->pl && eng->fwd_fmt == 1 ? " (an activation beyond the fp16 operand range of UMX_PRECISION=split: try split-bf16, bf16x3 or fp32)"
                                                : " (an overflow in float32)"));
    }
  return UMX_OK;
}

int umx_set_precision(umx_engine* eng, const char* mode) {
  if (!eng) return UMX_ERR_ARG;
  const std::string m = mode ? mode : "";
  if (!m.empty() && m != "auto" && m != "split" && m != "split-f16" && m != "split-bf16" && m != "bf16x3" && m != "split-exact" && m != "fp32")
    return fail(eng, UMX_ERR_ARG, "umx_set_precision: mode must be auto, split, split-f16, split-bf16, bf16x3 (= split-exact) or fp32");
  eng->precision = m;
  return UMX_OK;
}

int umx_last_graph_stats(const umx_engine* eng, int64_t* n_edges_total, int32_t* max_degree) {
  if (!eng) return UMX_ERR_ARG;
  if (n_edges_total) *n_edges_total = eng->last_edges;
  if (max_degree) *max_degree = eng->last_maxdeg;
  return UMX_OK;
}

int umx_last_partitions(const umx_engine* eng) { return eng ? eng->last_parts : 0; }
int umx_last_lanes(const umx_engine* eng) { return eng ? eng->last_lanes : 0; }

int umx_workspace_stats(const umx_engine* eng, int64_t* bytes, int32_t* allocations) {
  if (!eng) return UMX_ERR_ARG;
  if (bytes) *bytes = (int64_t)eng->arena_bytes;
  if (allocations) *allocations = eng->arena_allocs;
  return UMX_OK;
}

int umx_reserve_images(umx_engine* eng, int n_images) {
  if (!eng) return UMX_ERR_ARG;
  if (n_images < 0) return fail(eng, UMX_ERR_ARG, "umx_reserve_images: n_images must be >= 0");
  eng->hint_images = n_images;
  if (n_images == 0) eng->hint_applied = 0;
  return UMX_OK;
}

int umx_profile_enable(umx_engine* eng, int on) {
  if (!eng) return UMX_ERR_ARG;
  eng->prof_on = on != 0;
  return UMX_OK;
}

int umx_profile_read(umx_engine* eng, umx_profile_stats* out, int reset) {
  if (!eng) return UMX_ERR_ARG;
  if (out) std::memset(out, 0, sizeof(*out));
  HIPCHK(eng, hipSetDevice(eng->dev));
  HIPCHK(eng, hipStreamSynchronize(eng->stream));
  if (eng->prof_used) HIPCHK(eng, hipEventSynchronize(eng->prof[eng->prof_used - 1].b));   // events may sit on the caller's stream
  double ms = 0.0, fl = 0.0;
  FILE* dump = nullptr;
  if (const char* dp = std::getenv("UMX_PROFILE_DUMP")) dump = std::fopen(dp, "a");
  for (size_t i = 0; i < eng->prof_used; ++i) {
    float t = 0.f;
    HIPCHK(eng, hipEventElapsedTime(&t, eng->prof[i].a, eng->prof[i].b));
    ms += t; fl += eng->prof[i].flops;
    const ProfRec& r = eng->prof[i];
    if (out) {
      const int fam = r.prec > 0 ? 0 : (r.prec < 0 ? 2 : 1);
      out->ms[fam] += t; out->launches[fam] += 1; out->alg_flops[fam] += r.flops;
      out->mfma_flops[fam] += r.flops * (r.prec == 3 ? 6.0 : r.prec == 2 ? 3.0 : r.prec == 24 ? 4.0 : r.prec == 23 ? 3.0 : r.prec == 28 ? 6.0 : 1.0);   // (28: four fp16 + two bf8 products executed -- the bf8 ones at twice the rate)
    }
    if (dump) std::fprintf(dump, "%d,%d,%d,%d,%d,%d,%d,%.6f,%.6e\n", r.M, r.N, r.K, r.amode, r.cplx, r.prec, r.gz, t, r.flops);
  }
  if (dump) std::fclose(dump);
  (void)ms; (void)fl;
  if (reset) eng->prof_used = 0;
  return UMX_OK;
}

int umx_debug_keep(umx_engine* eng, int on) {
  if (!eng) return UMX_ERR_ARG;
  eng->dbg_on = on != 0;
  if (!on) eng->dbg.clear();
  return UMX_OK;
}

int umx_debug_fetch(umx_engine* eng, const char* name, void* host_buf, size_t capacity, size_t* nbytes_out) {
  if (!eng || !name) return UMX_ERR_ARG;
  auto it = eng->dbg.find(name);
  if (it == eng->dbg.end()) return fail(eng, UMX_ERR_ARG, std::string("umx_debug_fetch: no buffer named ") + name);
  if (nbytes_out) *nbytes_out = it->second.size();
  if (host_buf) {
    if (capacity < it->second.size()) return fail(eng, UMX_ERR_ARG, "umx_debug_fetch: buffer too small");
    std::memcpy(host_buf, it->second.data(), it->second.size());
  }
  return UMX_OK;
}

int umx_bond_changes(umx_engine* eng, int n, const double* r1, const double* r2, const double* cov, double bond_factor,
                     double margin_fraction, double delta_fraction, double* d1, double* d2, uint8_t* code) {
  if (!eng) return UMX_ERR_ARG;
  if (n <= 0 || !r1 || !r2 || !cov || !code) return fail(eng, UMX_ERR_ARG, "umx_bond_changes: bad arguments");
  if ((long)n * n > (1L << 31)) return fail(eng, UMX_ERR_CAPACITY, "umx_bond_changes: n*n exceeds 2^31 pairs");
  HIPCHK(eng, hipSetDevice(eng->dev));
  const size_t nn = (size_t)n * n, vb = (size_t)n * 3 * sizeof(double);
  double *d_r = nullptr, *d_d = nullptr; unsigned char* d_c = nullptr;
  HIPCHK(eng, hipMalloc(&d_r, 2 * vb + (size_t)n * sizeof(double)));
  hipError_t e1 = hipMalloc(&d_d, 2 * nn * sizeof(double)), e2 = hipMalloc(&d_c, nn);
  if (e1 != hipSuccess || e2 != hipSuccess) {
    (void)hipFree(d_r); if (d_d) (void)hipFree(d_d); if (d_c) (void)hipFree(d_c);
    return fail(eng, UMX_ERR_HIP, "umx_bond_changes: hipMalloc of the pair matrices failed");
  }
  double* d_r2 = d_r + (size_t)n * 3; double* d_cov = d_r2 + (size_t)n * 3;
  hipStream_t s = eng->stream;
  int st = UMX_OK;
  auto ok = [&](hipError_t e, const char* what) { if (e != hipSuccess && st == UMX_OK) st = fail(eng, UMX_ERR_HIP, std::string(what) + ": " + hipGetErrorName(e)); };
  ok(hipMemcpyAsync(d_r, r1, vb, hipMemcpyHostToDevice, s), "copy r1");
  ok(hipMemcpyAsync(d_r2, r2, vb, hipMemcpyHostToDevice, s), "copy r2");
  ok(hipMemcpyAsync(d_cov, cov, (size_t)n * sizeof(double), hipMemcpyHostToDevice, s), "copy cov");
  if (st == UMX_OK) {
    dim3 grid((n + 63) / 64, (n + 3) / 4);
    umx::k_bond_changes<<<grid, 256, 0, s>>>(d_r, d_r2, d_cov, n, bond_factor, margin_fraction, delta_fraction, d_d, d_d + nn, d_c);
    ok(hipGetLastError(), "k_bond_changes");
    if (d1) ok(hipMemcpyAsync(d1, d_d, nn * sizeof(double), hipMemcpyDeviceToHost, s), "copy d1");
    if (d2) ok(hipMemcpyAsync(d2, d_d + nn, nn * sizeof(double), hipMemcpyDeviceToHost, s), "copy d2");
    ok(hipMemcpyAsync(code, d_c, nn, hipMemcpyDeviceToHost, s), "copy code");
  }
  ok(hipStreamSynchronize(s), "sync");
  (void)hipFree(d_r); (void)hipFree(d_d); (void)hipFree(d_c);
  return st;
}

}  // extern "C"
