// umx_engine.h -- host side, part 1 of 5: the engine's state (struct umx_engine) and the small types it is made of: the precision
// descriptor, the weight views, the workspace view (WS), the launch plan (Seg / Plan and its one-lane executor), and the error / buffer helpers every other
// host header uses.  Host headers are included by umx_api.hip only, in this order: umx_engine.h, umx_launch.h, umx_workspace.h,
// umx_plan.h, umx_weights.h (one translation unit: every kernel template is instantiated once; they do not include one another).
#pragma once
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <chrono>
#include <cstring>
#include <functional>
#include <initializer_list>
#include <map>
#include <memory>
#include <set>
#include <string>
#include <type_traits>
#include <vector>

#include "../../include/umx.h"
#include "umx_common.h"
#include "umx_gemm.h"
#include "umx_gemm_pl.h"
#include "umx_gemm_q.h"
#include "umx_kernels.h"
#include "umx_edge.h"
#include "umx_graph.h"
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

// The positions of an evaluation as the graph kernels read them -- nothing else does: float32 (every entry but umx_energy_forces_f64[_dev])
// or float64, on the device.  Carried from the entry down to the two launchers of umx_periodic.h, which pick the instantiation.
struct PosPtr {
  const float* f = nullptr;
  const double* d = nullptr;
  PosPtr(const float* p) : f(p) {}
  PosPtr(const double* p) : d(p) {}
  PosPtr atom(long i) const { return d ? PosPtr(d + i * 3) : PosPtr(f + i * 3); }   // the same positions from atom i on
};

struct ProfRec { hipEvent_t a, b; double flops; int M, N, K, amode, cplx, prec, gz; };

// ---- precision mode ----------------------------------------------------------------------------
// What a mode name (UMX_PRECISION / umx_set_precision) means, resolved in ONE place (resolve_precision) at umx_load_weights -- the weight
// planes are packed in the forward operand format it selects -- and read everywhere else.
struct Precision {
  const char* name = "bf16x3";     // canonical name (umx_precision_mode)
  bool planes = true;              // split-precision plane GEMMs for the large SO(2) / radial linears; false (fp32): fp32 MFMA everywhere
  int fwd_fmt = 3;                 // forward operand format (QFmt, umx_edge.h): 1 = two fp16 planes (split-f16),
                                   // 3 = plain float32 quad-row blocks, split into three bf16 planes by the GEMM in registers (bf16x3, split-bf16)
  int rev_planes = 3;              // bf16 planes of the REVERSE-pass operands: 2 (3 products, 16-bit) or 3 (6 products, 24-bit: bf16x3)
  bool fwd_f16() const { return planes && fwd_fmt == 1; }
  bool rev_quad() const { return planes && rev_planes == 3; }   // reverse quad-row operands (g_msg, g_hg) as float32 blocks
  // what to tell the caller of a device-pointer entry about a non-finite energy
  const char* range_hint() const {
    return fwd_f16() ? " (an activation beyond the fp16 operand range of the split-f16 forward planes: re-load with UMX_PRECISION=split-bf16, bf16x3 or fp32)"
                     : " (non-finite input or an overflow in float32)";
  }
};

// "auto" (the default) = bf16x3: the reference runs fairchem's float32 inference settings (uma_pysis.py:229,246-250), and bf16x3 is the
// mode whose every product, forward and reverse, carries >= 24 significant bits -- the like-for-like arithmetic.  The faster split-f16
// (22-bit forward activations, 16-bit reverse products) meets the tolerances with margin but is narrower: an explicit choice.
bool resolve_precision(const std::string& mode, Precision* out) {
  Precision p;
  if (mode == "auto" || mode == "bf16x3" || mode == "split-exact") p = {"bf16x3", true, 3, 3};   // 24-bit products in BOTH passes
  else if (mode == "split" || mode == "split-f16") p = {"split-f16", true, 1, 2};
  else if (mode == "split-bf16") p = {"split-bf16", true, 3, 2};
  else if (mode == "fp32") p = {"fp32", false, 3, 2};      // (the plane copies are still packed, in the bf16 form; nothing reads them)
  else return false;
  if (out) *out = p;
  return true;
}

enum Pass { FWD, REV };   // which pass a split-precision product (gemm_pl) or a weight's plane copy (PlanePacker) belongs to

// one plane copy of a large weight, looked up by the weight's fp32 device pointer
struct PlaneCopy {
  const unsigned short* ptr;       // in d_bw
  bool quad;                       // quad-row layout (umx_gemm_q.h), else PL (umx_gemm_pl.h)
  float scale;                     // fp16 form: the power-of-two scale folded into the planes (else 0)
};

// ---- expert-form weights (umx_experts.h) -----------------------------------------------------------
// A blob whose 24 SO(2) weights are Mixture-of-Linear-Experts stacks (n, out, in) keeps the stacks on the device; umx_set_expert_coefficients
// merges them into the slots a host-merged blob would have filled (d_w, transposed copy in d_dw, plane copies in d_bw).  One record per
// weight (MergeJob) and per plane copy (PackJob), built by umx_load_weights, read by the two kernels from device memory.
constexpr int MAX_EXPERTS = 64;
constexpr int N_EXPERT_W = 6 * NL;          // the SO(2) weights of conv 1 and conv 2: fc_m0, so2_m_conv.0.fc, so2_m_conv.1.fc per layer
struct ExpertAlpha { double a[MAX_EXPERTS]; };
struct PackScales { float s[N_EXPERT_W]; };  // fp16 forward planes: the power-of-two scale of each forward weight (from its max |w|)
struct MergeJob {
  const float* stack;     // (n, rows, cols) float32
  float* w;               // merged (rows, cols) in d_w
  float* wT;              // reverse-pass copy in d_dw: (2, cols, half) with rows = 2 * half -- or the plain transpose, half = rows
  int rows, cols, half;
  int blk0;               // first workgroup of this job (32 x 128 tiles)
};
struct PackJob {
  const float* src;       // merged float32 weight (rows, K) in d_w or d_dw
  unsigned short* dst;    // its plane copy in d_bw
  int rows, K, P;         // P planes
  int quad, alignw;       // quad-row (else PL) layout; aligned leading planes
  int f16;                // fp16 planes of s * w, s = PackScales::s[f16 - 1] (0: bf16 planes)
  int blk0;               // first workgroup of this job (256 lanes, one 8-k group of one row each)
};

// ---- workspace view (carved by umx_workspace.h) --------------------------------------------------
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

// ---- launch plan (built by umx_plan.h) -----------------------------------------------------------
// A chunk's launch sequence is recorded as a PLAN of segments instead of being issued directly.  A segment is either
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
  // The one-lane executor: issue the segments from `at` on, on the stream eng->stream points at, up to the next exchange point or the
  // end.  *stop = the exchange point reached (`at` is behind it), nullptr at the end of the plan; a failing segment returns its status.
  int run_to_sync(size_t& at, const Seg** stop) {
    *stop = nullptr;
    while (at < segs.size()) {
      Seg& sg = segs[at++];
      if (sg.sync_buf) { *stop = &sg; return UMX_OK; }
      const int st = sg.fn();
      if (st != UMX_OK) return st;
    }
    return UMX_OK;
  }
};

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
  Precision prec;                  // the mode the weights were loaded in (umx_load_weights)
  std::string precision;           // umx_set_precision: overrides UMX_PRECISION when non-empty
  int low_sep = 3;                 // UMX_LOW_SEP (gemm_pl): which forward bf16x3 products chain their 2^-16-order plane products from zero
  int gate_epi = 1;                // UMX_GATE_EPI (plan_edge_bwd): conv 2^T of the bf16x3 reverse pass applies gate^T in its epilogues -- 0 never, 1 unless debug captures are on or the chunk is small, 2 always
  int gemm_half = 5;               // UMX_GEMM_HALF (gemm_pl, choose_pl): which Q_BF16 products run on half-height tiles, two 4-wave workgroups per CU
  int align = 2;                   // UMX_ALIGN_PLANES (round 6): "aligned planes" -- the leading bf16 plane of both operands of a FORWARD bf16x3 product is
                                   // quantised to its pass group (8 consecutive k of one row), so that stage 1 of the matrix core's adder (a cut TOWARD
                                   // ZERO at 2^-24 of the pass's largest product, i.e. an error that follows the product's sign) has nothing to cut:
                                   // umx_gemm.h qf_align_magic (A, in registers), pack_planes (umx_weights.h: weights, at load).  The remainder goes
                                   // down the planes: elements far below their group's largest keep 16-23 bits instead of 24, with an unbiased error.  2 (default): A's leading plane in the PLAIN products (fc3, conv m = 0) -- the complex m > 0
                                   // products take rotated l >= 1 components whose signs follow the edge direction, nothing coherent to remove -- the
                                   // weights' planes in every forward product (free); 1: A's in every forward product; 0: the plain nearest-bf16 leading
                                   // planes of rounds 4-5.  20 000 atoms, four cases (profiles/r06_energy_bias.txt): 0: -9e-7 ... -1.63e-4 eV, 1: -1.3e-5 ...
                                   // +3.9e-5, 2: +4e-7 ... -5.0e-5; c3 step 517.9 / 526.3 / 523.0 ms
  float odd_sign = -1.0f;          // sign-alternating operand rows (umx_edge.h): -1 = on (default), +1 = off (UMX_ALT_ROWS=0, dev A/B)
  bool node_ctx = false;           // set around the node-level launches (NodeCtx): only those take the float64-accumulating kernel
  bool node_f64_on = true;         // UMX_NODE_F64=0: node-level linears (atom-wise SO(3) linears, scalar MLP, readout and their transposes) on the
                                   // fp32 MFMA instead of the float64-accumulating kernel (k_gemm_f64acc).  Measured (round 3): the fp32-MFMA form of
                                   // these 14 chained GEMMs shifts the energy by a one-signed -2e-8 eV per atom; the double form costs +1 % at c3
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
  std::unique_ptr<Plan> gp_plan;   // the evaluation in progress ...
  std::unique_ptr<WS> gp_ws;       // ... and its workspace view, kept alive between the steps (the plan's closures refer to it)
  size_t gp_at = 0;
  hipStream_t gp_stream = nullptr;
  std::string err;
  // weights
  bool have_weights = false;
  float* d_w = nullptr;          // raw blob data section
  float* d_dw = nullptr;         // derived weights
  double* d_dtab = nullptr;      // derived double tables (per-element fc1 contributions of every radial MLP)
  unsigned short* d_bw = nullptr; // plane copies (bf16 / fp16) of the large SO(2)/radial weights
  std::map<const float*, PlaneCopy> planes;   // fp32 weight ptr -> its plane copy (forward weights and their transposes)
  std::map<std::string, Tensor> wt;
  std::vector<float> h_w;        // host copy of the data section (needed to build derived weights)
  size_t n_w = 0, n_dw = 0, n_bw = 0;   // elements of d_w / d_dw / d_bw (umx_debug_fetch "weights:w|dw|bw")
  // expert form (umx_experts.h): n_experts > 0 -- the 24 SO(2) weights of d_w / d_dw / d_bw are filled by umx_set_expert_coefficients;
  // h_w and d_w then hold the COMPACT data section (every stack takes the room of one expert, table order, 64-byte aligned)
  int n_experts = 0;
  bool experts_merged = false;
  float* d_ex = nullptr;           // the expert stacks
  MergeJob* d_mjobs = nullptr; PackJob* d_pjobs = nullptr; unsigned* d_mx = nullptr;
  int n_mjobs = 0, n_pjobs = 0, merge_blocks = 0, pack_blocks = 0;
  std::vector<const float*> f16_keys;   // fp16 forward planes: PackScales slot -> key of the weight's PlaneCopy (its scale follows the merge)
  hipEvent_t ev_m0 = nullptr, ev_m1 = nullptr;   // around the merge + pack kernels of the last umx_set_expert_coefficients
  bool need_merge() const { return n_experts > 0 && !experts_merged; }
  RadialW rdeg{};
  LayerW lw[NL]{};
  const float *emb_sphere = nullptr, *normw = nullptr, *normb = nullptr, *e0 = nullptr, *e0b = nullptr, *e0T = nullptr,
              *e2 = nullptr, *e2b = nullptr, *e2T = nullptr, *e4 = nullptr, *e4b = nullptr;
  double rmsd = 1.0;
  std::vector<double> elem_refs;
  // model variant, read off the tensors of the blob (umx_load_weights; SURVEY.md section 2.4 K8 / Appendix A.5 list them as possible for UMA-S)
  bool ff_grid = false;            // K8 = GridAtomwise (to-grid -> point-wise SiLU MLP -> from-grid) instead of SpectralAtomwise
  int grid_G = 0;                  // grid points (rows of so3_grid.to_grid_mat / from_grid_mat)
  int ws_grid() const { return ff_grid ? grid_G : 0; }   // what the per-node workspace scales with (0: spectral feed-forward)
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
  // recompute plans (umx_set_recompute / UMX_RECOMPUTE): keep only node-level state across the passes and replay a layer's forward edge
  // pipeline just before its reverse segments -- one activation slot instead of one per layer (carve_acts)
  int recompute = 0;               // 0 off, 1 when the stored plans do not fit the budget, 2 always
  bool rc_active = false;          // the evaluation being planned is a recompute plan (read by ws_bytes and plan_chunk)
  bool arena_rc = false;           // what cap_nodes / cap_edges of the arena were sized for
  bool arena_keep = false;         // the caps were cleared by a change of plan kind: keep an arena that is large enough (prepare_arena)
  int last_recompute = 0;          // 1: the most recent evaluation ran a recompute plan (umx_last_recompute)
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
  double* d_io_pos64 = nullptr; long io64_cap = 0;   // umx_energy_forces_f64: the float64 positions (forces and energies use the buffers above)
  // virial (umx_virial.h): the per-(image, slab) partials of the reduction, outside the arena; where the evaluation at hand writes W
  // (nullptr: no virial was asked for) and its slots per image; the host entry's staging
  double* d_vir_part = nullptr; long vir_cap = 0;
  double* d_vir_wp = nullptr;      // partitioned evaluation: the partitions' own W_p, [VIR_MAX_PARTS][9]
  double* vir_out = nullptr; int vir_slabs = 0;
  double* d_io_w = nullptr; long io_w_cap = 0;
  // stats / profiling / debug
  int64_t last_edges = 0; int32_t last_maxdeg = 0;
  // periodic boundary conditions (umx_periodic.h): the bound cells -- ONE, shared by all images of a call (umx_set_cell), or one per
  // image (umx_set_cells); they persist across umx_set_system
  bool pbc_on = false;
  int pbc[3] = {0, 0, 0};
  std::vector<double> cells;       // [n][9] the bound cells, kept for a rebuild at another cutoff and for the translations of a pinned graph
  bool cells_shared = true;        // cells holds one cell and every image reads it; false: cell k belongs to image k of a call
  std::vector<int> cell_shifts;    // [n] translation-table entries of every cell
  float per_cutoff = 0.f;          // the cutoff the device copies below were built for (rebuilt when umx_set_system changes it)
  Periodic* d_cells = nullptr; long cells_cap = 0;          // [n] what the periodic graph kernels read; `shifts` points into d_shifts_pk
  Lattice64* d_lats = nullptr;                              // [n] their float64 lattices (double positions), grown with d_cells
  float4* d_shifts_pk = nullptr; long shifts_pk_cap = 0;    // the cells' tables, packed: sum of n_shifts entries
  long n_cells() const { return (long)(cells.size() / 9); }
  float* d_wrap = nullptr; long wrap_cap = 0;   // positions wrapped into the cell: the copy the graph kernels read
  double* d_wrap64 = nullptr; long wrap64_cap = 0;   // the same for double positions, wrapped in float64
  int last_shifts = 0;             // lattice translations the most recent evaluation searched (umx_last_graph_shifts; 0: open boundaries)
  // pinned graphs (umx_pin_graph / umx_pin_graphs): the edge sets of the reference images, one of them replayed for every image while
  // pin_on (k_graph_replay).  Persistent buffers, a few bytes per reference edge, the references one behind the other; the host keeps the
  // degrees, so a pinned evaluation plans without reading anything back
  bool pin_on = false;
  int pin_refs = 0;                                // references pinned (1: umx_pin_graph)
  long pin_edges = 0; int pin_maxdeg = 0;          // directed edges of all references together and the largest in-degree among them
  bool pin_pbc_on = false; int pin_pbc[3] = {0, 0, 0};   // the boundary conditions of pin time (other flags unpin)
  std::vector<long> pin_ref_e0;                    // [pin_refs + 1] where a reference's edges start in d_pin_src / dst / tix
  std::vector<int> pin_ref_maxdeg;                 // [pin_refs] largest in-degree of every reference
  std::vector<int> pin_deg;                        // [pin_refs][natoms] in-degrees
  std::vector<long> pin_row;                       // [pin_refs][natoms + 1] their prefix sums within the reference: target-node partitions take contiguous edge ranges
  std::vector<unsigned> pin_codes;                 // the distinct lattice translations of all reference edges, packed as in the table's w
  std::vector<int> pin_assign;                     // umx_pin_assign: the reference of image k; empty = the default (pin_resolve)
  std::vector<int> pin_cur;                        // the reference of every image of the evaluation at hand
  std::vector<int> pin_dev_for;                    // the references d_pin_deg / d_pin_img hold, image by image
  int *d_pin_src = nullptr, *d_pin_dst = nullptr;  // [pin_edges] source / target atom of every edge, rows in the reference's order
  int* d_pin_tix = nullptr;                        // [pin_edges] index into pin_codes
  int* d_pin_wrap = nullptr;                       // [pin_refs][natoms][3] the wrap offsets of pin time
  int* d_pin_deg = nullptr; long pin_deg_imgs = 0; // the assigned references' degrees, image by image, room for pin_deg_imgs images: what k_scan reads for a chunk
  PinImage* d_pin_img = nullptr;                   // [pin_deg_imgs] what the replay reads of every image of a call (grown with d_pin_deg)
  float4* d_pin_shifts = nullptr; long pin_shifts_cap = 0;   // [cells in force][pin_codes] translation vectors (pin_upload_shifts)
  long pin_ref_edges(int r) const { return pin_ref_e0[(size_t)r + 1] - pin_ref_e0[(size_t)r]; }
  const long* pin_row_of(int r) const { return pin_row.data() + (size_t)r * ((size_t)natoms + 1); }
  // Hessian-vector products (umx_hvp, umx_hvp.h): the displaced images, their float32 forces and energies, and the base of every direction
  // on the device; engine-owned, grown like d_io_f.  The host entry's staging: bases and directions in, hv and curv out.
  bool hvp_rows = false;                           // set for the evaluation inside umx_hvp: every image starts at an even row of its chunk (plan_chunks)
  double* d_hvp_x = nullptr; float* d_hvp_f = nullptr; long hvp_cap = 0;       // [images][natoms][3]
  double* d_hvp_e = nullptr; long hvp_img_cap = 0;                            // [images]
  int* d_hvp_bof = nullptr; long hvp_bof_cap = 0; std::vector<int> hvp_bof_dev;   // [directions] base_of, and what the device copy holds
  double* d_hvp_in = nullptr; long hvp_in_cap = 0;                            // [bases + directions][natoms][3]
  double* d_hvp_out = nullptr; long hvp_out_cap = 0;                          // [directions][natoms][3] hv, then [directions] curv
  hipEvent_t ev_bond[4] = {nullptr, nullptr, nullptr, nullptr};   // umx_bond_events: before count | scan | fill | after fill, of the last call
  bool bond_timed = false;                                        // ev_bond hold a finished call (umx_debug_fetch "bond_events:kernel_ms")
  bool may_truncate = true;      // the largest degree of the evaluation being planned reaches max_neigh: k_graph_fill takes its truncating (LDS) form
  bool prof_on = false;
  std::vector<ProfRec> prof;
  size_t prof_used = 0;
  bool dbg_on = false;
  std::map<std::string, std::vector<char>> dbg;
  std::string gemm_log;          // umx_debug_fetch "gemm:launches": one line per gemm_pl launch of the last chunk, kept while dbg_on
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

// ---- growing a device buffer ---------------------------------------------------------------------
// The buffers that share one capacity counter are replaced together: drain the streams that may still be using the old ones, free them,
// clear pointers and capacity (a failed hipMalloc below must not leave a dangling pointer behind), allocate, record the capacity.
struct DevBuf {
  void** p; size_t bytes;
  template <class T> DevBuf(T*& ptr, size_t count) : p(reinterpret_cast<void**>(&ptr)), bytes(count * sizeof(T)) {}
};
template <class Cap>
int grow(umx_engine* eng, Cap& cap, Cap new_cap, std::initializer_list<hipStream_t> drain, std::initializer_list<DevBuf> bufs) {
  for (hipStream_t s : drain) HIPCHK(eng, hipStreamSynchronize(s));
  for (const DevBuf& b : bufs) if (*b.p) HIPCHK(eng, hipFree(*b.p));
  for (const DevBuf& b : bufs) *b.p = nullptr;
  cap = 0;
  for (const DevBuf& b : bufs) HIPCHK(eng, hipMalloc(b.p, b.bytes));
  cap = new_cap;
  return UMX_OK;
}
// edges a growing workspace is sized for when a chunk needs e: 2 % + 1024 on top, so that a slightly denser batch does not re-allocate
inline long grown_edges(long e) { return e + e / 50 + 1024; }
// the workspace arena: the second lane may still be running in it
int grow_arena(umx_engine* eng, hipStream_t s, size_t bytes) {
  CHK(grow(eng, eng->arena_bytes, bytes, {s, eng->stream2}, {DevBuf(eng->arena, bytes)}));
  ++eng->arena_allocs;
  return UMX_OK;
}

// ---- debug captures ------------------------------------------------------------------------------
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

}  // namespace
