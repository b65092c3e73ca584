// umx_api.hip -- the C ABI (include/umx.h) of the UMA-S engine for gfx950, and the one translation unit of the library.
//
// One engine = one GPU.  umx_energy_forces[_dev] evaluates K images of one system as a block
// diagonal graph: K1 radius graph -> K2 frames -> K4/K5 node init + edge-degree embedding ->
// 4 x (K6 norm, K7 edgewise SO(2) message passing, K8 atom-wise FF) -> K9 readout -> K10 analytic
// reverse pass (no autograd) -> K11 normaliser/element references.  Images are processed in
// chunks sized to the HBM workspace budget; activations needed by the reverse pass stay resident
// in HBM (the 288 GB part makes store-not-recompute the cheaper choice).
//
// The host code by concern (in the order of their dependences):
#include "umx_engine.h"      // engine state, precision descriptor, WS / Plan types, error and buffer helpers
#include "umx_launch.h"      // profiling bracket, GEMM launchers, the plane-GEMM dispatch table
#include "umx_workspace.h"   // carving the workspace arena
#include "umx_periodic.h"    // host side of the graph stage: the bound cells, the wrapped copy, the dispatcher and the graph-kernel launchers
#include "umx_virial.h"      // the strain derivative of every image: the two reduction kernels behind k_force_edge and their launcher
#include "umx_plan.h"        // the launch plan of one chunk, its executors, and one evaluation as its phases
#include "umx_hvp.h"         // Hessian-vector products: displace, difference and curvature kernels around one batched evaluation
#include "umx_weights.h"     // the weight loader
#include "umx_experts.h"     // expert-form weights: the Mixture-of-Linear-Experts merge and its plane copies on the device
#include "umx_bonds.h"       // bond-change events of many pairs of geometries: count, scan and fill kernels and their launcher
#include "umx_rowblocks.h"   // float64 row-block kernels of the Hessian-free solvers on umx_hvp: gram, combine, scale; dot, axpby, absmax

// ================================================================================================
//                                           C ABI
// ================================================================================================
#define NOT_MERGED "expert-form weights are loaded but not merged: call umx_set_expert_coefficients first (then umx_set_system)"

// ---- the evaluation entries, once for float and once for double positions (umx_energy_forces_f64[_dev]) ---------------------------
namespace {
// the device-pointer entries, for float or double positions
int energy_forces_dev_impl(umx_engine* eng, int n_images, const PosPtr d_pos, double* d_energy, float* d_forces, double* d_virial, void* hip_stream) {
  if (!eng) return UMX_ERR_ARG;
  if (eng->need_merge()) return fail(eng, UMX_ERR_ARG, "umx_energy_forces: " NOT_MERGED);
  if (!eng->have_system) return fail(eng, UMX_ERR_ARG, "umx_energy_forces: bind a system first (umx_set_system)");
  if (n_images <= 0 || !(d_pos.f || d_pos.d) || !d_energy) return fail(eng, UMX_ERR_ARG, "umx_energy_forces: bad arguments");
  if (d_virial && !d_forces) return fail(eng, UMX_ERR_ARG, "umx_energy_forces_virial: the virial comes out of the reverse pass: ask for the forces too");
  if (eng->gp_plan) return fail(eng, UMX_ERR_ARG, "umx_energy_forces: a graph-parallel evaluation is in progress (finish it with umx_gp_step)");
  CHK(periodic_check_images(eng, n_images, "umx_energy_forces"));
  HIPCHK(eng, hipSetDevice(eng->dev));
  // NULL = the legacy default stream (hipStream_t 0): the work is then ordered after everything the caller has enqueued on
  // the default stream (the producer of d_pos) and before whatever it enqueues next (the consumer of d_energy / d_forces),
  // exactly as with an explicit stream.  The engine's private non-blocking stream is never used for caller-owned buffers.
  return energy_forces_on(eng, static_cast<hipStream_t>(hip_stream), n_images, d_pos, d_energy, d_forces, d_virial);
}

// the host-pointer entries, for float or double positions: P* pos is staged in the device buffer of its own type
template <typename P>
int energy_forces_host_impl(umx_engine* eng, int n_images, const P* pos, double* energy, float* forces, double* virial) {
  if (!eng) return UMX_ERR_ARG;
  if (eng->need_merge()) return fail(eng, UMX_ERR_ARG, "umx_energy_forces: " NOT_MERGED);
  if (!eng->have_system) return fail(eng, UMX_ERR_ARG, "umx_energy_forces: bind a system first (umx_set_system)");
  if (n_images <= 0 || !pos || !energy) return fail(eng, UMX_ERR_ARG, "umx_energy_forces: bad arguments");
  if (virial && !forces) return fail(eng, UMX_ERR_ARG, "umx_energy_forces_virial: the virial comes out of the reverse pass: ask for the forces too");
  if (eng->gp_plan) return fail(eng, UMX_ERR_ARG, "umx_energy_forces: a graph-parallel evaluation is in progress (finish it with umx_gp_step)");
  CHK(periodic_check_images(eng, n_images, "umx_energy_forces"));
  HIPCHK(eng, hipSetDevice(eng->dev));
  const long nt = (long)n_images * eng->natoms;
  if (eng->io_cap < nt) CHK(grow(eng, eng->io_cap, nt, {eng->stream}, {DevBuf(eng->d_io_pos, nt * 3), DevBuf(eng->d_io_f, nt * 3)}));
  if (eng->io_img_cap < n_images) CHK(grow(eng, eng->io_img_cap, (long)n_images, {eng->stream}, {DevBuf(eng->d_io_e, n_images)}));
  if (virial && eng->io_w_cap < n_images) CHK(grow(eng, eng->io_w_cap, (long)n_images, {eng->stream}, {DevBuf(eng->d_io_w, (size_t)n_images * 9)}));
  P* d_stage;
  if constexpr (std::is_same_v<P, double>) {          // the float64 positions' own staging, grown as the float one above
    if (eng->io64_cap < nt) CHK(grow(eng, eng->io64_cap, nt, {eng->stream}, {DevBuf(eng->d_io_pos64, nt * 3)}));
    d_stage = eng->d_io_pos64;
  } else d_stage = eng->d_io_pos;
  for (long i = 0; i < nt * 3; ++i)         // a NaN coordinate would silently drop its atom from the radius graph (every comparison false)
    if (!std::isfinite(pos[i])) return fail(eng, UMX_ERR_ARG, "umx_energy_forces: non-finite position (image " + std::to_string(i / ((long)eng->natoms * 3)) + ")");
  HIPCHK(eng, hipMemcpyAsync(d_stage, pos, nt * 3 * sizeof(P), hipMemcpyHostToDevice, eng->stream));
  CHK(energy_forces_on(eng, eng->stream, n_images, PosPtr(d_stage), eng->d_io_e, forces ? eng->d_io_f : nullptr, virial ? eng->d_io_w : nullptr));
  HIPCHK(eng, hipMemcpyAsync(energy, eng->d_io_e, (size_t)n_images * sizeof(double), hipMemcpyDeviceToHost, eng->stream));
  if (forces) HIPCHK(eng, hipMemcpyAsync(forces, eng->d_io_f, nt * 3 * sizeof(float), hipMemcpyDeviceToHost, eng->stream));
  if (virial) HIPCHK(eng, hipMemcpyAsync(virial, eng->d_io_w, (size_t)n_images * 9 * sizeof(double), hipMemcpyDeviceToHost, eng->stream));
  HIPCHK(eng, hipStreamSynchronize(eng->stream));
  for (int k = 0; k < n_images; ++k)
    if (!std::isfinite(energy[k])) {
      (void)hipMemset(eng->d_flags, 0, sizeof(int));         // reported right here: do not fail the NEXT call for it as well
      return fail(eng, UMX_ERR_RANGE, "image " + std::to_string(k) + ": non-finite energy" +
                  (eng->prec.fwd_f16() ? " (an activation beyond the fp16 operand range of UMX_PRECISION=split: try split-bf16, bf16x3 or fp32)"
                                      : " (an overflow in float32)"));
    }
  return UMX_OK;
}

// ---- pinned graph (umx_pin_graph[_f64]) -----------------------------------------------------------------------------------------------
void pin_clear(umx_engine* eng) { eng->pin_on = false; }     // (the buffers stay: the next pin replaces them, umx_destroy frees them)

// umx_set_cell / umx_set_cells under a pin: the pbc flags of pin time keep it -- the pinned edges' translations are formed anew for the
// cell(s) now in force -- any other flags unpin
int pin_after_cell(umx_engine* eng) {
  if (!eng->pin_on) return UMX_OK;
  bool same = eng->pbc_on == eng->pin_pbc_on;
  for (int k = 0; k < 3 && same && eng->pbc_on; ++k) same = eng->pbc[k] == eng->pin_pbc[k];
  if (!same) { pin_clear(eng); return UMX_OK; }
  const int st = pin_upload_shifts(eng, eng->pin_codes, &eng->d_pin_shifts, &eng->pin_shifts_cap);
  if (st != UMX_OK) pin_clear(eng);
  return st;
}

// Build the graphs of R reference images exactly as an evaluation of that batch does -- wrapped copy, degree pass, scan, fill -- with the
// translation of every edge as one more output of the fill, and keep their structure.  Everything that can fail happens on new buffers:
// a failed pin leaves the previous state.  `who`: the entry (umx_pin_graph is R = 1).
template <typename P>
int pin_graphs_impl(umx_engine* eng, const char* who, int R, const P* pos) {
  if (!eng) return UMX_ERR_ARG;
  const std::string me(who);
  if (eng->need_merge()) return fail(eng, UMX_ERR_ARG, me + ": " NOT_MERGED);
  if (!eng->have_system) return fail(eng, UMX_ERR_ARG, me + ": bind a system first (umx_set_system)");
  if (!pos || R < 1) return fail(eng, UMX_ERR_ARG, me + ": bad arguments");
  if (eng->gp_plan) return fail(eng, UMX_ERR_ARG, me + ": a graph-parallel evaluation is in progress (finish it with umx_gp_step)");
  if (R > 1 && eng->pbc_on && !eng->cells_shared)
    return fail(eng, UMX_ERR_ARG, me + ": per-image cells are bound (umx_set_cells): several references are built open or in the one cell of umx_set_cell");
  CHK(periodic_check_images(eng, R, who));
  const int N = eng->natoms;
  const long NT = (long)R * N;
  for (long i = 0; i < NT * 3; ++i)
    if (!std::isfinite(pos[i])) return fail(eng, UMX_ERR_ARG, me + ": non-finite position (reference " + std::to_string(i / ((long)N * 3)) + ")");
  HIPCHK(eng, hipSetDevice(eng->dev));
  hipStream_t s = eng->stream;
  HIPCHK(eng, hipStreamSynchronize(s));                              // no evaluation may still be replaying the graphs these replace
  if (eng->ran_on_caller) HIPCHK(eng, hipEventSynchronize(eng->ev_done));
  if (eng->io_cap < NT) CHK(grow(eng, eng->io_cap, NT, {s}, {DevBuf(eng->d_io_pos, (size_t)NT * 3), DevBuf(eng->d_io_f, (size_t)NT * 3)}));
  P* d_stage;
  if constexpr (std::is_same_v<P, double>) {
    if (eng->io64_cap < NT) CHK(grow(eng, eng->io64_cap, NT, {s}, {DevBuf(eng->d_io_pos64, (size_t)NT * 3)}));
    d_stage = eng->d_io_pos64;
  } else d_stage = eng->d_io_pos;
  HIPCHK(eng, hipMemcpyAsync(d_stage, pos, (size_t)NT * 3 * sizeof(P), hipMemcpyHostToDevice, s));
  // the ordinary graph of the batch: the pin in force (if any) stands aside, and what the engine reports of its last evaluation stays
  struct Keep {
    umx_engine* e; bool pin; int64_t edges; int32_t maxdeg; int shifts; bool trunc;
    ~Keep() { e->pin_on = pin; e->last_edges = edges; e->last_maxdeg = maxdeg; e->last_shifts = shifts; e->may_truncate = trunc; }
  } keep{eng, eng->pin_on, eng->last_edges, eng->last_maxdeg, eng->last_shifts, eng->may_truncate};
  eng->pin_on = false;
  PosPtr dp(d_stage);
  CHK(periodic_prepare(eng, s, R, &dp));
  ImageEdges ie;
  CHK(degree_pass(eng, s, R, dp, ie));
  const long E = ie.etot;
  const bool trunc = eng->may_truncate;
  // new buffers: source, target, translation (first the packed triple, then its index), wrap offsets; scratch: row_ptr, edge vectors
  int *n_src = nullptr, *n_dst = nullptr, *n_tix = nullptr, *n_wrap = nullptr, *t_row = nullptr;
  float* t_evec = nullptr;
  float4* n_shifts = nullptr; long n_shifts_cap = 0;
  struct Bufs { void** p[7]; bool drop = true; ~Bufs() { if (drop) for (void** q : p) if (*q) (void)hipFree(*q); } }
      bufs{{(void**)&n_src, (void**)&n_dst, (void**)&n_tix, (void**)&n_wrap, (void**)&t_row, (void**)&t_evec, (void**)&n_shifts}};
  const size_t eb = (size_t)std::max(E, 1L);
  HIPCHK(eng, hipMalloc(&n_src, eb * sizeof(int)));
  HIPCHK(eng, hipMalloc(&n_dst, eb * sizeof(int)));
  HIPCHK(eng, hipMalloc(&n_tix, eb * sizeof(int)));
  HIPCHK(eng, hipMalloc(&n_wrap, (size_t)NT * 3 * sizeof(int)));
  HIPCHK(eng, hipMalloc(&t_row, ((size_t)NT + 3) * sizeof(int)));
  HIPCHK(eng, hipMalloc(&t_evec, eb * 4 * sizeof(float)));
  HIPCHK(eng, hipMemsetAsync(n_tix, 0, eb * sizeof(int), s));
  HIPCHK(eng, hipMemsetAsync(n_wrap, 0, (size_t)NT * 3 * sizeof(int), s));
  hipLaunchKernelGGL(k_scan, dim3(1), dim3(1024), 0, s, eng->d_deg_all, NT, t_row, t_row + NT + 1);
  launch_graph_fill(eng, s, trunc, dp, NT, eng->d_cand_all, t_row, n_src, n_dst, t_evec, 0, NT, 0, n_tix);
  if (R > 1 && E > 0) hipLaunchKernelGGL(k_pin_local, dim3(nblk(E, 256)), dim3(256), 0, s, n_src, n_dst, E, N);
  launch_wrap_index(eng, s, PosPtr(d_stage), R, n_wrap);
  HIPCHK(eng, hipGetLastError());
  std::vector<int> deg((size_t)NT), code(eb);
  HIPCHK(eng, hipMemcpyAsync(deg.data(), eng->d_deg_all, (size_t)NT * sizeof(int), hipMemcpyDeviceToHost, s));
  if (E > 0) HIPCHK(eng, hipMemcpyAsync(code.data(), n_tix, (size_t)E * sizeof(int), hipMemcpyDeviceToHost, s));
  HIPCHK(eng, hipStreamSynchronize(s));
  // every reference: its rows' prefix sums, its largest in-degree, and where its edges start among all of them
  std::vector<long> row((size_t)R * (N + 1), 0), e0((size_t)R + 1, 0);
  std::vector<int> ref_maxdeg((size_t)R, 0);
  int maxdeg = 0;
  for (int r = 0; r < R; ++r) {
    long* rw = row.data() + (size_t)r * (N + 1);
    for (int i = 0; i < N; ++i) { rw[i + 1] = rw[i] + deg[(size_t)r * N + i]; ref_maxdeg[r] = std::max(ref_maxdeg[r], deg[(size_t)r * N + i]); }
    if (rw[N] != ie.per_image[r]) return fail(eng, UMX_ERR_HIP, me + ": the degrees and the edge count of reference " + std::to_string(r) + " disagree");
    e0[(size_t)r + 1] = e0[r] + rw[N];
    maxdeg = std::max(maxdeg, ref_maxdeg[r]);
  }
  // the distinct translations, in ascending order of their packed triple, and every edge's index among them
  std::vector<unsigned> codes;
  if (eng->pbc_on && E > 0) {
    const std::set<unsigned> uniq(code.begin(), code.begin() + E);
    codes.assign(uniq.begin(), uniq.end());
    for (long e = 0; e < E; ++e) code[e] = (int)(std::lower_bound(codes.begin(), codes.end(), (unsigned)code[e]) - codes.begin());
    HIPCHK(eng, hipMemcpy(n_tix, code.data(), (size_t)E * sizeof(int), hipMemcpyHostToDevice));
  }
  CHK(pin_upload_shifts(eng, codes, &n_shifts, &n_shifts_cap));
  // nothing below fails: the new graphs replace the old ones
  bufs.drop = false;
  void* old[] = {eng->d_pin_src, eng->d_pin_dst, eng->d_pin_tix, eng->d_pin_wrap, eng->d_pin_shifts, eng->d_pin_deg, eng->d_pin_img, t_row, t_evec};
  for (void* q : old) if (q) (void)hipFree(q);
  eng->d_pin_src = n_src; eng->d_pin_dst = n_dst; eng->d_pin_tix = n_tix; eng->d_pin_wrap = n_wrap;
  eng->d_pin_shifts = n_shifts; eng->pin_shifts_cap = n_shifts_cap;
  eng->d_pin_deg = nullptr; eng->d_pin_img = nullptr; eng->pin_deg_imgs = 0;
  eng->pin_dev_for.clear(); eng->pin_cur.clear();
  eng->pin_assign.clear();                                           // pinning again: the default assignment
  eng->pin_refs = R;
  eng->pin_deg = std::move(deg); eng->pin_row = std::move(row); eng->pin_codes = std::move(codes);
  eng->pin_ref_e0 = std::move(e0); eng->pin_ref_maxdeg = std::move(ref_maxdeg);
  eng->pin_edges = E; eng->pin_maxdeg = maxdeg;
  eng->pin_pbc_on = eng->pbc_on;
  for (int k = 0; k < 3; ++k) eng->pin_pbc[k] = eng->pbc_on ? eng->pbc[k] : 0;
  keep.pin = true;
  return UMX_OK;
}

// ---- Hessian-vector products (umx_hvp[_dev]; kernels and launchers in umx_hvp.h) -------------------------------------------------------
// what both entries refuse before anything runs; base_of is a HOST pointer in both
int hvp_check(umx_engine* eng, int R, const void* base, int M, const void* dir, const int32_t* base_of, double step, int flags, const void* hv,
              const void* e0, const void* f0) {
  if (!eng) return UMX_ERR_ARG;
  if (eng->need_merge()) return fail(eng, UMX_ERR_ARG, "umx_hvp: " NOT_MERGED);
  if (!eng->have_system) return fail(eng, UMX_ERR_ARG, "umx_hvp: bind a system first (umx_set_system)");
  if (R < 1 || M < 1 || !base || !dir || !hv || (flags & ~(HVP_FORWARD | HVP_NO_PIN | HVP_GIVEN_F0))) return fail(eng, UMX_ERR_ARG, "umx_hvp: bad arguments");
  if ((flags & HVP_GIVEN_F0) && (!(flags & HVP_FORWARD) || !f0 || e0))
    return fail(eng, UMX_ERR_ARG, "umx_hvp: flags bit 2 hands the bases' forces IN through f0: the forward scheme (bit 0), f0 given, e0 NULL");
  if (eng->gp_plan) return fail(eng, UMX_ERR_ARG, "umx_hvp: a graph-parallel evaluation is in progress (finish it with umx_gp_step)");
  if (!std::isfinite(step) || step <= 0.0) return fail(eng, UMX_ERR_ARG, "umx_hvp: the step must be finite and positive");
  if (R > 1 && !base_of) return fail(eng, UMX_ERR_ARG, "umx_hvp: base_of may be NULL only with one base, " + std::to_string(R) + " were given");
  for (int m = 0; base_of && m < M; ++m)
    if (base_of[m] < 0 || base_of[m] >= R)
      return fail(eng, UMX_ERR_ARG, "umx_hvp: direction " + std::to_string(m) + " names base " + std::to_string(base_of[m]) + ", but " + std::to_string(R) + " were given");
  // (the rule of umx_pin_graphs for several bases; with one base the images +v and -v would each take another cell of the list)
  if (eng->pbc_on && !eng->cells_shared)
    return fail(eng, UMX_ERR_ARG, "umx_hvp: per-image cells are bound (umx_set_cells): the displaced images of a base share ONE cell -- the bases are "
                "evaluated open or in the one cell of umx_set_cell");
  if (!(flags & HVP_FORWARD) && (e0 || f0))
    return fail(eng, UMX_ERR_ARG, "umx_hvp: e0 and f0 are the bases' own energies and forces, which only the forward scheme evaluates (flags bit 0)");
  if ((flags & HVP_NO_PIN) && eng->pin_on)
    return fail(eng, UMX_ERR_ARG, "umx_hvp: flags bit 1 asks every image to build its own graph, but a graph is pinned: call umx_unpin_graph first");
  if (eng->pin_on && eng->pin_refs != 1 && eng->pin_refs != R)
    return fail(eng, UMX_ERR_ARG, "umx_hvp: " + std::to_string(eng->pin_refs) + " graphs are pinned and " + std::to_string(R) + " bases were given: "
                "the entry replays one pinned reference for all bases, or one per base");
  return periodic_check_images(eng, hvp_images(R, M, flags), "umx_hvp");
}

// The call on stream s with device pointers (h_base: the bases on the host as well, or nullptr -- then they are read back when the entry
// has to pin them itself).  Whatever the way out, the caller's assignment is back in force and a pin of the entry's own is gone.
int hvp_run(umx_engine* eng, hipStream_t s, int R, const double* d_base, const double* h_base, int M, const double* d_dir, const int32_t* base_of,
            double step, int flags, double* d_hv, double* d_curv, double* d_e0, float* d_f0) {
  const int N = eng->natoms;
  const long K = hvp_images(R, M, flags);
  const bool fwd = (flags & HVP_FORWARD) != 0;
  struct Restore {
    umx_engine* e; std::vector<int> assign; bool own_pin = false;
    ~Restore() { e->hvp_rows = false; if (own_pin) pin_clear(e); e->pin_assign = std::move(assign); }
  } restore{eng, eng->pin_assign};
  if (!(flags & HVP_NO_PIN) && !eng->pin_on) {
    std::vector<double> back;
    if (!h_base) {
      back.resize((size_t)R * N * 3);
      HIPCHK(eng, hipMemcpyAsync(back.data(), d_base, back.size() * sizeof(double), hipMemcpyDeviceToHost, s));
      HIPCHK(eng, hipStreamSynchronize(s));
      h_base = back.data();
    }
    CHK(pin_graphs_impl<double>(eng, "umx_hvp", R, h_base));
    restore.assign.clear();
    restore.own_pin = true;
  }
  if (eng->pin_on) {                    // image k replays the reference of its base (one reference: all of them that one)
    eng->pin_assign.clear();
    if (eng->pin_refs > 1) {
      eng->pin_assign.resize((size_t)K);
      const long nb = hvp_bases(R, flags);
      for (long k = 0; k < K; ++k) eng->pin_assign[k] = fwd ? (k < nb ? (int)k : base_of[k - nb]) : base_of[k >> 1];
    }
  }
  eng->hvp_rows = true;
  const int* d_bof = nullptr;
  CHK(hvp_prepare(eng, s, K, M, R > 1 ? base_of : nullptr, &d_bof));
  CHK(hvp_displace(eng, s, R, d_base, M, d_dir, d_bof, step, flags));
  CHK(energy_forces_on(eng, s, (int)K, PosPtr(static_cast<const double*>(eng->d_hvp_x)), eng->d_hvp_e, eng->d_hvp_f));
  CHK(hvp_combine(eng, s, R, M, d_dir, d_bof, step, flags, d_f0, d_hv, d_curv));
  if (d_e0) HIPCHK(eng, hipMemcpyAsync(d_e0, eng->d_hvp_e, (size_t)R * sizeof(double), hipMemcpyDeviceToDevice, s));
  if (d_f0 && !(flags & HVP_GIVEN_F0)) HIPCHK(eng, hipMemcpyAsync(d_f0, eng->d_hvp_f, (size_t)R * N * 3 * sizeof(float), hipMemcpyDeviceToDevice, s));
  HIPCHK(eng, hipEventRecord(eng->ev_done, s));
  return UMX_OK;
}
}  // namespace

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
  if (const char* ev = std::getenv("UMX_RECOMPUTE")) e->recompute = std::max(0, std::min(2, std::atoi(ev)));
  if (const char* ev = std::getenv("UMX_WS_GB")) e->ws_cap_default = (size_t)std::max(0L, std::atol(ev)) << 30;
  if (const char* ev = std::getenv("UMX_WS_EAGER")) e->ws_eager = std::atoi(ev) != 0;
  if (const char* ev = std::getenv("UMX_WS_SOFT_EDGES")) e->ws_soft_edges = std::max(1L, std::atol(ev));
  if (const char* ev = std::getenv("UMX_NODE_F64")) e->node_f64_on = std::atoi(ev) != 0;
  if (const char* ev = std::getenv("UMX_GRID_F64")) e->grid_f64 = std::atoi(ev) != 0;
  if (const char* ev = std::getenv("UMX_ALT_ROWS")) e->odd_sign = std::atoi(ev) != 0 ? -1.0f : 1.0f;
  if (const char* ev = std::getenv("UMX_LOW_SEP")) e->low_sep = std::atoi(ev);
  if (const char* ev = std::getenv("UMX_GEMM_HALF")) e->gemm_half = std::atoi(ev);
  if (const char* ev = std::getenv("UMX_GATE_EPI")) e->gate_epi = std::max(0, std::min(2, std::atoi(ev)));
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


int umx_destroy(umx_engine* eng) {
  if (!eng) return UMX_OK;
  gp_clear(eng);
  (void)hipSetDevice(eng->dev);
  (void)hipStreamSynchronize(eng->stream);
  for (auto& r : eng->prof) { (void)hipEventDestroy(r.a); (void)hipEventDestroy(r.b); }
  void* ptrs[] = {eng->d_w, eng->d_dw, eng->d_bw, eng->d_gmu, eng->d_z, eng->d_sysemb, eng->arena, eng->d_deg_all, eng->d_cand_all, eng->d_img_edges, eng->d_io_pos, eng->d_io_e, eng->d_io_f, eng->d_flags, eng->d_dtab, eng->d_part_deg, eng->d_part_f, eng->d_ex, eng->d_mjobs, eng->d_pjobs, eng->d_mx, eng->d_cells, eng->d_shifts_pk, eng->d_wrap, eng->d_wrap64, eng->d_lats, eng->d_io_pos64, eng->d_vir_part, eng->d_vir_wp, eng->d_io_w, eng->d_pin_src, eng->d_pin_dst, eng->d_pin_tix, eng->d_pin_wrap, eng->d_pin_deg, eng->d_pin_img, eng->d_pin_shifts, eng->d_hvp_x, eng->d_hvp_f, eng->d_hvp_e, eng->d_hvp_bof, eng->d_hvp_in, eng->d_hvp_out};
  for (void* p : ptrs) if (p) (void)hipFree(p);
  (void)hipStreamSynchronize(eng->stream2);
  (void)hipEventDestroy(eng->ev_fork); (void)hipEventDestroy(eng->ev_join);
  (void)hipEventDestroy(eng->ev_tok[0]); (void)hipEventDestroy(eng->ev_tok[1]);
  if (eng->ev_done) (void)hipEventDestroy(eng->ev_done);
  if (eng->ev_m0) { (void)hipEventDestroy(eng->ev_m0); (void)hipEventDestroy(eng->ev_m1); }
  for (hipEvent_t e : eng->ev_bond) if (e) (void)hipEventDestroy(e);
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

int umx_load_weights(umx_engine* eng, const void* blob, size_t nbytes) {
  if (!eng || !blob) return UMX_ERR_ARG;
  return load_weights_impl(eng, blob, nbytes);
}

int umx_set_expert_coefficients(umx_engine* eng, int n, const double* alpha) {
  if (!eng) return UMX_ERR_ARG;
  return set_expert_coefficients_impl(eng, n, alpha);
}

int umx_expert_count(const umx_engine* eng) { return eng && eng->have_weights ? eng->n_experts : 0; }

const char* umx_precision_mode(const umx_engine* eng) {
  if (!eng || !eng->have_weights) return "";
  return eng->prec.name;
}

const char* umx_model_variant(const umx_engine* eng) {
  if (!eng || !eng->have_weights) return "";
  return eng->variant.c_str();
}

int umx_set_system(umx_engine* eng, int n_atoms, const int32_t* z, int charge, int spin, int task_index, float radius, int max_neigh) {
  if (!eng) return UMX_ERR_ARG;
  if (!eng->have_weights) return fail(eng, UMX_ERR_ARG, "umx_set_system: load weights first");
  if (eng->need_merge()) return fail(eng, UMX_ERR_ARG, "umx_set_system: " NOT_MERGED);
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
  pin_clear(eng);                                         // a pinned graph belongs to the system it was built for
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
    // (bit 1 can be left only by the replay of a pinned graph: every other evaluation reads it behind its own degree pass)
    return fail(eng, UMX_ERR_RANGE, std::string("a device-pointer evaluation produced a non-finite energy") +
                ((flag & 2) ? " (a non-finite position reached an evaluation on the pinned graph)" : eng->prec.range_hint()));
  }
  return UMX_OK;
}

int umx_energy_forces_dev(umx_engine* eng, int n_images, const float* d_pos, double* d_energy, float* d_forces, void* hip_stream) {
  return umx_energy_forces_virial_dev(eng, n_images, d_pos, d_energy, d_forces, nullptr, hip_stream);
}

int umx_energy_forces_virial_dev(umx_engine* eng, int n_images, const float* d_pos, double* d_energy, float* d_forces, double* d_virial, void* hip_stream) {
  return energy_forces_dev_impl(eng, n_images, PosPtr(d_pos), d_energy, d_forces, d_virial, hip_stream);
}

int umx_energy_forces_f64_dev(umx_engine* eng, int n_images, const double* d_pos, double* d_energy, float* d_forces, double* d_virial, void* hip_stream) {
  return energy_forces_dev_impl(eng, n_images, PosPtr(d_pos), d_energy, d_forces, d_virial, hip_stream);
}

int umx_gp_begin(umx_engine* eng, const float* d_pos, int node_lo, int node_hi, double* d_energy, float* d_forces, void* hip_stream) {
  return umx_gp_begin_virial(eng, d_pos, node_lo, node_hi, d_energy, d_forces, nullptr, hip_stream);
}

// d_virial: this rank's share of W (nine float64), or nullptr -- then the plan is umx_gp_begin's, launch for launch
int umx_gp_begin_virial(umx_engine* eng, const float* d_pos, int node_lo, int node_hi, double* d_energy, float* d_forces, double* d_virial, void* hip_stream) {
  if (!eng) return UMX_ERR_ARG;
  if (eng->need_merge()) return fail(eng, UMX_ERR_ARG, "umx_gp_begin: " NOT_MERGED);
  if (!eng->have_system) return fail(eng, UMX_ERR_ARG, "umx_gp_begin: bind a system first (umx_set_system)");
  if (!d_pos || !d_energy || !d_forces) return fail(eng, UMX_ERR_ARG, "umx_gp_begin: bad arguments (forces are part of the exchange)");
  if (node_lo < 0 || node_hi > eng->natoms || node_lo > node_hi) return fail(eng, UMX_ERR_ARG, "umx_gp_begin: node range outside [0, n_atoms]");
  if (eng->recompute == 2)
    return fail(eng, UMX_ERR_ARG, "umx_gp_begin: recompute mode 2 (umx_set_recompute / UMX_RECOMPUTE=2) is a one-GPU plan; the multi-GPU graph-parallel mode "
                                  "keeps every rank's activations stored: set mode 0 or 1 on the engines that take part");
  if (eng->pin_on)
    return fail(eng, UMX_ERR_ARG, "umx_gp_begin: a graph is pinned (umx_pin_graph) and the graph-parallel entries build their own: call umx_unpin_graph first");
  if (eng->pbc_on && !eng->cells_shared && eng->n_cells() > 1)
    return fail(eng, UMX_ERR_ARG, "umx_gp_begin: one image, but umx_set_cells bound cells for " + std::to_string(eng->n_cells()) +
                                  " images: the graph-parallel mode takes per-image cells only when exactly one is bound");
  if (eng->gp_plan) gp_clear(eng);                       // an abandoned evaluation
  HIPCHK(eng, hipSetDevice(eng->dev));
  eng->gp = true; eng->gp_lo = node_lo; eng->gp_hi = node_hi;
  const int st = energy_forces_on(eng, static_cast<hipStream_t>(hip_stream), 1, d_pos, d_energy, d_forces, d_virial);
  if (st != UMX_OK) gp_clear(eng);
  return st;
}

int umx_gp_step(umx_engine* eng, float** d_buf, size_t* count, int* done) {
  if (!eng || !d_buf || !count || !done) return UMX_ERR_ARG;
  if (!eng->gp_plan) return fail(eng, UMX_ERR_ARG, "umx_gp_step: no graph-parallel evaluation in progress (umx_gp_begin)");
  HIPCHK(eng, hipSetDevice(eng->dev));
  hipStream_t own = eng->stream;
  eng->stream = eng->gp_stream;
  *d_buf = nullptr; *count = 0; *done = 0;
  const Seg* stop = nullptr;
  int st = eng->gp_plan->run_to_sync(eng->gp_at, &stop);
  eng->stream = own;
  if (stop) { *d_buf = stop->sync_buf; *count = stop->sync_count; return UMX_OK; }     // an exchange point: the caller sums, then steps again
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
  return umx_energy_forces_virial(eng, n_images, pos, energy, forces, nullptr);
}

int umx_energy_forces_virial(umx_engine* eng, int n_images, const float* pos, double* energy, float* forces, double* virial) {
  return energy_forces_host_impl(eng, n_images, pos, energy, forces, virial);
}

int umx_energy_forces_f64(umx_engine* eng, int n_images, const double* pos, double* energy, float* forces, double* virial) {
  return energy_forces_host_impl(eng, n_images, pos, energy, forces, virial);
}

int umx_set_precision(umx_engine* eng, const char* mode) {
  if (!eng) return UMX_ERR_ARG;
  const std::string m = mode ? mode : "";
  if (!m.empty() && !resolve_precision(m, nullptr))
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

int umx_set_cell(umx_engine* eng, const double cell[9], const int pbc[3]) {
  if (!eng) return UMX_ERR_ARG;
  if (eng->gp_plan) return fail(eng, UMX_ERR_ARG, "umx_set_cell: a graph-parallel evaluation is in progress (finish it with umx_gp_step)");
  CHK(set_cells_impl(eng, "umx_set_cell", true, 1, cell, pbc));
  return pin_after_cell(eng);
}
int umx_set_cells(umx_engine* eng, int n_images, const double* cells, const int pbc[3]) {
  if (!eng) return UMX_ERR_ARG;
  if (eng->gp_plan) return fail(eng, UMX_ERR_ARG, "umx_set_cells: a graph-parallel evaluation is in progress (finish it with umx_gp_step)");
  CHK(set_cells_impl(eng, "umx_set_cells", false, n_images, cells, pbc));
  return pin_after_cell(eng);
}
int umx_last_graph_shifts(const umx_engine* eng) { return eng ? eng->last_shifts : 0; }

int umx_pin_graph(umx_engine* eng, const float* pos_ang) { return pin_graphs_impl(eng, "umx_pin_graph", 1, pos_ang); }
int umx_pin_graph_f64(umx_engine* eng, const double* pos_ang) { return pin_graphs_impl(eng, "umx_pin_graph", 1, pos_ang); }
int umx_pin_graphs(umx_engine* eng, int n_refs, const float* pos_ang) { return pin_graphs_impl(eng, "umx_pin_graphs", n_refs, pos_ang); }
int umx_pin_graphs_f64(umx_engine* eng, int n_refs, const double* pos_ang) { return pin_graphs_impl(eng, "umx_pin_graphs", n_refs, pos_ang); }
int umx_pin_assign(umx_engine* eng, int n_images, const int32_t* ref_of_image) {
  if (!eng) return UMX_ERR_ARG;
  if (!eng->pin_on) return fail(eng, UMX_ERR_ARG, "umx_pin_assign: nothing is pinned (umx_pin_graphs)");
  if (n_images < 0) return fail(eng, UMX_ERR_ARG, "umx_pin_assign: bad arguments");
  if (n_images == 0 || !ref_of_image) { eng->pin_assign.clear(); return UMX_OK; }
  for (int k = 0; k < n_images; ++k)
    if (ref_of_image[k] < 0 || ref_of_image[k] >= eng->pin_refs)
      return fail(eng, UMX_ERR_ARG, "umx_pin_assign: image " + std::to_string(k) + " names reference " + std::to_string(ref_of_image[k]) + ", but " +
                  std::to_string(eng->pin_refs) + " are pinned");
  eng->pin_assign.assign(ref_of_image, ref_of_image + n_images);
  return UMX_OK;
}
int umx_pinned_graphs(const umx_engine* eng, int capacity, int64_t* n_edges, int32_t* max_degree) {
  if (!eng) return UMX_ERR_ARG;
  const int R = eng->pin_on ? eng->pin_refs : 0;
  for (int r = 0; r < R && r < capacity && n_edges; ++r) n_edges[r] = (int64_t)eng->pin_ref_edges(r);
  if (max_degree) *max_degree = R ? (int32_t)eng->pin_maxdeg : 0;
  return R;
}
int umx_unpin_graph(umx_engine* eng) {
  if (!eng) return UMX_ERR_ARG;
  pin_clear(eng);
  return UMX_OK;
}
int umx_pinned_graph(const umx_engine* eng, int64_t* n_edges, int32_t* max_degree) {
  if (!eng) return UMX_ERR_ARG;
  if (n_edges) *n_edges = eng->pin_on ? (int64_t)eng->pin_edges : 0;
  if (max_degree) *max_degree = eng->pin_on ? (int32_t)eng->pin_maxdeg : 0;
  return UMX_OK;
}

int umx_hvp_dev(umx_engine* eng, int n_bases, const double* d_base_ang, int n_dirs, const double* d_dir, const int32_t* base_of, double step_ang,
                int flags, double* d_hv, double* d_curv, double* d_e0, float* d_f0, void* hip_stream) {
  CHK(hvp_check(eng, n_bases, d_base_ang, n_dirs, d_dir, base_of, step_ang, flags, d_hv, d_e0, d_f0));
  HIPCHK(eng, hipSetDevice(eng->dev));
  return hvp_run(eng, static_cast<hipStream_t>(hip_stream), n_bases, d_base_ang, nullptr, n_dirs, d_dir, base_of, step_ang, flags, d_hv, d_curv, d_e0, d_f0);
}

int umx_hvp(umx_engine* eng, int n_bases, const double* base_ang, int n_dirs, const double* dir, const int32_t* base_of, double step_ang, int flags,
            double* hv, double* curv, double* e0, float* f0) {
  CHK(hvp_check(eng, n_bases, base_ang, n_dirs, dir, base_of, step_ang, flags, hv, e0, f0));
  const int R = n_bases, M = n_dirs;
  const size_t n3 = (size_t)eng->natoms * 3;
  for (size_t i = 0; i < (size_t)R * n3; ++i)
    if (!std::isfinite(base_ang[i])) return fail(eng, UMX_ERR_ARG, "umx_hvp: non-finite position (base " + std::to_string(i / n3) + ")");
  for (size_t i = 0; i < (size_t)M * n3; ++i)
    if (!std::isfinite(dir[i])) return fail(eng, UMX_ERR_ARG, "umx_hvp: non-finite component (direction " + std::to_string(i / n3) + ")");
  HIPCHK(eng, hipSetDevice(eng->dev));
  hipStream_t s = eng->stream;
  const bool given = (flags & HVP_GIVEN_F0) != 0;
  const long in = (long)(2 * R + M) * eng->natoms, out = (long)M * eng->natoms;      // (bases, directions, and room for the bases' forces handed in)
  if (eng->hvp_in_cap < in) CHK(grow(eng, eng->hvp_in_cap, in, {s}, {DevBuf(eng->d_hvp_in, (size_t)in * 3)}));
  if (eng->hvp_out_cap < out) CHK(grow(eng, eng->hvp_out_cap, out, {s}, {DevBuf(eng->d_hvp_out, (size_t)out * 3 + M)}));
  double *d_base = eng->d_hvp_in, *d_dir = eng->d_hvp_in + (size_t)R * n3, *d_hv = eng->d_hvp_out, *d_curv = eng->d_hvp_out + (size_t)M * n3;
  HIPCHK(eng, hipMemcpyAsync(d_base, base_ang, (size_t)R * n3 * sizeof(double), hipMemcpyHostToDevice, s));
  HIPCHK(eng, hipMemcpyAsync(d_dir, dir, (size_t)M * n3 * sizeof(double), hipMemcpyHostToDevice, s));
  float* d_f0 = given ? reinterpret_cast<float*>(eng->d_hvp_in + (size_t)(R + M) * n3) : nullptr;
  if (given) {
    for (size_t i = 0; i < (size_t)R * n3; ++i)
      if (!std::isfinite(f0[i])) return fail(eng, UMX_ERR_ARG, "umx_hvp: non-finite force handed in (base " + std::to_string(i / n3) + ")");
    HIPCHK(eng, hipMemcpyAsync(d_f0, f0, (size_t)R * n3 * sizeof(float), hipMemcpyHostToDevice, s));
  }
  CHK(hvp_run(eng, s, R, d_base, base_ang, M, d_dir, base_of, step_ang, flags, d_hv, curv ? d_curv : nullptr, nullptr, d_f0));
  const long K = hvp_images(R, M, flags);
  std::vector<double> en((size_t)K);
  HIPCHK(eng, hipMemcpyAsync(en.data(), eng->d_hvp_e, (size_t)K * sizeof(double), hipMemcpyDeviceToHost, s));
  HIPCHK(eng, hipMemcpyAsync(hv, d_hv, (size_t)M * n3 * sizeof(double), hipMemcpyDeviceToHost, s));
  if (curv) HIPCHK(eng, hipMemcpyAsync(curv, d_curv, (size_t)M * sizeof(double), hipMemcpyDeviceToHost, s));
  if (e0) HIPCHK(eng, hipMemcpyAsync(e0, eng->d_hvp_e, (size_t)R * sizeof(double), hipMemcpyDeviceToHost, s));
  if (f0 && !given) HIPCHK(eng, hipMemcpyAsync(f0, eng->d_hvp_f, (size_t)R * n3 * sizeof(float), hipMemcpyDeviceToHost, s));
  HIPCHK(eng, hipStreamSynchronize(s));
  for (long k = 0; k < K; ++k)
    if (!std::isfinite(en[k])) {
      (void)hipMemset(eng->d_flags, 0, sizeof(int));         // reported right here: do not fail the NEXT call for it as well
      return fail(eng, UMX_ERR_RANGE, "umx_hvp: image " + std::to_string(k) + ": non-finite energy" +
                  (eng->prec.fwd_f16() ? " (an activation beyond the fp16 operand range of UMX_PRECISION=split: try split-bf16, bf16x3 or fp32)"
                                      : " (an overflow in float32)"));
    }
  return UMX_OK;
}

int umx_last_partitions(const umx_engine* eng) { return eng ? eng->last_parts : 0; }
int umx_last_lanes(const umx_engine* eng) { return eng ? eng->last_lanes : 0; }

int umx_set_recompute(umx_engine* eng, int mode) {
  if (!eng) return UMX_ERR_ARG;
  if (mode < 0 || mode > 2) return fail(eng, UMX_ERR_ARG, "umx_set_recompute: mode must be 0 (off), 1 (when the stored plans do not fit) or 2 (always)");
  if (eng->gp_plan) return fail(eng, UMX_ERR_ARG, "umx_set_recompute: a graph-parallel evaluation is in progress (finish it with umx_gp_step)");
  eng->recompute = mode;
  return UMX_OK;
}
int umx_last_recompute(const umx_engine* eng) { return eng ? eng->last_recompute : 0; }

int64_t umx_workspace_bytes(const umx_engine* eng, int64_t n_nodes, int64_t n_edges, int parts, int recompute) {
  if (n_nodes < 0 || n_edges < 0 || parts < 0 || parts == 1 || parts > 16) return -1;
  const Precision pm = eng && eng->have_weights ? eng->prec : Precision();
  const int grid = eng && eng->have_weights ? eng->ws_grid() : 0;
  if (parts == 0) return (int64_t)carve(nullptr, n_nodes, n_edges, nullptr, pm, grid, recompute != 0);
  std::vector<long> pe(parts);
  for (int p = 0; p < parts; ++p) pe[p] = (long)(n_edges * (p + 1) / parts - n_edges * p / parts);
  return (int64_t)part_layout(pm, grid, recompute != 0, n_nodes, pe, nullptr);
}

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
  FILE* dump = nullptr;
  if (const char* dp = std::getenv("UMX_PROFILE_DUMP")) dump = std::fopen(dp, "a");
  for (size_t i = 0; i < eng->prof_used; ++i) {
    float t = 0.f;
    HIPCHK(eng, hipEventElapsedTime(&t, eng->prof[i].a, eng->prof[i].b));
    const ProfRec& r = eng->prof[i];
    if (out) {
      const int fam = r.prec > 0 ? 0 : (r.prec < 0 ? 2 : 1);
      out->ms[fam] += t; out->launches[fam] += 1; out->alg_flops[fam] += r.flops;
      out->mfma_flops[fam] += r.flops * (r.prec == 3 ? 6.0 : r.prec == 2 ? 3.0 : r.prec == 24 ? 4.0 : r.prec == 23 ? 3.0 : r.prec == 28 ? 6.0 : 1.0);   // (28: four fp16 + two bf8 products executed -- the bf8 ones at twice the rate)
    }
    if (dump) std::fprintf(dump, "%d,%d,%d,%d,%d,%d,%d,%.6f,%.6e\n", r.M, r.N, r.K, r.amode, r.cplx, r.prec, r.gz, t, r.flops);
  }
  if (dump) std::fclose(dump);
  if (reset) eng->prof_used = 0;
  return UMX_OK;
}

int umx_debug_keep(umx_engine* eng, int on) {
  if (!eng) return UMX_ERR_ARG;
  eng->dbg_on = on != 0;
  if (!on) { eng->dbg.clear(); eng->gemm_log.clear(); }
  return UMX_OK;
}

int umx_debug_fetch(umx_engine* eng, const char* name, void* host_buf, size_t capacity, size_t* nbytes_out) {
  if (!eng || !name) return UMX_ERR_ARG;
  const std::string nm(name);
  if (nm == "gemm:table" || nm == "gemm:table_gate" || nm == "gemm:launches") {
    // text, host side only: the rows of pl_kernels / of pl_gate_kernels ("fam cplx wide ls al half"), and the gemm_pl launches of the most recent evaluation's
    // last chunk in launch order ("fwd|rev fam cplx wide ls al half M N K blocks"; recorded while umx_debug_keep is on)
    const std::string text = nm == "gemm:table" ? pl_table_text() : nm == "gemm:table_gate" ? pl_gate_table_text() : eng->gemm_log;
    if (nbytes_out) *nbytes_out = text.size();
    if (host_buf) {
      if (capacity < text.size()) return fail(eng, UMX_ERR_ARG, "umx_debug_fetch: buffer too small");
      std::memcpy(host_buf, text.data(), text.size());
    }
    return UMX_OK;
  }
  if (nm == "bond_events:kernel_ms") {
    // three floats: the milliseconds of the count, scan and fill kernels of the last umx_bond_events, between its four events
    if (!eng->bond_timed) return fail(eng, UMX_ERR_ARG, "umx_debug_fetch: no umx_bond_events call has run");
    float ms[3];
    for (int k = 0; k < 3; ++k) HIPCHK(eng, hipEventElapsedTime(&ms[k], eng->ev_bond[k], eng->ev_bond[k + 1]));
    if (nbytes_out) *nbytes_out = sizeof(ms);
    if (host_buf) {
      if (capacity < sizeof(ms)) return fail(eng, UMX_ERR_ARG, "umx_debug_fetch: buffer too small");
      std::memcpy(host_buf, ms, sizeof(ms));
    }
    return UMX_OK;
  }
  if (nm.rfind("weights:", 0) == 0 || nm.rfind("experts:", 0) == 0) {
    // fetched on demand: the three weight arenas as they are on the device, the tensor table of d_w ("<name> <first float> <floats>" per
    // line), and the kernel time of the last umx_set_expert_coefficients (one float, milliseconds between its two events)
    if (!eng->have_weights) return fail(eng, UMX_ERR_ARG, "umx_debug_fetch: load weights first");
    HIPCHK(eng, hipSetDevice(eng->dev));
    HIPCHK(eng, hipStreamSynchronize(eng->stream));
    const void* dptr = nullptr; size_t nb = 0;
    std::string table; float ms = 0.f;
    if (nm == "weights:w") { dptr = eng->d_w; nb = eng->n_w * sizeof(float); }
    else if (nm == "weights:dw") { dptr = eng->d_dw; nb = eng->n_dw * sizeof(float); }
    else if (nm == "weights:bw") { dptr = eng->d_bw; nb = eng->n_bw * sizeof(unsigned short); }
    else if (nm == "weights:table") {
      for (const auto& kv : eng->wt) table += kv.first + " " + std::to_string(kv.second.off) + " " + std::to_string(kv.second.count) + "\n";
      nb = table.size();
    } else if (nm == "experts:kernel_ms") {
      if (!eng->experts_merged) return fail(eng, UMX_ERR_ARG, "umx_debug_fetch: no expert merge has run");
      HIPCHK(eng, hipEventElapsedTime(&ms, eng->ev_m0, eng->ev_m1));
      nb = sizeof(float);
    } else return fail(eng, UMX_ERR_ARG, std::string("umx_debug_fetch: no buffer named ") + name);
    if (nbytes_out) *nbytes_out = nb;
    if (host_buf) {
      if (capacity < nb) return fail(eng, UMX_ERR_ARG, "umx_debug_fetch: buffer too small");
      if (dptr) HIPCHK(eng, hipMemcpy(host_buf, dptr, nb, hipMemcpyDeviceToHost));
      else if (nm == "weights:table") std::memcpy(host_buf, table.data(), nb);
      else std::memcpy(host_buf, &ms, nb);
    }
    return UMX_OK;
  }
  auto it = eng->dbg.find(name);
  if (it == eng->dbg.end()) return fail(eng, UMX_ERR_ARG, std::string("umx_debug_fetch: no buffer named ") + name);
  if (nbytes_out) *nbytes_out = it->second.size();
  if (host_buf) {
    if (capacity < it->second.size()) return fail(eng, UMX_ERR_ARG, "umx_debug_fetch: buffer too small");
    std::memcpy(host_buf, it->second.data(), it->second.size());
  }
  return UMX_OK;
}

// umx_bond_changes and umx_bond_changes_cell: `cell` == nullptr launches the open kernel, else the minimum-image one on `cand`
static int bond_changes_run(umx_engine* eng, const char* who, int n, const double* r1, const double* r2, const double* cov, const umx::BondCell* cell,
                            const std::vector<double>& cand, double bond_factor, double margin_fraction, double delta_fraction, double* d1, double* d2,
                            uint8_t* code) {
  const std::string w = who;
  if (n <= 0 || !r1 || !r2 || !cov || !code) return fail(eng, UMX_ERR_ARG, w + ": bad arguments");
  if ((long)n * n > (1L << 31)) return fail(eng, UMX_ERR_CAPACITY, w + ": n*n exceeds 2^31 pairs");
  HIPCHK(eng, hipSetDevice(eng->dev));
  const size_t nn = (size_t)n * n, vb = (size_t)n * 3 * sizeof(double), cb = cand.size() * sizeof(double);
  double *d_r = nullptr, *d_d = nullptr; unsigned char* d_c = nullptr;
  HIPCHK(eng, hipMalloc(&d_r, 2 * vb + (size_t)n * sizeof(double) + cb));
  hipError_t e1 = hipMalloc(&d_d, 2 * nn * sizeof(double)), e2 = hipMalloc(&d_c, nn);
  if (e1 != hipSuccess || e2 != hipSuccess) {
    (void)hipFree(d_r); if (d_d) (void)hipFree(d_d); if (d_c) (void)hipFree(d_c);
    return fail(eng, UMX_ERR_HIP, w + ": hipMalloc of the pair matrices failed");
  }
  double* d_r2 = d_r + (size_t)n * 3; double* d_cov = d_r2 + (size_t)n * 3; double* d_cand = d_cov + n;
  hipStream_t s = eng->stream;
  int st = UMX_OK;
  auto ok = [&](hipError_t e, const char* what) { if (e != hipSuccess && st == UMX_OK) st = fail(eng, UMX_ERR_HIP, std::string(what) + ": " + hipGetErrorName(e)); };
  ok(hipMemcpyAsync(d_r, r1, vb, hipMemcpyHostToDevice, s), "copy r1");
  ok(hipMemcpyAsync(d_r2, r2, vb, hipMemcpyHostToDevice, s), "copy r2");
  ok(hipMemcpyAsync(d_cov, cov, (size_t)n * sizeof(double), hipMemcpyHostToDevice, s), "copy cov");
  if (cell) ok(hipMemcpyAsync(d_cand, cand.data(), cb, hipMemcpyHostToDevice, s), "copy the candidate translations");
  if (st == UMX_OK) {
    dim3 grid((n + 63) / 64, (n + 3) / 4);
    if (cell) {
      umx::k_bond_changes_cell<<<grid, 256, 0, s>>>(d_r, d_r2, d_cov, n, *cell, d_cand, (int)(cand.size() / 4), bond_factor, margin_fraction, delta_fraction,
                                                    d_d, d_d + nn, d_c);
      ok(hipGetLastError(), "k_bond_changes_cell");
    } else {
      umx::k_bond_changes<<<grid, 256, 0, s>>>(d_r, d_r2, d_cov, n, bond_factor, margin_fraction, delta_fraction, d_d, d_d + nn, d_c);
      ok(hipGetLastError(), "k_bond_changes");
    }
    if (d1) ok(hipMemcpyAsync(d1, d_d, nn * sizeof(double), hipMemcpyDeviceToHost, s), "copy d1");
    if (d2) ok(hipMemcpyAsync(d2, d_d + nn, nn * sizeof(double), hipMemcpyDeviceToHost, s), "copy d2");
    ok(hipMemcpyAsync(code, d_c, nn, hipMemcpyDeviceToHost, s), "copy code");
  }
  ok(hipStreamSynchronize(s), "sync");
  (void)hipFree(d_r); (void)hipFree(d_d); (void)hipFree(d_c);
  return st;
}

int umx_bond_changes(umx_engine* eng, int n, const double* r1, const double* r2, const double* cov, double bond_factor,
                     double margin_fraction, double delta_fraction, double* d1, double* d2, uint8_t* code) {
  if (!eng) return UMX_ERR_ARG;
  return bond_changes_run(eng, "umx_bond_changes", n, r1, r2, cov, nullptr, {}, bond_factor, margin_fraction, delta_fraction, d1, d2, code);
}

int umx_bond_changes_cell(umx_engine* eng, int n, const double* r1, const double* r2, const double* cov, const double cell[9], const int pbc[3],
                          double bond_factor, double margin_fraction, double delta_fraction, double* d1, double* d2, uint8_t* code) {
  if (!eng) return UMX_ERR_ARG;
  if (!cell || !pbc || !(pbc[0] || pbc[1] || pbc[2]))
    return bond_changes_run(eng, "umx_bond_changes", n, r1, r2, cov, nullptr, {}, bond_factor, margin_fraction, delta_fraction, d1, d2, code);
  umx::BondCell bc;
  std::vector<double> cand;
  std::string why;
  if (!bond_cell_candidates(cell, pbc, &bc, &cand, &why)) return fail(eng, UMX_ERR_ARG, "umx_bond_changes_cell: " + why);
  return bond_changes_run(eng, "umx_bond_changes_cell", n, r1, r2, cov, &bc, cand, bond_factor, margin_fraction, delta_fraction, d1, d2, code);
}

// every refusal comes before the first allocation and leaves the outputs as they were; the passes are umx_bonds.h
int umx_bond_events(umx_engine* eng, int n_atoms, int n_geoms, const double* r, int n_pairs, const int32_t* geom_a, const int32_t* geom_b,
                    const double* cov, const double cell[9], const int pbc[3], double bond_factor, double margin_fraction, double delta_fraction,
                    int64_t capacity, umx_bond_event* events, int64_t* n_events, int64_t* per_pair) {
  if (!eng) return UMX_ERR_ARG;
  const std::string w = "umx_bond_events: ";
  if (n_atoms <= 0 || n_geoms <= 0) return fail(eng, UMX_ERR_ARG, w + "n_atoms = " + std::to_string(n_atoms) + " and n_geoms = " + std::to_string(n_geoms) + " must be positive");
  if (!r || !cov || !n_events) return fail(eng, UMX_ERR_ARG, w + "r, cov and n_events must be given");
  if (!geom_a != !geom_b) return fail(eng, UMX_ERR_ARG, w + "only one of geom_a / geom_b is given (both, or neither for consecutive pairs)");
  std::vector<int32_t> consecutive;
  if (!geom_a) {
    if (n_geoms < 2) return fail(eng, UMX_ERR_ARG, w + "consecutive pairs need at least two geometries, n_geoms = " + std::to_string(n_geoms));
    n_pairs = n_geoms - 1;
    consecutive.resize(2 * (size_t)n_pairs);
    for (int p = 0; p < n_pairs; ++p) { consecutive[p] = p; consecutive[(size_t)n_pairs + p] = p + 1; }
    geom_a = consecutive.data(); geom_b = geom_a + n_pairs;
  }
  if (n_pairs <= 0) return fail(eng, UMX_ERR_ARG, w + "n_pairs = " + std::to_string(n_pairs) + " must be positive");
  if (capacity < 0 || (capacity > 0 && !events)) return fail(eng, UMX_ERR_ARG, w + "capacity = " + std::to_string(capacity) + (capacity < 0 ? " is negative" : " without an event buffer"));
  for (int p = 0; p < n_pairs; ++p)
    for (const int32_t g : {geom_a[p], geom_b[p]})
      if (g < 0 || g >= n_geoms)
        return fail(eng, UMX_ERR_ARG, w + "pair " + std::to_string(p) + " names geometry " + std::to_string(g) + ", outside [0, " + std::to_string(n_geoms) + ")");
  const size_t per_geom = (size_t)n_atoms * 3;
  for (int g = 0; g < n_geoms; ++g)
    for (size_t k = 0; k < per_geom; ++k)
      if (!std::isfinite(r[(size_t)g * per_geom + k]))
        return fail(eng, UMX_ERR_ARG, w + "non-finite coordinate in geometry " + std::to_string(g) + " (atom " + std::to_string(k / 3) + ")");
  for (int i = 0; i < n_atoms; ++i)
    if (!std::isfinite(cov[i])) return fail(eng, UMX_ERR_ARG, w + "non-finite radius of atom " + std::to_string(i));
  if (!cell || !pbc || !(pbc[0] || pbc[1] || pbc[2]))
    return bond_events_run(eng, n_atoms, n_geoms, r, n_pairs, geom_a, geom_b, cov, nullptr, {}, bond_factor, margin_fraction, delta_fraction, capacity, events,
                           n_events, per_pair);
  umx::BondCell bc;
  std::vector<double> cand;
  std::string why;
  if (!bond_cell_candidates(cell, pbc, &bc, &cand, &why)) return fail(eng, UMX_ERR_ARG, w + why);
  return bond_events_run(eng, n_atoms, n_geoms, r, n_pairs, geom_a, geom_b, cov, &bc, cand, bond_factor, margin_fraction, delta_fraction, capacity, events,
                         n_events, per_pair);
}

// ---- float64 block and row kernels (kernels, the shared refusals and the launch in umx_rowblocks.h): every refusal comes before the launch
int umx_blk_gram_dev(umx_engine* eng, int p, const double* d_x, int q, const double* d_y, int64_t n, double* d_g, void* hip_stream) {
  if (!eng) return UMX_ERR_ARG;
  CHK(blk_check(eng, "umx_blk_gram_dev", p, q, (long)n));
  if (!d_x || !d_y || !d_g) return fail(eng, UMX_ERR_ARG, "umx_blk_gram_dev: d_x, d_y and d_g must be given");
  return blk_launch(eng, umx::k_blk_gram, (unsigned)(p * q), hip_stream, d_x, d_y, q, n, d_g);
}

int umx_blk_combine_dev(umx_engine* eng, int p, const double* d_x, int q, const double* d_c, int64_t n, const double* d_z, int subtract, double* d_y,
                        void* hip_stream) {
  if (!eng) return UMX_ERR_ARG;
  CHK(blk_check(eng, "umx_blk_combine_dev", p, q, (long)n));
  if (!d_x || !d_c || !d_y) return fail(eng, UMX_ERR_ARG, "umx_blk_combine_dev: d_x, d_c and d_y must be given (d_z may be NULL)");
  if (blk_overlapped(d_y, (size_t)q * (size_t)n, {{"d_x", d_x, (size_t)p * (size_t)n}}))
    return fail(eng, UMX_ERR_ARG, "umx_blk_combine_dev: d_y overlaps d_x -- every output element reads a whole column of X (d_y may be d_z)");
  return blk_launch(eng, umx::k_blk_combine, nblk((long)q * (long)n, 256), hip_stream, d_x, d_c, d_z, p, q, n, subtract ? 1 : 0, d_y);
}

int umx_blk_scale_dev(umx_engine* eng, int p, const double* d_x, const double* d_w, int64_t n, double* d_y, void* hip_stream) {
  if (!eng) return UMX_ERR_ARG;
  CHK(blk_check(eng, "umx_blk_scale_dev", p, 1, (long)n));
  if (!d_x || !d_w || !d_y) return fail(eng, UMX_ERR_ARG, "umx_blk_scale_dev: d_x, d_w and d_y must be given");
  return blk_launch(eng, umx::k_blk_scale, nblk((long)p * (long)n, 256), hip_stream, d_x, d_w, p, n, d_y);
}

int umx_row_dot_dev(umx_engine* eng, int k, const double* d_x, const double* d_y, int64_t n, double* d_out, void* hip_stream) {
  if (!eng) return UMX_ERR_ARG;
  const char* who = "umx_row_dot_dev: ";
  CHK(blk_check(eng, "umx_row_dot_dev", k, 1, (long)n, true));
  if (!d_x || !d_y || !d_out) return fail(eng, UMX_ERR_ARG, std::string(who) + (!d_x ? "d_x" : !d_y ? "d_y" : "d_out") + " must be given");
  const size_t kn = (size_t)k * (size_t)n;
  if (const char* hit = blk_overlapped(d_out, (size_t)k, {{"d_x", d_x, kn}, {"d_y", d_y, kn}}))
    return fail(eng, UMX_ERR_ARG, std::string(who) + "d_out overlaps " + hit + " -- a sum is written while rows are still read");
  return blk_launch(eng, umx::k_row_dot, (unsigned)k, hip_stream, d_x, d_y, n, d_out);
}

int umx_row_axpby_dev(umx_engine* eng, int k, const double* d_a, const double* d_x, const double* d_b, const double* d_y, int64_t n, double* d_out,
                      void* hip_stream) {
  if (!eng) return UMX_ERR_ARG;
  const char* who = "umx_row_axpby_dev: ";
  CHK(blk_check(eng, "umx_row_axpby_dev", k, 1, (long)n, true));
  if (!d_a || !d_x || !d_out) return fail(eng, UMX_ERR_ARG, std::string(who) + (!d_a ? "d_a" : !d_x ? "d_x" : "d_out") + " must be given");
  if (!d_b != !d_y) return fail(eng, UMX_ERR_ARG, std::string(who) + (!d_b ? "d_b" : "d_y") + " is NULL and " + (!d_b ? "d_y" : "d_b") + " is not -- give both, or neither for out = a * x");
  const size_t kn = (size_t)k * (size_t)n;
  if (const char* hit = blk_overlapped(d_out, kn, {{"d_x", d_x, kn}, {"d_y", d_y, kn}}, true))       // d_out may BE d_x or d_y
    return fail(eng, UMX_ERR_ARG, std::string(who) + "d_out overlaps " + hit + " without being it");
  if (const char* hit = blk_overlapped(d_out, kn, {{"d_a", d_a, (size_t)k}, {"d_b", d_b, (size_t)k}}))
    return fail(eng, UMX_ERR_ARG, std::string(who) + "d_out overlaps " + hit + ", which every thread of a row reads");
  return blk_launch(eng, umx::k_row_axpby, nblk((long)k * (long)n, 256), hip_stream, d_a, d_x, d_b, d_y, k, n, d_out);
}

int umx_row_absmax_dev(umx_engine* eng, int k, const double* d_x, int64_t n, double* d_out, void* hip_stream) {
  if (!eng) return UMX_ERR_ARG;
  const char* who = "umx_row_absmax_dev: ";
  CHK(blk_check(eng, "umx_row_absmax_dev", k, 1, (long)n, true));
  if (!d_x || !d_out) return fail(eng, UMX_ERR_ARG, std::string(who) + (!d_x ? "d_x" : "d_out") + " must be given");
  if (blk_overlapped(d_out, (size_t)k, {{"d_x", d_x, (size_t)k * (size_t)n}}))
    return fail(eng, UMX_ERR_ARG, std::string(who) + "d_out overlaps d_x -- a maximum is written while rows are still read");
  return blk_launch(eng, umx::k_row_absmax, (unsigned)k, hip_stream, d_x, n, d_out);
}

}  // extern "C"
