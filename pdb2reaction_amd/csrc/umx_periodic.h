// umx_periodic.h -- host side of the neighbour-graph stage (umx_graph.h).  A cell is turned, in float64, into what the periodic
// instantiations of the graph kernels read (struct Periodic): the lattice vectors, the dual vectors of the periodic sub-lattice
// (fractional coordinates for the wrap and for pruning), and the table of lattice translations.  The bound cells are ONE list -- a
// single cell every image shares (umx_set_cell) or one per image (umx_set_cells) -- with one upload routine.  Also here: the wrapped
// copy of the positions, the dispatcher that resolves (boundary kind, position type, cell argument) once, and one launcher per kernel.
//
// Translations per periodic axis k: N_k = floor(cutoff / h_k + 1e-4) + 1, h_k the distance between the lattice planes of axis k within
// the periodic sub-lattice -- the whole cells the cutoff spans, plus one because two wrapped atoms may be almost a cell apart (the 1e-4
// covers the float32 rounding of the wrap).  The table holds every combination, (2 N_a + 1)(2 N_b + 1)(2 N_c + 1) entries with c
// running fastest; N_k <= PBC_MAX_AXIS = 4, i.e. plane distances down to cutoff / 4 (1.5 A at the 6 A cutoff; a 5 A edge needs N = 2).
#pragma once

namespace {

struct PeriodicHost { Periodic per{}; Lattice64 lat{}; std::vector<float4> table; };   // one cell; lat: what the double-position kernels read next to per

inline void cross3(const double* u, const double* v, double* o) {
  o[0] = u[1] * v[2] - u[2] * v[1]; o[1] = u[2] * v[0] - u[0] * v[2]; o[2] = u[0] * v[1] - u[1] * v[0];
}
inline double norm3(const double* u) { return std::sqrt(u[0] * u[0] + u[1] * u[1] + u[2] * u[2]); }

// One entry of a translation table: t = a cell[0] + b cell[1] + c cell[2] rounded to float32, and the integer triple packed in w.  The ONE
// routine behind the table of build_periodic and the translations of a pinned graph (pin_upload_shifts), so both hold the same bits.
inline float4 shift_entry(const double cell[9], int a, int b, int c) {
  const unsigned code = (unsigned)(a + 8) | ((unsigned)(b + 8) << 8) | ((unsigned)(c + 8) << 16);
  float w;
  std::memcpy(&w, &code, sizeof(w));
  return make_float4((float)(a * cell[0] + b * cell[3] + c * cell[6]), (float)(a * cell[1] + b * cell[4] + c * cell[7]),
                     (float)(a * cell[2] + b * cell[5] + c * cell[8]), w);
}

// false + *why: the cell is refused
bool build_periodic(const double cell[9], const int pbc[3], double cutoff, PeriodicHost* out, std::string* why) {
  const char ax[3] = {'a', 'b', 'c'};
  for (int i = 0; i < 9; ++i)
    if (!std::isfinite(cell[i])) { *why = "non-finite cell entry"; return false; }
  bool on[3];
  int np = 0;
  double M[3][3];                      // periodic rows as given; open rows are replaced by unit vectors orthogonal to the periodic span
  for (int k = 0; k < 3; ++k) {
    on[k] = pbc[k] != 0;
    np += on[k] ? 1 : 0;
    for (int c = 0; c < 3; ++c) M[k][c] = cell[k * 3 + c];
    if (on[k] && !(norm3(M[k]) > 0.0)) { *why = std::string("degenerate cell: lattice vector ") + ax[k] + " has zero length"; return false; }
  }
  if (np == 2) {
    const int o = !on[0] ? 0 : (!on[1] ? 1 : 2), i = (o + 1) % 3, j = (o + 2) % 3;
    double n[3];
    cross3(M[i], M[j], n);
    const double ln = norm3(n);
    if (!(ln > 1e-6 * norm3(M[i]) * norm3(M[j]))) { *why = "degenerate cell: the two periodic lattice vectors span no area"; return false; }
    for (int c = 0; c < 3; ++c) M[o][c] = n[c] / ln;
  } else if (np == 1) {
    const int i = on[0] ? 0 : (on[1] ? 1 : 2), p = (i + 1) % 3, q = (i + 2) % 3;
    int least = 0;
    for (int c = 1; c < 3; ++c) if (std::fabs(M[i][c]) < std::fabs(M[i][least])) least = c;
    double e[3] = {0, 0, 0}, u[3], v[3];
    e[least] = 1.0;
    cross3(M[i], e, u);
    const double lu = norm3(u);
    for (int c = 0; c < 3; ++c) u[c] /= lu;
    cross3(M[i], u, v);
    const double lv = norm3(v);
    for (int c = 0; c < 3; ++c) { M[p][c] = u[c]; M[q][c] = v[c] / lv; }
  }
  double c12[3], c20[3], c01[3];
  cross3(M[1], M[2], c12); cross3(M[2], M[0], c20); cross3(M[0], M[1], c01);
  const double det = M[0][0] * c12[0] + M[0][1] * c12[1] + M[0][2] * c12[2];
  if (!(std::fabs(det) > 1e-6 * norm3(M[0]) * norm3(M[1]) * norm3(M[2]))) { *why = "degenerate cell: the periodic lattice vectors span no volume"; return false; }
  // dual vectors: b_k . M_l = delta_kl; for a periodic k it lies in the periodic span, and 1 / |b_k| is the plane distance of axis k
  const double* cr[3] = {c12, c20, c01};
  double B[3][3], h[3];
  int N[3];
  Periodic& per = out->per;
  per = Periodic();
  out->lat = Lattice64();
  for (int k = 0; k < 3; ++k) {
    for (int c = 0; c < 3; ++c) B[k][c] = cr[k][c] / det;
    h[k] = 1.0 / norm3(B[k]);
    N[k] = 0;
    if (!on[k]) continue;
    const double spans = cutoff / h[k] + 1e-4;
    if (!(spans < (double)PBC_MAX_AXIS)) {
      char buf[256];
      std::snprintf(buf, sizeof(buf), "the lattice planes of axis %c are %.4g A apart: a cutoff of %.4g A needs more than the %d lattice translations per direction "
                    "this engine searches (plane distances down to cutoff / %d)", ax[k], h[k], cutoff, PBC_MAX_AXIS, PBC_MAX_AXIS);
      *why = buf;
      return false;
    }
    N[k] = (int)std::floor(spans) + 1;
    for (int c = 0; c < 3; ++c) { per.a[k][c] = (float)cell[k * 3 + c]; per.b[k][c] = (float)B[k][c]; }
    for (int c = 0; c < 3; ++c) { out->lat.a[k][c] = cell[k * 3 + c]; out->lat.b[k][c] = B[k][c]; }
    per.gmax[k] = (float)(1.001 * cutoff / h[k] + 1e-3);
  }
  out->table.clear();
  for (int a = -N[0]; a <= N[0]; ++a)
    for (int b = -N[1]; b <= N[1]; ++b)
      for (int c = -N[2]; c <= N[2]; ++c) {
        if (a == 0 && b == 0 && c == 0) per.zero = (int)out->table.size();
        out->table.push_back(shift_entry(cell, a, b, c));
      }
  per.n_shifts = (int)out->table.size();
  return true;
}

// What k_bond_changes_cell reads for a cell in the unit of its coordinates (umx_bond_changes_cell): the lattice and dual vectors of
// build_periodic (no cutoff enters them: it is called with cutoff 0) and the candidate translations of the minimum-image search.
// With R = 1/2 sum over the periodic axes of |a_k| and h_k = 1 / |b_k| the plane distance, M_k = floor(R / h_k + 1/2): the rounded
// difference d0 has fractional coordinates within 1/2, so |d0| <= R, while a translate with |m_k| > M_k lies more than
// (M_k + 1/2) h_k > R from the origin along axis k -- the minimum over m in prod [-M_k, M_k] is the minimum over the whole lattice.
// Entry (tx, ty, tz, lb2): lb = max_k (|m_k| - 1/2) h_k bounds |d0 + t| from below for every such d0; it is stored shortened by 1e-9
// (the rounding of the device's d0, n and sums is ~1e-16) and squared, and the entries ascend in it, the zero translation first.
// false + *why: the cell is refused (build_periodic's reasons, or M_k > PBC_MAX_AXIS)
bool bond_cell_candidates(const double cell[9], const int pbc[3], umx::BondCell* bc, std::vector<double>* cand, std::string* why) {
  PeriodicHost ph;
  if (!build_periodic(cell, pbc, 0.0, &ph, why)) return false;
  double R = 0.0, h[3] = {0, 0, 0};
  int M[3] = {0, 0, 0};
  for (int k = 0; k < 3; ++k) {
    for (int c = 0; c < 3; ++c) { bc->a[k][c] = ph.lat.a[k][c]; bc->b[k][c] = ph.lat.b[k][c]; }
    if (pbc[k]) R += 0.5 * norm3(ph.lat.a[k]);
  }
  for (int k = 0; k < 3; ++k) {
    if (!pbc[k]) continue;
    h[k] = 1.0 / norm3(ph.lat.b[k]);
    const double m = std::floor(R / h[k] + 0.5);
    if (!(m <= (double)PBC_MAX_AXIS)) {
      char buf[256];
      std::snprintf(buf, sizeof(buf), "the lattice planes of axis %c are %.4g apart in a cell of half perimeter %.4g: the minimum-image search needs more than the %d "
                    "lattice translations per direction this engine searches", "abc"[k], h[k], R, PBC_MAX_AXIS);
      *why = buf;
      return false;
    }
    M[k] = (int)m;
  }
  struct Entry { double t[3], lb2; };
  std::vector<Entry> es;
  for (int a = -M[0]; a <= M[0]; ++a)
    for (int b = -M[1]; b <= M[1]; ++b)
      for (int c = -M[2]; c <= M[2]; ++c) {
        const int m[3] = {a, b, c};
        double lb = 0.0;
        for (int k = 0; k < 3; ++k) lb = std::max(lb, (std::abs(m[k]) - 0.5) * h[k]);
        lb *= 1.0 - 1e-9;
        es.push_back({{a * cell[0] + b * cell[3] + c * cell[6], a * cell[1] + b * cell[4] + c * cell[7], a * cell[2] + b * cell[5] + c * cell[8]},
                      (a || b || c) ? lb * lb : 0.0});
      }
  std::stable_sort(es.begin(), es.end(), [](const Entry& x, const Entry& y) { return x.lb2 < y.lb2; });
  cand->clear();
  for (const Entry& e : es) cand->insert(cand->end(), {e.t[0], e.t[1], e.t[2], e.lb2});
  return true;
}

// ---- the bound cells: one list, shared by all images (umx_set_cell) or one cell per image (umx_set_cells) ---------------------------
// every cell through build_periodic for the bound cutoff; false + *why (per-image cells: it names the image): one of them is refused
bool build_cells(long n, const double* cells, const int pbc[3], double cutoff, bool shared, std::vector<PeriodicHost>* out, std::string* why) {
  out->resize(n);
  for (long k = 0; k < n; ++k) {
    std::string w;
    if (!build_periodic(cells + (size_t)k * 9, pbc, cutoff, &(*out)[k], &w)) { *why = shared ? w : "image " + std::to_string(k) + ": " + w; return false; }
  }
  return true;
}

// put the cells' structs and their tables, packed one behind the other, on the device
int periodic_upload(umx_engine* eng, const std::vector<PeriodicHost>& ph) {
  const long n = (long)ph.size();
  long total = 0;
  for (const PeriodicHost& h : ph) total += (long)h.table.size();
  HIPCHK(eng, hipSetDevice(eng->dev));
  HIPCHK(eng, hipStreamSynchronize(eng->stream));                     // no evaluation may still be reading the old tables
  if (eng->ran_on_caller) HIPCHK(eng, hipEventSynchronize(eng->ev_done));
  if (eng->cells_cap < n) CHK(grow(eng, eng->cells_cap, n, {}, {DevBuf(eng->d_cells, (size_t)n), DevBuf(eng->d_lats, (size_t)n)}));
  if (eng->shifts_pk_cap < total) CHK(grow(eng, eng->shifts_pk_cap, total, {}, {DevBuf(eng->d_shifts_pk, (size_t)total)}));
  std::vector<Periodic> pers(n);
  std::vector<Lattice64> lats(n);
  std::vector<float4> table;
  table.reserve(total);
  eng->cell_shifts.resize(n);
  for (long k = 0; k < n; ++k) {
    lats[k] = ph[k].lat;
    pers[k] = ph[k].per;
    pers[k].shifts = eng->d_shifts_pk + table.size();
    eng->cell_shifts[k] = ph[k].per.n_shifts;
    table.insert(table.end(), ph[k].table.begin(), ph[k].table.end());
  }
  HIPCHK(eng, hipMemcpy(eng->d_shifts_pk, table.data(), table.size() * sizeof(float4), hipMemcpyHostToDevice));
  HIPCHK(eng, hipMemcpy(eng->d_cells, pers.data(), pers.size() * sizeof(Periodic), hipMemcpyHostToDevice));
  HIPCHK(eng, hipMemcpy(eng->d_lats, lats.data(), lats.size() * sizeof(Lattice64), hipMemcpyHostToDevice));
  eng->per_cutoff = eng->cutoff;
  return UMX_OK;
}

// umx_set_cell (`shared`: one cell, n = 1) and umx_set_cells; a refused cell leaves the cells in force
int set_cells_impl(umx_engine* eng, const char* who, bool shared, int n, const double* cells, const int* pbc) {
  if (!cells || !pbc || !(pbc[0] || pbc[1] || pbc[2])) { eng->pbc_on = false; eng->cells_shared = true; return UMX_OK; }
  if (n <= 0) return fail(eng, UMX_ERR_ARG, "umx_set_cells: n_images must be positive when cells are given");
  std::vector<PeriodicHost> ph;
  std::string why;
  if (!build_cells(n, cells, pbc, eng->cutoff, shared, &ph, &why)) return fail(eng, UMX_ERR_ARG, std::string(who) + ": " + why);
  CHK(periodic_upload(eng, ph));
  eng->cells.assign(cells, cells + (size_t)n * 9);
  eng->cells_shared = shared;
  for (int k = 0; k < 3; ++k) eng->pbc[k] = pbc[k] != 0;
  eng->pbc_on = true;
  return UMX_OK;
}

// Per-image cells bound for another number of images than the evaluation holds: refused before anything runs (`who`: the entry).
int periodic_check_images(umx_engine* eng, long K, const char* who) {
  if (!eng->pbc_on || eng->cells_shared || K == eng->n_cells()) return UMX_OK;
  return fail(eng, UMX_ERR_ARG, std::string(who) + ": " + std::to_string(K) + " images, but umx_set_cells bound cells for " + std::to_string(eng->n_cells()) +
              " (cell k belongs to image k: bind one cell per image, or one cell for all with umx_set_cell)");
}

// ---- one dispatcher for the graph kernels ----------------------------------------------------------------------------------------------
// f(pos, cells): the positions in their own type and the boundary argument of the instantiation to launch -- NoCells, or Cells<P> for
// the cells in force.  img0: the index within the call of the image pos starts at (per-image cells: image img0 + k reads cell img0 + k;
// a shared cell: every image reads cell 0).
template <typename F>
void with_boundary(const umx_engine* eng, PosPtr pos, long img0, F&& f) {
  const int first = eng->cells_shared ? 0 : (int)img0, stride = eng->cells_shared ? 0 : 1;
  if (!eng->pbc_on) { if (pos.d) f(pos.d, NoCells{}); else f(pos.f, NoCells{}); }
  else if (pos.d) f(pos.d, Cells<double>{eng->d_cells, eng->d_lats, first, stride});
  else f(pos.f, Cells<float>{eng->d_cells, first, stride});
}
template <typename F> void with_flag(bool b, F&& f) { if (b) f(std::true_type{}); else f(std::false_type{}); }
template <typename P> using pos_t = std::remove_const_t<std::remove_pointer_t<P>>;

// the wrapped copy of positions of one type: its buffer and its capacity
inline std::pair<float*&, long&> wrap_copy(umx_engine* eng, const float*) { return {eng->d_wrap, eng->wrap_cap}; }
inline std::pair<double*&, long&> wrap_copy(umx_engine* eng, const double*) { return {eng->d_wrap64, eng->wrap64_cap}; }

// Start of an evaluation.  Open boundaries: nothing.  Periodic: the tables follow the bound cutoff, the positions of all images are
// wrapped into the scratch copy (every image into its own cell, if umx_set_cells bound them), and *d_pos is pointed at it -- a float64
// copy, wrapped in float64, for double positions.
int periodic_prepare(umx_engine* eng, hipStream_t s, long K, PosPtr* d_pos) {
  eng->last_shifts = 0;
  if (!eng->pbc_on) return UMX_OK;
  const bool img = !eng->cells_shared;
  CHK(periodic_check_images(eng, K, "umx_energy_forces"));
  if (eng->per_cutoff != eng->cutoff) {          // umx_set_system changed the cutoff since umx_set_cell / umx_set_cells
    std::vector<PeriodicHost> ph;
    std::string why;
    if (!build_cells(eng->n_cells(), eng->cells.data(), eng->pbc, eng->cutoff, !img, &ph, &why))
      return fail(eng, UMX_ERR_ARG, std::string("umx_energy_forces: the cell") + (img ? "s set by umx_set_cells" : " set by umx_set_cell") + " and the bound cutoff: " + why);
    CHK(periodic_upload(eng, ph));
  }
  // the rank key of the truncating fill carries translation index * n_atoms + source in its low 32 bits (the largest table decides)
  const int most_at = (int)(std::max_element(eng->cell_shifts.begin(), eng->cell_shifts.end()) - eng->cell_shifts.begin());
  const int most = eng->cell_shifts[most_at];
  if ((unsigned long long)most * (unsigned long long)eng->natoms > 0xffffffffull)
    return fail(eng, UMX_ERR_ARG, "umx_energy_forces: " + (img ? "image " + std::to_string(most_at) + ": " : std::string()) + std::to_string(most) + " lattice translations x " +
                std::to_string(eng->natoms) + " atoms do not fit the 32-bit candidate index of the periodic graph");
  if (eng->pin_on) {                             // pinned graph: nothing is searched; the replay shifts the positions by the stored wrap offsets itself
    eng->last_shifts = (int)eng->pin_codes.size();
    return UMX_OK;
  }
  const long nt = K * eng->natoms;
  int st = UMX_OK;
  with_boundary(eng, *d_pos, 0, [&](auto* pos, auto cells) {
    if constexpr (is_periodic<decltype(cells)>) {
      auto [buf, cap] = wrap_copy(eng, pos);
      if (cap < nt && (st = grow(eng, cap, nt, {s}, {DevBuf(buf, (size_t)nt * 3)})) != UMX_OK) return;
      hipLaunchKernelGGL((k_wrap_cell<pos_t<decltype(pos)>>), dim3(nblk(nt, 256)), dim3(256), 0, s, pos, buf, nt, eng->natoms, cells);
      *d_pos = PosPtr(buf);
    }
  });
  CHK(st);
  HIPCHK(eng, hipGetLastError());
  eng->last_shifts = most;
  return UMX_OK;
}

// ---- the launchers: one site per kernel ------------------------------------------------------------------------------------------------
void launch_graph_count(umx_engine* eng, hipStream_t s, PosPtr d_pos, long nt, int* deg, int* cand, long lo, long hi, long img0) {
  with_boundary(eng, d_pos, img0, [&](auto* pos, auto cells) {
    hipLaunchKernelGGL((k_graph_count<pos_t<decltype(pos)>, decltype(cells)>), dim3(nblk(nt, 4)), dim3(256), 0, s, pos, eng->natoms, nt, eng->cutoff * eng->cutoff,
                       eng->max_neigh, deg, cand, lo, hi, eng->d_flags, cells);
  });
}
// etr (the pinning call's fill of the periodic reference image): the translation of every edge as one more output, the packed integer
// triple.  Open boundaries have no translation to report and leave etr as it is.
void launch_graph_fill(umx_engine* eng, hipStream_t s, bool trunc, PosPtr d_pos, long nn, const int* cand, const int* row_ptr, int* esrc, int* edst,
                       float* evec, long lo, long hi, long img0, int* etr = nullptr) {
  with_boundary(eng, d_pos, img0, [&](auto* pos, auto cells) {
    with_flag(trunc, [&](auto TRUNC) {
      with_flag(etr != nullptr && is_periodic<decltype(cells)>, [&](auto TOUT) {
        if constexpr (is_periodic<decltype(cells)> || !TOUT())
          hipLaunchKernelGGL((k_graph_fill<TRUNC(), TOUT(), pos_t<decltype(pos)>, decltype(cells)>), dim3(nblk(nn, 4)), dim3(256), 0, s, pos, eng->natoms, nn,
                             eng->cutoff * eng->cutoff, eng->max_neigh, cand, row_ptr, esrc, edst, evec, lo, hi, cells, etr);
      });
    });
  });
}
// the wrap offsets of the nref reference images of a pin (d_pos: the caller's positions, not the wrapped copy; the one shared cell); open
// boundaries: out stays zero
void launch_wrap_index(umx_engine* eng, hipStream_t s, PosPtr d_pos, long nref, int* out) {
  const long nt = nref * eng->natoms;
  with_boundary(eng, d_pos, 0, [&](auto* pos, auto cells) {
    if constexpr (is_periodic<decltype(cells)>)
      hipLaunchKernelGGL((k_wrap_index<pos_t<decltype(pos)>>), dim3(nblk(nt, 256)), dim3(256), 0, s, pos, out, nt, eng->natoms, cells);
  });
}

// The translations of the pinned edges in the cell(s) in force, [cells][distinct triples], through shift_entry -- at pinning, and again
// when umx_set_cell / umx_set_cells bind other cells under the pin.  `into`: the buffer to fill (grown when too small).
int pin_upload_shifts(umx_engine* eng, const std::vector<unsigned>& codes, float4** into, long* cap) {
  const long nc = eng->n_cells(), nd = (long)codes.size();
  if (!eng->pbc_on || nd == 0) return UMX_OK;
  std::vector<float4> tab((size_t)(nc * nd));
  for (long k = 0; k < nc; ++k)
    for (long t = 0; t < nd; ++t)
      tab[(size_t)(k * nd + t)] = shift_entry(eng->cells.data() + (size_t)k * 9, (int)(codes[t] & 255u) - 8, (int)((codes[t] >> 8) & 255u) - 8, (int)((codes[t] >> 16) & 255u) - 8);
  if (*cap < nc * nd) {
    if (*into) HIPCHK(eng, hipFree(*into));
    *into = nullptr; *cap = 0;
    HIPCHK(eng, hipMalloc(into, tab.size() * sizeof(float4)));
    *cap = nc * nd;
  }
  HIPCHK(eng, hipMemcpy(*into, tab.data(), tab.size() * sizeof(float4), hipMemcpyHostToDevice));
  return UMX_OK;
}

// the replay of the pinned graphs for the nimg images d_pos starts at, `total` edges in all (k_graph_replay): img describes them one by
// one; sub_cnt >= 0: one image, rows of its reference that start sub0 edges into it (a target-node partition).  Nothing to write: no launch
void launch_graph_replay(umx_engine* eng, hipStream_t s, PosPtr d_pos, long nimg, const PinImage* img, long sub0, long sub_cnt, long total, int* esrc, int* edst,
                         float* evec, long img0) {
  if (total <= 0) return;
  with_boundary(eng, d_pos, img0, [&](auto* pos, auto cells) {
    hipLaunchKernelGGL((k_graph_replay<pos_t<decltype(pos)>, decltype(cells)>), dim3(nblk(total, 256)), dim3(256), 0, s, pos, eng->natoms, img, (int)nimg, sub0,
                       sub_cnt, total, eng->d_pin_src, eng->d_pin_dst, eng->d_pin_tix, eng->d_pin_wrap, eng->d_pin_shifts, (int)eng->pin_codes.size(), esrc, edst,
                       evec, eng->d_flags, cells);
  });
}

}  // namespace
