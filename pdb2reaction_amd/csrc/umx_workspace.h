// umx_workspace.h -- host side, part 3 of 5: carving the workspace arena into the buffers of one chunk (WS, umx_engine.h).
#pragma once

namespace {

struct Bump {
  char* base; size_t off = 0;
  template <class T> T* take(size_t n) {
    off = (off + 255) & ~size_t(255);
    T* p = base ? reinterpret_cast<T*>(base + off) : nullptr;
    off += n * sizeof(T);
    return p;
  }
  size_t bytes() const { return (off + 255) & ~size_t(255); }
};

// Workspace layout.  PERSISTENT buffers live from the forward to the reverse pass of an evaluation (node-level state, the graph, and the
// per-edge activations of all four layers: ~72 KB per directed edge); TRANSIENT buffers are the operands between a producer and a GEMM
// (~48 KB per edge) and are dead at every exchange point of the plan -- which is what lets the partitions of ONE oversized image share a
// single transient region (eval_partitioned).  gridG: the grid points of the grid feed-forward, whose per-node buffers scale with it
// (0 = spectral feed-forward); pm: the precision mode, which decides the operand buffers of the transient region.
// carve_persist: node-level state, the graph lists and the small per-edge buffers (~0.3 KB per edge); carve_acts: the per-edge, per-layer
// activations -- stored for every layer (and the edge-degree link), or, for a RECOMPUTE plan (rc), ONE slot of ~18 KB per edge that every
// layer's pointers alias: a layer overwrites the last, and the reverse pass replays a layer's forward edge pipeline into the slot just
// before that layer's reverse segments (plan_chunk).  The slot is dead at every exchange point, like the transient region.
void carve_persist(Bump& b, long nn, long ne, WS& t, int gridG) {
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
}
void carve_acts(Bump& b, long ne, WS& t, bool rc) {
  if (rc) {
    static_assert(3 * C <= ROW, "the edge-degree link's radial output shares the slot's message rows");
    float* h1 = b.take<float>(ne * RH); float* h2 = b.take<float>(ne * RH);
    float* rad = b.take<float>(ne * RAD); float* hg = b.take<float>(ne * HG); float* msg = b.take<float>(ne * ROW);
    for (auto& x : t.h1pre) x = h1;
    for (auto& x : t.h2pre) x = h2;
    for (auto& x : t.rad) x = rad;
    for (auto& x : t.hg) x = hg;
    for (auto& x : t.msg) x = msg;
    t.rad_deg = msg;            // (the edge-degree link is one more "layer" of the slot: E x 384 of its E x 1152 message rows)
    return;
  }
  for (auto& x : t.h1pre) x = b.take<float>(ne * RH);
  for (auto& x : t.h2pre) x = b.take<float>(ne * RH);
  t.rad_deg = b.take<float>(ne * 3 * C);
  for (auto& x : t.rad) x = b.take<float>(ne * RAD);
  for (auto& x : t.hg) x = b.take<float>(ne * HG);
  for (auto& x : t.msg) x = b.take<float>(ne * ROW);
}
void carve_trans(Bump& b, long ne, WS& t, const Precision& pm) {
  t.ra = b.take<float>(ne * RH);
  t.hid = b.take<float>(ne * ROW); t.gy1 = b.take<float>(ne * XROT);
  t.e128a = b.take<float>(ne * RH);
  t.xrot = t.ghg = t.grad = nullptr;
  t.y1pl = t.hidpl = t.a2pl = t.gmsgpl = t.ghgpl = t.gradpl = nullptr;
  if (pm.planes) {
    t.gmsg = b.take<float>(ne * 3 * C);                      // only the edge-degree backward uses fp32 g_msg (E x 384)
    const long ne4 = (ne + 3) / 4 * 4;          // the quad-row (Q3) layout stores rows in groups of four
    // 2-byte units per operand element: forward operands take 4 B in both split formats; the reverse operands are PL planes, but for
    // the quad-row ones of the bf16x3 mode (float32 blocks)
    const long fp = 2, rp = pm.rev_planes, rq = pm.rev_quad() ? 2 : rp;
    t.y1pl = b.take<unsigned short>(ne4 * XROT * fp); t.hidpl = b.take<unsigned short>(ne4 * ROW * fp);
    t.a2pl = b.take<unsigned short>(ne4 * RH * fp); t.gmsgpl = b.take<unsigned short>(ne4 * ROW * rq);      // (ne4: the quad-row form of the bf16x3 reverse operands)
    t.ghgpl = b.take<unsigned short>(ne4 * HG * rq); t.gradpl = b.take<unsigned short>(ne * RAD * rp);
  } else {
    t.xrot = b.take<float>(ne * XROT); t.gmsg = b.take<float>(ne * ROW);
    t.ghg = b.take<float>(ne * HG); t.grad = b.take<float>(ne * RAD);
  }
}
size_t carve(char* base, long nn, long ne, WS* w, const Precision& pm, int gridG, bool rc) {
  Bump b{base};
  WS t;
  carve_persist(b, nn, ne, t, gridG);
  carve_acts(b, ne, t, rc);
  carve_trans(b, ne, t, pm);
  if (w) *w = t;
  return b.bytes();
}
// bytes of the workspace of a chunk of nn nodes and ne directed edges, or (base, w) its carve-up, for this engine's model and mode and
// the kind of plan (stored / recompute) of the evaluation being planned
inline size_t ws_bytes(const umx_engine* eng, long nn, long ne, char* base = nullptr, WS* w = nullptr) { return carve(base, nn, ne, w, eng->prec, eng->ws_grid(), eng->rc_active); }

// One image in `parts` target-node partitions (eval_partitioned), edges[p] directed edges each: every partition's own region, then ONE
// region all of them share, sized for the largest partition -- the transient operands, and for a recompute plan the activation slot too.
// off: [parts + 1] offsets of the partitions' regions, off[parts] = the shared region's; returns the total.
size_t part_layout(const Precision& pm, int gridG, bool rc, long nn, const std::vector<long>& edges, std::vector<size_t>* off) {
  size_t at = 0, shared = 0;
  if (off) off->assign(edges.size() + 1, 0);
  for (size_t p = 0; p < edges.size(); ++p) {
    WS t;
    Bump bp{nullptr}; carve_persist(bp, nn, edges[p], t, gridG);
    if (!rc) carve_acts(bp, edges[p], t, false);
    at += bp.bytes();
    if (off) (*off)[p + 1] = at;
    Bump bs{nullptr};
    if (rc) carve_acts(bs, edges[p], t, true);
    carve_trans(bs, edges[p], t, pm);
    shared = std::max(shared, bs.bytes());
  }
  return at + shared;
}
// the views of partition p of that layout
void part_carve(char* arena, const std::vector<size_t>& off, const Precision& pm, int gridG, bool rc, long nn, long ne, size_t p, WS& t) {
  Bump bp{arena + off[p]}; carve_persist(bp, nn, ne, t, gridG);
  if (!rc) carve_acts(bp, ne, t, false);
  Bump bs{arena + off.back()};
  if (rc) carve_acts(bs, ne, t, true);
  carve_trans(bs, ne, t, pm);
}

}  // namespace
