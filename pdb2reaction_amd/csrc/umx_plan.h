// umx_plan.h -- host side, part 4 of 5:
//   the edge links between the GEMMs, one launcher each (link_*: instantiation by precision mode, grid, launch, operand capture);
//   the launch plan of one chunk, stage by stage (plan_chunk = plan_graph, plan_layer_fwd per layer, readout + reverse head, and per
//   layer in reverse the optional replay of plan_edge_fwd, plan_atomwise_bwd, plan_edge_bwd, plan_norm1_bwd, then force_assembly);
//   the executors (run_plan: Plan::run_to_sync of umx_engine.h on one stream; run_plans_alternating: two lanes and the matrix token);
//   one evaluation (energy_forces_on) as its phases -- degree pass, workspace budget, lane choice, amortised workspace size, chunk
//   planning, the partitioned fallback for an oversized image, the arena, execution.
// Functions named plan_* append segments to a Plan when the plan is made; the others issue launches when a segment runs.
#pragma once

namespace {

// ---- debug captures of the edge links' GEMM operands ---------------------------------------------
// (debug) An operand is captured as the GEMM reads it, directly behind the kernel that writes it, under the name of its format --
// tests/test_gpu_mfma_model.py holds the GEMMs' outputs against the bit-exact model of the matrix core on exactly these bits,
// tests/test_gpu_forward_links.py and test_gpu_edge_links.py the producers.  Odd rows are negated in every split-mode format.
enum OpFmt {
  OP_QUAD,      // <base>q:  float32 quad-row blocks, rows padded to 4 (bf16x3; the forward operands of split-bf16)
  OP_HALVES,    // <base>h:  the raw halves of the two-plane fp16 "Q2H" blocks (umx_edge.h): 4-row-padded rows x columns x 2 (split-f16 forward)
  OP_PLANES,    // <base>pl: PL bf16 planes of the rows themselves (the 16-bit reverse operands; the edge-degree fc3^T operand of every split mode)
  OP_ROWS       // <base>:   plain float32 rows (fp32 mode; g_rad of the bf16x3 reverse pass, which the fc3^T GEMM splits in registers)
};
OpFmt fwd_operand(const Precision& p) { return !p.planes ? OP_ROWS : p.fwd_fmt == 1 ? OP_HALVES : OP_QUAD; }
OpFmt rev_operand(const Precision& p) { return p.rev_quad() ? OP_QUAD : OP_PLANES; }
std::string link_tag(int slot) { return slot == NL ? ".deg" : "." + std::to_string(slot); }     // slot NL: the edge-degree embedding
int dbg_operand(umx_engine* eng, const char* base, int slot, OpFmt fmt, const void* ptr, long ne, long cols, int planes = 2) {
  if (!eng->dbg_on) return UMX_OK;
  const long rows = (fmt == OP_QUAD || fmt == OP_HALVES) ? (ne + 3) / 4 * 4 : ne;
  const size_t elem = fmt == OP_PLANES ? 2 * (size_t)planes : 4;
  return dbg_capture(eng, std::string(base) + (fmt == OP_QUAD ? "q" : fmt == OP_HALVES ? "h" : fmt == OP_PLANES ? "pl" : "") + link_tag(slot), ptr, (size_t)rows * cols * elem);
}

// ---- the edge links between the GEMMs ------------------------------------------------------------
// One launcher per link, in every precision mode: it picks the instantiation the mode runs (mode -> operand layout, umx_edge.h), computes
// the grid, launches on eng->stream and, in the split modes, captures the operand it wrote.
#define UMX_LAUNCH(kernel, grid, ...) hipLaunchKernelGGL(kernel, dim3(grid), dim3(256), 0, eng->stream, __VA_ARGS__)

// The radial MLP is split into its small layers (one fused kernel: "streaming" work) and the one large fc3 GEMM, so that the two-lane
// executor can treat the large GEMM as a matrix-pipe segment (Plan, umx_engine.h).
// Radial head, one persistent kernel: gaussians -> fc1 -> LN+SiLU -> fc2 -> LN+SiLU -> the fc3 operand (fp16 planes / float32 quad-row
// blocks of the split modes, or fp32 rows in w.ra); the intermediate rows never reach HBM
int link_radial_head(umx_engine* eng, const WS& w, const RadialW& r, int slot, long ne) {
  const bool planes = eng->prec.planes && eng->planes.count(r.w3);
  const unsigned tiles = nblk(ne, 64);                      // two 32-row MFMA tiles per workgroup tile, two workgroups per CU
  auto k = !planes ? k_radial_head<0> : eng->prec.fwd_fmt == 1 ? k_radial_head<2> : k_radial_head<4>;
  ProfRec* pr;
  CHK(prof_open(eng, &pr, 2.0 * ne * ((double)NG * RH + (double)RH * RH), -1, ne, RH, NG + RH));
  UMX_LAUNCH(k, vgrid(eng, tiles < 512u ? tiles : 512u), w.evec, w.ez, eng->gcoef, eng->d_gmu, r.w1g, r.tsd, r.ttd, r.ln1w, r.ln1b, r.w2, r.b2, r.ln2w, r.ln2b,
             w.h1pre[slot], w.h2pre[slot], planes ? (void*)w.a2pl : (void*)w.ra, ne, eng->odd_sign);
  CHK(prof_close(eng, pr));
  HIPCHK(eng, hipGetLastError());
  return dbg_operand(eng, "a2", slot, fwd_operand(eng->prec), eng->prec.planes ? (const void*)w.a2pl : (const void*)w.ra, ne, RH);
}
// K7a gather + rotate.  Split modes: + the radial modulation -> y1, conv 1's A operand.  fp32: the bare rotation -> xrot (conv 1 reads `rad`)
int link_gather_rotate(umx_engine* eng, const WS& w, int i, long ne) {
  if (!eng->prec.planes) {
    UMX_LAUNCH(k_gather_rotate, nblk(ne, 4), w.xn[i], w.esrc, w.edst, w.frame, w.xrot, ne);
    HIPCHK(eng, hipGetLastError());
    return UMX_OK;                             // (xrot is captured with the layer's forward captures, aggregate_fwd)
  }
  auto k = eng->prec.fwd_fmt == 1 ? k_gather_rotate_mod_q3<1> : k_gather_rotate_mod_q3<3>;
  UMX_LAUNCH(k, vgrid(eng, (nblk(ne, 4) + 7) / 8 * 8), w.xn[i], w.esrc, w.edst, w.frame, w.rad[i], w.y1pl, ne, eng->odd_sign);
  HIPCHK(eng, hipGetLastError());
  return dbg_operand(eng, "y1", i, fwd_operand(eng->prec), w.y1pl, ne, XROT);
}
// gate forward: hg = [gate | hpre] -> hid, conv 2's A operand
int link_gate_fwd(umx_engine* eng, const WS& w, int i, long ne) {
  if (!eng->prec.planes) {
    UMX_LAUNCH(k_gate_edge_fwd, nblk(ne * (H / 4), 256), w.hg[i], w.hid, ne);
    HIPCHK(eng, hipGetLastError());
    return UMX_OK;                             // (hid: aggregate_fwd)
  }
  auto k = eng->prec.fwd_fmt == 1 ? k_gate_edge_fwd_q3<1> : k_gate_edge_fwd_q3<3>;
  UMX_LAUNCH(k, vgrid(eng, nblk(ne, 8)), w.hg[i], w.hidpl, ne, eng->odd_sign);
  HIPCHK(eng, hipGetLastError());
  return dbg_operand(eng, "hid", i, fwd_operand(eng->prec), w.hidpl, ne, ROW);
}
// rotate-back backward (+ dE/dd and the torque of the rotation).  Of layer `slot`: g_xmid (G2) -> g_msg, conv 2^T's A operand.  Of the
// edge-degree embedding (slot NL): g_x0 (G0) -> the gradient of the edge-degree radial output, the fc3^T operand -- in the split modes
// straight into the PL planes of the fc3^T GEMM (gmsgpl is free here), three planes in the bf16x3 mode; else float32 rows in gmsg.
bool deg_rev_planes(const umx_engine* eng) { return eng->prec.planes && eng->planes.count(eng->rdeg.w3T) != 0; }
int link_rotate_back_bwd(umx_engine* eng, const WS& w, int slot, long ne) {
  const Precision& p = eng->prec;
  if (slot == NL) {
    const bool dpl = deg_rev_planes(eng);
    auto run = [&](auto k, auto* out) {
      UMX_LAUNCH(k, nblk(ne, 4), w.G0, w.rad_deg, w.frame, w.edst, out, w.dedd, w.tau, ne, DEG_RESCALE, dpl ? eng->odd_sign : 1.0f);
    };
    if (!dpl) run(k_rotate_back_bwd<3, 0>, w.gmsg);
    else if (p.rev_planes == 3) run(k_rotate_back_bwd<3, 3>, w.gmsgpl);
    else run(k_rotate_back_bwd<3, 2>, w.gmsgpl);
    HIPCHK(eng, hipGetLastError());
    return dpl ? dbg_operand(eng, "grad", NL, OP_PLANES, w.gmsgpl, ne, 3 * C, p.rev_planes) : UMX_OK;
  }
  if (!p.planes) {
    UMX_LAUNCH(k_rotate_back_bwd<9>, nblk(ne, 4), w.G2, w.msg[slot], w.frame, w.edst, w.gmsg, w.dedd, w.tau, ne, 1.0f, 1.0f);
    HIPCHK(eng, hipGetLastError());
    return UMX_OK;                             // (g_msg: plan_edge_bwd)
  }
  auto k = p.rev_quad() ? k_rotate_back_bwd_q3<3> : k_rotate_back_bwd_pl<2>;
  UMX_LAUNCH(k, vgrid(eng, (nblk(ne, 4) + 7) / 8 * 8), w.G2, w.msg[slot], w.frame, w.edst, w.gmsgpl, w.dedd, w.tau, ne, eng->odd_sign);
  HIPCHK(eng, hipGetLastError());
  return dbg_operand(eng, "gmsg", slot, rev_operand(p), w.gmsgpl, ne, ROW);
}
// gate backward: g_hid -> g_hg, conv 1^T's A operand
int link_gate_bwd(umx_engine* eng, const WS& w, int i, long ne) {
  if (!eng->prec.planes) {
    UMX_LAUNCH(k_gate_edge_bwd, nblk(ne * (H / 4), 256), w.hid, w.hg[i], w.ghg, ne, 1.0f);
    HIPCHK(eng, hipGetLastError());
    return UMX_OK;                             // (g_hg: plan_edge_bwd)
  }
  const bool quad = eng->prec.rev_quad();
  auto k = quad ? k_gate_edge_bwd_q3<3> : k_gate_edge_bwd_pl<2>;
  UMX_LAUNCH(k, vgrid(eng, quad ? nblk(ne, 8) : nblk(ne * (H / 4), 256)), w.hid, w.hg[i], w.ghgpl, ne, eng->odd_sign);
  HIPCHK(eng, hipGetLastError());
  return dbg_operand(eng, "ghg", i, rev_operand(eng->prec), w.ghgpl, ne, HG);
}
// One node-centric kernel: modulation backward + rotate-back + segmented sum -> g_xn in G1 (g_xrot stays in registers); g_rad, the fc3^T
// operand, as float32 rows (sign-alternating; split by the fc3^T GEMM in registers) in the bf16x3 mode, as two PL bf16 planes in the
// 16-bit-reverse modes.  Round 4: the fp32 mode takes it too (rows in w.grad, no alternating sign) instead of k_gather_rotate +
// k_modulate_bwd + k_gather_rotate_bwd -- the rotated message and g_xrot never touch HBM (-27 KB per edge and layer).
int link_modrot_bwd(umx_engine* eng, const WS& w, int i, long nn, long ne) {
  const bool pl = eng->prec.planes, rows = !pl || eng->prec.rev_quad();
  auto k = rows ? k_modrot_bwd_pl<0> : k_modrot_bwd_pl<2>;
  UMX_LAUNCH(k, (unsigned)nn, w.gy1, w.xn[i], w.frame, w.rad[i], w.row_ptr, w.out_ptr, w.out_edge, pl ? w.gradpl : reinterpret_cast<unsigned short*>(w.grad),
             w.tau, w.tau2, w.G1, nn, pl ? eng->odd_sign : 1.0f);
  HIPCHK(eng, hipGetLastError());
  if (!pl) return UMX_OK;                      // (fp32: with captures on the unfused kernels run, see plan_edge_bwd)
  return rows ? dbg_operand(eng, "gradq", i, OP_ROWS, w.gradpl, ne, RAD) : dbg_operand(eng, "grad", i, OP_PLANES, w.gradpl, ne, RAD);
}


// ---- radial MLP: the fc3 GEMM and the reverse pass -------------------------------------------------
int radial_fwd_fc3(umx_engine* eng, const WS& w, const RadialW& r, long ne, float* rad_out) {
  if (eng->prec.planes && eng->planes.count(r.w3)) return gemm_pl(eng, 0, FWD, w.a2pl, RH, 0, 0, r.w3, 0, r.b3, rad_out, r.out, 0, 0, ne, r.out, RH, 1.0f);
  return gemm_plain(eng, w.ra, RH, 0, r.w3, RH, r.b3, rad_out, r.out, 0, ne, r.out, RH);
}
int radial_fwd(umx_engine* eng, const WS& w, const RadialW& r, int slot, long ne, float* rad_out) {
  CHK(link_radial_head(eng, w, r, slot, ne));
  return radial_fwd_fc3(eng, w, r, ne, rad_out);
}
int radial_bwd_fc3(umx_engine* eng, const WS& w, const RadialW& r, long ne, const float* grad, const unsigned short* gradpl, bool f32rows = false) {
  if (gradpl) return gemm_pl(eng, 0, REV, gradpl, r.out, 0, 0, r.w3T, 0, nullptr, w.e128a, RH, 0, 0, ne, RH, r.out, 1.0f, f32rows);
  return gemm_plain(eng, grad, r.out, 0, r.w3T, r.out, nullptr, w.e128a, RH, 0, ne, RH, r.out);
}
int radial_bwd_tail(umx_engine* eng, const WS& w, const RadialW& r, int slot, long ne) {
  // one persistent kernel: LN+SiLU bwd -> fc2^T -> LN+SiLU bwd -> fc1^T -> dE/dd through the gaussians (accumulated into dedd_rad)
  const unsigned tiles = nblk(ne, 64);
  ProfRec* pr;
  CHK(prof_open(eng, &pr, 2.0 * ne * ((double)NG * RH + (double)RH * RH), -1, ne, RH, NG + RH));
  const std::string t = link_tag(slot);
  DBG("g_a2" + t, w.e128a, ne * RH);           // (debug) the output of fc3^T, the tail's input
  UMX_LAUNCH(k_radial_tail, vgrid(eng, tiles < 512u ? tiles : 512u), w.e128a, w.h2pre[slot], w.h1pre[slot], w.evec, eng->gcoef, eng->d_gmu, r.ln2w, r.ln2b, r.ln1w, r.ln1b,
             r.w2T, r.w1gT, w.dedd_rad, ne);
  CHK(prof_close(eng, pr));
  HIPCHK(eng, hipGetLastError());
  DBG("dedd_rad" + t, w.dedd_rad, ne);         // (debug) accumulated over the layers (NL - 1 first, then the edge-degree MLP)
  return UMX_OK;
}
int radial_bwd(umx_engine* eng, const WS& w, const RadialW& r, int slot, long ne, const float* grad, const unsigned short* gradpl = nullptr) {
  CHK(radial_bwd_fc3(eng, w, r, ne, grad, gradpl));
  return radial_bwd_tail(eng, w, r, slot, ne);
}

// ---- one chunk: nn nodes (= images * natoms), edges counted on the fly --------------------------
// What the stages of a chunk's plan share, computed once by plan_chunk.  A Plan outlives plan_chunk (run_chunks and eval_partitioned run
// it after planning has returned, umx_gp_step in later calls), so every closure holds its OWN COPY of the context: it is captured by
// value, never by reference.  The one reference a closure holds is the workspace view `w`, whose owner (the lanes' views of
// evaluate_planned, the partitions' of eval_partitioned, eng->gp_ws) outlives the plan.
//   eng->stream is read when a closure RUNS (the executor points it at the lane's stream);
//   eng->gp, gp_lo / gp_hi and the pinned ranges are read when the plan is MADE (eval_partitioned changes them around every plan_chunk).
struct ChunkCtx {
  umx_engine* eng;
  long nn, ne, nimg;
  long img0;                     // the index within the call of the chunk's first image (d_pos, d_deg, d_cand and the outputs start there; per-image cells are indexed by it)
  bool gp;                       // graph-parallel: partial sums over this rank's edges + exchange points
  long g_lo, g_hi;               // ... of the targets [g_lo, g_hi)
  bool pinned;                   // pinned graphs: what the replay reads of the chunk's images (pin_img), all edges of every image's reference --
  const PinImage* pin_img;       // or (pin_cnt >= 0: a partition, one image) the contiguous rows [g_lo, g_hi) of its reference, which start
  long pin_sub0, pin_cnt;        // pin_sub0 edges into it
  bool may_trunc;                // some node of this call has more candidates than max_neigh (known on the host)
  bool rc;                       // recompute plan: one activation slot (carve_acts), replayed layer by layer in the reverse pass
  bool fused_rev;                // k_modrot_bwd_pl produces g_xn itself (fp32 mode with debug captures: the unfused kernels, which expose xrot / g_xrot)
  PosPtr d_pos; const int *d_deg, *d_cand;
  double* d_energy; float* d_forces;
  VirialOut vir;                 // vir.out != nullptr: the chunk's final segment also takes the virial of its images (umx_virial.h)
};
#define UMX_STAGE(c) umx_engine* const eng = (c).eng; const hipStream_t s = eng->stream; const long nn = (c).nn, ne = (c).ne; (void)s; (void)nn; (void)ne

// K1 graph: row pointers, edge list, out-lists, frames, element pairs
int graph_build(const ChunkCtx& c, const WS& w) {
  UMX_STAGE(c);
  eng->gemm_log.clear();                        // a chunk starts here: "gemm:launches" names the last chunk's launches
  launch_scan(s, c.d_deg, nn, w.row_ptr, w.stats);
  if (c.pinned) launch_graph_replay(eng, s, c.d_pos, c.nimg, c.pin_img, c.pin_sub0, c.pin_cnt, ne, w.esrc, w.edst, w.evec, c.img0);
  else launch_graph_fill(eng, s, c.may_trunc, c.d_pos, nn, c.d_cand, w.row_ptr, w.esrc, w.edst, w.evec, c.g_lo, c.g_hi, c.img0);
  HIPCHK(eng, hipMemsetAsync(w.out_cur, 0, (nn + 1) * sizeof(int), s));
  if (ne > 0) UMX_LAUNCH(k_out_count, nblk(ne, 256), w.esrc, ne, w.out_cur);
  launch_scan(s, w.out_cur, nn, w.out_ptr, w.stats + 2);
  HIPCHK(eng, hipMemsetAsync(w.out_cur, 0, (nn + 1) * sizeof(int), s));
  if (ne > 0) {
    UMX_LAUNCH(k_out_fill, nblk(ne, 256), w.esrc, ne, w.out_ptr, w.out_cur, w.out_edge);
    UMX_LAUNCH(k_out_sort, nblk(nn, 4), w.out_ptr, nn, w.out_edge);
    UMX_LAUNCH(k_edge_geom, nblk(ne, 256), w.evec, ne, eng->cutoff, w.frame);
    UMX_LAUNCH(k_edge_z, nblk(ne, 256), w.esrc, w.edst, eng->d_z, eng->natoms, w.ez, ne);
  }
  HIPCHK(eng, hipGetLastError());
  DBG("row_ptr", w.row_ptr, nn + 1); DBG("src", w.esrc, ne); DBG("dst", w.edst, ne); DBG("out_ptr", w.out_ptr, nn + 1); DBG("out_edge", w.out_edge, ne);
  DBG("evec", w.evec, ne * 4); DBG("frame", w.frame, ne * FRAME);
  return UMX_OK;
}

// K4 + K5 edge-degree embedding: x0 = node init + sum over incoming edges (one kernel, the base added in double); graph-parallel: the bare
// partial sum goes to G1 and is all-reduced first, the base is added by k_node_init_add behind the exchange point
int edge_degree_embed(const ChunkCtx& c, const WS& w) {
  UMX_STAGE(c);
  if (ne > 0) {
    CHK(link_radial_head(eng, w, eng->rdeg, NL, ne));
    CHK(radial_fwd_fc3(eng, w, eng->rdeg, ne, w.rad_deg));
  }
  if (c.gp) UMX_LAUNCH(k_rotate_back_reduce<3>, nblk(nn, 4), w.rad_deg, w.frame, w.row_ptr, (const float*)nullptr, w.G1, nn, DEG_RESCALE,
                       (const int*)nullptr, 0, (const float*)nullptr, (const double*)nullptr);
  else UMX_LAUNCH(k_rotate_back_reduce<3>, nblk(nn, 4), w.rad_deg, w.frame, w.row_ptr, (const float*)nullptr, w.xs[0], nn, DEG_RESCALE,
                  (const int*)eng->d_z, eng->natoms, eng->emb_sphere, (const double*)eng->d_sysemb);
  HIPCHK(eng, hipGetLastError());
  if (!c.gp) { DBG("rad.deg", w.rad_deg, ne * 3 * C); DBG("x0", w.xs[0], nn * ROW); DBG("h1pre.deg", w.h1pre[NL], ne * RH); DBG("h2pre.deg", w.h2pre[NL], ne * RH); }
  return UMX_OK;
}

void plan_graph(Plan& P, WS& w, const ChunkCtx& c) {
  P.stream([c, &w]() -> int { CHK(graph_build(c, w)); return edge_degree_embed(c, w); });
  if (!c.gp) return;
  P.sync(w.G1, (size_t)c.nn * ROW);
  P.stream([c, &w]() -> int {
    UMX_STAGE(c);
    UMX_LAUNCH(k_node_init_add, nblk(nn * ROW, 256), eng->d_z, eng->natoms, nn, eng->emb_sphere, eng->d_sysemb, w.G1, w.xs[0]);
    HIPCHK(eng, hipGetLastError());
    return UMX_OK;
  });
}

// The edge pipeline of layer i's forward pass (radial MLP, gather / rotate / modulate, conv 1, gate, conv 2 -> rad, hg, msg, h1pre,
// h2pre of the layer), led by the layer's first norm.  replay (recompute plans, reverse pass): the same segments from the STORED node
// input xn[i] -- the norm, like everything node-level, is not issued again; no kernel of the pipeline writes node state.
void norm1_fwd(const ChunkCtx& c, const WS& w, int i) {       // xn[i] = norm 1 of the layer's input (+ the system embedding)
  UMX_STAGE(c);
  UMX_LAUNCH(k_norm_fwd, nblk(nn, 4), w.xs[2 * i], eng->lw[i].n1w, eng->lw[i].n1b, eng->d_sysemb, w.xn[i], nn);
}
void plan_edge_fwd(Plan& P, WS& w, const ChunkCtx& c, int i, bool replay) {
  const LayerW* L = &c.eng->lw[i];
  if (c.ne > 0 && c.eng->prec.planes) {
    P.stream([=, &w]() -> int {
      if (!replay) norm1_fwd(c, w, i);
      return link_radial_head(c.eng, w, L->rad, i, c.ne);
    });
    P.matrix([=, &w]() -> int { return radial_fwd_fc3(c.eng, w, L->rad, c.ne, w.rad[i]); });
    P.stream([=, &w]() -> int { return link_gather_rotate(c.eng, w, i, c.ne); });
    // SO(2) conv 1 on the pre-modulated planes -> hg = [gate | hpre]
    P.matrix([=, &w]() -> int { return so2_conv(c.eng, FWD, w.y1pl, SO2_Y1, w.hg[i], SO2_HG, L->c1m0, L->c1m1, L->c1m2, L->c1m0b, c.ne, 1.0f); });
    P.stream([=, &w]() -> int { return link_gate_fwd(c.eng, w, i, c.ne); });
    // SO(2) conv 2 -> msg
    P.matrix([=, &w]() -> int { return so2_conv(c.eng, FWD, w.hidpl, SO2_MSG, w.msg[i], SO2_MSG, L->c2m0, L->c2m1, L->c2m2, L->c2m0b, c.ne, 1.0f); });
    return;
  }
  // fp32 mode (or no edges): one stream segment
  P.stream([=, &w]() -> int {
    UMX_STAGE(c);
    if (!replay) norm1_fwd(c, w, i);
    if (ne > 0) {
      CHK(link_gather_rotate(eng, w, i, ne));
      CHK(radial_fwd(eng, w, L->rad, i, ne, w.rad[i]));
      // SO(2) conv 1 (radially modulated) -> hg = [gate | hpre]
      CHK(so2_conv(eng, FWD, w.xrot, SO2_Y1, w.hg[i], SO2_HG, L->c1m0, L->c1m1, L->c1m2, L->c1m0b, ne, 1.0f, w.rad[i]));
      CHK(link_gate_fwd(eng, w, i, ne));
      // SO(2) conv 2 -> msg
      CHK(so2_conv(eng, FWD, w.hid, SO2_MSG, w.msg[i], SO2_MSG, L->c2m0, L->c2m1, L->c2m2, L->c2m0b, ne, 1.0f));
    }
    HIPCHK(eng, hipGetLastError());
    return UMX_OK;
  });
}

// K7b aggregate: xmid = xin + the sum of the incoming messages.  Graph-parallel: the partial sum of this rank's edges has been all-reduced
// in xn2 (plan_layer_fwd).  Then the layer's forward captures, every buffer still holding this layer.
int aggregate_fwd(const ChunkCtx& c, const WS& w, int i) {
  UMX_STAGE(c);
  float *xin = w.xs[2 * i], *xmid = w.xs[2 * i + 1];
  const std::string t = "." + std::to_string(i);
  if (c.gp) UMX_LAUNCH(k_add_rows, nblk(nn * ROW / 4, 256), xmid, xin, w.xn2, nn * ROW / 4);
  else UMX_LAUNCH(k_rotate_back_reduce<9>, vgrid(eng, nblk(nn, 4)), w.msg[i], w.frame, w.row_ptr, xin, xmid, nn, 1.0f,
                  (const int*)nullptr, 0, (const float*)nullptr, (const double*)nullptr);
  HIPCHK(eng, hipGetLastError());
  DBG("xn" + t, w.xn[i], nn * ROW); DBG("rad" + t, w.rad[i], ne * RAD); DBG("h1pre" + t, w.h1pre[i], ne * RH); DBG("h2pre" + t, w.h2pre[i], ne * RH);
  if (!eng->prec.planes) { DBG("xrot" + t, w.xrot, ne * XROT); DBG("hid" + t, w.hid, ne * ROW); }
  DBG("hg" + t, w.hg[i], ne * HG); DBG("msg" + t, w.msg[i], ne * ROW); DBG("xmid" + t, xmid, nn * ROW);
  return UMX_OK;
}

// K8 atom-wise block, spectral form: xout = xmid + SO(3) linear 2 (gate (SO(3) linear 1 (xn2), scalar MLP (xn2)))
int atomwise_fwd_spectral(const ChunkCtx& c, const WS& w, int i) {
  UMX_STAGE(c);
  const LayerW& L = eng->lw[i];
  float *xmid = w.xs[2 * i + 1], *xout = w.xs[2 * i + 2];
  const std::string t = "." + std::to_string(i);
  CHK(gemm_node(eng, w.xn2, ROW, 0, L.smlp, C, L.smlpb, w.gspre[i], 2 * H, 0, nn, 2 * H, C));
  CHK(so3_linear(eng, w.xn2, L.l1w, L.l1b, w.ffh[i], nn, nullptr));
  UMX_LAUNCH(k_gate_node_fwd, nblk(nn * H, 256), w.ffh[i], w.gspre[i], w.ffhg, nn);
  CHK(so3_linear(eng, w.ffhg, L.l2w, L.l2b, xout, nn, xmid));
  HIPCHK(eng, hipGetLastError());
  DBG("xn2" + t, w.xn2, nn * ROW); DBG("gspre" + t, w.gspre[i], nn * 2 * H); DBG("ffh" + t, w.ffh[i], nn * ROW); DBG("x" + t, xout, nn * ROW);
  if (eng->dbg_on) DBG("ffhg" + t, w.ffhg, nn * ROW);         // (debug) the gated hidden rows: one buffer for all layers
  return UMX_OK;
}
// ... grid form (GridAtomwise): to-grid -> Linear, SiLU, Linear, SiLU, Linear over the channels of every grid point -> from-grid (+ residual).
// The hidden pre-activations stay resident for the reverse pass; the SiLUs are applied while the next GEMM stages its A operand.
int atomwise_fwd_grid(const ChunkCtx& c, const WS& w, int i) {
  UMX_STAGE(c);
  const LayerW& L = eng->lw[i];
  float *xmid = w.xs[2 * i + 1], *xout = w.xs[2 * i + 2];
  const std::string t = "." + std::to_string(i);
  const int G = eng->grid_G;
  const long ng = nn * G;
  UMX_LAUNCH(k_grid_expand, nblk(nn, 4), w.xn2, eng->to_grid, G, w.gridA, nn);
  if (eng->dbg_on) DBG("gridin" + t, w.gridA, ng * C);      // (debug) the to-grid projection: gridA is overwritten by the third GEMM
  CHK(gemm_grid(eng, w.gridA, C, 0, L.g1w, C, L.g1b, w.ffg1[i], H, 0, ng, H, C));
  CHK(gemm_grid(eng, w.ffg1[i], H, 0, L.g2w, H, L.g2b, w.ffg2[i], H, 0, ng, H, H, A_SILU));
  CHK(gemm_grid(eng, w.ffg2[i], H, 0, L.g3w, H, L.g3b, w.gridA, C, 0, ng, C, H, A_SILU));
  UMX_LAUNCH(k_grid_contract, nblk(nn, 4), w.gridA, eng->from_grid, G, xmid, xout, nn);
  HIPCHK(eng, hipGetLastError());
  if (eng->dbg_on) DBG("gridout" + t, w.gridA, ng * C);     // (debug) the grid MLP's output, from-grid's input
  DBG("xn2" + t, w.xn2, nn * ROW); DBG("ffg1" + t, w.ffg1[i], ng * H); DBG("ffg2" + t, w.ffg2[i], ng * H); DBG("x" + t, xout, nn * ROW);
  return UMX_OK;
}

// layer i forward: edge pipeline, aggregate, atom-wise block
void plan_layer_fwd(Plan& P, WS& w, const ChunkCtx& c, int i) {
  plan_edge_fwd(P, w, c, i, false);
  if (c.gp) {      // partial aggregate of this rank's edges -> xn2 (free until the norm below), all-reduce, xmid = xin + sum
    P.stream([c, &w, i]() -> int {
      UMX_STAGE(c);
      UMX_LAUNCH(k_rotate_back_reduce<9>, nblk(nn, 4), w.msg[i], w.frame, w.row_ptr, (const float*)nullptr, w.xn2, nn, 1.0f,
                 (const int*)nullptr, 0, (const float*)nullptr, (const double*)nullptr);
      HIPCHK(eng, hipGetLastError());
      return UMX_OK;
    });
    P.sync(w.xn2, (size_t)c.nn * ROW);
  }
  P.stream([c, &w, i]() -> int {
    UMX_STAGE(c);
    const LayerW& L = eng->lw[i];
    CHK(aggregate_fwd(c, w, i));
    UMX_LAUNCH(k_norm_fwd, nblk(nn, 4), w.xs[2 * i + 1], L.n2w, L.n2b, (const double*)nullptr, w.xn2, nn);
    return eng->ff_grid ? atomwise_fwd_grid(c, w, i) : atomwise_fwd_spectral(c, w, i);
  });
}

// K9 readout: final norm, the energy MLP on the l = 0 channels, per-image sums
int readout(const ChunkCtx& c, const WS& w) {
  UMX_STAGE(c);
  UMX_LAUNCH(k_norm_fwd, nblk(nn, 4), w.xs[2 * NL], eng->normw, eng->normb, (const double*)nullptr, w.xf, nn);
  CHK(gemm_node(eng, w.xf, ROW, 0, eng->e0, C, eng->e0b, w.pre1, H, 0, nn, H, C));
  CHK(gemm_node(eng, w.pre1, H, 0, eng->e2, H, eng->e2b, w.pre2, H, 0, nn, H, H, A_SILU));
  UMX_LAUNCH(k_energy_node, nblk(nn, 4), w.pre2, eng->e4, eng->e4b, w.enode, nn);
  UMX_LAUNCH(k_energy, (unsigned)c.nimg, w.enode, eng->natoms, eng->rmsd, eng->refsum, c.d_energy, eng->d_flags);
  HIPCHK(eng, hipGetLastError());
  DBG("e_node", w.enode, nn); DBG("pre1", w.pre1, nn * H); DBG("pre2", w.pre2, nn * H);
  if (eng->dbg_on) DBG("xf", w.xf, nn * ROW);
  return UMX_OK;
}

// K10, the analytic reverse pass: its node-level head, dE/d(energy MLP) back to G0 = dE/dx of the last layer's output.
// (debug) every capture of the reverse node links sits directly behind the launch that writes its buffer: n128a / n128b, G0 / G1 / G2,
// ggs and gridA / gridB are reused from link to link
int reverse_head(const ChunkCtx& c, const WS& w) {
  UMX_STAGE(c);
  if (ne > 0) {
    HIPCHK(eng, hipMemsetAsync(w.dedd, 0, ne * sizeof(float), s));
    HIPCHK(eng, hipMemsetAsync(w.dedd_rad, 0, ne * sizeof(float), s));
    HIPCHK(eng, hipMemsetAsync(w.tau, 0, ne * 4 * sizeof(float), s));
    HIPCHK(eng, hipMemsetAsync(w.tau2, 0, ne * 4 * sizeof(float), s));
  }
  UMX_LAUNCH(k_silu_bwd, nblk(nn * H, 256), eng->e4, 0L, w.pre2, w.n128a, nn, H);
  if (eng->dbg_on) DBG("g_pre2", w.n128a, nn * H);
  CHK(gemm_node(eng, w.n128a, H, 0, eng->e2T, H, nullptr, w.n128b, H, 0, nn, H, H));
  if (eng->dbg_on) DBG("g_sil1", w.n128b, nn * H);              // dE / d silu(pre1)
  UMX_LAUNCH(k_silu_bwd, nblk(nn * H, 256), w.n128b, (long)H, w.pre1, w.n128a, nn, H);
  if (eng->dbg_on) DBG("g_pre1", w.n128a, nn * H);
  HIPCHK(eng, hipMemsetAsync(w.G1, 0, nn * ROW * sizeof(float), s));
  CHK(gemm_node(eng, w.n128a, H, 0, eng->e0T, H, nullptr, w.G1, ROW, 0, nn, C, H));
  if (eng->dbg_on) DBG("g_xf", w.G1, nn * ROW);                 // the whole row: the columns of l > 0 must still be zero
  UMX_LAUNCH(k_norm_bwd, nblk(nn, 4), w.G1, w.xs[2 * NL], eng->normw, (const float*)nullptr, w.G0, nn);
  HIPCHK(eng, hipGetLastError());
  DBG("g_xfinal", w.G0, nn * ROW);
  return UMX_OK;
}

// atom-wise backward, spectral form: G0 = dE/dx_out -> G1 = g_xn2
int atomwise_bwd_spectral(const ChunkCtx& c, const WS& w, int i) {
  UMX_STAGE(c);
  const LayerW& L = eng->lw[i];
  const std::string t = "." + std::to_string(i);
  CHK(so3_linear(eng, w.G0, L.l2T, nullptr, w.G1, nn, nullptr));                         // G1 = g_ffhg
  if (eng->dbg_on) DBG("g_ffhg" + t, w.G1, nn * ROW);
  UMX_LAUNCH(k_gate_node_bwd, nblk(nn * H, 256), w.G1, w.ffh[i], w.gspre[i], w.G2, w.ggs, nn);
  if (eng->dbg_on) { DBG("g_ffh" + t, w.G2, nn * ROW); DBG("g_gs" + t, w.ggs, nn * 2 * H); }
  CHK(so3_linear(eng, w.G2, L.l1T, nullptr, w.G1, nn, nullptr));                         // G1 = g_xn2
  if (eng->dbg_on) DBG("g_xn2a" + t, w.G1, nn * ROW);         // before the scalar MLP's share lands in the l = 0 columns
  CHK(gemm_node(eng, w.ggs, 2 * H, 0, L.smlpT, 2 * H, nullptr, w.G1, ROW, 0, nn, C, 2 * H, A_PLAIN, 1, 0, 0, w.G1, ROW, 0, 0));
  if (eng->dbg_on) DBG("g_xn2" + t, w.G1, nn * ROW);
  return UMX_OK;
}
// ... grid form, the reverse of GridAtomwise: from-grid^T -> W3^T, SiLU', W2^T, SiLU', W1^T -> to-grid^T
int atomwise_bwd_grid(const ChunkCtx& c, const WS& w, int i) {
  UMX_STAGE(c);
  const LayerW& L = eng->lw[i];
  const std::string t = "." + std::to_string(i);
  const int G = eng->grid_G;
  const long ng = nn * G;
  UMX_LAUNCH(k_grid_expand, nblk(nn, 4), w.G0, eng->from_grid, G, w.gridA, nn);
  if (eng->dbg_on) DBG("g_gridout" + t, w.gridA, ng * C);
  CHK(gemm_grid(eng, w.gridA, C, 0, L.g3T, C, nullptr, w.gridB, H, 0, ng, H, C));
  if (eng->dbg_on) DBG("g_gsil2" + t, w.gridB, ng * H);       // dE / d silu(ffg2)
  UMX_LAUNCH(k_silu_bwd, nblk(ng * H, 256), w.gridB, (long)H, w.ffg2[i], w.gridA, ng, H);
  if (eng->dbg_on) DBG("g_ffg2" + t, w.gridA, ng * H);
  CHK(gemm_grid(eng, w.gridA, H, 0, L.g2T, H, nullptr, w.gridB, H, 0, ng, H, H));
  if (eng->dbg_on) DBG("g_gsil1" + t, w.gridB, ng * H);       // dE / d silu(ffg1)
  UMX_LAUNCH(k_silu_bwd, nblk(ng * H, 256), w.gridB, (long)H, w.ffg1[i], w.gridA, ng, H);
  if (eng->dbg_on) DBG("g_ffg1" + t, w.gridA, ng * H);
  CHK(gemm_grid(eng, w.gridA, H, 0, L.g1T, H, nullptr, w.gridB, C, 0, ng, C, H));
  if (eng->dbg_on) DBG("g_gridin" + t, w.gridB, ng * C);
  UMX_LAUNCH(k_grid_contract, nblk(nn, 4), w.gridB, eng->to_grid, G, (const float*)nullptr, w.G1, nn);     // G1 = g_xn2
  if (eng->dbg_on) DBG("g_xn2" + t, w.G1, nn * ROW);
  return UMX_OK;
}

// layer i's atom-wise backward (G0 = dE/dx_out -> G2 = g_xmid) + the first edge kernel of the layer (split modes)
void plan_atomwise_bwd(Plan& P, WS& w, const ChunkCtx& c, int i) {
  P.stream([c, &w, i]() -> int {
    UMX_STAGE(c);
    CHK(eng->ff_grid ? atomwise_bwd_grid(c, w, i) : atomwise_bwd_spectral(c, w, i));
    UMX_LAUNCH(k_norm_bwd, nblk(nn, 4), w.G1, w.xs[2 * i + 1], eng->lw[i].n2w, w.G0, w.G2, nn);   // G2 = g_xmid
    HIPCHK(eng, hipGetLastError());
    DBG("g_xmid." + std::to_string(i), w.G2, nn * ROW);
    if (ne > 0 && eng->prec.planes) CHK(link_rotate_back_bwd(eng, w, i, ne));
    return UMX_OK;
  });
}

// The edge pipeline of layer i's reverse pass: g_xmid (G2) -> conv 2^T, gate backward, conv 1^T, modulation + rotation backward (g_xn
// in G1 when fused), the radial MLP backward (dE/dd)
void plan_edge_bwd(Plan& P, WS& w, const ChunkCtx& c, int i) {
  if (c.ne <= 0) return;
  const LayerW* L = &c.eng->lw[i];
  if (c.eng->prec.planes) {
    // bf16x3: conv 2^T applies gate^T in its epilogues and writes g_hg itself (umx_gemm_q.h EP = 1; the gate sums pass through the first
    // E x 256 floats of w.hid, which then holds no g_hid).  With debug captures on the two links run apart, so that g_hid exists and
    // "gemm:launches" names the table's rows.  Small chunks keep the two links as well: where conv 2^T's m = 1 grid does not put a
    // workgroup on every CU (choose_pl's `fills`: fewer than 16 257 edges) a launch lasts as long as ONE tile, the epilogue's round trip
    // to hg lengthens exactly that, and there is no second tile on the CU to run beside it.  A precaution, not a measured gain: c1 (13 k
    // edges) measured the same step time with and without the epilogue (profiles/gate_epilogue_ab.txt sections 1, 1b); c2 and c3 gain.
    // UMX_GATE_EPI (dev): 0 never, 1 as described, 2 always
    const int ge = c.eng->gate_epi;
    const bool fills = (c.ne + 127) / 128 * (SO2_MSG.m1w / 128) >= 256;
    if (c.eng->prec.rev_quad() && (ge == 2 || (ge == 1 && !c.eng->dbg_on && fills))) {
      P.matrix([=, &w]() -> int {
        UMX_STAGE(c);
        // (so2_conv's C argument is not written in this form -- the epilogues store to gate.ghg --; w.hid is passed as the gate sums' buffer)
        const GateEpi gate{w.hg[i], reinterpret_cast<float*>(w.ghgpl), w.hid, 0};
        CHK(so2_conv(eng, REV, w.gmsgpl, SO2_MSG, w.hid, SO2_MSG, L->c2m0T, L->c2m1T, L->c2m2T, nullptr, ne, -1.0f, nullptr, &gate));
        return dbg_operand(eng, "ghg", i, OP_QUAD, w.ghgpl, ne, HG);
      });
    } else {
      P.matrix([=, &w]() -> int { return so2_conv(c.eng, REV, w.gmsgpl, SO2_MSG, w.hid, SO2_MSG, L->c2m0T, L->c2m1T, L->c2m2T, nullptr, c.ne, -1.0f); });
      P.stream([=, &w]() -> int {
        UMX_STAGE(c);
        DBG("g_hid." + std::to_string(i), w.hid, ne * ROW);
        return link_gate_bwd(eng, w, i, ne);
      });
    }
    P.matrix([=, &w]() -> int { return so2_conv(c.eng, REV, w.ghgpl, SO2_HG, w.gy1, SO2_Y1, L->c1m0T, L->c1m1T, L->c1m2T, nullptr, c.ne, -1.0f); });
    // (a matrix-token segment although it is HBM-bound: at 240 VGPRs its waves cannot share a SIMD with a GEMM wave, so beside
    //  the other lane's GEMM it would only take CUs away from it; the other lane's throttled stream kernels do fit beside it)
    P.matrix([=, &w]() -> int {
      UMX_STAGE(c);
      DBG("g_y1." + std::to_string(i), w.gy1, ne * XROT);        // (debug) conv-1^T's output
      return link_modrot_bwd(eng, w, i, nn, ne);
    });
    P.matrix([=, &w]() -> int { return radial_bwd_fc3(c.eng, w, L->rad, c.ne, nullptr, w.gradpl, c.eng->prec.rev_quad()); });
    P.stream([=, &w]() -> int { return radial_bwd_tail(c.eng, w, L->rad, i, c.ne); });     // feeds only the scalar dE/dd (own accumulator dedd_rad)
    return;
  }
  // fp32 mode: one stream segment
  P.stream([=, &w]() -> int {
    UMX_STAGE(c);
    const std::string t = "." + std::to_string(i);
    CHK(link_rotate_back_bwd(eng, w, i, ne));
    CHK(so2_conv(eng, REV, w.gmsg, SO2_MSG, w.hid, SO2_MSG, L->c2m0T, L->c2m1T, L->c2m2T, nullptr, ne, -1.0f));
    DBG("g_msg" + t, w.gmsg, ne * ROW); DBG("g_hid" + t, w.hid, ne * ROW);
    CHK(link_gate_bwd(eng, w, i, ne));
    CHK(so2_conv(eng, REV, w.ghg, SO2_HG, w.gy1, SO2_Y1, L->c1m0T, L->c1m1T, L->c1m2T, nullptr, ne, -1.0f));
    DBG("g_hg" + t, w.ghg, ne * HG); DBG("g_y1" + t, w.gy1, ne * XROT);      // (k_modulate_bwd below turns g_y1 into g_xrot in place)
    if (c.fused_rev) CHK(link_modrot_bwd(eng, w, i, nn, ne));
    else {       // with debug captures on the unfused kernels run: they expose xrot / g_xrot to the stage-by-stage test
      CHK(link_gather_rotate(eng, w, i, ne));
      UMX_LAUNCH(k_modulate_bwd, nblk(ne, 4), w.gy1, w.xrot, w.rad[i], w.grad, w.tau, ne);
      DBG("g_xrot" + t, w.gy1, ne * XROT); DBG("g_rad" + t, w.grad, ne * RAD);
    }
    return radial_bwd(eng, w, L->rad, i, ne, w.grad);
  });
}

// g_xn of layer i (G1) and the layer's first norm backward: G0 = g_xin, the next layer's dE/dx_out
void plan_norm1_bwd(Plan& P, WS& w, const ChunkCtx& c, int i) {
  const bool have_gxn = c.ne > 0 && c.fused_rev;         // k_modrot_bwd_pl has left g_xn in G1
  auto gather_rotate_bwd = [c, &w]() -> int {            // unfused reverse (or no edges): G1 = g_xn from g_xrot (in gy1)
    UMX_STAGE(c);
    UMX_LAUNCH(k_gather_rotate_bwd, nblk(nn, 4), w.gy1, w.frame, w.row_ptr, w.out_ptr, w.out_edge, w.G1, nn);
    HIPCHK(eng, hipGetLastError());
    return UMX_OK;
  };
  if (c.gp) {
    // g_xn: every rank holds the contributions of its own edges only.  A rank WITHOUT edges (fewer atoms than ranks, or only isolated
    // targets) has run no edge kernel: G1 still holds g_xn2 of the atom-wise backward and must not enter the sum
    if (c.ne == 0) P.stream([c, &w]() -> int { HIPCHK(c.eng, hipMemsetAsync(w.G1, 0, (size_t)c.nn * ROW * sizeof(float), c.eng->stream)); return UMX_OK; });
    else if (!c.fused_rev) P.stream(gather_rotate_bwd);       // unfused reverse: the partial g_xn of this rank's edges has to exist BEFORE the exchange
    P.sync(w.G1, (size_t)c.nn * ROW);
  }
  P.stream([=, &w]() -> int {
    UMX_STAGE(c);
    if (!have_gxn && !c.gp) CHK(gather_rotate_bwd());
    UMX_LAUNCH(k_norm_bwd, nblk(nn, 4), w.G1, w.xs[2 * i], eng->lw[i].n1w, w.G2, w.G0, nn);                      // G0 = g_xin
    HIPCHK(eng, hipGetLastError());
    const std::string t = "." + std::to_string(i);
    DBG("g_xn" + t, w.G1, nn * ROW); DBG("g_xin" + t, w.G0, nn * ROW);
    return UMX_OK;
  });
}

// the edge-degree embedding's reverse links, the per-edge force and its sum over the nodes (+ the virial of the chunk's images)
int force_assembly(const ChunkCtx& c, const WS& w) {
  UMX_STAGE(c);
  if (ne > 0) {
    if (c.rc) {      // recompute plan: the edge-degree link's radial MLP again (h1pre / h2pre / rad_deg of the slot), not its node sum
      CHK(link_radial_head(eng, w, eng->rdeg, NL, ne));
      CHK(radial_fwd_fc3(eng, w, eng->rdeg, ne, w.rad_deg));
    }
    CHK(link_rotate_back_bwd(eng, w, NL, ne));
    CHK(radial_bwd(eng, w, eng->rdeg, NL, ne, w.gmsg, deg_rev_planes(eng) ? w.gmsgpl : nullptr));
    if (c.fused_rev) UMX_LAUNCH(k_add4, nblk(ne, 256), w.tau, w.tau2, ne);
    UMX_LAUNCH(k_force_edge, nblk(ne, 256), w.dedd, w.dedd_rad, w.tau, w.frame, w.evec, w.gvec, ne);
  }
  UMX_LAUNCH(k_force_node, nblk(nn, 4), w.gvec, w.row_ptr, w.out_ptr, w.out_edge, (float)eng->rmsd, c.d_forces, nn);
  HIPCHK(eng, hipGetLastError());
  if (c.vir.out) CHK(virial_launch(eng, w, c.vir, c.nimg, ne));       // (a partition: before the next one overwrites the shared gvec)
  DBG("dedd", w.dedd, ne); DBG("tau", w.tau, ne * 4); DBG("gvec", w.gvec, ne * 4);
  return UMX_OK;
}

// The launch sequence of one chunk, stage by stage: graph and edge-degree embedding; NL layers forward; readout; with forces, the analytic
// reverse pass layer by layer and the force assembly.  d_pos, d_deg, d_cand and the outputs are the chunk's own (they start at image img0
// of the call).
void plan_chunk(umx_engine* eng, WS& w, const PosPtr d_pos, const int* d_deg, const int* d_cand, long img0, long nimg, long ne, double* d_energy,
                float* d_forces, Plan& P, const VirialOut vir = VirialOut()) {
  const bool gp = eng->gp, pinned = eng->pin_on;
  const long nn = nimg * eng->natoms, g_lo = gp ? eng->gp_lo : 0, g_hi = gp ? eng->gp_hi : nn;
  const long* pin_row = pinned && gp ? eng->pin_row_of(eng->pin_cur[(size_t)img0]) : nullptr;      // (a partition: of the image's own reference)
  const long pin_sub0 = pin_row ? pin_row[g_lo] : 0, pin_cnt = pin_row ? pin_row[g_hi] - pin_sub0 : -1;
  const ChunkCtx c{eng, nn, ne, nimg, img0, gp, g_lo, g_hi, pinned, pinned ? eng->d_pin_img + img0 : nullptr, pin_sub0, pin_cnt, eng->may_truncate, eng->rc_active && d_forces != nullptr,
                   eng->prec.planes || !eng->dbg_on, d_pos, d_deg, d_cand, d_energy, d_forces, vir};
  plan_graph(P, w, c);
  for (int i = 0; i < NL; ++i) plan_layer_fwd(P, w, c, i);
  // K9 readout (+ the node-level head of the reverse pass)
  P.stream([c, &w]() -> int {
    CHK(readout(c, w));
    return c.d_forces ? reverse_head(c, w) : UMX_OK;
  });
  if (!d_forces) return;
  for (int i = NL - 1; i >= 0; --i) {
    // recompute plan: the activation slot holds another layer (or, between exchange points, another partition): replay this layer's
    // forward edge pipeline into it first.  Every transient operand is free here: the reverse segments of layer i + 1 are complete.
    // (One piece: the slot still holds layer NL - 1 when the reverse pass starts.)
    if (c.rc && ne > 0 && (gp || i != NL - 1)) plan_edge_fwd(P, w, c, i, true);
    plan_atomwise_bwd(P, w, c, i);
    plan_edge_bwd(P, w, c, i);
    plan_norm1_bwd(P, w, c, i);
  }
  P.stream([c, &w]() -> int { return force_assembly(c, w); });
  if (gp) P.sync(d_forces, (size_t)nn * 3);           // forces: sum of the ranks' edge contributions
}
#undef UMX_STAGE
#undef UMX_LAUNCH

// Issue one plan without exchange points on the stream eng->stream points at.
int run_plan(umx_engine* eng, Plan& P) {
  size_t at = 0;
  const Seg* stop = nullptr;
  CHK(P.run_to_sync(at, &stop));
  return stop ? fail(eng, UMX_ERR_ARG, "run_plan: a plan with exchange points is issued step by step (umx_gp_step, eval_partitioned)") : UMX_OK;
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

}  // namespace

// (C linkage and global scope: the kernel's symbol is part of the code object)
extern "C" {
struct PartPtrs { float* p[16]; int n; };
__global__ void k_sum_parts(PartPtrs pp, size_t count, float* __restrict__ also) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= count) return;
  float sum = 0.f;
  for (int k = 0; k < pp.n; ++k) sum += pp.p[k][i];          // fixed order: deterministic
  for (int k = 0; k < pp.n; ++k) pp.p[k][i] = sum;
  if (also) also[i] = sum;
}
}

namespace {

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

// ---- degree pass -----------------------------------------------------------------------------------
// End of a degree pass (k_graph_count + k_image_edges enqueued on s): the n edge totals followed by the largest degree come back to the
// host together with the flag word, which is cleared when set.  Bit 1: THIS pass met a non-finite position (bit 2: see below).  Bit 0: an EARLIER
// evaluation through a device-pointer entry produced a non-finite energy (this one has not computed an energy yet; on this stream that
// evaluation is complete): its caller got NaN energies / forces and, most likely, derived these positions from them.  A pass that is
// not the first of its call (own_only) leaves bit 0 to the next host sync.
int read_degree_pass(umx_engine* eng, hipStream_t s, const int* d_cnt, size_t n, std::vector<int>& cnt, bool own_only) {
  HIPCHK(eng, hipGetLastError());
  cnt.resize(n + 1);
  int flag = 0;
  HIPCHK(eng, hipMemcpyAsync(cnt.data(), d_cnt, (n + 1) * sizeof(int), hipMemcpyDeviceToHost, s));
  HIPCHK(eng, hipMemcpyAsync(&flag, eng->d_flags, sizeof(int), hipMemcpyDeviceToHost, s));
  HIPCHK(eng, hipStreamSynchronize(s));
  if (own_only) flag &= 6;
  if (!flag) return UMX_OK;
  HIPCHK(eng, hipMemsetAsync(eng->d_flags, 0, sizeof(int), s));
  if ((flag & 6) == 4)       // bit 2 (periodic graph only): more candidates than the truncating fill ranks
    return fail(eng, UMX_ERR_CAPACITY, "periodic graph: an atom has more than " + std::to_string(GF_MAXC) + " candidates (source, translation) within the cutoff while "
                "max_neigh = " + std::to_string(eng->max_neigh) + " binds; the truncating form ranks at most that many (a density beyond 1 atom per cubic Angstrom)");
  if (flag & 2)
    return fail(eng, UMX_ERR_ARG, "umx_energy_forces: non-finite position (device buffer)" +
                std::string((flag & 1) ? "; the previous device-pointer evaluation had already produced a non-finite energy" : ""));
  return fail(eng, UMX_ERR_RANGE, std::string("the previous device-pointer evaluation produced a non-finite energy") + eng->prec.range_hint());
}

// The reference every image of a pinned evaluation of K images replays.  An assignment (umx_pin_assign) holds for exactly its own number
// of images; without one, several references are replayed one per image, in order, and a single reference by every image of any batch.
int pin_resolve(umx_engine* eng, long K, std::vector<int>& out) {
  const long R = eng->pin_refs, A = (long)eng->pin_assign.size();
  if (A > 0 && K != A)
    return fail(eng, UMX_ERR_ARG, "umx_energy_forces: " + std::to_string(K) + " images, but umx_pin_assign assigned references to " + std::to_string(A) +
                " (entry k belongs to image k: assign one reference per image, or restore the default with umx_pin_assign(eng, 0, NULL))");
  if (A == 0 && R > 1 && K != R)
    return fail(eng, UMX_ERR_ARG, "umx_energy_forces: " + std::to_string(K) + " images, but " + std::to_string(R) + " graphs are pinned and image k replays "
                "reference k by default: evaluate one image per reference, or say which reference each image replays (umx_pin_assign)");
  if (A > 0) out = eng->pin_assign;
  else { out.resize((size_t)K); for (long k = 0; k < K; ++k) out[k] = R > 1 ? (int)k : 0; }
  return UMX_OK;
}

// directed edges per image of the batch at hand, and what the planning below asks of them
// (per_image: [K], the largest degree behind them; emax / etot: the largest image's edges, all edges)
struct ImageEdges { std::vector<int> per_image; long emax = 0, etot = 0; };

// degrees of every node of every image, per-image edge totals; sets last_edges / last_maxdeg / may_truncate
int degree_pass(umx_engine* eng, hipStream_t s, long K, const PosPtr d_pos, ImageEdges& ie) {
  const int N = eng->natoms;
  const long nt = K * N;
  if (eng->pin_on) {
    // pinned graphs: every image has the edges of its reference; nothing is launched and nothing read back.  (Only a call whose
    // images replay other references than the device copies hold image by image -- after a pin or umx_pin_assign, or more images than
    // any call before it -- writes the degrees k_scan reads and the table of the replay anew.)
    CHK(pin_resolve(eng, K, eng->pin_cur));
    const std::vector<int>& a = eng->pin_cur;
    if ((long)eng->pin_dev_for.size() < K || !std::equal(a.begin(), a.end(), eng->pin_dev_for.begin())) {
      std::vector<int> deg((size_t)nt);
      std::vector<PinImage> img((size_t)K);
      long long out0 = 0;
      for (long k = 0; k < K; ++k) {
        std::copy(eng->pin_deg.begin() + (size_t)a[k] * N, eng->pin_deg.begin() + ((size_t)a[k] + 1) * N, deg.begin() + k * N);
        img[k] = PinImage{out0, (long long)eng->pin_ref_e0[a[k]], (int)eng->pin_ref_edges(a[k]), a[k]};
        out0 += img[k].cnt;
      }
      eng->pin_dev_for.clear();
      // no earlier evaluation may still be reading what is replaced or overwritten
      for (hipStream_t q : {s, eng->stream2}) HIPCHK(eng, hipStreamSynchronize(q));
      HIPCHK(eng, hipEventSynchronize(eng->ev_done));
      if (eng->pin_deg_imgs < K) CHK(grow(eng, eng->pin_deg_imgs, K, {}, {DevBuf(eng->d_pin_deg, (size_t)nt), DevBuf(eng->d_pin_img, (size_t)K)}));
      HIPCHK(eng, hipMemcpy(eng->d_pin_deg, deg.data(), deg.size() * sizeof(int), hipMemcpyHostToDevice));
      HIPCHK(eng, hipMemcpy(eng->d_pin_img, img.data(), img.size() * sizeof(PinImage), hipMemcpyHostToDevice));
      eng->pin_dev_for = a;
    }
    ie.per_image.assign((size_t)K + 1, 0);
    ie.emax = ie.etot = 0;
    int maxdeg = 0;
    for (long k = 0; k < K; ++k) {
      const long e = eng->pin_ref_edges(a[k]);
      ie.per_image[k] = (int)e;
      ie.emax = std::max(ie.emax, e); ie.etot += e;
      maxdeg = std::max(maxdeg, eng->pin_ref_maxdeg[a[k]]);
    }
    ie.per_image[K] = maxdeg;
    eng->last_maxdeg = maxdeg;
    eng->may_truncate = false;
    eng->last_edges = ie.etot;
    return UMX_OK;
  }
  if (eng->deg_all_cap < nt) CHK(grow(eng, eng->deg_all_cap, nt, {s}, {DevBuf(eng->d_deg_all, nt), DevBuf(eng->d_cand_all, nt)}));
  if (eng->img_edges_cap < K + 1) CHK(grow(eng, eng->img_edges_cap, K + 1, {s}, {DevBuf(eng->d_img_edges, K + 1)}));
  HIPCHK(eng, hipMemsetAsync(eng->d_img_edges + K, 0, sizeof(int), s));
  launch_graph_count(eng, s, d_pos, nt, eng->d_deg_all, eng->d_cand_all, eng->gp ? eng->gp_lo : 0L, eng->gp ? eng->gp_hi : nt, 0);
  hipLaunchKernelGGL(k_image_edges, dim3((unsigned)K), dim3(256), 0, s, eng->d_deg_all, N, eng->d_img_edges, eng->d_img_edges + K);
  CHK(read_degree_pass(eng, s, eng->d_img_edges, K, ie.per_image, false));
  eng->last_maxdeg = ie.per_image[K];
  eng->may_truncate = ie.per_image[K] >= eng->max_neigh;          // (degrees are min(candidates, max_neigh): below the cap nothing was cut)
  ie.emax = ie.etot = 0;
  for (long k = 0; k < K; ++k) { ie.emax = std::max(ie.emax, (long)ie.per_image[k]); ie.etot += ie.per_image[k]; }
  eng->last_edges = ie.etot;
  return UMX_OK;
}

// ---- one image in P target-node partitions on ONE GPU ----------------------------------------------------------------------------
// The graph-parallel plan (exchange points, partial sums over a rank's own edges) run for P "virtual ranks" one after another: each
// partition keeps its own PERSISTENT workspace (node-level state + the per-edge activations of its edges), all of them share ONE
// TRANSIENT region (the producer -> GEMM operands are dead at every exchange point), and the all-reduce of an exchange point is a local
// sum.  Memory per directed edge drops from ~120 KB to ~72 KB + 48 KB / P, i.e. a single image of up to ~1.5x the atoms fits the same
// HBM; node-level work (< 3 %) is done P times.  Used automatically when one image exceeds the workspace budget.
// img: the image's index within the call (d_pos and the outputs are the image's own)
int eval_partitioned(umx_engine* eng, hipStream_t s, long img, const PosPtr d_pos, double* d_energy, float* d_forces, double* d_virial, int P, size_t budget,
                     int64_t* edges_out, int* maxdeg_out) {
  const int N = eng->natoms;
  if (P < 2 || P > 16) return fail(eng, UMX_ERR_ARG, "eval_partitioned: 2..16 partitions");
  if (eng->part_cap < (long)P * N)
    CHK(grow(eng, eng->part_cap, (long)P * N, {s}, {DevBuf(eng->d_part_deg, (size_t)2 * P * N + 32), DevBuf(eng->d_part_f, (size_t)P * N * 3)}));
  int* d_cnt = eng->d_part_deg + (size_t)2 * P * N;           // [P] edge totals, [P] = max degree
  std::vector<long> lo(P), hi(P);
  std::vector<int> cnt;
  if (eng->pin_on) {
    // pinned graphs: partition p takes the rows [lo, hi) of the image's reference -- its degrees there, zero elsewhere -- and the host
    // knows the counts
    const int ref = eng->pin_cur[(size_t)img];
    const long* row = eng->pin_row_of(ref);
    const int* ref_deg = eng->d_pin_deg + (size_t)img * N;
    cnt.assign((size_t)P + 1, 0);
    for (int p = 0; p < P; ++p) {
      lo[p] = (long)N * p / P; hi[p] = (long)N * (p + 1) / P;
      int* deg = eng->d_part_deg + (size_t)(2 * p) * N;
      HIPCHK(eng, hipMemsetAsync(deg, 0, (size_t)N * sizeof(int), s));
      if (hi[p] > lo[p]) HIPCHK(eng, hipMemcpyAsync(deg + lo[p], ref_deg + lo[p], (size_t)(hi[p] - lo[p]) * sizeof(int), hipMemcpyDeviceToDevice, s));
      cnt[p] = (int)(row[hi[p]] - row[lo[p]]);
    }
    cnt[P] = eng->pin_ref_maxdeg[ref];
    eng->may_truncate = false;
  } else {
  HIPCHK(eng, hipMemsetAsync(d_cnt, 0, (P + 1) * sizeof(int), s));
  for (int p = 0; p < P; ++p) {
    lo[p] = (long)N * p / P; hi[p] = (long)N * (p + 1) / P;
    int* deg = eng->d_part_deg + (size_t)(2 * p) * N;
    launch_graph_count(eng, s, d_pos, (long)N, deg, deg + N, lo[p], hi[p], img);
    hipLaunchKernelGGL(k_image_edges, dim3(1), dim3(256), 0, s, deg, N, d_cnt + p, d_cnt + P);
  }
  CHK(read_degree_pass(eng, s, d_cnt, P, cnt, true));
  eng->may_truncate = cnt[P] >= eng->max_neigh;
  }
  // layout: P persistent regions, then one shared region sized for the largest partition -- the transient operands and, for a recompute
  // plan, the activation slot: between two exchange points a partition replays and reverses ONE layer, then the next partition runs
  std::vector<size_t> off;
  const std::vector<long> pe(cnt.begin(), cnt.begin() + P);
  const size_t total = part_layout(eng->prec, eng->ws_grid(), eng->rc_active, N, pe, &off);
  if (total > budget) return UMX_ERR_CAPACITY;              // (the caller tries more partitions)
  if (eng->arena_bytes < total) CHK(grow_arena(eng, s, total));
  eng->cap_nodes = 0; eng->cap_edges = 0;                    // the ordinary path re-carves (and re-sizes) the arena on its next call
  std::vector<WS> ws(P);
  for (int p = 0; p < P; ++p) part_carve(eng->arena, off, eng->prec, eng->ws_grid(), eng->rc_active, N, cnt[p], p, ws[p]);
  std::vector<Plan> plans(P);
  double* wpart = eng->d_vir_wp;                              // [VIR_MAX_PARTS][9] (virial_prepare); P <= 16 is checked above
  const bool gp_keep = eng->gp; const long lo_keep = eng->gp_lo, hi_keep = eng->gp_hi;
  for (int p = 0; p < P; ++p) {
    eng->gp = true; eng->gp_lo = lo[p]; eng->gp_hi = hi[p];
    int* deg = eng->d_part_deg + (size_t)(2 * p) * N;
    // virial: the partition's own W_p (its edges are a contiguous range of the image's), taken in ITS final segment; the partials' slots
    // are shared, the partitions run one after another on s
    VirialOut vir;
    if (d_virial && d_forces) { vir.out = wpart + (size_t)p * 9; vir.part = eng->d_vir_part; vir.slabs = eng->vir_slabs; }
    plan_chunk(eng, ws[p], d_pos, deg, deg + N, img, 1, cnt[p], d_energy, d_forces ? eng->d_part_f + (size_t)p * N * 3 : nullptr, plans[p], vir);
  }
  eng->gp = gp_keep; eng->gp_lo = lo_keep; eng->gp_hi = hi_keep;
  std::vector<size_t> at(P, 0);
  int st = UMX_OK;
  for (;;) {
    PartPtrs pp; pp.n = P;
    size_t count = 0; int waiting = 0;
    for (int p = 0; p < P && st == UMX_OK; ++p) {
      const Seg* stop = nullptr;
      st = plans[p].run_to_sync(at[p], &stop);
      pp.p[p] = stop ? stop->sync_buf : nullptr;
      if (stop) { count = stop->sync_count; ++waiting; }
    }
    if (st != UMX_OK || waiting == 0) break;
    if (waiting != P) { st = fail(eng, UMX_ERR_ARG, "eval_partitioned: the partitions' plans disagree on their exchange points"); break; }
    const bool is_forces = d_forces && pp.p[0] == eng->d_part_f;
    hipLaunchKernelGGL(k_sum_parts, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, s, pp, count, is_forces ? d_forces : (float*)nullptr);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) { st = fail(eng, UMX_ERR_HIP, std::string("k_sum_parts: ") + hipGetErrorName(e)); break; }
    if (is_forces && d_virial) {                               // next to the forces: W = sum of the W_p in partition order
      hipLaunchKernelGGL(k_virial_sum_parts, dim3(1), dim3(64), 0, s, wpart, P, d_virial);
      e = hipGetLastError();
      if (e != hipSuccess) { st = fail(eng, UMX_ERR_HIP, std::string("k_virial_sum_parts: ") + hipGetErrorName(e)); break; }
    }
  }
  if (st != UMX_OK) return st;
  *edges_out = 0;
  for (int p = 0; p < P; ++p) *edges_out += cnt[p];
  *maxdeg_out = cnt[P];
  return UMX_OK;
}

// partition fallback: one image does not fit the budget in one piece (or UMX_FORCE_PARTS) -- image by image, in as few target-node
// partitions as fit.  `why`: the capacity message of the ordinary planning.
int eval_images_partitioned(umx_engine* eng, hipStream_t s, long K, const PosPtr d_pos, double* d_energy, float* d_forces, size_t budget, const std::string why) {
  const int N = eng->natoms;
  int64_t etot = 0; int mdeg = 0;
  for (long k = 0; k < K; ++k) {
    int stp = UMX_ERR_CAPACITY;
    for (int parts = eng->force_parts >= 2 ? eng->force_parts : 2; parts <= 16 && stp == UMX_ERR_CAPACITY; parts = eng->force_parts >= 2 ? 17 : parts + 1) {
      int64_t e1 = 0; int m1 = 0;
      stp = eval_partitioned(eng, s, k, d_pos.atom(k * N), d_energy + k, d_forces ? d_forces + k * N * 3 : nullptr,
                             eng->vir_out ? eng->vir_out + k * 9 : nullptr, parts, budget, &e1, &m1);
      if (stp == UMX_OK) { etot += e1; mdeg = std::max(mdeg, m1); eng->last_parts = parts; }
    }
    if (stp == UMX_ERR_CAPACITY)
      return fail(eng, UMX_ERR_CAPACITY, why + " -- and not in 16 partitions on this GPU either" +
                  (eng->rc_active ? " (recompute plan)" : "; umx_set_recompute / UMX_RECOMPUTE=1 lets one GPU evaluate it by recomputing the per-edge activations layer by layer"));
    if (stp != UMX_OK) return stp;
  }
  eng->last_edges = etot; eng->last_maxdeg = mdeg;
  HIPCHK(eng, hipEventRecord(eng->ev_done, s));
  return UMX_OK;
}

// ---- budget, lanes, amortised size ---------------------------------------------------------------
// workspace budget of this call: the caller's limit, else 85 % of what is free, capped by default
int workspace_budget(umx_engine* eng, const ImageEdges& ie, size_t* out) {
  size_t budget = eng->ws_limit;
  if (!budget) {
    size_t fr = 0, tot = 0;
    HIPCHK(eng, hipMemGetInfo(&fr, &tot));
    budget = (size_t)((fr + eng->arena_bytes) * 0.85);
    // default cap (UMX_WS_GB, 0 = none): chunks beyond a few images buy no speed (NOTES.md section 4), and an engine that takes
    // 85 % of the HBM starves every other engine of the process (a second calculator, the FD-Hessian helper, ...)
    if (eng->ws_cap_default && budget > eng->ws_cap_default && ws_bytes(eng, eng->natoms, ie.emax) <= eng->ws_cap_default)
      budget = eng->ws_cap_default;                            // (a single image larger than the cap keeps the full budget)
  }
  *out = budget;
  return UMX_OK;
}

int choose_lanes(const umx_engine* eng, long K, const ImageEdges& ie, size_t budget) {
  const bool can = K >= 2 && !eng->dbg_on && !eng->gp;          // debug captures name ONE chunk's buffers
  if (eng->n_lanes >= 2 && can) return 2;
  if (eng->n_lanes == 0 && can && eng->force_parts < 2 && eng->lanes_auto_edges > 0 && ie.etot >= eng->lanes_auto_edges &&
      ws_bytes(eng, eng->natoms, ie.emax) <= budget / 2)
    return 2;
  return 1;
}

// Amortised workspace (ABI v8).  Allocating device memory costs ~45 ms per GiB on this driver (it is cleared), so a workspace sized for the
// whole batch -- up to the 160 GiB cap: 7 s -- is only worth it for a run that lasts: a one-off finite-difference Hessian of a 500-atom
// system spent 11 of its 15 s allocating.  Chunks of ~320 k directed edges already run within 3 % of the largest ones (DESIGN.md section
// 7), so without a hint (umx_reserve_images, which announces a long run of known batches) the workspace starts at that size and grows to
// what the batch would like only once the engine has been evaluating for 8x as long as the larger allocation takes.
size_t amortised_budget(umx_engine* eng, long K, const ImageEdges& ie, size_t budget) {
  const double now = std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count();
  if (eng->t_first_eval < 0.0) eng->t_first_eval = now;
  if (eng->ws_eager || eng->hint_images != 0 || eng->gp || eng->dbg_on || eng->force_parts >= 2) return budget;
  const int N = eng->natoms;
  const long emax = std::max(1L, ie.emax);
  const long per = std::max(1L, (eng->ws_soft_edges + emax - 1) / emax);                      // images per chunk for ~ws_soft_edges
  const size_t want = ws_bytes(eng, per * N, per * (emax + emax / 20 + 64));
  const size_t cur = eng->cap_nodes > 0 ? ws_bytes(eng, eng->cap_nodes, eng->cap_edges) : 0;
  const size_t soft = std::min(budget, std::max(want, cur));
  const size_t full = std::min(budget, ws_bytes(eng, K * N, grown_edges(ie.etot)));
  return (full > soft && (now - eng->t_first_eval) >= 8.0 * 0.045 * (double)(full >> 20) / (double)(1 << 10)) ? full : soft;
}

// ---- chunk planning --------------------------------------------------------------------------------
// (img: [k0, k1) of every chunk; need_*: the largest chunk's)
struct Chunks { std::vector<std::pair<long, long>> img; long need_nodes = 0, need_edges = 0; };
// consecutive images, at most `cap` per chunk, each chunk's workspace within the budget
int plan_chunks(umx_engine* eng, long K, const ImageEdges& ie, long cap, size_t budget, Chunks& c) {
  const int N = eng->natoms;
  c = Chunks();
  // Several pinned references: image k is promised to be, bit for bit, its evaluation alone.  The GEMM producers negate the operand rows
  // of odd index (umx_edge.h, sign-alternating rows), so the rounding of an edge depends on the parity of its row in the chunk:
  // an image never starts at an odd row -- behind an odd number of edges the chunk ends.  (Alone, an image starts at row 0.)
  // umx_hvp asks for the same of every evaluation it makes, one pinned reference and unpinned images included: +v and -v of a base with
  // an odd edge count would otherwise sit on different parities, and a central difference divides that rounding by 2 * step.
  const bool even_rows = (eng->pin_on && eng->pin_refs > 1) || eng->hvp_rows;
  for (long k0 = 0; k0 < K;) {
    long k1 = k0, e = 0;
    while (k1 < K && (k1 - k0) < cap) {
      if (even_rows && (e & 1)) break;
      const long e2 = e + ie.per_image[k1];
      if (k1 > k0 && ws_bytes(eng, (k1 - k0 + 1) * N, e2) > budget) break;
      e = e2; ++k1;
    }
    if (ws_bytes(eng, (k1 - k0) * N, e) > budget)
      return fail(eng, UMX_ERR_CAPACITY, "one image (" + std::to_string(N) + " atoms, " + std::to_string(e) + " directed edges) needs " +
                                             std::to_string(ws_bytes(eng, N, e) >> 20) + " MiB of workspace, budget is " +
                                             std::to_string(budget >> 20) + " MiB: a structure of this size has to be evaluated in the graph-parallel mode, its edges "
                                             "partitioned over several GPUs (umx_gp_begin / umx_gp_step; uma_pysis(workers=<ranks>) under torch.distributed, one rank per GPU)");
    c.img.push_back({k0, k1});
    c.need_nodes = std::max(c.need_nodes, (k1 - k0) * N);
    c.need_edges = std::max(c.need_edges, e);
    k0 = k1;
  }
  return UMX_OK;
}

// ---- arena -----------------------------------------------------------------------------------------
// Make the arena hold `lanes` workspaces of the largest chunk (growing it when the chunks, or the umx_reserve_images hint, ask for
// more) and carve one view per lane; may fall back to one lane.  env_cap: UMX_MAX_CHUNK_IMAGES (0: unset).
int prepare_arena(umx_engine* eng, hipStream_t s, const ImageEdges& ie, const Chunks& c, long env_cap, size_t budget, int* lanes_io, WS (&wl)[2]) {
  const int N = eng->natoms;
  int lanes = *lanes_io;
  const long need_nodes = c.need_nodes, need_edges = c.need_edges;
  // umx_reserve_images: the caller announced batches of up to hint_images images -- size the workspace once for that many images of the
  // densest image at hand (+5 %) instead of growing it batch by batch (every growth re-allocates the whole region); ignored when it
  // does not fit the budget
  long hint_nodes = 0, hint_edges = 0;
  if (eng->hint_images > 0 && !eng->gp && lanes == 1) {
    long hint_img = eng->hint_images;                                       // (a chunk never holds more than UMX_MAX_CHUNK_IMAGES images)
    if (env_cap > 0) hint_img = std::min(hint_img, env_cap);
    hint_nodes = hint_img * N;
    hint_edges = hint_img * (ie.emax + ie.emax / 20 + 64);
    if ((hint_nodes <= eng->cap_nodes && hint_edges <= eng->cap_edges) || ws_bytes(eng, hint_nodes, hint_edges) > budget) hint_nodes = hint_edges = 0;
  }
  // (the hint alone triggers ONE allocation; after that it only enlarges a growth the batches themselves ask for -- otherwise every batch
  // whose densest image is a little denser than the last one's would re-allocate)
  const bool hint_now = eng->hint_applied != eng->hint_images && (hint_nodes > eng->cap_nodes || hint_edges > eng->cap_edges);
  if (eng->hint_images > 0 && (hint_nodes || hint_edges || eng->cap_nodes >= (long)eng->hint_images * N)) eng->hint_applied = eng->hint_images;
  if (need_nodes > eng->cap_nodes || need_edges > eng->cap_edges || hint_now) {
    long cn = std::max(std::max(need_nodes, hint_nodes), eng->cap_nodes), ce = std::max(std::max(grown_edges(need_edges), hint_edges), eng->cap_edges);
    size_t bytes = ws_bytes(eng, cn, ce);
    if (bytes > budget && (hint_nodes || hint_edges)) {      // hint and need combined overshoot: size for the need alone
      cn = std::max(need_nodes, eng->cap_nodes); ce = std::max(grown_edges(need_edges), eng->cap_edges);
      bytes = ws_bytes(eng, cn, ce);
    }
    if (bytes > budget) { ce = std::max(need_edges, 1L); bytes = ws_bytes(eng, cn, ce); }
    // one workspace per lane.  (After a change of plan kind the caps were cleared, not outgrown: an arena that holds the new kind's
    // workspace is carved anew and kept -- mode 1 may change kind at every call.)
    if (!(eng->arena_keep && lanes * bytes <= eng->arena_bytes)) CHK(grow_arena(eng, s, lanes * bytes));
    eng->arena_keep = false;
    eng->cap_nodes = cn; eng->cap_edges = ce;
  }
  long use_nodes = eng->cap_nodes, use_edges = eng->cap_edges;
  if (lanes == 2 && eng->arena_bytes < 2 * ws_bytes(eng, use_nodes, use_edges)) {
    // the arena was sized for ONE lane of larger chunks (an engine that has seen smaller batches, or one lane, before): two lanes of THIS
    // call's chunks may still fit it -- else one lane
    const long ce = grown_edges(need_edges);
    if (2 * ws_bytes(eng, need_nodes, ce) <= eng->arena_bytes) { use_nodes = need_nodes; use_edges = ce; }
    else lanes = 1;
  }
  const size_t lane_bytes = ws_bytes(eng, use_nodes, use_edges, eng->arena, &wl[0]);
  if (lanes == 2) ws_bytes(eng, use_nodes, use_edges, eng->arena + lane_bytes, &wl[1]);
  *lanes_io = lanes;
  return UMX_OK;
}

// ---- execution ---------------------------------------------------------------------------------------
// issue the chunks' plans: one after another on s, or in pairs on the two lanes
int run_chunks(umx_engine* eng, hipStream_t s, int lanes, const ImageEdges& ie, const Chunks& c, WS (&wl)[2], const PosPtr d_pos, double* d_energy, float* d_forces) {
  const int N = eng->natoms;
  int st = UMX_OK;
  auto plan_of = [&](size_t ci, int lane, Plan& P) {
    const long k0 = c.img[ci].first, k1 = c.img[ci].second;
    long e = 0;
    for (long k = k0; k < k1; ++k) e += ie.per_image[k];
    VirialOut vir;       // the partials' slots follow the image's position in the call: the two lanes never share one
    if (eng->vir_out && d_forces) { vir.out = eng->vir_out + k0 * 9; vir.part = eng->d_vir_part + k0 * eng->vir_slabs * 9; vir.slabs = eng->vir_slabs; }
    // (pinned graphs: every image has its reference's degrees; no candidate counts)
    plan_chunk(eng, wl[lane], d_pos.atom(k0 * N), (eng->pin_on ? eng->d_pin_deg : eng->d_deg_all) + k0 * N, eng->pin_on ? nullptr : eng->d_cand_all + k0 * N, k0, k1 - k0, e, d_energy + k0,
               d_forces ? d_forces + k0 * N * 3 : nullptr, P, vir);
  };
  if (lanes == 2) {          // chunks in pairs, one per lane, matrix segments alternating between the lanes (run_plans_alternating)
    // lane 1 starts after everything enqueued so far on the primary stream (degree pass, caller's work)
    HIPCHK(eng, hipEventRecord(eng->ev_fork, s));
    HIPCHK(eng, hipStreamWaitEvent(eng->stream2, eng->ev_fork, 0));
    // UMX_LANES_ONE_STREAM=1 (tests): both lanes' segments in the same alternating order on ONE stream -- the two-lane plan without any
    // concurrency (what results must be bitwise equal to; with real concurrency see NOTES.md section 5, item 14)
    hipStream_t sts[2] = {s, std::getenv("UMX_LANES_ONE_STREAM") ? s : eng->stream2};
    hipEvent_t tok[2] = {eng->ev_tok[0], eng->ev_tok[1]};
    for (size_t ci = 0; ci < c.img.size() && st == UMX_OK; ci += 2) {
      Plan P[2];
      plan_of(ci, 0, P[0]);
      if (ci + 1 < c.img.size()) {
        plan_of(ci + 1, 1, P[1]);
        eng->throttle = true;
        st = run_plans_alternating(eng, P, sts, tok);
        eng->throttle = false;
      } else {
        eng->stream = s;
        st = run_plan(eng, P[0]);
      }
    }
    eng->stream = s;
    // join: the primary stream continues only after lane 1 has drained
    HIPCHK(eng, hipEventRecord(eng->ev_join, eng->stream2));
    HIPCHK(eng, hipStreamWaitEvent(s, eng->ev_join, 0));
  } else {
    for (size_t ci = 0; ci < c.img.size() && st == UMX_OK; ++ci) {
      Plan P;
      plan_of(ci, 0, P);
      eng->stream = s;
      st = run_plan(eng, P);
    }
  }
  return st;
}

// Plan and run one evaluation with the kind of plan eng->rc_active names: budget, lanes, chunks (or partitions), arena, execution.
int evaluate_planned(umx_engine* eng, hipStream_t s, long K, const PosPtr d_pos, double* d_energy, float* d_forces, const ImageEdges& ie) {
  // cap_nodes / cap_edges say what the arena holds in ws_bytes of ONE kind of plan: after a change of kind it is carved (and sized) anew
  if (eng->arena_rc != eng->rc_active) { eng->cap_nodes = 0; eng->cap_edges = 0; eng->arena_rc = eng->rc_active; eng->arena_keep = true; }
  size_t budget = 0;
  CHK(workspace_budget(eng, ie, &budget));
  int lanes = choose_lanes(eng, K, ie, budget);
  budget = amortised_budget(eng, K, ie, budget / lanes);
  long env_cap = 0;
  if (const char* ev = std::getenv("UMX_MAX_CHUNK_IMAGES")) env_cap = std::atol(ev);
  long max_chunk = (K + lanes - 1) / lanes;          // at least `lanes` chunks so both streams have work
  if (env_cap > 0) max_chunk = std::min(max_chunk, env_cap);
  Chunks chunks;
  const int pst = eng->force_parts >= 2 ? UMX_ERR_CAPACITY : plan_chunks(eng, K, ie, max_chunk, budget, chunks);
  // (debug captures name ONE chunk's buffers: an image too large for one piece is not partitioned behind their back.  Partitions that were
  // ASKED for, UMX_FORCE_PARTS, run with captures on -- every partition captures under the same names, the last one's stay)
  if (pst == UMX_ERR_CAPACITY && !eng->gp && (!eng->dbg_on || eng->force_parts >= 2)) {
    if (eng->dbg_on) eng->dbg.clear();
    return eval_images_partitioned(eng, s, K, d_pos, d_energy, d_forces, budget * lanes, eng->err);
  }
  if (pst != UMX_OK) return pst;
  eng->last_parts = 0;
  if (lanes == 2 && chunks.img.size() > 1) {
    // the lanes work in pairs of chunks: an even number of chunks of (nearly) equal size, so that no chunk runs without a partner
    const long n_even = (long)((chunks.img.size() + 1) / 2 * 2);
    CHK(plan_chunks(eng, K, ie, (K + n_even - 1) / n_even, budget, chunks));
  }
  WS wl[2];
  CHK(prepare_arena(eng, s, ie, chunks, env_cap, budget, &lanes, wl));
  if (eng->dbg_on) eng->dbg.clear();
  eng->last_lanes = (lanes == 2 && chunks.img.size() > 1) ? 2 : 1;
  if (eng->gp) {
    // graph-parallel: record the plan of the one chunk and hand control back; umx_gp_step issues it segment by segment, pausing at
    // every exchange point.  The workspace view must outlive this call (the closures hold a reference to it).
    eng->gp_ws = std::make_unique<WS>(wl[0]);
    eng->gp_plan = std::make_unique<Plan>();
    // virial: this rank's share of W -- its edge list is exactly the edges whose target it owns -- taken behind k_force_edge, in the
    // segment in front of the force exchange; the share needs no exchange point of its own (the caller adds nine doubles per rank)
    VirialOut vir;
    if (eng->vir_out && d_forces) { vir.out = eng->vir_out; vir.part = eng->d_vir_part; vir.slabs = eng->vir_slabs; }
    plan_chunk(eng, *eng->gp_ws, d_pos, eng->d_deg_all, eng->d_cand_all, 0, 1, ie.per_image[0], d_energy, d_forces, *eng->gp_plan, vir);
    eng->gp_at = 0; eng->gp_stream = s;
    return UMX_OK;
  }
  CHK(run_chunks(eng, s, lanes, ie, chunks, wl, d_pos, d_energy, d_forces));
  HIPCHK(eng, hipEventRecord(eng->ev_done, s));
  return UMX_OK;
}

// Evaluate on `run_stream` (may be the legacy default stream 0).  eng->stream is swapped for the duration so that every
// helper launches there; it is restored on every exit path.
// d_virial: [n_images][9] float64 or nullptr (then nothing of umx_virial.h runs).  Graph-parallel entry (eng->gp): the degree pass
// below counts this rank's own edges only, so the partial slots are sized for the rank's share, and d_virial receives that share.
int energy_forces_on(umx_engine* eng, hipStream_t run_stream, int n_images, PosPtr d_pos, double* d_energy, float* d_forces,
                     double* d_virial = nullptr) {
  hipStream_t own = eng->stream;
  eng->stream = run_stream;
  eng->ran_on_caller = (run_stream != own);
  struct Restore { umx_engine* e; hipStream_t s; ~Restore() { e->stream = s; e->vir_out = nullptr; } } restore{eng, own};
  hipStream_t s = eng->stream;
  CHK(periodic_prepare(eng, s, n_images, &d_pos));     // periodic: from here on d_pos is the wrapped copy (only the graph kernels read positions)
  ImageEdges ie;
  CHK(degree_pass(eng, s, n_images, d_pos, ie));
  if (d_virial) {
    eng->vir_slabs = virial_slabs(ie.emax);
    CHK(virial_prepare(eng, s, n_images, eng->vir_slabs));
    eng->vir_out = d_virial;
  }
  // recompute plans: never in the multi-GPU graph-parallel mode, nor with debug captures (they name the stored buffers of every layer)
  const bool rc_can = !eng->gp && !eng->dbg_on;
  eng->rc_active = rc_can && eng->recompute == 2;
  int st = evaluate_planned(eng, s, n_images, d_pos, d_energy, d_forces, ie);
  if (st == UMX_ERR_CAPACITY && rc_can && eng->recompute == 1) {      // no stored plan fits, in one piece or in partitions
    eng->rc_active = true;
    st = evaluate_planned(eng, s, n_images, d_pos, d_energy, d_forces, ie);
  }
  if (st == UMX_OK) eng->last_recompute = eng->rc_active ? 1 : 0;
  return st;
}

void gp_clear(umx_engine* eng) { eng->gp_plan.reset(); eng->gp_ws.reset(); eng->gp_at = 0; eng->gp = false; }

}  // namespace
