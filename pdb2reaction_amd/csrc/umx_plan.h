// umx_plan.h -- host side, part 4 of 5: the launch plan of one chunk (plan_chunk: forward, readout, analytic reverse pass), the
// executors that issue plans on one stream or on two lanes, and one evaluation (energy_forces_on) as its phases -- degree pass, workspace
// budget, lane choice, amortised workspace size, chunk planning, the partitioned fallback for an oversized image, the arena, execution.
// Seg / Plan themselves are in umx_engine.h.
#pragma once

namespace {

// ---- radial MLP forward / backward -------------------------------------------------------------
// Each is split into its small layers (fp32 GEMMs + LayerNorm/SiLU kernels: "streaming" work) and the one large fc3 GEMM, so that
// the two-lane executor can treat the large GEMM as a matrix-pipe segment (Plan, umx_engine.h).
int radial_fwd_head(umx_engine* eng, const WS& w, const RadialW& r, int slot, long ne) {
  // one persistent kernel: gaussians -> fc1 -> LN+SiLU -> fc2 -> LN+SiLU -> the fc3 operand (fp16 planes / float32 quad-row blocks of the
  // split modes, or fp32 rows in w.ra); the intermediate rows never reach HBM
  const bool planes = eng->prec.planes && eng->planes.count(r.w3);
  const unsigned tiles = nblk(ne, 64);                      // two 32-row MFMA tiles per workgroup tile, two workgroups per CU
  const dim3 grid(vgrid(eng, tiles < 512u ? tiles : 512u));
  ProfRec* pr;
  CHK(prof_open(eng, &pr, 2.0 * ne * ((double)NG * RH + (double)RH * RH), -1, ne, RH, NG + RH));
#define UMX_RH_LAUNCH(Q, OUT) hipLaunchKernelGGL((k_radial_head<Q>), grid, dim3(256), 0, eng->stream, w.evec, w.ez, eng->gcoef, eng->d_gmu, r.w1g, r.tsd, r.ttd, r.ln1w, \
                                                 r.ln1b, r.w2, r.b2, r.ln2w, r.ln2b, w.h1pre[slot], w.h2pre[slot], (void*)(OUT), ne, eng->odd_sign)
  if (planes && eng->prec.fwd_fmt == 1) UMX_RH_LAUNCH(2, w.a2pl); else if (planes) UMX_RH_LAUNCH(4, w.a2pl); else UMX_RH_LAUNCH(0, w.ra);
#undef UMX_RH_LAUNCH
  CHK(prof_close(eng, pr));
  HIPCHK(eng, hipGetLastError());
  return UMX_OK;
}
int radial_fwd_fc3(umx_engine* eng, const WS& w, const RadialW& r, long ne, float* rad_out) {
  if (eng->prec.planes && eng->planes.count(r.w3)) return gemm_pl(eng, 0, FWD, w.a2pl, RH, 0, 0, r.w3, 0, r.b3, rad_out, r.out, 0, 0, ne, r.out, RH, 1.0f);
  return gemm_plain(eng, w.ra, RH, 0, r.w3, RH, r.b3, rad_out, r.out, 0, ne, r.out, RH);
}
int radial_fwd(umx_engine* eng, const WS& w, const RadialW& r, int slot, long ne, float* rad_out) {
  CHK(radial_fwd_head(eng, w, r, slot, ne));
  if (eng->dbg_on && !eng->prec.planes) DBG("a2." + std::to_string(slot), w.ra, ne * RH);       // (debug) fp32 mode: the fc3 operand rows behind the head
  return radial_fwd_fc3(eng, w, r, ne, rad_out);
}

int radial_bwd_fc3(umx_engine* eng, const WS& w, const RadialW& r, long ne, const float* grad, const unsigned short* gradpl, bool f32rows = false) {
  if (gradpl) return gemm_pl(eng, 0, REV, gradpl, r.out, 0, 0, r.w3T, 0, nullptr, w.e128a, RH, 0, 0, ne, RH, r.out, 1.0f, f32rows);
  return gemm_plain(eng, grad, r.out, 0, r.w3T, r.out, nullptr, w.e128a, RH, 0, ne, RH, r.out);
}
int radial_bwd_tail(umx_engine* eng, const WS& w, const RadialW& r, int slot, long ne) {
  // one persistent kernel: LN+SiLU bwd -> fc2^T -> LN+SiLU bwd -> fc1^T -> dE/dd through the gaussians (accumulated into dedd_rad)
  const unsigned tiles = nblk(ne, 64);
  const dim3 grid(vgrid(eng, tiles < 512u ? tiles : 512u));
  ProfRec* pr;
  CHK(prof_open(eng, &pr, 2.0 * ne * ((double)NG * RH + (double)RH * RH), -1, ne, RH, NG + RH));
  const std::string t = slot == NL ? ".deg" : "." + std::to_string(slot);
  DBG("g_a2" + t, w.e128a, ne * RH);           // (debug) the output of fc3^T, the tail's input
  hipLaunchKernelGGL(k_radial_tail, grid, dim3(256), 0, eng->stream, w.e128a, w.h2pre[slot], w.h1pre[slot], w.evec, eng->gcoef, eng->d_gmu, r.ln2w, r.ln2b, r.ln1w, r.ln1b,
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
// vir.out != nullptr: the chunk's final segment also takes the virial of its images (umx_virial.h)
// img0: the index within the call of the chunk's first image (d_pos, d_deg, d_cand and the outputs start there; per-image cells are
// indexed by it)
void plan_chunk(umx_engine* eng, WS& w, const PosPtr d_pos, const int* d_deg, const int* d_cand, long img0, long nimg, long ne, double* d_energy,
                float* d_forces, Plan& P, const VirialOut vir = VirialOut()) {
  const int N = eng->natoms;
  const long nn = nimg * N;
  const float rc2 = eng->cutoff * eng->cutoff;
  const dim3 B256(256);
  const bool pl = eng->prec.planes;
  const bool gp = eng->gp;                                       // graph-parallel: partial sums over this rank's edges + exchange points
  const bool may_trunc = eng->may_truncate;                      // some node of this call has more candidates than max_neigh (known on the host)
  const bool rc = eng->rc_active && d_forces != nullptr;         // recompute plan: one activation slot (carve_acts), replayed layer by layer in the reverse pass
  const bool fused_rev = eng->prec.planes || !eng->dbg_on;     // k_modrot_bwd_pl produces g_xn itself (fp32 mode with debug captures: the unfused kernels, which expose xrot / g_xrot)
  const long g_lo = gp ? eng->gp_lo : 0, g_hi = gp ? eng->gp_hi : nn;
  // pinned graph: the reference edges this chunk replays per image -- all of them, or the contiguous rows [g_lo, g_hi) of a partition
  const bool pinned = eng->pin_on;
  const long pin_e0 = pinned && gp ? eng->pin_row[g_lo] : 0, pin_ecnt = pinned ? (gp ? eng->pin_row[g_hi] - pin_e0 : eng->pin_edges) : 0;
  // every closure reads eng->stream when it RUNS (the executor points it at the lane's stream)
  // K1 graph, K4 + K5
  P.stream([=, &w]() -> int {
    hipStream_t s = eng->stream;
    hipLaunchKernelGGL(k_scan, dim3(1), dim3(1024), 0, s, d_deg, nn, w.row_ptr, w.stats);
    if (pinned) launch_graph_replay(eng, s, d_pos, nimg, pin_e0, pin_ecnt, w.esrc, w.edst, w.evec, img0);
    else launch_graph_fill(eng, s, may_trunc, d_pos, nn, d_cand, w.row_ptr, w.esrc, w.edst, w.evec, g_lo, g_hi, img0);
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
      if (eng->prec.planes && eng->prec.fwd_fmt == 3) DBG("a2q.deg", reinterpret_cast<const float*>(w.a2pl), (ne + 3) / 4 * 4 * RH);
      // (debug) the fast mode's operand: the raw halves of the two-plane "Q2H" blocks (umx_kernels_pl.h), 4-row-padded rows x columns x 2;
      // fp32 mode: the float32 rows of the fc3 operand -- tests/test_gpu_forward_links.py
      if (eng->prec.planes && eng->prec.fwd_fmt == 1) DBG("a2h.deg", w.a2pl, (ne + 3) / 4 * 4 * RH * 2);
      if (!eng->prec.planes) DBG("a2.deg", w.ra, ne * RH);
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

  // The edge pipeline of layer i's forward pass (radial MLP, gather / rotate / modulate, conv 1, gate, conv 2 -> rad, hg, msg, h1pre,
  // h2pre of the layer), led by the layer's first norm.  replay (recompute plans, reverse pass): the same segments from the STORED node
  // input xn[i] -- the norm, like everything node-level, is not issued again; no kernel of the pipeline writes node state.
  auto edge_fwd = [&](int i, bool replay) {
    const LayerW* Lp = &eng->lw[i];
    float* xin = w.xs[2 * i];
    if (ne > 0 && pl) {
      P.stream([=, &w]() -> int {
        hipStream_t s = eng->stream;
        if (!replay) hipLaunchKernelGGL(k_norm_fwd, dim3(nblk(nn, 4)), B256, 0, s, xin, Lp->n1w, Lp->n1b, eng->d_sysemb, w.xn[i], nn);
        return radial_fwd_head(eng, w, Lp->rad, i, ne);
      });
      P.matrix([=, &w]() -> int {
        if (eng->prec.fwd_fmt == 3) DBG("a2q." + std::to_string(i), reinterpret_cast<const float*>(w.a2pl), (ne + 3) / 4 * 4 * RH);
        if (eng->prec.fwd_fmt == 1) DBG("a2h." + std::to_string(i), w.a2pl, (ne + 3) / 4 * 4 * RH * 2);
        return radial_fwd_fc3(eng, w, Lp->rad, ne, w.rad[i]);
      });
      P.stream([=, &w]() -> int {
        hipStream_t s = eng->stream;
        if (eng->prec.fwd_fmt == 1) hipLaunchKernelGGL(k_gather_rotate_mod_q3<1>, dim3(vgrid(eng, (nblk(ne, 4) + 7) / 8 * 8)), B256, 0, s, w.xn[i], w.esrc, w.edst, w.frame, w.rad[i], w.y1pl, ne, eng->odd_sign);
        else hipLaunchKernelGGL(k_gather_rotate_mod_q3<3>, dim3(vgrid(eng, (nblk(ne, 4) + 7) / 8 * 8)), B256, 0, s, w.xn[i], w.esrc, w.edst, w.frame, w.rad[i], w.y1pl, ne, eng->odd_sign);
        HIPCHK(eng, hipGetLastError());
        return UMX_OK;
      });
      // SO(2) conv 1 on the pre-modulated planes -> hg = [gate | hpre]
      P.matrix([=, &w]() -> int {
        if (eng->prec.fwd_fmt == 3) DBG("y1q." + std::to_string(i), reinterpret_cast<const float*>(w.y1pl), (ne + 3) / 4 * 4 * XROT);     // (debug) conv-1's A operand as the GEMMs read it
        if (eng->prec.fwd_fmt == 1) DBG("y1h." + std::to_string(i), w.y1pl, (ne + 3) / 4 * 4 * XROT * 2);
        CHK(gemm_pl(eng, 0, FWD, w.y1pl, XROT, 0, 0, Lp->c1m0, 0, Lp->c1m0b, w.hg[i], HG, 0, 0, ne, 640, 768, 1.0f));
        CHK(gemm_pl(eng, 1, FWD, w.y1pl, XROT, 768, 1280, Lp->c1m1, 256, nullptr, w.hg[i], HG, 640, 896, ne, 256, 512, 1.0f));
        return gemm_pl(eng, 1, FWD, w.y1pl, XROT, 1792, 2048, Lp->c1m2, 128, nullptr, w.hg[i], HG, 1152, 1280, ne, 128, 256, 1.0f);
      });
      P.stream([=, &w]() -> int {
        hipStream_t s = eng->stream;
        if (eng->prec.fwd_fmt == 1) hipLaunchKernelGGL(k_gate_edge_fwd_q3<1>, dim3(vgrid(eng, nblk(ne, 8))), B256, 0, s, w.hg[i], w.hidpl, ne, eng->odd_sign);
        else hipLaunchKernelGGL(k_gate_edge_fwd_q3<3>, dim3(vgrid(eng, nblk(ne, 8))), B256, 0, s, w.hg[i], w.hidpl, ne, eng->odd_sign);
        HIPCHK(eng, hipGetLastError());
        return UMX_OK;
      });
      P.matrix([=, &w]() -> int {
        if (eng->prec.fwd_fmt == 3) DBG("hidq." + std::to_string(i), reinterpret_cast<const float*>(w.hidpl), (ne + 3) / 4 * 4 * ROW);      // (debug) conv-2's A operand
        if (eng->prec.fwd_fmt == 1) DBG("hidh." + std::to_string(i), w.hidpl, (ne + 3) / 4 * 4 * ROW * 2);
        CHK(gemm_pl(eng, 0, FWD, w.hidpl, ROW, 0, 0, Lp->c2m0, 0, Lp->c2m0b, w.msg[i], ROW, 0, 0, ne, 384, 384, 1.0f));
        CHK(gemm_pl(eng, 1, FWD, w.hidpl, ROW, 384, 640, Lp->c2m1, 256, nullptr, w.msg[i], ROW, 384, 640, ne, 256, 256, 1.0f));
        return gemm_pl(eng, 1, FWD, w.hidpl, ROW, 896, 1024, Lp->c2m2, 128, nullptr, w.msg[i], ROW, 896, 1024, ne, 128, 128, 1.0f);
      });
    } else {
      P.stream([=, &w]() -> int {
        hipStream_t s = eng->stream;
        const LayerW& L = *Lp;
        if (!replay) hipLaunchKernelGGL(k_norm_fwd, dim3(nblk(nn, 4)), B256, 0, s, xin, L.n1w, L.n1b, eng->d_sysemb, w.xn[i], nn);
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
  };
  for (int i = 0; i < NL; ++i) {
    const LayerW* Lp = &eng->lw[i];
    float* xin = w.xs[2 * i];
    float* xmid = w.xs[2 * i + 1];
    float* xout = w.xs[2 * i + 2];
    edge_fwd(i, false);
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
      if (!eng->prec.planes) { DBG("xrot" + t, w.xrot, ne * XROT); DBG("hid" + t, w.hid, ne * ROW); }
      DBG("hg" + t, w.hg[i], ne * HG); DBG("msg" + t, w.msg[i], ne * ROW); DBG("xmid" + t, xmid, nn * ROW);
      // K8 atom-wise
      hipLaunchKernelGGL(k_norm_fwd, dim3(nblk(nn, 4)), B256, 0, s, xmid, L.n2w, L.n2b, (const double*)nullptr, w.xn2, nn);
      if (eng->ff_grid) {
        // GridAtomwise: to-grid -> Linear, SiLU, Linear, SiLU, Linear over the channels of every grid point -> from-grid (+ residual).
        // The hidden pre-activations stay resident for the reverse pass; the SiLUs are applied while the next GEMM stages its A operand.
        const int G = eng->grid_G;
        const long ng = nn * G;
        hipLaunchKernelGGL(k_grid_expand, dim3(nblk(nn, 4)), B256, 0, s, w.xn2, eng->to_grid, G, w.gridA, nn);
        if (eng->dbg_on) DBG("gridin" + t, w.gridA, ng * C);      // (debug) the to-grid projection: gridA is overwritten by the third GEMM
        CHK(gemm_grid(eng, w.gridA, C, 0, L.g1w, C, L.g1b, w.ffg1[i], H, 0, ng, H, C));
        CHK(gemm_grid(eng, w.ffg1[i], H, 0, L.g2w, H, L.g2b, w.ffg2[i], H, 0, ng, H, H, A_SILU));
        CHK(gemm_grid(eng, w.ffg2[i], H, 0, L.g3w, H, L.g3b, w.gridA, C, 0, ng, C, H, A_SILU));
        hipLaunchKernelGGL(k_grid_contract, dim3(nblk(nn, 4)), B256, 0, s, w.gridA, eng->from_grid, G, xmid, xout, nn);
        HIPCHK(eng, hipGetLastError());
        if (eng->dbg_on) DBG("gridout" + t, w.gridA, ng * C);     // (debug) the grid MLP's output, from-grid's input
        DBG("xn2" + t, w.xn2, nn * ROW); DBG("ffg1" + t, w.ffg1[i], ng * H); DBG("ffg2" + t, w.ffg2[i], ng * H); DBG("x" + t, xout, nn * ROW);
        return UMX_OK;
      }
      CHK(gemm_node(eng, w.xn2, ROW, 0, L.smlp, C, L.smlpb, w.gspre[i], 2 * H, 0, nn, 2 * H, C));
      CHK(so3_linear(eng, w.xn2, L.l1w, L.l1b, w.ffh[i], nn, nullptr));
      hipLaunchKernelGGL(k_gate_node_fwd, dim3(nblk(nn * H, 256)), B256, 0, s, w.ffh[i], w.gspre[i], w.ffhg, nn);
      CHK(so3_linear(eng, w.ffhg, L.l2w, L.l2b, xout, nn, xmid));
      HIPCHK(eng, hipGetLastError());
      DBG("xn2" + t, w.xn2, nn * ROW); DBG("gspre" + t, w.gspre[i], nn * 2 * H); DBG("ffh" + t, w.ffh[i], nn * ROW); DBG("x" + t, xout, nn * ROW);
      if (eng->dbg_on) DBG("ffhg" + t, w.ffhg, nn * ROW);         // (debug) the gated hidden rows: one buffer for all layers
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
    if (eng->dbg_on) DBG("xf", w.xf, nn * ROW);
    if (!d_forces) return UMX_OK;
    // ---------------- K10: analytic reverse pass ----------------
    if (ne > 0) {
      HIPCHK(eng, hipMemsetAsync(w.dedd, 0, ne * sizeof(float), s));
      HIPCHK(eng, hipMemsetAsync(w.dedd_rad, 0, ne * sizeof(float), s));
      HIPCHK(eng, hipMemsetAsync(w.tau, 0, ne * 4 * sizeof(float), s));
      HIPCHK(eng, hipMemsetAsync(w.tau2, 0, ne * 4 * sizeof(float), s));
    }
    // (debug) every capture of the reverse node links sits directly behind the launch that writes its buffer: n128a / n128b, G0 / G1 / G2,
    // ggs and gridA / gridB are reused from link to link
    hipLaunchKernelGGL(k_silu_bwd, dim3(nblk(nn * H, 256)), B256, 0, s, eng->e4, 0L, w.pre2, w.n128a, nn, H);
    if (eng->dbg_on) DBG("g_pre2", w.n128a, nn * H);
    CHK(gemm_node(eng, w.n128a, H, 0, eng->e2T, H, nullptr, w.n128b, H, 0, nn, H, H));
    if (eng->dbg_on) DBG("g_sil1", w.n128b, nn * H);              // dE / d silu(pre1)
    hipLaunchKernelGGL(k_silu_bwd, dim3(nblk(nn * H, 256)), B256, 0, s, w.n128b, (long)H, w.pre1, w.n128a, nn, H);
    if (eng->dbg_on) DBG("g_pre1", w.n128a, nn * H);
    HIPCHK(eng, hipMemsetAsync(w.G1, 0, nn * ROW * sizeof(float), s));
    CHK(gemm_node(eng, w.n128a, H, 0, eng->e0T, H, nullptr, w.G1, ROW, 0, nn, C, H));
    if (eng->dbg_on) DBG("g_xf", w.G1, nn * ROW);                 // the whole row: the columns of l > 0 must still be zero
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
    // recompute plan: the activation slot holds another layer (or, between exchange points, another partition): replay this layer's
    // forward edge pipeline into it first.  Every transient operand is free here: the reverse segments of layer i + 1 are complete.
    // (One piece: the slot still holds layer NL - 1 when the reverse pass starts.)
    if (rc && ne > 0 && (gp || i != NL - 1)) edge_fwd(i, true);
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
        if (eng->dbg_on) DBG("g_gridout" + t, w.gridA, ng * C);
        CHK(gemm_grid(eng, w.gridA, C, 0, L.g3T, C, nullptr, w.gridB, H, 0, ng, H, C));
        if (eng->dbg_on) DBG("g_gsil2" + t, w.gridB, ng * H);       // dE / d silu(ffg2)
        hipLaunchKernelGGL(k_silu_bwd, dim3(nblk(ng * H, 256)), B256, 0, s, w.gridB, (long)H, w.ffg2[i], w.gridA, ng, H);
        if (eng->dbg_on) DBG("g_ffg2" + t, w.gridA, ng * H);
        CHK(gemm_grid(eng, w.gridA, H, 0, L.g2T, H, nullptr, w.gridB, H, 0, ng, H, H));
        if (eng->dbg_on) DBG("g_gsil1" + t, w.gridB, ng * H);       // dE / d silu(ffg1)
        hipLaunchKernelGGL(k_silu_bwd, dim3(nblk(ng * H, 256)), B256, 0, s, w.gridB, (long)H, w.ffg1[i], w.gridA, ng, H);
        if (eng->dbg_on) DBG("g_ffg1" + t, w.gridA, ng * H);
        CHK(gemm_grid(eng, w.gridA, H, 0, L.g1T, H, nullptr, w.gridB, C, 0, ng, C, H));
        if (eng->dbg_on) DBG("g_gridin" + t, w.gridB, ng * C);
        hipLaunchKernelGGL(k_grid_contract, dim3(nblk(nn, 4)), B256, 0, s, w.gridB, eng->to_grid, G, (const float*)nullptr, w.G1, nn);     // G1 = g_xn2
        if (eng->dbg_on) DBG("g_xn2" + t, w.G1, nn * ROW);
      } else {
      CHK(so3_linear(eng, w.G0, L.l2T, nullptr, w.G1, nn, nullptr));                         // G1 = g_ffhg
      if (eng->dbg_on) DBG("g_ffhg" + t, w.G1, nn * ROW);
      hipLaunchKernelGGL(k_gate_node_bwd, dim3(nblk(nn * H, 256)), B256, 0, s, w.G1, w.ffh[i], w.gspre[i], w.G2, w.ggs, nn);
      if (eng->dbg_on) { DBG("g_ffh" + t, w.G2, nn * ROW); DBG("g_gs" + t, w.ggs, nn * 2 * H); }
      CHK(so3_linear(eng, w.G2, L.l1T, nullptr, w.G1, nn, nullptr));                         // G1 = g_xn2
      if (eng->dbg_on) DBG("g_xn2a" + t, w.G1, nn * ROW);         // before the scalar MLP's share lands in the l = 0 columns
      CHK(gemm_node(eng, w.ggs, 2 * H, 0, L.smlpT, 2 * H, nullptr, w.G1, ROW, 0, nn, C, 2 * H, A_PLAIN, 1, 0, 0, w.G1, ROW, 0, 0));
      if (eng->dbg_on) DBG("g_xn2" + t, w.G1, nn * ROW);
      }
      hipLaunchKernelGGL(k_norm_bwd, dim3(nblk(nn, 4)), B256, 0, s, w.G1, xmid, L.n2w, w.G0, w.G2, nn);   // G2 = g_xmid
      HIPCHK(eng, hipGetLastError());
      DBG("g_xmid" + t, w.G2, nn * ROW);
      if (ne > 0 && eng->prec.planes)
      {
        if (eng->prec.rev_quad()) hipLaunchKernelGGL(k_rotate_back_bwd_q3<3>, dim3(vgrid(eng, (nblk(ne, 4) + 7) / 8 * 8)), B256, 0, s, w.G2, w.msg[i], w.frame, w.edst, w.gmsgpl, w.dedd, w.tau, ne, eng->odd_sign);
        else hipLaunchKernelGGL(k_rotate_back_bwd_pl<2>, dim3(vgrid(eng, (nblk(ne, 4) + 7) / 8 * 8)), B256, 0, s, w.G2, w.msg[i], w.frame, w.edst, w.gmsgpl, w.dedd, w.tau, ne, eng->odd_sign);
        // (debug) conv-2^T's A operand as the GEMMs read it: float32 quad-row blocks (bf16x3) or two PL planes (split-bf16); odd rows negated
        if (eng->prec.rev_quad()) DBG("gmsgq" + t, reinterpret_cast<const float*>(w.gmsgpl), (ne + 3) / 4 * 4 * ROW);
        else DBG("gmsgpl" + t, w.gmsgpl, ne * ROW * 2);
      }
      HIPCHK(eng, hipGetLastError());
      return UMX_OK;
    });
    if (ne > 0 && pl) {
      P.matrix([=, &w]() -> int {
        CHK(gemm_pl(eng, 0, REV, w.gmsgpl, ROW, 0, 0, Lp->c2m0T, 0, nullptr, w.hid, ROW, 0, 0, ne, 384, 384, 1.0f));
        CHK(gemm_pl(eng, 1, REV, w.gmsgpl, ROW, 384, 640, Lp->c2m1T, 256, nullptr, w.hid, ROW, 384, 640, ne, 256, 256, -1.0f));
        return gemm_pl(eng, 1, REV, w.gmsgpl, ROW, 896, 1024, Lp->c2m2T, 128, nullptr, w.hid, ROW, 896, 1024, ne, 128, 128, -1.0f);
      });
      P.stream([=, &w]() -> int {
        hipStream_t s = eng->stream;
        DBG("g_hid." + std::to_string(i), w.hid, ne * ROW);
        if (eng->prec.rev_quad()) hipLaunchKernelGGL(k_gate_edge_bwd_q3<3>, dim3(vgrid(eng, nblk(ne, 8))), B256, 0, s, w.hid, w.hg[i], w.ghgpl, ne, eng->odd_sign);
        else hipLaunchKernelGGL(k_gate_edge_bwd_pl<2>, dim3(vgrid(eng, nblk(ne * (H / 4), 256))), B256, 0, s, w.hid, w.hg[i], w.ghgpl, ne, eng->odd_sign);
        HIPCHK(eng, hipGetLastError());
        // (debug) conv-1^T's A operand, in the format of gmsgq / gmsgpl
        if (eng->prec.rev_quad()) DBG("ghgq." + std::to_string(i), reinterpret_cast<const float*>(w.ghgpl), (ne + 3) / 4 * 4 * HG);
        else DBG("ghgpl." + std::to_string(i), w.ghgpl, ne * HG * 2);
        return UMX_OK;
      });
      P.matrix([=, &w]() -> int {
        CHK(gemm_pl(eng, 0, REV, w.ghgpl, HG, 0, 0, Lp->c1m0T, 0, nullptr, w.gy1, XROT, 0, 0, ne, 768, 640, 1.0f));
        CHK(gemm_pl(eng, 1, REV, w.ghgpl, HG, 640, 896, Lp->c1m1T, 512, nullptr, w.gy1, XROT, 768, 1280, ne, 512, 256, -1.0f));
        return gemm_pl(eng, 1, REV, w.ghgpl, HG, 1152, 1280, Lp->c1m2T, 256, nullptr, w.gy1, XROT, 1792, 2048, ne, 256, 128, -1.0f);
      });
      // (a matrix-token segment although it is HBM-bound: at 240 VGPRs its waves cannot share a SIMD with a GEMM wave, so beside
      //  the other lane's GEMM it would only take CUs away from it; the other lane's throttled stream kernels do fit beside it)
      P.matrix([=, &w]() -> int {
        hipStream_t s = eng->stream;
        const std::string t = "." + std::to_string(i);
        DBG("g_y1" + t, w.gy1, ne * XROT);        // (debug) conv-1^T's output
        // one node-centric kernel: modulation backward + rotate-back + segmented sum (g_xrot stays in registers); g_rad as float32 rows
        // (sign-alternating; split by the fc3^T GEMM in registers) in the bf16x3 mode, as two PL bf16 planes in the 16-bit-reverse modes
        if (eng->prec.rev_quad()) hipLaunchKernelGGL(k_modrot_bwd_pl<0>, dim3((unsigned)nn), B256, 0, s, w.gy1, w.xn[i], w.frame, w.rad[i], w.row_ptr, w.out_ptr, w.out_edge,
                                            w.gradpl, w.tau, w.tau2, w.G1, nn, eng->odd_sign);
        else hipLaunchKernelGGL(k_modrot_bwd_pl<2>, dim3((unsigned)nn), B256, 0, s, w.gy1, w.xn[i], w.frame, w.rad[i], w.row_ptr, w.out_ptr, w.out_edge,
                                w.gradpl, w.tau, w.tau2, w.G1, nn, eng->odd_sign);
        HIPCHK(eng, hipGetLastError());
        // (debug) fc3^T's A operand: float32 rows (bf16x3) or two PL planes (split-bf16); odd rows negated
        if (eng->prec.rev_quad()) DBG("gradq" + t, reinterpret_cast<const float*>(w.gradpl), ne * RAD);
        else DBG("gradpl" + t, w.gradpl, ne * RAD * 2);
        return UMX_OK;
      });
      P.matrix([=, &w]() -> int { return radial_bwd_fc3(eng, w, Lp->rad, ne, nullptr, w.gradpl, eng->prec.rev_quad()); });
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
      if (rc) {      // recompute plan: the edge-degree link's radial MLP again (h1pre / h2pre / rad_deg of the slot), not its node sum
        CHK(radial_fwd_head(eng, w, eng->rdeg, NL, ne));
        CHK(radial_fwd_fc3(eng, w, eng->rdeg, ne, w.rad_deg));
      }
      // split path: the gradient of the edge-degree radial output goes straight into the PL planes of the fc3^T GEMM (gmsgpl is free here)
      const bool dpl = eng->prec.planes && eng->planes.count(eng->rdeg.w3T) != 0;
      if (dpl && eng->prec.rev_planes == 3) hipLaunchKernelGGL((k_rotate_back_bwd<3, 3>), dim3(nblk(ne, 4)), B256, 0, s, w.G0, w.rad_deg, w.frame, w.edst,
                                                          reinterpret_cast<float*>(w.gmsgpl), w.dedd, w.tau, ne, DEG_RESCALE, eng->odd_sign);
      else if (dpl) hipLaunchKernelGGL((k_rotate_back_bwd<3, 2>), dim3(nblk(ne, 4)), B256, 0, s, w.G0, w.rad_deg, w.frame, w.edst,
                                       reinterpret_cast<float*>(w.gmsgpl), w.dedd, w.tau, ne, DEG_RESCALE, eng->odd_sign);
      if (dpl) DBG("gradpl.deg", w.gmsgpl, ne * 3 * C * eng->prec.rev_planes);      // (debug) the PL planes of the edge-degree fc3^T operand
      else hipLaunchKernelGGL(k_rotate_back_bwd<3>, dim3(nblk(ne, 4)), B256, 0, s, w.G0, w.rad_deg, w.frame, w.edst, w.gmsg, w.dedd, w.tau, ne,
                              DEG_RESCALE);
      CHK(radial_bwd(eng, w, eng->rdeg, NL, ne, w.gmsg, dpl ? w.gmsgpl : nullptr));
      if (fused_rev) hipLaunchKernelGGL(k_add4, dim3(nblk(ne, 256)), B256, 0, s, w.tau, w.tau2, ne);
      hipLaunchKernelGGL(k_force_edge, dim3(nblk(ne, 256)), B256, 0, s, w.dedd, w.dedd_rad, w.tau, w.frame, w.evec, w.gvec, ne);
    }
    hipLaunchKernelGGL(k_force_node, dim3(nblk(nn, 4)), B256, 0, s, w.gvec, w.row_ptr, w.out_ptr, w.out_edge, (float)eng->rmsd, d_forces, nn);
    HIPCHK(eng, hipGetLastError());
    if (vir.out) CHK(virial_launch(eng, w, vir, nimg, ne));       // (a partition: before the next one overwrites the shared gvec)
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

// directed edges per image of the batch at hand, and what the planning below asks of them
// (per_image: [K], the largest degree behind them; emax / etot: the largest image's edges, all edges)
struct ImageEdges { std::vector<int> per_image; long emax = 0, etot = 0; };

// degrees of every node of every image, per-image edge totals; sets last_edges / last_maxdeg / may_truncate
int degree_pass(umx_engine* eng, hipStream_t s, long K, const PosPtr d_pos, ImageEdges& ie) {
  const int N = eng->natoms;
  const long nt = K * N;
  if (eng->pin_on) {
    // pinned graph: every image has the reference's edges; nothing is launched and nothing read back.  (Only a call of more images
    // than any before it extends the repeated degrees k_scan reads.)
    if (eng->pin_deg_imgs < K) {
      std::vector<int> rep((size_t)nt);
      for (long k = 0; k < K; ++k) std::copy(eng->pin_deg.begin(), eng->pin_deg.end(), rep.begin() + k * N);
      CHK(grow(eng, eng->pin_deg_imgs, K, {s, eng->stream2}, {DevBuf(eng->d_pin_deg, (size_t)nt)}));
      HIPCHK(eng, hipMemcpy(eng->d_pin_deg, rep.data(), rep.size() * sizeof(int), hipMemcpyHostToDevice));
    }
    ie.per_image.assign((size_t)K + 1, (int)eng->pin_edges);
    ie.per_image[K] = eng->pin_maxdeg;
    eng->last_maxdeg = eng->pin_maxdeg;
    eng->may_truncate = false;
    ie.emax = eng->pin_edges; ie.etot = K * eng->pin_edges;
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
    // pinned graph: partition p takes the rows [lo, hi) of the reference -- its degrees there, zero elsewhere -- and the host knows the counts
    cnt.assign((size_t)P + 1, 0);
    for (int p = 0; p < P; ++p) {
      lo[p] = (long)N * p / P; hi[p] = (long)N * (p + 1) / P;
      int* deg = eng->d_part_deg + (size_t)(2 * p) * N;
      HIPCHK(eng, hipMemsetAsync(deg, 0, (size_t)N * sizeof(int), s));
      if (hi[p] > lo[p]) HIPCHK(eng, hipMemcpyAsync(deg + lo[p], eng->d_pin_deg + lo[p], (size_t)(hi[p] - lo[p]) * sizeof(int), hipMemcpyDeviceToDevice, s));
      cnt[p] = (int)(eng->pin_row[hi[p]] - eng->pin_row[lo[p]]);
    }
    cnt[P] = eng->pin_maxdeg;
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
  const size_t full = std::min(budget, ws_bytes(eng, K * N, ie.etot + ie.etot / 50 + 1024));
  return (full > soft && (now - eng->t_first_eval) >= 8.0 * 0.045 * (double)(full >> 20) / 1024.0) ? full : soft;
}

// ---- chunk planning --------------------------------------------------------------------------------
// (img: [k0, k1) of every chunk; need_*: the largest chunk's)
struct Chunks { std::vector<std::pair<long, long>> img; long need_nodes = 0, need_edges = 0; };
// consecutive images, at most `cap` per chunk, each chunk's workspace within the budget
int plan_chunks(umx_engine* eng, long K, const ImageEdges& ie, long cap, size_t budget, Chunks& c) {
  const int N = eng->natoms;
  c = Chunks();
  for (long k0 = 0; k0 < K;) {
    long k1 = k0, e = 0;
    while (k1 < K && (k1 - k0) < cap) {
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
    long cn = std::max(std::max(need_nodes, hint_nodes), eng->cap_nodes), ce = std::max(std::max(need_edges + need_edges / 50 + 1024, hint_edges), eng->cap_edges);
    size_t bytes = ws_bytes(eng, cn, ce);
    if (bytes > budget && (hint_nodes || hint_edges)) {      // hint and need combined overshoot: size for the need alone
      cn = std::max(need_nodes, eng->cap_nodes); ce = std::max(need_edges + need_edges / 50 + 1024, eng->cap_edges);
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
    const long ce = need_edges + need_edges / 50 + 1024;
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
    // (pinned graph: every image has the reference's degrees -- the repeated copy from its start; no candidate counts)
    plan_chunk(eng, wl[lane], d_pos.atom(k0 * N), eng->pin_on ? eng->d_pin_deg : eng->d_deg_all + k0 * N, eng->pin_on ? nullptr : eng->d_cand_all + k0 * N, k0, k1 - k0, e, d_energy + k0,
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
