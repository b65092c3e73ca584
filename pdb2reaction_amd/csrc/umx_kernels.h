// umx_kernels.h -- HBM-bound stages of the UMA-S engine: edge frames, the node-level kernels (norms,
// gates, grid transforms, readout), rotate-back + segmented reduction and force assembly.  (The
// neighbour graph, K1, is umx_graph.h; the edge links between the GEMMs are umx_edge.h.)
//
// Conventions: one 64-lane wave per edge or per node, 4 waves per 256-thread block; a lane owns 2
// (or 4) adjacent channels so every row access is a coalesced 512-B (1-KiB) segment; edges are
// sorted by target so reductions over incoming edges are deterministic segmented sums (no float
// atomics); contributions that flow to an edge's SOURCE node are collected through the reverse
// edge index rev[e] (the graph is symmetric).  Per-edge frame records are wave-uniform.
#pragma once
#include "umx_common.h"

namespace umx {

// K2 edge frames: R (R nhat = +y, minimal rotation, flipped branch for nhat_y < -0.9), D2, envelope.
// Carried in DOUBLE from the float32 unit vector and rounded to float32 once per entry (round 3): the frame formulas are full of
// constants that float32 cannot hold (sqrt 3, 2/3, 1/sqrt 3); a float32 evaluation puts the SAME relative error of a few 1e-8 on the
// same D2 entries of EVERY edge -- a systematic gain on the l = 2 message components, i.e. an energy error that grows with the number
// of atoms instead of averaging out.  0.3 kFLOP per edge, once per evaluation: free.
__global__ void k_edge_geom(const float* __restrict__ evec, long ne, float cutoff, float* __restrict__ frame) {
  const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= ne) return;
  const float4 v = *reinterpret_cast<const float4*>(evec + e * 4);
  const double sg = (v.y < -0.9f) ? -1.0 : 1.0;
  const double nx = v.x, ny = (double)v.y * sg, nz = (double)v.z * sg;
  const double k = 1.0 / (1.0 + ny);
  const double R[9] = {1.0 - k * nx * nx, -nx * sg, -k * nx * nz * sg,
                       nx,                ny * sg,  nz * sg,
                       -k * nx * nz,      -nz * sg, (1.0 - k * nz * nz) * sg};
  float* f = frame + e * FRAME;
#pragma unroll
  for (int i = 0; i < 9; ++i) f[i] = (float)R[i];
  // D2[a][b] = (2/3) <A_a, R A_b R^T>; columns c_k = R e_k
  const double c0[3] = {R[0], R[3], R[6]}, c1[3] = {R[1], R[4], R[7]}, c2[3] = {R[2], R[5], R[8]};
  const double s3 = 1.7320508075688772935, hs3 = 0.5 * s3;
#pragma unroll
  for (int b = 0; b < 5; ++b) {
    double M[3][3];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        double m;
        if (b == 0) m = hs3 * (c0[i] * c2[j] + c2[i] * c0[j]);
        else if (b == 1) m = hs3 * (c0[i] * c1[j] + c1[i] * c0[j]);
        else if (b == 2) m = -0.5 * c0[i] * c0[j] + c1[i] * c1[j] - 0.5 * c2[i] * c2[j];
        else if (b == 3) m = hs3 * (c1[i] * c2[j] + c2[i] * c1[j]);
        else m = hs3 * (c2[i] * c2[j] - c0[i] * c0[j]);
        M[i][j] = m;
      }
    const double t23 = 2.0 / 3.0;
    f[9 + 0 * 5 + b] = (float)(t23 * s3 * M[0][2]);
    f[9 + 1 * 5 + b] = (float)(t23 * s3 * M[0][1]);
    f[9 + 2 * 5 + b] = (float)(t23 * (-0.5 * M[0][0] + M[1][1] - 0.5 * M[2][2]));
    f[9 + 3 * 5 + b] = (float)(t23 * s3 * M[1][2]);
    f[9 + 4 * 5 + b] = (float)(t23 * hs3 * (M[2][2] - M[0][0]));
  }
  const double u = (double)v.w / (double)cutoff;
  double env = 0.0, denv = 0.0;
  if (u < 1.0) {
    const double u2 = u * u, u4 = u2 * u2, u5 = u4 * u;
    env = 1.0 + u5 * (-21.0 + u * (35.0 - 15.0 * u));
    denv = u4 * (-105.0 + u * (210.0 - 105.0 * u)) / (double)cutoff;
  }
  f[34] = (float)env;
  f[35] = (float)denv;
}

// ------------------------------------------------------------------------------------------------
// node-level kernels
// ------------------------------------------------------------------------------------------------
// sysemb is DOUBLE (round 3): the system embedding is added to every atom, here and in every layer's norm -- held in float32 its
// representation error (the same few 1e-8 for every atom) is a systematic energy error proportional to N; added in double and
// rounded once, what is left is the rounding of each atom's own sum.
// (The node init x0 = element embedding + system embedding has no kernel of its own: k_rotate_back_reduce<3> adds it as its base.)
// graph-parallel mode: x0 = node init + the all-reduced edge-degree aggregate, the l = 0 row in the SAME expression as the fused
// k_rotate_back_reduce<3> of the ordinary path (with all edges on one rank the two paths stay bitwise equal)
__global__ void k_node_init_add(const int* __restrict__ znode, int natoms, long nt, const float* __restrict__ emb,
                                const double* __restrict__ sysemb, const float* __restrict__ agg, float* __restrict__ x) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nt * ROW) return;
  const long node = i / ROW;
  const int r = (int)(i % ROW);
  x[i] = (r < C) ? (float)(((double)emb[znode[node % natoms] * C + r] + sysemb[r]) + (double)agg[i]) : agg[i];
}

// K6 RMS-norm-SH forward: wave per node, lane owns channels 2l, 2l+1
// Round 5: the whole row in DOUBLE (channel mean, sum of squares, 1/sqrt, scaling, affine), rounded once per output value.  The float32 form
// (compensated rstd, divisions instead of reciprocal constants -- rounds 3-4) still carried an energy error COHERENT over the atoms:
// tools/gpu_energy_cuts.py (linear response of the energy along cuts of the network) attributes +-1...3e-8 eV per atom to EACH norm, sign
// depending on the weight set -- for the seed-0 weights it happened to cancel the other terms, for seed 1 it was +2.1e-5 eV at 700 atoms in
// the final norm alone.  In double every norm's increment is +-3e-7 eV (noise).  Node-level work: no measurable cost.
__global__ __launch_bounds__(256) void k_norm_fwd(const float* __restrict__ x, const float* __restrict__ aw,
                                                  const float* __restrict__ ab, const double* __restrict__ sysemb,
                                                  float* __restrict__ y, long nt) {
  UMX_WAVE_ITEM(node, nt)
  const int c0 = lane * 2;
  float2 v[9];
#pragma unroll
  for (int r = 0; r < 9; ++r) v[r] = *reinterpret_cast<const float2*>(x + node * ROW + r * C + c0);
  // the whole row in double, rounded once per output value
  const double mean0 = wave_sum_d((double)v[0].x + (double)v[0].y) * (1.0 / C);
  double dx[9], dy[9];
#pragma unroll
  for (int r = 0; r < 9; ++r) { dx[r] = (double)v[r].x - (r == 0 ? mean0 : 0.0); dy[r] = (double)v[r].y - (r == 0 ? mean0 : 0.0); }
  double q0 = dx[0] * dx[0] + dy[0] * dy[0], q1 = 0.0, q2 = 0.0;
#pragma unroll
  for (int r = 1; r < 4; ++r) q1 += dx[r] * dx[r] + dy[r] * dy[r];
#pragma unroll
  for (int r = 4; r < 9; ++r) q2 += dx[r] * dx[r] + dy[r] * dy[r];
  const double qd = wave_sum_d(q0 / 3.0 + q1 / 9.0 + q2 / 15.0) * (1.0 / C);
  const double sd = 1.0 / sqrt(qd + (double)NORM_EPS);
#pragma unroll
  for (int r = 0; r < 9; ++r) {
    const int l = (r == 0) ? 0 : (r < 4 ? 1 : 2);
    const float2 w = *reinterpret_cast<const float2*>(aw + l * C + c0);
    double ox = dx[r] * sd * (double)w.x, oy = dy[r] * sd * (double)w.y;
    if (r == 0) {
      const float2 b = *reinterpret_cast<const float2*>(ab + c0);
      ox += (double)b.x + (sysemb ? sysemb[c0] : 0.0); oy += (double)b.y + (sysemb ? sysemb[c0 + 1] : 0.0);
    }
    *reinterpret_cast<float2*>(y + node * ROW + r * C + c0) = make_float2((float)ox, (float)oy);
  }
}

// backward: gx = gres + d(norm)/dx^T gy   (gres may be null)
__global__ __launch_bounds__(256) void k_norm_bwd(const float* __restrict__ gy, const float* __restrict__ x,
                                                  const float* __restrict__ aw, const float* __restrict__ gres,
                                                  float* __restrict__ gx, long nt) {
  UMX_WAVE_ITEM(node, nt)
  const int c0 = lane * 2;
  float2 v[9], g[9];
#pragma unroll
  for (int r = 0; r < 9; ++r) {
    v[r] = *reinterpret_cast<const float2*>(x + node * ROW + r * C + c0);
    g[r] = *reinterpret_cast<const float2*>(gy + node * ROW + r * C + c0);
  }
  const float mean0 = wave_sum(v[0].x + v[0].y) * (1.0f / C);
  v[0].x -= mean0; v[0].y -= mean0;
  float ql[3] = {0.f, 0.f, 0.f}, dot = 0.f;
#pragma unroll
  for (int r = 0; r < 9; ++r) {
    const int l = (r == 0) ? 0 : (r < 4 ? 1 : 2);
    const float2 w = *reinterpret_cast<const float2*>(aw + l * C + c0);
    g[r].x *= w.x; g[r].y *= w.y;
    ql[l] += v[r].x * v[r].x + v[r].y * v[r].y;
    dot += g[r].x * v[r].x + g[r].y * v[r].y;
  }
  float q = ql[0] / 3.0f + ql[1] / 9.0f + ql[2] / 15.0f;           // the forward's expression (k_norm_fwd)
  q = wave_sum(q) * (1.0f / C);
  dot = wave_sum(dot);
  const float s = rstd_eps(q, NORM_EPS).y;                 // (reverse pass: feeds forces only)
  const float k = s * s * s * dot * (1.0f / C);
  float2 o[9];
#pragma unroll
  for (int r = 0; r < 9; ++r) {
    const int l = (r == 0) ? 0 : (r < 4 ? 1 : 2);
    const float bal = (l == 0) ? (1.0f / 3.0f) : (l == 1 ? (1.0f / 9.0f) : (1.0f / 15.0f));
    o[r].x = g[r].x * s - k * bal * v[r].x;
    o[r].y = g[r].y * s - k * bal * v[r].y;
  }
  const float gm = wave_sum(o[0].x + o[0].y) * (1.0f / C);
  o[0].x -= gm; o[0].y -= gm;
#pragma unroll
  for (int r = 0; r < 9; ++r) {
    if (gres) {
      const float2 rr = *reinterpret_cast<const float2*>(gres + node * ROW + r * C + c0);
      o[r].x += rr.x; o[r].y += rr.y;
    }
    *reinterpret_cast<float2*>(gx + node * ROW + r * C + c0) = o[r];
  }
}

// K8, ff_type = grid (fairchem GridAtomwise [3P-UNVERIFIED]): the S2-grid projections of the atom-wise block.
// The (G, 9) matrices are DATA of the weight blob (so3_grid.to_grid_mat / from_grid_mat).  One wave per node, two channels per lane:
// every access is one contiguous 512-B row; the matrix entries are wave-uniform (scalar loads).
//   expand:   out[n, g, :] = sum_i M[g, i] x[n, i, :]      (to-grid forward with M = to_grid; reverse of from-grid with M = from_grid)
//   contract: out[n, i, :] = resid[n, i, :] + sum_g M[g, i] y[n, g, :]   (from-grid forward + residual; reverse of to-grid with M = to_grid),
//             G-term sums accumulated in double and rounded once (the same sum enters every atom's residual stream in every layer)
__global__ __launch_bounds__(256) void k_grid_expand(const float* __restrict__ x, const float* __restrict__ M, int G, float* __restrict__ out, long nt) {
  UMX_WAVE_ITEM(node, nt)
  const int c0 = lane * 2;
  float2 v[9];
#pragma unroll
  for (int r = 0; r < 9; ++r) v[r] = *reinterpret_cast<const float2*>(x + node * ROW + r * C + c0);
  float* op = out + node * (long)G * C + c0;
  for (int g = 0; g < G; ++g) {
    const float* m = M + g * 9;
    float ax = 0.f, ay = 0.f;
#pragma unroll
    for (int r = 0; r < 9; ++r) ax = fmaf(m[r], v[r].x, ax);
    asm volatile("" : "+v"(ax));          // keeps the backend from pairing the two chains into v_pk_fma_f32 (build.check_no_packed_fp32)
#pragma unroll
    for (int r = 0; r < 9; ++r) ay = fmaf(m[r], v[r].y, ay);
    *reinterpret_cast<float2*>(op + (long)g * C) = make_float2(ax, ay);
  }
}
__global__ __launch_bounds__(256) void k_grid_contract(const float* __restrict__ y, const float* __restrict__ M, int G, const float* __restrict__ resid,
                                                       float* __restrict__ out, long nt) {
  UMX_WAVE_ITEM(node, nt)
  const int c0 = lane * 2;
  double ax[9], ay[9];
#pragma unroll
  for (int r = 0; r < 9; ++r) { ax[r] = 0.0; ay[r] = 0.0; }
  const float* yp = y + node * (long)G * C + c0;
  for (int g = 0; g < G; ++g) {
    const float2 v = *reinterpret_cast<const float2*>(yp + (long)g * C);
    const float* m = M + g * 9;
#pragma unroll
    for (int r = 0; r < 9; ++r) { ax[r] = fma((double)m[r], (double)v.x, ax[r]); ay[r] = fma((double)m[r], (double)v.y, ay[r]); }
  }
#pragma unroll
  for (int r = 0; r < 9; ++r) {
    if (resid) { const float2 q = *reinterpret_cast<const float2*>(resid + node * ROW + r * C + c0); ax[r] += (double)q.x; ay[r] += (double)q.y; }
    *reinterpret_cast<float2*>(out + node * ROW + r * C + c0) = make_float2((float)ax[r], (float)ay[r]);
  }
}

// atom-wise gate (l-primary rows): row 0 SiLU, rows of degree l>0 * sigmoid(silu(gs_pre[l-1]))
__global__ void k_gate_node_fwd(const float* __restrict__ h, const float* __restrict__ gspre, float* __restrict__ hg, long nt) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nt * H) return;
  const long node = i / H;
  const int c = (int)(i % H);
  const float s1 = sigmoid_f(silu_f(gspre[node * 2 * H + c])), s2 = sigmoid_f(silu_f(gspre[node * 2 * H + H + c]));
  const float* hp = h + node * ROW + c;
  float* op = hg + node * ROW + c;
  op[0] = silu_f(hp[0]);
#pragma unroll
  for (int r = 1; r < 4; ++r) op[r * H] = hp[r * H] * s1;
#pragma unroll
  for (int r = 4; r < 9; ++r) op[r * H] = hp[r * H] * s2;
}

__global__ void k_gate_node_bwd(const float* __restrict__ ghg, const float* __restrict__ h, const float* __restrict__ gspre,
                                float* __restrict__ gh, float* __restrict__ ggspre, long nt) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nt * H) return;
  const long node = i / H;
  const int c = (int)(i % H);
  const float p1 = gspre[node * 2 * H + c], p2 = gspre[node * 2 * H + H + c];
  const float s1 = sigmoid_f(silu_f(p1)), s2 = sigmoid_f(silu_f(p2));
  const float* hp = h + node * ROW + c;
  const float* gp = ghg + node * ROW + c;
  float* op = gh + node * ROW + c;
  op[0] = gp[0] * silu_grad_f(hp[0]);
  float a1 = 0.f, a2 = 0.f;
#pragma unroll
  for (int r = 1; r < 4; ++r) { op[r * H] = gp[r * H] * s1; a1 += gp[r * H] * hp[r * H]; }
#pragma unroll
  for (int r = 4; r < 9; ++r) { op[r * H] = gp[r * H] * s2; a2 += gp[r * H] * hp[r * H]; }
  ggspre[node * 2 * H + c] = a1 * s1 * (1.0f - s1) * silu_grad_f(p1);
  ggspre[node * 2 * H + H + c] = a2 * s2 * (1.0f - s2) * silu_grad_f(p2);
}

// out = g .* silu'(pre)  (g may be a broadcast row vector when gstride == 0)
__global__ void k_silu_bwd(const float* __restrict__ g, long gstride, const float* __restrict__ pre, float* __restrict__ out,
                           long rows, int width) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= rows * width) return;
  const long r = i / width;
  const int c = (int)(i % width);
  out[i] = g[r * gstride + c] * silu_grad_f(pre[i]);
}

// K9 readout, stage 1: e_node[i] = silu(pre2_i) . w3 + b3   (one wave per node)
__global__ __launch_bounds__(256) void k_energy_node(const float* __restrict__ pre2, const float* __restrict__ w3,
                                                     const float* __restrict__ b3, float* __restrict__ e_node, long nt) {
  UMX_WAVE_ITEM(node, nt)
  const float2 w = *reinterpret_cast<const float2*>(w3 + lane * 2);
  const float2 v = *reinterpret_cast<const float2*>(pre2 + node * H + lane * 2);
  const double sx = (double)v.x / (1.0 + exp(-(double)v.x)), sy = (double)v.y / (1.0 + exp(-(double)v.y));
  const float en = (float)(wave_sum_d(sx * (double)w.x + sy * (double)w.y) + (double)b3[0]);
  if (lane == 0) e_node[node] = en;
}

// K9/K11 readout, stage 2: per image E = rmsd * sum_i e_node[i] + refsum, float64, fixed summation order (strided partial sums,
// then a tree over the 256 partials) so the result does not depend on scheduling
// flag: the engine's sticky range flag -- set when an image's energy is not finite (an activation beyond the fp16 operand range of the
// default precision mode, or a float32 overflow); read back by the host at the next synchronisation point (UMX_ERR_RANGE)
__global__ __launch_bounds__(256) void k_energy(const float* __restrict__ e_node, int natoms, double rmsd, double refsum,
                                                double* __restrict__ e_img, int* __restrict__ flag) {
  __shared__ double part[256];
  const int img = blockIdx.x, t = threadIdx.x;
  double acc = 0.0;
  for (int a = t; a < natoms; a += 256) acc += (double)e_node[(long)img * natoms + a];
  part[t] = acc;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (t < s) part[t] += part[t + s];
    __syncthreads();
  }
  if (t == 0) {
    const double e = part[0] * rmsd + refsum;
    e_img[img] = e;
    if (!isfinite(e)) atomicOr(flag, 1);
  }
}

// ------------------------------------------------------------------------------------------------
// edges -> nodes  (the edge links between the GEMMs are umx_edge.h)
// ------------------------------------------------------------------------------------------------
// K7b rotate back + segmented reduction over incoming edges: xout[n] = xin[n] + sum_e env_e W_e^T msg_e
// NROWS = 9 (SO(2) messages, ROW floats per edge) or 3 (edge-degree embedding, m=0 rows only, /5)
template <int NROWS>
__global__ __launch_bounds__(256) void k_rotate_back_reduce(const float* __restrict__ msg, const float* __restrict__ frame,
                                                            const int* __restrict__ row_ptr, const float* xin,
                                                            float* xout, long nt, float div,
                                                            const int* __restrict__ znode = nullptr, int natoms = 0,
                                                            const float* __restrict__ emb = nullptr, const double* __restrict__ sysemb = nullptr) {
  // emb != null (edge-degree embedding, K4 + K5 in one): the base of the l = 0 row is the node initialisation emb[Z] + sys_emb itself,
  // added in DOUBLE together with the aggregate and rounded once -- a float32 x0 row is the same for every atom of an element, and so
  // is its rounding error (round 3: no error may be shared by all atoms)
  UMX_WAVE_LOOP(node, nt) {
  const int c0 = lane * 2;
  double ax[9], ay[9];
#pragma unroll
  for (int r = 0; r < 9; ++r) { ax[r] = 0.f; ay[r] = 0.f; }
  const int e0 = row_ptr[node], e1 = row_ptr[node + 1];
  for (int e = e0; e < e1; ++e) {
    const float* f = frame + (long)e * FRAME;
    const float* m = msg + (long)e * (NROWS * C) + c0;
    float vx[9], vy[9];
#pragma unroll
    for (int r = 0; r < 9; ++r) {
      if (r < NROWS) { const float2 t = *reinterpret_cast<const float2*>(m + r * C); vx[r] = t.x; vy[r] = t.y; }
      else { vx[r] = 0.f; vy[r] = 0.f; }
    }
    // the rotated message of this edge in float32, scaled and ACCUMULATED over the incoming edges in double (round 5: a float32 running sum
    // over ~70 incoming edges is one more coherent 1e-8-level term per atom and layer; the kernel is HBM-bound, the double FMAs are free)
    float tx[9], ty[9];
#pragma unroll
    for (int r = 0; r < 9; ++r) { tx[r] = 0.f; ty[r] = 0.f; }
    const double scd = (double)f[34] / (double)div;
    rot_bwd_acc(f, vx, 1.0f, tx);
    rot_bwd_acc(f, vy, 1.0f, ty);
#pragma unroll
    for (int r = 0; r < 9; ++r) { ax[r] = fma(scd, (double)tx[r], ax[r]); ay[r] = fma(scd, (double)ty[r], ay[r]); }
  }
#pragma unroll
  for (int r = 0; r < 9; ++r) {
    if (emb && r == 0) {
      const float* er = emb + (long)znode[node % natoms] * C + c0;
      *reinterpret_cast<float2*>(xout + node * ROW + c0) = make_float2((float)(((double)er[0] + sysemb[c0]) + (double)ax[0]),
                                                                        (float)(((double)er[1] + sysemb[c0 + 1]) + (double)ay[0]));
      continue;
    }
    const float2 b = (xin && !emb) ? *reinterpret_cast<const float2*>(xin + node * ROW + r * C + c0) : make_float2(0.f, 0.f);   // null: the bare sum (graph-parallel partial)
    *reinterpret_cast<float2*>(xout + node * ROW + r * C + c0) = make_float2((float)((double)b.x + ax[r]), (float)((double)b.y + ay[r]));
  }
  }
}

// dst = a + b (a may alias dst); graph-parallel mode: residual + the all-reduced sum of the ranks' partial aggregates
__global__ void k_add_rows(float* dst, const float* a, const float* __restrict__ b, long n4) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n4) return;
  const float4 x = reinterpret_cast<const float4*>(a)[i], y = reinterpret_cast<const float4*>(b)[i];
  reinterpret_cast<float4*>(dst)[i] = make_float4(x.x + y.x, x.y + y.y, x.z + y.z, x.w + y.w);
}

// dE/dvec per edge from dE/dd and the torque (frame detached at the +y pole, as the reference does)
// dedd2: the radial-MLP part of dE/dd, accumulated apart (the fused radial tail kernels may run on the side stream, concurrently with
// edge kernels that add to dedd); the total is written back to dedd (debug capture)
__global__ void k_force_edge(float* __restrict__ dedd, const float* __restrict__ dedd2, const float* __restrict__ tau, const float* __restrict__ frame,
                             const float* __restrict__ evec, float* __restrict__ gvec, long ne) {
  const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= ne) return;
  const float4 v = *reinterpret_cast<const float4*>(evec + e * 4);
  const float* f = frame + e * FRAME;
  float lx = tau[e * 4 + 2], lz = -tau[e * 4 + 0];
  if (fabsf(v.y - 1.0f) <= 1e-8f + 1e-5f) { lx = 0.f; lz = 0.f; }
  const float inv = 1.0f / v.w, g = dedd[e] + dedd2[e];
  dedd[e] = g;
  // R^T (lx, 0, lz)
  const float tx = f[0] * lx + f[6] * lz, ty = f[1] * lx + f[7] * lz, tz = f[2] * lx + f[8] * lz;
  *reinterpret_cast<float4*>(gvec + e * 4) = make_float4(g * v.x + tx * inv, g * v.y + ty * inv, g * v.z + tz * inv, 0.f);
}

// F[n] = -dE/dpos[n] * rmsd,  dE/dpos[n] = sum_{e in out(n)} gvec[e] - sum_{e in in(n)} gvec[e]   (vec = pos[src] - pos[dst])
__global__ __launch_bounds__(256) void k_force_node(const float* __restrict__ gvec, const int* __restrict__ row_ptr,
                                                    const int* __restrict__ out_ptr, const int* __restrict__ out_edge, float rmsd,
                                                    float* __restrict__ forces, long nt) {
  UMX_WAVE_ITEM(node, nt)
  float fx = 0.f, fy = 0.f, fz = 0.f;
  for (int e = row_ptr[node] + lane; e < row_ptr[node + 1]; e += 64) {
    const float4 a = *reinterpret_cast<const float4*>(gvec + (long)e * 4);
    fx -= a.x; fy -= a.y; fz -= a.z;
  }
  for (int k = out_ptr[node] + lane; k < out_ptr[node + 1]; k += 64) {
    const float4 b = *reinterpret_cast<const float4*>(gvec + (long)out_edge[k] * 4);
    fx += b.x; fy += b.y; fz += b.z;
  }
  fx = wave_sum(fx); fy = wave_sum(fy); fz = wave_sum(fz);
  if (lane == 0) { forces[node * 3 + 0] = -rmsd * fx; forces[node * 3 + 1] = -rmsd * fy; forces[node * 3 + 2] = -rmsd * fz; }
}

// per-edge packed element indices for the first radial layer's lookup tables: z[src] | z[dst] << 16 (node ids are image-major)
__global__ void k_edge_z(const int* __restrict__ esrc, const int* __restrict__ edst, const int* __restrict__ znode, int natoms,
                         int* __restrict__ ez, long ne) {
  const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= ne) return;
  ez[e] = znode[esrc[e] % natoms] | (znode[edst[e] % natoms] << 16);
}

// ---- pairwise-distance bond-change classification (float64; reference bond_changes.py:142-187) ----------------------
// One thread per (i, j): D1, D2 in full and a code for i < j: 1 = bond formed, 2 = bond broken, 0 = neither.
// The arithmetic keeps the reference's operation order (no FMA contraction): T = bf (c_i + c_j); eps = mf T;
// bonded <=> D <= T - eps; considered only when |D2 - D1| >= df T.
__global__ __launch_bounds__(256) void k_bond_changes(const double* __restrict__ r1, const double* __restrict__ r2,
                                                      const double* __restrict__ cov, int n, double bf, double mf, double df,
                                                      double* __restrict__ d1, double* __restrict__ d2,
                                                      unsigned char* __restrict__ code) {
  const int j = blockIdx.x * 64 + (threadIdx.x & 63);
  const int i = blockIdx.y * 4 + (threadIdx.x >> 6);
  if (i >= n || j >= n) return;
  auto dist = [](const double* r, int a, int b) {
    const double dx = r[a * 3 + 0] - r[b * 3 + 0], dy = r[a * 3 + 1] - r[b * 3 + 1], dz = r[a * 3 + 2] - r[b * 3 + 2];
    return sqrt(__dadd_rn(__dadd_rn(__dmul_rn(dx, dx), __dmul_rn(dy, dy)), __dmul_rn(dz, dz)));
  };
  const double a = dist(r1, i, j), b = dist(r2, i, j);
  const long o = (long)i * n + j;
  if (d1) d1[o] = a;
  if (d2) d2[o] = b;
  unsigned char c = 0;
  if (i < j) {
    const double T = __dmul_rn(bf, __dadd_rn(cov[i], cov[j]));
    const double thr = __dsub_rn(T, __dmul_rn(mf, T));
    const bool A1 = a <= thr, A2 = b <= thr;
    const bool need = fabs(__dsub_rn(b, a)) >= __dmul_rn(df, T);
    c = need ? ((!A1 && A2) ? 1 : (A1 && !A2) ? 2 : 0) : 0;
  }
  code[o] = c;
}

// The same classification on MINIMUM-IMAGE distances in a periodic cell (umx_bond_changes_cell): same pair-per-thread shape, same
// explicit sums, the open kernel above left as it is.  BondCell: lattice vectors a (rows) and dual vectors b of the periodic
// sub-lattice as build_periodic forms them, both zero on an open axis -- so an open axis rounds to n = 0 by itself.
// For d = r_j - r_i: n_k = rint(d . b_k); d0 = d - sum_k n_k a_k; D = min over the candidate translations t of |d0 + t|.
// cand: [n_cand][4] float64 (tx, ty, tz, lb2), formed once on the host, read by every thread at the same index.  lb2 is a lower bound
// of |d0 + t|^2 that holds for every d0 with fractional coordinates in [-1/2, 1/2] (host: bond_cell_candidates), the entries ascend in
// it and the zero translation comes first with lb2 = 0: the search stops at the first entry whose bound exceeds the best so far.
// D_ij == D_ji bit for bit: negation is exact through every product, sum and rint, and the table holds -t bit for bit next to every t.
struct BondCell { double a[3][3], b[3][3]; };

__global__ __launch_bounds__(256) void k_bond_changes_cell(const double* __restrict__ r1, const double* __restrict__ r2,
                                                           const double* __restrict__ cov, int n, BondCell cell,
                                                           const double* __restrict__ cand, int n_cand, double bf, double mf, double df,
                                                           double* __restrict__ d1, double* __restrict__ d2,
                                                           unsigned char* __restrict__ code) {
  const int j = blockIdx.x * 64 + (threadIdx.x & 63);
  const int i = blockIdx.y * 4 + (threadIdx.x >> 6);
  if (i >= n || j >= n) return;
  auto sum3 = [](double x, double y, double z) { return __dadd_rn(__dadd_rn(x, y), z); };
  auto dist = [&](const double* r, int p, int q) {
    const double dx = r[q * 3 + 0] - r[p * 3 + 0], dy = r[q * 3 + 1] - r[p * 3 + 1], dz = r[q * 3 + 2] - r[p * 3 + 2];
    double m[3];
    for (int k = 0; k < 3; ++k) m[k] = rint(sum3(__dmul_rn(dx, cell.b[k][0]), __dmul_rn(dy, cell.b[k][1]), __dmul_rn(dz, cell.b[k][2])));
    const double x0 = __dsub_rn(dx, sum3(__dmul_rn(m[0], cell.a[0][0]), __dmul_rn(m[1], cell.a[1][0]), __dmul_rn(m[2], cell.a[2][0])));
    const double y0 = __dsub_rn(dy, sum3(__dmul_rn(m[0], cell.a[0][1]), __dmul_rn(m[1], cell.a[1][1]), __dmul_rn(m[2], cell.a[2][1])));
    const double z0 = __dsub_rn(dz, sum3(__dmul_rn(m[0], cell.a[0][2]), __dmul_rn(m[1], cell.a[1][2]), __dmul_rn(m[2], cell.a[2][2])));
    double best = sum3(__dmul_rn(x0, x0), __dmul_rn(y0, y0), __dmul_rn(z0, z0));      // cand[0]: the zero translation
    for (int t = 1; t < n_cand; ++t) {
      const double* c = cand + (size_t)t * 4;
      if (c[3] > best) break;
      const double x = __dadd_rn(x0, c[0]), y = __dadd_rn(y0, c[1]), z = __dadd_rn(z0, c[2]);
      best = fmin(best, sum3(__dmul_rn(x, x), __dmul_rn(y, y), __dmul_rn(z, z)));
    }
    return sqrt(best);
  };
  const double a = dist(r1, i, j), b = dist(r2, i, j);
  const long o = (long)i * n + j;
  if (d1) d1[o] = a;
  if (d2) d2[o] = b;
  unsigned char c = 0;
  if (i < j) {
    const double T = __dmul_rn(bf, __dadd_rn(cov[i], cov[j]));
    const double thr = __dsub_rn(T, __dmul_rn(mf, T));
    const bool A1 = a <= thr, A2 = b <= thr;
    const bool need = fabs(__dsub_rn(b, a)) >= __dmul_rn(df, T);
    c = need ? ((!A1 && A2) ? 1 : (A1 && !A2) ? 2 : 0) : 0;
  }
  code[o] = c;
}

}  // namespace umx
