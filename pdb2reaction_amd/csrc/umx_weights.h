// umx_weights.h -- host side, part 5 of 5: the weight loader (umx_load_weights): blob table, derived weights (transposes, the radial
// MLPs' per-element tables), the plane copies of the large weights in the precision mode's operand formats, the engine's weight views.
#pragma once

namespace {

std::vector<float> transpose(const float* src, int rows, int cols) {
  std::vector<float> t((size_t)rows * cols);
  for (int r = 0; r < rows; ++r)
    for (int c = 0; c < cols; ++c) t[(size_t)c * rows + r] = src[(size_t)r * cols + c];
  return t;
}

// ---- plane copies of the large weights ---------------------------------------------------------------
// IEEE binary16 <- binary32, round to nearest even, subnormals kept (what v_cvt_f16_f32 does for the activations)
unsigned short to_half(float f) {
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
}
float from_half(unsigned short h) {
  const uint32_t sign = (uint32_t)(h & 0x8000u) << 16, e = (h >> 10) & 0x1Fu, m = h & 0x3FFu;
  float v;
  if (e == 0) v = (float)m * (1.0f / 16777216.0f);
  else { const uint32_t u = ((e + 112u) << 23) | (m << 13); std::memcpy(&v, &u, 4); }     // (weights are finite: no inf/nan case)
  uint32_t u; std::memcpy(&u, &v, 4); u |= sign; std::memcpy(&v, &u, 4);
  return v;
}

// fp16 forward planes: the power of two that puts max|w| into [2^14, 2^15)
float f16_scale(float mx) {
  int ex = 0;
  if (mx > 0.f && std::isfinite(mx)) { std::frexp(mx, &ex); ex = std::max(-24, std::min(40, 15 - ex)); }   // mx = f * 2^ex', f in [0.5, 1)
  return std::ldexp(1.0f, ex);
}

// The host image of all plane copies (uploaded as d_bw) and where each weight's copy starts in it.  RNE split with exact residuals.
struct PlanePacker {
  struct Req { const float* dev; size_t off; bool quad; float scale; int rows, K, P; bool fwd, f16; };
  Precision pm; int align;
  std::vector<unsigned short> bw;
  std::vector<Req> req;
  size_t open(const float* dev, size_t count, bool quad, float scale, int rows, int K, int P, bool fwd, bool f16) {
    const size_t off = (bw.size() + 63) & ~size_t(63);
    bw.resize(off + count);
    req.push_back({dev, off, quad, scale, rows, K, P, fwd, f16});
    return off;
  }
  // fp16 quad-row copy of a forward weight: three half planes of s * w, s = the power of two that puts max|w| into [2^14, 2^15):
  // 33 significand bits -- exact for every weight above max|w| * 2^-16, an absolute 2^-39 max|w| below.
  void pack_f16(const float* host, const float* dev, int rows, int K) {
    const int PB = 3;
    float mx = 0.f;
    for (size_t i = 0; i < (size_t)rows * K; ++i) mx = std::max(mx, std::fabs(host[i]));
    const float sc = f16_scale(mx);
    const size_t off = open(dev, (size_t)rows * K * PB, true, sc, rows, K, PB, true, true);
    for (int rr = 0; rr < rows; ++rr)
      for (int k = 0; k < K; ++k) {
        float x = host[(size_t)rr * K + k] * sc;
        const size_t o = off + (((size_t)(rr / 4) * (K / 16) + k / 16) * (128 * PB) + (size_t)(rr % 4) * (32 * PB) + (size_t)(k % 16) * 2) / 2;
        for (int q = 0; q < PB; ++q) { const unsigned short hq = to_half(x); bw[o + 16 * q] = hq; x -= from_half(hq); }
      }
  }
  // FWD: a forward weight (quad-row layout; bf16 or fp16 planes as the mode says); REV: a transposed (reverse-pass) weight, with the
  // mode's reverse plane count -- in the PL layout, or (rev_quad, three planes) in the quad-row layout of its A operand
  void pack(const float* host, const float* dev, int rows, int K, Pass pass, bool rev_quad = false) {
    const bool fwdw = pass == FWD;
    const int P = fwdw ? 3 : pm.rev_planes;
    const bool quad = fwdw || (rev_quad && P == 3);
    if (fwdw && pm.fwd_fmt == 1) { pack_f16(host, dev, rows, K); return; }
    const size_t off = open(dev, (size_t)rows * K * P, quad, 0.f, rows, K, P, fwdw, false);
    // aligned planes (forward bf16 weights): the value that goes into plane q < 2 is first rounded to a multiple of 2^(e_max - 12), e_max =
    // exponent of the largest magnitude of what is left of the 8 weights the matrix core sees in one pass (k = 8 g ... 8 g + 7 of one row);
    // the exact remainder goes down the planes, so w0 + w1 + w2 is what it was (umx_gemm.h qf_align_magic does the same to A's leading plane)
    const bool alignw = fwdw && align != 0;
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
              bw[off + (((size_t)(rr / 4) * (K / 16) + k / 16) * 384 + (size_t)(rr % 4) * 96 + (size_t)q * 32 + (size_t)(k % 16) * 2) / 2] = hb;
            else
              bw[off + (size_t)rr * K * P + (size_t)(k / 32) * 32 * P + (size_t)q * 32 + (k % 32)] = hb;
            const uint32_t back = (uint32_t)hb << 16; float fb; std::memcpy(&fb, &back, 4);
            rem[j] -= fb;
          }
        }
      }
  }
};

// replace a device copy of a host array
template <class T> int upload(umx_engine* eng, T*& dst, const std::vector<T>& src) {
  if (dst) { HIPCHK(eng, hipFree(dst)); dst = nullptr; }
  HIPCHK(eng, hipMalloc(&dst, src.size() * sizeof(T)));
  HIPCHK(eng, hipMemcpy(dst, src.data(), src.size() * sizeof(T), hipMemcpyHostToDevice));
  return UMX_OK;
}

// ---- umx_load_weights ----------------------------------------------------------------------------------

// the 24 SO(2) weights a Mixture-of-Linear-Experts checkpoint stacks (umx_experts.h)
std::vector<std::string> expert_weight_names() {
  std::vector<std::string> v;
  for (int i = 0; i < NL; ++i)
    for (const char* c : {"1", "2"})
      for (const char* leaf : {".fc_m0.weight", ".so2_m_conv.0.fc.weight", ".so2_m_conv.1.fc.weight"})
        v.push_back("blocks." + std::to_string(i) + ".edge_wise.so2_conv_" + c + leaf);
  return v;
}

// drop what an earlier expert-form blob left on the device
int experts_release(umx_engine* eng) {
  HIPCHK(eng, hipStreamSynchronize(eng->stream));
  void** ptrs[] = {(void**)&eng->d_ex, (void**)&eng->d_mjobs, (void**)&eng->d_pjobs, (void**)&eng->d_mx};
  for (void** p : ptrs) if (*p) { HIPCHK(eng, hipFree(*p)); *p = nullptr; }
  eng->n_experts = 0; eng->experts_merged = false; eng->n_mjobs = eng->n_pjobs = eng->merge_blocks = eng->pack_blocks = 0;
  eng->f16_keys.clear();
  return UMX_OK;
}

int load_weights_impl(umx_engine* eng, const void* blob, size_t nbytes) {
  HIPCHK(eng, hipSetDevice(eng->dev));
  const char* b = static_cast<const char*>(blob);
  if (nbytes < 16 || std::memcmp(b, "UMXW0001", 8) != 0) return fail(eng, UMX_ERR_WEIGHTS, "weight blob: bad magic");
  uint32_t n;
  std::memcpy(&n, b + 8, 4);
  const size_t esz = 96 + 4 + 16 + 8 + 8;
  if (nbytes < 16 + (size_t)n * esz) return fail(eng, UMX_ERR_WEIGHTS, "weight blob: truncated table");
  size_t pos = 16;
  eng->wt.clear();
  std::vector<std::string> order;           // names in table order
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
    order.push_back(name);
    max_end = std::max(max_end, (size_t)(off + nb));
    pos += esz;
  }
  const size_t data0 = (pos + 63) & ~size_t(63);
  if (nbytes < data0 + max_end) return fail(eng, UMX_ERR_WEIGHTS, "weight blob: truncated data");
  const float* src = reinterpret_cast<const float*>(b + data0);
  for (const auto& kv : eng->wt)            // a non-finite parameter would only show up later as a non-finite energy
    for (size_t i = 0; i < kv.second.count; ++i)
      if (!std::isfinite(src[kv.second.off + i])) return fail(eng, UMX_ERR_WEIGHTS, "weight blob: non-finite value in " + kv.first);
  // ---- expert form?  The 24 SO(2) weights all stacked (n, out, in) with one n, or none of them
  int nex = 0;
  {
    int stacked = 0;
    for (const std::string& nm : expert_weight_names()) {
      auto it = eng->wt.find(nm);
      if (it == eng->wt.end() || it->second.shape.size() != 3) continue;
      if (stacked && it->second.shape[0] != nex) return fail(eng, UMX_ERR_WEIGHTS, "weight blob: expert stacks of different sizes (" + nm + ")");
      nex = it->second.shape[0];
      ++stacked;
    }
    if (stacked && stacked != N_EXPERT_W)
      return fail(eng, UMX_ERR_WEIGHTS, "weight blob: " + std::to_string(stacked) + " of the " + std::to_string(N_EXPERT_W) + " SO(2) weights are expert stacks: all of them or none");
    if (stacked && (nex < 1 || nex > MAX_EXPERTS)) return fail(eng, UMX_ERR_WEIGHTS, "weight blob: expert count outside [1, " + std::to_string(MAX_EXPERTS) + "]");
  }
  CHK(experts_release(eng));
  std::map<std::string, size_t> ex_off;      // expert form: where each stack starts in d_ex
  if (nex == 0) {
    eng->h_w.assign(src, src + (max_end + 3) / 4);
  } else {
    // the compact data section: the tensors in table order, 64-byte aligned, every stack in the room of ONE expert (what a host-merged blob
    // of the same tensors looks like); the stacks go straight from the blob to the device
    std::set<std::string> exn;
    for (const std::string& nm : expert_weight_names()) exn.insert(nm);
    size_t cur = 0, ex_total = 0;
    for (const std::string& nm : order) if (exn.count(nm)) ex_total += eng->wt[nm].count;
    HIPCHK(eng, hipMalloc(&eng->d_ex, ex_total * sizeof(float)));
    std::vector<std::pair<size_t, Tensor*>> moves;
    size_t exc = 0;
    for (const std::string& nm : order) {
      Tensor& t = eng->wt[nm];
      const size_t old = t.off;
      if (exn.count(nm)) {
        HIPCHK(eng, hipMemcpy(eng->d_ex + exc, src + old, t.count * sizeof(float), hipMemcpyHostToDevice));
        ex_off[nm] = exc; exc += t.count;
        t.count /= (size_t)nex; t.shape.erase(t.shape.begin());
        t.off = cur;
      } else {
        t.off = cur;
        moves.push_back({old, &t});
      }
      cur += (t.count + 15) & ~size_t(15);
    }
    eng->h_w.assign(cur, 0.f);
    for (const auto& mv : moves) std::copy(src + mv.first, src + mv.first + mv.second->count, eng->h_w.begin() + mv.second->off);
  }

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
  CHK(upload(eng, eng->d_w, eng->h_w)); CHK(upload(eng, eng->d_dw, dw)); CHK(upload(eng, eng->d_dtab, dtab));
  auto W = [&](const std::string& nm) -> const float* { return eng->d_w + eng->wt[nm].off; };
  auto D = [&](size_t o) -> const float* { return eng->d_dw + o; };
  // precision mode (read here: the weight planes below are packed in the forward operand format it selects)
  {
    const char* pv = std::getenv("UMX_PRECISION");
    const std::string mode = !eng->precision.empty() ? eng->precision : (pv && *pv ? pv : "auto");
    if (!resolve_precision(mode, &eng->prec))
      return fail(eng, UMX_ERR_ARG, "UMX_PRECISION must be auto, bf16x3 (= split-exact), split (= split-f16), split-bf16 or fp32");
    // a precision change alters the workspace carve-up: force a re-carve on the next call
    eng->cap_nodes = 0; eng->cap_edges = 0;
  }
  // ---- plane copies of the large weights (PlanePacker) ----
  PlanePacker pk{eng->prec, eng->align};
  const float* hd = dw.data();
  for (int i = 0; i < NL; ++i) {
    const std::string bpre = "blocks." + std::to_string(i);
    const std::string c1 = bpre + ".edge_wise.so2_conv_1", c2 = bpre + ".edge_wise.so2_conv_2";
    auto WH = [&](const std::string& nm, int rows, int K) { pk.pack(hw + eng->wt[nm].off, W(nm), rows, K, FWD); };
    WH(c1 + ".fc_m0.weight", 640, 768); WH(c1 + ".so2_m_conv.0.fc.weight", 512, 512); WH(c1 + ".so2_m_conv.1.fc.weight", 256, 256);
    WH(c2 + ".fc_m0.weight", 384, 384); WH(c2 + ".so2_m_conv.0.fc.weight", 512, 256); WH(c2 + ".so2_m_conv.1.fc.weight", 256, 128);
    WH(c1 + ".rad_func.fc3.weight", RAD, RH);
    // the conv^T weights follow their A operands (g_msg / g_hg): quad-row layout in the bf16x3 mode; fc3^T stays PL (g_rad comes from the
    // node-centric k_modrot_bwd_pl, whose rows are written edge by edge)
    pk.pack(hd + loff[i].c1m0T, D(loff[i].c1m0T), 768, 640, REV, true); pk.pack(hd + loff[i].c1m1T, D(loff[i].c1m1T), 2 * 512, 256, REV, true);
    pk.pack(hd + loff[i].c1m2T, D(loff[i].c1m2T), 2 * 256, 128, REV, true); pk.pack(hd + loff[i].c2m0T, D(loff[i].c2m0T), 384, 384, REV, true);
    pk.pack(hd + loff[i].c2m1T, D(loff[i].c2m1T), 2 * 256, 256, REV, true); pk.pack(hd + loff[i].c2m2T, D(loff[i].c2m2T), 2 * 128, 128, REV, true);
    pk.pack(hd + roff[c1 + ".rad_func"].w3T, D(roff[c1 + ".rad_func"].w3T), RH, RAD, REV);
  }
  {   // the edge-degree radial MLP's fc3 (128 -> 384) and its transpose run on the split path too
    const std::string nm = "edge_degree_embedding.rad_func.fc3.weight";
    pk.pack(hw + eng->wt[nm].off, W(nm), 3 * C, RH, FWD);
    const size_t t = roff["edge_degree_embedding.rad_func"].w3T;
    pk.pack(hd + t, D(t), RH, 3 * C, REV);
  }
  CHK(upload(eng, eng->d_bw, pk.bw));
  eng->planes.clear();
  for (const auto& r : pk.req) eng->planes[r.dev] = PlaneCopy{eng->d_bw + r.off, r.quad, r.scale};
  eng->n_w = eng->h_w.size(); eng->n_dw = dw.size(); eng->n_bw = pk.bw.size();
  if (nex) {
    // the 24 weights' slots in d_w, their reverse-pass copies in d_dw and the 48 plane copies in d_bw were built from zeros above: what
    // umx_set_expert_coefficients has to fill, as job records for its two kernels
    std::vector<MergeJob> mj;
    std::vector<PackJob> pj;
    std::set<const float*> slots;
    int mblk = 0, pblk = 0;
    for (int i = 0; i < NL; ++i) {
      const std::string bpre = "blocks." + std::to_string(i);
      const std::string c1 = bpre + ".edge_wise.so2_conv_1", c2 = bpre + ".edge_wise.so2_conv_2";
      auto job = [&](const std::string& nm, size_t toff, int rows, int cols, int half) {
        float* w = eng->d_w + eng->wt[nm].off;
        mj.push_back({eng->d_ex + ex_off[nm], w, eng->d_dw + toff, rows, cols, half, mblk});
        mblk += (rows / 32) * (cols / 128);
        slots.insert(w); slots.insert(eng->d_dw + toff);
      };
      job(c1 + ".fc_m0.weight", loff[i].c1m0T, 640, 768, 640); job(c1 + ".so2_m_conv.0.fc.weight", loff[i].c1m1T, 512, 512, 256);
      job(c1 + ".so2_m_conv.1.fc.weight", loff[i].c1m2T, 256, 256, 128); job(c2 + ".fc_m0.weight", loff[i].c2m0T, 384, 384, 384);
      job(c2 + ".so2_m_conv.0.fc.weight", loff[i].c2m1T, 512, 256, 256); job(c2 + ".so2_m_conv.1.fc.weight", loff[i].c2m2T, 256, 128, 128);
    }
    eng->f16_keys.clear();
    for (const auto& r : pk.req) {
      if (!slots.count(r.dev)) continue;
      int f16 = 0;
      if (r.f16) { eng->f16_keys.push_back(r.dev); f16 = (int)eng->f16_keys.size(); }
      pj.push_back({r.dev, eng->d_bw + r.off, r.rows, r.K, r.P, r.quad ? 1 : 0, (r.fwd && eng->align != 0) ? 1 : 0, f16, pblk});
      pblk += (int)(((size_t)r.rows * (r.K / 8) + 255) / 256);
    }
    if ((int)mj.size() != N_EXPERT_W || (int)pj.size() != 2 * N_EXPERT_W) return fail(eng, UMX_ERR_WEIGHTS, "weight blob: expert job table is incomplete");
    HIPCHK(eng, hipMalloc(&eng->d_mjobs, mj.size() * sizeof(MergeJob)));
    HIPCHK(eng, hipMalloc(&eng->d_pjobs, pj.size() * sizeof(PackJob)));
    HIPCHK(eng, hipMalloc(&eng->d_mx, N_EXPERT_W * sizeof(unsigned)));
    HIPCHK(eng, hipMemcpy(eng->d_mjobs, mj.data(), mj.size() * sizeof(MergeJob), hipMemcpyHostToDevice));
    HIPCHK(eng, hipMemcpy(eng->d_pjobs, pj.data(), pj.size() * sizeof(PackJob), hipMemcpyHostToDevice));
    eng->n_mjobs = (int)mj.size(); eng->n_pjobs = (int)pj.size(); eng->merge_blocks = mblk; eng->pack_blocks = pblk;
    if (!eng->ev_m0) { HIPCHK(eng, hipEventCreate(&eng->ev_m0)); HIPCHK(eng, hipEventCreate(&eng->ev_m1)); }
  }
  eng->n_experts = nex; eng->experts_merged = false;
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

}  // namespace
