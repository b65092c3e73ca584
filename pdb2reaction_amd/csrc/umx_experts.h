// umx_experts.h -- Mixture-of-Linear-Experts merge on the device: W = sum_k alpha_k W_k for the 24 SO(2)
// weights of an expert-form blob, their reverse-pass copies and their plane copies -- the device twins of the host loops of umx_weights.h
// (transpose, half_T, PlanePacker::pack / pack_f16), bit for bit.  Included by umx_api.hip after umx_weights.h.
//
// The merge is PINNED (checkpoint.merge_mole_ordered): s = 0.0; for k = 0 .. n-1: s = s + alpha[k] * (double)W_k, every product and every
// sum rounded to float64 (no fused multiply-add: contraction is off in these kernels), then ONE rounding to float32.
#pragma once

namespace umx {

// One workgroup = one 32 x 128 tile of one weight (MergeJob::blk0 says whose): every lane reads 4 x 16 bytes per expert (512-byte row
// segments: the stacks are n times the bytes of everything written), accumulates in float64 in expert order, writes the merged float32
// tile to d_w as it was read and, through LDS, transposed to d_dw (128-byte column segments).  mx (fp16 forward planes only): max |w| per
// weight as float bits, for the planes' power-of-two scale.
__global__ __launch_bounds__(256) void k_mole_merge(const MergeJob* __restrict__ jobs, int njobs, int n, ExpertAlpha al, unsigned* __restrict__ mx) {
#pragma clang fp contract(off)
  __shared__ float tile[32][129];
  int j = 0;
  while (j + 1 < njobs && (int)blockIdx.x >= jobs[j + 1].blk0) ++j;
  const MergeJob jb = jobs[j];
  const int t = (int)blockIdx.x - jb.blk0, tiles_c = jb.cols / 128;
  const int tr = t / tiles_c, tc = t % tiles_c;
  if (tr >= jb.rows / 32) return;
  const int c4 = threadIdx.x & 31, r0 = threadIdx.x >> 5;
  const size_t per = (size_t)jb.rows * jb.cols;
  const size_t base = (size_t)(tr * 32 + r0) * jb.cols + (size_t)tc * 128 + (size_t)c4 * 4;
  double acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int e = 0; e < 4; ++e) acc[i][e] = 0.0;
#pragma unroll 4
  for (int k = 0; k < n; ++k) {
    const double a = al.a[k];
    const float* p = jb.stack + (size_t)k * per + base;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const float4 v = *reinterpret_cast<const float4*>(p + (size_t)(8 * i) * jb.cols);
      acc[i][0] = acc[i][0] + a * (double)v.x;
      acc[i][1] = acc[i][1] + a * (double)v.y;
      acc[i][2] = acc[i][2] + a * (double)v.z;
      acc[i][3] = acc[i][3] + a * (double)v.w;
    }
  }
  unsigned m = 0;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const float4 w = make_float4((float)acc[i][0], (float)acc[i][1], (float)acc[i][2], (float)acc[i][3]);
    *reinterpret_cast<float4*>(jb.w + base + (size_t)(8 * i) * jb.cols) = w;
    tile[r0 + 8 * i][c4 * 4 + 0] = w.x; tile[r0 + 8 * i][c4 * 4 + 1] = w.y; tile[r0 + 8 * i][c4 * 4 + 2] = w.z; tile[r0 + 8 * i][c4 * 4 + 3] = w.w;
    m = max(max(m, __float_as_uint(w.x) & 0x7FFFFFFFu), max(__float_as_uint(w.y) & 0x7FFFFFFFu, max(__float_as_uint(w.z) & 0x7FFFFFFFu, __float_as_uint(w.w) & 0x7FFFFFFFu)));
  }
  if (mx) {                                   // |w| as bits orders like |w| (finite values)
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) m = max(m, (unsigned)__shfl_xor((int)m, s, 64));
    if ((threadIdx.x & 63) == 0) atomicMax(mx + j, m);
  }
  __syncthreads();
  // row R = ab * half + hh of the weight goes to wT[(ab * cols + c) * half + hh]; a 32-row tile lies within one ab (half is a multiple of 32)
  const int rr = threadIdx.x & 31, cc0 = threadIdx.x >> 5;
  const int R = tr * 32 + rr, ab = R / jb.half, hh = R % jb.half;
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const int cc = cc0 + 8 * i;
    jb.wT[((size_t)ab * jb.cols + (size_t)tc * 128 + cc) * jb.half + hh] = tile[rr][cc];
  }
}

// IEEE binary16 <- binary32 and back, as umx_weights.h to_half / from_half have them (round to nearest even, subnormals kept, >= 65520 -> inf)
__device__ inline unsigned short ex_to_half(float f) {
  unsigned x = __float_as_uint(f);
  const unsigned short sign = (unsigned short)((x >> 16) & 0x8000u);
  x &= 0x7FFFFFFFu;
  if (x > 0x7F800000u) return (unsigned short)(sign | 0x7E00u);
  if (x >= 0x477FF000u) return (unsigned short)(sign | 0x7C00u);
  if (x < 0x38800000u) return (unsigned short)(sign | (unsigned short)(int)rintf(__uint_as_float(x) * 16777216.0f));   // below 2^-14: a multiple of 2^-24
  unsigned h = (((x >> 23) - 112u) << 10) | ((x & 0x7FFFFFu) >> 13);
  const unsigned rem = x & 0x1FFFu;
  if (rem > 0x1000u || (rem == 0x1000u && (h & 1u))) ++h;
  return (unsigned short)(sign | h);
}
__device__ inline float ex_from_half(unsigned short h) {
  const unsigned sign = (unsigned)(h & 0x8000u) << 16, e = (h >> 10) & 0x1Fu, m = h & 0x3FFu;
  const float v = e == 0 ? (float)m * (1.0f / 16777216.0f) : __uint_as_float(((e + 112u) << 23) | (m << 13));
  return __uint_as_float(__float_as_uint(v) | sign);
}

// The device twin of PlanePacker::pack / pack_f16.  One lane owns one 8-k group of one row (k = 8 g ... 8 g + 7: what the matrix core sees
// in one pass), so the group maximum of the aligned planes needs no cross-lane traffic; one 16-byte store per plane.
__global__ __launch_bounds__(256) void k_pack_planes(const PackJob* __restrict__ jobs, int njobs, PackScales sc) {
#pragma clang fp contract(off)
  int j = 0;
  while (j + 1 < njobs && (int)blockIdx.x >= jobs[j + 1].blk0) ++j;
  const PackJob jb = jobs[j];
  const int G = jb.K / 8;
  const long idx = (long)((int)blockIdx.x - jb.blk0) * 256 + threadIdx.x;
  const int rr = (int)(idx / G), k0 = (int)(idx % G) * 8;
  if (rr >= jb.rows) return;
  const float4 lo = *reinterpret_cast<const float4*>(jb.src + (size_t)rr * jb.K + k0);
  const float4 hi = *reinterpret_cast<const float4*>(jb.src + (size_t)rr * jb.K + k0 + 4);
  float rem[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
  // first bf16 / fp16 element of plane 0 of this group; planes are `step` elements apart
  size_t o; int step;
  if (jb.quad) { o = ((size_t)(rr / 4) * (jb.K / 16) + k0 / 16) * (64 * jb.P) + (size_t)(rr % 4) * (16 * jb.P) + (k0 % 16); step = 16; }
  else { o = (size_t)rr * jb.K * jb.P + (size_t)(k0 / 32) * 32 * jb.P + (k0 % 32); step = 32; }
  unsigned short* dst = jb.dst + o;
  if (jb.f16) {
    const float s = sc.s[jb.f16 - 1];
#pragma unroll
    for (int e = 0; e < 8; ++e) rem[e] = rem[e] * s;
#pragma unroll
    for (int q = 0; q < 3; ++q) {
      unsigned short h[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) { h[e] = ex_to_half(rem[e]); rem[e] = rem[e] - ex_from_half(h[e]); }
      *reinterpret_cast<uint4*>(dst + (size_t)q * step) = make_uint4(h[0] | ((unsigned)h[1] << 16), h[2] | ((unsigned)h[3] << 16), h[4] | ((unsigned)h[5] << 16), h[6] | ((unsigned)h[7] << 16));
    }
    return;
  }
#pragma unroll
  for (int q = 0; q < 3; ++q) {
    if (q >= jb.P) break;
    // aligned planes: the value that goes into plane q < 2 is first rounded to a multiple of 2^(e_max - 12), e_max the exponent of the largest
    // magnitude left in the group; the exact remainder goes down the planes
    int eg = 0; bool al = false;
    if (jb.alignw && q < 2) {
      float gm = 0.f;
#pragma unroll
      for (int e = 0; e < 8; ++e) gm = fmaxf(gm, fabsf(rem[e]));
      if (gm > 0.f && gm < __uint_as_float(0x7F800000u)) { (void)frexpf(gm, &eg); al = ldexpf(1.0f, eg - 13) > 0.f; }
    }
    unsigned short h[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      // rem / quantum and its product with quantum are scalings by a power of two: ldexpf gives the host's quotient and product bit for bit
      const float lead = al ? ldexpf(rintf(ldexpf(rem[e], 13 - eg)), eg - 13) : rem[e];
      const unsigned u = __float_as_uint(lead);
      h[e] = (unsigned short)((u + 0x7FFFu + ((u >> 16) & 1u)) >> 16);
      rem[e] = rem[e] - __uint_as_float((unsigned)h[e] << 16);
    }
    *reinterpret_cast<uint4*>(dst + (size_t)q * step) = make_uint4(h[0] | ((unsigned)h[1] << 16), h[2] | ((unsigned)h[3] << 16), h[4] | ((unsigned)h[5] << 16), h[6] | ((unsigned)h[7] << 16));
  }
}

}  // namespace umx

namespace {

int set_expert_coefficients_impl(umx_engine* eng, int n, const double* alpha) {
  if (!eng->have_weights) return fail(eng, UMX_ERR_ARG, "umx_set_expert_coefficients: load weights first");
  if (eng->n_experts == 0) return fail(eng, UMX_ERR_ARG, "umx_set_expert_coefficients: the loaded blob is already merged (it holds no expert stacks)");
  if (n != eng->n_experts || !alpha)
    return fail(eng, UMX_ERR_ARG, "umx_set_expert_coefficients: " + std::to_string(n) + " coefficients for a blob of " + std::to_string(eng->n_experts) + " experts");
  ExpertAlpha al{};
  for (int k = 0; k < n; ++k) {
    if (!std::isfinite(alpha[k])) return fail(eng, UMX_ERR_ARG, "umx_set_expert_coefficients: coefficient " + std::to_string(k) + " is not finite");
    al.a[k] = alpha[k];
  }
  if (eng->gp_plan) return fail(eng, UMX_ERR_ARG, "umx_set_expert_coefficients: a graph-parallel evaluation is in progress (finish it with umx_gp_step)");
  HIPCHK(eng, hipSetDevice(eng->dev));
  HIPCHK(eng, hipStreamSynchronize(eng->stream));               // no evaluation may still be reading the weights
  if (eng->ran_on_caller) HIPCHK(eng, hipEventSynchronize(eng->ev_done));
  eng->experts_merged = false; eng->have_system = false;
  const bool f16 = !eng->f16_keys.empty();
  hipStream_t s = eng->stream;
  if (f16) HIPCHK(eng, hipMemsetAsync(eng->d_mx, 0, N_EXPERT_W * sizeof(unsigned), s));
  HIPCHK(eng, hipEventRecord(eng->ev_m0, s));
  umx::k_mole_merge<<<eng->merge_blocks, 256, 0, s>>>(eng->d_mjobs, eng->n_mjobs, n, al, f16 ? eng->d_mx : nullptr);
  HIPCHK(eng, hipGetLastError());
  PackScales sc{};
  if (f16) {
    // the planes' scale depends on the merged weight: one small read-back per merge; PlaneCopy::scale follows it.  Merge job i and
    // PackScales slot i are the same forward weight (both in the loader's layer order)
    unsigned mx[N_EXPERT_W];
    HIPCHK(eng, hipMemcpyAsync(mx, eng->d_mx, sizeof(mx), hipMemcpyDeviceToHost, s));
    HIPCHK(eng, hipStreamSynchronize(s));
    for (size_t i = 0; i < eng->f16_keys.size(); ++i) {
      float m; std::memcpy(&m, &mx[i], 4);
      sc.s[i] = f16_scale(m);
      eng->planes[eng->f16_keys[i]].scale = sc.s[i];
    }
  }
  umx::k_pack_planes<<<eng->pack_blocks, 256, 0, s>>>(eng->d_pjobs, eng->n_pjobs, sc);
  HIPCHK(eng, hipGetLastError());
  HIPCHK(eng, hipEventRecord(eng->ev_m1, s));
  HIPCHK(eng, hipStreamSynchronize(s));                        // evaluations may run on a caller's stream, which is not ordered after ours
  eng->experts_merged = true;
  return UMX_OK;
}

}  // namespace
