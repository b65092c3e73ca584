// umx_hvp.h -- Hessian-vector products by finite differences of the forces (umx_hvp / umx_hvp_dev, include/umx.h): the three small
// kernels around ONE batched evaluation of the displaced images, all of them float64, one thread per coordinate.
//
//   k_hvp_displace   x+- = base[base_of[m]] +- step * dir[m], product and sum rounded separately (no fused multiply-add): the bits are
//                    those of the NumPy expression base + step * dir (base - step * dir).  Central scheme: images 2m, 2m + 1; forward
//                    scheme: the R bases first, then base + step * dir[m].
//   k_hvp_combine    central: hv = -(double(F+) - double(F-)) / (2.0 * step) -- the operation order of hessian.fd_hessian, so that a unit
//                    direction gives that function's column bit for bit; forward: hv = -(double(F+) - double(F0)) / step.
//   k_hvp_curv       curv[m] = dir[m] . hv[m] / dir[m] . dir[m]: one workgroup per direction, lane t adds the coordinates t, t + 256, ...
//                    in ascending order, the 256 partials are added in a fixed LDS tree; no atomics.  The bits depend on dir[m] and hv[m]
//                    only -- not on the batch, the chunking or the lanes.  A zero direction gives 0, not 0 / 0.
//
// The displaced images live in an engine-owned float64 buffer and reach the graph kernels as double positions (k_graph_replay<double> on
// the pinned graphs, or the float64 build): nothing on this path is ever rounded to float32 before the edge vector is.
#pragma once

namespace umx {

// n3 = 3 * natoms; base_of == nullptr: every direction belongs to base 0; nb: the bases in front of the forward scheme's images (all of
// them, or none when the caller brought their forces)
__global__ __launch_bounds__(256) void k_hvp_displace(const double* __restrict__ base, const double* __restrict__ dir, const int* __restrict__ base_of,
                                                      double step, int forward, long nb, long M, long n3, double* __restrict__ x) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  const long K = forward ? nb + M : 2 * M;
  if (i >= K * n3) return;
  const long img = i / n3, c = i - img * n3;
  if (forward && img < nb) { x[i] = base[i]; return; }
  const long m = forward ? img - nb : img >> 1;
  const long b = base_of ? base_of[m] : 0;
  const double d = __dmul_rn(step, dir[m * n3 + c]);
  x[i] = (!forward && (img & 1)) ? __dsub_rn(base[b * n3 + c], d) : __dadd_rn(base[b * n3 + c], d);
}

// f: the float32 forces of the images in k_hvp_displace's order; f0: the bases' forces (forward scheme: f itself when the bases are among
// the images); den = 2.0 * step (central) or step (forward)
__global__ __launch_bounds__(256) void k_hvp_combine(const float* __restrict__ f, const float* __restrict__ f0, const int* __restrict__ base_of, double den,
                                                     int forward, long nb, long M, long n3, double* __restrict__ hv) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= M * n3) return;
  const long m = i / n3, c = i - m * n3;
  const long b = base_of ? base_of[m] : 0;
  const double fp = (double)f[(forward ? nb + m : 2 * m) * n3 + c];
  const double fm = forward ? (double)f0[b * n3 + c] : (double)f[(2 * m + 1) * n3 + c];
  hv[i] = __ddiv_rn(-__dsub_rn(fp, fm), den);
}

__global__ __launch_bounds__(256) void k_hvp_curv(const double* __restrict__ dir, const double* __restrict__ hv, long n3, double* __restrict__ curv) {
  __shared__ double sn[256], sd[256];
  const long m = blockIdx.x;
  const int t = threadIdx.x;
  const double* d = dir + m * n3;
  const double* h = hv + m * n3;
  double a = 0.0, b = 0.0;
  for (long c = t; c < n3; c += 256) {
    a = __dadd_rn(a, __dmul_rn(d[c], h[c]));
    b = __dadd_rn(b, __dmul_rn(d[c], d[c]));
  }
  sn[t] = a; sd[t] = b;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (t < s) { sn[t] = __dadd_rn(sn[t], sn[t + s]); sd[t] = __dadd_rn(sd[t], sd[t + s]); }
    __syncthreads();
  }
  if (t == 0) curv[m] = sd[0] > 0.0 ? __ddiv_rn(sn[0], sd[0]) : 0.0;
}

}  // namespace umx

namespace {

constexpr int HVP_FORWARD = 1, HVP_NO_PIN = 2, HVP_GIVEN_F0 = 4;     // umx_hvp's flags

// the bases among the images of a call, and the images
inline long hvp_bases(int R, int flags) { return (flags & HVP_FORWARD) && !(flags & HVP_GIVEN_F0) ? (long)R : 0L; }
inline long hvp_images(int R, int M, int flags) { return (flags & HVP_FORWARD) ? hvp_bases(R, flags) + M : 2L * M; }

// The engine-owned buffers of a call of K images and M directions, and base_of on the device (written only when it differs from what the
// device copy holds -- a Lanczos recursion asks for the same single direction of the same base every time, and then nothing is uploaded
// and nothing waited for).  *d_bof: nullptr when every direction belongs to base 0.
int hvp_prepare(umx_engine* eng, hipStream_t s, long K, int M, const int32_t* base_of, const int** d_bof) {
  const long nt = K * eng->natoms;
  if (eng->hvp_cap < nt || eng->hvp_img_cap < K) HIPCHK(eng, hipEventSynchronize(eng->ev_done));   // an earlier call on a caller's stream may still be using what is replaced
  if (eng->hvp_cap < nt) CHK(grow(eng, eng->hvp_cap, nt, {s, eng->stream, eng->stream2}, {DevBuf(eng->d_hvp_x, (size_t)nt * 3), DevBuf(eng->d_hvp_f, (size_t)nt * 3)}));
  if (eng->hvp_img_cap < K) CHK(grow(eng, eng->hvp_img_cap, K, {s, eng->stream, eng->stream2}, {DevBuf(eng->d_hvp_e, (size_t)K)}));
  *d_bof = nullptr;
  if (!base_of) return UMX_OK;
  bool same = (long)eng->hvp_bof_dev.size() >= M;
  for (int m = 0; m < M && same; ++m) same = eng->hvp_bof_dev[m] == base_of[m];
  if (!same) {
    eng->hvp_bof_dev.clear();
    for (hipStream_t q : {s, eng->stream, eng->stream2}) HIPCHK(eng, hipStreamSynchronize(q));      // an earlier call may still be reading the copy
    HIPCHK(eng, hipEventSynchronize(eng->ev_done));
    if (eng->hvp_bof_cap < M) CHK(grow(eng, eng->hvp_bof_cap, (long)M, {}, {DevBuf(eng->d_hvp_bof, (size_t)M)}));
    HIPCHK(eng, hipMemcpy(eng->d_hvp_bof, base_of, (size_t)M * sizeof(int), hipMemcpyHostToDevice));
    eng->hvp_bof_dev.assign(base_of, base_of + M);
  }
  *d_bof = eng->d_hvp_bof;
  return UMX_OK;
}

int hvp_displace(umx_engine* eng, hipStream_t s, int R, const double* d_base, int M, const double* d_dir, const int* d_bof, double step, int flags) {
  const long n3 = 3L * eng->natoms, K = hvp_images(R, M, flags);
  hipLaunchKernelGGL(k_hvp_displace, dim3(nblk(K * n3, 256)), dim3(256), 0, s, d_base, d_dir, d_bof, step, (flags & HVP_FORWARD) ? 1 : 0, hvp_bases(R, flags), (long)M, n3, eng->d_hvp_x);
  HIPCHK(eng, hipGetLastError());
  return UMX_OK;
}

// d_f0: the bases' forces the caller brought (HVP_GIVEN_F0), else nullptr
int hvp_combine(umx_engine* eng, hipStream_t s, int R, int M, const double* d_dir, const int* d_bof, double step, int flags, const float* d_f0, double* d_hv,
                double* d_curv) {
  const long n3 = 3L * eng->natoms;
  const bool fwd = (flags & HVP_FORWARD) != 0;
  hipLaunchKernelGGL(k_hvp_combine, dim3(nblk((long)M * n3, 256)), dim3(256), 0, s, eng->d_hvp_f, (flags & HVP_GIVEN_F0) ? d_f0 : eng->d_hvp_f,
                     d_bof, fwd ? step : 2.0 * step, fwd ? 1 : 0, hvp_bases(R, flags), (long)M, n3, d_hv);
  if (d_curv) hipLaunchKernelGGL(k_hvp_curv, dim3((unsigned)M), dim3(256), 0, s, d_dir, d_hv, n3, d_curv);
  HIPCHK(eng, hipGetLastError());
  return UMX_OK;
}

}  // namespace
