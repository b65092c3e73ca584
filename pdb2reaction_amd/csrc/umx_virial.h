// umx_virial.h -- the strain derivative ("virial") of every image, W_ab = dE/d eps_ab = rmsd * sum_e vec_e,a * gvec_e,b over the directed
// edges of the image, with the graph held fixed (include/umx.h).  The model sees a geometry only through its edge vectors, a homogeneous
// strain multiplies every one of them by (1 + eps), and k_force_edge has just written gvec[e] = dE_model/dvec_e: what is left is one
// reduction over the edges, in float64 and without atomics.
//
// Two stages.  k_virial_slab: one workgroup per (image, slab of VIR_SLAB edges COUNTED FROM THE IMAGE'S FIRST EDGE); a lane adds the nine
// products of its edges (lo + lane, lo + lane + 256, ...), the wave sums through the butterfly, the four waves through LDS in wave order;
// one partial per (image, slab).  k_virial_image: one wave per image adds its partials in ascending slab order, times rmsd.  The edges a
// partial covers, and the order in which everything is added, depend on the image's own edge list only: the bits of W do not depend on
// which batch the image is in, on how the batch is chunked, or on the lanes.  The partials live outside the workspace arena
// (umx_engine::d_vir_part), indexed by the image's position in the CALL, so two chunks in flight never share a slot.
//
// Graph-parallel entry (umx_gp_begin_virial): every target node outside the rank's range has an empty CSR row, so "the image's edges" of
// the rank's plan are exactly the edges whose target it owns, and the same two launches give the rank's share of W.  The shares are
// disjoint and cover the image; adding them over the ranks, in rank order, is the caller's (include/umx.h).
#pragma once

namespace umx {

constexpr int VIR_SLAB = 4096;        // edges per partial: 16 per lane of a 256-lane workgroup

// grid (images of the chunk, slabs); image k's edges are row_ptr[k * natoms] ... row_ptr[(k + 1) * natoms]
__global__ __launch_bounds__(256) void k_virial_slab(const float* __restrict__ evec, const float* __restrict__ gvec, const int* __restrict__ row_ptr,
                                                     int natoms, int slabs_max, double* __restrict__ part) {
  __shared__ double sh[4][9];
  const long img = blockIdx.x;
  const int slab = blockIdx.y, t = threadIdx.x;
  const long e0 = row_ptr[img * natoms], e1 = row_ptr[(img + 1) * natoms];
  const long lo = e0 + (long)slab * VIR_SLAB;
  if (lo >= e1) return;                                       // (the whole workgroup: no barrier is left behind)
  const long hi = lo + VIR_SLAB < e1 ? lo + VIR_SLAB : e1;
  double a[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  for (long e = lo + t; e < hi; e += 256) {
    const float4 v = *reinterpret_cast<const float4*>(evec + e * 4);        // (unit vector, distance)
    const float4 g = *reinterpret_cast<const float4*>(gvec + e * 4);
    const double d = (double)v.w;
    const double vx = (double)v.x * d, vy = (double)v.y * d, vz = (double)v.z * d;   // exact: 24 x 24 bits
    const double gx = (double)g.x, gy = (double)g.y, gz = (double)g.z;
    a[0] += vx * gx; a[1] += vx * gy; a[2] += vx * gz;
    a[3] += vy * gx; a[4] += vy * gy; a[5] += vy * gz;
    a[6] += vz * gx; a[7] += vz * gy; a[8] += vz * gz;
  }
#pragma unroll
  for (int c = 0; c < 9; ++c) a[c] = wave_sum_d(a[c]);
  if ((t & 63) == 0) {
#pragma unroll
    for (int c = 0; c < 9; ++c) sh[t >> 6][c] = a[c];
  }
  __syncthreads();
  if (t < 9) part[(img * slabs_max + slab) * 9 + t] = ((sh[0][t] + sh[1][t]) + sh[2][t]) + sh[3][t];
}

// one wave per image: W[img][c] = rmsd * (partials of the image's slabs, ascending); an image without edges gives nine zeros
__global__ __launch_bounds__(64) void k_virial_image(const double* __restrict__ part, const int* __restrict__ row_ptr, int natoms, int slabs_max,
                                                     double rmsd, double* __restrict__ W) {
  const long img = blockIdx.x;
  const int c = threadIdx.x;
  if (c >= 9) return;
  const long n = (long)row_ptr[(img + 1) * natoms] - (long)row_ptr[img * natoms];
  const long ns = (n + VIR_SLAB - 1) / VIR_SLAB;
  // slabs_max comes from the largest image of the call (degree pass), so this never holds; if the two counts ever disagreed, edges would
  // be missing from the partials: the image's W is then NaN, not a sum over some of its edges (the host checks what it can, virial_launch)
  if (ns > slabs_max) { W[img * 9 + c] = __longlong_as_double(0x7ff8000000000000LL); return; }
  double s = 0.0;
  for (long k = 0; k < ns; ++k) s += part[(img * slabs_max + k) * 9 + c];
  W[img * 9 + c] = s * rmsd;
}

// partitioned evaluation: W = the partitions' W_p added in partition order
__global__ void k_virial_sum_parts(const double* __restrict__ wp, int n_parts, double* __restrict__ W) {
  const int c = threadIdx.x;
  if (c >= 9) return;
  double s = 0.0;
  for (int p = 0; p < n_parts; ++p) s += wp[p * 9 + c];
  W[c] = s;
}

}  // namespace umx

namespace {

// What plan_chunk needs to take the virial of its images: where W goes ([images of the chunk][9]), the chunk's first partial, and the
// slots per image.  out == nullptr: no virial was asked for, nothing is launched.
struct VirialOut { double* out = nullptr; double* part = nullptr; int slabs = 0; };

// slots per image for a call whose largest image has emax directed edges
inline int virial_slabs(long emax) { return (int)std::max(1L, (emax + VIR_SLAB - 1) / VIR_SLAB); }

// Make the partial buffer hold K images of `slabs` slots each; both streams are drained before the old buffer goes.  The partitioned
// evaluation's per-partition results W_p have a small buffer of their own (VIR_MAX_PARTS x 9, allocated once).
constexpr int VIR_MAX_PARTS = 16;
int virial_prepare(umx_engine* eng, hipStream_t s, long K, int slabs) {
  const long need = K * slabs * 9;
  if (eng->vir_cap < need) CHK(grow(eng, eng->vir_cap, need, {s, eng->stream2}, {DevBuf(eng->d_vir_part, (size_t)need)}));
  if (!eng->d_vir_wp) HIPCHK(eng, hipMalloc(&eng->d_vir_wp, (size_t)VIR_MAX_PARTS * 9 * sizeof(double)));
  return UMX_OK;
}

// the two launches, on the stream of the segment that has just run k_force_edge (ne == 0: it has not, and gvec is not read)
int virial_launch(umx_engine* eng, const WS& w, const VirialOut& v, long nimg, long ne) {
  hipStream_t s = eng->stream;
  // the slots were sized from the degree pass; the chunk's edge total is what this side knows of the same graph
  if (ne > nimg * (long)v.slabs * VIR_SLAB) return fail(eng, UMX_ERR_CAPACITY, "virial: a chunk has more edges than its partial slots cover (degree pass and plan disagree)");
  if (ne > 0) {
    const unsigned sl = std::min((unsigned)v.slabs, nblk(ne, VIR_SLAB));
    hipLaunchKernelGGL(k_virial_slab, dim3((unsigned)nimg, sl), dim3(256), 0, s, w.evec, w.gvec, w.row_ptr, eng->natoms, v.slabs, v.part);
  }
  hipLaunchKernelGGL(k_virial_image, dim3((unsigned)nimg), dim3(64), 0, s, v.part, w.row_ptr, eng->natoms, v.slabs, eng->rmsd, v.out);
  HIPCHK(eng, hipGetLastError());
  return UMX_OK;
}

}  // namespace
