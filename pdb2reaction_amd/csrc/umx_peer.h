// umx_peer.h -- deterministic in-process sum of G float32 device buffers (umx_peer_sum, include/umx.h).
//
// The participants of a graph-parallel evaluation that live in ONE process (parallel.LocalEnginePool) can address each other's
// partial-sum buffers directly, so the sum at an exchange point needs no process group, no RCCL communicator and no host staging.
// The buffer is cut into G slices on 16-byte boundaries.  Participant r, on its own device and stream,
//   phase 1: reads slice r of all G buffers and adds them in LIST ORDER, ((b0 + b1) + b2) + ..., in float32 (plain v_add_f32: there is
//            no product to contract into an FMA, and __fadd_rn keeps it that way), and
//   phase 2: PUSHES the finished slice r into all G buffers (its own included).
// Pushing rather than pulling lets both phases share one pass of one kernel: the only thing a push overwrites in buffer q is slice r,
// which no other participant reads (q reads slice q of every buffer), so no barrier is needed between the phases -- a pull would need
// a third set of events (q may only overwrite its buffer after every peer has fetched slice q from it).  Remote writes are also posted
// where remote reads wait a round trip.  Neither has been MEASURED: no run on more than one physical device exists.
// Every buffer receives the very same float4, so all participants continue from identical bits.
#pragma once
#include <hip/hip_runtime.h>
#include <cstddef>

namespace umx {

constexpr int PEER_MAX = 16;            // participants of one umx_peer_sum (8 GPUs per node today)

struct PeerBufs { float* p[PEER_MAX]; };

// GT > 0: the number of participants at compile time (all loads of an element in flight before the first add); GT == 0: `n` at run time.
// [lo, hi) is this participant's slice: lo is a multiple of 4 floats, hi - lo is a multiple of 4 except in the last slice of a ragged count.
template <int GT>
__global__ void __launch_bounds__(256) k_peer_sum(PeerBufs b, int n, size_t lo, size_t hi) {
  const int g = GT ? GT : n;
  const size_t nq = (hi - lo) >> 2;
  const size_t tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  for (size_t q = tid; q < nq; q += stride) {
    const size_t i = lo + 4 * q;
    float4 v[GT ? GT : 1];
    float4 a;
    if (GT) {
#pragma unroll
      for (int j = 0; j < (GT ? GT : 1); ++j) v[j] = *reinterpret_cast<const float4*>(b.p[j] + i);
      a = v[0];
#pragma unroll
      for (int j = 1; j < (GT ? GT : 1); ++j) {
        a.x = __fadd_rn(a.x, v[j].x); a.y = __fadd_rn(a.y, v[j].y); a.z = __fadd_rn(a.z, v[j].z); a.w = __fadd_rn(a.w, v[j].w);
      }
    } else {
      a = *reinterpret_cast<const float4*>(b.p[0] + i);
      for (int j = 1; j < g; ++j) {
        const float4 w = *reinterpret_cast<const float4*>(b.p[j] + i);
        a.x = __fadd_rn(a.x, w.x); a.y = __fadd_rn(a.y, w.y); a.z = __fadd_rn(a.z, w.z); a.w = __fadd_rn(a.w, w.w);
      }
    }
    for (int j = 0; j < g; ++j) *reinterpret_cast<float4*>(b.p[j] + i) = a;
  }
  // ragged tail (count % 4 floats, last slice only)
  const size_t i = lo + 4 * nq + tid;
  if (i < hi) {
    float a = b.p[0][i];
    for (int j = 1; j < g; ++j) a = __fadd_rn(a, b.p[j][i]);
    for (int j = 0; j < g; ++j) b.p[j][i] = a;
  }
}

// Slice r of `count` floats over g participants: whole 16-byte quads dealt like parallel.shard_bounds (the first nq % g slices get one
// more), the ragged tail goes to the slice that holds the last quad.  Slices may be empty (count < 4 g).
inline void peer_slice(size_t count, int g, int r, size_t* lo, size_t* hi) {
  const size_t nq = (count + 3) / 4, base = nq / g, rem = nq % g;
  const size_t qlo = r * base + ((size_t)r < rem ? (size_t)r : rem), qhi = qlo + base + ((size_t)r < rem ? 1 : 0);
  *lo = 4 * qlo < count ? 4 * qlo : count;
  *hi = 4 * qhi < count ? 4 * qhi : count;
}

inline hipError_t launch_peer_sum(const PeerBufs& b, int g, size_t lo, size_t hi, hipStream_t s) {
  if (hi <= lo) return hipSuccess;
  const size_t nq = (hi - lo) >> 2;
  size_t blocks = (nq + 255) / 256;
  if (blocks < 1) blocks = 1;                       // (a slice that is only a ragged tail)
  if (blocks > 1024) blocks = 1024;                 // grid-stride beyond four workgroups per CU
  const dim3 grid((unsigned)blocks), block(256);
  switch (g) {
    case 2: hipLaunchKernelGGL(k_peer_sum<2>, grid, block, 0, s, b, g, lo, hi); break;
    case 3: hipLaunchKernelGGL(k_peer_sum<3>, grid, block, 0, s, b, g, lo, hi); break;
    case 4: hipLaunchKernelGGL(k_peer_sum<4>, grid, block, 0, s, b, g, lo, hi); break;
    case 8: hipLaunchKernelGGL(k_peer_sum<8>, grid, block, 0, s, b, g, lo, hi); break;
    default: hipLaunchKernelGGL(k_peer_sum<0>, grid, block, 0, s, b, g, lo, hi); break;
  }
  return hipGetLastError();
}

}  // namespace umx
