// Connected-component filtering of thresholded probability maps on gfx950: the step between
// the probabilities and the per-case scores ("keep the largest component", "drop components
// below V voxels").  All integer arithmetic from the threshold on; floats are copied or 0.0.
//
//   prob  fp32 [N][S][K]        (channels-last), S = D H W, D = 1 in 2D
//   out   fp32 [N][S][K]        out = prob outside F and on kept components, 0.0 on removed ones
//   info  int32 [N][K][4] = {components, kept components, size of the largest (0: none), kept voxels}
//   scratch int32: label [N][K][S], size [N][K][S], sel [N][K], part [N][K][P][5] with
//                  P = ceil(S / CC_CHUNK); every element is written (cc_init, cc_select_part,
//                  cc_select) before it is read
//
// F = {p >= thr} per (n, k); two voxels of F are connected when they share a face (4 / 6
// neighbours, as the surface of surf_dist.h); nothing wraps and samples and classes never
// connect.  A component's label is its smallest linear index (z H + y) W + x, its size its
// voxel count; the largest component is the one of maximal size, the smallest label among
// equals.  A component is kept when size >= min_size and, with keep_largest, it is the largest.
//
// Algorithm: label equivalence by union-find on the label plane itself (label[i] is i's
// parent, -1 outside F), with a fixed sequence of six launches and nothing read back:
//
//   1 cc_init      label[i] = first voxel of i's run of F inside its wave's 64-voxel segment of
//                  the row (two ballots and a count of leading zeros), size[i] = 0
//   2 cc_merge     union(i, i - 1) where a run continues across a segment boundary, and
//                  union(i, i - W) / union(i, i - H W) at the first column of every overlap of
//                  a run with the run above / behind it (where the left neighbours of both
//                  are in F as well, their union already implies this one)
//   3 cc_flatten   label[i] = root(i); size[root] += 1, one atomicAdd per distinct root per wave
//   4 cc_select_part  one workgroup per chunk of CC_CHUNK voxels of a plane: counts the roots,
//                  finds the largest, sums what passes min_size -> part (one workgroup per
//                  plane took 0.65 of the 0.80 ms of the op at b8 128^3, 8 workgroups in all)
//   5 cc_select    one wave per (n, k): combines the P parts, applies the policy -> info, and
//                  sel = the label keep_largest keeps (-1: none)
//   6 cc_write     out from prob, label, size[label] and sel
//
// Tile: there is none.  Runs are seeded in registers over the 64 lanes of a wave (the only
// "tile": 64 consecutive voxels of the linear index, cut at row starts) and everything else
// is unions on the global label plane.  An LDS-resident tile would have to be about 128 x 128
// int32 = 64 KiB to hold the model's slice, two workgroups per CU at most out of 160 KiB, and
// would still need this global merge at its seams; after run seeding only the run boundaries
// issue unions at all, so the plane is read about once per launch and the op is a handful of
// streaming passes.  The seam a test has to cross is therefore the 64-voxel segment (CC_SEG).
//
// Order independence.  The only concurrent writes are atomicMin on label[] (cc_merge),
// atomicAdd on size[] (cc_flatten) and, in cc_flatten, a thread's plain store of its own
// root to its own label.  Invariant: label[i] <= i for i in F at all times (cc_init sets a
// value <= i; atomicMin only lowers it; a root is <= every voxel on the path to it), and
// label[i] always names a voxel connected to i.  After cc_merge every pair of adjacent voxels
// is in one tree, a tree is one component, and its root, the only voxel with label[i] == i,
// is the smallest index of the tree because every path descends.  Labels are thus canonical
// and the counts exact whatever the order of the atomics.  Loads that race with atomics are
// relaxed agent-scope loads; a stale value is an earlier parent, still an ancestor-or-equal
// candidate that is connected and <= i, so it costs steps, never the result.
//
// Termination.  cc_find: a parent is < its index unless it is the root, so the walk
// descends strictly and ends after at most i steps.  cc_union: each round finds two roots
// a > b and tries atomicMin(label[a], b).  It ends when the value replaced was a itself (a was
// still a root: it now hangs below b).  Otherwise another thread had lowered label[a] to
// old < a; the link a -> old is kept or replaced by a -> b, and the round is repeated with
// (old, b), which unites what either link promised: a + b decreased strictly, and both are
// >= 0.  A retry thus happens only after a root decreased.  cc_flatten's aggregation loop
// retires at least the leading lane per round: at most 64 rounds.  No workgroup waits for
// another: ordering between workgroups is the kernel boundaries only.
#pragma once
#include "common.h"

namespace unet {
namespace {

constexpr int CC_SEG = 64;            // voxels of a row a wave seeds as runs (the wavefront)
constexpr int CC_BT = 256;            // lanes per workgroup of the per-voxel kernels
constexpr int CC_ST = 1024;           // lanes per workgroup of the selection's first stage
constexpr int CC_CHUNK = 16384;       // voxels of a plane per workgroup of that stage (16 per lane)
constexpr int CC_FT = 64;             // lanes per workgroup of its second stage (one wave)

__host__ __device__ inline long long cc_chunks(long long S) { return (S + CC_CHUNK - 1) / CC_CHUNK; }

__device__ __forceinline__ int cc_ld(const int* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// root of i's tree in the plane L (i in F)
__device__ __forceinline__ int cc_find(const int* L, int i) {
  int p;
  while ((p = cc_ld(L + i)) != i) i = p;
  return i;
}

__device__ __forceinline__ void cc_union(int* L, int a, int b) {
  for (;;) {
    a = cc_find(L, a);
    b = cc_find(L, b);
    if (a == b) return;
    if (a < b) {
      const int t = a;
      a = b;
      b = t;
    }
    const int old = atomicMin(L + a, b);
    if (old == a) return;
    a = old;
  }
}

// g: element of the label planes [planes][S]; prob element of (plane, s): ((n S) + s) K + k
__global__ void __launch_bounds__(CC_BT) cc_init_kernel(const float* __restrict__ prob, int* __restrict__ label,
                                                        int* __restrict__ size, long long total, int S, int W, int K,
                                                        float thr) {
  const long long g = (long long)blockIdx.x * CC_BT + threadIdx.x;
  const int lane = threadIdx.x & (CC_SEG - 1);
  bool fg = false;
  int s = 0, x = 0;
  if (g < total) {
    const long long plane = g / S;
    s = (int)(g - plane * S);
    x = s % W;
    const long long n = plane / K;
    const int k = (int)(plane - n * K);
    fg = prob[(n * S + s) * K + k] >= thr;
  }
  // bit j of conn: lane j continues the run of lane j - 1 (same row: x != 0; a plane starts at x = 0)
  const unsigned long long in = __ballot(fg);
  const unsigned long long conn = __ballot(fg && x != 0) & (in << 1);
  if (g < total) {
    int l = -1;
    if (fg) {
      const unsigned long long upto = lane == 63 ? ~0ull : ((2ull << lane) - 1);
      const int start = 63 - __clzll((long long)(~conn & upto));       // (bit 0 of ~conn is always set)
      l = s - (lane - start);
    }
    label[g] = l;
    size[g] = 0;
  }
}

__global__ void __launch_bounds__(CC_BT) cc_merge_kernel(int* __restrict__ label, long long total, int S, int H, int W) {
  const long long g = (long long)blockIdx.x * CC_BT + threadIdx.x;
  if (g >= total) return;
  const long long plane = g / S;
  const int s = (int)(g - plane * S);
  int* L = label + plane * S;
  if (cc_ld(L + s) < 0) return;
  const int x = s % W, r = s / W, y = r % H, z = r / H;
  const bool left = x > 0 && cc_ld(L + s - 1) >= 0;
  if (left && (threadIdx.x & (CC_SEG - 1)) == 0) cc_union(L, s, s - 1);
  if (y > 0 && cc_ld(L + s - W) >= 0 && !(left && cc_ld(L + s - W - 1) >= 0)) cc_union(L, s, s - W);
  const int HW = H * W;
  if (z > 0 && cc_ld(L + s - HW) >= 0 && !(left && cc_ld(L + s - HW - 1) >= 0)) cc_union(L, s, s - HW);
}

__global__ void __launch_bounds__(CC_BT) cc_flatten_kernel(int* __restrict__ label, int* __restrict__ size,
                                                           long long total, int S) {
  const long long g = (long long)blockIdx.x * CC_BT + threadIdx.x;
  const int lane = threadIdx.x & (CC_SEG - 1);
  long long root = -1;                  // element of the root in the planes
  if (g < total) {
    const long long plane = g / S;
    const int s = (int)(g - plane * S);
    int* L = label + plane * S;
    if (cc_ld(L + s) >= 0) {
      const int r = cc_find(L, s);
      // (other lanes may walk through s meanwhile: they see the old parent or the root, both on s's path)
      __hip_atomic_store(L + s, r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      root = plane * S + r;
    }
  }
  unsigned long long todo = __ballot(root >= 0);
  while (todo) {                        // (uniform over the wave)
    const int lead = __ffsll((long long)todo) - 1;
    const long long r = __shfl(root, lead);
    const unsigned long long same = __ballot(root == r);
    if (lane == lead) atomicAdd(size + r, __popcll(same));
    todo &= ~same;
  }
}

// (a, la) = the better of (a, la) and (b, lb): the larger size, the smaller label among equals
__device__ __forceinline__ void cc_better(int& a, int& la, int b, int lb) {
  if (b > a || (b == a && lb < la)) {
    a = b;
    la = lb;
  }
}

// workgroup = plane * P + chunk; part[workgroup] = {roots, largest size, its label, roots of
// size >= min_size, their voxels} of the chunk's roots
__global__ void __launch_bounds__(CC_ST) cc_select_part_kernel(const int* __restrict__ label,
                                                               const int* __restrict__ size, int S, int P,
                                                               int min_size, int* __restrict__ part) {
  __shared__ int red[5][CC_ST];
  const int tid = threadIdx.x;
  const int plane = blockIdx.x / P, chunk = blockIdx.x - plane * P;
  const int* L = label + (size_t)plane * S;
  const int* Z = size + (size_t)plane * S;
  const int s0 = chunk * CC_CHUNK, s1 = min(S - s0, CC_CHUNK) + s0;
  int comps = 0, big = 0, bigl = 0x7fffffff, nge = 0, vge = 0;
  for (int s = s0 + tid; s < s1; s += CC_ST) {
    if (L[s] != s) continue;
    const int z = Z[s];
    ++comps;
    cc_better(big, bigl, z, s);
    if (z >= min_size) {
      ++nge;
      vge += z;
    }
  }
  red[0][tid] = comps, red[1][tid] = big, red[2][tid] = bigl, red[3][tid] = nge, red[4][tid] = vge;
  __syncthreads();
  for (int h = CC_ST / 2; h > 0; h >>= 1) {
    if (tid < h) {
      red[0][tid] += red[0][tid + h];
      cc_better(red[1][tid], red[2][tid], red[1][tid + h], red[2][tid + h]);
      red[3][tid] += red[3][tid + h];
      red[4][tid] += red[4][tid + h];
    }
    __syncthreads();
  }
  if (tid < 5) part[(size_t)blockIdx.x * 5 + tid] = red[tid][0];
}

// workgroup = plane: the P parts of the plane -> info and sel
__global__ void __launch_bounds__(CC_FT) cc_select_kernel(const int* __restrict__ part, int P, int keep_largest,
                                                          int min_size, int* __restrict__ sel,
                                                          int* __restrict__ info) {
  __shared__ int red[5][CC_FT];
  const int tid = threadIdx.x;
  const int* Q = part + (size_t)blockIdx.x * P * 5;
  int comps = 0, big = 0, bigl = 0x7fffffff, nge = 0, vge = 0;
  for (int c = tid; c < P; c += CC_FT) {
    comps += Q[c * 5];
    cc_better(big, bigl, Q[c * 5 + 1], Q[c * 5 + 2]);
    nge += Q[c * 5 + 3];
    vge += Q[c * 5 + 4];
  }
  red[0][tid] = comps, red[1][tid] = big, red[2][tid] = bigl, red[3][tid] = nge, red[4][tid] = vge;
  __syncthreads();
  for (int h = CC_FT / 2; h > 0; h >>= 1) {
    if (tid < h) {
      red[0][tid] += red[0][tid + h];
      cc_better(red[1][tid], red[2][tid], red[1][tid + h], red[2][tid + h]);
      red[3][tid] += red[3][tid + h];
      red[4][tid] += red[4][tid + h];
    }
    __syncthreads();
  }
  if (tid == 0) {
    comps = red[0][0], big = red[1][0], bigl = red[2][0], nge = red[3][0], vge = red[4][0];
    const bool keep = comps > 0 && big >= min_size;       // the largest component passes min_size
    int* o = info + (size_t)blockIdx.x * 4;
    o[0] = comps;
    o[1] = keep_largest ? (keep ? 1 : 0) : nge;
    o[2] = big;
    o[3] = keep_largest ? (keep ? big : 0) : vge;
    sel[blockIdx.x] = keep ? bigl : -1;
  }
}

__global__ void __launch_bounds__(CC_BT) cc_write_kernel(const float* __restrict__ prob, const int* __restrict__ label,
                                                         const int* __restrict__ size, const int* __restrict__ sel,
                                                         long long total, int S, int K, int keep_largest,
                                                         int min_size, float* __restrict__ out) {
  const long long g = (long long)blockIdx.x * CC_BT + threadIdx.x;
  if (g >= total) return;
  const long long plane = g / S;
  const int s = (int)(g - plane * S);
  const long long n = plane / K;
  const int k = (int)(plane - n * K);
  const long long e = (n * S + s) * K + k;
  const float p = prob[e];
  const int l = label[g];
  bool keep = true;
  if (l >= 0) keep = keep_largest ? l == sel[plane] : size[plane * S + l] >= min_size;
  out[e] = keep ? p : 0.0f;
}

}  // namespace

const char* components_check(long long N, long long D, long long H, long long W, long long K, long long min_size);
long long components_scratch(long long N, long long D, long long H, long long W, long long K);

}  // namespace unet
