// Per-(sample, class) segmentation statistics on gfx950: one streaming pass over the
// head's probabilities and the target that keeps the sample and class axes.
//
//   prob   fp32 [N][S][K]       (the head's sigmoid outputs, channels-last)
//   target TT   [N][S][K]       (TT: the build's 16-bit type, or float for the fp32 executor)
//   stats  fp32 [N][K][6] = {I = sum t p, St = sum t, Sp = sum p,
//                            TP = #(p >= thr, t >= 0.5), FP = #(p >= thr, t < 0.5),
//                            FN = #(p < thr, t >= 0.5)}          (TN = S - TP - FP - FN)
//
// A sample's flat [S K] run is contiguous and S % 8 == 0, so it is a whole number of
// 8-element vectors (16 bytes of a 16-bit target, two 16-byte loads of prob), every one
// 16-byte aligned.  A workgroup owns one (sample, chunk); per iteration each lane loads U
// vectors 256 vectors apart (a wave's load instruction covers 1 KiB / 2 KiB contiguously),
// all loads issued before the first use.  The class of element e of vector v is
// (8 v + e) % K: e % K for K = 1, 2, 4, and (2 v + e) % 3 for K = 3.  With U = 3 for K = 3 a
// lane's vector index advances by a multiple of 3 per iteration and chunks start at
// multiples of 3, so v = 256 u + tid (mod 3): the lane accumulates by r = (e + 2 u) % 3, a
// compile-time index, and rotates r -> class (r + 2 tid) % 3 once after the loop.  No row of
// 12 / 6 bytes is ever addressed on its own.
//
// Reduction: lanes -> wave by shuffles -> workgroup through LDS in wave order -> one row of
// 6 K floats per workgroup.  A sample that is one chunk writes its stats row directly;
// otherwise the rows go to `partial` [N][chunks][6 K] and seg_stats_finish_kernel sums a
// sample's chunks in a fixed order.  No atomics: two runs give the same bits.  The counts
// are kept as integers per lane and are below 2^24 per sample (S < 2^24), so their fp32
// sums are exact in any order.
#pragma once
#include "common.h"

namespace unet {
namespace {

constexpr int SEG_T = 256;          // lanes per workgroup
constexpr int SEG_FG = 8;           // chunk groups of the finish, summed in group order

template <int K>
struct SegU {
  static constexpr int value = K == 3 ? 3 : 4;     // vectors per lane and iteration
};

__device__ __forceinline__ void seg_load_t(const h16* t, size_t e0, float* f) {
  unpack8(*(const u32x4*)(t + e0), f);
}
__device__ __forceinline__ void seg_load_t(const float* t, size_t e0, float* f) {
  const f32x4 a = *(const f32x4*)(t + e0), b = *(const f32x4*)(t + e0 + 4);
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    f[i] = a[i];
    f[4 + i] = b[i];
  }
}

// vecs: 8-element vectors per sample (S K / 8); chunk_vecs: a multiple of SEG_T * U
template <int K, typename TT>
__global__ void __launch_bounds__(SEG_T) seg_stats_kernel(const float* __restrict__ prob, const TT* __restrict__ tgt,
                                                          int vecs, int chunk_vecs, int chunks, float thr,
                                                          float* __restrict__ out) {
  constexpr int U = SegU<K>::value;
  __shared__ float red[SEG_T / 64][6 * K];
  const int n = blockIdx.x / chunks, c = blockIdx.x - n * chunks;
  const int v0 = c * chunk_vecs;
  const int v1 = min(v0 + chunk_vecs, vecs);
  const size_t base = (size_t)n * vecs * 8;
  const float* pp = prob + base;
  const TT* tt = tgt + base;
  float aI[K], aT[K], aP[K];
  int nTP[K], nPos[K], nFg[K];        // FP = #pos - TP, FN = #fg - TP
#pragma unroll
  for (int r = 0; r < K; ++r) {
    aI[r] = aT[r] = aP[r] = 0.f;
    nTP[r] = nPos[r] = nFg[r] = 0;
  }
  for (int vb = v0 + (int)threadIdx.x; vb < v1; vb += SEG_T * U) {
    f32x4 p0[U], p1[U];
    float t[U][8];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      // (a vector past the chunk's end re-reads the chunk's last one and is not counted:
      // no branch around the loads, so all of them are in flight together)
      const size_t e0 = (size_t)min(vb + u * SEG_T, v1 - 1) * 8;
      p0[u] = *(const f32x4*)(pp + e0);
      p1[u] = *(const f32x4*)(pp + e0 + 4);
      seg_load_t(tt, e0, t[u]);
    }
    __builtin_amdgcn_sched_barrier(0);            // every load of the iteration issued before its first use
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const bool ok = vb + u * SEG_T < v1;        // (selects, not a branch: see the loads)
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const int r = K == 3 ? (e + 2 * u) % 3 : e % K;      // (compile-time after unrolling)
        const float praw = e < 4 ? p0[u][e & 3] : p1[u][e & 3];
        const float p = ok ? praw : 0.f, tv = ok ? t[u][e] : 0.f;
        const bool pos = ok && praw >= thr, fg = tv >= 0.5f;
        aI[r] += tv * p;
        aT[r] += tv;
        aP[r] += p;
        nTP[r] += (pos && fg) ? 1 : 0;
        nPos[r] += pos ? 1 : 0;
        nFg[r] += fg ? 1 : 0;
      }
    }
  }
  // this lane's row in class order: q = k * 6 + slot
  float row[6 * K];
#pragma unroll
  for (int k = 0; k < K; ++k) {
    float vI = aI[k], vT = aT[k], vP = aP[k];
    int cTP = nTP[k], cPos = nPos[k], cFg = nFg[k];
    if (K == 3) {
      // class k holds accumulator r with (r + 2 tid) % 3 == k
      const int ph = (2 * (int)threadIdx.x) % 3;
      const int ra = (k + 2) % 3, rb = (k + 1) % 3;         // r for ph == 1, ph == 2
      vI = ph == 0 ? aI[k] : (ph == 1 ? aI[ra] : aI[rb]);
      vT = ph == 0 ? aT[k] : (ph == 1 ? aT[ra] : aT[rb]);
      vP = ph == 0 ? aP[k] : (ph == 1 ? aP[ra] : aP[rb]);
      cTP = ph == 0 ? nTP[k] : (ph == 1 ? nTP[ra] : nTP[rb]);
      cPos = ph == 0 ? nPos[k] : (ph == 1 ? nPos[ra] : nPos[rb]);
      cFg = ph == 0 ? nFg[k] : (ph == 1 ? nFg[ra] : nFg[rb]);
    }
    row[k * 6 + 0] = vI;
    row[k * 6 + 1] = vT;
    row[k * 6 + 2] = vP;
    row[k * 6 + 3] = (float)cTP;       // (integers below 2^24: exact from here on)
    row[k * 6 + 4] = (float)(cPos - cTP);
    row[k * 6 + 5] = (float)(cFg - cTP);
  }
  const int wv = threadIdx.x >> 6;
#pragma unroll
  for (int q = 0; q < 6 * K; ++q) row[q] = wave_sum(row[q]);
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int q = 0; q < 6 * K; ++q) red[wv][q] = row[q];
  }
  __syncthreads();
  if (threadIdx.x < 6 * K) {
    float s = 0.f;
#pragma unroll
    for (int w = 0; w < SEG_T / 64; ++w) s += red[w][threadIdx.x];
    out[(size_t)blockIdx.x * (6 * K) + threadIdx.x] = s;
  }
}

// stats[n][q] = sum_c partial[n][c][q], q < W = 6 K <= 32: group g of SEG_FG sums chunks
// g, g + SEG_FG, ... in order, then the groups are added in group order
__global__ void __launch_bounds__(SEG_T) seg_stats_finish_kernel(const float* __restrict__ partial, int chunks, int W,
                                                                 float* __restrict__ stats) {
  __shared__ float red[SEG_FG][32];
  const int q = threadIdx.x & 31, g = threadIdx.x >> 5;
  const float* src = partial + (size_t)blockIdx.x * chunks * W;
  float s = 0.f;
  if (q < W)
    for (int c = g; c < chunks; c += SEG_FG) s += src[(size_t)c * W + q];
  red[g][q] = s;
  __syncthreads();
  if (threadIdx.x < W) {
    float r = 0.f;
#pragma unroll
    for (int k = 0; k < SEG_FG; ++k) r += red[k][threadIdx.x];
    stats[(size_t)blockIdx.x * W + threadIdx.x] = r;
  }
}

}  // namespace

const char* seg_stats_check(long long N, long long S, long long K);
int seg_stats_chunks(int N, int S, int K);

// partial: N * seg_stats_chunks(N, S, K) * 6 K floats (unused when a sample is one chunk)
template <typename TT>
hipError_t seg_stats_launch_t(const float* prob, const TT* t, int N, int S, int K, float thr, float* partial,
                              float* stats, hipStream_t s) {
  if (seg_stats_check(N, S, K) || !prob || !t || !stats) return hipErrorInvalidValue;
  const int chunks = seg_stats_chunks(N, S, K);
  if (chunks > 1 && !partial) return hipErrorInvalidValue;
  const int vecs = S / 8 * K;
  const int iter = SEG_T * (K == 3 ? 3 : 4);
  const int iters = (vecs + iter - 1) / iter;
  const int chunk_vecs = (iters + chunks - 1) / chunks * iter;
  float* out = chunks > 1 ? partial : stats;
#define SEG_STATS(KK) \
  UNET_LAUNCH((seg_stats_kernel<KK, TT>), dim3(N * chunks), dim3(SEG_T), 0, s, prob, t, vecs, chunk_vecs, chunks, thr, out)
  switch (K) {
    case 1: SEG_STATS(1); break;
    case 2: SEG_STATS(2); break;
    case 3: SEG_STATS(3); break;
    default: SEG_STATS(4);
  }
#undef SEG_STATS
  if (chunks > 1) UNET_LAUNCH(seg_stats_finish_kernel, dim3(N), dim3(SEG_T), 0, s, partial, chunks, 6 * K, stats);
  return launch_status();
}

}  // namespace unet
