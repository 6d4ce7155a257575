// Test-time augmentation on gfx950: the device-side inverse transform and mean of the
// head's probability maps (data/augment.py tta_codes / tta_mean_torch is the oracle).
//
//   prob   fp32 [N][D][H][W][K]   (the head's sigmoid outputs, channels-last, K = 1..4; H == W)
//   acc    fp32 [N][D][H][W][K]
//   target TT   [N][D][H][W][K]   (TT: the build's 16-bit type, or float for the fp32 executor)
//
// tta_acc: acc[n][o][k] (=|+=) prob[n][f_code(o)][k] for ONE code, uniform over the launch,
// with f the source map of gather.h: output pixel (d, h, w) reads source pixel
//   d' = FD ? D-1-d : d;   (a, b) = T ? (w, h) : (h, w);   h' = FH ? H-1-a : a;   w' = FW ? W-1-b : b
// (bits: 0 FW, 1 FH, 2 T, 3 FD).  The caller passes the inverse of the code its gather used.
// In write mode no element of acc is read.
//
// Geometry (gather.h's): a workgroup of 256 lanes owns 1024 pixels of one (sample, slice),
// i.e. 1024 K floats, 4 K per lane.  prob and acc are addressed as flat float runs -- lane
// `tid` takes floats tid, tid + 256, ... of the workgroup's rows, so a wave's access is 256
// contiguous bytes whatever K is (a K = 3 pixel is 12 bytes and is never addressed as a vector).
//  * Without T the pixels are a strip of row segments 32, 64 or 128 pixels wide (whole rows up
//    to W = 128: one contiguous run in and out).  FH / FD pick another row / slice; FW reverses
//    the pixel order of a segment, not the K floats inside a pixel.  K = 1, 2, 4 with rows of
//    whole 16-byte vectors and aligned buffers take tta_acc_strip_kernel: the same strips with
//    one 16-byte access per 4 / K pixels (5.1 -> 5.6 TB/s at b1024 128 x 128, profiles/r12_tta.md).
//  * With T the pixels are a 32 x 32 tile: the source rows (32 K floats each) are written to LDS
//    by rows and read back by columns, so the global loads and stores are both whole row
//    segments of 128 K bytes.  LDS row pitch 33 K floats: a 32-lane half reads 32 consecutive
//    floats j = lw K + k of an output row from addresses lw * 33 K + lh K + k = 32 K lw + j +
//    const, 32 distinct banks; a half's row write is 32 consecutive dwords (tools/
//    lds_bank_model.py check_tta_tile, tests/test_tta_cpu.py).
// All of a lane's loads (the acc values of add mode too) are issued before the first use; a
// pixel past the image edge re-reads the edge pixel and is not stored.
//
// tta_finish: prob = (acc + prob) * inv_m in place (an add, then a multiplication by the exact
// 1 / M) and, of that mean p and the target t, the block partials of
//   I = sum t p, St = sum t, Sp = sum p, BCE = -sum [t max(log p, -100) + (1 - t) max(log(1 - p), -100)]
// (precise logf / log1pf), reduced in fixed order by partial_reduce_launch into sums[4].
// No atomics anywhere: two runs give the same bits.
#pragma once
#include "common.h"

namespace unet {
namespace {

constexpr int TTA_TILE = 32;                      // tile side (pixels)
constexpr int TTA_THREADS = 256;
constexpr int TTA_PIXELS = TTA_TILE * TTA_TILE;   // pixels per workgroup
constexpr int TTA_FB = 1024;                      // most blocks of the finish

// ntile: workgroups per (sample, slice); across: of them per row of strips / tiles;
// shift: log2 of the strip width (5 with T: the tile)
template <int K>
__global__ void __launch_bounds__(TTA_THREADS) tta_acc_kernel(const float* __restrict__ prob, float* __restrict__ acc,
                                                              int D, int H, int ntile, int across, int shift,
                                                              int code, int add) {
  constexpr int NF = TTA_PIXELS * K / TTA_THREADS;          // floats per lane
  constexpr int PITCH = (TTA_TILE + 1) * K;                 // LDS row pitch (floats)
  __shared__ float tile[TTA_TILE * PITCH];
  const int W = H;
  int bid = blockIdx.x;
  const int t = bid % ntile;
  bid /= ntile;
  const int d = bid % D, n = bid / D;
  const bool fw = code & 1, fh = code & 2, tr = code & 4, fd = code & 8;     // (workgroup-uniform)
  const int ti = t / across, tj = t - ti * across;
  const int oh0 = ti * (TTA_PIXELS >> shift), ow0 = tj << shift;
  const int a0 = tr ? ow0 : oh0, b0 = tr ? oh0 : ow0;       // source tile origin before the flips
  const size_t sbase = ((size_t)n * D + (fd ? D - 1 - d : d)) * H * W;
  const size_t obase = ((size_t)n * D + d) * H * W;
  const int cmask = (1 << shift) - 1;

  // float f = tid + 256 i of the workgroup: pixel q = f / K (row q >> shift, column q & cmask
  // of the strip / tile), class k = f % K
  float v[NF], old[NF];
  size_t oidx[NF];
  bool ok[NF];
#pragma unroll
  for (int i = 0; i < NF; ++i) {
    const int f = (int)threadIdx.x + TTA_THREADS * i;
    const int q = f / K, k = f - q * K;
    const int row = q >> shift, col = q & cmask;
    const int a = min(a0 + row, H - 1), b = min(b0 + col, W - 1);
    const size_t s = sbase + (size_t)(fh ? H - 1 - a : a) * W + (fw ? W - 1 - b : b);
    v[i] = prob[s * K + k];
    old[i] = 0.f;
    const int oh = oh0 + row, ow = ow0 + col;
    ok[i] = oh < H && ow < W;
    oidx[i] = (obase + (size_t)min(oh, H - 1) * W + min(ow, W - 1)) * K + k;
  }
  if (add) {
#pragma unroll
    for (int i = 0; i < NF; ++i) old[i] = acc[oidx[i]];
  }
  __builtin_amdgcn_sched_barrier(0);        // every load issued before the first use

  if (tr) {
    // transpose through LDS (shift == 5): float f sits at [row][col K + k] = row * PITCH + f % (32 K);
    // output float f of row lh reads [col][lh K + k]
#pragma unroll
    for (int i = 0; i < NF; ++i) {
      const int f = (int)threadIdx.x + TTA_THREADS * i;
      const int row = f / (TTA_TILE * K);
      tile[row * PITCH + (f - row * TTA_TILE * K)] = v[i];
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < NF; ++i) {
      const int f = (int)threadIdx.x + TTA_THREADS * i;
      const int q = f / K, k = f - q * K;
      v[i] = tile[(q & (TTA_TILE - 1)) * PITCH + (q >> 5) * K + k];
    }
  }
#pragma unroll
  for (int i = 0; i < NF; ++i)
    if (ok[i]) acc[oidx[i]] = add ? old[i] + v[i] : v[i];
}

// The strip path (codes without T) of K = 1, 2, 4 with 16-byte accesses, for rows of a whole
// number of vectors (W K % 4 == 0) and 16-byte aligned prob / acc: a vector is PV = 4 / K whole
// pixels of one row, lane tid takes vectors tid + 256 i (i < K) of the workgroup's rows.  A W
// flip reads the mirrored vector (also aligned: W and the vector's first column are multiples
// of PV) and reverses its pixels in registers, not the K floats inside a pixel.
template <int K>
__global__ void __launch_bounds__(TTA_THREADS) tta_acc_strip_kernel(const float* __restrict__ prob,
                                                                    float* __restrict__ acc, int D, int H, int ntile,
                                                                    int across, int shift, int code, int add) {
  static_assert(K == 1 || K == 2 || K == 4, "whole pixels per 16-byte vector");
  constexpr int PV = 4 / K;                                 // pixels per vector
  const int W = H;
  int bid = blockIdx.x;
  const int t = bid % ntile;
  bid /= ntile;
  const int d = bid % D, n = bid / D;
  const bool fw = code & 1, fh = code & 2, fd = code & 8;
  const int ti = t / across, tj = t - ti * across;
  const int oh0 = ti * (TTA_PIXELS >> shift), ow0 = tj << shift;
  const size_t sbase = ((size_t)n * D + (fd ? D - 1 - d : d)) * H * W;
  const size_t obase = ((size_t)n * D + d) * H * W;
  const int cmask = (1 << shift) - 1;
  f32x4 v[K], old[K];
  size_t oidx[K];
  bool ok[K];
#pragma unroll
  for (int i = 0; i < K; ++i) {
    const int q = ((int)threadIdx.x + TTA_THREADS * i) * PV;          // first pixel of the vector
    const int oh = oh0 + (q >> shift), ow = ow0 + (q & cmask);
    ok[i] = oh < H && ow < W;
    const int a = min(oh, H - 1), b = min(ow, W - PV);
    const size_t s = sbase + (size_t)(fh ? H - 1 - a : a) * W + (fw ? W - PV - b : b);
    v[i] = *(const f32x4*)(prob + s * K);
    oidx[i] = (obase + (size_t)a * W + b) * K;
    old[i] = (f32x4){0.f, 0.f, 0.f, 0.f};
  }
  if (add) {
#pragma unroll
    for (int i = 0; i < K; ++i) old[i] = *(const f32x4*)(acc + oidx[i]);
  }
  __builtin_amdgcn_sched_barrier(0);        // every load issued before the first use
#pragma unroll
  for (int i = 0; i < K; ++i) {
    f32x4 r = v[i];
    if (fw && K == 1) r = (f32x4){v[i][3], v[i][2], v[i][1], v[i][0]};
    if (fw && K == 2) r = (f32x4){v[i][2], v[i][3], v[i][0], v[i][1]};
    if (ok[i]) *(f32x4*)(acc + oidx[i]) = add ? old[i] + r : r;
  }
}

__device__ __forceinline__ void tta_load_t(const h16* t, size_t e0, float* f) {
  const u32x2 w = *(const u32x2*)(t + e0);
  const f32x2 lo = unpack2(w[0]), hi = unpack2(w[1]);
  f[0] = lo[0];
  f[1] = lo[1];
  f[2] = hi[0];
  f[3] = hi[1];
}
__device__ __forceinline__ void tta_load_t(const float* t, size_t e0, float* f) {
  const f32x4 a = *(const f32x4*)(t + e0);
#pragma unroll
  for (int i = 0; i < 4; ++i) f[i] = a[i];
}

// nvec: 4-element vectors (16 bytes of prob / acc); partial [gridDim.x][4] = {I, St, Sp, BCE}
template <typename TT>
__global__ void __launch_bounds__(TTA_THREADS) tta_finish_kernel(float* __restrict__ prob,
                                                                 const float* __restrict__ acc,
                                                                 const TT* __restrict__ tgt, int nvec, float inv_m,
                                                                 float* __restrict__ partial) {
  __shared__ float red[TTA_THREADS / 64][4];
  float s[4] = {0.f, 0.f, 0.f, 0.f};
  for (int vi = blockIdx.x * TTA_THREADS + (int)threadIdx.x; vi < nvec; vi += gridDim.x * TTA_THREADS) {
    const size_t e0 = (size_t)vi * 4;
    const f32x4 p = *(const f32x4*)(prob + e0), a = *(const f32x4*)(acc + e0);
    float t[4];
    tta_load_t(tgt, e0, t);
    f32x4 m;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      m[e] = (a[e] + p[e]) * inv_m;
      s[0] += t[e] * m[e];
      s[1] += t[e];
      s[2] += m[e];
      s[3] -= t[e] * fmaxf(logf(m[e]), -100.f) + (1.f - t[e]) * fmaxf(log1pf(-m[e]), -100.f);
    }
    *(f32x4*)(prob + e0) = m;
  }
#pragma unroll
  for (int q = 0; q < 4; ++q) s[q] = wave_sum(s[q]);
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int q = 0; q < 4; ++q) red[threadIdx.x >> 6][q] = s[q];
  }
  __syncthreads();
  if (threadIdx.x < 4) {
    float r = 0.f;
#pragma unroll
    for (int w = 0; w < TTA_THREADS / 64; ++w) r += red[w][threadIdx.x];
    partial[(size_t)blockIdx.x * 4 + threadIdx.x] = r;
  }
}

}  // namespace

const char* tta_acc_check(long long N, long long D, long long H, long long W, long long K, long long code,
                          long long mode);
const char* tta_finish_check(long long total);
int tta_finish_blocks(long long total);
hipError_t partial_reduce_launch(const float* partial, int nb, int width, float* out, hipStream_t s);

// partial: tta_finish_blocks(total) * 4 floats
template <typename TT>
hipError_t tta_finish_launch_t(float* prob, const float* acc, const TT* t, long long total, float inv_m,
                               float* partial, float* sums, hipStream_t s) {
  if (tta_finish_check(total) || !prob || !acc || !t || !partial || !sums) return hipErrorInvalidValue;
  const int nb = tta_finish_blocks(total);
  UNET_LAUNCH((tta_finish_kernel<TT>), dim3(nb), dim3(TTA_THREADS), 0, s, prob, acc, t, (int)(total / 4), inv_m,
              partial);
  return partial_reduce_launch(partial, nb, 4, sums, s);
}

}  // namespace unet
