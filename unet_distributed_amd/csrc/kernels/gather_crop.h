// Cropping, augmenting batch gather on gfx950: gather_batch_aug (gather_aug.h) reading a
// patch of a larger stored sample, so a resident set of full-size images feeds a model of a
// smaller input size in the same single pass.
//
//   x_all  fp32 [Nall][Ds][Hs][Ws][Cin]   y_all fp32 [Nall][Ds][Hs][Ws][K]
//   idx    int64 [B]   origin int32 [B][3] = (d, h, w)   code int32 [B] or null (= 0)
//   affine fp32 [B][Cin][2] = {scale, shift} or null
//   xb     TT [B][D][H][W][Cpad] (pad channels zero)      tb TT [B][D][H][W][K]
//   H == W, D <= Ds, H <= Hs, W <= Ws;  TT: the build's 16-bit type, or float
//
// Output pixel (d, h, w) of sample b reads source voxel origin[b] + (d', h', w') of sample
// idx[b], with (d', h', w') gather_aug.h's code mapping inside the patch, and the same affine
// fma and rounding.  Each origin component is clamped into [0, S_a - T_a] before use: the
// origin is device data the launch cannot validate, and no value of it reads out of bounds.
//
// The structure is gather_aug.h's (its packing helpers and LDS layout are used as they are):
// 256-lane workgroups own 1024 output pixels -- row strips 32, 64 or 128 pixels wide for the
// codes without T, 32 x 32 tiles through LDS with T -- all of a lane's loads are issued
// before the first use, and code, origin and affine are workgroup-uniform.  The one new thing
// is that a source row is a segment of W pixels at pitch Ws, no longer part of one contiguous
// run: a strip's rows are 16 W Cin / 4-byte segments Ws pixels apart.  At Cin = 4 a pixel is
// 16 bytes, so every origin keeps the 16-byte loads aligned.  All source offsets are size_t
// (a resident set of 155 x 240 x 240 x 4 volumes exceeds 2^31 elements).
//
// Any other Cpad <= 64: one lane per output pixel.  Plain vector loads and stores only: no
// atomics, two runs give the same bits.
#pragma once
#include "gather_aug.h"

namespace unet {
namespace {

// the clamped origin of sample n: (d, h, w), each in [0, S_a - T_a]
struct GcOrigin {
  int d, h, w;
};
__device__ __forceinline__ GcOrigin gc_origin(const int* __restrict__ origin, int n, int Ds, int Hs, int Ws, int D,
                                              int H, int W) {
  GcOrigin o;
  o.d = min(max(origin[3 * (size_t)n], 0), Ds - D);
  o.h = min(max(origin[3 * (size_t)n + 1], 0), Hs - H);
  o.w = min(max(origin[3 * (size_t)n + 2], 0), Ws - W);
  return o;
}

// grid, dynamic LDS, strip_log2: as gather_aug_tile_kernel
template <int CPAD, typename TT>
__global__ void __launch_bounds__(GA_THREADS) gather_crop_tile_kernel(
    const float* __restrict__ x_all, const float* __restrict__ y_all, const long long* __restrict__ idx,
    const int* __restrict__ origin, const int* __restrict__ code, const float* __restrict__ affine, int Ds, int Hs,
    int Ws, int D, int H, int tiles, int ntile, int strip_log2, int Cin, int K, TT* __restrict__ xb,
    TT* __restrict__ tb) {
  constexpr int NW = GaLayout<CPAD, TT>::NW, PITCH = GaLayout<CPAD, TT>::PITCH;
  __shared__ __attribute__((aligned(16))) uint32_t xs[GA_TILE * PITCH];
  extern __shared__ float ts[];
  const int W = H;
  int bid = blockIdx.x;
  const int t = bid % ntile;
  bid /= ntile;
  const int d = bid % D, n = bid / D;
  const int cd = code ? code[n] & (D > 1 ? 15 : 7) : 0;
  const bool fw = cd & 1, fh = cd & 2, tr = cd & 4, fd = cd & 8;
  const int shift = tr ? 5 : strip_log2;
  const int across = tr ? tiles : (W + (1 << shift) - 1) >> shift;
  const int ti = t / across, tj = t - ti * across;
  const int oh0 = ti * ((GA_TILE * GA_TILE) >> shift), ow0 = tj << shift;
  if (oh0 >= H) return;
  const int a0 = tr ? ow0 : oh0, b0 = tr ? oh0 : ow0;     // patch tile origin before the flips
  const GcOrigin og = gc_origin(origin, n, Ds, Hs, Ws, D, H, W);
  // the patch's first voxel of the source slice; rows from here are Ws pixels apart
  const size_t sbase = (((size_t)idx[n] * Ds + og.d + (fd ? D - 1 - d : d)) * Hs + og.h) * Ws + og.w;
  const size_t obase = ((size_t)n * D + d) * H * W;
  const float* af = affine ? affine + (size_t)n * Cin * 2 : nullptr;
  const int r = threadIdx.x >> shift, c = threadIdx.x & ((1 << shift) - 1), rows = GA_THREADS >> shift;

  float sc[CPAD], sf[CPAD];
#pragma unroll
  for (int ch = 0; ch < CPAD; ++ch) {
    sc[ch] = (af && ch < Cin) ? af[2 * ch] : 1.f;
    sf[ch] = (af && ch < Cin) ? af[2 * ch + 1] : 0.f;
  }
  // every load of the lane's pixels is issued before the first use: no branch around them (a
  // pixel past the patch edge re-reads the edge pixel and is never stored)
  float v[GA_PX][CPAD], tv[GA_PX][4];
#pragma unroll
  for (int i = 0; i < GA_PX; ++i) {
    const int a = min(a0 + r + rows * i, H - 1), b = min(b0 + c, W - 1);
    const size_t s = sbase + (size_t)(fh ? H - 1 - a : a) * Ws + (fw ? W - 1 - b : b);
    const float* src = x_all + s * Cin;
    if (Cin == CPAD) {
#pragma unroll
      for (int q = 0; q < CPAD; q += 4) {
        const f32x4 t = *(const f32x4*)(src + q);
#pragma unroll
        for (int e = 0; e < 4; ++e) v[i][q + e] = t[e];
      }
    } else {
#pragma unroll
      for (int ch = 0; ch < CPAD; ++ch) v[i][ch] = ch < Cin ? src[ch] : 0.f;
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) tv[i][k] = k < K ? y_all[s * K + k] : 0.f;
  }
  __builtin_amdgcn_sched_barrier(0);
  uint32_t w[GA_PX][NW];
#pragma unroll
  for (int i = 0; i < GA_PX; ++i) {
    if (af) {                                   // (no fma without an affine: fma(1, -0, 0) is +0)
#pragma unroll
      for (int ch = 0; ch < CPAD; ++ch)
        if (ch < Cin) v[i][ch] = fmaf(sc[ch], v[i][ch], sf[ch]);
    }
    ga_pack<CPAD>(v[i], w[i], (const TT*)nullptr);
  }

  if (!tr) {
#pragma unroll
    for (int i = 0; i < GA_PX; ++i) {
      const int oh = oh0 + r + rows * i, ow = ow0 + c;
      if (oh < H && ow < W) {
        const size_t o = obase + (size_t)oh * W + ow;
        ga_put<NW>((uint32_t*)(xb + o * CPAD), w[i]);
#pragma unroll
        for (int k = 0; k < 4; ++k)
          if (k < K) tb[o * K + k] = (TT)tv[i][k];
      }
    }
    return;
  }
  // transpose through LDS, exactly as gather_aug_tile_kernel
#pragma unroll
  for (int i = 0; i < GA_PX; ++i) {
    const int ra = r + GA_ROWS * i;
    ga_put<NW>(xs + ra * PITCH + c * NW, w[i]);
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (k < K) ts[(k * GA_TILE + ra) * GA_TP + c] = tv[i][k];
  }
  __syncthreads();
#pragma unroll
  for (int i = 0; i < GA_PX; ++i) {
    const int lh = r + GA_ROWS * i;
    const int oh = oh0 + lh, ow = ow0 + c;
    if (oh < H && ow < W) {
      const size_t o = obase + (size_t)oh * W + ow;
      uint32_t q[NW];
      ga_get<NW>(xs + c * PITCH + lh * NW, q);
      ga_put<NW>((uint32_t*)(xb + o * CPAD), q);
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (k < K) tb[o * K + k] = (TT)ts[(k * GA_TILE + c) * GA_TP + lh];
    }
  }
}

// any Cpad <= 64: one lane per output pixel, B D H W < 2^31
template <typename TT>
__global__ void __launch_bounds__(GA_THREADS) gather_crop_pixel_kernel(
    const float* __restrict__ x_all, const float* __restrict__ y_all, const long long* __restrict__ idx,
    const int* __restrict__ origin, const int* __restrict__ code, const float* __restrict__ affine, int B, int Ds,
    int Hs, int Ws, int D, int H, int Cin, int Cpad, int K, TT* __restrict__ xb, TT* __restrict__ tb) {
  const int W = H;
  const int total = B * D * H * W;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
    const int ow = i % W;
    int t = i / W;
    const int oh = t % H;
    t /= H;
    const int d = t % D, n = t / D;
    const int cd = code ? code[n] & (D > 1 ? 15 : 7) : 0;
    const int a = (cd & 4) ? ow : oh, b = (cd & 4) ? oh : ow;
    const GcOrigin og = gc_origin(origin, n, Ds, Hs, Ws, D, H, W);
    const size_t s = (((size_t)idx[n] * Ds + og.d + ((cd & 8) ? D - 1 - d : d)) * Hs + og.h +
                      ((cd & 2) ? H - 1 - a : a)) * Ws + og.w + ((cd & 1) ? W - 1 - b : b);
    const float* src = x_all + s * Cin;
    const float* af = affine ? affine + (size_t)n * Cin * 2 : nullptr;
    TT* dst = xb + (size_t)i * Cpad;
    for (int ch = 0; ch < Cpad; ++ch) {
      float v = 0.f;
      if (ch < Cin) v = af ? fmaf(af[2 * ch], src[ch], af[2 * ch + 1]) : src[ch];
      dst[ch] = (TT)v;
    }
    for (int k = 0; k < K; ++k) tb[(size_t)i * K + k] = (TT)y_all[s * K + k];
  }
}

}  // namespace

// null when the shape is one the launch accepts, else the reason: gather_aug_check's
// conditions on the patch, plus patch <= stored on every axis
const char* gather_crop_check(long long B, long long Ds, long long Hs, long long Ws, long long D, long long H,
                              long long W, long long Cin, long long Cpad, long long K);

template <typename TT>
hipError_t gather_batch_crop_launch_t(const float* x_all, const float* y_all, const long long* idx, const int* origin,
                                      const int* code, const float* affine, int B, int Ds, int Hs, int Ws, int D, int H,
                                      int W, int Cin, int Cpad, int K, TT* xb, TT* tb, hipStream_t s) {
  if (gather_crop_check(B, Ds, Hs, Ws, D, H, W, Cin, Cpad, K) || !x_all || !y_all || !idx || !origin || !xb || !tb)
    return hipErrorInvalidValue;
  const int tiles = (H + GA_TILE - 1) / GA_TILE;
  // strips of the codes without T: 32, 64 or 128 pixels wide, 1024 pixels each
  const int strip_log2 = W <= 32 ? 5 : (W <= 64 ? 6 : 7);
  const int strip_h = (GA_TILE * GA_TILE) >> strip_log2;
  const int nstrip = ((W + (1 << strip_log2) - 1) >> strip_log2) * ((H + strip_h - 1) / strip_h);
  const int ntile = tiles * tiles > nstrip ? tiles * tiles : nstrip;
  if ((long long)B * D * ntile >= (1LL << 31)) return hipErrorInvalidValue;
  const int grid = B * D * ntile;
  const size_t shm = (size_t)K * GA_TILE * GA_TP * sizeof(float);
  if (Cpad == 4) {
    UNET_LAUNCH((gather_crop_tile_kernel<4, TT>), dim3(grid), dim3(GA_THREADS), shm, s, x_all, y_all, idx, origin, code,
                affine, Ds, Hs, Ws, D, H, tiles, ntile, strip_log2, Cin, K, xb, tb);
  } else if (Cpad == 8) {
    UNET_LAUNCH((gather_crop_tile_kernel<8, TT>), dim3(grid), dim3(GA_THREADS), shm, s, x_all, y_all, idx, origin, code,
                affine, Ds, Hs, Ws, D, H, tiles, ntile, strip_log2, Cin, K, xb, tb);
  } else {
    const long long total = (long long)B * D * H * W;
    const int blocks = (int)((total + GA_THREADS - 1) / GA_THREADS < 65536 ? (total + GA_THREADS - 1) / GA_THREADS
                                                                           : 65536);
    UNET_LAUNCH((gather_crop_pixel_kernel<TT>), dim3(blocks), dim3(GA_THREADS), 0, s, x_all, y_all, idx, origin, code,
                affine, B, Ds, Hs, Ws, D, H, Cin, Cpad, K, xb, tb);
  }
  return launch_status();
}

}  // namespace unet
