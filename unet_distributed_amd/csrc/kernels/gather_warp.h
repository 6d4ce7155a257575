// Resampling batch gather on gfx950: gather_batch_crop (gather_crop.h) with a per-sample 2 x 2
// matrix in the (H, W) plane -- rotation by any angle and isotropic zoom -- riding on the same
// single pass.  The image is interpolated bilinearly, the target is read at the nearest voxel.
//
//   x_all  fp32 [Nall][Ds][Hs][Ws][Cin]   y_all fp32 [Nall][Ds][Hs][Ws][K]
//   idx    int64 [B]   origin int32 [B][3] = (d, h, w) or null (= 0)   code int32 [B] or null (= 0)
//   mat    int32 [B][4] = (a00, a01, a10, a11), Q16   affine fp32 [B][Cin][2] or null
//   xb     TT [B][D][H][W][Cpad] (pad channels zero)      tb TT [B][D][H][W][K]
//   H == W, D <= Ds, H <= Hs, W <= Ws;  TT: the build's 16-bit type, or float
//
// The geometry is integer, so the op equals its torch definition (data/augment.py warp_torch)
// bit for bit.  Output voxel (d, h, w) of sample b maps through gather_aug.h's code mapping to
// patch coordinates (d', h', w'); the slice is origin.d + d' (depth is not interpolated) and
//   u = 2 h' - (H - 1),  v = 2 w' - (W - 1)
//   Qh = (origin.h << 17) + (H - 1) 65536 + a00 u + a01 v      (2^-17 pixel of the stored image)
//   Qw = (origin.w << 17) + (W - 1) 65536 + a10 u + a11 v
// with the origin clamped as gather_crop.h clamps it and every matrix entry clamped into
// [-2^18, 2^18]: both are device data the launch cannot validate.  |u|, |v| < 2^16 and a stored
// side is below 2^20 (gather_warp_check), so |Q| < 2^38: Qh and Qw are 64-bit, the pixel
// indices Q >> 17 fit an int.  The flips negate u or v and T swaps them, so the code only
// permutes and negates the matrix applied to the output's own (u, v): there is no transposing
// path and no LDS.
//
// Image: ih = Qh >> 17, fh = Qh & 0x1FFFF (w alike); taps p_ij = x[ih + i][iw + j], 0.0f when the
// row or the column is outside the stored image (the address is clamped, the value selected:
// nothing is read out of bounds and there is no branch); weights wh1 = fh 2^-17, wh0 =
// (131072 - fh) 2^-17, exact in fp32;
//   r0 = p00 ww0 + p01 ww1,  r1 = p10 ww0 + p11 ww1,  value = r0 wh0 + r1 wh1
// every product and sum rounded to fp32 on its own: the kernels are compiled with
// `fp contract(off)` (sliding.h says why), the affine's explicit fmaf stays an fma.
// Target: nh = (Qh + 65536) >> 17, nw alike; y there, 0.0f outside.
//
// Tiled kernel (Cpad 4 and 8): output-centric, a lane owns whole output pixels.  A wave is a
// 16 x 4 pixel tile (16 along W): at 45 degrees its taps stay inside a few dozen 128-byte lines
// of the source where a 64 x 1 strip walks across 64 rows, and 16 pixels of 16-bit Cpad 4 are
// still one whole 128-byte line of the output.  A workgroup of 4 waves owns 32 x 8 pixels per
// pass and GW_PX = 4 passes, a 32 x 32 tile (measured against 64 x 1, 32 x 2 and 8 x 8 wave
// tiles and 1 or 2 passes: profiles/r16_warp.md); all tap and target loads of a lane are issued
// before the first use;
// code, origin, matrix and affine are workgroup-uniform.  At Cin == Cpad a tap is 16-byte loads
// (a pixel is 16 bytes at Cin = 4: every tap address is aligned).  All source offsets are size_t.
//
// Any other Cpad <= 64: one lane per output pixel.  Plain vector loads and stores only: no
// atomics, two runs give the same bits.
#pragma once
#include "gather_crop.h"

namespace unet {
namespace {

constexpr int GW_TW_LOG2 = 4;                     // wave tile: 16 pixels along W ...
constexpr int GW_TW = 1 << GW_TW_LOG2;
constexpr int GW_TH = 64 / GW_TW;                 // ... by 4 along H
constexpr int GW_WGW = GW_TW < 32 ? 32 : GW_TW;   // workgroup: waves side by side up to 32 pixels,
constexpr int GW_ACROSS = GW_WGW / GW_TW;
constexpr int GW_PH = GW_TH * (GA_THREADS / 64 / GW_ACROSS);    // the rest stacked: rows per pass
constexpr int GW_PX = 4;                          // passes = pixels per lane
constexpr int GW_TILE_H = GW_PH * GW_PX;
constexpr int GW_MAT_MAX = 1 << 18;               // clamp of a matrix entry (Q16: a zoom of 1/4)

// the sample's matrix acting on the output pixel's own (u, v) = (2 h - (H-1), 2 w - (W-1)), and
// the patch centre in 2^-17 pixel of the stored image
struct GwMap {
  long long ch, cw;
  int m00, m01, m10, m11;
};
__device__ __forceinline__ GwMap gw_map(const int* __restrict__ mat, int n, int cd, const GcOrigin& og, int H, int W) {
  int a[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) a[e] = min(max(mat[4 * (size_t)n + e], -GW_MAT_MAX), GW_MAT_MAX);
  // u' = (FH ? -1 : 1) (T ? v : u),  v' = (FW ? -1 : 1) (T ? u : v)
  const int sh = (cd & 2) ? -1 : 1, sw = (cd & 1) ? -1 : 1;
  GwMap g;
  if (cd & 4) {
    g.m00 = sw * a[1], g.m01 = sh * a[0], g.m10 = sw * a[3], g.m11 = sh * a[2];
  } else {
    g.m00 = sh * a[0], g.m01 = sw * a[1], g.m10 = sh * a[2], g.m11 = sw * a[3];
  }
  g.ch = ((long long)og.h << 17) + (long long)(H - 1) * 65536;
  g.cw = ((long long)og.w << 17) + (long long)(W - 1) * 65536;
  return g;
}

// one output pixel's source: clamped tap rows / columns, their validity, the weights, and the
// nearest voxel of the target
struct GwTap {
  int r0, r1, c0, c1, nr, nc;
  bool r0ok, r1ok, c0ok, c1ok, nok;
  float wh0, wh1, ww0, ww1;
};
__device__ __forceinline__ GwTap gw_tap(const GwMap& g, int oh, int ow, int H, int W, int Hs, int Ws) {
  const long long u = 2 * oh - (H - 1), v = 2 * ow - (W - 1);
  const long long qh = g.ch + g.m00 * u + g.m01 * v, qw = g.cw + g.m10 * u + g.m11 * v;
  const int ih = (int)(qh >> 17), iw = (int)(qw >> 17);
  const int fh = (int)(qh & 0x1FFFF), fw = (int)(qw & 0x1FFFF);
  const int nh = (int)((qh + 65536) >> 17), nw = (int)((qw + 65536) >> 17);
  GwTap t;
  t.r0ok = ih >= 0 && ih < Hs, t.r1ok = ih + 1 >= 0 && ih + 1 < Hs;
  t.c0ok = iw >= 0 && iw < Ws, t.c1ok = iw + 1 >= 0 && iw + 1 < Ws;
  t.nok = nh >= 0 && nh < Hs && nw >= 0 && nw < Ws;
  t.r0 = min(max(ih, 0), Hs - 1), t.r1 = min(max(ih + 1, 0), Hs - 1);
  t.c0 = min(max(iw, 0), Ws - 1), t.c1 = min(max(iw + 1, 0), Ws - 1);
  t.nr = min(max(nh, 0), Hs - 1), t.nc = min(max(nw, 0), Ws - 1);
  t.wh1 = (float)fh * 0x1p-17f, t.wh0 = (float)(131072 - fh) * 0x1p-17f;
  t.ww1 = (float)fw * 0x1p-17f, t.ww0 = (float)(131072 - fw) * 0x1p-17f;
  return t;
}

// products first, sums left to right, each rounded on its own (the caller's contract is off)
__device__ __forceinline__ float gw_lerp(float p00, float p01, float p10, float p11, const GwTap& t) {
#pragma clang fp contract(off)
  const float a = p00 * t.ww0, b = p01 * t.ww1, c = p10 * t.ww0, d = p11 * t.ww1;
  const float r0 = a + b, r1 = c + d;
  const float e = r0 * t.wh0, f = r1 * t.wh1;
  return e + f;
}

// grid: B * D * th * tw workgroups of a GW_WGW x GW_TILE_H pixel tile each
template <int CPAD, typename TT>
__global__ void __launch_bounds__(GA_THREADS) gather_warp_tile_kernel(
    const float* __restrict__ x_all, const float* __restrict__ y_all, const long long* __restrict__ idx,
    const int* __restrict__ origin, const int* __restrict__ code, const int* __restrict__ mat,
    const float* __restrict__ affine, int Ds, int Hs, int Ws, int D, int H, int th, int tw, int Cin, int K,
    TT* __restrict__ xb, TT* __restrict__ tb) {
#pragma clang fp contract(off)
  constexpr int NW = GaLayout<CPAD, TT>::NW;
  const int W = H;
  int bid = blockIdx.x;
  const int tj = bid % tw;
  bid /= tw;
  const int ti = bid % th;
  bid /= th;
  const int d = bid % D, n = bid / D;
  const int cd = code ? code[n] & (D > 1 ? 15 : 7) : 0;
  GcOrigin og = {0, 0, 0};
  if (origin) og = gc_origin(origin, n, Ds, Hs, Ws, D, H, W);
  const GwMap g = gw_map(mat, n, cd, og, H, W);
  // the source slice's first voxel
  const size_t sbase = (((size_t)idx[n] * Ds + og.d + ((cd & 8) ? D - 1 - d : d)) * Hs) * Ws;
  const size_t obase = ((size_t)n * D + d) * H * W;
  const float* af = affine ? affine + (size_t)n * Cin * 2 : nullptr;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int ow = tj * GW_WGW + (wave % GW_ACROSS) * GW_TW + (lane & (GW_TW - 1));
  const int oh0 = ti * GW_TILE_H + (wave / GW_ACROSS) * GW_TH + (lane >> GW_TW_LOG2);

  float sc[CPAD], sf[CPAD];
#pragma unroll
  for (int ch = 0; ch < CPAD; ++ch) {
    sc[ch] = (af && ch < Cin) ? af[2 * ch] : 1.f;
    sf[ch] = (af && ch < Cin) ? af[2 * ch + 1] : 0.f;
  }
  // every load of the lane's pixels is issued before the first use: no branch around them (a
  // pixel past the patch edge maps like the edge pixel and is never stored; every address is
  // clamped into the slice)
  GwTap t[GW_PX];
  float p[GW_PX][4][CPAD], tv[GW_PX][4];
#pragma unroll
  for (int i = 0; i < GW_PX; ++i) {
    t[i] = gw_tap(g, min(oh0 + GW_PH * i, H - 1), min(ow, W - 1), H, W, Hs, Ws);
    const size_t s[4] = {sbase + (size_t)t[i].r0 * Ws + t[i].c0, sbase + (size_t)t[i].r0 * Ws + t[i].c1,
                         sbase + (size_t)t[i].r1 * Ws + t[i].c0, sbase + (size_t)t[i].r1 * Ws + t[i].c1};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float* src = x_all + s[j] * Cin;
      if (Cin == CPAD) {
#pragma unroll
        for (int q = 0; q < CPAD; q += 4) {
          const f32x4 l = *(const f32x4*)(src + q);
#pragma unroll
          for (int e = 0; e < 4; ++e) p[i][j][q + e] = l[e];
        }
      } else {
#pragma unroll
        for (int ch = 0; ch < CPAD; ++ch) p[i][j][ch] = ch < Cin ? src[ch] : 0.f;
      }
    }
    const size_t sn = sbase + (size_t)t[i].nr * Ws + t[i].nc;
#pragma unroll
    for (int k = 0; k < 4; ++k) tv[i][k] = k < K ? y_all[sn * K + k] : 0.f;
  }
  __builtin_amdgcn_sched_barrier(0);
#pragma unroll
  for (int i = 0; i < GW_PX; ++i) {
    const bool ok[4] = {t[i].r0ok && t[i].c0ok, t[i].r0ok && t[i].c1ok, t[i].r1ok && t[i].c0ok,
                        t[i].r1ok && t[i].c1ok};
    float v[CPAD];
#pragma unroll
    for (int ch = 0; ch < CPAD; ++ch) {
      v[ch] = gw_lerp(ok[0] ? p[i][0][ch] : 0.f, ok[1] ? p[i][1][ch] : 0.f, ok[2] ? p[i][2][ch] : 0.f,
                      ok[3] ? p[i][3][ch] : 0.f, t[i]);
      if (af && ch < Cin) v[ch] = fmaf(sc[ch], v[ch], sf[ch]);
    }
    uint32_t w[NW];
    ga_pack<CPAD>(v, w, (const TT*)nullptr);
    const int oh = oh0 + GW_PH * i;
    if (oh < H && ow < W) {
      const size_t o = obase + (size_t)oh * W + ow;
      ga_put<NW>((uint32_t*)(xb + o * CPAD), w);
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (k < K) tb[o * K + k] = (TT)(t[i].nok ? tv[i][k] : 0.f);
    }
  }
}

// any Cpad <= 64: one lane per output pixel, B D H W < 2^31
template <typename TT>
__global__ void __launch_bounds__(GA_THREADS) gather_warp_pixel_kernel(
    const float* __restrict__ x_all, const float* __restrict__ y_all, const long long* __restrict__ idx,
    const int* __restrict__ origin, const int* __restrict__ code, const int* __restrict__ mat,
    const float* __restrict__ affine, int B, int Ds, int Hs, int Ws, int D, int H, int Cin, int Cpad, int K,
    TT* __restrict__ xb, TT* __restrict__ tb) {
#pragma clang fp contract(off)
  const int W = H;
  const int total = B * D * H * W;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
    const int ow = i % W;
    int r = i / W;
    const int oh = r % H;
    r /= H;
    const int d = r % D, n = r / D;
    const int cd = code ? code[n] & (D > 1 ? 15 : 7) : 0;
    GcOrigin og = {0, 0, 0};
    if (origin) og = gc_origin(origin, n, Ds, Hs, Ws, D, H, W);
    const GwMap g = gw_map(mat, n, cd, og, H, W);
    const GwTap t = gw_tap(g, oh, ow, H, W, Hs, Ws);
    const size_t sbase = (((size_t)idx[n] * Ds + og.d + ((cd & 8) ? D - 1 - d : d)) * Hs) * Ws;
    const float* s00 = x_all + (sbase + (size_t)t.r0 * Ws + t.c0) * Cin;
    const float* s01 = x_all + (sbase + (size_t)t.r0 * Ws + t.c1) * Cin;
    const float* s10 = x_all + (sbase + (size_t)t.r1 * Ws + t.c0) * Cin;
    const float* s11 = x_all + (sbase + (size_t)t.r1 * Ws + t.c1) * Cin;
    const bool ok00 = t.r0ok && t.c0ok, ok01 = t.r0ok && t.c1ok, ok10 = t.r1ok && t.c0ok, ok11 = t.r1ok && t.c1ok;
    const float* af = affine ? affine + (size_t)n * Cin * 2 : nullptr;
    TT* dst = xb + (size_t)i * Cpad;
    for (int ch = 0; ch < Cpad; ++ch) {
      float v = 0.f;
      if (ch < Cin) {
        v = gw_lerp(ok00 ? s00[ch] : 0.f, ok01 ? s01[ch] : 0.f, ok10 ? s10[ch] : 0.f, ok11 ? s11[ch] : 0.f, t);
        if (af) v = fmaf(af[2 * ch], v, af[2 * ch + 1]);
      }
      dst[ch] = (TT)v;
    }
    const size_t sn = sbase + (size_t)t.nr * Ws + t.nc;
    for (int k = 0; k < K; ++k) tb[(size_t)i * K + k] = (TT)(t.nok ? y_all[sn * K + k] : 0.f);
  }
}

}  // namespace

// null when the shape is one the launch accepts, else the reason: gather_crop_check's
// conditions (the 64-bit coordinates need no further bound on the sides)
const char* gather_warp_check(long long B, long long Ds, long long Hs, long long Ws, long long D, long long H,
                              long long W, long long Cin, long long Cpad, long long K);

template <typename TT>
hipError_t gather_batch_warp_launch_t(const float* x_all, const float* y_all, const long long* idx, const int* origin,
                                      const int* code, const int* mat, const float* affine, int B, int Ds, int Hs,
                                      int Ws, int D, int H, int W, int Cin, int Cpad, int K, TT* xb, TT* tb,
                                      hipStream_t s) {
  if (gather_warp_check(B, Ds, Hs, Ws, D, H, W, Cin, Cpad, K) || !x_all || !y_all || !idx || !mat || !xb || !tb)
    return hipErrorInvalidValue;
  const int th = (H + GW_TILE_H - 1) / GW_TILE_H, tw = (W + GW_WGW - 1) / GW_WGW;
  if ((long long)B * D * th * tw >= (1LL << 31)) return hipErrorInvalidValue;
  const int grid = B * D * th * tw;
  if (Cpad == 4) {
    UNET_LAUNCH((gather_warp_tile_kernel<4, TT>), dim3(grid), dim3(GA_THREADS), 0, s, x_all, y_all, idx, origin, code,
                mat, affine, Ds, Hs, Ws, D, H, th, tw, Cin, K, xb, tb);
  } else if (Cpad == 8) {
    UNET_LAUNCH((gather_warp_tile_kernel<8, TT>), dim3(grid), dim3(GA_THREADS), 0, s, x_all, y_all, idx, origin, code,
                mat, affine, Ds, Hs, Ws, D, H, th, tw, Cin, K, xb, tb);
  } else {
    const long long total = (long long)B * D * H * W;
    const int blocks = (int)((total + GA_THREADS - 1) / GA_THREADS < 65536 ? (total + GA_THREADS - 1) / GA_THREADS
                                                                           : 65536);
    UNET_LAUNCH((gather_warp_pixel_kernel<TT>), dim3(blocks), dim3(GA_THREADS), 0, s, x_all, y_all, idx, origin, code,
                mat, affine, B, Ds, Hs, Ws, D, H, Cin, Cpad, K, xb, tb);
  }
  return launch_status();
}

}  // namespace unet
