// Elastic batch gather on gfx950: gather_batch_warp (gather_warp.h) with a smooth per-pixel
// displacement added to its source coordinates, a quadratic B-spline through a per-sample lattice
// of control-node displacements, in the same single pass.
//
//   x_all  fp32 [Nall][Ds][Hs][Ws][Cin]   y_all fp32 [Nall][Ds][Hs][Ws][K]
//   idx    int64 [B]   origin int32 [B][3] or null (= 0)   code int32 [B] or null (= 0)
//   mat    int32 [B][4], Q16, or null (= the identity)     affine fp32 [B][Cin][2] or null
//   field  int32 [B][N][N][2] = node (i, j)'s displacement along (h, w) in 2^-17 pixel,
//          N = ((H - 1) >> s) + 3, cells of S = 1 << s patch pixels, 3 <= s <= 6
//   xb     TT [B][D][H][W][Cpad] (pad channels zero)      tb TT [B][D][H][W][K]
//
// The geometry is integer, so the op equals its torch definition (data/augment.py elastic_torch)
// bit for bit.  Output voxel (d, h, w) of sample b maps through gather_aug.h's code mapping to
// patch coordinates (d', h', w'); there, with u = 2 h' - (H - 1), v = 2 w' - (W - 1),
//   ci = h' >> s, t = h' & (S - 1),  wh = [(S - t)^2, -2 t^2 + 2 S t + S^2, t^2]   (sum 2 S^2)
//   d_c = (sum_a wh[a] sum_b ww[b] f[ci + a][cj + b][c]) >> (2 + 4 s)          (ww, cj from w')
//   Qh = (origin.h << 17) + (H - 1) 65536 + a00 u + a01 v + d_0
//   Qw = (origin.w << 17) + (W - 1) 65536 + a10 u + a11 v + d_1
// and from Q on everything is gather_warp.h's: taps, weights, per-op fp32 rounding, nearest target,
// zero outside the stored image, clamped addresses, no branch.  Every field entry is clamped into
// [-2^22, 2^22] (32 pixels) before use, the origin and the matrix as in gather_warp.h: all are
// device data the launch cannot validate.  A weight product wh[a] ww[b] is at most 9/4 S^4 < 2^26
// and fits an int; times an entry it is one 32 x 32 -> 64-bit multiply-add, nine per component;
// the sum stays below 4 S^4 2^22 = 2^48 and the shift is arithmetic (floor).  Every depth slice of
// a sample uses the same field.  Unlike the warp the code cannot be folded into the matrix (the
// displacement is indexed by (h', w')), so Q is evaluated at the patch coordinates themselves.
//
// Tiled kernel (Cpad 4 and 8): gather_warp.h's lane mapping (16 x 4 wave tile, four passes, a
// 32 x 32 workgroup tile).  A tile's patch coordinates span at most 32 pixels per axis, that is
// at most 32 / S + 1 cells and 32 / S + 3 <= 7 nodes: the workgroup stages those nodes of its
// sample once in LDS, clamped, as (d_h, d_w) pairs, and a pixel reads its 3 x 3 of them as nine
// 8-byte LDS loads.  A lane's column is the same in all four passes, so its three weights along
// that axis are formed once.  All tap and target loads of a lane are issued before the first use.
//
// Any other Cpad <= 64: one lane per output pixel, the nine nodes read from global memory.
// Plain vector loads and stores only: no atomics, two runs give the same bits.
#pragma once
#include "gather_warp.h"

namespace unet {
namespace {

constexpr int GE_FIELD_MAX = 1 << 22;             // clamp of a field entry (2^-17 pixel: 32 pixels)
constexpr int GE_NODES = 7;                       // nodes per axis a 32-pixel span can touch at S = 8

// the sample's clamped matrix (null: the identity) and the patch centre in 2^-17 pixel
__device__ __forceinline__ GwMap ge_map(const int* __restrict__ mat, int n, const GcOrigin& og, int H, int W) {
  GwMap g;
  g.m00 = g.m11 = 1 << 16, g.m01 = g.m10 = 0;
  if (mat) {
    int a[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) a[e] = min(max(mat[4 * (size_t)n + e], -GW_MAT_MAX), GW_MAT_MAX);
    g.m00 = a[0], g.m01 = a[1], g.m10 = a[2], g.m11 = a[3];
  }
  g.ch = ((long long)og.h << 17) + (long long)(H - 1) * 65536;
  g.cw = ((long long)og.w << 17) + (long long)(W - 1) * 65536;
  return g;
}

// the integer quadratic B-spline weights of offset t inside a cell of S = 1 << s pixels
__device__ __forceinline__ void ge_weights(int t, int s, int w[3]) {
  const int S = 1 << s;
  w[0] = (S - t) * (S - t), w[1] = -2 * t * t + 2 * S * t + S * S, w[2] = t * t;
}

// gw_tap at patch pixel (ph, pw) with the displacement (dh, dw) added to the source coordinates
__device__ __forceinline__ GwTap ge_tap(const GwMap& g, int ph, int pw, long long dh, long long dw, int H, int W,
                                        int Hs, int Ws) {
  const long long u = 2 * ph - (H - 1), v = 2 * pw - (W - 1);
  const long long qh = g.ch + g.m00 * u + g.m01 * v + dh, qw = g.cw + g.m10 * u + g.m11 * v + dw;
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

// grid: B * D * th * tw workgroups of a GW_WGW x GW_TILE_H pixel tile each
template <int CPAD, typename TT>
__global__ void __launch_bounds__(GA_THREADS) gather_elastic_tile_kernel(
    const float* __restrict__ x_all, const float* __restrict__ y_all, const long long* __restrict__ idx,
    const int* __restrict__ origin, const int* __restrict__ code, const int* __restrict__ mat,
    const float* __restrict__ affine, const int* __restrict__ field, int Ds, int Hs, int Ws, int D, int H, int th,
    int tw, int Cin, int K, int s, TT* __restrict__ xb, TT* __restrict__ tb) {
#pragma clang fp contract(off)
  constexpr int NW = GaLayout<CPAD, TT>::NW;
  __shared__ __attribute__((aligned(8))) int fs[GE_NODES * GE_NODES * 2];
  const int W = H;
  int bid = blockIdx.x;
  const int tj = bid % tw;
  bid /= tw;
  const int ti = bid % th;
  bid /= th;
  const int d = bid % D, n = bid / D;
  const int cd = code ? code[n] & (D > 1 ? 15 : 7) : 0;
  const bool fw = cd & 1, fh = cd & 2, tr = cd & 4;
  GcOrigin og = {0, 0, 0};
  if (origin) og = gc_origin(origin, n, Ds, Hs, Ws, D, H, W);
  const GwMap g = ge_map(mat, n, og, H, W);

  // the tile's span of patch coordinates: output rows [ti 32, ...] and columns [tj 32, ...] clipped
  // to the patch, swapped by T and mirrored by the flips; its first cell per axis
  const int olo_h = ti * GW_TILE_H, ohi_h = min(olo_h + GW_TILE_H, H) - 1;
  const int olo_w = tj * GW_WGW, ohi_w = min(olo_w + GW_WGW, W) - 1;
  const int alo = tr ? olo_w : olo_h, ahi = tr ? ohi_w : ohi_h;     // h' before the flip
  const int blo = tr ? olo_h : olo_w, bhi = tr ? ohi_h : ohi_w;     // w' before the flip
  const int ci0 = (fh ? H - 1 - ahi : alo) >> s, cj0 = (fw ? W - 1 - bhi : blo) >> s;
  const int N = ((H - 1) >> s) + 3;
  {
    // stage nodes (ci0 + r, cj0 + c), r, c < 7: the load is unconditional at a clamped address
    const int e = min((int)threadIdx.x, GE_NODES * GE_NODES * 2 - 1);
    const int r = e / (2 * GE_NODES), c = (e >> 1) % GE_NODES;
    const size_t at = (((size_t)n * N + min(ci0 + r, N - 1)) * N + min(cj0 + c, N - 1)) * 2 + (e & 1);
    const int f = min(max(field[at], -GE_FIELD_MAX), GE_FIELD_MAX);
    if (threadIdx.x < GE_NODES * GE_NODES * 2) fs[e] = f;
  }
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
  // the lane's column: a w' without T, an h' with it; the same in every pass
  const int cmask = (1 << s) - 1;
  const int owc = min(ow, W - 1);
  const int pcol = tr ? (fh ? H - 1 - owc : owc) : (fw ? W - 1 - owc : owc);
  int wcol[3];
  ge_weights(pcol & cmask, s, wcol);
  // LDS strides of the node pairs along the row's and the column's axis, and the column's base
  const int srow = tr ? 2 : 2 * GE_NODES, scol = tr ? 2 * GE_NODES : 2;
  const int bcol = ((pcol >> s) - (tr ? ci0 : cj0)) * scol;
  const int shift = 2 + 4 * s;
  __syncthreads();

  // every load of the lane's pixels is issued before the first use: no branch around them (a
  // pixel past the patch edge maps like the edge pixel and is never stored; every address is
  // clamped into the slice)
  GwTap t[GW_PX];
  float p[GW_PX][4][CPAD], tv[GW_PX][4];
#pragma unroll
  for (int i = 0; i < GW_PX; ++i) {
    const int ohc = min(oh0 + GW_PH * i, H - 1);
    const int prow = tr ? (fw ? W - 1 - ohc : ohc) : (fh ? H - 1 - ohc : ohc);
    int wrow[3];
    ge_weights(prow & cmask, s, wrow);
    const int* nd = fs + ((prow >> s) - (tr ? cj0 : ci0)) * srow + bcol;
    long long dh = 0, dw = 0;
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
      for (int b = 0; b < 3; ++b) {
        const int2 f = *(const int2*)(nd + a * srow + b * scol);
        const int w2 = wrow[a] * wcol[b];
        dh += (long long)w2 * f.x;
        dw += (long long)w2 * f.y;
      }
    dh >>= shift, dw >>= shift;
    t[i] = ge_tap(g, tr ? pcol : prow, tr ? prow : pcol, dh, dw, H, W, Hs, Ws);
    const size_t sa[4] = {sbase + (size_t)t[i].r0 * Ws + t[i].c0, sbase + (size_t)t[i].r0 * Ws + t[i].c1,
                          sbase + (size_t)t[i].r1 * Ws + t[i].c0, sbase + (size_t)t[i].r1 * Ws + t[i].c1};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float* src = x_all + sa[j] * Cin;
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
__global__ void __launch_bounds__(GA_THREADS) gather_elastic_pixel_kernel(
    const float* __restrict__ x_all, const float* __restrict__ y_all, const long long* __restrict__ idx,
    const int* __restrict__ origin, const int* __restrict__ code, const int* __restrict__ mat,
    const float* __restrict__ affine, const int* __restrict__ field, int B, int Ds, int Hs, int Ws, int D, int H,
    int Cin, int Cpad, int K, int s, TT* __restrict__ xb, TT* __restrict__ tb) {
#pragma clang fp contract(off)
  const int W = H;
  const int total = B * D * H * W;
  const int N = ((H - 1) >> s) + 3, cmask = (1 << s) - 1;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
    const int ow = i % W;
    int r = i / W;
    const int oh = r % H;
    r /= H;
    const int d = r % D, n = r / D;
    const int cd = code ? code[n] & (D > 1 ? 15 : 7) : 0;
    const int a = (cd & 4) ? ow : oh, b = (cd & 4) ? oh : ow;
    const int ph = (cd & 2) ? H - 1 - a : a, pw = (cd & 1) ? W - 1 - b : b;
    GcOrigin og = {0, 0, 0};
    if (origin) og = gc_origin(origin, n, Ds, Hs, Ws, D, H, W);
    const GwMap g = ge_map(mat, n, og, H, W);
    int wh[3], ww[3];
    ge_weights(ph & cmask, s, wh);
    ge_weights(pw & cmask, s, ww);
    const int* nd = field + (((size_t)n * N + (ph >> s)) * N + (pw >> s)) * 2;
    long long dh = 0, dw = 0;
    for (int e = 0; e < 3; ++e)
      for (int f = 0; f < 3; ++f) {
        const int w2 = wh[e] * ww[f];
        dh += (long long)w2 * min(max(nd[((size_t)e * N + f) * 2], -GE_FIELD_MAX), GE_FIELD_MAX);
        dw += (long long)w2 * min(max(nd[((size_t)e * N + f) * 2 + 1], -GE_FIELD_MAX), GE_FIELD_MAX);
      }
    const GwTap t = ge_tap(g, ph, pw, dh >> (2 + 4 * s), dw >> (2 + 4 * s), H, W, Hs, Ws);
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

// null when the shape is one the launch accepts, else the reason: gather_warp_check's conditions
// and 3 <= s <= 6
const char* gather_elastic_check(long long B, long long Ds, long long Hs, long long Ws, long long D, long long H,
                                 long long W, long long Cin, long long Cpad, long long K, long long s);

template <typename TT>
hipError_t gather_batch_elastic_launch_t(const float* x_all, const float* y_all, const long long* idx,
                                         const int* origin, const int* code, const int* mat, const float* affine,
                                         const int* field, int B, int Ds, int Hs, int Ws, int D, int H, int W, int Cin,
                                         int Cpad, int K, int s, TT* xb, TT* tb, hipStream_t st) {
  if (gather_elastic_check(B, Ds, Hs, Ws, D, H, W, Cin, Cpad, K, s) || !x_all || !y_all || !idx || !field || !xb ||
      !tb)
    return hipErrorInvalidValue;
  const int th = (H + GW_TILE_H - 1) / GW_TILE_H, tw = (W + GW_WGW - 1) / GW_WGW;
  if ((long long)B * D * th * tw >= (1LL << 31)) return hipErrorInvalidValue;
  const int grid = B * D * th * tw;
  if (Cpad == 4) {
    UNET_LAUNCH((gather_elastic_tile_kernel<4, TT>), dim3(grid), dim3(GA_THREADS), 0, st, x_all, y_all, idx, origin,
                code, mat, affine, field, Ds, Hs, Ws, D, H, th, tw, Cin, K, s, xb, tb);
  } else if (Cpad == 8) {
    UNET_LAUNCH((gather_elastic_tile_kernel<8, TT>), dim3(grid), dim3(GA_THREADS), 0, st, x_all, y_all, idx, origin,
                code, mat, affine, field, Ds, Hs, Ws, D, H, th, tw, Cin, K, s, xb, tb);
  } else {
    const long long total = (long long)B * D * H * W;
    const int blocks = (int)((total + GA_THREADS - 1) / GA_THREADS < 65536 ? (total + GA_THREADS - 1) / GA_THREADS
                                                                           : 65536);
    UNET_LAUNCH((gather_elastic_pixel_kernel<TT>), dim3(blocks), dim3(GA_THREADS), 0, st, x_all, y_all, idx, origin,
                code, mat, affine, field, B, Ds, Hs, Ws, D, H, Cin, Cpad, K, s, xb, tb);
  }
  return launch_status();
}

}  // namespace unet
