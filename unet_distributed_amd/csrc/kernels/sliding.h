// Sliding-window inference on gfx950: device-side tile extraction, the weighted blend of the
// tile predictions and the division by the summed weights (ops/sliding.py is the definition
// and the oracle; the kernels are held to it bit for bit).
//
//   x_all fp32 [N][D][H][W][C]      the images, any spatial size (D = 1 in 2D)
//   xb    fp32 [B][Td][Th][Tw][C]   one staging batch of tiles, the model's input shape
//   prob  fp32 [B][Td][Th][Tw][K]   the head's probabilities of that batch (K = 1..4)
//   w     fp32 [Td][Th][Tw]         the blend weights
//   acc   fp32 [N][D][H][W][K]      the accumulator, then the result
//   wsum  fp32 [D][H][W]            the summed weights of one image (host, once per geometry)
//
// Geometry (SwGeo): per axis of length L, tile T and stride s the tile origins are {0} when
// L <= T, else o_i = min(i s, L - T) for i < n = ceil((L - T) / s) + 1 -- the last tile is
// clamped to end at the edge.  Tile t = ((n_img nd + id) nh + ih) nw + iw; a batch holds the
// tiles [t0, t0 + nt), tile t0 + b in slot b.
//
// sw_extract: slot b < nt of xb = tile t0 + b, the slots b >= nt and the positions past an
// image smaller than the tile = 0.  A tile row is Tw C contiguous floats of the source: a
// workgroup owns a group of rows of one (slot, ld) slab (its tile decode is workgroup-uniform)
// and copies them as flat runs, lane `tid` taking units tid, tid + 256, ... -- 16-byte
// vectors when the rows, the row starts and both bases are 16-byte aligned, floats otherwise.
//
// sw_blend: output-centric, no atomics.  A workgroup owns (a 1024-float piece of) one row
// (n, d, h) of the images the batch touches, a lane the floats f = w K + k of it.  The
// covering grid indices of d and h are workgroup-uniform; per axis they are walked in
// ascending order, so the tile index ascends, and every covering tile inside [t0, t0 + nt)
// does a = a + w * p -- an fp32 multiplication, then an fp32 addition: the function body is
// compiled with `fp contract(off)`, which (unlike __fmul_rn / __fadd_rn) keeps hipcc from
// forming v_fmac_f32.  A float no tile of the batch covers is neither read nor written.
// Batches issued in order on one stream give every float its sum in ascending tile order.
//
// sw_finish: acc[n][p][k] = acc[n][p][k] / wsum[p] in place, the correctly rounded division
// (no fast-math in this build).
//
// Plain loads and stores only, no LDS; every loop bound comes from the geometry, never from
// data: two runs give the same bits.
#pragma once
#include "common.h"

namespace unet {
namespace {

constexpr int SW_THREADS = 256;
constexpr int SW_UNITS = 1024;        // units (extract) / floats (blend) per workgroup

__host__ __device__ __forceinline__ int sw_origin(int i, int s, int L, int T) {
  return L <= T ? 0 : (i * s < L - T ? i * s : L - T);
}

// VEC: floats per unit (4: 16-byte vectors, 1: floats); rowlen: units per tile row;
// rg: rows per workgroup.  grid (B Td, ceil(Th / rg))
template <int VEC>
__global__ void __launch_bounds__(SW_THREADS) sw_extract_kernel(const float* __restrict__ x_all,
                                                                float* __restrict__ xb, SwGeo g, int rowlen, int rg) {
  const int slab = blockIdx.x;                       // (b, ld)
  const int ld = slab % g.Td, b = slab / g.Td;
  const int h0 = blockIdx.y * rg;
  const int rows = min(rg, g.Th - h0);
  // workgroup-uniform tile decode
  bool live = b < g.nt;
  int n = 0, od = 0, oh = 0, ow = 0;
  if (live) {
    const int tpi = g.nd * g.nh * g.nw;
    const int t = g.t0 + b;
    n = t / tpi;
    int r = t - n * tpi;
    const int iw = r % g.nw;
    r /= g.nw;
    const int ih = r % g.nh, id = r / g.nh;
    od = sw_origin(id, g.sd, g.D, g.Td);
    oh = sw_origin(ih, g.sh, g.H, g.Th);
    ow = sw_origin(iw, g.sw, g.W, g.Tw);
    live = od + ld < g.D;
  }
  const int valid = min(g.Tw, g.W - ow) * g.C;       // floats of a row inside the image
  const size_t src0 = (((size_t)n * g.D + (od + ld)) * g.H + oh) * g.W + ow;   // pixel of row lh = 0
  const size_t dst0 = ((size_t)slab * g.Th + h0) * rowlen;                     // unit of the first row
  for (int u = threadIdx.x; u < rows * rowlen; u += SW_THREADS) {
    const int lr = u / rowlen, j = u - lr * rowlen;
    const int lh = h0 + lr;
    const bool in = live && oh + lh < g.H && j * VEC < valid;
    if (VEC == 4) {
      f32x4 v = (f32x4){0.f, 0.f, 0.f, 0.f};
      if (in) v = *(const f32x4*)(x_all + (src0 + (size_t)lh * g.W) * g.C + (size_t)j * 4);
      *(f32x4*)(xb + (dst0 + u) * 4) = v;
    } else {
      float v = 0.f;
      if (in) v = x_all[(src0 + (size_t)lh * g.W) * g.C + j];
      xb[dst0 + u] = v;
    }
  }
}

// covering grid indices [lo, hi] of coordinate x on an axis (a superset: the caller tests
// each origin): unclamped tiles i s <= x < i s + T, and the clamped last tile from L - T on
__device__ __forceinline__ void sw_range(int x, int L, int T, int s, int n, int& lo, int& hi) {
  lo = x >= T ? (x - T) / s + 1 : 0;
  hi = min(x / s, n - 1);
  if (L > T && x >= L - T) hi = n - 1;
}

// grid (rows = images touched x D x H, ceil(W K / SW_UNITS)); n_lo: the first image touched
template <int K>
__global__ void __launch_bounds__(SW_THREADS) sw_blend_kernel(const float* __restrict__ prob,
                                                              const float* __restrict__ wmap,
                                                              float* __restrict__ acc, SwGeo g, int n_lo) {
#pragma clang fp contract(off)
  int row = blockIdx.x;
  const int h = row % g.H;
  row /= g.H;
  const int d = row % g.D, n = n_lo + row / g.D;
  int dlo, dhi, hlo, hhi;
  sw_range(d, g.D, g.Td, g.sd, g.nd, dlo, dhi);
  sw_range(h, g.H, g.Th, g.sh, g.nh, hlo, hhi);
  const size_t e0 = (((size_t)n * g.D + d) * g.H + h) * g.W * K;
  const int rowf = g.W * K;
#pragma unroll 1
  for (int f = blockIdx.y * SW_UNITS + (int)threadIdx.x; f < min(rowf, (int)(blockIdx.y + 1) * SW_UNITS);
       f += SW_THREADS) {
    const int x = f / K, k = f - x * K;
    int wlo, whi;
    sw_range(x, g.W, g.Tw, g.sw, g.nw, wlo, whi);
    float a = 0.f;
    bool any = false;
    for (int id = dlo; id <= dhi; ++id) {
      const int ld = d - sw_origin(id, g.sd, g.D, g.Td);
      if (ld < 0 || ld >= g.Td) continue;
      for (int ih = hlo; ih <= hhi; ++ih) {
        const int lh = h - sw_origin(ih, g.sh, g.H, g.Th);
        if (lh < 0 || lh >= g.Th) continue;
        for (int iw = wlo; iw <= whi; ++iw) {
          const int lw = x - sw_origin(iw, g.sw, g.W, g.Tw);
          if (lw < 0 || lw >= g.Tw) continue;
          const int b = ((n * g.nd + id) * g.nh + ih) * g.nw + iw - g.t0;
          if (b < 0 || b >= g.nt) continue;
          if (!any) {
            a = acc[e0 + f];
            any = true;
          }
          const size_t q = (((size_t)b * g.Td + ld) * g.Th + lh) * g.Tw + lw;
          const float wv = wmap[((size_t)ld * g.Th + lh) * g.Tw + lw];
          const float pr = wv * prob[q * K + k];
          a = a + pr;
        }
      }
    }
    if (any) acc[e0 + f] = a;
  }
}

// total = N P K floats, P = D H W pixels of an image
template <int K>
__global__ void __launch_bounds__(SW_THREADS) sw_finish_kernel(float* __restrict__ acc,
                                                               const float* __restrict__ wsum, unsigned total,
                                                               unsigned P) {
  const unsigned e = blockIdx.x * SW_THREADS + threadIdx.x;      // (total < 2^31: no wrap)
  if (e >= total) return;
  const unsigned p = (e / K) % P;
  acc[e] = acc[e] / wsum[p];
}

}  // namespace

// kind 0: sw_extract (C >= 1), 1: sw_blend (C = K in 1..4)
const char* sw_check(long long kind, long long N, long long D, long long H, long long W, long long C, long long Td,
                     long long Th, long long Tw, long long sd, long long sh, long long sw, long long B, long long t0,
                     long long nt);
const char* sw_finish_check(long long N, long long D, long long H, long long W, long long K);
SwGeo sw_geo(const long long* v);
hipError_t sw_extract_launch(const float* x_all, float* xb, const SwGeo& g, hipStream_t s);
hipError_t sw_blend_launch(const float* prob, const float* w, float* acc, const SwGeo& g, hipStream_t s);
hipError_t sw_finish_launch(float* acc, const float* wsum, int N, int D, int H, int W, int K, hipStream_t s);

}  // namespace unet
