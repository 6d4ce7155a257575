// Augmenting, cropping batch gather on gfx950: gather_batch (elementwise.hip) reading a patch
// of a stored sample with a per-sample geometric transform and an optional per-channel affine
// riding on the same pass.  These are the copy kernels of gather_batch_aug (patch = the whole
// sample) and gather_batch_crop; gather_resample.h builds the warp and the elastic op on the
// helpers of this file, and the one launcher of all four is there.
//
//   x_all  fp32 [Nall][Ds][Hs][Ws][Cin]   y_all fp32 [Nall][Ds][Hs][Ws][K]
//   idx    int64 [B]   origin int32 [B][3] = (d, h, w) or null (= 0)   code int32 [B] or null (= 0)
//   affine fp32 [B][Cin][2] = {scale, shift} or null
//   xb     TT [B][D][H][W][Cpad] (pad channels zero)      tb TT [B][D][H][W][K]
//   H == W, D <= Ds, H <= Hs, W <= Ws;  TT: the build's 16-bit type, or float for the fp32 executor
//
// code bits: 0 FW (flip W), 1 FH (flip H), 2 T (swap H and W), 3 FD (flip D, 3D only).
// Output pixel (d, h, w) of sample b reads source voxel origin[b] + (d', h', w') of sample idx[b]:
//   d' = FD ? D-1-d : d;   (a, b) = T ? (w, h) : (h, w);   h' = FH ? H-1-a : a;   w' = FW ? W-1-b : b
// and x' = fma(scale[c], x, shift[c]) in fp32 before the rounding to TT (image only).  Each
// origin component is clamped into [0, S_a - T_a] before use: the origin is device data the
// launch cannot validate, and no value of it reads out of bounds.
//
// Tiled kernel (Cpad 4 and 8): a workgroup of 256 lanes owns 1024 pixels of one (sample,
// slice); code and origin are per sample, so every branch on them is workgroup-uniform.  The
// pixels are loaded in whole row segments (16 bytes per pixel at Cin = 4, which every origin
// keeps aligned), rows Ws pixels apart: FW only reverses the lane order inside a segment, FH /
// FD only pick another row / slice.  All of a lane's loads are issued before the first use; a
// pixel is converted (and the affine, read once per workgroup, applied) in registers.
//  * Without T the 1024 pixels are a strip of row segments 32, 64 or 128 pixels wide --
//    whole rows up to W = 128, so the workgroup writes one contiguous run (and reads one when
//    the patch is the whole sample), as gather_batch does -- and a lane stores the pixels it
//    loaded.  (32 x 32 tiles of a 128 x 128 image, 512-byte read and 256-byte write segments a
//    row apart, cost 4-7 % of the pass on an MI355X; at 32 x 32 images, where a tile is the
//    image, nothing: profiles/r9_augment.md.)
//  * With T the pixels are a 32 x 32 tile, lane (r, c) = (tid >> 5, tid & 31) loads patch
//    pixels (a0 + r + 8 i, b0 + c), i < 4; the tile goes through LDS, written [a][b] row by
//    row and read back [b][a], so the global stores are whole 32-pixel row segments too.
// LDS pitches (tools/lds_bank_model.py, tests/test_lds_gather_aug.py): a pixel is NW dwords
// (2, 4, 8); rows of 32 NW + 2 dwords for NW = 2 (the 8-byte transposed reads of a 32-lane
// half land on 32 distinct bank pairs) and 32 NW + 4 for NW = 4, 8 (the 16-byte reads of a
// lane group land on 16 distinct 16-byte slots; the row writes of NW = 8, fp32 with 8
// channels, are 2-way); the K target values are kept as fp32 planes [k][a][33].
// All source offsets are size_t (a resident set of 155 x 240 x 240 x 4 volumes exceeds 2^31
// elements).
//
// Any other Cpad <= 64: one lane per output pixel (correct, the T reads are not coalesced).
// Plain vector loads and stores only: no atomics, two runs give the same bits.
#pragma once
#include "common.h"

namespace unet {
namespace {

constexpr int GA_TILE = 32;                       // tile side (pixels)
constexpr int GA_THREADS = 256;
constexpr int GA_PX = GA_TILE * GA_TILE / GA_THREADS;   // pixels per lane
constexpr int GA_ROWS = GA_THREADS / GA_TILE;     // tile rows per pass
constexpr int GA_TP = GA_TILE + 1;                // pitch of a target plane (floats)

template <typename TT>
struct GaPerDword {
  static constexpr int value = sizeof(TT) == 4 ? 1 : 2;
};

// dwords per output pixel and the LDS row pitch in dwords
template <int CPAD, typename TT>
struct GaLayout {
  static constexpr int NW = CPAD / GaPerDword<TT>::value;
  static constexpr int PITCH = GA_TILE * NW + (NW == 2 ? 2 : 4);
};

template <int CPAD>
__device__ __forceinline__ void ga_pack(const float* v, uint32_t* w, const h16*) {
#pragma unroll
  for (int j = 0; j < CPAD / 2; ++j) w[j] = pack2h(v[2 * j], v[2 * j + 1]);
}
template <int CPAD>
__device__ __forceinline__ void ga_pack(const float* v, uint32_t* w, const float*) {
#pragma unroll
  for (int j = 0; j < CPAD; ++j) w[j] = __builtin_bit_cast(uint32_t, v[j]);
}

// NW dwords, 8-byte (NW = 2) or 16-byte aligned
template <int NW>
__device__ __forceinline__ void ga_put(uint32_t* p, const uint32_t* w) {
  if constexpr (NW == 2) {
    *(u32x2*)p = (u32x2){w[0], w[1]};
  } else {
#pragma unroll
    for (int q = 0; q < NW; q += 4) *(u32x4*)(p + q) = (u32x4){w[q], w[q + 1], w[q + 2], w[q + 3]};
  }
}
template <int NW>
__device__ __forceinline__ void ga_get(const uint32_t* p, uint32_t* w) {
  if constexpr (NW == 2) {
    const u32x2 v = *(const u32x2*)p;
    w[0] = v[0];
    w[1] = v[1];
  } else {
#pragma unroll
    for (int q = 0; q < NW; q += 4) {
      const u32x4 v = *(const u32x4*)(p + q);
#pragma unroll
      for (int e = 0; e < 4; ++e) w[q + e] = v[e];
    }
  }
}

// the transform code of sample n (null: 0); FD only in 3D
__device__ __forceinline__ int ga_code(const int* __restrict__ code, int n, int D) {
  return code ? code[n] & (D > 1 ? 15 : 7) : 0;
}

// the clamped origin of sample n: (d, h, w), each in [0, S_a - T_a]; (0, 0, 0) when a null origin
// is allowed and given
struct GcOrigin {
  int d, h, w;
};
template <bool NULLABLE = true>
__device__ __forceinline__ GcOrigin gc_origin(const int* __restrict__ origin, int n, int Ds, int Hs, int Ws, int D,
                                              int H, int W) {
  GcOrigin o = {0, 0, 0};
  if (!NULLABLE || origin) {
    o.d = min(max(origin[3 * (size_t)n], 0), Ds - D);
    o.h = min(max(origin[3 * (size_t)n + 1], 0), Hs - H);
    o.w = min(max(origin[3 * (size_t)n + 2], 0), Ws - W);
  }
  return o;
}

// row 0, column 0 of the stored slice that output slice d of sample n reads
__device__ __forceinline__ size_t ga_slice(const long long* __restrict__ idx, int n, int d, int cd, const GcOrigin& og,
                                           int Ds, int Hs, int Ws, int D) {
  return (((size_t)idx[n] * Ds + og.d + ((cd & 8) ? D - 1 - d : d)) * Hs) * Ws;
}

// the affine of sample n into sc[] / sf[] (only channels < Cin are used); null without an affine.
// One uniform branch and every load at a clamped address, so the scalar loads are issued
// together and waited for once
template <int CPAD>
__device__ __forceinline__ const float* ga_affine(const float* __restrict__ affine, int n, int Cin, float* sc,
                                                  float* sf) {
  if (!affine) {
#pragma unroll
    for (int ch = 0; ch < CPAD; ++ch) sc[ch] = 1.f, sf[ch] = 0.f;
    return nullptr;
  }
  const float* af = affine + (size_t)n * Cin * 2;
#pragma unroll
  for (int ch = 0; ch < CPAD; ++ch) {
    const int c = min(ch, Cin - 1);
    sc[ch] = af[2 * c], sf[ch] = af[2 * c + 1];
  }
  return af;
}
// the same for one channel of the pixel kernels (no fma without an affine: fma(1, -0, 0) is +0)
__device__ __forceinline__ float ga_affine1(const float* af, int ch, float v) {
  return af ? fmaf(af[2 * ch], v, af[2 * ch + 1]) : v;
}

// one pixel's Cin channels, zero-padded to CPAD: 16-byte loads at Cin == CPAD
template <int CPAD>
__device__ __forceinline__ void ga_load(const float* __restrict__ src, int Cin, float* v) {
  if (Cin == CPAD) {
#pragma unroll
    for (int q = 0; q < CPAD; q += 4) {
      const f32x4 t = *(const f32x4*)(src + q);
#pragma unroll
      for (int e = 0; e < 4; ++e) v[q + e] = t[e];
    }
  } else {
#pragma unroll
    for (int ch = 0; ch < CPAD; ++ch) v[ch] = ch < Cin ? src[ch] : 0.f;
  }
}

// the affine, where there is one, and the rounding to TT: v -> the pixel's NW dwords
template <int CPAD, typename TT>
__device__ __forceinline__ void ga_convert(const float* v, bool af, const float* sc, const float* sf, int Cin,
                                           uint32_t* w) {
  float u[CPAD];
#pragma unroll
  for (int ch = 0; ch < CPAD; ++ch) u[ch] = v[ch];
  if (af) {                                     // (no fma without an affine: fma(1, -0, 0) is +0)
#pragma unroll
    for (int ch = 0; ch < CPAD; ++ch)
      if (ch < Cin) u[ch] = fmaf(sc[ch], v[ch], sf[ch]);
  }
  ga_pack<CPAD>(u, w, (const TT*)nullptr);
}

// output pixel o: its dwords and its K target values
template <int CPAD, typename TT>
__device__ __forceinline__ void ga_store(TT* __restrict__ xb, TT* __restrict__ tb, size_t o, const uint32_t* w,
                                         const float* tv, int K) {
  ga_put<GaLayout<CPAD, TT>::NW>((uint32_t*)(xb + o * CPAD), w);
#pragma unroll
  for (int k = 0; k < 4; ++k)
    if (k < K) tb[o * K + k] = (TT)tv[k];
}

// output pixel i of [B][D][H][W] for the kernels of one lane per pixel: its sample, its slice
// and its patch coordinates (h', w') under the sample's code cd
struct GaPixel {
  int n, d, h, w, cd;
};
__device__ __forceinline__ GaPixel ga_pixel(int i, const int* __restrict__ code, int D, int H, int W) {
  GaPixel p;
  const int ow = i % W;
  int t = i / W;
  const int oh = t % H;
  t /= H;
  p.d = t % D, p.n = t / D;
  p.cd = ga_code(code, p.n, D);
  const int a = (p.cd & 4) ? ow : oh, b = (p.cd & 4) ? oh : ow;
  p.h = (p.cd & 2) ? H - 1 - a : a, p.w = (p.cd & 1) ? W - 1 - b : b;
  return p;
}

// grid: B * D * ntile workgroups (ntile: the larger of the two tilings' counts per slice; a
// workgroup past its sample's count leaves at once); dynamic LDS: K * GA_TILE * GA_TP floats.
// strip_log2: log2 of the strip width of the codes without T (5, 6 or 7).  CROP: origin is not
// null (its loads are then issued with the workgroup's other scalar loads, not behind a branch)
template <int CPAD, typename TT, bool CROP>
__global__ void __launch_bounds__(GA_THREADS) gather_copy_tile_kernel(
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
  const int cd = ga_code(code, n, D);
  const bool fw = cd & 1, fh = cd & 2, tr = cd & 4;
  // the workgroup's 1024 output pixels: a 32 x 32 tile with T, else a strip of whole row
  // segments 2^strip_log2 wide (whole rows up to W = 128: one contiguous run out)
  const int shift = tr ? 5 : strip_log2;
  const int across = tr ? tiles : (W + (1 << shift) - 1) >> shift;
  const int ti = t / across, tj = t - ti * across;
  const int oh0 = ti * ((GA_TILE * GA_TILE) >> shift), ow0 = tj << shift;
  if (oh0 >= H) return;
  const int a0 = tr ? ow0 : oh0, b0 = tr ? oh0 : ow0;     // patch tile origin before the flips
  const GcOrigin og = CROP ? gc_origin<false>(origin, n, Ds, Hs, Ws, D, H, W) : GcOrigin{0, 0, 0};
  // the patch's first voxel of the source slice; rows from here are Ws pixels apart
  const size_t sbase = ga_slice(idx, n, d, cd, og, Ds, Hs, Ws, D) + (size_t)og.h * Ws + og.w;
  const size_t obase = ((size_t)n * D + d) * H * W;
  const int r = threadIdx.x >> shift, c = threadIdx.x & ((1 << shift) - 1), rows = GA_THREADS >> shift;

  // the sample's affine, once per workgroup (scalar loads)
  float sc[CPAD], sf[CPAD];
  const bool af = ga_affine<CPAD>(affine, n, Cin, sc, sf);
  // every load of the lane's pixels is issued before the first use: no branch around them (a
  // pixel past the patch edge re-reads the edge pixel and is never stored)
  float v[GA_PX][CPAD], tv[GA_PX][4];
#pragma unroll
  for (int i = 0; i < GA_PX; ++i) {
    const int a = min(a0 + r + rows * i, H - 1), b = min(b0 + c, W - 1);
    const size_t s = sbase + (size_t)(fh ? H - 1 - a : a) * Ws + (fw ? W - 1 - b : b);
    ga_load<CPAD>(x_all + s * Cin, Cin, v[i]);
#pragma unroll
    for (int k = 0; k < 4; ++k) tv[i][k] = k < K ? y_all[s * K + k] : 0.f;
  }
  __builtin_amdgcn_sched_barrier(0);
  uint32_t w[GA_PX][NW];
#pragma unroll
  for (int i = 0; i < GA_PX; ++i) ga_convert<CPAD, TT>(v[i], af, sc, sf, Cin, w[i]);

  if (!tr) {
    // (a, b) is the output pixel
#pragma unroll
    for (int i = 0; i < GA_PX; ++i) {
      const int oh = oh0 + r + rows * i, ow = ow0 + c;
      if (oh < H && ow < W) ga_store<CPAD>(xb, tb, obase + (size_t)oh * W + ow, w[i], tv[i], K);
    }
    return;
  }
  // transpose through LDS (shift == 5: r < 8, c < 32, rows == GA_ROWS): rows in, columns out; pixels
  // past the patch edge are never read back
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
      uint32_t q[NW];
      float tq[4];
      ga_get<NW>(xs + c * PITCH + lh * NW, q);
#pragma unroll
      for (int k = 0; k < 4; ++k) tq[k] = k < K ? ts[(k * GA_TILE + c) * GA_TP + lh] : 0.f;
      ga_store<CPAD>(xb, tb, obase + (size_t)oh * W + ow, q, tq, K);
    }
  }
}

// any Cpad <= 64: one lane per output pixel, B D H W < 2^31
template <typename TT>
__global__ void __launch_bounds__(GA_THREADS) gather_copy_pixel_kernel(
    const float* __restrict__ x_all, const float* __restrict__ y_all, const long long* __restrict__ idx,
    const int* __restrict__ origin, const int* __restrict__ code, const float* __restrict__ affine, int B, int Ds,
    int Hs, int Ws, int D, int H, int Cin, int Cpad, int K, TT* __restrict__ xb, TT* __restrict__ tb) {
  const int W = H;
  const int total = B * D * H * W;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
    const GaPixel p = ga_pixel(i, code, D, H, W);
    const GcOrigin og = gc_origin(origin, p.n, Ds, Hs, Ws, D, H, W);
    const size_t s = ga_slice(idx, p.n, p.d, p.cd, og, Ds, Hs, Ws, D) + (size_t)(og.h + p.h) * Ws + og.w + p.w;
    const float* src = x_all + s * Cin;
    const float* af = affine ? affine + (size_t)p.n * Cin * 2 : nullptr;
    TT* dst = xb + (size_t)i * Cpad;
    for (int ch = 0; ch < Cpad; ++ch) dst[ch] = (TT)(ch < Cin ? ga_affine1(af, ch, src[ch]) : 0.f);
    for (int k = 0; k < K; ++k) tb[(size_t)i * K + k] = (TT)y_all[s * K + k];
  }
}

}  // namespace
}  // namespace unet
