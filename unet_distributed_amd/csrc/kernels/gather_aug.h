// Augmenting batch gather on gfx950: gather_batch (elementwise.hip) with a per-sample
// geometric transform and an optional per-channel affine riding on the same pass.
//
//   x_all  fp32 [Nall][D][H][W][Cin]      y_all fp32 [Nall][D][H][W][K]       (H == W)
//   idx    int64 [B]   code int32 [B]     affine fp32 [B][Cin][2] = {scale, shift} or null
//   xb     TT [B][D][H][W][Cpad] (pad channels zero)      tb TT [B][D][H][W][K]
//   TT: the build's 16-bit type, or float for the fp32 executor
//
// code bits: 0 FW (flip W), 1 FH (flip H), 2 T (swap H and W), 3 FD (flip D, 3D only).
// Output pixel (d, h, w) of sample b reads source pixel (d', h', w') of sample idx[b]:
//   d' = FD ? D-1-d : d;   (a, b) = T ? (w, h) : (h, w);   h' = FH ? H-1-a : a;   w' = FW ? W-1-b : b
// and x' = fma(scale[c], x, shift[c]) in fp32 before the rounding to TT (image only).
//
// Tiled kernel (Cpad 4 and 8): a workgroup of 256 lanes owns 1024 pixels of one (sample,
// slice); the code is per sample, so every branch on it is workgroup-uniform.  The pixels
// are loaded in whole contiguous row segments (16 bytes per pixel at Cin = 4): FW only
// reverses the lane order inside a segment, FH / FD only pick another row / slice.  All of
// a lane's loads are issued before the first use; a pixel is converted (and the affine,
// read once per workgroup, applied) in registers.
//  * Without T the 1024 pixels are a strip of row segments 32, 64 or 128 pixels wide --
//    whole rows up to W = 128, so the workgroup reads and writes one contiguous run, as
//    gather_batch does -- and a lane stores the pixels it loaded.  (32 x 32 tiles of a
//    128 x 128 image, 512-byte read and 256-byte write segments a row apart, cost 4-7 % of the
//    pass on an MI355X; at 32 x 32 images, where a tile is the image, nothing:
//    profiles/r9_augment.md.)
//  * With T the pixels are a 32 x 32 tile, lane (r, c) = (tid >> 5, tid & 31) loads source
//    pixels (a0 + r + 8 i, b0 + c), i < 4; the tile goes through LDS, written [a][b] row by
//    row and read back [b][a], so the global stores are whole 32-pixel row segments too.
// LDS pitches (tools/lds_bank_model.py, tests/test_lds_gather_aug.py): a pixel is NW dwords
// (2, 4, 8); rows of 32 NW + 2 dwords for NW = 2 (the 8-byte transposed reads of a 32-lane
// half land on 32 distinct bank pairs) and 32 NW + 4 for NW = 4, 8 (the 16-byte reads of a
// lane group land on 16 distinct 16-byte slots; the row writes of NW = 8, fp32 with 8
// channels, are 2-way); the K target values are kept as fp32 planes [k][a][33].
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

// grid: B * D * ntile workgroups (ntile: the larger of the two tilings' counts per slice; a
// workgroup past its sample's count leaves at once); dynamic LDS: K * GA_TILE * GA_TP floats.
// strip_log2: log2 of the strip width of the codes without T (5, 6 or 7)
template <int CPAD, typename TT>
__global__ void __launch_bounds__(GA_THREADS) gather_aug_tile_kernel(
    const float* __restrict__ x_all, const float* __restrict__ y_all, const long long* __restrict__ idx,
    const int* __restrict__ code, const float* __restrict__ affine, int D, int H, int tiles, int ntile, int strip_log2,
    int Cin, int K, TT* __restrict__ xb, TT* __restrict__ tb) {
  constexpr int NW = GaLayout<CPAD, TT>::NW, PITCH = GaLayout<CPAD, TT>::PITCH;
  __shared__ __attribute__((aligned(16))) uint32_t xs[GA_TILE * PITCH];
  extern __shared__ float ts[];
  const int W = H;
  int bid = blockIdx.x;
  const int t = bid % ntile;
  bid /= ntile;
  const int d = bid % D, n = bid / D;
  const int cd = code[n] & (D > 1 ? 15 : 7);
  const bool fw = cd & 1, fh = cd & 2, tr = cd & 4, fd = cd & 8;
  // the workgroup's 1024 output pixels: a 32 x 32 tile with T, else a strip of whole row
  // segments 2^strip_log2 wide (whole rows up to W = 128: one contiguous run in and out)
  const int shift = tr ? 5 : strip_log2;
  const int across = tr ? tiles : (W + (1 << shift) - 1) >> shift;
  const int ti = t / across, tj = t - ti * across;
  const int oh0 = ti * ((GA_TILE * GA_TILE) >> shift), ow0 = tj << shift;
  if (oh0 >= H) return;
  const int a0 = tr ? ow0 : oh0, b0 = tr ? oh0 : ow0;     // source tile origin before the flips
  const size_t sbase = ((size_t)idx[n] * D + (fd ? D - 1 - d : d)) * H * W;
  const size_t obase = ((size_t)n * D + d) * H * W;
  const float* af = affine ? affine + (size_t)n * Cin * 2 : nullptr;
  const int r = threadIdx.x >> shift, c = threadIdx.x & ((1 << shift) - 1), rows = GA_THREADS >> shift;

  // the sample's affine, once per workgroup (scalar loads)
  float sc[CPAD], sf[CPAD];
#pragma unroll
  for (int ch = 0; ch < CPAD; ++ch) {
    sc[ch] = (af && ch < Cin) ? af[2 * ch] : 1.f;
    sf[ch] = (af && ch < Cin) ? af[2 * ch + 1] : 0.f;
  }
  // every load of the lane's pixels is issued before the first use: no branch around them (a
  // pixel past the image edge re-reads the edge pixel and is never stored)
  float v[GA_PX][CPAD], tv[GA_PX][4];
#pragma unroll
  for (int i = 0; i < GA_PX; ++i) {
    const int a = min(a0 + r + rows * i, H - 1), b = min(b0 + c, W - 1);
    const size_t s = sbase + (size_t)(fh ? H - 1 - a : a) * W + (fw ? W - 1 - b : b);
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
    // (a, b) is the output pixel
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
  // transpose through LDS (shift == 5: r < 8, c < 32, rows == GA_ROWS): rows in, columns out; pixels
  // past the image edge are never read back
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
__global__ void __launch_bounds__(GA_THREADS) gather_aug_pixel_kernel(
    const float* __restrict__ x_all, const float* __restrict__ y_all, const long long* __restrict__ idx,
    const int* __restrict__ code, const float* __restrict__ affine, int B, int D, int H, int Cin, int Cpad, int K,
    TT* __restrict__ xb, TT* __restrict__ tb) {
  const int W = H;
  const int total = B * D * H * W;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
    const int ow = i % W;
    int t = i / W;
    const int oh = t % H;
    t /= H;
    const int d = t % D, n = t / D;
    const int cd = code[n] & (D > 1 ? 15 : 7);
    const int a = (cd & 4) ? ow : oh, b = (cd & 4) ? oh : ow;
    const size_t s = (((size_t)idx[n] * D + ((cd & 8) ? D - 1 - d : d)) * H + ((cd & 2) ? H - 1 - a : a)) * W +
                     ((cd & 1) ? W - 1 - b : b);
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

// null when (B, D, H, W, Cin, Cpad, K) is a shape the launch accepts, else the reason
const char* gather_aug_check(long long B, long long D, long long H, long long W, long long Cin, long long Cpad,
                             long long K);

template <typename TT>
hipError_t gather_batch_aug_launch_t(const float* x_all, const float* y_all, const long long* idx, const int* code,
                                     const float* affine, int B, int D, int H, int W, int Cin, int Cpad, int K, TT* xb,
                                     TT* tb, hipStream_t s) {
  if (gather_aug_check(B, D, H, W, Cin, Cpad, K) || !x_all || !y_all || !idx || !code || !xb || !tb)
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
    UNET_LAUNCH((gather_aug_tile_kernel<4, TT>), dim3(grid), dim3(GA_THREADS), shm, s, x_all, y_all, idx, code, affine,
                D, H, tiles, ntile, strip_log2, Cin, K, xb, tb);
  } else if (Cpad == 8) {
    UNET_LAUNCH((gather_aug_tile_kernel<8, TT>), dim3(grid), dim3(GA_THREADS), shm, s, x_all, y_all, idx, code, affine,
                D, H, tiles, ntile, strip_log2, Cin, K, xb, tb);
  } else {
    const long long total = (long long)B * D * H * W;
    const int blocks = (int)((total + GA_THREADS - 1) / GA_THREADS < 65536 ? (total + GA_THREADS - 1) / GA_THREADS
                                                                           : 65536);
    UNET_LAUNCH((gather_aug_pixel_kernel<TT>), dim3(blocks), dim3(GA_THREADS), 0, s, x_all, y_all, idx, code, affine, B,
                D, H, Cin, Cpad, K, xb, tb);
  }
  return launch_status();
}

}  // namespace unet
