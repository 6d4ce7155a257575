// Resampling batch gathers on gfx950: gather_batch_crop (gather.h) with a per-sample 2 x 2 matrix
// in the (H, W) plane -- rotation by any angle and isotropic zoom: gather_batch_warp -- and, on
// top of it, a smooth per-pixel displacement of the source coordinates, a quadratic B-spline
// through a per-sample lattice of control-node displacements: gather_batch_elastic.  One pass;
// the image is interpolated bilinearly, the target is read at the nearest voxel.  The launcher
// of all five gathers, gather_launch_t, is at the end of this file.
//
//   x_all, y_all, idx, origin, code, affine, xb, tb: as in gather.h
//   mat    int32 [B][4] = (a00, a01, a10, a11), Q16; elastic: or null (= the identity)
//   field  int32 [B][N][N][2] = node (i, j)'s displacement along (h, w) in 2^-17 pixel,
//          N = ((H - 1) >> s) + 3, cells of S = 1 << s patch pixels, 3 <= s <= 6  (elastic only)
//
// The geometry is integer, so the ops equal their torch definitions (data/augment.py warp_torch,
// elastic_torch) bit for bit.  Output voxel (d, h, w) of sample b maps through gather.h's code
// mapping to patch coordinates (d', h', w'); the slice is origin.d + d' (depth is not
// interpolated) and Q is defined at the patch coordinates themselves (the displacement is
// indexed by them; for the warp alone the flips only negate u or v and T swaps them, so its tile
// kernel folds the code into the matrix instead, gw_fold: the same integers):
//   u = 2 h' - (H - 1),  v = 2 w' - (W - 1)
//   Qh = (origin.h << 17) + (H - 1) 65536 + a00 u + a01 v + d_0      (2^-17 pixel of the stored image)
//   Qw = (origin.w << 17) + (W - 1) 65536 + a10 u + a11 v + d_1
//   ci = h' >> s, t = h' & (S - 1),  wh = [(S - t)^2, -2 t^2 + 2 S t + S^2, t^2]   (sum 2 S^2)
//   d_c = (sum_a wh[a] sum_b ww[b] f[ci + a][cj + b][c]) >> (2 + 4 s)   (ww, cj from w'; warp: d = 0)
// with the origin clamped as gather.h clamps it, every matrix entry clamped into [-2^18, 2^18] and
// every field entry into [-2^22, 2^22] (32 pixels): all are device data the launch cannot
// validate.  |u|, |v| < 2^16 and a stored side is below 2^20 (gather_check), so |Q| < 2^38 before
// the displacement: Qh and Qw are 64-bit, the pixel indices Q >> 17 fit an int.  A weight product
// wh[a] ww[b] is at most 9/4 S^4 < 2^26 and fits an int; times an entry it is one 32 x 32 ->
// 64-bit multiply-add, nine per component; the sum stays below 4 S^4 2^22 = 2^48 and the shift is
// arithmetic (floor).  Every depth slice of a sample uses the same field.
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
// before the first use; code, origin, matrix and affine are workgroup-uniform.  At Cin == Cpad a
// tap is 16-byte loads (a pixel is 16 bytes at Cin = 4: every tap address is aligned).  There is
// no transposing path; the warp uses no LDS and no barrier.
// Elastic: a tile's patch coordinates span at most 32 pixels per axis, that is at most 32 / S + 1
// cells and 32 / S + 3 <= 7 nodes: the workgroup stages those nodes of its sample once in LDS,
// clamped, as (d_h, d_w) pairs, and a pixel reads its 3 x 3 of them as nine 8-byte LDS loads.  A
// lane's column is the same in all four passes, so its three weights along that axis are formed
// once.
//
// Any other Cpad <= 64: one lane per output pixel, the nine nodes read from global memory.
// Plain vector loads and stores only: no atomics, two runs give the same bits.
//
// gather_batch_warp3 (WARP3 on the same two kernels): the matrix is 3 x 3 over (d, h, w), mat int32
// [B][9] row-major and required, and depth is rotated, zoomed and interpolated too (data/augment.py
// warp3_torch, bit for bit).  At patch coordinates (d', h', w'), d' = FD ? D-1-d : d:
//   t = 2 d' - (D - 1)
//   Qd = (origin.d << 17) + (D - 1) 65536 + m00 t + m01 u + m02 v,  Qh, Qw alike from rows 1 and 2
// D < 2^16 (gather_check), so |t| < 2^16 and |Q| < 2^38 as above.  id = Qd >> 17, fd = Qd & 0x1FFFF;
// s0 and s1 are the bilinear value above in the slices id and id + 1 (a tap whose slice is
// outside the stored volume is 0.0f too, its address clamped) and the voxel is
//   s0 wd0 + s1 wd1,  wd1 = fd 2^-17,  wd0 = (131072 - fd) 2^-17
// two products and one sum, each rounded once.  Target: y at ((Qd + 65536) >> 17, nh, nw), 0.0f
// outside.  field may be null (no displacement: the ELASTIC = false instantiation); with one the
// displacement above is added to Qh and Qw, the same in every slice.  A lane issues 8 taps and 1
// target voxel per output voxel, all before the first use.
// Tiled kernel: a wave is 8 x 4 voxels in each of 2 adjacent output slices and a lane owns 2 voxels
// at Cpad 4 (104 VGPRs, 4 waves / SIMD) and 1 at Cpad 8 (92 VGPRs, 5 waves), no scratch; a
// workgroup is 32 x 4 x 2 voxels per pass.  Once the plane tilts, a 16 x 4 tile in one slice walks
// across 16 sin(theta) source slices, each a line Hs Ws Cin 4 bytes away.  Measured at b8, 128^3 x 4
// of 155 x 240 x 240 x 4, bf16, us per launch for the identity / drawn matrices at the defaults / 30
// degrees about d, h, w / drawn with mixed codes (profiles/r21_rotate3d.md):
//   16 x 4 x 1, 2 passes:  173 / 268 / 205, 391, 181 / 308        (102 VGPRs)
//    8 x 4 x 2, 2 passes:  174 / 252 / 225, 276, 178 / 290        (kept)
//    4 x 4 x 4, 2 passes:  204 / 287 / 274, 276, 203 / 304        (104 VGPRs)
//   16 x 4 x 1, 4 passes:  244 / 281 / 258, 344, 244 / 306        (202 VGPRs, 2 waves / SIMD)
//   16 x 4 x 1, 1 pass:    160 / 285 / 226, 380, 164 / 310        (54 VGPRs, 8 waves / SIMD)
//    4 x 4 x 4, 1 pass:    239 / 298 / 283, 278, 231 / 319
// against 152 us of the in-plane warp with drawn matrices and mixed codes.  The Cpad 8 pass count
// with 2 passes (168 VGPRs, 3 waves) was compiled but not timed; 8 x 4 x 2 with 1 pass was not tried.
#pragma once
#include "gather.h"

namespace unet {
namespace {

// the wave tile of 64 output voxels: 16 x 4 in one slice (TDL = 0), 8 x 4 in each of 2 slices
// (TDL = 1) or 4 x 4 in each of 4 (TDL = 2); always 4 along H.  A workgroup of 4 waves puts them
// side by side up to 32 voxels along W and stacks the rest along H: PH rows per pass
template <int TDL>
struct GwGeo {
  static constexpr int TW_LOG2 = 4 - TDL, TW = 1 << TW_LOG2, TH = 4, TD = 1 << TDL;
  static constexpr int ACROSS = 32 / TW < GA_THREADS / 64 ? 32 / TW : GA_THREADS / 64;
  static constexpr int WGW = ACROSS * TW;
  static constexpr int PH = TH * (GA_THREADS / 64 / ACROSS);
};
constexpr int GW_PX = 4;                          // passes = pixels per lane (warp, elastic)
// ... of the 3D warp (8 taps per voxel: 2 passes at Cpad 4, 1 at Cpad 8) and its wave tile, 8 x 4 in
// each of 2 slices (GwGeo)
constexpr int GW3_TDL = 1;
template <int CPAD>
struct Gw3Px {
  static constexpr int value = CPAD == 4 ? 2 : 1;
};
constexpr int GW_MAT_MAX = 1 << 18;               // clamp of a matrix entry (Q16: a zoom of 1/4)
constexpr int GE_FIELD_MAX = 1 << 22;             // clamp of a field entry (2^-17 pixel: 32 pixels)
constexpr int GE_NODES = 7;                       // nodes per axis a 32-pixel span can touch at S = 8

// the sample's clamped matrix (null: the identity) and the patch centre in 2^-17 pixel of the
// stored image; gw_source gives the source coordinates (qh, qw) of patch pixel (ph, pw)
struct GwMap {
  long long ch, cw;
  int m00, m01, m10, m11;
};
__device__ __forceinline__ GwMap gw_map(const int* __restrict__ mat, int n, const GcOrigin& og, int H, int W) {
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
// the warp's tiles fold the code into the matrix and evaluate Q at the output pixel's own (u, v):
// u' = (FH ? -1 : 1) (T ? v : u), v' = (FW ? -1 : 1) (T ? u : v), the same integers.  (Kept because
// four warp cases measured 0.1-0.6 % over the parent's spread with every pixel mapped instead; the
// two forms were not measured against each other: profiles/r20_gather_core.md)
__device__ __forceinline__ void gw_fold(GwMap& g, int cd) {
  const int sh = (cd & 2) ? -1 : 1, sw = (cd & 1) ? -1 : 1;
  const int a0 = g.m00, a1 = g.m01, a2 = g.m10, a3 = g.m11;
  if (cd & 4) {
    g.m00 = sw * a1, g.m01 = sh * a0, g.m10 = sw * a3, g.m11 = sh * a2;
  } else {
    g.m00 = sh * a0, g.m01 = sw * a1, g.m10 = sh * a2, g.m11 = sw * a3;
  }
}
__device__ __forceinline__ void gw_source(const GwMap& g, int ph, int pw, int H, int W, long long& qh, long long& qw) {
  const long long u = 2 * ph - (H - 1), v = 2 * pw - (W - 1);
  qh = g.ch + g.m00 * u + g.m01 * v, qw = g.cw + g.m10 * u + g.m11 * v;
}

// one output pixel's source at (qh, qw): clamped tap rows / columns, their validity, the
// weights, and the nearest voxel of the target
struct GwTap {
  int r0, r1, c0, c1, nr, nc;
  bool r0ok, r1ok, c0ok, c1ok, nok;
  float wh0, wh1, ww0, ww1;
};
__device__ __forceinline__ GwTap gw_tap(long long qh, long long qw, int Hs, int Ws) {
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

// products first, sums left to right, each rounded on its own (the caller's contract is off);
// a tap outside the stored image counts as 0.0f
__device__ __forceinline__ float gw_lerp(float p00, float p01, float p10, float p11, const GwTap& t) {
#pragma clang fp contract(off)
  p00 = t.r0ok && t.c0ok ? p00 : 0.f, p01 = t.r0ok && t.c1ok ? p01 : 0.f;
  p10 = t.r1ok && t.c0ok ? p10 : 0.f, p11 = t.r1ok && t.c1ok ? p11 : 0.f;
  const float a = p00 * t.ww0, b = p01 * t.ww1, c = p10 * t.ww0, d = p11 * t.ww1;
  const float r0 = a + b, r1 = c + d;
  const float e = r0 * t.wh0, f = r1 * t.wh1;
  return e + f;
}

// warp3: the sample's clamped 3 x 3 matrix over (d, h, w) and the patch centre in 2^-17 voxel of
// the stored volume; gw3_source gives the source coordinates of patch voxel (pd, ph, pw)
struct Gw3Map {
  long long cd, ch, cw;
  int m[9];
};
__device__ __forceinline__ Gw3Map gw3_map(const int* __restrict__ mat, int n, const GcOrigin& og, int D, int H,
                                          int W) {
  Gw3Map g;
#pragma unroll
  for (int e = 0; e < 9; ++e) g.m[e] = min(max(mat[9 * (size_t)n + e], -GW_MAT_MAX), GW_MAT_MAX);
  g.cd = ((long long)og.d << 17) + (long long)(D - 1) * 65536;
  g.ch = ((long long)og.h << 17) + (long long)(H - 1) * 65536;
  g.cw = ((long long)og.w << 17) + (long long)(W - 1) * 65536;
  return g;
}
__device__ __forceinline__ void gw3_source(const Gw3Map& g, int pd, int ph, int pw, int D, int H, int W,
                                           long long& qd, long long& qh, long long& qw) {
  const long long t = 2 * pd - (D - 1), u = 2 * ph - (H - 1), v = 2 * pw - (W - 1);
  qd = g.cd + g.m[0] * t + g.m[1] * u + g.m[2] * v;
  qh = g.ch + g.m[3] * t + g.m[4] * u + g.m[5] * v;
  qw = g.cw + g.m[6] * t + g.m[7] * u + g.m[8] * v;
}

// warp3: the two clamped slices of a voxel at depth qd, their validity and weights, and the
// nearest slice of the target
struct GwDepth {
  int s0, s1, ns;
  bool s0ok, s1ok, nok;
  float wd0, wd1;
};
__device__ __forceinline__ GwDepth gw_depth(long long qd, int Ds) {
  const int id = (int)(qd >> 17), fd = (int)(qd & 0x1FFFF), nd = (int)((qd + 65536) >> 17);
  GwDepth z;
  z.s0ok = id >= 0 && id < Ds, z.s1ok = id + 1 >= 0 && id + 1 < Ds, z.nok = nd >= 0 && nd < Ds;
  z.s0 = min(max(id, 0), Ds - 1), z.s1 = min(max(id + 1, 0), Ds - 1), z.ns = min(max(nd, 0), Ds - 1);
  z.wd1 = (float)fd * 0x1p-17f, z.wd0 = (float)(131072 - fd) * 0x1p-17f;
  return z;
}
// s0 wd0 + s1 wd1 of the two slices' bilinear values: two products and one sum, each rounded once
__device__ __forceinline__ float gw_lerp_depth(float s0, float s1, const GwDepth& z) {
#pragma clang fp contract(off)
  const float e = s0 * z.wd0, f = s1 * z.wd1;
  return e + f;
}

// the integer quadratic B-spline weights of offset t inside a cell of S = 1 << s pixels
__device__ __forceinline__ void ge_weights(int t, int s, int w[3]) {
  const int S = 1 << s;
  w[0] = (S - t) * (S - t), w[1] = -2 * t * t + 2 * S * t + S * S, w[2] = t * t;
}

// the elastic tile's staged nodes: GE_NODES x GE_NODES (d_h, d_w) pairs.  Only the ELASTIC kernels
// call this, so the warp has no LDS
__device__ __forceinline__ int* ge_node_lds() {
  __shared__ __attribute__((aligned(8))) int fs[GE_NODES * GE_NODES * 2];
  return fs;
}

// grid: B * ceil(D / TD) * th * tw workgroups of a WGW x (PH PX) pixel tile in each of TD slices
// (GwGeo<TDL>; warp and elastic: one slice, 32 x 32); field and s are read with ELASTIC only.
// WARP3: mat is [B][9] and not null, depth is interpolated, and ELASTIC says a field was given
template <int CPAD, typename TT, bool ELASTIC, bool WARP3 = false, int PX = GW_PX, int TDL = 0>
__global__ void __launch_bounds__(GA_THREADS) gather_resample_tile_kernel(
    const float* __restrict__ x_all, const float* __restrict__ y_all, const long long* __restrict__ idx,
    const int* __restrict__ origin, const int* __restrict__ code, const int* __restrict__ mat,
    const float* __restrict__ affine, const int* __restrict__ field, int Ds, int Hs, int Ws, int D, int H, int th,
    int tw, int Cin, int K, int s, TT* __restrict__ xb, TT* __restrict__ tb) {
#pragma clang fp contract(off)
  using G = GwGeo<TDL>;
  constexpr int NW = GaLayout<CPAD, TT>::NW, TILE_H = G::PH * PX, TAPS = WARP3 ? 8 : 4;
  static_assert(WARP3 || TDL == 0, "only the 3D warp spreads a wave over slices");
  static_assert(TILE_H <= 32 && G::WGW <= 32, "the staged nodes cover a span of 32 pixels per axis");
  const int W = H;
  int bid = blockIdx.x;
  const int tj = bid % tw;
  bid /= tw;
  const int ti = bid % th;
  bid /= th;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int nsl = (D + G::TD - 1) >> TDL;            // groups of TD output slices
  const int n = bid / nsl;
  const int d = ((bid % nsl) << TDL) + (lane >> (G::TW_LOG2 + 2));     // TDL = 0: the workgroup's slice
  const int cd = ga_code(code, n, D);
  const bool fw = cd & 1, fh = cd & 2, tr = cd & 4;
  const GcOrigin og = gc_origin(origin, n, Ds, Hs, Ws, D, H, W);
  GwMap g = {};
  Gw3Map g3 = {};
  size_t sbase = 0;
  if constexpr (WARP3) {
    g3 = gw3_map(mat, n, og, D, H, W);
    sbase = (size_t)idx[n] * Ds;                     // the sample's slice 0, in slices
  } else {
    g = gw_map(mat, n, og, H, W);
    if constexpr (!ELASTIC) gw_fold(g, cd);
    sbase = ga_slice(idx, n, d, cd, og, Ds, Hs, Ws, D);
  }
  // WARP3: the lane's patch slice d' (a slice past the patch maps like the last and is never stored)
  const int dc = min(d, D - 1), pd = (cd & 8) ? D - 1 - dc : dc;
  const size_t obase = ((size_t)n * D + d) * H * W;
  const int ow = tj * G::WGW + (wave % G::ACROSS) * G::TW + (lane & (G::TW - 1));
  const int oh0 = ti * TILE_H + (wave / G::ACROSS) * G::TH + ((lane >> G::TW_LOG2) & (G::TH - 1));

  float sc[CPAD], sf[CPAD];
  const bool af = ga_affine<CPAD>(affine, n, Cin, sc, sf);
  // the lane's column, the same in every pass; ELASTIC: its patch coordinate, a w' without T, an
  // h' with it
  const int owc = min(ow, W - 1);
  const int pcol = tr ? (fh ? H - 1 - owc : owc) : (fw ? W - 1 - owc : owc);

  // ELASTIC: the staged nodes, the column's weights, the LDS strides of the node pairs along the
  // row's and the column's axis, and the column's base
  int* fs = nullptr;
  int wcol[3], ci0 = 0, cj0 = 0, srow = 0, scol = 0, bcol = 0;
  if constexpr (ELASTIC) {
    fs = ge_node_lds();
    // the tile's span of patch coordinates: output rows [ti 32, ...] and columns [tj 32, ...] clipped
    // to the patch, swapped by T and mirrored by the flips; its first cell per axis
    const int olo_h = ti * TILE_H, ohi_h = min(olo_h + TILE_H, H) - 1;
    const int olo_w = tj * G::WGW, ohi_w = min(olo_w + G::WGW, W) - 1;
    const int alo = tr ? olo_w : olo_h, ahi = tr ? ohi_w : ohi_h;     // h' before the flip
    const int blo = tr ? olo_h : olo_w, bhi = tr ? ohi_h : ohi_w;     // w' before the flip
    ci0 = (fh ? H - 1 - ahi : alo) >> s, cj0 = (fw ? W - 1 - bhi : blo) >> s;
    const int N = ((H - 1) >> s) + 3;
    // stage nodes (ci0 + r, cj0 + c), r, c < 7: the load is unconditional at a clamped address
    const int e = min((int)threadIdx.x, GE_NODES * GE_NODES * 2 - 1);
    const int r = e / (2 * GE_NODES), c = (e >> 1) % GE_NODES;
    const size_t at = (((size_t)n * N + min(ci0 + r, N - 1)) * N + min(cj0 + c, N - 1)) * 2 + (e & 1);
    const int f = min(max(field[at], -GE_FIELD_MAX), GE_FIELD_MAX);
    if (threadIdx.x < GE_NODES * GE_NODES * 2) fs[e] = f;
    ge_weights(pcol & ((1 << s) - 1), s, wcol);
    srow = tr ? 2 : 2 * GE_NODES, scol = tr ? 2 * GE_NODES : 2;
    bcol = ((pcol >> s) - (tr ? ci0 : cj0)) * scol;
    __syncthreads();
  }

  // every load of the lane's pixels is issued before the first use: no branch around them (a
  // pixel past the patch edge maps like the edge pixel and is never stored; every address is
  // clamped into the slice)
  GwTap t[PX];
  GwDepth z[PX];
  float p[PX][TAPS][CPAD], tv[PX][4];
#pragma unroll
  for (int i = 0; i < PX; ++i) {
    const int ohc = min(oh0 + G::PH * i, H - 1);
    long long qd = 0, qh, qw;
    const int prow = tr ? (fw ? W - 1 - ohc : ohc) : (fh ? H - 1 - ohc : ohc);
    if constexpr (WARP3) {
      gw3_source(g3, pd, tr ? pcol : prow, tr ? prow : pcol, D, H, W, qd, qh, qw);
    } else if constexpr (!ELASTIC) {
      gw_source(g, ohc, owc, H, W, qh, qw);       // (the code is in the matrix)
    } else {
      gw_source(g, tr ? pcol : prow, tr ? prow : pcol, H, W, qh, qw);
    }
    if constexpr (ELASTIC) {
      int wrow[3];
      ge_weights(prow & ((1 << s) - 1), s, wrow);
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
      qh += dh >> (2 + 4 * s), qw += dw >> (2 + 4 * s);
    }
    t[i] = gw_tap(qh, qw, Hs, Ws);
    // the offsets of the four taps and of the nearest voxel inside a slice
    const size_t so[4] = {(size_t)t[i].r0 * Ws + t[i].c0, (size_t)t[i].r0 * Ws + t[i].c1,
                          (size_t)t[i].r1 * Ws + t[i].c0, (size_t)t[i].r1 * Ws + t[i].c1};
    size_t sn = (size_t)t[i].nr * Ws + t[i].nc;
    if constexpr (WARP3) {
      z[i] = gw_depth(qd, Ds);
      const size_t b0 = (sbase + z[i].s0) * Hs * Ws, b1 = (sbase + z[i].s1) * Hs * Ws;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        ga_load<CPAD>(x_all + (b0 + so[j]) * Cin, Cin, p[i][j]);
        ga_load<CPAD>(x_all + (b1 + so[j]) * Cin, Cin, p[i][TAPS - 4 + j]);
      }
      sn += (sbase + z[i].ns) * Hs * Ws;
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) ga_load<CPAD>(x_all + (sbase + so[j]) * Cin, Cin, p[i][j]);
      sn += sbase;
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) tv[i][k] = k < K ? y_all[sn * K + k] : 0.f;
  }
  __builtin_amdgcn_sched_barrier(0);
#pragma unroll
  for (int i = 0; i < PX; ++i) {
    float v[CPAD];
    bool nok = t[i].nok;
    if constexpr (WARP3) {
      // a tap of a slice outside the stored volume counts as 0.0f, like one of a row or column outside
#pragma unroll
      for (int ch = 0; ch < CPAD; ++ch) {
        float q[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) q[j] = (j < 4 ? z[i].s0ok : z[i].s1ok) ? p[i][j % TAPS][ch] : 0.f;
        v[ch] = gw_lerp_depth(gw_lerp(q[0], q[1], q[2], q[3], t[i]), gw_lerp(q[4], q[5], q[6], q[7], t[i]), z[i]);
      }
      nok = nok && z[i].nok;
    } else {
#pragma unroll
      for (int ch = 0; ch < CPAD; ++ch) v[ch] = gw_lerp(p[i][0][ch], p[i][1][ch], p[i][2][ch], p[i][3][ch], t[i]);
    }
    uint32_t w[NW];
    ga_convert<CPAD, TT>(v, af, sc, sf, Cin, w);
#pragma unroll
    for (int k = 0; k < 4; ++k) tv[i][k] = nok ? tv[i][k] : 0.f;
    const int oh = oh0 + G::PH * i;
    if (oh < H && ow < W && (!WARP3 || d < D))
      ga_store<CPAD>(xb, tb, obase + (size_t)oh * W + ow, w, tv[i], K);
  }
}

// any Cpad <= 64: one lane per output pixel, B D H W < 2^31
template <typename TT, bool ELASTIC, bool WARP3 = false>
__global__ void __launch_bounds__(GA_THREADS) gather_resample_pixel_kernel(
    const float* __restrict__ x_all, const float* __restrict__ y_all, const long long* __restrict__ idx,
    const int* __restrict__ origin, const int* __restrict__ code, const int* __restrict__ mat,
    const float* __restrict__ affine, const int* __restrict__ field, int B, int Ds, int Hs, int Ws, int D, int H,
    int Cin, int Cpad, int K, int s, TT* __restrict__ xb, TT* __restrict__ tb) {
#pragma clang fp contract(off)
  const int W = H;
  const int total = B * D * H * W;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
    const GaPixel px = ga_pixel(i, code, D, H, W);
    const GcOrigin og = gc_origin(origin, px.n, Ds, Hs, Ws, D, H, W);
    long long qd = 0, qh, qw;
    if constexpr (WARP3) {
      const Gw3Map g3 = gw3_map(mat, px.n, og, D, H, W);
      gw3_source(g3, (px.cd & 8) ? D - 1 - px.d : px.d, px.h, px.w, D, H, W, qd, qh, qw);
    } else {
      const GwMap g = gw_map(mat, px.n, og, H, W);
      gw_source(g, px.h, px.w, H, W, qh, qw);
    }
    if constexpr (ELASTIC) {
      const int N = ((H - 1) >> s) + 3, cmask = (1 << s) - 1;
      int wh[3], ww[3];
      ge_weights(px.h & cmask, s, wh);
      ge_weights(px.w & cmask, s, ww);
      const int* nd = field + (((size_t)px.n * N + (px.h >> s)) * N + (px.w >> s)) * 2;
      long long dh = 0, dw = 0;
      for (int e = 0; e < 3; ++e)
        for (int f = 0; f < 3; ++f) {
          const int w2 = wh[e] * ww[f];
          dh += (long long)w2 * min(max(nd[((size_t)e * N + f) * 2], -GE_FIELD_MAX), GE_FIELD_MAX);
          dw += (long long)w2 * min(max(nd[((size_t)e * N + f) * 2 + 1], -GE_FIELD_MAX), GE_FIELD_MAX);
        }
      qh += dh >> (2 + 4 * s), qw += dw >> (2 + 4 * s);
    }
    const GwTap t = gw_tap(qh, qw, Hs, Ws);
    if constexpr (WARP3) {
      const GwDepth z = gw_depth(qd, Ds);
      const size_t v0 = (size_t)idx[px.n] * Ds;
      const size_t so[4] = {(size_t)t.r0 * Ws + t.c0, (size_t)t.r0 * Ws + t.c1, (size_t)t.r1 * Ws + t.c0,
                            (size_t)t.r1 * Ws + t.c1};
      const float* a = x_all + (v0 + z.s0) * Hs * Ws * Cin;
      const float* b = x_all + (v0 + z.s1) * Hs * Ws * Cin;
      const float* af = affine ? affine + (size_t)px.n * Cin * 2 : nullptr;
      TT* dst = xb + (size_t)i * Cpad;
      for (int ch = 0; ch < Cpad; ++ch) {
        float v = 0.f;
        if (ch < Cin) {
          float q[8];
          for (int j = 0; j < 4; ++j) {
            const float qa = a[so[j] * Cin + ch], qb = b[so[j] * Cin + ch];
            q[j] = z.s0ok ? qa : 0.f, q[4 + j] = z.s1ok ? qb : 0.f;
          }
          v = ga_affine1(af, ch, gw_lerp_depth(gw_lerp(q[0], q[1], q[2], q[3], t),
                                               gw_lerp(q[4], q[5], q[6], q[7], t), z));
        }
        dst[ch] = (TT)v;
      }
      const size_t sn = ((v0 + z.ns) * Hs + t.nr) * Ws + t.nc;
      for (int k = 0; k < K; ++k) tb[(size_t)i * K + k] = (TT)(t.nok && z.nok ? y_all[sn * K + k] : 0.f);
      continue;
    }
    const size_t sbase = ga_slice(idx, px.n, px.d, px.cd, og, Ds, Hs, Ws, D);
    const float* s00 = x_all + (sbase + (size_t)t.r0 * Ws + t.c0) * Cin;
    const float* s01 = x_all + (sbase + (size_t)t.r0 * Ws + t.c1) * Cin;
    const float* s10 = x_all + (sbase + (size_t)t.r1 * Ws + t.c0) * Cin;
    const float* s11 = x_all + (sbase + (size_t)t.r1 * Ws + t.c1) * Cin;
    const float* af = affine ? affine + (size_t)px.n * Cin * 2 : nullptr;
    TT* dst = xb + (size_t)i * Cpad;
    for (int ch = 0; ch < Cpad; ++ch)
      dst[ch] = (TT)(ch < Cin ? ga_affine1(af, ch, gw_lerp(s00[ch], s01[ch], s10[ch], s11[ch], t)) : 0.f);
    const size_t sn = sbase + (size_t)t.nr * Ws + t.nc;
    for (int k = 0; k < K; ++k) tb[(size_t)i * K + k] = (TT)(t.nok ? y_all[sn * K + k] : 0.f);
  }
}

}  // namespace

// null when op accepts the shape of a (gather.hip), else the reason
const char* gather_check(GatherOp op, const GatherArgs& a);

// the launcher of the five gathers; aug: stored = patch, no origin
template <typename TT>
hipError_t gather_launch_t(GatherOp op, GatherArgs a, TT* xb, TT* tb, hipStream_t st) {
  if (gather_check(op, a) || !a.x_all || !a.y_all || !a.idx || !gather_required(op, a) || !xb || !tb)
    return hipErrorInvalidValue;
  if (op == GatherOp::aug) a.Ds = a.D, a.Hs = a.H, a.Ws = a.W, a.origin = nullptr;
  const int B = a.B, Ds = a.Ds, Hs = a.Hs, Ws = a.Ws, D = a.D, H = a.H, W = a.W, Cin = a.Cin, Cpad = a.Cpad, K = a.K;
  const int s = a.s;
  const bool tiled = Cpad == 4 || Cpad == 8;
  // the kernels of one lane per pixel: a grid-stride loop
  const long long total = (long long)B * D * H * W;
  const int blocks = (int)((total + GA_THREADS - 1) / GA_THREADS < 65536 ? (total + GA_THREADS - 1) / GA_THREADS
                                                                         : 65536);
  if (op == GatherOp::aug || op == GatherOp::crop) {
    const int tiles = (H + GA_TILE - 1) / GA_TILE;
    // strips of the codes without T: 32, 64 or 128 pixels wide, 1024 pixels each
    const int strip_log2 = W <= 32 ? 5 : (W <= 64 ? 6 : 7);
    const int strip_h = (GA_TILE * GA_TILE) >> strip_log2;
    const int nstrip = ((W + (1 << strip_log2) - 1) >> strip_log2) * ((H + strip_h - 1) / strip_h);
    const int ntile = tiles * tiles > nstrip ? tiles * tiles : nstrip;
    if ((long long)B * D * ntile >= (1LL << 31)) return hipErrorInvalidValue;
    const size_t shm = (size_t)K * GA_TILE * GA_TP * sizeof(float);
    if (tiled) {
      UNET_LAUNCH((Cpad == 4 ? (a.origin ? gather_copy_tile_kernel<4, TT, true> : gather_copy_tile_kernel<4, TT, false>)
                             : (a.origin ? gather_copy_tile_kernel<8, TT, true> : gather_copy_tile_kernel<8, TT, false>)),
                  dim3(B * D * ntile),
                  dim3(GA_THREADS), shm, st, a.x_all, a.y_all, a.idx, a.origin, a.code, a.affine, Ds, Hs, Ws, D, H,
                  tiles, ntile, strip_log2, Cin, K, xb, tb);
    } else {
      UNET_LAUNCH((gather_copy_pixel_kernel<TT>), dim3(blocks), dim3(GA_THREADS), 0, st, a.x_all, a.y_all, a.idx,
                  a.origin, a.code, a.affine, B, Ds, Hs, Ws, D, H, Cin, Cpad, K, xb, tb);
    }
    return launch_status();
  }
  if (op == GatherOp::warp3) {
    // a null field: no displacement (the ELASTIC flag of the kernels)
    const bool el = a.field != nullptr;
    if (!tiled) {
      UNET_LAUNCH((el ? gather_resample_pixel_kernel<TT, true, true> : gather_resample_pixel_kernel<TT, false, true>),
                  dim3(blocks), dim3(GA_THREADS), 0, st, a.x_all, a.y_all, a.idx, a.origin, a.code, a.mat, a.affine,
                  a.field, B, Ds, Hs, Ws, D, H, Cin, Cpad, K, s, xb, tb);
      return launch_status();
    }
    using G = GwGeo<GW3_TDL>;
    const int px = Cpad == 4 ? Gw3Px<4>::value : Gw3Px<8>::value;
    const int th = (H + G::PH * px - 1) / (G::PH * px), tw = (W + G::WGW - 1) / G::WGW;
    const long long grid = (long long)B * ((D + G::TD - 1) / G::TD) * th * tw;
    if (grid >= (1LL << 31)) return hipErrorInvalidValue;
    UNET_LAUNCH((Cpad == 4 ? (el ? gather_resample_tile_kernel<4, TT, true, true, Gw3Px<4>::value, GW3_TDL>
                                 : gather_resample_tile_kernel<4, TT, false, true, Gw3Px<4>::value, GW3_TDL>)
                           : (el ? gather_resample_tile_kernel<8, TT, true, true, Gw3Px<8>::value, GW3_TDL>
                                 : gather_resample_tile_kernel<8, TT, false, true, Gw3Px<8>::value, GW3_TDL>)),
                dim3((unsigned)grid), dim3(GA_THREADS), 0, st, a.x_all, a.y_all, a.idx, a.origin, a.code, a.mat,
                a.affine, a.field, Ds, Hs, Ws, D, H, th, tw, Cin, K, s, xb, tb);
    return launch_status();
  }
  const bool el = op == GatherOp::elastic;
  constexpr int GW_TILE_H = GwGeo<0>::PH * GW_PX, GW_WGW = GwGeo<0>::WGW;
  const int th = (H + GW_TILE_H - 1) / GW_TILE_H, tw = (W + GW_WGW - 1) / GW_WGW;
  if ((long long)B * D * th * tw >= (1LL << 31)) return hipErrorInvalidValue;
  if (tiled) {
    UNET_LAUNCH((Cpad == 4 ? (el ? gather_resample_tile_kernel<4, TT, true> : gather_resample_tile_kernel<4, TT, false>)
                           : (el ? gather_resample_tile_kernel<8, TT, true> : gather_resample_tile_kernel<8, TT, false>)),
                dim3(B * D * th * tw), dim3(GA_THREADS), 0, st, a.x_all, a.y_all, a.idx, a.origin, a.code, a.mat,
                a.affine, a.field, Ds, Hs, Ws, D, H, th, tw, Cin, K, s, xb, tb);
  } else {
    UNET_LAUNCH((el ? gather_resample_pixel_kernel<TT, true> : gather_resample_pixel_kernel<TT, false>), dim3(blocks),
                dim3(GA_THREADS), 0, st, a.x_all, a.y_all, a.idx, a.origin, a.code, a.mat, a.affine, a.field, B, Ds,
                Hs, Ws, D, H, Cin, Cpad, K, s, xb, tb);
  }
  return launch_status();
}

}  // namespace unet
