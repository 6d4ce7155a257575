// Sliding-window inference ops (sliding.h): plan-time validation and the launchers.  fp32 in
// and out, element-type independent: the bf16 build's copy of the launchers serves every
// executor (there is no f32_ twin).
#include "sliding.h"

namespace unet {

namespace {

// tiles of an axis of length L (ops/sliding.py tile_origins)
long long sw_tiles(long long L, long long T, long long s) { return L <= T ? 1 : (L - T + s - 1) / s + 1; }

}  // namespace

// plan-time validation (bindings.cpp make_generic): nullptr when the launch is accepted
const char* sw_check(long long kind, long long N, long long D, long long H, long long W, long long C, long long Td,
                     long long Th, long long Tw, long long sd, long long sh, long long sw, long long B, long long t0,
                     long long nt) {
  const long long lim = 1LL << 31;
  if (kind == 1 && (C < 1 || C > 4)) return "sw_blend: 1..4 classes";
  if (C < 1 || C >= lim) return "sw_extract: C >= 1";
  if (N < 1 || D < 1 || H < 1 || W < 1) return "sliding window: N, D, H, W >= 1";
  if (N >= lim || D >= lim || H >= lim || W >= lim) return "sliding window: N, D, H, W < 2^31";
  if (Td < 1 || Th < 1 || Tw < 1 || Td >= lim || Th >= lim || Tw >= lim) return "sliding window: tile sides >= 1";
  if (sd < 1 || sh < 1 || sw < 1 || sd > Td || sh > Th || sw > Tw || 4 * sd < Td || 4 * sh < Th || 4 * sw < Tw)
    return "sliding window: a stride outside [T / 4, T]";
  if (B < 1 || B >= lim) return "sliding window: B >= 1";
  // (every factor is below 2^31 and each product is tested before the next factor: no overflow)
  const long long P = D * H;
  if (P >= lim || P * W >= lim) return "sliding window: D H W >= 2^31";
  const long long T = Td * Th;
  if (T >= lim || T * Tw >= lim || T * Tw * C >= lim || T * Tw * C * B >= lim)
    return "sliding window: a batch of B Td Th Tw C elements >= 2^31";
  const long long tpi = sw_tiles(D, Td, sd) * sw_tiles(H, Th, sh) * sw_tiles(W, Tw, sw);   // (<= D H W)
  if (N * tpi >= lim) return "sliding window: 2^31 tiles or more";
  if (t0 < 0 || nt < 1 || nt > B || t0 + nt > N * tpi) return "sliding window: tiles [t0, t0 + nt) outside the grid";
  if (B * Td >= lim) return "sw_extract: B Td >= 2^31";
  if (kind == 1) {
    // floats of the images the batch touches: one launch's rows x row floats
    const long long imgs = (t0 + nt - 1) / tpi - t0 / tpi + 1;
    if (imgs * P >= lim || imgs * P * W * C >= lim) return "sw_blend: the images of a batch hold 2^31 floats or more";
  }
  return nullptr;
}

const char* sw_finish_check(long long N, long long D, long long H, long long W, long long K) {
  const long long lim = 1LL << 31;
  if (K < 1 || K > 4) return "sw_finish: 1..4 classes";
  if (N < 1 || D < 1 || H < 1 || W < 1) return "sw_finish: N, D, H, W >= 1";
  if (N >= lim || D >= lim || H >= lim || W >= lim) return "sw_finish: N, D, H, W < 2^31";
  const long long P = D * H;
  if (P >= lim || P * W >= lim || P * W * K >= lim || P * W * K * N >= lim) return "sw_finish: N D H W K >= 2^31";
  return nullptr;
}

// v: the 14 integers N, D, H, W, C, Td, Th, Tw, sd, sh, sw, B, t0, nt that sw_check accepted
SwGeo sw_geo(const long long* v) {
  SwGeo g;
  g.N = (int)v[0], g.D = (int)v[1], g.H = (int)v[2], g.W = (int)v[3], g.C = (int)v[4];
  g.Td = (int)v[5], g.Th = (int)v[6], g.Tw = (int)v[7];
  g.sd = (int)v[8], g.sh = (int)v[9], g.sw = (int)v[10];
  g.nd = (int)sw_tiles(v[1], v[5], v[8]), g.nh = (int)sw_tiles(v[2], v[6], v[9]),
  g.nw = (int)sw_tiles(v[3], v[7], v[10]);
  g.B = (int)v[11], g.t0 = (int)v[12], g.nt = (int)v[13];
  return g;
}

#ifndef UNET_FP16        // (fp32 in and out: element-type independent, the bf16 build's copy serves both)
namespace {
const char* sw_geo_check(int kind, const SwGeo& g) {
  const char* m = sw_check(kind, g.N, g.D, g.H, g.W, g.C, g.Td, g.Th, g.Tw, g.sd, g.sh, g.sw, g.B, g.t0, g.nt);
  if (m) return m;
  if (g.nd != sw_tiles(g.D, g.Td, g.sd) || g.nh != sw_tiles(g.H, g.Th, g.sh) || g.nw != sw_tiles(g.W, g.Tw, g.sw))
    return "sliding window: tile counts do not match the geometry";
  return nullptr;
}
}  // namespace

hipError_t sw_extract_launch(const float* x_all, float* xb, const SwGeo& g, hipStream_t s) {
  if (sw_geo_check(0, g) || !x_all || !xb) return hipErrorInvalidValue;
  // 16-byte vectors: whole vectors per tile row and per image row, every tile's first column
  // (i sw, or the clamped W - Tw) on a vector, both bases aligned
  const bool vec = (g.Tw * (long long)g.C) % 4 == 0 && (g.W * (long long)g.C) % 4 == 0 &&
                   (g.sw * (long long)g.C) % 4 == 0 && (g.W <= g.Tw || ((g.W - g.Tw) * (long long)g.C) % 4 == 0) &&
                   !(((uintptr_t)x_all | (uintptr_t)xb) & 15);
  const int rowlen = vec ? g.Tw * g.C / 4 : g.Tw * g.C;
  int rg = SW_UNITS / rowlen;
  rg = rg < 1 ? 1 : (rg > g.Th ? g.Th : rg);
  const long long gy = (g.Th + rg - 1) / rg;
  if (gy > 65535) return hipErrorInvalidValue;
  const dim3 grid((unsigned)(g.B * g.Td), (unsigned)gy);
  if (vec)
    UNET_LAUNCH((sw_extract_kernel<4>), grid, dim3(SW_THREADS), 0, s, x_all, xb, g, rowlen, rg);
  else
    UNET_LAUNCH((sw_extract_kernel<1>), grid, dim3(SW_THREADS), 0, s, x_all, xb, g, rowlen, rg);
  return launch_status();
}

hipError_t sw_blend_launch(const float* prob, const float* w, float* acc, const SwGeo& g, hipStream_t s) {
  if (sw_geo_check(1, g) || !prob || !w || !acc) return hipErrorInvalidValue;
  const long long tpi = (long long)g.nd * g.nh * g.nw;
  const int n_lo = (int)(g.t0 / tpi), n_hi = (int)((g.t0 + g.nt - 1) / tpi);
  const long long rows = (long long)(n_hi - n_lo + 1) * g.D * g.H;
  const long long gy = ((long long)g.W * g.C + SW_UNITS - 1) / SW_UNITS;
  if (rows >= (1LL << 31) || gy > 65535) return hipErrorInvalidValue;
  const dim3 grid((unsigned)rows, (unsigned)gy);
#define SW_BLEND(KK) UNET_LAUNCH((sw_blend_kernel<KK>), grid, dim3(SW_THREADS), 0, s, prob, w, acc, g, n_lo)
  switch (g.C) {
    case 1: SW_BLEND(1); break;
    case 2: SW_BLEND(2); break;
    case 3: SW_BLEND(3); break;
    default: SW_BLEND(4);
  }
#undef SW_BLEND
  return launch_status();
}

hipError_t sw_finish_launch(float* acc, const float* wsum, int N, int D, int H, int W, int K, hipStream_t s) {
  if (sw_finish_check(N, D, H, W, K) || !acc || !wsum) return hipErrorInvalidValue;
  const unsigned P = (unsigned)(D * H * W), total = (unsigned)N * P * K;
  const dim3 grid((unsigned)((total + SW_THREADS - 1) / SW_THREADS));
#define SW_FINISH(KK) UNET_LAUNCH((sw_finish_kernel<KK>), grid, dim3(SW_THREADS), 0, s, acc, wsum, total, P)
  switch (K) {
    case 1: SW_FINISH(1); break;
    case 2: SW_FINISH(2); break;
    case 3: SW_FINISH(3); break;
    default: SW_FINISH(4);
  }
#undef SW_FINISH
  return launch_status();
}
#endif

}  // namespace unet
