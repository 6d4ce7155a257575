// Surface distances of thresholded masks on gfx950, for the 95th-percentile Hausdorff
// distance (HD95) of the evaluation report.  All integer arithmetic from the thresholds on.
//
//   prob   fp32 [N][S][K]       (the head's sigmoid outputs, channels-last), S = D H W
//   target TT   [N][S][K]       (TT: the build's 16-bit type, or float for the fp32 executor)
//   surf   int32 [N][K][4] = {mp, mt, q_lo, q_hi}
//   field  int32 [N][K][2][S]   (scratch; every element is written before it is read)
//
// P = {p >= thr}, T = {t >= 0.5}.  The surface of a mask is its voxels with a face neighbour
// (4 in 2D, 6 in 3D) outside the mask; outside the grid counts as outside the mask.
// mp = |surface P|, mt = |surface T|.  Q is the multiset of squared Euclidean voxel distances
// {d2(a, surface T) : a in surface P} + {d2(b, surface P) : b in surface T}, m = mp + mt,
// r = 95 (m - 1), lo = r / 100, hi = min(lo + 1, m - 1): q_lo and q_hi are the elements of
// rank lo and hi of Q in ascending order, or -1 when either surface is empty.  The host
// forms sqrt and the interpolation (ops/seg_metrics.py).
//
// field[n][k][side] is the exact squared distance transform to the surface of side 0 (P) or
// side 1 (T), built separably, one axis per launch, in place:
//
//   W pass  g(x)    = min_x' (x - x')^2 + (surface(x') ? 0 : INF)     (reads prob / target)
//   H pass  g(y, x) = min_y' (y - y')^2 + g(y', x)
//   D pass  g(z, .) = min_z' (z - z')^2 + g(z', .)                    (3D only)
//
// Each is the lower envelope of equal parabolas along a line, found in O(L) by one lane per
// line with the two scans of Meijster, Roerdink and Hesselink (2000), whose separator is an
// integer floor division: no float anywhere.  A workgroup (one wave) loads a tile of TL lines
// into LDS with coalesced accesses (a tile of rows is one contiguous run; a tile of columns
// is TL adjacent columns), each lane scans its line in LDS, and the tile is stored the way
// it was loaded.  A tile is private to its workgroup and fully loaded before the first
// store, so the pass runs in place.  INF = 2^28 exceeds every real value (3 * 4095^2 < 2^26)
// and INF + 2 * 4095^2 stays below 2^31, so the sentinel needs no special case.
//
// A voxel is on a side's surface exactly when that side's field is 0 there, so the selection
// reads the two fields only: one workgroup per (n, k) samples field[1] where field[0] == 0
// and the reverse, counts mp and mt, and finds rank lo by a two-level radix select (bits
// 25..13, then 12..0) with integer histograms in LDS.  q_hi is q_lo when the cumulative
// count through q_lo covers rank hi, else the smallest sampled value above q_lo (the next
// occupied low bin, or the minimum of the higher bins, taken by an integer atomicMin during
// the second scan).  Integer atomics only: the result does not depend on their order.
#pragma once
#include "common.h"

namespace unet {
namespace {

constexpr int SD_INF = 1 << 28;
constexpr int SD_MAX_AXIS = 4096;     // 3 * 4095^2 < 2^26: two 13-bit radix levels; positions fit 16 bits
constexpr int SD_LT = 64;             // lanes per workgroup of a line pass (one wave)
constexpr int SD_LDS = 65536;         // LDS bytes a line-pass workgroup may use
constexpr int SD_ST = 1024;           // lanes per workgroup of the selection
constexpr int SD_BINS = 8192;         // bins per radix level (13 bits)

__device__ __forceinline__ bool sd_in(const float* m, size_t e, float thr) { return m[e] >= thr; }
__device__ __forceinline__ bool sd_in(const h16* m, size_t e, float thr) { return h2f(m[e]) >= thr; }

// voxel (z, y, x) of the mask {m[s K] >= thr} (m: sample base + class) is on its surface
template <typename MT>
__device__ __forceinline__ bool sd_surface(const MT* m, int K, float thr, int z, int y, int x, int D, int H, int W) {
  const size_t s = ((size_t)z * H + y) * W + x;
  if (!sd_in(m, s * K, thr)) return false;
  if (x == 0 || y == 0 || x == W - 1 || y == H - 1) return true;
  if (D > 1 && (z == 0 || z == D - 1)) return true;
  const size_t sy = (size_t)W * K, sz = (size_t)H * W * K;
  bool all = sd_in(m, (s - 1) * K, thr) && sd_in(m, (s + 1) * K, thr) && sd_in(m, s * K - sy, thr) &&
             sd_in(m, s * K + sy, thr);
  if (D > 1) all = all && sd_in(m, s * K - sz, thr) && sd_in(m, s * K + sz, thr);
  return !all;
}

// rows of LDS per line: odd, so that the lanes of a wave (one line each) hit distinct banks
__host__ __device__ inline int sd_row(int L) { return L | 1; }

// lines per workgroup: the largest power of two <= 64 whose tile (line + envelope stack, 8
// bytes per element) and the 64 line bases fit SD_LDS
__host__ __device__ inline int sd_tile_lines(int L) {
  const int fit = (SD_LDS - SD_LT * 4) / (8 * sd_row(L));
  int tl = 1;
  while (tl * 2 <= fit && tl * 2 <= SD_LT) tl *= 2;
  return tl;
}

// One axis of the transform.  AXIS 0: lines along W, sourced from the masks; 1: along H;
// 2: along D (both in place on `field`).  planes = N K 2; tiles = ceil(lines / TL).
template <int AXIS, typename TT>
__global__ void __launch_bounds__(SD_LT) surf_dist_line_kernel(const float* __restrict__ prob,
                                                               const TT* __restrict__ tgt, int* __restrict__ field,
                                                               int D, int H, int W, int K, float thr, int TL,
                                                               int tiles) {
  extern __shared__ int sd_lds[];
  const int L = AXIS == 0 ? W : (AXIS == 1 ? H : D);
  const int lines = AXIS == 0 ? D * H : (AXIS == 1 ? D * W : H * W);
  const int stride = AXIS == 0 ? 1 : (AXIS == 1 ? W : H * W);
  const int LP = sd_row(L);
  const int S = D * H * W;
  int* base = sd_lds;                                   // [SD_LT] first element of each line
  int* g = sd_lds + SD_LT;                              // [TL][LP] the lines
  uint32_t* st = (uint32_t*)(g + TL * LP);              // [TL][LP] envelope stack s | t << 16, then the result
  const int tid = threadIdx.x;
  const int plane = blockIdx.x / tiles, tile = blockIdx.x - plane * tiles;
  const int l0 = tile * TL;
  const int nl = min(TL, lines - l0);
  int* fp = field + (size_t)plane * S;

  if (tid < TL) {
    const int i = l0 + tid;
    int b = 0;
    if (tid < nl) {
      if (AXIS == 0) b = i * W;
      else if (AXIS == 1) b = (i / W) * H * W + i % W;
      else b = i;
    }
    base[tid] = b;
  }
  __syncthreads();

  const int n_el = TL * L;
  const int tsh = __ffs(TL) - 1;                        // (TL is a power of two)
  if (AXIS == 0) {
    const int side = plane & 1, nk = plane >> 1;
    const int n = nk / K, k = nk - n * K;
    const size_t sample = (size_t)n * S * K + k;
    for (int idx = tid; idx < n_el; idx += SD_LT) {
      const int l = idx / L, j = idx - l * L;
      if (l >= nl) break;
      const int row = l0 + l, z = row / H, y = row - z * H;
      const bool on = side == 0 ? sd_surface(prob + sample, K, thr, z, y, j, D, H, W)
                                : sd_surface(tgt + sample, K, 0.5f, z, y, j, D, H, W);
      g[l * LP + j] = on ? 0 : SD_INF;
    }
  } else {
    for (int idx = tid; idx < n_el; idx += SD_LT) {
      const int l = idx & (TL - 1), j = idx >> tsh;
      if (l < nl) g[l * LP + j] = fp[(size_t)base[l] + (size_t)j * stride];
    }
  }
  __syncthreads();

  if (tid < nl) {
    const int* G = g + tid * LP;
    uint32_t* ST = st + tid * LP;
    // forward scan: ST[0..q] = the parabolas of the lower envelope, s their positions and t
    // the first position each one owns; t is strictly increasing, so t[q] >= q
    int q = 0;
    ST[0] = 0;
    for (int u = 1; u < L; ++u) {
      const int Gu = G[u];
      int s = 0;
      while (q >= 0) {
        const uint32_t e = ST[q];
        s = (int)(e & 0xffffu);
        const int t = (int)(e >> 16);
        if ((t - s) * (t - s) + G[s] > (t - u) * (t - u) + Gu) --q;
        else break;
      }
      if (q < 0) {
        q = 0;
        ST[0] = (uint32_t)u;
      } else {
        // the last x at which parabola s is no worse than parabola u: x = t[q] is one, so
        // the numerator is >= 0 and the division is a floor
        const uint32_t num = (uint32_t)(u * u - s * s + Gu - G[s]);
        const int w = 1 + (int)(num / (uint32_t)(2 * (u - s)));
        if (w < L) {
          ++q;
          ST[q] = (uint32_t)u | ((uint32_t)w << 16);
        }
      }
    }
    // backward scan; the result of position u overwrites ST[u]: the live entries are
    // 0..q with q <= t[q] <= u, and q == u only when t[q] == u, the entry popped here
    for (int u = L - 1; u >= 0; --u) {
      const uint32_t e = ST[q];
      const int s = (int)(e & 0xffffu), t = (int)(e >> 16);
      if (u == t) --q;
      ST[u] = (uint32_t)((u - s) * (u - s) + G[s]);
    }
  }
  __syncthreads();

  if (AXIS == 0) {
    for (int idx = tid; idx < n_el; idx += SD_LT) {
      const int l = idx / L, j = idx - l * L;
      if (l >= nl) break;
      fp[(size_t)base[l] + j] = (int)st[l * LP + j];
    }
  } else {
    for (int idx = tid; idx < n_el; idx += SD_LT) {
      const int l = idx & (TL - 1), j = idx >> tsh;
      if (l < nl) fp[(size_t)base[l] + (size_t)j * stride] = (int)st[l * LP + j];
    }
  }
}

// bin of `rank` in hist[SD_BINS] (ranks count from 0; rank < the histogram's total) and the
// count below that bin -> res[0], res[1].  Called by every lane of the workgroup.
__device__ __forceinline__ void sd_find(const int* hist, int* part, int* part2, int rank, int* res) {
  const int tid = threadIdx.x;
  constexpr int PER = SD_BINS / SD_ST;          // 8 bins per lane
  int s = 0;
#pragma unroll
  for (int i = 0; i < PER; ++i) s += hist[tid * PER + i];
  part[tid] = s;
  __syncthreads();
  if (tid < 32) {
    int s2 = 0;
    for (int i = 0; i < 32; ++i) s2 += part[tid * 32 + i];
    part2[tid] = s2;
  }
  __syncthreads();
  if (tid == 0) {
    int c = 0, a = 0;
    while (a < 31 && c + part2[a] <= rank) c += part2[a++];
    int b = a * 32;
    const int bend = b + 31;
    while (b < bend && c + part[b] <= rank) c += part[b++];
    int h = b * PER;
    const int hend = h + PER - 1;
    while (h < hend && c + hist[h] <= rank) c += hist[h++];
    res[0] = h;
    res[1] = c;
  }
  __syncthreads();
}

// field: [NK][2][S]; surf: [NK][4]
__global__ void __launch_bounds__(SD_ST) surf_dist_select_kernel(const int* __restrict__ field, int S,
                                                                 int* __restrict__ surf) {
  typedef int i32x4 __attribute__((ext_vector_type(4)));
  __shared__ int hist[SD_BINS];
  __shared__ int part[SD_ST];
  __shared__ int part2[32];
  __shared__ int sh[8];          // 0 mp, 1 mt, 2..3 sd_find result, 4 minimum above
  const int tid = threadIdx.x;
  const i32x4* f0 = (const i32x4*)(field + (size_t)blockIdx.x * 2 * S);
  const i32x4* f1 = (const i32x4*)(field + ((size_t)blockIdx.x * 2 + 1) * S);
  int* out = surf + (size_t)blockIdx.x * 4;
  const int vecs = S / 4;

  for (int i = tid; i < SD_BINS; i += SD_ST) hist[i] = 0;
  if (tid < 8) sh[tid] = tid == 4 ? 0x7fffffff : 0;
  __syncthreads();
  int mp = 0, mt = 0;
  for (int v = tid; v < vecs; v += SD_ST) {
    const i32x4 a = f0[v], b = f1[v];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      if (a[e] == 0) {                         // on the surface of P: its distance to the surface of T
        ++mp;
        atomicAdd(&hist[min(b[e] >> 13, SD_BINS - 1)], 1);
      }
      if (b[e] == 0) {
        ++mt;
        atomicAdd(&hist[min(a[e] >> 13, SD_BINS - 1)], 1);
      }
    }
  }
  if (mp) atomicAdd(&sh[0], mp);
  if (mt) atomicAdd(&sh[1], mt);
  __syncthreads();
  mp = sh[0];
  mt = sh[1];
  if (mp == 0 || mt == 0) {                    // (uniform over the workgroup)
    if (tid == 0) {
      out[0] = mp;
      out[1] = mt;
      out[2] = out[3] = -1;
    }
    return;
  }
  const long long m = (long long)mp + mt;
  const int lo = (int)(95 * (m - 1) / 100);
  const int hi = (int)min((long long)lo + 1, m - 1);
  sd_find(hist, part, part2, lo, &sh[2]);
  const int B = sh[2], below = sh[3];
  __syncthreads();
  for (int i = tid; i < SD_BINS; i += SD_ST) hist[i] = 0;
  __syncthreads();
  int above = 0x7fffffff;
  for (int v = tid; v < vecs; v += SD_ST) {
    const i32x4 a = f0[v], b = f1[v];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      if (a[e] == 0) {
        const int hb = b[e] >> 13;
        if (hb == B) atomicAdd(&hist[b[e] & (SD_BINS - 1)], 1);
        else if (hb > B) above = min(above, b[e]);
      }
      if (b[e] == 0) {
        const int hb = a[e] >> 13;
        if (hb == B) atomicAdd(&hist[a[e] & (SD_BINS - 1)], 1);
        else if (hb > B) above = min(above, a[e]);
      }
    }
  }
  if (above != 0x7fffffff) atomicMin(&sh[4], above);
  __syncthreads();
  sd_find(hist, part, part2, lo - below, &sh[2]);
  const int h = sh[2];
  const int through = below + sh[3] + hist[h];       // sampled values <= q_lo
  const int q_lo = (B << 13) | h;
  if (through > hi) {
    if (tid == 0) {
      out[0] = mp;
      out[1] = mt;
      out[2] = out[3] = q_lo;
    }
    return;
  }
  // hi = lo + 1 lies above q_lo: the next occupied low bin, else the minimum of the higher bins
  constexpr int PER = SD_BINS / SD_ST;
  int nxt = 0x7fffffff;
#pragma unroll
  for (int i = PER - 1; i >= 0; --i) {
    const int bin = tid * PER + i;
    if (bin > h && hist[bin] > 0) nxt = (B << 13) | bin;
  }
  if (nxt != 0x7fffffff) atomicMin(&sh[4], nxt);
  __syncthreads();
  if (tid == 0) {
    out[0] = mp;
    out[1] = mt;
    out[2] = q_lo;
    out[3] = sh[4];
  }
}

}  // namespace

const char* surf_dist_check(long long N, long long D, long long H, long long W, long long K);
long long surf_dist_scratch(long long N, long long D, long long H, long long W, long long K);

// field: surf_dist_scratch(N, D, H, W, K) bytes, 16-byte aligned
template <typename TT>
hipError_t surf_dist_launch_t(const float* prob, const TT* t, int N, int D, int H, int W, int K, float thr, int* field,
                              int* surf, hipStream_t s) {
  if (surf_dist_check(N, D, H, W, K) || !prob || !t || !surf || !field || ((uintptr_t)field & 15))
    return hipErrorInvalidValue;
  const long long planes = (long long)N * K * 2;
  const int axes[3] = {W, H, D};
  const int lines[3] = {D * H, D * W, H * W};
  for (int a = 0; a < 3; ++a) {
    if (a > 0 && axes[a] == 1) continue;          // (a one-voxel axis leaves the field as it is)
    const int TL = sd_tile_lines(axes[a]);
    const int tiles = (lines[a] + TL - 1) / TL;
    if (planes * tiles >= (1LL << 31)) return hipErrorInvalidValue;
    const unsigned grid = (unsigned)(planes * tiles);
    const size_t shm = (size_t)(SD_LT + 2 * TL * sd_row(axes[a])) * 4;
    if (a == 0)
      UNET_LAUNCH((surf_dist_line_kernel<0, TT>), dim3(grid), dim3(SD_LT), shm, s, prob, t, field, D, H, W, K, thr, TL,
                  tiles);
    else if (a == 1)
      UNET_LAUNCH((surf_dist_line_kernel<1, TT>), dim3(grid), dim3(SD_LT), shm, s, prob, t, field, D, H, W, K, thr, TL,
                  tiles);
    else
      UNET_LAUNCH((surf_dist_line_kernel<2, TT>), dim3(grid), dim3(SD_LT), shm, s, prob, t, field, D, H, W, K, thr, TL,
                  tiles);
  }
  UNET_LAUNCH(surf_dist_select_kernel, dim3(N * K), dim3(SD_ST), 0, s, field, D * H * W, surf);
  return launch_status();
}

}  // namespace unet
