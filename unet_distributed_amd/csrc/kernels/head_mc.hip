// Multi-class segmentation head + loss on gfx950: K = 2..4 sigmoid outputs per pixel
// (`model.py:119-120` Mask 1x1 conv + sigmoid with n_cl_out > 1, `model.py:4-21` Dice).
//
// Forward:
//   z[p][k] = sum_c x[p][c] W[c][k] + b[k];   prob[p][k] = sigmoid(z[p][k])
//   (Mask/kernel [C][K]: flat index c K + k; prob / target [P][K], channels-last)
//   The Dice sums run over batch, space and class together, so the per-block partials
//   and `sums` stay the four scalars {I, St, Sp, BCE} of the single-class head (head.hip)
//   and a = -2 / (2I + 1), bb = 1 / (St + Sp + 1) are shared by every class.
// Backward:
//   dz[p][k] = head_dlogit(prob, t, a, bb, 1 / (P K), bce_w, g)        (head_grad.h, unchanged)
//   dx[p][c] = (x[p][c] > 0) sum_k dz[p][k] W[c][k]                    (ReLU of conv9b folded in)
//   dW[c][k] = sum_p dz[p][k] x[p][c],  db[k] = sum_p dz[p][k]  -> per-block partials, reduced in
//   a fixed order (no atomics: two runs give the same bits).
//
// A pixel's row of prob / target is 4K / 2K bytes (12 / 6 for K = 3): never a multiple of a
// vector width for every K, so those arrays are accessed with scalar loads and stores only;
// the head input (C / 8 aligned 16-byte chunks per pixel) is read in 16-byte loads, once.
// The single-class head (head.hip) keeps its own kernels and its fused variants; this file
// is the unfused K-class path the planner takes for n_cl_out > 1.
#include "common.h"
#include "head_grad.h"

namespace unet {

int head_blocks(int P);
hipError_t partial_reduce_launch(const float* partial, int nb, int width, float* out, hipStream_t s);

namespace {

constexpr int HT = 256;

// One lane per (pixel, 8-channel chunk): the CP = C / 8 lanes of a pixel are adjacent, so a
// wave reads 1 KiB of the head input per load instruction.  Each lane forms its chunk's K
// partial dots, xor shuffles add them across the pixel's lanes, and lane cc < K of the pixel
// takes class cc: its sigmoid / loss terms, the probability store and the target load, so
// the transcendental tail is spread over the pixel's lanes and a wave's stores of
// prob[p][k] are contiguous (K <= 4 <= CP).  FU pixels per lane and iteration, their loads
// issued first (a read-only pass needs several 16-byte loads in flight per lane).
// BCE term: max(z, 0) - z t + log1p(exp(-|z|)) with log1p(exp(-|z|)) = -log(max(p, 1 - p))
// (one fast log of a value in [0.5, 1]; absolute error ~1e-7 per term of a sum of O(1) terms).
constexpr int FU = 4;

template <int C, int K>
__global__ void __launch_bounds__(HT) head_mc_fwd_kernel(const h16* __restrict__ x, const float* __restrict__ w,
                                                         const float* __restrict__ b, const h16* __restrict__ t,
                                                         int P, float* __restrict__ prob,
                                                         float* __restrict__ partial) {
  constexpr int CP = C / 8;
  static_assert(K <= CP, "one class per lane of a pixel");
  __shared__ float red[4][HT / 64];
  const int cc = threadIdx.x % CP;
  float wr[8][K];
#pragma unroll
  for (int e = 0; e < 8; ++e)
#pragma unroll
    for (int k = 0; k < K; ++k) wr[e][k] = w[(cc * 8 + e) * K + k];
  const float bias = cc < K ? b[cc] : 0.f;
  float sI = 0.f, sT = 0.f, sP = 0.f, sB = 0.f;
  const long long total = (long long)P * CP, step = (long long)gridDim.x * HT;
  // (step is a multiple of CP: the lanes of a pixel run the same iterations)
  for (long long i0 = blockIdx.x * (long long)HT + threadIdx.x; i0 < total; i0 += FU * step) {
    u32x4 raw[FU];
#pragma unroll
    for (int u = 0; u < FU; ++u) {
      const long long i = i0 + u * step;
      raw[u] = i < total ? *(const u32x4*)(x + i * 8) : (u32x4){0u, 0u, 0u, 0u};
    }
#pragma unroll
    for (int u = 0; u < FU; ++u) {
      const long long i = i0 + u * step;
      float f[8], d[K];
      unpack8(raw[u], f);
#pragma unroll
      for (int k = 0; k < K; ++k) {
        d[k] = 0.f;
#pragma unroll
        for (int e = 0; e < 8; ++e) d[k] += f[e] * wr[e][k];
#pragma unroll
        for (int o = 1; o < CP; o <<= 1) d[k] += __shfl_xor(d[k], o, 64);
      }
      float z = d[0];
#pragma unroll
      for (int k = 1; k < K; ++k) z = cc == k ? d[k] : z;
      z += bias;
      if (i < total && cc < K) {
        const size_t q = (size_t)(i / CP) * K + cc;
        const float pr = 1.f / (1.f + __expf(-z));
        prob[q] = pr;
        sP += pr;
        if (t) {
          const float tv = (float)t[q];
          sI += tv * pr;
          sT += tv;
          sB += fmaxf(z, 0.f) - z * tv - __logf(fmaxf(pr, 1.f - pr));
        }
      }
    }
  }
  sI = wave_sum(sI);
  sT = wave_sum(sT);
  sP = wave_sum(sP);
  sB = wave_sum(sB);
  const int wv = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) {
    red[0][wv] = sI;
    red[1][wv] = sT;
    red[2][wv] = sP;
    red[3][wv] = sB;
  }
  __syncthreads();
  if (threadIdx.x < 4) {
    float s = 0.f;
    for (int k = 0; k < HT / 64; ++k) s += red[threadIdx.x][k];
    partial[blockIdx.x * 4 + threadIdx.x] = s;
  }
}

// One lane per (pixel, 8-channel chunk), as head_bwd_kernel.  Lane cc < K of a pixel loads
// class cc's probability and target (contiguous across the wave), forms its dlogit and sums
// db[cc]; the pixel's lanes then read the K dlogits from each other.  Block partial row:
// [C][K] weight sums then [K] bias sums.
template <int C, int K>
__global__ void __launch_bounds__(HT) head_mc_bwd_kernel(const h16* __restrict__ x, const float* __restrict__ w,
                                                         const float* __restrict__ prob, const h16* __restrict__ t,
                                                         const float* __restrict__ sums, int P, float inv_total,
                                                         float bce_w, float gscale,
                                                         const float* __restrict__ gscale_ptr, h16* __restrict__ dx,
                                                         float* __restrict__ partial) {
  constexpr int CP = C / 8, WD = C * K + K;
  if (gscale_ptr) gscale = *gscale_ptr;      // loss scale kept on the device (fp16 dynamic scaling)
  __shared__ float red[HT / 64][WD];
  const int cc = threadIdx.x % CP;
  float wr[8][K];
#pragma unroll
  for (int e = 0; e < 8; ++e)
#pragma unroll
    for (int k = 0; k < K; ++k) wr[e][k] = w[(cc * 8 + e) * K + k];
  const float I = sums[0], St = sums[1], Sp = sums[2];
  const float a = -2.f / (2.f * I + 1.f);
  const float bb = 1.f / (St + Sp + 1.f);
  float gw[8][K], gb = 0.f;
#pragma unroll
  for (int k = 0; k < K; ++k)
#pragma unroll
    for (int e = 0; e < 8; ++e) gw[e][k] = 0.f;
  const int lane0 = (threadIdx.x & 63) - cc;          // first lane of this lane's pixel
  const long long total = (long long)P * CP;
  // (the stride is a multiple of CP: the lanes of a pixel run the same iterations)
  for (long long i = blockIdx.x * (long long)HT + threadIdx.x; i < total; i += (long long)gridDim.x * HT) {
    float dzc = 0.f;
    if (cc < K) {
      const size_t q = (size_t)(i / CP) * K + cc;
      dzc = head_dlogit(prob[q], (float)t[q], a, bb, inv_total, bce_w, gscale);
      gb += dzc;
    }
    float dz[K];
#pragma unroll
    for (int k = 0; k < K; ++k) dz[k] = __shfl(dzc, lane0 + k, 64);
    float f[8], o[8];
    unpack8(*(const u32x4*)(x + i * 8), f);
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      float d = 0.f;
#pragma unroll
      for (int k = 0; k < K; ++k) {
        gw[e][k] += dz[k] * f[e];
        d += dz[k] * wr[e][k];
      }
      o[e] = f[e] > 0.f ? d : 0.f;      // ReLU of the head's input folded in
    }
    *(u32x4*)(dx + i * 8) = pack8(o);
  }
  // lanes l, l + CP, l + 2CP, ... hold the same channels: fold them, then across waves
#pragma unroll
  for (int e = 0; e < 8; ++e)
#pragma unroll
    for (int k = 0; k < K; ++k)
#pragma unroll
      for (int o = CP; o < 64; o <<= 1) gw[e][k] += __shfl_xor(gw[e][k], o, 64);
  // gb: lane l holds class l % CP's sum (0 for l % CP >= K)
#pragma unroll
  for (int o = CP; o < 64; o <<= 1) gb += __shfl_xor(gb, o, 64);
  const int wv = threadIdx.x >> 6, ln = threadIdx.x & 63;
  if (ln < CP) {
#pragma unroll
    for (int e = 0; e < 8; ++e)
#pragma unroll
      for (int k = 0; k < K; ++k) red[wv][(ln * 8 + e) * K + k] = gw[e][k];
  }
  if (ln < K) red[wv][C * K + ln] = gb;
  __syncthreads();
  for (int j = threadIdx.x; j < WD; j += HT) {
    float s = 0.f;
    for (int k = 0; k < HT / 64; ++k) s += red[k][j];
    partial[(size_t)blockIdx.x * WD + j] = s;
  }
}

// grad_w[j] = sum_b partial[b][j] (j < CK, flat [C][K]), grad_b[j - CK] = sum_b partial[b][j]:
// one block per column, fixed order
__global__ void __launch_bounds__(256) head_mc_grad_reduce_kernel(const float* __restrict__ partial, int nb, int CK,
                                                                  int K, float* __restrict__ gw,
                                                                  float* __restrict__ gb) {
  __shared__ float red[256];
  const int j = blockIdx.x;
  float s = 0.f;
  for (int k = threadIdx.x; k < nb; k += 256) s += partial[(size_t)k * (CK + K) + j];
  red[threadIdx.x] = s;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    if (j < CK)
      gw[j] = red[0];
    else
      gb[j - CK] = red[0];
  }
}

// 32-bit element indices of the K-wide arrays and of the 16-byte chunks
bool head_mc_fits(int P, int C, int K) {
  return P >= 0 && (long long)P * K < (1LL << 31) && (long long)P * (C / 8) < (1LL << 31);
}

}  // namespace

const char* head_mc_check(int C, int K) {
  if (K < 2 || K > 4) return "multi-class head: 2..4 output classes";
  if (C != 32 && C != 64) return "multi-class head: feature channels must be 32 or 64";
  return nullptr;
}

// blocks of the forward: FU (pixel, chunk) items per lane, at most 1024 blocks (all resident
// at once: a grid past the residency ran a short second round) -- never more than
// 2 head_blocks(P), so its 4 floats per block fit the backward's workspace
static int head_mc_fwd_blocks(int P, int C) {
  const long long nb = ((long long)P * (C / 8) + HT * FU - 1) / (HT * FU);
  return nb > 1024 ? 1024 : (nb < 1 ? 1 : (int)nb);
}

// workspace (both launches): head_blocks(P) * (C K + K) floats
hipError_t head_mc_fwd_launch(const void* x, const float* w, const float* b, const void* t, int P, int C, int K,
                              float* prob, float* partial, float* sums, hipStream_t s) {
  if (head_mc_check(C, K) || !head_mc_fits(P, C, K)) return hipErrorInvalidValue;
  const int nb = head_mc_fwd_blocks(P, C);
#define HEAD_MC_FWD(CC, KK)                                                                                     \
  UNET_LAUNCH((head_mc_fwd_kernel<CC, KK>), dim3(nb), dim3(HT), 0, s, (const h16*)x, w, b, (const h16*)t, P, prob, \
              partial)
  switch (C * 8 + K) {
    case 32 * 8 + 2: HEAD_MC_FWD(32, 2); break;
    case 32 * 8 + 3: HEAD_MC_FWD(32, 3); break;
    case 32 * 8 + 4: HEAD_MC_FWD(32, 4); break;
    case 64 * 8 + 2: HEAD_MC_FWD(64, 2); break;
    case 64 * 8 + 3: HEAD_MC_FWD(64, 3); break;
    default: HEAD_MC_FWD(64, 4);
  }
#undef HEAD_MC_FWD
  const hipError_t e = launch_status();
  if (e != hipSuccess) return e;
  return partial_reduce_launch(partial, nb, 4, sums, s);
}

hipError_t head_mc_bwd_launch(const void* x, const float* w, const float* prob, const void* t, const float* sums,
                              int P, int C, int K, float inv_total, float bce_w, float gscale,
                              const float* gscale_ptr, void* dx, float* partial, float* gw, float* gb,
                              hipStream_t s) {
  if (head_mc_check(C, K) || !head_mc_fits(P, C, K) || !dx) return hipErrorInvalidValue;
  const int nb = head_blocks(P);
#define HEAD_MC_BWD(CC, KK)                                                                                      \
  UNET_LAUNCH((head_mc_bwd_kernel<CC, KK>), dim3(nb), dim3(HT), 0, s, (const h16*)x, w, prob, (const h16*)t, sums, \
              P, inv_total, bce_w, gscale, gscale_ptr, (h16*)dx, partial)
  switch (C * 8 + K) {
    case 32 * 8 + 2: HEAD_MC_BWD(32, 2); break;
    case 32 * 8 + 3: HEAD_MC_BWD(32, 3); break;
    case 32 * 8 + 4: HEAD_MC_BWD(32, 4); break;
    case 64 * 8 + 2: HEAD_MC_BWD(64, 2); break;
    case 64 * 8 + 3: HEAD_MC_BWD(64, 3); break;
    default: HEAD_MC_BWD(64, 4);
  }
#undef HEAD_MC_BWD
  UNET_LAUNCH(head_mc_grad_reduce_kernel, dim3(C * K + K), dim3(256), 0, s, partial, nb, C * K, K, gw, gb);
  return launch_status();
}

}  // namespace unet
