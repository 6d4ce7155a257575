// Label maps from probability maps on gfx950: the last step of a prediction, from the (filtered)
// fp32 probabilities to the uint8 label volume that is written to a file, pasted into a larger
// destination at an offset (ops/labelmap.py is the definition and the oracle; the kernel is
// held to it bit for bit).  All integer arithmetic from the threshold on.
//
//   prob   fp32  [N][D][H][W][K]     channels-last, K = 1..4, D = 1 in 2D
//   out    uint8 [N][Do][Ho][Wo]     source voxel (d, h, w) at (d + od, h + oh, w + ow), 0 elsewhere
//   counts int32 [N][5]              source voxels of image n per slot m = 0..K (slots above K: 0)
//
// Per voxel on_k = p_k >= thr (NaN is never on) and the slot m is
//   rule 0 (nested): the number of leading channels that are on;
//   rule 1 (argmax): 0 when no channel is on, else 1 + the on channel of the greatest probability,
//                    the lowest index among equals (a sequential scan with a strict >).
// label = 0 for m = 0, else byte m - 1 of `vals` (values[1..K] packed, values[m] in 1..255).
//
// A streaming kernel: 4 K bytes read and 1 byte written per voxel, nothing else.
//
// Destination-centric.  A unit is a piece of LM_PIECE = 256 consecutive labels of one
// destination row (n, d', h'), 4 per lane of a wave; a row of Wo labels is ceil(Wo / LM_PIECE)
// units.  A wave owns a contiguous range of units and walks it: the unit's row decode, kept by
// increments (no division in the loop), and the test "this row is outside the box" are uniform
// over the wave.  The owner is the wave and not the workgroup because the project's rows are
// short (240 or 128 labels: one unit): a workgroup per row would run one wave in four.  Every
// destination byte is written exactly once, padding included: there is no memset of `out`
// and no read of it.
//
// MODE 1 / 2 (Wo and the base of `out` multiples of 4): a lane produces the 4 consecutive labels
// x' = 4 lane .. 4 lane + 3 of the piece and stores them as one aligned 4-byte word.  MODE 2 (ow K,
// W K multiples of 4 and `prob` 16-byte aligned) reads the 4 K contiguous floats of those voxels as
// K 16-byte vectors where all four lie in the box; MODE 1, and the lanes of MODE 2 that straddle
// an end of the box, read floats.  MODE 0 (any Wo, any base): the byte path, a lane's labels are
// x' = lane, lane + 64, ...: byte stores and float loads that are contiguous over the wave.
//
// Counts: per unit and slot a wave ballot and a population count into wave-uniform counters.
// At the end of the kernel the four waves' counters are summed through LDS and the workgroup
// issues one integer atomicAdd per image it ends in and non-empty slot; a wave whose range
// passes to the next image adds the finished image's counters itself (one lane per slot).
// A launch has at most LM_WGS_PER_IMAGE workgroups per image (and LM_MAX_WGS in all): the adds of
// one image all hit one cache line and are served one after the other, about 12 ns per workgroup
// measured on the MI355X -- 7440 one-wave workgroups on one 155 x 240 x 240 image took 92 us, the
// same voxels as 155 images 20 us -- so their number, not the bytes, would set the time of a single
// case (2048 workgroups: 30 us, 1024: 23 us), while many images want the waves (1024 slices pasted
// into 240 x 240: 67 us at 1024 workgroups, 51 us at 2048).  `counts` is
// zeroed by a launch of its own in front, on the same stream.  Integer sums do not depend on
// their order: two runs give the same bits.  No float atomics, and every loop bound comes
// from the geometry, never from data.
#pragma once
#include "common.h"

namespace unet {
namespace {

constexpr int LM_THREADS = 256;                // lanes per workgroup: four waves
constexpr int LM_WAVES = LM_THREADS / 64;
constexpr int LM_VOX = 4;                      // labels per lane and unit
constexpr int LM_PIECE = 256;                  // labels of a destination row per unit (64 lanes x LM_VOX)
constexpr int LM_MAX_WGS = 2048;               // workgroups of a launch, at most (256 CUs x 8: 32 waves per CU)
constexpr int LM_WGS_PER_IMAGE = 1024;         // ... and per image, at most (the adds of an image serialise)
constexpr int LM_SLOTS = 5;                    // counts per image (K + 1 <= 5 in use)
static_assert(LM_PIECE == 64 * LM_VOX, "a unit is 4 labels per lane of a wave");

struct LmGeo {
  int N, D, H, W, Do, Ho, Wo, od, oh, ow;
  int rule;                 // 0 nested, 1 argmax
  unsigned vals;            // byte m - 1: values[m]
  float thr;
};

// slot of one voxel from its K probabilities
template <int K>
__device__ __forceinline__ int lm_slot(const float* p, float thr, int rule) {
  int m = 0;
  if (rule == 0) {
    bool run = true;
#pragma unroll
    for (int k = 0; k < K; ++k) {
      run = run && p[k] >= thr;
      m += run ? 1 : 0;
    }
  } else {
    float best = -__builtin_huge_valf();
#pragma unroll
    for (int k = 0; k < K; ++k) {
      if (p[k] >= thr && p[k] > best) {
        best = p[k];
        m = k + 1;
      }
    }
  }
  return m;
}

__device__ __forceinline__ unsigned lm_label(int m, unsigned vals) {
  return m == 0 ? 0u : (vals >> (8 * (m - 1))) & 255u;
}

__global__ void __launch_bounds__(64) lm_zero_kernel(int* __restrict__ counts, long long n) {
  const long long i = (long long)blockIdx.x * 64 + threadIdx.x;
  if (i < n) counts[i] = 0;
}

// units = rows x pieces (< 2^31), pieces = ceil(Wo / LM_PIECE); upv: units per wave
template <int K, int MODE>
__global__ void __launch_bounds__(LM_THREADS) labelmap_kernel(const float* __restrict__ prob,
                                                              uint8_t* __restrict__ out, int* __restrict__ counts,
                                                              LmGeo g, int pieces, unsigned units, unsigned upv) {
  __shared__ int red[LM_WAVES][LM_SLOTS];
  __shared__ int redn[LM_WAVES];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const unsigned long long first = ((unsigned long long)blockIdx.x * LM_WAVES + wave) * upv;
  const unsigned u0 = first < units ? (unsigned)first : units;
  const unsigned u1 = units - u0 < upv ? units : u0 + upv;
  int cnt[K + 1];                                // wave-uniform
#pragma unroll
  for (int m = 0; m <= K; ++m) cnt[m] = 0;
  // wave-uniform decode of the first unit, kept by increments
  unsigned row = u0 / (unsigned)pieces;
  int piece = (int)(u0 - row * (unsigned)pieces);
  int hd = (int)(row % (unsigned)g.Ho);
  const unsigned t = row / (unsigned)g.Ho;
  int dd = (int)(t % (unsigned)g.Do), n = (int)(t / (unsigned)g.Do);
  const int cur0 = u0 < u1 ? n : -1;             // (an empty range: nothing to add)

  for (unsigned u = u0; u < u1; ++u) {
    const int d = dd - g.od, h = hd - g.oh;
    const bool live = d >= 0 && d < g.D && h >= 0 && h < g.H;      // the row crosses the box
    const int p0 = piece * LM_PIECE;
    uint8_t* orow = out + (size_t)row * g.Wo;
    const float* srow = prob + (((size_t)n * g.D + (live ? d : 0)) * g.H + (live ? h : 0)) * g.W * K;

    int slot[LM_VOX];                            // -1: outside the box (label 0, not counted)
    int xd[LM_VOX];                              // the destination column of label j
#pragma unroll
    for (int j = 0; j < LM_VOX; ++j) {
      xd[j] = MODE == 0 ? p0 + j * 64 + lane : p0 + lane * LM_VOX + j;
      slot[j] = -1;
    }
    if (live) {
      bool done = false;
      if (MODE == 2) {
        const int x = xd[0] - g.ow;
        if (x >= 0 && x + LM_VOX - 1 < g.W) {    // (then xd[3] < Wo: the box lies in the row)
          const f32x4* q = (const f32x4*)(srow + (size_t)x * K);
          float f[LM_VOX * K];
#pragma unroll
          for (int k = 0; k < K; ++k) {
            const f32x4 v = q[k];
            f[4 * k] = v[0], f[4 * k + 1] = v[1], f[4 * k + 2] = v[2], f[4 * k + 3] = v[3];
          }
#pragma unroll
          for (int j = 0; j < LM_VOX; ++j) slot[j] = lm_slot<K>(f + j * K, g.thr, g.rule);
          done = true;
        }
      }
      if (!done) {
#pragma unroll
        for (int j = 0; j < LM_VOX; ++j) {
          const int x = xd[j] - g.ow;
          if (x >= 0 && x < g.W) {               // (then xd[j] < Wo)
            float f[K];
#pragma unroll
            for (int k = 0; k < K; ++k) f[k] = srow[(size_t)x * K + k];
            slot[j] = lm_slot<K>(f, g.thr, g.rule);
          }
        }
      }
    }
    if (MODE == 0) {
#pragma unroll
      for (int j = 0; j < LM_VOX; ++j)
        if (xd[j] < g.Wo) orow[xd[j]] = (uint8_t)(slot[j] < 0 ? 0u : lm_label(slot[j], g.vals));
    } else if (xd[0] < g.Wo) {                   // (Wo % 4 == 0: the whole word lies in the row)
      unsigned w = 0;
#pragma unroll
      for (int j = 0; j < LM_VOX; ++j) w |= (slot[j] < 0 ? 0u : lm_label(slot[j], g.vals)) << (8 * j);
      *(unsigned*)(orow + xd[0]) = w;
    }
    if (live) {                                  // (wave-uniform)
#pragma unroll
      for (int m = 0; m <= K; ++m) {
        int c = 0;
#pragma unroll
        for (int j = 0; j < LM_VOX; ++j) c += __popcll(__ballot(slot[j] == m));
        cnt[m] += c;
      }
    }
    // the next unit
    if (++piece == pieces) {
      piece = 0;
      ++row;
      if (++hd == g.Ho) {
        hd = 0;
        if (++dd == g.Do) {
          dd = 0;
          if (u + 1 < u1) {                      // the range goes on in the next image: this one is done
            int v = 0;
#pragma unroll
            for (int m = 0; m <= K; ++m) {
              if (lane == m) v = cnt[m];
              cnt[m] = 0;
            }
            if (lane <= K && v) atomicAdd(counts + (size_t)n * LM_SLOTS + lane, v);
            ++n;
          }
        }
      }
    }
  }
  // the image each wave ended in: one add per distinct image of the workgroup and non-empty slot
  if (lane == 0) {
    redn[wave] = cur0 < 0 ? -1 : n;
#pragma unroll
    for (int m = 0; m <= K; ++m) red[wave][m] = cnt[m];
  }
  __syncthreads();
  if (tid < LM_WAVES * LM_SLOTS) {
    const int w = tid / LM_SLOTS, m = tid - w * LM_SLOTS;
    const int nw = redn[w];
    if (m <= K && nw >= 0) {
      bool lead = true;
      int s = 0;
      for (int w2 = 0; w2 < LM_WAVES; ++w2) {
        if (redn[w2] != nw) continue;
        lead = lead && w2 >= w;
        s += red[w2][m];
      }
      if (lead && s) atomicAdd(counts + (size_t)nw * LM_SLOTS + m, s);
    }
  }
}

}  // namespace

// rule: 0 nested, 1 argmax; values: values[1..K] packed, values[m] in byte m - 1
const char* labelmap_check(long long N, long long D, long long H, long long W, long long K, long long Do, long long Ho,
                           long long Wo, long long od, long long oh, long long ow, long long rule, long long values,
                           double thr);
hipError_t labelmap_launch(const float* prob, int N, int D, int H, int W, int K, int Do, int Ho, int Wo, int od, int oh,
                           int ow, int rule, unsigned values, float thr, uint8_t* out, int* counts, hipStream_t s);

}  // namespace unet
