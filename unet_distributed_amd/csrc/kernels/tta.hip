// Test-time augmentation ops (tta.h): plan-time validation, the type-independent tta_acc
// launcher and tta_finish for the build's 16-bit target type (bf16 in namespace unet, fp16 in
// unet_f16); the fp32-target instantiation of the fp32 executor is f32_tta.hip.
#include "tta.h"

namespace unet {

// plan-time validation (bindings.cpp make_generic): nullptr when the launch is accepted
const char* tta_acc_check(long long N, long long D, long long H, long long W, long long K, long long code,
                          long long mode) {
  if (K < 1 || K > 4) return "tta_acc: 1..4 classes";
  if (code < 0 || code > 15) return "tta_acc: code 0..15";
  if (mode != 0 && mode != 1) return "tta_acc: mode 0 (write) or 1 (add)";
  if (N < 1 || D < 1 || H < 1) return "tta_acc: N, D, H >= 1";
  if (H != W) return "tta_acc: H == W (square slices)";
  if (N * D * H * W * K >= (1LL << 31)) return "tta_acc: N D H W K >= 2^31";
  return nullptr;
}

const char* tta_finish_check(long long total) {
  if (total < 4 || total % 4) return "tta_finish: a positive multiple of 4 elements";
  if (total >= (1LL << 31)) return "tta_finish: 2^31 elements or more";
  return nullptr;
}

// blocks of the finish = rows of its partial buffer: one 4-element vector per lane and pass
int tta_finish_blocks(long long total) {
  const long long nb = (total / 4 + TTA_THREADS - 1) / TTA_THREADS;
  return (int)(nb < 1 ? 1 : (nb > TTA_FB ? TTA_FB : nb));
}

#ifndef UNET_FP16        // (fp32 in and out: element-type independent, the bf16 build's copy serves both)
hipError_t tta_acc_launch(const float* prob, float* acc, int N, int D, int H, int W, int K, int code, int mode,
                          hipStream_t s) {
  if (tta_acc_check(N, D, H, W, K, code, mode) || !prob || !acc) return hipErrorInvalidValue;
  code &= D > 1 ? 15 : 7;                   // (bits outside the dims are ignored, as the gather ignores them)
  // 1024 pixels per workgroup: a 32 x 32 tile with T, else a strip 32, 64 or 128 pixels wide
  const int shift = (code & 4) ? 5 : (W <= 32 ? 5 : (W <= 64 ? 6 : 7));
  const int sw = 1 << shift, sh = TTA_PIXELS >> shift;
  const int across = (W + sw - 1) / sw;
  const int ntile = across * ((H + sh - 1) / sh);
  if ((long long)N * D * ntile >= (1LL << 31)) return hipErrorInvalidValue;
  const int grid = N * D * ntile;
  // codes without T, whole pixels per 16-byte vector, rows of whole vectors, aligned buffers:
  // the 16-byte strip kernel; everything else (T, K = 3, odd rows) the flat float kernel
  const bool vec = !(code & 4) && K != 3 && (W * K) % 4 == 0 &&
                   !(((uintptr_t)prob | (uintptr_t)acc) & 15);
#define TTA_STRIP(KK) \
  UNET_LAUNCH((tta_acc_strip_kernel<KK>), dim3(grid), dim3(TTA_THREADS), 0, s, prob, acc, D, H, ntile, across, shift, code, mode)
  if (vec) {
    switch (K) {
      case 1: TTA_STRIP(1); break;
      case 2: TTA_STRIP(2); break;
      default: TTA_STRIP(4);
    }
    return launch_status();
  }
#undef TTA_STRIP
#define TTA_ACC(KK) \
  UNET_LAUNCH((tta_acc_kernel<KK>), dim3(grid), dim3(TTA_THREADS), 0, s, prob, acc, D, H, ntile, across, shift, code, mode)
  switch (K) {
    case 1: TTA_ACC(1); break;
    case 2: TTA_ACC(2); break;
    case 3: TTA_ACC(3); break;
    default: TTA_ACC(4);
  }
#undef TTA_ACC
  return launch_status();
}
#endif

hipError_t tta_finish_launch(float* prob, const float* acc, const void* t, long long total, float inv_m,
                             float* partial, float* sums, hipStream_t s) {
  return tta_finish_launch_t<h16>(prob, acc, (const h16*)t, total, inv_m, partial, sums, s);
}

}  // namespace unet
