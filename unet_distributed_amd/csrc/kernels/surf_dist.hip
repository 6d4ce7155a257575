// surf_dist for the build's 16-bit target type (bf16 in namespace unet, fp16 in unet_f16):
// the kernels and their launcher are in surf_dist.h; the fp32-target instantiation of the
// fp32 executor is f32_surf_dist.hip.
#include "surf_dist.h"

namespace unet {

// plan-time validation (bindings.cpp make_generic): nullptr when the layout is accepted
const char* surf_dist_check(long long N, long long D, long long H, long long W, long long K) {
  if (K < 1 || K > 4) return "surf_dist: 1..4 classes";
  if (N < 1 || D < 1 || H < 1 || W < 1) return "surf_dist: N, D, H, W >= 1";
  if (D > SD_MAX_AXIS || H > SD_MAX_AXIS || W > SD_MAX_AXIS)
    return "surf_dist: D, H, W <= 4096 (squared distances below 2^26, 16-bit line positions)";
  const long long S = D * H * W;
  if (S % 8) return "surf_dist: S % 8 (16-byte aligned sample bases and field planes)";
  if (S >= (1LL << 24)) return "surf_dist: S >= 2^24";
  if (N * S * K >= (1LL << 31)) return "surf_dist: N S K >= 2^31";
  return nullptr;
}

// bytes of the field scratch of one launch over N samples: int32 [N][K][2][S]
long long surf_dist_scratch(long long N, long long D, long long H, long long W, long long K) {
  return N * K * 2 * D * H * W * 4;
}

hipError_t surf_dist_launch(const float* prob, const void* t, int N, int D, int H, int W, int K, float thr, int* field,
                            int* surf, hipStream_t s) {
  return surf_dist_launch_t<h16>(prob, (const h16*)t, N, D, H, W, K, thr, field, surf, s);
}

}  // namespace unet
