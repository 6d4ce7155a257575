// tta_finish with an fp32 target (the fp32 executor's target buffer): element-type
// independent, built once (tta.h; validation and the tta_acc launcher: tta.hip).
#include "tta.h"

namespace unet {

hipError_t f32_tta_finish_launch(float* prob, const float* acc, const float* t, long long total, float inv_m,
                                 float* partial, float* sums, hipStream_t s) {
  return tta_finish_launch_t<float>(prob, acc, t, total, inv_m, partial, sums, s);
}

}  // namespace unet
