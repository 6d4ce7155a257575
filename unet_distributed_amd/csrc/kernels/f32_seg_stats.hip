// seg_stats with an fp32 target (the fp32 executor's target buffer): element-type
// independent, built once (seg_stats.h; validation and chunking: seg_stats.hip).
#include "seg_stats.h"

namespace unet {

hipError_t f32_seg_stats_launch(const float* prob, const float* t, int N, int S, int K, float thr, float* partial,
                                float* stats, hipStream_t s) {
  return seg_stats_launch_t<float>(prob, t, N, S, K, thr, partial, stats, s);
}

}  // namespace unet
