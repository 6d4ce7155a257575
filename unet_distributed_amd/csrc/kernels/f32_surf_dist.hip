// surf_dist with an fp32 target (the fp32 executor's target buffer): element-type
// independent, built once (surf_dist.h; validation and scratch size: surf_dist.hip).
#include "surf_dist.h"

namespace unet {

hipError_t f32_surf_dist_launch(const float* prob, const float* t, int N, int D, int H, int W, int K, float thr,
                                int* field, int* surf, hipStream_t s) {
  return surf_dist_launch_t<float>(prob, t, N, D, H, W, K, thr, field, surf, s);
}

}  // namespace unet
