// gather_batch_aug with fp32 outputs (the fp32 executor's input and target buffers,
// Cpad = Cin): element-type independent, built once (gather_aug.h; validation:
// gather_aug.hip).
#include "gather_aug.h"

namespace unet {

hipError_t f32_gather_batch_aug_launch(const float* x_all, const float* y_all, const long long* idx, const int* code,
                                       const float* affine, int B, int D, int H, int W, int Cin, int Cpad, int K,
                                       float* xb, float* tb, hipStream_t s) {
  return gather_batch_aug_launch_t<float>(x_all, y_all, idx, code, affine, B, D, H, W, Cin, Cpad, K, xb, tb, s);
}

}  // namespace unet
