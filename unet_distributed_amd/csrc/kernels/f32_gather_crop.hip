// gather_batch_crop with fp32 outputs (the fp32 executor's input and target buffers,
// Cpad = Cin): element-type independent, built once (gather_crop.h; validation:
// gather_crop.hip).
#include "gather_crop.h"

namespace unet {

hipError_t f32_gather_batch_crop_launch(const float* x_all, const float* y_all, const long long* idx,
                                        const int* origin, const int* code, const float* affine, int B, int Ds, int Hs,
                                        int Ws, int D, int H, int W, int Cin, int Cpad, int K, float* xb, float* tb,
                                        hipStream_t s) {
  return gather_batch_crop_launch_t<float>(x_all, y_all, idx, origin, code, affine, B, Ds, Hs, Ws, D, H, W, Cin, Cpad,
                                           K, xb, tb, s);
}

}  // namespace unet
