// gather_batch_warp with fp32 outputs (the fp32 executor's input and target buffers,
// Cpad = Cin): element-type independent, built once (gather_warp.h; validation:
// gather_warp.hip).
#include "gather_warp.h"

namespace unet {

hipError_t f32_gather_batch_warp_launch(const float* x_all, const float* y_all, const long long* idx,
                                        const int* origin, const int* code, const int* mat, const float* affine, int B,
                                        int Ds, int Hs, int Ws, int D, int H, int W, int Cin, int Cpad, int K,
                                        float* xb, float* tb, hipStream_t s) {
  return gather_batch_warp_launch_t<float>(x_all, y_all, idx, origin, code, mat, affine, B, Ds, Hs, Ws, D, H, W, Cin,
                                           Cpad, K, xb, tb, s);
}

}  // namespace unet
