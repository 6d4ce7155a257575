// gather_batch_elastic with fp32 outputs (the fp32 executor's input and target buffers,
// Cpad = Cin): element-type independent, built once (gather_elastic.h; validation:
// gather_elastic.hip).
#include "gather_elastic.h"

namespace unet {

hipError_t f32_gather_batch_elastic_launch(const float* x_all, const float* y_all, const long long* idx,
                                           const int* origin, const int* code, const int* mat, const float* affine,
                                           const int* field, int B, int Ds, int Hs, int Ws, int D, int H, int W,
                                           int Cin, int Cpad, int K, int s, float* xb, float* tb, hipStream_t st) {
  return gather_batch_elastic_launch_t<float>(x_all, y_all, idx, origin, code, mat, affine, field, B, Ds, Hs, Ws, D,
                                              H, W, Cin, Cpad, K, s, xb, tb, st);
}

}  // namespace unet
