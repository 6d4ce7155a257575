// gather_batch_aug for the build's 16-bit type (bf16 in namespace unet, fp16 in unet_f16):
// the kernels and their launcher are in gather_aug.h; the fp32-output instantiation of the
// fp32 executor is f32_gather_aug.hip.
#include "gather_aug.h"

namespace unet {

const char* gather_aug_check(long long B, long long D, long long H, long long W, long long Cin, long long Cpad,
                             long long K) {
  if (B < 1 || D < 1 || H < 1) return "gather_batch_aug: B, D, H >= 1";
  if (H != W) return "gather_batch_aug: H == W (the rotations swap the two axes)";
  if (Cin < 1 || Cin > Cpad || Cpad > 64) return "gather_batch_aug: 1 <= Cin <= Cpad <= 64";
  if (K < 1 || K > 4) return "gather_batch_aug: 1..4 target channels";
  // (B, D <= 2^31 and H <= 2^16 from here on: the product cannot overflow 64 bits)
  if (B >= (1LL << 31) || D >= (1LL << 31) || H >= (1LL << 16) ||
      B * D >= (1LL << 31) || B * D * H * W * (Cpad > K ? Cpad : K) >= (1LL << 31))
    return "gather_batch_aug: B D H W max(Cpad, K) >= 2^31";
  return nullptr;
}

hipError_t gather_batch_aug_launch(const float* x_all, const float* y_all, const long long* idx, const int* code,
                                   const float* affine, int B, int D, int H, int W, int Cin, int Cpad, int K, void* xb,
                                   void* tb, hipStream_t s) {
  return gather_batch_aug_launch_t<h16>(x_all, y_all, idx, code, affine, B, D, H, W, Cin, Cpad, K, (h16*)xb, (h16*)tb,
                                        s);
}

}  // namespace unet
