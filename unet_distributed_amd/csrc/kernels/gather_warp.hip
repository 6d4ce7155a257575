// gather_batch_warp for the build's 16-bit type (bf16 in namespace unet, fp16 in unet_f16):
// the kernels and their launcher are in gather_warp.h; the fp32-output instantiation of the
// fp32 executor is f32_gather_warp.hip.
#include "gather_warp.h"

namespace unet {

const char* gather_warp_check(long long B, long long Ds, long long Hs, long long Ws, long long D, long long H,
                              long long W, long long Cin, long long Cpad, long long K) {
  if (B < 1 || D < 1 || H < 1) return "gather_batch_warp: B, D, H >= 1";
  if (H != W) return "gather_batch_warp: H == W (the rotations swap the two axes)";
  if (D > Ds || H > Hs || W > Ws) return "gather_batch_warp: the patch exceeds the stored sample (D <= Ds, H <= Hs, W <= Ws)";
  if (Cin < 1 || Cin > Cpad || Cpad > 64) return "gather_batch_warp: 1 <= Cin <= Cpad <= 64";
  if (K < 1 || K > 4) return "gather_batch_warp: 1..4 target channels";
  // (stored sides below 2^20: a sample's voxel count fits 64 bits with room for the channel count,
  // and a source coordinate in 2^-17 pixel stays below 2^38)
  if (Ds >= (1LL << 20) || Hs >= (1LL << 20) || Ws >= (1LL << 20))
    return "gather_batch_warp: stored side >= 2^20";
  // (B, D <= 2^31 and H <= 2^16 from here on: the product cannot overflow 64 bits)
  if (B >= (1LL << 31) || D >= (1LL << 31) || H >= (1LL << 16) ||
      B * D >= (1LL << 31) || B * D * H * W * (Cpad > K ? Cpad : K) >= (1LL << 31))
    return "gather_batch_warp: B D H W max(Cpad, K) >= 2^31";
  return nullptr;
}

hipError_t gather_batch_warp_launch(const float* x_all, const float* y_all, const long long* idx, const int* origin,
                                    const int* code, const int* mat, const float* affine, int B, int Ds, int Hs,
                                    int Ws, int D, int H, int W, int Cin, int Cpad, int K, void* xb, void* tb,
                                    hipStream_t s) {
  return gather_batch_warp_launch_t<h16>(x_all, y_all, idx, origin, code, mat, affine, B, Ds, Hs, Ws, D, H, W, Cin,
                                         Cpad, K, (h16*)xb, (h16*)tb, s);
}

}  // namespace unet
