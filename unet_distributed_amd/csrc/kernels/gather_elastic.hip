// gather_batch_elastic for the build's 16-bit type (bf16 in namespace unet, fp16 in unet_f16):
// the kernels and their launcher are in gather_elastic.h; the fp32-output instantiation of the
// fp32 executor is f32_gather_elastic.hip.
#include "gather_elastic.h"

namespace unet {

const char* gather_elastic_check(long long B, long long Ds, long long Hs, long long Ws, long long D, long long H,
                                 long long W, long long Cin, long long Cpad, long long K, long long s) {
  if (B < 1 || D < 1 || H < 1) return "gather_batch_elastic: B, D, H >= 1";
  if (H != W) return "gather_batch_elastic: H == W (the rotations swap the two axes)";
  if (D > Ds || H > Hs || W > Ws)
    return "gather_batch_elastic: the patch exceeds the stored sample (D <= Ds, H <= Hs, W <= Ws)";
  if (Cin < 1 || Cin > Cpad || Cpad > 64) return "gather_batch_elastic: 1 <= Cin <= Cpad <= 64";
  if (K < 1 || K > 4) return "gather_batch_elastic: 1..4 target channels";
  // (a cell of 8 .. 64 patch pixels: a 32-pixel tile touches at most 7 nodes per axis and the
  // displacement's 64-bit sum stays below 2^48)
  if (s < 3 || s > 6) return "gather_batch_elastic: cell side 8, 16, 32 or 64 (3 <= s <= 6)";
  // (stored sides below 2^20, as gather_batch_warp: a source coordinate in 2^-17 pixel stays below
  // 2^38 before the displacement of at most 2^22)
  if (Ds >= (1LL << 20) || Hs >= (1LL << 20) || Ws >= (1LL << 20))
    return "gather_batch_elastic: stored side >= 2^20";
  // (B, D <= 2^31 and H <= 2^16 from here on: the product cannot overflow 64 bits)
  if (B >= (1LL << 31) || D >= (1LL << 31) || H >= (1LL << 16) ||
      B * D >= (1LL << 31) || B * D * H * W * (Cpad > K ? Cpad : K) >= (1LL << 31))
    return "gather_batch_elastic: B D H W max(Cpad, K) >= 2^31";
  return nullptr;
}

hipError_t gather_batch_elastic_launch(const float* x_all, const float* y_all, const long long* idx,
                                       const int* origin, const int* code, const int* mat, const float* affine,
                                       const int* field, int B, int Ds, int Hs, int Ws, int D, int H, int W, int Cin,
                                       int Cpad, int K, int s, void* xb, void* tb, hipStream_t st) {
  return gather_batch_elastic_launch_t<h16>(x_all, y_all, idx, origin, code, mat, affine, field, B, Ds, Hs, Ws, D, H,
                                            W, Cin, Cpad, K, s, (h16*)xb, (h16*)tb, st);
}

}  // namespace unet
