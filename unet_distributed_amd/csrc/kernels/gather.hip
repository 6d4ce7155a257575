// The five batch gathers for the build's 16-bit type (bf16 in namespace unet, fp16 in unet_f16)
// and their shape check: the kernels are in gather.h and gather_resample.h, the launcher at the
// end of the latter; the fp32-output instantiation of the fp32 executor is f32_gather.hip.
#include "gather_resample.h"

namespace unet {

// every reason starts with the op's generic name
#define GATHER_REFUSE(text)                                                                        \
  do {                                                                                             \
    static const char* const why[5] = {"gather_batch_aug: " text, "gather_batch_crop: " text,      \
                                       "gather_batch_warp: " text, "gather_batch_elastic: " text,  \
                                       "gather_batch_warp3: " text};                               \
    return why[(int)op];                                                                           \
  } while (0)

const char* gather_check(GatherOp op, const GatherArgs& a) {
  const long long B = a.B, D = a.D, H = a.H, W = a.W, Cin = a.Cin, Cpad = a.Cpad, K = a.K;
  if (B < 1 || D < 1 || H < 1) GATHER_REFUSE("B, D, H >= 1");
  if (H != W) GATHER_REFUSE("H == W (the rotations swap the two axes)");
  if (op != GatherOp::aug && (D > a.Ds || H > a.Hs || W > a.Ws))
    GATHER_REFUSE("the patch exceeds the stored sample (D <= Ds, H <= Hs, W <= Ws)");
  if (Cin < 1 || Cin > Cpad || Cpad > 64) GATHER_REFUSE("1 <= Cin <= Cpad <= 64");
  if (K < 1 || K > 4) GATHER_REFUSE("1..4 target channels");
  // (a cell of 8 .. 64 patch pixels: a 32-pixel tile touches at most 7 nodes per axis and the
  // displacement's 64-bit sum stays below 2^48; warp3 reads s only with a field)
  if ((op == GatherOp::elastic || (op == GatherOp::warp3 && a.field)) && (a.s < 3 || a.s > 6))
    GATHER_REFUSE("cell side 8, 16, 32 or 64 (3 <= s <= 6)");
  // (stored sides below 2^20: a sample's voxel count fits 64 bits with room for the channel count,
  // and a source coordinate in 2^-17 pixel stays below 2^38 before the displacement of at most 2^22)
  if (op != GatherOp::aug && (a.Ds >= (1LL << 20) || a.Hs >= (1LL << 20) || a.Ws >= (1LL << 20)))
    GATHER_REFUSE("stored side >= 2^20");
  // (warp3: t = 2 d' - (D - 1) stays below 2^16 in magnitude like u and v, so three products of at
  // most 2^34 and the centre below 2^37 keep |Q| < 2^38)
  if (op == GatherOp::warp3 && D >= (1LL << 16)) GATHER_REFUSE("D >= 2^16");
  // (B, D <= 2^31 and H <= 2^16 from here on: the product cannot overflow 64 bits)
  if (B >= (1LL << 31) || D >= (1LL << 31) || H >= (1LL << 16) ||
      B * D >= (1LL << 31) || B * D * H * W * (Cpad > K ? Cpad : K) >= (1LL << 31))
    GATHER_REFUSE("B D H W max(Cpad, K) >= 2^31");
  return nullptr;
}
#undef GATHER_REFUSE

hipError_t gather_launch(GatherOp op, const GatherArgs& a, void* xb, void* tb, hipStream_t s) {
  return gather_launch_t<h16>(op, a, (h16*)xb, (h16*)tb, s);
}

}  // namespace unet
