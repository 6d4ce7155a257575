// Label maps from probability maps (labelmap.h): plan-time validation and the launcher.  The
// op reads fp32 probabilities and writes bytes and integers only, so it is element-type
// independent and built once (the f32* convention); it serves every executor.
#include "labelmap.h"

namespace unet {

// plan-time validation (bindings.cpp make_generic): nullptr when the launch is accepted
const char* labelmap_check(long long N, long long D, long long H, long long W, long long K, long long Do, long long Ho,
                           long long Wo, long long od, long long oh, long long ow, long long rule, long long values,
                           double thr) {
  const long long lim = 1LL << 31;
  if (K < 1 || K > 4) return "labelmap: 1..4 classes";
  if (N < 1 || D < 1 || H < 1 || W < 1 || Do < 1 || Ho < 1 || Wo < 1) return "labelmap: N, D, H, W, Do, Ho, Wo >= 1";
  if (N >= lim || D >= lim || H >= lim || W >= lim || Do >= lim || Ho >= lim || Wo >= lim)
    return "labelmap: N, D, H, W, Do, Ho, Wo < 2^31";
  if (Wo >= lim - LM_PIECE) return "labelmap: Wo < 2^31 - 256 (a row is walked in pieces of 256 labels)";
  // (every factor is below 2^31 and each product is tested before the next factor: no overflow)
  if (N * D >= lim || N * D * H >= lim || N * D * H * W >= lim) return "labelmap: N D H W >= 2^31";
  if (N * Do >= lim || N * Do * Ho >= lim || N * Do * Ho * Wo >= lim) return "labelmap: N Do Ho Wo >= 2^31";
  if (od < 0 || oh < 0 || ow < 0 || od > Do - D || oh > Ho - H || ow > Wo - W)
    return "labelmap: the box (offset + source extent) lies outside the destination";
  if (rule != 0 && rule != 1) return "labelmap: rule 0 (nested) or 1 (argmax)";
  if (!(thr > 0.0 && thr < 1.0) || !((float)thr > 0.0f && (float)thr < 1.0f)) return "labelmap: threshold in (0, 1)";
  if (values < 0 || values >= (1LL << 32)) return "labelmap: values are K bytes packed in 32 bits";
  for (int k = 0; k < K; ++k)
    if (((values >> (8 * k)) & 255) == 0) return "labelmap: a values byte of 0 (values[1..K] in 1..255)";
  return nullptr;
}

hipError_t labelmap_launch(const float* prob, int N, int D, int H, int W, int K, int Do, int Ho, int Wo, int od, int oh,
                           int ow, int rule, unsigned values, float thr, uint8_t* out, int* counts, hipStream_t s) {
  if (labelmap_check(N, D, H, W, K, Do, Ho, Wo, od, oh, ow, rule, values, thr) || !prob || !out || !counts ||
      (((uintptr_t)prob | (uintptr_t)counts) & 3))
    return hipErrorInvalidValue;
  LmGeo g;
  g.N = N, g.D = D, g.H = H, g.W = W, g.Do = Do, g.Ho = Ho, g.Wo = Wo, g.od = od, g.oh = oh, g.ow = ow;
  g.rule = rule, g.vals = values, g.thr = thr;
  // word stores: every row start and the base on a 4-byte boundary; 16-byte loads on top: every
  // source row start, the first voxel of every lane (x' - ow, x' % 4 == 0) and the base on a vector
  const bool word = Wo % 4 == 0 && !((uintptr_t)out & 3);
  const bool vec = word && ((long long)W * K) % 4 == 0 && ((long long)ow * K) % 4 == 0 && !((uintptr_t)prob & 15);
  const int mode = vec ? 2 : word ? 1 : 0;
  // a wave per contiguous range of units; workgroups of LM_WAVES waves, LM_WGS_PER_IMAGE per image
  // and LM_MAX_WGS in all at most
  const int pieces = (Wo + LM_PIECE - 1) / LM_PIECE;
  const unsigned units = (unsigned)((long long)N * Do * Ho * pieces);     // (<= N Do Ho Wo < 2^31)
  const long long per_image = (long long)N * LM_WGS_PER_IMAGE;
  const unsigned max_waves = (unsigned)(per_image < LM_MAX_WGS ? per_image : LM_MAX_WGS) * LM_WAVES;
  const unsigned upv = (units + max_waves - 1) / max_waves;
  const unsigned waves = (units + upv - 1) / upv;
  const unsigned grid = (waves + LM_WAVES - 1) / LM_WAVES;
  const long long nc = (long long)N * LM_SLOTS;
  UNET_LAUNCH(lm_zero_kernel, dim3((unsigned)((nc + 63) / 64)), dim3(64), 0, s, counts, nc);
#define LM_GO(KK, MM) \
  UNET_LAUNCH((labelmap_kernel<KK, MM>), dim3(grid), dim3(LM_THREADS), 0, s, prob, out, counts, g, pieces, units, upv)
#define LM_MODE(KK)              \
  switch (mode) {                \
    case 2: LM_GO(KK, 2); break; \
    case 1: LM_GO(KK, 1); break; \
    default: LM_GO(KK, 0);       \
  }
  switch (K) {
    case 1: LM_MODE(1); break;
    case 2: LM_MODE(2); break;
    case 3: LM_MODE(3); break;
    default: LM_MODE(4);
  }
#undef LM_MODE
#undef LM_GO
  return launch_status();
}

}  // namespace unet
