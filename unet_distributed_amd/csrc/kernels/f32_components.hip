// Connected-component filtering (components.h): plan-time validation, scratch size and the
// launcher.  The op reads and writes fp32 probabilities only, so it is element-type
// independent and built once (the f32* convention); it serves every executor.
#include "components.h"

namespace unet {

// plan-time validation (bindings.cpp make_generic): nullptr when the launch is accepted
const char* components_check(long long N, long long D, long long H, long long W, long long K, long long min_size) {
  const long long lim = 1LL << 31;
  if (K < 1 || K > 4) return "components: 1..4 classes";
  if (N < 1 || D < 1 || H < 1 || W < 1) return "components: N, D, H, W >= 1";
  if (N >= lim || D >= lim || H >= lim || W >= lim) return "components: N, D, H, W < 2^31";
  if (min_size < 0) return "components: min_size >= 0";
  if (min_size >= lim) return "components: min_size < 2^31";
  // (every factor is below 2^31 and each product is tested before the next factor: no overflow)
  const long long P = D * H;
  if (P >= lim || P * W >= lim) return "components: S = D H W >= 2^31 (int32 labels)";
  // one lane per element of the label planes, CC_BT lanes per workgroup, a 2^31 - 1 grid
  if (P * W * K >= lim || P * W * K * N >= lim * CC_BT) return "components: N S K >= 2^39 (the grid of a launch)";
  return nullptr;
}

// bytes of the scratch of one launch over N samples: int32 label [N][K][S], size [N][K][S],
// sel [N][K] and part [N][K][P][5], P = ceil(S / CC_CHUNK), rounded up to 16
long long components_scratch(long long N, long long D, long long H, long long W, long long K) {
  const long long S = D * H * W;
  const long long ints = N * K * (2 * S + 1 + 5 * cc_chunks(S));
  return (ints * 4 + 15) / 16 * 16;
}

hipError_t components_launch(const float* prob, int N, int D, int H, int W, int K, float thr, int keep_largest,
                             int min_size, int* scratch, float* out, int* info, hipStream_t s) {
  if (components_check(N, D, H, W, K, min_size) || !prob || !scratch || !out || !info || ((uintptr_t)scratch & 15))
    return hipErrorInvalidValue;
  if (!(thr > 0.0f && thr < 1.0f)) return hipErrorInvalidValue;
  const int S = D * H * W;
  const long long total = (long long)N * K * S;
  int* label = scratch;
  int* size = scratch + total;
  int* sel = scratch + 2 * total;
  int* part = sel + (long long)N * K;
  const int P = (int)cc_chunks(S);
  const unsigned grid = (unsigned)((total + CC_BT - 1) / CC_BT);
  UNET_LAUNCH(cc_init_kernel, dim3(grid), dim3(CC_BT), 0, s, prob, label, size, total, S, W, K, thr);
  UNET_LAUNCH(cc_merge_kernel, dim3(grid), dim3(CC_BT), 0, s, label, total, S, H, W);
  UNET_LAUNCH(cc_flatten_kernel, dim3(grid), dim3(CC_BT), 0, s, label, size, total, S);
  UNET_LAUNCH(cc_select_part_kernel, dim3((unsigned)((long long)N * K * P)), dim3(CC_ST), 0, s, label, size, S, P,
              min_size, part);
  UNET_LAUNCH(cc_select_kernel, dim3(N * K), dim3(CC_FT), 0, s, part, P, keep_largest, min_size, sel, info);
  UNET_LAUNCH(cc_write_kernel, dim3(grid), dim3(CC_BT), 0, s, prob, label, size, sel, total, S, K, keep_largest,
              min_size, out);
  return launch_status();
}

}  // namespace unet
