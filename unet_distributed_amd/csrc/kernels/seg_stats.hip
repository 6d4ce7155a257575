// seg_stats for the build's 16-bit target type (bf16 in namespace unet, fp16 in unet_f16):
// the kernel and its launcher are in seg_stats.h; the fp32-target instantiation of the
// fp32 executor is f32_seg_stats.hip.
#include "seg_stats.h"

namespace unet {

// plan-time validation (bindings.cpp make_generic): nullptr when the layout is accepted
const char* seg_stats_check(long long N, long long S, long long K) {
  if (K < 1 || K > 4) return "seg_stats: 1..4 classes";
  if (N < 1 || S < 1) return "seg_stats: N, S >= 1";
  if (S % 8) return "seg_stats: S % 8 (16-byte aligned sample bases)";
  if (S >= (1LL << 24)) return "seg_stats: S >= 2^24 (the counts must stay exact in fp32)";
  if (N * S * K >= (1LL << 31)) return "seg_stats: N S K >= 2^31";
  return nullptr;
}

// chunks a sample is split into: ~1024 workgroups over the launch (4 per CU), whole
// iterations of 256 U vectors per chunk, at most 256 chunks (the finish walks them)
int seg_stats_chunks(int N, int S, int K) {
  if (seg_stats_check(N, S, K)) return 1;
  const int iter = SEG_T * (K == 3 ? 3 : 4);
  const int vecs = S / 8 * K;
  const int iters = (vecs + iter - 1) / iter;
  int chunks = (1024 + N - 1) / N;
  chunks = chunks > 256 ? 256 : chunks;
  chunks = chunks > iters ? iters : chunks;
  const int per = (iters + chunks - 1) / chunks;
  return (iters + per - 1) / per;           // (no empty chunk)
}

hipError_t seg_stats_launch(const float* prob, const void* t, int N, int S, int K, float thr, float* partial,
                            float* stats, hipStream_t s) {
  return seg_stats_launch_t<h16>(prob, (const h16*)t, N, S, K, thr, partial, stats, s);
}

}  // namespace unet
