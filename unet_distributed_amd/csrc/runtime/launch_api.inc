// Host entry points of the HIP kernels (csrc/kernels/*.hip).  Included by
// launch_api.h once per element-type build: inside `namespace unet` (bf16) and
// `namespace unet_f16` (fp16); both builds share the unet_types parameter blocks.
// No include guard on purpose.
const char* conv_fwd_prepare(ConvFwdParams& p);
hipError_t conv_fwd_launch(const ConvFwdParams& p, hipStream_t s);
int conv_fwd_grid(const ConvFwdParams& p);   // row-window launches: workgroups; else 0
int conv_fwd_pick(const ConvFwdParams& p);   // kernel / tile id the launch runs (conv_fwd.hip)
// rows of p.stats written by the picked kernel (one per M tile) and pixels per tile;
// 0 rows when that kernel has no statistics epilogue for these parameters
void conv_stat_tiles(const ConvFwdParams& p, int* rows, int* tile_px);

const char* wgrad_check(const WgradParams& p);
WgradCfg wgrad_pick(const WgradParams& p);
hipError_t wgrad_launch(const WgradParams& p, hipStream_t s);
hipError_t wgrad_reduce_launch(const float* slab, int splits, int taps, int Mtot, int Mout, int Nc, int rg, int rkeep,
                               float scale, float* out, float* stage, hipStream_t s);
size_t wgrad_reduce_stage_floats(int splits, int taps, int Mtot, int Nc);
int reduce_groups(int splits);
hipError_t multi_reduce_launch(const void* jobs, int njobs, long long total1, long long total2, hipStream_t s);
hipError_t colsum_launch(const void* x, int rows, int C, int blocks, float* partial, hipStream_t s);

hipError_t cast_input_launch(const float* x, int P, int Cin, int Cpad, void* y, hipStream_t s);
// batch of the HBM-resident dataset by sample index -> padded 16-bit input + 16-bit target
// (K target channels per pixel, 1..4)
hipError_t gather_batch_launch(const float* x_all, const float* y_all, const long long* idx, int B, int P, int Cin,
                               int Cpad, void* xb, void* tb, int K, hipStream_t s);
// the five batch gathers with a per-sample transform riding on the pass (gather.h,
// gather_resample.h; GatherOp and GatherArgs: conv_params.h).  aug: a code (int32 [B]: bit 0 flip
// W, 1 flip H, 2 swap H and W, 3 flip D) and an optional per-channel affine (fp32 [B][Cin][2] =
// {scale, shift}) on the image; crop: the same on a D x H x W patch at origin (int32 [B][3] = (d,
// h, w), clamped into the sample by the kernel) of stored Ds x Hs x Ws samples; warp: the patch
// resampled through a Q16 matrix in the (H, W) plane (mat int32 [B][4], entries clamped into
// [-2^18, 2^18]): bilinear image, nearest target, zero outside the stored image; elastic: the
// warp with a per-pixel displacement of the source coordinates, a quadratic B-spline through
// field int32 [B][N][N][2] (2^-17 pixel, entries clamped into [-2^22, 2^22]), N = ((H - 1) >> s)
// + 3, cells of 1 << s patch pixels; warp3: the patch resampled trilinearly through a Q16 matrix
// over (d, h, w) (mat int32 [B][9], row-major), with the elastic displacement along (h, w) when a
// field is given.  H == W, patch <= stored on every axis.  Required besides x_all, y_all, idx, xb
// and tb: code (aug), origin (crop), mat (warp, warp3), field (elastic); every other pointer may
// be null (origin, code = 0; mat = the identity; warp3's field = no displacement)
const char* gather_check(GatherOp op, const GatherArgs& a);
hipError_t gather_launch(GatherOp op, const GatherArgs& a, void* xb, void* tb, hipStream_t s);
// code: optional uint32 per (pooled pixel, 8 channels) = first-argmax index per channel
// (2 / 3 bits); the backward reads it instead of x when non-null
hipError_t maxpool2_fwd_launch(const void* x, int N, int D, int H, int W, int C, int dims3, void* y, void* code,
                               hipStream_t s);
hipError_t maxpool2_bwd_launch(const void* x, const void* code, const void* dy, const void* skip, int N, int D, int H,
                               int W, int C, int dims3, void* dx, hipStream_t s);
// y = relu(fa z + fc) stored + 2x2 max-pool of it (pooled py, argmax codes) in one pass
hipError_t norm_pool_launch(const void* z, const float* fa, const float* fc, int cstride, int N, int D, int H, int W,
                            int C, int dims3, void* y, void* py, void* code, hipStream_t s);
// + the norm backward statistics rows[(n * nbp + b)][2][C] = {sum dx, sum dx z} (z: pre-norm input)
hipError_t maxpool2_bwd_norm_launch(const void* code, const void* dy, const void* skip, const void* z, int N, int D,
                                    int H, int W, int C, int dims3, int nbp, void* dx, float* rows, hipStream_t s);
hipError_t upsample2_fwd_launch(const void* x, int N, int D, int H, int W, int C, int dims3, void* y, hipStream_t s);
hipError_t upsample2_bwd_launch(const void* dup, const void* mask, int N, int D, int H, int W, int C, int dims3,
                                void* dlow, hipStream_t s);

int head_blocks(int P);
const char* head_check(int C, int K = 1);     // K: output classes (1: head.hip; 2..4: head_mc.hip)
hipError_t head_fwd_launch(const void* x, const float* w, const float* b, const void* t, int P, int C, float* prob,
                           float* partial, float* sums, hipStream_t s);
hipError_t head_bwd_launch(const void* x, const float* w, const float* prob, const void* t, const float* sums, int P,
                           int C, float inv_total, float bce_w, float gscale, const float* gscale_ptr, void* dx,
                           float* partial, float* gw, float* gb, hipStream_t s);
hipError_t partial_reduce_launch(const float* partial, int nb, int width, float* out, hipStream_t s);
// multi-class head (head_mc.hip), K = 2..4 sigmoid outputs: w [C][K], b [K], prob / t [P][K];
// partial: head_blocks(P) * max(4, C K + K) floats; hipErrorInvalidValue when P K or P C / 8
// does not fit a 32-bit index
const char* head_mc_check(int C, int K);
hipError_t head_mc_fwd_launch(const void* x, const float* w, const float* b, const void* t, int P, int C, int K,
                              float* prob, float* partial, float* sums, hipStream_t s);
hipError_t head_mc_bwd_launch(const void* x, const float* w, const float* prob, const void* t, const float* sums,
                              int P, int C, int K, float inv_total, float bce_w, float gscale,
                              const float* gscale_ptr, void* dx, float* partial, float* gw, float* gb,
                              hipStream_t s);
// dY of the head input from its ReLU bits (no head-input read; Mask gradients from head_ws)
hipError_t head_dy_launch(const void* bits, const float* w, const float* prob, const void* t, const float* sums, int P,
                          int C, float inv_total, float bce_w, float gscale, const float* gscale_ptr, void* dx,
                          hipStream_t s);
// Mask weight / bias gradients from the forward's per-workgroup sums (conv_params.h head_ws,
// rows [nrows][100], 32 head-input channels) and the loss sums
hipError_t head_wsum_grad_launch(const float* rows, int nrows, const float* sums, float inv_total, float bce_w,
                                 float gscale, const float* gscale_ptr, float* gw, float* gb, hipStream_t s);
// prob holds fp32 logits (fused-head conv epilogue): sigmoid in place + loss partials -> sums
hipError_t head_finish_launch(float* prob, const void* t, int P, float* partial, float* sums, hipStream_t s);
// norm mode: y = relu(fa z + fc) of the head input stored + the head logits (-> head_finish)
hipError_t norm_head_launch(const void* z, const float* fa, const float* fc, int cstride, int npix, const float* w,
                            const float* b, int P, int C, void* y, float* logit, hipStream_t s);
// norm-mode training head (head.hip): normalisation + logits + sigmoid + loss sums + the
// nine per-channel pixel sums of the backward in one pass (y optional), then the
// backward's coefficient rows / head gradients and dz = a w dlogit m + b z + c
int hn_blocks_per_sample(int N, int P);
int hn_partial_floats(int N, int P, int C);
hipError_t norm_head_loss_launch(const void* z, const float* fa, const float* fc, int cstride, int N, int npix,
                                 const float* w, const float* b, const void* t, void* y, int C, float* prob,
                                 float* partial, float* sums, hipStream_t s);
hipError_t head_norm_coef_launch(const float* partial, int N, int npix, int C, const float* sums, const float* w,
                                 const float* fa, const float* fc, int cstride, float inv_total, float bce_w,
                                 float gscale, const float* gscale_ptr, float* rows, float* gw, float* gb,
                                 hipStream_t s);
hipError_t head_norm_bwd_launch(const void* z, const float* prob, const void* t, const float* sums, const float* w,
                                const float* fa, const float* fc, const float* ca, const float* cb, const float* cc,
                                int cstride, int N, int P, int C, float inv_total, float bce_w, float gscale,
                                const float* gscale_ptr, void* dz, hipStream_t s);

// per-(sample, class) evaluation statistics (seg_stats.h): prob fp32 [N][S][K], t [N][S][K] in
// the build's 16-bit type, stats fp32 [N][K][6] = {I, St, Sp, TP, FP, FN} at threshold thr;
// partial: N * seg_stats_chunks(N, S, K) * 6 K floats (may be null when that is one chunk)
const char* seg_stats_check(long long N, long long S, long long K);
int seg_stats_chunks(int N, int S, int K);
hipError_t seg_stats_launch(const float* prob, const void* t, int N, int S, int K, float thr, float* partial,
                            float* stats, hipStream_t s);

// surface distances for HD95 (surf_dist.h): prob fp32 [N][S][K], t [N][S][K] in the build's 16-bit
// type, S = D H W; surf int32 [N][K][4] = {mp, mt, q_lo, q_hi} at threshold thr; field: scratch of
// surf_dist_scratch(N, D, H, W, K) bytes, 16-byte aligned, written before it is read
const char* surf_dist_check(long long N, long long D, long long H, long long W, long long K);
long long surf_dist_scratch(long long N, long long D, long long H, long long W, long long K);
hipError_t surf_dist_launch(const float* prob, const void* t, int N, int D, int H, int W, int K, float thr, int* field,
                            int* surf, hipStream_t s);

// test-time augmentation (tta.h): acc (= | +=) prob under one transform code (fp32 [N][D][H][W][K],
// H == W; mode 0 writes, 1 adds), then prob = (acc + prob) * inv_m in place with the loss sums
// {I, St, Sp, BCE} of that mean against t (the build's 16-bit type);
// partial: tta_finish_blocks(total) * 4 floats
const char* tta_acc_check(long long N, long long D, long long H, long long W, long long K, long long code,
                          long long mode);
const char* tta_finish_check(long long total);
int tta_finish_blocks(long long total);
hipError_t tta_acc_launch(const float* prob, float* acc, int N, int D, int H, int W, int K, int code, int mode,
                          hipStream_t s);
hipError_t tta_finish_launch(float* prob, const float* acc, const void* t, long long total, float inv_m,
                             float* partial, float* sums, hipStream_t s);

// sliding-window inference (sliding.h; fp32 in and out): xb [B][Td][Th][Tw][C] = the tiles
// [t0, t0 + nt) of x_all [N][D][H][W][C] (zeros elsewhere); acc [N][D][H][W][K] += w * prob of
// those tiles in ascending tile order (a multiplication, then an addition); acc /= wsum [D][H][W].
// sw_check: kind 0 extract, 1 blend; sw_geo: the SwGeo of the 14 integers sw_check accepted
const char* sw_check(long long kind, long long N, long long D, long long H, long long W, long long C, long long Td,
                     long long Th, long long Tw, long long sd, long long sh, long long sw, long long B, long long t0,
                     long long nt);
const char* sw_finish_check(long long N, long long D, long long H, long long W, long long K);
SwGeo sw_geo(const long long* v);
hipError_t sw_extract_launch(const float* x_all, float* xb, const SwGeo& g, hipStream_t s);
hipError_t sw_blend_launch(const float* prob, const float* w, float* acc, const SwGeo& g, hipStream_t s);
hipError_t sw_finish_launch(float* acc, const float* wsum, int N, int D, int H, int W, int K, hipStream_t s);

int norm_blocks_per_sample(int N, int P);
int sample_slices(int N);  // partial workspace of the finalize launchers: sample_slices(N) * 2 * C floats
const char* norm_check(int C, int G);
hipError_t norm_moments_launch(const void* A, const void* B, int N, int P, int C, float* partial, float* S,
                               hipStream_t s);
hipError_t bn_finalize_launch(const float* S, int N, int C, float count, int mode, const float* gamma, float eps,
                              float momentum, float* run_mean, float* run_var, float* mean, float* rstd, float* ca,
                              float* cb, float* cc, float* dgamma, float* dbeta, float* partial, const float* beta,
                              float* fa, float* fc, hipStream_t s);
hipError_t gn_finalize_launch(const float* S, int N, int C, int G, int P, int mode, const float* gamma, float eps,
                              float* mean, float* rstd, float* ca, float* cb, float* cc, float* dgamma, float* dbeta,
                              float* partial, const float* beta, float* fa, float* fc, hipStream_t s);
hipError_t moments_collect_launch(const float* partial, int N, int C, int nbp, float* S, hipStream_t s);
// statistics from partial rows [R][2][C] (conv-epilogue tiles or norm_rows blocks)
int row_slices(int R);      // slice workspace of bn_stats: row_slices(R) * 2 * C floats
hipError_t bn_stats_launch(const float* rows, int R, int C, float count, int mode, const float* gamma,
                           const float* beta, float eps, float momentum, float* run_mean, float* run_var, float* mean,
                           float* rstd, float* fa, float* fc, float* ca, float* cb, float* cc, float* dgamma,
                           float* dbeta, float* slices, hipStream_t s);
hipError_t gn_stats_launch(const float* rows, int N, int rps, int C, int G, int P, int mode, const float* gamma,
                           const float* beta, float eps, float* mean, float* rstd, float* fa, float* fc, float* ca,
                           float* cb, float* cc, float* dgamma, float* dbeta, float* work, hipStream_t s);
hipError_t norm_rows_launch(const void* A, const void* B, int N, int P, int C, float* rows, hipStream_t s);
hipError_t norm_apply_launch(const void* z, int N, int P, int C, const float* mean, const float* rstd, int cstride,
                             const float* gamma, const float* beta, int relu, float drop_rate, uint32_t seed,
                             const uint32_t* seed_ptr, uint32_t salt, int n0, void* y, hipStream_t s);
hipError_t norm_bwd_apply_launch(const void* g, const void* z, int N, int P, int C, const float* ca, const float* cb,
                                 const float* cc, int cstride, void* dz, hipStream_t s);

// composite transposed-conv backward (tconv_fused.hip): the S2D dgrad weights from the
// fp32 masters, and the chain rule from the 4x4-tap slab sums to the tconv gradients
const char* tconv_fused_check(int C, int K, int O, int Ca);
hipError_t tconv_compose_launch(const float* wt, const float* wa, int C, int K, int O, int Ca, int rowstride,
                                void* out, hipStream_t s);
hipError_t tconv_chain_launch(const float* Hs, const float* bs, const float* wa, int C, int K, int O, int Ca,
                              float* dwt, float* dbt, const float* wt, const float* bt, const float* skg, float* dwa,
                              hipStream_t s);

const char* adam_check(int nseg);
hipError_t adam_pack_launch(float* w, const float* g, float* m, float* v, int n_total, const void* segs, int nseg,
                            float lr_t, float b1, float b2, float eps, float gscale, int do_adam,
                            const float* dev_scalars, void* arena, hipStream_t s);

uint32_t crc32c_extend(uint32_t crc, const uint8_t* p, size_t n);
void gather_rows(const uint8_t* src, const int64_t* idx, int64_t n, int64_t row_bytes, uint8_t* dst, int threads);

// fp32 path (f32.hip)
const char* f32_conv_check(const F32Conv& p);
const char* f32_wgrad_check(const F32Wgrad& p);
void f32_wgrad_tile(int M1, int M2, int Nc, int* bm, int* bn);
hipError_t f32_conv_launch(const F32Conv& p, hipStream_t s);
hipError_t f32_wgrad_launch(const F32Wgrad& p, hipStream_t s);
hipError_t f32_pool_fwd_launch(const float* x, int N, int D, int H, int W, int C, int dims3, float* y, hipStream_t s);
hipError_t f32_pool_bwd_launch(const float* x, const float* dy, const float* skip, int N, int D, int H, int W, int C,
                               int dims3, float* dx, hipStream_t s);
// (D, H, W): the low resolution; bwd: dst[low] = sum of the children (times mask > 0 if given)
hipError_t f32_ups_launch(const float* src, const float* mask, int N, int D, int H, int W, int C, int dims3, int bwd,
                          float* dst, hipStream_t s);
int f32_head_blocks(int P);
hipError_t f32_head_fwd_launch(const float* x, const float* w, const float* b, const float* t, int P, int C,
                               float* prob, float* partial, float* sums, hipStream_t s);
// partial: f32_head_blocks(P) * (C + 1) + (C + 1) floats
hipError_t f32_head_bwd_launch(const float* x, const float* w, const float* prob, const float* t, const float* sums,
                               int P, int C, float inv_total, float bce_w, float* dx, float* partial, float* gw,
                               float* gb, hipStream_t s);
hipError_t f32_colsum_launch(const float* x, long long rows, int C, int blocks, float* partial, float* out,
                             hipStream_t s);
// seg_stats with an fp32 target (f32_seg_stats.hip)
hipError_t f32_seg_stats_launch(const float* prob, const float* t, int N, int S, int K, float thr, float* partial,
                                float* stats, hipStream_t s);
// gather_launch with fp32 outputs (f32_gather.hip)
hipError_t f32_gather_launch(GatherOp op, const GatherArgs& a, void* xb, void* tb, hipStream_t s);
// surf_dist with an fp32 target (f32_surf_dist.hip)
hipError_t f32_surf_dist_launch(const float* prob, const float* t, int N, int D, int H, int W, int K, float thr,
                                int* field, int* surf, hipStream_t s);
// tta_finish with an fp32 target (f32_tta.hip)
hipError_t f32_tta_finish_launch(float* prob, const float* acc, const float* t, long long total, float inv_m,
                                 float* partial, float* sums, hipStream_t s);
// connected-component filtering of thresholded probabilities (components.h, f32_components.hip):
// prob, out fp32 [N][S][K], S = D H W; info int32 [N][K][4] = {components, kept components, largest
// size, kept voxels} under the policy (keep_largest, min_size) at threshold thr; scratch:
// components_scratch(N, D, H, W, K) bytes, 16-byte aligned, written before it is read
const char* components_check(long long N, long long D, long long H, long long W, long long K, long long min_size);
long long components_scratch(long long N, long long D, long long H, long long W, long long K);
hipError_t components_launch(const float* prob, int N, int D, int H, int W, int K, float thr, int keep_largest,
                             int min_size, int* scratch, float* out, int* info, hipStream_t s);
// label maps from probabilities (labelmap.h, f32_labelmap.hip): prob fp32 [N][D][H][W][K] -> out uint8
// [N][Do][Ho][Wo], the source pasted at (od, oh, ow) and 0 elsewhere; counts int32 [N][5]: source
// voxels per slot (zeroed by the launch).  rule 0 nested, 1 argmax; values: values[m] in byte m - 1
const char* labelmap_check(long long N, long long D, long long H, long long W, long long K, long long Do, long long Ho,
                           long long Wo, long long od, long long oh, long long ow, long long rule, long long values,
                           double thr);
hipError_t labelmap_launch(const float* prob, int N, int D, int H, int W, int K, int Do, int Ho, int Wo, int od, int oh,
                           int ow, int rule, unsigned values, float thr, uint8_t* out, int* counts, hipStream_t s);
hipError_t f32_transpose_launch(const float* src, int T, int A, int B, int flip, float* dst, hipStream_t s);
