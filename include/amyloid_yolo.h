/*
 * amyloid_yolo.h -- C ABI of libamyloid_yolo_hip.so (gfx950 / MI355X).
 *
 * The reference (keiserlab/amyloid-yolo-paper) is pure Python/PyTorch and has no FFI for this path
 * (SURVEY.md §8b); its "operator interface" is the Python call surface of models.py / utils/utils.py.
 * Each entry point below names the reference code it replaces.  The host-side mirror of that Python
 * surface lives in amyloid_yolo_paper_amd/{models,utils}.py and binds these symbols with ctypes
 * (INTEGRATION.md shows the stub).
 *
 * Conventions: every function returns 0 on success or a negative AY_ERR_* code; ay_last_error() gives
 * a thread-local message.  All buffers are caller-allocated DEVICE pointers (the library never
 * allocates or frees), every call is stream-ordered on `stream` (a hipStream_t passed as void*) and
 * performs no host synchronisation.  No torch types appear here.
 *
 * Activation layouts
 *   "blocked bf16"  [B][C/16][H][W][16] bfloat16   -- the MFMA path ("c16" planes; C padded to 16)
 *   "blocked f32"   [B][C/16][H][W][16] float      -- head outputs of the bf16 path
 *   "nchw f32"      [B][C][H][W] float             -- the reference's layout; fp32 parity path + I/O
 */
#ifndef AMYLOID_YOLO_H
#define AMYLOID_YOLO_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define AY_OK 0
#define AY_ERR_ARG (-1)      /* bad argument / unsupported shape */
#define AY_ERR_LAUNCH (-2)   /* HIP launch error */
#define AY_ERR_WORKSPACE (-3)

typedef void* ay_stream_t; /* hipStream_t */

/* 16-bit storage type of the MFMA path's activations and packed filters.  Same layouts, bytes and MFMA rate; bfloat16 keeps
 * fp32's exponent range (training, default), IEEE half (inference only: the *_f16 entry points below) has an 11-bit
 * significand -- an 8x smaller rounding step per stored activation (BASELINE.json configs[4] "fp16 MFMA path") -- and is
 * finite up to 65504: stored activations are post-BatchNorm, heads leave the path as fp32. */
#define AY_DT_BF16 0
#define AY_DT_F16 1

/* ABI version of this header: bumped whenever an exported signature changes (2: ay_plan_create gained `act_dtype` in the middle of
 * its argument list).  A binding compares ay_version() with the version it was written against before the first call, so that a
 * stale libamyloid_yolo_hip.so (or an out-of-tree caller of the old 7-argument form) fails at load time instead of passing a pointer
 * as a dtype (amyloid_yolo_paper_amd/_lib.py: ABI_VERSION). */
#define AY_ABI_VERSION 2
int ay_version(void);
const char* ay_last_error(void);

/* One convolutional block: conv -> (BN affine | bias) -> LeakyReLU(0.1)? -> (+ residual)?
 * Replaces models.py:26-45 executed at models.py:242-243, with the following shortcut
 * (models.py:246-248) fused as `residual`. */
typedef struct ay_conv_desc {
    int32_t batch;
    int32_t cin, cout;         /* logical channels */
    int32_t hin, win;          /* input spatial size; hin != win is pinned bit for bit by tests/test_gpu_conv_exact.py for the
                                  convolution, data- and weight-gradient, fused-block and stem entry points (16-bit and fp32);
                                  ay_head_decode_fwd_* refuses a rectangle */
    int32_t hout, wout;        /* output spatial size = floor((hin + 2*pad - k)/stride) + 1, pad=(k-1)/2 */
    int32_t ksize, stride;     /* 1|3 ; 1|2 */
    int32_t leaky;             /* 1: LeakyReLU(0.1) after the affine */
    int32_t out_f32;           /* bf16 path only: 1 = store blocked f32 (linear heads), 0 = blocked bf16 */
    int32_t cout_pad;          /* channels in scale/shift/packed weights/output planes: multiple of 16 (bf16 path: 32) */
} ay_conv_desc;

/* ---- bf16 MFMA path -------------------------------------------------------------------------- */

/* OIHW fp32 weights -> packed bf16 [cin/16][k*k][2][cout_pad][8] (zero rows for cout..cout_pad). */
int ay_pack_conv_weights_bf16(const float* w_oihw, void* packed, int cout, int cout_pad, int cin, int ksize,
                              ay_stream_t stream);
size_t ay_packed_weight_bytes(int cout_pad, int cin, int ksize);

/* BN (eval) -> per-channel scale/shift (models.py:43 semantics, eps passed in); bias-only layers use
 * gamma=NULL: scale=1, shift=bias.  Pads [n, n_pad) with scale=0, shift=0. */
int ay_fold_bn(const float* gamma, const float* beta, const float* mean, const float* var, const float* bias,
               float eps, float* scale, float* shift, int n, int n_pad, ay_stream_t stream);

/* Stem: nchw f32 image [B,3,H,W] -> blocked bf16 [B][2][H][W][16] (3x3 s1 conv 3->32, fp32 math). */
int ay_stem_conv_fwd(const float* x_nchw, const float* w_oihw, const float* scale, const float* shift,
                     void* out_blocked, int batch, int h, int w, int leaky, ay_stream_t stream);

/* Layer 0 + layer 1 of the Darknet-53 stem fused (3x3 s1 3->32, then 3x3 s2 32->64, each with BN affine + leaky): the
 * 32-channel full-resolution intermediate stays in LDS.  stem_w_bf16: [32][32] bf16, k = ci*9+kh*3+kw (27..31 zero);
 * w1_packed: ay_pack_conv_weights_bf16 of the 64x32x3x3 filters (cout_pad 64); out: blocked bf16 [B][4][H/2][W/2][16].
 * The image and the stem filters enter the MFMA as bf16 (fp32 accumulate). */
int ay_stem_s2_fused_fwd(const float* x_nchw, const void* stem_w_bf16, const float* scale0, const float* shift0, int leaky0,
                         const void* w1_packed, const float* scale1, const float* shift1, int leaky1, void* out_blocked,
                         int batch, int h, int w, ay_stream_t stream);

/* Direction in which the persistent convolution launches (stem, ay_conv_fwd_*, ay_conv3x3_m16_fwd_*, ay_conv1x1_cat_fwd_*,
 * ay_resblock_fwd_*, ay_head_decode_fwd_*) that THIS host thread issues from now on walk their work items: 0 (the default) upward,
 * 1 downward inside each XCD's range.  Same results bit for bit; a plan with alternation sets it per op (ay_plan_set_alternation)
 * and puts back what it found.  Training never sets it. */
void ay_conv_set_traversal(int reverse);
int ay_conv_get_traversal(void);

/* TESTS AND DEBUGGING ONLY -- the one convolution entry that synchronises: it waits for the current device, then reads the state of
 * the dynamic item dealing there.  The rule it lets a test observe: a ring-convolution launch that deals dynamically takes one
 * counter set (16 words: 8 per-XCD item counters, an exit counter) from the 64 that its (device, stream) pair owns, in rotation;
 * up to 16 streams per device own sets, in the order of their first dynamic launch, for the life of the process; a launch on a
 * further stream, and every launch that deals statically, takes none.  A set belongs to its launch from the launch's first
 * workgroup to its last, which hands it back zeroed: with no launch in flight every word of every set is zero.  A captured kernel
 * node keeps the pointer of the set it was given at capture -- a set of the CAPTURE stream -- so a replay is correct on the
 * capture stream, or on any stream while no other library work runs on the capture stream.
 *   slot           index of `stream` among the current device's owners, -1 if it owns no sets
 *   launches       counter sets `stream` has taken so far (0 without an entry)
 *   nonzero_words  non-zero 32-bit words in all sets of the device
 * The call neither registers `stream` nor advances a rotation. */
int ay_conv_deal_probe(ay_stream_t stream, int32_t* slot, uint32_t* launches, int32_t* nonzero_words);

/* 3x3 (stride 1|2) and 1x1 convolution, blocked bf16 in, MFMA 32x32x16 bf16, fp32 accumulate,
 * fused scale/shift + leaky + residual epilogue; `residual` (blocked bf16, output shape) may be NULL. */
int ay_conv_fwd_bf16(const ay_conv_desc* d, const void* src, const void* w_packed, const float* scale,
                     const float* shift, const void* residual, void* out, ay_stream_t stream);

/* The 3x3 stride-1 member of ay_conv_fwd_bf16 for cout_pad % 128 == 0, cin % 32 == 0, at least 16 output rows: the same
 * block (models.py:26-45, 246-248) on v_mfma_f32_16x16x32_bf16, which the chip clocks higher than the 32x32x16 form on
 * non-trivial data.  ay_conv_fwd_bf16 dispatches to it (AY_M16=0 in the environment keeps the 32x32x16 kernel); same
 * arguments, same rounding contract (bf16 operands, fp32 accumulation in a different order, one rounding per output). */
int ay_conv3x3_m16_fwd_bf16(const ay_conv_desc* d, const void* src, const void* w_packed, const float* scale, const float* shift,
                            const void* residual, void* out, ay_stream_t stream);

/* The same 1x1 convolution over a route that is never materialised (models.py:86-96,244-245): input channels
 * [0, c1) come from src1_halfres ([B][c1/16][H/2][W/2][16], nearest x2 upsample folded into the loader), channels
 * [c1, cin) from src2 ([B][(cin-c1)/16][H][W][16]); c1 and cin-c1 multiples of 64, cout_pad a multiple of 128. */
int ay_conv1x1_cat_fwd_bf16(const ay_conv_desc* d, const void* src1_halfres, int c1, const void* src2, const void* w_packed,
                            const float* scale, const float* shift, void* out, ay_stream_t stream);

/* Fused Darknet-53 residual block (models.py:26-45 twice + the shortcut at :246-248):
 * out = leaky(bn2(conv3x3(leaky(bn1(conv1x1(x)))))) + x, channels C -> C/2 -> C, in one kernel: the C/2-channel
 * intermediate stays in LDS.  x/out blocked bf16 [B][C/16][H][W][16] (out != x); w1_packed = ay_pack_conv_weights_bf16 of
 * the [C/2][C][1][1] filters (cout_pad C/2), w2_packed of the [C][C/2][3][3] filters (cout_pad C); scale/shift from
 * ay_fold_bn.  Same rounding points as the two ay_conv_fwd_bf16 calls it replaces (one bf16 rounding of the intermediate,
 * one of the output).  ay_resblock_supported(C) says whether C has a fused kernel (64 and 128); other blocks use the
 * two-call path. */
int ay_resblock_supported(int channels);
int ay_resblock_fwd_bf16(const void* x, const void* w1_packed, const float* scale1, const float* shift1, int leaky1,
                         const void* w2_packed, const float* scale2, const float* shift2, int leaky2, void* out, int batch,
                         int channels, int h, int w, ay_stream_t stream);

/* route (models.py:244-245) + nearest x2 upsample (models.py:86-96) as one gather into a blocked bf16
 * tensor [B][(c1+c2)/16][H][W][16]: src1 [B][c1/16][H>>up1][W>>up1][16], src2 [B][c2/16][H][W][16]|NULL. */
int ay_concat_upsample_bf16(const void* src1, int c1, int up1, const void* src2, int c2, void* out,
                            int batch, int h, int w, ay_stream_t stream);

/* layout converters (tests, fp32<->bf16 path bridges): to blocked rounds to nearest even and writes +0 into the lanes C .. 16*ceil(C/16);
 * from blocked never reads those lanes */
int ay_blocked_bf16_to_nchw_f32(const void* src, float* dst, int batch, int c, int h, int w, ay_stream_t stream);
int ay_blocked_f32_to_nchw_f32(const float* src, float* dst, int batch, int c, int h, int w, ay_stream_t stream);
int ay_nchw_f32_to_blocked_bf16(const float* src, void* dst, int batch, int c, int h, int w, ay_stream_t stream);

/* ---- the same inference entry points on IEEE half ("blocked f16": [B][C/16][H][W][16] half; packed filters half) ----------
 * Identical arguments, layouts, fusion and rounding points (operands 16-bit, fp32 accumulate, fp32 epilogue, ONE rounding per
 * stored activation -- to half instead of bfloat16); v_mfma_f32_{32x32x16,16x16x32}_f16 in place of the _bf16 forms.
 * ay_concat_upsample_bf16 moves 16-bit elements untouched and serves both types.  Replaces the same reference lines as the
 * _bf16 entry point of the same name (models.py:26-45, 86-96, 244-248). */
int ay_pack_conv_weights_f16(const float* w_oihw, void* packed, int cout, int cout_pad, int cin, int ksize, ay_stream_t stream);
int ay_stem_conv_fwd_f16(const float* x_nchw, const float* w_oihw, const float* scale, const float* shift,
                         void* out_blocked, int batch, int h, int w, int leaky, ay_stream_t stream);
/* stem_w_f16: [32][32] half, k = ci*9+kh*3+kw (27..31 zero) */
int ay_stem_s2_fused_fwd_f16(const float* x_nchw, const void* stem_w_f16, const float* scale0, const float* shift0, int leaky0,
                             const void* w1_packed, const float* scale1, const float* shift1, int leaky1, void* out_blocked,
                             int batch, int h, int w, ay_stream_t stream);
int ay_conv_fwd_f16(const ay_conv_desc* d, const void* src, const void* w_packed, const float* scale,
                    const float* shift, const void* residual, void* out, ay_stream_t stream);
int ay_conv3x3_m16_fwd_f16(const ay_conv_desc* d, const void* src, const void* w_packed, const float* scale, const float* shift,
                           const void* residual, void* out, ay_stream_t stream);
int ay_conv1x1_cat_fwd_f16(const ay_conv_desc* d, const void* src1_halfres, int c1, const void* src2, const void* w_packed,
                           const float* scale, const float* shift, void* out, ay_stream_t stream);
int ay_resblock_fwd_f16(const void* x, const void* w1_packed, const float* scale1, const float* shift1, int leaky1,
                        const void* w2_packed, const float* scale2, const float* shift2, int leaky2, void* out, int batch,
                        int channels, int h, int w, ay_stream_t stream);
int ay_blocked_f16_to_nchw_f32(const void* src, float* dst, int batch, int c, int h, int w, ay_stream_t stream);
/* Rounds to nearest even like ay_nchw_f32_to_blocked_bf16 (subnormal results included), with ONE difference from IEEE: a finite value
 * that would round to +-inf is stored as +-65504 (every kernel that stores halves saturates); +-inf and NaN pass through. */
int ay_nchw_f32_to_blocked_f16(const float* src, void* dst, int batch, int c, int h, int w, ay_stream_t stream);

/* ---- fp32 parity path (reference layout) ------------------------------------------------------ */

/* Same block in nchw f32 with OIHW fp32 weights; src2/c-split/up1 implement route+upsample in the
 * loader: channels [0,cin1) come from src1 read at (y>>up1, x>>up1), [cin1,cin) from src2.
 * up1 is 0 or 1; with up1 == 1 src1 is (hin/2) x (win/2) and hin, win must be even (an x2 upsample's sides are): an odd side is
 * refused with AY_ERR_ARG and `out` is not touched.  The same holds for ay_conv_fwd_f32_valu and ay_conv_fwd_split. */
int ay_conv_fwd_f32(const ay_conv_desc* d, const float* src1, int cin1, int up1, const float* src2,
                    const float* w_oihw, const float* scale, const float* shift, const float* residual,
                    float* out, ay_stream_t stream);
/* The same block restricted to the VALU kernel (one fmaf chain per output in (ci, kh, kw) order; no matrix cores): the fp32
 * training engine's forward, whose gradients are pinned element-wise by the reference's training fixtures on that summation
 * order.  ay_conv_fwd_f32 itself runs the cfg format's shapes on exact-fp32 MFMA (v_mfma_f32_32x32x2_f32). */
int ay_conv_fwd_f32_valu(const ay_conv_desc* d, const float* src1, int cin1, int up1, const float* src2,
                    const float* w_oihw, const float* scale, const float* shift, const float* residual,
                    float* out, ay_stream_t stream);

/* ---- split-bf16 parity path: fp32-grade products on the bf16 matrix cores ------------------------ */

/* The block of ay_conv_fwd_f32 -- same operands, layouts, route / upsample loader and epilogue -- with both fp32 operands split
 * into bf16 planes in the loader and the plane products run on v_mfma_f32_32x32x16_bf16 into fp32 accumulators.
 *
 * THE SPLIT RULE.  For an fp32 value x:
 *     p0 = bf16_rne(x),   p1 = bf16_rne(x - p0),   p2 = bf16_rne(x - p0 - p1)
 * (bf16_rne: round to nearest even to 8 significand bits; every subtraction is in fp32 and exact).  p0 + p1 + p2 == x exactly;
 * |x - p0 - p1| <= 2^-16 |x|.  With q the planes of the other operand,
 *     nsplit = 2 ("bf16x3"):  x*y ~ p0q0 + p0q1 + p1q0                        dropped terms <= 3 * 2^-16 |x||y|
 *     nsplit = 3 ("bf16x6"):  x*y ~ p0q0 + p0q1 + p1q0 + p0q2 + p2q0 + p1q1   dropped terms <= 2^-22 |x||y|
 * Every included product is exact in fp32 (8 x 8 significand bits) and is accumulated in fp32 by the MFMA (nsplit = 3: p0q0 in one
 * accumulator, the five correction products in a second one, the two added in fp32 before the epilogue).  The epilogue is
 * ay_conv_fwd_f32's, operation for operation and unfused: acc * scale + shift, LeakyReLU(0.1), + residual, fp32 store.
 * Outside the rule: non-finite inputs (inf - inf in the split gives NaN planes) and fp32 subnormals (inputs, and residuals
 * x - p0 that fall below 2^-126, which the matrix cores may flush).
 *
 * Covered: 3x3 stride 1 / 2 and 1x1 stride 1 (the cfg format's shapes).  Anything else is refused with AY_ERR_ARG and a message
 * (ay_last_error) and `out` is not touched -- there is no fallback to another arithmetic: other kernel sizes, a route whose
 * cin1 is not a multiple of 16, an image or filter tensor beyond the 32-bit descriptor range (2 GiB), nsplit outside {2, 3}. */
int ay_conv_fwd_split(const ay_conv_desc* d, const float* src1, int cin1, int up1, const float* src2,
                      const float* w_oihw, const float* scale, const float* shift, const float* residual,
                      float* out, int nsplit, ay_stream_t stream);

/* ---- YOLO head decode: models.py:127-172 ------------------------------------------------------- */
/* head: blocked f32 [B][cpad/16][G][G][16], cpad = A*(5+C) rounded up to 32 (layout=1) or nchw f32 [B][A*(5+C)][G][G] (layout=0).
 * Writes rows [row_offset, row_offset + A*G*G) of out [B][n_total][5+C]:
 * (sig(tx)+gx)*s, (sig(ty)+gy)*s, exp(tw)*aw, exp(th)*ah, sig(conf), sig(cls...) ; s = img_dim/G. */
int ay_yolo_decode(const float* head, int layout, float* out, int batch, int num_anchors, int num_classes,
                   int grid, int img_dim, const float* anchors_wh /* host, A*2, pixels */, int n_total,
                   int row_offset, ay_stream_t stream);
/* A detection head AND its decode in one launch (models.py:33-40 for the linear 1x1 head convolution 81 / 93 / 105, then
 * models.py:127-172): the head tensor never goes to memory, the convolution's epilogue writes rows [row_offset, row_offset + A*G*G)
 * of pred [B][n_total][5+C] -- the same bits ay_conv_fwd_bf16 (out_f32) + ay_yolo_decode produce.  d: ksize 1, stride 1, leaky 0,
 * cout = A*(5+C), cout_pad = cout rounded up to 32; scale = ones, shift = the bias (ay_fold_bn without BatchNorm). */
int ay_head_decode_fwd_bf16(const ay_conv_desc* d, const void* src_blocked_bf16, const void* w_packed, const float* scale,
                            const float* shift, int num_anchors, int num_classes, int img_dim,
                            const float* anchors_wh /* host, A*2, pixels */, float* pred, int n_total, int row_offset,
                            ay_stream_t stream);
int ay_head_decode_fwd_f16(const ay_conv_desc* d, const void* src_blocked_f16, const void* w_packed, const float* scale,
                           const float* shift, int num_anchors, int num_classes, int img_dim, const float* anchors_wh, float* pred,
                           int n_total, int row_offset, ay_stream_t stream);

/* ---- box math: utils/utils.py:53-59,193-232 ---------------------------------------------------- */
int ay_xywh2xyxy(float* boxes, int64_t n_rows, int row_stride, ay_stream_t stream); /* in place, first 4 cols */
/* mode 0: IoU with the reference's +1-pixel rule (bbox_iou); mode 1: GIoU (no +1; new, unpinned).
 * n1 == n2 (elementwise) or n1 == 1 (broadcast); xyxy=0 means (cx,cy,w,h) inputs. out[n2]. */
int ay_box_iou(const float* box1, int n1, const float* box2, int n2, int xyxy, int mode, float* out,
               ay_stream_t stream);
/* all pairs: out[n1][n2] */
int ay_box_iou_pairwise(const float* box1, int n1, const float* box2, int n2, int mode, float* out,
                        ay_stream_t stream);

/* ---- merge-NMS: utils/utils.py:235-273 ---------------------------------------------------------- */
/* pred [B][N][5+C] (cx,cy,w,h,conf,cls..) is converted to corners IN PLACE (reference :244).
 * Per image: rows with conf >= conf_thres, ordered by conf*max(cls) descending (ties: lower row first),
 * greedy class-aware suppression (IoU > nms_thres, strict) with confidence-weighted box merge.
 * out_rows [B][max_det][7] (x1,y1,x2,y2,conf,cls_conf,cls_pred), keep_idx [B][max_det] original row of
 * each emitted cluster head, count[B] (clamped to max_det), cand_count[B] candidates after the filter. */
size_t ay_nms_workspace_bytes(int batch, int n_rows);
/* step 1: corners in place + conf filter + sort keys -> cand_count[B] (lets the caller size max_det exactly) */
int ay_nms_filter(float* pred, int batch, int n_rows, int num_classes, float conf_thres, int32_t* cand_count,
                  void* workspace, size_t workspace_bytes, ay_stream_t stream);
/* step 2: per-image sort + greedy merge scan; pred must already hold corners (step 1) */
int ay_nms_sort_merge(const float* pred, int batch, int n_rows, int num_classes, float nms_thres, int max_det,
                      float* out_rows, int32_t* keep_idx, int32_t* count, const int32_t* cand_count,
                      void* workspace, size_t workspace_bytes, ay_stream_t stream);
/* both steps back to back, no host sync; count[b] > max_det tells the caller rows were dropped */
int ay_nms_merge(float* pred, int batch, int n_rows, int num_classes, float conf_thres, float nms_thres,
                 int max_det, float* out_rows, int32_t* keep_idx, int32_t* count, int32_t* cand_count,
                 void* workspace, size_t workspace_bytes, ay_stream_t stream);

/* ---- training step, fp32 reference-precision path (nchw f32) -------------------------------------- */

/* Train-mode BatchNorm2d + LeakyReLU forward (models.py:43-45): batch statistics over (B,H,W), biased variance for the
 * normalisation, running stats updated with PyTorch semantics running = (1-momentum)*running + momentum*batch
 * (unbiased variance), momentum = 0.9 in the reference.  z = raw conv output, y = block output.
 * n = B*H*W = 1 has no unbiased variance (n / (n - 1)): running_var then receives the BIASED variance, 0 (PyTorch refuses that
 * input in training mode).  Statistics are summed in fp64 and rounded to fp32 once (mean, invstd), so a channel mean far above
 * its spread does not cancel; a channel of constants has invstd = 1 / sqrt(eps). */
int ay_bn_train_fwd_f32(const float* z, const float* gamma, const float* beta, float* running_mean, float* running_var,
                        float momentum, float eps, int leaky, float* y, float* save_mean, float* save_invstd,
                        int batch, int channels, int hw, ay_stream_t stream);
/* its backward (autograd of the above): dy -> dz, dgamma, dbeta (written, not accumulated) */
int ay_bn_train_bwd_f32(const float* dy, const float* y, const float* z, const float* gamma, const float* save_mean,
                        const float* save_invstd, int leaky, float* dz, float* dgamma, float* dbeta, int batch,
                        int channels, int hw, ay_stream_t stream);
int ay_bias_grad_f32(const float* dz, float* dbias, int batch, int channels, int hw, ay_stream_t stream);
int ay_bias_grad_f32_acc(const float* dz, float* dbias, int accumulate, int batch, int channels, int hw, ay_stream_t stream);
/* autograd of nn.Conv2d (models.py:33-40): input gradient (optionally accumulated into dx) and weight gradient */
int ay_conv_dgrad_f32(const ay_conv_desc* d, const float* dz, const float* w_oihw, float* dx, int accumulate,
                      ay_stream_t stream);
int ay_conv_wgrad_f32(const ay_conv_desc* d, const float* x, const float* dz, float* dw, ay_stream_t stream);
/* shortcut add (models.py:246-248), gradient accumulation, route/upsample copy (models.py:86-96,244-245) and its backward */
int ay_add_f32(const float* a, const float* b, float* out, size_t n, ay_stream_t stream);
int ay_accumulate_f32(float* dst, const float* src, size_t n, ay_stream_t stream);
int ay_copy_channels_f32(const float* src, float* out, int batch, int csrc, int ctotal, int c0, int h, int w, int up,
                         ay_stream_t stream);
int ay_slice_accumulate_f32(const float* dout, float* dsrc, int batch, int csrc, int ctotal, int c0, int h, int w, int up,
                            ay_stream_t stream);
/* YOLO layer loss (models.py:174-222) with build_targets (utils/utils.py:276-330) fused: target assignment
 * (best-of-A anchor by wh-IoU, ignore threshold, last-writer-wins scatter in target order), the six loss terms and the
 * gradient w.r.t. the raw head tensor [B][A*(5+C)][G][G].  sums_out (device, 16 floats): [0..3] sum sq err x,y,w,h @obj,
 * [4] BCE conf @obj, [5] BCE conf @noobj, [6] BCE cls @obj, [7] n_obj, [8] n_noobj, [9] class hits, [10] sum conf @obj,
 * [11] sum conf @noobj, [12] #conf>0.5, [13] #(iou>0.5 & detected), [14] #(iou>0.75 & detected).
 * loss = (s0+s1+s2+s3)/n_obj + s4/n_obj + 100*s5/n_noobj + s6/(n_obj*C); dhead = grad_scale * dloss/dhead. */
size_t ay_yolo_loss_workspace_bytes(int batch, int num_anchors, int num_classes, int grid);
int ay_yolo_loss_fwd_bwd(const float* head_nchw, const float* targets, int n_targets, int batch, int num_anchors,
                         int num_classes, int grid, int img_dim, const float* anchors_wh /* host */, float ignore_thres,
                         float grad_scale, float* dhead, float* sums_out, void* workspace, size_t workspace_bytes,
                         ay_stream_t stream);
/* GIoU variant of the box term (BASELINE.json configs[4]; new feature, no reference counterpart): same call, same sums
 * layout, but sums[0] = sum over object cells of 1 - GIoU(decoded box, target box) (grid units, no +1 rule) and
 * sums[1..3] = 0; loss = s0/n_obj + s4/n_obj + 100*s5/n_noobj + s6/(n_obj*C). */
int ay_yolo_loss_giou_fwd_bwd(const float* head_nchw, const float* targets, int n_targets, int batch, int num_anchors,
                              int num_classes, int grid, int img_dim, const float* anchors_wh /* host */, float ignore_thres,
                              float grad_scale, float* dhead, float* sums_out, void* workspace, size_t workspace_bytes,
                              ay_stream_t stream);
/* utils/utils.py:276-330 build_targets on device, as the dense 10-tuple the reference returns (same order):
 * pred_boxes [B,A,G,G,4] cxcywh in grid units, pred_cls [B,A,G,G,C], targets [nT,6] (sample, class, cx, cy, w, h in [0,1]),
 * anchors_grid (HOST) [A,2] = anchors / stride (models.py:123).  Masks are bytes (0/1).  Duplicate (sample, anchor, cell)
 * targets: the last one in target order wins, classes accumulate (multi-hot), as on the reference's CPU path. */
size_t ay_build_targets_workspace_bytes(int batch, int num_anchors, int grid);
int ay_build_targets(const float* pred_boxes, const float* pred_cls, const float* targets, int n_targets, int batch,
                     int num_anchors, int num_classes, int grid, const float* anchors_grid /* host */, float ignore_thres,
                     float* iou_scores, float* class_mask, uint8_t* obj_mask, uint8_t* noobj_mask, float* tx, float* ty,
                     float* tw, float* th, float* tcls, float* tconf, void* workspace, size_t workspace_bytes,
                     ay_stream_t stream);
/* torch.optim.Adam step (train.py:81,118) on one flat buffer; grads are multiplied by grad_scale first (1/world size) */
int ay_adam_flat(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, size_t n, float lr, float beta1,
                 float beta2, float eps, int step, float grad_scale, ay_stream_t stream);

/* ---- evaluation statistics ------------------------------------------------------- */
/* Greedy true-positive matching of get_batch_statistics (utils/utils.py:154-190) for a batch: rows [B][max_det][7]
 * (x1,y1,x2,y2,conf,cls_conf,cls_pred, detections in descending-score order as non_max_suppression emits them), count[B],
 * targets [nT][6] = (sample, class, x1, y1, x2, y2) in pixels -> tp [B][max_det] (1.0 = true positive).  *overflow is set
 * to 1 if an image has more than 2048 targets (only the first 2048 are matched). */
int ay_match_detections(const float* rows, const int32_t* count, int batch, int max_det, const float* targets, int n_targets,
                        float iou_thres, float* tp, int32_t* overflow, ay_stream_t stream);

/* ---- tile ingest ----------------------------------------------------------------- */
/* uint8 HWC RGB tiles [B,H,W,3] -> float32 NCHW [B,3,S,S]: x/255 (utils/transforms.py:96), centre zero pad to square
 * (utils/datasets.py:22-32), nearest resize src = min(floor(dst * (float)in/out), in-1) (utils/datasets.py:35-37), one pass. */
int ay_ingest_tiles_u8(const void* img_hwc_u8, int batch, int h, int w, int out_size, float pad_value, float* out_nchw,
                       ay_stream_t stream);

/* WSI -> tile streaming (crop.py:13-25,44-47): tile t = (ty, tx) of the tile_size grid dzsave(layout='google')
 * lays over the slide, cut out of a resident uint8 HWC region (rows `row_stride_bytes` apart; region_h x region_w source pixels),
 * edge tiles padded with the background 255; shrink 2 = the 40x -> 20x halving first (2x2 mean, round half up; the grid then lies
 * on the region_h/2 x region_w/2 image); then x/255 and the nearest resize to out_size as in ay_ingest_tiles_u8.
 * out [tiles_y*tiles_x][3][out_size][out_size] fp32.  The three entry points below are ONE cut (one kernel, one pixel rule, the tile
 * origins computed or read from a list); this one is ay_ingest_region_tiles_step_u8 at step == tile: the same launch, the same stores. */
int ay_ingest_region_tiles_u8(const void* region_hwc_u8, int region_h, int region_w, size_t row_stride_bytes, int shrink,
                              int tile, int tiles_y, int tiles_x, int out_size, float* out_nchw, ay_stream_t stream);

/* The same with tile origins `step` apart: tile (ty, tx) starts at (ty * step, tx * step) on the (halved) image, 0 < step <= tile.
 * step < tile gives tiles that overlap by tile - step pixels (wsi.tile_grid, wsi.detect_region(overlap > 0)); step == tile is
 * ay_ingest_region_tiles_u8.  Stores 16 bytes per lane when out_size is a multiple of 4 and `out_nchw` is 16-byte aligned, 4 bytes
 * with the same bits otherwise. */
int ay_ingest_region_tiles_step_u8(const void* region_hwc_u8, int region_h, int region_w, size_t row_stride_bytes, int shrink,
                                   int tile, int step, int tiles_y, int tiles_x, int out_size, float* out_nchw, ay_stream_t stream);

/* The same cut for a LIST of n tile origins: origins_xy [n][2] int32 ON THE DEVICE = (x, y) of a tile's corner in pixels of the
 * (halved) region, any position (on a grid or not, repeated or not; what lies outside the region, also left of or above it, is the
 * background 255, for every int32 origin: origin + offset is formed without signed overflow and nothing outside the region is read)
 * -> out[0..n) densely, in list order; rows of `out` behind n are not touched.  The same kernel and the same stores as the step form,
 * only the origins are read: those of a full grid in grid order give ay_ingest_region_tiles_step_u8 bit for bit.
 * wsi.RegionTileStream(tile_mask=...) cuts only the wanted tiles of a strip with it. */
int ay_ingest_region_tiles_list_u8(const void* region_hwc_u8, int region_h, int region_w, size_t row_stride_bytes, int shrink,
                                   int tile, const int32_t* origins_xy, int n, int out_size, float* out_nchw, ay_stream_t stream);

/* ---- training augmentation fused into the ingest (amyloid_yolo_paper_amd/augment.py; csrc/ay_augment.hip) -------------------
 * The reference trains behind an imgaug pipeline (utils/augmentations.py: Dropout, Sharpen, Affine +-20 deg / +-20 %,
 * AddToBrightness, AddToHue, Fliplr).  imgaug cannot be installed where this project is built, so PARITY WITH IMGAUG IS UNPINNED:
 * the behaviour is defined by the rule below and restated in NumPy by tests/augment_reference.py.
 *
 * THE AUGMENTATION RULE (every operation IEEE fp32, in the order written, nothing fused).
 *   One record per image (ay_aug_params, device memory).  For output pixel (x, y) of the S x S image of a record (h, w, ...):
 *   1. Square pixel, the nearest rule of ay_ingest_tiles_u8 unchanged: D = max(h, w), scale = (float)D / (float)S,
 *        qx = min((int)floorf(x * scale), D - 1) - left,  qy = min((int)floorf(y * scale), D - 1) - top,
 *      left / top the centre-pad offsets of ay_ingest_tiles_u8 (h <= w: top = (w - h) / 2, left = 0; else left = (h - w) / 2).
 *   2. Flip: if flip, qx = w - 1 - qx (the reference flips last, so the inverse mapping flips first).
 *   3. Inverse affine about the image centre: cx = (float)(w - 1) / 2, cy = (float)(h - 1) / 2, xc = qx - cx, yc = qy - cy,
 *        sx = ((inv[0] * xc + inv[1] * yc) + inv[2]) + cx,  sy = ((inv[3] * xc + inv[4] * yc) + inv[5]) + cy.
 *   4. Bilinear sample of the uint8 source: x0 = floorf(sx), fx = sx - x0, the same for y; taps a, b, c, d at (y0, x0), (y0, x0+1),
 *      (y0+1, x0), (y0+1, x0+1) as floats in 0..255, a tap outside [0, h) x [0, w) is 0 (imgaug's cval = 0, and the pad value);
 *        t = a + fx * (b - a),  u = c + fx * (d - c),  W = t + fy * (u - t).
 *   5. Sharpen, on the warped S x S image W: ring = the sum of the 8 neighbours of W, indices clamped at the edge of the output
 *      image, summed rows top to bottom, left to right, centre skipped;  v = W + sharpen_alpha * (8 * W - ring).
 *   6. Dropout: idx = y * S + x; hsh = drop_seed ^ (idx * 0x9E3779B9); hsh ^= hsh >> 16; hsh *= 0x7feb352d; hsh ^= hsh >> 15;
 *      hsh *= 0x846ca68b; hsh ^= hsh >> 16 (all uint32); if hsh < drop_threshold, v = 0 in all three channels.
 *   7. Colour: o_k = ((color[3k] * v_r + color[3k+1] * v_g) + color[3k+2] * v_b) + bright.
 *   8. out = min(max(o, 0), 255) / 255.0f (evaluated as o > 0 ? o : 0, then o < 255 ? o : 255), fp32 NCHW.
 *   With inv = (1,0,0, 0,1,0), flip = 0, sharpen_alpha = 0, drop_threshold = 0, color = I, bright = 0 every step is exact and the
 *   output is bit-identical to ay_ingest_tiles_u8(pad_value = 0).
 *   Departures from the reference: sharpen and dropout act on the warped image at output resolution, not on the source; brightness
 *   is an additive offset on R, G and B; hue is a rotation about the grey axis handed over as the matrix `color` (the host computes
 *   it in float64; the device does no trigonometry and no HSV round trip); imgaug's kernels and colour spaces are not restated. */
typedef struct ay_aug_params {
    int64_t src_offset;            /* byte offset of the image [h][w][3] uint8 in the source buffer (a batch may be ragged) */
    int32_t h, w;
    float inv[6];                  /* output -> source, about the image centre: rows (inv0 inv1 inv2), (inv3 inv4 inv5) */
    int32_t flip;                  /* 0 | 1 */
    float sharpen_alpha;
    uint32_t drop_threshold;       /* floor(p * 2^32): a pixel is dropped iff its hash is below */
    uint32_t drop_seed;
    float color[9];                /* row-major 3 x 3 on (R, G, B) */
    float bright;                  /* added after the matrix, in 0..255 units */
} ay_aug_params;

/* src_u8: `src_bytes` bytes of device memory holding the images one after another; params_device [batch]; out [batch][3][S][S] fp32.
 * A record whose image does not lie inside [src_u8, src_u8 + src_bytes) (or with h, w <= 0) is treated as all padding: nothing
 * outside the buffer is read.  One kernel: a 256-thread workgroup warps a 16 x 64 block of output pixels plus a one-pixel halo into
 * LDS, then sharpens from there; 16-byte stores per lane when out_size is a multiple of 4 and `out_nchw` is 16-byte aligned, the
 * scalar form with the same bits otherwise.  batch <= 65535, out_size <= 32768.  Kernel launches only. */
int ay_augment_ingest_u8(const void* src_u8, size_t src_bytes, const ay_aug_params* params_device, int batch, int out_size,
                         float* out_nchw, ay_stream_t stream);

/* THE WINDOW RULE (training windows cut out of an annotated slide: wsi.SlideSampler), as a difference to THE AUGMENTATION RULE.
 *   One record per image (ay_aug_window_params).  The BLOCK is the bh x bw pixels that may be read: pixel (0, 0) at byte
 *   src_offset of the source buffer, rows row_stride bytes apart (>= 3 * bw, no multiple of anything).  The WINDOW is the h x w
 *   (aug.h, aug.w) pixels whose origin lies at block pixel (x0, y0), of any sign: it may leave the block on every side.
 *   Steps 1-3 and 5-8 are unchanged, with (h, w) the window.  Step 4 computes x0 = floorf(sx), y0 = floorf(sy), fx, fy and the tap
 *   positions (ty, tx) in WINDOW coordinates as before; the value of a tap is
 *     - if context == 0 and (ty, tx) lies outside [0, h) x [0, w): 0 (the tile rule);
 *     - else, with (by, bx) = (y0 + ty, x0 + tx) computed without overflow: the source byte of block pixel (by, bx) if it lies
 *       inside [0, bh) x [0, bw), otherwise `fill`.
 *   So with context == 1 a rotated or shifted window shows the real surroundings it has on the slide instead of black wedges, and
 *   `fill` (the slide's background) only beyond the block.
 *   Consequences:
 *     - context == 0, x0 == y0 == 0, bh == h, bw == w, row_stride == 3 * w: ay_augment_ingest_u8 bit for bit.
 *     - context == 0 and the window inside a larger block: ay_augment_ingest_u8 on the cut-out tile, bit for bit.
 *     - context == 1: the output depends on the block only through the pixels the taps touch; any sub-block that holds them (and
 *       has `fill` semantics beyond the same outer edge) gives the same bytes.
 *     - A block without pixels (bh <= 0 or bw <= 0) has every tap outside: `fill` (context == 1, or inside the window), else 0.
 *   Safety: a record with h, w <= 0, a negative src_offset or row_stride, or a block (with pixels) that does not lie inside
 *   [src_u8, src_u8 + src_bytes) -- src_offset + (bh - 1) * row_stride + 3 * bw <= src_bytes, evaluated without overflow --
 *   reads nothing and yields the all-padding image of ay_augment_ingest_u8 (W = 0).  Tap positions are clamped in block
 *   coordinates before any address is formed, so every float in `inv` (inf and NaN included) reads inside the block. */
typedef struct ay_aug_window_params {
    int64_t src_offset;            /* byte offset of block pixel (0, 0) in the source buffer */
    int64_t row_stride;            /* bytes between block rows */
    int32_t bh, bw;                /* the block: the pixels that may be read */
    int32_t x0, y0;                /* the window's origin in block pixels, of any sign */
    int32_t context;               /* 0: outside the window is 0 | 1: outside the window is the block, then `fill` */
    float fill;                    /* 0..255: the value of a tap outside the block */
    ay_aug_params aug;             /* h, w = the window's size; its src_offset is ignored */
} ay_aug_window_params;

/* ay_augment_ingest_u8 under THE WINDOW RULE: the same kernel body with another tap fetch, the same argument checks and limits. */
int ay_augment_ingest_window_u8(const void* src_u8, size_t src_bytes, const ay_aug_window_params* params_device, int batch,
                                int out_size, float* out_nchw, ay_stream_t stream);

/* ---- tissue map: which tiles of a slide are worth reading (wsi.tissue_counts, wsi.wanted_tiles; csrc/ay_tissue.hip) ------------
 * THE TISSUE RULE (exact, integer).
 *   A pixel of the (halved, for shrink == 2) image is TISSUE iff min(R, G, B) < bg_level on its uint8 values; for shrink == 2 the
 *   values are the 2x2 means with round-half-up of the ingest, (a + b + c + d + 2) >> 2.  bg_level is an int in [0, 256]: 0 makes
 *   nothing tissue, 256 everything.
 *   The TISSUE COUNT of tile (ty, tx) of a grid with origins `step` apart is the number of tissue pixels in
 *   [ty * step, ty * step + tile) x [tx * step, tx * step + tile) that lie inside the H x W image (H = region_h / shrink, W =
 *   region_w / shrink).  What lies outside is the ingest's 255 padding and never counts.  With step < tile a pixel in a shared band
 *   counts for every tile that contains it.
 *   A tile is WANTED iff count >= max(1, ceil(min_tissue * tile * tile)), the right-hand side computed once on the host
 *   (wsi.wanted_tiles).
 * ay_tile_tissue_u8 writes the counts [tiles_y * tiles_x] (int32, device; zeroed by a kernel of the call, not by the caller) of a
 * resident region; tile <= 46340, so that a count fits int32.  A pure read stream over the image: a source byte comes from memory
 * once, also where tiles overlap (neighbouring lanes and units re-read a few bytes through the cache); 16-byte loads per lane when
 * the base and row_stride_bytes are multiples of 16, byte loads (about three times slower, same counts) for any other alignment;
 * integer sums with one atomic per tile and workgroup: the same bits every run.  Kernel launches only. */
int ay_tile_tissue_u8(const void* region_hwc_u8, int region_h, int region_w, size_t row_stride_bytes, int shrink, int tile, int step,
                      int tiles_y, int tiles_x, int bg_level, int32_t* counts, ay_stream_t stream);

/* ---- training step, bf16 MFMA path (blocked bf16 activations and activation gradients) ------------- */

/* Train-mode BatchNorm + LeakyReLU (+ fused shortcut add of `skip`) around the MFMA convolution: statistics pass (fp64
 * atomics into sums_ws[2*C]), finalize (mean/invstd/running stats, PyTorch momentum semantics), apply pass -> y. */
int ay_bn_train_fwd_bf16(const void* z, const float* gamma, const float* beta, float* running_mean, float* running_var,
                         float momentum, float eps, int leaky, const void* skip, void* y, float* save_mean, float* save_invstd,
                         double* sums_ws, int batch, int channels, int h, int w, ay_stream_t stream);
/* dy (gradient of the block output, before the shortcut add) -> dz, dgamma, dbeta; leaky' is taken from the recomputed
 * pre-activation gamma*xhat+beta */
int ay_bn_train_bwd_bf16(const void* dy, const void* z, const float* gamma, const float* beta, const float* save_mean,
                         const float* save_invstd, int leaky, void* dz, float* dgamma, float* dbeta, double* sums_ws, int batch,
                         int channels, int h, int w, ay_stream_t stream);
/* The `_acc` forms with accumulate != 0 ADD the parameter gradients to what dgamma / dbeta / dw / dbias hold: the parameter
 * gradients of a step go straight into the caller's (flat) gradient buffer, also across the batches of a gradient
 * accumulation (train.py:116-119), instead of through per-layer temporaries and autograd's accumulation pass. */
int ay_bn_train_bwd_bf16_acc(const void* dy, const void* z, const float* gamma, const float* beta, const float* save_mean,
                             const float* save_invstd, int leaky, void* dz, float* dgamma, float* dbeta, double* sums_ws,
                             int accumulate, int batch, int channels, int h, int w, ay_stream_t stream);
/* The two BatchNorm calls for a caller that has CLEARED sums_ws itself (fp64 zeros on entry): a training step of Darknet-53
 * zeroes the workspaces of all 72 layers and both passes with one memset instead of 144 small fill launches.  Otherwise
 * identical to ay_bn_train_fwd_bf16 / ay_bn_train_bwd_bf16_acc (models.py:43 train-mode semantics and its backward). */
int ay_bn_train_fwd_bf16_zeroed_ws(const void* z, const float* gamma, const float* beta, float* running_mean, float* running_var,
                                   float momentum, float eps, int leaky, const void* skip, void* y, float* save_mean, float* save_invstd,
                                   double* sums_ws_zeroed, int batch, int channels, int h, int w, ay_stream_t stream);
int ay_bn_train_bwd_bf16_acc_zeroed_ws(const void* dy, const void* z, const float* gamma, const float* beta, const float* save_mean,
                                       const float* save_invstd, int leaky, void* dz, float* dgamma, float* dbeta, double* sums_ws_zeroed,
                                       int accumulate, int batch, int channels, int h, int w, ay_stream_t stream);
int ay_accumulate_bf16(void* dst, const void* src, size_t n_elems, ay_stream_t stream);
/* route / nearest-upsample backward on blocked tensors (channel counts multiples of 16) */
int ay_slice_accumulate_bf16(const void* dout, void* dsrc, int batch, int csrc, int ctotal, int c0, int h, int w, int up,
                             int accumulate, ay_stream_t stream);
/* stride-2 data gradient = stride-1 convolution of the zero-inserted output gradient: out[2y][2x] = in[y][x] */
int ay_zero_insert_bf16(const void* in, void* out, int batch, int channels, int h, int w, int ho, int wo, ay_stream_t stream);
/* filters that make ay_conv_fwd_bf16 compute the data gradient: W'[ci][co][kh][kw] = W[co][ci][k-1-kh][k-1-kw], packed
 * [ceil(cout/16)][k*k][2][cin_pad][8]; use with desc{cin=ceil16(cout), cout=cin, cout_pad=cin_pad, stride 1}. */
int ay_pack_dgrad_weights_bf16(const float* w_oihw, void* packed, int cout, int cin, int cin_pad, int ksize, ay_stream_t stream);
size_t ay_packed_dgrad_weight_bytes(int cout, int cin_pad, int ksize);
/* Every filter image a training step needs, re-packed in ONE launch after the optimiser moved the weights (the reference has no
 * counterpart: its convolutions read nn.Conv2d.weight directly; this replaces ~145 ay_pack_*_bf16 launches per step).  `jobs` and
 * `work` live in DEVICE memory and are built once per weight layout: job j packs `total` elements of image kind `kind` (0 =
 * ay_pack_conv_weights_bf16, `cin` = channels of the source tensor; 1 = ay_pack_dgrad_weights_bf16; 2 =
 * ay_pack_dgrad_s2_weights_bf16) exactly as the single calls do; work item w = (job, first_block) covers elements
 * [first_block * ay_pack_batch_block(), +ay_pack_batch_block()) of that job. */
typedef struct ay_pack_job {
    const float* src;
    void* dst;
    int32_t kind, cout, cout_pad, cin, cin_pad, ksize;
    uint64_t total;
} ay_pack_job;
typedef struct ay_pack_work {
    uint32_t job, first_block;
} ay_pack_work;
int ay_pack_batch_block(void);
int ay_pack_batch_bf16(const void* jobs_device, const void* work_device, int n_work, ay_stream_t stream);
/* The stem Conv2d(3, 32, 3, 1, 1) (models.py:33-41, layer 0) on the bf16 training path, straight from the fp32 NCHW image (W % 4 == 0,
 * 16-byte aligned): forward z = bf16(conv(bf16(x), bf16(w))) with fp32 accumulation -> blocked bf16 [B][2][H][W][16]
 * (w_bf16: [32][32] bf16, index ci*9 + kh*3 + kw, entries 27..31 unused), and the filter gradient dW[32][3][3][3] (fp32,
 * overwritten or, accumulate != 0, added to) from the blocked bf16 output gradient; partial sums per workgroup go to
 * `workspace` (ay_stem_train_wgrad_workspace_bytes()) and are added in a fixed order.  What loss.backward() (train.py:113)
 * computes for that layer, on bf16-rounded operands. */
int ay_stem_train_fwd_bf16(const float* x_nchw, const void* w_bf16, void* z_blocked, int batch, int h, int w, ay_stream_t stream);
/* ... and the layer's BatchNorm batch statistics gathered where z is produced ("stats reduce fused with the conv
 * epilogue"): sums[0..31] = sum z, sums[32..63] = sum z^2 over the batch (of the bf16-rounded values, fp64, fixed summation order), to
 * be followed by ay_bn_train_apply_bf16 -- ay_bn_train_fwd_bf16 without its statistics pass. */
size_t ay_stem_train_stats_workspace_bytes(void);
int ay_stem_train_fwd_stats_bf16(const float* x_nchw, const void* w_bf16, void* z_blocked, double* sums, void* workspace, size_t workspace_bytes,
                                 int batch, int h, int w, ay_stream_t stream);
int ay_bn_train_apply_bf16(const void* z, const float* gamma, const float* beta, float* running_mean, float* running_var, float momentum,
                           float eps, int leaky, const void* skip, void* y, float* save_mean, float* save_invstd, const double* sums_ws,
                           int batch, int channels, int h, int w, ay_stream_t stream);
size_t ay_stem_train_wgrad_workspace_bytes(void);
int ay_stem_train_wgrad_bf16(const float* x_nchw, const void* dz_blocked, float* dw_oihw, int accumulate, void* workspace,
                             size_t workspace_bytes, int batch, int h, int w, ay_stream_t stream);
/* Data gradient of a 3x3 stride-2 convolution (the reference gets it from autograd: loss.backward(), train.py:113, through
 * nn.Conv2d(stride=2), models.py:33-41) WITHOUT zero insertion: output pixel (y, x) only receives the filter taps with
 * (y + 1 - kh) and (x + 1 - kw) even, so each parity class (y & 1, x & 1) of dx is a stride-1 convolution of dz with a
 * 2x2 window of 1, 2, 2 or 4 live taps -- 16 tap slots per dz pixel instead of the 36 of the zero-inserted form, and dz is
 * read at its own (quarter) size.  `d` is the FORWARD convolution's descriptor (ksize 3, stride 2, even hin/win; cout_pad =
 * channels of dz's planes); dx has cin_pad (multiple of 32) channel planes of hin x win; residual (may alias dx) is
 * added before the bf16 rounding; ones / zeros: cin_pad floats of 1 / 0 (the kernel's affine epilogue).
 * Filters from ay_pack_dgrad_s2_weights_bf16: [class py*2+px][cout_pad/16][window tap][2][cin_pad][8] bf16. */
size_t ay_packed_dgrad_s2_weight_bytes(int cout_pad, int cin_pad);
int ay_pack_dgrad_s2_weights_bf16(const float* w_oihw, void* packed, int cout, int cout_pad, int cin, int cin_pad, ay_stream_t stream);
int ay_conv_dgrad_s2_bf16(const ay_conv_desc* d, const void* dz, const void* w_s2_packed, const float* ones, const float* zeros,
                          const void* residual, void* dx, int cin_pad, ay_stream_t stream);
/* weight gradient on the MFMA path: dW (OIHW fp32, overwritten) from blocked bf16 input x and output gradient dz
 * (desc as in the forward; cout_pad = channels of dz's planes) */
int ay_conv_wgrad_bf16(const ay_conv_desc* d, const void* x_blocked, const void* dz_blocked, float* dw_oihw, ay_stream_t stream);
int ay_conv_wgrad_bf16_acc(const ay_conv_desc* d, const void* x_blocked, const void* dz_blocked, float* dw_oihw, int accumulate,
                           ay_stream_t stream);
/* The same with a caller-owned workspace of ay_conv_wgrad_workspace_bytes(d) bytes: the split-K partial filters are written to
 * slabs and summed in a fixed order by a second small kernel -- bit-identical results from run to run, and faster than the
 * fp32 atomics of the forms above (which remain for callers without a workspace; a too small workspace falls back to them). */
size_t ay_conv_wgrad_workspace_bytes(const ay_conv_desc* d);
int ay_conv_wgrad_bf16_ws(const ay_conv_desc* d, const void* x_blocked, const void* dz_blocked, float* dw_oihw, int accumulate,
                          void* workspace, size_t workspace_bytes, ay_stream_t stream);

/* ---- inference plan: Darknet.forward (models.py:237-255) lowered to a flat op list ------------------------------
 * The host lowers the cfg graph once (which layers fuse, which routes fold into a loader) and hands the ops over; the
 * library lays the layer outputs ("values") out in ONE caller-allocated workspace -- a value's bytes are reused once its
 * last reader has been issued (first-fit over lifetimes; everything is stream-ordered) -- and ay_plan_forward issues the
 * whole network: one C call per batch instead of ~85.  Weight/scale/shift pointers are device memory owned by the caller
 * and must outlive the plan.  src/res/dst are value ids (0 .. n_values-1); AY_PLAN_INPUT names the network input. */
#define AY_PLAN_INPUT (-1)
#define AY_PLAN_NONE (-2)
enum {
    AY_OP_STEM_S2_FUSED = 1, /* ay_stem_s2_fused_fwd: input -> dst; w = stem filters bf16, w2 = packed layer-1 filters */
    AY_OP_STEM = 2,          /* ay_stem_conv_fwd: input -> dst; w = OIHW fp32 filters */
    AY_OP_CONV = 3,          /* ay_conv_fwd_bf16: src (+ res) -> dst */
    AY_OP_RESBLOCK = 4,      /* ay_resblock_fwd_bf16: src -> dst; (w, scale, shift, conv.leaky) = 1x1, (w2, ..2, leaky2) = 3x3 */
    AY_OP_CONV1X1_CAT = 5,   /* ay_conv1x1_cat_fwd_bf16: src = half-resolution source (c1 channels), src2 = direct source */
    AY_OP_CONCAT_UPSAMPLE = 6, /* ay_concat_upsample_bf16: src (c1 channels, up1) [+ src2 (c2 channels)] -> dst, conv.hout x wout */
    AY_OP_DECODE = 7         /* ay_yolo_decode of a blocked-f32 head: src -> rows [row_offset, ..) of the output */
};
typedef struct ay_plan_op {
    int32_t kind;
    int32_t src, src2, res, dst;   /* value ids; AY_PLAN_NONE where unused */
    ay_conv_desc conv;             /* shapes (all kinds use batch/hout/wout; RESBLOCK: cin = channels) */
    int32_t c1, c2, up1;           /* CONV1X1_CAT: c1; CONCAT_UPSAMPLE: c1, c2, up1 */
    int32_t leaky2;                /* STEM_S2_FUSED / RESBLOCK: activation of the second convolution */
    int32_t num_anchors, num_classes, grid, row_offset; /* DECODE */
    float anchors_wh[12];          /* DECODE: up to 6 anchors (w,h) in pixels */
    const void* w;
    const float* scale;
    const float* shift;
    const void* w2;
    const float* scale2;
    const float* shift2;
} ay_plan_op;
typedef struct ay_plan ay_plan;
/* value_bytes[i] = size of value i.  Fails (AY_ERR_ARG) on a value read before it is written or never written.
 * act_dtype: AY_DT_BF16 | AY_DT_F16 -- the storage type of the blocked activations and of every packed filter image in `ops`
 * (the plan then issues the _bf16 or the _f16 entry points). */
int ay_plan_create(const ay_plan_op* ops, int n_ops, const size_t* value_bytes, int n_values, int img_dim, int n_total_rows,
                   int act_dtype, ay_plan** out_plan);
void ay_plan_destroy(ay_plan* plan);
size_t ay_plan_workspace_bytes(const ay_plan* plan);       /* 256-byte aligned arena the caller allocates */
size_t ay_plan_value_offset(const ay_plan* plan, int value); /* where a value lives in the arena (tests) */
/* Traversal directions.  Off (as created): every launch walks its items upward.  On: each persistent convolution launch walks
 * opposite to the launch that last touched (wrote or read) the largest value it reads (the first one, which reads the image, forward), so that it starts
 * on the lines its producer wrote last, while they are still in the Infinity Cache.  The results do not depend on it, bit for bit.
 * Takes effect with the next ay_plan_forward (a captured forward keeps the directions it was captured with).
 * ay_plan_op_reversed: 1 if op `op` of the plan is issued reversed (0 with alternation off). */
int ay_plan_set_alternation(ay_plan* plan, int on);
int ay_plan_op_reversed(const ay_plan* plan, int op);
/* x: [B][3][S][S] fp32 NCHW; out_rows: [B][n_total_rows][5+C] fp32.  Stream-ordered, no host synchronisation. */
int ay_plan_forward(const ay_plan* plan, const float* x_nchw, void* workspace, float* out_rows, ay_stream_t stream);
/* Profiling without a host synchronisation inside the measured region: between begin and end every ay_plan_forward records
 * an event pair around each selected op (op_selected[n_ops] of 0/1, NULL = all; an event record costs the stream a few
 * microseconds), on the stream it issues to; end waits for them and returns, per op, the time summed over the recorded
 * forwards (0 for unselected ops).  A plan is driven by one host thread at a time. */
int ay_plan_profile_begin(ay_plan* plan, const unsigned char* op_selected);
/* the same with event pairs on every `every`-th forward only (the first one included): 62 event records cost a 24-ms step 0.17 ms;
 * ay_plan_profile_end then returns the number of forwards that were RECORDED */
int ay_plan_profile_begin_every(ay_plan* plan, const unsigned char* op_selected, int every);
int ay_plan_profile_end(ay_plan* plan, float* op_ms_sum /* n_ops */, int* n_forwards);
/* one forward with a HIP event pair around every op on `stream`; synchronises the stream and fills op_ms[n_ops] */
int ay_plan_forward_timed(const ay_plan* plan, const float* x_nchw, void* workspace, float* out_rows, float* op_ms,
                          ay_stream_t stream);

/* ---- union-merge of overlapping same-class detections (core.py:366-423 mergeDetections, :326-364) ----------
 * rows [batch][max_rows][7] = (x1, y1, x2, y2, conf, cls_conf, cls_pred) as ay_nms_merge leaves them (after rescaling), count[batch]
 * valid rows per image -> rows_out [batch][max_rows][7], count_out[batch]: pairs of rows of class 0 or 1 whose truncated integer pixel
 * rectangles share a pixel are replaced by the rectangle of the covered pixels (min of the confidences), pass after pass until
 * nothing changes, exactly as the reference does -- with the pair order the reference leaves to a Python set made explicit: rows
 * in input order, merged rows appended.  One wavefront per image, rows in LDS; max_rows <= ay_merge_detections_max_rows().
 * count[b] is clamped to [0, max_rows] (ay_nms_merge counts every kept row, also those it had no room for); rows behind count[b]
 * are not read.  Image b's rows lie at b * max_rows * 7 in both buffers; the rows of rows_out behind count_out[b] are NOT written
 * (a caller that wants zeros there clears the buffer first).  Rows and order are exact -- input values are copied, sign of zero
 * included, the label of a merged row is that of the lower-index row of the pair -- as long as every coordinate stays below 2^24 px:
 * a merged corner is an integer stored as float.  Identical rows collapse to the first; +0.0 and -0.0 are the same value.
 * Returns -1 (and launches nothing) for a null pointer, batch <= 0, max_rows outside 1 .. ay_merge_detections_max_rows() or
 * rows == rows_out. */
int ay_merge_detections_max_rows(void);
int ay_merge_detections(const float* rows, const int* count, int batch, int max_rows, float* rows_out, int* count_out,
                        ay_stream_t stream);

/* ---- slide-level seam merge for overlapping tiles (wsi.detect_region(overlap > 0); csrc/ay_seam.hip) --------------------------
 * THE RULE.  Input: rows [M][7] fp32 (x1, y1, x2, y2, conf, cls_conf, cls_pred) in slide pixels and tile_id [M] int32.  Output: a keep
 * flag per row and the number kept; rows are never altered, so the result is a subset of the input, bit for bit.
 *   score_i = conf_i * cls_conf_i (one fp32 multiply).  Rank: i comes before j iff score_i > score_j, or the scores are equal and i < j.
 *   ov(i, j) = inter / min(area_i, area_j) in fp32 with the +1 pixel convention of bbox_iou(x1y1x2y2=True):
 *   iw = min(x2_i, x2_j) - max(x1_i, x1_j) + 1, likewise ih, both clamped at 0, inter = iw * ih, area = (x2 - x1 + 1) * (y2 - y1 + 1),
 *   no fused multiply-add.  Intersection over the SMALLER box, not IoU: the second sighting of an object is often a truncated box.
 *   Walk the rows in rank order: row i is dropped iff some row j that ranks before it AND WAS KEPT has the same cls_pred, a different
 *   tile_id and ov(i, j) > seam_thres; otherwise it is kept (exact greedy suppression: a row whose only stronger partner was itself
 *   dropped is kept).  Rows of one tile never suppress each other.
 *
 * ay_seam_append: what ay_nms_merge leaves on the device for one batch (rows [batch][max_det][7], count [batch]) -> the valid rows of
 * image b, moved to slide coordinates v = fl32(fl32(v * scale) + origin) (origins_xy [batch][2] fp32 = (x, y) of the tile's corner, on
 * the device), appended with tile_ids[b] (device) behind the slide_count[0] rows the slide buffer holds.  Rows land in image order and,
 * within an image, in NMS output order (one ordered prefix over count).  slide_count is int32[2] on the device, zeroed by the caller
 * before the first append: [0] rows held, [1] AY_SEAM_FLAG_* bits.  An image with count > max_det contributes its first max_det rows
 * and sets AY_SEAM_FLAG_MAX_DET; rows past `capacity` are not written and set AY_SEAM_FLAG_CAPACITY.  Kernel launches only, no host
 * synchronisation; issue it on the stream of the NMS whose buffers it reads. */
#define AY_SEAM_FLAG_MAX_DET 1
#define AY_SEAM_FLAG_CAPACITY 2
int ay_seam_append(const float* rows, const int32_t* count, int batch, int max_det, float scale, const float* origins_xy,
                   const int32_t* tile_ids, float* slide_rows, int32_t* slide_tile, int32_t* slide_count, int capacity,
                   ay_stream_t stream);
/* ay_seam_merge applies the rule to n_rows rows: keep [n_rows] uint8 (1 = kept), stats int32[2] on the device = (rows kept, round
 * launches taken).  Work scales with the number of neighbouring pairs (rows binned by cell, cell side from the data, boxes larger than
 * a cell tested against everything).  Runs once per slide and SYNCHRONISES `stream` with the host (the cell side, and a "rows still
 * undecided" word every few rounds; the number of rounds is the longest chain of suppressions and is not capped): not for graph
 * capture.  workspace: 16-byte aligned, ay_seam_merge_workspace_bytes(n_rows) bytes.  Two runs on one input give the same bytes. */
size_t ay_seam_merge_workspace_bytes(int n_rows);
int ay_seam_merge(const float* slide_rows, const int32_t* slide_tile, int n_rows, float seam_thres, uint8_t* keep, int32_t* stats,
                  void* workspace, size_t workspace_bytes, ay_stream_t stream);

/* ---- dihedral test-time views (wsi.detect_region(views=...), amyloid_yolo_paper_amd/views.py; csrc/ay_views.hip) ----------------
 * Plaques have no orientation: a tile can be run in several of the 8 orientations of the square, the boxes mapped back and merged,
 * and a detection kept only if enough orientations support it.  Both rules are exact and restated in NumPy by
 * tests/views_reference.py.
 *
 * THE VIEW RULE.  A view id v is in 0 .. 7 with FX = v & 1, FY = (v >> 1) & 1, T = (v >> 2) & 1.  Let I0 be the S x S image that
 *   ay_ingest_region_tiles_list_u8 produces for a tile origin.  View v of that tile is defined on the OUTPUT grid, after the nearest
 *   resize, so it is a pure permutation of I0's bits:
 *     out_v[c][y][x] = I0[c][sy][sx],  (a, b) = T ? (y, x) : (x, y),  sx = FX ? S-1-a : a,  sy = FY ? S-1-b : b.
 *   View 0 is I0; in torch terms: flip I0 along x and / or y, then transpose if T.
 *   A decoded row (cx, cy, w, h, conf, cls...) of view v goes back to the frame of I0 in fp32, one operation each:
 *     (a, b) = T ? (cy, cx) : (cx, cy),  X = FX ? (float)S - a : a,  Y = FY ? (float)S - b : b,  (W, H) = T ? (h, w) : (w, h);
 *   confidence and class scores are copied untouched.  (In the decode pixel x covers [x, x+1): hence S - a, not S-1-a.)
 *
 * THE VOTE RULE.  After the merge-NMS over the concatenated rows of all views of a tile (n_views * N rows per image, view j of the list
 *   in rows [j*N, (j+1)*N)), `pred` holds corners in place.  View j votes for emitted detection d of image b iff some row r of that
 *   range satisfies all of: conf >= conf_thres; its arg-max class (first maximum) equals (int)rows[d][6]; its IoU with rows[d][0:4] is
 *   strictly greater than vote_thres -- the +1-pixel IoU in the operation order of ay_box_iou mode 0 on corners.  votes[b][d] is the bit
 *   mask over j; entries at or behind min(count[b], max_det) are 0.  The result does not depend on any order.
 *
 * ay_ingest_region_tiles_views_u8: the list cut in n_views views; `views` is a HOST array of 1 .. 8 distinct ids (else AY_ERR_ARG),
 *   origins_xy [n][2] on the device with the list form's semantics, out [n][n_views][3][S][S] fp32, TILE-major.  views = {0} gives
 *   ay_ingest_region_tiles_list_u8 bit for bit (the pixel rule is the one function both kernels call).  A workgroup computes a 32 x 32
 *   block of I0 once, holds it in LDS (rows padded to 33
 *   floats) and stores it into every view from there, row-contiguously also for the transposed views: the slide bytes are fetched
 *   once for all views.  16-byte stores per lane when out_size is a multiple of 4 and `out_nchw` is 16-byte aligned, the scalar form
 *   with the same bits otherwise.
 * ay_unview_rows: the box rule, in place on pred [n_images][n_rows][5 + num_classes], image i in view views[i % n_views] (host array).
 *   Runs behind the forward and BEFORE ay_nms_filter / ay_nms_merge (it needs cx, cy, w, h); pred seen as [n_images / n_views][n_views *
 *   n_rows][5 + C] is then the per-tile concatenation, without a copy.
 * ay_view_votes: the vote rule; votes int32 [batch][max_det], zeroed by a kernel of the call; integer OR atomics, the same bits every
 *   run.
 * ay_view_select: per image a stable in-place compaction of the rows (and of keep_idx, which may be null) whose vote mask has at least
 *   min_views bits set; count[b] becomes the number kept, but an image with count[b] > max_det keeps its count (its first max_det rows
 *   are compacted), so that the caller's overflow check still fires.  `votes` is left as it is.
 * All four: kernel launches only, no scratch. */
int ay_ingest_region_tiles_views_u8(const void* region_hwc_u8, int region_h, int region_w, size_t row_stride_bytes, int shrink,
                                    int tile, const int32_t* origins_xy, int n, const int* views, int n_views, int out_size,
                                    float* out_nchw, ay_stream_t stream);
int ay_unview_rows(float* pred, int n_images, const int* views, int n_views, int n_rows, int num_classes, int img_dim,
                   ay_stream_t stream);
int ay_view_votes(const float* pred, int batch, int n_views, int n_rows_per_view, int num_classes, float conf_thres, float vote_thres,
                  const float* rows, const int32_t* count, int max_det, int32_t* votes, ay_stream_t stream);
int ay_view_select(float* rows, int32_t* keep_idx, int32_t* count, const int32_t* votes, int batch, int max_det, int min_views,
                   ay_stream_t stream);

/* ---- slide-level evaluation: detections of a whole slide against its annotations (stats.match_slide; csrc/ay_slidematch.hip) ------
 * The true-positive rule of get_batch_statistics (utils/utils.py:154-190) for one image of any size.  ay_match_detections walks an
 * image's detections with one wavefront and holds 2048 targets; a slide has 10^4 .. 10^5 annotated objects and a few 10^5 rows.
 *
 * THE SLIDE MATCH RULE.  Input: rows [M][7] fp32 (x1, y1, x2, y2, conf, cls_conf, cls_pred) and targets [T][5] fp32 (class, x1, y1, x2,
 *   y2), both in slide pixels; K thresholds with 0 < thr_k <= 1, 1 <= K <= AY_SLIDE_MAX_THRES; optionally a region of interest
 *   roi = (rx1, ry1, rx2, ry2).  tests/slide_match_reference.py restates the rule in NumPy as the reference writes it.
 *   ROI: a row or target is IGNORED iff a roi is given and its centre (fl32((x1 + x2) * 0.5f), fl32((y1 + y2) * 0.5f)) lies outside
 *     the closed rectangle.  Ignored rows and targets take no part, as if deleted before the rule ran; indices in all outputs still
 *     refer to the original arrays.
 *   Rank (the seam rule's): score_i = conf_i * cls_conf_i, one fp32 multiply; row i comes before j iff score_i > score_j, or the
 *     scores are equal and i < j.  A NaN or negative score is a caller error (the result is then unspecified, but in bounds); so is
 *     a coordinate that is not finite.
 *   IoU: iou_p1 of csrc/ay_box.h exactly: +1 pixel convention, inter / (a1 + a2 - inter + 1e-16f), fp32, no fused multiply-add.
 *   Best target: for a non-ignored row, best_target is the lowest-index non-ignored target among those with the largest IoU (torch's
 *     first maximum) and best_iou that value; if no target has a positive IoU, best_target = -1 and best_iou = 0 (thr > 0: this never
 *     changes a flag).  Ignored rows get -1 and 0.
 *   Eligibility: a row is eligible at k iff it is not ignored, its cls_pred equals the class of at least one non-ignored target (the
 *     reference's `pred_label not in target_labels`) and best_iou >= thr_k.  As in the reference, the row's label is NOT compared
 *     with the label of its best target: a row whose best target has another class still claims it.
 *   Claim and flags: claim[k][g] is the first eligible-at-k row in rank order whose best_target is g, or -1;
 *     tp[k][i] = 1 iff claim[k][best_target_i] == i.  This equals the reference's sequential walk in rank order with its claimed set,
 *     including the early exit once every target is claimed: a row's candidate is its own first maximum whatever earlier rows did,
 *     so the walk is an argmax per row and a minimum per target.
 *   The result is exact for any box sizes, has no cap on M or T other than int32 and memory, and is the same bytes on every run.
 *   Classes are integers in 0 .. AY_SLIDE_MAX_CLASSES - 1 (class presence is a flag array on the device): a non-ignored target with
 *     another class value sets AY_SLIDE_FLAG_CLASS and matches no label; a row with such a cls_pred is simply never eligible.
 *
 * ay_slide_match: rows, targets and every output on the device; iou_thres (n_thres floats) and roi (4 floats, or NULL) on the HOST.
 *   tp uint8 [n_thres][n_rows], best_iou fp32 [n_rows], best_target int32 [n_rows], claim int32 [n_thres][n_targets], row_ignored uint8
 *   [n_rows], target_ignored uint8 [n_targets], stats int32 [2 * n_thres + 2] = per k (rows eligible at k, targets claimed at k), then
 *   AY_SLIDE_FLAG_* bits, then the number of targets on the oversize list.  n_rows == 0 or n_targets == 0 is legal (every flag 0, every
 *   claim -1; arrays of length 0 may be NULL).  The non-ignored targets are binned by the cell of their centre; a target larger than a
 *   cell goes to an oversize list that every row tests in full.  cell_side <= 0: the side comes from the targets (a reduction, read by
 *   the host); cell_side >= 2: that side.  Either way it is doubled until the grid over the targets' extent stays bounded, and the
 *   result does not depend on it.  With n_targets > 0 the call SYNCHRONISES `stream` with the host once (the grid): not for graph
 *   capture.  workspace: 16-byte aligned, ay_slide_match_workspace_bytes(n_rows, n_targets, n_thres) bytes.  No scratch. */
#define AY_SLIDE_MAX_THRES 16
#define AY_SLIDE_MAX_CLASSES 4096
#define AY_SLIDE_FLAG_CLASS 1
size_t ay_slide_match_workspace_bytes(int n_rows, int n_targets, int n_thres);
int ay_slide_match(const float* rows, int n_rows, const float* targets, int n_targets, const float* iou_thres, int n_thres,
                   const float* roi, float cell_side, uint8_t* tp, float* best_iou, int32_t* best_target, int32_t* claim,
                   uint8_t* row_ignored, uint8_t* target_ignored, int32_t* stats, void* workspace, size_t workspace_bytes,
                   ay_stream_t stream);

/* ---- slide-level burden: class count maps and the densest fields (wsi.burden_map, wsi.densest_fields, wsi.quantify_region;
 *      csrc/ay_burden.hip) ------------------------------------------------------------------------------------------------------------
 * What a slide's detections are for: how many objects of every class it carries per area of tissue, and how dense the densest
 * microscope-sized field is.  Both rules are exact (two fp32 operations, integers after them) and tests/burden_reference.py restates
 * them in NumPy.
 *
 * THE BURDEN RULE.  Input: rows [M][7] fp32 (x1, y1, x2, y2, conf, cls_conf, cls_pred) in pixels of the (halved) slide, the slide's
 *   H, W >= 1, an integer cell >= 1 (pixels), C classes with 1 <= C <= AY_BURDEN_MAX_CLASSES, and min_conf.
 *   Grid: Gy = ceil(H / cell), Gx = ceil(W / cell): wsi.tile_grid(H, W, cell, 0), the grid ay_tile_tissue_u8 counts on with tile = step
 *     = cell.
 *   For each row, in this order:
 *   Centre: cx = fl32((x1 + x2) * 0.5f), cy = fl32((y1 + y2) * 0.5f): the slide-match rule's two fp32 operations, no fused multiply-add.
 *   Flagged: a row whose cx or cy is not finite sets AY_BURDEN_FLAG_NONFINITE; a row whose cls_pred is not an integer value in
 *     0 .. C - 1 (a NaN included) sets AY_BURDEN_FLAG_CLASS.  A row that sets a bit is FLAGGED and counts nowhere.
 *   Below: any other row with !(conf >= min_conf) is BELOW and counts nowhere; a NaN confidence is therefore below.
 *   Counted: any other row counts once: px = (int)floorf(min(max(cx, 0), W - 1)) (W - 1 as fp32; and at most W - 1 on integers,
 *     which only matters above 2^24), py alike -- a centre outside the slide goes to the nearest border cell, nothing is lost --
 *     ix = px / cell, iy = py / cell (integer division), counts[c][iy][ix] += 1.
 *   Output: counts int32 [C][Gy][Gx] and stats int32 [C + 3] = rows counted per class, rows below, rows flagged, AY_BURDEN_FLAG_* bits.
 *     counts[c].sum() == stats[c], and sum(stats[:C]) + below + flagged == M.
 *
 * THE FIELD RULE.  Input: counts [C][Gy][Gx] (non-negative); optionally tissue int32 [Gy][Gx], the tissue pixels of every cell;
 *   field = F >= 1 cells per side with F * cell <= 46340, so that a field's tissue sum fits int32 (THE TISSUE RULE's bound);
 *   need_tissue >= 0; top_k = K, 1 <= K <= AY_BURDEN_MAX_FIELDS.
 *   Fields: the F x F blocks of cells that lie entirely inside the grid: field (fy, fx), 0 <= fy <= Gy - F, 0 <= fx <= Gx - F, has the
 *     linear index fy * (Gx - F + 1) + fx; there is none if Gy < F or Gx < F.  n_c(f) is the sum of counts[c] over the field's
 *     cells, t(f) the sum of tissue.  A field is ELIGIBLE iff tissue is NULL or t(f) >= need_tissue.
 *   Selection, for every class on its own, for up to K rounds: among the eligible fields that overlap no field already picked for
 *     this class (|fy - py| < F and |fx - px| < F is an overlap) take the largest n_c, ties to the lowest linear index; stop if there
 *     is no such field or that largest count is 0.
 *   Output: fields int32 [C][K][4] = (fy, fx, n, t) in pick order, rows not filled hold -1, -1, -1, -1, t is 0 when tissue is NULL;
 *     n_found int32 [C].  Integers, max and min only: a function of the inputs alone, the same bytes on every run.
 *
 * ay_burden_bin, ay_field_select: everything on the device.  Both are kernel launches only -- no memset node, no allocation, no host
 *   read -- and can sit in a captured step.  A kernel of the call zeroes counts and stats and fills fields with -1.  n_rows == 0 is
 *   legal (rows may then be NULL).  ay_field_select does not know the cell side: it refuses field > 46340, and the caller who knows
 *   both keeps field * cell <= 46340 (wsi.quantify_region does).  The field sums are separable (a row pass of F, a column pass of F,
 *   over the C count planes and the tissue plane, into the workspace); one workgroup per class runs the rounds.  workspace: 16-byte
 *   aligned, ay_field_select_workspace_bytes(num_classes, gy, gx, field) bytes (0 for arguments the call refuses).  No scratch. */
#define AY_BURDEN_MAX_CLASSES 64
#define AY_BURDEN_MAX_FIELDS 64
#define AY_BURDEN_FLAG_NONFINITE 1
#define AY_BURDEN_FLAG_CLASS 2
int ay_burden_bin(const float* rows, int n_rows, int num_classes, int slide_h, int slide_w, int cell, float min_conf, int32_t* counts,
                  int32_t* stats, ay_stream_t stream);
size_t ay_field_select_workspace_bytes(int num_classes, int gy, int gx, int field);
int ay_field_select(const int32_t* counts, int num_classes, int gy, int gx, const int32_t* tissue, int field, int need_tissue, int top_k,
                    int32_t* fields, int32_t* n_found, void* workspace, size_t workspace_bytes, ay_stream_t stream);

/* ---- spatial statistics of a slide's detections: pair counts within a radius (wsi.spatial_stats, wsi.quantify_region(spatial_radii=...);
 *      csrc/ay_spatial.hip) -----------------------------------------------------------------------------------------------------------
 * How the objects of a slide lie with respect to one another: are the cored plaques clustered, and at which scale; do CAA vessels and
 * cored plaques occur together more often than their densities predict.  The cross-class pair counts within a radius are what
 * Ripley's K and L, the pair correlation g and the nearest-neighbour distribution G are made of (on the host, in float64).  The rule
 * is exact (two fp32 operations, integers after them) and tests/spatial_reference.py restates it in NumPy by brute force.
 *
 * THE PAIR RULE.  Input: rows [M][7] fp32 (x1, y1, x2, y2, conf, cls_conf, cls_pred) in pixels of the (halved) slide; the slide's H, W
 *   with 1 <= H, W <= AY_PAIR_MAX_SIDE (2^21, so that 4W is exact in fp32); C classes, 1 <= C <= AY_PAIR_MAX_CLASSES; min_conf; B
 *   radii R_0 < R_1 < ... < R_{B-1} as int32 in QUARTER PIXELS, 1 <= B <= AY_PAIR_MAX_RADII, 1 <= R_0, R_{B-1} <=
 *   AY_PAIR_MAX_RADIUS_Q (with that bound dx^2 + dy^2 fits int32 once |dx|, |dy| <= R_{B-1}); optionally roi_q = (X1, Y1, X2, Y2),
 *   int32 in quarter pixels, a closed rectangle with X1 <= X2, Y1 <= Y2 (NULL: (0, 0, 4W - 1, 4H - 1)); a flag `border`.
 *   For each row, in this order:
 *   Centre: cx = fl32((x1 + x2) * 0.5f), cy alike: THE BURDEN RULE's two operations.
 *   Flagged / below: exactly THE BURDEN RULE's tests, with its flag bits (AY_BURDEN_FLAG_*), in its order.  Such a row is NOT COUNTED
 *     and takes part in nothing.
 *   Position of a counted row: qx = (int)floorf(min(max(fl32(cx * 4.0f), 0), 4W - 1)), qy alike with H: a centre outside the slide
 *     goes to the nearest border position; the multiply is exact or overflows to an infinity, which the clamp takes.
 *   Border distance: bd_i = min(qx - X1, X2 - qx, qy - Y1, Y2 - qy), negative when the position lies outside the ROI.
 *   Eligibility: a counted row i is an ELIGIBLE CENTRE at k iff bd_i >= (border ? R_k : 0).  This is minus-sampling: the partners j may
 *     lie anywhere, only the centres are restricted.
 *   Pair: for counted i != j, d2_ij = (qx_i - qx_j)^2 + (qy_i - qy_j)^2 on integers; the pair is WITHIN k iff d2_ij <= R_k^2
 *     (equality counts; two rows at one position are a pair at distance 0).
 *   Output: pairs int64 [C][C][B]: pairs[a][b][k] = the sum over the eligible-at-k centres i of class a of the number of counted
 *     j != i of class b within k (cumulative in k, ordered pairs).  centres int32 [C][B]: the eligible centres of class a at k.
 *     nn int32 [M][C][2]: for every counted row i, whatever the ROI, and every class b, (d2, j) of the counted j != i of class b with
 *     the smallest d2 <= R_{B-1}^2, ties to the lowest row index j; (-1, -1) if there is none, and for rows not counted.
 *     bd int32 [M]: bd_i; -1 for rows not counted and for any negative value.  stats int32 [2C + 3] = rows counted per class, counted
 *     rows with bd_i >= 0 per class, rows below, rows flagged, flag bits; sum(stats[:C]) + below + flagged == M.
 *   Integer sums and minima with an index tie-break: a function of the inputs alone, the same bytes on every run.
 *   THE RELABEL RULE (include/amyloid_yolo_spatial_sim.h, ay_pair_counts_relabel) counts the same pairs under many labellings of the
 *   counted rows at once: the null band of random labelling that an observed K[a][b] is held against.
 *
 * ay_pair_counts: rows and every output on the device; radii_q (n_radii int32) and roi_q (4 int32, or NULL) on the HOST: they travel
 *   as kernel arguments.  Kernel launches only -- no memset node, no allocation, no host read, no synchronisation -- so the call can
 *   sit in a captured step; a kernel of the call zeroes or fills every output.  n_rows == 0 is legal (rows, nn, bd may then be NULL).
 *   The counted rows are binned by the cell of their position on a grid that comes from the ARGUMENTS: cell side S = R_{B-1} * 2^m
 *   quarter pixels, m the smallest for which ceil(4W / S) * ceil(4H / S) stays within the centre grid's cell cap for n_rows; a search
 *   reads the 3 x 3 cells around its own.  cell_side_q > 0 overrides S (refused below R_{B-1}, or where the grid would exceed 2^30
 *   cells); the result does not depend on it.  The cost is the number of pairs within 3 x 3 cells.  workspace: 16-byte aligned,
 *   ay_pair_counts_workspace_bytes(n_rows, slide_h, slide_w, R_{B-1}, cell_side_q) bytes (0 for arguments the call refuses).  No
 *   scratch. */
#define AY_PAIR_MAX_CLASSES 8
#define AY_PAIR_MAX_RADII 32
#define AY_PAIR_MAX_RADIUS_Q 32767
#define AY_PAIR_MAX_SIDE 2097152
size_t ay_pair_counts_workspace_bytes(int n_rows, int slide_h, int slide_w, int r_max_q, int cell_side_q);
int ay_pair_counts(const float* rows, int n_rows, int num_classes, int slide_h, int slide_w, float min_conf, const int32_t* radii_q,
                   int n_radii, const int32_t* roi_q, int border, int cell_side_q, int64_t* pairs, int32_t* centres, int32_t* nn,
                   int32_t* bd, int32_t* stats, void* workspace, size_t workspace_bytes, ay_stream_t stream);

/* THE PAIR WINDOW RULE (wsi.spatial_stats(window=...), wsi.quantify_region(spatial_window=True)): minus-sampling inside a window that
 *   is no rectangle -- a tissue outline -- given as a mask on cells.  (THE WINDOW RULE is the sampler's.)  tests/
 *   spatial_window_reference.py restates it by brute force over the OUT cells.
 *   Input: THE PAIR RULE's, and mask uint8 [Gy][Gx] on the device (non-zero: IN) with its cell side mask_cell in pixels, an integer
 *   >= AY_PAIR_WINDOW_MIN_CELL; Gx = ceil(W / mask_cell), Gy = ceil(H / mask_cell), Gx * Gy <= AY_PAIR_WINDOW_MAX_CELLS; Sc = 4 *
 *   mask_cell quarter pixels.
 *   OUT positions: position (x, y) of the unbounded quarter-pixel lattice is OUT iff it lies outside the slide (x < 0, x > 4W - 1, y < 0
 *     or y > 4H - 1) or the mask cell (y / Sc, x / Sc) is zero.  The last cell of a row or column is cut by the slide.
 *   For a counted row i at (qx, qy): d2out_i = the minimum over all OUT positions p of |q_i - p|^2, on integers; wbd_i = the largest
 *     integer d in -1 .. R_{B-1} with d * d < d2out_i (so -1 in an OUT cell, and capped at the largest radius);
 *     bd_i = min(THE PAIR RULE's bd_i, wbd_i): the window is mask AND ROI.
 *   Everything after bd_i is THE PAIR RULE unchanged: with `border` a row is an eligible centre at k iff bd_i >= R_k (for the mask
 *     that is R_k^2 < d2out_i: the closed disc holds no OUT position), without it iff bd_i >= 0; stats[C + c] counts the rows with
 *     bd_i >= 0; the output bd is this bd_i, -1 for negatives; partners may lie anywhere, in OUT cells too.
 *   With an all-IN mask and no ROI the nearest OUT position is the slide's edge at the rectangle's bd + 1: pairs, centres, nn and stats
 *     are byte for byte ay_pair_counts', and bd is the rectangle's capped at R_{B-1}.
 *   With both offsets capped at R_{B-1} + 1 <= 32768, dx^2 + dy^2 reaches 2^31: the kernel computes it in UNSIGNED 32 bits.  No float
 *     reaches an output: wbd is an integer square root, a float estimate corrected on integers.
 *
 * ay_pair_counts_window: ay_pair_counts with `mask` (device) and `mask_cell` behind cell_side_q, under the same contract: kernel
 *   launches only, every output reset by the call's own kernels, n_rows == 0 legal, no scratch.  Two more kernels run in front of
 *   the count kernel: the OUT cells of every 64 mask rows of a column as the bits of one word (Gy * Gx / 8 bytes of workspace), and
 *   per row, on 16 lanes, the minimum over the mask columns within R_{B-1}, the vertical distance in a column read off its words.
 *   mask == NULL, mask_cell < 16 (or beyond AY_PAIR_MAX_SIDE) and more than 2^26 mask cells are refused (ay_last_error).  workspace:
 *   16-byte aligned, ay_pair_counts_window_workspace_bytes(n_rows, slide_h, slide_w, R_{B-1}, cell_side_q, mask_cell) bytes (0 for
 *   arguments the call refuses). */
#define AY_PAIR_WINDOW_MIN_CELL 16
#define AY_PAIR_WINDOW_MAX_CELLS 67108864
size_t ay_pair_counts_window_workspace_bytes(int n_rows, int slide_h, int slide_w, int r_max_q, int cell_side_q, int mask_cell);
int ay_pair_counts_window(const float* rows, int n_rows, int num_classes, int slide_h, int slide_w, float min_conf, const int32_t* radii_q,
                          int n_radii, const int32_t* roi_q, int border, int cell_side_q, const uint8_t* mask, int mask_cell, int64_t* pairs,
                          int32_t* centres, int32_t* nn, int32_t* bd, int32_t* stats, void* workspace, size_t workspace_bytes,
                          ay_stream_t stream);

/* ---- stain normalisation for whole-slide detection (wsi.stain_stats, wsi.StainMap, wsi.detect_region(stain=...); csrc/ay_stain.hip) --
 * Amyloid IHC slides are hematoxylin + DAB and differ in stain strength from batch to batch and from scanner to scanner.  The slide's
 * optical densities are unmixed on a fixed two-stain basis, each stain is scaled by a gain that brings its strength to a target's,
 * and the result is mixed again: a per-pixel colour map, fused into the region cut.  PARITY WITH ANY OUTSIDE STAIN-NORMALISATION
 * PACKAGE IS UNPINNED: the behaviour is defined by the rule below and restated in NumPy fp32 by tests/stain_reference.py.
 *
 * THE STAIN RULE (every device operation IEEE fp32, in the order written, nothing fused; no transcendental on the device).
 *   The pixel is (b0, b1, b2), the uint8 values of the (halved) image; for shrink == 2 the ingest's 2x2 round-half-up means.
 *   Tables (ay_stain_params, built on the host in float64, rounded to fp32 once, uploaded once per slide):
 *     od[256]   od[v] = fp32(-log10((v + 1) / 256));  od[255] == 0.
 *     M         3 x 3: rows 0 and 1 the unit OD vectors of stain 0 and stain 1, row 2 their normalised cross product.  The default
 *               basis H_DAB is Ruifrok's hematoxylin (0.650, 0.704, 0.286) and DAB (0.268, 0.570, 0.776), each normalised.
 *     D[9]      fp32(inv(M)), row-major.
 *     A[9]      fp32(inv(M) . diag(g0, g1, 1) . M), row-major, from the float64 factors; g0, g1 the gains.
 *     T[257]    T[k] = fp32((256 * 10^(-k / 64) - 1) / 255);  T[0] == 1.
 *   On the device, with o_c = od[b_c]:
 *     Concentration of stain s in {0, 1}:  c_s = (o_0 * D[0*3+s] + o_1 * D[1*3+s]) + o_2 * D[2*3+s].
 *     Bin of c_s (512 bins of 1/64 OD):    c_s < 0 ? 0 : min((int)(c_s * 64), 511).  With H_DAB no uint8 pixel exceeds 4.55; the
 *                                          clamp is for user bases.
 *     Mapped value of channel c:
 *       o'_c = (o_0 * A[0*3+c] + o_1 * A[1*3+c]) + o_2 * A[2*3+c]
 *       u    = min(max(o'_c, 0), 4) * 64   (evaluated as o > 0 ? o : 0, then o < 4 ? o : 4),  k = min((int)u, 255),  f = u - (float)k
 *       x_c  = T[k] + f * (T[k+1] - T[k])
 *       x_c  = min(max(x_c, 0), 1)         (x > 0 ? x : 0, then x < 1 ? x : 1)
 *     What lies outside the region stays exactly 1.0f (it is not mapped; the rule gives 1.0f for 255 as well).
 *     uint8 form: (uint8)(x_c * 255.0f + 0.5f).
 *   On the host (float64):
 *     Strength of stain s at percentile p (0 < p <= 100) over the n tissue pixels of a histogram: K = max(1, ceil(p * n / 100)),
 *       b* the first bin whose cumulative count reaches K, q_s = (b* + 1) / 64.  n == 0 is an error.
 *     Gain: g_s = clip(t_s / q_s, 1 / max_gain, max_gain), t_s the target's strength.
 *   The table is piecewise linear in 1/64-OD steps: against the exact exponential its error is at most (ln 10 / 64)^2 / 8 * 256 / 255
 *   = 1.63e-4 of full scale (0.04 grey levels); the identity map (gains 1, 1) returns every uint8 value unchanged in the uint8 form.
 *
 * ay_stain_hist_u8: for every TISSUE pixel (THE TISSUE RULE with bg_level) of the (halved) image of a resident region, hist[s * 512 +
 *   bin_s] += 1 for s = 0 and 1 and hist[1024] += 1; hist is uint64 [1025] on the device and is ADDED to: the caller zeroes it, and
 *   the strips of a slide accumulate with no host synchronisation.  Only od and D of the params are read.  A read stream with
 *   ay_tile_tissue_u8's choice of loads (16-byte loads when the base and row_stride_bytes are multiples of 16, byte loads otherwise,
 *   the same counts); od in LDS; per-workgroup int32 histograms in LDS, flushed with 64-bit integer atomics at the latest every 2048
 *   work units of at most 524288 pixels, so that no LDS counter can overflow; integers only: the same bits every run.
 * ay_ingest_region_tiles_stain_u8: ay_ingest_region_tiles_views_u8 (views = {0}: ay_ingest_region_tiles_list_u8) with the mapped
 *   value x_c in place of byte / 255: the same kernels instantiated with another colour stage (od, A and T in LDS), the same
 *   geometry, argument checks and choice of 16-byte or scalar stores, and nothing outside the region is read.
 * ay_stain_apply_u8: the (halved) image, mapped, in the uint8 form: out [region_h / shrink][region_w / shrink][3] uint8, rows
 *   out_stride_bytes apart.
 * All three: kernel launches only (capturable), no scratch. */
#define AY_STAIN_BINS 512
typedef struct ay_stain_params {
    float od[256];
    float D[9];
    float A[9];
    float T[257];
} ay_stain_params;
int ay_stain_hist_u8(const void* region_hwc_u8, int region_h, int region_w, size_t row_stride_bytes, int shrink, int bg_level,
                     const ay_stain_params* params_device, uint64_t* hist, ay_stream_t stream);
int ay_ingest_region_tiles_stain_u8(const void* region_hwc_u8, int region_h, int region_w, size_t row_stride_bytes, int shrink,
                                    int tile, const int32_t* origins_xy, int n, const int* views, int n_views,
                                    const ay_stain_params* params_device, int out_size, float* out_nchw, ay_stream_t stream);
int ay_stain_apply_u8(const void* region_hwc_u8, int region_h, int region_w, size_t row_stride_bytes, int shrink,
                      const ay_stain_params* params_device, uint8_t* out_hwc_u8, size_t out_stride_bytes, ay_stream_t stream);

/* ---- stain basis estimation: each slide's own two stain vectors (wsi.estimate_basis, wsi.StainEstimate, wsi.StainMap(remix=True);
 *      csrc/ay_stain_basis.hip) --------------------------------------------------------------------------------------------------------
 * THE STAIN RULE unmixes on a basis that is given.  The DAB hue shifts with the chromogen batch, the counterstain and the scanner; a
 * gain corrects a stain's strength and cannot correct its direction.  This is the producer of a basis: a Macenko-style estimate of the
 * plane the optical densities of a slide lie in and of the two extreme directions inside it.  PARITY WITH ANY OUTSIDE
 * STAIN-NORMALISATION PACKAGE IS UNPINNED: the behaviour is the rule below, restated in NumPy and Python integers by
 * tests/stain_basis_reference.py.
 *
 * THE BASIS RULE (integers only on the device, float64 on the host; a function of the inputs alone, the same bytes on every run).
 *   Pixels.  (b0, b1, b2) are the bytes of the (halved) image; for shrink == 2 the ingest's 2x2 round-half-up means.  TISSUE is THE
 *     TISSUE RULE's: min(b0, b1, b2) < bg_level.
 *   Integer optical density.  odq[v] = rint(-log10((v + 1) / 256) * 1024), built on the host in float64 (ay_stain_basis_params);
 *     odq[255] == 0, odq[0] == 2466.  With o_c = odq[b_c], a tissue pixel is SELECTED iff min(o_0, o_1, o_2) >= beta_q, beta_q =
 *     rint(beta * 1024): Macenko's beta, default 0.15 (beta_q = 154).
 *   Pass 1, moments (ay_stain_moments_u8).  Output uint64 [11]: n_tissue, n_sel, S_c = sum of o_c (3 words), P_cd = sum of o_c * o_d
 *     for c <= d (6 words, in the order 00, 01, 02, 11, 12, 22); n_tissue counts the tissue pixels, the other ten run over the selected
 *     pixels.  The call ADDS to the output: the caller zeroes it once and the strips accumulate with no host synchronisation.  Bounds:
 *     one pixel adds at most 2466^2 = 6 081 156 to a word, so an item of 16 pixels fits int32 (97 298 496); whatever is summed over more
 *     than one item is 64 bits wide (a lane sees up to 128 items of a work unit).
 *   Host, the plane (float64).  With n = n_sel the numerators n * P_cd - S_c * S_d are taken in exact (Python) integers, divided by
 *     n * (n - 1) and given to a symmetric eigensolver (numpy.linalg.eigh).  e1 is the eigenvector of the largest eigenvalue with the
 *     sign that makes e1_0 + e1_1 + e1_2 > 0; e2 that of the second eigenvalue with the sign that makes its component of largest
 *     magnitude positive (the lowest index on ties).  eq1 = rint(1024 * e1), eq2 = rint(1024 * e2), int32.  n_sel < 2 or a second
 *     eigenvalue that is not positive is an error: such a slide has no stain plane.
 *   Pass 2, direction histogram (ay_stain_direction_hist_u8).  For every selected pixel, in int32: p1 = sum of o_c * eq1_c, p2 = sum of
 *     o_c * eq2_c.  |eq_c| <= 1024 (the entry point refuses more) keeps |256 * p2| <= 2466 * 1024 * 3 * 256 = 1 939 341 312 < 2^31.
 *     p1 <= 0: hist[512] += 1 (the "outside" count).  Otherwise k = floor(256 * p2 / (p1 + |p2|)) -- the floor, not C's truncation: for
 *     p2 < 0 it is -ceil(256 * |p2| / (p1 + |p2|)) -- which lies in -256 .. 255, and hist[k + 256] += 1.  Every selected pixel:
 *     hist[513] += 1.  Output uint64 [514], ADDED to.  d = p2 / (p1 + |p2|) is monotone in the angle atan2(p2, p1) on the half plane p1
 *     > 0, so a percentile of the angle is a percentile of d: no division by a float and no transcendental runs on the device.
 *   Host, the vectors (float64).  n = the sum of hist[0 .. 511].  For K_lo = max(1, ceil(alpha * n / 100)) and K_hi = max(1,
 *     ceil((100 - alpha) * n / 100)): b the first bin whose cumulative count reaches K, d = (b - 256 + 0.5) / 256, v = (1 - |d|) * eq1 +
 *     d * eq2, normalised.  alpha = 1 is Macenko's.  The two vectors go to stain 0 and stain 1 of a prior basis (default H_DAB) by the
 *     pairing with the larger sum of dot products (the straight pairing on a tie).  n == 0 is an error.
 *   Guard.  A vector further than max_angle degrees from its prior vector is replaced by the prior's and reported.  The default is half
 *     the angle between the prior's two vectors (H_DAB: about 18.6 degrees): the two results can then neither swap nor coincide.
 *   Limit.  The extreme on the DAB side is the alpha-th percentile of the selected pixels: on a slide whose DAB-positive share of
 *     selected pixels is below alpha per cent it is not DAB, and the guard catches it or the caller lowers alpha.
 *
 * Both entry points: ay_stain_hist_u8's read stream (48-byte items, work units of 16 rows x up to 2048 items, 16-byte loads when the
 *   base and row_stride_bytes are multiples of 16, byte loads otherwise, the same sums), the tissue test before anything else, odq in
 *   LDS; kernel launches only -- no allocation, no memset node, no host read, no scratch.  A region without a halved image returns
 *   AY_OK.  Refused (-1, nothing launched, nothing written): a null pointer, a bad shape or stride, shrink outside {1, 2}, bg_level
 *   outside 0 .. 256, beta_q outside 0 .. 2466, an output that is not 8-byte aligned, |eq_c| > 1024.
 * ay_stain_moments_u8: a lane sums an item in int32 registers and its items in 64-bit registers; a wavefront reduction, the four
 *   wavefronts through LDS, and at most 11 64-bit integer atomics per workgroup.
 * ay_stain_direction_hist_u8: eq1 and eq2 by value (scalar registers); per-workgroup int32 LDS bins flushed with 64-bit integer atomics
 *   as ay_stain_hist_u8 flushes its own, with the same overflow argument. */
#define AY_BASIS_OD_SCALE 1024
#define AY_BASIS_OD_MAX 2466
#define AY_BASIS_MOMENT_WORDS 11
#define AY_BASIS_DIR_BINS 512
#define AY_BASIS_HIST_WORDS 514
typedef struct ay_stain_basis_params {
    int32_t odq[256];
} ay_stain_basis_params;
int ay_stain_moments_u8(const void* region_hwc_u8, int region_h, int region_w, size_t row_stride_bytes, int shrink, int bg_level,
                        int beta_q, const ay_stain_basis_params* params_device, uint64_t* moments, ay_stream_t stream);
int ay_stain_direction_hist_u8(const void* region_hwc_u8, int region_h, int region_w, size_t row_stride_bytes, int shrink, int bg_level,
                               int beta_q, int eq1_0, int eq1_1, int eq1_2, int eq2_0, int eq2_1, int eq2_2,
                               const ay_stain_basis_params* params_device, uint64_t* hist, ay_stream_t stream);

/* ---- amyloid load: stain-positive area per map cell and per detection (wsi.stain_load, wsi.box_morphometry,
 *      wsi.quantify_region(load=True); csrc/ay_load.hip) ----------------------------------------------------------------------------------
 * The field's second read-out next to object counts: the share of tissue area that is DAB-positive, on THE BURDEN RULE's grid, and the
 * positive pixels inside every detection's box (plaque area, fill, mean optical density).  tests/load_reference.py restates the rule
 * in NumPy.
 *
 * THE LOAD RULE (integers, and the fp32 operations written below, in that order; a function of the inputs alone, the same bytes on
 *   every run).
 *   Pixel classes.  A pixel (X, Y) of the (halved) H x W slide is TISSUE by THE TISSUE RULE: min(b0, b1, b2) < bg_level; for shrink ==
 *     2 the bytes are the ingest's 2x2 round-half-up means.  Its bin q is THE STAIN RULE's bin of c_s for the chosen stain s in {0,
 *     1}: od, D, the same expression, the same clamp.  It is POSITIVE iff it is tissue and q >= thres_bin; thres_bin is an integer in
 *     0 .. 512, and 512 makes nothing positive.  The host turns an optical density into thres_bin as StainStats.positive_fraction
 *     does: min(round(thres * 64), 512).  The threshold applies to the slide's OWN concentrations (a caller who wants it on a
 *     normalised scale divides it by the stain map's gain); A and T of the params are never read.
 *   Three sums per entity (a cell or a box): tissue = its tissue pixels, positive = its positive pixels, bin_sum = the sum of q over
 *     its positive pixels.
 *   Cells.  The grid is wsi.tile_grid(H, W, cell, 0) over the whole (halved) slide: Gy = ceil(H / cell), Gx = ceil(W / cell); pixel
 *     (X, Y) belongs to cell (Y / cell, X / cell).  cell >= AY_LOAD_MIN_CELL = 16: the cell pass takes 16 pixels of a row per lane and
 *     16 rows per work unit, and its on-chip table holds the two cells and two cell rows those can touch.  Output: uint64 [Gy][Gx][3] =
 *     (tissue, positive, bin_sum).
 *   Boxes.  Input: rows [M][7] fp32, detect_region's rows in pixels of the (halved) slide; only columns 0 .. 3 = (x1, y1, x2, y2) are
 *     read.  A row with a coordinate that is not finite sets AY_LOAD_FLAG_NONFINITE in the flags word and gets nothing.  Otherwise, in
 *     fp32: lo_x = min(max(ceilf(x1 - 0.5f), 0.0f), (float)W), hi_x the same of x2, lo_y and hi_y the same of y1 and y2 with H, then
 *     each converted to int.  The box OWNS the pixels lo_x <= X < hi_x, lo_y <= Y < hi_y: those whose centre (X + 0.5, Y + 0.5) lies
 *     in [x1, x2) x [y1, y2).  An inverted or empty box owns none.  H, W <= 2^24, so that (float)W is exact.  Output: uint64 [M][4] =
 *     (pixels, tissue, positive, bin_sum), pixels the owned pixels that were visited: (hi_x - lo_x) * (hi_y - lo_y) once every strip
 *     has been seen.  Overlapping boxes are independent: each counts its own pixels.
 *   Accumulation.  A call sees one resident region (a strip) whose (halved) image has its top-left pixel at (origin_y, origin_x) of
 *     the slide, both >= 0 and the image inside H x W; the origin need not be a multiple of cell.  The call ADDS to cells and boxes
 *     and ORs into flags: the caller zeroes them once, visits every pixel of the slide once over the strips and reads back once.
 *
 * ay_stain_load_u8: kernel launches only -- no allocation, no memset node, no host read, no scratch -- so it can sit in a captured
 *   step.  cells == NULL skips the cell pass; n_rows == 0 skips the box pass (rows, boxes and flags may then be NULL).  A region
 *   without a halved image returns AY_OK.  Refused (-1, nothing launched): a bad shape or stride, shrink outside {1, 2}, bg_level
 *   outside 0 .. 256, stain outside {0, 1}, thres_bin outside 0 .. 512, cell < AY_LOAD_MIN_CELL (with or without cells), slide_h or
 *   slide_w outside 1 .. 2^24, a region that does not lie inside the slide, cells or boxes not 8-byte aligned.
 *   The cell pass is a read stream over the image with ay_stain_hist_u8's items and choice of loads (16-byte loads when the base and
 *   row_stride_bytes are multiples of 16, byte loads otherwise, the same counts), od in LDS, the chosen stain's three D in scalar
 *   registers, the tissue test before the unmixing; a lane sums its 16 pixels in registers, a workgroup its unit of 16 rows x 4096
 *   pixels in an int32 LDS table (at most 65536 * 511 < 2^31 per word), and memory sees one 64-bit integer atomic per (workgroup,
 *   unit, cell, sum) that is not 0.  The box pass is a gather for detection boxes: one wavefront per box, an integer intersection
 *   with the region first, at most four 64-bit atomics per box and call.  It is correct for any box, a whole-slide rectangle
 *   included, but ONE HUGE BOX RUNS ON ONE WAVEFRONT. */
#define AY_LOAD_MIN_CELL 16
#define AY_LOAD_FLAG_NONFINITE 1
int ay_stain_load_u8(const void* region_hwc_u8, int region_h, int region_w, size_t row_stride_bytes, int shrink, int origin_y,
                     int origin_x, int slide_h, int slide_w, int bg_level, const ay_stain_params* params_device, int stain, int thres_bin,
                     int cell, uint64_t* cells /* or NULL */, const float* rows, int n_rows, uint64_t* boxes,
                     int32_t* flags /* NULL iff n_rows == 0 */, ay_stream_t stream);

/* ---- focus map: image sharpness per map cell and per detection (wsi.focus_map, wsi.focus_summary, wsi.quantify_region(focus=True);
 *      csrc/ay_focus.hip) ------------------------------------------------------------------------------------------------------------
 * Every number of a slide assumes that the scanner was in focus where it counted; a blurred patch is still tissue, loses its
 * detections and reads as "low burden".  The variance of the Laplacian of the luma over tissue is the read-out, on THE BURDEN RULE's
 * grid and inside every detection's box.  The reference has no such read-out: PARITY IS UNPINNED, the behaviour is the rule below,
 * restated in NumPy by tests/focus_reference.py.
 *
 * THE FOCUS RULE (integers only; a function of the inputs alone, the same bytes on every run).
 *   Bytes.  (b0, b1, b2) of pixel (X, Y) of the (halved) H x W slide are THE TISSUE RULE's: for shrink == 2 the ingest's 2x2
 *     round-half-up means.
 *   Luma.  g = (77 * b0 + 150 * b1 + 29 * b2 + 128) >> 8, in 0 .. 255.
 *   Evaluated pixel.  (X, Y) is EVALUATED iff 1 <= X <= W - 2 and 1 <= Y <= H - 2 and the pixel and its four edge neighbours
 *     (X - 1, Y), (X + 1, Y), (X, Y - 1), (X, Y + 1) are all TISSUE at bg_level (min(b0, b1, b2) < bg_level).  A tissue / glass edge is
 *     not texture and never counts as sharpness.
 *   Laplacian.  lap = 4 * g(X, Y) - g(X - 1, Y) - g(X + 1, Y) - g(X, Y - 1) - g(X, Y + 1), in -1020 .. 1020.
 *   Sums.  Per owner: n = its evaluated pixels, s1 = the sum of lap over them (signed), s2 = the sum of lap * lap, as int64 in two's
 *     complement.  A cell of the grid wsi.tile_grid(H, W, cell, 0) (Gy = ceil(H / cell), Gx = ceil(W / cell)) owns the evaluated
 *     pixels with (X, Y) in it -- cell (Y / cell, X / cell); the neighbours may lie in another cell.  A box (rows [M][7] fp32, columns
 *     0 .. 3 read) owns the evaluated pixels THE LOAD RULE gives it: lo_x <= X < hi_x, lo_y <= Y < hi_y with the four edges computed in
 *     fp32 exactly as there (centre in [x1, x2) x [y1, y2), clamped to the slide); overlapping boxes are independent.  A row with a
 *     coordinate that is not finite sets AY_FOCUS_FLAG_NONFINITE in the flags word and gets nothing.
 *   Host, float64.  sharpness = s2 / n - (s1 / n)^2, the variance of the Laplacian; NaN where n == 0.  It depends on the texture of
 *     the tissue and on the strength of the stain as well as on focus: it compares regions of one slide, or slides of one protocol.
 *   Limits.  cell >= AY_FOCUS_MIN_CELL = 16; H, W <= 2^24; H * W < 2^43, so that s2 fits int64 (1020^2 * 2^43 < 2^63).
 *   Accumulation.  A call sees one resident region that holds whole rows of the slide, origin_y .. origin_y + region_h / shrink - 1,
 *     (region_w / shrink == W), and is told the rows it OWNS: it ADDS the sums of the evaluated pixels with own_y0 <= Y < own_y1, and
 *     nothing else, to cells and boxes, and ORs into flags.  The rows it needs resident are max(own_y0, 1) - 1 .. min(own_y1, H - 1),
 *     one more than it owns on either side.  The caller zeroes the outputs once and makes the owned ranges of its calls a partition of
 *     1 .. H - 2 (wsi.focus_map: strips that share two rows).  A call that owns no row of 1 .. H - 2, or any call when W < 3, has no
 *     pixel to evaluate: it needs no row, launches nothing, adds nothing and flags nothing.
 *
 * ay_focus_u8: kernel launches only -- no allocation, no memset node, no host read, no scratch -- so it can sit in a captured step.
 *   cells == NULL skips the cell pass; n_rows == 0 skips the box pass (rows, boxes and flags may then be NULL).  Refused (-1, nothing
 *   launched, nothing written): a needed row that is not resident; a null region, a bad shape or stride, shrink outside {1, 2},
 *   bg_level outside 0 .. 256, cell < AY_FOCUS_MIN_CELL (with or without cells), slide_h or slide_w outside 1 .. 2^24 or their product
 *   not below 2^43, region_w / shrink != slide_w, a region that does not lie inside the slide, own_y0 < 0, own_y0 > own_y1, own_y1 >
 *   slide_h, n_rows < 0 or rows without boxes and flags, cells or boxes not 8-byte aligned.
 *   The cell pass is a read stream with ay_stain_load_u8's items and choice of loads (16-byte loads when the base and
 *   row_stride_bytes are multiples of 16, byte loads otherwise, the same sums).  A work unit is up to 32 centre rows x 32 items (512
 *   pixels, 256 of the halved image); its rows and one halo row above and below go through LDS once as a luma byte and a tissue bit
 *   per pixel, the pixels left and right of the unit with them, and the four neighbours of every pixel come from LDS.  A lane sums
 *   at most 4 x 16 pixels in int32 registers (s2 <= 66 585 600), a workgroup its unit in a uint64 LDS table, and memory sees one 64-bit
 *   integer atomic per (workgroup, unit, cell, sum) that is not 0: no 32-bit word ever holds more than one lane's share.  The box pass
 *   is a gather for detection boxes: one wavefront per box, an integer intersection with the owned rows first, at most three 64-bit
 *   atomics per box and call; correct for any box, but ONE HUGE BOX RUNS ON ONE WAVEFRONT. */
#define AY_FOCUS_MIN_CELL 16
#define AY_FOCUS_FLAG_NONFINITE 1
int ay_focus_u8(const void* region_hwc_u8, int region_h, int region_w, size_t row_stride_bytes, int shrink, int origin_y, int slide_h,
                int slide_w, int own_y0, int own_y1, int bg_level, int cell, int64_t* cells /* [Gy][Gx][3], or NULL */,
                const float* rows, int n_rows, int64_t* boxes /* [M][3] */, int32_t* flags /* NULL iff n_rows == 0 */,
                ay_stream_t stream);

/* ---- plaque segmentation: the stained component under every detection (wsi.segment_boxes, wsi.plaque_morphometry,
 *      wsi.quantify_region(segment=True); csrc/ay_segment.hip) ------------------------------------------------------------------------
 * ay_stain_load_u8's box sums count every positive pixel in the detector's rectangle: the neighbouring plaque that pokes into it and
 * the speckle included, the part of the plaque the box cuts off excluded.  The object itself is the connected stained component under
 * the detection: its area, core, perimeter, centre and tight box.  The reference has no such read-out: PARITY IS UNPINNED, the
 * behaviour is the rule below, restated in NumPy (with a plain flood fill) by tests/segment_reference.py.
 *
 * THE SEGMENT RULE (integers, and the fp32 steps of THE LOAD RULE's box; a function of the inputs alone, the same bytes on every run).
 *   Pixel classes.  TISSUE and the bin q of the chosen stain s in {0, 1} are exactly THE LOAD RULE's (the 2x2 round-half-up means for
 *     shrink == 2, od, D, the same expression, the same clamp).  A pixel is POSITIVE iff it is tissue and q >= thres_bin, and CORE iff
 *     it is positive and q >= core_bin; 0 <= thres_bin <= core_bin <= 512, and a core_bin of 512 makes no pixel core.
 *   Box and window.  A row's edges lo_x, hi_x, lo_y, hi_y are THE LOAD RULE's (the same four fp32 steps).  A row with a coordinate
 *     that is not finite is NONFINITE; one with lo_x >= hi_x or lo_y >= hi_y is EMPTY.  Every other row has a WINDOW, the box grown by
 *     `margin` (0 .. AY_SEG_MAX_MARGIN = 127) pixels on every side and cut to the H x W slide: wx0 = max(lo_x - margin, 0), wx1 =
 *     min(hi_x + margin, W), wy0 and wy1 the same with lo_y, hi_y and H, ww = wx1 - wx0, wh = wy1 - wy0.  A row with ww or wh above
 *     AY_SEG_MAX_SIDE = 255 is LARGE (a window then holds at most 65 025 pixels: a pixel's index in it and a sentinel fit 16 bits); any
 *     other row is normal.
 *   Components.  The 8-connected sets of the positive pixels of the window; pixels outside the window connect nothing.  A component
 *     is a CANDIDATE iff at least one of its pixels lies in the box proper (lo_x <= X < hi_x, lo_y <= Y < hi_y) and its area -- its
 *     pixels in the whole window -- is >= min_area (>= 1).  The SELECTED component is the candidate with the largest area, among
 *     equals the one that holds the lowest window raster index (Y - wy0) * ww + (X - wx0).
 *   Output.  int32 [M][AY_SEG_COLS = 20] per row:
 *      0       status: 0, or exactly one of AY_SEG_NONFINITE, AY_SEG_EMPTY, AY_SEG_LARGE, AY_SEG_NOT_RESIDENT, AY_SEG_INTERNAL
 *      1 .. 4  wx0, wy0, ww, wh (0 for NONFINITE and EMPTY)
 *      5       the positive pixels of the window
 *      6       the number of candidates
 *      7       area of the selected component
 *      8       its core pixels
 *      9       bin_sum: the sum of q over it (at most 65 025 * 511 < 2^31)
 *     10       perimeter: the number of pairs (pixel of the component, one of its four edge neighbours) whose neighbour is not in the
 *              component, outside the window counting as "not": one pixel has 4, a 2x2 block 8, two diagonal pixels 8
 *     11, 12   the sums of X - wx0 and of Y - wy0 over the component (at most 65 025 * 254)
 *     13 .. 16 its tight bounding box bx0, by0, bx1, by1 in slide pixels, the high edges exclusive
 *     17       sides: bit 1 / 2 / 4 / 8 iff it has a pixel in the window's first column / first row / last column / last row
 *     18       its pixels inside the box proper
 *     19       0
 *     Words 5 .. 19 are 0 for any status other than 0; words 7 .. 18 are 0 when nothing is selected.  The flags word gets the OR of
 *     every status written.
 *   Ownership.  Every row has an OWNER ROW: wy0 if it has a window (LARGE rows included), else 0.  A call sees one resident region
 *     whose (halved) image has its top-left pixel at (origin_y, origin_x) of the slide, like ay_stain_load_u8, and is told a range
 *     [own_y0, own_y1): it WRITES all 20 words of exactly the rows whose owner row lies in that range and touches no other row.  An
 *     owned normal row whose window is not wholly inside the region gets AY_SEG_NOT_RESIDENT (the window words filled, the rest 0):
 *     the caller's error, reported and not guessed around.  The caller makes the owned ranges of its calls a partition of [0, H);
 *     the result does not depend on how the slide was cut (wsi.segment_boxes: strips 254 rows short of their height apart, so that
 *     every window lies wholly in the strip that owns it).
 *
 * ay_box_segments_u8: kernel launches only -- no allocation, no memset node, no host read, no scratch, no workspace beyond `out` --
 *   so it can sit in a captured step.  n_rows == 0 returns AY_OK without a launch.  Refused (-1, nothing launched, nothing written): a
 *   null region or params, a bad shape or stride, shrink outside {1, 2}, bg_level outside 0 .. 256, stain outside {0, 1}, thres_bin
 *   or core_bin outside 0 .. 512 or core_bin < thres_bin, margin outside 0 .. 127, min_area < 1, slide_h or slide_w outside 1 .. 2^24,
 *   a region that does not lie inside the slide, own_y0 < 0, own_y0 > own_y1, own_y1 > slide_h, n_rows < 0, null rows, out or flags
 *   with n_rows > 0.
 *   One workgroup of 256 per owned row, the rows grid-stride; a row that is not owned costs its four fp32 edges.  The window is
 *   classified once into a positive and a core bit plane in LDS and labelled there by a union-find over its row runs (32-bit parents,
 *   LDS atomicMin; one pass, no sweeps to convergence: a one-pixel spiral costs what a disc costs), then the areas per root, the
 *   selection, and one pass of sums over the selected component.  Two instances run one after the other: windows up to 96 pixels a
 *   side (22 KiB of LDS, several workgroups per CU) and up to 255 (147 KiB).  Every find and union loop has a strictly decreasing
 *   variable and a cap on top; a workgroup that hits the cap writes AY_SEG_INTERNAL for that row and goes on: it never appears unless
 *   the labelling has a bug. */
#define AY_SEG_COLS 20
#define AY_SEG_MAX_SIDE 255
#define AY_SEG_MAX_MARGIN 127
#define AY_SEG_NONFINITE 1
#define AY_SEG_EMPTY 2
#define AY_SEG_LARGE 4
#define AY_SEG_NOT_RESIDENT 8
#define AY_SEG_INTERNAL 16
int ay_box_segments_u8(const void* region_hwc_u8, int region_h, int region_w, size_t row_stride_bytes, int shrink, int origin_y,
                       int origin_x, int slide_h, int slide_w, int own_y0, int own_y1, int bg_level,
                       const ay_stain_params* params_device, int stain, int thres_bin, int core_bin, int margin, int min_area,
                       const float* rows, int n_rows, int32_t* out /* [M][20] */, int32_t* flags, ay_stream_t stream);

/* Replaying a captured HIP graph of these calls.  Every entry point is plain stream work -- kernel launches only: no allocation,
 * no host copy, no memset node, no symbol access inside a call (the once-per-slide calls ay_seam_merge and ay_slide_match excepted:
 * they memset, read a few words back and synchronise the stream, and are not for capture; ay_burden_bin and ay_field_select, also
 * once per slide, are kernel launches only and capturable) -- so a stream capture of a step
 * (ay_plan_forward + ay_nms_merge ...) replays like any other graph (scripts/micro/graph_sync.hip, graph_coherence.hip,
 * graph_input_coherence.hip: every wait covers a replayed graph, a kernel behind a replay sees its writes, a replay sees eager writes to its inputs).  The persistent kernels rely on
 * stream order between launches (a launch hands its work-counter set back zeroed for a later launch on that stream, the plan's
 * arena reuses a block once its last reader has been issued): replay a graph on ONE stream at a time and do not run other library
 * work on the capture stream concurrently.  ay_stream_fence records a library-owned event on `stream` and makes the stream wait for
 * it: an optional stream-ordered fence (utils.graph_replay() places it behind a replay; the product test replays without it). */
int ay_stream_fence(ay_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* AMYLOID_YOLO_H */
