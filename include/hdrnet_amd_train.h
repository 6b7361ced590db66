/* Training-loop helpers of libhdrnet_amd.so that are not part of the bilateral-grid operator boundary
 * (include/hdrnet_amd.h): the optimizer update of the reference's training loop.
 *
 * hdrnet/bin/train.py:108-115 minimises the l2 loss with tf.train.AdamOptimizer; one update of the whole model
 * (~482 k parameters) is 2 MB of state.  As a multi-tensor launch over 35 separate tensors it takes ~40 us of a
 * 0.7-ms training step on MI355X (few, long-running workgroups); over ONE flat buffer it is a 2-us kernel.
 *
 * hdrnet_adam_step_f32: Adam (Kingma & Ba; the update of torch.optim.Adam without amsgrad / weight decay) on flat
 * fp32 buffers of n elements, in place:
 *   t = step[0] + 1;  m = b1 m + (1 - b1) g;  v = b2 v + (1 - b2) g^2
 *   param -= lr / (1 - b1^t) * m / (sqrt(v) / sqrt(1 - b2^t) + eps)
 * hdrnet_adam_step_tf_f32: the same with TensorFlow's placement of epsilon -- tf.train.AdamOptimizer, the optimizer the
 * reference constructs (hdrnet/bin/train.py:113), applies "epsilon hat" (tensorflow/python/training/adam.py):
 *   param -= lr sqrt(1 - b2^t) / (1 - b1^t) * m / (sqrt(v) + eps)
 * i.e. the formula above with eps / sqrt(1 - b2^t) in place of eps.  The two agree to rounding once sqrt(v) >> eps.
 * `step` is a DEVICE float holding the number of updates done so far; the call increments it (a second, one-thread
 * launch), so a captured hipGraph replays correctly.  Returns 0, or 1 for a bad argument (null / misaligned buffer,
 * n <= 0), 2 when a launch fails -- with the reason in hdrnet_last_error(), as for every helper of this header; no host
 * synchronisation. */
#ifndef HDRNET_AMD_TRAIN_H_
#define HDRNET_AMD_TRAIN_H_

#include <stddef.h>

/* the coefficient network trained with batch norm: hdrnet_coefficients_bn_train_f32 / hdrnet_coefficients_bn_grad_f32 */
#include "hdrnet_amd_coeff_bn.h"
/* the same training entry points, with and without batch norm, for batches up to 32 */
#include "hdrnet_amd_coeff_wide.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The l2 loss of hdrnet/metrics.py:21-24 WITH its unit gradient in one pass over the batch (the training step's form of
 * hdrnet_l2_loss_f32 + hdrnet_l2_loss_grad_f32 of include/hdrnet_amd.h, which read prediction and target twice):
 *   loss[0] = mean((target - prediction)^2);   dprediction_unit = (2 / n) * (prediction - target)
 * `workspace`: hdrnet_l2_loss_workspace_bytes(n) bytes.  hdrnet_l2_loss_grad_scale_f32 then turns the unit gradient into
 * the gradient, dprediction *= grad_output[0] (a DEVICE scalar), and does nothing but read that scalar when it is 1 --
 * the loss as the root of the backward pass.  Tensors 16-byte aligned; 0 on success, 1 for a bad argument. */
int hdrnet_l2_loss_with_grad_f32(const float* prediction, const float* target, long long n, float* loss,
                                 float* dprediction_unit, void* workspace, size_t workspace_bytes, void* stream);
int hdrnet_l2_loss_grad_scale_f32(float* dprediction, const float* grad_output, long long n, void* stream);

/* The training loop's monitors in the loss's own pass (csrc/loss_psnr.hip; hdrnet/bin/train.py:95-96, 117-125, 160-174):
 * prediction / target are [batch][n / batch] fp32.  ONE pass over both leaves the sum of squared differences per image and,
 * with dprediction_unit given, hdrnet_l2_loss_with_grad_f32's unit gradient (2 / n)(prediction - target); a second,
 * one-workgroup launch finishes in double:
 *   image_mse[b] = float(S_b / (n / batch))                             (optional output, [batch])
 *   loss[0]      = float(sum_b S_b / n)
 *   psnr[0]      = float(mean_b(-10 / ln 10 * log(image_mse[b])))       (hdrnet/metrics.py:27-33; S_b == 0 gives +inf)
 *   ema          (optional, DEVICE fp32 {ema_loss, ema_psnr, updates}): s <- s - (1 - decay)(s - value) for the loss and
 *                the psnr just stored, in double from the stored floats, rounded once; updates += 1.  The shadow is
 *                whatever the block held (start it at 0) and is not debiased: tf.train.ExponentialMovingAverage(decay)
 *                .apply([tensor]) of TF 1.x as remembered, not confirmed against TensorFlow.  s / (1 - decay^updates)
 *                is the debiased reading.  decay in [0, 1).
 *   totals       (optional, DEVICE float64 {sum of per-image psnr, sum of image_mse, images}): accumulated in place, image
 *                by image in index order -- an evaluation set's running sums, whatever the batch size.
 * No atomics: every partial sum belongs to one image and is added in a fixed order, so results are bit-repeatable.  Nothing
 * is read from the host between calls: a captured hipGraph replays correctly.  n % batch == 0; n / batch need not be a
 * multiple of 4.  prediction, target, dprediction_unit and workspace 16-byte aligned, totals 8-byte, the other outputs
 * 4-byte; `workspace`: hdrnet_loss_psnr_workspace_bytes(n, batch) bytes (0 for arguments the call refuses).  Validation
 * precedes any HIP call: 1 for a null required buffer, n <= 0, batch <= 0, n % batch != 0, a short workspace, a misaligned
 * pointer, or decay outside [0, 1) with ema given; 2 for a launch failure; else 0.  The backward stays
 * hdrnet_l2_loss_grad_scale_f32 (first) / hdrnet_l2_loss_grad_f32 (again, through a retained graph). */
size_t hdrnet_loss_psnr_workspace_bytes(long long n, int batch);
int hdrnet_loss_psnr_f32(const float* prediction, const float* target, long long n, int batch, float* loss, float* psnr,
                         float* image_mse /*opt*/, float* dprediction_unit /*opt*/, float* ema /*opt, 3 floats*/,
                         float decay, double* totals /*opt, 3 doubles*/, void* workspace, size_t workspace_bytes,
                         void* stream);

/* The pyramid model's up-add and its VJP (hdrnet/models.py:283-287: `current = tf.image.resize_images(current, sz, BILINEAR,
 * align_corners=True) + out_lvl`), NHWC fp32, the resize of hdrnet_resize_bilinear_f32 (include/hdrnet_amd.h):
 *   hdrnet_resize_add_f32            output[B, OH, OW, C] = resize(coarse[B, IH, IW, C]) + fine[B, OH, OW, C], one pass
 *   hdrnet_resize_bilinear_grad_f32  dinput[B, IH, IW, C] = the transpose of the resize applied to doutput[B, OH, OW, C], as a
 *                                    gather in a fixed order (no atomics: bit-reproducible)
 * (the gradient of the up-add with respect to `fine` is doutput itself).  0 on success, 1 for a bad argument. */
int hdrnet_resize_add_f32(const float* coarse, const float* fine, float* output, int batch, int in_height, int in_width,
                          int out_height, int out_width, int channels, void* stream);
int hdrnet_resize_bilinear_grad_f32(const float* doutput, float* dinput, int batch, int in_height, int in_width,
                                    int out_height, int out_width, int channels, void* stream);

int hdrnet_adam_step_f32(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, long long n,
                         float* step, float lr, float beta1, float beta2, float eps, void* stream);
int hdrnet_adam_step_tf_f32(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, long long n,
                            float* step, float lr, float beta1, float beta2, float eps, void* stream);

/* Sample preparation (csrc/sample_prep.hip): one launch turns wire-format source images that sit in device memory into
 * the fp32 NHWC tensors a training step consumes -- the reference's hdrnet/data_pipeline.py:126-171 (`_augment_data`),
 * :228-241, :267-287 on the device.  For each output sample b a 32-byte record of the DEVICE table
 *   ops[b] = {index, flip_lr, flip_ud, rot90, crop_y, crop_x, 0, 0}   (int32)
 * selects source image `index` and the geometry, in the reference's order:
 *   s   = source[index]                                        [Hs][Ws][3], dtype 0 f32, 1 u8, 2 u16
 *   s   = s[:, ::-1] if flip_lr;  s = s[::-1] if flip_ud;  s = rot90(s, rot90)   (counter-clockwise, tf.image.rot90)
 *   out = s[crop_y : crop_y + H, crop_x : crop_x + W] / white_level   (fp32, rounded as the IEEE division; f32 sources are
 *                                                                      copied unscaled)
 *   low[y, x] = out[min(floor(y * (H / (float)n)), H - 1), min(floor(x * (W / (float)n)), W - 1)],  n = net_input_size
 * (TF1 ResizeNearestNeighbor, align_corners=False; fp32 scale and product).  Outputs, each optional (NULL = skipped):
 * image_input [B][H][W][3] from src_input, image_target [B][H][W][3] from src_target (same table, its own dtype and white
 * level; src_target may be NULL when image_target is), lowres_input [B][n][n][3] from src_input.  ops == NULL is the
 * identity with index = b: it needs B <= N and (H, W) == (Hs, Ws).
 * The table is read on the device, so a captured graph replays with new draws after a copy into it.  Memory safety does
 * not depend on its contents: index is clamped to [0, N), the crop offsets to [0, extent - size] of the turned source,
 * rot90 is masked with 3 and the flips with 1 -- such a record is a caller error whose result is the clamped sample,
 * never an out-of-bounds access.  A crop that does not fit the source turned by a quarter (H > Ws or W > Hs) is refused
 * when a table is given, unless HDRNET_SAMPLE_EVEN_TURNS_ONLY is set: the device then reads rot90 & 2.
 * W % 4 == 0 when a full-resolution output is requested; outputs 16-byte, sources and table 4-byte aligned; the sources
 * are read as aligned dwords (an allocation ends on a dword boundary).  Validation precedes any HIP call: 0, or 1 with
 * hdrnet_last_error() set (include/hdrnet_amd.h).  B == 0 is a no-op.  No workspace, no atomics, asynchronous on `stream`. */
#define HDRNET_SAMPLE_EVEN_TURNS_ONLY 1u
int hdrnet_prepare_batch(const void* src_input, int input_dtype, float input_white_level, const void* src_target,
                         int target_dtype, float target_white_level, int N, int Hs, int Ws, const int* ops, int B,
                         float* image_input, float* image_target, int H, int W, float* lowres_input,
                         int net_input_size, unsigned flags, void* stream);

/* The same from a set of images of MIXED extents (photographs of many sizes and both orientations, as the reference's
 * ImageFilesDataPipeline / HDRpDataPipeline decode them, data_pipeline.py:183-287).  src_input / src_target are FLAT
 * buffers of n_samples samples each (3 per pixel): the images back to back with no padding between them, so an image
 * starts at any byte (u8) or even byte (u16).  The DEVICE table
 *   images[i] = {offset_lo, offset_hi, Hs, Ws}   (int32; 16-byte aligned)
 * gives image i's first sample (a 64-bit count of SAMPLES split in two words, the same for both buffers: a pair has
 * equal extents, only the element size differs) and its extents.  ops[b] is hdrnet_prepare_batch's record; the crop
 * offsets are clamped to the room of the record's OWN image, [0, (odd turn ? Ws_i : Hs_i) - H] and so on.  `ops` is
 * required: there is no identity geometry over mixed extents.  That every image holds the crop (turned too, unless
 * HDRNET_SAMPLE_EVEN_TURNS_ONLY) is the table builder's business (hdrnet_amd/data.py checks it); memory safety depends
 * on neither table: index is clamped to [0, N), turns and flips are masked, and every dword index is clamped to the flat
 * buffer, so a bad record or descriptor gives a wrong sample, never an access outside the buffer.
 * Dtype codes, white levels, the flag, W % 4 == 0, the alignment rules, the return codes, "validation precedes any HIP
 * call" and the B == 0 no-op are hdrnet_prepare_batch's.  One launch, no workspace, no atomics, capturable. */
int hdrnet_prepare_batch_ragged(const void* src_input, int input_dtype, float input_white_level, const void* src_target,
                                int target_dtype, float target_white_level, long long n_samples, const int* images, int N,
                                const int* ops, int B, float* image_input, float* image_target, int H, int W,
                                float* lowres_input, int net_input_size, unsigned flags, void* stream);

#ifdef __cplusplus
} /* extern "C" */
#endif

#endif /* HDRNET_AMD_TRAIN_H_ */
