/* segs_eval.h -- C ABI of the keyframe evaluation (part of libsegs_raster.so; csrc/eval_metrics.hip):
 * the three quality numbers the reference records per keyframe -- SSIM, PSNR and the per-channel PSNR of the original
 * Gaussian-splatting code -- of a rendered image against its target, accumulated into a table on the device, and the three
 * recorded images as bytes.
 *
 * Replaces the tensor chain of GaussianMapper::renderAndRecordKeyframe (src/gaussian_mapper.cpp:1811-1840): the mask (:1811-1815),
 * loss_utils::ssim / psnr / psnr_gaussian_splatting (include/loss_utils.h:39-49, 51-124) with one .item() each (:1816-1818), and
 * the convertTo(CV_8UC3, 255.0f) of the three images (:1820-1840).
 *
 * image, gt: float32 (3, H, W), device pointers.  1 <= H, W <= SEGS_EVAL_MAX_SIZE.  Every entry is stream-ordered, allocates
 * nothing, synchronises nothing and uses no atomics: the same inputs give the same bits in every run.  A null pointer or a size or
 * slot outside the stated ranges returns SEGS_ERR_INVALID_ARGUMENT (text: segs_last_error) before any launch; nothing is touched.
 *
 * ---- The specification: float32 operations, none contracted (built with -ffp-contract=off) -----------------------------------
 * THE MASK (row_mask != 0):  m[c][y] = 1 if any x has gt[c][y][x] != 0 (a NaN counts as non-zero), else 0 -- the reference's
 *     (gt != 0).any(-1) on a CHW tensor: one flag per (channel, row).  row_mask = 0: m = 1 everywhere.
 *     X = image * m      T = gt * m                  (a product, so a NaN or an infinity in a blanked row stays a NaN)
 * THE SUMS, per channel c over the H W pixels:  d = X - T,   A_c = sum |d|,   Q_c = sum d d,   S_c = sum of the SSIM map.
 *     The SSIM map is the one of csrc/loss.hip's forward kernel: the 11-tap window g of loss_utils.h:51-64 applied to X, T, X X,
 *     T T and X T along rows, then along columns, zero padding of 5, every tap sum as a = a + g[k] v[k] from a = 0 in the order
 *     k = 0..10;  S = ((2 mu1 mu2 + C1) (2 s12 + C2)) (1 / ((mu1^2 + mu2^2 + C1) (s11 + s22 + C2))),  C1 = 0.01f 0.01f,  C2 = 0.03f 0.03f.
 *     Every sum is a fixed tree of float32 additions: 1 or 3 in a thread, 6 + 2 in a workgroup, then over the workgroups' slots
 *     at most ceil(slots / 4096) - 1 + 2 in a thread and 6 + 4 in the finishing workgroup.  Up to SEGS_EVAL_MAX_SIZE squared the
 *     longest chain from a term to a channel's sum is 26 additions, 28 to a sum over the three channels.
 * THE ROW, eight float32 words, n = (float)(H W), n3 = (float)(3 H W):
 *     [0] ssim    = ((S_0 + S_1) + S_2) / n3
 *     [3] mse     = ((Q_0 + Q_1) + Q_2) / n3            [4..6] mse_c = Q_c / n
 *     [1] psnr    = 10 log10f(1 / mse)                                         (mse = 0 gives +inf, as in the reference)
 *     [2] psnr_gs = 20 (((p_0 + p_1) + p_2) / 3),   p_c = log10f(1 / sqrtf(mse_c))
 *     [7] l1      = ((A_0 + A_1) + A_2) / n3
 * THE BYTES of a float v (recorded images):  p = v 255.0f;  r = rintf(p) (to nearest, ties to even);  byte = 0 if p is a NaN or
 *     r <= 0, 255 if r >= 255, else (uint8) r -- OpenCV's documented convertTo(CV_8UC3, 255.0f), written from its documentation;
 *     parity with OpenCV's bytes is not claimed.
 */
#ifndef SEGS_EVAL_H_
#define SEGS_EVAL_H_
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define SEGS_EVAL_MAX_SIZE 4096   /* 1 <= H, W <= this */
#define SEGS_EVAL_ROW_WORDS 8     /* ssim, psnr, psnr_gs, mse, mse_r, mse_g, mse_b, l1 */

/* Bytes of the `temp` scratch of an (H, W) evaluation: the 3 H row flags and one slot of partial sums per workgroup.
 * 0 for a size outside the range. */
size_t segs_eval_temp_bytes(int H, int W);

/* One keyframe's row (src/gaussian_mapper.cpp:1811-1818, without the three .item() readbacks): writes the eight words of row
 * `slot` of table, a float32 (n_slots, 8) device array the caller owns, 0 <= slot < n_slots; the other rows are not touched.
 * temp: segs_eval_temp_bytes(H, W) bytes, 16-byte aligned, contents irrelevant on entry.  Launches: the row flags (row_mask
 * != 0 only), the metrics kernel, the one-workgroup finish. */
int segs_eval_frame(const float* image, const float* gt, int H, int W, int row_mask, float* table, int n_slots, int slot,
                    char* temp, void* stream);

/* The recorded images (src/gaussian_mapper.cpp:1820-1840): uint8 (H, W, 3) RGB, the bytes of X, T and |X - T|.  Any of the
 * three output pointers may be null (all three null: nothing is launched).  temp_or_null: with row_mask != 0, the temp of a
 * segs_eval_frame call with row_mask != 0 on the SAME gt, whose row flags are then read instead of being computed again; null:
 * the kernel computes them itself.  One pointwise launch, four pixels per thread. */
int segs_eval_images_u8(const float* image, const float* gt, int H, int W, int row_mask, uint8_t* image_u8, uint8_t* gt_u8,
                        uint8_t* loss_u8, const char* temp_or_null, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SEGS_EVAL_H_ */
