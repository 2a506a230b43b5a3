/* segs_frame_intake.h -- C ABI of the frame intake (part of libsegs_raster.so; csrc/frame_intake.hip):
 * a camera frame as the sensor delivers it -> the undistorted, rectified float32 CHW image, its grey bytes, the depth map,
 * the validity mask and the Gaussian-pyramid levels that the step, the stereo matcher, the depth loss and the depth seeding take.
 *
 * What the reference does with OpenCV on the host (Camera::initUndistortRectifyMapAndMask / undistortImage, include/camera.h:71-115;
 * the cv::cuda::resize loops of src/gaussian_mapper.cpp:623-631, 1286-1297), written from OpenCV's documentation of
 * initUndistortRectifyMap, remap (INTER_LINEAR, constant border 0) and resize (INTER_LINEAR), not from its code; parity with
 * OpenCV's bytes (fixed-point remap weights) is not claimed.  The map is computed per pixel in registers and never stored.
 *
 * Camera model: pinhole with OpenCV's five coefficients (k1, k2, p1, p2, k3) -- every `Camera.type: "PinHole"` settings file.
 * The fisheye (Kannala-Brandt) model is NOT supported, as in the reference (src/gaussian_mapper.cpp:205-207).
 *
 * All image pointers are device pointers; the structs and the arrays of segs_resize_levels are host memory, read during the call.
 * Every entry is stream-ordered, allocates nothing, synchronises nothing, uses no atomics and may be captured into a graph.
 * A null pointer or a size outside the stated ranges returns SEGS_ERR_INVALID_ARGUMENT (text: segs_last_error) before any launch.
 *
 * ---- The specification: float32 operations in this order, none contracted (built with -ffp-contract=off) -------------------
 * THE MAP of output pixel (u, v), 0 <= u < out_w, 0 <= v < out_h; every name is a float32:
 *     x  = ((float)u - ncx) / nfx                     y  = ((float)v - ncy) / nfy
 *     X  = (rinv[0] x + rinv[1] y) + rinv[2]
 *     Y  = (rinv[3] x + rinv[4] y) + rinv[5]
 *     Wc = (rinv[6] x + rinv[7] y) + rinv[8]
 *     x1 = X / Wc                                     y1 = Y / Wc
 *     x2 = x1 x1        y2 = y1 y1        r2 = x2 + y2        xy2 = (2 x1) y1
 *     kr = 1 + r2 (k1 + r2 (k2 + r2 k3))                          (innermost product first)
 *     xd = (x1 kr + p1 xy2) + p2 (r2 + 2 x2)
 *     yd = (y1 kr + p1 (r2 + 2 y2)) + p2 xy2
 *     mx = fx xd + cx                                 my = fy yd + cy
 * THE SAMPLER of a source (in_h, in_w) at (mx, my):
 *     reach = mx > -1 and mx < (float)in_w and my > -1 and my < (float)in_h        (false for a NaN coordinate)
 *     without reach all four taps are outside: the result is 0 (image, grey, depth, mask alike) and nothing is read.
 *     x0 = floorf(mx)   ax = mx - x0   bx = 1 - ax          y0 = floorf(my)   ay = my - y0   by = 1 - ay
 *     w00 = bx by    w01 = ax by    w10 = bx ay    w11 = ax ay         taps t00 (x0, y0)  t01 (x0+1, y0)  t10 (x0, y0+1)  t11 (x0+1, y0+1)
 *     a tap outside the source reads as 0 (cv::remap's default constant border)
 *     sum = ((t00 w00 + t01 w01) + t10 w10) + t11 w11
 * THE RESIZE of a (C, H, W) image to a level (C, h, w), output pixel (x, y):
 *     sx = ((float)x + 0.5) ((float)W / (float)w) - 0.5       x0 = floorf(sx)   ax = sx - x0   bx = 1 - ax      (y alike with H, h)
 *     taps at columns clamp(x0, 0, W-1), clamp(x0+1, 0, W-1) and rows alike (replicate); weights and sum as in the sampler.
 *     No antialiasing: cv::cuda::resize with its default INTER_LINEAR.
 */
#ifndef SEGS_FRAME_INTAKE_H_
#define SEGS_FRAME_INTAKE_H_
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define SEGS_INTAKE_MAX_SIZE 8192   /* 1 <= in_w, in_h, out_w, out_h, level sizes <= this */
#define SEGS_INTAKE_MAX_LEVELS 8    /* levels of one segs_resize_levels call */

/* The camera as the kernels take it: every float is the float64 calibration value rounded once to float32 by the host. */
typedef struct SegsIntakeCamera {
  int in_w, in_h;              /* the source frame */
  int out_w, out_h;            /* the new camera's image */
  float fx, fy, cx, cy;        /* the source camera */
  float k1, k2, p1, p2, k3;    /* OpenCV's order of the five coefficients */
  float rinv[9];               /* inverse of the rectifying rotation R, row-major (identity: no rectification) */
  float nfx, nfy, ncx, ncy;    /* the new camera; nfx, nfy non-zero.  Every float must be finite. */
} SegsIntakeCamera;

/* src: uint8 (in_h, in_w, C) interleaved, C = 1 or 3.  out: float32 (C, out_h, out_w) = sum / 255 with taps (float)byte.
 * gray (may be NULL): uint8 (out_h, out_w).  C = 3: the bytes of segs_rgb_to_gray_u8 on `out`, i.e. g = (0.299f R + 0.587f G) +
 * 0.114f B of the three float outputs, byte = (uint8) min(max(rintf(g 255), 0), 255).  C = 1: the same rounding of the one output,
 * (uint8) min(max(rintf(out 255), 0), 255).  rintf rounds to nearest, ties to even. */
int segs_undistort_u8(const SegsIntakeCamera* cam, int C, const uint8_t* src, float* out, uint8_t* gray, void* stream);

/* src: (in_h, in_w) uint16 (src_is_float = 0) or float32 (src_is_float = 1); taps are (float)raw * inv_factor, inv_factor =
 * 1 / RGBD.DepthMapFactor.  out: float32 (out_h, out_w).  hole_aware = 0: the sum, the reference's undistortImage(imgAux)
 * (src/gaussian_mapper.cpp:1262-1263).  hole_aware = 1: 0 wherever a tap of non-zero weight lies outside the source or has
 * raw <= 0 (a NaN raw counts as a hole), else the sum: a hole is never averaged into a depth. */
int segs_undistort_depth(const SegsIntakeCamera* cam, int src_is_float, const void* src, float inv_factor, int hole_aware,
                         float* out, void* stream);

/* Camera::undistort_mask: the remap of an all-ones image, i.e. the sum with t = 1 inside the source and 0 outside.
 * out: float32 (out_h, out_w). */
int segs_undistort_mask(const SegsIntakeCamera* cam, float* out, void* stream);

/* The map itself, for tests and inspection: out (out_h, out_w, 2) float32 = (mx, my). */
int segs_debug_undistort_map(const SegsIntakeCamera* cam, float* out, void* stream);

/* Every level of one image in one launch.  src: float32 (C, H, W), C = 1 or 3.  widths, heights, outs: host arrays of n_levels
 * entries (1 <= n_levels <= SEGS_INTAKE_MAX_LEVELS); outs[l] is the device pointer of level l, float32 (C, heights[l], widths[l]). */
int segs_resize_levels(int C, int W, int H, const float* src, int n_levels, const int* widths, const int* heights,
                       float* const* outs, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SEGS_FRAME_INTAKE_H_ */
