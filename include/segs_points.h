/* segs_points.h -- C ABI of the point-set helpers named by the north star next to the rasterizer
 * (part of libsegs_raster.so): simple-knn, operate_points, stereo_vision.
 *
 * Reference interfaces (C++ ABI over torch::Tensor, no extern "C"):
 *   distCUDA2 / SimpleKNN::knn              third_party/simple-knn/spatial.h:13, simple_knn.h:14-18, simple_knn.cu:185-220
 *   transformPoints, scaleAndTransformThenMarkVisiblePoints   include/operate_points.h:27-40, src/operate_points.cu:73-143
 *   reprojectDepthPinhole, monocularPinholeInactiveGeoDensifyBySearchingNeighborhoodKeypoints
 *                                           include/stereo_vision.h:26-40, src/stereo_vision.cu:136-213
 * All pointers are device pointers; `bool` tensors are passed as bytes; status as in segs_raster.h.
 */
#ifndef SEGS_POINTS_H_
#define SEGS_POINTS_H_
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* SimpleKNN::knn (simple_knn.cu:185-220): mean_dists[i] = mean of the 3 smallest squared distances from point i
 * to the other points.  `temp` holds segs_knn_temp_bytes(P) bytes.  No host synchronisation (the reference copies
 * the bounding box to the host twice and cudaMallocs per call). */
size_t segs_knn_temp_bytes(int P);
int segs_knn_mean_dist2(int P, const float* points /*P,3*/, float* mean_dists /*P*/, char* temp, void* stream);

/* transform_points (operate_points.cu:38-50): out = M * p with the transposed-layout 4x4 of auxiliary.h:59-67. */
int segs_transform_points(int P, const float* points, const float* transformmatrix, float* out_points, void* stream);

/* scale_and_transform_points (operate_points.cu:52-71): for mask[i] != 0, out_points[i] = M * (scale * p_i) and
 * out_rots[i] = quaternion of (M_rot * R(q_i)) (Shoemake).  The reference's insert_rot_to_rots writes element +2
 * twice and never +3 (cuda_rasterizer/operate_points.h:175-178); that behaviour is kept: out_rots[i] = (w, x, z, untouched). */
int segs_scale_and_transform_points(int P, float scale, const float* points, const float* rots, const float* transformmatrix,
                                    const uint8_t* mask, float* out_points, float* out_rots, void* stream);

/* reproject_depths_pinhole (stereo_vision.cu:39-61): pixel idx = v*width+u -> ((u-cx)*d/fx, (v-cy)*d/fy, d) where mask. */
int segs_reproject_depths_pinhole(int P, int width, float fx, float fy, float cx, float cy, const float* depths,
                                  const uint8_t* mask, float* points, void* stream);

/* search_neighborhood_to_estimate_depth_and_reproject_pinhole (stereo_vision.cu:63-134), quirks kept: the colour index
 * is v*width+u (not x3) and max_pixel_dist is compared with the SQUARED pixel distance. */
int segs_search_neighborhood_depth(int N, int width, float fx, float fy, float cx, float cy, float max_pixel_dist,
                                   const float* pixels /*N,2*/, const uint8_t* has3D, const float* point3D_orig /*N,3*/,
                                   const float* colors, float* point3D_result /*N,3*/, float* colors_result /*N,3*/, void* stream);

/* ---- stereo frames as depth frames: semi-global matching (csrc/stereo_sgm.hip; specification in DESIGN.md 3i).
 * What the reference asks of cv::cuda::StereoSGM (src/gaussian_mapper.cpp:93-95, 1591-1610), written from the published
 * algorithm (Hirschmueller's SGM over a centre-symmetric 9x7 census cost); parity with OpenCV's bytes is not claimed.
 * Integer arithmetic throughout, a fixed launch sequence and no float atomics: the same inputs give the same bytes. */
typedef struct SegsStereoParams {
  int num_disparities;   /* D: 64, 128 or 256 */
  int min_disparity;     /* dmin >= 0, D + dmin <= 2047 */
  int P1, P2;            /* 0 <= P1 <= P2 <= 224: a path cost fits 8 bits */
  int uniqueness_ratio;  /* u in [0, 100); 0 = off */
  int paths;             /* 4 or 8 */
  int lr_max_diff;       /* >= -1; -1 = no left-right check */
  int median;            /* 0 or 1: 3x3 median of the raw disparities */
} SegsStereoParams;

/* Scratch of one call: the two census maps, the summed path costs S (H x W x D uint16, d fastest), the raw disparity before and
 * after the median, and the right view's disparity.  0 for sizes segs_stereo_sgm refuses. */
size_t segs_stereo_sgm_temp_bytes(int W, int H, int D, int paths);

/* left, right: (H, W) uint8, rectified.  disp16: (H, W) int16 = 16 x disparity (4 fractional bits, min_disparity included) where
 * valid and 16 (min_disparity - 1) where not, so that the reference's own test `disp / 16 > min_disparity` drops the invalid
 * pixels.  depth (may be NULL): (H, W) float32 = fb16 / (float)disp16 where valid and disp16 > 0, else 0 -- the "no measurement"
 * of segs_depth_target; fb16 = 16 fx baseline.  1 <= W, H <= 4096.  Any parameter outside the ranges above returns
 * SEGS_ERR_INVALID_ARGUMENT before any launch.  No host synchronisation and no allocation. */
int segs_stereo_sgm(const SegsStereoParams* params, int W, int H, const uint8_t* left, const uint8_t* right, int16_t* disp16,
                    float* depth, float fb16, char* temp, void* stream);

/* cvtColor(RGB2GRAY) + convertTo(CV_8UC1, 255) of src/gaussian_mapper.cpp:1599-1603 on a (3, H, W) float32 image:
 * g = (0.299f R + 0.587f G) + 0.114f B, out = (uint8) min(max(rintf(255 g), 0), 255); NaN gives 0. */
int segs_rgb_to_gray_u8(int W, int H, const float* rgb, uint8_t* out, void* stream);

/* segs_stereo_sgm, and afterwards copies of its stages (each pointer may be NULL): the census maps (H, W) uint32, S (H, W, D)
 * uint16, the raw disparity after the winner stage and after the median (H, W) uint16 (equal when median = 0; 0xFFFF = invalid),
 * and the right view's disparity (H, W) int16 (-1 = none). */
int segs_debug_stereo_sgm_stages(const SegsStereoParams* params, int W, int H, const uint8_t* left, const uint8_t* right,
                                 int16_t* disp16, float* depth, float fb16, char* temp, uint32_t* census_left,
                                 uint32_t* census_right, uint16_t* S, uint16_t* raw_winner, uint16_t* raw_median,
                                 int16_t* disp_right, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SEGS_POINTS_H_ */
