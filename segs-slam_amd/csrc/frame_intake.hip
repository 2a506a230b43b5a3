// frame_intake.hip -- a camera frame to what the step takes (include/segs_frame_intake.h holds the specification).
// The reference's Camera::undistortImage / initUndistortRectifyMapAndMask (include/camera.h:71-115) and its cv::cuda::resize pyramid
// loops (src/gaussian_mapper.cpp:623-631, 1286-1297), written from OpenCV's documentation.  Pinhole model with five coefficients;
// the fisheye model is not supported, as in the reference (src/gaussian_mapper.cpp:205-207).
// Built with -ffp-contract=off: the float32 operations the header states are the ones that run.  Launches:
//   undistort_kernel<MODE, C> : one launch per frame.  Workgroup = 64 x 4 output pixels, a wave = 64 consecutive x of one row, so
//                               every channel's float store of a wave is one contiguous 256-byte segment.  The map is computed in
//                               registers from the camera in the kernel arguments; the taps are gathers whose neighbouring lanes
//                               share cache lines (no LDS staging).
//   resize_levels_kernel<C>   : one launch for every level; a workgroup finds its level by the prefix table in the arguments.
// Every address is bounded by construction: a tap is loaded only after its own bounds test, and a lane past the image's edge returns
// before it forms an address.
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdint>
#include "../../include/segs_raster.h"
#include "../../include/segs_frame_intake.h"
#include "kernels.h"

#pragma clang fp contract(off)

namespace {

constexpr int TILE_W = 64, TILE_H = 4;

enum Mode { MODE_U8 = 0, MODE_DEPTH_U16 = 1, MODE_DEPTH_F32 = 2, MODE_MASK = 3, MODE_MAP = 4 };

struct Taps {
  bool reach;
  int x0, y0;
  float w00, w01, w10, w11;
  bool in00, in01, in10, in11;
};

__device__ __forceinline__ void camera_map(const SegsIntakeCamera& c, int u, int v, float& mx, float& my) {
  const float x = ((float)u - c.ncx) / c.nfx;
  const float y = ((float)v - c.ncy) / c.nfy;
  const float X = (c.rinv[0] * x + c.rinv[1] * y) + c.rinv[2];
  const float Y = (c.rinv[3] * x + c.rinv[4] * y) + c.rinv[5];
  const float Wc = (c.rinv[6] * x + c.rinv[7] * y) + c.rinv[8];
  const float x1 = X / Wc, y1 = Y / Wc;
  const float x2 = x1 * x1, y2 = y1 * y1;
  const float r2 = x2 + y2;
  const float xy2 = (2.0f * x1) * y1;
  const float kr = 1.0f + r2 * (c.k1 + r2 * (c.k2 + r2 * c.k3));
  const float xd = (x1 * kr + c.p1 * xy2) + c.p2 * (r2 + 2.0f * x2);
  const float yd = (y1 * kr + c.p1 * (r2 + 2.0f * y2)) + c.p2 * xy2;
  mx = c.fx * xd + c.cx;
  my = c.fy * yd + c.cy;
}

__device__ __forceinline__ Taps make_taps(float mx, float my, int in_w, int in_h) {
  Taps t{};
  t.reach = mx > -1.0f && mx < (float)in_w && my > -1.0f && my < (float)in_h;   // false for NaN: x0, y0 below are then unused
  if (!t.reach) return t;
  const float fx0 = floorf(mx), fy0 = floorf(my);
  const float ax = mx - fx0, ay = my - fy0;
  const float bx = 1.0f - ax, by = 1.0f - ay;
  t.x0 = (int)fx0;                      // in [-1, in_w - 1]
  t.y0 = (int)fy0;                      // in [-1, in_h - 1]
  t.w00 = bx * by; t.w01 = ax * by; t.w10 = bx * ay; t.w11 = ax * ay;
  const bool xl = t.x0 >= 0, xr = t.x0 + 1 < in_w, yt = t.y0 >= 0, yb = t.y0 + 1 < in_h;
  t.in00 = xl && yt; t.in01 = xr && yt; t.in10 = xl && yb; t.in11 = xr && yb;
  return t;
}

__device__ __forceinline__ float weighted(const Taps& t, float t00, float t01, float t10, float t11) {
  return ((t00 * t.w00 + t01 * t.w01) + t10 * t.w10) + t11 * t.w11;
}

__device__ __forceinline__ uint8_t to_byte(float v) {   // fmaxf(NaN, 0) = 0
  return (uint8_t)fminf(fmaxf(rintf(v * 255.0f), 0.0f), 255.0f);
}

template <typename T> __device__ __forceinline__ float load_tap(const T* __restrict__ src, bool in, int idx) {
  return in ? (float)src[idx] : 0.0f;   // the index is formed and used only inside the source
}

template <int MODE, int C>
__global__ void __launch_bounds__(TILE_W * TILE_H) undistort_kernel(SegsIntakeCamera cam, const void* __restrict__ src_, float* __restrict__ out,
                                                                    uint8_t* __restrict__ gray, float inv_factor, int hole_aware) {
  const int u = blockIdx.x * TILE_W + (threadIdx.x & (TILE_W - 1));
  const int v = blockIdx.y * TILE_H + (threadIdx.x >> 6);
  if (u >= cam.out_w || v >= cam.out_h) return;
  const int pix = v * cam.out_w + u;
  const int plane = cam.out_w * cam.out_h;
  float mx, my;
  camera_map(cam, u, v, mx, my);
  if (MODE == MODE_MAP) {
    *reinterpret_cast<float2*>(out + 2 * (size_t)pix) = make_float2(mx, my);
    return;
  }
  const Taps t = make_taps(mx, my, cam.in_w, cam.in_h);
  const int i00 = t.y0 * cam.in_w + t.x0, i01 = i00 + 1, i10 = i00 + cam.in_w, i11 = i10 + 1;   // used only where in.. holds
  if (MODE == MODE_MASK) {
    out[pix] = t.reach ? weighted(t, t.in00 ? 1.0f : 0.0f, t.in01 ? 1.0f : 0.0f, t.in10 ? 1.0f : 0.0f, t.in11 ? 1.0f : 0.0f) : 0.0f;
  } else if (MODE == MODE_U8) {
    const uint8_t* __restrict__ src = static_cast<const uint8_t*>(src_);
    float val[C];
#pragma unroll
    for (int c = 0; c < C; c++) {
      float s = 0.0f;
      if (t.reach)
        s = weighted(t, load_tap(src, t.in00, i00 * C + c), load_tap(src, t.in01, i01 * C + c), load_tap(src, t.in10, i10 * C + c),
                     load_tap(src, t.in11, i11 * C + c));
      val[c] = s / 255.0f;
      out[(size_t)c * plane + pix] = val[c];
    }
    if (gray) gray[pix] = to_byte(C == 3 ? (0.299f * val[0] + 0.587f * val[C > 1 ? 1 : 0]) + 0.114f * val[C > 2 ? 2 : 0] : val[0]);
  } else {
    float raw[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    if (t.reach) {
      if (MODE == MODE_DEPTH_U16) {
        const uint16_t* __restrict__ src = static_cast<const uint16_t*>(src_);
        raw[0] = load_tap(src, t.in00, i00); raw[1] = load_tap(src, t.in01, i01);
        raw[2] = load_tap(src, t.in10, i10); raw[3] = load_tap(src, t.in11, i11);
      } else {
        const float* __restrict__ src = static_cast<const float*>(src_);
        raw[0] = load_tap(src, t.in00, i00); raw[1] = load_tap(src, t.in01, i01);
        raw[2] = load_tap(src, t.in10, i10); raw[3] = load_tap(src, t.in11, i11);
      }
    }
    float s = 0.0f;
    if (t.reach) {
      s = weighted(t, raw[0] * inv_factor, raw[1] * inv_factor, raw[2] * inv_factor, raw[3] * inv_factor);
      if (hole_aware) {
        // an outside tap has raw = 0 here, so `!(raw > 0)` covers outside, zero, negative and NaN alike
        const bool hole = (t.w00 != 0.0f && !(raw[0] > 0.0f)) || (t.w01 != 0.0f && !(raw[1] > 0.0f)) ||
                          (t.w10 != 0.0f && !(raw[2] > 0.0f)) || (t.w11 != 0.0f && !(raw[3] > 0.0f));
        if (hole) s = 0.0f;
      }
    }
    out[pix] = s;
  }
}

struct LevelTable {
  int n;
  int w[SEGS_INTAKE_MAX_LEVELS], h[SEGS_INTAKE_MAX_LEVELS];
  int first_block[SEGS_INTAKE_MAX_LEVELS + 1];   // workgroups of the levels before this one
  float* out[SEGS_INTAKE_MAX_LEVELS];
};

template <int C>
__global__ void __launch_bounds__(TILE_W * TILE_H) resize_levels_kernel(int W, int H, const float* __restrict__ src, LevelTable tab) {
  int l = 0;
  while (l + 1 < tab.n && (int)blockIdx.x >= tab.first_block[l + 1]) l++;   // uniform over the workgroup
  const int w = tab.w[l], h = tab.h[l];
  const int b = blockIdx.x - tab.first_block[l];
  const int bw = (w + TILE_W - 1) / TILE_W;
  const int by_ = b / bw, bx_ = b - by_ * bw;
  const int x = bx_ * TILE_W + (threadIdx.x & (TILE_W - 1));
  const int y = by_ * TILE_H + (threadIdx.x >> 6);
  if (x >= w || y >= h) return;
  const float sx = ((float)x + 0.5f) * ((float)W / (float)w) - 0.5f;
  const float sy = ((float)y + 0.5f) * ((float)H / (float)h) - 0.5f;
  const float fx0 = floorf(sx), fy0 = floorf(sy);
  const float ax = sx - fx0, ay = sy - fy0;
  const float bx = 1.0f - ax, by = 1.0f - ay;
  const float w00 = bx * by, w01 = ax * by, w10 = bx * ay, w11 = ax * ay;
  // sx lies in (-0.5, W): fx0 in [-1, W - 1]; the clamp makes every column and row one of the image's
  const int x0 = (int)fx0, y0 = (int)fy0;
  const int xa = min(max(x0, 0), W - 1), xb = min(max(x0 + 1, 0), W - 1);
  const int ya = min(max(y0, 0), H - 1), yb = min(max(y0 + 1, 0), H - 1);
  float* __restrict__ out = tab.out[l];
#pragma unroll
  for (int c = 0; c < C; c++) {
    const float* __restrict__ p = src + (size_t)c * W * H;
    const float t00 = p[ya * W + xa], t01 = p[ya * W + xb], t10 = p[yb * W + xa], t11 = p[yb * W + xb];
    out[(size_t)c * w * h + y * w + x] = ((t00 * w00 + t01 * w01) + t10 * w10) + t11 * w11;
  }
}

int bad(const char* what) { return segs::set_error(SEGS_ERR_INVALID_ARGUMENT, what); }
#define LAUNCH_OK() do { hipError_t _e = hipGetLastError(); if (_e != hipSuccess) return segs::set_error((int)_e, hipGetErrorString(_e)); } while (0)

bool size_ok(int n) { return n >= 1 && n <= SEGS_INTAKE_MAX_SIZE; }

// null when the camera can be launched, else the reason
const char* camera_fault(const SegsIntakeCamera* cam) {
  if (!cam) return "frame intake: null camera";
  if (!size_ok(cam->in_w) || !size_ok(cam->in_h) || !size_ok(cam->out_w) || !size_ok(cam->out_h))
    return "frame intake: 1 <= in_w, in_h, out_w, out_h <= 8192";
  const float f[] = {cam->fx, cam->fy, cam->cx, cam->cy, cam->k1, cam->k2, cam->p1, cam->p2, cam->k3, cam->nfx, cam->nfy, cam->ncx, cam->ncy};
  for (float v : f) if (!std::isfinite(v)) return "frame intake: every camera parameter must be finite";
  for (float v : cam->rinv) if (!std::isfinite(v)) return "frame intake: every camera parameter must be finite";
  if (cam->nfx == 0.0f || cam->nfy == 0.0f) return "frame intake: the new camera's focal lengths must be non-zero";
  return nullptr;
}

dim3 tiles(const SegsIntakeCamera& cam) { return dim3((cam.out_w + TILE_W - 1) / TILE_W, (cam.out_h + TILE_H - 1) / TILE_H); }

}  // namespace

extern "C" {

int segs_undistort_u8(const SegsIntakeCamera* cam, int C, const uint8_t* src, float* out, uint8_t* gray, void* stream) {
  if (const char* why = camera_fault(cam)) return bad(why);
  if (C != 1 && C != 3) return bad("segs_undistort_u8: C must be 1 or 3");
  if (!src || !out) return bad("segs_undistort_u8: null pointer");
  hipStream_t st = (hipStream_t)stream;
  if (C == 3) undistort_kernel<MODE_U8, 3><<<tiles(*cam), TILE_W * TILE_H, 0, st>>>(*cam, src, out, gray, 0.0f, 0);
  else        undistort_kernel<MODE_U8, 1><<<tiles(*cam), TILE_W * TILE_H, 0, st>>>(*cam, src, out, gray, 0.0f, 0);
  LAUNCH_OK();
  return SEGS_OK;
}

int segs_undistort_depth(const SegsIntakeCamera* cam, int src_is_float, const void* src, float inv_factor, int hole_aware,
                         float* out, void* stream) {
  if (const char* why = camera_fault(cam)) return bad(why);
  if ((src_is_float != 0 && src_is_float != 1) || (hole_aware != 0 && hole_aware != 1))
    return bad("segs_undistort_depth: src_is_float and hole_aware are 0 or 1");
  if (!std::isfinite(inv_factor)) return bad("segs_undistort_depth: inv_factor must be finite");
  if (!src || !out) return bad("segs_undistort_depth: null pointer");
  hipStream_t st = (hipStream_t)stream;
  if (src_is_float) undistort_kernel<MODE_DEPTH_F32, 1><<<tiles(*cam), TILE_W * TILE_H, 0, st>>>(*cam, src, out, nullptr, inv_factor, hole_aware);
  else              undistort_kernel<MODE_DEPTH_U16, 1><<<tiles(*cam), TILE_W * TILE_H, 0, st>>>(*cam, src, out, nullptr, inv_factor, hole_aware);
  LAUNCH_OK();
  return SEGS_OK;
}

int segs_undistort_mask(const SegsIntakeCamera* cam, float* out, void* stream) {
  if (const char* why = camera_fault(cam)) return bad(why);
  if (!out) return bad("segs_undistort_mask: null pointer");
  undistort_kernel<MODE_MASK, 1><<<tiles(*cam), TILE_W * TILE_H, 0, (hipStream_t)stream>>>(*cam, nullptr, out, nullptr, 0.0f, 0);
  LAUNCH_OK();
  return SEGS_OK;
}

int segs_debug_undistort_map(const SegsIntakeCamera* cam, float* out, void* stream) {
  if (const char* why = camera_fault(cam)) return bad(why);
  if (!out) return bad("segs_debug_undistort_map: null pointer");
  undistort_kernel<MODE_MAP, 1><<<tiles(*cam), TILE_W * TILE_H, 0, (hipStream_t)stream>>>(*cam, nullptr, out, nullptr, 0.0f, 0);
  LAUNCH_OK();
  return SEGS_OK;
}

int segs_resize_levels(int C, int W, int H, const float* src, int n_levels, const int* widths, const int* heights,
                       float* const* outs, void* stream) {
  if (C != 1 && C != 3) return bad("segs_resize_levels: C must be 1 or 3");
  if (!size_ok(W) || !size_ok(H)) return bad("segs_resize_levels: 1 <= W, H <= 8192");
  if (n_levels < 1 || n_levels > SEGS_INTAKE_MAX_LEVELS) return bad("segs_resize_levels: 1 <= n_levels <= 8");
  if (!src || !widths || !heights || !outs) return bad("segs_resize_levels: null pointer");
  LevelTable tab{};
  tab.n = n_levels;
  int blocks = 0;
  for (int l = 0; l < n_levels; l++) {
    if (!size_ok(widths[l]) || !size_ok(heights[l])) return bad("segs_resize_levels: 1 <= level width, height <= 8192");
    if (!outs[l]) return bad("segs_resize_levels: null level pointer");
    tab.w[l] = widths[l]; tab.h[l] = heights[l]; tab.out[l] = outs[l];
    tab.first_block[l] = blocks;
    blocks += ((widths[l] + TILE_W - 1) / TILE_W) * ((heights[l] + TILE_H - 1) / TILE_H);   // at most 128 * 2048 per level
  }
  tab.first_block[n_levels] = blocks;
  hipStream_t st = (hipStream_t)stream;
  if (C == 3) resize_levels_kernel<3><<<blocks, TILE_W * TILE_H, 0, st>>>(W, H, src, tab);
  else        resize_levels_kernel<1><<<blocks, TILE_W * TILE_H, 0, st>>>(W, H, src, tab);
  LAUNCH_OK();
  return SEGS_OK;
}

}  // extern "C"
