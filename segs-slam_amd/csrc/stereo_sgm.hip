// stereo_sgm.hip -- semi-global matching of a rectified stereo pair (include/segs_points.h; specification: DESIGN.md 3i).
// What the reference asks of cv::cuda::StereoSGM (src/gaussian_mapper.cpp:93-95, 1591-1610), written from the published
// algorithm: centre-symmetric 9x7 census, Hamming cost, 4 or 8 aggregation paths, winner with uniqueness and sub-pixel
// fit, 3x3 median, left-right check.  Integer arithmetic except the grey conversion and the final division (built with
// -ffp-contract=off for those two).  Launches of one call, in order:
//   census_kernel        : both images, thread = pixel
//   sgm_path_kernel<K>   : one launch per direction (4 or 8).  A wave owns one line of the image -- a row for the horizontal
//                          directions, a start column for the others -- and walks it serially with the D = 64 K disparities on
//                          its lanes, K adjacent ones per lane.  The first launch stores L_r into S, the others add into it:
//                          launches of one stream are ordered, so there are no atomics and S is the same on every run.
//   winner_kernel        : wave = pixel; argmin, uniqueness, sub-pixel fit
//   right_view_kernel    : wave = pixel of the right view; argmin along the (x, d) diagonal of S
//   median_kernel        : thread = pixel (skipped with median = 0)
//   check_output_kernel  : thread = pixel; left-right check, disp16, depth
// Every address is bounded by construction: x - d - dmin < 0 and xr + d + dmin >= W select a constant instead of a load.
#include <hip/hip_runtime.h>
#include <cstdint>
#include "../../include/segs_raster.h"
#include "../../include/segs_points.h"
#include "kernels.h"
#include "gs_layout.h"

#pragma clang fp contract(off)

namespace {

constexpr int DPP_ROW_ROR = 0x120;    // row_ror:n  = 0x120 + n: rotation inside a row of 16 lanes
constexpr int DPP_WAVE_SHL1 = 0x130;  // lane i reads lane i + 1; lane 63 keeps `old`
constexpr int DPP_WAVE_SHR1 = 0x138;  // lane i reads lane i - 1; lane 0 keeps `old`
constexpr int FAR = 0x3FFF;           // larger than any path cost or S, small enough to add P1 to
constexpr uint32_t RAW_INVALID = 0xFFFFu;

// Minimum over the 64 lanes, the same value in every lane.  min is idempotent, so four rotations inside each row of 16 lanes
// leave the row's minimum in all of its lanes (no masks needed); the four rows meet through SGPRs.  All lanes must be active.
__device__ __forceinline__ int wave_min(int v) {
  v = min(v, __builtin_amdgcn_update_dpp(v, v, DPP_ROW_ROR + 1, 0xf, 0xf, false));
  v = min(v, __builtin_amdgcn_update_dpp(v, v, DPP_ROW_ROR + 2, 0xf, 0xf, false));
  v = min(v, __builtin_amdgcn_update_dpp(v, v, DPP_ROW_ROR + 4, 0xf, 0xf, false));
  v = min(v, __builtin_amdgcn_update_dpp(v, v, DPP_ROW_ROR + 8, 0xf, 0xf, false));
  return min(min(__builtin_amdgcn_readlane(v, 0), __builtin_amdgcn_readlane(v, 16)),
             min(__builtin_amdgcn_readlane(v, 32), __builtin_amdgcn_readlane(v, 48)));
}

// ---------------------------------------------------------------- stage 1: grey
__global__ void __launch_bounds__(256) rgb_to_gray_kernel(int n, const float* __restrict__ rgb, uint8_t* __restrict__ out) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const float r = rgb[i], g = rgb[(size_t)n + i], b = rgb[2 * (size_t)n + i];
  const float y = (0.299f * r + 0.587f * g) + 0.114f * b;
  const float q = fminf(fmaxf(rintf(y * 255.0f), 0.0f), 255.0f);   // fmaxf(NaN, 0) = 0
  out[i] = (uint8_t)q;
}

// ---------------------------------------------------------------- stage 2: census
// 31 comparisons I(y+dy, x+dx) > I(y-dy, x-dx), offsets in raster order: dy = -3..-1 with dx = -4..4, then dy = 0 with dx = -4..-1.
__global__ void __launch_bounds__(256) census_kernel(int W, int H, const uint8_t* __restrict__ left, const uint8_t* __restrict__ right,
                                                     uint32_t* __restrict__ cl, uint32_t* __restrict__ cr) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= W * H) return;
  const uint8_t* __restrict__ img = blockIdx.y ? right : left;
  uint32_t* __restrict__ out = blockIdx.y ? cr : cl;
  const int y = i / W, x = i - y * W;
  uint32_t bits = 0;
  if (x >= 4 && x < W - 4 && y >= 3 && y < H - 3) {
    int bit = 0;
#pragma unroll
    for (int dy = -3; dy <= 0; dy++)
#pragma unroll
      for (int dx = -4; dx <= (dy < 0 ? 4 : -1); dx++, bit++)
        bits |= (uint32_t)(img[(y + dy) * W + (x + dx)] > img[(y - dy) * W + (x - dx)]) << bit;
  }
  out[i] = bits;
}

// ---------------------------------------------------------------- stages 3 + 4: cost and one path direction
template <int K> struct SRun;   // K adjacent uint16 of S, moved as one word
template <> struct SRun<1> { using type = uint16_t; };
template <> struct SRun<2> { using type = uint32_t; };
template <> struct SRun<4> { using type = uint2; };

template <int K> __device__ __forceinline__ void unpack_run(typename SRun<K>::type w, int (&v)[K]);
template <> __device__ __forceinline__ void unpack_run<1>(uint16_t w, int (&v)[1]) { v[0] = w; }
template <> __device__ __forceinline__ void unpack_run<2>(uint32_t w, int (&v)[2]) { v[0] = w & 0xFFFFu; v[1] = w >> 16; }
template <> __device__ __forceinline__ void unpack_run<4>(uint2 w, int (&v)[4]) {
  v[0] = w.x & 0xFFFFu; v[1] = w.x >> 16; v[2] = w.y & 0xFFFFu; v[3] = w.y >> 16;
}
template <int K> __device__ __forceinline__ typename SRun<K>::type pack_run(const int (&v)[K]);
template <> __device__ __forceinline__ uint16_t pack_run<1>(const int (&v)[1]) { return (uint16_t)v[0]; }
template <> __device__ __forceinline__ uint32_t pack_run<2>(const int (&v)[2]) { return (uint32_t)v[0] | ((uint32_t)v[1] << 16); }
template <> __device__ __forceinline__ uint2 pack_run<4>(const int (&v)[4]) {
  return make_uint2((uint32_t)v[0] | ((uint32_t)v[1] << 16), (uint32_t)v[2] | ((uint32_t)v[3] << 16));
}

constexpr int PATH_WAVES = 4;    // lines (rows or start columns) of one workgroup: adjacent, so that S is touched in adjacent runs
constexpr int PATH_AHEAD = 4;    // steps whose census words and S runs are requested together, ahead of the serial recurrence

// One direction r = (dx, dy).  dy == 0: line = row, the walk starts at x = 0 (dx > 0) or W - 1.  dy != 0: line = start column, the
// walk starts in row 0 (dy > 0) or H - 1 and moves dx columns per row, wrapping at the image's edge; a wrap restarts the
// recurrence, because the predecessor p - r of the pixel behind the wrap lies outside the image.  Each row's W pixels are
// visited by W different lines, so every pixel takes its L_r exactly once.
// Lane l holds d = l K .. l K + K - 1 of L_r(p - r, .): the d +- 1 neighbours across lanes come by a whole-wave DPP shift, m by
// wave_min; no LDS in the recurrence.  Control flow is uniform over the wave throughout (DPP needs every lane active).
template <int K>
__global__ void __launch_bounds__(64 * PATH_WAVES) sgm_path_kernel(int W, int H, int dmin, int P1, int P2, int dx, int dy, int first,
                                                                   const uint32_t* __restrict__ cl, const uint32_t* __restrict__ cr,
                                                                   uint16_t* __restrict__ S) {
  using Run = typename SRun<K>::type;
  constexpr int D = 64 * K;
  const int lane = threadIdx.x & 63;
  const int line = blockIdx.x * PATH_WAVES + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int nlines = dy == 0 ? H : W, steps = dy == 0 ? W : H;
  if (line >= nlines) return;
  int x, y;
  if (dy == 0) { y = line; x = dx > 0 ? 0 : W - 1; }
  else         { x = line; y = dy > 0 ? 0 : H - 1; }
  const int d0 = lane * K + dmin;          // x - d0 - k is the right image's column of this lane's k-th disparity
  int Lp[K];
#pragma unroll
  for (int k = 0; k < K; k++) Lp[k] = 0;
  int m = 0;
  bool restart = true;

  for (int t0 = 0; t0 < steps; t0 += PATH_AHEAD) {
    int pix[PATH_AHEAD];
    bool rs[PATH_AHEAD];
    uint32_t wl[PATH_AHEAD], wr[PATH_AHEAD][K];
    Run old[PATH_AHEAD];
#pragma unroll
    for (int u = 0; u < PATH_AHEAD; u++) {
      if (t0 + u < steps) {                 // 0 <= x < W and 0 <= y < H here
        pix[u] = y * W + x;
        rs[u] = restart;
        wl[u] = cl[pix[u]];
#pragma unroll
        for (int k = 0; k < K; k++) {
          const int xr = x - d0 - k;        // < W always; a negative one reads as census 0 and forms no address
          const uint32_t w = cr[y * W + max(xr, 0)];
          wr[u][k] = xr >= 0 ? w : 0u;
        }
        if (!first) old[u] = *reinterpret_cast<const Run*>(S + (size_t)pix[u] * D + lane * K);
        x += dx; y += dy;
        restart = false;
        if (dy != 0) {
          if (x >= W) { x = 0; restart = true; }
          else if (x < 0) { x = W - 1; restart = true; }
        }
      }
    }
#pragma unroll
    for (int u = 0; u < PATH_AHEAD; u++) {
      if (t0 + u < steps) {
        int L[K];
        if (rs[u]) {
#pragma unroll
          for (int k = 0; k < K; k++) L[k] = __popc(wl[u] ^ wr[u][k]);
        } else {
          const int below = __builtin_amdgcn_update_dpp(FAR, Lp[K - 1], DPP_WAVE_SHR1, 0xf, 0xf, false);   // L(d0 - 1); none for d = 0
          const int above = __builtin_amdgcn_update_dpp(FAR, Lp[0], DPP_WAVE_SHL1, 0xf, 0xf, false);       // L(d0 + K); none for d = D - 1
          const int jump = m + P2;
#pragma unroll
          for (int k = 0; k < K; k++) {
            const int lo = k > 0 ? Lp[k - 1] : below, hi = k < K - 1 ? Lp[k + 1] : above;
            L[k] = __popc(wl[u] ^ wr[u][k]) + min(min(Lp[k], jump), min(lo, hi) + P1) - m;
          }
        }
        int s[K];
        if (first) {
#pragma unroll
          for (int k = 0; k < K; k++) s[k] = L[k];
        } else {
          unpack_run<K>(old[u], s);
#pragma unroll
          for (int k = 0; k < K; k++) s[k] += L[k];
        }
        *reinterpret_cast<Run*>(S + (size_t)pix[u] * D + lane * K) = pack_run<K>(s);
        int mine = L[0];
#pragma unroll
        for (int k = 0; k < K; k++) { Lp[k] = L[k]; mine = min(mine, L[k]); }
        m = wave_min(mine);
      }
    }
  }
}

// ---------------------------------------------------------------- stage 5: winner
// wave = pixel, WIN_PIXELS consecutive pixels per wave.  The argmin is the wave minimum of (S << 8 | d): the lowest d wins a tie.
constexpr int WIN_PIXELS = 8;
template <int K>
__global__ void __launch_bounds__(256) winner_kernel(int n, int u, const uint16_t* __restrict__ S, uint16_t* __restrict__ raw) {
  using Run = typename SRun<K>::type;
  constexpr int D = 64 * K;
  const int lane = threadIdx.x & 63;
  const int wave = blockIdx.x * 4 + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  for (int j = 0; j < WIN_PIXELS; j++) {
    const int p = wave * WIN_PIXELS + j;
    if (p >= n) return;                                    // uniform over the wave
    const uint16_t* __restrict__ Sp = S + (size_t)p * D;
    int s[K];
    unpack_run<K>(*reinterpret_cast<const Run*>(Sp + lane * K), s);
    int key = (s[0] << 8) | (lane * K);
#pragma unroll
    for (int k = 1; k < K; k++) key = min(key, (s[k] << 8) | (lane * K + k));
    key = wave_min(key);
    const int best = key & 0xFF, sbest = key >> 8;
    bool rival = false;
    if (u > 0) {
#pragma unroll
      for (int k = 0; k < K; k++) {
        const int d = lane * K + k;
        rival |= (d < best - 1 || d > best + 1) && s[k] * (100 - u) < sbest * 100;
      }
    }
    const bool invalid = __any(rival);
    int frac = 0;
    if (best > 0 && best < D - 1) {                         // uniform; both neighbours exist
      const int sm = Sp[best - 1], sp = Sp[best + 1];
      const int num = sm - sp, den = sm - 2 * sbest + sp;
      if (den > 0) {
        const int a = 16 * num + den, b = 2 * den;
        frac = a / b - ((a % b != 0 && a < 0) ? 1 : 0);      // floor, not truncation
      }
    }
    if (lane == 0) raw[p] = invalid ? (uint16_t)RAW_INVALID : (uint16_t)(16 * best + frac);
  }
}

// ---------------------------------------------------------------- stage 7a: the right view's disparity
// wave = pixel (xr, y) of the right view; lane l looks at d = l K + k, whose left pixel is x = xr + d + dmin.  The read is a gather
// with a stride of D + 1 entries; the four waves of a workgroup take adjacent xr, and a 128-byte line of S at (x, y) serves the 64
// right pixels xr = x - d - dmin of its d, all in this row and within D columns, so the lines are re-used out of L2.
template <int K>
__global__ void __launch_bounds__(256) right_view_kernel(int W, int H, int dmin, const uint16_t* __restrict__ S, int16_t* __restrict__ dr) {
  constexpr int D = 64 * K;
  const int lane = threadIdx.x & 63;
  const int wave = blockIdx.x * 4 + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  for (int j = 0; j < WIN_PIXELS; j++) {
    const int p = wave * WIN_PIXELS + j;
    if (p >= W * H) return;
    const int y = p / W, xr = p - y * W;
    int key = (FAR << 8);
#pragma unroll
    for (int k = 0; k < K; k++) {
      const int d = lane * K + k, x = xr + d + dmin;
      const int xs = min(x, W - 1);                          // x >= W takes no part and forms no address
      const int s = S[((size_t)y * W + xs) * D + d];
      key = min(key, x < W ? ((s << 8) | d) : (FAR << 8));
    }
    key = wave_min(key);
    if (lane == 0) dr[p] = (key >> 8) == FAR ? (int16_t)-1 : (int16_t)(key & 0xFF);
  }
}

// ---------------------------------------------------------------- stage 6: median
__device__ __forceinline__ void sort2(uint32_t& a, uint32_t& b) { const uint32_t lo = min(a, b), hi = max(a, b); a = lo; b = hi; }
__global__ void __launch_bounds__(256) median_kernel(int W, int H, const uint16_t* __restrict__ in, uint16_t* __restrict__ out) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= W * H) return;
  const int y = i / W, x = i - y * W;
  if (x == 0 || y == 0 || x == W - 1 || y == H - 1) { out[i] = in[i]; return; }
  uint32_t v[9];
#pragma unroll
  for (int dy = -1; dy <= 1; dy++)
#pragma unroll
    for (int dx = -1; dx <= 1; dx++) v[(dy + 1) * 3 + dx + 1] = in[(y + dy) * W + x + dx];
  // the classic 19-exchange median-of-9 network; v[4] ends as the 5th smallest
  sort2(v[1], v[2]); sort2(v[4], v[5]); sort2(v[7], v[8]); sort2(v[0], v[1]); sort2(v[3], v[4]); sort2(v[6], v[7]);
  sort2(v[1], v[2]); sort2(v[4], v[5]); sort2(v[7], v[8]); sort2(v[0], v[3]); sort2(v[5], v[8]); sort2(v[4], v[7]);
  sort2(v[3], v[6]); sort2(v[1], v[4]); sort2(v[2], v[5]); sort2(v[4], v[7]); sort2(v[4], v[2]); sort2(v[6], v[4]);
  sort2(v[4], v[2]);
  out[i] = (uint16_t)v[4];
}

// ---------------------------------------------------------------- stages 7b + 8: left-right check and the outputs
__global__ void __launch_bounds__(256) check_output_kernel(int W, int H, int dmin, int lr_max_diff, const uint16_t* __restrict__ raw,
                                                           const int16_t* __restrict__ dr, int16_t* __restrict__ disp16,
                                                           float* __restrict__ depth, float fb16) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= W * H) return;
  const int y = i / W, x = i - y * W;
  const int v = raw[i];
  bool valid = v != (int)RAW_INVALID;
  if (valid) {
    const int dl = (v + 8) >> 4, xr = x - dl - dmin;
    if (xr < 0) valid = false;                              // no right pixel: dr is not read
    else if (lr_max_diff >= 0) valid = abs(dl - (int)dr[y * W + xr]) <= lr_max_diff;
  }
  const int out = valid ? v + 16 * dmin : 16 * (dmin - 1);
  disp16[i] = (int16_t)out;
  if (depth) depth[i] = (valid && out > 0) ? fb16 / (float)out : 0.0f;
}

struct SgmLayout { size_t cl, cr, S, raw5, raw6, dr, total; };
SgmLayout sgm_layout(int W, int H, int D) {
  using segs::align_up;
  const size_t n = (size_t)W * H;
  SgmLayout l{};
  size_t o = 0;
  l.cl = o;   o = align_up(o + n * 4);
  l.cr = o;   o = align_up(o + n * 4);
  l.S = o;    o = align_up(o + n * D * 2);
  l.raw5 = o; o = align_up(o + n * 2);
  l.raw6 = o; o = align_up(o + n * 2);
  l.dr = o;   o = align_up(o + n * 2);
  l.total = o + segs::ALIGN;
  return l;
}
bool size_ok(int W, int H, int D, int paths) {
  return W >= 1 && H >= 1 && W <= 4096 && H <= 4096 && (D == 64 || D == 128 || D == 256) && (paths == 4 || paths == 8);
}
int bad(const char* what) { return segs::set_error(SEGS_ERR_INVALID_ARGUMENT, what); }
#define LAUNCH_OK() do { hipError_t _e = hipGetLastError(); if (_e != hipSuccess) return segs::set_error((int)_e, hipGetErrorString(_e)); } while (0)

template <int K>
int run_volume(const SegsStereoParams& p, int W, int H, const uint32_t* cl, const uint32_t* cr, uint16_t* S, uint16_t* raw5, int16_t* dr,
               hipStream_t st) {
  static const int dirs[8][2] = {{1, 0}, {-1, 0}, {0, 1}, {0, -1}, {1, 1}, {-1, -1}, {1, -1}, {-1, 1}};
  for (int r = 0; r < p.paths; r++) {
    const int dx = dirs[r][0], dy = dirs[r][1];
    const int nlines = dy == 0 ? H : W;
    sgm_path_kernel<K><<<(nlines + PATH_WAVES - 1) / PATH_WAVES, 64 * PATH_WAVES, 0, st>>>(W, H, p.min_disparity, p.P1, p.P2, dx, dy,
                                                                                         r == 0, cl, cr, S); LAUNCH_OK();
  }
  const int n = W * H, per_block = 4 * WIN_PIXELS;
  winner_kernel<K><<<(n + per_block - 1) / per_block, 256, 0, st>>>(n, p.uniqueness_ratio, S, raw5); LAUNCH_OK();
  right_view_kernel<K><<<(n + per_block - 1) / per_block, 256, 0, st>>>(W, H, p.min_disparity, S, dr); LAUNCH_OK();
  return SEGS_OK;
}

}  // namespace

extern "C" {

size_t segs_stereo_sgm_temp_bytes(int W, int H, int D, int paths) {
  return size_ok(W, H, D, paths) ? sgm_layout(W, H, D).total : 0;
}

int segs_rgb_to_gray_u8(int W, int H, const float* rgb, uint8_t* out, void* stream) {
  if (W < 1 || H < 1 || W > 4096 || H > 4096 || !rgb || !out) return bad("invalid argument (null pointer or bad size)");
  const int n = W * H;
  rgb_to_gray_kernel<<<(n + 255) / 256, 256, 0, (hipStream_t)stream>>>(n, rgb, out); LAUNCH_OK();
  return SEGS_OK;
}

int segs_debug_stereo_sgm_stages(const SegsStereoParams* params, int W, int H, const uint8_t* left, const uint8_t* right,
                                 int16_t* disp16, float* depth, float fb16, char* temp, uint32_t* census_left,
                                 uint32_t* census_right, uint16_t* S_out, uint16_t* raw_winner, uint16_t* raw_median,
                                 int16_t* disp_right, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  if (!params || !left || !right || !disp16 || !temp) return bad("invalid argument (null pointer)");
  const SegsStereoParams p = *params;
  if (!size_ok(W, H, p.num_disparities, p.paths)) return bad("stereo: 1 <= W, H <= 4096, D in {64, 128, 256}, paths 4 or 8");
  if (p.min_disparity < 0 || p.num_disparities + p.min_disparity > 2047) return bad("stereo: min_disparity >= 0 and D + min_disparity <= 2047");
  if (p.P1 < 0 || p.P1 > p.P2 || p.P2 > 224) return bad("stereo: 0 <= P1 <= P2 <= 224");
  if (p.uniqueness_ratio < 0 || p.uniqueness_ratio >= 100) return bad("stereo: uniqueness_ratio in [0, 100)");
  if (p.lr_max_diff < -1 || (p.median != 0 && p.median != 1)) return bad("stereo: lr_max_diff >= -1, median 0 or 1");
  const int D = p.num_disparities;
  const SgmLayout L = sgm_layout(W, H, D);
  char* base = segs::align_ptr(temp);
  uint32_t* cl = (uint32_t*)(base + L.cl);
  uint32_t* cr = (uint32_t*)(base + L.cr);
  uint16_t* S = (uint16_t*)(base + L.S);
  uint16_t* raw5 = (uint16_t*)(base + L.raw5);
  uint16_t* raw6 = (uint16_t*)(base + L.raw6);
  int16_t* dr = (int16_t*)(base + L.dr);
  const int n = W * H, nb = (n + 255) / 256;
  census_kernel<<<dim3(nb, 2), 256, 0, st>>>(W, H, left, right, cl, cr); LAUNCH_OK();
  const int rc = D == 64 ? run_volume<1>(p, W, H, cl, cr, S, raw5, dr, st)
               : D == 128 ? run_volume<2>(p, W, H, cl, cr, S, raw5, dr, st) : run_volume<4>(p, W, H, cl, cr, S, raw5, dr, st);
  if (rc) return rc;
  if (p.median) { median_kernel<<<nb, 256, 0, st>>>(W, H, raw5, raw6); LAUNCH_OK(); }
  const uint16_t* raw = p.median ? raw6 : raw5;
  check_output_kernel<<<nb, 256, 0, st>>>(W, H, p.min_disparity, p.lr_max_diff, raw, dr, disp16, depth, fb16); LAUNCH_OK();
  // the debug copies: device to device on the same stream, behind the run
  struct Copy { void* dst; const void* src; size_t bytes; };
  const Copy copies[] = {{census_left, cl, (size_t)n * 4}, {census_right, cr, (size_t)n * 4}, {S_out, S, (size_t)n * D * 2},
                         {raw_winner, raw5, (size_t)n * 2}, {raw_median, raw, (size_t)n * 2}, {disp_right, dr, (size_t)n * 2}};
  for (const Copy& c : copies)
    if (c.dst) {
      const hipError_t e = hipMemcpyAsync(c.dst, c.src, c.bytes, hipMemcpyDeviceToDevice, st);
      if (e != hipSuccess) return segs::set_error((int)e, hipGetErrorString(e));
    }
  return SEGS_OK;
}

int segs_stereo_sgm(const SegsStereoParams* params, int W, int H, const uint8_t* left, const uint8_t* right, int16_t* disp16,
                    float* depth, float fb16, char* temp, void* stream) {
  return segs_debug_stereo_sgm_stages(params, W, H, left, right, disp16, depth, fb16, temp, nullptr, nullptr, nullptr, nullptr,
                                      nullptr, nullptr, stream);
}

}  // extern "C"
