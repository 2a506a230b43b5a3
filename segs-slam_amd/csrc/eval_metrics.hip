// eval_metrics.hip -- keyframe evaluation on the device (include/segs_eval.h).
// Reference: GaussianMapper::renderAndRecordKeyframe (src/gaussian_mapper.cpp:1811-1840): the (channel, row) mask of the target,
// loss_utils::ssim / psnr / psnr_gaussian_splatting of the masked pair -- five grouped conv2d, a dozen image-sized pointwise ops
// and three .item() readbacks per keyframe -- and convertTo(CV_8UC3, 255.0f) of the three recorded images.  Here:
//   row_flag_kernel     : gt -> 3 H bytes, one wave per (channel, row)                       (row_mask only)
//   eval_metrics_kernel : the tiling of loss.hip's ssim_fwd_kernel; the flag is applied while the tile is staged, |d| and d^2
//                         come from the staged centre, nothing image-sized is written: one slot of three sums per workgroup
//   eval_finish_kernel  : one workgroup folds the slots in a fixed order and writes the eight words of the table row
//   eval_images_kernel  : pointwise, a workgroup per image row, four pixels per thread, bytes leave as dwords   (on request)
// No atomics anywhere: every sum is a fixed tree, so every run gives the same bits.
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdint>
#include "../../include/segs_raster.h"
#include "kernels.h"
#include "ssim_tile.h"
#include "../../include/segs_eval.h"

namespace {
using namespace ssim_tile;

constexpr int FINISH_THREADS = 1024;   // 16 waves
constexpr int FINISH_ACC = 4;          // independent accumulators per thread and sum: the chain grows by slots / 4096

// m[c][y] = any(gt[c][y][:] != 0): one wave per row, four rows per workgroup.
__global__ void __launch_bounds__(256) row_flag_kernel(const float* __restrict__ gt, int rows /* 3 H */, int W, uint8_t* __restrict__ flag) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;             // (whole waves leave; no barrier below)
  const float* p = gt + (size_t)row * W;
  bool any = false;
  for (int x = threadIdx.x & 63; x < W; x += 64) any |= p[x] != 0.f;
  const unsigned long long hit = __ballot(any);
  if ((threadIdx.x & 63) == 0) flag[row] = hit != 0ull ? 1 : 0;
}

// load_tiles (ssim_tile.h) for the image / target pair with the row flag multiplied in: dst[0] = image * m, dst[1] = gt * m.
// flag = nullptr: m = 1.
template <int IH>
__device__ __forceinline__ void load_pair_masked(float (*dst)[IH][SP], const float* __restrict__ img, const float* __restrict__ gt,
                                                 const uint8_t* __restrict__ flag, int H, int W, int x0, int y0) {
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  constexpr int RI = (IH + 7) / 8;
  float v[2][RI][2];
#pragma unroll
  for (int i = 0; i < RI; i++) {
    const int r = ty + 8 * i;
    const int gy = y0 + r - HALO;
    const bool row_in = r < IH && gy >= 0 && gy < H;
    const float m = (flag != nullptr && row_in) ? (float)flag[gy] : 1.f;
#pragma unroll
    for (int j = 0; j < 2; j++) {
      const int c = tx + 32 * j;
      const int gx = x0 + c - HALO;
      const bool in = row_in && c < IW && gx >= 0 && gx < W;
      const size_t o = in ? (size_t)gy * W + gx : 0;
      const float a = img[o], b = gt[o];
      v[0][i][j] = in ? a * m : 0.f;
      v[1][i][j] = in ? b * m : 0.f;
    }
  }
#pragma unroll
  for (int i = 0; i < RI; i++) {
    const int r = ty + 8 * i;
#pragma unroll
    for (int j = 0; j < 2; j++) {
      const int c = tx + 32 * j;
      if (r < IH && c < IW) { dst[0][r][c] = v[0][i][j]; dst[1][r][c] = v[1][i][j]; }
    }
  }
}

template <int TY>
__global__ void __launch_bounds__(256) eval_metrics_kernel(const float* __restrict__ img, const float* __restrict__ gt, int H, int W,
                                                           Win win, const uint8_t* __restrict__ flag /* 3 H or null */,
                                                           float4* __restrict__ partial /* per workgroup: (sum S, sum|d|, sum d^2, 0) */) {
  constexpr int IH = TY + 2 * HALO;
  constexpr int RPT = TY / 8;
  __shared__ __attribute__((aligned(16))) float sin[2][IH][SP];
  float (*s1)[SP] = sin[0];
  float (*s2)[SP] = sin[1];
  __shared__ __attribute__((aligned(16))) float h[5][IH][TX];
  __shared__ float red[3][4];
  const int ch = blockIdx.z;
  const size_t plane = (size_t)ch * H * W;
  const int x0 = blockIdx.x * TX, y0 = blockIdx.y * TY;
  const int tid = threadIdx.x;
  load_pair_masked<IH>(sin, img + plane, gt + plane, flag ? flag + (size_t)ch * H : nullptr, H, W, x0, y0);
  __syncthreads();
  {  // horizontal pass
    const int p = tid & 15;
    for (int r = tid >> 4; r < IH; r += 16) {
      float u[12], v[12];
#pragma unroll
      for (int k = 0; k < 6; k++) {
        const float2 a = *reinterpret_cast<const float2*>(&s1[r][2 * p + 2 * k]);
        const float2 b = *reinterpret_cast<const float2*>(&s2[r][2 * p + 2 * k]);
        u[2 * k] = a.x; u[2 * k + 1] = a.y; v[2 * k] = b.x; v[2 * k + 1] = b.y;
      }
      float uu[12], vv[12], uv[12];
#pragma unroll
      for (int k = 0; k < 12; k++) { uu[k] = u[k] * u[k]; vv[k] = v[k] * v[k]; uv[k] = u[k] * v[k]; }
      float o[5][2];
#pragma unroll
      for (int e = 0; e < 2; e++) {
        float a = 0.f, b = 0.f, aa = 0.f, bb = 0.f, ab = 0.f;
#pragma unroll
        for (int k = 0; k < 11; k++) {
          const float g = win.g[k];
          a += g * u[e + k]; b += g * v[e + k]; aa += g * uu[e + k]; bb += g * vv[e + k]; ab += g * uv[e + k];
        }
        o[0][e] = a; o[1][e] = b; o[2][e] = aa; o[3][e] = bb; o[4][e] = ab;
      }
#pragma unroll
      for (int m = 0; m < 5; m++) *reinterpret_cast<float2*>(&h[m][r][2 * p]) = make_float2(o[m][0], o[m][1]);
    }
  }
  __syncthreads();
  const int lx = tid & 31, ly = (tid >> 5) * RPT;
  float acc[5][RPT];
#pragma unroll
  for (int m = 0; m < 5; m++) {
    float col[RPT + 10];
#pragma unroll
    for (int j = 0; j < RPT + 10; j++) col[j] = h[m][ly + j][lx];
#pragma unroll
    for (int e = 0; e < RPT; e++) {
      float a = 0.f;
#pragma unroll
      for (int k = 0; k < 11; k++) a += win.g[k] * col[e + k];
      acc[m][e] = a;
    }
  }
  const int gx = x0 + lx;
  float sum[3] = {0.f, 0.f, 0.f};   // S, |d|, d^2
#pragma unroll
  for (int e = 0; e < RPT; e++) {
    const int gy = y0 + ly + e;
    if (gx < W && gy < H) {
      const float mu1 = acc[0][e], mu2 = acc[1][e], e11 = acc[2][e], e22 = acc[3][e], e12 = acc[4][e];
      const float C1 = 0.01f * 0.01f, C2 = 0.03f * 0.03f;
      const float mu1_sq = mu1 * mu1, mu2_sq = mu2 * mu2, mu12 = mu1 * mu2;
      const float s11 = e11 - mu1_sq, s22 = e22 - mu2_sq, s12 = e12 - mu12;
      const float A1 = 2.f * mu12 + C1, A2 = 2.f * s12 + C2, B1 = mu1_sq + mu2_sq + C1, B2 = s11 + s22 + C2;
      const float inv = 1.f / (B1 * B2);
      sum[0] += A1 * A2 * inv;
      const float d = s1[ly + e + HALO][lx + HALO] - s2[ly + e + HALO][lx + HALO];
      sum[1] += fabsf(d);
      sum[2] += d * d;
    }
  }
#pragma unroll
  for (int q = 0; q < 3; q++) {
    float v = sum[q];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    if ((tid & 63) == 0) red[q][tid >> 6] = v;
  }
  __syncthreads();
  if (tid == 0) {
    float t[3];
#pragma unroll
    for (int q = 0; q < 3; q++) t[q] = (red[q][0] + red[q][1]) + (red[q][2] + red[q][3]);
    // slots of a channel are contiguous: the finish kernel walks [ch * n, (ch + 1) * n)
    partial[(blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x] = make_float4(t[0], t[1], t[2], 0.f);
  }
}

// One workgroup: the nine sums (three per channel) over n slots per channel, in a fixed order, then the eight words.
__global__ void __launch_bounds__(FINISH_THREADS) eval_finish_kernel(const float4* __restrict__ partial, int n /* slots per channel */,
                                                                      float n_pix /* H W */, float n_all /* 3 H W */,
                                                                      float* __restrict__ row /* 8 words */) {
  __shared__ float red[9][FINISH_THREADS / 64];
  __shared__ float tot[9];
  const int tid = threadIdx.x;
  float acc[9][FINISH_ACC];
#pragma unroll
  for (int s = 0; s < 9; s++)
#pragma unroll
    for (int j = 0; j < FINISH_ACC; j++) acc[s][j] = 0.f;
  for (int i = tid; i < n; i += FINISH_THREADS * FINISH_ACC) {
#pragma unroll
    for (int j = 0; j < FINISH_ACC; j++) {
      const int k = i + FINISH_THREADS * j;
      if (k < n) {
#pragma unroll
        for (int c = 0; c < 3; c++) {
          const float4 v = partial[(size_t)c * n + k];
          acc[3 * c + 0][j] += v.x; acc[3 * c + 1][j] += v.y; acc[3 * c + 2][j] += v.z;
        }
      }
    }
  }
#pragma unroll
  for (int s = 0; s < 9; s++) {
    float v = (acc[s][0] + acc[s][1]) + (acc[s][2] + acc[s][3]);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    if ((tid & 63) == 0) red[s][tid >> 6] = v;
  }
  __syncthreads();
  if (tid < 9) {
    const float* r = red[tid];
    tot[tid] = (((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]))) +
               (((r[8] + r[9]) + (r[10] + r[11])) + ((r[12] + r[13]) + (r[14] + r[15])));
  }
  __syncthreads();
  if (tid == 0) {
    // tot[3 c + q]: q = 0 SSIM, 1 |d|, 2 d^2.  Divided, not multiplied by a rounded reciprocal (N ones must average to 1).
    const float S = (tot[0] + tot[3]) + tot[6], A = (tot[1] + tot[4]) + tot[7], Q = (tot[2] + tot[5]) + tot[8];
    const float mse = Q / n_all;
    float p[3], mc[3];
#pragma unroll
    for (int c = 0; c < 3; c++) {
      mc[c] = tot[3 * c + 2] / n_pix;
      p[c] = log10f(1.f / sqrtf(mc[c]));
    }
    row[0] = S / n_all;
    row[1] = 10.f * log10f(1.f / mse);
    row[2] = 20.f * (((p[0] + p[1]) + p[2]) / 3.f);   // 20 * log10(..).mean(), loss_utils.h:48
    row[3] = mse;
    row[4] = mc[0]; row[5] = mc[1]; row[6] = mc[2];
    row[7] = A / n_all;
  }
}

__device__ __forceinline__ uint32_t to_byte(float v) {   // segs_eval.h, THE BYTES
  const float r = rintf(v * 255.0f);
  return (uint32_t)fminf(fmaxf(r, 0.f), 255.f);          // fmaxf(NaN, 0) = 0
}

// A workgroup per image row y, all three channels; thread t takes pixels 4 t .. 4 t + 3 (+ 1024 per round).  FLAGS: 0 no mask,
// 1 flags from `flag`, 2 computed here.  DWORDS: W % 4 == 0 and dword-aligned outputs: 12 bytes leave as three dword stores.
template <bool DWORDS>
__global__ void __launch_bounds__(256) eval_images_kernel(const float* __restrict__ img, const float* __restrict__ gt, int H, int W,
                                                          int flags_mode, const uint8_t* __restrict__ flag, uint8_t* __restrict__ o_img,
                                                          uint8_t* __restrict__ o_gt, uint8_t* __restrict__ o_loss) {
  const int y = blockIdx.x, tid = threadIdx.x;
  const size_t plane = (size_t)H * W;
  float m[3] = {1.f, 1.f, 1.f};
  if (flags_mode == 1) {
#pragma unroll
    for (int c = 0; c < 3; c++) m[c] = (float)flag[(size_t)c * H + y];
  } else if (flags_mode == 2) {
#pragma unroll
    for (int c = 0; c < 3; c++) {
      const float* p = gt + c * plane + (size_t)y * W;
      int any = 0;
      for (int x = tid; x < W; x += 256) any |= p[x] != 0.f;
      m[c] = __syncthreads_or(any) ? 1.f : 0.f;
    }
  }
  for (int x4 = 4 * tid; x4 < W; x4 += 1024) {
    uint32_t b[3][4][3];   // [image, gt, loss][pixel][channel]
#pragma unroll
    for (int k = 0; k < 4; k++) {
      const bool in = x4 + k < W;
#pragma unroll
      for (int c = 0; c < 3; c++) {
        const size_t o = c * plane + (size_t)y * W + (in ? x4 + k : x4);
        const float X = img[o] * m[c], T = gt[o] * m[c];
        b[0][k][c] = to_byte(X); b[1][k][c] = to_byte(T); b[2][k][c] = to_byte(fabsf(X - T));
      }
    }
    uint8_t* const outs[3] = {o_img, o_gt, o_loss};
#pragma unroll
    for (int i = 0; i < 3; i++) {
      if (outs[i] == nullptr) continue;
      uint8_t* dst = outs[i] + ((size_t)y * W + x4) * 3;
      if (DWORDS) {   // all four pixels are inside the row
        uint32_t w[3];
#pragma unroll
        for (int j = 0; j < 3; j++) {
          w[j] = 0;
#pragma unroll
          for (int q = 0; q < 4; q++) { const int e = 4 * j + q; w[j] |= b[i][e / 3][e % 3] << (8 * q); }
        }
        uint32_t* d32 = reinterpret_cast<uint32_t*>(dst);
        d32[0] = w[0]; d32[1] = w[1]; d32[2] = w[2];
      } else {
#pragma unroll
        for (int k = 0; k < 4; k++) {
          if (x4 + k < W) {
#pragma unroll
            for (int c = 0; c < 3; c++) dst[3 * k + c] = (uint8_t)b[i][k][c];
          }
        }
      }
    }
  }
}

size_t flag_bytes(int H) { return ((size_t)3 * H + 255) & ~(size_t)255; }
bool size_ok(int H, int W) { return H > 0 && W > 0 && H <= SEGS_EVAL_MAX_SIZE && W <= SEGS_EVAL_MAX_SIZE; }

}  // namespace

extern "C" {

size_t segs_eval_temp_bytes(int H, int W) {
  if (!size_ok(H, W)) return 0;
  const size_t nblk = (size_t)3 * ((W + TX - 1) / TX) * ((H + 15) / 16);   // sized for the smaller tile
  return flag_bytes(H) + ((nblk * sizeof(float4) + 255) & ~(size_t)255);
}

int segs_eval_frame(const float* image, const float* gt, int H, int W, int row_mask, float* table, int n_slots, int slot,
                    char* temp, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  if (!image || !gt || !table || !temp || !size_ok(H, W) || n_slots <= 0 || slot < 0 || slot >= n_slots)
    return segs::set_error(SEGS_ERR_INVALID_ARGUMENT, "invalid argument (null pointer, bad size or slot outside the table)");
  const Win win = make_window();
  uint8_t* flag = reinterpret_cast<uint8_t*>(temp);
  float4* partial = reinterpret_cast<float4*>(temp + flag_bytes(H));
  if (row_mask) row_flag_kernel<<<dim3((3 * H + 3) / 4), dim3(256), 0, st>>>(gt, 3 * H, W, flag);
  const int ty = tile_rows(H, W);
  const dim3 grid((W + TX - 1) / TX, (H + ty - 1) / ty, 3), block(256);
  if (ty == 32) eval_metrics_kernel<32><<<grid, block, 0, st>>>(image, gt, H, W, win, row_mask ? flag : nullptr, partial);
  else eval_metrics_kernel<16><<<grid, block, 0, st>>>(image, gt, H, W, win, row_mask ? flag : nullptr, partial);
  const float n_pix = (float)((size_t)H * W), n_all = (float)((size_t)3 * H * W);
  eval_finish_kernel<<<dim3(1), dim3(FINISH_THREADS), 0, st>>>(partial, (int)(grid.x * grid.y), n_pix, n_all,
                                                               table + (size_t)slot * SEGS_EVAL_ROW_WORDS);
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? SEGS_OK : segs::set_hip_error(e, __func__);
}

int segs_eval_images_u8(const float* image, const float* gt, int H, int W, int row_mask, uint8_t* image_u8, uint8_t* gt_u8,
                        uint8_t* loss_u8, const char* temp_or_null, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  if (!image || !gt || !size_ok(H, W)) return segs::set_error(SEGS_ERR_INVALID_ARGUMENT, "invalid argument (null pointer or bad size)");
  if (!image_u8 && !gt_u8 && !loss_u8) return SEGS_OK;
  const int mode = !row_mask ? 0 : (temp_or_null ? 1 : 2);
  const uint8_t* flag = reinterpret_cast<const uint8_t*>(temp_or_null);
  const bool dwords = W % 4 == 0 && (((uintptr_t)image_u8 | (uintptr_t)gt_u8 | (uintptr_t)loss_u8) & 3) == 0;
  if (dwords) eval_images_kernel<true><<<dim3(H), dim3(256), 0, st>>>(image, gt, H, W, mode, flag, image_u8, gt_u8, loss_u8);
  else eval_images_kernel<false><<<dim3(H), dim3(256), 0, st>>>(image, gt, H, W, mode, flag, image_u8, gt_u8, loss_u8);
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? SEGS_OK : segs::set_hip_error(e, __func__);
}

}  // extern "C"
