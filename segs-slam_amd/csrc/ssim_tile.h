// ssim_tile.h -- what the 11x11 Gaussian-window kernels share: the tile geometry, the window, the block sum and the staging of
// input tiles into LDS.  Used by loss.hip (fused L1 + SSIM loss, forward and backward) and eval_metrics.hip (keyframe metrics).
#pragma once
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstddef>

namespace ssim_tile {
// Tiling (both kernels): a 256-thread workgroup produces a 32 x 32 output tile from a 42 x 42 input tile (halo 5).
//  * horizontal pass: a thread owns one input row and a PAIR of adjacent output columns, reads its 12 inputs as six
//    ds_read_b64 (16 lanes cover one contiguous 128-B row segment -> no bank conflicts) and forms the products once per
//    input, not once per tap;
//  * vertical pass: a thread owns one column and FOUR adjacent output rows, so the 14 rows it needs are read once for
//    4 x 11 taps (half-waves read contiguous 128-B rows -> no bank conflicts).
// The first version (16 x 16 tiles, one output per thread, odd LDS pitches) spent 43 % of its LDS cycles in bank
// conflicts and 2.3x the VALU instructions on index arithmetic and per-tap products: 45 + 35 us at 1200x680.
// Small images (640x480: 900 tiles of 32 x 32 on 256 CUs) use 32 x 16 tiles instead (template parameter TY).
constexpr int TX = 32;              // output tile width; height TY = 32 or 16
constexpr int HALO = 5;
constexpr int IW = TX + 2 * HALO;   // 42 input columns
constexpr int SP = 44;              // input pitch in floats: even (b64 reads), 44 mod 32 = 12 keeps row pairs apart
struct Win { float g[11]; };

__device__ __forceinline__ float block_sum(float v, float* red) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
  const int tid = threadIdx.x;
  if ((tid & 63) == 0) red[tid >> 6] = v;
  __syncthreads();
  return red[0] + red[1] + red[2] + red[3];
}

// Stage the IH x IW windows of N planes at (y0 - HALO, x0 - HALO) into dst[n][IH][SP], zero outside the image.  All
// N * 12 loads of a thread are issued before the first LDS store: a rolled loop here costs one global round trip per
// iteration (18 in the backward), which at 3 workgroups per CU was most of the kernel time.
template <int N, int IH>
__device__ __forceinline__ void load_tiles(float (*dst)[IH][SP], const float* const (&src)[N], int H, int W, int x0, int y0) {
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  constexpr int RI = (IH + 7) / 8;   // 6 row rounds
  float v[N][RI][2];
#pragma unroll
  for (int i = 0; i < RI; i++) {
    const int r = ty + 8 * i;
    const int gy = y0 + r - HALO;
    const bool row_in = r < IH && gy >= 0 && gy < H;
#pragma unroll
    for (int j = 0; j < 2; j++) {
      const int c = tx + 32 * j;
      const int gx = x0 + c - HALO;
      const bool in = row_in && c < IW && gx >= 0 && gx < W;
      const size_t o = in ? (size_t)gy * W + gx : 0;
#pragma unroll
      for (int n = 0; n < N; n++) { const float t = src[n][o]; v[n][i][j] = in ? t : 0.f; }
    }
  }
#pragma unroll
  for (int i = 0; i < RI; i++) {
    const int r = ty + 8 * i;
#pragma unroll
    for (int j = 0; j < 2; j++) {
      const int c = tx + 32 * j;
      if (r < IH && c < IW) {
#pragma unroll
        for (int n = 0; n < N; n++) dst[n][r][c] = v[n][i][j];
      }
    }
  }
}

// The window of loss_utils.h:51-64: integer offsets, float arithmetic.
inline Win make_window() {
  Win win;
  float sum = 0.f;
  for (int x = 0; x < 11; ++x) {
    const int t = x - 11 / 2;
    win.g[x] = std::exp(-(float)(t * t) / (2.0f * 1.5f * 1.5f));
    sum += win.g[x];
  }
  for (int x = 0; x < 11; ++x) win.g[x] /= sum;
  return win;
}

// 32-row tiles once they fill the chip about twice over
inline int tile_rows(int H, int W) {
  return (size_t)3 * ((W + TX - 1) / TX) * ((H + 31) / 32) >= 1536 ? 32 : 16;
}
}  // namespace ssim_tile
