// preprocess.hip -- per-Gaussian kernels of the rasterizer (gfx950 / MI355X).
//
//   preprocess_fwd_kernel   K1  reference: preprocessCUDA          cuda_rasterizer/forward.cu:155-256
//   visible_filter_kernel   K2  reference: filter_preprocessCUDA   cuda_rasterizer/forward.cu:259-334
//   mark_visible_kernel     K4  reference: checkFrustum            cuda_rasterizer/rasterizer_impl.cu:54-66
//   preprocess_bwd_kernel   K12+K13 fused; reference: computeCov2DCUDA backward.cu:144-274,
//                           preprocessCUDA backward.cu:346-396, computeCov3D backward.cu:278-341
//                           <true>: + the depth map's dL/dz (row dword [9]); no reference counterpart
//                           <., true>: + the 24 per-workgroup sums of the camera gradient (dL/dviewmatrix, dL/dprojmatrix)
//   preprocess_bwd_packed_kernel   the same stage for the resident backward: the reached rows of a workgroup packed into one wave
//                           (both kernels are callers of one projection_backward_row, one preprocess_bwd_rows, one camera_fold)
//   camera_grad_reduce_kernel   sums those partials in a fixed order into the two 4x4 gradients; no reference counterpart
//
// All are HBM-bound streaming kernels (one Gaussian per lane, 256-thread workgroups):
//  * the (P,3) AoS inputs are fetched as three fully coalesced dword sweeps per workgroup and
//    transposed through LDS (stride-3 LDS reads are conflict free), rotations as 16 B/lane;
//  * everything the tile kernels need is emitted as ONE 64-byte record per Gaussian (gs_layout.h);
//  * the per-workgroup sum of tiles_touched is produced here so the prefix sum needs no extra pass
//    over the per-Gaussian data;
//  * the backward fuses the reference's two kernels and its 108 B/Gaussian of zero-fills (K14): every
//    output row is written exactly once (zeros for culled Gaussians), cov3D is recomputed instead of
//    being stored and re-read.
//
// Arithmetic: this translation unit is built with -ffp-contract=off and evaluates every expression
// in the reference's order with one binary32 rounding per operation, so that radii, rects, depths
// (hence tile/sort keys) are bit-identical to the CPU oracle.  glm semantics: mat3 is column-major,
// m[c][r] = column c, row r.
#include <hip/hip_runtime.h>
#include <cstdint>
#include "gs_layout.h"
#include "kernels.h"
#include "project_gaussian.h"
#include "sh_color.h"

#pragma clang fp contract(off)

namespace segs {

// Workgroup-coalesced fetch of row `tid` of a (P,3) float array: three dword sweeps + LDS transpose.
__device__ __forceinline__ float3 load_row3(const float* __restrict__ a, int P, float* lds /*768 floats*/) {
  const int tid = threadIdx.x;
  const size_t base = (size_t)blockIdx.x * 768;
  const size_t lim = (size_t)P * 3;
#pragma unroll
  for (int k = 0; k < 3; k++) {
    const size_t i = base + k * 256 + tid;
    lds[k * 256 + tid] = i < lim ? a[i] : 0.f;
  }
  __syncthreads();
  float3 v = make_float3(lds[3 * tid], lds[3 * tid + 1], lds[3 * tid + 2]);
  __syncthreads();
  return v;
}

// Up to three (P,3) arrays at once: all nine dword sweeps are in flight before the first wait and ONE barrier pair covers
// them.  Three load_row3 calls in a row were three dependent memory round trips per wave, and the per-Gaussian kernels run
// only a few waves per SIMD, so that latency was not hidden: 131 -> 108 us (forward) and 153 -> 122 us (backward) at 3 M
// Gaussians.  (Hoisting the remaining per-lane loads -- opacity, radii, rotation -- the same way changed nothing.)
// lds: 768 floats per array; null arrays are skipped.
__device__ __forceinline__ void load_rows3(const float* __restrict__ a0, const float* __restrict__ a1, const float* __restrict__ a2,
                                           int P, float* lds /*3 x 768 floats*/, float3& v0, float3& v1, float3& v2) {
  const int tid = threadIdx.x;
  const size_t base = (size_t)blockIdx.x * 768;
  const size_t lim = (size_t)P * 3;
  const float* arr[3] = {a0, a1, a2};
  float t[3][3];
#pragma unroll
  for (int m = 0; m < 3; m++)
#pragma unroll
    for (int k = 0; k < 3; k++) {
      const size_t i = base + k * 256 + tid;
      t[m][k] = (arr[m] && i < lim) ? arr[m][i] : 0.f;
    }
#pragma unroll
  for (int m = 0; m < 3; m++)
#pragma unroll
    for (int k = 0; k < 3; k++) lds[m * 768 + k * 256 + tid] = t[m][k];
  __syncthreads();
  v0 = make_float3(lds[3 * tid], lds[3 * tid + 1], lds[3 * tid + 2]);
  v1 = make_float3(lds[768 + 3 * tid], lds[768 + 3 * tid + 1], lds[768 + 3 * tid + 2]);
  v2 = make_float3(lds[1536 + 3 * tid], lds[1536 + 3 * tid + 1], lds[1536 + 3 * tid + 2]);
  __syncthreads();
}

__global__ void __launch_bounds__(256) preprocess_fwd_kernel(
    int P, const float* __restrict__ means3D, const float* __restrict__ scales, float mod,
    const float* __restrict__ rotations, const float* __restrict__ opacities, const float* __restrict__ colors,
    const float* __restrict__ cov3D_precomp, const float* __restrict__ viewmatrix, const float* __restrict__ projmatrix,
    int W, int H, float tan_fovx, float tan_fovy, float focal_x, float focal_y, uint32_t gx, uint32_t gy,
    int* __restrict__ radii, float* __restrict__ rec, BinInfo* __restrict__ bin, uint32_t* __restrict__ block_sums,
    uint32_t* __restrict__ depth_range /* per workgroup: [b] = max(depth_bits), [nblocks + b] = max(~depth_bits), visible only */,
    const float* __restrict__ shs, int D, int M, const float* __restrict__ cam_pos, uint32_t* __restrict__ clamped,
    uint32_t flags, uint32_t* __restrict__ depth_keys, uint32_t* __restrict__ depth_vals, uint2* __restrict__ ranges,
    int num_tiles, uint32_t* __restrict__ depth_overflow /* resident: set when a binned depth leaves the 27-bit key range */,
    uint32_t* __restrict__ touched_dense) {
  __shared__ float lds[3 * 768];
  __shared__ uint32_t wave_sums[4], wave_dmax[4], wave_dnmin[4];
  const int idx = blockIdx.x * 256 + threadIdx.x;
  float4 rot = make_float4(0, 0, 0, 0);
  if (scales && idx < P) rot = reinterpret_cast<const float4*>(rotations)[idx];   // in flight together with the sweeps below
  float3 p, sc, col;
  load_rows3(means3D, scales, colors, P, lds, p, sc, col);

  uint32_t touched = 0, dbits_mine = 0;
  float4 rq0 = make_float4(0, 0, 0, 0), rq1 = rq0, rq2 = rq0, rq3 = rq0;   // this Gaussian's record, stored below
  bool has_record = false;
  if (idx < P) {
    Projected g = project_gaussian(p, sc, mod, rot, cov3D_precomp ? cov3D_precomp + (size_t)6 * idx : nullptr,
                                   viewmatrix, projmatrix, W, H, tan_fovx, tan_fovy, focal_x, focal_y, gx, gy);
    // SEGS_RASTER_SKIP_NONPOSITIVE_OPACITY: such a Gaussian can never pass alpha >= 1/255; dropping it here equals
    // the reference's compaction of masked-out neural Gaussians before the rasterizer (gaussian_renderer.cpp:320)
    if ((flags & 1u) && !(opacities[idx] > 0.f)) g.radius = 0;
    BinInfo b{0u, 0u, 0u, 0u};
    if (g.radius > 0) {
      const float op = opacities[idx];
      if (!colors) {  // forward.cu:241-247
        uint32_t cb;
        col = sh::to_rgb(idx, D, M, p, cam_pos, shs, &cb);
        clamped[idx] = cb;
      }
      const BinnedRecord br = make_record(g, op, col, flags);
      touched = br.touched;
      b.depth_bits = br.depth_bits;
      dbits_mine = b.depth_bits;
      b.rect_min = br.rect_min;
      b.rect_max = br.rect_max;
      b.tiles_touched = touched;
      rq0 = br.q0; rq1 = br.q1; rq2 = br.q2; rq3 = br.q3;
      has_record = true;
    }
    radii[idx] = g.radius;
    // BinInfo feeds make_depth_keys_kernel and the parity-test unpackers of the reference-shaped path; the resident path
    // (depth keys written right here) reads it nowhere: 16 B x P saved per step
    if (!depth_keys) reinterpret_cast<uint4*>(bin)[idx] = make_uint4(b.depth_bits, b.rect_min, b.rect_max, b.tiles_touched);
    touched_dense[idx] = b.tiles_touched;
    if (depth_keys) {   // resident mode: what make_depth_keys_kernel would write (32-bit depth keys, culled = 0xFFFFFFFF)
      // The resident depth sort looks at DEPTH_KEY_BITS bits above the near plane's bit pattern (three 9-bit passes).
      // Gaussians without instances carry the all-ones key: the FIRST pass gives them no histogram count and no rank, so the
      // later passes, the depth-ordered prefix and the emitter's searches only see the binned ones (30 % fewer at 3 M).  A
      // binned depth beyond the key range -- 0.2 * 2^16 = 13 107 -- flags the step; the host redoes it through the exact path.
      depth_keys[idx] = b.tiles_touched ? b.depth_bits : 0xFFFFFFFFu;
      (void)depth_vals;   // the sort's first pass takes the index itself as the value (no iota array)
      if (depth_overflow && b.tiles_touched && (b.depth_bits - DEPTH_KEY_MIN) >= ((1u << DEPTH_KEY_BITS) - 1u)) *depth_overflow = 1u;
    }
  }
  // The records leave through a per-wave LDS transpose: a lane storing its own 64 bytes as four float4 makes every store
  // instruction touch 64 different lines, a quarter of each; transposed, an instruction writes sixteen whole records (1 KB
  // contiguous), 32 records of the wave at a time in the (by now free) staging buffer of the input sweeps.
  {
    const int lane = threadIdx.x & 63;
    float* const wl = lds + (threadIdx.x >> 6) * 576;   // 32 records x 16 dwords of this wave (576 = 2304 / 4)
    const uint64_t recs = __ballot(has_record);
    const size_t wave_first = (size_t)blockIdx.x * 256 + (threadIdx.x & ~63);
#pragma unroll
    for (int half = 0; half < 2; half++) {
      if ((lane >> 5) == half) {
        float4* mine = reinterpret_cast<float4*>(wl + (lane & 31) * REC_DWORDS);
        mine[0] = rq0; mine[1] = rq1; mine[2] = rq2; mine[3] = rq3;
      }
      asm volatile("" ::: "memory");   // (a wave's LDS instructions complete in order)
#pragma unroll
      for (int j = 0; j < 2; j++) {
        const int r = 16 * j + (lane >> 2);        // record of this half the lane carries a quarter of
        const int owner = 32 * half + r;
        if ((recs >> owner) & 1ull)
          reinterpret_cast<float4*>(rec + (wave_first + owner) * REC_DWORDS)[lane & 3] = reinterpret_cast<const float4*>(wl + r * REC_DWORDS)[lane & 3];
      }
      asm volatile("" ::: "memory");
    }
  }
  if (ranges)
    for (int t = idx; t < num_tiles; t += gridDim.x * 256) ranges[t] = make_uint2(RANGE_EMPTY_START, 0u);   // rasterizer_impl.cu:310 ({0,0} there; see kernels.h)
  // workgroup sum of tiles_touched -> block_sums[blockIdx] (feeds the prefix sum, K5); depth range for the sort
  uint32_t s = touched;
  uint32_t dmax = touched ? dbits_mine : 0u, dnmin = touched ? ~dbits_mine : 0u;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    s += __shfl_down(s, off, 64);
    dmax = max(dmax, (uint32_t)__shfl_down((int)dmax, off, 64));
    dnmin = max(dnmin, (uint32_t)__shfl_down((int)dnmin, off, 64));
  }
  if ((threadIdx.x & 63) == 0) {
    wave_sums[threadIdx.x >> 6] = s; wave_dmax[threadIdx.x >> 6] = dmax; wave_dnmin[threadIdx.x >> 6] = dnmin;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    block_sums[blockIdx.x] = wave_sums[0] + wave_sums[1] + wave_sums[2] + wave_sums[3];
    depth_range[blockIdx.x] = max(max(wave_dmax[0], wave_dmax[1]), max(wave_dmax[2], wave_dmax[3]));
    depth_range[gridDim.x + blockIdx.x] = max(max(wave_dnmin[0], wave_dnmin[1]), max(wave_dnmin[2], wave_dnmin[3]));
  }
}

__global__ void __launch_bounds__(256) visible_filter_kernel(
    int P, const float* __restrict__ means3D, const float* __restrict__ scales, float mod,
    const float* __restrict__ rotations, const float* __restrict__ cov3D_precomp,
    const float* __restrict__ viewmatrix, const float* __restrict__ projmatrix, int W, int H,
    float tan_fovx, float tan_fovy, float focal_x, float focal_y, uint32_t gx, uint32_t gy, int* __restrict__ radii,
    int log_scale_stride /* > 0: `scales` holds LOG-scales in rows of this many floats and the first three are used through
    exp(): prefilter_voxel's get_scaling()[:, :3] (src/gaussian_renderer.cpp:150-152) without the intermediate tensor */) {
  __shared__ float lds[768];
  const int idx = blockIdx.x * 256 + threadIdx.x;
  const float3 p = load_row3(means3D, P, lds);
  float3 sc = make_float3(0, 0, 0);
  float4 rot = make_float4(0, 0, 0, 0);
  if (scales) {
    if (log_scale_stride > 0) {
      if (idx < P) {
        const float* r = scales + (size_t)idx * log_scale_stride;
        sc = make_float3(expf(r[0]), expf(r[1]), expf(r[2]));
      }
    } else {
      sc = load_row3(scales, P, lds);
    }
    if (idx < P) rot = reinterpret_cast<const float4*>(rotations)[idx];
  }
  if (idx >= P) return;
  Projected g = project_gaussian(p, sc, mod, rot, cov3D_precomp ? cov3D_precomp + (size_t)6 * idx : nullptr,
                                 viewmatrix, projmatrix, W, H, tan_fovx, tan_fovy, focal_x, focal_y, gx, gy);
  radii[idx] = g.radius;
}

__global__ void __launch_bounds__(256) mark_visible_kernel(int P, const float* __restrict__ means3D,
                                                           const float* __restrict__ viewmatrix, uint8_t* __restrict__ present) {
  __shared__ float lds[768];
  const int idx = blockIdx.x * 256 + threadIdx.x;
  const float3 p = load_row3(means3D, P, lds);
  if (idx >= P) return;
  float3 p_view = transformPoint4x3(p, viewmatrix);
  present[idx] = (p_view.z <= 0.2f) ? 0 : 1;
}

// Workgroup-coalesced store of row `tid` of a (P,3) float array: LDS transpose + three dword sweeps (the mirror of
// load_row3; per-lane 12-byte rows written as three strided dwords filled only a third of every store instruction).
__device__ __forceinline__ void store_row3(float* __restrict__ a, int P, float* lds /*768 floats*/, float x, float y, float z) {
  const int tid = threadIdx.x;
  lds[3 * tid] = x; lds[3 * tid + 1] = y; lds[3 * tid + 2] = z;
  __syncthreads();
  const size_t base = (size_t)blockIdx.x * 768;
  const size_t lim = (size_t)P * 3;
#pragma unroll
  for (int k = 0; k < 3; k++) {
    const size_t i = base + k * 256 + tid;
    if (i < lim) a[i] = lds[k * 256 + tid];
  }
  __syncthreads();
}

// ---- Backward of the per-Gaussian stage: the reference's computeCov2DCUDA + preprocessCUDA + computeCov3D backward
// (backward.cu:144-274, 346-396, 278-341) as ONE pass, derived here from the forward map rather than transcribed:
//
//   t  = Wv p + tv                        view space; t.xy/t.z clamped to +-1.3 tan(fov/2)      (forward.cu:74-113)
//   J  = [[fx/tz, 0, -fx tx/tz^2], [0, fy/tz, -fy ty/tz^2]]                   M2 = J Wv   (2x3)
//   L  = R(q) diag(s),  s = mod * scale,  Sigma = L L^T                       U  = M2 L   (2x3)
//   C  = U U^T + 0.3 I  = [[a, b], [b, c]]                                    conic Q = adj(C) / det
//
// Given the tile kernel's  G = [[gA, gB], [gB, gC]]  (dL/dconic with the off-diagonal stored once, backward.cu:545-549):
//   Dc    = dL/dC = -k adj(C) G adj(C),   k = 1 / (det^2 + 1e-7)             (the reference's guarded 1/det^2, :205)
//   dL/dSigma = M2^T Dc M2                 -> dL_dcov3D (off-diagonals doubled: six unique entries)
//   dL/dM2    = 2 Dc (U L^T)               -> dL/dJ = dL/dM2 Wv^T -> dL/dt  (a clamped coordinate passes nothing, :175-176)
//   dL/dL     = 2 M2^T (Dc U)              -> dL/ds_k = sum_i R_ik dL/dL_ik  (w.r.t. the MODIFIED scale s: the reference
//                                             applies no chain factor for mod, :316-320),  dL/dR_ik = s_k dL/dL_ik -> dL/dq
//                                             through R(q) with q taken as given (no normalisation Jacobian, :340)
//   dL/dp     = Wv^T dL/dt  +  d(ndc.xy)/dp^T (g2x, g2y),   ndc = (PV p).xy / ((PV p).w + 1e-7)                 (:370-387)
// The factorisation through U = M2 L never forms Sigma when scales and rotations are given.
struct Sym2 { float xx, xy, yy; };

__device__ __forceinline__ void quat_rows(float4 q, float R[3][3]) {   // standard rotation matrix of (r, x, y, z), rows
  const float r = q.x, x = q.y, y = q.z, z = q.w;
  R[0][0] = 1.f - 2.f * (y * y + z * z); R[0][1] = 2.f * (x * y - r * z);       R[0][2] = 2.f * (x * z + r * y);
  R[1][0] = 2.f * (x * y + r * z);       R[1][1] = 1.f - 2.f * (x * x + z * z); R[1][2] = 2.f * (y * z - r * x);
  R[2][0] = 2.f * (x * z - r * y);       R[2][1] = 2.f * (y * z + r * x);       R[2][2] = 1.f - 2.f * (x * x + y * y);
}

// One binned Gaussian through the derivation above: the ONE copy of this arithmetic.  Its callers are the lane-per-row body
// (preprocess_bwd_rows, below) and the packed kernel's one heavy wave, so the same inputs give the same bits whichever kernel and
// path a row takes.  a0 = (Mx, My, Mxx, Mxy) of the accumulator row, G = dL/dconic, q = the rotation as stored (the caller loads
// it; unused with cov3D_precomp).  mean2d_from_moments: g2x / g2y = dL/dmean2D (NDC-scaled, backward.cu:541-542) are formed here
// from a0 and the conic; false only for the stage-alone debug entries, whose caller supplies them in g2x / g2y.
// DEPTH: dz is dL/dz of the view-space depth z = V[2] x + V[6] y + V[10] z + V[14] that the depth map composites, which adds
// dL/dz (V[2], V[6], V[10]) to dL/dmean3D.
// CAM: the gradient with respect to the two camera matrices, taken as independent inputs in their transposed layout
// (t_i = sum_j view[4 j + i] p_j + view[12 + i]).  With dt = (dtx, dty, dtz [+ dz]):
//   dL/dview[12 + i] += dt_i                 dL/dview[4 j + i] += dt_i p_j + sum_r J[r][i] dM2[r][j]     (the Wv inside M2 = J Wv)
//   dL/dproj[4 j + i] += dh_i p_j (p_3 = 1), dh = (g2x w, g2y w, 0, -(g2x hom.x + g2y hom.y) w^2)
// 12 + 12 live sums (row 3 of view and column 2 of proj are structurally zero): cam[] holds view slots 3 j + i (i < 3, j < 4;
// j = 3 is the translation row), then proj slots 12 + 3 j + {x, y, w}.
template <bool DEPTH, bool CAM>
__device__ __forceinline__ void projection_backward_row(
    size_t idx, float3 mean, float3 scale, float4 q, float mod, const float* __restrict__ cov3D_precomp, bool has_scales, bool want_cov,
    bool mean2d_from_moments, const float* __restrict__ view, const float* __restrict__ proj, float h_x, float h_y, float tan_fovx,
    float tan_fovy, float img_w, float img_h, float4 a0, Sym2 G, float dz, float& g2x, float& g2y, float (&out_mean)[3],
    float (&out_cov)[6], float (&out_scale)[3], float (&out_rot)[4], float (&cam)[CAM ? CAM_SUMS : 1]) {
  // ---- forward quantities again (cheaper than storing them: 36 B of inputs against ~30 floats of intermediates)
  const float tx0 = view[0] * mean.x + view[4] * mean.y + view[8] * mean.z + view[12];
  const float ty0 = view[1] * mean.x + view[5] * mean.y + view[9] * mean.z + view[13];
  const float tz = view[2] * mean.x + view[6] * mean.y + view[10] * mean.z + view[14];
  const float limx = 1.3f * tan_fovx, limy = 1.3f * tan_fovy;
  const float rx = tx0 / tz, ry = ty0 / tz;
  const bool free_x = !(rx < -limx || rx > limx), free_y = !(ry < -limy || ry > limy);
  const float tx = fminf(limx, fmaxf(-limx, rx)) * tz, ty = fminf(limy, fmaxf(-limy, ry)) * tz;
  const float iz = 1.f / tz, iz2 = iz * iz;
  const float J00 = h_x * iz, J02 = -h_x * tx * iz2, J11 = h_y * iz, J12 = -h_y * ty * iz2;
  float M2[2][3];   // M2 = J Wv,  Wv[i][j] = view[4 j + i]
#pragma unroll
  for (int j = 0; j < 3; j++) {
    M2[0][j] = J00 * view[4 * j] + J02 * view[4 * j + 2];
    M2[1][j] = J11 * view[4 * j + 1] + J12 * view[4 * j + 2];
  }
  float R[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}}, s3[3] = {0, 0, 0};
  float E[2][3];    // E = M2 Sigma (= U L^T)
  float U[2][3] = {{0, 0, 0}, {0, 0, 0}};
  float a, b, c;
  if (cov3D_precomp) {
    const float* cv = cov3D_precomp + (size_t)6 * idx;
    const float S[3][3] = {{cv[0], cv[1], cv[2]}, {cv[1], cv[3], cv[4]}, {cv[2], cv[4], cv[5]}};
#pragma unroll
    for (int r = 0; r < 2; r++)
#pragma unroll
      for (int j = 0; j < 3; j++) E[r][j] = M2[r][0] * S[0][j] + M2[r][1] * S[1][j] + M2[r][2] * S[2][j];
    a = E[0][0] * M2[0][0] + E[0][1] * M2[0][1] + E[0][2] * M2[0][2] + 0.3f;
    b = E[0][0] * M2[1][0] + E[0][1] * M2[1][1] + E[0][2] * M2[1][2];
    c = E[1][0] * M2[1][0] + E[1][1] * M2[1][1] + E[1][2] * M2[1][2] + 0.3f;
    q = make_float4(0, 0, 0, 0);
  } else {
    quat_rows(q, R);
    s3[0] = mod * scale.x; s3[1] = mod * scale.y; s3[2] = mod * scale.z;
#pragma unroll
    for (int r = 0; r < 2; r++)
#pragma unroll
      for (int k = 0; k < 3; k++) U[r][k] = (M2[r][0] * R[0][k] + M2[r][1] * R[1][k] + M2[r][2] * R[2][k]) * s3[k];
#pragma unroll
    for (int r = 0; r < 2; r++)
#pragma unroll
      for (int j = 0; j < 3; j++) E[r][j] = U[r][0] * R[j][0] * s3[0] + U[r][1] * R[j][1] * s3[1] + U[r][2] * R[j][2] * s3[2];
    a = U[0][0] * U[0][0] + U[0][1] * U[0][1] + U[0][2] * U[0][2] + 0.3f;
    b = U[0][0] * U[1][0] + U[0][1] * U[1][1] + U[0][2] * U[1][2];
    c = U[1][0] * U[1][0] + U[1][1] * U[1][1] + U[1][2] * U[1][2] + 0.3f;
  }
  // ---- Dc = -k adj(C) G adj(C)
  const float det = a * c - b * b;
  const float k = 1.0f / (det * det + 0.0000001f);
  if (mean2d_from_moments) {   // with the conic (c, -b, a) / det (forward.cu:217-218)
    const float di = 1.0f / det;
    const float cA = c * di, cB = -b * di, cC = a * di;
    g2x = -(cA * a0.x + cB * a0.y) * (0.5f * img_w);
    g2y = -(cC * a0.y + cB * a0.x) * (0.5f * img_h);
  }
  const float h0 = c * G.xx - b * G.xy, h1 = c * G.xy - b * G.yy;     // rows of adj(C) G
  const float h2 = a * G.xy - b * G.xx, h3 = a * G.yy - b * G.xy;
  Sym2 Dc;
  Dc.xx = -k * (h0 * c - h1 * b);
  Dc.xy = -k * (h1 * a - h0 * b);
  Dc.yy = -k * (h3 * a - h2 * b);
  float DM[2][3];   // Dc M2
#pragma unroll
  for (int j = 0; j < 3; j++) { DM[0][j] = Dc.xx * M2[0][j] + Dc.xy * M2[1][j]; DM[1][j] = Dc.xy * M2[0][j] + Dc.yy * M2[1][j]; }
  if (want_cov || cov3D_precomp) {   // dL/dSigma = M2^T Dc M2, six unique entries
    const int ii[6] = {0, 0, 0, 1, 1, 2}, jj[6] = {0, 1, 2, 1, 2, 2};
#pragma unroll
    for (int e = 0; e < 6; e++) {
      const float v = M2[0][ii[e]] * DM[0][jj[e]] + M2[1][ii[e]] * DM[1][jj[e]];
      out_cov[e] = ii[e] == jj[e] ? v : 2.f * v;
    }
  }
  // ---- through M2 = J Wv to t, then to the mean
  float dM2[2][3];
#pragma unroll
  for (int j = 0; j < 3; j++) {
    dM2[0][j] = 2.f * (Dc.xx * E[0][j] + Dc.xy * E[1][j]);
    dM2[1][j] = 2.f * (Dc.xy * E[0][j] + Dc.yy * E[1][j]);
  }
  // dL/dJ[r][i] = sum_j dM2[r][j] Wv[i][j]; only the four structural entries of J
  const float dJ00 = dM2[0][0] * view[0] + dM2[0][1] * view[4] + dM2[0][2] * view[8];
  const float dJ02 = dM2[0][0] * view[2] + dM2[0][1] * view[6] + dM2[0][2] * view[10];
  const float dJ11 = dM2[1][0] * view[1] + dM2[1][1] * view[5] + dM2[1][2] * view[9];
  const float dJ12 = dM2[1][0] * view[2] + dM2[1][1] * view[6] + dM2[1][2] * view[10];
  const float iz3 = iz2 * iz;
  const float dtx = free_x ? -h_x * iz2 * dJ02 : 0.f;
  const float dty = free_y ? -h_y * iz2 * dJ12 : 0.f;
  const float dtz = -h_x * iz2 * dJ00 - h_y * iz2 * dJ11 + 2.f * h_x * tx * iz3 * dJ02 + 2.f * h_y * ty * iz3 * dJ12;
  // projection term: ndc = hom.xy * w,  w = 1 / (hom.w + 1e-7)
  const float hx = proj[0] * mean.x + proj[4] * mean.y + proj[8] * mean.z + proj[12];
  const float hy = proj[1] * mean.x + proj[5] * mean.y + proj[9] * mean.z + proj[13];
  const float hw = proj[3] * mean.x + proj[7] * mean.y + proj[11] * mean.z + proj[15];
  const float w = 1.0f / (hw + 0.0000001f);
  const float ux = hx * w * w, uy = hy * w * w;
#pragma unroll
  for (int j = 0; j < 3; j++) {
    const float from_cov = view[4 * j] * dtx + view[4 * j + 1] * dty + view[4 * j + 2] * dtz;
    const float from_proj = (proj[4 * j] * w - proj[4 * j + 3] * ux) * g2x + (proj[4 * j + 1] * w - proj[4 * j + 3] * uy) * g2y;
    out_mean[j] = from_cov + from_proj;
  }
  if (DEPTH) {
#pragma unroll
    for (int j = 0; j < 3; j++) out_mean[j] += dz * view[4 * j + 2];
  }
  if constexpr (CAM) {
    const float dtz_all = DEPTH ? dtz + dz : dtz;
    const float pm[3] = {mean.x, mean.y, mean.z};
    const float dh0 = g2x * w, dh1 = g2y * w, dh3 = -(g2x * hx + g2y * hy) * (w * w);
#pragma unroll
    for (int j = 0; j < 3; j++) {
      cam[3 * j + 0] = dtx * pm[j] + J00 * dM2[0][j];
      cam[3 * j + 1] = dty * pm[j] + J11 * dM2[1][j];
      cam[3 * j + 2] = dtz_all * pm[j] + (J02 * dM2[0][j] + J12 * dM2[1][j]);
      cam[12 + 3 * j + 0] = dh0 * pm[j];
      cam[12 + 3 * j + 1] = dh1 * pm[j];
      cam[12 + 3 * j + 2] = dh3 * pm[j];
    }
    cam[9] = dtx; cam[10] = dty; cam[11] = dtz_all;
    cam[21] = dh0; cam[22] = dh1; cam[23] = dh3;
  }
  // ---- scales and rotation: dL/dL = 2 M2^T (Dc U)
  if (has_scales) {
    float DU[2][3];
#pragma unroll
    for (int kk = 0; kk < 3; kk++) { DU[0][kk] = Dc.xx * U[0][kk] + Dc.xy * U[1][kk]; DU[1][kk] = Dc.xy * U[0][kk] + Dc.yy * U[1][kk]; }
    float GR[3][3];   // dL/dR
#pragma unroll
    for (int kk = 0; kk < 3; kk++) {
      float ds = 0.f;
#pragma unroll
      for (int i = 0; i < 3; i++) {
        const float dLik = 2.f * (M2[0][i] * DU[0][kk] + M2[1][i] * DU[1][kk]);
        ds += R[i][kk] * dLik;
        GR[i][kk] = dLik * s3[kk];
      }
      out_scale[kk] = ds;
    }
    const float r = q.x, x = q.y, y = q.z, z = q.w;
    out_rot[0] = 2.f * (z * (GR[1][0] - GR[0][1]) + y * (GR[0][2] - GR[2][0]) + x * (GR[2][1] - GR[1][2]));
    out_rot[1] = 2.f * (y * (GR[0][1] + GR[1][0]) + z * (GR[0][2] + GR[2][0]) + r * (GR[2][1] - GR[1][2])) - 4.f * x * (GR[1][1] + GR[2][2]);
    out_rot[2] = 2.f * (x * (GR[0][1] + GR[1][0]) + r * (GR[0][2] - GR[2][0]) + z * (GR[1][2] + GR[2][1])) - 4.f * y * (GR[0][0] + GR[2][2]);
    out_rot[3] = 2.f * (r * (GR[1][0] - GR[0][1]) + x * (GR[0][2] + GR[2][0]) + y * (GR[1][2] + GR[2][1])) - 4.f * z * (GR[0][0] + GR[1][1]);
  }
}

// CAM: a workgroup's 256 x CAM_SUMS values -> its row of cam_partials, on chip: three passes of eight values through the input
// sweeps' staging buffer (lds[value][256 slots], no LDS of its own), then 32 lanes per value add eight slots each and finish with
// five shuffle steps, and 24 floats are plain-stored; camera_grad_reduce_kernel adds the workgroups' rows in a fixed order.  No
// atomics: every operand and the order of every addition are fixed by the slot numbering alone, so the same per-Gaussian inputs
// give the same bits.  deposit(slots, i) puts value i of the calling thread's Gaussian into slots[its row]; all 256 slots must
// get written between them (a row without a binned Gaussian holds zero).
template <class Deposit>
__device__ __forceinline__ void camera_fold(float* lds /*8 x 256 floats*/, float* __restrict__ cam_partials, Deposit deposit) {
  const int v = threadIdx.x >> 5, l = threadIdx.x & 31;
#pragma unroll
  for (int pass = 0; pass < CAM_SUMS / 8; pass++) {
#pragma unroll
    for (int k = 0; k < 8; k++) deposit(lds + k * 256, pass * 8 + k);
    __syncthreads();
    float s = lds[v * 256 + l];
#pragma unroll
    for (int q = 1; q < 8; q++) s += lds[v * 256 + l + 32 * q];
#pragma unroll
    for (int off = 16; off > 0; off >>= 1) s += __shfl_down(s, off, 64);
    if (l == 0) cam_partials[(size_t)blockIdx.x * CAM_SUMS + pass * 8 + v] = s;
    __syncthreads();
  }
}

// The lane-per-row data path, the ONE copy of it: row blockIdx.x * 256 + threadIdx.x in lane threadIdx.x, everything from the
// "row written" decision on -- input sweeps, accumulator rows through a per-wave LDS transpose (and cleared), the conversion
// (projection_backward_row), the camera fold, every output row written exactly once (zeros for a Gaussian that is culled or was
// not reached).  Called by all 256 threads of
//  * preprocess_bwd_kernel: the synchronising backward, SEGS_RASTER_UNPACKED_BACKWARD / SEGS_RASTER_NO_WRITTEN_BYTES and the
//    stage-alone debug entries.  from_rows = (gacc given), row_written from the byte it read itself (or `live` without bytes),
//    clear_bytes = the bytes when consumed rows are cleaned: the body then zeroes each wave's 64-byte run;
//  * preprocess_bwd_packed_kernel's DENSE branch, with the facts of the resident backward as literals, which fold: from_rows,
//    rows_by_bytes and clean_gacc true, no dz_in, and clear_bytes NULL -- that kernel has balloted its 256 bytes and its wave 3 is
//    already zeroing them, so the body must neither read nor clear them again.
// from_rows: gacc rows hold the tile kernel's per-Gaussian sums (gs_layout.h); false: the caller supplied dL_dmean2D / dL_dconic
// directly (segs_debug_preprocess_backward: this stage alone against the oracle) and, CAM only, dz_in = per-Gaussian dL/dz.
// DEPTH (after render_bwd_depth_kernel): row dword [9] holds dL/dz.
// rows_by_bytes: the accumulator rows read are those with row_written set.  In a scene with occlusion most binned Gaussians are
// never reached by the tile backward (about four in five at 3 M Gaussians / 1080p): their rows hold zeros, which this stage used to
// read, write back and push through the whole projection backward to arrive at zeros.  With the bytes only written rows are read,
// cleared (together with their bytes, so the arena stays clean from step to step) and converted; every other lane writes the
// zeros a culled Gaussian writes.  false (no bytes: the synchronising backward, SEGS_RASTER_NO_WRITTEN_BYTES): every binned
// Gaussian's row is read.
// lds / gl: the caller's __shared__ staging (3 x 768 floats for the sweeps, 32 rows per wave for the transpose).
template <bool DEPTH, bool CAM>
__device__ __forceinline__ void preprocess_bwd_rows(
    int P, const float* __restrict__ means3D, const int* __restrict__ radii, const float* __restrict__ scales,
    const float* __restrict__ rotations, float mod, const float* __restrict__ cov3D_precomp,
    const float* __restrict__ view, const float* __restrict__ proj, float h_x, float h_y, float tan_fovx, float tan_fovy,
    float* __restrict__ gacc, float img_w, float img_h,
    float* __restrict__ dL_dmean2D, float* __restrict__ dL_dconic,
    float* __restrict__ dL_dopacity, float* __restrict__ dL_dcolor, float* __restrict__ dL_dmean3D,
    float* __restrict__ dL_dcov3D, float* __restrict__ dL_dscale, float* __restrict__ dL_drot,
    bool clean_gacc /* write zeros back over the consumed accumulator row (resident backward) */,
    const float* __restrict__ dz_in, float* __restrict__ cam_partials /* CAM: CAM_SUMS floats per workgroup */,
    bool from_rows, bool row_written, bool rows_by_bytes, uint8_t* __restrict__ clear_bytes,
    float* lds /*3 x 768 floats*/, float (*gl)[32 * GACC_DWORDS] /*one per wave, 16-byte aligned*/) {
  const int idx = blockIdx.x * 256 + threadIdx.x;
  const bool live = idx < P;
  const bool binned = live && radii[idx] > 0 && row_written;   // from here on: binned AND reached by the tile backward
  float3 mean, scale, unused;
  load_rows3(means3D, scales, nullptr, P, lds, mean, scale, unused);

  // ---- what arrives from the tile kernel
  float g2x = 0.f, g2y = 0.f;            // dL/dmean2D, NDC-scaled (backward.cu:541-542)
  Sym2 G{0.f, 0.f, 0.f};                 // dL/dconic
  float dcol0 = 0.f, dcol1 = 0.f, dcol2 = 0.f, dop = 0.f, dz = 0.f;
  float4 a0 = make_float4(0.f, 0.f, 0.f, 0.f), a1 = a0;   // the tile kernel's row: Mx My Mxx Mxy | Myy dL/dopacity Sr Sg | Sb
  if (from_rows) {
    // Rows hold raw moments (render.hip): sums over the (pixel, Gaussian) pairs of w = dL/dG * G times 1, dx, dy, dx^2, ...;
    // the reference's per-pair terms (backward.cu:541-554) are linear in them:
    //   dL/dmean2D.x = -(A Mx + B My) W/2,  .y = -(C My + B Mx) H/2,  dL/dconic = -(Mxx, Mxy, Myy)/2
    // with (A, B, C) the conic, formed below from this kernel's own 2D covariance (round 2 gathered it -- and the opacity, which
    // the tile kernel now divides out itself -- from the 32-byte emit record: 9 % of this kernel's traffic).
    // The rows arrive (and are cleared) through a per-wave LDS transpose, like K1's records: a lane reading its own row as
    // two float4 and a dword makes each load touch 64 lines; transposed, an instruction moves sixteen whole rows.
    {
      const int lane = threadIdx.x & 63;
      float* const wl = gl[threadIdx.x >> 6];
      // only binned Gaussians' rows can have been touched by the tile kernel; with the bytes, exactly the rows that were
      const uint64_t rows = __ballot(rows_by_bytes ? row_written : binned);
      const size_t wave_first = (size_t)blockIdx.x * 256 + (threadIdx.x & ~63);
      // the consumed bytes: the wave's whole 64-byte run as sixteen dwords (the region is padded past P, gs_layout.h)
      if (clear_bytes && rows != 0ull && lane < 16 && wave_first + 4 * lane < (size_t)P)
        reinterpret_cast<uint32_t*>(clear_bytes + wave_first)[lane] = 0u;
#pragma unroll
      for (int half = 0; half < 2; half++) {
        float4 q[2];
#pragma unroll
        for (int j = 0; j < 2; j++) {
          const int r = 16 * j + (lane >> 2), owner = 32 * half + r;
          q[j] = make_float4(0.f, 0.f, 0.f, 0.f);
          if (((rows >> owner) & 1ull) && (lane & 3) < 3) {
            float4* src = reinterpret_cast<float4*>(gacc + (wave_first + owner) * GACC_DWORDS) + (lane & 3);
            q[j] = *src;
            if (clean_gacc) *src = make_float4(0.f, 0.f, 0.f, 0.f);
          }
        }
#pragma unroll
        for (int j = 0; j < 2; j++) reinterpret_cast<float4*>(wl + (16 * j + (lane >> 2)) * GACC_DWORDS)[lane & 3] = q[j];
        asm volatile("" ::: "memory");   // (a wave's LDS instructions complete in order)
        if ((lane >> 5) == half) {
          const float4* mine = reinterpret_cast<const float4*>(wl + (lane & 31) * GACC_DWORDS);
          a0 = mine[0]; a1 = mine[1]; dcol2 = wl[(lane & 31) * GACC_DWORDS + 8];
          if (DEPTH) dz = wl[(lane & 31) * GACC_DWORDS + 9];
        }
        asm volatile("" ::: "memory");
      }
    }
    if (binned) {
      G.xx = -0.5f * a0.z; G.xy = -0.5f * a0.w; G.yy = -0.5f * a1.x;
      dop = a1.y;
      dcol0 = a1.z; dcol1 = a1.w;
    }
    store_row3(dL_dcolor, P, lds, dcol0, dcol1, dcol2);
    if (live) {
      if (dL_dconic) reinterpret_cast<float4*>(dL_dconic)[idx] = make_float4(G.xx, G.xy, 0.f, G.yy);   // internal product: optional
      dL_dopacity[idx] = dop;
    }
  } else if (live) {
    g2x = dL_dmean2D[3 * (size_t)idx + 0]; g2y = dL_dmean2D[3 * (size_t)idx + 1];
    G.xx = dL_dconic[4 * (size_t)idx + 0]; G.xy = dL_dconic[4 * (size_t)idx + 1]; G.yy = dL_dconic[4 * (size_t)idx + 3];
    if constexpr (CAM && DEPTH) { if (dz_in) dz = dz_in[idx]; }
  }

  float out_mean[3] = {0, 0, 0}, out_cov[6] = {0, 0, 0, 0, 0, 0}, out_scale[3] = {0, 0, 0}, out_rot[4] = {0, 0, 0, 0};
  float cam[CAM ? CAM_SUMS : 1] = {0};   // CAM: view slots 3 j + i (i < 3, j < 4; j = 3 is the translation row), then proj slots
                                         // 12 + 3 j + {x, y, w}; lanes without a binned Gaussian contribute zero
  if (binned) {
    const float4 rot = cov3D_precomp ? make_float4(0, 0, 0, 0) : reinterpret_cast<const float4*>(rotations)[idx];
    projection_backward_row<DEPTH, CAM>(idx, mean, scale, rot, mod, cov3D_precomp, scales != nullptr, dL_dcov3D != nullptr, from_rows,
                                        view, proj, h_x, h_y, tan_fovx, tan_fovy, img_w, img_h, a0, G, dz, g2x, g2y, out_mean, out_cov,
                                        out_scale, out_rot, cam);
  }
  if constexpr (CAM) camera_fold(lds, cam_partials, [&](float* slots, int i) { slots[threadIdx.x] = cam[i]; });
  if (from_rows) store_row3(dL_dmean2D, P, lds, g2x, g2y, 0.f);
  store_row3(dL_dmean3D, P, lds, out_mean[0], out_mean[1], out_mean[2]);
  if (dL_dscale) store_row3(dL_dscale, P, lds, out_scale[0], out_scale[1], out_scale[2]);
  if (!live) return;
  if (dL_dcov3D) {   // only a caller that passed cov3D_precomp has a use for it
#pragma unroll
    for (int e = 0; e < 6; e++) dL_dcov3D[6 * (size_t)idx + e] = out_cov[e];
  }
  if (dL_drot) reinterpret_cast<float4*>(dL_drot)[idx] = make_float4(out_rot[0], out_rot[1], out_rot[2], out_rot[3]);
}

// Every row in its lane: preprocess_bwd_rows with what this launch was given.  written (with gacc; null = every binned Gaussian's
// row is read): the tile backward's "row written" bytes; the byte is fetched with the body's input sweeps, no dependent round trip
// of its own.  dz_in (CAM only, gacc null): per-Gaussian dL/dz of the stage-alone debug entry.
// (History: when the depth form arrived this was made a template kernel rather than a kernel around an inlined body, because the
// wrapped <false> took 92 instead of 86 VGPRs.  It is a wrapper now, at 90 / 90 / 114 / 108 VGPRs <ff, tf, ft, tt> against 86 / 86 /
// 106 / 106: with an allocation granule of 8 that is the same 5 / 5 / 4 / 4 waves per SIMD, and since the packed kernel it is off
// the resident hot path.)
template <bool DEPTH, bool CAM>
__global__ void __launch_bounds__(256) preprocess_bwd_kernel(
    int P, const float* __restrict__ means3D, const int* __restrict__ radii, const float* __restrict__ scales,
    const float* __restrict__ rotations, float mod, const float* __restrict__ cov3D_precomp,
    const float* __restrict__ view, const float* __restrict__ proj, float h_x, float h_y, float tan_fovx, float tan_fovy,
    float* __restrict__ gacc, float img_w, float img_h,
    float* __restrict__ dL_dmean2D, float* __restrict__ dL_dconic,
    float* __restrict__ dL_dopacity, float* __restrict__ dL_dcolor, float* __restrict__ dL_dmean3D,
    float* __restrict__ dL_dcov3D, float* __restrict__ dL_dscale, float* __restrict__ dL_drot, int clean_gacc,
    const float* __restrict__ dz_in, float* __restrict__ cam_partials, uint8_t* __restrict__ written) {
  __shared__ float lds[3 * 768];
  __shared__ __attribute__((aligned(16))) float gl[4][32 * GACC_DWORDS];
  const int idx = blockIdx.x * 256 + threadIdx.x;
  const bool by_bytes = gacc && written;
  const bool row_written = by_bytes ? (idx < P && written[idx] != 0) : idx < P;
  preprocess_bwd_rows<DEPTH, CAM>(P, means3D, radii, scales, rotations, mod, cov3D_precomp, view, proj, h_x, h_y, tan_fovx, tan_fovy, gacc,
                                  img_w, img_h, dL_dmean2D, dL_dconic, dL_dopacity, dL_dcolor, dL_dmean3D, dL_dcov3D, dL_dscale, dL_drot,
                                  clean_gacc != 0, dz_in, cam_partials, gacc != nullptr, row_written, by_bytes,
                                  by_bytes && clean_gacc ? written : nullptr, lds, gl);
}

#define SEGS_PREPROCESS_BWD_ARGS int, const float*, const int*, const float*, const float*, float, const float*, const float*, \
    const float*, float, float, float, float, float*, float, float, float*, float*, float*, float*, float*, float*, float*, float*, int, \
    const float*, float*, uint8_t*
template __global__ void preprocess_bwd_kernel<false, false>(SEGS_PREPROCESS_BWD_ARGS);
template __global__ void preprocess_bwd_kernel<true, false>(SEGS_PREPROCESS_BWD_ARGS);
template __global__ void preprocess_bwd_kernel<false, true>(SEGS_PREPROCESS_BWD_ARGS);
template __global__ void preprocess_bwd_kernel<true, true>(SEGS_PREPROCESS_BWD_ARGS);
#undef SEGS_PREPROCESS_BWD_ARGS

// Zeros over the workgroup's window of a (P, D) output array: dword sweeps by the `nz` lanes numbered zt = 0 .. nz - 1 over the
// rows < `rows`, leaving out the dwords of reached rows (their heavy lane stores them, in no order with this sweep).
template <int D>
__device__ __forceinline__ void zero_window(float* __restrict__ a, size_t first, int rows, int zt, int nz,
                                            const uint64_t* reached_masks /* LDS: one ballot per wave */) {
  if (!a) return;
  float* const w = a + first * D;
  const int lim = rows * D;
  for (int i = zt; i < lim; i += nz) {
    const int row = i / D;
    if (!((reached_masks[row >> 6] >> (row & 63)) & 1ull)) w[i] = 0.f;
  }
}

// The resident backward with the "row written" bytes, packed (capi.hip: launch_preprocess_bwd).  In a scene with occlusion the tile
// backward reaches about one binned Gaussian in seven (27 of a workgroup's 256 rows at 3 M Gaussians / 1080p), scattered in index
// order, so preprocess_bwd_kernel ran the ~650 instructions of the projection backward in every wave for about 7 live lanes, and
// all four waves went through its dependent round trips and barrier pairs to write rows that are constant zeros.  Here the
// workgroup (256 consecutive rows, as there) reads its 256 bytes, ballots, and clears them as one run when any was set.  Then
//  * SPARSE, at most 64 reached rows: they are prefixed into an LDS list in ascending row order -- local to the workgroup: no
//    global list, no atomics, the row -> Gaussian mapping stays what it was -- and wave 0 alone runs the arithmetic, each lane on
//    one list entry: it fetches its row's radius, mean, scale, rotation and accumulator row (three float4, cleared right away) in
//    one go -- no LDS staging, no barrier between them; the rows lie inside the workgroup's own windows of the arrays -- and
//    stores its row of every output itself.  The zeros of the rows not reached (what a culled Gaussian gets: +0.0, every output,
//    every row < P) depend on nothing the backward computes: waves 1-3 store them straight after the ballot, as coalesced dword
//    sweeps over the workgroup's windows that leave out the reached rows' dwords -- no dependency on wave 0, no barrier.  (Whole
//    windows with a barrier in front of wave 0's stores: 3 us slower at 3 M Gaussians; non-temporal stores: no different;
//    profiles/r07_packed_rows.txt.)  CAM: a lane of wave 0 deposits its 24 values in the slot of its row's ORIGINAL lane, all
//    other slots hold zeros, and camera_fold sums them: the same operands in the same order as on the lane-per-row path, the
//    same bits;
//  * DENSE, more than 64: every row keeps its lane and the workgroup calls preprocess_bwd_rows, the body of preprocess_bwd_kernel
//    -- coalesced sweeps and LDS transposes.  Per-lane rows written as strided dwords cost more than packing saves once most
//    lanes have one (with several heavy waves per workgroup this kernel was 23 % SLOWER than preprocess_bwd_kernel at 0.41
//    reached, 15 % where nearly all are).
// Always with gacc, written and the write-back of zeros over consumed rows (the resident backward).
template <bool DEPTH, bool CAM>
__global__ void __launch_bounds__(256) preprocess_bwd_packed_kernel(
    int P, const float* __restrict__ means3D, const int* __restrict__ radii, const float* __restrict__ scales,
    const float* __restrict__ rotations, float mod, const float* __restrict__ cov3D_precomp,
    const float* __restrict__ view, const float* __restrict__ proj, float h_x, float h_y, float tan_fovx, float tan_fovy,
    float* __restrict__ gacc, float img_w, float img_h,
    float* __restrict__ dL_dmean2D, float* __restrict__ dL_dconic,
    float* __restrict__ dL_dopacity, float* __restrict__ dL_dcolor, float* __restrict__ dL_dmean3D,
    float* __restrict__ dL_dcov3D, float* __restrict__ dL_dscale, float* __restrict__ dL_drot,
    float* __restrict__ cam_partials, uint8_t* __restrict__ written) {
  __shared__ float lds[3 * 768];
  __shared__ __attribute__((aligned(16))) float gl[4][32 * GACC_DWORDS];
  __shared__ uint64_t wave_mask[4];
  __shared__ uint16_t list[64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const size_t first = (size_t)blockIdx.x * 256;
  const int rows = (size_t)P - first < 256 ? (int)((size_t)P - first) : 256;   // of this workgroup that exist
  const bool live = tid < rows;
  const bool reached = live && written[first + tid] != 0;
  const uint64_t mask = __ballot(reached);
  if (lane == 0) wave_mask[wave] = mask;
  __syncthreads();
  const int c0 = __popcll(wave_mask[0]), c1 = __popcll(wave_mask[1]), c2 = __popcll(wave_mask[2]), c3 = __popcll(wave_mask[3]);
  const int n = __builtin_amdgcn_readfirstlane(c0 + c1 + c2 + c3);
  // every byte has been read by now: the consumed ones go back to zero as one run (the region is padded past P, gs_layout.h)
  if (n > 0 && wave == 3 && lane * 4 < rows) reinterpret_cast<uint32_t*>(written + first)[lane] = 0u;

  if (n > 64) {
    // ---- DENSE: row `tid` in lane `tid`, the bytes balloted and cleared above
    preprocess_bwd_rows<DEPTH, CAM>(P, means3D, radii, scales, rotations, mod, cov3D_precomp, view, proj, h_x, h_y, tan_fovx, tan_fovy, gacc,
                                    img_w, img_h, dL_dmean2D, dL_dconic, dL_dopacity, dL_dcolor, dL_dmean3D, dL_dcov3D, dL_dscale, dL_drot,
                                    /*clean_gacc*/ true, /*dz_in*/ nullptr, cam_partials, /*from_rows*/ true, reached,
                                    /*rows_by_bytes*/ true, /*clear_bytes*/ nullptr, lds, gl);
    return;
  }

  // ---- SPARSE
  float g2x = 0.f, g2y = 0.f;
  Sym2 G{0.f, 0.f, 0.f};
  float dcol0 = 0.f, dcol1 = 0.f, dcol2 = 0.f, dop = 0.f, dz = 0.f;
  float out_mean[3] = {0, 0, 0}, out_cov[6] = {0, 0, 0, 0, 0, 0}, out_scale[3] = {0, 0, 0}, out_rot[4] = {0, 0, 0, 0};
  float cam[CAM ? CAM_SUMS : 1] = {0};
  if (reached) list[(wave > 0 ? c0 : 0) + (wave > 1 ? c1 : 0) + (wave > 2 ? c2 : 0) + __popcll(mask & ((1ull << lane) - 1ull))] = (uint16_t)tid;
  __syncthreads();                                        // the list
  const bool heavy = wave == 0 && lane < n;
  int r = 0;
  size_t g = first;
  if (wave == 0) {
    int radius = 0;
    float3 mean = make_float3(0, 0, 0), scale = mean;
    float4 rot = make_float4(0, 0, 0, 0), a0 = rot, a1 = rot, a2 = rot;
    if (heavy) {   // everything this row needs, in flight together
      r = list[lane];
      g = first + r;
      radius = radii[g];
      mean = make_float3(means3D[3 * g], means3D[3 * g + 1], means3D[3 * g + 2]);
      if (scales) scale = make_float3(scales[3 * g], scales[3 * g + 1], scales[3 * g + 2]);
      float4* const src = reinterpret_cast<float4*>(gacc + g * GACC_DWORDS);
      // no branch around the rotation's load (with cov3D_precomp there are no rotations: the row's first 16 bytes are fetched
      // in their place and never looked at): behind a branch the load's result was copied at the join, and that copy made the
      // wave wait for every load so far before it issued the row's -- a dependent round trip, 4 us at 3 M Gaussians
      rot = *(cov3D_precomp ? src : reinterpret_cast<const float4*>(rotations) + g);
      a0 = src[0]; a1 = src[1]; a2 = src[2];
      const float4 z4 = make_float4(0.f, 0.f, 0.f, 0.f);
      src[0] = z4; src[1] = z4; src[2] = z4;
      dcol2 = a2.x;   // (as there: dword [8] leaves whatever the radius says)
      if (DEPTH) dz = a2.y;
    }
    if (heavy && radius > 0) {
      G.xx = -0.5f * a0.z; G.xy = -0.5f * a0.w; G.yy = -0.5f * a1.x;
      dop = a1.y;
      dcol0 = a1.z; dcol1 = a1.w;
    }
    if (heavy) {   // (in the order of preprocess_bwd_rows: what needs no arithmetic leaves before it)
      dL_dcolor[3 * g] = dcol0; dL_dcolor[3 * g + 1] = dcol1; dL_dcolor[3 * g + 2] = dcol2;
      if (dL_dconic) reinterpret_cast<float4*>(dL_dconic)[g] = make_float4(G.xx, G.xy, 0.f, G.yy);
      dL_dopacity[g] = dop;
    }
    if (heavy && radius > 0) {
      projection_backward_row<DEPTH, CAM>(g, mean, scale, rot, mod, cov3D_precomp, scales != nullptr, dL_dcov3D != nullptr, true, view, proj, h_x,
                                          h_y, tan_fovx, tan_fovy, img_w, img_h, a0, G, dz, g2x, g2y, out_mean, out_cov, out_scale, out_rot, cam);
    }
    if (heavy) {
      dL_dmean2D[3 * g] = g2x; dL_dmean2D[3 * g + 1] = g2y; dL_dmean2D[3 * g + 2] = 0.f;
      dL_dmean3D[3 * g] = out_mean[0]; dL_dmean3D[3 * g + 1] = out_mean[1]; dL_dmean3D[3 * g + 2] = out_mean[2];
      if (dL_dscale) { dL_dscale[3 * g] = out_scale[0]; dL_dscale[3 * g + 1] = out_scale[1]; dL_dscale[3 * g + 2] = out_scale[2]; }
      if (dL_dcov3D) {
#pragma unroll
        for (int k = 0; k < 6; k++) dL_dcov3D[6 * g + k] = out_cov[k];
      }
      if (dL_drot) reinterpret_cast<float4*>(dL_drot)[g] = make_float4(out_rot[0], out_rot[1], out_rot[2], out_rot[3]);
    }
  } else {
    const int zt = tid - 64, nz = 192;
    zero_window<3>(dL_dcolor, first, rows, zt, nz, wave_mask);
    zero_window<4>(dL_dconic, first, rows, zt, nz, wave_mask);
    zero_window<1>(dL_dopacity, first, rows, zt, nz, wave_mask);
    zero_window<3>(dL_dmean2D, first, rows, zt, nz, wave_mask);
    zero_window<3>(dL_dmean3D, first, rows, zt, nz, wave_mask);
    zero_window<3>(dL_dscale, first, rows, zt, nz, wave_mask);
    zero_window<6>(dL_dcov3D, first, rows, zt, nz, wave_mask);
    zero_window<4>(dL_drot, first, rows, zt, nz, wave_mask);
  }
  // the fold over lds[value][original lane]: the slots of reached rows come from wave 0's lanes, every other slot is this
  // thread's own zero (disjoint, so the fold's one barrier covers both)
  if constexpr (CAM) camera_fold(lds, cam_partials, [&](float* slots, int i) {
    if (!reached) slots[tid] = 0.f;
    if (heavy) slots[r] = cam[i];
  });
}

#define SEGS_PREPROCESS_BWD_PACKED_ARGS int, const float*, const int*, const float*, const float*, float, const float*, const float*, \
    const float*, float, float, float, float, float*, float, float, float*, float*, float*, float*, float*, float*, float*, float*, \
    float*, uint8_t*
template __global__ void preprocess_bwd_packed_kernel<false, false>(SEGS_PREPROCESS_BWD_PACKED_ARGS);
template __global__ void preprocess_bwd_packed_kernel<true, false>(SEGS_PREPROCESS_BWD_PACKED_ARGS);
template __global__ void preprocess_bwd_packed_kernel<false, true>(SEGS_PREPROCESS_BWD_PACKED_ARGS);
template __global__ void preprocess_bwd_packed_kernel<true, true>(SEGS_PREPROCESS_BWD_PACKED_ARGS);
#undef SEGS_PREPROCESS_BWD_PACKED_ARGS

// The workgroups' CAM_SUMS-float rows (preprocess_bwd_kernel<., true>) -> dL/dviewmatrix and dL/dprojmatrix, all 32 floats written.
// ONE workgroup of 960 threads = 160 rows x 6 float4 per sweep: a thread keeps its float4 column and adds the rows r0, r0 + 160, ...
// in that order, then 10 x 16 and 1 x 10 more additions through LDS -- a fixed tree, so the result does not depend on timing.
__global__ void __launch_bounds__(960) camera_grad_reduce_kernel(const float* __restrict__ partials, int nblocks,
                                                                 float* __restrict__ dL_dview, float* __restrict__ dL_dproj) {
  __shared__ float rows[160 * CAM_SUMS];
  __shared__ float mid[10 * CAM_SUMS];
  __shared__ float sums[CAM_SUMS];
  const int t = threadIdx.x, q = t % 6, r0 = t / 6;
  float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll 8
  for (int r = r0; r < nblocks; r += 160) {
    const float4 x = reinterpret_cast<const float4*>(partials + (size_t)r * CAM_SUMS)[q];
    acc.x += x.x; acc.y += x.y; acc.z += x.z; acc.w += x.w;
  }
  reinterpret_cast<float4*>(rows + r0 * CAM_SUMS)[q] = acc;
  __syncthreads();
  if (t < 10 * CAM_SUMS) {
    const int v = t % CAM_SUMS, g = t / CAM_SUMS;
    float s = 0.f;
    for (int k = 0; k < 16; k++) s += rows[(16 * g + k) * CAM_SUMS + v];
    mid[g * CAM_SUMS + v] = s;
  }
  __syncthreads();
  if (t < CAM_SUMS) {
    float s = 0.f;
    for (int g = 0; g < 10; g++) s += mid[g * CAM_SUMS + t];
    sums[t] = s;
  }
  __syncthreads();
  if (t < 32) {
    const int e = t & 15, i = e & 3, j = e >> 2;
    if (t < 16) dL_dview[e] = i < 3 ? sums[3 * j + i] : 0.f;                            // dL/dview[4 j + 3] = 0
    else dL_dproj[e] = i != 2 ? sums[12 + 3 * j + (i == 3 ? 2 : i)] : 0.f;              // column i = 2 never enters the render
  }
}

// SH colour branch only (callers that pass `shs`; off the live SEGS-SLAM path): dL/dsh and the view-direction term of
// dL/dmean3D from the summed dL/dcolor (backward.cu:390-391), as a pass of its own so that its tables stay out of the
// per-Gaussian backward every training step runs.
__global__ void __launch_bounds__(256) sh_backward_kernel(int P, const float* __restrict__ means3D, const int* __restrict__ radii,
                                                          const float* __restrict__ shs, int D, int M, const float* __restrict__ cam_pos,
                                                          const uint32_t* __restrict__ clamped, const float* __restrict__ dL_dcolor,
                                                          float* __restrict__ dL_dmean3D, float* __restrict__ dL_dsh) {
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= P || radii[idx] <= 0) return;
  const float3 mean = make_float3(means3D[3 * (size_t)idx], means3D[3 * (size_t)idx + 1], means3D[3 * (size_t)idx + 2]);
  const float3 dcol = make_float3(dL_dcolor[3 * (size_t)idx], dL_dcolor[3 * (size_t)idx + 1], dL_dcolor[3 * (size_t)idx + 2]);
  const float3 g = sh::backward(idx, D, M, mean, cam_pos, shs, clamped[idx], dcol, dL_dsh);
  dL_dmean3D[3 * (size_t)idx] += g.x; dL_dmean3D[3 * (size_t)idx + 1] += g.y; dL_dmean3D[3 * (size_t)idx + 2] += g.z;
}

}  // namespace segs
