// depth_loss.hip -- depth supervision of the mapper / tracking step from an RGB-D frame (include/segs_train.h).
// The reference reads the sensor depth only to back-project new points (src/gaussian_mapper.cpp:1673-1676); its validity rule
// (finite, strictly inside (min_depth, max_depth)) is what makes a pixel count here.  D = rendered depth (sum z alpha T),
// A = rendered opacity (1 - T_final), Z = sensor depth:
//   depth_target_kernel : Z -> T = Z where valid else 0, N = number of valid pixels (exact: integer atomics); once per keyframe;
//   depth_loss_kernel   : D, A, T -> dL/dD, dL/dA and one (sum |d - Z|, sum (1 - A), used count) slot per workgroup;
//   depth_loss_finish_kernel : ONE workgroup folds the slots in a fixed order, divides by n = max(N, 1) (read from the device
//                         word behind T: no host synchronisation) and writes the four result words.
// 24 B per pixel (three maps read, two written).  The gradient scale depends on N alone, so the streaming pass needs nothing from
// its own sums and the value is the only thing the second, tiny launch produces: no float atomics, the same bits on every run.
// Built with -ffp-contract=off: total = lambda_depth * L_depth + lambda_alpha * L_alpha and *loss_inout += total are each the
// float32 operations they are written as.
#include <hip/hip_runtime.h>
#include <cfloat>
#include <cstdint>
#include "../../include/segs_raster.h"
#include "kernels.h"
#include "../../include/segs_train.h"

namespace {
// A 256-thread workgroup covers a span of SPAN = 1024 consecutive pixels of the flat (H*W) map, four per thread.
//  * vector form (every pointer 16-byte aligned): thread t owns pixels 4t .. 4t+3 of the span, one dwordx4 per map; the last
//    H*W mod 4 pixels of the map go one by one;
//  * scalar form (any 4-byte-aligned pointer): thread t owns pixels t, t+256, t+512, t+768 (coalesced dword accesses).
// All loads of a thread are issued before the first use.  1200 x 680: 797 workgroups, three per CU.
constexpr int BLOCK = 256;
constexpr int PER_THREAD = 4;
constexpr int SPAN = BLOCK * PER_THREAD;

__device__ __forceinline__ bool depth_valid(float z, float min_depth, float max_depth) {
  // z > min_depth is false for NaN; z <= FLT_MAX drops +inf (the reference's cv::Mat test has no infinities to drop)
  return z > min_depth && z <= FLT_MAX && (max_depth <= 0.f || z < max_depth);
}

template <bool VEC>
__device__ __forceinline__ void load4(const float* __restrict__ src, size_t base, size_t n, float (&v)[PER_THREAD]) {
  const int tid = threadIdx.x;
  if (VEC) {
    const size_t i = base + (size_t)tid * PER_THREAD;
    if (i + PER_THREAD <= n) {
      const float4 q = *reinterpret_cast<const float4*>(src + i);
      v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
    } else {
#pragma unroll
      for (int e = 0; e < PER_THREAD; e++) v[e] = i + e < n ? src[i + e] : 0.f;
    }
  } else {
#pragma unroll
    for (int e = 0; e < PER_THREAD; e++) {
      const size_t i = base + (size_t)e * BLOCK + tid;
      v[e] = i < n ? src[i] : 0.f;
    }
  }
}

template <bool VEC>
__device__ __forceinline__ void store4(float* __restrict__ dst, size_t base, size_t n, const float (&v)[PER_THREAD]) {
  const int tid = threadIdx.x;
  if (VEC) {
    const size_t i = base + (size_t)tid * PER_THREAD;
    if (i + PER_THREAD <= n) {
      *reinterpret_cast<float4*>(dst + i) = make_float4(v[0], v[1], v[2], v[3]);
    } else {
#pragma unroll
      for (int e = 0; e < PER_THREAD; e++)
        if (i + e < n) dst[i + e] = v[e];
    }
  } else {
#pragma unroll
    for (int e = 0; e < PER_THREAD; e++) {
      const size_t i = base + (size_t)e * BLOCK + tid;
      if (i < n) dst[i] = v[e];
    }
  }
}

// pixel index of element e of this thread (for the in-range test of the sums)
template <bool VEC>
__device__ __forceinline__ size_t pixel_of(size_t base, int e) {
  return VEC ? base + (size_t)threadIdx.x * PER_THREAD + e : base + (size_t)e * BLOCK + threadIdx.x;
}

template <bool VEC>
__global__ void __launch_bounds__(BLOCK) depth_target_kernel(const float* __restrict__ sensor, size_t n, float min_depth, float max_depth,
                                                             float* __restrict__ target, uint32_t* __restrict__ count) {
  __shared__ uint32_t red[BLOCK / 64];
  const size_t base = (size_t)blockIdx.x * SPAN;
  float z[PER_THREAD], t[PER_THREAD];
  load4<VEC>(sensor, base, n, z);
  uint32_t c = 0;
#pragma unroll
  for (int e = 0; e < PER_THREAD; e++) {
    const bool ok = pixel_of<VEC>(base, e) < n && depth_valid(z[e], min_depth, max_depth);
    t[e] = ok ? z[e] : 0.f;
    c += ok ? 1u : 0u;
  }
  store4<VEC>(target, base, n, t);
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) c += __shfl_down(c, off, 64);
  const int tid = threadIdx.x;
  if ((tid & 63) == 0) red[tid >> 6] = c;
  __syncthreads();
  if (tid == 0) {
    const uint32_t total = red[0] + red[1] + red[2] + red[3];
    if (total) atomicAdd(count, total);
  }
}

template <bool VEC, bool NORMALIZE>
__global__ void __launch_bounds__(BLOCK) depth_loss_kernel(const float* __restrict__ depth, const float* __restrict__ alpha,
                                                           const float* __restrict__ target, size_t n, const uint32_t* __restrict__ n_valid,
                                                           float lambda_depth, float lambda_alpha, float alpha_min,
                                                           float* __restrict__ dL_ddepth, float* __restrict__ dL_dalpha,
                                                           float2* __restrict__ partial, uint32_t* __restrict__ partial_used) {
  __shared__ float r1[BLOCK / 64], r2[BLOCK / 64];
  __shared__ uint32_t r3[BLOCK / 64];
  const size_t base = (size_t)blockIdx.x * SPAN;
  float D[PER_THREAD], A[PER_THREAD], Z[PER_THREAD];
  load4<VEC>(depth, base, n, D);
  load4<VEC>(alpha, base, n, A);
  load4<VEC>(target, base, n, Z);
  const uint32_t N = *n_valid;
  const float nf = (float)(N > 1u ? N : 1u);
  const float gd = lambda_depth / nf, ga = lambda_alpha / nf;   // the gradient scale: known from the target alone
  float gD[PER_THREAD], gA[PER_THREAD];
  float sum_abs = 0.f, sum_alpha = 0.f;
  uint32_t used_count = 0;
#pragma unroll
  for (int e = 0; e < PER_THREAD; e++) {
    const bool valid = Z[e] > 0.f;                     // invalid pixels and the out-of-range tail read 0
    const bool used = valid && A[e] >= alpha_min;
    float d = D[e];
    if (NORMALIZE) d = used ? D[e] / A[e] : 0.f;       // (alpha_min > 0: A > 0 on used pixels)
    const float diff = d - Z[e];
    const float s = diff > 0.f ? 1.f : (diff < 0.f ? -1.f : 0.f);
    float a_grad = valid ? 0.f - ga : 0.f;        // (0 - x, not -x: a zero weight leaves +0)
    float d_grad = 0.f;
    if (used) {
      sum_abs += fabsf(diff);
      used_count += 1u;
      if (NORMALIZE) {
        d_grad = s * (gd / A[e]);                      // dL/dD = lambda s / (n A)
        a_grad = 0.f - d_grad * d - ga;                // dL/dA = -lambda s D / (n A^2) - lambda_alpha / n
      } else {
        d_grad = s * gd;
      }
    }
    if (valid) sum_alpha += 1.f - A[e];
    gD[e] = d_grad;
    gA[e] = a_grad;
  }
  store4<VEC>(dL_ddepth, base, n, gD);
  store4<VEC>(dL_dalpha, base, n, gA);
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    sum_abs += __shfl_down(sum_abs, off, 64);
    sum_alpha += __shfl_down(sum_alpha, off, 64);
    used_count += __shfl_down(used_count, off, 64);
  }
  const int tid = threadIdx.x;
  if ((tid & 63) == 0) { r1[tid >> 6] = sum_abs; r2[tid >> 6] = sum_alpha; r3[tid >> 6] = used_count; }
  __syncthreads();
  if (tid == 0) {
    partial[blockIdx.x] = make_float2((r1[0] + r1[1]) + (r1[2] + r1[3]), (r2[0] + r2[1]) + (r2[2] + r2[3]));
    partial_used[blockIdx.x] = (r3[0] + r3[1]) + (r3[2] + r3[3]);
  }
}

// The value: slot i goes to thread i mod 256, each thread adds its slots in rising order, then the same tree as above.
__global__ void __launch_bounds__(BLOCK) depth_loss_finish_kernel(const float2* __restrict__ partial, const uint32_t* __restrict__ partial_used,
                                                                  int n_partial, const uint32_t* __restrict__ n_valid, float lambda_depth,
                                                                  float lambda_alpha, float* __restrict__ loss_out, float* __restrict__ loss_inout) {
  __shared__ float r1[BLOCK / 64], r2[BLOCK / 64];
  __shared__ uint32_t r3[BLOCK / 64];
  const int tid = threadIdx.x;
  float a = 0.f, b = 0.f;
  uint32_t c = 0;
  for (int i = tid; i < n_partial; i += BLOCK) {
    const float2 v = partial[i];
    a += v.x; b += v.y; c += partial_used[i];
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    a += __shfl_down(a, off, 64);
    b += __shfl_down(b, off, 64);
    c += __shfl_down(c, off, 64);
  }
  if ((tid & 63) == 0) { r1[tid >> 6] = a; r2[tid >> 6] = b; r3[tid >> 6] = c; }
  __syncthreads();
  if (tid == 0) {
    const uint32_t N = *n_valid;
    const float nf = (float)(N > 1u ? N : 1u);
    const float l_depth = ((r1[0] + r1[1]) + (r1[2] + r1[3])) / nf, l_alpha = ((r2[0] + r2[1]) + (r2[2] + r2[3])) / nf;
    const float total = lambda_depth * l_depth + lambda_alpha * l_alpha;
    loss_out[0] = total;
    loss_out[1] = l_depth;
    loss_out[2] = l_alpha;
    loss_out[3] = (float)((r3[0] + r3[1]) + (r3[2] + r3[3]));
    if (loss_inout) *loss_inout += total;
  }
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }
size_t n_spans(size_t n) { return (n + SPAN - 1) / SPAN; }
size_t round256(size_t b) { return (b + 255) & ~(size_t)255; }

}  // namespace

extern "C" {

size_t segs_depth_target_floats(int H, int W) { return H > 0 && W > 0 ? (size_t)H * W + 4 : 0; }   // the map, then N (uint32) + 3 spare words

int segs_depth_target(const float* sensor_depth, int H, int W, float min_depth, float max_depth, float* target_out, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  if (!sensor_depth || !target_out || H <= 0 || W <= 0) return segs::set_error(SEGS_ERR_INVALID_ARGUMENT, "invalid argument (null pointer or bad size)");
  if (!(min_depth >= 0.f)) return segs::set_error(SEGS_ERR_INVALID_ARGUMENT, "min_depth must not be negative");
  const size_t n = (size_t)H * W;
  if (n_spans(n) > 0x7FFFFFFFu) return segs::set_error(SEGS_ERR_INVALID_ARGUMENT, "image too large");
  uint32_t* count = reinterpret_cast<uint32_t*>(target_out + n);
  hipError_t e = hipMemsetAsync(count, 0, 4 * sizeof(uint32_t), st);
  if (e != hipSuccess) return segs::set_hip_error(e, __func__);
  const dim3 grid((unsigned)n_spans(n)), block(BLOCK);
  if (aligned16(sensor_depth) && aligned16(target_out))
    depth_target_kernel<true><<<grid, block, 0, st>>>(sensor_depth, n, min_depth, max_depth, target_out, count);
  else
    depth_target_kernel<false><<<grid, block, 0, st>>>(sensor_depth, n, min_depth, max_depth, target_out, count);
  e = hipGetLastError();
  return e == hipSuccess ? SEGS_OK : segs::set_hip_error(e, __func__);
}

size_t segs_depth_loss_temp_bytes(int H, int W) {
  if (H <= 0 || W <= 0) return 0;
  const size_t nblk = n_spans((size_t)H * W);
  return round256(nblk * sizeof(float2)) + round256(nblk * sizeof(uint32_t));
}

int segs_depth_loss(const float* depth, const float* alpha, const float* target, int H, int W, const segs_depth_loss_params* p,
                    float* dL_ddepth, float* dL_dalpha, float* loss_out, float* loss_inout, char* temp, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  if (!depth || !alpha || !target || !p || !dL_ddepth || !dL_dalpha || !loss_out || !temp || H <= 0 || W <= 0)
    return segs::set_error(SEGS_ERR_INVALID_ARGUMENT, "invalid argument (null pointer or bad size)");
  if (p->normalize != 0 && !(p->alpha_min > 0.f))
    return segs::set_error(SEGS_ERR_INVALID_ARGUMENT, "normalize = 1 divides by the opacity: it needs alpha_min > 0");
  const size_t n = (size_t)H * W;
  const size_t nblk = n_spans(n);
  if (nblk > 0x7FFFFFFFu) return segs::set_error(SEGS_ERR_INVALID_ARGUMENT, "image too large");
  float2* partial = reinterpret_cast<float2*>(temp);
  uint32_t* partial_used = reinterpret_cast<uint32_t*>(temp + round256(nblk * sizeof(float2)));
  const uint32_t* n_valid = reinterpret_cast<const uint32_t*>(target + n);
  const bool vec = aligned16(depth) && aligned16(alpha) && aligned16(target) && aligned16(dL_ddepth) && aligned16(dL_dalpha);
  const dim3 grid((unsigned)nblk), block(BLOCK);
#define SEGS_DEPTH_LOSS_LAUNCH(V, NRM)                                                                                              \
  depth_loss_kernel<V, NRM><<<grid, block, 0, st>>>(depth, alpha, target, n, n_valid, p->lambda_depth, p->lambda_alpha, p->alpha_min, \
                                                    dL_ddepth, dL_dalpha, partial, partial_used)
  if (vec) { if (p->normalize) SEGS_DEPTH_LOSS_LAUNCH(true, true); else SEGS_DEPTH_LOSS_LAUNCH(true, false); }
  else     { if (p->normalize) SEGS_DEPTH_LOSS_LAUNCH(false, true); else SEGS_DEPTH_LOSS_LAUNCH(false, false); }
#undef SEGS_DEPTH_LOSS_LAUNCH
  depth_loss_finish_kernel<<<1, block, 0, st>>>(partial, partial_used, (int)nblk, n_valid, p->lambda_depth, p->lambda_alpha, loss_out, loss_inout);
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? SEGS_OK : segs::set_hip_error(e, __func__);
}

}  // extern "C"
