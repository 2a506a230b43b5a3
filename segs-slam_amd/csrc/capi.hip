// capi.hip -- host orchestration + extern "C" entry points declared in include/segs_raster.h.
//
// Mirrors CudaRasterizer::Rasterizer::{forward,backward,visible_filter,markVisible,project2_image}
// (cuda_rasterizer/rasterizer_impl.cu:141-153,198-336,339-393,397-490,494-585) as a C ABI.
// Launch order of forward: K1 preprocess -> K5 scan -> (one host sync for R, as the reference's
// cudaMemcpy at :281) -> K7 duplicate -> K8 radix sort -> K9 ranges -> K10 render.
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <algorithm>
#include <cstring>
#include <string>
#include <vector>
#include "../../include/segs_raster.h"
#include "gs_layout.h"
#include "kernels.h"
#include "capi_args.h"

using namespace segs;

namespace {
thread_local std::string g_err;   // segs_last_error(): message of the last failing entry point on this host thread
}
// Shared by every translation unit of the library (kernels.h): record the message, return the status code.
int segs::set_error(int code, const char* what) {
  g_err = what;
  return code;
}
int segs::set_hip_error(hipError_t e, const char* where) {
  g_err = std::string(where) + ": " + hipGetErrorString(e);
  return (int)e > 0 ? (int)e : 1;
}

namespace {

thread_local uint32_t g_flags = 0u;   // segs_raster_set_flags
thread_local uint32_t* g_status_mirror = nullptr;   // segs_raster_set_status_mirror

int fail(int code, const char* what) { return segs::set_error(code, what); }
int hip_fail(hipError_t e, const char* where) { return segs::set_hip_error(e, where); }
#define HIP_TRY(expr)                                   \
  do {                                                  \
    hipError_t _e = (expr);                             \
    if (_e != hipSuccess) return hip_fail(_e, #expr);   \
  } while (0)
#define LAUNCH_TRY(name)                                \
  do {                                                  \
    hipError_t _e = hipGetLastError();                  \
    if (_e != hipSuccess) return hip_fail(_e, name);    \
  } while (0)

// ---- measurement support: per-kernel HIP-event timing on the launch stream (segs_profile_*) ----
enum KernelId { K_PREPROCESS_FWD = 0, K_SCAN, K_DUPLICATE, K_RADIX_COUNT, K_RADIX_SCAN, K_RADIX_SCATTER, K_RANGES,
                K_RENDER_FWD, K_RENDER_BWD, K_PREPROCESS_BWD, K_MEMSET, K_COUNT };
const char* const kKernelNames[K_COUNT] = {"preprocess_fwd_kernel", "scan_block_sums_kernel", "duplicate_with_keys_kernel",
                                           "radix_count_kernel", "radix_scan_kernel", "radix_scatter_kernel",
                                           "identify_tile_ranges_kernel", "render_fwd_kernel", "render_bwd_kernel",
                                           "preprocess_bwd_kernel", "memset"};
struct Profiler {
  unsigned mask = 0;
  std::vector<hipEvent_t> pool;
  size_t used = 0;
  struct Span { int id; size_t e0, e1; };
  std::vector<Span> spans;
  double total_ms[K_COUNT] = {0};
  long count[K_COUNT] = {0};
  hipEvent_t get() {
    if (used == pool.size()) { hipEvent_t e; if (hipEventCreate(&e) != hipSuccess) return nullptr; pool.push_back(e); }
    return pool[used++];
  }
} g_prof;
struct ProfScope {
  int id; hipStream_t st; size_t e0 = 0; bool on;
  ProfScope(int id_, hipStream_t st_) : id(id_), st(st_), on((g_prof.mask >> id_) & 1u) {
    if (on) { e0 = g_prof.used; hipEvent_t e = g_prof.get(); if (e) (void)hipEventRecord(e, st); else on = false; }
  }
  ~ProfScope() {
    if (on) { size_t e1 = g_prof.used; hipEvent_t e = g_prof.get(); if (e) { (void)hipEventRecord(e, st); g_prof.spans.push_back({id, e0, e1}); } }
  }
};
#define PROF(id) ProfScope _prof_scope_##id(id, st)

// rasterizer_impl.cu:35-50
uint32_t getHigherMsb(uint32_t n) {
  uint32_t msb = sizeof(n) * 4, step = msb;
  while (step > 1) {
    step /= 2;
    if (n >> msb) msb += step; else msb -= step;
  }
  if (n >> msb) msb++;
  return msb;
}

// Tiles per chunk of the count kernel (a workgroup walks its chunk's tiles one after the other; only the chunk totals go
// through the row scan).  Few tiles: one tile per workgroup -- the launch is latency-bound and a 4-tile walk quadruples
// that latency for nothing (50 k Gaussians at 640x480: 0.206 -> 0.187 ms per step with one tile per chunk).  Many tiles:
// longer chunks keep the row scan short (3 M Gaussians at 1080p: 1.102 / 1.108 / 1.126 ms with 4 / 2 / 1).
int count_chunk_tiles(int nblocks) {
#ifdef SEGS_MEASURE   // measurement builds only (tools/): anything but 1, 2 or 4 tiles per chunk is ignored
  static const int chunk_override = [] { const char* e = getenv("SEGS_COUNT_CHUNK"); const int v = e ? atoi(e) : 0; return (v == 1 || v == 2 || v == 4) ? v : 0; }();
  if (chunk_override > 0) return chunk_override;
#endif
  return nblocks <= 256 ? 1 : (nblocks <= 2048 ? 2 : SORT_COUNT_CHUNK_TILES);
}

int check_tile_grid(const View& V) {
  if (V.gx > 0xFFFFu || V.gy > 0xFFFFu) return fail(SEGS_ERR_INVALID_ARGUMENT, "image too large for 16-bit tile coordinates");
  return SEGS_OK;
}
// forwards that run K1: colours and covariances must come from somewhere
int check_colour_and_shape(const Gaussians& g, const View& V) {
  if (!g.colors_precomp && (!g.shs || !V.cam_pos || g.M <= 0 || g.D < 0 || (g.D + 1) * (g.D + 1) > g.M || g.D > 3))
    return fail(SEGS_ERR_INVALID_ARGUMENT, "need colors_precomp, or shs + cam_pos with (D+1)^2 <= M, D <= 3");
  if (!g.cov3D_precomp && (!g.scales || !g.rotations)) return fail(SEGS_ERR_INVALID_ARGUMENT, "need scales+rotations or cov3D_precomp");
  return SEGS_OK;
}

// K8: stable LSD radix sort, BITS bits per pass over key bits [0, end_bit).  Input is expected in side sort_first_side() of
// the ping-pong pair so that the result lands in side 0.  What else a caller may ask of it: SortOptions (capi_args.h).
template <typename K, int BITS>
int sort_pairs_digits(char* bin, const BinningLayout& L, int n, const SortOptions& o, hipStream_t st) {
  if (n <= 0) return SEGS_OK;
  uint32_t* n_live = (uint32_t*)(bin + L.n_live);
  const int end_bit = o.end_bit, passes = (end_bit + BITS - 1) / BITS;
  int side = sort_first_side(end_bit, BITS);
  uint32_t* tile_prefix = (uint32_t*)(bin + L.tile_prefix);
  uint32_t* chunk_hist = (uint32_t*)(bin + L.chunk_hist);
  uint32_t* digit_totals = (uint32_t*)(bin + L.digit_totals);
  const int chunk_tiles = count_chunk_tiles(L.nblocks);
  const int nchunks = (L.nblocks + chunk_tiles - 1) / chunk_tiles;
  for (int p = 0; p < passes; p++) {
    const K* kin = (p == 0 && o.first_keys) ? (const K*)o.first_keys : (const K*)(bin + L.keys[side]);
    const uint32_t* vin = (const uint32_t*)(bin + L.vals[side]);
    K* kout = (K*)(bin + L.keys[side ^ 1]);
    uint32_t* vout = (uint32_t*)(bin + L.vals[side ^ 1]);
    const int shift = BITS * p;
    const int drop = o.drop_dead && p == 0;
    const uint32_t* n_in = (o.drop_dead && p > 0) ? n_live : o.n_dev;
    const int nbits = std::min(BITS, end_bit - shift);   // the last pass may have fewer significant bits than a full digit
    { PROF(K_RADIX_COUNT);
    radix_count_kernel<K, BITS><<<(nchunks + 7) / 8 * 8, SORT_THREADS, 0, st>>>(kin, n, shift, o.dmin, o.dbits, tile_prefix, chunk_hist, L.nblocks, nchunks, n_in, drop, chunk_tiles, nbits);
    }
    LAUNCH_TRY("radix_count_kernel");
    const bool last = p == passes - 1;
    { PROF(K_RADIX_SCAN);
    radix_scan_kernel<<<1 << BITS, 256, 0, st>>>(chunk_hist, nchunks, digit_totals);
    }
    LAUNCH_TRY("radix_scan_kernel");
    if (o.iota_vals && p == 0) vin = nullptr;
    const int scatter_grid = (L.nblocks + 7) / 8 * 8;   // a multiple of the XCD count: see radix_scatter_kernel's tile mapping
    uint2* fr = last ? o.ranges : nullptr;
    uint32_t* fs = last ? o.status : nullptr;
    uint32_t* fm = last ? o.status_mirror : nullptr;
    const int wk = (last && !o.keep_sorted_keys) ? 0 : 1;
    { PROF(K_RADIX_SCATTER);
    bool gathered = false;
    if constexpr (sizeof(K) == 4 && BITS <= 9) {   // the gather form exists for 32-bit keys and the depth sort's digit widths only
      if (o.aux_in && o.aux_final && last) {
        radix_scatter_kernel<K, BITS, true><<<scatter_grid, SORT_THREADS, 0, st>>>(kin, vin, kout, vout, n, shift, o.dmin, o.dbits, tile_prefix, chunk_hist,
                                                                        digit_totals, L.nblocks, nchunks, n_in, drop,
                                                                        drop ? n_live : nullptr, o.aux_in, o.aux_final, nbits, chunk_tiles, 0, fr, fs, fm, wk);
        gathered = true;
      }
    }
    if (!gathered)
      radix_scatter_kernel<K, BITS, false><<<scatter_grid, SORT_THREADS, 0, st>>>(kin, vin, kout, vout, n, shift, o.dmin, o.dbits, tile_prefix, chunk_hist,
                                                                       digit_totals, L.nblocks, nchunks, n_in, drop,
                                                                       drop ? n_live : nullptr, (o.pack_shift > 0 && p == 0) ? o.aux_in : nullptr, nullptr,
                                                                       nbits, chunk_tiles, (p == 0) ? o.pack_shift : 0, fr, fs, fm, wk);
    }
    LAUNCH_TRY("radix_scatter_kernel");
    side ^= 1;
  }
  return SEGS_OK;
}
// the one place that maps the runtime digit width to an instantiation (binning.hip instantiates exactly these)
template <typename K>
int sort_pairs(char* bin, const BinningLayout& L, int n, const SortOptions& o, hipStream_t st) {
  if constexpr (sizeof(K) == 4) {
    if (o.digit_bits == 9) return sort_pairs_digits<K, 9>(bin, L, n, o, st);
    if (o.digit_bits == 11) return sort_pairs_digits<K, 11>(bin, L, n, o, st);
  }
  return sort_pairs_digits<K, 8>(bin, L, n, o, st);
}

bool drop_dead_instances() { return (g_flags & SEGS_RASTER_KEEP_DEAD_INSTANCES) == 0u; }
uint32_t resident_k1_flags() { return drop_dead_instances() ? PREPROCESS_TIGHT_RECT : 0u; }

int run_preprocess(const Geom& G, const Gaussians& g, const View& V, int* radii, const K1Targets& k1, hipStream_t st) {
  { PROF(K_PREPROCESS_FWD);
  preprocess_fwd_kernel<<<G.L.nblocks, 256, 0, st>>>(g.P, g.means3D, g.kernel_scales(), g.scale_modifier, g.rotations, g.opacities, g.colors_precomp,
                                                     g.cov3D_precomp, V.viewmatrix, V.projmatrix, V.width, V.height, V.tan_fovx, V.tan_fovy,
                                                     V.focal_x, V.focal_y, V.gx, V.gy, radii, G.rec(), G.bin(), G.block_sums(),
                                                     G.block_sums() + (G.L.nblocks + 1), g.shs, g.D, g.M, V.cam_pos, G.clamped(),
                                                     g_flags | k1.extra_flags, k1.depth_keys, k1.depth_vals, k1.ranges, (int)V.tiles,
                                                     k1.depth_overflow, G.touched());
  }
  LAUNCH_TRY("preprocess_fwd_kernel");
  return SEGS_OK;
}

// Tile binning (K7, K8, K9).  The reference sorts all R instances on key bits [0, 32+bit) = (tile | depth)
// (rasterizer_impl.cu:300-308).  Same order, far less traffic: (1) stable-sort the P GAUSSIANS by depth (P << R),
// (2) emit instances in that order, (3) stable-sort the R instances by tile id only.  Ties in (tile, depth) keep
// increasing Gaussian index in both formulations, so keys / point_list / ranges are bit-identical.
// S.BL.R is R (host-known) or, in resident mode, the capacity of the instance arrays with the true R in S.status[0]; the
// instance count produced by the depth-ordered scan (3 device words) goes to S.status or, without one, into the sort scratch.
int run_binning(const Scratch& S, const View& V, const BinningMode& mode, hipStream_t st) {
  const Geom& G = S.G; const BinningLayout& BL = S.BL; const GaussSortLayout& GS = S.GS;
  char* const bin = S.bin; uint2* const ranges = S.ranges();
  const int P = G.L.P, n_cap = BL.R;
  const uint32_t* const n_dev = S.status;
  uint32_t* const total_out = S.status ? S.status : (uint32_t*)(bin + GS.block_sums) + G.L.nblocks;
  const int bit = (int)getHigherMsb(V.tiles);
  // (1)
  char* gbin = bin + GS.base;
  const BinningLayout& GL = GS.inner;
  if (!mode.k1_keys) { PROF(K_DUPLICATE);
  const DepthSortInput in = depth_sort_input(bin, GS, mode.dbits, mode.digit_bits);
  make_depth_keys_kernel<<<G.L.nblocks, 256, 0, st>>>(P, G.bin(), mode.dcull, in.keys, in.vals, ranges, (int)V.tiles);
  }
  LAUNCH_TRY("make_depth_keys_kernel");
  const bool drop_culled = mode.k1_keys != nullptr;
  // The values are the Gaussian indices 0..P-1 (never materialised); tiles_touched must follow them into depth order for the
  // emitter's offsets.  It rides in the values' spare high bits, picked up by the FIRST pass (where entry i is Gaussian i: a
  // coalesced read) and taken apart by ordered_block_sums_kernel; a count that does not fit the spare bits saturates and is
  // fetched there.  (As a gather by the sorted values in the last pass it cost 44 instead of 21 us at 3 M Gaussians.)  With
  // fewer than six spare bits (P > 2^26) the last pass gathers it after all.
  int idx_bits = 1;
  while (idx_bits < 32 && ((uint64_t)1 << idx_bits) < (uint64_t)P) idx_bits++;
  int pack_shift = (32 - idx_bits >= 6 && !(g_flags & SEGS_RASTER_GATHER_TILES_TOUCHED)) ? idx_bits : 0;
  if (pack_shift && (g_flags & SEGS_RASTER_TEST_NARROW_PACK)) pack_shift = 30;
  SortOptions depth_sort;
  depth_sort.end_bit = mode.dbits; depth_sort.digit_bits = mode.digit_bits;
  depth_sort.dmin = mode.dmin; depth_sort.dbits = mode.dbits;
  depth_sort.drop_dead = drop_culled; depth_sort.iota_vals = true;
  depth_sort.aux_in = G.touched(); depth_sort.aux_final = pack_shift ? nullptr : G.offsets(); depth_sort.pack_shift = pack_shift;
  depth_sort.first_keys = mode.k1_keys;
  int rc = sort_pairs<uint32_t>(gbin, GL, P, depth_sort, st);
  if (rc) return rc;
  uint32_t* order = (uint32_t*)(gbin + GL.vals[0]);
  const uint32_t* ng_dev = drop_culled ? (const uint32_t*)(gbin + GL.n_live) : nullptr;
  // (2)
  uint32_t* sums2 = (uint32_t*)(bin + GS.block_sums);
  uint32_t* first_owner = (uint32_t*)(bin + GS.first_owner);
  const int prefix_wgs = (P + 256 * PREFIX_ROWS_PER_WG - 1) / (256 * PREFIX_ROWS_PER_WG);
  { PROF(K_SCAN);
  ordered_block_sums_kernel<<<prefix_wgs, 256, 0, st>>>(P, pack_shift ? G.touched() : G.offsets(), nullptr, sums2, G.offsets(), ng_dev, order, pack_shift);
  }
  LAUNCH_TRY("ordered_block_sums_kernel");
  // tile-id sort: two 8-bit passes in general; ONE 11-bit pass when the image has at most 2048 tiles and the instances fit
  // SORT_WIDE_MAX_TILES sort tiles (640x480: three launches and a pass over the instances less)
#ifdef SEGS_MEASURE   // measurement builds only (tools/)
  static const bool no_wide = getenv("SEGS_NO_WIDE_DIGIT") != nullptr;
#else
  constexpr bool no_wide = false;
#endif
  SortOptions tile_sort;
  tile_sort.end_bit = bit;
  tile_sort.digit_bits = (!no_wide && bit <= 11 && BL.nblocks <= SORT_WIDE_MAX_TILES) ? 11 : 8;
  tile_sort.n_dev = n_dev; tile_sort.drop_dead = mode.drop_dead;
  const int tpasses = (bit + tile_sort.digit_bits - 1) / tile_sort.digit_bits;
  const int side = sort_first_side(bit, tile_sort.digit_bits);
  { PROF(K_SCAN);
  ordered_offsets_kernel<<<prefix_wgs, 256, 0, st>>>(P, sums2, G.offsets(), total_out, ng_dev, first_owner,
                                                      (uint32_t)(n_cap / EMIT_SLOTS_PER_WG + 2));
  }
  LAUNCH_TRY("ordered_offsets_kernel");
  const bool unfused = (g_flags & SEGS_RASTER_UNFUSED_BINNING) != 0u;
  { PROF(K_DUPLICATE);
  duplicate_with_keys_kernel<<<(n_cap + EMIT_SLOTS_PER_WG - 1) / EMIT_SLOTS_PER_WG, 256, 0, st>>>(P, n_cap, G.rec(), order, G.offsets(),
                                                                    (uint32_t*)(bin + BL.keys[side]), (uint32_t*)(bin + BL.vals[side]), V.gx, n_dev,
                                                                    mode.drop_dead ? 1 : 0, ng_dev, first_owner);
  }
  LAUNCH_TRY("duplicate_with_keys_kernel");
  // (3)  With two passes the last one fills the range table and the status words itself (radix_scatter_kernel); a single pass
  // over depth-ordered input would need two atomics per instance for that and keeps the range kernel.
  const bool fused_ranges = !unfused && tpasses >= 2;
  if (fused_ranges) {
    tile_sort.ranges = ranges;
    tile_sort.status = n_dev ? total_out : nullptr;
    tile_sort.status_mirror = n_dev ? g_status_mirror : nullptr;
    tile_sort.keep_sorted_keys = n_dev == nullptr;   // resident mode: nothing reads the sorted tile ids after this
  }
  rc = sort_pairs<uint32_t>(bin, BL, n_cap, tile_sort, st);
  if (rc) return rc;
  if (!fused_ranges) { PROF(K_RANGES);
  identify_tile_ranges_kernel<<<(n_cap + 256 * RANGE_KEYS_PER_THREAD - 1) / (256 * RANGE_KEYS_PER_THREAD), 256, 0, st>>>(n_cap, (const uint32_t*)(bin + BL.keys[0]), ranges, n_dev,
                                                                   n_dev ? total_out : nullptr, n_dev ? g_status_mirror : nullptr,
                                                                   mode.drop_dead ? (const uint32_t*)(bin + BL.n_live) : nullptr);
  }
  LAUNCH_TRY("identify_tile_ranges_kernel");
  return SEGS_OK;
}

// K10: the plain tile forward, or its depth form when the caller asked for a depth or an alpha map (segs_*_depth entry points).
int launch_render_fwd(const Scratch& S, const View& V, const float* background, float* out_color, const segs_depth_outputs* dout,
                      hipStream_t st) {
  PROF(K_RENDER_FWD);
  if (dout && (dout->depth || dout->alpha))
    render_fwd_depth_kernel<<<V.tiles, 256, 0, st>>>(S.ranges(), S.point_list(), V.width, V.height, S.G.rec(), background, S.final_T(),
                                                     S.n_contrib(), out_color, dout->depth, dout->alpha);
  else
    render_fwd_kernel<<<V.tiles, 256, 0, st>>>(S.ranges(), S.point_list(), V.width, V.height, S.G.rec(), background, S.final_T(), S.n_contrib(),
                                               out_color);
  LAUNCH_TRY("render_fwd_kernel");
  return SEGS_OK;
}

// The tile backward.  Depth form: the gradients of the depth / alpha maps of segs_rasterize_forward*_depth; it is the VALU form
// only: SEGS_RASTER_MFMA_MOMENTS (an A/B switch of the plain kernel) does not apply to it.
int launch_render_bwd(const Scratch& S, const View& V, const float* background, const float* dL_dpix, const segs_depth_grads* dgrad,
                      uint8_t* written, hipStream_t st) {
  PROF(K_RENDER_BWD);
  const uint32_t grid = (V.tiles + 7) / 8 * 32;
  if (dgrad && (dgrad->dL_ddepth || dgrad->dL_dalpha)) {
    render_bwd_depth_kernel<<<grid, 64, 0, st>>>(S.ranges(), S.point_list(), V.width, V.height, S.G.rec(), background, S.final_T(),
                                                 S.n_contrib(), dL_dpix, S.G.gacc(), V.tiles, dgrad->dL_ddepth, dgrad->dL_dalpha, written);
    LAUNCH_TRY("render_bwd_depth_kernel");
    return SEGS_OK;
  }
  static const bool mfma_env = [] { const char* e = getenv("SEGS_RENDER_BWD_MFMA"); return e && e[0] == '1'; }();   // measurement A/B only
  ((mfma_env || (g_flags & SEGS_RASTER_MFMA_MOMENTS)) ? render_bwd_mfma_kernel : render_bwd_kernel)<<<grid, 64, 0, st>>>(
      S.ranges(), S.point_list(), V.width, V.height, S.G.rec(), background, S.final_T(), S.n_contrib(), dL_dpix, S.G.gacc(), V.tiles, written);
  LAUNCH_TRY("render_bwd_kernel");
  return SEGS_OK;
}

// Camera form of the backward (segs_*_camera entry points): checks the struct, zero-fills both 4x4 gradients when there is nothing
// to sum (*live = false: the caller then runs the form without it), and the fixed-order sum over the workgroups' partial rows.
int camera_grads_begin(const segs_camera_grads* cam, const float* shs, bool empty, hipStream_t st, bool* live) {
  *live = false;
  if (!cam) return SEGS_OK;
  if (!cam->dL_dviewmatrix || !cam->dL_dprojmatrix || !cam->temp) return fail(SEGS_ERR_INVALID_ARGUMENT, "segs_camera_grads: null field");
  if (shs) return fail(SEGS_ERR_INVALID_ARGUMENT, "camera gradients need colors_precomp: the SH colours depend on campos, which they do not cover");
  if (empty) {
    HIP_TRY(hipMemsetAsync(cam->dL_dviewmatrix, 0, 16 * sizeof(float), st));
    HIP_TRY(hipMemsetAsync(cam->dL_dprojmatrix, 0, 16 * sizeof(float), st));
    return SEGS_OK;
  }
  *live = true;
  return SEGS_OK;
}
float* camera_partials(const segs_camera_grads* cam) { return (float*)align_ptr(cam->temp); }
int camera_grads_finish(const segs_camera_grads* cam, int nblocks, hipStream_t st) {
  camera_grad_reduce_kernel<<<1, 960, 0, st>>>(camera_partials(cam), nblocks, cam->dL_dviewmatrix, cam->dL_dprojmatrix);
  LAUNCH_TRY("camera_grad_reduce_kernel");
  return SEGS_OK;
}

int launch_preprocess_bwd(const Gaussians& g, const View& V, const int* radii, const GradOutputs& o, const PerGaussianBwd& m, hipStream_t st) {
  const bool depth = m.depth || m.dz_in;
  auto* const kernel = m.cam ? (depth ? preprocess_bwd_kernel<true, true> : preprocess_bwd_kernel<false, true>)
                             : (depth ? preprocess_bwd_kernel<true, false> : preprocess_bwd_kernel<false, false>);
  const int nblocks = (g.P + 255) / 256;
  if (m.packed) {   // the resident backward with the bytes (preprocess.hip)
    auto* const packed = m.cam ? (depth ? preprocess_bwd_packed_kernel<true, true> : preprocess_bwd_packed_kernel<false, true>)
                               : (depth ? preprocess_bwd_packed_kernel<true, false> : preprocess_bwd_packed_kernel<false, false>);
    packed<<<nblocks, 256, 0, st>>>(g.P, g.means3D, radii, g.kernel_scales(), g.rotations, g.scale_modifier, g.cov3D_precomp, V.viewmatrix,
                                    V.projmatrix, V.focal_x, V.focal_y, V.tan_fovx, V.tan_fovy, m.gacc, (float)V.width, (float)V.height,
                                    o.dL_dmean2D, o.dL_dconic, o.dL_dopacity, o.dL_dcolor, o.dL_dmean3D, o.dL_dcov3D, o.dL_dscale, o.dL_drot,
                                    m.cam ? camera_partials(m.cam) : nullptr, m.written);
    LAUNCH_TRY("preprocess_bwd_packed_kernel");
    return m.cam ? camera_grads_finish(m.cam, nblocks, st) : SEGS_OK;
  }
  kernel<<<nblocks, 256, 0, st>>>(g.P, g.means3D, radii, g.kernel_scales(), g.rotations, g.scale_modifier, g.cov3D_precomp, V.viewmatrix,
                                  V.projmatrix, V.focal_x, V.focal_y, V.tan_fovx, V.tan_fovy, m.gacc, (float)V.width, (float)V.height,
                                  o.dL_dmean2D, o.dL_dconic, o.dL_dopacity, o.dL_dcolor, o.dL_dmean3D, o.dL_dcov3D, o.dL_dscale, o.dL_drot,
                                  m.clean_gacc ? 1 : 0, m.dz_in, m.cam ? camera_partials(m.cam) : nullptr, m.written);
  LAUNCH_TRY("preprocess_bwd_kernel");
  return m.cam ? camera_grads_finish(m.cam, nblocks, st) : SEGS_OK;
}

// The synchronising forward: K1 -> scan -> one host sync for R -> binning -> K10.
int rasterize_forward(const Allocators& A, const Gaussians& g, const View& V, const float* background, float* out_color, int* radii,
                      const segs_depth_outputs* dout, hipStream_t st, int* num_rendered) {
  const int P = g.P;
  if (!A.geometry_alloc || !A.binning_alloc || !A.image_alloc) return fail(SEGS_ERR_INVALID_ARGUMENT, "null allocator callback");
  if (P < 0 || V.width <= 0 || V.height <= 0) return fail(SEGS_ERR_INVALID_ARGUMENT, "bad P / image size");
  if (P > MAX_GAUSSIANS) return fail(SEGS_ERR_INVALID_ARGUMENT, "P exceeds 2^28 Gaussians (sort values carry a 4-bit quadrant mask)");
  if (!background || !out_color || !V.viewmatrix || !V.projmatrix || !num_rendered) return fail(SEGS_ERR_INVALID_ARGUMENT, "null required pointer");
  if (P > 0 && (!g.means3D || !g.opacities)) return fail(SEGS_ERR_INVALID_ARGUMENT, "null means3D/opacities");
  if (P > 0)
    if (int rc = check_colour_and_shape(g, V)) return rc;
  if (int rc = check_tile_grid(V)) return rc;

  Scratch S{};
  char* geom_raw = A.geometry_alloc(A.geometry_ctx, geom_layout(P).total);
  S.IL = image_layout(V.width, V.height);
  char* img_raw = A.image_alloc(A.image_ctx, S.IL.total);
  if (!geom_raw || !img_raw) return fail(SEGS_ERR_ALLOC, "allocator callback returned null");
  S.G = geom_at(geom_raw, P);
  S.img = align_ptr(img_raw);
  const Geom& G = S.G;
  if (!radii) radii = G.radii_internal();

  int R = 0;
  uint32_t hdr[3] = {0u, 0u, 0u};  // num_rendered, max(~depth_bits), max(depth_bits)
  const bool tight = (g_flags & SEGS_RASTER_TIGHT_BINNING) != 0u;   // segs_raster.h: shorter lists, same image and gradients
  // Tight mode has no use for the per-Gaussian bin records (they feed make_depth_keys_kernel and the debug unpackers): K1 writes
  // the 32-bit depth keys of the resident forward instead -- into the bin records' place, the sort scratch does not exist before
  // R is known -- and the depth sort's first pass reads them there (16 B x P less to write, one launch and a 12 B x P pass less).
  bool fast_keys = tight;
  if (P > 0) {
    K1Targets k1;
    k1.extra_flags = tight ? PREPROCESS_TIGHT_RECT : 0u;
    if (fast_keys) { k1.depth_keys = (uint32_t*)G.bin(); k1.ranges = S.ranges(); }
    int rc = run_preprocess(G, g, V, radii, k1, st);
    if (rc) return rc;
    { PROF(K_SCAN);
    scan_block_sums_kernel<<<1, 1024, 0, st>>>(G.block_sums(), G.L.nblocks, G.block_sums() + (G.L.nblocks + 1), G.num_rendered());
    }
    LAUNCH_TRY("scan_block_sums_kernel");
    HIP_TRY(hipMemcpyAsync(hdr, G.num_rendered(), sizeof(hdr), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    R = (int)hdr[0];
    if (R < 0) return fail(SEGS_ERR_INVALID_ARGUMENT, "num_rendered overflows int32");
    if (fast_keys && R > 0 && (hdr[2] - DEPTH_KEY_MIN) >= ((1u << DEPTH_KEY_BITS) - 1u)) {
      // a binned depth beyond the 27-bit key range of the three 9-bit passes (13 107 m): redo K1 for the exact-range sort
      fast_keys = false;
      K1Targets exact;
      exact.extra_flags = PREPROCESS_TIGHT_RECT;
      rc = run_preprocess(G, g, V, radii, exact, st);
      if (rc) return rc;
    }
  }
  S.BL = binning_layout(R);
  S.GS = gauss_sort_layout(R, P);
  char* bin_raw = A.binning_alloc(A.binning_ctx, S.GS.total);
  if (!bin_raw) return fail(SEGS_ERR_ALLOC, "binning allocator returned null");
  S.bin = align_ptr(bin_raw);

  if (R == 0) {   // rasterizer_impl.cu:310; with instances run_binning zeroes the table itself
    PROF(K_MEMSET);
    HIP_TRY(hipMemsetAsync(S.ranges(), 0, (size_t)V.gx * V.gy * sizeof(uint2), st));
  }
  if (R > 0) {
    const BinningMode mode = fast_keys ? BinningMode::resident_keys((const uint32_t*)G.bin(), tight)
                                       : BinningMode::exact_range(hdr[1], hdr[2], tight);
    if (int rc = run_binning(S, V, mode, st)) return rc;
  }
  if (int rc = launch_render_fwd(S, V, background, out_color, dout, st)) return rc;
  *num_rendered = R;
  return SEGS_OK;
}

// The one validation of the resident forms, and their carve-up.  `others_present`: the caller's further required pointers are all there
// (one check with the buffers); `k1`: the Gaussians when K1 runs here, null when their producer ran it (segs_neural_forward_projected).
int open_resident(const ScratchBuffers& B, int P, const View& V, uint32_t* status, bool others_present, const Gaussians* k1, Scratch* S) {
  if (P <= 0 || B.capacity <= 0 || V.width <= 0 || V.height <= 0) return fail(SEGS_ERR_INVALID_ARGUMENT, "bad sizes");
  if (B.geom_rows < P) return fail(SEGS_ERR_INVALID_ARGUMENT, "geom_rows (rows the geometry buffer was sized for) must be >= P");
  if (B.geom_rows > MAX_GAUSSIANS) return fail(SEGS_ERR_INVALID_ARGUMENT, "P exceeds 2^28 Gaussians");
  if (!B.geom_buffer || !B.binning_buffer || !B.image_buffer || !status || !others_present) return fail(SEGS_ERR_INVALID_ARGUMENT, "null required pointer");
  if (k1)
    if (int rc = check_colour_and_shape(*k1, V)) return rc;
  if (int rc = check_tile_grid(V)) return rc;
  *S = carve(B, P, V, status);
  return SEGS_OK;
}

// Resident forward, with K1 (k1 non-null) or after the producer's K1: no host synchronisation, a fixed launch sequence.
int rasterize_forward_resident(const ScratchBuffers& B, int P, const Gaussians* k1, const View& V, const float* background, float* out_color,
                               int* radii, uint32_t* status, const segs_depth_outputs* dout, hipStream_t st) {
  Scratch S{};
  const bool others_present = background && out_color && (!k1 || (V.viewmatrix && V.projmatrix && k1->means3D && k1->opacities));
  if (int rc = open_resident(B, P, V, status, others_present, k1, &S)) return rc;
  const DepthSortInput keys = resident_depth_sort_input(S.bin, S.GS);
  if (k1) {   // K1 writes the depth keys and zeroes the range table itself (one launch less)
    K1Targets t;
    t.depth_keys = keys.keys; t.depth_vals = keys.vals; t.ranges = S.ranges();
    t.extra_flags = resident_k1_flags(); t.depth_overflow = status + 2;
    if (int rc = run_preprocess(S.G, *k1, V, radii ? radii : S.G.radii_internal(), t, st)) return rc;
  }
  // lists, ranges and n_contrib count live entries only (43 % of the instances are dead at 500 k Gaussians / 1080p) -- an
  // internal contract between this forward and its backward, like the reference's own scratch layout
  if (int rc = run_binning(S, V, BinningMode::resident_keys(keys.keys, drop_dead_instances()), st)) return rc;
  // status[3] (overflow) and the host mirror are written at the end of run_binning
  return launch_render_fwd(S, V, background, out_color, dout, st);
}

// SELF_CLEAN (resident entry points): the per-Gaussian accumulator rows are not cleared by a memset before the tile kernel;
// preprocess_bwd_kernel writes zeros back over every row it consumes, so a buffer that starts out zero-filled is clean
// again after every backward (one 32 MB fill and its launch less per iteration).  The same holds for the "row written" bytes
// (gs_layout.h) that only this form uses: the tile backward sets them, preprocess_bwd_kernel reads and clears only the rows
// that carry one.  Invariant: after any resident backward -- of a valid step, of one the device drops (instance capacity
// exceeded, depth key out of range: its tile kernels walk truncated lists, but still set a byte with every row they add into)
// or of one that is redone -- every accumulator row and every byte is zero again.  The synchronising form clears the caller's
// scratch with its memset per call and hands the kernels no bytes: it reads every binned row, as before.
int rasterize_backward(const Gaussians& g, const View& V, const ScratchBuffers& B, const BackwardInputs& in, const GradOutputs& o,
                       GaccCleaning cleaning, hipStream_t st) {
  const int P = g.P, R = B.capacity;
  const bool self_clean = cleaning == SELF_CLEAN;
  if (P < 0 || R < 0 || V.width <= 0 || V.height <= 0) return fail(SEGS_ERR_INVALID_ARGUMENT, "bad sizes");
  if (B.geom_rows < P) return fail(SEGS_ERR_INVALID_ARGUMENT, "geom_rows must be >= P");
  bool cam_live = false;   // without Gaussians or instances both matrices are zero-filled here, ahead of the early return
  if (int rc = camera_grads_begin(in.cam, g.shs, P == 0 || R == 0, st, &cam_live)) return rc;
  if (P == 0) return SEGS_OK;  // src/rasterize_points.cu:159
  if (g.shs && (!V.cam_pos || !o.dL_dsh || g.M <= 0)) return fail(SEGS_ERR_INVALID_ARGUMENT, "SH path needs campos, dL_dsh and M > 0");
  if (!B.geom_buffer || !B.binning_buffer || !B.image_buffer || !in.dL_dpix || !in.background || !g.means3D || !V.viewmatrix || !V.projmatrix)
    return fail(SEGS_ERR_INVALID_ARGUMENT, "null required pointer");
  // dL_dconic (the tile kernel's internal product) and dL_dcov3D (of use only with cov3D_precomp) may be null: not written
  if (!o.dL_dmean2D || !o.dL_dopacity || !o.dL_dcolor || !o.dL_dmean3D || (g.cov3D_precomp && !o.dL_dcov3D))
    return fail(SEGS_ERR_INVALID_ARGUMENT, "null gradient output");
  if (!g.cov3D_precomp && (!g.scales || !g.rotations || !o.dL_dscale || !o.dL_drot))
    return fail(SEGS_ERR_INVALID_ARGUMENT, "need scales+rotations (+ their gradient outputs) or cov3D_precomp");
  uint32_t* const no_status = nullptr;
  const Scratch S = carve(B, P, V, no_status);
  const Geom& G = S.G;
  const int* radii = in.radii ? in.radii : G.radii_internal();

  if (!self_clean) { PROF(K_MEMSET);
  HIP_TRY(hipMemsetAsync(G.gacc(), 0, (size_t)P * GACC_DWORDS * 4, st));
  }
  PerGaussianBwd m;
  m.gacc = G.gacc(); m.depth = in.dgrad && in.dgrad->dL_ddepth; m.clean_gacc = self_clean;
  if (cam_live) m.cam = in.cam;
  m.written = (self_clean && !(g_flags & SEGS_RASTER_NO_WRITTEN_BYTES)) ? G.written() : nullptr;
  m.packed = m.written && !(g_flags & SEGS_RASTER_UNPACKED_BACKWARD);
  if (R > 0)
    if (int rc = launch_render_bwd(S, V, in.background, in.dL_dpix, in.dgrad, m.written, st)) return rc;
  { PROF(K_PREPROCESS_BWD);   // the camera form's second kernel runs inside the same profile slot
  if (int rc = launch_preprocess_bwd(g, V, radii, o, m, st)) return rc;
  }
  if (g.shs) {   // SH colour branch (off the live SEGS-SLAM path): its own pass over the summed dL/dcolor
    sh_backward_kernel<<<G.L.nblocks, 256, 0, st>>>(P, g.means3D, radii, g.shs, g.D, g.M, V.cam_pos, G.clamped(), o.dL_dcolor, o.dL_dmean3D, o.dL_dsh);
    LAUNCH_TRY("sh_backward_kernel");
  }
  return SEGS_OK;
}

int visible_filter(const Gaussians& g, const View& V, int log_scale_stride, int* radii, hipStream_t st) {
  if (g.P < 0 || V.width <= 0 || V.height <= 0) return fail(SEGS_ERR_INVALID_ARGUMENT, "bad sizes");
  if (g.P == 0) return SEGS_OK;
  if (!g.means3D || !V.viewmatrix || !V.projmatrix || !radii) return fail(SEGS_ERR_INVALID_ARGUMENT, "null required pointer");
  if (!g.cov3D_precomp && (!g.scales || !g.rotations)) return fail(SEGS_ERR_INVALID_ARGUMENT, "need scales+rotations or cov3D_precomp");
  visible_filter_kernel<<<(g.P + 255) / 256, 256, 0, st>>>(g.P, g.means3D, g.kernel_scales(), g.scale_modifier, g.rotations, g.cov3D_precomp,
                                                           V.viewmatrix, V.projmatrix, V.width, V.height, V.tan_fovx, V.tan_fovy, V.focal_x,
                                                           V.focal_y, V.gx, V.gy, radii, log_scale_stride);
  LAUNCH_TRY("visible_filter_kernel");
  return SEGS_OK;
}

// segs_debug_preprocess_backward*: the per-Gaussian backward alone, dL_dmean2D / dL_dconic as inputs
int debug_preprocess_backward(const Gaussians& g, const View& V, const int* radii, const GradOutputs& o, const float* dL_dz,
                              const segs_camera_grads* cam, hipStream_t st) {
  bool cam_live = false;
  if (int rc = camera_grads_begin(cam, g.shs, g.P <= 0, st, &cam_live)) return rc;
  if (g.P <= 0) return SEGS_OK;
  if (!g.means3D || !radii || !V.viewmatrix || !V.projmatrix || !o.dL_dmean2D || !o.dL_dconic || !o.dL_dmean3D || !o.dL_dcov3D)
    return fail(SEGS_ERR_INVALID_ARGUMENT, "null pointer");
  PerGaussianBwd m;
  if (cam_live) { m.dz_in = dL_dz; m.cam = cam; }
  return launch_preprocess_bwd(g, V, radii, o, m, st);
}

}  // namespace

extern "C" {

const char* segs_last_error(void) { return g_err.c_str(); }

uint32_t* segs_raster_set_status_mirror(uint32_t* host_mapped_status) {
  uint32_t* old = g_status_mirror;
  g_status_mirror = host_mapped_status;
  return old;
}

uint32_t segs_raster_set_flags(uint32_t flags) {
  const uint32_t old = g_flags;
  g_flags = flags;
  return old;
}

size_t segs_geometry_bytes(int P) { return geom_layout(P < 0 ? 0 : P).total; }
size_t segs_image_bytes(int width, int height) { return image_layout(width, height).total; }

int segs_debug_geometry_layout(int P, size_t* offset_and_bytes, int regions) {
  if (P < 0 || !offset_and_bytes || regions != SEGS_GEOMETRY_REGIONS) return fail(SEGS_ERR_INVALID_ARGUMENT, "bad P / region count");
  const GeomLayout g = geom_layout(P);
  const size_t p = (size_t)P;
  const size_t v[SEGS_GEOMETRY_REGIONS][2] = {
      {g.rec, p * REC_DWORDS * 4}, {g.bin, p * sizeof(BinInfo)}, {g.offsets, p * 4}, {g.radii_internal, p * 4},
      {g.block_sums, (size_t)(g.nblocks + 1) * 4 * 3}, {g.clamped, p * 4}, {g.num_rendered, 64}, {g.gacc, p * GACC_DWORDS * 4},
      {g.touched, p * 4}, {g.written, p}};
  for (int i = 0; i < SEGS_GEOMETRY_REGIONS; i++) { offset_and_bytes[2 * i] = v[i][0]; offset_and_bytes[2 * i + 1] = v[i][1]; }
  return SEGS_OK;
}
size_t segs_binning_bytes(int num_rendered) { return binning_layout(num_rendered < 0 ? 0 : num_rendered).total; }

int segs_rasterize_forward(segs_alloc_fn geometry_alloc, void* geometry_ctx, segs_alloc_fn binning_alloc, void* binning_ctx,
                           segs_alloc_fn image_alloc, void* image_ctx, int P, int D, int M, const float* background,
                           int width, int height, const float* means3D, const float* shs, const float* colors_precomp,
                           const float* opacities, const float* scales, float scale_modifier, const float* rotations,
                           const float* cov3D_precomp, const float* viewmatrix, const float* projmatrix,
                           const float* cam_pos, float tan_fovx, float tan_fovy, int prefiltered, float* out_color,
                           int* radii, void* stream, int* num_rendered) {
  (void)prefiltered;
  return rasterize_forward(Allocators{geometry_alloc, geometry_ctx, binning_alloc, binning_ctx, image_alloc, image_ctx},
                           Gaussians{P, means3D, scales, scale_modifier, rotations, cov3D_precomp, D, M, shs, colors_precomp, opacities},
                           camera_view(width, height, viewmatrix, projmatrix, cam_pos, tan_fovx, tan_fovy), background, out_color, radii,
                           NO_DEPTH_OUTPUTS, (hipStream_t)stream, num_rendered);
}

int segs_rasterize_forward_depth(segs_alloc_fn geometry_alloc, void* geometry_ctx, segs_alloc_fn binning_alloc, void* binning_ctx,
                                 segs_alloc_fn image_alloc, void* image_ctx, int P, int D, int M, const float* background,
                                 int width, int height, const float* means3D, const float* shs, const float* colors_precomp,
                                 const float* opacities, const float* scales, float scale_modifier, const float* rotations,
                                 const float* cov3D_precomp, const float* viewmatrix, const float* projmatrix,
                                 const float* cam_pos, float tan_fovx, float tan_fovy, int prefiltered, float* out_color,
                                 int* radii, const segs_depth_outputs* depth_out, void* stream, int* num_rendered) {
  (void)prefiltered;
  return rasterize_forward(Allocators{geometry_alloc, geometry_ctx, binning_alloc, binning_ctx, image_alloc, image_ctx},
                           Gaussians{P, means3D, scales, scale_modifier, rotations, cov3D_precomp, D, M, shs, colors_precomp, opacities},
                           camera_view(width, height, viewmatrix, projmatrix, cam_pos, tan_fovx, tan_fovy), background, out_color, radii,
                           depth_out, (hipStream_t)stream, num_rendered);
}

int segs_rasterize_backward(int P, int D, int M, int R, const float* background, int width, int height,
                            const float* means3D, const float* shs, const float* colors_precomp, const float* scales,
                            float scale_modifier, const float* rotations, const float* cov3D_precomp,
                            const float* viewmatrix, const float* projmatrix, const float* campos, float tan_fovx,
                            float tan_fovy, const int* radii, char* geom_buffer, char* binning_buffer, char* image_buffer,
                            const float* dL_dpix, float* dL_dmean2D, float* dL_dconic, float* dL_dopacity, float* dL_dcolor,
                            float* dL_dmean3D, float* dL_dcov3D, float* dL_dsh, float* dL_dscale, float* dL_drot, void* stream) {
  (void)colors_precomp;
  return rasterize_backward(Gaussians{P, means3D, scales, scale_modifier, rotations, cov3D_precomp, D, M, shs},
                            camera_view(width, height, viewmatrix, projmatrix, campos, tan_fovx, tan_fovy),
                            ScratchBuffers{geom_buffer, binning_buffer, image_buffer, R, P},
                            BackwardInputs{background, radii, dL_dpix, NO_DEPTH_GRADS, NO_CAMERA_GRADS},
                            GradOutputs{dL_dmean2D, dL_dconic, dL_dmean3D, dL_dcov3D, dL_dscale, dL_drot, dL_dopacity, dL_dcolor, dL_dsh},
                            MEMSET_PER_CALL, (hipStream_t)stream);
}

int segs_rasterize_backward_depth(int P, int D, int M, int R, const float* background, int width, int height,
                                  const float* means3D, const float* shs, const float* colors_precomp, const float* scales,
                                  float scale_modifier, const float* rotations, const float* cov3D_precomp,
                                  const float* viewmatrix, const float* projmatrix, const float* campos, float tan_fovx,
                                  float tan_fovy, const int* radii, char* geom_buffer, char* binning_buffer, char* image_buffer,
                                  const float* dL_dpix, float* dL_dmean2D, float* dL_dconic, float* dL_dopacity, float* dL_dcolor,
                                  float* dL_dmean3D, float* dL_dcov3D, float* dL_dsh, float* dL_dscale, float* dL_drot,
                                  const segs_depth_grads* depth_grads, void* stream) {
  (void)colors_precomp;
  return rasterize_backward(Gaussians{P, means3D, scales, scale_modifier, rotations, cov3D_precomp, D, M, shs},
                            camera_view(width, height, viewmatrix, projmatrix, campos, tan_fovx, tan_fovy),
                            ScratchBuffers{geom_buffer, binning_buffer, image_buffer, R, P},
                            BackwardInputs{background, radii, dL_dpix, depth_grads, NO_CAMERA_GRADS},
                            GradOutputs{dL_dmean2D, dL_dconic, dL_dmean3D, dL_dcov3D, dL_dscale, dL_drot, dL_dopacity, dL_dcolor, dL_dsh},
                            MEMSET_PER_CALL, (hipStream_t)stream);
}

size_t segs_camera_grad_temp_bytes(int rows) { return align_up((size_t)((rows < 0 ? 0 : rows) + 255) / 256 * CAM_SUMS * sizeof(float)) + ALIGN; }

int segs_rasterize_backward_camera(int P, int D, int M, int R, const float* background, int width, int height,
                                   const float* means3D, const float* shs, const float* colors_precomp, const float* scales,
                                   float scale_modifier, const float* rotations, const float* cov3D_precomp,
                                   const float* viewmatrix, const float* projmatrix, const float* campos, float tan_fovx,
                                   float tan_fovy, const int* radii, char* geom_buffer, char* binning_buffer, char* image_buffer,
                                   const float* dL_dpix, float* dL_dmean2D, float* dL_dconic, float* dL_dopacity, float* dL_dcolor,
                                   float* dL_dmean3D, float* dL_dcov3D, float* dL_dsh, float* dL_dscale, float* dL_drot,
                                   const segs_depth_grads* depth_grads, const segs_camera_grads* camera_grads, void* stream) {
  (void)colors_precomp;
  return rasterize_backward(Gaussians{P, means3D, scales, scale_modifier, rotations, cov3D_precomp, D, M, shs},
                            camera_view(width, height, viewmatrix, projmatrix, campos, tan_fovx, tan_fovy),
                            ScratchBuffers{geom_buffer, binning_buffer, image_buffer, R, P},
                            BackwardInputs{background, radii, dL_dpix, depth_grads, camera_grads},
                            GradOutputs{dL_dmean2D, dL_dconic, dL_dmean3D, dL_dcov3D, dL_dscale, dL_drot, dL_dopacity, dL_dcolor, dL_dsh},
                            MEMSET_PER_CALL, (hipStream_t)stream);
}

int segs_visible_filter(int P, int M, int width, int height, const float* means3D, const float* scales,
                        float scale_modifier, const float* rotations, const float* cov3D_precomp, const float* viewmatrix,
                        const float* projmatrix, float tan_fovx, float tan_fovy, int prefiltered, int* radii, void* stream) {
  (void)M; (void)prefiltered;
  return visible_filter(Gaussians{P, means3D, scales, scale_modifier, rotations, cov3D_precomp},
                        camera_view(width, height, viewmatrix, projmatrix, NO_CAM_POS, tan_fovx, tan_fovy), 0, radii, (hipStream_t)stream);
}

int segs_visible_filter_log_scales(int P, int width, int height, const float* means3D, const float* scaling_log, int stride,
                                   const float* rotations, const float* viewmatrix, const float* projmatrix, float tan_fovx,
                                   float tan_fovy, int* radii, void* stream) {
  if (stride < 3 || !scaling_log || !rotations) return fail(SEGS_ERR_INVALID_ARGUMENT, "need log-scales (stride >= 3) and rotations");
  return visible_filter(Gaussians{P, means3D, scaling_log, 1.0f, rotations},
                        camera_view(width, height, viewmatrix, projmatrix, NO_CAM_POS, tan_fovx, tan_fovy), stride, radii, (hipStream_t)stream);
}

int segs_mark_visible(int P, const float* means3D, const float* viewmatrix, const float* projmatrix, uint8_t* present, void* stream) {
  (void)projmatrix;
  hipStream_t st = (hipStream_t)stream;
  if (P < 0) return fail(SEGS_ERR_INVALID_ARGUMENT, "bad P");
  if (P == 0) return SEGS_OK;
  if (!means3D || !viewmatrix || !present) return fail(SEGS_ERR_INVALID_ARGUMENT, "null required pointer");
  mark_visible_kernel<<<(P + 255) / 256, 256, 0, st>>>(P, means3D, viewmatrix, present);
  LAUNCH_TRY("mark_visible_kernel");
  return SEGS_OK;
}

int segs_debug_unpack_geometry(const char* geom_buffer, int P, const int* radii, float* means2D, float* conic_opacity,
                               float* depths, uint32_t* tiles_touched, uint32_t* point_offsets, float* rgb, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  if (P <= 0) return SEGS_OK;
  if (!geom_buffer || !means2D || !conic_opacity || !depths || !tiles_touched) return fail(SEGS_ERR_INVALID_ARGUMENT, "null pointer");
  Geom G = geom_at(const_cast<char*>(geom_buffer), P);
  if (!radii) radii = G.radii_internal();
  unpack_geometry_kernel<<<(P + 255) / 256, 256, 0, st>>>(P, G.rec(), G.bin(), radii, means2D, conic_opacity, depths, tiles_touched, rgb);
  LAUNCH_TRY("unpack_geometry_kernel");
  if (point_offsets) {
    point_offsets_kernel<<<1, 1024, 0, st>>>(P, G.bin(), point_offsets);
    LAUNCH_TRY("point_offsets_kernel");
  }
  return SEGS_OK;
}

int segs_debug_unpack_binning(const char* binning_buffer, const char* geom_buffer, int P, int R, int width, int height,
                              uint64_t* keys_sorted, uint32_t* point_list, void* stream) {
  (void)width; (void)height;
  hipStream_t st = (hipStream_t)stream;
  if (R <= 0) return SEGS_OK;
  if (!binning_buffer || (keys_sorted && (!geom_buffer || P <= 0))) return fail(SEGS_ERR_INVALID_ARGUMENT, "null pointer");
  const BinningLayout BL = binning_layout(R);
  const char* bin = align_ptr(binning_buffer);
  if (keys_sorted) {   // the pipeline sorts 32-bit tile ids; the reference's 64-bit keys are rebuilt for parity checks
    const Geom G = geom_at(const_cast<char*>(geom_buffer), P);
    rebuild_keys_kernel<<<(R + 255) / 256, 256, 0, st>>>(R, (const uint32_t*)(bin + BL.keys[0]), (const uint32_t*)(bin + BL.vals[0]),
                                                        G.bin(), keys_sorted);
    LAUNCH_TRY("rebuild_keys_kernel");
  }
  if (point_list) {
    strip_mask_kernel<<<(R + 255) / 256, 256, 0, st>>>(R, (const uint32_t*)(bin + BL.vals[0]), point_list);
    LAUNCH_TRY("strip_mask_kernel");
  }
  return SEGS_OK;
}

int segs_debug_instance_values(const char* binning_buffer, int R, uint32_t* values, void* stream) {
  if (R <= 0) return SEGS_OK;
  if (!binning_buffer || !values) return fail(SEGS_ERR_INVALID_ARGUMENT, "null pointer");
  const BinningLayout BL = binning_layout(R);
  HIP_TRY(hipMemcpyAsync(values, align_ptr(binning_buffer) + BL.vals[0], (size_t)R * 4, hipMemcpyDeviceToDevice, (hipStream_t)stream));
  return SEGS_OK;
}

int segs_debug_unpack_image(const char* image_buffer, int width, int height, uint32_t* ranges, float* final_T,
                            uint32_t* n_contrib, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  if (!image_buffer) return fail(SEGS_ERR_INVALID_ARGUMENT, "null pointer");
  const ImageLayout IL = image_layout(width, height);
  const char* img = align_ptr(image_buffer);
  const size_t tiles = image_view(width, height).tiles;
  if (ranges) {
    HIP_TRY(hipMemcpyAsync(ranges, img + IL.ranges, tiles * 8, hipMemcpyDeviceToDevice, st));
    normalize_ranges_kernel<<<(int)((tiles + 255) / 256), 256, 0, st>>>((int)tiles, (uint2*)ranges);   // empty tiles: {0, 0} as in the reference
    LAUNCH_TRY("normalize_ranges_kernel");
  }
  if (final_T) HIP_TRY(hipMemcpyAsync(final_T, img + IL.final_T, (size_t)width * height * 4, hipMemcpyDeviceToDevice, st));
  if (n_contrib) HIP_TRY(hipMemcpyAsync(n_contrib, img + IL.n_contrib, (size_t)width * height * 4, hipMemcpyDeviceToDevice, st));
  return SEGS_OK;
}

int segs_debug_preprocess_backward(int P, int width, int height, const float* means3D, const int* radii, const float* scales,
                                   float scale_modifier, const float* rotations, const float* cov3D_precomp,
                                   const float* viewmatrix, const float* projmatrix, float tan_fovx, float tan_fovy,
                                   const float* dL_dmean2D, const float* dL_dconic, float* dL_dmean3D, float* dL_dcov3D,
                                   float* dL_dscale, float* dL_drot, void* stream) {
  return debug_preprocess_backward(Gaussians{P, means3D, scales, scale_modifier, rotations, cov3D_precomp},
                                   camera_view(width, height, viewmatrix, projmatrix, NO_CAM_POS, tan_fovx, tan_fovy), radii,
                                   GradOutputs{const_cast<float*>(dL_dmean2D), const_cast<float*>(dL_dconic), dL_dmean3D, dL_dcov3D, dL_dscale, dL_drot}, NO_DL_DZ,
                                   NO_CAMERA_GRADS, (hipStream_t)stream);
}

int segs_debug_preprocess_backward_camera(int P, int width, int height, const float* means3D, const int* radii, const float* scales,
                                          float scale_modifier, const float* rotations, const float* cov3D_precomp,
                                          const float* viewmatrix, const float* projmatrix, float tan_fovx, float tan_fovy,
                                          const float* dL_dmean2D, const float* dL_dconic, float* dL_dmean3D, float* dL_dcov3D,
                                          float* dL_dscale, float* dL_drot, const float* dL_dz, const segs_camera_grads* camera_grads,
                                          void* stream) {
  return debug_preprocess_backward(Gaussians{P, means3D, scales, scale_modifier, rotations, cov3D_precomp},
                                   camera_view(width, height, viewmatrix, projmatrix, NO_CAM_POS, tan_fovx, tan_fovy), radii,
                                   GradOutputs{const_cast<float*>(dL_dmean2D), const_cast<float*>(dL_dconic), dL_dmean3D, dL_dcov3D, dL_dscale, dL_drot}, dL_dz, camera_grads,
                                   (hipStream_t)stream);
}

int segs_sort_pairs(const uint64_t* keys_in, const uint32_t* vals_in, uint64_t* keys_out, uint32_t* vals_out, int n,
                    int end_bit, char* temp, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  if (n < 0 || end_bit <= 0 || end_bit > 64) return fail(SEGS_ERR_INVALID_ARGUMENT, "bad n / end_bit");
  if (n == 0) return SEGS_OK;
  if (!keys_in || !vals_in || !keys_out || !vals_out || !temp) return fail(SEGS_ERR_INVALID_ARGUMENT, "null pointer");
  const BinningLayout BL = binning_layout(n);
  char* bin = align_ptr(temp);
  SortOptions sort;
  sort.end_bit = end_bit; sort.dbits = 32;
  const int side = sort_first_side(end_bit, sort.digit_bits);
  HIP_TRY(hipMemcpyAsync(bin + BL.keys[side], keys_in, (size_t)n * 8, hipMemcpyDeviceToDevice, st));
  HIP_TRY(hipMemcpyAsync(bin + BL.vals[side], vals_in, (size_t)n * 4, hipMemcpyDeviceToDevice, st));
  int rc = sort_pairs<uint64_t>(bin, BL, n, sort, st);
  if (rc) return rc;
  HIP_TRY(hipMemcpyAsync(keys_out, bin + BL.keys[0], (size_t)n * 8, hipMemcpyDeviceToDevice, st));
  HIP_TRY(hipMemcpyAsync(vals_out, bin + BL.vals[0], (size_t)n * 4, hipMemcpyDeviceToDevice, st));
  return SEGS_OK;
}

int segs_project2_image(int P, int D, int M, int width, int height, const float* means3D, const float* shs,
                        const float* colors_precomp, const float* opacities, const float* scales, float scale_modifier,
                        const float* rotations, const float* cov3D_precomp, const float* viewmatrix, const float* projmatrix,
                        const float* cam_pos, float tan_fovx, float tan_fovy, int prefiltered, float* out_color,
                        float* points_image, int* radii, void* stream) {
  (void)prefiltered;
  hipStream_t st = (hipStream_t)stream;
  if (P < 0 || width <= 0 || height <= 0) return fail(SEGS_ERR_INVALID_ARGUMENT, "bad sizes");
  if (P == 0) return SEGS_OK;
  if (!colors_precomp && (!shs || !cam_pos || M <= 0)) return fail(SEGS_ERR_INVALID_ARGUMENT, "need colors_precomp or shs + cam_pos");
  if (!means3D || !opacities || !viewmatrix || !projmatrix || !out_color || !points_image || !radii)
    return fail(SEGS_ERR_INVALID_ARGUMENT, "null required pointer");
  // scratch: this entry has no allocator callbacks worth keeping (the reference allocates full geometry and
  // image states it then discards); use a stream-ordered temporary.
  const GeomLayout GL = geom_layout(P);
  char* raw = nullptr;
  HIP_TRY(hipMallocAsync((void**)&raw, GL.total + (size_t)P * 4 * 8, st));
  Geom G = geom_at(raw, P);
  float* tmp = (float*)(align_ptr(raw) + GL.total - ALIGN);  // conic(4P) + depth(P) + tiles(P)
  int rc = run_preprocess(G, Gaussians{P, means3D, scales, scale_modifier, rotations, cov3D_precomp, D, M, shs, colors_precomp, opacities},
                          camera_view(width, height, viewmatrix, projmatrix, cam_pos, tan_fovx, tan_fovy), radii, K1Targets(), st);
  if (rc == SEGS_OK) {
    unpack_geometry_kernel<<<(P + 255) / 256, 256, 0, st>>>(P, G.rec(), G.bin(), radii, points_image, tmp, tmp + (size_t)4 * P,
                                                            (uint32_t*)(tmp + (size_t)5 * P), out_color);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) rc = hip_fail(e, "unpack_geometry_kernel");
  }
  hipError_t fe = hipFreeAsync(raw, st);
  if (rc == SEGS_OK && fe != hipSuccess) return hip_fail(fe, "hipFreeAsync");
  return rc;
}


// ---- Resident (steady-state) variants: no host synchronisation, fixed launch sequence (hipGraph-capturable). ----
size_t segs_resident_binning_bytes(int P, int capacity) { return gauss_sort_layout(capacity < 0 ? 0 : capacity, P < 0 ? 0 : P).total; }

int segs_rasterize_forward_resident(char* geom_buffer, char* binning_buffer, char* image_buffer, int capacity, int geom_rows, int P, int D, int M,
                                    const float* background, int width, int height, const float* means3D, const float* shs,
                                    const float* colors_precomp, const float* opacities, const float* scales, float scale_modifier,
                                    const float* rotations, const float* cov3D_precomp, const float* viewmatrix,
                                    const float* projmatrix, const float* cam_pos, float tan_fovx, float tan_fovy, float* out_color,
                                    int* radii, uint32_t* status, void* stream) {
  const Gaussians g{P, means3D, scales, scale_modifier, rotations, cov3D_precomp, D, M, shs, colors_precomp, opacities};
  return rasterize_forward_resident(ScratchBuffers{geom_buffer, binning_buffer, image_buffer, capacity, geom_rows}, P, &g,
                                    camera_view(width, height, viewmatrix, projmatrix, cam_pos, tan_fovx, tan_fovy), background, out_color,
                                    radii, status, NO_DEPTH_OUTPUTS, (hipStream_t)stream);
}

int segs_rasterize_forward_resident_depth(char* geom_buffer, char* binning_buffer, char* image_buffer, int capacity, int geom_rows, int P,
                                          int D, int M, const float* background, int width, int height, const float* means3D,
                                          const float* shs, const float* colors_precomp, const float* opacities, const float* scales,
                                          float scale_modifier, const float* rotations, const float* cov3D_precomp,
                                          const float* viewmatrix, const float* projmatrix, const float* cam_pos, float tan_fovx,
                                          float tan_fovy, float* out_color, int* radii, uint32_t* status,
                                          const segs_depth_outputs* depth_out, void* stream) {
  const Gaussians g{P, means3D, scales, scale_modifier, rotations, cov3D_precomp, D, M, shs, colors_precomp, opacities};
  return rasterize_forward_resident(ScratchBuffers{geom_buffer, binning_buffer, image_buffer, capacity, geom_rows}, P, &g,
                                    camera_view(width, height, viewmatrix, projmatrix, cam_pos, tan_fovx, tan_fovy), background, out_color,
                                    radii, status, depth_out, (hipStream_t)stream);
}

// ---- K1 done by the producer of the Gaussians (segs_neural_forward_projected): where its outputs go, and the forward without K1.
int segs_resident_projection_targets(char* geom_buffer, char* binning_buffer, char* image_buffer, int capacity, int geom_rows, int P,
                                     int width, int height, int* radii, uint32_t* status, segs_projection_targets* out) {
  if (!out) return fail(SEGS_ERR_INVALID_ARGUMENT, "bad sizes");
  const View V = image_view(width, height);
  Scratch S{};
  const bool nothing_else_required = true;
  if (int rc = open_resident(ScratchBuffers{geom_buffer, binning_buffer, image_buffer, capacity, geom_rows}, P, V, status, nothing_else_required,
                             K1_RAN_AT_PRODUCER, &S))
    return rc;
  out->records = S.G.rec();
  out->radii = radii ? radii : S.G.radii_internal();
  out->tiles_touched = S.G.touched();
  out->depth_keys = resident_depth_sort_input(S.bin, S.GS).keys;
  out->tile_ranges = (uint32_t*)S.ranges();
  out->depth_overflow = status + 2;
  out->num_tiles = (int)V.tiles;
  out->flags = resident_k1_flags();
  return SEGS_OK;
}

int segs_rasterize_forward_resident_projected(char* geom_buffer, char* binning_buffer, char* image_buffer, int capacity, int geom_rows, int P,
                                              const float* background, int width, int height, float* out_color, uint32_t* status,
                                              void* stream) {
  return rasterize_forward_resident(ScratchBuffers{geom_buffer, binning_buffer, image_buffer, capacity, geom_rows}, P, K1_RAN_AT_PRODUCER,
                                    image_view(width, height), background, out_color, NO_RADII, status, NO_DEPTH_OUTPUTS, (hipStream_t)stream);
}

int segs_rasterize_forward_resident_projected_depth(char* geom_buffer, char* binning_buffer, char* image_buffer, int capacity,
                                                    int geom_rows, int P, const float* background, int width, int height,
                                                    float* out_color, uint32_t* status, const segs_depth_outputs* depth_out,
                                                    void* stream) {
  return rasterize_forward_resident(ScratchBuffers{geom_buffer, binning_buffer, image_buffer, capacity, geom_rows}, P, K1_RAN_AT_PRODUCER,
                                    image_view(width, height), background, out_color, NO_RADII, status, depth_out, (hipStream_t)stream);
}

// The resident backwards are the synchronising ones except that the scratch layout is keyed by the capacity, not by R, and that
// the accumulator rows of geom_buffer are kept clean by the backward itself (the buffer must start out zero-filled).
int segs_rasterize_backward_resident(char* geom_buffer, char* binning_buffer, char* image_buffer, int capacity, int geom_rows, int P, int D, int M,
                                     const float* background, int width, int height, const float* means3D, const float* shs,
                                     const float* scales, float scale_modifier, const float* rotations, const float* cov3D_precomp,
                                     const float* viewmatrix, const float* projmatrix, const float* campos, float tan_fovx,
                                     float tan_fovy, const int* radii, const float* dL_dpix, float* dL_dmean2D, float* dL_dconic,
                                     float* dL_dopacity, float* dL_dcolor, float* dL_dmean3D, float* dL_dcov3D, float* dL_dsh,
                                     float* dL_dscale, float* dL_drot, void* stream) {
  return rasterize_backward(Gaussians{P, means3D, scales, scale_modifier, rotations, cov3D_precomp, D, M, shs},
                            camera_view(width, height, viewmatrix, projmatrix, campos, tan_fovx, tan_fovy),
                            ScratchBuffers{geom_buffer, binning_buffer, image_buffer, capacity, geom_rows},
                            BackwardInputs{background, radii, dL_dpix, NO_DEPTH_GRADS, NO_CAMERA_GRADS},
                            GradOutputs{dL_dmean2D, dL_dconic, dL_dmean3D, dL_dcov3D, dL_dscale, dL_drot, dL_dopacity, dL_dcolor, dL_dsh},
                            SELF_CLEAN, (hipStream_t)stream);
}

int segs_rasterize_backward_resident_depth(char* geom_buffer, char* binning_buffer, char* image_buffer, int capacity, int geom_rows, int P,
                                           int D, int M, const float* background, int width, int height, const float* means3D,
                                           const float* shs, const float* scales, float scale_modifier, const float* rotations,
                                           const float* cov3D_precomp, const float* viewmatrix, const float* projmatrix,
                                           const float* campos, float tan_fovx, float tan_fovy, const int* radii, const float* dL_dpix,
                                           float* dL_dmean2D, float* dL_dconic, float* dL_dopacity, float* dL_dcolor, float* dL_dmean3D,
                                           float* dL_dcov3D, float* dL_dsh, float* dL_dscale, float* dL_drot,
                                           const segs_depth_grads* depth_grads, void* stream) {
  return rasterize_backward(Gaussians{P, means3D, scales, scale_modifier, rotations, cov3D_precomp, D, M, shs},
                            camera_view(width, height, viewmatrix, projmatrix, campos, tan_fovx, tan_fovy),
                            ScratchBuffers{geom_buffer, binning_buffer, image_buffer, capacity, geom_rows},
                            BackwardInputs{background, radii, dL_dpix, depth_grads, NO_CAMERA_GRADS},
                            GradOutputs{dL_dmean2D, dL_dconic, dL_dmean3D, dL_dcov3D, dL_dscale, dL_drot, dL_dopacity, dL_dcolor, dL_dsh},
                            SELF_CLEAN, (hipStream_t)stream);
}

int segs_rasterize_backward_resident_camera(char* geom_buffer, char* binning_buffer, char* image_buffer, int capacity, int geom_rows, int P,
                                            int D, int M, const float* background, int width, int height, const float* means3D,
                                            const float* shs, const float* scales, float scale_modifier, const float* rotations,
                                            const float* cov3D_precomp, const float* viewmatrix, const float* projmatrix,
                                            const float* campos, float tan_fovx, float tan_fovy, const int* radii, const float* dL_dpix,
                                            float* dL_dmean2D, float* dL_dconic, float* dL_dopacity, float* dL_dcolor, float* dL_dmean3D,
                                            float* dL_dcov3D, float* dL_dsh, float* dL_dscale, float* dL_drot,
                                            const segs_depth_grads* depth_grads, const segs_camera_grads* camera_grads, void* stream) {
  return rasterize_backward(Gaussians{P, means3D, scales, scale_modifier, rotations, cov3D_precomp, D, M, shs},
                            camera_view(width, height, viewmatrix, projmatrix, campos, tan_fovx, tan_fovy),
                            ScratchBuffers{geom_buffer, binning_buffer, image_buffer, capacity, geom_rows},
                            BackwardInputs{background, radii, dL_dpix, depth_grads, camera_grads},
                            GradOutputs{dL_dmean2D, dL_dconic, dL_dmean3D, dL_dcov3D, dL_dscale, dL_drot, dL_dopacity, dL_dcolor, dL_dsh},
                            SELF_CLEAN, (hipStream_t)stream);
}

// ---- measurement support (bench.py): HIP events recorded on the launch stream around selected kernels.
int segs_profile_begin(unsigned kernel_mask) {
  g_prof.mask = kernel_mask; g_prof.used = 0; g_prof.spans.clear();
  for (int i = 0; i < K_COUNT; i++) { g_prof.total_ms[i] = 0; g_prof.count[i] = 0; }
  return SEGS_OK;
}
int segs_profile_end(void) {
  g_prof.mask = 0;
  for (const auto& sp : g_prof.spans) {
    HIP_TRY(hipEventSynchronize(g_prof.pool[sp.e1]));
    float ms = 0.f;
    HIP_TRY(hipEventElapsedTime(&ms, g_prof.pool[sp.e0], g_prof.pool[sp.e1]));
    g_prof.total_ms[sp.id] += ms; g_prof.count[sp.id]++;
  }
  g_prof.spans.clear(); g_prof.used = 0;
  return SEGS_OK;
}
int segs_profile_kernel_count(void) { return K_COUNT; }
const char* segs_profile_kernel_name(int id) { return (id >= 0 && id < K_COUNT) ? kKernelNames[id] : ""; }
int segs_profile_query(int id, double* total_ms, long* launches) {
  if (id < 0 || id >= K_COUNT || !total_ms || !launches) return fail(SEGS_ERR_INVALID_ARGUMENT, "bad profile query");
  *total_ms = g_prof.total_ms[id]; *launches = g_prof.count[id];
  return SEGS_OK;
}

}  // extern "C"
