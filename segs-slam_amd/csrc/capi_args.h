// capi_args.h -- the argument structs of the host layer (capi.hip, which alone includes this file): plain aggregates that an
// entry point packs once, so that nothing in capi.hip forwards a long positional list, and the arithmetic that belongs to them.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include "../../include/segs_raster.h"
#include "gs_layout.h"
#include "kernels.h"

namespace segs {

struct Gaussians {   // shape first: the visible filters and the debug entry points stop after cov3D_precomp, the backwards after shs
  int P; const float *means3D, *scales; float scale_modifier; const float *rotations, *cov3D_precomp;
  int D, M; const float *shs, *colors_precomp, *opacities;
  const float* kernel_scales() const { return cov3D_precomp ? nullptr : scales; }   // a precomputed covariance replaces the scales
};

struct View {   // camera and image, with the tile grid and the focal lengths every kernel is handed
  int width, height; const float *viewmatrix, *projmatrix, *cam_pos; float tan_fovx, tan_fovy;
  uint32_t gx, gy, tiles; float focal_x, focal_y;
};
inline View image_view(int width, int height) {
  View v{};
  v.width = width; v.height = height;
  v.gx = (width + TILE_X - 1) / TILE_X; v.gy = (height + TILE_Y - 1) / TILE_Y; v.tiles = v.gx * v.gy;
  return v;
}
inline View camera_view(int width, int height, const float* viewmatrix, const float* projmatrix, const float* cam_pos, float tan_fovx, float tan_fovy) {
  View v = image_view(width, height);
  v.viewmatrix = viewmatrix; v.projmatrix = projmatrix; v.cam_pos = cam_pos; v.tan_fovx = tan_fovx; v.tan_fovy = tan_fovy;
  v.focal_y = height / (2.0f * tan_fovy);   // rasterizer_impl.cu:221-222; K1's outputs are bit-compared: keep the operand order
  v.focal_x = width / (2.0f * tan_fovx);
  return v;
}

// the debug entry points stop after dL_drot
struct GradOutputs { float *dL_dmean2D, *dL_dconic, *dL_dmean3D, *dL_dcov3D, *dL_dscale, *dL_drot, *dL_dopacity, *dL_dcolor, *dL_dsh; };
// The caller's three scratch buffers, sized for `capacity` instances (the synchronising backward: R) and `geom_rows` Gaussians.
struct ScratchBuffers { char *geom_buffer, *binning_buffer, *image_buffer; int capacity, geom_rows; };

// The ping-pong side a sort of `end_bit` key bits in `digit_bits`-bit passes reads first, so that its result lands in side 0.
inline int sort_first_side(int end_bit, int digit_bits) { return ((end_bit + digit_bits - 1) / digit_bits) & 1; }
struct SortOptions {
  int end_bit = 0;                   // key bits [0, end_bit) are sorted ...
  int digit_bits = 8;                // ... this many per pass: 8, 9 or 11 (64-bit keys: 8)
  uint32_t dmin = 0u; int dbits = 0; // depth keys: see radix_count_kernel
  const uint32_t* n_dev = nullptr;   // resident mode: the true count, on the device
  bool drop_dead = false;            // entries whose key is all ones take no count and no rank in the FIRST pass: the later passes --
                                     // and the caller, through *n_live -- work on the survivors only: a stable partition for free
  bool iota_vals = false;            // the values of the input are 0..n-1 and are not read (nor need they have been written)
  const uint32_t* aux_in = nullptr;  // aux_in / aux_final (32-bit keys only): the LAST pass also writes aux_final[position] =
  uint32_t* aux_final = nullptr;     // aux_in[value] (a gather by the sorted values, fused into the scatter)
  int pack_shift = 0;                // > 0 (with iota_vals, aux_in, no aux_final): the FIRST pass packs min(aux_in[i], tmax) into the
                                     // value's bits from pack_shift up; the caller takes the sorted values apart
  const void* first_keys = nullptr;  // the FIRST pass reads its keys here instead of from its ping-pong side
  uint2* ranges = nullptr;           // fused by run_binning: the LAST pass fills the range table (K9) -- only valid with >= 2 passes or a
                                     // single pass whose digit is the whole key (see radix_scatter_kernel)
  uint32_t* status = nullptr;        // resident mode, with `ranges`: the last pass also writes the status words ...
  uint32_t* status_mirror = nullptr; // ... and their host-mapped mirror
  bool keep_sorted_keys = true;      // false: the last pass does not store the sorted keys (nobody reads them)
};

struct Geom {
  GeomLayout L;
  char* base;
  float* rec() const { return (float*)(base + L.rec); }
  BinInfo* bin() const { return (BinInfo*)(base + L.bin); }
  uint32_t* offsets() const { return (uint32_t*)(base + L.offsets); }
  int* radii_internal() const { return (int*)(base + L.radii_internal); }
  uint32_t* block_sums() const { return (uint32_t*)(base + L.block_sums); }
  uint32_t* num_rendered() const { return (uint32_t*)(base + L.num_rendered); }
  uint32_t* clamped() const { return (uint32_t*)(base + L.clamped); }
  float* gacc() const { return (float*)(base + L.gacc); }
  uint32_t* touched() const { return (uint32_t*)(base + L.touched); }
  uint8_t* written() const { return (uint8_t*)(base + L.written); }
};
inline Geom geom_at(char* p, int P) { return Geom{geom_layout(P), align_ptr(p)}; }
// Resident buffers are carved up for the `rows` they were ALLOCATED (and zero-filled) for, so that the self-cleaned
// accumulator rows stay where they are when the caller rasterizes fewer rows (a map that shrinks inside pre-sized
// buffers); only the launch extent follows P.
inline Geom geom_at(char* p, int P, int rows) {
  Geom g{geom_layout(rows), align_ptr(p)};
  g.L.P = P;
  g.L.nblocks = (P + 255) / 256;
  return g;
}

// The carve-up of the three scratch buffers that one call works on.
struct Scratch {
  Geom G;
  char *img, *bin;
  ImageLayout IL;
  BinningLayout BL;       // instance-level state (what backward re-parses)
  GaussSortLayout GS;     // + Gaussian-level depth sort scratch behind it
  uint32_t* status;       // resident forms: the device status words, [0] the instance count; null: the host knows R = BL.R
  uint2* ranges() const { return (uint2*)(img + IL.ranges); }
  const uint32_t* point_list() const { return (const uint32_t*)(bin + BL.vals[0]); }
  float* final_T() const { return (float*)(img + IL.final_T); }
  uint32_t* n_contrib() const { return (uint32_t*)(img + IL.n_contrib); }
};
inline Scratch carve(const ScratchBuffers& B, int P, const View& V, uint32_t* status) {
  return Scratch{geom_at(B.geom_buffer, P, B.geom_rows), align_ptr(B.image_buffer), align_ptr(B.binning_buffer), image_layout(V.width, V.height),
                 binning_layout(B.capacity), gauss_sort_layout(B.capacity, P), status};
}

// Where the depth sort of the Gaussians reads its keys and values first -- where make_depth_keys_kernel or K1 has to leave them.
struct DepthSortInput { uint32_t *keys, *vals; };
inline DepthSortInput depth_sort_input(char* bin, const GaussSortLayout& GS, int dbits, int digit_bits) {
  const int side = sort_first_side(dbits, digit_bits);
  return DepthSortInput{(uint32_t*)(bin + GS.base + GS.inner.keys[side]), (uint32_t*)(bin + GS.base + GS.inner.vals[side])};
}

// How run_binning orders the Gaussians by depth: keys in [dmin, dcull], dcull - dmin < 2^dbits; culled Gaussians carry dcull.
struct BinningMode {
  uint32_t dmin; int dbits; uint32_t dcull;
  int digit_bits;              // of the depth sort: 8 or 9
  const uint32_t* k1_keys;     // non-null: K1 wrote the keys here (culled Gaussians carry the all-ones key and are dropped by the
                               // first depth pass); null: make_depth_keys_kernel makes them from the bin records
  bool drop_dead;              // dead instances (no quadrant of their tile can reach alpha >= 1/255) are dropped by the first tile-id pass
  // The exact depth range is only known on the device, so K1 writes the raw depth bits as keys and the sort looks at
  // DEPTH_KEY_BITS = 27 bits above the near plane's pattern in three 9-bit passes (see kernels.h).
  static constexpr int RESIDENT_DIGIT_BITS = 9;
  static BinningMode resident_keys(const uint32_t* k1_keys, bool drop_dead) {
    return BinningMode{DEPTH_KEY_MIN, DEPTH_KEY_BITS, 0xFFFFFFFFu, RESIDENT_DIGIT_BITS, k1_keys, drop_dead};
  }
  // hdr[1], hdr[2] of the synchronising forward: max(~depth_bits), max(depth_bits)
  static BinningMode exact_range(uint32_t max_not_depth, uint32_t max_depth, bool drop_dead) {
    const uint32_t dmin = ~max_not_depth, dspan = max_depth - dmin + 1u;   // +1: the key of culled Gaussians, one past the deepest visible
    int dbits = 1;
    while (dbits < 32 && (dspan >> dbits) != 0u) dbits++;
    const bool nine = (dbits + 8) / 9 < (dbits + 7) / 8;   // e.g. the usual 26 bits: three 9-bit passes instead of four 8-bit ones
    return BinningMode{dmin, dbits, dmin + dspan, nine ? 9 : 8, nullptr, drop_dead};
  }
};
inline DepthSortInput resident_depth_sort_input(char* bin, const GaussSortLayout& GS) { return depth_sort_input(bin, GS, DEPTH_KEY_BITS, BinningMode::RESIDENT_DIGIT_BITS); }

// Where K1 writes beyond the geometry buffer (all optional), and the flags it gets on top of segs_raster_set_flags.
struct K1Targets {
  uint32_t *depth_keys = nullptr, *depth_vals = nullptr;
  uint2* ranges = nullptr;          // non-null: K1 zeroes the range table
  uint32_t extra_flags = 0u;
  uint32_t* depth_overflow = nullptr;
};

// The per-Gaussian backward: what differs between its callers besides the Gaussians and the outputs.
struct PerGaussianBwd {
  float* gacc = nullptr;           // the tile backward's accumulator rows; null (debug): dL_dmean2D / dL_dconic are inputs
  bool depth = false;              // + row dword [9] (dL/dz) into dL/dmean3D; it is only ever non-zero after a depth-map gradient
  bool clean_gacc = false;         // write zeros back over every row consumed
  const float* dz_in = nullptr;    // debug: dL/dz as an input
  const segs_camera_grads* cam = nullptr;   // camera form: + one row of partial sums per workgroup, added up by a second kernel
  uint8_t* written = nullptr;      // the "row written" bytes (gs_layout.h)
  bool packed = false;             // with the bytes: preprocess_bwd_packed_kernel (a workgroup's reached rows in one wave when they are at most 64)
};

struct Allocators { segs_alloc_fn geometry_alloc; void* geometry_ctx; segs_alloc_fn binning_alloc; void* binning_ctx; segs_alloc_fn image_alloc; void* image_ctx; };

enum GaccCleaning { MEMSET_PER_CALL, SELF_CLEAN };
struct BackwardInputs { const float* background; const int* radii; const float* dL_dpix; const segs_depth_grads* dgrad; const segs_camera_grads* cam; };

// the optional arguments an entry point does not have, by name
constexpr const Gaussians* K1_RAN_AT_PRODUCER = nullptr;
constexpr const segs_depth_outputs* NO_DEPTH_OUTPUTS = nullptr;
constexpr const segs_depth_grads* NO_DEPTH_GRADS = nullptr;
constexpr const segs_camera_grads* NO_CAMERA_GRADS = nullptr;
constexpr const float *NO_CAM_POS = nullptr, *NO_DL_DZ = nullptr;
constexpr int* NO_RADII = nullptr;

}  // namespace segs
