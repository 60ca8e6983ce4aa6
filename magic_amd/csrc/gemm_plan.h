// Which kernel a GEMM runs on, at which tile and split: one host-side planner (gemm_plan.cpp, no
// kernels, no HIP calls). gemm_run launches what gemm_plan returns; the context's planning stages
// and mvae_debug_plan ask the same function. DESIGN.md 5q.
#pragma once
#include <cstddef>

namespace mvae {

struct GemmDesc;

enum GemmKernel {
  K_AUTO = 0,   // (a force only) the planner decides
  K_F32 = 1,    // fp32 MFMA, 128x128 tiles (gemm_f32.hip)
  K_VALU = 2,   // fp32 VALU, 64x64 tiles, skinny shapes (gemm_valu.hip)
  K_PLANE = 3,  // bf16 planes, 128x128 register-staged tiles (gemm_bf16.hip)
  K_RING = 4,   // bf16 planes, 256 / 192-row LDS-DMA ring tiles (gemm_bf16.hip)
  K_X3 = 5,     // ... the plane-stacked form of a six-pair f32x ring plan (create option x3)
  K_E8 = 6,     // bf16 planes, 256x256 eight-phase kernel (gemm_bf16e.hip)
};

// What a caller fixes of the choice; the default-constructed value leaves everything to the planner.
struct GemmForce {
  // K_VALU: that kernel. K_PLANE: the 128x128 kernel of the precision (K_F32 in fp32 mode). K_RING:
  // the 256-row ring kernels, never the eight-phase one. K_E8: the eight-phase kernel where its
  // 32-bit plane offsets fit, else the ring kernels. (K_RING / K_E8 in a plane mode; K_F32 / K_X3
  // are outcomes, not forces.)
  int kernel = K_AUTO;
  // K_RING / K_E8 on any shape; else the default shape rules still decide between the 256-row
  // kernels and the 128x128 one (gemm_wide)
  bool any_shape = false;
  bool no_e8 = false;        // the planner's choice, without the eight-phase kernel
  // (ABI number 6 only) a forced K_E8 whose offsets do not fit keeps the ring candidates to output
  // dimensions >= 128; below, the unsplit 256x256 ring tile runs
  bool ring_from_128 = false;
  // (ABI numbers 5, 7, 8: once timing forms of the ring kernel, kept for the tests that pass them)
  // K_RING by the default shape rules but for the one-k-tile exclusion, launched at 256x256 tiles
  // with the split the planner chose for its own tile
  bool late_256 = false;
  int tile_n = 0;            // ring tile N: 128 or 256; 0 = planner
  int tile_m = 0;            // ring tile M: 192 (where eligible) or 256; 0 = planner
  bool cd_epilogue = false;  // ring kernels: the accumulator (C/D) layout's epilogue, never through LDS
  int staging = 0;           // 128x128 kernels, store epilogue: diagnostic staging forms 1 / 2
  int split = 0;             // split-K; 0 = planner
  // a kernel family is named or excluded (every ABI number but 0): the step's wiring then leaves the
  // GEMM where it is (gemm_valu_fits)
  bool names_kernel() const { return kernel != K_AUTO || no_e8; }
};

// What gemm_run launches.
struct GemmPlan {
  int kernel = K_F32;
  int staging = 0;
  int tm = 128, tn = 128;    // workgroup tile (K_E8: 256 x 256)
  int ntm = 0, ntn = 0;      // tiles of one batch element's output
  int group = 0;             // tile order (gemm::Params::group)
  int split = 1;
  int kchunk = 0;            // k per split-K slice, whole k-tiles
  bool lds_epilogue = false; // 256-row kernels: row-major epilogue through LDS (else the C/D layout's)
  bool vec_epilogue = false; // ... with 16-byte accesses (bases and strides allow them)
  int epi_launched = 0;      // EpiMode of the kernel instantiation (EPI_STORE when split > 1)
  size_t ws_elems = 0;       // floats of split-K slabs
};

inline bool gemm_wide_kernel(int kernel) { return kernel >= K_RING; }  // the 256-row bf16-plane kernels

// the kernels' tiles the plan counts in: 128x128 (gemm_common.h BM / BN) with k-tiles of 32 (fp32)
// or 64 (bf16 planes, every plane kernel); the VALU kernel's 64x64 with k-chunks of 32
constexpr int PLAN_T128 = 128, PLAN_BK_F32 = 32, PLAN_BK_PLANE = 64, PLAN_VT = 64, PLAN_VKC = 32;

// One pass: the plan of d with at most max_ws floats of workspace (a forced split is kept whatever
// max_ws: gemm_run then refuses the launch). ws_aligned: the workspace is 16-byte aligned (it decides
// the eight-phase kernel's 16-byte slab stores).
GemmPlan gemm_plan(const GemmDesc& d, size_t max_ws, bool ws_aligned = true);
// gemm_run refuses the plan (hipErrorInvalidValue): its slabs do not fit the workspace given
inline bool gemm_plan_refused(const GemmPlan& pl, bool has_ws, size_t ws_elems) {
  return pl.split > 1 && (!has_ws || pl.ws_elems > ws_elems);
}
// The skinny shapes the step's wiring moves to K_VALU (an output dimension or K <= 64), where nothing
// is forced.
bool gemm_valu_fits(const GemmDesc& d);
// Floats of workspace d needs when the planner is free to split: gemm_plan(d, unlimited).ws_elems.
size_t gemm_workspace_elems(const GemmDesc& d);

}  // namespace mvae
