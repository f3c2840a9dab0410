// uva_plan.h -- the host-side frame planner of libuva (csrc/uva_plan.cpp): the plane list of a frame and every table of HBM
// byte offsets the Compact kernels walk (trunk_kernel's tile schedule, the step lists of trunk2_kernel and trunkw_kernel, the
// row lists of sub10_kernel and sub5_kernel), with the structs and geometry constants host and kernels share.
//
// Plain C++17: the standard library and HIP's vector types (uint4), no HIP runtime, no device code, no environment reads.
// Every builder is a function of its arguments, so the unit also compiles and runs alone, under the host sanitizers
// (tests/host/plan_check.cpp).  The kernel headers include this file instead of defining the shared names themselves.
#pragma once
#include <hip/hip_vector_types.h>
#include <stddef.h>
#include <stdint.h>

#include <string>
#include <vector>

namespace uva {

constexpr int TH = 8;           // work-tile rows
constexpr int TW = 32;          // work-tile columns (= one MFMA N fragment)
constexpr int MAX_PLANES = 64;

// One independent sub-image.  The reference cuts a frame into <=980x980 tiles
// (upscale_processing.py:395-434) and feeds each through the net on its own; each such tile is a
// "plane" here, and all planes of a frame go through every layer in one launch.
struct PlaneDesc {
    int h, w;               // plane size in input pixels
    int nty, ntx;           // work tiles
    int tile_begin;         // first global work-tile index of this plane
    int pitch;              // activation row pitch in pixels (ntx*TW + 2)
    long long act_off;      // pixel offset of the plane's padded array inside the activation buffer
    int src_y0, src_x0;     // plane origin inside the source frame
    int core_y0, core_y1;   // plane-local rows whose output is written (border cropped, :464-477)
    int core_x0, core_x1;   // plane-local columns whose output is written
    int nty4;               // work tiles of the trunk kernel (4-row tiles)
    int tile_begin4;        // first global 4-row work-tile index of this plane
};
static_assert(sizeof(PlaneDesc) == 64, "PlaneDesc layout");

struct Trunk2Step {                             // 32 bytes
    // A half: x = input halo origin byte offset (low 32), y = offset bits 32..39 | row mask << 8 (bit r:
    // intermediate row r of the block is inside the plane) | c_lo << 12 | c_hi << 18 (intermediate columns
    // [c_lo, c_hi) of the block are inside the plane) | active << 24, z = row pitch in bytes
    uint4 a;
    // B half: x = output origin byte offset (low 32), y = offset bits 32..39 | valid rows << 8 |
    // valid columns << 11 | active << 24, z = row pitch in bytes
    uint4 b;
};
static_assert(sizeof(Trunk2Step) == 32, "Trunk2Step layout");

constexpr int PLAN_PIXB = 128;                  // HBM bytes per pixel of the 64-feature nets' activations (Geo<64>::PIXB)

// trunk2_kernel (csrc/uva_kernels.hip.h)
constexpr int T2_SW = 30;                       // output columns per strip
constexpr int T2_SLOTS = 4;                     // input halo-tile ring (A only: one tile per period; tile it+1 is complete
                                                // one barrier before its k-loop, so its first fragments are read early)
constexpr int T2_PAD_STEPS = T2_SLOTS;          // dummy entries behind a workgroup's last step (DMA look-ahead)

// trunkw_kernel (csrc/uva_wino.hip.h)
constexpr int TW_SW = 30;                         // output columns per strip
constexpr int TW_PAD_STEPS = 2;                   // dummy entries behind a workgroup's last step (DMA look-ahead)
constexpr int TW_FOLD_MAXW = 12;                  // widest last strip two planes can share (folded steps: pairs 0..6 per plane)

// sub10_kernel's row lists (csrc/uva_sub10.h)
constexpr int S10_WC = 80;                       // computed columns per strip (five 16-pixel fragments)
constexpr int S10_NL = 10;                       // layers = pipeline stages
constexpr int S10_VALID = S10_WC - 2 * S10_NL;   // columns of the strip the last layer gets right
constexpr int S10_MAX_ROWS = 640;                // row descriptors of a workgroup, copied to LDS (8 B each)
constexpr int S10_MAXB = 8;                      // frames per launch (uva_net_process_u8_device_batch)
constexpr int S10_YBIAS = 16;                    // a descriptor's row travels as y + S10_YBIAS (rows -10.. are warm-up rows) ...
constexpr int S10_FSHIFT = 16;                   // ... below the frame's index: ((frame << S10_FSHIFT) | (y + S10_YBIAS))
constexpr int S10_MAX_H = (1 << S10_FSHIFT) - 2 * S10_YBIAS;

// sub5_kernel's row lists (csrc/uva_sub5.h)
constexpr int S5_WC = 64;                        // computed columns per strip: four 16-pixel MFMA fragments
constexpr int S5_NL = 5;                         // layers per launch = stages of a pipeline
constexpr int S5_VALID = S5_WC - 2 * S5_NL;      // 54: the columns of a strip the fifth layer gets right
constexpr int S5_PAIRW = 2 * S5_VALID;           // 108: a workgroup's two pipelines cover neighbouring strips
constexpr int S5_MAX_ROWS = 1024;                // row descriptors of a workgroup, copied to LDS (8 B each)

// ---- the builders.  All return 0, or 1 with the refusal in `err`; every one that deals work out to workgroups refuses a
// `grid` that is not a multiple of 8 of at least 8 (workgroup_of_chunk is a bijection only then).

// whole-frame planes carry no tiling: tile_size <= 0 means (0, 0)
inline void normalize_tiling(int& tile_size, int& border)
{
    if (tile_size <= 0) tile_size = border = 0;
}
// consecutive chunks of a dealt-out sequence go to the workgroups of one XCD (block b runs on XCD b % 8)
inline int workgroup_of_chunk(size_t c, int grid) { return (int)(c % (grid / 8)) * 8 + (int)(c / (grid / 8)); }

int build_planes(int h, int w, int tile_size, int border, std::vector<PlaneDesc>& out, std::string& err);
size_t plan_guard_bytes(const std::vector<PlaneDesc>& planes, int nf);      // eight rows of the widest plane
int build_sched4(const std::vector<PlaneDesc>& planes, std::vector<uint4>& sched4, std::string& err);
int build_trunk2_schedule(const std::vector<PlaneDesc>& planes, int grid, size_t guard_bytes, std::vector<Trunk2Step>& steps,
                          std::vector<int>& nsteps, int* max_steps, bool narrow_ok, std::string& err);
// trunkw's A/B switches (uva_api.hip reads UVA_TW_SIX / UVA_TW_FOLD into them per call)
struct TrunkwOpts {
    int six_mode = -1;                // six-row segment starts: 1 always, 0 never, -1 where they shorten the longest list
    bool fold = true;                 // two planes of one size share the walk of their narrow last strips
    int fold_maxw = TW_FOLD_MAXW;     // (14: the known-bad first version, kept for the tests' structured-error detector)
};
int build_trunkw_schedule(const std::vector<PlaneDesc>& planes, int grid, size_t guard_bytes, std::vector<Trunk2Step>& steps,
                          std::vector<int>& nsteps, int* max_steps, const TrunkwOpts& opts, std::string& err);
// Row lists of the strip-walking 1x kernels: `frames` x `units_per_frame` strip units of `unit_w` columns, every segment
// with `nl` warm-up rows above and below.  A row word is (y, first computed column, written-out bit | frame << 8,
// dist_in_w ? rows to the nearest written-out row : 0).  Returns 2 (no text) where a list outgrows max_rows.
struct StripRowsSpec { int unit_w, units_per_frame, frames, nl, max_rows; bool dist_in_w; };
int build_strip_rows(const StripRowsSpec& s, int h, int grid, std::vector<uint4>& rows, std::vector<int>& nrows, int* max_rows,
                     std::string& err);
int build_sub10_rows(int h, int w, int frames, int grid, std::vector<uint4>& rows, std::vector<int>& nrows, int* max_rows, std::string& err);
int build_sub5_rows(int h, int w, int grid, std::vector<uint4>& rows, std::vector<int>& nrows, int* max_rows, std::string& err);

struct PlanOpts {
    TrunkwOpts tw;
    bool narrow_ok = true;            // trunk2: strips of <= 14 columns compute one fragment column (UVA_T2_NARROW=0: both)
};
// What get_workspace needs to know about one frame geometry before it allocates: the planes and their layout ...
struct PlaneLayout {
    std::vector<PlaneDesc> planes;
    size_t act_pixels = 0;            // pixels of all padded plane arrays
    int ntiles = 0, ntiles4 = 0;      // 8-row work tiles (head, tail, 24-feature trunk) / 4-row work tiles (64-feature trunk kernel)
    // Zeroed, never written bytes on both ends of an activation buffer: they keep trunk2_kernel's halo reads of rows -2 / h+4
    // and columns -2 / pitch+1 -- which only ever feed pixels it masks to zero -- inside the allocation.
    size_t guard_bytes = 0;
};
void layout_planes(PlaneLayout& l);    // from planes[].h / .w: everything else of the layout but the guard
// ... and, for the 64-feature nets, the three schedules on `grid` workgroups
struct FramePlan : PlaneLayout {
    std::vector<uint4> sched4;
    std::vector<Trunk2Step> steps2, stepsw;
    std::vector<int> nsteps2, nstepsw;
    int max_steps2 = 0, max_stepsw = 0;
};
int plan_frame(int h, int w, int tile_size, int border, int nf, int grid, const PlanOpts& opts, FramePlan& plan, std::string& err);

}  // namespace uva
