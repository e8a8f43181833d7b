// Device-side views and launcher declarations shared by the kernels and the C-ABI layer.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <type_traits>
#include <utility>

#include "cpf.h"
#include "cpf_internal.h"   // kGroupBase

namespace cpf {

constexpr int kBlock = 256;   // 4 waves of 64
constexpr int kCounterSlots = 1024;   // statistics counters are sharded over this many 32-byte slots

// Mesh as the kernels see it (all arrays resident in HBM, L2-resident for tutorial-size meshes)
struct MeshView {
    const int32_t* cellOff;   // [nCells+1]
    const double4* planes;    // [nSlots]   (nx, ny, nz, d), unit normal into the cell
    const int32_t* nbr;       // [nSlots]   neighbour cell | -(face + 1) on the boundary | kGroupBase + g: face group g (cpf_mesh.cpp)
    const int32_t* groupOff;  // [nGroups+1] face groups: the cells behind the coplanar pieces of one slot, in face order
    const int32_t* groupNbr;
    const double4* U;         // [nCells]   cell-constant velocity, w unused (32-B aligned gathers)
    const double4* cellRec;   // [nCells][8] packed 256-B records (null: generic walk only); layout: cpf_walk.h "cell records"
    const double4* boxRec;    // [nCells][4] 128-B box records (null: some cell is not an axis-aligned box); cpf_walk.h "box records"
    int32_t nCells;
    int32_t allHex;           // every cell has exactly 6 face slots (slot = 6*cell + s) and there are no face groups
    int32_t zPairLast;        // ... and slots 4, 5 of every cell are its two faces with an exactly z-parallel normal (cpf_mesh.cpp)
    int32_t zSide0;           // ... and the four other faces of every cell have nz == 0 exactly (2-D mesh extruded straight in z)
    int32_t zThin;            // ... and both are boundary faces in every cell: one cell thick in z (cpf_walk.h, fold_z)
    int32_t mixed;            // records exist although the mesh is not all-hex: 1 = padded records (< 6 slots) and face groups only, 2 = header-only records (> 6 slots) as well
};

struct GridView {
    double origin[3], invBin[3], lo[3], hi[3];
    int32_t dims[3];
    const int32_t* binOff;
    const int32_t* binCells;
};

// Host-side state of the streaming step kernel (cpf_stream.hip): two sets of per-group chunk counters (a launch
// uses one and zeroes the other for the launch after it on the same stream) and the tuning knobs.
constexpr size_t kStreamGrabBytes = 2 * 256 * 16 * sizeof(unsigned);
constexpr int kStreamHitSpillDoubles = 3 * 64;          // x[64] | y[64] | z[64] per wave
struct StreamState {
    unsigned* d_grab = nullptr;
    double* d_hitSpill = nullptr;   // wall hit points that do not fit a wave's LDS pool: kStreamHitSpillDoubles per wave slot (cpf_stream.hip)
    int hitSpillWaves = 0;          // wave slots d_hitSpill has room for (the launcher never starts more single-wave workgroups)
    int parity = 0;
    int numCU = 256;
    int tilesPerChunk = 0;    // "stream_tiles_per_chunk"; 0 = by lookup method: 4 (loop lookup), 3 (fixed lookup: slower tiles, finer dealing)
    int wavesPerCU = 0;       // "stream_waves_per_cu": 0 = what the occupancy query says
    int coopMaxCells = 0;     // "coop_max_cells": test hook, lowers the wave-cooperative kernel's 2^24-cell limit (0 = the limit)
    int lookup = -1;          // "stream_lookup": a mode of kLookupModes (below), 0 ... 6; -1 = by particles per cell
    double tailFraction = -1.0; // "stream_tail_fraction": share of the cloud dealt tile by tile at the end of a launch; < 0 = by lookup method: 0.1 / 0.2
    int debug = 0;            // "stream_debug": diagnostics only (1 = no stores, 2 = no loads; results are wrong)
    // What the last sort found: [0] cells that hold particles, [1] live particles (pinned host memory, written by an async copy
    // behind every sort; null / zeros = not known).  With "stream_lookup_by_density" 1 the lookup method goes by particles per
    // OCCUPIED cell instead of per cell of the whole mesh: the tutorials seed their clouds in a small box (TJunction: 4e6
    // particles in 20 000 of 248 000 cells -- 200 per cell, not 16).  Read without synchronisation: an old value only costs
    // a launch or two on the other -- bit-identical -- instantiation.  OFF by default, measured (round 4, one box): TJunction
    // as its dictionary runs it, D = 1.5e-5, takes 0.150 ms per step with the fixed compare the whole-mesh figure picks and
    // 0.177 ms with the loop lookup the density picks -- on a 3-D mesh with the kick a tile's lanes spread over more cells
    // per round than the 128-per-cell threshold, tuned on pitzDaily, assumes.
    const volatile unsigned long long* occupiedHost = nullptr;
    int densityLookup = 0;    // "stream_lookup_by_density"
    // the velocity field last set has no z component anywhere (U.z == +-0 in every cell; found by the kernel that lays the field
    // out, read back behind it): with MeshView::zSide0 and without the kick the FLAT instantiation runs (cpf_walk.h "flat walk")
    bool flatField = false;
    int flat = 1;             // "flat_walk": 0 = never (diagnostics; bit-identical either way)
    int flatZ = 1;            // "flat_z": 0 = the flat instantiations always stream z (A/B; bit-identical either way)
    // pinned host word that a flat launch streaming z sets when it loads a live particle with a non-finite z (StreamArgs::zBad);
    // its owner reads it behind that launch, before it calls the cloud settled.  Null: nobody asks (such a cloud never counts as settled)
    unsigned* zBad = nullptr;
};

constexpr int kCoopMaxCells = 1 << 24;     // 32-bit record byte offsets in step_kernel_coop (plan_step falls back above that)
constexpr int kFusedCoopCycles = 1 << 30;  // fused launches of this many cycles or more run the wave-cooperative kernel: never since round 4
                                          // (round 3, 8: the streaming kernel was 4 % faster per cycle at 3 fused cycles, 2 % slower at 8; with
                                          // the flat walk and box records it is 5-30 % faster at 8 and 16 -- cpf_stream.hip, plan_step)
struct VertexField;                  // cpf_walk.h

// ------------------------------------------------------------------------------------------------
// The streaming kernels' LOOKUP (cpf_stream.hip: the last template argument of step_kernel_stream, _vertex and _flat; StepPlan::lookup):
// how a wave finds its cells in its record cache, and which records can turn up.  THE legend of the modes and the one place that
// says what a number means -- the planner, the launcher, the option check and the kernel all read kLookupModes; what a mode costs in
// record slots, waves per SIMD and hit pool is StreamShape (cpf_stream.hip), what it measured docs/design_r04.md 5.1.  The values
// are part of every kernel's name (profiles, tests, tools/condense_profile.py know them): a new mode takes a new number.
//   0  kLookupLoop       all-hex mesh, many particles per cell (>= 128: 1-3 distinct cells per round): one scalar iteration per
//                        DISTINCT cell of the wave, a compare against the scalar cell id
//   1  kLookupFixed      all-hex mesh, few particles per cell (3-D meshes: 5-13 distinct cells per tile): six compares of every
//                        lane's cell against the broadcast tags
//   2  kLookupMixedBig   as 3, and header records of cells with more than six slots may turn up as well (two-record cells: a visit
//                        in two rounds; beyond twelve slots the CSR walk) -- MeshView::mixed == 2
//   3  kLookupMixed      fixed compare on a mesh that is not all-hex (MeshView::mixed) whose cells all have at most six slots: face
//                        groups and padded records only, the usual 2:1-refined hex mesh
//   4  kLookupSparse     fixed compare for SPARSE clouds on all-hex meshes (fewer than kStreamSparsePerCell particles per cell: nearly
//                        every lane of a tile sits in a cell of its own and walks by per-lane gathers from L2 / HBM): the gather walk
//                        keeps three planes in flight instead of one -- two dependent round trips per visit instead of six -- for 24
//                        more registers, i.e. five waves per SIMD.  2.1e6-cell box: 1.25e6 particles (one rank's share of BASELINE
//                        configs[4]) 0.187 -> 0.141 ms, 1e7 particles 0.673 / 0.631 -> 0.641 / 0.607; in the dense regime the same
//                        change costs 6 % (0.259 -> 0.277)
//   5  kLookupMixedLoop  as 3 with the LOOP lookup and six slots: a refined mesh that still holds hundreds of particles per cell
//                        (pitzDaily with a 2:1 patch: 0.157 -> see docs/design_r04.md 5.6)
//   6  kLookupBox        as 1 on the mesh's 128-byte BOX records instead of the 256-byte ones (every cell an axis-aligned box:
//                        cpf_walk.h "box records") -- dense and sparse clouds alike: three candidate faces per visit, one LDS round
//                        trip per record, one cache line per gathered record
//   8  kLookupFlatLoop   as 0 with the FLAT walk (cpf_walk.h): a 2-D mesh extruded straight in z, a field without a z component, no
//                        kick -- the headline; behind it every live particle's z is settled (StepPlan::flat)
//   9  kLookupFlatFixed  as 1 with the flat walk (a 2-D mesh with fewer than 128 particles per cell: refined 2-D cases)
//   11 kLookupBoxGroups  as 6 on a mesh with face groups: 2:1-refined boxes (box records with group slots)
// "stream_lookup" (StreamState::lookup) may ask for 0 ... 6; 8, 9 and 11 are the planner's own (stream_lookup_mode).
enum : int { kLookupLoop = 0, kLookupFixed = 1, kLookupMixedBig = 2, kLookupMixed = 3, kLookupSparse = 4, kLookupMixedLoop = 5,
             kLookupBox = 6, kLookupFlatLoop = 8, kLookupFlatFixed = 9, kLookupBoxGroups = 11 };
struct LookupMode {
    int id;
    bool fixed;        // compare every lane's cell against the tags (else: loop over the wave's distinct cells)
    bool mixed;        // mixed records: face groups and padded records can turn up
    bool bigCells;     // ... and two-record cells and header records
    bool box;          // 128-byte box records
    bool flat;         // the flat walk
    int gatherAhead;   // planes the per-lane gather walk keeps in flight beyond the one it tests (0: the plain gather walk)
};
constexpr LookupMode kLookupModes[] = {
    // id               fixed  mixed  big    box    flat   ahead
    {kLookupLoop,       false, false, false, false, false, 0},
    {kLookupFixed,      true,  false, false, false, false, 0},
    {kLookupMixedBig,   true,  true,  true,  false, false, 0},
    {kLookupMixed,      true,  true,  false, false, false, 0},
    {kLookupSparse,     true,  false, false, false, false, 3},
    {kLookupMixedLoop,  false, true,  false, false, false, 0},
    {kLookupBox,        true,  false, false, true,  false, 0},
    {kLookupFlatLoop,   false, false, false, false, true,  0},
    {kLookupFlatFixed,  true,  false, false, false, true,  0},
    {kLookupBoxGroups,  true,  true,  false, true,  false, 0},
};
constexpr int kLookupModeCount = (int)(sizeof(kLookupModes) / sizeof(kLookupModes[0]));
// the table's row of a mode; id -1: no such mode
constexpr LookupMode lookup_traits(int lookup) {
    for (const LookupMode& r : kLookupModes)
        if (r.id == lookup) return r;
    return {-1, false, false, false, false, false, 0};
}
// the table pinned to the numbers every profile and test knows: the modes that have a property, as a bit set of their values
constexpr unsigned lookup_set(bool LookupMode::*property) {
    unsigned s = 0;
    for (const LookupMode& r : kLookupModes)
        if (r.*property) s |= 1u << r.id;
    return s;
}
constexpr unsigned lookup_bits() { return 0u; }
template <class... T>
constexpr unsigned lookup_bits(int id, T... more) { return (1u << id) | lookup_bits(more...); }
static_assert(kLookupModeCount == 10 && lookup_traits(7).id == -1 && lookup_traits(10).id == -1, "ten modes: 0 ... 6, 8, 9, 11");
static_assert(lookup_set(&LookupMode::fixed) == lookup_bits(1, 2, 3, 4, 6, 9, 11), "loop lookup: 0, 5, 8");
static_assert(lookup_set(&LookupMode::mixed) == lookup_bits(2, 3, 5, 11), "mixed records");
static_assert(lookup_set(&LookupMode::bigCells) == lookup_bits(2), "two-record cells");
static_assert(lookup_set(&LookupMode::box) == lookup_bits(6, 11), "box records");
static_assert(lookup_set(&LookupMode::flat) == lookup_bits(8, 9), "flat walk");
static_assert(lookup_traits(4).gatherAhead == 3 && lookup_traits(0).gatherAhead + lookup_traits(1).gatherAhead +
              lookup_traits(2).gatherAhead + lookup_traits(3).gatherAhead + lookup_traits(5).gatherAhead + lookup_traits(6).gatherAhead +
              lookup_traits(8).gatherAhead + lookup_traits(9).gatherAhead + lookup_traits(11).gatherAhead == 0, "gather ahead: 4 only");

// What one step launch runs: plan_step (cpf_stream.hip) decides, launch_step runs it, cpf_step_dev times it and learns from
// it whether the launch settles z, cpf_step_kernel_name prints it.
struct StepPlan {
    // kGeneric .. kAhead: the kernels of the step variants (cpf_walk.h kVariant*, "step_variant"); kVertex, kStreamVertex: the
    // "VertexVelocity" cycle (CPF_STEP_VERTEX_VELOCITY) on step_kernel_vertex / step_kernel_stream_vertex
    enum Kernel { kGeneric = 0, kFixed = 1, kFixedScalar = 2, kCoop = 3, kStream = 4, kAhead = 5, kVertex, kStreamVertex };
    Kernel kernel = kGeneric;
    bool brown = false, reflect = false, storeVel = false, stats = false;   // the template flags
    int lookup = -1;      // the streaming kernels' LOOKUP: a mode of kLookupModes (above)
    bool cone = false;    // the vertex kernels: cone locate (else all tets)
    // timed, the streaming kernels take the events to hipExtLaunchKernelGGL -- start and stop are then the dispatch's own begin
    // / end time stamps, what rocprofv3's kernel trace reports, instead of events recorded around the launch (which also time
    // the gap an event record puts between two otherwise back-to-back kernels: 5 % on a 0.12 ms kernel)
    bool stamped() const { return kernel == kStream || kernel == kStreamVertex; }
    // the flat walk: every live particle's z is settled behind it (CPF_STEP_Z_SETTLED)
    bool flat() const { return kernel == kStream && lookup_traits(lookup).flat; }
    // ... on a cloud whose z is settled: step_kernel_stream_flat, the body in which z does not exist ("flat_z" 0: never)
    bool flat_body(const StreamState& ss, bool zSettled) const { return flat() && zSettled && ss.flatZ != 0; }
};
// vf: the "VertexVelocity" cycle's tables (null: the cell-constant cycle); stats: statistics counters are on
StepPlan plan_step(const MeshView& m, const StreamState& ss, int variant, const VertexField* vf, int64_t n, int nCyc, double D,
                   unsigned flags, bool stats);
// zSettled: the cloud's z is settled (CPF_STEP_Z_SETTLED; a flat launch then runs the body without z, StepPlan::flat_body);
// evStart / evStop: the time stamps of a plan.stamped() launch (null: untimed)
hipError_t launch_step(const StepPlan& p, hipStream_t st, double* x, double* y, double* z, int32_t* cell, const int64_t* gid,
                       double* vel, int64_t n, double dt, double D, uint32_t step0, int nCyc, uint32_t seed, const MeshView& m,
                       unsigned long long* counters, const VertexField* vf, StreamState& ss, bool zSettled, hipEvent_t evStart,
                       hipEvent_t evStop);
// launch_step's kernels in the other translation units
hipError_t launch_step_stream(const StepPlan& p, hipStream_t st, double* x, double* y, double* z, int32_t* cell, const int64_t* gid,
                              double* vel, int64_t n, double dt, double sigma, uint32_t step0, int nCyc, uint32_t seed,
                              const MeshView& m, unsigned long long* counters, const VertexField* vf, StreamState& ss, bool zSettled,
                              hipEvent_t evStart, hipEvent_t evStop);
hipError_t launch_step_ahead(const StepPlan& p, hipStream_t st, double* x, double* y, double* z, int32_t* cell, int64_t n, double dt,
                             const MeshView& m, unsigned long long* counters, StreamState& ss, double* dbg);
// f(std::bool_constant<b>{}...) for the run-time bools b...: a launcher's flags as template arguments, one instantiation per combination
template <class F>
decltype(auto) with_bools(F&& f) { return f(); }
template <class F, class... Bs>
decltype(auto) with_bools(F&& f, bool b, Bs... bs) {
    if (b) return with_bools([&](auto... c) -> decltype(auto) { return f(std::true_type{}, c...); }, bs...);
    return with_bools([&](auto... c) -> decltype(auto) { return f(std::false_type{}, c...); }, bs...);
}

// f(std::integral_constant<int, id>{}) for the mode `lookup` of kLookupModes (none: hipErrorInvalidValue): a launcher's LOOKUP as a
// template argument, one instantiation per mode of the table -- f itself refuses, with `if constexpr`, the modes it has no kernel for
template <class F, size_t... I>
hipError_t with_lookup(int lookup, F&& f, std::index_sequence<I...>) {
    hipError_t e = hipErrorInvalidValue;
    (void)((lookup == kLookupModes[I].id && ((e = f(std::integral_constant<int, kLookupModes[I].id>{})), true)) || ...);
    return e;
}
template <class F>
hipError_t with_lookup(int lookup, F&& f) { return with_lookup(lookup, f, std::make_index_sequence<kLookupModeCount>{}); }

hipError_t launch_locate_initial(hipStream_t st, const double* x, const double* y, const double* z, int32_t* cell,
                                 int64_t n, const MeshView& m, const GridView& g);
hipError_t launch_seed_box(hipStream_t st, double* x, double* y, double* z, int64_t first, int64_t n,
                           const double lower[3], const double upper[3], int order);
hipError_t launch_iota64(hipStream_t st, int64_t* p, int64_t n, int64_t first);
hipError_t launch_unpack_xyz(hipStream_t st, const double* xyz, double* x, double* y, double* z, int64_t n);
hipError_t launch_pack_by_gid(hipStream_t st, const double* x, const double* y, const double* z, const int32_t* cell,
                              const int64_t* gid, const double* vel, double* xyzw, int32_t* cellOut, double* velOut,
                              int64_t n);
hipError_t launch_count_negative(hipStream_t st, const int32_t* cell, int64_t n, unsigned long long* out);
hipError_t launch_build_cell_records(hipStream_t st, const double4* planes, const int32_t* nbr, const double4* U,
                                     double4* rec, int64_t nCells);
hipError_t launch_build_cell_records_mixed(hipStream_t st, const int32_t* cellOff, const double4* planes, const int32_t* nbr,
                                           const double4* U, const int32_t* recB, double4* rec, int64_t nCells);
hipError_t launch_update_record_velocity(hipStream_t st, const double4* U, double4* rec, double* box, int64_t nCells);
hipError_t launch_u3_to_u4(hipStream_t st, const double* u3, double4* u4, int64_t nCells, unsigned long long* zFlag = nullptr);
// meshes with decomposed cells (cpf_parent.hip): per-parent U -> per-derived U[3]; derived -> parent cell ids (negative codes kept)
hipError_t launch_gather_parent_u3(hipStream_t st, const double* uParent, const int32_t* parentOf, double* uDerived, int64_t nDerived);
hipError_t launch_cells_to_parent(hipStream_t st, const int32_t* in, int32_t* out, const int32_t* parentOf, int64_t n, int64_t nDerived);

// stage-by-stage kernels on the reference's AoS layouts
hipError_t launch_stage_advect(hipStream_t st, double* P, const int32_t* ids, double* vels, double* disps, double dt,
                               int64_t n, const MeshView& m);
hipError_t launch_stage_advect_const(hipStream_t st, double* P, const int32_t* ids, const double* vels, double* disps, double dt,
                                     int64_t n);
hipError_t launch_stage_advect_vertex(hipStream_t st, double* P, const int32_t* ids, double* vels, double* disps, double dt,
                                      int64_t n, const double* pos, const int32_t* tets, int tetsPerCell,
                                      const double* vertVel, const double* cone, const double* apex);
// tet records of the "VertexVelocity" advect's cone locate: cone[nTets][32], apex[nCells][4] (cpf_walk.h, VertexField); the
// velocity part of the records follows every cpf_set_vertex_velocity
hipError_t launch_vertex_cone_tables(hipStream_t st, const double* pos, const int32_t* tets, int64_t nTets, int tetsPerCell, double* cone,
                                     double* apex);
hipError_t launch_vertex_record_velocity(hipStream_t st, const int32_t* tets, const double* vel, int64_t nTets, double* cone);
hipError_t launch_stage_brownian(hipStream_t st, const double* P, double* disps, double dt, int64_t n, double D,
                                 uint32_t step, uint32_t seed);
hipError_t launch_stage_locate(hipStream_t st, const double* P, const double* disps, int32_t* ids, int64_t n,
                               const MeshView& m);
hipError_t launch_stage_reflect(hipStream_t st, int32_t* ids, double* P, double* vels, double* disps, int64_t n,
                                const MeshView& m);
hipError_t launch_stage_move(hipStream_t st, double* P, double* disps, int64_t n);
hipError_t launch_aos_to_soa(hipStream_t st, const double* P, double* x, double* y, double* z, int64_t n);
hipError_t launch_soa_to_aos(hipStream_t st, const double* x, const double* y, const double* z, double* P, int64_t n);

// the re-sort by cell (cpf_sort.hip).  ox ... ogid: all null = in place; occupied, rank: may be null; method: "sort_method" -- 0 = the
// library radix sort (the order tests compare with), otherwise this library's own
size_t sort_scratch_bytes(int64_t n, int endBit);
hipError_t sort_by_cell(hipStream_t st, double* x, double* y, double* z, int32_t* cell, int64_t* gid, double* vel3,
                        int64_t n, int endBit, const float* cellBox, const int* subBits, const int* subOrder,
                        void* scratch, size_t scratchBytes, double* ox, double* oy, double* oz, int32_t* ocell, int64_t* ogid,
                        unsigned long long* occupied, const int32_t* rank, int method);

// multi-GPU hand-off (cpf_handoff.hip)
size_t handoff_scratch_bytes(int64_t n, int nRanks);
hipError_t pack_leavers(hipStream_t st, double* x, double* y, double* z, int32_t* cell, int64_t* gid, int64_t n,
                        const int32_t* cellLo, int nRanks, int myRank, double* sendbuf, int64_t sendCapacity,
                        int64_t* counts, int64_t* nStay, void* scratch, size_t scratchBytes);
size_t histogram_scratch_bytes(int64_t nCells);
hipError_t cell_histogram(hipStream_t st, const int32_t* cell, int64_t n, int64_t nCells, double scale, double* weights,
                          void* scratch, size_t scratchBytes);
hipError_t cell_ranges(hipStream_t st, const double* weights, int64_t nCells, int nRanks, int32_t* cellLo);
// per-cell occupancy (cpf_occupancy.hip): acc[parent of cell[i]] += 1 for every i with 0 <= cell[i] < nDerived, in place, one launch;
// parentOf null: the ids are parent ids already.  acc: 64-bit integers per PARENT cell
hipError_t occupancy_accumulate(hipStream_t st, const int32_t* cell, int64_t n, const int32_t* parentOf, int64_t nDerived,
                                unsigned long long* acc);
// recycling (cpf_recycle.hip).  sink_apply: cell[i] = CPF_CELL_LOST for every i with 0 <= cell[i] < nDerived whose bit is set in mask
// (ceil(nDerived / 32) words over DERIVED cells), *absorbed += their number.  respawn_box: the first maxCount (< 0: all) slots with
// cell < 0, in array order, get the position respawn_position(seed, gid, epoch) (cpf_philox.h; gid null: the index) and the cell of
// the initial locate; counters[1] += slots drawn, counters[2] += those found inside.  scratch: respawn_scratch_bytes(n) bytes
hipError_t sink_apply(hipStream_t st, int32_t* cell, int64_t n, const uint32_t* mask, int64_t nDerived, unsigned long long* absorbed);
size_t respawn_scratch_bytes(int64_t n);
hipError_t respawn_box(hipStream_t st, double* x, double* y, double* z, int32_t* cell, const int64_t* gid, int64_t n,
                       const double lower[3], const double upper[3], int64_t maxCount, uint32_t seed, uint32_t epoch,
                       const MeshView& m, const GridView& g, void* scratch, size_t scratchBytes, unsigned long long* counters);
// passes (a) and (b) of a limited respawn, for the place kernels of cpf_recycle.hip and cpf_inlet.hip: *offsets = the exclusive
// offsets of the slices' dead slots (in `scratch`), or null where maxCount cannot bind (< 0, or >= n)
hipError_t respawn_offsets(hipStream_t st, const int32_t* cell, int64_t n, int64_t maxCount, void* scratch, size_t scratchBytes,
                           const unsigned** offsets);
// patch source (cpf_inlet.hip).  The same candidates, order and counters as respawn_box; the position is source_point's
// (cpf_philox.h) on the table of cpf_source_table_host: rec[nKept][16] doubles, hi[nKept] bounds padded with 0xFFFFFFFF to a
// multiple of 4 entries (the kernel stages them with 16-byte loads)
struct SourceView { const double* rec; const uint32_t* hi; int32_t nKept; };
hipError_t respawn_source(hipStream_t st, double* x, double* y, double* z, int32_t* cell, const int64_t* gid, int64_t n,
                          const SourceView& src, int64_t maxCount, uint32_t seed, uint32_t epoch, const MeshView& m,
                          const GridView& g, void* scratch, size_t scratchBytes, unsigned long long* counters);
// flux table (cpf_inflow.hip; the rule: include/cpf.h "flux table", the arithmetic: cpf_inflow.h).  One refresh of hi[] and, with
// depthScale > 0, of column 13 of rec from U (uStride doubles a cell, indexed by owner[]), asynchronous on `st`: no allocation, no
// copy to the host, no wait.  area[nKept], owner[nKept]; w: 2 * nKept doubles; sums: 2 * inflow_blocks(nKept) words; slots: 4 words,
// [2] counts the refreshes that found no inflow and left the table alone
struct InflowView {
    double* rec; uint32_t* hi; int32_t nKept; double depthScale;
    const double* area; const int32_t* owner; double* w; unsigned long long* sums; unsigned long long* slots;
};
int64_t inflow_blocks(int64_t nKept);
hipError_t inflow_refresh(hipStream_t st, const InflowView& v, const double* U, int uStride);
// tracer age (cpf_age.hip).  birth[id] (n entries, id = gid[slot]; gid null: the slot) is the cycle count at which particle id last
// became live, an age is (uint32_t)(now - birth).  age_absorb: sink_apply, and hist[min(age / binCycles, nBins - 1)] += 1 for every
// particle it absorbs.  age_stamp: birth[id] = now for every slot with cell < 0.  age_field: for every i with 0 <= cell[i] <
// nDerived, field[2 * parent] += age and field[2 * parent + 1] += 1 (parentOf null: the ids are parent ids already)
hipError_t age_absorb(hipStream_t st, int32_t* cell, const int64_t* gid, const uint32_t* birth, int64_t n, const uint32_t* mask,
                      int64_t nDerived, unsigned long long* absorbed, uint32_t now, int32_t binCycles, int32_t nBins,
                      unsigned long long* hist);
hipError_t age_stamp(hipStream_t st, const int32_t* cell, const int64_t* gid, uint32_t* birth, int64_t n, uint32_t now);
hipError_t age_field(hipStream_t st, const int32_t* cell, const int64_t* gid, const uint32_t* birth, int64_t n,
                     const int32_t* parentOf, int64_t nDerived, uint32_t now, unsigned long long* field);
// tracer tags (cpf_tags.hip).  origin[id] (n bytes, id = gid[slot]; gid null: the slot) is the origin the respawn that last made
// particle id live gave it, sinkGroup[d] the group of DERIVED cell d.  tag_transfer: reads only; transfer[origin * nSinks + group]
// += 1 for every i that sink_apply would absorb (transfer: room for 16 x 16 words).  tag_stamp: for every slot with cell < 0,
// origin[id] = boxOrigin (hi null), or originOfKept[source_pick(hi, nKept, source_words(seed, id, epoch)[0])].  tag_field: for
// every i with 0 <= cell[i] < nDerived, field[parent * nOrigins + origin[id]] += 1 (parentOf null: the ids are parent ids already)
hipError_t tag_transfer(hipStream_t st, const int32_t* cell, const int64_t* gid, const uint8_t* origin, int64_t n, const uint32_t* mask,
                        int64_t nDerived, const uint8_t* sinkGroup, int32_t nOrigins, int32_t nSinks, unsigned long long* transfer);
hipError_t tag_stamp(hipStream_t st, const int32_t* cell, const int64_t* gid, uint8_t* origin, int64_t n, const uint32_t* hi,
                     int32_t nKept, const uint8_t* originOfKept, uint32_t seed, uint32_t epoch, int32_t boxOrigin);
hipError_t tag_field(hipStream_t st, const int32_t* cell, const int64_t* gid, const uint8_t* origin, int64_t n, const int32_t* parentOf,
                     int64_t nDerived, int64_t nParent, int32_t nOrigins, unsigned long long* field);
// routes (cpf_routes.hip), on age's birth[] and tags' origin[] and sinkGroup[].  route_absorb: sink_apply, and for every particle
// it absorbs the adds of tag_transfer and age_absorb and routeHist[(origin * nSinks + group) * nBins + min(age / binCycles,
// nBins - 1)] += 1.  route_field: for every i with 0 <= cell[i] < nDerived, field[2 * v] += age and field[2 * v + 1] += 1 with
// v = parent * nOrigins + origin[id] (parentOf null: the ids are parent ids already)
hipError_t route_absorb(hipStream_t st, int32_t* cell, const int64_t* gid, const uint32_t* birth, const uint8_t* origin, int64_t n,
                        const uint32_t* mask, int64_t nDerived, const uint8_t* sinkGroup, unsigned long long* absorbed, uint32_t now,
                        int32_t binCycles, int32_t nBins, int32_t nOrigins, int32_t nSinks, unsigned long long* hist,
                        unsigned long long* transfer, unsigned long long* routeHist);
hipError_t route_field(hipStream_t st, const int32_t* cell, const int64_t* gid, const uint32_t* birth, const uint8_t* origin, int64_t n,
                       const int32_t* parentOf, int64_t nDerived, int64_t nParent, int32_t nOrigins, uint32_t now,
                       unsigned long long* field);
// exposure (cpf_exposure.hip).  dose[id] (n doubles, id = gid[slot]; gid null: the slot), rate[d] one double per DERIVED cell.
// exposure_accumulate: dose[id] = dose[id] + scale * rate[cell[i]] for every i with 0 <= cell[i] < nDerived and a rate that is
// not zero.  exposure_absorb: reads only; hist[(origin * nSinks + group) * nBins + exposure_bin(dose[id], invWidth, nBins)] += 1
// for every i that sink_apply would absorb (cpf_exposure_bins.h; origin and sinkGroup both null: no tagging, origin and group 0;
// nOrigins * nSinks * nBins <= 4096).  exposure_stamp: dose[id] = +0.0 for every slot with cell < 0
hipError_t exposure_accumulate(hipStream_t st, const int32_t* cell, const int64_t* gid, const double* rate, double* dose, int64_t n,
                               int64_t nDerived, double scale);
hipError_t exposure_absorb(hipStream_t st, const int32_t* cell, const int64_t* gid, const double* dose, const uint8_t* origin, int64_t n,
                           const uint32_t* mask, int64_t nDerived, const uint8_t* sinkGroup, double invWidth, int32_t nBins,
                           int32_t nOrigins, int32_t nSinks, unsigned long long* hist);
hipError_t exposure_stamp(hipStream_t st, const int32_t* cell, const int64_t* gid, double* dose, int64_t n);
// zones (cpf_zones.hip).  last[id] (n bytes, id = gid[slot]; gid null: the slot) is the zone particle id was in at the last sample,
// 0xFF: none; zoneOf[d] the zone of DERIVED cell d, below nZones; flow[nZones + 1][nZones + 1], row and column nZones: outside.
// zone_sample: for every i with 0 <= cell[i] < nDerived, flow[last[id]][zoneOf[cell[i]]] += 1 and last[id] = that zone where it
// differs.  zone_leave: reads only; flow[last[id]][nZones] += 1 for every i that sink_apply would absorb.  zone_stamp:
// last[id] = 0xFF for every slot with cell < 0.  1 <= nZones <= 63
hipError_t zone_sample(hipStream_t st, const int32_t* cell, const int64_t* gid, const uint8_t* zoneOf, uint8_t* last, int64_t n,
                       int64_t nDerived, int32_t nZones, unsigned long long* flow);
hipError_t zone_leave(hipStream_t st, const int32_t* cell, const int64_t* gid, const uint8_t* last, int64_t n, const uint32_t* mask,
                      int64_t nDerived, int32_t nZones, unsigned long long* flow);
hipError_t zone_stamp(hipStream_t st, const int32_t* cell, const int64_t* gid, uint8_t* last, int64_t n);
// sink log (cpf_sinklog.hip).  Reads only, but for the cursor and the records: for every i that sink_apply would absorb, one
// cpf_sink_record at rec[k], k the index a returning add on *cursor reserved, unless k >= capacity.  The tables by id (birth,
// origin, dose, last: n entries, id = gid[slot]; gid null: the slot) and by DERIVED cell (sinkGroup, parentOf) are nullable:
// null is "that group is off" (parentOf: no cell decomposed), and the record's field takes its off value (include/cpf.h).
struct SinkLogView {
    const double *x, *y, *z;
    const int32_t* cell;
    const int64_t* gid;
    const uint32_t* birth;
    const uint8_t* origin;
    const double* dose;
    const uint8_t* last;
    const uint8_t* sinkGroup;
    const int32_t* parentOf;
    const uint32_t* mask;
    unsigned long long* cursor;
    cpf_sink_record* rec;                   // 16-byte aligned
    int64_t n, capacity;
    uint32_t now, apply, fields;
};
hipError_t sink_log(hipStream_t st, const SinkLogView& v, int64_t nDerived);
hipError_t unpack_arrivals(hipStream_t st, double* x, double* y, double* z, int32_t* cell, int64_t* gid,
                           int64_t nStay, const double* recvbuf, int64_t nRecv);
// output of a sharded cloud (cpf_shard_gather): records of kOutputDoubles doubles = x, y, z, cell, gid, vx, vy, vz
constexpr int kOutputDoubles = 8;
hipError_t pack_output(hipStream_t st, const double* x, const double* y, const double* z, const int32_t* cell,
                       const int64_t* gid, const double* vel3, double* rec, int64_t n);
hipError_t scatter_output(hipStream_t st, const double* rec, int64_t nRec, int64_t nGlobal, double* xyzw, int32_t* cellOut,
                          double* velOut, unsigned long long* bad);
hipError_t sum_rows(hipStream_t st, const double* rows, int nRows, size_t count, double* out);

}  // namespace cpf
