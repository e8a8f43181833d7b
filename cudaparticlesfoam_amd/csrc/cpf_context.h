// What a context is made of, for the two translation units that define its entry points: cpf_api.cpp (context, mesh, cloud,
// step, sort, recycling, output) and cpf_ledger.cpp (the six tracer groups).  Everybody else goes through the accessors of
// cpf_internal.h.
#pragma once
#include <hip/hip_runtime.h>

#include <condition_variable>
#include <mutex>
#include <string>
#include <thread>
#include <utility>
#include <vector>

#include "cpf.h"
#include "cpf_device.h"
#include "cpf_internal.h"
#include "cpf_own.h"

// (device-scope release is all a time stamp needs; measured against the default flags: no difference)
#ifndef CPF_TIMING_EVENT_FLAGS
#define CPF_TIMING_EVENT_FLAGS hipEventReleaseToDevice
#endif

// (private to the library: nothing declared here is one of its dynamic symbols, but for cpf_context itself)
#pragma GCC visibility push(hidden)
namespace cpf { namespace state {
using cpf::DevBuf; using cpf::Event; using cpf::PinnedBuf;

// What the context owns, grouped by lifetime: each group goes away as a whole -- assigned over with an empty one, or with the
// context.  The members are owners (cpf_own.h): nothing here is freed by hand.

// Flux table (cpf_source_follow; cpf_inflow.hip): what a refresh of the source table needs, allocated once.  It belongs to the
// source table it was made for: a new table and a new mesh each replace it with an empty one.
struct SourceFollow {
    bool on = false;
    double depthScale = 0.0;
    DevBuf<double> area;                    // [sourceKept] len / 2 of every kept record
    DevBuf<int32_t> owner;                  // [sourceKept] its owner cell, as the id the device's U is indexed by (a DERIVED cell)
    DevBuf<double> w;                       // [2][sourceKept] scratch of the four-launch path: the weights, the depths
    DevBuf<unsigned long long> sums;        // [2][inflow_blocks(sourceKept)] ... the tiles' sums, their offsets
    DevBuf<unsigned long long> slots;       // [4] wmax's bits, Q_last, refreshes skipped for zero inflow, spare
    int64_t refreshes = 0;                  // refreshes put on the stream since cpf_source_follow
};

// The mesh: the host tables and every device table made from them.  Replaced by cpf_set_mesh.
struct Mesh {
    bool have = false, haveU = false;
    cpf::HostTables host;
    DevBuf<int32_t> cellOff, nbr, groupOff, groupNbr;
    DevBuf<double4> planes;
    DevBuf<double4> U;
    DevBuf<double> U3;          // staging for host uploads
    DevBuf<double> boxRec;      // 128-byte box records (meshes of axis-aligned boxes with records; cpf_walk.h "box records")
    DevBuf<double4> cellRec;    // packed per-cell records (all-hex meshes; mixed meshes: cpf_walk.h "cell records")
    int64_t nSecondRecords = 0; // second records (cells with 7..12 slots), behind the nCells first ones
    DevBuf<float> cellBox;      // per-cell boxes for the sort key
    DevBuf<int32_t> curveRank;  // per-cell rank along the Morton curve: the sort's major key for sparse clouds ("sort_curve")
    DevBuf<int32_t> binOff, binCells;
    size_t bytes = 0;           // of the device tables (cpf_mesh_info)
    // warped / concave cells (cpf_mesh.cpp: measure_mesh, derive_mesh; DESIGN.md "Warped cells")
    cpf_mesh_quality quality{};         // of the mesh as the caller gave it
    int64_t nParent = 0;                // cells of the mesh as given: == host.nCells unless cells were decomposed
    std::vector<int32_t> first;         // [nParent+1] derived cells of parent c: first[c] .. first[c+1] (decomposed meshes only)
    DevBuf<int32_t> parentOf;           // [host.nCells] parent of every derived cell; null: no cell decomposed
    DevBuf<double> Uparent;             // [nParent][3] staging of cpf_set_velocity on a decomposed mesh
    std::vector<double> volume;         // [nParent] OpenFOAM's cell volumes of the mesh as given (cpf_get_cell_volumes)
    // per-cell occupancy (cpf_occupancy_sample*; cpf_occupancy.hip): it belongs to the mesh and goes with it
    DevBuf<unsigned long long> occupancy;   // [nParent] accumulated counts; null until the first sample
    int64_t occupancySamples = 0;           // samples added since the last reset
    // recycling (cpf_set_sink_cells; cpf_recycle.hip): the sink set belongs to the mesh and goes with it
    DevBuf<uint32_t> sinkMask;              // one bit per DERIVED cell, ceil(host.nCells / 32) words; null: no sink set
    // patch source (cpf_set_source_triangles; cpf_inlet.hip): it belongs to the mesh too
    DevBuf<double> sourceRec;               // [sourceKept][16] triangle records; null: no source
    DevBuf<uint32_t> sourceHi;              // [sourceKept] bounds, padded with 0xFFFFFFFF to a multiple of 4 entries
    int64_t sourceKept = 0;
    std::vector<double> sourceRecHost;      // the table as built (cpf_get_source_table)
    std::vector<uint32_t> sourceHiHost;
    SourceFollow follow;                    // the table follows U (cpf_source_follow): hi and column 13 live on the device then
};

// "VertexVelocity" advect only: the tet decomposition and one velocity per tet-mesh vertex.  It belongs to the mesh it was made
// for (cpf_set_tets checks it against that mesh's cell count): a new mesh starts without one.  Built by cpf_set_tets into a
// local and moved in whole, so nTets, tetsPerCell and the cone pair never describe tables that do not exist.
struct TetField {
    DevBuf<double> pos; DevBuf<int32_t> tets; DevBuf<double> vel;
    int64_t nVerts = 0, nTets = 0; int tetsPerCell = 0; bool haveVel = false;
    DevBuf<double> cone;        // cone-locate tet records (cpf_walk.h, VertexField), if the decomposition admits them
    DevBuf<double> apex;        // ... and the cells' apexes: both or neither
    std::string coneWhy;        // why the tables were not built (cpf_step_kernel_name says so)
};

struct CloudArrays {
    DevBuf<double> x, y, z;
    DevBuf<int32_t> cell;
    DevBuf<int64_t> gid;
    hipError_t alloc(size_t c) {                // (stops at the first failure)
        hipError_t e;
        (void)((e = x.alloc(c)) || (e = y.alloc(c)) || (e = z.alloc(c)) || (e = cell.alloc(c)) || (e = gid.alloc(c)));
        return e;
    }
};
// The context's own cloud.  Replaced by cpf_alloc_particles.
struct Cloud {
    int64_t cap = 0, n = 0;
    CloudArrays cur;
    // second set of x, y, z, cell, gid: the sort writes the reordered cloud there and the sets swap roles (no copy back);
    // allocated by the first sort, all five or none
    CloudArrays spare;
    DevBuf<double> vel;
    bool located = false;
    // z of the cloud is a fixed point of the flat cycle (CPF_STEP_Z_SETTLED): set behind a flat launch that streamed z, cleared
    // by everything else that writes x, y, z or cell -- except a sort, which only permutes
    bool zSettled = false;
    uint32_t respawnEpoch = 0;  // cpf_respawn_box calls on this cloud so far: the epoch of the next one's positions
};

// ---- the tracer ledger: six opt-in groups of the context's own cloud.  Their entry points, and the one statement of which group
// falls with which, are in cpf_ledger.cpp.

// Tracer age (cpf_age_*; cpf_age.hip).  The stamps belong to a cloud, the field to a mesh: a new cloud and a new mesh each replace
// the group with an empty one.
struct Age {
    bool on = false;
    int32_t binCycles = 1, nBins = 0;
    DevBuf<uint32_t> birth;                 // [cloud.n] by particle id: the cycle counter when the particle last became live
    DevBuf<unsigned long long> hist;        // [nBins] absorptions by age / binCycles, the last bin open-ended
    DevBuf<unsigned long long> field;       // [nParent][2] = age sum, count of the samples since the last reset
    int64_t samples = 0;
};

// Tracer tags (cpf_tag_*; cpf_tags.hip).  The origins belong to a cloud, the groups and the field to a mesh: a new cloud and a new
// mesh each replace the group with an empty one.
struct Tags {
    bool on = false;
    int32_t nOrigins = 1, nSinks = 1, boxOrigin = 0;
    DevBuf<uint8_t> origin;                 // [cloud.n] by particle id: the origin of the respawn that last made the particle live
    DevBuf<uint8_t> sinkGroup;              // [host.nCells] the group of every DERIVED cell (read for cells of the sink mask only)
    DevBuf<uint8_t> originOfKept;           // [sourceKept] the origin of every kept record of the source table; null: no source
    DevBuf<unsigned long long> transfer;    // [nOrigins][nSinks] absorptions (room for 16 x 16: cpf_tag_enable's limit)
    DevBuf<unsigned long long> field;       // [nParent][nOrigins] counts of the samples since the last reset
    int64_t samples = 0;
};

// Routes (cpf_route_*; cpf_routes.hip): tables sized by age's nBins and tags' nOrigins, nSinks, so the group lives only while both
// are on and is replaced by an empty one with either of them.
struct Routes {
    bool on = false;
    DevBuf<unsigned long long> hist;        // [nOrigins][nSinks][nBins] absorptions by route and age / binCycles
    DevBuf<unsigned long long> field;       // [nParent][nOrigins][2] = age sum, count of the samples since the last reset
    int64_t samples = 0;
};

// Exposure (cpf_exposure_*; cpf_exposure.hip).  The doses belong to a cloud, the rates to a mesh, the histogram's shape to
// tagging: a new cloud, a new mesh and tagging going on or off each replace the group with an empty one.
struct Exposure {
    bool on = false;
    double binWidth = 0.0, invWidth = 0.0;  // invWidth = 1.0 / binWidth, computed once (cpf_exposure_bins.h)
    int32_t nBins = 0, nOrigins = 1, nSinks = 1;
    bool tagged = false;                    // tagging was on at enable time: origin and sink group are read, else both are 0
    DevBuf<double> dose;                    // [cloud.n] by particle id: the sum since the particle last became live
    DevBuf<double> rate;                    // [host.nCells] per DERIVED cell: the caller's field expanded through `first`
    DevBuf<unsigned long long> hist;        // [nOrigins][nSinks][nBins] absorptions by origin, sink group and dose bin
};

// Zones (cpf_zone_*; cpf_zones.hip).  The last zones belong to a cloud, the map to a mesh: a new cloud and a new mesh each replace
// the group with an empty one.  Age, tags, routes and exposure know nothing of it, nor it of them.
struct Zones {
    bool on = false;
    int32_t nZones = 0;
    DevBuf<uint8_t> zoneOf;                 // [host.nCells] per DERIVED cell: the caller's map expanded through `first`
    DevBuf<uint8_t> last;                   // [cloud.n] by particle id: the zone at the last sample, 0xFF: none
    DevBuf<unsigned long long> flow;        // [nZones + 1][nZones + 1] transitions from sample to sample; index nZones: outside
    int64_t samples = 0;
};

// Sink log (cpf_sink_log_*; cpf_sinklog.hip).  The records speak of a cloud and a mesh: a new cloud and a new mesh each replace
// the group with an empty one.  The five groups above know nothing of it; it reads their tables at an apply, whichever of them are
// on then.
struct SinkLog {
    bool on = false;
    int64_t capacity = 0;
    uint32_t apply = 0;                     // logged applies since enable: the next one's index
    DevBuf<cpf_sink_record> rec;            // [capacity]
    DevBuf<unsigned long long> cursor;      // [1] absorbed particles since enable or the last clear, stored or not
};

// asynchronous output (cpf_write_vtu_async): one frame in flight.  Lives as long as the context.
struct FrameWriter {
    std::thread thread;
    bool live = false;
    int status = CPF_OK;
    // the frame's snapshot: packed in particle-id order on the compute stream into `snapDev`, copied to pinned host memory on
    // `io` behind an event, read by the worker thread only -- the step loop's stream never waits for PCIe (round 6)
    DevBuf<char> snapDev;
    PinnedBuf<char> snapHost;
    size_t snapBytes = 0;
    cpf::Stream io;
    Event evSnap, evCopied;
    double ke = 0.0;                            // of the frame the worker wrote last (valid after its join)
    std::mutex keMutex; std::condition_variable keCv; bool keReady = false;
};

// cpf_timing_*: event pairs round step launches.  Lives as long as the context.
struct Timing {
    int stride = 1;                             // "timing_stride": bracket every k-th step launch only
    uint64_t launch = 0;
    bool on = false;
    std::vector<std::pair<Event, Event>> recorded;
    std::vector<Event> pool;
    hipError_t take(Event& ev) {
        if (pool.empty()) return ev.create(CPF_TIMING_EVENT_FLAGS);
        ev = std::move(pool.back()); pool.pop_back();
        return hipSuccess;
    }
    void give_back(Event& ev) { if (ev) pool.push_back(std::move(ev)); }
    // sums the recorded pairs and hands their events back, from the oldest on: all of them (the caller has synchronised), or,
    // polling, those whose end has been reached -- launches complete in stream order
    hipError_t drain(bool poll, int64_t* launches, double* total_ms) {
        double tot = 0.0; size_t done = 0; hipError_t e = hipSuccess;
        for (; done < recorded.size(); ++done) {
            auto& p = recorded[done];
            if (poll && (e = hipEventQuery(p.second)) != hipSuccess) break;
            float ms = 0.f;
            if ((e = hipEventElapsedTime(&ms, p.first, p.second)) != hipSuccess) break;
            tot += (double)ms;
            give_back(p.first); give_back(p.second);
        }
        recorded.erase(recorded.begin(), recorded.begin() + (std::ptrdiff_t)done);
        if (e != hipSuccess && e != hipErrorNotReady) return e;
        *launches = (int64_t)done;
        *total_ms = tot;
        return hipSuccess;
    }
};
}}  // namespace cpf::state
#pragma GCC visibility pop

// Members are destroyed in reverse order: everything below is released before `ownStream` is.
struct cpf_context {
    int device = 0;
    cpf::Stream ownStream;
    hipStream_t stream = nullptr;               // ownStream, or the caller's (cpf_set_stream)
    mutable std::string err;
    // ---- options: they survive a new mesh and a new cloud
    bool zFold = true;               // "z_fold": mirror the kicked end point about the planes of a one-cell-thick mesh before the walk
    bool boxRecords = true;         // "box_records": 0 = never use them (diagnostics; bit-identical either way)
    int sortMethod = 2;             // "sort_method": the (key, index) sort: 2 = this library's radix sort (cpf_sort.hip, rt_sort_pairs), 0 = hipcub's;
                                    // the same order either way
    int sortCurve = -1;             // "sort_curve": -1 = Morton rank when the cloud has fewer than 8 particles per cell, 0 = cell id, 1 = Morton rank
    int sortInterval = 50;                      // "sort_interval": cpf_step re-sorts the owned cloud by cell every N cycles
    bool stats = false;                         // "stats": per-launch counters (steps, cells visited, reflections, lost)
    int stepVariant = -1;                       // cpf_set_option("step_variant"), see include/cpf.h: -1 = choose per launch
    bool vtuBinary = false;                     // cpf_set_option("vtu_binary"): frames with raw appended arrays instead of the reference's ASCII
    bool mixedRecords = true;                   // cpf_set_option("mixed_records"): build cell records for hex-dominant meshes too (before cpf_set_mesh)
    double nonplanarTol = cpf::kNonPlanarTolDefault;    // "nonplanar_tol" (before cpf_set_mesh)
    bool splitNonplanar = true;                         // "split_nonplanar" (before cpf_set_mesh): 0 = one plane per face everywhere
    bool vertexFast = true;                     // cpf_set_option("vertex_fast")
    uint32_t seed = 1591593751u;                // cuda/particles.cu:544
    // ---- the groups
    cpf::state::Mesh mesh; cpf::state::TetField tet; cpf::state::Cloud cloud;
    cpf::state::Age age; cpf::state::Tags tags; cpf::state::Routes routes; cpf::state::Exposure exposure; cpf::state::Zones zones;
    cpf::state::SinkLog sinkLog;
    cpf::state::FrameWriter frame; cpf::state::Timing timing;
    // ---- what lives as long as the context
    cpf::DevBuf<char> scratch;
    size_t scratchBytes = 0;
    // [kCounterSlots][4] = steps, hops, reflections, lost, sharded by block id (one hot word would
    // serialise every block of every launch on a single L2 atomic unit), then 4 scratch words
    cpf::DevBuf<unsigned long long> counters;
    cpf::DevBuf<unsigned long long> recycleCounts;   // [0] absorbed, [1] drawn, [2] placed (cpf_get_recycle_counts); allocated at first use
    cpf::DevBuf<unsigned long long> occupied;        // [0] occupied cells, [1] live particles of the last sort (device) ...
    cpf::PinnedBuf<unsigned long long> h_occupied;   // ... and their pinned host copy (StreamState::occupiedHost)
    cpf::Event evFieldFlag;                          // recorded behind the read-back of "the field has a z component" (cpf_set_velocity_dev)
    bool fieldFlagPending = false;              // ... and not yet seen complete: until then the field counts as having one
    // "a live particle's z is not finite", written by a flat launch that streams z (StreamState::zBad, pinned); evZBad is recorded
    // behind such a launch, and while zBadPending the launch's verdict has not been read: the first launch that would leave z
    // alone waits for it -- one wait per unsettling event, no pass over the cloud
    cpf::PinnedBuf<unsigned> h_zBad;
    cpf::Event evZBad;
    bool zBadPending = false;
    cpf::DevBuf<unsigned> grab;                      // the streaming kernel's chunk counters ...
    cpf::DevBuf<double> hitSpill;                    // ... and the overflow area of its hit pool: StreamState views them
    cpf::StreamState streamState;               // chunk counter + tuning of the streaming step kernel
    uint32_t stepCounter = 0;
    uint32_t lastSortStep = 0;
    int64_t lastStepN = -1;                     // particle count of the most recent step launch (cpf_step_kernel_name)
    int lastStepCycles = 1;                     // ... and its cycles per launch
    bool lastStepZSettled = false;              // what the most recent cpf_step_dev left behind on ITS arrays (cpf_shard.cpp)
};

#pragma GCC visibility push(hidden)
namespace cpf {
// stores `msg` as the context's last error -- or, without a context, as cpf_create's -- and returns `code`
int fail(const cpf_context* ctx, int code, const std::string& msg);

#define CPF_HIP(ctx, call)                                                                              \
    do {                                                                                                \
        hipError_t e__ = (call);                                                                        \
        if (e__ != hipSuccess)                                                                          \
            return cpf::fail(ctx, CPF_ERR_HIP, std::string(#call) + ": " + hipGetErrorString(e__));     \
    } while (0)

#define CPF_REQUIRE(ctx, cond, code, msg) \
    do { if (!(cond)) return cpf::fail(ctx, code, msg); } while (0)

// ---- defined in cpf_api.cpp
int ensureScratch(cpf_context* ctx, size_t bytes);      // at least `bytes` of ctx->scratch (growing it waits for the stream)
MeshView meshView(const cpf_context* ctx);
GridView gridView(const cpf_context* ctx);

// ---- defined in cpf_ledger.cpp: where the sink, the respawns, a new mesh and a new cloud meet the six groups
// cpf_sink_apply's passes of the groups that are on, in their order: log, dose, zone-leave, then route, or tag followed by age.
// *marked: a pass (route's, age's) has marked and counted the absorbed already; else the caller's plain sink pass is still to run.
int ledger_sink_passes(cpf_context* ctx, bool* marked);
// A respawn of the context's own cloud is about to run: every candidate is stamped in each group that is on -- with the origin of
// the source triangle this call's epoch picks for it (fromSource), or with the box's.
int ledger_respawn_stamps(cpf_context* ctx, bool fromSource);
// A new mesh, or new arrays for the cloud: all six groups become empty.  The caller has waited for the stream.
void ledger_clear(cpf_context* ctx);
// New particles in the cloud's arrays: age, tags (and so routes and exposure), zones and the log go off; the stream is waited
// for only where one of them was on.
int ledger_new_cloud(cpf_context* ctx);
}  // namespace cpf
#pragma GCC visibility pop

// ctx->recycleCounts, zeroed at first use (cpf_api.cpp).  Not part of include/cpf.h, but one of the library's dynamic symbols since
// the recycling entries came, under this name: it stays one, so that the list of exports is what it was.
extern "C" int ensureRecycleCounts(cpf_context* ctx);
