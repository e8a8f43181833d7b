// C-ABI layer of libcudaParticleAdvection.so: context, device memory, call-order checks, errors.
// The entry points declared in include/cpf.h are defined here, but for the tracer ledger's (cpf_ledger.cpp); kernels live in
// cpf_kernels.hip, cpf_sort.hip and cpf_handoff.hip, the host-side mesh ingest in cpf_mesh.cpp.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <limits>
#include <condition_variable>
#include <mutex>
#include <string>
#include <thread>
#include <utility>
#include <vector>

#include "cpf.h"
#include "cpf_context.h"   // cpf_context and its groups, fail, CPF_HIP, CPF_REQUIRE
#include "cpf_device.h"
#include "cpf_inflow.h"    // the flux table's arithmetic (cpf_source_flux_host)
#include "cpf_internal.h"
#include "cpf_own.h"
#include "cpf_philox.h"    // respawn_position (cpf_respawn_positions_host)
#include "cpf_walk.h"      // VertexField

using namespace cpf::state;
using cpf::ensureScratch; using cpf::fail; using cpf::gridView; using cpf::meshView;

namespace {

std::string g_createError = "";
std::mutex g_mutex;

// Contexts with an output frame still being written.  A host that never calls cpf_destroy (the reference's
// solvers simply return from main) must not lose its last frame: the registry's destructor runs at exit and
// joins the workers.
struct WriterRegistry {
    std::vector<cpf_context*> live;
    ~WriterRegistry();
} g_writers;

// What kind of mesh the tables describe: all-hex, and for any other mesh whose cells have records (`records`) which kinds of
// record can turn up -- 0: none, 1: padded ones only, 2: two-record and / or header cells too (cpf_walk.h "cell records")
bool isAllHex(const cpf::HostTables& t) { return t.minCellFaces == 6 && t.maxCellFaces == 6 && t.nGroups() == 0; }
int mixedKind(const cpf::HostTables& t, bool records) { return (records && !isAllHex(t)) ? (t.nBigCells > 0 ? 2 : 1) : 0; }
// a mesh that is not all-hex gets records where at most a quarter of its cells have more than TWELVE slots ("mixed_records")
bool mixedRecordsFit(const cpf::HostTables& t) { return t.nHugeCells * 4 <= t.nCells; }
}  // namespace

namespace cpf {     // (declared in cpf_context.h)
int fail(const cpf_context* ctx, int code, const std::string& msg) {
    if (ctx) ctx->err = msg;
    else { std::lock_guard<std::mutex> lk(g_mutex); g_createError = msg; }
    return code;
}

cpf::MeshView meshView(const cpf_context* c) {
    cpf::MeshView m;
    m.cellOff = c->mesh.cellOff; m.planes = c->mesh.planes; m.nbr = c->mesh.nbr; m.U = c->mesh.U;
    m.groupOff = c->mesh.groupOff; m.groupNbr = c->mesh.groupNbr;
    m.cellRec = c->mesh.cellRec;
    m.boxRec = c->boxRecords ? reinterpret_cast<const double4*>(c->mesh.boxRec.get()) : nullptr;
    m.nCells = (int32_t)c->mesh.host.nCells;
    m.allHex = isAllHex(c->mesh.host) ? 1 : 0;
    m.zPairLast = c->mesh.host.zPairLast ? 1 : 0;
    m.zThin = (c->mesh.host.zThin && c->zFold) ? 1 : 0;
    m.zSide0 = c->mesh.host.zSide0 ? 1 : 0;
    m.mixed = mixedKind(c->mesh.host, c->mesh.cellRec != nullptr);
    return m;
}
cpf::GridView gridView(const cpf_context* c) {
    cpf::GridView g;
    for (int k = 0; k < 3; ++k) {
        g.origin[k] = c->mesh.host.origin[k]; g.invBin[k] = c->mesh.host.invBin[k];
        g.lo[k] = c->mesh.host.lo[k]; g.hi[k] = c->mesh.host.hi[k]; g.dims[k] = c->mesh.host.dims[k];
    }
    g.binOff = c->mesh.binOff; g.binCells = c->mesh.binCells;
    return g;
}

int ensureScratch(cpf_context* ctx, size_t bytes) {
    if (bytes <= ctx->scratchBytes) return CPF_OK;
    CPF_HIP(ctx, hipStreamSynchronize(ctx->stream));
    ctx->scratchBytes = 0;
    CPF_HIP(ctx, ctx->scratch.alloc(bytes));
    ctx->scratchBytes = bytes;
    return CPF_OK;
}
}  // namespace cpf

extern "C" int ensureRecycleCounts(cpf_context* ctx) {
    if (ctx->recycleCounts) return CPF_OK;
    DevBuf<unsigned long long> c;
    CPF_HIP(ctx, c.alloc(4));
    CPF_HIP(ctx, hipMemsetAsync(c, 0, 4 * 8, ctx->stream));
    ctx->recycleCounts = std::move(c);
    return CPF_OK;
}

namespace {
int sortEndBit(const cpf_context* ctx) {
    int bits = 1;
    while (((int64_t)1 << bits) < ctx->mesh.host.nCells + 2) ++bits;   // the all-ones key of lost/frozen sorts last
    return std::min(bits + ctx->mesh.host.subBits[0] + ctx->mesh.host.subBits[1] + ctx->mesh.host.subBits[2], 32);  // + sub-cell bits
}

cpf_mesh_quality toQuality(const cpf::MeshQuality& q, int64_t nDerived) {
    cpf_mesh_quality r{};
    r.maxNonPlanarity = q.maxEta; r.worstFace = q.worstFace;
    r.maxNonConvexity = q.maxXi; r.worstCell = q.worstCell;
    r.nCells = q.nCells; r.nFlaggedCells = q.nFlagged; r.nBadCells = q.nBad; r.nDerivedCells = nDerived;
    r.tol = q.tol;
    return r;
}

template <typename Label>
int setMeshImpl(cpf_context* ctx, const double* points, int64_t nPoints, const Label* faceOffsets,
                const Label* faceVerts, int64_t nFaces, const Label* owner, const Label* neighbour,
                int64_t nInternal, int64_t nCells) {
    CPF_REQUIRE(ctx, ctx, CPF_ERR_ARG, "null context");
    CPF_REQUIRE(ctx, points && faceOffsets && faceVerts && owner && (neighbour || nInternal == 0), CPF_ERR_ARG,
                "cpf_set_mesh: null array");
    // warped faces and concave cells: measured on every mesh; where some cell needs it (and "split_nonplanar" is on) the walk
    // runs on the derived mesh, those cells replaced by their fans of tets -- otherwise on the mesh as given, exactly as before
    cpf::MeshQuality q;
    std::string why = cpf::measure_mesh<Label>(points, nPoints, faceOffsets, faceVerts, nFaces, owner, neighbour, nInternal,
                                               nCells, ctx->nonplanarTol, q);
    if (!why.empty()) return fail(ctx, CPF_ERR_MESH, "cpf_set_mesh: " + why);
    bool derive = ctx->splitNonplanar && q.decompose();
    cpf::DerivedMesh dm;
    cpf::HostTables t;
    if (derive) {
        why = cpf::derive_mesh<Label>(points, nPoints, faceOffsets, faceVerts, nFaces, owner, neighbour, nInternal, nCells, q, dm);
        if (why.empty())
            why = cpf::build_tables<int64_t>(dm.points.data(), dm.nPoints, dm.faceOff.data(), dm.faceVerts.data(), dm.nFaces,
                                             dm.owner.data(), dm.neighbour.data(), dm.nInternal, dm.nCells, t);
        // a whole cell must see each face it shares with a decomposed cell as ONE slot (its triangles merged into a face
        // group): else a segment could leave it through the wrong triangle.  Where that fails, keep the one-plane model.
        for (int64_t c = 0; c < nCells && why.empty() && derive; ++c)
            if (dm.first[(size_t)c + 1] - dm.first[(size_t)c] == 1) {
                const int32_t d = dm.first[(size_t)c];
                if (t.cellOff[(size_t)d + 1] - t.cellOff[(size_t)d] > q.cellOff[(size_t)c + 1] - q.cellOff[(size_t)c]) derive = false;
            }
    }
    if (!derive) {
        why = cpf::build_tables<Label>(points, nPoints, faceOffsets, faceVerts, nFaces, owner, neighbour, nInternal, nCells, t);
    }
    if (!why.empty()) return fail(ctx, CPF_ERR_MESH, "cpf_set_mesh: " + why);
    CPF_HIP(ctx, hipSetDevice(ctx->device));
    CPF_HIP(ctx, hipStreamSynchronize(ctx->stream));
    ctx->mesh = Mesh{};
    ctx->tet = TetField{};
    cpf::ledger_clear(ctx);
    ctx->streamState.flatField = false;
    ctx->mesh.host = std::move(t);
    ctx->mesh.nParent = nCells;
    ctx->mesh.quality = toQuality(q, ctx->mesh.host.nCells);
    ctx->mesh.volume = std::move(q.volume);
    nCells = ctx->mesh.host.nCells;                         // from here on: the cells the walk runs on
    const cpf::HostTables& h = ctx->mesh.host;
    auto up = [&](auto& buf, const auto& src) -> hipError_t {      // (planes: four doubles of `src` per element of `buf`)
        const size_t bytes = src.size() * sizeof(src[0]);
        hipError_t e = buf.alloc(bytes / sizeof(*buf.get()));
        if (e != hipSuccess) return e;
        ctx->mesh.bytes += bytes;
        return hipMemcpy(buf, src.data(), bytes, hipMemcpyHostToDevice);
    };
    CPF_HIP(ctx, up(ctx->mesh.cellOff, h.cellOff));
    CPF_HIP(ctx, up(ctx->mesh.planes, h.planes));
    CPF_HIP(ctx, up(ctx->mesh.nbr, h.nbr));
    CPF_HIP(ctx, up(ctx->mesh.groupOff, h.groupOff));
    CPF_HIP(ctx, up(ctx->mesh.groupNbr, h.groupNbr));
    CPF_HIP(ctx, up(ctx->mesh.binOff, h.binOff));
    CPF_HIP(ctx, up(ctx->mesh.binCells, h.binCells));
    CPF_HIP(ctx, up(ctx->mesh.cellBox, h.cellBox));
    CPF_HIP(ctx, up(ctx->mesh.curveRank, h.curveRank));
    if (derive) {
        ctx->mesh.first = std::move(dm.first);
        CPF_HIP(ctx, up(ctx->mesh.parentOf, dm.parent));
        CPF_HIP(ctx, ctx->mesh.Uparent.alloc((size_t)ctx->mesh.nParent * 3));
        ctx->mesh.bytes += (size_t)ctx->mesh.nParent * 24;
    }
    CPF_HIP(ctx, ctx->mesh.U.alloc((size_t)nCells));
    CPF_HIP(ctx, ctx->mesh.U3.alloc((size_t)nCells * 3));
    CPF_HIP(ctx, hipMemset(ctx->mesh.U, 0, (size_t)nCells * sizeof(double4)));
    if (isAllHex(h)) {
        CPF_HIP(ctx, ctx->mesh.cellRec.alloc((size_t)nCells * 8));
        CPF_HIP(ctx, cpf::launch_build_cell_records(ctx->stream, ctx->mesh.planes, ctx->mesh.nbr, ctx->mesh.U, ctx->mesh.cellRec, nCells));
        CPF_HIP(ctx, hipStreamSynchronize(ctx->stream));
        ctx->mesh.bytes += (size_t)nCells * 256;
        if (!h.boxRec.empty()) CPF_HIP(ctx, up(ctx->mesh.boxRec, h.boxRec));
    } else if (mixedRecordsFit(h) && ctx->mixedRecords) {
        // not all-hex, but at most a quarter of the cells have more than TWELVE slots: records for the streaming kernel --
        // padded where a cell has fewer than six slots, a second record for slots 6..11 of a cell with 7..12 (true polyhedra
        // keep the LDS face test: two rounds per visit), a header record + CSR walk only beyond that (cpf_walk.h "cell
        // records").  Refinement interfaces need none of it: their split faces are face groups, one slot each.
        std::vector<int32_t> recB((size_t)nCells, -1);
        int64_t nSecond = 0;
        for (int64_t c = 0; c < nCells; ++c) {
            const int nf = ctx->mesh.host.cellOff[(size_t)c + 1] - ctx->mesh.host.cellOff[(size_t)c];
            if (nf > 6 && nf <= 12) recB[(size_t)c] = (int32_t)(nCells + nSecond++);
        }
        CPF_REQUIRE(ctx, nCells + nSecond < ((int64_t)1 << 31), CPF_ERR_MESH, "cpf_set_mesh: too many cell records");
        DevBuf<int32_t> d_recB;                                                 // (gone with this block on every path)
        hipError_t e = hipSuccess;
        if (nSecond > 0) e = up(d_recB, recB);
        if (e == hipSuccess) e = ctx->mesh.cellRec.alloc((size_t)(nCells + nSecond) * 8);
        if (e == hipSuccess) e = cpf::launch_build_cell_records_mixed(ctx->stream, ctx->mesh.cellOff, ctx->mesh.planes, ctx->mesh.nbr, ctx->mesh.U, d_recB,
                                                                      ctx->mesh.cellRec, nCells);
        if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
        CPF_HIP(ctx, e);
        ctx->mesh.nSecondRecords = nSecond;
        ctx->mesh.bytes += (size_t)(nCells + nSecond) * 256;
        // every cell an axis-aligned box although the mesh has face groups (2:1-refined boxes): box records too
        if (!h.boxRec.empty() && nSecond == 0) CPF_HIP(ctx, up(ctx->mesh.boxRec, h.boxRec));
    }
    ctx->mesh.bytes += (size_t)nCells * (sizeof(double4) + 24);
    ctx->mesh.have = true;
    ctx->cloud.located = false;
    ctx->cloud.zSettled = false;
    if (ctx->h_occupied) ctx->h_occupied[0] = ctx->h_occupied[1] = 0;      // (what the last sort counted belonged to the old mesh)
    return CPF_OK;
}

}  // namespace

namespace {
WriterRegistry::~WriterRegistry() {
    for (cpf_context* c : live)
        if (c->frame.live && c->frame.thread.joinable()) { c->frame.thread.join(); c->frame.live = false; }
}
}  // namespace

namespace cpf {
bool vtu_binary(const cpf_context* ctx) { return ctx && ctx->vtuBinary; }
bool context_derived(const cpf_context* ctx) { return ctx && ctx->mesh.parentOf != nullptr; }
void* context_stream(const cpf_context* ctx) { return (void*)ctx->stream; }
int context_device(const cpf_context* ctx) { return ctx->device; }
bool context_timing(const cpf_context* ctx) { return ctx->timing.on; }
int64_t context_cells(const cpf_context* ctx) { return ctx->mesh.have ? ctx->mesh.host.nCells : 0; }
bool context_step_settled_z(const cpf_context* ctx) { return ctx->lastStepZSettled; }
}  // namespace cpf

namespace {
// Is the tet decomposition of every cell a FAN about one apex that covers every direction exactly once?  (What the reference's
// fragment builds: apex = the cell centre, one tet per face triangle, src/initCuda.H:99-105.)  Then no two tets of a cell
// overlap, which is what makes the cone locate of the "VertexVelocity" advect exact (cpf_kernels.hip).  Checked per cell: every
// tet starts at the same vertex; all determinants have one sign and none is flat beyond a condition of 1e5 (weights then carry
// rounding errors below 1e-10, two orders inside the locate's margin); the base triangles form a closed oriented surface (every
// directed edge once, its reverse once); the solid angles the tets subtend at the apex (Van Oosterom-Strackee) add up to
// 4 pi -- a closed surface seen from its inner side everywhere that winds round the apex once projects one-to-one onto the
// sphere of directions, i.e. the cones do not overlap.
// Returns "" or the first defect.
std::string tetFanDefect(const double* pos, const int32_t* tets, int64_t nCells, int tetsPerCell) {
    auto P = [&](int32_t v, int k) { return pos[3 * (int64_t)v + k]; };
    const double fourPi = 12.566370614359172;
    std::vector<uint64_t> edges;
    for (int64_t c = 0; c < nCells; ++c) {
        const int32_t* t0 = tets + 4 * c * tetsPerCell;
        const int32_t apex = t0[0];
        double omega = 0.0;
        int sign = 0;
        for (int k = 0; k < tetsPerCell; ++k) {
            const int32_t* ix = t0 + 4 * k;
            if (ix[0] != apex) return "cell " + std::to_string(c) + ": its tets do not share their first vertex";
            double e[3][3], len[3];
            for (int j = 0; j < 3; ++j) {
                for (int q = 0; q < 3; ++q) e[j][q] = P(ix[j + 1], q) - P(apex, q);
                len[j] = std::sqrt(e[j][0] * e[j][0] + e[j][1] * e[j][1] + e[j][2] * e[j][2]);
            }
            const double det = e[0][0] * (e[1][1] * e[2][2] - e[1][2] * e[2][1]) - e[0][1] * (e[1][0] * e[2][2] - e[1][2] * e[2][0]) +
                               e[0][2] * (e[1][0] * e[2][1] - e[1][1] * e[2][0]);
            const double scale = len[0] * len[1] * len[2];
            if (!(std::fabs(det) * 1e5 > scale)) return "cell " + std::to_string(c) + ": a flat (or badly conditioned) tet";
            const int sg = det > 0 ? 1 : -1;
            if (sign == 0) sign = sg;
            else if (sg != sign) return "cell " + std::to_string(c) + ": tets of both orientations";
            auto dot = [&](int i, int j) { return e[i][0] * e[j][0] + e[i][1] * e[j][1] + e[i][2] * e[j][2]; };
            omega += 2.0 * std::atan2(std::fabs(det), scale + dot(0, 1) * len[2] + dot(0, 2) * len[1] + dot(1, 2) * len[0]);
        }
        if (std::fabs(omega - fourPi) > 1e-6) return "cell " + std::to_string(c) + ": the tets' solid angles at the apex do not add up to 4 pi";
        // the base triangles form a closed oriented surface: every directed edge once, its reverse once (a tet listed twice in
        // place of its mirror image keeps the angles' sum and is caught here)
        edges.clear();
        for (int k = 0; k < tetsPerCell; ++k) {
            const int32_t* ix = t0 + 4 * k;
            for (int j = 0; j < 3; ++j) edges.push_back(((uint64_t)(uint32_t)ix[1 + j] << 32) | (uint32_t)ix[1 + (j + 1) % 3]);
        }
        std::sort(edges.begin(), edges.end());
        for (size_t i = 0; i < edges.size(); ++i) {
            const uint64_t rev = (edges[i] << 32) | (edges[i] >> 32);
            if ((i > 0 && edges[i] == edges[i - 1]) || !std::binary_search(edges.begin(), edges.end(), rev))
                return "cell " + std::to_string(c) + ": the tets' base triangles do not form a closed surface";
        }
    }
    return "";
}

// U[nCells][3] (device) -> the padded field and the cell records; on a mesh that qualifies for the flat walk (cpf_walk.h) the
// kernel also notes whether any cell has a z component, and the note is read back behind it (8 bytes, asynchronous)
hipError_t layOutField(cpf_context* ctx, const double* dU3, int64_t nCells) {
    const bool ask = ctx->mesh.host.zSide0 && ctx->occupied && ctx->h_occupied;
    ctx->streamState.flatField = false;
    ctx->fieldFlagPending = false;
    hipError_t e = hipSuccess;
    if (ask) e = hipMemsetAsync(ctx->occupied + 2, 0, 8, ctx->stream);
    if (e == hipSuccess) e = cpf::launch_u3_to_u4(ctx->stream, dU3, ctx->mesh.U, nCells, ask ? ctx->occupied + 2 : nullptr);
    if (e == hipSuccess && ctx->mesh.cellRec) e = cpf::launch_update_record_velocity(ctx->stream, ctx->mesh.U, ctx->mesh.cellRec, ctx->mesh.boxRec, nCells);
    if (e == hipSuccess && ask) {
        e = hipMemcpyAsync(ctx->h_occupied + 2, ctx->occupied + 2, 8, hipMemcpyDeviceToHost, ctx->stream);
        if (e == hipSuccess) e = hipEventRecord(ctx->evFieldFlag, ctx->stream);
        ctx->fieldFlagPending = e == hipSuccess;
    }
    return e;
}
// The source table follows U (cpf_source_follow): one refresh on the stream from U[.][uStride] -- the array layOutField was given
// (uStride 3), or the padded field (uStride 4).  Nothing here waits, copies to the host or allocates.
hipError_t refreshSource(cpf_context* ctx, const double* dU, int uStride) {
    SourceFollow& f = ctx->mesh.follow;
    const cpf::InflowView v{ctx->mesh.sourceRec, ctx->mesh.sourceHi, (int32_t)ctx->mesh.sourceKept, f.depthScale,
                            f.area, f.owner, f.w, f.sums, f.slots};
    const hipError_t e = cpf::inflow_refresh(ctx->stream, v, dU, uStride);
    if (e == hipSuccess) ++f.refreshes;
    return e;
}
// Sub-cell resolve of cpf_set_particles on a decomposed mesh: parent cell c -> the lowest derived cell of first[c] .. first[c+1]
// whose every plane has the point within kTol on its inner side (the walk's face test, cpf_walk.h plane_dist), or else the one
// whose worst plane distance is smallest.  Negative codes pass through.
std::string resolveSubCells(const cpf_context* ctx, int64_t n, const double* xyz, const int32_t* cell, std::vector<int32_t>& out) {
    const cpf::HostTables& h = ctx->mesh.host;
    out.resize((size_t)n);
    for (int64_t i = 0; i < n; ++i) {
        const int32_t c = cell[i];
        if (c < 0) { out[(size_t)i] = c; continue; }
        if (c >= ctx->mesh.nParent) return "cell[" + std::to_string(i) + "] = " + std::to_string(c) + " is not a cell of the mesh";
        const double px = xyz[3 * i], py = xyz[3 * i + 1], pz = xyz[3 * i + 2];
        int32_t pick = ctx->mesh.first[(size_t)c];
        double pickWorst = HUGE_VAL;
        for (int32_t d = ctx->mesh.first[(size_t)c]; d < ctx->mesh.first[(size_t)c + 1]; ++d) {
            double worst = -HUGE_VAL;
            for (int32_t s = h.cellOff[(size_t)d]; s < h.cellOff[(size_t)d + 1]; ++s) {
                const double* pl = &h.planes[4 * (size_t)s];
                worst = std::max(worst, std::fma(-pl[2], pz, std::fma(-pl[1], py, std::fma(-pl[0], px, pl[3]))));
            }
            if (worst < cpf::kTol) { pick = d; break; }
            if (worst < pickWorst) { pickWorst = worst; pick = d; }
        }
        out[(size_t)i] = pick;
    }
    return std::string();
}
// the read-back is known to be complete (after a synchronise, or its event has been seen): take the note
void fieldFlagArrived(cpf_context* ctx) {
    if (!ctx->fieldFlagPending) return;
    ctx->streamState.flatField = ctx->h_occupied[2] == 0;
    ctx->fieldFlagPending = false;
}
// the verdict of the flat launch that streamed z last (cpf_context::h_zBad), waited for if it is still on its way: true = a live
// particle's z is not finite, and z is not settled
bool zBadArrived(cpf_context* ctx) {
    if (ctx->zBadPending) {
        (void)hipEventSynchronize(ctx->evZBad);
        ctx->zBadPending = false;
    }
    return *static_cast<volatile unsigned*>(ctx->h_zBad) != 0u;
}
void pollFieldFlag(cpf_context* ctx) {
    if (ctx->fieldFlagPending && hipEventQuery(ctx->evFieldFlag) == hipSuccess) fieldFlagArrived(ctx);
}
// how many of ids[0 .. n) are negative, read back (synchronises the stream); counted in the counters' scratch words
int countNegative(cpf_context* ctx, const int32_t* ids, int64_t n, int64_t* out) {
    unsigned long long* cnt = ctx->counters + cpf::kCounterSlots * 4;
    CPF_HIP(ctx, hipMemsetAsync(cnt, 0, 8, ctx->stream));
    CPF_HIP(ctx, cpf::launch_count_negative(ctx->stream, ids, n, cnt));
    unsigned long long h = 0;
    CPF_HIP(ctx, hipMemcpyAsync(&h, cnt, 8, hipMemcpyDeviceToHost, ctx->stream));
    CPF_HIP(ctx, hipStreamSynchronize(ctx->stream));
    *out = (int64_t)h;
    return CPF_OK;
}
// cpf::launch_pack_by_gid's three outputs for n particles in one buffer: xyzw[n][4] at 0, cell[n] at offC, vel[n][4] at offV
struct PackLayout {
    size_t offC, offV, bytes;
    static size_t al(size_t b) { return (b + 255) & ~(size_t)255; }
    explicit PackLayout(size_t n) : offC(al(n * 32)), offV(offC + al(n * 4)), bytes(offV + al(n * 32)) {}
};
}  // namespace

extern "C" {

int cpf_abi_version(void) { return CPF_ABI_VERSION; }

int cpf_create(int device, cpf_context** out) {
    if (!out) return fail(nullptr, CPF_ERR_ARG, "cpf_create: out is null");
    *out = nullptr;
    int count = 0;
    hipError_t e = hipGetDeviceCount(&count);
    if (e != hipSuccess || count <= 0)
        return fail(nullptr, CPF_ERR_HIP,
                    std::string("cpf_create: no HIP device available (") + hipGetErrorString(e) + ")");
    if (device < 0 || device >= count) return fail(nullptr, CPF_ERR_ARG, "cpf_create: device index out of range");
    e = hipSetDevice(device);
    if (e != hipSuccess) return fail(nullptr, CPF_ERR_HIP, std::string("hipSetDevice: ") + hipGetErrorString(e));
    cpf_context* ctx = new (std::nothrow) cpf_context();
    if (!ctx) return fail(nullptr, CPF_ERR_NOMEM, "cpf_create: out of host memory");
    ctx->device = device;
    e = ctx->ownStream.create(hipStreamNonBlocking);
    if (e == hipSuccess) e = ctx->counters.alloc(cpf::kCounterSlots * 4 + 4);
    if (e == hipSuccess) e = hipMemset(ctx->counters, 0, (cpf::kCounterSlots * 4 + 4) * sizeof(unsigned long long));
    // ([2]: "the velocity field has a z component", written by the kernel that lays the field out -- the flat walk)
    if (e == hipSuccess) e = ctx->occupied.alloc(4);
    if (e == hipSuccess) e = ctx->h_occupied.alloc(4);
    if (e == hipSuccess) { ctx->h_occupied[0] = ctx->h_occupied[1] = 0; ctx->h_occupied[2] = 1; ctx->streamState.occupiedHost = ctx->h_occupied; }
    if (e == hipSuccess) e = ctx->evFieldFlag.create(hipEventDisableTiming);
    if (e == hipSuccess) e = ctx->h_zBad.alloc(16);
    if (e == hipSuccess) { *ctx->h_zBad = 0u; ctx->streamState.zBad = ctx->h_zBad; }
    if (e == hipSuccess) e = ctx->evZBad.create(hipEventDisableTiming);
    if (e == hipSuccess) e = ctx->grab.alloc(cpf::kStreamGrabBytes / sizeof(unsigned));
    if (e == hipSuccess) e = hipMemset(ctx->grab, 0, cpf::kStreamGrabBytes);
    if (e == hipSuccess) ctx->streamState.d_grab = ctx->grab;
    if (e == hipSuccess) {
        int cus = 0;
        e = hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device);
        if (e == hipSuccess && cus > 0) ctx->streamState.numCU = cus;
    }
    if (e == hipSuccess) {
        // overflow area of the streaming kernel's per-wave pool of wall hit points: 1.5 KB per wave slot the chip can hold
        ctx->streamState.hitSpillWaves = 32 * ctx->streamState.numCU;
        e = ctx->hitSpill.alloc((size_t)ctx->streamState.hitSpillWaves * cpf::kStreamHitSpillDoubles);
        if (e == hipSuccess) ctx->streamState.d_hitSpill = ctx->hitSpill;
    }
    if (e != hipSuccess) {
        std::string m = std::string("cpf_create: ") + hipGetErrorString(e);
        delete ctx;
        return fail(nullptr, CPF_ERR_HIP, m);
    }
    ctx->stream = ctx->ownStream;
    *out = ctx;
    return CPF_OK;
}

int cpf_destroy(cpf_context* ctx) {
    if (!ctx) return CPF_OK;
    (void)cpf_write_vtu_wait(ctx);                                             // never lose a frame
    (void)hipSetDevice(ctx->device);
    (void)hipStreamSynchronize(ctx->stream);
    delete ctx;
    return CPF_OK;
}

const char* cpf_last_error(const cpf_context* ctx) {
    if (ctx) return ctx->err.c_str();
    std::lock_guard<std::mutex> lk(g_mutex);
    return g_createError.c_str();
}

int cpf_set_stream(cpf_context* ctx, void* hip_stream) {
    CPF_REQUIRE(ctx, ctx, CPF_ERR_ARG, "null context");
    CPF_HIP(ctx, hipStreamSynchronize(ctx->stream));
    fieldFlagArrived(ctx);                      // (a field note still on its way was recorded on the old stream: complete now)
    ctx->stream = (hipStream_t)hip_stream;      // NULL == HIP's default stream, a valid choice
    return CPF_OK;
}

int cpf_use_own_stream(cpf_context* ctx) {
    CPF_REQUIRE(ctx, ctx, CPF_ERR_ARG, "null context");
    CPF_HIP(ctx, hipStreamSynchronize(ctx->stream));
    fieldFlagArrived(ctx);
    ctx->stream = ctx->ownStream;
    return CPF_OK;
}

int cpf_synchronize(cpf_context* ctx) {
    CPF_REQUIRE(ctx, ctx, CPF_ERR_ARG, "null context");
    CPF_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return CPF_OK;
}

int cpf_set_mesh(cpf_context* ctx, const double* points, int64_t nPoints, const int32_t* faceOffsets,
                 const int32_t* faceVerts, int64_t nFaces, const int32_t* owner, const int32_t* neighbour,
                 int64_t nInternal, int64_t nCells) {
    return setMeshImpl<int32_t>(ctx, points, nPoints, faceOffsets, faceVerts, nFaces, owner, neighbour, nInternal,
                                nCells);
}
int cpf_set_mesh_l64(cpf_context* ctx, const double* points, int64_t nPoints, const int64_t* faceOffsets,
                     const int64_t* faceVerts, int64_t nFaces, const int64_t* owner, const int64_t* neighbour,
                     int64_t nInternal, int64_t nCells) {
    return setMeshImpl<int64_t>(ctx, points, nPoints, faceOffsets, faceVerts, nFaces, owner, neighbour, nInternal,
                                nCells);
}

}  // extern "C"
namespace {
// The *_host entry points (no context, no GPU): the mesh arrays and whatever else must not be null (`more`) checked, then
// `body` under the guard against a host that runs out of memory.  hostTables: ... with the mesh's tables built for `use`.
template <typename Body>
int hostMesh(const double* points, const int32_t* faceOffsets, const int32_t* faceVerts, const int32_t* owner,
             const int32_t* neighbour, int64_t nInternal, bool more, Body body) {
    if (!points || !faceOffsets || !faceVerts || !owner || (!neighbour && nInternal != 0) || !more) return CPF_ERR_ARG;
    try { return body(); } catch (const std::bad_alloc&) { return CPF_ERR_NOMEM; }
}
template <typename Use>
int hostTables(const double* points, int64_t nPoints, const int32_t* faceOffsets, const int32_t* faceVerts, int64_t nFaces,
               const int32_t* owner, const int32_t* neighbour, int64_t nInternal, int64_t nCells, Use use) {
    return hostMesh(points, faceOffsets, faceVerts, owner, neighbour, nInternal, true, [&] {
        cpf::HostTables t;
        if (!cpf::build_tables<int32_t>(points, nPoints, faceOffsets, faceVerts, nFaces, owner, neighbour, nInternal, nCells, t).empty())
            return CPF_ERR_MESH;
        use(t);
        return CPF_OK;
    });
}
}  // namespace
extern "C" {

int cpf_build_mesh_tables_host(const double* points, int64_t nPoints, const int32_t* faceOffsets, const int32_t* faceVerts,
                               int64_t nFaces, const int32_t* owner, const int32_t* neighbour, int64_t nInternal, int64_t nCells,
                               int64_t* nSlots, int64_t* nGroups, int64_t* nMembers, int32_t* cellOff, double* planes,
                               int32_t* nbr, int32_t* groupOff, int32_t* groupNbr) {
    return hostTables(points, nPoints, faceOffsets, faceVerts, nFaces, owner, neighbour, nInternal, nCells, [&](const cpf::HostTables& t) {
        const int64_t g = t.nGroups(), mem = t.groupOff[(size_t)g];
        if (nSlots) *nSlots = t.nSlots;
        if (nGroups) *nGroups = g;
        if (nMembers) *nMembers = mem;
        if (cellOff) std::memcpy(cellOff, t.cellOff.data(), t.cellOff.size() * 4);
        if (planes) std::memcpy(planes, t.planes.data(), t.planes.size() * 8);
        if (nbr) std::memcpy(nbr, t.nbr.data(), t.nbr.size() * 4);
        if (groupOff) std::memcpy(groupOff, t.groupOff.data(), (size_t)(g + 1) * 4);
        if (groupNbr) std::memcpy(groupNbr, t.groupNbr.data(), (size_t)mem * 4);
    });
}

int cpf_mesh_flags_host(const double* points, int64_t nPoints, const int32_t* faceOffsets, const int32_t* faceVerts,
                        int64_t nFaces, const int32_t* owner, const int32_t* neighbour, int64_t nInternal, int64_t nCells,
                        int32_t* allHex, int32_t* zLayered, int32_t* zThin, int32_t* mixed) {
    return hostTables(points, nPoints, faceOffsets, faceVerts, nFaces, owner, neighbour, nInternal, nCells, [&](const cpf::HostTables& t) {
        // (what a context with the default options reports for this mesh: cpf_get_mesh_flags)
        if (allHex) *allHex = isAllHex(t) ? 1 : 0;
        if (zLayered) *zLayered = t.zPairLast ? 1 : 0;
        if (zThin) *zThin = t.zThin ? 1 : 0;
        if (mixed) *mixed = mixedKind(t, mixedRecordsFit(t));
    });
}

int cpf_mesh_box_records_host(const double* points, int64_t nPoints, const int32_t* faceOffsets, const int32_t* faceVerts,
                              int64_t nFaces, const int32_t* owner, const int32_t* neighbour, int64_t nInternal, int64_t nCells,
                              int32_t* isBox, double* boxRec) {
    return hostTables(points, nPoints, faceOffsets, faceVerts, nFaces, owner, neighbour, nInternal, nCells, [&](const cpf::HostTables& t) {
        if (isBox) *isBox = t.boxRec.empty() ? 0 : 1;
        if (boxRec && !t.boxRec.empty()) std::memcpy(boxRec, t.boxRec.data(), t.boxRec.size() * 8);
    });
}

int cpf_mesh_quality_host(const double* points, int64_t nPoints, const int32_t* faceOffsets, const int32_t* faceVerts,
                          int64_t nFaces, const int32_t* owner, const int32_t* neighbour, int64_t nInternal, int64_t nCells,
                          double tol, int split, cpf_mesh_quality* out) {
    return hostMesh(points, faceOffsets, faceVerts, owner, neighbour, nInternal, out && tol > 0.0, [&] {
        cpf::MeshQuality q;
        if (!cpf::measure_mesh<int32_t>(points, nPoints, faceOffsets, faceVerts, nFaces, owner, neighbour, nInternal, nCells, tol, q).empty())
            return CPF_ERR_MESH;
        int64_t nDerived = nCells;
        if (split && q.decompose()) {
            cpf::DerivedMesh dm;
            if (!cpf::derive_mesh<int32_t>(points, nPoints, faceOffsets, faceVerts, nFaces, owner, neighbour, nInternal, nCells, q, dm).empty())
                return CPF_ERR_MESH;
            nDerived = dm.nCells;
        }
        *out = toQuality(q, nDerived);
        return CPF_OK;
    });
}

int cpf_build_derived_mesh_host(const double* points, int64_t nPoints, const int32_t* faceOffsets, const int32_t* faceVerts,
                                int64_t nFaces, const int32_t* owner, const int32_t* neighbour, int64_t nInternal, int64_t nCells,
                                double tol, int64_t sizes[5], double* pointsOut, int32_t* faceOffOut, int32_t* faceVertsOut,
                                int32_t* ownerOut, int32_t* neighbourOut, int32_t* first) {
    return hostMesh(points, faceOffsets, faceVerts, owner, neighbour, nInternal, sizes && tol > 0.0, [&] {
        cpf::MeshQuality q;
        if (!cpf::measure_mesh<int32_t>(points, nPoints, faceOffsets, faceVerts, nFaces, owner, neighbour, nInternal, nCells, tol, q).empty())
            return CPF_ERR_MESH;
        cpf::DerivedMesh dm;     // (no cell to decompose: the derived mesh is the mesh as given)
        if (!cpf::derive_mesh<int32_t>(points, nPoints, faceOffsets, faceVerts, nFaces, owner, neighbour, nInternal, nCells, q, dm).empty())
            return CPF_ERR_MESH;
        if (dm.faceVerts.size() > (size_t)INT32_MAX) return CPF_ERR_MESH;
        sizes[0] = dm.nPoints; sizes[1] = dm.nFaces; sizes[2] = (int64_t)dm.faceVerts.size(); sizes[3] = dm.nInternal; sizes[4] = dm.nCells;
        auto narrow = [](const std::vector<int64_t>& v, int32_t* o) { if (o) for (size_t i = 0; i < v.size(); ++i) o[i] = (int32_t)v[i]; };
        if (pointsOut) std::memcpy(pointsOut, dm.points.data(), dm.points.size() * 8);
        narrow(dm.faceOff, faceOffOut); narrow(dm.faceVerts, faceVertsOut); narrow(dm.owner, ownerOut); narrow(dm.neighbour, neighbourOut);
        if (first) std::memcpy(first, dm.first.data(), dm.first.size() * 4);
        return CPF_OK;
    });
}

int cpf_cell_volumes_host(const double* points, int64_t nPoints, const int32_t* faceOffsets, const int32_t* faceVerts,
                          int64_t nFaces, const int32_t* owner, const int32_t* neighbour, int64_t nInternal, int64_t nCells, double* V) {
    return hostMesh(points, faceOffsets, faceVerts, owner, neighbour, nInternal, V != nullptr, [&] {
        cpf::MeshQuality q;
        if (!cpf::measure_mesh<int32_t>(points, nPoints, faceOffsets, faceVerts, nFaces, owner, neighbour, nInternal, nCells,
                                        cpf::kNonPlanarTolDefault, q).empty())
            return CPF_ERR_MESH;
        std::memcpy(V, q.volume.data(), q.volume.size() * 8);
        return CPF_OK;
    });
}

int cpf_get_cell_volumes(const cpf_context* ctx, double* V) {
    CPF_REQUIRE(ctx, ctx && V, CPF_ERR_ARG, "null argument");
    CPF_REQUIRE(ctx, ctx->mesh.have, CPF_ERR_STATE, "cpf_get_cell_volumes: call cpf_set_mesh first");
    std::memcpy(V, ctx->mesh.volume.data(), ctx->mesh.volume.size() * 8);
    return CPF_OK;
}

int cpf_get_mesh_quality(const cpf_context* ctx, cpf_mesh_quality* out) {
    CPF_REQUIRE(ctx, ctx && out, CPF_ERR_ARG, "null argument");
    CPF_REQUIRE(ctx, ctx->mesh.have, CPF_ERR_STATE, "cpf_get_mesh_quality: call cpf_set_mesh first");
    *out = ctx->mesh.quality;
    return CPF_OK;
}

int cpf_cells_to_parent_dev(cpf_context* ctx, const int32_t* in, int32_t* out, int64_t n) {
    CPF_REQUIRE(ctx, ctx, CPF_ERR_ARG, "null context");
    CPF_REQUIRE(ctx, ctx->mesh.have, CPF_ERR_STATE, "cpf_cells_to_parent_dev: call cpf_set_mesh first");
    CPF_REQUIRE(ctx, n >= 0 && (n == 0 || (in && out)), CPF_ERR_ARG, "cpf_cells_to_parent_dev: bad arguments");
    CPF_HIP(ctx, hipSetDevice(ctx->device));
    if (ctx->mesh.parentOf) CPF_HIP(ctx, cpf::launch_cells_to_parent(ctx->stream, in, out, ctx->mesh.parentOf, n, ctx->mesh.host.nCells));
    else if (n > 0 && in != out) CPF_HIP(ctx, hipMemcpyAsync(out, in, (size_t)n * 4, hipMemcpyDeviceToDevice, ctx->stream));
    return CPF_OK;
}

int cpf_mesh_info(const cpf_context* ctx, int64_t* nCells, int64_t* nSlots, int64_t* deviceBytes) {
    CPF_REQUIRE(ctx, ctx, CPF_ERR_ARG, "null context");
    CPF_REQUIRE(ctx, ctx->mesh.have, CPF_ERR_STATE, "cpf_mesh_info: no mesh set");
    if (nCells) *nCells = ctx->mesh.host.nCells;
    if (nSlots) *nSlots = ctx->mesh.host.nSlots;
    if (deviceBytes) *deviceBytes = (int64_t)ctx->mesh.bytes;
    return CPF_OK;
}

int cpf_get_mesh_tables(const cpf_context* ctx, int32_t* cellOff, double* planes, int32_t* nbr) {
    CPF_REQUIRE(ctx, ctx, CPF_ERR_ARG, "null context");
    CPF_REQUIRE(ctx, ctx->mesh.have, CPF_ERR_STATE, "cpf_get_mesh_tables: no mesh set");
    const cpf::HostTables& h = ctx->mesh.host;
    if (cellOff) std::memcpy(cellOff, h.cellOff.data(), h.cellOff.size() * 4);
    if (planes) std::memcpy(planes, h.planes.data(), h.planes.size() * 8);
    if (nbr) std::memcpy(nbr, h.nbr.data(), h.nbr.size() * 4);
    return CPF_OK;
}

int cpf_get_mesh_groups(const cpf_context* ctx, int64_t* nGroups, int64_t* nMembers, int32_t* groupOff, int32_t* groupNbr) {
    CPF_REQUIRE(ctx, ctx, CPF_ERR_ARG, "null context");
    CPF_REQUIRE(ctx, ctx->mesh.have, CPF_ERR_STATE, "cpf_get_mesh_groups: no mesh set");
    const cpf::HostTables& h = ctx->mesh.host;
    const int64_t g = h.nGroups();
    if (nGroups) *nGroups = g;
    if (nMembers) *nMembers = h.groupOff[(size_t)g];
    if (groupOff) std::memcpy(groupOff, h.groupOff.data(), (size_t)(g + 1) * 4);
    if (groupNbr) std::memcpy(groupNbr, h.groupNbr.data(), (size_t)h.groupOff[(size_t)g] * 4);
    return CPF_OK;
}

int cpf_get_mesh_flags(const cpf_context* ctx, int32_t* allHex, int32_t* zLayered, int32_t* zThin, int32_t* mixed) {
    CPF_REQUIRE(ctx, ctx, CPF_ERR_ARG, "null context");
    CPF_REQUIRE(ctx, ctx->mesh.have, CPF_ERR_STATE, "cpf_get_mesh_flags: no mesh set");
    const cpf::MeshView m = meshView(ctx);
    if (allHex) *allHex = m.allHex;
    if (zLayered) *zLayered = m.zPairLast;
    if (zThin) *zThin = m.zThin;
    if (mixed) *mixed = m.mixed;
    return CPF_OK;
}

int cpf_set_velocity(cpf_context* ctx, const double* U, int64_t nCells) {
    CPF_REQUIRE(ctx, ctx, CPF_ERR_ARG, "null context");
    CPF_REQUIRE(ctx, ctx->mesh.have, CPF_ERR_STATE, "cpf_set_velocity: call cpf_set_mesh first");
    CPF_REQUIRE(ctx, U && nCells == ctx->mesh.nParent, CPF_ERR_ARG, "cpf_set_velocity: U is null or nCells differs from the mesh");
    CPF_HIP(ctx, hipSetDevice(ctx->device));
    if (ctx->mesh.parentOf) {                             // per parent cell -> every derived cell of it
        CPF_HIP(ctx, hipMemcpyAsync(ctx->mesh.Uparent, U, (size_t)nCells * 24, hipMemcpyHostToDevice, ctx->stream));
        CPF_HIP(ctx, cpf::launch_gather_parent_u3(ctx->stream, ctx->mesh.Uparent, ctx->mesh.parentOf, ctx->mesh.U3, ctx->mesh.host.nCells));
    } else {
        CPF_HIP(ctx, hipMemcpyAsync(ctx->mesh.U3, U, (size_t)nCells * 24, hipMemcpyHostToDevice, ctx->stream));
    }
    CPF_HIP(ctx, layOutField(ctx, ctx->mesh.U3, ctx->mesh.host.nCells));
    if (ctx->mesh.follow.on) CPF_HIP(ctx, refreshSource(ctx, ctx->mesh.U3, 3));
    CPF_HIP(ctx, hipStreamSynchronize(ctx->stream));   // U may be pageable host memory owned by the caller
    fieldFlagArrived(ctx);
    ctx->mesh.haveU = true;
    return CPF_OK;
}

int cpf_set_velocity_dev(cpf_context* ctx, const double* dU, int64_t nCells) {
    CPF_REQUIRE(ctx, ctx, CPF_ERR_ARG, "null context");
    CPF_REQUIRE(ctx, ctx->mesh.have, CPF_ERR_STATE, "cpf_set_velocity_dev: call cpf_set_mesh first");
    CPF_REQUIRE(ctx, dU && nCells == ctx->mesh.nParent, CPF_ERR_ARG, "cpf_set_velocity_dev: bad arguments");
    CPF_HIP(ctx, hipSetDevice(ctx->device));
    if (ctx->mesh.parentOf) {                             // per parent cell -> every derived cell of it
        CPF_HIP(ctx, cpf::launch_gather_parent_u3(ctx->stream, dU, ctx->mesh.parentOf, ctx->mesh.U3, ctx->mesh.host.nCells));
        dU = ctx->mesh.U3;
    }
    CPF_HIP(ctx, layOutField(ctx, dU, ctx->mesh.host.nCells));   // (asynchronous: the flat walk waits until the flag has been seen to arrive)
    if (ctx->mesh.follow.on) CPF_HIP(ctx, refreshSource(ctx, dU, 3));
    ctx->mesh.haveU = true;
    return CPF_OK;
}

int cpf_alloc_particles(cpf_context* ctx, int64_t capacity) {
    CPF_REQUIRE(ctx, ctx, CPF_ERR_ARG, "null context");
    CPF_REQUIRE(ctx, capacity > 0 && capacity < ((int64_t)1 << 31), CPF_ERR_ARG, "cpf_alloc_particles: capacity must be in (0, 2^31)");
    CPF_HIP(ctx, hipSetDevice(ctx->device));
    CPF_HIP(ctx, hipStreamSynchronize(ctx->stream));
    ctx->cloud = Cloud{};
    cpf::ledger_clear(ctx);
    const size_t c = (size_t)capacity;
    CPF_HIP(ctx, ctx->cloud.cur.alloc(c));
    CPF_HIP(ctx, ctx->cloud.vel.alloc(c * 3));
    CPF_HIP(ctx, hipMemsetAsync(ctx->cloud.vel, 0, c * 24, ctx->stream));          // src/initCuda.H:148-149
    CPF_HIP(ctx, hipMemsetAsync(ctx->cloud.cur.cell, 0xFF, c * 4, ctx->stream));       // -1, src/initCuda.H:145
    ctx->cloud.cap = capacity;
    return CPF_OK;
}

int cpf_seed_box(cpf_context* ctx, int64_t n, const double lower[3], const double upper[3], int order) {
    CPF_REQUIRE(ctx, ctx, CPF_ERR_ARG, "null context");
    CPF_REQUIRE(ctx, lower && upper && n > 0, CPF_ERR_ARG, "cpf_seed_box: bad arguments");
    if (ctx->cloud.cap < n) { int r = cpf_alloc_particles(ctx, n); if (r) return r; }
    if (int r = cpf::ledger_new_cloud(ctx)) return r;       // (the stamps, origins, doses, last zones and records were the old one's)
    CPF_HIP(ctx, hipSetDevice(ctx->device));
    CPF_HIP(ctx, cpf::launch_seed_box(ctx->stream, ctx->cloud.cur.x, ctx->cloud.cur.y, ctx->cloud.cur.z, 0, n, lower, upper, order));
    CPF_HIP(ctx, cpf::launch_iota64(ctx->stream, ctx->cloud.cur.gid, n, 0));
    CPF_HIP(ctx, hipMemsetAsync(ctx->cloud.cur.cell, 0xFF, (size_t)n * 4, ctx->stream));
    ctx->cloud.n = n; ctx->cloud.located = false; ctx->cloud.zSettled = false; ctx->cloud.respawnEpoch = 0;
    return CPF_OK;
}

int cpf_set_particles(cpf_context* ctx, int64_t n, const double* xyz, const int32_t* cell) {
    CPF_REQUIRE(ctx, ctx, CPF_ERR_ARG, "null context");
    CPF_REQUIRE(ctx, xyz && n > 0, CPF_ERR_ARG, "cpf_set_particles: bad arguments");
    if (ctx->cloud.cap < n) { int r = cpf_alloc_particles(ctx, n); if (r) return r; }
    int r = cpf::ledger_new_cloud(ctx);                     // (as in cpf_seed_box)
    if (r) return r;
    CPF_HIP(ctx, hipSetDevice(ctx->device));
    ctx->cloud.zSettled = false;
    r = ensureScratch(ctx, (size_t)n * 24);
    if (r) return r;
    CPF_HIP(ctx, hipMemcpyAsync(ctx->scratch, xyz, (size_t)n * 24, hipMemcpyHostToDevice, ctx->stream));
    CPF_HIP(ctx, cpf::launch_unpack_xyz(ctx->stream, (const double*)ctx->scratch.get(), ctx->cloud.cur.x, ctx->cloud.cur.y, ctx->cloud.cur.z, n));
    CPF_HIP(ctx, cpf::launch_iota64(ctx->stream, ctx->cloud.cur.gid, n, 0));
    std::vector<int32_t> sub;
    if (cell && ctx->mesh.parentOf) {                     // parent cells -> the derived cell of each that holds the point
        std::string why = resolveSubCells(ctx, n, xyz, cell, sub);
        if (!why.empty()) { (void)hipStreamSynchronize(ctx->stream); return fail(ctx, CPF_ERR_ARG, "cpf_set_particles: " + why); }
        cell = sub.data();
    }
    if (cell) CPF_HIP(ctx, hipMemcpyAsync(ctx->cloud.cur.cell, cell, (size_t)n * 4, hipMemcpyHostToDevice, ctx->stream));
    else CPF_HIP(ctx, hipMemsetAsync(ctx->cloud.cur.cell, 0xFF, (size_t)n * 4, ctx->stream));
    CPF_HIP(ctx, hipStreamSynchronize(ctx->stream));
    ctx->cloud.n = n; ctx->cloud.located = cell != nullptr; ctx->cloud.respawnEpoch = 0;
    return CPF_OK;
}

int cpf_locate_initial_dev(cpf_context* ctx, const double* x, const double* y, const double* z, int32_t* cell,
                           int64_t n) {
    CPF_REQUIRE(ctx, ctx, CPF_ERR_ARG, "null context");
    CPF_REQUIRE(ctx, ctx->mesh.have, CPF_ERR_STATE, "cpf_locate_initial: call cpf_set_mesh first");
    CPF_REQUIRE(ctx, n >= 0 && (n == 0 || (x && y && z && cell)), CPF_ERR_ARG, "cpf_locate_initial: null array");
    CPF_HIP(ctx, hipSetDevice(ctx->device));
    CPF_HIP(ctx, cpf::launch_locate_initial(ctx->stream, x, y, z, cell, n, meshView(ctx), gridView(ctx)));
    return CPF_OK;
}

int cpf_locate_initial(cpf_context* ctx, int64_t* nOutside) {
    CPF_REQUIRE(ctx, ctx, CPF_ERR_ARG, "null context");
    CPF_REQUIRE(ctx, ctx->cloud.n > 0, CPF_ERR_STATE, "cpf_locate_initial: no particles (seed or set them first)");
    ctx->cloud.zSettled = false;                    // (a frozen particle found inside the mesh is live again, with whatever z it had)
    int r = cpf_locate_initial_dev(ctx, ctx->cloud.cur.x, ctx->cloud.cur.y, ctx->cloud.cur.z, ctx->cloud.cur.cell, ctx->cloud.n);
    if (r) return r;
    ctx->cloud.located = true;
    return nOutside ? countNegative(ctx, ctx->cloud.cur.cell, ctx->cloud.n, nOutside) : CPF_OK;
}

// the "VertexVelocity" cycle's tables (the cone-locate records only with "vertex_fast")
static cpf::VertexField vertexField(const cpf_context* ctx) {
    return {ctx->tet.pos, ctx->tet.tets, ctx->tet.vel, ctx->tet.tetsPerCell, ctx->vertexFast ? ctx->tet.cone.get() : nullptr,
            reinterpret_cast<const double4*>(ctx->tet.apex.get())};
}

int cpf_step_dev(cpf_context* ctx, double* x, double* y, double* z, int32_t* cell, const int64_t* gid, double* vel,
                 int64_t n, double dt, double D, uint32_t step0, int nCycles, unsigned flags) {
    CPF_REQUIRE(ctx, ctx, CPF_ERR_ARG, "null context");
    CPF_REQUIRE(ctx, ctx->mesh.have, CPF_ERR_STATE, "cpf_step: call cpf_set_mesh first");
    CPF_REQUIRE(ctx, ctx->mesh.haveU, CPF_ERR_STATE, "cpf_step: call cpf_set_velocity first");
    CPF_REQUIRE(ctx, n >= 0 && nCycles >= 0, CPF_ERR_ARG, "cpf_step: negative count");
    CPF_REQUIRE(ctx, n == 0 || (x && y && z && cell), CPF_ERR_ARG, "cpf_step: null particle array");
    CPF_REQUIRE(ctx, std::isfinite(dt) && std::isfinite(D) && D >= 0.0, CPF_ERR_ARG, "cpf_step: dt/D not finite or D < 0");
    CPF_REQUIRE(ctx, !(flags & CPF_STEP_STORE_VEL) || vel, CPF_ERR_ARG, "cpf_step: CPF_STEP_STORE_VEL needs a vel array");
    CPF_HIP(ctx, hipSetDevice(ctx->device));
    const bool vertexU = (flags & CPF_STEP_VERTEX_VELOCITY) != 0;
    CPF_REQUIRE(ctx, !vertexU || (ctx->tet.haveVel && ctx->tet.nTets == (int64_t)ctx->tet.tetsPerCell * ctx->mesh.host.nCells), CPF_ERR_STATE,
                "cpf_step: CPF_STEP_VERTEX_VELOCITY needs cpf_set_tets and cpf_set_vertex_velocity for the current mesh");
    const cpf::MeshView m = meshView(ctx);
    const cpf::VertexField vf = vertexField(ctx);
    const bool fuse = (flags & CPF_STEP_FUSE_CYCLES) != 0;
    pollFieldFlag(ctx);
    // z settled: the caller's word for the first launch; after a launch, what that launch left behind -- settled behind a
    // flat instantiation (it maps every live particle's z to a fixed point, or was given settled z and left it alone), not
    // settled behind any other; a launch of zero cycles loads and stores only and changes nothing
    bool settled = (flags & CPF_STEP_Z_SETTLED) != 0;
    ctx->lastStepZSettled = false;
    const int nLaunch = fuse ? 1 : nCycles;   // fused with nCycles == 0: load+store only (bandwidth calibration)
    const int cycPerLaunch = fuse ? nCycles : 1;
    for (int c = 0; c < nLaunch; ++c) {
        const cpf::StepPlan plan = cpf::plan_step(m, ctx->streamState, ctx->stepVariant, vertexU ? &vf : nullptr, n, cycPerLaunch, D,
                                                  flags, ctx->stats);
        // A flat launch that streams z reports live particles whose z is not finite (StreamState::zBad): z of such a cloud is not
        // settled, whatever the flat cycle's fixed points are -- at a wall the streaming launch mirrors such a particle to NaN in
        // x and y, a launch without z would reflect it.  The verdict of the launch that settled z is read here, once, before the
        // first launch that would rely on it; a launch that streams z starts from a clean flag
        if (plan.flat_body(ctx->streamState, settled) && zBadArrived(ctx)) settled = false;
        // ("flat_z" 0: nobody asks.  A verdict still pending belongs to an older launch of the same kind: its 1 may stand)
        const bool reportsZ = n > 0 && cycPerLaunch > 0 && plan.flat() && !settled && ctx->streamState.flatZ != 0;
        if (reportsZ && !ctx->zBadPending) *static_cast<volatile unsigned*>(ctx->h_zBad) = 0u;
        Event e0, e1;
        const bool timed = ctx->timing.on && (ctx->timing.launch++ % (uint64_t)ctx->timing.stride) == 0;
        // the streaming kernels stamp the events with the dispatch's own begin / end (StepPlan::stamped); any other kernel,
        // and a launch without particles (nothing is dispatched), is bracketed by two event records
        const bool stamped = timed && n > 0 && plan.stamped();
        if (timed) {
            CPF_HIP(ctx, ctx->timing.take(e0)); CPF_HIP(ctx, ctx->timing.take(e1));
            if (!stamped) CPF_HIP(ctx, hipEventRecord(e0, ctx->stream));
        }
        ctx->lastStepN = n; ctx->lastStepCycles = cycPerLaunch;
        const hipError_t le = cpf::launch_step(plan, ctx->stream, x, y, z, cell, gid, vel, n, dt, D, step0 + (uint32_t)c, cycPerLaunch,
                                               ctx->seed, m, ctx->stats ? ctx->counters : nullptr, vertexU ? &vf : nullptr,
                                               ctx->streamState, settled, stamped ? e0.get() : nullptr, stamped ? e1.get() : nullptr);
        if (le != hipSuccess) {
            // a launch that did not go out (occupancy query, tile count, missing spill area): the two events go back to the
            // pool instead of leaking
            ctx->timing.give_back(e0); ctx->timing.give_back(e1);
        }
        CPF_HIP(ctx, le);
        if (n > 0 && cycPerLaunch > 0) settled = plan.flat();
        if (reportsZ) {
            CPF_HIP(ctx, hipEventRecord(ctx->evZBad, ctx->stream));
            ctx->zBadPending = true;
        }
        if (timed) {
            if (!stamped) CPF_HIP(ctx, hipEventRecord(e1, ctx->stream));
            ctx->timing.recorded.emplace_back(std::move(e0), std::move(e1));
        }
    }
    ctx->lastStepZSettled = settled;
    return CPF_OK;
}

int cpf_step(cpf_context* ctx, double dt, double D, int nCycles, unsigned flags) {
    CPF_REQUIRE(ctx, ctx, CPF_ERR_ARG, "null context");
    CPF_REQUIRE(ctx, ctx->cloud.n > 0, CPF_ERR_STATE, "cpf_step: no particles");
    CPF_REQUIRE(ctx, ctx->cloud.located, CPF_ERR_STATE, "cpf_step: particles have no cells yet (call cpf_locate_initial)");
    // a frame holds the velocities of the particles this call steps; one that is not stepped -- lost, frozen -- has none (the
    // reference's array keeps the velocity of such a particle's last advect, cuda/particles.cu:316-373; with the velocities stored
    // on frame cycles only that would be the one of its last FRAME, and a sharded cloud does not carry it along at all)
    if ((flags & CPF_STEP_STORE_VEL) && ctx->cloud.vel) {
        CPF_HIP(ctx, hipSetDevice(ctx->device));
        CPF_HIP(ctx, hipMemsetAsync(ctx->cloud.vel, 0, (size_t)ctx->cloud.n * 24, ctx->stream));
    }
    const bool settled = ctx->cloud.zSettled;
    ctx->cloud.zSettled = false;
    int r = cpf_step_dev(ctx, ctx->cloud.cur.x, ctx->cloud.cur.y, ctx->cloud.cur.z, ctx->cloud.cur.cell, ctx->cloud.cur.gid, ctx->cloud.vel, ctx->cloud.n, dt, D, ctx->stepCounter,
                         nCycles, (flags & ~CPF_STEP_Z_SETTLED) | (settled ? CPF_STEP_Z_SETTLED : 0u));
    if (r != CPF_OK) return r;
    ctx->cloud.zSettled = ctx->lastStepZSettled;
    // a cycle of zero length without a kick moves nothing: it is the frame-0 idiom (velocities of one advect in the
    // first output file, out-of-domain particles frozen; src/initCuda.H:184-201) and not a step of the run, so the
    // counter-based Brownian stream and the sort cadence do not see it
    if (!(dt == 0.0 && D == 0.0)) ctx->stepCounter += (uint32_t)nCycles;
    // keep waves cell-coherent: particle ids (and stored velocities) travel with the particles, so callers
    // never see the reordering
    if (ctx->sortInterval > 0 && ctx->stepCounter - ctx->lastSortStep >= (uint32_t)ctx->sortInterval) {
        r = cpf_sort_by_cell(ctx);
        ctx->lastSortStep = ctx->stepCounter;
    }
    return r;
}

int cpf_seed_box_dev(cpf_context* ctx, double* x, double* y, double* z, int64_t first, int64_t n,
                     const double lower[3], const double upper[3], int order) {
    CPF_REQUIRE(ctx, ctx, CPF_ERR_ARG, "null context");
    CPF_REQUIRE(ctx, n >= 0 && first >= 0 && lower && upper && (n == 0 || (x && y && z)), CPF_ERR_ARG, "cpf_seed_box_dev: bad arguments");
    CPF_HIP(ctx, hipSetDevice(ctx->device));
    CPF_HIP(ctx, cpf::launch_seed_box(ctx->stream, x, y, z, first, n, lower, upper, order));
    return CPF_OK;
}

namespace {
// in place (ox == nullptr) or into the out arrays
int sortImpl(cpf_context* ctx, double* x, double* y, double* z, int32_t* cell, int64_t* gid, int64_t n, double* ox, double* oy,
             double* oz, int32_t* ocell, int64_t* ogid, double* vel3) {
    CPF_REQUIRE(ctx, ctx->mesh.have, CPF_ERR_STATE, "cpf_sort_by_cell: call cpf_set_mesh first");
    CPF_REQUIRE(ctx, n >= 0 && n < ((int64_t)1 << 31) && (n == 0 || (x && y && z && cell)), CPF_ERR_ARG, "cpf_sort_by_cell: bad arguments");
    CPF_REQUIRE(ctx, ctx->mesh.host.nCells < ((int64_t)1 << 26) - 2, CPF_ERR_STATE, "cpf_sort_by_cell: more than 2^26 cells");
    CPF_HIP(ctx, hipSetDevice(ctx->device));
    const int endBit = sortEndBit(ctx);
    const bool census = ctx->streamState.densityLookup != 0 && ctx->occupied && ctx->h_occupied;
    // sparse clouds (the regime of the streaming kernel's LOOKUP 4: fewer than 8 particles per cell) are ordered along the mesh
    // layer's Morton curve instead of by cell id: measured 0.164 -> 0.153 ms per step at 0.6 particles per cell on the 2.1e6-cell
    // box; dense clouds on a 3-D mesh LOSE 7 % with it (blockMesh's numbering runs along the flow), hence by regime
    const bool curve = ctx->mesh.curveRank != nullptr && (ctx->sortCurve == 1 || (ctx->sortCurve < 0 && n < 8 * ctx->mesh.host.nCells));
    int r = ensureScratch(ctx, cpf::sort_scratch_bytes(n, endBit));
    if (r) return r;
    CPF_HIP(ctx, cpf::sort_by_cell(ctx->stream, x, y, z, cell, gid, vel3, n, endBit, ctx->mesh.cellBox, ctx->mesh.host.subBits,
                                   ctx->mesh.host.subOrder, ctx->scratch, ctx->scratchBytes, ox, oy, oz, ocell, ogid, census ? ctx->occupied : nullptr,
                                   curve ? ctx->mesh.curveRank : nullptr, ctx->sortMethod));
    // how many cells hold particles: what the streaming kernel's lookup method goes by with "stream_lookup_by_density"
    // (StreamState::occupiedHost).  Only then: the 16-byte device-to-host copy behind the sort costs 0.9 ms on this stack
    // (measured: 1.50 against 0.60 ms per sort of 1e7 particles) -- more than the sort itself.
    if (census)
        CPF_HIP(ctx, hipMemcpyAsync(ctx->h_occupied, ctx->occupied, 16, hipMemcpyDeviceToHost, ctx->stream));
    return CPF_OK;
}
}  // namespace

int cpf_sort_by_cell_dev(cpf_context* ctx, double* x, double* y, double* z, int32_t* cell, int64_t* gid, int64_t n) {
    CPF_REQUIRE(ctx, ctx, CPF_ERR_ARG, "null context");
    if (n <= 1) return CPF_OK;
    return sortImpl(ctx, x, y, z, cell, gid, n, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr);
}

int cpf_sort_by_cell_dev_to(cpf_context* ctx, const double* x, const double* y, const double* z, const int32_t* cell,
                            const int64_t* gid, double* ox, double* oy, double* oz, int32_t* ocell, int64_t* ogid, int64_t n) {
    CPF_REQUIRE(ctx, ctx, CPF_ERR_ARG, "null context");
    CPF_REQUIRE(ctx, n == 0 || (ox && oy && oz && ocell && (ogid || !gid)), CPF_ERR_ARG, "cpf_sort_by_cell_dev_to: null output array");
    CPF_REQUIRE(ctx, n == 0 || (ox != x && oy != y && oz != z && ocell != cell), CPF_ERR_ARG, "cpf_sort_by_cell_dev_to: outputs alias inputs");
    if (n <= 0) return CPF_OK;
    if (n == 1) {           // nothing to sort, but the contract is "the cloud is in the out arrays"
        CPF_HIP(ctx, hipSetDevice(ctx->device));
        CPF_HIP(ctx, hipMemcpyAsync(ox, x, 8, hipMemcpyDeviceToDevice, ctx->stream));
        CPF_HIP(ctx, hipMemcpyAsync(oy, y, 8, hipMemcpyDeviceToDevice, ctx->stream));
        CPF_HIP(ctx, hipMemcpyAsync(oz, z, 8, hipMemcpyDeviceToDevice, ctx->stream));
        CPF_HIP(ctx, hipMemcpyAsync(ocell, cell, 4, hipMemcpyDeviceToDevice, ctx->stream));
        if (gid) CPF_HIP(ctx, hipMemcpyAsync(ogid, gid, 8, hipMemcpyDeviceToDevice, ctx->stream));
        return CPF_OK;
    }
    return sortImpl(ctx, const_cast<double*>(x), const_cast<double*>(y), const_cast<double*>(z), const_cast<int32_t*>(cell),
                    const_cast<int64_t*>(gid), n, ox, oy, oz, ocell, ogid, nullptr);
}

int cpf_sort_by_cell(cpf_context* ctx) {
    CPF_REQUIRE(ctx, ctx, CPF_ERR_ARG, "null context");
    CPF_REQUIRE(ctx, ctx->cloud.n > 0 && ctx->cloud.located, CPF_ERR_STATE, "cpf_sort_by_cell: no located particles");
    if (ctx->cloud.n <= 1) return CPF_OK;
    // the context's own cloud: sorted into its second set of arrays, then the sets swap roles
    CloudArrays &cur = ctx->cloud.cur, &spare = ctx->cloud.spare;
    if (spare.x == nullptr) {
        CPF_HIP(ctx, hipSetDevice(ctx->device));
        CloudArrays s;                         // moved in whole: a failure part-way leaves no second set behind
        CPF_HIP(ctx, s.alloc((size_t)ctx->cloud.cap));
        CPF_HIP(ctx, hipMemsetAsync(s.cell, 0xFF, (size_t)ctx->cloud.cap * 4, ctx->stream));
        spare = std::move(s);
    }
    int r = sortImpl(ctx, cur.x, cur.y, cur.z, cur.cell, cur.gid, ctx->cloud.n, spare.x, spare.y, spare.z, spare.cell, spare.gid, ctx->cloud.vel);
    if (r) return r;
    std::swap(cur, spare);
    return CPF_OK;
}

int cpf_num_particles(const cpf_context* ctx, int64_t* n) {
    CPF_REQUIRE(ctx, ctx && n, CPF_ERR_ARG, "null argument");
    *n = ctx->cloud.n;
    return CPF_OK;
}

int cpf_get_particles(cpf_context* ctx, double* xyzw, int32_t* cell, double* vel) {
    CPF_REQUIRE(ctx, ctx, CPF_ERR_ARG, "null context");
    CPF_REQUIRE(ctx, ctx->cloud.n > 0, CPF_ERR_STATE, "cpf_get_particles: no particles");
    CPF_HIP(ctx, hipSetDevice(ctx->device));
    const size_t n = (size_t)ctx->cloud.n;
    const PackLayout lay(n);
    int r = ensureScratch(ctx, lay.bytes);
    if (r) return r;
    double* dX = (double*)ctx->scratch.get();
    int32_t* dC = (int32_t*)(ctx->scratch + lay.offC);
    double* dV = (double*)(ctx->scratch + lay.offV);
    CPF_HIP(ctx, cpf::launch_pack_by_gid(ctx->stream, ctx->cloud.cur.x, ctx->cloud.cur.y, ctx->cloud.cur.z, ctx->cloud.cur.cell, ctx->cloud.cur.gid, ctx->cloud.vel,
                                         xyzw ? dX : nullptr, cell ? dC : nullptr, vel ? dV : nullptr, ctx->cloud.n));
    if (cell && ctx->mesh.parentOf) CPF_HIP(ctx, cpf::launch_cells_to_parent(ctx->stream, dC, dC, ctx->mesh.parentOf, ctx->cloud.n, ctx->mesh.host.nCells));
    if (xyzw) CPF_HIP(ctx, hipMemcpyAsync(xyzw, dX, n * 32, hipMemcpyDeviceToHost, ctx->stream));
    if (cell) CPF_HIP(ctx, hipMemcpyAsync(cell, dC, n * 4, hipMemcpyDeviceToHost, ctx->stream));
    if (vel) CPF_HIP(ctx, hipMemcpyAsync(vel, dV, n * 32, hipMemcpyDeviceToHost, ctx->stream));
    CPF_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return CPF_OK;
}

int cpf_get_counters(cpf_context* ctx, int64_t out[4]) {
    CPF_REQUIRE(ctx, ctx && out, CPF_ERR_ARG, "null argument");
    CPF_HIP(ctx, hipSetDevice(ctx->device));
    std::vector<unsigned long long> h((size_t)cpf::kCounterSlots * 4);
    CPF_HIP(ctx, hipMemcpyAsync(h.data(), ctx->counters, h.size() * 8, hipMemcpyDeviceToHost, ctx->stream));
    CPF_HIP(ctx, hipStreamSynchronize(ctx->stream));
    for (int k = 0; k < 4; ++k) {
        unsigned long long sum = 0;
        for (int s = 0; s < cpf::kCounterSlots; ++s) sum += h[(size_t)s * 4 + k];
        out[k] = (int64_t)sum;
    }
    return CPF_OK;
}

}  // extern "C"
namespace {
// "sort_key_bits": sub-cell sort key layout: 100*bx + 10*by + bz bits for the position inside the cell's box along x, y, z
// (most significant axis first as chosen at mesh ingest); default chosen by cpf_set_mesh
int setSortKeyBits(cpf_context* ctx, double value) {
    CPF_REQUIRE(ctx, ctx->mesh.have, CPF_ERR_STATE, "sort_key_bits: call cpf_set_mesh first");
    const int v = (int)value, nb[3] = {v / 100, (v / 10) % 10, v % 10};
    CPF_REQUIRE(ctx, value == v && v >= 0 && nb[0] <= 9 && nb[0] + nb[1] + nb[2] <= 12, CPF_ERR_ARG, "sort_key_bits: at most 12 bits");
    cpf::HostTables& h = ctx->mesh.host;
    for (int a = 0; a < 3; ++a) {
        const float f = std::ldexp(1.0f, nb[a] - h.subBits[a]);
        for (size_t c = 0; c < h.cellBox.size() / 6; ++c) h.cellBox[6 * c + 3 + a] *= f;
        h.subBits[a] = nb[a];
    }
    CPF_HIP(ctx, hipSetDevice(ctx->device));
    CPF_HIP(ctx, hipMemcpyAsync(ctx->mesh.cellBox, h.cellBox.data(), h.cellBox.size() * 4, hipMemcpyHostToDevice, ctx->stream));
    CPF_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return CPF_OK;
}
int setStepVariant(cpf_context* ctx, double value) {
#ifndef CPF_EXPERIMENTS
    CPF_REQUIRE(ctx, value != 1 && value != 2 && value != 5, CPF_ERR_ARG,
                "step_variant 1, 2 and 5 are experiments (measured slower on every mesh) and not in this build: make EXPERIMENTS=1");
#endif
    ctx->stepVariant = (int)value;
    return CPF_OK;
}

// cpf_set_option's keys.  A value is accepted if lo <= value <= hi and, with step > 0, it is one of lo, lo + step, ...; a refused
// one gets CPF_ERR_ARG and `message`.  No message: any value goes (the setter may still refuse).
struct Option {
    const char* key;
    double lo, hi, step;
    const char* message;
    int (*set)(cpf_context*, double);
};
#define CPF_OPT(lvalue, expr) [](cpf_context* c, double v) -> int { c->lvalue = (expr); return CPF_OK; }
constexpr double kTiny = std::numeric_limits<double>::denorm_min(), kHuge = std::numeric_limits<double>::max();
const Option kOptions[] = {
    {"step_variant", -1, 5, 1, "step_variant must be -1..5", setStepVariant},
    {"vertex_fast", 0, 1, 1, "vertex_fast must be 0 or 1", CPF_OPT(vertexFast, v != 0)},
    {"z_fold", 0, 1, 1, "z_fold must be 0 or 1", CPF_OPT(zFold, v != 0)},
    {"mixed_records", 0, 1, 1, "mixed_records must be 0 or 1", CPF_OPT(mixedRecords, v != 0)},
    {"flat_walk", 0, 1, 1, "flat_walk must be 0 or 1", CPF_OPT(streamState.flat, (int)v)},
    {"flat_z", 0, 1, 1, "flat_z must be 0 or 1", CPF_OPT(streamState.flatZ, (int)v)},
    {"box_records", 0, 1, 1, "box_records must be 0 or 1", CPF_OPT(boxRecords, v != 0)},
    {"stream_tiles_per_chunk", 1, 1024, 1, "stream_tiles_per_chunk must be 1..1024", CPF_OPT(streamState.tilesPerChunk, (int)v)},
    {"sort_key_bits", 0, 0, 0, nullptr, setSortKeyBits},
    {"stream_tail_fraction", 0, 1, 0, "stream_tail_fraction must be in [0, 1]", CPF_OPT(streamState.tailFraction, v)},
    {"coop_max_cells", 0, 1 << 24, 0, "coop_max_cells must be in [0, 2^24]", CPF_OPT(streamState.coopMaxCells, (int)v)},
    // (2, 3, 5 on an all-hex mesh: diagnostics -- what the mixed-mesh instantiations cost by themselves; same results.
    // 8: chosen by the library, "flat_walk".  -1, auto, sits right below the first mode)
    {"stream_lookup", cpf::kLookupLoop - 1, cpf::kLookupBox, 1, "stream_lookup must be -1 (auto) or 0 ... 6", CPF_OPT(streamState.lookup, (int)v)},
    {"stream_lookup_by_density", 0, 1, 1, "stream_lookup_by_density must be 0 or 1", CPF_OPT(streamState.densityLookup, (int)v)},
    {"sort_method", 0, 2, 2, "sort_method must be 2 (this library's radix sort) or 0 (hipcub's)", CPF_OPT(sortMethod, (int)v)},
    {"sort_curve", -1, 1, 1, "sort_curve must be -1 (by regime), 0 (cell id) or 1 (Morton rank)", CPF_OPT(sortCurve, (int)v)},
    {"vtu_binary", 0, 1, 1, "vtu_binary must be 0 or 1", CPF_OPT(vtuBinary, v != 0)},
    {"stream_debug", 0, 0, 0, nullptr, CPF_OPT(streamState.debug, (int)v)},
    {"stream_waves_per_cu", 0, 32, 1, "stream_waves_per_cu must be 0..32 (0 = auto)", CPF_OPT(streamState.wavesPerCU, (int)v)},
    {"sort_interval", 0, 1e9, 0, "sort_interval must be >= 0 (0 = never)", CPF_OPT(sortInterval, (int)v)},
    {"timing_stride", 1, 1e6, 1, "timing_stride must be an integer >= 1", CPF_OPT(timing.stride, (int)v)},
    {"stats", 0, 0, 0, nullptr, CPF_OPT(stats, v != 0)},
    {"nonplanar_tol", kTiny, kHuge, 0, "nonplanar_tol must be a positive number", CPF_OPT(nonplanarTol, v)},    // (> 0 and finite)
    {"split_nonplanar", 0, 1, 1, "split_nonplanar must be 0 or 1", CPF_OPT(splitNonplanar, v != 0)},
};
#undef CPF_OPT
}  // namespace
extern "C" {

int cpf_set_option(cpf_context* ctx, const char* key, double value) {
    CPF_REQUIRE(ctx, ctx && key, CPF_ERR_ARG, "null argument");
    for (const Option& o : kOptions) {
        if (std::strcmp(key, o.key) != 0) continue;
        CPF_REQUIRE(ctx, !o.message || (value >= o.lo && value <= o.hi && (o.step == 0 || std::fmod(value - o.lo, o.step) == 0)),
                    CPF_ERR_ARG, o.message);
        return o.set(ctx, value);
    }
    return fail(ctx, CPF_ERR_ARG, std::string("cpf_set_option: unknown key '") + key + "'");
}

}  // extern "C"   (helper for the other translation units, C++ linkage)
namespace cpf {
void set_context_error(cpf_context* ctx, const char* message) {
    if (ctx) ctx->err = message ? message : "";
}
}  // namespace cpf
extern "C" {

int cpf_step_kernel_name(cpf_context* ctx, double D, unsigned flags, char* buf, size_t bufBytes) {
    CPF_REQUIRE(ctx, ctx && buf && bufBytes > 0, CPF_ERR_ARG, "null argument");
    CPF_REQUIRE(ctx, ctx->mesh.have, CPF_ERR_STATE, "cpf_step_kernel_name: call cpf_set_mesh first");
    const cpf::MeshView m = meshView(ctx);
    const cpf::VertexField vf = vertexField(ctx);
    pollFieldFlag(ctx);
    // the plan of a launch with these flags.  A fused launch's kernel depends on how many cycles it fuses, the streaming
    // kernels' record lookup on the particle count: the most recent launch's stand in, else the owned cloud's (the
    // "VertexVelocity" cycle's also after a launch without particles)
    const bool vertexU = (flags & CPF_STEP_VERTEX_VELOCITY) != 0;
    const int64_t n = (vertexU ? ctx->lastStepN > 0 : ctx->lastStepN >= 0) ? ctx->lastStepN : ctx->cloud.n;
    const cpf::StepPlan p = cpf::plan_step(m, ctx->streamState, ctx->stepVariant, vertexU ? &vf : nullptr, n,
                                           (flags & CPF_STEP_FUSE_CYCLES) ? ctx->lastStepCycles : 1, D, flags, ctx->stats);
    const char* b[2] = {"false", "true"};
    char tmp[192];
    if (p.kernel == cpf::StepPlan::kStreamVertex)
        snprintf(tmp, sizeof tmp, "cpf::step_kernel_stream_vertex<%s, %s, %s, %s, %d> (cone locate)", b[p.brown], b[p.reflect],
                 b[p.storeVel], b[p.stats], p.lookup);
    else if (p.kernel == cpf::StepPlan::kVertex)
        snprintf(tmp, sizeof tmp, "cpf::step_kernel_vertex<%s, %s, %s> (%s)", b[p.brown], b[p.reflect], b[p.storeVel],
                 p.cone ? "cone locate" : (ctx->tet.cone || ctx->tet.coneWhy.empty() ? "all tets" : ("all tets: " + ctx->tet.coneWhy).c_str()));
    else if (p.kernel == cpf::StepPlan::kAhead)
        snprintf(tmp, sizeof tmp, "cpf::step_kernel_ahead<%s, %s>", b[p.reflect], b[p.stats]);
    else if (p.flat_body(ctx->streamState, ctx->cloud.zSettled) && !zBadArrived(ctx))       // (what cpf_step launches next on the context's own cloud)
        snprintf(tmp, sizeof tmp, "cpf::step_kernel_stream_flat<%s, %s, %s, %d>", b[p.reflect], b[p.storeVel], b[p.stats], p.lookup);
    else if (p.kernel == cpf::StepPlan::kStream)
        snprintf(tmp, sizeof tmp, "cpf::step_kernel_stream<%s, %s, %s, %s, %d>", b[p.brown], b[p.reflect], b[p.storeVel], b[p.stats], p.lookup);
    else if (p.kernel == cpf::StepPlan::kCoop)
        snprintf(tmp, sizeof tmp, "cpf::step_kernel_coop<%s, %s, %s, %s>", b[p.brown], b[p.reflect], b[p.storeVel], b[p.stats]);
    else snprintf(tmp, sizeof tmp, "cpf::step_kernel<%d, %s, %s, %s>", (int)p.kernel, b[p.brown], b[p.reflect], b[p.storeVel]);
    snprintf(buf, bufBytes, "%s", tmp);
    return CPF_OK;
}

int cpf_set_seed(cpf_context* ctx, uint32_t seed) {
    CPF_REQUIRE(ctx, ctx, CPF_ERR_ARG, "null context");
    ctx->seed = seed;
    return CPF_OK;
}

int cpf_pack_leavers_dev(cpf_context* ctx, double* x, double* y, double* z, int32_t* cell, int64_t* gid, int64_t n,
                         const int32_t* cellLo_dev, int nRanks, int myRank, double* sendbuf, int64_t sendCapacity,
                         int64_t* counts_dev, int64_t* nStay_dev) {
    CPF_REQUIRE(ctx, ctx, CPF_ERR_ARG, "null context");
    CPF_REQUIRE(ctx, n >= 0 && n < ((int64_t)1 << 31) && nRanks >= 1 && nRanks <= CPF_MAX_RANKS && myRank >= 0 && myRank < nRanks,
                CPF_ERR_ARG, "cpf_pack_leavers_dev: bad sizes (1 .. CPF_MAX_RANKS ranks)");
    CPF_REQUIRE(ctx, cellLo_dev && counts_dev && nStay_dev && (sendbuf || sendCapacity == 0) && (n == 0 || (x && y && z && cell)),
                CPF_ERR_ARG, "cpf_pack_leavers_dev: null array");
    CPF_REQUIRE(ctx, !ctx->mesh.parentOf, CPF_ERR_MESH, "cpf_pack_leavers_dev: the mesh has cells decomposed into tets "
                "(cpf_get_mesh_quality): ownership ranges are parent ids, the cloud's cells derived ids");
    CPF_HIP(ctx, hipSetDevice(ctx->device));
    int r = ensureScratch(ctx, cpf::handoff_scratch_bytes(n, nRanks));
    if (r) return r;
    CPF_HIP(ctx, cpf::pack_leavers(ctx->stream, x, y, z, cell, gid, n, cellLo_dev, nRanks, myRank, sendbuf,
                                   sendCapacity, counts_dev, nStay_dev, ctx->scratch, ctx->scratchBytes));
    return CPF_OK;
}

int cpf_cell_histogram_dev(cpf_context* ctx, const int32_t* cell, int64_t n, double scale, double* weights_dev) {
    CPF_REQUIRE(ctx, ctx, CPF_ERR_ARG, "null context");
    CPF_REQUIRE(ctx, ctx->mesh.have, CPF_ERR_STATE, "cpf_cell_histogram_dev: call cpf_set_mesh first");
    CPF_REQUIRE(ctx, n >= 0 && weights_dev && (cell || n == 0), CPF_ERR_ARG, "cpf_cell_histogram_dev: bad arguments");
    CPF_HIP(ctx, hipSetDevice(ctx->device));
    if (ctx->mesh.parentOf) {                             // weights per PARENT cell: the ids are mapped first, into the scratch's head
        const size_t head = ((size_t)n * 4 + 255) & ~(size_t)255;
        int r = ensureScratch(ctx, head + cpf::histogram_scratch_bytes(ctx->mesh.nParent));
        if (r != CPF_OK) return r;
        int32_t* parent = (int32_t*)ctx->scratch.get();
        CPF_HIP(ctx, cpf::launch_cells_to_parent(ctx->stream, cell, parent, ctx->mesh.parentOf, n, ctx->mesh.host.nCells));
        CPF_HIP(ctx, cpf::cell_histogram(ctx->stream, parent, n, ctx->mesh.nParent, scale, weights_dev, ctx->scratch + head,
                                         ctx->scratchBytes - head));
        return CPF_OK;
    }
    int r = ensureScratch(ctx, cpf::histogram_scratch_bytes(ctx->mesh.host.nCells));
    if (r != CPF_OK) return r;
    CPF_HIP(ctx, cpf::cell_histogram(ctx->stream, cell, n, ctx->mesh.host.nCells, scale, weights_dev, ctx->scratch,
                                     ctx->scratchBytes));
    return CPF_OK;
}

int cpf_occupancy_sample_dev(cpf_context* ctx, const int32_t* cell, int64_t n) {
    CPF_REQUIRE(ctx, ctx, CPF_ERR_ARG, "null context");
    CPF_REQUIRE(ctx, ctx->mesh.have, CPF_ERR_STATE, "cpf_occupancy_sample: call cpf_set_mesh first");
    CPF_REQUIRE(ctx, n >= 0 && (cell || n == 0), CPF_ERR_ARG, "cpf_occupancy_sample_dev: bad arguments");
    CPF_HIP(ctx, hipSetDevice(ctx->device));
    if (!ctx->mesh.occupancy) {                          // first use: allocated and zeroed
        DevBuf<unsigned long long> acc;
        CPF_HIP(ctx, acc.alloc((size_t)ctx->mesh.nParent));
        CPF_HIP(ctx, hipMemsetAsync(acc, 0, (size_t)ctx->mesh.nParent * 8, ctx->stream));
        ctx->mesh.occupancy = std::move(acc);
        ctx->mesh.occupancySamples = 0;
    }
    CPF_HIP(ctx, cpf::occupancy_accumulate(ctx->stream, cell, n, ctx->mesh.parentOf, ctx->mesh.host.nCells, ctx->mesh.occupancy));
    ++ctx->mesh.occupancySamples;
    return CPF_OK;
}

int cpf_occupancy_sample(cpf_context* ctx) {
    CPF_REQUIRE(ctx, ctx, CPF_ERR_ARG, "null context");
    CPF_REQUIRE(ctx, ctx->mesh.have, CPF_ERR_STATE, "cpf_occupancy_sample: call cpf_set_mesh first");
    CPF_REQUIRE(ctx, ctx->cloud.n > 0 && ctx->cloud.located, CPF_ERR_STATE, "cpf_occupancy_sample: no located particles");
    return cpf_occupancy_sample_dev(ctx, ctx->cloud.cur.cell, ctx->cloud.n);
}

int cpf_occupancy_reset(cpf_context* ctx) {
    CPF_REQUIRE(ctx, ctx, CPF_ERR_ARG, "null context");
    ctx->mesh.occupancySamples = 0;
    if (ctx->mesh.occupancy) {
        CPF_HIP(ctx, hipSetDevice(ctx->device));
        CPF_HIP(ctx, hipMemsetAsync(ctx->mesh.occupancy, 0, (size_t)ctx->mesh.nParent * 8, ctx->stream));
    }
    return CPF_OK;
}

int cpf_get_occupancy(cpf_context* ctx, uint64_t* counts, int64_t* nSamples) {
    CPF_REQUIRE(ctx, ctx, CPF_ERR_ARG, "null context");
    CPF_REQUIRE(ctx, ctx->mesh.have, CPF_ERR_STATE, "cpf_get_occupancy: call cpf_set_mesh first");
    if (nSamples) *nSamples = ctx->mesh.occupancySamples;
    if (counts && !ctx->mesh.occupancy) std::memset(counts, 0, (size_t)ctx->mesh.nParent * 8);      // before any sample
    if (ctx->mesh.occupancy) {
        CPF_HIP(ctx, hipSetDevice(ctx->device));
        if (counts) CPF_HIP(ctx, hipMemcpyAsync(counts, ctx->mesh.occupancy, (size_t)ctx->mesh.nParent * 8, hipMemcpyDeviceToHost, ctx->stream));
        CPF_HIP(ctx, hipStreamSynchronize(ctx->stream));
    }
    return CPF_OK;
}

// ---- recycling: sink cells and a source box (cpf_recycle.hip) ---------------------------------
int cpf_set_sink_cells(cpf_context* ctx, const int32_t* parentCells, int64_t n) {
    CPF_REQUIRE(ctx, ctx, CPF_ERR_ARG, "null context");
    CPF_REQUIRE(ctx, ctx->mesh.have, CPF_ERR_STATE, "cpf_set_sink_cells: call cpf_set_mesh first");
    CPF_REQUIRE(ctx, n >= 0 && (parentCells || n == 0), CPF_ERR_ARG, "cpf_set_sink_cells: bad arguments");
    for (int64_t k = 0; k < n; ++k)
        CPF_REQUIRE(ctx, parentCells[k] >= 0 && parentCells[k] < ctx->mesh.nParent, CPF_ERR_ARG,
                    "cpf_set_sink_cells: cell " + std::to_string(parentCells[k]) + " is not in [0, nCells)");
    CPF_HIP(ctx, hipSetDevice(ctx->device));
    CPF_HIP(ctx, hipStreamSynchronize(ctx->stream));        // (a pass over the old mask may still be running)
    ctx->mesh.sinkMask = DevBuf<uint32_t>{};
    // tagging: every cell of a plain sink set is in group 0 (cpf_set_sink_groups says otherwise)
    if (ctx->tags.on) CPF_HIP(ctx, hipMemset(ctx->tags.sinkGroup, 0, (size_t)ctx->mesh.host.nCells));
    if (n == 0) return CPF_OK;
    // one bit per DERIVED cell: every derived cell of a sink parent is set
    const int64_t nDerived = ctx->mesh.host.nCells;
    std::vector<uint32_t> mask((size_t)((nDerived + 31) / 32), 0u);
    const bool derived = !ctx->mesh.first.empty();
    for (int64_t k = 0; k < n; ++k) {
        const int64_t c = parentCells[k];
        const int64_t lo = derived ? ctx->mesh.first[(size_t)c] : c, hi = derived ? ctx->mesh.first[(size_t)c + 1] : c + 1;
        for (int64_t d = lo; d < hi; ++d) mask[(size_t)(d >> 5)] |= 1u << (d & 31);
    }
    DevBuf<uint32_t> dev;
    CPF_HIP(ctx, dev.alloc(mask.size()));
    CPF_HIP(ctx, hipMemcpy(dev, mask.data(), mask.size() * 4, hipMemcpyHostToDevice));
    ctx->mesh.sinkMask = std::move(dev);
    return CPF_OK;
}

int cpf_sink_apply_dev(cpf_context* ctx, int32_t* cell, int64_t n) {
    CPF_REQUIRE(ctx, ctx, CPF_ERR_ARG, "null context");
    CPF_REQUIRE(ctx, ctx->mesh.have, CPF_ERR_STATE, "cpf_sink_apply: call cpf_set_mesh first");
    CPF_REQUIRE(ctx, n >= 0 && (cell || n == 0), CPF_ERR_ARG, "cpf_sink_apply_dev: bad arguments");
    if (!ctx->mesh.sinkMask) return CPF_OK;                // no sink set: nothing runs
    CPF_HIP(ctx, hipSetDevice(ctx->device));
    int r = ensureRecycleCounts(ctx);
    if (r) return r;
    CPF_HIP(ctx, cpf::sink_apply(ctx->stream, cell, n, ctx->mesh.sinkMask, ctx->mesh.host.nCells, ctx->recycleCounts));
    return CPF_OK;
}

int cpf_sink_apply(cpf_context* ctx) {
    CPF_REQUIRE(ctx, ctx, CPF_ERR_ARG, "null context");
    CPF_REQUIRE(ctx, ctx->mesh.have, CPF_ERR_STATE, "cpf_sink_apply: call cpf_set_mesh first");
    CPF_REQUIRE(ctx, ctx->cloud.n > 0 && ctx->cloud.located, CPF_ERR_STATE, "cpf_sink_apply: no located particles");
    // the groups of the ledger that are on run their passes first; age's and route's mark and count as the plain pass does
    bool marked = false;
    if (int r = cpf::ledger_sink_passes(ctx, &marked)) return r;
    return marked ? CPF_OK : cpf_sink_apply_dev(ctx, ctx->cloud.cur.cell, ctx->cloud.n);
}

int cpf_respawn_box_dev(cpf_context* ctx, double* x, double* y, double* z, int32_t* cell, const int64_t* gid, int64_t n,
                        const double lower[3], const double upper[3], int64_t maxCount, uint32_t epoch) {
    CPF_REQUIRE(ctx, ctx, CPF_ERR_ARG, "null context");
    CPF_REQUIRE(ctx, ctx->mesh.have, CPF_ERR_STATE, "cpf_respawn_box: call cpf_set_mesh first");
    CPF_REQUIRE(ctx, lower && upper && n >= 0 && n < ((int64_t)1 << 31) && (n == 0 || (x && y && z && cell)), CPF_ERR_ARG,
                "cpf_respawn_box: bad arguments");
    for (int k = 0; k < 3; ++k)
        CPF_REQUIRE(ctx, std::isfinite(lower[k]) && std::isfinite(upper[k]) && upper[k] >= lower[k], CPF_ERR_ARG,
                    "cpf_respawn_box: the box needs finite bounds with upper >= lower on every axis");
    CPF_HIP(ctx, hipSetDevice(ctx->device));
    int r = ensureRecycleCounts(ctx);
    if (r) return r;
    const bool limited = maxCount > 0 && maxCount < n;
    if (limited) {
        r = ensureScratch(ctx, cpf::respawn_scratch_bytes(n));
        if (r) return r;
    }
    CPF_HIP(ctx, cpf::respawn_box(ctx->stream, x, y, z, cell, gid, n, lower, upper, maxCount, ctx->seed, epoch, meshView(ctx),
                                  gridView(ctx), ctx->scratch, ctx->scratchBytes, ctx->recycleCounts));
    return CPF_OK;
}

int cpf_respawn_box(cpf_context* ctx, const double lower[3], const double upper[3], int64_t maxCount) {
    CPF_REQUIRE(ctx, ctx, CPF_ERR_ARG, "null context");
    CPF_REQUIRE(ctx, ctx->mesh.have, CPF_ERR_STATE, "cpf_respawn_box: call cpf_set_mesh first");
    CPF_REQUIRE(ctx, ctx->cloud.n > 0 && ctx->cloud.located, CPF_ERR_STATE, "cpf_respawn_box: no located particles");
    bool boxOk = lower && upper;                    // (a box the respawn is about to refuse: no stamp either)
    for (int k = 0; k < 3 && boxOk; ++k) boxOk = std::isfinite(lower[k]) && std::isfinite(upper[k]) && upper[k] >= lower[k];
    // the ledger: every candidate is stamped now -- the ones this call leaves dead are stamped again by the call that places them
    if (boxOk && maxCount != 0)
        if (int r = cpf::ledger_respawn_stamps(ctx, false)) return r;
    int r = cpf_respawn_box_dev(ctx, ctx->cloud.cur.x, ctx->cloud.cur.y, ctx->cloud.cur.z, ctx->cloud.cur.cell, ctx->cloud.cur.gid,
                                ctx->cloud.n, lower, upper, maxCount, ctx->cloud.respawnEpoch);
    if (r) return r;
    ctx->cloud.zSettled = false;                    // (a respawned particle is live again, with a z the flat cycle never settled)
    ++ctx->cloud.respawnEpoch;
    return CPF_OK;
}

int cpf_get_recycle_counts(cpf_context* ctx, int64_t out[4]) {
    CPF_REQUIRE(ctx, ctx && out, CPF_ERR_ARG, "null argument");
    unsigned long long h[3] = {0, 0, 0};
    CPF_HIP(ctx, hipSetDevice(ctx->device));
    if (ctx->recycleCounts) CPF_HIP(ctx, hipMemcpyAsync(h, ctx->recycleCounts, sizeof h, hipMemcpyDeviceToHost, ctx->stream));
    CPF_HIP(ctx, hipStreamSynchronize(ctx->stream));
    for (int k = 0; k < 3; ++k) out[k] = (int64_t)h[k];
    out[3] = (int64_t)ctx->cloud.respawnEpoch;
    return CPF_OK;
}

int cpf_recycle_reset_counts(cpf_context* ctx) {
    CPF_REQUIRE(ctx, ctx, CPF_ERR_ARG, "null context");
    if (ctx->recycleCounts) {
        CPF_HIP(ctx, hipSetDevice(ctx->device));
        CPF_HIP(ctx, hipMemsetAsync(ctx->recycleCounts, 0, 4 * 8, ctx->stream));
    }
    return CPF_OK;
}

int cpf_respawn_positions_host(uint32_t seed, const int64_t* gid, int64_t n, uint32_t epoch, const double lower[3],
                               const double upper[3], double* xyz) {
    if (n < 0 || !lower || !upper || (n > 0 && !xyz)) return CPF_ERR_ARG;
    for (int64_t i = 0; i < n; ++i) cpf::respawn_position(seed, (uint64_t)(gid ? gid[i] : i), epoch, lower, upper, xyz + 3 * i);
    return CPF_OK;
}

// ---- patch source: dead slots respawn on weighted triangles (cpf_inlet.hip; the position: cpf_philox.h) ---------------------
int cpf_source_table_host(const double* tri, const double* weight, const double* depth, double d0, double d1, int64_t n,
                          double* rec, uint32_t* hi, int64_t* nKept) {
    if (!nKept || n < 0 || (n > 0 && !tri)) return CPF_ERR_ARG;
    *nKept = 0;
    if (!depth && !(std::isfinite(d0) && std::isfinite(d1) && d0 <= d1)) return CPF_ERR_ARG;
    // per triangle, every operation rounded on its own: e1 = B - A, e2 = C - A, c = e1 x e2, len = sqrt(c.c)
    struct Geo { double e1[3], e2[3], c[3], len; };
    const auto geometry = [tri](int64_t t) {
        const double *A = tri + 9 * t, *B = A + 3, *C = A + 6;
        Geo g;
        for (int a = 0; a < 3; ++a) { g.e1[a] = B[a] - A[a]; g.e2[a] = C[a] - A[a]; }
        for (int a = 0; a < 3; ++a) {
            const int b = (a + 1) % 3, d = (a + 2) % 3;
            const double p = g.e1[b] * g.e2[d], q = g.e1[d] * g.e2[b];
            g.c[a] = p - q;
        }
        const double xx = g.c[0] * g.c[0], yy = g.c[1] * g.c[1], zz = g.c[2] * g.c[2];
        const double xy = xx + yy;
        g.len = std::sqrt(xy + zz);
        return g;
    };
    struct Kept { int64_t t; double sum; };                // a kept triangle and the running sum C_t of the kept weights
    std::vector<Kept> kept;
    double sum = 0.0;
    for (int64_t t = 0; t < n; ++t) {
        if (depth && !(std::isfinite(depth[2 * t]) && std::isfinite(depth[2 * t + 1]) && depth[2 * t] <= depth[2 * t + 1]))
            return CPF_ERR_ARG;
        const double len = geometry(t).len;
        const double area = len / 2.0;
        const double w = weight ? weight[t] : area;
        if (!(std::isfinite(w) && w >= 0.0)) return CPF_ERR_ARG;
        if (len == 0.0 || w == 0.0) continue;
        if (!std::isfinite(len)) return CPF_ERR_ARG;
        sum = sum + w;
        kept.push_back({t, sum});
    }
    if (kept.empty() || !std::isfinite(sum)) return CPF_ERR_ARG;
    // b_t = floor(C_t / C_last * 2^32), the last one 2^32; a triangle whose bound is its predecessor's has a share below 2^-32
    int64_t m = 0;
    uint64_t before = 0;
    const uint64_t full = (uint64_t)1 << 32;
    for (size_t i = 0; i < kept.size(); ++i) {
        const Kept& k = kept[i];
        const double share = k.sum / sum;
        uint64_t b = i + 1 == kept.size() ? full : (uint64_t)std::floor(share * 4294967296.0);
        if (b > full) b = full;
        if (b == before) continue;
        before = b;
        if (m >= ((int64_t)1 << 24)) return CPF_ERR_ARG;
        if (hi) hi[m] = (uint32_t)(b - 1);
        if (rec) {
            double* r = rec + cpf::kSourceDoubles * m;
            const double* A = tri + 9 * k.t;
            const Geo g = geometry(k.t);
            for (int a = 0; a < 3; ++a) { r[a] = A[a]; r[3 + a] = g.e1[a]; r[6 + a] = g.e2[a]; r[9 + a] = -g.c[a] / g.len; }
            const double lo = depth ? depth[2 * k.t] : d0, up = depth ? depth[2 * k.t + 1] : d1;
            r[12] = lo; r[13] = up - lo; r[14] = (double)k.t; r[15] = 0.0;
        }
        ++m;
    }
    *nKept = m;
    return CPF_OK;
}

int cpf_source_positions_host(uint32_t seed, const int64_t* gid, int64_t n, uint32_t epoch, const double* rec, const uint32_t* hi,
                              int64_t nKept, double* xyz) {
    if (n < 0 || !rec || !hi || nKept <= 0 || nKept > ((int64_t)1 << 24) || hi[nKept - 1] != 0xFFFFFFFFu || (n > 0 && !xyz))
        return CPF_ERR_ARG;
    for (int64_t i = 0; i < n; ++i) {
        uint32_t c[4];
        cpf::source_words(seed, (uint64_t)(gid ? gid[i] : i), epoch, c);
        const int t = cpf::source_pick(hi, (int)nKept, c[0]);
        cpf::source_point(c, rec + cpf::kSourceDoubles * (int64_t)t, xyz + 3 * i);
    }
    return CPF_OK;
}

int cpf_set_source_triangles(cpf_context* ctx, const double* tri, const double* weight, const double* depth, double d0, double d1,
                             int64_t n) {
    CPF_REQUIRE(ctx, ctx, CPF_ERR_ARG, "null context");
    CPF_REQUIRE(ctx, ctx->mesh.have, CPF_ERR_STATE, "cpf_set_source_triangles: call cpf_set_mesh first");
    CPF_REQUIRE(ctx, n >= 0 && (tri || n == 0), CPF_ERR_ARG, "cpf_set_source_triangles: bad arguments");
    std::vector<double> rec((size_t)n * cpf::kSourceDoubles);
    std::vector<uint32_t> hi((size_t)n + 4);
    int64_t kept = 0;
    if (n > 0)
        CPF_REQUIRE(ctx, cpf_source_table_host(tri, weight, depth, d0, d1, n, rec.data(), hi.data(), &kept) == CPF_OK, CPF_ERR_ARG,
                    "cpf_set_source_triangles: weights must be finite and >= 0, depths finite with d0 <= d1, and between 1 and 2^24 "
                    "triangles must keep a share of at least 2^-32");
    CPF_HIP(ctx, hipSetDevice(ctx->device));
    CPF_HIP(ctx, hipStreamSynchronize(ctx->stream));        // (a pass over the old table may still be running)
    ctx->mesh.sourceRec = DevBuf<double>{};
    ctx->mesh.sourceHi = DevBuf<uint32_t>{};
    ctx->mesh.sourceKept = 0;
    ctx->mesh.sourceRecHost.clear();
    ctx->mesh.sourceHiHost.clear();
    ctx->mesh.follow = SourceFollow{};                      // (a new table does not follow U until cpf_source_follow says so)
    ctx->tags.originOfKept = DevBuf<uint8_t>{};
    if (n == 0) return CPF_OK;
    DevBuf<uint8_t> dOrigin;                                // tagging: a new source starts with every triangle in origin 0
    if (ctx->tags.on) {
        CPF_HIP(ctx, dOrigin.alloc((size_t)kept));
        CPF_HIP(ctx, hipMemset(dOrigin, 0, (size_t)kept));
    }
    rec.resize((size_t)kept * cpf::kSourceDoubles);
    const size_t padded = ((size_t)kept + 3) / 4 * 4;
    hi.resize(padded);
    for (size_t i = (size_t)kept; i < padded; ++i) hi[i] = 0xFFFFFFFFu;
    DevBuf<double> dRec;
    DevBuf<uint32_t> dHi;
    CPF_HIP(ctx, dRec.alloc(rec.size()));
    CPF_HIP(ctx, dHi.alloc(hi.size()));
    CPF_HIP(ctx, hipMemcpy(dRec, rec.data(), rec.size() * sizeof(double), hipMemcpyHostToDevice));
    CPF_HIP(ctx, hipMemcpy(dHi, hi.data(), hi.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
    hi.resize((size_t)kept);
    ctx->mesh.sourceRec = std::move(dRec);
    ctx->mesh.sourceHi = std::move(dHi);
    ctx->mesh.sourceKept = kept;
    ctx->mesh.sourceRecHost = std::move(rec);
    ctx->mesh.sourceHiHost = std::move(hi);
    ctx->tags.originOfKept = std::move(dOrigin);
    return CPF_OK;
}

int cpf_get_source_table(cpf_context* ctx, double* rec, uint32_t* hi, int64_t* nKept) {
    CPF_REQUIRE(ctx, ctx && nKept, CPF_ERR_ARG, "null argument");
    *nKept = ctx->mesh.sourceKept;
    if (ctx->mesh.follow.on) {                              // the table lives on the device: the host copies are the table as built
        CPF_HIP(ctx, hipSetDevice(ctx->device));
        CPF_HIP(ctx, hipStreamSynchronize(ctx->stream));
        const size_t k = (size_t)ctx->mesh.sourceKept;
        if (rec) CPF_HIP(ctx, hipMemcpy(rec, ctx->mesh.sourceRec, k * cpf::kSourceDoubles * sizeof(double), hipMemcpyDeviceToHost));
        if (hi) CPF_HIP(ctx, hipMemcpy(hi, ctx->mesh.sourceHi, k * sizeof(uint32_t), hipMemcpyDeviceToHost));
        return CPF_OK;
    }
    if (rec) std::copy(ctx->mesh.sourceRecHost.begin(), ctx->mesh.sourceRecHost.end(), rec);
    if (hi) std::copy(ctx->mesh.sourceHiHost.begin(), ctx->mesh.sourceHiHost.end(), hi);
    return CPF_OK;
}

// ---- flux table: the source's bounds and depths follow U (cpf_inflow.hip; the arithmetic: cpf_inflow.h) ----------------------
namespace {
// len of a kept record from its e1, e2, exactly as cpf_source_table_host computes it
double sourceRecordLen(const double* r) {
    const double *e1 = r + 3, *e2 = r + 6;
    double c[3];
    for (int a = 0; a < 3; ++a) {
        const int b = (a + 1) % 3, d = (a + 2) % 3;
        const double p = e1[b] * e2[d], q = e1[d] * e2[b];
        c[a] = p - q;
    }
    const double xx = c[0] * c[0], yy = c[1] * c[1], zz = c[2] * c[2];
    const double xy = xx + yy;
    return std::sqrt(xy + zz);
}
}  // namespace

int cpf_source_flux_host(const double* rec, int64_t nKept, const int32_t* cellOfTriangle, int64_t nTriangles, const double* U,
                         int64_t nCells, double depthScale, double* span, uint32_t* hi, uint64_t* q, int32_t* empty) {
    if (!rec || !cellOfTriangle || !U || !empty || nKept <= 0 || nKept > ((int64_t)1 << 24) || nTriangles <= 0 || nCells <= 0 ||
        !(std::isfinite(depthScale) && depthScale >= 0.0))
        return CPF_ERR_ARG;
    std::vector<cpf::InflowTerm> term((size_t)nKept);
    uint64_t wmaxBits = 0;                                  // (non-negative doubles order like their bits)
    for (int64_t k = 0; k < nKept; ++k) {
        const double* r = rec + cpf::kSourceDoubles * k;
        if (!(r[14] >= 0.0 && r[14] < (double)nTriangles)) return CPF_ERR_ARG;
        const int64_t c = cellOfTriangle[(int64_t)r[14]];
        if (c < 0 || c >= nCells) return CPF_ERR_ARG;
        const double area = sourceRecordLen(r) / 2.0;
        term[(size_t)k] = cpf::inflow_term(U[3 * c], U[3 * c + 1], U[3 * c + 2], r[9], r[10], r[11], area, depthScale);
        wmaxBits = std::max(wmaxBits, cpf::inflow_bits(term[(size_t)k].w));
    }
    *empty = wmaxBits == 0 ? 1 : 0;
    if (wmaxBits == 0) return CPF_OK;
    double wmax;
    std::memcpy(&wmax, &wmaxBits, 8);
    const int E = cpf::inflow_exponent(wmax);
    uint64_t last = 0;
    for (int64_t k = 0; k < nKept; ++k) last += cpf::inflow_quantum(term[(size_t)k].w, E);
    uint64_t Q = 0;
    for (int64_t k = 0; k < nKept; ++k) {
        const uint64_t qk = cpf::inflow_quantum(term[(size_t)k].w, E);
        Q += qk;
        if (q) q[k] = qk;
        if (hi) hi[k] = cpf::inflow_bound(Q, last);
        if (span) span[k] = term[(size_t)k].span;
    }
    return CPF_OK;
}

int cpf_source_follow(cpf_context* ctx, const int32_t* cellOfTriangle, int64_t nTriangles, double depthScale) {
    CPF_REQUIRE(ctx, ctx, CPF_ERR_ARG, "null context");
    CPF_REQUIRE(ctx, ctx->mesh.have, CPF_ERR_STATE, "cpf_source_follow: call cpf_set_mesh first");
    CPF_REQUIRE(ctx, ctx->mesh.sourceKept > 0, CPF_ERR_STATE, "cpf_source_follow: call cpf_set_source_triangles first");
    CPF_REQUIRE(ctx, cellOfTriangle && nTriangles > 0, CPF_ERR_ARG, "cpf_source_follow: bad arguments");
    CPF_REQUIRE(ctx, std::isfinite(depthScale) && depthScale >= 0.0, CPF_ERR_ARG,
                "cpf_source_follow: depthScale must be finite and >= 0");
    for (int64_t t = 0; t < nTriangles; ++t)
        CPF_REQUIRE(ctx, cellOfTriangle[t] >= 0 && cellOfTriangle[t] < ctx->mesh.nParent, CPF_ERR_ARG,
                    "cpf_source_follow: cell " + std::to_string(cellOfTriangle[t]) + " is not in [0, nCells)");
    // per kept record: the area, and the owner as a cell of the mesh the walk runs on (any derived cell carries its parent's U)
    const size_t kept = (size_t)ctx->mesh.sourceKept;
    const bool derived = !ctx->mesh.first.empty();
    std::vector<double> area(kept);
    std::vector<int32_t> owner(kept);
    for (size_t k = 0; k < kept; ++k) {
        const double* r = &ctx->mesh.sourceRecHost[k * cpf::kSourceDoubles];
        const int64_t t = (int64_t)r[14];
        CPF_REQUIRE(ctx, t >= 0 && t < nTriangles, CPF_ERR_ARG,
                    "cpf_source_follow: the source has a triangle " + std::to_string(t) + ", beyond nTriangles");
        area[k] = sourceRecordLen(r) / 2.0;
        const int32_t c = cellOfTriangle[t];
        owner[k] = derived ? ctx->mesh.first[(size_t)c] : c;
    }
    CPF_HIP(ctx, hipSetDevice(ctx->device));
    CPF_HIP(ctx, hipStreamSynchronize(ctx->stream));        // (a refresh from the old state may still be running)
    SourceFollow f;
    const size_t nBlocks = (size_t)cpf::inflow_blocks((int64_t)kept);
    CPF_HIP(ctx, f.area.alloc(kept));
    CPF_HIP(ctx, f.owner.alloc(kept));
    CPF_HIP(ctx, f.w.alloc(2 * kept));
    CPF_HIP(ctx, f.sums.alloc(2 * nBlocks));
    CPF_HIP(ctx, f.slots.alloc(4));
    CPF_HIP(ctx, hipMemcpy(f.area, area.data(), kept * sizeof(double), hipMemcpyHostToDevice));
    CPF_HIP(ctx, hipMemcpy(f.owner, owner.data(), kept * sizeof(int32_t), hipMemcpyHostToDevice));
    CPF_HIP(ctx, hipMemset(f.slots, 0, 4 * 8));
    f.on = true;
    f.depthScale = depthScale;
    ctx->mesh.follow = std::move(f);
    if (ctx->mesh.haveU) CPF_HIP(ctx, refreshSource(ctx, reinterpret_cast<const double*>(ctx->mesh.U.get()), 4));
    return CPF_OK;
}

int cpf_source_unfollow(cpf_context* ctx) {
    CPF_REQUIRE(ctx, ctx, CPF_ERR_ARG, "null context");
    if (!ctx->mesh.follow.on) return CPF_OK;
    CPF_HIP(ctx, hipSetDevice(ctx->device));
    CPF_HIP(ctx, hipStreamSynchronize(ctx->stream));        // (a refresh may still be running)
    // the table stays as last refreshed, on the host too from now on
    const size_t k = (size_t)ctx->mesh.sourceKept;
    CPF_HIP(ctx, hipMemcpy(ctx->mesh.sourceRecHost.data(), ctx->mesh.sourceRec, k * cpf::kSourceDoubles * sizeof(double), hipMemcpyDeviceToHost));
    CPF_HIP(ctx, hipMemcpy(ctx->mesh.sourceHiHost.data(), ctx->mesh.sourceHi, k * sizeof(uint32_t), hipMemcpyDeviceToHost));
    ctx->mesh.follow = SourceFollow{};
    return CPF_OK;
}

int cpf_source_refresh(cpf_context* ctx) {
    CPF_REQUIRE(ctx, ctx, CPF_ERR_ARG, "null context");
    CPF_REQUIRE(ctx, ctx->mesh.follow.on, CPF_ERR_STATE, "cpf_source_refresh: call cpf_source_follow first");
    CPF_REQUIRE(ctx, ctx->mesh.haveU, CPF_ERR_STATE, "cpf_source_refresh: call cpf_set_velocity first");
    CPF_HIP(ctx, hipSetDevice(ctx->device));
    CPF_HIP(ctx, refreshSource(ctx, reinterpret_cast<const double*>(ctx->mesh.U.get()), 4));
    return CPF_OK;
}

int cpf_get_source_follow(cpf_context* ctx, int64_t out[3]) {
    CPF_REQUIRE(ctx, ctx && out, CPF_ERR_ARG, "null argument");
    unsigned long long skipped = 0;
    CPF_HIP(ctx, hipSetDevice(ctx->device));
    if (ctx->mesh.follow.on)
        CPF_HIP(ctx, hipMemcpyAsync(&skipped, ctx->mesh.follow.slots + 2, 8, hipMemcpyDeviceToHost, ctx->stream));
    CPF_HIP(ctx, hipStreamSynchronize(ctx->stream));
    out[0] = ctx->mesh.follow.on ? 1 : 0;
    out[1] = ctx->mesh.follow.refreshes;
    out[2] = (int64_t)skipped;
    return CPF_OK;
}

int cpf_respawn_source_dev(cpf_context* ctx, double* x, double* y, double* z, int32_t* cell, const int64_t* gid, int64_t n,
                           int64_t maxCount, uint32_t epoch) {
    CPF_REQUIRE(ctx, ctx, CPF_ERR_ARG, "null context");
    CPF_REQUIRE(ctx, ctx->mesh.have, CPF_ERR_STATE, "cpf_respawn_source: call cpf_set_mesh first");
    CPF_REQUIRE(ctx, ctx->mesh.sourceKept > 0, CPF_ERR_STATE, "cpf_respawn_source: call cpf_set_source_triangles first");
    CPF_REQUIRE(ctx, n >= 0 && n < ((int64_t)1 << 31) && (n == 0 || (x && y && z && cell)), CPF_ERR_ARG,
                "cpf_respawn_source: bad arguments");
    CPF_HIP(ctx, hipSetDevice(ctx->device));
    int r = ensureRecycleCounts(ctx);
    if (r) return r;
    if (maxCount > 0 && maxCount < n) {
        r = ensureScratch(ctx, cpf::respawn_scratch_bytes(n));
        if (r) return r;
    }
    const cpf::SourceView src{ctx->mesh.sourceRec, ctx->mesh.sourceHi, (int32_t)ctx->mesh.sourceKept};
    CPF_HIP(ctx, cpf::respawn_source(ctx->stream, x, y, z, cell, gid, n, src, maxCount, ctx->seed, epoch, meshView(ctx), gridView(ctx),
                                     ctx->scratch, ctx->scratchBytes, ctx->recycleCounts));
    return CPF_OK;
}

int cpf_respawn_source(cpf_context* ctx, int64_t maxCount) {
    CPF_REQUIRE(ctx, ctx, CPF_ERR_ARG, "null context");
    CPF_REQUIRE(ctx, ctx->mesh.have, CPF_ERR_STATE, "cpf_respawn_source: call cpf_set_mesh first");
    CPF_REQUIRE(ctx, ctx->mesh.sourceKept > 0, CPF_ERR_STATE, "cpf_respawn_source: call cpf_set_source_triangles first");
    CPF_REQUIRE(ctx, ctx->cloud.n > 0 && ctx->cloud.located, CPF_ERR_STATE, "cpf_respawn_source: no located particles");
    if (maxCount != 0)                              // (the ledger's stamps, as in cpf_respawn_box)
        if (int r = cpf::ledger_respawn_stamps(ctx, true)) return r;
    int r = cpf_respawn_source_dev(ctx, ctx->cloud.cur.x, ctx->cloud.cur.y, ctx->cloud.cur.z, ctx->cloud.cur.cell, ctx->cloud.cur.gid,
                                   ctx->cloud.n, maxCount, ctx->cloud.respawnEpoch);
    if (r) return r;
    ctx->cloud.zSettled = false;                    // (as behind cpf_respawn_box)
    ++ctx->cloud.respawnEpoch;
    return CPF_OK;
}

int cpf_source_picks_host(uint32_t seed, const int64_t* gid, int64_t n, uint32_t epoch, const uint32_t* hi, int64_t nKept,
                          int32_t* pick) {
    if (n < 0 || !hi || nKept <= 0 || nKept > ((int64_t)1 << 24) || hi[nKept - 1] != 0xFFFFFFFFu || (n > 0 && !pick)) return CPF_ERR_ARG;
    for (int64_t i = 0; i < n; ++i) {
        uint32_t c[4];
        cpf::source_words(seed, (uint64_t)(gid ? gid[i] : i), epoch, c);
        pick[i] = cpf::source_pick(hi, (int)nKept, c[0]);
    }
    return CPF_OK;
}

int cpf_cell_ranges_dev(cpf_context* ctx, const double* weights_dev, int nRanks, int32_t* cellLo_dev) {
    CPF_REQUIRE(ctx, ctx, CPF_ERR_ARG, "null context");
    CPF_REQUIRE(ctx, ctx->mesh.have, CPF_ERR_STATE, "cpf_cell_ranges_dev: call cpf_set_mesh first");
    CPF_REQUIRE(ctx, weights_dev && cellLo_dev && nRanks >= 1 && nRanks <= CPF_MAX_RANKS, CPF_ERR_ARG,
                "cpf_cell_ranges_dev: bad arguments (1 <= nRanks <= CPF_MAX_RANKS)");
    CPF_HIP(ctx, hipSetDevice(ctx->device));
    CPF_HIP(ctx, cpf::cell_ranges(ctx->stream, weights_dev, ctx->mesh.nParent, nRanks, cellLo_dev));   // (weights: per parent cell)
    return CPF_OK;
}

int cpf_unpack_arrivals_dev(cpf_context* ctx, double* x, double* y, double* z, int32_t* cell, int64_t* gid,
                            int64_t nStay, const double* recvbuf, int64_t nRecv) {
    CPF_REQUIRE(ctx, ctx, CPF_ERR_ARG, "null context");
    CPF_REQUIRE(ctx, nStay >= 0 && nRecv >= 0 && (nRecv == 0 || (x && y && z && cell && recvbuf)), CPF_ERR_ARG,
                "cpf_unpack_arrivals_dev: bad arguments");
    CPF_HIP(ctx, hipSetDevice(ctx->device));
    CPF_HIP(ctx, cpf::unpack_arrivals(ctx->stream, x, y, z, cell, gid, nStay, recvbuf, nRecv));
    return CPF_OK;
}

// ---- device memory helpers ------------------------------------------------------------------
int cpf_dev_alloc(cpf_context* ctx, size_t bytes, void** out) {
    CPF_REQUIRE(ctx, ctx && out, CPF_ERR_ARG, "null argument");
    *out = nullptr;
    CPF_HIP(ctx, hipSetDevice(ctx->device));
    CPF_HIP(ctx, hipMalloc(out, std::max<size_t>(bytes, 16)));
    return CPF_OK;
}
int cpf_dev_free(cpf_context* ctx, void* ptr) {
    CPF_REQUIRE(ctx, ctx, CPF_ERR_ARG, "null context");
    if (!ptr) return CPF_OK;
    CPF_HIP(ctx, hipSetDevice(ctx->device));
    CPF_HIP(ctx, hipStreamSynchronize(ctx->stream));
    CPF_HIP(ctx, hipFree(ptr));
    return CPF_OK;
}
int cpf_dev_memset(cpf_context* ctx, void* ptr, int value, size_t bytes) {
    CPF_REQUIRE(ctx, ctx && (ptr || bytes == 0), CPF_ERR_ARG, "null argument");
    CPF_HIP(ctx, hipSetDevice(ctx->device));
    if (bytes) CPF_HIP(ctx, hipMemsetAsync(ptr, value, bytes, ctx->stream));
    return CPF_OK;
}
int cpf_copy_to_device(cpf_context* ctx, void* dst, const void* src, size_t bytes) {
    CPF_REQUIRE(ctx, ctx && ((dst && src) || bytes == 0), CPF_ERR_ARG, "null argument");
    CPF_HIP(ctx, hipSetDevice(ctx->device));
    if (bytes) {
        CPF_HIP(ctx, hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, ctx->stream));
        CPF_HIP(ctx, hipStreamSynchronize(ctx->stream));
    }
    return CPF_OK;
}
int cpf_copy_to_host(cpf_context* ctx, void* dst, const void* src, size_t bytes) {
    CPF_REQUIRE(ctx, ctx && ((dst && src) || bytes == 0), CPF_ERR_ARG, "null argument");
    CPF_HIP(ctx, hipSetDevice(ctx->device));
    if (bytes) {
        CPF_HIP(ctx, hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, ctx->stream));
        CPF_HIP(ctx, hipStreamSynchronize(ctx->stream));
    }
    return CPF_OK;
}

int cpf_copy_dev(cpf_context* ctx, void* dst, const void* src, size_t bytes) {
    CPF_REQUIRE(ctx, ctx && ((dst && src) || bytes == 0), CPF_ERR_ARG, "null argument");
    CPF_HIP(ctx, hipSetDevice(ctx->device));
    if (bytes) CPF_HIP(ctx, hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, ctx->stream));
    return CPF_OK;
}

// ---- stage-by-stage entry points (reference layouts) --------------------------------------------
#define CPF_STAGE_PRE(name, needU)                                                                      \
    CPF_REQUIRE(ctx, ctx, CPF_ERR_ARG, "null context");                                                 \
    CPF_REQUIRE(ctx, ctx->mesh.have, CPF_ERR_STATE, name ": call cpf_set_mesh first");                   \
    CPF_REQUIRE(ctx, !ctx->mesh.parentOf, CPF_ERR_MESH, name ": the mesh has warped or concave cells decomposed " \
                "into tets (cpf_get_mesh_quality); the reference-layout stages take the mesh's own cells only"); \
    CPF_REQUIRE(ctx, !(needU) || ctx->mesh.haveU, CPF_ERR_STATE, name ": call cpf_set_velocity first");      \
    CPF_REQUIRE(ctx, n >= 0, CPF_ERR_ARG, name ": negative particle count");                            \
    CPF_HIP(ctx, hipSetDevice(ctx->device))

int cpf_stage_seed_box(cpf_context* ctx, double* particles, int64_t n, const double lower[3], const double upper[3],
                       int order) {
    CPF_REQUIRE(ctx, ctx, CPF_ERR_ARG, "null context");
    CPF_REQUIRE(ctx, n >= 0 && lower && upper && (particles || n == 0), CPF_ERR_ARG, "cpf_stage_seed_box: bad arguments");
    CPF_HIP(ctx, hipSetDevice(ctx->device));
    int r = ensureScratch(ctx, (size_t)std::max<int64_t>(n, 1) * 24);
    if (r) return r;
    double* x = (double*)ctx->scratch.get(); double* y = x + n; double* z = y + n;
    CPF_HIP(ctx, cpf::launch_seed_box(ctx->stream, x, y, z, 0, n, lower, upper, order));
    CPF_HIP(ctx, cpf::launch_soa_to_aos(ctx->stream, x, y, z, particles, n));
    return CPF_OK;
}
int cpf_stage_locate_initial(cpf_context* ctx, const double* particles, int32_t* ids, int64_t n) {
    CPF_STAGE_PRE("cpf_stage_locate_initial", false);
    CPF_REQUIRE(ctx, n == 0 || (particles && ids), CPF_ERR_ARG, "cpf_stage_locate_initial: null array");
    int r = ensureScratch(ctx, (size_t)std::max<int64_t>(n, 1) * 24);
    if (r) return r;
    double* x = (double*)ctx->scratch.get(); double* y = x + n; double* z = y + n;
    CPF_HIP(ctx, cpf::launch_aos_to_soa(ctx->stream, particles, x, y, z, n));
    CPF_HIP(ctx, cpf::launch_locate_initial(ctx->stream, x, y, z, ids, n, meshView(ctx), gridView(ctx)));
    return CPF_OK;
}
int cpf_stage_count_outside(cpf_context* ctx, const int32_t* ids, int64_t n, int64_t* nNegative) {
    CPF_REQUIRE(ctx, ctx && nNegative && (ids || n == 0) && n >= 0, CPF_ERR_ARG, "cpf_stage_count_outside: bad arguments");
    CPF_HIP(ctx, hipSetDevice(ctx->device));
    return countNegative(ctx, ids, n, nNegative);
}
int cpf_stage_advect(cpf_context* ctx, double* particles, const int32_t* ids, double* vels, double* disps, double dt,
                     int64_t n) {
    CPF_STAGE_PRE("cpf_stage_advect", true);
    CPF_REQUIRE(ctx, n == 0 || (particles && ids && vels && disps), CPF_ERR_ARG, "cpf_stage_advect: null array");
    CPF_HIP(ctx, cpf::launch_stage_advect(ctx->stream, particles, ids, vels, disps, dt, n, meshView(ctx)));
    return CPF_OK;
}
int cpf_stage_advect_const(cpf_context* ctx, double* particles, const int32_t* ids, const double* vels, double* disps, double dt,
                           int64_t n) {
    CPF_STAGE_PRE("cpf_stage_advect_const", false);
    CPF_REQUIRE(ctx, n == 0 || (particles && ids && vels && disps), CPF_ERR_ARG, "cpf_stage_advect_const: null array");
    CPF_HIP(ctx, cpf::launch_stage_advect_const(ctx->stream, particles, ids, vels, disps, dt, n));
    return CPF_OK;
}
int cpf_set_tets(cpf_context* ctx, const double* positions, int64_t nVerts, const int32_t* tets, int64_t nTets,
                 int tetsPerCell) {
    CPF_REQUIRE(ctx, ctx, CPF_ERR_ARG, "null context");
    CPF_REQUIRE(ctx, ctx->mesh.have, CPF_ERR_STATE, "cpf_set_tets: call cpf_set_mesh first");
    CPF_REQUIRE(ctx, !ctx->mesh.parentOf, CPF_ERR_MESH, "cpf_set_tets: the mesh has warped or concave cells decomposed into tets "
                "(cpf_get_mesh_quality); the \"VertexVelocity\" mode needs the mesh's own cells (set option \"split_nonplanar\" 0)");
    CPF_REQUIRE(ctx, positions && tets && nVerts > 0 && tetsPerCell > 0, CPF_ERR_ARG, "cpf_set_tets: bad arguments");
    CPF_REQUIRE(ctx, nTets == (int64_t)tetsPerCell * ctx->mesh.host.nCells, CPF_ERR_MESH,
                "cpf_set_tets: nTets must be tetsPerCell x nCells (tets in cell order, src/initCuda.H:99-105)");
    for (int64_t k = 0; k < 4 * nTets; ++k)
        CPF_REQUIRE(ctx, tets[k] >= 0 && tets[k] < nVerts, CPF_ERR_MESH, "cpf_set_tets: tet vertex out of range");
    CPF_HIP(ctx, hipSetDevice(ctx->device));
    CPF_HIP(ctx, hipStreamSynchronize(ctx->stream));
    ctx->tet = TetField{};
    // built into a local and moved in once nothing can fail any more: a call that fails leaves the context without a tet
    // field -- never with nTets set, a lone cone table or unbuilt records for cpf_set_vertex_velocity to write into
    TetField t;
    CPF_HIP(ctx, t.pos.alloc((size_t)nVerts * 3));
    CPF_HIP(ctx, t.tets.alloc((size_t)nTets * 4));
    CPF_HIP(ctx, t.vel.alloc((size_t)nVerts * 3));
    CPF_HIP(ctx, hipMemcpyAsync(t.pos, positions, (size_t)nVerts * 24, hipMemcpyHostToDevice, ctx->stream));
    CPF_HIP(ctx, hipMemcpyAsync(t.tets, tets, (size_t)nTets * 16, hipMemcpyHostToDevice, ctx->stream));
    CPF_HIP(ctx, hipStreamSynchronize(ctx->stream));
    // the cone locate (cpf_kernels.hip, VertexField) is exact only on a decomposition whose tets cannot overlap: decided here
    t.coneWhy = tetFanDefect(positions, tets, ctx->mesh.host.nCells, tetsPerCell);
    if (t.coneWhy.empty()) {
        CPF_HIP(ctx, t.cone.alloc((size_t)nTets * 32));
        CPF_HIP(ctx, t.apex.alloc((size_t)ctx->mesh.host.nCells * 4));
        CPF_HIP(ctx, cpf::launch_vertex_cone_tables(ctx->stream, t.pos, t.tets, nTets, tetsPerCell, t.cone, t.apex));
        CPF_HIP(ctx, hipStreamSynchronize(ctx->stream));
    }
    t.nVerts = nVerts; t.nTets = nTets; t.tetsPerCell = tetsPerCell;
    ctx->tet = std::move(t);
    return CPF_OK;
}
int cpf_set_vertex_velocity(cpf_context* ctx, const double* vertexU, int64_t nVerts) {
    CPF_REQUIRE(ctx, ctx && vertexU, CPF_ERR_ARG, "null argument");
    CPF_REQUIRE(ctx, ctx->tet.tets, CPF_ERR_STATE, "cpf_set_vertex_velocity: call cpf_set_tets first");
    CPF_REQUIRE(ctx, nVerts == ctx->tet.nVerts, CPF_ERR_ARG, "cpf_set_vertex_velocity: one velocity per tet-mesh vertex");
    CPF_HIP(ctx, hipSetDevice(ctx->device));
    CPF_HIP(ctx, hipMemcpyAsync(ctx->tet.vel, vertexU, (size_t)nVerts * 24, hipMemcpyHostToDevice, ctx->stream));
    if (ctx->tet.cone) CPF_HIP(ctx, cpf::launch_vertex_record_velocity(ctx->stream, ctx->tet.tets, ctx->tet.vel, ctx->tet.nTets, ctx->tet.cone));
    CPF_HIP(ctx, hipStreamSynchronize(ctx->stream));
    ctx->tet.haveVel = true;
    return CPF_OK;
}
int cpf_stage_advect_vertex(cpf_context* ctx, double* particles, const int32_t* ids, double* vels, double* disps,
                            double dt, int64_t n) {
    CPF_STAGE_PRE("cpf_stage_advect_vertex", false);
    CPF_REQUIRE(ctx, ctx->tet.haveVel && ctx->tet.nTets == (int64_t)ctx->tet.tetsPerCell * ctx->mesh.host.nCells, CPF_ERR_STATE,
                "cpf_stage_advect_vertex: call cpf_set_tets and cpf_set_vertex_velocity (for the current mesh) first");
    CPF_REQUIRE(ctx, n == 0 || (particles && ids && vels && disps), CPF_ERR_ARG, "cpf_stage_advect_vertex: null array");
    CPF_HIP(ctx, cpf::launch_stage_advect_vertex(ctx->stream, particles, ids, vels, disps, dt, n, ctx->tet.pos, ctx->tet.tets,
                                                 ctx->tet.tetsPerCell, ctx->tet.vel, ctx->vertexFast ? ctx->tet.cone.get() : nullptr, ctx->tet.apex));
    return CPF_OK;
}
int cpf_stage_brownian(cpf_context* ctx, const double* particles, double* disps, double dt, int64_t n, double D,
                       uint32_t step) {
    CPF_REQUIRE(ctx, ctx, CPF_ERR_ARG, "null context");
    CPF_REQUIRE(ctx, n >= 0 && (n == 0 || (particles && disps)) && D >= 0.0, CPF_ERR_ARG, "cpf_stage_brownian: bad arguments");
    CPF_HIP(ctx, hipSetDevice(ctx->device));
    CPF_HIP(ctx, cpf::launch_stage_brownian(ctx->stream, particles, disps, dt, n, D, step, ctx->seed));
    return CPF_OK;
}
int cpf_stage_locate(cpf_context* ctx, const double* particles, const double* disps, int32_t* ids, int64_t n) {
    CPF_STAGE_PRE("cpf_stage_locate", false);
    CPF_REQUIRE(ctx, n == 0 || (particles && disps && ids), CPF_ERR_ARG, "cpf_stage_locate: null array");
    CPF_HIP(ctx, cpf::launch_stage_locate(ctx->stream, particles, disps, ids, n, meshView(ctx)));
    return CPF_OK;
}
int cpf_stage_reflect(cpf_context* ctx, int32_t* ids, double* particles, double* vels, double* disps, int64_t n) {
    CPF_STAGE_PRE("cpf_stage_reflect", false);
    CPF_REQUIRE(ctx, n == 0 || (particles && disps && ids && vels), CPF_ERR_ARG, "cpf_stage_reflect: null array");
    CPF_HIP(ctx, cpf::launch_stage_reflect(ctx->stream, ids, particles, vels, disps, n, meshView(ctx)));
    return CPF_OK;
}
int cpf_stage_move(cpf_context* ctx, double* particles, double* disps, int64_t n) {
    CPF_REQUIRE(ctx, ctx, CPF_ERR_ARG, "null context");
    CPF_REQUIRE(ctx, n >= 0 && (n == 0 || (particles && disps)), CPF_ERR_ARG, "cpf_stage_move: bad arguments");
    CPF_HIP(ctx, hipSetDevice(ctx->device));
    CPF_HIP(ctx, cpf::launch_stage_move(ctx->stream, particles, disps, n));
    return CPF_OK;
}

int cpf_write_vtu_wait(cpf_context* ctx) {
    CPF_REQUIRE(ctx, ctx, CPF_ERR_ARG, "null context");
    if (!ctx->frame.live) return CPF_OK;
    ctx->frame.thread.join();
    ctx->frame.live = false;
    {
        std::lock_guard<std::mutex> lk(g_mutex);
        auto& v = g_writers.live;
        v.erase(std::remove(v.begin(), v.end(), ctx), v.end());
    }
    const int r = ctx->frame.status;
    ctx->frame.status = CPF_OK;
    if (r != CPF_OK && r != CPF_WARN_NAN) return fail(ctx, r, "cpf_write_vtu_async: the frame could not be written");
    return r;
}

int cpf_write_vtu_async(cpf_context* ctx, const char* path, double* totalKE) {
    CPF_REQUIRE(ctx, ctx && path, CPF_ERR_ARG, "null argument");
    int r = cpf_write_vtu_wait(ctx);                       // one frame in flight; reports the previous frame's failure
    if (r != CPF_OK && r != CPF_WARN_NAN) return r;
    CPF_REQUIRE(ctx, ctx->cloud.n > 0, CPF_ERR_STATE, "cpf_write_vtu_async: no particles");
    CPF_HIP(ctx, hipSetDevice(ctx->device));
    const size_t n = (size_t)ctx->cloud.n;
    const PackLayout lay(n);
    const size_t offC = lay.offC, offV = lay.offV, need = lay.bytes;
    if (!ctx->frame.io) {
        CPF_HIP(ctx, ctx->frame.io.create(hipStreamNonBlocking));
        CPF_HIP(ctx, ctx->frame.evSnap.create(hipEventDisableTiming));
        CPF_HIP(ctx, ctx->frame.evCopied.create(hipEventDisableTiming));
    }
    if (need > ctx->frame.snapBytes) {                           // (the previous frame's worker has been joined: nobody reads these)
        ctx->frame.snapDev.reset();
        ctx->frame.snapHost.reset();
        ctx->frame.snapBytes = 0;
        const size_t want = need + need / 8;
        hipError_t e = ctx->frame.snapDev.alloc(want);
        if (e == hipSuccess) e = ctx->frame.snapHost.alloc(want);
        if (e != hipSuccess) {
            ctx->frame.snapDev.reset();
            return fail(ctx, e == hipErrorOutOfMemory ? CPF_ERR_NOMEM : CPF_ERR_HIP, std::string("cpf_write_vtu_async: snapshot buffers: ") + hipGetErrorString(e));
        }
        ctx->frame.snapBytes = want;
    }
    // ---- the snapshot: ONE kernel on the compute stream (particle-id order, the layouts the writer reads); everything else --
    // PCIe, the energy sum, formatting, the file -- happens behind the caller's back
    char* d = ctx->frame.snapDev;
    CPF_HIP(ctx, cpf::launch_pack_by_gid(ctx->stream, ctx->cloud.cur.x, ctx->cloud.cur.y, ctx->cloud.cur.z, ctx->cloud.cur.cell, ctx->cloud.cur.gid, ctx->cloud.vel, (double*)d, (int32_t*)(d + offC),
                                         (double*)(d + offV), ctx->cloud.n));
    if (ctx->mesh.parentOf)
        CPF_HIP(ctx, cpf::launch_cells_to_parent(ctx->stream, (const int32_t*)(d + offC), (int32_t*)(d + offC), ctx->mesh.parentOf, ctx->cloud.n,
                                                 ctx->mesh.host.nCells));
    CPF_HIP(ctx, hipEventRecord(ctx->frame.evSnap, ctx->stream));
    CPF_HIP(ctx, hipStreamWaitEvent(ctx->frame.io, ctx->frame.evSnap, 0));
    CPF_HIP(ctx, hipMemcpyAsync(ctx->frame.snapHost, ctx->frame.snapDev, need, hipMemcpyDeviceToHost, ctx->frame.io));
    CPF_HIP(ctx, hipEventRecord(ctx->frame.evCopied, ctx->frame.io));
    const std::string file(path);
    { std::lock_guard<std::mutex> lk(g_mutex); g_writers.live.push_back(ctx); }
    ctx->frame.live = true;
    ctx->frame.keReady = false;
    const bool binary = ctx->vtuBinary;
    ctx->frame.thread = std::thread([ctx, file, n, binary, offC, offV] {
        (void)hipSetDevice(ctx->device);
        const hipError_t e = hipEventSynchronize(ctx->frame.evCopied);
        const char* h = ctx->frame.snapHost;
        const double* xyzw = (const double*)h; const int32_t* cell = (const int32_t*)(h + offC); const double* vel = (const double*)(h + offV);
        double total = 0.0;                                // in index order, like the reference's running sum
        if (e == hipSuccess)
            for (size_t i = 0; i < n; ++i) total += 0.5 * (vel[4 * i] * vel[4 * i] + vel[4 * i + 1] * vel[4 * i + 1] + vel[4 * i + 2] * vel[4 * i + 2]);
        { std::lock_guard<std::mutex> lk(ctx->frame.keMutex); ctx->frame.ke = total; ctx->frame.keReady = true; }
        ctx->frame.keCv.notify_all();
        ctx->frame.status = e != hipSuccess ? CPF_ERR_HIP
                                            : (binary ? cpf_write_vtu_arrays_binary : cpf_write_vtu_arrays)(file.c_str(), (int64_t)n, xyzw, cell, vel, nullptr);
    });
    if (!totalKE) return CPF_OK;                           // the caller is back in its step loop after the one kernel launch
    // the energy at once (a host that prints it where the reference does): that host waits for the copy and one pass over it
    std::unique_lock<std::mutex> lk(ctx->frame.keMutex);
    ctx->frame.keCv.wait(lk, [ctx] { return ctx->frame.keReady; });
    *totalKE = ctx->frame.ke;
    return std::isnan(ctx->frame.ke) ? CPF_WARN_NAN : CPF_OK;
}

int cpf_timing_enable(cpf_context* ctx, int on) {
    CPF_REQUIRE(ctx, ctx, CPF_ERR_ARG, "null context");
    ctx->timing.on = on != 0;
    return CPF_OK;
}

int cpf_timing_read(cpf_context* ctx, int64_t* launches, double* total_ms) {
    CPF_REQUIRE(ctx, ctx && launches && total_ms, CPF_ERR_ARG, "null argument");
    CPF_HIP(ctx, hipSetDevice(ctx->device));
    CPF_HIP(ctx, hipStreamSynchronize(ctx->stream));
    CPF_HIP(ctx, ctx->timing.drain(false, launches, total_ms));
    return CPF_OK;
}

int cpf_timing_poll(cpf_context* ctx, int64_t* launches, double* total_ms) {
    CPF_REQUIRE(ctx, ctx && launches && total_ms, CPF_ERR_ARG, "null argument");
    CPF_HIP(ctx, hipSetDevice(ctx->device));
    CPF_HIP(ctx, ctx->timing.drain(true, launches, total_ms));
    return CPF_OK;
}

}  // extern "C"
