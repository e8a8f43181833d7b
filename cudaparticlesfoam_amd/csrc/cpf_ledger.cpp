// The tracer ledger's host side: the entry points of the six opt-in groups of the context's own cloud -- age, tags, routes,
// exposure, zones, the sink log (include/cpf.h; kernels in cpf_age.hip, cpf_tags.hip, cpf_routes.hip, cpf_exposure.hip,
// cpf_zones.hip, cpf_sinklog.hip) -- and the four places where cpf_api.cpp meets them (cpf_context.h).  Each idiom the entries
// share is written once, below; a new group's entries are made of the same pieces.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "cpf.h"
#include "cpf_context.h"
#include "cpf_device.h"
#include "cpf_exposure_bins.h"   // exposure_bin (cpf_exposure_bins_host)
#include "cpf_philox.h"          // kSourceDoubles (cpf_set_source_origins)

using namespace cpf::state;
using cpf::ensureScratch;

namespace {
constexpr int32_t kTagMax = 16;             // origins, and sink groups, at most: tag_transfer_kernel has one thread per matrix entry
constexpr int32_t kExposureWords = 4096;    // histogram words at most: exposure_absorb_kernel stages them in LDS
constexpr int32_t kZoneMax = 63;            // zones at most: zone_sample_kernel stages (nZones + 1)^2 <= 4096 words in LDS
constexpr uint8_t kZoneOutside = 0xFF;

// ---- the groups, and who clears whom (include/cpf.h states the rule; this is its one statement in code) ---------------------
enum : unsigned { kAge = 1, kTags = 2, kRoutes = 4, kExposure = 8, kZones = 16, kSinkLog = 32, kAllGroups = 63 };
constexpr unsigned kWithAge = kRoutes;                  // routes' tables are sized by nBins
constexpr unsigned kWithTags = kRoutes | kExposure;     // ... and by nOrigins and nSinks; so is exposure's histogram

bool isOn(const cpf_context* ctx, unsigned group) {
    return (group == kAge && ctx->age.on) || (group == kTags && ctx->tags.on) || (group == kRoutes && ctx->routes.on) ||
           (group == kExposure && ctx->exposure.on) || (group == kZones && ctx->zones.on) || (group == kSinkLog && ctx->sinkLog.on);
}
const char* enableOf(unsigned group) {
    return group == kAge ? "cpf_age_enable" : group == kTags ? "cpf_tag_enable" : group == kRoutes ? "cpf_route_enable" :
           group == kExposure ? "cpf_exposure_enable" : group == kZones ? "cpf_zone_enable" : "cpf_sink_log_enable";
}
// the groups of the set become empty ones (their device memory is released: the caller has waited for the stream)
void clear(cpf_context* ctx, unsigned groups) {
    if (groups & kAge) ctx->age = Age{};
    if (groups & kTags) ctx->tags = Tags{};
    if (groups & kRoutes) ctx->routes = Routes{};
    if (groups & kExposure) ctx->exposure = Exposure{};
    if (groups & kZones) ctx->zones = Zones{};
    if (groups & kSinkLog) ctx->sinkLog = SinkLog{};
}
// a pass over the old tables may still be running: wait, then clear
int waitAndClear(cpf_context* ctx, unsigned groups) {
    CPF_HIP(ctx, hipSetDevice(ctx->device));
    CPF_HIP(ctx, hipStreamSynchronize(ctx->stream));
    clear(ctx, groups);
    return CPF_OK;
}
// one group off, and `with` it the groups that cannot live without it; nothing happens, and nobody waits, where it is off already
int drop(cpf_context* ctx, unsigned group, unsigned with) {
    return isOn(ctx, group) ? waitAndClear(ctx, group | with) : CPF_OK;
}
// tagging off: exposure goes first, on or off as tagging was (the shape of its histogram is tagging's either way)
int dropTags(cpf_context* ctx) {
    if (int r = drop(ctx, kExposure, 0)) return r;
    return drop(ctx, kTags, kWithTags);
}

// ---- how an entry begins ------------------------------------------------------------------------------------------------------
// an entry of a group that has to be on
int enter(cpf_context* ctx, unsigned group, const char* entry) {
    CPF_REQUIRE(ctx, ctx, CPF_ERR_ARG, "null context");
    CPF_REQUIRE(ctx, isOn(ctx, group), CPF_ERR_STATE, std::string(entry) + ": call " + enableOf(group) + " first");
    return CPF_OK;
}
// ... that also takes one array it cannot do without
int enterArray(cpf_context* ctx, unsigned group, const char* entry, const void* array) {
    if (int r = enter(ctx, group, entry)) return r;
    CPF_REQUIRE(ctx, array, CPF_ERR_ARG, std::string(entry) + ": null array");
    return CPF_OK;
}
// an enable that needs a mesh and a located cloud
int enterEnable(cpf_context* ctx, const char* entry) {
    CPF_REQUIRE(ctx, ctx, CPF_ERR_ARG, "null context");
    CPF_REQUIRE(ctx, ctx->mesh.have, CPF_ERR_STATE, std::string(entry) + ": call cpf_set_mesh first");
    CPF_REQUIRE(ctx, ctx->cloud.n > 0 && ctx->cloud.located, CPF_ERR_STATE, std::string(entry) + ": no located particles");
    return CPF_OK;
}

// ---- copies: every one of them waits for the stream, so the caller's array is free (or filled) on return ------------------------
// `bytes` from the device buffer `src` to the host; dst null: the wait alone
int readBack(cpf_context* ctx, void* dst, const void* src, size_t bytes) {
    CPF_HIP(ctx, hipSetDevice(ctx->device));
    if (dst) CPF_HIP(ctx, hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, ctx->stream));
    CPF_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return CPF_OK;
}
// `bytes` from the host into the device buffer `dst`
int writeThrough(cpf_context* ctx, void* dst, const void* src, size_t bytes) {
    CPF_HIP(ctx, hipSetDevice(ctx->device));
    CPF_HIP(ctx, hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, ctx->stream));
    CPF_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return CPF_OK;
}
// a field of [n][2] = (sum, count) pairs, split into the caller's two arrays; either may be null
int readPairs(cpf_context* ctx, const unsigned long long* field, size_t n, uint64_t* sum, uint64_t* count) {
    std::vector<unsigned long long> h(n * 2);
    if (int r = readBack(ctx, (sum || count) ? h.data() : nullptr, field, n * 16)) return r;
    for (size_t c = 0; c < n; ++c) {
        if (sum) sum[c] = h[2 * c];
        if (count) count[c] = h[2 * c + 1];
    }
    return CPF_OK;
}
// A read-back for checks and restarts, not a hot path: the cells of the cloud in particle-id order (cpf_get_particles' pass) into
// `cell`, and behind them `bytes` of the by-id array `src` into `dst`; one wait for both.  The caller patches the dead on the host.
int cellsInIdOrder(cpf_context* ctx, std::vector<int32_t>& cell, void* dst, const void* src, size_t bytes) {
    CPF_HIP(ctx, hipSetDevice(ctx->device));
    const size_t n = (size_t)ctx->cloud.n;
    if (int r = ensureScratch(ctx, n * 4)) return r;
    int32_t* dC = (int32_t*)ctx->scratch.get();
    CPF_HIP(ctx, cpf::launch_pack_by_gid(ctx->stream, ctx->cloud.cur.x, ctx->cloud.cur.y, ctx->cloud.cur.z, ctx->cloud.cur.cell,
                                         ctx->cloud.cur.gid, nullptr, nullptr, dC, nullptr, ctx->cloud.n));
    cell.resize(n);
    CPF_HIP(ctx, hipMemcpyAsync(cell.data(), dC, n * 4, hipMemcpyDeviceToHost, ctx->stream));
    CPF_HIP(ctx, hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, ctx->stream));
    CPF_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return CPF_OK;
}

// One value per cell of the mesh as given -> one per DERIVED cell: every derived cell of a parent gets the parent's.
template <typename T, typename S>
std::vector<T> toDerived(const cpf_context* ctx, const S* ofParent) {
    const std::vector<int32_t>& first = ctx->mesh.first;    // (empty: no cell decomposed, derived cell c is parent c)
    std::vector<T> out((size_t)ctx->mesh.host.nCells);
    for (int64_t c = 0; c < ctx->mesh.nParent; ++c) {
        const int64_t lo = first.empty() ? c : first[(size_t)c], hi = first.empty() ? c + 1 : first[(size_t)c + 1];
        for (int64_t d = lo; d < hi; ++d) out[(size_t)d] = (T)ofParent[c];
    }
    return out;
}

// ---- a group's tables of 64-bit counters: their sizes in words, each in one place for enable, reset and the getters ---------------
struct TableWords { size_t hist, field; };
TableWords ageWords(const cpf_context* ctx, const Age& a) { return {(size_t)a.nBins, (size_t)ctx->mesh.nParent * 2}; }
TableWords tagWords(const cpf_context* ctx, const Tags& t) { return {(size_t)kTagMax * kTagMax, (size_t)ctx->mesh.nParent * t.nOrigins}; }
TableWords routeWords(const cpf_context* ctx) {         // (of age and tags as they are on now)
    return {(size_t)ctx->tags.nOrigins * ctx->tags.nSinks * ctx->age.nBins, (size_t)ctx->mesh.nParent * ctx->tags.nOrigins * 2};
}
size_t exposureWords(const Exposure& e) { return (size_t)e.nOrigins * e.nSinks * e.nBins; }
size_t zoneWords(const Zones& zn) { return (size_t)(zn.nZones + 1) * (zn.nZones + 1); }
// one table of `words` counters to zero on the stream; a group's two
int zeroTable(cpf_context* ctx, unsigned long long* table, size_t words) {
    CPF_HIP(ctx, hipSetDevice(ctx->device));
    CPF_HIP(ctx, hipMemsetAsync(table, 0, words * 8, ctx->stream));
    return CPF_OK;
}
int zeroTables(cpf_context* ctx, unsigned long long* hist, unsigned long long* field, TableWords w) {
    if (int r = zeroTable(ctx, hist, w.hist)) return r;
    return zeroTable(ctx, field, w.field);
}
}  // namespace

// ---- where cpf_api.cpp meets the groups (cpf_context.h) -----------------------------------------------------------------------
namespace cpf {
void ledger_clear(cpf_context* ctx) { clear(ctx, kAllGroups); }

int ledger_new_cloud(cpf_context* ctx) {
    if (int r = drop(ctx, kAge, kWithAge)) return r;        // (the stamps were the old cloud's)
    if (int r = dropTags(ctx)) return r;                    // (... and so were the origins, and the doses)
    if (int r = drop(ctx, kZones, 0)) return r;             // (... and the last zones)
    return drop(ctx, kSinkLog, 0);                          // (... and the records)
}

int ledger_sink_passes(cpf_context* ctx, bool* marked) {
    *marked = false;
    const Age& age = ctx->age; const Tags& tags = ctx->tags; const Exposure& e = ctx->exposure; const Zones& zn = ctx->zones;
    // no sink set: nothing runs, and the log's apply index stays
    if (!ctx->mesh.sinkMask || !(age.on || tags.on || e.on || zn.on || ctx->sinkLog.on)) return CPF_OK;
    const Cloud& cl = ctx->cloud;
    const uint32_t* mask = ctx->mesh.sinkMask;
    const int64_t nDerived = ctx->mesh.host.nCells;
    CPF_HIP(ctx, hipSetDevice(ctx->device));
    if (ctx->sinkLog.on) {
        // the sink log: a read-only pass of its own appends one record for everybody the sink is about to absorb, made of what the
        // cloud and the tables of the groups that are on hold now, before anyone is marked (cpf_sinklog.hip)
        SinkLog& lg = ctx->sinkLog;
        cpf::SinkLogView v{};
        v.x = cl.cur.x; v.y = cl.cur.y; v.z = cl.cur.z; v.cell = cl.cur.cell; v.gid = cl.cur.gid;
        v.birth = age.on ? age.birth.get() : nullptr;
        v.origin = tags.on ? tags.origin.get() : nullptr;
        v.sinkGroup = tags.on ? tags.sinkGroup.get() : nullptr;
        v.dose = e.on ? e.dose.get() : nullptr;
        v.last = zn.on ? zn.last.get() : nullptr;
        v.parentOf = ctx->mesh.parentOf.get();
        v.mask = mask; v.cursor = lg.cursor; v.rec = lg.rec;
        v.n = cl.n; v.capacity = lg.capacity;
        v.now = ctx->stepCounter; v.apply = lg.apply;
        v.fields = (age.on ? CPF_SINK_LOG_AGE : 0u) | (tags.on ? CPF_SINK_LOG_TAGS : 0u) | (e.on ? CPF_SINK_LOG_EXPOSURE : 0u) |
                   (zn.on ? CPF_SINK_LOG_ZONES : 0u);
        CPF_HIP(ctx, cpf::sink_log(ctx->stream, v, nDerived));
        ++lg.apply;
    }
    // exposure: a read-only pass of its own bins the dose of everybody the sink is about to absorb (cpf_exposure.hip)
    if (e.on)
        CPF_HIP(ctx, cpf::exposure_absorb(ctx->stream, cl.cur.cell, cl.cur.gid, e.dose, e.tagged ? tags.origin.get() : nullptr, cl.n, mask,
                                          nDerived, e.tagged ? tags.sinkGroup.get() : nullptr, e.invWidth, e.nBins, e.nOrigins, e.nSinks,
                                          e.hist));
    // zones: a read-only pass of its own counts them, by the zone of their last sample, as leaving for "outside" (cpf_zones.hip)
    if (zn.on) CPF_HIP(ctx, cpf::zone_leave(ctx->stream, cl.cur.cell, cl.cur.gid, zn.last, cl.n, mask, nDerived, zn.nZones, zn.flow));
    if (ctx->routes.on) {
        // routes (so tags and age are on): ONE pass in place of tags' and age's, which adds what they add and the joint histogram
        // besides, and marks and counts as the plain sink pass does (cpf_routes.hip)
        if (int r = ensureRecycleCounts(ctx)) return r;
        CPF_HIP(ctx, cpf::route_absorb(ctx->stream, cl.cur.cell, cl.cur.gid, age.birth, tags.origin, cl.n, mask, nDerived, tags.sinkGroup,
                                       ctx->recycleCounts, ctx->stepCounter, age.binCycles, age.nBins, tags.nOrigins, tags.nSinks,
                                       age.hist, tags.transfer, ctx->routes.hist));
        *marked = true;
        return CPF_OK;
    }
    // tagging: a read-only pass of its own counts (origin, sink group) of everybody the sink is about to absorb (cpf_tags.hip)
    if (tags.on)
        CPF_HIP(ctx, cpf::tag_transfer(ctx->stream, cl.cur.cell, cl.cur.gid, tags.origin, cl.n, mask, nDerived, tags.sinkGroup,
                                       tags.nOrigins, tags.nSinks, tags.transfer));
    if (age.on) {
        // age tracking: the plain sink pass, which also bins the age of every particle it absorbs (cpf_age.hip)
        if (int r = ensureRecycleCounts(ctx)) return r;
        CPF_HIP(ctx, cpf::age_absorb(ctx->stream, cl.cur.cell, cl.cur.gid, age.birth, cl.n, mask, nDerived, ctx->recycleCounts,
                                     ctx->stepCounter, age.binCycles, age.nBins, age.hist));
        *marked = true;
    }
    return CPF_OK;
}

int ledger_respawn_stamps(cpf_context* ctx, bool fromSource) {
    const Cloud& cl = ctx->cloud;
    if (!(ctx->age.on || ctx->tags.on || ctx->exposure.on || ctx->zones.on)) return CPF_OK;
    CPF_HIP(ctx, hipSetDevice(ctx->device));
    // age tracking: every candidate is born now
    if (ctx->age.on) CPF_HIP(ctx, cpf::age_stamp(ctx->stream, cl.cur.cell, cl.cur.gid, ctx->age.birth, cl.n, ctx->stepCounter));
    // tagging: ... and gets the origin of the triangle this call's epoch picks for its id (cpf_tags.hip), or the box's
    if (ctx->tags.on)
        CPF_HIP(ctx, cpf::tag_stamp(ctx->stream, cl.cur.cell, cl.cur.gid, ctx->tags.origin, cl.n,
                                    fromSource ? ctx->mesh.sourceHi.get() : nullptr, fromSource ? (int32_t)ctx->mesh.sourceKept : 0,
                                    fromSource ? ctx->tags.originOfKept.get() : nullptr, ctx->seed, cl.respawnEpoch,
                                    fromSource ? 0 : ctx->tags.boxOrigin));
    // exposure: ... starts from dose +0.0
    if (ctx->exposure.on) CPF_HIP(ctx, cpf::exposure_stamp(ctx->stream, cl.cur.cell, cl.cur.gid, ctx->exposure.dose, cl.n));
    // zones: ... and is outside until its next sample
    if (ctx->zones.on) CPF_HIP(ctx, cpf::zone_stamp(ctx->stream, cl.cur.cell, cl.cur.gid, ctx->zones.last, cl.n));
    return CPF_OK;
}
}  // namespace cpf

extern "C" {

// ---- tracer age: birth stamps by particle id, residence times at the sink, the mean-age field (cpf_age.hip) ----------------
int cpf_age_enable(cpf_context* ctx, int32_t binCycles, int32_t nBins) {
    if (int r = enterEnable(ctx, __func__)) return r;
    CPF_REQUIRE(ctx, binCycles >= 1 && nBins >= 1 && nBins <= 4096, CPF_ERR_ARG, "cpf_age_enable: binCycles >= 1 and 1 <= nBins <= 4096");
    if (int r = waitAndClear(ctx, kAge | kWithAge)) return r;
    Age a;                                                  // moved in whole: a failure part-way leaves tracking off
    a.binCycles = binCycles; a.nBins = nBins;
    const size_t n = (size_t)ctx->cloud.n;
    const TableWords w = ageWords(ctx, a);
    CPF_HIP(ctx, a.birth.alloc(n));
    CPF_HIP(ctx, a.hist.alloc(w.hist));
    CPF_HIP(ctx, a.field.alloc(w.field));
    CPF_HIP(ctx, hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(a.birth.get()), (int)ctx->stepCounter, n, ctx->stream));
    if (int r = zeroTables(ctx, a.hist, a.field, w)) return r;
    a.on = true;
    ctx->age = std::move(a);
    return CPF_OK;
}

int cpf_age_disable(cpf_context* ctx) {
    CPF_REQUIRE(ctx, ctx, CPF_ERR_ARG, "null context");
    return drop(ctx, kAge, kWithAge);
}

int cpf_age_sample(cpf_context* ctx) {
    if (int r = enter(ctx, kAge, __func__)) return r;
    CPF_HIP(ctx, hipSetDevice(ctx->device));
    CPF_HIP(ctx, cpf::age_field(ctx->stream, ctx->cloud.cur.cell, ctx->cloud.cur.gid, ctx->age.birth, ctx->cloud.n, ctx->mesh.parentOf,
                                ctx->mesh.host.nCells, ctx->stepCounter, ctx->age.field));
    ++ctx->age.samples;
    return CPF_OK;
}

int cpf_age_reset(cpf_context* ctx) {
    if (int r = enter(ctx, kAge, __func__)) return r;
    ctx->age.samples = 0;
    return zeroTables(ctx, ctx->age.hist, ctx->age.field, ageWords(ctx, ctx->age));
}

int cpf_get_age_histogram(cpf_context* ctx, uint64_t* bins, int32_t nBins) {
    if (int r = enter(ctx, kAge, __func__)) return r;
    CPF_REQUIRE(ctx, bins && nBins == ctx->age.nBins, CPF_ERR_ARG, "cpf_get_age_histogram: nBins is not cpf_age_enable's");
    return readBack(ctx, bins, ctx->age.hist, ageWords(ctx, ctx->age).hist * 8);
}

int cpf_get_age_field(cpf_context* ctx, uint64_t* ageSum, uint64_t* count, int64_t* nSamples) {
    if (int r = enter(ctx, kAge, __func__)) return r;
    if (nSamples) *nSamples = ctx->age.samples;
    return readPairs(ctx, ctx->age.field, (size_t)ctx->mesh.nParent, ageSum, count);
}

int cpf_age_get_births(cpf_context* ctx, uint32_t* birth) {
    if (int r = enterArray(ctx, kAge, __func__, birth)) return r;
    return readBack(ctx, birth, ctx->age.birth, (size_t)ctx->cloud.n * 4);
}

int cpf_age_set_births(cpf_context* ctx, const uint32_t* birth) {
    if (int r = enterArray(ctx, kAge, __func__, birth)) return r;
    return writeThrough(ctx, ctx->age.birth, birth, (size_t)ctx->cloud.n * 4);
}

int cpf_get_ages(cpf_context* ctx, int64_t* age) {
    if (int r = enterArray(ctx, kAge, __func__, age)) return r;
    const size_t n = (size_t)ctx->cloud.n;
    std::vector<int32_t> cell;
    std::vector<uint32_t> birth(n);
    if (int r = cellsInIdOrder(ctx, cell, birth.data(), ctx->age.birth, n * 4)) return r;
    const uint32_t now = ctx->stepCounter;
    for (size_t i = 0; i < n; ++i) age[i] = cell[i] >= 0 ? (int64_t)(uint32_t)(now - birth[i]) : -1;
    return CPF_OK;
}

// ---- tracer tags: an origin per particle id, grouped sinks, the transfer matrix, the per-origin field (cpf_tags.hip) -------
int cpf_tag_enable(cpf_context* ctx, int32_t nOrigins, int32_t nSinks) {
    if (int r = enterEnable(ctx, __func__)) return r;
    CPF_REQUIRE(ctx, nOrigins >= 1 && nOrigins <= kTagMax && nSinks >= 1 && nSinks <= kTagMax, CPF_ERR_ARG,
                "cpf_tag_enable: 1 <= nOrigins <= 16 and 1 <= nSinks <= 16");
    CPF_REQUIRE(ctx, ctx->mesh.nParent * (int64_t)nOrigins < ((int64_t)1 << 31), CPF_ERR_ARG,
                "cpf_tag_enable: nCells * nOrigins must stay below 2^31");
    if (int r = waitAndClear(ctx, kTags | kWithTags)) return r;
    Tags t;                                                 // moved in whole: a failure part-way leaves tagging off
    t.nOrigins = nOrigins; t.nSinks = nSinks;
    const size_t n = (size_t)ctx->cloud.n, nDerived = (size_t)ctx->mesh.host.nCells;
    const TableWords w = tagWords(ctx, t);
    CPF_HIP(ctx, t.origin.alloc(n));
    CPF_HIP(ctx, t.sinkGroup.alloc(nDerived));
    CPF_HIP(ctx, t.transfer.alloc(w.hist));
    CPF_HIP(ctx, t.field.alloc(w.field));
    CPF_HIP(ctx, hipMemsetAsync(t.origin, 0, n, ctx->stream));
    CPF_HIP(ctx, hipMemsetAsync(t.sinkGroup, 0, nDerived, ctx->stream));
    if (int r = zeroTables(ctx, t.transfer, t.field, w)) return r;
    if (ctx->mesh.sourceKept > 0) {
        CPF_HIP(ctx, t.originOfKept.alloc((size_t)ctx->mesh.sourceKept));
        CPF_HIP(ctx, hipMemsetAsync(t.originOfKept, 0, (size_t)ctx->mesh.sourceKept, ctx->stream));
    }
    t.on = true;
    ctx->tags = std::move(t);
    return CPF_OK;
}

int cpf_tag_disable(cpf_context* ctx) {
    CPF_REQUIRE(ctx, ctx, CPF_ERR_ARG, "null context");
    return dropTags(ctx);
}

int cpf_set_sink_groups(cpf_context* ctx, const int32_t* parentCells, const int32_t* group, int64_t n) {
    if (int r = enter(ctx, kTags, __func__)) return r;
    CPF_REQUIRE(ctx, n >= 0 && ((parentCells && group) || n == 0), CPF_ERR_ARG, "cpf_set_sink_groups: bad arguments");
    for (int64_t k = 0; k < n; ++k) {
        CPF_REQUIRE(ctx, parentCells[k] >= 0 && parentCells[k] < ctx->mesh.nParent, CPF_ERR_ARG,
                    "cpf_set_sink_groups: cell " + std::to_string(parentCells[k]) + " is not in [0, nCells)");
        CPF_REQUIRE(ctx, group[k] >= 0 && group[k] < ctx->tags.nSinks, CPF_ERR_ARG,
                    "cpf_set_sink_groups: group " + std::to_string(group[k]) + " is not in [0, nSinks)");
    }
    int r = cpf_set_sink_cells(ctx, parentCells, n);        // (the mask; it waits for the stream and puts everybody in group 0)
    if (r || n == 0) return r;
    std::vector<uint8_t> ofParent((size_t)ctx->mesh.nParent, (uint8_t)0);
    for (int64_t k = 0; k < n; ++k) ofParent[(size_t)parentCells[k]] = (uint8_t)group[k];
    const std::vector<uint8_t> g = toDerived<uint8_t>(ctx, ofParent.data());
    CPF_HIP(ctx, hipMemcpy(ctx->tags.sinkGroup, g.data(), g.size(), hipMemcpyHostToDevice));
    return CPF_OK;
}

int cpf_set_source_origins(cpf_context* ctx, const int32_t* originOfTriangle, int64_t nTriangles) {
    if (int r = enter(ctx, kTags, __func__)) return r;
    CPF_REQUIRE(ctx, ctx->mesh.sourceKept > 0, CPF_ERR_STATE, "cpf_set_source_origins: call cpf_set_source_triangles first");
    CPF_REQUIRE(ctx, originOfTriangle && nTriangles > 0, CPF_ERR_ARG, "cpf_set_source_origins: bad arguments");
    for (int64_t t = 0; t < nTriangles; ++t)
        CPF_REQUIRE(ctx, originOfTriangle[t] >= 0 && originOfTriangle[t] < ctx->tags.nOrigins, CPF_ERR_ARG,
                    "cpf_set_source_origins: origin " + std::to_string(originOfTriangle[t]) + " is not in [0, nOrigins)");
    // a kept record carries the index of the CALLER's triangle (dropped ones have no record)
    std::vector<uint8_t> o((size_t)ctx->mesh.sourceKept);
    for (size_t k = 0; k < o.size(); ++k) {
        const int64_t t = (int64_t)ctx->mesh.sourceRecHost[k * cpf::kSourceDoubles + 14];
        CPF_REQUIRE(ctx, t >= 0 && t < nTriangles, CPF_ERR_ARG,
                    "cpf_set_source_origins: the source has a triangle " + std::to_string(t) + ", beyond nTriangles");
        o[k] = (uint8_t)originOfTriangle[t];
    }
    CPF_HIP(ctx, hipSetDevice(ctx->device));
    CPF_HIP(ctx, hipStreamSynchronize(ctx->stream));        // (a stamp over the old origins may still be running)
    CPF_HIP(ctx, hipMemcpy(ctx->tags.originOfKept, o.data(), o.size(), hipMemcpyHostToDevice));
    return CPF_OK;
}

int cpf_set_box_origin(cpf_context* ctx, int32_t origin) {
    if (int r = enter(ctx, kTags, __func__)) return r;
    CPF_REQUIRE(ctx, origin >= 0 && origin < ctx->tags.nOrigins, CPF_ERR_ARG,
                "cpf_set_box_origin: origin " + std::to_string(origin) + " is not in [0, nOrigins)");
    ctx->tags.boxOrigin = origin;
    return CPF_OK;
}

int cpf_tag_sample(cpf_context* ctx) {
    if (int r = enter(ctx, kTags, __func__)) return r;
    CPF_HIP(ctx, hipSetDevice(ctx->device));
    CPF_HIP(ctx, cpf::tag_field(ctx->stream, ctx->cloud.cur.cell, ctx->cloud.cur.gid, ctx->tags.origin, ctx->cloud.n, ctx->mesh.parentOf,
                                ctx->mesh.host.nCells, ctx->mesh.nParent, ctx->tags.nOrigins, ctx->tags.field));
    ++ctx->tags.samples;
    return CPF_OK;
}

int cpf_tag_reset(cpf_context* ctx) {
    if (int r = enter(ctx, kTags, __func__)) return r;
    ctx->tags.samples = 0;
    return zeroTables(ctx, ctx->tags.transfer, ctx->tags.field, tagWords(ctx, ctx->tags));
}

int cpf_get_transfer(cpf_context* ctx, uint64_t* T) {
    if (int r = enterArray(ctx, kTags, __func__, T)) return r;
    return readBack(ctx, T, ctx->tags.transfer, (size_t)ctx->tags.nOrigins * ctx->tags.nSinks * 8);
}

int cpf_get_tag_field(cpf_context* ctx, uint64_t* counts, int64_t* nSamples) {
    if (int r = enter(ctx, kTags, __func__)) return r;
    if (nSamples) *nSamples = ctx->tags.samples;
    return readBack(ctx, counts, ctx->tags.field, tagWords(ctx, ctx->tags).field * 8);
}

int cpf_tag_get_origins(cpf_context* ctx, uint8_t* origin) {
    if (int r = enterArray(ctx, kTags, __func__, origin)) return r;
    return readBack(ctx, origin, ctx->tags.origin, (size_t)ctx->cloud.n);
}

int cpf_tag_set_origins(cpf_context* ctx, const uint8_t* origin) {
    if (int r = enterArray(ctx, kTags, __func__, origin)) return r;
    for (int64_t i = 0; i < ctx->cloud.n; ++i)
        CPF_REQUIRE(ctx, (int32_t)origin[i] < ctx->tags.nOrigins, CPF_ERR_ARG,
                    "cpf_tag_set_origins: origin " + std::to_string((int)origin[i]) + " is not in [0, nOrigins)");
    return writeThrough(ctx, ctx->tags.origin, origin, (size_t)ctx->cloud.n);
}

// ---- routes: the residence-time histogram per (origin, sink group), the age field per origin (cpf_routes.hip) ---------------
int cpf_route_enable(cpf_context* ctx) {
    CPF_REQUIRE(ctx, ctx, CPF_ERR_ARG, "null context");
    CPF_REQUIRE(ctx, ctx->age.on && ctx->tags.on, CPF_ERR_STATE, "cpf_route_enable: call cpf_age_enable and cpf_tag_enable first");
    if (int r = waitAndClear(ctx, kRoutes)) return r;
    Routes t;                                               // moved in whole: a failure part-way leaves routes off
    const TableWords w = routeWords(ctx);
    CPF_HIP(ctx, t.hist.alloc(w.hist));
    CPF_HIP(ctx, t.field.alloc(w.field));
    if (int r = zeroTables(ctx, t.hist, t.field, w)) return r;
    t.on = true;
    ctx->routes = std::move(t);
    return CPF_OK;
}

int cpf_route_disable(cpf_context* ctx) {
    CPF_REQUIRE(ctx, ctx, CPF_ERR_ARG, "null context");
    return drop(ctx, kRoutes, 0);
}

int cpf_route_sample(cpf_context* ctx) {
    if (int r = enter(ctx, kRoutes, __func__)) return r;
    CPF_HIP(ctx, hipSetDevice(ctx->device));
    CPF_HIP(ctx, cpf::route_field(ctx->stream, ctx->cloud.cur.cell, ctx->cloud.cur.gid, ctx->age.birth, ctx->tags.origin, ctx->cloud.n,
                                  ctx->mesh.parentOf, ctx->mesh.host.nCells, ctx->mesh.nParent, ctx->tags.nOrigins, ctx->stepCounter,
                                  ctx->routes.field));
    ++ctx->routes.samples;
    return CPF_OK;
}

int cpf_route_reset(cpf_context* ctx) {
    if (int r = enter(ctx, kRoutes, __func__)) return r;
    ctx->routes.samples = 0;
    return zeroTables(ctx, ctx->routes.hist, ctx->routes.field, routeWords(ctx));
}

int cpf_get_route_histogram(cpf_context* ctx, uint64_t* bins) {
    if (int r = enterArray(ctx, kRoutes, __func__, bins)) return r;
    return readBack(ctx, bins, ctx->routes.hist, routeWords(ctx).hist * 8);
}

int cpf_get_route_field(cpf_context* ctx, uint64_t* ageSum, uint64_t* count, int64_t* nSamples) {
    if (int r = enter(ctx, kRoutes, __func__)) return r;
    if (nSamples) *nSamples = ctx->routes.samples;
    return readPairs(ctx, ctx->routes.field, routeWords(ctx).field / 2, ageSum, count);
}

// ---- exposure: a dose per particle id summed along the path, the dose histogram at the sink (cpf_exposure.hip) -------------
int cpf_exposure_enable(cpf_context* ctx, double binWidth, int32_t nBins) {
    if (int r = enterEnable(ctx, __func__)) return r;
    CPF_REQUIRE(ctx, std::isfinite(binWidth) && binWidth > 0.0, CPF_ERR_ARG, "cpf_exposure_enable: binWidth must be finite and > 0");
    Exposure e;                                             // moved in whole: a failure part-way leaves exposure off
    e.binWidth = binWidth; e.invWidth = 1.0 / binWidth; e.nBins = nBins;
    e.tagged = ctx->tags.on; e.nOrigins = e.tagged ? ctx->tags.nOrigins : 1; e.nSinks = e.tagged ? ctx->tags.nSinks : 1;
    CPF_REQUIRE(ctx, nBins >= 1 && (int64_t)e.nOrigins * e.nSinks * nBins <= kExposureWords, CPF_ERR_ARG,
                "cpf_exposure_enable: nOrigins * nSinks * nBins must be in [1, 4096]");
    if (int r = waitAndClear(ctx, kExposure)) return r;
    const size_t n = (size_t)ctx->cloud.n, nDerived = (size_t)ctx->mesh.host.nCells;
    CPF_HIP(ctx, e.dose.alloc(n));
    CPF_HIP(ctx, e.rate.alloc(nDerived));
    CPF_HIP(ctx, e.hist.alloc(exposureWords(e)));
    CPF_HIP(ctx, hipMemsetAsync(e.dose, 0, n * 8, ctx->stream));            // (+0.0)
    CPF_HIP(ctx, hipMemsetAsync(e.rate, 0, nDerived * 8, ctx->stream));
    if (int r = zeroTable(ctx, e.hist, exposureWords(e))) return r;
    e.on = true;
    ctx->exposure = std::move(e);
    return CPF_OK;
}

int cpf_exposure_disable(cpf_context* ctx) {
    CPF_REQUIRE(ctx, ctx, CPF_ERR_ARG, "null context");
    return drop(ctx, kExposure, 0);
}

int cpf_set_exposure_field(cpf_context* ctx, const double* rate, int64_t nCells) {
    if (int r = enter(ctx, kExposure, __func__)) return r;
    CPF_REQUIRE(ctx, rate && nCells == ctx->mesh.nParent, CPF_ERR_ARG, "cpf_set_exposure_field: one value per cell of the mesh as given");
    for (int64_t c = 0; c < nCells; ++c)
        CPF_REQUIRE(ctx, std::isfinite(rate[c]) && rate[c] >= 0.0, CPF_ERR_ARG,
                    "cpf_set_exposure_field: the rate of cell " + std::to_string(c) + " is not finite and >= 0");
    if (ctx->mesh.first.empty()) return writeThrough(ctx, ctx->exposure.rate, rate, (size_t)nCells * 8);   // (no cell decomposed)
    const std::vector<double> expanded = toDerived<double>(ctx, rate);
    return writeThrough(ctx, ctx->exposure.rate, expanded.data(), expanded.size() * 8);
}

int cpf_exposure_accumulate(cpf_context* ctx, double scale) {
    if (int r = enter(ctx, kExposure, __func__)) return r;
    CPF_REQUIRE(ctx, std::isfinite(scale) && scale >= 0.0, CPF_ERR_ARG, "cpf_exposure_accumulate: scale must be finite and >= 0");
    CPF_HIP(ctx, hipSetDevice(ctx->device));
    CPF_HIP(ctx, cpf::exposure_accumulate(ctx->stream, ctx->cloud.cur.cell, ctx->cloud.cur.gid, ctx->exposure.rate, ctx->exposure.dose,
                                          ctx->cloud.n, ctx->mesh.host.nCells, scale));
    return CPF_OK;
}

int cpf_exposure_reset(cpf_context* ctx) {
    if (int r = enter(ctx, kExposure, __func__)) return r;
    return zeroTable(ctx, ctx->exposure.hist, exposureWords(ctx->exposure));
}

int cpf_get_dose_histogram(cpf_context* ctx, uint64_t* bins) {
    if (int r = enterArray(ctx, kExposure, __func__, bins)) return r;
    return readBack(ctx, bins, ctx->exposure.hist, exposureWords(ctx->exposure) * 8);
}

int cpf_exposure_get_doses(cpf_context* ctx, double* dose) {
    if (int r = enterArray(ctx, kExposure, __func__, dose)) return r;
    return readBack(ctx, dose, ctx->exposure.dose, (size_t)ctx->cloud.n * 8);
}

int cpf_exposure_set_doses(cpf_context* ctx, const double* dose) {
    if (int r = enterArray(ctx, kExposure, __func__, dose)) return r;
    for (int64_t i = 0; i < ctx->cloud.n; ++i)              // (what the accumulate rule can produce: no NaN, nothing negative, no -0.0)
        CPF_REQUIRE(ctx, dose[i] >= 0.0 && !std::signbit(dose[i]), CPF_ERR_ARG,
                    "cpf_exposure_set_doses: the dose of particle " + std::to_string(i) + " is negative or not a number");
    return writeThrough(ctx, ctx->exposure.dose, dose, (size_t)ctx->cloud.n * 8);
}

int cpf_get_doses(cpf_context* ctx, double* dose) {
    if (int r = enterArray(ctx, kExposure, __func__, dose)) return r;
    const size_t n = (size_t)ctx->cloud.n;
    std::vector<int32_t> cell;
    if (int r = cellsInIdOrder(ctx, cell, dose, ctx->exposure.dose, n * 8)) return r;
    for (size_t i = 0; i < n; ++i)
        if (cell[i] < 0) dose[i] = -1.0;
    return CPF_OK;
}

int cpf_exposure_bins_host(const double* dose, int64_t n, double binWidth, int32_t nBins, int32_t* bin) {
    if (n < 0 || !std::isfinite(binWidth) || !(binWidth > 0.0) || nBins < 1 || (n > 0 && (!dose || !bin))) return CPF_ERR_ARG;
    const double invWidth = 1.0 / binWidth;
    for (int64_t i = 0; i < n; ++i) bin[i] = cpf::exposure_bin(dose[i], invWidth, nBins);
    return CPF_OK;
}

// ---- the sink log: one record per absorbed particle, appended on the device (cpf_sinklog.hip) ----------------------------------
int cpf_sink_log_enable(cpf_context* ctx, int64_t capacity) {
    if (int r = enterEnable(ctx, __func__)) return r;
    CPF_REQUIRE(ctx, capacity >= 1 && capacity < ((int64_t)1 << 40), CPF_ERR_ARG, "cpf_sink_log_enable: capacity must be in [1, 2^40)");
    if (int r = waitAndClear(ctx, kSinkLog)) return r;
    SinkLog lg;                                             // moved in whole: a failure part-way leaves the log off
    CPF_HIP(ctx, lg.rec.alloc((size_t)capacity));
    CPF_HIP(ctx, lg.cursor.alloc(1));
    if (int r = zeroTable(ctx, lg.cursor, 1)) return r;
    lg.on = true; lg.capacity = capacity;
    ctx->sinkLog = std::move(lg);
    return CPF_OK;
}

int cpf_sink_log_disable(cpf_context* ctx) {
    CPF_REQUIRE(ctx, ctx, CPF_ERR_ARG, "null context");
    return drop(ctx, kSinkLog, 0);
}

int cpf_sink_log_clear(cpf_context* ctx) {
    if (int r = enter(ctx, kSinkLog, __func__)) return r;
    return zeroTable(ctx, ctx->sinkLog.cursor, 1);
}

namespace {
// the cursor as the device holds it once the stream has drained
int sinkLogCursor(cpf_context* ctx, uint64_t* cursor) {
    unsigned long long c = 0;
    if (int r = readBack(ctx, &c, ctx->sinkLog.cursor, 8)) return r;
    *cursor = (uint64_t)c;
    return CPF_OK;
}
}  // namespace

int cpf_sink_log_counts(cpf_context* ctx, int64_t* stored, int64_t* dropped) {
    if (int r = enter(ctx, kSinkLog, __func__)) return r;
    uint64_t cursor = 0;
    if (int r = sinkLogCursor(ctx, &cursor)) return r;
    const uint64_t kept = std::min(cursor, (uint64_t)ctx->sinkLog.capacity);
    if (stored) *stored = (int64_t)kept;
    if (dropped) *dropped = (int64_t)(cursor - kept);
    return CPF_OK;
}

int cpf_sink_log_read(cpf_context* ctx, cpf_sink_record* rec, int64_t maxRecords, int64_t* nRead) {
    if (int r = enter(ctx, kSinkLog, __func__)) return r;
    CPF_REQUIRE(ctx, maxRecords >= 0 && (rec || maxRecords == 0), CPF_ERR_ARG, "cpf_sink_log_read: bad arguments");
    uint64_t cursor = 0;
    if (int r = sinkLogCursor(ctx, &cursor)) return r;
    const size_t kept = (size_t)std::min(cursor, (uint64_t)ctx->sinkLog.capacity);
    const size_t take = std::min(kept, (size_t)maxRecords);
    if (nRead) *nRead = (int64_t)take;
    if (take == 0) return CPF_OK;
    // the order on the device is whichever workgroup reserved first: sorted here by the unique key (apply, id)
    std::vector<cpf_sink_record> all(kept);
    CPF_HIP(ctx, hipMemcpy(all.data(), ctx->sinkLog.rec, kept * sizeof(cpf_sink_record), hipMemcpyDeviceToHost));
    std::sort(all.begin(), all.end(), [](const cpf_sink_record& a, const cpf_sink_record& b) {
        return a.apply != b.apply ? a.apply < b.apply : a.id < b.id;
    });
    std::memcpy(rec, all.data(), take * sizeof(cpf_sink_record));
    return CPF_OK;
}

// ---- zones: the zone of every particle id at the last sample, the zone-to-zone transition counts (cpf_zones.hip) ------------
int cpf_zone_enable(cpf_context* ctx, int32_t nZones) {
    if (int r = enterEnable(ctx, __func__)) return r;
    CPF_REQUIRE(ctx, nZones >= 1 && nZones <= kZoneMax, CPF_ERR_ARG, "cpf_zone_enable: nZones must be in [1, 63]");
    if (int r = waitAndClear(ctx, kZones)) return r;
    Zones zn;                                               // moved in whole: a failure part-way leaves zones off
    zn.nZones = nZones;
    const size_t n = (size_t)ctx->cloud.n, nDerived = (size_t)ctx->mesh.host.nCells;
    CPF_HIP(ctx, zn.zoneOf.alloc(nDerived));
    CPF_HIP(ctx, zn.last.alloc(n));
    CPF_HIP(ctx, zn.flow.alloc(zoneWords(zn)));
    CPF_HIP(ctx, hipMemsetAsync(zn.zoneOf, 0, nDerived, ctx->stream));
    CPF_HIP(ctx, hipMemsetAsync(zn.last, kZoneOutside, n, ctx->stream));
    if (int r = zeroTable(ctx, zn.flow, zoneWords(zn))) return r;
    zn.on = true;
    ctx->zones = std::move(zn);
    return CPF_OK;
}

int cpf_zone_disable(cpf_context* ctx) {
    CPF_REQUIRE(ctx, ctx, CPF_ERR_ARG, "null context");
    return drop(ctx, kZones, 0);
}

int cpf_set_zone_map(cpf_context* ctx, const int32_t* zone, int64_t nCells) {
    if (int r = enter(ctx, kZones, __func__)) return r;
    CPF_REQUIRE(ctx, zone && nCells == ctx->mesh.nParent, CPF_ERR_ARG, "cpf_set_zone_map: one value per cell of the mesh as given");
    for (int64_t c = 0; c < nCells; ++c)
        CPF_REQUIRE(ctx, zone[c] >= 0 && zone[c] < ctx->zones.nZones, CPF_ERR_ARG,
                    "cpf_set_zone_map: the zone of cell " + std::to_string(c) + " is not in [0, nZones)");
    const std::vector<uint8_t> expanded = toDerived<uint8_t>(ctx, zone);
    return writeThrough(ctx, ctx->zones.zoneOf, expanded.data(), expanded.size());
}

int cpf_zone_sample(cpf_context* ctx) {
    if (int r = enter(ctx, kZones, __func__)) return r;
    Zones& zn = ctx->zones;
    CPF_HIP(ctx, hipSetDevice(ctx->device));
    CPF_HIP(ctx, cpf::zone_sample(ctx->stream, ctx->cloud.cur.cell, ctx->cloud.cur.gid, zn.zoneOf, zn.last, ctx->cloud.n,
                                  ctx->mesh.host.nCells, zn.nZones, zn.flow));
    ++zn.samples;
    return CPF_OK;
}

int cpf_zone_reset(cpf_context* ctx) {
    if (int r = enter(ctx, kZones, __func__)) return r;
    ctx->zones.samples = 0;
    return zeroTable(ctx, ctx->zones.flow, zoneWords(ctx->zones));
}

int cpf_get_zone_flows(cpf_context* ctx, uint64_t* flow, int64_t* nSamples) {
    if (int r = enter(ctx, kZones, __func__)) return r;
    if (nSamples) *nSamples = ctx->zones.samples;
    return readBack(ctx, flow, ctx->zones.flow, zoneWords(ctx->zones) * 8);
}

int cpf_zone_get_last(cpf_context* ctx, uint8_t* last) {
    if (int r = enterArray(ctx, kZones, __func__, last)) return r;
    return readBack(ctx, last, ctx->zones.last, (size_t)ctx->cloud.n);
}

int cpf_zone_set_last(cpf_context* ctx, const uint8_t* last) {
    if (int r = enterArray(ctx, kZones, __func__, last)) return r;
    for (int64_t i = 0; i < ctx->cloud.n; ++i)              // (what the sample rule can produce)
        CPF_REQUIRE(ctx, last[i] < ctx->zones.nZones || last[i] == kZoneOutside, CPF_ERR_ARG,
                    "cpf_zone_set_last: the byte of particle " + std::to_string(i) + " is neither a zone nor 0xFF");
    return writeThrough(ctx, ctx->zones.last, last, (size_t)ctx->cloud.n);
}

}  // extern "C"
