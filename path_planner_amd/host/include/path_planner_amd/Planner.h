// Planner / GpuAStarPlanner — the drop-in seam.
//
// Planner mirrors /root/reference/path_planner/src/planner/Planner.h:17-80 (same Stats fields, same plan() signature);
// GpuAStarPlanner is AStarPlanner (AStarPlanner.cpp:12-148) + SamplingBasedPlanner::expand (SamplingBasedPlanner.cpp:52-151)
// with every sample drawn, every Dubins length computed and every edge costed on the device through include/ppgpu.h.
// The A* control flow, the open list and the clock polling stay on the host in the reference's order, so that with the same
// injected clock and seed the same vertices are expanded in the same order.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <atomic>
#include <condition_variable>
#include <functional>
#include <memory>
#include <mutex>
#include <thread>
#include <unordered_map>
#include <vector>

#include "DubinsWrapper.h"
#include "RibbonManager.h"
#include "World.h"

struct ppgpu_ctx;

struct ppgpu_edge_result;   // include/ppgpu.h
struct ppgpu_vertex;
struct ppgpu_wrapper_edge;
struct ppgpu_ribbon_water_record;
struct ppgpu_water_route_record;

namespace ppamd {

class Planner {
public:
    struct Stats {
        unsigned long Samples = 0;
        unsigned long Generated = 0;
        unsigned long Expanded = 0;
        unsigned long Iterations = 0;
        double PlanFValue = 0;
        double PlanCollisionPenalty = 0;
        double PlanTimePenalty = 0;
        double PlanHValue = 0;
        unsigned long PlanDepth = 0;
        DubinsPlan Plan;
        // With PlannerConfig::setPlanTrace: Trace[s] = the executed collision-check steps of Plan's segment s as the device swept
        // them (ppgpu_trace_wrapper_edges_host from the segment's parent vertex; the layout is ppgpu_step_record's).
        struct TraceStep { double x, y, heading, time, collision, penaltyBefore; uint32_t flags, step; double reserved; };
        std::vector<std::vector<TraceStep>> Trace;
        // With PlannerConfig::setPlanCoverage: Coverage[s][k] = what step k of Plan's segment s did to the ribbons (the coverage
        // branch of Edge::computeTrueCost executed step by step on the device, ppgpu_trace_cover_wrapper_edges_host: the fields of
        // ppgpu_cover_record, and the step's time, Edge.cpp:114-120,173), parallel to Trace[s][k].  Segment s starts from the
        // vertex segment s - 1 left.
        struct CoverStep { double time, toCover, remaining; uint32_t flags, step, ribbons; };
        std::vector<std::vector<CoverStep>> Coverage;
        // With PlannerConfig::setPlanContacts: Contacts[s][j] = what Plan's segment s has to do with contact j (the rows of the
        // obstacle manager's deviceRows, named by deviceIds): the fields of ppgpu_contact_record from one
        // ppgpu_trace_contacts_wrapper_edges_host call over the segments — on how many steps the contact is hit, from when to
        // when, what it adds to the penalty, the closest approach.  PlanContacts[j] = the segments merged (mergeContacts).
        struct Contact {
            uint32_t mmsi = 0;
            double cpaDistance = -1, cpaTime = -1, firstHitTime = -1, lastHitTime = -1, exposure = 0, peak = 0;
            int32_t cpaStep = -1, hitSteps = 0, firstHitStep = -1, lastHitStep = -1;     // steps count within their segment
        };
        std::vector<std::vector<Contact>> Contacts;
        std::vector<Contact> PlanContacts;
        // hitSteps and exposure summed, first and last hit the earliest and latest, the closest approach the smallest (the
        // earlier segment on ties), peak the largest.  Step indices belong to a segment: the merged record keeps those of the
        // segment its times come from.
        static std::vector<Contact> mergeContacts(const std::vector<std::vector<Contact>>& segments) {
            std::vector<Contact> out;
            for (const std::vector<Contact>& seg : segments) {
                if (out.empty()) {
                    out.resize(seg.size());
                    for (size_t j = 0; j < seg.size(); j++) out[j].mmsi = seg[j].mmsi;
                }
                for (size_t j = 0; j < seg.size() && j < out.size(); j++) {
                    const Contact& c = seg[j];
                    Contact& o = out[j];
                    if (c.hitSteps > 0) {
                        if (o.hitSteps == 0 || c.firstHitTime < o.firstHitTime) { o.firstHitTime = c.firstHitTime; o.firstHitStep = c.firstHitStep; }
                        if (o.hitSteps == 0 || c.lastHitTime > o.lastHitTime) { o.lastHitTime = c.lastHitTime; o.lastHitStep = c.lastHitStep; }
                    }
                    o.hitSteps += c.hitSteps;
                    o.exposure += c.exposure;
                    if (c.peak > o.peak) o.peak = c.peak;
                    if (c.cpaStep >= 0 && (o.cpaStep < 0 || c.cpaDistance < o.cpaDistance)) {
                        o.cpaDistance = c.cpaDistance; o.cpaTime = c.cpaTime; o.cpaStep = c.cpaStep;
                    }
                }
            }
            return out;
        }
        // With PlannerConfig::setPlanClearance: Clearance[s] = how close Plan's segment s passes to a charted hazard (a cell that is
        // blocked or outside the grid): the fields of ppgpu_clearance_record from one ppgpu_trace_clearance_wrapper_edges_host call
        // over the segments, with PlannerConfig::planClearanceMargin.  `clearance` is a certified lower bound in metres (the true
        // distance is at most a cell's diagonal more).  PlanClearance = the segments merged (mergeClearance).
        struct ClearanceReport {
            enum : uint32_t { Empty = 0x1, Blocked = 0x2, Capped = 0x4, NoMap = 0x8 };      // PPGPU_CL_*
            double clearance = -1, time = -1, x = 0, y = 0, firstBelowTime = -1;
            int32_t step = -1;                    // steps count within their segment ...
            uint32_t gap2 = 0;
            int32_t belowSteps = 0, firstBelowStep = -1;
            uint32_t flags = Empty;
            int32_t segment = -1;                 // ... a merged report says which one `step` counts in (-1: none)
            int32_t firstBelowSegment = -1;       // ... and firstBelowStep
        };
        std::vector<ClearanceReport> Clearance;
        ClearanceReport PlanClearance;
        // The smallest clearance wins, the earlier segment on equality; belowSteps summed; the earliest firstBelowTime; flags ORed,
        // except Empty, which is set only when every segment is empty (no segment at all included).
        static ClearanceReport mergeClearance(const std::vector<ClearanceReport>& segments) {
            ClearanceReport out;
            uint32_t flags = 0;
            for (size_t s = 0; s < segments.size(); s++) {
                const ClearanceReport& c = segments[s];
                flags |= c.flags & ~(uint32_t)ClearanceReport::Empty;
                if (c.flags & ClearanceReport::Empty) continue;
                if (out.step < 0 || c.clearance < out.clearance) {
                    out.clearance = c.clearance; out.time = c.time; out.x = c.x; out.y = c.y; out.step = c.step; out.gap2 = c.gap2;
                    out.segment = (int32_t)s;
                }
                out.belowSteps += c.belowSteps;
                if (c.firstBelowStep >= 0 && (out.firstBelowStep < 0 || c.firstBelowTime < out.firstBelowTime)) {
                    out.firstBelowTime = c.firstBelowTime; out.firstBelowStep = c.firstBelowStep; out.firstBelowSegment = (int32_t)s;
                }
            }
            out.flags = out.step < 0 ? (uint32_t)ClearanceReport::Empty : flags;
            return out;
        }
        // PlannerConfig::keepoutMargin as this call applied it.  Limit2Requested = limit2 of the margin (ppgpu_keepout_limit2);
        // Limit2Applied = min(Limit2Requested, StartGap2): the planner never demands more clearance than the vehicle has at its
        // start, so a start inside the band (Relaxed) can still plan its way out, and one on a hazard's neighbour plans on the
        // grid as set.  Every free cell the call planned over has certified clearance of at least CertifiedMetres.  With the
        // margin off (or the base Map) everything is 0 and the start's gap2 is not asked for.
        struct KeepoutReport {
            double Margin = 0, CertifiedMetres = 0;           // metres; CertifiedMetres = resolution * sqrt(Limit2Applied)
            uint32_t Limit2Requested = 0, Limit2Applied = 0, StartGap2 = 0;     // cells squared
            bool Relaxed = false;                             // Limit2Applied < Limit2Requested
        };
        KeepoutReport Keepout;
        // PlannerConfig::setPlanReach: the water the call's start can reach and the ribbons beyond it (ppgpu.h, "reachable water"),
        // after the keep-out margin was applied.  FreeCells .. Flags are ppgpu_reach_info's, Ribbons the fields of
        // ppgpu_ribbon_reach_record, one per ribbon of the call's RibbonManager in its order.  Certified = collision checking
        // increment <= resolution: consecutive collision-check poses then lie in the same or in 8-neighbouring cells, so no feasible
        // chain of edges leaves the start's component; otherwise the report makes no claim.  A ribbon that is not out of reach is
        // not thereby coverable (the turning radius may still prevent it).  With the switch off Valid is false and nothing was asked.
        struct ReachReport {
            enum : uint32_t { SeedBlocked = 0x1, NoMap = 0x2 };                                 // PPGPU_REACH_*
            enum : uint32_t { AnyOut = 0x01, WholeOut = 0x02, StartOut = 0x04, EndOut = 0x08, Degenerate = 0x10, Capped = 0x20, NoSeed = 0x40,
                              RibbonNoMap = 0x80 };                                             // PPGPU_RB_*
            struct Ribbon {
                double length = 0, pitch = 0, outLength = 0;
                uint32_t samples = 0, outSamples = 0;
                int32_t firstOut = -1, lastOut = -1;
                uint32_t minRgap2 = 0, maxRgap2 = 0, lim2 = 0, flags = 0;
            };
            bool Valid = false, Certified = false;
            uint64_t FreeCells = 0, ReachableCells = 0;
            uint32_t Components = 0, SeedLabel = 0xFFFFFFFFu, Flags = 0;
            std::vector<Ribbon> Ribbons;
            int RibbonsWhollyOut = 0, RibbonsPartlyOut = 0;    // every sample out; some but not all
            double OutMetres = 0;                              // the records' outLength summed
        };
        ReachReport Reach;
        // PlannerConfig::setPlanWater: how far it is by water from the call's start (ppgpu.h, "distance by water"), after the keep-out
        // margin was applied.  WetCells .. Builds are ppgpu_water_info's, Ribbons the fields of ppgpu_ribbon_water_record, one per ribbon
        // of the call's RibbonManager in its order.  resolution * wd / 12 metres is an upper bound on the shortest route through the
        // centres of free cells, NOT a lower bound on what the vehicle must travel.  Certified as in ReachReport (collision checking
        // increment <= resolution): a ribbon that is dry can then not be approached at all; otherwise the report makes no claim about
        // that.  With the switch off Valid is false and nothing was asked.
        struct WaterReport {
            enum : uint32_t { SeedBlocked = 0x1, NoMap = 0x2 };                                 // PPGPU_WATER_*
            enum : uint32_t { AnyDry = 0x01, WholeDry = 0x02, Degenerate = 0x10, NoSeed = 0x40, RibbonNoMap = 0x80 };   // PPGPU_RW_*
            static constexpr uint32_t None = 0xFFFFFFFFu;                                       // PPGPU_WATER_NONE
            struct Ribbon {
                double length = 0, pitch = 0, nearestMetres = 0;
                uint32_t samples = 0, wetSamples = 0;
                int32_t nearestSample = -1, farthestSample = -1;
                uint32_t minAd = None, maxAd = None, startAd = None, endAd = None, lim2 = 0, flags = 0;
            };
            bool Valid = false, Certified = false;
            uint64_t WetCells = 0;
            uint32_t MaxWd = 0, FarthestCell = None, SeedCell = None, Flags = 0, Rounds = 0, Builds = 0;
            double Resolution = 0, MaxMetres = 0;              // of the grid the map was built on; Resolution * MaxWd / 12
            std::vector<Ribbon> Ribbons;
            int RibbonsDry = 0;                                // no sample can be approached
            int NearestRibbon = -1;                            // the smallest minAd (the lowest index on a tie); -1 without a wet ribbon
            double NearestWaterMetres = -1, NearestStraightMetres = -1;   // its nearestMetres; the straight line from the start to its nearestSample point
            // PlannerConfig::setPlanWaterRoute (ppgpu.h, "route by water"): which way those distances go.  One route per ribbon, to the
            // approach cell of its nearestSample point (sample 0, and a dry route, without a wet sample): the fields of
            // ppgpu_water_route_record, flags and the code of firstDir taken apart, and the vertices (the seed's cell, the turns, the
            // approach cell; at most 256, the seed's end kept) as the centres of their cells.  Empty with that switch off.
            struct RouteReport {
                enum : uint32_t { Dry = 0x01, Outside = 0x02, AtSeed = 0x04, Truncated = 0x08, NoSeed = 0x40, RouteNoMap = 0x80 };   // PPGPU_WR_*
                uint32_t pointCell = None, fromCell = None, wd = None, lim2 = 0, straightSteps = 0, diagonalSteps = 0, turns = 0, vertices = 0;
                uint32_t verticesWritten = 0, firstDir = 0xFF, flags = 0, minGap2 = None, minGap2Cell = None;
                double metres = 0, narrowestMetres = 0;
                std::vector<std::pair<double, double>> Vertices;   // (x, y) = ((c + 0.5) * resolution, (r + 0.5) * resolution), from the seed
            };
            std::vector<RouteReport> Routes;
            int NearestRoute = -1;                             // the index into Routes of NearestRibbon; -1 without one or with the switch off
        };
        WaterReport Water;
        // The vertices the walk over the previous plan made (AStarPlanner.cpp:46-59), in order: what each leg costs in this cycle's world
        struct PreviousLeg { double g, collisionPenalty; bool infeasible; };
        std::vector<PreviousLeg> PreviousPlanLegs;
        // extra, for parity checks against the CPU oracle
        long FirstGoalIteration = -1;
        unsigned long EdgesCosted = 0;
        unsigned long HostHeuristics = 0;     // children whose ribbon list exceeded the device's TSP enumeration: h computed on the host
        unsigned long TableHeuristics = 0;    // PlannerConfig::deviceTspTable: costed records (speculated ones included) the device's table pass answered ...
        unsigned long TableRefused = 0;       // ... and refused for a tie of sort keys (ppgpu_tsp_table_stats over this plan())
        unsigned long DeadlineStops = 0;      // round trips / sample doublings not started because they could not end before the deadline
        unsigned long OrderFallbacks = 0;     // (vertex, radius) lists whose push order the device could not replay (ppgpu_order_fallbacks)
        // Where the budget of this call went, for the time contract ("guaranteed to return before timeRemaining has elapsed",
        // Planner.h:42): wall milliseconds from plan()'s entry, measured with the steady clock whatever clock is injected.
        struct BudgetTrace {
            double PrologueMs = 0;            // entry -> first pass of the big loop (world upload, sampler, root, previous plan)
            double LoopEndMs = 0;             // when the big loop was left
            double TotalMs = 0;               // when plan() returned
            int LastOpKind = 0;               // the last device operation started: 0 none, 1 round trip, 2 sample doubling, 3 Brown-path re-cost
            double LastOpStartMs = 0, LastOpPredictedMs = 0, LastOpActualMs = 0;
            double MarginMs = 0;              // what the deadline guard kept clear of the deadline
            double MaxTripMs = 0;             // the slowest round trip of the call
            double WorstUnderPredictionMs = 0;   // max over guarded operations of (actual - predicted)
            unsigned long NodeRegrowths = 0;  // reallocations of the search tree's node array inside the call ...
            double NodeRegrowthMs = 0;        // ... and what they took
            unsigned long DeviceGrowths = 0;  // device / pinned buffers the device library grew inside the call (ppgpu_growth_stats) ...
            double DeviceGrowthMs = 0;        // ... and what that took
            unsigned long RoundTrips = 0;
            unsigned long PrologueTrips = 0;  // device round trips of the previous-plan pass (one per leg, or one for the whole chained prefix)
            unsigned long StrideRetries = 0;  // round trips repeated because a child's ribbon list did not fit the stride they were costed with
            double MaxWakeMs = 0;             // the longest a context's thread took to start a round trip handed to it
            double PickMs = 0, MaxPickMs = 0;  // choosing the open vertices of the round trips (pickBatch): total and the longest single walk
            bool GridUploaded = false;        // the occupancy grid went to the device in this call (false: the device already held this map)
        } Budget;
    };
    Planner();
    virtual ~Planner() = default;
    virtual Stats plan(const RibbonManager& ribbonManager, const State& start, PlannerConfig config,
                       const DubinsPlan& previousPlan, double timeRemaining);
    void setConfig(PlannerConfig config) { m_Config = std::move(config); }

protected:
    double now() const { return m_Config.now(); }
    PlannerConfig m_Config;
    Stats m_Stats;
};

// One search-tree node: what Vertex + its parent Edge hold in the reference (Vertex.h:180-187, Edge.h:133-143)
struct SearchNode {
    State state;
    int parent = -1;
    RibbonManager ribbons;
    double g = -1, h = -1;
    bool coverageAllowed = false;
    bool infeasible = false;
    double collisionPenalty = 0;
    int steps = 0;             // collision-check steps the edge's sweep executed (visualisation only)
    DubinsWrapper wrapper;     // parent edge's curve
    double f() const { return g + h; }
};

// What one device round trip of GpuAStarPlanner brought back — edge descriptors, records, child ribbons, compacted vertex by
// vertex — kept whole: the children of an open vertex costed ahead of its expansion are a RANGE of one block, not copies.  Blocks
// are recycled through their context's pool (a 300 KB buffer from malloc is a fresh mmap, page faults and all, every time).
struct TripBlock {
    std::unique_ptr<uint64_t[]> edges;
    std::unique_ptr<unsigned char[]> records;     // ppgpu_edge_result (128 bytes) each
    std::unique_ptr<double[]> child;              // `stride` x 4 doubles per edge
    size_t edgeCap = 0, childCap = 0;
    int stride = 0;
    // PlannerConfig::deviceTrajectories with the search dump on (traceStride > 0): how many steps the device traced of every edge
    // of the round trip, and the ones the dump prints — every tracePer-th, Edge.cpp:135-136 — traceStride slots per edge
    std::vector<int32_t> traceCounts;
    std::vector<Planner::Stats::TraceStep> traceSteps;     // [edge][traceStride]: steps tracePer - 1, 2 tracePer - 1, ...
    int traceStride = 0, tracePer = 1;
    void reserve(size_t nEdges, size_t childDoubles);
};

// Process-level device handle: stream, persistent buffers (the reference builds a new planner every cycle,
// executive.cpp:85-90, so nothing device-side may live in the planner object).  Throws std::runtime_error.
// shared(device) hands out ONE context per device for the life of the process: the cache holds a strong reference, so the
// buffers a cycle grew (samples, workspace, pinned staging) are there for the next cycle's planner; releaseShared() drops them.
// Each context owns one host thread bound to its device: a planner that is given several contexts runs its per-device work
// there (run()), so the devices of a node cost their parts of a batch at the same time.
class GpuContext {
public:
    explicit GpuContext(int device = 0);
    ~GpuContext();
    GpuContext(const GpuContext&) = delete;
    GpuContext& operator=(const GpuContext&) = delete;
    ppgpu_ctx* handle() const { return m_Handle; }
    int device() const { return m_Device; }
    // one per (device, lane) per process, kept until releaseShared().  Lane 0 is "the" context of a device; further lanes are further
    // streams (with their own buffers) on the same device: a planner given {shared(0, 0), shared(0, 1)} keeps two round trips in flight.
    static std::shared_ptr<GpuContext> shared(int device = 0, int lane = 0);
    static std::vector<std::shared_ptr<GpuContext>> shared(const std::vector<int>& devices);
    static void releaseShared();
    // run `job` on this context's thread; wait() blocks until it has finished and rethrows what it threw
    void run(std::function<void()> job);
    void wait();
    bool idle();               // no job of run() is running (its result, or what it threw, is waiting for wait())

    // What this device's recent round trips and sample doublings took (wall seconds), kept with the context so that the first
    // cycle of a new planner already knows: the deadline guard (PlannerConfig::deadlineGuard) predicts the next one from them.
    // Written and read by the planning thread only.
    struct Observed { double samples = 0, seconds = 0; };
    static constexpr int kTrips = 8;
    Observed trips[kTrips];   // the last round trips of expandBatch: sample count, duration
    int tripSlot = 0;
    Observed doubling;        // the last addSamples: attempts, duration
    void noteTrip(double samples, double seconds) { trips[tripSlot] = {samples, seconds}; tripSlot = (tripSlot + 1) % kTrips; }
    // a round trip over `samples` samples: no longer than the recent ones scaled up to that sample count (their cost grows
    // less than linearly), plus 15 %
    double predictTrip(double samples) const {
        double worst = 0;
        for (const Observed& o : trips)
            if (o.seconds > 0) worst = std::max(worst, o.seconds * std::max(1.0, samples / std::max(1.0, o.samples)));
        return worst * 1.15 + 1e-4;
    }
    double predictDoubling(double attempts) const {
        if (doubling.seconds <= 0) return 0;
        return doubling.seconds * std::max(1.0, attempts / std::max(1.0, doubling.samples)) * 1.15 + 1e-4;
    }
    // How far a round trip overran its prediction, remembered for a while (round 4: one trip in a few hundred takes 0.8-3 ms longer
    // than any of the eight before it scaled to its sample count would suggest — children with long ribbon lists whose heuristic one
    // wavefront enumerates, a second pass at a larger child stride — and when it happened to be a cycle's last the cycle ended
    // 0.05-0.4 ms late): the largest excess seen, decaying by 0.1 % per round trip (half of it is left four cycles later), at most 3 ms.
    double tailExcess = 0;
    void noteExcess(double seconds) { tailExcess = std::max(tailExcess * 0.999, std::min(seconds, 3e-3)); }
    // What the guard keeps clear of the deadline on top of its predictions, so that "before" holds and not "at": half a
    // millisecond (the return path: tracing the plan, the caller's clock read), or twice the spread of the recent round trips,
    // or the remembered excess above, whichever is largest.
    double guardMargin() const {
        double n = 0, sum = 0, sq = 0;
        for (const Observed& o : trips)
            if (o.seconds > 0) { n += 1; sum += o.seconds; sq += o.seconds * o.seconds; }
        double sigma = 0;
        if (n >= 2) { const double mean = sum / n; sigma = std::sqrt(std::max(0.0, sq / n - mean * mean)); }
        return std::max(std::max(5e-4, 2 * sigma), tailExcess);
    }
    // The search tree's node array lives HERE between plan() calls (a planner takes it at the start of plan() and hands it back,
    // emptied, when it is destroyed): its capacity — and its pages — survive the cycle.  Measured in round 4 (Stats::Budget): a
    // std::vector that doubles at 65 536 nodes moves 16 MB and faults in 31 MB of fresh pages, 6.9 ms inside a 100 ms budget —
    // round 3's unexplained +6 ms cycles.
    std::vector<SearchNode> nodeArena;
    // Which occupancy map the device holds (identity + Map::version): the planner of the next cycle uploads the grid only when
    // the Executive has been given another map.  nullptr / 0: nothing cached.
    // The range of the table pass this context's two switches were last set to by a planner (-1: never set): beginCall sets them
    // again only when the call's PlannerConfig::deviceTspTable differs.
    int tspTableRibbons = -1;
    const void* gridOf = nullptr;
    unsigned long gridVersion = 0;
    double gridResolution = 0;             // cell size of the grid the device holds (0: the base Map, no grid), whichever call uploaded it
    int gridRows = 0, gridCols = 0;        // ... and its shape
    // ppgpu_water_routes_host against the water map of the handle's current seed: one record per point {x, y} and up to `stride`
    // vertices per route in vertices[i * stride ...] (slots no route wrote hold PPGPU_WATER_NONE).  Throws std::runtime_error.
    std::vector<ppgpu_water_route_record> waterRoutes(const std::vector<double>& pointsXY, uint32_t lim2, int stride, std::vector<uint32_t>& vertices);
    // round-trip result blocks not referred to by any planner any more are handed out again (used by this context's thread only)
    std::vector<std::shared_ptr<TripBlock>> tripPool;
    std::shared_ptr<TripBlock> takeTripBlock(size_t nEdges, size_t childDoubles);

private:
    ppgpu_ctx* m_Handle = nullptr;
    int m_Device = 0;
    std::thread m_Thread;
    std::mutex m_Mutex;
    std::condition_variable m_Wake;
    std::function<void()> m_Job;
    bool m_Busy = false, m_Quit = false;
    std::atomic<bool> m_Running{false};    // run() .. the end of its job (wait() polls it for a while before it sleeps)
    std::atomic<bool> m_Posted{false};     // a job is waiting (what the thread polls for a millisecond after each job before it sleeps)
    std::exception_ptr m_Error;
    void serve();
};

class GpuAStarPlanner : public Planner {
public:
    explicit GpuAStarPlanner(std::shared_ptr<GpuContext> ctx = GpuContext::shared()) : m_Ctx(ctx), m_Ctxs{ctx} {}
    // several devices of one node: world and samples are replicated on each (the sampler stream is deterministic: every device
    // draws the same samples itself), the open vertices of a batch are dealt across them, records come back to the host search
    explicit GpuAStarPlanner(std::vector<std::shared_ptr<GpuContext>> ctxs) : m_Ctx(ctxs.at(0)) {
        for (auto& c : ctxs)                 // (a context named twice is one context)
            if (std::find(m_Ctxs.begin(), m_Ctxs.end(), c) == m_Ctxs.end()) m_Ctxs.push_back(c);
    }
    ~GpuAStarPlanner() override;      // the search tree is torn down here, as the reference's is (not inside plan()'s budget)
    Stats plan(const RibbonManager& ribbonManager, const State& start, PlannerConfig config, const DubinsPlan& previousPlan,
               double timeRemaining) override;

    typedef SearchNode Node;

    // What a whole plan costs in the current world and how far along it is still feasible (evaluatePlans).
    struct PlanEvaluation {
        struct Leg { bool feasible = false; double g = 0, collisionPenalty = 0; };
        enum Stop { RanOutOfLegs = 1, Infeasible = 2, Goal = 3, Throws = 4, Capacity = 5 };     // PPGPU_CHAIN_*
        int legsCosted = 0;                   // legs walked, the one the walk stopped at included
        Stop stop = RanOutOfLegs;
        std::vector<Leg> legs;                // [legsCosted]
        double g = 0;                         // currentCost of the last feasible vertex reached (0: none)
        double collisionPenalty = 0;          // summed over the feasible legs
        double coverageCompletedTime = -1;    // of that vertex's RibbonManager
        bool goalReached = false;
        RibbonManager ribbons;                // ... and what it has left to cover
        std::vector<Planner::Stats::Contact> contacts;   // PlannerConfig::setPlanContacts: the costed legs merged, per contact (Stats::mergeContacts)
        Planner::Stats::ClearanceReport clearance;       // PlannerConfig::setPlanClearance: the costed legs merged (Stats::mergeClearance)
        Planner::Stats::KeepoutReport keepout;           // PlannerConfig::setKeepoutMargin as the call applied it (the same for every plan)
        Planner::Stats::ReachReport reach;               // PlannerConfig::setPlanReach: what the call's start can reach (the same for every plan)
        Planner::Stats::WaterReport water;               // PlannerConfig::setPlanWater: how far it is by water from the call's start (likewise)
    };
    // AStarPlanner::plan's walk over a previous plan (AStarPlanner.cpp:46-59) for ANY number of candidate plans, all from `start`,
    // in one device call (ppgpu_cost_plans_host).  Legs are filtered as plan() filters them (:49-50); a leg at a radius the
    // configuration no longer has ends its plan's walk before it (legsCosted says how far it got, stop == RanOutOfLegs).
    std::vector<PlanEvaluation> evaluatePlans(const RibbonManager& ribbonManager, const State& start, PlannerConfig config,
                                              const std::vector<DubinsPlan>& plans);

private:
    std::shared_ptr<GpuContext> m_Ctx;                    // device 0 of this planner: sampling read-back, wrapper edges, explicit targets
    std::vector<std::shared_ptr<GpuContext>> m_Ctxs;      // all of them (m_Ctxs[0] == m_Ctx)
    std::vector<Node> m_Nodes;
    // binary heap of node indices, min f (AStarPlanner.cpp:6-10).  Each entry carries its node's f: the heap's comparisons then read
    // 16-byte neighbours instead of two 400-byte nodes somewhere in a 100 MB tree (round 4: a push's cache misses were most of the
    // 0.3 us a child cost the planner's thread).  Same comparisons, same results, same heap.
    struct QEntry { double f; int v; };
    std::vector<QEntry> m_Queue;
    int m_Best = -1;
    double m_StartStateTime = 0;
    RibbonManager m_RibbonManager;
    long m_NumSamples = 0;
    // Edges of open vertices costed ahead of their expansion, as the device returned them: a child Node is built only when the
    // search expands the parent, and only for edges it would push (an infeasible edge never becomes a vertex).
    struct Costed {
        std::shared_ptr<TripBlock> block;     // the round trip that costed them
        size_t first = 0, count = 0;          // this vertex's edges: [first, first + count) of the block, in push order
        // children built ahead while the planner's thread waited for a round trip (prebuildWhileWaiting): kids[i] is edge first + i's
        // child vertex, complete, where ready[i] is set; the others are left to expand() (never pushed, or the planner's own judgement)
        std::vector<Node> kids;
        std::vector<unsigned char> ready;
    };
    std::unordered_map<int, Costed> m_Speculated;

    void pushVertexQueue(int v);
    int popVertexQueue();
    bool goalCondition(const Node& v) const;
    bool expand(int source);               // false: the deadline guard did not start the round trip it needed
    struct Batch;                          // one device round trip, from the pick to the harvest (planner.cpp)
    std::vector<std::shared_ptr<Batch>> m_InFlight;        // started, not yet harvested: at most one per context
    std::unordered_map<int, Batch*> m_InFlightOf;          // open vertex -> the round trip that is costing its children
    void packBatch(Batch& b) const;
    static void runBatch(Batch& b, int k);
    void harvestFinished();
    void submitBatch(std::shared_ptr<Batch> b, GpuContext& ctx);
    void harvestBatch(Batch* b, bool keep);
    std::shared_ptr<Batch> dropBatch(Batch* b);
    void drainInFlight();
    GpuContext& freeContext();
    void pickBatch(int source, std::vector<int>& batch);
    std::shared_ptr<Batch> pickedBatch(int source);        // a new Batch: pickBatch + the guard's allowance for its longest ribbon list
    double m_EndTime = 0;                  // the deadline of this plan() call, on the injected clock
    int costEdgeList(const std::vector<uint64_t>& edges, int maxParentRibbons, std::vector<::ppgpu_edge_result>& res, std::vector<double>& child);
    // record -> Node, the one path: makeChild judges (throws, counts the host heuristic), fillChild only fills.  `given`: a previous plan's leg
    Node makeChild(int source, unsigned cfgBits, const ::ppgpu_edge_result& r, const double* childRibbons, int stride, const DubinsWrapper* given = nullptr);
    void fillChild(Node& c, int source, unsigned cfgBits, const ::ppgpu_edge_result& r, const double* childRibbons, const DubinsWrapper* given = nullptr) const;
    void prebuildWhileWaiting(GpuContext& busy);
    void addNode(Node&& n);                // m_Nodes.push_back that counts and times reallocations (Stats::Budget)
    void noteOperation(int kind, double startedAt, double predicted, double actual);
    double m_PlanEntry = 0;                // steady-clock time of plan()'s entry
    bool m_DeadlineStop = false;           // aStar() stopped on the deadline guard: the big loop ends too
    int m_StrideFloor = 0;                 // child-ribbon stride a round trip of this plan() had to be repeated with: later ones start there
    int aStar(double endTime);
    void addSamples(long n);
    std::vector<int> branch(int v) const;  // root's child .. v
    void packVertices(const std::vector<int>& nodes, std::vector<::ppgpu_vertex>& verts, std::vector<double>& pool) const;
    // plan() step by step (planner.cpp, in this order)
    void resetSearch();
    struct DeviceCounters;
    DeviceCounters deviceCounters() const;
    Node beginCall(const RibbonManager& ribbonManager, const State& start);      // shared with evaluatePlans
    void reportReach(const State& start);                                         // ... PlannerConfig::planReach from the first context (after applyKeepout)
    void reportWater(const State& start);                                         // ... PlannerConfig::planWater, likewise
    void reportWaterRoutes(Stats::WaterReport& r, const std::vector<ppgpu_ribbon_water_record>& recs);   // ... PlannerConfig::planWaterRoute, into reportWater's report
    void applyKeepout(const State& start);                                        // ... PlannerConfig::keepoutMargin on every context
    void initSampler(const State& start, unsigned long seed);
    struct WalkedLegs;                     // the previous-plan leg filter
    size_t costGivenLegs(const WalkedLegs& walked, std::vector<::ppgpu_edge_result>& res, std::vector<double>& child);
    void reSolveLeg(int source, const DubinsWrapper& p);
    int walkPreviousPlan(const DubinsPlan& previousPlan, std::vector<int>& made);
    bool costBrownPathSeeds(const std::vector<State>& seeds, double tPoll, double endTime);
    void anytimeLoop(double endTime, int lastPlanEnd, const std::vector<int>& previousPlanNodes, const std::vector<State>& brownPathSamples);
    void reportPlan();
    DubinsPlan tracePlan(int v, bool addToStats = true);
    void setOpenVertex(const Node& n);     // ppgpu_set_vertices on the planner's own device: this node alone
    // the reference's search dump (SamplingBasedPlanner.cpp:210-238, Edge.cpp:122-143); no-ops unless the config enables it
    void visualizeVertex(int v, const char* tag, bool expanded);
    void visualizeTrajectory(const Node& child, const Stats::TraceStep* steps = nullptr, int count = 0);
    // Reports about a plan, one route (planner.cpp): Segments = what the device sweeps again (open vertices, one wrapper edge per segment,
    // the steps its costed edge executed), built from a branch of the tree or from the records of a ppgpu_cost_plans_host call;
    // sweepSegments = one device call per report asked for -> out.Trace / Coverage / Contacts / Clearance, per segment.  tracePlanSteps: those of
    // the plan that ends at node v into m_Stats (whatever m_Config has on); evaluationReports: contacts and clearance merged per candidate plan.
    struct Segments;
    Segments branchSegments(int v) const;
    static Segments chainSegments(const Node& root, const std::vector<int32_t>& offsets, const std::vector<ppgpu_wrapper_edge>& legs,
                                  const std::vector<ppgpu_edge_result>& res, const std::vector<double>& child, const std::vector<int32_t>& costed);
    std::vector<uint32_t> sweepSegments(const Segments& seg, bool trace, bool coverage, bool contacts, bool clearance, Stats& out);
    void tracePlanSteps(int v);
    void evaluationReports(const Node& root, const std::vector<int32_t>& offsets, const std::vector<ppgpu_wrapper_edge>& legs,
                            const std::vector<ppgpu_edge_result>& res, const std::vector<double>& child, const std::vector<int32_t>& costed,
                            std::vector<PlanEvaluation>& out);
    void visualizePlan(const DubinsPlan& plan);
    void visualizeSamples();
    int costStateEdges(int source, const std::vector<State>& targets, const std::vector<unsigned>& cfgBits,
                       const std::vector<long>& sampleIndex);
};

// One planner iteration in its BATCH form, sample-sharded over the GPUs of a node (SURVEY.md 8 e; BASELINE's north_star: "the
// sample batch shards naturally across the 8 GPUs of one node with a single RCCL all-reduce of the per-shard best cost/vertex
// each iteration").  The iteration's batch of `attempts` draws from the StateGenerator stream is cut into contiguous slices, one
// per device context; every device skips the slices below its own (ppgpu_sampler_skip), draws and filters its slice, costs the
// edges from the open vertex to its samples under the four (radius, speed) configurations and reduces its best (f, edge); then
// ONE collective — ppgpu_allreduce_best on the communicator ppgpu_comm_init_all made of the contexts — leaves the global
// incumbent on every device.  No sample, edge or record crosses between devices.  Each context's work runs on its own host
// thread (GpuContext::run), which is also what the collective needs: every rank must have joined before any returns.
// The reference has no counterpart (its incumbent update is AStarPlanner.cpp:109-117 on one thread); GpuAStarPlanner's anytime
// search keeps dealing open VERTICES to the devices (the host pops goals in f order, no collective needed there).
class ShardedIteration {
public:
    struct Result {
        double f = 0;                          // the global incumbent: smallest f over every shard's feasible edges ...
        uint64_t fBits = ~0ull, edge = ~0ull;  // ... its bit pattern and global edge id (shard * edgesPerShard + local index); ~0: none
        int shard = -1;                        // which device found it
        std::vector<int64_t> kept;             // samples each shard kept (map filter)
        int64_t edges = 0;                     // edges costed over all shards
        int rcclRanks = 0;                     // ncclCommCount of the communicator (0: host combine, see below)
        bool agreed = false;                   // every device ended with the same key
    };
    // One context per device: the communicator is RCCL's.  Two contexts on ONE device (a one-GPU box rehearsing the split) cannot
    // form one — RCCL takes one rank per device — and the keys are then combined on the host instead; Result::rcclRanks says which.
    explicit ShardedIteration(std::vector<std::shared_ptr<GpuContext>> ctxs);
    ~ShardedIteration();
    // Throws what a shard threw.  A shard that fails before the collective keeps every shard out of it (nothing is left waiting);
    // a failure inside the collective aborts the communicators (ppgpu_comm_abort) so that the other ranks return.
    Result run(const RibbonManager& ribbonManager, const State& start, const PlannerConfig& config, unsigned long seed, int64_t attempts);
    int failShardForTest = -1;                 // tests only: this shard throws at the start of its work

private:
    void release();
    std::vector<std::shared_ptr<GpuContext>> m_Ctxs;
    std::vector<void*> m_Keys, m_Records;      // per device: the 16-byte key and the record buffer (device memory)
    std::vector<size_t> m_RecordCap;
    bool m_Rccl = false;
};

}  // namespace ppamd
