// plan_cli — drives GpuAStarPlanner::plan() from a small text scenario and prints the Stats as JSON.
// Used by tests/test_gpu_host_planner.py to compare the C++ host path with the CPU oracle's AStarPlanner::plan
// under the same injected clock (PlannerConfig::setNowFunction).
//
// Scenario lines:  cfg <key> <value> | start x y heading speed time | ribbon x1 y1 x2 y2 | heuristic H K radius |
//                  ribbon_width w | obstacle x y heading speed time width length | gaussian x y heading speed time [c00 c01 c10 c11] | map_file path | clock t0 dt |
//                  plan_trace_file path (with cfg plan_trace 1: one line per step of the returned plan) |
//                  plan_coverage_file path (with cfg plan_coverage 1: one line per step, what it did to the ribbons) |
//                  plan_contacts_file path (with cfg plan_contacts 1: one line per segment and contact, what the segment has to do with it;
//                  the MMSIs are those the obstacle / gaussian lines were given, 1, 2, ... in file order) |
//                  plan_clearance_file path (with cfg plan_clearance 1, and cfg plan_clearance_margin M in metres: one line per segment, how
//                  close it passes to a charted hazard and how many of its steps lie inside the margin) |
//                  cfg keepout_margin M (PlannerConfig::setKeepoutMargin: plan M metres clear of charted hazards; a value other than 0 adds
//                  keepout_margin, keepout_limit2, keepout_certified and keepout_relaxed to the JSON, and to every plan under evaluate) |
//                  cfg plan_reach 1 (PlannerConfig::setPlanReach: which water the start can reach and which ribbons lie beyond it; adds
//                  reach_free_cells, reach_cells, reach_components, reach_certified, reach_seed_blocked, ribbons_out_of_reach,
//                  ribbons_partly_out_of_reach and out_of_reach_metres to the JSON, and to every plan under evaluate) |
//                  plan_reach_file path (with cfg plan_reach 1: one line per ribbon of the call) |
//                  cfg plan_water 1 (PlannerConfig::setPlanWater: how far it is by water from the start to the chart's cells and to every
//                  ribbon; adds water_cells, water_max_metres, water_seed_blocked, water_rounds, ribbons_dry, nearest_ribbon_by_water,
//                  nearest_ribbon_water_metres and nearest_ribbon_straight_metres to the JSON, and to every plan under evaluate) |
//                  plan_water_file path (with cfg plan_water 1: one line per ribbon of the call) |
//                  cfg plan_water_route 1 (PlannerConfig::setPlanWaterRoute, with cfg plan_water 1: which way the distance by water goes;
//                  adds water_route_metres, water_route_turns, water_route_vertices, water_route_truncated, water_route_narrowest_metres
//                  and water_route_first_dir of the ribbon nearest by water to the JSON, and to every plan under evaluate) |
//                  plan_water_route_file path (with both: one line per vertex of every ribbon's route, from the start) |
//                  time_remaining T | prev qi0 qi1 qi2 p0 p1 p2 rho type speed start end | repeat n |
//                  sharded_batch attempts seed   (instead of plan(): one iteration's batch, sample-sharded over `devices`: ShardedIteration)
//                  cfg chained_previous_plan 0|1 (PlannerConfig::setChainedPreviousPlan; naming it at all adds round_trips, prologue_trips,
//                  prologue_ms and previous_plan_legs to the JSON) | evaluate (instead of plan(): GpuAStarPlanner::evaluatePlans on the `prev`
//                  plan, or on every prev_begin ... prev_end block of prev lines; one JSON line of PlanEvaluations) |
//                  cfg device_tsp_table N (PlannerConfig::setDeviceTspTable; naming it at all adds table_heuristics and table_refused to the JSON) |
//                  replan_clock_calls n (replan under a counting clock: every cycle gets n polls of dt) | plan_log path (replan: one JSON
//                  line per cycle with the plan and the search counters)
#include <algorithm>
#include <array>
#include <chrono>
#include <cstdio>
#include <fstream>
#include <iostream>
#include <sstream>
#include <string>

#include "path_planner_amd/Planner.h"

using namespace ppamd;

// ", plan_contacts_hit ..., nearest_contact_mmsi ..., nearest_contact_cpa ..." of a plan's merged contact records (-1 / -1 without a
// contact that has a closest approach)
static std::string contactKeys(const std::vector<Planner::Stats::Contact>& contacts) {
    int hit = 0;
    long nearest = -1;
    double cpa = -1;
    for (const Planner::Stats::Contact& c : contacts) {
        if (c.hitSteps > 0) hit++;
        if (c.cpaStep >= 0 && (nearest < 0 || c.cpaDistance < cpa)) { nearest = (long)c.mmsi; cpa = c.cpaDistance; }
    }
    char buf[160];
    std::snprintf(buf, sizeof buf, ", \"plan_contacts_hit\": %d, \"nearest_contact_mmsi\": %ld, \"nearest_contact_cpa\": %.17g", hit, nearest, cpa);
    return buf;
}

// ", plan_clearance ..., plan_clearance_time ..., plan_below_margin_steps ..." of a plan's merged clearance report (-1 / -1 / 0 for an
// empty plan)
static std::string clearanceKeys(const Planner::Stats::ClearanceReport& c) {
    char buf[160];
    std::snprintf(buf, sizeof buf, ", \"plan_clearance\": %.17g, \"plan_clearance_time\": %.17g, \"plan_below_margin_steps\": %d", c.clearance, c.time, c.belowSteps);
    return buf;
}

// ", keepout_margin ..., keepout_limit2 ..., keepout_certified ..., keepout_relaxed ..." of a call's Stats::Keepout: the margin asked for, the
// limit2 applied (cells squared), the clearance that certifies in metres, and whether the start's own clearance lowered it
static std::string keepoutKeys(const Planner::Stats::KeepoutReport& k) {
    char buf[200];
    std::snprintf(buf, sizeof buf, ", \"keepout_margin\": %.17g, \"keepout_limit2\": %u, \"keepout_certified\": %.17g, \"keepout_relaxed\": %s", k.Margin, k.Limit2Applied,
                  k.CertifiedMetres, k.Relaxed ? "true" : "false");
    return buf;
}

// ", reach_free_cells ..., ..., out_of_reach_metres ..." of a call's Stats::Reach: the free cells of the effective grid, those the start
// can reach, the components, whether the collision-check pitch certifies the claim, and the ribbons no plan can get to
static std::string reachKeys(const Planner::Stats::ReachReport& r) {
    char buf[360];
    std::snprintf(buf, sizeof buf, ", \"reach_free_cells\": %llu, \"reach_cells\": %llu, \"reach_components\": %u, \"reach_certified\": %s, "
                  "\"reach_seed_blocked\": %s, \"ribbons_out_of_reach\": %d, \"ribbons_partly_out_of_reach\": %d, \"out_of_reach_metres\": %.17g",
                  (unsigned long long)r.FreeCells, (unsigned long long)r.ReachableCells, r.Components, r.Certified ? "true" : "false",
                  (r.Flags & Planner::Stats::ReachReport::SeedBlocked) ? "true" : "false", r.RibbonsWhollyOut, r.RibbonsPartlyOut, r.OutMetres);
    return buf;
}

// ", water_cells ..., ..., nearest_ribbon_straight_metres ..." of a call's Stats::Water: the cells with a distance by water from the start,
// the largest of them in metres, the rounds the build took, the ribbons that cannot be approached, and the ribbon nearest by water with
// its distance by water and in a straight line (-1 for all three without one)
static std::string waterKeys(const Planner::Stats::WaterReport& w) {
    char buf[420];
    std::snprintf(buf, sizeof buf, ", \"water_cells\": %llu, \"water_max_metres\": %.17g, \"water_seed_blocked\": %s, \"water_rounds\": %u, "
                  "\"ribbons_dry\": %d, \"nearest_ribbon_by_water\": %d, \"nearest_ribbon_water_metres\": %.17g, \"nearest_ribbon_straight_metres\": %.17g",
                  (unsigned long long)w.WetCells, w.MaxMetres, (w.Flags & Planner::Stats::WaterReport::SeedBlocked) ? "true" : "false", w.Rounds, w.RibbonsDry,
                  w.NearestRibbon, w.NearestWaterMetres, w.NearestStraightMetres);
    return buf;
}

// ", water_route_metres ..., ..., water_route_first_dir ..." of the route to the ribbon nearest by water (Stats::Water.Routes[NearestRoute]):
// its length, its turns, its vertices and whether the list was cut, its narrowest place and the code of the step that leaves the start
// (-1 for the numbers, false, without a wet ribbon)
static std::string waterRouteKeys(const Planner::Stats::WaterReport& w) {
    char buf[420];
    if (w.NearestRoute < 0) {
        std::snprintf(buf, sizeof buf, ", \"water_route_metres\": -1, \"water_route_turns\": -1, \"water_route_vertices\": -1, \"water_route_truncated\": false, "
                      "\"water_route_narrowest_metres\": -1, \"water_route_first_dir\": -1");
        return buf;
    }
    const auto& r = w.Routes[(size_t)w.NearestRoute];
    std::snprintf(buf, sizeof buf, ", \"water_route_metres\": %.17g, \"water_route_turns\": %u, \"water_route_vertices\": %u, \"water_route_truncated\": %s, "
                  "\"water_route_narrowest_metres\": %.17g, \"water_route_first_dir\": %u",
                  r.metres, r.turns, r.vertices, (r.flags & Planner::Stats::WaterReport::RouteReport::Truncated) ? "true" : "false", r.narrowestMetres, r.firstDir);
    return buf;
}

// One report file: rows(f, s) prints the lines of segment s.  No path, no file; -> false (and the complaint) when it cannot be written.
template <class Rows>
static bool writeReport(const std::string& path, size_t segments, Rows rows) {
    if (path.empty()) return true;
    FILE* f = std::fopen(path.c_str(), "w");
    if (!f) { std::fprintf(stderr, "cannot write %s\n", path.c_str()); return false; }
    for (size_t sg = 0; sg < segments; sg++) rows(f, sg);
    std::fclose(f);
    return true;
}

int main(int argc, char** argv) {
    if (argc < 2) { std::fprintf(stderr, "usage: plan_cli scenario.txt\n"); return 2; }
    std::ifstream in(argv[1]);
    if (!in) { std::fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    PlannerConfig config(&std::cerr);
    State start;
    int H = 0, K = 0;
    double hr = 8;
    std::vector<std::array<double, 4>> ribs;
    auto obst = std::make_shared<BinaryDynamicObstaclesManager>();
    auto gauss = std::make_shared<GaussianDynamicObstaclesManager>();
    bool haveObst = false, haveGauss = false;
    Map::SharedPtr map = std::make_shared<Map>();
    double t0 = 1000, dt = 1e-3, timeRemaining = 0.05;
    DubinsPlan prev;
    int repeat = 1;
    bool realClock = false;
    int replans = 0;
    double replanStep = 0.1;
    uint32_t mmsi = 1;
    std::vector<int> devices;
    long long shardedAttempts = 0;
    unsigned long shardedSeed = 7;
    int failShard = -1;
    std::string cycleLogPath, planTracePath, planCoveragePath, planContactsPath, planClearancePath, planReachPath, planWaterPath, planWaterRoutePath, planLogPath;
    bool chainNamed = false, tableNamed = false, evaluate = false, inBlock = false;
    std::vector<DubinsPlan> candidates;
    long replanClockCalls = 0;
    std::string line;
    while (std::getline(in, line)) {
        std::istringstream s(line);
        std::string k;
        if (!(s >> k)) continue;
        if (k == "cfg") {
            std::string name; double v; s >> name >> v;
            if (name == "max_speed") config.setMaxSpeed(v);
            else if (name == "slow_speed") config.setSlowSpeed(v);
            else if (name == "turning_radius") config.setTurningRadius(v);
            else if (name == "coverage_turning_radius") config.setCoverageTurningRadius(v);
            else if (name == "time_horizon") config.setTimeHorizon(v);
            else if (name == "time_minimum") config.setTimeMinimum(v);
            else if (name == "collision_checking_increment") config.setCollisionCheckingIncrement(v);
            else if (name == "branching_factor") config.setBranchingFactor((int)v);
            else if (name == "initial_samples") config.setInitialSamples((int)v);
            else if (name == "use_brown_paths") config.setUseBrownPaths(v != 0);
            else if (name == "speculation") config.setSpeculation((int)v);
            else if (name == "plan_trace") config.setPlanTrace(v != 0);
            else if (name == "plan_coverage") config.setPlanCoverage(v != 0);
            else if (name == "plan_contacts") config.setPlanContacts(v != 0);
            else if (name == "plan_clearance") config.setPlanClearance(v != 0);
            else if (name == "plan_clearance_margin") config.setPlanClearanceMargin(v);
            else if (name == "keepout_margin") config.setKeepoutMargin(v);
            else if (name == "plan_reach") config.setPlanReach(v != 0);
            else if (name == "plan_water") config.setPlanWater(v != 0);
            else if (name == "plan_water_route") config.setPlanWaterRoute(v != 0);
            else if (name == "device_trajectories") config.setDeviceTrajectories(v != 0);
            else if (name == "chained_previous_plan") { config.setChainedPreviousPlan(v != 0); chainNamed = true; }
            else if (name == "device_tsp_table") { config.setDeviceTspTable((int)v); tableNamed = true; }
            else { std::fprintf(stderr, "unknown cfg %s\n", name.c_str()); return 2; }
        } else if (k == "start") {
            double x, y, h, v, t; s >> x >> y >> h >> v >> t; start = State(x, y, h, v, t);
        } else if (k == "ribbon") {
            std::array<double, 4> r; s >> r[0] >> r[1] >> r[2] >> r[3]; ribs.push_back(r);
        } else if (k == "heuristic") { s >> H >> K >> hr;
        } else if (k == "ribbon_width") { double w; s >> w; RibbonManager::setRibbonWidth(w);
        } else if (k == "obstacle") {
            double x, y, h, v, t, w, l; s >> x >> y >> h >> v >> t >> w >> l; obst->update(mmsi++, x, y, h, v, t, w, l); haveObst = true;
        } else if (k == "gaussian") {      // x y heading speed time [c00 c01 c10 c11]
            double x, y, h, v, t, c[4]; s >> x >> y >> h >> v >> t;
            if (s >> c[0] >> c[1] >> c[2] >> c[3]) gauss->update(mmsi++, x, y, h, v, t, c); else gauss->update(mmsi++, x, y, h, v, t);
            haveGauss = true;
        } else if (k == "map_file") { std::string p; s >> p; map = std::make_shared<GridWorldMap>(p);
        } else if (k == "visualization_file") {   // the search dump visualizer.py reads (executive.cpp:443-449)
            std::string p; s >> p;
            config.setVisualizations(true);
            config.setVisualizer(std::make_shared<Visualizer>(p));
        } else if (k == "clock") { s >> t0 >> dt;
        } else if (k == "time_remaining") { s >> timeRemaining;
        } else if (k == "devices") {          // device ids of the planner; an id that repeats gets its own second context on that device
            int d; while (s >> d) devices.push_back(d);
        } else if (k == "sharded_batch") { s >> shardedAttempts >> shardedSeed;
        } else if (k == "fail_shard") { s >> failShard;      // tests: this shard of a sharded_batch throws before its work
        } else if (k == "cycle_log") { s >> cycleLogPath;    // replan: one JSON line per cycle (Stats::Budget and what the cycle reached)
        } else if (k == "plan_trace_file") { s >> planTracePath;   // segment step x y heading time collision penalty_before flags
        } else if (k == "plan_coverage_file") { s >> planCoveragePath;   // segment step time to_cover remaining ribbons flags
        } else if (k == "plan_contacts_file") { s >> planContactsPath;   // segment mmsi hit_steps first_hit_time last_hit_time cpa_distance cpa_time exposure peak
        } else if (k == "plan_clearance_file") { s >> planClearancePath;   // segment clearance time x y step gap2 below_steps first_below_time flags
        } else if (k == "plan_reach_file") { s >> planReachPath;   // ribbon length pitch samples out_samples first_out last_out min_rgap2 max_rgap2 lim2 out_length flags
        } else if (k == "plan_water_file") { s >> planWaterPath;   // ribbon length pitch samples wet_samples nearest_sample farthest_sample min_ad max_ad start_ad end_ad lim2 flags nearest_metres
        } else if (k == "plan_water_route_file") { s >> planWaterRoutePath;   // ribbon j x y
        } else if (k == "plan_log") { s >> planLogPath;
        } else if (k == "replan_clock_calls") { s >> replanClockCalls;
        } else if (k == "evaluate") { evaluate = true;
        } else if (k == "prev_begin") { candidates.emplace_back(); inBlock = true;
        } else if (k == "prev_end") { inBlock = false;
        } else if (k == "repeat") { s >> repeat;
        } else if (k == "replan") { s >> replans >> replanStep;   // N consecutive cycles, start moved replanStep seconds along the plan
        } else if (k == "real_clock") { int v; s >> v; realClock = v != 0;   // now() = t0 + wall seconds since plan() began
        } else if (k == "prev") {
            DubinsPath p; double speed, st, en; int type;
            s >> p.qi[0] >> p.qi[1] >> p.qi[2] >> p.param[0] >> p.param[1] >> p.param[2] >> p.rho >> type >> speed >> st >> en;
            p.type = (DubinsPathType)type;
            DubinsWrapper w; w.fill(p, speed, st);
            if (w.getEndTime() > en) w.updateEndTime(en);
            if (inBlock) candidates.back().append(w); else prev.append(w);
        }
    }
    RibbonManager rm((RibbonManager::Heuristic)H, hr, K);
    for (auto& r : ribs) rm.add(r[0], r[1], r[2], r[3]);
    config.setMap(map);
    if (haveObst) config.setObstaclesManager(obst);
    if (haveGauss) config.setObstaclesManager(gauss);
    std::vector<std::shared_ptr<GpuContext>> contexts;
    try {
        if (!devices.empty()) contexts = GpuContext::shared(devices);     // an id that repeats: a further context (stream) on that device
        if (contexts.empty()) contexts.push_back(GpuContext::shared(0));
    } catch (const std::exception& e) {
        std::printf("{\"exception\": \"%s\"}\n", e.what());
        return 1;
    }
    if (shardedAttempts > 0) {
        try {
            ShardedIteration it(contexts);
            it.failShardForTest = failShard;
            ShardedIteration::Result r;
            std::vector<double> wall;
            for (int rep = 0; rep < repeat; rep++) {
                const auto w0 = std::chrono::steady_clock::now();
                r = it.run(rm, start, config, shardedSeed, shardedAttempts);
                wall.push_back(1e3 * std::chrono::duration<double>(std::chrono::steady_clock::now() - w0).count());
            }
            std::sort(wall.begin(), wall.end());
            std::printf("{\"sharded_batch\": %lld, \"shards\": %zu, \"rccl_ranks\": %d, \"agreed\": %s, \"best_f\": %.17g, \"best_f_bits\": %llu, \"best_edge\": %llu, "
                        "\"best_shard\": %d, \"edges\": %lld, \"wall_ms_median\": %.4f, \"kept\": [",
                        shardedAttempts, contexts.size(), r.rcclRanks, r.agreed ? "true" : "false", r.f, (unsigned long long)r.fBits, (unsigned long long)r.edge, r.shard,
                        (long long)r.edges, wall[wall.size() / 2]);
            for (size_t i = 0; i < r.kept.size(); i++) std::printf("%s%lld", i ? ", " : "", (long long)r.kept[i]);
            std::printf("]}\n");
            return 0;
        } catch (const std::exception& e) {
            std::printf("{\"exception\": \"%s\"}\n", e.what());
            return 1;
        }
    }
    if (evaluate) {
        try {
            if (candidates.empty()) candidates.push_back(prev);
            GpuAStarPlanner planner(contexts);
            const std::vector<GpuAStarPlanner::PlanEvaluation> ev = planner.evaluatePlans(rm, start, config, candidates);
            static const char* const why[] = {"?", "ran_out_of_legs", "infeasible", "goal", "throws", "capacity"};
            std::printf("{\"evaluations\": [");
            for (size_t i = 0; i < ev.size(); i++) {
                const GpuAStarPlanner::PlanEvaluation& e = ev[i];
                std::printf("%s{\"legs_costed\": %d, \"stop\": \"%s\", \"stop_code\": %d, \"goal\": %s, \"g\": %.17g, \"collision_penalty\": %.17g, "
                            "\"coverage_completed_time\": %.17g, \"ribbons_left\": %d, \"legs\": [", i ? ", " : "", e.legsCosted,
                            why[(int)e.stop >= 1 && (int)e.stop <= 5 ? (int)e.stop : 0], (int)e.stop, e.goalReached ? "true" : "false", e.g, e.collisionPenalty,
                            e.coverageCompletedTime, (int)e.ribbons.count());
                for (size_t k = 0; k < e.legs.size(); k++)
                    std::printf("%s{\"feasible\": %s, \"g\": %.17g, \"collision_penalty\": %.17g}", k ? ", " : "", e.legs[k].feasible ? "true" : "false", e.legs[k].g,
                                e.legs[k].collisionPenalty);
                std::printf("]%s%s", config.planContacts() ? contactKeys(e.contacts).c_str() : "", config.planClearance() ? clearanceKeys(e.clearance).c_str() : "");
                if (config.keepoutMargin() != 0) std::printf("%s", keepoutKeys(e.keepout).c_str());
                if (config.planReach()) std::printf("%s", reachKeys(e.reach).c_str());
                if (config.planWater()) std::printf("%s", waterKeys(e.water).c_str());
                if (config.planWater() && config.planWaterRoute()) std::printf("%s", waterRouteKeys(e.water).c_str());
                std::printf("}");
            }
            std::printf("]}\n");
            return 0;
        } catch (const std::exception& e) {
            std::printf("{\"exception\": \"%s\"}\n", e.what());
            return 1;
        }
    }
    try {
        Planner::Stats st;
        std::vector<double> wall;
        if (replans > 0) {
            // the 10 Hz loop of Executive::planLoop (executive.cpp:85-305) without ROS: plan, move the start replanStep seconds
            // along the returned plan, hand the plan back as previousPlan, repeat.  Real clock, fixed budget per cycle.
            double tNow = t0;
            State cur = start;
            unsigned long iters = 0, expanded = 0, failures = 0, samples = 0, deadlineStops = 0, edges = 0, trips = 0, gridUploads = 0;
            unsigned long failuresExplained = 0;       // failed plans whose start state was in collision (an obstacle's box or a blocked cell)
            unsigned long nodeRegrowths = 0, deviceGrowths = 0, late = 0;
            long firstGoalSum = 0, firstGoalCount = 0, firstGoalMax = -1;
            std::vector<long> firstGoals;
            std::vector<int> failedCycles;
            double insidePlanMs = 0;                   // plan() wall time over the cycles after the first
            Planner::Stats::BudgetTrace worst;         // the budget trace of the slowest cycle after the first
            int worstCycle = -1;
            double worstMs = 0;
            int failureCount = 0, horizonHalvings = 0;  // Executive::planLoop's back-off (executive.cpp:263-277)
            FILE* cycleLog = cycleLogPath.empty() ? nullptr : std::fopen(cycleLogPath.c_str(), "w");
            FILE* planLog = planLogPath.empty() ? nullptr : std::fopen(planLogPath.c_str(), "w");
            if (replanClockCalls > 0) { timeRemaining = (double)replanClockCalls * dt; config.setDeadlineGuard(false); }
            for (int cyc = 0; cyc < replans; cyc++) {
                const auto w0 = std::chrono::steady_clock::now();
                long calls = 0;
                if (replanClockCalls > 0) config.setNowFunction([&]() { return tNow + (double)(calls++) * dt; });
                else config.setNowFunction([&]() { return tNow + std::chrono::duration<double>(std::chrono::steady_clock::now() - w0).count(); });
                GpuAStarPlanner planner(contexts);
                st = planner.plan(rm, cur, config, prev, timeRemaining);
                wall.push_back(1e3 * std::chrono::duration<double>(std::chrono::steady_clock::now() - w0).count());
                iters += st.Iterations; expanded += st.Expanded; samples += st.Samples; deadlineStops += st.DeadlineStops; edges += st.EdgesCosted;
                trips += st.Budget.RoundTrips; gridUploads += st.Budget.GridUploaded ? 1 : 0;
                nodeRegrowths += st.Budget.NodeRegrowths; deviceGrowths += st.Budget.DeviceGrowths;
                if (st.FirstGoalIteration >= 0) { firstGoalSum += st.FirstGoalIteration; firstGoalCount++; firstGoalMax = std::max(firstGoalMax, st.FirstGoalIteration); }
                firstGoals.push_back(st.FirstGoalIteration);
                const bool startHit = config.obstaclesManager().collisionExists(cur, true) > 0 || (config.map() && config.map()->isBlocked(cur.x(), cur.y()));
                if (cyc > 0) {
                    insidePlanMs += wall.back();
                    if (wall.back() >= 1e3 * timeRemaining) late++;
                    if (wall.back() > worstMs) { worstMs = wall.back(); worst = st.Budget; worstCycle = cyc; }
                }
                const Planner::Stats::BudgetTrace& b = st.Budget;
                if (cycleLog)
                    std::fprintf(cycleLog, "{\"cycle\": %d, \"wall_ms\": %.3f, \"iterations\": %lu, \"first_goal_iteration\": %ld, \"samples\": %lu, \"expanded\": %lu, "
                                 "\"edges\": %lu, \"round_trips\": %lu, \"deadline_stops\": %lu, \"plan_empty\": %s, \"start_in_collision\": %s, \"prologue_ms\": %.3f, "
                                 "\"loop_end_ms\": %.3f, \"total_ms\": %.3f, \"last_op\": %d, \"last_op_start_ms\": %.3f, \"last_op_predicted_ms\": %.3f, "
                                 "\"last_op_actual_ms\": %.3f, \"margin_ms\": %.3f, \"max_trip_ms\": %.3f, \"worst_under_prediction_ms\": %.3f, \"node_regrowths\": %lu, "
                                 "\"node_regrowth_ms\": %.3f, \"device_growths\": %lu, \"device_growth_ms\": %.3f, \"grid_uploaded\": %s, \"pick_ms\": %.3f, \"max_pick_ms\": %.3f, "
                                 "\"order_fallbacks\": %lu, \"max_wake_ms\": %.3f, \"stride_retries\": %lu}\n",
                                 cyc, wall.back(), (unsigned long)st.Iterations, st.FirstGoalIteration, (unsigned long)st.Samples, (unsigned long)st.Expanded,
                                 (unsigned long)st.EdgesCosted, b.RoundTrips, (unsigned long)st.DeadlineStops, st.Plan.empty() ? "true" : "false", startHit ? "true" : "false",
                                 b.PrologueMs, b.LoopEndMs, b.TotalMs, b.LastOpKind, b.LastOpStartMs, b.LastOpPredictedMs, b.LastOpActualMs, b.MarginMs, b.MaxTripMs,
                                 b.WorstUnderPredictionMs, b.NodeRegrowths, b.NodeRegrowthMs, b.DeviceGrowths, b.DeviceGrowthMs, b.GridUploaded ? "true" : "false", b.PickMs, b.MaxPickMs,
                                 (unsigned long)st.OrderFallbacks, b.MaxWakeMs, b.StrideRetries);
                if (cyc > 0 && wall.back() >= 1e3 * timeRemaining)      // late: what was the cycle doing when the budget ran out?
                    std::fprintf(stderr, "[replan] cycle %d LATE: %.3f ms of %.1f | loop left at %.3f, last op kind %d started %.3f predicted %.3f took %.3f (margin %.3f) | "
                                 "max trip %.3f, worst under-prediction %.3f | node regrowths %lu (%.3f ms), device growths %lu (%.3f ms), prologue %.3f | picks %.3f ms (longest %.3f), "
                                 "%lu order fallbacks, longest thread wake %.3f | %lu iterations, %lu samples, %lu expanded\n",
                                 cyc, wall.back(), 1e3 * timeRemaining, b.LoopEndMs, b.LastOpKind, b.LastOpStartMs, b.LastOpPredictedMs, b.LastOpActualMs, b.MarginMs, b.MaxTripMs,
                                 b.WorstUnderPredictionMs, b.NodeRegrowths, b.NodeRegrowthMs, b.DeviceGrowths, b.DeviceGrowthMs, b.PrologueMs, b.PickMs, b.MaxPickMs,
                                 (unsigned long)st.OrderFallbacks, b.MaxWakeMs, (unsigned long)st.Iterations, (unsigned long)st.Samples, (unsigned long)st.Expanded);
                if (planLog) {
                    std::fprintf(planLog, "{\"cycle\": %d, \"expanded\": %lu, \"generated\": %lu, \"edges\": %lu, \"iterations\": %lu, \"first_goal_iteration\": %ld, "
                                 "\"round_trips\": %lu, \"prologue_trips\": %lu, \"prologue_ms\": %.3f, \"previous_plan_legs\": %zu, \"plan\": [", cyc, (unsigned long)st.Expanded,
                                 (unsigned long)st.Generated, (unsigned long)st.EdgesCosted, (unsigned long)st.Iterations, st.FirstGoalIteration, b.RoundTrips + b.PrologueTrips,
                                 b.PrologueTrips, b.PrologueMs, st.PreviousPlanLegs.size());
                    bool firstSeg = true;
                    for (const auto& w : st.Plan.get()) {
                        const DubinsPath& p = w.unwrap();
                        std::fprintf(planLog, "%s[%.17g, %.17g, %.17g, %.17g, %.17g, %.17g, %.17g, %d, %.17g, %.17g, %.17g]", firstSeg ? "" : ", ", p.qi[0], p.qi[1], p.qi[2],
                                     p.param[0], p.param[1], p.param[2], p.rho, (int)p.type, w.getSpeed(), w.getStartTime(), w.getEndTime());
                        firstSeg = false;
                    }
                    std::fprintf(planLog, "]}\n");
                }
                tNow += replanStep;
                if (st.Plan.empty()) {
                    failures++; failedCycles.push_back(cyc);
                    if (startHit) failuresExplained++;
                    // executive.cpp:263-277: the third empty plan in a row halves the time horizon (never below timeMinimum, never restored)
                    failureCount++;
                    if (failureCount > 2) {
                        config.setTimeHorizon(config.timeHorizon() / 2);
                        if (config.timeHorizon() < config.timeMinimum()) config.setTimeHorizon(config.timeMinimum());
                        else { failureCount = 0; horizonHalvings++; }
                    }
                    cur.time() = tNow; prev = DubinsPlan(); continue;
                }
                failureCount = 0;                       // executive.cpp:220
                prev = st.Plan;
                State nxt; nxt.time() = tNow;
                if (prev.containsTime(tNow)) { prev.sample(nxt); cur = nxt; } else { cur.time() = tNow; }
                cur.speed() = config.maxSpeed();
                rm.cover(cur.x(), cur.y(), false);      // Executive::updateCovered: the vehicle covers as it moves
            }
            if (cycleLog) std::fclose(cycleLog);
            if (planLog) std::fclose(planLog);
            // the first cycle of a process allocates the device buffers (they persist in the contexts): reported on its own,
            // the percentiles are over the cycles after it
            const double firstCycle = wall.front();
            if (wall.size() > 1) wall.erase(wall.begin());
            std::sort(wall.begin(), wall.end());
            const double p50 = wall[wall.size() / 2], p99 = wall[std::min(wall.size() - 1, (size_t)(0.99 * wall.size()))];
            std::vector<long> fg = firstGoals;
            std::sort(fg.begin(), fg.end());
            std::printf("{\"replans\": %d, \"budget_ms\": %.3f, \"first_cycle_ms\": %.3f, \"wall_ms_p50\": %.3f, \"wall_ms_p99\": %.3f, \"wall_ms_max\": %.3f, "
                        "\"late_cycles\": %lu, \"mean_iterations\": %.2f, \"mean_expanded\": %.1f, \"mean_samples\": %.1f, \"mean_edges\": %.1f, \"mean_round_trips\": %.1f, "
                        "\"first_goal_iteration_median\": %ld, \"first_goal_iteration_max\": %ld, \"first_goal_iteration_mean\": %.3f, \"cycles_with_a_goal\": %ld, "
                        "\"failed_plans\": %lu, \"failed_plans_with_start_in_collision\": %lu, \"horizon_halvings\": %d, \"final_time_horizon\": %.3f, \"deadline_stops\": %lu, \"grid_uploads\": %lu, "
                        "\"node_regrowths\": %lu, \"device_growths\": %lu, \"expansions_per_s_inside_plan\": %.1f, \"edges_per_s_inside_plan\": %.1f, "
                        "\"worst_cycle\": {\"cycle\": %d, \"wall_ms\": %.3f, \"loop_end_ms\": %.3f, \"last_op\": %d, \"last_op_start_ms\": %.3f, \"last_op_predicted_ms\": %.3f, "
                        "\"last_op_actual_ms\": %.3f, \"margin_ms\": %.3f, \"max_trip_ms\": %.3f, \"node_regrowths\": %lu, \"node_regrowth_ms\": %.3f, \"device_growths\": %lu, "
                        "\"device_growth_ms\": %.3f, \"prologue_ms\": %.3f}, \"failed_cycles\": [",
                        replans, 1e3 * timeRemaining, firstCycle, p50, p99, wall.back(), late, (double)iters / replans, (double)expanded / replans,
                        (double)samples / replans, (double)edges / replans, (double)trips / replans, fg[fg.size() / 2], firstGoalMax,
                        firstGoalCount ? (double)firstGoalSum / firstGoalCount : -1.0, firstGoalCount, failures, failuresExplained, horizonHalvings, config.timeHorizon(), deadlineStops, gridUploads,
                        nodeRegrowths, deviceGrowths, insidePlanMs > 0 ? 1e3 * (double)expanded / insidePlanMs : 0.0, insidePlanMs > 0 ? 1e3 * (double)edges / insidePlanMs : 0.0,
                        worstCycle, worstMs, worst.LoopEndMs, worst.LastOpKind, worst.LastOpStartMs, worst.LastOpPredictedMs, worst.LastOpActualMs, worst.MarginMs,
                        worst.MaxTripMs, worst.NodeRegrowths, worst.NodeRegrowthMs, worst.DeviceGrowths, worst.DeviceGrowthMs, worst.PrologueMs);
            for (size_t i = 0; i < failedCycles.size(); i++) std::printf("%s%d", i ? ", " : "", failedCycles[i]);
            std::printf("], \"devices\": %zu}\n", contexts.size());
            return 0;
        }
        for (int rep = 0; rep < repeat; rep++) {
            long calls = 0;
            const auto w0 = std::chrono::steady_clock::now();
            if (realClock)
                config.setNowFunction([&]() { return t0 + std::chrono::duration<double>(std::chrono::steady_clock::now() - w0).count(); });
            else
                config.setNowFunction([&]() { return t0 + (double)(calls++) * dt; });
            config.setDeadlineGuard(realClock);   // a counting clock does not advance while the device works
            GpuAStarPlanner planner(contexts);   // a fresh planner every cycle, like Executive::planLoop (executive.cpp:85-90)
            st = planner.plan(rm, start, config, prev, timeRemaining);
            wall.push_back(1e3 * std::chrono::duration<double>(std::chrono::steady_clock::now() - w0).count());
        }
        std::sort(wall.begin(), wall.end());
        std::fprintf(stderr, "plan() wall ms: min %.3f median %.3f max %.3f over %d calls\n", wall.front(), wall[wall.size() / 2], wall.back(), repeat);
        std::printf("{\"samples\": %lu, \"generated\": %lu, \"expanded\": %lu, \"iterations\": %lu, \"plan_f\": %.17g, "
                    "\"plan_collision_penalty\": %.17g, \"plan_time_penalty\": %.17g, \"plan_h\": %.17g, \"plan_depth\": %lu, "
                    "\"first_goal_iteration\": %ld, \"edges_costed\": %lu, \"host_heuristics\": %lu, \"order_fallbacks\": %lu, \"wall_ms_median\": %.4f, "
                    "\"wall_ms_max\": %.4f, \"plan\": [",
                    st.Samples, st.Generated, st.Expanded, st.Iterations, st.PlanFValue, st.PlanCollisionPenalty, st.PlanTimePenalty,
                    st.PlanHValue, st.PlanDepth, st.FirstGoalIteration, st.EdgesCosted, st.HostHeuristics, st.OrderFallbacks, wall[wall.size() / 2], wall.back());
        bool first = true;
        for (const auto& w : st.Plan.get()) {
            const DubinsPath& p = w.unwrap();
            std::printf("%s[%.17g, %.17g, %.17g, %.17g, %.17g, %.17g, %.17g, %d, %.17g, %.17g, %.17g]", first ? "" : ", ", p.qi[0], p.qi[1],
                        p.qi[2], p.param[0], p.param[1], p.param[2], p.rho, (int)p.type, w.getSpeed(), w.getStartTime(), w.getEndTime());
            first = false;
        }
        std::string tail;                     // (only when the scenario names the switch: without it the line is what it always was)
        if (chainNamed) {
            char buf[256];
            std::snprintf(buf, sizeof buf, ", \"round_trips\": %lu, \"prologue_trips\": %lu, \"prologue_ms\": %.3f, \"previous_plan_legs\": [",
                          st.Budget.RoundTrips + st.Budget.PrologueTrips, st.Budget.PrologueTrips, st.Budget.PrologueMs);
            tail = buf;
            for (size_t i = 0; i < st.PreviousPlanLegs.size(); i++) {
                std::snprintf(buf, sizeof buf, "%s{\"g\": %.17g, \"collision_penalty\": %.17g, \"infeasible\": %s}", i ? ", " : "", st.PreviousPlanLegs[i].g,
                              st.PreviousPlanLegs[i].collisionPenalty, st.PreviousPlanLegs[i].infeasible ? "true" : "false");
                tail += buf;
            }
            tail += "]";
        }
        if (tableNamed) {
            char buf[96];
            std::snprintf(buf, sizeof buf, ", \"table_heuristics\": %lu, \"table_refused\": %lu", st.TableHeuristics, st.TableRefused);
            tail += buf;
        }
        if (config.planCoverage()) {              // (only with the switch on: without it the line is what it always was)
            size_t nSteps = 0;
            for (const auto& seg : st.Coverage) nSteps += seg.size();
            char buf[64];
            std::snprintf(buf, sizeof buf, ", \"plan_coverage_steps\": %zu", nSteps);
            tail += buf;
            if (!writeReport(planCoveragePath, st.Coverage.size(), [&](FILE* f, size_t sg) {
                    for (const auto& c : st.Coverage[sg])
                        std::fprintf(f, "%zu %u %.17g %.17g %.17g %u %u\n", sg, c.step, c.time, c.toCover, c.remaining, c.ribbons, c.flags);
                })) return 2;
        }
        if (config.planContacts()) {              // (only with the switch on: without it the line is what it always was)
            tail += contactKeys(st.PlanContacts);
            if (!writeReport(planContactsPath, st.Contacts.size(), [&](FILE* f, size_t sg) {
                    for (const auto& c : st.Contacts[sg])
                        std::fprintf(f, "%zu %u %d %.17g %.17g %.17g %.17g %.17g %.17g\n", sg, c.mmsi, c.hitSteps, c.firstHitTime, c.lastHitTime, c.cpaDistance, c.cpaTime,
                                     c.exposure, c.peak);
                })) return 2;
        }
        if (config.planClearance()) {             // (only with the switch on: without it the line is what it always was)
            tail += clearanceKeys(st.PlanClearance);
            if (!writeReport(planClearancePath, st.Clearance.size(), [&](FILE* f, size_t sg) {
                    const auto& c = st.Clearance[sg];
                    std::fprintf(f, "%zu %.17g %.17g %.17g %.17g %d %u %d %.17g %u\n", sg, c.clearance, c.time, c.x, c.y, c.step, c.gap2, c.belowSteps, c.firstBelowTime, c.flags);
                })) return 2;
        }
        if (config.keepoutMargin() != 0) tail += keepoutKeys(st.Keepout);      // (only with a margin named: without it the line is what it always was)
        if (config.planReach()) {                 // (only with the switch on: without it the line is what it always was)
            tail += reachKeys(st.Reach);
            if (!writeReport(planReachPath, st.Reach.Ribbons.size(), [&](FILE* f, size_t rb) {
                    const auto& r = st.Reach.Ribbons[rb];
                    std::fprintf(f, "%zu %.17g %.17g %u %u %d %d %u %u %u %.17g %u\n", rb, r.length, r.pitch, r.samples, r.outSamples, r.firstOut, r.lastOut, r.minRgap2,
                                 r.maxRgap2, r.lim2, r.outLength, r.flags);
                })) return 2;
        }
        if (config.planWater()) {                 // (likewise)
            tail += waterKeys(st.Water);
            if (!writeReport(planWaterPath, st.Water.Ribbons.size(), [&](FILE* f, size_t rb) {
                    const auto& r = st.Water.Ribbons[rb];
                    std::fprintf(f, "%zu %.17g %.17g %u %u %d %d %u %u %u %u %u %u %.17g\n", rb, r.length, r.pitch, r.samples, r.wetSamples, r.nearestSample,
                                 r.farthestSample, r.minAd, r.maxAd, r.startAd, r.endAd, r.lim2, r.flags, r.nearestMetres);
                })) return 2;
            if (config.planWaterRoute()) {
                tail += waterRouteKeys(st.Water);
                if (!writeReport(planWaterRoutePath, st.Water.Routes.size(), [&](FILE* f, size_t rb) {
                        const auto& vs = st.Water.Routes[rb].Vertices;
                        for (size_t j = 0; j < vs.size(); j++) std::fprintf(f, "%zu %zu %.17g %.17g\n", rb, j, vs[j].first, vs[j].second);
                    })) return 2;
            }
        }
        if (config.planTrace()) {
            size_t nSteps = 0;
            for (const auto& seg : st.Trace) nSteps += seg.size();
            std::printf("], \"plan_trace_segments\": %zu, \"plan_trace_steps\": %zu%s}\n", st.Trace.size(), nSteps, tail.c_str());
            if (!writeReport(planTracePath, st.Trace.size(), [&](FILE* f, size_t sg) {
                    for (const auto& t : st.Trace[sg])
                        std::fprintf(f, "%zu %u %.17g %.17g %.17g %.17g %.17g %.17g %u\n", sg, t.step, t.x, t.y, t.heading, t.time, t.collision, t.penaltyBefore, t.flags);
                })) return 2;
        } else {
            std::printf("]%s}\n", tail.c_str());
        }
    } catch (const std::exception& e) {
        std::printf("{\"exception\": \"%s\"}\n", e.what());
        return 1;
    }
    return 0;
}
