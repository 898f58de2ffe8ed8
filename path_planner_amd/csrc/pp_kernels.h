// pp_kernels.h — the gfx950 kernels of the hot path, one header per stage of the path.  Included once by ppgpu.hip.
#pragma once
#include "../../include/ppgpu.h"
#include "pp_device.h"
#include "pp_k_common.h"       // PPParams, PPEdgeSetup, clearance map, time grids, edge decoding, work queues
#include "pp_k_solve.h"        // pp_k_solve_edges
#include "pp_k_sweep.h"        // pp_k_plan_skips, pp_k_pose_sweep
#include "pp_k_heuristic.h"    // pp_k_heuristic*, pp_k_deferred_list
#include "pp_k_finish.h"       // phase C of an edge: the pieces every route shares, pp_lane_phase_c, pp_k_cover_finish
#include "pp_k_cover.h"        // pp_k_approach_events, pp_k_cover_sweep
#include "pp_k_trace_common.h"  // what the traces share: edge head, window walk, record store
#include "pp_k_trace.h"        // pp_k_trace_steps
#include "pp_k_cover_trace.h"  // pp_k_trace_cover
#include "pp_k_contact_trace.h"  // pp_k_trace_contacts
#include "pp_k_distance.h"     // pp_k_dist_cols, pp_k_dist_rows, pp_k_grid_clearance_at: the distance map behind the chart clearance
#include "pp_k_clearance_trace.h"  // pp_k_trace_clearance
#include "pp_k_keepout.h"      // pp_k_keepout_bits: the distance map thresholded into the effective grid of a keep-out margin
#include "pp_k_reach.h"        // pp_k_reach_tiles / _merge / _flatten, pp_k_reach_bits, pp_k_reach_ribbons: which water a seed can reach
#include "pp_k_water.h"        // pp_k_water_seed / _round / _totals, pp_k_water_distance_at, pp_k_water_ribbons: how far it is by water from a seed
#include "pp_k_route.h"        // pp_k_water_dirs, pp_k_water_routes: which way the distance by water goes, per query point
#include "pp_k_chain.h"        // pp_k_chain_advance
#include "pp_k_tsp_table.h"    // pp_k_tsp_table_list, pp_k_tsp_table
#include "pp_k_expand.h"       // pp_k_dubins_lengths, pp_k_select_nearest, the push-order pipeline, the round trip's pack / unpack
#include "pp_k_incumbent.h"    // pp_k_best_stage1/2, pp_k_key_min_n
