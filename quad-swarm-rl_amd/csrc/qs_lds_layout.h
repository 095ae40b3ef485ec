// qs_lds_layout.h - the dynamic-LDS layout of a step / reset workgroup (LdsLayout) and the one host function that lays it out: whether
// a workgroup fits a CU, a literal of every config-specialised object, half of its cache key.  Plain C++17 without HIP, like
// qs_env_plan.h: tests/test_lds_layout.py compiles it alone.  Included by qs_obs_rows.h for the device code, which only reads the struct.
#pragma once
#include <cstring>
#include "../../include/quadswarm.h"
#include "qs_scen_slots.h"

struct LdsLayout { int off_mask, off_omap, off_si, off_sr, off_envflag, off_scratch, off_pos, off_vel, off_zax, off_om, off_goal,
    off_obst, off_metric, off_obs, goal_rows, total;
                   int off_t_rot, off_t_goal, off_t_prox, off_t_col, off_t_dw, off_t_ohit;
                   // team kernels: the step's 17 reward terms + the done flag, for the wave that keeps the episode sums
                   int off_t_ri;
                   // team kernels, N > 8 (pair-once scan): proximity masks, per-wave top-8 lists, per-env "velocities changed" flags
                   int off_t_near, off_topk, off_t_redo;
                   int off_self, off_rows, rows_per_pass, scr_cap;   // single-wave kernels: observation output (see obs_copy_rows)
                   int off_cur; };   // QS_TAPE kernels: per-env tape cursor
// neighbour + SDF columns a lane can keep in registers between the row passes (K <= 8)   // single-wave kernels: observation columns staged
// per pass (see obs_flush)
#define QS_NV_MAX 57
#define QS_RESET_SCRATCH_INTS 160   // per env, full scenario set: virtual-pool index/value lists (2x64) + two DP rows (2x16)

// Observation rows leave through LDS so that they reach HBM as whole, aligned cache lines (a first version wrote column
// groups straight from a small stage: 72-byte runs at a 216-byte stride cost more than the rest of the step - see
// profiles/r02_exp_colgroup_flush.txt).  Team kernels (small batches, occupancy irrelevant) stage the workgroup's complete
// rows [64][D].  Single-wave (throughput) kernels keep the self columns in a dense block [64][S] (written early, read by
// the bookkeeping) and pass the other D-S columns through a stage of `rows_per_pass` rows: each lane holds its neighbour / SDF
// values in registers, the lanes of one row group store them, the whole wave copies that group's complete rows
// (rows_per_pass * D * 4 contiguous bytes) out, next group.  The stage shares its LDS with the buffers of the rare paths
// (collision responses, goal scratch rows, reset scratch), none of which is live while rows are being copied: a workgroup
// needs ~9.5 KB instead of ~21 KB, and 16 of them fit a CU.
inline LdsLayout lds_layout(int real_size, int B, int N, int epb, int obs_dim, int num_obst, int K, int team /* waves per workgroup of the team kernels, 0 = single-wave */,
                            bool full /* kernels of the full scenario set: per-env scenario state in LDS */,
                            bool tape /* the noise-tape kernels (qs_tape_kernels.hip): a tape cursor per env */, int scenario = -1, int rows_per_pass = 64) {
    LdsLayout L;
    memset(&L, 0, sizeof L);
    const int self_dim = obs_dim - 6 * K - (num_obst > 0 ? 9 : 0), extra = obs_dim - self_dim;
    // goal scratch rows per env: two formations (+ sphere padding) for swarm_vs_swarm and the full scenario set, one otherwise
    L.goal_rows = (full || scenario < 0 || scenario == QS_SCENARIO_SWARM_VS_SWARM) ? 2 * N + 8 : (N < 3 ? 3 : N);
    // reset scratch per env: virtual-pool index / value lists (2 x cap: at most one entry per obstacle / per drone) + two DP rows
    // (2 x 16); the full scenario set keeps the fixed 2 x 64 split its scenario code addresses
    L.scr_cap = full ? 64 : (num_obst > N ? num_obst : N);
    const int goal_bytes = real_size * 3 * L.goal_rows * epb, scratch_bytes = num_obst > 0 ? 4 * (2 * L.scr_cap + 32) * epb : 0;
    int o = 0;
    L.off_omap = o; o += full ? 8 * 4 * epb : 0;      // full-scenario kernels: obstacle map bitset, scenario ints / reals per env
    L.off_si = o; o += full ? 4 * qs::SI_COUNT * epb : 0;
    L.off_sr = o; o += full ? real_size * qs::SR_COUNT * epb : 0;
    o = (o + 15) & ~15;
    // [epb] have-spawn-points flags + [epb] swarm_vs_swarm periods + [epb] obstacle-size choice
    L.off_envflag = o; o += 4 * ((3 * epb + 3) & ~3);
    if (tape) { L.off_cur = o; o += 4 * ((epb + 3) & ~3); }
    o = (o + 15) & ~15;
    L.off_pos = o; o += real_size * 3 * B;
    L.off_vel = o; o += real_size * 3 * B;
    L.off_zax = o; o += real_size * 3 * B;            // body z axes (downwash); spawn points in the reset tail
    L.off_obst = o; o += real_size * 2 * (num_obst > 0 ? num_obst : 1) * epb;   // obstacle xy of the block's envs
    // neighbour metric rows [N][B]; team kernels with N > 8 reserve at least (real_size + 4) * 8 * team * B bytes: the room of the
    // round-2 ranking's lists, which no kernel uses any more - the bytes beyond the [N][B] rows are unused (kept: L.total is a literal
    // of every N > 8 object and half of its cache key)
    L.off_metric = o; o += ((team ? K > 0 : K > 8) && K < N - 1)
        ? ((team && N > 8) ? ((real_size + 4) * 8 * team > real_size * N
        ? (real_size + 4) * 8 * team : real_size * N) * B : real_size * N * B) : 0;
    o = (o + 15) & ~15;
    if (team) {
        L.off_mask = o; o += 8 * B;                   // u64 per lane: new-pair masks for the serial response path
        L.off_om = o; o += real_size * 3 * B;
        L.off_goal = o; o += goal_bytes;
        L.off_scratch = o; o += scratch_bytes;
        o = (o + 15) & ~15;
        L.off_t_col = o; o += 8 * B;                  // exchange rows of the team kernels
        L.off_t_dw = o; o += 8 * B;
        L.off_t_rot = o; o += real_size * 6 * B;
        L.off_t_goal = o; o += real_size * 3 * B;
        L.off_t_prox = o; o += real_size * (team - 1) * B;
        L.off_t_ohit = o; o += 4 * B;
        L.off_t_near = o; o += 8 * B;
        L.off_t_ri = o; o += real_size * (QS_RI_COUNT + 1) * B;
        L.off_t_redo = o; o += 4 * ((epb + 3) & ~3);
        o = (o + 15) & ~15;
        // N > 8 with K <= 8: every ranking wave (all but wave 0) publishes the top-8 of its candidates, compacted by local rank:
        // float32: one 64-bit (metric, index) key per entry; float64: metric + index
        L.off_topk = o; o += (N > 8 && K > 0 && K < N - 1 && K <= 8) ? (team - 1) * 8 * (real_size + 4) * B : 0;
        o = (o + 15) & ~15;
        L.rows_per_pass = B;
        L.off_obs = o; L.off_self = o; L.off_rows = o + real_size * self_dim * B;   // complete rows [B][D]; the reset kernel sees them as
        o += real_size * obs_dim * B;                                                // the self block followed by the rows stage
    } else {
        L.rows_per_pass = rows_per_pass < 1 ? 1 : (rows_per_pass > B ? B : rows_per_pass);
        L.off_self = o; L.off_obs = o; o += real_size * self_dim * B;
        o = (o + 15) & ~15;
        // the rows stage and, in the same bytes, what only the rare paths touch: (a) collision responses: pair masks + angular
        // velocities, (b) scenario goal switch / reset: goal scratch rows + reset scratch
        const int stage_bytes = real_size * extra * L.rows_per_pass, rare_a = 8 * B + real_size * 3 * B,
            rare_b = goal_bytes + scratch_bytes;
        int u = stage_bytes > rare_a ? stage_bytes : rare_a;
        u = u > rare_b ? u : rare_b;
        L.off_rows = o; L.off_mask = o; L.off_om = o + 8 * B; L.off_goal = o; L.off_scratch = o + goal_bytes;
        o += u;
    }
    L.total = (o + 15) & ~15;
    return L;
}
