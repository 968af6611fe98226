// Host side only: the process-wide switches of the appearance and density backward, and what the two shape-dependent
// launchers decide from them.  A launcher asks knobs() once, hands the record to a PURE plan function (no HIP call, no getenv,
// no static state: plan_shade_bwd<C> in jt_shade.hip, plan_march_bwd in jt_march.hip) and executes the plan it gets back; the
// queries jt_shade_backward_plan / jt_march_backward_plan report the same plan without a device.
#pragma once
#include "jt_common.h"

#ifndef JT_SCATTER_CLAIM_DEFAULT
#define JT_SCATTER_CLAIM_DEFAULT 1
#endif

namespace jt {

// Every switch, read ONCE per process (the environment) or set through the library's setters.  DESIGN.md section 3 has the
// table: values, defaults, what each selects and which bench.py extra uses it.
struct Knobs {
  // setter-backed (the environment variable gives the initial value)
  int matrix_mode;    // JT_BF16X3 / jt_shade_set_matrix_mode: 0..7, default JT_BF16X3_DEFAULT
  int split;          // JT_BWD_SPLIT / jt_shade_set_bwd_split: -1 (per scene kind), 0, 1, 8, 16
  int lean;           // JT_LEAN_TAPE / jt_shade_set_lean_tape: 0 / 1, default 1
  int chunk_log2;     // JT_SHADE_CHUNK_LOG2 / jt_shade_set_chunk_log2: 16..22, default 22
  // environment only
  int scatter_wgs;    // JT_SCATTER_WGS: workgroups of k_shade_scatter, 0 = chosen by the plan
  int scatter_waves;  // JT_SCATTER_WAVES: 8 / 12 / 16 waves per scatter workgroup, 0 = chosen by the plan
  int scatter_flags;  // JT_SCATTER_FLAGS: bit 0 line gradients through LDS, default 1
  int scatter_first;  // JT_SCATTER_FIRST: the scatter in front of the fork, default 0
  int scatter_claim;  // JT_SCATTER_CLAIM: 0 a fixed stride per wave, 1 the twelve-wave scatter's waves draw their batches
  int wgrad_pipe;     // JT_WGRAD_PIPE: the GEMMs of chunk c forked behind the chain of chunk c, default 1
  int ablate;         // JT_ABLATE (profiling): 1 no scatter, 2 no gradient records, 4 no weight-gradient GEMMs
  int pose_bwd;       // JT_POSE_BWD: the walker-free pose-only kernels of both backwards, default 1
  int tile_wgs;       // JT_TILE_WGS: workgroups of the tile-owned scatter (>= 6), 0 = one per CU
  int tile_ratio;     // JT_TILE_RATIO: per cent of a plane's workgroups for the first of two channel classes, default 62
  int walk_lds_line;  // JT_WALK_LDS_LINE: 0 no LDS line, 1 floats, 2 doubles, -1 = chosen by the plan
  int walk_waves;     // JT_WALK_WAVES: 8 / 16 waves per walk workgroup, 0 = chosen by the plan
  int walk_wgs;       // JT_WALK_WGS: fewer walk workgroups (a multiple of three), 0 = all
};
Knobs knobs();  // the one reader (jt_shade.hip): the environment, read once, under whatever the setters have stored since

constexpr int kLdsBudget = 160 * 1024;  // bytes of LDS a workgroup of this library may ask for

// ---- appearance backward (plan_shade_bwd<C>, jt_shade.hip) ---------------------------------------------------------------------
struct ShadeBwdInputs {
  int line_len[3], plane_h[3], plane_w[3];
  bool det;                  // deterministic mode
  bool want_factor_grads;    // g_factors given
  bool want_mlp_grads;       // g_mlp given
  int flags;                 // the caller's JT_SHADE_* flags
  bool have_aux;             // auxiliary stream and both events given
};
enum ShadeChain { kChainFused = 0, kChainFusedDet = 1, kChainSplit = 2, kChainSplitB16 = 3 };
enum ShadeSecond { kSecondNone = 0, kSecondScatter = 1, kSecondTile = 2, kSecondPoseGather = 3, kSecondPoseGatherB16 = 4 };
struct ShadeBwdPlan {
  int status;                // JT_OK, or why this scene cannot run
  int split_requested;       // the split mode with -1 resolved (what the tape and the caller's stream choice follow)
  int split;                 // the split that runs: after the tile fallback, the pose-only override, the twelve-wave choice
  int chain;                 // ShadeChain
  int chain_lds;             // its dynamic LDS bytes
  int second;                // ShadeSecond
  bool sc_det;               // k_shade_scatter<C, DET, RUN, WAVES, FLAGS> (second == kSecondScatter)
  int sc_run, sc_waves, sc_flags;
  int sc_lds;                // its dynamic LDS bytes
  int sc_wgs;                // its workgroups at most, and the slab count k_dbasis_reduce sums
  bool lean;                 // the tape the forward left: no product rows
  int rec_rows;              // rows of a tile's record block
  bool dbasis_in_scatter;
  bool gemm_b16;             // the weight-gradient GEMMs on the bf16 matrix cores
  int gemm_count;            // GEMMs per chunk: 0 (none wanted), 3 (dBasis out of the scatter) or 4
  bool gemm_forked;          // on the auxiliary stream
  // how the launcher runs it (not part of the query)
  int ablate;                // the kernels' `ablate` argument
  bool pose_only, gemm_pipe, scatter_first;
  int line_floats, tile_line_len, tile_wgs, tile_ratio;
};

// ---- density backward (plan_march_bwd, jt_march.hip) ---------------------------------------------------------------------------
struct MarchBwdPlan {
  int status;
  int scan;                  // k_march_bwd_scan<scan>: 0 training form, 1 pose-only, 2 pose-only with stored derivatives
  int scan_lds;
  bool walk;                 // k_march_bwd_walk<cd, det, line_mode, waves> runs behind the scan
  int cd;                    // density channels
  bool det;                  // deterministic mode: fixed-point sums, no LDS line
  int runs;                  // runs per (ray, plane), a multiple of four
  int line_mode;             // 0 no LDS line, 1 a float copy, 2 a copy of doubles
  int waves;                 // 8 / 16 per workgroup
  int prefix;                // the prefix table of the rays' item counts is kept in LDS
  int lds;                   // dynamic LDS bytes of the walk
  int wgs;                   // its workgroups
};

}  // namespace jt
