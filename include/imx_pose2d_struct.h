#ifndef IMX_POSE2D_STRUCT_H_
#define IMX_POSE2D_STRUCT_H_
/* imx_pose2d_command_t: the pose-2d command term (isaaclab/envs/mdp/commands/pose_2d_command.py: UniformPose2dCommand :26-143,
 * TerrainBasedPose2dCommand :146-203) as imx_pose2d_command and imx_reset_orchestrate_pose2d (imx.h, where the entry points are) take
 * it.  A header of its own, included by imx.h, like imx_orch_manip.h; it can be included alone. */
#include <stdint.h>

typedef struct imx_pose2d_command {
    int32_t kind;                      /* 0 UniformPose2dCommand, 1 TerrainBasedPose2dCommand */
    int32_t simple_heading;            /* cfg.simple_heading: the heading points at the target (or away from it, whichever is closer) */
    float cfg[8];                      /* resampling_time_range lo, hi; ranges.pos_x lo, hi; ranges.pos_y lo, hi; ranges.heading lo, hi */
    const float* env_origins_d;        /* (N,3) scene.env_origins (kind 0) */
    const float* default_root_z_d;     /* (N) robot.data.default_root_state[:, 2] */
    const float* valid_targets_d;      /* (L,T,P,3) terrain.flat_patches["target"] (kind 1) */
    const int64_t* terrain_levels_d;   /* (N) terrain.terrain_levels, each in [0, L) (kind 1) */
    const int64_t* terrain_types_d;    /* (N) terrain.terrain_types, each in [0, T) (kind 1) */
    int32_t num_levels, num_types, num_patches; /* L, T, P */
    int32_t reserved;
    /* parity draws, NULL = the counter-based in-kernel generator.  uniforms: (2,N,4) samples in [0,1) for {time_left, pos_x, pos_y,
     * heading} of the (up to) two resamplings of a call (reset, timer), the order of the uniform_ calls in CommandTerm._resample
     * (command_manager.py:183) and _resample_command (:92-93, :115); patch_ids: (2,N) the torch.randint draws of kind 1 (:176),
     * each in [0, P).  Kind 1 reads column 0 and, with simple_heading off, column 3 of the uniforms. */
    const float* uniforms_d;
    const int64_t* patch_ids_d;
    float* command_d;                  /* (N,4) [pos_command_b, heading_command_b]: CommandTerm.command (:73-76) */
    float* pos_command_w_d;            /* (N,3) */
    float* heading_command_w_d;        /* (N) */
    float* time_left_d;                /* (N) */
    int64_t* command_counter_d;        /* (N) */
    float* metric_error_pos_2d_d;      /* (N) metrics["error_pos_2d"] (:84) */
    float* metric_error_heading_d;     /* (N) metrics["error_heading"] (:85) */
} imx_pose2d_command_t;

#endif
