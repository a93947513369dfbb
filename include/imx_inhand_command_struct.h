#ifndef IMX_INHAND_COMMAND_STRUCT_H_
#define IMX_INHAND_COMMAND_STRUCT_H_
/* imx_inhand_command_t: the in-hand re-orientation command term (isaaclab_tasks .../manipulation/inhand/mdp/commands/
 * orientation_command.py:22-124, InHandReOrientationCommand, cfg commands_cfg.py:19-71) as imx_inhand_command (imx.h, where the entry
 * point is) takes it.  A header of its own, included by imx.h, like imx_pose2d_struct.h; it can be included alone.  The term is
 * stand-alone: imx_orch_t does not grow for it and no orchestration launch runs it yet. */
#include <stdint.h>

typedef struct imx_inhand_command {
    float cfg[4];                        /* resampling_time_range lo, hi; orientation_success_threshold; reserved (0) */
    int32_t make_quat_unique;            /* cfg.make_quat_unique: quat_unique on a resampled goal (utils/math.py:448-460) */
    int32_t update_goal_on_success;      /* cfg.update_goal_on_success: _update_command resamples where orientation_error < threshold */
    /* fixed at construction (:43-45): pos_command_e = default object root position + cfg.init_pos_offset lies in command_d[:, :3],
     * pos_command_w = pos_command_e + env_origins here */
    const float* pos_command_w_d;        /* (N,3) */
    /* the object's root pose of the current (post-physics) state: RigidObjectData.root_pos_w / root_quat_w */
    const float* object_root_pos_w_d;    /* (N,3) */
    const float* object_root_quat_w_d;   /* (N,4) w, x, y, z */
    const uint8_t* reset_mask_d;         /* (N) the envs CommandTerm.reset runs on before the compute, or NULL = none */
    /* parity draws, NULL = the counter-based in-kernel generator keyed by (seed, column, *step_counter_d (NULL = 0), env).  (3,N,3)
     * samples in [0,1) for {time_left, rand_floats[:, 0], rand_floats[:, 1]} of the (up to) three resamplings of a call -- reset, timer,
     * goal reached -- in the order CommandTerm._resample (command_manager.py:172-187) and _resample_command (:104-111) draw them */
    const float* uniforms_d;
    uint64_t seed;
    const int32_t* step_counter_d;
    float* command_d;                    /* (N,7) CommandTerm.command (:75-78): [pos_command_e, quat_command_w]; columns 3..6 are written */
    float* time_left_d;                  /* (N) */
    int64_t* command_counter_d;          /* (N) */
    float* metric_orientation_error_d;   /* (N) metrics["orientation_error"] (:94-97) */
    float* metric_position_error_d;      /* (N) metrics["position_error"] (:98) */
    float* metric_consecutive_success_d; /* (N) metrics["consecutive_success"] (:99-101), a float tensor */
    /* optional (ceil(N / 64), 4): per 64 envs, the sums over the reset envs of the three metrics as they stood before the reset (what
     * CommandTerm.reset logs the mean of, command_manager.py:136-141) in this order, then the number of reset envs */
    float* log_part_d;
} imx_inhand_command_t;

#endif
