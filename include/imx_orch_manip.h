#ifndef IMX_ORCH_MANIP_H_
#define IMX_ORCH_MANIP_H_
/* imx_orch_manip_t: what imx_reset_orchestrate_manip (imx.h, where the entry point is) takes beside imx_orch_t.  A header of its
 * own, included by imx.h, like imx_osc_struct.h; it can be included alone. */
#include <stdint.h>

#define IMX_ORCH_MAX_WEIGHT_TERMS 4

/* one modify_reward_weight curriculum term (envs/mdp/curriculums.py:21-36) */
typedef struct imx_weight_term {
    float* weight_d;        /* imx_plan_reward_weight_ptr(plan, index of params["term_name"]) */
    float* step_reward_d;   /* the term's column of RewardManager._step_reward, &step_reward[0][index] (rows step_reward_stride apart):
                               from the step after the one that puts the term to sleep (a non-zero weight word becomes 0) it is
                               zeroed for every env, since the zero-weight skip (reward_manager.py:145) never writes the column
                               again.  NULL = left as it is */
    int32_t* switch_step_d; /* one int32 of device state for step_reward_d, 0 at the start: 1 + the step count of that switch */
    float weight;           /* params["weight"] */
    int32_t num_steps;      /* params["num_steps"]: stored when common_step_counter > num_steps, in a launch that resets an env */
} imx_weight_term_t;

typedef struct imx_orch_manip {
    /* the scene's one RigidObject (assets/rigid_object): NULL default = the scene has none */
    const float* object_default_root_state_d;  /* (N,13) RigidObjectData.default_root_state */
    float* object_root_pose_out_d;             /* (N,7) what object.write_root_pose_to_sim receives */
    float* object_root_vel_out_d;              /* (N,6) what object.write_root_velocity_to_sim receives */
    int32_t num_weight_terms;                  /* 0..IMX_ORCH_MAX_WEIGHT_TERMS, cfg order */
    int32_t step_reward_stride;                /* K, the number of reward terms: floats per row of the (N,K) step_reward */
    imx_weight_term_t weight_terms[IMX_ORCH_MAX_WEIGHT_TERMS];
} imx_orch_manip_t;

#endif
