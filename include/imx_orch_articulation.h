#ifndef IMX_ORCH_ARTICULATION_H_
#define IMX_ORCH_ARTICULATION_H_
/* imx_orch_articulation_t: what imx_reset_orchestrate_scene (imx.h, where the entry point is) takes beside imx_orch_t and
 * imx_orch_manip_t -- the scene's SECOND articulation (Isaac-Open-Drawer-Franka-v0: the cabinet) as the reset events see it
 * (imx_event_term_t.asset = 2): its defaults, its limits and its four "to simulator" buffers.  A header of its own, included by
 * imx.h, like imx_pose2d_struct.h; it can be included alone. */
#include <stdint.h>

typedef struct imx_orch_articulation {
    int64_t num_joints;                    /* J2 > 0 */
    const float* default_root_state_d;     /* (N,13) ArticulationData.default_root_state */
    const float* default_joint_pos_d;      /* (N,J2) */
    const float* default_joint_vel_d;      /* (N,J2) */
    const float* soft_joint_pos_limits_d;  /* (N,J2,2) or NULL: read by reset_joints_by_offset / reset_joints_by_scale on this asset only */
    const float* soft_joint_vel_limits_d;  /* (N,J2)   or NULL, likewise */
    float* root_pose_out_d;                /* (N,7)  what asset.write_root_pose_to_sim receives */
    float* root_vel_out_d;                 /* (N,6)  what asset.write_root_velocity_to_sim receives */
    float* joint_pos_out_d;                /* (N,J2) what asset.write_joint_state_to_sim receives */
    float* joint_vel_out_d;                /* (N,J2) */
} imx_orch_articulation_t;

#endif
