#ifndef IMX_ARTICULATION_STATE_H_
#define IMX_ARTICULATION_STATE_H_
/* imx_articulation_state_t: the per-step tensors of the scene's SECOND articulation (Isaac-Open-Drawer-Franka-v0: the cabinet) --
 * ArticulationData.joint_pos / joint_vel / body_pos_w / body_quat_w of that asset.  imx_state_t does not grow for them: they travel in
 * this struct, bound to the plan with imx_plan_bind_articulation_state (imx.h) before the launches that read them.  Its row widths J2
 * (joints) and B2 (bodies) are the first two words of the plan's frame table (imx.h, IMX_FT_*).  A header of its own, included by
 * imx.h, like imx_object_state.h; it can be included alone.  Each pointer is NULL unless a term of the plan reads it; a plan that
 * reads one is refused with the field's name when it is NULL or nothing is bound. */

typedef struct imx_articulation_state {
    const float* joint_pos;   /* (N,J2)   ArticulationData.joint_pos (joint_pos_rel on the asset, open_drawer_bonus, multi_stage_open_drawer) */
    const float* joint_vel;   /* (N,J2)   ArticulationData.joint_vel (joint_vel_rel on the asset) */
    const float* body_pos_w;  /* (N,B2,3) ArticulationData.body_pos_w (a FrameTransformer frame on a body of the asset) */
    const float* body_quat_w; /* (N,B2,4) ArticulationData.body_quat_w w,x,y,z */
} imx_articulation_state_t;

#endif
