#ifndef IMX_OBJECT_STATE_H_
#define IMX_OBJECT_STATE_H_
/* imx_object_state_t: the per-step tensors of the in-hand task (Isaac-Repose-Cube-Allegro-v0) beyond imx_state_t -- the rest of the
 * scene's rigid object's root state (RigidObjectData) and the command term's consecutive_success metric.  imx_state_t does not grow
 * for them: they travel in this struct, bound to the plan with imx_plan_bind_object_state (imx.h) before the launches that read them.
 * A header of its own, included by imx.h, like imx_pose2d_struct.h; it can be included alone.  Each pointer is NULL unless a term of
 * the plan reads it; a plan that reads one is refused with the field's name when it is NULL or nothing is bound. */

typedef struct imx_object_state {
    const float* object_root_quat_w;    /* (N,4) RigidObjectData.root_quat_w w,x,y,z (the in-hand terms, root_quat_w on the object) */
    const float* object_root_lin_vel_w; /* (N,3) RigidObjectData.root_lin_vel_w (root_lin_vel_w on the object) */
    const float* object_root_ang_vel_w; /* (N,3) RigidObjectData.root_ang_vel_w (root_ang_vel_w on the object) */
    const float* command_consecutive_success; /* (N) InHandReOrientationCommand.metrics["consecutive_success"] (orientation_command.py:62, a
                                           float tensor; max_consecutive_success) */
} imx_object_state_t;

#endif
