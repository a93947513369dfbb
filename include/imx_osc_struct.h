#ifndef IMX_OSC_STRUCT_H_
#define IMX_OSC_STRUCT_H_
/* imx_osc_t, the parameters of one OperationalSpaceControllerAction (imx_osc in imx.h, where the enums, IMX_OSC_CMD_WIDTH and the
 * citations of the reference are).  Included by imx.h after IMX_IK_MAX_JOINTS; not meant to be included on its own.  The binding reads
 * this file with the parser that reads imx.h (isaaclab_amd/_abi.py, OSC_STRUCTS). */
typedef struct imx_osc {
    int32_t pose_type;            /* imx_osc_pose: the motion target, 7 (absolute) or 6 (relative) processed columns */
    int32_t has_wrench;           /* "wrench_abs" in target_types (open loop: contact_wrench_stiffness_task is None) */
    int32_t impedance_mode;       /* imx_osc_impedance */
    int32_t decoupling;           /* imx_osc_decoupling */
    int32_t gravity_compensation;
    int32_t nullspace_position;   /* nullspace_control == "position" (needs full decoupling and more than six joints) */
    int32_t has_offset;           /* cfg.body_offset is not None */
    int32_t pose_col;             /* first column of each part in the (N, PA) processed action; -1 = the part is absent */
    int32_t wrench_col;
    int32_t stiffness_col;
    int32_t damping_ratio_col;
    float motion_axes[6];         /* motion_control_axes_task */
    float wrench_axes[6];         /* contact_wrench_control_axes_task */
    float motion_stiffness[6];    /* motion_stiffness_task (fixed) */
    float motion_damping_ratio[6];/* motion_damping_ratio_task (fixed, variable_kp) */
    float stiffness_limits[2];    /* motion_stiffness_limits_task */
    float damping_ratio_limits[2];/* motion_damping_ratio_limits_task */
    float nullspace_kp;           /* nullspace_stiffness */
    float nullspace_kd;           /* 2 sqrt(nullspace_stiffness) nullspace_damping_ratio (:135-140) */
    float offset_pos[3];
    float offset_rot[4];          /* w, x, y, z */
    int32_t body_idx;             /* row of body_pos_w / body_quat_w / body_lin_vel_w / body_ang_vel_w */
    int32_t jacobi_body_idx;      /* row of the Jacobian tensor: body_idx - 1 for a fixed base (:266-274) */
    int32_t num_joints;           /* 1 .. IMX_IK_MAX_JOINTS */
    int32_t joint_ids[IMX_IK_MAX_JOINTS];        /* columns of joint_pos / joint_vel, rows and columns of the mass matrix (:571-574) */
    int32_t jacobi_joint_ids[IMX_IK_MAX_JOINTS]; /* columns of the Jacobian: joint_ids (+ 6 for a floating base) */
} imx_osc_t;
#endif /* IMX_OSC_STRUCT_H_ */
