/* imx.h -- C ABI of libimx: the MI355X (gfx950) implementation of IsaacLab's post-physics env-step hot path.
 *
 * The reference (godk1122/IsaacLab v2.1.0) has NO native ABI on this path: the boundary is two Python protocols
 * (ManagerBasedRLEnv.step/reset and RslRlVecEnvWrapper).  This header is what the Python
 * shim (isaaclab_amd/_lib.py, ctypes) binds; each entry point cites the reference code it replaces.
 * Paths are relative to /root/reference/source/isaaclab/isaaclab unless noted.
 *
 * Conventions
 *   - every pointer named *_d / inside imx_state_t / imx_buffers_t is a DEVICE pointer owned by the caller
 *     (torch tensors); the library never allocates per call, never synchronises the stream, never frees them;
 *   - all launches go to the hipStream_t passed in (the caller passes torch's current stream);
 *   - return value: 0 = ok, non-zero = error; imx_last_error() gives the message (thread-local);
 *   - floats are fp32, bools are 1-byte (torch.bool layout), indices int64 (torch.long), row-major contiguous.
 */
#ifndef IMX_H_
#define IMX_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct imx_plan imx_plan_t; /* compiled term tables (one per env cfg) */
typedef struct imx_mesh imx_mesh_t; /* terrain mesh + 2-D uniform grid acceleration structure */
typedef void* imx_stream_t;         /* hipStream_t */

/* ---- plan blob: int32 words written by isaaclab_amd/plan.py -------------------------------------------------- */
#define IMX_MAGIC 0x31584D49 /* "IMX1" */
#define IMX_PLAN_VERSION 3
#define IMX_HEADER_WORDS 48
#define IMX_MAX_OBS_GROUPS 4
#define IMX_REC_WORDS 20
/* The frame table of a plan whose terms read FrameTransformer frames (the manipulation/cabinet terms): written once into the blob's
 * list area, referenced by the records that read it (their IMX_R_AUX0 word = its offset).  IMX_FT_HEADER_WORDS words
 * [J2, B2, number of ee_frame targets, number of cabinet_frame targets] -- J2 / B2 = joints / bodies of the scene's second
 * articulation, the row widths of imx_articulation_state_t (0 without one) -- then one frame of IMX_FRAME_WORDS words
 * [body id, asset (0 the robot: imx_state_t.body_pos_w / body_quat_w, 1 the second articulation: imx_articulation_state_t),
 * offset position x y z (f32), offset rotation w x y z (f32)] for: the ee_frame's source, its targets in cfg order, the
 * cabinet_frame's source, its targets.  imx_frame_transformer takes frames in the same 9-word form. */
#define IMX_FRAME_WORDS 9
#define IMX_FT_HEADER_WORDS 4

enum imx_header_word {
    IMX_H_MAGIC = 0, IMX_H_VERSION, IMX_H_J, IMX_H_B, IMX_H_H, IMX_H_A, IMX_H_D, IMX_H_R, IMX_H_NTERM, IMX_H_NREW,
    IMX_H_NOBS, IMX_H_NACT, IMX_H_MAX_EP_LEN, IMX_H_STEP_DT /*f32*/, IMX_H_TERM_OFF, IMX_H_REW_OFF, IMX_H_OBS_OFF,
    IMX_H_ACT_OFF, IMX_H_TOTAL_WORDS, IMX_H_NB /* articulation bodies */, IMX_H_GRAV_X /*f32*/, IMX_H_GRAV_Y,
    IMX_H_GRAV_Z, IMX_H_NREW_ALL /* reward terms incl. zero-weight */, IMX_H_RAY_OFF /* R*3 f32 local ray starts */,
    IMX_H_RAYDIR_X /*f32*/, IMX_H_RAYDIR_Y, IMX_H_RAYDIR_Z, IMX_H_RAY_MAXDIST /*f32*/, IMX_H_MAX_EP_LEN_S /*f32*/,
    IMX_H_NEXT_REW, IMX_H_NEXT_TERM, IMX_H_NEXT_OBS, IMX_H_RAY_YAW_ONLY, IMX_H_CMD_DIM,
    IMX_H_MOD_STATE /* floats of observation-modifier state per env (imx_buffers.mod_state row width) */,
    IMX_H_NGROUPS /* observation groups (ObservationManager group loop, observation_manager.py:238-258), 1..IMX_MAX_OBS_GROUPS */,
    IMX_H_GROUP_OFF /* NGROUPS x 4 words: D_g, enable_corruption, first obs record, number of obs records (IMX_H_D = sum of D_g) */,
    /* height scanner as a SensorBase (sensors/sensor_base.py:182-205,287-297; ray_caster.py:107-114,236-237) */
    IMX_H_SCAN_PERIOD /* f32 cfg.update_period */, IMX_H_SCAN_DT /* f32 physics dt: SensorBase.update(dt) per physics step */,
    IMX_H_SCAN_SUBSTEPS /* decimation: update() calls per env step */, IMX_H_SCAN_DRIFT_LO /* f32 cfg.drift_range */,
    IMX_H_SCAN_DRIFT_HI, IMX_H_SCAN_STATEFUL /* 1: per-env timestamps / drift are kept (imx_buffers.scan_state) */,
    IMX_H_TERM_SLOTS /* per-env reward-term state slots (imx_buffers.term_state rows): one per IMX_W_PROGRESS_REWARD record */,
    IMX_H_PA /* width of buf.processed_action (joint targets of all action terms side by side); 0 = IMX_H_A: every term writes as many
                processed columns as it takes raw ones.  Differs for a IMX_A_BINARY_JOINT term (1 raw column, NIDS targets) */
};

/* record layout (IMX_REC_WORDS int32/f32 words) */
enum imx_rec_word {
    IMX_R_OP = 0, IMX_R_IDS_OFF, IMX_R_NIDS, IMX_R_IDS2_OFF, IMX_R_NIDS2,
    IMX_R_WEIGHT /*f32 reward weight (0 = skipped, reward_manager.py:145); termination: time_out flag; observation: group index*/,
    IMX_R_P0 /*f32*/, IMX_R_P1, IMX_R_P2, IMX_R_P3, IMX_R_OUT /* obs: column offset; reward/term: term index */,
    IMX_R_DIM, IMX_R_FLAGS, IMX_R_NOISE_LO /*f32*/, IMX_R_NOISE_HI, IMX_R_CLIP_LO, IMX_R_CLIP_HI, IMX_R_SCALE,
    IMX_R_AUX0, IMX_R_AUX1
};
/* obs post-processing flags (observation_manager.py:310-318) */
#define IMX_F_NOISE_ADD 1
#define IMX_F_NOISE_SCALE 2
#define IMX_F_NOISE_ABS 4
#define IMX_F_CLIP 8
#define IMX_F_SCALE 16
#define IMX_F_QUAT_UNIQUE 32
/* the obs record carries a modifier program (ObservationTermCfg.modifiers, observation_manager.py:310-312), run on the raw
 * term value before noise/clip/scale: IMX_R_IDS2_OFF = word offset of the program, IMX_R_NIDS2 = its length in words,
 * IMX_R_P1 (int) = first float of the term's state in a mod_state row.  Program = ops back to back, 4 words each
 * [op, a, b, soff] (DIGITAL_FILTER: [op, na, nb, soff] followed by na + nb f32 coefficients A then B).  State of element
 * j of a term of width d: mod_state[e][P1 + (soff + k) * d + j]; zeroed for envs reset this step before it is used. */
#define IMX_F_MODIFIERS 64
/* a height_scan record that reuses the ray hits of an earlier height_scan record (IMX_R_AUX0 = that record's index), e.g. the
 * "critic" group scanning the same sensor as "policy": one cast per ray and step, as the reference's lazily updated sensor. */
#define IMX_F_SCAN_TWIN 128
/* the noise of the term is gaussian_noise (utils/noise/noise_model.py:71-94): NOISE_LO = mean, NOISE_HI = std, combined by the ADD / SCALE / ABS bit;
 * samples: the fed array holds the reference's randn draws, else an in-kernel Box-Muller pair of the counter-based uniforms.
 * (constant_noise, :17-39, needs no flag: a uniform noise with NOISE_LO = NOISE_HI = bias is bit-identical) */
#define IMX_F_NOISE_GAUSS 1024
enum imx_mod_op {            /* utils/modifiers/modifier.py */
    IMX_M_SCALE = 1,         /* :22-32   a = multiplier */
    IMX_M_BIAS,              /* :49-60   a = value */
    IMX_M_CLIP,              /* :35-46   a = lo (-inf if None), b = hi (+inf if None) */
    IMX_M_INTEGRATOR,        /* :179-259 a = dt; state: integral, y_prev */
    IMX_M_DIGITAL_FILTER     /* :63-176  state: x_n[nb], y_n[na] */
};
/* action record flags */
#define IMX_F_ACT_DEFAULT_POS_OFFSET 1 /* JointPositionAction use_default_offset (joint_actions.py:152-154) */
#define IMX_F_ACT_DEFAULT_VEL_OFFSET 2 /* JointVelocityAction (joint_actions.py:206-208) */
#define IMX_F_ACT_CLIP 4
#define IMX_F_ACT_EMA 16 /* EMAJointPositionToLimitsAction (joint_actions_to_limits.py:142-230): alpha * processed + (1 - alpha) * previous applied action,
                           clamped to the soft limits; alpha = P1 or the per-joint table AUX1; the previous applied action is processed_action
                           itself (an env reset in the last step starts from its joint positions, :208-217: reset_buf is read) */
#define IMX_F_ACT_TO_LIMITS 8 /* JointPositionToLimitsAction rescale_to_limits: clamp(-1, 1), unscale_transform onto soft_joint_pos_limits (joint_actions_to_limits.py:116-126) */

/* termination ops -- envs/mdp/terminations.py */
enum imx_term_op {
    IMX_T_TIME_OUT = 1,            /* :30-32 */
    IMX_T_ILLEGAL_CONTACT,         /* :150-158  ids=bodies p0=threshold */
    IMX_T_JOINT_POS_MANUAL_LIMIT,  /* :90-105   ids=joints p0=lo p1=hi */
    IMX_T_BAD_ORIENTATION,         /* :50-59    p0=limit_angle */
    IMX_T_ROOT_HEIGHT_BELOW_MIN,   /* :62-72    p0=minimum_height; aux0 = the asset: 0 robot root (state.root_pos_w), 1 the rigid object
                                                (state.object_root_pos_w) */
    IMX_T_JOINT_VEL_LIMIT,         /* :108-114  ids=joints */
    IMX_T_JOINT_VEL_MANUAL_LIMIT,  /* :117-124  ids=joints p0=max_velocity */
    IMX_T_JOINT_EFFORT_LIMIT,      /* :127-142  ids=joints (torch.isclose(computed, applied)) */
    IMX_T_TERRAIN_OUT_OF_BOUNDS,   /* isaaclab_tasks .../velocity/mdp/terminations.py:24-52  p0=x_lim p1=y_lim */
    IMX_T_EXTERNAL,                /* value computed by a Python term; aux0 = column in ext_term */
    IMX_T_COMMAND_RESAMPLE,        /* :35-42    p0 = f32(step_dt), nids = num_resamples; state.command_time_left / command_counter */
    IMX_T_OBJECT_REACHED_GOAL,     /* isaaclab_tasks .../manipulation/lift/mdp/terminations.py:25-53  ||des_pos_w - object_root_pos_w|| < p0
                                      (threshold); des_pos_w as for the reach rewards, CMD == 7 */
    /* isaaclab_tasks .../manipulation/inhand/mdp/terminations.py (Isaac-Repose-Cube-Allegro-v0); command = (N, 7): the goal position in
       the ENV frame + the goal quaternion in the world frame (InHandReOrientationCommand.command, orientation_command.py:75-78) */
    IMX_T_MAX_CONSECUTIVE_SUCCESS, /* :18-28   imx_object_state_t.command_consecutive_success >= p0 (num_success as f32: the metric is a float tensor) */
    IMX_T_OBJECT_AWAY_FROM_GOAL,   /* :31-56   ||(object_root_pos_w - env_origins) - cmd[:3]|| > p0 (threshold): env frame */
    IMX_T_OBJECT_AWAY_FROM_ROBOT   /* :59-83   ||root_pos_w - object_root_pos_w|| > p0 (threshold) */
};

/* reward ops -- envs/mdp/rewards.py unless noted */
enum imx_rew_op {
    IMX_W_IS_ALIVE = 1,               /* :31-33 */
    IMX_W_IS_TERMINATED,              /* :36-38 */
    IMX_W_IS_TERMINATED_TERM,         /* :41-68   ids = termination term indices */
    IMX_W_LIN_VEL_Z_L2,               /* :76-80 */
    IMX_W_ANG_VEL_XY_L2,              /* :83-87 */
    IMX_W_FLAT_ORIENTATION_L2,        /* :90-97 */
    IMX_W_BASE_HEIGHT_L2,             /* :100-122 (no sensor) p0=target */
    IMX_W_JOINT_TORQUES_L2,           /* :136-143 */
    IMX_W_JOINT_VEL_L1,               /* :146-150 */
    IMX_W_JOINT_VEL_L2,               /* :153-160 */
    IMX_W_JOINT_ACC_L2,               /* :163-170 */
    IMX_W_JOINT_DEVIATION_L1,         /* :173-179 */
    IMX_W_JOINT_POS_LIMITS,           /* :182-196 */
    IMX_W_JOINT_VEL_LIMITS,           /* :199-218 p0=soft_ratio */
    IMX_W_APPLIED_TORQUE_LIMITS,      /* :226-242 */
    IMX_W_ACTION_RATE_L2,             /* :245-247 */
    IMX_W_ACTION_L2,                  /* :250-252 */
    IMX_W_UNDESIRED_CONTACTS,         /* :260-268 ids=bodies p0=threshold */
    IMX_W_CONTACT_FORCES,             /* :271-279 ids=bodies p0=threshold */
    IMX_W_TRACK_LIN_VEL_XY_EXP,       /* :287-298 p0=std */
    IMX_W_TRACK_ANG_VEL_Z_EXP,        /* :301-309 p0=std */
    IMX_W_FEET_AIR_TIME,              /* isaaclab_tasks .../velocity/mdp/rewards.py:25-44 ids=bodies p0=threshold */
    IMX_W_FEET_AIR_TIME_POSITIVE_BIPED, /* ...:47-66 */
    IMX_W_FEET_SLIDE,                 /* ...:69-83  ids=sensor bodies ids2=asset bodies */
    IMX_W_TRACK_LIN_VEL_XY_YAW_FRAME_EXP, /* ...:86-96 */
    IMX_W_TRACK_ANG_VEL_Z_WORLD_EXP,  /* ...:99-106 */
    IMX_W_JOINT_POS_TARGET_L2,        /* isaaclab_tasks .../classic/cartpole/mdp/rewards.py:19-26 p0=target */
    IMX_W_EXTERNAL,                   /* aux0 = column in ext_reward */
    IMX_W_BODY_LIN_ACC_L2,            /* :125-128 ids = asset bodies; state.body_lin_acc_w */
    /* isaaclab_tasks .../velocity/config/spot/mdp/rewards.py.  "stand still" = ||cmd|| == 0 (all 3 components) and ||v_b,xy|| <= threshold */
    IMX_W_AIR_TIME_REWARD,            /* :31-58   ids = 4 sensor bodies; p0 = mode_time, p1 = velocity_threshold */
    IMX_W_BASE_ANGULAR_VELOCITY_REWARD, /* :61-68 p0 = std: exp(-|cmd_z - w_b,z| / std) */
    IMX_W_BASE_LINEAR_VELOCITY_REWARD,  /* :71-83 p0 = std, p1 = ramp_rate, p2 = ramp_at_vel */
    IMX_W_GAIT_REWARD,                /* :86-177  ids = sensor bodies pair0[0], pair0[1], pair1[0], pair1[1]; p0 = std, p1 = max_err^2,
                                                  p2 = velocity_threshold */
    IMX_W_FOOT_CLEARANCE_REWARD,      /* :180-188 ids = asset bodies; p0 = target_height, p1 = std, p2 = tanh_mult; state.body_pos_w */
    IMX_W_ACTION_SMOOTHNESS_PENALTY,  /* :196-198 ||a - a_prev|| */
    IMX_W_AIR_TIME_VARIANCE_PENALTY,  /* :201-212 ids = sensor bodies; unbiased var of last air / contact time clipped at 0.5 */
    IMX_W_BASE_MOTION_PENALTY,        /* :216-222 */
    IMX_W_BASE_ORIENTATION_PENALTY,   /* :225-232 */
    IMX_W_FOOT_SLIP_PENALTY,          /* :235-249 ids = sensor bodies, ids2 = asset bodies; p0 = threshold */
    IMX_W_JOINT_ACCELERATION_PENALTY, /* :252-256 ids = ALL joints (the function ignores asset_cfg.joint_ids) */
    IMX_W_JOINT_POSITION_PENALTY,     /* :259-268 ids = all joints; p0 = stand_still_scale, p1 = velocity_threshold */
    IMX_W_JOINT_TORQUES_PENALTY,      /* :271-275 ids = all joints */
    IMX_W_JOINT_VELOCITY_PENALTY,     /* :278-282 ids = all joints */
    /* isaaclab_tasks .../classic/humanoid/mdp/rewards.py (Isaac-Ant-v0, Isaac-Humanoid-v0) */
    IMX_W_UPRIGHT_POSTURE_BONUS,      /* :21-27   p0 = threshold: -projected_gravity_b.z > threshold */
    IMX_W_MOVE_TO_TARGET_BONUS,       /* :30-40   p0 = threshold, p1, p2 = target x, y (base_heading_proj) */
    IMX_W_PROGRESS_REWARD,            /* :43-78   p0..p2 = target; aux0 = term_state slot (the potentials; prev_potentials is the value
                                                  read before the update) */
    IMX_W_JOINT_POS_LIMITS_PENALTY_RATIO, /* :81-111 ids = all joints; ids2 = (J) f32 gear_ratio_scaled; p0 = threshold,
                                                  p1 = f32(1 - threshold) (the Python double) */
    IMX_W_POWER_CONSUMPTION,          /* :114-140 ids = all joints; ids2 = (J) f32 gear_ratio_scaled; reads buf.action (raw, A == J) */
    /* isaaclab_tasks .../manipulation/reach/mdp/rewards.py (Isaac-Reach-Franka-v0, Isaac-Reach-UR10-v0); ids = the ONE asset body
       (asset_cfg.body_ids[0]); command = (N, 7) pose in the base frame (CMD == 7); des_pos_w = root_pos_w + quat_apply(root_quat_w,
       cmd[:3]) (combine_frame_transforms, utils/math.py:750-786 -> quat_apply :546-566) */
    IMX_W_POSITION_COMMAND_ERROR,     /* :19-33  ||body_pos_w[:, id] - des_pos_w|| */
    IMX_W_POSITION_COMMAND_ERROR_TANH,/* :36-53  1 - tanh(||body_pos_w[:, id] - des_pos_w|| / p0), p0 = std */
    IMX_W_ORIENTATION_COMMAND_ERROR,  /* :56-72  quat_error_magnitude(body_quat_w[:, id], quat_mul(root_quat_w, cmd[3:7])) (math.py:678-690:
                                                  ||axis_angle_from_quat(quat_mul(q1, quat_conjugate(q2)))||, :646-675) */
    /* isaaclab_tasks .../manipulation/lift/mdp/rewards.py (Isaac-Lift-Cube-Franka-v0); the object = state.object_root_pos_w */
    IMX_W_OBJECT_IS_LIFTED,           /* :20-25  object z > p0 (minimal_height) -> 1 / 0 */
    IMX_W_OBJECT_EE_DISTANCE,         /* :28-45  1 - tanh(||object - ee_w|| / p0), p0 = std; ee_w = the FrameTransformer's first target frame =
                                                  body_pos_w[:, id] + quat_apply(body_quat_w[:, id], (p1, p2, p3)): ids = the ONE robot body the frame
                                                  sits on, p1..p3 = its offset position (frame_transformer.py:358; identity offset rotation) */
    IMX_W_OBJECT_GOAL_DISTANCE,       /* :48-67  (object z > p1) * (1 - tanh(||des_pos_w - object|| / p0)), p0 = std, p1 = minimal_height;
                                                  des_pos_w as for the reach rewards, CMD == 7 */
    /* isaaclab_tasks .../navigation/mdp/rewards.py (Isaac-Navigation-Flat-Anymal-C-v0); command = (N, 4) pose-2d command in the base
       frame (CMD == 4): pos_command_b 3, heading_command_b 1.  A plan with these ops runs k_term_rew_nav and holds no classic, reach or
       lift op */
    IMX_W_NAV_POSITION_COMMAND_ERROR_TANH, /* :17-22  1 - tanh(||cmd[:3]|| / p0), p0 = std */
    IMX_W_NAV_HEADING_COMMAND_ERROR_ABS,   /* :25-29  |cmd[3]| */
    /* isaaclab_tasks .../manipulation/inhand/mdp/rewards.py (Isaac-Repose-Cube-Allegro-v0); command as for the in-hand terminations
       (CMD == 7); dtheta = quat_error_magnitude(object_root_quat_w, cmd[3:7]) (utils/math.py:678-690), computed once per env.  A plan with
       these ops or the three in-hand termination ops runs k_term_rew_inhand and holds no classic, reach, lift or navigation reward op and
       no object_reached_goal termination; root_height_below_minimum on the object (aux0 = 1) is served there as well */
    IMX_W_TRACK_ORIENTATION_INV_L2,   /* :71-96  1 / (dtheta + p0), p0 = rot_eps */
    IMX_W_SUCCESS_BONUS,              /* :20-44  dtheta <= p0 -> 1 / 0, p0 = the command cfg's orientation_success_threshold (`<=`: the
                                                  command term's own success test is `<`) */
    IMX_W_TRACK_POS_L2,               /* :47-68  ||cmd[:3] - (object_root_pos_w - env_origins)|| */
    /* (op number IMX_W_TRACK_POS_L2 + 1 = 60 is reserved: imx_plan_create keeps refusing it as an unknown reward op)
       isaaclab_tasks .../manipulation/cabinet/mdp/rewards.py (Isaac-Open-Drawer-Franka-v0).  Every record: aux0 = the plan's frame table
       (IMX_FT_*).  tcp / lfinger / rfinger = targets 0 / 1 / 2 of the ee_frame, handle = target 0 of the cabinet_frame, each
       combine_frame_transforms(body pose, offset) (frame_transformer.py:357-363), computed once per env; is_graspable =
       (rfinger.z < handle.z) & (lfinger.z > handle.z).  A plan with these ops runs k_term_rew_cabinet and holds no classic, reach, lift,
       navigation or in-hand op */
    IMX_W_APPROACH_EE_HANDLE = 61,    /* :18-40   r = (1 / (1 + d^2))^2, d = ||handle - tcp||; 2 r where d <= p0 (threshold) */
    IMX_W_ALIGN_EE_HANDLE,            /* :43-72   0.5 (sign(az) az^2 + sign(ax) ax^2), az = tcp_z . -handle_x, ax = tcp_x . -handle_y (columns of
                                                  matrix_from_quat, utils/math.py:144-174) */
    IMX_W_ALIGN_GRASP_AROUND_HANDLE,  /* :75-91   is_graspable -> 1 / 0 (the manager's multiplication turns the bool into a float) */
    IMX_W_APPROACH_GRIPPER_HANDLE,    /* :94-114  is_graspable * ((p0 - |lfinger.z - handle.z|) + (p0 - |rfinger.z - handle.z|)), p0 = offset */
    IMX_W_GRASP_HANDLE,               /* :117-135 (d <= p0) * sum_ids(p1 - joint_pos[id]); p0 = threshold, p1 = open_joint_pos, ids = the
                                                  robot's gripper joints */
    IMX_W_OPEN_DRAWER_BONUS,          /* :138-146 (is_graspable + 1) * joint_pos[ids[0]]; aux1 = whose joint: 0 the robot, 1 the second
                                                  articulation (imx_articulation_state_t.joint_pos, row width J2) */
    IMX_W_MULTI_STAGE_OPEN_DRAWER     /* :149-162 (q > 0.01) 0.5 + (q > 0.2) g + (q > 0.3) g, q = joint_pos[ids[0]] as above, g = is_graspable */
};

/* observation ops -- envs/mdp/observations.py */
enum imx_obs_op {
    IMX_O_BASE_POS_Z = 1,   /* :33-37 */
    IMX_O_BASE_LIN_VEL,     /* :40-44 */
    IMX_O_BASE_ANG_VEL,     /* :47-51 */
    IMX_O_PROJECTED_GRAVITY,/* :54-58 */
    /* the four root observations: aux0 = the asset -- 0 the robot (the word every older blob has), 1 the scene's rigid object
       (state.object_root_pos_w and imx_object_state_t; as IMX_T_ROOT_HEIGHT_BELOW_MIN's selector) */
    IMX_O_ROOT_POS_W,       /* :61-65 (minus env origins, on either asset) */
    IMX_O_ROOT_QUAT_W,      /* :68-83 */
    IMX_O_ROOT_LIN_VEL_W,   /* :85-89 */
    IMX_O_ROOT_ANG_VEL_W,   /* :92-96 */
    IMX_O_JOINT_POS,        /* :104-111 */
    IMX_O_JOINT_POS_REL,    /* :114-121 */
    IMX_O_JOINT_POS_LIMIT_NORMALIZED, /* :124-137 */
    IMX_O_JOINT_VEL,        /* :140-147 */
    IMX_O_JOINT_VEL_REL,    /* :150-157 */
    IMX_O_HEIGHT_SCAN,      /* :165-173 p0=offset */
    IMX_O_LAST_ACTION,      /* :512-521 */
    IMX_O_GENERATED_COMMANDS, /* :529-531 */
    IMX_O_EXTERNAL,         /* aux0 = column offset in ext_obs */
    /* isaaclab_tasks .../classic/humanoid/mdp/observations.py; angles are atan2(sin, cos) of the euler_xyz_from_quat angle mod 2 pi */
    IMX_O_BASE_YAW_ROLL,    /* :19-30  2 columns: yaw, roll */
    IMX_O_BASE_UP_PROJ,     /* :33-40  -projected_gravity_b.z */
    IMX_O_BASE_HEADING_PROJ,/* :43-58  p0..p2 = target_pos: quat_rotate(q, FORWARD_VEC_B) . normalize((target - pos) * (1, 1, 0)) */
    IMX_O_BASE_ANGLE_TO_TARGET, /* :61-77 p0..p2 = target_pos */
    IMX_O_BODY_INCOMING_WRENCH, /* envs/mdp/observations.py:176-185 ids = asset bodies; 6 columns per body in id order;
                                   state.link_incoming_joint_force */
    IMX_O_OBJECT_POSITION_IN_ROBOT_ROOT_FRAME, /* isaaclab_tasks .../manipulation/lift/mdp/observations.py:19-31  3 columns:
                                   quat_apply(quat_inv(root_quat_w), object_root_pos_w - root_pos_w) (subtract_frame_transforms,
                                   utils/math.py:785-816; quat_inv = normalize(conjugate), :239-248) */
    IMX_O_GOAL_QUAT_DIFF,   /* isaaclab_tasks .../manipulation/inhand/mdp/observations.py:20-38  4 columns:
                                   quat_mul(object_root_quat_w, quat_conjugate(cmd[3:7])), CMD == 7; IMX_F_QUAT_UNIQUE when make_quat_unique */
    /* isaaclab_tasks .../manipulation/cabinet/mdp/observations.py (Isaac-Open-Drawer-Franka-v0); aux0 = the plan's frame table
       (IMX_FT_*), frames as for the cabinet rewards.  A plan with one of the six ops below runs k_obs_cabinet */
    IMX_O_REL_EE_DRAWER_DISTANCE, /* :27-32  3 columns: handle - tcp */
    IMX_O_EE_POS,           /* :43-48  3 columns: tcp - env_origins */
    IMX_O_EE_QUAT,          /* :51-59  4 columns: the tcp's quaternion; IMX_F_QUAT_UNIQUE when make_quat_unique */
    IMX_O_FINGERTIPS_POS,   /* :35-40  3 x (ee_frame targets - 1) columns: targets 1.. minus env_origins */
    /* envs/mdp/observations.py joint_pos_rel :114-121 / joint_vel_rel :150-157 on the scene's second articulation: ids = its joints,
       p2 (int) = word offset of as many f32 defaults (default_joint_pos / default_joint_vel of those joints, from the asset's
       init_state), aux0 = the frame table (its first word is the row width J2 of imx_articulation_state_t.joint_pos / joint_vel) */
    IMX_O_ARTICULATION_JOINT_POS_REL,
    IMX_O_ARTICULATION_JOINT_VEL_REL,
    /* envs/mdp/observations.py:188-231 on an Imu sensor of the scene; aux0 = the sensor's index among those imx_plan_bind_imu bound.
       A plan with one of the three ops below runs k_obs_imu */
    IMX_O_IMU_ORIENTATION = 32, /* :188-201  4 columns: data.quat_w  (31 stays unknown: tests/test_cabinet_plan.py pins it) */
    IMX_O_IMU_ANG_VEL = 33,     /* :204-216  3 columns: data.ang_vel_b */
    IMX_O_IMU_LIN_ACC = 34      /* :219-231  3 columns: data.lin_acc_b */
};

/* action ops.  A record takes the raw columns [OUT, OUT + DIM) of the action and writes the processed columns [PCOL, PCOL + NIDS) of
 * buf.processed_action (row width IMX_H_PA), PCOL = the record's IMX_R_P2 word (int; 0 = OUT, as in every plan whose terms are all
 * IMX_A_JOINT_AFFINE).
 *   IMX_A_JOINT_AFFINE  envs/mdp/actions/joint_actions.py:130-139 (raw*scale+offset[,clamp]); DIM == NIDS
 *   IMX_A_BINARY_JOINT  BinaryJointPositionAction / BinaryJointVelocityAction (binary_joint_actions.py:118-133): DIM == 1; every one of the
 *                       NIDS joints gets its entry of the close table (AUX1) where the raw action is < 0, else of the open table (AUX0);
 *                       NIDS floats each, the term's clip already applied to both (clamp commutes with the selection) */
enum imx_act_op { IMX_A_JOINT_AFFINE = 1, IMX_A_BINARY_JOINT };

/* ---- per-step inputs: the tensors ArticulationData / ContactSensorData / CommandManager expose ---------------- */
typedef struct imx_state {
    const float* root_pos_w;            /* (N,3)   assets/articulation/articulation_data.py root_pos_w */
    const float* root_quat_w;           /* (N,4) w,x,y,z */
    const float* root_lin_vel_w;        /* (N,3) */
    const float* root_ang_vel_w;        /* (N,3) */
    const float* joint_pos;             /* (N,J) */
    const float* joint_vel;             /* (N,J) */
    const float* joint_acc;             /* (N,J) */
    const float* applied_torque;        /* (N,J) */
    const float* computed_torque;       /* (N,J) */
    const float* default_joint_pos;     /* (N,J) */
    const float* default_joint_vel;     /* (N,J) */
    const float* soft_joint_pos_limits; /* (N,J,2) */
    const float* soft_joint_vel_limits; /* (N,J) */
    const float* body_lin_vel_w;        /* (N,NB,3) */
    const float* command;               /* (N,CMD) command_manager.get_command() */
    const float* net_forces_w_history;  /* (N,H,B,3) sensors/contact_sensor/contact_sensor_data.py */
    const float* last_air_time;         /* (N,B) */
    const float* current_air_time;      /* (N,B) */
    const float* current_contact_time;  /* (N,B) */
    const float* env_origins;           /* (N,3) scene.env_origins */
    const float* ext_reward;            /* (N,next_rew) values of Python-evaluated reward terms, or NULL */
    const uint8_t* ext_term;            /* (N,next_term) */
    const float* ext_obs;               /* (N,next_obs) */
    const float* body_lin_acc_w;        /* (N,NB,3) ArticulationData.body_lin_acc_w */
    const float* command_time_left;     /* (N)   CommandTerm.time_left (managers/command_manager.py:60-61) */
    const int64_t* command_counter;     /* (N)   CommandTerm.command_counter */
    const float* body_pos_w;            /* (N,NB,3) ArticulationData.body_pos_w, or NULL unless a term reads it */
    const float* last_contact_time;     /* (N,B) ContactSensorData.last_contact_time, or NULL unless a term reads it */
    const float* link_incoming_joint_force; /* (N,NB,6) root_physx_view.get_link_incoming_joint_force() (force, torque), or NULL
                                               unless a term reads it */
    const float* body_quat_w;           /* (N,NB,4) ArticulationData.body_quat_w w,x,y,z = body_state_w[..., 3:7] (articulation_data.py:776-782), or NULL
                                           unless a term reads it (orientation_command_error) */
    const float* object_root_pos_w;     /* (N,3) RigidObjectData.root_pos_w of the scene's rigid object ("object"), or NULL unless a term reads
                                           it (the manipulation/lift terms, root_height_below_minimum on the object) */
} imx_state_t;

/* ---- manager state + outputs (caller-owned, persistent across steps) ------------------------------------------ */
typedef struct imx_buffers {
    int64_t* episode_length_buf; /* (N)   envs/manager_based_rl_env.py:200 */
    float* action;               /* (N,A) managers/action_manager.py:318-331 */
    float* prev_action;          /* (N,A) */
    float* processed_action;     /* (N,PA), PA = IMX_H_PA (= A unless a term's processed width differs from its raw width) */
    float* reward_buf;           /* (N)   managers/reward_manager.py:128-157 */
    float* episode_sums;         /* (NREW_ALL,N) */
    float* step_reward;          /* (N,NREW_ALL) */
    uint8_t* term_dones;         /* (NTERM,N) managers/termination_manager.py:151-174 */
    uint8_t* terminated;         /* (N) */
    uint8_t* truncated;          /* (N) */
    uint8_t* reset_buf;          /* (N) */
    int64_t* reset_env_ids;      /* (N) ascending ids of reset envs; valid prefix = counters[0] */
    int32_t* counters;           /* (8) [0] reset count [1] ticket [2] step counter (RNG streams, sensor stamps): imx_terminations_rewards
                                    publishes [3] + 1 there [3] its shadow, written by imx_observations (a step = one of each)
                                    [4],[5] low / high word of the sensor-drift seed (caller-written) [6..] reserved */
    float* log_out;              /* (NREW_ALL + NTERM + 1 + 3) Episode_Reward/<term>, Episode_Termination/<term>, count, then the three
                                    orchestration entries (see ev_part) */
    float* obs;                  /* (N,D_0) first observation group; managers/observation_manager.py:238-335 */
    void* scratch;               /* imx_plan_scratch_bytes(plan, N) bytes */
    float* mod_state;            /* (N, IMX_H_MOD_STATE) DigitalFilter / Integrator state; NULL when the plan has none */
    float* obs_extra1;           /* (N,D_1) second observation group (e.g. "critic"); NULL when the plan has one group */
    float* obs_extra2;           /* (N,D_2) */
    float* obs_extra3;           /* (N,D_3) */
    float* scan_state;           /* (N,8) [timestamp, timestamp_last_update, drift xyz, data.pos_w z, outdated, step stamp] of the
                                    height scanner; required when IMX_H_SCAN_STATEFUL; the caller starts it with zeros and
                                    outdated = 1 (sensors start outdated, sensor_base.py _initialize_impl).  The sensor clock is advanced
                                    where the env's frame row is produced: by imx_terminations_rewards (which knows the step's reset
                                    flags) or, without it, by imx_observations.  The stamp (counters[2] + 1 as uint bits) makes a
                                    second call within one step repeat the first one's decision instead of advancing the clock again */
    float* scan_hit_z;           /* (N,R) data.ray_hits_w[..., 2] kept for envs whose sensor is not outdated at the next step */
    const float* scan_drift_feed;/* optional (N,3): drift values taken at a sensor reset instead of the in-kernel draw (parity runs) */
    float* log_accum;            /* optional (NREW_ALL + NTERM + 1): running sum over the steps of log_out -- the runner's per-iteration
                                    mean of extras["log"] (upstream on_policy_runner.py: ep_infos.append(infos["log"]) every step; the
                                    dict is only REFRESHED on steps that reset something, manager_based_rl_env.py:216, so a step without
                                    resets adds the entries of the last refresh again).  Updated where log_out is (the step tail) */
    const float* ev_part;        /* optional: imx_orch_t.ev_part_d of the imx_reset_orchestrate launch between imx_terminations_rewards and
                                    imx_observations -- the step tail then also writes log_out[NREW_ALL + NTERM + 1 ..]: the two
                                    Metrics/<command>/error_vel_xy|yaw entries (command_manager.py:123-149: means over the reset envs) and
                                    Curriculum/terrain_levels (curriculum_manager.py:95-118: mean level over all envs); needs the deferred
                                    tail (flags bit 0 / enable_corruption bit 4) */
    int64_t ev_flags;            /* bit 0: the metrics entries exist, bit 1: the curriculum entry exists */
    float* term_state;           /* (IMX_H_TERM_SLOTS, N) per-env state of stateful reward terms (progress_reward.potentials), carried
                                    across steps; written by imx_terminations_rewards (the reset branch once the env's reset flag is
                                    known) and imx_term_state_reset.  NULL unless the plan has stateful terms */
} imx_buffers_t;

/* ---- slot t of an rsl_rl RolloutStorage, filled by the step kernel itself (imx_terminations_rewards_rollout) ------------------ */
typedef struct imx_rollout_slot {
    const float* value_t;        /* (N)   critic values of this step (storage.values[t]) -- the time-out bootstrap reads them */
    float* rewards_out;          /* (N)   storage.rewards[t] = reward + gamma * value_t * time_out   (PPO.process_env_step) */
    uint8_t* dones_out;          /* (N)   storage.dones[t] = terminated | time_out                   (vecenv_wrapper.py:178) */
    float* cur_reward_sum;       /* (N)   optional, with cur_ep_len: the runner's running episode return / length ... */
    float* cur_ep_len;           /* (N) */
    float* ep_stats3;            /* (3)   optional: finished episodes {sum return, sum length, count} (float atomics: logging only) */
    float gamma;
    int32_t bootstrap_time_outs; /* 0 for a finite-horizon task (vecenv_wrapper.py:184-185: no "time_outs" key) */
} imx_rollout_slot_t;

/* ---- the reset / interval orchestration around the step (imx_reset_orchestrate) ------------------------------------------------
 * ManagerBasedRLEnv._reset_idx (envs/manager_based_rl_env.py:347-392) for the envs the step reset -- CurriculumManager.compute
 * (terrain_levels_vel + TerrainImporter.update_env_origins), scene.reset (contact sensor, actuator state), EventManager.apply("reset")
 * with min_step_count_between_reset (managers/event_manager.py:233-260), CommandTerm.reset (metrics for the log, resample) -- followed by
 * what ManagerBasedRLEnv.step does next (:232-236): CommandManager.compute(dt) and EventManager.apply("interval", dt) with per-env or
 * global timers re-sampled in the kernel (event_manager.py:205-232).  One lane per env, ONE launch, no host read: the reference walks
 * nonzero() id lists with a host sync per interval term and per manager reset. */
#define IMX_ORCH_MAX_TERMS 8
enum imx_event_op {
    IMX_E_RESET_ROOT_STATE_UNIFORM = 1, /* envs/mdp/events.py:823-868;  ranges: pose lo/hi x 6 [0..11], velocity lo/hi x 6 [12..23] */
    IMX_E_RESET_JOINTS_BY_SCALE,        /* :987-1015;  ranges: position lo, hi, velocity lo, hi */
    IMX_E_RESET_JOINTS_BY_OFFSET,       /* :1020-1049 */
    IMX_E_PUSH_BY_SETTING_VELOCITY,     /* :795-820;   ranges: lo/hi x 6 */
    IMX_E_APPLY_EXTERNAL_FORCE_TORQUE,  /* :764-791;   ranges: force lo, hi, torque lo, hi; body ids */
    IMX_E_RESET_JOINTS_AROUND_DEFAULT,  /* isaaclab_tasks .../velocity/config/spot/mdp/events.py:26-60; ranges as the joint resets: the
                                           default +- range is clamped to the soft limits BEFORE sampling */
    IMX_E_RESET_SCENE_TO_DEFAULT        /* envs/mdp/events.py:1096-1118; no ranges, no draws: default root state (+ env origin) and default
                                           joint state of the robot, default root state of the scene's rigid object (imx_orch_manip_t);
                                           imx_reset_orchestrate_manip only */
};
typedef struct imx_event_term {
    int32_t op;                            /* enum imx_event_op */
    int32_t mode;                          /* 0 = "reset", 1 = "interval" (EventTermCfg.mode) */
    int32_t is_global_time;                /* interval terms: one timer for all envs (event_manager.py:213-221) */
    int32_t min_step_count_between_reset;  /* reset terms (:233-260) */
    float interval_lo, interval_hi;        /* interval_range_s */
    float ranges[24];
    int32_t num_body_ids;
    int32_t asset;                         /* IMX_E_RESET_ROOT_STATE_UNIFORM: whose root state -- 0 the robot (imx_orch_t's default_root_state_d,
                                              root_pose_out_d, root_vel_out_d), 1 the scene's rigid object (imx_orch_manip_t's;
                                              imx_reset_orchestrate_manip only).  0 for every other op */
    const int32_t* body_ids_d;             /* IMX_E_APPLY_EXTERNAL_FORCE_TORQUE: resolved body ids (NULL = all bodies) */
    int32_t* last_triggered_step_d;        /* (N) reset terms: _reset_term_last_triggered_step_id */
    uint8_t* triggered_once_d;             /* (N) reset terms: _reset_term_last_triggered_once */
    float* time_left_d;                    /* interval terms: (N) per-env timers, or (2) for a global timer -- slot [step & 1] is read,
                                              slot [(step + 1) & 1] written (no read-modify-write race across workgroups) */
    const float* uniforms_d;               /* optional (N, width) samples in [0,1) replacing the in-kernel draws (parity runs); width =
                                              12 (root state), 2J (joints), 6 (push), 6 x bodies (wrench: forces first) */
    const float* interval_uniforms_d;      /* optional (N) samples for the timer re-sampling (a global timer takes [0]) */
} imx_event_term_t;

typedef struct imx_orch {
    int64_t num_envs, num_joints, num_bodies;
    const uint8_t* reset_mask_d;           /* (N) imx_buffers.reset_buf of this step; NULL = every env (ManagerBasedEnv.reset) */
    const int32_t* step_counter_d;         /* the global env step count on the device (_sim_step_counter // decimation): buf->counters + 2 */
    uint64_t seed;
    float dt;                              /* step_dt */
    int32_t do_step;                       /* 1: inside step() -- CommandManager.compute + interval events follow the resets; 0: reset() */
    int32_t num_terms;
    int32_t reserved0;
    imx_event_term_t terms[IMX_ORCH_MAX_TERMS];   /* cfg order */
    /* the asset: defaults, limits, the current (post-physics) root state */
    const float* default_root_state_d;     /* (N,13) */
    const float* default_joint_pos_d;      /* (N,J) */
    const float* default_joint_vel_d;
    const float* soft_joint_pos_limits_d;  /* (N,J,2) */
    const float* soft_joint_vel_limits_d;  /* (N,J) */
    const float* root_pos_w_d;             /* (N,3) */
    const float* root_quat_w_d;            /* (N,4) */
    const float* root_lin_vel_w_d;         /* (N,3) */
    const float* root_ang_vel_w_d;         /* (N,3) */
    float* env_origins_d;                  /* (N,3) scene.env_origins: read by the events, updated by the curriculum */
    /* what write_root_pose_to_sim / write_root_velocity_to_sim / write_joint_state_to_sim / set_external_force_and_torque receive */
    float* root_pose_out_d;                /* (N,7) */
    float* root_vel_out_d;                 /* (N,6) */
    float* joint_pos_out_d;                /* (N,J) */
    float* joint_vel_out_d;                /* (N,J) */
    float* ext_force_out_d;                /* (N,NB,3) */
    float* ext_torque_out_d;               /* (N,NB,3) */
    /* CurriculumManager: terrain_levels_vel (isaaclab_tasks/.../velocity/mdp/curriculums.py:26-55); NULL terrain_levels_d = none */
    const float* terrain_origins_d;        /* (R,C,3) */
    const int64_t* terrain_types_d;        /* (N) */
    int64_t* terrain_levels_d;             /* (N) */
    const int64_t* rand_levels_d;          /* optional (N): the randint_like draw (parity runs) */
    int32_t terrain_rows, terrain_cols;
    float terrain_size_x, max_episode_length_s;
    /* CommandManager: has_command = 0: none, 1: UniformVelocityCommand, 2: UniformPoseCommand (its fields are at the struct's end) */
    int32_t has_command, heading_command;
    float command_cfg[16];                 /* as imx_velocity_command's cfg15 */
    float* vel_command_b_d;                /* (N,3) */
    float* heading_target_d;
    uint8_t* is_heading_env_d;
    uint8_t* is_standing_env_d;
    float* command_time_left_d;
    int64_t* command_counter_d;
    float* metric_error_vel_xy_d;
    float* metric_error_vel_yaw_d;
    const float* command_uniforms_d;       /* optional (2,N,7) */
    /* scene.reset(env_ids): ContactSensor.reset (contact_sensor.py:143-165 + sensor_base.py:182-194), ActuatorNetLSTM.reset */
    float* cs_timestamp_d;                 /* NULL: the scene has no env-owned contact sensor */
    float* cs_timestamp_last_update_d;
    uint8_t* cs_is_outdated_d;
    float* cs_net_forces_w_d;              /* (N,B,3) */
    float* cs_net_forces_w_history_d;      /* (N,H,B,3) or NULL */
    float* cs_last_air_time_d;             /* (N,B) or NULL (track_air_time off) */
    float* cs_current_air_time_d;
    float* cs_last_contact_time_d;
    float* cs_current_contact_time_d;
    int32_t cs_num_bodies, cs_history_length;
    float* lstm_hidden_d;                  /* (L, N*J, H) sea_hidden_state or NULL */
    float* lstm_cell_d;
    int32_t lstm_layers, lstm_hidden_dim;
    /* per-workgroup partial sums for the step tail's log entries (imx_buffers.ev_part): {error_vel_xy, error_vel_yaw over the reset
     * envs; terrain levels over all envs; reset count} x ceil(N / 64) */
    float* ev_part_d;
    /* has_command = 2: the command term is a UniformPoseCommand (envs/mdp/commands/pose_command.py:25-127; pose_command_env).  It shares
     * command_time_left_d, command_counter_d, command_uniforms_d and command_cfg (imx_pose_command's cfg16) with the velocity command;
     * metric_error_vel_xy_d / metric_error_vel_yaw_d hold its metrics position_error / orientation_error (the log's first / second
     * command slot, ev_part columns 0 / 1); the body count is num_bodies.  Not combined with the terrain curriculum. */
    float* pose_command_b_d;               /* (N,7) position + w, x, y, z quaternion in the base frame */
    float* pose_command_w_d;               /* (N,7) */
    const float* body_pos_w_d;             /* (N,NB,3) of the current (post-physics) state */
    const float* body_quat_w_d;            /* (N,NB,4) */
    int32_t pose_body_idx;                 /* robot.find_bodies(cfg.body_name)[0][0] */
    int32_t make_quat_unique;
} imx_orch_t;
/* number of floats of ev_part for num_envs */
size_t imx_orch_part_floats(int64_t num_envs);
int imx_reset_orchestrate(const imx_orch_t* orch, imx_stream_t stream);

/* ---- the manipulation tasks' part of _reset_idx (Isaac-Lift-Cube-Franka-v0, Isaac-Reach-*): imx_reset_orchestrate_manip -------
 * imx_orch_t does not grow for it: what these tasks add travels in imx_orch_manip_t (imx_orch_manip.h, which this header includes).
 *   - reset_scene_to_default (envs/mdp/events.py:1096-1118) and reset_root_state_uniform (:823-868) on the scene's one RigidObject
 *     (imx_event_term_t.asset = 1) write the object's own "to simulator" buffers;
 *   - modify_reward_weight (envs/mdp/curriculums.py:21-36: `if env.common_step_counter > num_steps: set_term_cfg(weight)`), evaluated
 *     where the reference evaluates it -- CurriculumManager.compute inside _reset_idx (envs/manager_based_rl_env.py:347-392), that is
 *     only in a launch that resets at least one env -- by a plain store of the new weight into the term's IMX_R_WEIGHT word of the
 *     device-resident reward table (imx_plan_reward_weight_ptr).  *step_counter_d is common_step_counter at that point (the step
 *     kernel has published this step's count; after ManagerBasedEnv.reset it is the last step's).  The next imx_terminations_rewards
 *     launch reads the new weight (stream order).  Every workgroup with a reset env stores the same value: idempotent.
 * The same launch otherwise does what imx_reset_orchestrate does; has_command is 0 or 2 (a pose command), no terrain curriculum. */
typedef struct imx_orch_manip imx_orch_manip_t;
#include "imx_orch_manip.h" /* IMX_ORCH_MAX_WEIGHT_TERMS, imx_weight_term_t and the definition of imx_orch_manip_t */
int imx_reset_orchestrate_manip(const imx_orch_t* orch, const imx_orch_manip_t* manip, imx_stream_t stream);

/* ---- _reset_idx on a scene with a second articulation (Isaac-Open-Drawer-Franka-v0: the cabinet): imx_reset_orchestrate_scene ---
 * What imx_reset_orchestrate_manip does, plus the second articulation (imx_orch_articulation.h, which this header includes;
 * imx_event_term_t.asset = 2): reset_scene_to_default (envs/mdp/events.py:1096-1118) also writes its default root pose (+ env origin),
 * root velocity and joint state, unclamped; reset_joints_by_offset / reset_joints_by_scale (:987-1049) on it draw 2 * J2 columns keyed
 * as the robot's are and clamp to ITS soft position limits and +- velocity limits; reset_root_state_uniform (:823-868) on it writes its
 * root pose and velocity.  All four go to the asset's own out buffers.  The limit tables are required only when a joint event acts on
 * the asset.  Any other op with asset = 2 is refused, and so is a term with asset = 2 handed to imx_reset_orchestrate[_manip]. */
typedef struct imx_orch_articulation imx_orch_articulation_t;
#include "imx_orch_articulation.h" /* the definition of imx_orch_articulation_t */
int imx_reset_orchestrate_scene(const imx_orch_t* orch, const imx_orch_manip_t* manip, const imx_orch_articulation_t* articulation,
                                imx_stream_t stream);

/* ---- the pose-2d command term (Isaac-Navigation-Flat-Anymal-C-v0): imx_pose2d_command, imx_reset_orchestrate_pose2d -------------
 * UniformPose2dCommand (isaaclab/envs/mdp/commands/pose_2d_command.py:26-143) and TerrainBasedPose2dCommand (:146-203) under
 * CommandTerm.reset / compute (isaaclab/managers/command_manager.py:120-187), one lane per env (pose2d_command_env).  The term travels
 * in imx_pose2d_command_t (imx_pose2d_struct.h, which this header includes): its cfg, the terrain's valid targets, the optional parity
 * draws and its state / output buffers.
 *   imx_pose2d_command: reset(the envs of reset_mask_d; NULL = none) and then, with do_compute, compute(dt), on the root pose given.
 *     In-kernel draws are keyed by (seed, column, *step_counter_d (NULL = 0), env).
 *   imx_reset_orchestrate_pose2d: what imx_reset_orchestrate does -- scene.reset, the reset events, the command term's reset and
 *     compute in their place (envs/manager_based_rl_env.py:347-392, :215-236), the interval events -- with this term as the command
 *     term.  imx_orch_t does not grow for it and orch->has_command must be 0; the sums of error_pos_2d / error_heading over the reset
 *     envs leave in ev_part columns 0 / 1.  No terrain curriculum (orch->terrain_levels_d must be NULL).
 * Every NULL pointer or out-of-range value is refused and named in imx_last_error before any launch. */
typedef struct imx_pose2d_command imx_pose2d_command_t;
#include "imx_pose2d_struct.h" /* the definition of imx_pose2d_command_t */
int imx_pose2d_command(int64_t N, const imx_pose2d_command_t* cmd, float dt, int do_compute, const float* root_pos_w_d,
                       const float* root_quat_w_d, const uint8_t* reset_mask_d, uint64_t seed, const int32_t* step_counter_d,
                       imx_stream_t stream);
int imx_reset_orchestrate_pose2d(const imx_orch_t* orch, const imx_pose2d_command_t* cmd, imx_stream_t stream);

/* ---- the in-hand re-orientation command term (Isaac-Repose-Cube-Allegro-v0): imx_inhand_command ---------------------------------
 * InHandReOrientationCommand (isaaclab_tasks .../manipulation/inhand/mdp/commands/orientation_command.py:22-124) under
 * CommandTerm.reset / compute (isaaclab/managers/command_manager.py:120-187), one lane per env.  The term travels in
 * imx_inhand_command_t (imx_inhand_command_struct.h, which this header includes): its cfg, the fixed goal position, the object's root
 * pose, the reset mask, the optional parity draws, the seed and its state / output buffers.
 *   One launch: CommandTerm.reset on the envs of term->reset_mask_d (NULL = none) -- the metrics of those envs are summed for the log
 *   first (term->log_part_d), then zeroed, command_counter = 0, resample -- and then, with flags bit 0, CommandTerm.compute(dt):
 *   _update_metrics, time_left -= dt with a resample where it ran out, _update_command (a resample where the goal was reached).
 * STAND-ALONE: no orchestration launch runs this term yet and imx_orch_t does not grow for it.
 * Every NULL pointer or out-of-range value is refused and named in imx_last_error before any launch. */
typedef struct imx_inhand_command imx_inhand_command_t;
#include "imx_inhand_command_struct.h" /* the definition of imx_inhand_command_t */
int imx_inhand_command(const imx_inhand_command_t* term, int64_t N, float dt, int flags, imx_stream_t stream);

/* ---- the in-hand task's further per-step tensors: imx_object_state_t, imx_plan_bind_object_state -------------------------------
 * The rest of the rigid object's root state (object_root_quat_w, object_root_lin_vel_w, object_root_ang_vel_w) and the command term's
 * consecutive_success metric (imx_object_state.h, which this header includes).  imx_state_t does not grow for them: the caller binds
 * the struct to the plan, and imx_terminations_rewards[_rollout] / imx_observations on that plan read the pointers bound at the time
 * of the call (host side: a captured graph keeps what was bound when its launch was recorded).  os = NULL unbinds.  The struct is
 * copied: it need not outlive the call. */
typedef struct imx_object_state imx_object_state_t;
#include "imx_object_state.h" /* the definition of imx_object_state_t */
int imx_plan_bind_object_state(imx_plan_t* plan, const imx_object_state_t* os);

/* ---- the scene's second articulation (Isaac-Open-Drawer-Franka-v0: the cabinet): imx_articulation_state_t ----------------------
 * Its joint state and body poses (imx_articulation_state.h, which this header includes), bound to the plan like the object state:
 * imx_terminations_rewards[_rollout] / imx_observations read the pointers bound at the time of the call; as = NULL unbinds; the
 * struct is copied.  A launch whose plan reads a tensor that is NULL names it in imx_last_error and launches nothing. */
typedef struct imx_articulation_state imx_articulation_state_t;
#include "imx_articulation_state.h" /* the definition of imx_articulation_state_t */
int imx_plan_bind_articulation_state(imx_plan_t* plan, const imx_articulation_state_t* as);

/* ---- FrameTransformer (sensors/frame_transformer/frame_transformer.py:337-384): imx_frame_transformer -----------------------------
 * One launch fills the six FrameTransformerData tensors from the body poses of ONE articulation: the source frame and num_targets
 * target frames, each combine_frame_transforms(body pose, offset) (utils/math.py:750-781: quat_apply, then add; quat_mul), and every
 * target relative to the source (subtract_frame_transforms :785-816, quat_inv = normalised conjugate).  frames_d: (1 + num_targets) x
 * IMX_FRAME_WORDS device words, the source first, in the form of the plan's frame table (the asset word is not read: every body id
 * indexes body_pos_w / body_quat_w (N, num_bodies, 3 | 4)).  Lane = (env, target frame).  Outputs: source_pos_w (N,3), source_quat_w
 * (N,4), target_pos_w (N,T,3), target_quat_w (N,T,4), target_pos_source (N,T,3), target_quat_source (N,T,4).  frames_h: the same
 * words on the host, for the range check of the body ids before the launch. */
int imx_frame_transformer(int64_t N, int num_targets, int num_bodies, const float* body_pos_w_d, const float* body_quat_w_d,
                          const int32_t* frames_d, const int32_t* frames_h, float* source_pos_w_d, float* source_quat_w_d,
                          float* target_pos_w_d, float* target_quat_w_d, float* target_pos_source_d, float* target_quat_source_d,
                          imx_stream_t stream);

/* ---- RayCaster (sensors/ray_caster/ray_caster.py, sensors/sensor_base.py): imx_ray_caster ---------------------------------------
 * One launch, one block per env, for a sensor with any ray pattern and the full orientation of the body it sits on.  The sensor
 * travels in imx_ray_caster_t (imx_ray_caster_struct.h, which this header includes).  Per env, in the reference's order: reset (the envs
 * of reset_mask_d: clocks to zero, outdated, a new drift), the clocks (substeps times timestamp += dt, outdated once the update period
 * has passed), and with `refresh` the cast for the outdated envs only -- pos_w = body_pos + drift, quat_w, ray_hits_w (+inf on a miss)
 * and the optional range image and world rays; the other envs keep what they had.  The rays go through the z-pruned grid walk of
 * csrc/imx_ray_walk.h, whose hit is the closest one of ALL triangles with t in [0, max_distance], bit for bit what imx_raycast gives.
 *   imx_mesh_build_ray_bounds: the walk's z-bounds (8 bytes per grid cell and per 8x8 tile), built once per mesh on the device from the
 *   cell records, reference lists and triangle records; synchronises and allocates, so not inside a stream capture.  imx_ray_caster
 *   builds them itself on a mesh that has none (same restriction for that first call).  info4 (may be NULL) = bytes of the bounds, build
 *   time in nanoseconds (host clock around the build, 0 when they existed), grid cells, tiles.
 * Every NULL pointer or out-of-range value is refused and named in imx_last_error before any launch. */
typedef struct imx_ray_caster imx_ray_caster_t;
#include "imx_ray_caster_struct.h" /* the definition of imx_ray_caster_t */
int imx_mesh_build_ray_bounds(imx_mesh_t* mesh, imx_stream_t stream, int64_t* info4);
int imx_ray_caster(const imx_ray_caster_t* sensor, int64_t N, imx_mesh_t* mesh, imx_stream_t stream);

/* ---- Imu (sensors/imu/imu.py, sensors/sensor_base.py): imx_imu, imx_plan_bind_imu ------------------------------------------------
 * One launch for 1..IMX_MAX_IMU sensors, lane = (sensor, env).  A sensor travels in imx_imu_t (imx_imu_struct.h, which this header
 * includes).  Per env, in the reference's order: reset (the envs of reset_mask_d: clocks to zero, outdated, quat_w and the four
 * body-frame vectors to zero; pos_w and the previous velocities stay), the clocks (substeps times timestamp += dt, outdated once the
 * update period has passed), and with `refresh` _update_buffers_impl for the outdated envs only: pos_w, quat_w (offset included), the
 * linear velocity carried from the centre of mass to the sensor, both accelerations as (v - previous v) / dt with dt the value of
 * this call (Imu._dt: the dt of the last update, not the time since the last refresh), and the four vectors rotated into the sensor's
 * frame; the other envs keep what they had.  The velocity inputs are never written.  No host synchronisation: capturable.
 *   imx_plan_bind_imu: the sensors' data tensors for the IMX_O_IMU_* observation ops of `plan`, by sensor index (the record's aux0);
 *   like imx_plan_bind_object_state the pointers are read at the time of an imx_observations call.  num_sensors = 0 unbinds.
 * Every NULL pointer or out-of-range value is refused and named in imx_last_error before any launch. */
#define IMX_MAX_IMU 4
typedef struct imx_imu imx_imu_t;
#include "imx_imu_struct.h" /* the definition of imx_imu_t */
int imx_imu(const imx_imu_t* sensors, int32_t num_sensors, int64_t N, imx_stream_t stream);
int imx_plan_bind_imu(imx_plan_t* plan, const imx_imu_t* sensors, int32_t num_sensors);

/* ---- library ---------------------------------------------------------------------------------------------------- */
const char* imx_version(void);
/* sizeof of an ABI struct as this library was compiled (which: 0 imx_state_t, 1 imx_buffers_t, 2 imx_head_loss_t, 3 imx_rollout_slot_t, 4 imx_policy_act_t, 5 imx_orch_t, 6 imx_event_term_t,
 * 7 imx_diff_ik_t, 8 imx_osc_t, 10 imx_orch_manip_t, 11 imx_weight_term_t, 12 imx_pretrained_policy_t,
 * 13 imx_pose2d_command_t, 15 imx_inhand_command_t, 16 imx_object_state_t, 18 imx_articulation_state_t,
 * 20 imx_orch_articulation_t, 22 imx_norm_group_t, 23 imx_infer_norm_t, 25 imx_ray_caster_t, 27 imx_imu_t), 0 for an unknown index
 * (9, 14, 17, 19, 21, 24 and 26 are):
 * a binding checks its own layout against it at load time. */
size_t imx_struct_size(int which);
const char* imx_last_error(void);
int imx_device_count(void);

/* term compiler output -> device tables.  Replaces ManagerBase._prepare_terms (managers/manager_base.py:160). */
int imx_plan_create(const int32_t* blob, size_t nwords, imx_plan_t** out);
void imx_plan_destroy(imx_plan_t* plan);
/* RewardManager.set_term_cfg / TerminationManager.set_term_cfg (managers/reward_manager.py:163-176,
 * managers/termination_manager.py:207-220; used by envs/mdp/curriculums.py:20-37 modify_reward_weight): replace the tables of
 * `plan` IN PLACE by a recompiled blob of the same shape (same term counts, widths and table sizes -- a changed weight, threshold,
 * id list of equal length ...).  The copy is enqueued on `stream`; graphs that captured launches on `plan` stay valid. */
int imx_plan_update(imx_plan_t* plan, const int32_t* blob, size_t nwords, imx_stream_t stream);
/* Device address of reward term `reward_term_index`'s IMX_R_WEIGHT word (an f32; cfg order, as RewardManager.active_terms,
 * managers/reward_manager.py:163-176) in the plan's device tables: what imx_orch_manip_t.weight_terms[].weight_d points at, and what a
 * host reads back before it recompiles the tables (imx_plan_update would otherwise restore the weight of its blob).  The address is
 * stable for the plan's lifetime (imx_plan_update copies in place). */
int imx_plan_reward_weight_ptr(const imx_plan_t* plan, int reward_term_index, float** out);
/* The f32 that word holds now, after everything enqueued on `stream` so far: waits for the stream (a host sync -- for set_term_cfg /
 * get_term_cfg, never for the step or rollout path). */
int imx_plan_reward_weight_get(const imx_plan_t* plan, int reward_term_index, imx_stream_t stream, float* out);
size_t imx_plan_scratch_bytes(const imx_plan_t* plan, int64_t num_envs);
int imx_plan_obs_dim(const imx_plan_t* plan);

/* ActionManager.process_action (managers/action_manager.py:318-337) + JointAction.process_actions
 * (envs/mdp/actions/joint_actions.py:130-139); pre_clip = RslRlVecEnvWrapper clip_actions
 * (isaaclab_rl/rsl_rl/vecenv_wrapper.py:173-174) or +inf. */
int imx_action_process(const imx_plan_t* plan, int64_t num_envs, const float* actions_d, float pre_clip,
                       const imx_state_t* state, const imx_buffers_t* buf, imx_stream_t stream);

/* Post-physics, pre-reset half of ManagerBasedRLEnv.step (envs/manager_based_rl_env.py:200-230):
 * episode_length_buf += 1; TerminationManager.compute; RewardManager.compute(dt); reset_env_ids = nonzero(reset_buf);
 * the manager-side part of _reset_idx (:347-392): Episode_* log reductions, episode sums / actions / episode length
 * zeroed for reset envs.
 * flags bit 0: leave the end of the step -- reset_env_ids, the reset count (counters[0]) and the Episode_* entries of log_out,
 * which need every env group's partial results -- to the imx_observations call that follows on the same stream (its
 * enable_corruption bit 4): a kernel boundary then orders them instead of a fence + ticket inside this launch.  Masks, rewards,
 * episodic sums and the reset of manager state are complete either way.
 * With state->root_pos_w present the launch also leaves the per-env frame rows (body-frame velocities, projected gravity, the
 * height scanner's update decision: SensorBase.update / reset, sensors/sensor_base.py:182-205) imx_observations reads when called
 * with enable_corruption bit 2. */
int imx_terminations_rewards(const imx_plan_t* plan, int64_t num_envs, const imx_state_t* state,
                             const imx_buffers_t* buf, int flags, imx_stream_t stream);
/* The same launch also doing what imx_rollout_post does (RslRlVecEnvWrapper.step dones, PPO.process_env_step time-out bootstrap, the
 * runner's episode statistics) for slot t of the storage: the lanes that produce reward and masks write them there too -- one launch
 * and one pass over the masks less per rollout step.  Bit-identical to imx_terminations_rewards followed by imx_rollout_post.
 * slot == NULL: plain imx_terminations_rewards.  (The log accumulation of imx_rollout_post is buf->log_accum.) */
int imx_terminations_rewards_rollout(const imx_plan_t* plan, int64_t num_envs, const imx_state_t* state, const imx_buffers_t* buf,
                                     int flags, const imx_rollout_slot_t* slot, imx_stream_t stream);

/* ObservationManager.compute (managers/observation_manager.py:238-335) fused with RayCaster._update_buffers_impl
 * (sensors/ray_caster/ray_caster.py:220-260) + raycast_mesh (utils/warp/ops.py:24-127).
 * noise_u_d: optional (N,D) uniform [0,1) samples replacing torch.rand_like (parity mode); NULL -> in-kernel
 * counter-based RNG keyed by (seed, step counter, env, column).  ray_hits_out_d: optional (N,R,3).
 * Terms with ObservationTermCfg.history_length > 0 keep their flattened (H, d) window (oldest first; CircularBuffer,
 * utils/buffers/circular_buffer.py:107-135) in the obs row itself: envs flagged in buf->reset_buf -- or every env when bit 1
 * of enable_corruption is set (env.reset()) -- take the new value in every slot, the others slide by one.  * enable_corruption bit 2 (value 4): the per-env frame table (root-frame vectors, scanner yaw) is current -- imx_terminations_rewards was
 * called with root_pos_w on the SAME state tensors since they last changed and wrote it -- so the k_frame launch is skipped.
 * enable_corruption bit 4 (value 16): finish the step tail a preceding imx_terminations_rewards (flags bit 0) deferred.
 * enable_corruption bit 3 (value 8): with a stateful height scanner, keep the hit heights of EVERY env in scan_hit_z, not only of
 * those whose fp32 timestamps say they will skip the next update (a caller that is about to overwrite the timestamps in scan_state). */
int imx_observations(const imx_plan_t* plan, int64_t num_envs, const imx_state_t* state, const imx_buffers_t* buf,
                     const imx_mesh_t* mesh, const float* noise_u_d, uint64_t seed, int enable_corruption,
                     float* ray_hits_out_d, imx_stream_t stream);
/* Name of the kernel imx_observations launches for this plan ("k_obs_lean<false>", "k_obs<false,true>", ...): benchmarks and
 * profiles attribute their timings to the kernel that actually ran.  Static string. */
const char* imx_observations_kernel_name(const imx_plan_t* plan);
/* The reset(env_ids) of the plan's stateful reward terms (RewardManager.reset -> ManagerTermBase.reset, reward_manager.py:100-126):
 * progress_reward.potentials = -||target - root_pos_w|| / step_dt over all three components (classic/humanoid/mdp/rewards.py:54-63),
 * the same device function as the reset branch of imx_terminations_rewards.  mask_d: optional (N) uint8, NULL = every env.  Reads
 * state->root_pos_w; a no-op for a plan without stateful terms. */
int imx_term_state_reset(const imx_plan_t* plan, int64_t num_envs, const imx_state_t* state, const imx_buffers_t* buf,
                         const uint8_t* mask_d, imx_stream_t stream);

/* ArticulationData.root_lin_vel_b / root_ang_vel_b / projected_gravity_b
 * (assets/articulation/articulation_data.py:512-515,603-619) = quat_rotate_inverse (utils/math.py:605-625). */
int imx_root_frame(int64_t num_envs, const float* quat_wxyz_d, const float* lin_vel_w_d, const float* ang_vel_w_d,
                   float gx, float gy, float gz, float* lin_vel_b_d, float* ang_vel_b_d, float* proj_gravity_d,
                   imx_stream_t stream);

/* convert_to_warp_mesh (utils/warp/ops.py:130-145): host vertices/triangles -> device mesh + grid. cell<=0: auto */
int imx_mesh_create(const float* vertices_h, int64_t num_vertices, const uint32_t* triangles_h, int64_t num_triangles,
                    float cell_size, imx_mesh_t** out);
void imx_mesh_destroy(imx_mesh_t* mesh);
/* info[0..7] = nx, ny, num_triangles, general triangle records, max refs per cell (low 32 bits) | FLAT cells (high 32 bits),
 * lattice cells, general cells (FLAT ones included), cell size (float bits) */
int imx_mesh_info(const imx_mesh_t* mesh, int64_t* info8);

/* raycast_mesh (utils/warp/ops.py:24-127): closest hit per ray, misses = +inf / face -1. */
int imx_raycast(const imx_mesh_t* mesh, const float* ray_starts_d, const float* ray_dirs_d, int64_t num_rays,
                float max_dist, float* ray_hits_d, float* ray_distance_d, int32_t* ray_face_id_d,
                imx_stream_t stream);

/* rsl_rl (3rd-party, v2.3.1) RolloutStorage.compute_returns: GAE backward scan over (T,N) + advantage
 * normalisation over all T*N.  scratch_d: >= imx_gae_scratch_bytes(T,N).  PARITY UNPINNED (rsl_rl absent). */
size_t imx_gae_scratch_bytes(int64_t T, int64_t N);
int imx_gae(int64_t T, int64_t N, const float* rewards_d, const float* values_d, const uint8_t* dones_d,
            const float* last_values_d, float gamma, float lam, int normalize, float* returns_d,
            float* advantages_d, void* scratch_d, imx_stream_t stream);

/* rsl_rl PPO.update elementwise part: surrogate / clipped value / entropy losses and the KL estimate for a
 * minibatch of M samples with A action dims.  sigma_stride = A for a per-sample (M,A) std, 0 for the shared (A) std
 * parameter.  fwd writes out8 = {surrogate_loss, value_loss, entropy_mean, kl_mean, loss, -, -, -} with
 * loss = surrogate + value_loss_coef*value_loss - entropy_coef*entropy, and (optional) accum5 += {value_loss,
 * surrogate, entropy, kl, 1}; bwd writes grad_scale * d(loss)/d(mu), /d(sigma) (per sample, (M,A)), /d(value); the policy
 * part (dmu_d, dsigma_d) and the value part (dvalue_d) are independent: pass NULL for one to launch them separately
 * (actor and critic then run forward -> loss gradient -> backward on their own streams without meeting).
 * PARITY UNPINNED (rsl_rl absent). */
size_t imx_ppo_scratch_bytes(int64_t M);
int imx_ppo_loss_fwd(int64_t M, int64_t A, const float* mu_d, const float* sigma_d, int64_t sigma_stride,
                     const float* actions_d, const float* old_logp_d, const float* old_mu_d, const float* old_sigma_d,
                     const float* advantages_d, const float* returns_d, const float* values_d, const float* old_values_d,
                     float clip_param, int use_clipped_value_loss, float value_loss_coef, float entropy_coef,
                     float* out8_d, float* accum5_d, void* scratch_d, imx_stream_t stream);
int imx_ppo_loss_bwd(int64_t M, int64_t A, const float* mu_d, const float* sigma_d, int64_t sigma_stride,
                     const float* actions_d, const float* old_logp_d, const float* advantages_d, const float* returns_d,
                     const float* values_d, const float* old_values_d, float clip_param, int use_clipped_value_loss,
                     float value_loss_coef, float entropy_coef, float grad_scale, float* dmu_d, float* dsigma_d,
                     float* dvalue_d, imx_stream_t stream);

/* out[c] = sum_m x[m][c] * (y ? y[m][c] : 1), x / y (M,A) row-major, A <= 64: the action-noise gradient from the per-sample
 * dsigma (``std.grad = dsigma.sum(0)``, or ``(dsigma * sigma).sum(0)`` for the log-std parametrisation of rsl_rl's ActorCritic).
 * Two launches, fixed summation order.  scratch_d: imx_colsum_scratch_bytes() bytes. */
size_t imx_colsum_scratch_bytes(void);
int imx_colsum(int64_t M, int64_t A, const float* x_d, const float* y_d, float* out_d, void* scratch_d, imx_stream_t stream);

/* torch.nn.utils.clip_grad_norm_ + torch.optim.Adam.step (as used by rsl_rl PPO.update) on one flat fp32 bucket.
 * lr_d / grad_norm_d are DEVICE scalars (adaptive-KL learning rate, ||g||_2); grad_norm_d NULL = no clipping.
 * step = 1-based Adam step count. */
int imx_adam_step(int64_t n, float* param_d, const float* grad_d, float* exp_avg_d, float* exp_avg_sq_d,
                  const float* lr_d, const float* grad_norm_d, float max_norm, float beta1, float beta2, float eps,
                  int64_t step, imx_stream_t stream);

/* The same with the whole schedule on the device (capturable in a hipGraph): state8_d = {lr, step, beta1^t, beta2^t,
 * clip coef, lr/bias1, sqrt(bias2), -}.  A one-thread kernel applies rsl_rl's adaptive-KL rule to lr when kl_d != NULL
 * (lr /= 1.5 if kl > 2*desired_kl; lr *= 1.5 if 0 < kl < desired_kl/2; bounds [1e-5, 1e-2]), advances the Adam step
 * and derives the clip coefficient from grad_norm_d; a second kernel applies Adam to the bucket. */
int imx_adam_update(int64_t n, float* param_d, const float* grad_d, float* exp_avg_d, float* exp_avg_sq_d, float* state8_d,
                    const float* kl_d, float desired_kl, const float* grad_norm_d, float max_norm, float beta1,
                    float beta2, float eps, imx_stream_t stream);

/* Same, with clip_grad_norm_'s total norm computed inside (one launch does the norm reduction, the adaptive-KL rule and
 * the step bookkeeping; state8[7] receives the norm).  max_norm <= 0 disables clipping.  scratch_d:
 * imx_adam_norm_scratch_bytes(n) bytes, ZERO-filled once by the caller (the kernel re-arms its ticket). */
size_t imx_adam_norm_scratch_bytes(int64_t n);
int imx_adam_update_norm(int64_t n, float* param_d, const float* grad_d, float* exp_avg_d, float* exp_avg_sq_d, float* state8_d,
                         const float* kl_d, float desired_kl, float max_norm, float beta1, float beta2, float eps,
                         void* scratch_d, size_t scratch_bytes, imx_stream_t stream);

/* rsl_rl RolloutStorage.mini_batch_generator: dst[k][r, :] = src[k][idx[r], :] for n <= 12 fp32 arrays of
 * width_floats[k] columns, one launch.  src_d / dst_d / width_floats are HOST arrays of device pointers / widths. */
int imx_gather_rows(int64_t M, const int64_t* idx_d, int n, const void* const* src_d, void* const* dst_d,
                    const int32_t* width_floats, imx_stream_t stream);
/* The same with a row pitch per destination array (floats, >= width; NULL = packed): a minibatch buffer whose rows start on 16-byte
 * boundaries lets imx_mlp_dw read it with 16-byte loads when the observation width is not a multiple of four (235, 310). */
int imx_gather_rows_pitched(int64_t M, const int64_t* idx_d, int n, const void* const* src_d, void* const* dst_d,
                            const int32_t* width_floats, const int32_t* dst_pitch_floats, imx_stream_t stream);

/* rsl_rl PPO.act after the actor / critic GEMMs: sample a = mu + std*N(0,1) (counter-based in-kernel generator keyed by
 * seed and *step_counter_d), log-prob, and the transition written into slot t of the RolloutStorage (obs, actions,
 * log-prob, mu, sigma, value); actions_env_d (optional) receives a second copy for env.step.  PARITY UNPINNED. */
int imx_policy_act(int64_t N, int64_t A, int64_t D, const float* mu_d, const float* std_d, const float* value_d,
                   const float* obs_d, uint64_t seed, const int32_t* step_counter_d, float* actions_out_d,
                   float* logp_out_d, float* mu_out_d, float* sigma_out_d, float* values_out_d, float* obs_out_d,
                   float* actions_env_d, imx_stream_t stream);

/* RslRlVecEnvWrapper.step dones (isaaclab_rl/rsl_rl/vecenv_wrapper.py:178) + rsl_rl PPO.process_env_step time-out
 * bootstrap (rewards += gamma * values * time_outs) + the runner's episode statistics, into slot t of the storage.
 * log_accum_d (optional, num_log floats) += log_in_d: the per-step extras["log"] entries (imx_buffers.log_out,
 * envs/manager_based_rl_env.py:365-389) summed on the device for the runner's per-iteration ep_infos mean. */
int imx_rollout_post(int64_t N, const float* reward_d, const uint8_t* terminated_d, const uint8_t* truncated_d,
                     const float* value_t_d, float gamma, int bootstrap_time_outs, float* rewards_out_d,
                     uint8_t* dones_out_d, int64_t* dones_long_d, float* cur_reward_sum_d, float* cur_ep_len_d,
                     float* ep_stats3_d, const float* log_in_d, float* log_accum_d, int num_log, imx_stream_t stream);

/* ---- input producers -------------------------------------------------------------------- */

/* SensorBase.update + ContactSensor._update_buffers_impl (sensors/sensor_base.py:196-205,287-297;
 * sensors/contact_sensor/contact_sensor.py:320-379): timestamp += dt; for outdated envs (flag set or
 * timestamp - last_update + 1e-6 >= update_period): net_forces_w <- new forces (N,B,3), history shifted by one
 * ((N,H,B,3), H may be 0), air/contact-time state machine with elapsed = timestamp - last_update; stamps updated. */
int imx_contact_sensor_update(int64_t N, int64_t B, int64_t H, const float* new_net_forces_d, float dt, float update_period,
                              float force_threshold, int track_air_time, float* timestamp_d,
                              float* timestamp_last_update_d, uint8_t* is_outdated_d, float* net_forces_w_d,
                              float* net_forces_w_history_d, float* last_air_time_d, float* current_air_time_d,
                              float* last_contact_time_d, float* current_contact_time_d, imx_stream_t stream);

/* CommandTerm.reset (for envs flagged in reset_mask_d, may be NULL) followed -- when do_compute != 0 -- by
 * CommandTerm.compute(dt) of
 * UniformVelocityCommand (managers/command_manager.py:119-187, envs/mdp/commands/velocity_command.py:111-160).
 * cfg15 (HOST floats) = {resampling_time lo,hi, lin_vel_x lo,hi, lin_vel_y lo,hi, ang_vel_z lo,hi, heading lo,hi,
 * rel_standing_envs, rel_heading_envs, heading_control_stiffness, resampling_time_range[1]/step_dt, -}.
 * uniforms_d: optional (2,N,7) samples in [0,1) {time_left, lin_x, lin_y, ang_z, heading, is_heading, is_standing} for
 * the first / second resampling of an env within this call (parity mode); NULL -> counter-based in-kernel generator. */
int imx_velocity_command(int64_t N, const float* cfg15, int heading_command, float dt, int do_compute,
                         const float* root_quat_w_d,
                         const float* root_lin_vel_w_d, const float* root_ang_vel_w_d, const uint8_t* reset_mask_d,
                         const float* uniforms_d, uint64_t seed, const int32_t* step_counter_d, float* vel_command_b_d,
                         float* heading_target_d, uint8_t* is_heading_env_d, uint8_t* is_standing_env_d,
                         float* time_left_d, int64_t* command_counter_d, float* metric_error_vel_xy_d,
                         float* metric_error_vel_yaw_d, imx_stream_t stream);

/* The same two steps for UniformPoseCommand (managers/command_manager.py:120-187, envs/mdp/commands/pose_command.py:25-127):
 * CommandTerm.reset for the envs flagged in reset_mask_d (may be NULL), then -- when do_compute != 0 -- CommandTerm.compute(dt):
 * _update_metrics (pose_command_w = combine_frame_transforms(root pose, pose_command_b), utils/math.py:750-781; position_error /
 * orientation_error = norms of compute_pose_error(..., "axis_angle"), :820-867, against body body_idx of body_pos_w_d (N,NB,3) /
 * body_quat_w_d (N,NB,4) -- ASSIGNED, not accumulated), time_left -= dt, resampling where time_left <= 0 (six uniform draws, then
 * quat_from_euler_xyz :252-278 and, with make_quat_unique, quat_unique :448-460).
 * cfg16 (HOST floats) = {resampling_time lo,hi, pos_x lo,hi, pos_y lo,hi, pos_z lo,hi, roll lo,hi, pitch lo,hi, yaw lo,hi, -, -}.
 * uniforms_d: optional (2,N,7) samples in [0,1) {time_left, pos_x, pos_y, pos_z, roll, pitch, yaw} for the first / second resampling
 * of an env within this call (parity mode); NULL -> counter-based in-kernel generator.  pose_command_b_d / pose_command_w_d: (N,7)
 * position + w, x, y, z quaternion.  Refused: a null state tensor, body_idx outside [0, num_bodies), resampling_time hi <= 0. */
int imx_pose_command(int64_t N, const float* cfg16, int make_quat_unique, int64_t body_idx, int64_t num_bodies, float dt,
                     int do_compute, const float* root_pos_w_d, const float* root_quat_w_d, const float* body_pos_w_d,
                     const float* body_quat_w_d, const uint8_t* reset_mask_d, const float* uniforms_d, uint64_t seed,
                     const int32_t* step_counter_d, float* pose_command_b_d, float* pose_command_w_d, float* time_left_d,
                     int64_t* command_counter_d, float* metric_position_error_d, float* metric_orientation_error_d,
                     imx_stream_t stream);

/* ArticulationData.root_state_w + joint_acc (assets/articulation/articulation_data.py:365-380,546-556): split PhysX's
 * root transforms (N,7: pos, quat XYZW) / velocities (N,6) into root_pos_w, root_quat_w (WXYZ, convert_quat
 * utils/math.py:177-222), root_lin_vel_w, root_ang_vel_w; joint_acc = (dof_vel - previous)/time_elapsed, previous <-
 * dof_vel (pass joint_acc_d = NULL to skip).  SURVEY 8f row 4. */
int imx_articulation_update(int64_t N, int64_t J, const float* root_transforms_xyzw_d, const float* root_velocities_d,
                            const float* dof_velocities_d, float time_elapsed, float* root_pos_w_d, float* root_quat_w_d,
                            float* root_lin_vel_w_d, float* root_ang_vel_w_d, float* previous_joint_vel_d,
                            float* joint_acc_d, imx_stream_t stream);

/* IdealPDActuator / ImplicitActuator (dc_motor = 0) and DCMotor (dc_motor = 1) .compute (actuators/actuator_pd.py:115-145,
 * 184-199, 264-286): computed = kp (q_des - q) + kd (qd_des - qd) + ff, applied = computed clipped to +-effort_limit or, for
 * the DC motor, to the velocity-dependent window built from saturation_effort and velocity_limit.  All arrays (N,J);
 * joint_vel_target_d / effort_ff_d may be NULL (zeros).  SURVEY 8f row 4. */
int imx_actuator_pd(int64_t N, int64_t J, int dc_motor, float saturation_effort, const float* joint_pos_target_d,
                    const float* joint_vel_target_d, const float* effort_ff_d, const float* joint_pos_d, const float* joint_vel_d,
                    const float* stiffness_d, const float* damping_d, const float* effort_limit_d, const float* velocity_limit_d,
                    float* computed_effort_d, float* applied_effort_d, imx_stream_t stream);

/* DelayedPDActuator / RemotizedPDActuator .compute (actuators/actuator_pd.py:289-412; DelayBuffer utils/buffers/delay_buffer.py,
 * CircularBuffer utils/buffers/circular_buffer.py).  ring_d: (max_delay+1, N, 3, J) f32, caller-owned, persistent; `step` = number of
 * calls so far (host counter, replaces the reference's pointer); reset_step_d[e] = the `step` of env e's first call after its last
 * reset (the caller sets it, with the new time_lags_d[e] in [min_delay, max_delay], when it resets the env); effort_limit_d NULL =
 * no box limit; lookup_d (num_lookup,3) = angle / transmission ratio / max torque samples, ascending angles, or NULL. */
int imx_actuator_delayed_pd(int64_t N, int64_t J, int max_delay, int64_t step, const int32_t* time_lags_d,
                            const int64_t* reset_step_d, float* ring_d, const float* joint_pos_target_d,
                            const float* joint_vel_target_d, const float* effort_ff_d, const float* joint_pos_d,
                            const float* joint_vel_d, const float* stiffness_d, const float* damping_d,
                            const float* effort_limit_d, const float* lookup_d, int num_lookup, float* computed_effort_d,
                            float* applied_effort_d, imx_stream_t stream);

/* ActuatorNetLSTM.compute (actuators/actuator_net.py:72-104; ANYDRIVE_3_LSTM_ACTUATOR_CFG, isaaclab_assets/robots/anymal.py:45-51,
 * is the actuator of ANYmal-B/C): network input (pos target - pos, vel) per (env, joint) sample, LSTM stack, dense head, the
 * DC-motor clip of the torque (DCMotor._clip_effort, actuators/actuator_pd.py:276-286).  The network travels as one packed float
 * array: per LSTM layer W_ih (4H x in), W_hh (4H x H), b_ih (4H), b_hh (4H) (torch's gate order i, f, g, o; in = 2 for the first
 * layer, H after), then per dense layer W (out x in), b (out); dense_out_h[k] = width of dense layer k (the last must be 1);
 * act = activation BETWEEN dense layers (0 identity, 1 softsign, 2 tanh, 3 relu, 4 elu).  hidden_state_d / cell_state_d:
 * (num_lstm, N*J, H), the reference's sea_hidden_state / sea_cell_state, updated in place (the caller zeroes rows at reset, :65-69).
 * All other arrays (N,J).  SURVEY 8f row 4. */
int imx_actuator_net_lstm(int64_t N, int64_t J, int num_lstm, int hidden, int num_dense, const int32_t* dense_out_h, int act,
                          const float* weights_d, int64_t num_weights, const float* joint_pos_target_d, const float* joint_pos_d,
                          const float* joint_vel_d, float* hidden_state_d, float* cell_state_d, float saturation_effort,
                          const float* effort_limit_d, const float* velocity_limit_d, float* computed_effort_d,
                          float* applied_effort_d, imx_stream_t stream);

/* ActuatorNetMLP.compute (actuators/actuator_net.py:160-195): the position-error and velocity queues (N, history_length, J) are
 * rolled by one and topped up in place; the sample of (env, joint) is the entries input_idx_d[0..num_idx) of both queues, scaled
 * by pos_scale / vel_scale, position block first (vel_first = 0, "pos_vel") or second ("vel_pos"); dense network as above (packed
 * W, b per layer; first width 2 * num_idx); torque * torque_scale, then the DC-motor clip. */
int imx_actuator_net_mlp(int64_t N, int64_t J, int num_dense, const int32_t* dense_out_h, int act, const float* weights_d,
                         int64_t num_weights, int history_length, const int32_t* input_idx_d, int num_idx, float pos_scale,
                         float vel_scale, float torque_scale, int vel_first, const float* joint_pos_target_d,
                         const float* joint_pos_d, const float* joint_vel_d, float* pos_error_history_d, float* vel_history_d,
                         float saturation_effort, const float* effort_limit_d, const float* velocity_limit_d,
                         float* computed_effort_d, float* applied_effort_d, imx_stream_t stream);

/* rsl_rl EmpiricalNormalization.forward (3rd party v2.3.1, absent): if update != 0 fold the batch (N,D) into the running
 * mean / variance (count (int64, like upstream's long buffer), mean, var, std are device buffers; Chan's update with the biased
 * batch variance, rate = N / (count + N) from the exact count), then out = (x - mean) / (std + eps).  PARITY UNPINNED.
 * SURVEY 8f row 3. */
int imx_empirical_normalization(int64_t N, int64_t D, const float* x_d, int update, float eps, float* mean_d, float* var_d,
                                float* std_d, int64_t* count_d, float* out_d, imx_stream_t stream);

/* The statistics half of EmpiricalNormalization.forward alone, for one or two normalisers in TWO wide launches (the fused rollout:
 * the rows are normalised where they are read, imx_mlp_infer_act2n).  Launch A: row slabs x 64-column blocks of every group in one grid,
 * each workgroup leaves its slab's (mean, M2) per column in partials_d (two-pass within the slab, the four waves merged in a fixed
 * order; no atomics).  Launch B: one workgroup per group merges the slabs in slab order (Chan), applies the running update of
 * imx_empirical_normalization (rate from the exact integer count) and, after a workgroup barrier, stores count + N.  Both launches read
 * count_d on the device and do nothing when until >= 0 && count >= until (upstream's `until` gate without a host round trip: a captured
 * rollout keeps it).  Results depend on (N, D, ldx) only. */
typedef struct imx_norm_group imx_norm_group_t;
typedef struct imx_infer_norm imx_infer_norm_t;
#include "imx_normalization_struct.h" /* the definitions of imx_norm_group_t (struct-size index 22) and imx_infer_norm_t (23) */
size_t imx_empirical_normalization_partials_bytes(int64_t N, int64_t D);
/* groups: HOST array of ngroups (1 or 2) entries.  A refused argument is named in imx_last_error and nothing is launched. */
int imx_empirical_normalization_update(int ngroups, const imx_norm_group_t* groups, imx_stream_t stream);

/* ---- actor / critic MLP inside PPO.update (rsl_rl v2.3.1 ppo.py::update `loss.backward()` through the nn.Linear / nn.ELU
 * stacks of actor_critic.py; 3rd party, absent: PARITY UNPINNED, checked against torch autograd).  fp32 on the f32 MFMA.
 * The wide forward / dX GEMMs stay library calls; these are the shapes a library GEMM handles badly. */

/* Bytes of scratch imx_mlp_dw / imx_mlp_head_bwd need for a layer (out_features x in_features) at M samples. */
size_t imx_mlp_scratch_bytes(int64_t M, int out_features, int in_features);

/* nn.Linear backward, parameter part: dW[N][K] = dY^T X and (db_d != NULL) db[N] = column sums of dY, for
 * dY (M,N; row pitch ldy floats) and the layer input X (M,K; pitch ldx).  Split over the M samples across all CUs,
 * partials summed in a fixed order (deterministic). */
int imx_mlp_dw(int64_t M, int N, int K, const float* dY_d, int64_t ldy, const float* X_d, int64_t ldx, float* dW_d,
               float* db_d, void* scratch_d, size_t scratch_bytes, imx_stream_t stream);

/* Deferred reductions: imx_mlp_dw / imx_mlp_dw_elu / imx_mlp_head_bwd end with a small kernel that sums their split partials
 * into dW / db.  Between imx_reduce_batch_begin(b) and imx_reduce_batch_flush(b, stream), calls issued from the SAME host
 * thread queue that step on `b` instead (at most 8) and flush launches one kernel for all of them: dW / db are only needed
 * by the optimiser, so the backward chain loses a 6 us launch per layer.  Every deferred call needs its OWN scratch.
 * A batch empties at flush (not at begin): imx_mlp_head_fwd_bwd(..., defer_to = b, ...) may queue on it before it is opened. */
typedef struct imx_reduce_batch imx_reduce_batch_t;
int imx_reduce_batch_create(imx_reduce_batch_t** out);
void imx_reduce_batch_destroy(imx_reduce_batch_t* batch);
/* How many workgroups (one per CU) an imx_mlp_dw / imx_mlp_dw_elu launch may split its samples over; 0 = every CU (the default).  The PPO
 * update runs actor and critic backward passes on two streams at once: with half the chip each (128) the two launches stop competing for
 * the same CUs and the split partials (written, then re-read by the reduction) halve.  Returns the previous value.  Scratch sized
 * (imx_mlp_scratch_bytes) under a budget is valid for any budget <= that one. */
int imx_mlp_set_dw_cu_budget(int cus);
int imx_reduce_batch_begin(imx_reduce_batch_t* batch);
int imx_reduce_batch_flush(imx_reduce_batch_t* batch, imx_stream_t stream);
/* Ends the open batch WITHOUT launching: what it holds stays queued, the host thread is free to open another network's batch, and a
 * later begin + flush (or further defer_to = batch calls before that) launches everything in one kernel. */
int imx_reduce_batch_end(imx_reduce_batch_t* batch);

/* Same with the ELU backward of this layer fused in: dH_d is the gradient w.r.t. the layer's ACTIVATED output h = ELU(z),
 * H_d that saved output; dZ = dH * (h > 0 ? 1 : h + elu_alpha) (aten elu_backward with is_result) is formed on the way
 * into LDS -- no separate elementwise pass -- and written to dZ_out_d (M,N; may be NULL when no layer below needs it; must
 * not alias dH_d); dW = dZ^T X, db = colsum(dZ). */
int imx_mlp_dw_elu(int64_t M, int N, int K, const float* dH_d, int64_t ldg, const float* H_d, int64_t ldh, float elu_alpha,
                   float* dZ_out_d, int64_t ldd, const float* X_d, int64_t ldx, float* dW_d, float* db_d, void* scratch_d,
                   size_t scratch_bytes, imx_stream_t stream);

/* imx_mlp_dw_elu on a workgroup tile of 128 out-features x 256 in-features, for a layer with 128 < K <= 256 (anything else is refused):
 * one tile column, so the ELU' of a dH / H tile is formed once instead of once per 128-wide column tile.  Meant for the first layers of
 * actor and critic stacked into one launch when both read the same X: H_d is the stacked saved output (M, N; pitch ldh) and the
 * incoming gradient arrives as n_seg (1..4) column segments -- dH_seg_d is a HOST array of device pointers, segment i holds columns
 * [i * seg_cols, (i + 1) * seg_cols) of dH with the common pitch ldg; seg_cols a multiple of 128 when n_seg > 1 -- so the dX GEMMs
 * of the two networks need no copy.  dW (N, K) and db are bit-identical to imx_mlp_dw_elu run on every segment's rows of the layer
 * whenever both plan the same sample split (N / n_seg a multiple of 128 rows per segment).  No dZ output.  The reduction is queued
 * on defer_to (may be a batch that is not open on this thread) or, when NULL, launched now.  Scratch: imx_mlp_dw_wide_scratch_bytes. */
size_t imx_mlp_dw_wide_scratch_bytes(int64_t M, int out_features, int in_features);
int imx_mlp_dw_elu_wide(int64_t M, int N, int K, int n_seg, const float* const* dH_seg_d, int seg_cols, int64_t ldg, const float* H_d,
                        int64_t ldh, float elu_alpha, const float* X_d, int64_t ldx, float* dW_d, float* db_d, void* scratch_d,
                        size_t scratch_bytes, imx_reduce_batch_t* defer_to, imx_stream_t stream);

/* Rollout inference (rsl_rl actor_critic.py::act / evaluate): the whole Linear+ELU stack of up to two
 * networks sharing the input X (M, dims[0]; pitch ldx) in ONE launch, 32 samples per workgroup, activations in LDS.
 * nlayers[k] <= 4 Linear layers per network, ELU(elu_alpha[k]) after every layer but the last; dims = the layer widths of
 * network 0 (nlayers[0]+1 values, each <= 512) followed by those of network 1; weights_d / biases_d = HOST arrays of device
 * pointers, network 0's layers first; W (out,in) row-major with row pitch weight_pitch[i] floats (NULL = dense), which must
 * be a multiple of 32 with ZERO padding and 16-byte aligned rows -- a 235-wide first layer is passed as a padded copy
 * (pitch 256) -- so that every weight load is an unconditional 16-byte load; out_d[k] (M, last width). */
int imx_mlp_infer(int64_t M, const float* X_d, int64_t ldx, int nnets, const int* nlayers, const int* dims,
                  const float* const* weights_d, const int* weight_pitch, const float* const* biases_d, const float* elu_alpha,
                  float* const* out_d, imx_stream_t stream);

/* PPO.act (imx_policy_act) and ActionManager.process_action (imx_action_process) in the epilogue of the actor head of imx_mlp_infer:
 * the actor's workgroups keep their action means in LDS, sample a = mu + std * N(0,1) with the draws imx_policy_act makes (same seed,
 * step counter and element index), write the transition {obs, actions, log-prob, mu, sigma} into slot t of the RolloutStorage and -- when
 * `plan` is given -- run the sampled action through the env's action terms (buf->prev_action <- action <- clamp(a, pre_clip),
 * buf->processed_action: managers/action_manager.py:318-337, envs/mdp/actions/joint_actions.py:130-139).  All of it is pre-physics, so
 * it is valid with a simulator in the loop as well.  The critic's value goes where out_d[1] points (storage.values[t]).  Three launches
 * (k_mlp_infer, k_policy_act, k_action) become one; results are bit-identical to the three. */
typedef struct imx_policy_act {
    const float* std_d;            /* (A) action std (scalar noise_std_type) */
    uint64_t seed;
    const int32_t* step_counter_d; /* device step counter keying the draws (buf->counters + 2), or NULL */
    float* actions_out_d;          /* (N,A) storage.actions[t] */
    float* logp_out_d;             /* (N)   storage.actions_log_prob[t] */
    float* mu_out_d;               /* (N,A) storage.mu[t] */
    float* sigma_out_d;            /* (N,A) storage.sigma[t] */
    float* obs_out_d;              /* (N,D) storage.observations[t] (dense rows) */
    const imx_plan_t* plan;        /* optional: also process the action (with state, buf, pre_clip) */
    const imx_state_t* state;
    const imx_buffers_t* buf;
    float pre_clip;                /* RslRlVecEnvWrapper clip_actions or +inf */
} imx_policy_act_t;
/* out_d[0] may be NULL when act != NULL (the means go to mu_out_d); act == NULL: plain imx_mlp_infer.
 * packed_weights_d (optional, HOST array of device pointers like weights_d): the same weights re-ordered by imx_mlp_pack_weights.  In
 * the row layout a wave's load instruction reads 16 bytes from each of 32 weight rows; the packed image holds those 64 x 16 bytes
 * contiguously, in the order the 32-sample kernel consumes them, so every load is one full KiB.  Same values, same arithmetic, same
 * results; weights_d must still be given (the 16-sample kernel for small M reads the rows). */
int imx_mlp_infer_act(int64_t M, const float* X_d, int64_t ldx, int nnets, const int* nlayers, const int* dims,
                      const float* const* weights_d, const int* weight_pitch, const float* const* packed_weights_d,
                      const float* const* biases_d, const float* elu_alpha, float* const* out_d, const imx_policy_act_t* act,
                      imx_stream_t stream);
/* The same launch for networks that do NOT share their input: an env with a privileged ("critic") observation group, where the actor
 * reads the policy group and the critic its own.  X_d and ldx are HOST arrays of nnets entries: network k reads X_d[k] (M, width_k; pitch
 * ldx[k] >= width_k), width_k = the first of its dims, and the widths may differ.  critic_obs_out_d (optional, nnets == 2 only): network
 * 1's workgroups also store their input rows densely there, (M, width_1) -- storage.privileged_observations[t] -- on the way into LDS, as
 * the actor's workgroups do for act->obs_out_d.  act == NULL and critic_obs_out_d == NULL: plain inference.  Everything else is
 * imx_mlp_infer_act's: limits, weight layout, the rule between 16- and 32-row tiles, and -- on equal inputs -- its results, bit for bit.
 * A refused argument is named in imx_last_error and nothing is launched. */
int imx_mlp_infer_act2(int64_t M, const float* const* X_d, const int64_t* ldx, int nnets, const int* nlayers, const int* dims,
                       const float* const* weights_d, const int* weight_pitch, const float* const* packed_weights_d,
                       const float* const* biases_d, const float* elu_alpha, float* const* out_d, const imx_policy_act_t* act,
                       float* critic_obs_out_d, imx_stream_t stream);
/* imx_mlp_infer_act2 that normalises its input rows where it loads them (EmpiricalNormalization in the fused rollout): every element of
 * network k's rows becomes (x - mean_d[c]) / (std_d[c] + eps) -- the expression of imx_empirical_normalization, a true division -- before
 * it goes to LDS and to act->obs_out_d / critic_obs_out_d, so outputs and stored rows are bit-identical to an apply launch followed by
 * imx_mlp_infer_act2.  norm: HOST array of nnets entries; an entry whose mean_d and std_d are both NULL leaves that network's rows as
 * they are.  An env without a critic group passes the policy rows and the policy statistics for both networks. */
int imx_mlp_infer_act2n(int64_t M, const float* const* X_d, const int64_t* ldx, int nnets, const int* nlayers, const int* dims,
                        const float* const* weights_d, const int* weight_pitch, const float* const* packed_weights_d,
                        const float* const* biases_d, const float* elu_alpha, float* const* out_d, const imx_policy_act_t* act,
                        float* critic_obs_out_d, const imx_infer_norm_t* norm, imx_stream_t stream);
/* Floats of the packed image of an (out_features x in_features) nn.Linear weight (both rounded up to multiples of 32), and the packing
 * itself (W_d row-major with row pitch ldw >= in_features; packed_d 16-byte aligned; to be repeated whenever the weights change). */
size_t imx_mlp_packed_floats(int out_features, int in_features);
int imx_mlp_pack_weights(int out_features, int in_features, const float* W_d, int64_t ldw, float* packed_d, imx_stream_t stream);
/* The same for up to 8 layers in ONE launch (HOST arrays of nlayers entries): the refresh after an optimiser step. */
int imx_mlp_pack_weights_batch(int nlayers, const int* out_features, const int* in_features, const float* const* W_d, const int64_t* ldw,
                               float* const* packed_d, imx_stream_t stream);

/* First-layer forward of the update with the activation fused: Y (M,N; pitch ldy) = ELU(X W^T + b) (apply_elu = 0: no activation),
 * X (M,K; pitch ldx), W (N,K) dense row-major, K <= 256 (the observation width: 235, 48, 4 ...).  A library GEMM + a separate ELU pass
 * writes, reads and writes the output again.  Each wave keeps the weight rows of its 32 output columns in registers, the samples stream
 * through LDS in tiles of 32 rows (LDS DMA for K > 128 with 16-byte aligned rows), bias + ELU are applied to the accumulators.  fp32
 * products accumulated in fp32 (v_mfma_f32_32x32x2_f32; inputs k and NS + k paired per step, NS = the kernel's step count: another
 * summation order than a library GEMM's, same error class).  nn.Linear + nn.ELU of rsl_rl's ActorCritic MLPs (upstream
 * rsl_rl/modules/actor_critic.py). */
int imx_mlp_fwd_elu(int64_t M, int N, int K, const float* X_d, int64_t ldx, const float* W_d, const float* b_d, float elu_alpha,
                    int apply_elu, float* Y_d, int64_t ldy, imx_stream_t stream);

/* Output layer forward, A <= 64 outputs (action means / value): y[M][A] = h W^T + b, h (M,K; pitch ldh), W (A,K).
 * elu_in_place != 0: h_d holds the PRE-activation output of the layer below; h <- ELU(h) (aten elu, alpha = elu_alpha) is
 * applied on the way in and written back in place, so that layer needs no separate activation pass. */
int imx_mlp_head_fwd(int64_t M, int K, int A, float* h_d, int64_t ldh, const float* W_d, const float* b_d, float* y_d,
                     int elu_in_place, float elu_alpha, imx_stream_t stream);

/* imx_mlp_head_fwd followed by imx_ppo_loss_bwd in ONE launch: the lane that holds a sample's outputs computes the loss gradient
 * from them right away (policy head: mode 1 -> dmu_d, dsigma_d from mu = y; value head, A = 1: mode 2 -> dvalue_d from value = y).
 * Same arithmetic, same order as k_ppo_bwd (bit-identical gradients); saves a dependent launch on the update's critical chain. */
typedef struct imx_head_loss {
    int mode;                  /* 1 policy gradient, 2 value gradient */
    int sigma_stride;          /* 0 (shared std) or A */
    int use_clipped_value_loss;
    float clip_param, value_loss_coef, entropy_coef, grad_scale;
    const float* sigma_d;      /* mode 1 */
    const float* actions_d;
    const float* old_logp_d;
    const float* advantages_d;
    const float* returns_d;    /* mode 2 */
    const float* old_values_d;
    float* dmu_d;              /* mode 1 outputs (M,A) */
    float* dsigma_d;
    float* dvalue_d;           /* mode 2 output (M,1) */
} imx_head_loss_t;
int imx_mlp_head_fwd_loss(int64_t M, int K, int A, float* h_d, int64_t ldh, const float* W_d, const float* b_d, float* y_d,
                          int elu_in_place, float elu_alpha, const imx_head_loss_t* loss, imx_stream_t stream);

/* Output layer backward in one pass over h: dW[A][K] = dY^T h, db[A] = colsum(dY), and the gradient handed to the layer
 * below, dprev[M][K] = (dY W) * ELU'(h) with ELU' taken from the saved output h (h > 0 ? 1 : h + elu_alpha; aten
 * elu_backward with is_result) when has_activation != 0, else dprev = dY W. */
int imx_mlp_head_bwd(int64_t M, int K, int A, const float* dY_d, const float* h_d, int64_t ldh, const float* W_d, float elu_alpha,
                     int has_activation, float* dprev_d, float* dW_d, float* db_d, void* scratch_d, size_t scratch_bytes,
                     imx_stream_t stream);

/* imx_mlp_head_fwd_loss and imx_mlp_head_bwd in one pass over the last hidden layer's output z (M,K; pitch ldz; K = 128 or 256, A <= 16):
 * h = ELU(z) when elu_in != 0 (else h = z), y = h W^T + b, the loss gradient dY from y (loss->mode 1 or 2, written to loss->dmu_d /
 * dsigma_d / dvalue_d as imx_mlp_head_fwd_loss does), dprev = (dY W) * ELU'(h), dW = dY^T h, db = colsum(dY).  z is only read: the
 * activated values never travel to memory (the split pair wrote them in place and read them again).  defer_to: a reduce batch to
 * queue the reduction of the split partials on (NULL: the batch open on this thread, or an immediate launch). */
int imx_mlp_head_fwd_bwd(int64_t M, int K, int A, const float* z_d, int64_t ldz, const float* W_d, const float* b_d, float* y_d,
                         int elu_in, float elu_alpha, const imx_head_loss_t* loss, float* dprev_d, float* dW_d, float* db_d,
                         void* scratch_d, size_t scratch_bytes, imx_reduce_batch_t* defer_to, imx_stream_t stream);

/* ---- reset / interval events and terrain curriculum, masked: only rows with mask != 0 are rewritten
 * (mask NULL = every env).  The reference runs these on a compacted env_ids list (EventManager.apply,
 * managers/event_manager.py:150-273); draws are sample_uniform (utils/math.py:1313) = u*(hi-lo)+lo with u from the
 * counter-based generator (seed, *step_counter_d, env, column) or from uniforms_d in parity runs. */

/* reset_root_state_uniform (envs/mdp/events.py:823-868) and reset_joints_by_scale / _by_offset (:987-1049).
 * ranges28 (HOST) = pose {x,y,z,roll,pitch,yaw} (lo,hi) x6, velocity (lo,hi) x6, joint position lo,hi, joint velocity lo,hi.
 * joint_mode 0 = by scale, 1 = by offset, 2 = around default (reset_joints_around_default: default + range clamped to the
 * soft limits, then sampled), < 0 = joints untouched.  default_root_state (N,13: pos, quat wxyz, lin, ang),
 * soft_joint_pos_limits (N,J,2), soft_joint_vel_limits (N,J).  uniforms_d: optional (N, 12 + 2J) = [pose 6 | velocity 6 |
 * joint pos J | joint vel J].  Outputs = what write_root_pose_to_sim (N,7), write_root_velocity_to_sim (N,6) and
 * write_joint_state_to_sim (N,J)x2 receive. */
int imx_reset_events(int64_t N, int64_t J, const uint8_t* reset_mask_d, const float* ranges28, int joint_mode,
                     const float* default_root_state_d, const float* env_origins_d, const float* default_joint_pos_d,
                     const float* default_joint_vel_d, const float* soft_joint_pos_limits_d, const float* soft_joint_vel_limits_d,
                     const float* uniforms_d, uint64_t seed, const int32_t* step_counter_d, float* root_pose_d, float* root_vel_d,
                     float* joint_pos_d, float* joint_vel_d, imx_stream_t stream);

/* push_by_setting_velocity (events.py:795-820): root_vel_w (N,6) += sample; ranges12 (HOST) = (lo,hi) x6; uniforms_d (N,6). */
int imx_push_velocity(int64_t N, const uint8_t* mask_d, const float* ranges12, const float* uniforms_d, uint64_t seed,
                      const int32_t* step_counter_d, float* root_vel_w_d, imx_stream_t stream);

/* apply_external_force_torque (events.py:764-791): forces / torques ~ U(range) for bodies body_ids_d[0..num_ids) (device int32;
 * NULL = all num_bodies) of the masked envs, written into the (N, num_bodies, 3) buffers set_external_force_and_torque fills.
 * ranges4 (HOST) = force lo,hi, torque lo,hi; uniforms_d: optional (2, N, nb, 3), forces first. */
int imx_external_force_torque(int64_t N, int64_t num_bodies, const uint8_t* mask_d, const int32_t* body_ids_d, int64_t num_ids,
                              const float* ranges4, const float* uniforms_d, uint64_t seed, const int32_t* step_counter_d,
                              float* forces_d, float* torques_d, imx_stream_t stream);

/* terrain_levels_vel (isaaclab_tasks/.../velocity/mdp/curriculums.py:26-55) + TerrainImporter.update_env_origins
 * (terrains/terrain_importer.py:307-326): move up when the robot walked more than half a tile, down when less than half
 * the commanded distance; levels past the last are replaced by rand_levels_d[e] (randint_like; NULL -> in-kernel draw);
 * env_origins <- terrain_origins[level, type] (num_levels, num_types, 3); mean_level_d (optional) <- mean level. */
int imx_terrain_levels(int64_t N, int64_t num_levels, int64_t num_types, const uint8_t* mask_d, const float* root_pos_w_d,
                       const float* command_d, const float* terrain_origins_d, const int64_t* terrain_types_d, float terrain_size_x,
                       float max_episode_length_s, const int64_t* rand_levels_d, uint64_t seed, const int32_t* step_counter_d,
                       int64_t* terrain_levels_d, float* env_origins_d, float* mean_level_d, imx_stream_t stream);

/* ---- DifferentialInverseKinematicsAction ----------------------------------------------------------------------
 * Parameters of one term (envs/mdp/actions/task_space_actions.py:53-121, controllers/differential_ik_cfg.py:60-70), resolved by
 * isaaclab_amd/plan.py (plan.ik_terms).  Kept out of the plan blob and of imx_state_t / imx_buffers_t / imx_orch_t. */
#define IMX_IK_MAX_JOINTS 8
enum imx_ik_command { IMX_IK_POSITION = 0, IMX_IK_POSE = 1 };
enum imx_ik_method { IMX_IK_DLS = 0, IMX_IK_TRANS = 1 };
typedef struct imx_diff_ik {
    int32_t command_type;      /* imx_ik_command: processed width 3, or 6 (relative) / 7 (absolute) */
    int32_t use_relative_mode;
    int32_t ik_method;         /* imx_ik_method */
    int32_t has_offset;        /* cfg.body_offset is not None */
    float lambda_val;          /* dls, default 0.01 */
    float k_val;               /* trans, default 1.0 */
    float offset_pos[3];
    float offset_rot[4];       /* w, x, y, z */
    int32_t body_idx;          /* row of body_pos_w / body_quat_w */
    int32_t jacobi_body_idx;   /* row of the Jacobian tensor: body_idx - 1 for a fixed base (:72-77) */
    int32_t num_joints;        /* 1 .. IMX_IK_MAX_JOINTS */
    int32_t joint_ids[IMX_IK_MAX_JOINTS];        /* columns of joint_pos */
    int32_t jacobi_joint_ids[IMX_IK_MAX_JOINTS]; /* columns of the Jacobian: joint_ids (+ 6 for a floating base) */
    int32_t processed_col;     /* first column of the term in the (N, PA) processed action */
} imx_diff_ik_t;

/* DifferentialInverseKinematicsAction.process_actions / apply_actions (envs/mdp/actions/task_space_actions.py:155-179, 188-229) with
 * DifferentialIKController.set_command / compute (controllers/differential_ik.py:98-146, 148-240), one lane per env, one launch.
 * mode bit 1: the command half of process_actions -- ee_pos_des / ee_quat_des from the term's processed columns and the current
 *   end-effector pose (_compute_frame_pose :188-207; apply_delta_pose utils/math.py:873-910);
 * mode bit 2: apply_actions (:168-179) -- jacobian_b (:142-149), _compute_frame_jacobian (:209-229), compute_pose_error (utils/math.py:
 *   820-867, "axis_angle"), then dls (J^T (J J^T + lambda^2 I)^-1 dx, solved by a Cholesky factorisation: no inverse is formed) or trans
 *   (k J^T dx), joint_pos_des = joint_pos[joint_ids] + dq.  mode 3 does both.
 * The reference's global test `ee_quat_curr.norm() != 0` (:173), one host sync that is false only before the simulation has produced a
 * pose, is NOT reproduced: the kernel always computes.
 * processed_action_d (N, PA); root_pos_w_d (N,3), root_quat_w_d (N,4); body_pos_w_d (N, num_bodies, 3), body_quat_w_d (N, num_bodies, 4);
 * jacobians_d (N, NB, 6, ND) as root_physx_view.get_jacobians() hands them out, world frame; joint_pos_d (N, J);
 * ee_pos_des_d (N,3), ee_quat_des_d (N,4); joint_pos_des_d (N, ld_des) with the term's num_joints columns first.
 * Refused without a launch: a null pointer the mode needs, num_joints outside [1, 8], a body, joint or column index out of range,
 * processed columns past PA, ld_des < num_joints, an unknown command type / method / mode. */
int imx_diff_ik(const imx_diff_ik_t* cfg, int64_t N, int mode, const float* processed_action_d, int64_t PA,
                const float* root_pos_w_d, const float* root_quat_w_d, const float* body_pos_w_d, const float* body_quat_w_d,
                int64_t num_bodies, const float* jacobians_d, int64_t NB, int64_t ND, const float* joint_pos_d, int64_t J,
                float* ee_pos_des_d, float* ee_quat_des_d, float* joint_pos_des_d, int64_t ld_des, imx_stream_t stream);

/* ---- OperationalSpaceControllerAction --------------------------------------------------------------------------
 * Parameters of one term (envs/mdp/actions/task_space_actions.py:248-378 __init__, :504-537 _resolve_command_indexes, :539-566
 * _resolve_nullspace_joint_pos_targets; controllers/operational_space.py:34-140 __init__, :146-160 action_dim and the defaults of
 * operational_space_cfg.py), resolved by isaaclab_amd/plan.py (plan.osc_terms).  Kept out of the plan blob and of imx_state_t /
 * imx_buffers_t / imx_orch_t.  Only the identity task frame is built (task_frame_rel_path is refused by the term compiler), so the
 * task-frame gains, selection matrices and targets are the root-frame ones. */
#define IMX_OSC_CMD_WIDTH 25
enum imx_osc_pose { IMX_OSC_POSE_ABS = 0, IMX_OSC_POSE_REL = 1 };
enum imx_osc_impedance { IMX_OSC_FIXED = 0, IMX_OSC_VARIABLE_KP = 1, IMX_OSC_VARIABLE = 2 };
enum imx_osc_decoupling { IMX_OSC_DECOUPLING_NONE = 0, IMX_OSC_DECOUPLING_FULL = 1, IMX_OSC_DECOUPLING_PARTIAL = 2 };
/* The struct itself is in imx_osc_struct.h, which this header includes: imx.h declares the type and the entry point. */
typedef struct imx_osc imx_osc_t;
#include "imx_osc_struct.h"

/* OperationalSpaceControllerAction.process_actions / apply_actions (envs/mdp/actions/task_space_actions.py:416-438, :440-462; reset
 * :464-474 zeroes raw actions only and is the env's) with OperationalSpaceController.set_command / compute
 * (controllers/operational_space.py:173-343, :345-548), one lane per env, one launch.  The raw -> processed half (_preprocess_actions
 * :664-700) is an ordinary action record of the plan.
 * mode bit 1: the command half of process_actions -- the end-effector pose in the root frame (_compute_ee_pose :597-615), the term's
 *   processed columns split into target, stiffness and damping ratio and clamped as set_command does, Kp = S_motion diag(stiffness),
 *   Kd = 2 sqrt(Kp) ratio, the desired pose (apply_delta_pose for pose_rel, the seven values as they are for pose_abs: not normalised),
 *   the desired wrench.  Written to the env's row of command_state_d: pose 7, Kp 6, Kd 6, wrench 6 (IMX_OSC_CMD_WIDTH).
 * mode bit 2: apply_actions -- jacobian_b (:403-410) with the offset correction (_compute_ee_jacobian :576-595), the pose and the velocity
 *   relative to the root (_compute_ee_velocity :617-634), _compute_dynamic_quantities (:568-574: mass matrix and gravity indexed by
 *   joint_ids), _compute_joint_states (:645-649), the axis-angle pose error, a = Kp e - Kd v, Lambda = (J M^-1 J^T)^-1 (whole, two 3 x 3
 *   blocks, or none), tau = J^T S_m Lambda a + J^T S_f F + g + (I - J^T Lambda J M^-1) M (kp_n (q* - q) - kd_n qd).  M and J M^-1 J^T
 *   are factored by an unrolled Cholesky and solved, no inverse is formed; only the lower triangle of M is read; the null-space term is
 *   M qdd - J^T Lambda (J qdd).  mode 3 does both.
 * processed_action_d (N, PA); root_pos_w_d (N,3), root_quat_w_d (N,4), root_lin_vel_w_d / root_ang_vel_w_d (N,3); body_pos_w_d,
 * body_lin_vel_w_d, body_ang_vel_w_d (N, num_bodies, 3), body_quat_w_d (N, num_bodies, 4); jacobians_d (N, NB, 6, ND), mass_matrices_d
 * (N, NM, NM), gravity_d (N, NM) as root_physx_view hands them out; joint_pos_d, joint_vel_d (N, J); nullspace_target_d (N, num_joints);
 * command_state_d (N, ld_cmd); joint_efforts_d (N, ld_eff) with the term's num_joints columns first.
 * Refused without a launch: a null pointer the mode and cfg need, num_joints outside [1, 8], a body, joint, row or column index out of
 * range, processed columns past PA, ld_cmd < 25, ld_eff < num_joints, null-space control without full decoupling or on six joints or
 * fewer, an unknown pose type / impedance mode / decoupling / mode. */
int imx_osc(const imx_osc_t* cfg, int64_t N, int mode, const float* processed_action_d, int64_t PA,
            const float* root_pos_w_d, const float* root_quat_w_d, const float* root_lin_vel_w_d, const float* root_ang_vel_w_d,
            const float* body_pos_w_d, const float* body_quat_w_d, const float* body_lin_vel_w_d, const float* body_ang_vel_w_d,
            int64_t num_bodies, const float* jacobians_d, int64_t NB, int64_t ND, const float* mass_matrices_d, const float* gravity_d,
            int64_t NM, const float* joint_pos_d, const float* joint_vel_d, int64_t J, const float* nullspace_target_d,
            float* command_state_d, int64_t ld_cmd, float* joint_efforts_d, int64_t ld_eff, imx_stream_t stream);

/* ---- PreTrainedPolicyAction -------------------------------------------------------------------------------------------
 * One low-level locomotion step of the term (isaaclab_tasks .../navigation/mdp/pre_trained_policy_action.py:93-100) for all envs in
 * ONE launch: the masked zero of the last_action() closure (:53-57), the low-level observation group, the policy MLP and the
 * low-level JointPositionAction.process_actions.
 * ll_plan: the low-level observation group and the low-level action term compiled as a plan of their own (isaaclab_amd/plan.py,
 *   plan.policy_terms): one observation group without history, modifiers, height scan or Python-evaluated term; its D = dims[0] of
 *   the policy, its A = dims[nlayers].  Its generated_commands op reads st->command (the env points it at the term's raw action, CMD
 *   columns), its last_action op reads bf->action = low_level_actions (N, A).
 * Per workgroup of tile_rows (16 or 32; 0 = the choice imx_mlp_infer makes for one network at this N) envs: the root-frame vectors of
 * the rows; every observation column through the device functions of imx_observations (value, noise, clip, scale; a last_action column
 * of an env with bf->episode_length_buf == 0 reads 0) straight into the LDS tile; the Linear + ELU layers on the MFMA; then
 * bf->action <- the policy output, bf->prev_action <- the old bf->action, bf->processed_action <- the action records (N, PA): the joint
 * position targets.  Every element equals what the chain imx_observations(ll_plan) -> imx_mlp_infer -> imx_action_process(ll_plan)
 * gives after the masked zero, bit for bit, when the chain's imx_mlp_infer runs the same tile height.
 * noise_u_d: (N, D) uniforms replacing the in-kernel draws (parity runs), or NULL: draws keyed by (seed, step, env * D + column) with
 *   step = (step_counter_d ? step_counter_d[0] : 0) * step_stride + step_offset.  enable_corruption: bit 0, as in imx_observations.
 * obs_out_d: optional (N, D) copy of the observation rows (debug / tests), or NULL.
 * Refused without a launch: a null plan / state / buffers / policy, N < 1, a plan outside the description above, nlayers outside
 * [1, IMX_PP_MAX_LAYERS], a width outside [1, 512], dims that do not match the plan, a null or misaligned weight, a pitch that is
 * no multiple of 32 or below the layer's inputs, packed weights for some layers only, tile_rows other than 0, 16, 32, a state tensor
 * an observation or action record needs, a null action / prev_action / processed_action / episode_length_buf. */
typedef struct imx_pretrained_policy imx_pretrained_policy_t;
#include "imx_pretrained_policy_struct.h"
int imx_pretrained_policy(const imx_plan_t* ll_plan, int64_t N, const imx_state_t* st, const imx_buffers_t* bf,
                          const imx_pretrained_policy_t* policy, const float* noise_u_d, uint64_t seed, const int32_t* step_counter_d,
                          int32_t step_stride, int32_t step_offset, int enable_corruption, int tile_rows, float* obs_out_d,
                          imx_stream_t stream);
/* The refusals of imx_pretrained_policy alone, without a device: 0 = the launch would be made. */
int imx_pretrained_policy_check(const imx_plan_t* ll_plan, int64_t N, const imx_state_t* st, const imx_buffers_t* bf,
                                const imx_pretrained_policy_t* policy, int tile_rows);
/* The tile height imx_pretrained_policy(tile_rows = 0) and imx_mlp_infer (one network) run at N rows: 16 or 32. */
int imx_pretrained_policy_tile_rows(int64_t N);

#ifdef __cplusplus
}
#endif
#endif /* IMX_H_ */
