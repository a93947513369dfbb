#ifndef IMX_IMU_STRUCT_H_
#define IMX_IMU_STRUCT_H_
/* imx_imu_t: the Imu sensor (isaaclab/sensors/imu/imu.py:92-181 under SensorBase.reset / update / _update_outdated_buffers,
 * sensors/sensor_base.py:182-205,287-296) as imx_imu (imx.h, where the entry point is) takes it.  A header of its own, included by
 * imx.h, like imx_ray_caster_struct.h; it can be included alone. */
#include <stdint.h>

typedef struct imx_imu {
    int32_t body_index;                /* column b of the (N, B, .) inputs */
    int32_t num_bodies;                /* B of the inputs; 1 with body_index 0 for (N, .) inputs */
    int32_t com_per_env;               /* com_pos_b_d is (N,3) (1) or one (3,) row for every env (0) */
    int32_t substeps;                  /* SensorBase.update(dt) calls of this launch (0: the clocks stand, as for a `data` access) */
    int32_t refresh;                   /* 1: _update_outdated_buffers (the outdated envs are recomputed); 0: clocks and flags only */
    float dt;                          /* of one SensorBase.update; Imu._dt, the divisor of both accelerations */
    float update_period;               /* cfg.update_period */
    float offset_pos[3];               /* cfg.offset.pos */
    float offset_quat[4];              /* cfg.offset.rot, w x y z */
    float gravity_bias[3];             /* cfg.gravity_bias */
    const float* body_pos_w_d;         /* (N,B,3) link position of the body the sensor sits on */
    const float* body_quat_w_d;        /* (N,B,4) link orientation, w x y z */
    const float* body_lin_vel_w_d;     /* (N,B,3) linear velocity of the body's centre of mass; never written */
    const float* body_ang_vel_w_d;     /* (N,B,3) angular velocity; never written */
    const float* com_pos_b_d;          /* the centre of mass in the link frame (see com_per_env); NULL = zeros */
    const uint8_t* reset_mask_d;       /* (N) envs to reset before the clocks advance; NULL = none */
    float* timestamp_d;                /* (N) SensorBase._timestamp */
    float* timestamp_last_update_d;    /* (N) SensorBase._timestamp_last_update */
    uint8_t* is_outdated_d;            /* (N) SensorBase._is_outdated */
    float* pos_w_d;                    /* (N,3) data.pos_w */
    float* quat_w_d;                   /* (N,4) data.quat_w */
    float* lin_vel_b_d;                /* (N,3) data.lin_vel_b */
    float* ang_vel_b_d;                /* (N,3) data.ang_vel_b */
    float* lin_acc_b_d;                /* (N,3) data.lin_acc_b */
    float* ang_acc_b_d;                /* (N,3) data.ang_acc_b */
    float* prev_lin_vel_w_d;           /* (N,3) Imu._prev_lin_vel_w: the corrected velocity of the last refresh */
    float* prev_ang_vel_w_d;           /* (N,3) Imu._prev_ang_vel_w */
} imx_imu_t;

#endif
