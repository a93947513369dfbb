#ifndef IMX_RAY_CASTER_STRUCT_H_
#define IMX_RAY_CASTER_STRUCT_H_
/* imx_ray_caster_t: the RayCaster sensor (isaaclab/sensors/ray_caster/ray_caster.py:107-114,220-260 under SensorBase.reset / update /
 * _update_outdated_buffers, sensors/sensor_base.py:182-205,287-296) as imx_ray_caster (imx.h, where the entry point is) takes it.  A
 * header of its own, included by imx.h, like imx_pose2d_struct.h; it can be included alone. */
#include <stdint.h>

typedef struct imx_ray_caster {
    int32_t num_rays;                  /* R: rays of the pattern */
    int32_t attach_yaw_only;           /* cfg.attach_yaw_only: starts by quat_apply_yaw, directions unrotated */
    int32_t substeps;                  /* SensorBase.update(dt) calls of this launch (0: the clocks stand, as for a `data` access) */
    int32_t refresh;                   /* 1: _update_outdated_buffers (cast for the outdated envs); 0: clocks and flags only */
    float dt;                          /* of one SensorBase.update */
    float update_period;               /* cfg.update_period */
    float max_distance;                /* cfg.max_distance */
    float drift_lo, drift_hi;          /* cfg.drift_range */
    float range_clip;                  /* of ranges_d */
    uint64_t seed;                     /* of the counter-based generator (drift), with reset_count_d as its step */
    const float* ray_starts_d;         /* (R,3) pattern starts + offset.pos */
    const float* ray_directions_d;     /* (R,3) pattern directions rotated by offset.rot */
    const float* body_pos_w_d;         /* (N,3) the body the sensor sits on */
    const float* body_quat_w_d;        /* (N,4) w, x, y, z */
    const uint8_t* reset_mask_d;       /* (N) envs to reset before the clocks advance; NULL = none */
    const float* uniforms_d;           /* (N,3) parity draws in [0,1) for the drift of a reset; NULL = the in-kernel generator */
    int32_t* reset_count_d;            /* (N) resets seen so far: the generator's step */
    float* timestamp_d;                /* (N) SensorBase._timestamp */
    float* timestamp_last_update_d;    /* (N) SensorBase._timestamp_last_update */
    uint8_t* is_outdated_d;            /* (N) SensorBase._is_outdated */
    float* drift_d;                    /* (N,3) RayCaster.drift */
    float* pos_w_d;                    /* (N,3) data.pos_w */
    float* quat_w_d;                   /* (N,4) data.quat_w */
    float* ray_hits_w_d;               /* (N,R,3) data.ray_hits_w: +inf in all three components on a miss */
    float* ranges_d;                   /* (N,R) min(||ray_hits_w - pos_w||, range_clip), a miss = range_clip; NULL = not wanted */
    float* ray_starts_w_d;             /* (N,R,3) the world-frame starts the kernel cast; NULL = not wanted */
    float* ray_directions_w_d;         /* (N,R,3) the world-frame directions; NULL = not wanted */
} imx_ray_caster_t;

#endif
