// The Imu sensor for ONE env: SensorBase.reset / update / _update_outdated_buffers (isaaclab/sensors/sensor_base.py:182-205,287-296)
// around Imu.reset / _update_buffers_impl (sensors/imu/imu.py:92-181).  Included by imu.hip (k_imu) and by the host program
// tools/imu_host.cpp -- this file compiles as gfx950 device code and as plain host C++.
#pragma once
#include <math.h>

#include "../../include/imx_imu_struct.h"
#include "imx_quat.h"

// In the reference's order: reset (clocks to zero, outdated, quat_w and the four body-frame vectors to zero -- pos_w and the previous
// velocities stay, so the first refresh after a reset differentiates against the pre-reset velocity), `substeps` times
// SensorBase.update(dt), and with `refresh` _update_buffers_impl for an outdated env.  An env that is not refreshed keeps its data.
// Both accelerations divide by c.dt, the dt of the last update call, whatever time has passed since the last refresh (Imu._dt).
IMX_HD void imu_env(const imx_imu_t& c, int64_t e) {
    float ts = c.timestamp_d[e], last = c.timestamp_last_update_d[e];
    bool outdated = c.is_outdated_d[e] != 0;
    if (c.reset_mask_d && c.reset_mask_d[e]) {
        ts = 0.0f; last = 0.0f; outdated = true;
        IMX_UNROLL
        for (int k = 0; k < 4; ++k) c.quat_w_d[e * 4 + k] = 0.0f;
        IMX_UNROLL
        for (int k = 0; k < 3; ++k) {
            c.lin_vel_b_d[e * 3 + k] = 0.0f; c.ang_vel_b_d[e * 3 + k] = 0.0f;
            c.lin_acc_b_d[e * 3 + k] = 0.0f; c.ang_acc_b_d[e * 3 + k] = 0.0f;
        }
    }
    for (int k = 0; k < c.substeps; ++k) {  // SensorBase.update(dt), fp32 like the tensors
        ts = ts + c.dt;
        outdated = outdated || (ts - last + 1.0e-6f >= c.update_period);
    }
    if (outdated && c.refresh != 0) {
        const int64_t b = e * c.num_bodies + c.body_index;
        const float* p = c.body_pos_w_d + b * 3;
        const float* qp = c.body_quat_w_d + b * 4;
        const float* lv = c.body_lin_vel_w_d + b * 3;
        const float* av = c.body_ang_vel_w_d + b * 3;
        const float4 q = make_float4(qp[0], qp[1], qp[2], qp[3]);
        // pos_w = p + quat_rotate(q, offset_pos); quat_w = quat_mul(q, offset_quat)
        float rx, ry, rz;
        quat_rotate_ref(q, 1.0f, c.offset_pos[0], c.offset_pos[1], c.offset_pos[2], rx, ry, rz);
        c.pos_w_d[e * 3] = p[0] + rx; c.pos_w_d[e * 3 + 1] = p[1] + ry; c.pos_w_d[e * 3 + 2] = p[2] + rz;
        const float4 qs = quat_mul_ref(q, make_float4(c.offset_quat[0], c.offset_quat[1], c.offset_quat[2], c.offset_quat[3]));
        c.quat_w_d[e * 4] = qs.x; c.quat_w_d[e * 4 + 1] = qs.y; c.quat_w_d[e * 4 + 2] = qs.z; c.quat_w_d[e * 4 + 3] = qs.w;
        // lin_vel_w += cross(ang_vel_w, quat_rotate(q, offset_pos - com_pos_b)): into locals, the inputs are never written
        const float* com = c.com_pos_b_d ? c.com_pos_b_d + (c.com_per_env ? e * 3 : 0) : nullptr;
        const float cx = com ? com[0] : 0.0f, cy = com ? com[1] : 0.0f, cz = com ? com[2] : 0.0f;
        quat_rotate_ref(q, 1.0f, c.offset_pos[0] - cx, c.offset_pos[1] - cy, c.offset_pos[2] - cz, rx, ry, rz);
        const float wx = av[0], wy = av[1], wz = av[2];
        const float vx = lv[0] + (wy * rz - wz * ry), vy = lv[1] + (wz * rx - wx * rz), vz = lv[2] + (wx * ry - wy * rx);
        // numerical derivative against the velocities of the last refresh
        const float lax = (vx - c.prev_lin_vel_w_d[e * 3]) / c.dt + c.gravity_bias[0];
        const float lay = (vy - c.prev_lin_vel_w_d[e * 3 + 1]) / c.dt + c.gravity_bias[1];
        const float laz = (vz - c.prev_lin_vel_w_d[e * 3 + 2]) / c.dt + c.gravity_bias[2];
        const float aax = (wx - c.prev_ang_vel_w_d[e * 3]) / c.dt;
        const float aay = (wy - c.prev_ang_vel_w_d[e * 3 + 1]) / c.dt;
        const float aaz = (wz - c.prev_ang_vel_w_d[e * 3 + 2]) / c.dt;
        // the four vectors in the SENSOR's frame: quat_rotate_inverse(data.quat_w, .), offset rotation included
        float ox, oy, oz;
        quat_rotate_ref(qs, -1.0f, vx, vy, vz, ox, oy, oz);
        c.lin_vel_b_d[e * 3] = ox; c.lin_vel_b_d[e * 3 + 1] = oy; c.lin_vel_b_d[e * 3 + 2] = oz;
        quat_rotate_ref(qs, -1.0f, wx, wy, wz, ox, oy, oz);
        c.ang_vel_b_d[e * 3] = ox; c.ang_vel_b_d[e * 3 + 1] = oy; c.ang_vel_b_d[e * 3 + 2] = oz;
        quat_rotate_ref(qs, -1.0f, lax, lay, laz, ox, oy, oz);
        c.lin_acc_b_d[e * 3] = ox; c.lin_acc_b_d[e * 3 + 1] = oy; c.lin_acc_b_d[e * 3 + 2] = oz;
        quat_rotate_ref(qs, -1.0f, aax, aay, aaz, ox, oy, oz);
        c.ang_acc_b_d[e * 3] = ox; c.ang_acc_b_d[e * 3 + 1] = oy; c.ang_acc_b_d[e * 3 + 2] = oz;
        c.prev_lin_vel_w_d[e * 3] = vx; c.prev_lin_vel_w_d[e * 3 + 1] = vy; c.prev_lin_vel_w_d[e * 3 + 2] = vz;
        c.prev_ang_vel_w_d[e * 3] = wx; c.prev_ang_vel_w_d[e * 3 + 1] = wy; c.prev_ang_vel_w_d[e * 3 + 2] = wz;
        last = ts;
        outdated = false;
    }
    c.timestamp_d[e] = ts;
    c.timestamp_last_update_d[e] = last;
    c.is_outdated_d[e] = outdated ? 1 : 0;
}

// the argument check of the entry point, as a message (NULL = fine): no launch is made with a sensor this names
static inline const char* imu_check(const imx_imu_t* c) {
    if (!c) return "null imx_imu_t";
    if (c->num_bodies < 1 || c->body_index < 0 || c->body_index >= c->num_bodies) return "body_index outside [0, num_bodies)";
    if (c->substeps < 0 || c->substeps > 1024) return "substeps outside [0, 1024]";
    if (!(c->dt >= 0.0f) || !(c->update_period >= 0.0f)) return "negative dt or update_period";
    if (c->refresh && !(c->dt > 0.0f)) return "a refresh divides by dt, which must be positive (call update first)";
    if (c->refresh && !c->body_pos_w_d) return "body_pos_w missing";
    if (c->refresh && !c->body_quat_w_d) return "body_quat_w missing";
    if (c->refresh && !c->body_lin_vel_w_d) return "body_lin_vel_w missing";
    if (c->refresh && !c->body_ang_vel_w_d) return "body_ang_vel_w missing";
    if (!c->timestamp_d || !c->timestamp_last_update_d || !c->is_outdated_d) return "a clock tensor is missing";
    if (!c->pos_w_d || !c->quat_w_d || !c->lin_vel_b_d || !c->ang_vel_b_d || !c->lin_acc_b_d || !c->ang_acc_b_d) return "a data tensor is missing";
    if (!c->prev_lin_vel_w_d || !c->prev_ang_vel_w_d) return "a previous-velocity tensor is missing";
    return nullptr;
}
