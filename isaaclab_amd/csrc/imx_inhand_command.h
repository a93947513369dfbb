// The in-hand re-orientation command for ONE env: CommandTerm.reset / compute (isaaclab/managers/command_manager.py:120-187) +
// InHandReOrientationCommand (isaaclab_tasks .../manipulation/inhand/mdp/commands/orientation_command.py:22-124).  Included by
// inhand_command.hip (k_inhand_command) and by the host program tools/inhand_command_host.cpp -- this file compiles as gfx950 device code
// and as plain host C++.
#pragma once
#include <math.h>

#include "../../include/imx_inhand_command_struct.h"
#include "imx_quat.h"

// column k of {time_left, rand_floats[:, 0], rand_floats[:, 1]} of one resampling: the recorded table or the counter-based generator
// (the seeds and columns scheme of u_at, imx_producers.h, and pose2d_u_at)
IMX_HD float inhand_u_at(const float* U, int64_t e, int k, uint64_t seed, uint32_t step) {
    return U ? U[e * 3 + k] : uniform01(seed + 0x1234567ull * (uint64_t)(k + 1), step, (uint64_t)e);
}

// quat_from_angle_axis (utils/math.py:629-642) about unit axis X (axis 0) or Y (axis 1): normalize(axis) * sin(angle / 2), cos(angle / 2),
// then normalize (:82-92: x / max(||x||, 1e-9)) of the four components
IMX_HD float4 inhand_quat_about(float angle, int axis) {
    const float theta = angle / 2.0f;
    const float s = sinf(theta), w = cosf(theta);
    const float x = (axis == 0 ? 1.0f : 0.0f) * s, y = (axis == 1 ? 1.0f : 0.0f) * s, z = 0.0f * s;
    const float n = fmaxf(sqrtf(((w * w + x * x) + y * y) + z * z), 1.0e-9f);
    return make_float4(w / n, x / n, y / n, z / n);
}

// quat_error_magnitude (utils/math.py:678-690): ||axis_angle_from_quat(quat_mul(q1, quat_conjugate(q2)))||
IMX_HD float inhand_quat_error_magnitude(float4 q1, float4 q2) {
    float ax, ay, az;
    axis_angle_from_quat_ref(quat_mul_ref(q1, make_float4(q2.x, -q2.y, -q2.z, -q2.w)), ax, ay, az);
    return sqrtf((ax * ax + ay * ay) + az * az);
}

// `reset`: CommandTerm.reset for this env first (metrics logged and zeroed, counter zeroed, resample); `do_compute`: then
// CommandTerm.compute(dt) in the reference's order -- _update_metrics (the consecutive_success metric ACCUMULATES, `<` threshold),
// time_left -= dt and a resample where it ran out, _update_command (a resample where the goal was reached, with update_goal_on_success).
// m0[3] receives orientation_error, position_error, consecutive_success as they stood BEFORE the reset (what CommandTerm.reset logs).
IMX_HD void inhand_command_env(int64_t N, int64_t e, const imx_inhand_command_t& c, float dt, int do_compute, bool reset, uint32_t step,
                               float* m0) {
    const float PI = 3.14159265358979323846f;
    float* cmd = c.command_d + e * 7;
    float4 goal = make_float4(cmd[3], cmd[4], cmd[5], cmd[6]);
    float tl = c.time_left_d[e];
    int64_t cnt = c.command_counter_d[e];
    float m_ori = c.metric_orientation_error_d[e], m_pos = c.metric_position_error_d[e], m_succ = c.metric_consecutive_success_d[e];
    m0[0] = m_ori; m0[1] = m_pos; m0[2] = m_succ;
    int draw = 0;  // which of the three possible resamplings of this call (reset, timer, goal reached) -> distinct in-kernel streams
    auto resample = [&]() {  // CommandTerm._resample (command_manager.py:172-187) + _resample_command (orientation_command.py:104-111)
        const float* U = c.uniforms_d ? c.uniforms_d + (size_t)draw * N * 3 : nullptr;
        const uint64_t sd = c.seed + 0x9E3779B97F4A7C15ull * (uint64_t)draw;
        tl = inhand_u_at(U, e, 0, sd, step) * (c.cfg[1] - c.cfg[0]) + c.cfg[0];
        cnt += 1;
        const float u0 = 2.0f * inhand_u_at(U, e, 1, sd, step) - 1.0f, u1 = 2.0f * inhand_u_at(U, e, 2, sd, step) - 1.0f;
        goal = quat_mul_ref(inhand_quat_about(u0 * PI, 0), inhand_quat_about(u1 * PI, 1));
        if (c.make_quat_unique && goal.x < 0.0f) goal = make_float4(-goal.x, -goal.y, -goal.z, -goal.w);
        ++draw;
    };
    if (reset) {  // CommandTerm.reset (command_manager.py:120-149)
        m_ori = 0.0f; m_pos = 0.0f; m_succ = 0.0f; cnt = 0;
        resample();
    }
    if (do_compute) {  // CommandTerm.compute (:151-168)
        const float* oq = c.object_root_quat_w_d + e * 4;
        const float* op = c.object_root_pos_w_d + e * 3;
        const float* pw = c.pos_command_w_d + e * 3;
        m_ori = inhand_quat_error_magnitude(make_float4(oq[0], oq[1], oq[2], oq[3]), goal);
        const float dx = op[0] - pw[0], dy = op[1] - pw[1], dz = op[2] - pw[2];
        m_pos = sqrtf((dx * dx + dy * dy) + dz * dz);
        const bool reached = m_ori < c.cfg[2];
        m_succ += reached ? 1.0f : 0.0f;
        tl -= dt;
        if (tl <= 0.0f) resample();
        if (c.update_goal_on_success && reached) resample();
    }
    cmd[3] = goal.x; cmd[4] = goal.y; cmd[5] = goal.z; cmd[6] = goal.w;
    c.time_left_d[e] = tl;
    c.command_counter_d[e] = cnt;
    c.metric_orientation_error_d[e] = m_ori;
    c.metric_position_error_d[e] = m_pos;
    c.metric_consecutive_success_d[e] = m_succ;
}

// the argument check of the entry point, as a message (NULL = fine): no launch is made with a pointer this names
static inline const char* inhand_command_check(const imx_inhand_command_t* c, int do_compute) {
    if (!c) return "null imx_inhand_command_t";
    if (!(c->cfg[1] > 0.0f) || c->cfg[0] > c->cfg[1]) return "resampling_time_range must be ordered and its upper end positive";
    if (!(c->cfg[2] >= 0.0f)) return "orientation_success_threshold must not be negative";
    if (do_compute && !c->pos_command_w_d) return "pos_command_w missing";
    if (do_compute && !c->object_root_pos_w_d) return "object_root_pos_w missing";
    if (do_compute && !c->object_root_quat_w_d) return "object_root_quat_w missing";
    if (!do_compute && !c->reset_mask_d) return "neither a reset mask nor compute: nothing to do";
    if (!c->command_d) return "command missing";
    if (!c->time_left_d) return "time_left missing";
    if (!c->command_counter_d) return "command_counter missing";
    if (!c->metric_orientation_error_d) return "metric orientation_error missing";
    if (!c->metric_position_error_d) return "metric position_error missing";
    if (!c->metric_consecutive_success_d) return "metric consecutive_success missing";
    return nullptr;
}
