// One FrameTransformer frame (isaaclab/sensors/frame_transformer/frame_transformer.py:337-384) in the reference's operation order.
// Included by step.hip (k_term_rew_cabinet, k_obs_cabinet), frame_transformer.hip (k_frame_transformer) and by the host program
// tools/frame_transformer_host.cpp -- this file compiles as gfx950 device code and as plain host C++.
#pragma once

#include "imx_quat.h"

#ifndef IMX_FRAME_WORDS
#define IMX_FRAME_WORDS 9  // include/imx.h: [body id, asset, offset position 3 f32, offset rotation w x y z f32]
#endif

struct ImxFramePose {
    float px, py, pz;  // position
    float4 q;          // orientation w, x, y, z in .x .. .w
};

IMX_HD float imx_word_as_float(int32_t w) {
    union {
        int32_t i;
        float f;
    } u;
    u.i = w;
    return u.f;
}

// combine_frame_transforms(body position, body quaternion, offset position, offset rotation) (utils/math.py:750-781):
// t02 = t01 + quat_apply(q01, t12) (quat_apply :546-566, then the add), q02 = quat_mul(q01, q12) (:464-500).
// bp = the body's position (3 floats), bq = its quaternion (4 floats w, x, y, z), fr = the frame's IMX_FRAME_WORDS words.
IMX_HD ImxFramePose imx_frame_pose(const float* bp, const float* bq, const int32_t* fr) {
    ImxFramePose o;
    float ax, ay, az;
    quat_apply(bq[0], bq[1], bq[2], bq[3], imx_word_as_float(fr[2]), imx_word_as_float(fr[3]), imx_word_as_float(fr[4]), ax, ay, az);
    o.px = bp[0] + ax;
    o.py = bp[1] + ay;
    o.pz = bp[2] + az;
    o.q = quat_mul_ref(make_float4(bq[0], bq[1], bq[2], bq[3]),
                       make_float4(imx_word_as_float(fr[5]), imx_word_as_float(fr[6]), imx_word_as_float(fr[7]), imx_word_as_float(fr[8])));
    return o;
}

// subtract_frame_transforms(source, target) (utils/math.py:785-816): q10 = quat_inv(q01) = normalize(conjugate(q01)) (:239-248, normalize
// :82-92 = x / max(||x||, 1e-9)), q12 = quat_mul(q10, q02), t12 = quat_apply(q10, t02 - t01): the target in the source's frame.
IMX_HD ImxFramePose imx_frame_relative(const ImxFramePose& src, const ImxFramePose& tgt) {
    const float w = src.q.x, x = src.q.y, y = src.q.z, z = src.q.w;
    const float n = fmaxf(sqrtf(((w * w + x * x) + y * y) + z * z), 1.0e-9f);
    const float4 inv = make_float4(w / n, -x / n, -y / n, -z / n);
    ImxFramePose o;
    o.q = quat_mul_ref(inv, tgt.q);
    quat_apply(inv.x, inv.y, inv.z, inv.w, tgt.px - src.px, tgt.py - src.py, tgt.pz - src.pz, o.px, o.py, o.pz);
    return o;
}
