// Quaternion helpers that compile both as gfx950 device code and as plain host C++ (tools/diff_ik_host.cpp): no HIP header is needed on
// the host side.  Quaternions are w, x, y, z in .x .. .w of a float4.
#pragma once

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define IMX_HD static __host__ __device__ __forceinline__
#define IMX_UNROLL _Pragma("unroll")
#else
#include <cmath>
#include <cstdint>
struct float4 {
    float x, y, z, w;
};
static inline float4 make_float4(float x, float y, float z, float w) { return float4{x, y, z, w}; }
#define IMX_HD static inline
#define IMX_UNROLL
#endif

// full quat_apply (isaaclab/utils/math.py:545-564): t = 2*cross(xyz, v);  out = v + w*t + cross(xyz, t)
IMX_HD void quat_apply(float w, float x, float y, float z, float vx, float vy, float vz, float& ox, float& oy,
                       float& oz) {
    const float tx = (y * vz - z * vy) * 2.0f, ty = (z * vx - x * vz) * 2.0f, tz = (x * vy - y * vx) * 2.0f;
    ox = vx + w * tx + (y * tz - z * ty);
    oy = vy + w * ty + (z * tx - x * tz);
    oz = vz + w * tz + (x * ty - y * tx);
}

// quat_rotate_inverse (isaaclab/utils/math.py:605-625): a - b + c with
//   a = v*(2 w^2 - 1), b = cross(q_vec, v)*w*2, c = q_vec*dot(q_vec, v)*2   (same association as the reference)
IMX_HD void quat_rotate_inverse(float w, float x, float y, float z, float vx, float vy, float vz, float& ox, float& oy,
                                 float& oz) {
    const float s = 2.0f * (w * w) - 1.0f;
    const float ax = vx * s, ay = vy * s, az = vz * s;
    const float cx = y * vz - z * vy, cy = z * vx - x * vz, cz = x * vy - y * vx;
    const float bx = cx * w * 2.0f, by = cy * w * 2.0f, bz = cz * w * 2.0f;
    const float d = (x * vx + y * vy) + z * vz;  // bmm: sequential dot
    const float ccx = x * d * 2.0f, ccy = y * d * 2.0f, ccz = z * d * 2.0f;
    ox = ax - bx + ccx;
    oy = ay - by + ccy;
    oz = az - bz + ccz;
}

// yaw_quat (isaaclab/utils/math.py:521-542) -> (qw, qz) of the yaw-only quaternion (x = y = 0)
IMX_HD void yaw_quat_wz(float w, float x, float y, float z, float& yw, float& yz) {
    const float yaw = atan2f(2.0f * (w * z + x * y), 1.0f - 2.0f * (y * y + z * z));
    const float s = sinf(yaw * 0.5f), c = cosf(yaw * 0.5f);
    const float n = fmaxf(sqrtf(c * c + s * s), 1.0e-9f);  // normalize(): x / norm.clamp(min=eps)
    yw = c / n;
    yz = s / n;
}

// wrap_to_pi (isaaclab/utils/math.py:95-117), torch.remainder semantics
IMX_HD float wrap_to_pi(float a) {
    const float PI = 3.14159265358979323846f, TWO_PI = 6.28318530717958647692f;
    float m = fmodf(a + PI, TWO_PI);
    if (m != 0.0f && m < 0.0f) m += TWO_PI;
    return (m == 0.0f && a > 0.0f) ? PI : m - PI;
}

// counter-based uniform [0,1): two rounds of a 32-bit multiply-xorshift hash (Wellons' "lowbias32") over
// (seed, step, element index); 24-bit mantissa like torch.rand.  ~12 VALU ops (a 64-bit splitmix cost ~40).
IMX_HD float uniform01(uint64_t seed, uint32_t step, uint64_t idx) {
    uint32_t x = (uint32_t)idx ^ ((uint32_t)(idx >> 32) * 0x9E3779B9u) ^ (uint32_t)seed ^ ((uint32_t)(seed >> 32) * 0x85EBCA6Bu);
    x += step * 0x9E3779B9u + 0x7F4A7C15u;
    x ^= x >> 16; x *= 0x7FEB352Du;
    x ^= x >> 15; x *= 0x846CA68Bu;
    x ^= x >> 16;
    x += step; x ^= x >> 16; x *= 0x7FEB352Du; x ^= x >> 15;
    return (float)(x >> 8) * (1.0f / 16777216.0f);
}

// quat_rotate (sign +1) / quat_rotate_inverse (sign -1) (utils/math.py:583-625): a +- b + c.  Not quat_apply: the two round differently.
IMX_HD void quat_rotate_ref(float4 q, float sign, float vx, float vy, float vz, float& ox, float& oy, float& oz) {
    const float w = q.x, x = q.y, y = q.z, z = q.w;
    const float f = 2.0f * (w * w) - 1.0f;
    const float bx = (y * vz - z * vy) * w * 2.0f, by = (z * vx - x * vz) * w * 2.0f, bz = (x * vy - y * vx) * w * 2.0f;
    const float d = (x * vx + y * vy) + z * vz;
    ox = (vx * f + sign * bx) + x * d * 2.0f;
    oy = (vy * f + sign * by) + y * d * 2.0f;
    oz = (vz * f + sign * bz) + z * d * 2.0f;
}

// quat_mul (utils/math.py:464-500): the reference's eight-product form with its association, quaternions w, x, y, z in .x .. .w
IMX_HD float4 quat_mul_ref(float4 a, float4 b) {
    const float w1 = a.x, x1 = a.y, y1 = a.z, z1 = a.w, w2 = b.x, x2 = b.y, y2 = b.z, z2 = b.w;
    const float ww = (z1 + x1) * (x2 + y2);
    const float yy = (w1 - y1) * (w2 + z2);
    const float zz = (w1 + y1) * (w2 - z2);
    const float xx = ww + yy + zz;
    const float qq = 0.5f * (xx + (z1 - x1) * (x2 - y2));
    return make_float4(qq - ww + (z1 - y1) * (y2 - z2), qq - xx + (x1 + w1) * (x2 + w2), qq - yy + (w1 - x1) * (y2 + z2),
                       qq - zz + (z1 + y1) * (w2 - x2));
}

// quat_error of compute_pose_error (utils/math.py:820-867): target * conj(source) / (source * conj(source)).w
IMX_HD float4 quat_error_ref(float4 target, float4 source) {
    const float4 conj = make_float4(source.x, -source.y, -source.z, -source.w);
    const float nrm = quat_mul_ref(source, conj).x;
    return quat_mul_ref(target, make_float4(conj.x / nrm, conj.y / nrm, conj.z / nrm, conj.w / nrm));
}

// axis_angle_from_quat (utils/math.py:646-675) step by step: the w < 0 flip (q * (1 - 2 (w < 0))), half = atan2(||xyz||, w),
// angle = 2 half, the |angle| <= 1e-6 Taylor branch 0.5 - angle^2 / 48, then xyz / that factor
IMX_HD void axis_angle_from_quat_ref(float4 d, float& ax, float& ay, float& az) {
    const float sg = 1.0f - 2.0f * (d.x < 0.0f ? 1.0f : 0.0f);
    const float w = d.x * sg, x = d.y * sg, y = d.z * sg, z = d.w * sg;
    const float mag = sqrtf((x * x + y * y) + z * z);
    const float half = atan2f(mag, w);
    const float angle = 2.0f * half;
    const float s = fabsf(angle) > 1.0e-6f ? sinf(half) / angle : 0.5f - angle * angle / 48.0f;
    ax = x / s;
    ay = y / s;
    az = z / s;
}
