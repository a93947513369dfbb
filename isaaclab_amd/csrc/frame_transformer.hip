// k_frame_transformer: FrameTransformer._update_buffers_impl (isaaclab/sensors/frame_transformer/frame_transformer.py:337-384) -- the six
// FrameTransformerData tensors of one sensor from the body poses of one articulation.  The per-frame arithmetic is imx_frame_pose /
// imx_frame_relative (imx_frame_transformer.h, shared with the step kernels and with tools/frame_transformer_host.cpp).
#include "imx_internal.h"
#include "imx_frame_transformer.h"

// Lane = (env, target frame): i = e * T + t.  Each lane derives the source pose itself (the frame words are wave-uniform scalar loads,
// the source body's pose is shared by the T lanes of an env: one cache line) -- no LDS, no barrier.  Lane t == 0 of an env also stores
// the source pose.
__global__ void __launch_bounds__(256)
k_frame_transformer(int64_t N, int T, int NB, const float* __restrict__ body_pos_w, const float* __restrict__ body_quat_w,
                    const int32_t* __restrict__ frames, float* __restrict__ source_pos_w, float* __restrict__ source_quat_w,
                    float* __restrict__ target_pos_w, float* __restrict__ target_quat_w, float* __restrict__ target_pos_source,
                    float* __restrict__ target_quat_source) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N * T) return;
    const int64_t e = i / T;
    const int t = (int)(i - e * T);
    const int32_t* __restrict__ fs = frames;
    const int32_t* __restrict__ ft = frames + (size_t)(1 + t) * IMX_FRAME_WORDS;
    const int64_t bs = e * NB + fs[0], bt = e * NB + ft[0];
    const ImxFramePose src = imx_frame_pose(body_pos_w + bs * 3, body_quat_w + bs * 4, fs);
    const ImxFramePose tgt = imx_frame_pose(body_pos_w + bt * 3, body_quat_w + bt * 4, ft);
    const ImxFramePose rel = imx_frame_relative(src, tgt);
    if (t == 0) {
        source_pos_w[e * 3] = src.px; source_pos_w[e * 3 + 1] = src.py; source_pos_w[e * 3 + 2] = src.pz;
        reinterpret_cast<float4*>(source_quat_w)[e] = src.q;
    }
    target_pos_w[i * 3] = tgt.px; target_pos_w[i * 3 + 1] = tgt.py; target_pos_w[i * 3 + 2] = tgt.pz;
    reinterpret_cast<float4*>(target_quat_w)[i] = tgt.q;
    target_pos_source[i * 3] = rel.px; target_pos_source[i * 3 + 1] = rel.py; target_pos_source[i * 3 + 2] = rel.pz;
    reinterpret_cast<float4*>(target_quat_source)[i] = rel.q;
}

extern "C" int imx_frame_transformer(int64_t N, int num_targets, int num_bodies, const float* body_pos_w_d, const float* body_quat_w_d,
                                     const int32_t* frames_d, const int32_t* frames_h, float* source_pos_w_d, float* source_quat_w_d,
                                     float* target_pos_w_d, float* target_quat_w_d, float* target_pos_source_d, float* target_quat_source_d,
                                     imx_stream_t stream) {
    IMX_REQUIRE(N > 0 && N < (1ll << 31), "imx_frame_transformer: N out of range");
    IMX_REQUIRE(num_targets >= 1 && num_targets <= 4096, "imx_frame_transformer: %d target frames (1..4096)", num_targets);
    IMX_REQUIRE(num_bodies >= 1 && num_bodies <= 4096, "imx_frame_transformer: %d bodies (1..4096)", num_bodies);
    IMX_REQUIRE(N * (int64_t)num_targets < (1ll << 31), "imx_frame_transformer: %lld envs x %d frames exceed the grid", (long long)N, num_targets);
    IMX_REQUIRE(body_pos_w_d, "imx_frame_transformer: body_pos_w missing");
    IMX_REQUIRE(body_quat_w_d, "imx_frame_transformer: body_quat_w missing");
    IMX_REQUIRE(frames_d && frames_h, "imx_frame_transformer: frame table missing (device and host words)");
    IMX_REQUIRE(source_pos_w_d && source_quat_w_d && target_pos_w_d && target_quat_w_d && target_pos_source_d && target_quat_source_d,
                "imx_frame_transformer: null output");
    for (int f = 0; f <= num_targets; ++f) {
        const int b = frames_h[(size_t)f * IMX_FRAME_WORDS];
        IMX_REQUIRE(b >= 0 && b < num_bodies, "imx_frame_transformer: frame %d sits on body %d outside [0, %d)", f, b, num_bodies);
    }
    const int64_t n = N * num_targets;
    hipLaunchKernelGGL(k_frame_transformer, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, N, num_targets, num_bodies,
                       body_pos_w_d, body_quat_w_d, frames_d, source_pos_w_d, source_quat_w_d, target_pos_w_d, target_quat_w_d,
                       target_pos_source_d, target_quat_source_d);
    IMX_HIP(hipGetLastError());
    return 0;
}
