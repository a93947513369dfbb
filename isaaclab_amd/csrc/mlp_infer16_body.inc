// The body of k_mlp_infer16 / k_mlp_infer16_binary (mlp.hip), included once per kernel with IMX_ACT_BINARY = false (the kernel as it always was) or true (the actor
// head's epilogue with the binary joint term's path).  A textual include, not a device function: the existing kernels then compile to the
// instruction streams they had.  Also the body of k_mlp_infer2_16 / k_mlp_infer2_16_binary (IMX_INFER_TWO_INPUTS = 1, below).
    extern __shared__ float smem[];  // two activation buffers of INF16_ROWS x INF_PITCH floats
    float* buf0 = smem;
    float* buf1 = smem + INF16_ROWS * INF_PITCH;
    const int which = blockIdx.x / a.tiles;
    const InferNet& net = a.net[which];
    const int64_t m0 = (int64_t)(blockIdx.x - which * a.tiles) * INF16_ROWS;
    const bool act_here = act.enabled && which == 0;
    // (input source and dense copy of the tile: as in mlp_infer_body.inc)
#if IMX_INFER_TWO_INPUTS
    const float* const x_in = which ? two.X1 : a.X;
    const int64_t ldx_in = which ? two.ldx1 : a.ldx;
    float* const obs_dst = which ? two.obs_out1 : (act.enabled ? act.obs_out : nullptr);
#define IMX_INFER_X x_in
#define IMX_INFER_LDX ldx_in
#define IMX_INFER_OBS_ON (obs_dst != nullptr)
#define IMX_INFER_OBS_DST obs_dst
#else
#define IMX_INFER_X a.X
#define IMX_INFER_LDX a.ldx
#define IMX_INFER_OBS_ON act_here
#define IMX_INFER_OBS_DST act.obs_out
#endif
    const int K0 = net.dim[0], K0p = (K0 + 31) & ~31;
    {
        const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
        float v[4][INF_MAXD / 64];  // wave w: rows w, w+4, w+8, w+12; all loads before the first LDS store
#if IMX_INFER_NORMALIZE
        // (k_mlp_infer2n_16*: as in mlp_infer_body.inc)
        const float* const n_mean = nrm.mean[which];
        const float* const n_std = nrm.stdv[which];
        float nmu[INF_MAXD / 64], nsd[INF_MAXD / 64];
#pragma unroll
        for (int cc = 0; cc < INF_MAXD / 64; ++cc) {
            const int c = lane + 64 * cc;
            nmu[cc] = n_mean ? n_mean[c < K0 ? c : 0] : 0.0f;
            nsd[cc] = n_mean ? n_std[c < K0 ? c : 0] : 1.0f;
        }
#endif
#pragma unroll
        for (int rr = 0; rr < 4; ++rr) {
            const int row = w + 4 * rr;
            const float* src = IMX_INFER_X + (m0 + row < a.M ? m0 + row : 0) * IMX_INFER_LDX;
#pragma unroll
            for (int cc = 0; cc < INF_MAXD / 64; ++cc) {
                const int c = lane + 64 * cc;
                const float x = src[c < K0 ? c : 0];
                v[rr][cc] = (c < K0 && m0 + row < a.M) ? x : 0.0f;
            }
        }
#if IMX_INFER_NORMALIZE
        if (n_mean) {
            const float n_eps = nrm.eps[which];
#pragma unroll
            for (int rr = 0; rr < 4; ++rr) {
                const int row = w + 4 * rr;
#pragma unroll
                for (int cc = 0; cc < INF_MAXD / 64; ++cc) {
                    const int c = lane + 64 * cc;
                    if (c < K0 && m0 + row < a.M) v[rr][cc] = (v[rr][cc] - nmu[cc]) / (nsd[cc] + n_eps);
                }
            }
        }
#endif
#pragma unroll
        for (int rr = 0; rr < 4; ++rr) {
            const int row = w + 4 * rr;
#pragma unroll
            for (int cc = 0; cc < INF_MAXD / 64; ++cc) {
                const int c = lane + 64 * cc;
                if (c < K0p) buf0[row * INF_PITCH + c] = v[rr][cc];
                if (IMX_INFER_OBS_ON && c < K0 && m0 + row < a.M) IMX_INFER_OBS_DST[(m0 + row) * (int64_t)K0 + c] = v[rr][cc];
            }
        }
    }
    __syncthreads();
    float* in = buf0;
    float* out = buf1;
    for (int l = 0; l < net.nlayers; ++l) {
        const int K = net.dim[l], N = net.dim[l + 1];
        const bool last = l == net.nlayers - 1;
        const int nbw = ((N + 15) / 16 + 3) / 4;  // 16-column blocks per wave
        float* so = (last && !act_here) ? nullptr : out;
        if (!last) {
            const int Np = (N + 31) & ~31;
            for (int i = threadIdx.x; i < INF16_ROWS * (Np - N); i += blockDim.x) {
                const int row = i / (Np - N), col = N + i - row * (Np - N);
                out[row * INF_PITCH + col] = 0.0f;
            }
        }
        if (nbw <= 1) infer_layer16<1>(in, K, net.W[l], net.ldw[l], net.b[l], N, !last, net.alpha, so, net.out, m0, a.M);
        else if (nbw == 2) infer_layer16<2>(in, K, net.W[l], net.ldw[l], net.b[l], N, !last, net.alpha, so, net.out, m0, a.M);
        else if (nbw <= 4) infer_layer16<4>(in, K, net.W[l], net.ldw[l], net.b[l], N, !last, net.alpha, so, net.out, m0, a.M);
        else infer_layer16<8>(in, K, net.W[l], net.ldw[l], net.b[l], N, !last, net.alpha, so, net.out, m0, a.M);
        __syncthreads();
        float* t = in; in = out; out = t;
    }
    if (act_here) act_epilogue<INF16_ROWS, IMX_ACT_BINARY>(act, in, out, m0, a.M);
#undef IMX_INFER_X
#undef IMX_INFER_LDX
#undef IMX_INFER_OBS_ON
#undef IMX_INFER_OBS_DST
