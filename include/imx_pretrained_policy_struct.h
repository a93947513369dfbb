/* imx_pretrained_policy_t: the low-level policy of a PreTrainedPolicyAction (imx_pretrained_policy, imx.h).  imx.h declares the type and
 * the entry point and includes this header for the definition.
 * An MLP of nlayers Linear layers with ELU(elu_alpha) between them: layer l maps dims[l] -> dims[l + 1] columns.  weights_d[l] is the
 * (dims[l + 1], weight_pitch[l]) row-major weight, rows zero-padded to a pitch that is a multiple of 32 floats, 16-byte aligned;
 * packed_weights_d[l] is the same layer in the lane order of the 32-row kernel (imx_mlp_pack_weights), or NULL for all layers;
 * biases_d[l] holds dims[l + 1] floats.  The limits are imx_mlp_infer's: at most IMX_PP_MAX_LAYERS layers, widths 1..512. */
#ifndef IMX_PRETRAINED_POLICY_STRUCT_H_
#define IMX_PRETRAINED_POLICY_STRUCT_H_

#define IMX_PP_MAX_LAYERS 4

typedef struct imx_pretrained_policy {
    int32_t nlayers;
    int32_t dims[5];
    int32_t weight_pitch[IMX_PP_MAX_LAYERS];
    float elu_alpha;
    int32_t reserved;
    const float* weights_d[IMX_PP_MAX_LAYERS];
    const float* packed_weights_d[IMX_PP_MAX_LAYERS];
    const float* biases_d[IMX_PP_MAX_LAYERS];
} imx_pretrained_policy_t;

#endif
