// layer/multihead_attention.h -- nn.MultiheadAttention (torch semantics, eval mode, no mask, no dropout, the attention output only; no
// reference counterpart).  Three stages in stream order: the input projection through the 1x1 path of si_hip_conv2d_f32 / _f16 into the
// column slices Q | K | V of a [rows, 3E] workspace, the fused attention kernel (include/si_attention.h) on strided views of that
// workspace, and the output projection through the same conv entry into the output operand.  The parameter and attribute keys are the
// ones pnnx writes for the module.  1 input (self-attention), 2 (query; key = value) or 3 (query, key, value), all of rank 3: [L, N, E],
// or [N, L, E] with batch_first.
#ifndef SIMPLE_INFER_SRC_LAYER_MULTIHEAD_ATTENTION_H_
#define SIMPLE_INFER_SRC_LAYER_MULTIHEAD_ATTENTION_H_

#include "layer.h"
#include "layer_util.h"
#include "si_attention.h"

namespace SimpleInfer {

class MultiheadAttention : public Layer {
public:
    virtual Status Init(const pnnx::Operator* op) override;
    virtual Status Deinit() override;
    virtual Status Validate() override;
    virtual Status Forward(const Tensor& input, Tensor& output) override;
    virtual Status Forward(const std::vector<Tensor>& inputs, Tensor& output) override;

    virtual const char* KernelName() const override;
    virtual double Flops() const override;
    virtual bool HalfStorageOk(std::string& why) const override;

public:
    int embed_dim_ = 0, num_heads_ = 0, kdim_ = 0, vdim_ = 0;
    bool use_bias_ = true, batch_first_ = false, add_bias_kv_ = false, add_zero_attn_ = false;
    std::vector<float> in_proj_weight_, in_proj_bias_, out_proj_weight_, out_proj_bias_;

private:
    struct Geometry {
        int batch = 0, lq = 0, lk = 0;
    };
    bool GetGeometry(const std::vector<const Tensor*>& in, const Tensor& out, Geometry& g) const;
    bool MakeDesc(const Geometry& g, SiAttentionDesc& d) const;
    Status PrepareDevice(bool half, int n_in, const Geometry& g);
    Status Run(const std::vector<Tensor>& in, Tensor& out);

    // weight images of the projection launches: [0 .. n_in) the row blocks of in_proj_weight each input feeds (1 input: all 3E rows; 2: E and
    // 2E; 3: E each), [3] out_proj
    DeviceBuffer weight_dev_[4];
    DeviceBuffer bias_dev_;        // [in_proj_bias (3E) | out_proj.bias (E)]
    DeviceBuffer workspace_dev_;   // [rows, 3E] Q | K | V, then [rows_q, E] the attention output
    bool device_ready_ = false, prepared_half_ = false;
    int prepared_inputs_ = 0;
};

}  // namespace SimpleInfer

#endif
