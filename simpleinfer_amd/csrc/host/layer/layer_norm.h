// layer/layer_norm.h -- F.layer_norm over the last dimension (torch semantics; no reference counterpart): one launch of
// si_hip_layernorm_f32 / _f16 (include/si_layernorm.h).  Parameters as pnnx writes them:
//   F.layer_norm   `normalized_shape` int tuple, `eps` float; `weight` / `bias` either the key `=None` or a further INPUT operand, which
//                  must be a graph constant (pnnx.Attribute): `F.layer_norm name 3 1 x w b out ...`.  With one constant and no key the
//                  constant is the weight.
//   the module form (no registry line yet; see layer_registry.cpp): `elementwise_affine` bool, attributes `@weight` / `@bias`.
// The constants are read on the host at Init and kept as the layer's own fp32 device copy (the kernels' gamma / beta are fp32 under both
// storage types), as FunctionalConv2d keeps a constant bias.  A weight or bias that is an activation is kUnsupport with the reason logged.
//
// Served: rank-2 [N, F] and rank-3 [A, B, E] operands with normalized_shape == (last dim,): both are stored dense in file order, so the
// last axis is contiguous.  A rank-4 operand (stored NHWC: the file's last axis is not the memory's) and a normalized_shape of more than
// one dimension are kUnsupport at LoadModel; a normalized_shape, weight or bias of the wrong length is kErrorShape.
#ifndef SIMPLE_INFER_SRC_LAYER_LAYER_NORM_H_
#define SIMPLE_INFER_SRC_LAYER_LAYER_NORM_H_

#include "layer.h"
#include "layer_util.h"
#include "si_layernorm.h"

namespace SimpleInfer {

class LayerNorm : public Layer {
public:
    virtual Status Init(const pnnx::Operator* op) override;
    virtual Status Deinit() override;
    virtual Status Validate() override;
    virtual Status Forward(const Tensor& input, Tensor& output) override;
    virtual Status Forward(const std::vector<Tensor>& inputs, Tensor& output) override;

    virtual const char* KernelName() const override;
    virtual double Flops() const override;
    virtual double Bytes() const override;
    // halves in and out run the fp16 kernel (the constants stay fp32 and do not enter); a mixed pair goes through the engine's fp32 fallback
    virtual bool HalfStorageOk(std::string& why) const override;

public:
    std::vector<int> normalized_shape_;
    float eps_ = 1e-5f;
    bool has_weight_ = false, has_bias_ = false;
    std::vector<float> weight_, bias_;

private:
    bool MakeDesc(const Tensor& input, const Tensor& output, SiLayerNormDesc& d) const;
    Status Refuse(const std::string& why, Status status = Status::kUnsupport) const;
    // the constant behind input `index` into `dst`; kUnsupport: an activation
    Status ReadConstant(const pnnx::Operator* op, size_t index, const char* what, std::vector<float>& dst) const;
    Status Launch(const Tensor& input, Tensor& output);

    int constants_ = 0;   // input operands behind x
    DeviceBuffer weight_dev_, bias_dev_;
    bool device_ready_ = false;
};

}  // namespace SimpleInfer

#endif
