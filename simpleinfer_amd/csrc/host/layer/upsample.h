// layer/upsample.h -- nn.Upsample, F.interpolate and F.upsample on rank-4 tensors: nearest (reference src/layer/upsample.cpp:18-45
// Init, :76-99 index rule src = clamp(int(float(dst) * (1/scale)))) and bilinear with torch's rule (include/si_hip.h, "bilinear
// upsample"), each by scale_factor= or by size=.  Nearest with a scale factor is the reference's layer, unchanged.
#pragma once

#include "layer.h"
#include "layer_util.h"

namespace SimpleInfer {

class Upsample : public Layer {
public:
    virtual Status Init(const pnnx::Operator* op) override;
    virtual Status Validate() override;
    virtual Status Forward(const Tensor& input, Tensor& output) override;
    virtual const char* KernelName() const override;

    // the reference's form -- nearest, scale factor, no size: the only one FuseUpsampleIntoConvs may fold into the consumer convs
    // (their dual-source kernels implement that index rule only)
    bool IsNearestByScale() const { return UpsampleMode::kNearest == upsample_mode_ && !by_size_; }

public:
    enum class UpsampleMode { kNearest = 0, kBilinear = 1 } upsample_mode_ = UpsampleMode::kNearest;
    float scale_factor_h_ = 1.0f;
    float scale_factor_w_ = 1.0f;

private:
    bool MakeDesc(const Tensor& input, const Tensor& output, SiUpsampleDesc& d) const;

    bool align_corners_ = false;
    bool has_scale_ = false;   // scale_factor= given
    bool by_size_ = false;     // the output size is size= (or recompute_scale_factor=True: the steps come from the sizes)
    int size_h_ = 0, size_w_ = 0;
    double scale_h_ = 0.0, scale_w_ = 0.0;   // scale_factor as the double torch saw (the shortest decimal that reads back as the file's float)
    float step_h_ = 0.0f, step_w_ = 0.0f;    // set by Validate for every form but nearest-by-scale
};

}  // namespace SimpleInfer
