// layer/group_norm.h -- nn.GroupNorm and nn.InstanceNorm2d (torch semantics, eval mode; no reference counterpart): statistics
// from the activation itself, per image and group, on every forward -- si_hip_groupnorm_f32 / _f16 (include/si_norm.h), one or
// two launches by shape, an activation in the epilogue.  InstanceNorm2d is the case groups = channels.  The parameter keys are
// the ones pnnx's own passes write for the two modules.
#ifndef SIMPLE_INFER_SRC_LAYER_GROUP_NORM_H_
#define SIMPLE_INFER_SRC_LAYER_GROUP_NORM_H_

#include "layer.h"
#include "layer_util.h"
#include "si_norm.h"

namespace SimpleInfer {

class GroupNorm : public Layer {
public:
    virtual Status Init(const pnnx::Operator* op) override;
    virtual Status Deinit() override;
    virtual Status Validate() override;
    virtual Status Forward(const Tensor& input, Tensor& output) override;

    virtual const char* KernelName() const override;
    virtual double Flops() const override;
    // (Bytes: the base class's one read plus one write of the tensor -- the algorithmic traffic, whichever form runs)

    // engine fusion hook: y = act(norm(x))
    void SetFusion(int act, float act_param = 0.0f) {
        act_ = act;
        act_param_ = act_param;
    }

public:
    int num_groups_ = 0;      // 0: one group per channel (nn.InstanceNorm2d)
    int num_channels_ = 0;
    float eps_ = 1e-5f;
    bool use_affine_ = false;
    bool track_running_stats_ = false;
    std::vector<float> weight_, bias_;

    int act_ = SI_ACT_NONE;
    float act_param_ = 0.0f;

private:
    bool MakeDesc(const Tensor& input, const Tensor& output, SiGroupNormDesc& d) const;
    Status PrepareDevice(const SiGroupNormDesc& d);

    DeviceBuffer params_dev_;   // [weight | bias]
    DeviceBuffer workspace_dev_;
    bool params_ready_ = false;
};

}  // namespace SimpleInfer

#endif
