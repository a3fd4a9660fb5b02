// layer/roi_align.h -- torchvision.ops.RoIAlign / torchvision.ops.roi_align (torchvision semantics; no reference counterpart) on the MI355X:
// one launch of si_hip_roi_align_f32 / _f16 (include/si_roi.h).  Parameters as pnnx writes them for the module and the function:
// output_size= (an int or a pair), spatial_scale= (1.0), sampling_ratio= (-1), aligned= (False).
//
// Inputs: x [N, C, H, W] and the boxes as ONE tensor [K, 5], rows (image index, x1, y1, x2, y2); the boxes given as a list of per-image
// tensors are kUnsupport at load.  Output [K, C, ph, pw].  The boxes stay fp32 whatever the engine's storage type (fp16 cannot hold pixel
// coordinates): with fp32 boxes -- a graph input keeps the file's type -- x and the output are served in half natively; any other mix runs
// on the fp32 kernel between casts (HalfStorageOk names the reason).
//
// Dimension 0 of the output counts boxes, not images: batch_rule.h has the family kRoi for both type strings, which is never per-image, and
// the engine refuses to re-batch a graph that holds the operator.
#ifndef SIMPLE_INFER_SRC_LAYER_ROI_ALIGN_H_
#define SIMPLE_INFER_SRC_LAYER_ROI_ALIGN_H_

#include "layer.h"
#include "layer_util.h"
#include "si_roi.h"

namespace SimpleInfer {

class RoiAlign : public Layer {
public:
    virtual Status Init(const pnnx::Operator* op) override;
    virtual Status Validate() override;
    virtual Status Forward(const std::vector<Tensor>& inputs, Tensor& output) override;

    virtual const char* KernelName() const override;
    virtual bool HalfStorageOk(std::string& why) const override;
    virtual double Flops() const override;
    virtual double Bytes() const override;

public:
    int pooled_h_ = 0, pooled_w_ = 0;
    float spatial_scale_ = 1.0f;
    int sampling_ratio_ = -1;
    bool aligned_ = false;

private:
    // false: the operands are not tensors the descriptor can be made of
    bool MakeDesc(const Tensor& x, const Tensor& rois, const Tensor& out, SiRoiAlignDesc& d) const;
    // samples per bin the cost estimates assume (adaptive sampling depends on the data: 2 x 2, detectron's usual count)
    double SamplesPerBin() const;
};

}  // namespace SimpleInfer

#endif
