// layer/affine_grid.h -- F.affine_grid (torch semantics; no reference counterpart) for 2-D transforms: theta [N, 2, 3] -> the sampling grid
// [N, H, W, 2] of F.grid_sample, one launch of si_hip_affine_grid_f32 / _f16 (include/si_grid.h).  Parameters as pnnx writes them:
// size=(N, C, H, W), align_corners= (None reads as False).  The output operand's shape in the file is the truth; size= must agree with it, its
// leading entry following a re-batch the way Layout's shape= does.  The output is a rank-4 tensor and is written in this project's storage
// order for it ([N][W][2][H]).  When its only reader is an F.grid_sample the planner drops this step and hands the sampler theta
// (EngineImpl::FuseAffineGrids): the grid is then never written.
#ifndef SIMPLE_INFER_SRC_LAYER_AFFINE_GRID_H_
#define SIMPLE_INFER_SRC_LAYER_AFFINE_GRID_H_

#include "layer.h"
#include "layer_util.h"
#include "si_grid.h"

namespace SimpleInfer {

class AffineGrid : public Layer {
public:
    virtual Status Init(const pnnx::Operator* op) override;
    virtual Status Validate() override;
    virtual Status Forward(const Tensor& input, Tensor& output) override;

    virtual const char* KernelName() const override;
    virtual bool HalfStorageOk(std::string& why) const override;
    virtual double Flops() const override;

public:
    std::vector<int> size_;        // size= as the file has it
    bool align_corners_ = false;

private:
    bool MakeDesc(const Tensor& theta, const Tensor& out, SiAffineGridDesc& d) const;
};

}  // namespace SimpleInfer

#endif
