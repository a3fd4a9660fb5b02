// layer/grid_sample.h -- F.grid_sample (torch semantics; no reference counterpart) on the MI355X: one launch of si_hip_grid_sample_f32 / _f16
// (include/si_grid.h).  4-D inputs, bilinear and nearest, the three padding modes, align_corners both ways; bicubic and 5-D inputs are
// kUnsupport at load.  Parameters as pnnx writes them: mode=, padding_mode= (strings), align_corners= (None reads as False).
//
// The grid operand [N, Ho, Wo, 2] is a rank-4 tensor, which this project stores as [N][Wo][2][Ho]: on its own the layer hands the kernel the
// strides of that image.  Two planner passes (engine_plan.cpp) replace the second input:
//   SetGridInPlace(root)   the grid came through permute(0, 2, 3, 1) from `root` [N, 2, Ho, Wo], whose NHWC storage already is torch's dense
//                          grid: the layout step is gone and the kernel reads root with the strides (Ho Wo ld, Wo ld, ld, 1)
//   SetTheta(theta)        the grid came from F.affine_grid(theta) with the sampler's own align_corners: the affine step is gone, the kernel
//                          computes the coordinates from theta [N, 2, 3] and the grid is never written
#ifndef SIMPLE_INFER_SRC_LAYER_GRID_SAMPLE_H_
#define SIMPLE_INFER_SRC_LAYER_GRID_SAMPLE_H_

#include "layer.h"
#include "layer_util.h"
#include "si_grid.h"

namespace SimpleInfer {

class GridSample : public Layer {
public:
    enum class GridForm { kStored, kInPlace, kTheta };

    virtual Status Init(const pnnx::Operator* op) override;
    virtual Status Validate() override;
    virtual Status Forward(const std::vector<Tensor>& inputs, Tensor& output) override;

    virtual const char* KernelName() const override;
    virtual bool HalfStorageOk(std::string& why) const override;
    virtual double Flops() const override;
    virtual double Bytes() const override;

    // planner hooks (see above); false: `root` / `theta` does not have the shape the form needs, and nothing has changed
    bool SetGridInPlace(TensorNode* root);
    bool SetTheta(TensorNode* theta);
    GridForm Form() const { return form_; }

public:
    int mode_ = SI_GRID_BILINEAR;
    int padding_mode_ = SI_GRID_PAD_ZEROS;
    bool align_corners_ = false;

private:
    // false: the operands are not tensors the descriptor can be made of
    bool MakeDesc(const Tensor& x, const Tensor& grid, const Tensor& out, SiGridSampleDesc& d) const;

    GridForm form_ = GridForm::kStored;
};

}  // namespace SimpleInfer

#endif
