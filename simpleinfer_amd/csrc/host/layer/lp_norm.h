// layer/lp_norm.h -- F.normalize and torch.norm (torch semantics; no reference counterpart), one class -- si_hip_lpnorm_f32 / _f16
// (include/si_lpnorm.h), one launch.  Parameters as pnnx writes them:
//   F.normalize   `dim` int, `eps` float, `p` float
//   torch.norm    `dim` int or int array, `keepdim` bool, `p` int or float; `dtype`, if present, must be None
// p is 1, 2 or inf in either numeric spelling (2 / 2.0; inf arrives as the text "inf"); the text "fro" is p = 2.  Any other p (0, -inf, 3,
// "nuc"), a missing dim on torch.norm (the reduction to a scalar) and a dtype are kUnsupport with the reason logged; a mistyped key is
// kFail.  The file's dims are NCHW (or [N, F]); Validate maps each to its NHWC axis as Softmax::NhwcAxis does and checks the file's
// output shape against the rule.
//
// torch.norm with keepdim=False is served exactly where the result is the same memory as the keepdim result (rank 4 is stored NHWC, every
// other rank dense row-major, include/si_layout.h): dim=1 of a rank-4 input, whose [N, H, W] result is the [N, H, W, 1] the kernel writes
// (SuperPoint's descriptor norm), and dims (2, 3) of a rank-4 input, whose [N, C] result is the [N, 1, 1, C] memory.  Every other
// keepdim=False, a rank-1 result included, is kUnsupport at load.
//
// The planner pass FuseNormDivisions (option fuse_norm) turns torch.norm -> [torch.unsqueeze] -> BinaryOp div into this layer's normalize
// form with eps = 0: SetNormalize.
#ifndef SIMPLE_INFER_SRC_LAYER_LP_NORM_H_
#define SIMPLE_INFER_SRC_LAYER_LP_NORM_H_

#include "layer.h"
#include "layer_util.h"
#include "si_lpnorm.h"

namespace SimpleInfer {

class LpNorm : public Layer {
public:
    virtual Status Init(const pnnx::Operator* op) override;
    virtual Status Validate() override;
    virtual Status Forward(const Tensor& input, Tensor& output) override;

    virtual const char* KernelName() const override;
    virtual double Flops() const override;
    // (Bytes: the base class's one read of the input plus one write of the output.  HalfStorageOk: the base class's -- halves in and
    // out run the fp16 kernel; a mixed pair at the graph boundary goes through the engine's fp32 fallback, as for Reduce)

    // torch.norm over one dim whose result only divides its own input: the launch writes x / norm into `out` (x's shape) instead of the
    // norm.  false, and nothing changed: not a torch.norm over a single axis, or `out` has another shape than the input
    bool SetNormalize(TensorNode* out);
    bool Normalizes() const { return normalize_; }

public:
    int p_ = SI_LPNORM_P2;       // SI_LPNORM_P*
    std::vector<int> dims_;      // as the file has them
    bool keepdim_ = false;       // torch.norm
    bool normalize_ = false;     // F.normalize, or a fused torch.norm
    float eps_ = 0.0f;           // F.normalize
    int axes_ = 0;               // the NHWC mask, set by Validate

private:
    bool MakeDesc(const Tensor& input, const Tensor& output, SiLpNormDesc& d) const;
};

}  // namespace SimpleInfer

#endif
