// layer/cdist.h -- torch.cdist (torch semantics; no reference counterpart): one launch of si_hip_cdist_f32 / _f16 (include/si_cdist.h).
// Parameters as pnnx writes them: `torch.cdist name 2 1 x1 x2 out compute_mode=None p=2.000000e+00`; `p` a float (an int is read too, inf
// as a float or as the text), `compute_mode` the key `=None` (torch's default, use_mm_for_euclid_dist_if_necessary) or one of torch's three
// strings.  p other than 1, 2, inf and another compute_mode are kUnsupport at Init, with the reason logged.
//
// Served: each operand rank 2 [P, M] or rank 3 [B, P, M] -- token tensors, stored dense in file order, rows of M contiguous elements --
// with equal last dimensions and batch dimensions equal or 1; the output is [B, P, R], or [P, R] for two rank-2 operands.  An operand may be
// a graph constant (pnnx.Attribute): the codebook of a VQ encoder, bound like any tensor and read with batch stride 0.  Another rank, or
// shapes that do not fit, are kErrorShape at LoadModel.  What the batch means (images, or points when both operands are rank-2
// activations) is batch_rule.h's family kCdist.
//
// nearest_rows=1 (written by pnnx/lower_nearest_rows.cpp, never by pnnx): the operator stands for cdist -> argmin -> embedding against the
// constant codebook x2.  The output is [.., P, M], the nearest codebook row of every row of x1, from one launch of si_hip_nearest_f32 / _f16
// (include/si_nearest.h) with the rows output alone and one split -- no workspace, so lanes on two streams share nothing.  p must be 2.
#ifndef SIMPLE_INFER_SRC_LAYER_CDIST_H_
#define SIMPLE_INFER_SRC_LAYER_CDIST_H_

#include "layer.h"
#include "layer_util.h"
#include "si_cdist.h"
#include "si_nearest.h"

namespace SimpleInfer {

class Cdist : public Layer {
public:
    virtual Status Init(const pnnx::Operator* op) override;
    virtual Status Validate() override;
    virtual Status Forward(const std::vector<Tensor>& inputs, Tensor& output) override;

    virtual const char* KernelName() const override;
    virtual double Flops() const override;
    virtual double Bytes() const override;
    // halves in and out run the fp16 kernels when M % 8 == 0 (a lane's matrix-core fragment is 8 consecutive halves); otherwise, and for
    // mixed storage types, the engine runs the layer in fp32 between casts
    virtual bool HalfStorageOk(std::string& why) const override;

public:
    int norm_ = SI_CDIST_NORM_2;
    int mode_ = SI_CDIST_MODE_MM_IF_NECESSARY;
    bool nearest_rows_ = false;

private:
    // the descriptor for a pair of operands and the output; false with `why`: the shapes do not make a cdist
    bool MakeDesc(const Tensor& x1, const Tensor& x2, const Tensor& out, SiCdistDesc& d, std::string* why = nullptr) const;
    Status Refuse(const std::string& why, Status status) const;
    // the search's descriptor from the cdist one of a nearest_rows operator (out's strides are the rows')
    static SiNearestDesc NearestDesc(const SiCdistDesc& d);
};

}  // namespace SimpleInfer

#endif
