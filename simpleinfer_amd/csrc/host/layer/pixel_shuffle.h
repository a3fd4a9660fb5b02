// layer/pixel_shuffle.h -- nn.PixelShuffle / F.pixel_shuffle (depth-to-space) and nn.PixelUnshuffle / F.pixel_unshuffle (space-to-depth;
// torch semantics, no reference counterpart), one class -- si_hip_pixel_shuffle_f32 / _f16 (include/si_superres.h), one launch, bits
// moved as they are.  The parameter keys are torch's constructor / functional argument names, which is what pnnx writes for the
// modules it passes through: `upscale_factor` for the shuffle, `downscale_factor` for the unshuffle (an int).
#ifndef SIMPLE_INFER_SRC_LAYER_PIXEL_SHUFFLE_H_
#define SIMPLE_INFER_SRC_LAYER_PIXEL_SHUFFLE_H_

#include "layer.h"
#include "layer_util.h"
#include "si_superres.h"

namespace SimpleInfer {

class PixelShuffle : public Layer {
public:
    virtual Status Init(const pnnx::Operator* op) override;
    virtual Status Validate() override;
    virtual Status Forward(const Tensor& input, Tensor& output) override;

    virtual const char* KernelName() const override;
    // (Bytes: the base class's input bytes plus output bytes; no arithmetic: Flops stays 0)

public:
    int factor_ = 1;         // upscale_factor / downscale_factor
    bool inverse_ = false;   // nn.PixelUnshuffle / F.pixel_unshuffle

private:
    bool MakeDesc(const Tensor& input, const Tensor& output, SiPixelShuffleDesc& d) const;
};

}  // namespace SimpleInfer

#endif
