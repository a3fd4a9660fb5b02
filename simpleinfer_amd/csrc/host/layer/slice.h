// layer/slice.h -- torch.chunk, torch.split and Tensor.slice (torch semantics, no reference counterpart), one class.  `dim` is the file's
// NCHW dimension (negative: from the end) and maps to NHWC as Cat::NhwcAxis does; rank 4 on every axis, rank 2 on dim 1.
//
// The parameter keys are pnnx's spellings for the operators it passes through -- no pnnx converter was at hand to confirm them on an export:
//   torch.chunk    chunks= dim=                           pieces of ceil(size / chunks), the last one may be smaller (torch's rule)
//   torch.split    split_size_or_sections= dim=           an int (a smaller last piece) or a list that sums to the size
//   Tensor.slice   dim= start= end= step=                 or   dims=(..) starts=(..) ends=(..) steps=(..)   (several axes in one operator);
//                  a negative start / end wraps, an end that is missing, None or >= the size (pnnx writes 2147483647) is the size
//
// Forward: an output the engine has pointed at its channel range of the input (EngineImpl::AliasSplits) is skipped -- Cat::Forward makes the
// same test for its inputs; the other pure channel ranges (every step 1) go through ONE si_hip_split_channels_* launch; anything else (H / W / N
// ranges, steps > 1) through si_hip_slice_* per output (include/si_slice.h).
#ifndef SIMPLE_INFER_SRC_LAYER_SLICE_H_
#define SIMPLE_INFER_SRC_LAYER_SLICE_H_

#include "layer.h"
#include "layer_util.h"
#include "si_slice.h"

namespace SimpleInfer {

class Slice : public Layer {
public:
    virtual Status Init(const pnnx::Operator* op) override;
    virtual Status Validate() override;
    virtual Status Forward(const Tensor& input, Tensor& output) override;
    virtual Status Forward(const Tensor& input, std::vector<Tensor>& outputs) override;

    // "view" (every output is in place: no launch), "split_channels", or "slice" -- for the tensors bound now
    virtual const char* KernelName() const override;
    // (no arithmetic: Flops stays 0)

    // one output of the operator: out[i0, i1, i2, i3] = in[start + i * step] per NHWC axis
    struct Piece {
        int start[4] = {0, 0, 0, 0};
        int step[4] = {1, 1, 1, 1};
        int dims[4] = {0, 0, 0, 0};
    };
    // the pieces Validate() derived from the input's shape, one per output
    const std::vector<Piece>& Pieces() const { return pieces_; }
    // a range of channels of every pixel, taken with step 1: what can be a view of the input
    static bool ChannelRange(const Piece& p, const int in_dims[4]);

public:
    enum class Kind { kChunk, kSplit, kSlice };
    Kind kind_ = Kind::kSlice;
    int chunks_ = 0;                       // torch.chunk
    std::vector<int> sections_;            // torch.split: one entry = split_size, several = the sections
    bool sections_is_list_ = false;
    std::vector<int> dims_, starts_, ends_, steps_;   // NCHW dims as the file has them; one entry each for chunk / split (dims_ only)
    std::vector<bool> has_end_;

private:
    Status MakePieces(const int in_dims[4], int rank, std::vector<Piece>& pieces) const;
    // 0: already in place, 1: a channel range to copy, 2: a strided slice
    static int Route(const Piece& p, const int in_dims[4], const Tensor& in, const Tensor& out);
    Status Run(const Tensor& input, const std::vector<Tensor*>& outputs);

    std::vector<Piece> pieces_;
};

}  // namespace SimpleInfer

#endif
