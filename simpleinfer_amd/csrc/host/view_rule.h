// view_rule.h -- which rows the fp16 launches take.  Concat and split aliasing turn an operand into a channel slice of a wider buffer: its pixel
// stride `ld` becomes the parent's channel count and it starts `off` channels into the row.  The fp16 entries that read or write through 16-byte
// vectors answer SI_E_UNSUPPORTED for a row that is no whole number of them (8 halves); where the layer has no second launch to go to, that
// answer would be a failing Forward() on a model that loaded.  The planner therefore puts the question here BEFORE it makes the view
// (Layer::TakesView, asked by EngineImpl::AliasConcats / AliasSplits of every step that touches the operand): a declined view costs the copy
// the concat or the split launches anyway.  Pure functions of a few integers, no device: tests/cpp/test_view_rule.cpp spells the table out.
//
// The table restates the entries' own preconditions (csrc/hip):
//   si_hip_conv2d_f16 / _split_f16 / _upcat_f16   in_ld % 8, up.ld % 8; out_ld, out2_ld, res_ld any (2-byte stores and loads)
//   si_hip_conv2d_depthwise_f16                   in_ld, out_ld, res_ld % 8
//   si_hip_conv2d_pw_slab_f16 (patch or slab)     in_ld % 8 (the two launches behind a refusal read the same row: no second choice);
//                                                 out_ld % 8 and res_ld % 4 on the slab form, res_ld % 2 on the patch form -- refused there,
//                                                 the pair runs as its two launches (Conv2d::Launch), which take any out_ld and res_ld
//   si_hip_conv2d_pw_cv3_f16                      in_ld % 8, z_ld % 8, res_ld % 2; out_ld any.  No second launch
//   the stem-fused launches                       read the fp32 image; 2-byte stores at any out_ld
//   si_hip_binary_bcast_f16                       a_ld, s_ld, out_ld % 8
// A row of whole vectors is taken by every entry, so no plan whose rows are multiples of 8 halves changes.
#ifndef SIMPLE_INFER_SRC_VIEW_RULE_H_
#define SIMPLE_INFER_SRC_VIEW_RULE_H_

namespace SimpleInfer {

// the fp16 launch a conv step makes
enum class HalfConvForm { kIgemm = 0, kDepthwise, kPair, kCv3, kStemFused };
// the part an operand plays in it
enum class ConvOperand { kInput = 0, kOutput, kResidual, kUpsampledSource, kCv3Z };

constexpr int kHalfVector = 8;   // halves in a 16-byte vector

// rows and slice starts in whole 16-byte vectors: what every vector-reading entry asks of a view
inline bool HalfVectorRow(int ld, int off) { return ld > 0 && off >= 0 && ld % kHalfVector == 0 && off % kHalfVector == 0; }

// does the launch of `form` take `operand` as half data at pixel stride `ld`, `off` channels into the row -- itself, or through a second
// launch the layer has for a refusal?
inline bool HalfConvTakesView(HalfConvForm form, ConvOperand operand, int ld, int off) {
    if (ld <= 0 || off < 0) return false;
    if (HalfVectorRow(ld, off)) return true;
    switch (form) {
        case HalfConvForm::kIgemm:
            return operand == ConvOperand::kOutput || operand == ConvOperand::kResidual;
        case HalfConvForm::kDepthwise:
            return false;
        case HalfConvForm::kPair:
            return operand == ConvOperand::kOutput || operand == ConvOperand::kResidual;
        case HalfConvForm::kCv3:
            return operand == ConvOperand::kOutput || (operand == ConvOperand::kResidual && ld % 2 == 0 && off % 2 == 0);
        case HalfConvForm::kStemFused:
            return operand == ConvOperand::kOutput;
    }
    return false;
}

// fp32 storage: the routes have a second launch for a refused input row (the Winograd re-pack, f32_split's demotion, the implicit GEMM's scalar
// loads); the dual-source form alone has none -- si_hip_conv2d_upcat_f32 reads the low-resolution source in 16-byte vectors (up.ld % 4)
inline bool FloatUpsampledSourceTakesView(int ld, int off) { return ld > 0 && off >= 0 && ld % 4 == 0 && off % 4 == 0; }

// BinaryOp's per-image channel vector form (the squeeze-excite scale): all three operands in whole vectors
inline bool HalfBroadcastTakesView(int ld, int off) { return HalfVectorRow(ld, off); }

}  // namespace SimpleInfer

#endif  // SIMPLE_INFER_SRC_VIEW_RULE_H_
