// The planner's view rule on its own, without a device (csrc/host/view_rule.h): for every fp16 conv form and operand, and for the broadcast
// BinaryOp, whether a channel slice at pixel stride ld / channel offset off is taken.  The expected answers are spelled out here from the
// kernels' entry checks (conv_igemm_f16.hip dispatch_h and f16_upcat_shape_ok, conv_depthwise_f16.hip, conv_slab_f16.hip slab_shape_ok and
// pw_pair_ok, conv_pw_patch_f16.hip, ops.hip si_hip_binary_bcast_f16) and from which refusals Conv2d::Launch has a second launch for.
// Stand-alone, header only; built by tests/test_view_rule_cpu.py.
#include <cstdio>

#include "view_rule.h"

using SimpleInfer::ConvOperand;
using SimpleInfer::HalfConvForm;

static int failures = 0;
#define EXPECT(cond)                                                            \
    do {                                                                        \
        if (!(cond)) {                                                          \
            std::printf("%s:%d: EXPECT(%s) failed\n", __FILE__, __LINE__, #cond); \
            ++failures;                                                         \
        }                                                                       \
    } while (0)

// by value, not read from the header
enum { fIgemm = 0, fDepthwise, fPair, fCv3, fStemFused, kForms };
enum { oInput = 0, oOutput, oResidual, oUpsampled, oCv3Z, kOperands };
static const char* const kFormNames[] = {"igemm", "depthwise", "pair", "cv3", "stem-fused"};
static const char* const kOperandNames[] = {"input", "output", "residual", "upsampled source", "cv3 z"};

// rows: cat(32, 4, 32) = 68 and cat(128, 4) = 132 halves (even, 8-byte rows), cat(32, 3, 32) = 67 (odd), a split's 20-channel input
struct Row { int ld, off; };
static const Row kVectorRows[] = {{8, 0}, {64, 32}, {72, 40}, {128, 64}, {256, 8}};
static const Row kEvenRows[] = {{68, 0}, {68, 32}, {132, 0}, {20, 0}, {36, 0}, {12, 8}, {4, 0}};
static const Row kOddRows[] = {{67, 0}, {67, 32}, {35, 8}, {9, 0}};

// what is taken at a row that is NOT whole 16-byte vectors: [form][operand], for an even row and for an odd one
static const bool kEven[kForms][kOperands] = {
    /* igemm      */ {false, true, true, false, false},
    /* depthwise  */ {false, false, false, false, false},
    /* pair       */ {false, true, true, false, false},
    /* cv3        */ {false, true, true, false, false},
    /* stem-fused */ {false, true, false, false, false},
};
static const bool kOdd[kForms][kOperands] = {
    /* igemm      */ {false, true, true, false, false},
    /* depthwise  */ {false, false, false, false, false},
    /* pair       */ {false, true, true, false, false},
    /* cv3        */ {false, true, false, false, false},   // (its shortcut is read in pairs of halves)
    /* stem-fused */ {false, true, false, false, false},
};

static void Check(int form, int operand, const Row& r, bool want) {
    const bool got = SimpleInfer::HalfConvTakesView(static_cast<HalfConvForm>(form), static_cast<ConvOperand>(operand), r.ld, r.off);
    if (got == want) return;
    std::printf("[%s, %s] ld %d off %d: %s, expected %s\n", kFormNames[form], kOperandNames[operand], r.ld, r.off, got ? "taken" : "declined",
                want ? "taken" : "declined");
    ++failures;
}

int main() {
    EXPECT((int)HalfConvForm::kIgemm == fIgemm && (int)HalfConvForm::kDepthwise == fDepthwise && (int)HalfConvForm::kPair == fPair &&
           (int)HalfConvForm::kCv3 == fCv3 && (int)HalfConvForm::kStemFused == fStemFused);
    EXPECT((int)ConvOperand::kInput == oInput && (int)ConvOperand::kOutput == oOutput && (int)ConvOperand::kResidual == oResidual &&
           (int)ConvOperand::kUpsampledSource == oUpsampled && (int)ConvOperand::kCv3Z == oCv3Z);
    int asked = 0;
    for (int f = 0; f < kForms; ++f)
        for (int o = 0; o < kOperands; ++o) {
            // whole vectors: every entry takes them, so no plan over such rows changes
            for (const Row& r : kVectorRows) Check(f, o, r, true), ++asked;
            for (const Row& r : kEvenRows) Check(f, o, r, kEven[f][o]), ++asked;
            for (const Row& r : kOddRows) Check(f, o, r, kOdd[f][o]), ++asked;
            // a slice start off the vector grid is no better than a row off it
            Check(f, o, Row{64, 4}, kEven[f][o]), ++asked;
            Check(f, o, Row{64, 3}, kOdd[f][o]), ++asked;
            // nonsense is declined
            Check(f, o, Row{0, 0}, false), ++asked;
            Check(f, o, Row{64, -8}, false), ++asked;
        }
    for (const Row& r : kVectorRows) EXPECT(SimpleInfer::HalfBroadcastTakesView(r.ld, r.off));
    for (const Row& r : kEvenRows) EXPECT(!SimpleInfer::HalfBroadcastTakesView(r.ld, r.off));
    for (const Row& r : kOddRows) EXPECT(!SimpleInfer::HalfBroadcastTakesView(r.ld, r.off));
    EXPECT(!SimpleInfer::HalfBroadcastTakesView(64, 4) && !SimpleInfer::HalfBroadcastTakesView(0, 0));
    // fp32: the dual-source form's low-resolution source in 16-byte vectors of four floats (68 = 64 + 4 is one, 67 = 64 + 3 is none)
    EXPECT(SimpleInfer::FloatUpsampledSourceTakesView(68, 0) && SimpleInfer::FloatUpsampledSourceTakesView(132, 64) && SimpleInfer::FloatUpsampledSourceTakesView(64, 32));
    EXPECT(!SimpleInfer::FloatUpsampledSourceTakesView(67, 0) && !SimpleInfer::FloatUpsampledSourceTakesView(131, 0) && !SimpleInfer::FloatUpsampledSourceTakesView(68, 2) &&
           !SimpleInfer::FloatUpsampledSourceTakesView(0, 0) && !SimpleInfer::FloatUpsampledSourceTakesView(68, -4));
    if (failures) {
        std::printf("%d failure(s)\n", failures);
        return 1;
    }
    std::printf("view rule ok (%d questions)\n", asked);
    return 0;
}
