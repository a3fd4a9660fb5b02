// The batch rule (simpleinfer_amd/csrc/host/batch_rule.h) for F.layer_norm (family kRows: over the last dimension, per-image unless that is
// the batch; weight and bias are graph constants [E]) and F.gelu (kElementwise): PerImageOperator with the batch in dimension 0 and 1 of token
// tensors, and in the last dimension, which is refused.
// Stand-alone (the header needs pnnx/ir.h and pnnx/param_read.h only); built with -fsanitize=address,undefined by tests/test_layernorm_cpu.py.
#include <cstdio>
#include <string>
#include <utility>
#include <vector>

#include "batch_rule.h"

using namespace SimpleInfer;

static int failures = 0;
#define EXPECT(cond) \
    do { if (!(cond)) { std::printf("%s:%d: EXPECT(%s) failed\n", __FILE__, __LINE__, #cond); ++failures; } } while (0)

using Ints = std::vector<int>;

static BatchOperand Opd(Ints shape, int axis, bool constant = false) {
    BatchOperand b;
    b.shape = std::move(shape);
    b.axis = axis;
    b.constant = constant;
    return b;
}

static bool Has(const std::string& text, const char* part) { return text.find(part) != std::string::npos; }

int main() {
    EXPECT(BatchFamilyOf("F.layer_norm") == BatchFamily::kRows && BatchFamilyOf("F.gelu") == BatchFamily::kElementwise);
    // the module spellings have no row yet
    EXPECT(BatchFamilyOf("nn.LayerNorm") == BatchFamily::kUnknown && BatchFamilyOf("nn.GELU") == BatchFamily::kUnknown);
    std::string why;
    pnnx::Operator ln;
    ln.type = "F.layer_norm";
    ln.name = "ln";
    ln.params["normalized_shape"] = Ints{32};
    ln.params["eps"] = 1e-5f;
    const BatchOperand w = Opd({32}, -1, true), b = Opd({32}, -1, true);
    // batch-first tokens, seq-first tokens, [N, F]; with both constants, one, none
    EXPECT(PerImageOperator(&ln, {Opd({4, 16, 32}, 0), w, b}, {Opd({4, 16, 32}, 0)}, 4, why) && why.empty());
    EXPECT(PerImageOperator(&ln, {Opd({16, 4, 32}, 1), w, b}, {Opd({16, 4, 32}, 1)}, 4, why) && why.empty());
    EXPECT(PerImageOperator(&ln, {Opd({4, 32}, 0), w}, {Opd({4, 32}, 0)}, 4, why) && why.empty());
    EXPECT(PerImageOperator(&ln, {Opd({4, 32}, 0)}, {Opd({4, 32}, 0)}, 4, why) && why.empty());
    // a constant [E] with E == the batch is still no image
    EXPECT(PerImageOperator(&ln, {Opd({4, 16, 4}, 0), Opd({4}, -1, true)}, {Opd({4, 16, 4}, 0)}, 4, why) && why.empty());
    // the batch in the last dimension: the norm runs over the images
    EXPECT(!PerImageOperator(&ln, {Opd({16, 32, 4}, 2)}, {Opd({16, 32, 4}, 2)}, 4, why) && Has(why, "the last dimension, which is the batch"));
    EXPECT(!PerImageOperator(&ln, {Opd({32, 4}, 1)}, {Opd({32, 4}, 1)}, 4, why) && Has(why, "the last dimension, which is the batch"));
    // ... and with constants, whose extent then lies along the batch
    EXPECT(!PerImageOperator(&ln, {Opd({32, 4}, 1), Opd({4}, -1, true)}, {Opd({32, 4}, 1)}, 4, why) && !why.empty());
    // a weight that is an activation carrying no batch is one value against every image (the layer refuses it as well)
    EXPECT(!PerImageOperator(&ln, {Opd({4, 16, 32}, 0), Opd({32}, -1)}, {Opd({4, 16, 32}, 0)}, 4, why) && Has(why, "no batch dimension"));

    pnnx::Operator gelu;
    gelu.type = "F.gelu";
    gelu.name = "act";
    gelu.params["approximate"] = "tanh";
    for (int axis : {0, 1, 2}) EXPECT(PerImageOperator(&gelu, {Opd({4, 4, 4}, axis)}, {Opd({4, 4, 4}, axis)}, 4, why) && why.empty());
    EXPECT(!PerImageOperator(&gelu, {Opd({4, 16, 32}, 0)}, {Opd({64, 32}, -1)}, 4, why) && Has(why, "does not carry the batch"));

    std::printf(failures ? "%d failures\n" : "layernorm rule ok\n", failures);
    return failures ? 1 : 0;
}
