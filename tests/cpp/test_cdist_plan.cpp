// The host arithmetic of torch.cdist: cdist_plan.h (simpleinfer_amd/csrc/hip: refusals, the kernel choice, the vector rule, extents next to
// 2^31, the grid) and the family kCdist of the batch rule (simpleinfer_amd/csrc/host/batch_rule.h).
// Stand-alone (plain C++ headers only); built with -fsanitize=address,undefined by tests/test_cdist_cpu.py.
#include <cstdio>
#include <string>
#include <utility>
#include <vector>

#include "batch_rule.h"
#include "cdist_plan.h"

using namespace SimpleInfer;
namespace plan = si_cdist_plan;

static int failures = 0;
#define EXPECT(cond) \
    do { if (!(cond)) { std::printf("%s:%d: EXPECT(%s) failed\n", __FILE__, __LINE__, #cond); ++failures; } } while (0)

using Ints = std::vector<int>;

// dense operands [b1, p, m] and [b2, r, m]
static SiCdistDesc Desc(int b1, int b2, int p, int r, int m, int norm = SI_CDIST_NORM_2, int mode = SI_CDIST_MODE_MM_IF_NECESSARY) {
    SiCdistDesc d = {};
    d.b1 = b1; d.b2 = b2; d.p = p; d.r = r; d.m = m;
    d.x1_ld = d.x2_ld = m; d.out_ld = r;
    d.x1_sb = (int)((long long)p * m); d.x2_sb = (int)((long long)r * m); d.out_sb = (int)((long long)p * r);
    d.norm = norm; d.mode = mode;
    return d;
}

static BatchOperand Opd(Ints shape, int axis, bool constant = false) {
    BatchOperand b;
    b.shape = std::move(shape);
    b.axis = axis;
    b.constant = constant;
    return b;
}

static bool Has(const std::string& text, const char* part) { return text.find(part) != std::string::npos; }

int main() {
    // ---- the plan
    EXPECT(plan::Check(Desc(3, 3, 5, 4, 8)) == 0 && plan::Check(Desc(1, 3, 5, 4, 8)) == 0 && plan::Check(Desc(3, 1, 5, 4, 8)) == 0);
    EXPECT(plan::Check(Desc(3, 2, 5, 4, 8)) == SI_E_BADARG && plan::Check(Desc(0, 1, 5, 4, 8)) == SI_E_BADARG && plan::Check(Desc(1, 1, 5, 4, 0)) == SI_E_BADARG);
    for (int norm : {0, 4, -1}) EXPECT(plan::Check(Desc(1, 1, 5, 4, 8, norm)) == SI_E_UNSUPPORTED);
    EXPECT(plan::Check(Desc(1, 1, 5, 4, 8, SI_CDIST_NORM_2, 3)) == SI_E_UNSUPPORTED);
    // a bad stride is looked for before an unsupported norm
    SiCdistDesc d = Desc(1, 1, 5, 4, 8, 0);
    d.x2_ld = 7;
    EXPECT(plan::Check(d) == SI_E_BADARG);
    // next to 2^31: the last element offset of every view is at most 2^31 - 1
    EXPECT(plan::Check(Desc(1, 1, 1 << 15, 1 << 15, 8)) == 0);                       // 2^30 outputs
    EXPECT(plan::Check(Desc(1, 1, 1 << 16, 1 << 15, 8)) == SI_E_UNSUPPORTED);        // 2^31 outputs: one past
    EXPECT(plan::Check(Desc(1, 1, (1 << 16) - 1, 1 << 15, 8)) == 0);                 // 2^31 - 2^15
    d = Desc(1, 1, 1, 1, 0x7fffffff);                                                // one row of 2^31 - 1 elements on each side
    EXPECT(plan::Check(d) == 0 && plan::FormOf(d) == plan::kDirect && plan::OperandExtent(1, 1, d.m, 0, d.m) == plan::kIndexLimit);
    d.r = d.out_ld = 2;                                                              // ... and a second row of x2
    EXPECT(plan::Check(d) == SI_E_UNSUPPORTED && plan::FormOf(d) == plan::kNone);
    d = Desc(1, 1, 2, 1, 1 << 30);                                                   // x1: 2 rows of 2^30 = 2^31 elements
    EXPECT(plan::Check(d) == SI_E_UNSUPPORTED);
    d.x1_ld = (1 << 30) - 1;
    EXPECT(plan::Check(d) == SI_E_BADARG);
    d = Desc(2, 2, 1 << 14, 4, 1 << 16);                                             // the second batch item of x1 ends at 2^31
    EXPECT(plan::Check(d) == SI_E_UNSUPPORTED);
    d = Desc(2, 1, (1 << 14) - 1, 4, 1 << 16);
    d.x1_sb = 1 << 30;
    EXPECT(plan::Check(d) == 0 && plan::OperandExtent(2, d.p, d.m, d.x1_sb, d.x1_ld) == (1ull << 31) - (1u << 16));
    // torch's mode rule, from the descriptor alone
    EXPECT(plan::FormOf(Desc(1, 1, 25, 25, 8)) == plan::kDirect && plan::FormOf(Desc(1, 1, 26, 1, 8)) == plan::kMm && plan::FormOf(Desc(1, 1, 1, 26, 8)) == plan::kMm);
    EXPECT(plan::FormOf(Desc(1, 1, 2, 2, 8, SI_CDIST_NORM_2, SI_CDIST_MODE_MM)) == plan::kMm);
    EXPECT(plan::FormOf(Desc(1, 1, 99, 99, 8, SI_CDIST_NORM_2, SI_CDIST_MODE_NO_MM)) == plan::kDirect);
    EXPECT(plan::FormOf(Desc(1, 1, 99, 99, 8, SI_CDIST_NORM_1, SI_CDIST_MODE_MM)) == plan::kDirect && plan::FormOf(Desc(1, 1, 99, 99, 8, 0)) == plan::kNone);
    // the vector rule
    d = Desc(3, 1, 64, 64, 8);
    EXPECT(plan::Vector(d, 4, 256, 512) && plan::Vector(d, 8, 256, 512) && !plan::Vector(d, 4, 260, 512) && !plan::Vector(d, 4, 256, 520));
    d.x1_sb += 2;
    EXPECT(!plan::Vector(d, 4, 256, 512));
    d = Desc(1, 3, 64, 64, 12);
    EXPECT(plan::Vector(d, 4, 256, 512) && !plan::Vector(d, 8, 256, 512));
    // overlap of out with either operand, in bytes
    d = Desc(1, 1, 5, 4, 8);
    EXPECT(plan::Overlaps(d, 1000, 2000, 1000 + 159, 4) && !plan::Overlaps(d, 1000, 2000, 1000 + 160, 4) && plan::Overlaps(d, 1000, 2000, 2000 - 79, 4) &&
           !plan::Overlaps(d, 1000, 2000, 2000 + 128, 4) && plan::Overlaps(d, 1000, 2000, 2000 + 63, 2));
    // the grid: p tiles rounded up to 8, times the r tiles; z capped
    plan::Grid g = plan::MakeGrid(Desc(70000, 70000, 65, 129, 8));
    EXPECT(g.p_tiles == 2 && g.r_tiles == 3 && g.x == 24 && g.z == 65535);
    g = plan::MakeGrid(Desc(1, 1, (1 << 16) - 1, 1 << 15, 8));
    EXPECT(g.p_tiles == 1024 && g.r_tiles == 512 && g.x == 1024u * 512u && g.z == 1);

    // ---- the batch rule
    EXPECT(BatchFamilyOf("torch.cdist") == BatchFamily::kCdist && BatchFamilyOf("F.pairwise_distance") == BatchFamily::kUnknown);
    std::string why;
    pnnx::Operator op;
    op.type = "torch.cdist";
    op.name = "dist";
    // rank-3 operands, and a rank-2 / rank-3 constant with batch extent 1: per-image over dimension 0
    EXPECT(PerImageOperator(&op, {Opd({4, 16, 32}, 0), Opd({4, 9, 32}, 0)}, {Opd({4, 16, 9}, 0)}, 4, why) && why.empty());
    EXPECT(PerImageOperator(&op, {Opd({4, 16, 32}, 0), Opd({40, 32}, -1, true)}, {Opd({4, 16, 40}, 0)}, 4, why) && why.empty());
    EXPECT(PerImageOperator(&op, {Opd({4, 32}, -1, true), Opd({4, 16, 32}, 0)}, {Opd({4, 4, 16}, 0)}, 4, why) && why.empty());
    EXPECT(PerImageOperator(&op, {Opd({4, 16, 32}, 0), Opd({1, 40, 32}, -1, true)}, {Opd({4, 16, 40}, 0)}, 4, why) && why.empty());
    EXPECT(PerImageOperator(&op, {Opd({4, 32}, 0), Opd({40, 32}, -1, true)}, {Opd({4, 40}, 0)}, 4, why) && why.empty());     // rows against a codebook
    // a constant with one slice per image; the batch in the points' dimension; an activation without a batch
    EXPECT(!PerImageOperator(&op, {Opd({4, 16, 32}, 0), Opd({4, 40, 32}, -1, true)}, {Opd({4, 16, 40}, 0)}, 4, why) && Has(why, "one slice of itself"));
    EXPECT(!PerImageOperator(&op, {Opd({16, 4, 32}, 1), Opd({16, 4, 32}, 1)}, {Opd({16, 4, 4}, 1)}, 4, why) && Has(why, "dimension 1"));
    EXPECT(!PerImageOperator(&op, {Opd({4, 16, 32}, 0), Opd({9, 32}, -1)}, {Opd({4, 16, 9}, 0)}, 4, why) && Has(why, "no batch dimension"));
    // two rank-2 activations: never, whatever the shapes say
    EXPECT(!PerImageOperator(&op, {Opd({4, 32}, 0), Opd({4, 32}, 0)}, {Opd({4, 4}, 0)}, 4, why) && why == CdistBatchReason());
    EXPECT(!PerImageOperator(&op, {Opd({4, 32}, 0), Opd({9, 32}, -1)}, {Opd({4, 9}, 0)}, 4, why) && Has(why, "counts points"));

    // HasPointSets on a graph's operands
    pnnx::Operand a, b, c;
    a.shape = {4, 32}; b.shape = {9, 32}; c.shape = {4, 9, 32};
    op.inputs = {&a, &b};
    EXPECT(HasPointSets(&op, {}) && !HasPointSets(&op, {&b}));
    op.inputs = {&c, &b};
    EXPECT(!HasPointSets(&op, {}));
    op.type = "BinaryOp";
    op.inputs = {&a, &b};
    EXPECT(!HasPointSets(&op, {}));

    std::printf(failures ? "%d failures\n" : "cdist plan ok\n", failures);
    return failures ? 1 : 0;
}
