// The typed pnnx parameter readers (simpleinfer_amd/csrc/host/pnnx/param_read.h) on hand-built operators: every reader on a missing key, a
// type-0 parameter, the string "None", an int, a float, a bool, a list and a string -- the outcome, and that a refused read leaves the
// caller's default as it was.  Stand-alone (the header needs ir.h only); built with -fsanitize=address,undefined by tests/test_param_read_cpu.py.
#include <cstdio>
#include <string>
#include <vector>

#include "pnnx/param_read.h"

using namespace SimpleInfer;

static int failures = 0;
#define EXPECT(cond)                                                            \
    do {                                                                        \
        if (!(cond)) {                                                          \
            std::printf("%s:%d: EXPECT(%s) failed\n", __FILE__, __LINE__, #cond); \
            ++failures;                                                         \
        }                                                                       \
    } while (0)

// one key per kind of value; "missing" is not there
static const char* const kKeys[] = {"missing", "zero", "none", "i", "f", "b", "l", "s"};

static pnnx::Operator MakeOp() {
    pnnx::Operator op;
    op.params["zero"] = pnnx::Parameter();
    op.params["none"] = pnnx::Parameter("None");
    op.params["i"] = pnnx::Parameter(7);
    op.params["f"] = pnnx::Parameter(2.5f);
    op.params["b"] = pnnx::Parameter(true);
    op.params["l"] = pnnx::Parameter(std::vector<int>{1, 2, 3});
    op.params["s"] = pnnx::Parameter("reflect");
    return op;
}

// Get(op, key, v) succeeds on `good` (and `also`, for the strings) and gives the value; on every other key it fails and v keeps `dflt`
template <typename T>
static void CheckGet(const pnnx::Operator& op, const char* good, const T& dflt, const T& want, const char* also = "", const T& also_want = T()) {
    for (const char* key : kKeys) {
        T v = dflt;
        const bool ok = Get(&op, key, v);
        if (std::string(key) == good) {
            EXPECT(ok && v == want);
        } else if (std::string(key) == also) {
            EXPECT(ok && v == also_want);
        } else {
            EXPECT(!ok && v == dflt);
        }
    }
    T v = dflt;
    EXPECT(!Get(nullptr, good, v) && v == dflt);
}

int main() {
    const pnnx::Operator op = MakeOp();

    CheckGet<bool>(op, "b", false, true);
    CheckGet<int>(op, "i", -3, 7);
    CheckGet<float>(op, "f", -1.5f, 2.5f);
    CheckGet<std::string>(op, "s", "dflt", "reflect", "none", "None");   // ("None" is a string like any other to the string reader)
    CheckGet<std::vector<int>>(op, "l", {9}, {1, 2, 3});

    // FindParam: presence, and presence with a type
    EXPECT(FindParam(&op, "missing") == nullptr && FindParam(nullptr, "i") == nullptr);
    EXPECT(FindParam(&op, "zero") != nullptr && FindParam(&op, "zero")->type == 0);
    EXPECT(FindParam(&op, "i", 2) != nullptr && FindParam(&op, "i", 3) == nullptr && FindParam(&op, "l", 5)->ai.size() == 3);

    // the two rules for "not given": they differ on the string "None" alone
    for (const char* key : kKeys) {
        const std::string k = key;
        const bool absent = k == "missing" || k == "zero";
        EXPECT(IsNone(&op, key) == absent);
        EXPECT(IsNoneOrText(&op, key) == (absent || k == "none"));
    }
    EXPECT(!IsNoneOrText(&op, "s"));   // another string is a value

    // GetNumber: a float or an int; everything else, "None" included, is refused and the default stays
    for (const char* key : kKeys) {
        const std::string k = key;
        float v = -1.5f;
        const bool ok = GetNumber(&op, key, v);
        if (k == "f") EXPECT(ok && v == 2.5f);
        else if (k == "i") EXPECT(ok && v == 7.0f);
        else EXPECT(!ok && v == -1.5f);
    }

    // Number: not given (missing, type 0, "None") is fine with have == false and the default untouched; a float or an int is read;
    // another type is an error, again with have == false and the default untouched
    for (const char* key : kKeys) {
        const std::string k = key;
        float v = -1.5f;
        bool have = true;
        const bool ok = Number(&op, key, v, have);
        if (k == "missing" || k == "zero" || k == "none") EXPECT(ok && !have && v == -1.5f);
        else if (k == "f") EXPECT(ok && have && v == 2.5f);
        else if (k == "i") EXPECT(ok && have && v == 7.0f);
        else EXPECT(!ok && !have && v == -1.5f);   // bool, list, string
    }

    // OptionalInt: the same with an int alone; a float is an error
    for (const char* key : kKeys) {
        const std::string k = key;
        int v = -3;
        bool have = true;
        const bool ok = OptionalInt(&op, key, v, have);
        if (k == "missing" || k == "zero" || k == "none") EXPECT(ok && !have && v == -3);
        else if (k == "i") EXPECT(ok && have && v == 7);
        else EXPECT(!ok && !have && v == -3);   // float, bool, list, string
    }

    // the narrow rule followed by a typed read, as Pad2d's `value` and Upsample's keys do it: "None" as text is refused, not skipped
    {
        float v = 0.25f;
        EXPECT(!IsNone(&op, "none") && !GetNumber(&op, "none", v) && v == 0.25f);
        EXPECT(IsNone(&op, "zero") && IsNone(&op, "missing"));
    }

    if (failures) {
        std::printf("%d failures\n", failures);
        return 1;
    }
    std::printf("param read ok\n");
    return 0;
}
