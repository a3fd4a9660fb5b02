// The engine's options as a value type (simpleinfer_amd/csrc/host/engine_options.h) on its own: the defaults, the set of keys, that every key sets
// exactly its own field by its own rule, and what a child engine (a half-batch lane, the sliced pipeline's engine) inherits.  Everything expected
// is spelled out here, not read from the header.  Stand-alone; built with -fsanitize=address,undefined by tests/test_engine_options_cpu.py.
#include <cctype>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "engine_options.h"

using SimpleInfer::EngineOptions;

static int failures = 0;
#define EXPECT(cond)                                                            \
    do {                                                                        \
        if (!(cond)) {                                                          \
            std::printf("%s:%d: EXPECT(%s) failed\n", __FILE__, __LINE__, #cond); \
            ++failures;                                                         \
        }                                                                       \
    } while (0)

// Every field of the struct by name, the ten members of `plan` included, in one fixed order: what "a field changed" is measured on.  A field
// that is added to EngineOptions is added here, to kDefaults and to Flat, and its key to kKeys.
static const char* const kFields[] = {"device", "batch", "streams", "host_slices", "pin_inputs", "fail_slicer", "fuse", "fuse_upsample", "fuse_stem",
                                      "fuse_pw", "fuse_layout", "fuse_grid", "alias_cat", "alias_split", "alias_view", "f32_split", "f32_split_policy",
                                      "fp16", "arena", "graph", "outputs_to_host", "winograd", "detect_stream", "detect_priority", "plan_set",
                                      "f32_tile", "wino23_form", "wino23_ocg", "f16_tile", "f16_detect_tile", "f16_s2c32", "f16_slab", "f16_slab_w2",
                                      "f16_pw_patch", "split3_bm"};
static const int kDefaults[] = {-1, 0, 1, 0, 0, 0, 1, 1, 2, 1, 1, 1, 1, 1, 1, 0, 4, 0, 1, 0, 1, 1, 1, 0, 0, -1, 0, 0, -1, -1, -1, -1, -1, -1, 0};
static const size_t kNumFields = sizeof(kFields) / sizeof(kFields[0]);
static_assert(sizeof(kDefaults) / sizeof(kDefaults[0]) == kNumFields, "one default per field");

static std::vector<int> Flat(const EngineOptions& o) {
    return {o.device, o.batch, o.streams, o.host_slices, o.pin_inputs, o.fail_slicer, o.fuse, o.fuse_upsample, o.fuse_stem,
            o.fuse_pw, o.fuse_layout, o.fuse_grid, o.alias_cat, o.alias_split, o.alias_view, o.f32_split, o.f32_split_policy,
            o.fp16, o.arena, o.graph, o.outputs_to_host, o.winograd, o.detect_stream, o.detect_priority, o.plan_set,
            o.plan.f32_tile, o.plan.wino23_form, o.plan.wino23_ocg, o.plan.f16_tile, o.plan.f16_detect_tile, o.plan.f16_s2c32, o.plan.f16_slab,
            o.plan.f16_slab_w2, o.plan.f16_pw_patch, o.plan.split3_bm};
}

static size_t FieldIndex(const char* name) {
    for (size_t i = 0; i < kNumFields; ++i)
        if (0 == std::strcmp(kFields[i], name)) return i;
    std::printf("no field [%s]\n", name);
    ++failures;
    return 0;
}

// today's 34 keys: the key, the field it sets, and its rule
enum Rule { kBool, kInt, kSign, kPlan };
struct Key { const char* key; const char* field; Rule rule; };
static const Key kKeys[] = {
    {"fuse", "fuse", kBool}, {"alias_cat", "alias_cat", kBool}, {"alias_split", "alias_split", kBool}, {"fuse_layout", "fuse_layout", kBool},
    {"fuse_grid", "fuse_grid", kBool}, {"alias_view", "alias_view", kBool}, {"graph", "graph", kBool}, {"outputs_to_host", "outputs_to_host", kBool},
    {"fp16", "fp16", kBool}, {"arena", "arena", kBool}, {"fuse_upsample", "fuse_upsample", kBool}, {"f32_split", "f32_split", kBool},
    {"_fail_slicer", "fail_slicer", kBool}, {"pin_inputs", "pin_inputs", kBool},
    {"device", "device", kInt}, {"batch", "batch", kInt}, {"fuse_pw", "fuse_pw", kInt}, {"fuse_stem", "fuse_stem", kInt},
    {"detect_stream", "detect_stream", kInt}, {"f32_split_policy", "f32_split_policy", kInt}, {"winograd", "winograd", kInt},
    {"streams", "streams", kInt}, {"host_slices", "host_slices", kInt},
    {"f32_tile", "f32_tile", kPlan}, {"wino23_form", "wino23_form", kPlan}, {"wino23_ocg", "wino23_ocg", kPlan}, {"f16_tile", "f16_tile", kPlan},
    {"f16_detect_tile", "f16_detect_tile", kPlan}, {"f16_s2c32", "f16_s2c32", kPlan}, {"f16_slab", "f16_slab", kPlan},
    {"f16_slab_w2", "f16_slab_w2", kPlan}, {"f16_pw_patch", "f16_pw_patch", kPlan}, {"split3_bm", "split3_bm", kPlan},
    {"detect_priority", "detect_priority", kSign},
};
static const size_t kNumKeys = sizeof(kKeys) / sizeof(kKeys[0]);
static_assert(kNumKeys == 34, "the 34 keys of SetOption");

static int Expected(Rule rule, int value) {
    if (rule == kBool) return value != 0 ? 1 : 0;
    if (rule == kSign) return value < 0 ? -1 : (value > 0 ? 1 : 0);
    return value;
}

// 1. a default-constructed struct holds the documented defaults
static void Defaults() {
    const std::vector<int> got = Flat(EngineOptions());
    EXPECT(got.size() == kNumFields);
    for (size_t i = 0; i < kNumFields && i < got.size(); ++i) {
        if (got[i] != kDefaults[i]) std::printf("default of [%s]: %d, expected %d\n", kFields[i], got[i], kDefaults[i]);
        EXPECT(got[i] == kDefaults[i]);
    }
}

// 2. Set accepts exactly the 34 keys (each key sets a field of its own -- 3. -- so 34 accepted keys over 34 distinct fields, none twice) and
// nothing else: every field name that is no key, an unknown key, the empty key, keys in another case, keys with blanks
static void KeySet() {
    for (const Key& k : kKeys) {
        EngineOptions o;
        EXPECT(o.Set(k.key, 1));
    }
    for (size_t a = 0; a < kNumKeys; ++a)
        for (size_t b = a + 1; b < kNumKeys; ++b) EXPECT(0 != std::strcmp(kKeys[a].key, kKeys[b].key) && 0 != std::strcmp(kKeys[a].field, kKeys[b].field));
    std::vector<std::string> bad = {"", "nope", "fail_slicer", "plan", "plan_set", "opt_fuse_", "fuse ", " fuse", "fuse\n", "f32", "f32_split_", "max_graphs"};
    for (const Key& k : kKeys) {
        std::string up = k.key, cap = k.key;
        for (char& c : up) c = (char)std::toupper((unsigned char)c);
        for (char& c : cap)
            if (c >= 'a' && c <= 'z') { c = (char)std::toupper((unsigned char)c); break; }
        if (up != k.key) bad.push_back(up);
        if (cap != k.key) bad.push_back(cap);
    }
    for (const std::string& key : bad) {
        for (int value : {0, 1, -1, 7}) {
            EngineOptions o;
            const std::vector<int> before = Flat(o);
            if (o.Set(key, value)) std::printf("key [%s] was accepted\n", key.c_str());
            EXPECT(!o.Set(key, value));
            EXPECT(Flat(o) == before);
        }
    }
}

// 3. every key, from the defaults and from a struct with every field off its default, for every value: its own field holds what its rule says,
// a plan key also sets plan_set, and nothing else moves
static void OneFieldPerKey(const EngineOptions& start) {
    const size_t plan_set = FieldIndex("plan_set");
    for (const Key& k : kKeys) {
        const size_t own = FieldIndex(k.field);
        for (int value : {-3, -1, 0, 1, 2, 7}) {
            EngineOptions o = start;
            const std::vector<int> before = Flat(o);
            EXPECT(o.Set(k.key, value));
            const std::vector<int> after = Flat(o);
            for (size_t i = 0; i < kNumFields; ++i) {
                int want = before[i];
                if (i == own) want = Expected(k.rule, value);
                if (i == plan_set && k.rule == kPlan) want = 1;
                if (after[i] != want) std::printf("Set(%s, %d): field [%s] is %d, expected %d\n", k.key, value, kFields[i], after[i], want);
                EXPECT(after[i] == want);
            }
        }
    }
}

// a struct whose every field differs from its default, each value distinct where the type allows it
static EngineOptions AllNonDefault() {
    EngineOptions o;
    o.device = 6, o.batch = 12, o.streams = 2, o.host_slices = 4, o.pin_inputs = true, o.fail_slicer = true;
    o.fuse = false, o.fuse_upsample = false, o.fuse_stem = 0, o.fuse_pw = 2, o.fuse_layout = false, o.fuse_grid = false;
    o.alias_cat = false, o.alias_split = false, o.alias_view = false, o.f32_split = true, o.f32_split_policy = 2, o.fp16 = true;
    o.arena = false, o.graph = true, o.outputs_to_host = false, o.winograd = 0, o.detect_stream = 2, o.detect_priority = -1, o.plan_set = true;
    o.plan.f32_tile = 21, o.plan.wino23_form = 16, o.plan.wino23_ocg = 2, o.plan.f16_tile = 9, o.plan.f16_detect_tile = 0, o.plan.f16_s2c32 = 0;
    o.plan.f16_slab = 0, o.plan.f16_slab_w2 = 0, o.plan.f16_pw_patch = 0, o.plan.split3_bm = 64;
    const std::vector<int> f = Flat(o);
    for (size_t i = 0; i < kNumFields; ++i) {
        if (f[i] == kDefaults[i]) std::printf("AllNonDefault leaves [%s] at its default\n", kFields[i]);
        EXPECT(f[i] != kDefaults[i]);
    }
    return o;
}

// 4. / 5. ForChild: the parent in every field but seven
static void Child(const EngineOptions& parent) {
    const std::vector<int> before = Flat(parent);
    const EngineOptions child = parent.ForChild(3, 5);
    EXPECT(Flat(parent) == before);
    const std::vector<int> got = Flat(child);
    const struct { const char* field; int value; } over[] = {{"device", 3}, {"batch", 5}, {"streams", 1}, {"outputs_to_host", 0},
                                                             {"host_slices", 1}, {"pin_inputs", 0}, {"fail_slicer", 0}};
    std::vector<int> want = before;
    for (const auto& ov : over) want[FieldIndex(ov.field)] = ov.value;
    for (size_t i = 0; i < kNumFields; ++i) {
        if (got[i] != want[i]) std::printf("ForChild: field [%s] is %d, expected %d\n", kFields[i], got[i], want[i]);
        EXPECT(got[i] == want[i]);
    }
}

int main() {
    Defaults();
    KeySet();
    OneFieldPerKey(EngineOptions());
    const EngineOptions loaded = AllNonDefault();
    OneFieldPerKey(loaded);
    Child(loaded);
    Child(EngineOptions());
    EXPECT(!EngineOptions().ForChild(3, 5).plan_set);
    if (failures) {
        std::printf("%d failure(s)\n", failures);
        return 1;
    }
    std::printf("engine options ok\n");
    return 0;
}
