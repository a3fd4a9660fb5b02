// engine_options.h -- every engine option (Engine::SetOption, include/engine.h) as one value type: the field with its default, ONE table row that
// gives the key's text and rule, and ForChild, the one place that says what a half-batch lane or the sliced pipeline's engine inherits.
// Pure: si_hip.h for SiConvPlan and standard headers only, so it is tested without a device (tests/cpp/test_engine_options.cpp).
#ifndef SIMPLE_INFER_SRC_ENGINE_OPTIONS_H_
#define SIMPLE_INFER_SRC_ENGINE_OPTIONS_H_

#include <string>

#include "si_hip.h"

namespace SimpleInfer {

struct EngineOptions {
    int device = -1;
    bool fuse = true;
    bool alias_cat = true;
    bool alias_split = true;   // torch.chunk / torch.split / Tensor.slice outputs that are channel ranges become views of the input (0: always copied)
    bool fuse_grid = true;     // F.grid_sample reads a permuted grid in place and an affine grid from theta (0: the grid is written first; A/B runs)
    bool fuse_layout = true;   // a run of permute / reshape / view / transpose / squeeze / unsqueeze operators is planned as ONE layout step (0: one step each)
    bool alias_view = true;    // a layout step that moves no byte makes its output a view of its input's buffer (0: one permute_rows copy)
    bool fuse_const = true;    // BinaryOp(x, c0) whose only reader is BinaryOp(., c1), c0 / c1 graph constants, is ONE two-stage launch (0: two launches, the same bits)
    bool fuse_xcorr = true;    // view -> view -> F.conv2d(groups = N C) -> view is ONE launch of the depthwise kernel in its per-sample addressing (0: the four steps, the same bits)
    bool fuse_norm = true;     // torch.norm(x, p, dim = d) -> [torch.unsqueeze(d)] -> BinaryOp div(x, .) is ONE lpnorm launch with normalize = 1, eps = 0 (0: the steps as they are; fp32: the same bits)
    bool fuse_upsample = true; // upsample -> cat -> 1x1 conv read at the source
    int fuse_stem = 2;         // fp16: 1 RGB stem conv + the 3x3 s2 conv behind it in one launch; 2 ... and the 1x1 conv(s) reading that; 0 off
    int fuse_pw = 1;   // fp16: 1 a C3 bottleneck's 1x1 conv computed inside the kernel of its 3x3 conv; 0 off
                       // (2: ... and the C3's closing conv behind its last 64-channel pair -- built in round 6, bit-identical, 0.74-0.84x of the launches
                       // it replaces: the fused workgroup is bound by its three SiLU epilogues on two waves per SIMD; opt-in, LAB_NOTEBOOK R6.4)
    bool f32_split = false;    // fp32 tensors, conv contraction from three fp16 MFMA products (0: true fp32)
    int f32_split_policy = 4;  // which layers f32_split takes: 1 round 5's, 2 + sibling-fused / wide 1x1 from K = 256, 3 + dual-source (upsampled) layers, 4 + the RGB stem
    // kernel-form choices handed to every conv launch (SiConvPlan, include/si_hip.h; every form of a family produces the same bits; all default: the
    // policy): A/B runs and tests.  Until round 6 these were process-global setters / environment switches of the kernel library.
    SiConvPlan plan = SI_CONV_PLAN_DEFAULT;
    bool plan_set = false;
    bool arena = true;         // intermediate operands share one HBM arena by lifetime (0: one allocation per operand, as the reference)
    bool graph = false;
    bool outputs_to_host = true;
    int winograd = 1;          // 0 off, 1 F(2,3) where faster, 2 F(4,3) on those layers
    int batch = 0;             // > 0: serve this batch whatever batch the file was traced with (the file bakes its batch into every shape)
    int detect_stream = 1;     // Detect's early levels on a second stream beside the layers that follow their inputs: 0 never, 1 for levels with enough work, 2 always
    int detect_priority = 0;   // si_hip_stream_create_priority level of that stream: -1 low, 0 the device default, +1 high.  -1 (lowest: the
                               // neck on the main stream is the critical path, Detect fills what it leaves) measured +0.7 % fp16 / flat fp32 on ONE engine
                               // (r05_ab_detect_priority.txt) -- inside the box-to-box spread, and with several engines on a device a lowest-priority
                               // stream can be starved by the others' default-priority work: opt-in since round 6
    bool fp16 = false;         // fp16 storage for internal activations and weights (BASELINE.json configs[3])
    int streams = 1;           // 2: two half-batch lanes on two streams; 1: one stream
    int host_slices = 0;       // host inputs + host outputs: G batch slices pipelined over PCIe inside one Forward(); 1: off; 0: auto
    bool pin_inputs = false;   // the sliced pipeline may hipHostRegister a borrowed input buffer in place (opt-in: the caller keeps it mapped until the next Input() / Release)
    bool fail_slicer = false;  // key "_fail_slicer" (tests): the sliced pipeline's setup fails half way

    // Sets the field of `key` by the key's rule; an unknown key changes nothing and returns false.
    bool Set(const std::string& key, int value) {
        typedef EngineOptions O;
        struct Row {
            const char* key;
            bool O::*flag = nullptr;           // stores value != 0
            int O::*number = nullptr; bool sign = false;   // stores the value as given -- or its sign (-1, 0, 1), when `sign` is set
            int SiConvPlan::*form = nullptr;   // stores into `plan` and sets `plan_set`
            Row(const char* k, bool O::*f) : key(k), flag(f) {}
            Row(const char* k, int O::*n, bool s = false) : key(k), number(n), sign(s) {}
            Row(const char* k, int SiConvPlan::*f) : key(k), form(f) {}
        };
        static const Row kRows[] = {
            // value != 0
            {"fuse", &O::fuse}, {"fuse_upsample", &O::fuse_upsample}, {"fuse_layout", &O::fuse_layout}, {"fuse_grid", &O::fuse_grid}, {"fuse_const", &O::fuse_const}, {"fuse_xcorr", &O::fuse_xcorr}, {"fuse_norm", &O::fuse_norm},
            {"alias_cat", &O::alias_cat}, {"alias_split", &O::alias_split}, {"alias_view", &O::alias_view}, {"arena", &O::arena},
            {"fp16", &O::fp16}, {"f32_split", &O::f32_split}, {"graph", &O::graph}, {"outputs_to_host", &O::outputs_to_host},
            {"pin_inputs", &O::pin_inputs}, {"_fail_slicer", &O::fail_slicer},
            // the value as given; detect_priority: its sign
            {"device", &O::device}, {"batch", &O::batch}, {"streams", &O::streams}, {"host_slices", &O::host_slices}, {"winograd", &O::winograd},
            {"fuse_stem", &O::fuse_stem}, {"fuse_pw", &O::fuse_pw}, {"f32_split_policy", &O::f32_split_policy},
            {"detect_stream", &O::detect_stream}, {"detect_priority", &O::detect_priority, true},
            // the SiConvPlan member of the same name
            {"f32_tile", &SiConvPlan::f32_tile}, {"wino23_form", &SiConvPlan::wino23_form}, {"wino23_ocg", &SiConvPlan::wino23_ocg},
            {"f16_tile", &SiConvPlan::f16_tile}, {"f16_detect_tile", &SiConvPlan::f16_detect_tile}, {"f16_s2c32", &SiConvPlan::f16_s2c32},
            {"f16_slab", &SiConvPlan::f16_slab}, {"f16_slab_w2", &SiConvPlan::f16_slab_w2}, {"f16_pw_patch", &SiConvPlan::f16_pw_patch},
            {"split3_bm", &SiConvPlan::split3_bm},
        };
        for (const Row& r : kRows) {
            if (key != r.key) continue;
            if (r.flag) this->*r.flag = value != 0;
            else if (r.number) this->*r.number = r.sign ? (value < 0 ? -1 : (value > 0 ? 1 : 0)) : value;
            else { plan.*r.form = value; plan_set = true; }
            return true;
        }
        return false;
    }

    // The options of a child engine -- a half-batch lane ("streams") or the sliced pipeline's engine ("host_slices"): all of the parent's, on the parent's
    // device at its own batch, one stream, outputs left on the device (the parent owns the host mirrors).  (graph is inherited: a lane replays its OWN
    // captured graph -- one graph holding both branches measured 10 % SLOWER than one stream, profiles/r03_ab_streams.txt -- the slicer's one per slice.)
    EngineOptions ForChild(int child_device, int child_batch) const {
        EngineOptions c = *this;
        c.device = child_device, c.batch = child_batch;
        c.streams = 1, c.outputs_to_host = false;
        c.host_slices = 1, c.pin_inputs = false, c.fail_slicer = false;   // (is_lane_ makes a child ignore these three: reset all the same)
        return c;
    }
};

}  // namespace SimpleInfer

#endif
