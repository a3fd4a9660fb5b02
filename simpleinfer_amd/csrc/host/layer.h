// layer.h -- the operator plugin base class.  Virtual surface and call order are the reference's
// (src/layer.h:15-89; engine call order creator -> Init(op) -> SetContext -> SetInputNodes ->
// SetOutputNodes -> Validate, src/engine_impl.cpp:252-306): a layer written against SimpleInfer's
// Layer compiles against this one, minus GetEigenThreadPoolDevice (there is no CPU device here).
//
// What is new: tensors handed to Forward() normally live in HBM and the layer enqueues HIP kernels
// on context_->stream().  When a caller passes HOST tensors (the reference's layer tests do:
// test/test_layer/*.cpp construct a layer, poke its public fields and call Forward(in, out)),
// RunOnDevice() stages them through temporary device buffers and synchronises, so the same test
// code still exercises the HIP kernels -- there is no CPU compute path.
#ifndef SIMPLE_INFER_SRC_LAYER_H_
#define SIMPLE_INFER_SRC_LAYER_H_

#include <functional>
#include <map>
#include <string>
#include <vector>

#include "context.h"
#include "layer_registry.h"
#include "logger.h"
#include "pnnx/ir.h"
#include "pnnx/param_read.h"
#include "pnnx/pnnx_helper.h"
#include "tensor.h"
#include "tensor_node.h"
#include "types.h"

namespace SimpleInfer {

class Layer {
public:
    Layer();
    virtual ~Layer();

    // ---- the reference's virtual surface (src/layer.h:15-89), in the order the engine calls it --------------------
    virtual Status Init(const pnnx::Operator* op);                                   // 1. parse params / attrs of one operator
    virtual Status Init(const std::map<std::string, pnnx::Parameter>& params,       //    (the form layers usually override)
                        const std::map<std::string, pnnx::Attribute>& attrs);
    virtual void SetContext(Context* context);                                       // 2. device + stream
    virtual void SetInputNodes(const std::vector<TensorNode*>& input_tensor_nodes);  // 3.
    virtual void SetOutputNodes(const std::vector<TensorNode*>& output_tensor_nodes);  // 4.
    virtual Status Validate();                                                       // 5. arity / dtype / shape checks
    virtual Status Deinit();                                                         // before the registry destroyer

    virtual Status Forward();  // arity dispatch on the bound nodes (src/layer.cpp:45-79) into one of:
    virtual Status Forward(const Tensor& input, Tensor& output);
    virtual Status Forward(const std::vector<Tensor>& inputs, Tensor& output);
    virtual Status Forward(const Tensor& input, std::vector<Tensor>& outputs);
    virtual Status Forward(const std::vector<Tensor>& inputs, std::vector<Tensor>& outputs);

    const pnnx::Operator* GetOp();

public:
    // ---- extensions used by the engine ---------------------------------------------------
    // kernel family name for profiles ("conv_igemm", "maxpool", ...)
    virtual const char* KernelName() const { return "none"; }
    // algorithmic cost of one Forward with the currently bound nodes
    virtual double Flops() const { return 0.0; }
    // tensors a layer reads besides its bound input nodes (fusion hooks: a conv's residual, its upsampled source); the engine's
    // memory planner needs every reader of a buffer
    virtual void ExtraReads(std::vector<TensorNode*>& nodes) const { (void)nodes; }
    // rebind one of the ExtraReads nodes (the engine's fp32 fallback hands a layer fp32 shadows of its half operands); false: cannot
    virtual bool ReplaceExtraRead(TensorNode* from, TensorNode* to) { (void)from; (void)to; return false; }
    // the stream this layer's launches go to (its context's)
    si_stream_t LaunchStream() const { return Stream(); }
    // fp16 storage (Engine option "fp16"): can this layer run with the storage types its bound nodes now have?  Asked once, at
    // LoadModel, so that an unsupported combination is a load-time Status with a reason instead of a failing first Forward().
    // Default: fine when no bound tensor is fp16, or when inputs and outputs are all fp16.
    virtual bool HalfStorageOk(std::string& why) const;
    // Asked by the planner BEFORE it makes `node` (one of this layer's bound or extra operands) a channel slice of a wider buffer: does the
    // launch this layer will make take the operand at pixel stride `ld` elements, `off` channels into the row, in the storage type the node
    // has -- itself or through a second launch of its own?  Fusions and HalfStorageOk were decided on dense strides; this is where they meet
    // the real view, and a "no" leaves the operand its own buffer (view_rule.h).  Default: yes (kernels that step by ld with scalar accesses).
    virtual bool TakesView(const TensorNode* node, int ld, int off) const { (void)node; (void)ld; (void)off; return true; }
    virtual double Bytes() const;

    const std::vector<TensorNode*>& InputNodes() const { return input_tensor_nodes_; }
    const std::vector<TensorNode*>& OutputNodes() const { return output_tensor_nodes_; }

protected:
    virtual Status ValidateShape(const int input_size, const int output_size);

    // all-float check shared by the concrete Validate()s (reference e.g. src/layer/conv_2d.cpp:94-101)
    Status ValidateFloat32();
    // fp32 or fp16 storage (the fp16 engine path, SetOption("fp16", 1)); inputs / outputs may differ at the graph boundary
    Status ValidateFloat();
    // the same, logging "<layer>::Validate fail [unsupport input/output data type]" on refusal
    Status ValidateFloatLogged(const char* layer);
    static bool IsHalf(const Tensor& t) { return t.GetDataType() == DataType::kFloat16; }

    si_stream_t Stream() const;

    using DeviceFn = std::function<Status(const std::vector<Tensor>&, std::vector<Tensor>&)>;
    // Calls fn with device-resident views of inputs/outputs; host tensors are staged (H2D, run,
    // D2H, sync).  Device tensors pass straight through with no copy and no sync.
    Status RunOnDevice(const std::vector<const Tensor*>& inputs, const std::vector<Tensor*>& outputs,
                       const DeviceFn& fn);

    // maps a C-ABI return code to Status, logging the HIP error string
    Status CheckHip(int rc, const char* what) const;

    // ---- descriptor operators: entries si_hip_X_f32 / si_hip_X_f16 / si_hip_X_kernel_name(&desc, in, out, ..), include/si_*.h ----
    // `make(in, out, desc)` fills the descriptor for a pair of tensors and says whether it could.
    //
    // The launch on device tensors: inputs and outputs of one storage type or kUnsupport, the descriptor or `bad_desc`, then the entry of
    // the type.  (The f32 entries take float pointers, the f16 ones void pointers, slice / permute void pointers for both.)
    template <typename Desc, typename I32, typename O32, typename I16, typename O16, typename Make>
    Status LaunchDesc(int (*f32)(const Desc*, I32*, O32*, si_stream_t), int (*f16)(const Desc*, I16*, O16*, si_stream_t), const char* label,
                      const Tensor& in, const Tensor& out, const Make& make, Status bad_desc = Status::kErrorShape) const {
        if (IsHalf(in) != IsHalf(out)) return Status::kUnsupport;
        Desc d;
        if (!make(in, out, d)) return bad_desc;
        const int rc = IsHalf(in) ? f16(&d, static_cast<I16*>(in.RawData()), static_cast<O16*>(out.RawData()), Stream())
                                  : f32(&d, static_cast<I32*>(in.RawData()), static_cast<O32*>(out.RawData()), Stream());
        return CheckHip(rc, label);
    }
    // Forward(input, output) of a layer that is nothing but that launch
    template <typename F32, typename F16, typename Make>
    Status ForwardDesc(F32 f32, F16 f16, const char* label, const Tensor& input, Tensor& output, const Make& make) {
        const auto launch = [&](const Tensor& in, const Tensor& out) { return LaunchDesc(f32, f16, label, in, out, make); };
        // (one captured reference: the std::function holds it in place, no allocation)
        return RunOnDevice({&input}, {&output}, [&launch](const std::vector<Tensor>& in, std::vector<Tensor>& out) { return launch(in[0], out[0]); });
    }
    // KernelName(): the entry's answer for the bound nodes; `fallback` while nothing is bound or the descriptor cannot be made.
    // `half_of_output`: the storage type asked about is the output's (the pools), not the input's.
    template <typename Desc, typename Make>
    const char* DescKernelName(const char* (*name)(const Desc*, const void*, const void*, int), const char* fallback, const Make& make,
                               bool half_of_output = false) const {
        if (input_tensor_nodes_.empty() || output_tensor_nodes_.empty()) return fallback;
        const Tensor& in = input_tensor_nodes_[0]->tensor;
        const Tensor& out = output_tensor_nodes_[0]->tensor;
        Desc d;
        if (!make(in, out, d)) return fallback;
        return name(&d, in.RawData(), out.RawData(), IsHalf(half_of_output ? out : in) ? 1 : 0);
    }

protected:
    Context* context_ = nullptr;

    const pnnx::Operator* op_ = nullptr;

    std::vector<TensorNode*> input_tensor_nodes_;
    std::vector<TensorNode*> output_tensor_nodes_;
};

// default layer registry entry (same macro names as reference src/layer.h:74-87)
#define DEFINE_LAYER_CREATOR(type) \
    Layer* type##_LayerCreator() { return (new type); }

#define DEFINE_LAYER_DESTROYER(type)           \
    void type##_LayerDestroyer(Layer* layer) { \
        if (nullptr != layer) { delete layer; } \
    }

#define DEFINE_LAYER_REGISTRY(type) \
    DEFINE_LAYER_CREATOR(type)      \
    DEFINE_LAYER_DESTROYER(type)

}  // namespace SimpleInfer

#endif  // SIMPLE_INFER_SRC_LAYER_H_
