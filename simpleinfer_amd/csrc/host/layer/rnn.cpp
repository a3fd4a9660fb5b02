#include "rnn.h"

#include <cstring>

namespace SimpleInfer {

DEFINE_LAYER_REGISTRY(Rnn);

namespace {

// a rank-2 fp32 attribute of exactly rows x cols
bool ReadMatrix(const pnnx::Operator* op, const std::string& key, int rows, int cols, std::vector<float>& dst) {
    if (!CheckAttr(op, key, 1)) return false;
    const pnnx::Attribute& a = op->attrs.at(key);
    if (2 != a.shape.size() || a.shape[0] != rows || a.shape[1] != cols || a.data.size() != (size_t)rows * cols * sizeof(float)) return false;
    dst.resize((size_t)rows * cols);
    memcpy(dst.data(), a.data.data(), a.data.size());
    return true;
}

// the 1x1 convolution over `rows` pixels that is the input projection: ic -> oc
SiConv2dDesc ProjectionDesc(int rows, int ic, int in_ld, int oc, bool bias) {
    SiConv2dDesc d;
    memset(&d, 0, sizeof(d));
    d.n = rows; d.ih = d.iw = 1; d.ic = ic; d.in_ld = in_ld;
    d.oh = d.ow = 1; d.oc = oc; d.out_ld = oc;
    d.kh = d.kw = d.sh = d.sw = d.dh = d.dw = 1; d.groups = 1;
    d.has_bias = bias ? 1 : 0;
    return d;
}

}  // namespace

// pnnx: input_size, hidden_size, num_layers, bias, batch_first, bidirectional, proj_size (nn.LSTM alone), dropout (read and ignored: this is
// inference); weight_ih_l{k}, weight_hh_l{k}, bias_ih_l{k}, bias_hh_l{k} and their _reverse twins.  A missing key is kFail; what the kernel
// does not serve is refused by Validate().
Status Rnn::Init(const pnnx::Operator* op) {
    CHECK_STATUS(Layer::Init(op));
    cell_ = op->type == "nn.GRU" ? SI_RNN_GRU : SI_RNN_LSTM;
    CHECK_BOOL(Get(op, "input_size", input_size_));
    CHECK_BOOL(Get(op, "hidden_size", hidden_size_));
    CHECK_BOOL(Get(op, "num_layers", num_layers_));
    CHECK_BOOL(Get(op, "bias", use_bias_));
    CHECK_BOOL(Get(op, "batch_first", batch_first_));
    CHECK_BOOL(Get(op, "bidirectional", bidirectional_));
    proj_size_ = 0;
    Get(op, "proj_size", proj_size_);
    float dropout = 0.0f;
    GetNumber(op, "dropout", dropout);
    CHECK_BOOL(input_size_ > 0 && hidden_size_ > 0 && num_layers_ > 0);
    device_ready_ = false;
    half_refused_ = false;
    if (proj_size_ != 0) return Status::kSuccess;   // (the file then carries weight_hr_l{k} and narrower weight_hh: Validate() refuses it)
    const int rows = Gates() * hidden_size_, slots = num_layers_ * Dirs();
    weight_ih_.assign(slots, {});
    weight_hh_.assign(slots, {});
    bias_ih_.assign(slots, {});
    bias_hh_.assign(slots, {});
    for (int l = 0; l < num_layers_; ++l)
        for (int d = 0; d < Dirs(); ++d) {
            const std::string sfx = "_l" + std::to_string(l) + (d ? "_reverse" : "");
            const int s = l * Dirs() + d;
            CHECK_BOOL(ReadMatrix(op, "weight_ih" + sfx, rows, LayerInput(l), weight_ih_[s]));
            CHECK_BOOL(ReadMatrix(op, "weight_hh" + sfx, rows, hidden_size_, weight_hh_[s]));
            if (use_bias_) {
                CHECK_BOOL(ReadVec(op, ("bias_ih" + sfx).c_str(), bias_ih_[s]) && bias_ih_[s].size() == (size_t)rows);
                CHECK_BOOL(ReadVec(op, ("bias_hh" + sfx).c_str(), bias_hh_[s]) && bias_hh_[s].size() == (size_t)rows);
            }
        }
    return Status::kSuccess;
}

Status Rnn::Deinit() {
    for (LayerBuffers& b : dev_) {
        b.w_ih.Free();
        b.bias.Free();
        b.b_hn.Free();
        b.w_hh.Free();
    }
    dev_.clear();
    gates_dev_.Free();
    state_dev_.Free();
    inner_dev_[0].Free();
    inner_dev_[1].Free();
    device_ready_ = false;
    return Status::kSuccess;
}

bool Rnn::GetGeometry(const Tensor& in, const std::vector<const Tensor*>& outs, Geometry& g) const {
    const std::vector<int>& x = in.Shape();
    if (x.size() != 3 || x[2] != input_size_ || outs.empty()) return false;
    const int bi = batch_first_ ? 0 : 1, ti = batch_first_ ? 1 : 0;
    g.t = x[ti]; g.batch = x[bi];
    if (g.t <= 0 || g.batch <= 0) return false;
    std::vector<int> y = x;
    y[2] = Dirs() * hidden_size_;
    if (outs[0]->Shape() != y) return false;
    const std::vector<int> state = {num_layers_ * Dirs(), g.batch, hidden_size_};
    for (size_t i = 1; i < outs.size(); ++i)
        if (outs[i]->Shape() != state) return false;
    return true;
}

Status Rnn::Validate() {
    CHECK_STATUS(Layer::Validate());
    const char* const name = cell_ == SI_RNN_GRU ? "GRU" : "LSTM";
    CHECK_STATUS(ValidateFloatLogged(name));
    auto refuse = [&](const char* why) {
        LOG(ERROR) << name << "::Validate fail [" << why << "]";
        return Status::kUnsupport;
    };
    if (proj_size_ != 0) return refuse("proj_size != 0 is not served");
    if (input_tensor_nodes_.size() > 1) return refuse("initial states (h0 / c0) as inputs are not served: the state starts at zero");
    if (hidden_size_ > SI_RNN_MAX_HIDDEN) return refuse("hidden_size above 2048");
    const size_t n_out = output_tensor_nodes_.size();
    if (input_tensor_nodes_.size() != 1 || (n_out != 1 && n_out != 1 + StateOutputs())) {
        LOG(ERROR) << name << "::Validate fail [one input; outputs y, or y and " << StateOutputs() << " state tensor(s); got " << n_out << " outputs]";
        return Status::kErrorShape;
    }
    std::vector<const Tensor*> outs;
    for (auto* n : output_tensor_nodes_) outs.push_back(&n->tensor);
    Geometry g;
    if (!GetGeometry(input_tensor_nodes_[0]->tensor, outs, g)) {
        LOG(ERROR) << name << "::Validate fail [a rank-3 input of " << input_size_ << " features, " << (batch_first_ ? "[N, T, I]" : "[T, N, I]")
                   << ", y of " << Dirs() * hidden_size_ << " features, states [" << num_layers_ * Dirs() << ", N, " << hidden_size_ << "]; input "
                   << ShapeString(input_tensor_nodes_[0]->tensor.Shape()) << "]";
        return Status::kErrorShape;
    }
    return Status::kSuccess;
}

// time s of batch item b is row (batch_first ? b * T + s : s * N + b) of its tensor; rows are `ld` elements apart
SiRnnDesc Rnn::MakeDesc(const Geometry& g, int layer, long long in_ld, long long out_ld) const {
    SiRnnDesc d;
    memset(&d, 0, sizeof(d));
    d.cell = cell_;
    d.t = g.t; d.batch = g.batch; d.input = LayerInput(layer); d.hidden = hidden_size_; d.dirs = Dirs();
    const long long g_ld = (long long)Dirs() * Gates() * hidden_size_;
    auto strides = [&](long long ld, long long& st, long long& sb) {
        st = batch_first_ ? ld : (long long)g.batch * ld;
        sb = batch_first_ ? (long long)g.t * ld : ld;
    };
    strides(in_ld, d.x_st, d.x_sb);
    strides(g_ld, d.g_st, d.g_sb);
    strides(out_ld, d.y_st, d.y_sb);
    d.step0 = 0;
    return d;
}

// The weight images once per storage type; the workspaces whenever the shape asks for more than there is (the engine's first Forward is
// never captured, and a shape change rebuilds the plan: nothing is allocated during a graph capture).
Status Rnn::PrepareDevice(bool half, const Geometry& g) {
    const int G = Gates(), H = hidden_size_, D = Dirs();
    if (!device_ready_ || half != prepared_half_) {
        device_ready_ = false;
        CHECK_BOOL(weight_ih_.size() == (size_t)num_layers_ * D);
        dev_ = std::vector<LayerBuffers>(num_layers_);
        for (int l = 0; l < num_layers_; ++l) {
            const int I = LayerInput(l);
            // both directions' W_ih as ONE [D G H, I] matrix, both W_hh as [D][G H][H]
            std::vector<float> w_ih, w_hh, bias((size_t)D * G * H, 0.0f), b_hn((size_t)D * H, 0.0f);
            for (int d = 0; d < D; ++d) {
                const int s = l * D + d;
                w_ih.insert(w_ih.end(), weight_ih_[s].begin(), weight_ih_[s].end());
                w_hh.insert(w_hh.end(), weight_hh_[s].begin(), weight_hh_[s].end());
                if (!use_bias_) continue;
                // summed once, in fp32: LSTM b_ih + b_hh; GRU b_ih + b_hh for r and z, b_ih alone for n (b_hn goes to the step kernel)
                for (int j = 0; j < G * H; ++j) {
                    const bool gru_n = cell_ == SI_RNN_GRU && j >= 2 * H;
                    bias[(size_t)d * G * H + j] = gru_n ? bias_ih_[s][j] : bias_ih_[s][j] + bias_hh_[s][j];
                    if (gru_n) b_hn[(size_t)d * H + (j - 2 * H)] = bias_hh_[s][j];
                }
            }
            Geometry one;
            one.t = one.batch = 1;
            const SiRnnDesc rd = MakeDesc(one, l, I, (long long)D * H);
            const SiConv2dDesc cd = ProjectionDesc(1, I, I, D * G * H, false);
            LayerBuffers& b = dev_[l];
            const size_t img_bytes = si_hip_rnn_workspace_bytes(&rd, SI_RNN_WS_WHH, half ? 1 : 0);
            if (img_bytes == 0) {
                LOG(ERROR) << "Rnn: no " << (half ? "fp16" : "fp32") << " step kernel for hidden_size " << H << ", input " << I;
                return Status::kUnsupport;
            }
            std::vector<char> img(img_bytes);
            if (half) {
                if (si_hip_conv2d_f16_supported(&cd) != 1) {
                    LOG(ERROR) << "Rnn: no fp16 projection kernel for input " << I;
                    return Status::kUnsupport;
                }
                std::vector<uint16_t> packed(si_hip_conv2d_f16_weight_elems(&cd));
                CHECK_STATUS(CheckHip(si_hip_conv2d_f16_pack_weight_host(&cd, w_ih.data(), packed.data()), "pack fp16 weight"));
                CHECK_STATUS(CheckHip(b.w_ih.Upload(packed.data(), packed.size() * sizeof(uint16_t)), "upload weight"));
                CHECK_STATUS(CheckHip(si_hip_rnn_pack_whh_f16(&rd, w_hh.data(), img.data()), "pack fp16 W_hh"));
            } else {
                std::vector<float> packed(si_hip_conv2d_weight_elems(&cd));
                CHECK_STATUS(CheckHip(si_hip_conv2d_pack_weight_host(&cd, w_ih.data(), packed.data()), "pack weight"));
                CHECK_STATUS(CheckHip(b.w_ih.Upload(packed.data(), packed.size() * sizeof(float)), "upload weight"));
                CHECK_STATUS(CheckHip(si_hip_rnn_pack_whh_f32(&rd, w_hh.data(), reinterpret_cast<float*>(img.data())), "pack W_hh"));
            }
            CHECK_STATUS(CheckHip(b.w_hh.Upload(img.data(), img.size()), "upload W_hh"));
            if (use_bias_) {
                CHECK_STATUS(CheckHip(b.bias.Upload(bias.data(), bias.size() * sizeof(float)), "upload bias"));
                if (cell_ == SI_RNN_GRU) CHECK_STATUS(CheckHip(b.b_hn.Upload(b_hn.data(), b_hn.size() * sizeof(float)), "upload b_hn"));
            }
        }
        prepared_half_ = half;
        device_ready_ = true;
    }
    const size_t es = half ? 2 : 4, rows = (size_t)g.t * g.batch;
    const size_t need_gates = rows * D * G * H * es, need_state = cell_ == SI_RNN_LSTM ? (size_t)D * g.batch * H * 4 : 0, need_inner = rows * D * H * es;
    if (need_gates > gates_dev_.bytes()) CHECK_STATUS(CheckHip(gates_dev_.Alloc(need_gates), "rnn gate workspace"));
    if (need_state > state_dev_.bytes()) CHECK_STATUS(CheckHip(state_dev_.Alloc(need_state), "rnn state"));
    for (int i = 0; i < 2 && i < num_layers_ - 1; ++i)
        if (need_inner > inner_dev_[i].bytes()) CHECK_STATUS(CheckHip(inner_dev_[i].Alloc(need_inner), "rnn inner output"));
    return Status::kSuccess;
}

Status Rnn::Run(const Tensor& in, std::vector<Tensor>& outs) {
    const bool half = IsHalf(in);
    std::vector<const Tensor*> optrs;
    for (const Tensor& t : outs) {
        if (IsHalf(t) != half) return Status::kUnsupport;
        optrs.push_back(&t);
    }
    Geometry g;
    if ((outs.size() != 1 && outs.size() != 1 + StateOutputs()) || !GetGeometry(in, optrs, g)) return Status::kErrorShape;
    for (size_t i = 1; i < outs.size(); ++i)
        if (outs[i].PixelStride() != hidden_size_) return Status::kUnsupport;   // the state outputs are dense
    CHECK_STATUS(PrepareDevice(half, g));

    const int G = Gates(), H = hidden_size_, D = Dirs();
    const size_t es = half ? 2 : 4, state_bytes = (size_t)D * g.batch * H * es;
    const int rows = g.t * g.batch;
    for (int l = 0; l < num_layers_; ++l) {
        const bool last = l == num_layers_ - 1;
        const void* const src = l == 0 ? in.RawData() : inner_dev_[(l - 1) % 2].As<void>();
        const int src_ld = l == 0 ? in.PixelStride() : D * H;
        void* const dst = last ? outs[0].RawData() : inner_dev_[l % 2].As<void>();
        const int dst_ld = last ? outs[0].PixelStride() : D * H;
        const LayerBuffers& b = dev_[l];
        const float* const bias = use_bias_ ? b.bias.As<float>() : nullptr;
        const float* const b_hn = (use_bias_ && cell_ == SI_RNN_GRU) ? b.b_hn.As<float>() : nullptr;
        // 1. the input projection of every row and both directions into the gate workspace
        const SiConv2dDesc cd = ProjectionDesc(rows, LayerInput(l), src_ld, D * G * H, bias != nullptr);
        const int prc = half ? si_hip_conv2d_f16(&cd, src, b.w_ih.As<void>(), bias, nullptr, gates_dev_.As<void>(), 0, Stream())
                             : si_hip_conv2d_f32(&cd, static_cast<const float*>(src), b.w_ih.As<float>(), bias, nullptr, gates_dev_.As<float>(), Stream());
        CHECK_STATUS(CheckHip(prc, "Rnn input projection"));
        // 2. + 3. the steps, and this layer's slots of the state outputs
        const SiRnnDesc rd = MakeDesc(g, l, src_ld, dst_ld);
        char* const hn = outs.size() > 1 ? static_cast<char*>(outs[1].RawData()) + (size_t)l * state_bytes : nullptr;
        char* const cn = outs.size() > 2 ? static_cast<char*>(outs[2].RawData()) + (size_t)l * state_bytes : nullptr;
        const int rc = half ? si_hip_rnn_layer_f16(&rd, gates_dev_.As<void>(), b.w_hh.As<void>(), b_hn, dst, state_dev_.As<float>(), hn, cn, Stream())
                            : si_hip_rnn_layer_f32(&rd, gates_dev_.As<float>(), b.w_hh.As<float>(), b_hn, static_cast<float*>(dst), state_dev_.As<float>(),
                                                   reinterpret_cast<float*>(hn), reinterpret_cast<float*>(cn), Stream());
        CHECK_STATUS(CheckHip(rc, "Rnn steps"));
    }
    return Status::kSuccess;
}

Status Rnn::Forward(const Tensor& input, Tensor& output) {
    return RunOnDevice({&input}, {&output}, [this](const std::vector<Tensor>& in, std::vector<Tensor>& out) { return Run(in[0], out); });
}

Status Rnn::Forward(const Tensor& input, std::vector<Tensor>& outputs) {
    std::vector<Tensor*> outs;
    for (Tensor& t : outputs) outs.push_back(&t);
    return RunOnDevice({&input}, outs, [this](const std::vector<Tensor>& in, std::vector<Tensor>& out) { return Run(in[0], out); });
}

const char* Rnn::KernelName() const {
    if (input_tensor_nodes_.empty() || output_tensor_nodes_.empty()) return "rnn_step";
    const Tensor& in = input_tensor_nodes_[0]->tensor;
    std::vector<const Tensor*> outs;
    for (auto* n : output_tensor_nodes_) outs.push_back(&n->tensor);
    Geometry g;
    if (!GetGeometry(in, outs, g)) return "rnn_step";
    const SiRnnDesc d = MakeDesc(g, num_layers_ - 1, LayerInput(num_layers_ - 1), (long long)Dirs() * hidden_size_);
    // (gates and y are buffers of the layer or the engine, 256-byte aligned: the name is asked for such addresses)
    const uintptr_t base = (uintptr_t)1 << 40;
    return si_hip_rnn_kernel_name(&d, (const void*)base, (const void*)(base << 1), IsHalf(in) ? 1 : 0);
}

// per layer and row: the projection I_l -> D G H and, per direction, the recurrent product H -> G H
double Rnn::Flops() const {
    if (input_tensor_nodes_.empty() || output_tensor_nodes_.empty()) return 0.0;
    const std::vector<int>& x = input_tensor_nodes_[0]->tensor.Shape();
    if (x.size() != 3) return 0.0;
    const double rows = (double)x[0] * x[1], gh = (double)Dirs() * Gates() * hidden_size_;
    double f = 0.0;
    for (int l = 0; l < num_layers_; ++l) f += 2.0 * rows * gh * ((double)LayerInput(l) + hidden_size_);
    return f;
}

// the operands, W_ih once per layer and W_hh once per step: what a step reads from L2 is the whole recurrent matrix
double Rnn::Bytes() const {
    double b = Layer::Bytes();
    if (input_tensor_nodes_.empty()) return b;
    const Tensor& in = input_tensor_nodes_[0]->tensor;
    if (in.Shape().size() != 3) return b;
    const double es = IsHalf(in) ? 2.0 : 4.0, t = in.Shape()[batch_first_ ? 1 : 0], gh = (double)Dirs() * Gates() * hidden_size_;
    for (int l = 0; l < num_layers_; ++l) b += es * gh * ((double)LayerInput(l) + t * hidden_size_);
    return b;
}

// The recurrence is not offered in fp32 between casts: a refusal is final for this layer object, so the engine's retry with fp32 shadow
// operands ends in kUnsupport with the reason below instead of a model whose precision depends on its shape.
bool Rnn::HalfStorageOk(std::string& why) const {
    const char* const rule = "the fp16 step kernel of nn.LSTM / nn.GRU needs hidden_size % 8 == 0 and input_size % 8 == 0";
    if (half_refused_) { why = rule; return false; }
    if (!Layer::HalfStorageOk(why)) return false;
    bool half = false;
    for (auto* n : input_tensor_nodes_) half = half || IsHalf(n->tensor);
    if (!half) return true;
    if (hidden_size_ % 8 != 0 || input_size_ % 8 != 0) {
        half_refused_ = true;
        why = rule;
        return false;
    }
    return true;
}

}  // namespace SimpleInfer
