#include "multihead_attention.h"

#include <cmath>
#include <cstring>

namespace SimpleInfer {

DEFINE_LAYER_REGISTRY(MultiheadAttention);

namespace {

// a rank-2 fp32 attribute of exactly rows x cols
bool ReadMatrix(const pnnx::Operator* op, const char* key, int rows, int cols, std::vector<float>& dst) {
    if (!CheckAttr(op, key, 1)) return false;
    const pnnx::Attribute& a = op->attrs.at(key);
    if (2 != a.shape.size() || a.shape[0] != rows || a.shape[1] != cols || a.data.size() != (size_t)rows * cols * sizeof(float)) return false;
    dst.resize((size_t)rows * cols);
    memcpy(dst.data(), a.data.data(), a.data.size());
    return true;
}

// the 1x1 convolution over `rows` pixels that is a Linear: ic -> oc
SiConv2dDesc LinearDesc(int rows, int ic, int in_ld, int oc, int out_ld, bool bias) {
    SiConv2dDesc d;
    memset(&d, 0, sizeof(d));
    d.n = rows; d.ih = d.iw = 1; d.ic = ic; d.in_ld = in_ld;
    d.oh = d.ow = 1; d.oc = oc; d.out_ld = out_ld;
    d.kh = d.kw = d.sh = d.sw = d.dh = d.dw = 1; d.groups = 1;
    d.has_bias = bias ? 1 : 0;
    return d;
}

size_t Align256(size_t bytes) { return (bytes + 255) / 256 * 256; }

}  // namespace

// pnnx: embed_dim, num_heads, bias, batch_first, add_bias_kv, add_zero_attn, kdim, vdim; in_proj_weight (3E, E), in_proj_bias (3E),
// out_proj.weight (E, E), out_proj.bias (E).  A missing key is kFail; what the kernel does not serve is refused by Validate().
Status MultiheadAttention::Init(const pnnx::Operator* op) {
    CHECK_STATUS(Layer::Init(op));
    CHECK_BOOL(Get(op, "embed_dim", embed_dim_));
    CHECK_BOOL(Get(op, "num_heads", num_heads_));
    CHECK_BOOL(Get(op, "bias", use_bias_));
    CHECK_BOOL(Get(op, "batch_first", batch_first_));
    CHECK_BOOL(Get(op, "add_bias_kv", add_bias_kv_));
    CHECK_BOOL(Get(op, "add_zero_attn", add_zero_attn_));
    CHECK_BOOL(Get(op, "kdim", kdim_));
    CHECK_BOOL(Get(op, "vdim", vdim_));
    CHECK_BOOL(embed_dim_ > 0 && num_heads_ > 0);
    device_ready_ = false;
    // (with kdim / vdim of their own the file carries q_proj_weight / k_proj_weight / v_proj_weight instead: Validate() refuses those)
    if (kdim_ != embed_dim_ || vdim_ != embed_dim_) return Status::kSuccess;
    CHECK_BOOL(ReadMatrix(op, "in_proj_weight", 3 * embed_dim_, embed_dim_, in_proj_weight_));
    CHECK_BOOL(ReadMatrix(op, "out_proj.weight", embed_dim_, embed_dim_, out_proj_weight_));
    if (use_bias_) {
        CHECK_BOOL(ReadVec(op, "in_proj_bias", in_proj_bias_) && in_proj_bias_.size() == (size_t)3 * embed_dim_);
        CHECK_BOOL(ReadVec(op, "out_proj.bias", out_proj_bias_) && out_proj_bias_.size() == (size_t)embed_dim_);
    }
    return Status::kSuccess;
}

Status MultiheadAttention::Deinit() {
    for (DeviceBuffer& w : weight_dev_) w.Free();
    bias_dev_.Free();
    workspace_dev_.Free();
    device_ready_ = false;
    return Status::kSuccess;
}

bool MultiheadAttention::GetGeometry(const std::vector<const Tensor*>& in, const Tensor& out, Geometry& g) const {
    if (in.empty() || in.size() > 3) return false;
    for (const Tensor* t : in)
        if (t->Shape().size() != 3 || t->Shape()[2] != embed_dim_) return false;
    const std::vector<int>& q = in[0]->Shape();
    const std::vector<int>& k = in[in.size() > 1 ? 1 : 0]->Shape();
    const std::vector<int>& v = in[in.size() > 2 ? 2 : (in.size() > 1 ? 1 : 0)]->Shape();
    if (k != v || out.Shape() != q) return false;
    const int bi = batch_first_ ? 0 : 1, li = batch_first_ ? 1 : 0;
    if (q[bi] != k[bi]) return false;
    g.batch = q[bi]; g.lq = q[li]; g.lk = k[li];
    return g.batch > 0 && g.lq > 0 && g.lk > 0;
}

Status MultiheadAttention::Validate() {
    CHECK_STATUS(Layer::Validate());
    CHECK_STATUS(ValidateFloatLogged("MultiheadAttention"));
    auto refuse = [](const char* why) {
        LOG(ERROR) << "MultiheadAttention::Validate fail [" << why << "]";
        return Status::kUnsupport;
    };
    if (add_bias_kv_) return refuse("add_bias_kv=True is not served");
    if (add_zero_attn_) return refuse("add_zero_attn=True is not served");
    if (kdim_ != embed_dim_) return refuse("kdim differs from embed_dim");
    if (vdim_ != embed_dim_) return refuse("vdim differs from embed_dim");
    if (output_tensor_nodes_.size() > 1) return refuse("a second output operand (the attention weights) is not served");
    if (input_tensor_nodes_.size() > 3) return refuse("a fourth input (an attention mask) is not served");
    if (embed_dim_ % num_heads_ != 0) return refuse("embed_dim is no multiple of num_heads");
    if (embed_dim_ / num_heads_ > SI_ATTENTION_MAX_D) return refuse("head dim above 128");
    if (input_tensor_nodes_.empty() || output_tensor_nodes_.size() != 1) {
        LOG(ERROR) << "MultiheadAttention::Validate fail [1 to 3 inputs and one output]";
        return Status::kErrorShape;
    }
    std::vector<const Tensor*> in;
    for (auto* n : input_tensor_nodes_) in.push_back(&n->tensor);
    Geometry g;
    if (!GetGeometry(in, output_tensor_nodes_[0]->tensor, g)) {
        LOG(ERROR) << "MultiheadAttention::Validate fail [rank-3 operands of " << embed_dim_ << " features, " << (batch_first_ ? "[N, L, E]" : "[L, N, E]")
                   << ", key and value of one shape, output of the query's; query " << ShapeString(in[0]->Shape()) << "]";
        return Status::kErrorShape;
    }
    return Status::kSuccess;
}

// token s of batch item b is row (batch_first ? b * L + s : s * N + b) of its tensor; rows are `ld` elements apart
static void RowStrides(bool batch_first, int batch, int len, long long ld, long long& sb, long long& ss) {
    sb = batch_first ? (long long)len * ld : ld;
    ss = batch_first ? ld : (long long)batch * ld;
}

bool MultiheadAttention::MakeDesc(const Geometry& g, SiAttentionDesc& d) const {
    if (num_heads_ <= 0 || embed_dim_ % num_heads_ != 0) return false;
    memset(&d, 0, sizeof(d));
    d.batch = g.batch; d.heads = num_heads_; d.lq = g.lq; d.lk = g.lk; d.d = embed_dim_ / num_heads_;
    const long long ld = 3LL * embed_dim_;
    RowStrides(batch_first_, g.batch, g.lq, ld, d.q_sb, d.q_ss);
    RowStrides(batch_first_, g.batch, g.lk, ld, d.k_sb, d.k_ss);
    d.v_sb = d.k_sb; d.v_ss = d.k_ss;
    RowStrides(batch_first_, g.batch, g.lq, embed_dim_, d.o_sb, d.o_ss);
    d.scale = 1.0f / sqrtf((float)d.d);
    return true;
}

// The weight images once per (storage type, input count); the workspace whenever the shape asks for more than there is (the engine's first
// Forward is never captured, and a shape change rebuilds the plan: nothing is allocated during a graph capture).
Status MultiheadAttention::PrepareDevice(bool half, int n_in, const Geometry& g) {
    const int E = embed_dim_;
    if (!device_ready_ || half != prepared_half_ || n_in != prepared_inputs_) {
        device_ready_ = false;
        CHECK_BOOL(in_proj_weight_.size() == (size_t)3 * E * E && out_proj_weight_.size() == (size_t)E * E);
        // the row blocks of in_proj_weight that input i feeds: 1 input 3E rows; 2 inputs E and 2E; 3 inputs E each
        const int start[3] = {0, E, 2 * E};
        const int count[3] = {n_in == 1 ? 3 * E : E, n_in == 2 ? 2 * E : E, E};
        for (int i = 0; i < 4; ++i) {
            if (i < 3 && i >= n_in) { weight_dev_[i].Free(); continue; }
            const float* const src = i < 3 ? in_proj_weight_.data() + (size_t)start[i] * E : out_proj_weight_.data();
            const SiConv2dDesc d = LinearDesc(1, E, E, i < 3 ? count[i] : E, i < 3 ? count[i] : E, false);
            if (half) {
                if (si_hip_conv2d_f16_supported(&d) != 1) {
                    LOG(ERROR) << "MultiheadAttention: no fp16 projection kernel for embed_dim " << E;
                    return Status::kUnsupport;
                }
                std::vector<uint16_t> packed(si_hip_conv2d_f16_weight_elems(&d));
                CHECK_STATUS(CheckHip(si_hip_conv2d_f16_pack_weight_host(&d, src, packed.data()), "pack fp16 weight"));
                CHECK_STATUS(CheckHip(weight_dev_[i].Upload(packed.data(), packed.size() * sizeof(uint16_t)), "upload weight"));
            } else {
                std::vector<float> packed(si_hip_conv2d_weight_elems(&d));
                CHECK_STATUS(CheckHip(si_hip_conv2d_pack_weight_host(&d, src, packed.data()), "pack weight"));
                CHECK_STATUS(CheckHip(weight_dev_[i].Upload(packed.data(), packed.size() * sizeof(float)), "upload weight"));
            }
        }
        if (use_bias_) {
            std::vector<float> all(in_proj_bias_);
            all.insert(all.end(), out_proj_bias_.begin(), out_proj_bias_.end());
            CHECK_BOOL(all.size() == (size_t)4 * E);
            CHECK_STATUS(CheckHip(bias_dev_.Upload(all.data(), all.size() * sizeof(float)), "upload attention bias"));
        }
        prepared_half_ = half;
        prepared_inputs_ = n_in;
        device_ready_ = true;
    }
    const size_t es = half ? 2 : 4;
    const size_t rows_q = (size_t)g.batch * g.lq, rows_k = (size_t)g.batch * g.lk;
    const size_t need = Align256((rows_q > rows_k ? rows_q : rows_k) * 3 * E * es) + rows_q * E * es;
    if (need > workspace_dev_.bytes()) CHECK_STATUS(CheckHip(workspace_dev_.Alloc(need), "attention workspace"));
    return Status::kSuccess;
}

Status MultiheadAttention::Run(const std::vector<Tensor>& in, Tensor& out) {
    const int n_in = (int)in.size();
    const bool half = IsHalf(in[0]);
    for (const Tensor& t : in)
        if (IsHalf(t) != half) return Status::kUnsupport;
    if (IsHalf(out) != half) return Status::kUnsupport;
    std::vector<const Tensor*> ptrs;
    for (const Tensor& t : in) ptrs.push_back(&t);
    Geometry g;
    SiAttentionDesc ad;
    if (!GetGeometry(ptrs, out, g) || !MakeDesc(g, ad)) return Status::kErrorShape;
    CHECK_STATUS(PrepareDevice(half, n_in, g));

    const int E = embed_dim_;
    const size_t es = half ? 2 : 4;
    const int rows_q = g.batch * g.lq, rows_k = g.batch * g.lk;
    char* const ws = workspace_dev_.As<char>();
    char* const att = ws + Align256((size_t)(rows_q > rows_k ? rows_q : rows_k) * 3 * E * es);
    const float* const bias = use_bias_ ? bias_dev_.As<float>() : nullptr;

    auto linear = [&](const void* src, int rows, int in_ld, const DeviceBuffer& w, const float* b, int oc, void* dst, int out_ld, const char* what) {
        const SiConv2dDesc d = LinearDesc(rows, E, in_ld, oc, out_ld, b != nullptr);
        if (half) return CheckHip(si_hip_conv2d_f16(&d, src, w.As<void>(), b, nullptr, dst, 0, Stream()), what);
        return CheckHip(si_hip_conv2d_f32(&d, static_cast<const float*>(src), w.As<float>(), b, nullptr, static_cast<float*>(dst), Stream()), what);
    };

    // 1. the input projection into the column slices Q | K | V of the workspace
    const int start[3] = {0, E, 2 * E};
    const int count[3] = {n_in == 1 ? 3 * E : E, n_in == 2 ? 2 * E : E, E};
    for (int i = 0; i < n_in; ++i)
        CHECK_STATUS(linear(in[i].RawData(), i == 0 ? rows_q : rows_k, in[i].PixelStride(), weight_dev_[i], bias ? bias + start[i] : nullptr, count[i],
                            ws + (size_t)start[i] * es, 3 * E, "MultiheadAttention in_proj"));
    // 2. attention on the strided views
    const void* const q = ws;
    const void* const k = ws + (size_t)E * es;
    const void* const v = ws + (size_t)2 * E * es;
    const int rc = half ? si_hip_attention_f16(&ad, q, k, v, att, Stream())
                        : si_hip_attention_f32(&ad, static_cast<const float*>(q), static_cast<const float*>(k), static_cast<const float*>(v),
                                               reinterpret_cast<float*>(att), Stream());
    CHECK_STATUS(CheckHip(rc, "MultiheadAttention attention"));
    // 3. the output projection into the output operand
    return linear(att, rows_q, E, weight_dev_[3], bias ? bias + 3 * E : nullptr, E, out.RawData(), out.PixelStride(), "MultiheadAttention out_proj");
}

Status MultiheadAttention::Forward(const Tensor& input, Tensor& output) {
    return RunOnDevice({&input}, {&output}, [this](const std::vector<Tensor>& in, std::vector<Tensor>& out) { return Run(in, out[0]); });
}

Status MultiheadAttention::Forward(const std::vector<Tensor>& inputs, Tensor& output) {
    if (inputs.empty() || inputs.size() > 3) return Status::kUnsupport;
    std::vector<const Tensor*> in;
    for (const Tensor& t : inputs) in.push_back(&t);
    return RunOnDevice(in, {&output}, [this](const std::vector<Tensor>& din, std::vector<Tensor>& out) { return Run(din, out[0]); });
}

const char* MultiheadAttention::KernelName() const {
    if (input_tensor_nodes_.empty() || output_tensor_nodes_.empty()) return "attention";
    std::vector<const Tensor*> in;
    for (auto* n : input_tensor_nodes_) in.push_back(&n->tensor);
    Geometry g;
    SiAttentionDesc d;
    if (!GetGeometry(in, output_tensor_nodes_[0]->tensor, g) || !MakeDesc(g, d)) return "attention";
    // (the views are slices of the layer's own workspace, 256-byte aligned and disjoint: the name is asked for such addresses)
    const uintptr_t base = (uintptr_t)1 << 40, apart = (uintptr_t)1 << 34;
    return si_hip_attention_kernel_name(&d, (const void*)base, (const void*)(base + 256), (const void*)(base + 512), (const void*)(base + apart),
                                        IsHalf(*in[0]) ? 1 : 0);
}

// the three input projections, the output projection, and per (batch, head) the two products of lq x lk x d
double MultiheadAttention::Flops() const {
    if (input_tensor_nodes_.empty() || output_tensor_nodes_.empty()) return 0.0;
    std::vector<const Tensor*> in;
    for (auto* n : input_tensor_nodes_) in.push_back(&n->tensor);
    Geometry g;
    if (!GetGeometry(in, output_tensor_nodes_[0]->tensor, g)) return 0.0;
    const double E = embed_dim_, rows_q = (double)g.batch * g.lq, rows_k = (double)g.batch * g.lk;
    return 2.0 * E * E * (2.0 * rows_q + 2.0 * rows_k) + 4.0 * g.batch * (double)g.lq * g.lk * E;
}

bool MultiheadAttention::HalfStorageOk(std::string& why) const {
    if (!Layer::HalfStorageOk(why)) return false;
    bool half = false;
    for (auto* n : input_tensor_nodes_) half = half || IsHalf(n->tensor);
    if (!half) return true;
    if (embed_dim_ % 8 != 0) { why = "MultiheadAttention's fp16 kernels need embed_dim % 8 == 0"; return false; }
    if (num_heads_ > 0 && (embed_dim_ / num_heads_) % 8 != 0) { why = "MultiheadAttention's fp16 kernel needs head_dim % 8 == 0"; return false; }
    return true;
}

}  // namespace SimpleInfer
