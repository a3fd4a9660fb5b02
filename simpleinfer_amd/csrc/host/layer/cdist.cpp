#include "cdist.h"

#include <cmath>
#include <cstring>

namespace SimpleInfer {

DEFINE_LAYER_REGISTRY(Cdist);

Status Cdist::Refuse(const std::string& why, Status status) const {
    LOG(ERROR) << "torch.cdist [" << (op_ ? op_->name : std::string("-")) << "] refused [" << why << "]";
    return status;
}

// A key of another type is kFail; a p or a compute_mode the kernels do not serve is kUnsupport; shapes are left for Validate.
Status Cdist::Init(const pnnx::Operator* op) {
    CHECK_STATUS(Layer::Init(op));
    float p = 2.0f;
    std::string text;
    if (Get(op, "p", text)) {
        if (text != "inf") return Refuse("p=" + text + ": p = 1, 2 and inf only", Status::kUnsupport);
        p = INFINITY;
    } else if (FindParam(op, "p")) {
        CHECK_BOOL(GetNumber(op, "p", p));
    }
    if (p == 1.0f) norm_ = SI_CDIST_NORM_1;
    else if (p == 2.0f) norm_ = SI_CDIST_NORM_2;
    else if (std::isinf(p) && p > 0.0f) norm_ = SI_CDIST_NORM_INF;
    else return Refuse("p=" + std::to_string(p) + ": p = 1, 2 and inf only", Status::kUnsupport);
    mode_ = SI_CDIST_MODE_MM_IF_NECESSARY;
    if (!IsNone(op, "compute_mode")) {
        std::string mode;
        CHECK_BOOL(Get(op, "compute_mode", mode));
        if (mode == "None" || mode == "use_mm_for_euclid_dist_if_necessary") mode_ = SI_CDIST_MODE_MM_IF_NECESSARY;
        else if (mode == "use_mm_for_euclid_dist") mode_ = SI_CDIST_MODE_MM;
        else if (mode == "donot_use_mm_for_euclid_dist") mode_ = SI_CDIST_MODE_NO_MM;
        else return Refuse("compute_mode=" + mode + " is none of torch's three", Status::kUnsupport);
    }
    int rows = 0;
    if (FindParam(op, "nearest_rows")) CHECK_BOOL(Get(op, "nearest_rows", rows));
    nearest_rows_ = rows != 0;
    if (nearest_rows_ && norm_ != SI_CDIST_NORM_2) return Refuse("nearest_rows with p != 2: the fused search is Euclidean", Status::kUnsupport);
    return Status::kSuccess;
}

SiNearestDesc Cdist::NearestDesc(const SiCdistDesc& d) {
    SiNearestDesc n;
    memset(&n, 0, sizeof(n));
    n.b1 = d.b1; n.b2 = d.b2; n.p = d.p; n.r = d.r; n.m = d.m;
    n.x1_ld = d.x1_ld; n.x2_ld = d.x2_ld; n.rows_ld = d.out_ld;
    n.x1_sb = d.x1_sb; n.x2_sb = d.x2_sb; n.rows_sb = d.out_sb;
    n.k = 1;
    n.splits = 1;
    return n;
}

bool Cdist::MakeDesc(const Tensor& x1, const Tensor& x2, const Tensor& out, SiCdistDesc& d, std::string* why) const {
    auto fail = [&](const std::string& text) {
        if (why) *why = text;
        return false;
    };
    const std::vector<int>&s1 = x1.Shape(), &s2 = x2.Shape(), &so = out.Shape();
    for (const std::vector<int>* s : {&s1, &s2}) {
        if (s->size() != 2 && s->size() != 3)
            return fail("a rank-" + std::to_string(s->size()) + " operand " + ShapeString(*s) + ": ranks 2 [P, M] and 3 [B, P, M] are served");
        for (int e : *s)
            if (e <= 0) return fail("an empty operand " + ShapeString(*s));
    }
    memset(&d, 0, sizeof(d));
    d.b1 = s1.size() == 3 ? s1[0] : 1;
    d.b2 = s2.size() == 3 ? s2[0] : 1;
    d.p = s1[s1.size() - 2];
    d.r = s2[s2.size() - 2];
    d.m = s1.back();
    if (s2.back() != d.m) return fail("rows of " + std::to_string(d.m) + " and of " + std::to_string(s2.back()) + " elements: the last dimensions differ");
    if (d.b1 != d.b2 && d.b1 != 1 && d.b2 != 1)
        return fail("batch dimensions " + std::to_string(d.b1) + " and " + std::to_string(d.b2) + ": equal, or one of them 1");
    const int batch = d.b1 > d.b2 ? d.b1 : d.b2;
    std::vector<int> want = {d.p, nearest_rows_ ? d.m : d.r};   // the winning rows of x2, or the distances
    if (s1.size() == 3 || s2.size() == 3) want.insert(want.begin(), batch);
    if (so != want) return fail("the output is " + ShapeString(so) + ", the operands " + ShapeString(s1) + " and " + ShapeString(s2) + " give " + ShapeString(want));
    d.x1_ld = x1.PixelStride();
    d.x2_ld = x2.PixelStride();
    d.out_ld = out.PixelStride();
    const long long sb1 = (long long)d.p * d.x1_ld, sb2 = (long long)d.r * d.x2_ld, sbo = (long long)d.p * d.out_ld;
    if (sb1 > 0x7fffffffLL || sb2 > 0x7fffffffLL || sbo > 0x7fffffffLL) return fail("element offsets beyond 31 bits");
    d.x1_sb = (int)sb1;
    d.x2_sb = (int)sb2;
    d.out_sb = (int)sbo;
    d.norm = norm_;
    d.mode = mode_;
    return true;
}

Status Cdist::Validate() {
    CHECK_STATUS(Layer::Validate());
    CHECK_STATUS(ValidateShape(2, 1));
    CHECK_STATUS(ValidateFloatLogged("Cdist"));
    SiCdistDesc d;
    std::string why;
    if (!MakeDesc(input_tensor_nodes_[0]->tensor, input_tensor_nodes_[1]->tensor, output_tensor_nodes_[0]->tensor, d, &why))
        return Refuse(why, Status::kErrorShape);
    // (the pointers are compared, never followed: three aligned addresses far apart)
    const uintptr_t base = (uintptr_t)1 << 40, apart = (uintptr_t)1 << 34;
    const SiNearestDesc n = NearestDesc(d);
    const char* const name = nearest_rows_ ? si_hip_nearest_kernel_name(&n, (const void*)base, (const void*)(base + apart), (const void*)(base + 2 * apart), 0)
                                           : si_hip_cdist_kernel_name(&d, (const void*)base, (const void*)(base + apart), (const void*)(base + 2 * apart), 0);
    if (0 == strcmp("none", name))
        return Refuse("the kernels refuse these tensors (element offsets beyond 31 bits)", Status::kUnsupport);
    return Status::kSuccess;
}

Status Cdist::Forward(const std::vector<Tensor>& inputs, Tensor& output) {
    if (inputs.size() != 2) return Status::kErrorShape;
    return RunOnDevice({&inputs[0], &inputs[1]}, {&output}, [this](const std::vector<Tensor>& in, std::vector<Tensor>& out) {
        const bool half = IsHalf(in[0]);
        if (IsHalf(in[1]) != half || IsHalf(out[0]) != half) return Status::kUnsupport;
        SiCdistDesc d;
        if (!MakeDesc(in[0], in[1], out[0], d)) return Status::kErrorShape;
        if (nearest_rows_) {
            const SiNearestDesc n = NearestDesc(d);
            const int rc = half ? si_hip_nearest_f16(&n, in[0].RawData(), in[1].RawData(), nullptr, nullptr, out[0].RawData(), nullptr, 0, Stream())
                                : si_hip_nearest_f32(&n, in[0].Data<float>(), in[1].Data<float>(), nullptr, nullptr, out[0].Data<float>(), nullptr, 0, Stream());
            return CheckHip(rc, "Cdist (nearest rows)");
        }
        const int rc = half ? si_hip_cdist_f16(&d, in[0].RawData(), in[1].RawData(), out[0].RawData(), Stream())
                            : si_hip_cdist_f32(&d, in[0].Data<float>(), in[1].Data<float>(), out[0].Data<float>(), Stream());
        return CheckHip(rc, "Cdist");
    });
}

const char* Cdist::KernelName() const {
    if (input_tensor_nodes_.size() != 2 || output_tensor_nodes_.empty()) return "cdist";
    const Tensor &x1 = input_tensor_nodes_[0]->tensor, &x2 = input_tensor_nodes_[1]->tensor, &out = output_tensor_nodes_[0]->tensor;
    SiCdistDesc d;
    if (!MakeDesc(x1, x2, out, d) || !x1.RawData() || !x2.RawData() || !out.RawData()) return "cdist";
    if (nearest_rows_) {
        const SiNearestDesc n = NearestDesc(d);
        return si_hip_nearest_kernel_name(&n, x1.RawData(), x2.RawData(), out.RawData(), IsHalf(x1) ? 1 : 0);
    }
    return si_hip_cdist_kernel_name(&d, x1.RawData(), x2.RawData(), out.RawData(), IsHalf(x1) ? 1 : 0);
}

// per pair of rows: M products and M additions on the matrix cores, or M differences, magnitudes (squares) and additions
double Cdist::Flops() const {
    if (input_tensor_nodes_.size() != 2 || output_tensor_nodes_.empty()) return 0.0;
    SiCdistDesc d;
    if (!MakeDesc(input_tensor_nodes_[0]->tensor, input_tensor_nodes_[1]->tensor, output_tensor_nodes_[0]->tensor, d)) return 0.0;
    const double pairs = (double)(d.b1 > d.b2 ? d.b1 : d.b2) * d.p * d.r;
    const bool mm = nearest_rows_ || d.norm == SI_CDIST_NORM_2 && d.mode != SI_CDIST_MODE_NO_MM &&
                    (d.mode == SI_CDIST_MODE_MM || d.p > SI_CDIST_MM_THRESHOLD || d.r > SI_CDIST_MM_THRESHOLD);
    return (mm ? 2.0 : 3.0) * pairs * d.m;
}

// one read of each operand (the panels a tile re-reads come from L2), one write of the output
double Cdist::Bytes() const {
    if (input_tensor_nodes_.size() != 2 || output_tensor_nodes_.empty()) return 0.0;
    return (double)input_tensor_nodes_[0]->tensor.ByteSize() + (double)input_tensor_nodes_[1]->tensor.ByteSize() +
           (double)output_tensor_nodes_[0]->tensor.ByteSize();
}

bool Cdist::HalfStorageOk(std::string& why) const {
    bool any = false, all = true;
    for (auto* n : input_tensor_nodes_) { any = any || IsHalf(n->tensor); all = all && IsHalf(n->tensor); }
    for (auto* n : output_tensor_nodes_) { any = any || IsHalf(n->tensor); all = all && IsHalf(n->tensor); }
    if (!any) return true;
    if (!all) {
        why = "torch.cdist reads both operands and writes the output in one storage type";
        return false;
    }
    if (!input_tensor_nodes_.empty() && input_tensor_nodes_[0]->tensor.Shape().back() % 8 != 0) {
        why = "torch.cdist's fp16 kernels need rows of a multiple of 8 elements";
        return false;
    }
    return true;
}

}  // namespace SimpleInfer
