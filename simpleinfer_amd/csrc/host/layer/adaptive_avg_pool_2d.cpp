#include "adaptive_avg_pool_2d.h"

#include <cstring>

#include "layer_util.h"
#include "si_hip.h"
#include "si_pool.h"

namespace SimpleInfer {

DEFINE_LAYER_REGISTRY(AdaptiveAvgPool2d);

Status AdaptiveAvgPool2d::Init(const pnnx::Operator* op) {
    CHECK_STATUS(Layer::Init(op));
    std::vector<int> v;
    CHECK_BOOL(Get(op, "output_size", v) && 2 == v.size());
    output_h_ = v[0];
    output_w_ = v[1];
    return Status::kSuccess;
}

Status AdaptiveAvgPool2d::Validate() {
    CHECK_STATUS(Layer::Validate());
    CHECK_STATUS(ValidateShape(1, 1));
    CHECK_STATUS(ValidateFloatLogged("AdaptiveAvgPool2d"));
    return Status::kSuccess;
}

Status AdaptiveAvgPool2d::Forward(const Tensor& input, Tensor& output) {
    return RunOnDevice({&input}, {&output}, [this](const std::vector<Tensor>& in, std::vector<Tensor>& out) {
        Dims4 id, od;
        if (!GetDims4(in[0], id) || !GetDims4(out[0], od) || id.c != od.c || id.n != od.n) return Status::kErrorShape;
        if (IsHalf(in[0]) != IsHalf(out[0])) return Status::kUnsupport;
        // torch's general windows [floor(j i / o), ceil((j + 1) i / o)): include/si_pool.h (the divisible shapes keep the kernels below and their bits)
        if (0 != id.h % od.h || 0 != id.w % od.w)
            return LaunchDesc(si_hip_avgpool2d_f32, si_hip_avgpool2d_f16, "AdaptiveAvgPool2d", in[0], out[0], MakeGeneralDesc);
        if (IsHalf(in[0]))
            return CheckHip(si_hip_adaptive_avgpool2d_f16(in[0].RawData(), id.n, id.h, id.w, id.c, in[0].PixelStride(),
                                                          out[0].RawData(), od.h, od.w, out[0].PixelStride(), Stream()),
                            "AdaptiveAvgPool2d");
        return CheckHip(si_hip_adaptive_avgpool2d_f32(in[0].Data<float>(), id.n, id.h, id.w, id.c, in[0].PixelStride(),
                                                      out[0].Data<float>(), od.h, od.w, out[0].PixelStride(), Stream()),
                        "AdaptiveAvgPool2d");
    });
}

bool AdaptiveAvgPool2d::MakeGeneralDesc(const Tensor& input, const Tensor& output, SiAvgPool2dDesc& d) {
    Dims4 id, od;
    if (!GetDims4(input, id) || !GetDims4(output, od) || id.c != od.c || id.n != od.n) return false;
    memset(&d, 0, sizeof(d));
    d.n = id.n; d.ih = id.h; d.iw = id.w; d.c = id.c; d.in_ld = input.PixelStride();
    d.oh = od.h; d.ow = od.w; d.out_ld = output.PixelStride();
    d.adaptive = 1;
    return 0 != id.h % od.h || 0 != id.w % od.w;
}

// "avgpool" for the divisible shapes, as before; the instantiation of include/si_pool.h for the others
const char* AdaptiveAvgPool2d::KernelName() const {
    return DescKernelName(si_hip_avgpool2d_kernel_name, "avgpool", MakeGeneralDesc, true);
}

}  // namespace SimpleInfer
