#include "layer_registry.h"

#include <map>
#include <set>

namespace SimpleInfer {

#define SI_DECLARE_LAYER(type)    \
    Layer* type##_LayerCreator(); \
    void type##_LayerDestroyer(Layer*);

SI_DECLARE_LAYER(AdaptiveAvgPool2d)
SI_DECLARE_LAYER(AffineGrid)
SI_DECLARE_LAYER(AvgPool2d)
SI_DECLARE_LAYER(BatchNorm2d)
SI_DECLARE_LAYER(BinaryOp)
SI_DECLARE_LAYER(Cat)
SI_DECLARE_LAYER(Conv1d)
SI_DECLARE_LAYER(Conv2d)
SI_DECLARE_LAYER(ConvTranspose2d)
SI_DECLARE_LAYER(DeformConv2d)
SI_DECLARE_LAYER(Flatten)
SI_DECLARE_LAYER(FunctionalConv2d)
SI_DECLARE_LAYER(GridSample)
SI_DECLARE_LAYER(GroupNorm)
SI_DECLARE_LAYER(HardSigmoid)
SI_DECLARE_LAYER(HardSwish)
SI_DECLARE_LAYER(Layout)
SI_DECLARE_LAYER(LeakyReLU)
SI_DECLARE_LAYER(Linear)
SI_DECLARE_LAYER(LpNorm)
SI_DECLARE_LAYER(MaxPool2d)
SI_DECLARE_LAYER(MultiheadAttention)
SI_DECLARE_LAYER(Pad2d)
SI_DECLARE_LAYER(ParamActivation)
SI_DECLARE_LAYER(PixelShuffle)
SI_DECLARE_LAYER(PReLU)
SI_DECLARE_LAYER(Reduce)
SI_DECLARE_LAYER(ReLU)
SI_DECLARE_LAYER(Rnn)
SI_DECLARE_LAYER(RoiAlign)
SI_DECLARE_LAYER(Sigmoid)
SI_DECLARE_LAYER(SiLU)
SI_DECLARE_LAYER(Slice)
SI_DECLARE_LAYER(Softmax)
SI_DECLARE_LAYER(Tanh)
SI_DECLARE_LAYER(UnaryOp)
SI_DECLARE_LAYER(Upsample)
SI_DECLARE_LAYER(YoloDetect)

#define SI_ENTRY(pnnx_type, type) \
    { pnnx_type, LayerRegistryEntry{type##_LayerCreator, type##_LayerDestroyer} }

static std::map<std::string, LayerRegistryEntry>& Table() {
    // the 15 type strings of reference src/layer_registry.cpp:33-49, plus nn.LeakyReLU
    // (north_star extension) nn.ConvTranspose2d (U-Net / segmentation decoders; no reference layer)
    // F.interpolate / F.upsample, the functional spellings of nn.Upsample, and nn.GroupNorm / nn.InstanceNorm2d (one class: the
    // instance norm is the group norm with one group per channel); the explicit pads (one class, layer/pad_2d.h) and nn.Tanh
    // (UnaryOp code 16 as a module); nn.AvgPool2d / F.avg_pool2d (layer/avg_pool_2d.h) and the functional spelling of the adaptive pool;
    // nn.Softmax / nn.LogSoftmax / nn.Softmax2d / F.softmax / F.log_softmax (one class, layer/softmax.h); nn.PixelShuffle / nn.PixelUnshuffle /
    // F.pixel_shuffle / F.pixel_unshuffle (one class, layer/pixel_shuffle.h) and nn.PReLU (layer/prelu.h); torch.chunk / torch.split /
    // Tensor.slice (one class, layer/slice.h); torch.mean / torch.sum / torch.amax / torch.amin (one class, layer/reduce.h); nn.ReLU6 / nn.Hardtanh /
    // torch.clamp / nn.Softplus / nn.Mish and their F.* spellings (one class, layer/param_activation.h: never folded into an epilogue); the
    // functional spellings of the activations above, on the classes of their nn.* twins (they fuse as those do; F.tanh, like nn.Tanh, does not);
    // Tensor.permute / torch.permute / Tensor.reshape / Tensor.view / torch.transpose / torch.squeeze / torch.unsqueeze / Tensor.contiguous (one
    // class, layer/layout.h: the layout algebra of layout_plan.h decides between a view and one permute launch); nn.MultiheadAttention
    // (layer/multihead_attention.h: two projections around the fused attention kernel of include/si_attention.h); torchvision.ops.DeformConv2d
    // (layer/deform_conv_2d.h: DCNv1 / DCNv2 in one launch of include/si_deform.h; the type string is the one pnnx writes for the module);
    // F.grid_sample and F.affine_grid (layer/grid_sample.h, layer/affine_grid.h: the sampler and the tiny grid kernel of include/si_grid.h);
    // torchvision.ops.RoIAlign / torchvision.ops.roi_align (one class, layer/roi_align.h: the box-pooling kernel of include/si_roi.h);
    // nn.LSTM / nn.GRU (one class with a cell kind, layer/rnn.h: the input projection and the recurrent step kernel of include/si_rnn.h);
    // nn.Conv1d (layer/conv_1d.h: the temporal convolution kernels of include/si_conv1d.h on rank-3 operands in their native layout);
    // F.conv2d (layer/functional_conv_2d.h: the filter is an operand, read as stored by the cross-correlation kernels of include/si_xcorr.h);
    // F.normalize / torch.norm (one class, layer/lp_norm.h: the Lp-norm kernels of include/si_lpnorm.h)
    static std::map<std::string, LayerRegistryEntry> table = {
        SI_ENTRY("nn.AdaptiveAvgPool2d", AdaptiveAvgPool2d),
        SI_ENTRY("nn.AvgPool2d", AvgPool2d),
        SI_ENTRY("nn.BatchNorm2d", BatchNorm2d),
        SI_ENTRY("nn.CircularPad2d", Pad2d),
        SI_ENTRY("nn.ConstantPad2d", Pad2d),
        SI_ENTRY("BinaryOp", BinaryOp),
        SI_ENTRY("torch.cat", Cat),
        SI_ENTRY("nn.Conv2d", Conv2d),
        SI_ENTRY("nn.ConvTranspose2d", ConvTranspose2d),
        SI_ENTRY("torch.flatten", Flatten),
        SI_ENTRY("nn.GroupNorm", GroupNorm),
        SI_ENTRY("nn.Hardsigmoid", HardSigmoid),
        SI_ENTRY("nn.Hardswish", HardSwish),
        SI_ENTRY("nn.InstanceNorm2d", GroupNorm),
        SI_ENTRY("nn.LeakyReLU", LeakyReLU),
        SI_ENTRY("nn.LogSoftmax", Softmax),
        SI_ENTRY("nn.Linear", Linear),
        SI_ENTRY("nn.MaxPool2d", MaxPool2d),
        SI_ENTRY("nn.MultiheadAttention", MultiheadAttention),
        SI_ENTRY("nn.PixelShuffle", PixelShuffle),
        SI_ENTRY("nn.PixelUnshuffle", PixelShuffle),
        SI_ENTRY("nn.PReLU", PReLU),
        SI_ENTRY("nn.ReflectionPad2d", Pad2d),
        SI_ENTRY("nn.ReLU", ReLU),
        SI_ENTRY("nn.ReplicationPad2d", Pad2d),
        SI_ENTRY("nn.Sigmoid", Sigmoid),
        SI_ENTRY("nn.SiLU", SiLU),
        SI_ENTRY("nn.Softmax", Softmax),
        SI_ENTRY("nn.Softmax2d", Softmax),
        SI_ENTRY("nn.Tanh", Tanh),
        SI_ENTRY("UnaryOp", UnaryOp),   // emitted by expand_expression, never registered by the reference
        SI_ENTRY("nn.Upsample", Upsample),
        SI_ENTRY("nn.ZeroPad2d", Pad2d),
        SI_ENTRY("F.interpolate", Upsample),
        SI_ENTRY("F.upsample", Upsample),
        SI_ENTRY("F.pad", Pad2d),
        SI_ENTRY("F.avg_pool2d", AvgPool2d),
        SI_ENTRY("F.adaptive_avg_pool2d", AdaptiveAvgPool2d),
        SI_ENTRY("F.softmax", Softmax),
        SI_ENTRY("F.log_softmax", Softmax),
        SI_ENTRY("F.pixel_shuffle", PixelShuffle),
        SI_ENTRY("F.pixel_unshuffle", PixelShuffle),
        SI_ENTRY("torch.chunk", Slice),
        SI_ENTRY("torch.split", Slice),
        SI_ENTRY("Tensor.slice", Slice),
        SI_ENTRY("torch.mean", Reduce),
        SI_ENTRY("torch.sum", Reduce),
        SI_ENTRY("torch.amax", Reduce),
        SI_ENTRY("torch.amin", Reduce),
        SI_ENTRY("nn.ReLU6", ParamActivation),
        SI_ENTRY("F.relu6", ParamActivation),
        SI_ENTRY("nn.Hardtanh", ParamActivation),
        SI_ENTRY("F.hardtanh", ParamActivation),
        SI_ENTRY("torch.clamp", ParamActivation),
        SI_ENTRY("nn.Softplus", ParamActivation),
        SI_ENTRY("F.softplus", ParamActivation),
        SI_ENTRY("nn.Mish", ParamActivation),
        SI_ENTRY("F.mish", ParamActivation),
        SI_ENTRY("F.relu", ReLU),
        SI_ENTRY("F.silu", SiLU),
        SI_ENTRY("F.sigmoid", Sigmoid),
        SI_ENTRY("F.hardsigmoid", HardSigmoid),
        SI_ENTRY("F.hardswish", HardSwish),
        SI_ENTRY("F.leaky_relu", LeakyReLU),
        SI_ENTRY("F.tanh", Tanh),
        SI_ENTRY("Tensor.permute", Layout),
        SI_ENTRY("torch.permute", Layout),
        SI_ENTRY("Tensor.reshape", Layout),
        SI_ENTRY("Tensor.view", Layout),
        SI_ENTRY("torch.transpose", Layout),
        SI_ENTRY("torch.squeeze", Layout),
        SI_ENTRY("torch.unsqueeze", Layout),
        SI_ENTRY("Tensor.contiguous", Layout),
        SI_ENTRY("models.yolo.Detect", YoloDetect),
        SI_ENTRY("torchvision.ops.DeformConv2d", DeformConv2d),
        SI_ENTRY("F.grid_sample", GridSample),
        SI_ENTRY("F.affine_grid", AffineGrid),
        SI_ENTRY("torchvision.ops.RoIAlign", RoiAlign),
        SI_ENTRY("torchvision.ops.roi_align", RoiAlign),
        SI_ENTRY("nn.LSTM", Rnn),
        SI_ENTRY("nn.GRU", Rnn),
        SI_ENTRY("nn.Conv1d", Conv1d),
        SI_ENTRY("F.conv2d", FunctionalConv2d),
        SI_ENTRY("F.normalize", LpNorm),
        SI_ENTRY("torch.norm", LpNorm),
    };
    return table;
}

const LayerRegistryEntry* GetLayerRegistry(std::string type) {
    auto& t = Table();
    auto it = t.find(type);
    return it == t.end() ? nullptr : &it->second;
}

static std::set<std::string>& UserTypes() {
    static std::set<std::string> types;
    return types;
}

bool RegisterLayer(const std::string& type, LayerCreatorFunc creator, LayerDestroyerFunc destroyer) {
    if (!creator || !destroyer) return false;
    Table()[type] = LayerRegistryEntry{creator, destroyer};
    UserTypes().insert(type);
    return true;
}

bool IsUserRegisteredLayer(const std::string& type) { return UserTypes().count(type) > 0; }

std::vector<std::string> RegisteredLayerTypes() {
    std::vector<std::string> out;
    for (auto& kv : Table()) out.push_back(kv.first);
    return out;
}

}  // namespace SimpleInfer
