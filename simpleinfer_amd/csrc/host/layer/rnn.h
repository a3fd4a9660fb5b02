// layer/rnn.h -- nn.LSTM / nn.GRU (torch semantics, eval mode, zero initial state, no projection; no reference counterpart): one class with a
// cell kind.  Every layer of the stack is three stages in stream order: the input projection of all t * batch rows and both directions
// through the 1x1 path of si_hip_conv2d_f32 / _f16 into a gate workspace, t launches of the step kernel (include/si_rnn.h), and, for the
// multi-output form, the state copy.  Layer l + 1 projects the [T, N, D H] output of layer l; the last layer writes the output operand, inner
// layers a workspace.  The parameter and attribute keys are the ones pnnx writes for the modules.  One input of rank 3: [T, N, I], or
// [N, T, I] with batch_first; outputs y alone, or y, h_n, c_n (LSTM) / y, h_n (GRU) with the states as [layers * D, N, H].
#ifndef SIMPLE_INFER_SRC_LAYER_RNN_H_
#define SIMPLE_INFER_SRC_LAYER_RNN_H_

#include "layer.h"
#include "layer_util.h"
#include "si_rnn.h"

namespace SimpleInfer {

class Rnn : public Layer {
public:
    virtual Status Init(const pnnx::Operator* op) override;
    virtual Status Deinit() override;
    virtual Status Validate() override;
    virtual Status Forward(const Tensor& input, Tensor& output) override;
    virtual Status Forward(const Tensor& input, std::vector<Tensor>& outputs) override;

    virtual const char* KernelName() const override;
    virtual double Flops() const override;
    virtual double Bytes() const override;
    virtual bool HalfStorageOk(std::string& why) const override;

public:
    int cell_ = SI_RNN_LSTM;   // SI_RNN_LSTM / SI_RNN_GRU, by the operator's type string
    int input_size_ = 0, hidden_size_ = 0, num_layers_ = 1, proj_size_ = 0;
    bool use_bias_ = true, batch_first_ = false, bidirectional_ = false;
    // [layer * dirs + dir]: weight_ih (G H, I_l), weight_hh (G H, H), bias_ih (G H), bias_hh (G H)
    std::vector<std::vector<float>> weight_ih_, weight_hh_, bias_ih_, bias_hh_;

private:
    struct Geometry {
        int t = 0, batch = 0;
    };
    int Gates() const { return cell_ == SI_RNN_LSTM ? 4 : 3; }
    int Dirs() const { return bidirectional_ ? 2 : 1; }
    int LayerInput(int layer) const { return layer == 0 ? input_size_ : Dirs() * hidden_size_; }
    size_t StateOutputs() const { return cell_ == SI_RNN_LSTM ? 2 : 1; }
    bool GetGeometry(const Tensor& in, const std::vector<const Tensor*>& outs, Geometry& g) const;
    // the descriptor of layer `layer` reading rows of in_ld elements and writing rows of out_ld elements
    SiRnnDesc MakeDesc(const Geometry& g, int layer, long long in_ld, long long out_ld) const;
    Status PrepareDevice(bool half, const Geometry& g);
    Status Run(const Tensor& in, std::vector<Tensor>& outs);

    struct LayerBuffers {
        DeviceBuffer w_ih, bias, b_hn, w_hh;   // conv weight image [D G H, I_l]; projection bias [D G H]; GRU b_hn [D, H]; W_hh image
    };
    std::vector<LayerBuffers> dev_;
    DeviceBuffer gates_dev_, state_dev_, inner_dev_[2];   // [T N, D G H]; c [D, N, H] fp32; the outputs of the inner layers, alternating
    bool device_ready_ = false, prepared_half_ = false;
    mutable bool half_refused_ = false;
};

}  // namespace SimpleInfer

#endif
