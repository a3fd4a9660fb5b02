/*
 * si_rnn.h -- C-ABI of the recurrent step kernel behind nn.LSTM / nn.GRU (torch inference semantics, one layer, one or two directions, zero
 * initial state, no projection; no reference counterpart).  The symbols live in libsi_hip.so beside those of include/si_hip.h; they have a
 * header of their own as include/si_attention.h has.
 *
 *     LSTM   i, f, o = sigmoid(.), g = tanh(.) of  W_i* x_t + b_i* + W_h* h_{t-1} + b_h*      c_t = f c_{t-1} + i g      h_t = o tanh(c_t)
 *     GRU    r, z = sigmoid(.) of the same sum;  n = tanh(W_in x_t + b_in + r (W_hn h_{t-1} + b_hn));  h_t = (1 - z) n + z h_{t-1}
 *     gate order in W_ih / W_hh / the biases: i, f, g, o (LSTM), r, z, n (GRU); G = 4 or 3 gates of H = hidden rows each
 *
 * One layer is three stages in stream order.
 *   1. Input projection -- the CALLER's, through the 1x1 path of si_hip_conv2d_f32 / _f16 (include/si_hip.h): x W_ih^T + bias for all t * batch
 *      rows and both directions in one launch, into the gate workspace [rows, dirs * G * H] (direction-major, then gate, then unit).  The
 *      bias of that launch is summed ONCE on the host in fp32, in this order: LSTM b_ih + b_hh for every gate; GRU b_ih + b_hh for r and z and
 *      b_ih ALONE for n -- b_hn stays inside r * (W_hn h + b_hn) and travels to the step kernel as `b_hn` [dirs, H] fp32 (null: zeros).
 *   2. t launches of the step kernel (si_hip_rnn_layer_*).  One launch is one time step of BOTH directions: forward at time s, reverse at
 *      time t - 1 - s.  The grid runs over (direction, tile of 16 batch rows, block of 64 hidden units); a workgroup of four waves stages its
 *      16 rows of h_{t-1} in LDS once, a wave owns 16 hidden units for ALL gates: G products h_{t-1} W_hh^T on v_mfma_f32_16x16x4_f32 (fp32) or
 *      v_mfma_f32_16x16x32_f16 (fp16 storage) with W_hh as the A operand, read from the image si_hip_rnn_pack_whh_* wrote in MFMA lane
 *      order (k zero-padded to the instruction's k: 4 / 32).  The C/D map leaves the G pre-activations of one (batch row, unit) in one
 *      lane; sigmoid / tanh and the cell update are the epilogue.  h_{t-1} is READ FROM `y`: the previous step's row, columns dir * H ..;
 *      there is no h buffer.  c is an fp32 buffer [dirs, batch, H], updated in place, each element by one lane.  The first step skips the
 *      product (h = 0, c = 0) and reads neither a previous row of y nor c.
 *      No workgroup waits for another one: the dependence of step s + 1 on the whole of h_s is the kernel boundary.
 *   3. optional state outputs, one small launch: h_n [dirs, batch, H] = the last forward / first reverse rows of y; c_n = c rounded to the
 *      storage type (LSTM only).
 *
 * Views.  Row (time s, batch item b) of x / the gates / y starts s * st + b * sb elements into its tensor; that serves seq-first [T, N, F]
 * (st = N * ld, sb = ld), batch_first [N, T, F] (st = ld, sb = T * ld) and column slices of wider rows with the same code.  x belongs to
 * stage 1 alone: its strides make the descriptor the description of the whole layer, the entries below never see the tensor (y may take
 * x's place once the projection has run).  Of y exactly the dirs * H columns of every row are written; the space between rows is untouched.
 *
 * fp16 storage.  y, h_n, c_n, the gate workspace (what the f16 conv entry stores: one rounding) and the W_hh image are halves; products
 * accumulate in fp32; gates, c and the cell arithmetic are fp32; h is rounded ONCE, to nearest even, at the store into y, and the next
 * step reads that rounded value.  H % 8 == 0, input % 8 == 0, every stride a multiple of 8, every pointer 16-byte aligned.
 *
 * Contract.  Every reduction runs in a fixed k-ascending order: two runs give the same bits.  The bits of batch item b depend on item b's
 * data alone -- not on batch, on the item's position in its tile or on the other direction.  Rows, columns and batch items beyond the
 * extents are neither read nor written.  Every launch is safe inside a captured graph; the entries never allocate.  Saturated gates are
 * exact and finite: sigmoid is rcp(1 + exp(-v)) as in nn.Sigmoid (exactly 1 / 0 for pre-activations of +-100 or +-1e4), tanh is tanhf as in
 * nn.Tanh.  A NaN in x[s, b, :] makes item b NaN from s onward in the forward direction and from s backward in the reverse direction, no
 * other item and no earlier (reverse: later) time.
 *
 * Refused before any device call: a null descriptor or tensor (c for an LSTM, c_n without an LSTM), an unknown cell, non-positive sizes,
 * dirs outside 1..2, step0 outside 0..t, a stride below its row width (x: input, gates: dirs * G * H, y: dirs * H) or rows of y that share an
 * element, y intersecting the gates, c, the W_hh image, h_n or c_n (SI_E_BADARG); element offsets, the W_hh image or the grid beyond 31 bits,
 * H above SI_RNN_MAX_HIDDEN, and for fp16 the divisibility / alignment rule above (SI_E_UNSUPPORTED).
 */
#ifndef SI_RNN_H_
#define SI_RNN_H_

#include "si_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

enum { SI_RNN_LSTM = 0, SI_RNN_GRU = 1 };
enum { SI_RNN_TILE_ROWS = 16, SI_RNN_BLOCK_UNITS = 64, SI_RNN_MAX_HIDDEN = 2048 };
/* `which` of si_hip_rnn_workspace_bytes */
enum { SI_RNN_WS_GATES = 0, SI_RNN_WS_STATE = 1, SI_RNN_WS_WHH = 2 };

typedef struct SiRnnDesc {
    int cell;               /* SI_RNN_LSTM / SI_RNN_GRU */
    int t, batch, input, hidden, dirs;
    long long x_st, x_sb;   /* element strides of the time index and of the batch index */
    long long g_st, g_sb;
    long long y_st, y_sb;
    int step0;              /* the first step to run: 0 starts from the zero state; s > 0 continues a call that ran steps 0 .. s - 1 on the same views */
} SiRnnDesc;

/* stages 2 and 3.  gates: the projected [rows, dirs * G * H]; whh: the image of si_hip_rnn_pack_whh_*; b_hn: GRU [dirs, H] or null;
 * c: fp32 [dirs, batch, H] (LSTM; GRU: ignored, may be null); h_n / c_n: [dirs, batch, H] or null */
int si_hip_rnn_layer_f32(const SiRnnDesc* d, const float* gates, const float* whh, const float* b_hn, float* y, float* c, float* h_n, float* c_n,
                         si_stream_t stream);
int si_hip_rnn_layer_f16(const SiRnnDesc* d, const void* gates, const void* whh, const float* b_hn, void* y, float* c, void* h_n, void* c_n,
                         si_stream_t stream);

/* bytes of a caller-owned buffer: the dense gate workspace, the c buffer (0 for a GRU), the W_hh image; 0 for a refused descriptor */
size_t si_hip_rnn_workspace_bytes(const SiRnnDesc* d, int which, int half);

/* host: w_hh fp32 [dirs][G * H][H] (torch's weight_hh_l{k}, then its _reverse twin) -> the image, workspace_bytes(SI_RNN_WS_WHH) bytes */
int si_hip_rnn_pack_whh_f32(const SiRnnDesc* d, const float* w_hh, float* image);
int si_hip_rnn_pack_whh_f16(const SiRnnDesc* d, const float* w_hh, void* image);

/* "rnn_step_kernel<float, 4>" (LSTM) / "<float, 3>" (GRU), "rnn_step_kernel<_Float16, 4>" / "<_Float16, 3>"; "none" for what the launch refuses */
const char* si_hip_rnn_kernel_name(const SiRnnDesc* d, const void* gates, const void* y, int half);

#ifdef __cplusplus
}
#endif

#endif /* SI_RNN_H_ */
