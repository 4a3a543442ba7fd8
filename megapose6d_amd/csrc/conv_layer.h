// One convolution layer of a network executor (backbone.hip, detector.hip), host side only: state_dict lookup, the eval-BatchNorm fold,
// the weight blobs of the kernels a layer may run on, and the dispatch between those kernels.  Defined in conv_layer.hip.
#pragma once
#include <map>
#include <string>
#include <vector>

#include "common.h"

namespace mp {

typedef std::map<std::string, std::pair<const float*, int64_t>> StateMap;   // state_dict key -> (host data, element count)

// `who` names the entry the error text belongs to ("mp_backbone_create" / "mp_detector_create")
const float* find(const StateMap& sm, const std::string& key, int64_t numel, const char* who);
// eval BatchNorm / FrozenBatchNorm2d (eps = 1e-5) -> per-channel (scale, shift)
int bn_affine(const StateMap& sm, const std::string& prefix, int C, const char* who, std::vector<float>& scale, std::vector<float>& shift);
// device copy of `h`, owned by `allocs` (the executor frees them in its destroy)
int upload(std::vector<void*>& allocs, const std::vector<float>& h, float** d);

struct ConvLayer {
  int Cin = 0, Cin_p = 0, Cout = 0, K = 1, stride = 1, pad = 0;   // Cout = channels the kernel writes (zero-padded heads included)
  float* d_w = nullptr;   // packed fp32 weights
  float* d_u = nullptr;   // Winograd-transformed weights of an eligible 3x3 / stride-1 layer: fp32 (conv_wino.hip) ...
  void* d_ub = nullptr;   // ... or split into three exact bf16 pieces (conv_wino_bf16.hip)
  void* d_wb = nullptr;   // the direct weights split into three exact bf16 pieces (conv_bf16x9.hip) of an eligible non-Winograd layer
  float* d_b = nullptr;   // folded BN shift + bias (may be null)
};

// the forms a layer is packed in besides the fp32 one, which every layer has; a form is packed only where the layer's shape fits its kernel
enum ConvForms : unsigned { CONV_FORM_WINO_F32 = 1u, CONV_FORM_WINO_BF16 = 2u, CONV_FORM_DIRECT_BF16 = 4u };

// OIHW weights `w` [Cout][Cin][K][K] (+ BatchNorm `bn`, "" = none; + `bias` [Cout], null = none) -> the layer's device blobs;
// cout_pad > Cout appends zero output channels
int make_conv_layer(std::vector<void*>& allocs, const StateMap& sm, const char* who, const float* w, const std::string& bn, const float* bias,
                    int cout_pad, int Cin, int Cin_p, int Cout, int K, int stride, int pad, unsigned forms, ConvLayer* L);

// y = epilogue(conv(x)) on the fastest kernel the layer has a blob for: Winograd, else the exact-piece direct kernel, else fp32 MFMA
int run_conv_layer(const ConvLayer& L, const float* x, int N, int H, int W, int in_border, float* y, int out_border, const float* res, int relu,
                   hipStream_t s, float* splitk_ws, size_t splitk_ws_floats, float* y_act = nullptr, const float* act_scale = nullptr,
                   const float* act_shift = nullptr, bool x_f16 = false);

}  // namespace mp
