// conv_layer.hip -- the convolution layer both network executors are built from (host-side C++; the kernels live in conv.hip,
// conv_bf16x9.hip, conv_wino.hip and conv_wino_bf16.hip): load-time fold + packing, run-time kernel choice.
#include <algorithm>
#include <cmath>

#include "conv_layer.h"

namespace mp {

const float* find(const StateMap& sm, const std::string& key, int64_t numel, const char* who) {
  auto it = sm.find(key);
  if (it == sm.end()) {
    set_error("%s: missing state_dict key '%s'", who, key.c_str());
    return nullptr;
  }
  if (it->second.second != numel) {
    set_error("%s: key '%s' has %ld elements, expected %ld", who, key.c_str(), (long)it->second.second, (long)numel);
    return nullptr;
  }
  return it->second.first;
}

int bn_affine(const StateMap& sm, const std::string& prefix, int C, const char* who, std::vector<float>& scale, std::vector<float>& shift) {
  const float* g = find(sm, prefix + ".weight", C, who);
  const float* b = find(sm, prefix + ".bias", C, who);
  const float* m = find(sm, prefix + ".running_mean", C, who);
  const float* v = find(sm, prefix + ".running_var", C, who);
  if (!g || !b || !m || !v) return MP_ERR_INVALID;
  scale.resize(C);
  shift.resize(C);
  for (int c = 0; c < C; ++c) {
    const float s = g[c] / sqrtf(v[c] + 1e-5f);
    scale[c] = s;
    shift[c] = b[c] - m[c] * s;
  }
  return MP_OK;
}

int upload(std::vector<void*>& allocs, const std::vector<float>& h, float** d) {
  MP_CHECK_HIP(hipMalloc(d, h.size() * sizeof(float)));
  MP_CHECK_HIP(hipMemcpy(*d, h.data(), h.size() * sizeof(float), hipMemcpyHostToDevice));
  allocs.push_back(*d);
  return MP_OK;
}

int make_conv_layer(std::vector<void*>& allocs, const StateMap& sm, const char* who, const float* w, const std::string& bn, const float* bias,
                    int cout_pad, int Cin, int Cin_p, int Cout, int K, int stride, int pad, unsigned forms, ConvLayer* L) {
  const int Co = std::max(Cout, cout_pad);
  L->Cin = Cin; L->Cin_p = Cin_p; L->Cout = Co; L->K = K; L->stride = stride; L->pad = pad;
  std::vector<float> scale, shift;
  if (!bn.empty()) {
    int rc = bn_affine(sm, bn, Cout, who, scale, shift);
    if (rc) return rc;
    scale.resize(Co, 0.f);
  }
  shift.resize(Co, 0.f);
  if (bias)
    for (int c = 0; c < Cout; ++c) shift[c] += bias[c];
  std::vector<float> w_padded;
  if (Co > Cout) {
    w_padded.assign(w, w + (size_t)Cout * Cin * K * K);
    w_padded.resize((size_t)Co * Cin * K * K, 0.f);
    w = w_padded.data();
  }
  const float* sc = scale.empty() ? nullptr : scale.data();
  std::vector<float> packed(mp_conv_packed_floats(Cin_p, Co, K, K));
  int rc = mp_conv_pack_weights(w, Co, Cin, K, K, Cin_p, sc, packed.data());
  if (rc) return rc;
  rc = upload(allocs, packed, &L->d_w);
  // 3x3 / stride-1 layers in their Winograd F(2x2, 3x3) form: the fp32-MFMA kernel's blob or the bf16x9 exact-piece kernel's
  if (!rc && (forms & (CONV_FORM_WINO_F32 | CONV_FORM_WINO_BF16)) && K == 3 && stride == 1 && pad == 1 && Cin_p % 16 == 0 && Co % 64 == 0) {
    if (forms & CONV_FORM_WINO_F32) {
      std::vector<float> u(mp_conv_wino_packed_floats(Cin_p, Co));
      rc = mp_conv_wino_pack_weights(w, Co, Cin, Cin_p, sc, u.data());
      if (!rc) rc = upload(allocs, u, &L->d_u);
    } else {
      std::vector<float> u((mp_conv_wino_bf16_packed_bytes(Cin_p, Co) + 3) / 4);
      rc = mp_conv_wino_bf16_pack_weights(w, Co, Cin, Cin_p, sc, u.data());
      float* d = nullptr;
      if (!rc) rc = upload(allocs, u, &d);
      L->d_ub = d;
    }
  }
  // the other 3x3 / 1x1 layers (stride 2, 1x1 downsample) in the exact-piece direct form
  if (!rc && (forms & CONV_FORM_DIRECT_BF16) && !L->d_u && !L->d_ub && (K == 1 || K == 3) && Cin_p % 16 == 0 && (K * Cin_p) % 32 == 0 &&
      Co % 64 == 0) {
    std::vector<float> wb((mp_conv_bf16x9_packed_bytes(Cin_p, Co, K, K) + 3) / 4);
    rc = mp_conv_bf16x9_pack_weights(w, Co, Cin, K, K, Cin_p, sc, wb.data());
    float* d = nullptr;
    if (!rc) rc = upload(allocs, wb, &d);
    L->d_wb = d;
  }
  if (rc) return rc;
  return (!bn.empty() || bias) ? upload(allocs, shift, &L->d_b) : MP_OK;
}

int run_conv_layer(const ConvLayer& L, const float* x, int N, int H, int W, int in_border, float* y, int out_border, const float* res, int relu,
                   hipStream_t s, float* splitk_ws, size_t splitk_ws_floats, float* y_act, const float* act_scale, const float* act_shift,
                   bool x_f16) {
  mp_conv_desc d;
  memset(&d, 0, sizeof(d));
  d.x_f16 = x_f16 ? 1 : 0;
  d.d_x = x; d.N = N; d.H = H; d.W = W; d.C = L.Cin_p; d.c_real = L.Cin; d.in_border = in_border;
  d.d_w = L.d_w; d.d_bias = L.d_b; d.Cout = L.Cout; d.KH = L.K; d.KW = L.K; d.stride = L.stride; d.pad = L.pad;
  d.d_y = y; d.out_border = out_border; d.d_residual = res; d.relu = relu;
  d.d_y_act = y_act;
  if (y_act) { d.d_act_scale = act_scale; d.d_act_shift = act_shift; }
  d.d_splitk_ws = splitk_ws;
  d.splitk_ws_floats = splitk_ws ? (int64_t)splitk_ws_floats : 0;
  if ((L.d_u || L.d_ub || L.d_wb) && !x_f16) {
    const int n_cu = device_cu_count();
    // the Winograd kernels take 128.5 KB of LDS per workgroup (gfx950: 160 KB per CU); a part with less keeps the direct kernel
    // (the executors' workspace buffers carry the read slack the Winograd kernels need)
    if ((L.d_u || L.d_ub) && device_lds_bytes() >= 132 * 1024 && mp_conv_wino_eligible(&d, n_cu))
      return L.d_ub ? mp_conv3x3_wino_bf16_nhwc(&d, L.d_ub, s) : mp_conv3x3_wino_nhwc(&d, L.d_u, s);
    // exact-piece direct kernel unless the fp32 kernel's plan splits every tile along K (small grids: mode 1).  A "whole rounds + split-K
    // tail" plan (mode 2) runs as ONE single-pass launch here: on the bf16 pipe its extra, partly filled round costs less than the split tail.
    if (L.d_wb) {
      int32_t plan[5] = {0, 1, 0, 0, 0};
      const int rc = mp_conv2d_plan(&d, n_cu, plan);
      if (rc) return rc;
      if (plan[0] != 1) return mp_conv2d_bf16x9_nhwc(&d, L.d_wb, s);
    }
  }
  return mp_conv2d_nhwc(&d, s);
}

}  // namespace mp
