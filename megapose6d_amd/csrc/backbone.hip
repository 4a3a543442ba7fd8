// backbone.hip -- native executor for the CNN backbones + heads (host-side C++; kernels live in conv.hip / pool_fc.hip).
//
// Reference graph: src/megapose/models/torchvision_resnet.py:181-316 (vanilla_resnet34 = torchvision ResNet-34 with
// n_input_channels and fc 512->512), src/megapose/models/wide_resnet.py:29-126 (pre-activation WideResNet18/34),
// heads src/megapose/models/pose_rigid.py:122-130, selection src/megapose/training/pose_models_cfg.py:90-138.
// Weights arrive as the reference checkpoint's state_dict (SURVEY.md App. F key layout); eval-mode BatchNorm is folded
// into the preceding conv at load time (w' = w * g/sqrt(var+eps), b' = beta - mean * g/sqrt(var+eps)); the WideResNet
// block-input BN (bn1) cannot fold and is emitted by the PRODUCER's epilogue as a second "activated" output.
#include <cmath>
#include <cstdlib>
#include <map>
#include <mutex>
#include <string>
#include <vector>

#include "conv_layer.h"

namespace mp {

struct BnAct {  // unfoldable pre-activation BN: relu(x*scale + shift)
  float* d_scale = nullptr;
  float* d_shift = nullptr;
};

struct Block {
  ConvLayer conv1, conv2, down;
  bool has_down = false;
  BnAct pre;   // WideResNet: bn1 of THIS block (applied by the producer of its input)
};

}  // namespace mp

using namespace mp;

struct mp_backbone {
  int kind, c_in, c_in_p, in_border, head_kind, n_out, n_feat;
  int width = 1;      // WideResNet width multiplier (`resnet34_width=N`, training/pose_models_cfg.py:114-116): stage widths 64N .. 512N
  int stageC[4] = {64, 128, 256, 512};
  bool wide;
  bool direct_bf16 = true;   // MP_CONV_DIRECT_BF16 when the backbone was created: 0 = the non-Winograd layers stay on the fp32-MFMA kernel
  bool stem_tail = true;     // MP_STEM_TAIL when the backbone was created: 0 = the stem keeps the walks without the tail plane (conv_stem.hip)
  ConvLayer stem;
  std::vector<Block> blocks;
  std::vector<int> stage_of_block;  // 0..3
  float *d_fc_w = nullptr, *d_fc_b = nullptr, *d_head_w = nullptr, *d_head_b = nullptr;
  std::vector<void*> allocs;
  // exact-piece bf16 stem (conv_stem.hip): the stem's OIHW weights + folded BN scale stay on the host so that the piece blob can be
  // packed for the record layout (number of fp32-kind channels) the caller's rasteriser launch writes
  std::vector<float> stem_w_host, stem_scale_host;
  std::mutex blob_mu;                     // guards the two maps below: prepare (one thread) vs forwards looking blobs up on other threads / streams
  std::map<uint32_t, void*> stem_blobs;   // f32-kind channel mask -> device blob (mp_backbone_xrec_prepare); never freed before destroy
  std::map<uint32_t, void*> stem_blobs_sparse;   // ... -> blob of the background-tile walk (leading-channel masks with something to skip)
  std::map<uint32_t, int> stem_tail_forms;       // ... -> which of the two blobs is packed for a tail-plane walk (mp_conv_stem_tail_forms bits)
  // workspace bookkeeping: borders are zeroed once per (pointer, batch, h, w); several workspaces may be live at once
  // (one per HIP stream when half-batches are interleaved on two streams)
  struct WsKey { void* ptr; int batch, h, w; bool stem_written; };   // stem_written: the last forward there wrote S (not the fused-pool record path)
  std::vector<WsKey> ws_known;
};

namespace {

const char* const WHO = "mp_backbone_create";

int make_conv(mp_backbone* bb, const StateMap& sm, const std::string& wkey, const std::string& bnkey /* "" = none */, int Cin,
              int Cin_p, int Cout, int K, int stride, int pad, ConvLayer* L) {
  const float* w = find(sm, wkey, (int64_t)Cout * Cin * K * K, WHO);
  if (!w) return MP_ERR_INVALID;
  // 3x3 / stride-1 layers of the residual stages also get their Winograd F(2x2, 3x3) form.  MP_CONV_WINO: 2 (default) = the bf16x9
  // exact-piece kernel, 1 = the fp32-MFMA kernel, 0 = keep the direct kernel
  static const int wino_mode = getenv("MP_CONV_WINO") ? atoi(getenv("MP_CONV_WINO")) : 2;
  unsigned forms = wino_mode == 0 ? 0u : wino_mode == 1 ? CONV_FORM_WINO_F32 : CONV_FORM_WINO_BF16;
  if (L == &bb->stem) {   // the stem's exact-piece form is packed per record layout (mp_backbone_xrec_prepare) from the host copies
    bb->stem_w_host.assign(w, w + (size_t)Cout * Cin * K * K);
    std::vector<float> shift;
    if (!bnkey.empty() && bn_affine(sm, bnkey, Cout, WHO, bb->stem_scale_host, shift)) return MP_ERR_INVALID;
  } else if (bb->direct_bf16) {
    // the other 3x3 / 1x1 layers of the residual stages (stride 2: layer{2,3,4}.0.conv1 / .downsample) also get the exact-piece direct form
    forms |= CONV_FORM_DIRECT_BF16;
  }
  return make_conv_layer(bb->allocs, sm, WHO, w, bnkey, nullptr, 0, Cin, Cin_p, Cout, K, stride, pad, forms, L);
}

int make_bnact(mp_backbone* bb, const StateMap& sm, const std::string& bnkey, int C, BnAct* a) {
  std::vector<float> scale, shift;
  int rc = bn_affine(sm, bnkey, C, WHO, scale, shift);
  if (rc) return rc;
  rc = upload(bb->allocs, scale, &a->d_scale);
  if (rc) return rc;
  return upload(bb->allocs, shift, &a->d_shift);
}

constexpr size_t SPLITK_WS_FLOATS = 12u << 20;  // 48 MB of split-K scratch at the end of the workspace (>= 512 tiles of 128 x 128)

inline size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }
// (+ one padded row + one pixel of slack: the Winograd kernel reads -- and discards -- that much past an odd-sized tensor)
inline size_t buf_floats(int N, int H, int W, int C) { return (size_t)N * (H + 2) * (W + 2) * C + (size_t)(W + 3) * C + 64; }

struct Geometry {
  int h1, w1;       // stem output
  int hs[4], ws[4]; // stage resolutions
};

Geometry geometry(const mp_backbone* bb, int h, int w) {
  Geometry g;
  g.h1 = (h + 2 * bb->stem.pad - bb->stem.K) / 2 + 1;
  g.w1 = (w + 2 * bb->stem.pad - bb->stem.K) / 2 + 1;
  g.hs[0] = (g.h1 + 2 - 3) / 2 + 1;
  g.ws[0] = (g.w1 + 2 - 3) / 2 + 1;
  for (int s = 1; s < 4; ++s) {
    g.hs[s] = (g.hs[s - 1] + 2 - 3) / 2 + 1;
    g.ws[s] = (g.ws[s - 1] + 2 - 3) / 2 + 1;
  }
  return g;
}

// The carve-up of a workspace: [stem out S][per stage: A, Aact (wide only), B, C][split-K scratch].  Offsets in floats from the base, so
// that the size (mp_backbone_workspace_bytes), the forward and the debug taps (mp_backbone_debug_tensor) read the same layout.
struct WsLayout {
  Geometry g;
  size_t S = 0, A[4], Aact[4], B[4], C[4], SK = 0;   // Aact: the pre-activation nets only (0 and unused on the vanilla net)
  size_t total = 0;                                  // floats, the split-K scratch included
};

WsLayout ws_layout(const mp_backbone* bb, int batch, int h, int w) {
  WsLayout L;
  L.g = geometry(bb, h, w);
  size_t p = align_up(buf_floats(batch, L.g.h1, L.g.w1, bb->stageC[0]), 64);
  for (int st = 0; st < 4; ++st) {
    const size_t n = align_up(buf_floats(batch, L.g.hs[st], L.g.ws[st], bb->stageC[st]), 64);
    L.A[st] = p; p += n;
    L.Aact[st] = 0;
    if (bb->wide) { L.Aact[st] = p; p += n; }
    L.B[st] = p; p += n;
    L.C[st] = p; p += n;
  }
  L.SK = p;
  L.total = p + SPLITK_WS_FLOATS;
  return L;
}

}  // namespace

extern "C" int mp_backbone_create_wide(int kind, int width, int c_in, int head_kind, int n_head_out, const mp_named_tensor* st, int n_tensors,
                                       mp_backbone** out) {
  MP_REQUIRE(out && st && n_tensors > 0, "mp_backbone_create: bad arguments");
  MP_REQUIRE(kind >= 0 && kind <= 2, "mp_backbone_create: unknown backbone kind %d", kind);
  MP_REQUIRE(width >= 1 && width <= 8 && (width == 1 || kind != MP_BACKBONE_VANILLA_RESNET34),
             "mp_backbone_create: width multiplier %d (1..8, WideResNets only: training/pose_models_cfg.py:114-116)", width);
  MP_REQUIRE(c_in >= 1 && c_in <= 512, "mp_backbone_create: bad c_in %d", c_in);   // (sphere_26views: 3 + 27 * 6 = 165 input channels)
  StateMap sm;
  for (int i = 0; i < n_tensors; ++i) sm[st[i].name] = std::make_pair(st[i].h_data, st[i].numel);
  mp_backbone* bb = new mp_backbone();
  bb->kind = kind;
  bb->wide = kind != MP_BACKBONE_VANILLA_RESNET34;
  bb->direct_bf16 = !(getenv("MP_CONV_DIRECT_BF16") && atoi(getenv("MP_CONV_DIRECT_BF16")) == 0);   // read per backbone: one process can build both forms
  bb->stem_tail = !(getenv("MP_STEM_TAIL") && atoi(getenv("MP_STEM_TAIL")) == 0);                   // (the same: A/B in one build)
  bb->c_in = c_in;
  bb->c_in_p = (c_in + 3) / 4 * 4;
  bb->head_kind = head_kind;
  bb->n_out = n_head_out;
  bb->width = width;
  for (int k = 0; k < 4; ++k) bb->stageC[k] = bb->stageC[k] * width;
  const int C0 = bb->stageC[0], NF = bb->stageC[3];
  bb->n_feat = NF;
  int rc;
#define MP_TRY(e) do { rc = (e); if (rc) { mp_backbone_destroy(bb); return rc; } } while (0)
  const std::string B = "backbone.";
  if (!bb->wide) {
    bb->in_border = 3;
    MP_TRY(make_conv(bb, sm, B + "conv1.weight", B + "bn1", c_in, bb->c_in_p, C0, 7, 2, 3, &bb->stem));
  } else {
    bb->in_border = 2;
    MP_TRY(make_conv(bb, sm, B + "conv1.weight", B + "bn1", c_in, bb->c_in_p, C0, 5, 2, 2, &bb->stem));
  }
  static const int n34[4] = {3, 4, 6, 3}, n18[4] = {2, 2, 2, 2};
  const int* nblocks = (kind == MP_BACKBONE_WIDE_RESNET18) ? n18 : n34;
  int inplanes = C0;
  for (int s = 0; s < 4; ++s) {
    const int planes = bb->stageC[s];
    for (int i = 0; i < nblocks[s]; ++i) {
      Block blk;
      const int stride = (i == 0 && s > 0) ? 2 : 1;
      const std::string P = B + "layer" + std::to_string(s + 1) + "." + std::to_string(i) + ".";
      blk.has_down = (i == 0) && (stride != 1 || inplanes != planes);
      if (!bb->wide) {
        MP_TRY(make_conv(bb, sm, P + "conv1.weight", P + "bn1", inplanes, inplanes, planes, 3, stride, 1, &blk.conv1));
        MP_TRY(make_conv(bb, sm, P + "conv2.weight", P + "bn2", planes, planes, planes, 3, 1, 1, &blk.conv2));
        if (blk.has_down)
          MP_TRY(make_conv(bb, sm, P + "downsample.0.weight", P + "downsample.1", inplanes, inplanes, planes, 1, stride, 0, &blk.down));
      } else {
        // out = conv2(relu(bn2(conv1(a)))) + residual,  a = relu(bn1(x))   (wide_resnet.py:50-56)
        MP_TRY(make_bnact(bb, sm, P + "bn1", inplanes, &blk.pre));
        MP_TRY(make_conv(bb, sm, P + "conv1.weight", P + "bn2", inplanes, inplanes, planes, 3, stride, 1, &blk.conv1));
        MP_TRY(make_conv(bb, sm, P + "conv2.weight", "", planes, planes, planes, 3, 1, 1, &blk.conv2));
        if (blk.has_down) MP_TRY(make_conv(bb, sm, P + "downsample.weight", "", inplanes, inplanes, planes, 1, stride, 0, &blk.down));
      }
      bb->blocks.push_back(blk);
      bb->stage_of_block.push_back(s);
      inplanes = planes;
    }
  }
  if (!bb->wide) {
    const float* fw = find(sm, B + "fc.weight", 512 * 512, WHO);
    const float* fb = find(sm, B + "fc.bias", 512, WHO);
    if (!fw || !fb) { mp_backbone_destroy(bb); return MP_ERR_INVALID; }
    MP_TRY(upload(bb->allocs, std::vector<float>(fw, fw + 512 * 512), &bb->d_fc_w));
    MP_TRY(upload(bb->allocs, std::vector<float>(fb, fb + 512), &bb->d_fc_b));
  }
  const std::string H = head_kind == 0 ? "pose_fc" : "views_logits_head";
  const float* hw = find(sm, H + ".weight", (int64_t)n_head_out * NF, WHO);
  const float* hb = find(sm, H + ".bias", n_head_out, WHO);
  if (!hw || !hb) { mp_backbone_destroy(bb); return MP_ERR_INVALID; }
  MP_TRY(upload(bb->allocs, std::vector<float>(hw, hw + (size_t)n_head_out * NF), &bb->d_head_w));
  MP_TRY(upload(bb->allocs, std::vector<float>(hb, hb + n_head_out), &bb->d_head_b));
#undef MP_TRY
  *out = bb;
  return MP_OK;
}

extern "C" int mp_backbone_destroy(mp_backbone* bb) {
  if (!bb) return MP_OK;
  for (void* p : bb->allocs) (void)hipFree(p);
  delete bb;
  return MP_OK;
}

extern "C" int mp_backbone_input_channels_padded(const mp_backbone* bb) { return bb ? bb->c_in_p : 0; }
extern "C" int mp_backbone_input_border(const mp_backbone* bb) { return bb ? bb->in_border : 0; }

// workspace layout: [stem out][per stage: A, A_act (wide only), B, C]
extern "C" size_t mp_backbone_workspace_bytes(const mp_backbone* bb, int batch, int h, int w) {
  if (!bb || batch <= 0) return 0;
  return ws_layout(bb, batch, h, w).total * sizeof(float);
}

extern "C" int mp_backbone_workspace_reset(mp_backbone* bb, const void* d_ws) {
  MP_REQUIRE(bb, "mp_backbone_workspace_reset: null handle");
  for (size_t i = 0; i < bb->ws_known.size();)
    if (bb->ws_known[i].ptr == d_ws) bb->ws_known.erase(bb->ws_known.begin() + i); else ++i;
  return MP_OK;
}

// The piece blob of the stem for records whose fp32-kind channels are the set bits of `f32_mask` (packed and uploaded on the first call
// for a mask: host work + a synchronous copy, so this is the explicit PREPARE step -- once, outside stream capture, from one thread; the
// forward only looks the blob up); returns the record length in bf16 elements, 0 if this backbone's stem has no exact-piece form.
extern "C" int mp_backbone_xrec_prepare(mp_backbone* bb, uint32_t f32_mask) {
  if (!bb || bb->stem_w_host.empty() || bb->c_in > 32) return 0;
  if (bb->c_in < 32 && (f32_mask >> bb->c_in) != 0u) return 0;
  const int n_f32 = __builtin_popcount(f32_mask), n_u8 = bb->c_in - n_f32;
  if (!mp_conv_stem_supported(bb->stem.K, n_f32, n_u8) || bb->stem.Cout % 64 != 0) return 0;
  std::lock_guard<std::mutex> blob_lock(bb->blob_mu);
  if (!bb->stem_blobs.count(f32_mask)) {
    const bool leading = f32_mask == (n_f32 >= 32 ? 0xFFFFFFFFu : (1u << n_f32) - 1u);
    // tail-plane walks where the record has them (the background one for leading-channel masks only, like the background walk itself)
    int forms = bb->stem_tail ? mp_conv_stem_tail_forms(bb->stem.K, n_f32, n_u8) & (leading ? 3 : 1) : 0;
    const float* h_scale = bb->stem_scale_host.empty() ? nullptr : bb->stem_scale_host.data();
    std::vector<unsigned char> blob((forms & 1) ? mp_conv_stem_tail_packed_bytes(bb->stem.K, n_f32, n_u8, bb->stem.Cout, 0)
                                                : mp_conv_stem_packed_bytes(bb->stem.K, n_f32, n_u8, bb->stem.Cout));
    if (((forms & 1) ? mp_conv_stem_pack_weights_tail(bb->stem_w_host.data(), bb->stem.Cout, bb->c_in, bb->stem.K, f32_mask, 0, h_scale, blob.data())
                     : mp_conv_stem_pack_weights_mask(bb->stem_w_host.data(), bb->stem.Cout, bb->c_in, bb->stem.K, f32_mask, h_scale, blob.data())) != MP_OK)
      return 0;
    void* d = nullptr;
    if (hipMalloc(&d, blob.size()) != hipSuccess) return 0;
    if (hipMemcpy(d, blob.data(), blob.size(), hipMemcpyHostToDevice) != hipSuccess) { (void)hipFree(d); return 0; }
    bb->allocs.push_back(d);
    bb->stem_blobs[f32_mask] = d;
    // the background-tile walk: only for leading-channel masks (no depth channels) with fewer fp32-kind chunks than the record has
    // (in its tail-plane form the coarse net's 16-element record has one too)
    bool have_sparse = false;
    if (leading && ((forms & 2) || mp_conv_stem_sparse_chunks(bb->stem.K, n_f32, n_u8) > 0)) {
      std::vector<unsigned char> sb((forms & 2) ? mp_conv_stem_tail_packed_bytes(bb->stem.K, n_f32, n_u8, bb->stem.Cout, 1)
                                                : mp_conv_stem_sparse_packed_bytes(bb->stem.K, n_f32, n_u8, bb->stem.Cout));
      void* ds = nullptr;
      if (((forms & 2) ? mp_conv_stem_pack_weights_tail(bb->stem_w_host.data(), bb->stem.Cout, bb->c_in, bb->stem.K, f32_mask, 1, h_scale, sb.data())
                       : mp_conv_stem_pack_weights_sparse(bb->stem_w_host.data(), bb->stem.Cout, bb->c_in, bb->stem.K, n_f32, h_scale, sb.data())) == MP_OK &&
          hipMalloc(&ds, sb.size()) == hipSuccess) {
        if (hipMemcpy(ds, sb.data(), sb.size(), hipMemcpyHostToDevice) == hipSuccess) {
          bb->allocs.push_back(ds);
          bb->stem_blobs_sparse[f32_mask] = ds;
          have_sparse = true;
        } else {
          (void)hipFree(ds);
        }
      }
    }
    if (!have_sparse) forms &= 1;
    bb->stem_tail_forms[f32_mask] = forms;
  }
  return mp_xrec_elements(n_f32, n_u8);
}

// x_mode: 0 = fp32 padded NHWC, 1 = binary16 elements (MP_RASTER_F16), 2 = bf16 stem records whose fp32-kind channels are f32_mask (MP_RASTER_XREC)
static int backbone_forward_impl(mp_backbone* bb, const float* d_x, int x_mode, uint32_t f32_mask, int batch, int h, int w, float* d_out, float* d_sigmoid,
                                 float* d_feat, void* d_ws, size_t ws_bytes, mp_stream stream, const unsigned char* d_tile_flags = nullptr) {
  const bool x_f16 = x_mode == 1;
  MP_REQUIRE(bb && d_x && d_out && d_ws, "mp_backbone_forward: null pointer");
  if (batch == 0) return MP_OK;
  const WsLayout lay = ws_layout(bb, batch, h, w);
  const size_t need = lay.total * sizeof(float);
  MP_REQUIRE(ws_bytes >= need, "mp_backbone_forward: workspace %zu < %zu bytes", ws_bytes, need);
  hipStream_t s = (hipStream_t)stream;
  const Geometry& g = lay.g;
  bool known = false;
  for (const auto& k : bb->ws_known) known = known || (k.ptr == d_ws && k.batch == batch && k.h == h && k.w == w);
  if (!known) {
    MP_CHECK_HIP(hipMemsetAsync(d_ws, 0, need, s));  // zero borders once; interiors are always overwritten
    for (size_t i = 0; i < bb->ws_known.size();)     // a pointer re-used with another geometry invalidates its old entry
      if (bb->ws_known[i].ptr == d_ws) bb->ws_known.erase(bb->ws_known.begin() + i); else ++i;
    if (bb->ws_known.size() >= 8) bb->ws_known.erase(bb->ws_known.begin());
    bb->ws_known.push_back({d_ws, batch, h, w, false});
  }
  float* const base = (float*)d_ws;
  float* S = base + lay.S;
  float *A[4], *Aact[4], *Bf[4], *Cf[4];
  for (int st = 0; st < 4; ++st) {
    A[st] = base + lay.A[st];
    Aact[st] = bb->wide ? base + lay.Aact[st] : nullptr;
    Bf[st] = base + lay.B[st];
    Cf[st] = base + lay.C[st];
  }
  float* SK = base + lay.SK;  // split-K scratch (SPLITK_WS_FLOATS)
  int rc;
  bool stem_pooled = false;
  // stem: conv + folded bn + relu, then 3x3/s2 max pool (+ first block's pre-activation for the wide nets)
  if (x_mode == 2) {
    const void* d_stem_pieces = nullptr;
    const void* d_sparse_blob = nullptr;
    int tail_forms = 0;
    {
      std::lock_guard<std::mutex> blob_lock(bb->blob_mu);
      const auto blob_it = bb->stem_blobs.find(f32_mask);
      if (blob_it != bb->stem_blobs.end()) d_stem_pieces = blob_it->second;
      const auto sp_it = bb->stem_blobs_sparse.find(f32_mask);
      if (sp_it != bb->stem_blobs_sparse.end()) d_sparse_blob = sp_it->second;
      const auto tf_it = bb->stem_tail_forms.find(f32_mask);
      if (tf_it != bb->stem_tail_forms.end()) tail_forms = tf_it->second;
    }
    MP_REQUIRE(d_stem_pieces != nullptr, "mp_backbone_forward_xrec: no piece blob for the fp32-kind channel mask 0x%x of this %d-channel stem: "
               "call mp_backbone_xrec_prepare first (it returns 0 if the stem has no exact-piece form)", f32_mask, bb->c_in);
    const int n_f32 = __builtin_popcount(f32_mask);
    mp_conv_desc d;
    memset(&d, 0, sizeof(d));
    d.d_x = d_x; d.N = batch; d.H = h; d.W = w; d.C = bb->stem.Cin_p; d.c_real = bb->c_in; d.in_border = bb->in_border;
    d.d_bias = bb->stem.d_b; d.Cout = bb->stem.Cout; d.KH = bb->stem.K; d.KW = bb->stem.K; d.stride = 2; d.pad = bb->stem.pad;
    d.d_y = S; d.out_border = 1; d.relu = 1;
    // the max pool rides in the stem's epilogue and the stem map is never written (MP_STEM_POOL=0: separate kernels)
    static const bool fuse_pool = !(getenv("MP_STEM_POOL") && atoi(getenv("MP_STEM_POOL")) == 0);
    const void* d_sparse = d_tile_flags ? d_sparse_blob : nullptr;   // background-tile walk where it applies
    if (fuse_pool) {
      d.d_y = nullptr;
      rc = tail_forms ? mp_conv_stem_xrec_tail(&d, d_stem_pieces, d_sparse, n_f32, d_sparse ? d_tile_flags : nullptr, A[0], 1, tail_forms, s)
           : d_sparse ? mp_conv_stem_xrec_sparse(&d, d_stem_pieces, d_sparse, n_f32, d_tile_flags, A[0], 1, s)
                      : mp_conv_stem_xrec_pool(&d, d_stem_pieces, n_f32, A[0], 1, s);
      // pre-activation WideResNets (round 6): relu(bn1(pooled)) by a small elementwise pass over the pooled map (the fused pool completes
      // straddling windows with atomics, so the stem itself cannot emit it) instead of the separate pool kernel's pass over the 4x larger stem map
      if (!rc && bb->wide) rc = mp_bn_relu_nhwc(A[0], batch, g.hs[0], g.ws[0], bb->stageC[0], 1, Aact[0], bb->blocks[0].pre.d_scale, bb->blocks[0].pre.d_shift, s);
      stem_pooled = true;
    } else {
      rc = tail_forms ? mp_conv_stem_xrec_tail(&d, d_stem_pieces, d_sparse, n_f32, d_sparse ? d_tile_flags : nullptr, nullptr, 0, tail_forms, s)
           : d_sparse ? mp_conv_stem_xrec_sparse(&d, d_stem_pieces, d_sparse, n_f32, d_tile_flags, nullptr, 0, s)
                      : mp_conv_stem_xrec(&d, d_stem_pieces, n_f32, s);
    }
  } else {
    rc = run_conv_layer(bb->stem, d_x, batch, h, w, bb->in_border, S, 1, nullptr, 1, s, SK, SPLITK_WS_FLOATS, nullptr, nullptr, nullptr, x_f16);
  }
  if (rc) return rc;
  for (auto& k : bb->ws_known)
    if (k.ptr == d_ws && k.batch == batch && k.h == h && k.w == w) k.stem_written = !stem_pooled;
  const Block& b0 = bb->blocks[0];
  if (!stem_pooled) {
    rc = mp_maxpool3x3s2(S, batch, g.h1, g.w1, bb->stageC[0], 1, A[0], 1, bb->wide ? Aact[0] : nullptr, bb->wide ? b0.pre.d_scale : nullptr,
                         bb->wide ? b0.pre.d_shift : nullptr, s);
    if (rc) return rc;
  }
  const int nb = (int)bb->blocks.size();
  for (int i = 0; i < nb; ++i) {
    const Block& blk = bb->blocks[i];
    const int so = bb->stage_of_block[i];                 // output stage
    const int si = (blk.has_down && so > 0) ? so - 1 : so;  // input stage
    const int Hi = g.hs[si], Wi = g.ws[si];
    const bool last = (i + 1 == nb);
    if (!bb->wide) {
      // y1 = relu(bn1(conv1(x))); idn = bn(down(x)) | x; out = relu(bn2(conv2(y1)) + idn)
      rc = run_conv_layer(blk.conv1, A[si], batch, Hi, Wi, 1, Bf[so], 1, nullptr, 1, s, SK, SPLITK_WS_FLOATS);
      if (rc) return rc;
      const float* idn = A[si];
      if (blk.has_down) {
        rc = run_conv_layer(blk.down, A[si], batch, Hi, Wi, 1, Cf[so], 1, nullptr, 0, s, SK, SPLITK_WS_FLOATS);
        if (rc) return rc;
        idn = Cf[so];
      }
      rc = run_conv_layer(blk.conv2, Bf[so], batch, g.hs[so], g.ws[so], 1, A[so], 1, idn, 1, s, SK, SPLITK_WS_FLOATS);
      if (rc) return rc;
    } else {
      // a = relu(bn1(x)) was produced upstream into Aact[si]; residual = down(a) | x
      rc = run_conv_layer(blk.conv1, Aact[si], batch, Hi, Wi, 1, Bf[so], 1, nullptr, 1, s, SK, SPLITK_WS_FLOATS);
      if (rc) return rc;
      const float* idn = A[si];
      if (blk.has_down) {
        rc = run_conv_layer(blk.down, Aact[si], batch, Hi, Wi, 1, Cf[so], 1, nullptr, 0, s, SK, SPLITK_WS_FLOATS);
        if (rc) return rc;
        idn = Cf[so];
      }
      const BnAct next_pre = last ? BnAct() : bb->blocks[i + 1].pre;
      rc = run_conv_layer(blk.conv2, Bf[so], batch, g.hs[so], g.ws[so], 1, A[so], 1, idn, 0, s, SK, SPLITK_WS_FLOATS, last ? nullptr : Aact[so],
                          next_pre.d_scale, next_pre.d_shift);
      if (rc) return rc;
    }
  }
  return mp_pool_fc_heads(A[3], batch, g.hs[3], g.ws[3], bb->stageC[3], 1, bb->d_fc_w, bb->d_fc_b, bb->n_feat, bb->d_head_w, bb->d_head_b, bb->n_out,
                          d_feat, d_out, d_sigmoid, s);
}

extern "C" int mp_backbone_forward(mp_backbone* bb, const float* d_x, int batch, int h, int w, float* d_out, float* d_sigmoid,
                                   float* d_feat, void* d_ws, size_t ws_bytes, mp_stream stream) {
  return backbone_forward_impl(bb, d_x, 0, 0, batch, h, w, d_out, d_sigmoid, d_feat, d_ws, ws_bytes, stream);
}

extern "C" int mp_backbone_forward_xrec_mask(mp_backbone* bb, const void* d_xrec, uint32_t f32_mask, int batch, int h, int w, float* d_out,
                                             float* d_sigmoid, float* d_feat, void* d_ws, size_t ws_bytes, mp_stream stream) {
  return backbone_forward_impl(bb, (const float*)d_xrec, 2, f32_mask, batch, h, w, d_out, d_sigmoid, d_feat, d_ws, ws_bytes, stream);
}

extern "C" int mp_backbone_forward_xrec_sparse(mp_backbone* bb, const void* d_xrec, uint32_t f32_mask, const unsigned char* d_tile_flags, int batch,
                                               int h, int w, float* d_out, float* d_sigmoid, float* d_feat, void* d_ws, size_t ws_bytes,
                                               mp_stream stream) {
  return backbone_forward_impl(bb, (const float*)d_xrec, 2, f32_mask, batch, h, w, d_out, d_sigmoid, d_feat, d_ws, ws_bytes, stream, d_tile_flags);
}

extern "C" int mp_backbone_forward_f16(mp_backbone* bb, const void* d_x_half, int batch, int h, int w, float* d_out, float* d_sigmoid,
                                       float* d_feat, void* d_ws, size_t ws_bytes, mp_stream stream) {
  return backbone_forward_impl(bb, (const float*)d_x_half, 1, 0, batch, h, w, d_out, d_sigmoid, d_feat, d_ws, ws_bytes, stream);
}

// Parity taps (tests): where an intermediate that survives a forward lies in the workspace.  Nothing on the forward path reads this.
extern "C" int mp_backbone_debug_tensor(const mp_backbone* bb, const char* what, const void* d_ws, int batch, int h, int w, const void** d_ptr,
                                        int64_t shape4[4], int32_t* border) {
  MP_REQUIRE(bb && what && d_ws && d_ptr && shape4 && border, "mp_backbone_debug_tensor: null pointer");
  MP_REQUIRE(batch > 0, "mp_backbone_debug_tensor: batch %d", batch);
  const mp_backbone::WsKey* key = nullptr;
  for (const auto& k : bb->ws_known)
    if (k.ptr == d_ws && k.batch == batch && k.h == h && k.w == w) key = &k;
  MP_REQUIRE(key, "mp_backbone_debug_tensor: the last forward on this workspace was not one of %d x %d x %d (or none has run)", batch, h, w);
  const WsLayout lay = ws_layout(bb, batch, h, w);
  const std::string name(what);
  size_t off = 0;
  int H = 0, W = 0, C = 0;
  bool found = false;
  if (name == "stem") {
    MP_REQUIRE(key->stem_written, "mp_backbone_debug_tensor: 'stem' was not written: the record path pools inside the stem kernel "
               "(the fp32 and f16 tensor paths write it)");
    off = lay.S; H = lay.g.h1; W = lay.g.w1; C = bb->stageC[0];
    found = true;
  } else if (name.size() >= 6 && name.compare(0, 5, "layer") == 0 && name[5] >= '1' && name[5] <= '4') {
    const int st = name[5] - '1';
    const std::string rest = name.substr(6);
    H = lay.g.hs[st]; W = lay.g.ws[st]; C = bb->stageC[st];
    if (rest.empty()) {
      off = lay.A[st];
      found = true;
    } else if (rest == "_act") {
      MP_REQUIRE(bb->wide && st < 3, "mp_backbone_debug_tensor: '%s' does not apply: only the pre-activation nets write a second output, "
                 "and only stages 1..3 have a next block", what);
      off = lay.Aact[st];
      found = true;
    } else if (rest == "_down") {
      MP_REQUIRE(st > 0, "mp_backbone_debug_tensor: '%s' does not apply: stage 1 has no downsample", what);
      off = lay.C[st];
      found = true;
    }
  }
  MP_REQUIRE(found, "mp_backbone_debug_tensor: '%s' is not a published tensor (stem, layer1..4, layer1..3_act, layer2..4_down)", what);
  *d_ptr = (const float*)d_ws + off;
  shape4[0] = batch; shape4[1] = H; shape4[2] = W; shape4[3] = C;
  *border = 1;
  return MP_OK;
}

extern "C" double mp_backbone_flops(const mp_backbone* bb, int batch, int h, int w) {
  if (!bb) return 0.0;
  const Geometry g = geometry(bb, h, w);
  auto conv_flops = [](const ConvLayer& L, int Ho, int Wo) { return 2.0 * L.Cout * L.Cin * L.K * L.K * (double)Ho * Wo; };
  double f = conv_flops(bb->stem, g.h1, g.w1);
  for (size_t i = 0; i < bb->blocks.size(); ++i) {
    const Block& blk = bb->blocks[i];
    const int so = bb->stage_of_block[i];
    f += conv_flops(blk.conv1, g.hs[so], g.ws[so]) + conv_flops(blk.conv2, g.hs[so], g.ws[so]);
    if (blk.has_down) f += conv_flops(blk.down, g.hs[so], g.ws[so]);
  }
  if (!bb->wide) f += 2.0 * 512 * 512;
  f += 2.0 * bb->n_feat * bb->n_out;
  return f * batch;
}
