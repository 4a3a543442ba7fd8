// detector.hip -- the 2D detector network (Mask R-CNN, ResNet-50 + FPN) as one native, device-resident inference graph.
//
// Replaces `self.model([image_n for image_n in images])` of the reference's Detector
//   (/root/reference/src/megapose/inference/detector.py:92; model = DetectorMaskRCNN, src/megapose/models/mask_rcnn.py:23-46 =
//    torchvision.models.detection.MaskRCNN(resnet_fpn_backbone("resnet50"), n_classes, AnchorGenerator(anchor_sizes, (0.5, 1, 2)),
//    min_size, max_size), created by training/detector_models_cfg.py:31-38).
// torchvision (0.12.0) is third-party code that is not under /root/reference; the inference algorithm restated here is the
// published one, file by file as listed at the top of oracle/mask_rcnn.py -- the independent CPU restatement this file is tested
// against ("parity unpinned" vs torchvision itself).
//
// Design (MI355X-first, not a port of torchvision's op-by-op graph):
//   * every feature map is padded NHWC fp32 in ONE caller-provided workspace; all 100+ convolutions (ResNet-50 bottlenecks with the
//     FrozenBatchNorm folded in, FPN, RPN head, mask head) and the box head's FC layers (as 1x1 convolutions over [R,1,1,12544]) run
//     on the library's fp32-MFMA implicit-GEMM kernel (conv.hip) with fused bias / residual / ReLU epilogues;
//   * the RPN's two 1x1 heads are one convolution (3 + 12 -> 16 channels), the predictor's two Linear layers one (C + 4C channels),
//     the mask predictor's 2x2 stride-2 transposed convolution is a 1x1 convolution onto 4 x 256 sub-pixel channels;
//   * selection (top-k, sort) is a stable rank sort on the device -- rank(i) = #{j: key_j > key_i or (key_j == key_i and j < i)} --,
//     NMS a sequential-greedy sweep with a parallel inner loop, one workgroup per (image, level | class) segment: deterministic,
//     no host round trip, no library sort;
//   * no synchronisation: detections come back as fixed-size [n, D] arrays + counts.
// None of this is on the pose hot path (one call per frame set); it is bounded by the ResNet-50 convolutions (MFMA).
#include <algorithm>
#include <cmath>
#include <string>
#include <vector>

#include "conv_layer.h"

namespace mp {

constexpr int DET_LEVELS = 5;       // P2..P6
constexpr int DET_A = 3;            // anchors per location
constexpr int DET_FPN_C = 256;
constexpr int DET_MAX_SEG = 1024;   // NMS segment capacity (LDS)
constexpr float DET_XFORM_CLIP = 4.135166556742356f;   // log(1000 / 16)

// ---------------------------------------------------------------------------------------------------------------------------------
// kernels
// ---------------------------------------------------------------------------------------------------------------------------------
// GeneralizedRCNNTransform: (x - mean) / std, bilinear resize (align_corners = False, scale = in / out), zero pad; NCHW -> padded NHWC4
__global__ __launch_bounds__(256) void det_preprocess_kernel(const float* __restrict__ img, int H, int W, int hr, int wr, float sy, float sx,
                                                             float m0, float m1, float m2, float s0, float s1, float s2,
                                                             float* __restrict__ out, int Hp, int Wp, int border) {
  const int n = blockIdx.y;
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= hr * wr) return;
  const int y = i / wr, x = i - y * wr;
  const float mean[3] = {m0, m1, m2}, sd[3] = {s0, s1, s2};
  float v[3];
  const float* base = img + (size_t)n * 3 * H * W;
  if (hr == H && wr == W) {
#pragma unroll
    for (int c = 0; c < 3; ++c) v[c] = (base[((size_t)c * H + y) * W + x] - mean[c]) / sd[c];
  } else {
    float fy = sy * ((float)y + 0.5f) - 0.5f, fx = sx * ((float)x + 0.5f) - 0.5f;
    fy = fy < 0.f ? 0.f : fy;
    fx = fx < 0.f ? 0.f : fx;
    const int y0 = (int)fy, x0 = (int)fx;
    const int y1 = y0 + (y0 < H - 1 ? 1 : 0), x1 = x0 + (x0 < W - 1 ? 1 : 0);
    const float ly = fy - (float)y0, lx = fx - (float)x0, hy = 1.f - ly, hx = 1.f - lx;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float* p = base + (size_t)c * H * W;
      const float a = (p[(size_t)y0 * W + x0] - mean[c]) / sd[c], b = (p[(size_t)y0 * W + x1] - mean[c]) / sd[c];
      const float cc = (p[(size_t)y1 * W + x0] - mean[c]) / sd[c], d = (p[(size_t)y1 * W + x1] - mean[c]) / sd[c];
      v[c] = hy * (hx * a + lx * b) + ly * (hx * cc + lx * d);
    }
  }
  const int Wq = Wp + 2 * border, Hq = Hp + 2 * border;
  *reinterpret_cast<float4*>(out + (((size_t)n * Hq + y + border) * Wq + x + border) * 4) = make_float4(v[0], v[1], v[2], 0.f);
}

// nearest-neighbour resize of a padded-NHWC map (FPN top-down path: F.interpolate(size=..., mode="nearest"))
__global__ __launch_bounds__(256) void det_resize_nearest_kernel(const float* __restrict__ src, int hs, int ws, float* __restrict__ dst, int hd,
                                                                 int wd, int C, int N, int sb, int db, int step_y, int step_x) {
  // step > 0: dst(y, x) = src(y * step, x * step) (LastLevelMaxPool = max_pool2d(kernel 1, stride 2)); step == 0: src index = floor(dst * in / out)
  const int c4n = C / 4;
  const long total = (long)N * hd * wd * c4n;
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= total) return;
  const int c4 = (int)(idx % c4n);
  long t = idx / c4n;
  const int x = (int)(t % wd);
  t /= wd;
  const int y = (int)(t % hd);
  const int n = (int)(t / hd);
  const int ys = step_y > 0 ? y * step_y : min((int)(((long)y * hs) / hd), hs - 1);
  const int xs = step_x > 0 ? x * step_x : min((int)(((long)x * ws) / wd), ws - 1);
  const float4 v = *reinterpret_cast<const float4*>(src + (((size_t)n * (hs + 2 * sb) + ys + sb) * (ws + 2 * sb) + xs + sb) * C + c4 * 4);
  *reinterpret_cast<float4*>(dst + (((size_t)n * (hd + 2 * db) + y + db) * (wd + 2 * db) + x + db) * C + c4 * 4) = v;
}

struct RpnLevels {
  const float* head[DET_LEVELS];   // [n, gh, gw, 16]: 3 objectness logits, 12 deltas (a * 4 + k), 1 pad
  int gh[DET_LEVELS], gw[DET_LEVELS], off[DET_LEVELS + 1];   // off: anchor offset of the level inside one image's key row
  int stride_y[DET_LEVELS], stride_x[DET_LEVELS];
  float base[DET_LEVELS][DET_A][4];   // base anchors (rounded), anchor_utils.py generate_anchors
};

// objectness logits of every anchor, (level, y, x, a) order = torchvision's concat_box_prediction_layers order
__global__ __launch_bounds__(256) void det_rpn_keys_kernel(RpnLevels L, int n_images, float* __restrict__ keys) {
  const int total = L.off[DET_LEVELS];
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (long)n_images * total) return;
  const int n = (int)(idx / total), i = (int)(idx % total);
  int l = 0;
#pragma unroll
  for (int k = 1; k < DET_LEVELS; ++k) l += i >= L.off[k];
  const int j = i - L.off[l], pix = j / DET_A, a = j - pix * DET_A;
  keys[idx] = L.head[l][((size_t)n * L.gh[l] * L.gw[l] + pix) * 16 + a];
}

// segment tables of the sorts, built on the device (no H2D copy whose source could die before the copy runs)
__global__ void det_rpn_seg_offsets_kernel(RpnLevels L, int n_images, int* __restrict__ out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  const int total = L.off[DET_LEVELS];
  if (i < n_images * DET_LEVELS) out[i] = (i / DET_LEVELS) * total + L.off[i % DET_LEVELS];
  if (i == n_images * DET_LEVELS) out[i] = n_images * total;
}
__global__ void det_seg_offsets_kernel(int n_seg, int stride, int* __restrict__ out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i <= n_seg) out[i] = i * stride;
}

// Stable rank sort: element i of a segment goes to position #{j: key_j > key_i or (key_j == key_i and j < i)}; only the first K
// positions are stored, -inf keys are "absent".  grid = (ceil(max_len / 256), n_segments).  out_cnt must be zero on entry.
__global__ __launch_bounds__(256) void det_rank_topk_kernel(const float* __restrict__ keys, const int* __restrict__ seg_off, int K,
                                                            int* __restrict__ out_idx, int* __restrict__ out_cnt) {
  __shared__ float tile[1024];
  const int seg = blockIdx.y;
  const int beg = seg_off[seg], len = seg_off[seg + 1] - beg;
  if ((int)(blockIdx.x * 256) >= len) return;   // whole workgroup beyond the segment (uniform)
  const int i = blockIdx.x * 256 + threadIdx.x;
  const bool live = i < len;
  const float mine = live ? keys[beg + i] : 0.f;
  int rank = 0;
  for (int t0 = 0; t0 < len; t0 += 1024) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int j = t0 + k * 256 + threadIdx.x;
      tile[k * 256 + threadIdx.x] = j < len ? keys[beg + j] : -INFINITY;
    }
    __syncthreads();
    const int m = min(1024, len - t0);
    for (int j = 0; j < m; ++j) {
      const float kj = tile[j];
      rank += (kj > mine || (kj == mine && t0 + j < i)) ? 1 : 0;
    }
    __syncthreads();
  }
  if (live && mine > -INFINITY) {
    atomicAdd(&out_cnt[seg], 1);
    if (rank < K) out_idx[(size_t)seg * K + rank] = i;
  }
}

// BoxCoder.decode_single for one box (models/detection/_utils.py), then clip_boxes_to_image
__device__ __forceinline__ float4 det_decode(float4 box, float dx, float dy, float dw, float dh, float wx, float wy, float ww, float wh,
                                             float clip_h, float clip_w) {
  const float width = box.z - box.x, height = box.w - box.y;
  const float ctr_x = box.x + 0.5f * width, ctr_y = box.y + 0.5f * height;
  dx = dx / wx; dy = dy / wy;
  dw = fminf(dw / ww, DET_XFORM_CLIP); dh = fminf(dh / wh, DET_XFORM_CLIP);
  const float pcx = dx * width + ctr_x, pcy = dy * height + ctr_y;
  const float pw = expf(dw) * width, ph = expf(dh) * height;
  float4 o = make_float4(pcx - 0.5f * pw, pcy - 0.5f * ph, pcx + 0.5f * pw, pcy + 0.5f * ph);
  o.x = fminf(fmaxf(o.x, 0.f), clip_w); o.z = fminf(fmaxf(o.z, 0.f), clip_w);
  o.y = fminf(fmaxf(o.y, 0.f), clip_h); o.w = fminf(fmaxf(o.w, 0.f), clip_h);
  return o;
}

// the pre-NMS top-k anchors of every (image, level): decode, clip, sigmoid, small-box / score filter (rpn.py filter_proposals)
__global__ __launch_bounds__(256) void det_rpn_gather_kernel(RpnLevels L, int n_images, const float* __restrict__ keys, const int* __restrict__ idx,
                                                             const int* __restrict__ cnt, int K, float clip_h, float clip_w, float min_size,
                                                             float score_thresh, float4* __restrict__ cand_box, float* __restrict__ cand_score,
                                                             int* __restrict__ cand_keep) {
  const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (long)n_images * DET_LEVELS * K) return;
  const int r = (int)(t % K), seg = (int)(t / K), l = seg % DET_LEVELS, n = seg / DET_LEVELS;
  const int len = L.off[l + 1] - L.off[l];
  const int c = min(min(cnt[seg], K), len);
  float4 box = make_float4(0.f, 0.f, 0.f, 0.f);
  float score = -INFINITY;
  int keep = 0;
  if (r < c) {
    const int j = idx[(size_t)seg * K + r];
    const int pix = j / DET_A, a = j - pix * DET_A;
    const int y = pix / L.gw[l], x = pix - y * L.gw[l];
    const float shx = (float)(x * L.stride_x[l]), shy = (float)(y * L.stride_y[l]);
    const float4 anchor = make_float4(shx + L.base[l][a][0], shy + L.base[l][a][1], shx + L.base[l][a][2], shy + L.base[l][a][3]);
    const float* h = L.head[l] + ((size_t)n * L.gh[l] * L.gw[l] + pix) * 16;
    box = det_decode(anchor, h[3 + a * 4], h[4 + a * 4], h[5 + a * 4], h[6 + a * 4], 1.f, 1.f, 1.f, 1.f, clip_h, clip_w);
    const float logit = keys[(size_t)n * L.off[DET_LEVELS] + L.off[l] + j];
    score = 1.f / (1.f + expf(-logit));
    keep = (box.z - box.x >= min_size && box.w - box.y >= min_size && score >= score_thresh) ? 1 : 0;
  }
  cand_box[t] = box;
  cand_score[t] = score;
  cand_keep[t] = keep;
}

// greedy NMS of one score-sorted segment per workgroup (torchvision/csrc/ops/cpu/nms_kernel.cpp semantics: suppress IoU > thr)
__global__ __launch_bounds__(256) void det_nms_kernel(const float4* __restrict__ boxes, int* __restrict__ keep, const int* __restrict__ cnt, int stride,
                                                      float thr) {
  __shared__ float4 sb[DET_MAX_SEG];
  __shared__ int sk[DET_MAX_SEG];
  const int seg = blockIdx.x;
  const int n = min(cnt ? cnt[seg] : stride, stride);
  for (int i = threadIdx.x; i < n; i += 256) {
    sb[i] = boxes[(size_t)seg * stride + i];
    sk[i] = keep[(size_t)seg * stride + i];
  }
  __syncthreads();
  for (int i = 0; i < n; ++i) {
    if (sk[i]) {   // (uniform: every thread reads the same word)
      const float4 bi = sb[i];
      const float ai = (bi.z - bi.x) * (bi.w - bi.y);
      for (int j = i + 1 + threadIdx.x; j < n; j += 256) {
        if (!sk[j]) continue;
        const float4 bj = sb[j];
        const float w = fmaxf(0.f, fminf(bi.z, bj.z) - fmaxf(bi.x, bj.x)), h = fmaxf(0.f, fminf(bi.w, bj.w) - fmaxf(bi.y, bj.y));
        const float inter = w * h;
        const float ovr = inter / (ai + (bj.z - bj.x) * (bj.w - bj.y) - inter);
        if (ovr > thr) sk[j] = 0;
      }
    }
    __syncthreads();
  }
  for (int i = threadIdx.x; i < n; i += 256) keep[(size_t)seg * stride + i] = sk[i];
}

// keys[i] = keep[i] ? score[i] : -inf
__global__ __launch_bounds__(256) void det_masked_keys_kernel(const float* __restrict__ score, const int* __restrict__ keep, long n, float* __restrict__ keys) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) keys[i] = keep[i] ? score[i] : -INFINITY;
}

// proposals[n][r] = cand_box[n][idx[n][r]] for r < min(cnt[n], K), zero boxes beyond; counts clamped to K
__global__ __launch_bounds__(256) void det_gather_boxes_kernel(const float4* __restrict__ cand_box, const float* __restrict__ cand_score, int per_image,
                                                               const int* __restrict__ idx, int* __restrict__ cnt, int K, int n_images,
                                                               float4* __restrict__ out_box, float* __restrict__ out_score) {
  const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (long)n_images * K) return;
  const int n = (int)(t / K), r = (int)(t % K);
  const int c = min(cnt[n], K);
  float4 b = make_float4(0.f, 0.f, 0.f, 0.f);
  float s = 0.f;
  if (r < c) {
    const int j = idx[t];
    b = cand_box[(size_t)n * per_image + j];
    s = cand_score[(size_t)n * per_image + j];
  }
  out_box[t] = b;
  if (out_score) out_score[t] = s;
}
__global__ void det_clamp_counts_kernel(int* __restrict__ cnt, int n, int K) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) cnt[i] = min(cnt[i], K);
}

struct PyramidRef {
  const float* feat[4];   // P2..P5, padded NHWC (border 1), 256 channels
  int h[4], w[4];
};

// MultiScaleRoIAlign(["0","1","2","3"], P, sampling_ratio = 2) (ops/poolers.py LevelMapper + ops/roi_align, aligned = False); one
// thread per (roi, bin, 4 channels); output [roi][P][P][256] with border `ob` (row stride (P + 2 ob)^2 * 256)
__global__ __launch_bounds__(256) void det_roi_align_kernel(PyramidRef py, const float4* __restrict__ rois, const int* __restrict__ cnt, int R, int n_images,
                                                            int P, int ob, float* __restrict__ out) {
  constexpr int C = DET_FPN_C, C4 = C / 4;
  const long total = (long)n_images * R * P * P * C4;
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= total) return;
  const int c4 = (int)(idx % C4);
  long t = idx / C4;
  const int pw = (int)(t % P);
  t /= P;
  const int ph = (int)(t % P);
  t /= P;
  const int r = (int)(t % R), n = (int)(t / R);
  const int Pq = P + 2 * ob;
  float* o = out + ((((size_t)n * R + r) * Pq + ph + ob) * Pq + pw + ob) * C + c4 * 4;
  if (r >= min(cnt[n], R)) {
    *reinterpret_cast<float4*>(o) = make_float4(0.f, 0.f, 0.f, 0.f);
    return;
  }
  const float4 b = rois[(size_t)n * R + r];
  // LevelMapper: k = floor(4 + log2(sqrt(area) / 224) + 1e-6) clamped to [2, 5]
  const float s = sqrtf((b.z - b.x) * (b.w - b.y));
  float lv = floorf(4.f + log2f(s / 224.f) + 1e-6f);
  lv = fminf(fmaxf(lv, 2.f), 5.f);
  const int l = (int)lv - 2;
  const float scale = 1.f / (float)(4 << l);
  const int H = py.h[l], W = py.w[l];
  const float* f = py.feat[l] + (size_t)n * (H + 2) * (W + 2) * C + c4 * 4;
  const float x1 = b.x * scale, y1 = b.y * scale, x2 = b.z * scale, y2 = b.w * scale;
  const float roi_w = fmaxf(x2 - x1, 1.f), roi_h = fmaxf(y2 - y1, 1.f);
  const float bin_h = roi_h / (float)P, bin_w = roi_w / (float)P;
  float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
  for (int iy = 0; iy < 2; ++iy) {
    float y = y1 + (float)ph * bin_h + ((float)iy + 0.5f) * bin_h / 2.f;
#pragma unroll
    for (int ix = 0; ix < 2; ++ix) {
      float x = x1 + (float)pw * bin_w + ((float)ix + 0.5f) * bin_w / 2.f;
      float yy = y;
      if (yy < -1.f || yy > (float)H || x < -1.f || x > (float)W) continue;
      if (yy <= 0.f) yy = 0.f;
      if (x <= 0.f) x = 0.f;
      int yl = (int)yy, xl = (int)x, yh, xh;
      if (yl >= H - 1) { yh = yl = H - 1; yy = (float)yl; } else yh = yl + 1;
      if (xl >= W - 1) { xh = xl = W - 1; x = (float)xl; } else xh = xl + 1;
      const float ly = yy - (float)yl, lx = x - (float)xl, hy = 1.f - ly, hx = 1.f - lx;
      const float w1 = hy * hx, w2 = hy * lx, w3 = ly * hx, w4 = ly * lx;
      const float4 v1 = *reinterpret_cast<const float4*>(f + ((size_t)(yl + 1) * (W + 2) + xl + 1) * C);
      const float4 v2 = *reinterpret_cast<const float4*>(f + ((size_t)(yl + 1) * (W + 2) + xh + 1) * C);
      const float4 v3 = *reinterpret_cast<const float4*>(f + ((size_t)(yh + 1) * (W + 2) + xl + 1) * C);
      const float4 v4 = *reinterpret_cast<const float4*>(f + ((size_t)(yh + 1) * (W + 2) + xh + 1) * C);
      acc.x += w1 * v1.x + w2 * v2.x + w3 * v3.x + w4 * v4.x;
      acc.y += w1 * v1.y + w2 * v2.y + w3 * v3.y + w4 * v4.y;
      acc.z += w1 * v1.z + w2 * v2.z + w3 * v3.z + w4 * v4.z;
      acc.w += w1 * v1.w + w2 * v2.w + w3 * v3.w + w4 * v4.w;
    }
  }
  *reinterpret_cast<float4*>(o) = make_float4(acc.x / 4.f, acc.y / 4.f, acc.z / 4.f, acc.w / 4.f);
}

// roi_heads.py postprocess_detections up to the NMS: softmax, per-class decode (weights 10, 10, 5, 5), clip, score / size filter.
// pred row = [C logits | 4C deltas (c * 4 + k)]; candidates are written class-major: seg = n * (C - 1) + (c - 1), element r
__global__ __launch_bounds__(256) void det_box_post_kernel(const float* __restrict__ pred, int row_stride, int C, const float4* __restrict__ props,
                                                           const int* __restrict__ prop_cnt, int R, int n_images, float clip_h, float clip_w,
                                                           float score_thresh, float min_size, float4* __restrict__ cand_box,
                                                           float* __restrict__ cand_key) {
  const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (long)n_images * R) return;
  const int n = (int)(t / R), r = (int)(t % R);
  const bool live = r < min(prop_cnt[n], R);
  const float* row = pred + (size_t)t * row_stride;
  float m = -INFINITY, sum = 0.f;
  if (live) {
    for (int c = 0; c < C; ++c) m = fmaxf(m, row[c]);
    for (int c = 0; c < C; ++c) sum += expf(row[c] - m);
  }
  const float4 p = props[t];
  for (int c = 1; c < C; ++c) {
    const size_t o = ((size_t)n * (C - 1) + (c - 1)) * R + r;
    float4 b = make_float4(0.f, 0.f, 0.f, 0.f);
    float key = -INFINITY;
    if (live) {
      const float sc = expf(row[c] - m) / sum;
      const float* d = row + C + c * 4;
      b = det_decode(p, d[0], d[1], d[2], d[3], 10.f, 10.f, 5.f, 5.f, clip_h, clip_w);
      if (sc > score_thresh && b.z - b.x >= min_size && b.w - b.y >= min_size) key = sc;
    }
    cand_box[o] = b;
    cand_key[o] = key;
  }
}

// sorted copies of a segment's candidates: out[seg][r] = in[seg][idx[seg][r]] for r < min(cnt, K); keep = 1 there, 0 beyond;
// inv[seg][idx[seg][r]] = r (the sorted position of every live candidate)
__global__ __launch_bounds__(256) void det_sorted_gather_kernel(const float4* __restrict__ box, const float* __restrict__ key, const int* __restrict__ idx,
                                                                const int* __restrict__ cnt, int K, long n_total, float4* __restrict__ sbox,
                                                                float* __restrict__ skey, int* __restrict__ keep, int* __restrict__ inv) {
  const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n_total) return;
  const int seg = (int)(t / K), r = (int)(t % K);
  const bool live = r < min(cnt[seg], K);
  const int j = live ? idx[t] : 0;
  sbox[t] = live ? box[(size_t)seg * K + j] : make_float4(0.f, 0.f, 0.f, 0.f);
  skey[t] = live ? key[(size_t)seg * K + j] : -INFINITY;
  keep[t] = live ? 1 : 0;
  if (live) inv[(size_t)seg * K + j] = r;
}

// keys of the final selection in torchvision's candidate order (roi_heads.py flattens [proposal, class]): fkey[n][r * (C - 1) + c - 1] =
// the class-c candidate of proposal r if it survived its class's NMS, else -inf.  The stable rank sort then breaks score ties by
// (proposal, class) as torchvision's stable score sort of batched_nms does, not by class first.
__global__ __launch_bounds__(256) void det_final_keys_kernel(const float* __restrict__ key, const int* __restrict__ keep, const int* __restrict__ inv,
                                                             int C1, int R, long n_total, float* __restrict__ fkey) {
  const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n_total) return;
  const long nr = t / C1;
  const int c1 = (int)(t - nr * C1), n = (int)(nr / R), r = (int)(nr % R);
  const size_t o = ((size_t)n * C1 + c1) * R + r;   // class-major candidate slot
  const float k = key[o];
  fkey[t] = (k > -INFINITY && keep[((size_t)n * C1 + c1) * R + inv[o]]) ? k : -INFINITY;
}

// final outputs of one image: the D best surviving candidates over all classes (idx in det_final_keys_kernel's proposal-major order,
// box / key read from the class-major candidate lists); boxes mapped back to the original frame
__global__ __launch_bounds__(256) void det_final_kernel(const float4* __restrict__ box, const float* __restrict__ key, const int* __restrict__ idx,
                                                        const int* __restrict__ cnt, int D, int C1, int R, int n_images, float ratio_h,
                                                        float ratio_w, float4* __restrict__ out_box, float* __restrict__ out_score,
                                                        int* __restrict__ out_label, int* __restrict__ out_cnt, float4* __restrict__ resized_box) {
  const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (long)n_images * D) return;
  const int n = (int)(t / D), d = (int)(t % D);
  const int c = min(cnt[n], D);
  float4 b = make_float4(0.f, 0.f, 0.f, 0.f), br = b;
  float s = 0.f;
  int lab = 0;
  if (d < c) {
    const int j = idx[t], r = j / C1, c1 = j - r * C1;
    const size_t o = ((size_t)n * C1 + c1) * R + r;
    br = box[o];
    s = key[o];
    lab = c1 + 1;
    b = make_float4(br.x * ratio_w, br.y * ratio_h, br.z * ratio_w, br.w * ratio_h);   // transform.py resize_boxes
  }
  out_box[t] = b;
  out_score[t] = s;
  out_label[t] = lab;
  resized_box[t] = br;
  if (d == 0) out_cnt[n] = c;
}

// roi_heads.py maskrcnn_inference (sigmoid, class selection) + paste_masks_in_image: one thread per pixel of [n, D, H, W]
__global__ __launch_bounds__(256) void det_mask_paste_kernel(const float* __restrict__ logits /*[n*D*14*14*4][Cs]*/, int Cs, const float4* __restrict__ boxes,
                                                             const int* __restrict__ labels, const int* __restrict__ cnt, int D, int H, int W,
                                                             float* __restrict__ out) {
  const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const int det = blockIdx.y;   // n * D + d
  if (t >= (long)H * W) return;
  const int n = det / D, d = det - n * D;
  float* o = out + (size_t)det * H * W + t;
  if (d >= min(cnt[n], D)) { *o = 0.f; return; }
  const int Y = (int)(t / W), X = (int)(t % W);
  const float4 b = boxes[det];
  constexpr int M = 28, PAD = 1, MP = M + 2 * PAD;
  const float scale = (float)MP / (float)M;
  const float w_half = (b.z - b.x) * 0.5f * scale, h_half = (b.w - b.y) * 0.5f * scale;
  const float xc = (b.z + b.x) * 0.5f, yc = (b.w + b.y) * 0.5f;
  const int bx0 = (int)(xc - w_half), by0 = (int)(yc - h_half), bx1 = (int)(xc + w_half), by1 = (int)(yc + h_half);   // .to(int64): truncation
  const int w = max(bx1 - bx0 + 1, 1), h = max(by1 - by0 + 1, 1);
  const int x_0 = max(bx0, 0), x_1 = min(bx1 + 1, W), y_0 = max(by0, 0), y_1 = min(by1 + 1, H);
  if (X < x_0 || X >= x_1 || Y < y_0 || Y >= y_1) { *o = 0.f; return; }
  // bilinear resize of the zero-padded 30 x 30 probability map to (h, w), align_corners = False
  const int dx = X - bx0, dy = Y - by0;
  float fy = ((float)MP / (float)h) * ((float)dy + 0.5f) - 0.5f, fx = ((float)MP / (float)w) * ((float)dx + 0.5f) - 0.5f;
  fy = fy < 0.f ? 0.f : fy;
  fx = fx < 0.f ? 0.f : fx;
  const int y0 = (int)fy, x0 = (int)fx;
  const int y1 = y0 + (y0 < MP - 1 ? 1 : 0), x1 = x0 + (x0 < MP - 1 ? 1 : 0);
  const float ly = fy - (float)y0, lx = fx - (float)x0, hy = 1.f - ly, hx = 1.f - lx;
  const int lab = labels[det];
  auto prob = [&](int py, int px) -> float {
    if (py < PAD || py >= M + PAD || px < PAD || px >= M + PAD) return 0.f;
    const int my = py - PAD, mx = px - PAD;   // 28 x 28 mask pixel = (2 y + a, 2 x + b) of the transposed convolution
    const size_t row = (((size_t)det * 14 + (my >> 1)) * 14 + (mx >> 1)) * 4 + ((my & 1) * 2 + (mx & 1));
    return 1.f / (1.f + expf(-logits[row * Cs + lab]));
  };
  *o = hy * (hx * prob(y0, x0) + lx * prob(y0, x1)) + ly * (hx * prob(y1, x0) + lx * prob(y1, x1));
}

// ---------------------------------------------------------------------------------------------------------------------------------
// host side: the network, stated once
// ---------------------------------------------------------------------------------------------------------------------------------
}  // namespace mp

using namespace mp;

namespace {

constexpr int RES_BLOCKS[4] = {3, 4, 6, 3};          // ResNet-50: bottlenecks per stage ...
constexpr int RES_PLANES[4] = {64, 128, 256, 512};   // ... and their inner width; a stage writes 4 x planes channels (C2..C5, the FPN's inputs)
constexpr int RES_MAX_BLOCKS = 6;
constexpr size_t DET_SPLITK_FLOATS = 16u << 20;
const char* const WHO = "mp_detector_create";

inline int pad4(int c) { return (c + 3) / 4 * 4; }   // row strides of the predictor (5 C) / mask-logit (C) outputs, input channels of a layer

struct Bottleneck {
  ConvLayer c1, c2, c3, down;   // `down` only in a stage's first block
};

struct DetLayers {
  ConvLayer stem;
  Bottleneck block[4][RES_MAX_BLOCKS];
  ConvLayer fpn_inner[4], fpn_layer[4], rpn_conv, rpn_head, fc6, fc7, pred, mask_fcn[4], mask_deconv, mask_logits;
};

struct Dims {
  int n;
  int64_t d[4];
  int64_t numel() const {
    int64_t m = 1;
    for (int k = 0; k < n; ++k) m *= d[k];
    return m;
  }
};

// The checkpoint's tensors (torchvision's state_dict keys) and the layers built from them, in checkpoint order.  A Sink has
//   bool tensor(name, dims, &p)   one checkpoint tensor; p = its host data where the sink `builds`
//   bool layer(L, w, bn, bias, cout_pad, Cout, Cin, K, stride, pad)   OIHW weights (+ bn prefix or "", + bias or null) -> *L
// and `rc`, what a false return of those leaves behind: the walk stops there and returns it.
template <class Sink>
int det_walk(int C, DetLayers& net, Sink& k) {
#define DET_STEP(e) do { if (!(e)) return k.rc; } while (0)
  // a layer that takes its weight as the checkpoint holds it, [Cout, Cin, K, K] (`linear`: [Cout, Cin]), under FrozenBatchNorm `bn` or,
  // with bn = "", with a bias of its own
  auto plain = [&](ConvLayer* L, const std::string& name, const std::string& bn, int Cout, int Cin, int K, int stride, int pad, bool linear = false,
                   int cout_pad = 0) {
    const float *w = nullptr, *b = nullptr, *folded = nullptr;   // (make_conv_layer reads the four vectors of `bn` itself and folds them)
    if (!k.tensor(name + ".weight", linear ? Dims{2, {Cout, Cin}} : Dims{4, {Cout, Cin, K, K}}, &w)) return false;
    if (bn.empty() && !k.tensor(name + ".bias", Dims{1, {Cout}}, &b)) return false;
    for (const char* s : {"weight", "bias", "running_mean", "running_var"})
      if (!bn.empty() && !k.tensor(bn + "." + s, Dims{1, {Cout}}, &folded)) return false;
    return k.layer(L, w, bn, b, cout_pad, Cout, Cin, K, stride, pad);
  };
  // two heads over one input as ONE 1x1 layer: the rows of `a`, then those of `b`, then zero rows up to cout_p
  auto stacked = [&](ConvLayer* L, const std::string& a, const std::string& b, int Ca, int Cb, int Cin, int cout_p, bool linear) {
    const float *wa = nullptr, *ba = nullptr, *wb = nullptr, *bb = nullptr;
    auto wd = [&](int c) { return linear ? Dims{2, {c, Cin}} : Dims{4, {c, Cin, 1, 1}}; };
    if (!k.tensor(a + ".weight", wd(Ca), &wa) || !k.tensor(a + ".bias", Dims{1, {Ca}}, &ba) || !k.tensor(b + ".weight", wd(Cb), &wb) ||
        !k.tensor(b + ".bias", Dims{1, {Cb}}, &bb))
      return false;
    std::vector<float> w, bias;
    if (Sink::builds) {
      w.assign((size_t)cout_p * Cin, 0.f);
      bias.assign(cout_p, 0.f);
      memcpy(w.data(), wa, sizeof(float) * Ca * Cin);
      memcpy(w.data() + (size_t)Ca * Cin, wb, sizeof(float) * Cb * Cin);
      memcpy(bias.data(), ba, sizeof(float) * Ca);
      memcpy(bias.data() + Ca, bb, sizeof(float) * Cb);
    }
    return k.layer(L, w.data(), "", bias.data(), cout_p, cout_p, Cin, 1, 1, 0);
  };

  const std::string B = "backbone.body.";
  DET_STEP(plain(&net.stem, B + "conv1", B + "bn1", 64, 3, 7, 2, 3));
  int inplanes = 64;
  for (int st = 0; st < 4; ++st)
    for (int bi = 0; bi < RES_BLOCKS[st]; ++bi) {
      const std::string P = B + "layer" + std::to_string(st + 1) + "." + std::to_string(bi) + ".";
      const int p = RES_PLANES[st], stride = (bi == 0 && st > 0) ? 2 : 1;
      Bottleneck& blk = net.block[st][bi];
      DET_STEP(plain(&blk.c1, P + "conv1", P + "bn1", p, inplanes, 1, 1, 0));
      DET_STEP(plain(&blk.c2, P + "conv2", P + "bn2", p, p, 3, stride, 1));   // (torchvision: stride on the 3x3)
      DET_STEP(plain(&blk.c3, P + "conv3", P + "bn3", 4 * p, p, 1, 1, 0));
      if (bi == 0) DET_STEP(plain(&blk.down, P + "downsample.0", P + "downsample.1", 4 * p, inplanes, 1, stride, 0));
      inplanes = 4 * p;
    }
  for (int i = 0; i < 4; ++i) {
    const std::string s = std::to_string(i);
    DET_STEP(plain(&net.fpn_inner[i], "backbone.fpn.inner_blocks." + s, "", DET_FPN_C, 4 * RES_PLANES[i], 1, 1, 0));
    DET_STEP(plain(&net.fpn_layer[i], "backbone.fpn.layer_blocks." + s, "", DET_FPN_C, DET_FPN_C, 3, 1, 1));
  }
  DET_STEP(plain(&net.rpn_conv, "rpn.head.conv", "", DET_FPN_C, DET_FPN_C, 3, 1, 1));
  DET_STEP(stacked(&net.rpn_head, "rpn.head.cls_logits", "rpn.head.bbox_pred", DET_A, 4 * DET_A, DET_FPN_C, 16, false));
  {  // fc6: torchvision flattens [R, 256, 7, 7] channel-major; the RoIAlign output here is [R, 7, 7, 256]
    const float *w6 = nullptr, *b6 = nullptr;
    DET_STEP(k.tensor("roi_heads.box_head.fc6.weight", Dims{2, {1024, 256 * 7 * 7}}, &w6));
    DET_STEP(k.tensor("roi_heads.box_head.fc6.bias", Dims{1, {1024}}, &b6));
    std::vector<float> w;
    if (Sink::builds) {
      w.resize((size_t)1024 * 12544);
      for (int o = 0; o < 1024; ++o)
        for (int c = 0; c < 256; ++c)
          for (int q = 0; q < 49; ++q) w[(size_t)o * 12544 + (size_t)q * 256 + c] = w6[(size_t)o * 12544 + (size_t)c * 49 + q];
    }
    DET_STEP(k.layer(&net.fc6, w.data(), "", b6, 0, 1024, 12544, 1, 1, 0));
  }
  DET_STEP(plain(&net.fc7, "roi_heads.box_head.fc7", "", 1024, 1024, 1, 1, 0, true));
  DET_STEP(stacked(&net.pred, "roi_heads.box_predictor.cls_score", "roi_heads.box_predictor.bbox_pred", C, 4 * C, 1024, pad4(5 * C), true));
  for (int i = 0; i < 4; ++i)
    DET_STEP(plain(&net.mask_fcn[i], "roi_heads.mask_head.mask_fcn" + std::to_string(i + 1), "", DET_FPN_C, DET_FPN_C, 3, 1, 1));
  {  // ConvTranspose2d(256, 256, 2, 2): out[o, 2y+a, 2x+b] = sum_i in[i, y, x] W[i, o, a, b] + bias[o]  ->  1x1 conv onto (a, b, o)
    const float *wt = nullptr, *bt = nullptr;
    DET_STEP(k.tensor("roi_heads.mask_predictor.conv5_mask.weight", Dims{4, {256, 256, 2, 2}}, &wt));
    DET_STEP(k.tensor("roi_heads.mask_predictor.conv5_mask.bias", Dims{1, {256}}, &bt));
    std::vector<float> w, b;
    if (Sink::builds) {
      w.resize((size_t)1024 * 256);
      b.resize(1024);
      for (int ab = 0; ab < 4; ++ab)
        for (int o = 0; o < 256; ++o) {
          b[ab * 256 + o] = bt[o];
          for (int i = 0; i < 256; ++i) w[((size_t)ab * 256 + o) * 256 + i] = wt[((size_t)i * 256 + o) * 4 + ab];
        }
    }
    DET_STEP(k.layer(&net.mask_deconv, w.data(), "", b.data(), 0, 1024, 256, 1, 1, 0));
  }
  // (zero output channels up to the padded row; the bias is read for the C real ones only)
  DET_STEP(plain(&net.mask_logits, "roi_heads.mask_predictor.mask_fcn_logits", "", C, DET_FPN_C, 1, 1, 0, false, pad4(C)));
#undef DET_STEP
  return MP_OK;
}

struct SpecEntry {
  std::string name;
  Dims dims;
};

struct SpecSink {   // mp_detector_state_spec: the list of (name, shape)
  static constexpr bool builds = false;
  int rc = MP_OK;
  std::vector<SpecEntry> v;
  bool tensor(const std::string& name, const Dims& d, const float** p) {
    *p = nullptr;
    v.push_back({name, d});
    return true;
  }
  bool layer(ConvLayer*, const float*, const std::string&, const float*, int, int, int, int, int, int) { return true; }
};

struct CreateSink {   // mp_detector_create: look the tensor up, build the layer in its fp32 form
  static constexpr bool builds = true;
  std::vector<void*>& allocs;
  const StateMap& sm;
  int rc = MP_OK;
  bool tensor(const std::string& name, const Dims& d, const float** p) {
    *p = find(sm, name, d.numel(), WHO);
    if (!*p) rc = MP_ERR_INVALID;
    return *p != nullptr;
  }
  bool layer(ConvLayer* L, const float* w, const std::string& bn, const float* bias, int cout_pad, int Cout, int Cin, int K, int stride, int pad) {
    rc = make_conv_layer(allocs, sm, WHO, w, bn, bias, cout_pad, Cin, pad4(Cin), Cout, K, stride, pad, 0u, L);
    return rc == MP_OK;
  }
};

// ---------------------------------------------------------------------------------------------------------------------------------
// host side: workspace plan
// ---------------------------------------------------------------------------------------------------------------------------------
inline size_t tensor_floats(int N, int H, int W, int C, int b) { return (size_t)N * (H + 2 * b) * (W + 2 * b) * C + (size_t)(W + 2 * b) * C + 64; }

// one workspace buffer: where it lies and what it was sized from (what mp_detector_debug_tensor publishes of it)
struct DetBuf {
  size_t off = 0;                    // from the workspace's start, in 4-byte elements
  int64_t shape[4] = {0, 0, 0, 0};   // logical extent
  int border = 0;                    // zero ring around a padded NHWC map
  int64_t row_stride = 0;
  int64_t n_elements = 0;            // 4-byte elements the layout spans, border and row padding included (the slack behind it is not)
  bool is_int = false;               // int32, else float
};

struct DetStage {
  DetBuf x[2], t1, t1in, t2, d;   // the blocks' outputs alternate between x[0] and x[1]
};

// every buffer of a forward at (n, H, W), bump-allocated in floats (64-float aligned, + the slack the conv's last K chunk may read past a
// tensor's end)
struct DetPlan {
  int n, H, W, hr, wr, Hp, Wp;          // input, resized, padded (multiple of 32)
  float ratio_h, ratio_w;               // input / resized
  int fh[DET_LEVELS], fw[DET_LEVELS];   // P2..P6
  int a_total;                          // anchors per image
  size_t total = 0;
  DetBuf x0, stem, pool;
  DetStage stage[4];
  int stage_buf[4] = {0, 0, 0, 0};      // which x[] of a stage holds its output C2..C5 (set by the forward: what the FPN read)
  DetBuf L[4], U[4], P[DET_LEVELS], rpn_t[DET_LEVELS], rpn_h[DET_LEVELS];
  DetBuf keys, seg_off, seg_off2, seg_off3, idx1, cnt1, cand_box, cand_score, cand_keep, keys2, idx2, proposals, proposal_scores, proposal_counts;
  DetBuf roi7, fc6, fc7, class_logits, c2_box, c2_key, c2_idx, c2_cnt, c2_sbox, c2_skey, c2_keep, c2_inv, c2_fkey, f_idx, f_cnt, det_resized;
  DetBuf roi14, m_a, m_b, m_up, mask_logits, splitk, end;

  void take(DetBuf& b, size_t floats, DetBuf what) {
    b = what;
    b.off = total;
    total += (floats + 63) / 64 * 64;
  }
  // padded NHWC map {N, h, w, c} inside a zero ring of b pixels
  void map(DetBuf& B, int N, int h, int w, int c, int b) {
    take(B, tensor_floats(N, h, w, c, b), DetBuf{0, {N, h, w, c}, b, c, (int64_t)N * (h + 2 * b) * (w + 2 * b) * c, false});
  }
  // row matrix {rows, width}, the rows `stride` >= width apart
  void rows(DetBuf& B, int rows, int width, int stride) {
    take(B, tensor_floats(rows, 1, 1, stride, 0), DetBuf{0, {rows, width, 1, 1}, 0, stride, (int64_t)rows * stride, false});
  }
  // flat list {N, per, width} (+ slack elements behind it)
  void list(DetBuf& B, size_t N, size_t per, int width, bool is_int = false, size_t slack = 0) {
    const int64_t n_el = (int64_t)(N * per * width);
    take(B, (size_t)n_el + slack, DetBuf{0, {(int64_t)N, (int64_t)per, width, 1}, 0, width, n_el, is_int});
  }
};

int det_make_plan(const mp_detector_config& c, int n, int H, int W, DetPlan* p) {
  *p = DetPlan();
  p->n = n; p->H = H; p->W = W;
  // transform.py _resize_image_and_masks: scale = min(min_size / min(h, w), max_size / max(h, w)) in float32; out = floor(in * scale)
  const float scale = std::min((float)c.min_size / (float)std::min(H, W), (float)c.max_size / (float)std::max(H, W));
  p->hr = (int)std::floor((double)H * (double)scale);
  p->wr = (int)std::floor((double)W * (double)scale);
  MP_REQUIRE(p->hr >= 32 && p->wr >= 32, "mp_detector: resized image %dx%d too small", p->hr, p->wr);
  p->Hp = (p->hr + 31) / 32 * 32;
  p->Wp = (p->wr + 31) / 32 * 32;
  p->ratio_h = (float)H / (float)p->hr;
  p->ratio_w = (float)W / (float)p->wr;
  for (int l = 0; l < 4; ++l) { p->fh[l] = p->Hp >> (l + 2); p->fw[l] = p->Wp >> (l + 2); }
  p->fh[4] = (p->fh[3] - 1) / 2 + 1;
  p->fw[4] = (p->fw[3] - 1) / 2 + 1;
  p->a_total = 0;
  for (int l = 0; l < DET_LEVELS; ++l) p->a_total += p->fh[l] * p->fw[l] * DET_A;
  const int C = c.n_classes, R = c.rpn_post_nms_top_n, Kp = c.rpn_pre_nms_top_n, D = c.box_detections_per_img;
  const bool i32 = true;
  p->map(p->x0, n, p->Hp, p->Wp, 4, 3);
  p->map(p->stem, n, p->Hp / 2, p->Wp / 2, 64, 1);
  p->map(p->pool, n, p->Hp / 4, p->Wp / 4, 64, 1);
  for (int s = 0; s < 4; ++s) {
    const int h = p->fh[s], w = p->fw[s], pl = RES_PLANES[s];
    DetStage& S = p->stage[s];
    p->map(S.x[0], n, h, w, 4 * pl, 1);
    p->map(S.x[1], n, h, w, 4 * pl, 1);
    p->map(S.t1, n, h, w, pl, 1);
    // block 0 runs its first 1x1 at the INPUT resolution of the stage: its own buffer (a buffer must keep ONE geometry, its zero
    // border is only established once per forward)
    p->map(S.t1in, n, s == 0 ? h : 2 * h, s == 0 ? w : 2 * w, pl, 1);
    p->map(S.t2, n, h, w, pl, 1);
    p->map(S.d, n, h, w, 4 * pl, 1);
    p->map(p->L[s], n, h, w, DET_FPN_C, 1);
    p->map(p->U[s], n, h, w, DET_FPN_C, 1);
  }
  for (int l = 0; l < DET_LEVELS; ++l) {
    p->map(p->P[l], n, p->fh[l], p->fw[l], DET_FPN_C, 1);
    p->map(p->rpn_t[l], n, p->fh[l], p->fw[l], DET_FPN_C, 0);
    p->map(p->rpn_h[l], n, p->fh[l], p->fw[l], 16, 0);
  }
  const size_t N = n, n_lv = N * DET_LEVELS, n_cls = N * (C - 1);   // segments of the sorts: images, (image, level), (image, class)
  p->list(p->keys, N, p->a_total, 1);
  p->list(p->seg_off, N, std::max(DET_LEVELS, C), 1, i32, 64 + 2);   // segment tables of the sorts
  p->list(p->seg_off2, N, 1, 1, i32, 64 + 2);
  p->list(p->seg_off3, N, 1, 1, i32, 64 + 2);
  p->list(p->idx1, n_lv, Kp, 1, i32);
  p->list(p->cnt1, n_lv, 1, 1, i32, 64);
  p->list(p->cand_box, n_lv, Kp, 4);
  p->list(p->cand_score, n_lv, Kp, 1);
  p->list(p->cand_keep, n_lv, Kp, 1, i32);
  p->list(p->keys2, n_lv, Kp, 1);
  p->list(p->idx2, N, R, 1, i32);
  p->list(p->proposals, N, R, 4);
  p->list(p->proposal_scores, N, R, 1);
  p->list(p->proposal_counts, N, 1, 1, i32, 64);
  p->rows(p->roi7, n * R, 7 * 7 * DET_FPN_C, 7 * 7 * DET_FPN_C);   // (y, x, channel)
  p->rows(p->fc6, n * R, 1024, 1024);
  p->rows(p->fc7, n * R, 1024, 1024);
  p->rows(p->class_logits, n * R, 5 * C, pad4(5 * C));
  p->list(p->c2_box, n_cls, R, 4);
  p->list(p->c2_key, n_cls, R, 1);
  p->list(p->c2_idx, n_cls, R, 1, i32);
  p->list(p->c2_cnt, n_cls, 1, 1, i32, 64);
  p->list(p->c2_sbox, n_cls, R, 4);
  p->list(p->c2_skey, n_cls, R, 1);
  p->list(p->c2_keep, n_cls, R, 1, i32);
  p->list(p->c2_inv, n_cls, R, 1, i32);
  p->list(p->c2_fkey, n_cls, R, 1);
  p->list(p->f_idx, N, D, 1, i32);
  p->list(p->f_cnt, N, 1, 1, i32, 64);
  p->list(p->det_resized, N, D, 4);
  p->map(p->roi14, n * D, 14, 14, DET_FPN_C, 1);
  p->map(p->m_a, n * D, 14, 14, DET_FPN_C, 1);
  p->map(p->m_b, n * D, 14, 14, DET_FPN_C, 1);
  p->map(p->m_up, n * D, 14, 14, 4 * DET_FPN_C, 0);
  p->rows(p->mask_logits, n * D * 14 * 14 * 4, C, pad4(C));
  p->list(p->splitk, 1, DET_SPLITK_FLOATS, 1);
  p->list(p->end, 1, 4096, 1);
  return MP_OK;
}

// the taps mp_detector_debug_tensor publishes; every other buffer is internal
struct DetTap {
  const char* name;
  DetBuf DetPlan::*buf;
};
const DetTap DET_TAPS[] = {{"x0", &DetPlan::x0}, {"pool", &DetPlan::pool}, {"keys", &DetPlan::keys}, {"proposals", &DetPlan::proposals},
                           {"proposal_scores", &DetPlan::proposal_scores}, {"proposal_counts", &DetPlan::proposal_counts},
                           {"roi7", &DetPlan::roi7}, {"class_logits", &DetPlan::class_logits}, {"f_cnt", &DetPlan::f_cnt},
                           {"det_resized", &DetPlan::det_resized}, {"roi14", &DetPlan::roi14}, {"mask_logits", &DetPlan::mask_logits}};

const DetBuf* det_find_tap(const DetPlan& p, const char* what) {
  if (what[0] && what[1] && !what[2]) {   // C2..C5: the buffer the stage's last block wrote; L2..L5: the FPN's top-down maps; P2..P6
    const int k = what[1] - '2';
    if (what[0] == 'C' && k >= 0 && k < 4) return &p.stage[k].x[p.stage_buf[k]];
    if (what[0] == 'L' && k >= 0 && k < 4) return &p.L[k];
    if (what[0] == 'P' && k >= 0 && k < DET_LEVELS) return &p.P[k];
  }
  for (const DetTap& t : DET_TAPS)
    if (!strcmp(t.name, what)) return &(p.*t.buf);
  return nullptr;
}

// what the steps of one forward share; the first error sticks and turns the steps after it into no-ops
struct DetRun {
  hipStream_t s;
  float* splitk;
  int n;   // images
  int rc = MP_OK;
  void conv(const ConvLayer& L, const float* x, int N, int H, int W, int in_border, float* y, int out_border, const float* res, int relu) {
    if (!rc) rc = run_conv_layer(L, x, N, H, W, in_border, y, out_border, res, relu, s, splitk, DET_SPLITK_FLOATS);
  }
  // stable rank sort of `per_image` x n segments of `len` keys each: the indices of every segment's `top` largest keys + how many it has
  void rank_topk(const float* keys, int per_image, int len, int top, int* seg_off, int* idx, int* cnt) {
    if (rc) return;
    const int n_seg = n * per_image;
    hipLaunchKernelGGL(det_seg_offsets_kernel, dim3(ceil_div((long)n_seg + 1, 256)), dim3(256), 0, s, n_seg, len, seg_off);
    hipLaunchKernelGGL(det_rank_topk_kernel, dim3(ceil_div(len, 256), n_seg), dim3(256), 0, s, keys, seg_off, top, idx, cnt);
  }
};

}  // namespace

struct mp_detector {
  mp_detector_config cfg;
  DetLayers net;
  float base_anchors[DET_LEVELS][DET_A][4];
  std::vector<void*> allocs;
  // last forward (debug taps)
  bool ran = false;
  DetPlan last;
  void* last_ws = nullptr;
};

extern "C" int mp_detector_default_config(mp_detector_config* cfg, int n_classes, int min_size, int max_size) {
  MP_REQUIRE(cfg && n_classes >= 2 && min_size > 0 && max_size >= min_size, "mp_detector_default_config: bad arguments");
  memset(cfg, 0, sizeof(*cfg));
  cfg->n_classes = n_classes;
  cfg->min_size = min_size;
  cfg->max_size = max_size;
  const float mean[3] = {0.485f, 0.456f, 0.406f}, sd[3] = {0.229f, 0.224f, 0.225f};
  const int sizes[5] = {32, 64, 128, 256, 512};
  const float ar[3] = {0.5f, 1.0f, 2.0f};
  memcpy(cfg->image_mean, mean, sizeof(mean));
  memcpy(cfg->image_std, sd, sizeof(sd));
  memcpy(cfg->anchor_sizes, sizes, sizeof(sizes));
  memcpy(cfg->aspect_ratios, ar, sizeof(ar));
  cfg->rpn_pre_nms_top_n = 1000; cfg->rpn_post_nms_top_n = 1000;
  cfg->rpn_nms_thresh = 0.7f; cfg->rpn_score_thresh = 0.0f; cfg->rpn_min_size = 1e-3f;
  cfg->box_score_thresh = 0.05f; cfg->box_nms_thresh = 0.5f; cfg->box_min_size = 1e-2f;
  cfg->box_detections_per_img = 100;
  return MP_OK;
}

extern "C" int mp_detector_state_spec(int n_classes, int idx, char* name, int name_len, int64_t* shape4, int32_t* n_dims) {
  MP_REQUIRE(n_classes >= 2 && idx >= 0 && name && name_len > 0 && shape4 && n_dims, "mp_detector_state_spec: bad arguments");
  SpecSink k;
  DetLayers unbuilt;
  det_walk(n_classes, unbuilt, k);
  if (idx >= (int)k.v.size()) return 1;
  const SpecEntry& e = k.v[idx];
  snprintf(name, name_len, "%s", e.name.c_str());
  for (int i = 0; i < 4; ++i) shape4[i] = i < e.dims.n ? e.dims.d[i] : 1;
  *n_dims = e.dims.n;
  return MP_OK;
}

extern "C" int mp_detector_destroy(mp_detector* d) {
  if (!d) return MP_OK;
  for (void* p : d->allocs) (void)hipFree(p);
  delete d;
  return MP_OK;
}

extern "C" int mp_detector_create(const mp_detector_config* cfg, const mp_named_tensor* st, int n_tensors, mp_detector** out) {
  MP_REQUIRE(cfg && st && n_tensors > 0 && out, "mp_detector_create: bad arguments");
  MP_REQUIRE(cfg->n_classes >= 2 && cfg->n_classes <= 1024, "mp_detector_create: n_classes %d", cfg->n_classes);
  MP_REQUIRE(cfg->rpn_pre_nms_top_n >= 1 && cfg->rpn_pre_nms_top_n <= DET_MAX_SEG && cfg->rpn_post_nms_top_n >= 1 &&
                 cfg->rpn_post_nms_top_n <= DET_MAX_SEG && cfg->box_detections_per_img >= 1 && cfg->box_detections_per_img <= DET_MAX_SEG,
             "mp_detector_create: top-n sizes must lie in [1, %d]", DET_MAX_SEG);
  for (int k = 0; k < 3; ++k) MP_REQUIRE(cfg->image_std[k] > 0.f && cfg->aspect_ratios[k] > 0.f, "mp_detector_create: bad std / aspect ratio");
  StateMap sm;
  for (int i = 0; i < n_tensors; ++i) sm[st[i].name] = std::make_pair(st[i].h_data, st[i].numel);
  mp_detector* d = new mp_detector();
  d->cfg = *cfg;
  CreateSink k{d->allocs, sm};
  const int rc = det_walk(cfg->n_classes, d->net, k);
  if (rc) {   // a missing or mis-sized tensor (find has set the message), or a layer that could not be built
    mp_detector_destroy(d);
    return rc;
  }
  // anchor_utils.py generate_anchors: h_ratios = sqrt(ar), w_ratios = 1 / h_ratios, base = round([-w, -h, w, h] / 2) (float32, half to even)
  for (int l = 0; l < DET_LEVELS; ++l)
    for (int a = 0; a < DET_A; ++a) {
      const float hr = sqrtf(cfg->aspect_ratios[a]), wr = 1.0f / hr;
      const float ws = wr * (float)cfg->anchor_sizes[l], hs = hr * (float)cfg->anchor_sizes[l];
      d->base_anchors[l][a][0] = nearbyintf(-ws / 2.f);
      d->base_anchors[l][a][1] = nearbyintf(-hs / 2.f);
      d->base_anchors[l][a][2] = nearbyintf(ws / 2.f);
      d->base_anchors[l][a][3] = nearbyintf(hs / 2.f);
    }
  *out = d;
  return MP_OK;
}

extern "C" size_t mp_detector_workspace_bytes(const mp_detector* d, int n_images, int H, int W) {
  if (!d || n_images <= 0 || H <= 0 || W <= 0) return 0;
  DetPlan p;
  if (det_make_plan(d->cfg, n_images, H, W, &p)) return 0;
  return p.total * sizeof(float);
}

extern "C" int mp_detector_forward(mp_detector* d, const float* d_images, int n, int H, int W, float* d_boxes, float* d_scores, int32_t* d_labels,
                                   int32_t* d_counts, float* d_masks, void* d_ws, size_t ws_bytes, mp_stream stream) {
  MP_REQUIRE(d && d_images && d_boxes && d_scores && d_labels && d_counts && d_ws, "mp_detector_forward: null pointer");
  MP_REQUIRE(n > 0 && n <= 4096 && H > 0 && W > 0, "mp_detector_forward: bad size");
  const mp_detector_config& cfg = d->cfg;
  const DetLayers& net = d->net;
  const int C = cfg.n_classes, R = cfg.rpn_post_nms_top_n, Kp = cfg.rpn_pre_nms_top_n, D = cfg.box_detections_per_img;
  DetPlan p;
  const int plan_rc = det_make_plan(cfg, n, H, W, &p);
  if (plan_rc) return plan_rc;
  MP_REQUIRE(ws_bytes >= p.total * sizeof(float), "mp_detector_forward: workspace %zu < %zu bytes", ws_bytes, p.total * sizeof(float));
  MP_REQUIRE((long)n * p.a_total < (1L << 31) && (long)n * (C - 1) * R < (1L << 31),
             "mp_detector_forward: %d images of %d anchors exceed the 32-bit index range of the selection kernels; split the batch", n, p.a_total);
  // The selection kernels rank by counting (O(len^2) compares per segment: deterministic, no library sort).  That is ~3e9 compares for
  // the 57.6 k P2 anchors of a 480x640 frame (1.5 ms) but grows quadratically: bound the segment sizes instead of degrading silently
  // (torchvision's default 800x1333 transform gives ~200 k anchors on P2 = 4e10 compares per frame -- use a radix select there).
  MP_REQUIRE((long)p.hr * p.wr <= 1024L * 1024L && C <= 256,
             "mp_detector_forward: resized frame %dx%d / %d classes exceed what the rank-sort selection is sized for (<= 1024x1024, <= 256 classes)",
             p.hr, p.wr, C);
  hipStream_t s = (hipStream_t)stream;
  float* ws = (float*)d_ws;
  auto F = [&](const DetBuf& b) { return ws + b.off; };
  auto I = [&](const DetBuf& b) { return reinterpret_cast<int*>(ws + b.off); };
  auto B4 = [&](const DetBuf& b) { return reinterpret_cast<float4*>(ws + b.off); };
  // zero everything: borders of every padded map, the pad region of the batched input, counters (cheap next to ResNet-50)
  MP_CHECK_HIP(hipMemsetAsync(d_ws, 0, p.total * sizeof(float), s));
  DetRun r{s, F(p.splitk), n};

  // ---- transform + backbone + FPN --------------------------------------------------------------------------------------------
  {
    ProfScope prof("det_preprocess", 0.0, (double)n * (12.0 * H * W + 16.0 * p.hr * p.wr), s);
    hipLaunchKernelGGL(det_preprocess_kernel, dim3(ceil_div((long)p.hr * p.wr, 256), n), dim3(256), 0, s, d_images, H, W, p.hr, p.wr, p.ratio_h,
                       p.ratio_w, cfg.image_mean[0], cfg.image_mean[1], cfg.image_mean[2], cfg.image_std[0], cfg.image_std[1], cfg.image_std[2],
                       F(p.x0), p.Hp, p.Wp, 3);
  }
  r.conv(net.stem, F(p.x0), n, p.Hp, p.Wp, 3, F(p.stem), 1, nullptr, 1);
  if (!r.rc) r.rc = mp_maxpool3x3s2(F(p.stem), n, p.Hp / 2, p.Wp / 2, 64, 1, F(p.pool), 1, nullptr, nullptr, nullptr, s);
  const float* x = F(p.pool);
  int xh = p.Hp / 4, xw = p.Wp / 4;
  const float* stage_out[4];
  for (int st = 0; st < 4; ++st) {
    const DetStage& S = p.stage[st];
    const int oh = p.fh[st], ow = p.fw[st];
    int cur = 1;   // the first block writes x[0]
    for (int bi = 0; bi < RES_BLOCKS[st]; ++bi) {
      const Bottleneck& b = net.block[st][bi];
      const bool first = bi == 0;   // takes the previous stage's map (stride 2 from stage 1 on) and has the downsample branch
      float* t1 = F(first ? S.t1in : S.t1);
      r.conv(b.c1, x, n, xh, xw, 1, t1, 1, nullptr, 1);
      r.conv(b.c2, t1, n, xh, xw, 1, F(S.t2), 1, nullptr, 1);
      const float* idn = x;
      if (first) {
        r.conv(b.down, x, n, xh, xw, 1, F(S.d), 1, nullptr, 0);
        idn = F(S.d);
      }
      cur ^= 1;
      float* y = F(S.x[cur]);
      r.conv(b.c3, F(S.t2), n, oh, ow, 1, y, 1, idn, 1);
      x = y; xh = oh; xw = ow;
    }
    stage_out[st] = x;
    p.stage_buf[st] = cur;
  }
  if (r.rc) return r.rc;
  // FPN (ops/feature_pyramid_network.py): last_inner = inner[3](C5); P5 = layer[3](last_inner); going down: lateral + nearest upsample
  r.conv(net.fpn_inner[3], stage_out[3], n, p.fh[3], p.fw[3], 1, F(p.L[3]), 1, nullptr, 0);
  r.conv(net.fpn_layer[3], F(p.L[3]), n, p.fh[3], p.fw[3], 1, F(p.P[3]), 1, nullptr, 0);
  for (int l = 2; l >= 0 && !r.rc; --l) {
    {
      const long total = (long)n * p.fh[l] * p.fw[l] * (DET_FPN_C / 4);
      ProfScope prof("det_resize_nearest", 0.0, (double)total * 32.0, s);
      hipLaunchKernelGGL(det_resize_nearest_kernel, dim3(ceil_div(total, 256)), dim3(256), 0, s, F(p.L[l + 1]), p.fh[l + 1], p.fw[l + 1], F(p.U[l]),
                         p.fh[l], p.fw[l], DET_FPN_C, n, 1, 1, 0, 0);
    }
    r.conv(net.fpn_inner[l], stage_out[l], n, p.fh[l], p.fw[l], 1, F(p.L[l]), 1, F(p.U[l]), 0);
    r.conv(net.fpn_layer[l], F(p.L[l]), n, p.fh[l], p.fw[l], 1, F(p.P[l]), 1, nullptr, 0);
  }
  if (r.rc) return r.rc;
  {  // LastLevelMaxPool: F.max_pool2d(P5, 1, 2, 0)
    const long total = (long)n * p.fh[4] * p.fw[4] * (DET_FPN_C / 4);
    hipLaunchKernelGGL(det_resize_nearest_kernel, dim3(ceil_div(total, 256)), dim3(256), 0, s, F(p.P[3]), p.fh[3], p.fw[3], F(p.P[4]), p.fh[4], p.fw[4],
                       DET_FPN_C, n, 1, 1, 2, 2);
  }

  // ---- RPN (models/detection/rpn.py) --------------------------------------------------------------------------------------------
  RpnLevels L;
  L.off[0] = 0;
  for (int l = 0; l < DET_LEVELS; ++l) {
    r.conv(net.rpn_conv, F(p.P[l]), n, p.fh[l], p.fw[l], 1, F(p.rpn_t[l]), 0, nullptr, 1);
    r.conv(net.rpn_head, F(p.rpn_t[l]), n, p.fh[l], p.fw[l], 0, F(p.rpn_h[l]), 0, nullptr, 0);
    L.head[l] = F(p.rpn_h[l]);
    L.gh[l] = p.fh[l]; L.gw[l] = p.fw[l];
    L.off[l + 1] = L.off[l] + p.fh[l] * p.fw[l] * DET_A;
    L.stride_y[l] = p.Hp / p.fh[l];   // anchor_utils.py: strides = image_size // grid_size (padded batch size)
    L.stride_x[l] = p.Wp / p.fw[l];
    memcpy(L.base[l], d->base_anchors[l], sizeof(L.base[l]));
  }
  if (r.rc) return r.rc;
  {
    const long total = (long)n * p.a_total;
    hipLaunchKernelGGL(det_rpn_keys_kernel, dim3(ceil_div(total, 256)), dim3(256), 0, s, L, n, F(p.keys));
  }
  int max_len = 0;
  for (int l = 0; l < DET_LEVELS; ++l) max_len = std::max(max_len, L.off[l + 1] - L.off[l]);
  hipLaunchKernelGGL(det_rpn_seg_offsets_kernel, dim3(ceil_div((long)n * DET_LEVELS + 1, 256)), dim3(256), 0, s, L, n, I(p.seg_off));
  {
    ProfScope prof("det_rank_topk", 0.0, 0.0, s);
    hipLaunchKernelGGL(det_rank_topk_kernel, dim3(ceil_div(max_len, 256), n * DET_LEVELS), dim3(256), 0, s, F(p.keys), I(p.seg_off), Kp, I(p.idx1),
                       I(p.cnt1));
  }
  {
    const long total = (long)n * DET_LEVELS * Kp;
    hipLaunchKernelGGL(det_rpn_gather_kernel, dim3(ceil_div(total, 256)), dim3(256), 0, s, L, n, F(p.keys), I(p.idx1), I(p.cnt1), Kp, (float)p.hr,
                       (float)p.wr, cfg.rpn_min_size, cfg.rpn_score_thresh, B4(p.cand_box), F(p.cand_score), I(p.cand_keep));
    ProfScope prof("det_nms", 0.0, 0.0, s);
    hipLaunchKernelGGL(det_nms_kernel, dim3(n * DET_LEVELS), dim3(256), 0, s, B4(p.cand_box), I(p.cand_keep), (const int*)nullptr, Kp,
                       cfg.rpn_nms_thresh);
    hipLaunchKernelGGL(det_masked_keys_kernel, dim3(ceil_div(total, 256)), dim3(256), 0, s, F(p.cand_score), I(p.cand_keep), total, F(p.keys2));
  }
  r.rank_topk(F(p.keys2), 1, DET_LEVELS * Kp, R, I(p.seg_off2), I(p.idx2), I(p.proposal_counts));
  hipLaunchKernelGGL(det_gather_boxes_kernel, dim3(ceil_div((long)n * R, 256)), dim3(256), 0, s, B4(p.cand_box), F(p.cand_score), DET_LEVELS * Kp,
                     I(p.idx2), I(p.proposal_counts), R, n, B4(p.proposals), F(p.proposal_scores));
  hipLaunchKernelGGL(det_clamp_counts_kernel, dim3(ceil_div(n, 256)), dim3(256), 0, s, I(p.proposal_counts), n, R);

  // ---- box head (roi_heads.py) ----------------------------------------------------------------------------------------------------
  PyramidRef py;
  for (int l = 0; l < 4; ++l) { py.feat[l] = F(p.P[l]); py.h[l] = p.fh[l]; py.w[l] = p.fw[l]; }
  {
    const long total = (long)n * R * 49 * (DET_FPN_C / 4);
    ProfScope prof("det_roi_align", 0.0, (double)total * 16.0 * 5.0, s);
    hipLaunchKernelGGL(det_roi_align_kernel, dim3(ceil_div(total, 256)), dim3(256), 0, s, py, B4(p.proposals), I(p.proposal_counts), R, n, 7, 0,
                       F(p.roi7));
  }
  r.conv(net.fc6, F(p.roi7), n * R, 1, 1, 0, F(p.fc6), 0, nullptr, 1);
  r.conv(net.fc7, F(p.fc6), n * R, 1, 1, 0, F(p.fc7), 0, nullptr, 1);
  r.conv(net.pred, F(p.fc7), n * R, 1, 1, 0, F(p.class_logits), 0, nullptr, 0);
  if (r.rc) return r.rc;
  hipLaunchKernelGGL(det_box_post_kernel, dim3(ceil_div((long)n * R, 256)), dim3(256), 0, s, F(p.class_logits), pad4(5 * C), C, B4(p.proposals),
                     I(p.proposal_counts), R, n, (float)p.hr, (float)p.wr, cfg.box_score_thresh, cfg.box_min_size, B4(p.c2_box), F(p.c2_key));
  const int n_seg2 = n * (C - 1);
  // (seg_off is free again: the RPN sort that used it was enqueued earlier on the same stream)
  r.rank_topk(F(p.c2_key), C - 1, R, R, I(p.seg_off), I(p.c2_idx), I(p.c2_cnt));
  {
    const long total = (long)n_seg2 * R;
    hipLaunchKernelGGL(det_sorted_gather_kernel, dim3(ceil_div(total, 256)), dim3(256), 0, s, B4(p.c2_box), F(p.c2_key), I(p.c2_idx), I(p.c2_cnt), R,
                       total, B4(p.c2_sbox), F(p.c2_skey), I(p.c2_keep), I(p.c2_inv));
    hipLaunchKernelGGL(det_nms_kernel, dim3(n_seg2), dim3(256), 0, s, B4(p.c2_sbox), I(p.c2_keep), I(p.c2_cnt), R, cfg.box_nms_thresh);
    hipLaunchKernelGGL(det_final_keys_kernel, dim3(ceil_div(total, 256)), dim3(256), 0, s, F(p.c2_key), I(p.c2_keep), I(p.c2_inv), C - 1, R, total,
                       F(p.c2_fkey));
  }
  r.rank_topk(F(p.c2_fkey), 1, (C - 1) * R, D, I(p.seg_off3), I(p.f_idx), I(p.f_cnt));
  hipLaunchKernelGGL(det_final_kernel, dim3(ceil_div((long)n * D, 256)), dim3(256), 0, s, B4(p.c2_box), F(p.c2_key), I(p.f_idx), I(p.f_cnt), D, C - 1,
                     R, n, p.ratio_h, p.ratio_w, reinterpret_cast<float4*>(d_boxes), d_scores, d_labels, d_counts, B4(p.det_resized));

  // ---- mask head --------------------------------------------------------------------------------------------------------------------
  if (d_masks) {
    {
      const long total = (long)n * D * 196 * (DET_FPN_C / 4);
      hipLaunchKernelGGL(det_roi_align_kernel, dim3(ceil_div(total, 256)), dim3(256), 0, s, py, B4(p.det_resized), d_counts, D, n, 14, 1, F(p.roi14));
    }
    const float* mx = F(p.roi14);
    for (int i = 0; i < 4; ++i) {
      float* my = F((i & 1) ? p.m_b : p.m_a);
      r.conv(net.mask_fcn[i], mx, n * D, 14, 14, 1, my, 1, nullptr, 1);
      mx = my;
    }
    r.conv(net.mask_deconv, mx, n * D, 14, 14, 1, F(p.m_up), 0, nullptr, 1);
    r.conv(net.mask_logits, F(p.m_up), n * D * 196 * 4, 1, 1, 0, F(p.mask_logits), 0, nullptr, 0);
    if (r.rc) return r.rc;
    ProfScope prof("det_mask_paste", 0.0, (double)n * D * H * W * 4.0, s);
    hipLaunchKernelGGL(det_mask_paste_kernel, dim3(ceil_div((long)H * W, 256), n * D), dim3(256), 0, s, F(p.mask_logits), pad4(C),
                       reinterpret_cast<const float4*>(d_boxes), d_labels, d_counts, D, H, W, d_masks);
  }
  MP_CHECK_HIP(hipGetLastError());
  d->ran = true;
  d->last = p;
  d->last_ws = d_ws;
  return MP_OK;
}

extern "C" int mp_detector_debug_tensor(const mp_detector* d, const char* what, const void** d_ptr, int64_t* shape4, int32_t* border,
                                        int64_t* row_stride, int64_t* n_elements) {
  MP_REQUIRE(d && what && d_ptr && shape4 && border && row_stride && n_elements, "mp_detector_debug_tensor: null pointer");
  MP_REQUIRE(d->ran, "mp_detector_debug_tensor: no forward has run yet");
  const DetBuf* b = det_find_tap(d->last, what);
  MP_REQUIRE(b, "mp_detector_debug_tensor: '%s' is not a published tensor (unknown, or an internal buffer)", what);
  *d_ptr = (const float*)d->last_ws + b->off;
  for (int k = 0; k < 4; ++k) shape4[k] = b->shape[k];
  *border = b->border;
  *row_stride = b->row_stride;
  *n_elements = b->n_elements;
  return MP_OK;
}
