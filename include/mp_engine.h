/* mp_engine.h -- C-ABI of the MI355X-native render-and-compare pose engine.
 *
 * This is the drop-in boundary for the reference's hot path.
 * The reference (megapose6d) is pure Python and has no FFI layer; the seam is three
 * duck-typed Python objects.  Each entry point below names the reference interface it
 * replaces (paths relative to /root/reference/src/megapose/).  INTEGRATION.md shows the
 * ctypes binding a reference maintainer would add.
 *
 * Conventions
 *  - plain C, no torch types; every pointer named d_* is DEVICE memory (HBM), h_* is HOST.
 *  - mp_stream is a hipStream_t; all work is enqueued on it, nothing synchronises.
 *  - return value: 0 = ok, negative = error (message via mp_last_error()).
 *  - handles are opaque, thread-compatible (one thread per handle at a time).
 *  - outputs are caller-allocated.
 *  - images/activations inside the engine are fp32 NHWC with a zero border ("padded NHWC"):
 *    element (n, y, x, c) of a tensor with logical size H x W, border B, channels C lives at
 *    ((n*(H+2B) + y+B)*(W+2B) + x+B)*C + c.  Borders are zero and never written.
 */
#ifndef MP_ENGINE_H
#define MP_ENGINE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* mp_stream; /* hipStream_t */

#define MP_OK 0
#define MP_ERR_INVALID (-22)
#define MP_ERR_NOMEM (-12)
#define MP_ERR_HIP (-5)

int mp_version(void);
const char* mp_last_error(void);
/* Per-launch HIP-event profiler: between begin/end every instrumented kernel launch is bracketed by hipEvents recorded on
 * its launch stream.  mp_profile_query_ex aggregates by kernel name (idx enumerates the distinct names): number of launches, summed
 * duration (ms), and the summed ALGORITHMIC flops / bytes of those launches (DESIGN.md states each kernel's per-unit figures).  Returns 1
 * past the end. */
int mp_profile_begin(void);
int mp_profile_end(void);
int mp_profile_active(void); /* 1 between begin and end */
/* Besides those, the FLOPs the launches EXECUTED on the matrix pipe (= the algorithmic figure for the direct kernels; 16/36 of it for the
 * fp32 Winograd kernel; 9 bf16 piece products per Winograd multiplication / 3 or 9 per stem multiplication for the exact-piece kernels)
 * and the dense peak (TFLOP/s) of the pipe they run on (157.3 fp32 MFMA, 2500 bf16 MFMA): executed / time / peak = MFMA utilisation.
 * Every output pointer may be NULL. */
int mp_profile_query_ex(int idx, char* name, int name_len, int64_t* launches, double* total_ms, double* total_flops,
                        double* total_bytes, double* total_executed_flops, double* peak_tflops);



/* number of CUs etc. of the current device; fails loudly when no gfx950 device is usable */
int mp_device_info(int* n_cus, int* lds_bytes, char* arch_name, int arch_name_len);

/* ------------------------------------------------------------------------------------ */
/* Mesh database: replaces the per-worker Panda3D model cache                            */
/* (panda3d_renderer/panda3d_scene_renderer.py:192-207 get_object_node) and the          */
/* BatchedMeshes point tensors (lib3d/rigid_mesh_database.py:90-130).                     */
/* ------------------------------------------------------------------------------------ */
typedef struct mp_mesh_db mp_mesh_db;

typedef struct {
  const float* h_vertices; /* [n_vertices,3] metres (RigidObject.scale and ypr offset applied) */
  const float* h_normals;  /* [n_vertices,3] unit vertex normals (object frame)                */
  const float* h_colors;   /* [n_vertices,3] albedo in [0,1] (uint8/255)                       */
  const int32_t* h_faces;  /* [n_faces,3]                                                      */
  int32_t n_vertices;
  int32_t n_faces;
} mp_mesh_desc;

int mp_mesh_db_create(const mp_mesh_desc* h_meshes, int n_meshes, mp_mesh_db** out);
/* UV texture of mesh `mesh_id` (replaces Panda3D's assimp/texture loading, panda3d_scene_renderer.py:192-207: the albedo of a
 * textured RigidObject): h_uvs = per-corner (u,v) [n_faces][3][2] float32 in the corner order of h_faces (v = 0 at the FIRST
 * texel row passed here, i.e. the host flips image rows so that v grows with the row index); h_texels = RGBA8 mip chain, level l
 * of size max(1,w>>l) x max(1,h>>l), levels concatenated (built on the host: megapose6d_amd.mesh_io.build_mip_chain).
 * Sampling: repeat wrap, trilinear (bilinear taps in the two mip levels around a per-pixel level of detail derived from the
 * analytic screen-space uv derivatives; texture-minfilter mipmap, panda3d_scene_renderer.py:71); albedo = vertex colour x
 * texel / 255.  16x anisotropic filtering (:72) is not reproduced. */
#define MP_TEX_MAX_LEVELS 15
int mp_mesh_db_set_texture(mp_mesh_db* db, int mesh_id, const float* h_uvs, const uint32_t* h_texels, int tex_w, int tex_h,
                           int n_levels);
int mp_mesh_db_destroy(mp_mesh_db* db);
int mp_mesh_db_max_vertices(const mp_mesh_db* db);
/* bounding-sphere radius (AABB centre) of mesh i, used for the point-light placement
 * (panda3d_scene_renderer.py:121-125 pos_fn) */
float mp_mesh_db_radius(const mp_mesh_db* db, int mesh_id);

/* ------------------------------------------------------------------------------------ */
/* Rasteriser: replaces Panda3dBatchRenderer.render                                       */
/* (panda3d_renderer/panda3d_batch_renderer.py:217-282; worker_loop :89-150;              */
/*  Panda3dSceneRenderer.render_scene panda3d_scene_renderer.py:298-358).                 */
/* One object per view, pinhole K, near 0.1 m / far 10 m (types.py:63-64).                */
/* ------------------------------------------------------------------------------------ */
#define MP_RASTER_NORMALS 1u      /* render_normals=True: eye-normal LUT pass               */
#define MP_RASTER_DEPTH 2u        /* render_depth=True: metric z, 0 = background            */
#define MP_RASTER_NORMALS_GL 4u   /* eye space = GL (x right,y up,z back) instead of Panda  */
#define MP_RASTER_MSAA4 16u        /* 4x multisampling (the reference's configuration: framebuffer-multisample 1,
                                     multisamples 4, panda3d_scene_renderer.py:73-74): coverage and depth per sample of the
                                     standard 4-sample pattern, shading once per (pixel, piece) at the pixel centre, 8-bit
                                     per-sample colours averaged; without the flag: one sample at the pixel centre          */

#define MP_RASTER_F16 32u          /* "fp16 renders" (BASELINE.json configs[4]; the reference's output path, panda3d_batch_renderer.py:
                                     261-274, converts uint8 -> fp32): d_out points at IEEE binary16 elements instead of floats --
                                     same ELEMENT strides and channel numbers, every written channel (renders and, with
                                     mp_raster_render_crop, the observation crop) rounded to nearest-even.  The consumer is
                                     mp_backbone_forward_f16 / mp_conv_desc.x_f16.                                              */

#define MP_RASTER_XREC 64u         /* d_out points at the bf16 pixel RECORDS of the exact-piece stem convolution (mp_conv_stem_xrec):
                                     [x1,x2,x3 of every crop channel | the 8-bit integer k of every render channel (NOT divided by 255) |
                                     zero padding], mp_xrec_elements(C_crop, n_render_channels) elements per pixel.  mp_raster_render_crop
                                     (c0_crop = 0, no depth channel, one launch writes every channel of the record) or, with depth channels,
                                     mp_raster_render_xrec; stride_v /
                                     stride_y / stride_x count bf16 elements (stride_x = the record length), c_rgb / c_normals /
                                     stride_view stay logical channel numbers.  The values are the ones the fp32 output holds: k = the
                                     integer whose k / 255 the fp32 path stores, x1 + x2 + x3 = the fp32 crop value exactly.            */

typedef struct {
  float ambient[3];        /* sum of ambient light colours                                  */
  int32_t n_point;         /* number of point lights (<= 8)                                 */
  float point_dir[8][3];   /* light position (object frame) = dir * 10 * mesh radius + offset: the affine-in-the-radius  */
  float point_color[8][3]; /* form of Panda3dLightData.positioning_function (panda3d_scene_renderer.py:104-136,         */
  float point_offset[8][3];/* types.py:104-114); make_scene_lights: dir = +-axes, offset = 0                            */
} mp_lights;

/* scratch for the per-view tile lists of a launch of n_views views at h x w (<= 1024 x 1024) */
size_t mp_raster_workspace_bytes(const mp_mesh_db* db, int n_views, int h, int w);

/* d_out addressing: element (view v, y, x, channel c) at
 *   d_out[(v / views_per_item)*stride_v + (v % views_per_item)*stride_view + y*stride_y + x*stride_x + c]
 * (views_per_item = 1, stride_view = 0 for a plain batch; = n_rendered_views / channels-per-view when the views of
 * one hypothesis are folded into the channels of one CNN input row, models/pose_rigid.py:405-408).
 * c_rgb / c_normals / c_depth are the first channel of each group (negative = not written).
 * Values are uint8-quantised then /255 exactly as panda3d_batch_renderer.py:261-274
 * (depth is not quantised).  Non-finite TCO/K rows produce zeros (:109-135).  Triangles crossing the near plane are
 * clipped.  One launch writes at most 32 consecutive channels per pixel (c_lo .. c_hi over all groups / views / the crop),
 * and stride_x must be >= that run.                                                        */
int mp_raster_render(const mp_mesh_db* db, const int32_t* d_mesh_ids, const float* d_TCO /*[n,4,4]*/,
                     const float* d_K /*[n,3,3]*/, int n_views, int h, int w, uint32_t flags,
                     const mp_lights* h_lights, float* d_out, int64_t stride_v, int views_per_item,
                     int64_t stride_view, int64_t stride_y, int64_t stride_x, int c_rgb, int c_normals,
                     int c_depth, void* d_workspace, size_t workspace_bytes, mp_stream stream);

/* mp_raster_render + the observation crop of every item (mp_crop_roi_align semantics, boxes / im_ids per ITEM = n_views /
 * views_per_item) written by the same launch into channels c0_crop.. of the item's pixels: what PosePredictor.forward does per
 * iteration with crop_inputs (models/pose_rigid.py:180-247) + render_images_multiview (:336-408) + torch.cat (:567).  The wave
 * that rasterises an 8x8-pixel tile of the item's views also computes the roi_align of those pixels, so every pixel of the CNN
 * input leaves the chip once, as one contiguous record of all its channels. */
int mp_raster_render_crop(const mp_mesh_db* db, const int32_t* d_mesh_ids, const float* d_TCO, const float* d_K, int n_views,
                          int h, int w, uint32_t flags, const mp_lights* lights, float* d_out, int64_t stride_v,
                          int views_per_item, int64_t stride_view, int64_t stride_y, int64_t stride_x, int c_rgb,
                          int c_normals, int c_depth, void* d_workspace, size_t workspace_bytes,
                          const float* d_images /*[n_im,C,H,W], or [n_im,H,W,4] if images_nhwc4*/, int images_nhwc4, int n_im,
                          int C, int H, int W, const int32_t* d_im_ids, const float* d_boxes, int c0_crop, mp_stream stream);
/* The record form of that launch for models WITH depth channels (the RGBD refiner, training/pose_models_cfg.py:101-103: observation depth
 * + one rendered depth per view; BASELINE.json configs[2]): MP_RASTER_XREC is implied, d_out = bf16 records of
 * mp_xrec_elements(popcount(f32_mask), n_channels - popcount(f32_mask)) elements.  Bit c of f32_mask marks logical channel c as fp32-kind
 * (three exact bf16 pieces): the crop's channels and every depth channel must be marked, the rgb / normal channels must not.  Depth
 * channels -- the 4th crop channel and c_depth of every view -- are normalised BEFORE the split exactly as mp_normalize_depth does it on the
 * fp32 tensor (models/pose_rigid.py:466-496; depth_mode 0..3, d_tCR [n_items,3]: the row's object-centre translation, z = reference depth;
 * background depth 0 is normalised like any other value), so the record decodes to the fp32 tensor path's values bit for bit. */
int mp_raster_render_xrec(const mp_mesh_db* db, const int32_t* d_mesh_ids, const float* d_TCO, const float* d_K, int n_views,
                          int h, int w, uint32_t flags, const mp_lights* lights, void* d_out_records, int64_t stride_v,
                          int views_per_item, int64_t stride_view, int64_t stride_y, int64_t stride_x, int c_rgb,
                          int c_normals, int c_depth, void* d_workspace, size_t workspace_bytes,
                          const float* d_images, int images_nhwc4, int n_im, int C, int H, int W, const int32_t* d_im_ids,
                          const float* d_boxes, uint32_t f32_mask, const float* d_tCR, int depth_mode, mp_stream stream);
/* The job flags of the LAST mp_raster_render* launch on `d_workspace`: NULL unless that launch ran in the compacted form (default;
 * MP_RASTER_COMPACT=0 = direct form) with exactly this n_views, h and w (the library keeps a host-side record per workspace, so stale
 * or foreign bytes are never handed out); else the device pointer to [n_items][tiles_y = ceil(h / 8)][tiles_x = ceil(w / 8)] bytes, 0 = no
 * view of the item reaches that 8x8-pixel tile (its render channels are all background).  Consumer: mp_conv_stem_xrec_sparse /
 * mp_backbone_forward_xrec_sparse on the same stream, before the next raster launch on this workspace. */
const unsigned char* mp_raster_job_flags(const mp_mesh_db* db, const void* d_workspace, int n_views, int h, int w);
/* observation frames [n_im,C,H,W] (C = 3 | 4) -> [n_im,H,W,4] (4th channel 0 for RGB): one 16-byte load per roi_align tap in the
 * fused crop; done once per observation, not per step */
int mp_pack_observation_nhwc4(const float* d_images, int n_im, int C, int H, int W, float* d_out, mp_stream stream);

/* ------------------------------------------------------------------------------------ */
/* Scene rasteriser: replaces Panda3dSceneRenderer.render_scene                           */
/* (panda3d_renderer/panda3d_scene_renderer.py:298-358, setup_scene :218-236,             */
/*  render_images :255-272, binary mask :329-335; CameraRenderingData types.py:43-55).    */
/* Several objects per camera image, depth-tested against each other.                     */
/* ------------------------------------------------------------------------------------ */
/* scratch of one mp_raster_render_scene launch with n_objects objects in all (summed over the cameras) at h x w */
size_t mp_raster_scene_workspace_bytes(const mp_mesh_db* db, int n_objects, int h, int w);

/* Render n_cams cameras; camera c owns the objects [obj_off[c], obj_off[c+1]) (h_obj_off: the same n_cams + 1 offsets on the HOST, for
 * validation and sizing; obj_off[0] = 0).  Per object o: mesh d_mesh_ids[o], camera-from-object pose d_TCO[o] (float32 [4,4]) and light
 * rig d_lights[o] (DEVICE array of mp_lights, given in the object's frame: point light l sits at point_dir[l] * 10 * scene radius +
 * point_offset[l]).  Per camera: d_K[c] ([3,3]) and the scene radius d_radius[c], which replaces the mesh radius in that formula.
 * Output addressing and values as mp_raster_render with views_per_item = 1: element (camera c, y, x, channel k) at
 * d_out[c*stride_v + y*stride_y + x*stride_x + k], fp32 only (flags: MP_RASTER_NORMALS / _DEPTH / _NORMALS_GL / _MSAA4).
 * d_instance (optional, int32 [n_cams][h][w]): the slot, relative to the camera's first object, of the object that owns sample 0 of the
 * pixel (the sample whose depth the depth channel reports); -1 = background.
 * Contract: per sample, the coverage and depth rules of mp_raster_render applied to the pieces of ALL objects of the camera, the nearest
 * piece wins; on exactly equal depth the object listed first wins (draw order under a less-than depth test), within one object the lower
 * piece id.  Shading once per (pixel, winning piece) with that object's mesh, texture, pose and light rig; 4-sample 8-bit resolve; depth
 * = metric z of sample 0, 0 for background.  An object with a non-finite pose contributes nothing; a camera with a non-finite K or with
 * no object renders background.  At most 256 objects per camera, h, w <= 1024. */
int mp_raster_render_scene(const mp_mesh_db* db, int n_cams, const int32_t* h_obj_off, const int32_t* d_obj_off,
                           const int32_t* d_mesh_ids, const float* d_TCO, const float* d_K, const float* d_radius,
                           const mp_lights* d_lights, int h, int w, uint32_t flags, float* d_out, int64_t stride_v, int64_t stride_y,
                           int64_t stride_x, int c_rgb, int c_normals, int c_depth, int32_t* d_instance, void* d_workspace,
                           size_t workspace_bytes, mp_stream stream);

/* ------------------------------------------------------------------------------------ */
/* Crop: replaces lib3d/cropping.py:113-144 crop_images (torchvision.ops.roi_align,       */
/* sampling_ratio=4, aligned=False) incl. the RGBD validity rule (:131-142), reading the  */
/* observation by batch_im_id (no per-row gather, pose_estimator.py:389).                 */
/* C is 3 or 4; 0 <= b <= 65535 (one grid row per box; b = 0 launches nothing), anything  */
/* else is MP_ERR_INVALID, nothing launched.  d_im_ids are NOT range-checked: every id    */
/* must lie in [0, n_im) and every box must be finite.                                    */
/* ------------------------------------------------------------------------------------ */
int mp_crop_roi_align(const float* d_images /*[n_im,C,H,W] NCHW*/, int n_im, int C, int H, int W,
                      const int32_t* d_im_ids /*[b]*/, const float* d_boxes /*[b,4] x1,y1,x2,y2*/, int b,
                      int out_h, int out_w, float* d_out, int64_t stride_b, int64_t stride_y,
                      int64_t stride_x, int c0, mp_stream stream);

/* ------------------------------------------------------------------------------------ */
/* Depth normalisation: models/pose_rigid.py:466-496 normalize_depth                      */
/* mode: 0 none, 1 tCR_scale, 2 tCR_scale_clamp_center, 3 tCR_center_clamp                */
/* applied in place to `n_ch` channels (list h_channels) of a padded-NHWC tensor.         */
/* ------------------------------------------------------------------------------------ */
int mp_normalize_depth(float* d_x, int b, int h, int w, int border, int C, const int32_t* h_channels,
                       int n_ch, const float* d_tCR /*[b,3]*/, int mode, mp_stream stream);
/* the same on a half-precision padded-NHWC tensor (MP_RASTER_F16 output): read, normalise in fp32, round back to binary16 */
int mp_normalize_depth_f16(void* d_x_half, int b, int h, int w, int border, int C, const int32_t* h_channels,
                           int n_ch, const float* d_tCR /*[b,3]*/, int mode, mp_stream stream);

/* ------------------------------------------------------------------------------------ */
/* Convolution stack: replaces `self.backbone(x)` (models/pose_rigid.py:323) for           */
/* models/torchvision_resnet.py (vanilla_resnet34) and models/wide_resnet.py               */
/* (WideResNet18/34).  fp32 in, fp32 MFMA (v_mfma_f32_32x32x2_f32), fp32 out.             */
/* ------------------------------------------------------------------------------------ */
/* number of floats of the packed weight blob of one conv (Cin_p = padded input channels) */
size_t mp_conv_packed_floats(int Cin_p, int Cout, int KH, int KW);
/* host-side packing of OIHW weights with per-output-channel scale folded in (eval BN).    */
int mp_conv_pack_weights(const float* h_w_oihw, int Cout, int Cin, int KH, int KW, int Cin_p,
                         const float* h_scale /*[Cout] or NULL*/, float* h_packed);

typedef struct {
  const float* d_x;        /* padded NHWC input                                             */
  int32_t N, H, W, C;      /* logical input size; C = padded channel count (multiple of 4)   */
  int32_t in_border;
  const float* d_w;        /* packed weights (mp_conv_pack_weights)                          */
  const float* d_bias;     /* [Cout] or NULL                                                 */
  int32_t Cout, KH, KW, stride, pad;
  float* d_y;              /* padded NHWC output (may be NULL when only d_y_act is wanted)   */
  int32_t out_border;
  const float* d_residual; /* same geometry as d_y, or NULL                                  */
  int32_t relu;            /* y = relu(conv + bias + residual)                               */
  float* d_y_act;          /* optional second output relu(y*act_scale + act_shift)           */
  const float* d_act_scale;
  const float* d_act_shift;
  int32_t c_real;          /* real (unpadded) input channels, for the profiler's algorithmic FLOP count; 0 = C   */
  float* d_splitk_ws;      /* optional scratch: with it, launches whose tile grid cannot fill the chip (small batches) split  */
  int64_t splitk_ws_floats;/* the K loop over several workgroups and reduce deterministically (fixed order); NULL = never    */
  int32_t x_f16;           /* != 0: d_x holds IEEE binary16 values in the same padded-NHWC geometry (what MP_RASTER_F16 writes);    */
                           /* the kernel widens them to fp32 on the way into LDS, arithmetic and outputs stay fp32.  Cout <= 64     */
                           /* (the stem convolutions)                                                                              */
} mp_conv_desc;

int mp_conv2d_nhwc(const mp_conv_desc* desc, mp_stream stream);
/* Host-side launch plan of mp_conv2d_nhwc for a device with n_cu compute units (no GPU work; pointers in `desc` are only tested
 * for NULL): out5 = {mode, k_split, chunks_per_split, n_main_tiles, first_row_of_the_split_part}; mode 0 = one single-pass launch,
 * 1 = small grid, every tile split along K, 2 = whole rounds single-pass + split-K for the tiles of a half-empty last round. */
int mp_conv2d_plan(const mp_conv_desc* desc, int n_cu, int32_t* out5);

/* the name of the kernel instantiation mp_conv2d_nhwc would launch (for profiling)        */
const char* mp_conv2d_kernel_name(const mp_conv_desc* desc);

/* The direct convolution of mp_conv2d_nhwc with its multiplications on the bf16 MFMA through EXACT operand pieces (csrc/conv_bf16x9.hip):
 * the weights (scale folded as in mp_conv_pack_weights) and every fp32 activation fragment are split by truncation into three bf16 pieces
 * and ALL nine piece products are accumulated in fp32 -- the result differs from mp_conv2d_nhwc only in the order of the fp32 additions.
 * Same descriptor and fused epilogue; d_w_pieces = the blob of mp_conv_bf16x9_pack_weights uploaded to the device; `desc->d_w` and the
 * split-K fields are ignored (always one single-pass launch), x_f16 is refused.  Needs C % 16 == 0 and KW * C % 32 == 0. */
size_t mp_conv_bf16x9_packed_bytes(int Cin_p, int Cout, int KH, int KW);
int mp_conv_bf16x9_pack_weights(const float* h_w_oihw, int Cout, int Cin, int KH, int KW, int Cin_p, const float* h_scale /*[Cout] or NULL*/,
                                void* h_packed);
int mp_conv2d_bf16x9_nhwc(const mp_conv_desc* desc, const void* d_w_pieces, mp_stream stream);

/* Fused Winograd F(2x2, 3x3) form of the 3x3 / stride-1 / pad-1 convolutions of the residual stages (same call sites as
 * mp_conv2d_nhwc: models/torchvision_resnet.py:74-120 BasicBlock conv1 / conv2, models/wide_resnet.py:29-56) -- 16 instead of 36
 * multiplications per (2x2 output tile, cin, cout); fp32 MFMA, fp32 transforms; same fused epilogue (bias, residual, ReLU, second
 * pre-activated output).  d_u = the blob of mp_conv_wino_pack_weights uploaded to the device; `desc->d_w` and the split-K fields
 * are ignored.  Needs C % 16 == 0, Cout % 64 == 0, in_border >= 1.  When H or W is odd the kernel reads (and discards) up to one
 * padded row + one pixel past the end of the input tensor: the caller provides that much readable slack (the backbone workspace
 * does).  mp_conv_wino_eligible: 1 if a layer qualifies AND its grid gives each of n_cu compute units a workgroup (small grids stay
 * on mp_conv2d_nhwc's split-K path).  See csrc/conv_wino.hip. */
size_t mp_conv_wino_packed_floats(int Cin_p, int Cout);
int mp_conv_wino_pack_weights(const float* h_w_oi33, int Cout, int Cin, int Cin_p, const float* h_scale /*[Cout] or NULL*/, float* h_packed);
int mp_conv_wino_eligible(const mp_conv_desc* desc, int n_cu);
int mp_conv3x3_wino_nhwc(const mp_conv_desc* desc, const float* d_u, mp_stream stream);

/* The same fused Winograd convolution with its multiplications on the bf16 MFMA through EXACT operand pieces (csrc/conv_wino_bf16.hip):
 * U = G g G^T and every fp32 fragment of V = B^T d B are split by truncation into three bf16 pieces (24 = 3 x 8 mantissa bits) and ALL
 * nine piece products are accumulated in fp32 -- every product is exact, the result differs from mp_conv3x3_wino_nhwc only in the order
 * of the fp32 additions -- at 9/16 of the fp32-MFMA matrix time.  Same descriptor, eligibility (mp_conv_wino_eligible) and read-slack
 * contract; d_u_pieces = the blob of mp_conv_wino_bf16_pack_weights.  Launch form: persistent (one workgroup per CU walks the 64-tile x
 * 64-channel units; MP_WINO_PERSIST=0 = one workgroup per unit); results are identical.  (Counters / clock telemetry: mp_engine_debug.h.) */
size_t mp_conv_wino_bf16_packed_bytes(int Cin_p, int Cout);
int mp_conv_wino_bf16_pack_weights(const float* h_w_oi33, int Cout, int Cin, int Cin_p, const float* h_scale /*[Cout] or NULL*/, void* h_packed);
int mp_conv3x3_wino_bf16_nhwc(const mp_conv_desc* desc, const void* d_u_pieces, mp_stream stream);

/* Stem convolution on the bf16 MFMA through EXACT operand pieces (csrc/conv_stem.hip; same call site as mp_conv2d_nhwc for the first
 * layer: models/torchvision_resnet.py:213-216, models/wide_resnet.py:65-67).  The render channels of the CNN input are 8-bit integers
 * k / 255 by the reference's contract (uint8 -> float, panda3d_batch_renderer.py:261-274): k is ONE bf16 exactly; the weights (BN scale
 * and 1/255 folded in) and the fp32 observation-crop channels are split by truncation into three bf16 pieces each (24 = 3 x 8 mantissa
 * bits), so every bf16 x bf16 product is exact in the fp32 accumulator and the result differs from the fp32 convolution in the order of
 * the fp32 additions and in one rounding per integer-channel weight (the folded 1/255) -- at 3/16 (9/16 for the fp32-kind channels) of
 * the fp32-MFMA time.
 * Input = "xrec": padded NHWC of bf16 RECORDS, mp_xrec_elements(n_f32, n_u8) = roundup8(3 n_f32 + n_u8) elements per pixel:
 *   [x1,x2,x3 of the first fp32-kind channel | .. | of the last | k of the first integer channel | .. | zero padding]   (what MP_RASTER_XREC writes).
 * mp_conv_stem_xrec: desc as for mp_conv2d_nhwc with d_x = the record tensor, C ignored, c_real = n_f32 + n_u8; KH = KW in {5, 7},
 * stride 2, Cout % 64 == 0, records of 16..48 elements, no residual / second output. */
int mp_xrec_elements(int n_f32, int n_u8);
int mp_conv_stem_supported(int KS, int n_f32, int n_u8);
size_t mp_conv_stem_packed_bytes(int KS, int n_f32, int n_u8, int Cout);
/* the piece blob of a record: input channel c (< 32) is fp32-kind iff bit c of f32_mask is set -- (1u << n_f32) - 1u when the fp32-kind
 * channels are the n_f32 leading ones; an RGBD refiner: crop rgb + crop depth + one rendered depth per view = 0x8102040F for 32
 * channels, 4 views */
int mp_conv_stem_pack_weights_mask(const float* h_w_oihw, int Cout, int Cin, int KS, uint32_t f32_mask,
                                   const float* h_scale /*[Cout] or NULL*/, void* h_packed);
int mp_conv_stem_xrec(const mp_conv_desc* desc, const void* d_packed, int n_f32, mp_stream stream);
/* the same with the 3x3 / stride-2 / pad-1 max pool that follows the stem (models/torchvision_resnet.py:216) fused into the epilogue:
 * d_ypool = padded NHWC [N, (Ho-1)/2+1, (Wo-1)/2+1, Cout] with border pool_border; desc->relu must be set; desc->d_y may be NULL (the stem
 * map is then never written).  Windows that straddle the kernel's 8 x 16 tiles are combined with unsigned atomicMax on the (non-negative)
 * float bits: deterministic. */
int mp_conv_stem_xrec_pool(const mp_conv_desc* desc, const void* d_packed, int n_f32, float* d_ypool, int pool_border, mp_stream stream);

/* Background tiles (round 5).  A stem workgroup (8 x 16 output pixels) whose input patch holds no rendered geometry -- every integer
 * channel of every pixel 0: 47 % of a refiner step's tiles (measured, profiles/r05_stem_sparse_ab.txt) -- needs only the record chunks that hold fp32-kind pieces:
 * mp_conv_stem_sparse_chunks = ceil(3 n_f32 / 8) if that is fewer than the record's chunks and the fp32-kind channels are the leading
 * ones (no depth channels), else 0.  mp_conv_stem_xrec_sparse = mp_conv_stem_xrec[_pool] (d_ypool may be NULL) that takes, besides the
 * dense blob, the blob packed for that short walk and the rasteriser's job flags of the launch that wrote the records
 * (mp_raster_job_flags): such workgroups run 26 instead of 62 steps (7x7, 40-element records) and stage 2 of 5 chunks.  Skipped products
 * are exact zeros; the evaluated ones are grouped into MFMAs differently from the dense walk (order of the fp32 additions).
 * (mp_conv_stem_bg_stats, mp_engine_debug.h: how many workgroups took the short walk.) */
int mp_conv_stem_sparse_chunks(int KS, int n_f32, int n_u8);
size_t mp_conv_stem_sparse_packed_bytes(int KS, int n_f32, int n_u8, int Cout);
int mp_conv_stem_pack_weights_sparse(const float* h_w_oihw, int Cout, int Cin, int KS, int n_f32, const float* h_scale, void* h_packed);
int mp_conv_stem_xrec_sparse(const mp_conv_desc* desc, const void* d_packed, const void* d_packed_sparse, int n_f32,
                             const unsigned char* d_tile_flags, float* d_ypool, int pool_border, mp_stream stream);

/* Tail plane (round 8).  A walk whose last real record element sits alone in its 16-byte chunk (real elements mod 8 = 1) multiplies
 * seven zeros per tap for it.  Its tail-plane form walks only the chunks in front of that element and takes the element from a plane
 * the kernel builds in LDS: one K slice per kernel row holds the element's KS taps of that row.  mp_conv_stem_tail_forms: bit 0 = the
 * dense walk has the form (the RGB refiner's 33 real elements: 7x7 62 -> 52 steps), bit 1 = the background walk has it (3 n_f32 mod
 * 8 = 1, leading fp32-kind channels, integer channels behind them: the RGB crop's 9 pieces, 7x7 26 -> 14 steps; this also gives the
 * coarse net's 16-element record a background walk, which mp_conv_stem_sparse_chunks has none for); 0 = the record has no lone tail
 * element or the widened patch does not fit (7x7, 48 elements).  mp_conv_stem_pack_weights_tail packs the blob of one form (background
 * = 0 / 1) in the layout of mp_conv_stem_pack_weights_mask; mp_conv_stem_xrec_tail = mp_conv_stem_xrec_sparse where bit 0 / bit 1 of
 * tail_forms says that d_packed / d_packed_sparse is the tail blob (d_packed_sparse and d_tile_flags may be NULL: dense walk only).
 * Evaluated products are the same exact piece products; skipped ones are exact zeros; the order of the fp32 additions differs. */
int mp_conv_stem_tail_forms(int KS, int n_f32, int n_u8);
size_t mp_conv_stem_tail_packed_bytes(int KS, int n_f32, int n_u8, int Cout, int background);
int mp_conv_stem_pack_weights_tail(const float* h_w_oihw, int Cout, int Cin, int KS, uint32_t f32_mask, int background, const float* h_scale,
                                   void* h_packed);
int mp_conv_stem_xrec_tail(const mp_conv_desc* desc, const void* d_packed, const void* d_packed_sparse, int n_f32,
                           const unsigned char* d_tile_flags, float* d_ypool, int pool_border, int tail_forms, mp_stream stream);

/* 3x3 stride-2 pad-1 max pool on padded NHWC (input must be >= 0, i.e. post-ReLU).        */
int mp_maxpool3x3s2(const float* d_x, int N, int H, int W, int C, int in_border, float* d_y,
                    int out_border, float* d_y_act, const float* d_act_scale, const float* d_act_shift,
                    mp_stream stream);

/* y_act = relu(x * scale[c] + shift[c]) on the interior of a padded NHWC map (same border in and out): the pre-activation of a
 * WideResNet's first block (models/wide_resnet.py:29-44 bn1 / relu) when the max pool in front of it is fused into the stem
 * (mp_conv_stem_xrec_pool) -- bit-identical to the second output of mp_maxpool3x3s2. */
int mp_bn_relu_nhwc(const float* d_x, int N, int H, int W, int C, int border, float* d_y_act, const float* d_act_scale,
                    const float* d_act_shift, mp_stream stream);

/* global average pool (+ optional fc) + heads: models/torchvision_resnet.py:311-314 and  */
/* models/pose_rigid.py:326-333.  d_fc_w may be NULL (WideResNet: features = pooled).      */
int mp_pool_fc_heads(const float* d_x, int N, int H, int W, int C, int in_border, const float* d_fc_w,
                     const float* d_fc_b, int n_feat, const float* d_head_w, const float* d_head_b,
                     int n_out, float* d_feat /*[N,n_feat] or NULL*/, float* d_out /*[N,n_out]*/,
                     float* d_sigmoid /*[N,n_out] or NULL*/, mp_stream stream);

/* ------------------------------------------------------------------------------------ */
/* Backbone executor: whole network as one call (weights resident on the device).         */
/* ------------------------------------------------------------------------------------ */
typedef struct mp_backbone mp_backbone;
#define MP_BACKBONE_VANILLA_RESNET34 0
#define MP_BACKBONE_WIDE_RESNET34 1
#define MP_BACKBONE_WIDE_RESNET18 2

typedef struct {
  const char* name;    /* state_dict key, e.g. "backbone.layer1.0.conv1.weight"             */
  const float* h_data; /* host fp32, contiguous                                              */
  int64_t numel;
} mp_named_tensor;

/* state_dict layout = the reference checkpoints' (SURVEY.md, appendix F): backbone.*, pose_fc.*, views_logits_head.*.  head: 0 = pose_fc
 * (9 outputs), 1 = views_logits_head (n_views).  width = the WideResNet width multiplier of `resnet34_width=N`
 * (training/pose_models_cfg.py:114-116, models/wide_resnet.py:62: stage widths 64N .. 512N, features 512N); width = 1 for the released
 * models */
int mp_backbone_create_wide(int kind, int width, int c_in, int head_kind, int n_head_out, const mp_named_tensor* state, int n_tensors,
                            mp_backbone** out);
int mp_backbone_destroy(mp_backbone* bb);
int mp_backbone_input_channels_padded(const mp_backbone* bb);
int mp_backbone_input_border(const mp_backbone* bb);
size_t mp_backbone_workspace_bytes(const mp_backbone* bb, int batch, int h, int w);
/* The executor zeroes a workspace's borders once per (pointer, batch, h, w) and then trusts them.  Call this whenever the
 * memory behind `d_workspace` is a NEW allocation (the owner knows; an allocator may hand an old address back after foreign
 * writes): the next forward on it re-zeroes.                                                                            */
int mp_backbone_workspace_reset(mp_backbone* bb, const void* d_workspace);
/* d_x: padded NHWC [batch, h, w, Cp] with border mp_backbone_input_border().                */
int mp_backbone_forward(mp_backbone* bb, const float* d_x, int batch, int h, int w, float* d_out,
                        float* d_sigmoid, float* d_feat, void* d_workspace, size_t workspace_bytes,
                        mp_stream stream);
/* the same forward on a half-precision input tensor (binary16 elements, same padded-NHWC geometry: what the rasteriser writes  */
/* with MP_RASTER_F16).  Only the stem convolution differs (it widens the halves on their way into LDS).                       */
int mp_backbone_forward_f16(mp_backbone* bb, const void* d_x_half, int batch, int h, int w, float* d_out,
                            float* d_sigmoid, float* d_feat, void* d_workspace, size_t workspace_bytes,
                            mp_stream stream);
/* the same forward on the bf16 stem RECORDS the rasteriser writes with MP_RASTER_XREC (the fp32-kind channels first, all other
 * input channels 8-bit integers): only the stem convolution differs (mp_conv_stem_xrec: exact bf16 pieces, 16x the fp32 MFMA rate).
 * The fp32-kind channels are given as a mask (bit c = input channel c: (1u << n_f32) - 1u for n_f32 leading ones; also the depth
 * channels of an RGBD model).  mp_backbone_xrec_prepare packs and uploads the stem's piece blob for that mask (host work + a
 * synchronous copy) and returns the record length in bf16 elements for this backbone, 0 = the stem has no such form (records outside
 * 16..48 elements): use mp_backbone_forward.  The tensor has the geometry of the fp32 input (border mp_backbone_input_border()) with
 * records of that many bf16 elements per pixel.
 * PRECONDITION of every mp_backbone_forward_xrec_*: mp_backbone_xrec_prepare was called for that mask before (once, outside stream
 * capture, from one thread): the forwards only look the blob up and fail with MP_ERR_INVALID if it is missing -- they never allocate. */
int mp_backbone_xrec_prepare(mp_backbone* bb, uint32_t f32_mask);
int mp_backbone_forward_xrec_mask(mp_backbone* bb, const void* d_xrec, uint32_t f32_mask, int batch, int h, int w, float* d_out,
                                  float* d_sigmoid, float* d_feat, void* d_workspace, size_t workspace_bytes,
                                  mp_stream stream);
/* ... with the rasteriser's job flags of the launch that wrote the records (mp_raster_job_flags; NULL = dense): the stem takes the
 * background-tile walk where it applies (mp_conv_stem_xrec_sparse; the blob for it is packed by mp_backbone_xrec_prepare) */
int mp_backbone_forward_xrec_sparse(mp_backbone* bb, const void* d_xrec, uint32_t f32_mask, const unsigned char* d_tile_flags, int batch,
                                    int h, int w, float* d_out, float* d_sigmoid, float* d_feat, void* d_workspace,
                                    size_t workspace_bytes, mp_stream stream);
/* algorithmic conv+fc FLOPs of one forward at this batch (2*MACs, real channels only)       */
double mp_backbone_flops(const mp_backbone* bb, int batch, int h, int w);

/* ------------------------------------------------------------------------------------ */
/* Pose math (all fp32, one thread block per row)                                          */
/* ------------------------------------------------------------------------------------ */
/* lib3d/transform_ops.py:117-119 normalize_T (ortho6d Gram-Schmidt, rotations.py:25-40)    */
int mp_normalize_T(const float* d_T, int b, float* d_T_out, mp_stream stream);

/* per-(mesh, rotation) extents for TCO_init_from_boxes_autodepth_with_R                     */
/* (lib3d/cosypose_ops.py:198-208): d_ext[(mesh*n_rot + r)*2 + {0,1}] = max-min of x,y of R p */
int mp_init_extents(const float* d_points /*[n_mesh,n_pts,3]*/, int n_mesh, int n_pts,
                    const float* d_R /*[n_rot,3,3]*/, int n_rot, float* d_ext, mp_stream stream);
/* lib3d/cosypose_ops.py:169-218.  row i uses mesh d_mesh_ids[i], rotation d_rot_ids[i]      */
int mp_init_poses_from_boxes(const float* d_boxes /*[b,4]*/, const float* d_K /*[b,3,3]*/,
                             const int32_t* d_mesh_ids, const int32_t* d_rot_ids, const float* d_R,
                             int n_rot, const float* d_ext, int b, float* d_TCO /*[b,4,4]*/,
                             mp_stream stream);

/* One refiner/coarse "prepare" step for b rows x V views:                                  */
/*   TCO_n = normalize_T(TCO)                     (models/pose_rigid.py:524, :678)           */
/*   tCR   = TCO_n[:3,3]                          (:527-529)                                 */
/*   TCV_O = make_TCO_multiview(...)              (lib3d/multiview.py:165-246; App. A.5)     */
/*   boxes_rend/boxes_crop/K_crop from 2000 pts   (pose_rigid.py:180-247 crop_inputs)        */
/*   KV_crop from 200 pts for views >= 1          (:249-303; KV_crop[:,0] = K_crop :551-552) */
/* multiview: low byte = mode: 0 single view (V = 1), 1 "TCO+front_3views", 2 "TCO+front_1view", 3 "sphere_26views"            */
/* (lib3d/multiview.py:197-234), | MP_MV_REMOVE_TCO (remove_TCO_rendering: the TCO view is not in the list and KV_crop[:,0] is  */
/* NOT replaced by K_crop, models/pose_rigid.py:551-552), | MP_MV_INPLANE (views_inplane_rotations: every view 4x, rotated by   */
/* 0/90/180/270 degrees about the optical axis, multiview.py:236-245).  V must equal mp_pose_multiview_n_views(multiview).       */
/* d_K_main (may be NULL) additionally receives K_crop of crop_inputs ([b,3,3], what update_pose consumes).                    */
#define MP_MV_REMOVE_TCO 256
#define MP_MV_INPLANE 512
int mp_pose_multiview_n_views(int multiview);
int mp_pose_prepare_ex(const float* d_TCO_in /*[b,4,4]*/, const float* d_K /*[b,3,3]*/,
                       const int32_t* d_mesh_ids, const float* d_points /*[n_mesh,n_pts,3] sampled*/,
                       int n_pts_stride, int n_pts_main, int n_pts_views, int b, int V, int multiview,
                       int im_h, int im_w, int out_h, int out_w, float lamb,
                       float* d_TCO_n /*[b,4,4]*/, float* d_tCR /*[b,3]*/, float* d_TCV_O /*[b,V,4,4]*/,
                       float* d_KV_crop /*[b,V,3,3]*/, float* d_boxes_rend /*[b,4]*/,
                       float* d_boxes_crop /*[b,4]*/, float* d_K_main /*[b,3,3] or NULL*/, mp_stream stream);

/* models/pose_rigid.py:305-312 update_pose + lib3d/cosypose_ops.py:33-58                    */
int mp_pose_update(const float* d_TCO /*[b,4,4]*/, const float* d_K_crop /*[b,3,3] (stride 9*kstride)*/,
                   int k_stride_floats, const float* d_out9 /*[b,9]*/, const float* d_tCR /*[b,3]*/, int b,
                   float* d_TCO_out, mp_stream stream);

/* ------------------------------------------------------------------------------------ */
/* Pose errors (evaluation): the arithmetic between two pose tables and a mesh, fused so    */
/* that no point pair is stored (csrc/pose_error.hip; contract in csrc/pose_error_core.h).  */
/* Points are addressed as in mp_pose_prepare_ex: row i reads mesh d_mesh_ids[i] of d_points */
/* [n_mesh, n_pts_stride, 3] and averages its first min(d_n_points[mesh], n_pts) points     */
/* (d_n_points NULL: all n_pts), so BatchedMeshes.points with mesh ids and a per-row        */
/* [b,N,3] tensor (ids 0..b-1) both fit.  Outputs sized by n_pts have a zero / -1 tail.     */
/* A pose with a non-finite entry gives NaN errors and index -1.  split = 0 picks the work  */
/* split per row; > 0 forces it (any value gives the same bits).                            */
/* ------------------------------------------------------------------------------------ */
#define MP_POSE_ERROR_MEAN 0
#define MP_POSE_ERROR_MAX 1
/* bytes of device scratch any of the launches below needs for b rows (pass S_max = 1 for the nearest-neighbour launch alone). */
size_t mp_pose_error_workspace_bytes(int b, int n_pts, int S_max);
/* evaluation/utils.py:175-238 mssd_torch, lib3d/distances.py:26-41 dists_add (S_max = 1) and dists_add_symmetries: errs[i,s] =
   reduce_p |T_gt_s p - T_pred p| with reduce = mean (the reference) or max (BOP's MSSD), idx = argmin_s (lowest index on a tie).
   Composed form: d_symmetries [n_mesh,S_max,4,4] identity-padded, d_n_sym [n_mesh] (NULL: S_max), d_T_gt [b,4,4], T_gt_s = T_gt
   Sym_s.  Explicit form (d_symmetries NULL): d_T_gt holds the candidates [b,S_max,4,4].  Optional (NULL to skip): d_err_alt [b] the
   minimum of the OTHER reduction, d_T_gt_sym [b,4,4], d_errs [b,S_max] (+inf beyond n_sym), d_diffs [b,n_pts,3] = T_gt_idx p -
   T_pred p.  S_max <= 512. */
int mp_pose_error_sym(const float* d_T_pred /*[b,4,4]*/, const float* d_T_gt, const float* d_symmetries, const int32_t* d_n_sym, int S_max,
                      const float* d_points, int n_pts_stride, const int32_t* d_mesh_ids /*[b]*/, const int32_t* d_n_points, int n_pts,
                      int b, int reduce, int split, float* d_err /*[b]*/, float* d_err_alt, int32_t* d_idx /*[b]*/, float* d_T_gt_sym,
                      float* d_errs, float* d_diffs, void* d_workspace, size_t workspace_bytes, mp_stream stream);
/* lib3d/distances.py:44-53 dists_add_symmetric (ADD-S): for every ground-truth point j, assign[i,j] = argmin_k |T_gt p_j - T_pred
   p_k|^2 over the row's valid points (lowest k on a tie), d_diffs [b,n_pts,3] = T_gt p_j - T_pred p_assign, d_assign [b,n_pts]
   (both optional), d_mean / d_max [b] of the norms.  b * n_pts^2 pairs, none stored. */
int mp_pose_error_nn(const float* d_T_pred /*[b,4,4]*/, const float* d_T_gt /*[b,4,4]*/, const float* d_points, int n_pts_stride,
                     const int32_t* d_mesh_ids, const int32_t* d_n_points, int n_pts, int b, int split, float* d_diffs, int32_t* d_assign,
                     float* d_mean /*[b]*/, float* d_max /*[b]*/, void* d_workspace, size_t workspace_bytes, mp_stream stream);
/* evaluation/utils.py:50-66 compute_pose_error (trans_err = |t_a - t_b|, rot_err_deg = angle of R_b R_a^T, by atan2 and not acos)
   and, when d_proj_err is given, evaluation/meters/modelnet_meters.py:75-79: the mean over the valid points of the 2D distance
   between project_points (lib3d/camera_geometry.py:26-37) of the two poses with d_K [b,3,3].  Without it K / points may be NULL. */
int mp_pose_error_rigid(const float* d_T_a /*[b,4,4]*/, const float* d_T_b /*[b,4,4]*/, int b, const float* d_K, const float* d_points,
                        int n_pts_stride, const int32_t* d_mesh_ids, const int32_t* d_n_points, int n_pts, float* d_trans_err /*[b]*/,
                        float* d_rot_err_deg /*[b]*/, float* d_proj_err, mp_stream stream);

/* BOP's MSPD (maximum symmetry-aware projection distance): mp_pose_error_sym with the norm taken between pixel positions, errs[i,s] =
   reduce_p |proj(K_i, T_pred p) - proj(K_i, T_gt_s p)|_2 with proj the projection of mp_pose_error_rigid's d_proj_err (P = K T[:3],
   perspective division), reduce = max for MSPD (mean is there too), idx = argmin_s with the lowest index on a tie.  Every other
   argument (composed / explicit symmetry forms, point addressing, S_max <= 512, optional outputs, NaN and -1 for a non-finite pose,
   workspace of mp_pose_error_workspace_bytes(b, n_pts, S_max)) means what it means for mp_pose_error_sym; d_K [b,3,3] is required.
   Pixels, not metres.  The maximum does not depend on the order of reduction: the same bits for every split. */
int mp_pose_error_mspd(const float* d_T_pred /*[b,4,4]*/, const float* d_T_gt, const float* d_symmetries, const int32_t* d_n_sym, int S_max,
                       const float* d_points, int n_pts_stride, const int32_t* d_mesh_ids /*[b]*/, const int32_t* d_n_points, int n_pts,
                       int b, int reduce, int split, const float* d_K /*[b,3,3]*/, float* d_err /*[b]*/, float* d_err_alt,
                       int32_t* d_idx /*[b]*/, float* d_T_gt_sym, float* d_errs, void* d_workspace, size_t workspace_bytes, mp_stream stream);

/* ------------------------------------------------------------------------------------ */
/* BOP's VSD (visible surface discrepancy, BOP 2019: visibility "bop19", step cost) between */
/* rendered depth maps and an observed frame (csrc/vsd.hip; contract in csrc/vsd_core.h).   */
/* All maps are [n,h,w] fp32 metres along the optical axis (0 = nothing), pixel centres as   */
/* in mp_render's geometric depth; an observed depth that is not finite or < 0 counts as 0.  */
/* Row i compares map d_est_ids[i] of d_depth_est with map d_gt_ids[i] of d_depth_gt under   */
/* frame d_im_ids[i] of d_depth_test (an id array NULL: map i), so K hypotheses share one     */
/* ground-truth render and many rows one frame; the ids are the caller's responsibility.     */
/* ------------------------------------------------------------------------------------ */
/* bytes of device scratch mp_vsd needs for b rows (0 for arguments mp_vsd rejects). */
size_t mp_vsd_workspace_bytes(int b, int n_tau);
/* With r the length of pixel (x, y)'s ray at unit depth under K_i and dist = depth * r: vis_gt = dist_gt > 0 and (dist_test == 0 or
   dist_gt - dist_test <= delta); vis_est the same with dist_est, or-ed with vis_gt inside the bracket; n_union / n_inter count the
   union / intersection of the two masks, n_far_t the intersection pixels with |dist_gt - dist_est| >= thr_t, thr_t = h_taus[t] *
   d_diameter[i] (h_taus[t] alone when normalized == 0); d_errs[i,t] = (n_far_t + n_union - n_inter) / n_union, 1 on an empty union.
   h_taus is a HOST array of n_tau in 1..16 values, read before the call returns.  A row whose K has a non-finite entry or whose
   diameter is not positive and finite gives NaN errors and counts of -1.  d_counts [b,2+n_tau] = n_union, n_inter, n_far_t is optional
   (NULL to skip).  h, w in 1..1024.  split = 0 picks the number of strips of image rows a row is cut into; > 0 forces it (counts are
   integers: any value gives the same bits).  The counters live in d_workspace and are zeroed on `stream` inside the call.  b == 0
   is a successful no-op; any other bad argument returns non-zero before anything is launched. */
int mp_vsd(const float* d_depth_est /*[n_est,h,w]*/, const int32_t* d_est_ids /*[b] or NULL: 0..b-1*/,
           const float* d_depth_gt /*[n_gt,h,w]*/, const int32_t* d_gt_ids, const float* d_depth_test /*[n_im,h,w]*/,
           const int32_t* d_im_ids, int n_est, int n_gt, int n_im, const float* d_K /*[b,3,3]*/, const float* d_diameter /*[b]*/,
           int b, int h, int w, float delta, const float* h_taus, int n_tau /*1..16*/, int normalized, int split,
           float* d_errs /*[b,n_tau]*/, int32_t* d_counts /*[b,2+n_tau]: n_union, n_inter, n_far_t; optional*/,
           void* d_workspace, size_t workspace_bytes, mp_stream stream);

/* ------------------------------------------------------------------------------------ */
/* BOP's ground-truth info (what the reference reads from a BOP dataset's scene_gt_info:   */
/* evaluation/meters/utils.py:86-104 visib_fract, datasets/bop_scene_dataset.py:238-262     */
/* bbox_visib / bbox_obj, inference/utils.py:214-225 ground-truth detections) computed from  */
/* depth renders of the object and an observed frame (csrc/gt_info.hip; contract in          */
/* csrc/gt_info_core.h).  Maps are fp32 metres as for mp_vsd.  The object is rendered on a    */
/* canvas of canvas x canvas tiles of the image's size (canvas 1 or 3, tiles row-major,       */
/* c = (canvas - 1) / 2): tile (ty, tx) is the render under K with cx - (tx - c) w and         */
/* cy - (ty - c) h, so its pixel (x, y) is image pixel (x + (tx - c) w, y + (ty - c) h); the    */
/* centre tile is the render under K itself and the only one compared with the frame.         */
/* ------------------------------------------------------------------------------------ */
/* bytes of device scratch mp_gt_info needs for b rows (0 for b < 0). */
size_t mp_gt_info_workspace_bytes(int b);
/* Row i takes canvas map d_gt_ids[i] of d_depth_gt and frame d_im_ids[i] of d_depth_test (an id array NULL: map i; the ids are the
   caller's responsibility).  With obj = depth_gt > 0: d_counts[i] = px_count_all (obj pixels over all tiles), px_count_image (obj pixels
   of the centre tile), px_count_valid (centre tile: obj and an observed distance > 0), px_count_visib (centre tile: mp_vsd's vis_gt under
   K_i and delta); d_visib_fract[i] = px_count_visib / px_count_all as one fp32 division, 0 when px_count_all == 0; d_boxes[i] = inclusive
   extents xmin ymin xmax ymax in image coordinates (-w .. 2w - 1) of the obj pixels over all tiles, then of the vis_gt pixels; a box over
   no pixel is -1 -1 -1 -1.  d_mask / d_mask_visib [b,h,w] uint8 (0 / 255: obj / vis_gt on the centre tile) are optional (NULL to skip).
   A row whose K has a non-finite entry gives counts and boxes of -1, NaN and zero masks.  h, w in 1..1024.  split = 0 picks the number
   of strips of image rows a tile is cut into; > 0 forces it (counts and extents are integers: any value gives the same bits).  The
   accumulators live in d_workspace and are initialised on `stream` inside the call.  b == 0 is a successful no-op; any other bad
   argument returns non-zero before anything is launched. */
int mp_gt_info(const float* d_depth_gt /*[n_gt,canvas*canvas,h,w]*/, const int32_t* d_gt_ids /*[b] or NULL: 0..b-1*/,
               const float* d_depth_test /*[n_im,h,w]*/, const int32_t* d_im_ids, int n_gt, int n_im, const float* d_K /*[b,3,3]*/,
               int b, int h, int w, int canvas /*1 or 3*/, float delta, int split,
               int32_t* d_counts /*[b,4]: all, image, valid, visib*/, int32_t* d_boxes /*[b,8]: obj, visib*/,
               float* d_visib_fract /*[b]*/, uint8_t* d_mask /*[b,h,w] or NULL*/, uint8_t* d_mask_visib /*[b,h,w] or NULL*/,
               void* d_workspace, size_t workspace_bytes, mp_stream stream);

/* ------------------------------------------------------------------------------------ */
/* BOP's greedy matching of pose estimates to ground truths (what the reference does in    */
/* pandas: evaluation/meters/utils.py:51-83 get_top_n_ids, :120-152 match_poses on          */
/* cand[cand.error < theta]), every (group, error column, threshold) problem in one launch   */
/* (csrc/bop_match.hip; contract in csrc/bop_match_core.h).  A group is one (image, label);  */
/* an estimate or a ground truth belongs to one group.  THE INDEX the caller builds:         */
/*   candidates sorted by (group, walk order of their estimate, gt_row), where a group's      */
/*   estimates are walked by decreasing score, ties by ascending pred_row:                    */
/*     d_errs [C,E], d_cand_gt [C] = gt_row, d_cand_lgt [C] = the number of that ground truth  */
/*     inside its group, 0 .. d_group_n_gt[g] - 1 by ascending gt_row;                         */
/*   listed estimates (those with a candidate) in the same order:                             */
/*     d_est_row [n_est] = pred_row, d_est_off [n_est+1] = first candidate of each;            */
/*   groups: d_group_est_off [n_groups+1] = first listed estimate of each, d_group_n_gt        */
/*     [n_groups], d_group_taken_off [n_groups+1] = running sum of ceil(d_group_n_gt / 32)     */
/*     (n_taken_words = its last entry), d_n_top [n_groups] (or NULL: all 0),                  */
/*     d_thr [n_groups,E,n_theta] float64.                                                     */
/* The index is the caller's responsibility: it is not range-checked.                         */
/* ------------------------------------------------------------------------------------ */
/* what mp_bop_match was built for: E <= max_errors, n_theta <= max_thetas; a group with at most mask_bits ground truths and walked
   candidates * E <= stage_floats takes the fast path (any other group the general one, with the same results). */
int mp_bop_match_limits(int* max_errors, int* max_thetas, int* mask_bits, int* stage_floats);
/* bytes of device scratch mp_bop_match needs (0 for arguments it rejects). */
size_t mp_bop_match_workspace_bytes(int n_taken_words, int E, int n_theta);
/* d_match [P,E,n_theta] = for problem (group, e, k), walking the group's first n_top estimates (0: all) in the index's order, each
   estimate takes, among its candidates whose ground truth no earlier estimate of the walk took and with (double)err < thr[group,e,k]
   (strict, float64; never for NaN), the one of the smallest error, the first in gt_row order on an exact tie; -1 for no match, for an
   estimate without candidates and for one cut by n_top.  E, n_theta in 1..16.  P == 0 is a successful no-op, C == 0 (or no listed
   estimate, or no group) writes -1 everywhere and launches nothing; any bad argument (a null pointer where one is needed, a negative
   count, E or n_theta out of range, a workspace too small) returns non-zero before anything is launched. */
int mp_bop_match(const float* d_errs /*[C,E]*/, const int32_t* d_cand_gt /*[C]*/, const int32_t* d_cand_lgt /*[C]*/,
                 const int32_t* d_est_row /*[n_est]*/, const int32_t* d_est_off /*[n_est+1]*/,
                 const int32_t* d_group_est_off /*[n_groups+1]*/, const int32_t* d_group_n_gt /*[n_groups]*/,
                 const int32_t* d_group_taken_off /*[n_groups+1]*/, const int32_t* d_n_top /*[n_groups] or NULL*/,
                 const double* d_thr /*[n_groups,E,n_theta]*/, int P, int C, int n_est, int n_groups, int n_taken_words, int E,
                 int n_theta, int32_t* d_match /*[P,E,n_theta]*/, void* d_workspace, size_t workspace_bytes, mp_stream stream);

/* ------------------------------------------------------------------------------------ */
/* BOP's 2D detection and 2D segmentation scores (COCO average precision): the pixel counts */
/* behind the mask IoU of every (detection, ground truth) candidate, and COCO's greedy       */
/* matching (pycocotools' COCOeval.evaluateImg with iscrowd = 0 and one area range) at every  */
/* IoU threshold in one launch (csrc/det_ap.hip; contract in csrc/det_ap_core.h).  The        */
/* accumulation to AP / AR is host arithmetic (evaluation.coco_accumulate).                   */
/* ------------------------------------------------------------------------------------ */
/* Masks are bytes; a pixel is set when its byte is non-zero (a bool tensor's 0 / 1, mp_gt_info's 0 / 255, anything else).
   d_counts[c] = {pixels set in both d_pred_masks[d_cand_pred[c]] and d_gt_masks[d_cand_gt[c]], pixels set in the former, pixels set in
   the latter}; a candidate whose index is outside [0, P) or [0, G) reads nothing and gives -1 -1 -1.  H * W in 1 .. 2^31 - 1 (a count fits
   an int32; mask offsets are size_t), C <= 2^23 per call.  16-byte loads when H * W is a multiple of 16 and both tensors are 16-byte
   aligned, else byte loads with the same results.  split = 0 picks the number of slices a mask is cut into; > 0 forces it (integer sums:
   any value gives the same bits).  d_counts is zeroed on `stream` inside the call; there is no scratch.  C == 0 is a successful no-op;
   any other bad argument (a null pointer, a negative count, H * W out of range, candidates without masks) returns non-zero before
   anything is launched. */
int mp_mask_pair_counts(const uint8_t* d_pred_masks /*[P,H,W]*/, const uint8_t* d_gt_masks /*[G,H,W]*/,
                        const int32_t* d_cand_pred /*[C]*/, const int32_t* d_cand_gt /*[C]*/, int P, int G, int C, int H, int W, int split,
                        int32_t* d_counts /*[C,3]: intersection, area pred, area gt*/, mp_stream stream);
/* bytes of device scratch mp_det_match needs (0 for arguments it rejects). */
size_t mp_det_match_workspace_bytes(int n_taken_words, int n_theta);
/* THE INDEX is mp_bop_match's, unchanged.  d_match [P,n_theta] = for problem (group, k), walking the group's first n_top estimates (0:
   all) in the index's order, each estimate looks at its candidates whose ground truth no earlier estimate of the walk took and whose
   d_iou >= min(d_thr[k], 1 - 1e-10) (float64; never for NaN): first at those with d_gt_ignore[gt_row] == 0, taking the largest IoU, the
   LAST in gt_row order on an exact tie; only if there is none, the same among those with d_gt_ignore != 0.  A taken ground truth, ignored
   or not, stays taken.  -1 for no match, for an estimate without candidates and for one cut by n_top.  n_theta in 1..16.  P == 0 is a
   successful no-op, C == 0 (or no listed estimate, or no group) writes -1 everywhere and launches nothing; any bad argument (a null
   pointer where one is needed, a negative count, n_theta out of range, a workspace too small) returns non-zero before anything is
   launched.  The index is not range-checked. */
int mp_det_match(const double* d_iou /*[C], the index's order*/, const int32_t* d_cand_gt /*[C]*/, const int32_t* d_cand_lgt /*[C]*/,
                 const int32_t* d_est_row /*[n_est]*/, const int32_t* d_est_off /*[n_est+1]*/,
                 const int32_t* d_group_est_off /*[n_groups+1]*/, const int32_t* d_group_n_gt /*[n_groups]*/,
                 const int32_t* d_group_taken_off /*[n_groups+1]*/, const int32_t* d_n_top /*[n_groups] or NULL*/,
                 const uint8_t* d_gt_ignore /*[G]*/, const double* d_thr /*[n_theta]*/, int P, int C, int n_est, int n_groups,
                 int n_taken_words, int n_theta, int32_t* d_match /*[P,n_theta]*/, void* d_workspace, size_t workspace_bytes,
                 mp_stream stream);

/* ------------------------------------------------------------------------------------ */
/* BOP's result files: COCO run-length encoding (RLE) of binary masks, the form in which the */
/* detection and segmentation tasks carry a mask, both ways (csrc/rle.hip; contract in       */
/* csrc/rle_core.h).  pycocotools is third party: its format is restated, parity unpinned.   */
/* The compressed string and the files are host Python (megapose6d_amd/bop_files.py).        */
/* ------------------------------------------------------------------------------------ */
/* bytes of device scratch mp_rle_count and mp_rle_encode need (0 for arguments they reject). */
size_t mp_rle_workspace_bytes(int n, int h, int w, int rows_per_segment);
/* Masks are h x w bytes, row-major; a pixel is set when its byte is non-zero (the rule of mp_mask_pair_counts).  The list of mask m walks
   it in column-major order, p = x * h + y, and alternates run lengths of unset and set pixels, starting with unset (so its first entry
   is 0 when pixel 0 is set); a run continues from the bottom of a column into the top of the next; the entries sum to h * w.
   d_n_counts[m] = the length of the list (1 .. h * w + 1), d_areas[m] = the number of set pixels, d_boxes[m] = x_min, y_min, x_max, y_max
   of the set pixels, inclusive, (0, 0, -1, -1) for an empty mask.  rows_per_segment = the rows one lane walks: 0 the library's choice
   (32), any other value only changes the decomposition, never a result.  16-byte loads where a row's 16 columns lie inside it on a
   16-byte boundary, else byte loads with the same results (any width, any byte alignment of d_masks).  h, w >= 1, h * w <= 2^31 - 2,
   at most 2^30 jobs (mask, row segment, 16 columns) and as many (mask, column, row segment) entries.  Two launches on `stream`, no
   atomics, no workgroup waits for another.  What the call leaves in d_ws is the input of mp_rle_encode on the same masks and arguments.
   n == 0 is a successful no-op; any bad argument (a null pointer where one is needed, h or w < 1, too many pixels or jobs, a negative
   count, a workspace too small or not 16-byte aligned) returns non-zero before anything is launched. */
int mp_rle_count(const uint8_t* d_masks /*[n,h,w]*/, int n, int h, int w, int rows_per_segment, int32_t* d_n_counts /*[n]*/,
                 int32_t* d_areas /*[n] or NULL*/, int32_t* d_boxes /*[n,4] or NULL*/, void* d_ws, size_t ws_bytes, mp_stream stream);
/* Writes the lists: mask m's into d_counts[h_offsets[m] .. h_offsets[m + 1] - 1].  To be called after mp_rle_count on the same masks,
   arguments and workspace, with h_offsets (host memory, n + 1 entries) the exclusive sums of the d_n_counts it gave.  h_offsets must
   start at 0, not descend and end within `capacity`, the number of int32 d_counts holds; every store is checked against the list's
   length as h_offsets states it, so offsets that do not fit the masks cost wrong lists, never a store outside d_counts.  One launch on
   `stream`; h_offsets is copied from pageable host memory.  n == 0 is a successful no-op; any bad argument returns non-zero before
   anything is launched. */
int mp_rle_encode(const uint8_t* d_masks /*[n,h,w]*/, int n, int h, int w, int rows_per_segment, const int64_t* h_offsets /*[n+1], host*/,
                  int32_t* d_counts /*[h_offsets[n]]*/, long long capacity, void* d_ws, size_t ws_bytes, mp_stream stream);
/* bytes of device scratch mp_rle_decode needs for n lists of h x w masks in `capacity` counts (0 for arguments it rejects). */
size_t mp_rle_decode_workspace_bytes(int n, int h, int w, long long capacity);
/* The masks of n lists: d_masks[m] (0 / 1 bytes, row-major) from d_counts[h_offsets[m] .. h_offsets[m + 1] - 1].  d_status[m] = 0 for a
   well-formed list, else the OR of 1 (no entries), 2 (a negative entry), 4 (the entries do not sum to h * w), and the mask is all
   zeros.  h_offsets (host memory) must start at 0, not descend and end within `capacity`, the number of int32 d_counts holds, and is
   tested before anything is launched; the counts themselves are only summed and compared until their list has passed, so a wrong file
   costs a status, never an access out of range.  A pixel is the parity of its run, found by a search of at most 32 steps over the
   cumulative ends.  Limits of h, w and n as for mp_rle_count.  Three launches on `stream`, no atomics; h_offsets is copied from pageable
   host memory.  n == 0 is a successful no-op; any bad argument returns non-zero before anything is launched. */
int mp_rle_decode(const int32_t* d_counts /*[capacity]*/, const int64_t* h_offsets /*[n+1], host*/, long long capacity, int n, int h, int w,
                  uint8_t* d_masks /*[n,h,w]*/, int32_t* d_status /*[n]*/, void* d_ws, size_t ws_bytes, mp_stream stream);

/* ------------------------------------------------------------------------------------ */
/* Onboarding an object without a CAD model: posed depth views fused into a truncated     */
/* signed distance field (TSDF) on a voxel grid in the object's frame, and the welded,     */
/* coloured triangle mesh of its zero level by marching tetrahedra (csrc/tsdf.hip; contract */
/* in csrc/tsdf_core.h).  The reference has no counterpart; Open3D / KinectFusion-style      */
/* tools are third party and absent: parity with them is unpinned.                          */
/* ------------------------------------------------------------------------------------ */
/* bytes of a volume of nx x ny x nz nodes: 2 planes of 32-bit words (fp32 sum of truncated distances, int32 count of views), 6 with
   colours (+ fp32 sums of red, green, blue, int32 colour count); x fastest; 0 for dims out of range (each 2 .. 512, at most 2^27 nodes).
   A volume of zero bytes is an empty one. */
size_t mp_tsdf_volume_bytes(int nx, int ny, int nz, int color);
/* Integrates n views, in ascending order, into the volume (rules: csrc/tsdf_core.h).  Node (i,j,k) lies at origin + voxel * (i,j,k) in
   the object's frame; TCO maps object to camera (rows of 4; tco_floats = 12 or 16 per view); K is 3 x 3 row-major.  Per view and node:
   pc = R p + t, skipped unless pc.z > z_min; pixel = floor(f * pc / pc.z + c), skipped outside the frame; with d_masks given, a pixel
   with mask == 0 adds +1 to the sum and 1 to the count when `carve` (free space: the visual hull) and nothing otherwise; a depth that is
   not finite or <= 0 adds nothing; else sd = depth - pc.z, skipped when sd < -mu, else min(1, sd / mu) is added to the sum and 1 to the
   count, and with colours in the volume, d_rgb given and |sd| <= mu the pixel's bytes to the colour sums.  Sums and counts: calls
   continue each other bit for bit.  A view whose K or TCO holds a non-finite entry contributes nothing, never an access out of range.
   One launch on `stream`, one lane per node, no atomics.  n == 0 is a successful no-op; any bad argument (a null pointer where one is
   needed, dims out of range, a non-finite origin, a non-finite or non-positive voxel or mu, a negative or non-finite z_min, frames
   outside 1 .. 8192 a side) returns non-zero before anything is launched. */
int mp_tsdf_integrate(void* d_volume, int nx, int ny, int nz, int color, float ox, float oy, float oz, float voxel,
                      const float* d_depth /*[n,h,w]*/, const uint8_t* d_masks /*[n,h,w] or NULL*/, const uint8_t* d_rgb /*[n,h,w,3] or NULL*/,
                      const float* d_K /*[n,9]*/, const float* d_TCO /*[n,tco_floats]*/, int tco_floats, int n, int h, int w, float mu,
                      float z_min, int carve, mp_stream stream);
/* bytes of device scratch mp_tsdf_extract_count and mp_tsdf_extract need (0 for dims they reject). */
size_t mp_tsdf_extract_workspace_bytes(int nx, int ny, int nz);
/* Counts the surface: d_totals[0] = vertices, d_totals[1] = triangles of the zero level of f = sum / count over the nodes with
   count >= min_views (>= 1), by marching tetrahedra over the cells whose eight corners are all observed (six tetrahedra around the
   main diagonal; a vertex per edge with exactly one end inside, f < 0).  Four launches on `stream`, no atomics, no workgroup waits for
   another.  What the call leaves in d_ws is the input of mp_tsdf_extract on the same volume.  Any bad argument (a null pointer, dims
   out of range, min_views < 1, a workspace too small or not 16-byte aligned) returns non-zero before anything is launched. */
int mp_tsdf_extract_count(const void* d_volume, int nx, int ny, int nz, int color, int min_views, int32_t* d_totals /*[2]*/, void* d_ws,
                          size_t ws_bytes, mp_stream stream);
/* Writes the mesh: vertices and colours (0 .. 1; white without colours) in the order of (node * 7 + edge kind), triangles in the
   order of (cell, tetrahedron, triangle), wound so that normals point out of the object.  To be called after mp_tsdf_extract_count on
   the same volume and workspace, with the two totals it gave; every store is checked against them, so totals that do not fit the
   volume cost a wrong mesh, never a store outside the arrays.  One launch on `stream`.  n_vertices == n_triangles == 0 is a successful
   no-op; any bad argument (a null pointer where one is needed, dims out of range, a bad origin or voxel, negative totals, capacities
   smaller than the totals, a workspace too small or not 16-byte aligned) returns non-zero before anything is launched. */
int mp_tsdf_extract(const void* d_volume, int nx, int ny, int nz, int color, float ox, float oy, float oz, float voxel, int n_vertices,
                    int n_triangles, float* d_vertices /*[cap_vertices,3]*/, float* d_colors /*[cap_vertices,3]*/,
                    int32_t* d_faces /*[cap_triangles,3]*/, long long cap_vertices, long long cap_triangles, void* d_ws, size_t ws_bytes,
                    mp_stream stream);
/* Tracking the camera against the volume (csrc/tsdf_track.hip; contract in csrc/tsdf_track_core.h): the poses of unposed depth frames by
   Gauss-Newton on the signed distances the volume holds at the frames' own back-projected pixels -- no raycast, no projective association. */
/* records of 32 doubles a frame of h x w leaves in d_partials of mp_tsdf_track: one per group of 1024 pixels, ceil(h * w / 1024); 0 for a
   refused frame size (a side outside 1 .. 8192).  Host only. */
int mp_tsdf_track_groups(int h, int w);
/* Tracks n frames against the same volume, each from its own pose d_TCO_in (object to camera, rows of 4, 16 floats), independently: n
   frames in one call equal n calls of one.  Per iteration and pixel inside the mask (every pixel without masks) with a depth that is
   finite and > 0: the pixel's centre back-projected, taken to the object's frame by the current pose, the field sum / count interpolated
   trilinearly from the eight nodes around it (skipped outside the volume, where a corner has count < min_views, or where |f| >= 1), the
   residual f * mu and its Jacobian for a small motion in the object's frame; the normal equations are summed in fp64 in one fixed order
   (one record per group of 1024 pixels into d_partials, a typed output, every entry written by plain stores), solved with the damping
   1e-9 * used, the increment applied through the Cayley map, the rotation re-orthonormalised, the pose rounded to fp32.  d_status: 0 ran
   all iterations, 1 converged (|rotation| < eps_rot rad and |translation| < eps_trans metres; later iterations skip the frame), -1 lost
   (fewer than min_pixels used pixels, a pivot that is not positive, a non-finite pose), -2 the frame's K or pose holds a non-finite
   entry.  A frame of status -1 or -2 returns its input pose bit for bit in d_TCO_out.  d_used / d_rms: the used pixels and the
   root-mean-square residual (metres) of the last iteration that ran.  1 + 2 * iters launches on `stream`, no atomics, no workgroup waits
   for another, nothing is read back.  n == 0 is a successful no-op; any bad argument (a null pointer, dims out of range, a bad origin,
   voxel or mu, min_views < 1, min_pixels < 1, iters outside 1 .. 64, an eps that is negative or not finite, n outside 0 .. 65535, frames
   outside 1 .. 8192 a side, d_TCO_out == d_TCO_in, partials_capacity < n * groups, a misaligned volume or partials) returns non-zero
   before anything is launched, with the outputs untouched. */
int mp_tsdf_track(const void* d_volume, int nx, int ny, int nz, int color, float ox, float oy, float oz, float voxel,
                  const float* d_depth /*[n,h,w]*/, const uint8_t* d_masks /*[n,h,w] or NULL*/, const float* d_K /*[n,9]*/,
                  const float* d_TCO_in /*[n,16]*/, int n, int h, int w, float mu, int min_views, int min_pixels, int iters, float eps_rot,
                  float eps_trans, float* d_TCO_out /*[n,16]*/, int32_t* d_status /*[n]*/, int32_t* d_used /*[n]*/, float* d_rms /*[n]*/,
                  double* d_partials /*[n,groups,32]*/, long long partials_capacity /*records*/, mp_stream stream);

/* ------------------------------------------------------------------------------------ */
/* A texture atlas for a triangle mesh (a reconstruction's) from the posed colour + depth   */
/* views it was made from: every triangle gets a chart, every texel of a chart gathers its  */
/* colour from the views that see its surface point (csrc/texture_bake.hip; contract in     */
/* csrc/texture_bake_core.h).  The reference has no counterpart; Open3D, xatlas and          */
/* MVS-texturing are third party and absent: parity with them is unpinned.                  */
/* The atlas is size x size texels (a power of two, 64 .. 8192; row 0 is v = 0), cut into    */
/* blocks of B x B texels in row-major order; block k holds triangle 2k (the lower chart,    */
/* legs of B - 3 texels from the block's first texel) and 2k + 1 (the upper chart, the lower */
/* one turned by 180 degrees).                                                              */
/* ------------------------------------------------------------------------------------ */
/* B for n_triangles in an atlas of `size`: the largest of 64, 32, 16, 8, 4 with ceil(n_triangles / 2) <= (size / B)^2; 0 when none fits,
   when size is no power of two in 64 .. 8192, or n_triangles < 1.  Host only. */
int mp_texture_atlas_block(long long n_triangles, int size);
/* Writes the per-corner texture coordinates of the charts: corner c of triangle t at the centre of its chart's corner texel,
   ((i + 0.5) / size, (j + 0.5) / size).  One launch on `stream`.  Any bad argument (a null or misaligned pointer, n_triangles outside
   1 .. 2^29, a bad size, triangles that do not fit) returns non-zero before anything is launched. */
int mp_texture_atlas_uvs(int n_triangles, int size, float* d_uvs /*[n_triangles,3,2]*/, mp_stream stream);
/* Bakes the atlas (rules: csrc/texture_bake_core.h).  Per texel of a chart: its chart coordinates (a, b), clamped onto the triangle,
   give the surface point p = v0 + a (v1 - v0) + b (v2 - v0); per view, in ascending order: pc = R p + t, skipped unless pc.z > z_min and
   the pixel floor(f * pc / pc.z + c) lies in the frame; skipped unless the face normal looks at the camera with cos > cos_min (weight
   cos^2); a pixel counts when its mask is non-zero (d_masks given), its depth is finite, > 0 and within depth_tol of pc.z (the occlusion
   test); the colour is the bilinear mix of the four pixels around the projection when all four count, else the nearest pixel's, else
   the view is skipped.  The texel is the weighted mean over the views (best_view: the colour of the heaviest view), rounded half up;
   d_seen the number of contributing views, capped at 255.  A texel no view contributes to takes the interpolated d_colors ([V,3] floats
   in 0 .. 1) or white; texels of no triangle are four zero bytes.  TCO maps object to camera (rows of 4; tco_floats = 12 or 16 per
   view); K is 3 x 3 row-major; a view whose K or TCO holds a non-finite entry contributes nothing.  A face with an index outside
   [0, n_vertices), a non-finite vertex or no area bakes as unseen, never an access out of range.  One launch on `stream`, one lane per
   texel, no atomics, no workspace.  n == 0 bakes the fallback everywhere (the view pointers may then be null); any bad argument (a
   null pointer where one is needed, texels or a 32-bit input not 4-byte aligned, counts or size out of range, triangles that do not
   fit, a non-finite or non-positive depth_tol, cos_min outside [0, 1), a negative or non-finite z_min, frames outside 1 .. 8192 a
   side) returns non-zero before anything is launched. */
int mp_texture_bake(const float* d_vertices /*[n_vertices,3]*/, int n_vertices, const int32_t* d_faces /*[n_triangles,3]*/, int n_triangles,
                    const float* d_colors /*[n_vertices,3] or NULL*/, const float* d_depth /*[n,h,w]*/, const uint8_t* d_masks /*[n,h,w] or NULL*/,
                    const uint8_t* d_rgb /*[n,h,w,3]*/, const float* d_K /*[n,9]*/, const float* d_TCO /*[n,tco_floats]*/, int tco_floats, int n,
                    int h, int w, int size, float depth_tol, float cos_min, float z_min, int best_view, uint8_t* d_texels /*[size,size,4]*/,
                    uint8_t* d_seen /*[size,size]*/, mp_stream stream);

/* ------------------------------------------------------------------------------------ */
/* Cleaning up a triangle mesh (a reconstruction's, a heavy scan's): its connected          */
/* components, the selection of faces with the vertices they reference, and decimation by   */
/* vertex clustering, Rossignac-Borrel (csrc/mesh_cleanup.hip; contract in                  */
/* csrc/mesh_cleanup_core.h).  The reference has no counterpart; Open3D, trimesh and         */
/* meshlab are third party and absent: parity with them is unpinned.                        */
/* A mesh is V vertices [V,3] fp32 and F faces [F,3] int32, each 0 .. 2^29.  A face with an  */
/* index outside [0, V) is bad: it joins nothing, is never emitted, and its index is never   */
/* used as an address.  V == 0 or F == 0 is a success with zero totals.                      */
/* ------------------------------------------------------------------------------------ */
/* bytes of device scratch mp_mesh_components needs (0 for counts it rejects). */
size_t mp_mesh_components_workspace_bytes(int V, int F);
/* Connected components: d_labels[v] = the smallest vertex index of v's component (vertices joined by a chain of good faces; a vertex
   on no good face is its own label), d_face_labels[f] = the label of the face's first vertex or -1 for a bad face, d_face_count[l] = the
   good faces of label l (0 where l is not a label), d_totals = {components that own a face, the label of the one with the most faces
   (the smaller label on equal counts; -1 without any), bad faces, status}.  A lock-free union-find (atomicMin hooks the larger root
   under the smaller; d_labels is its parent array) whose loops are capped at V + 1 rounds: status is 0, or 1 when a loop reached the
   cap, and the labels are then not to be used.  Five launches and a memset on `stream`, nothing synchronises; the result is unique, so
   no arrival order changes it.  Any bad argument (a null pointer where one is needed, counts out of range, a workspace too small or
   not 16-byte aligned) returns non-zero before anything is launched. */
int mp_mesh_components(int V, const int32_t* d_faces /*[F,3]*/, int F, int32_t* d_labels /*[V]*/, int32_t* d_face_labels /*[F]*/,
                       int32_t* d_face_count /*[V]*/, int32_t* d_totals /*[4]*/, void* d_ws, size_t ws_bytes, mp_stream stream);
/* bytes of device scratch mp_mesh_select_count and mp_mesh_select need (0 for counts they reject). */
size_t mp_mesh_select_workspace_bytes(int V, int F);
/* Counts a selection: d_keep[f] != 0 keeps face f; d_totals = {vertices that a kept good face references, kept good faces, bad faces}.
   Flags by plain byte stores, two ordered rank passes (16 bytes a lane), one scan; no atomics but the count of bad faces.  What the
   call leaves in d_ws is the input of mp_mesh_select on the same mesh.  Bad arguments as above. */
int mp_mesh_select_count(int V, const int32_t* d_faces /*[F,3]*/, int F, const uint8_t* d_keep /*[F]*/, int32_t* d_totals /*[3]*/, void* d_ws,
                         size_t ws_bytes, mp_stream stream);
/* Writes the selection: the kept good faces in input order, the vertices they reference in input order, renumbered; vertices and
   (with d_colors) colours are copied bit for bit.  To be called after mp_mesh_select_count on the same mesh and workspace with the two
   totals it gave; every store is checked against them.  One launch on `stream`.  Refused before anything is launched: negative totals,
   capacities smaller than the totals, a null pointer where one is needed, counts out of range, a bad workspace. */
int mp_mesh_select(const float* d_vertices /*[V,3]*/, const float* d_colors /*[V,3] or NULL*/, int V, const int32_t* d_faces /*[F,3]*/, int F,
                   int n_vertices, int n_faces, float* d_out_vertices /*[cap_vertices,3]*/, float* d_out_colors /*[cap_vertices,3] or NULL*/,
                   int32_t* d_out_faces /*[cap_faces,3]*/, long long cap_vertices, long long cap_faces, void* d_ws, size_t ws_bytes,
                   mp_stream stream);
/* bytes of device scratch mp_mesh_cluster_count and mp_mesh_cluster need (0 for counts or a grid they reject). */
size_t mp_mesh_cluster_workspace_bytes(int V, int F, int gx, int gy, int gz);
/* Counts a decimation by vertex clustering on the grid of gx x gy x gz cells (each side 1 .. 512, at most 2^27 cells) of size `cell`
   from the origin: a vertex lies in cell floor((p - o) / cell) per axis; one outside the grid or with a non-finite coordinate is bad.
   A face is kept iff it is good, none of its vertices is bad and its three cells differ pairwise; a cell is used iff a kept face
   references it.  d_totals = {used cells = vertices out, kept faces, bad faces + faces dropped for a bad vertex}.  Two per-element
   launches, two rank passes, one scan; what the call leaves in d_ws is the input of mp_mesh_cluster.  Refused before anything is
   launched: dims out of range, a non-finite origin, a cell size that is not finite and > 0, and the bad arguments above. */
int mp_mesh_cluster_count(const float* d_vertices /*[V,3]*/, int V, const int32_t* d_faces /*[F,3]*/, int F, float ox, float oy, float oz,
                          float cell, int gx, int gy, int gz, int32_t* d_totals /*[3]*/, void* d_ws, size_t ws_bytes, mp_stream stream);
/* Writes the decimated mesh: output vertex = the rank of its used cell in cell-id order, at the exact mean of ALL good vertices of the
   cell (16.16 fixed-point grid coordinates summed in int64 by integer atomics, one float conversion per coordinate at the end; colours
   likewise in steps of 1/65535): no floating-point atomic, bit-reproducible whatever the arrival order.  Faces in input order with
   their corners in order; duplicate and opposite triangles are kept, so a closed mesh stays closed.  To be called after
   mp_mesh_cluster_count on the same mesh, grid and workspace with the two totals it gave; every store is checked against them.  A
   memset and two launches on `stream`.  Refused as mp_mesh_select and mp_mesh_cluster_count refuse. */
int mp_mesh_cluster(const float* d_vertices /*[V,3]*/, const float* d_colors /*[V,3] or NULL*/, int V, const int32_t* d_faces /*[F,3]*/, int F,
                    float ox, float oy, float oz, float cell, int gx, int gy, int gz, int n_vertices, int n_faces,
                    float* d_out_vertices /*[cap_vertices,3]*/, float* d_out_colors /*[cap_vertices,3] or NULL*/,
                    int32_t* d_out_faces /*[cap_faces,3]*/, long long cap_vertices, long long cap_faces, void* d_ws, size_t ws_bytes,
                    mp_stream stream);

/* ------------------------------------------------------------------------------------ */
/* BOP's model info: the exact diameter of a point set (the largest distance between two of */
/* its points: `diameter` of a BOP dataset's models_info.json, bop_toolkit's calc_model_info */
/* / calc_pts_diameter, an O(N^2) maximum) and its axis-aligned bounds                       */
/* (csrc/model_info.hip; contract in csrc/model_info_core.h).                                */
/* ------------------------------------------------------------------------------------ */
/* bytes of device scratch mp_model_info needs (0 for arguments it rejects: n_obj < 1, an object without points, a bad tile, more than
   2^31 - 1 jobs).  h_n_points [n_obj] is host memory. */
size_t mp_model_info_scratch_bytes(int n_obj, const int32_t* h_n_points, int tile);
/* For object o, over rows 0 .. n_points[o] - 1 of d_points[o] (the rows beyond are padding and are never read): d_d2[o] = the largest
   squared distance between two points, fmaf(dz, dz, fmaf(dy, dy, dx * dx)) on fp32 differences; d_pair[o] = the two rows (i <= j) that
   reach it, on equal distances the pair with the lowest i, then the lowest j; d_bounds[o] = min x y z, then size x y z (max - min).  The
   result is the maximum of a total order, so no tile, grid or arrival order changes a bit.  One point gives 0 and (0, 0).  An object with
   a NaN or infinite coordinate gives NaN, (-1, -1), NaN and leaves the other objects alone.  d_n_points (device) and h_n_points (host)
   hold the same n_obj counts, each in 1 .. stride.  tile = the j points of one LDS stage: 0 the library's choice, else a multiple of 64
   in 64 .. 1024 (a forced tile also shortens the chunk of a job, so that a few hundred points reach every path).  Two launches on
   `stream`, no atomics; the prefix array of job counts (n_obj + 1 entries) is copied from pageable host memory.  Any bad argument
   returns non-zero before anything is launched. */
int mp_model_info(const float* d_points /*[n_obj,stride,3]*/, int stride, const int32_t* d_n_points /*[n_obj]*/,
                  const int32_t* h_n_points /*[n_obj], host*/, int n_obj, int tile, void* d_scratch, float* d_d2 /*[n_obj]*/,
                  int32_t* d_pair /*[n_obj,2]*/, float* d_bounds /*[n_obj,6]*/, mp_stream stream);

/* ------------------------------------------------------------------------------------ */
/* Points drawn uniformly over the surface of triangle meshes: the reference's              */
/* MeshDataBase.batched(resample_n_points=n) (lib3d/rigid_mesh_database.py:100-104,          */
/* trimesh.sample.sample_surface), on uniforms the caller supplies                           */
/* (csrc/surface_sample.hip; contract in csrc/surface_sample_core.h).                        */
/* ------------------------------------------------------------------------------------ */
/* bytes of device scratch mp_surface_sample needs (0 for arguments it refuses: n_obj < 1, offsets that do not ascend, an object without
   faces or with more than 2^22, a bad block or one that cuts an object into more than 2048 blocks, count < 1).  h_face_off [n_obj + 1]
   is host memory. */
size_t mp_surface_sample_scratch_bytes(int n_obj, const int32_t* h_face_off, int count, int block);
/* For object o, with vertices vert_off[o] .. vert_off[o+1] - 1 of d_vertices and faces face_off[o] .. face_off[o+1] - 1 of d_faces
   (indices local to the object), and for sample s with the uniforms (u0, u1, u2) = d_u[o][s]: d_face[o][s] = the lowest face f whose
   inclusive prefix sum of quantised weights exceeds floor(total * k / 2^24), k = min((uint32)(u0 * 2^24), 2^24 - 1); d_points[o][s] =
   a + e1 * r1 + e2 * r2 on that face (fmaf, fp32) with (r1, r2) = (u1, u2) clamped to [0, 1] and reflected when r1 + r2 > 1.  A weight is
   twice the face's area in fp32, quantised to a 2^-40 grid under the object's largest weight, so all sums are exact integers and no
   grid, block size or arrival order changes a bit.  An object with a non-finite coordinate of a referenced vertex, an index outside
   its vertices (tested before the load), a non-finite weight or no area at all gives NaN points and face -1 and leaves the other
   objects alone.  The d_ and h_ prefix arrays hold the same n_obj + 1 values, starting at 0.  block = the faces of one job: 0 the
   library's choice (2048), else a multiple of 64 in 64 .. 2048 (for tests: a few hundred faces then make several blocks).  Five
   launches on `stream`, no atomics, no workgroup waits for another; the prefix array of job counts is copied from pageable host memory.
   Any bad argument returns non-zero before anything is launched. */
int mp_surface_sample(const float* d_vertices /*[V_total,3]*/, const int32_t* d_faces /*[F_total,3]*/, const int32_t* d_vert_off /*[n_obj+1]*/,
                      const int32_t* d_face_off /*[n_obj+1]*/, const int32_t* h_vert_off /*host*/, const int32_t* h_face_off /*host*/,
                      int n_obj, const float* d_u /*[n_obj,count,3]*/, int count, int block, void* d_workspace,
                      float* d_points /*[n_obj,count,3]*/, int32_t* d_face /*[n_obj,count]*/, mp_stream stream);

/* ------------------------------------------------------------------------------------ */
/* Object symmetries: does a candidate rotation about the object's centre map its surface    */
/* into itself within a tolerance?  The `symmetries_discrete` / `symmetries_continuous` of   */
/* a BOP models_info.json are built from the answers (evaluation.find_symmetries)            */
/* (csrc/symmetry.hip; contract in csrc/symmetry_core.h).                                    */
/* ------------------------------------------------------------------------------------ */
/* bytes of device scratch mp_symmetry_check needs (0 for n_obj < 1): the prefix arrays and tolerances of the call. */
size_t mp_symmetry_check_scratch_bytes(int n_obj);
/* For candidate k of object o (rows cand_off[o] .. cand_off[o+1] - 1 of d_cand_R, each a row-major 3x3 rotation R) with g(p) = R (p - c)
   + c, c = d_centers[o]: d_dev2[k] = the maximum over the object's test points p (rows test_off[o] .. test_off[o+1] - 1 of d_tests) of
   the minimum over its triangles (faces face_off[o] .. face_off[o+1] - 1 of d_faces, indices local to its vertices vert_off[o] ..
   vert_off[o+1] - 1 of d_vertices) of the squared point-to-triangle distance of g(p) (closest-point case analysis in fp32; a zero-area
   triangle acts as a segment or a point); d_worst[k] = the test point that reaches it, the lowest on equal distances; d_accept[k] =
   d_dev2[k] <= tol[o]^2.  mode 0: a screen with early outs sets d_accept (a lane stops at its first triangle within tol, a candidate at
   its first block of 256 test points with an unsatisfied lane), then only the accepted candidates are measured: a rejected one gets
   d_dev2 = NaN and d_worst = -1.  mode 1: every candidate is measured, no early out.  The flags of the two modes are equal; the result
   is the maximum of a total order, so no tile, grid or arrival order changes a bit.  A non-finite coordinate makes the distances it
   enters NaN, which never win: the candidate gets dev2 = +inf and is rejected.  The prefix arrays (n_obj + 1 entries, starting at 0),
   h_tol [n_obj] and h_faces (a copy of d_faces) are host memory; rows beyond the last prefix entry are padding and are never read.
   tile = the triangles of one LDS stage: 0 the library's choice (256), else a multiple of 64 in 64 .. 512.  At most 2^20 candidates in
   one call; none at all is a successful no-op.  One or two launches on `stream`, no atomics; the prefix arrays are copied from pageable
   host memory.  Any bad argument (n_obj < 1, an object without vertices, triangles or test points, a face index outside the object's
   vertices, a tol that is not finite or is negative, too many candidates, a bad tile or mode, a null pointer) returns non-zero before
   anything is launched. */
int mp_symmetry_check(const float* d_vertices /*[V_total,3]*/, const int32_t* d_faces /*[F_total,3]*/, const int32_t* h_faces /*host copy*/,
                      const float* d_tests /*[T_total,3]*/, const float* d_cand_R /*[C_total,9]*/, const float* d_centers /*[n_obj,3]*/,
                      const int32_t* h_vert_off /*host*/, const int32_t* h_face_off /*host*/, const int32_t* h_test_off /*host*/,
                      const int32_t* h_cand_off /*host*/, const float* h_tol /*[n_obj], host*/, int n_obj, int tile, int mode,
                      void* d_scratch, uint8_t* d_accept /*[C_total]*/, float* d_dev2 /*[C_total]*/, int32_t* d_worst /*[C_total]*/,
                      mp_stream stream);

/* ------------------------------------------------------------------------------------ */
/* Prediction overlays: the contour overlay of visualization/utils.py:56-85                 */
/* make_contour_overlay (get_mask_from_rgb, cv2.Canny(mask, 30, 100), cv2.dilate 3x3, masked */
/* paint), the mesh blend of visualization/bokeh_plotter.py:106-130 plot_overlay and the     */
/* box frames of visualization/utils.py:129-146 draw_bounding_box, on uint8 images on the    */
/* device (csrc/overlay.hip; contract in csrc/overlay_core.h).  OpenCV is third party: its   */
/* Canny, dilate and rectangle are restated, parity unpinned.                                */
/* ------------------------------------------------------------------------------------ */
/* For each of n images of h x w: the label of a pixel is d_labels' (< 0 background, l >= 0 an instance) or, with d_labels == NULL, 0
   where any channel of d_render is > 0 and -1 elsewhere.  A pixel is an EDGE of label l by OpenCV's Canny (L1 norm, aperture 3) on the
   0 / 1 mask m = [label == l]: gx, gy the 3x3 Sobel responses of m with the border replicated, mag = |gx| + |gy| (zero outside the
   image), and mag != 0 and non-maximum suppression with ax = |gx|, ay = |gy| << 15, t = ax * 13573: ay < t: mag > mag(x-1,y) and mag >=
   mag(x+1,y); else ay > t + (ax << 16): mag > mag(x,y-1) and mag >= mag(x,y+1); else with s = -1 when (gx ^ gy) < 0, else +1: mag >
   mag(x-s,y-1) and mag > mag(x+s,y+1).  (Every gradient of a 0 / 255 mask is a multiple of 255 and above both thresholds: hysteresis
   changes nothing.)  e(q) = the largest label with an edge at q, or -1; out(p) = the largest e(q) over the q of the image within
   Chebyshev distance k = dilate_iterations of p (k rounds of a 3x3 dilation per label, painted in ascending order).  d_contour = colour
   (out mod n_colors) of d_colors where out >= 0, else the pixel of d_images; d_canny = 255 where out >= 0, else 0; d_mask = 255 where
   label >= 0, else 0; d_mesh per channel = trunc((float)(render * 0.8 + 255 * 0.2)) where label >= 0, else trunc((float)(image * 0.6 +
   255 * 0.4)), the sums in float64 (two 256-entry tables).  Integer arithmetic throughout, no atomics, every output byte written by one
   thread: no grid or tile changes a bit.  Every output pointer is optional (NULL: not written).  h, w in 1 .. 8192, n * h * w * 3 <
   2^31, k in 0 .. 8, n_colors >= 1.  One launch on `stream`, no scratch.  n == 0 is a successful no-op; any other bad argument (null
   d_images or d_colors, neither d_render nor d_labels, d_mesh without d_render, a size, k or n_colors out of range) returns non-zero
   before anything is launched. */
int mp_overlay(const uint8_t* d_images /*[n,h,w,3]*/, const uint8_t* d_render /*[n,h,w,3] or NULL*/, const int32_t* d_labels /*[n,h,w] or NULL*/,
               const uint8_t* d_colors /*[n_colors,3]*/, int n_colors, int n, int h, int w, int dilate_iterations,
               uint8_t* d_contour /*[n,h,w,3] or NULL*/, uint8_t* d_canny /*[n,h,w] or NULL*/, uint8_t* d_mask /*[n,h,w] or NULL*/,
               uint8_t* d_mesh /*[n,h,w,3] or NULL*/, mp_stream stream);
/* Box frames on images: box j = d_boxes[j] (x1, y1, x2, y2, fp32, clamped to +-2^20 and truncated to integers; a box with a NaN
   corner draws nothing) belongs to image d_image_ids[j] (one outside 0 .. n - 1 draws nothing).  Corners are not reordered.  A pixel (x, y) is on frame j when it lies inside
   the box grown by t / 2 (x1 - t/2 <= x <= x2 + t/2, the same in y) and not inside the box shrunk by (t + 1) / 2 (x1 + (t+1)/2 <= x <=
   x2 - (t+1)/2, the same in y), t = thickness in 1 .. 8.  d_out = colour (j mod n_colors) of the highest such j of the pixel's image,
   else the pixel of d_images: a gather per pixel over the boxes, so no drawing order can race.  No text is drawn.  Sizes as mp_overlay;
   n_boxes >= 0 (0 copies the images).  One launch, no scratch.  n == 0 is a successful no-op; any other bad argument returns non-zero
   before anything is launched. */
int mp_draw_boxes(const uint8_t* d_images /*[n,h,w,3]*/, const float* d_boxes /*[n_boxes,4]*/, const int32_t* d_image_ids /*[n_boxes]*/,
                  int n_boxes, const uint8_t* d_colors /*[n_colors,3]*/, int n_colors, int n, int h, int w, int thickness,
                  uint8_t* d_out /*[n,h,w,3]*/, mp_stream stream);

/* ------------------------------------------------------------------------------------ */
/* Training-free detector: LINE-2D template matching on quantised gradient orientations   */
/* (the colour modality of LINE-MOD, Hinterstoisser et al., PAMI 2012), for objects that   */
/* have a mesh but no trained detector (csrc/template_match.hip; contract in               */
/* csrc/template_match_core.h).  Not in the reference; OpenCV's linemod is third party and */
/* absent, parity unpinned.  Integer arithmetic throughout, no atomics, no scratch: every  */
/* buffer is a typed tensor whose shape the caller states.                                 */
/* ------------------------------------------------------------------------------------ */
/* Quantised gradient orientations of n images d_images uint8 [n,h,w,3].  With blur != 0 each channel is first smoothed by the separable
   binomial (1 4 6 4 1) / 16, border replicated, rounded to nearest once after both passes.  Per channel the 3x3 Sobel responses (border
   replicated); the channel with the largest gx^2 + gy^2 wins (the lowest on a tie), mag2 = that sum.  The angle of (gx, gy) modulo 180
   degrees falls into one of eight half-open bins [k 22.5, (k + 1) 22.5), decided by integer comparisons ((|gy| + |gx|)^2 < 2 gx^2 for
   tan 22.5, (|gy| - |gx|)^2 < 2 gx^2 for tan 67.5).  A pixel is a candidate when mag2 >= weak_threshold^2 and mag2 > 0; it keeps bit o when
   at least 5 of the 9 pixels of its 3x3 neighbourhood (those inside the image) are candidates of bin o.  d_ori uint8 [n,h,w] (0 or one bit),
   d_mag2 int32 [n,h,w] or NULL.  h, w in 1 .. 8192, n * h * w * 3 < 2^31, weak_threshold in 0 .. 1443.  One launch on `stream`.  n == 0 is
   a successful no-op; any other bad argument returns non-zero before anything is launched. */
int mp_tm_quantize(const uint8_t* d_images /*[n,h,w,3]*/, int n, int h, int w, int blur, int weak_threshold, uint8_t* d_ori /*[n,h,w]*/,
                   int32_t* d_mag2 /*[n,h,w] or NULL*/, mp_stream stream);
/* Linearised response maps of d_ori: s(x, y) = the OR of d_ori over [x, x + T) x [y, y + T) clipped to the image, T in 1 .. 8; r_o(x, y) = 4
   when bit o is set in s, else 1 when bit o - 1 or o + 1 (circular over eight) is, else 0.  d_resp uint8 [n][8][T][T][gh][gw] with gh =
   ceil(h / T), gw = ceil(w / T): r_o(x, y) at [n][o][y mod T][x mod T][y div T][x div T], 0 in the cells beyond the image; every byte is
   written.  n * 8 * T * T * gh * gw < 2^31.  One launch.  n == 0 is a successful no-op; any other bad argument returns non-zero before
   anything is launched. */
int mp_tm_response(const uint8_t* d_ori /*[n,h,w]*/, int n, int h, int w, int T, uint8_t* d_resp /*[n,8,T,T,gh,gw]*/, mp_stream stream);
/* Every template at every grid location.  templates int32 [n_templates,5] = (object, first feature, n_features f, width, height), features
   uint8 [n_features,4] = (dx, dy, orientation index, 0), each on the device and as a host copy: the host copy is validated before anything
   is launched (0 <= object < n_objects, 1 <= f <= 63, sides in 1 .. 256, first + f <= n_features, dx < width, dy < height, index < 8).
   Template t at location (gx, gy) has its corner at pixel (gx T, gy T), is valid when its box lies inside the image, and scores the sum
   over its features of r_o(gx T + dx, gy T + dy).  Per (image, object, location) the best valid template by the exact ratio score / (4 f)
   (cross-multiplied integers), a tie to the lower index: d_best_score, d_best_f uint8 and d_best_template int32, each
   [n,n_objects,gh,gw]; 0, 0 and -1 where no template is valid.  n_objects in 1 .. 65535, n <= 65535, n_templates in 0 .. 2^20.  One
   launch.  n == 0 is a successful no-op; any other bad argument returns non-zero before anything is launched. */
int mp_tm_match(const uint8_t* d_resp /*[n,8,T,T,gh,gw]*/, int n, int h, int w, int T, const int32_t* d_templates /*[n_templates,5]*/,
                const int32_t* h_templates /*host copy*/, const uint8_t* d_features /*[n_features,4]*/, const uint8_t* h_features /*host copy*/,
                int n_templates, int n_features, int n_objects, uint8_t* d_best_score /*[n,n_objects,gh,gw]*/,
                uint8_t* d_best_f /*[n,n_objects,gh,gw]*/, int32_t* d_best_template /*[n,n_objects,gh,gw]*/, mp_stream stream);

/* ------------------------------------------------------------------------------------ */
/* Depth refiner (ICP): replaces inference/icp_refiner.py:128-175 icp_refinement +          */
/* :195-262 ICPRefiner.refine_poses (masks refiner_utils.py:30-56).  The reference's ICP    */
/* core is OpenCV-contrib ppf_match_3d_ICP (third party, parity unpinned); this is a        */
/* projective point-to-plane ICP with the same budget / acceptance rule (csrc/icp.hip).     */
/* d_depth_meas [n_images,H,W] metres (0 = invalid), d_depth_rend [n_rows,H,W] rendered at  */
/* d_TCO, d_K_images [n_images,3,3], d_K_rows [n_rows,3,3].  retval[n] = 0 ok / -1 kept.    */
/* user_masks != 0: the caller's segmentation masks have been applied to d_depth_meas and     */
/* the |measured - rendered| <= 0.1 m test is skipped (icp_refiner.py:249-250).               */
/* ------------------------------------------------------------------------------------ */
size_t mp_icp_workspace_bytes(int n_images, int n_rows, int H, int W);
int mp_icp_refine(const float* d_depth_meas, int n_images, const int32_t* d_im_ids, const float* d_depth_rend,
                  const float* d_K_images, const float* d_K_rows, const float* d_TCO, int n_rows, int H, int W,
                  int n_iterations, int n_levels, float tolerance, int n_min_points, int user_masks, float* d_TCO_out,
                  int32_t* d_retval, float* d_residual, void* d_workspace, size_t workspace_bytes, mp_stream stream);

/* The same refiner with the REFERENCE's algorithm, step for step (csrc/icp_nn.hip): get_normal (hole fill, Gaussian sigma 2, gradient,
 * inference/icp_refiner.py:37-95), getXYZ, masks / 1000-point rule, centroid pre-shift, and OpenCV's ppf_match_3d ICP as restated in
 * oracle/icp_opencv.py (mean / scale normalisation, 4 levels, exact nearest neighbours, median + 2.5 MAD rejection, one-to-one filter,
 * linearised point-to-plane solve, relative-change stop).  Arguments as mp_icp_refine (n_iterations = 100, n_levels = 4, tolerance = 0.05
 * are the reference's) except d_masks: the caller's per-frame masks [n_images][H][W] uint8 (icp_refiner.py:249-250: they replace the
 * threshold mask and only select points -- the measured depth is passed unmasked, its normals come from the whole frame) or NULL; d_iters (optional, [n_rows][8] int32) receives the iterations run per level.  At most
 * mp_icp_nn_max_points() mask pixels per object (more -> that object is rejected, retval -1). */
int mp_icp_nn_max_points(void);
size_t mp_icp_nn_workspace_bytes(int n_images, int n_rows, int H, int W);
int mp_icp_refine_nn(const float* d_depth_meas, int n_images, const int32_t* d_im_ids, const float* d_depth_rend, const float* d_K_images,
                     const float* d_K_rows, const float* d_TCO, int n_rows, int H, int W, int n_iterations, int n_levels, float tolerance,
                     int n_min_points, const unsigned char* d_masks, float* d_TCO_out, int32_t* d_retval, float* d_residual, int32_t* d_iters,
                     void* d_ws, size_t ws_bytes, mp_stream stream);

/* ------------------------------------------------------------------------------------ */
/* Depth refiner (TEASER++): replaces inference/teaserpp_refiner.py:53-162                  */
/* compute_teaserpp_refinement + :193-289 TeaserppRefiner.refine_poses (masks               */
/* refiner_utils.py:30-56, points visualization/meshcat_utils.py:278-300).  pytorch3d's     */
/* farthest point sampling and teaserpp_python's solver are third party (parity unpinned);  */
/* the algorithm is the one stated in csrc/teaser_core.h and csrc/teaser_clique_core.h      */
/* (csrc/teaser.hip, csrc/teaser_clique.hip).                                               */
/* ------------------------------------------------------------------------------------ */
/* Farthest point sampling of n_rows point sets d_points [n_rows,stride,3] fp32, of which the first d_counts[r] (clamped to 0 .. stride)
   are valid: M = min(n_points, count) picks; pick 0 is point 0, every later pick the point with the largest running minimum of the
   squared fp32 distance to the picks so far, a tie to the lowest index (pytorch3d.ops.sample_farthest_points without a random start).
   use_fps == 0: index floor(k * count / M) instead.  d_idx [n_rows,n_points] int32 (-1 past M), d_m [n_rows] = M.  One launch, one
   workgroup per row; d_workspace of mp_fps_workspace_bytes(n_rows, stride) bytes.  Any bad argument returns non-zero before the launch. */
size_t mp_fps_workspace_bytes(int n_rows, int stride);
int mp_fps(const float* d_points, const int32_t* d_counts, int n_rows, int stride, int n_points, int use_fps, int32_t* d_idx, int32_t* d_m,
           void* d_workspace, size_t workspace_bytes, mp_stream stream);
/* bytes of scratch of mp_teaser_refine for n_rows rows of H x W frames; with H = W = 0, of mp_teaser_solve (0 for sizes it refuses). */
size_t mp_teaser_workspace_bytes(int n_rows, int H, int W);
/* Robust registration of given correspondences d_src[r][k] -> d_dst[r][k], k < d_counts[r] <= stride <= 1024 ([n_rows,stride,3] fp32):
   consistency graph (edge when the two pair distances differ by at most 2 noise_bound), inlier selection (0: the vertices of the largest
   core number; 1: every vertex; 2: a maximum clique, see mp_teaser_solve_ex), GNC-TLS rotation over the TIMs of the selected vertices (tim_graph 0: consecutive pairs, 1: all pairs),
   component-wise TLS translation, inlier count over all correspondences.  d_Rt [n_rows,12] float64 = [R t] row-major (the identity for
   a row with fewer than 3 selected vertices), d_retval [n_rows] = 0 when num_inliers >= min_num_inliers, else -1.  Optional (NULL to
   skip): d_degree, d_core, d_selected [n_rows,stride] int32 (-1 past a row's count), d_info [n_rows,5] int32 =
   count, count, selected, GNC iterations, num_inliers.  Three launches; no atomics, every sum in a fixed order.  Any bad argument
   returns non-zero before anything is launched. */
int mp_teaser_solve(const float* d_src, const float* d_dst, const int32_t* d_counts, int n_rows, int stride, float noise_bound,
                    int inlier_selection, int tim_graph, int min_num_inliers, double* d_Rt, int32_t* d_retval, int32_t* d_degree,
                    int32_t* d_core, int32_t* d_selected, int32_t* d_info, void* d_workspace, size_t workspace_bytes, mp_stream stream);
/* The whole refiner from depth frames: d_depth_meas [n_images,H,W] metres, d_depth_rend [n_rows,H,W] rendered at d_TCO, d_K_rows
   [n_rows,3,3].  Mask (mask_type 0 "simple": measured > 0 and rendered > 0; 1 "threshold": also |measured - rendered| <=
   depth_delta_thresh), back-projection of both depths at the N mask pixels, M = min(n_points, N) samples of the source points (a row
   with N < n_min_points keeps its pose), then mp_teaser_solve's chain; an accepted row's pose becomes [R t] * TCO.  n_points <= 1024.
   Optional outputs as mp_teaser_solve with stride = n_points, d_sample_idx [n_rows,n_points] = indices into the row's mask pixels (-1 past
   M), d_info = N, M, selected, GNC iterations, num_inliers.  Six launches on `stream`, no host round trip. */
int mp_teaser_refine(const float* d_depth_meas, int n_images, const int32_t* d_im_ids, const float* d_depth_rend, const float* d_K_rows,
                     const float* d_TCO, int n_rows, int H, int W, int mask_type, float depth_delta_thresh, int n_min_points, int n_points,
                     float noise_bound, int min_num_inliers, int use_fps, int inlier_selection, int tim_graph, float* d_TCO_out,
                     int32_t* d_retval, double* d_Rt, int32_t* d_sample_idx, int32_t* d_degree, int32_t* d_core, int32_t* d_selected,
                     int32_t* d_info, void* d_workspace, size_t workspace_bytes, mp_stream stream);
/* Exact maximum-clique inlier selection (inlier_selection 2: TEASER++'s default, PMC_EXACT): a bounded, deterministic branch and bound
   on the consistency graph (the rule is stated in csrc/teaser_clique_core.h, the kernel is csrc/teaser_clique.hip).  The selected
   vertices are the members of a maximum clique -- of the equal ones the first the rule meets -- or, when the search has coloured more
   than max_clique_steps vertices, the best clique found until then (exact = 0).  mp_max_clique_default_steps() is the budget the
   entries without the argument use; an argument may ask for 0 .. 16 times as much.
   mp_max_clique: the search alone on n_rows adjacency matrices d_adjacency [n_rows,stride,stride] uint8, stride <= 1024, of which the
   first d_counts[r] vertices (NULL: stride) are the graph; an edge exists when i != j and a[i][j] | a[j][i].  d_members [n_rows,stride]
   int32 = the members in ascending order, -1 past the size; d_info [n_rows,4] int32 = size, upper bound (largest core number + 1),
   exact, steps.  Three launches (pack, peel, search), one wave per row, no atomics. */
int mp_max_clique_default_steps(void);
size_t mp_max_clique_workspace_bytes(int n_rows, int stride);
int mp_max_clique(const uint8_t* d_adjacency, const int32_t* d_counts, int n_rows, int stride, int max_steps, int32_t* d_members, int32_t* d_info,
                  void* d_workspace, size_t workspace_bytes, mp_stream stream);
/* mp_teaser_workspace_bytes, mp_teaser_solve and mp_teaser_refine with the step budget and the optional d_clique_info [n_rows,4] (as
   d_info of mp_max_clique; written with inlier_selection 2 only).  The size also takes stride (= n_points of mp_teaser_refine) and the
   selection: only selection 2 allocates search stacks.  The three entries above are these with the default budget and NULL; they
   accept inlier_selection 2 when the workspace has the size given here.  With selections 0 and 1 nothing differs, bit for bit.
   A negative max_clique_steps or one above 16 times the default returns non-zero before anything is launched. */
size_t mp_teaser_workspace_bytes_ex(int n_rows, int H, int W, int stride, int inlier_selection);
int mp_teaser_solve_ex(const float* d_src, const float* d_dst, const int32_t* d_counts, int n_rows, int stride, float noise_bound,
                       int inlier_selection, int tim_graph, int min_num_inliers, double* d_Rt, int32_t* d_retval, int32_t* d_degree,
                       int32_t* d_core, int32_t* d_selected, int32_t* d_info, int max_clique_steps, int32_t* d_clique_info, void* d_workspace,
                       size_t workspace_bytes, mp_stream stream);
int mp_teaser_refine_ex(const float* d_depth_meas, int n_images, const int32_t* d_im_ids, const float* d_depth_rend, const float* d_K_rows,
                        const float* d_TCO, int n_rows, int H, int W, int mask_type, float depth_delta_thresh, int n_min_points, int n_points,
                        float noise_bound, int min_num_inliers, int use_fps, int inlier_selection, int tim_graph, float* d_TCO_out,
                        int32_t* d_retval, double* d_Rt, int32_t* d_sample_idx, int32_t* d_degree, int32_t* d_core, int32_t* d_selected,
                        int32_t* d_info, int max_clique_steps, int32_t* d_clique_info, void* d_workspace, size_t workspace_bytes, mp_stream stream);

/* ------------------------------------------------------------------------------------ */
/* Detector network: replaces the torchvision Mask R-CNN    */
/* behind `self.model([image_n ...])` in inference/detector.py:92                          */
/* (models/mask_rcnn.py:23-46 = MaskRCNN(resnet_fpn_backbone("resnet50"), num_classes,     */
/* AnchorGenerator(((32,),(64,),(128,),(256,),(512,)), ((0.5,1,2),)*5), min/max_size);     */
/* all other hyper-parameters torchvision 0.12 defaults).  One call runs the whole         */
/* inference graph on the device: normalise + resize + pad, ResNet-50 + FPN (the fp32 MFMA */
/* convolution of this library, FrozenBatchNorm folded), RPN (top-k, decode, NMS), RoIAlign,*/
/* box head (the two FC layers run as 1x1 convolutions on the same kernel), per-class NMS, */
/* mask head and mask pasting.  No host synchronisation, deterministic (ties resolve to    */
/* the lower index).  csrc/detector.hip.                                                   */
/* ------------------------------------------------------------------------------------ */
typedef struct mp_detector mp_detector;

typedef struct {
  int32_t n_classes;               /* including the background class 0                                           */
  int32_t min_size, max_size;      /* GeneralizedRCNNTransform (cfg.input_resize: (480, 640) for the released detectors) */
  float image_mean[3], image_std[3];
  int32_t anchor_sizes[5];         /* one per pyramid level P2..P6                                                */
  float aspect_ratios[3];
  int32_t rpn_pre_nms_top_n, rpn_post_nms_top_n;   /* <= 1024 each                                              */
  float rpn_nms_thresh, rpn_score_thresh, rpn_min_size;
  float box_score_thresh, box_nms_thresh, box_min_size;
  int32_t box_detections_per_img;                  /* <= 1024                                                    */
} mp_detector_config;

/* torchvision's eval defaults: 1000 / 1000 / 0.7 / 0.0 / 1e-3, 0.05 / 0.5 / 1e-2 / 100, ImageNet mean / std, the reference's anchors */
int mp_detector_default_config(mp_detector_config* cfg, int n_classes, int min_size, int max_size);
/* The checkpoint layout the detector expects (torchvision's state_dict keys: backbone.body.*, backbone.fpn.*, rpn.head.*,
 * roi_heads.*): entry `idx` -> name, dims.  Returns 1 past the end.  Host only. */
int mp_detector_state_spec(int n_classes, int idx, char* name, int name_len, int64_t* shape4, int32_t* n_dims);
int mp_detector_create(const mp_detector_config* cfg, const mp_named_tensor* h_state, int n_tensors, mp_detector** out);
int mp_detector_destroy(mp_detector* det);
size_t mp_detector_workspace_bytes(const mp_detector* det, int n_images, int H, int W);
/* d_images [n,3,H,W] fp32 in [0,1] (what Detector.get_detections passes, detector.py:88-92).  Outputs, D = box_detections_per_img:
 * d_boxes [n,D,4] (x1,y1,x2,y2 in ORIGINAL image pixels), d_scores [n,D], d_labels [n,D] (category ids >= 1), d_counts [n]; entries
 * past the count are zero.  d_masks: NULL or [n,D,H,W] soft masks in [0,1] pasted into the original frame (roi_heads.py
 * paste_masks_in_image); the caller thresholds them (detector.py:106).  Images of one call share H x W. */
int mp_detector_forward(mp_detector* det, const float* d_images, int n_images, int H, int W, float* d_boxes, float* d_scores,
                        int32_t* d_labels, int32_t* d_counts, float* d_masks, void* d_workspace, size_t workspace_bytes,
                        mp_stream stream);
/* Parity taps (tests): after a forward, the device address + logical shape of an intermediate inside `d_workspace`:
 * "P2".."P6" padded-NHWC pyramid levels {n, h, w, 256} with border 1; "x0" the preprocessed batch {n, Hp, Wp, 4} with border 3;
 * "pool" the stem + max-pool output {n, Hp/4, Wp/4, 64} and "C2".."C5" the ResNet stage outputs the FPN read {n, h, w, 256 << (k-2)}, border 1;
 * "L2".."L5" the FPN's top-down maps (lateral 1x1 + upsampled upper level; P_k is the 3x3 convolution of L_k) {n, h, w, 256}, border 1;
 * "roi7" the box head's RoIAlign rows {n*post, 7*7*256} ((y, x, channel) order); "roi14" the mask head's {n*D, 14, 14, 256} with border 1;
 * "keys" the RPN objectness logits {n, anchors} in (level, y, x, anchor) order; "proposals" {n, post_nms_top_n, 4} + "proposal_counts" {n} (int32);
 * "class_logits" {n*post, padded 5*n_classes row: n_classes logits then 4*n_classes deltas}; "mask_logits" {n*D*14*14*4, padded n_classes}.
 * Returns MP_ERR_INVALID for an unknown name or before the first forward. */
int mp_detector_debug_tensor(const mp_detector* det, const char* what, const void** d_ptr, int64_t* shape4, int32_t* border,
                             int64_t* row_stride, int64_t* n_elements /* 4-byte elements of the whole buffer (borders / row padding included) */);

#ifdef __cplusplus
}
#endif
#endif /* MP_ENGINE_H */
