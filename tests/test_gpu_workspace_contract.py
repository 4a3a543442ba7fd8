"""GPU: every engine entry that takes a device workspace, run on DIRTY scratch between canaries.

`engine.py` hands the kernels their workspace as `torch.empty(...)`; in a fresh test process the caching allocator mostly returns
zeros.  The other GPU tests pin each entry's values to its emulation bit for bit, but always on such memory.  This module repeats each
entry's launch with the workspace taken from `support.workspace_arena` instead (monkeypatched over `engine._workspace`; for `MeshDB`
a slice of exactly `mp_raster_workspace_bytes` is put into `db._ws[slot]`), in five states:

    want  unpatched engine                          the values the other tests pin to the emulations
    A     arena filled 0x00                         clean memory
    B     arena filled 0xFF                         every int -1, every float a NaN, every flag set
    C     arena filled with seeded random bytes     neither
    D     keep() after C, the same launch again     the launch's own leftovers (counters not reset, ...)
    E     keep() after ANOTHER launch in the bytes  another entry's leftovers; for the rasteriser a LARGER launch (more views, a bigger
                                                    frame) on the same database and slot, which is what production reuses

After every run the device is synchronised and every canary byte (256 B before, 4096 B behind the reported size, 0xA5) is checked;
then every output of A .. E must equal `want` bit for bit (floats through their bytes).  Nothing is compared with a tolerance: the
reference is the project's own result on a fresh allocation, which the other tests tie to the float64 and emulation oracles.

"Passes on dirty memory" holds for the shapes listed here, not in general.  Every case has the shape "one" (the smallest the entry
accepts) and "off" (every tiled count off a multiple of 64 and 256 and across one boundary); "tight" where a small shape exists at
which the plan's last region ends on the last reported byte, so that an overrun of a single byte reaches the canary.

Outputs compared in part (a cap on what is skipped, not a convenience; no output is left out entirely):
  * `raster_job_flags`: "one byte per (item, 8x8-pixel tile)" (engine.raster_job_flags) -- n_items * n_tiles bytes are compared; the
    bytes up to the next multiple of 16 that pad the region belong to no pair.
Every other output is compared whole: the headers specify the tails (pose errors: "Outputs sized by n_pts have a zero / -1 tail";
sampling, clique and TEASER telemetry: "-1 past" the row's count; symmetry: NaN / -1 for a rejected candidate).

Not covered here:
  * `Backbone.workspace`, `DetectorNet` (mp_backbone_workspace_bytes, mp_detector_workspace_bytes): their workspaces carry zeroed
    borders that mp_backbone_workspace_reset establishes once per allocation, so an arbitrary fill is outside their contract.
  * `icp_refine`, both associations (mp_icp_workspace_bytes, mp_icp_nn_workspace_bytes):
    test_gpu_icp_edges.py::test_refiners_read_nothing_of_the_workspace_they_have_not_written does this for them.
  * mp_teaser_workspace_bytes: mp_teaser_workspace_bytes_ex at stride 1024, k-core; no wrapper calls it.

The audit: per region the first writer and its extent, the readers and theirs (read before anything ran on a device; b rows, S
symmetries, nch = ceil(n_pts / 256), P = n_prob, N nodes / elements, nb workgroups).  "slack" = reported size - last used byte.

  entry / size function            region           first written by (extent)                      read by (extent)                    slack: one | off | tight
  pose_error_sym, _mspd            part f32         sym_partial: s < n_sym, every c < nch          sym_finalize: the same              fixed 256 + rounding: 504 | 6416 (the
    mp_pose_error_workspace_bytes  (b S nch 2)      (chunks past n_points hold 0)                                                      size also covers the NN launch)
  pose_error_nn (same function)    keys u64 (b n)   hipMemsetAsync 0xff, b * n_pts                 nn_pairs atomicMin, nn_finalize j < nv  fixed 256 + rounding: 504 | 488
  vsd  mp_vsd_workspace_bytes      counters i32     hipMemsetAsync 0, b * (2 + n_tau)              count atomicAdd, finalize row < b   fixed 256: 464 | 264
  gt_info  mp_gt_info_..           acc i32 (b 12)   gt_info_init_kernel, b * 12                    count atomics, finalize row < b     fixed 256 (by design): 464 | 272
  bop_match  mp_bop_match_..       taken u32        each lane zeroes its own taken_words(n_gt)     the same lane, bits < n_gt          fixed 256: 256 | 256
                                   (words E theta)  words (slow path only; the fast path keeps 64 bits in a register)
  det_match  mp_det_match_..       taken u32        as bop_match, every group                      the same lane                       fixed 256: 256 | 256
  rle_encode  mp_rle_workspace_..  offsets i64      hipMemcpyAsync n + 1 (encode call)             walk<true> m, m + 1 <= n            last region mask_tot (n 2 i32):
                                   ent_count/_last  walk<false>: x < w of every job                scan, walk<true>: x < w             248 | 176 | 0 at n = 32
                                   job_stats        walk<false>: every job                         scan: S * U per mask
                                   mask_tot         scan: 2 per mask                               walk<true>: 2 per mask
  rle_decode  mp_rle_decode_..     offsets, ends    memcpy n + 1; ends_kernel i < n_runs           seek / fill: inside a list          fixed 256 + rounding: 508 | >= 256
                                   ent_run          seek: g < n_ent                                fill: x < w
  tsdf_extract                     flags cell emask flags / cells / count kernels: g < N           count, emit: g < N (neighbours      last region block_nt (nb i32):
    mp_tsdf_extract_workspace_..   lrank u16        count: g < N                                   bounds-checked against the grid)    252 | 176 | 0 at 16 x 32 x 32
                                   block_nv/_nt     count: one per workgroup                       scan b < nb, emit blockIdx.x
  mesh_components  mp_mesh_comp..  counters (256 B) hipMemsetAsync 0, 256                          atomics, totals kernel: 5 ints      236 (fixed: 256 B for 5 ints)
  mesh_select  mp_mesh_select_..   counters         memset 0, 256                                  atomicAdd, scan                     last region f.base (nb_f i32):
                                   v.bytes          memset 0, nb_v * 4096                          rank e0 < V (16 B, masked to V)     252 | 248 | 0 at F = 262 144
                                   f.bytes          select_faces: f < F                            rank e0 < F (16 B, masked to F)
                                   lrank, base      rank: every group, every workgroup             scan, mc_rank
  mesh_cluster_count (same plan    counters, vcell  memset; cells_kernel v < V                     faces kernel (good indices only)    the plan ends with acc, which the
    as mesh_cluster)               u.bytes          memset 0, nb_u * 4096                          rank (masked to cells)              count call does not use
                                   f.bytes ..       as mesh_select
  mesh_cluster                     acc u64 (6 nv),  hipMemsetAsync 0, nv * 52 (nv = vertices out   accumulate atomicAdd r < nv,        last region acc (max_out * 52):
    mp_mesh_cluster_workspace_..   acc_count (nv)   <= max_out = min(cells, V))                    emit g < nv                         100 | (max_out - nv) * 52 or more |
                                                                                                                                       0 at 128 cells, all of them used
  model_info                       job_off i32      hipMemcpyAsync n_obj + 1                       pairs / reduce: obj, obj + 1        0 at every shape (the partials
    mp_model_info_scratch_bytes    partials int4    pairs kernel: one per job                      reduce: job_off[obj] .. [obj + 1]   end the plan, unpadded)
  symmetry_check                   meta i32         hipMemcpyAsync 5 n_obj + 4 words               object_info: inside them            220 | 0 at n_obj = 12
    mp_symmetry_check_scratch_..
  surface_sample                   job_off, obj_e   memcpy; block_sum kernel (block 0 of an obj)   every later kernel                  last region C (faces u64):
    mp_surface_sample_scratch_..   job_max/_bad     weights: one per job                           block_sum: the object's jobs        248 | 144 | 0 at 64 faces
                                   block_sum        block_sum: one per job                         prefix, scan, pick: the object's
                                   w, C             weights / scan: i < the block's faces          block_sum, scan, pick: the same
  farthest_point_sample            mind f32         teaser_fps: i in [16384, N) = INFINITY         the same thread, the same i         fixed 256 + rounding: 508 | >= 256
    mp_fps_workspace_bytes         (rows stride)    (touched only when N > 16384)
  max_clique                       adj              clique_pack: rows of the tiles below M         kcore v < M, search v < M           fixed 256 (behind the search
    mp_max_clique_workspace_bytes  core sel ..      kcore v < M; search: list to stride            search v < M; memcpy2D stride       stacks)
                                   order / pset     search: written before read at every depth     the same workgroup
  teaser_solve, teaser_refine      m_arr, n_arr     memcpy of the counts / compact, fps            every kernel                        fixed 256 (by design)
    mp_teaser_workspace_bytes_ex   deg core sel     hipMemsetAsync 0xFF (3 regions), then v < M    memcpy2D [n][stride] telemetry
    (kcore and max_clique plans)   adj, sel_list    graph: tiles below M; kcore / search           kcore, search v < M; solve < msel
                                   src dst idx      gather k < M; fps: all n_points                graph k < M; gather k < M
                                   pts pix mind     compact pos < N; fps as above                  fps i < N; gather through idx
  raster_render                    view blocks      raster_bin: headers, offsets, lists up to      raster_tiles: up to the totals      last region view_flags (pairs
    mp_raster_workspace_bytes      counters (4)     their totals; view 0 zeroes the 4 counters     classify atomicAdd, light kernel    rounded up to 16): 15 | 0 (576
                                   light_list       classify: base + rank < counters[0]            light kernel: j < counters[0]       pairs) ; job flags 4 | 0 (768)
                                   job_flags        classify: idx < items * tiles                  raster_tiles: the same
                                   view_flags       raster_bin: every (view, tile)                 classify: the same
  raster_render_scene              view blocks      raster_bin (no counters, no flags)             scene tiles                         fixed 16 (by design)
    mp_raster_scene_workspace_..   K_obj, lights    raster_scene_prep: o < n_obj                   bin, tiles: o < n_obj

No region was found whose read extent exceeds its written extent.
"""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

# ---------------------------------------------------------------------------------------------------------------------------------------
# The table.  Plain data: tests/test_workspace_arena_cpu.py imports it without a device and holds it against engine.py and
# include/mp_engine.h.  name -> entry (the engine function), via (how the entry obtains its workspace), size_fns (the size functions
# the entry calls), shapes, after (shape -> the launch that leaves its state for run E; None: a donor launch of another entry).
# ---------------------------------------------------------------------------------------------------------------------------------------
_WS, _DB = "_workspace", "MeshDB.workspace"
_PE = ("mp_pose_error_workspace_bytes",)
_TE = ("mp_teaser_workspace_bytes_ex",)
CASES = {
    "pose_error_sym": dict(entry="pose_error_sym", via=_WS, size_fns=_PE, shapes=("one", "off")),
    "pose_error_mspd": dict(entry="pose_error_mspd", via=_WS, size_fns=_PE, shapes=("one", "off")),
    "pose_error_nn": dict(entry="pose_error_nn", via=_WS, size_fns=_PE, shapes=("one", "off")),
    "vsd": dict(entry="vsd", via=_WS, size_fns=("mp_vsd_workspace_bytes",), shapes=("one", "off")),
    "gt_info": dict(entry="gt_info", via=_WS, size_fns=("mp_gt_info_workspace_bytes",), shapes=("one", "off")),
    "bop_match": dict(entry="bop_match", via=_WS, size_fns=("mp_bop_match_workspace_bytes",), shapes=("one", "off")),
    "det_match": dict(entry="det_match", via=_WS, size_fns=("mp_det_match_workspace_bytes",), shapes=("one", "off")),
    "rle_encode": dict(entry="rle_encode", via=_WS, size_fns=("mp_rle_workspace_bytes",), shapes=("one", "off", "tight")),
    "rle_decode": dict(entry="rle_decode", via=_WS, size_fns=("mp_rle_decode_workspace_bytes",), shapes=("one", "off")),
    "tsdf_extract": dict(entry="tsdf_extract", via=_WS, size_fns=("mp_tsdf_extract_workspace_bytes",), shapes=("one", "off", "tight")),
    "mesh_components": dict(entry="mesh_components", via=_WS, size_fns=("mp_mesh_components_workspace_bytes",), shapes=("one", "off")),
    "mesh_select": dict(entry="mesh_select", via=_WS, size_fns=("mp_mesh_select_workspace_bytes",), shapes=("one", "off", "tight")),
    "mesh_cluster_count": dict(entry="mesh_cluster_count", via=_WS, size_fns=("mp_mesh_cluster_workspace_bytes",), shapes=("one", "off")),
    "mesh_cluster": dict(entry="mesh_cluster", via=_WS, size_fns=("mp_mesh_cluster_workspace_bytes",), shapes=("one", "off", "tight")),
    "model_info": dict(entry="model_info", via=_WS, size_fns=("mp_model_info_scratch_bytes",), shapes=("one", "off")),
    "symmetry_check": dict(entry="symmetry_check", via=_WS, size_fns=("mp_symmetry_check_scratch_bytes",), shapes=("one", "tight")),
    "surface_sample": dict(entry="surface_sample", via=_WS, size_fns=("mp_surface_sample_scratch_bytes",), shapes=("one", "off", "tight")),
    "farthest_point_sample": dict(entry="farthest_point_sample", via=_WS, size_fns=("mp_fps_workspace_bytes",), shapes=("one", "off")),
    "max_clique": dict(entry="max_clique", via=_WS, size_fns=("mp_max_clique_workspace_bytes",), shapes=("one", "off")),
    "teaser_solve/kcore": dict(entry="teaser_solve", via=_WS, size_fns=_TE, shapes=("one", "off")),
    "teaser_solve/max_clique": dict(entry="teaser_solve", via=_WS, size_fns=_TE, shapes=("one", "off")),
    "teaser_refine/kcore": dict(entry="teaser_refine", via=_WS, size_fns=_TE, shapes=("one", "off")),
    "teaser_refine/max_clique": dict(entry="teaser_refine", via=_WS, size_fns=_TE, shapes=("one", "off")),
    # the rasteriser: the shapes name launches of RASTER_LAUNCHES; run E follows the larger launch named in `after` on the same slot
    "raster_render/plain": dict(entry="raster_render", via=_DB, size_fns=("mp_raster_workspace_bytes",), shapes=("one", "off"),
                                launches=dict(one="pyramid_1_8x8", off="A_3_92x124"), after=dict(one="pyramid_3_20x28", off="A_4_96x128")),
    "raster_render/job_flags": dict(entry="raster_render", via=_DB, size_fns=("mp_raster_workspace_bytes",), shapes=("one", "off"), reads="raster_job_flags",
                                    launches=dict(one="pyramid_item2_12x20", off="A_item4_92x124"),
                                    after=dict(one="pyramid_2items_20x28", off="A_2items_96x128")),
    "raster_render_scene": dict(entry="raster_render_scene", via=_WS, size_fns=("mp_raster_scene_workspace_bytes",), shapes=("one", "off")),
}
# launch -> (mesh, views, views_per_item, h, w); the views: N = near (mesh A: its lists overflow), F = far, E = a non-finite pose
RASTER_LAUNCHES = {
    "pyramid_1_8x8": ("pyramid", "N", 1, 8, 8),
    "pyramid_3_20x28": ("pyramid", "NEF", 1, 20, 28),
    "pyramid_item2_12x20": ("pyramid", "NF", 2, 12, 20),
    "pyramid_2items_20x28": ("pyramid", "NFEN", 2, 20, 28),
    "A_3_92x124": ("A", "NFE", 1, 92, 124),
    "A_4_96x128": ("A", "NFEN", 1, 96, 128),
    "A_item4_92x124": ("A", "EFNF", 4, 92, 124),
    "A_2items_96x128": ("A", "NFEFFFNE", 4, 96, 128),
}
# size functions of include/mp_engine.h that no case reaches, each with its reason (see the module docstring)
EXCLUDED_SIZE_FNS = {
    "mp_backbone_workspace_bytes": "zeroed borders established once per allocation by mp_backbone_workspace_reset: an arbitrary fill is outside the contract",
    "mp_detector_workspace_bytes": "as the backbone's: the detector's workspace carries zeroed borders",
    "mp_icp_workspace_bytes": "covered by test_gpu_icp_edges.py::test_refiners_read_nothing_of_the_workspace_they_have_not_written",
    "mp_icp_nn_workspace_bytes": "covered by test_gpu_icp_edges.py::test_refiners_read_nothing_of_the_workspace_they_have_not_written",
    "mp_teaser_workspace_bytes": "mp_teaser_workspace_bytes_ex at stride 1024 and k-core selection; no wrapper calls it",
}
# launches of other entries whose leftovers run E starts from, by ascending workspace: the first that is another entry's and large enough
# (tsdf_extract "big" is no tested shape: 96 x 96 x 64 nodes, 5 bytes of workspace a node, every one of them written -- larger than any case's)
DONORS = (("vsd", "off"), ("tsdf_extract", "tight"), ("mesh_select", "tight"), ("max_clique", "off"), ("tsdf_extract", "big"))
ARENA_BYTES = 16 << 20
ITEMS = [(name, shape) for name, c in CASES.items() for shape in c["shapes"]]


# ---------------------------------------------------------------------------------------------------------------------------------------
# the launches.  _build_<entry>(name, shape) moves the inputs to the device once and returns launch(ctx) -> the outputs
# ---------------------------------------------------------------------------------------------------------------------------------------
def _dev(a, dtype=None):
    import torch

    return None if a is None else torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).cuda()


class _Ctx:
    """what a launch needs to know of the run: the arena in use (None: the unpatched engine)"""

    def __init__(self, arena=None):
        self.arena = arena

    def raster_slot(self, db, n_views, h, w, slot=0):
        """the slot's workspace: a slice of exactly the reported size from the arena, or nothing (MeshDB allocates its own)"""
        from megapose6d_amd import _lib

        if self.arena is None:
            db._ws.pop(slot, None)
            return
        import torch

        need = int(_lib.load().mp_raster_workspace_bytes(db.handle, n_views, h, w))
        db._ws[slot] = self.arena.slice(need, torch.device("cuda", torch.cuda.current_device()))


def _mspd_case(shape):
    from support import vsd as vs

    return vs.mspd_case(1, 1, 1, seed=401) if shape == "one" else vs.mspd_case(3, 257, 5, seed=657, n_mesh=2, ragged=True)


def _build_pose_error(name, shape):
    from megapose6d_amd import engine as eng

    c = {k: _dev(v) for k, v in _mspd_case(shape).items()}
    if name == "pose_error_sym":
        return lambda ctx: eng.pose_error_sym(c["T_pred"], c["T_gt"], c["syms"], c["n_sym"], c["pts"], c["ids"], c["n_points"], with_diffs=True, with_alt=True)
    if name == "pose_error_mspd":
        return lambda ctx: eng.pose_error_mspd(c["T_pred"], c["T_gt"], c["syms"], c["n_sym"], c["pts"], c["K"], c["ids"], c["n_points"], with_alt=True)
    return lambda ctx: eng.pose_error_nn(c["T_pred"], c["T_gt"], c["pts"], c["ids"], c["n_points"])


def _build_vsd(name, shape):
    from megapose6d_amd import engine as eng
    from support import vsd as vs

    b, h, w, n_tau = (1, 1, 1, 10) if shape == "one" else (7, 37, 53, 16)
    c = {k: _dev(v) for k, v in vs.scene(1000 + b + h + n_tau, b, h, w).items()}
    taus = vs.taus_of(n_tau)
    return lambda ctx: eng.vsd(c["est"], c["gt"], c["test"], c["K"], c["diam"], taus=taus)


def _build_gt_info(name, shape):
    from megapose6d_amd import engine as eng
    from support import gt_info as gi

    b, h, w, canvas = (1, 1, 1, 1) if shape == "one" else (5, 33, 65, 3)
    c = gi.case(2000 + b + h + w, b, h, w, canvas)
    gt, test, K = _dev(c["gt"]), _dev(c["test"]), _dev(c["K"])
    return lambda ctx: eng.gt_info(gt, test, K, canvas=canvas, with_masks=True)


def _match_index(c, n_groups=None):
    from megapose6d_amd import engine as eng
    from megapose6d_amd import evaluation as ev

    index = ev.bop_match_index(c["pred_id"], c["gt_id"], c["group_id"], c["scores"], n_groups)
    on_dev = {k: _dev(index[k]) for k in eng.BOP_MATCH_INDEX}
    on_dev["n_taken_words"] = index["n_taken_words"]
    return index, on_dev


def _build_bop_match(name, shape):
    from megapose6d_amd import engine as eng
    from support import bop_match as bm

    # "off": two groups past the 64 ground truths of the fast path (65 and 133: the taken bits of the workspace, 3 and 5 words) among small ones
    c = bm.case(1, [(1, 1)], 1, 1, nan_share=0.0) if shape == "one" else bm.case(19, [(2, 3), (3, 65), (4, 2), (1, 133)], 12, 10, nan_share=0.01)
    index, on_dev = _match_index(c, c["thr"].shape[0])
    errs, thr, n_pred = _dev(np.ascontiguousarray(c["errs"][index["order"]], np.float32)), _dev(c["thr"]), len(c["scores"])
    return lambda ctx: eng.bop_match(errs, on_dev, thr, n_pred)


def _build_det_match(name, shape):
    from megapose6d_amd import engine as eng
    from support import det_ap as da

    c = da.case(1, [(1, 1)], nan_share=0.0) if shape == "one" else da.case(7, da.ragged_sizes(8, 65) + [(3, 70)])
    index, on_dev = _match_index(c)
    iou, ign, thr, n_pred = _dev(c["iou"][index["order"]]), _dev(c["gt_ignore"].astype(np.uint8)), _dev(da.IOU_THRS), len(c["scores"])
    return lambda ctx: eng.det_match(iou, on_dev, ign, thr, n_pred)


def _rle_masks(shape):
    from support import rle as rs

    if shape == "one":
        return rs.batch(("first_pixel",), 1, 1)
    if shape == "off":
        return rs.batch(rs.KINDS, 65, 257, seed=3)        # 10 masks; 257 columns = 17 units of 16, the last one partial
    return rs.blobs(32, 63, 65, seed=5)                   # 32 masks: mask_tot, the plan's last region, is exactly 256 bytes


def _build_rle_encode(name, shape):
    from megapose6d_amd import engine as eng

    masks = _dev(_rle_masks(shape))
    return lambda ctx: eng.rle_encode(masks)


def _build_rle_decode(name, shape):
    from megapose6d_amd import engine as eng
    from support import rle as rs

    masks = _rle_masks(shape)
    counts, offsets, _, _ = rs.restated_encode(masks)
    counts = _dev(counts)
    return lambda ctx: eng.rle_decode(counts, offsets, masks.shape[1], masks.shape[2])


def _build_tsdf_extract(name, shape):
    from megapose6d_amd import engine as eng
    from support import tsdf as st

    if shape == "one":
        vol, g = st.corner_volume()
    else:   # "off": 33 x 17 x 9 = 5049 nodes, 20 workgroups; "tight": 16 x 32 x 32 = 64 workgroups, block_nt ends on the last reported byte
        g = st.ODD_GRID if shape == "off" else st.Grid(st.ODD_GRID.origin, st.ODD_GRID.voxel, (16, 32, 32) if shape == "tight" else (96, 96, 64))
        vol = st.plane_volume(g)
    vol = _dev(vol)
    return lambda ctx: eng.tsdf_extract(vol, g.origin, g.voxel)


def _mesh(name, shape):
    from support import mesh_cleanup as sm

    if shape == "one":
        return sm.chain("forward", 1)                     # a single triangle
    if shape == "tight":
        # select: 262 144 faces = 64 workgroups of the rank pass, f.base is exactly 256 bytes.  cluster: 128 vertices, one in each of
        # 64 x 2 x 1 cells, every cell used: acc = 128 * 52 bytes = 26 * 256
        return sm.chain("forward", 262144 if name == "mesh_select" else 126)
    if name in ("mesh_select",):
        return sm.chain("reverse", 4097)                  # 4097 faces, 4099 vertices: a second, partial workgroup of the rank pass
    return sm.scene()                                     # 27 616 faces with two bad ones, loose vertices, permuted


def _build_mesh_components(name, shape):
    from megapose6d_amd import engine as eng

    m = _mesh(name, shape)
    V, faces = m.V, _dev(m["faces"])

    def launch(ctx):
        out = eng.mesh_components(V, faces)
        assert int(out[3][3]) == 0, "the union-find reached its cap: the labels are not specified"
        return out

    return launch


def _build_mesh_select(name, shape):
    from megapose6d_amd import engine as eng

    m = _mesh(name, shape)
    keep = np.zeros(m.F, np.uint8)
    keep[::3] = 200
    keep[:1] = 1
    v, f, k = _dev(m["vertices"]), _dev(m["faces"]), _dev(keep)
    return lambda ctx: eng.mesh_select(v, f, k)


def _cluster_grid(m, shape):
    from support import mesh_cleanup as sm

    if shape == "tight":
        return (-0.005, -0.005, -0.005), 0.01, (64, 2, 1)
    return sm.grid_of(m, 2.0, 0.37)


def _build_mesh_cluster(name, shape):
    from megapose6d_amd import engine as eng

    m = _mesh(name, shape)
    grid = _cluster_grid(m, shape)
    v, f, c = _dev(m["vertices"]), _dev(m["faces"]), _dev(m.get("colors"))
    if name == "mesh_cluster_count":
        return lambda ctx: eng.mesh_cluster_count(v, f, *grid)

    def launch(ctx):
        out = eng.mesh_cluster(v, f, *grid, colors=c)
        if shape == "tight":
            assert out[0].shape[0] == 128, "the tight shape needs every cell used: acc then ends on the last reported byte"
        return out

    return launch


def _build_model_info(name, shape):
    from megapose6d_amd import engine as eng
    from support import model_info as mi

    if shape == "one":
        points, n_points = mi.cases()["random_1"]["points"][None], np.asarray([1], np.int32)
    else:
        points, n_points = mi.three_objects()             # 300, 1025 and 65 points in rows of 1100
    points = _dev(points)
    return lambda ctx: eng.model_info(points, n_points)


def _build_symmetry_check(name, shape):
    from megapose6d_amd import engine as eng
    from megapose6d_amd import evaluation as ev
    from support import symmetry as sy

    if shape == "one":
        ms = sy.fixture_set(["tetrahedron"])
        backend = sy.EmulBackend()
        ev.find_symmetries(ms, rel_tol=sy.REL_TOL, n_samples=8, diameters=ms.diameters(), device="cpu", backend=backend)
        args = backend.calls[0]["args"]
    else:                                                 # the twelve fixtures in one call: 5 * 12 + 4 = 64 words of meta, exactly 256 bytes
        args = sy.found()[1].calls[0]["args"]
    v, f, t, R, c, vo, fo, to, co, tol = args
    d = lambda a: _dev(np.ascontiguousarray(a, np.float32))   # noqa: E731
    v, t, R, c = d(v), d(t), d(R).reshape(-1, 3, 3), d(c)
    f = np.asarray(f, np.int32)
    return lambda ctx: eng.symmetry_check(v, f, t, R, c, vo, fo, to, co, tol, mode=0)


def _build_surface_sample(name, shape):
    from megapose6d_amd import engine as eng
    from support import surface_sample as ss

    meshes, count = {"one": ([ss.soup(1)], 1), "off": ([ss.soup(257), ss.soup(65), ss.cube()], 65), "tight": ([ss.soup(64)], 64)}[shape]
    v, f, vo, fo = ss.pack(meshes)
    u = _dev(ss.uniforms((len(meshes), count), seed=11, edges=count > 1))
    v, f = _dev(v), _dev(f)
    return lambda ctx: eng.surface_sample(v, f, vo, fo, u)


def _build_farthest_point_sample(name, shape):
    import torch

    from megapose6d_amd import engine as eng
    from support import teaser as ts

    # the workspace holds the running minima of the points past the 16 384 a workgroup keeps in registers: only a longer row touches it
    counts = (1,) if shape == "one" else (1, 65, 257, ts.FPS_RESIDENT + 257)
    n_points = 1 if shape == "one" else 65
    clouds = (np.random.RandomState(0).uniform(-0.2, 0.2, size=(len(counts), max(counts), 3)) + [0, 0, 0.6]).astype(np.float32)
    clouds, counts = _dev(clouds), _dev(counts, torch.int32)
    return lambda ctx: eng.farthest_point_sample(clouds, counts, n_points)


def _build_max_clique(name, shape):
    import torch

    from megapose6d_amd import engine as eng
    from support import teaser_clique as tc

    if shape == "one":
        a, counts = np.zeros((1, 1, 1), np.uint8), np.asarray([1], np.int32)
    else:
        a, counts = tc.stride70_rows()                    # rows of 1 .. 70 vertices around the word and the wave edges
    a, counts = _dev(a), _dev(counts, torch.int32)
    return lambda ctx: eng.max_clique(a, counts, tc.FULL_BUDGET)


def _build_teaser_solve(name, shape):
    import torch

    from megapose6d_amd import engine as eng
    from support import teaser as ts
    from support import teaser_clique as tc

    selection = name.split("/")[1]
    if shape == "one":
        src, dst = (a[None, :1] for a in ts.correspondences(*ts.SOLVE_CASES[0])[:2])
        S, D, counts, min_inliers = np.ascontiguousarray(src), np.ascontiguousarray(dst), [1], 0
    else:                                                 # the rows of test_solve_matches_the_emulation: 50 .. 200 correspondences, a row of two
        cases = ts.SOLVE_CASES + ((2, 0.0, 7),)
        S, D, counts, min_inliers = np.zeros((len(cases), 200, 3), np.float32), np.zeros((len(cases), 200, 3), np.float32), [], 25
        for r, case in enumerate(cases):
            src, dst = ts.correspondences(*case)[:2]
            S[r, : len(src)], D[r, : len(src)] = src, dst
            counts.append(len(src))
    S, D, counts = _dev(S), _dev(D), _dev(counts, torch.int32)
    steps = tc.FULL_BUDGET if selection == "max_clique" else None

    def launch(ctx):
        Rt, retval, tel = eng.teaser_solve(S, D, counts, ts.NOISE_BOUND, min_inliers, selection, "chain", telemetry=True, max_clique_steps=steps)
        return Rt, retval, tel

    return launch


def _build_teaser_refine(name, shape):
    import torch

    from megapose6d_amd import engine as eng
    from support import teaser as ts
    from support import teaser_clique as tc

    selection = name.split("/")[1]
    if shape == "one":
        frames, kw = (2, 2, (1,), ("",), 1), dict(n_min_points=1, n_points=1, min_num_inliers=0)
    else:                                                 # 24 x 32, five rows with masks of 1, 63, 64, 65 and 0 pixels, n_points 64
        frames, kw = ts.FRAME_CASES["tiny"]
    meas, im_ids, rend, K, TCO = ts.frame_case(*frames)
    meas, im_ids, rend, K, TCO = _dev(meas), _dev(im_ids, torch.int32), _dev(rend), _dev(K), _dev(TCO)
    steps = tc.FULL_BUDGET if selection == "max_clique" else None
    return lambda ctx: eng.teaser_refine(meas, im_ids, rend, K, TCO, noise_bound=ts.NOISE_BOUND, telemetry=True, inlier_selection=selection,
                                         max_clique_steps=steps, **kw)


@functools.lru_cache(None)
def _raster_db(mesh):
    """one database per mesh for the whole module: a launch and the larger one before it share the database and its slot"""
    from megapose6d_amd import engine as eng
    from support import raster_limits as rl

    return eng.MeshDB([rl.pyramid_mesh() if mesh == "pyramid" else rl.layered_grid(**rl.CASE_A)])


@functools.lru_cache(None)
def _raster_launch(launch_name, with_flags):
    """a launch of RASTER_LAUNCHES -> launch(ctx): fp32 [n_items,h,w,32], rgb normals depth of view r at channels 7 r .. 7 r + 6; with_flags:
    also the job flags raster_job_flags hands out for it"""
    import torch

    from megapose6d_amd import engine as eng
    from support import raster_limits as rl

    mesh, views, vpi, h, w = RASTER_LAUNCHES[launch_name]
    db = _raster_db(mesh)
    near, far = (rl.Z_NEAR_VIEW, rl.Z_FAR_VIEW) if mesh == "A" else (0.4, 1.2)
    T = np.stack([rl.pose_z(near if v == "N" else far) for v in views])
    for i, v in enumerate(views):
        if v == "E":
            T[i, 0, 3] = np.nan
    n, Cp = len(views), 32
    K = np.repeat(np.array([[300.0, 0, w / 2], [0, 300.0, h / 2], [0, 0, 1]], np.float32)[None], n, 0)
    T, K, ids = _dev(T), _dev(K), torch.zeros(n, dtype=torch.int32, device="cuda")
    n_items, n_tiles = n // vpi, -(-h // 8) * -(-w // 8)

    def launch(ctx):
        ctx.raster_slot(db, n, h, w)
        out = torch.full((n_items, h, w, Cp), -123.0, device="cuda")
        eng.raster_render(db, ids, T, K, h, w, 3, eng.make_lights(), out, h * w * Cp, w * Cp, Cp, 0, 3, 6, views_per_item=vpi, stride_view=7)
        if not with_flags:
            return [out]
        ws = db.workspace(n, h, w, out.device)
        addr = eng.raster_job_flags(db, n, h, w, out.device)
        assert addr != 0, "the launch left no job flags"
        off = addr - ws.data_ptr()
        assert 0 < off and off + n_items * n_tiles <= ws.numel()
        # "one byte per (item, 8x8-pixel tile)" (engine.raster_job_flags): the padding of the region up to a multiple of 16 is no pair's
        return [out, ws[off:off + n_items * n_tiles].clone()]

    return launch


def _build_raster_render(name, shape):
    return _raster_launch(CASES[name]["launches"][shape], CASES[name].get("reads") == "raster_job_flags")


def _build_raster_render_scene(name, shape):
    import torch

    from megapose6d_amd import engine as eng
    from support import raster_limits as rl

    if shape == "one":
        meshes, obj_off, mesh_ids, T, h, w = [rl.pyramid_mesh()], [0, 1], [0], rl.pose_z(0.4)[None], 8, 8
        K, radius = np.array([[[300.0, 0, 4], [0, 300.0, 4], [0, 0, 1]]], np.float32), np.array([0.2], np.float32)
    else:                                                 # two cameras, four objects, two of them overflowing their lists
        meshes, obj_off, mesh_ids, T, K, radius = rl.overflow_scene()
        h, w = rl.H, rl.W
    db = eng.MeshDB(meshes)
    dev = torch.device("cuda")
    lights = eng.lights_array([eng.make_lights() for _ in mesh_ids], dev)
    mesh_ids, T, K, radius = _dev(mesh_ids, torch.int32), _dev(np.asarray(T, np.float32)), _dev(K), _dev(radius)
    n_cams = len(obj_off) - 1

    def launch(ctx):
        out = torch.full((n_cams, h, w, 8), -123.0, device=dev)
        inst = torch.full((n_cams, h, w), -7, dtype=torch.int32, device=dev)
        eng.raster_render_scene(db, obj_off, mesh_ids, T, K, radius, lights, h, w, 3, out, h * w * 8, w * 8, 8, 0, 3, 6, inst)
        return [out, inst]

    return launch


_BUILDERS = {"pose_error_sym": _build_pose_error, "pose_error_mspd": _build_pose_error, "pose_error_nn": _build_pose_error, "vsd": _build_vsd,
             "gt_info": _build_gt_info, "bop_match": _build_bop_match, "det_match": _build_det_match, "rle_encode": _build_rle_encode,
             "rle_decode": _build_rle_decode, "tsdf_extract": _build_tsdf_extract, "mesh_components": _build_mesh_components,
             "mesh_select": _build_mesh_select, "mesh_cluster_count": _build_mesh_cluster, "mesh_cluster": _build_mesh_cluster,
             "model_info": _build_model_info, "symmetry_check": _build_symmetry_check, "surface_sample": _build_surface_sample,
             "farthest_point_sample": _build_farthest_point_sample, "max_clique": _build_max_clique, "teaser_solve": _build_teaser_solve,
             "teaser_refine": _build_teaser_refine, "raster_render": _build_raster_render, "raster_render_scene": _build_raster_render_scene}


@functools.lru_cache(None)
def _launch_of(name, shape):
    return _BUILDERS[CASES[name]["entry"]](name, shape)


# ---------------------------------------------------------------------------------------------------------------------------------------
# the runs
# ---------------------------------------------------------------------------------------------------------------------------------------
def _flat(out):
    """the outputs of a launch as a list of host arrays (dicts by key; host ints as arrays; an absent optional output stays None)"""
    import torch

    if isinstance(out, dict):
        return [a for k in sorted(out) for a in _flat(out[k])]
    if isinstance(out, (tuple, list)):
        return [a for o in out for a in _flat(o)]
    if isinstance(out, torch.Tensor):
        return [out.detach().cpu().numpy()]
    return [None if out is None else np.asarray(out)]


def _same_bits(got, want, what):
    assert len(got) == len(want), (what, len(got), len(want))
    for i, (a, b) in enumerate(zip(got, want)):
        if a is None or b is None:
            assert a is None and b is None, (what, i)
            continue
        assert a.shape == b.shape and a.dtype == b.dtype, (what, i, a.shape, b.shape, a.dtype, b.dtype)
        if a.tobytes() != b.tobytes():
            differ = np.flatnonzero(np.ascontiguousarray(a).view(np.uint8).reshape(-1) != np.ascontiguousarray(b).view(np.uint8).reshape(-1))
            raise AssertionError(f"{what}: output {i} ({a.dtype} {a.shape}) differs from the fresh-allocation run in {differ.size} bytes, the first at byte "
                                 f"{int(differ[0])} (element {int(differ[0]) // a.itemsize})")


_faulted = []          # a device fault poisons the process: nothing more is started on the card after one
_donor_bytes = {}      # donor -> the bytes it took, once it has run: a donor known to be too small is not run again


@pytest.fixture(scope="module")
def arena():
    import torch

    from support.workspace_arena import WorkspaceArena

    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return WorkspaceArena(ARENA_BYTES, torch.device("cuda", torch.cuda.current_device()))


def _run(launch, arena, what):
    import torch

    out = launch(_Ctx(arena))
    torch.cuda.synchronize()
    assert arena is None or arena.handouts, (what, "the launch took no workspace from the arena")
    if arena is not None:
        arena.check()
    return _flat(out)


def _taken(arena):
    return sum(n for _, n in arena.handouts)


def _leave_state_of_another(name, shape, own_bytes, arena):
    """run E's first half: another launch in the arena's bytes -> what ran"""
    after = CASES[name].get("after")
    if after is not None:                                  # the rasteriser: the larger launch on the same database and slot
        before = after[shape]
        _run(_raster_launch(before, False), arena, ("before E", before))
        assert _taken(arena) > own_bytes, (before, "is not the larger launch", _taken(arena), own_bytes)
        return before
    for donor in DONORS:
        if CASES[donor[0]]["entry"] == CASES[name]["entry"] or _donor_bytes.get(donor, own_bytes) < own_bytes:
            continue
        arena.reset()
        _run(_launch_of(*donor), arena, ("before E", donor))
        _donor_bytes[donor] = _taken(arena)
        if _taken(arena) >= own_bytes:
            return donor
    raise AssertionError(f"no donor launch with a workspace of {own_bytes} bytes or more: add one to DONORS")


@pytest.mark.parametrize("name,shape", ITEMS, ids=[f"{n}:{s}" for n, s in ITEMS])
def test_entry_on_dirty_workspace_between_canaries(name, shape, arena, monkeypatch):
    from megapose6d_amd import engine as eng

    if _faulted:
        pytest.fail(f"not run: the device faulted in {_faulted[0]}")
    try:
        launch = _launch_of(name, shape)
        want = _run(launch, None, "want")
        assert any(a is not None and a.size for a in want), "the launch has no output to compare"
        monkeypatch.setattr(eng, "_workspace", arena.workspace)
        runs = {}
        for state, prepare in (("A", lambda: arena.fill(0x00)), ("B", lambda: arena.fill(0xFF)), ("C", lambda: arena.fill_random(20240611)),
                               ("D", arena.keep)):
            arena.reset()
            prepare()
            runs[state] = _run(launch, arena, state)
        own_bytes = _taken(arena)
        arena.reset()
        before = _leave_state_of_another(name, shape, own_bytes, arena)
        arena.keep()
        runs["E"] = _run(launch, arena, ("E", before))
        assert _taken(arena) == own_bytes
        for state, got in runs.items():
            _same_bits(got, want, (name, shape, state) + ((before,) if state == "E" else ()))
    except RuntimeError as e:
        if any(word in str(e).lower() for word in ("hip error", "illegal memory", "cuda error", "device-side")):
            _faulted.append(f"{name}:{shape}")
        raise
