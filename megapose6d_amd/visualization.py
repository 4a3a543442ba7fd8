"""Prediction overlays on the device: the estimate drawn on the image (mp_overlay / mp_draw_boxes, csrc/overlay.hip).

What the reference's inference script draws in `--vis-detections` and `--vis-outputs` (scripts/run_inference_on_example.py:94-106,
:151-194) without OpenCV, bokeh or seaborn:

  - `make_contour_overlay` has the signature of visualization/utils.py:56-85: a mask from the render (get_mask_from_rgb), its Canny
    edges, `dilate_iterations` rounds of a 3x3 dilation, painted on the image.  `megapose.visualization.utils.make_contour_overlay =
    megapose6d_amd.visualization.make_contour_overlay` swaps it in.
  - `make_mesh_overlay` is the image BokehPlotter.plot_overlay (visualization/bokeh_plotter.py:106-130) hands to plot_image.
  - `overlay_scenes` is the batched form on a `SceneRenderOutput`: the renderer's instance map gives every object its own
    occlusion-aware contour in its own colour, which the reference (one green contour for the union of all objects) cannot draw.
  - `draw_detections` draws box frames (plot_detections / draw_bounding_box).  No text labels are drawn: there is no font rasteriser.
  - `make_output_visualization` / `save_visualizations` produce and write the pictures of `--vis-outputs`.

Unpinned third parties: cv2.Canny, cv2.dilate and cv2.rectangle are restated in csrc/overlay_core.h (the box frame rule is this
project's: inside the box grown by t / 2, outside the box shrunk by (t + 1) / 2); DEFAULT_PALETTE holds the ten colours the reference's seaborn call returns when no
theme is set (matplotlib's "tab10").
"""
from __future__ import annotations

from pathlib import Path
from typing import Any, Dict, List, Optional, Tuple, Union

import numpy as np
import torch

from . import engine as eng
from .types import Panda3dLightData

# The reference's plotter cycles `sns.color_palette(n_colors=40)` (bokeh_plotter.py:57-62) and never sets a seaborn theme; without one that
# call returns matplotlib's active colour cycle, whose default is the ten "tab10" colours below.  seaborn is absent, so this is unpinned:
# under `sns.set_theme()` the reference would draw seaborn's "deep" palette instead.
DEFAULT_PALETTE: Tuple[Tuple[int, int, int], ...] = (
    (31, 119, 180), (255, 127, 14), (44, 160, 44), (214, 39, 40), (148, 103, 189),
    (140, 86, 75), (227, 119, 194), (127, 127, 127), (188, 189, 34), (23, 190, 207))

# file names of scripts/run_inference_on_example.py:102, :190-192
VISUALIZATION_FILES = {"detections": "detections.png", "mesh_overlay": "mesh_overlay.png", "contour_overlay": "contour_overlay.png",
                       "all_results": "all_results.png"}


def _device_images(a: Union[np.ndarray, torch.Tensor], name: str) -> torch.Tensor:
    """uint8 [h,w,3] or [n,h,w,3], numpy or tensor -> a contiguous uint8 [n,h,w,3] tensor on the GPU"""
    t = torch.as_tensor(a)
    if t.dtype != torch.uint8 or t.dim() not in (3, 4) or t.shape[-1] != 3:
        raise ValueError(f"{name} must be uint8 [h,w,3] or [n,h,w,3], got {t.dtype} {tuple(t.shape)}")
    if t.dim() == 3:
        t = t[None]
    return t.cuda().contiguous()


def make_contour_overlay(img: np.ndarray, render: np.ndarray, color: Optional[Tuple[int, int, int]] = None,
                         dilate_iterations: int = 1) -> Dict[str, Any]:
    """The reference's make_contour_overlay: img, render uint8 [h,w,3] numpy -> {"img": the image with the contour of the render's mask
    painted in `color` (default green), "mask": bool [h,w] (any channel of the render > 0), "canny": uint8 [h,w], 0 or 255}."""
    green = (0, 255, 0)
    out = eng.overlay(_device_images(img, "img"), render=_device_images(render, "render"), colors=[tuple(int(c) for c in (green if color is None else color))],
                      dilate_iterations=dilate_iterations, outputs=("contour", "canny", "mask"))
    return {"img": out["contour"][0].cpu().numpy(), "mask": out["mask"][0].cpu().numpy() > 0, "canny": out["canny"][0].cpu().numpy()}


def make_mesh_overlay(rgb_input: np.ndarray, rgb_rendered: np.ndarray) -> np.ndarray:
    """The image BokehPlotter.plot_overlay plots: render * 0.8 + 255 * 0.2 where any channel of the render is > 0, else
    image * 0.6 + 255 * 0.4, evaluated as numpy does (float64, rounded to float32, truncated) -> uint8 [h,w,3]."""
    out = eng.overlay(_device_images(rgb_input, "rgb_input"), render=_device_images(rgb_rendered, "rgb_rendered"), outputs=("mesh",))
    return out["mesh"][0].cpu().numpy()


def render_to_uint8(rgbs: torch.Tensor) -> torch.Tensor:
    """float renders [n,3,h,w] in [0,1] -> uint8 [n,h,w,3], with the rounding of Panda3dSceneRenderer.render_scene"""
    return torch.round(rgbs * 255).to(torch.uint8).permute(0, 2, 3, 1).contiguous()


def overlay_scenes(images: Union[np.ndarray, torch.Tensor], scene_output, colors=None, dilate_iterations: int = 1) -> Dict[str, torch.Tensor]:
    """Batched overlays of Panda3dSceneRenderer.render_scenes' output on the observed images uint8 [n,h,w,3]: the instance map is the
    label map, so every object has its own contour, cut where another object occludes it, in colour `colors[instance mod n_colors]`
    (default DEFAULT_PALETTE) -> device tensors "contour", "mesh" [n,h,w,3], "canny", "mask" [n,h,w], uint8.  The blend takes the
    render wherever an instance owns the pixel (also where it rendered black, which the reference's mask would miss)."""
    if scene_output.instance_ids is None:
        raise ValueError("overlay_scenes needs the instance map: render_scenes(..., with_instance_ids=True)")
    return eng.overlay(_device_images(images, "images"), render=render_to_uint8(scene_output.rgbs), labels=scene_output.instance_ids,
                       colors=DEFAULT_PALETTE if colors is None else colors, dilate_iterations=dilate_iterations)


def draw_detections(images: Union[np.ndarray, torch.Tensor], detections, colors=None, thickness: int = 2):
    """Box frames of a detections collection (tensor `bboxes` [n_det,4], column `batch_im_id`) on images uint8 [n,h,w,3] (or one
    [h,w,3]); colors default to red, the reference's; detection j takes colour j mod n_colors.  No text labels are drawn (there is no
    font rasteriser).  Returns what it was given: numpy for numpy, a device tensor for a tensor."""
    t = _device_images(images, "images")
    ids = torch.as_tensor(np.asarray(detections.infos["batch_im_id"], np.int32))
    out = eng.draw_boxes(t, detections.bboxes.to(t.device).float(), ids.to(t.device), colors=((255, 0, 0),) if colors is None else colors,
                         thickness=thickness)
    single = torch.as_tensor(images).dim() == 3
    out = out[0] if single else out
    return out.cpu().numpy() if isinstance(images, np.ndarray) else out


def make_output_visualization(rgb: np.ndarray, labels: List[str], TCO, K, scene_renderer, per_instance: bool = False) -> Dict[str, np.ndarray]:
    """The pictures of the reference's `--vis-outputs` for one image: the objects `labels` at camera-from-object poses TCO [n,4,4] are
    rendered by `scene_renderer` (a Panda3dSceneRenderer) with camera matrix K [3,3] at rgb's resolution under the script's white ambient
    light, and laid over rgb uint8 [h,w,3].  per_instance=False gives the reference's picture (one mask from the render, in green);
    True gives each object its own contour in its own colour.  -> "rgb", "contour_overlay", "mesh_overlay" [h,w,3] and "all_results"
    [h,3w,3] (the three side by side, as the reference's grid), uint8 numpy."""
    rgb = np.ascontiguousarray(rgb)
    h, w = rgb.shape[:2]
    n = len(labels)
    light_datas = [Panda3dLightData(light_type="ambient", color=(1.0, 1.0, 1.0, 1))]
    K_rows = torch.as_tensor(np.asarray(K, np.float64).reshape(1, 3, 3)).repeat(n, 1, 1)
    r = scene_renderer.render_scenes(labels, torch.as_tensor(TCO), K_rows, [0] * n, (h, w), light_datas, with_instance_ids=per_instance)
    if per_instance:
        out = overlay_scenes(rgb, r)
    else:
        out = eng.overlay(_device_images(rgb, "rgb"), render=render_to_uint8(r.rgbs), colors=((0, 255, 0),), outputs=("contour", "mesh"))
    contour, mesh = out["contour"][0].cpu().numpy(), out["mesh"][0].cpu().numpy()
    return {"rgb": rgb, "contour_overlay": contour, "mesh_overlay": mesh, "all_results": np.concatenate([rgb, contour, mesh], axis=1)}


def save_visualizations(vis_dir, images: Dict[str, np.ndarray]) -> List[Path]:
    """Write the entries of `images` the reference's script writes ("detections", "mesh_overlay", "contour_overlay", "all_results") as
    PNG files under its file names into vis_dir (created if missing) -> the paths written."""
    from PIL import Image

    vis_dir = Path(vis_dir)
    vis_dir.mkdir(parents=True, exist_ok=True)
    written = []
    for key, name in VISUALIZATION_FILES.items():
        if key in images:
            Image.fromarray(np.ascontiguousarray(images[key], np.uint8)).save(vis_dir / name)
            written.append(vis_dir / name)
    return written
